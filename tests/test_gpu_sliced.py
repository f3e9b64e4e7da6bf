"""GPU: rf_sliced_wasserstein (include/rfops.h) against sw_ref, the float64 restatement of the contract
(tests/test_sliced_host.py).

Inputs whose projections are EXACT in fp32 make the reference unambiguous: coordinates multiples of 2^-10 in [-0.5, 0.5)
and direction components multiples of 2^-8 in [-1, 1] give products that are multiples of 2^-18 below 1.5 -- 20 bits, exact
in any order, fused or not.  On those the bars are
    loss       |got - ref| <= 2^-23 ref              one final rounding (2^-24) with a factor 2 of margin; the double sums
                                                     contribute far below 2^-40
    gradients  |got - ref| <= 2^-23 |ref| + 1e-12    the absolute term covers cancellation in double at unit scale
On general floats only the loss is compared (a near-tie legitimately swaps partners, and with them the gradients), at
    |got - ref| <= 4 eps sqrt(ref) + 4 eps^2 + 2^-23 ref,   eps = 3 * 2^-24 * max(|x| + |y| + |z|) * max|dir|
eps bounds the fp32 projection's error (three roundings of terms below max(|x|+|y|+|z|) max|dir|); sorting is 1-Lipschitz
in the sup norm, so every sorted value moves by at most eps, every difference by 2 eps, and by Cauchy-Schwarz the weighted
mean of squares by at most 2 (2 eps) sqrt(ref) + (2 eps)^2."""
import numpy as np
import pytest
import torch

from test_sliced_host import exact_inputs, sw_ref

pytestmark = pytest.mark.gpu

CHUNK = 16  # _raw.SW_DIR_CHUNK (asserted below)
REL = 2.0 ** -23


def run(a, c, d, l1=None, l2=None, grad=True):
    from rfnet_amd import _raw
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).cuda()  # noqa: E731
    out = _raw.sliced_wasserstein(t(a), t(c), t(d), t(None if l1 is None else np.asarray(l1, np.int32)),
                                  t(None if l2 is None else np.asarray(l2, np.int32)), want_grad=grad)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out] if grad else out.cpu().numpy()


def ref(a, c, d, l1=None, l2=None):
    b = a.shape[0]
    loss, g1, g2 = np.zeros(b), np.zeros(a.shape), np.zeros(c.shape)
    for i in range(b):
        loss[i], g1[i], g2[i] = sw_ref(a[i], c[i], d, None if l1 is None else l1[i], None if l2 is None else l2[i])
    return loss, g1, g2


def check(got, exp, what=""):
    (loss, g1, g2), (el, e1, e2) = got, exp
    for i in range(len(el)):
        print(f"{what} sample {i}: loss {loss[i]!r} ref {el[i]!r} rel err {abs(loss[i] - el[i]) / max(el[i], 1e-300):.3e}")
    assert (np.abs(loss - el) <= REL * el).all(), (what, loss, el)
    for k, g, e in (("grad1", g1, e1), ("grad2", g2, e2)):
        err = np.abs(g - e)
        print(f"{what} {k}: max abs err {err.max():.3e}, max |ref| {np.abs(e).max():.3e}")
        assert (err <= REL * np.abs(e) + 1e-12).all(), (what, k, float(err.max()))


def zero_behind(g1, g2, l1, l2):
    for i in range(g1.shape[0]):
        assert not g1[i, l1[i]:].view(np.uint32).any() and not g2[i, l2[i]:].view(np.uint32).any(), i  # exactly +0


# ---- 1. ragged counts over hostile padding, below a chunk and across three -------------------------------------------------
LEN1 = np.array([300, 1, 257], np.int32)  # the full size, 1, and the coprime pair (257, 199)
LEN2 = np.array([129, 200, 199], np.int32)
_RAGGED = {}


def ragged(nproj):
    if nproj not in _RAGGED:
        a, c, d = exact_inputs(5, 3, 300, 200, nproj)
        exp = ref(a, c, d, LEN1, LEN2)
        for i in range(3):  # padding: NaN in one cloud, copies of valid points of the partner cloud in the other
            a[i, LEN1[i]:] = np.nan
            c[i, LEN2[i]:] = a[i, np.arange(200 - LEN2[i]) % LEN1[i]]
        _RAGGED[nproj] = (a, c, d, exp)
    return _RAGGED[nproj]


@pytest.mark.parametrize("nproj", [1, 7, 2 * CHUNK + 3])
def test_ragged_counts(nproj):
    from rfnet_amd import _raw
    assert _raw.SW_DIR_CHUNK == CHUNK
    a, c, d, exp = ragged(nproj)
    got = run(a, c, d, LEN1, LEN2)
    check(got, exp, f"ragged nproj={nproj}")
    zero_behind(got[1], got[2], LEN1, LEN2)
    # the loss-only form returns the same bits
    assert run(a, c, d, LEN1, LEN2, grad=False).tobytes() == got[0].tobytes()


def test_full_counts_are_the_default():
    a, c, d = exact_inputs(6, 2, 300, 200, 5)
    got = run(a, c, d)
    check(got, ref(a, c, d), "n != m, no counts")
    full = run(a, c, d, [300, 300], [200, 200])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, full))


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index():
    """A coarse grid (coordinates k / 32, directions k / 4) with duplicated points: most projections are tied, and the
    tie rule alone fixes which point gets which gradient."""
    a, c, d = exact_inputs(9, 2, 300, 300, 6, cgrid=32, dgrid=4)
    a[:, 200:] = a[:, :100]
    c[:, 250:] = a[:, 50:100]
    d[0] = (1.0, 0.0, 0.0)
    p = a[0].astype(np.float64) @ d[1].astype(np.float64)
    tied = len(p) - len(np.unique(p))
    assert tied >= 150, tied
    check(run(a, c, d), ref(a, c, d), "ties")
    l1, l2 = [211, 300], [300, 177]
    check(run(a, c, d, l1, l2), ref(a, c, d, l1, l2), "ties, ragged")


# ---- 3. - 5. sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b, n, m, nproj", [(2, 1, 1, 3), (2, 64, 65, 4), (2, 65, 1, 2), (1, 1025, 130, CHUNK + 1),
                                            (1, 4097, 2049, 2), (1, 8193, 4096, 2)])  # sorts of 8192 and 4096, of 16384 and 4096 words
def test_small_and_odd_sizes(b, n, m, nproj):
    a, c, d = exact_inputs(n * 7 + m, b, n, m, nproj)
    check(run(a, c, d), ref(a, c, d), f"{n} x {m}")


def test_lds_capacity():
    """n = 16384: the 128 KiB of words, every stage of the network; m = 16383: a padded word, and no rank has one partner."""
    a, c, d = exact_inputs(21, 1, 16384, 16383, 2)
    check(run(a, c, d), ref(a, c, d), "16384 x 16383")


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------
def test_bits():
    a, c, d, _ = ragged(2 * CHUNK + 3)
    one = run(a, c, d, LEN1, LEN2)
    two = run(a, c, d, LEN1, LEN2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two)), "two calls differ"
    part = run(a[1:3], c[1:3], d, LEN1[1:3], LEN2[1:3])
    assert all(x[1:3].tobytes() == y.tobytes() for x, y in zip(one, part)), "a sample depends on its batch"
    # a neighbour with NaN / inf in VALID rows: RF_OK (run raises otherwise), and the other samples keep their bits
    a2, c2 = a.copy(), c.copy()
    a2[0, 3], a2[0, 100, 1], c2[0, 7, 2], c2[0, 50] = np.nan, np.inf, -np.inf, np.nan
    bad = run(a2, c2, d, LEN1, LEN2)
    assert all(x[1:3].tobytes() == y[1:3].tobytes() for x, y in zip(one, bad)), "a non-finite neighbour changed a sample"
    zero_behind(bad[1], bad[2], LEN1, LEN2)


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------
def test_graph_capture_with_device_counts():
    """No host synchronisation anywhere: the call is captured with device counts, and a replay returns the eager bits --
    also after the counts changed in place."""
    from rfnet_amd import _raw
    a, c, d, _ = ragged(2 * CHUNK + 3)
    a, c = np.nan_to_num(a, nan=0.25), c.copy()  # (other counts below make padded rows valid)
    ta, tc, td = (torch.from_numpy(x).cuda() for x in (a, c, d))
    l1, l2 = torch.from_numpy(LEN1).cuda(), torch.from_numpy(LEN2).cuda()
    call = lambda: _raw.sliced_wasserstein(ta, tc, td, l1, l2, want_grad=True)  # noqa: E731
    eager = [t.clone() for t in call()]
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, eager))
    l1.copy_(torch.tensor([7, 300, 64], dtype=torch.int32))
    l2.copy_(torch.tensor([200, 3, 65], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    again = call()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, again))
    assert not torch.equal(out[0], eager[0])


# ---- 8. glue ------------------------------------------------------------------------------------------------------------------
def test_glue_backward_with_a_non_uniform_grad_output():
    from rfnet_amd import glue
    a, c, d, (el, e1, e2) = ragged(7)
    ta, tc = torch.from_numpy(a).cuda().requires_grad_(), torch.from_numpy(c).cuda().requires_grad_()
    loss = glue.sliced_wasserstein(ta, tc, directions=torch.from_numpy(d).cuda(), lengths1=LEN1, lengths2=LEN2)
    assert loss.shape == (3,)
    w = np.array([0.5, -2.0, 4.0])
    (loss * torch.from_numpy(w).cuda().float()).sum().backward()
    check((loss.detach().cpu().numpy(), ta.grad.cpu().numpy() / w[:, None, None], tc.grad.cpu().numpy() / w[:, None, None]),
          (el, e1, e2), "glue")  # (the weights are powers of two: the products are exact)
    # only one side requires grad; and none
    tb = torch.from_numpy(c).cuda()
    one = glue.sliced_wasserstein(ta, tb, directions=torch.from_numpy(d).cuda(), lengths1=LEN1, lengths2=LEN2)
    assert torch.equal(one, loss) and one.requires_grad
    none = glue.sliced_wasserstein(ta.detach(), tb, directions=torch.from_numpy(d).cuda(), lengths1=LEN1, lengths2=LEN2)
    assert torch.equal(none, loss.detach()) and not none.requires_grad


def test_glue_draws_directions_on_the_device():
    from rfnet_amd import glue
    a, c, _ = exact_inputs(31, 2, 130, 97, 1)
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    glue.sliced_wasserstein(ta, tc, nproj=20, generator=gen)  # (first use: library load, workspace)
    gen.manual_seed(1234)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = glue.sliced_wasserstein(ta, tc, nproj=20, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    gen.manual_seed(1234)
    two = glue.sliced_wasserstein(ta, tc, nproj=20, generator=gen)
    assert torch.equal(one, two) and one.shape == (2,)
    # the same directions, drawn here: unit vectors from the same generator state
    gen.manual_seed(1234)
    d = torch.randn(20, 3, device="cuda", generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    assert torch.equal(glue.sliced_wasserstein(ta, tc, directions=d), one)
    assert not torch.equal(glue.sliced_wasserstein(ta, tc, nproj=20, generator=gen), one)  # the state moved on


def test_numpy_inputs_round_trip():
    from rfnet_amd import _raw
    a, c, d = exact_inputs(33, 2, 70, 90, 3)
    loss, g1, g2 = _raw.sliced_wasserstein(a, c, d, lengths1=[70, 9], lengths2=[1, 90], want_grad=True)
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in (loss, g1, g2))
    check((loss, g1, g2), ref(a, c, d, [70, 9], [1, 90]), "numpy")
    assert isinstance(_raw.sliced_wasserstein(a, c, d), np.ndarray)
    cpu = _raw.sliced_wasserstein(torch.from_numpy(a), torch.from_numpy(c), torch.from_numpy(d))
    assert isinstance(cpu, torch.Tensor) and not cpu.is_cuda and cpu.numpy().tobytes() == _raw.sliced_wasserstein(a, c, d).tobytes()


# ---- general floats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b, n, m, nproj", [(2, 1000, 1000, 24), (2, 777, 2048, 9)])
def test_general_floats_loss(b, n, m, nproj):
    rng = np.random.RandomState(n + m)
    a, c = rng.rand(b, n, 3).astype(np.float32), (rng.rand(b, m, 3) * 0.9).astype(np.float32)
    d = rng.randn(nproj, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    got = run(a, c, d, grad=False)
    exp = ref(a, c, d)[0]
    eps = 3 * 2.0 ** -24 * max(np.abs(a).sum(-1).max(), np.abs(c).sum(-1).max()) * np.abs(d).max()
    for i in range(b):
        bar = 4 * eps * np.sqrt(exp[i]) + 4 * eps * eps + REL * exp[i]
        print(f"general {n} x {m} sample {i}: loss {got[i]!r} ref {exp[i]!r} err {abs(got[i] - exp[i]):.3e} bar {bar:.3e}")
        assert abs(got[i] - exp[i]) <= bar
