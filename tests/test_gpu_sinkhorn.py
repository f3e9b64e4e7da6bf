"""GPU: rf_sinkhorn (include/rfops.h) against sk_ref, the numpy restatement of the contract
(tests/test_sinkhorn_host.py).

The bar comes from the reference alone.  For every case (three samples) and every quantity q of (loss, pot, delta, grad1,
grad2), E32(q) is the largest error over the case's samples of sk_ref run in float32 against sk_ref in float64 on the same
inputs: what the number formats cost a straightforward implementation.  The GPU may differ from float64 by
    |got - ref64| <= K * E32(q) + 4 * 2^-23 * mag(q)
with mag the largest |entry| of the float64 quantity (delta is a difference of potentials: its magnitude is theirs).  K
covers v_exp_f32 / v_log_f32 / v_sqrt_f32 / v_rcp_f32 against libm and the tiled summation order.  The case takes the
largest E32 of its three samples because a scalar such as the loss can come out of float32 almost exact by luck.

Measured on the MI355X, the largest |got - ref64| / E32 over all cases below, counted where the error is above the 4-ulp
term (below it that term alone carries the comparison, and E32 can be anything: at 1 x 1 the float32 delta is exact):
    pot 2.45 (257 x 130, p = 2, blur 0.05)    grad1 1.39 (300 x 1000, p = 2, blur 0.05)    grad2 2.64 (257 x 1025, p = 2,
    blur 0.05)    loss and delta: never above the 4-ulp term    stabilisation case: gradients 0.03, the rest below the term
K is the next power of two above twice the largest, 2 * 2.64: 8.  Without that filter the largest ratio is the loss's, 18.6
(257 x 1025, p = 1, blur 0.01): an error of 7e-9 on a loss of 0.1, which is the rounding of the fp32 output itself (half an
ulp is 3.7e-9) against a reference whose float32 form adds its loss in float64 and so has E32 = 4e-10.
"""
import numpy as np
import pytest
import torch

from test_sinkhorn_host import STAB_EPS, clouds, schedule, sk_ref, stab_clouds

pytestmark = pytest.mark.gpu

K = 8
NAMES = ("loss", "pot", "delta", "grad1", "grad2")
TILE, NSPLIT = 256, 4  # _raw.SK_COL_TILE, _raw.SK_NSPLIT (asserted below)


def run(a, c, eps, p=1, l1=None, l2=None, grad=True):
    from rfnet_amd import _raw
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).cuda()  # noqa: E731
    out = _raw.sinkhorn(t(a), t(c), eps, p, t(None if l1 is None else np.asarray(l1, np.int32)),
                        t(None if l2 is None else np.asarray(l2, np.int32)), want_grad=grad)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(x, y):
    return all(u.tobytes() == v.tobytes() for u, v in zip(x, y))


def _abs(q):
    return float(np.max(np.abs(q)))


def bars(a, c, eps, p, l1=None, l2=None):
    """-> (ref64 per sample, E32 per quantity, mag per sample and quantity)"""
    b = a.shape[0]
    r64 = [sk_ref(a[i], c[i], eps, p, None if l1 is None else l1[i], None if l2 is None else l2[i]) for i in range(b)]
    r32 = [sk_ref(a[i], c[i], eps, p, None if l1 is None else l1[i], None if l2 is None else l2[i], dtype=np.float32)
           for i in range(b)]
    e32 = [max(_abs(np.asarray(r32[i][q], np.float64) - np.asarray(r64[i][q])) for i in range(b)) for q in range(5)]
    mag = [[_abs(r64[i][q]) for q in range(5)] for i in range(b)]
    for i in range(b):
        mag[i][2] = mag[i][1]
    return r64, e32, mag


def check(got, ref, what, quantities=range(5)):
    """got: the five outputs of the batch; ref: bars(...).  Prints every figure, then asserts.  -> the largest ratio among
    the entries whose error is above the 4-ulp term"""
    r64, e32, mag = ref
    worst, fails = 0.0, []
    for q in quantities:
        for i in range(len(r64)):
            err = _abs(np.asarray(got[q][i], np.float64) - np.asarray(r64[i][q]))
            ulp = 4 * 2.0 ** -23 * mag[i][q]
            ratio = err / e32[q] if e32[q] > 0 else (0.0 if err <= ulp else float("inf"))
            if err > ulp:  # (below the 4-ulp term the ratio says nothing about K)
                worst = max(worst, ratio)
            print(f"{what} sample {i} {NAMES[q]}: err {err:.3e} E32 {e32[q]:.3e} ratio {ratio:.2f} mag {mag[i][q]:.3e}"
                  f"{'' if err > ulp else ' (within 4 ulp)'}")
            if not err <= K * e32[q] + ulp:
                fails.append((NAMES[q], i, err, e32[q], ulp))
    assert not fails, (what, fails)
    return worst


# ---- 1. the reference over column edges -----------------------------------------------------------------------------------
# (257, 1025): one column behind a tile (256) on one side; on the other the count at which a chunk becomes two tiles
# (1024 = NSPLIT tiles in four chunks of one; 1025 = five tiles in three chunks of two, two and one) with one column in the last
SHAPES = [(1, 1), (1, 200), (63, 65), (64, 64), (257, 130), (300, 1000), (1000, 300), (257, 1025)]
SCHEDULES = {"blur0.05": (0.05, 0.5, 7), "blur0.01": (0.01, 0.7, 16)}


def case(n, m, seeds=(1, 2, 3)):
    pairs = [clouds(1000 * s + n + m, n, m) for s in seeds]
    return np.stack([x for x, _ in pairs]), np.stack([y for _, y in pairs])


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n, m", SHAPES)
def test_reference(n, m, p, sched):
    from rfnet_amd import _raw
    assert (_raw.SK_COL_TILE, _raw.SK_NSPLIT) == (TILE, NSPLIT)
    blur, scaling, steps = SCHEDULES[sched]
    eps = schedule(p, blur, scaling)
    assert len(eps) == steps
    a, c = case(n, m)
    got = run(a, c, eps, p)
    worst = check(got, bars(a, c, eps, p), f"{n} x {m} p={p} {sched}")
    print(f"RATIO {n} x {m} p={p} {sched}: {worst:.2f}")
    # the loss-only form: the same bits
    assert same_bits(run(a, c, eps, p, grad=False), got[:3])


# ---- 2. stabilisation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2])
def test_far_apart_clouds_stay_finite(p):
    a, c = stab_clouds()
    a, c = np.stack([a, a[::-1].copy(), a * 0.5]), np.stack([c, c, c[::-1].copy()])
    got = run(a, c, STAB_EPS, p)
    assert all(np.isfinite(g).all() for g in got)
    worst = check(got, bars(a, c, STAB_EPS, p), f"stabilisation p={p}")
    print(f"RATIO stabilisation p={p}: {worst:.2f}")


# ---- 3. self distance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n", [300, 1000])
def test_self_distance_is_exactly_zero(n, p):
    from rfnet_amd import glue
    x = torch.from_numpy(case(n, 1)[0]).cuda().requires_grad_()
    loss, info = glue.sinkhorn_divergence(x, x, p=p, return_info=True)
    assert loss.shape == (3,) and not loss.detach().cpu().numpy().view(np.uint32).any()  # +0.0, not -0.0
    loss.sum().backward()
    assert not x.grad.cpu().numpy().view(np.uint32).any()
    pot = info["pot"].cpu().numpy()
    assert pot[:, :n].tobytes() == pot[:, n:].tobytes() and np.abs(pot).max() > 0  # (it did run)
    raw = run(x.detach().cpu().numpy(), x.detach().cpu().numpy(), schedule(p), p)
    assert not raw[3].view(np.uint32).any() and not raw[4].view(np.uint32).any()


# ---- 4. purity -------------------------------------------------------------------------------------------------------------
LEN1 = np.array([300, 1, 129], np.int32)
LEN2 = np.array([1000, 257, 64], np.int32)


def ragged():
    a, c = case(300, 1000, seeds=(7, 8, 9))
    for i in range(3):  # NaN behind the counts
        a[i, LEN1[i]:] = np.nan
        c[i, LEN2[i]:] = np.nan
    return a, c


@pytest.mark.parametrize("p", [1, 2])
def test_bits(p):
    eps = schedule(p, 0.05, 0.5)
    a, c = case(300, 1000, seeds=(4, 5, 6))
    one = run(a, c, eps, p)
    assert same_bits(one, run(a, c, eps, p)), "two calls differ"
    alone = run(a[1:2], c[1:2], eps, p)
    assert same_bits([x[1:2] for x in one], alone), "a sample depends on its batch"
    # a ragged batch: the per-sample calls on the sliced clouds, bit for bit
    a, c = ragged()
    got = run(a, c, eps, p, LEN1, LEN2)
    assert same_bits(got, run(a, c, eps, p, LEN1.tolist(), LEN2.tolist())), "device and host counts differ"
    from rfnet_amd import _raw
    host = _raw.sinkhorn(torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda(), eps, p, LEN1.tolist(), LEN2.tolist(),
                         want_grad=True)
    assert same_bits(got, [t.cpu().numpy() for t in host])
    for i in range(3):
        l1, l2 = int(LEN1[i]), int(LEN2[i])
        loss, pot, delta, g1, g2 = run(a[i:i + 1, :l1], c[i:i + 1, :l2], eps, p)
        assert loss.tobytes() == got[0][i:i + 1].tobytes() and delta.tobytes() == got[2][i:i + 1].tobytes(), i
        assert pot[0, :l1].tobytes() == got[1][i, :l1].tobytes() and pot[0, l1:].tobytes() == got[1][i, 300:300 + l2].tobytes()
        assert g1[0].tobytes() == got[3][i, :l1].tobytes() and g2[0].tobytes() == got[4][i, :l2].tobytes(), i
        # exactly +0 behind the counts
        assert not got[1][i, l1:300].view(np.uint32).any() and not got[1][i, 300 + l2:].view(np.uint32).any()
        assert not got[3][i, l1:].view(np.uint32).any() and not got[4][i, l2:].view(np.uint32).any()
    check(got, bars(a, c, eps, p, LEN1, LEN2), f"ragged p={p}")


def test_nan_stays_in_its_sample():
    eps = schedule(1, 0.05, 0.5)
    a, c = case(300, 1000, seeds=(4, 5, 6))
    clean = run(a, c, eps, 1)
    a2 = a.copy()
    a2[1, 17, 1] = np.nan
    bad = run(a2, c, eps, 1)  # (run raises unless the call returns RF_OK)
    assert np.isnan(bad[0][1]) and np.isnan(bad[2][1])
    for i in (0, 2):
        assert same_bits([x[i] for x in clean], [x[i] for x in bad]), i


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_with_device_counts():
    """No host synchronisation anywhere: the call is captured with device counts, and a replay returns the eager bits --
    also after the inputs and the counts changed in place."""
    from rfnet_amd import _raw
    eps = schedule(1, 0.05, 0.5)
    a, c = case(300, 1000, seeds=(4, 5, 6))
    a2, c2 = case(300, 1000, seeds=(14, 15, 16))
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    l1, l2 = torch.from_numpy(LEN1).cuda(), torch.from_numpy(LEN2).cuda()
    call = lambda: _raw.sinkhorn(ta, tc, eps, 1, l1, l2, want_grad=True)  # noqa: E731
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
    ta.copy_(torch.from_numpy(a2))
    tc.copy_(torch.from_numpy(c2))
    l1.copy_(torch.tensor([7, 300, 64], dtype=torch.int32))
    l2.copy_(torch.tensor([513, 3, 1000], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    again = call()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, again))
    assert not torch.equal(out[0], eager[0])


# ---- 6. glue -------------------------------------------------------------------------------------------------------------------
def test_glue_backward_with_a_non_uniform_grad_output():
    from rfnet_amd import _raw, glue
    a, c = ragged()
    a, c = np.nan_to_num(a, nan=9.0), np.nan_to_num(c, nan=-9.0)  # (a NaN times a zero gradient would be NaN in autograd)
    ta, tc = torch.from_numpy(a).cuda().requires_grad_(), torch.from_numpy(c).cuda().requires_grad_()
    loss, info = glue.sinkhorn_divergence(ta, tc, p=2, blur=0.05, lengths1=LEN1, lengths2=LEN2, return_info=True)
    raw = _raw.sinkhorn(ta.detach(), tc.detach(), schedule(2, 0.05, 0.5), 2, LEN1, LEN2, want_grad=True)
    assert loss.shape == (3,) and torch.equal(loss.detach(), raw[0])
    assert torch.equal(info["pot"], raw[1]) and torch.equal(info["delta"], raw[2])
    assert not info["pot"].requires_grad and not info["delta"].requires_grad
    w = torch.tensor([0.5, -2.0, 4.0], device="cuda")
    (loss * w).sum().backward()
    assert torch.equal(ta.grad, w[:, None, None] * raw[3]) and torch.equal(tc.grad, w[:, None, None] * raw[4])
    assert ta.grad.abs().max() > 0
    # an explicit schedule; only one side requires grad; and none
    tb = tc.detach()
    e = schedule(2, 0.05, 0.5)
    one = glue.sinkhorn_divergence(ta, tb, p=2, eps=e, lengths1=LEN1, lengths2=LEN2)
    assert torch.equal(one, loss) and one.requires_grad
    none = glue.sinkhorn_divergence(ta.detach(), tb, p=2, eps=e, lengths1=LEN1, lengths2=LEN2)
    assert torch.equal(none, loss.detach()) and not none.requires_grad


def test_numpy_inputs_round_trip():
    from rfnet_amd import _raw
    a, c = case(70, 90)
    out = _raw.sinkhorn(a, c, schedule(1), 1, lengths1=[70, 9, 1], lengths2=[1, 90, 5], want_grad=True)
    assert len(out) == 5 and all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in out)
    assert same_bits(out, run(a, c, schedule(1), 1, [70, 9, 1], [1, 90, 5]))
    assert len(_raw.sinkhorn(torch.from_numpy(a), torch.from_numpy(c), schedule(1))) == 3


# ---- 7. against the exact earth mover's distance ----------------------------------------------------------------------------------
def test_against_exact_emd():
    """Reported, not asserted beyond 0 < S_eps: the ratio of S_eps to the exact EMD at a small blur.  The asserted part is
    the agreement with sk_ref."""
    from rfnet_amd import glue
    eps = schedule(1, 0.02, 0.7, extra=32)
    a, c = case(256, 256)
    got = run(a, c, eps, 1)
    check(got, bars(a, c, eps, 1), "256 x 256 blur 0.02")
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    cost = glue.emd_assignment(ta, tc)["cost"].cpu().numpy() / 256.0
    for i in range(3):
        print(f"EMD sample {i}: S_eps {got[0][i]:.6f} exact EMD {cost[i]:.6f} ratio {got[0][i] / cost[i]:.4f} "
              f"delta {got[2][i]:.3e}")
    assert (got[0] > 0).all()
