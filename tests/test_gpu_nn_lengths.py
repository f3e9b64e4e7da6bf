"""Ragged batches on the GPU (rf_nn_distance_lengths and the loss / gradient entries, include/rfops.h): on every valid slot the
outputs are bit for bit what the existing op returns on that sample's unpadded slices alone, padded slots are (0, -1), nothing
in the padding reaches a result (NaN, inf, huge values or copies of valid points there change nothing), and the losses and
gradients match a per-sample loop of the existing functions."""
import numpy as np
import pytest
import torch

from rfnet_amd import _raw, glue

pytestmark = pytest.mark.gpu

MODES = ("dense", "culled", "auto")
SHAPES = [(1, 1, 1), (3, 999, 301), (2, 5000, 700), (3, 2048, 2048), (2, 16384, 16384), (1, 65536, 4096),
          (3, 65536, 4096)]


def _lengths(rng, b, n):
    """Random counts in [1, n] with 1 and n among them (when b allows)."""
    v = rng.randint(1, n + 1, size=b).astype(np.int32)
    v[-1] = n
    if b > 1:
        v[0] = 1
    return v


def _clouds(seed, b, n, m):
    rng = np.random.RandomState(seed)
    return rng, rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _per_sample(a, c, l1, l2, mode):
    """The existing op on each sample's unpadded slices."""
    out = []
    for i in range(a.shape[0]):
        ai = torch.from_numpy(a[i:i + 1, :l1[i]].copy()).cuda()
        ci = torch.from_numpy(c[i:i + 1, :l2[i]].copy()).cuda()
        out.append([t.cpu().numpy()[0] for t in _raw.nn_distance(ai, ci, mode=mode)])
    return out


def _check_against(got, ref, l1, l2):
    d1, i1, d2, i2 = [t.cpu().numpy() for t in got]
    for i, (r1, ri1, r2, ri2) in enumerate(ref):
        n1, n2 = l1[i], l2[i]
        assert _same(d1[i, :n1], r1) and _same(i1[i, :n1], ri1), ("direction 1", i, n1, n2)
        assert _same(d2[i, :n2], r2) and _same(i2[i, :n2], ri2), ("direction 2", i, n1, n2)
        assert _same(d1[i, n1:], np.zeros(d1.shape[1] - n1, np.float32)) and (i1[i, n1:] == -1).all(), i
        assert _same(d2[i, n2:], np.zeros(d2.shape[1] - n2, np.float32)) and (i2[i, n2:] == -1).all(), i
        assert ((i1[i, :n1] >= 0) & (i1[i, :n1] < n2)).all() and ((i2[i, :n2] >= 0) & (i2[i, :n2] < n1)).all(), i


def _ragged(a, c, l1, l2, mode="auto"):
    return _raw.nn_distance(torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda(), mode=mode,
                            lengths1=torch.from_numpy(l1).cuda(), lengths2=torch.from_numpy(l2).cuda())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,m", SHAPES)
def test_matches_per_sample_slices(orc, mode, b, n, m):
    rng, a, c = _clouds(b * 7 + n + m, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    got = _ragged(a, c, l1, l2, mode)
    _check_against(got, _per_sample(a, c, l1, l2, mode), l1, l2)
    if (n * m <= 2048 * 2048) or b == 1 and n * m <= 1 << 24:  # finite data: also the CPU oracle, where it is quick
        for i in range(b):
            e = orc.nn_distance(a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]])
            d1, i1, d2, i2 = [t.cpu().numpy()[i] for t in got]
            assert _same(d1[:l1[i]], e[0][0]) and _same(i1[:l1[i]], e[1][0]), i
            assert _same(d2[:l2[i]], e[2][0]) and _same(i2[:l2[i]], e[3][0]), i


def _fill(a, lens, how, rng):
    a = a.copy()
    for i, l in enumerate(lens):
        k = a.shape[1] - l
        if k == 0:
            continue
        if how == "copies":  # exact ties with the valid points: a wrong implementation resolves them into the padding
            a[i, l:] = a[i, np.arange(k) % l]
        elif how == "nearest":  # copies of a valid point slightly moved: the padding would win the minimum
            a[i, l:] = a[i, rng.randint(0, l, size=k)] + np.float32(1e-7)
        else:
            a[i, l:] = np.float32({"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "1e30": 1e30}[how])
    return a


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,m", [(4, 999, 301), (3, 3000, 16384), (2, 8192, 8192)])
def test_hostile_padding_changes_nothing(mode, b, n, m):
    rng, a, c = _clouds(11 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    clean = [t.cpu().numpy() for t in _ragged(a, c, l1, l2, mode)]
    for how in ("nan", "inf", "-inf", "1e30", "copies", "nearest"):
        got = _ragged(_fill(a, l1, how, rng), _fill(c, l2, how, rng), l1, l2, mode)
        for g, e in zip(got, clean):
            assert _same(g, e), (how, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,m", [(2, 999, 301), (3, 2048, 2048), (2, 3000, 16384)])
def test_full_lengths_equal_the_existing_op(mode, b, n, m):
    _, a, c = _clouds(5, b, n, m)
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    exp = _raw.nn_distance(ta, tc, mode=mode)
    got = _raw.nn_distance(ta, tc, mode=mode, lengths1=[n] * b, lengths2=torch.full((b,), m, device="cuda"))
    for g, e in zip(got, exp):
        assert _same(g, e)


def _resample_style(rng, a, lens):
    """Each sample's valid region: its first few points repeated at random (evalio.resample_pcd's duplicates)."""
    a = a.copy()
    for i, l in enumerate(lens):
        k = max(1, l // 3)
        a[i, k:l] = a[i, rng.randint(0, k, size=l - k)]
    return a


def _many_copies(a, lens):
    """Three or more exact copies of one point, far apart in index (different blocks of either sweep)."""
    a = a.copy()
    for i, l in enumerate(lens):
        third = l // 3
        for j in range(0, third, 61):
            a[i, [j + third, j + 2 * third]] = a[i, j]
            if j + 3 * third < l:
                a[i, j + 3 * third] = a[i, j]
    return a


def _non_finite(rng, a, lens):
    a = a.copy()
    for i, l in enumerate(lens):
        for v in (np.nan, np.inf, -np.inf):
            j = rng.randint(0, l)
            a[i, j, rng.randint(0, 3)] = v
    return a


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["resample", "copies", "non_finite"])
@pytest.mark.parametrize("b,n,m", [(3, 999, 301), (2, 3000, 16384), (2, 4096, 4096)])
def test_hard_valid_regions(mode, kind, b, n, m):
    rng, a, c = _clouds(23 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[0] = max(l1[0], 2)
    if kind == "resample":
        a, c = _resample_style(rng, a, l1), _resample_style(rng, c, l2)
    elif kind == "copies":
        a, c = _many_copies(a, l1), _many_copies(c, l2)
        c = np.where(rng.rand(b, m, 1) < 0.5, c, a[:, :1]).astype(np.float32)  # ties across the clouds too
    else:
        a, c = _non_finite(rng, a, l1), _non_finite(rng, c, l2)
    _check_against(_ragged(a, c, l1, l2, mode), _per_sample(a, c, l1, l2, mode), l1, l2)


def test_length_formats_agree():
    b, n, m = 3, 2000, 1500
    rng, a, c = _clouds(3, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    ref = [t.cpu().numpy() for t in _raw.nn_distance(ta, tc, lengths1=l1.tolist(), lengths2=tuple(l2.tolist()))]
    for f in (lambda v: torch.from_numpy(v).cuda(), lambda v: torch.from_numpy(v.astype(np.int64)).cuda(),
              lambda v: torch.from_numpy(v), lambda v: v.astype(np.int64)):
        got = _raw.nn_distance(ta, tc, lengths1=f(l1), lengths2=f(l2))
        for g, e in zip(got, ref):
            assert _same(g, e)
    # CPU clouds come back on the CPU
    got = _raw.nn_distance(a, c, lengths1=l1, lengths2=l2)
    assert isinstance(got[0], np.ndarray)
    for g, e in zip(got, ref):
        assert _same(g, e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,m,l1,l2", [(4, 16384, 16384, [1, 7, 64, 16384], [64, 1, 33, 500]),
                                         (3, 65536, 2048, [1, 40000, 65535], [2048, 5, 1]),
                                         (2, 65536, 65536, [40000, 17], [3, 65536])])
def test_short_counts_at_large_sizes(mode, b, n, m, l1, l2):
    """Counts far below the size, on the sizes whose culled sort does not fit the registers (n > 16384) too."""
    rng, a, c = _clouds(n + len(l1), b, n, m)
    l1, l2 = np.array(l1, np.int32), np.array(l2, np.int32)
    got = _ragged(a, c, l1, l2, mode)
    _check_against(got, _per_sample(a, c, l1, l2, mode), l1, l2)
    for how in ("nan", "copies"):
        bad = _ragged(_fill(a, l1, how, rng), _fill(c, l2, how, rng), l1, l2, mode)
        for g, e in zip(bad, got):
            assert _same(g, e), how


def test_out_of_range_device_lengths_are_clamped():
    b, n, m = 3, 700, 500
    _, a, c = _clouds(9, b, n, m)
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    bad = _raw.nn_distance(ta, tc, lengths1=torch.tensor([0, -5, 10 ** 6], device="cuda"),
                           lengths2=torch.tensor([m + 1, 3, 2 ** 31 - 1], device="cuda", dtype=torch.int64))
    ok = _raw.nn_distance(ta, tc, lengths1=[1, 1, n], lengths2=[m, 3, m])
    for g, e in zip(bad, ok):
        assert _same(g, e)
    # int64 counts beyond the int32 range are clamped, not wrapped into the domain
    wide = _raw.nn_distance(ta, tc, lengths1=torch.tensor([2 ** 32 + 5, -(2 ** 32) + 3, 1], device="cuda"),
                            lengths2=[m, 3, m])
    ok = _raw.nn_distance(ta, tc, lengths1=[n, 1, 1], lengths2=[m, 3, m])
    for g, e in zip(wide, ok):
        assert _same(g, e)


def _tol(got, exp):
    return torch.allclose(got, exp, rtol=1e-4, atol=1e-5 * max(float(exp.abs().max()), 1e-30))


@pytest.mark.parametrize("b,n,m", [(3, 999, 301), (2, 3000, 16384), (4, 2048, 2048)])
def test_nn_distance_lengths_gradient(b, n, m):
    rng, a, c = _clouds(31 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    ta = torch.from_numpy(a).cuda().requires_grad_(True)
    tc = torch.from_numpy(c).cuda().requires_grad_(True)
    w1 = torch.from_numpy(rng.rand(b, n).astype(np.float32) + 0.5).cuda()  # nonzero upstream grads in padded slots too
    w2 = torch.from_numpy(rng.rand(b, m).astype(np.float32) + 0.5).cuda()
    d1, i1, d2, i2 = glue.nn_distance_lengths(ta, tc, torch.from_numpy(l1).cuda(), l2.tolist())
    ((d1 * w1).sum() + (d2 * w2).sum()).backward()
    for i in range(b):
        ai, ci = a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]]
        e = _raw.nn_distance(torch.from_numpy(ai.copy()).cuda(), torch.from_numpy(ci.copy()).cuda())
        g1, g2 = _raw.nn_distance_grad(torch.from_numpy(ai.copy()).cuda(), torch.from_numpy(ci.copy()).cuda(),
                                       w1[i:i + 1, :l1[i]].contiguous(), e[1], w2[i:i + 1, :l2[i]].contiguous(), e[3])
        assert _tol(ta.grad[i, :l1[i]], g1[0]) and _tol(tc.grad[i, :l2[i]], g2[0]), i
        assert (ta.grad[i, l1[i]:] == 0).all() and (tc.grad[i, l2[i]:] == 0).all(), i
        assert not torch.signbit(ta.grad[i, l1[i]:]).any() and not torch.signbit(tc.grad[i, l2[i]:]).any(), i


@pytest.mark.parametrize("b,n,m", [(3, 999, 301), (4, 3000, 16384), (3, 16384, 16384), (4, 2048, 2048)])
@pytest.mark.parametrize("which", ["per_sample", "big", "fidelity"])
def test_losses_match_a_per_sample_loop(b, n, m, which):
    rng, a, c = _clouds(41 + n + m, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    # hostile padding: nothing of it may reach the losses or the valid gradient rows
    a, c = _fill(a, l1, "nan", rng), _fill(c, l2, "copies", rng)
    ta = torch.from_numpy(a).cuda().requires_grad_(True)
    tc = torch.from_numpy(c).cuda().requires_grad_(True)
    wl = torch.from_numpy(rng.rand(b, 2).astype(np.float32) + 0.5).cuda()
    if which == "per_sample":
        loss, idx1 = glue.chamfer_per_sample(ta, tc, lengths1=l1, lengths2=torch.from_numpy(l2).cuda())
        (loss * wl).sum().backward()
    elif which == "big":
        loss, idx1 = glue.chamfer_big(ta, tc, lengths1=torch.from_numpy(l1).cuda(), lengths2=l2)
        loss.backward()
    else:
        loss = glue.fidelity_loss(ta, tc, lengths1=l1, lengths2=l2)
        loss.backward()
    parts, g1s, g2s = [], [], []
    for i in range(b):
        ai = torch.from_numpy(a[i:i + 1, :l1[i]].copy()).cuda().requires_grad_(True)
        ci = torch.from_numpy(c[i:i + 1, :l2[i]].copy()).cuda().requires_grad_(True)
        if which == "per_sample":
            li, _ = glue.chamfer_per_sample(ai, ci)
            (li * wl[i:i + 1]).sum().backward()
            parts.append(li[0].detach())
        elif which == "big":
            li, _ = glue.chamfer_per_sample(ai, ci)
            ((li[0, 0] + li[0, 1]) / (2 * b)).backward()
            parts.append(li[0].detach())
        else:
            li = glue.fidelity_loss(ai, ci)
            (li / b).backward()
            parts.append(li.detach().reshape(1))
        g1s.append(ai.grad[0])
        g2s.append(ci.grad[0])
    if which == "per_sample":
        exp = torch.stack(parts)
        assert torch.allclose(loss.detach(), exp, rtol=1e-6, atol=0)
        assert (idx1[0, l1[0]:] == -1).all()
    elif which == "big":
        exp = torch.stack(parts)
        ref = (exp[:, 0].mean() + exp[:, 1].mean()) / 2
        assert torch.allclose(loss.detach(), ref, rtol=1e-6, atol=0)
    else:
        assert torch.allclose(loss.detach(), torch.cat(parts).mean(), rtol=1e-6, atol=0)
    for i in range(b):
        assert _tol(ta.grad[i, :l1[i]], g1s[i]) and _tol(tc.grad[i, :l2[i]], g2s[i]), i
        assert (ta.grad[i, l1[i]:] == 0).all() and (tc.grad[i, l2[i]:] == 0).all(), i


def test_losses_bit_identical_per_sample():
    """The per-sample means are summed in the order the sample alone takes: bit-identical, not just close."""
    b, n, m = 4, 3000, 2500
    rng, a, c = _clouds(77, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    loss, d1, i1, d2, i2 = _raw.chamfer_loss(a, c, lengths1=l1, lengths2=l2)
    for i in range(b):
        li = _raw.chamfer_loss(a[i:i + 1, :l1[i]].copy(), c[i:i + 1, :l2[i]].copy())[0]
        assert _same(loss[i], li[0]), i


def test_graph_capture_with_device_lengths():
    """Lengths live on the device: a ragged call captures into a HIP graph (no host synchronisation) and replays."""
    b, n, m = 4, 1500, 1200
    rng, a, c = _clouds(5, b, n, m)
    ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    l1 = torch.from_numpy(_lengths(rng, b, n)).cuda()
    l2 = torch.from_numpy(_lengths(rng, b, m)).cuda()
    exp = [t.clone() for t in _raw.nn_distance(ta, tc, lengths1=l1, lengths2=l2)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _raw.nn_distance(ta, tc, lengths1=l1, lengths2=l2)  # warm the workspace cache outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _raw.nn_distance(ta, tc, lengths1=l1, lengths2=l2)
    l1.copy_(torch.full((b,), n, device="cuda", dtype=torch.int32))  # new counts, same graph
    g.replay()
    torch.cuda.synchronize()
    full = _raw.nn_distance(ta, tc, lengths1=l1, lengths2=l2)
    for o, f in zip(out, full):
        assert _same(o, f)
    assert not all(_same(o, e) for o, e in zip(out, exp))
