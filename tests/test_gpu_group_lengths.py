"""Ragged batches through sampling, grouping and neighbour search on the GPU (include/rfops.h: rf_farthestpointsampling_lengths,
rf_queryballpoint_lengths, rf_sample_and_group_lengths, rf_threenn_lengths, rf_knn_lengths, rf_knn_grad_lengths): on every valid
slot the outputs are bit for bit what the existing op returns on that sample's unpadded slices alone (and what the CPU oracle,
or for knn the numpy statement of its contract, returns there), in every form; padded output slots are zeros; and nothing in
the padding reaches a result -- NaN, inf, huge values or copies of valid points there change nothing, while the same batch
through the plain op does pick them up (the inputs are proven hostile).  The reference of a ragged call is never the code
under test."""
import numpy as np
import pytest
import torch

from rfnet_amd import _raw

pytestmark = pytest.mark.gpu

FILLS = ("nan", "inf", "-inf", "1e30", "copies", "nearest")


def _lengths(rng, b, n):
    """Random counts in [1, n] with 1 and n among them (when b allows)."""
    v = rng.randint(1, n + 1, size=b).astype(np.int32)
    v[-1] = n
    if b > 1:
        v[0] = 1
    return v


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _zeros(a):
    """Exactly zero, bit pattern included (no -0.0)."""
    return not _bits(a).any()


def _fill(a, lens, how, rng):
    a = a.copy()
    for i, l in enumerate(lens):
        k = a.shape[1] - l
        if k == 0:
            continue
        if how == "copies":  # exact ties with the valid points: a wrong implementation resolves them into the padding
            a[i, l:] = a[i, np.arange(k) % l]
        elif how == "nearest":  # copies of a valid point slightly moved
            a[i, l:] = a[i, rng.randint(0, l, size=k)] + np.float32(1e-7)
        else:
            a[i, l:] = np.float32({"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "1e30": 1e30}[how])
    return a


def _non_finite(rng, a, lens):
    a = a.copy()
    for i, l in enumerate(lens):
        for v in (np.nan, np.inf, -np.inf):
            a[i, rng.randint(0, l), rng.randint(0, 3)] = v
    return a


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ farthest_point_sample -----------------------------------
def _fps(a, m, ln, lo=None, with_xyz=True):
    return _raw.farthest_point_sample(m, _cuda(a), lengths=None if ln is None else _cuda(ln),
                                      npoints=None if lo is None else _cuda(lo), with_xyz=with_xyz)


def _fps_check(got, a, m, ln, lo, orc=None):
    """Rows [0, lo[i]) = the existing op (and the oracle) on a[i, :ln[i]]; zeros behind; new_xyz = the gathered rows."""
    idx, nx = [t.cpu().numpy() for t in got]
    for i in range(a.shape[0]):
        l, k = int(ln[i]), int(m if lo is None else lo[i])
        sl = a[i:i + 1, :l].copy()
        ref = _raw.farthest_point_sample(k, _cuda(sl)).cpu().numpy()[0]
        assert _same(idx[i, :k], ref), ("existing op", i, l, k)
        if orc is not None:
            assert _same(idx[i, :k], orc.farthest_point_sample(k, sl)[0]), ("oracle", i, l, k)
        assert ((idx[i, :k] >= 0) & (idx[i, :k] < l)).all(), i
        assert _same(nx[i, :k], a[i, idx[i, :k]]), ("new_xyz", i)
        assert _zeros(idx[i, k:]) and _zeros(nx[i, k:]), ("padded rows", i)


# (b, n, m): n <= 512 / 1024 / 2048 / 4096 / 8192 / 16384 reach the six register-resident instantiations, (3000, 512),
# (8000, 300) and (16384, 1024) the sorted form with 4, 8 and 16 points per lane, (2500, 600) with 4, 40000 the global-memory kernel
FPS_SHAPES = [(3, 300, 40), (3, 700, 64), (3, 700, 900), (2, 2000, 128), (3, 3000, 64), (3, 3000, 512), (2, 2500, 600),
              (3, 8000, 100), (3, 8000, 300), (3, 16384, 64), (4, 16384, 1024), (2, 40000, 200)]


@pytest.mark.parametrize("b,n,m", FPS_SHAPES)
def test_fps_matches_per_sample_slices(orc, b, n, m):
    rng = np.random.RandomState(b + n + m)
    a = rng.randn(b, n, 3).astype(np.float32)
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)  # counts of 1 among them: m above the smallest cloud
    _fps_check(_fps(a, m, ln, lo), a, m, ln, lo, orc)
    _fps_check(_fps(a, m, ln, None), a, m, ln, None, orc)
    big = np.maximum(ln, min(n, m + 1)).astype(np.int32)  # ... and every cloud larger than m
    _fps_check(_fps(a, m, big, lo), a, m, big, lo, orc)
    idx_only = _fps(a, m, ln, lo, with_xyz=False)
    assert _same(idx_only, _fps(a, m, ln, lo)[0])


@pytest.mark.parametrize("b,n,m", [(4, 700, 64), (3, 3000, 512), (3, 16384, 300), (2, 40000, 100)])
def test_fps_hostile_padding_changes_nothing(b, n, m):
    rng = np.random.RandomState(11 + n)
    a = rng.randn(b, n, 3).astype(np.float32)
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)
    ln[1] = n // 2
    clean = _fps(a, m, ln, lo)
    for how in FILLS:
        bad = _fill(a, ln, how, rng)
        got = _fps(bad, m, ln, lo)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), how
    if n == 700:  # the inputs are hostile: the plain op on the same batch picks the far-away padding as its second sample
        plain = _raw.farthest_point_sample(m, _cuda(_fill(a, ln, "1e30", rng))).cpu().numpy()
        assert plain[1, 1] >= ln[1] and clean[0].cpu().numpy()[1, 1] < ln[1]


@pytest.mark.parametrize("n,m", [(16384, 64), (16384, 512), (65536, 40)])
def test_fps_short_counts_at_large_sizes(orc, n, m):
    ln = np.array([1, 7, 64, n], np.int32)
    rng = np.random.RandomState(n + m)
    a = rng.randn(4, n, 3).astype(np.float32)
    lo = np.array([m, m, 5, m], np.int32)
    got = _fps(a, m, ln, lo)
    _fps_check(got, a, m, ln, lo, orc)  # m > 1, 7 (and 64 at m = 512): the repeats of the reference, in the sorted form too
    for how in ("nan", "copies"):
        bad = _fps(_fill(a, ln, how, rng), m, ln, lo)
        assert _same(bad[0], got[0]) and _same(bad[1], got[1]), how


@pytest.mark.parametrize("b,n,m", [(2, 700, 64), (2, 3000, 512), (2, 16384, 1024), (1, 40000, 50)])
def test_fps_full_counts_equal_the_existing_op(b, n, m):
    rng = np.random.RandomState(5)
    a = rng.randn(b, n, 3).astype(np.float32)
    exp = _raw.farthest_point_sample(m, _cuda(a))
    for ln, lo in (([n] * b, None), (None, [m] * b), (torch.full((b,), n, device="cuda"), [m] * b)):
        got = _raw.farthest_point_sample(m, _cuda(a), lengths=ln, npoints=lo)
        assert _same(got, exp)
    # npoints: a prefix of the full result, zeros behind
    lo = np.array([1, m // 2][:b], np.int32)
    got = _raw.farthest_point_sample(m, _cuda(a), npoints=lo).cpu().numpy()
    for i in range(b):
        assert _same(got[i, :lo[i]], exp[i, :lo[i]]) and _zeros(got[i, lo[i]:])


def test_fps_count_formats_agree_and_device_counts_are_clamped():
    b, n, m = 3, 2000, 150
    rng = np.random.RandomState(3)
    a = rng.randn(b, n, 3).astype(np.float32)
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)
    ta = _cuda(a)
    ref = _raw.farthest_point_sample(m, ta, lengths=ln.tolist(), npoints=tuple(lo.tolist()))
    for f in (lambda v: torch.from_numpy(v).cuda(), lambda v: torch.from_numpy(v.astype(np.int64)).cuda(),
              lambda v: torch.from_numpy(v), lambda v: v.astype(np.int64)):
        assert _same(_raw.farthest_point_sample(m, ta, lengths=f(ln), npoints=f(lo)), ref)
    got = _raw.farthest_point_sample(m, a, lengths=ln, npoints=lo)  # CPU clouds come back on the CPU
    assert isinstance(got, np.ndarray) and _same(got, ref)
    # out-of-range device values are clamped into [1, n] / [1, m], not wrapped
    bad = _raw.farthest_point_sample(m, ta, lengths=torch.tensor([0, -5, 10 ** 6], device="cuda", dtype=torch.int32),
                                     npoints=torch.tensor([m + 1, 0, 2 ** 31 - 1], device="cuda", dtype=torch.int64))
    assert _same(bad, _raw.farthest_point_sample(m, ta, lengths=[1, 1, n], npoints=[m, 1, m]))
    wide = _raw.farthest_point_sample(m, ta, lengths=torch.tensor([2 ** 32 + 5, -(2 ** 32) + 3, 1], device="cuda"))
    assert _same(wide, _raw.farthest_point_sample(m, ta, lengths=[n, 1, 1]))


@pytest.mark.parametrize("b,n,m", [(3, 700, 64), (3, 3000, 512), (2, 16384, 300), (2, 20000, 60)])
def test_fps_non_finite_values_inside_the_valid_region(b, n, m):
    rng = np.random.RandomState(23 + n)
    a = rng.randn(b, n, 3).astype(np.float32)
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)
    ln[0] = 5
    a = _non_finite(rng, a, ln)
    _fps_check(_fps(a, m, ln, lo), a, m, ln, lo)


@pytest.mark.parametrize("n,m", [(1500, 100), (5000, 600)])
def test_fps_graph_capture_with_device_counts(n, m):
    """Counts live on the device: a ragged call captures into a HIP graph (no host synchronisation) and a replay sees new ones."""
    b = 4
    rng = np.random.RandomState(5)
    ta = _cuda(rng.randn(b, n, 3).astype(np.float32))
    ln, lo = _cuda(_lengths(rng, b, n)), _cuda(_lengths(rng, b, m))
    exp = _raw.farthest_point_sample(m, ta, lengths=ln, npoints=lo).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _raw.farthest_point_sample(m, ta, lengths=ln, npoints=lo)  # warm the workspace cache outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _raw.farthest_point_sample(m, ta, lengths=ln, npoints=lo)
    ln.copy_(torch.full((b,), n, device="cuda", dtype=torch.int32))  # new counts, same graph
    lo.copy_(torch.full((b,), m, device="cuda", dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, _raw.farthest_point_sample(m, ta))
    assert not _same(out, exp)


@pytest.mark.parametrize("seed", range(30))
def test_fps_fuzz(orc, seed):
    rng = np.random.RandomState(1000 + seed)
    b = int(rng.randint(1, 5))
    n = int(rng.choice([rng.randint(1, 600), rng.randint(600, 5000), rng.randint(5000, 16385), rng.randint(16385, 30000)]))
    m = int(rng.choice([rng.randint(1, 40), rng.randint(40, 700)]))
    a = (rng.randn(b, n, 3) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
    if seed % 3 == 0:  # duplicates: ties decided by the (k mod 512) rule
        a[:, n // 2:] = a[:, :n - n // 2]
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)
    a = _fill(a, ln, FILLS[seed % len(FILLS)], rng)
    _fps_check(_fps(a, m, ln, lo), a, m, ln, lo, orc)


# ------------------------------------------------------------------ query_ball_point ----------------------------------------
FORMS = ("scan", "boxes", "auto")
ORACLE_PAIRS = 1 << 24  # per sample: where the CPU oracle is quick


def _qb(r, ns, a, q, l1, l2, form="auto"):
    return [t.cpu().numpy() for t in _raw.query_ball_point(r, ns, _cuda(a), _cuda(q), form=form,
                                                           lengths1=None if l1 is None else _cuda(l1),
                                                           lengths2=None if l2 is None else _cuda(l2))]


def _qb_check(got, r, ns, a, q, l1, l2, orc=None):
    """Valid queries: the existing op (its untouched rows of empty balls read 0 through the wrapper's zero fill) and the
    oracle on the slices; padded queries: zeros."""
    idx, cnt = got
    for i in range(a.shape[0]):
        n1, n2 = int(l1[i]), int(l2[i])
        ai, qi = a[i:i + 1, :n1].copy(), q[i:i + 1, :n2].copy()
        ri, rc = _raw.query_ball_point(r, ns, ai, qi)
        assert _same(idx[i, :n2], ri[0]) and _same(cnt[i, :n2], rc[0]), ("existing op", i, n1, n2)
        if orc is not None and n1 * n2 <= ORACLE_PAIRS:
            oi, oc = orc.query_ball_point(r, ns, ai, qi)
            assert _same(idx[i, :n2], oi[0]) and _same(cnt[i, :n2], oc[0]), ("oracle", i, n1, n2)
        assert ((idx[i, :n2] >= 0) & (idx[i, :n2] < n1)).all(), i
        assert _zeros(idx[i, n2:]) and _zeros(cnt[i, n2:]), ("padded rows", i)


def _qb_data(seed, b, n, m):
    rng = np.random.RandomState(seed)
    a = rng.randn(b, n, 3).astype(np.float32)
    q = (rng.randn(b, m, 3) * 1.3).astype(np.float32)  # some queries out in the thin: empty balls
    return rng, a, q


# n < 8 and nsample > 64: query_ball_kernel; the rest of the scans: query_ball_lanes_kernel; boxes: padded n >= 64
QB_SHAPES = [(3, 5, 9, 4, 0.8), (3, 300, 77, 80, 0.5), (3, 300, 200, 1, 0.3), (3, 999, 301, 32, 0.3), (2, 2048, 700, 64, 0.25),
             (3, 5000, 1024, 32, 0.2), (2, 16384, 2048, 32, 0.1), (2, 16384, 512, 1, 0.15), (2, 65536, 256, 64, 0.08)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,ns,r", QB_SHAPES)
def test_ball_matches_per_sample_slices(orc, form, b, n, m, ns, r):
    if form == "boxes" and (n < 64 or ns > 64):
        with pytest.raises(ValueError):
            _qb(r, ns, *_qb_data(0, b, n, m)[1:], None, [1] * b, form)
        return
    rng, a, q = _qb_data(n + m + ns, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    _qb_check(_qb(r, ns, a, q, l1, l2, form), r, ns, a, q, l1, l2, orc)
    _qb_check(_qb(r, ns, a, q, None, l2, form), r, ns, a, q, [n] * b, l2)
    _qb_check(_qb(r, ns, a, q, l1, None, form), r, ns, a, q, l1, [m] * b)
    # the device radius of the reference's op
    got = _raw.query_ball_point(torch.tensor([r], device="cuda"), ns, _cuda(a), _cuda(q), form=form, lengths1=l1, lengths2=l2)
    assert all(_same(g, e) for g, e in zip(got, _qb(r, ns, a, q, l1, l2, form)))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,ns,r", [(4, 999, 301, 32, 0.3), (3, 3000, 1024, 16, 0.25), (2, 16384, 512, 64, 0.12)])
def test_ball_hostile_padding_changes_nothing(form, b, n, m, ns, r):
    rng, a, q = _qb_data(11 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[1], l2[1] = n // 3, m // 2
    clean = _qb(r, ns, a, q, l1, l2, form)
    for how in FILLS:
        got = _qb(r, ns, _fill(a, l1, how, rng), _fill(q, l2, how, rng), l1, l2, form)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), how
    if form == "auto":  # the inputs are hostile: the plain op on the same batch counts the copies
        plain = _raw.query_ball_point(r, 2 * ns, _fill(a, l1, "copies", rng)[1:2], q[1:2, :l2[1]].copy())[1]
        alone = _raw.query_ball_point(r, 2 * ns, a[1:2, :l1[1]].copy(), q[1:2, :l2[1]].copy())[1]
        assert (plain >= alone).all() and (plain > alone).any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,m", [(16384, 300), (65536, 100)])
def test_ball_short_counts_at_large_sizes(orc, form, n, m):
    """Counts of 1, 7 and 64 in large slots: below the boxed form's own minimum of 64 points too."""
    rng, a, q = _qb_data(n, 4, n, m)
    l1, l2 = np.array([1, 7, 64, n], np.int32), np.array([m, 1, 7, 64], np.int32)
    q[:, ::2] = a[:, :1] + np.float32(0.01)  # balls that do hold the few valid points
    for ns, r in ((32, 0.3), (1, 5.0), (64, 1e30)):
        got = _qb(r, ns, a, q, l1, l2, form)
        _qb_check(got, r, ns, a, q, l1, l2, orc)
        for how in ("nan", "copies"):
            bad = _qb(r, ns, _fill(a, l1, how, rng), _fill(q, l2, how, rng), l1, l2, form)
            assert _same(bad[0], got[0]) and _same(bad[1], got[1]), how


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,ns,r", [(2, 300, 100, 16, 0.4), (2, 4096, 512, 32, 0.2)])
def test_ball_full_counts_equal_the_existing_op(form, b, n, m, ns, r):
    _, a, q = _qb_data(5, b, n, m)
    exp = _raw.query_ball_point(r, ns, _cuda(a), _cuda(q), form=form)
    got = _raw.query_ball_point(r, ns, _cuda(a), _cuda(q), form=form, lengths1=[n] * b,
                                lengths2=torch.full((b,), m, device="cuda"))
    assert _same(got[0], exp[0]) and _same(got[1], exp[1])
    # clamped device counts, every host format
    l1, l2 = np.array([n // 2, 1][:b], np.int32), np.array([1, m][:b], np.int32)
    ref = _qb(r, ns, a, q, l1, l2, form)
    for f in (lambda v: v.tolist(), lambda v: torch.from_numpy(v.astype(np.int64)).cuda(), lambda v: v.astype(np.int64)):
        got = _raw.query_ball_point(r, ns, _cuda(a), _cuda(q), form=form, lengths1=f(l1), lengths2=f(l2))
        assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    bad = _raw.query_ball_point(r, ns, _cuda(a), _cuda(q), form=form,
                                lengths1=torch.tensor([0, 10 ** 6][:b], device="cuda", dtype=torch.int32),
                                lengths2=torch.tensor([-3, 2 ** 40][:b], device="cuda"))
    ok = _qb(r, ns, a, q, np.array([1, n][:b], np.int32), np.array([1, m][:b], np.int32), form)
    assert _same(bad[0], ok[0]) and _same(bad[1], ok[1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,ns,r", [(3, 999, 301, 32, 0.3), (2, 4096, 700, 16, 0.2)])
def test_ball_non_finite_values_inside_the_valid_region(form, b, n, m, ns, r):
    rng, a, q = _qb_data(23 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[0], l2[0] = 9, 9
    a, q = _non_finite(rng, a, l1), _non_finite(rng, q, l2)
    _qb_check(_qb(r, ns, a, q, l1, l2, form), r, ns, a, q, l1, l2)


@pytest.mark.parametrize("form", ("scan", "boxes"))
def test_ball_then_group_point_round_trip(form):
    """Zero-filled indices keep the existing gather in range: group_point of a ragged idx equals the per-sample result on the
    valid rows (and gathers point 0 on the padded ones)."""
    b, n, m, ns, r, c = 3, 3000, 400, 16, 0.3, 5
    rng, a, q = _qb_data(7, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    feat = rng.randn(b, n, c).astype(np.float32)
    idx, _ = _raw.query_ball_point(r, ns, _cuda(_fill(a, l1, "nan", rng)), _cuda(q), form=form, lengths1=l1, lengths2=l2)
    out = _raw.group_point(_cuda(feat), idx).cpu().numpy()
    for i in range(b):
        ri, _ = _raw.query_ball_point(r, ns, a[i:i + 1, :l1[i]].copy(), q[i:i + 1, :l2[i]].copy())
        exp = _raw.group_point(feat[i:i + 1, :l1[i]].copy(), ri)
        assert _same(out[i, :l2[i]], exp[0]), i
        assert _same(out[i, l2[i]:], np.broadcast_to(feat[i, 0], out[i, l2[i]:].shape)), i


def _graph_replay(call, set_full):
    """Capture `call` (device counts), change the counts, replay: the outputs are those of the new counts."""
    before = [t.clone() for t in call()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm the workspace cache outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    set_full()
    g.replay()
    torch.cuda.synchronize()
    after = call()
    assert all(_same(o, f) for o, f in zip(out, after))
    assert not all(_same(o, e) for o, e in zip(out, before))


@pytest.mark.parametrize("form", ("scan", "boxes"))
def test_ball_graph_capture_with_device_counts(form):
    b, n, m = 4, 3000, 500
    rng, a, q = _qb_data(5, b, n, m)
    ta, tq = _cuda(a), _cuda(q)
    l1, l2 = _cuda(_lengths(rng, b, n)), _cuda(_lengths(rng, b, m))

    def full():
        l1.fill_(n)
        l2.fill_(m)
    _graph_replay(lambda: _raw.query_ball_point(0.3, 16, ta, tq, form=form, lengths1=l1, lengths2=l2), full)


@pytest.mark.parametrize("seed", range(30))
def test_ball_fuzz(orc, seed):
    rng = np.random.RandomState(2000 + seed)
    b = int(rng.randint(1, 4))
    n = int(rng.choice([rng.randint(1, 64), rng.randint(64, 2048), rng.randint(2048, 20000)]))
    m = int(rng.choice([rng.randint(1, 64), rng.randint(64, 1500)]))
    ns = int(rng.choice([1, 3, 32, 64, 70]))
    r = float(rng.choice([1e-21, 0.05, 0.3, 1.0, 50.0]))
    a = rng.randn(b, n, 3).astype(np.float32)
    q = np.where(rng.rand(b, m, 1) < 0.3, a[:, rng.randint(0, n, size=m)], rng.randn(b, m, 3)).astype(np.float32)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    a, q = _fill(a, l1, FILLS[seed % 6], rng), _fill(q, l2, FILLS[(seed // 6) % 6], rng)
    for form in FORMS:
        if form == "boxes" and (n < 64 or ns > 64):
            continue
        _qb_check(_qb(r, ns, a, q, l1, l2, form), r, ns, a, q, l1, l2, orc)


# ------------------------------------------------------------------ sample_and_group ----------------------------------------
@pytest.mark.parametrize("aux", (False, True))
@pytest.mark.parametrize("b,n,m,ns,r", [(3, 999, 128, 32, 0.3), (3, 3000, 512, 16, 0.25), (2, 16384, 1024, 32, 0.1),
                                        (2, 20000, 100, 64, 0.2)])
def test_sample_and_group_equals_the_ragged_ops(aux, b, n, m, ns, r):
    rng = np.random.RandomState(n + m)
    a = rng.randn(b, n, 3).astype(np.float32)
    ln, lo = _lengths(rng, b, n), _lengths(rng, b, m)
    ln[0] = 40  # below the boxed form's minimum, and fewer points than samples
    ta = _cuda(_fill(a, ln, "copies", rng))
    stream = torch.cuda.Stream() if aux else None
    fi, nx, gi, cnt, gx = _raw.sample_and_group(m, r, ns, ta, aux_stream=stream, lengths=_cuda(ln), npoints=_cuda(lo))
    torch.cuda.synchronize()
    efi, enx = _raw.farthest_point_sample(m, ta, lengths=ln, npoints=lo, with_xyz=True)
    egi, ecnt = _raw.query_ball_point(r, ns, ta, enx, form="boxes", lengths1=ln, lengths2=lo)
    assert _same(fi, efi) and _same(nx, enx) and _same(gi, egi) and _same(cnt, ecnt)
    egx = _raw.group_point(ta, egi).cpu().numpy()
    gx = gx.cpu().numpy()
    for i in range(b):
        assert _same(gx[i, :lo[i]], egx[i, :lo[i]]), i
        assert _zeros(gx[i, lo[i]:]) and _zeros(gi[i, lo[i]:]) and _zeros(cnt[i, lo[i]:]) and _zeros(nx[i, lo[i]:]), i
    # ... and the whole chain on each sample alone
    for i in range(b):
        one = _raw.sample_and_group(int(lo[i]), r, ns, a[i:i + 1, :ln[i]].copy()) if ln[i] >= 64 else None
        if one is not None:
            for g, e in zip((fi, nx, gi, cnt, gx), one):
                assert _same(g[i, :lo[i]], e[0]), i
    full = _raw.sample_and_group(m, r, ns, ta, lengths=[n] * b)
    assert all(_same(g, e) for g, e in zip(full, _raw.sample_and_group(m, r, ns, ta)))


# ------------------------------------------------------------------ three_nn ------------------------------------------------
def _tn(a, k, l1, l2, form="auto"):
    return [t.cpu().numpy() for t in _raw.three_nn(_cuda(a), _cuda(k), form=form, lengths1=None if l1 is None else _cuda(l1),
                                                   lengths2=None if l2 is None else _cuda(l2))]


def _tn_check(got, a, k, l1, l2, orc=None):
    dist, idx = got
    for i in range(a.shape[0]):
        n1, n2 = int(l1[i]), int(l2[i])
        ai, ki = a[i:i + 1, :n1].copy(), k[i:i + 1, :n2].copy()
        rd, ri = _raw.three_nn(ai, ki, form="scan")
        assert _same(dist[i, :n1], rd[0]) and _same(idx[i, :n1], ri[0]), ("existing op", i, n1, n2)
        if orc is not None and n1 * n2 <= ORACLE_PAIRS:
            od, oi = orc.three_nn(ai, ki)
            assert _same(dist[i, :n1], od[0]) and _same(idx[i, :n1], oi[0]), ("oracle", i, n1, n2)
        assert ((idx[i, :n1] >= 0) & (idx[i, :n1] < n2)).all(), i
        assert _zeros(dist[i, n1:]) and _zeros(idx[i, n1:]), ("padded rows", i)


def _pair(seed, b, n, m):
    rng = np.random.RandomState(seed)
    return rng, rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


TN_SHAPES = [(3, 1, 1), (3, 70, 2), (3, 999, 301), (2, 2048, 2048), (2, 16384, 1024), (2, 5000, 16384), (1, 65536, 4096)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m", TN_SHAPES)
def test_three_nn_matches_per_sample_slices(orc, form, b, n, m):
    rng, a, k = _pair(n + m, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    _tn_check(_tn(a, k, l1, l2, form), a, k, l1, l2, orc)
    _tn_check(_tn(a, k, None, l2, form), a, k, [n] * b, l2)
    _tn_check(_tn(a, k, l1, None, form), a, k, l1, [m] * b)
    exp = _raw.three_nn(_cuda(a), _cuda(k), form=form)  # full counts: the existing op
    got = _raw.three_nn(_cuda(a), _cuda(k), form=form, lengths1=[n] * b, lengths2=torch.full((b,), m, device="cuda"))
    assert _same(got[0], exp[0]) and _same(got[1], exp[1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m", [(4, 999, 301), (3, 3000, 16384), (2, 8192, 8192)])
def test_three_nn_hostile_padding_changes_nothing(form, b, n, m):
    rng, a, k = _pair(11 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[1], l2[1] = n // 2, m // 3
    clean = _tn(a, k, l1, l2, form)
    for how in FILLS:
        got = _tn(_fill(a, l1, how, rng), _fill(k, l2, how, rng), l1, l2, form)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), how
    if form == "auto":  # the inputs are hostile: the plain op finds neighbours in the moved copies
        plain = _raw.three_nn(a[1:2, :l1[1]].copy(), _fill(k, l2, "nearest", rng)[1:2])[1]
        assert (plain >= l2[1]).any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,m", [(16384, 16384), (65536, 2048)])
def test_three_nn_short_counts_at_large_sizes(orc, form, n, m):
    """Counts of 1, 7 and 64 in large slots, and fewer than three known points: (+inf, 0) in the slots without a neighbour."""
    rng, a, k = _pair(n + 1, 4, n, m)
    l1, l2 = np.array([1, 7, 64, n], np.int32), np.array([64, 1, 2, 7], np.int32)
    got = _tn(a, k, l1, l2, form)
    _tn_check(got, a, k, l1, l2, orc)
    assert np.isinf(got[0][1, :7, 1:]).all() and _zeros(got[1][1, :7, 1:]) and np.isinf(got[0][2, :64, 2]).all()
    for how in ("nan", "copies"):
        bad = _tn(_fill(a, l1, how, rng), _fill(k, l2, how, rng), l1, l2, form)
        assert _same(bad[0], got[0]) and _same(bad[1], got[1]), how


@pytest.mark.parametrize("form", FORMS)
def test_three_nn_non_finite_formats_and_clamping(form):
    b, n, m = 3, 3000, 2500
    rng, a, k = _pair(23, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[0], l2[0] = 9, 9
    a, k = _non_finite(rng, a, l1), _non_finite(rng, k, l2)
    ref = _tn(a, k, l1, l2, form)
    _tn_check(ref, a, k, l1, l2)
    for f in (lambda v: v.tolist(), lambda v: torch.from_numpy(v.astype(np.int64)).cuda(), lambda v: torch.from_numpy(v)):
        got = _raw.three_nn(_cuda(a), _cuda(k), form=form, lengths1=f(l1), lengths2=f(l2))
        assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    bad = _raw.three_nn(_cuda(a), _cuda(k), form=form, lengths1=torch.tensor([0, -7, 10 ** 6], device="cuda", dtype=torch.int32),
                        lengths2=torch.tensor([2 ** 33, 0, 5], device="cuda"))
    ok = _tn(a, k, np.array([1, 1, n], np.int32), np.array([m, 1, 5], np.int32), form)
    assert _same(bad[0], ok[0]) and _same(bad[1], ok[1])


@pytest.mark.parametrize("form", ("scan", "boxes"))
def test_three_nn_then_interpolate_round_trip(form):
    """Zero-filled indices keep the existing interpolation in range: its valid rows equal the per-sample result."""
    b, n, m, c = 3, 2000, 700, 8
    rng, a, k = _pair(9, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l2 = np.maximum(l2, 3)
    feat = rng.randn(b, m, c).astype(np.float32)
    dist, idx = _raw.three_nn(_cuda(_fill(a, l1, "nan", rng)), _cuda(_fill(k, l2, "copies", rng)), form=form, lengths1=l1, lengths2=l2)
    w = torch.softmax(-dist, -1).contiguous()
    out = _raw.three_interpolate(_cuda(feat), idx, w).cpu().numpy()
    for i in range(b):
        di, ii = _raw.three_nn(_cuda(a[i:i + 1, :l1[i]]), _cuda(k[i:i + 1, :l2[i]]))
        exp = _raw.three_interpolate(_cuda(feat[i:i + 1, :l2[i]]), ii, torch.softmax(-di, -1).contiguous())
        assert _same(out[i, :l1[i]], exp[0]), i


@pytest.mark.parametrize("form", ("scan", "boxes"))
def test_three_nn_graph_capture_with_device_counts(form):
    b, n, m = 4, 3000, 1500
    rng, a, k = _pair(5, b, n, m)
    ta, tk = _cuda(a), _cuda(k)
    l1, l2 = _cuda(_lengths(rng, b, n)), _cuda(_lengths(rng, b, m))

    def full():
        l1.fill_(n)
        l2.fill_(m)
    _graph_replay(lambda: _raw.three_nn(ta, tk, form=form, lengths1=l1, lengths2=l2), full)


@pytest.mark.parametrize("seed", range(30))
def test_three_nn_fuzz(orc, seed):
    rng = np.random.RandomState(3000 + seed)
    b = int(rng.randint(1, 4))
    n = int(rng.choice([rng.randint(1, 300), rng.randint(300, 6000), rng.randint(6000, 20000)]))
    m = int(rng.choice([rng.randint(1, 10), rng.randint(10, 3000), rng.randint(3000, 18000)]))
    a = rng.randn(b, n, 3).astype(np.float32)
    k = rng.randn(b, m, 3).astype(np.float32)
    if seed % 4 == 0:  # ties: known points in exact copies, unknown points on top of known ones
        k[:, m // 2:] = k[:, :m - m // 2]
        a[:, ::3] = k[:, rng.randint(0, m, size=len(range(0, n, 3)))]
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    a, k = _fill(a, l1, FILLS[seed % 6], rng), _fill(k, l2, FILLS[(seed // 6) % 6], rng)
    for form in FORMS:
        _tn_check(_tn(a, k, l1, l2, form), a, k, l1, l2, orc)


# ------------------------------------------------------------------ knn_point -----------------------------------------------
def ref_knn(k, xyz1, xyz2, chunk=256):
    """-> val (b,m,k) float32 = -d, idx (b,m,k): d = ((dx*dx)+(dy*dy))+(dz*dz) in float32, dx = x1 - x2; ascending by
    (d, index) with a NaN distance before every number (tests/test_gpu_knn.py, restated)."""
    b, m = xyz2.shape[0], xyz2.shape[1]
    val = np.empty((b, m, k), np.float32)
    idx = np.empty((b, m, k), np.int64)
    for bi in range(b):
        x1 = xyz1[bi]
        for j0 in range(0, m, chunk):
            q = xyz2[bi, j0:j0 + chunk]
            dx = x1[None, :, 0] - q[:, None, 0]
            dy = x1[None, :, 1] - q[:, None, 1]
            dz = x1[None, :, 2] - q[:, None, 2]
            with np.errstate(invalid="ignore", over="ignore"):
                d = (dx * dx + dy * dy) + dz * dz
            key = np.where(np.isnan(d), np.float32(-1), d)
            o = np.argsort(key, axis=1, kind="stable")[:, :k]
            idx[bi, j0:j0 + chunk] = o
            val[bi, j0:j0 + chunk] = -np.take_along_axis(d, o, axis=1)
    return val, idx


def same_val(got, exp):
    """bit-equal for numbers, NaN where NaN"""
    got, exp = np.asarray(got), np.asarray(exp)
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), exp[~nan].view(np.int32))


def _kn(k, a, q, l1, l2, form="auto"):
    return [t.cpu().numpy() for t in _raw.knn_point(k, _cuda(a), _cuda(q), form=form, lengths1=None if l1 is None else _cuda(l1),
                                                    lengths2=None if l2 is None else _cuda(l2))]


def _kn_check(got, k, a, q, l1, l2, numpy_too=True):
    """Valid rows, slots [0, min(k, len1)): the existing op with that k on the slices, and the numpy statement where the
    sample is small enough; zeros behind the neighbours and in the rows of padded queries."""
    val, idx = got
    for i in range(a.shape[0]):
        n1, n2 = int(l1[i]), int(l2[i])
        kv = min(k, n1)
        ai, qi = a[i:i + 1, :n1].copy(), q[i:i + 1, :n2].copy()
        rv, ri = _raw.knn_point(kv, ai, qi, form="scan")
        assert same_val(val[i, :n2, :kv], rv[0]) and _same(idx[i, :n2, :kv], ri[0]), ("existing op", i, n1, n2, kv)
        if numpy_too and n1 * n2 <= 1 << 22:
            ev, ei = ref_knn(kv, ai, qi)
            assert same_val(val[i, :n2, :kv], ev[0]) and np.array_equal(idx[i, :n2, :kv], ei[0]), ("numpy", i, n1, n2, kv)
        assert ((idx[i, :n2, :kv] >= 0) & (idx[i, :n2, :kv] < n1)).all(), i
        assert _zeros(val[i, :n2, kv:]) and _zeros(idx[i, :n2, kv:]), ("behind the neighbours", i)
        assert _zeros(val[i, n2:]) and _zeros(idx[i, n2:]), ("padded rows", i)


KN_SHAPES = [(3, 1, 1, 1), (3, 70, 33, 3), (3, 999, 301, 16), (2, 777, 300, 64), (2, 2048, 2048, 1), (2, 5000, 3000, 16),
             (2, 16384, 8192, 16), (2, 16384, 2048, 64), (1, 65536, 1024, 3)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,k", KN_SHAPES)
def test_knn_matches_per_sample_slices(form, b, n, m, k):
    rng, a, q = _pair(n + m + k, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)  # a count of 1 among them: fewer candidates than k
    _kn_check(_kn(k, a, q, l1, l2, form), k, a, q, l1, l2)
    _kn_check(_kn(k, a, q, None, l2, form), k, a, q, [n] * b, l2, numpy_too=False)
    _kn_check(_kn(k, a, q, l1, None, form), k, a, q, l1, [m] * b, numpy_too=False)
    exp = _raw.knn_point(k, _cuda(a), _cuda(q), form=form)  # full counts: the existing op
    got = _raw.knn_point(k, _cuda(a), _cuda(q), form=form, lengths1=[n] * b, lengths2=torch.full((b,), m, device="cuda"))
    assert same_val(got[0].cpu().numpy(), exp[0].cpu().numpy()) and _same(got[1], exp[1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b,n,m,k", [(4, 999, 301, 16), (3, 3000, 4096, 3), (2, 16384, 8192, 32)])
def test_knn_hostile_padding_changes_nothing(form, b, n, m, k):
    rng, a, q = _pair(11 + n, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[1], l2[1] = n // 2, m // 3
    clean = _kn(k, a, q, l1, l2, form)
    for how in FILLS:
        got = _kn(k, _fill(a, l1, how, rng), _fill(q, l2, how, rng), l1, l2, form)
        assert same_val(got[0], clean[0]) and _same(got[1], clean[1]), how
    if form == "auto":  # the inputs are hostile: a NaN candidate ranks first in the plain op
        plain = _raw.knn_point(k, _fill(a, l1, "nan", rng)[1:2], q[1:2, :l2[1]].copy())[1]
        assert (plain >= l1[1]).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("inf_query", (False, True))
@pytest.mark.parametrize("n,m,k", [(16384, 8192, 16), (65536, 512, 64), (16384, 300, 8)])
def test_knn_short_counts_and_fewer_candidates_than_k(form, inf_query, n, m, k):
    """len1 = 1, 7 (< k) and 64 in large slots: the lists cannot fill, and what they start with must not go out -- with a
    query that has an infinite coordinate too (the boxed form then visits every superblock, padding records included)."""
    rng, a, q = _pair(n + k, 4, n, m)
    l1, l2 = np.array([1, 7, 64, n], np.int32), np.array([m, 64, 7, 1], np.int32)
    if inf_query:
        q[:, 0, 0] = np.inf
        q[:, 3, 1] = -np.inf
        q[1, 5, 2] = np.nan
    got = _kn(k, a, q, l1, l2, form)
    _kn_check(got, k, a, q, l1, l2)
    for how in ("nan", "copies"):
        bad = _kn(k, _fill(a, l1, how, rng), _fill(q, l2, how, rng), l1, l2, form)
        assert same_val(bad[0], got[0]) and _same(bad[1], got[1]), how


@pytest.mark.parametrize("form", FORMS)
def test_knn_non_finite_formats_and_clamping(form):
    b, n, m, k = 3, 3000, 2500, 8
    rng, a, q = _pair(23, b, n, m)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[0], l2[0] = 9, 9
    a, q = _non_finite(rng, a, l1), _non_finite(rng, q, l2)
    ref = _kn(k, a, q, l1, l2, form)
    _kn_check(ref, k, a, q, l1, l2)
    for f in (lambda v: v.tolist(), lambda v: torch.from_numpy(v.astype(np.int64)).cuda(), lambda v: torch.from_numpy(v)):
        got = _raw.knn_point(k, _cuda(a), _cuda(q), form=form, lengths1=f(l1), lengths2=f(l2))
        assert same_val(got[0].cpu().numpy(), ref[0]) and _same(got[1], ref[1])
    bad = _raw.knn_point(k, _cuda(a), _cuda(q), form=form, lengths1=torch.tensor([0, -7, 10 ** 6], device="cuda", dtype=torch.int32),
                         lengths2=torch.tensor([2 ** 33, 0, 5], device="cuda"))
    ok = _kn(k, a, q, np.array([1, 1, n], np.int32), np.array([m, 1, 5], np.int32), form)
    assert same_val(bad[0].cpu().numpy(), ok[0]) and _same(bad[1], ok[1])


@pytest.mark.parametrize("form", ("scan", "boxes"))
def test_knn_graph_capture_with_device_counts(form):
    b, n, m, k = 4, 3000, 1500, 8
    rng, a, q = _pair(5, b, n, m)
    ta, tq = _cuda(a), _cuda(q)
    l1, l2 = _cuda(_lengths(rng, b, n)), _cuda(_lengths(rng, b, m))

    def full():
        l1.fill_(n)
        l2.fill_(m)
    _graph_replay(lambda: _raw.knn_point(k, ta, tq, form=form, lengths1=l1, lengths2=l2), full)


@pytest.mark.parametrize("seed", range(30))
def test_knn_fuzz(seed):
    rng = np.random.RandomState(4000 + seed)
    b = int(rng.randint(1, 4))
    n = int(rng.choice([rng.randint(1, 300), rng.randint(300, 6000), rng.randint(6000, 20000)]))
    m = int(rng.choice([rng.randint(1, 10), rng.randint(10, 2000), rng.randint(2000, 9000)]))
    k = int(min(n, rng.choice([1, 3, 16, 64, rng.randint(1, 65)])))
    a = rng.randn(b, n, 3).astype(np.float32)
    q = rng.randn(b, m, 3).astype(np.float32)
    if seed % 4 == 0:  # ties
        a[:, n // 2:] = a[:, :n - n // 2]
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    a, q = _fill(a, l1, FILLS[seed % 6], rng), _fill(q, l2, FILLS[(seed // 6) % 6], rng)
    for form in FORMS:
        _kn_check(_kn(k, a, q, l1, l2, form), k, a, q, l1, l2)


# ---- knn_point's gradient
def np_grads(x1, x2, idx, g):
    """tests/test_gpu_knn.py's float64 statement of the gradient, restated."""
    x1, x2, g = x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64)
    g1, g2 = np.zeros_like(x1), np.zeros_like(x2)
    b, m, k = idx.shape
    for bi in range(b):
        nb = x1[bi][idx[bi]]  # (m, k, 3)
        term = 2 * g[bi][..., None] * (nb - x2[bi][:, None, :])
        g2[bi] = term.sum(1)
        np.add.at(g1[bi], idx[bi].reshape(-1), -term.reshape(-1, 3))
    return g1, g2


@pytest.mark.parametrize("form", ("scan", "boxes"))
@pytest.mark.parametrize("b,n,m,k", [(3, 3000, 500, 16), (3, 400, 1000, 33), (2, 20000, 4096, 8)])
def test_knn_gradients(form, b, n, m, k):
    from tf_ops.grouping.tf_grouping import knn_point
    rng = np.random.RandomState(b + n + k)
    a = rng.rand(b, n, 3).astype(np.float32)
    q = rng.rand(b, m, 3).astype(np.float32)
    l1, l2 = _lengths(rng, b, n), _lengths(rng, b, m)
    l1[1] = k - 1  # fewer candidates than k
    g = rng.randn(b, m, k).astype(np.float32)  # non-zero in the padded slots too
    a, q = _fill(a, l1, "nan", rng), _fill(q, l2, "1e30", rng)  # nothing of the padding may reach a valid row
    t1, t2 = _cuda(a).requires_grad_(True), _cuda(q).requires_grad_(True)
    v, i = knn_point(k, t1, t2, lengths1=_cuda(l1), lengths2=l2.tolist(), form=form)
    v.backward(_cuda(g))
    g1, g2 = t1.grad.cpu().numpy(), t2.grad.cpu().numpy()
    i = i.cpu().numpy()
    for s in range(b):
        n1, n2, kv = int(l1[s]), int(l2[s]), min(k, int(l1[s]))
        ai, qi, gi = a[s:s + 1, :n1], q[s:s + 1, :n2], g[s:s + 1, :n2, :kv]
        e1, e2 = np_grads(ai, qi, i[s:s + 1, :n2, :kv], gi)
        assert np.allclose(g1[s, :n1], e1[0], rtol=1e-5, atol=1e-6) and np.allclose(g2[s, :n2], e2[0], rtol=1e-5, atol=1e-6), s
        assert _zeros(g1[s, n1:]) and _zeros(g2[s, n2:]), ("padded rows: exactly +0", s)
        # ... and a per-sample call of the existing gradient
        o1, o2 = _raw.knn_point_grad(ai.copy(), qi.copy(), i[s:s + 1, :n2, :kv].copy(), gi.copy())
        assert np.allclose(g1[s, :n1], o1[0], rtol=1e-5, atol=1e-6) and np.allclose(g2[s, :n2], o2[0], rtol=1e-5, atol=1e-6), s
    # garbage in the padded slots of idx and grad_val changes nothing
    junk_i, junk_g = i.copy(), g.copy()
    for s in range(b):
        junk_i[s, l2[s]:] = rng.randint(-5, n + 5, size=junk_i[s, l2[s]:].shape)
        junk_i[s, :, min(k, l1[s]):] = rng.randint(-5, n + 5, size=junk_i[s, :, min(k, l1[s]):].shape)
        junk_g[s, l2[s]:] = np.nan
    j1, j2 = _raw.knn_point_grad(_cuda(a), _cuda(q), _cuda(junk_i.astype(np.int32)), _cuda(junk_g), lengths1=l1, lengths2=l2)
    assert _same(j1, g1) and _same(j2, g2)
