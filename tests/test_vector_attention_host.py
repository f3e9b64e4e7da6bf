"""CPU: the vector attention pair (include/rfops.h, "the vector attention pair") at the boundary -- declared, exported, bound; the
workspace sizes; every argument rule answered before a device is touched; the wrappers' checks -- and sub_ref, sub_grad_ref,
agg_ref, agg_grad_ref, the numpy restatements of the contract that the GPU tests hold the kernels to (float32 where the contract
says fp32, float64 with the contract's roundings for the sums; the order-free sums as a plain float64 sum in slot order, reversed,
and as the correctly rounded exact sum by math.fsum), pinned here by independent means: a case by hand with a dead slot of each of
the three kinds, a float64 einsum formula, and the adjoint identities of both ops."""
import ctypes

import numpy as np
import pytest

from test_point_voxel_host import _scatter

F32, F64, I32, I64, U32 = np.float32, np.float64, np.int32, np.int64, np.uint32
MAX_K, MAX_CHANNELS = 64, 1024


# ---- the references -----------------------------------------------------------------------------------------------------
def _clamp(L, n):
    return n if L is None else min(max(int(L), 1), n)


def live_mask(idx, n, L1=None, L2=None):
    """idx (m, k) -> (m, k) bool: i < len2', t < len1', 0 <= idx < len1'"""
    idx = np.asarray(idx)
    m, k = idx.shape
    nv, mv = _clamp(L1, n), _clamp(L2, m)
    return (np.arange(m)[:, None] < mv) & (np.arange(k)[None, :] < nv) & (idx >= 0) & (idx < nv)


def _rows(idx, lv):
    return np.where(lv, idx, 0).astype(I64)


def sub_ref(q, src, idx, L1=None, L2=None):
    """q (m, c), src (n, c), idx (m, k) -> (m, k, c) float32: one fp32 subtraction per element of a live slot, +0 elsewhere"""
    q, src = np.asarray(q, F32), np.asarray(src, F32)
    lv = live_mask(idx, src.shape[0], L1, L2)
    with np.errstate(invalid="ignore", over="ignore"):
        out = q[:, None, :] - src[_rows(idx, lv)]
    return np.where(lv[:, :, None], out, F32(0)).astype(F32)


def va_tol(G, A, K):
    """the header's 2^-23 |exact| + K 2^-52 sum |terms|, less 2^-52 |exact| for what fsum leaves"""
    return (2.0 ** -23 - 2.0 ** -52) * np.abs(G) + K[:, None] * 2.0 ** -52 * A


def sub_grad_ref(idx, g, n, L1=None, L2=None, fsum=False, reverse=False):
    """idx (m, k), g (m, k, c) -> (grad_q (m, c) float32; GS (n, c) float64: grad_src before its rounding to float32, A: the sums
    of the terms' magnitudes, K (n,): the number of terms per row).  GS is the plain double sum of the terms -(double)g in slot
    order (reversed on request), with `fsum` their correctly rounded exact sum."""
    g = np.asarray(g, F32)
    m, k, c = g.shape
    lv = live_mask(idx, n, L1, L2)
    acc = np.zeros((m, c), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k):  # ascending, from +0.0: a dead slot adds +0.0
            acc = acc + np.where(lv[:, t, None], g[:, t].astype(F64), 0.0)
        gq = acc.astype(F32)
        GS, A, K = _scatter(np.asarray(idx)[lv].astype(I64), -g[lv].astype(F64), n, fsum, reverse)
    return gq, GS, A, K


def _s(value, idx, lv, pos):
    """s = fl32(value[idx] + pos) (m, k, c) float32; whatever it holds in dead slots is dropped by the callers"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(value, F32)[_rows(idx, lv)]
        return s if pos is None else (s + np.asarray(pos, F32)).astype(F32)


def agg_ref(value, weight, idx, pos=None, L1=None, L2=None, raw=False):
    """value (n, c), weight (m, k, cw), idx (m, k), pos (m, k, c) or None -> (m, c) float32 (raw: float64 before the rounding)"""
    value, weight = np.asarray(value, F32), np.asarray(weight, F32)
    (n, c), (m, k, cw) = value.shape, weight.shape
    lv = live_mask(idx, n, L1, L2)
    s, chw = _s(value, idx, lv, pos), np.arange(c) % cw
    acc = np.zeros((m, c), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k):  # ascending, from +0.0; the product of two float32 values is exact in float64
            acc = acc + np.where(lv[:, t, None], s[:, t].astype(F64) * weight[:, t][:, chw].astype(F64), 0.0)
        return acc if raw else acc.astype(F32)


def agg_grad_ref(value, weight, idx, g, pos=None, L1=None, L2=None, fsum=False, reverse=False):
    """g (m, c) -> (GV (n, c) float64: grad_value before its rounding, A, K as sub_grad_ref's; grad_pos (m, k, c) float32;
    grad_weight (m, k, cw) float32)"""
    value, weight, g = np.asarray(value, F32), np.asarray(weight, F32), np.asarray(g, F32)
    (n, c), (m, k, cw) = value.shape, weight.shape
    lv = live_mask(idx, n, L1, L2)
    s, chw = _s(value, idx, lv, pos), np.arange(c) % cw
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        gp = np.where(lv[:, :, None], g[:, None, :] * weight[:, :, chw], F32(0)).astype(F32)  # one fp32 product
        acc = np.zeros((m, k, cw), F64)
        for q in range(c // cw):  # ascending, from +0.0
            acc = acc + g[:, None, q * cw:(q + 1) * cw].astype(F64) * s[:, :, q * cw:(q + 1) * cw].astype(F64)
        gw = np.where(lv[:, :, None], acc, 0.0).astype(F32)
        qi = np.nonzero(lv)[0]
        terms = g[qi].astype(F64) * weight[lv][:, chw].astype(F64)
        GV, A, K = _scatter(np.asarray(idx)[lv].astype(I64), terms, n, fsum, reverse)
    return GV, A, K, gp, gw


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------------
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def indices(kind, seed, m, k, n):
    """idx (m, k) int32: "random"; "identity" (slot t of query i names (i + t) mod n); "hub" (every slot names one row); "perm"
    (every row named about m k / n times: a permutation of the slots' round-robin); "hostile" (random with -1, n, INT_MIN and
    INT_MAX sprinkled in)"""
    rng = np.random.RandomState(seed)
    if kind == "identity":
        return ((np.arange(m)[:, None] + np.arange(k)[None, :]) % n).astype(I32)
    if kind == "hub":
        return np.full((m, k), rng.randint(0, n), I32)
    if kind == "perm":
        return rng.permutation(np.arange(m * k) % n).reshape(m, k).astype(I32)
    idx = rng.randint(0, n, (m, k)).astype(I64)
    if kind == "hostile":
        pick = rng.rand(m, k)
        for j, v in enumerate((-1, n, INT_MIN, INT_MAX)):
            idx = np.where((pick >= 0.08 * j) & (pick < 0.08 * (j + 1)), v, idx)
    else:
        assert kind == "random", kind
    return idx.astype(I32)


def wide(seed, *shape):
    """random finite float32 of wide dynamic range, -0.0, +0.0 and denormals among them"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(*shape) * np.exp(3 * rng.randn(*shape))).astype(F32)
    pick = rng.rand(*shape)
    x = np.where(pick < 0.05, F32(-0.0), x)
    x = np.where((pick >= 0.05) & (pick < 0.1), F32(0.0), x)
    x = np.where((pick >= 0.1) & (pick < 0.15), (x * F32(1e-40)).astype(F32), x)
    return np.ascontiguousarray(x, F32)


def normal(seed, *shape):
    """random float32 over a few decades, all of it far inside float32's normal range: sums of products of such values stay
    there too, which is where the header's bar for the order-free sums holds"""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(rng.randn(*shape) * np.exp(rng.randn(*shape)), F32)


def ints(seed, *shape):
    """integer-valued float32 in [-64, 64]: products are at most 4096 and every sum of the tests stays far below 2^53"""
    return np.random.RandomState(seed).randint(-64, 65, shape).astype(F32)


# ---- pinned ---------------------------------------------------------------------------------------------------------------
def test_by_hand():
    """n = 3 rows, m = 3 queries, k = 3 slots, c = 2, cw = 1, len1 = 2, len2 = 2.  Dead: query 2 (behind len2), slot t = 2 of every
    query (t >= len1), the slot naming row 2 (>= len1) and the slot naming -1.  NaN sits in everything dead."""
    nan = float("nan")
    src = np.array([[1, 2], [10, 20], [nan, nan]], F32)
    q = np.array([[100, 200], [300, 400], [nan, nan]], F32)
    idx = np.array([[1, 0, 0], [2, 1, 1], [0, 0, 0]], I32)
    lv = live_mask(idx, 3, 2, 2)
    assert lv.tolist() == [[True, True, False], [False, True, False], [False, False, False]]
    assert live_mask(np.array([[-1, 0]], I32), 3).tolist() == [[False, True]]
    assert live_mask(np.array([[INT_MIN, 3, 2], [INT_MAX, 0, 1]], I32), 3).tolist() == [[False, False, True], [False, True, True]]
    assert live_mask(np.zeros((2, 2), I32), 3, L1=0, L2=-5).tolist() == [[True, False], [False, False]]  # counts clamp to 1
    sub = sub_ref(q, src, idx, 2, 2)
    assert sub.tolist() == [[[90, 180], [99, 198], [0, 0]], [[0, 0], [290, 380], [0, 0]], [[0, 0]] * 3]
    assert not sub[~lv].view(U32).any()
    g = np.array([[[1, 2], [4, 8], [nan, nan]], [[nan, nan], [16, 32], [nan, nan]], [[nan, nan]] * 3], F32)
    gq, GS, A, K = sub_grad_ref(idx, g, 3, 2, 2)
    assert gq.tolist() == [[5, 10], [16, 32], [0, 0]] and not gq[2].view(U32).any()
    assert GS.tolist() == [[-4, -8], [-17, -34], [0, 0]] and K.tolist() == [1, 2, 0] and A.tolist() == [[4, 8], [17, 34], [0, 0]]
    assert not GS[2].view(np.uint64).any()
    # the aggregation: weight one channel wide, shared by both channels
    w = np.array([[[2], [3], [nan]], [[nan], [0.5], [nan]], [[nan]] * 3], F32)
    pos = np.array([[[1, 1], [0, 0], [nan, nan]], [[nan, nan], [2, 4], [nan, nan]], [[nan, nan]] * 3], F32)
    out = agg_ref(src, w, idx, pos, 2, 2)
    assert out.tolist() == [[(10 + 1) * 2 + 1 * 3, (20 + 1) * 2 + 2 * 3], [(10 + 2) * 0.5, (20 + 4) * 0.5], [0, 0]]
    assert agg_ref(src, w, idx, None, 2, 2).tolist() == [[23, 46], [5, 10], [0, 0]]
    go = np.array([[1, 10], [2, 20], [nan, nan]], F32)
    GV, A, K, gp, gw = agg_grad_ref(src, w, idx, go, pos, 2, 2)
    assert gp.tolist() == [[[2, 20], [3, 30], [0, 0]], [[0, 0], [1, 10], [0, 0]], [[0, 0]] * 3]
    assert gw.tolist() == [[[1 * 11 + 10 * 21], [1 * 1 + 10 * 2], [0]], [[0], [2 * 12 + 20 * 24], [0]], [[0]] * 3]
    assert GV.tolist() == [[3, 30], [2 + 1, 20 + 10], [0, 0]] and K.tolist() == [1, 2, 0]
    assert not gp[~lv].view(U32).any() and not gw[~lv].view(U32).any()
    # the sum of negated terms: an exact zero is +0.0, and so is the negation of a lone -0.0 ... +0.0 pair
    gz = np.array([[[1.0], [-1.0]]], F32)
    assert not sub_grad_ref(np.zeros((1, 2), I32), gz, 2)[1].view(np.uint64).any()
    assert not sub_grad_ref(np.zeros((1, 1), I32), np.array([[[0.0]]], F32), 1)[1].view(np.uint64).any()
    # cw = c: every channel its own weight; cw = 1 < c: the weight shared
    v2, i2 = np.array([[1, 2, 3, 4]], F32), np.zeros((1, 1), I32)
    assert agg_ref(v2, np.array([[[1, 10, 100, 1000]]], F32), i2).tolist() == [[1, 20, 300, 4000]]
    assert agg_ref(v2, np.array([[[1, 10]]], F32), i2).tolist() == [[1, 20, 3, 40]]  # ch mod cw
    assert agg_grad_ref(v2, np.array([[[1, 10]]], F32), i2, np.array([[1, 1, 2, 2]], F32))[4].tolist() == [[[1 + 6, 2 + 8]]]


CASES = [(1, 1, 1, 1, 1), (7, 5, 3, 4, 2), (33, 20, 16, 12, 3), (9, 40, 5, 8, 8), (65, 17, 17, 6, 1)]  # n, m, k, c, cw


@pytest.mark.parametrize("kind", ["random", "identity", "hub", "perm", "hostile"])
@pytest.mark.parametrize("n,m,k,c,cw", CASES)
def test_refs_against_the_float64_einsum(kind, n, m, k, c, cw):
    """the formulas of the issue in float64 with 0 / 1 masks: the contract's fp32 roundings stay within a few 2^-24 of the terms"""
    rng = np.random.RandomState(n)
    idx = indices(kind, n, m, k, n)
    for L1, L2 in ((None, None), (1, m), (max(n // 2, 1), max(m // 2, 1))):
        lv = live_mask(idx, n, L1, L2).astype(F64)
        r = _rows(idx, lv > 0)
        q, src, v = rng.randn(m, c).astype(F32), rng.randn(n, c).astype(F32), rng.randn(n, c).astype(F32)
        pos, w = rng.randn(m, k, c).astype(F32), rng.randn(m, k, cw).astype(F32)
        wx = np.tile(w.astype(F64), (1, 1, c // cw))
        sub = (q.astype(F64)[:, None] - src.astype(F64)[r]) * lv[:, :, None]
        assert np.abs(sub_ref(q, src, idx, L1, L2) - sub).max() <= 2.0 ** -23 * 8
        for p in (pos, None):
            s64 = v.astype(F64)[r] + (0 if p is None else p.astype(F64))
            out = np.einsum("mkc,mkc,mk->mc", s64, wx, lv)
            mag = np.einsum("mkc,mkc,mk->mc", np.abs(s64), np.abs(wx), lv)
            assert (np.abs(agg_ref(v, w, idx, p, L1, L2, raw=True) - out) <= 2.0 ** -22 * mag + 1e-300).all()
            g = rng.randn(m, c).astype(F32)
            GV, A, K, gp, gw = agg_grad_ref(v, w, idx, g, p, L1, L2, fsum=True)
            e_gp = g.astype(F64)[:, None] * wx * lv[:, :, None]
            assert (np.abs(gp - e_gp) <= 2.0 ** -23 * np.abs(e_gp) + 1e-44).all()
            e_gw = np.einsum("mc,mkc,mk->mkc", g.astype(F64), s64, lv).reshape(m, k, c // cw, cw).sum(2)
            m_gw = np.einsum("mc,mkc,mk->mkc", np.abs(g).astype(F64), np.abs(s64), lv).reshape(m, k, c // cw, cw).sum(2)
            assert (np.abs(gw - e_gw) <= 2.0 ** -21 * m_gw + 1e-44).all()
            e_gv = np.zeros((n, c), F64)
            np.add.at(e_gv, r.ravel(), (e_gp).reshape(-1, c))  # dead slots add their masked zeros to row 0
            assert (np.abs(GV - e_gv) <= 1e-12 * A + 1e-300).all() and K.sum() == lv.sum()


@pytest.mark.parametrize("kind", ["random", "identity", "hub", "perm", "hostile"])
@pytest.mark.parametrize("n,m,k,c,cw", CASES)
def test_adjoint_identities(kind, n, m, k, c, cw):
    """the aggregation is bilinear: <out, g> = <weight, grad_weight> = <value, grad_value> + <pos, grad_pos>; the subtraction is
    linear: <sub, g> = <q, grad_q> + <src, grad_src>.  To double rounding (and the float32 roundings of s, grad_pos, grad_weight,
    grad_q) on random data, exactly on integer data, where nothing rounds."""
    idx = indices(kind, 10 + n, m, k, n)
    for L1, L2 in ((None, None), (1, m), (max(n // 2, 1), max(m // 2, 1))):
        for exact in (False, True):
            gen = ints if exact else (lambda s, *sh: np.random.RandomState(s).randn(*sh).astype(F32))
            q, src, v = gen(1, m, c), gen(2, n, c), gen(3, n, c)
            pos, w, g, gs = gen(4, m, k, c), gen(5, m, k, cw), gen(6, m, c), gen(7, m, k, c)
            d = lambda a, b_: float((np.asarray(a, F64) * np.asarray(b_, F64)).sum())  # noqa: E731
            lv = live_mask(idx, n, L1, L2)
            r, wx = _rows(idx, lv), np.tile(np.abs(w), (1, 1, c // cw))
            gq, GS, A, K = sub_grad_ref(idx, gs, n, L1, L2, fsum=True)
            lhs, rhs = d(sub_ref(q, src, idx, L1, L2), gs), d(q, gq) + d(src, GS)
            scale = d((np.abs(q)[:, None] + np.abs(src)[r]) * lv[:, :, None], np.abs(gs)) + 1e-300
            assert lhs == rhs if exact else abs(lhs - rhs) <= 2.0 ** -20 * scale
            out = agg_ref(v, w, idx, pos, L1, L2, raw=True)
            GV, A, K, gp, gw = agg_grad_ref(v, w, idx, g, pos, L1, L2, fsum=True)
            a1, a2, a3 = d(out, g), d(w, gw), d(v, GV) + d(pos, gp)
            scale = d((np.abs(v)[r] + np.abs(pos)) * wx * lv[:, :, None], np.abs(g)[:, None]) + 1e-300
            if exact:
                assert a1 == a2 == a3
            else:
                assert abs(a1 - a2) <= 2.0 ** -20 * scale and abs(a1 - a3) <= 2.0 ** -20 * scale
            out0 = agg_ref(v, w, idx, None, L1, L2, raw=True)
            GV0, _, _, _, gw0 = agg_grad_ref(v, w, idx, g, None, L1, L2, fsum=True)
            if exact:
                assert d(out0, g) == d(w, gw0) == d(v, GV0) and GV0.tobytes() == GV.tobytes()


def test_sums_by_fsum_and_in_two_orders():
    """the three forms of the order-free sums agree bit for bit where the sums are exact, and fsum is the exact one where not"""
    n, m, k, c, cw = 9, 40, 5, 8, 4
    for kind in ("random", "hub", "hostile"):
        idx = indices(kind, 3, m, k, n)
        g3, g2, v, w = ints(1, m, k, c), ints(2, m, c), ints(3, n, c), ints(4, m, k, cw)
        forms = ((False, False), (False, True), (True, False))
        a, b_, c_ = (sub_grad_ref(idx, g3, n, 5, 30, fsum=f, reverse=r)[1] for f, r in forms)
        assert a.tobytes() == b_.tobytes() == c_.tobytes()
        a, b_, c_ = (agg_grad_ref(v, w, idx, g2, None, 5, 30, fsum=f, reverse=r)[0] for f, r in forms)
        assert a.tobytes() == b_.tobytes() == c_.tobytes() and (kind == "hub" or np.abs(a).max() > 0)
    big = np.array([[[1e16], [1.0], [-1e16], [1.0]]], F32)
    z = np.zeros((1, 4), I32)  # (n = 4: a slot t is live only below the row count)
    assert sub_grad_ref(z, big, 4, fsum=True)[1][0].tolist() == [-2.0] and sub_grad_ref(z, big, 4)[1][0].tolist() != [-2.0]
    GS, A, K = sub_grad_ref(z, big, 4, fsum=True)[1:]
    assert K.tolist() == [4, 0, 0, 0] and abs(sub_grad_ref(z, big, 4)[1][0, 0] - GS[0, 0]) <= va_tol(GS, A, K)[0, 0]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_neighbor_sub", "rf_neighbor_sub_grad", "rf_neighbor_sub_grad_workspace_bytes", "rf_neighbor_aggregate",
           "rf_neighbor_aggregate_grad", "rf_neighbor_aggregate_grad_workspace_bytes")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw, glue
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    assert (_raw.VA_MAX_K, _raw.VA_MAX_CHANNELS, _raw.KNN_MAX_K) == (MAX_K, MAX_CHANNELS, MAX_K)
    hdr = open(_lib._PKG + "/../include/rfops.h").read()
    assert f"#define RF_VA_MAX_K {MAX_K}\n" in hdr and f"#define RF_VA_MAX_CHANNELS {MAX_CHANNELS}\n" in hdr
    for name in ("neighbor_subtraction", "neighbor_subtraction_grad", "neighbor_aggregation", "neighbor_aggregation_grad"):
        assert callable(getattr(_raw, name))
    assert callable(glue.neighbor_subtraction) and callable(glue.neighbor_aggregation)


def test_workspace_sizes():
    """rows_csr_workspace_bytes(b, n, m k) and nothing more: 4 b (n + 1) + 4 b m k, each part rounded up to 256 bytes"""
    from rfnet_amd._lib import lib
    for f in (lib.rf_neighbor_sub_grad_workspace_bytes, lib.rf_neighbor_aggregate_grad_workspace_bytes):
        for shape in ((0, 10, 10, 4), (-1, 10, 10, 4), (65536, 10, 10, 4), (2, 0, 10, 4), (2, 65537, 10, 4), (2, 10, 0, 4),
                      (2, 10, 65537, 4), (2, 10, 10, 0), (2, 10, 10, 65), (2, 10, 10, -1), (2, -10, 10, 4)):
            assert f(*shape) == 0, shape
        r = lambda v: (v + 255) // 256 * 256  # noqa: E731
        for b, n, m, k in ((1, 1, 1, 1), (3, 257, 65, 17), (32, 2048, 2048, 16), (2, 10, 10, 64), (65535, 65536, 65536, 64)):
            assert f(b, n, m, k) == r(4 * b * (n + 1)) + r(4 * b * m * k), (b, n, m, k)


P, WS, BIG = 0x10000, 0x200000, 1 << 60  # never dereferenced: every call below must return at its argument checks


def _t(k, null, at):
    t = [P] * k
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return t


def _sub(b=2, n=30, m=20, k=4, c=8, l1=P, l2=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # feat_q, feat_src, idx, out
    return lib.rf_neighbor_sub(b, n, m, k, c, t[0], t[1], t[2], l1, l2, t[3], None)


def _sub_grad(b=2, n=30, m=20, k=4, c=8, l1=P, l2=P, gq=P, gs=P, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(2, null, at)  # idx, grad_out
    return lib.rf_neighbor_sub_grad(b, n, m, k, c, t[0], l1, l2, t[1], gq, gs, ws, wsz, None)


def _agg(b=2, n=30, m=20, k=4, c=8, cw=4, l1=P, l2=P, pos=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # value, weight, idx, out
    return lib.rf_neighbor_aggregate(b, n, m, k, c, cw, t[0], pos, t[1], t[2], l1, l2, t[3], None)


def _agg_grad(b=2, n=30, m=20, k=4, c=8, cw=4, l1=P, l2=P, pos=P, gv=P, gp=P, gw=P, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # value, weight, idx, grad_out
    return lib.rf_neighbor_aggregate_grad(b, n, m, k, c, cw, t[0], pos, t[1], t[2], l1, l2, t[3], gv, gp, gw, ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    bad_sizes = (dict(b=-1), dict(b=65536), dict(n=0), dict(n=-3), dict(n=65537), dict(m=0), dict(m=-1), dict(m=65537), dict(k=0),
                 dict(k=65), dict(k=-1), dict(c=0), dict(c=1025), dict(c=-4), dict(b=0, n=-1), dict(b=0, k=-1), dict(b=0, c=-1),
                 dict(m=65536, k=64, c=512), dict(m=65536, k=64, c=1024), dict(m=32768, k=64, c=1024))  # m k c = 2^31, 2^32, 2^31
    calls = ((_sub, 4), (_sub_grad, 2), (_agg, 4), (_agg_grad, 4))
    for f, k in calls:
        assert f(b=0) == OK and f(b=0, n=0, m=0, k=0, c=0) == OK
        for bad in bad_sizes:
            assert f(**bad) == EINVAL, (f.__name__, bad)
        for j in range(k):
            assert f(null=j) == EINVAL and f(at=(j, P + 2)) == EINVAL and f(at=(j, P + 1)) == EINVAL, (f.__name__, j)
        for ln in ("l1", "l2"):
            assert f(**{ln: P + 2}) == EINVAL and f(**{ln: P + 1}) == EINVAL, f.__name__
    for f in (_agg, _agg_grad):
        for bad in (dict(cw=0), dict(cw=-1), dict(cw=3), dict(cw=16), dict(c=8, cw=5), dict(b=0, cw=-1), dict(pos=P + 2), dict(pos=P + 1)):
            assert f(**bad) == EINVAL, (f.__name__, bad)
    # the optional outputs: misaligned is an error, NULL is "not wanted"
    for out in ("gq", "gs"):
        assert _sub_grad(**{out: P + 2}) == EINVAL
    for out in ("gv", "gp", "gw"):
        assert _agg_grad(**{out: P + 1}) == EINVAL
    assert _sub_grad(b=0, ws=None, wsz=0, gq=None, gs=None) == OK and _agg_grad(b=0, ws=None, wsz=0) == OK
    # nothing wanted: nothing to do (no workspace is looked at, no launch is made)
    assert _sub_grad(gq=None, gs=None, ws=None, wsz=0) == OK and _agg_grad(gv=None, gp=None, gw=None, ws=None, wsz=0) == OK
    for f, need in ((_sub_grad, lib.rf_neighbor_sub_grad_workspace_bytes(2, 30, 20, 4)),
                    (_agg_grad, lib.rf_neighbor_aggregate_grad_workspace_bytes(2, 30, 20, 4))):
        assert f(ws=None) == EINVAL and f(ws=WS + 8) == EINVAL and f(ws=WS + 4) == EINVAL
        assert need > 0 and f(wsz=need - 1) == EWORKSPACE and f(wsz=0, l1=None, l2=None) == EWORKSPACE
        assert f(b=65535, n=65536, m=65536, k=32, c=4, wsz=0) == EWORKSPACE  # the largest sizes are sizes
        assert f(m=65536, k=64, c=508, wsz=0) == EWORKSPACE and f(n=65536, c=1024, k=1, wsz=0) == EWORKSPACE  # just below 2^31
        assert f(k=64, wsz=0) == EWORKSPACE and f(k=1, wsz=0) == EWORKSPACE
    assert _agg_grad(pos=None, wsz=0) == EWORKSPACE and _agg_grad(c=1024, cw=1, wsz=0) == EWORKSPACE
    assert _agg_grad(c=1024, cw=1024, wsz=0) == EWORKSPACE and _agg_grad(c=8, cw=8, wsz=0) == EWORKSPACE


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    b, n, m, k, c, cw = 2, 6, 5, 3, 8, 4
    q, src = np.zeros((b, m, c), F32), np.zeros((b, n, c), F32)
    idx, pos, w = np.zeros((b, m, k), I32), np.zeros((b, m, k, c), F32), np.zeros((b, m, k, cw), F32)
    g4, g3 = np.zeros((b, m, k, c), F32), np.zeros((b, m, c), F32)
    calls = {
        "neighbor_subtraction": lambda **a: _raw.neighbor_subtraction(a.pop("q", q), a.pop("src", src), a.pop("idx", idx), **a),
        "neighbor_subtraction_grad": lambda **a: _raw.neighbor_subtraction_grad(a.pop("idx", idx), a.pop("g", g4), a.pop("n", n), **a),
        "neighbor_aggregation": lambda **a: _raw.neighbor_aggregation(a.pop("v", src), a.pop("w", w), a.pop("idx", idx),
                                                                      a.pop("pos", pos), **a),
        "neighbor_aggregation_grad": lambda **a: _raw.neighbor_aggregation_grad(a.pop("v", src), a.pop("w", w), a.pop("idx", idx),
                                                                                a.pop("g", g3), a.pop("pos", pos), **a),
    }
    for name, call in calls.items():
        for bad in (np.zeros((b, m), I32), np.zeros((b, m, k, 1), I32)):
            with pytest.raises(ValueError, match=name + r" requires idx be of shape \(batch,#queries,k\)"):
                call(idx=bad)
        for bad in (np.zeros((b, m, 0), I32), np.zeros((b, m, 65), I32)):
            with pytest.raises(ValueError, match=name + " takes 1 to 64 neighbours"):
                call(idx=bad)
        with pytest.raises(ValueError, match="1 to 65536 queries"):
            call(idx=np.zeros((b, 0, k), I32))
        for ln, hi in (("lengths1", n), ("lengths2", m)):
            for bad in ([0, 1], [1, hi + 1], [1], [1.5, 2.0]):
                with pytest.raises(ValueError, match=ln):
                    call(**{ln: bad})
    sub, sgr, agg, agr = (calls[k_] for k_ in ("neighbor_subtraction", "neighbor_subtraction_grad", "neighbor_aggregation",
                                               "neighbor_aggregation_grad"))
    for bad in (np.zeros((b, m), F32), np.zeros((b, m + 1, c), F32), np.zeros((b + 1, m, c), F32)):
        with pytest.raises(ValueError, match=r"feat_q be of shape \(batch,#queries,channels\)"):
            sub(q=bad)
    for bad in (np.zeros((b, n), F32), np.zeros((b, n, c + 1), F32), np.zeros((b + 1, n, c), F32)):
        with pytest.raises(ValueError, match=r"feat_src be of shape \(batch,#points,channels\)"):
            sub(src=bad)
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        sub(q=np.zeros((b, m, 1025), F32), src=np.zeros((b, n, 1025), F32))
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        sub(q=np.zeros((b, m, 0), F32), src=np.zeros((b, n, 0), F32))
    with pytest.raises(ValueError, match="1 to 65536 points"):
        sub(src=np.zeros((b, 0, c), F32))
    for bad in (np.zeros((b, m, k), F32), np.zeros((b, m, k + 1, c), F32), np.zeros((b, m + 1, k, c), F32)):
        with pytest.raises(ValueError, match=r"grad_out be of shape \(batch,#queries,k,channels\)"):
            sgr(g=bad)
    for bad in (0, 65537, -1):
        with pytest.raises(ValueError, match="1 to 65536 points"):
            sgr(n=bad)
    for f in (agg, agr):
        for bad in (np.zeros((b, n), F32), np.zeros((b + 1, n, c), F32)):
            with pytest.raises(ValueError, match=r"value be of shape \(batch,#points,channels\)"):
                f(v=bad)
        for bad in (np.zeros((b, m, k), F32), np.zeros((b, m, k + 1, cw), F32)):
            with pytest.raises(ValueError, match=r"weight be of shape \(batch,#queries,k,channels\)"):
                f(w=bad)
        for bad in (np.zeros((b, m, k, 3), F32), np.zeros((b, m, k, 16), F32), np.zeros((b, m, k, 0), F32)):
            with pytest.raises(ValueError, match="channels of weight to divide those of value"):
                f(w=bad)
        for bad in (np.zeros((b, m, k), F32), np.zeros((b, m, k, c + 4), F32), np.zeros((b, m, k, cw), F32)):
            with pytest.raises(ValueError, match=r"pos be of shape \(batch,#queries,k,channels\)"):
                f(pos=bad)
    for bad in (np.zeros((b, m), F32), np.zeros((b, m, c + 4), F32), np.zeros((b, m + 1, c), F32)):
        with pytest.raises(ValueError, match=r"grad_out be of shape \(batch,#queries,channels\)"):
            agr(g=bad)
    with pytest.raises(ValueError, match="idx be of shape"):
        glue.neighbor_subtraction(q, src, np.zeros((b, m), I32))
    with pytest.raises(ValueError, match="divide"):
        glue.neighbor_aggregation(src, np.zeros((b, m, k, 3), F32), idx)
    with pytest.raises(ValueError, match="lengths1"):
        glue.neighbor_aggregation(src, w, idx, pos=pos, lengths1=[0, 1])
