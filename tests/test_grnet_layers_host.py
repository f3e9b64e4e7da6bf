"""CPU: Gridding Reverse and Cubic Feature Sampling (include/rfops.h, "Gridding Reverse and Cubic Feature Sampling") at the
boundary -- declared, exported, bound; the workspace sizes; every argument rule answered before a device is touched; the
wrappers' checks -- and cfs_ref, cfs_grad_ref, grev_ref, grev_grad_ref, the numpy restatements of the contract that the GPU tests
hold the kernels to (float32 for u, float64 for every sum of the backward passes and for all of Gridding Reverse), pinned here by
independent means: a case by hand, a round trip through the Gridding layer's reference, central differences of an unquantised
float64 forward, and the adjoint identity of the sampling."""
import ctypes

import numpy as np
import pytest

from test_gridding_host import BOUNDS, CORNERS, F32, F64, family, gr_grid_ref, gr_points, gr_spread, pair, vertex_coord

BRICK, CHUNK = 8, 8  # brick_sort.hpp: GR_SUB_E, the sub-brick edge of the sampling's backward in vertices, and GR_CHUNK, its channels
TILE = 256           # grnet_layers.hip: GV_TILE, the cells per tile of Gridding Reverse's compaction
MAX_CHANNELS = 1024
U32, I32 = np.uint32, np.int32


# ---- the references -----------------------------------------------------------------------------------------------------
def _clamp(L, n):
    return n if L is None else min(max(int(L), 1), n)


def cloud(kind, seed, n, R, lo, hi):
    """family() of test_gridding_host; "seams" also gets the seams of this file's sub-bricks (multiples of BRICK = 8)"""
    x = family(kind, seed, n, R, lo, hi)
    if kind == "seams":
        rng = np.random.RandomState(seed + 5)
        k = rng.randint(0, (R + BRICK - 1) // BRICK + 1, (n, 3)) * BRICK - rng.randint(0, 2, (n, 3))
        x = np.where(rng.rand(n, 3) < 0.4, vertex_coord(np.clip(k, 0, R - 1), R, lo, hi), x).astype(F32)
    return np.ascontiguousarray(x)


def cfs_cells(x, R, lo, hi, L=None):
    """x (n, 3) -> (inside (n,) bool, vertex ids (k, 8) of the inside points' cells, d in the order of CORNERS)"""
    ins, cell, _, q1 = gr_points(x, R, lo, hi, _clamp(L, np.shape(x)[0]))
    return ins, gr_spread(cell[ins], q1[ins], R)[0]


def cfs_ref(x, vol, lo, hi, L=None):
    """x (n, 3), vol (c, R, R, R) float32 -> (feat (n, 8, c) float32, inside int): copies, bit for bit; +0 elsewhere"""
    vol = np.ascontiguousarray(vol, F32)
    c, R = vol.shape[0], vol.shape[1]
    ins, ids = cfs_cells(x, R, lo, hi, L)
    feat = np.zeros((np.shape(x)[0], 8, c), U32)
    feat[ins] = vol.reshape(c, -1).view(U32)[:, ids].transpose(1, 2, 0)
    return feat.view(F32), int(ins.sum())


def cfs_grad_ref(x, gf, R, lo, hi, L=None):
    """gf (n, 8, c) -> (grad (c, R, R, R) float64 before its rounding to float32, mag: the sums of the terms' magnitudes, cnt:
    the number of contributions per vertex (R, R, R))"""
    gf = np.asarray(gf, F32)
    c = gf.shape[2]
    ins, ids = cfs_cells(x, R, lo, hi, L)
    terms = gf[ins].reshape(-1, c).astype(F64)
    G, A = np.zeros((R ** 3, c), F64), np.zeros((R ** 3, c), F64)
    np.add.at(G, ids.ravel(), terms)
    np.add.at(A, ids.ravel(), np.abs(terms))
    cnt = np.bincount(ids.ravel(), minlength=R ** 3).reshape(R, R, R)
    return G.T.reshape(c, R, R, R), A.T.reshape(c, R, R, R), cnt


def cfs_grad_tol(G, A, cnt):
    """2^-23 |ref| + k 2^-52 sum |terms|: one float32 rounding plus the k - 1 roundings of a double sum of k terms"""
    return 2.0 ** -23 * np.abs(G) + cnt[None] * 2.0 ** -52 * A


def _cell_sums(g64, R):
    """g64 (R, R, R) float64 -> S, (Tx, Ty, Tz) over the (R - 1)^3 cells in the contract's order of additions"""
    C = R - 1
    w = [g64[dx:dx + C, dy:dy + C, dz:dz + C] for dx, dy, dz in CORNERS]
    with np.errstate(invalid="ignore", over="ignore"):
        S = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7]
        T = (((w[4] + w[5]) + w[6]) + w[7], ((w[2] + w[3]) + w[6]) + w[7], ((w[1] + w[3]) + w[5]) + w[7])
    return S, T


def _h_of(R, lo, hi):
    return (F64(F32(hi)) - F64(F32(lo))) / F64(R - 1)


def grev_ref(grid, lo, hi, eps=1e-6, compact=False):
    """grid (R, R, R) float32 -> (points (M, 3) float32, row (M,) int32, count int): include/rfops.h word for word"""
    grid = np.asarray(grid, F32)
    R = grid.shape[0]
    C, M = R - 1, (R - 1) ** 3
    S, T = _cell_sums(grid.astype(F64), R)
    with np.errstate(invalid="ignore"):
        valid = ((S >= F64(F32(eps))) & (S < np.inf)).ravel()
    idx = np.unravel_index(np.flatnonzero(valid), (C, C, C))
    Sv = S.ravel()[valid]
    p = np.stack([(F64(F32(lo)) + (idx[a].astype(F64) + T[a].ravel()[valid] / Sv) * _h_of(R, lo, hi)).astype(F32)
                  for a in range(3)], 1)
    count = int(valid.sum())
    row = np.full(M, -1, I32)
    row[valid] = np.arange(count, dtype=I32) if compact else np.flatnonzero(valid).astype(I32)
    points = np.zeros((M, 3), F32)
    points[row[valid]] = p
    return points, row, count


def grev_grad_ref(grid, row, gp, lo, hi):
    """-> (grad (R, R, R) float64 before its rounding to float32, tolerance: 2^-23 |ref| + 2^-45 sum |terms|).  The kernel and
    this function form S, T_a and f_a by the same IEEE operations, so they can differ only in the products and the sum over the
    at most 24 terms of a vertex: 2^-45 = 256 x 2^-53 of their magnitudes covers that with room, plus one float32 rounding."""
    grid, gp = np.asarray(grid, F32), np.asarray(gp, F32)
    R = grid.shape[0]
    C, M = R - 1, (R - 1) ** 3
    row = np.asarray(row).reshape(M)
    ok = (row >= 0) & (row < M)
    S, T = _cell_sums(grid.astype(F64), R)
    g = np.zeros((M, 3), F64)
    g[ok] = gp[row[ok]].astype(F64)
    ok3, g = ok.reshape(C, C, C), g.reshape(C, C, C, 3)
    h = _h_of(R, lo, hi)
    G, A = np.zeros((R, R, R), F64), np.zeros((R, R, R), F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        coef = h / S
        f = [T[a] / S for a in range(3)]
        for d in CORNERS:  # ascending d at every vertex, as the kernel adds
            t = [(F64(d[a]) - f[a]) * g[..., a] for a in range(3)]
            term = np.where(ok3, coef * ((t[0] + t[1]) + t[2]), 0.0)
            mag = np.where(ok3, np.abs(coef) * ((np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])), 0.0)
            G[d[0]:d[0] + C, d[1]:d[1] + C, d[2]:d[2] + C] += term
            A[d[0]:d[0] + C, d[1]:d[1] + C, d[2]:d[2] + C] += mag
    return G, 2.0 ** -23 * np.abs(G) + 2.0 ** -45 * A


def grev_exact(g64, lo, hi, valid):
    """The forward in float64 without the float32 rounding, the validity held fixed -> points (M, 3), zeros where invalid"""
    R = g64.shape[0]
    C = R - 1
    S, T = _cell_sums(g64, R)
    idx = np.stack(np.meshgrid(np.arange(C), np.arange(C), np.arange(C), indexing="ij"), -1).astype(F64)
    p = np.stack([F64(F32(lo)) + (idx[..., a] + T[a] / S) * _h_of(R, lo, hi) for a in range(3)], -1).reshape(-1, 3)
    return np.where(valid[:, None], p, 0.0)


def grev_grids(kind, seed, R, eps=1e-6):
    """(R, R, R) float32 grids of the families the tests use"""
    rng = np.random.RandomState(seed)
    if kind == "zeros":
        return np.zeros((R, R, R), F32)
    if kind == "dense":
        return (0.25 + rng.rand(R, R, R)).astype(F32)
    if kind == "sparse":  # the Gridding layer's output for a cloud of 2048 points
        return gr_grid_ref(family("uniform", seed, 2048, R, -0.5, 0.5), R, -0.5, 0.5)[0]
    if kind == "wild":  # mostly zeros; negatives, NaN, inf, and lone weights of eps and its two neighbours.  (No huge finite entries:
        # h / S would put gradients into float32's subnormal range, where the backward's relative bar does not apply.)
        g = (rng.rand(R, R, R) * (rng.rand(R, R, R) < 0.1)).astype(F32)
        k = max(R ** 3 // 32, 1)
        for val in (np.nan, np.inf, -np.inf, -0.75):
            g.ravel()[rng.randint(0, R ** 3, k)] = val
        near = np.array([eps, np.nextafter(F32(eps), F32(0)), np.nextafter(F32(eps), F32(1))], F32)
        g.ravel()[rng.randint(0, R ** 3, 4 * k)] = rng.choice(near, 4 * k)  # S is that weight where the other corners are zero
        return g
    raise ValueError(kind)


COUNT_EPS = 6.0


def grid_with_count(R, count, seed=0):
    """A grid with exactly `count` valid cells at eps = COUNT_EPS: ones on all eight corners (S = 8) of `count` cells whose
    coordinates are multiples of 3.  Such cells share no vertex, and any other cell has, per axis, a vertex plane in common with
    at most one of them, so its S is at most 4."""
    k = (R - 1 + 2) // 3
    assert count <= k ** 3
    g = np.zeros((R, R, R), F32)
    for c in np.random.RandomState(seed).permutation(k ** 3)[:count]:
        x, y, z = 3 * (c // (k * k)), 3 * ((c // k) % k), 3 * (c % k)
        g[x:x + 2, y:y + 2, z:z + 2] = 1.0
    return g


# ---- pinned ---------------------------------------------------------------------------------------------------------------
HAND = np.array([1, 0, 0, 1, 0, 2, 0, 4], F32).reshape(2, 2, 2)  # w_d at (dx, dy, dz), dz fastest


def test_by_hand():
    """R = 2 over [-0.5, 0.5]: one cell, h = 1, the weights w_0 .. w_7 = 1, 0, 0, 1, 0, 2, 0, 4.
    S = 8;  T_x = w4 + w5 + w6 + w7 = 6,  T_y = w2 + w3 + w6 + w7 = 5,  T_z = w1 + w3 + w5 + w7 = 7;  f = (0.75, 0.625, 0.875);
    the point is lo + f h = (0.25, 0.125, 0.375).  With grad_points = (1, 2, 4):
    grad_grid[d] = (h / S) ((dx - 0.75) 1 + (dy - 0.625) 2 + (dz - 0.875) 4) = (dx + 2 dy + 4 dz - 5.5) / 8.
    Cubic feature sampling of a point in that cell returns the eight values in that order, per channel."""
    for compact in (False, True):
        points, row, count = grev_ref(HAND, -0.5, 0.5, 1e-6, compact)
        assert points.tolist() == [[0.25, 0.125, 0.375]] and row.tolist() == [0] and count == 1
    G, tol = grev_grad_ref(HAND, [0], [[1, 2, 4]], -0.5, 0.5)
    assert G.ravel().tolist() == [(dx + 2 * dy + 4 * dz - 5.5) / 8 for dx, dy, dz in CORNERS] and (tol > 0).all()
    assert not grev_grad_ref(HAND, [-1], [[1, 2, 4]], -0.5, 0.5)[0].any() and not grev_grad_ref(HAND, [1], [[1, 2, 4]], -0.5, 0.5)[0].any()
    # S below eps, a NaN and an infinite S are invalid; a negative entry passes if S does
    assert grev_ref(HAND, -0.5, 0.5, 8.5)[2] == 0 and grev_ref(HAND, -0.5, 0.5, 8.0)[2] == 1
    for bad in (np.nan, np.inf, -np.inf):
        g = HAND.copy()
        g[0, 1, 0] = bad
        points, row, count = grev_ref(g, -0.5, 0.5)
        assert count == 0 and row.tolist() == [-1] and not points.view(U32).any()
    g = HAND.copy()
    g[0, 1, 0] = -4
    assert grev_ref(g, -0.5, 0.5)[2] == 1 and grev_ref(g, -0.5, 0.5)[0].tolist() == [[1.0, -0.25, 1.25]]  # S = 4, T = (6, 1, 7)
    vol = np.stack([HAND, -HAND])
    feat, inside = cfs_ref(np.array([[0.1, -0.2, 0.3], [0.6, 0, 0], [0.5, 0.5, -0.5]], F32), vol, -0.5, 0.5)
    assert inside == 2 and feat[0].T.tolist() == [HAND.ravel().tolist(), (-HAND).ravel().tolist()]
    assert not feat[1].view(U32).any() and feat[2].tobytes() == feat[0].tobytes()
    G, A, cnt = cfs_grad_ref(np.array([[0.1, -0.2, 0.3], [0.6, 0, 0], [0.5, 0.5, -0.5]], F32), np.ones((3, 8, 2), F32), 2, -0.5, 0.5)
    assert (G == 2).all() and (A == 2).all() and (cnt == 2).all()


@pytest.mark.parametrize("compact", [False, True])
def test_round_trip_through_the_gridding_layer(compact):
    """One point at a cell's centre: q1 = 256 exactly on every axis, the layer puts 1 / 8 on the cell's eight vertices, and the
    centre cell (S = 1, T_a = 1 / 2) returns that centre exactly."""
    R, (lo, hi) = 5, BOUNDS[0]
    cell = (1, 2, 1)
    centre = np.array([[lo + (k + 0.5) * 0.25 for k in cell]], F32)
    grid, inside, _ = gr_grid_ref(centre, R, lo, hi)
    assert inside == 1 and sorted(set(grid.ravel().tolist())) == [0.0, 0.125]
    points, row, count = grev_ref(grid, lo, hi, 1e-6, compact)
    c = (cell[0] * 4 + cell[1]) * 4 + cell[2]
    assert count == 27 and row[c] == (13 if compact else c)  # the 3^3 cells that touch a weighted vertex; 13 before the centre
    assert points[row[c]].tolist() == centre[0].tolist()
    assert (row >= 0).sum() == count
    if compact:
        assert sorted(row[row >= 0].tolist()) == list(range(count)) and not points[count:].view(U32).any()


@pytest.mark.parametrize("R", [2, 4])
def test_reverse_gradient_against_central_differences(R):
    """grev_grad_ref against central differences of the float64 forward, <gp, points>, on dense grids whose S (>= 2) stays far
    from eps: the forward is a ratio of linear functions of a vertex, so a step of 1e-6 leaves a relative error of ~1e-10."""
    lo, hi = BOUNDS[1]
    grid = grev_grids("dense", 3 + R, R)
    M = (R - 1) ** 3
    points, row, count = grev_ref(grid, lo, hi, 1e-6, True)
    assert count == M
    gp = np.random.RandomState(R).randn(M, 3).astype(F32)
    G, tol = grev_grad_ref(grid, row, gp, lo, hi)
    valid, h = np.ones(M, bool), 1e-6
    for v in range(R ** 3):
        up, dn = grid.astype(F64), grid.astype(F64)
        up.ravel()[v] += h
        dn.ravel()[v] -= h
        cd = ((grev_exact(up, lo, hi, valid) - grev_exact(dn, lo, hi, valid)) * gp.astype(F64)).sum() / (2 * h)
        assert abs(cd - G.ravel()[v]) <= 1e-7 * max(1.0, abs(cd)), (v, cd, G.ravel()[v])
    assert (tol > 0).all()


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 9])
def test_sampling_adjoint_identity(R, lo, hi):
    """<cfs_ref(vol), G> = <vol, cfs_grad_ref(G)>, exactly, for integer-valued vol and G"""
    rng = np.random.RandomState(R)
    for kind in ("uniform", "outside", "seams", "vertices"):
        x = pair(kind, R, 65, 33, R, lo, hi)[0]
        vol = rng.randint(-8, 9, (3, R, R, R)).astype(F32)
        gf = rng.randint(-1024, 1025, (65, 8, 3)).astype(F32)
        for L in (None, 1, 33):
            feat, inside = cfs_ref(x, vol, lo, hi, L)
            G, A, cnt = cfs_grad_ref(x, gf, R, lo, hi, L)
            assert (feat.astype(F64) * gf).sum() == (vol.astype(F64) * G).sum()
            assert cnt.sum() == 8 * inside and (G == np.rint(G)).all() and not feat[_clamp(L, 65):].view(U32).any()


def test_grid_with_count():
    for R, count in ((4, 0), (4, 1), (5, 8), (11, 26), (22, TILE - 1), (22, TILE), (22, TILE + 1)):
        points, row, got = grev_ref(grid_with_count(R, count, count), -0.5, 0.5, COUNT_EPS, True)
        assert got == count and (row >= 0).sum() == count


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_cubic_feature_sampling", "rf_cubic_feature_sampling_grad", "rf_cubic_feature_sampling_grad_workspace_bytes",
           "rf_gridding_reverse", "rf_gridding_reverse_grad", "rf_gridding_reverse_workspace_bytes")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    assert f"#define RF_CFS_MAX_CHANNELS {_raw.CFS_MAX_CHANNELS}\n" in header and _raw.CFS_MAX_CHANNELS == MAX_CHANNELS
    assert (_raw.CFS_BRICK, _raw.CFS_CHUNK, _raw.GREV_TILE) == (BRICK, CHUNK, TILE)
    src = open(_lib._PKG + "/csrc/grnet_layers.hip").read()
    shared = open(_lib._PKG + "/csrc/brick_sort.hpp").read()
    assert '#include "brick_sort.hpp"' in src and f"GR_SUB_E = {BRICK}," in shared and f"GR_CHUNK = {CHUNK};" in shared
    assert f"GV_TILE = {TILE}," in src


def test_workspace_sizes():
    from rfnet_amd._lib import lib
    fc, fr = lib.rf_cubic_feature_sampling_grad_workspace_bytes, lib.rf_gridding_reverse_workspace_bytes
    for shape in ((0, 10, 8), (-1, 10, 8), (2, 0, 8), (2, 65537, 8), (65536, 10, 8), (2, 10, 1), (2, 10, 257), (2, 10, -3)):
        assert fc(*shape) == 0, shape
    for shape in ((0, 8), (-1, 8), (65536, 8), (2, 1), (2, 257), (2, 0), (2, -3)):
        assert fr(*shape) == 0, shape
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for b, n, R in ((1, 1, 2), (3, 300, 17), (32, 16384, 64), (65535, 65536, 256)):
        nb3 = ((R + 15) // 16) ** 3
        assert fc(b, n, R) == r(4 * b * (nb3 + 1)) + r(8 * b * n), (b, n, R)
        assert fr(b, R) == r(4 * b * (((R - 1) ** 3 + TILE - 1) // TILE)), (b, R)


P, WS, BIG = 0x10000, 0x200000, 1 << 60  # never dereferenced: every call below must return at its argument checks


def _t(k, null, at):
    t = [P] * k
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return t


def _cfs(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(3, null, at)  # xyz, vol, feat
    return lib.rf_cubic_feature_sampling(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], P, None)


def _cfs_grad(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(3, null, at)  # xyz, grad_feat, grad_vol
    return lib.rf_cubic_feature_sampling_grad(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], ws, wsz, None)


def _rev(b=2, res=17, lo=-0.5, hi=0.5, eps=1e-6, compact=1, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # grid, points, row, count
    return lib.rf_gridding_reverse(b, res, lo, hi, eps, compact, t[0], t[1], t[2], t[3], ws, wsz, None)


def _rev_grad(b=2, res=17, lo=-0.5, hi=0.5, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # grid, row, grad_points, grad_grid
    return lib.rf_gridding_reverse_grad(b, res, lo, hi, t[0], t[1], t[2], t[3], None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    nan, inf = float("nan"), float("inf")
    box = (dict(lo=nan), dict(hi=nan), dict(lo=-inf), dict(hi=inf), dict(lo=0.5, hi=0.5), dict(lo=0.5, hi=-0.5),
           dict(lo=1e39), dict(res=1), dict(res=0), dict(res=257), dict(res=-2), dict(b=-1), dict(b=65536))
    cloud = (dict(n=-3), dict(b=0, n=-1), dict(b=0, c=-1), dict(n=0), dict(n=65537), dict(c=0), dict(c=-1), dict(c=1025))
    assert _cfs(b=0) == OK and _cfs(b=0, n=0, c=0, res=0, lo=nan) == OK
    assert _cfs_grad(b=0) == OK and _cfs_grad(b=0, n=0, c=0, res=0, ws=None, wsz=0) == OK
    for bad in box + cloud:
        assert _cfs(**bad) == EINVAL, bad
        assert _cfs_grad(**bad) == EINVAL, bad
    for k in range(3):
        assert _cfs(null=k) == EINVAL and _cfs(at=(k, P + 2)) == EINVAL, k
        assert _cfs_grad(null=k) == EINVAL and _cfs_grad(at=(k, P + 1)) == EINVAL, k
    assert lib.rf_cubic_feature_sampling(2, 300, 5, 17, -0.5, 0.5, P, P, P, P, None, None) == EINVAL  # inside
    assert lib.rf_cubic_feature_sampling(2, 300, 5, 17, -0.5, 0.5, P, P, P, P, P + 2, None) == EINVAL
    assert _cfs(ln=P + 2) == EINVAL and _cfs_grad(ln=P + 2) == EINVAL
    assert _cfs_grad(ws=None) == EINVAL and _cfs_grad(ws=WS + 8) == EINVAL
    need = lib.rf_cubic_feature_sampling_grad_workspace_bytes(2, 300, 17)
    assert need > 0 and _cfs_grad(wsz=need - 1) == EWORKSPACE and _cfs_grad(wsz=0, ln=None) == EWORKSPACE
    assert _cfs_grad(b=65535, n=65536, c=1024, res=256, wsz=0) == EWORKSPACE  # the largest sizes are sizes

    assert _rev(b=0) == OK and _rev(b=0, res=0, lo=nan, eps=nan, compact=7, ws=None, wsz=0) == OK and _rev_grad(b=0) == OK
    for bad in box:
        assert _rev(**bad) == EINVAL, bad
        assert _rev_grad(**bad) == EINVAL, bad
    for bad in (dict(eps=0.0), dict(eps=-1e-6), dict(eps=nan), dict(eps=inf), dict(compact=2), dict(compact=-1)):
        assert _rev(**bad) == EINVAL, bad
    for k in range(4):
        assert _rev(null=k) == EINVAL and _rev(at=(k, P + 2)) == EINVAL, k
        assert _rev_grad(null=k) == EINVAL and _rev_grad(at=(k, P + 1)) == EINVAL, k
    assert _rev(ws=None) == EINVAL and _rev(ws=WS + 4) == EINVAL
    assert _rev(wsz=lib.rf_gridding_reverse_workspace_bytes(2, 17) - 1) == EWORKSPACE and _rev(compact=0, wsz=0) == EWORKSPACE
    assert _rev(b=65535, res=256, wsz=0) == EWORKSPACE and _rev(res=2, lo=-3e38, hi=3e38, wsz=0) == EWORKSPACE


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, vol, grid = np.zeros((2, 4, 3), F32), np.zeros((2, 3, 8, 8, 8), F32), np.zeros((2, 8, 8, 8), F32)
    with pytest.raises(ValueError, match=r"xyz be of shape \(batch,#points,3\)"):
        _raw.cubic_feature_sampling(np.zeros((2, 4), F32), vol, -0.5, 0.5)
    for bad in (np.zeros((2, 3, 8, 8), F32), np.zeros((3, 3, 8, 8, 8), F32), np.zeros((2, 3, 8, 8, 7), F32)):
        with pytest.raises(ValueError, match=r"vol be of shape \(batch,channels,res,res,res\)"):
            _raw.cubic_feature_sampling(a, bad, -0.5, 0.5)
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        _raw.cubic_feature_sampling(a, np.zeros((2, 1025, 2, 2, 2), F32), -0.5, 0.5)
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        _raw.cubic_feature_sampling_grad(a, np.zeros((2, 4, 8, 0), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="2 to 256"):
        _raw.cubic_feature_sampling(a, np.zeros((2, 3, 1, 1, 1), F32), -0.5, 0.5)
    with pytest.raises(ValueError, match="2 to 256"):
        _raw.cubic_feature_sampling_grad(a, np.zeros((2, 4, 8, 3), F32), 257, -0.5, 0.5)
    with pytest.raises(ValueError, match=r"grad_feat be of shape \(batch,#points,8,channels\)"):
        _raw.cubic_feature_sampling_grad(a, np.zeros((2, 4, 7, 3), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="at least one point"):
        _raw.cubic_feature_sampling(np.zeros((2, 0, 3), F32), vol, -0.5, 0.5)
    with pytest.raises(ValueError, match="65536"):
        _raw.cubic_feature_sampling(np.zeros((2, 65537, 3), F32), vol, -0.5, 0.5)
    with pytest.raises(ValueError, match="lengths"):
        _raw.cubic_feature_sampling(a, vol, -0.5, 0.5, lengths=[0, 1])
    with pytest.raises(ValueError, match="lengths"):
        _raw.cubic_feature_sampling_grad(a, np.zeros((2, 4, 8, 3), F32), 8, -0.5, 0.5, lengths=[4])
    with pytest.raises(ValueError, match=r"grid be of shape \(batch,res,res,res\)"):
        _raw.gridding_reverse(np.zeros((2, 8, 8), F32), -0.5, 0.5)
    with pytest.raises(ValueError, match=r"grid be of shape \(batch,res,res,res\)"):
        _raw.gridding_reverse_grad(np.zeros((2, 8, 8, 9), F32), np.zeros((2, 343), I32), np.zeros((2, 343, 3), F32), -0.5, 0.5)
    with pytest.raises(ValueError, match="2 to 256"):
        _raw.gridding_reverse(np.zeros((2, 1, 1, 1), F32), -0.5, 0.5)
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50):
        with pytest.raises(ValueError, match="finite eps > 0"):
            _raw.gridding_reverse(grid, -0.5, 0.5, eps=eps)
    with pytest.raises(ValueError, match=r"row be of shape \(batch,\(res-1\)\^3\)"):
        _raw.gridding_reverse_grad(grid, np.zeros((2, 342), I32), np.zeros((2, 343, 3), F32), -0.5, 0.5)
    with pytest.raises(ValueError, match=r"grad_points be of shape \(batch,\(res-1\)\^3,3\)"):
        _raw.gridding_reverse_grad(grid, np.zeros((2, 343), I32), np.zeros((2, 343, 2), F32), -0.5, 0.5)
    for lo, hi in ((0.5, 0.5), (1.0, -1.0), (float("nan"), 1.0), (0.0, float("inf")), (0.0, 1e39)):
        with pytest.raises(ValueError, match="finite bounds"):
            _raw.cubic_feature_sampling(a, vol, lo, hi)
        with pytest.raises(ValueError, match="finite bounds"):
            _raw.gridding_reverse(grid, lo, hi)
        with pytest.raises(ValueError, match="finite bounds"):
            glue.gridding_reverse(grid, bounds=(lo, hi))
    with pytest.raises(ValueError, match="finite bounds"):
        glue.cubic_feature_sampling(a, vol, bounds=(0.5, -0.5))
