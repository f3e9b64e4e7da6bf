"""CPU: the point-voxel pair (include/rfops.h, "the point-voxel pair") at the boundary -- declared, exported, bound; the workspace
sizes; every argument rule answered before a device is touched; the wrappers' checks -- and vox_ref, vox_grad_ref, devox_ref,
devox_grad_ref, the numpy restatements of the contract that the GPU tests hold the kernels to (float32 for u and t, float64 with
the contract's roundings for everything else; the order-free sums as a plain float64 sum in point order and, on request, as the
correctly rounded exact sum by math.fsum), pinned here by independent means: cases by hand, a float64 trilinear formula, the
adjoint identities of both ops, and central differences of the float64 interpolant."""
import ctypes
import math

import numpy as np
import pytest

from test_gridding_host import BOUNDS, CORNERS, F32, F64, gr_gather, gr_points, gr_spread, inv_h_of
from test_grnet_layers_host import cloud

BRICK, CHUNK = 8, 8  # brick_sort.hpp: GR_SUB_E, the sub-brick edge of the two scatter kernels in vertices, and GR_CHUNK, their channels
MAX_CHANNELS = 1024
U32, I32, I64 = np.uint32, np.int32, np.int64


# ---- the references -----------------------------------------------------------------------------------------------------
def _clamp(L, n):
    return n if L is None else min(max(int(L), 1), n)


def pv_points(x, R, lo, hi, L=None):
    """x (n, 3) -> (inside (n,) bool, cell (n, 3), t (n, 3) float32, nearest vertex (n, 3)): k = i + (t >= 0.5f)"""
    ins, cell, t, _ = gr_points(x, R, lo, hi, _clamp(L, np.shape(x)[0]))
    return ins, cell, t, cell + (t >= F32(0.5))


def group_fsum(ids, terms, size):
    """ids (k,), terms (k, c) float64 -> (size, c): the exact sums per id, correctly rounded to float64 (+0 where nothing fell)"""
    out = np.zeros((size, terms.shape[1]), F64)
    order = np.argsort(ids, kind="stable")
    sid, st = ids[order], terms[order]
    cuts = np.concatenate([[0], np.flatnonzero(np.diff(sid)) + 1, [sid.size]])
    for s, e in zip(cuts[:-1], cuts[1:]):
        if e > s:
            out[sid[s]] = st[s] + 0.0 if e - s == 1 else [math.fsum(col) for col in st[s:e].T.tolist()]
    return out


def _scatter(ids, terms, size, fsum, reverse=False):
    """-> (sums (size, c), sums of magnitudes (size, c), contributions (size,))"""
    def plain(i, t):  # a plain double sum per column from +0, in the order given (np.bincount adds sequentially)
        return np.stack([np.bincount(i, weights=t[:, ch], minlength=size) for ch in range(t.shape[1])], 1)

    sl = slice(None, None, -1) if reverse else slice(None)
    G = group_fsum(ids, terms, size) if fsum else plain(ids[sl], terms[sl])
    A = plain(ids, np.abs(terms))
    return G, A, np.bincount(ids, minlength=size)


def vox_ref(x, feat, R, lo, hi, L=None, fsum=False, reverse=False):
    """x (n, 3), feat (n, c) -> (mean (c, R, R, R) float64: S / cnt before its rounding to float32 and +0 where cnt = 0, mag
    (c, R, R, R): the sums of |feat|, cnt (R, R, R) int32, inside int).  S is the plain double sum in point order, with `fsum`
    the correctly rounded exact sum."""
    feat = np.asarray(feat, F32)
    c = feat.shape[1]
    ins, _, _, k = pv_points(x, R, lo, hi, L)
    ids = ((k[ins, 0] * R + k[ins, 1]) * R + k[ins, 2]).astype(I64)
    S, A, cnt = _scatter(ids, feat[ins].astype(F64), R ** 3, fsum, reverse)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[:, None] > 0, S / cnt[:, None].astype(F64), 0.0)
    return mean.T.reshape(c, R, R, R), A.T.reshape(c, R, R, R), cnt.reshape(R, R, R).astype(I32), int(ins.sum())


def vox_tol(mean, mag):
    """the header's 2^-23 |exact| + 2^-52 sum |terms|, less 2^-51 |exact| for what fsum and the reference's own division leave"""
    return (2.0 ** -23 - 2.0 ** -51) * np.abs(mean) + 2.0 ** -52 * mag


def vox_grad_ref(x, cnt, gv, lo, hi, L=None, raw=False):
    """cnt (R, R, R), gv (c, R, R, R) -> grad_feat (n, c) float32 (raw: float64 before the rounding)"""
    gv, cnt = np.asarray(gv, F32), np.asarray(cnt)
    c, R = gv.shape[0], gv.shape[1]
    ins, _, _, k = pv_points(x, R, lo, hi, L)
    ids = (k[:, 0] * R + k[:, 1]) * R + k[:, 2]
    num = cnt.reshape(-1)[np.where(ins, ids, 0)]
    ok = ins & (num >= 1)
    out = np.zeros((np.shape(x)[0], c), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        out[ok] = gv.reshape(c, -1).astype(F64)[:, ids[ok]].T / num[ok, None].astype(F64)
        return out if raw else out.astype(F32)


def _weights(t):
    """t (k, 3) float32 -> W (k, 8) float64: ((double)w_x * (double)w_y) * (double)w_z with w(0) = 1.0f - t, w(1) = t"""
    w = np.stack([(F32(1) - t).astype(F64), t.astype(F64)], 0)  # w[d_a][point, axis]
    return np.stack([(w[dx][:, 0] * w[dy][:, 1]) * w[dz][:, 2] for dx, dy, dz in CORNERS], 1)


def devox_ref(x, vol, lo, hi, L=None, raw=False):
    """x (n, 3), vol (c, R, R, R) float32 -> (feat (n, c) float32 (raw: float64 before the rounding), inside int)"""
    vol = np.ascontiguousarray(vol, F32)
    c, R = vol.shape[0], vol.shape[1]
    ins, cell, t, _ = pv_points(x, R, lo, hi, L)
    ids = gr_spread(cell[ins], np.zeros_like(cell[ins]), R)[0]
    W, v64 = _weights(t[ins]), vol.reshape(c, -1).astype(F64)
    acc = np.zeros((ids.shape[0], c), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(8):  # ascending, from +0: one rounding per product and per addition
            acc = acc + W[:, d, None] * v64[:, ids[:, d]].T
        out = np.zeros((np.shape(x)[0], c), F64)
        out[ins] = acc
        return (out if raw else out.astype(F32)), int(ins.sum())


def devox_grad_ref(x, vol, gf, lo, hi, L=None, fsum=False, reverse=False):
    """vol (c, R, R, R), gf (n, c) -> (G (c, R, R, R) float64: grad_vol before its rounding to float32, A: the sums of the terms'
    magnitudes, k (R, R, R): the number of terms per vertex, grad_xyz (n, 3) float32).  G is the plain double sum of the prescribed
    terms W_d * (double)gf in (point, corner) order, with `fsum` their correctly rounded exact sum."""
    vol, gf = np.ascontiguousarray(vol, F32), np.asarray(gf, F32)
    c, R = vol.shape[0], vol.shape[1]
    ins, cell, t, _ = pv_points(x, R, lo, hi, L)
    ids = gr_spread(cell[ins], np.zeros_like(cell[ins]), R)[0]
    W, g64, v64 = _weights(t[ins]), gf[ins].astype(F64), vol.reshape(c, -1).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (W[:, :, None] * g64[:, None, :]).reshape(-1, c)
        G, A, k = _scatter(ids.ravel(), terms, R ** 3, fsum, reverse)
        gd = np.zeros(ids.shape, F64)
        for ch in range(c):  # ascending, from +0; every product of two float32 values is exact in float64
            gd = gd + g64[:, ch, None] * v64[ch][ids]
        gx = np.zeros((np.shape(x)[0], 3), F32)
        gx[ins] = (F64(inv_h_of(R, lo, hi)) * gr_gather(gd, t[ins])[0]).astype(F32)
    return G.T.reshape(c, R, R, R), A.T.reshape(c, R, R, R), k.reshape(R, R, R), gx


def devox_grad_tol(G, A, k):
    """the header's 2^-23 |exact| + k 2^-52 sum |terms|, less 2^-52 |exact| for what fsum leaves"""
    return (2.0 ** -23 - 2.0 ** -52) * np.abs(G) + k[None] * 2.0 ** -52 * A


def interp64(x, vol, lo, hi):
    """the float64 trilinear interpolant of vol (c, R, R, R) at x (n, 3) float64, all inside: nothing of the contract's float32"""
    c, R = vol.shape[0], vol.shape[1]
    u = (np.asarray(x, F64) - F64(F32(lo))) * (F64(R - 1) / (F64(F32(hi)) - F64(F32(lo))))
    i = np.minimum(np.floor(u).astype(I64), R - 2)
    t = u - i
    out = np.zeros((u.shape[0], c), F64)
    for dx, dy, dz in CORNERS:
        w = np.where(dx, t[:, 0], 1 - t[:, 0]) * np.where(dy, t[:, 1], 1 - t[:, 1]) * np.where(dz, t[:, 2], 1 - t[:, 2])
        out += w[:, None] * vol.astype(F64)[:, i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz].T
    return out


def volume(seed, c, R, wild=True):
    """random finite features; wild: denormals, -0.0 and +0.0 among them"""
    rng = np.random.RandomState(seed)
    vol = (rng.randn(c, R, R, R) * np.exp(2 * rng.randn(c, 1, 1, 1))).astype(F32)
    if wild:
        pick = rng.rand(c, R, R, R)
        vol = np.where(pick < 0.1, F32(-0.0), vol)
        vol = np.where((pick >= 0.1) & (pick < 0.15), F32(0.0), vol)
        vol = np.where((pick >= 0.15) & (pick < 0.25), (vol * F32(1e-40)).astype(F32), vol)
    return np.ascontiguousarray(vol, F32)


def family(kind, seed, n, R, lo, hi):
    """test_grnet_layers_host.cloud, and "collapsed": every point in one cell, its first point the cell's centre"""
    if kind != "collapsed":
        return cloud(kind, seed, n, R, lo, hi)
    rng = np.random.RandomState(seed)
    h = (F64(F32(hi)) - F64(F32(lo))) / (R - 1)
    cell = rng.randint(0, R - 1, 3)
    x = F64(F32(lo)) + (cell + 0.02 + 0.96 * rng.rand(n, 3)) * h
    x[0] = F64(F32(lo)) + (cell + 0.5) * h
    return np.ascontiguousarray(x, F32)


# ---- pinned ---------------------------------------------------------------------------------------------------------------
HAND = np.array([1, 0, 0, 1, 0, 2, 0, 4], F32).reshape(2, 2, 2)  # the values at (dx, dy, dz), dz fastest


def test_by_hand():
    """R = 2 over [-0.5, 0.5]: one cell, h = 1, u = x + 0.5.  Five points: on vertex 0; at t = 0.5 on x alone (the nearest vertex
    is the upper one: t >= 0.5f); on the upper face of all three axes (i = 0, t = 1); outside; NaN."""
    nan = float("nan")
    x = np.array([[-0.5, -0.5, -0.5], [0.0, -0.5, -0.5], [0.5, 0.5, 0.5], [0.6, 0, 0], [0, nan, 0]], F32)
    ins, cell, t, k = pv_points(x, 2, -0.5, 0.5)
    assert ins.tolist() == [True, True, True, False, False]
    assert k[:3].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1]] and t[:3].tolist() == [[0, 0, 0], [0.5, 0, 0], [1, 1, 1]]
    just_below = np.array([[-2.0 ** -25, -0.5, -0.5]], F32)  # u = 0.5 - 2^-25, the float32 below 0.5
    assert pv_points(just_below, 2, -0.5, 0.5)[3].tolist() == [[0, 0, 0]]
    feat = np.array([[1, 10], [2, 20], [4, 40], [8, 80], [16, 160]], F32)
    mean, mag, cnt, inside = vox_ref(x, feat, 2, -0.5, 0.5)
    assert inside == 3 and cnt.ravel().tolist() == [1, 0, 0, 0, 1, 0, 0, 1]
    assert mean[0].ravel().tolist() == [1, 0, 0, 0, 2, 0, 0, 4] and mean[1].ravel().tolist() == [10, 0, 0, 0, 20, 0, 0, 40]
    both = np.array([[-0.4, -0.4, -0.4], [-0.3, -0.2, -0.1], [0.0, 0.0, 0.0]], F32)  # two at vertex 0, the centre goes up
    mean, mag, cnt, inside = vox_ref(both, np.array([[1], [-4], [7]], F32), 2, -0.5, 0.5)
    assert cnt.ravel().tolist() == [2, 0, 0, 0, 0, 0, 0, 1] and mean.ravel().tolist() == [-1.5, 0, 0, 0, 0, 0, 0, 7]
    assert mag.ravel().tolist() == [5, 0, 0, 0, 0, 0, 0, 7]
    assert vox_ref(both, np.array([[1], [-4], [7]], F32), 2, -0.5, 0.5, L=1)[2].ravel().tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    # the backward: grad_vol at the nearest vertex over its count
    g = vox_grad_ref(both, cnt, np.arange(1, 9, dtype=F32).reshape(1, 2, 2, 2), -0.5, 0.5)
    assert g.ravel().tolist() == [0.5, 0.5, 8.0]
    assert vox_grad_ref(x, np.ones((2, 2, 2), I32), HAND[None], -0.5, 0.5).ravel().tolist() == [1, 0, 4, 0, 0]
    assert vox_grad_ref(x, np.zeros((2, 2, 2), I32), HAND[None], -0.5, 0.5).ravel().tolist() == [0, 0, 0, 0, 0]
    # devoxelization: a vertex returns its value, the midpoint of an edge the mean of its two ends, the corner the last value
    feat, inside = devox_ref(x, np.stack([HAND, -HAND]), -0.5, 0.5)
    assert inside == 3 and feat[:, 0].tolist() == [1, 0.5, 4, 0, 0] and feat[:, 1].tolist() == [-1, -0.5, -4, 0, 0]
    assert not feat[3:].view(U32).any()
    centre = np.zeros((1, 3), F32)
    assert devox_ref(centre, HAND[None], -0.5, 0.5)[0].tolist() == [[1.0]]  # (1 + 1 + 2 + 4) / 8
    # its backward: the centre spreads g / 8 on every vertex; d feat / dx = the mean of the upper face less the mean of the lower
    G, A, k, gx = devox_grad_ref(centre, HAND[None], np.array([[8]], F32), -0.5, 0.5)
    assert (G == 1).all() and (A == 1).all() and (k == 1).all()
    assert gx.tolist() == [[8.0, 4.0, 12.0]]  # 8 (T_a - (S - T_a)) / 4 with T = (6, 5, 7), S = 8
    G, A, k, gx = devox_grad_ref(x, HAND[None], np.ones((5, 1), F32), -0.5, 0.5, L=4)
    assert G.ravel().tolist() == [1.5, 0, 0, 0, 0.5, 0, 0, 1] and k.ravel().tolist() == [3] * 8 and not gx[3:].view(U32).any()


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 9])
def test_devox_ref_against_the_float64_formula(R, lo, hi):
    """the contract computes u and t in float32: an error of a few 2^-24 R in t, far inside 1e-6 of the volume's scale"""
    x = family("uniform", R, 200, R, lo, hi)
    vol = volume(R, 3, R, wild=False)
    ins = pv_points(x, R, lo, hi)[0]
    feat, inside = devox_ref(x, vol, lo, hi)
    assert inside == ins.sum() == 200
    assert np.abs(feat - interp64(x, vol, lo, hi)).max() <= 1e-6 * R * np.abs(vol).max()


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 9])
def test_devox_adjoint_identity(R, lo, hi):
    """<devox(vol), g> = <vol, devox_grad(g)> to double rounding; exactly where the terms are dyadic and small (integer values,
    coordinates that are multiples of 1/8 of a cell in a box with inv_h = 1)"""
    rng = np.random.RandomState(R)
    for kind in ("uniform", "outside", "seams", "vertices", "collapsed"):
        x = family(kind, R, 65, R, lo, hi)
        vol, g = volume(R + 1, 3, R, wild=False), rng.randn(65, 3).astype(F32)
        for L in (None, 1, 33):
            feat, inside = devox_ref(x, vol, lo, hi, L, raw=True)
            G, A, k, gx = devox_grad_ref(x, vol, g, lo, hi, L, fsum=True)
            lhs, rhs = (feat * g.astype(F64)).sum(), (vol.astype(F64) * G).sum()
            assert abs(lhs - rhs) <= 1e-12 * (np.abs(vol).astype(F64) * A).sum() + 1e-300
            assert k.sum() == 8 * inside and not feat[_clamp(L, 65):].any()
    x = (rng.randint(0, 8 * (R - 1) + 1, (65, 3)) / 8.0).astype(F32)
    vol, g = rng.randint(-64, 65, (3, R, R, R)).astype(F32), rng.randint(-64, 65, (65, 3)).astype(F32)
    feat, inside = devox_ref(x, vol, 0.0, R - 1.0, raw=True)
    G = devox_grad_ref(x, vol, g, 0.0, R - 1.0)[0]
    assert inside == 65 and (feat * g.astype(F64)).sum() == (vol.astype(F64) * G).sum()


@pytest.mark.parametrize("R", [2, 5])
def test_grad_xyz_against_central_differences(R):
    """grad_xyz against central differences of the float64 interpolant, <g, interp64(x)>, at points at least 0.05 of a cell from
    every face of their cell.  The interpolant is linear along an axis inside a cell, so a central difference with a step of
    0.01 cell has no truncation error: what is left is the contract's float32 u, t and 1.0f - t (each within 2^-23 R of the
    float64 value, entering a sum of 8 c terms through one factor of the product) and the float32 rounding of the result:
    2^-20 R inv_h sum |g| |vol| covers both with room, plus the difference quotient's own rounding 2^-50 sum |g| |vol| / step."""
    lo, hi = BOUNDS[1]
    rng = np.random.RandomState(R)
    h = (F64(F32(hi)) - F64(F32(lo))) / (R - 1)
    x = (F64(F32(lo)) + (rng.randint(0, R - 1, (40, 3)) + 0.05 + 0.9 * rng.rand(40, 3)) * h).astype(F32)
    vol, g = volume(R, 4, R, wild=False), rng.randn(40, 4).astype(F32)
    gx = devox_grad_ref(x, vol, g, lo, hi)[3]
    scale = (np.abs(g).astype(F64).sum(1) * np.abs(vol).max())[:, None]
    step = 0.01 * h
    for a in range(3):
        e = np.zeros(3)
        e[a] = step
        up, dn = interp64(x.astype(F64) + e, vol, lo, hi), interp64(x.astype(F64) - e, vol, lo, hi)
        cd = ((up - dn) * g.astype(F64)).sum(1) / (2 * step)
        tol = 2.0 ** -20 * R / h * scale[:, 0] + 2.0 ** -50 * scale[:, 0] / step
        assert (np.abs(cd - gx[:, a]) <= tol).all(), (a, np.abs(cd - gx[:, a]).max(), tol.min())
    assert np.abs(gx).max() > 0


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 9])
def test_vox_grad_is_the_adjoint_of_the_mean(R, lo, hi):
    """<vox(feat), gv> = <feat, vox_grad(gv)> to double rounding, and the mean of equal features is that feature"""
    rng = np.random.RandomState(R)
    for kind in ("uniform", "outside", "seams", "vertices", "collapsed"):
        x = family(kind, R + 1, 65, R, lo, hi)
        feat, gv = rng.randn(65, 3).astype(F32), rng.randn(3, R, R, R).astype(F32)
        for L in (None, 1, 33):
            mean, mag, cnt, inside = vox_ref(x, feat, R, lo, hi, L, fsum=True)
            gf = vox_grad_ref(x, cnt, gv, lo, hi, L, raw=True)
            lhs, rhs = (mean * gv.astype(F64)).sum(), (feat.astype(F64) * gf).sum()
            assert abs(lhs - rhs) <= 1e-12 * (np.abs(feat).astype(F64) * np.abs(gf)).sum() + 1e-300
            assert cnt.sum() == inside and not gf[_clamp(L, 65):].any() and (mag[:, cnt == 0] == 0).all()
            same = vox_ref(x, np.full((65, 2), 3.25, F32), R, lo, hi, L)[0]
            assert (same[:, cnt > 0] == 3.25).all() and not same[:, cnt == 0].any()


def test_sums_by_fsum_and_in_two_orders():
    """the three forms of the order-free sums agree where the sum is exact, and fsum is the exact one where it is not"""
    rng = np.random.RandomState(0)
    ids = rng.randint(0, 5, 400)
    t = rng.randint(-64, 65, (400, 2)).astype(F64)
    a, b_, c = (_scatter(ids, t, 6, f, r)[0] for f, r in ((False, False), (False, True), (True, False)))
    assert a.tobytes() == b_.tobytes() == c.tobytes() and not a[5].any()
    t = np.array([[1e16], [1.0], [-1e16], [1.0]])
    assert _scatter(np.zeros(4, I64), t, 1, True)[0].tolist() == [[2.0]] and _scatter(np.zeros(4, I64), t, 1, False)[0].tolist() != [[2.0]]
    assert _scatter(np.zeros(1, I64), np.array([[-0.0]]), 1, True)[0].view(np.uint64).tolist() == [[0]]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_voxelize_mean", "rf_voxelize_mean_workspace_bytes", "rf_voxelize_mean_grad", "rf_trilinear_devoxelize",
           "rf_trilinear_devoxelize_grad", "rf_trilinear_devoxelize_grad_workspace_bytes")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw, glue
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    assert (_raw.PV_BRICK, _raw.PV_CHUNK) == (BRICK, CHUNK) and _raw.CFS_MAX_CHANNELS == MAX_CHANNELS
    src = open(_lib._PKG + "/csrc/brick_sort.hpp").read()
    assert f"GR_SUB_E = {BRICK}," in src and f"GR_CHUNK = {CHUNK};" in src
    assert '#include "brick_sort.hpp"' in open(_lib._PKG + "/csrc/point_voxel.hip").read()
    for name in ("avg_voxelize", "avg_voxelize_grad", "trilinear_devoxelize", "trilinear_devoxelize_grad"):
        assert callable(getattr(_raw, name))
    assert callable(glue.avg_voxelize) and callable(glue.trilinear_devoxelize)


def test_workspace_sizes():
    from rfnet_amd._lib import lib
    for f in (lib.rf_voxelize_mean_workspace_bytes, lib.rf_trilinear_devoxelize_grad_workspace_bytes):
        for shape in ((0, 10, 8), (-1, 10, 8), (2, 0, 8), (2, 65537, 8), (65536, 10, 8), (2, 10, 1), (2, 10, 257), (2, 10, -3)):
            assert f(*shape) == 0, shape
        r = lambda v: (v + 255) // 256 * 256  # noqa: E731
        for b, n, R in ((1, 1, 2), (3, 300, 17), (32, 16384, 64), (65535, 65536, 256)):
            nb3 = ((R + 15) // 16) ** 3
            assert f(b, n, R) == r(4 * b * (nb3 + 1)) + r(8 * b * n), (b, n, R)


P, WS, BIG = 0x10000, 0x200000, 1 << 60  # never dereferenced: every call below must return at its argument checks


def _t(k, null, at):
    t = [P] * k
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return t


def _vox(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(5, null, at)  # xyz, feat, vol, cnt, inside
    return lib.rf_voxelize_mean(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], t[3], t[4], ws, wsz, None)


def _vox_grad(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # xyz, cnt, grad_vol, grad_feat
    return lib.rf_voxelize_mean_grad(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], t[3], None)


def _devox(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # xyz, vol, feat, inside
    return lib.rf_trilinear_devoxelize(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], t[3], None)


def _devox_grad(b=2, n=300, c=5, res=17, lo=-0.5, hi=0.5, ln=P, gx=P, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = _t(4, null, at)  # xyz, vol, grad_feat, grad_vol
    return lib.rf_trilinear_devoxelize_grad(b, n, c, res, lo, hi, t[0], ln, t[1], t[2], t[3], gx, ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    nan, inf = float("nan"), float("inf")
    bad_sizes = (dict(lo=nan), dict(hi=nan), dict(lo=-inf), dict(hi=inf), dict(lo=0.5, hi=0.5), dict(lo=0.5, hi=-0.5),
                 dict(lo=1e39), dict(res=1), dict(res=0), dict(res=257), dict(res=-2), dict(b=-1), dict(b=65536),
                 dict(n=-3), dict(b=0, n=-1), dict(b=0, c=-1), dict(b=0, res=-1), dict(n=0), dict(n=65537), dict(c=0), dict(c=-1),
                 dict(c=1025))
    calls = ((_vox, 5), (_vox_grad, 4), (_devox, 4), (_devox_grad, 4))
    for f, k in calls:
        assert f(b=0) == OK and f(b=0, n=0, c=0, res=0, lo=nan) == OK
        for bad in bad_sizes:
            assert f(**bad) == EINVAL, (f.__name__, bad)
        for j in range(k):
            assert f(null=j) == EINVAL and f(at=(j, P + 2)) == EINVAL and f(at=(j, P + 1)) == EINVAL, (f.__name__, j)
        assert f(ln=P + 2) == EINVAL and f(ln=P + 1) == EINVAL, f.__name__
    assert _vox(b=0, ws=None, wsz=0) == OK and _devox_grad(b=0, ws=None, wsz=0, gx=None) == OK
    assert _devox_grad(gx=P + 2) == EINVAL
    for f, need in ((_vox, lib.rf_voxelize_mean_workspace_bytes(2, 300, 17)),
                    (_devox_grad, lib.rf_trilinear_devoxelize_grad_workspace_bytes(2, 300, 17))):
        assert f(ws=None) == EINVAL and f(ws=WS + 8) == EINVAL
        assert need > 0 and f(wsz=need - 1) == EWORKSPACE and f(wsz=0, ln=None) == EWORKSPACE
        assert f(b=65535, n=65536, c=1024, res=256, wsz=0) == EWORKSPACE  # the largest sizes are sizes
        assert f(res=2, lo=-3e38, hi=3e38, wsz=0) == EWORKSPACE
    assert _devox_grad(gx=None, wsz=0) == EWORKSPACE  # grad_xyz is optional


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, f = np.zeros((2, 4, 3), F32), np.zeros((2, 4, 5), F32)
    vol, cnt = np.zeros((2, 5, 8, 8, 8), F32), np.zeros((2, 8, 8, 8), I32)
    calls = {
        "avg_voxelize": lambda xyz=a, **k: _raw.avg_voxelize(xyz, k.pop("feat", f), k.pop("res", 8), *k.pop("box", (-0.5, 0.5)), **k),
        "avg_voxelize_grad": lambda xyz=a, **k: _raw.avg_voxelize_grad(xyz, k.pop("cnt", cnt), k.pop("vol", vol), *k.pop("box", (-0.5, 0.5)), **k),
        "trilinear_devoxelize": lambda xyz=a, **k: _raw.trilinear_devoxelize(xyz, k.pop("vol", vol), *k.pop("box", (-0.5, 0.5)), **k),
        "trilinear_devoxelize_grad": lambda xyz=a, **k: _raw.trilinear_devoxelize_grad(xyz, k.pop("vol", vol), k.pop("gf", f), *k.pop("box", (-0.5, 0.5)), **k),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name + r" requires xyz be of shape \(batch,#points,3\)"):
            call(np.zeros((2, 4), F32))
        with pytest.raises(ValueError, match="at least one point"):
            call(np.zeros((2, 0, 3), F32))
        with pytest.raises(ValueError, match="65536"):
            call(np.zeros((2, 65537, 3), F32))
        with pytest.raises(ValueError, match="lengths"):
            call(lengths=[0, 1])
        with pytest.raises(ValueError, match="lengths"):
            call(lengths=[4])
        for lo, hi in ((0.5, 0.5), (1.0, -1.0), (float("nan"), 1.0), (0.0, float("inf")), (0.0, 1e39)):
            with pytest.raises(ValueError, match=name + " expects finite bounds"):
                call(box=(lo, hi))
        if name != "avg_voxelize":
            for bad in (np.zeros((2, 5, 8, 8), F32), np.zeros((3, 5, 8, 8, 8), F32), np.zeros((2, 5, 8, 8, 7), F32)):
                with pytest.raises(ValueError, match=r"vol be of shape \(batch,channels,res,res,res\)"):
                    call(vol=bad)
            with pytest.raises(ValueError, match="1 to 1024 channels"):
                call(vol=np.zeros((2, 1025, 2, 2, 2), F32))
            with pytest.raises(ValueError, match="2 to 256"):
                call(vol=np.zeros((2, 5, 1, 1, 1), F32))
    for bad in (np.zeros((2, 4), F32), np.zeros((2, 5, 5), F32), np.zeros((3, 4, 5), F32)):
        with pytest.raises(ValueError, match=r"feat be of shape \(batch,#points,channels\)"):
            calls["avg_voxelize"](feat=bad)
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        calls["avg_voxelize"](feat=np.zeros((2, 4, 0), F32))
    with pytest.raises(ValueError, match="1 to 1024 channels"):
        calls["avg_voxelize"](feat=np.zeros((2, 4, 1025), F32))
    for res in (1, 257, 0, -4):
        with pytest.raises(ValueError, match="2 to 256"):
            calls["avg_voxelize"](res=res)
    for bad in (np.zeros((2, 8, 8), I32), np.zeros((2, 8, 8, 7), I32), np.zeros((1, 8, 8, 8), I32)):
        with pytest.raises(ValueError, match=r"cnt be of shape \(batch,res,res,res\)"):
            calls["avg_voxelize_grad"](cnt=bad)
    for bad in (np.zeros((2, 4, 4), F32), np.zeros((2, 5, 5), F32), np.zeros((2, 4, 5, 1), F32)):
        with pytest.raises(ValueError, match=r"grad_feat be of shape \(batch,#points,channels\)"):
            calls["trilinear_devoxelize_grad"](gf=bad)
    with pytest.raises(ValueError, match="finite bounds"):
        glue.avg_voxelize(a, f, 8, bounds=(0.5, -0.5))
    with pytest.raises(ValueError, match="finite bounds"):
        glue.trilinear_devoxelize(a, vol, bounds=(0.5, -0.5))
    with pytest.raises(ValueError, match="2 to 256"):
        glue.avg_voxelize(a, f, resolution=1)
