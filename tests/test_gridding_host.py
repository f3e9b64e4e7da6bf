"""CPU: the gridding entries (include/rfops.h, "the Gridding layer and the Gridding loss") at the boundary -- declared, exported,
bound; the workspace sizes; every argument rule answered before a device is touched; the wrappers' checks -- and gr_ref, the numpy
restatement of the contract that the GPU tests hold the kernels to bit for bit (float32 for u and t, int64 for every sum, float64
for the gradients), pinned here by independent means: a case by hand, the mass identity, the self distance, permutations, central
differences of the unquantised float64 loss, and the derived distance from that loss."""
import ctypes

import numpy as np
import pytest
import torch

Q = 512
Q3 = Q ** 3
COUNTS, DENSITY = 0, 1
BRICK = 16  # gridding.hip's brick edge E, in vertices
F32, F64, I64 = np.float32, np.float64, np.int64
CORNERS = [(d >> 2, (d >> 1) & 1, d & 1) for d in range(8)]  # d = 0 .. 7, dz fastest


# ---- the reference ------------------------------------------------------------------------------------------------------
def inv_h_of(R, lo, hi):
    return F32(F64(R - 1) / (F64(F32(hi)) - F64(F32(lo))))


def gr_points(x, R, lo, hi, L=None):
    """x (n, 3) -> (inside (n,) bool, cell (n, 3) int64, t (n, 3) float32, q1 (n, 3) int64): the per-point quantities of the
    contract, u and t in float32; rows behind the count L are not inside."""
    x = np.ascontiguousarray(x, F32)
    n = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - F32(lo)) * inv_h_of(R, lo, hi)  # a subtraction, then a multiplication: two float32 roundings
        ins = ((u >= F32(0)) & (u <= F32(R - 1))).all(1)
    if L is not None:
        ins &= np.arange(n) < int(L)
    u = np.where(ins[:, None], u, F32(0)).astype(F32)
    cell = np.minimum(np.floor(u).astype(I64), R - 2)
    t = u - cell.astype(F32)
    assert t.dtype == F32
    q1 = np.rint(t * F32(512)).astype(I64)
    return ins, cell, t, q1


def gr_spread(cell, q1, R):
    """-> (vertex ids (k, 8), integer weights (k, 8)) of points with the given cells and q1, d in the order of CORNERS"""
    q = np.stack([Q - q1, q1], 0)  # q[d_k][point, axis]
    ids = np.empty((cell.shape[0], 8), I64)
    W = np.empty((cell.shape[0], 8), I64)
    for d, (dx, dy, dz) in enumerate(CORNERS):
        ids[:, d] = ((cell[:, 0] + dx) * R + cell[:, 1] + dy) * R + cell[:, 2] + dz
        W[:, d] = q[dx][:, 0] * q[dy][:, 1] * q[dz][:, 2]
    return ids, W


def gr_gather(vals, t, negate=False):
    """sum_d (sigma_a(d) val_d) (prod_{k != a} w_k(d_k)) for a = 0, 1, 2, in float64 from +0, d ascending; vals (k, 8) float64.
    -> (sums (k, 3), sums of the terms' magnitudes (k, 3))"""
    w = np.stack([(F32(1) - t).astype(F64), t.astype(F64)], 0)  # w[d_k][point, axis]; 1.0f - t in float32
    acc, mag = np.zeros((t.shape[0], 3), F64), np.zeros((t.shape[0], 3), F64)
    for d, dd in enumerate(CORNERS):
        v = -vals[:, d] if negate else vals[:, d]
        for a in range(3):
            k0, k1 = [k for k in range(3) if k != a]
            term = (v if dd[a] else -v) * (w[dd[k0]][:, k0] * w[dd[k1]][:, k1])
            acc[:, a] = acc[:, a] + term
            mag[:, a] = mag[:, a] + np.abs(term)
    return acc, mag


def gr_ref(a, c, R, lo, hi, mode=COUNTS, L1=None, L2=None, full=False):
    """a (n, 3), c (m, 3); the first L1 / L2 rows are the clouds -> (loss float32, inside (2,) int32, grad_a (n, 3) float32,
    grad_c (m, 3) float32): include/rfops.h's definitions word for word.  full: also {"ids": the touched vertices, "D": their
    int64 differences, "sum": sum |D| as a Python int}."""
    n, m = np.shape(a)[0], np.shape(c)[0]
    L1 = n if L1 is None else min(max(int(L1), 1), n)
    L2 = m if L2 is None else min(max(int(L2), 1), m)
    in1, cell1, t1, q1 = gr_points(a, R, lo, hi, L1)
    in2, cell2, t2, q2 = gr_points(c, R, lo, hi, L2)
    ids1, W1 = gr_spread(cell1[in1], q1[in1], R)
    ids2, W2 = gr_spread(cell2[in2], q2[in2], R)
    mu1, mu2 = (L2, L1) if mode == DENSITY else (1, 1)
    keys = np.concatenate([ids1.ravel(), ids2.ravel()])
    vals = np.concatenate([mu1 * W1.ravel(), -mu2 * W2.ravel()]).astype(I64)
    uniq, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1)
    D = np.zeros(uniq.shape[0], I64)
    np.add.at(D, inv, vals)  # int64: exact, any order
    S = int(np.abs(D).sum())
    assert S <= 2 ** 60
    den = F64(L1) * F64(L2) if mode == DENSITY else F64(R) * F64(R) * F64(R)
    loss = F32(F64(S) / F64(Q3) / den)
    sgn = np.sign(D).astype(F64)
    k1 = ids1.shape[0]
    s1, s2 = sgn[inv[:k1 * 8]].reshape(-1, 8), sgn[inv[k1 * 8:]].reshape(-1, 8)
    ih = F64(inv_h_of(R, lo, hi))
    c1, c2 = (F64(1) / F64(L1), F64(1) / F64(L2)) if mode == DENSITY else (F64(1) / den, F64(1) / den)
    g1, g2 = np.zeros((n, 3), F32), np.zeros((m, 3), F32)
    g1[in1] = (gr_gather(s1, t1[in1])[0] * (ih * c1)).astype(F32)
    g2[in2] = (gr_gather(s2, t2[in2], negate=True)[0] * (ih * c2)).astype(F32)
    inside = np.array([in1.sum(), in2.sum()], np.int32)
    if full:
        return loss, inside, g1, g2, {"ids": uniq, "D": D, "sum": S}
    return loss, inside, g1, g2


def gr_grid_ref(a, R, lo, hi, L=None):
    """-> (grid (R, R, R) float32 with x slowest, inside int, G (R^3,) int64)"""
    n = np.shape(a)[0]
    L = n if L is None else min(max(int(L), 1), n)
    ins, cell, t, q1 = gr_points(a, R, lo, hi, L)
    ids, W = gr_spread(cell[ins], q1[ins], R)
    G = np.zeros(R ** 3, I64)
    np.add.at(G, ids.ravel(), W.ravel())
    return (G.astype(F64) / F64(Q3)).astype(F32).reshape(R, R, R), int(ins.sum()), G


def gr_grid_grad_ref(a, gg, R, lo, hi, L=None):
    """The backward of the layer for grad_grid gg (R, R, R) -> (grad (n, 3) float64 before its rounding to float32, tolerance
    (n, 3): 2^-23 |ref| + 2^-45 inv_h sum |terms| -- one float32 rounding plus the double sum's own roundings)."""
    n = np.shape(a)[0]
    L = n if L is None else min(max(int(L), 1), n)
    ins, cell, t, q1 = gr_points(a, R, lo, hi, L)
    ids, _ = gr_spread(cell[ins], q1[ins], R)
    acc, mag = gr_gather(np.asarray(gg, F32).reshape(-1)[ids].astype(F64), t[ins])
    ih = F64(inv_h_of(R, lo, hi))
    g, tol = np.zeros((n, 3), F64), np.zeros((n, 3), F64)
    g[ins] = ih * acc
    tol[ins] = 2.0 ** -23 * np.abs(g[ins]) + 2.0 ** -45 * ih * mag
    return g, tol


def gr_exact_grids(x, R, lo, hi, L=None):
    """The unquantised trilinear grid in float64 (dense, for small R) -> (G (R^3,), inside)"""
    x = np.asarray(x, F64)
    n = x.shape[0]
    L = n if L is None else int(L)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - F64(F32(lo))) * (F64(R - 1) / (F64(F32(hi)) - F64(F32(lo))))
        ins = ((u >= 0) & (u <= R - 1)).all(1) & (np.arange(n) < L)
    u = u[ins]
    cell = np.minimum(np.floor(u).astype(I64), R - 2)
    t = u - cell
    w = np.stack([1.0 - t, t], 0)
    G = np.zeros(R ** 3, F64)
    for dx, dy, dz in CORNERS:
        np.add.at(G, ((cell[:, 0] + dx) * R + cell[:, 1] + dy) * R + cell[:, 2] + dz, w[dx][:, 0] * w[dy][:, 1] * w[dz][:, 2])
    return G, int(ins.sum())


def gr_exact(a, c, R, lo, hi, mode=COUNTS, L1=None, L2=None, full=False):
    """The unquantised loss in float64: the mean over the vertices of |G1 - G2|, or sum |G1 / L1 - G2 / L2|"""
    L1 = np.shape(a)[0] if L1 is None else int(L1)
    L2 = np.shape(c)[0] if L2 is None else int(L2)
    G1, i1 = gr_exact_grids(a, R, lo, hi, L1)
    G2, i2 = gr_exact_grids(c, R, lo, hi, L2)
    Dn = L2 * G1 - L1 * G2 if mode == DENSITY else G1 - G2  # in the units of D / Q^3
    loss = np.abs(Dn).sum() / (F64(L1) * L2 if mode == DENSITY else F64(R) ** 3)
    return (loss, Dn, i1 + i2) if full else loss


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def vertex_coord(k, R, lo, hi):
    """the float32 coordinate of vertex k (exactly on it where lo, hi and h are dyadic)"""
    return (F32(lo) + np.asarray(k, F32) * F32((F64(F32(hi)) - F64(F32(lo))) / (R - 1))).astype(F32)


def family(kind, seed, n, R, lo, hi):
    """(n, 3) float32 clouds of the families the tests use"""
    rng = np.random.RandomState(seed)
    w = F32(hi) - F32(lo)
    x = (F32(lo) + w * rng.rand(n, 3)).astype(F32)
    if kind == "uniform":
        pass
    elif kind == "vertices":  # t = 0: many weights 0 and many D = 0 ties
        x = vertex_coord(rng.randint(0, R, (n, 3)), R, lo, hi)
    elif kind == "seams":  # brick seams, the faces of the box
        k = rng.randint(0, (R + BRICK - 1) // BRICK + 1, (n, 3)) * BRICK - rng.randint(0, 2, (n, 3))
        seam = vertex_coord(np.clip(k, 0, R - 1), R, lo, hi)
        seam = np.where(rng.rand(n, 3) < 0.25, F32(hi), seam)
        seam = np.where(rng.rand(n, 3) < 0.1, F32(lo), seam)
        x = np.where(rng.rand(n, 3) < 0.6, seam, x).astype(F32)
    elif kind == "outside":
        x = (F32(lo) - F32(0.3) * w + F32(1.6) * w * rng.rand(n, 3)).astype(F32)
    elif kind == "nonfinite":
        bad = rng.rand(n) < 0.2
        bad[:1] = True
        fill = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F32), (n, 3))
        x = np.where(bad[:, None] & (rng.rand(n, 3) < 0.5), fill, x).astype(F32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x)


KINDS = ("uniform", "vertices", "seams", "outside", "nonfinite")
BOUNDS = ((-0.5, 0.5), (-0.3, 0.7001))


def pair(kind, seed, n, m, R, lo, hi):
    return family(kind, seed, n, R, lo, hi), family(kind, seed + 1000, m, R, lo, hi)


# ---- gr_ref, pinned -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [COUNTS, DENSITY])
def test_gr_ref_by_hand(mode):
    """R = 2, one point at the centre of the one cell: eight weights of Q^3 / 8, against one point ON vertex 0."""
    a, c = np.zeros((1, 3), F32), np.full((1, 3), -0.5, F32)
    ins, cell, t, q1 = gr_points(a, 2, -0.5, 0.5)
    assert ins.all() and not cell.any() and (t == 0.5).all() and (q1 == 256).all()
    ids, W = gr_spread(cell, q1, 2)
    assert ids.tolist() == [list(range(8))] and (W == Q3 // 8).all()
    loss, inside, g1, g2, info = gr_ref(a, c, 2, -0.5, 0.5, mode, full=True)
    # c puts Q^3 on vertex 0: D = Q^3 / 8 - Q^3 there and Q^3 / 8 on the other seven; L1 = L2 = 1 in both modes
    assert info["D"].tolist() == [Q3 // 8 - Q3] + [Q3 // 8] * 7 and info["sum"] == Q3 * 14 // 8
    assert loss == F32(1.75 / (8 if mode == COUNTS else 1)) and inside.tolist() == [1, 1]
    # d loss / d a_x = c inv_h sum_d s sigma_x w_y w_z = c (+ 0.25 (vertex 0: s = -1, sigma = -1) - 3 * 0.25 + 4 * 0.25) = c / 2
    cc = 1 / 8 if mode == COUNTS else 1.0
    assert g1.tolist() == [[0.5 * cc] * 3]
    # c sits on vertex 0 with t = 0: -s sigma w w = -(-1)(-1)(1) = -1 from vertex 0, and -(+1)(+1)(1) = -1 from its neighbour
    assert g2.tolist() == [[-2.0 * cc] * 3]


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 16, 17, 33])
def test_t_is_exact_and_mass_is_conserved(R, lo, hi):
    for kind in KINDS:
        a = family(kind, R, 257, R, lo, hi)
        ins, cell, t, q1 = gr_points(a, R, lo, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            u = ((a - F32(lo)) * inv_h_of(R, lo, hi))[ins]
        assert 0 < ins.sum() and (ins.sum() < 257 or kind not in ("outside", "nonfinite"))
        assert ((t[ins] >= 0) & (t[ins] <= 1)).all() and (cell[ins] >= 0).all() and (cell[ins] <= R - 2).all()
        assert (cell[ins].astype(F64) + t[ins].astype(F64) == u.astype(F64)).all()  # t = u - i without a rounding
        ids, W = gr_spread(cell[ins], q1[ins], R)
        assert (W.sum(1) == Q3).all() and (W >= 0).all() and W.max() <= 2 ** 27
        grid, inside, G = gr_grid_ref(a, R, lo, hi)
        assert inside == ins.sum() and G.sum() == inside * Q3
        assert grid.dtype == F32 and abs(float(grid.astype(F64).sum()) - inside) <= inside * 2.0 ** -24


def test_upper_face_negative_zero_and_a_count_of_one():
    R, lo, hi = 17, -0.5, 0.5
    ins, cell, t, q1 = gr_points(np.array([[0.5, 0.5, 0.5], [0.5, -0.5, 0.0]], F32), R, lo, hi)
    assert ins.all() and cell.tolist() == [[15, 15, 15], [15, 0, 8]] and t.tolist() == [[1, 1, 1], [1, 0, 0]]
    ids, W = gr_spread(cell, q1, R)
    assert W[0].tolist() == [0] * 7 + [Q3] and ids[0, 7] == R ** 3 - 1  # all of the mass on the last vertex
    # -0.0 with lo = 0: u = -0.0 is inside (>= 0), the cell is 0, t = -0.0, q1 = 0
    ins, cell, t, q1 = gr_points(np.array([[-0.0, -0.0, -0.0]], F32), 3, 0.0, 1.0)
    assert ins.all() and not cell.any() and not q1.any() and (t == 0).all()
    loss, inside, g1, g2 = gr_ref(np.array([[-0.0, -0.0, -0.0]], F32), np.zeros((1, 3), F32), 3, 0.0, 1.0)
    assert loss == 0 and not g1.view(np.uint32).any() and not g2.view(np.uint32).any()  # +0, bit for bit
    # just below lo is outside; a NaN is outside
    assert not gr_points(np.array([[-1e-30, 0, 0], [np.nan, 0, 0]], F32), 3, 0.0, 1.0)[0].any()
    # a count of 1 (and anything below it is clamped to 1)
    a, c = pair("uniform", 3, 9, 7, 5, lo, hi)
    for L in (1, 0, -4):
        got = gr_ref(a, c, 5, lo, hi, DENSITY, L, 1)
        exp = gr_ref(a[:1], c[:1], 5, lo, hi, DENSITY)
        assert got[0] == exp[0] and got[1].tolist() == [1, 1]
        assert got[2][:1].tobytes() == exp[2].tobytes() and not got[2][1:].view(np.uint32).any()


@pytest.mark.parametrize("mode", [COUNTS, DENSITY])
@pytest.mark.parametrize("kind", KINDS)
def test_self_distance_and_permutations(kind, mode):
    R, (lo, hi) = 17, BOUNDS[1]
    a, c = pair(kind, 5, 257, 130, R, lo, hi)
    loss, inside, g1, g2 = gr_ref(a, a, R, lo, hi, mode)
    assert loss.view(np.uint32) == 0 and not g1.view(np.uint32).any() and not g2.view(np.uint32).any()
    exp = gr_ref(a, c, R, lo, hi, mode)
    p1, p2 = np.random.RandomState(1).permutation(257), np.random.RandomState(2).permutation(130)
    got = gr_ref(a[p1], c[p2], R, lo, hi, mode)
    assert got[0].tobytes() == exp[0].tobytes() and got[1].tolist() == exp[1].tolist()
    assert got[2].tobytes() == exp[2][p1].tobytes() and got[3].tobytes() == exp[3][p2].tobytes()
    assert gr_grid_ref(a[p1], R, lo, hi)[0].tobytes() == gr_grid_ref(a, R, lo, hi)[0].tobytes()


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("R", [2, 3, 16, 17, 33])
def test_distance_from_the_unquantised_loss(R, lo, hi):
    """|gr_ref - float64 loss| <= (I1 + I2) (12 / Q + 24 R 2^-22) / R^3 in COUNTS mode: a per-axis weight is off by at most
    1 / (2 Q) from the quantisation plus R 2^-22 from the float32 roundings of u (x - lo, inv_h itself, the product: three
    relative errors of 2^-24 on a value of at most R); a vertex weight is a product of three factors of at most 1, so off by at
    most three times that, and a point has eight vertices."""
    for kind in ("uniform", "vertices", "seams", "outside"):
        a, c = pair(kind, 7 + R, 257, 130, R, lo, hi)
        loss, inside, _, _ = gr_ref(a, c, R, lo, hi)
        exact, _, cnt = gr_exact(a, c, R, lo, hi, full=True)
        bound = int(inside.sum()) * (12 / Q + 24 * R * 2.0 ** -22) / R ** 3
        err = abs(float(loss) - exact)
        print(f"R = {R}, {kind}: loss {float(loss):.6g}, exact {exact:.6g}, |difference| {err:.3e}, bound {bound:.3e}")
        assert cnt == inside.sum() or kind in ("seams", "vertices", "outside")  # (a face point may be inside in one precision only)
        assert err <= bound


@pytest.mark.parametrize("mode", [COUNTS, DENSITY])
@pytest.mark.parametrize("R", [3, 17])
def test_gradient_against_central_differences(R, mode):
    """gr_ref's gradient is the analytic gradient of the unquantised loss under the quantised grid's signs.  At a point whose eight
    vertices keep their sign over the step -- |D| / Q^3 of the quantised grid and |D| of the float64 grid both above four times
    the most a step can move a vertex, mu h inv_h, and the two signs equal -- and which stays inside its cell, the float64 loss
    is trilinear in that point, so its central difference along an axis is its derivative up to rounding."""
    lo, hi = BOUNDS[1]
    n, m, h = 40, 31, 1e-5
    a, c = pair("uniform", 20 + R, n, m, R, lo, hi)
    loss, inside, g1, g2, info = gr_ref(a, c, R, lo, hi, mode, full=True)
    _, Dn, _ = gr_exact(a, c, R, lo, hi, mode, full=True)
    Dq = np.zeros(R ** 3, F64)
    Dq[info["ids"]] = info["D"].astype(F64) / Q3
    ih = float(inv_h_of(R, lo, hi))
    checked, worst = 0, 0.0
    for x, g, which, mu, cnt in ((a, g1, 0, m if mode else 1, n), (c, g2, 1, n if mode else 1, m)):
        ins, cell, t, q1 = gr_points(x, R, lo, hi)
        ids, _ = gr_spread(cell, q1, R)
        margin = 4 * mu * h * ih
        for k in range(cnt):
            stable = (np.abs(Dq[ids[k]]) > margin).all() and (np.abs(Dn[ids[k]]) > margin).all() \
                and (np.sign(Dq[ids[k]]) == np.sign(Dn[ids[k]])).all()
            if not (ins[k] and stable and (t[k] > 4 * h * ih).all() and (t[k] < 1 - 4 * h * ih).all()):
                continue
            for ax in range(3):
                up, dn = x.astype(F64), x.astype(F64)
                up[k, ax] += h
                dn[k, ax] -= h
                lu = gr_exact(up, c, R, lo, hi, mode) if which == 0 else gr_exact(a, up, R, lo, hi, mode)
                ld = gr_exact(dn, c, R, lo, hi, mode) if which == 0 else gr_exact(a, dn, R, lo, hi, mode)
                cd = (lu - ld) / (2 * h)
                cc = 1 / cnt if mode else 1 / R ** 3
                # the float32 t is off by at most R 2^-22: 8 terms of two factors; one float32 rounding; the difference's own
                tol = ih * cc * 16 * R * 2.0 ** -22 + 2.0 ** -23 * abs(cd) + 64 * 2.0 ** -53 * max(lu, 1.0) / h
                worst = max(worst, abs(cd - float(g[k, ax])) / tol)
                assert abs(cd - float(g[k, ax])) <= tol, (which, k, ax, cd, float(g[k, ax]), tol)
            checked += 1
    print(f"R = {R}, mode {mode}: {checked} points checked, worst |central difference - gradient| / tolerance {worst:.3f}")
    assert checked >= 5


def test_layer_gradient_reference():
    """gr_grid_grad_ref against central differences of <gg, exact grid>, which is trilinear in a point inside its cell."""
    R, (lo, hi) = 5, BOUNDS[0]
    a = family("uniform", 9, 12, R, lo, hi)
    gg = np.random.RandomState(3).randn(R, R, R).astype(F32)
    g, tol = gr_grid_grad_ref(a, gg, R, lo, hi)
    h = 1e-6
    for k in range(12):
        for ax in range(3):
            up, dn = a.astype(F64), a.astype(F64)
            up[k, ax] += h
            dn[k, ax] -= h
            cd = (gr_exact_grids(up, R, lo, hi)[0] - gr_exact_grids(dn, R, lo, hi)[0]) @ gg.reshape(-1).astype(F64) / (2 * h)
            assert abs(cd - g[k, ax]) <= 1e-5 * max(1.0, abs(cd)), (k, ax, cd, g[k, ax])
    assert (tol > 0).all()


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_gridding_loss", "rf_gridding_loss_workspace_bytes", "rf_gridding", "rf_gridding_workspace_bytes", "rf_gridding_grad")


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
    assert f"#define RF_GR_Q {_raw.GR_Q}\n" in header and _raw.GR_Q == Q
    assert f"#define RF_GR_MAX_RES {_raw.GR_MAX_RES}\n" in header and _raw.GR_MAX_RES == 256
    assert f"#define RF_GR_MAX_POINTS {_raw.GR_MAX_POINTS}\n" in header and _raw.GR_MAX_POINTS == 65536
    assert "#define RF_GR_COUNTS 0\n" in header and "#define RF_GR_DENSITY 1\n" in header
    assert _raw.GR_MODES == {"counts": COUNTS, "density": DENSITY} and _raw.GR_BRICK == BRICK


def test_workspace_sizes():
    from rfnet_amd._lib import lib
    fl, fg = lib.rf_gridding_loss_workspace_bytes, lib.rf_gridding_workspace_bytes
    for shape in ((0, 10, 10, 8), (-1, 10, 10, 8), (2, 0, 10, 8), (2, 10, 0, 8), (2, -5, 10, 8), (2, 65537, 10, 8),
                  (2, 10, 65537, 8), (65536, 10, 10, 8), (2, 10, 10, 1), (2, 10, 10, 257), (2, 10, 10, 0), (2, 10, 10, -3)):
        assert fl(*shape, 0) == 0 and fl(*shape, 1) == 0, shape
    for shape in ((0, 10, 8), (-1, 10, 8), (2, 0, 8), (2, 65537, 8), (65536, 10, 8), (2, 10, 1), (2, 10, 257)):
        assert fg(*shape) == 0, shape
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for b, n, m, R in ((1, 1, 1, 2), (3, 300, 203, 17), (32, 2048, 16384, 64), (65535, 65536, 65536, 256)):
        nb3 = ((R + 15) // 16) ** 3
        base = r(4 * 2 * b * (nb3 + 1)) + r(8 * b * (n + m)) + r(8 * b * nb3)
        assert fl(b, n, m, R, 0) == base and fl(b, n, m, R, 1) == base + r(b * R ** 3), (b, n, m, R)
        assert fg(b, n, R) == r(4 * b * (nb3 + 1)) + r(8 * b * n)


P, WS, BIG = 0x10000, 0x200000, 1 << 60  # never dereferenced: every call below must return at its argument checks


def _loss(b=2, n=300, m=200, res=17, lo=-0.5, hi=0.5, mode=0, ws=WS, wsz=BIG, l1=P, l2=P, g1=P, g2=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 4  # xyz1, xyz2, loss, inside
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_gridding_loss(b, n, m, res, lo, hi, mode, t[0], t[1], l1, l2, t[2], t[3], g1, g2, ws, wsz, None)


def _layer(b=2, n=300, res=17, lo=-0.5, hi=0.5, ws=WS, wsz=BIG, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 3  # xyz, grid, inside
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_gridding(b, n, res, lo, hi, t[0], ln, t[1], t[2], ws, wsz, None)


def _layer_grad(b=2, n=300, res=17, lo=-0.5, hi=0.5, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 3  # xyz, grad_grid, grad_xyz
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_gridding_grad(b, n, res, lo, hi, t[0], ln, t[1], t[2], None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    nan, inf = float("nan"), float("inf")
    box = (dict(lo=nan), dict(hi=nan), dict(lo=-inf), dict(hi=inf), dict(lo=0.5, hi=0.5), dict(lo=0.5, hi=-0.5),
           dict(lo=1e39), dict(res=1), dict(res=0), dict(res=257), dict(res=-2))
    assert _loss(b=0) == OK and _loss(b=0, n=0, m=0, res=0, lo=nan, mode=7, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(m=-3), dict(b=0, n=-1), dict(b=0, res=-1), dict(n=0), dict(m=0), dict(n=65537),
                dict(m=65537), dict(b=65536), dict(mode=2), dict(mode=-1)) + box:
        assert _loss(**bad) == EINVAL, bad
    for k in range(4):
        assert _loss(null=k) == EINVAL, f"NULL tensor {k}"
        assert _loss(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _loss(g1=None) == EINVAL and _loss(g2=None) == EINVAL  # both gradients or neither
    assert _loss(g1=P + 2) == EINVAL and _loss(g2=P + 1) == EINVAL
    assert _loss(l1=P + 2) == EINVAL and _loss(l2=P + 1) == EINVAL
    assert _loss(ws=None) == EINVAL and _loss(ws=WS + 4) == EINVAL and _loss(ws=WS + 8) == EINVAL
    need = lib.rf_gridding_loss_workspace_bytes(2, 300, 200, 17, 1)
    less = lib.rf_gridding_loss_workspace_bytes(2, 300, 200, 17, 0)
    assert 0 < less < need
    assert _loss(wsz=need - 1) == EWORKSPACE and _loss(wsz=0) == EWORKSPACE
    assert _loss(g1=None, g2=None, wsz=less - 1) == EWORKSPACE
    assert _loss(wsz=0, l1=None, l2=None) == EWORKSPACE  # NULL counts mean "all"
    assert _loss(b=65535, n=65536, m=65536, res=256, mode=1, wsz=0) == EWORKSPACE  # the largest sizes are sizes
    assert _loss(res=2, lo=-3e38, hi=3e38, wsz=0) == EWORKSPACE

    assert _layer(b=0) == OK and _layer(b=0, n=0, res=0, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(b=0, n=-1), dict(n=0), dict(n=65537), dict(b=65536)) + box:
        assert _layer(**bad) == EINVAL, bad
        assert _layer_grad(**bad) == EINVAL, bad
    for k in range(3):
        assert _layer(null=k) == EINVAL and _layer(at=(k, P + 2)) == EINVAL, k
        assert _layer_grad(null=k) == EINVAL and _layer_grad(at=(k, P + 1)) == EINVAL, k
    assert _layer(ln=P + 2) == EINVAL and _layer_grad(ln=P + 2) == EINVAL
    assert _layer(ws=None) == EINVAL and _layer(ws=WS + 8) == EINVAL
    assert _layer(wsz=lib.rf_gridding_workspace_bytes(2, 300, 17) - 1) == EWORKSPACE
    assert _layer(b=65535, n=65536, res=256, ln=None, wsz=0) == EWORKSPACE
    assert _layer_grad(b=0) == OK


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, c = np.zeros((2, 4, 3), F32), np.zeros((2, 5, 3), F32)
    with pytest.raises(ValueError, match="xyz1"):
        _raw.gridding_loss(np.zeros((2, 4), F32), c, 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="xyz2"):
        _raw.gridding_loss(a, np.zeros((2, 5, 2), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="batch"):
        _raw.gridding_loss(a, np.zeros((3, 5, 3), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="mode"):
        _raw.gridding_loss(a, c, 8, -0.5, 0.5, mode="mean")
    for res in (1, 257, 0):
        with pytest.raises(ValueError, match="2 to 256"):
            _raw.gridding_loss(a, c, res, -0.5, 0.5)
        with pytest.raises(ValueError, match="2 to 256"):
            _raw.gridding(a, res, -0.5, 0.5)
    for lo, hi in ((0.5, 0.5), (1.0, -1.0), (float("nan"), 1.0), (0.0, float("inf")), (0.0, 1e39), (1.0, 1.0 + 1e-9)):
        with pytest.raises(ValueError, match="finite bounds"):
            _raw.gridding_loss(a, c, 8, lo, hi)
        with pytest.raises(ValueError, match="finite bounds"):
            _raw.gridding_grad(a, np.zeros((2, 8, 8, 8), F32), 8, lo, hi)
    with pytest.raises(ValueError, match="at least one point"):
        _raw.gridding_loss(np.zeros((2, 0, 3), F32), c, 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="65536"):
        _raw.gridding(np.zeros((1, 65537, 3), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="lengths1"):
        _raw.gridding_loss(a, c, 8, -0.5, 0.5, lengths1=[4, 5])
    with pytest.raises(ValueError, match="lengths2"):
        _raw.gridding_loss(a, c, 8, -0.5, 0.5, lengths2=[5])
    with pytest.raises(ValueError, match="lengths"):
        _raw.gridding(a, 8, -0.5, 0.5, lengths=[0, 1])
    with pytest.raises(ValueError, match="grad_grid"):
        _raw.gridding_grad(a, np.zeros((2, 8, 8, 7), F32), 8, -0.5, 0.5)
    with pytest.raises(ValueError, match="2 to 256"):
        glue.gridding_loss(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3), resolution=1)
    with pytest.raises(ValueError, match="finite bounds"):
        glue.gridding(a, bounds=(0.5, -0.5))
