"""GPU: the Chamfer gradient kernels and the fused loss ops against the float64 references of tests/chamfer_grad_ref.py
(checked on the CPU by tests/test_chamfer_grad_ref_host.py), element by element:
  nn_grad_kernel<LOSS, CNT>   (rf_nn_distance_grad, rf_chamfer_loss_grad and their _lengths forms) at a shape per launch
                              route -- sliced with zero-fill and atomic flush, a full 2048-point tile, a last tile of one
                              point, a tile larger than the cloud -- each case first asserting its route;
  grad_tile                   (rf_chamfer_step's sorted-space backward) at the smallest culled shapes;
  chamfer_loss_reduce_kernel  at the boundaries of its four-way unrolled loop;
  merge_pull(_grad)_kernel    over decfactor 0, tiny, usual, negative, large, with coincident pairs in every case.
Family A (a dyadic grid, proven exact) must come out bit for bit; family B within K U mag per element, K counted from
the roundings on the kernel's path (chamfer_grad_ref.py; measured ratios: profiles/chamfer_grad_bounds.txt).  Indices
are INPUTS of the backward: most cases need no forward pass.  Garbage indices stay inside the padded tensors, so a
wrong kernel shows as a wrong number."""
import zlib

import numpy as np
import pytest
import torch

import chamfer_grad_ref as G

pytestmark = pytest.mark.gpu
K = G.kernel_constants()
F32 = np.float32


def cu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def run_plain(a, c, gd1, i1, gd2, i2, l1=None, l2=None):
    from rfnet_amd import _raw as R
    return host(R.nn_distance_grad(cu(a), cu(c), cu(gd1), cu(i1), cu(gd2), cu(i2), lengths1=l1, lengths2=l2))


def run_loss(a, c, d1, i1, d2, i2, gl, l1=None, l2=None):
    from rfnet_amd import _raw as R
    return host(R.chamfer_loss_grad(cu(a), cu(c), cu(d1), cu(i1) if d1 is not None else None, cu(d2),
                                    cu(i2) if d2 is not None else None, cu(gl), lengths1=l1, lengths2=l2))


def pos_zero(x):
    return not x.any() and not np.signbit(x).any()


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def route_of(shape):
    b, n, m = shape
    r = G.grad_route(b, n, m, K)
    assert r == G.GRAD_SHAPES[shape], f"{shape} takes {r}, it is here for {G.GRAD_SHAPES[shape]}"
    return r


def idx_maker(orc, pattern, rng, b, n, m, l1=None, l2=None):
    if pattern == "nn":
        def f(a, c):
            e = orc.nn_distance(a, c)
            return e[1], e[3]
        return f
    return lambda a, c: (G.indices(pattern, rng, b, n, m, l1, l2), G.indices(pattern, rng, b, m, n, l2, l1))


GRAD_SHAPES = list(G.GRAD_SHAPES)


# ------------------------------------------------------------------ nn_grad_kernel, plain mode ------------------------------
@pytest.mark.parametrize("pattern", G.PATTERNS + ("nn",))
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_plain_exact(orc, shape, pattern):
    b, n, m = shape
    route_of(shape)
    rng = np.random.RandomState(seed_of(shape, pattern))
    a, c, gd1, i1, gd2, i2, e1, e2 = G.exact_case(rng, b, n, m, idx_maker(orc, pattern, rng, b, n, m))
    g1, g2 = run_plain(a, c, gd1, i1, gd2, i2)
    assert np.array_equal(g1, e1), f"grad_xyz1: {(g1 != e1).sum()} of {g1.size} elements differ"
    assert np.array_equal(g2, e2), f"grad_xyz2: {(g2 != e2).sum()} of {g2.size} elements differ"


B_CASES = [("randn", "uniform"), ("randn", "perm"), ("randn", "hub_first"), ("randn", "hub_last"), ("randn", "runs"),
           ("dup", "nn"), ("collapsed", "nn"), ("same", "nn")]


@pytest.mark.parametrize("kind,pattern", B_CASES)
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_plain_within_bound(orc, shape, kind, pattern):
    b, n, m = shape
    r1, r2 = route_of(shape)
    rng = np.random.RandomState(seed_of(shape, kind, pattern))
    a, c = G.clouds(kind, rng, b, n, m)
    i1, i2 = idx_maker(orc, pattern, rng, b, n, m)(a, c)
    gd1, gd2 = G.signed_gd(rng, (b, n)), G.signed_gd(rng, (b, m))
    g1, g2 = run_plain(a, c, gd1, i1, gd2, i2)
    f1, f2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2)
    G.assert_within(g1, f1, G.k_plain(r1[2]) * G.U * m1, f"nn_grad {shape} {kind} {pattern} grad_xyz1")
    G.assert_within(g2, f2, G.k_plain(r2[2]) * G.U * m2, f"nn_grad {shape} {kind} {pattern} grad_xyz2")


# ------------------------------------------------------------------ nn_grad_kernel, loss mode -------------------------------
@pytest.mark.parametrize("dirs", ["both", "dir1", "dir2"])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_loss_grad_within_bound(shape, dirs):
    b, n, m = shape
    r1, r2 = route_of(shape)
    rng = np.random.RandomState(seed_of(shape, dirs))
    a, c = G.clouds("randn", rng, b, n, m)
    pattern = ("uniform", "hub_last", "runs")[(b + n) % 3]
    i1, i2 = G.indices(pattern, rng, b, n, m), G.indices(pattern, rng, b, m, n)
    d1 = G.decade_dist(rng, (b, n)) if dirs != "dir2" else None
    d2 = G.decade_dist(rng, (b, m)) if dirs != "dir1" else None
    gl = G.signed_gd(rng, (b, 2))
    g1, g2 = run_loss(a, c, d1, i1, d2, i2, gl)
    f1, f2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl)
    G.assert_within(g1, f1, G.k_loss(r1[2]) * G.U * m1, f"loss_grad {shape} {dirs} grad_xyz1")
    G.assert_within(g2, f2, G.k_loss(r2[2]) * G.U * m2, f"loss_grad {shape} {dirs} grad_xyz2")


def test_loss_grad_coincident_pairs_give_the_reference_nan_mask():
    """dist = 0 exactly on coincident pairs (difference 0): 0.5 / sqrt(0) is inf and inf * 0 NaN, on the own row and on
    the winner's row -- in the float64 reference on the same fp32 inputs and in the kernel alike."""
    shape = (2, 3000, 2049)
    b, n, m = shape
    r1, r2 = route_of(shape)
    rng = np.random.RandomState(5)
    a, c = G.clouds("randn", rng, b, n, m)
    i1, i2 = G.indices("uniform", rng, b, n, m), G.indices("uniform", rng, b, m, n)
    d1, d2 = G.decade_dist(rng, (b, n)), G.decade_dist(rng, (b, m))
    for i in range(b):
        js = rng.choice(m, 200, replace=False)          # rows of c copied from their winner in a: dist2 = 0
        c[i, js] = a[i, i2[i, js]]
        d2[i, js] = 0.0
        rows = np.unique(i2[i, js[:60]], return_index=True)
        i1[i, rows[0]] = js[:60][rows[1]]               # rows of a whose winner is their copy in c: dist1 = 0
        d1[i, rows[0]] = 0.0
    gl = G.signed_gd(rng, (b, 2))
    g1, g2 = run_loss(a, c, d1, i1, d2, i2, gl)
    f1, f2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl)
    assert np.isnan(f1).any() and np.isnan(f2).any() and not np.isnan(f1).all() and not np.isnan(f2).all()
    G.assert_within(g1, f1, G.k_loss(r1[2]) * G.U * m1, "loss_grad coincident grad_xyz1")
    G.assert_within(g2, f2, G.k_loss(r2[2]) * G.U * m2, "loss_grad coincident grad_xyz2")


# ------------------------------------------------------------------ nn_grad_kernel, ragged forms ----------------------------
RAGGED_SHAPES = [(1, 100, 4096), (2, 3000, 2049), (300, 70, 33)]


def count_sets(shape, rng):
    """Count pairs (len1, len2) per shape: 1, the full size, 64, 65 and one past a slice boundary of each sliced
    direction (the sources of direction 1 are the points of xyz2, cut into `slices` ranges of ceil(m / slices))."""
    b, n, m = shape
    (_, _, s1, _), (_, _, s2, _) = G.grad_route(b, n, m, K)
    past1 = min(-(-n // s2) + 1, n)  # one past the first slice of direction 2's sources
    past2 = min(-(-m // s1) + 1, m)
    if b == 1:
        return [(np.array([x]), np.array([y])) for x, y in ((n, m), (1, 1), (64, past2), (65, 64), (past1, 65), (n, 1), (1, m))]
    if b == 2:
        return [(np.array(x), np.array(y)) for x, y in (((1, n), (m, 1)), ((past1, 64), (past2, 65)), ((65, n), (64, m)))]
    l1, l2 = rng.randint(1, n + 1, b), rng.randint(1, m + 1, b)
    l1[:6], l2[:6] = (1, n, 64, 65, n, 1), (m, 1, 1, m, m, 1)
    return [(l1, l2)]


def garbage_behind(x, cnt, value=np.nan):
    x = x.copy()
    for i in range(x.shape[0]):
        x[i, cnt[i]:] = value
    return x


@pytest.mark.parametrize("shape", RAGGED_SHAPES)
def test_ragged_plain_exact(shape):
    b, n, m = shape
    route_of(shape)
    rng = np.random.RandomState(seed_of(shape, "ragged A"))
    for l1, l2 in count_sets(shape, rng):
        a, c, gd1, i1, gd2, i2, e1, e2 = G.exact_case(rng, b, n, m, idx_maker(None, "uniform", rng, b, n, m, l1, l2), l1, l2)
        g1, g2 = run_plain(garbage_behind(a, l1), garbage_behind(c, l2), garbage_behind(gd1, l1), i1, garbage_behind(gd2, l2), i2, l1, l2)
        assert np.array_equal(g1, e1) and np.array_equal(g2, e2), (l1[:6], l2[:6])
        for g, ln in ((g1, l1), (g2, l2)):
            assert all(pos_zero(g[i, ln[i]:]) for i in range(b)), "rows behind a count are not +0.0"


@pytest.mark.parametrize("mode", ["plain", "loss"])
@pytest.mark.parametrize("shape", RAGGED_SHAPES)
def test_ragged_within_bound(shape, mode):
    b, n, m = shape
    r1, r2 = route_of(shape)
    rng = np.random.RandomState(seed_of(shape, mode, "ragged B"))
    for l1, l2 in count_sets(shape, rng):
        a, c = G.clouds("randn", rng, b, n, m)
        a, c = garbage_behind(a, l1), garbage_behind(c, l2)
        pattern = "hub_last" if (int(l1[0]) + int(l2[0])) % 2 else "uniform"
        i1, i2 = G.indices(pattern, rng, b, n, m, l1, l2), G.indices(pattern, rng, b, m, n, l2, l1)
        if mode == "plain":
            gd1, gd2 = garbage_behind(G.signed_gd(rng, (b, n)), l1), garbage_behind(G.signed_gd(rng, (b, m)), l2)
            g1, g2 = run_plain(a, c, gd1, i1, gd2, i2, l1, l2)
            f1, f2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2, l1, l2)
            k1, k2 = G.k_plain(r1[2]), G.k_plain(r2[2])
        else:
            d1, d2 = garbage_behind(G.decade_dist(rng, (b, n)), l1), garbage_behind(G.decade_dist(rng, (b, m)), l2)
            gl = G.signed_gd(rng, (b, 2))
            g1, g2 = run_loss(a, c, d1, i1, d2, i2, gl, l1, l2)
            f1, f2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl, l1, l2)
            k1, k2 = G.k_loss(r1[2]), G.k_loss(r2[2])
        G.assert_within(g1, f1, k1 * G.U * m1, f"ragged {mode} {shape} {l1[:3]} {l2[:3]} grad_xyz1")
        G.assert_within(g2, f2, k2 * G.U * m2, f"ragged {mode} {shape} {l1[:3]} {l2[:3]} grad_xyz2")
        for g, ln in ((g1, l1), (g2, l2)):
            assert all(pos_zero(g[i, ln[i]:]) for i in range(b)), "rows behind a count are not +0.0"


# ------------------------------------------------------------------ rf_chamfer_step, sorted route ---------------------------
STEP_SHAPES = list(G.STEP_SHAPES)


def run_step(a, c, gd1, gd2):
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    assert G.step_route(b, n, m, K) == (True, G.STEP_SHAPES[(b, n, m)]), G.step_route(b, n, m, K)
    assert lib.rf_chamfer_step_workspace_bytes(b, n, m) > lib.rf_nn_distance_workspace_bytes(b, n, m), \
        "the library does not take the sorted-space step at this shape"
    return host(R.ChamferStep(b, n, m, "cuda")(cu(a), cu(c), cu(gd1), cu(gd2)))


def forward_is_the_oracles(orc, a, c, out):
    e = orc.nn_distance(a, c)
    for got, exp, name in zip(out[:4], e, ("dist1", "idx1", "dist2", "idx2")):
        assert np.array_equal(got, exp), name
    return e[1], e[3]


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_step_sorted_exact(orc, shape, dup):
    """Grid clouds: massive distance ties (the forward's indices are held bit-exact there); resampled with duplicates
    they give long runs of equal winners through the segmented pre-sum."""
    b, n, m = shape
    rng = np.random.RandomState(seed_of(shape, dup))
    a, c = G.grid_clouds(rng, b, n, m)
    if dup:
        a = np.take_along_axis(a[:, :max(n // 3, 1)], rng.randint(0, max(n // 3, 1), (b, n))[..., None], 1)
        c = np.take_along_axis(c[:, :max(m // 40, 1)], np.sort(rng.randint(0, max(m // 40, 1), (b, m)), 1)[..., None], 1)
    gd1, gd2 = G.grid_gd(rng, (b, n)), G.grid_gd(rng, (b, m))
    out = run_step(a, c, gd1, gd2)
    i1, i2 = forward_is_the_oracles(orc, a, c, out)
    e1, e2 = G.nn_grad_exact(a, c, gd1, i1, gd2, i2)
    assert np.array_equal(out[4], e1), f"grad_xyz1: {(out[4] != e1).sum()} of {e1.size} elements differ"
    assert np.array_equal(out[5], e2), f"grad_xyz2: {(out[5] != e2).sum()} of {e2.size} elements differ"


@pytest.mark.parametrize("kind", ["randn", "collapsed", "same"])
@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_step_sorted_within_bound(orc, shape, kind):
    b, n, m = shape
    rng = np.random.RandomState(seed_of(shape, kind))
    a, c = G.clouds(kind, rng, b, n, m)
    gd1, gd2 = G.signed_gd(rng, (b, n)), G.signed_gd(rng, (b, m))
    out = run_step(a, c, gd1, gd2)
    i1, i2 = forward_is_the_oracles(orc, a, c, out)
    f1, f2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2)
    G.assert_within(out[4], f1, G.k_sorted() * G.U * m1, f"step {shape} {kind} grad_xyz1")
    G.assert_within(out[5], f2, G.k_sorted() * G.U * m2, f"step {shape} {kind} grad_xyz2")


# ------------------------------------------------------------------ chamfer_loss forward ------------------------------------
def loss_shapes():
    t = K["LR_TPB"]  # 0, 1 and 2 full trips of the four-way unrolled loop, and every tail length class
    return [(3, t - 1, 1), (3, t, 1), (2, 4 * t, 2), (2, 4 * t + 1, 2), (2, 8 * t + 1, 1)]


@pytest.mark.parametrize("want", ["both", "want1", "want2"])
@pytest.mark.parametrize("shape", loss_shapes())
def test_chamfer_loss_forward(orc, shape, want):
    from rfnet_amd import _raw as R
    b, n, m = shape
    rng = np.random.RandomState(seed_of(shape, want))
    a, c = G.clouds("randn", rng, b, n, m)
    w1, w2 = want != "want2", want != "want1"
    got = host(R.chamfer_loss(cu(a), cu(c), want1=w1, want2=w2))
    e = orc.nn_distance(a, c)
    d1, d2 = (e[0] if w1 else None), (e[2] if w2 else None)
    for g, x in zip(got[1:], (d1, e[1] if w1 else None, d2, e[3] if w2 else None)):
        assert (g is None and x is None) or np.array_equal(g, x)
    G.assert_within(got[0], G.loss(d1, d2)[0], G.loss_bound(d1, d2), f"chamfer_loss {shape} {want}")
    if not w1 or not w2:
        assert pos_zero(got[0][:, 0 if not w1 else 1])


@pytest.mark.parametrize("shape", loss_shapes())
def test_chamfer_loss_forward_lengths(orc, shape):
    from rfnet_amd import _raw as R
    b, n, m = shape
    t = K["LR_TPB"]
    rng = np.random.RandomState(seed_of(shape, "lengths"))
    a, c = G.clouds("randn", rng, b, n, m)
    l1 = np.array([1, n, min(n, 4 * t + 3)][:b])
    l2 = np.array([m, 1, m][:b])
    got = host(R.chamfer_loss(cu(garbage_behind(a, l1, 7.5)), cu(garbage_behind(c, l2, -7.5)), lengths1=l1, lengths2=l2))
    d1, d2 = np.zeros((b, n), F32), np.zeros((b, m), F32)
    for i in range(b):
        e = orc.nn_distance(a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]])
        d1[i, :l1[i]], d2[i, :l2[i]] = e[0][0], e[2][0]
        assert np.array_equal(got[1][i, :l1[i]], e[0][0]) and np.array_equal(got[3][i, :l2[i]], e[2][0])
        assert np.array_equal(got[2][i, :l1[i]], e[1][0]) and np.array_equal(got[4][i, :l2[i]], e[3][0])
    G.assert_within(got[0], G.loss(d1, d2, l1, l2)[0], G.loss_bound(d1, d2, l1, l2), f"chamfer_loss lengths {shape}")


# ------------------------------------------------------------------ merge_layer ----------------------------------------------
def merge_edges_forward(raw, new, idx, out, dec, keep):
    """The exact edges: s = 0 gives the raw winner itself; s / c > 104 (ratio exactly 0) gives the new point itself."""
    g = np.take_along_axis(raw, idx[..., None].astype(np.int64), 1)
    d = g.astype(np.float64) - new
    s = (d * d).sum(-1)
    x = s / (G.C_EPS + float(F32(dec)) ** 2)
    zero, far = keep & (s == 0), keep & (x > G.RATIO_ZERO_ABOVE)
    assert zero.any(), "the case has no coincident pair"
    assert np.array_equal(out[zero], g[zero]) and np.array_equal(out[far], new[far])
    return zero, far


@pytest.mark.parametrize("dec", G.MERGE_DECS)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("shape", [(2, 64, 300), (3, 1, 5), (2, 3000, 1024)])
def test_merge_layer_forward(orc, shape, ragged, dec):
    from rfnet_amd import _raw as R
    b, n, m = shape
    rng = np.random.RandomState(seed_of(shape, ragged, dec))
    lr = np.array([n, max(n // 3, 1), 1][:b]) if ragged else None
    ln = np.array([max(m // 2, 1), m, 1][:b]) if ragged else None
    raw, new, _, _ = G.merge_case(rng, b, n, m, dec, "uniform", lr, ln)
    cr, cn = G.counts_of(lr, b, n), G.counts_of(ln, b, m)
    idx = np.zeros((b, m), np.int32)
    for i in range(b):
        idx[i, :cn[i]] = orc.nn_distance(raw[i:i + 1, :cr[i]], new[i:i + 1, :cn[i]])[3][0]
    if ragged:
        out, gi = host(R.merge_layer(cu(garbage_behind(raw, cr, 7.5)), cu(garbage_behind(new, cn, -7.5)), dec, lengths=lr, lengths_new=ln))
    else:
        out, gi = host(R.merge_layer(cu(raw), cu(new), dec))
    assert np.array_equal(gi, idx), "idx2 is not the oracle's (padded rows: 0)"
    keep = np.arange(m)[None] < cn[:, None]
    ref, _ = G.merge_forward(raw, new, idx, dec, ln)
    G.assert_within(out, ref, G.merge_forward_bound(raw, new, idx, dec, ln), f"merge_layer {shape} dec {dec} ragged {ragged}")
    merge_edges_forward(raw, new, idx, out, dec, keep)
    assert pos_zero(out[~keep])
    if dec == 0.0:  # every non-coincident pair is beyond the pull's reach
        s0 = (np.take_along_axis(raw, idx[..., None].astype(np.int64), 1) == new).all(-1)
        assert np.array_equal(out[keep & ~s0], new[keep & ~s0])


MERGE_GRAD_SHAPES = [(1, 1, 1), (3, 64, 1023), (2, 300, 1025), (2, 2048, 4097), (4, 7, 16384)]


def check_merge_grad(shape, dec, pattern, lr=None, ln=None):
    from rfnet_amd import _raw as R
    b, n, m = shape
    rng = np.random.RandomState(seed_of(shape, dec, pattern, lr is None))
    raw, new, idx, go = G.merge_case(rng, b, n, m, dec, pattern, lr, ln)
    cr, cn = G.counts_of(lr, b, n), G.counts_of(ln, b, m)
    if lr is not None:
        gn, gd, gr = host(R.merge_layer_grad(cu(garbage_behind(raw, cr)), cu(garbage_behind(new, cn)), dec, cu(idx),
                                             cu(garbage_behind(go, cn)), want_raw=True, lengths=lr, lengths_new=ln))
    else:
        gn, gd, gr = host(R.merge_layer_grad(cu(raw), cu(new), dec, cu(idx), cu(go), want_raw=True))
    r = G.merge_grad_all(raw, new, idx, dec, go, lr, ln, K["MG_TPB"])
    what = f"merge_layer_grad {shape} dec {dec} {pattern}"
    G.assert_within(gn, r["grad_new"][0], r["grad_new"][1], what + " grad_new")
    G.assert_within(gr, r["grad_raw"][0], r["grad_raw"][1], what + " grad_raw")
    G.assert_within(gd, r["grad_dec"][0], r["grad_dec"][1], what + " grad_dec")
    # exact edges
    keep = r["keep"]
    zero, far = keep & (r["s"] == 0), keep & (r["x"] > G.RATIO_ZERO_ABOVE)
    assert zero.any(), "the case has no coincident pair"
    assert not gn[zero].any(), "s = 0: grad_new is not 0"
    assert np.array_equal(gn[far], go[far]), "s / c > 104: grad_new is not grad_out"
    assert pos_zero(gn[~keep])
    for i in range(b):
        assert pos_zero(gr[i, cr[i]:]), "grad_raw behind len_raw is not +0.0"
        # a raw row whose only term is a coincident pair gets that pair's grad_out; one named by far pairs only gets 0
        single = np.flatnonzero(r["terms"][i] == 1)
        owner = np.full(n, -1)
        owner[r["idx"][i, :cn[i]]] = np.arange(cn[i])
        for k in single[:64]:
            j = owner[k]
            if zero[i, j]:
                assert np.array_equal(gr[i, k], go[i, j]), "s = 0: the pair's grad_raw term is not grad_out"
        named = np.zeros(n, bool)
        named[r["idx"][i, :cn[i]][~far[i, :cn[i]]]] = True
        assert not gr[i, ~named].any(), "s / c > 104: a contribution to grad_raw"
    if dec == 0.0:  # every non-coincident pair is beyond the pull's reach
        assert (zero | far | ~keep).all() and not gd.any(), "dec = 0: a contribution to grad_dec"


@pytest.mark.parametrize("pattern", ["uniform", "hub_last", "perm"])
@pytest.mark.parametrize("dec", G.MERGE_DECS)
@pytest.mark.parametrize("shape", MERGE_GRAD_SHAPES)
def test_merge_layer_grad(shape, dec, pattern):
    check_merge_grad(shape, dec, pattern)


@pytest.mark.parametrize("dec", [0.0, 0.07, 1e3])
@pytest.mark.parametrize("shape", MERGE_GRAD_SHAPES)
def test_merge_layer_grad_lengths(shape, dec):
    b, n, m = shape
    lr = np.array([n, max(n // 2, 1), 1, n][:b])
    ln = np.array([max(m - 1, 1), m, 1, K["MG_TPB"] + 1][:b])
    check_merge_grad(shape, dec, "uniform", lr, np.minimum(ln, m))
