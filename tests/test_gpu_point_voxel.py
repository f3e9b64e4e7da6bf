"""GPU: rf_voxelize_mean, rf_trilinear_devoxelize and their backward passes (include/rfops.h) against the numpy
restatements of the contract in tests/test_point_voxel_host.py.

Bit-equal: the devoxelization's forward and grad_xyz and the voxelization's backward (every operation is a prescribed IEEE
operation); cnt and inside; the two scatters -- vol of the voxelization, grad_vol of the devoxelization -- wherever the double sums
are exact: integer features / gradients in [-64, 64], and for the weighted scatter the box [0, R - 1] (inv_h is exactly 1) with
coordinates that are multiples of 1/8, so that every weight is a multiple of 2^-9 and every partial sum a multiple of 2^-9 below
2^31.  Within the header's bars for random float32 values: 2^-23 |exact| + 2^-52 sum |terms| for vol, 2^-23 |exact| + k 2^-52
sum |terms| for grad_vol, against the exact sums by math.fsum.

The grids are the smallest with one cell, one sub-brick and a sub-brick seam (R = 2, 3, E, E + 1, 2 E + 1, 4 E + 1 with E = 8, the
scatters' sub-brick edge; 17 and 33 also cross the seams of the counting sort's 16-bricks), the channels straddle the chunk of 8
(1, 7, 8, 9, 64, 65), the clouds have 1, 63, 64, 65 and 257 points around the wave of 64 records and the workgroup of 256."""
import numpy as np
import pytest
import torch

from test_gridding_host import BOUNDS, F32
from test_point_voxel_host import (BRICK, CHUNK, devox_grad_ref, devox_grad_tol, devox_ref, family, volume, vox_grad_ref, vox_ref,
                                   vox_tol)

pytestmark = pytest.mark.gpu

E = BRICK
GRIDS = (2, 3, E, E + 1, 2 * E + 1, 4 * E + 1)
SIZES = (1, 63, 64, 65, 257)
CHANNELS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 8 * CHUNK, 8 * CHUNK + 1)
KINDS = ("uniform", "seams", "collapsed", "vertices")
I32, F64 = np.int32, np.float64


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype} != {ref.shape} {ref.dtype}"
    bad = np.flatnonzero(got.view(np.uint32).ravel() != ref.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {bad[0]}: {got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def within(got, exact, tol, what):
    """-> the worst error / bar; the figure is in the assertion message"""
    err = np.abs(got.astype(F64) - exact)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    assert (err <= tol).all(), f"{what}: worst error / bar {worst:.3f}"
    return worst


def check_prescribed(x, vol, lo, hi, ln=None, what="", seed=0):
    """the outputs with prescribed bits -- devoxelize, its grad_xyz, the voxelization's backward, cnt and inside -- bit-equal"""
    from rfnet_amd import _raw
    b, n = x.shape[:2]
    c, R = vol.shape[1], vol.shape[2]
    tl = None if ln is None else cu(ln)
    rng = np.random.RandomState(seed)
    gf = (rng.randn(b, n, c) * np.exp(2 * rng.randn(b, n, 1))).astype(F32)
    feat, inside = (t.cpu().numpy() for t in _raw.trilinear_devoxelize(cu(x), cu(vol), lo, hi, tl))
    gx = _raw.trilinear_devoxelize_grad(cu(x), cu(vol), cu(gf), lo, hi, tl)[1].cpu().numpy()
    _, cnt, inside2 = (t.cpu().numpy() for t in _raw.avg_voxelize(cu(x), cu(gf), R, lo, hi, tl))
    back = _raw.avg_voxelize_grad(cu(x), cu(cnt), cu(vol), lo, hi, tl).cpu().numpy()
    assert feat.shape == (b, n, c) and gx.shape == (b, n, 3) and cnt.shape == (b, R, R, R) and back.shape == (b, n, c)
    for i in range(b):
        L = None if ln is None else ln[i]
        w = f"{what} sample {i}"
        rf, ri = devox_ref(x[i], vol[i], lo, hi, L)
        assert int(inside[i]) == ri == int(inside2[i]), f"{w}: inside {inside[i]}, {inside2[i]} != {ri}"
        same_bits(feat[i], rf, f"{w}: feat")
        same_bits(gx[i], devox_grad_ref(x[i], vol[i], gf[i], lo, hi, L)[3], f"{w}: grad_xyz")
        rc = vox_ref(x[i], gf[i], R, lo, hi, L)[2]
        assert np.array_equal(cnt[i], rc) and cnt.dtype == I32, f"{w}: cnt differs at {np.flatnonzero(cnt[i] != rc)[:4]}"
        same_bits(back[i], vox_grad_ref(x[i], rc, vol[i], lo, hi, L), f"{w}: grad_feat of the voxelization")
    return feat, gx, cnt, back


def check_scatters(x, lo, hi, R, c, ln=None, what="", seed=0):
    """random float32 values: vol and grad_vol inside the header's bars, +0 where nothing fell -> the worst error / bar"""
    from rfnet_amd import _raw
    b, n = x.shape[:2]
    tl = None if ln is None else cu(ln)
    rng = np.random.RandomState(seed)
    f = (rng.randn(b, n, c) * np.exp(4 * rng.randn(b, n, 1))).astype(F32)
    base = np.stack([volume(seed + i, c, R, wild=False) for i in range(b)])
    vol = _raw.avg_voxelize(cu(x), cu(f), R, lo, hi, tl)[0].cpu().numpy()
    gv = _raw.trilinear_devoxelize_grad(cu(x), cu(base), cu(f), lo, hi, tl, want_xyz=False)[0].cpu().numpy()
    assert vol.shape == gv.shape == (b, c, R, R, R)
    worst = [0.0, 0.0]
    for i in range(b):
        L = None if ln is None else ln[i]
        mean, mag, cnt, _ = vox_ref(x[i], f[i], R, lo, hi, L, fsum=True)
        worst[0] = max(worst[0], within(vol[i], mean, vox_tol(mean, mag), f"{what} sample {i}: vol"))
        assert not vol[i][:, cnt == 0].view(np.uint32).any()
        G, A, k, _ = devox_grad_ref(x[i], base[i], f[i], lo, hi, L, fsum=True)
        worst[1] = max(worst[1], within(gv[i], G, devox_grad_tol(G, A, k), f"{what} sample {i}: grad_vol"))
        assert not gv[i][:, k == 0].view(np.uint32).any()
    print(f"{what}: random values, worst error / bar: vol {worst[0]:.3f}, grad_vol {worst[1]:.3f}")
    return worst


def exact_case(kind, seed, b, n, R, c):
    """-> (x (b, n, 3) on multiples of 1/8 in the box [0, R - 1], integer values f (b, n, c) in [-64, 64], a volume) after
    checking on the CPU that the reference's own sums are exact for them: fsum and a plain double sum in two orders agree"""
    lo, hi = 0.0, R - 1.0
    rng = np.random.RandomState(seed)
    x = np.stack([np.round(family(kind, seed + i, n, R, lo, hi) * 8) / 8 for i in range(b)]).astype(F32)
    f = rng.randint(-64, 65, (b, n, c)).astype(F32)
    base = np.stack([volume(seed + i, c, R) for i in range(b)])
    refs = []
    for i in range(b):
        forms = [vox_ref(x[i], f[i], R, lo, hi, **kw) for kw in (dict(), dict(reverse=True), dict(fsum=True))]
        assert forms[0][0].tobytes() == forms[1][0].tobytes() == forms[2][0].tobytes(), "the voxelization's reference sums are not exact"
        gforms = [devox_grad_ref(x[i], base[i], f[i], lo, hi, **kw) for kw in (dict(), dict(reverse=True), dict(fsum=True))]
        assert gforms[0][0].tobytes() == gforms[1][0].tobytes() == gforms[2][0].tobytes(), "the scatter's reference sums are not exact"
        refs.append((forms[0], gforms[0]))
    return x, f, base, refs


def check_exact(kind, seed, b, n, R, c, what):
    from rfnet_amd import _raw
    lo, hi = 0.0, R - 1.0
    x, f, base, refs = exact_case(kind, seed, b, n, R, c)
    vol, cnt, inside = (t.cpu().numpy() for t in _raw.avg_voxelize(cu(x), cu(f), R, lo, hi))
    gv = _raw.trilinear_devoxelize_grad(cu(x), cu(base), cu(f), lo, hi, want_xyz=False)[0].cpu().numpy()
    for i in range(b):
        (mean, _, rc, ri), (G, _, _, _) = refs[i]
        assert int(inside[i]) == ri and np.array_equal(cnt[i], rc), f"{what} sample {i}: cnt / inside"
        same_bits(vol[i], mean.astype(F32), f"{what} sample {i}: vol of integer features")
        same_bits(gv[i], G.astype(F32), f"{what} sample {i}: grad_vol of integer gradients")
    return x, f, base, vol, gv


def channels(k, R, n):
    """the channel count of a case: all six in turn; at R = 4 E + 1, where the references' arrays are large, the two wide ones go
    to the largest cloud only (tests stay quick)"""
    return CHANNELS[k % 6] if R <= 2 * E + 1 or n == SIZES[-1] else CHANNELS[k % 4]


# ---- 1. the small grids --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", GRIDS)
def test_prescribed_outputs_on_small_grids(R, kind):
    for k, n in enumerate(SIZES):
        for j, (lo, hi) in enumerate(BOUNDS):
            c = channels(k + 3 * j + R, R, n)
            x = np.stack([family(kind, 10 * k + s + j, n, R, lo, hi) for s in range(2)])
            vol = np.stack([volume(k + R + s, c, R) for s in range(2)])
            check_prescribed(x, vol, lo, hi, what=f"R = {R}, {kind}, n = {n}, c = {c}, box {lo, hi}", seed=k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", GRIDS)
def test_scatters_on_small_grids(R, kind):
    for k, n in enumerate(SIZES):
        c = channels(k + R, R, n)
        check_exact(kind, 20 * k + R, 2, n, R, c, f"R = {R}, {kind}, n = {n}, c = {c}")
        lo, hi = BOUNDS[k % 2]
        x = np.stack([family(kind, 30 * k + s, n, R, lo, hi) for s in range(2)])
        check_scatters(x, lo, hi, R, c, what=f"R = {R}, {kind}, n = {n}, c = {c}, box {lo, hi}", seed=k)


def test_every_channel_count_at_the_seams():
    R, (lo, hi) = 2 * E + 1, BOUNDS[1]
    for c in CHANNELS + (2 * CHUNK + 1,):
        x = np.stack([family(k, 5 + c, 257, R, lo, hi) for k in ("seams", "outside")])
        check_prescribed(x, np.stack([volume(c + s, c, R) for s in range(2)]), lo, hi, what=f"c = {c}", seed=c)
        check_scatters(x, lo, hi, R, c, what=f"c = {c}", seed=c)
        check_exact("seams", c, 2, 257, R, c, f"c = {c}")


def test_every_output_element_is_written():
    """the four entries straight through the C ABI into outputs filled with 0xFF bytes: the bits of the plain calls, nothing left"""
    from rfnet_amd import _raw
    from rfnet_amd._lib import lib
    R, b, n, c = 2 * E + 1, 2, 257, CHUNK + 1
    lo, hi = 0.0, R - 1.0  # exact sums (exact_case): the bits of the two scatters are promised, call after call
    x, f, base, refs = exact_case("outside", 3, b, n, R, c)  # part of the cloud is outside the box
    ln = np.array([n, 129], I32)
    tx, tf, tv, tl = cu(x), cu(f), cu(base), cu(ln)
    poison = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device="cuda")  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731
    ws = torch.empty(max(lib.rf_voxelize_mean_workspace_bytes(b, n, R), 16), dtype=torch.uint8, device="cuda")
    vol, cnt, inside = poison(b, c, R, R, R), poison(b, R, R, R), poison(b)
    assert lib.rf_voxelize_mean(b, n, c, R, lo, hi, p(tx), p(tl), p(tf), p(vol), p(cnt), p(inside), p(ws), ws.numel(), None) == 0
    gf = poison(b, n, c)
    assert lib.rf_voxelize_mean_grad(b, n, c, R, lo, hi, p(tx), p(tl), p(cnt), p(tv), p(gf), None) == 0
    feat, inside2 = poison(b, n, c), poison(b)
    assert lib.rf_trilinear_devoxelize(b, n, c, R, lo, hi, p(tx), p(tl), p(tv), p(feat), p(inside2), None) == 0
    gv, gx = poison(b, c, R, R, R), poison(b, n, 3)
    assert lib.rf_trilinear_devoxelize_grad(b, n, c, R, lo, hi, p(tx), p(tl), p(tv), p(tf), p(gv), p(gx), p(ws), ws.numel(), None) == 0
    torch.cuda.synchronize()
    plain = _raw.avg_voxelize(tx, tf, R, lo, hi, tl)
    for got, ref, name in zip((vol, cnt, inside), plain, ("vol", "cnt", "inside")):
        assert bits(got) == bits(ref), name
    assert bits(gf) == bits(_raw.avg_voxelize_grad(tx, plain[1], tv, lo, hi, tl))
    plain = _raw.trilinear_devoxelize(tx, tv, lo, hi, tl)
    assert bits(feat) == bits(plain[0]) and bits(inside2) == bits(plain[1]) == bits(inside)
    plain = _raw.trilinear_devoxelize_grad(tx, tv, tf, lo, hi, tl)
    assert bits(gv) == bits(plain[0]) and bits(gx) == bits(plain[1])
    for i in range(b):
        mean, _, rc, ri = vox_ref(x[i], f[i], R, lo, hi, ln[i])
        assert 0 < ri < ln[i] and int(inside[i]) == ri and np.array_equal(cnt[i].cpu().numpy(), rc)
        same_bits(vol[i].cpu().numpy().view(F32), mean.astype(F32), f"sample {i}: vol")
        same_bits(feat[i].cpu().numpy().view(F32), devox_ref(x[i], base[i], lo, hi, ln[i])[0], f"sample {i}: feat")
        assert not feat[i, ln[i]:].any() and not gf[i, ln[i]:].any() and not gx[i, ln[i]:].any()


# ---- 2. the collapsed and the larger cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [CHUNK, 8 * CHUNK])
def test_collapsed_cloud(c):
    """2048 points in one cell: the contention case of the LDS adds -- at most eight vertices take every addition"""
    x, f, base, vol, gv = check_exact("collapsed", c, 1, 2048, 2 * E + 1, c, f"collapsed, c = {c}")
    assert (vol != 0).any(axis=1).sum() <= 8 and (gv != 0).any(axis=1).sum() <= 8
    lo, hi = BOUNDS[0]
    xr = family("collapsed", c, 2048, 2 * E + 1, lo, hi)[None]
    check_scatters(xr, lo, hi, 2 * E + 1, c, what=f"collapsed, c = {c}", seed=c)


def test_r256_with_few_points():
    """the many-empty-bricks case: 4096 bricks and 32768 sub-bricks for 257 points"""
    lo, hi = BOUNDS[1]
    x = family("seams", 8, 257, 256, lo, hi)[None]
    check_prescribed(x, volume(4, 1, 256)[None], lo, hi, what="R = 256, c = 1, n = 257")
    check_scatters(x, lo, hi, 256, 1, what="R = 256, c = 1, n = 257")


def test_pvcnn_size():
    lo, hi = BOUNDS[0]
    b, n, R, c = 2, 2048, 32, 64
    x = np.stack([family("uniform", 1, n, R, lo, hi), family("seams", 2, n, R, lo, hi)])
    feat, gx, cnt, back = check_prescribed(x, np.stack([volume(s, c, R) for s in range(b)]), lo, hi, what="b = 2, n = 2048, R = 32, c = 64")
    assert cnt.reshape(b, -1).sum(1).tolist() == [n, n]
    check_scatters(x, lo, hi, R, c, what="b = 2, n = 2048, R = 32, c = 64")
    check_exact("uniform", 3, b, n, R, c, "b = 2, n = 2048, R = 32, c = 64")


# ---- 3. purity ---------------------------------------------------------------------------------------------------------------------
def test_ragged_calls_are_the_sliced_calls():
    from rfnet_amd import _raw
    R, c, n = 2 * E + 1, CHUNK + 1, 257
    lo, hi = 0.0, R - 1.0
    kinds = ("uniform", "seams", "outside", "collapsed")
    x = np.stack([np.round(family(k, 30 + i, n, R, lo, hi) * 8) / 8 for i, k in enumerate(kinds)]).astype(F32)
    ln = np.array([n, 1, 129, 64], I32)
    rng = np.random.RandomState(2)
    f = rng.randint(-64, 65, (4, n, c)).astype(F32)  # exact sums: the bits of the order-free outputs are promised too
    vol = np.stack([volume(i, c, R) for i in range(4)])

    def run(xx, ff, vv, ll):
        v, k, ins = _raw.avg_voxelize(xx, ff, R, lo, hi, ll)
        feat, ins2 = _raw.trilinear_devoxelize(xx, vv, lo, hi, ll)
        gv, gx = _raw.trilinear_devoxelize_grad(xx, vv, ff, lo, hi, ll)
        return v, k, ins, _raw.avg_voxelize_grad(xx, k, vv, lo, hi, ll), feat, ins2, gv, gx

    POINTWISE = (3, 4, 7)  # the outputs with a row per point
    outs = []
    for fill in (np.nan, 1e30):  # what the rows behind the counts hold changes nothing
        xp, fp = x.copy(), f.copy()
        for i in range(4):
            xp[i, ln[i]:] = fill
            fp[i, ln[i]:] = fill
        got = run(cu(xp), cu(fp), cu(vol), cu(ln))
        outs.append(tuple(bits(t) for t in got))
        assert outs[-1] == tuple(bits(t) for t in run(cu(xp), cu(fp), cu(vol), cu(ln))), "two calls differ"
    assert outs[0] == outs[1]
    for i in range(4):
        L = int(ln[i])
        mean, _, rc, ri = vox_ref(x[i], f[i], R, lo, hi, L)
        same_bits(got[0][i].cpu().numpy(), mean.astype(F32), f"ragged sample {i}: vol")
        assert int(got[2][i]) == ri == int(got[5][i]) and np.array_equal(got[1][i].cpu().numpy(), rc)
        same_bits(got[4][i].cpu().numpy(), devox_ref(x[i], vol[i], lo, hi, L)[0], f"ragged sample {i}: feat")
        sliced = run(cu(x[i:i + 1, :L]), cu(f[i:i + 1, :L]), cu(vol[i:i + 1]), None)  # the sliced cloud
        one = run(cu(xp[i:i + 1]), cu(fp[i:i + 1]), cu(vol[i:i + 1]), cu(ln[i:i + 1]))  # the batch slice
        for j, (s, o, g) in enumerate(zip(sliced, one, got)):
            assert bits(o) == bits(g[i:i + 1]), f"batch slice {i}, output {j}"
            assert bits(s) == bits(g[i:i + 1, :L] if j in POINTWISE else g[i:i + 1]), f"sliced call {i}, output {j}"
            if j in POINTWISE:
                assert not g[i, L:].cpu().numpy().view(np.uint32).any(), f"sample {i}, output {j}: rows behind the count"
    # counts outside [1, n] are clamped by the kernels
    wild = run(cu(x), cu(f), cu(vol), cu(np.array([9999, -5, 129, 64], I32)))
    ref = run(cu(x), cu(f), cu(vol), cu(ln))
    assert all(bits(a) == bits(r) for a, r in zip(wild, ref))


# ---- 4. autograd -------------------------------------------------------------------------------------------------------------------
def test_glue_through_autograd():
    from rfnet_amd import _raw, glue
    R, c, n = E + 1, 5, 130
    lo, hi = 0.0, R - 1.0  # with coordinates on multiples of 1/8 and integer gradients the scatters' sums are exact: equal bits
    kinds = ("uniform", "seams", "outside", "collapsed")
    x = np.stack([np.round(family(k, 40 + i, n, R, lo, hi) * 8) / 8 for i, k in enumerate(kinds)]).astype(F32)
    ln = np.array([n, 1, 129, 64], I32)
    rng = np.random.RandomState(1)
    tx, tf = cu(x).requires_grad_(), cu(rng.randint(-64, 65, (4, n, c)).astype(F32)).requires_grad_()
    vol, cnt, inside = glue.avg_voxelize(tx, tf, R, (lo, hi), lengths=ln, return_counts=True)
    raw = _raw.avg_voxelize(tx.detach(), tf.detach(), R, lo, hi, ln)
    assert vol.shape == (4, c, R, R, R) and torch.equal(vol.detach(), raw[0]) and torch.equal(cnt, raw[1]) and torch.equal(inside, raw[2])
    assert vol.requires_grad and not cnt.requires_grad and not inside.requires_grad
    gv = cu(rng.randint(-64, 65, (4, c, R, R, R)).astype(F32))
    (vol * gv).sum().backward()
    assert tx.grad is None  # piecewise constant in the points
    assert bits(tf.grad) == bits(_raw.avg_voxelize_grad(tx.detach(), cnt, gv, lo, hi, ln)) and tf.grad.abs().max() > 0
    assert not glue.avg_voxelize(tx, tf.detach(), R, (lo, hi), lengths=ln).requires_grad
    assert torch.equal(glue.avg_voxelize(tx, tf, R, (lo, hi), lengths=ln).detach(), raw[0])

    tv = cu(rng.randint(-8, 9, (4, c, R, R, R)).astype(F32)).requires_grad_()
    feat = glue.trilinear_devoxelize(tx, tv, (lo, hi), lengths=ln)
    assert feat.shape == (4, n, c) and torch.equal(feat.detach(), _raw.trilinear_devoxelize(tx.detach(), tv.detach(), lo, hi, ln)[0])
    g = cu(rng.randint(-64, 65, (4, n, c)).astype(F32))
    (feat * g).sum().backward()
    rv, rx = _raw.trilinear_devoxelize_grad(tx.detach(), tv.detach(), g, lo, hi, ln)
    assert bits(tx.grad) == bits(rx) and tx.grad.abs().max() > 0
    assert bits(tv.grad) == bits(rv) and tv.grad.abs().max() > 0
    # pcd.requires_grad = False skips the xyz gradient: the raw call is made without it
    calls = []
    real = _raw.trilinear_devoxelize_grad
    try:
        _raw.trilinear_devoxelize_grad = lambda *a, **k: (calls.append(k.get("want_xyz")), real(*a, **k))[1]
        tv.grad = None
        (glue.trilinear_devoxelize(tx.detach(), tv, (lo, hi), lengths=ln) * g).sum().backward()
        (glue.trilinear_devoxelize(tx, tv.detach(), (lo, hi), lengths=ln) * g).sum().backward()
    finally:
        _raw.trilinear_devoxelize_grad = real
    assert [bool(k) for k in calls] == [False, True] and tv.grad is not None
    # numpy in, numpy out
    out = _raw.trilinear_devoxelize(x, tv.detach().cpu().numpy(), lo, hi, ln)
    assert isinstance(out[0], np.ndarray) and out[0].tobytes() == bits(feat)


# ---- 5. the chain: voxelize -> (a stand-in for the 3-D convolution) -> devoxelize, eager and replayed ------------------------------
def stand_in(vol):
    """what stands where PVCNN's 3-D convolutions do, fixed and exact in float32 (powers of two): the channels scaled by 1 / 2, and
    their negatives doubled, stacked -> (b, 2 c, R, R, R).  The same code serves torch and numpy."""
    cat = torch.cat if isinstance(vol, torch.Tensor) else np.concatenate
    return cat([vol * 0.5, vol * -2.0], 1)


def test_chain_eager_and_from_a_graph():
    from rfnet_amd import glue
    lo, hi = BOUNDS[0]
    b, n, R, c = 2, 2048, 16, 4
    rng = np.random.RandomState(5)
    P = [np.stack([family(k, 7 + 10 * v + i, n, R, lo, hi) for i, k in enumerate(("uniform", "seams"))]) for v in range(2)]
    Fs = [rng.randint(-64, 65, (b, n, c)).astype(F32) for v in range(2)]
    Ls = [np.array([n, 1500], I32), np.array([700, n], I32)]
    tp, tf, tl = cu(P[0]), cu(Fs[0]), cu(Ls[0])

    def run():
        vol, cnt, inside = glue.avg_voxelize(tp, tf, R, (lo, hi), lengths=tl, return_counts=True)
        return vol, inside, glue.trilinear_devoxelize(tp, stand_in(vol), (lo, hi), lengths=tl)

    def compare(got, v, what):
        for i in range(b):
            mean, _, _, ri = vox_ref(P[v][i], Fs[v][i], R, lo, hi, Ls[v][i])
            same_bits(got[0][i].cpu().numpy(), mean.astype(F32), f"{what}: volume of sample {i}")
            assert int(got[1][i]) == ri
            ref = devox_ref(P[v][i], stand_in(mean.astype(F32)[None])[0], lo, hi, Ls[v][i])[0]
            same_bits(got[2][i].cpu().numpy(), ref, f"{what}: features of sample {i}")

    compare(run(), 0, "eager")
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    compare(out, 0, "replay")
    first = bits(out[2])
    tp.copy_(cu(P[1]))  # the inputs and the counts change in place, on the device: nothing is read back
    tf.copy_(cu(Fs[1]))
    tl.copy_(cu(Ls[1]))
    graph.replay()
    torch.cuda.synchronize()
    compare(out, 1, "replay after the inputs and the counts changed")
    assert bits(out[2]) != first
