"""GPU: the bins and the boxes of the register-resident sort of the culled Chamfer (nnp_sort_reg_kernel, nn_pruned.hip) on
inputs that sit on the instructions they are made of: a bin is one fma and one saturating float-to-byte conversion
(v_cvt_pk_u8_f32), the boxes are bare v_min_f32 / v_max_f32 over coordinates canonicalised once, and the Chamfer's private
sorts leave out the non-finite flag that only the ball query reads.

The order the sort produces only steers the culling, so every case is the culled route against the dense sweep, bit for bit
(rf_nn_distance, mode "culled" vs "dense").  What the sort itself must keep is checked on the sorted handle (rf_nn_sort):
`orig` is a permutation plus padding -- the two workgroups of a split cloud (8193 points and more) each bin EVERY point and keep
their own slice, so a point they binned differently would be lost or doubled --, every 16- and 64-record box contains its
records, and a NaN coordinate is in no box: no bound is a NaN, quiet or signalling.  (An infinite coordinate is a bound like any
other: it orders.)  rf_chamfer_step takes the same sort without the flag: two shapes at the smallest batch size that takes the
sorted-space step (asserted, as tests/test_gpu_sort_valu_tables.py does), gradients against rf_nn_distance_grad at that file's
bar (rel 1e-5 + 1e-5 of the largest term).  The flag where it is needed: the ball query over a handle of a cloud that holds a NaN
equals its scan form.

Inputs: every coordinate on a k / 256 lattice of the cloud's extent with both ends present (bins 0 and 255; where rounding and
truncation differ), every point on a corner of the box, no extent on one axis, extents of 1e30 and 1e-30, -0.0 and denormals,
+-inf with a quiet and two signalling NaNs (bit patterns 0x7FA00000 and 0xFFA00001), resample_pcd duplicates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(64, 100), (2048, 2048), (8193, 2048), (16384, 512)]  # one slab | four slabs | the smallest split cloud | seven slabs, split


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def lattice(rng, n, b=B):
    """lo + k * ext / 256, k in 0..256: sample 0 in a frame where that is exact (lo -1, ext 2), the others where it rounds."""
    k = rng.randint(0, 257, (b, n, 3))
    if n >= 2:
        k[:, 0], k[:, n - 1] = 0, 256  # both ends of every axis are there
    lo = np.array([-1.0] + [0.3 + 1.7 * i for i in range(1, b)], np.float32)[:, None, None]
    ext = np.array([2.0] + [3.7 * i for i in range(1, b)], np.float32)[:, None, None]
    return (lo + k.astype(np.float32) * (ext / np.float32(256))).astype(np.float32)


def corners(rng, n, b=B):
    """Every point on a corner of the cloud's box: each coordinate is its axis' minimum or maximum."""
    lo, hi = rng.randn(b, 1, 3).astype(np.float32) - 2, rng.randn(b, 1, 3).astype(np.float32) + 2
    x = np.where(rng.randint(0, 2, (b, n, 3)) == 1, hi, lo).astype(np.float32)
    if n >= 2:
        x[:, 0], x[:, n - 1] = lo[:, 0], hi[:, 0]
    return x


def flat_axis(rng, n, b=B):
    x = rng.randn(b, n, 3).astype(np.float32)
    for bi in range(b):
        x[bi, :, (1 + bi) % 3] = np.float32(-0.625)
    return x


def huge(rng, n, b=B):
    return (rng.rand(b, n, 3).astype(np.float32) - np.float32(0.5)) * np.float32(1e30)


def tiny(rng, n, b=B):
    return (rng.rand(b, n, 3).astype(np.float32) - np.float32(0.5)) * np.float32(1e-30)


def zeros_and_denormals(rng, n, b=B):
    """Sample 0: -0.0, +0.0 and denormals only (an extent of a few hundred denormal steps); the others: ordinary points with
    -0.0 and denormals among them."""
    x = rng.randn(b, n, 3).astype(np.float32)
    x[0] = (rng.randint(-300, 301, (n, 3)).astype(np.int64) * np.float64(1.4e-45)).astype(np.float32)
    sel = rng.rand(b, n, 3) < 0.2
    x[sel] = np.float32(-0.0)
    sel = rng.rand(b, n, 3) < 0.1
    sel[0] = False
    x[sel] = np.float32(3e-42)
    return x


def nonfinite(rng, n, b=B):
    """+inf, -inf, a quiet NaN and two signalling NaNs (written as bits), each in a sample of otherwise ordinary points."""
    x = rng.randn(b, n, 3).astype(np.float32)
    bits = x.view(np.int32)
    x[0, n // 3, 1] = np.nan
    bits[0, n // 2, 0] = 0x7FA00000
    bits[0, n - 1, 2] = np.int32(-0x5FFFFF)  # 0xFFA00001
    x[0, 1, 2] = np.inf
    x[1, n - 2, 0] = -np.inf
    x[1, 0, 1] = np.inf
    bits[1, n // 5, 1] = 0x7FA00000
    assert np.isnan(x).sum() == 4
    return x


def duplicates(rng, n, b=B):
    """data_util.resample_pcd: a short scan filled up with copies of its own points."""
    base = rng.rand(b, max(n // 3, 1), 3).astype(np.float32)
    return np.take_along_axis(base, rng.randint(0, base.shape[1], (b, n))[..., None], 1)


MAKERS = [lattice, corners, flat_axis, huge, tiny, zeros_and_denormals, nonfinite, duplicates]
CASES = [(n, m, mk) for n, m in SHAPES for mk in MAKERS]
IDS = [f"{n}x{m}-{mk.__name__}" for n, m, mk in CASES]


def same(got, exp):
    return np.array_equal(got, exp, equal_nan=exp.dtype.kind == "f")


@pytest.mark.parametrize("n,m,mk", CASES, ids=IDS)
def test_culled_route_matches_dense(n, m, mk):
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(n + 7 * m + 13 * MAKERS.index(mk))
    ta, tc = cu(mk(rng, n)), cu(mk(rng, m))
    ref = R.nn_distance(ta, tc, mode="dense")
    out = R.nn_distance(ta, tc, mode="culled")
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert same(got.cpu().numpy(), exp.cpu().numpy()), name


def handle_parts(s):
    """The arrays of a sorted handle (rf_nn_sort), as tests/test_gpu_sort_valu_tables.py reads them: xyz (npad, 3) | orig (npad) |
    box16 (npad / 64, 4 blocks, lo.xyz hi.xyz) | box64 (npad / 64, lo.xyz - hi.xyz -) | pos0, crowded, non-finite (b each), each
    part at a multiple of 256 bytes; a cloud sorted by two workgroups carries one superblock more."""
    from rfnet_amd._lib import lib
    b, n = s.b, s.n
    up = lambda v: (v + 255) // 256 * 256
    total = int(lib.rf_nn_sort_bytes(b, n))
    for npad in ((n + 63) // 64 * 64, (n + 63) // 64 * 64 + 64):
        sizes = [up(b * npad * 12 + 256), up(b * npad * 4), up(b * (npad // 64) * 96), up(b * (npad // 64) * 32), up(3 * b * 4)]
        if sum(sizes) == total:
            break
    else:
        raise AssertionError("handle size matches neither padded length")
    raw = s.buf.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(sizes)])
    xyz = raw[off[0]:off[0] + b * npad * 12].view(np.float32).reshape(b, npad, 3)
    orig = raw[off[1]:off[1] + b * npad * 4].view(np.int32).reshape(b, npad)
    box16 = raw[off[2]:off[2] + b * (npad // 64) * 96].view(np.float32).reshape(b, npad // 16, 2, 3)
    box64 = raw[off[3]:off[3] + b * (npad // 64) * 32].view(np.float32).reshape(b, npad // 64, 2, 4)[..., :3]
    flags = raw[off[4]:off[4] + 3 * b * 4].view(np.int32).reshape(3, b)
    return xyz, orig, box16, box64, flags


@pytest.mark.parametrize("n", [100, 2048, 8193, 16384])
@pytest.mark.parametrize("mk", MAKERS, ids=[mk.__name__ for mk in MAKERS])
def test_sorted_handle_invariants(n, mk):
    from rfnet_amd import _raw as R
    src = mk(np.random.RandomState(n + MAKERS.index(mk)), n)
    s = R.nn_sort(cu(src))
    torch.cuda.synchronize()
    xyz, orig, box16, box64, flags = handle_parts(s)
    for bi in range(B):
        real = orig[bi] >= 0
        # every workgroup of a split cloud binned every point alike: none lost, none doubled (non-finite points included)
        assert np.array_equal(np.sort(orig[bi][real]), np.arange(n)), "orig is not a permutation of 0..n-1"
        assert (orig[bi][~real] == -1).all()
        rec, pts = xyz[bi][real], src[bi][orig[bi][real]]
        nan = np.isnan(pts)
        assert np.array_equal(np.isnan(rec), nan) and np.array_equal(rec[~nan], pts[~nan]), "a record is not its point"
        assert bool(flags[2, bi]) == (not np.isfinite(src[bi]).all()), "the non-finite flag of a sorted handle"
        for box, size in ((box16, 16), (box64, 64)):
            assert not np.isnan(box[bi]).any(), f"a NaN in a {size}-record box"
            lo = np.repeat(box[bi, :, 0], size, 0)[real]
            hi = np.repeat(box[bi, :, 1], size, 0)[real]
            assert ((lo <= rec) | nan).all() and ((rec <= hi) | nan).all(), f"a {size}-record box misses a record"


# (n, m, maker, the smallest power-of-two batch size at which culled_pays(b, n, m) holds: b * n * m >= 2^24 up to 4096 points,
# >= 2^27 up to 16384 -- nn_distance.hip)
STEP = [(2048, 2048, lattice, 4), (2048, 2048, nonfinite, 4), (8193, 2048, lattice, 8), (8193, 2048, nonfinite, 8)]


@pytest.mark.parametrize("n,m,mk,b", STEP, ids=[f"{n}x{m}-{mk.__name__}" for n, m, mk, _ in STEP])
def test_step_matches_dense(n, m, mk, b):
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    assert lib.rf_chamfer_step_workspace_bytes(b, n, m) > lib.rf_nn_distance_workspace_bytes(b, n, m), \
        "shape does not take the sorted-space step"
    rng = np.random.RandomState(n + m + b)
    ta, tc = cu(mk(rng, n, b)), cu(mk(rng, m, b))
    ref = [t.cpu().numpy() for t in R.nn_distance(ta, tc, mode="dense")]
    tg1 = cu((rng.rand(b, n) + 0.25).astype(np.float32) * rng.choice([-1, 1], (b, n)).astype(np.float32))
    tg2 = cu((rng.rand(b, m) + 0.25).astype(np.float32))
    plan = R.ChamferStep(b, n, m, "cuda")
    for _ in range(2):  # the plan's buffers and workspace are reused
        out = plan(ta, tc, tg1, tg2)
    for got, exp, name in zip(out[:4], ref, ("dist1", "idx1", "dist2", "idx2")):
        assert same(got.cpu().numpy(), exp), name
    r1, r2 = R.nn_distance_grad(ta, tc, tg1, cu(ref[1]), tg2, cu(ref[3]))
    for got, exp in ((out[4], r1), (out[5], r2)):
        top = float(exp[torch.isfinite(exp)].abs().max())
        assert torch.allclose(got, exp, rtol=1e-5, atol=1e-5 * top, equal_nan=True)


@pytest.mark.parametrize("n", [2048, 8193])
def test_ball_query_over_a_handle_sees_the_nan(n):
    """A NaN distance is inside every ball (grouping.hip), so the boxed ball query must know that the cloud holds one: the
    handle's sort keeps the flag that the Chamfer's private sorts leave out."""
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(n)
    ds = (rng.rand(B, n, 3).astype(np.float32))
    ds[0, n // 7, 0] = np.nan
    ds.view(np.int32)[1, n - 3, 2] = 0x7FA00000
    q = rng.rand(B, 300, 3).astype(np.float32)
    si, sc = R.query_ball_point(0.08, 16, cu(ds), cu(q), form="scan")
    h = R.nn_sort(cu(ds))
    gi, gc = R.query_ball_point(0.08, 16, cu(ds), cu(q), form="boxes", sorted1=h.buf)
    assert torch.equal(gc, sc) and torch.equal(gi, si)
