"""GPU: the keys of the register-resident sort of the culled Chamfer (nnp_sort_reg_kernel, nn_pruned.hip) -- a point's slab,
strip and z rank from the equal-mass tables, its slice of a split cloud, the lower slice's count -- on the sizes and inputs
at which those tables and counts change shape.  The order the sort produces only steers the culling, so every case is the
culled route against the dense sweep, bit for bit (rf_nn_distance, mode "culled" vs "dense"), rf_chamfer_step against the
same (gradients against rf_nn_distance_grad at the step suite's bar: rel 1e-5 + 1e-5 of the largest term), and the sorted
handle's own invariants: `orig` is a permutation plus padding and every 16- and 64-record box contains its records.

Sizes: one slab (no threshold at all), four slabs, the leaf change with one workgroup per cloud, the smallest split cloud,
seven slabs with a split cloud.  Inputs that bend the tables: no extent, a few spots (repeated thresholds, empty slabs, the
crowded path), a plane x = const (every slab but one empty), y strictly decreasing in x (the snake of the odd slabs), a NaN
and an infinite coordinate, resample_pcd duplicates.

rf_chamfer_step chooses its route by shape AND batch size (culled_pays, nn_distance.hip): every step case carries the
smallest batch size at which its shape takes the sorted-space step, and the test asserts that it does.  A shape whose smaller
cloud has fewer than 512 points never takes it at any batch size (64 vs 100, 64 vs 16384): those have no step case; the
pinned culled route above still sorts them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2  # batch size of the pinned-route cases and of the handles


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def randn(rng, n, b=B):
    return rng.randn(b, n, 3).astype(np.float32)


def identical(rng, n, b=B):
    """Sample 0: every point the same (no extent on any axis); the others as drawn."""
    x = randn(rng, n, b)
    x[0] = x[0, :1]
    return x


def five_spots(rng, n, b=B):
    """Exact copies of five spots, in coherent runs (a wave's 64 consecutive points on one or two spots: the crowded path)
    in sample 0 and at random in the others."""
    spots = rng.randn(b, 5, 3).astype(np.float32)
    sid = np.stack([np.arange(n) * 5 // n] + [rng.randint(0, 5, n) for _ in range(b - 1)])
    return np.take_along_axis(spots, sid[..., None], 1)


def plane(rng, n, b=B):
    x = randn(rng, n, b)
    x[..., 0] = np.float32(0.375)
    return x


def y_falls_with_x(rng, n, b=B):
    """y strictly decreasing in x: every odd slab's strips run against the even slabs'."""
    x = randn(rng, n, b)
    xs = np.sort(rng.rand(b, n).astype(np.float32) + np.arange(n, dtype=np.float32) / n, 1)  # increasing
    assert (np.diff(xs, axis=1) >= 0).all()
    ys = -np.arange(n, dtype=np.float32)[None] / n - 0.25 * xs
    perm = np.stack([rng.permutation(n) for _ in range(b)])
    x[..., 0] = np.take_along_axis(xs, perm, 1)
    x[..., 1] = np.take_along_axis(ys, perm, 1)
    return x


def nonfinite(rng, n, b=B):
    x = randn(rng, n, b)
    x[0, n // 3, 1] = np.nan
    x[1, n - 1, 0] = np.inf
    return x


def duplicates(rng, n, b=B):
    """data_util.resample_pcd: a short scan filled up with copies of its own points."""
    base = rng.rand(b, max(n // 3, 1), 3).astype(np.float32)
    return np.take_along_axis(base, rng.randint(0, base.shape[1], (b, n))[..., None], 1)


# (name, n, m, maker of the first set, maker of the second, batch size of the step case: the smallest power of two at which
# culled_pays(b, n, m) holds -- b * n * m >= 2^24 up to 4096 points, >= 2^27 up to 16384 -- or None where the smaller cloud
# is below its 512 points and no batch size takes the sorted-space step)
CASES = [
    ("one_slab_64_100", 64, 100, randn, randn, None),
    ("four_slabs_2048_2048", 2048, 2048, randn, randn, 4),
    ("leaf_change_4096_8192", 4096, 8192, randn, randn, 4),
    ("smallest_split_8193_2048", 8193, 2048, randn, randn, 8),
    ("seven_slabs_split_12000_16384", 12000, 16384, randn, randn, 2),
    ("no_extent", 2048, 8193, identical, identical, 8),
    ("five_spots", 2048, 8193, five_spots, five_spots, 8),
    ("five_spots_one_slab_query", 64, 16384, randn, five_spots, None),
    ("five_spots_seven_slabs", 512, 16384, randn, five_spots, 16),
    ("plane_x_const", 2048, 12000, plane, plane, 8),
    ("y_falls_with_x", 2048, 12000, y_falls_with_x, y_falls_with_x, 8),
    ("nan_and_inf", 2048, 8193, nonfinite, nonfinite, 8),
    ("duplicates", 2048, 12000, duplicates, duplicates, 8),
]
IDS = [c[0] for c in CASES]
STEP = [i for i, c in enumerate(CASES) if c[5] is not None]


@pytest.fixture(scope="module")
def dense():
    """Inputs and the dense route's result per case, computed once."""
    from rfnet_amd import _raw as R
    cache = {}

    def get(i):
        if i not in cache:
            _, n, m, mk1, mk2, _ = CASES[i]
            rng = np.random.RandomState(40 + i)
            ta, tc = cu(mk1(rng, n)), cu(mk2(rng, m))
            cache[i] = (ta, tc, [t.cpu().numpy() for t in R.nn_distance(ta, tc, mode="dense")])
        return cache[i]
    return get


def same(got, exp):
    return np.array_equal(got, exp, equal_nan=exp.dtype.kind == "f")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_culled_route_matches_dense(dense, i):
    from rfnet_amd import _raw as R
    ta, tc, ref = dense(i)
    out = R.nn_distance(ta, tc, mode="culled")
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert same(got.cpu().numpy(), exp), name


@pytest.mark.parametrize("i", STEP, ids=[IDS[i] for i in STEP])
def test_step_matches_dense(i):
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    _, n, m, mk1, mk2, b = CASES[i]
    assert lib.rf_chamfer_step_workspace_bytes(b, n, m) > lib.rf_nn_distance_workspace_bytes(b, n, m), \
        "shape does not take the sorted-space step"
    rng = np.random.RandomState(70 + i)
    ta, tc = cu(mk1(rng, n, b)), cu(mk2(rng, m, b))
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


def test_ragged_split_cloud():
    """Per-sample counts on a split size: one point, the smallest count that still means something to a split cloud's
    second workgroup, the whole cloud."""
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(9)
    n, m = 12000, 16384
    ta, tc = cu(rng.randn(3, n, 3).astype(np.float32)), cu(rng.randn(3, m, 3).astype(np.float32))
    l1, l2 = [1, 8193, n], [m, 1, 8193]
    ref = R.nn_distance(ta, tc, mode="dense", lengths1=l1, lengths2=l2)
    out = R.nn_distance(ta, tc, mode="culled", lengths1=l1, lengths2=l2)
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert torch.equal(got, exp), name


def handle_parts(s):
    """The arrays of a sorted handle (rf_nn_sort): xyz (npad, 3) | orig (npad) | box16 (npad / 64, 4 blocks, lo.xyz hi.xyz) |
    box64 (npad / 64, lo.xyz - hi.xyz -), each part at a multiple of 256 bytes.  A cloud sorted by two workgroups carries
    one superblock more: the padded length is the one that gives the handle its size.
    This mirrors rfp::sorted_bytes / rfp::sorted_view (nn_pruned.hip), which the C ABI does not expose: a change of the
    layout there fails the size match below or the "a record is not its point" check, and is made here as well."""
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
    return xyz, orig, box16, box64


@pytest.mark.parametrize("n,maker", [(100, randn), (2048, randn), (8193, randn), (16384, randn), (12000, five_spots),
                                     (12000, plane), (8193, y_falls_with_x), (12000, identical)],
                         ids=["100", "2048", "8193", "16384", "five_spots", "plane", "y_falls_with_x", "no_extent"])
def test_sorted_handle_invariants(n, maker):
    from rfnet_amd import _raw as R
    src = maker(np.random.RandomState(n), n)
    s = R.nn_sort(cu(src))
    torch.cuda.synchronize()
    xyz, orig, box16, box64 = handle_parts(s)
    for bi in range(B):
        real = orig[bi] >= 0
        assert np.array_equal(np.sort(orig[bi][real]), np.arange(n)), "orig is not a permutation of 0..n-1"
        assert (orig[bi][~real] == -1).all()
        assert np.array_equal(xyz[bi][real], src[bi][orig[bi][real]]), "a record is not its point"
        for box, size in ((box16, 16), (box64, 64)):
            lo = np.repeat(box[bi, :, 0], size, 0)[real]
            hi = np.repeat(box[bi, :, 1], size, 0)[real]
            assert (lo <= xyz[bi][real]).all() and (xyz[bi][real] <= hi).all(), f"a {size}-record box misses a record"
