"""GPU: the back half of the register-resident sort of the culled Chamfer (nnp_sort_reg_kernel, nn_pruned.hip) -- the chain behind
the keys.  A second slice's `base` comes out of the scan's one read of the wave totals (the slice counts ride in its spare lanes),
the octet steps of the staging boxes are minima and maxima with a DPP operand (two quad permutations and the mirror of a row's
half), and col_start is a shift.  A staging round of more than 8192 records takes a second trip of the box loop in the first lanes.

The order only steers the culling, so every case is the culled route against the dense sweep, bit for bit (rf_nn_distance, mode
"culled" vs "dense").  What the staging must keep is checked on the sorted handle (rf_nn_sort) of the case's larger cloud: `orig`
is a permutation of 0..n-1 plus padding of -1 (a wrong `base` makes the two slices overlap or leaves a gap), and every 16-record
and every 64-record box EQUALS the minimum and maximum of its non-padding records bit for bit -- equality, not containment: a
wrong lane pattern in a reduction then fails instead of only loosening the culling -- with a NaN coordinate in no box, an
infinite one a bound like any other, and an all-padding block (+inf, -inf).  (The ragged case has no handle of its own: rf_nn_sort
takes no counts.  Its handle check is that of the full cloud; the counts go through rf_nn_distance_lengths, both routes.)

Shapes: the smallest at which each path can go wrong (B = 2).  8193: the smallest split cloud.  16384 randn: both slices near
8192, the larger one with a second trip of the box loop.  12 000 copies of one point: one slice of more than 9216 records, so a
second staging round (h0 = HALF), the other slice short.  16383 and 9000: segment lengths that are no multiple of 64 or 16.
2048: one workgroup per cloud, no `base`.  rf_chamfer_step at the smallest batch that takes the sorted-space step (asserted, as
tests/test_gpu_sort_bins.py does), gradients against rf_nn_distance_grad at that file's bar (rel 1e-5 + 1e-5 of the largest
term)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def randn(rng, n, b=B):
    return rng.randn(b, n, 3).astype(np.float32)


def copies(rng, n, b=B):
    """12 000 copies of one point in front of uniform points (n = 16384: 4384 of them)."""
    x = rng.rand(b, n, 3).astype(np.float32)
    x[:, :12000] = rng.rand(b, 1, 3).astype(np.float32)
    return x


def nonfinite(rng, n, b=B):
    """A NaN point and a +-inf point among ordinary ones (sample 0: a whole NaN point and +inf; sample 1: one NaN coordinate
    and -inf)."""
    x = rng.randn(b, n, 3).astype(np.float32)
    x[0, n // 3] = np.nan
    x[0, n // 2, 1] = np.inf
    x[1, n - 5, 2] = np.nan
    x[1, 7] = -np.inf
    return x


# (n, m, maker)
CASES = [(8193, 300, randn), (16384, 512, randn), (16384, 512, copies), (16383, 64, randn), (9000, 64, randn),
         (2048, 2048, randn), (16384, 512, nonfinite)]
IDS = [f"{n}x{m}-{mk.__name__}" for n, m, mk in CASES]


def same(got, exp):
    return np.array_equal(got, exp, equal_nan=exp.dtype.kind == "f")


def handle_parts(s):
    """The arrays of a sorted handle (rf_nn_sort), as tests/test_gpu_sort_bins.py reads them: xyz (npad, 3) | orig (npad) |
    box16 (npad / 64, 4 blocks, lo.xyz hi.xyz) | box64 (npad / 64, lo.xyz - hi.xyz -) | three flags (b each), each part at a
    multiple of 256 bytes; a cloud sorted by two workgroups carries one superblock more."""
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


def check_handle(src):
    """rf_nn_sort of `src` (b, n, 3): the permutation and the exact boxes."""
    from rfnet_amd import _raw as R
    b, n = src.shape[:2]
    s = R.nn_sort(cu(src))
    torch.cuda.synchronize()
    xyz, orig, box16, box64 = handle_parts(s)
    for bi in range(b):
        real = orig[bi] >= 0
        assert np.array_equal(np.sort(orig[bi][real]), np.arange(n)), "orig is not a permutation of 0..n-1"
        assert (orig[bi][~real] == -1).all(), "padding carries an index"
        assert same(xyz[bi][real], src[bi][orig[bi][real]]), "a record is not its point"
        # the reference boxes: padding out (+inf for the minimum, -inf for the maximum), a NaN dropped per coordinate by fmin / fmax
        # (the inputs hold no zero, so a minimum has one bit pattern)
        rec = xyz[bi]
        lo_in = np.where(real[:, None], rec, np.float32(np.inf))
        hi_in = np.where(real[:, None], rec, np.float32(-np.inf))
        for box, size in ((box16, 16), (box64, 64)):
            lo = np.fmin.reduce(np.fmin(lo_in, np.float32(np.inf)).reshape(-1, size, 3), axis=1)
            hi = np.fmax.reduce(np.fmax(hi_in, np.float32(-np.inf)).reshape(-1, size, 3), axis=1)
            assert not np.isnan(box[bi]).any(), f"a NaN in a {size}-record box"
            for got, exp, what in ((box[bi, :, 0], lo, "minimum"), (box[bi, :, 1], hi, "maximum")):
                bad = np.flatnonzero((got.view(np.int32) != exp.view(np.int32)).any(axis=1))
                assert bad.size == 0, f"{size}-record boxes {bad[:8]} of sample {bi}: {what} {got[bad[0]]} != {exp[bad[0]]}"
            empty = ~real.reshape(-1, size).any(axis=1)
            assert (box[bi, empty, 0] == np.inf).all() and (box[bi, empty, 1] == -np.inf).all(), "an all-padding block"


@pytest.mark.parametrize("n,m,mk", CASES, ids=IDS)
def test_staging_matches_dense_and_boxes_are_exact(n, m, mk):
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(n + 7 * m + 13 * CASES.index((n, m, mk)))
    a = mk(rng, n)
    c = rng.rand(B, m, 3).astype(np.float32) if mk is copies else randn(rng, m)
    ta, tc = cu(a), cu(c)
    ref = R.nn_distance(ta, tc, mode="dense")
    out = R.nn_distance(ta, tc, mode="culled")
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert same(got.cpu().numpy(), exp.cpu().numpy()), name
    check_handle(a)


def test_ragged_counts_behind_a_split():
    """Counts {8193, 16384} in a batch of 16384-point clouds: the split is decided by the full size, sample 0's slices hold 8193
    points between them and everything behind the count is padding."""
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(16384 + 8193)
    a, c = randn(rng, 16384), randn(rng, 300)
    ta, tc = cu(a), cu(c)
    l1 = torch.tensor([8193, 16384], dtype=torch.int32)
    ref = R.nn_distance(ta, tc, mode="dense", lengths1=l1)
    out = R.nn_distance(ta, tc, mode="culled", lengths1=l1)
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert same(got.cpu().numpy(), exp.cpu().numpy()), name
    # the same counts as clouds of their own
    d1, i1, d2, i2 = R.nn_distance(cu(a[:1, :8193]), cu(c[:1]), mode="dense")
    assert same(out[0][0, :8193].cpu().numpy(), d1[0].cpu().numpy()) and same(out[1][0, :8193].cpu().numpy(), i1[0].cpu().numpy())
    assert same(out[2][0].cpu().numpy(), d2[0].cpu().numpy()) and same(out[3][0].cpu().numpy(), i2[0].cpu().numpy())
    check_handle(a)


def test_step_takes_the_sorted_space_route_and_matches_dense():
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    n, m, b = 16384, 512, 16  # b * n * m = 2^27: the smallest batch of this shape on the sorted-space step (nn_distance.hip)
    assert lib.rf_chamfer_step_workspace_bytes(b, n, m) > lib.rf_nn_distance_workspace_bytes(b, n, m), \
        "shape does not take the sorted-space step"
    assert lib.rf_chamfer_step_workspace_bytes(b // 2, n, m) <= lib.rf_nn_distance_workspace_bytes(b // 2, n, m), \
        "a smaller batch takes it too"
    rng = np.random.RandomState(n + m + b)
    ta, tc = cu(randn(rng, n, b)), cu(randn(rng, m, b))
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
