"""GPU: rf_cubic_feature_sampling, rf_gridding_reverse and their backward passes (include/rfops.h) against the numpy
restatements of the contract in tests/test_grnet_layers_host.py.

Bit-equal: the sampling's forward (a copy) and `inside`; its backward wherever the double sums are exact (integer gradients
|g| <= 1024: every partial sum is an integer below 2^53); Gridding Reverse's points, row and count (every operation is a prescribed
IEEE double operation).  Within a bar: the sampling's backward for random gradients, 2^-23 |ref| + k 2^-52 sum |terms| for k
contributions (one float32 rounding plus the double sum's own roundings -- the order of the additions is open), and Gridding
Reverse's backward, 2^-23 |ref| + 2^-45 sum |terms| (grev_grad_ref's docstring derives it).

The grids are the smallest with one cell, one sub-brick and a sub-brick seam (R = 2, 3, E, E + 1, 2 E + 1, 4 E + 1 with E = 8, the
backward's sub-brick edge; 2 E + 1 = 17 also crosses the seam of the counting sort's 16-bricks, and 4 E + 1 = 33 has three bricks
per axis: a brick in the middle of the grid with lower neighbours to skip), the channels straddle the chunk of 8, the
clouds have 1, 63, 64, 65 and 257 points; Gridding Reverse runs at R = 2, 3, at R = 7 and 8 (216 and 343 cells: the nearest to its
tile of 256 cells), at 22 with 255, 256 and 257 valid cells, at 64 and, one sample, at 256."""
import numpy as np
import pytest
import torch

from test_gridding_host import BOUNDS, F32, gr_grid_ref, pair
from test_grnet_layers_host import (BRICK, CHUNK, COUNT_EPS, TILE, cfs_grad_ref, cfs_grad_tol, cfs_ref, cloud, grev_grad_ref,
                                    grev_grids, grev_ref, grid_with_count)

pytestmark = pytest.mark.gpu

E = BRICK
SIZES = (1, 63, 64, 65, 257)
CHANNELS = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1)
KINDS = ("uniform", "outside", "seams", "vertices")
I32 = np.int32


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def same_bits(got, ref, what):
    bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint32).ravel() != np.ascontiguousarray(ref).view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {bad[0]}: {got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def volume(seed, b, c, R):
    """random features with a NaN (with a payload) and an inf in every sample"""
    vol = np.random.RandomState(seed).randn(b, c, R, R, R).astype(F32)
    vol.reshape(b, -1).view(np.uint32)[:, 0] = 0x7FC12345
    vol.reshape(b, -1)[:, -1] = np.inf
    vol.reshape(b, -1)[:, (c * R ** 3) // 2] = -np.inf
    return vol


def check_cfs(x, vol, lo, hi, ln=None, what="", seed=0):
    """forward bit-equal; backward bit-equal for integer gradients and within the bar for random ones -> the random case's outputs"""
    from rfnet_amd import _raw
    b, n = x.shape[:2]
    c, R = vol.shape[1], vol.shape[2]
    tl = None if ln is None else cu(ln)
    feat, inside = _raw.cubic_feature_sampling(cu(x), cu(vol), lo, hi, tl)
    feat, inside = feat.cpu().numpy(), inside.cpu().numpy()
    rng = np.random.RandomState(seed)
    gi = rng.randint(-1024, 1025, (b, n, 8, c)).astype(F32)
    gr = (rng.randn(b, n, 8, c) * np.exp(4 * rng.randn(b, n, 1, 1))).astype(F32)
    gvi = _raw.cubic_feature_sampling_grad(cu(x), cu(gi), R, lo, hi, tl).cpu().numpy()
    gvr = _raw.cubic_feature_sampling_grad(cu(x), cu(gr), R, lo, hi, tl).cpu().numpy()
    assert feat.shape == (b, n, 8, c) and gvi.shape == (b, c, R, R, R)
    worst = 0.0
    for i in range(b):
        L = None if ln is None else ln[i]
        rf, ri = cfs_ref(x[i], vol[i], lo, hi, L)
        assert int(inside[i]) == ri, f"{what} sample {i}: inside {inside[i]} != {ri}"
        same_bits(feat[i], rf, f"{what} sample {i}: feat")
        G, A, cnt = cfs_grad_ref(x[i], gi[i], R, lo, hi, L)
        same_bits(gvi[i], G.astype(F32), f"{what} sample {i}: grad_vol of integer gradients")
        G, A, cnt = cfs_grad_ref(x[i], gr[i], R, lo, hi, L)
        err, tol = np.abs(gvr[i].astype(np.float64) - G), cfs_grad_tol(G, A, cnt)
        worst = max(worst, float(np.max(err / np.maximum(tol, 1e-300))))
        assert (err <= tol).all(), f"{what} sample {i}: worst error / bar {worst:.3f}"
        assert not gvr[i][:, cnt == 0].view(np.uint32).any()  # +0 where nothing fell
    print(f"{what}: random gradients, worst error / bar {worst:.3f}")
    return feat, inside, gvr


# ---- 1. cubic feature sampling: the small grids ---------------------------------------------------------------------------------
def channels(k, R, n):
    """the channel count of a case: all five in turn; at R = 4 E + 1, where the references' arrays are large, the widest goes to
    the largest cloud only (tests stay quick)"""
    return CHANNELS[k % 5] if R <= 2 * E + 1 or n == SIZES[-1] else CHANNELS[k % 4]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", [2, 3, E, E + 1, 2 * E + 1, 4 * E + 1])
def test_sampling_small_grids(R, kind):
    for k, n in enumerate(SIZES):
        for j, (lo, hi) in enumerate(BOUNDS):
            c = channels(k + 2 * j + R, R, n)
            x = np.stack([cloud(kind, 10 * k + s + j, n, R, lo, hi) for s in range(2)])
            check_cfs(x, volume(k + R, 2, c, R), lo, hi, what=f"R = {R}, {kind}, n = {n}, c = {c}, box {lo, hi}", seed=k)


def test_sampling_every_channel_count_at_the_seam():
    R, (lo, hi) = 2 * E + 1, BOUNDS[1]
    for c in CHANNELS + (2 * CHUNK + 1,):
        x = np.stack([cloud(k, 5 + c, 257, R, lo, hi) for k in ("seams", "uniform")])
        check_cfs(x, volume(c, 2, c, R), lo, hi, what=f"c = {c}", seed=c)


# ---- 2. the larger cases ------------------------------------------------------------------------------------------------------------
def test_sampling_grnet_size():
    lo, hi = BOUNDS[0]
    x = np.stack([cloud("uniform", 1, 2048, 32, lo, hi), cloud("seams", 2, 2048, 32, lo, hi)])
    feat, inside, _ = check_cfs(x, volume(3, 2, 32, 32), lo, hi, what="b = 2, n = 2048, R = 32, c = 32")
    assert inside.tolist() == [2048, 2048]


def test_sampling_r256():
    lo, hi = BOUNDS[1]
    x = cloud("seams", 8, 257, 256, lo, hi)[None]
    check_cfs(x, volume(4, 1, 1, 256), lo, hi, what="R = 256, c = 1, n = 257")


def test_sampling_backward_collapsed():
    """65536 points in one cell, c = 2, R = 17: eight LDS words per channel take 65536 adds each; with |g| <= 1024 the sums stay
    below 2^26 and exact, so the result is bit-equal whatever the order"""
    from rfnet_amd import _raw
    R, (lo, hi) = 17, BOUNDS[0]
    n = 65536
    x = np.empty((1, n, 3), F32)
    x[0] = (0.01, 0.02, 0.03)
    g = np.random.RandomState(1).randint(-1024, 1025, (1, n, 8, 2)).astype(F32)
    got = _raw.cubic_feature_sampling_grad(cu(x), cu(g), R, lo, hi).cpu().numpy()
    G, A, cnt = cfs_grad_ref(x[0], g[0], R, lo, hi)
    assert cnt.max() == n and np.abs(G).max() <= 2 ** 26
    same_bits(got[0], G.astype(F32), "collapsed")


# ---- 3. gridding reverse ------------------------------------------------------------------------------------------------------------
def check_reverse(grid, lo, hi, eps=1e-6, what="", backward=True):
    """grid (b, R, R, R): both placements bit-equal to grev_ref, the backward within its bar"""
    from rfnet_amd import _raw
    b, R = grid.shape[:2]
    M = (R - 1) ** 3
    counts = None
    for compact in (False, True):
        points, row, count = (t.cpu().numpy() for t in _raw.gridding_reverse(cu(grid), lo, hi, eps, compact))
        assert points.shape == (b, M, 3) and row.shape == (b, M) and count.shape == (b,)
        gp = np.random.RandomState(R + compact).randn(b, M, 3).astype(F32)
        gg = _raw.gridding_reverse_grad(cu(grid), cu(row), cu(gp), lo, hi).cpu().numpy() if backward else None
        for i in range(b):
            rp, rr, rc = grev_ref(grid[i], lo, hi, eps, compact)
            w = f"{what} sample {i}, compact {compact}"
            assert int(count[i]) == rc, f"{w}: count {count[i]} != {rc}"
            assert np.array_equal(row[i], rr), f"{w}: row differs at {np.flatnonzero(row[i] != rr)[:4]}"
            same_bits(points[i], rp, f"{w}: points")
            if backward:
                G, tol = grev_grad_ref(grid[i], rr, gp[i], lo, hi)
                err = np.abs(gg[i].astype(np.float64) - G)
                assert (err <= tol).all(), f"{w}: backward, worst error / bar {np.max(err / np.maximum(tol, 1e-300)):.3f}"
                assert not gg[i][tol == 0].view(np.uint32).any()
        counts = count
    return counts


@pytest.mark.parametrize("R", [2, 3, 7, 8])
def test_reverse_small_grids(R):
    for j, (lo, hi) in enumerate(BOUNDS):
        grid = np.stack([grev_grids(k, R + j, R) for k in ("zeros", "dense", "wild", "wild")])
        count = check_reverse(grid, lo, hi, what=f"R = {R}, box {lo, hi}")
        assert count[0] == 0 and count[1] == (R - 1) ** 3


def test_reverse_of_the_gridding_layer():
    """the rf_gridding output of clouds of 2048 points: sparse at R = 64"""
    from rfnet_amd import _raw
    lo, hi = BOUNDS[0]
    x = np.stack([cloud("uniform", 1, 2048, 64, lo, hi), cloud("seams", 2, 2048, 64, lo, hi)])
    grid = _raw.gridding(cu(x), 64, lo, hi)[0].cpu().numpy()
    count = check_reverse(grid, lo, hi, what="R = 64, gridding")
    assert 0 < count.min() and count.max() < 63 ** 3 // 4
    grid = np.stack([grev_grids("dense", 5, 64), grev_grids("wild", 6, 64)])
    check_reverse(grid, lo, hi, what="R = 64")


def test_reverse_r256():
    lo, hi = BOUNDS[0]
    grid = grev_grids("sparse", 3, 256)[None]
    check_reverse(grid, lo, hi, what="R = 256", backward=False)


@pytest.mark.parametrize("count", [TILE - 1, TILE, TILE + 1])
def test_reverse_valid_counts_around_the_tile(count):
    lo, hi = BOUNDS[1]
    grid = np.stack([grid_with_count(22, count, 1), grid_with_count(22, count - 1, 2), grid_with_count(22, 0)])
    got = check_reverse(grid, lo, hi, eps=COUNT_EPS, what=f"{count} valid cells")
    assert got.tolist() == [count, count - 1, 0]


def test_reverse_backward_ignores_corrupt_rows():
    from rfnet_amd import _raw
    R, (lo, hi) = 9, BOUNDS[0]
    M = (R - 1) ** 3
    grid = np.stack([grev_grids("dense", 1, R), grev_grids("wild", 2, R)])
    row = _raw.gridding_reverse(cu(grid), lo, hi, 1e-6, True)[1].cpu().numpy()
    rng = np.random.RandomState(3)
    bad = rng.rand(2, M) < 0.3
    row[bad] = rng.choice(np.array([-1, -7, M, M + 1, 2 ** 31 - 1, -2 ** 31], I32), int(bad.sum()))
    gp = rng.randn(2, M, 3).astype(F32)
    gg = _raw.gridding_reverse_grad(cu(grid), cu(row), cu(gp), lo, hi).cpu().numpy()
    for i in range(2):
        G, tol = grev_grad_ref(grid[i], row[i], gp[i], lo, hi)
        assert (np.abs(gg[i].astype(np.float64) - G) <= tol).all()


# ---- 4. purity -------------------------------------------------------------------------------------------------------------------
def ragged_case(R, lo, hi, n=257):
    x = np.stack([cloud(k, 30 + i, n, R, lo, hi) for i, k in enumerate(("uniform", "seams", "outside", "nonfinite"))])
    ln = np.array([n, 1, 129, 64], I32)
    return x, ln


def test_sampling_ragged_calls_are_the_sliced_calls():
    from rfnet_amd import _raw
    R, (lo, hi), c = 2 * E + 1, BOUNDS[1], CHUNK + 1
    x, ln = ragged_case(R, lo, hi)
    vol = volume(1, 4, c, R)
    g = np.random.RandomState(2).randint(-1024, 1025, (4, 257, 8, c)).astype(F32)  # exact sums: the bits are promised
    outs = []
    for fill in (np.nan, 1e30):  # what the rows behind the counts hold changes nothing
        xp, gp = x.copy(), g.copy()
        for i in range(4):
            xp[i, ln[i]:] = fill
            gp[i, ln[i]:] = fill
        feat, inside = _raw.cubic_feature_sampling(cu(xp), cu(vol), lo, hi, cu(ln))
        gv = _raw.cubic_feature_sampling_grad(cu(xp), cu(gp), R, lo, hi, cu(ln))
        outs.append((bits(feat), bits(inside), bits(gv)))
        again = _raw.cubic_feature_sampling(cu(xp), cu(vol), lo, hi, cu(ln)) + (_raw.cubic_feature_sampling_grad(cu(xp), cu(gp), R, lo, hi, cu(ln)),)
        assert outs[-1] == tuple(bits(t) for t in again), "two calls differ"
    assert outs[0] == outs[1]
    for i in range(4):
        L = ln[i]
        rf, ri = cfs_ref(x[i], vol[i], lo, hi, L)
        same_bits(feat[i].cpu().numpy(), rf, f"ragged sample {i}")
        sl = _raw.cubic_feature_sampling(cu(x[i:i + 1, :L]), cu(vol[i:i + 1]), lo, hi)
        assert bits(sl[0]) == bits(feat[i:i + 1, :L]) and bits(sl[1]) == bits(inside[i:i + 1]), f"sliced call {i}"
        assert not feat[i, L:].cpu().numpy().view(np.uint32).any()
        assert bits(_raw.cubic_feature_sampling_grad(cu(x[i:i + 1, :L]), cu(g[i:i + 1, :L]), R, lo, hi)) == bits(gv[i:i + 1])
        one = _raw.cubic_feature_sampling(cu(xp[i:i + 1]), cu(vol[i:i + 1]), lo, hi, cu(ln[i:i + 1]))  # the batch slice
        assert bits(one[0]) == bits(feat[i:i + 1]) and bits(one[1]) == bits(inside[i:i + 1])
        assert bits(_raw.cubic_feature_sampling_grad(cu(xp[i:i + 1]), cu(gp[i:i + 1]), R, lo, hi, cu(ln[i:i + 1]))) == bits(gv[i:i + 1])
    # counts outside [1, n] are clamped by the kernels
    wild = _raw.cubic_feature_sampling(cu(x), cu(vol), lo, hi, cu(np.array([9999, -5, 129, 64], I32)))
    ref = _raw.cubic_feature_sampling(cu(x), cu(vol), lo, hi, cu(ln))
    assert bits(wild[0]) == bits(ref[0]) and bits(wild[1]) == bits(ref[1])


def test_reverse_calls_are_pure():
    from rfnet_amd import _raw
    R, (lo, hi) = 9, BOUNDS[1]
    grid = np.stack([grev_grids(k, 40 + i, R) for i, k in enumerate(("dense", "wild", "zeros", "wild"))])
    for compact in (False, True):
        out = _raw.gridding_reverse(cu(grid), lo, hi, 1e-6, compact)
        gp = cu(np.random.RandomState(4).randn(4, (R - 1) ** 3, 3).astype(F32))
        gg = _raw.gridding_reverse_grad(cu(grid), out[1], gp, lo, hi)
        again = _raw.gridding_reverse(cu(grid), lo, hi, 1e-6, compact)
        assert all(bits(a) == bits(c) for a, c in zip(out, again)), "two calls differ"
        assert bits(gg) == bits(_raw.gridding_reverse_grad(cu(grid), out[1], gp, lo, hi))
        for i in range(4):
            one = _raw.gridding_reverse(cu(grid[i:i + 1]), lo, hi, 1e-6, compact)
            assert all(bits(a) == bits(c[i:i + 1]) for a, c in zip(one, out)), f"batch slice {i}"
            assert bits(_raw.gridding_reverse_grad(cu(grid[i:i + 1]), one[1], gp[i:i + 1], lo, hi)) == bits(gg[i:i + 1])


# ---- 5. autograd ------------------------------------------------------------------------------------------------------------------
def test_glue_through_autograd():
    from rfnet_amd import _raw, glue
    R, (lo, hi), c = E + 1, BOUNDS[1], 5
    x, ln = ragged_case(R, lo, hi, 130)
    x = np.clip(np.nan_to_num(x, nan=9.0, posinf=9.0, neginf=-9.0), -9, 9)
    ln = np.minimum(ln, 130)
    tx, tv = cu(x).requires_grad_(), cu(np.random.RandomState(1).randint(-8, 9, (4, c, R, R, R)).astype(F32)).requires_grad_()
    feat = glue.cubic_feature_sampling(tx, tv, bounds=(lo, hi), lengths=ln)
    raw = _raw.cubic_feature_sampling(tx.detach(), tv.detach(), lo, hi, ln)[0]
    assert feat.shape == (4, 130, 8, c) and torch.equal(feat.detach(), raw) and feat.requires_grad
    g = cu(np.random.RandomState(2).randint(-64, 65, (4, 130, 8, c)).astype(F32))
    (feat * g).sum().backward()
    assert tx.grad is None  # piecewise constant in the points
    assert torch.equal(tv.grad, _raw.cubic_feature_sampling_grad(tx.detach(), g, R, lo, hi, ln)) and tv.grad.abs().max() > 0
    assert not glue.cubic_feature_sampling(tx, tv.detach(), bounds=(lo, hi), lengths=ln).requires_grad

    grid = cu(np.stack([grev_grids("dense", 1, R), grev_grids("wild", 2, R)])).requires_grad_()
    for compact in (True, False):
        grid.grad = None
        pts, cnt = glue.gridding_reverse(grid, bounds=(lo, hi), compact=compact)
        rp, rr, rc = _raw.gridding_reverse(grid.detach(), lo, hi, 1e-6, compact)
        assert torch.equal(pts.detach(), rp) and torch.equal(cnt, rc) and cnt.dtype == torch.int32 and cnt.is_cuda
        assert pts.requires_grad and not cnt.requires_grad
        gp = cu(np.random.RandomState(3).randn(2, (R - 1) ** 3, 3).astype(F32))
        (pts * gp).sum().backward()
        assert bits(grid.grad) == bits(_raw.gridding_reverse_grad(grid.detach(), rr, gp, lo, hi)) and grid.grad[0].abs().max() > 0
    # numpy in, numpy out
    out = _raw.gridding_reverse(grid.detach().cpu().numpy(), lo, hi, compact=True)
    assert isinstance(out[0], np.ndarray) and out[0].tobytes() == bits(_raw.gridding_reverse(grid.detach(), lo, hi, compact=True)[0])


# ---- 6. the path: gridding -> (a stand-in for the 3-D CNN) -> reverse -> sampling -> gather -> features, eager and replayed ---------
def stand_in(grid):
    """what stands where GRNet's 3-D CNN does, fixed and exact in float32 (powers of two): the occupancy halved, and a feature
    volume (b, 4, 8, 8, 8) of every second vertex scaled by 1, 2, -1 and 1 / 2.  The same code serves torch and numpy."""
    sub = grid[:, ::2, ::2, ::2]
    stack = torch.stack if isinstance(grid, torch.Tensor) else np.stack
    return grid * 0.5, stack([sub, sub * 2.0, -sub, sub * 0.5], 1)


def test_path_eager_and_from_a_graph(orc):
    from rfnet_amd import _raw, glue
    lo, hi = BOUNDS[0]
    b, n, R, k = 2, 2048, 16, 64
    P = [np.stack(pair("uniform", 7 + 10 * v, n, n, R, lo, hi)) for v in range(2)]
    tp = cu(P[0])

    def run():
        occ, vol = stand_in(glue.gridding(tp, R, (lo, hi)))
        pts, cnt = glue.gridding_reverse(occ, (lo, hi), compact=True)
        new = _raw.gather_point(pts, _raw.farthest_point_sample(k, pts, lengths=cnt))
        return pts, cnt, new, glue.cubic_feature_sampling(new, vol, (lo, hi))

    def reference(p):
        out = []
        for i in range(b):
            occ, vol = stand_in(gr_grid_ref(p[i], R, lo, hi)[0][None])
            pts, row, cnt = grev_ref(occ[0], lo, hi, 1e-6, True)
            assert cnt >= k
            idx = orc.farthest_point_sample(k, pts[None, :cnt])
            new = orc.gather_point(pts[None, :cnt], idx)[0]
            out.append((pts, cnt, new, cfs_ref(new, vol[0], lo, hi)[0]))
        return out

    def compare(got, ref, what):
        for i in range(b):
            same_bits(got[0][i].cpu().numpy(), ref[i][0], f"{what}: points of sample {i}")
            assert int(got[1][i]) == ref[i][1]
            same_bits(got[2][i].cpu().numpy(), ref[i][2], f"{what}: sampled points of sample {i}")
            same_bits(got[3][i].cpu().numpy(), ref[i][3], f"{what}: features of sample {i}")

    compare(run(), reference(P[0]), "eager")
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
    compare(out, reference(P[0]), "replay")
    first = bits(out[0])
    tp.copy_(cu(P[1]))  # the input changes in place: the counts change on the device, nothing is read back
    graph.replay()
    torch.cuda.synchronize()
    compare(out, reference(P[1]), "replay after the input changed")
    assert bits(out[0]) != first
