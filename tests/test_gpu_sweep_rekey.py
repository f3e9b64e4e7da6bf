"""GPU: the culled sweep's one-wave groups with one candidate superblock per lane (candidate sets of up to 4096
points) keep the lane's candidate box for the whole traversal and carry ONE key register; a re-key -- the bounds of the
remaining superblocks against the box of the lanes still active, every time their number has halved -- then loads
nothing (nn_pruned.hip, sweep_group).  Shapes that force re-keys or sit on a boundary of that code, the culled route
(rf_nn_distance, mode "culled") and rf_chamfer_step against the dense sweep: dist / idx bit-identical, gradients at the
gradient tolerance of the step's suite (rel 1e-5 + 1e-5 of the largest term).  The small shapes are checked against
the CPU oracle as well, so what they are compared with does not come from the code under test.

A direction takes one wave per query group from b * groups >= 4096 on; below that its groups are quad tiles or shared by
four waves.  The small shapes therefore cover the boundaries on the tile / shared paths, which keep their code, and the
same constructions at a batch size past that threshold run the one-key traversal itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def randn_pair(seed, b, n, m):
    rng = np.random.RandomState(seed)
    return rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


def outlier_pair(seed, b, n, m):
    """One point in 64 of the large set thrown out to 50x the cloud's extent: the outliers' lanes finish late and keep
    their wave alive, so the active set halves again and again and the keys are recomputed each time."""
    rng = np.random.RandomState(seed)
    a = rng.randn(b, n, 3).astype(np.float32)
    c = rng.randn(b, m, 3).astype(np.float32)
    extent = float(np.abs(c).max())
    for bi in range(b):
        out = rng.permutation(m)[:m // 64]
        d = rng.randn(len(out), 3)
        c[bi, out] = (50.0 * extent * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return a, c


def dup_pair(seed, b, n, m, unique=700):
    """The small set as `unique` points resampled with duplicates (data_util.resample_pcd fills short scans this way): a
    query's minimum is attained by several copies of one point.  Copies are neighbours in the sorted order and straddle at
    most a block boundary, so the re-scan of the winning block and of the second block that equalled it resolves them: by the
    kernel's counters this input takes NO second traversal on the one-wave path (profiles/sweep_rekey_ab.txt).  What it
    covers is the two-block re-scan behind the one-key traversal and exact ties in the re-keyed bounds."""
    rng = np.random.RandomState(seed)
    base = rng.rand(b, unique, 3).astype(np.float32)
    a = np.take_along_axis(base, rng.randint(0, unique, (b, n))[..., None], 1)
    return a, rng.rand(b, m, 3).astype(np.float32)


def lattice_pair(seed, b, n, m, side=12):
    """Both sets on a coarse integer lattice, the candidates moved by half a cell: a query has up to eight DIFFERENT nearest
    candidates at the same distance, each present about twice, in more than two blocks of the sorted order.  Such a lane is
    flagged and its wave runs the second traversal, which starts from the flagged lanes' box and re-keys as they finish.
    By the kernel's counters for lattice_pair(19, 80, 3500, 3500), the case below: 8757 of its 8800 one-wave groups take the
    second traversal, 1108 of them re-key once there and 39 twice (profiles/sweep_rekey_ab.txt, section 1)."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, side, (b, n, 3)).astype(np.float32)
    c = (rng.randint(0, side, (b, m, 3)) + 0.5).astype(np.float32)
    return a, c


# (name, maker, b, n, m, also against the CPU oracle)
CASES = [
    # the shapes of the issue: boundaries of the list length, forced re-keys, duplicates (b * groups < 4096: tile / shared paths)
    ("kk1_bound_64_entries", randn_pair, 2, 4096, 2053, True),
    ("kk5_first_65_entries", randn_pair, 2, 4160, 2048, True),
    ("outliers_halve_the_active_set", outlier_pair, 1, 2048, 16384, True),
    ("duplicates_two_block_rescan", dup_pair, 2, 2048, 3000, True),
    # the same constructions with b * groups >= 4096: one wave per query group
    ("one_wave_64_entries_both_ways", randn_pair, 64, 4096, 4096, False),
    ("one_wave_64_and_65_entries", randn_pair, 64, 4160, 4096, False),
    ("one_wave_outliers", outlier_pair, 16, 2048, 16384, False),
    ("one_wave_duplicates", dup_pair, 96, 2048, 3000, False),
    # the second traversal of the one-key instance (55 candidate superblocks, one wave per group both ways)
    ("one_wave_lattice_second_traversal", lattice_pair, 80, 3500, 3500, False),
]


@pytest.fixture(scope="module")
def dense():
    """Inputs and the dense route's result per case, computed once."""
    from rfnet_amd import _raw as R
    cache = {}

    def get(i):
        if i not in cache:
            name, maker, b, n, m, _ = CASES[i]
            a, c = maker(11 + i, b, n, m)
            ta, tc = cu(a), cu(c)
            ref = [t.cpu().numpy() for t in R.nn_distance(ta, tc, mode="dense")]
            cache[i] = (a, c, ta, tc, ref)
        return cache[i]
    return get


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_culled_route_matches_dense(orc, dense, i):
    from rfnet_amd import _raw as R
    a, c, ta, tc, ref = dense(i)
    if CASES[i][5]:
        for got, exp, name in zip(ref, orc.nn_distance(a, c), ("dist1", "idx1", "dist2", "idx2")):
            assert np.array_equal(got, exp), "dense route vs oracle: " + name
    out = R.nn_distance(ta, tc, mode="culled")
    for got, exp, name in zip(out, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert np.array_equal(got.cpu().numpy(), exp), name


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_step_matches_dense(dense, i):
    from rfnet_amd import _raw as R
    a, c, ta, tc, ref = dense(i)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    rng = np.random.RandomState(3)
    tg1 = cu((rng.rand(b, n) + 0.25).astype(np.float32) * rng.choice([-1, 1], (b, n)).astype(np.float32))
    tg2 = cu((rng.rand(b, m) + 0.25).astype(np.float32))
    plan = R.ChamferStep(b, n, m, "cuda")
    for _ in range(2):  # the plan's buffers and workspace are reused
        out = plan(ta, tc, tg1, tg2)
    for got, exp, name in zip(out[:4], ref, ("dist1", "idx1", "dist2", "idx2")):
        assert np.array_equal(got.cpu().numpy(), exp), name
    r1, r2 = R.nn_distance_grad(ta, tc, tg1, cu(ref[1]), tg2, cu(ref[3]))
    for got, exp in ((out[4], r1), (out[5], r2)):
        assert torch.allclose(got, exp, rtol=1e-5, atol=1e-5 * float(exp.abs().max()))
