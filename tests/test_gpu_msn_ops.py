"""GPU: rf_expansion_penalty, rf_expansion_penalty_grad and rf_mds against the numpy restatements of
tests/test_msn_ops_host.py, bit for bit (`view(np.uint32)` for floats): every patch size on either side of a routing
threshold, the input families with ties, duplicates and lattices, non-finite patches between healthy ones, determinism and
independence of batch and patch, the gradient against the float64 closed form under the reference tree (entry and glue),
ragged and badly scaled MDS batches, and the chain expansion_penalty -> mean_mst -> minimum_density_sample -> gather_point
captured in a graph."""
import numpy as np
import pytest
import torch

from test_gpu_emd_assign import ulp32
from test_msn_ops_host import MDS_BADSIGMA, MDS_OK, XP_FAMILIES, XP_NONFINITE, XP_OK, mds_ref, xp_family, xp_penalty, xp_tree

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
ALPHAS = (0.0, 1.0, 1.5)
NAMES = ("dist", "father", "length", "mean", "info")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == F32 else x


def xp_call(xyz, S, alpha):
    from rfnet_amd import _raw
    out = _raw.expansion_penalty(torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), S, alpha)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (t.cpu().numpy() for t in out)))


def xp_batch(family, S, b, P, seed):
    return np.stack([np.concatenate([xp_family(family, S, seed + 17 * i + p) for p in range(P)]) for i in range(b)])


def xp_trees(xyz, S):
    b, n, _ = xyz.shape
    return [[xp_tree(xyz[i, p * S:(p + 1) * S]) for p in range(n // S)] for i in range(b)]


def xp_expect(trees, S, alpha):
    """The five outputs of the call from the per-patch references (father as cloud-level rows)."""
    b, P = len(trees), len(trees[0])
    e = dict(dist=np.zeros((b, P * S), F32), father=np.zeros((b, P * S), I32), length=np.zeros((b, P * S), F32),
             mean=np.zeros((b, P), F32), info=np.zeros((b, P), I32))
    for i in range(b):
        for p in range(P):
            t, rows = trees[i][p], slice(p * S, (p + 1) * S)
            e["dist"][i, rows], e["father"][i, rows], e["length"][i, rows] = xp_penalty(t, alpha), t["father"] + p * S, t["length"]
            e["mean"][i, p], e["info"][i, p] = t["mean"], t["status"]
    return e


def xp_same(got, exp, what):
    for k in NAMES:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        diff = np.flatnonzero(bits(got[k]).ravel() != bits(exp[k]).ravel())
        assert diff.size == 0, (what, k, int(diff.size), int(diff[0]), got[k].ravel()[diff[0]], exp[k].ravel()[diff[0]])


# ---- 1. the penalty, bit for bit ----------------------------------------------------------------------------------------
# one size on each side of every routing threshold (one wave up to 256, 256 threads up to 1024, 1024 threads up to 4096)
@pytest.mark.parametrize("family", XP_FAMILIES)
@pytest.mark.parametrize("S", [2, 3, 37, 64, 65, 256, 257, 512, 1024, 1025, 4096])
def test_penalty_is_the_reference_bit_for_bit(S, family):
    b, P = (1, 2) if S == 4096 else (3, 4)
    xyz = xp_batch(family, S, b, P, 1000 + S)
    trees = xp_trees(xyz, S)
    for alpha in ALPHAS:
        got = xp_call(xyz, S, alpha)
        xp_same(got, xp_expect(trees, S, alpha), (family, S, alpha))
        assert (got["info"] == XP_OK).all()
    if family == "uniform" and S >= 37:
        k = int((got["dist"] != 0).sum())
        assert 0 < k < b * P * (S - 1)  # alpha 1.5 penalises some edges and not all


# ---- 2. non-finite patches ----------------------------------------------------------------------------------------------
def test_a_non_finite_patch_is_reported_and_its_neighbours_are_untouched():
    S, b, P = 65, 2, 4
    xyz = xp_batch("uniform", S, b, P, 7)
    healthy = xp_call(xyz, S, 1.5)
    bad = xyz.copy()
    bad[0, 1 * S + 40, 2] = np.nan
    bad[1, 2 * S + 64, 0] = np.inf
    bad[1, 3 * S, 1] = -np.inf  # the patch's root
    got = xp_call(bad, S, 1.5)
    xp_same(got, xp_expect(xp_trees(bad, S), S, 1.5), "non-finite")
    status = np.zeros((b, P), I32)
    status[0, 1] = status[1, 2] = status[1, 3] = XP_NONFINITE
    assert np.array_equal(got["info"], status)
    for i in range(b):
        for p in range(P):
            rows = slice(p * S, (p + 1) * S)
            if status[i, p]:
                assert np.array_equal(got["father"][i, rows], np.arange(p * S, (p + 1) * S))
                assert not bits(got["dist"][i, rows]).any() and not bits(got["length"][i, rows]).any() and bits(got["mean"])[i, p] == 0
            else:
                for k in ("dist", "father", "length"):
                    assert got[k][i, rows].tobytes() == healthy[k][i, rows].tobytes(), (i, p, k)
                assert got["mean"][i, p].tobytes() == healthy["mean"][i, p].tobytes()


# ---- 3. determinism and independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 257, 1025])
def test_penalty_is_deterministic_and_independent_of_batch_and_patch(S):
    b, P = 3, 4
    xyz = xp_batch("lattice", S, b, P, 3)
    xyz[1] = xp_batch("uniform", S, 1, P, 4)[0]
    one, two = xp_call(xyz, S, 1.0), xp_call(xyz, S, 1.0)
    for k in NAMES:
        assert one[k].tobytes() == two[k].tobytes(), k
    for i in range(b):
        alone = xp_call(xyz[i:i + 1], S, 1.0)
        for k in NAMES:
            assert alone[k][0].tobytes() == one[k][i].tobytes(), (i, k)
    for i, p in ((0, 0), (1, 3), (2, 2)):
        rows = slice(p * S, (p + 1) * S)
        patch = xp_call(xyz[i:i + 1, rows], S, 1.0)
        for k in ("dist", "length"):
            assert patch[k][0].tobytes() == one[k][i, rows].tobytes(), (i, p, k)
        assert np.array_equal(patch["father"][0] + p * S, one["father"][i, rows])
        assert patch["mean"][0, 0] == one["mean"][i, p] and patch["info"][0, 0] == one["info"][i, p]


# ---- 4. the gradient ----------------------------------------------------------------------------------------------------
def xp_grad_ref(xyz, S, trees, alpha, g):
    """The closed form in float64 under the reference tree -> (grad (b, n, 3), bar (b, n, 3), touched (b, n) bool).
    bar: per component the sum over the contributing terms of 4 ulp32(t_k) (grad_close's bar of test_gpu_emd_assign.py for
    the same term) plus ulp32 of the sum (the one rounding of the double sum to fp32)."""
    b, n, _ = xyz.shape
    x64 = xyz.astype(np.float64)
    grad, bar, touched = np.zeros((b, n, 3)), np.zeros((b, n, 3)), np.zeros((b, n), bool)
    for i in range(b):
        for p in range(n // S):
            t, X = trees[i][p], x64[i, p * S:(p + 1) * S]
            pen = np.flatnonzero(xp_penalty(t, alpha) != 0)
            f = t["father"][pen]
            diff = X[pen] - X[f]
            term = g[i, p * S + pen, None].astype(np.float64) * diff / np.sqrt((diff * diff).sum(1))[:, None]
            G, B, T = np.zeros((S, 3)), np.zeros((S, 3)), np.zeros(S, bool)
            G[pen] += term
            B[pen] += 4 * ulp32(term)
            np.subtract.at(G, f, term)
            np.add.at(B, f, 4 * ulp32(term))
            T[pen] = T[f] = True
            rows = slice(p * S, (p + 1) * S)
            grad[i, rows], bar[i, rows], touched[i, rows] = G, B + ulp32(G), T
    return grad, bar, touched


def xp_grad_close(got, ref, what):
    grad, bar, touched = ref
    err = np.abs(got.astype(np.float64) - grad)
    worst = float((err[touched] / bar[touched]).max()) if touched.any() else 0.0
    print(f"{what}: worst error {worst:.3f} of the bar over {int(touched.sum())} rows; {int((~touched).sum())} rows without a term")
    assert (err <= bar).all(), (what, worst)
    assert not bits(got[~touched]).any(), what  # exactly +0 where nothing contributes


@pytest.mark.parametrize("family,S", [("uniform", 37), ("duplicates", 64), ("lattice", 257), ("uniform", 1025), ("outlier", 4096)])
def test_gradient_entry_against_the_closed_form(family, S):
    """alpha = 0: every edge of positive length is active, so a father receives from several children."""
    from rfnet_amd import _raw
    b, P = (1, 2) if S == 4096 else (3, 4)
    xyz = xp_batch(family, S, b, P, 2000 + S)
    trees = xp_trees(xyz, S)
    e = xp_expect(trees, S, 0.0)
    g = np.random.RandomState(S).randn(b, P * S).astype(F32)
    children = np.bincount(np.concatenate([t["father"][1:] for row in trees for t in row]))
    assert children.max() >= 3
    tx = torch.from_numpy(xyz).cuda()
    args = (tx, S, torch.from_numpy(e["father"]).cuda(), torch.from_numpy(e["dist"]).cuda(), torch.from_numpy(g).cuda())
    one, two = _raw.expansion_penalty_grad(*args).cpu().numpy(), _raw.expansion_penalty_grad(*args).cpu().numpy()
    assert one.shape == (b, P * S, 3) and one.tobytes() == two.tobytes()
    xp_grad_close(one, xp_grad_ref(xyz, S, trees, 0.0, g), (family, S))
    if family == "duplicates":  # a duplicate hangs on its twin with length 0: no term, exactly +0 unless it has children
        zero = e["length"] == 0
        assert zero.sum() > b * P and not (e["dist"][zero] != 0).any()
    # alpha 1.5: only the long edges
    e15 = xp_expect(trees, S, 1.5)
    got = _raw.expansion_penalty_grad(tx, S, args[2], torch.from_numpy(e15["dist"]).cuda(), args[4]).cpu().numpy()
    xp_grad_close(got, xp_grad_ref(xyz, S, trees, 1.5, g), (family, S, 1.5))


@pytest.mark.parametrize("alpha", [0.0, 1.5])
def test_gradient_through_glue_against_the_closed_form(alpha):
    from rfnet_amd import glue
    S, b, P = 257, 3, 4
    xyz = xp_batch("uniform", S, b, P, 77)
    xyz[2] = xp_batch("duplicates", S, 1, P, 78)[0]
    trees = xp_trees(xyz, S)
    tx = torch.from_numpy(xyz).cuda().requires_grad_()
    dist, father, mean, length, info = glue.expansion_penalty(tx, S, alpha, return_info=True)
    assert dist.requires_grad and not father.requires_grad and not mean.requires_grad and father.dtype == torch.int32
    e = xp_expect(trees, S, alpha)
    for k, t in zip(NAMES, (dist, father, length, mean, info)):
        assert bits(t.detach().cpu().numpy()).tobytes() == bits(e[k]).tobytes(), k
    loss = glue.expansion_loss(tx, S, alpha)
    assert float(loss.detach()) == float(dist.detach().mean())
    loss.backward()
    g = np.full((b, P * S), F32(1.0) / F32(b * P * S), F32)
    xp_grad_close(tx.grad.cpu().numpy(), xp_grad_ref(xyz, S, trees, alpha, g), ("glue", alpha))


# ---- 5. minimum density sampling ----------------------------------------------------------------------------------------
def mds_call(xyz, m, sigma, lengths=None):
    from rfnet_amd import _raw
    t = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    if isinstance(sigma, np.ndarray):
        sigma = torch.from_numpy(sigma).cuda()
    if lengths is not None:
        lengths = torch.from_numpy(np.asarray(lengths, I32)).cuda()
    out, info, nx = _raw.minimum_density_sample(t, m, sigma, lengths=lengths, return_xyz=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy(), nx.cpu().numpy()


def mds_same(got, xyz, m, sigmas, lengths, what):
    out, info, nx = got
    assert out.shape == (xyz.shape[0], m) and out.dtype == I32 and nx.shape == (xyz.shape[0], m, 3) and nx.dtype == F32
    for i in range(xyz.shape[0]):
        L = None if lengths is None else int(lengths[i])
        eo, es, ex = mds_ref(xyz[i], m, sigmas[i], L)
        assert info[i] == es, (what, i, info[i], es)
        diff = np.flatnonzero(out[i] != eo)
        assert diff.size == 0, (what, i, int(diff.size), int(diff[0]), out[i, diff[0]], eo[diff[0]])
        assert bits(nx[i]).tobytes() == bits(ex).tobytes(), (what, i)


# (63 .. 65, 1024 / 1025: the thresholds of the one-wave and the 256-thread form; 5000: 8 points per lane; 16384: 16)
@pytest.mark.parametrize("sigma", [0.02, 0.1, 5.0])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 2), (63, 20), (64, 64), (65, 33), (256, 40), (257, 40), (700, 256), (1024, 100),
                                 (1025, 100), (3000, 512), (4096, 50), (4097, 50), (5000, 64), (8193, 40), (16384, 64)])
def test_mds_is_the_reference_bit_for_bit(n, m, sigma):
    rng = np.random.RandomState(n + m)
    xyz = rng.rand(2, n, 3).astype(F32)
    xyz[1] = (rng.rand(n, 3) * [1.0, 1.0, 0.01]).astype(F32)  # a sheet
    got = mds_call(xyz, m, sigma)
    mds_same(got, xyz, m, [sigma] * 2, None, (n, m, sigma))
    assert (got[1] == MDS_OK).all()
    for i in range(2):
        assert len(set(got[0][i].tolist())) == m


def test_mds_ragged_batch_over_hostile_padding():
    n, m = 300, 100
    lens = np.array([1, n, 77, 150, 100], I32)
    rng = np.random.RandomState(5)
    xyz = rng.rand(len(lens), n, 3).astype(F32)
    for i, L in enumerate(lens):
        xyz[i, L:] = np.nan
    got = mds_call(xyz, m, 0.1, lens)
    mds_same(got, xyz, m, [0.1] * len(lens), lens, "ragged")
    out, info, nx = got
    assert not out[0].any() and not out[2, 77:].any() and not bits(nx[2, 77:]).any() and not bits(nx[0, 1:]).any()
    assert sorted(out[2, :77].tolist()) == list(range(77)) and (info == MDS_OK).all()
    # the same clouds without their padding
    for i in (2, 3):
        alone = mds_call(xyz[i:i + 1, :lens[i]], m, 0.1)
        assert np.array_equal(alone[0][0], out[i]) and bits(alone[2][0]).tobytes() == bits(nx[i]).tobytes()


def test_mds_sigma_as_a_device_tensor_with_bad_entries():
    n, m = 700, 90
    xyz = np.random.RandomState(6).rand(5, n, 3).astype(F32)
    sigma = np.array([0.1, 0.0, np.nan, 0.05, -1.0], F32)
    got = mds_call(xyz, m, sigma)
    mds_same(got, xyz, m, sigma, None, "sigma tensor")
    out, info, nx = got
    assert info.tolist() == [MDS_OK, MDS_BADSIGMA, MDS_BADSIGMA, MDS_OK, MDS_BADSIGMA]
    for i in (1, 2, 4):
        assert np.array_equal(out[i], np.arange(m)) and np.array_equal(nx[i], xyz[i, :m])
    good = mds_call(xyz[[0, 3]], m, sigma[[0, 3]])  # the healthy samples are untouched by their neighbours
    assert np.array_equal(good[0], out[[0, 3]]) and good[2].tobytes() == nx[[0, 3]].tobytes()


def test_mds_is_deterministic_and_independent_of_the_batch():
    n, m = 3000, 300
    xyz = np.random.RandomState(8).rand(3, n, 3).astype(F32)
    sigma = np.array([0.03, 0.1, 0.3], F32)
    one, two = mds_call(xyz, m, sigma), mds_call(xyz, m, sigma)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    for i in range(3):
        alone = mds_call(xyz[i:i + 1], m, sigma[i:i + 1])
        for x, y in zip(alone, one):
            assert x[0].tobytes() == y[i].tobytes(), i
    from rfnet_amd import glue
    t = torch.from_numpy(xyz).cuda()
    idx = glue.minimum_density_sample(t, m, torch.from_numpy(sigma).cuda())
    idx2, pts = glue.minimum_density_sample(t, m, torch.from_numpy(sigma).cuda(), return_xyz=True)
    assert np.array_equal(idx.cpu().numpy(), one[0]) and torch.equal(idx, idx2) and pts.cpu().numpy().tobytes() == one[2].tobytes()
    scalar = glue.minimum_density_sample(t[1:2], m, 0.1)  # a float scale is the same scale
    assert np.array_equal(scalar.cpu().numpy()[0], one[0][1])


# ---- 6. the chain in a graph --------------------------------------------------------------------------------------------
def test_the_chain_is_captured_in_a_graph_and_replays():
    from rfnet_amd import glue
    from rfnet_amd.tf_ops.sampling.tf_sampling import gather_point
    S, b, P, m = 128, 2, 4, 200
    xyz = torch.from_numpy(xp_batch("uniform", S, b, P, 31)).cuda()

    def chain():
        dist, father, mean_mst = glue.expansion_penalty(xyz, S, 1.5)
        idx = glue.minimum_density_sample(xyz, m, mean_mst.mean(1))
        return dist, father, mean_mst, idx, gather_point(xyz, idx)

    eager = [t.clone() for t in chain()]
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        chain()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out, eager))
    # new inputs in place: the replay follows them
    xyz.copy_(torch.from_numpy(xp_batch("sheet", S, b, P, 32)))
    graph.replay()
    torch.cuda.synchronize()
    again = chain()
    assert all(torch.equal(x, y) for x, y in zip(out, again)) and not torch.equal(out[3], eager[3])
    # and the sampler saw the tree's scale: the reference on the same sigma
    sg = again[2].mean(1).cpu().numpy()
    for i in range(b):
        assert np.array_equal(mds_ref(xyz[i].cpu().numpy(), m, sg[i])[0], again[3][i].cpu().numpy())
