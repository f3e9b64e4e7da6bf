"""GPU: rf_local_pca against pca_ref (tests/test_normals_host.py) AS BYTES -- normals, eigenvalues and axes, over planes,
exact-grid planes (with -0 coordinates), lines, duplicates, balls and clouds scaled by 1e18 and 1e-30, with and without a
viewpoint and the axes, on knn_point's idx and on a hand-made one; ragged batches against the calls on the slices; isolation of
a NaN point; glue.estimate_normals on large clouds; rf_nn_normal_consistency against nc_ref in float64 within one fp32 rounding
plus the double additions; both glue calls captured in a HIP graph with device counts."""
import numpy as np
import pytest
import torch

from test_normals_host import FAMILIES, QNAN_BITS, family_cloud, nc_bound, nc_ref, pca_ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
B, N, M = 3, 70, 65  # one query row lies behind a wave boundary
GPU_KS = (1, 2, 3, 16, 64)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def clouds(family, b, n, seed):
    return np.stack([family_cloud(family, n, seed + 11 * i) for i in range(b)])


def viewpoints(xyz, seed):
    """One viewpoint per sample at the cloud's own scale, so that some normals turn and some do not."""
    rng = np.random.RandomState(seed)
    mid = np.nanmean(xyz.astype(np.float64), 1)  # (rows behind a count are NaN in the ragged tests)
    ext = np.nanmax(np.abs(xyz - mid[:, None]), (1, 2))
    return (mid + 0.5 * ext[:, None] * rng.randn(xyz.shape[0], 3)).astype(F32)


def same_bytes(what, got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        g, e = got.reshape(-1).view(np.uint32), exp.reshape(-1).view(np.uint32)
        at = np.flatnonzero(g != e)
        raise AssertionError(f"{what}: {at.size} of {g.size} words differ from the restatement; first at {at[0]}: "
                             f"{got.reshape(-1)[at[0]]!r} ({g[at[0]]:#010x}) against {exp.reshape(-1)[at[0]]!r} ({e[at[0]]:#010x})")


def run_pca(xyz, idx, l1=None, l2=None, vp=None, axes=True):
    from rfnet_amd import glue
    r = glue.local_pca(cu(xyz), cu(idx), None if l1 is None else cu(np.asarray(l1, I32)), None if l2 is None else cu(np.asarray(l2, I32)),
                       None if vp is None else cu(vp), return_axes=axes)
    assert ("axes" in r) == axes
    return host(r["normals"]), host(r["eigenvalues"]), host(r["axes"]) if axes else None


def check_pca(what, xyz, idx, l1=None, l2=None):
    """The four forms of the call -- viewpoint or none, axes or none -- against the restatement, as bytes."""
    for vp in (None, viewpoints(xyz, 5)):
        exp = pca_ref(xyz, idx, l1, l2, vp)
        for axes in (True, False):
            got = run_pca(xyz, idx, l1, l2, vp, axes)
            tag = f"{what}, viewpoint {vp is not None}, axes {axes}"
            same_bytes(f"{tag}: normals", got[0], exp[0])
            same_bytes(f"{tag}: eigenvalues", got[1], exp[1])
            if axes:
                same_bytes(f"{tag}: axes", got[2], exp[2])
    return exp


# ---- 1. bit equality --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GPU_KS)
@pytest.mark.parametrize("family", FAMILIES)
def test_local_pca_is_the_restatement_bit_for_bit(family, k):
    from rfnet_amd import _raw
    xyz = clouds(family, B, N, 40 + k)
    if family == "grid":
        assert (np.signbit(xyz) & (xyz == 0)).any()  # -0 coordinates are part of the family
    _, idx = _raw.knn_point(k, cu(xyz), cu(xyz[:, :M]))
    idx = host(idx)
    assert idx.shape == (B, M, k)
    exp = check_pca(f"{family}, k = {k}", xyz, idx)
    assert np.isfinite(exp[1]).all()


@pytest.mark.parametrize("k", GPU_KS)
def test_local_pca_on_a_hand_made_idx(k):
    """Repeated indices, descending order, slots outside [0, len1) -- and rows with nothing left."""
    rng = np.random.RandomState(60 + k)
    xyz = clouds("ball", B, N, 61)
    idx = rng.randint(0, N, (B, M, k)).astype(I32)
    idx[:, 1::4] = np.sort(idx[:, 1::4], -1)[..., ::-1]            # descending
    idx[:, 2::4, k // 2:] = idx[:, 2::4, :1]                        # repeated
    outside = np.array([-1, N, -2 ** 31, 2 ** 31 - 1, N + 1000], I32)
    hit = rng.rand(B, M, k) < 0.25
    idx[hit] = outside[rng.randint(0, outside.size, int(hit.sum()))]
    idx[:, 7] = outside[np.arange(k) % outside.size]                # a row with no slot left: non-finite
    exp = check_pca(f"hand-made idx, k = {k}", xyz, idx)
    assert (exp[1][:, 7].view(np.uint32) == QNAN_BITS).all() and not exp[0][:, 7].any()


# ---- 2. ragged batches ------------------------------------------------------------------------------------------------------
LEN1, LEN2, K_RAGGED = (70, 5, 1), (65, 64, 1), 16


@pytest.fixture(scope="module")
def ragged():
    from rfnet_amd import _raw
    xyz = clouds("ball", B, N, 70)
    q = xyz[:, :M].copy()
    for i in range(B):
        xyz[i, LEN1[i]:] = np.nan
        q[i, LEN2[i]:] = np.nan
    _, idx = _raw.knn_point(K_RAGGED, cu(xyz), cu(q), lengths1=cu(np.array(LEN1, I32)), lengths2=cu(np.array(LEN2, I32)))
    idx = host(idx).copy()
    for i in range(B):
        idx[i, LEN2[i]:] = 2 ** 30 + 7  # rows behind the count are not read
    return xyz, idx


def test_ragged_batch_equals_the_slices(ragged):
    xyz, idx = ragged
    exp = check_pca("ragged", xyz, idx, LEN1, LEN2)
    vp = viewpoints(xyz, 6)
    got = run_pca(xyz, idx, LEN1, LEN2, vp)
    for i in range(B):
        L1, L2 = LEN1[i], LEN2[i]
        alone = run_pca(xyz[i:i + 1, :L1], idx[i:i + 1, :L2], None, None, vp[i:i + 1])
        one = run_pca(xyz[i:i + 1], idx[i:i + 1], LEN1[i:i + 1], LEN2[i:i + 1], vp[i:i + 1])
        for name, g, a, o in zip(("normals", "eigenvalues", "axes"), got, alone, one):
            same_bytes(f"sample {i}: {name} against the call on the slices", g[i, :L2], a[0])
            same_bytes(f"sample {i}: {name} against the [i : i + 1] call", g[i], o[0])
            assert not g[i, L2:].view(np.uint32).any(), f"sample {i}: padded rows of {name} are not +0"
    assert np.isfinite(exp[1][0]).all() and not exp[1][2, 0].any()  # the one-point cloud: a zero covariance


# ---- 3. isolation -----------------------------------------------------------------------------------------------------------
def test_a_nan_point_changes_only_the_rows_that_name_it():
    from rfnet_amd import _raw
    k = 16
    xyz = clouds("ball", B, N, 80)
    _, idx = _raw.knn_point(k, cu(xyz), cu(xyz[:, :M]))
    idx = host(idx)
    clean = run_pca(xyz, idx)
    again = run_pca(xyz, idx)
    for a, c in zip(again, clean):
        assert a.tobytes() == c.tobytes()  # two calls, the same bytes
    bad = xyz.copy()
    bad[1, 17, 1] = np.nan
    got = run_pca(bad, idx)
    names = (idx[1] == 17).any(-1)
    assert 0 < names.sum() < M
    for name, g, c in zip(("normals", "eigenvalues", "axes"), got, clean):
        same_bytes(f"{name} of the other samples", g[[0, 2]], c[[0, 2]])
        same_bytes(f"{name} of the rows that do not name the point", g[1][~names], c[1][~names])
    assert (got[1][1][names].view(np.uint32) == QNAN_BITS).all()
    assert not got[0][1][names].view(np.uint32).any() and not got[2][1][names].view(np.uint32).any()


# ---- 4. estimate_normals on large clouds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", [(2, 4096), (1, 16384)])  # the scan of knn_point, and its walk over the sorted sets
def test_estimate_normals_is_the_restatement_on_knn_points_idx(b, n):
    from rfnet_amd import _raw, glue
    k = 16
    rng = np.random.RandomState(n)
    p = rng.randn(b, n, 3)
    xyz = (p / np.linalg.norm(p, axis=-1, keepdims=True) * (1 + 0.002 * rng.randn(b, n, 1))).astype(F32)  # a noisy sphere
    assert _raw.knn_auto_boxes(k, n, n) == (n >= 16384)
    x = cu(xyz)
    vp = np.array([0.0, 0.0, 4.0], F32)
    nrm, eig = glue.estimate_normals(x, k, viewpoint=vp)
    _, idx = _raw.knn_point(k, x, x)
    exp = pca_ref(xyz, host(idx), viewpoint=np.repeat(vp[None], b, 0))
    same_bytes("normals", host(nrm), exp[0])
    same_bytes("eigenvalues", host(eig), exp[1])
    # and they are normals: on a sphere seen from outside along z, those of the upper cap point outwards
    cap = xyz[..., 2] > 0.5
    assert ((host(nrm) * xyz).sum(-1)[cap] > 0.8).all()


# ---- 5. normal consistency --------------------------------------------------------------------------------------------------
NC_N, NC_M = 70, 130
NC_LEN1, NC_LEN2 = (70, 5, 1), (130, 64, 1)


def unit_normals(seed, *shape):
    v = np.random.RandomState(seed).randn(*shape, 3)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def check_nc(what, got, n1, n2, i1, i2, l1=None, l2=None):
    ref, mean_abs, Ls = nc_ref(n1, n2, i1, i2, l1, l2)
    err, bar = np.abs(got.astype(np.float64) - ref), nc_bound(ref, mean_abs, Ls)
    print(f"{what}: max error {err.max():.3e}, smallest bound {bar.min():.3e}, worst error / bound {(err / np.where(bar > 0, bar, 1)).max():.3f}")
    assert (err <= bar).all(), f"{what}: {err} against {bar}"
    return ref


@pytest.mark.parametrize("is_ragged", [False, True], ids=["dense", "ragged"])
def test_normal_consistency_against_float64(is_ragged):
    from rfnet_amd import _raw
    x1, x2 = clouds("ball", B, NC_N, 90), clouds("ball", B, NC_M, 91)
    n1, n2 = unit_normals(92, B, NC_N), unit_normals(93, B, NC_M)
    l1, l2 = (NC_LEN1, NC_LEN2) if is_ragged else (None, None)
    if is_ragged:
        for i in range(B):
            for t, L in ((x1, l1), (n1, l1), (x2, l2), (n2, l2)):
                t[i, L[i]:] = np.nan
    dl1, dl2 = (cu(np.array(l1, I32)), cu(np.array(l2, I32))) if is_ragged else (None, None)
    _, i1, _, i2 = _raw.nn_distance(cu(x1), cu(x2), lengths1=dl1, lengths2=dl2)
    got = host(_raw.nn_normal_consistency(cu(n1), cu(n2), i1, i2, dl1, dl2))
    assert got.shape == (B, 4) and got.dtype == F32
    ref = check_nc("rf_nn_normal_consistency", got, n1, n2, host(i1), host(i2), l1, l2)
    assert (ref[:, :2] > 0).all() and (np.abs(ref[:, 2:]) <= ref[:, :2]).all()
    again = host(_raw.nn_normal_consistency(cu(n1), cu(n2), i1, i2, dl1, dl2))
    assert again.tobytes() == got.tobytes()
    if is_ragged:  # a sample does not depend on its batch
        for i in range(B):
            one = host(_raw.nn_normal_consistency(cu(n1[i:i + 1]), cu(n2[i:i + 1]), i1[i:i + 1], i2[i:i + 1], dl1[i:i + 1], dl2[i:i + 1]))
            assert one.tobytes() == got[i:i + 1].tobytes()


def test_normal_consistency_identities():
    from rfnet_amd import _raw, glue
    x = clouds("ball", B, NC_N, 95)
    # signed axis vectors: every dot of a normal with itself is exactly 1
    rng = np.random.RandomState(96)
    nrm = np.zeros((B, NC_N, 3), F32)
    nrm[np.arange(B)[:, None], np.arange(NC_N)[None], rng.randint(0, 3, (B, NC_N))] = rng.choice([-1.0, 1.0], (B, NC_N))
    r = glue.normal_consistency(cu(x), cu(x), cu(nrm), cu(nrm))
    assert set(r) == {"nc", "nc12", "nc21", "signed12", "signed21"}
    for key in r:
        assert r[key].shape == (B,) and (host(r[key]) == 1.0).all(), key
    r = glue.normal_consistency(cu(x), cu(x), cu(nrm), cu(-nrm))
    assert (host(r["nc"]) == 1.0).all() and (host(r["signed12"]) == -1.0).all() and (host(r["signed21"]) == -1.0).all()
    n1 = unit_normals(97, B, NC_N)
    r = glue.normal_consistency(cu(x), cu(x), cu(n1), cu(-n1))
    for d in ("12", "21"):
        assert host(r["signed" + d]).tobytes() == (-host(r["nc" + d])).tobytes()  # signed = -abs, exactly
    # an index outside the other cloud and a zero normal contribute 0
    i1 = np.tile(np.arange(NC_N, dtype=I32), (B, 1))
    i2 = i1.copy()
    i1[:, 3], i1[:, 4], i2[:, 5] = NC_N, -1, 2 ** 31 - 1
    hurt = nrm.copy()
    hurt[:, 9] = 0
    got = host(_raw.nn_normal_consistency(cu(hurt), cu(nrm), cu(i1), cu(i2)))
    assert (got[:, 0] == F32((NC_N - 3) / NC_N)).all() and (got[:, 1] == F32((NC_N - 2) / NC_N)).all()
    assert np.array_equal(got[:, 2:], got[:, :2])
    check_nc("hand-made idx", got, hurt, nrm, i1, i2)
    # estimated normals: a cloud against itself is exactly consistent
    r = glue.normal_consistency(cu(x), cu(x), k=8)
    assert (np.abs(host(r["nc"]) - 1.0) <= 2.0 ** -22).all()


# ---- 6. capture -------------------------------------------------------------------------------------------------------------
def test_estimate_normals_and_normal_consistency_captured():
    from rfnet_amd import glue
    n, m, k = 200, 150, 8
    sets = []
    for v in range(2):
        sets.append(dict(x1=clouds("ball", B, n, 100 + v), x2=clouds("plane", B, m, 110 + v), vp=np.array([[0.5, -2.0, 1.0], [3.0, 0.1, -1.0]][v], F32),
                         l1=np.array([[n, 9, 120], [64, n, 30]][v], I32), l2=np.array([[m, 77, 3], [5, 140, m]][v], I32)))
    t = {nm: cu(a) for nm, a in sets[0].items()}

    def chain():
        nrm, eig = glue.estimate_normals(t["x1"], k, lengths=t["l1"], viewpoint=t["vp"])
        nc = glue.normal_consistency(t["x1"], t["x2"], normals1=nrm, k=k, lengths1=t["l1"], lengths2=t["l2"])
        return nrm, eig, nc["nc"], nc["signed12"], nc["signed21"]

    def load(s):
        for nm, a in s.items():
            t[nm].copy_(cu(a))

    eager = []
    for s in (sets[1], sets[0]):
        load(s)
        eager.insert(0, [host(o).copy() for o in chain()])
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        chain()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for v in (0, 1):
        load(sets[v])  # inputs and counts change in place, on the device: nothing is read back
        graph.replay()
        torch.cuda.synchronize()
        for name, got, exp in zip(("normals", "eigenvalues", "nc", "signed12", "signed21"), outs, eager[v]):
            assert host(got).tobytes() == exp.tobytes(), f"replay on set {v}: {name} differs from the eager bits"
    assert eager[0][0].tobytes() != eager[1][0].tobytes()
