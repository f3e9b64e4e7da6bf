"""GPU: the memory contract of include/rfops.h for rf_local_pca and rf_nn_normal_consistency, straight through the C ABI: the
outputs exactly (b, m, 3), (b, m, 3), (b, m, 3, 3) and (b, 4), no workspace, every tensor and count array at the residues the
header allows (4 bytes), ragged counts with 1, fewer than k and the full size among them; the rows behind a count hold NaN
(points, normals) or indices of such rows (idx): read, they would show in the outputs.  After the call every byte outside the
outputs is unchanged, every output slot is written, and the outputs are the restatements of tests/test_normals_host.py -- pca_ref
as bytes, nc_ref within its bound.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_knn_feature.py does; `test_memory_contract_normals` runs them."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_normals_host import family_cloud, nc_bound, nc_ref, pca_ref

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, M, K = 3, 131, 67, 17
LEN1, LEN2 = np.array([N, 1, K - 2], I32), np.array([33, M, 1], I32)


def _pca_ref(ragged, viewpoint):
    rng = np.random.RandomState(5)
    r = dict(xyz=np.stack([family_cloud("ball", N, 20 + i) for i in range(B)]), idx=rng.randint(0, N, (B, M, K)).astype(I32))
    r["idx"][rng.rand(B, M, K) < 0.1] = -1  # skipped slots
    if ragged:
        for i in range(B):
            r["idx"][i] = rng.randint(0, LEN1[i], (M, K))
            r["xyz"][i, LEN1[i]:] = np.nan
            r["idx"][i, LEN2[i]:] = N - 1  # a NaN row, were it read and used
    r["vp"] = rng.randn(B, 3).astype(F32) if viewpoint else None
    r["out"] = pca_ref(r["xyz"], r["idx"], LEN1 if ragged else None, LEN2 if ragged else None, r["vp"])
    return r


def _local_pca(x, ragged, viewpoint, axes):
    r = x.ref(lambda: _pca_ref(ragged, viewpoint))
    A = x.arena()
    A.add("xyz", r["xyz"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.res(12))
    if ragged:
        A.add("l1", LEN1, I32, "in", x.L)
        A.add("l2", LEN2, I32, "in", x.L)
    if viewpoint:
        A.add("vp", r["vp"], F32, "in", x.res(8))
    A.add("nrm", (B, M, 3), F32, "out", x.res(8))
    A.add("eig", (B, M, 3), F32, "out", x.res(4))
    if axes:
        A.add("axes", (B, M, 3, 3), F32, "out", x.T)
    A.build()
    l1, l2 = ("l1", "l2") if ragged else (None, None)
    x.call(A, "rf_local_pca", B, N, M, K, "xyz", "idx", l1, l2, "vp" if viewpoint else None, "nrm", "eig", "axes" if axes else None, None)
    for name, exp in zip(("nrm", "eig", "axes") if axes else ("nrm", "eig"), r["out"]):
        got = A.get(name)
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)
    assert np.isfinite(A.get("nrm")).all()  # every slot written: no poison, nothing from the padding
    if ragged:
        for i in range(B):
            assert not A.get("eig")[i, LEN2[i]:].view(np.uint32).any() and not A.get("nrm")[i, LEN2[i]:].view(np.uint32).any()


@own("rf_local_pca")
def local_pca_dense(x):
    _local_pca(x, False, True, True)


@own("rf_local_pca")
def local_pca_dense_normals_only(x):
    _local_pca(x, False, False, False)


@own("rf_local_pca")
def local_pca_ragged(x):
    _local_pca(x, True, True, True)


NC_N, NC_M = 131, 203
NC_LEN1, NC_LEN2 = np.array([NC_N, 1, 40], I32), np.array([77, NC_M, 1], I32)


def _nc_ref(ragged):
    rng = np.random.RandomState(9)
    r = dict(n1=rng.randn(B, NC_N, 3).astype(F32), n2=rng.randn(B, NC_M, 3).astype(F32))
    r["i1"], r["i2"] = rng.randint(0, NC_M, (B, NC_N)).astype(I32), rng.randint(0, NC_N, (B, NC_M)).astype(I32)
    if ragged:
        for i in range(B):
            r["i1"][i], r["i2"][i] = rng.randint(0, NC_LEN2[i], NC_N), rng.randint(0, NC_LEN1[i], NC_M)
            r["n1"][i, NC_LEN1[i]:], r["n2"][i, NC_LEN2[i]:] = np.nan, np.nan
    r["i1"][:, 0] = -1  # an index outside the other cloud
    r["ref"] = nc_ref(r["n1"], r["n2"], r["i1"], r["i2"], NC_LEN1 if ragged else None, NC_LEN2 if ragged else None)
    return r


def _normal_consistency(x, ragged):
    r = x.ref(lambda: _nc_ref(ragged))
    A = x.arena()
    A.add("n1", r["n1"], F32, "in", x.T)
    A.add("n2", r["n2"], F32, "in", x.res(12))
    A.add("i1", r["i1"], I32, "in", x.res(8))
    A.add("i2", r["i2"], I32, "in", x.T)
    if ragged:
        A.add("l1", NC_LEN1, I32, "in", x.L)
        A.add("l2", NC_LEN2, I32, "in", x.L)
    A.add("out", (B, 4), F32, "out", x.res(4))
    A.build()
    l1, l2 = ("l1", "l2") if ragged else (None, None)
    x.call(A, "rf_nn_normal_consistency", B, NC_N, NC_M, "n1", "n2", "i1", "i2", l1, l2, "out", None)
    out = A.get("out")
    ref, mean_abs, Ls = r["ref"]
    assert out.shape == (B, 4) and np.isfinite(out).all()
    assert (np.abs(out.astype(np.float64) - ref) <= nc_bound(ref, mean_abs, Ls)).all(), f"{x.cid}: out differs from float64"
    x.keep("out", out)  # a fixed summation order: bit-equal across the runs


@own("rf_nn_normal_consistency")
def normal_consistency_dense(x):
    _normal_consistency(x, False)


@own("rf_nn_normal_consistency")
def normal_consistency_ragged(x):
    _normal_consistency(x, True)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_normals(orc, cid, variant, poison):
    x = T.Ctx(cid, variant, poison, orc)
    T._SEEN[cid] = T._SEEN.get(cid, 0) + 1
    try:
        T.CASES[cid][1](x)
        assert x.kept, "a case must check at least one output"
        x.across_runs()
    finally:
        if T._SEEN[cid] == T.RUNS_PER_CASE:
            T._REFS.pop(cid, None)
            T._RUNS.pop(cid, None)
