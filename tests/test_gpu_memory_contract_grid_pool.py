"""GPU: the memory contract of include/rfops.h for rf_grid_cluster, rf_grid_pool and rf_grid_unpool, straight through the C ABI:
the outputs exactly (b, 3), (b), (b), (b, n), (b, n + 1), (b, n), (b, n, 3), (b, n) int64 and (b, n, c), no workspace, every
tensor and count array at the residues the header allows (4 bytes; 8 for the int64 code), ragged counts with 1 and the full size
among them and NaN rows behind them.  After the call every byte outside the outputs is unchanged, every output element is
written (the poison is gone: the outputs equal the restatement of tests/grid_pool_ref.py as bytes), and the four runs of a case
agree bit for bit -- the aligned variant moves rows of c = 12 channels as 16-byte vectors, the natural one as floats.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_normals.py does; `test_memory_contract_grid_pool` runs them."""
import numpy as np
import pytest

import grid_pool_ref as R
import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, C = 3, 331, 12
CELL = 0.11
LEN = np.array([N, 1, 77], I32)
ORDER_ID = {"xyz": 0, "z": 1, "hilbert": 2}
OUTS = (("origin", (B, 3), F32, 8), ("inside", (B,), I32, 4), ("nclusters", (B,), I32, 12), ("order", (B, N), I32, 4),
        ("starts", (B, N + 1), I32, 8), ("cluster", (B, N), I32, 12), ("coords", (B, N, 3), I32, 4))


def _inputs(ragged, origin, order):
    rng = np.random.RandomState(11)
    xyz = (rng.rand(B, N, 3) - 0.5).astype(F32)
    xyz[0, 7] = np.nan
    xyz[0, 9, 2] = -np.inf
    xyz[2, 5] = 1e30
    if ragged:
        for i in range(B):
            xyz[i, LEN[i]:] = np.nan
    r = dict(xyz=xyz, og=(rng.rand(B, 3) + 0.6).astype(F32) if origin else None)
    r["out"] = R.cluster_ref(xyz, CELL, order, LEN if ragged else None, r["og"])
    return r


def _grid_cluster(x, ragged, origin, order, code):
    r = x.ref(lambda: _inputs(ragged, origin, order))
    A = x.arena()
    A.add("xyz", r["xyz"], F32, "in", x.T)
    if ragged:
        A.add("len", LEN, I32, "in", x.L)
    if origin:
        A.add("og", r["og"], F32, "in", x.res(12))
    for name, shape, dt, res in OUTS:
        A.add(name, shape, dt, "out", x.res(res))
    if code:
        A.add("code", (B, N), np.int64, "out", x.res(8))
    A.build()
    x.call(A, "rf_grid_cluster", B, N, CELL, ORDER_ID[order], "xyz", "len" if ragged else None, "og" if origin else None,
           *(name for name, *_ in OUTS), "code" if code else None, None)
    for name in [o[0] for o in OUTS] + (["code"] if code else []):
        got, exp = A.get(name), r["out"][name]
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)


@own("rf_grid_cluster")
def grid_cluster_dense_with_code(x):
    _grid_cluster(x, False, False, "hilbert", True)


@own("rf_grid_cluster")
def grid_cluster_ragged_with_origin(x):
    _grid_cluster(x, True, True, "z", False)


@own("rf_grid_cluster")
def grid_cluster_ragged_xyz_with_code(x):
    _grid_cluster(x, True, False, "xyz", True)


def _pool_inputs():
    rng = np.random.RandomState(13)
    r = _inputs(True, False, "xyz")
    r["feat"] = (rng.randn(B, N, C) * 4).astype(F32)
    r["feat"][rng.rand(B, N, C) < 0.05] = np.nan  # (max copies a NaN as it is; sum and mean get the clean copy)
    r["clean"] = np.nan_to_num(r["feat"], nan=0.5)
    r["grad"] = rng.randn(B, N, C).astype(F32)
    k = (r["out"]["order"], r["out"]["starts"], r["out"]["nclusters"])
    r["sum"], r["mean"] = R.pool_ref(r["clean"], *k, "sum"), R.pool_ref(r["clean"], *k, "mean")
    r["max"], r["arg"] = R.pool_ref(r["feat"], *k, "max")
    return r


def _grid_pool(x, reduce):
    r = x.ref(_pool_inputs)
    A = x.arena()
    A.add("feat", r["feat"] if reduce == "max" else r["clean"], F32, "in", x.T)
    A.add("order", r["out"]["order"], I32, "in", x.res(8))
    A.add("starts", r["out"]["starts"], I32, "in", x.res(12))
    A.add("ncl", r["out"]["nclusters"], I32, "in", x.L)
    A.add("out", (B, N, C), F32, "out", x.T)
    if reduce == "max":
        A.add("arg", (B, N, C), I32, "out", x.T)
    A.build()
    x.call(A, "rf_grid_pool", B, N, C, {"sum": 0, "mean": 1, "max": 2}[reduce], "feat", "order", "starts", "ncl", "out",
           "arg" if reduce == "max" else None, None)
    for name, exp in (("out", r[reduce]),) + ((("arg", r["arg"]),) if reduce == "max" else ()):
        got = A.get(name)
        assert got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)


@own("rf_grid_pool")
def grid_pool_sum(x):
    _grid_pool(x, "sum")


@own("rf_grid_pool")
def grid_pool_mean(x):
    _grid_pool(x, "mean")


@own("rf_grid_pool")
def grid_pool_max(x):
    _grid_pool(x, "max")


def _grid_unpool(x, mode):
    r = x.ref(_pool_inputs)
    A = x.arena()
    A.add("src", r["grad"], F32, "in", x.T)
    A.add("cluster", r["out"]["cluster"], I32, "in", x.res(8))
    if mode == "mean":
        A.add("starts", r["out"]["starts"], I32, "in", x.res(12))
    if mode == "max":
        A.add("arg", r["arg"], I32, "in", x.T)
    A.add("dst", (B, N, C), F32, "out", x.T)
    A.build()
    x.call(A, "rf_grid_unpool", B, N, C, {"copy": 0, "mean": 1, "max": 2}[mode], "src", "cluster",
           "starts" if mode == "mean" else None, "arg" if mode == "max" else None, "dst", None)
    exp = R.unpool_ref(r["grad"], r["out"]["cluster"], starts=r["out"]["starts"], arg=r["arg"], mode=mode)
    got = A.get("dst")
    assert got.tobytes() == exp.tobytes(), f"{x.cid}: dst differs from the restatement"
    x.keep("dst", got)


@own("rf_grid_unpool")
def grid_unpool_copy(x):
    _grid_unpool(x, "copy")


@own("rf_grid_unpool")
def grid_unpool_mean(x):
    _grid_unpool(x, "mean")


@own("rf_grid_unpool")
def grid_unpool_max(x):
    _grid_unpool(x, "max")


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_grid_pool(orc, cid, variant, poison):
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
