"""GPU: the memory contract of include/rfops.h for rf_knn_feature, straight through the C ABI: val and idx exactly (b, m, k), the
workspace exactly what rf_knn_feature_workspace_bytes states and poisoned, the features and the count arrays at the residues the
header allows (4 bytes; the workspace 16), ragged counts with 1, fewer than k and the full size among them over NaN padding; after
the call every byte outside the outputs and the workspace is unchanged, every output slot is written, and the outputs are the
bits of the numpy restatement (tests/test_knn_feature_host.py).  A workspace one byte short is answered with RF_EWORKSPACE and
nothing is touched.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_vector_attention.py does; `test_memory_contract_knn_feature` runs them."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_knn_feature_host import knn_feature_ref

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, M, C, K = 3, 131, 67, 33, 17
LEN1, LEN2 = np.array([N, 1, K - 2], I32), np.array([33, M, 1], I32)
EWORKSPACE = -2


def _ref(ragged):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((B, 1, C))
    r = dict(f1=(base + 0.01 * rng.standard_normal((B, N, C))).astype(F32), f2=(base + 0.01 * rng.standard_normal((B, M, C))).astype(F32))
    if ragged:
        for i in range(B):
            r["f1"][i, LEN1[i]:] = np.nan
            r["f2"][i, LEN2[i]:] = np.nan
    r["val"], r["idx"] = knn_feature_ref(K, r["f1"], r["f2"], LEN1 if ragged else None, LEN2 if ragged else None)
    return r


def _knn_feature(x, ragged):
    r = x.ref(lambda: _ref(ragged))
    A = x.arena()
    A.add("f1", r["f1"], F32, "in", x.T)
    A.add("f2", r["f2"], F32, "in", x.res(12))
    if ragged:
        A.add("l1", LEN1, I32, "in", x.L)
        A.add("l2", LEN2, I32, "in", x.L)
    A.add("val", (B, M, K), F32, "out", x.res(8))
    A.add("idx", (B, M, K), I32, "out", x.res(4))
    need = x.lib.rf_knn_feature_workspace_bytes(B, N, M, C, K)
    assert need >= 4 * B * (N + M)
    ws, wsz = x.ws(A, need)
    A.build()
    l1, l2 = ("l1", "l2") if ragged else (None, None)
    st = x.lib.rf_knn_feature(B, N, M, C, K, A.ptr("f1"), A.ptr("f2"), A.ptr(l1), A.ptr(l2), A.ptr("val"), A.ptr("idx"), A.ptr(ws),
                              wsz - 1, None)
    torch.cuda.synchronize()
    assert st == EWORKSPACE and A.still_poison("val") and A.still_poison("idx") and A.still_poison(ws)
    x.call(A, "rf_knn_feature", B, N, M, C, K, "f1", "f2", l1, l2, "val", "idx", ws, wsz, None)
    val, idx = A.get("val"), A.get("idx")
    assert val.shape == (B, M, K) and val.tobytes() == r["val"].tobytes(), f"{x.cid}: val differs from the restatement"
    assert np.array_equal(idx, r["idx"]), f"{x.cid}: idx differs from the restatement"
    assert np.isfinite(val).all()  # every slot written: no poison, no NaN from the padding
    if ragged:
        for i in range(B):
            kv = min(K, LEN1[i])
            assert not val[i, LEN2[i]:].view(np.uint32).any() and not idx[i, LEN2[i]:].any()
            assert not val[i, :, kv:].view(np.uint32).any() and not idx[i, :, kv:].any()
    x.keep("val", val)
    x.keep("idx", idx)


@own("rf_knn_feature")
def knn_feature_dense(x):
    _knn_feature(x, False)


@own("rf_knn_feature")
def knn_feature_ragged(x):
    _knn_feature(x, True)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_knn_feature(orc, cid, variant, poison):
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
