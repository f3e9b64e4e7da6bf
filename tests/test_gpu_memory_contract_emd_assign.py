"""GPU: the memory contract of include/rfops.h for rf_emd_assign and rf_emd_assign_grad, straight through
the C ABI: match12 / match21 / dist exactly (b, n), val (b, 3), cert (b, 2) 64-bit, info (b, 4), the gradients exactly
(b, n, 3); the workspace exactly its stated size and poisoned (the final prices come back in it); inputs, outputs and the
count array at the residues the header allows (4 bytes; cert 8; the workspace 16); counts with 1 and n among them over
hostile padding; after the call every byte outside the outputs and the workspace is unchanged.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this
module is imported, exactly as tests/test_gpu_memory_contract_sliced.py does; `test_memory_contract_emd_assign` runs them."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_emd_assign_host import ea_family, ea_ref
from test_gpu_emd_assign import grad_close, grad_ref, ulp32
from test_gpu_memory_contract import F32, I32, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N = 3, 131
LEN = np.array([N, 1, 77], I32)
FAMS = ("uniform", "lattice", "dup_both")
GCOST = np.array([1.0, -3.0, 0.6], F32)


def _ref():
    """Sample by sample on the unpadded slices; padding: NaN behind the count in xyz1, copies of valid points in xyz2."""
    a = np.stack([ea_family(f, N, 61 + i)[0] for i, f in enumerate(FAMS)])
    c = np.stack([ea_family(f, N, 61 + i)[1] for i, f in enumerate(FAMS)])
    refs = [ea_ref(a[i, :LEN[i]].copy(), c[i, :LEN[i]].copy()) for i in range(B)]
    for i in range(B):
        a[i, LEN[i]:] = np.nan
        c[i, LEN[i]:] = c[i, np.arange(N - LEN[i]) % LEN[i]]
    m12, m21, dist = np.zeros((B, N), I32), np.zeros((B, N), I32), np.zeros((B, N), F32)
    g1, g2 = np.zeros((B, N, 3)), np.zeros((B, N, 3))
    for i, r in enumerate(refs):
        L = LEN[i]
        m12[i, :L], m21[i, :L], dist[i, :L] = r["match12"], r["match21"], r["dist"]
        g1[i, :L], g2[i, :L] = grad_ref(a[i, :L], c[i, :L], r, L, float(GCOST[i]))
    return dict(a=a, c=c, refs=refs, m12=m12, m21=m21, dist=dist, g1=g1, g2=g2)


@own("rf_emd_assign")
def emd_assign_ragged(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("len", LEN, I32, "in", x.L)
    A.add("m12", (B, N), I32, "out", x.T)
    A.add("m21", (B, N), I32, "out", x.res(12))
    A.add("dist", (B, N), F32, "out", x.T)
    A.add("val", (B, 3), F32, "out", x.res(4))
    A.add("cert", (B, 2), np.int64, "out", x.res(8))
    A.add("info", (B, 4), I32, "out", x.T)
    need = x.lib.rf_emd_assign_workspace_bytes(B, N)
    assert need == (4 * B * N + 255) // 256 * 256
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_emd_assign", B, N, "a", "c", "len", 0, "m12", "m21", "dist", "val", "cert", "info", ws, wsz, None)
    assert A.get("m12").nbytes == B * N * 4 and A.get("cert").nbytes == B * 16 and A.get("val").nbytes == B * 12
    x.exact("match12", A.get("m12"), r["m12"])
    x.exact("match21", A.get("m21"), r["m21"])
    assert np.array_equal(A.get("dist").view(np.uint32), r["dist"].view(np.uint32))  # +0.0f behind the counts included
    x.keep("dist", A.get("dist"))
    refs = r["refs"]
    x.exact("cert", A.get("cert"), np.array([[q["P"], q["D"]] for q in refs], np.int64))
    x.exact("info", A.get("info"), np.array([[q["status"], q["rounds"], q["bids"], q["k"]] for q in refs], I32))
    val = A.get("val")
    for i, q in enumerate(refs):
        assert abs(float(val[i, 0]) - q["cost64"]) <= ulp32(q["cost64"]) and val[i, 1] == q["gap"] and val[i, 2] == q["bound"]
    x.keep("val", val)
    # the workspace holds the final prices of the valid slots: D can be recomputed from them
    prices = A.get("ws")[:4 * B * N].view(I32).reshape(B, N)
    for i, q in enumerate(refs):
        assert np.array_equal(prices[i, :LEN[i]], q["prices"])


@own("rf_emd_assign_grad")
def emd_assign_grad_ragged(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("m12", r["m12"], I32, "in", x.T)
    A.add("m21", r["m21"], I32, "in", x.T)
    A.add("len", LEN, I32, "in", x.L)
    A.add("g", GCOST, F32, "in", x.T)
    A.add("g1", (B, N, 3), F32, "out", x.res(4))
    A.add("g2", (B, N, 3), F32, "out", x.res(8))
    A.build()
    x.call(A, "rf_emd_assign_grad", B, N, "a", "c", "m12", "m21", "len", "g", "g1", "g2", None)
    for k in ("g1", "g2"):
        g = A.get(k)
        assert g.shape == (B, N, 3) and g.nbytes == B * N * 12
        grad_close(g, r[k], k)  # test_gpu_emd_assign.py's bar; exactly +0 behind the counts and where d = 0
        x.keep(k, g)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_emd_assign(orc, cid, variant, poison):
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
