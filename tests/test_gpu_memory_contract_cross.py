"""GPU: the memory contract of include/rfops.h for rf_chamfer_cross, straight through the C ABI: `out`
exactly s * r * 6 floats, the workspace exactly its stated size and poisoned, inputs and count arrays at the residues the
header allows (4 bytes; the workspace 16), ragged counts with 1 and the full size among them over hostile padding; after
the call every byte outside `out` and the workspace is unchanged.

The case uses the machinery of tests/test_gpu_memory_contract.py and registers itself in its CASES table when this module
is imported, exactly as tests/test_gpu_memory_contract_model.py does (see its docstring for what that means for a run of
tests/test_memory_contract_host.py on its own); `test_memory_contract_cross` here runs it."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_chamfer_cross_host import NCOL, cross_ref
from test_gpu_memory_contract import F32, I32, M, N, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


S, R = 3, 4
LEN1 = np.array([N, 1, 129], I32)
LEN2 = np.array([77, M, 1, 64], I32)


def _ref(x):
    """Pair by pair on the unpadded slices; padding: NaN behind len1, copies of valid xyz1 points behind len2 (distance
    0: read, they would win every search)."""
    rng = np.random.RandomState(43)
    a, c = (rng.rand(S, N, 3) - 0.5).astype(F32), (rng.rand(R, M, 3) - 0.5).astype(F32)
    for i, n_ in enumerate(LEN1):
        a[i, n_:] = np.nan
    for j, m_ in enumerate(LEN2):
        c[j, m_:] = a[j % S, np.arange(M - m_) % LEN1[j % S]]
    out = np.zeros((S, R, NCOL))
    for i, n_ in enumerate(LEN1):
        for j, m_ in enumerate(LEN2):
            e = x.orc.nn_distance(a[i:i + 1, :n_].copy(), c[j:j + 1, :m_].copy())
            out[i, j] = cross_ref(e[0][0], e[2][0])
    return dict(a=a, c=c, out=out)


@own("rf_chamfer_cross")
def chamfer_cross_lengths(x):
    r = x.ref(lambda: _ref(x))
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("out", (S, R, NCOL), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_chamfer_cross_workspace_bytes(S, R, N, M))
    A.build()
    x.call(A, "rf_chamfer_cross", S, R, N, M, "a", "c", "l1", "l2", "out", ws, wsz, None)
    out = A.get("out")
    assert out.shape == (S, R, NCOL) and out.nbytes == S * R * NCOL * 4
    x.exact("out[4:6]", out[..., 4:6], r["out"][..., 4:6].astype(F32))
    x.close("out[0:4]", out[..., 0:4], r["out"][..., 0:4], 1e-5, fixed_order=True)  # integer sums: the same bits every run


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_cross(orc, cid, variant, poison):
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
