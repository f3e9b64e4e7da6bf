"""GPU: the memory contract of include/rfops.h for rf_sliced_wasserstein, straight through the C ABI:
`loss` exactly b floats, the gradients exactly (b, n, 3) and (b, m, 3), the workspace exactly its stated size and
poisoned, inputs, directions and count arrays at the residues the header allows (4 bytes; the workspace 16), ragged
counts with 1 and the full size among them over hostile padding; after the call every byte outside the outputs and the
workspace is unchanged.  Both forms: loss only (the gradient pointers NULL) and loss with gradients.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this
module is imported, exactly as tests/test_gpu_memory_contract_cross.py does; `test_memory_contract_sliced` runs them."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, M, N, case
from test_sliced_host import exact_inputs, sw_ref

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, NPROJ = 3, 19  # 19 directions: two chunks
LEN1 = np.array([N, 1, 129], I32)
LEN2 = np.array([77, M, 1], I32)


def _ref():
    """Sample by sample on the unpadded slices, on inputs whose projections are exact in fp32; padding: NaN behind
    len1, copies of valid xyz1 points behind len2."""
    a, c, d = exact_inputs(47, B, N, M, NPROJ)
    loss, g1, g2 = np.zeros(B), np.zeros((B, N, 3)), np.zeros((B, M, 3))
    for i in range(B):
        loss[i], g1[i], g2[i] = sw_ref(a[i], c[i], d, LEN1[i], LEN2[i])
    for i in range(B):
        a[i, LEN1[i]:] = np.nan
        c[i, LEN2[i]:] = a[i, np.arange(M - LEN2[i]) % LEN1[i]]
    return dict(a=a, c=c, d=d, loss=loss, g1=g1, g2=g2)


def _run(x, grad):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("d", r["d"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("loss", (B,), F32, "out", x.T)
    if grad:
        A.add("g1", (B, N, 3), F32, "out", x.res(4))
        A.add("g2", (B, M, 3), F32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_sliced_wasserstein_workspace_bytes(B, N, M, NPROJ, int(grad)))
    A.build()
    x.call(A, "rf_sliced_wasserstein", B, N, M, NPROJ, "a", "c", "l1", "l2", "d", "loss", "g1" if grad else None,
           "g2" if grad else None, ws, wsz, None)
    loss = A.get("loss")
    assert loss.shape == (B,) and loss.nbytes == B * 4
    # test_gpu_sliced.py's bars on exact-projection inputs; a fixed order: the same bits every run
    x.close("loss", loss, r["loss"], 2.0 ** -23, fixed_order=True)
    if grad:
        for k in ("g1", "g2"):
            g = A.get(k)
            x.close(k, g, r[k], 2.0 ** -23, 1e-12, fixed_order=True)
        for i in range(B):  # exactly +0 behind the counts
            assert not A.get("g1")[i, LEN1[i]:].view(np.uint32).any() and not A.get("g2")[i, LEN2[i]:].view(np.uint32).any()


@own("rf_sliced_wasserstein")
def sliced_wasserstein_loss_only(x):
    _run(x, False)


@own("rf_sliced_wasserstein")
def sliced_wasserstein_with_gradients(x):
    _run(x, True)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_sliced(orc, cid, variant, poison):
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
