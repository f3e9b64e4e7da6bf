"""GPU: the memory contract of include/rfops.h for rf_sinkhorn, straight through the C ABI: `loss` and
`delta` exactly b floats, `pot` exactly (b, n + m), the gradients exactly (b, n, 3) and (b, m, 3), the workspace exactly
rf_sinkhorn_workspace_bytes and poisoned, inputs and count arrays at the residues the header allows (4 bytes; the workspace
16), ragged counts with 1 and the full size among them over NaN padding; after the call every byte outside the outputs and
the workspace is unchanged, every output slot is written, and the outputs are the bits of the plain call.  Both forms:
loss only (the gradient pointers NULL) and loss with gradients.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this
module is imported, exactly as tests/test_gpu_memory_contract_sliced.py does; `test_memory_contract_sinkhorn` runs them."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_sinkhorn_host import clouds, schedule

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, M, P = 3, 257, 130, 2
LEN1 = np.array([N, 1, 129], I32)
LEN2 = np.array([77, M, 1], I32)


def _ref():
    """Inputs with NaN behind the counts, and the plain call's outputs on them."""
    from rfnet_amd import _raw
    pairs = [clouds(50 + i, N, M) for i in range(B)]
    a, c = np.stack([x for x, _ in pairs]), np.stack([y for _, y in pairs])
    for i in range(B):
        a[i, LEN1[i]:] = np.nan
        c[i, LEN2[i]:] = np.nan
    eps = np.asarray(schedule(P, 0.05, 0.5), np.float32)
    out = _raw.sinkhorn(torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda(), eps, P, torch.from_numpy(LEN1).cuda(),
                        torch.from_numpy(LEN2).cuda(), want_grad=True)
    names = ("loss", "pot", "delta", "g1", "g2")
    return dict(a=a, c=c, eps=eps, **{k: t.cpu().numpy() for k, t in zip(names, out)})


def _run(x, grad):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("loss", (B,), F32, "out", x.T)
    A.add("pot", (B, N + M), F32, "out", x.res(8))
    A.add("delta", (B,), F32, "out", x.res(12))
    if grad:
        A.add("g1", (B, N, 3), F32, "out", x.res(4))
        A.add("g2", (B, M, 3), F32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_sinkhorn_workspace_bytes(B, N, M))
    A.build()
    eps = r["eps"]
    x.call(A, "rf_sinkhorn", B, N, M, "a", "c", "l1", "l2", P, eps.ctypes.data_as(ctypes.c_void_p), len(eps), "loss", "pot",
           "delta", "g1" if grad else None, "g2" if grad else None, ws, wsz, None)
    for k in ("loss", "pot", "delta") + (("g1", "g2") if grad else ()):
        got = A.get(k)
        # every slot written (no poison left: the padded slots are +0) and the bits of the plain call
        assert got.shape == r[k].shape and got.tobytes() == r[k].tobytes(), f"{x.cid}: {k} differs from the plain call"
        x.keep(k, got)
    assert np.isfinite(A.get("loss")).all() and (A.get("loss") > 0).all()
    for i in range(B):  # exactly +0 behind the counts
        pot = A.get("pot")[i]
        assert not pot[LEN1[i]:N].view(np.uint32).any() and not pot[N + LEN2[i]:].view(np.uint32).any()
        if grad:
            assert not A.get("g1")[i, LEN1[i]:].view(np.uint32).any() and not A.get("g2")[i, LEN2[i]:].view(np.uint32).any()


@own("rf_sinkhorn")
def sinkhorn_loss_only(x):
    _run(x, False)


@own("rf_sinkhorn")
def sinkhorn_with_gradients(x):
    _run(x, True)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_sinkhorn(orc, cid, variant, poison):
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
