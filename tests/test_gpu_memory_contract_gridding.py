"""GPU: the memory contract of include/rfops.h for rf_gridding_loss, rf_gridding and rf_gridding_grad, straight
through the C ABI: `loss` exactly b floats, `inside` exactly (b, 2) or (b) int32, the gradients exactly (b, n, 3) and (b, m, 3),
the grid exactly (b, R, R, R), the workspace exactly what the _workspace_bytes function states and poisoned, inputs and count
arrays at the residues the header allows (4 bytes; the workspace 16), ragged counts with 1 and the full size among them over NaN
padding; after the call every byte outside the outputs and the workspace is unchanged, every output slot is written, and the
outputs are the bits of the plain call.  The loss in both forms: loss only (the gradient pointers NULL) and with gradients.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module
is imported, exactly as tests/test_gpu_memory_contract_sliced.py does; `test_memory_contract_gridding` runs them."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_gridding_host import BOUNDS, DENSITY, family

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, M, R = 3, 257, 130, 33  # 3^3 bricks, the last of them one vertex wide
LO, HI = BOUNDS[1]
LEN1 = np.array([N, 1, 129], I32)
LEN2 = np.array([77, M, 1], I32)


def _ref():
    """Inputs with NaN behind the counts, and the plain calls' outputs on them."""
    from rfnet_amd import _raw
    a = np.stack([family(k, 50 + i, N, R, LO, HI) for i, k in enumerate(("uniform", "seams", "outside"))])
    c = np.stack([family(k, 60 + i, M, R, LO, HI) for i, k in enumerate(("nonfinite", "uniform", "vertices"))])
    for i in range(B):
        a[i, LEN1[i]:] = np.nan
        c[i, LEN2[i]:] = np.nan
    gg = np.random.RandomState(7).randn(B, R, R, R).astype(F32)
    ta, l1 = torch.from_numpy(a).cuda(), torch.from_numpy(LEN1).cuda()
    out = _raw.gridding_loss(ta, torch.from_numpy(c).cuda(), R, LO, HI, "density", l1, torch.from_numpy(LEN2).cuda(),
                             want_grad=True)
    grid, cnt = _raw.gridding(ta, R, LO, HI, l1)
    gx = _raw.gridding_grad(ta, torch.from_numpy(gg).cuda(), R, LO, HI, l1)
    r = dict(a=a, c=c, gg=gg, grid=grid, cnt=cnt, gx=gx, **dict(zip(("loss", "inside", "g1", "g2"), out)))
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _same(x, A, r, names):
    for k in names:
        got = A.get(k)
        # every slot written (no poison left: the padded slots are +0) and the bits of the plain call
        assert got.shape == r[k].shape and got.tobytes() == r[k].tobytes(), f"{x.cid}: {k} differs from the plain call"
        x.keep(k, got)


def _loss(x, grad):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("loss", (B,), F32, "out", x.T)
    A.add("inside", (B, 2), I32, "out", x.res(12))
    if grad:
        A.add("g1", (B, N, 3), F32, "out", x.res(4))
        A.add("g2", (B, M, 3), F32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_gridding_loss_workspace_bytes(B, N, M, R, 1 if grad else 0))
    A.build()
    x.call(A, "rf_gridding_loss", B, N, M, R, LO, HI, DENSITY, "a", "c", "l1", "l2", "loss", "inside", "g1" if grad else None,
           "g2" if grad else None, ws, wsz, None)
    _same(x, A, r, ("loss", "inside") + (("g1", "g2") if grad else ()))
    assert np.isfinite(A.get("loss")).all() and (A.get("loss") >= 0).all() and A.get("loss")[0] > 0
    assert A.get("inside")[0, 0] == N and A.get("inside")[0, 1] < 77  # (cloud 2 of sample 0 has non-finite rows)
    if grad:
        for i in range(B):  # exactly +0 behind the counts
            assert not A.get("g1")[i, LEN1[i]:].view(np.uint32).any() and not A.get("g2")[i, LEN2[i]:].view(np.uint32).any()


@own("rf_gridding_loss")
def gridding_loss_only(x):
    _loss(x, False)


@own("rf_gridding_loss")
def gridding_loss_with_gradients(x):
    _loss(x, True)


@own("rf_gridding")
def gridding_layer(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("grid", (B, R, R, R), F32, "out", x.res(4))
    A.add("cnt", (B,), I32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_gridding_workspace_bytes(B, N, R))
    A.build()
    x.call(A, "rf_gridding", B, N, R, LO, HI, "a", "l1", "grid", "cnt", ws, wsz, None)
    _same(x, A, r, ("grid", "cnt"))
    assert np.isfinite(A.get("grid")).all() and A.get("cnt")[0] == N and A.get("cnt")[1] == 1


@own("rf_gridding_grad")
def gridding_layer_grad(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("gg", r["gg"], F32, "in", x.res(8))
    A.add("gx", (B, N, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_gridding_grad", B, N, R, LO, HI, "a", "l1", "gg", "gx", None)
    _same(x, A, r, ("gx",))
    for i in range(B):
        assert not A.get("gx")[i, LEN1[i]:].view(np.uint32).any()
    assert np.abs(A.get("gx")).max() > 0


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_gridding(orc, cid, variant, poison):
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
