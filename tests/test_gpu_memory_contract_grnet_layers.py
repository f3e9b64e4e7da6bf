"""GPU: the memory contract of include/rfops.h for rf_cubic_feature_sampling, rf_cubic_feature_sampling_grad, rf_gridding_reverse
and rf_gridding_reverse_grad, straight through the C ABI: `feat` exactly (b, n, 8, c), `grad_vol` exactly
(b, c, R, R, R), `points` / `row` / `count` exactly (b, M, 3) / (b, M) / (b), `grad_grid` exactly (b, R, R, R), the workspaces exactly
what the two _workspace_bytes functions state and poisoned, inputs and count arrays at the residues the header allows (4 bytes; the
workspace 16), ragged counts with 1 and the full size among them over NaN padding; after the call every byte outside the outputs
and the workspace is unchanged, every output slot is written, and the outputs are the bits of the plain call.  A workspace one byte
short is answered with RF_EWORKSPACE and nothing is touched.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_gridding.py does; `test_memory_contract_grnet_layers` runs them."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_gridding_host import BOUNDS
from test_grnet_layers_host import cloud, grev_grids

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, C, R = 3, 257, 9, 17  # 3^3 sub-bricks, the last of them one vertex wide; two channel chunks, the second one channel wide
M = (R - 1) ** 3
LO, HI = BOUNDS[1]
LEN = np.array([N, 1, 129], I32)
EPS = 1e-6
EWORKSPACE = -2


def _ref():
    """Inputs with NaN behind the counts, and the plain calls' outputs on them."""
    from rfnet_amd import _raw
    a = np.stack([cloud(k, 50 + i, N, R, LO, HI) for i, k in enumerate(("uniform", "seams", "outside"))])
    gf = np.random.RandomState(7).randint(-1024, 1025, (B, N, 8, C)).astype(F32)  # exact sums: the bits are promised
    for i in range(B):
        a[i, LEN[i]:] = np.nan
        gf[i, LEN[i]:] = np.nan
    vol = np.random.RandomState(8).randn(B, C, R, R, R).astype(F32)
    grid = np.stack([grev_grids(k, 60 + i, R) for i, k in enumerate(("dense", "wild", "zeros"))])
    gp = np.random.RandomState(9).randn(B, M, 3).astype(F32)
    ta, tl = torch.from_numpy(a).cuda(), torch.from_numpy(LEN).cuda()
    feat, inside = _raw.cubic_feature_sampling(ta, torch.from_numpy(vol).cuda(), LO, HI, tl)
    gv = _raw.cubic_feature_sampling_grad(ta, torch.from_numpy(gf).cuda(), R, LO, HI, tl)
    r = dict(a=a, gf=gf, vol=vol, grid=grid, gp=gp, feat=feat, inside=inside, gv=gv)
    for compact in (0, 1):
        pts, row, cnt = _raw.gridding_reverse(torch.from_numpy(grid).cuda(), LO, HI, EPS, bool(compact))
        gg = _raw.gridding_reverse_grad(torch.from_numpy(grid).cuda(), row, torch.from_numpy(gp).cuda(), LO, HI)
        r.update({f"pts{compact}": pts, f"row{compact}": row, f"cnt{compact}": cnt, f"gg{compact}": gg})
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _same(x, A, r, names):
    for k, rk in names:
        got = A.get(k)
        # every slot written (no poison left: the padded slots are +0) and the bits of the plain call
        assert got.shape == r[rk].shape and got.tobytes() == r[rk].tobytes(), f"{x.cid}: {k} differs from the plain call"
        x.keep(k, got)


@own("rf_cubic_feature_sampling")
def cubic_feature_sampling(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("vol", r["vol"], F32, "in", x.res(8))
    A.add("feat", (B, N, 8, C), F32, "out", x.res(4))
    A.add("inside", (B,), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_cubic_feature_sampling", B, N, C, R, LO, HI, "a", "ln", "vol", "feat", "inside", None)
    _same(x, A, r, (("feat", "feat"), ("inside", "inside")))
    assert A.get("inside")[0] == N and A.get("inside")[1] == 1
    for i in range(B):  # exactly +0 behind the counts
        assert not A.get("feat")[i, LEN[i]:].view(np.uint32).any()


@own("rf_cubic_feature_sampling_grad")
def cubic_feature_sampling_grad(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("gf", r["gf"], F32, "in", x.res(12))
    A.add("gv", (B, C, R, R, R), F32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_cubic_feature_sampling_grad_workspace_bytes(B, N, R))
    A.build()
    st = x.lib.rf_cubic_feature_sampling_grad(B, N, C, R, LO, HI, A.ptr("a"), A.ptr("ln"), A.ptr("gf"), A.ptr("gv"), A.ptr(ws),
                                              wsz - 1, None)
    torch.cuda.synchronize()
    assert st == EWORKSPACE and A.still_poison("gv") and A.still_poison(ws)
    x.call(A, "rf_cubic_feature_sampling_grad", B, N, C, R, LO, HI, "a", "ln", "gf", "gv", ws, wsz, None)
    _same(x, A, r, (("gv", "gv"),))
    assert np.isfinite(A.get("gv")).all() and np.abs(A.get("gv")).max() > 0


def _reverse(x, compact):
    r = x.ref(_ref)
    A = x.arena()
    A.add("grid", r["grid"], F32, "in", x.T)
    A.add("pts", (B, M, 3), F32, "out", x.res(4))
    A.add("row", (B, M), I32, "out", x.res(8))
    A.add("cnt", (B,), I32, "out", x.res(12))
    ws, wsz = x.ws(A, x.lib.rf_gridding_reverse_workspace_bytes(B, R))
    A.build()
    st = x.lib.rf_gridding_reverse(B, R, LO, HI, EPS, compact, A.ptr("grid"), A.ptr("pts"), A.ptr("row"), A.ptr("cnt"), A.ptr(ws),
                                   wsz - 1, None)
    torch.cuda.synchronize()
    assert st == EWORKSPACE and all(A.still_poison(k) for k in ("pts", "row", "cnt", ws))
    x.call(A, "rf_gridding_reverse", B, R, LO, HI, EPS, compact, "grid", "pts", "row", "cnt", ws, wsz, None)
    _same(x, A, r, (("pts", f"pts{compact}"), ("row", f"row{compact}"), ("cnt", f"cnt{compact}")))
    cnt = A.get("cnt")
    assert cnt[0] == M and 0 < cnt[1] < M and cnt[2] == 0
    if compact:
        for i in range(B):
            assert not A.get("pts")[i, cnt[i]:].view(np.uint32).any()


@own("rf_gridding_reverse")
def gridding_reverse_in_place(x):
    _reverse(x, 0)


@own("rf_gridding_reverse")
def gridding_reverse_compact(x):
    _reverse(x, 1)


@own("rf_gridding_reverse_grad")
def gridding_reverse_grad(x):
    r = x.ref(_ref)
    for compact in (0, 1):
        A = x.arena()
        A.add("grid", r["grid"], F32, "in", x.T)
        A.add("row", r[f"row{compact}"], I32, "in", x.res(4))
        A.add("gp", r["gp"], F32, "in", x.res(8))
        A.add("gg", (B, R, R, R), F32, "out", x.res(12))
        A.build()
        x.call(A, "rf_gridding_reverse_grad", B, R, LO, HI, "grid", "row", "gp", "gg", None)
        got = A.get("gg")
        assert got.tobytes() == r[f"gg{compact}"].tobytes(), f"{x.cid}: gg differs from the plain call (compact {compact})"
        x.keep(f"gg{compact}", got)
        assert np.isfinite(got).all() and np.abs(got[0]).max() > 0 and not got[2].view(np.uint32).any()


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_grnet_layers(orc, cid, variant, poison):
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
