"""GPU: the memory contract of include/rfops.h for rf_voxelize_mean, rf_voxelize_mean_grad, rf_trilinear_devoxelize and
rf_trilinear_devoxelize_grad, straight through the C ABI: `vol` / `grad_vol` exactly (b, c, R, R, R), `cnt` exactly
(b, R, R, R), `feat` / `grad_feat` exactly (b, n, c), `grad_xyz` exactly (b, n, 3), `inside` exactly (b), the workspaces exactly what the
two _workspace_bytes functions state and poisoned, inputs and count arrays at the residues the header allows (4 bytes; the workspace
16), ragged counts with 1 and the full size among them over NaN padding; after the call every byte outside the outputs and the
workspace is unchanged, every output slot is written, and the outputs are the bits of the plain call.  A workspace one byte short is
answered with RF_EWORKSPACE and nothing is touched.  The inputs make the sums of the two scatters exact (integer values, a box
with inv_h = 1, coordinates on multiples of 1/8), so that their bits are promised from call to call.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_grnet_layers.py does; `test_memory_contract_point_voxel` runs them."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_point_voxel_host import family, volume

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, C, R = 3, 257, 9, 17  # 3^3 sub-bricks, the last of them one vertex wide; two channel chunks, the second one channel wide
LO, HI = 0.0, R - 1.0
LEN = np.array([N, 1, 129], I32)
EWORKSPACE = -2


def _ref():
    """Inputs with NaN behind the counts, and the plain calls' outputs on them."""
    from rfnet_amd import _raw
    a = np.stack([np.round(family(k, 50 + i, N, R, LO, HI) * 8) / 8 for i, k in enumerate(("uniform", "seams", "outside"))]).astype(F32)
    f = np.random.RandomState(7).randint(-64, 65, (B, N, C)).astype(F32)  # exact sums: the bits are promised
    for i in range(B):
        a[i, LEN[i]:] = np.nan
        f[i, LEN[i]:] = np.nan
    vol = np.stack([volume(8 + i, C, R) for i in range(B)])
    ta, tf, tv, tl = (torch.from_numpy(t).cuda() for t in (a, f, vol, LEN))
    vox, cnt, inside = _raw.avg_voxelize(ta, tf, R, LO, HI, tl)
    gf = _raw.avg_voxelize_grad(ta, cnt, tv, LO, HI, tl)
    feat, inside2 = _raw.trilinear_devoxelize(ta, tv, LO, HI, tl)
    gv, gx = _raw.trilinear_devoxelize_grad(ta, tv, tf, LO, HI, tl)
    r = dict(a=a, f=f, vol=vol, vox=vox, cnt=cnt, inside=inside, gf=gf, feat=feat, inside2=inside2, gv=gv, gx=gx)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _same(x, A, r, names):
    for k, rk in names:
        got = A.get(k)
        # every slot written (no poison left: the padded slots are +0) and the bits of the plain call
        assert got.shape == r[rk].shape and got.tobytes() == r[rk].tobytes(), f"{x.cid}: {k} differs from the plain call"
        x.keep(k, got)


@own("rf_voxelize_mean")
def voxelize_mean(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("f", r["f"], F32, "in", x.res(8))
    A.add("vox", (B, C, R, R, R), F32, "out", x.res(4))
    A.add("cnt", (B, R, R, R), I32, "out", x.res(8))
    A.add("inside", (B,), I32, "out", x.res(12))
    ws, wsz = x.ws(A, x.lib.rf_voxelize_mean_workspace_bytes(B, N, R))
    A.build()
    st = x.lib.rf_voxelize_mean(B, N, C, R, LO, HI, A.ptr("a"), A.ptr("ln"), A.ptr("f"), A.ptr("vox"), A.ptr("cnt"), A.ptr("inside"),
                                A.ptr(ws), wsz - 1, None)
    torch.cuda.synchronize()
    assert st == EWORKSPACE and all(A.still_poison(k) for k in ("vox", "cnt", "inside", ws))
    x.call(A, "rf_voxelize_mean", B, N, C, R, LO, HI, "a", "ln", "f", "vox", "cnt", "inside", ws, wsz, None)
    _same(x, A, r, (("vox", "vox"), ("cnt", "cnt"), ("inside", "inside")))
    assert A.get("inside")[0] == N and A.get("inside")[1] == 1 and A.get("cnt").reshape(B, -1).sum(1).tolist() == A.get("inside").tolist()
    assert np.isfinite(A.get("vox")).all() and np.abs(A.get("vox")).max() > 0


@own("rf_voxelize_mean_grad")
def voxelize_mean_grad(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("cnt", r["cnt"], I32, "in", x.res(4))
    A.add("gv", r["vol"], F32, "in", x.res(12))
    A.add("gf", (B, N, C), F32, "out", x.res(8))
    A.build()
    x.call(A, "rf_voxelize_mean_grad", B, N, C, R, LO, HI, "a", "ln", "cnt", "gv", "gf", None)
    _same(x, A, r, (("gf", "gf"),))
    for i in range(B):  # exactly +0 behind the counts
        assert not A.get("gf")[i, LEN[i]:].view(np.uint32).any()
    assert np.abs(A.get("gf")).max() > 0


@own("rf_trilinear_devoxelize")
def trilinear_devoxelize(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("vol", r["vol"], F32, "in", x.res(8))
    A.add("feat", (B, N, C), F32, "out", x.res(4))
    A.add("inside", (B,), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_trilinear_devoxelize", B, N, C, R, LO, HI, "a", "ln", "vol", "feat", "inside", None)
    _same(x, A, r, (("feat", "feat"), ("inside", "inside2")))
    assert A.get("inside")[0] == N and A.get("inside")[1] == 1
    for i in range(B):
        assert not A.get("feat")[i, LEN[i]:].view(np.uint32).any()


def _devox_grad(x, want_xyz):
    r = x.ref(_ref)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("ln", LEN, I32, "in", x.L)
    A.add("vol", r["vol"], F32, "in", x.res(8))
    A.add("gf", r["f"], F32, "in", x.res(12))
    A.add("gv", (B, C, R, R, R), F32, "out", x.res(4))
    if want_xyz:
        A.add("gx", (B, N, 3), F32, "out", x.res(8))
    gx = "gx" if want_xyz else None
    ws, wsz = x.ws(A, x.lib.rf_trilinear_devoxelize_grad_workspace_bytes(B, N, R))
    A.build()
    st = x.lib.rf_trilinear_devoxelize_grad(B, N, C, R, LO, HI, A.ptr("a"), A.ptr("ln"), A.ptr("vol"), A.ptr("gf"), A.ptr("gv"),
                                            A.ptr(gx) if gx else None, A.ptr(ws), wsz - 1, None)
    torch.cuda.synchronize()
    assert st == EWORKSPACE and A.still_poison("gv") and A.still_poison(ws) and (not want_xyz or A.still_poison("gx"))
    x.call(A, "rf_trilinear_devoxelize_grad", B, N, C, R, LO, HI, "a", "ln", "vol", "gf", "gv", gx, ws, wsz, None)
    _same(x, A, r, (("gv", "gv"),) + ((("gx", "gx"),) if want_xyz else ()))
    assert np.isfinite(A.get("gv")).all() and np.abs(A.get("gv")).max() > 0
    if want_xyz:
        for i in range(B):
            assert not A.get("gx")[i, LEN[i]:].view(np.uint32).any()


@own("rf_trilinear_devoxelize_grad")
def trilinear_devoxelize_grad(x):
    _devox_grad(x, True)


@own("rf_trilinear_devoxelize_grad")
def trilinear_devoxelize_grad_without_xyz(x):
    _devox_grad(x, False)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_point_voxel(orc, cid, variant, poison):
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
