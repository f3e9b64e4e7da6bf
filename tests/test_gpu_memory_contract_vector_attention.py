"""GPU: the memory contract of include/rfops.h for rf_neighbor_sub, rf_neighbor_sub_grad, rf_neighbor_aggregate and
rf_neighbor_aggregate_grad, straight through the C ABI: `out` of the subtraction, `grad_pos` exactly (b, m, k, c),
`grad_weight` exactly (b, m, k, cw), `out` of the aggregation and `grad_q` exactly (b, m, c), `grad_src` / `grad_value` exactly
(b, n, c), the workspaces exactly what the two _workspace_bytes functions state and poisoned, inputs and count arrays at the residues
the header allows (4 bytes; the workspace 16), ragged counts with 1 and the full size among them over NaN padding and garbage
indices; after the call every byte outside the outputs and the workspace is unchanged, every output slot is written, and the outputs
are the bits of the plain call.  A workspace one byte short is answered with RF_EWORKSPACE and nothing is touched.  The inputs are
integer-valued, so the sums of the two scatters are exact and their bits are promised from call to call.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_point_voxel.py does; `test_memory_contract_vector_attention` runs them."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_vector_attention_host import INT_MAX, INT_MIN, indices, ints

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, M, N, K, C, CW = 3, 65, 257, 17, 12, 4
LEN1, LEN2 = np.array([N, 1, 129], I32), np.array([33, M, 1], I32)
EWORKSPACE = -2


def _ref():
    """Inputs with NaN behind the counts and garbage in idx there, and the plain calls' outputs on them."""
    from rfnet_amd import _raw
    r = dict(q=ints(1, B, M, C), src=ints(2, B, N, C), v=ints(3, B, N, C), pos=ints(4, B, M, K, C), w=ints(5, B, M, K, CW),
             g3=ints(6, B, M, C), g4=ints(7, B, M, K, C))
    r["idx"] = np.stack([indices("hostile", 8 + i, M, K, N) for i in range(B)])
    garbage = np.array([INT_MIN, INT_MAX, -1, N, 5], I32)
    for i in range(B):
        for k in ("src", "v"):
            r[k][i, LEN1[i]:] = np.nan
        for k in ("q", "g3", "pos", "w", "g4"):
            r[k][i, LEN2[i]:] = np.nan
        for k in ("pos", "w", "g4"):
            r[k][i, :, LEN1[i]:] = np.nan
        r["idx"][i, LEN2[i]:] = garbage[np.arange((M - LEN2[i]) * K) % 5].reshape(M - LEN2[i], K)
    t = {k: torch.from_numpy(x).cuda() for k, x in r.items()}
    l1, l2 = torch.from_numpy(LEN1).cuda(), torch.from_numpy(LEN2).cuda()
    r["sub"] = _raw.neighbor_subtraction(t["q"], t["src"], t["idx"], l1, l2)
    r["gq"], r["gs"] = _raw.neighbor_subtraction_grad(t["idx"], t["g4"], N, l1, l2)
    r["out"] = _raw.neighbor_aggregation(t["v"], t["w"], t["idx"], t["pos"], l1, l2)
    r["out0"] = _raw.neighbor_aggregation(t["v"], t["w"], t["idx"], None, l1, l2)
    r["gv"], r["gp"], r["gw"] = _raw.neighbor_aggregation_grad(t["v"], t["w"], t["idx"], t["g3"], t["pos"], l1, l2)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _same(x, A, r, names):
    for k, rk in names:
        got = A.get(k)
        # every slot written (no poison left: the dead slots and padded rows are +0) and the bits of the plain call
        assert got.shape == r[rk].shape and got.tobytes() == r[rk].tobytes(), f"{x.cid}: {k} differs from the plain call"
        assert np.isfinite(got).all() and np.abs(got).max() > 0, f"{x.cid}: {k}"
        x.keep(k, got)


def _zero_behind(got, counts):
    for i in range(B):
        assert not got[i, counts[i]:].view(np.uint32).any()


def _counts(x, A):
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)


@own("rf_neighbor_sub")
def neighbor_sub(x):
    r = x.ref(_ref)
    A = x.arena()
    A.add("q", r["q"], F32, "in", x.T)
    A.add("src", r["src"], F32, "in", x.res(8))
    A.add("idx", r["idx"], I32, "in", x.res(12))
    _counts(x, A)
    A.add("sub", (B, M, K, C), F32, "out", x.res(4))
    A.build()
    x.call(A, "rf_neighbor_sub", B, N, M, K, C, "q", "src", "idx", "l1", "l2", "sub", None)
    _same(x, A, r, (("sub", "sub"),))
    _zero_behind(A.get("sub"), LEN2)


def _sub_grad(x, want_q, want_src):
    r = x.ref(_ref)
    A = x.arena()
    A.add("idx", r["idx"], I32, "in", x.T)
    _counts(x, A)
    A.add("g", r["g4"], F32, "in", x.res(8))
    if want_q:
        A.add("gq", (B, M, C), F32, "out", x.res(4))
    if want_src:
        A.add("gs", (B, N, C), F32, "out", x.res(12))
    ws, wsz = x.ws(A, x.lib.rf_neighbor_sub_grad_workspace_bytes(B, N, M, K)) if want_src else (None, 0)
    A.build()
    gq, gs = ("gq" if want_q else None), ("gs" if want_src else None)
    if want_src:
        st = x.lib.rf_neighbor_sub_grad(B, N, M, K, C, A.ptr("idx"), A.ptr("l1"), A.ptr("l2"), A.ptr("g"), A.ptr(gq) if gq else None,
                                        A.ptr("gs"), A.ptr(ws), wsz - 1, None)
        torch.cuda.synchronize()
        assert st == EWORKSPACE and A.still_poison("gs") and A.still_poison(ws) and (not want_q or A.still_poison("gq"))
    x.call(A, "rf_neighbor_sub_grad", B, N, M, K, C, "idx", "l1", "l2", "g", gq, gs, ws, wsz, None)
    _same(x, A, r, ((("gq", "gq"),) if want_q else ()) + ((("gs", "gs"),) if want_src else ()))
    if want_q:
        _zero_behind(A.get("gq"), LEN2)
    if want_src:
        _zero_behind(A.get("gs"), LEN1)


@own("rf_neighbor_sub_grad")
def neighbor_sub_grad(x):
    _sub_grad(x, True, True)


@own("rf_neighbor_sub_grad")
def neighbor_sub_grad_query_only(x):
    """no sort runs and no workspace is passed"""
    _sub_grad(x, True, False)


@own("rf_neighbor_sub_grad")
def neighbor_sub_grad_source_only(x):
    _sub_grad(x, False, True)


def _aggregate(x, with_pos):
    r = x.ref(_ref)
    A = x.arena()
    A.add("v", r["v"], F32, "in", x.T)
    if with_pos:
        A.add("pos", r["pos"], F32, "in", x.res(12))
    A.add("w", r["w"], F32, "in", x.res(8))
    A.add("idx", r["idx"], I32, "in", x.T)
    _counts(x, A)
    A.add("out", (B, M, C), F32, "out", x.res(4))
    A.build()
    x.call(A, "rf_neighbor_aggregate", B, N, M, K, C, CW, "v", "pos" if with_pos else None, "w", "idx", "l1", "l2", "out", None)
    _same(x, A, r, (("out", "out" if with_pos else "out0"),))
    _zero_behind(A.get("out"), LEN2)


@own("rf_neighbor_aggregate")
def neighbor_aggregate(x):
    _aggregate(x, True)


@own("rf_neighbor_aggregate")
def neighbor_aggregate_without_pos(x):
    _aggregate(x, False)


def _aggregate_grad(x, want):
    """want: the outputs asked for, of gv, gp, gw; the others are passed as NULL"""
    r = x.ref(_ref)
    A = x.arena()
    A.add("v", r["v"], F32, "in", x.res(8))
    A.add("pos", r["pos"], F32, "in", x.T)
    A.add("w", r["w"], F32, "in", x.res(12))
    A.add("idx", r["idx"], I32, "in", x.T)
    _counts(x, A)
    A.add("g", r["g3"], F32, "in", x.res(4))
    shapes = dict(gv=(B, N, C), gp=(B, M, K, C), gw=(B, M, K, CW))
    for j, k in enumerate(want):
        A.add(k, shapes[k], F32, "out", x.res(4 * (j + 1)))
    ws, wsz = x.ws(A, x.lib.rf_neighbor_aggregate_grad_workspace_bytes(B, N, M, K)) if "gv" in want else (None, 0)
    A.build()
    outs = [k if k in want else None for k in ("gv", "gp", "gw")]
    if "gv" in want:
        st = x.lib.rf_neighbor_aggregate_grad(B, N, M, K, C, CW, A.ptr("v"), A.ptr("pos"), A.ptr("w"), A.ptr("idx"), A.ptr("l1"),
                                              A.ptr("l2"), A.ptr("g"), *[A.ptr(k) if k else None for k in outs], A.ptr(ws), wsz - 1, None)
        torch.cuda.synchronize()
        assert st == EWORKSPACE and A.still_poison(ws) and all(A.still_poison(k) for k in want)
    x.call(A, "rf_neighbor_aggregate_grad", B, N, M, K, C, CW, "v", "pos", "w", "idx", "l1", "l2", "g", *outs, ws, wsz, None)
    _same(x, A, r, tuple((k, k) for k in want))
    for k in want:
        _zero_behind(A.get(k), LEN1 if k == "gv" else LEN2)


@own("rf_neighbor_aggregate_grad")
def neighbor_aggregate_grad(x):
    _aggregate_grad(x, ("gv", "gp", "gw"))


@own("rf_neighbor_aggregate_grad")
def neighbor_aggregate_grad_value_only(x):
    _aggregate_grad(x, ("gv",))


@own("rf_neighbor_aggregate_grad")
def neighbor_aggregate_grad_without_value(x):
    """no sort runs and no workspace is passed"""
    _aggregate_grad(x, ("gp", "gw"))


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_vector_attention(orc, cid, variant, poison):
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
