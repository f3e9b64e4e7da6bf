"""GPU: the memory contract of include/rfops.h for the network's ragged entries: the pooled maximum and
the merge layer with per-sample counts, straight through the C ABI.

The cases use the machinery of tests/test_gpu_memory_contract.py (guarded arena, the four variant x poison runs, checks
(a)-(d) of its docstring) and register themselves in its CASES table when this module is imported.  That table is what
tests/test_memory_contract_host.py holds against _lib.SIGNATURES: pytest imports every test module while it collects, so
a run of the suite (`pytest tests`, with or without -m) sees these cases there; a run of the host file on its own does
not import this module and reports the four entries below as uncovered.  The parametrised test of the other module was
built before this module was imported and does not run these cases: `test_memory_contract_model` here does."""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as T
from test_gpu_memory_contract import B, CF, F32, I32, M, N, _amax, _feat, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


LEN_X = np.array([N, 1, 257], I32)      # rows pooled per sample (N = 301: two strips of 256; one row; one row into the second)
LEN_RAW = np.array([N, 1, 37], I32)
LEN_NEW = np.array([M, 100, 1], I32)


def _feat_len(seed):
    xv = _feat(seed)
    for i, ln in enumerate(LEN_X):
        xv[i, ln:] = np.nan if i % 2 else np.inf  # read, either would show in the maximum
    return dict(x=xv, out=np.stack([xv[i, :ln].max(0) for i, ln in enumerate(LEN_X)]),
                idx=np.stack([xv[i, :ln].argmax(0) for i, ln in enumerate(LEN_X)]).astype(I32))


@own("rf_maxpool_points_lengths")
def maxpool_points_lengths(x):
    r = x.ref(lambda: _feat_len(98))
    A = x.arena()
    A.add("x", r["x"], F32, "in", x.T16)
    A.add("len", LEN_X, I32, "in", x.L)
    A.add("out", (B, CF), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_maxpool_points_lengths_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_maxpool_points_lengths", B, N, CF, "x", "len", "out", ws, wsz, None)
    x.exact("out", A.get("out"), r["out"])


@own("rf_maxpool_points_idx_lengths")
def maxpool_points_idx_lengths(x):
    r = x.ref(lambda: _feat_len(98))
    A = x.arena()
    A.add("x", r["x"], F32, "in", x.T16)
    A.add("len", LEN_X, I32, "in", x.L)
    A.add("out", (B, CF), F32, "out", x.T)
    A.add("idx", (B, CF), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_maxpool_points_idx_lengths_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_maxpool_points_idx_lengths", B, N, CF, "x", "len", "out", "idx", ws, wsz, None)
    x.exact("out", A.get("out"), r["out"])
    x.exact("idx", A.get("idx"), r["idx"])


def _merge_len_ref(x):
    """The merge layer per sample on the unpadded slices, in float64; zeros in every padded row.  Padded raw rows hold copies
    of the sample's new points (distance 0: read, they win every search), padded new rows and their upstream gradient NaN."""
    rng = np.random.RandomState(19)
    raw, new = (rng.rand(B, N, 3) - 0.5).astype(F32), (rng.rand(B, M, 3) - 0.5).astype(F32)
    dec, go = np.array([0.07], F32), rng.randn(B, M, 3).astype(F32)
    i2, out, gnew = np.zeros((B, M), I32), np.zeros((B, M, 3)), np.zeros((B, M, 3))
    graw, gdec = np.zeros((B, N, 3)), np.zeros(B)
    for i, (lr, ln) in enumerate(zip(LEN_RAW, LEN_NEW)):
        raw[i, lr:] = new[i, np.arange(N - lr) % M]
        ri, ni = raw[i:i + 1, :lr].copy(), new[i:i + 1, :ln].copy()
        i2[i, :ln] = x.orc.nn_distance(ri, ni)[3][0]
        traw, tnew = torch.from_numpy(ri[0]).double().requires_grad_(True), torch.from_numpy(ni[0]).double().requires_grad_(True)
        tdec = torch.from_numpy(dec).double().requires_grad_(True)
        diff = traw[torch.from_numpy(i2[i, :ln]).long()] - tnew
        o = tnew + torch.exp(-(diff * diff).sum(-1, keepdim=True) / (1e-8 + tdec ** 2)) * diff
        (o * torch.from_numpy(go[i, :ln]).double()).sum().backward()
        out[i, :ln], gnew[i, :ln], graw[i, :lr], gdec[i] = o.detach().numpy(), tnew.grad.numpy(), traw.grad.numpy(), tdec.grad.item()
        new[i, ln:], go[i, ln:] = np.nan, np.nan
    return dict(raw=raw, new=new, dec=dec, i2=i2, go=go, out=out, gnew=gnew, graw=graw, gdec=gdec)


@own("rf_merge_layer_lengths")
def merge_layer_lengths(x):
    r = x.ref(lambda: _merge_len_ref(x))
    A = x.arena()
    A.add("raw", r["raw"], F32, "in", x.T)
    A.add("new", r["new"], F32, "in", x.T)
    A.add("lr", LEN_RAW, I32, "in", x.L)
    A.add("ln", LEN_NEW, I32, "in", x.L)
    A.add("dec", r["dec"], F32, "in", x.L)
    A.add("out", (B, M, 3), F32, "out", x.T)
    A.add("i2", (B, M), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_merge_layer_lengths_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_merge_layer_lengths", B, N, M, "raw", "new", "lr", "ln", "dec", "out", "i2", ws, wsz, None)
    x.exact("i2", A.get("i2"), r["i2"])
    got = A.get("out")
    for i, ln in enumerate(LEN_NEW):
        assert not got[i, ln:].any() and not np.signbit(got[i, ln:]).any(), i  # padded new rows: +0.0
    x.close("out", got, r["out"], 1e-5, 1e-6)  # rf_merge_layer's bar


@own("rf_merge_layer_grad_lengths")
def merge_layer_grad_lengths(x):
    r = x.ref(lambda: _merge_len_ref(x))
    A = x.arena()
    for k, dt in (("raw", F32), ("new", F32), ("i2", I32), ("go", F32)):
        A.add(k, r[k], dt, "in", x.T)
    A.add("lr", LEN_RAW, I32, "in", x.L)
    A.add("ln", LEN_NEW, I32, "in", x.L)
    A.add("dec", r["dec"], F32, "in", x.L)
    A.add("gnew", (B, M, 3), F32, "out", x.res(4))
    A.add("gdec", (B,), F32, "out", x.res(8))
    A.add("graw", (B, N, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_merge_layer_grad_lengths", B, N, M, "raw", "new", "lr", "ln", "dec", "i2", "go", "gnew", "gdec", "graw", None)
    gnew, graw = A.get("gnew"), A.get("graw")
    for i, (lr, ln) in enumerate(zip(LEN_RAW, LEN_NEW)):
        assert not gnew[i, ln:].any() and not graw[i, lr:].any(), i  # exactly zero behind the counts
    x.close("gnew", gnew, r["gnew"], 1e-4, 1e-5 * _amax(r["gnew"]))  # rf_merge_layer_grad's bars
    x.close("graw", graw, r["graw"], 1e-4, 1e-5 * _amax(r["graw"]))
    x.close("gdec", A.get("gdec"), r["gdec"], 1e-3, 1e-4 * _amax(r["gdec"]) + 1e-6)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_model(orc, cid, variant, poison):
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
