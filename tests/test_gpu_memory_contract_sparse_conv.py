"""GPU: the memory contract of include/rfops.h for rf_sparse_conv_map, rf_sparse_conv and rf_sparse_conv_grad_weight, straight
through the C ABI: the outputs exactly (b, n, K), (b, n, cout) and (K, cin, cout), the workspace exactly what the size query
says, every tensor and count array at the residues the header allows (4 bytes; 16 for the workspace), ragged counts with 0, 1
and the full size among them, NaN rows and garbage map entries behind them.  After the call every byte outside the outputs and
the workspace is unchanged, every output element is written (the poison is gone: the map equals the restatement of
tests/sparse_conv_ref.py as bytes, the fp32 outputs bit for bit with zeros of either sign equal), and the four runs of a case
agree bit for bit -- the aligned variant loads rows of 12 and 8 channels as 16-byte vectors, the natural one as floats.  Two
cases repeat the map and the forward at n = 16384, the top of the range, where the guards stand directly behind row 16383.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_grid_pool.py does; `test_memory_contract_sparse_conv` runs them."""
import functools

import numpy as np
import pytest

import sparse_conv_ref as R
import sparse_sizes as Z
import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N, CIN, COUT = 4, 331, 12, 8
COUNT = np.array([N, 0, 77, 1], I32)


def _inputs(ks, dilation, ragged):
    rng = np.random.RandomState(17 + ks)
    coords = rng.randint(-4, 4, (B, N, 3)).astype(I32)
    coords[0, 1] = [40000, 0, 0]
    coords[0, 2] = [32767, -32768, 32767]
    coords[0, 3] = [32767, -32768, 32766]
    coords[2, 6] = coords[2, 7]
    cnt = COUNT if ragged else None
    K = ks ** 3
    r = dict(coords=coords, nbr=R.map_ref(coords, cnt, ks, dilation))
    r["feat"], r["gout"] = rng.randn(B, N, CIN).astype(F32), rng.randn(B, N, COUT).astype(F32)
    r["weight"] = rng.randn(K, CIN, COUT).astype(F32)
    r["hostile"] = r["nbr"].copy()
    for s in range(B):  # what the convolution must ignore
        M = int(COUNT[s]) if ragged else N
        r["feat"][s, M:], r["gout"][s, M:] = np.nan, np.nan
        r["hostile"][s, M:] = rng.randint(-3, N + 3, (N - M, K))
        hole = r["hostile"][s, :M] == -1
        r["hostile"][s, :M][hole] = rng.choice([-1, -9, M, N, 1 << 30], int(hole.sum()))
    r["out"] = R.conv_ref(r["feat"], r["weight"], r["nbr"], cnt)
    r["gfeat"] = R.grad_input_ref(r["gout"], r["weight"], r["nbr"], cnt)
    r["gweight"] = R.grad_weight_ref(r["feat"], r["gout"], r["nbr"], cnt)
    return r


def _same(x, name, got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype and R.same_bits(got, exp), f"{x.cid}: {name} differs from the restatement"
    x.keep(name, np.where(got == 0, F32(0), got))  # (across the runs: bit for bit, zeros of either sign equal)


def _map(x, ks, dilation, ragged):
    r = x.ref(lambda: _inputs(ks, dilation, ragged))
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("nbr", (B, N, ks ** 3), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_conv_map", B, N, ks, dilation, "coords", "count" if ragged else None, "nbr", None)
    got = A.get("nbr")
    assert got.shape == r["nbr"].shape and got.tobytes() == r["nbr"].tobytes(), f"{x.cid}: nbr differs from the restatement"
    x.keep("nbr", got)


@own("rf_sparse_conv_map")
def sparse_conv_map_ragged(x):
    _map(x, 3, 1, True)


@own("rf_sparse_conv_map")
def sparse_conv_map_dense_5_dilated(x):
    _map(x, 5, 2, False)


def _conv(x, mode, ks, ragged):
    r = x.ref(lambda: _inputs(ks, 1, ragged))
    A = x.arena()
    cin, cout = (CIN, COUT) if mode == 0 else (COUT, CIN)
    A.add("feat", r["feat"] if mode == 0 else r["gout"], F32, "in", x.T)
    A.add("weight", r["weight"], F32, "in", x.res(8))
    A.add("nbr", r["hostile"], I32, "in", x.res(12))
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("out", (B, N, cout), F32, "out", x.T)
    A.build()
    x.call(A, "rf_sparse_conv", B, N, ks ** 3, cin, cout, mode, "feat", "weight", "nbr", "count" if ragged else None, "out", None)
    _same(x, "out", A.get("out"), r["out"] if mode == 0 else r["gfeat"])


@own("rf_sparse_conv")
def sparse_conv_forward_ragged(x):
    _conv(x, 0, 3, True)


@own("rf_sparse_conv")
def sparse_conv_grad_input_ragged(x):
    _conv(x, 1, 3, True)


@own("rf_sparse_conv")
def sparse_conv_forward_dense_5(x):
    _conv(x, 0, 5, False)


def _grad_weight(x, ragged):
    r = x.ref(lambda: _inputs(3, 1, ragged))
    A = x.arena()
    A.add("feat", r["feat"], F32, "in", x.T)
    A.add("gout", r["gout"], F32, "in", x.res(12))
    A.add("nbr", r["hostile"], I32, "in", x.res(8))
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("gw", (27, CIN, COUT), F32, "out", x.T)
    need = x.lib.rf_sparse_conv_grad_weight_workspace_bytes(B, 27, CIN, COUT)
    assert need >= B * 27 * CIN * COUT * 8
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_sparse_conv_grad_weight", B, N, 27, CIN, COUT, "feat", "gout", "nbr", "count" if ragged else None, "gw", ws, wsz,
           None)
    _same(x, "gw", A.get("gw"), r["gweight"])


@own("rf_sparse_conv_grad_weight")
def sparse_conv_grad_weight_ragged(x):
    _grad_weight(x, True)


@own("rf_sparse_conv_grad_weight")
def sparse_conv_grad_weight_dense(x):
    _grad_weight(x, False)


# ---- the top of the range: n = 16384, where a store past nbr or past the last rows of out is what a wrong row number writes ----
NB, CB = 16384, np.array([16384, 8191, 4096, 77], I32)


@functools.lru_cache(maxsize=1)
def _inputs_at_size():
    """shared by the two cases below (never written to: the arena copies)"""
    rng = np.random.RandomState(29)
    coords = Z.family("lattice", NB, 29, b=B)
    r = dict(coords=coords, nbr=R.map_ref(coords, CB, 3, 1))
    r["feat"], r["weight"] = rng.randn(B, NB, 3).astype(F32), rng.randn(27, 3, 5).astype(F32)
    r["hostile"] = r["nbr"].copy()
    for s in range(B):  # what the convolution must ignore
        M = int(CB[s])
        r["feat"][s, M:] = np.nan
        r["hostile"][s, M:] = rng.randint(-3, NB + 3, (NB - M, 27))
        hole = r["hostile"][s, :M] == -1
        r["hostile"][s, :M][hole] = rng.choice([-1, -9, M, NB, 1 << 30], int(hole.sum()))
    r["out"] = R.conv_ref(r["feat"], r["weight"], r["nbr"], CB)
    return r


@own("rf_sparse_conv_map")
def sparse_conv_map_16384_rows(x):
    r = x.ref(_inputs_at_size)
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    A.add("count", CB, I32, "in", x.L)
    A.add("nbr", (B, NB, 27), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_conv_map", B, NB, 3, 1, "coords", "count", "nbr", None)
    got = A.get("nbr")
    assert got.shape == r["nbr"].shape and got.tobytes() == r["nbr"].tobytes(), f"{x.cid}: nbr differs from the restatement"
    assert got[0].max() == NB - 1 and (got[0, NB - 1] >= 0).any()  # the last row is named and has neighbours
    x.keep("nbr", got)


@own("rf_sparse_conv")
def sparse_conv_forward_16384_rows(x):
    r = x.ref(_inputs_at_size)
    A = x.arena()
    A.add("feat", r["feat"], F32, "in", x.T)
    A.add("weight", r["weight"], F32, "in", x.res(8))
    A.add("nbr", r["hostile"], I32, "in", x.res(12))
    A.add("count", CB, I32, "in", x.L)
    A.add("out", (B, NB, 5), F32, "out", x.T)
    A.build()
    x.call(A, "rf_sparse_conv", B, NB, 27, 3, 5, 0, "feat", "weight", "nbr", "count", "out", None)
    _same(x, "out", A.get("out"), r["out"])


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_sparse_conv(orc, cid, variant, poison):
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
