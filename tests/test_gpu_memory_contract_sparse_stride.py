"""GPU: the memory contract of include/rfops.h for rf_sparse_stride_map, rf_sparse_conv_strided and
rf_sparse_conv_strided_grad_weight, straight through the C ABI: the outputs exactly (b, n_coarse, 3), (b), (b), (b, n_coarse, 8)
and (b, n); (b, rows, cout); (8, cin, cout); the workspace exactly what the size query says; every tensor and count array at the
residues the header allows (4 bytes; 16 for the workspace); ragged counts with 0, 1 and the full size among them, NaN rows
behind the counts, hostile child / up: garbage behind the counts, entries outside [0, M) in the absent slots, claims in up that
child does not confirm.  After the call every byte outside the outputs and the workspace is unchanged, every output element is
written (the poison is gone: the int outputs equal the restatement of tests/sparse_stride_ref.py as bytes, the fp32 outputs bit
for bit with zeros of either sign equal), and the four runs of a case agree bit for bit -- the aligned variant loads rows of 12
and 8 channels as 16-byte vectors, the natural one as floats.  Two cases repeat the map and the mode "up" at n = n_coarse =
16384, the top of the range, where the guards stand directly behind the last row of child, up and the fine rows.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, exactly as tests/test_gpu_memory_contract_sparse_conv.py does; `test_memory_contract_sparse_stride` runs them."""
import functools

import numpy as np
import pytest

import sparse_sizes as Z
import sparse_stride_ref as R
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
MODES = {R.DOWN: ("fine_in", "out_down"), R.UP: ("coarse_in", "out_up"), R.DOWN_GRAD_INPUT: ("coarse_g", "out_dgi"),
         R.UP_GRAD_INPUT: ("fine_g", "out_ugi")}  # mode -> (the source, the reference result) in _inputs' dict


def _inputs(nc, ragged):
    rng = np.random.RandomState(23 + nc)
    coords = rng.randint(-5, 5, (B, N, 3)).astype(I32)
    coords[0, 1] = [40000, 0, 0]
    coords[0, 2] = [32767, -32768, 32767]
    coords[0, 3] = [32767, -32768, 32766]
    coords[2, 6] = coords[2, 7]
    cnt = COUNT if ragged else None
    m = R.map_ref(coords, cnt, nc)
    r = dict(coords=coords, m=m, child=m["child"].copy(), up=m["up"].copy())
    r["fine_in"], r["fine_g"] = rng.randn(B, N, CIN).astype(F32), rng.randn(B, N, COUT).astype(F32)
    r["coarse_in"], r["coarse_g"] = rng.randn(B, nc, CIN).astype(F32), rng.randn(B, nc, COUT).astype(F32)
    r["weight"] = rng.randn(8, CIN, COUT).astype(F32)
    for s in range(B):  # what the convolutions must ignore
        M, Mc = (int(COUNT[s]) if ragged else N), int(m["count"][s])
        r["fine_in"][s, M:], r["fine_g"][s, M:] = np.nan, np.nan
        r["coarse_in"][s, Mc:], r["coarse_g"][s, Mc:] = np.nan, np.nan
        r["child"][s, Mc:] = rng.randint(-3, N + 3, (nc - Mc, 8))
        hole = r["child"][s, :Mc] == -1
        r["child"][s, :Mc][hole] = rng.choice([-1, -9, M, N, 1 << 30], int(hole.sum()))
        r["up"][s, M:] = rng.randint(-3, 8 * nc + 9, N - M)
        dead = r["up"][s, :M] == -1
        r["up"][s, :M][dead] = rng.choice([-1, -9, 8 * Mc, 8 * nc + 5, 1 << 30, 0, 9], int(dead.sum()))
    a = (m["child"], m["up"], N, cnt, m["count"])
    for mode, (src, name) in MODES.items():
        r[name] = R.conv_ref(mode, r[src], r["weight"], *a)
    r["gw_down"] = R.grad_weight_ref(R.DOWN, r["fine_in"], r["coarse_g"], m["child"], cnt, m["count"])
    r["gw_up"] = R.grad_weight_ref(R.UP, r["fine_g"], r["coarse_in"], m["child"], cnt, m["count"])
    return r


def _same(x, name, got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype and R.same_bits(got, exp), f"{x.cid}: {name} differs from the restatement"
    x.keep(name, np.where(got == 0, F32(0), got))  # (across the runs: bit for bit, zeros of either sign equal)


def _map(x, nc, ragged):
    r = x.ref(lambda: _inputs(nc, ragged))
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("coords_out", (B, nc, 3), I32, "out", x.res(12))
    A.add("count_out", (B,), I32, "out", x.L)
    A.add("total_out", (B,), I32, "out", x.res(8))
    A.add("child", (B, nc, 8), I32, "out", x.T)
    A.add("up", (B, N), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_stride_map", B, N, nc, "coords", "count" if ragged else None, "coords_out", "count_out", "total_out", "child",
           "up", None)
    for name, key in (("coords_out", "coords"), ("count_out", "count"), ("total_out", "total"), ("child", "child"), ("up", "up")):
        got, exp = A.get(name), r["m"][key]
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)


@own("rf_sparse_stride_map")
def sparse_stride_map_ragged(x):
    _map(x, N, True)


@own("rf_sparse_stride_map")
def sparse_stride_map_dense_truncating(x):
    _map(x, 40, False)


def _conv(x, mode, nc, ragged):
    r = x.ref(lambda: _inputs(nc, ragged))
    A = x.arena()
    src, name = MODES[mode]
    cin, cout = (CIN, COUT) if mode in (R.DOWN, R.UP) else (COUT, CIN)
    rows_out = nc if mode in (R.DOWN, R.UP_GRAD_INPUT) else N
    A.add("src", r[src], F32, "in", x.T)
    A.add("weight", r["weight"], F32, "in", x.res(8))
    A.add("child", r["child"], I32, "in", x.res(12))
    A.add("up", r["up"], I32, "in", x.T)
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("count_coarse", r["m"]["count"], I32, "in", x.L)
    A.add("out", (B, rows_out, cout), F32, "out", x.T)
    A.build()
    x.call(A, "rf_sparse_conv_strided", B, N, nc, cin, cout, mode, "src", "weight", "child", "up", "count" if ragged else None,
           "count_coarse", "out", None)
    _same(x, "out", A.get("out"), r[name])


@own("rf_sparse_conv_strided")
def sparse_conv_strided_down_ragged(x):
    _conv(x, R.DOWN, N, True)


@own("rf_sparse_conv_strided")
def sparse_conv_strided_up_ragged(x):
    _conv(x, R.UP, N, True)


@own("rf_sparse_conv_strided")
def sparse_conv_strided_down_grad_input_ragged(x):
    _conv(x, R.DOWN_GRAD_INPUT, N, True)


@own("rf_sparse_conv_strided")
def sparse_conv_strided_up_grad_input_ragged(x):
    _conv(x, R.UP_GRAD_INPUT, N, True)


@own("rf_sparse_conv_strided")
def sparse_conv_strided_up_dense_truncating(x):
    _conv(x, R.UP, 40, False)


def _grad_weight(x, mode, nc, ragged):
    r = x.ref(lambda: _inputs(nc, ragged))
    A = x.arena()
    A.add("fine", r["fine_in"] if mode == R.DOWN else r["fine_g"], F32, "in", x.T)
    A.add("coarse", r["coarse_g"] if mode == R.DOWN else r["coarse_in"], F32, "in", x.res(12))
    A.add("child", r["child"], I32, "in", x.res(8))
    if ragged:
        A.add("count", COUNT, I32, "in", x.L)
    A.add("count_coarse", r["m"]["count"], I32, "in", x.L)
    A.add("gw", (8, CIN, COUT), F32, "out", x.T)
    need = x.lib.rf_sparse_conv_strided_grad_weight_workspace_bytes(B, CIN, COUT)
    assert need >= B * 8 * CIN * COUT * 8
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_sparse_conv_strided_grad_weight", B, N, nc, CIN, COUT, mode, "fine", "coarse", "child", "count" if ragged else None,
           "count_coarse", "gw", ws, wsz, None)
    _same(x, "gw", A.get("gw"), r["gw_down"] if mode == R.DOWN else r["gw_up"])


@own("rf_sparse_conv_strided_grad_weight")
def sparse_conv_strided_grad_weight_down_ragged(x):
    _grad_weight(x, R.DOWN, N, True)


@own("rf_sparse_conv_strided_grad_weight")
def sparse_conv_strided_grad_weight_up_dense_truncating(x):
    _grad_weight(x, R.UP, 40, False)


# ---- the top of the range: n = n_coarse = 16384, every row alone in its coarse cell, so child, up and the fine rows of "up" are
# written up to their last element: a store past them is what a wrong row number writes ----
NB, CB = 16384, np.array([16384, 8191, 4096, 77], I32)


@functools.lru_cache(maxsize=1)
def _inputs_at_size():
    """shared by the two cases below (never written to: the arena copies)"""
    rng = np.random.RandomState(31)
    coords = Z.family("spread", NB, 31, b=B)
    m = R.map_ref(coords, CB, NB)
    assert np.array_equal(m["count"], CB)
    r = dict(coords=coords, m=m, child=m["child"].copy(), up=m["up"].copy())
    r["coarse_in"], r["weight"] = rng.randn(B, NB, 3).astype(F32), rng.randn(8, 3, 5).astype(F32)
    for s in range(B):  # what the convolution must ignore
        M = int(CB[s])
        r["coarse_in"][s, M:] = np.nan
        r["child"][s, M:] = rng.randint(-3, NB + 3, (NB - M, 8))
        hole = r["child"][s, :M] == -1
        r["child"][s, :M][hole] = rng.choice([-1, -9, M, NB, 1 << 30], int(hole.sum()))
        r["up"][s, M:] = rng.randint(-3, 8 * NB + 9, NB - M)
    r["out_up"] = R.conv_ref(R.UP, r["coarse_in"], r["weight"], m["child"], m["up"], NB, CB, m["count"])
    return r


@own("rf_sparse_stride_map")
def sparse_stride_map_16384_rows(x):
    r = x.ref(_inputs_at_size)
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    A.add("count", CB, I32, "in", x.L)
    A.add("coords_out", (B, NB, 3), I32, "out", x.res(12))
    A.add("count_out", (B,), I32, "out", x.L)
    A.add("total_out", (B,), I32, "out", x.res(8))
    A.add("child", (B, NB, 8), I32, "out", x.T)
    A.add("up", (B, NB), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_stride_map", B, NB, NB, "coords", "count", "coords_out", "count_out", "total_out", "child", "up", None)
    for name, key in (("coords_out", "coords"), ("count_out", "count"), ("total_out", "total"), ("child", "child"), ("up", "up")):
        got, exp = A.get(name), r["m"][key]
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)
    assert (A.get("child")[0, NB - 1] >= 0).sum() == 1 and A.get("up")[0].max() >= 8 * (NB - 1)  # the last coarse row is in use


@own("rf_sparse_conv_strided")
def sparse_conv_strided_up_16384_rows(x):
    r = x.ref(_inputs_at_size)
    A = x.arena()
    A.add("src", r["coarse_in"], F32, "in", x.T)
    A.add("weight", r["weight"], F32, "in", x.res(8))
    A.add("child", r["child"], I32, "in", x.res(12))
    A.add("up", r["up"], I32, "in", x.T)
    A.add("count", CB, I32, "in", x.L)
    A.add("count_coarse", r["m"]["count"], I32, "in", x.L)
    A.add("out", (B, NB, 5), F32, "out", x.T)
    A.build()
    x.call(A, "rf_sparse_conv_strided", B, NB, NB, 3, 5, R.UP, "src", "weight", "child", "up", "count", "count_coarse", "out", None)
    _same(x, "out", A.get("out"), r["out_up"])


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_sparse_stride(orc, cid, variant, poison):
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
