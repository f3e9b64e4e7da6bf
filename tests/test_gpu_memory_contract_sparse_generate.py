"""GPU: the memory contract of include/rfops.h for rf_sparse_generate_map, rf_sparse_prune_map, rf_sparse_lookup and
rf_sparse_take_rows, straight through the C ABI: the outputs exactly (b, n_fine, 3), (b), (b), (b, n_coarse, 8) and (b, n_fine);
(b, n_out, 3), (b), (b), (b, n_out) and (b, n); (b, n); (b, n_dst, c); every tensor and count array at the residues the header
allows (4 bytes; keep at an odd address); ragged counts with 0, 1 and the full size among them; behind the counts garbage
coordinates, selected rows of keep and hostile indices, which are never read; hostile indices in front of the counts, which read
nothing.  After the call every byte outside the outputs is unchanged and every output element is written: the int outputs equal
the restatement of tests/sparse_generate_ref.py as bytes under both poisons (0xFF is the -1 the maps are padded with, 0x5A is not),
the moved rows equal it as bytes, and the four runs of a case agree bit for bit -- the aligned variant moves rows of 12 channels
as 16-byte vectors, the natural one as floats.  Three cases stand at the top of the range, 16384 rows, where the guards are
directly behind the last row of every output and the sort fills its LDS.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module is
imported, as tests/test_gpu_memory_contract_sparse_stride.py does; `test_memory_contract_sparse_generate` runs them."""
import functools

import numpy as np
import pytest

import sparse_generate_ref as G
import sparse_sizes as Z
import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, U8, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, N = 4, 331
COUNT = np.array([N, 0, 77, 1], I32)
JUNK = 0x7F7F7F7F  # coordinates behind a count: far out of range, never read


def _cells(seed, n=N):
    rng = np.random.RandomState(seed)
    c = rng.randint(-5, 5, (B, n, 3)).astype(I32)
    c[0, 1], c[0, 2], c[0, 3], c[0, 4] = [40000, 0, 0], [16383, -16384, 16383], [16384, 0, 0], [-32768, 32767, 0]
    c[2, 6] = c[2, 7]
    return c


def _behind(a, count, value):
    """a copy of a (b, n, ...) with `value` in the rows behind the counts"""
    a = a.copy()
    if count is not None:
        for s, M in enumerate(count):
            a[s, int(M):] = value
    return a


def _ints(x, A, names, want):
    for name, key in names:
        got, exp = A.get(name), want[key]
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"{x.cid}: {name} differs from the restatement"
        x.keep(name, got)


# ---- rf_sparse_generate_map ------------------------------------------------------------------------------------------------------
def _generate(x, coords, count, nf):
    b, nc = coords.shape[:2]
    r = x.ref(lambda: dict(coords=_behind(coords, count, JUNK), m=G.generate_ref(coords, count, nf)))
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    if count is not None:
        A.add("count", count, I32, "in", x.L)
    A.add("coords_out", (b, nf, 3), I32, "out", x.res(12))
    A.add("count_out", (b,), I32, "out", x.L)
    A.add("total_out", (b,), I32, "out", x.res(8))
    A.add("child", (b, nc, 8), I32, "out", x.T)
    A.add("up", (b, nf), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_generate_map", b, nc, nf, "coords", "count" if count is not None else None, "coords_out", "count_out",
           "total_out", "child", "up", None)
    _ints(x, A, (("coords_out", "coords"), ("count_out", "count"), ("total_out", "total"), ("child", "child"), ("up", "up")), r["m"])
    return A, r["m"]


@own("rf_sparse_generate_map")
def sparse_generate_map_ragged_capped(x):
    _, m = _generate(x, _cells(3), COUNT, 1003)
    assert m["total"][0] > m["count"][0] == 1000 and m["count"][1] == 0 and m["count"][3] == 8


@own("rf_sparse_generate_map")
def sparse_generate_map_dense_all_children(x):
    _, m = _generate(x, _cells(4), None, 8 * N)
    assert (m["total"] == m["count"]).all() and m["count"].min() > 800


@functools.lru_cache(maxsize=1)
def _lattice():
    return Z.family("lattice", 16384, 41, b=B)  # 16384 distinct cells per sample: every row a parent


@own("rf_sparse_generate_map")
def sparse_generate_map_16384_rows(x):
    A, m = _generate(x, _lattice(), np.array([16384, 8191, 2048, 77], I32), 16384)
    assert m["count"].tolist() == [16384, 16384, 16384, 616] and m["total"][0] == 8 * 16384
    assert A.get("up")[0, 16383] == 8 * 2047 + 7 and A.get("child")[0, 2047, 7] == 16383  # the last fine row is in use


# ---- rf_sparse_prune_map ---------------------------------------------------------------------------------------------------------
def _prune(x, coords, keep, count, no):
    b, n = coords.shape[:2]
    r = x.ref(lambda: dict(coords=_behind(coords, count, JUNK), keep=_behind(keep, count, 9), m=G.prune_ref(coords, keep, count, no)))
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    A.add("keep", r["keep"], U8, "in", x.res(1))  # no alignment requirement
    if count is not None:
        A.add("count", count, I32, "in", x.L)
    A.add("coords_out", (b, no, 3), I32, "out", x.res(8))
    A.add("count_out", (b,), I32, "out", x.L)
    A.add("total_out", (b,), I32, "out", x.res(12))
    A.add("src", (b, no), I32, "out", x.T)
    A.add("dst", (b, n), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_prune_map", b, n, no, "coords", "keep", "count" if count is not None else None, "coords_out", "count_out",
           "total_out", "src", "dst", None)
    _ints(x, A, (("coords_out", "coords"), ("count_out", "count"), ("total_out", "total"), ("src", "src"), ("dst", "dst")), r["m"])
    return r["m"]


def _keep(seed, n):
    k = np.random.RandomState(seed).choice(np.array([0, 0, 1, 255], U8), (B, n))
    k[3] = 1
    return k


@own("rf_sparse_prune_map")
def sparse_prune_map_ragged(x):
    m = _prune(x, _cells(5), _keep(5, N), COUNT, N)
    assert 100 < m["count"][0] == m["total"][0] < N and m["count"].tolist()[1:] == [0, int(m["count"][2]), 1]


@own("rf_sparse_prune_map")
def sparse_prune_map_dense_capped(x):
    m = _prune(x, _cells(6), _keep(6, N), None, 40)
    assert (m["count"] == 40).all() and (m["total"] > 40).all() and m["total"][3] == N


@own("rf_sparse_prune_map")
def sparse_prune_map_16384_rows(x):
    m = _prune(x, _lattice(), _keep(7, 16384), np.array([16384, 8191, 4096, 77], I32), 16384)
    assert m["count"][3] == 77 and m["src"][3, 76] == 76 and m["count"][0] > 8000


# ---- rf_sparse_lookup ------------------------------------------------------------------------------------------------------------
def _lookup(x, coords, table, count, tcount, shift):
    b, n = coords.shape[:2]
    m = table.shape[1]
    r = x.ref(lambda: dict(coords=_behind(coords, count, JUNK), table=_behind(table, tcount, JUNK),
                           idx=G.lookup_ref(coords, table, count, tcount, shift)))
    A = x.arena()
    A.add("coords", r["coords"], I32, "in", x.T)
    A.add("table", r["table"], I32, "in", x.res(8))
    if count is not None:
        A.add("count", count, I32, "in", x.L)
        A.add("tcount", tcount, I32, "in", x.L)
    A.add("idx", (b, n), I32, "out", x.res(12))
    A.build()
    x.call(A, "rf_sparse_lookup", b, n, m, shift, "coords", "count" if count is not None else None, "table",
           "tcount" if count is not None else None, "idx", None)
    got = A.get("idx")
    assert got.tobytes() == r["idx"].tobytes(), f"{x.cid}: idx differs from the restatement"
    x.keep("idx", got)
    return r["idx"]


@own("rf_sparse_lookup")
def sparse_lookup_ragged(x):
    idx = _lookup(x, _cells(8), _cells(9, 200), COUNT, np.array([200, 200, 0, 77], I32), 0)
    assert (idx[0] >= 0).sum() > 50 and (idx[1:3] == -1).all()


@own("rf_sparse_lookup")
def sparse_lookup_dense_shift_3(x):
    table = _cells(10, 500) * 7
    idx = _lookup(x, _cells(11), table, None, None, 3)
    assert (idx >= 0).mean() > 0.3 and (idx == -1).any()


@own("rf_sparse_lookup")
def sparse_lookup_16384_table_rows(x):
    table = _lattice()
    idx = _lookup(x, table[:, 16000:], table, np.array([384, 0, 77, 1], I32), np.array([16384, 16384, 16383, 4096], I32), 0)
    assert idx[0].tolist() == list(range(16000, 16384)) and idx[2, 76] == 16076 and idx[3, 0] == -1


# ---- rf_sparse_take_rows ---------------------------------------------------------------------------------------------------------
def _take(x, c, count):
    ns, nd = 57, N

    def inputs():
        rng = np.random.RandomState(c)
        src = rng.randn(B, ns, c).astype(F32)
        src[0, 3], src[1, 0, 0] = np.nan, np.inf
        idx = rng.randint(0, ns, (B, nd)).astype(I32)
        idx[:, ::5], idx[:, 1::11], idx[:, 2::13], idx[:, 3::17] = -1, ns, -(1 << 31), (1 << 31) - 1  # hostile, in front of the counts
        idx[0, :4] = [3, 56, 0, 3]
        want = G.take_ref(src, idx, count)
        return dict(src=src, idx=_behind(idx, count, 1 << 28), want=want)  # behind the counts: never read
    r = x.ref(inputs)
    A = x.arena()
    A.add("src", r["src"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.res(12))
    if count is not None:
        A.add("count", count, I32, "in", x.L)
    A.add("dst", (B, nd, c), F32, "out", x.T)
    A.build()
    x.call(A, "rf_sparse_take_rows", B, ns, nd, c, "src", "idx", "count" if count is not None else None, "dst", None)
    got = A.get("dst")
    assert got.tobytes() == r["want"].tobytes(), f"{x.cid}: dst is not a copy of the rows the restatement names"
    x.keep("dst", got)
    assert np.isnan(got[0, 0]).all() and not got[:, 0::5][:, 1:].view(np.uint32).any()


@own("rf_sparse_take_rows")
def sparse_take_rows_c12_ragged(x):
    _take(x, 12, COUNT)


@own("rf_sparse_take_rows")
def sparse_take_rows_c5_dense(x):
    _take(x, 5, None)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_sparse_generate(orc, cid, variant, poison):
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
