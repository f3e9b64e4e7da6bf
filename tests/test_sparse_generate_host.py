"""CPU: the numpy restatements of the decoder entries (tests/sparse_generate_ref.py) against independent routes -- np.unique
and dictionaries over whole samples instead of the row loops -- the properties the entries promise (up / child and src / dst
inverse, all eight children or none, stable pruning, the arithmetic shift of the lookup), the generated maps under
tests/sparse_stride_ref.py's convolution, and the ABI of the four entries: declared, exported, bound, every argument rule
answered by the built library on made-up pointers without a device."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_generate_ref as G
from sparse_conv_ref import live_rows
from sparse_generate_ref import F32, I32, I64
from test_sparse_conv_host import null_rule


def cells(seed, b, n, span=6, extra=True):
    """random cells of a small cube round the origin (duplicates, negative coordinates), with rows out of range and at both edges
    of the parents' range"""
    rng = np.random.RandomState(seed)
    c = rng.randint(-span, span, (b, n, 3)).astype(I32)
    if extra and n >= 12:
        c[0, 1] = [40000, 0, 0]            # out of range
        c[0, 2] = [0, -32769, 0]
        c[0, 3] = [16383, -16384, 16383]   # the parents' edges: children at 32767 and -32768
        c[0, 4] = [16384, 0, 0]            # live, no parent
        c[0, 5] = [0, 0, -16385]
        c[0, 6] = c[0, 7]                  # a duplicate of a LATER row: row 6 is the live one
        c[0, 8] = [-16383, 16383, -1]
        c[0, 9] = [32767, 32767, 32767]    # live, no parent
        c[0, 11] = c[0, 4]                 # a duplicate of a row that is no parent
    return c


# ---- the restatements against other routes --------------------------------------------------------------------------------------
def brute_generate(coords, count, nf):
    b, nc, _ = coords.shape
    out = dict(coords=np.zeros((b, nf, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               child=np.full((b, nc, 8), -1, I32), up=np.full((b, nf), -1, I32))
    live = live_rows(coords, count)  # np.unique over packed keys
    bits = np.array([[(t >> 2) & 1, (t >> 1) & 1, t & 1] for t in range(8)], I64)
    for s in range(b):
        c = coords[s].astype(I64)
        par = np.nonzero(live[s] & ((c >= -16384) & (c <= 16383)).all(1))[0]  # ascending rows
        kept = par[:nf // 8]
        out["total"][s], out["count"][s] = 8 * len(par), 8 * len(kept)
        fine = 8 * np.arange(len(kept))[:, None] + np.arange(8)[None, :]
        out["child"][s, kept] = fine
        out["up"][s, :8 * len(kept)] = (8 * kept[:, None] + np.arange(8)[None, :]).reshape(-1)
        out["coords"][s, :8 * len(kept)] = (2 * c[kept][:, None, :] + bits[None]).reshape(-1, 3)
    return out


@pytest.mark.parametrize("nc,nf", [(200, 1600), (200, 203), (20, 20), (12, 96), (1, 8), (3, 15)])
def test_generate_ref_against_unique_and_slices(nc, nf):
    coords = cells(nc + nf, 4, nc)
    count = np.array([nc, min(77, nc), 0, 1], I32)
    for cnt in (None, count):
        got, want = G.generate_ref(coords, cnt, nf), brute_generate(coords, cnt, nf)
        assert G.same_maps(got, want)
    if nf == 20:
        assert want["total"][0] > 16 and want["count"][0] == 16  # the cap: two parents of many
    if (nc, nf) == (3, 15):
        assert (want["count"] <= 8).all()  # 15 // 8 = 1 parent


def test_generate_ref_edges_and_default_size():
    coords = cells(1, 1, 40)
    m = G.generate_ref(coords)
    assert m["coords"].shape == (1, 320, 3)
    child, up, D = m["child"][0], m["up"][0], int(m["count"][0])
    assert (child[[1, 2, 4, 5, 7, 9, 11]] == -1).all() and (child[[3, 6, 8]] >= 0).all()
    r = child[3, 0] >> 3
    assert m["coords"][0, 8 * r].tolist() == [32766, -32768, 32766] and m["coords"][0, 8 * r + 7].tolist() == [32767, -32767, 32767]
    assert D == m["total"][0] and (up[D:] == -1).all() and not m["coords"][0, D:].any()
    # with no dead row the fine row of parent j, slot t is 8 j + t
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(1, -1, 3).astype(I32) - 1
    full = G.generate_ref(g)
    assert np.array_equal(full["child"][0], np.arange(27 * 8).reshape(27, 8)) and np.array_equal(full["up"][0], np.arange(216))
    # the children are distinct, in range, and their parents are the cells they came from; the slot is sparse_stride's
    fc = full["coords"][0].astype(I64)
    assert len({tuple(v) for v in fc}) == 216 and np.array_equal(fc >> 1, np.repeat(g[0], 8, 0))
    assert np.array_equal((fc[:, 0] & 1) * 4 + (fc[:, 1] & 1) * 2 + (fc[:, 2] & 1), np.tile(np.arange(8), 27))
    assert G.generate_ref(np.zeros((1, 5000, 3), I32))["up"].shape == (1, 16384)  # min(8 nc, 16384)


def test_up_and_child_are_inverse_and_a_parent_has_eight_children_or_none():
    coords = cells(7, 3, 300)
    count = np.array([300, 150, 300], I32)
    for nf in (2400, 333, 300):
        m = G.generate_ref(coords, count, nf)
        for s in range(3):
            up, child = m["up"][s], m["child"][s]
            has = (child >= 0).sum(1)
            assert set(has.tolist()) <= {0, 8}
            assert 8 * int((has == 8).sum()) == m["count"][s] <= m["total"][s] and m["count"][s] == min(m["total"][s], nf // 8 * 8)
            i = np.nonzero(up >= 0)[0]
            assert np.array_equal(i, np.arange(m["count"][s])) and np.array_equal(child[up[i] >> 3, up[i] & 7], i)
            j, t = np.nonzero(child >= 0)
            assert np.array_equal(up[child[j, t]], 8 * j + t)
            assert (np.diff(child[has == 8, 0]) == 8).all()  # the input order is kept


def test_generated_maps_under_the_strided_restatement():
    """RF_SS_UP on the generated maps: every created row is its parent's row times the slot's weight, exactly on integers"""
    rng = np.random.RandomState(3)
    coords = cells(3, 2, 60)
    count = np.array([60, 31], I32)
    m = G.generate_ref(coords, count, 200)
    feat, w = rng.randint(-8, 9, (2, 60, 5)).astype(F32), rng.randint(-8, 9, (8, 5, 7)).astype(F32)
    out = G.S.conv_ref(G.S.UP, feat, w, m["child"], m["up"], 200, m["count"], count)
    want = np.zeros((2, 200, 7), np.float64)
    for s in range(2):
        for i in range(int(m["count"][s])):
            want[s, i] = feat[s, m["up"][s, i] >> 3].astype(np.float64) @ w[m["up"][s, i] & 7].astype(np.float64)
    assert np.array_equal(out.astype(np.float64), want) and np.abs(want).max() > 50
    g = rng.randint(-8, 9, (2, 200, 7)).astype(F32)
    gf = G.S.conv_ref(G.S.UP_GRAD_INPUT, g, w, m["child"], m["up"], 200, m["count"], count)
    wantf = np.zeros((2, 60, 5), np.float64)
    for s in range(2):
        for i in range(int(m["count"][s])):
            wantf[s, m["up"][s, i] >> 3] += w[m["up"][s, i] & 7].astype(np.float64) @ g[s, i].astype(np.float64)
    assert np.array_equal(gf.astype(np.float64), wantf)


def brute_prune(coords, keep, count, no):
    b, n, _ = coords.shape
    out = dict(coords=np.zeros((b, no, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               src=np.full((b, no), -1, I32), dst=np.full((b, n), -1, I32))
    for s in range(b):
        M = n if count is None else min(max(int(count[s]), 0), n)
        sel = np.nonzero(keep[s, :M] != 0)[0]
        k = sel[:no]
        out["total"][s], out["count"][s] = len(sel), len(k)
        out["src"][s, :len(k)], out["dst"][s, k] = k, np.arange(len(k))
        out["coords"][s, :len(k)] = coords[s, k]
    return out


@pytest.mark.parametrize("n,no", [(200, 200), (200, 37), (200, 1), (1, 1)])
def test_prune_ref_against_nonzero(n, no):
    rng = np.random.RandomState(n + no)
    coords = cells(5, 4, n)
    keep = rng.randint(0, 3, (4, n)).astype(np.uint8) * np.array([1, 1, 1, 77], np.uint8)[:, None]  # any nonzero byte selects
    count = np.array([n, min(77, n), 0, 1], I32)
    for cnt in (None, count):
        got, want = G.prune_ref(coords, keep, cnt, no), brute_prune(coords, keep, cnt, no)
        assert G.same_maps(got, want)
        for s in range(4):  # src / dst inverse, stable
            src, dst, D = got["src"][s], got["dst"][s], int(got["count"][s])
            assert (np.diff(src[:D]) > 0).all() and (src[D:] == -1).all() and np.array_equal(dst[src[:D]], np.arange(D))
            i = np.nonzero(dst >= 0)[0]
            assert np.array_equal(src[dst[i]], i) and len(i) == D
    if no == 37:
        assert want["total"][0] > 37 == want["count"][0]
    # rows are carried as they are: out of range and duplicate rows too
    assert no < 200 or [40000, 0, 0] in G.prune_ref(coords, np.ones((4, n), np.uint8))["coords"][0].tolist()


def brute_lookup(coords, table, count, tcount, shift):
    b, n, _ = coords.shape
    idx = np.full((b, n), -1, I32)
    for s in range(b):
        M = n if count is None else min(max(int(count[s]), 0), n)
        Mt = table.shape[1] if tcount is None else min(max(int(tcount[s]), 0), table.shape[1])
        first = {}
        for k in range(Mt):
            t = tuple(int(v) for v in table[s, k])
            if all(-32768 <= v <= 32767 for v in t):
                first.setdefault(tuple(v // (1 << shift) for v in t), k)  # (python's // is the floor)
        for i in range(M):
            idx[s, i] = first.get(tuple(int(v) for v in coords[s, i]), -1)
    return idx


@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_lookup_ref_against_a_dictionary(shift):
    n, m = 150, 230
    table = cells(11, 3, m, span=40)
    table[1, 5] = [-32768, 32767, -1]
    table[1, 6] = [32768, 0, 0]  # not usable, though its shifted cell would be in range
    rng = np.random.RandomState(shift)
    coords = (table[:, rng.randint(0, m, n)].astype(I64) >> shift).astype(I32)  # cells that are there
    coords[:, ::7] += rng.randint(-3, 4, coords[:, ::7].shape)                  # and some that may not be
    coords[0, 3] = [-70000, 0, 0]
    count, tcount = np.array([n, 0, 40], I32), np.array([m, m, 0], I32)
    for cnt, tc in ((None, None), (count, None), (None, tcount), (count, tcount)):
        got = G.lookup_ref(coords, table, cnt, tc, shift)
        assert got.dtype == I32 and np.array_equal(got, brute_lookup(coords, table, cnt, tc, shift))
    full = G.lookup_ref(coords, table, None, None, shift)
    assert (full >= 0).sum() > n and full[0, 3] == -1


def test_lookup_finds_every_coarsened_cell_and_the_shift_is_arithmetic():
    table = cells(2, 2, 300, span=50, extra=False)
    table[0, 0], table[0, 1] = [-1, -8, -9], [-32768, 32767, 7]
    for s in (0, 1, 2, 5, 15):
        q = (table.astype(I64) >> s).astype(I32)
        idx = G.lookup_ref(q, table, shift=s)
        assert (idx >= 0).all() and (idx <= np.arange(300)[None, :]).all()  # found, at its own row or a lower one with that cell
        assert np.array_equal(table[0][idx[0]].astype(I64) >> s, q[0])
    assert G.lookup_ref(np.array([[[-1, -1, -2]]], I32), table[:1], shift=3)[0, 0] == 0   # -1 >> 3 = -1, -8 >> 3 = -1, -9 >> 3 = -2
    assert G.lookup_ref(np.array([[[0, -1, -1]]], I32), table[:1, :1], shift=3)[0, 0] == -1  # not a division towards zero
    assert G.lookup_ref(np.array([[[-1, 0, 0]]], I32), table[:1, 1:2], shift=15)[0, 0] == 0
    # duplicates in the table: the lowest row; queries are not de-duplicated
    t2 = np.array([[[5, 5, 5], [4, 4, 4], [5, 5, 5], [4, 4, 4]]], I32)
    assert G.lookup_ref(np.array([[[4, 4, 4], [5, 5, 5], [4, 4, 4]]], I32), t2)[0].tolist() == [1, 0, 1]
    # shift 0 between two duplicate-free levels: the two lookups are mutually inverse (sparse_take's precondition)
    rng = np.random.RandomState(0)
    a = np.unique(rng.randint(-4, 4, (90, 3)), axis=0).astype(I32)
    a, bb = a[rng.permutation(len(a))][None, :60], a[rng.permutation(len(a))][None, :50]
    ab, ba = G.lookup_ref(a, bb)[0], G.lookup_ref(bb, a)[0]
    i = np.nonzero(ab >= 0)[0]
    assert len(i) > 5 and np.array_equal(ba[ab[i]], i) and (ab >= 0).sum() == (ba >= 0).sum()


def test_take_ref_is_a_copy_with_zeros_elsewhere():
    rng = np.random.RandomState(4)
    src = rng.randn(2, 9, 5).astype(F32)
    src[0, 2, 1], src[0, 2, 3] = np.float32(np.nan), -0.0
    src.view(np.uint32)[0, 2, 2] = 0x7FC12345  # a NaN with a payload
    idx = np.array([[2, -1, 9, 0, 8, 2, -(1 << 31), 1 << 30, 3, 3, 3], [8] * 11], I32)
    out = G.take_ref(src, idx, np.array([11, 4], I32))
    assert out.shape == (2, 11, 5) and out[0, 0].tobytes() == src[0, 2].tobytes() == out[0, 5].tobytes()
    assert not out[0, [1, 2, 6, 7]].view(np.uint32).any() and not out[1, 4:].view(np.uint32).any()
    assert out[1, :4].tobytes() == np.repeat(src[1, 8:9], 4, 0).tobytes() and out[0, 4].tobytes() == src[0, 8].tobytes()
    # through a pruning and back: by src forward, by dst backward
    coords, keep = cells(4, 2, 9, extra=False), rng.randint(0, 2, (2, 9)).astype(np.uint8)
    p = G.prune_ref(coords, keep)
    fwd = G.take_ref(src, p["src"], p["count"])
    back = G.take_ref(fwd, p["dst"])
    assert np.array_equal(back.view(np.uint32), np.where(keep[:, :, None] != 0, src, F32(0)).view(np.uint32))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_sparse_generate_map", "rf_sparse_prune_map", "rf_sparse_lookup", "rf_sparse_take_rows")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw, glue
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    for fn in ("sparse_generate_map", "sparse_prune_map", "sparse_lookup", "sparse_take_rows"):
        assert callable(getattr(_raw, fn))
    for fn in ("sparse_generate_map", "sparse_conv_generate", "sparse_prune", "sparse_lookup", "sparse_take"):
        assert callable(getattr(glue, fn))
    assert issubclass(glue.SparseGenerativeConvTranspose3d, glue._SparseStrided) and issubclass(glue.SparsePrune, torch.nn.Module)
    assert "mutually inverse" in glue.sparse_take.__doc__  # the precondition is stated
    assert "generative" not in _raw.SS_MODES  # no new mode string: the generated maps go through "up"


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks


def _call(name, sizes, nptr, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * nptr + [None]  # ..., (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return getattr(lib, name)(*sizes, *t)


def _gen(b=2, nc=60, nf=100, **kw):  # coords, count, coords_out, count_out, total_out, child, up
    return _call("rf_sparse_generate_map", (b, nc, nf), 7, **kw)


def _prune(b=2, n=100, no=60, **kw):  # coords, keep, count, coords_out, count_out, total_out, src, dst
    return _call("rf_sparse_prune_map", (b, n, no), 8, **kw)


def _look(b=2, n=100, m=60, shift=0, **kw):  # coords, count, table, tcount, idx
    return _call("rf_sparse_lookup", (b, n, m, shift), 5, **kw)


def _take(b=2, ns=100, nd=60, c=8, **kw):  # src, idx, count_dst, dst
    return _call("rf_sparse_take_rows", (b, ns, nd, c), 4, **kw)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL = 0, -1
    assert _gen(b=0) == OK and _gen(b=0, nc=0, nf=3) == OK
    for bad in (dict(b=-1), dict(b=0, nc=-1), dict(b=0, nf=-1), dict(b=65536), dict(nf=7, nc=7), dict(nf=7, nc=1), dict(nf=16385),
                dict(nf=16385, nc=16385), dict(nc=0), dict(nc=101), dict(nc=9, nf=8)):
        assert _gen(**bad) == EINVAL, bad
    for t in range(7):
        null_rule(_gen, t, t == 1, f"rf_sparse_generate_map: NULL tensor {t}")  # count may be NULL
        assert _gen(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_generate_map: tensor {t} not 4-byte aligned"

    assert _prune(b=0) == OK and _prune(b=0, n=0, no=9) == OK
    for bad in (dict(b=-1), dict(b=0, n=-1), dict(b=0, no=-1), dict(b=65536), dict(n=0, no=0), dict(n=16385), dict(n=16385, no=16385),
                dict(no=0), dict(no=101)):
        assert _prune(**bad) == EINVAL, bad
    for t in range(8):
        null_rule(_prune, t, t == 2, f"rf_sparse_prune_map: NULL tensor {t}")  # count may be NULL; keep may not
        if t != 1:
            assert _prune(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_prune_map: tensor {t} not 4-byte aligned"

    assert _look(b=0) == OK and _look(b=0, n=0, m=0, shift=99) == OK
    for bad in (dict(b=-1), dict(b=0, n=-1), dict(b=0, m=-1), dict(b=65536), dict(n=0), dict(m=0), dict(n=16385), dict(m=16385),
                dict(shift=-1), dict(shift=16)):
        assert _look(**bad) == EINVAL, bad
    for t in range(5):
        null_rule(_look, t, t in (1, 3), f"rf_sparse_lookup: NULL tensor {t}")
        assert _look(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_lookup: tensor {t} not 4-byte aligned"

    assert _take(b=0) == OK and _take(b=0, ns=0, nd=0, c=0) == OK
    for bad in (dict(b=-1), dict(b=0, ns=-1), dict(b=0, nd=-1), dict(b=0, c=-1), dict(b=65536), dict(ns=0), dict(nd=0), dict(ns=16385),
                dict(nd=16385), dict(c=0), dict(c=2049)):
        assert _take(**bad) == EINVAL, bad
    for t in range(4):
        null_rule(_take, t, t == 2, f"rf_sparse_take_rows: NULL tensor {t}")
        assert _take(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_take_rows: tensor {t} not 4-byte aligned"

    if not torch.cuda.is_available():  # a call that passes the rules gets as far as the device check
        assert _gen() == -3 and _gen(nc=16384, nf=16384, null=1) == -3 and _gen(nc=1, nf=8) == -3
        assert _prune() == -3 and _prune(n=16384, no=1) == -3 and _prune(at=(1, PTR + 1)) == -3  # keep at an odd address
        assert _look() == -3 and _look(shift=15, n=1, m=16384) == -3 and _look(n=16384, m=1) == -3
        assert _take() == -3 and _take(c=2048, ns=16384, nd=1) == -3 and _take(c=1, at=(0, PTR + 4)) == -3


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    coords = np.zeros((2, 8, 3), I32)
    with pytest.raises(ValueError, match="coords"):
        _raw.sparse_generate_map(np.zeros((2, 8, 2), I32))
    with pytest.raises(ValueError, match="16384"):
        _raw.sparse_generate_map(np.zeros((1, 16385, 3), I32))
    for bad in (7, 16385, 0):
        with pytest.raises(ValueError, match="max_cells"):
            _raw.sparse_generate_map(coords, max_cells=bad)
    with pytest.raises(ValueError, match="max_cells"):
        _raw.sparse_generate_map(np.zeros((1, 9, 3), I32), max_cells=8)  # fewer fine rows than coarse rows
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_generate_map(coords, nclusters=[8, 9])
    with pytest.raises(ValueError, match="keep"):
        _raw.sparse_prune_map(coords, np.ones((2, 7), bool))
    with pytest.raises(ValueError, match="coords"):
        _raw.sparse_prune_map(np.zeros((2, 8), I32), np.ones((2, 8), bool))
    for bad in (0, 9):
        with pytest.raises(ValueError, match="max_cells"):
            _raw.sparse_prune_map(coords, np.ones((2, 8), bool), max_cells=bad)
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_prune_map(coords, np.ones((2, 8), np.float32), nclusters=[1, -1])
    with pytest.raises(ValueError, match="table"):
        _raw.sparse_lookup(coords, np.zeros((2, 8, 4), I32))
    with pytest.raises(ValueError, match="batch"):
        _raw.sparse_lookup(coords, np.zeros((3, 8, 3), I32))
    for bad in (-1, 16):
        with pytest.raises(ValueError, match="shift"):
            _raw.sparse_lookup(coords, coords, shift=bad)
    with pytest.raises(ValueError, match="table_nclusters"):
        _raw.sparse_lookup(coords, np.zeros((2, 5, 3), I32), None, [6, 1])
    with pytest.raises(ValueError, match="src"):
        _raw.sparse_take_rows(np.zeros((2, 8), F32), np.zeros((2, 8), I32))
    with pytest.raises(ValueError, match="2048"):
        _raw.sparse_take_rows(np.zeros((1, 2, 2049), F32), np.zeros((1, 2), I32))
    with pytest.raises(ValueError, match="idx"):
        _raw.sparse_take_rows(np.zeros((2, 8, 4), F32), np.zeros((3, 8), I32))
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_take_rows(np.zeros((2, 8, 4), F32), np.zeros((2, 5), I32), [6, 1])
    m = glue.SparseGenerativeConvTranspose3d(4, 6, bias=False)
    assert tuple(m.weight.shape) == (8, 4, 6) and m.bias is None and bool(torch.isfinite(m.weight).all())
    assert tuple(glue.SparseGenerativeConvTranspose3d(4, 6).bias.shape) == (6,)
    assert glue.SparsePrune(max_cells=5).max_cells == 5
