"""CPU: the numpy restatement of the strided sparse convolution contract (tests/sparse_stride_ref.py) against independent
routes -- a python dictionary of cells for the level map, float64 einsum on small-integer inputs for the four modes and both
weight gradients (where every fp32 operation is exact, so any order and any realisation must agree), the scatter definitions
of the two gradients, a float64 evaluation within the derived chain bound on random inputs -- and the ABI of the entries:
declared, exported, bound, every argument rule answered without a device."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_sizes as Z
import sparse_stride_ref as R
from sparse_stride_ref import F32, F64, I32
from test_sparse_conv_host import gamma, null_rule


def cells(seed, b, n, span=6, extra=True):
    """random cells of a small cube round the origin (negative coordinates, children sharing a coarse cell, duplicates), with
    rows out of range and at both edges of the range"""
    rng = np.random.RandomState(seed)
    c = rng.randint(-span, span, (b, n, 3)).astype(I32)
    if extra and n >= 10:
        c[0, 1] = [40000, 0, 0]          # out of range
        c[0, 2] = [0, -32769, 0]
        c[0, 3] = [32767, 32767, 32767]  # slot 7 of the last coarse cell
        c[0, 4] = [32766, 32767, 32767]  # slot 3 of the same
        c[0, 5] = [-32768, -32768, -32768]  # slot 0 of the first
        c[0, 6] = c[0, 7]                # a duplicate of a LATER row: row 6 is the live one
        c[0, 8] = [-1, -1, -1]           # floor: coarse (-1, -1, -1), slot 7
        c[0, 9] = [-2, -1, -3]           # coarse (-1, -1, -2), slot 0 1 1 = 3
    return c


def brute_map(coords, count, nc):
    b, n, _ = coords.shape
    out = dict(coords=np.zeros((b, nc, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               child=np.full((b, nc, 8), -1, I32), up=np.full((b, n), -1, I32))
    for s in range(b):
        M = n if count is None else min(max(int(count[s]), 0), n)
        first = {}
        for i in range(M):
            c = tuple(int(v) for v in coords[s, i])
            if all(-32768 <= v <= 32767 for v in c) and c not in first:
                first[c] = i
        coarse = sorted({(x // 2, y // 2, z // 2) for x, y, z in first})  # (python's // is the floor; tuples sort row-major)
        rank = {c: j for j, c in enumerate(coarse)}
        out["total"][s], out["count"][s] = len(coarse), min(len(coarse), nc)
        for j, c in enumerate(coarse[:nc]):
            out["coords"][s, j] = c
        for (x, y, z), i in first.items():
            j, t = rank[(x // 2, y // 2, z // 2)], (x % 2) * 4 + (y % 2) * 2 + (z % 2)
            if j < nc:
                out["child"][s, j, t], out["up"][s, i] = i, 8 * j + t
    return out


def same_map(got, want):
    return all(got[k].dtype == I32 and got[k].tobytes() == want[k].tobytes() and got[k].shape == want[k].shape for k in want)


# ---- the map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nc", [(200, 200), (200, 37), (10, 10), (1, 1)])
def test_map_ref_against_a_dictionary(n, nc):
    coords = cells(n + nc, 4, n)
    count = np.array([n, min(77, n), 0, 1], I32)
    for cnt in (None, count):
        got, want = R.map_ref(coords, cnt, nc), brute_map(coords, cnt, nc)
        assert same_map(got, want)
    if nc == 37:
        assert (want["total"][:2] > 37).all() and (want["count"][:2] == 37).all()  # truncation happened


def test_map_ref_edges():
    coords = cells(1, 1, 40)
    m = R.map_ref(coords)
    up, child, D = m["up"][0], m["child"][0], int(m["count"][0])
    assert (up[[1, 2, 7]] == -1).all() and up[6] >= 0  # out of range, and the later duplicate
    assert m["coords"][0, 0].tolist() == [-16384] * 3 and up[5] == 0  # the first cell, slot 0
    assert m["coords"][0, D - 1].tolist() == [16383] * 3 and up[3] == 8 * (D - 1) + 7 and up[4] == 8 * (D - 1) + 3
    assert child[D - 1].tolist() == [-1, -1, -1, 4, -1, -1, -1, 3]
    j8, j9 = up[8] >> 3, up[9] >> 3  # the shift is a floor: -1 >> 1 = -1, -3 >> 1 = -2
    assert m["coords"][0, j8].tolist() == [-1, -1, -1] and up[8] & 7 == 7
    assert m["coords"][0, j9].tolist() == [-1, -1, -2] and up[9] & 7 == 3
    assert (m["coords"][0, D:] == 0).all() and (child[D:] == -1).all() and m["total"][0] == D
    # a full 4^3 block: eight coarse cells of eight children each, in any order of the rows
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.array([-4, 8, 100])
    perm = np.random.RandomState(0).permutation(64)
    full = R.map_ref(g[perm][None].astype(I32))
    assert full["count"][0] == 8 and (full["child"][0, :8] >= 0).all() and (full["child"][0, 8:] == -1).all()
    assert np.array_equal(np.sort(full["child"][0, :8].reshape(-1)), np.arange(64))
    # the level's coords go into the next level
    nxt = R.map_ref(full["coords"], full["count"])
    assert nxt["count"][0] == 1 and nxt["coords"][0, 0].tolist() == [-1, 2, 25] and (nxt["child"][0, 0] == np.arange(8)).all()


def test_up_and_child_are_inverse_on_the_live_set():
    coords = cells(7, 3, 300)
    count = np.array([300, 150, 300], I32)
    for nc in (300, 41):
        m = R.map_ref(coords, count, nc)
        live = R.live_rows(coords, count)
        for s in range(3):
            up, child = m["up"][s], m["child"][s]
            assert (up[~live[s]] == -1).all() and (~live[s, :150]).any()
            i = np.nonzero(up >= 0)[0]
            assert live[s, i].all() and np.array_equal(child[up[i] >> 3, up[i] & 7], i)
            j, t = np.nonzero(child >= 0)
            assert np.array_equal(up[child[j, t]], 8 * j + t) and (j < m["count"][s]).all()
            dropped = live[s] & (up < 0)  # live rows without a parent: only under truncation
            assert dropped.any() == (m["total"][s] > nc)


@pytest.mark.parametrize("kind", ["spread", "lattice"])
def test_map_ref_at_16384_rows_against_unique_coarse_cells(kind):
    """The GPU tests trust map_ref at the contract's limit, so it is held there to another route: np.unique over the rows of
    the coarse cells themselves (lexicographic, which is row-major ascending) instead of over packed keys.  Every row of these
    two families is live, so the route needs no rule for duplicates."""
    n = 16384
    coords = Z.family(kind, n, 7, b=2)
    count = np.array([n // 2 + 1, n], I32)
    assert np.array_equal(R.live_rows(coords, count).sum(1), count)
    D = []
    for nc in (n, 700):  # all cells; truncating
        m = R.map_ref(coords, count, nc)
        for s, M in enumerate(count):
            c = coords[s, :M].astype(np.int64)
            cells_, rank = np.unique(np.floor_divide(c, 2), axis=0, return_inverse=True)
            rank, t = rank.reshape(-1), (c[:, 0] % 2) * 4 + (c[:, 1] % 2) * 2 + c[:, 2] % 2
            child, up = np.full((nc, 8), -1, I32), np.full(n, -1, I32)
            kept = rank < nc
            child[rank[kept], t[kept]] = np.arange(M)[kept]
            up[:M][kept] = (8 * rank + t)[kept]
            Dk = min(len(cells_), nc)
            assert m["total"][s] == len(cells_) and m["count"][s] == Dk
            assert np.array_equal(m["coords"][s, :Dk], cells_[:nc]) and not m["coords"][s, Dk:].any()
            assert np.array_equal(m["child"][s], child) and np.array_equal(m["up"][s], up)
            D.append(len(cells_))
    assert D[:2] == [n // 2 + 1, n] if kind == "spread" else 1900 < D[0] <= D[1] == 2048  # (the block has 2048 coarse cells)


# ---- the chains on integers: exact, so they must equal float64 einsum ----------------------------------------------------------
def int_case(seed, b=3, n=90, cin=5, cout=7, nc=None):
    rng = np.random.RandomState(seed)
    coords = cells(seed, b, n, span=4)
    count = np.array([n, n // 2, n][:b], I32)
    m = R.map_ref(coords, count, nc or n)
    nc = m["child"].shape[1]
    fine_in, coarse_in = rng.randint(-8, 9, (b, n, cin)).astype(F32), rng.randint(-8, 9, (b, nc, cin)).astype(F32)
    fine_g, coarse_g = rng.randint(-8, 9, (b, n, cout)).astype(F32), rng.randint(-8, 9, (b, nc, cout)).astype(F32)
    weight = rng.randint(-8, 9, (8, cin, cout)).astype(F32)
    return count, m, fine_in, coarse_in, fine_g, coarse_g, weight


def one_hot(m, count, n):
    """S (b, nc, 8, n) float64: S[s, j, t, i] = 1 where child[j][t] == i is in front of both counts"""
    child = m["child"]
    b, nc, _ = child.shape
    S = np.zeros((b, nc, 8, n), F64)
    for s in range(b):
        j, t = np.nonzero((child[s] >= 0) & (child[s] < count[s]) & (np.arange(nc)[:, None] < m["count"][s]))
        S[s, j, t, child[s, j, t]] = 1
    return S


@pytest.mark.parametrize("nc", [None, 23])
def test_modes_on_integers_equal_einsum_and_the_scatter_definitions(nc):
    count, m, fine_in, coarse_in, fine_g, coarse_g, w = int_case(3, nc=nc)
    n = fine_in.shape[1]
    S, w64 = one_hot(m, count, n), w.astype(F64)
    args = (m["child"], m["up"], n, count, m["count"])
    down = R.conv_ref(R.DOWN, fine_in, w, *args)
    assert np.array_equal(down.astype(F64), np.einsum("bjti,bic,tco->bjo", S, fine_in.astype(F64), w64)) and np.abs(down).max() > 100
    up = R.conv_ref(R.UP, coarse_in, w, *args)
    assert np.array_equal(up.astype(F64), np.einsum("bjti,bjc,tco->bio", S, coarse_in.astype(F64), w64)) and np.abs(up).max() > 50
    # the gradients by their scatter definitions: d down / d feat sends grad_out[j] @ weight[t]^T to child[j][t], d up / d feat
    # collects grad_out[child[j][t]] @ weight[t]^T at j
    dgi = R.conv_ref(R.DOWN_GRAD_INPUT, coarse_g, w, *args)
    want = np.zeros(fine_in.shape, F64)
    upgi_want = np.zeros(coarse_in.shape, F64)
    for s in range(len(count)):
        for j in range(int(m["count"][s])):
            for t in range(8):
                i = m["child"][s, j, t]
                if 0 <= i < count[s]:
                    want[s, i] += w64[t] @ coarse_g[s, j].astype(F64)
                    upgi_want[s, j] += w64[t] @ fine_g[s, i].astype(F64)
    assert np.array_equal(dgi.astype(F64), want) and np.abs(want).max() > 50
    upgi = R.conv_ref(R.UP_GRAD_INPUT, fine_g, w, *args)
    assert np.array_equal(upgi.astype(F64), upgi_want) and np.abs(upgi_want).max() > 100
    # up is down's gradient to the features with the weight transposed
    wt = np.ascontiguousarray(w.transpose(0, 2, 1))
    assert np.array_equal(R.conv_ref(R.UP, coarse_in, w, *args), R.conv_ref(R.DOWN_GRAD_INPUT, coarse_in, wt, *args))
    assert np.array_equal(R.conv_ref(R.DOWN, fine_in, w, *args), R.conv_ref(R.UP_GRAD_INPUT, fine_in, wt, *args))
    # rows behind the counts and rows that are not served: +0
    assert not down[1, int(m["count"][1]):].view(np.uint32).any() and not up[1, int(count[1]):].view(np.uint32).any()
    assert not up[m["up"] < 0].view(np.uint32).any()
    # the weight gradients
    gwd = R.grad_weight_ref(R.DOWN, fine_in, coarse_g, m["child"], count, m["count"])
    assert np.array_equal(gwd.astype(F64), np.einsum("bjti,bic,bjo->tco", S, fine_in.astype(F64), coarse_g.astype(F64)))
    gwu = R.grad_weight_ref(R.UP, fine_g, coarse_in, m["child"], count, m["count"])
    assert np.array_equal(gwu.astype(F64), np.einsum("bjti,bjc,bio->tco", S, coarse_in.astype(F64), fine_g.astype(F64)))
    assert np.abs(gwd).max() > 100 and np.abs(gwu).max() > 100


def test_garbage_in_child_and_up_is_absent():
    count, m, fine_in, coarse_in, fine_g, coarse_g, w = int_case(6)
    n, nc = fine_in.shape[1], coarse_in.shape[1]
    rng = np.random.RandomState(0)
    child, up = m["child"].copy(), m["up"].copy()
    for s in range(3):
        M, Mc = int(count[s]), int(m["count"][s])
        child[s, Mc:] = rng.randint(-3, n + 3, (nc - Mc, 8))  # coarse rows behind the count name live rows: never read
        hole = child[s, :Mc] == -1
        child[s, :Mc][hole] = rng.choice([-7, M, n, 1 << 20, -(1 << 31)], int(hole.sum()))  # outside [0, M)
        up[s, M:] = rng.randint(-3, 8 * nc + 9, n - M)  # fine rows behind the count
        dead = up[s, :M] == -1
        # a row that is not live claims a slot that is not its own: child does not confirm it
        up[s, :M][dead] = rng.choice([-9, 8 * Mc, 8 * nc + 5, 1 << 30, 0, 9], int(dead.sum()))
    good, bad = (m["child"], m["up"], n, count, m["count"]), (child, up, n, count, m["count"])
    for mode, src in ((R.DOWN, fine_in), (R.UP, coarse_in), (R.DOWN_GRAD_INPUT, coarse_g), (R.UP_GRAD_INPUT, fine_g)):
        assert np.array_equal(R.conv_ref(mode, src, w, *bad), R.conv_ref(mode, src, w, *good)), mode
    assert np.array_equal(R.grad_weight_ref(R.DOWN, fine_in, coarse_g, child, count, m["count"]),
                          R.grad_weight_ref(R.DOWN, fine_in, coarse_g, m["child"], count, m["count"]))
    assert np.array_equal(R.grad_weight_ref(R.UP, fine_g, coarse_in, child, count, m["count"]),
                          R.grad_weight_ref(R.UP, fine_g, coarse_in, m["child"], count, m["count"]))
    # a child entry that two coarse slots claim has the one writer `up` names
    two = m["child"].copy()
    s, (j, t) = 0, np.argwhere(m["child"][0] >= 0)[0]
    free = np.argwhere(two[0] == -1)[0]
    two[0, free[0], free[1]] = two[0, j, t]
    assert np.array_equal(R.conv_ref(R.UP, coarse_in, w, two, m["up"], n, count, m["count"]), R.conv_ref(R.UP, coarse_in, w, *good))


# ---- random fp32 inputs: within the chain bound of a float64 evaluation ---------------------------------------------------------
def pairs(m, count):
    """(sample, coarse row, slot, fine row) of every entry of child in front of both counts"""
    child = m["child"]
    nc = child.shape[1]
    ok = (child >= 0) & (child < count[:, None, None]) & (np.arange(nc)[None, :, None] < m["count"][:, None, None])
    s, j, t = np.nonzero(ok)
    return s, j, t, child[s, j, t]


def test_restatements_within_the_chain_bound_of_float64():
    """A chain of L fmaf steps from +0 differs from the exact sum by at most gamma_L * sum |terms| (Higham, Lemma 3.1 with one
    rounding per step): L = 8 cin for the gather modes, L = cin for the fan-out modes; the weight gradient has chains of at most
    1024 steps, double sums and one last rounding."""
    rng = np.random.RandomState(9)
    b, n, cin, cout = 2, 2300, 6, 4
    coords = cells(9, b, n, span=16)
    count = np.array([n, 400], I32)
    m = R.map_ref(coords, count)
    assert m["count"][0] > 1024  # the weight gradient's second chunk
    s, j, t, i = pairs(m, count)
    w = rng.randn(8, cin, cout).astype(F32)
    w64 = w.astype(F64)
    args = (m["child"], m["up"], n, count, m["count"])

    def check(mode, src, rows_out, at_out, at_src, wt, L):
        x64, cw = src.astype(F64), wt.shape[2]
        exact, mag = np.zeros((b, rows_out, cw)), np.zeros((b, rows_out, cw))
        np.add.at(exact, (s, at_out), np.einsum("pc,pco->po", x64[s, at_src], wt[t]))
        np.add.at(mag, (s, at_out), np.einsum("pc,pco->po", np.abs(x64[s, at_src]), np.abs(wt[t])))
        err = np.abs(R.conv_ref(mode, src, w, *args).astype(F64) - exact)
        assert (err <= gamma(L) * mag).all() and err.max() > 0, mode

    x, g = rng.randn(b, n, cin).astype(F32), rng.randn(b, n, cout).astype(F32)
    y, h = rng.randn(b, n, cin).astype(F32), rng.randn(b, n, cout).astype(F32)  # on the coarse rows (n_coarse = n)
    w64t = np.ascontiguousarray(w64.transpose(0, 2, 1))
    check(R.DOWN, x, n, j, i, w64, 8 * cin)
    check(R.UP_GRAD_INPUT, g, n, j, i, w64t, 8 * cout)
    check(R.UP, y, n, i, j, w64, cin)
    check(R.DOWN_GRAD_INPUT, h, n, i, j, w64t, cout)
    gm, u = gamma(R.WGRAD_ROWS), 2.0 ** -24  # (1 + g)(1 + u) - 1, and 2^-50 for the double sums
    bound = gm + u + gm * u + 2.0 ** -50
    for mode, fine, coarse in ((R.DOWN, x, h), (R.UP, g, y)):
        a64, b64 = (fine.astype(F64)[s, i], coarse.astype(F64)[s, j]) if mode == R.DOWN else (coarse.astype(F64)[s, j], fine.astype(F64)[s, i])
        exact, mag = np.zeros((8, cin, cout)), np.zeros((8, cin, cout))
        np.add.at(exact, t, np.einsum("pc,po->pco", a64, b64))
        np.add.at(mag, t, np.einsum("pc,po->pco", np.abs(a64), np.abs(b64)))
        err = np.abs(R.grad_weight_ref(mode, fine, coarse, m["child"], count, m["count"]).astype(F64) - exact)
        assert (err <= bound * mag).all() and err.max() > 0, mode


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_sparse_stride_map", "rf_sparse_conv_strided", "rf_sparse_conv_strided_grad_weight",
           "rf_sparse_conv_strided_grad_weight_workspace_bytes")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw, glue
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    for name, value in _raw.SS_MODES.items():
        assert f"#define RF_SS_{name.upper()} {value}\n" in header
    assert (R.DOWN, R.UP, R.DOWN_GRAD_INPUT, R.UP_GRAD_INPUT) == tuple(_raw.SS_MODES[k] for k in ("down", "up", "down_grad_input", "up_grad_input"))
    assert "Kernel 3 / stride 2" in header  # what is out of scope is said
    for fn in ("sparse_stride_map", "sparse_conv_strided", "sparse_conv_strided_grad_weight"):
        assert callable(getattr(_raw, fn))
    for fn in ("sparse_stride_map", "sparse_conv_down", "sparse_conv_up"):
        assert callable(getattr(glue, fn))
    assert issubclass(glue.SparseConv3d, torch.nn.Module) and issubclass(glue.SparseConvTranspose3d, torch.nn.Module)


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks
WS = 0x200000
BIG = 1 << 40


def _map(b=2, n=100, nc=60, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 7 + [None]  # coords, count, coords_out, count_out, total_out, child, up, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_stride_map(b, n, nc, *t)


def _conv(b=2, n=100, nc=60, cin=8, cout=8, mode=0, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 7 + [None]  # src, weight, child, up, count, count_coarse, out, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_conv_strided(b, n, nc, cin, cout, mode, *t)


def _wgrad(b=2, n=100, nc=60, cin=8, cout=8, mode=0, null=None, at=None, ws=WS, wsz=BIG):
    from rfnet_amd._lib import lib
    t = [PTR] * 6  # fine, coarse, child, count, count_coarse, grad_weight
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_conv_strided_grad_weight(b, n, nc, cin, cout, mode, *t, ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    from rfnet_amd._lib import lib
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    sizes = (dict(b=-1), dict(b=0, n=-1), dict(b=0, nc=-1), dict(b=65536), dict(n=0, nc=0), dict(n=16385), dict(nc=0), dict(nc=101))
    assert _map(b=0) == OK and _map(b=0, n=0, nc=5) == OK
    for bad in sizes:
        assert _map(**bad) == EINVAL, bad
    for t in range(7):
        null_rule(_map, t, t == 1, f"rf_sparse_stride_map: NULL tensor {t}")  # count may be NULL
        assert _map(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_stride_map: tensor {t} not 4-byte aligned"
    assert _conv(b=0) == OK and _conv(b=0, n=0, nc=7, cin=0, cout=0, mode=9) == OK
    for bad in sizes + (dict(b=0, cin=-1), dict(cin=0), dict(cin=257), dict(cout=0), dict(cout=257), dict(mode=4), dict(mode=-1)):
        assert _conv(**bad) == EINVAL, bad
    for t in range(7):
        null_rule(_conv, t, t in (4, 5), f"rf_sparse_conv_strided: NULL tensor {t}")
        assert _conv(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_conv_strided: tensor {t} not 4-byte aligned"
    assert _wgrad(b=0) == OK and _wgrad(b=0, n=0, nc=3, cin=0, cout=0, mode=7, ws=None, wsz=0) == OK
    for bad in sizes + (dict(b=0, cout=-1), dict(cin=0), dict(cin=257), dict(cout=0), dict(cout=257), dict(mode=2), dict(mode=3),
                        dict(mode=-1), dict(ws=None), dict(ws=WS + 8), dict(ws=WS + 4)):
        assert _wgrad(**bad) == EINVAL, bad
    for t in range(6):
        null_rule(_wgrad, t, t in (3, 4), f"rf_sparse_conv_strided_grad_weight: NULL tensor {t}")
        assert _wgrad(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_conv_strided_grad_weight: tensor {t} not 4-byte aligned"
    need = lib.rf_sparse_conv_strided_grad_weight_workspace_bytes(2, 8, 8)
    assert _wgrad(wsz=need - 1) == EWORKSPACE and _wgrad(wsz=0) == EWORKSPACE
    if not torch.cuda.is_available():  # a call that passes the rules gets as far as the device check
        assert _map() == -3 and _map(null=1, n=16384, nc=16384) == -3 and _map(nc=1) == -3
        assert all(_conv(mode=mode) == -3 for mode in range(4)) and _conv(mode=1, cin=256, cout=1, null=4) == -3
        assert _wgrad() == -3 and _wgrad(wsz=need, mode=1) == -3


def test_workspace_query_is_a_pure_host_function():
    from rfnet_amd._lib import lib
    q = lib.rf_sparse_conv_strided_grad_weight_workspace_bytes
    for b, cin, cout in ((1, 1, 1), (2, 8, 8), (32, 64, 128), (3, 256, 256), (65535, 3, 5)):
        w = q(b, cin, cout)
        assert w >= b * 8 * cin * cout * 8 and w % 256 == 0 and w < b * 8 * cin * cout * 8 + 256  # a double per element, honest
        assert q(b, cin, cout) == w
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (2, 0, 8), (2, 8, 257)):
        assert q(*bad) == 0, bad


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    coords = np.zeros((2, 8, 3), I32)
    with pytest.raises(ValueError, match="coords"):
        _raw.sparse_stride_map(np.zeros((2, 8, 2), I32))
    with pytest.raises(ValueError, match="16384"):
        _raw.sparse_stride_map(np.zeros((1, 16385, 3), I32))
    with pytest.raises(ValueError, match="max_cells"):
        _raw.sparse_stride_map(coords, max_cells=9)
    with pytest.raises(ValueError, match="max_cells"):
        _raw.sparse_stride_map(coords, max_cells=0)
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_stride_map(coords, nclusters=[8, 9])
    fine, coarse, w = np.zeros((2, 8, 4), F32), np.zeros((2, 5, 4), F32), np.zeros((8, 4, 6), F32)
    child, up = np.zeros((2, 5, 8), I32), np.zeros((2, 8), I32)
    with pytest.raises(ValueError, match="child"):
        _raw.sparse_conv_strided(fine, w, np.zeros((2, 5, 27), I32), up)
    with pytest.raises(ValueError, match="rows"):
        _raw.sparse_conv_strided(coarse, w, child, up)  # down takes the fine rows
    with pytest.raises(ValueError, match="rows"):
        _raw.sparse_conv_strided(fine, w, child, up, mode="up")
    with pytest.raises(ValueError, match="weight"):
        _raw.sparse_conv_strided(fine, np.zeros((27, 4, 6), F32), child, up)
    with pytest.raises(ValueError, match="weight"):
        _raw.sparse_conv_strided(coarse, w, child, up, mode="down_grad_input")  # (8, ci, co): 6 is not src's 4
    with pytest.raises(ValueError, match="256"):
        _raw.sparse_conv_strided(fine, np.zeros((8, 4, 257), F32), child, up)
    with pytest.raises(ValueError, match="mode"):
        _raw.sparse_conv_strided(fine, w, child, up, mode="generative")
    with pytest.raises(ValueError, match="nclusters_coarse"):
        _raw.sparse_conv_strided(fine, w, child, up, None, [6, 1])
    with pytest.raises(ValueError, match="max_cells"):
        _raw.sparse_conv_strided(coarse, w, np.zeros((2, 8, 8), I32), np.zeros((2, 5), I32))  # more coarse rows than fine
    with pytest.raises(ValueError, match="child"):
        _raw.sparse_conv_strided_grad_weight(fine, np.zeros((2, 5, 6), F32), np.zeros((2, 6, 8), I32))
    with pytest.raises(ValueError, match="mode"):
        _raw.sparse_conv_strided_grad_weight(fine, np.zeros((2, 5, 6), F32), child, mode="down_grad_input")
    for cls in (glue.SparseConv3d, glue.SparseConvTranspose3d):
        m = cls(4, 6, bias=False)
        assert tuple(m.weight.shape) == (8, 4, 6) and m.bias is None and bool(torch.isfinite(m.weight).all())
        assert tuple(cls(4, 6).bias.shape) == (6,)
