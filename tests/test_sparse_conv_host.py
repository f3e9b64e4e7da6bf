"""CPU: the numpy restatement of the sparse convolution contract (tests/sparse_conv_ref.py) against independent routes -- a
dictionary of cells for the map, int64 brute force on small-integer inputs for the convolution and both gradients (where every
fp32 operation is exact, so any order and any realisation must agree), a float64 evaluation within the derived chain bound on
random inputs -- and the ABI of the entries: declared, exported, bound, every argument rule answered without a device."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_ref as R
import sparse_sizes as Z
from sparse_conv_ref import F32, F64, I32, I64


def cells(seed, b, n, span=6, extra=True):
    """random cells in a small cube (many neighbours, some duplicates), with rows out of range and at the range's edge"""
    rng = np.random.RandomState(seed)
    c = rng.randint(-span, span, (b, n, 3)).astype(I32)
    if extra and n >= 8:
        c[0, 1] = [40000, 0, 0]        # out of range
        c[0, 2] = [0, -32769, 0]
        c[0, 3] = [32767, 32767, 32767]  # neighbours fall outside
        c[0, 4] = [32766, 32767, 32767]
        c[0, 5] = [-32768, -32768, -32768]
        c[0, 6] = c[0, 7]              # a duplicate of a LATER row: row 6 is the live one
    return c


def brute_map(coords, count, ks, dilation):
    b, n, _ = coords.shape
    off = R.offsets(ks, dilation)
    nbr = np.full((b, n, ks ** 3), -1, I32)
    for s in range(b):
        M = n if count is None else min(max(int(count[s]), 0), n)
        first = {}
        for i in range(M):
            c = tuple(int(v) for v in coords[s, i])
            if all(-32768 <= v <= 32767 for v in c) and c not in first:
                first[c] = i
        for c, i in first.items():
            for t, o in enumerate(off):
                nbr[s, i, t] = first.get((c[0] + int(o[0]), c[1] + int(o[1]), c[2] + int(o[2])), -1)
    return nbr


# ---- the map -----------------------------------------------------------------------------------------------------------------
def test_offsets_are_mirrored_about_the_centre():
    for ks, d in ((3, 1), (5, 1), (3, 2), (5, 7)):
        off = R.offsets(ks, d)
        K = ks ** 3
        assert off.shape == (K, 3) and np.array_equal(off[::-1], -off) and not off[(K - 1) // 2].any()
        r = ks // 2
        t = ((1 + r) * ks + (-1 + r)) * ks + (0 + r)
        assert off[t].tolist() == [d, -d, 0]


@pytest.mark.parametrize("ks,dilation", [(3, 1), (5, 1), (3, 2), (5, 3)])
def test_map_ref_against_a_dictionary(ks, dilation):
    coords = cells(ks + dilation, 3, 200)
    count = np.array([200, 77, 0], I32)
    for cnt in (None, count):
        assert np.array_equal(R.map_ref(coords, cnt, ks, dilation), brute_map(coords, cnt, ks, dilation))


def test_map_ref_edges():
    coords = cells(1, 1, 40)
    nbr = R.map_ref(coords, None, 3, 1)
    live = R.live_rows(coords)
    assert not live[0, 1] and not live[0, 2] and live[0, 6] and not live[0, 7]
    assert (nbr[0, [1, 2, 7]] == -1).all() and not (nbr == 7).any()  # rows that are not live name nobody, nobody names them
    assert nbr[0, 3, 13] == 3 and nbr[0, 3, 4] == 4 and nbr[0, 4, 22] == 3  # (32767,..) and its -x neighbour
    assert (nbr[0, 3, [14, 16, 22]] == -1).all()  # targets beyond 32767 are absent
    assert nbr[0, 5, 13] == 5 and (np.delete(nbr[0, 5], 13) == -1).all()  # isolated at -32768: only the centre
    assert (R.map_ref(coords, [0], 3, 1) == -1).all()
    # a full 5^3 block: every slot of the centre cell is live
    blk = (R.offsets(5, 1) + 100).astype(I32)[None]
    full = R.map_ref(blk, None, 5, 1)
    assert np.array_equal(full[0, 62], np.arange(125))
    # coordinates in another order give the same map up to the renaming of the rows
    perm = np.random.RandomState(0).permutation(125)
    again = R.map_ref(blk[:, perm], None, 5, 1)
    inv = np.argsort(perm)
    assert np.array_equal(np.where(again[0] >= 0, perm[np.maximum(again[0], 0)], -1)[inv], full[0])


@pytest.mark.parametrize("ks", [3, 5])
def test_map_symmetry_on_the_live_set(ks):
    coords = cells(7, 2, 300)
    count = np.array([300, 150], I32)
    nbr = R.map_ref(coords, count, ks, 2 if ks == 3 else 1)
    live, K = R.live_rows(coords, count), ks ** 3
    assert (nbr[~live] == -1).all() and (~live[0, :300]).any()
    for s in range(2):
        i, t = np.nonzero(nbr[s] >= 0)
        j = nbr[s, i, t]
        assert len(i) > 300 and live[s, j].all() and live[s, i].all()
        assert np.array_equal(nbr[s, j, K - 1 - t], i)  # nbr[i][t] = j  =>  nbr[j][K-1-t] = i (and <= by symmetry of the roles)


# ---- the chains on integers: exact, so they must equal int64 brute force ------------------------------------------------------
def int_case(seed, b=2, n=90, cin=5, cout=7, ks=3):
    rng = np.random.RandomState(seed)
    coords = cells(seed, b, n, span=3)
    count = np.array([n, n // 2][:b], I32)
    nbr = R.map_ref(coords, count, ks, 1)
    feat = rng.randint(-8, 9, (b, n, cin)).astype(F32)
    weight = rng.randint(-8, 9, (ks ** 3, cin, cout)).astype(F32)
    gout = rng.randint(-8, 9, (b, n, cout)).astype(F32)
    return coords, count, nbr, feat, weight, gout


def test_conv_ref_on_integers_is_exact():
    _, count, nbr, feat, weight, _ = int_case(3)
    b, n, cin = feat.shape
    want = np.zeros((b, n, weight.shape[2]), I64)
    for s in range(b):
        for i in range(int(count[s])):
            for t in range(27):
                j = nbr[s, i, t]
                if 0 <= j < count[s]:
                    want[s, i] += feat[s, j].astype(I64) @ weight[t].astype(I64)
    got = R.conv_ref(feat, weight, nbr, count)
    assert np.array_equal(got.astype(I64), want) and np.abs(want).max() > 100
    assert not got[1, int(count[1]):].view(np.uint32).any()  # rows behind the count: +0


def test_grad_input_ref_equals_the_scatter_definition():
    """grad_feat[j] = sum over (i, t) with nbr[i][t] = j of grad_out[i] @ weight[t]^T -- the mirrored gather of the contract
    must give exactly that: the test of the symmetry argument"""
    _, count, nbr, feat, weight, gout = int_case(4)
    b, n, cin = feat.shape
    want = np.zeros((b, n, cin), I64)
    for s in range(b):
        for i in range(int(count[s])):
            for t in range(27):
                j = nbr[s, i, t]
                if 0 <= j < count[s]:
                    want[s, j] += weight[t].astype(I64) @ gout[s, i].astype(I64)
    got = R.grad_input_ref(gout, weight, nbr, count)
    assert np.array_equal(got.astype(I64), want) and np.abs(want).max() > 100


def test_grad_weight_ref_on_integers_is_exact():
    _, count, nbr, feat, weight, gout = int_case(5)
    b, n, cin = feat.shape
    want = np.zeros(weight.shape, I64)
    for s in range(b):
        for i in range(int(count[s])):
            for t in range(27):
                j = nbr[s, i, t]
                if 0 <= j < count[s]:
                    want[t] += np.outer(feat[s, j].astype(I64), gout[s, i].astype(I64))
    got = R.grad_weight_ref(feat, gout, nbr, count)
    assert np.array_equal(got.astype(I64), want) and np.abs(want).max() > 100


def test_garbage_in_nbr_is_absent():
    _, count, nbr, feat, weight, gout = int_case(6)
    bad = nbr.copy()
    bad[1, int(count[1]):] = 5            # rows behind the count name live rows: never read
    hole = bad[0] == -1
    bad[0][hole] = np.random.RandomState(0).choice([-7, 90, 1 << 20, -(1 << 31)], int(hole.sum()))  # outside [0, M)
    assert np.array_equal(R.conv_ref(feat, weight, bad, count), R.conv_ref(feat, weight, nbr, count))
    assert np.array_equal(R.grad_weight_ref(feat, gout, bad, count), R.grad_weight_ref(feat, gout, nbr, count))


# ---- random fp32 inputs: within the chain bound of a float64 evaluation ---------------------------------------------------------
def gamma(L):
    u = 2.0 ** -24
    return L * u / (1 - L * u)


def test_restatements_within_the_chain_bound_of_float64():
    """A chain of L fmaf steps from +0 differs from the exact sum by at most gamma_L * sum |terms| (Higham, Accuracy and
    Stability, Lemma 3.1 with one rounding per step); the float64 evaluation's own error is 2^-29 of that and is covered by
    the slack of counting L from the slots actually taken, rounded up.  The weight gradient adds 2^-24 for its last rounding."""
    rng = np.random.RandomState(9)
    coords = cells(9, 2, 1100, span=7)
    count = np.array([1100, 400], I32)
    nbr = R.map_ref(coords, count, 3, 1)
    b, n, cin, cout = 2, 1100, 6, 4
    feat, gout = rng.randn(b, n, cin).astype(F32), rng.randn(b, n, cout).astype(F32)
    weight = rng.randn(27, cin, cout).astype(F32)
    M = count[:, None, None]
    use = (np.arange(n)[None, :, None] < M) & (nbr >= 0) & (nbr < M)
    fpad = np.concatenate([feat, np.zeros((b, 1, cin), F32)], 1).astype(F64)
    col = fpad[np.arange(b)[:, None, None], np.where(use, nbr, n)]  # (b, n, K, cin), zeros in absent slots
    taken = use.sum(2)
    # forward
    exact = np.einsum("bnkc,kco->bno", col, weight.astype(F64))
    mag = np.einsum("bnkc,kco->bno", np.abs(col), np.abs(weight.astype(F64)))
    err = np.abs(R.conv_ref(feat, weight, nbr, count).astype(F64) - exact)
    bound = gamma(taken * cin + 1)[:, :, None] * mag
    assert (err <= bound).all() and err.max() > 0
    # gradient to the features, against the scatter in float64
    g64 = gout.astype(F64) * (np.arange(n)[None, :, None] < count[:, None, None])
    contrib = np.einsum("bno,kco->bnkc", g64, weight.astype(F64)) * use[..., None]
    exact_gi, mag_gi = np.zeros((b, n + 1, cin)), np.zeros((b, n + 1, cin))
    idx = np.where(use, nbr, n)
    for s in range(b):
        np.add.at(exact_gi[s], idx[s].reshape(-1), contrib[s].reshape(-1, cin))
        np.add.at(mag_gi[s], idx[s].reshape(-1), np.einsum("no,kco->nkc", np.abs(g64[s]), np.abs(weight.astype(F64))).reshape(-1, cin)
                  * use[s].reshape(-1, 1))
    err = np.abs(R.grad_input_ref(gout, weight, nbr, count).astype(F64) - exact_gi[:, :n])
    # (by symmetry a row is named as often as it names: its chain has taken * cout steps)
    assert (err <= gamma(taken * cout + 1)[:, :, None] * mag_gi[:, :n]).all() and err.max() > 0
    # gradient to the weight: chains of at most 1024 steps, then exact-to-2^-53 double sums, then one rounding
    exact_gw = np.einsum("bnkc,bno->kco", col, g64)
    mag_gw = np.einsum("bnkc,bno->kco", np.abs(col), np.abs(g64))
    err = np.abs(R.grad_weight_ref(feat, gout, nbr, count).astype(F64) - exact_gw)
    g, u = gamma(R.WGRAD_ROWS), 2.0 ** -24  # (1 + g)(1 + u) - 1, and 2^-50 for the double sums
    assert (err <= (g + u + g * u + 2.0 ** -50) * mag_gw).all() and err.max() > 0


# ---- the restatement at the contract's limit: the GPU tests trust it at 16384 rows, so it is held there too ----------------------
@pytest.mark.parametrize("kind", ["lattice", "cube"])
def test_map_ref_at_16384_rows_against_a_dictionary(kind):
    """a plain lookup of cell -> lowest row: "lattice" has every row live and most slots present, "cube" a fifth duplicates"""
    n = 16384
    coords = Z.family("lattice", n, 3, b=2) if kind == "lattice" else cells(3, 2, n, span=16)
    count = np.array([n // 2 + 1, n], I32)
    nbr = R.map_ref(coords, count, 3, 1)
    assert np.array_equal(nbr, brute_map(coords, count, 3, 1))
    live = R.live_rows(coords, count).sum(1)
    if kind == "lattice":
        assert np.array_equal(live, count) and (nbr[1] >= 0).mean() > 0.9 and nbr[1].max() == n - 1
    else:
        assert 0.1 * n < n - live[1] < 0.3 * n and live[0] < count[0]


def test_grad_weight_ref_over_16_chunks_within_the_chain_bound_of_float64():
    """n = 16384: sixteen chains of 1024 steps per slot and sample, added in double.  The bound is that of the test above: every
    chunk's chain is within gamma_1024 of its exact sum, so their sum is within gamma_1024 of sum |terms|; then one rounding."""
    rng = np.random.RandomState(11)
    b, n, cin, cout = 2, 16384, 3, 5
    coords = Z.family("lattice", n, 5, b=b)
    count = np.array([n // 2 + 1, n], I32)
    nbr = R.map_ref(coords, count, 3, 1)
    feat, gout = rng.randn(b, n, cin).astype(F32), rng.randn(b, n, cout).astype(F32)
    M = count[:, None, None]
    use = (np.arange(n)[None, :, None] < M) & (nbr >= 0) & (nbr < M)
    assert use[1, -R.WGRAD_ROWS:].any(0).all() and use[0, 8 * R.WGRAD_ROWS].any()  # the sixteenth chunk; the ninth's one row
    fpad = np.concatenate([feat, np.zeros((b, 1, cin), F32)], 1).astype(F64)
    col = fpad[np.arange(b)[:, None, None], np.where(use, nbr, n)]  # (b, n, K, cin), zeros in absent slots
    g64 = gout.astype(F64) * (np.arange(n)[None, :, None] < count[:, None, None])
    exact = np.einsum("bnkc,bno->kco", col, g64)
    mag = np.einsum("bnkc,bno->kco", np.abs(col), np.abs(g64))
    err = np.abs(R.grad_weight_ref(feat, gout, nbr, count).astype(F64) - exact)
    g, u = gamma(R.WGRAD_ROWS), 2.0 ** -24
    assert (err <= (g + u + g * u + 2.0 ** -50) * mag).all() and err.max() > 0


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_sparse_conv_map", "rf_sparse_conv", "rf_sparse_conv_grad_weight", "rf_sparse_conv_grad_weight_workspace_bytes")


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
    assert f"#define RF_SC_MAX_CHANNELS {_raw.SC_MAX_CHANNELS}\n" in header and _raw.SC_MAX_CHANNELS == R.MAX_CHANNELS == 256
    assert f"#define RF_SC_MAX_DILATION {_raw.SC_MAX_DILATION}\n" in header and _raw.SC_MAX_DILATION == R.MAX_DILATION
    assert f"#define RF_SC_WGRAD_ROWS {_raw.SC_WGRAD_ROWS}\n" in header and _raw.SC_WGRAD_ROWS == R.WGRAD_ROWS
    for name, value in _raw.SC_MODES.items():
        assert f"#define RF_SC_{name.upper()} {value}\n" in header
    for fn in ("sparse_conv_map", "sparse_conv"):
        assert callable(getattr(_raw, fn)) and callable(getattr(glue, fn))
    assert callable(_raw.sparse_conv_grad_weight) and issubclass(glue.SubMConv3d, torch.nn.Module)


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks
WS = 0x200000
BIG = 1 << 40


def _map(b=2, n=100, ks=3, dilation=1, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR, PTR, PTR, None]  # coords, count, nbr, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_conv_map(b, n, ks, dilation, *t)


def _conv(b=2, n=100, K=27, cin=8, cout=8, mode=0, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 5 + [None]  # feat, weight, nbr, count, out, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_conv(b, n, K, cin, cout, mode, *t)


def _wgrad(b=2, n=100, K=27, cin=8, cout=8, null=None, at=None, ws=WS, wsz=BIG):
    from rfnet_amd._lib import lib
    t = [PTR] * 5  # feat, grad_out, nbr, count, grad_weight
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sparse_conv_grad_weight(b, n, K, cin, cout, *t, ws, wsz, None)


def null_rule(call, t, optional, what):
    """A mandatory tensor left out is RF_EINVAL.  An optional one left out passes the rules, and the call goes on to the device:
    it is made only where there is none -- with a device it would launch a kernel on the made-up pointers."""
    if optional and torch.cuda.is_available():
        return
    assert (call(null=t) == -1) == (not optional), what


def test_argument_rules_are_answered_without_a_device():
    from rfnet_amd._lib import lib
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    assert _map(b=0) == OK and _map(b=0, n=0, ks=4, dilation=0) == OK
    for bad in (dict(b=-1), dict(b=0, n=-1), dict(b=65536), dict(n=0), dict(n=16385), dict(ks=1), dict(ks=4), dict(ks=7), dict(ks=-3),
                dict(dilation=0), dict(dilation=-1), dict(dilation=1025)):
        assert _map(**bad) == EINVAL, bad
    for t in range(3):
        null_rule(_map, t, t == 1, f"rf_sparse_conv_map: NULL tensor {t}")  # count may be NULL
        assert _map(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_conv_map: tensor {t} not 4-byte aligned"
    assert _conv(b=0) == OK and _conv(b=0, n=0, K=5, cin=0, cout=0, mode=9) == OK
    for bad in (dict(b=-1), dict(b=0, cin=-1), dict(b=65536), dict(n=0), dict(n=16385), dict(K=26), dict(K=9), dict(K=343), dict(cin=0),
                dict(cin=257), dict(cout=0), dict(cout=257), dict(mode=2), dict(mode=-1)):
        assert _conv(**bad) == EINVAL, bad
    for t in range(5):
        null_rule(_conv, t, t == 3, f"rf_sparse_conv: NULL tensor {t}")
        assert _conv(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_conv: tensor {t} not 4-byte aligned"
    assert _wgrad(b=0) == OK and _wgrad(b=0, n=0, K=5, cin=0, cout=0, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(b=0, cout=-1), dict(b=65536), dict(n=0), dict(n=16385), dict(K=28), dict(cin=0), dict(cin=257),
                dict(cout=0), dict(cout=257), dict(ws=None), dict(ws=WS + 8), dict(ws=WS + 4)):
        assert _wgrad(**bad) == EINVAL, bad
    for t in range(5):
        null_rule(_wgrad, t, t == 3, f"rf_sparse_conv_grad_weight: NULL tensor {t}")
        assert _wgrad(at=(t, PTR + 2)) == EINVAL, f"rf_sparse_conv_grad_weight: tensor {t} not 4-byte aligned"
    need = lib.rf_sparse_conv_grad_weight_workspace_bytes(2, 27, 8, 8)
    assert _wgrad(wsz=need - 1) == EWORKSPACE and _wgrad(wsz=0) == EWORKSPACE
    if not torch.cuda.is_available():  # a call that passes the rules gets as far as the device check
        assert _map() == -3 and _map(null=1, ks=5, dilation=1024, n=16384) == -3
        assert _conv() == -3 and _conv(mode=1, K=125, cin=256, cout=1, null=3) == -3
        assert _wgrad() == -3 and _wgrad(wsz=need) == -3


def test_workspace_query_is_a_pure_host_function():
    from rfnet_amd._lib import lib
    q = lib.rf_sparse_conv_grad_weight_workspace_bytes
    for b, K, cin, cout in ((1, 27, 1, 1), (2, 27, 8, 8), (32, 27, 64, 64), (3, 125, 256, 256), (65535, 27, 3, 5)):
        w = q(b, K, cin, cout)
        assert w >= b * K * cin * cout * 8 and w % 256 == 0 and w < b * K * cin * cout * 8 + 256  # a double per element, honest
        assert q(b, K, cin, cout) == w
    for bad in ((0, 27, 8, 8), (-1, 27, 8, 8), (65536, 27, 8, 8), (2, 26, 8, 8), (2, 27, 0, 8), (2, 27, 8, 257)):
        assert q(*bad) == 0, bad


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    coords = np.zeros((2, 8, 3), I32)
    with pytest.raises(ValueError, match="coords"):
        _raw.sparse_conv_map(np.zeros((2, 8, 2), I32))
    with pytest.raises(ValueError, match="16384"):
        _raw.sparse_conv_map(np.zeros((1, 16385, 3), I32))
    with pytest.raises(ValueError, match="kernel_size"):
        _raw.sparse_conv_map(coords, kernel_size=4)
    with pytest.raises(ValueError, match="dilation"):
        _raw.sparse_conv_map(coords, dilation=0)
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_conv_map(coords, nclusters=[8, 9])
    with pytest.raises(ValueError, match="nclusters"):
        _raw.sparse_conv_map(coords, nclusters=[8, 8, 8])
    feat, w, nbr = np.zeros((2, 8, 4), F32), np.zeros((27, 4, 6), F32), np.zeros((2, 8, 27), I32)
    with pytest.raises(ValueError, match="feat"):
        _raw.sparse_conv(np.zeros((2, 8), F32), w, nbr)
    with pytest.raises(ValueError, match="weight"):
        _raw.sparse_conv(feat, np.zeros((27, 5, 6), F32), nbr)
    with pytest.raises(ValueError, match="weight"):
        _raw.sparse_conv(feat, w, nbr, mode="grad_input")  # (K, cout, cin): 6 is not feat's 4
    with pytest.raises(ValueError, match="K = 27"):
        _raw.sparse_conv(feat, np.zeros((9, 4, 6), F32), np.zeros((2, 8, 9), I32))
    with pytest.raises(ValueError, match="256"):
        _raw.sparse_conv(feat, np.zeros((27, 4, 257), F32), nbr)
    with pytest.raises(ValueError, match="nbr"):
        _raw.sparse_conv(feat, w, np.zeros((2, 8, 125), I32))
    with pytest.raises(ValueError, match="mode"):
        _raw.sparse_conv(feat, w, nbr, mode="transposed")
    with pytest.raises(ValueError, match="grad_out"):
        _raw.sparse_conv_grad_weight(feat, np.zeros((2, 9, 6), F32), nbr)
    with pytest.raises(ValueError, match="nbr"):
        _raw.sparse_conv_grad_weight(feat, np.zeros((2, 8, 6), F32), np.zeros((2, 9, 27), I32))
    with pytest.raises(ValueError, match="kernel_size"):
        glue.SubMConv3d(4, 6, kernel_size=7)
    m = glue.SubMConv3d(4, 6, kernel_size=5, dilation=2, bias=False)
    assert tuple(m.weight.shape) == (125, 4, 6) and m.bias is None and bool(torch.isfinite(m.weight).all())
