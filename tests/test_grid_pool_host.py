"""CPU: the numpy restatement of the grid pooling contract (tests/grid_pool_ref.py) against independent routes -- np.unique on
the cell triples, np.add.at in float64, a bit loop for Morton, the curve properties of the Hilbert key -- and the ABI of the
three entries: declared, exported, bound, and every argument rule answered without a device."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import grid_pool_ref as R
from grid_pool_ref import F32, F64, I32, I64, U64


def cloud(seed, b, n, scale=1.0):
    return (np.random.RandomState(seed).rand(b, n, 3).astype(F32) - F32(0.5)) * F32(scale)


# ---- the clustering against np.unique -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [0.03, 0.2])
def test_cluster_ref_against_unique(cell):
    xyz = cloud(1, 3, 700)
    xyz[1, 5] = np.nan
    xyz[2, 9, 1] = np.inf
    lengths = [700, 650, 1]
    r = R.cluster_ref(xyz, cell, "xyz", lengths)
    for s in range(3):
        L = lengths[s]
        ok = np.isfinite(xyz[s]).all(1) & (np.arange(700) < L)
        o = xyz[s][ok].min(0)
        assert np.array_equal(r["origin"][s], o)
        k = np.floor((xyz[s][ok].astype(F64) - o.astype(F64)) / F64(F32(cell))).astype(I64)
        cells, inverse, sizes = np.unique(k, axis=0, return_inverse=True, return_counts=True)  # rows in lexicographic order
        M = len(cells)
        assert r["nclusters"][s] == M and r["inside"][s] == ok.sum()
        assert np.array_equal(r["coords"][s, :M], cells) and not r["coords"][s, M:].any()
        assert np.array_equal(np.diff(r["starts"][s])[:M], sizes) and not np.diff(r["starts"][s])[M:].any()
        assert np.array_equal(r["cluster"][s][ok], inverse.reshape(-1)) and (r["cluster"][s][~ok] == -1).all()
        assert (r["code"][s][~ok] == -1).all()
        # order: the members of every cluster in ascending index
        for j in range(M):
            mem = r["order"][s, r["starts"][s, j]:r["starts"][s, j + 1]]
            assert np.array_equal(mem, np.nonzero(ok)[0][inverse.reshape(-1) == j])
        assert not r["order"][s, r["inside"][s]:].any()


def test_cluster_ref_edges():
    # -0 origin becomes +0; cells beyond +-32768 are not inside; an explicit origin gives negative k; no usable row
    xyz = np.array([[[-0.0, 0.0, 0.0], [0.0, -0.0, 1.0], [40000.0, 0.0, 0.0], [np.nan, 0, 0]]], F32)
    r = R.cluster_ref(xyz, 1.0)
    assert not r["origin"].view(np.uint32).any()
    assert r["cluster"][0].tolist() == [0, 1, -1, -1] and r["inside"][0] == 2
    r = R.cluster_ref(xyz, 1.0, origin=np.array([[32768.0, 5.0, 5.0]], F32))
    assert r["coords"][0, 0].tolist() == [-32768, -5, -5] and r["cluster"][0, 2] >= 0  # t = -32768 is inside
    r = R.cluster_ref(xyz, 1.0, origin=np.array([[32769.0, 5.0, 5.0]], F32))
    assert r["cluster"][0].tolist() == [-1, -1, 0, -1]
    r = R.cluster_ref(np.full((1, 4, 3), np.nan, F32), 0.5)
    assert r["inside"][0] == 0 and r["nclusters"][0] == 0 and not r["starts"].any() and (r["cluster"] == -1).all()
    assert not r["origin"].view(np.uint32).any()
    # exactly on a face: j / 64 with cell 1 / 16 is exact
    xyz = (np.arange(12, dtype=F32) / F32(64)).reshape(1, 4, 3)
    r = R.cluster_ref(xyz, 1.0 / 16, origin=np.zeros((1, 3), F32))
    assert r["coords"][0, :r["nclusters"][0]].tolist() == [[0, 0, 0], [0, 1, 1], [1, 1, 2], [2, 2, 2]]


# ---- the reductions against np.add.at -----------------------------------------------------------------------------------------
def test_pool_ref_against_add_at():
    xyz, feat = cloud(2, 2, 900), np.random.RandomState(3).randn(2, 900, 7).astype(F32) * F32(100)
    r = R.cluster_ref(xyz, 0.12)
    s_ref = R.pool_ref(feat, r["order"], r["starts"], r["nclusters"], "sum")
    m_ref = R.pool_ref(feat, r["order"], r["starts"], r["nclusters"], "mean")
    x_ref, arg = R.pool_ref(feat, r["order"], r["starts"], r["nclusters"], "max")
    for s in range(2):
        M = r["nclusters"][s]
        acc, mag, cnt = np.zeros((900, 7), F64), np.zeros((900, 7), F64), np.zeros(900, F64)
        np.add.at(acc, r["cluster"][s], feat[s].astype(F64))
        np.add.at(mag, r["cluster"][s], np.abs(feat[s].astype(F64)))
        np.add.at(cnt, r["cluster"][s], 1.0)
        # one fp32 rounding, plus n 2^-53 <= 2^-39 per term for a double sum of at most 16384 terms in another order, doubled
        assert (np.abs(s_ref[s] - acc) <= 2.0 ** -23 * np.abs(acc) + 2.0 ** -38 * mag).all()
        mean = acc[:M] / cnt[:M, None]
        assert (np.abs(m_ref[s, :M] - mean) <= 2.0 ** -23 * np.abs(mean) + 2.0 ** -38 * mag[:M] / cnt[:M, None]).all()
        assert not s_ref[s, M:].any() and not m_ref[s, M:].any() and not x_ref[s, M:].any() and not arg[s, M:].any()
        mx = np.full((900, 7), -np.inf)
        np.maximum.at(mx, r["cluster"][s], feat[s].astype(F64))
        assert np.array_equal(x_ref[s, :M], mx[:M].astype(F32))
        assert np.array_equal(np.take_along_axis(feat[s], arg[s, :M].astype(I64), 0), x_ref[s, :M])
        assert (r["cluster"][s][arg[s, :M]] == np.arange(M)[:, None]).all()


def test_pool_ref_max_rules():
    # ties go to the first member; a NaN is taken and ends the walk
    feat = np.array([[[1.0, 5.0], [1.0, np.nan], [2.0, 9.0], [7.0, 7.0]]], F32)
    order, starts, ncl = np.array([[0, 1, 2, 3]], I32), np.array([[0, 3, 4, 4, 4]], I32), np.array([2], I32)
    out, arg = R.pool_ref(feat, order, starts, ncl, "max")
    assert out[0, 0, 0] == 2.0 and arg[0, 0].tolist() == [2, 1] and np.isnan(out[0, 0, 1])
    assert out[0, 1].tolist() == [7.0, 7.0] and arg[0, 1].tolist() == [3, 3] and not out[0, 2:].any()
    feat[0, 2, 0] = 1.0
    assert R.pool_ref(feat, order, starts, ncl, "max")[1][0, 0, 0] == 0
    cluster = np.array([[0, 0, 0, 1]], I32)
    back = R.unpool_ref(out, cluster, arg=arg, mode="max")
    assert back[0, :, 0].tolist() == [0.0, 0.0, 2.0, 7.0]
    mean = R.unpool_ref(np.ones((1, 4, 2), F32), np.array([[0, -1, 0, 1]], I32), starts=starts, mode="mean")
    assert mean[0, :, 0].tolist() == [F32(1.0 / 3), 0.0, F32(1.0 / 3), 1.0]


# ---- the curves ---------------------------------------------------------------------------------------------------------------
def test_morton_against_a_bit_loop():
    rng = np.random.RandomState(4)
    pts = rng.randint(0, 65536, (200, 3))
    got = R.morton(pts[:, 0], pts[:, 1], pts[:, 2])
    for (x, y, z), g in zip(pts.tolist(), got.tolist()):
        want = 0
        for j in range(16):
            want |= ((x >> j) & 1) << (3 * j + 2) | ((y >> j) & 1) << (3 * j + 1) | ((z >> j) & 1) << (3 * j)
        assert g == want
    back = R.deinterleave(got)
    assert all(np.array_equal(back[a], pts[:, a].astype(U64)) for a in range(3))


@pytest.mark.parametrize("bits", [1, 2, 3, 4])
def test_hilbert_exhaustively_at_few_bits(bits):
    side = 1 << bits
    g = np.array(list(itertools.product(range(side), repeat=3)))
    h = R.hilbert_encode(g[:, 0], g[:, 1], g[:, 2], bits)
    assert sorted(h.tolist()) == list(range(side ** 3))  # a bijection
    assert h[0] == 0  # code 0 at cell (0, 0, 0)
    path = g[np.argsort(h)]
    assert (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()  # consecutive codes are face-adjacent
    x, y, z = R.hilbert_decode(h, bits)
    assert np.array_equal(np.stack([x, y, z], 1), g.astype(U64))
    m = R.morton(g[:, 0], g[:, 1], g[:, 2], bits)
    assert sorted(m.tolist()) == list(range(side ** 3)) and m[0] == 0


def test_hilbert_at_16_bits():
    rng = np.random.RandomState(5)
    p = rng.randint(0, 65536, (4000, 3))
    p[:8] = [[0, 0, 0], [65535, 65535, 65535], [65535, 0, 0], [0, 65535, 0], [0, 0, 65535], [32768, 32768, 32768],
             [32767, 32767, 32767], [1, 0, 0]]
    h = R.hilbert_encode(p[:, 0], p[:, 1], p[:, 2])
    assert h[0] == 0 and (h < U64(1) << U64(48)).all()
    assert np.array_equal(np.stack(R.hilbert_decode(h), 1), p.astype(U64))
    codes = rng.randint(0, 1 << 48, 4000, dtype=np.int64).astype(U64)
    codes[:2] = [0, (1 << 48) - 2]
    a, c = np.stack(R.hilbert_decode(codes), 1).astype(I64), np.stack(R.hilbert_decode(codes + U64(1)), 1).astype(I64)
    assert (np.abs(a - c).sum(1) == 1).all()
    assert np.array_equal(R.hilbert_encode(a[:, 0], a[:, 1], a[:, 2]), codes)


@pytest.mark.parametrize("curve", ["z", "hilbert"])
def test_prefix_property(curve):
    """code16(p) >> 3s == code(16 - s)(p >> s): coarsening a code coarsens the cell"""
    p = np.random.RandomState(6).randint(0, 65536, (3000, 3))
    enc = R.morton if curve == "z" else R.hilbert_encode
    full = enc(p[:, 0], p[:, 1], p[:, 2])
    for s in (1, 2, 5, 11, 15):
        q = p >> s
        assert np.array_equal(full >> U64(3 * s), enc(q[:, 0], q[:, 1], q[:, 2], 16 - s)), s


def test_orders_agree_on_the_clusters():
    """the three orders name the same cells: same sizes per cell, other ranks"""
    xyz = cloud(7, 1, 500)
    rs = {o: R.cluster_ref(xyz, 0.1, o) for o in R.ORDERS}
    for o in ("z", "hilbert"):
        assert rs[o]["nclusters"][0] == rs["xyz"]["nclusters"][0]
        M = rs[o]["nclusters"][0]
        a = {tuple(k): n for k, n in zip(rs[o]["coords"][0, :M].tolist(), np.diff(rs[o]["starts"][0])[:M].tolist())}
        b = {tuple(k): n for k, n in zip(rs["xyz"]["coords"][0, :M].tolist(), np.diff(rs["xyz"]["starts"][0])[:M].tolist())}
        assert a == b
        code = rs[o]["code"][0]
        assert np.array_equal(np.argsort(code, kind="stable"), rs[o]["order"][0])  # all inside here


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_grid_cluster", "rf_grid_pool", "rf_grid_unpool")


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
    assert f"#define RF_GC_MAX_POINTS {_raw.GC_MAX_POINTS}\n" in header and _raw.GC_MAX_POINTS == R.MAX_POINTS == 16384
    assert f"#define RF_GP_MAX_CHANNELS {_raw.GP_MAX_CHANNELS}\n" in header and _raw.GP_MAX_CHANNELS == R.MAX_CHANNELS
    for table, prefix in ((_raw.GC_ORDERS, "RF_GC_"), (_raw.GP_REDUCES, "RF_GP_"), (_raw.GU_MODES, "RF_GU_")):
        for name, value in table.items():
            assert f"#define {prefix}{name.upper()} {value}\n" in header
    for fn in ("grid_cluster", "grid_pool", "grid_unpool"):
        assert callable(getattr(_raw, fn)) and callable(getattr(glue, fn))
    assert callable(glue.serialize)


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks


def _gc(b=2, n=100, cell=0.05, order=0, null=None, at=None):
    from rfnet_amd._lib import lib
    # xyz, len, origin, origin_out, inside, nclusters, point_order, starts, cluster, coords, code, (stream)
    t = [PTR] * 11 + [None]
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_grid_cluster(b, n, cell, order, *t)


def _gp(b=2, n=100, c=8, reduce=1, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 5 + [PTR if reduce == 2 else None, None]  # feat, point_order, starts, nclusters, out, arg, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_grid_pool(b, n, c, reduce, *t)


def _gu(b=2, n=100, c=8, mode=0, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 5 + [None]  # src, cluster, starts, arg, dst, (stream)
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_grid_unpool(b, n, c, mode, *t)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL = 0, -1
    # an optional tensor left out passes the rules and the call goes on to the device: it is made only where there is none --
    # with a device it would launch a kernel on the made-up pointers
    launches = torch.cuda.is_available()
    assert _gc(b=0) == OK and _gc(b=0, n=0, cell=0.0, order=9) == OK
    for bad in (dict(b=-1), dict(b=0, n=-1), dict(b=65536), dict(n=0), dict(n=-3), dict(n=16385), dict(cell=0.0), dict(cell=-1.0),
                dict(cell=float("nan")), dict(cell=float("inf")), dict(order=3), dict(order=-1)):
        assert _gc(**bad) == EINVAL, bad
    for t in range(11):
        optional = t in (1, 2, 10)  # len, origin, code
        assert (optional and launches) or (_gc(null=t) == EINVAL) == (not optional), f"rf_grid_cluster: NULL tensor {t}"
        assert _gc(at=(t, PTR + 2)) == EINVAL, f"rf_grid_cluster: tensor {t} not 4-byte aligned"
    assert _gc(at=(10, PTR + 4)) == EINVAL  # code: 8 bytes
    assert _gp(b=0) == OK and _gp(b=0, n=0, c=0, reduce=7) == OK
    for bad in (dict(b=-1), dict(b=0, c=-1), dict(b=65536), dict(n=0), dict(n=16385), dict(c=0), dict(c=2049), dict(reduce=3),
                dict(reduce=-1)):
        assert _gp(**bad) == EINVAL, bad
    for t in range(5):
        assert _gp(null=t) == EINVAL and _gp(at=(t, PTR + 2)) == EINVAL, f"rf_grid_pool: tensor {t}"
    assert _gp(reduce=2, null=5) == EINVAL and _gp(reduce=1, at=(5, PTR)) == EINVAL and _gp(reduce=2, at=(5, PTR + 2)) == EINVAL
    assert _gu(b=0) == OK and _gu(b=0, n=0, c=0, mode=7) == OK
    for bad in (dict(b=-1), dict(b=0, n=-1), dict(b=65536), dict(n=0), dict(n=16385), dict(c=0), dict(c=2049), dict(mode=3),
                dict(mode=-1)):
        assert _gu(**bad) == EINVAL, bad
    for t in range(5):
        optional = t in (2, 3)  # starts, arg (mode copy)
        assert (optional and launches) or (_gu(null=t) == EINVAL) == (not optional), f"rf_grid_unpool: NULL tensor {t}"
        assert _gu(at=(t, PTR + 2)) == EINVAL, f"rf_grid_unpool: tensor {t} not 4-byte aligned"
    assert _gu(mode=1, null=2) == EINVAL and _gu(mode=2, null=3) == EINVAL
    if not torch.cuda.is_available():  # a call that passes the rules gets as far as the device check
        assert _gc() == -3 and _gc(null=10) == -3 and _gc(n=16384, order=2) == -3
        assert _gp() == -3 and _gp(reduce=2) == -3 and _gu() == -3 and _gu(mode=2) == -3


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    xyz = np.zeros((2, 8, 3), F32)
    with pytest.raises(ValueError, match="xyz"):
        _raw.grid_cluster(np.zeros((2, 8, 2), F32), 0.1)
    with pytest.raises(ValueError, match="16384"):
        _raw.grid_cluster(np.zeros((1, 16385, 3), F32), 0.1)
    for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="cell"):
            _raw.grid_cluster(xyz, cell)
    with pytest.raises(ValueError, match="order"):
        _raw.grid_cluster(xyz, 0.1, order="trans")
    with pytest.raises(ValueError, match="origin"):
        _raw.grid_cluster(xyz, 0.1, origin=np.zeros((3, 3), F32))
    with pytest.raises(ValueError, match="lengths"):
        _raw.grid_cluster(xyz, 0.1, lengths=[8, 9])
    with pytest.raises(ValueError, match="origin"):
        glue.grid_cluster(torch.zeros(2, 8, 3), 0.1, origin=[0.0, 1.0])
    feat, od, ss, nc = np.zeros((2, 8, 4), F32), np.zeros((2, 8), I32), np.zeros((2, 9), I32), np.zeros(2, I32)
    with pytest.raises(ValueError, match="feat"):
        _raw.grid_pool(np.zeros((2, 8), F32), od, ss, nc)
    with pytest.raises(ValueError, match="2048"):
        _raw.grid_pool(np.zeros((1, 2, 2049), F32), od, ss, nc)
    with pytest.raises(ValueError, match="reduce"):
        _raw.grid_pool(feat, od, ss, nc, reduce="min")
    with pytest.raises(ValueError, match="starts"):
        _raw.grid_pool(feat, od, od, nc)
    with pytest.raises(ValueError, match="nclusters"):
        _raw.grid_pool(feat, od, ss, np.zeros(3, I32))
    with pytest.raises(ValueError, match="cluster"):
        _raw.grid_unpool(feat, ss)
    with pytest.raises(ValueError, match="starts"):
        _raw.grid_unpool(feat, od, mode="mean")
    with pytest.raises(ValueError, match="arg"):
        _raw.grid_unpool(feat, od, mode="max")
    with pytest.raises(ValueError, match="mode"):
        _raw.grid_unpool(feat, od, mode="first")
    with pytest.raises(ValueError, match="reduce"):
        glue.grid_pool(torch.zeros(2, 8, 3), 0.1, reduce="first")
    with pytest.raises(ValueError, match="nclusters"):
        glue.grid_unpool(torch.zeros(2, 8, 4), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 9, dtype=torch.int32),
                         order=torch.zeros(2, 8, dtype=torch.int32))
