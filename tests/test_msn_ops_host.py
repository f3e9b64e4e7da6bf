"""CPU: the expansion penalty and minimum density sampling (include/rfops.h, "the expansion penalty and minimum density
sampling") at the boundary -- declared, exported, bound; every argument rule answered before a device is touched; the
wrappers' checks -- and xp_ref / mds_ref, the numpy restatements of the contract that the GPU tests hold the kernels to
bit for bit.  The restatements are checked here: the tree's total weight against scipy's minimum spanning tree, every
tree a spanning tree, a case by hand, the polynomial of the MDS weight against exp2."""
import ctypes
import re

import numpy as np
import pytest
import torch

XP_OK, XP_NONFINITE = 0, 1
MDS_OK, MDS_BADSIGMA = 0, 1
F32 = np.float32
XP_FAMILIES = ("uniform", "sheet", "lattice", "duplicates", "collinear", "outlier")
# rfnet_amd/csrc/msn_poly.hpp: c0 .. c5 of the degree-5 polynomial for 2^-f on [0, 1)
MDS_POLY = tuple(F32(float.fromhex(h)) for h in
                 ("0x1.fffffep-1", "-0x1.62e3a8p-1", "0x1.ebe2f2p-3", "-0x1.c5009p-5", "0x1.2dc434p-7", "-0x1.f06faep-11"))


# ---- the references ------------------------------------------------------------------------------------------------------
def d2_to(P, u):
    """((dx dx) + (dy dy)) + (dz dz) in fp32 from every row of P (k, 3) float32 to row u."""
    with np.errstate(all="ignore"):
        d = P - P[u]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        out = ((dx * dx) + (dy * dy)) + (dz * dz)
    assert out.dtype == F32
    return out


def _argmin_bits(val, barred):
    """The index minimising (bits(val), index) among the rows that are not barred."""
    key = (val.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(val.size, dtype=np.uint64)
    key[barred] = np.uint64(2 ** 64 - 1)
    return int(key.argmin())


def xp_tree(patch):
    """Steps 1-5 of the contract for one patch (S, 3) -> dict(status, key, father (local), length, mean64, mean)."""
    P = np.ascontiguousarray(patch, F32)
    S = P.shape[0]
    assert S >= 2
    if not np.isfinite(P).all():
        z = np.zeros(S, F32)
        return dict(status=XP_NONFINITE, key=z, father=np.arange(S, dtype=np.int32), length=z.copy(), mean64=0.0, mean=F32(0))
    key, father = d2_to(P, 0), np.zeros(S, np.int32)
    intree = np.zeros(S, bool)
    intree[0] = True
    for _ in range(S - 1):
        u = _argmin_bits(key, intree)
        intree[u] = True
        d = d2_to(P, u)
        upd = ~intree & (d < key)  # strictly: the earliest tree vertex keeps a tie
        key[upd], father[upd] = d[upd], u
    key[0] = 0
    length = np.sqrt(key)
    assert length.dtype == F32
    mean64 = float(np.cumsum(length[1:].astype(np.float64))[-1]) / float(S - 1)  # ascending, one pass
    return dict(status=XP_OK, key=key, father=father, length=length, mean64=mean64, mean=F32(mean64))


def xp_penalty(tree, alpha):
    """Step 6: dist (S,) float32."""
    bar = np.float64(F32(alpha)) * np.float64(tree["mean64"])
    return np.where(tree["length"].astype(np.float64) > bar, tree["length"], F32(0)).astype(F32)


def xp_ref(patch, alpha):
    """rf_expansion_penalty for one patch -> dict(dist, father (local indices), length, mean, status, key, mean64)."""
    r = xp_tree(patch)
    r["dist"] = xp_penalty(r, alpha)
    return r


def mds_weight(d2, c):
    with np.errstate(all="ignore"):
        s = d2 * c
        near = s < F32(64)
        sv = np.where(near, s, F32(0)).astype(F32)
        k = np.floor(sv)
        f = sv - k
        p = np.full_like(f, MDS_POLY[5])
        for ci in MDS_POLY[4::-1]:
            p = p * f
            p = p + ci
        w = np.where(near, np.ldexp(p, -k.astype(np.int32)), F32(0))
    assert f.dtype == F32 and p.dtype == F32
    return w.astype(F32)


def mds_ref(cloud, m, sigma, L=None):
    """rf_mds for one sample: cloud (n, 3), the first L rows valid -> (out (m,) int32, status, xyz (m, 3) float32)."""
    cloud = np.ascontiguousarray(cloud, F32)
    n = cloud.shape[0]
    L = n if L is None else min(max(int(L), 1), n)
    P, mo = cloud[:L], min(int(m), L)
    out, nx = np.zeros(m, np.int32), np.zeros((m, 3), F32)
    sg = F32(sigma)
    with np.errstate(all="ignore"):
        c = F32(np.float64(1.4426950408889634) / (np.float64(2.0) * np.float64(sg) * np.float64(sg)))
    if not (sg > 0) or c == 0 or np.isinf(c):
        out[:mo] = np.arange(mo)
        nx[:mo] = P[:mo]
        return out, MDS_BADSIGMA, nx
    dens, taken, u = np.zeros(L, F32), np.zeros(L, bool), 0
    for j in range(1, mo):
        taken[u] = True
        dens = dens + mds_weight(d2_to(P, u), c)
        assert dens.dtype == F32
        u = _argmin_bits(dens, taken)
        out[j] = u
    nx[:mo] = P[out[:mo]]
    return out, MDS_OK, nx


def xp_family(name, S, seed):
    """The input families of the penalty's tests -> (S, 3) float32."""
    rng = np.random.RandomState(seed)
    f = lambda x: np.ascontiguousarray(x, F32)  # noqa: E731
    if name == "uniform":
        return f(rng.rand(S, 3))
    if name == "sheet":  # a thin sheet
        return f(rng.rand(S, 3) * [1.0, 1.0, 1e-3])
    if name == "lattice":  # an 8^3 lattice in a random order (all ties; repeated beyond 512 points)
        g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) / 8.0
        return f(g[rng.permutation(512)[np.arange(S) % 512]])
    if name == "duplicates":  # 8 copies of every point: zero edges
        return f(rng.rand((S + 7) // 8, 3)[np.arange(S) // 8])
    if name == "collinear":
        return f(rng.rand(S, 1) * rng.randn(3))
    if name == "outlier":
        a = rng.rand(S, 3)
        a[rng.randint(0, S)] += 10.0
        return f(a)
    raise KeyError(name)


# ---- the restatements are checked ------------------------------------------------------------------------------------------
def _reaches_root(father):
    S = father.size
    cur = np.arange(S)
    for _ in range(S):
        cur = father[cur]
    return not cur.any()


@pytest.mark.parametrize("family", ["uniform", "sheet", "lattice", "duplicates"])
def test_xp_ref_total_weight_is_the_minimum_spanning_tree(family):
    from scipy.sparse.csgraph import minimum_spanning_tree
    S = 512
    P = xp_family(family, S, 3)
    r = xp_ref(P, 1.5)
    d2 = np.stack([d2_to(P, u) for u in range(S)]).astype(np.float64)
    assert np.array_equal(d2, d2.T)  # symmetric bit for bit
    pos = d2[d2 > 0]
    assert pos.size == 0 or pos.min() >= 2.0 ** -28  # so that d2 + 1 is exact in float64
    shifted = d2 + 1.0  # keeps zero-length edges in scipy's sparse graph
    np.fill_diagonal(shifted, 0.0)
    want = float(minimum_spanning_tree(shifted).sum()) - (S - 1)
    got = float(r["key"].astype(np.float64).sum())
    print(f"{family}: tree weight {got!r} scipy {want!r}")
    assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300) or got == want
    assert r["status"] == XP_OK and _reaches_root(r["father"]) and r["father"][0] == 0 and r["length"][0] == 0
    # every edge is the distance to its father
    v = np.arange(1, S)
    assert np.array_equal(r["key"][v], np.array([d2_to(P, int(r["father"][k]))[k] for k in v]))


@pytest.mark.parametrize("family", XP_FAMILIES)
@pytest.mark.parametrize("S", [2, 3, 37, 65])
def test_xp_ref_every_tree_is_a_spanning_tree(family, S):
    r = xp_ref(xp_family(family, S, 10 + S), 1.0)
    assert _reaches_root(r["father"]) and (r["father"] >= 0).all() and (r["father"] < S).all()


def test_xp_ref_by_hand():
    """Four collinear points at unit steps and one outlier 10 away from the last: edges 1, 1, 1, 10, mean 3.25; with
    alpha 1.5 the bar is 4.875 and exactly the outlier's edge is penalised."""
    P = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [3, 10, 0]], F32)
    r = xp_ref(P, 1.5)
    assert r["father"].tolist() == [0, 0, 1, 2, 3] and r["length"].tolist() == [0, 1, 1, 1, 10]
    assert r["mean"] == F32(3.25) and r["dist"].tolist() == [0, 0, 0, 0, 10]
    assert xp_ref(P, 0.0)["dist"].tolist() == [0, 1, 1, 1, 10]  # alpha 0: every edge of positive length
    # a tie: 0 and 2 are equally far from 1, the earliest tree vertex keeps the edge
    Q = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0]], F32)
    assert xp_ref(Q, 1.5)["father"].tolist() == [0, 2, 0]
    bad = P.copy()
    bad[2, 1] = np.inf
    r = xp_ref(bad, 1.5)
    assert r["status"] == XP_NONFINITE and r["father"].tolist() == [0, 1, 2, 3, 4] and not r["dist"].any() and r["mean"] == 0


def test_xp_ref_penalises_some_edges_and_not_all():
    r = xp_ref(xp_family("uniform", 512, 0), 1.5)
    k = int((r["dist"] != 0).sum())
    print(f"uniform, seed 0, S = 512, alpha 1.5: {k} of 511 edges penalised")
    assert 0 < k < 511


def test_the_polynomial_against_exp2():
    f = np.arange(1 << 20, dtype=np.float64) / float(1 << 20)
    ref = np.exp2(-f)
    p64 = np.full_like(f, float(MDS_POLY[5]))
    for ci in MDS_POLY[4::-1]:
        p64 = p64 * f + float(ci)
    fit = float(np.abs(p64 / ref - 1.0).max())  # the committed coefficients, evaluated in float64
    f32 = f.astype(F32)
    assert np.array_equal(f32.astype(np.float64), f)
    p = np.full_like(f32, MDS_POLY[5])
    for ci in MDS_POLY[4::-1]:
        p = p * f32
        p = p + ci
    assert p.dtype == F32
    got = float(np.abs(p.astype(np.float64) / ref - 1.0).max())
    bar = 4.0 * fit + 10.0 * 2.0 ** -24
    print(f"fit error in float64 {fit:.3e}; fp32 Horner {got:.3e}; bar {bar:.3e} = 4 x {fit:.3e} + 10 x 2^-24")
    assert got <= bar
    assert fit < 1.1e-7  # the figure msn_poly.hpp states
    # the weight itself: 2^-(d2 c) where d2 c < 64, exactly 0 from there on, NaN and inf included
    d2 = np.array([0.0, 0.5, 1.0, 63.99, 64.0, 1e30, np.inf, np.nan], F32)
    w = mds_weight(d2, F32(1.0))
    assert w[0] == MDS_POLY[0] and w[2] == F32(0.5) * MDS_POLY[0] and not w[4:].any() and 0 < w[3] < 2.0 ** -63


def test_the_polynomial_header_is_mirrored():
    from rfnet_amd import _lib
    src = open(_lib._PKG + "/csrc/msn_poly.hpp").read()
    got = [F32(float.fromhex(h)) for h in re.findall(r"#define RF_MDS_POLY_C\d (-?0x[0-9a-fp.\-]+)f\n", src)]
    assert len(got) == 6 and all(a == b for a, b in zip(got, MDS_POLY))


@pytest.mark.parametrize("sigma", [0.02, 0.1, 5.0, 1e15])
def test_mds_ref_returns_distinct_indices(sigma):
    rng = np.random.RandomState(4)
    P = rng.rand(300, 3).astype(F32)
    out, st, nx = mds_ref(P, 120, sigma)
    assert st == MDS_OK and out[0] == 0 and len(set(out.tolist())) == 120 and np.array_equal(nx, P[out])
    out, st, nx = mds_ref(P, 120, sigma, L=40)  # m above the count: the tail is zeros
    assert sorted(out[:40].tolist()) == list(range(40)) and not out[40:].any() and not nx[40:].any()


def test_mds_ref_bad_sigma_and_a_case_by_hand():
    P = np.array([[0, 0, 0], [1, 0, 0], [0.1, 0, 0], [5, 0, 0]], F32)
    for bad in (0.0, -1.0, np.nan, 1e-30, 1e30):
        out, st, _ = mds_ref(P, 3, bad)
        assert st == MDS_BADSIGMA and out.tolist() == [0, 1, 2]
    out, st, _ = mds_ref(P, 4, 1.0)  # the farthest first (lowest density under {0}), the nearest last
    assert st == MDS_OK and out.tolist() == [0, 3, 1, 2]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_expansion_penalty", "rf_expansion_penalty_grad", "rf_expansion_penalty_supported", "rf_mds", "rf_mds_supported")


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
    assert f"#define RF_XP_MAX_PATCH {_raw.XP_MAX_PATCH}\n" in header and _raw.XP_MAX_PATCH == 4096
    assert f"#define RF_MDS_MAX_POINTS {_raw.MDS_MAX_POINTS}\n" in header and _raw.MDS_MAX_POINTS == 16384
    for name, v in (("XP_OK", _raw.XP_OK), ("XP_NONFINITE", _raw.XP_NONFINITE), ("MDS_OK", _raw.MDS_OK),
                    ("MDS_BADSIGMA", _raw.MDS_BADSIGMA)):
        assert f"#define RF_{name} {v}\n" in header
    assert (_raw.XP_OK, _raw.XP_NONFINITE, _raw.MDS_OK, _raw.MDS_BADSIGMA) == (XP_OK, XP_NONFINITE, MDS_OK, MDS_BADSIGMA)
    for fn in ("expansion_penalty", "expansion_loss", "minimum_density_sample"):
        assert callable(getattr(glue, fn))


def test_supported():
    from rfnet_amd._lib import lib
    xs = lib.rf_expansion_penalty_supported
    assert xs(8192, 512) == 1 and xs(4096, 4096) == 1 and xs(2, 2) == 1 and xs(8192, 4096) == 1
    assert xs(8192, 4097) == 0 and xs(10, 1) == 0 and xs(10, 0) == 0 and xs(10, 3) == 0 and xs(0, 2) == 0 and xs(-4, 2) == 0
    assert xs(8194, 8194) == 0 and xs(10, -2) == 0
    ms = lib.rf_mds_supported
    assert ms(1) == 1 and ms(16384) == 1 and ms(16385) == 0 and ms(0) == 0 and ms(-1) == 0


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks


def _xp(b=2, n=1024, S=256, alpha=1.5, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 6  # xyz, dist, father, length, mean, info
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_expansion_penalty(b, n, S, alpha, *t, None)


def _xg(b=2, n=1024, S=256, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 5  # xyz, father, dist, gdist, grad
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_expansion_penalty_grad(b, n, S, *t, None)


def _mds(b=2, n=1000, m=10, ln=PTR, nx=PTR, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 4  # xyz, sigma, out, info
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_mds(b, n, m, t[0], t[1], ln, t[2], t[3], nx, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL = 0, -1
    sizes = (dict(S=1), dict(S=0), dict(S=4097, n=8194), dict(n=1000), dict(n=0), dict(n=128), dict(b=1 << 30, n=8, S=2))
    for call, ntensors in ((_xp, 6), (_xg, 5)):
        assert call(b=0) == OK and call(b=0, n=0, S=0) == OK and call(b=0, n=7, S=5) == OK
        for bad in (dict(b=-1), dict(n=-3), dict(S=-2), dict(b=0, n=-1)) + sizes:
            assert call(**bad) == EINVAL, (call.__name__, bad)
        for k in range(ntensors):
            assert call(null=k) == EINVAL, f"{call.__name__}: NULL tensor {k}"
            assert call(at=(k, PTR + 2)) == EINVAL, f"{call.__name__}: tensor {k} not 4-byte aligned"
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert _xp(alpha=bad) == EINVAL, bad
    # minimum density sampling
    assert _mds(b=0) == OK and _mds(b=0, n=0, m=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(m=-1), dict(b=0, n=-1), dict(n=0), dict(n=16385), dict(m=0)):
        assert _mds(**bad) == EINVAL, bad
    for k in range(4):
        assert _mds(null=k) == EINVAL, f"NULL tensor {k}"
        assert _mds(at=(k, PTR + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _mds(ln=PTR + 2) == EINVAL and _mds(nx=PTR + 1) == EINVAL


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a = np.zeros((2, 8, 3), F32)
    for fn, more in ((_raw.expansion_penalty, ()), (_raw.expansion_penalty_grad, (np.zeros((2, 8), np.int32),) + (np.zeros((2, 8), F32),) * 2)):
        with pytest.raises(ValueError, match="xyz"):
            fn(np.zeros((2, 8), F32), 4, *more)
        with pytest.raises(ValueError, match="primitive size"):
            fn(a, 1, *more)
        with pytest.raises(ValueError, match="primitive size"):
            fn(np.zeros((1, 8194, 3), F32), 4097, *more)
        with pytest.raises(ValueError, match="multiple"):
            fn(a, 3, *more)
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="alpha"):
            _raw.expansion_penalty(a, 4, bad)
    with pytest.raises(ValueError, match="father"):
        _raw.expansion_penalty_grad(a, 4, np.zeros((2, 7), np.int32), np.zeros((2, 8), F32), np.zeros((2, 8), F32))
    with pytest.raises(ValueError, match="grad_dist"):
        _raw.expansion_penalty_grad(a, 4, np.zeros((2, 8), np.int32), np.zeros((2, 8), F32), np.zeros((2, 9), F32))
    with pytest.raises(ValueError, match="xyz"):
        _raw.minimum_density_sample(np.zeros((2, 8, 2), F32), 4, 0.1)
    with pytest.raises(ValueError, match="at least one point"):
        _raw.minimum_density_sample(np.zeros((2, 0, 3), F32), 4, 0.1)
    with pytest.raises(ValueError, match="16384"):
        _raw.minimum_density_sample(np.zeros((1, 16385, 3), F32), 4, 0.1)
    with pytest.raises(ValueError, match="npoint"):
        _raw.minimum_density_sample(a, 0, 0.1)
    with pytest.raises(ValueError, match="sigma"):
        _raw.minimum_density_sample(a, 4, np.ones(3, F32))
    with pytest.raises(ValueError, match="lengths"):
        _raw.minimum_density_sample(a, 4, 0.1, lengths=[8, 9])
    with pytest.raises(ValueError, match="primitive size"):
        glue.expansion_penalty(torch.zeros(2, 8, 3), 1)
    with pytest.raises(ValueError, match="npoint"):
        glue.minimum_density_sample(torch.zeros(2, 8, 3), 0, 0.1)
