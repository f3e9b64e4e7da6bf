"""CPU: the exact-EMD entries (include/rfops.h, "the exact earth mover's distance") at the boundary -- declared, exported,
bound; the workspace size; every argument rule answered before a device is touched; the wrappers' checks -- and ea_ref,
the numpy restatement of the contract that the GPU tests hold the kernel to bit for bit, checked here against scipy's
linear_sum_assignment on the integer cost matrix (D <= OPT <= P, and P - D <= L when the auction ran to its end), a case
by hand and the capped route."""
import ctypes

import numpy as np
import pytest
import torch

EA_OK, EA_CAPPED, EA_NONFINITE = 0, 1, 2
EPS = (1 << 17, 1 << 14, 1 << 11, 1 << 8, 1 << 5, 1 << 2, 1)
FAMILIES = ("uniform", "noisy_copy", "dup_objects", "dup_both", "lattice", "identical", "collinear")


# ---- the reference ------------------------------------------------------------------------------------------------------
def ea_grid(a, c, L):
    """-> k (S = 2^k), or None when the largest extent of the 2 L valid points is NaN or infinite."""
    pts = np.concatenate([a[:L], c[:L]]).astype(np.float32)
    with np.errstate(all="ignore"):
        E = np.float32((pts.max(0) - pts.min(0)).max())  # numpy's min / max propagate a NaN
    if not np.isfinite(E):
        return None
    ex = 0 if E == 0 else int(np.frexp(E)[1])
    return 19 - max(ex, -100)


def ea_costs(a, c, L, k):
    """-> (d (L, L) float32, c (L, L) int64): unfused fp32 distances, correctly rounded sqrt, costs on the grid 2^-k."""
    a, c = np.asarray(a, np.float32), np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (a[:L, None, t] - c[None, :L, t] for t in range(3))
        d = np.sqrt(((dx * dx) + (dy * dy)) + (dz * dz))
        assert d.dtype == np.float32
        q = np.fmin(d * np.float32(2.0 ** k), np.float32(2.0 ** 20))
    return d, np.rint(q).astype(np.int64)


def ea_ref(a, c, L=None, max_rounds=0):
    """a, c (n, 3) float32, the first L rows are the clouds -> dict with the outputs of rf_emd_assign for one sample
    (match12, match21 (n,) int32, dist (n,) float32, cost / gap / bound float32, cost64 the float64 sum, P, D, status,
    rounds, bids, k, prices (L,)).  Integers are int64 throughout; p < 2^26 is asserted after every round."""
    a, c = np.asarray(a, np.float32), np.asarray(c, np.float32)
    n = a.shape[0]
    L = n if L is None else int(L)
    ar = np.arange(L)
    out = dict(match12=np.zeros(n, np.int32), match21=np.zeros(n, np.int32), dist=np.zeros(n, np.float32), rounds=0, bids=0,
               k=0, status=EA_OK)
    k = ea_grid(a, c, L)
    if k is None:
        out["match12"][:L] = out["match21"][:L] = ar
        out["status"] = EA_NONFINITE
        return out
    d, C = ea_costs(a, c, L, k)
    assert C.min() >= 0 and C.max() < 1 << 20
    cap = int(max_rounds) if max_rounds else 64 * L + 1024
    p, owner = np.zeros(L, np.int64), np.full(L, -1, np.int64)
    rounds = bids = 0
    capped = False
    for eps in EPS:
        owner[:] = -1
        U = ar.copy()
        while U.size:
            if rounds >= cap:
                capped = True
                break
            V = C[U] + p[None, :]
            key = V * 8192 + (ar[None, :] - U[:, None]) % L  # (v, (j - i) mod L) as one integer: L <= 4096
            rows = np.arange(U.size)
            js = key.argmin(1)
            v1 = V[rows, js]
            if L == 1:
                w = v1
            else:
                key[rows, js] = np.iinfo(np.int64).max
                w = key.min(1) >> 13
            beta = p[js] + (w - v1) + eps
            order = np.lexsort((U, -beta, js))  # by object, the highest bid first, ties to the lowest person
            first = np.r_[True, js[order][1:] != js[order][:-1]]
            win = order[first]
            old = owner[js[win]]
            owner[js[win]], p[js[win]] = U[win], beta[win]
            lost = np.ones(U.size, bool)
            lost[win] = False
            rounds, bids = rounds + 1, bids + U.size
            U = np.sort(np.r_[U[lost], old[old >= 0]])
            assert p.max() < 1 << 26
        if capped:
            break
    if capped:  # the unassigned persons in ascending i take the free objects in ascending j
        has = np.zeros(L, bool)
        has[owner[owner >= 0]] = True
        owner[np.flatnonzero(owner < 0)] = np.flatnonzero(~has)
    m12 = np.empty(L, np.int64)
    m12[owner] = ar
    assert sorted(owner.tolist()) == list(range(L))
    out["match21"][:L], out["match12"][:L] = owner, m12
    out["dist"][:L] = d[ar, m12]
    P, D = int(C[ar, m12].sum()), int((C + p[None, :]).min(1).sum() - p.sum())
    cost64 = float(np.cumsum(out["dist"][:L].astype(np.float64))[-1])  # in index order
    out.update(P=P, D=D, k=k, rounds=rounds, bids=bids, status=EA_CAPPED if capped else EA_OK, prices=p, cost64=cost64,
               cost=np.float32(cost64), gap=np.float32((P - D) / 2.0 ** k), bound=np.float32((P - D + L) / 2.0 ** k))
    return out


def ea_family(name, n, seed):
    """The input families of the issue -> (xyz1 (n, 3), xyz2 (n, 3)) float32."""
    rng = np.random.RandomState(seed)
    f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    if name == "uniform":
        return f(rng.rand(n, 3)), f(rng.rand(n, 3))
    if name == "noisy_copy":
        a = rng.rand(n, 3)
        return f(a), f(a[rng.permutation(n)] + 0.01 * rng.randn(n, 3))
    if name == "dup_objects":  # 8 copies of every object
        return f(rng.rand(n, 3)), f(rng.rand((n + 7) // 8, 3)[np.arange(n) // 8])
    if name == "dup_both":
        return f(rng.rand((n + 7) // 8, 3)[np.arange(n) // 8]), f(rng.rand((n + 7) // 8, 3)[rng.permutation(n) // 8])
    if name == "lattice":  # a 4^3 lattice: many exact ties
        g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) / 4.0
        return f(g[rng.randint(0, 64, n)]), f(g[rng.randint(0, 64, n)])
    if name == "identical":
        return f(np.tile(rng.rand(1, 3), (n, 1))), f(np.tile(rng.rand(1, 3), (n, 1)) * 0 + 0.25)
    if name == "collinear":
        u = rng.randn(3)
        return f(rng.rand(n, 1) * u), f(rng.rand(n, 1) * u)
    raise KeyError(name)


def check_certificate(r, a, c, L):
    """D <= OPT <= P on the integer grid (scipy's optimum), P - D <= L when the auction ran to its end."""
    from scipy.optimize import linear_sum_assignment
    _, C = ea_costs(a, c, L, r["k"])
    rows, cols = linear_sum_assignment(C)
    opt = int(C[rows, cols].sum())
    assert r["D"] <= opt <= r["P"], (r["D"], opt, r["P"])
    if r["status"] == EA_OK:
        assert r["P"] - r["D"] <= L, (r["P"], r["D"], L)
    return opt


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130, 257])
@pytest.mark.parametrize("family", FAMILIES)
def test_ea_ref_is_certified_against_the_hungarian_optimum(family, n):
    a, c = ea_family(family, n, 100 + n)
    r = ea_ref(a, c)
    assert r["status"] == EA_OK and r["rounds"] < 64 * n + 1024  # the default cap is not what ended it
    opt = check_certificate(r, a, c, n)
    print(f"{family} n={n}: rounds {r['rounds']} ({r['rounds'] / n:.1f} L) bids {r['bids']} P-OPT {r['P'] - opt} P-D {r['P'] - r['D']}")
    assert sorted(r["match12"].tolist()) == list(range(n))
    assert np.array_equal(r["match21"][r["match12"]], np.arange(n))
    if family == "identical":
        assert r["rounds"] == 7  # one round per phase: the rotating tie rule


def test_ea_ref_ragged_counts_ignore_the_padding():
    a, c = ea_family("uniform", 40, 5)
    full = ea_ref(a[:23].copy(), c[:23].copy())
    a[23:], c[23:] = np.nan, 7e30
    r = ea_ref(a, c, L=23)
    for key in ("P", "D", "k", "rounds", "bids", "status"):
        assert r[key] == full[key]
    assert np.array_equal(r["match12"][:23], full["match12"]) and not r["match12"][23:].any() and not r["dist"][23:].any()


def test_ea_ref_by_hand():
    """Persons (0,0,0), (1,0,0); objects (.25,0,0), (2,0,0).  E = 2 = 0.5 * 2^2: k = 17, c = [[2^15, 2^18], [3 * 2^15, 2^17]].
    Phase 1 (eps 2^17), round 1: person 0 bids 0 + (2^18 - 2^15) + 2^17 = 360448 for object 0, person 1 bids
    0 + (2^17 - 3 * 2^15) + 2^17 = 163840 for it too; person 0 wins.  Round 2: person 1 sees v = (98304 + 360448, 2^17),
    bids 0 + (458752 - 131072) + 131072 = 458752 for object 1.  Every later phase repeats the pattern: 14 rounds, 21 bids."""
    a = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    c = np.array([[0.25, 0, 0], [2, 0, 0]], np.float32)
    first = ea_ref(a, c, max_rounds=2)
    assert first["status"] == EA_CAPPED and first["prices"].tolist() == [360448, 458752] and first["bids"] == 3
    r = ea_ref(a, c)
    assert r["k"] == 17 and r["status"] == EA_OK and (r["rounds"], r["bids"]) == (14, 21)
    assert r["match12"].tolist() == [0, 1] and r["match21"].tolist() == [0, 1]
    assert r["dist"].tolist() == [0.25, 1.0] and r["cost"] == 1.25
    assert r["P"] == (1 << 15) + (1 << 17) and r["P"] - 2 <= r["D"] <= r["P"]
    assert r["gap"] == np.float32((r["P"] - r["D"]) / 2.0 ** 17) and r["bound"] == np.float32((r["P"] - r["D"] + 2) / 2.0 ** 17)
    # one point: one round per phase, the price rises by eps each time
    one = ea_ref(a[:1], c[:1])
    assert one["k"] == 20  # E = 0.25 = 0.5 * 2^-1
    assert (one["rounds"], one["bids"], one["P"], one["D"]) == (7, 7, 1 << 18, 1 << 18) and one["prices"].tolist() == [sum(EPS)]


@pytest.mark.parametrize("family", ["uniform", "dup_both", "lattice"])
def test_ea_ref_capped_is_a_permutation_with_a_valid_certificate(family):
    n = 65
    a, c = ea_family(family, n, 9)
    r = ea_ref(a, c, max_rounds=5)
    assert r["status"] == EA_CAPPED and r["rounds"] == 5
    assert sorted(r["match12"].tolist()) == list(range(n)) and np.array_equal(r["match21"][r["match12"]], np.arange(n))
    check_certificate(r, a, c, n)


def test_ea_ref_nonfinite_is_reported():
    a, c = ea_family("uniform", 8, 1)
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[3, 1] = bad
        r = ea_ref(x, c)
        assert r["status"] == EA_NONFINITE and r["match12"].tolist() == list(range(8))
    r = ea_ref(a * np.float32(3e38), -c * np.float32(3e38))  # finite coordinates, an extent that overflows
    assert r["status"] == EA_NONFINITE


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_emd_assign", "rf_emd_assign_grad", "rf_emd_assign_workspace_bytes", "rf_emd_assign_supported")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    assert f"#define RF_EA_MAX_POINTS {_raw.EA_MAX_POINTS}\n" in header and _raw.EA_MAX_POINTS == 4096
    for name, v in (("OK", _raw.EA_OK), ("CAPPED", _raw.EA_CAPPED), ("NONFINITE", _raw.EA_NONFINITE)):
        assert f"#define RF_EA_{name} {v}\n" in header
    assert (_raw.EA_OK, _raw.EA_CAPPED, _raw.EA_NONFINITE) == (EA_OK, EA_CAPPED, EA_NONFINITE)
    src = open(_lib._PKG + "/csrc/emd_assign.hip").read()  # the tiles the GPU tests place their shapes by
    assert f"constexpr int EA_TPB = {_raw.EA_TPB};" in src and _raw.EA_WAVE == 64


def test_workspace_size_and_supported():
    from rfnet_amd._lib import lib
    fn = lib.rf_emd_assign_workspace_bytes
    for shape in ((0, 10), (-1, 10), (2, 0), (2, -5), (2, 4097), (65536, 10)):
        assert fn(*shape) == 0, shape
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for b, n in ((1, 1), (3, 257), (32, 2048), (65535, 4096)):
        assert fn(b, n) == r(4 * b * n), (b, n)  # the final prices: nothing of size n^2
    sup = lib.rf_emd_assign_supported
    assert sup(4096) == 1 and sup(4097) == 0 and sup(1) == 1 and sup(0) == 0 and sup(-3) == 0


P, WS, BIG = 0x10000, 0x200000, 1 << 40  # never dereferenced: every call below must return at its argument checks


def _call(b=2, n=300, ln=P, mr=0, ws=WS, wsz=BIG, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 8  # xyz1, xyz2, match12, match21, dist, val, cert, info
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_emd_assign(b, n, t[0], t[1], ln, mr, t[2], t[3], t[4], t[5], t[6], t[7], ws, wsz, None)


def _call_grad(b=2, n=300, ln=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 7  # xyz1, xyz2, match12, match21, gcost, grad1, grad2
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_emd_assign_grad(b, n, t[0], t[1], t[2], t[3], ln, t[4], t[5], t[6], None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    assert _call(b=0) == OK and _call(b=0, n=0, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(b=0, n=-1), dict(n=0), dict(n=4097), dict(b=65536), dict(mr=-1)):
        assert _call(**bad) == EINVAL, bad
    for k in range(8):
        assert _call(null=k) == EINVAL, f"NULL tensor {k}"
        assert _call(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _call(at=(6, P + 4)) == EINVAL  # cert: 8 bytes
    assert _call(ln=P + 2) == EINVAL  # the count array: 4 bytes
    assert _call(ws=None) == EINVAL
    assert _call(ws=WS + 4) == EINVAL and _call(ws=WS + 8) == EINVAL  # workspace: 16 bytes
    need = lib.rf_emd_assign_workspace_bytes(2, 300)
    assert _call(wsz=need - 1) == EWORKSPACE and _call(wsz=0) == EWORKSPACE
    # NULL counts mean "all", and the largest sizes are sizes: neither is the error here
    assert _call(wsz=0, ln=None) == EWORKSPACE
    assert _call(b=65535, n=4096, mr=(1 << 31) - 1, wsz=0) == EWORKSPACE
    # the gradient entry
    assert _call_grad(b=0) == OK and _call_grad(b=0, n=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(b=0, n=-1), dict(n=0), dict(n=4097), dict(b=65536)):
        assert _call_grad(**bad) == EINVAL, bad
    for k in range(7):
        assert _call_grad(null=k) == EINVAL, f"NULL tensor {k}"
        assert _call_grad(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _call_grad(ln=P + 1) == EINVAL


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, c = np.zeros((2, 4, 3), np.float32), np.zeros((2, 4, 3), np.float32)
    for fn, more in ((_raw.emd_assign, ()), (_raw.emd_assign_grad, (np.zeros((2, 4), np.int32),) * 2 + (np.ones(2, np.float32),))):
        with pytest.raises(ValueError, match="xyz1"):
            fn(np.zeros((2, 4), np.float32), c, *more)
        with pytest.raises(ValueError, match="xyz2"):
            fn(a, np.zeros((2, 4, 2), np.float32), *more)
        with pytest.raises(ValueError, match="batch"):
            fn(a, np.zeros((3, 4, 3), np.float32), *more)
        with pytest.raises(ValueError, match="same number of points"):
            fn(a, np.zeros((2, 5, 3), np.float32), *more)
        with pytest.raises(ValueError, match="at least one point"):
            fn(np.zeros((2, 0, 3), np.float32), np.zeros((2, 0, 3), np.float32), *more)
        with pytest.raises(ValueError, match="4096"):
            fn(np.zeros((1, 4097, 3), np.float32), np.zeros((1, 4097, 3), np.float32), *more)
        with pytest.raises(ValueError, match="lengths"):
            fn(a, c, *more, lengths=[4, 5])
    with pytest.raises(ValueError, match="max_rounds"):
        _raw.emd_assign(a, c, max_rounds=-1)
    with pytest.raises(ValueError, match="match12"):
        _raw.emd_assign_grad(a, c, np.zeros((2, 5), np.int32), np.zeros((2, 4), np.int32), np.ones(2, np.float32))
    with pytest.raises(ValueError, match="grad_cost"):
        _raw.emd_assign_grad(a, c, np.zeros((2, 4), np.int32), np.zeros((2, 4), np.int32), np.ones(3, np.float32))
    with pytest.raises(ValueError, match="same number of points"):
        glue.emd_assignment(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="xyz1"):
        glue.emd_exact(torch.zeros(2, 4), torch.zeros(2, 4, 3))
