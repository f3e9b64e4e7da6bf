"""CPU: the Sinkhorn divergence entry (include/rfops.h, "the Sinkhorn divergence of two clouds") at the boundary -- declared,
exported, bound; the workspace size; every argument rule answered before a device is touched; the wrappers' checks; the
host schedule -- and sk_ref, the numpy restatement of the contract that the GPU tests hold the kernels to, pinned here by
independent means: a case by hand, the self distance, central differences of the converged loss, ragged counts, and a case
in which the unstabilised sum underflows."""
import ctypes

import numpy as np
import pytest
import torch


# ---- the reference ------------------------------------------------------------------------------------------------------
def _cost(x, y, p):
    d = x[:, None, :] - y[None, :, :]
    d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    return np.sqrt(d2) if p == 1 else d2 * x.dtype.type(0.5)


def _softmin(C, h, w, e):
    """-e log sum_j w exp((h_j - C_ij) / e), the row maximum subtracted"""
    z = (h[None, :] - C) / e
    mx = z.max(1)
    return -e * (mx + np.log((w * np.exp(z - mx[:, None])).sum(1)))


def _plan_grad(x, y, C, f1, h, w, e, p):
    """sum_j pi_ij d1C(x_i, y_j),  pi_ij = w exp((f1_i + h_j - C_ij) / e)"""
    pi = w * np.exp((f1[:, None] + h[None, :] - C) / e)
    d = x[:, None, :] - y[None, :, :]
    if p == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(C[..., None] > 0, d / C[..., None], x.dtype.type(0))
    return (pi[..., None] * d).sum(1)


def sk_ref(a, c, eps, p=1, L1=None, L2=None, dtype=np.float64):
    """a (n, 3), c (m, 3); the first L1 / L2 rows are the clouds; eps the schedule -> (loss, pot (n + m), delta, grad_a
    (n, 3), grad_c (m, 3)): include/rfops.h's definitions word for word, every operation in `dtype` (the loss sum in
    float64 either way).  The four problems run through the same functions on contiguous arrays, so sk_ref(x, x) is 0."""
    dt = np.dtype(dtype).type
    n, m = np.shape(a)[0], np.shape(c)[0]
    L1 = n if L1 is None else int(L1)
    L2 = m if L2 is None else int(L2)
    x, y = np.ascontiguousarray(np.asarray(a)[:L1], dtype), np.ascontiguousarray(np.asarray(c)[:L2], dtype)
    wa, wb = dt(1) / dt(L1), dt(1) / dt(L2)
    Cxy = _cost(x, y, p)
    Cyx, Cxx, Cyy = np.ascontiguousarray(Cxy.T), _cost(x, x, p), _cost(y, y, p)
    f, g, fx, gy = (np.zeros(k, dtype) for k in (L1, L2, L1, L2))
    half = dt(0.5)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for e in eps:
            e = dt(e)
            f, g, fx, gy = (half * (f + _softmin(Cxy, g, wb, e)), half * (g + _softmin(Cyx, f, wa, e)),
                            half * (fx + _softmin(Cxx, fx, wa, e)), half * (gy + _softmin(Cyy, gy, wb, e)))
        e = dt(eps[-1])
        f1, g1 = _softmin(Cxy, g, wb, e), _softmin(Cyx, f, wa, e)
        fx1, gy1 = _softmin(Cxx, fx, wa, e), _softmin(Cyy, gy, wb, e)
        loss = ((f1.astype(np.float64) - fx1.astype(np.float64)).sum() / L1
                + (g1.astype(np.float64) - gy1.astype(np.float64)).sum() / L2)
        delta = max(np.abs(f1 - f).max(), np.abs(g1 - g).max())
        g_a, g_c = np.zeros((n, 3), dtype), np.zeros((m, 3), dtype)
        g_a[:L1] = wa * (_plan_grad(x, y, Cxy, f1, g, wb, e, p) - _plan_grad(x, x, Cxx, fx1, fx, wa, e, p))
        g_c[:L2] = wb * (_plan_grad(y, x, Cyx, g1, f, wa, e, p) - _plan_grad(y, y, Cyy, gy1, gy, wb, e, p))
    pot = np.zeros(n + m, dtype)
    pot[:L1], pot[n:n + L2] = f1, g1
    return float(loss), pot, float(delta), g_a, g_c


def clouds(seed, n, m, shift=0.0):
    """Two clouds inside the unit ball (the schedule's default diameter): uniform in cubes of edge 1 and 0.9."""
    rng = np.random.RandomState(seed)
    a = (rng.rand(n, 3) - 0.5).astype(np.float32)
    c = ((rng.rand(m, 3) - 0.5) * 0.9 + shift).astype(np.float32)
    return a, c


def schedule(*args, **kw):
    from rfnet_amd import glue
    return glue.sinkhorn_schedule(*args, **kw)


# ---- sk_ref, pinned ------------------------------------------------------------------------------------------------------
def test_schedule():
    assert schedule(1, 0.05, 0.5) == [2.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 0.05]
    assert len(schedule(2, 0.05, 0.5)) == 7 and schedule(2, 0.05, 0.5)[0] == 4.0 and schedule(2, 0.05, 0.5)[-1] == 0.05 ** 2
    assert len(schedule(1, 0.01, 0.7)) == 16 and len(schedule(2, 0.01, 0.7)) == 16
    e = schedule(1, 0.3, 0.5, 2.0, extra=3)
    assert e == [2.0, 1.0, 0.5, 0.3, 0.3, 0.3, 0.3]
    assert schedule(1, 5.0) == [5.0]  # a blur above the diameter: the steps at blur alone
    for bad in (dict(p=3), dict(blur=0.0), dict(scaling=1.0), dict(scaling=0.0), dict(diameter=-1.0), dict(extra=-1)):
        with pytest.raises(ValueError):
            schedule(**bad)


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_sk_ref_by_hand(p, T):
    """n = m = 1: f + g = C after the first step, the self potentials stay 0, so the loss is C(x, y) whatever the schedule."""
    x, y = np.array([[0.25, -0.5, 1.0]]), np.array([[-0.5, 0.5, 0.0]])
    d = x[0] - y[0]
    C = np.sqrt(d @ d) if p == 1 else 0.5 * (d @ d)
    loss, pot, delta, g1, g2 = sk_ref(x, y, [1.0, 0.5, 0.25, 0.1, 0.1][:T], p)
    assert abs(loss - C) <= 4 * 2.0 ** -53 * C and np.abs(pot - C / 2).max() <= 4 * 2.0 ** -53 * C
    unit = d / np.sqrt(d @ d) if p == 1 else d
    assert np.abs(g1[0] - unit).max() <= 1e-15 and np.abs(g2[0] + unit).max() <= 1e-15


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("p", [1, 2])
def test_sk_ref_self_distance_is_zero(p, dtype):
    x, _ = clouds(4, 70, 1)
    loss, pot, delta, g1, g2 = sk_ref(x, x, schedule(p, 0.05, 0.5), p, dtype=dtype)
    assert loss == 0.0 and not g1.any() and not g2.any()
    assert pot[:70].tobytes() == pot[70:].tobytes() and np.abs(pot).max() > 0


@pytest.mark.parametrize("p", [1, 2])
def test_sk_ref_gradients_against_central_differences(p):
    """At convergence the potentials are stationary, so the derivative of the loss through them vanishes (the envelope
    argument) and the gradient through the final step alone is the whole gradient."""
    rng = np.random.RandomState(11)
    a, c = rng.rand(12, 3) - 0.5, rng.rand(9, 3) - 0.5
    L1, L2, h = 10, 9, 1e-6
    eps = schedule(p, 0.3, 0.5, 2.0, extra=300)
    loss, pot, delta, g1, g2 = sk_ref(a, c, eps, p, L1, L2)
    assert delta <= 1e-14, delta
    worst = 0.0
    for x, g, L, which in ((a, g1, L1, 0), (c, g2, L2, 1)):
        for k in range(L):
            for ax in range(3):
                hi, lo = x.copy(), x.copy()
                hi[k, ax] += h
                lo[k, ax] -= h
                up = sk_ref(hi, c, eps, p, L1, L2)[0] if which == 0 else sk_ref(a, hi, eps, p, L1, L2)[0]
                dn = sk_ref(lo, c, eps, p, L1, L2)[0] if which == 0 else sk_ref(a, lo, eps, p, L1, L2)[0]
                worst = max(worst, abs((up - dn) / (2 * h) - g[k, ax]))
    print(f"p = {p}: delta {delta:.3e}, worst |central difference - gradient| {worst:.3e}")
    assert worst <= 1e-9
    assert not g1[L1:].any() and g1[:L1].any() and g2.any()


@pytest.mark.parametrize("p", [1, 2])
def test_sk_ref_ignores_rows_behind_the_counts(p):
    a, c = clouds(5, 40, 33)
    eps = schedule(p, 0.05, 0.5)
    L1, L2 = 17, 29
    exp = sk_ref(a[:L1], c[:L2], eps, p)
    a2, c2 = a.copy(), c.copy()
    a2[L1:], c2[L2:] = np.nan, np.inf
    got = sk_ref(a2, c2, eps, p, L1, L2)
    assert got[0] == exp[0] and got[2] == exp[2]
    assert got[1][:L1].tobytes() == exp[1][:L1].tobytes() and got[1][40:40 + L2].tobytes() == exp[1][L1:].tobytes()
    assert not got[1][L1:40].any() and not got[1][40 + L2:].any()
    assert got[3][:L1].tobytes() == exp[3].tobytes() and got[4][:L2].tobytes() == exp[4].tobytes()
    assert not got[3][L1:].any() and not got[4][L2:].any()  # exactly 0 behind the counts


STAB_EPS = [4.0, 1.0, 1e-2, 1e-4, 1e-4]


def stab_clouds():
    return clouds(8, 65, 70, shift=3.0)


@pytest.mark.parametrize("p", [1, 2])
def test_sk_ref_is_stabilised(p):
    a, c = stab_clouds()
    x, y = a.astype(np.float64), c.astype(np.float64)
    # without the maximum every term of the cross sum underflows at eps = 1e-4: the soft-min would be +inf
    assert (np.exp((0.0 - _cost(x, y, p)) / 1e-4) == 0.0).all()
    for dtype in (np.float64, np.float32):
        loss, pot, delta, g1, g2 = sk_ref(a, c, STAB_EPS, p, dtype=dtype)
        assert np.isfinite(loss) and np.isfinite(pot).all() and np.isfinite(delta)
        assert np.isfinite(g1).all() and np.isfinite(g2).all() and loss > 0


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ("rf_sinkhorn", "rf_sinkhorn_workspace_bytes"):
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    assert f"#define RF_SK_MAX_POINTS {_raw.SK_MAX_POINTS}\n" in header and _raw.SK_MAX_POINTS == 65536
    assert f"#define RF_SK_MAX_ITERS {_raw.SK_MAX_ITERS}\n" in header and _raw.SK_MAX_ITERS == 256


def test_workspace_size():
    from rfnet_amd._lib import lib
    fn = lib.rf_sinkhorn_workspace_bytes
    for shape in ((0, 10, 10), (-1, 10, 10), (2, 0, 10), (2, 10, 0), (2, -5, 10), (2, 10, -5), (2, 65537, 10),
                  (2, 10, 65537), (65536, 10, 10)):
        assert fn(*shape) == 0, shape
    for b, n, m in ((1, 1, 1), (3, 300, 200), (32, 2048, 16384), (65535, 65536, 65536)):
        assert fn(b, n, m) > 0, (b, n, m)
    # the formula of the header, each part rounded up to 256 bytes
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    b, n, m = 3, 300, 203
    rows = 2 * b * (n + m)
    assert fn(b, n, m) == 2 * r(4 * rows) + 2 * r(32 * rows) + r(48 * rows)
    assert fn(65535, 65536, 65536) == 2 * r(4 * 65535 * 2 ** 18) + 2 * r(32 * 65535 * 2 ** 18) + r(48 * 65535 * 2 ** 18)


P, WS, BIG = 0x10000, 0x200000, 1 << 60  # never dereferenced: every call below must return at its argument checks


def _call(b=2, n=300, m=200, p=1, eps=(1.0, 0.5), T=None, ws=WS, wsz=BIG, l1=P, l2=P, g1=P, g2=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 5  # xyz1, xyz2, loss, pot, delta
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    arr = None if eps is None else (ctypes.c_float * max(len(eps), 1))(*eps)  # a HOST array: this one is read
    T = (0 if eps is None else len(eps)) if T is None else T
    return lib.rf_sinkhorn(b, n, m, t[0], t[1], l1, l2, p, arr, T, t[2], t[3], t[4], g1, g2, ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    assert _call(b=0) == OK
    assert _call(b=0, n=0, m=0, eps=None, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(m=-3), dict(b=0, n=-1), dict(n=0), dict(m=0), dict(n=65537), dict(m=65537),
                dict(b=65536), dict(p=0), dict(p=3), dict(p=-1), dict(T=0), dict(T=-1), dict(eps=None, T=2),
                dict(eps=(1.0,) * 257), dict(eps=(1.0, 0.0)), dict(eps=(-1.0, 1.0)), dict(eps=(1.0, float("nan"))),
                dict(eps=(float("inf"),))):
        assert _call(**bad) == EINVAL, bad
    for k in range(5):
        assert _call(null=k) == EINVAL, f"NULL tensor {k}"
        assert _call(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _call(g1=None) == EINVAL and _call(g2=None) == EINVAL  # both gradients or neither
    assert _call(g1=P + 2) == EINVAL and _call(g2=P + 1) == EINVAL
    assert _call(l1=P + 2) == EINVAL and _call(l2=P + 1) == EINVAL  # count arrays: 4 bytes
    assert _call(ws=None) == EINVAL
    assert _call(ws=WS + 4) == EINVAL and _call(ws=WS + 8) == EINVAL  # workspace: 16 bytes
    need = lib.rf_sinkhorn_workspace_bytes(2, 300, 200)
    assert _call(wsz=need - 1) == EWORKSPACE and _call(wsz=0) == EWORKSPACE
    assert _call(g1=None, g2=None, wsz=need - 1) == EWORKSPACE
    # NULL counts mean "all", and the largest sizes are sizes: neither is the error here
    assert _call(wsz=0, l1=None, l2=None) == EWORKSPACE
    assert _call(b=65535, n=65536, m=65536, p=2, eps=(1e-30,) * 256, wsz=0) == EWORKSPACE


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, c, e = np.zeros((2, 4, 3), np.float32), np.zeros((2, 5, 3), np.float32), [1.0, 0.5]
    with pytest.raises(ValueError, match="xyz1"):
        _raw.sinkhorn(np.zeros((2, 4), np.float32), c, e)
    with pytest.raises(ValueError, match="xyz2"):
        _raw.sinkhorn(a, np.zeros((2, 5, 2), np.float32), e)
    with pytest.raises(ValueError, match="batch"):
        _raw.sinkhorn(a, np.zeros((3, 5, 3), np.float32), e)
    with pytest.raises(ValueError, match="p be 1 or 2"):
        _raw.sinkhorn(a, c, e, p=3)
    for bad in ([], [1.0] * 257):
        with pytest.raises(ValueError, match="1 to 256 steps"):
            _raw.sinkhorn(a, c, bad)
    for bad in ([1.0, 0.0], [-1.0], [float("nan")], [float("inf")], [1e-60]):
        with pytest.raises(ValueError, match="positive and finite"):
            _raw.sinkhorn(a, c, bad)
    with pytest.raises(ValueError, match="at least one point"):
        _raw.sinkhorn(np.zeros((2, 0, 3), np.float32), c, e)
    with pytest.raises(ValueError, match="65536"):
        _raw.sinkhorn(np.zeros((1, 65537, 3), np.float32), np.zeros((1, 5, 3), np.float32), e)
    with pytest.raises(ValueError, match="lengths1"):
        _raw.sinkhorn(a, c, e, lengths1=[4, 5])
    with pytest.raises(ValueError, match="lengths2"):
        _raw.sinkhorn(a, c, e, lengths2=[5])
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        glue.sinkhorn_divergence(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3), p=0)
    with pytest.raises(ValueError, match="positive and finite"):
        glue.sinkhorn_divergence(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3), eps=[0.0])
