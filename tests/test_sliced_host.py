"""CPU: the sliced Wasserstein entry (include/rfops.h, "the sliced Wasserstein distance of two clouds") at the boundary --
declared, exported, bound; the workspace size; every argument rule answered before a device is touched; the wrappers'
checks -- and sw_ref, the float64 restatement of the contract that the GPU tests hold the kernels to, checked here
against independent constructions (sorted means, the repeat-to-lcm construction, central differences, a case by hand)."""
import ctypes
import math

import numpy as np
import pytest
import torch


# ---- the reference ------------------------------------------------------------------------------------------------------
def sw_ref(a, c, dirs, L1=None, L2=None):
    """a (n, 3), c (m, 3), dirs (L, 3); the first L1 / L2 rows are the clouds -> (loss, grad_a (n, 3), grad_c (m, 3)) in
    float64.  Per direction: projections, the order by (value, original index), the two-pointer merge of the two quantile
    step functions with INTEGER weights (one division by L1 L2 per sum), the gradients through the fixed permutation."""
    a, c, dirs = np.asarray(a, np.float64), np.asarray(c, np.float64), np.asarray(dirs, np.float64)
    L1 = a.shape[0] if L1 is None else int(L1)
    L2 = c.shape[0] if L2 is None else int(L2)
    loss, g1, g2 = 0.0, np.zeros(a.shape), np.zeros(c.shape)
    for th in dirs:
        p = a[:L1, 2] * th[2] + (a[:L1, 0] * th[0] + a[:L1, 1] * th[1]) + 0.0
        q = c[:L2, 2] * th[2] + (c[:L2, 0] * th[0] + c[:L2, 1] * th[1]) + 0.0
        o1, o2 = np.lexsort((np.arange(L1), p)), np.lexsort((np.arange(L2), q))
        u, v = p[o1], q[o2]
        cost, cu, cv = 0.0, np.zeros(L1), np.zeros(L2)
        i = j = 0
        while i < L1 and j < L2:
            lo, hi = max(i * L2, j * L1), min((i + 1) * L2, (j + 1) * L1)
            d = u[i] - v[j]
            wd = (hi - lo) * d
            cost += wd * d
            cu[i] += wd
            cv[j] -= wd
            ni, nj = (i + 1) * L2 <= hi, (j + 1) * L1 <= hi
            i, j = i + ni, j + nj
        assert i == L1 and j == L2
        den = float(L1 * L2)
        loss += cost / den
        g1[o1] += np.outer(cu / den, th)
        g2[o2] += np.outer(cv / den, th)
    L = len(dirs)
    return loss / L, 2.0 * g1 / L, 2.0 * g2 / L


def exact_inputs(seed, b, n, m, nproj, cgrid=1024, dgrid=256):
    """Inputs whose projections are exact in fp32 (and in any order, fused or not): coordinates multiples of 1 / cgrid in
    [-0.5, 0.5), direction components multiples of 1 / dgrid in [-1, 1]."""
    rng = np.random.RandomState(seed)
    a = (rng.randint(-cgrid // 2, cgrid // 2, (b, n, 3)) / cgrid).astype(np.float32)
    c = (rng.randint(-cgrid // 2, cgrid // 2, (b, m, 3)) / cgrid).astype(np.float32)
    d = (rng.randint(-dgrid, dgrid + 1, (nproj, 3)) / dgrid).astype(np.float32)
    return a, c, d


def test_sw_ref_by_hand():
    a = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    c = [[0.5, 0.0, 0.0]]
    # direction x: u = (0, 1), v = (0.5), both weights 1/2, cost 1/4; direction y: every projection 0
    loss, g1, g2 = sw_ref(a, c, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert loss == 0.125
    assert g1.tolist() == [[-0.25, 0.0, 0.0], [0.25, 0.0, 0.0]] and g2.tolist() == [[0.0, 0.0, 0.0]]
    # ties go to the lower index: both points of a project to 0, c = (-1, 1): point 0 is moved towards -1
    loss, g1, g2 = sw_ref([[0.0, 5.0, 0.0], [0.0, -5.0, 0.0]], [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]])
    assert loss == 1.0 and g1[:, 0].tolist() == [1.0, -1.0] and g2[:, 0].tolist() == [1.0, -1.0]


def test_sw_ref_equal_counts_is_the_mean_of_sorted_differences():
    rng = np.random.RandomState(3)
    n, nproj = 300, 5
    a, c, d = rng.rand(n, 3) - 0.5, rng.rand(n, 3) - 0.5, rng.randn(nproj, 3)
    exp = np.mean([np.mean((np.sort(a @ t) - np.sort(c @ t)) ** 2) for t in d])
    got = sw_ref(a, c, d)[0]
    # two float64 sums of n terms each in different orders, and projections summed in different orders
    assert abs(got - exp) <= 8 * n * 2.0 ** -53 * exp


@pytest.mark.parametrize("L1, L2", [(300, 200), (1, 200), (299, 1), (257, 199), (64, 65)])
def test_sw_ref_unequal_counts_is_the_repeat_to_lcm_construction(L1, L2):
    """On exact inputs every sum is an exact integer multiple of 2^-36 below 2^53 of it: both constructions round once."""
    a, c, d = exact_inputs(L1 * 1000 + L2, 1, 310, 205, 3)
    a, c = a[0].astype(np.float64), c[0].astype(np.float64)
    lcm = L1 * L2 // math.gcd(L1, L2)
    exp = 0.0
    for t in d.astype(np.float64):
        u, v = np.sort(a[:L1] @ t), np.sort(c[:L2] @ t)
        exp += ((np.repeat(u, lcm // L1) - np.repeat(v, lcm // L2)) ** 2).sum() / lcm
    loss, g1, g2 = sw_ref(a, c, d, L1, L2)
    assert loss == exp / len(d)
    assert not g1[L1:].any() and not g2[L2:].any()  # rows behind the counts: exactly 0


def test_sw_ref_gradients_against_central_differences():
    """The loss is piecewise quadratic: away from ties a central difference is exact up to the rounding of the two losses,
    a few 2^-53 * loss / (2 h) < 1e-11 here."""
    rng = np.random.RandomState(11)
    a, c, d = rng.rand(12, 3) - 0.5, rng.rand(9, 3) - 0.5, rng.randn(4, 3)
    L1, L2, h = 10, 9, 1e-5
    _, g1, g2 = sw_ref(a, c, d, L1, L2)
    for x, g, which in ((a, g1, 0), (c, g2, 1)):
        num = np.zeros_like(x)
        for k in range(x.shape[0]):
            for ax in range(3):
                hi, lo = x.copy(), x.copy()
                hi[k, ax] += h
                lo[k, ax] -= h
                args = (lambda y: (y, c)) if which == 0 else (lambda y: (a, y))
                num[k, ax] = (sw_ref(*args(hi), d, L1, L2)[0] - sw_ref(*args(lo), d, L1, L2)[0]) / (2 * h)
        assert np.abs(num - g).max() <= 1e-10, which
    assert not g1[L1:].any() and g1[:L1].any()


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ("rf_sliced_wasserstein", "rf_sliced_wasserstein_workspace_bytes"):
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    assert "#define RF_SW_MAX_POINTS 16384" in header and _raw.SW_MAX_POINTS == 16384
    assert f"#define RF_SW_DIR_CHUNK {_raw.SW_DIR_CHUNK}\n" in header


def test_workspace_size():
    from rfnet_amd._lib import lib
    from rfnet_amd._raw import SW_DIR_CHUNK
    fn = lib.rf_sliced_wasserstein_workspace_bytes
    for shape in ((0, 10, 10, 4), (-1, 10, 10, 4), (2, 0, 10, 4), (2, 10, 0, 4), (2, -5, 10, 4), (2, 10, -5, 4),
                  (2, 10, 10, 0), (2, 10, 10, -1), (2, 16385, 10, 4), (2, 10, 16385, 4), (65536, 10, 10, 4)):
        for g in (0, 1):
            assert fn(*shape, g) == 0, shape
    for b, n, m in ((1, 1, 1), (3, 300, 200), (32, 2048, 2048), (32, 16384, 16384), (65535, 1, 2)):
        for g in (0, 1):
            assert fn(b, n, m, 1, g) > 0, (b, n, m)
            # nothing grows with the number of directions beyond a chunk
            assert fn(b, n, m, 4096, g) == fn(b, n, m, SW_DIR_CHUNK, g) == fn(b, n, m, SW_DIR_CHUNK + 1, g)
            assert fn(b, n, m, 1, g) <= fn(b, n, m, SW_DIR_CHUNK, g)
        assert fn(b, n, m, 128, 0) <= fn(b, n, m, 128, 1)
    # the formula of the header, each part rounded up to 256 bytes
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    b, n, m, c = 3, 300, 200, SW_DIR_CHUNK
    loss_only = 2 * r(4 * c * b * (n + m)) + r(8 * c * b) + r(8 * b)
    assert fn(b, n, m, 100, 0) == loss_only
    assert fn(b, n, m, 100, 1) == loss_only + r(8 * c * b * (n + m)) + r(24 * b * (n + m))


P, WS, BIG = 0x10000, 0x200000, 1 << 40  # never dereferenced: every call below must return at its argument checks


def _call(b=2, n=300, m=200, nproj=7, ws=WS, wsz=BIG, l1=P, l2=P, g1=P, g2=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 4  # xyz1, xyz2, dirs, loss
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_sliced_wasserstein(b, n, m, nproj, t[0], t[1], l1, l2, t[2], t[3], g1, g2, ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    assert _call(b=0) == OK
    assert _call(b=0, n=0, m=0, nproj=0, ws=None, wsz=0) == OK
    for bad in (dict(b=-1), dict(n=-3), dict(m=-3), dict(nproj=-1), dict(b=0, n=-1), dict(b=0, nproj=-2), dict(n=0),
                dict(m=0), dict(nproj=0), dict(n=16385), dict(m=16385), dict(b=65536)):
        assert _call(**bad) == EINVAL, bad
    for k in range(4):
        assert _call(null=k) == EINVAL, f"NULL tensor {k}"
        assert _call(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _call(g1=None) == EINVAL and _call(g2=None) == EINVAL  # both gradients or neither
    assert _call(g1=P + 2) == EINVAL and _call(g2=P + 1) == EINVAL
    assert _call(l1=P + 2) == EINVAL and _call(l2=P + 1) == EINVAL  # count arrays: 4 bytes
    assert _call(ws=None) == EINVAL
    assert _call(ws=WS + 4) == EINVAL and _call(ws=WS + 8) == EINVAL  # workspace: 16 bytes
    need = lib.rf_sliced_wasserstein_workspace_bytes(2, 300, 200, 7, 1)
    assert _call(wsz=need - 1) == EWORKSPACE and _call(wsz=0) == EWORKSPACE
    need0 = lib.rf_sliced_wasserstein_workspace_bytes(2, 300, 200, 7, 0)
    assert _call(g1=None, g2=None, wsz=need0 - 1) == EWORKSPACE
    # NULL counts mean "all", and the largest sizes are sizes: neither is the error here
    assert _call(wsz=0, l1=None, l2=None) == EWORKSPACE
    assert _call(b=65535, n=16384, m=16384, nproj=1 << 20, wsz=0) == EWORKSPACE


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, c, d = np.zeros((2, 4, 3), np.float32), np.zeros((2, 5, 3), np.float32), np.ones((3, 3), np.float32)
    with pytest.raises(ValueError, match="xyz1"):
        _raw.sliced_wasserstein(np.zeros((2, 4), np.float32), c, d)
    with pytest.raises(ValueError, match="xyz2"):
        _raw.sliced_wasserstein(a, np.zeros((2, 5, 2), np.float32), d)
    with pytest.raises(ValueError, match="batch"):
        _raw.sliced_wasserstein(a, np.zeros((3, 5, 3), np.float32), d)
    with pytest.raises(ValueError, match="directions"):
        _raw.sliced_wasserstein(a, c, np.ones((3, 2), np.float32))
    with pytest.raises(ValueError, match="directions"):
        _raw.sliced_wasserstein(a, c, np.ones((0, 3), np.float32))
    with pytest.raises(ValueError, match="at least one point"):
        _raw.sliced_wasserstein(np.zeros((2, 0, 3), np.float32), c, d)
    with pytest.raises(ValueError, match="16384"):
        _raw.sliced_wasserstein(np.zeros((1, 16385, 3), np.float32), np.zeros((1, 5, 3), np.float32), d)
    with pytest.raises(ValueError, match="lengths1"):
        _raw.sliced_wasserstein(a, c, d, lengths1=[4, 5])
    with pytest.raises(ValueError, match="lengths2"):
        _raw.sliced_wasserstein(a, c, d, lengths2=[5])
    with pytest.raises(ValueError, match="nproj"):
        glue.sliced_wasserstein(torch.zeros(2, 4, 3), torch.zeros(2, 5, 3), nproj=0)
