"""CPU: the contract of rf_knn_feature (include/rfops.h) restated in numpy, and its C ABI.

`fma32` is an exact fp32 fused multiply-add in numpy: the float64 product of two float32 values is exact; the addend is added in
float64, the addition's error recovered with TwoSum, and where the sum is inexact and the float64 result's last bit is even it is
stepped one ulp towards the error (round to odd) before the rounding to float32 -- the plain float32(float64(a) * b + c) rounds
twice.  It is held to `fractions.Fraction` here.  `knn_feature_ref` is the header's contract on top of it (the channel chain,
the odd channel's padding step, d = fma(-2, ip, sq2 + sq1), the (d, index) order with NaN first, the ragged rule) and is held to
an int64 brute force on integer-valued inputs, where every quantity is exact.  tests/test_gpu_knn_feature.py compares the
kernels with it bit for bit.  The ABI checks run without a device: every argument error is answered before any HIP call."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------ fma32 ----
def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding, elementwise with broadcasting."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)  # exact: 48 significant bits, exponents inside float64's
        c64 = c.astype(F64)
        s = p + c64
        bb = s - p  # TwoSum: s + err == p + c64 exactly
        err = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(p) & np.isfinite(c64) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)  # round to odd
        return s.astype(F32)


def _round_f32(fr):
    """the float32 nearest to a rational, ties to even (overflow: inf)"""
    if fr == 0:
        return F32(0)
    sign, mag = (-1 if fr < 0 else 1), abs(fr)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = mag / quantum
    nint = q.numerator // q.denominator
    rem = q - nint
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and nint & 1):
        nint += 1
    v = nint * quantum
    if v >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(v))  # exact: at most 24 significant bits


def _bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


ADVERSARIAL = (F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -12 * (1 - 2.0 ** -23)), F32(1 + 2.0 ** -23))


def test_fma32_is_the_exact_fma():
    rng = np.random.default_rng(11)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F32)
    c[: n // 4] = (-(a[: n // 4].astype(F64) * b[: n // 4])).astype(F32)  # cancellation
    a[-50:] *= F32(2.0 ** -70)  # results among the float32 subnormals
    b[-50:] *= F32(2.0 ** -60)
    c[-50:] *= F32(2.0 ** -130)
    got = fma32(a, b, c)
    for i in range(n):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert _bits(got[i]) == _bits(want), (a[i], b[i], c[i])


def test_fma32_on_the_double_rounding_triple():
    a, b, c = ADVERSARIAL
    for sgn, right, naive in ((1, 0x3F800001, 0x3F800002), (-1, 0xBF800001, 0xBF800002)):
        bb, cc = F32(sgn) * b, F32(sgn) * c
        assert _bits(fma32(a, bb, cc)) == right
        assert _bits(_round_f32(Fraction(float(a)) * Fraction(float(bb)) + Fraction(float(cc)))) == right
        assert _bits(F32(F64(a) * F64(bb) + F64(cc))) == naive  # what rounding twice gives


def test_fma32_non_finite_and_zeros():
    inf, nan = F32(np.inf), F32(np.nan)
    assert np.isnan(fma32(inf, 0, 1)) and np.isnan(fma32(inf, 1, -inf)) and np.isnan(fma32(nan, 1, 1))
    assert fma32(inf, 2, 1) == inf and fma32(F32(3e38), 2, 0) == inf
    assert _bits(fma32(0, 0, F32(-0.0))) == 0  # the padding step turns -0 into +0
    assert _bits(fma32(F32(1e-30), F32(-1e-30), 0)) == 0x80000000


# ------------------------------------------------------------------------- the restatement ----
def feature_distances(f1, f2):
    """d (m, n) float32 of one sample by the contract's chain: f1 (n, c) candidates, f2 (m, c) queries."""
    f1, f2 = np.asarray(f1, F32), np.asarray(f2, F32)
    c = f1.shape[1]
    ip = np.zeros((f2.shape[0], f1.shape[0]), F32)
    sq1, sq2 = np.zeros(f1.shape[0], F32), np.zeros(f2.shape[0], F32)
    for ch in range(c):
        ip = fma32(f2[:, ch, None], f1[None, :, ch], ip)
        sq1 = fma32(f1[:, ch], f1[:, ch], sq1)
        sq2 = fma32(f2[:, ch], f2[:, ch], sq2)
    if c & 1:
        ip = fma32(0, 0, ip)  # the channel padded up to the matrix instruction's K
    with np.errstate(all="ignore"):
        return fma32(F32(-2), ip, sq2[:, None] + sq1[None, :])


def knn_feature_ref(k, f1, f2, len1=None, len2=None):
    """-> val (b, m, k) float32, idx (b, m, k) int32: rf_knn_feature's contract."""
    f1, f2 = np.asarray(f1, F32), np.asarray(f2, F32)
    b, n, m = f1.shape[0], f1.shape[1], f2.shape[1]
    val, idx = np.zeros((b, m, k), F32), np.zeros((b, m, k), np.int32)
    for s in range(b):
        nv = n if len1 is None else int(np.clip(len1[s], 1, n))
        mv = m if len2 is None else int(np.clip(len2[s], 1, m))
        kv = min(k, nv)
        d = feature_distances(f1[s, :nv], f2[s, :mv])
        isnan = np.isnan(d)
        dd = np.where(isnan, F32(-np.inf), d + F32(0))  # (-0 as +0)
        cols = np.broadcast_to(np.arange(nv), d.shape)
        for j in range(mv):
            order = np.lexsort((cols[j], dd[j], ~isnan[j]))[:kv]  # NaN first, then d, then the index
            v = -dd[j, order]
            v[isnan[j, order]] = np.uint32(0xFFC00000).view(F32)
            val[s, j, :kv], idx[s, j, :kv] = v, order
    return val, idx


def brute_int(k, f1, f2):
    """integer-valued inputs: exact int64 squared distances, lexicographic (d, i)"""
    a, q = np.asarray(f1).astype(np.int64), np.asarray(f2).astype(np.int64)
    d = ((q[:, :, None, :] - a[:, None, :, :]) ** 2).sum(-1)
    key = d * (1 << 20) + np.arange(a.shape[1])[None, None, :]
    idx = np.argsort(key, axis=-1, kind="stable")[..., :k]
    return -np.take_along_axis(d, idx, -1).astype(F32), idx.astype(np.int32)  # (val = -d: -0.0 for a zero distance)


def int_features(seed, b, n, c, hi=8):
    return np.random.default_rng(seed).integers(-hi, hi + 1, (b, n, c)).astype(F32)


@pytest.mark.parametrize("c", [1, 2, 5, 64, 130])
def test_restatement_is_the_brute_force_on_integers(c):
    f1, f2 = int_features(c, 2, 60, c, hi=8 if c > 2 else 2), int_features(100 + c, 2, 23, c, hi=8 if c > 2 else 2)
    f2[:, :10] = f1[:, 5:15]  # exact duplicates: zero distances and ties
    k = 13
    val, idx = knn_feature_ref(k, f1, f2)
    bv, bi = brute_int(k, f1, f2)
    assert np.array_equal(idx, bi) and val.tobytes() == bv.tobytes()
    ties = sum(len(np.unique(row)) < k for row in val.reshape(-1, k))
    assert ties > 0, "the case must hold ties"


def test_restatement_ragged_and_non_finite():
    f1, f2 = int_features(1, 3, 9, 4), int_features(2, 3, 5, 4)
    f1[0, 4:] = np.nan
    f2[1, 2:] = np.nan
    val, idx = knn_feature_ref(6, f1, f2, [4, 9, 1], [5, 2, 5])
    v0, i0 = knn_feature_ref(4, f1[:1, :4], f2[:1])
    assert np.array_equal(idx[0, :, :4], i0[0]) and not idx[0, :, 4:].any() and not val[0, :, 4:].view(np.uint32).any()
    assert not idx[1, 2:].any() and not val[1, 2:].view(np.uint32).any()
    assert not idx[2].any() and not val[2, :, 1:].view(np.uint32).any()
    f1 = int_features(3, 1, 6, 3)
    f1[0, 4] = np.nan
    f1[0, 2, 0] = np.inf
    val, idx = knn_feature_ref(6, f1, np.array([[[1, 0, 0], [0, 1, 1]]], F32))
    assert (idx[0, :, 0] == 2).all() and (val[0, :, 0].view(np.uint32) == 0xFFC00000).all()  # inf - 2 inf and 0 inf: NaN, as -NaN
    assert (idx[0, :, 1] == 4).all() and (val[0, :, 1].view(np.uint32) == 0xFFC00000).all()  # NaN first, the lower index ahead
    assert np.isfinite(val[0, :, 2:]).all()
    f1 = np.zeros((1, 3, 2), F32)
    f1[0, 0, 0], f1[0, 1, 0] = 1.5e19, -1.5e19  # |x|^2 finite, its sum with |q|^2 overflows: d = +inf, after the finite one
    f2 = np.zeros((1, 1, 2), F32)
    f2[0, 0, 0] = 1.5e19
    val, idx = knn_feature_ref(3, f1, f2)
    assert idx[0, 0].tolist() == [2, 0, 1] and np.isneginf(val[0, 0, 1:]).all()


# --------------------------------------------------------------------------------- the ABI ----
@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer
BAD = [(0, 10, 10, 8, 2), (65536, 10, 10, 8, 2), (-1, 10, 10, 8, 2), (2, 0, 10, 8, 1), (2, 65537, 10, 8, 2), (2, 10, 0, 8, 2),
       (2, 10, 65537, 8, 2), (2, 10, 10, 0, 2), (2, 10, 10, 2049, 2), (2, 10, 10, 8, 0), (2, 10, 10, 8, 11), (2, 100, 10, 8, 65),
       (2, 10, 10, 8, -3)]
GOOD = [(1, 1, 1, 1, 1), (32, 2048, 2048, 64, 20), (1, 65536, 65536, 2048, 64), (65535, 4, 4, 3, 4)]


def test_symbols_exported(lib):
    from rfnet_amd import _lib
    for name in ("rf_knn_feature_workspace_bytes", "rf_knn_feature"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_workspace_is_zero_exactly_outside_the_domain(lib):
    for t in BAD:
        assert lib.rf_knn_feature_workspace_bytes(*t) == 0, t
    for b, n, m, c, k in GOOD:
        w = lib.rf_knn_feature_workspace_bytes(b, n, m, c, k)
        assert w >= 4 * b * (n + m) and w % 16 == 0, (b, n, m, c, k)


@pytest.mark.parametrize("b,n,m,c,k", BAD)
def test_out_of_domain_is_einval(lib, b, n, m, c, k):
    assert lib.rf_knn_feature(b, n, m, c, k, P, P, None, None, P, P, P, 1 << 40, None) == RF_EINVAL


def test_pointers_alignment_and_workspace(lib):
    b, n, m, c, k = 2, 500, 300, 33, 16
    ws = 1 << 20
    need = lib.rf_knn_feature_workspace_bytes(b, n, m, c, k)
    assert need > 0
    args = [P, P, None, None, P, P]
    for hole in (0, 1, 4, 5):  # a NULL tensor
        a = list(args)
        a[hole] = None
        assert lib.rf_knn_feature(b, n, m, c, k, *a, ws, need, None) == RF_EINVAL
    for hole in range(6):  # a tensor or count array off the 4-byte grid
        a = list(args)
        a[hole] = (1 << 20) + 2
        assert lib.rf_knn_feature(b, n, m, c, k, *a, ws, need, None) == RF_EINVAL
    assert lib.rf_knn_feature(b, n, m, c, k, *args, ws, need - 1, None) == RF_EWORKSPACE
    assert lib.rf_knn_feature(b, n, m, c, k, *args, ws, 0, None) == RF_EWORKSPACE
    assert lib.rf_knn_feature(b, n, m, c, k, *args, ws + 8, need, None) == RF_EINVAL
    assert lib.rf_knn_feature(b, n, m, c, k, *args, None, need, None) == RF_EINVAL


def test_python_wrappers_reject_bad_arguments_before_the_device():
    import torch
    from rfnet_amd import _raw as R
    from rfnet_amd import glue as G
    f1, f2 = torch.zeros(1, 10, 5), torch.zeros(1, 4, 5)
    for fn in (R.knn_feature, G.knn_feature):
        for k in (0, 11, 65):
            with pytest.raises(ValueError):
                fn(k, f1, f2)
        with pytest.raises(ValueError):
            fn(3, f1, torch.zeros(1, 4, 6))  # channels differ
        with pytest.raises(ValueError):
            fn(3, f1, torch.zeros(2, 4, 5))  # batches differ
        with pytest.raises(ValueError):
            fn(3, torch.zeros(10, 5), f2)
        with pytest.raises(ValueError):
            fn(3, torch.zeros(1, 10, 2049), torch.zeros(1, 4, 2049))
        with pytest.raises(ValueError):
            fn(3, f1, f2, lengths1=[11])
        with pytest.raises(ValueError):
            fn(3, f1, f2, lengths2=[0])
        with pytest.raises(ValueError):
            fn(3, f1, f2, lengths1=[1.5])
    with pytest.raises(ValueError):
        G.edge_feature(f2, f1, torch.zeros(1, 4, 3, 2, dtype=torch.int32))  # idx must be (b, m, k)
    with pytest.raises(ValueError):
        G.edge_feature(f2, torch.zeros(1, 10, 6), torch.zeros(1, 4, 3, dtype=torch.int32))
