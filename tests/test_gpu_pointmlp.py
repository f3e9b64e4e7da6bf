"""The six entries of rfnet_amd/csrc/pointmlp.hip -- rf_point_affine, rf_maxpool_points, rf_maxpool_points_idx, their two
_lengths forms, rf_act_grad_colsum -- against the float64 references of tests/pointmlp_ref.py (themselves checked on the CPU
by tests/test_pointmlp_host.py) at the smallest shapes that reach every path of their shared indexing: quads = c / 4,
ppi = 256 / quads point-lanes, idle threads where quads does not divide 256, strips of PA_STRIP / MP_STRIP rows, the fold
over point-lanes in LDS and over strips in the second kernel.

Two input families.  A: values on a dyadic grid on which every fp32 operation of the kernel is exact in any order, fused or
not -- the reference proves that (scaled int64, every sum of magnitudes below 2^24) and the comparison is bit for bit, so an
indexing, tail, stride or tie error shows as a wrong bit.  B: randn against float64 under bounds derived from the number of
roundings (pointmlp_ref.py), U = 2^-24.  The one figure that cannot be derived, tanhf's own error, is measured by
test_tanhf_error_against_float64 and recorded in TANHF_ULP.

A shared r of shape (c,) is always handed over as the first row of a (b, c) buffer whose other rows are NaN: a kernel that
strode over a shared row would read them."""
import itertools

import numpy as np
import pytest
import torch

import pointmlp_ref as R

pytestmark = pytest.mark.gpu

K = R.kernel_constants()
PA_STRIP, PA_KMAX, PA_TPB, MP_STRIP, MP_TPB = K["PA_STRIP"], K["PA_KMAX"], K["PA_TPB"], K["MP_STRIP"], K["MP_TPB"]
CS = [4, 12, 20, 128, 256, 260, 512, 516, 1024]  # ppi 256, 85, 51, 8, 4, 3, 2, 1, 1; idle threads 0, 1, 1, 0, 0, 61, 0, 127, 0
C_ALL_KP = 20                                    # the width that runs every kp from 0 to PA_KMAX
AFFINE_NS = [1, PA_STRIP - 1, PA_STRIP, PA_STRIP + 1, 2 * PA_STRIP + 1]
POOL_NS = [1, 2, MP_STRIP - 1, MP_STRIP, MP_STRIP + 1, 2 * MP_STRIP - 1, 2 * MP_STRIP + 1, 3 * MP_STRIP + 1]
RAGGED_N = 600
RAGGED_COUNTS = [1, 255, 256, 257, 512, 600, 0, RAGGED_N + 7]  # the last two only as device counts: held to 1 and n

# tanhf on gfx950 against float64 tanh of the same fp32 argument, worst case over the 65,536 arguments of
# test_tanhf_error_against_float64 (|x| from 1e-6 to 20, both signs, +-inf), in units of the fp32 spacing at the result.
# MEASURED on an MI355X, not derived: 1.262 spacings, at x = -0.6279215.  Only a sample of arguments is seen, so the bar is
# twice the figure.
TANHF_ULP = 1.262


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    """The bit patterns of an fp32 array, the sign of a zero set aside (x + 0 is +0 for either zero)."""
    return (np.asarray(a, np.float32) + np.float32(0.0)).view(np.int32)


def raw_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def give_r(r, b):
    """r on the GPU as the entry takes it; a shared row (c,) is row 0 of a (b, c) buffer of NaN."""
    if r.ndim > 1:
        return cu(r)
    buf = np.full((max(b, 2), r.shape[0]), np.nan, np.float32)
    buf[0] = r
    return cu(buf)[0]


def run_affine(y, p, w, r, act, **kw):
    from rfnet_amd import _raw
    b = (y if y is not None else p).shape[0]
    return host(_raw.point_affine(cu(y), cu(p), cu(w), give_r(r, b), act, **kw))


def affine_cases(c):
    """(n, kp, has_y, r_shape, b): every n with every kp of this width; each with a shared row r (c,) at b = 3 -- its stride
    of 0 is what is under test -- and with a per-sample r, (b, 1, c) and (b, c) taking turns, as do y present / absent and
    b in {1, 3}."""
    kps = range(PA_KMAX + 1) if c == C_ALL_KP else (0, 3, PA_KMAX)
    turn = itertools.count()
    for n, kp in itertools.product(AFFINE_NS, kps):
        t = next(turn)
        yield n, kp, kp == 0 or t % 2 == 0, "c", 3
        yield n, kp, kp == 0 or t % 2 == 1, ("b1c", "bc")[t // 2 % 2], (3, 1, 3)[t % 3]


# ------------------------------------------------------------------ rf_point_affine -----------------------------------------
@pytest.mark.parametrize("c", CS)
def test_affine_exact_grid_bit_for_bit(c):
    rng = np.random.RandomState(c)
    for n, kp, has_y, r_shape, b in affine_cases(c):
        y, p, w, r = R.affine_inputs(rng, b, n, c, kp, has_y, r_shape, "A")
        exp = R.point_affine_exact(y, p, w, r, None)
        for act in (None, "relu"):
            want = exp if act is None else np.maximum(exp, np.float32(0.0))  # exact too
            assert np.array_equal(bits(run_affine(y, p, w, r, act)), bits(want)), (n, kp, has_y, r_shape, b, act)


@pytest.mark.parametrize("c", CS)
def test_affine_randn_within_the_rounding_bound(c):
    rng = np.random.RandomState(1000 + c)
    worst = 0.0
    for n, kp, has_y, r_shape, b in affine_cases(c):
        y, p, w, r = R.affine_inputs(rng, b, n, c, kp, has_y, r_shape, "B")
        pre, mag = R.affine_terms(y, p, w, r)
        bound = (kp + 2) * R.U * mag  # R.point_affine_bound
        for act in R.ACTS:
            got, ref = run_affine(y, p, w, r, act), R.activate(pre, act)
            bar = bound if act != "tanh" else bound + 2 * TANHF_ULP * np.spacing(np.abs(ref).astype(np.float32))
            err = np.abs(got - ref)
            worst = max(worst, float((err / bar).max()))
            assert np.all(err <= bar), (n, kp, has_y, r_shape, b, act, float((err / bar).max()))
    print(f"c={c}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("c", CS)
def test_affine_aliasing_strides_and_invariance(c):
    from rfnet_amd import _raw
    rng = np.random.RandomState(2000 + c)
    b, n, kp = 3, PA_STRIP + 1, 3
    y, p, w, r = R.affine_inputs(rng, b, n, c, kp, True, "bc", "A")
    exp = R.point_affine_exact(y, p, w, r, "relu")
    # out = y, which the header allows
    yg = cu(y.copy())
    ret = _raw.point_affine(yg, cu(p), cu(w), cu(r), "relu", out=yg)
    assert ret.data_ptr() == yg.data_ptr() and np.array_equal(bits(host(yg)), bits(exp))
    # y and p that are views with gaps
    wide_y, wide_p = cu(np.concatenate([y, y + 1], -1)), cu(np.concatenate([p, p + 1], -1))
    yv, pv = wide_y[:, :, :c], wide_p[:, :, :kp]
    assert not yv.is_contiguous() and not pv.is_contiguous()
    assert np.array_equal(bits(host(_raw.point_affine(yv, pv, cu(w), cu(r), "relu"))), bits(exp))
    assert np.array_equal(host(wide_y), np.concatenate([y, y + 1], -1))  # and the views' owner is as it was
    # the same bits again, and every sample is the call on its slice (randn, all activations, both kinds of r)
    y, p, w, r = R.affine_inputs(rng, b, n, c, kp, True, "bc", "B")
    shared = r[0].copy()
    for act in R.ACTS:
        got = run_affine(y, p, w, r, act)
        assert np.array_equal(raw_bits(got), raw_bits(run_affine(y, p, w, r, act))), act
        got_s = run_affine(y, p, w, shared, act)
        for i in range(b):
            assert np.array_equal(raw_bits(got[i:i + 1]), raw_bits(run_affine(y[i:i + 1], p[i:i + 1], w, r[i:i + 1], act))), (act, i)
            assert np.array_equal(raw_bits(got_s[i:i + 1]), raw_bits(run_affine(y[i:i + 1], p[i:i + 1], w, shared, act))), (act, i)


@pytest.mark.parametrize("act", R.ACTS)
def test_affine_non_finite_values_reach_out_as_torch_gives_them(act):
    """NaN and +-inf in y, p or r: no activation and relu hand them on as torch.relu(y + p @ w + r) does (a NaN stays a NaN:
    fmaxf(v, 0) would give 0), tanh(+-inf) = +-1 and tanh(NaN) = NaN."""
    for c in (12, 128):
        rng = np.random.RandomState(3000 + c)
        b, n, kp = 3, PA_STRIP + 1, 3
        y, p, w, r = R.affine_inputs(rng, b, n, c, kp, True, "bc", "B")
        w[np.abs(w) < 0.05] = 0.5  # inf * w is an infinity of a known sign
        y[0, 0, 0], y[0, 1, 1], y[0, 2, 2], y[0, PA_STRIP, 3] = np.nan, np.inf, -np.inf, np.nan
        p[1, 0, 0], p[1, 1, 1], p[1, 2, 2], p[1, PA_STRIP, 0] = np.nan, np.inf, -np.inf, -np.inf
        r[2, 5], r[2, 6], r[2, 7] = np.nan, np.inf, -np.inf
        y[2, 3, 6] = -np.inf  # inf - inf
        got = run_affine(y, p, w, r, act)
        ref = R.point_affine(y, p, w, r, act)
        ty, tp, tw, tr = (torch.from_numpy(a) for a in (y, p, w, r))
        pre = ty + tp @ tw + tr[:, None, :]
        tor = (torch.relu(pre) if act == "relu" else torch.tanh(pre) if act == "tanh" else pre).numpy()
        plain = np.isfinite(R.affine_terms(y, p, w, r)[1])  # elements no non-finite value reaches
        assert (~plain).sum() >= 3 * c and np.isnan(ref).any()
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(got), np.isnan(tor)), act
        # where a non-finite value arrives, the result is exactly the reference's and torch's: NaN, an infinity, 0 or +-1
        assert np.array_equal(got[~plain], ref[~plain].astype(np.float32), equal_nan=True), act
        assert np.array_equal(got[~plain], tor[~plain], equal_nan=True), act
        if act == "relu":
            assert (ref[~plain] == 0).any() and np.isnan(got[0, 0, 0]) and np.isnan(got[2, :, 5]).all()
        if act == "tanh":
            assert set(np.unique(got[~plain & ~np.isnan(ref)]).tolist()) == {-1.0, 1.0}
        bar = R.point_affine_bound(y, p, w, r)[plain]
        if act == "tanh":
            bar = bar + 2 * TANHF_ULP * np.spacing(np.abs(ref[plain]).astype(np.float32))
        assert np.all(np.abs(got[plain] - ref[plain]) <= bar), act


def test_tanhf_error_against_float64():
    """tanhf's own error, the one term of the tanh bar that cannot be derived: the worst distance between the kernel's
    tanh output and float64 tanh of the kernel's OWN act = 0 output on the same inputs, in fp32 spacings at the result.
    Arguments: 65,536 pre-activations with |x| spread evenly in log from 1e-6 to 20, both signs, with 1e-6, 0.5, 1, 5, 9, 20
    and +-inf planted.  Measured on an MI355X: 1.262 spacings, at x = -0.6279215 (TANHF_ULP).  The bar, here and in the
    tanh comparisons with float64, is twice that."""
    rng = np.random.RandomState(7)
    n, c = 512, 128
    mag = np.exp(rng.uniform(np.log(1e-6), np.log(20.0), size=(1, n, c)))
    y = (mag * rng.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
    planted = [1e-6, 0.5, 1.0, 5.0, 9.0, 20.0, np.inf]
    y[0, 0, :14] = np.array(planted + [-v for v in planted], np.float32)
    p, w = (rng.standard_normal((1, n, 3)) * 1e-3).astype(np.float32), (rng.standard_normal((3, c)) * 1e-3).astype(np.float32)
    r = np.zeros(c, np.float32)
    p[0, 0], r[:] = 0.0, 0.0  # the planted arguments arrive as they are
    pre, got = run_affine(y, p, w, r, None), run_affine(y, p, w, r, "tanh")
    assert np.array_equal(pre[0, 0, :14], y[0, 0, :14])
    assert got[0, 0, 6] == 1.0 and got[0, 0, 13] == -1.0  # tanh(+-inf)
    dist = R.ulp_distance(got, np.tanh(pre.astype(np.float64)))
    worst = float(dist.max())
    at = np.unravel_index(dist.argmax(), dist.shape)
    print(f"tanhf: worst distance {worst:.3f} fp32 spacings at x = {pre[at]!r}; recorded {TANHF_ULP}")
    assert np.all(np.abs(got) <= 1.0) and np.array_equal(np.sign(got), np.sign(pre))
    assert worst <= 2 * TANHF_ULP


# ------------------------------------------------------------------ the poolings ---------------------------------------------
def run_pools(x, lengths=None):
    """(values of rf_maxpool_points, values and indices of rf_maxpool_points_idx) as numpy, values (b, c)."""
    from rfnet_amd import _raw
    xg = cu(x)
    v0 = _raw.maxpool_points(xg, lengths)
    v1, i1 = _raw.maxpool_points_idx(xg, lengths)
    assert v0.shape == (x.shape[0], 1, x.shape[2]) and v1.shape == v0.shape and i1.dtype == torch.int32
    return host(v0)[:, 0], host(v1)[:, 0], host(i1).astype(np.int64)


def check_pools(x, lengths, what, want_idx=None, device_counts=None):
    """Both poolings against the float64 scan: indices exactly, values as numbers (the sign of a zero may differ between
    the two entries: the rule is `lowest index among == ties`, not a bit pattern of zero)."""
    v0, v1, i1 = run_pools(x, device_counts if device_counts is not None else lengths)
    rv, ri = R.maxpool(x, lengths)
    assert np.array_equal(i1, ri), what
    if want_idx is not None:
        assert np.array_equal(i1, want_idx), what
    assert not np.isnan(v0).any() and not np.isnan(v1).any(), what
    assert np.array_equal(v1, rv) and np.array_equal(v0, rv) and np.array_equal(v0, v1), what
    return v0, v1, i1


@pytest.mark.parametrize("c", CS)
def test_pool_planted_winners_and_ties(c):
    """The maximum of every channel planted at rows {0, 1, ppi - 1, ppi, 255, 256, n - 1} in turn and duplicated at a higher
    row of the same point-lane, at another lane of the same strip, or in a later strip: the lower row is the answer.  Then
    small integers alone, where every channel ties many times within lanes, across lanes and across strips."""
    rng = np.random.RandomState(4000 + c)
    ppi = R.ppi_of(c, MP_TPB)
    for k, n in enumerate(POOL_NS):
        b = (3, 1)[k % 2]
        x, want = R.pool_planted(rng, b, n, c, ppi, MP_STRIP)
        v0, v1, i1 = check_pools(x, None, ("planted", n), want_idx=want)
        assert np.all(v1 == 5.0)
        ties = rng.randint(-3, 4, size=(b, n, c)).astype(np.float32)
        t0, t1, ti = check_pools(ties, None, ("ties", n))
        # a second call returns the same bits, and every sample is the call on its slice
        s0, s1, si = run_pools(ties)
        assert np.array_equal(raw_bits(s0), raw_bits(t0)) and np.array_equal(raw_bits(s1), raw_bits(t1)) and np.array_equal(si, ti)
        for i in range(b if b > 1 else 0):
            s0, s1, si = run_pools(ties[i:i + 1])
            assert np.array_equal(raw_bits(s0), raw_bits(t0[i:i + 1])) and np.array_equal(raw_bits(s1), raw_bits(t1[i:i + 1])), (n, i)
            assert np.array_equal(si, ti[i:i + 1]), (n, i)


@pytest.mark.parametrize("c", CS)
def test_pool_special_values(c):
    """NaN among valid rows is skipped, an all-NaN and an all -inf channel give -inf with index 0, +inf ties and -0.0 / +0.0
    ties go to the lower row, within a strip and across strips."""
    rng = np.random.RandomState(5000 + c)
    n = 2 * MP_STRIP + 1
    x = rng.standard_normal((3, n, c)).astype(np.float32)
    x[0, ::3] = np.nan                                   # NaN rows among the valid ones, row 0 included
    x[0, 1, 0], x[0, 4, 0] = 9.0, 9.0                    # ... with a tie between the numbers that are left
    x[1, :, 0] = np.nan                                  # an all-NaN channel
    x[1, :, 1] = -np.inf                                 # an all -inf channel
    x[1, :, 2], x[1, 0, 2] = -np.inf, np.nan             # NaN first, then -inf only
    x[1, [5, MP_STRIP + 9], 3] = np.inf                  # +inf twice, in two strips
    x[2, :, 0] = -1.0
    x[2, 3, 0], x[2, 4, 0], x[2, MP_STRIP + 1, 0] = -0.0, 0.0, 0.0   # zeros of both signs tie: row 3
    x[2, :, 1] = -1.0
    x[2, MP_STRIP - 1, 1], x[2, MP_STRIP, 1] = 0.0, -0.0             # the same across the strip edge
    x[2, :, 2] = np.inf                                   # +inf everywhere
    v0, v1, i1 = check_pools(x, None, "special")
    assert i1[0, 0] == 1 and v1[0, 0] == 9.0
    assert np.isneginf(v1[1, :3]).all() and not i1[1, :3].any() and v1[1, 3] == np.inf and i1[1, 3] == 5
    assert i1[2, 0] == 3 and v1[2, 0] == 0.0 and i1[2, 1] == MP_STRIP - 1 and v1[2, 1] == 0.0 and i1[2, 2] == 0


@pytest.mark.parametrize("fill", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("c", CS)
def test_pool_ragged_against_the_float64_scan(c, fill):
    """The _lengths forms against the reference run on x[i, :count] -- not against the dense entries, with which they share
    their indexing.  Counts {1, 255, 256, 257, 512, 600} and, as device counts, {0, n + 7} (held to 1 and n); +inf or NaN
    behind every count, which would win or poison the maximum if read; small integers, so ties are everywhere."""
    rng = np.random.RandomState(6000 + c)
    b, n = len(RAGGED_COUNTS), RAGGED_N
    x = rng.randint(-3, 4, size=(b, n, c)).astype(np.float32)
    held = R.counts_of(RAGGED_COUNTS, b, n)
    assert held.tolist()[-2:] == [1, n]
    for i, ln in enumerate(held):
        x[i, ln:] = fill
    dev = torch.tensor(RAGGED_COUNTS, dtype=torch.int32).cuda()
    v0, v1, i1 = check_pools(x, RAGGED_COUNTS, ("device counts", fill), device_counts=dev)
    assert np.all(i1 < held[:, None]) and np.isfinite(v1).all()
    check_pools(x[:6], RAGGED_COUNTS[:6], ("host counts", fill))
    s0, s1, si = run_pools(x, dev)
    assert np.array_equal(raw_bits(s0), raw_bits(v0)) and np.array_equal(raw_bits(s1), raw_bits(v1)) and np.array_equal(si, i1)
    for i in (1, 3, 5):  # a sample is the ragged call on its slice
        s0, s1, si = run_pools(x[i:i + 1], [int(held[i])])
        assert np.array_equal(raw_bits(s0), raw_bits(v0[i:i + 1])) and np.array_equal(raw_bits(s1), raw_bits(v1[i:i + 1]))
        assert np.array_equal(si, i1[i:i + 1])


# ------------------------------------------------------------------ rf_act_grad_colsum --------------------------------------
def colsum_ns(c):
    """n = MP_STRIP + t: a last strip of 1, ppi, 4 ppi - 1, 4 ppi and 4 ppi + 1 rows (the point loop keeps four rows in
    flight per lane), at every ppi, and the strip edge itself.  n <= 2048 keeps family A exact."""
    ppi = R.ppi_of(c, MP_TPB)
    ns = {1, MP_STRIP - 1, MP_STRIP} | {MP_STRIP + t for t in (1, ppi, 4 * ppi - 1, 4 * ppi, 4 * ppi + 1)}
    return sorted(n for n in ns if n <= 2048)


def run_colsum(grad, out, act, **kw):
    from rfnet_amd import _raw
    g, sums = _raw.act_grad_colsum(cu(grad), cu(out), act, **kw)
    return host(g), host(sums)


@pytest.mark.parametrize("c", CS)
def test_colsum_exact_grid_bit_for_bit(c):
    rng = np.random.RandomState(7000 + c)
    for k, n in enumerate(colsum_ns(c)):
        grad, out = R.colsum_inputs(rng, (3, 1)[k % 2], n, c, "A")
        for act in R.GRAD_ACTS:
            g, sums = run_colsum(grad, out, act)
            if act != "tanh":  # a copy, a select or one product: the bits of the fp32 restatement, the sign of a zero included
                assert np.array_equal(raw_bits(g), raw_bits(R.act_grad_f32(grad, out, act))), (n, act)
            if act != "leaky_relu":
                eg, es = R.act_grad_exact(grad, out, act)
                assert np.array_equal(bits(g), bits(eg)) and np.array_equal(bits(sums), bits(es)), (n, act)
            else:  # 0.2f * grad rounds: the sums take the bound of family B
                assert np.all(np.abs(sums - R.act_grad(grad, out, act)[1]) <= R.colsum_bound(grad, out, act, MP_STRIP, MP_TPB)), n


@pytest.mark.parametrize("c", CS)
def test_colsum_randn_within_the_rounding_bound(c):
    """g: bit for bit for none, relu and leaky relu; tanh within 3 U |grad| (1 + out^2) -- a square, a subtraction and a
    product, with the INCOMING gradient: where out^2 is near 1 the rounding of out^2 alone is U |grad| while the result is
    near 0, so no bound in terms of the result holds for grad * (1 - out * out) in fp32 (tests/test_pointmlp_host.py shows
    it on the CPU).  sums: against the float64 column sum of the REFERENCE's g, within
    sum_j |g error bound_j| + D U sum_j |g_j|, D = ceil(MP_STRIP / ppi) + ppi - 1 + nstrips."""
    rng = np.random.RandomState(8000 + c)
    worst = 0.0
    for k, n in enumerate(colsum_ns(c)):
        grad, out = R.colsum_inputs(rng, (1, 3)[k % 2], n, c, "B")
        out[0, : min(n, 40), 0] = np.linspace(0.97, 1.03, 40)[: min(n, 40)]  # where 1 - out^2 cancels
        for act in R.GRAD_ACTS:
            g, sums = run_colsum(grad, out, act)
            rg, rs = R.act_grad(grad, out, act)
            if act != "tanh":
                assert np.array_equal(raw_bits(g), raw_bits(R.act_grad_f32(grad, out, act))), (n, act)
            assert np.all(np.abs(g - rg) <= R.act_grad_bound(grad, out, act, rg)), (n, act)
            bar = R.colsum_bound(grad, out, act, MP_STRIP, MP_TPB, rg)
            err = np.abs(sums - rs)
            assert np.all(err <= bar), (n, act, float((err / bar).max()))
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    print(f"c={c}: worst sums error / bound {worst:.3f}")


@pytest.mark.parametrize("c", CS)
def test_colsum_in_place_null_g_and_invariance(c):
    from rfnet_amd import _host as H
    from rfnet_amd import _raw
    from rfnet_amd._lib import lib
    rng = np.random.RandomState(9000 + c)
    ppi = R.ppi_of(c, MP_TPB)
    b, n = 3, min(MP_STRIP + 4 * ppi + 1, 2048)
    grad, out = R.colsum_inputs(rng, b, n, c, "B")
    dev = torch.device("cuda", torch.cuda.current_device())
    for act in R.GRAD_ACTS:
        g, sums = run_colsum(grad, out, act)
        g2, sums2 = run_colsum(grad, out, act)
        assert np.array_equal(raw_bits(g), raw_bits(g2)) and np.array_equal(raw_bits(sums), raw_bits(sums2)), act
        for i in range(b):  # every sample is the call on its slice, sums included
            gi, si = run_colsum(grad[i:i + 1], out[i:i + 1], act)
            assert np.array_equal(raw_bits(gi), raw_bits(g[i:i + 1])) and np.array_equal(raw_bits(si), raw_bits(sums[i:i + 1])), (act, i)
        # in place: g overwrites grad
        gg, og = cu(grad.copy()), cu(out)
        ret, s_in = _raw.act_grad_colsum(gg, og, act, inplace=True)
        assert ret.data_ptr() == gg.data_ptr()
        assert np.array_equal(raw_bits(host(gg)), raw_bits(g)) and np.array_equal(raw_bits(host(s_in)), raw_bits(sums)), act
        assert np.array_equal(raw_bits(host(og)), raw_bits(out))
        # g = NULL through the C ABI: the sums alone, nothing else written
        gg, og = cu(grad), cu(out)
        s_null = torch.full((b, c), float("nan"), device="cuda")
        ws, wsz = H.workspace(lib.rf_act_grad_colsum_workspace_bytes(b, n, c), dev, "maxpool")
        rc = lib.rf_act_grad_colsum(b, n, c, gg.data_ptr(), og.data_ptr(), {None: 0, "relu": 1, "tanh": 2, "leaky_relu": 3}[act],
                                    None, s_null.data_ptr(), ws.data_ptr(), wsz, H.stream(dev))
        assert rc == 0
        assert np.array_equal(raw_bits(host(s_null)), raw_bits(sums)), act
        assert np.array_equal(raw_bits(host(gg)), raw_bits(grad)) and np.array_equal(raw_bits(host(og)), raw_bits(out)), act
