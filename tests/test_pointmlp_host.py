"""tests/pointmlp_ref.py -- the float64 references, exact-grid references, bounds and input families behind
tests/test_gpu_pointmlp.py -- against independent formulations, on the CPU: torch float64 einsum for the affine part,
amax and first-occurrence argmax for the poolings, autograd of the float64 activations for the activation gradient."""
import numpy as np
import pytest
import torch

import pointmlp_ref as R

K = R.kernel_constants()
F64 = torch.float64


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def same(a, b):
    """Equal as numbers, NaN in the same places."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ------------------------------------------------------------------ constants -------------------------------------------------
def test_constants_come_from_the_kernel_source():
    assert set(K) >= {"PA_TPB", "PA_KMAX", "PA_STRIP", "MP_TPB", "MP_STRIP"} and all(type(v) is int and v > 0 for v in K.values())
    from rfnet_amd import _lib
    src = open(_lib._PKG + "/csrc/pointmlp.hip").read()
    # what the shapes of the GPU tests assume about the indexing: a thread owns four channels, the point-lanes of a
    # workgroup are TPB / quads
    assert src.count("const int quads = c >> 2") >= 3 and "ppi = PA_TPB / quads" in src and "ppi = MP_TPB / quads" in src
    assert "c / 4 <= PA_TPB" in src and "c / 4 > MP_TPB" in src  # c <= 4 * TPB: at least one point-lane
    if K["MP_TPB"] == 256:  # the widths of the GPU tests were chosen for these lane counts
        assert [R.ppi_of(c, 256) for c in (4, 12, 20, 128, 256, 260, 512, 516, 1024)] == [256, 85, 51, 8, 4, 3, 2, 1, 1]


# ------------------------------------------------------------------ point_affine ----------------------------------------------
def _torch_affine(y, p, w, r, act):
    b, n = (y if y is not None else p).shape[:2]
    c = r.shape[-1]
    v = torch.zeros(b, n, c, dtype=F64)
    if y is not None:
        v = v + t64(y)
    if p is not None:
        v = v + torch.einsum("bnk,kc->bnc", t64(p), t64(w))
    v = v + (t64(r).reshape(b, 1, c) if r.size == b * c and r.ndim > 1 else t64(r))
    return (torch.relu(v) if act == "relu" else torch.tanh(v) if act == "tanh" else v).numpy()


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("family", ["A", "B"])
def test_point_affine_is_the_einsum(family, act):
    rng = np.random.RandomState(3)
    for b, n, c, kp, has_y, r_shape in ((1, 1, 4, 0, True, "c"), (3, 5, 12, 3, True, "b1c"), (3, 7, 20, 16, False, "c"),
                                        (2, 9, 8, 1, False, "bc"), (3, 4, 16, 5, True, "bc"), (1, 3, 4, 2, True, "b1c")):
        y, p, w, r = R.affine_inputs(rng, b, n, c, kp, has_y, r_shape, family)
        got, exp = R.point_affine(y, p, w, r, act), _torch_affine(y, p, w, r, act)
        assert got.shape == (b, n, c) and got.dtype == np.float64
        # float64 sums in two orders: 20 roundings of 2^-53 at the most; tanh is 1-Lipschitz and the two libraries' own
        # tanh are a few float64 steps apart
        assert np.all(np.abs(got - exp) <= 20 * 2.0 ** -53 * R.affine_terms(y, p, w, r)[1] + 4 * 2.0 ** -53), (b, n, c, kp)
        if family == "A":
            if act != "tanh":
                assert np.array_equal(got, exp)  # exact in float64 whatever the order
                ex = R.point_affine_exact(y, p, w, r, act)
                assert ex.dtype == np.float32 and np.array_equal(ex.astype(np.float64), got)


@pytest.mark.parametrize("act", R.ACTS)
def test_point_affine_non_finite_values_follow_torch(act):
    rng = np.random.RandomState(4)
    y, p, w, r = R.affine_inputs(rng, 2, 6, 8, 3, True, "bc", "B")
    y[0, 0, 0], y[0, 1, 1], y[0, 2, 2] = np.nan, np.inf, -np.inf
    p[1, 0, 0], p[1, 1, 1], p[1, 2, 2] = np.nan, np.inf, -np.inf
    r[0, 5], r[1, 6], r[1, 7] = np.nan, np.inf, -np.inf
    got, exp = R.point_affine(y, p, w, r, act), _torch_affine(y, p, w, r, act)
    assert np.isnan(exp).any() and np.isinf(_torch_affine(y, p, w, r, None)).any()
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and same(got[~np.isfinite(exp)], exp[~np.isfinite(exp)])
    assert np.allclose(got[np.isfinite(exp)], exp[np.isfinite(exp)], rtol=1e-14, atol=0)
    if act == "relu":
        assert np.isnan(R.activate(np.array([np.nan]), "relu"))[0] and R.activate(np.array([-np.inf, -0.0, 2.0]), "relu").tolist() == [0, 0, 2]
    if act == "tanh":
        assert R.activate(np.array([np.inf, -np.inf]), "tanh").tolist() == [1.0, -1.0]


def _fma_chain_f32(y, p, w, r, b, n, c):
    """The kernel's arithmetic restated in fp32: kp fused multiply-adds onto y (the product and the sum formed in float64,
    which holds a product of two fp32 numbers exactly, then rounded once), then the add of r."""
    acc = np.zeros((b, n, c), np.float32) if y is None else y.copy()
    if p is not None:
        for k in range(p.shape[-1]):
            acc = (p[:, :, k, None].astype(np.float64) * w[k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc + r.reshape(-1, 1, c)


def test_point_affine_bound_holds_for_an_fp32_evaluation():
    rng = np.random.RandomState(5)
    for kp in (0, 1, 3, 16):
        y, p, w, r = R.affine_inputs(rng, 3, 50, 32, kp, True, "bc", "B")
        f32 = _fma_chain_f32(y, p, w, r, 3, 50, 32)
        err, bound = np.abs(f32 - R.point_affine(y, p, w, r, None)), R.point_affine_bound(y, p, w, r)
        assert np.all(err <= bound) and bound.max() < 1e-4, kp
        # and it is a bound with something to say: a dropped term of one unit is far outside it
        assert np.all(bound < 1e-5 * (1 + R.affine_terms(y, p, w, r)[1]))


def test_exact_references_refuse_what_could_round():
    rng = np.random.RandomState(6)
    y, p, w, r = R.affine_inputs(rng, 1, 2, 4, 3, True, "c", "A")
    with pytest.raises(AssertionError):
        R.point_affine_exact(y + np.float32(1 / 16), p, w, r, None)        # off the grid
    with pytest.raises(AssertionError):
        R.point_affine_exact(y * np.float32(2.0 ** 18), p, w, r, None)     # a sum that could round
    grad, out = R.colsum_inputs(rng, 1, 5, 4, "A")
    with pytest.raises(AssertionError):
        R.act_grad_exact(grad, out * np.float32(2.0), "tanh")              # out beyond [-1, 1]
    with pytest.raises(AssertionError):
        R.act_grad_exact(grad * np.float32(2.0 ** 22), out, None)


# ------------------------------------------------------------------ maxpool ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_maxpool_is_amax_and_first_argmax_without_nan(n):
    rng = np.random.RandomState(7)
    for x in (rng.standard_normal((3, n, 8)), rng.randint(-3, 4, size=(3, n, 8)).astype(np.float64)):
        val, idx = R.maxpool(x)
        exp = x.max(axis=1)
        first = (x == exp[:, None, :]).argmax(axis=1)  # argmax of a boolean: its first True
        assert np.array_equal(val, exp) and np.array_equal(idx, first) and idx.dtype == np.int64
        tv, ti = t64(x).max(dim=1)
        assert np.array_equal(val, tv.numpy()) and np.array_equal(np.take_along_axis(x, idx[:, None, :], 1)[:, 0], tv.numpy())
        lens = [1, max(1, n // 2), n]
        val, idx = R.maxpool(x, lens)
        for i, ln in enumerate(lens):
            exp = x[i, :ln].max(axis=0)
            assert np.array_equal(val[i], exp) and np.array_equal(idx[i], (x[i, :ln] == exp).argmax(axis=0))


def test_maxpool_special_values():
    inf, nan = np.inf, np.nan
    #             NaN skipped   all NaN   all -inf  -inf after NaN  +inf tie  zeros tie (-0 first)  zeros tie (+0 first)
    x = np.array([[nan,         nan,      -inf,     nan,            inf,      -0.0,                 0.0],
                  [2.0,         nan,      -inf,     -inf,           1.0,      0.0,                  -0.0],
                  [nan,         nan,      -inf,     -inf,           inf,      -1.0,                 -1.0],
                  [2.0,         nan,      -inf,     nan,            inf,      0.0,                  0.0]])[None]
    val, idx = R.maxpool(x)
    assert idx[0].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert same(val[0], [2.0, -inf, -inf, -inf, inf, 0.0, 0.0])
    assert np.signbit(val[0, 5]) and not np.signbit(val[0, 6])  # the value is the first of the tied zeros
    # counts are clamped into [1, n]
    x2 = np.concatenate([x, x])
    v0, i0 = R.maxpool(x2, [0, 11])
    v1, i1 = R.maxpool(x2, [1, 4])
    assert same(v0, v1) and np.array_equal(i0, i1) and R.counts_of([0, 11, -5, 3], 4, 4).tolist() == [1, 4, 1, 3]
    assert same(v0[0], [-inf, -inf, -inf, -inf, inf, -0.0, 0.0]) and not i0[0].any()


def test_pool_planted_winners_are_what_the_reference_finds():
    rng = np.random.RandomState(8)
    strip, tpb = K["MP_STRIP"], K["MP_TPB"]
    for c in (4, 20, 256, 1024):
        ppi = R.ppi_of(c, tpb)
        for n in (1, 2, strip + 1, 3 * strip + 1):
            x, want = R.pool_planted(rng, 2, n, c, ppi, strip)
            val, idx = R.maxpool(x)
            assert np.array_equal(idx, want) and np.all(val == 5.0) and np.all(x <= 5.0), (c, n)
            if n > 2 * strip and ppi < strip:
                # each kind of duplicate is there: the winner's value again one lane on, one pass on, one strip on
                peaks = x == 5.0
                later = [np.any(peaks[:, d:] & peaks[:, :-d] & (np.arange(n - d)[None, :, None] == want[:, None, :]))
                         for d in (1, ppi, strip)]
                assert all(later), (c, later)
                assert (peaks.sum(axis=1) == 1).any()  # and some channels have a single winner


# ------------------------------------------------------------------ act_grad --------------------------------------------------
def _activation(x, act):
    if act == "relu":
        return torch.relu(x)
    if act == "tanh":
        return torch.tanh(x)
    if act == "leaky_relu":
        return torch.nn.functional.leaky_relu(x, R.LEAKY_SLOPE)
    return x


@pytest.mark.parametrize("act", R.GRAD_ACTS)
def test_act_grad_is_autograd_of_the_float64_activation(act):
    rng = np.random.RandomState(9)
    pre = rng.standard_normal((3, 11, 8))
    pre[0, 0, :4] = [0.0, -0.0, 1.0, -1.0]  # zero is not positive: relu' = 0, leaky' = slope there
    grad = rng.standard_normal((3, 11, 8))
    x = t64(pre).requires_grad_(True)
    out = _activation(x, act)
    (exp,) = torch.autograd.grad(out, x, t64(grad))
    g, sums = R.act_grad(grad, out.detach().numpy(), act)
    assert g.dtype == np.float64 and sums.shape == (3, 8)
    # tanh: 1 - out^2 against autograd's own evaluation of it: a few float64 roundings of terms of size |grad| (1 + out^2)
    assert np.all(np.abs(g - exp.numpy()) <= 4 * 2.0 ** -53 * np.abs(grad) * (1 + out.detach().numpy() ** 2))
    if act != "tanh":
        assert np.array_equal(g, exp.numpy())
    assert np.allclose(sums, exp.sum(1).numpy(), rtol=0, atol=11 * 2.0 ** -53 * np.abs(g).sum(1).max())


@pytest.mark.parametrize("act", R.GRAD_ACTS)
def test_act_grad_f32_and_the_bounds(act):
    rng = np.random.RandomState(10)
    grad, out = R.colsum_inputs(rng, 3, 301, 16, "B")
    out[0, :40, 0] = np.linspace(0.97, 1.03, 40)  # where 1 - out^2 cancels
    g64, _ = R.act_grad(grad, out, act)
    g32 = R.act_grad_f32(grad, out, act)
    assert g32.dtype == np.float32
    if act != "tanh":
        # a single rounding: the float64 result rounded once IS the float32 restatement (a product of two fp32 numbers is exact
        # in float64), -0.0 and +0.0 included
        assert np.array_equal(g64.astype(np.float32).view(np.int32), g32.view(np.int32))
    err, bound = np.abs(g32.astype(np.float64) - g64), R.act_grad_bound(grad, out, act)
    assert np.all(err <= bound)
    if act in (None, "relu"):
        assert not bound.any()
    if act == "tanh":
        # the bound is stated with the INCOMING gradient: 3 U |grad| (1 + out^2).  With the result g in its place it is no bound
        # of any fp32 evaluation of grad * (1 - out * out): where out^2 is near 1 the rounding of out^2 alone, U |grad|, exceeds it
        literal = 3 * R.U * np.abs(g64) * (1.0 + out.astype(np.float64) ** 2)
        assert (err > literal).any() and np.all(literal[np.abs(out) < 0.5] <= bound[np.abs(out) < 0.5])
    if act in (None, "relu", "tanh"):
        ga, oa = R.colsum_inputs(rng, 3, 2048, 8, "A")
        ge, se = R.act_grad_exact(ga, oa, act)
        gr, sr = R.act_grad(ga, oa, act)
        assert np.array_equal(ge.astype(np.float64), gr) and np.array_equal(se.astype(np.float64), sr)
        assert np.array_equal(R.act_grad_f32(ga, oa, act), ge)  # exact: the fp32 restatement rounds nowhere
        flat = oa.reshape(3, -1)[:, :28]
        assert all(np.any(flat == v) for v in (0.0, 1.0, -1.0)) and np.any(np.signbit(flat) & (flat == 0))


def test_colsum_chain_and_bound():
    strip, tpb = K["MP_STRIP"], K["MP_TPB"]
    assert R.colsum_chain(strip + 1, 4 * tpb, strip, tpb) == strip + 0 + 2     # one lane: the strip's rows in a row, two strips
    assert R.colsum_chain(1, 4, strip, tpb) == -(-strip // tpb) + tpb - 1 + 1  # a lane per row: the lanes in a row
    rng = np.random.RandomState(11)
    grad, out = R.colsum_inputs(rng, 2, 700, 16, "B")
    for act in R.GRAD_ACTS:
        g32 = R.act_grad_f32(grad, out, act)
        seq = np.zeros((2, 16), np.float32)
        for j in range(700):  # one chain of 700 additions: longer than any of the kernel's
            seq = seq + g32[:, j]
        bound = R.colsum_bound(grad, out, act, strip, tpb)
        long_chain = bound + (700 - R.colsum_chain(700, 16, strip, tpb)) * R.U * np.abs(R.act_grad(grad, out, act)[0]).sum(1)
        assert np.all(np.abs(seq - R.act_grad(grad, out, act)[1]) <= long_chain), act
        # and a dropped row of typical size is outside the bound
        assert np.median(np.abs(R.act_grad(grad, out, act)[0])) > 10 * bound.max() or act == "relu"


def test_ulp_distance():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert R.ulp_distance(up, 1.0) == 1.0 and R.ulp_distance(one, 1.0) == 0.0
    assert R.ulp_distance(np.float32(np.inf), np.inf) == 0.0 and R.ulp_distance(np.float32(np.nan), np.nan) == 0.0
    assert R.ulp_distance(np.float32(1e-6), 1e-6 * (1 + 2.0 ** -24)) < 1.0
