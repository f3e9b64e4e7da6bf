"""numpy float64 restatements of the six entries of rfnet_amd/csrc/pointmlp.hip (rf_point_affine, rf_maxpool_points,
rf_maxpool_points_idx, their two _lengths forms, rf_act_grad_colsum), the derived error bounds of their fp32 kernels and
the input families of tests/test_gpu_pointmlp.py.  Nothing here follows the kernels' indexing: every function is the
operation as include/rfops.h states it, written the plainest way.  tests/test_pointmlp_host.py checks these functions
against independent formulations on the CPU, so that the GPU tests rest on references that were themselves checked.

Two input families (tests/test_gpu_pointmlp.py):
  A  values on a dyadic grid on which every fp32 operation of the kernel is exact, in any order and with or without
     FMA contraction: the *_exact functions compute in scaled int64, PROVE the exactness (the sum of the magnitudes of
     all terms, in units of the grid, stays below 2^24, so every partial sum of any order is a representable number) and
     return the one fp32 result every correct kernel must give bit for bit.
  B  randn inputs against the float64 functions under the bounds derived below (U = 2^-24, the fp32 unit roundoff)."""
import os
import re

import numpy as np

U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)
LEAKY_SLOPE = float(np.float32(0.2))  # the op is defined on fp32 tensors: its slope is the fp32 number 0.2f
ACTS = (None, "relu", "tanh")
GRAD_ACTS = (None, "relu", "tanh", "leaky_relu")


def kernel_constants():
    """{name: value} of the `constexpr int` tile constants of pointmlp.hip (PA_TPB, PA_KMAX, PA_STRIP, MP_TPB, MP_STRIP):
    read from the source, so that the shapes of the tests move with the kernels."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rfnet_amd", "csrc", "pointmlp.hip")
    src = open(path).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+((?:PA|MP)_[A-Z]+)\s*=\s*(\d+)\s*;", src)}
    for name in ("PA_TPB", "PA_KMAX", "PA_STRIP", "MP_TPB", "MP_STRIP"):
        assert name in found, f"{name} is not a constexpr int of pointmlp.hip any more"
    return found


def ppi_of(c, tpb):
    """Point-lanes of a workgroup of `tpb` threads at `c` channels: a thread owns four channels."""
    return tpb // (c // 4)


# ------------------------------------------------------------------ the operations, float64 ----------------------------------
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _row(r, b, c):
    """r of shape (b, 1, c), (b, c) or (c,) -> (b or 1, 1, c)."""
    r = _f64(r)
    assert r.shape in ((b, 1, c), (b, c), (c,)), r.shape
    return r.reshape(-1, 1, c)


def affine_terms(y, p, w, r):
    """The pre-activation y + sum_k p_k w_k + r of rf_point_affine and the sum of the magnitudes of its terms
    |y| + sum_k |p_k w_k| + |r|, both (b, n, c) float64.  y or p may be None (not both)."""
    ref = y if y is not None else p
    b, n = ref.shape[0], ref.shape[1]
    c = np.shape(r)[-1]
    rr = _row(r, b, c)
    v = np.zeros((b, n, c)) + rr
    mag = np.zeros((b, n, c)) + np.abs(rr)
    with np.errstate(invalid="ignore"):  # inf - inf and inf * 0 are NaN, as they are in the kernel
        if y is not None:
            v = v + _f64(y)
            mag = mag + np.abs(_f64(y))
        if p is not None and np.shape(p)[-1] > 0:
            p64, w64 = _f64(p), _f64(w)
            v = v + p64 @ w64
            mag = mag + np.abs(p64) @ np.abs(w64)
    return v, mag


def activate(v, act):
    """none / relu / tanh in float64.  relu is torch.relu's and tf.nn.relu's: a NaN stays a NaN, a negative number and
    -0.0 give +0.0 or -0.0 (compared by value)."""
    if act in (None, "none"):
        return v
    if act == "relu":
        with np.errstate(invalid="ignore"):
            return np.where(v < 0, 0.0, v)
    if act == "tanh":
        return np.tanh(v)
    raise ValueError(act)


def point_affine(y, p, w, r, act):
    """out[i,j,:] = act(y[i,j,:] + sum_k p[i,j,k] w[k,:] + r[i,:]), float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return activate(affine_terms(y, p, w, r)[0], act)


def point_affine_bound(y, p, w, r):
    """|fp32 kernel - float64 reference| per element for act none and relu: (kp + 2) U (|y| + sum_k |p_k w_k| + |r|).
    The kernel rounds kp times in the FMA chain and once in the add of r, each time by at most U times the magnitude of
    a partial sum, which the sum of the magnitudes of the terms bounds; one more step covers the reference's own float64
    arithmetic and the second-order terms.  relu is exact and 1-Lipschitz, so it inherits the bound."""
    kp = 0 if p is None else np.shape(p)[-1]
    return (kp + 2) * U * affine_terms(y, p, w, r)[1]


def counts_of(lengths, b, n):
    """Per-sample row counts as the ragged kernels hold them: clamped into [1, n]; None = all rows."""
    if lengths is None:
        return np.full(b, n, np.int64)
    ln = np.asarray(lengths, np.int64)
    assert ln.shape == (b,)
    return np.clip(ln, 1, n)


def maxpool(x, lengths=None):
    """Max over the points axis of x (b, n, c) -> values (b, c) float64 and indices (b, c) int64: one scan over the rows
    [0, count) in ascending order that moves on `v > m` only.  So a NaN is skipped, the lowest index among == ties wins
    (-0.0 == +0.0 is a tie: the value carries the sign of the FIRST of them), and a channel with no value above -inf
    returns -inf with index 0."""
    x = _f64(x)
    b, n, c = x.shape
    cnt = counts_of(lengths, b, n)
    val = np.full((b, c), -np.inf)
    idx = np.zeros((b, c), np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(b):
            for j in range(int(cnt[i])):
                take = x[i, j] > val[i]
                val[i] = np.where(take, x[i, j], val[i])
                idx[i] = np.where(take, j, idx[i])
    return val, idx


def act_grad(grad, out, act):
    """g = grad * act'(out) with `out` the layer's OUTPUT, and its column sums over the points axis: (b, n, c) and (b, c)
    float64.  relu: out > 0; tanh: 1 - out^2; leaky_relu: slope LEAKY_SLOPE where out is not > 0."""
    grad = _f64(grad)
    if act in (None, "none"):
        g = grad.copy()
    else:
        o = _f64(out)
        if act == "relu":
            g = np.where(o > 0, grad, 0.0)
        elif act == "tanh":
            g = grad * (1.0 - o * o)
        elif act == "leaky_relu":
            g = np.where(o > 0, grad, grad * LEAKY_SLOPE)
        else:
            raise ValueError(act)
    return g, g.sum(axis=1)


def act_grad_f32(grad, out, act):
    """The float32 restatement of g.  A single rounding (so: the bits a correct kernel must give) for none, relu (+0
    where out is not > 0) and leaky_relu (one fp32 product); tanh rounds three times and is NOT compared through this."""
    grad = np.asarray(grad, np.float32)
    if act in (None, "none"):
        return grad.copy()
    o = np.asarray(out, np.float32)
    if act == "relu":
        return np.where(o > 0, grad, np.float32(0.0)).astype(np.float32)
    if act == "leaky_relu":
        return np.where(o > 0, grad, grad * np.float32(0.2)).astype(np.float32)
    if act == "tanh":
        return (grad * (np.float32(1.0) - o * o)).astype(np.float32)
    raise ValueError(act)


def act_grad_bound(grad, out, act, g=None):
    """|fp32 g - float64 g| per element: none and relu copy (0), leaky_relu is one product (U |g|), tanh is a square, a
    subtraction and a product: with s = fl(o^2), d = fl(1 - s), g = fl(grad d) the error is at most
    U |grad| (o^2 + 2 |1 - o^2|) <= U |grad| (2 + 3 o^2) <= 3 U |grad| (1 + o^2).  It is stated with the INCOMING gradient:
    where o^2 is near 1 the rounding of o^2 alone, U |grad|, stays while the result goes to 0.
    g: the reference's g, if the caller has it."""
    if g is None:
        g, _ = act_grad(grad, out, act)
    if act in (None, "none", "relu"):
        return np.zeros_like(g)
    if act == "leaky_relu":
        return U * np.abs(g)
    o = _f64(out)
    return 3 * U * np.abs(_f64(grad)) * (1.0 + o * o)


def colsum_chain(n, c, mp_strip, mp_tpb):
    """D, the longest chain of fp32 additions behind one entry of `sums`: a point-lane adds its ceil(MP_STRIP / ppi) rows
    of a strip, the ppi lanes of a strip are added in a row, then the strips."""
    ppi = ppi_of(c, mp_tpb)
    nstrips = -(-n // mp_strip)
    return -(-mp_strip // ppi) + ppi - 1 + nstrips


def colsum_bound(grad, out, act, mp_strip, mp_tpb, g=None):
    """|fp32 sums - float64 column sum of the reference's g| per (sample, channel):
    sum_j |g error bound_j| + D U sum_j |g_j|."""
    grad = _f64(grad)
    _, n, c = grad.shape
    if g is None:
        g, _ = act_grad(grad, out, act)
    d = colsum_chain(n, c, mp_strip, mp_tpb)
    return act_grad_bound(grad, out, act, g).sum(axis=1) + d * U * np.abs(g).sum(axis=1)


def ulp_distance(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref| (float64 ref, fp32 got); 0 where both are the same infinity or
    both NaN."""
    got = _f64(got)
    ref64 = _f64(ref64)
    with np.errstate(invalid="ignore"):
        sp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
        d = np.abs(got - ref64) / sp
    same = (got == ref64) | (np.isnan(got) & np.isnan(ref64))
    return np.where(same, 0.0, d)


# ------------------------------------------------------------------ family A: exact on a dyadic grid -----------------------
EXACT_LIMIT = 2 ** 24  # integers below it are fp32 numbers


def _scaled(a, scale):
    """a * scale as int64, asserting that a lies on the grid 1 / scale."""
    s = _f64(a) * scale
    i = np.rint(s).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "input is not on the dyadic grid"
    return i


def point_affine_exact(y, p, w, r, act):
    """rf_point_affine for y, r, p, w on the grid 1/8 and act none or relu: the fp32 result, proven exact.  Every term is
    a multiple of 1/64 (a product p_k w_k is formed exactly, fused or not); if the sum of the magnitudes of the terms, in
    units of 1/64, is below 2^24, every partial sum of any order is a multiple of 1/64 below 2^24 / 64: representable."""
    assert act in (None, "none", "relu")
    ref = y if y is not None else p
    b, n = ref.shape[0], ref.shape[1]
    c = np.shape(r)[-1]
    rr = _scaled(r, 8).reshape(-1, 1, c) * 8
    tot = np.zeros((b, n, c), np.int64) + rr
    mag = np.zeros((b, n, c), np.int64) + np.abs(rr)
    if y is not None:
        yy = _scaled(y, 8) * 8
        tot, mag = tot + yy, mag + np.abs(yy)
    if p is not None and np.shape(p)[-1] > 0:
        pp, ww = _scaled(p, 8), _scaled(w, 8)
        tot, mag = tot + pp @ ww, mag + np.abs(pp) @ np.abs(ww)
    assert int(mag.max()) < EXACT_LIMIT, "a partial sum could round"
    if act == "relu":
        tot = np.maximum(tot, 0)
    out = (tot.astype(np.float64) / 64.0).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * 64.0, tot.astype(np.float64))
    return out


def act_grad_exact(grad, out, act):
    """rf_act_grad_colsum for grad on the grid 1/8 and out on the grid 1/4 within [-1, 1], act none, relu or tanh: g and
    sums in fp32, proven exact.  tanh: out^2 is a multiple of 1/16 in [0, 1], 1 - out^2 too, g a multiple of 1/128; if
    the column sum of |g| in units of 1/128 is below 2^24, every partial sum of any order is representable.  (The sign
    of a zero is left open: compare by value.)"""
    assert act in (None, "none", "relu", "tanh")
    gi = _scaled(grad, 8) * 16                      # units of 1/128
    if act in ("relu", "tanh"):
        oi = _scaled(out, 4)
        assert int(np.abs(oi).max()) <= 4
        gi = np.where(oi > 0, gi, 0) if act == "relu" else (gi // 16) * (16 - oi * oi)
    assert int(np.abs(gi).sum(axis=1).max()) < EXACT_LIMIT, "a partial sum could round"
    g = (gi.astype(np.float64) / 128.0).astype(np.float32)
    sums = (gi.sum(axis=1).astype(np.float64) / 128.0).astype(np.float32)
    assert np.array_equal(g.astype(np.float64) * 128.0, gi.astype(np.float64))
    assert np.array_equal(sums.astype(np.float64) * 128.0, gi.sum(axis=1).astype(np.float64))
    return g, sums


# ------------------------------------------------------------------ the input families ------------------------------------
def grid(rng, shape, step, kmax):
    """Uniform draws from {k * step : |k| <= kmax}, float32."""
    return (rng.randint(-kmax, kmax + 1, size=shape) * step).astype(np.float32)


def affine_inputs(rng, b, n, c, kp, has_y, r_shape, family):
    """(y, p, w, r) float32: family "A" on the grid {k/8 : |k| <= 32}, family "B" randn."""
    draw = (lambda s: grid(rng, s, 0.125, 32)) if family == "A" else (lambda s: rng.standard_normal(s).astype(np.float32))
    y = draw((b, n, c)) if has_y else None
    p = draw((b, n, kp)) if kp else None
    w = draw((kp, c)) if kp else None
    r = draw({"b1c": (b, 1, c), "bc": (b, c), "c": (c,)}[r_shape])
    return y, p, w, r


def colsum_inputs(rng, b, n, c, family):
    """(grad, out) float32: family "A" has grad in {k/8 : |k| <= 32} and out in {k/4 : |k| <= 4} with 0.0, -0.0, +1 and
    -1 planted in every sample; family "B" is randn with the same zeros planted (zero is NOT positive)."""
    if family == "A":
        grad, out = grid(rng, (b, n, c), 0.125, 32), grid(rng, (b, n, c), 0.25, 4)
    else:
        grad, out = rng.standard_normal((b, n, c)).astype(np.float32), rng.standard_normal((b, n, c)).astype(np.float32)
    flat = out.reshape(b, -1)
    special = [0.0, -0.0, 1.0, -1.0] if family == "A" else [0.0, -0.0]
    for k, v in enumerate(special):
        flat[:, k::7][:, :3] = np.float32(v)
    return grad, out


def pool_winner_rows(n, ppi, mp_strip):
    """The rows a channel's maximum is planted at, in turn: the first rows, both sides of the first point-lane wrap,
    both sides of the first strip edge, the last row."""
    rows = [0, 1, ppi - 1, ppi, mp_strip - 1, mp_strip, n - 1]
    return [j for j in rows if 0 <= j < n]


def pool_planted(rng, b, n, c, ppi, mp_strip, peak=5.0):
    """Family A pooling input with planted winners: small integers in [-3, 3] (ties everywhere), and per channel a
    maximum `peak` at a row cycling over pool_winner_rows, duplicated at a HIGHER row chosen, in turn, as
      0  the next row of the same point-lane (row + ppi),
      1  another lane of the same strip (row + 1),
      2  a row of a later strip (row + mp_strip),
      3  no duplicate,
    wherever that row exists.  Returns x (b, n, c) float32 and the expected indices (b, c) -- always the lower row."""
    x = rng.randint(-3, 4, size=(b, n, c)).astype(np.float32)
    rows = pool_winner_rows(n, ppi, mp_strip)
    want = np.zeros((b, c), np.int64)
    for i in range(b):
        for ch in range(c):
            k = ch + i  # samples differ
            j = rows[k % len(rows)]
            dup = (j + ppi, j + 1, j + mp_strip, -1)[(k // len(rows)) % 4]
            x[i, j, ch] = peak
            if 0 <= dup < n:
                x[i, dup, ch] = peak
            want[i, ch] = j
    return x, want
