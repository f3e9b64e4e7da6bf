"""A float64 replay of approx_match, level by level, driven by the kernels' OWN stored vectors (numpy only).

Why.  `match` is the end of a chain of up to 64 annealing levels whose clamps make it ill-conditioned
(tests/test_oracle_golden.py::test_match_bar_is_ill_conditioned), so a comparison of `match` with an oracle needs
bars that a sweep which leaves out a sub-chunk of columns still passes.  One LAUNCH of the chain is well-conditioned: P1,
P2 and P3 of a level are sums of non-negative terms followed by a division or a clamped subtraction.  The workspace of
rf_approxmatch* / rf_earth_mover* keeps what every launch wrote (approxmatch.hip, am_init_kernel / AmLayout):

    sample bi at float offset bi * bstride, bstride = (1 + nlevels) * V, V = npad + mpad (both rounded up to CPAD);
    slot s at s * V = [set 1: npad | set 2: mpad]; slot 0 = remainL | remainR, slot 1 + v = ratioL_v | ratioR_v;
    after a call slot 0 holds remainL as the last level's P1 read it (the last P3 is not launched) and remainR after
    the last P2.

`replay` walks the schedule in float64 and, at every level, forms what that level's launches should have written FROM
WHAT THE EARLIER LAUNCHES DID WRITE ("teacher-forced"): 3 * nlevels + 2 comparisons per call, each with a bound per
element and each attributable to one launch.  Nothing here follows the kernels' indexing; `schedule` is
oracle/rfops_oracle.c's orc_approxmatch_levels (the formula of tests/test_gpu_memory_contract.py::_am64).

Notation: u = 2^-24 (half an fp32 spacing, the relative error of one rounding), d2 the squared distance of a pair,
x = d2 * level * log2(e) the exp2 argument, e = 2^x the pair's weight; hats are the kernels' fp32 values.

The weight's error, |e^ - e| <= e * (ln2 * |x| * A_ARG * u + h) + E_FLOOR:
  * argument: dx = fl(x2 - x1) carries u, so dx^2 carries 2 u and so does the sum of the three non-negative squares;
    rf::d2_fma rounds three times (dy * dy, two fmas) on non-negative partial sums: 3 u; the level constant
    fl(level * kLog2e) carries u and kLog2e = 0x3FB8AA3B is 1.34e-8 = 0.224 u off log2(e); the product d2 * c rounds
    once more: A_ARG = 2 + 3 + 1 + 0.224 + 1 = 7.224, taken as 7.25.  A relative error delta of x is a relative error
    ln2 * |x| * delta of 2^x (first order; |x| <= 160 keeps it below 5e-5);
  * h = H_EXP2 = 2^-23: the accuracy the CDNA ISA documents for v_exp_f32 (1 ulp), as a relative error.  Measured on the
    MI355X with rf_probe_exp2 against float64 at 2e6 arguments over [-160, 0] (tests/test_gpu_emd_levels.py::
    test_exp2_error_is_within_the_replays_h, which asserts it): see MEASURED below;
  * E_FLOOR = 2^-126: below it a result may be flushed (and is exactly +0 from x = -160 on); an absolute term;
  * a level whose multiplier is 0 has e = 1.0 exactly in the kernels: no weight error at all.

A sum of N non-negative terms t_i accumulated in fp32 in ANY order (fma chains per column segment or lane, then the
partials combined): the step that adds t_i to a partial sum p errs by at most min(t_i, u (p + t_i)) -- half a spacing
of the result, and never more than the addend itself -- and p + t_i <= S, the whole sum; combining the partials (16
column segments in am_rowk / am_rowl; in am_p2_live a pair, six lane steps, a step per tile and three waves) is at most
COMBINE = 16 more roundings of at most u S.  So   round(S) = sum_i min(t_i, u S) + COMBINE u S   (`_rounding`; first
order in u).  It does not depend on the order, so it covers every route.

The replay's state is its estimate rl, rr of the kernels' remainL^, remainR^ with error terms El, Er (|rl - remainL^|
<= El).  At level v, with RL = ratioL_v and RR = ratioR_v as stored:
  P2   S[l] = sum_k e RL[k] (its error ES: the weights' and the rounding), s = S rr, Es = ES rr + S Er + ES Er + u s
       (the product's rounding); expected ratioR = f(rr, s) = rr min(rr / (s + EPS), 1).  f is 2-Lipschitz in rr
       (2 rr / (s + EPS) < 2 where clamped, 1 elsewhere) and 1-Lipschitz in s, and the kernel rounds the sum with
       EPS, the division and the product: bound 2 Er + Es + 4 u f.  Compared in units of multiR.
  anchoring.  Where the clamp is clearly 1, rr - Er > (s + Es + EPS)(1 + 2 u), the kernel's ratioR = remainR^ * 1 is
       remainR^ bit for bit as P1 and P2 of this level read it: rr = RR[l], Er = 0 from here.  Where the demand clearly
       reaches the supply, s - Es > (rr + Er)(1 + 2 u), max(0, .) leaves exactly +0 on both sides: Er = 0 afterwards.
       (The comparison above is made BEFORE anchoring, with the chain's rr.)
  P1   T[k] = EPS + sum_l e rr[l] (error ET: the weights', e Er, the rounding), expected ratioL = rl / T:
       |RL^ - rl / T| <= u rl / T + El / (T - ET) + (rl / T) ET / (T - ET).  Compared in SHIPPED MASS, times
       U[k] / multiL with U[k] = sum_l e RR[l]: a relative bar on ratioL means nothing for a row that is almost
       consumed, the mass it ships with that ratio does.  Then the row is anchored the same way where that is tighter:
       remainL^ = RL^ T^ / (1 + delta), so rl = RL T with El = RL ET + u RL T whenever that is below the chain's El.
  state  rr' = max(0, rr - s), Er' = Er + Es + u rr';  rl' = max(0, rl - RL U), El' = El + RL EU + u RL U + RL
       round(U) + u rl' (EU: the weights' error in U; u RL U: the product ratioL * e of P3; max(0, .) is
       1-Lipschitz).  P3 of a level is thereby checked by the next level's P1, and by the end comparison.
  L    the same identity read as a comparison of its own, in units of multiL: RL T against the chain's rl, bound El + RL ET
       + u RL T.  It is what shows a P3 that went wrong where nothing is shipped any more (U = 0 hides it from P1).
  end  rl as the last P1 read it against slot 0's remainL (bound El), rr after the last P2 against remainR (bound Er').
Two caps keep the error terms from feeding on themselves: a remainder lies in [0, what it was], so Er' <= rr + Er and El' <=
rl + El, and ratioR lies in [0, remainR], so P2's bound is at most rr + Er.  T^ >= EPS (1 - 2 u) whatever the columns hold.
Where a bound comes out large -- a row that divides by the crumbs of all but consumed columns -- the element IS
ill-conditioned, in the kernels as in any fp32 evaluation; no element is excluded, the bound says what it is worth.
Every error is taken less half the spacing of the STORED fp32 number (`excess`): the last rounding of a stored value at its
exact size, so that a comparison which is nothing but that rounding reads 0 instead of anything up to 1 (u x is the envelope
of half a spacing, reached just above a power of two); the bounds keep their own rounding terms.
Every bound gets REF_ABS = 1e-12 of a unit mass for the float64 arithmetic of the replay itself.

`match`, the cost and the gradients have no chain behind them: match[l][k] = sum_v e_v RL_v[k] RR_v[l] from the stored
vectors.  A term errs by its weight's error -- with 4 h + 3 u in place of h, because am_match and emd_fused take an odd
level's weight as the next one's squared twice -- plus u (ratioL * e) and the chain's rounding, sum_v min(t_v, u match).
The cost's and the gradients' terms add W_GEOM = 8 u (the distance: 2.5 u from d2, a square root or reciprocal square
root of at most 2 u, the difference's u, a product, the fma), and their sums pass through at most (terms of a row or
column) + 64 roundings of at most u * (sum of |terms|).

MEASURED
  v_exp_f32 (MI355X, rf_probe_exp2, 2 000 161 arguments over [-160, 0]): max relative error 8.271e-08 = 1.39 u where the result
  is a normal number (h = 2 u covers it); results below 2^-126 come back as +0 (max absolute error 1.000 * 2^-126 = E_FLOOR).
  CPU, the fp32 numpy restatement against this replay (tests/test_approxmatch_replay_host.py, every input of the GPU test):
  largest ratio 0.26 (P1 0.26, P2 0.20, L 0.26, end 0.21 / 0.25); its own `match` chain 0.62 of the entry bound; the float64
  schedule replays itself at 4e-10.  Planted omissions: smallest ratio 59 wherever a well-conditioned point moves >= 1e-3 of a
  unit mass through the omitted points (p2 at level 7 of 780 x 260, 9.0e-3 of a unit mass), typically 1e3 .. 1e12.
  MI355X, largest replay ratio per route (tests/test_gpu_emd_levels.py): dense pipeline 0.24, live sets 0.25, sorted and masked
  sweeps 0.26, the same batches pinned to RF_EMD_SWEPT 0.26, schedules 0.22 (513 x 700) / 0.22 (300 x 257), ragged 0.24,
  earth_mover 0.23 -- none between 0.5 and 1.0.  `match` entries at most 0.61 of their bound (recorded: between 0.5 and 1.0, the
  squared weights of am_match take 5 ulp of the 11 u a term is allowed), cost 0.005, gradients 0.063.
  With the library built from a local edit that ends the last column segment of am_rowl_kernel one sub-chunk (8 columns) early
  at level 1, the GPU test fails in its four cases whose set 1 fills its padding (512, 640, 2048 points) and names (1, "P2")
  at ratios 6e2 .. 4e4; with level 2's term left out of am_match_any_kernel the fourteen schedule cases on that kernel fail at
  `match` entries 1e5 .. 2e7 bounds off.
"""
import os
import re

import numpy as np

U32 = 2.0 ** -24
A_ARG = 7.25
H_EXP2 = 2.0 ** -23
E_FLOOR = 2.0 ** -126
COMBINE = 16
W_GEOM = 8 * U32
REF_ABS = 1e-12
LOG2E = float(np.log2(np.e))
KLOG2E = np.float32(1.44269502)  # approxmatch.hip kLog2e
EPS = float(np.float32(1e-9))    # the kernels' (and the oracle's) 1e-9f
SHARP_RANGE = float(np.sqrt(161.0 / (16384.0 * LOG2E)))  # beyond it the sharpest reference level's weight is exactly 0
FAULTS = ("p1", "p2", "p3", "match")
OMIT = 16


def kernel_constants():
    """{name: value} of approxmatch.hip's layout constants, read from the source so that the slicing moves with it."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rfnet_amd", "csrc", "approxmatch.hip")
    src = open(path).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+([A-Z_0-9]+)\s*=\s*(\d+)\s*[;,]", src)}
    for name in ("CPAD", "SUB", "AM_SMALL"):
        assert name in found, f"{name} is not a constexpr int of approxmatch.hip any more"
    return found


def default_levels():
    return [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]


def multipliers(n, m):
    """multiL, multiR of tf_approxmatch.cu:4-10 (am_multi) from a sample's counts."""
    return float(max(1, m // n)), float(max(1, n // m))


def _d2(a, c, dtype):
    """(m, n) squared distances; float32: rf::d2_fma's three roundings on the fp32 differences."""
    if dtype == np.float64:
        a, c = a.astype(np.float64), c.astype(np.float64)
        return ((c[:, None, :] - a[None, :, :]) ** 2).sum(-1)
    d = (c.astype(np.float32)[:, None, :] - a.astype(np.float32)[None, :, :]).astype(np.float64)  # (products of fp32 are exact in float64)
    t = (d[..., 1] * d[..., 1]).astype(np.float32).astype(np.float64)
    t = (d[..., 0] * d[..., 0] + t).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + t).astype(np.float32)


def _weights(d2, level, dtype):
    if level == 0.0:
        return np.ones(d2.shape, dtype)
    if dtype == np.float64:
        return np.exp(level * d2)
    c = np.float32(np.float32(level) * KLOG2E)
    return np.exp2((d2 * c).astype(np.float32)).astype(np.float32)


def schedule(a, c, levels, dtype=np.float64, fault=None, upto=None):
    """One sample's annealing schedule in `dtype` -> dict(RL (nlv, n), RR (nlv, m), rl_last, rr_last, match (m, n)).
    rl_last: remainL as the last level's P1 read it; rr_last: remainR after the last P2 (the kernels' slot 0).
    fault = (level, kind) plants one omission at that level: "p1" the last 16 columns out of P1's sum, "p2" the last 16
    points of set 1 out of P2's, "p3" the last 16 columns out of P3's, "match" the level's term missing from `match` for
    the rows of set 1 whose ratioL at that level is below the median.  upto: stop behind that many levels."""
    dt = np.dtype(dtype).type
    n, m = len(a), len(c)
    d2 = _d2(a, c, dt)
    mL, mR = multipliers(n, m)
    rl, rr = np.full(n, mL, dt), np.full(m, mR, dt)
    eps = dt(EPS)
    levels = list(levels)[:upto]
    RL, RR = np.zeros((len(levels), n), dt), np.zeros((len(levels), m), dt)
    match = np.zeros((m, n), dt)
    rl_in = rl
    for v, lv in enumerate(levels):
        kind = fault[1] if fault is not None and fault[0] == v else None
        e = _weights(d2, lv, dt)
        ecols = m - OMIT if kind == "p1" else m
        ratio_l = (rl / (eps + (e[:ecols] * rr[:ecols, None]).sum(0, dtype=dt))).astype(dt)
        epts = n - OMIT if kind == "p2" else n
        s = ((e[:, :epts] * ratio_l[None, :epts]).sum(1, dtype=dt) * rr).astype(dt)
        ratio_r = (rr * np.minimum(rr / (s + eps), dt(1))).astype(dt)
        rr = np.maximum(dt(0), rr - s).astype(dt)
        p = (e * ratio_l[None, :]).astype(dt).astype(np.float64) * ratio_r[:, None]  # (float64: exact for fp32 factors -- the fma's product)
        RL[v], RR[v] = ratio_l, ratio_r
        keep = ratio_l >= np.median(ratio_l) if kind == "match" else np.ones(n, bool)
        match = (match + p * keep[None, :]).astype(dt)
        p = p.astype(dt)
        rl_in = rl
        pcols = m - OMIT if kind == "p3" else m
        rl = np.maximum(dt(0), rl - p[:pcols].sum(0, dtype=dt)).astype(dt)
    return dict(RL=RL, RR=RR, rl_last=rl_in, rr_last=rr, match=match)


def layout(n, m, nlevels):
    cpad = kernel_constants()["CPAD"]
    npad, mpad = -(-n // cpad) * cpad, -(-m // cpad) * cpad
    V = npad + mpad
    return npad, mpad, V, (1 + nlevels) * V


def read_vectors(ws, b, n, m, nlevels, lengths=None):
    """Slice the vector region of a workspace (a float32 numpy array from its start) -> a list of b dicts
    (RL, RR, rl_last, rr_last), each cut to the sample's counts; asserts that every padded entry of every slot -- behind n / m,
    and (lengths) behind a ragged sample's counts -- is 0."""
    npad, mpad, V, bstride = layout(n, m, nlevels)
    ws = np.asarray(ws, np.float32)
    assert ws.size >= b * bstride
    out = []
    for bi in range(b):
        slots = ws[bi * bstride:(bi + 1) * bstride].reshape(1 + nlevels, V)
        n1, m1 = (n, m) if lengths is None else (int(lengths[0][bi]), int(lengths[1][bi]))
        L, R = slots[:, :npad], slots[:, npad:]
        assert (L[:, n1:] == 0).all() and (R[:, m1:] == 0).all(), f"sample {bi}: a padded entry of the vector region is not 0"
        out.append(dict(RL=L[1:, :n1].copy(), RR=R[1:, :m1].copy(), rl_last=L[0, :n1].copy(), rr_last=R[0, :m1].copy()))
    return out


def cheap_invariants(vec, n, m):
    """What every sample's vectors must satisfy whatever the clouds: finite, 0 <= ratioR <= multiR, ratioL >= 0, a
    column at exactly 0 stays there (ratioR_v == 0 behind the level that consumed it), remainR consistent with that."""
    mL, mR = multipliers(n, m)
    RL, RR = vec["RL"], vec["RR"]
    assert np.isfinite(RL).all() and np.isfinite(RR).all()
    assert (RL >= 0).all() and (RR >= 0).all() and (RR <= mR).all()
    assert (vec["rl_last"] >= 0).all() and (vec["rl_last"] <= mL).all()
    assert (vec["rr_last"] >= 0).all() and (vec["rr_last"] <= mR).all()
    dead = np.zeros(RR.shape[1], bool)
    for v in range(RR.shape[0]):
        # (ratioR = rem * min(rem / (t + 1e-9), 1) is 0 for rem = 0 -- for good -- or where rem^2 / t underflows: rem < 1e-23)
        assert (RR[v][dead] <= 1e-20).all(), f"level {v}: a column that was consumed has ratioR != 0"
        dead |= RR[v] == 0
    assert (vec["rr_last"][dead] <= 1e-20).all()


def _rounding(terms, total, axis):
    """sum_i min(t_i, u S) + COMBINE u S along `axis` (module docstring)."""
    cap = U32 * total
    capb = cap[None, :] if axis == 0 else cap[:, None]
    return np.minimum(terms, capb).sum(axis) + COMBINE * cap


def _weight_pair(d2, level, h):
    """float64 weights e = exp(level * d2) and their error bound de."""
    if level == 0.0:
        return np.ones_like(d2), np.zeros_like(d2)
    e = np.exp(level * d2)
    x = np.abs(level * LOG2E * d2)
    return e, e * (np.log(2.0) * A_ARG * U32 * x + h) + E_FLOOR


def excess(stored, expected):
    """|stored - expected| less half the spacing of the stored fp32 number: what is left of a difference once the last rounding
    of the stored value is taken off at its exact size (so that a comparison which is nothing but that rounding reads 0)."""
    stored = np.asarray(stored, np.float64)
    return np.maximum(0.0, np.abs(stored - expected) - 0.5 * np.spacing(np.abs(stored).astype(np.float32)).astype(np.float64))


def ratio_of(stored, expected, bound):
    """(max of excess / bound, its flat position); a difference where the bound is 0 counts as infinite."""
    return _worst(np.ravel(excess(stored, expected)), np.ravel(np.broadcast_to(bound, np.shape(expected))))


def _worst(err, bound):
    r = np.where(err <= bound, 0.0, np.inf)
    np.divide(err, bound, out=r, where=bound > 0)
    i = int(np.argmax(r))
    return float(r[i]), i


def replay(a, c, levels, RL, RR, rl_last=None, rr_last=None, lengths=None, h=H_EXP2, detail=False):
    """The teacher-forced float64 replay of one sample (module docstring) -> {(level, "P1" | "P2") and ("end", "rl" | "rr"):
    (max of error / bound, its position)}.  lengths = (count1, count2): a ragged sample -- the replay runs on the slices,
    multipliers from the counts.  Without rl_last / rr_last (a run cut short) the end comparisons are left out.
    detail: -> (that dict, {key: (err, bound) arrays})."""
    if lengths is not None:
        a, c = a[:lengths[0]], c[:lengths[1]]
        RL, RR = RL[:, :lengths[0]], RR[:, :lengths[1]]
    n, m = len(a), len(c)
    mL, mR = multipliers(n, m)
    d2 = _d2(a, c, np.float64)
    RL, RR = np.asarray(RL, np.float64), np.asarray(RR, np.float64)
    rl, rr = np.full(n, mL), np.full(m, mR)
    El, Er = np.zeros(n), np.zeros(m)
    out, det = {}, {}

    def put(key, stored, expected, scale, bound):
        # (a stored fp32 number is known to half its spacing: that much is taken off the error at its exact size, so a
        # comparison that is nothing but the last rounding has ratio 0; the bounds keep their own rounding terms)
        err = excess(stored, expected) * scale
        out[key] = _worst(err, bound)
        if detail:
            det[key] = (err, bound)

    rl_in, El_in = rl, El
    for v, lv in enumerate(list(levels)[:len(RL)]):
        e, de = _weight_pair(d2, float(lv), h)
        gl, gr = RL[v], RR[v]
        # ---- P2 (with the chain's rr), then the anchoring of rr
        S = e @ gl
        ES = de @ gl + _rounding(e * gl[None, :], S, 1)
        s = S * rr
        Es = ES * rr + S * Er + ES * Er + U32 * s
        want = rr * np.minimum(rr / (s + EPS), 1.0)
        put((v, "P2"), gr, want, 1.0 / mR, (np.minimum(2 * Er + Es + 4 * U32 * want, rr + Er) + REF_ABS) / mR)
        one = rr - Er > (s + Es + EPS) * (1 + 2 * U32)
        rr = np.where(one, gr, rr)
        Er = np.where(one, 0.0, Er)
        # ---- P1 in shipped mass, then the anchoring of rl
        T = EPS + rr @ e
        ET = rr @ de + Er @ e + _rounding(e * rr[:, None], T, 0)
        Tlo = np.maximum(T - ET, EPS * (1 - 2 * U32))  # (the kernel's sum starts at EPS and adds non-negative terms)
        U = gr @ e
        exp_l = rl / T
        b1 = U32 * exp_l + El / Tlo + exp_l * ET / Tlo
        put((v, "P1"), gl, exp_l, U / mL, (b1 * U + REF_ABS) / mL)
        rl_in, El_in = rl, El
        Eb = gl * ET + U32 * gl * T
        put((v, "L"), gl * T, rl, 1.0 / mL, (El + Eb + REF_ABS) / mL)
        tighter = Eb < El
        rl = np.where(tighter, gl * T, rl)
        El = np.where(tighter, Eb, El)
        # ---- state
        s2 = S * rr  # (with the anchored rr)
        Es2 = ES * rr + S * Er + ES * Er + U32 * s2
        gone = s2 - Es2 > (rr + Er) * (1 + 2 * U32)
        nr = np.maximum(0.0, rr - s2)
        Er = np.where(gone, 0.0, np.minimum(Er + Es2 + U32 * nr, rr + Er))
        rr = np.where(gone, 0.0, nr)
        A = gl * U
        EA = gl * (gr @ de) + U32 * A + gl * _rounding(e * gr[:, None], U, 0)
        nl = np.maximum(0.0, rl - A)
        El = np.minimum(El + EA + U32 * nl, rl + El)
        rl = nl
    if rl_last is not None:
        put(("end", "rl"), np.asarray(rl_last, np.float64)[:n], rl_in, 1.0 / mL, (El_in + REF_ABS) / mL)
    if rr_last is not None:
        put(("end", "rr"), np.asarray(rr_last, np.float64)[:m], rr, 1.0 / mR, (Er + REF_ABS) / mR)
    return (out, det) if detail else out


def worst_ratio(res):
    """(ratio, key, position) of the worst comparison of a replay."""
    key = max(res, key=lambda k: res[k][0])
    return res[key][0], key, res[key][1]


def match_from_vectors(a, c, levels, RL, RR, h=H_EXP2, with_terms=False):
    """match[l][k] = sum_v e_v RL_v[k] RR_v[l] in float64 from the stored vectors -> (match (m, n), bound (m, n))."""
    d2 = _d2(a, c, np.float64)
    RL, RR = np.asarray(RL, np.float64), np.asarray(RR, np.float64)
    mt, werr, terms = np.zeros_like(d2), np.zeros_like(d2), []
    for v, lv in enumerate(list(levels)[:len(RL)]):
        e, de = _weight_pair(d2, float(lv), 4 * h + 3 * U32)
        w = RL[v][None, :] * RR[v][:, None]
        t = e * w
        mt += t
        werr += de * w + (U32 * t if lv != 0.0 else 0.0)
        terms.append(t)
    rnd = np.zeros_like(d2)
    for t in terms:
        rnd += np.minimum(t, U32 * mt)
    return mt, werr + rnd + REF_ABS


def cost_from_vectors(a, c, match, mbound):
    """sum match * sqrt(d2) in float64 -> (cost, bound)."""
    dist = np.sqrt(_d2(a, c, np.float64))
    t = match * dist
    cost = float(t.sum())
    depth = match.shape[0] + 64
    return cost, float((mbound * dist).sum() + W_GEOM * cost + depth * U32 * cost + REF_ABS)


def grads_from_vectors(a, c, match, mbound):
    """The two match_cost_grad sums, with the kernels' max(d2, 1e-20) guard -> (grad1 (n, 3), bound1, grad2 (m, 3), bound2)."""
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    diff = a64[None, :, :] - c64[:, None, :]  # (m, n, 3): x1 - x2
    q = 1.0 / np.sqrt(np.maximum((diff ** 2).sum(-1), 1e-20))
    t = diff * (match * q)[..., None]
    at = np.abs(t)
    tb = np.abs(diff) * (mbound * q)[..., None] + W_GEOM * at
    m, n = match.shape
    g1, g2 = t.sum(0), -t.sum(1)
    b1 = tb.sum(0) + (m + 64) * U32 * at.sum(0) + REF_ABS
    b2 = tb.sum(1) + (n + 64) * U32 * at.sum(1) + REF_ABS
    return g1, b1, g2, b2


def paired_clouds(rng, n, m, kind="jitter"):
    """Two clouds (n, 3), (m, 3) float32, both drawn around the same sites so that every point of one set has a partner of the
    other within SHARP_RANGE -- the last 16 points of both sets included, which are what the planted faults leave out -- and
    neither set is ordered by site.  A site holds at least one point of each set.
      jitter      sites in the unit cube, every point its site + a uniform offset of at most 0.01 per coordinate (partners
                  within 0.035);
      duplicates  as jitter, but half of the points of both sets sit exactly on their site: exact ties, d2 = 0;
      lopsided    four clusters of sites: halves 24 units apart along x, each split into quarters 5.5 units apart along y.  The
                  two sets put their surplus points on different quarters (set 1: 50 / 10 / 30 / 10 %, set 2: 10 / 30 / 10 /
                  50 %), so a quarter keeps the excess of one set while the levels act locally, the quarters of a half meet
                  at the broadest non-zero reference level (-1/4: exp(-7.6) across, against exp(-30) one level earlier) and
                  the halves only at the last level (exp(-144) is exactly +0 in the kernels): both sets hold mass at
                  every level of the reference schedule, the last included."""
    assert kind in ("jitter", "duplicates", "lopsided")
    nsites = max(8, min(n, m) // 3)
    sites = rng.random_sample((nsites, 3)) * 0.96 - 0.48
    q = nsites // 4
    if kind == "lopsided":
        sites[: 2 * q, 0] += 24.0
        sites[:q, 1] += 5.5
        sites[2 * q: 3 * q, 1] += 5.5
    lo = np.array([0, q, 2 * q, 3 * q]), np.array([q, 2 * q, 3 * q, nsites])

    def draw(cnt, first):
        extra = cnt - nsites
        if kind == "lopsided":
            quarter = rng.choice(4, extra, p=[0.5, 0.1, 0.3, 0.1] if first else [0.1, 0.3, 0.1, 0.5])
            own = lo[0][quarter] + (rng.random_sample(extra) * (lo[1] - lo[0])[quarter]).astype(int)
        else:
            own = rng.randint(0, nsites, extra)
        own = np.concatenate([rng.permutation(nsites), own])
        rng.shuffle(own)
        off = rng.random_sample((cnt, 3)) * 0.02 - 0.01
        if kind == "duplicates":
            off[rng.random_sample(cnt) < 0.5] = 0.0
        return (sites[own] + off).astype(np.float32), own

    a, sa = draw(n, True)
    c, sc = draw(m, False)
    assert np.isin(sa, sc).all() and np.isin(sc, sa).all()  # every point has a partner: its site holds a point of the other set
    return a, c


def sample_clouds(seed, i, n, m, kind):
    """Sample i of the batch `seed`: every sample from its own stream, so that the host tests can make the few they replay."""
    return paired_clouds(np.random.RandomState([seed, i]), n, m, kind)


def batch_clouds(seed, b, n, m, kind):
    pairs = [sample_clouds(seed, i, n, m, kind) for i in range(b)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def replayed_samples(b):
    """The samples of a batch that are replayed: the first, the middle one and the last."""
    return sorted({0, b // 2, b - 1})


def _ladder(nlv):
    """nlv levels: a geometric ladder from -16384 to -0.25, then 0."""
    return [float(np.float32(-(16384.0 * (0.25 / 16384.0) ** (i / (nlv - 2.0))))) for i in range(nlv - 1)] + [0.0]  # (fp32 numbers: the op takes fp32 levels)


_REF = default_levels()
SCHEDULES = {
    "1": _REF[:1], "2": _REF[:2], "3": _REF[:3], "4": _REF[:4],
    "reference": None,  # (passed to the library as NULL, 0)
    "ten_off_chain": [-10000.0, -3000.0, -1000.0, -300.0, -100.0, -30.0, -10.0, -3.0, -1.0, 0.0],
    "ten_last_nonzero": _REF[:9] + [-0.0625],
    "17": _ladder(17), "33": _ladder(33), "49": _ladder(49),
    "fifty": [v for v in _REF for _ in range(5)],
    "repeated": _REF[:3] + [_REF[3]] * 2 + _REF[4:],
    "zero_inside": [-16384.0, -1024.0, 0.0, -64.0, -4.0, 0.0],
}

# (route, b, n, m, kind): tests/test_gpu_emd_levels.py runs them, tests/test_approxmatch_replay_host.py calibrates and mutates
# the same inputs.  The seed of a case is its position in its table.
DENSE = [(2, 300, 257, "jitter"), (2, 257, 300, "duplicates"), (1, 260, 780, "lopsided"), (1, 780, 260, "lopsided"),
         (2, 301, 450, "lopsided")]
LIVE = [(2, 512, 512, "lopsided"), (1, 513, 700, "jitter"), (1, 640, 2048, "lopsided"), (1, 2048, 640, "duplicates"),
        (1, 4100, 520, "lopsided")]
SORTED = [(229, 512, 512, "jitter"), (41, 1000, 1500, "lopsided")]
SCHEDULE_SHAPES = [(1, 513, 700, "lopsided"), (2, 300, 257, "lopsided")]
RAGGED = (3, 700, 600, "lopsided", [700, 513, 257], [600, 300, 599])
EARTH_MOVER = [(2, 513, 700, "lopsided"), (2, 300, 257, "jitter")]


def case_seed(table, idx):
    return {"dense": 100, "live": 200, "sorted": 300, "schedule": 400, "ragged": 500, "emd": 600}[table] + idx


T_MIN = 1e-3


def carried(a, c, levels, sch):
    """From a (float64) run of the schedule: per level, the most mass that a single well-conditioned point ships or receives
    through the points a planted fault leaves out -- {"p1" | "p2" | "p3": array over levels}.
      p1, p3  max over the rows k of set 1 whose sum T[k] = sum_l e rr[l] is at least T_MIN (a row that divides by crumbs --
              every column in its reach all but consumed -- has a ratioL that hangs on the last bits of those crumbs, in the
              kernels as in any fp32 evaluation, and the replay's bound says so) of sum over the last 16 columns of
              e RL[k] RR[l]: what the row ships to them (P1 divides by a sum that lacks them, P3 fails to subtract it);
      p2      max over the columns l that stay live behind this level with the clamp at 1 (s + EPS < rr and rr - s >= T_MIN:
              their new remainder is a plain difference, not a cancellation) of what l receives from the last 16 points."""
    d2 = _d2(a, c, np.float64)
    mL, mR = multipliers(len(a), len(c))
    rr = np.full(len(c), mR)
    out = {k: np.zeros(len(levels)) for k in ("p1", "p2", "p3")}
    for v, lv in enumerate(levels):
        e = np.ones_like(d2) if lv == 0.0 else np.exp(lv * d2)
        p = e * sch["RL"][v][None, :] * sch["RR"][v][:, None]
        sound = rr @ e >= T_MIN
        out["p1"][v] = out["p3"][v] = (p[-OMIT:].sum(0) * sound).max()
        s = (e @ sch["RL"][v]) * rr
        plain = (s + EPS < rr) & (rr - s >= T_MIN)
        out["p2"][v] = (p[:, -OMIT:].sum(1) * plain).max()
        rr = np.maximum(0.0, rr - s)
    return out
