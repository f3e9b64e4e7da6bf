"""numpy float64 restatements of the Chamfer gradients and the fused loss ops (NnDistanceGrad, the mean-sqrt loss and its
backward, merge_layer and its three gradients), the derived error bounds of their fp32 kernels (nn_grad_kernel in
nn_distance.hip, grad_tile in nn_pruned.hip, chamfer_loss_reduce_kernel / merge_pull_kernel / merge_pull_grad_kernel in
chamfer_ext.hip), a model of the launch routes, and the input families of tests/test_gpu_chamfer_grad.py.  Nothing here
follows a kernel's indexing: every function is the operation as include/rfops.h and the kernels' header comments state
it.  tests/test_chamfer_grad_ref_host.py checks these functions against independent formulations on the CPU.

Two input families:
  A  coordinates and upstream gradients on a dyadic grid on which every fp32 product and every partial sum of any order is
     exact: nn_grad_exact computes in int64, PROVES the exactness (the sum of the magnitudes of all terms of an element, in
     grid units, stays below 2^24) and returns the one fp32 result every correct kernel must give bit for bit.
  B  randn / dup / collapsed / same clouds against the float64 functions under the bounds K U mag derived below
     (U = 2^-24, the fp32 unit roundoff; mag the sum of the magnitudes of the terms that enter the element)."""
import os
import re

import numpy as np

U = 2.0 ** -24
EXACT_LIMIT = 2 ** 24            # integers below it are fp32 numbers
C_EPS = float(np.float32(1e-8))  # merge_layer's 1e-8f: the op is defined on fp32 tensors
# expf: the HIP math documentation shipped with the ROCm install states no error for expf, so 2 ulp are allowed here
# (the device library's own tables claim less); the measured worst error against float64 exp of the same fp32
# argument is recorded in profiles/chamfer_grad_bounds.txt (tools/chamfer_grad_ratios.py: 0.815 ulp, 1.000 where the
# result is subnormal).
EXPF_ULP = 2.0
# Below the normal range (s / c above 87.3) fp32 errors are absolute: expf's EXPF_ULP ulp are EXPF_ULP 2^-149 there, and
# every operation whose result is subnormal loses up to half the subnormal spacing, 2^-150, whatever the result's size.
RATIO_FLOOR = EXPF_ULP * 2.0 ** -149
UNDER = 2.0 ** -150
RATIO_ZERO_ABOVE = 104.0         # exp(-x) < 2^-150 for x > 103.98: expf gives exactly 0


def _csrc(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rfnet_amd", "csrc", name)).read()


def kernel_constants():
    """{name: value} of the constants the routes depend on, read from the sources so that the shapes of the tests move
    with the kernels: GT, GTPB (nn_distance.hip), GS_GT, RFP_GS_WG, SB (= BS * SBB), RFP_SORT_SPLIT, RFP_SORT_SPLIT_ABOVE,
    RPT, STPB (nn_pruned.hip), LR_TPB, MG_TPB (chamfer_ext.hip)."""
    found = {}
    for fname, names in (("nn_distance.hip", ("GT", "GTPB")),
                         ("nn_pruned.hip", ("GS_GT", "BS", "SBB", "RPT", "STPB", "RFP_GS_WG", "RFP_SORT_SPLIT",
                                            "RFP_SORT_SPLIT_ABOVE", "RFP_GS_SEG")),
                         ("chamfer_ext.hip", ("LR_TPB", "MG_TPB"))):
        src = _csrc(fname)
        for name in names:
            mt = re.search(r"(?:constexpr\s+int\s+%s\s*=|#define\s+%s\s)\s*(\d+)\b" % (name, name), src)
            assert mt, f"{name} is not a constant of {fname} any more"
            found[name] = int(mt.group(1))
    assert re.search(r"constexpr\s+int\s+SB\s*=\s*BS\s*\*\s*SBB\s*;", _csrc("nn_pruned.hip")), "SB is not BS * SBB any more"
    found["SB"] = found["BS"] * found["SBB"]
    return found


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ route model ---------------------------------------------
def grad_route(b, n, m, k=None):
    """Per direction (gt, tiles, slices, points in the last tile) of rfd::nn_distance_grad: direction 1 has the n points
    of xyz1 as destinations and the m points of xyz2 as sources.  tile_for: 64..GT destinations per tile so that
    b * tiles >= 256; slices_for: sources split only when even that leaves fewer than 256 workgroups, >= 1024 a slice."""
    k = k or kernel_constants()

    def one(nd, ns):
        want = (nd * b + 255) // 256
        gt = min(max(_cdiv(want, 64) * 64, 64), k["GT"])
        tiles = _cdiv(nd, gt)
        slices = min(max(_cdiv(256, b * tiles), 1), max(ns // 1024, 1))
        return gt, tiles, slices, nd - (tiles - 1) * gt
    return one(n, m), one(m, n)


def culled_pays(b, n, m):
    """nn_distance.hip culled_pays: the shapes whose rf_chamfer_step runs the sorted-space backward."""
    lo, hi = min(n, m), max(n, m)
    if b <= 0 or lo < 512 or hi > 65536 or n * m < (1 << 21):
        return False
    pairs = b * n * m
    if hi <= 4096:
        return pairs >= (1 << 24)
    if hi <= 16384:
        return pairs >= (1 << 27)
    return pairs >= 44000 * hi


def step_route(b, n, m, k=None):
    """(culled?, per set (npad, bucket, gt, tiles)) of rf_chamfer_step: npad_of and pruned_step of nn_pruned.hip.  A set is
    padded to whole superblocks of SB records (one more when its sort is split), cut into 64 buckets, and a tile is a
    whole number of buckets, at most GS_GT records, aiming at RFP_GS_WG workgroups per set."""
    k = k or kernel_constants()

    def one(np_):
        split = k["RFP_SORT_SPLIT"] if (k["RFP_SORT_SPLIT"] > 1 and k["RFP_SORT_SPLIT_ABOVE"] < np_ <= k["RPT"] * k["STPB"]) else 1
        npad = _cdiv(np_, k["SB"]) * k["SB"] + (split - 1) * k["SB"]
        q = _cdiv(npad, 64)
        nbk = max(_cdiv(_cdiv(npad * b, k["RFP_GS_WG"]), q), 1)
        while nbk > 1 and nbk * q > k["GS_GT"]:
            nbk -= 1
        return npad, q, nbk * q, _cdiv(npad, nbk * q)
    return culled_pays(b, n, m), (one(n), one(m))


# (b, n, m) -> direction 1 and 2 as (gt, tiles, slices, points in the last tile): the shapes of
# test_gpu_chamfer_grad.py and the routes they are there for, computed from the constants as they were when the table was written;
# test_chamfer_grad_ref_host.py names the shapes that no longer cover their route when a constant changes
GRAD_SHAPES = {
    (1, 1, 1): ((64, 1, 1, 1), (64, 1, 1, 1)),
    (3, 130, 1): ((64, 3, 1, 2), (64, 1, 1, 1)),
    (300, 70, 33): ((128, 1, 1, 70), (64, 1, 1, 33)),
    (1, 100, 4096): ((64, 2, 4, 36), (64, 64, 1, 64)),
    (2, 3000, 2049): ((64, 47, 2, 56), (64, 33, 2, 1)),
    (1, 5, 2048): ((64, 1, 2, 5), (64, 32, 1, 64)),
    (33, 16001, 64): ((2048, 8, 1, 1665), (64, 1, 8, 64)),
    (40, 2048, 600): ((320, 7, 1, 128), (128, 5, 2, 88)),
}
# (b, n, m) -> per set (npad, bucket, gt, tiles) of the sorted-space step
STEP_SHAPES = {
    (8, 1024, 2048): ((1024, 16, 16, 64), (2048, 32, 32, 64)),
    (4, 2048, 2048): ((2048, 32, 32, 64), (2048, 32, 32, 64)),
    (16, 512, 4096): ((512, 8, 8, 64), (4096, 64, 64, 64)),
    (2, 8193, 8193): ((8320, 130, 130, 64), (8320, 130, 130, 64)),
}


# ------------------------------------------------------------------ the operations, float64 ----------------------------------
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def counts_of(lengths, b, n):
    """Per-sample counts as rf::ragged_count holds them: clamped into [1, n]; None = all rows."""
    if lengths is None:
        return np.full(b, n, np.int64)
    ln = np.asarray(lengths, np.int64)
    assert ln.shape == (b,)
    return np.clip(ln, 1, n)


def _scatter_both(a, c, w1, idx1, w2, idx2, cnt1, cnt2):
    """The two gradients and their magnitudes in the dtype of the inputs (float64 or int64), w = 2 gd.  Direction 1:
    t = w1[j] (a[j] - c[idx1[j]]) enters g1[j] with + and g2[idx1[j]] with -; direction 2 likewise.  Only the first
    cnt rows of a sample are read."""
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    g1, g2 = np.zeros((b, n, 3), a.dtype), np.zeros((b, m, 3), a.dtype)
    mag1, mag2 = np.zeros_like(g1), np.zeros_like(g2)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(b):
            ni, mi = int(cnt1[i]), int(cnt2[i])
            for own, oth, w, idx, go, gt_, mo, mt, no, nt in ((a, c, w1, idx1, g1, g2, mag1, mag2, ni, mi),
                                                              (c, a, w2, idx2, g2, g1, mag2, mag1, mi, ni)):
                if w is None:
                    continue
                kk = np.asarray(idx[i, :no], np.int64)
                assert kk.size == 0 or (kk.min() >= 0 and kk.max() < nt), "a valid source names a row outside the other count"
                t = w[i, :no, None] * (own[i, :no] - oth[i, kk])
                go[i, :no] += t
                mo[i, :no] += np.abs(t)
                np.add.at(gt_[i], kk, -t)
                np.add.at(mt[i], kk, np.abs(t))
    return g1, g2, mag1, mag2


def nn_grad(xyz1, xyz2, gd1, idx1, gd2, idx2, len1=None, len2=None):
    """NnDistanceGrad: grad_own[j] = 2 gd_own[j] (own_j - other[idx_own[j]]) - sum_{k: idx_other[k] == j} 2 gd_other[k]
    (other_k - own_j) -> (g1, g2, mag1, mag2) float64, mag the per-element sum of the magnitudes of all terms that
    enter the element.  gd1 / gd2 may be None (a direction that was not computed).  With counts only rows and sources
    inside a count contribute and rows behind a count are 0."""
    a, c = _f64(xyz1), _f64(xyz2)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    w1 = None if gd1 is None else 2.0 * _f64(gd1)
    w2 = None if gd2 is None else 2.0 * _f64(gd2)
    return _scatter_both(a, c, w1, idx1, w2, idx2, counts_of(len1, b, n), counts_of(len2, b, m))


def loss(dist1, dist2, len1=None, len2=None):
    """rf_chamfer_loss: mean over the sample's count of sqrt(dist), per sample and direction -> (loss (b, 2), mag (b, 2));
    a missing direction (None) gives 0.  mag is the same mean: every term is positive."""
    ref = dist1 if dist1 is not None else dist2
    b = ref.shape[0]
    out = np.zeros((b, 2))
    for col, (d, ln) in enumerate(((dist1, len1), (dist2, len2))):
        if d is None:
            continue
        cnt = counts_of(ln, b, d.shape[1])
        for i in range(b):
            out[i, col] = np.sqrt(_f64(d[i, :cnt[i]])).sum() / cnt[i]
    return out, out.copy()


def loss_gd(dist, gl_col, lengths=None):
    """The upstream gradient the loss backward builds per row: gl / count * 0.5 / sqrt(dist), float64; dist = 0 gives inf."""
    d = _f64(dist)
    cnt = counts_of(lengths, d.shape[0], d.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (_f64(gl_col) / cnt)[:, None] * 0.5 / np.sqrt(d)


def loss_grad(xyz1, xyz2, dist1, idx1, dist2, idx2, gl, len1=None, len2=None):
    """rf_chamfer_loss_grad: nn_grad with gd = gl[:, dir] / count * 0.5 / sqrt(dist); `dist` is a given fp32 array (it
    need not be a true distance); a direction whose dist is None contributes nothing."""
    gl = _f64(gl)
    gd1 = None if dist1 is None else loss_gd(dist1, gl[:, 0], len1)
    gd2 = None if dist2 is None else loss_gd(dist2, gl[:, 1], len2)
    return nn_grad(xyz1, xyz2, gd1, idx1 if dist1 is not None else None, gd2, idx2 if dist2 is not None else None, len1, len2)


def _merge_parts(raw, new, idx2, dec):
    raw, new = _f64(raw), _f64(new)
    g = np.take_along_axis(raw, np.asarray(idx2, np.int64)[..., None], 1)
    d = g - new
    s = (d * d).sum(-1)
    dec = float(np.float32(dec))
    c = C_EPS + dec * dec
    x = s / c
    with np.errstate(under="ignore"):
        ratio = np.exp(-x)
    return new, d, s, c, x, ratio, dec


def _ratio_k(x):
    """Relative error of the fp32 ratio in units of U.  d = fl(g - q) (1), its square (2 + 1), the two adds (2): s carries
    5 U; c = fl(1e-8f + fl(dec dec)) 2 U; the division 1 U: the argument s / c carries 8 U relative, which exp turns into
    8 (s / c) U; expf's own EXPF_ULP ulp are at most 2 EXPF_ULP U relative."""
    return 8.0 * x + 2.0 * EXPF_ULP


def _pad_new(arr, b, m, len_new):
    """Zero the rows of `arr` (b, m, ...) behind len_new."""
    cnt = counts_of(len_new, b, m)
    keep = np.arange(m)[None] < cnt[:, None]
    return np.where(keep.reshape(keep.shape + (1,) * (arr.ndim - 2)), arr, 0.0), keep


def _merge_forward_all(raw, new, idx2, dec, len_new=None):
    """(out, mag, bound) of merge_forward / merge_forward_bound."""
    q, d, s, c, x, ratio, _ = _merge_parts(raw, new, idx2, dec)
    rd = np.abs(ratio[..., None] * d)
    out, mag = q + ratio[..., None] * d, np.abs(q) + rd
    bound = U * ((_ratio_k(x)[..., None] + 2.0) * rd + mag) + RATIO_FLOOR * np.abs(d) + UNDER
    b, m = q.shape[:2]
    keep = _pad_new(out, b, m, len_new)[1][..., None]
    return np.where(keep, out, 0.0), np.where(keep, mag, 0.0), np.where(keep, bound, 0.0)


def merge_forward(raw, new, idx2, dec, len_new=None):
    """merge_layer's tail: g = raw[idx2], diff = g - q, c = 1e-8 + dec^2, ratio = exp(-|diff|^2 / c), out = q + ratio diff
    -> (out, mag) float64 (b, m, 3); mag = |q| + |ratio diff|; rows behind len_new are 0."""
    return _merge_forward_all(raw, new, idx2, dec, len_new)[:2]


def merge_forward_bound(raw, new, idx2, dec, len_new=None):
    """|fp32 out - float64 out| per element: ratio diff carries the ratio's error, diff's rounding and the product's,
    (_ratio_k + 2) U |ratio diff|; the add U mag; a ratio below the normal range RATIO_FLOOR |diff|, a subnormal product UNDER."""
    return _merge_forward_all(raw, new, idx2, dec, len_new)[2]


def merge_grad(raw, new, idx2, dec, go, len_raw=None, len_new=None):
    """rf_merge_layer_grad by the formulas above merge_pull_grad_kernel: g_ratio = go . diff, g_diff = ratio go -
    (2 ratio g_ratio / c) diff, grad_new = go - g_diff, grad_raw[idx2] += g_diff, grad_dec = 2 dec sum g_ratio ratio s / c^2
    -> ((grad_new (b, m, 3), grad_dec (b,), grad_raw (b, n, 3)), (their magnitudes)).  Only the first len_new new
    points of a sample take part; a stored index is held inside [0, len_raw) as the kernel holds it."""
    r = merge_grad_all(raw, new, idx2, dec, go, len_raw, len_new)
    return tuple(r[k][0] for k in ("grad_new", "grad_dec", "grad_raw")), tuple(r[k][2] for k in ("grad_new", "grad_dec", "grad_raw"))


def merge_grad_all(raw, new, idx2, dec, go, len_raw=None, len_new=None, mg_tpb=None):
    """merge_grad with its bounds: a dict of (value, bound, magnitude) for "grad_new", "grad_dec", "grad_raw", plus
    "terms" (the raw rows' term counts), "s", "x" = s / c, "idx" (the held indices) and "keep" (valid new rows).

    Bounds, in units of U, with GA = sum_c |go_c diff_c| and R = _ratio_k(s / c):
      g_ratio  each product carries diff's rounding and its own (2), the two adds 2: 4 U GA absolute
      k2       = 2 ratio g_ratio / c: R + 4 + product 1 + c 2 + division 1: (R + 8) U K2A, K2A = 2 ratio GA / c
      g_diff   ratio go (R + 1), k2 diff (R + 8 + 2), the subtraction 1: (R + 11) U F, F = |ratio go| + K2A |diff|
      grad_new err(g_diff) + U (|go| + F)
      grad_raw sum of err(g_diff) over the row's T terms + T U sum F (global fp32 atomics arrive in any order)
      grad_dec term g_ratio ratio s / (c c): 4 + R + 1 + s 5 + 1 + c c 5 + 1: (R + 17) U W, W = GA ratio s / c^2; the
               sum is ceil(count / MG_TPB) serial adds per thread, 6 butterfly levels, MG_TPB / 64 - 1 serial wave
               adds, and the product with 2 dec: D + 1 more U on sum W.
      Underflow (absolute, next to the relative terms above): the ratio's RATIO_FLOOR reaches g_diff through ratio go and
      through k2 diff, RATIO_FLOOR (|go| + 2 GA |diff| / c); the subnormal results of 2 ratio g_ratio (then divided by c and
      multiplied by diff), of the division, and of the two products lose UNDER each: UNDER (|diff| / c + |diff| + 2).
      grad_dec's term likewise: RATIO_FLOOR GA s / c^2 + UNDER ((s + 1) / c^2 + 1)."""
    mg_tpb = mg_tpb or kernel_constants()["MG_TPB"]
    b, n, m = raw.shape[0], raw.shape[1], new.shape[1]
    cr, cn = counts_of(len_raw, b, n), counts_of(len_new, b, m)
    idx = np.clip(np.asarray(idx2, np.int64), 0, (cr - 1)[:, None])
    q, d, s, c, x, ratio, dec = _merge_parts(raw, new, idx, dec)
    go = _f64(go)
    keep = (np.arange(m)[None] < cn[:, None])
    with np.errstate(invalid="ignore"):
        go = np.where(keep[..., None], go, 0.0)  # padded rows: their grad_out is not read
    R = _ratio_k(x)
    g_ratio, GA = (go * d).sum(-1), np.abs(go * d).sum(-1)
    K2A = 2.0 * ratio * GA / c
    f = ratio[..., None] * go - (2.0 * ratio * g_ratio / c)[..., None] * d
    F = np.abs(ratio[..., None] * go) + K2A[..., None] * np.abs(d)
    floor = RATIO_FLOOR * (np.abs(go) + 2.0 * GA[..., None] * np.abs(d) / c) + UNDER * (np.abs(d) / c + np.abs(d) + 2.0)
    ef = (R[..., None] + 11.0) * U * F + floor
    gn, bn = go - f, ef + U * (np.abs(go) + F)
    gn, bn = np.where(keep[..., None], gn, 0.0), np.where(keep[..., None], bn, 0.0)
    gr, br, sf, terms = np.zeros((b, n, 3)), np.zeros((b, n, 3)), np.zeros((b, n, 3)), np.zeros((b, n), np.int64)
    for i in range(b):
        k = idx[i, :cn[i]]
        np.add.at(gr[i], k, f[i, :cn[i]])
        np.add.at(br[i], k, ef[i, :cn[i]])
        np.add.at(sf[i], k, F[i, :cn[i]])
        np.add.at(terms[i], k, 1)
    br = br + terms[..., None] * U * sf
    W = np.where(keep, GA * ratio * s / (c * c), 0.0)
    w = np.where(keep, g_ratio * ratio * s / (c * c), 0.0)
    depth = np.array([_cdiv(int(v), mg_tpb) for v in cn]) + 6 + (mg_tpb // 64 - 1)
    gd = 2.0 * dec * w.sum(1)
    bd = abs(2.0 * dec) * (((R + 17.0) * U * W).sum(1) + (depth + 1) * U * W.sum(1)
                           + np.where(keep, RATIO_FLOOR * GA * s / (c * c) + UNDER * ((s + 1.0) / (c * c) + 1.0), 0.0).sum(1))
    mn = np.where(keep[..., None], np.abs(go) + F, 0.0)
    return {"grad_new": (gn, bn, mn), "grad_dec": (gd, bd, abs(2.0 * dec) * W.sum(1)), "grad_raw": (gr, br, sf), "terms": terms,
            "s": np.where(keep, s, np.nan), "x": np.where(keep, x, np.nan), "idx": idx, "keep": keep}


# ------------------------------------------------------------------ derived bounds -----------------------------------------
def k_plain(slices=1):
    """nn_grad_kernel, plain mode: per term the subtraction and the product round (gd + gd is exact): 2; the tile's sum
    is a double (its own roundings are 2^-29 of these); the cast of the tile to float 1 and the add of the own term 1.
    A sliced tile casts per slice (together U mag) and leaves through `slices` global fp32 adds: + slices."""
    return 4 + (slices if slices > 1 else 0)


def k_loss(slices=1):
    """Loss mode: the upstream gradient is built in fp32 -- the division by the count, sqrtf and the division (correctly
    rounded: the build sets -fno-fast-math; the product with 0.5 is exact): + 3 per term."""
    return k_plain(slices) + 3


def k_sorted():
    """grad_tile (rf_chamfer_step's sorted route): as the unsliced route, plus the four levels of the segmented fp32
    pre-sum of runs inside a 16-lane row (RFP_GS_SEG = 1)."""
    return k_plain(1) + 4


def k_loss_forward(cnt, lr_tpb=None):
    """chamfer_loss_reduce_kernel: sqrtf 1; per thread ceil(cnt / (4 LR_TPB)) adds into one of four partials, up to 3
    more in the tail loop and 2 for (a0 + a1) + (a2 + a3); 6 butterfly levels; LR_TPB / 64 - 1 serial wave adds; the
    division by the count 1.  All terms are positive: every add's error is at most U times the final sum."""
    lr_tpb = lr_tpb or kernel_constants()["LR_TPB"]
    return 1 + _cdiv(int(cnt), 4 * lr_tpb) + 3 + 2 + 6 + (lr_tpb // 64 - 1) + 1


def loss_bound(dist1, dist2, len1=None, len2=None):
    val, mag = loss(dist1, dist2, len1, len2)
    b = val.shape[0]
    kk = np.zeros((b, 2))
    for col, (d, ln) in enumerate(((dist1, len1), (dist2, len2))):
        if d is not None:
            kk[:, col] = [k_loss_forward(v) for v in counts_of(ln, b, d.shape[1])]
    return kk * U * mag


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements whose reference is a number (0 / 0 counts as 0), and the NaN masks'
    agreement."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    nan = np.isnan(ref)
    same = np.array_equal(np.isnan(got), nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(nan, 0.0, r)
    return (float(r.max()) if r.size else 0.0), same


def assert_within(got, ref, bound, what):
    """Every element: |got - ref| <= bound; where the reference is NaN the kernel's must be too, and nowhere else."""
    ratio, same = worst_ratio(got, ref, bound)
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}")
    assert same, f"{what}: NaN masks differ"
    if ratio > 1.0:
        g, r, bd = _f64(got), _f64(ref), _f64(bound)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(np.isnan(r) | (g == r), 0.0, np.abs(g - r) / bd)
        at = np.unravel_index(int(np.argmax(q)), q.shape)
        raise AssertionError(f"{what}: worst |got - ref| / bound = {ratio:.3f} at {at}: got {g[at]!r}, reference {r[at]!r}, "
                             f"bound {bd[at]!r}; {int((q > 1).sum())} of {q.size} elements outside")
    return ratio


# ------------------------------------------------------------------ family A: exact on a dyadic grid -----------------------
def _scaled(a, scale):
    s = _f64(a) * scale
    i = np.rint(s).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "input is not on the dyadic grid"
    return i


def nn_grad_exact(xyz1, xyz2, gd1, idx1, gd2, idx2, len1=None, len2=None, step=2.0 ** -6):
    """NnDistanceGrad for coordinates on the grid `step` and upstream gradients on the grid 1/4: (g1, g2) in fp32, proven
    exact.  A term 2 gd (own - other) is a multiple of step / 2, formed exactly (the difference of two grid numbers and
    its product with a small integer over 2).  If the sum of the magnitudes of an element's terms, in units of step / 2,
    is below 2^24, every partial sum of any order and grouping -- fp32 registers, the double tile, global fp32 atomics
    -- is a multiple of step / 2 below 2^24 step / 2: representable, no rounding anywhere.  Raises AssertionError when
    the proof fails."""
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    cnt1, cnt2 = counts_of(len1, b, n), counts_of(len2, b, m)

    def grid_rows(x, cnt, scale):  # rows behind a count may hold garbage (NaN): they are not read
        keep = np.arange(x.shape[1])[None] < cnt[:, None]
        with np.errstate(invalid="ignore"):
            return _scaled(np.where(keep.reshape(keep.shape + (1,) * (x.ndim - 2)), x, 0.0), scale)
    ia, ic = grid_rows(xyz1, cnt1, 1.0 / step), grid_rows(xyz2, cnt2, 1.0 / step)
    k1, k2 = grid_rows(gd1, cnt1, 4.0), grid_rows(gd2, cnt2, 4.0)
    g1, g2, mag1, mag2 = _scatter_both(ia, ic, k1, idx1, k2, idx2, cnt1, cnt2)
    worst = max(int(mag1.max()), int(mag2.max()))
    assert worst < EXACT_LIMIT, f"a partial sum could round: {worst} grid units in one element"
    unit = step / 2.0
    out = []
    for g in (g1, g2):
        f = (g.astype(np.float64) * unit).astype(np.float32)
        assert np.array_equal(f.astype(np.float64) / unit, g.astype(np.float64))
        out.append(f)
    return out[0], out[1]


def grid_clouds(rng, b, n, m, step=2.0 ** -6, span=2.0):
    """Two clouds with coordinates k step in [-span, span), float32."""
    kmax = int(round(span / step))
    return ((rng.randint(-kmax, kmax, size=(b, n, 3)) * step).astype(np.float32),
            (rng.randint(-kmax, kmax, size=(b, m, 3)) * step).astype(np.float32))


def grid_gd(rng, shape):
    """Upstream gradients k / 4, k in {+-1, +-2, +-3}, float32."""
    return (rng.choice([-3, -2, -1, 1, 2, 3], size=shape) * 0.25).astype(np.float32)


# ------------------------------------------------------------------ family B and the index patterns -------------------------
def clouds(kind, rng, b, n, m):
    """The cloud families of test_gpu_chamfer_step_sorted.py (its make()): randn; dup (resampled duplicates: exact ties,
    hubs); collapsed (the large cloud on ~120 spots); same (the same cloud on both sides: every winner at distance 0)."""
    from test_gpu_chamfer_step_sorted import make
    return make(kind, int(rng.randint(2 ** 31 - 1)), b, n, m)


PATTERNS = ("uniform", "perm", "hub_first", "hub_last", "runs")


def indices(pattern, rng, b, ns, nd, cnt_s=None, cnt_d=None):
    """(b, ns) int32: for each of a sample's cnt_s valid sources a destination row in [0, cnt_d); behind cnt_s garbage
    that stays inside [0, nd) and names padded rows too.
      uniform    random rows
      perm       a random permutation (cycled when there are more sources than rows)
      hub_first  every source names row min(1, cnt_d - 1): the first tile
      hub_last   every source names row cnt_d - 1: the last tile
      runs       ascending runs of 2 to 40 equal rows: what the segmented pre-sum and a sorted cloud see"""
    cnt_s = np.full(b, ns) if cnt_s is None else cnt_s
    cnt_d = np.full(b, nd) if cnt_d is None else cnt_d
    out = rng.randint(0, nd, size=(b, ns))
    for i in range(b):
        s, d = int(cnt_s[i]), int(cnt_d[i])
        if pattern == "uniform":
            v = rng.randint(0, d, size=s)
        elif pattern == "perm":
            v = np.concatenate([rng.permutation(d) for _ in range(_cdiv(s, d))])[:s]
        elif pattern == "hub_first":
            v = np.full(s, min(1, d - 1))
        elif pattern == "hub_last":
            v = np.full(s, d - 1)
        elif pattern == "runs":
            lens = rng.randint(2, 41, size=s // 2 + 1)
            rows = np.sort(rng.randint(0, d, size=lens.size))
            v = np.repeat(rows, lens)[:s]
        else:
            raise ValueError(pattern)
        out[i, :s] = v
    return out.astype(np.int32)


def ulp_distance(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref|."""
    got, ref64 = _f64(got), _f64(ref64)
    sp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return np.abs(got - ref64) / sp


def signed_gd(rng, shape):
    """Family B's upstream gradients: magnitudes in [0.25, 1.25), both signs."""
    return ((rng.rand(*shape) + 0.25) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def decade_dist(rng, shape):
    """Positive `dist` inputs of the loss backward, independent of the clouds, over ten decades (1e-8 to 1e2)."""
    return (10.0 ** rng.uniform(-8.0, 2.0, size=shape)).astype(np.float32)


def exact_case(rng, b, n, m, idx_of, len1=None, len2=None):
    """Family A inputs and the one correct fp32 answer: (a, c, gd1, idx1, gd2, idx2, g1, g2).  idx_of(a, c) -> (idx1,
    idx2).  The grid 2^-6 in [-2, 2) first; where its proof fails (a hub of very many terms) the grid 2^-5 in [-1, 1):
    the proof decides, and a case neither grid proves raises."""
    state = rng.get_state()
    for step, span in ((2.0 ** -6, 2.0), (2.0 ** -5, 1.0)):
        rng.set_state(state)
        a, c = grid_clouds(rng, b, n, m, step, span)
        gd1, gd2 = grid_gd(rng, (b, n)), grid_gd(rng, (b, m))
        idx1, idx2 = idx_of(a, c)
        try:
            g1, g2 = nn_grad_exact(a, c, gd1, idx1, gd2, idx2, len1, len2, step)
        except AssertionError as e:
            if "could round" not in str(e):
                raise
            continue
        return a, c, gd1, idx1, gd2, idx2, g1, g2
    raise AssertionError("no grid proves this case exact")


MERGE_DECS = (0.0, 1e-4, 0.07, -0.07, 1.0, 1e3)


def merge_case(rng, b, n, m, dec, pattern="uniform", len_raw=None, len_new=None):
    """(raw, new, idx2, go) float32 / int32 with coordinates in [-0.5, 0.5): a quarter of the new points are copies of the
    raw point idx2 names (s = 0), a quarter sit at the scale of the pull sqrt(c) from it (ratio neither 0 nor 1; none at
    dec = 0), the rest anywhere.  idx2 follows `pattern` (indices()) inside the counts."""
    raw = (rng.rand(b, n, 3) - 0.5).astype(np.float32)
    new = (rng.rand(b, m, 3) - 0.5).astype(np.float32)
    cr = None if len_raw is None else counts_of(len_raw, b, n)
    cn = None if len_new is None else counts_of(len_new, b, m)
    idx = indices(pattern, rng, b, m, n, cn, cr)
    g = np.take_along_axis(raw, idx[..., None].astype(np.int64), 1)
    scale = min(float(np.sqrt(C_EPS + float(np.float32(dec)) ** 2)), 0.3)
    kind = rng.randint(0, 4, (b, m))
    kind[:, :min(m, 2)] = np.arange(min(m, 2))  # every case has a copy (and a near pair where there are two points)
    if float(dec) == 0.0:
        kind[kind == 1] = 2  # dec = 0: every non-coincident pair is far beyond the pull's reach (s / c > 104)
    near = np.clip(g + scale * rng.randn(b, m, 3), -0.5, 0.49999).astype(np.float32)
    new = np.where((kind == 0)[..., None], g, np.where((kind == 1)[..., None], near, new)).astype(np.float32)
    return raw, new, idx, rng.randn(b, m, 3).astype(np.float32)
