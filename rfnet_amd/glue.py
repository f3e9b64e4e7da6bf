"""Loss / geometry glue: the direct callers of the operator hot path in the reference model
(layer L2 of SURVEY.md's map, the first "next" row, section 8(f1)), restated on torch tensors with the
reference's function names and semantics.  Everything heavy happens inside the HIP ops; the rest
are small elementwise / reduction tensor ops that autograd differentiates.

  sampling        vv_recon.py:67-83      merge_layer   vv_recon.py:132-139
  re_chamfer      vv_recon.py:171-193    chamfer_big   vv_recon.py:381-385
  fidelity_loss   vv_recon.py:386-390    earth_mover   vv_recon.py:392-399
  groupin_near    vv_recon.py:410-414    zero_groupnear vv_recon.py:415-419
"""
import torch
from torch.autograd.function import once_differentiable

from . import _raw
from .pc_distance.tf_approxmatch import earth_mover_cost
from .tf_ops.CD.tf_nndistance import nn_distance
from .tf_ops.grouping.tf_grouping import group_point
from .tf_ops.sampling.tf_sampling import farthest_point_sample, gather_point

SortedCloud = _raw.SortedCloud  # sort a cloud once, use it in several Chamfers of a step


def sort_if_large(xyz, min_points=1024):
    """A SortedCloud handle for clouds the culled sweep is used on (>= 1024 points), else None."""
    if isinstance(xyz, torch.Tensor) and xyz.is_cuda and 1024 <= xyz.shape[1] <= 65536 and xyz.shape[1] >= min_points:
        return SortedCloud(xyz.detach())
    return None


def sampling(npoint, xyz, use_type='f', generator=None, lengths=None):
    """Returns (idx, new_xyz).  'f': farthest point sampling + gather; 'r': one random subset of
    `npoint` indices shared by the whole batch (the reference shuffles arange(ptnum) once).
    `lengths` ('f' only): per-sample point counts of a ragged batch -- sample i is sampled from
    xyz[i, :lengths[i]] (rf_farthestpointsampling_lengths); one shared random subset has no ragged form."""
    if use_type == 'f':
        if lengths is not None:
            idx = _raw.farthest_point_sample(npoint, xyz.detach(), lengths=lengths)
            return idx, gather_point(xyz, idx)
        idx = farthest_point_sample(npoint, xyz)
        return idx, gather_point(xyz, idx)
    if use_type == 'r':
        if lengths is not None:
            raise ValueError("sampling: use_type 'r' draws one subset for the whole batch and takes no lengths")
        perm = torch.randperm(xyz.shape[1], device=xyz.device, generator=generator)[:npoint]
        idx = perm.to(torch.int32).unsqueeze(0).expand(xyz.shape[0], -1).contiguous()
        return idx, gather_point(xyz, idx)
    raise ValueError("use_type must be 'f' or 'r'")


class _MergeLayer(torch.autograd.Function):
    """rf_merge_layer / rf_merge_layer_grad: direction-2 Chamfer + gather + Gaussian pull as one op."""

    @staticmethod
    def forward(ctx, rawpts, newpts, decfactor, sorted_raw, lengths=None):
        refined, idx2 = _raw.merge_layer(rawpts, newpts, decfactor, sorted_raw, lengths=lengths)
        ctx.save_for_backward(rawpts, newpts, decfactor, idx2)
        ctx.lengths = lengths
        ctx.mark_non_differentiable(idx2)
        return refined, idx2

    @staticmethod
    def backward(ctx, grad_refined, _):
        rawpts, newpts, decfactor, idx2 = ctx.saved_tensors
        gn, gd, gr = _raw.merge_layer_grad(rawpts, newpts, decfactor, idx2, grad_refined.contiguous(),
                                           want_raw=ctx.needs_input_grad[0], lengths=ctx.lengths)
        return gr, gn, gd.sum().reshape(decfactor.shape).to(decfactor.dtype), None, None


def merge_layer(rawpts, newpts, decfactor, knum=16, sorted_raw=None, return_idx=False, lengths=None):
    """Pull every new point towards its nearest raw point with a Gaussian weight:
    refine = newpts + exp(-|g-newpts|^2 / (1e-8 + decfactor^2)) * (g - newpts), g = nn of newpts
    in rawpts (idx2 of nn_distance, grouped with nsample = 1).  `knum` is unused in the reference.
    One fused op (direction 2 of the Chamfer only, gather and pull in its epilogue); `sorted_raw`:
    optional SortedCloud of rawpts (the model merges into the same `pointcloud` three times).
    `lengths`: per-sample point counts of rawpts in a ragged batch (rf_merge_layer_lengths): the nearest raw
    point is looked for in rawpts[i, :lengths[i]] only and padded raw rows get a zero gradient; not combined
    with `sorted_raw`."""
    dec = torch.as_tensor(decfactor, dtype=newpts.dtype, device=newpts.device)
    refined, idx2 = _MergeLayer.apply(rawpts, newpts.contiguous(), dec, sorted_raw, lengths)
    return (refined, idx2) if return_idx else refined


def merge_layer_unfused(rawpts, newpts, decfactor, knum=16):
    """The same layer as the reference writes it (nn_distance -> group_point -> tensor ops); kept as
    the cross-check of the fused op."""
    _, _, _, idx2 = nn_distance(rawpts, newpts)
    grouped = group_point(rawpts, idx2.unsqueeze(-1))  # (b, npoint_new, 1, 3)
    diff = grouped - newpts.unsqueeze(2)
    dismat = (diff * diff).sum(-1, keepdim=True)
    dec = torch.as_tensor(decfactor, dtype=newpts.dtype, device=newpts.device)
    ratio = torch.exp(-dismat / (1e-8 + dec * dec))
    return newpts + (ratio * diff).sum(2)


class _NnDistanceLengths(torch.autograd.Function):
    """rf_nn_distance_lengths / rf_nn_distance_grad_lengths: the reference's 4-tuple over a ragged batch."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, lengths1, lengths2):
        d1, i1, d2, i2 = _raw.nn_distance(xyz1, xyz2, lengths1=lengths1, lengths2=lengths2)
        ctx.save_for_backward(xyz1, xyz2, i1, i2)
        ctx.lens = (lengths1, lengths2)
        ctx.mark_non_differentiable(i1, i2)
        return d1, i1, d2, i2

    @staticmethod
    def backward(ctx, gd1, _gi1, gd2, _gi2):
        xyz1, xyz2, i1, i2 = ctx.saved_tensors
        gd1 = torch.zeros_like(i1, dtype=xyz1.dtype) if gd1 is None else gd1.contiguous()
        gd2 = torch.zeros_like(i2, dtype=xyz2.dtype) if gd2 is None else gd2.contiguous()
        g1, g2 = _raw.nn_distance_grad(xyz1, xyz2, gd1, i1, gd2, i2, lengths1=ctx.lens[0], lengths2=ctx.lens[1])
        return g1, g2, None, None


def nn_distance_lengths(xyz1, xyz2, lengths1=None, lengths2=None):
    """nn_distance over a ragged batch: sample i uses xyz1[i, :lengths1[i]] and xyz2[i, :lengths2[i]]
    (None: all points).  Returns (dist1, idx1, dist2, idx2) with (0, -1) in the padded slots; the
    gradient of a padded point is 0.  Lengths: list, tuple, numpy array, CPU or CUDA tensor."""
    return _NnDistanceLengths.apply(xyz1.contiguous(), xyz2.contiguous(), lengths1, lengths2)


class _ChamferLoss(torch.autograd.Function):
    """rf_chamfer_loss / rf_chamfer_loss_grad: per-sample mean sqrt(dist) (b, 2) and idx1; the
    0.5/sqrt(d)/N factor of the backward is formed inside the scatter kernel.  With per-sample
    lengths: the _lengths entries (means and their backward over each sample's own count)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, sorted1, sorted2, want1, want2, lengths1=None, lengths2=None):
        loss, d1, i1, d2, i2 = _raw.chamfer_loss(xyz1, xyz2, sorted1, sorted2, want1, want2,
                                                 lengths1=lengths1, lengths2=lengths2)
        ctx.lens = (lengths1, lengths2)
        ctx.dirs = (want1, want2)
        ctx.save_for_backward(xyz1, xyz2, *[t for t in (d1, i1, d2, i2) if t is not None])
        idx1 = i1 if i1 is not None else torch.empty(0, dtype=torch.int32, device=loss.device)
        ctx.mark_non_differentiable(idx1)
        return loss, idx1

    @staticmethod
    def backward(ctx, grad_loss, _):
        saved = list(ctx.saved_tensors)
        xyz1, xyz2 = saved[0], saved[1]
        rest = saved[2:]
        d1 = i1 = d2 = i2 = None
        if ctx.dirs[0]:
            d1, i1, rest = rest[0], rest[1], rest[2:]
        if ctx.dirs[1]:
            d2, i2 = rest[0], rest[1]
        g1, g2 = _raw.chamfer_loss_grad(xyz1, xyz2, d1, i1, d2, i2, grad_loss.contiguous(),
                                        lengths1=ctx.lens[0], lengths2=ctx.lens[1])
        return g1, g2, None, None, None, None, None, None


def chamfer_per_sample(pcd1, pcd2, sorted1=None, sorted2=None, want1=True, want2=True, lengths1=None, lengths2=None):
    """(loss (b, 2), idx1): loss[:, 0] = mean_j sqrt(dist1), loss[:, 1] = mean_k sqrt(dist2) per sample.
    lengths1 / lengths2: per-sample point counts of a ragged batch (means over each sample's own points,
    idx1 = -1 in padded slots); not combined with sorted handles."""
    return _ChamferLoss.apply(pcd1.contiguous(), pcd2.contiguous(), sorted1, sorted2, want1, want2, lengths1, lengths2)


def chamfer_big(pcd1, pcd2, sorted1=None, sorted2=None, lengths1=None, lengths2=None):
    """(mean sqrt(dist1) + mean sqrt(dist2)) / 2 over the whole batch, and idx1 (vv_recon.py:381-385).
    One fused forward (sweep + sqrt-mean epilogue) and one fused backward.  With lengths: the batch mean
    of the per-sample means."""
    loss, idx1 = chamfer_per_sample(pcd1, pcd2, sorted1, sorted2, lengths1=lengths1, lengths2=lengths2)
    return (loss[:, 0].mean() + loss[:, 1].mean()) / 2, idx1


def fidelity_loss(pcd1, pcd2, sorted1=None, sorted2=None, lengths1=None, lengths2=None):
    """mean sqrt(dist1) (vv_recon.py:386-390): direction 1 only is computed."""
    loss, _ = chamfer_per_sample(pcd1, pcd2, sorted1, sorted2, True, False, lengths1, lengths2)
    return loss[:, 0].mean()


class _ChamferMetrics(torch.autograd.Function):
    """rf_chamfer_metrics / rf_chamfer_metrics_grad: the (b, 11) metrics tensor and idx1.  Columns 0-3, 9 and 10
    carry gradients; the maxima, the threshold fractions and the F-score (4-8) do not, and the counts inside DCD
    are constants."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, tau, alpha, lengths1, lengths2):
        met, d1, i1, d2, i2, c1, c2 = _raw.chamfer_metrics(xyz1, xyz2, tau, alpha, lengths1=lengths1, lengths2=lengths2)
        ctx.save_for_backward(xyz1, xyz2, d1, i1, d2, i2, c1, c2)
        ctx.alpha, ctx.lens = alpha, (lengths1, lengths2)
        ctx.mark_non_differentiable(i1)
        return met, i1

    @staticmethod
    def backward(ctx, grad_metrics, _):
        xyz1, xyz2, d1, i1, d2, i2, c1, c2 = ctx.saved_tensors
        g1, g2 = _raw.chamfer_metrics_grad(xyz1, xyz2, d1, i1, d2, i2, c1, c2, ctx.alpha, grad_metrics.contiguous(),
                                           lengths1=ctx.lens[0], lengths2=ctx.lens[1])
        return g1, g2, None, None, None, None


def chamfer_metrics(pcd1, pcd2, tau=0.01, alpha=1000.0, lengths1=None, lengths2=None):
    """What a completion is judged by, per sample, from one fused call (sweep + metrics epilogue).  `pcd1` plays the
    PREDICTION and `pcd2` the ground truth: precision is the fraction of pcd1's points within `tau` (a distance) of
    pcd2, recall the fraction of pcd2's points within `tau` of pcd1.  Returns a dict of (b,) tensors
      cd_l1      (mean sqrt(dist1) + mean sqrt(dist2)) / 2   (chamfer_big's number, per sample)
      cd_l2      mean dist1 + mean dist2
      hausdorff  sqrt(max(max dist1, max dist2))
      precision, recall, fscore   (fscore = their harmonic mean, 0 when both are 0)
      dcd        density-aware Chamfer distance: the mean over both directions of 1 - exp(-alpha dist) / count, count =
                 the number of queries that chose the point's neighbour (exponent 1, no set-size ratio factor)
    plus "raw", the (b, 11) tensor of include/rfops.h, and "idx1".  cd_l1, cd_l2 and dcd are differentiable (one
    fused backward); hausdorff, precision, recall and fscore carry no gradient.  lengths1 / lengths2: per-sample
    point counts of a ragged batch (every mean over a sample's own points)."""
    raw, idx1 = _ChamferMetrics.apply(pcd1.contiguous(), pcd2.contiguous(), float(tau), float(alpha), lengths1, lengths2)
    fixed = raw.detach()
    return {
        "cd_l1": (raw[:, 0] + raw[:, 1]) / 2,
        "cd_l2": raw[:, 2] + raw[:, 3],
        "hausdorff": torch.sqrt(torch.maximum(fixed[:, 4], fixed[:, 5])),
        "precision": fixed[:, 6],
        "recall": fixed[:, 7],
        "fscore": fixed[:, 8],
        "dcd": (raw[:, 9] + raw[:, 10]) / 2,
        "raw": raw,
        "idx1": idx1,
    }


def dcd_loss(pcd1, pcd2, alpha=1000.0, lengths1=None, lengths2=None):
    """The batch mean of chamfer_metrics(...)["dcd"]: the density-aware Chamfer distance as a training loss."""
    return chamfer_metrics(pcd1, pcd2, alpha=alpha, lengths1=lengths1, lengths2=lengths2)["dcd"].mean()


def _matrix_keys(raw):
    return {
        "cd_l1": (raw[..., 0] + raw[..., 1]) / 2,
        "cd_l2": raw[..., 2] + raw[..., 3],
        "hausdorff": torch.sqrt(torch.maximum(raw[..., 4], raw[..., 5])),
        "raw": raw,
    }


def chamfer_matrix(set1, set2=None, lengths1=None, lengths2=None):
    """The Chamfer matrix of two collections of clouds, set1 (s, n, 3) against set2 (r, m, 3), from one call
    (rf_chamfer_cross: each collection sorted once, nothing stored per point).  set2=None: set1 against itself.
    Returns a dict of (s, r) tensors with chamfer_metrics' conventions -- cd_l1, cd_l2, hausdorff -- plus "raw", the
    (s, r, 6) tensor of include/rfops.h.  An entry depends on its two clouds alone, not on the collections around
    them.  No gradient.  lengths1 (s,) / lengths2 (r,): per-cloud point counts."""
    return _matrix_keys(_raw.chamfer_cross(set1, set2, lengths1=lengths1, lengths2=lengths2))


def _argmin_low(d, dim):
    """(min, argmin) along `dim` with the LOWEST index on ties (torch.min leaves the choice open)."""
    v = d.min(dim=dim, keepdim=True).values
    pos = torch.arange(d.shape[dim], device=d.device).view([-1 if k == dim % d.dim() else 1 for k in range(d.dim())])
    idx = torch.where(d == v, pos, d.shape[dim]).min(dim=dim).values
    return v.squeeze(dim), idx.clamp_(max=max(d.shape[dim] - 1, 0))  # (a row of NaN matches nothing)


def minimal_matching(pred, refs, metric="cd_l2", lengths1=None, lengths2=None, chunk=None):
    """Minimal matching distance: for every cloud of pred (s, n, 3) the smallest chamfer_matrix entry `metric`
    ("cd_l1", "cd_l2" or "hausdorff") over the reference clouds refs (r, m, 3), and where it is -> (value (s,),
    index (s,) int64), ties to the lowest index.  `chunk`: references per rf_chamfer_cross call, which bounds the
    matrix and the workspace; the results are the same bits for every chunk (an entry depends on its pair alone)."""
    if metric not in ("cd_l1", "cd_l2", "hausdorff"):
        raise ValueError(f"minimal_matching: unknown metric {metric!r}")
    r = refs.shape[0]
    if r < 1:
        raise ValueError("minimal_matching needs at least one reference cloud")
    step = r if chunk is None else int(chunk)
    if step < 1:
        raise ValueError("minimal_matching: chunk must be positive")
    l2 = None if lengths2 is None else _raw._check_lengths(lengths2, r, refs.shape[1], "lengths2")
    best = best_at = None
    for j0 in range(0, r, step):
        d = chamfer_matrix(pred, refs[j0:j0 + step], lengths1=lengths1,
                           lengths2=None if l2 is None else l2[j0:j0 + step])[metric]
        v, at = _argmin_low(d, 1)
        at = at + j0
        if best is None:
            best, best_at = v, at
        else:
            take = v < best  # strict: a tie stays with the earlier chunk
            best, best_at = torch.where(take, v, best), torch.where(take, at, best_at)
    return best, best_at


def set_metrics(d_gr, d_gg=None, d_rr=None):
    """Set-level scores from distance matrices (any entry of chamfer_matrix): d_gr (g, r) generated against
    reference clouds, and optionally d_gg (g, g) and d_rr (r, r).  Plain tensor ops (CPU tensors allowed), 0-d
    results, no host synchronisation.
      mmd      mean over references j of min_i d_gr[i, j]
      cov      #{distinct argmin_j d_gr[i, :] over i} / r
      one_nna  (with d_gg and d_rr) the leave-one-out 1-NN accuracy over the g + r clouds: the fraction whose nearest
               other cloud, in [[d_gg, d_gr], [d_gr^T, d_rr]] with an infinite diagonal, carries their own label
    Every argmin is the lowest index on ties."""
    if d_gr.dim() != 2 or d_gr.shape[0] < 1 or d_gr.shape[1] < 1:
        raise ValueError("set_metrics requires a non-empty (generated, references) matrix")
    g, r = d_gr.shape
    out = {"mmd": d_gr.min(dim=0).values.mean()}
    hit = torch.zeros(r, dtype=d_gr.dtype, device=d_gr.device)
    hit[_argmin_low(d_gr, 1)[1]] = 1
    out["cov"] = hit.sum() / r
    if d_gg is not None and d_rr is not None:
        if d_gg.shape != (g, g) or d_rr.shape != (r, r):
            raise ValueError("set_metrics requires d_gg (g, g) and d_rr (r, r)")
        full = torch.cat([torch.cat([d_gg, d_gr], 1), torch.cat([d_gr.t(), d_rr], 1)], 0).clone()
        full.fill_diagonal_(float("inf"))
        own = torch.arange(g + r, device=full.device) < g
        out["one_nna"] = ((_argmin_low(full, 1)[1] < g) == own).to(d_gr.dtype).mean()
    elif d_gg is not None or d_rr is not None:
        raise ValueError("set_metrics: one_nna needs both d_gg and d_rr")
    return out


class _SlicedWasserstein(torch.autograd.Function):
    """rf_sliced_wasserstein: the loss (b,) and, when an input needs it, both gradients from the same call."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, directions, lengths1, lengths2):
        if xyz1.requires_grad or xyz2.requires_grad:
            loss, g1, g2 = _raw.sliced_wasserstein(xyz1, xyz2, directions, lengths1, lengths2, want_grad=True)
            ctx.save_for_backward(g1, g2)
            return loss
        return _raw.sliced_wasserstein(xyz1, xyz2, directions, lengths1, lengths2)

    @staticmethod
    def backward(ctx, grad_loss):
        g1, g2 = ctx.saved_tensors
        w = grad_loss[:, None, None]
        return (w * g1 if ctx.needs_input_grad[0] else None, w * g2 if ctx.needs_input_grad[1] else None, None, None,
                None)


def sliced_wasserstein(pcd1, pcd2, nproj=128, directions=None, generator=None, lengths1=None, lengths2=None):
    """The sliced Wasserstein distance SW_2^2 per sample, (b,): the mean over the directions of the 1-D optimal
    transport cost between the projections of pcd1 (b, n, 3) and pcd2 (b, m, 3) -- a transport-type loss at
    O(nproj n log n) that takes n != m and ragged batches exactly (lengths1 / lengths2: per-sample point counts; padded
    rows get a zero gradient).  `directions` (nproj, 3) are used as given; None draws `nproj` unit vectors on the
    inputs' device from `generator` (no host round trip).  Differentiable in pcd1 and pcd2: one fused call returns the
    loss and both gradients, with ties in a projection going to the lower index (rf_sliced_wasserstein)."""
    if directions is None:
        if int(nproj) < 1:
            raise ValueError("sliced_wasserstein: nproj must be positive")
        directions = torch.randn(int(nproj), 3, device=pcd1.device, dtype=torch.float32, generator=generator)
        directions = directions / directions.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return _SlicedWasserstein.apply(pcd1.contiguous(), pcd2.contiguous(), directions.detach(), lengths1, lengths2)


def sinkhorn_schedule(p=1, blur=0.05, scaling=0.5, diameter=2.0, extra=0):
    """The annealed eps schedule of sinkhorn_divergence, on the host: diameter^p, then down by factors scaling^p while
    above blur^p, then 1 + extra steps at blur^p.  The default diameter covers clouds in the unit ball; it is a number the
    caller states, never read from the device.  (rf_sinkhorn takes up to 256 steps; the helper itself has no cap.)"""
    p, blur, scaling, diameter, extra = int(p), float(blur), float(scaling), float(diameter), int(extra)
    if p not in (1, 2):
        raise ValueError("sinkhorn_schedule: p must be 1 or 2")
    if not (blur > 0.0 and diameter > 0.0 and 0.0 < scaling < 1.0 and extra >= 0):
        raise ValueError("sinkhorn_schedule: expects blur > 0, diameter > 0, 0 < scaling < 1, extra >= 0")
    eps, s = [], diameter
    while s > blur:
        eps.append(s ** p)
        s *= scaling
    return eps + [blur ** p] * (1 + extra)


class _Sinkhorn(torch.autograd.Function):
    """rf_sinkhorn: the loss (b,) with pot and delta and, when an input needs it, both gradients from the same call."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, p, lengths1, lengths2):
        if xyz1.requires_grad or xyz2.requires_grad:
            loss, pot, delta, g1, g2 = _raw.sinkhorn(xyz1, xyz2, eps, p, lengths1, lengths2, want_grad=True)
            ctx.save_for_backward(g1, g2)
        else:
            loss, pot, delta = _raw.sinkhorn(xyz1, xyz2, eps, p, lengths1, lengths2)
        ctx.mark_non_differentiable(pot, delta)
        return loss, pot, delta

    @staticmethod
    def backward(ctx, grad_loss, *_):
        g1, g2 = ctx.saved_tensors
        w = grad_loss[:, None, None]
        return (w * g1 if ctx.needs_input_grad[0] else None, w * g2 if ctx.needs_input_grad[1] else None, None, None,
                None, None)


def sinkhorn_divergence(pcd1, pcd2, p=1, blur=0.05, scaling=0.5, diameter=2.0, extra=0, eps=None, lengths1=None,
                        lengths2=None, return_info=False):
    """The Sinkhorn divergence S_eps per sample, (b,): debiased entropy-regularised optimal transport between pcd1
    (b, n, 3) and pcd2 (b, m, 3) with uniform weights, for the cost |x - y| (p = 1) or |x - y|^2 / 2 (p = 2).  S(a, a) = 0,
    S >= 0; it approaches the transport cost as blur -> 0.  The regularisation is annealed along
    sinkhorn_schedule(p, blur, scaling, diameter, extra), or along `eps` (a host sequence) when given.  n != m and ragged
    batches (lengths1 / lengths2: per-sample point counts) are exact; padded rows get a zero gradient.  Differentiable in
    pcd1 and pcd2 through the last step, the potentials before it held fixed: one fused call returns the loss and both
    gradients (rf_sinkhorn).  return_info: also {"pot": (b, n + m) the final potentials f | g, "delta": (b,) how far they
    moved in the last step, in units of cost}."""
    if eps is None:
        eps = sinkhorn_schedule(p, blur, scaling, diameter, extra)
    loss, pot, delta = _Sinkhorn.apply(pcd1.contiguous(), pcd2.contiguous(), eps, p, lengths1, lengths2)
    if return_info:
        return loss, {"pot": pot, "delta": delta}
    return loss


def _cloud_tensor(x):
    """A cloud given as a torch tensor or a numpy array -> a contiguous fp32 tensor (a tensor keeps its graph and device)."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    return t.to(torch.float32).contiguous()


def _grid_bounds(bounds):
    lo, hi = bounds
    return float(lo), float(hi)


class _GriddingLoss(torch.autograd.Function):
    """rf_gridding_loss: the loss (b,) with the inside counts and, when an input needs it, both gradients from the same call."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, res, lo, hi, mode, lengths1, lengths2):
        if xyz1.requires_grad or xyz2.requires_grad:
            loss, inside, g1, g2 = _raw.gridding_loss(xyz1, xyz2, res, lo, hi, mode, lengths1, lengths2, want_grad=True)
            ctx.save_for_backward(g1, g2)
        else:
            loss, inside = _raw.gridding_loss(xyz1, xyz2, res, lo, hi, mode, lengths1, lengths2)
        ctx.mark_non_differentiable(inside)
        return loss, inside

    @staticmethod
    def backward(ctx, grad_loss, *_):
        g1, g2 = ctx.saved_tensors
        w = grad_loss[:, None, None]
        return (w * g1 if ctx.needs_input_grad[0] else None, w * g2 if ctx.needs_input_grad[1] else None, None, None,
                None, None, None, None)


def gridding_loss(pcd1, pcd2, resolution=64, bounds=(-0.5, 0.5), density=False, lengths1=None, lengths2=None,
                  return_info=False):
    """GRNet's Gridding loss per sample, (b,): every point of pcd1 (b, n, 3) and pcd2 (b, m, 3) inside the cube
    [bounds[0], bounds[1]]^3 spreads its mass trilinearly over the eight vertices of its cell of a grid of `resolution`
    vertices per axis, and the loss is the L1 difference of the two grids -- the mean over the vertices of |G1 - G2|, or with
    `density` sum |G1 / L1 - G2 / L2| (in [0, 2]; clouds of different sizes compare as distributions).  No correspondence,
    linear in the point counts.  The sums are exact integers on a fixed-point weight grid, so the value is the same bits for
    every order of the points and every batch.  n != m and ragged batches (lengths1 / lengths2: per-sample point counts) are
    exact; points outside the box and padded rows contribute nothing and get a zero gradient.  Differentiable in pcd1 and pcd2:
    one fused call returns the loss and both gradients (rf_gridding_loss).  return_info: also {"inside": (b, 2) how many points
    of each cloud fell inside the box}."""
    lo, hi = _grid_bounds(bounds)
    loss, inside = _GriddingLoss.apply(_cloud_tensor(pcd1), _cloud_tensor(pcd2), int(resolution), lo, hi,
                                       "density" if density else "counts", lengths1, lengths2)
    if return_info:
        return loss, {"inside": inside}
    return loss


class _Gridding(torch.autograd.Function):
    """rf_gridding / rf_gridding_grad: the trilinear grid of a cloud."""

    @staticmethod
    def forward(ctx, xyz, res, lo, hi, lengths):
        grid, _ = _raw.gridding(xyz, res, lo, hi, lengths)
        ctx.save_for_backward(xyz)
        ctx.box, ctx.lengths = (res, lo, hi), lengths
        return grid

    @staticmethod
    def backward(ctx, grad_grid):
        (xyz,) = ctx.saved_tensors
        return _raw.gridding_grad(xyz, grad_grid.contiguous(), *ctx.box, lengths=ctx.lengths), None, None, None, None


def gridding(pcd, resolution=64, bounds=(-0.5, 0.5), lengths=None):
    """GRNet's Gridding layer: the cloud pcd (b, n, 3) as a grid (b, R, R, R) of R = `resolution` vertices per axis over the
    cube [bounds[0], bounds[1]]^3, x slowest -- every point inside spreads a mass of 1 trilinearly over the eight vertices of
    its cell (exact integer sums, rf_gridding).  Differentiable in pcd (rf_gridding_grad); `lengths`: per-sample point counts."""
    lo, hi = _grid_bounds(bounds)
    return _Gridding.apply(_cloud_tensor(pcd), int(resolution), lo, hi, lengths)


class _CubicFeatureSampling(torch.autograd.Function):
    """rf_cubic_feature_sampling / rf_cubic_feature_sampling_grad: only the volume carries a gradient."""

    @staticmethod
    def forward(ctx, xyz, vol, lo, hi, lengths):
        feat, _ = _raw.cubic_feature_sampling(xyz, vol, lo, hi, lengths)
        ctx.save_for_backward(xyz)
        ctx.box, ctx.lengths = (vol.shape[2], lo, hi), lengths
        return feat

    @staticmethod
    def backward(ctx, grad_feat):
        (xyz,) = ctx.saved_tensors
        gv = _raw.cubic_feature_sampling_grad(xyz, grad_feat.contiguous(), *ctx.box, lengths=ctx.lengths)
        return None, gv, None, None, None


def cubic_feature_sampling(pcd, volume, bounds=(-0.5, 0.5), lengths=None):
    """GRNet's Cubic Feature Sampling: for every point of pcd (b, n, 3) the feature vectors of volume (b, c, R, R, R) at the
    eight vertices of its cell of the grid over [bounds[0], bounds[1]]^3 (the geometry of `gridding`) -> (b, n, 8, c), the
    corners with z fastest; zeros for points outside the cube and padded rows (`lengths`: per-sample point counts).  Autograd
    goes to `volume` only (rf_cubic_feature_sampling_grad: double sums in LDS, no float atomics in memory); the op is piecewise
    constant in the points."""
    lo, hi = _grid_bounds(bounds)
    vol = volume if isinstance(volume, torch.Tensor) else torch.as_tensor(volume)
    return _CubicFeatureSampling.apply(_cloud_tensor(pcd).detach(), vol.to(torch.float32).contiguous(), lo, hi, lengths)


class _GriddingReverse(torch.autograd.Function):
    """rf_gridding_reverse / rf_gridding_reverse_grad: the points carry a gradient to the grid; the counts do not."""

    @staticmethod
    def forward(ctx, grid, lo, hi, eps, compact):
        points, row, count = _raw.gridding_reverse(grid, lo, hi, eps, compact)
        ctx.save_for_backward(grid, row)
        ctx.box = (lo, hi)
        ctx.mark_non_differentiable(count)
        return points, count

    @staticmethod
    def backward(ctx, grad_points, _):
        grid, row = ctx.saved_tensors
        return _raw.gridding_reverse_grad(grid, row, grad_points.contiguous(), *ctx.box), None, None, None, None


def gridding_reverse(grid, bounds=(-0.5, 0.5), eps=1e-6, compact=True):
    """GRNet's Gridding Reverse: the grid (b, R, R, R) back to a cloud -> (points (b, (R - 1)^3, 3), lengths (b,) int32 on the
    device).  Every cell whose eight corner weights sum to at least `eps` gives one point, the weighted mean of its corners.
    `compact`: the valid cells fill the first lengths[i] rows in cell order and the rest is zeros, so the pair is a padded batch
    for every `lengths=` argument of this library -- no boolean mask, no host sync, capturable in a graph; otherwise cell c stays
    in row c and invalid rows are zeros.  Differentiable in grid (rf_gridding_reverse_grad)."""
    lo, hi = _grid_bounds(bounds)
    g = grid if isinstance(grid, torch.Tensor) else torch.as_tensor(grid)
    return _GriddingReverse.apply(g.to(torch.float32).contiguous(), lo, hi, float(eps), bool(compact))


class _AvgVoxelize(torch.autograd.Function):
    """rf_voxelize_mean / rf_voxelize_mean_grad: only the features carry a gradient."""

    @staticmethod
    def forward(ctx, xyz, feat, res, lo, hi, lengths):
        vol, cnt, inside = _raw.avg_voxelize(xyz, feat, res, lo, hi, lengths)
        ctx.save_for_backward(xyz, cnt)
        ctx.box, ctx.lengths = (lo, hi), lengths
        ctx.mark_non_differentiable(cnt, inside)
        return vol, cnt, inside

    @staticmethod
    def backward(ctx, grad_vol, *_):
        xyz, cnt = ctx.saved_tensors
        gf = _raw.avg_voxelize_grad(xyz, cnt, grad_vol.contiguous(), *ctx.box, lengths=ctx.lengths)
        return None, gf, None, None, None, None


def avg_voxelize(pcd, feat, resolution=32, bounds=(-0.5, 0.5), lengths=None, return_counts=False):
    """PVCNN's average voxelization: the feature vectors feat (b, n, c) of the points pcd (b, n, 3), averaged per nearest
    vertex of the grid of `resolution` vertices per axis over the cube [bounds[0], bounds[1]]^3 (the geometry of `gridding`;
    the vertices are PVCNN's voxel lattice) -> a volume (b, c, R, R, R), zeros where no point fell.  Points outside the cube and
    padded rows (`lengths`: per-sample point counts) contribute nothing.  Double sums in LDS, no float atomics in memory
    (rf_voxelize_mean).  Differentiable in feat (rf_voxelize_mean_grad); the op is piecewise constant in the points.
    PVCNN's coordinate normalisation (mean-centre, scale by the largest norm) is torch code in front of this call.
    return_counts: also (cnt (b, R, R, R) int32, inside (b,) int32)."""
    lo, hi = _grid_bounds(bounds)
    f = feat if isinstance(feat, torch.Tensor) else torch.as_tensor(feat)
    vol, cnt, inside = _AvgVoxelize.apply(_cloud_tensor(pcd).detach(), f.to(torch.float32).contiguous(), int(resolution), lo, hi,
                                          lengths)
    if return_counts:
        return vol, cnt, inside
    return vol


class _TrilinearDevoxelize(torch.autograd.Function):
    """rf_trilinear_devoxelize / rf_trilinear_devoxelize_grad: the volume and the points carry gradients."""

    @staticmethod
    def forward(ctx, xyz, vol, lo, hi, lengths):
        feat, _ = _raw.trilinear_devoxelize(xyz, vol, lo, hi, lengths)
        ctx.save_for_backward(xyz, vol)
        ctx.box, ctx.lengths = (lo, hi), lengths
        return feat

    @staticmethod
    def backward(ctx, grad_feat):
        xyz, vol = ctx.saved_tensors
        gv, gx = _raw.trilinear_devoxelize_grad(xyz, vol, grad_feat.contiguous(), *ctx.box, lengths=ctx.lengths,
                                                want_xyz=ctx.needs_input_grad[0])
        return gx, (gv if ctx.needs_input_grad[1] else None), None, None, None


def trilinear_devoxelize(pcd, volume, bounds=(-0.5, 0.5), lengths=None):
    """PVCNN's trilinear devoxelization: volume (b, c, R, R, R) interpolated at every point of pcd (b, n, 3) from the eight
    vertices of its cell of the grid over [bounds[0], bounds[1]]^3 (the geometry of `gridding`) -> (b, n, c); zeros for points
    outside the cube and padded rows (`lengths`: per-sample point counts).  Every rounding is prescribed
    (rf_trilinear_devoxelize).  Differentiable in volume (double sums in LDS, no float atomics in memory) and in pcd; the
    gradient to the points is computed only when pcd requires it (rf_trilinear_devoxelize_grad)."""
    lo, hi = _grid_bounds(bounds)
    vol = volume if isinstance(volume, torch.Tensor) else torch.as_tensor(volume)
    return _TrilinearDevoxelize.apply(_cloud_tensor(pcd), vol.to(torch.float32).contiguous(), lo, hi, lengths)


class _NeighborSubtraction(torch.autograd.Function):
    """rf_neighbor_sub / rf_neighbor_sub_grad: both feature tensors carry gradients, idx does not."""

    @staticmethod
    def forward(ctx, feat_q, feat_src, idx, lengths1, lengths2):
        ctx.save_for_backward(idx)
        ctx.n, ctx.lengths = feat_src.shape[1], (lengths1, lengths2)
        return _raw.neighbor_subtraction(feat_q, feat_src, idx, lengths1, lengths2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        gq, gs = _raw.neighbor_subtraction_grad(idx, grad_out.contiguous(), ctx.n, *ctx.lengths, want_q=ctx.needs_input_grad[0],
                                                want_src=ctx.needs_input_grad[1])
        return gq, gs, None, None, None


def _feature_tensor(x):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    return t.to(torch.float32).contiguous()


def _index_tensor(idx):
    t = idx if isinstance(idx, torch.Tensor) else torch.as_tensor(idx)
    return t.detach().to(torch.int32).contiguous()


def neighbor_subtraction(feat_q, feat_src, idx, lengths1=None, lengths2=None):
    """The relative features in front of a vector attention's MLP (pointops' `subtraction`, on padded batches):
    feat_q (b, m, c) less the rows of feat_src (b, n, c) that idx (b, m, k) names -> (b, m, k, c).  idx is what `knn_point`
    returns, and a ragged batch passes knn_point's own lengths1 / lengths2 (source rows / queries per sample): its padded slots
    and rows are zeros here and receive no gradient (rf_neighbor_sub).  Differentiable in both feature tensors: the gradient
    to feat_src is a sort of the slots by row and a gather in double, no float atomics (rf_neighbor_sub_grad); only the
    gradients that are needed are computed."""
    return _NeighborSubtraction.apply(_feature_tensor(feat_q), _feature_tensor(feat_src), _index_tensor(idx), lengths1, lengths2)


class _KnnFeature(torch.autograd.Function):
    """rf_knn_feature; the backward has no kernel of its own: it recomputes the relative features and goes through
    rf_neighbor_sub_grad."""

    @staticmethod
    def forward(ctx, feat1, feat2, k, lengths1, lengths2):
        val, idx = _raw.knn_feature(k, feat1, feat2, lengths1, lengths2)
        ctx.save_for_backward(feat1, feat2, idx)
        ctx.lengths = (lengths1, lengths2)
        ctx.mark_non_differentiable(idx)
        return val, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_val, _):
        feat1, feat2, idx = ctx.saved_tensors
        diff = _raw.neighbor_subtraction(feat2, feat1, idx, *ctx.lengths)  # f2[j] - f1[idx[j, t]], +0 in dead slots
        grad_diff = (-2.0 * grad_val.unsqueeze(-1) * diff).contiguous()
        g2, g1 = _raw.neighbor_subtraction_grad(idx, grad_diff, feat1.shape[1], *ctx.lengths, want_q=ctx.needs_input_grad[1],
                                                want_src=ctx.needs_input_grad[0])
        return g1, g2, None, None, None


def knn_feature(k, feat1, feat2, lengths1=None, lengths2=None):
    """k-nearest neighbours in feature space, the graph DGCNN's EdgeConv rebuilds at every layer: per row of feat2 (b, m, c)
    the k rows of feat1 (b, n, c) of smallest d = |q|^2 + |x|^2 - 2 q.x -> (val (b, m, k) = -d, idx (b, m, k) int32), ascending
    by (d, index); `knn_point`'s argument order, tie rule and ragged rule (lengths1 / lengths2: candidate / query rows per
    sample; padded rows and slots are zeros).  No (b, m, n) matrix is formed (rf_knn_feature).  d is the formula's fp32 value and
    can be slightly negative under cancellation, so a row that queries itself is not guaranteed slot 0 among near-duplicates.
    idx is non-differentiable.  val is differentiable in both inputs, as -|feat2[j] - feat1[idx[j, t]]|^2 at fixed idx: the
    backward recomputes the differences (rf_neighbor_sub) and scatters -2 g diff through rf_neighbor_sub_grad -- the derivative
    of the squared distance itself, not of the rounded three-term formula."""
    return _KnnFeature.apply(_feature_tensor(feat1), _feature_tensor(feat2), int(k), lengths1, lengths2)


def edge_feature(feat_q, feat_src, idx, lengths1=None, lengths2=None):
    """DGCNN's get_graph_feature: cat(f_j - f_i, f_i) -> (b, m, k, 2c), f_i = feat_q (b, m, c) the centre rows and f_j the rows
    of feat_src (b, n, c) that idx (b, m, k) names -- what `knn_feature(k, feat_src, feat_q)` returns.  Torch glue over
    `neighbor_subtraction`, whose gradients it inherits; with lengths1 / lengths2 (source rows / queries per sample) padded rows
    and slots are zeros in both halves."""
    fq = _feature_tensor(feat_q)
    ix = _index_tensor(idx)
    fs = _feature_tensor(feat_src)
    rel = 0.0 - neighbor_subtraction(fq, fs, ix, lengths1, lengths2)  # f_j - f_i exactly; dead slots stay +0
    b, m, k = ix.shape
    n, dev = int(fs.shape[1]), rel.device
    centre = fq.to(dev).unsqueeze(2).expand(b, m, k, fq.shape[2])
    if lengths1 is not None or lengths2 is not None:  # the dead slots of rf_neighbor_sub, from the counts on the device
        live = torch.ones((b, m, k), dtype=torch.bool, device=dev)
        if lengths1 is not None:
            l1 = _raw._lengths_up(_raw._check_lengths(lengths1, b, n, "lengths1"), dev, n).clamp(1, n)[:, None, None]
            jx = ix.to(dev)
            live = live & (torch.arange(k, device=dev)[None, None, :] < l1) & (jx >= 0) & (jx < l1)
        if lengths2 is not None:
            l2 = _raw._lengths_up(_raw._check_lengths(lengths2, b, m, "lengths2"), dev, m).clamp(1, m)[:, None, None]
            live = live & (torch.arange(m, device=dev)[None, :, None] < l2)
        centre = torch.where(live.unsqueeze(-1), centre, torch.zeros((), dtype=centre.dtype, device=dev))
    return torch.cat((rel, centre), dim=-1)


def _viewpoint_tensor(viewpoint, b, dev):
    """A (3,) or (b, 3) viewpoint, tensor or sequence -> a contiguous (b, 3) fp32 tensor on `dev` (a tensor that is there stays)."""
    if viewpoint is None:
        return None
    v = viewpoint if isinstance(viewpoint, torch.Tensor) else torch.as_tensor(viewpoint, dtype=torch.float32)
    v = v.detach().to(device=dev, dtype=torch.float32)
    if v.dim() == 1 and v.shape[0] == 3:
        v = v.unsqueeze(0).expand(b, 3)
    if tuple(v.shape) != (b, 3):
        raise ValueError("viewpoint must be of shape (3,) or (batch, 3)")
    return v.contiguous()


def local_pca(pcd, idx, lengths1=None, lengths2=None, viewpoint=None, return_axes=False):
    """The PCA of every neighbourhood that idx (b, m, k) names among the points of pcd (b, n, 3) -- idx is what
    `knn_point(k, pcd, queries)` returned, and a ragged batch passes knn_point's own lengths1 / lengths2 (points / queries per
    sample; padded rows are zeros).  Returns a dict: "normals" (b, m, 3), the unit eigenvector of the smallest eigenvalue;
    "eigenvalues" (b, m, 3) of the neighbourhood's covariance, ascending (l0, l1, l2); with return_axes "axes" (b, m, 3, 3),
    the three eigenvectors as rows in that order.  The surface variation of a point is l0 / (l0 + l1 + l2).
    Every vector has a canonical sign (its largest component positive); with `viewpoint` ((3,) or (b, 3)) the normal is turned
    towards the viewer.  A neighbourhood with a non-finite covariance gets NaN eigenvalues and a zero normal.  Cyclic Jacobi in
    double with every operation prescribed (rf_local_pca): the same bits in every run, batch and shard.  Non-differentiable:
    the inputs are detached."""
    x = _cloud_tensor(pcd).detach()
    vp = _viewpoint_tensor(viewpoint, x.shape[0], x.device)
    nrm, eig, axes = _raw.local_pca(x, _index_tensor(idx), lengths1, lengths2, vp, want_axes=return_axes)
    out = {"normals": nrm, "eigenvalues": eig}
    if return_axes:
        out["axes"] = axes
    return out


def estimate_normals(pcd, k=16, lengths=None, viewpoint=None):
    """Surface normals of a cloud (b, n, 3) by PCA of every point's k nearest neighbours, the point itself included:
    `knn_point` of the cloud against itself with its usual routing, then `local_pca` -> (normals (b, n, 3), eigenvalues
    (b, n, 3) ascending).  k is capped at n.  lengths: points per sample of a ragged batch (rows behind a count are zeros);
    viewpoint: (3,) or (b, 3), tensor or sequence -- normals are turned towards it, without one their largest component is
    positive.  Non-differentiable: the cloud is detached."""
    x = _cloud_tensor(pcd).detach()
    _, idx = _raw.knn_point(min(int(k), int(x.shape[1])), x, x, lengths1=lengths, lengths2=lengths)
    r = local_pca(x, idx, lengths, lengths, viewpoint)
    return r["normals"], r["eigenvalues"]


def normal_consistency(pcd1, pcd2, normals1=None, normals2=None, k=16, lengths1=None, lengths2=None):
    """Normal consistency of two clouds, the third column of the reconstruction benchmarks next to Chamfer and F-score: every
    point's normal against the normal of its nearest neighbour in the other cloud (`nn_distance_lengths`' indices).  normals1 /
    normals2 (b, n, 3) / (b, m, 3): whichever is None is estimated with `estimate_normals(., k)`.  Returns a dict of (b,)
    tensors: "nc12" = mean_j |n1[j] . n2[idx1[j]]|, "nc21" the other direction, "nc" = (nc12 + nc21) / 2 -- the unsigned
    figures, for estimated normals whose sign means nothing -- and "signed12", "signed21", the means without the absolute
    value, for clouds that carry oriented normals.  A zero normal contributes 0.  lengths1 / lengths2: points per sample of a
    ragged batch.  Non-differentiable: the inputs are detached (rf_nn_normal_consistency)."""
    x1, x2 = _cloud_tensor(pcd1).detach(), _cloud_tensor(pcd2).detach()
    n1 = estimate_normals(x1, k, lengths1)[0] if normals1 is None else _cloud_tensor(normals1).detach()
    n2 = estimate_normals(x2, k, lengths2)[0] if normals2 is None else _cloud_tensor(normals2).detach()
    _, idx1, _, idx2 = _raw.nn_distance(x1, x2, lengths1=lengths1, lengths2=lengths2)
    raw = _raw.nn_normal_consistency(n1, n2, idx1, idx2, lengths1, lengths2)
    return {"nc12": raw[:, 0], "nc21": raw[:, 1], "nc": (raw[:, 0] + raw[:, 1]) / 2, "signed12": raw[:, 2],
            "signed21": raw[:, 3]}


def _origin_tensor(origin, b, dev):
    """A (3,) or (b, 3) grid origin, tensor or sequence -> a contiguous (b, 3) fp32 tensor on `dev`, or None."""
    if origin is None:
        return None
    o = origin if isinstance(origin, torch.Tensor) else torch.as_tensor(origin, dtype=torch.float32)
    o = o.detach().to(device=dev, dtype=torch.float32)
    if o.dim() == 1 and o.shape[0] == 3:
        o = o.unsqueeze(0).expand(b, 3)
    if tuple(o.shape) != (b, 3):
        raise ValueError("origin must be of shape (3,) or (batch, 3)")
    return o.contiguous()


def grid_cluster(pcd, cell, origin=None, order="xyz", lengths=None, return_code=False):
    """The occupied cells of a sparse, unbounded voxel grid of edge `cell` over every cloud of pcd (b, n, 3), n <= 16384: a
    point with finite coordinates falls in cell floor((x - origin) / cell) per axis (in double), and is `inside` when every
    cell index fits 16 bits (+-32768 cells round the origin).  origin: (3,) or (b, 3), default the per-axis minimum of each
    sample's points.  Returns a dict of device tensors: "cluster" (b, n) int32, the rank of each point's cell among the
    sample's occupied cells in the order of `order` ("xyz" row-major, "z" Morton, "hilbert"), -1 for rows that are not inside;
    "order" (b, n) the inside points sorted by (cell, index); "starts" (b, n + 1) where each cell's points begin in "order"
    (entries behind the cell count hold the inside count); "coords" (b, n, 3) int32 each cell's indices; "nclusters" and
    "inside" (b,) int32; "origin" (b, 3); with return_code "code" (b, n) int64, each point's 48-bit key.  Other axis
    conventions ("trans" orders, a z-major Morton) are a column permutation of pcd in front of the call.  lengths: points
    per sample of a ragged batch.  One launch per call, no host synchronisation (capturable), the same bits on every call
    and for every batch (rf_grid_cluster).  Non-differentiable."""
    x = _cloud_tensor(pcd).detach()
    return _raw.grid_cluster(x, cell, order, lengths, _origin_tensor(origin, x.shape[0], x.device), want_code=return_code)


_GP_BACKWARD = {"sum": "copy", "mean": "mean", "max": "max"}


class _GridPoolRows(torch.autograd.Function):
    """rf_grid_pool at a fixed clustering; its backward is rf_grid_unpool in the mode that belongs to the reduction."""

    @staticmethod
    def forward(ctx, rows, order, starts, nclusters, cluster, reduce):
        if reduce == "max":
            out, arg = _raw.grid_pool(rows, order, starts, nclusters, "max")
            ctx.save_for_backward(cluster, starts, arg)
            ctx.mark_non_differentiable(arg)
        else:
            out, arg = _raw.grid_pool(rows, order, starts, nclusters, reduce), None
            ctx.save_for_backward(cluster, starts)
        ctx.reduce = reduce
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _):
        cluster, starts = ctx.saved_tensors[:2]
        arg = ctx.saved_tensors[2] if ctx.reduce == "max" else None
        return _raw.grid_unpool(grad_out.contiguous(), cluster, starts, arg, _GP_BACKWARD[ctx.reduce]), None, None, None, None, None


def grid_pool(pcd, cell, feat=None, reduce="mean", origin=None, order="xyz", lengths=None):
    """Voxel-grid subsampling (KPConv's grid_subsampling, Point Transformer's GridPool, Open3D's voxel_down_sample): one row
    per occupied cell of edge `cell` -> (points (b, n, 3), feat_pooled (b, n, c) or None, lengths_out, info).  points are the
    means of each cell's points, valid rows in front in the order of `order`, zeros behind; feat (b, n, c), c <= 2048, is
    reduced per cell with `reduce` "mean", "sum" or "max".  lengths_out is the device int32 count of cells per sample, ready
    for every `lengths=` argument of this library (farthest_point_sample, knn_point, ...) without a host synchronisation;
    info is `grid_cluster`'s dict (with "arg", the winning point per cell and channel, under "max").  Sums are double in
    ascending point index and rounded once: the same bits on every call and for every batch.  Differentiable in pcd (through
    the mean, at the fixed clustering) and in feat; only the gradients that are needed are computed, by rf_grid_unpool: no
    atomics.  n <= 16384; rows that are not inside (NaN / inf rows, padding, cells beyond +-32768) are in no cell and get a
    zero gradient."""
    if reduce not in _GP_BACKWARD:
        raise ValueError("reduce must be 'mean', 'sum' or 'max'")
    x = _cloud_tensor(pcd)
    info = grid_cluster(x, cell, origin, order, lengths)
    keys = (info["order"], info["starts"], info["nclusters"], info["cluster"])
    points, _ = _GridPoolRows.apply(x, *keys, "mean")
    pooled = None
    if feat is not None:
        f = feat if isinstance(feat, torch.Tensor) else torch.as_tensor(feat)
        pooled, arg = _GridPoolRows.apply(f.to(torch.float32).contiguous(), *keys, reduce)
        if reduce == "max":
            info = dict(info, arg=arg)
    return points, pooled, info["nclusters"], info


class _GridUnpool(torch.autograd.Function):
    """rf_grid_unpool (copy); its backward is rf_grid_pool's sum over each cluster's points."""

    @staticmethod
    def forward(ctx, src, cluster, starts, order, nclusters):
        ctx.save_for_backward(cluster, starts, *(() if order is None else (order, nclusters)))
        return _raw.grid_unpool(src, cluster, mode="copy")

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dst):
        cluster, starts = ctx.saved_tensors[:2]
        if len(ctx.saved_tensors) == 4:
            order, nclusters = ctx.saved_tensors[2:]
        else:  # the points by (cluster, index), rows that are in no cluster last: a stable sort in torch, on the device
            n = cluster.shape[1]
            order = torch.argsort(torch.where(cluster < 0, n, cluster), dim=1, stable=True).to(torch.int32)
            nclusters = (cluster.max(dim=1).values + 1).clamp(min=0).to(torch.int32)
        return _raw.grid_pool(grad_dst.contiguous(), order, starts, nclusters, "sum"), None, None, None, None


def grid_unpool(feat_pooled, cluster, starts, order=None, nclusters=None):
    """Pooled rows back to the points: feat_pooled (b, n, c), one row per cell as `grid_pool` returns them -> (b, n, c), row i
    the row of point i's cell, zeros for points in no cell (rf_grid_unpool).  cluster (b, n) and starts (b, n + 1) are
    `grid_cluster`'s.  Differentiable in feat_pooled: the gradient of a cell is the double sum over its points in ascending
    index (rf_grid_pool), for which `grid_cluster`'s "order" and "nclusters" are taken from the arguments or -- given neither
    -- rebuilt from `cluster` by a stable torch sort in the backward."""
    if (order is None) != (nclusters is None):
        raise ValueError("grid_unpool takes order and nclusters together")
    f = feat_pooled if isinstance(feat_pooled, torch.Tensor) else torch.as_tensor(feat_pooled)
    return _GridUnpool.apply(f.to(torch.float32).contiguous(), _index_tensor(cluster), _index_tensor(starts),
                             None if order is None else _index_tensor(order), None if order is None else _index_tensor(nclusters))


def serialize(pcd, cell, order="z", origin=None, lengths=None):
    """The point order along a space-filling curve over the grid of edge `cell` (Point Transformer v3's serialisation):
    -> (code (b, n) int64, order (b, n) int32, inverse (b, n) int32).  code is each point's 48-bit key along `order` ("z"
    Morton, "hilbert", "xyz" row-major; code >> 3 s is the code on the grid of edge cell * 2^s for both curves), -1 for rows
    that are not inside; order lists the inside points by ascending (code, index), zeros behind them; inverse[order[r]] = r
    for the inside points and -1 elsewhere.  code and order come from the cluster kernel (`grid_cluster`); inverse is torch
    code on order -- one scatter on the device, rows behind the inside count into a spare column: no host synchronisation.
    Other axis conventions are a column permutation of pcd in front of the call."""
    info = grid_cluster(pcd, cell, origin, order, lengths, return_code=True)
    od, inside = info["order"], info["inside"]
    b, n = od.shape
    r = torch.arange(n, device=od.device, dtype=torch.int32).expand(b, n)
    live = r < inside[:, None]
    inverse = torch.full((b, n + 1), -1, device=od.device, dtype=torch.int32)
    inverse.scatter_(1, torch.where(live, od, n).long(), torch.where(live, r, -1))
    return info["code"], od, inverse[:, :n].contiguous()


def sparse_conv_map(coords, nclusters=None, kernel_size=3, dilation=1):
    """The kernel map of a submanifold sparse convolution over the occupied cells of `grid_cluster`: coords (b, n, 3) int32
    cell indices ("coords" of its dict, in any order; `coords >> s` of a coarser level too) and nclusters (b,), the cells per
    sample (its "nclusters"; None: all n) -> nbr (b, n, K) int32, K = kernel_size^3, kernel_size 3 or 5.  With r =
    kernel_size // 2, slot t = ((dx + r) ks + (dy + r)) ks + (dz + r) names the cell at offset dilation * (dx, dy, dz):
    nbr[i, t] is its row, or -1 where no cell is there.  Rows behind a count, rows with an index outside +-32768 and
    duplicates of an earlier row are all -1 and nobody names them, so nbr[i, t] == j exactly when nbr[j, K-1-t] == i.  One
    launch: a sort of the cell keys in LDS and a binary search per slot, no host synchronisation (capturable), n <= 16384
    (rf_sparse_conv_map).  Build it once per grid level and dilation; every convolution of that level shares it."""
    return _raw.sparse_conv_map(_index_tensor(coords), nclusters, kernel_size, dilation)


class _SparseConv(torch.autograd.Function):
    """rf_sparse_conv; the gradient to the features is the same kernel on the mirrored slots and the transposed weight, the
    gradient to the weight rf_sparse_conv_grad_weight.  nbr and the counts carry no gradient."""

    @staticmethod
    def forward(ctx, feat, weight, nbr, nclusters):
        ctx.save_for_backward(feat, weight, nbr)
        ctx.nclusters = nclusters
        return _raw.sparse_conv(feat, weight, nbr, nclusters)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        feat, weight, nbr = ctx.saved_tensors
        g = grad_out.contiguous()
        gf = _raw.sparse_conv(g, weight, nbr, ctx.nclusters, "grad_input") if ctx.needs_input_grad[0] else None
        gw = _raw.sparse_conv_grad_weight(feat, g, nbr, ctx.nclusters) if ctx.needs_input_grad[1] else None
        return gf, gw, None, None


def sparse_conv(feat, weight, nbr, nclusters=None):
    """Submanifold sparse convolution (spconv's SubMConv3d, MinkowskiEngine's stride-1 convolution, the 3 x 3 x 3 layers of
    SPVCNN and MinkUNet, Point Transformer v3's xCPE): feat (b, n, cin), one row per occupied cell as `grid_pool` returns
    them, weight (K, cin, cout) and `sparse_conv_map`'s nbr (b, n, K) -> (b, n, cout): out[i] = sum over the slots t whose
    cell nbr[i, t] exists of feat[nbr[i, t]] @ weight[t]; the output cells are the input cells, rows behind nclusters are
    zeros.  cin, cout <= 256.  The sum is one fp32 fmaf chain over (slot, channel) in ascending order, run on the fp32 matrix
    instruction: the same bits on every call, for every batch and shard.  Weights must be finite.  Differentiable in feat
    and weight; only the gradients that are needed are computed: the gradient to feat by the same kernel (no atomics), the
    gradient to weight by fmaf chains over 1024 rows summed in double over chunks and samples -- a sum over the batch, and
    dependent on nothing else.  nclusters may be a device tensor: no host synchronisation, capturable."""
    return _SparseConv.apply(_feature_tensor(feat), _feature_tensor(weight), _index_tensor(nbr), nclusters)


class SubMConv3d(torch.nn.Module):
    """`sparse_conv` as a layer: weight (kernel_size^3, cin, cout), kernel_size 3 or 5, an optional bias (added by torch, to
    the rows in front of the counts only).  forward(feat (b, n, cin), coords or nbr, nclusters=None): given coords (b, n, 3)
    the map is built with the layer's kernel_size and dilation; a stack of layers on one grid level builds it once with
    `sparse_conv_map` and passes nbr (b, n, K)."""

    def __init__(self, cin, cout, kernel_size=3, dilation=1, bias=True):
        super().__init__()
        if kernel_size not in (3, 5):
            raise ValueError("kernel_size must be 3 or 5")
        self.cin, self.cout, self.kernel_size, self.dilation = int(cin), int(cout), int(kernel_size), int(dilation)
        K = self.kernel_size ** 3
        self.weight = torch.nn.Parameter(torch.empty(K, self.cin, self.cout))
        self.bias = torch.nn.Parameter(torch.zeros(self.cout)) if bias else None
        bound = (K * self.cin) ** -0.5  # torch's convolution default: uniform in +-1 / sqrt(fan_in)
        torch.nn.init.uniform_(self.weight, -bound, bound)
        if bias:
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, feat, coords_or_nbr, nclusters=None):
        nbr = coords_or_nbr
        if nbr.shape[-1] == 3:  # coords (K is 27 or 125)
            nbr = sparse_conv_map(nbr, nclusters, self.kernel_size, self.dilation)
        out = sparse_conv(feat, self.weight, nbr, nclusters)
        if self.bias is not None:
            if nclusters is None:
                out = out + self.bias
            else:
                n = out.shape[1]
                cnt = torch.as_tensor(nclusters, device=out.device)
                live = torch.arange(n, device=out.device)[None, :] < cnt[:, None]
                out = out + live.unsqueeze(-1).to(out.dtype) * self.bias
        return out


def sparse_stride_map(coords, nclusters=None, max_cells=None):
    """The next coarser level of the voxel grid, for a 2 x 2 x 2 stride-2 convolution and its transpose: coords (b, n, 3) int32
    cell indices (`grid_cluster`'s "coords", or a level dict's, in any order) and nclusters (b,) (None: all n) -> a dict of
    device tensors: "coords" (b, nc, 3) the distinct cells coords >> 1 of the live rows in ascending row-major order, zeros
    behind the count; "nclusters" (b,) their count, at most nc = max_cells (default n: nothing is dropped); "total" (b,) the
    count before that cap; "child" (b, nc, 8), child[j, t] the fine row in coarse cell j at slot t = (x & 1) 4 + (y & 1) 2 +
    (z & 1), or -1; "up" (b, n), 8 j + t for a live fine row whose coarse cell was kept and -1 for every other row.  "coords"
    and "nclusters" go as they are into `sparse_conv_map` for the level's submanifold layers and into another
    `sparse_stride_map`.  One launch, no host synchronisation (capturable), n <= 16384 (rf_sparse_stride_map)."""
    co, cn, tot, child, up = _raw.sparse_stride_map(_index_tensor(coords), nclusters, max_cells)
    return {"coords": co, "nclusters": cn, "total": tot, "child": child, "up": up}


class _SparseConvStrided(torch.autograd.Function):
    """rf_sparse_conv_strided in the direction `mode` ("down" or "up"); the gradient to the features is the mode
    `mode`_grad_input, the gradient to the weight rf_sparse_conv_strided_grad_weight.  The maps and counts carry no gradient."""

    @staticmethod
    def forward(ctx, feat, weight, child, up, nclusters, nclusters_coarse, mode):
        ctx.save_for_backward(feat, weight, child, up)
        ctx.counts, ctx.mode = (nclusters, nclusters_coarse), mode
        return _raw.sparse_conv_strided(feat, weight, child, up, nclusters, nclusters_coarse, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        feat, weight, child, up = ctx.saved_tensors
        g = grad_out.contiguous()
        gf = gw = None
        if ctx.needs_input_grad[0]:
            gf = _raw.sparse_conv_strided(g, weight, child, up, *ctx.counts, ctx.mode + "_grad_input")
        if ctx.needs_input_grad[1]:
            fine, coarse = (feat, g) if ctx.mode == "down" else (g, feat)
            gw = _raw.sparse_conv_strided_grad_weight(fine, coarse, child, *ctx.counts, ctx.mode)
        return gf, gw, None, None, None, None, None


def _strided(feat, weight, level, nclusters, mode):
    return _SparseConvStrided.apply(_feature_tensor(feat), _feature_tensor(weight), _index_tensor(level["child"]),
                                    _index_tensor(level["up"]), nclusters, level["nclusters"], mode)


def sparse_conv_down(feat, weight, level, nclusters=None):
    """Strided sparse convolution, kernel 2, stride 2 (MinkowskiEngine's Convolution(kernel_size=2, stride=2), spconv's
    SparseConv3d(2, 2), the downsampling of MinkUNet and SPVCNN): feat (b, n, cin) on the fine cells, weight (8, cin, cout) and
    `sparse_stride_map`'s level dict -> (b, nc, cout) on the level's cells: out[j] = sum over the slots t with a child of
    feat[child[j, t]] @ weight[t], zeros behind the level's count.  nclusters is the fine level's count.  One fp32 fmaf chain
    over (slot, channel) ascending on the fp32 matrix instruction: the same bits on every call and for every batch.
    Differentiable in feat and weight; only the gradients that are needed are computed, without atomics."""
    return _strided(feat, weight, level, nclusters, "down")


def sparse_conv_up(feat, weight, level, nclusters=None):
    """The transpose of `sparse_conv_down` onto the fine level's cells (MinkowskiEngine's ConvolutionTranspose(kernel_size=2,
    stride=2) onto the encoder's coordinates, spconv's SparseInverseConv3d): feat (b, nc, cin) on the level's cells, weight
    (8, cin, cout) -> (b, n, cout): out[i] = feat[j] @ weight[t] for the fine row i = child[j, t], zeros for rows in no kept
    coarse cell and behind nclusters, the fine level's count.  No cell is created (`sparse_conv_generate` does that).  One
    fmaf chain over the channels per row; every fine row has one writer: no atomics.  Differentiable in feat and weight."""
    return _strided(feat, weight, level, nclusters, "up")


class _SparseStrided(torch.nn.Module):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.cin, self.cout = int(cin), int(cout)
        self.weight = torch.nn.Parameter(torch.empty(8, self.cin, self.cout))
        self.bias = torch.nn.Parameter(torch.zeros(self.cout)) if bias else None
        bound = (8 * self.cin) ** -0.5  # torch's convolution default: uniform in +-1 / sqrt(fan_in)
        torch.nn.init.uniform_(self.weight, -bound, bound)
        if bias:
            torch.nn.init.uniform_(self.bias, -bound, bound)

    @staticmethod
    def _level(coords_or_level, nclusters):
        return coords_or_level if isinstance(coords_or_level, dict) else sparse_stride_map(coords_or_level, nclusters)

    def _add_bias(self, out, cnt):
        if self.bias is None:
            return out
        if cnt is None:
            return out + self.bias
        live = torch.arange(out.shape[1], device=out.device)[None, :] < torch.as_tensor(cnt, device=out.device)[:, None]
        return out + live.unsqueeze(-1).to(out.dtype) * self.bias


class SparseConv3d(_SparseStrided):
    """`sparse_conv_down` as a layer: kernel 2, stride 2, weight (8, cin, cout), an optional bias (added by torch, to the rows
    in front of the level's count only).  forward(feat (b, n, cin), coords or level, nclusters=None) -> (b, nc, cout): given
    coords (b, n, 3) the level is built here; an encoder builds it once with `sparse_stride_map` and passes the dict, which the
    decoder's `SparseConvTranspose3d` takes too."""

    def forward(self, feat, coords_or_level, nclusters=None):
        level = self._level(coords_or_level, nclusters)
        return self._add_bias(sparse_conv_down(feat, self.weight, level, nclusters), level["nclusters"])


class SparseConvTranspose3d(_SparseStrided):
    """`sparse_conv_up` as a layer: kernel 2, stride 2, weight (8, cin, cout), an optional bias (to the rows in front of
    nclusters, the fine level's count, only).  forward(feat (b, nc, cin), coords or level, nclusters=None) -> (b, n, cout),
    coords being the FINE level's (b, n, 3) and feat living on the cells `sparse_stride_map` makes of them."""

    def forward(self, feat, coords_or_level, nclusters=None):
        level = self._level(coords_or_level, nclusters)
        return self._add_bias(sparse_conv_up(feat, self.weight, level, nclusters), nclusters)


def sparse_generate_map(coords, nclusters=None, max_cells=None):
    """The next FINER level of the voxel grid with every cell created (MinkowskiEngine's GenerativeConvolutionTranspose,
    the upsampling of SGNN-style completion decoders): coords (b, nc, 3) int32 coarse cells and nclusters (b,) (None: all nc)
    -> a dict of device tensors for the FINE level: "coords" (b, nf, 3), the eight children 2 c + bit of every live coarse row
    whose indices are in [-16384, 16383], parents in ROW order, the children of a parent in slot order t = (x & 1) 4 + (y & 1) 2
    + (z & 1), zeros behind the count; "nclusters" (b,) = 8 x the parents kept, at most nf = max_cells (default min(8 nc, 16384));
    a parent gets all eight children or none; "total" (b,) = 8 x all parents, the count without that cap; "child" (b, nc, 8), the
    fine row 8 r + t of parent j's slot t (r = j when no row is dead) or -1; "up" (b, nf) = 8 j + t, -1 behind the count.  The
    dict goes into `sparse_conv_generate`, its "coords" / "nclusters" into `sparse_conv_map`, `sparse_lookup`, `sparse_prune` and
    the next `sparse_generate_map`.  One launch, no host synchronisation (capturable) (rf_sparse_generate_map)."""
    co, cn, tot, child, up = _raw.sparse_generate_map(_index_tensor(coords), nclusters, max_cells)
    return {"coords": co, "nclusters": cn, "total": tot, "child": child, "up": up}


def sparse_conv_generate(feat, weight, gen, nclusters=None):
    """Generative transposed convolution, kernel 2, stride 2: feat (b, nc, cin) on the coarse cells, weight (8, cin, cout) and
    `sparse_generate_map`'s dict -> (b, nf, cout) on the created cells: out[8 r + t] = feat[j] @ weight[t] for parent j of rank
    r, zeros behind the dict's count.  nclusters is the COARSE level's count (the dict's "nclusters" is the fine one: the
    reverse of `sparse_conv_up`'s roles).  It is rf_sparse_conv_strided's "up" on the generated maps: one fmaf chain over the
    channels per row, every fine row one writer, the same bits on every call.  Differentiable in feat and weight."""
    return _SparseConvStrided.apply(_feature_tensor(feat), _feature_tensor(weight), _index_tensor(gen["child"]),
                                    _index_tensor(gen["up"]), gen["nclusters"], nclusters, "up")


class SparseGenerativeConvTranspose3d(_SparseStrided):
    """`sparse_conv_generate` as a layer: weight (8, cin, cout), an optional bias (to the rows in front of the fine count only).
    forward(feat (b, nc, cin), coords or gen, nclusters=None) -> (out (b, nf, cout), gen): given the coarse coords (b, nc, 3)
    the level is generated here with the default max_cells; given `sparse_generate_map`'s dict it is used as it is.  nclusters
    is the coarse level's count."""

    def forward(self, feat, coords_or_gen, nclusters=None):
        gen = coords_or_gen if isinstance(coords_or_gen, dict) else sparse_generate_map(coords_or_gen, nclusters)
        return self._add_bias(sparse_conv_generate(feat, self.weight, gen, nclusters), gen["nclusters"]), gen


class _SparseTake(torch.autograd.Function):
    """rf_sparse_take_rows by idx under the count of the destination rows; its backward is the same entry by `inverse` under the
    count of the source rows.  The maps and counts carry no gradient."""

    @staticmethod
    def forward(ctx, feat, idx, inverse, count_dst, count_src):
        ctx.save_for_backward(inverse)
        ctx.count_src = count_src
        return _raw.sparse_take_rows(feat, idx, count_dst)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        inverse, = ctx.saved_tensors
        return _raw.sparse_take_rows(grad_out.contiguous(), inverse, ctx.count_src), None, None, None, None


def sparse_take(feat, idx, inverse, nclusters=None):
    """Rows by index: feat (b, n_src, c), idx (b, n_dst) int32 -> (b, n_dst, c), row r a copy of feat[idx[r]], zeros where
    idx[r] is outside [0, n_src) (-1: no such cell) and behind nclusters, the count of the DESTINATION rows (rf_sparse_take_rows).
    Differentiable in feat: the gradient is the same copy by `inverse` (b, n_src).  PRECONDITION, not checked: idx and inverse
    are mutually inverse on their non-negative entries -- idx[r] == i >= 0 exactly when inverse[i] == r >= 0 -- so that every
    gradient row has one source and nothing is summed.  This holds for `sparse_prune`'s "src" / "dst", and for the two
    `sparse_lookup` calls at shift 0 between two levels neither of which has duplicate rows (a skip connection: idx =
    sparse_lookup(decoder, encoder), inverse = sparse_lookup(encoder, decoder)).  With duplicates, a lookup names the lowest row
    only and the gradient of the others would be lost."""
    return _SparseTake.apply(_feature_tensor(feat), _index_tensor(idx), _index_tensor(inverse), nclusters, None)


def sparse_prune(coords, keep, feat=None, nclusters=None, max_cells=None):
    """Pruning (MinkowskiEngine's MinkowskiPruning): the rows of coords (b, n, 3) with keep (b, n) set, in their order, in
    front -> a dict of device tensors: "coords" (b, no, 3), zeros behind the count; "nclusters" (b,), at most no = max_cells
    (default n); "total" (b,) the count without that cap; "src" (b, no) the row each kept row came from, "dst" (b, n) where each
    row went, -1 elsewhere; "feat" (b, no, c) the rows of feat (b, n, c) moved along, or None.  keep is a bool or uint8 tensor,
    or any other dtype taken as > 0 (a classifier's logits); rows behind nclusters are not selected.  Nothing is tested but
    keep: rows are carried as they are.  One launch for the map and one for the rows, the counts stay on the device: no
    `nonzero`, no boolean mask, no host synchronisation (capturable) (rf_sparse_prune_map, rf_sparse_take_rows).  Differentiable
    in feat: the gradient goes back by "dst"."""
    co, cn, tot, src, dst = _raw.sparse_prune_map(_index_tensor(coords), keep, nclusters, max_cells)
    moved = None if feat is None else _SparseTake.apply(_feature_tensor(feat), src, dst, cn, nclusters)
    return {"coords": co, "nclusters": cn, "total": tot, "src": src, "dst": dst, "feat": moved}


class SparsePrune(torch.nn.Module):
    """`sparse_prune` as a layer: forward(coords, keep, feat=None, nclusters=None) -> its dict; max_cells is the layer's."""

    def __init__(self, max_cells=None):
        super().__init__()
        self.max_cells = max_cells

    def forward(self, coords, keep, feat=None, nclusters=None):
        return sparse_prune(coords, keep, feat, nclusters, self.max_cells)


def sparse_lookup(coords, table, nclusters=None, table_nclusters=None, shift=0):
    """Where the cells of one set are in another: coords (b, n, 3) and table (b, m, 3) int32 with their counts -> idx (b, n)
    int32, the LOWEST row of table whose cell `table >> shift` (the arithmetic shift, per axis) equals coords[i], -1 where there
    is none, for rows behind nclusters and for rows outside +-32768.  shift = 0 maps a decoder level to the encoder's cells of
    that level (a skip connection, with `sparse_take`); shift = s tells whether a generated cell of level s is occupied among
    the ground truth's FINEST cells, without a pyramid of the target (`idx >= 0` is the occupancy label and the keep mask of
    `sparse_prune`).  One launch: a sort of the table's keys in LDS and a binary search per row, no host synchronisation
    (capturable), n, m <= 16384 (rf_sparse_lookup).  Non-differentiable."""
    return _raw.sparse_lookup(_index_tensor(coords), _index_tensor(table), nclusters, table_nclusters, shift)


class _NeighborAggregation(torch.autograd.Function):
    """rf_neighbor_aggregate / rf_neighbor_aggregate_grad: value, weight and pos carry gradients, idx does not."""

    @staticmethod
    def forward(ctx, value, weight, idx, pos, lengths1, lengths2):
        ctx.save_for_backward(value, weight, idx, pos)
        ctx.lengths = (lengths1, lengths2)
        return _raw.neighbor_aggregation(value, weight, idx, pos, lengths1, lengths2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        value, weight, idx, pos = ctx.saved_tensors
        need = ctx.needs_input_grad
        gv, gp, gw = _raw.neighbor_aggregation_grad(value, weight, idx, grad_out.contiguous(), pos, *ctx.lengths, want_value=need[0],
                                                    want_pos=pos is not None and need[3], want_weight=need[1])
        return gv, gw, None, gp, None, None


def neighbor_aggregation(value, weight, idx, pos=None, lengths1=None, lengths2=None):
    """Vector attention's weighted sum (pointops' `aggregation`, on padded batches): out[i, ch] = the sum over the k
    neighbours t of (value[idx[i, t], ch] + pos[i, t, ch]) * weight[i, t, ch mod cw] -> (b, m, c); value (b, n, c), weight
    (b, m, k, cw) with cw dividing c (Point Transformer's share_planes = c / cw), pos (b, m, k, c) or None, idx (b, m, k) from
    `knn_point`.  The softmax over k stays torch code in front of this call.  Nothing of size (b, m, k, c) is formed or kept for
    autograd; sums in double in ascending neighbour order (rf_neighbor_aggregate).  lengths1 / lengths2 as in
    `neighbor_subtraction`.  Differentiable in value, weight and pos; only the gradients that are needed are computed, the one
    to value without float atomics (rf_neighbor_aggregate_grad)."""
    p = None if pos is None else _feature_tensor(pos)
    return _NeighborAggregation.apply(_feature_tensor(value), _feature_tensor(weight), _index_tensor(idx), p, lengths1, lengths2)


class _EmdAssign(torch.autograd.Function):
    """rf_emd_assign / rf_emd_assign_grad: the exact assignment; only the cost (b,) carries a gradient, under the
    fixed assignment."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, lengths, max_rounds):
        m12, m21, dist, val, cert, info = _raw.emd_assign(xyz1, xyz2, lengths, max_rounds)
        ctx.save_for_backward(xyz1, xyz2, m12, m21)
        ctx.lengths = lengths
        ctx.mark_non_differentiable(m12, m21, dist, val, cert, info)
        return val[:, 0].clone(), m12, m21, dist, val, cert, info

    @staticmethod
    def backward(ctx, grad_cost, *_):
        xyz1, xyz2, m12, m21 = ctx.saved_tensors
        g1, g2 = _raw.emd_assign_grad(xyz1, xyz2, m12, m21, grad_cost.contiguous(), ctx.lengths)
        return g1, g2, None, None


def emd_assignment(pcd1, pcd2, lengths=None, max_rounds=0):
    """The earth mover's distance itself: the one-to-one assignment of pcd1 (b, n, 3) to pcd2 (b, n, 3) of minimal total
    distance, n <= 4096, by a deterministic integer auction (rf_emd_assign).  Returns a dict of per-sample tensors:
      match12, match21  (b, n) int32, inverse permutations     dist  (b, n) the distance of every pair
      cost   (b,) the sum of dist -- differentiable in pcd1 and pcd2 under the fixed assignment
      gap    (b,) the certified distance of the integer cost from the integer optimum, in units of distance
      bound  (b,) cost - EMD <= bound (gap plus the price of the quantisation)
      status (b,) 0 ok, 1 stopped at max_rounds (still a permutation; gap and bound still hold), 2 non-finite input
      rounds (b,) auction rounds
    plus "cert" (b, 2) int64 (P, D: the exact integers behind gap) and "info" (b, 4).  lengths (b,): per-sample point
    counts shared by both clouds; slots behind a count are zeros and get a zero gradient."""
    cost, m12, m21, dist, val, cert, info = _EmdAssign.apply(pcd1.contiguous(), pcd2.contiguous(), lengths, max_rounds)
    return {"match12": m12, "match21": m21, "dist": dist, "cost": cost, "gap": val[:, 1], "bound": val[:, 2],
            "status": info[:, 0], "rounds": info[:, 1], "cert": cert, "info": info}


def emd_exact(pcd1, pcd2, lengths=None):
    """The batch mean of cost_i / #points of the exact assignment (emd_assignment): earth_mover's normalisation, so the
    two numbers compare directly.  With lengths: cost_i / lengths[i]."""
    cost = emd_assignment(pcd1, pcd2, lengths=lengths)["cost"]
    b, n = pcd1.shape[0], pcd1.shape[1]
    ln = _raw._check_lengths(lengths, b, n, "lengths")
    if ln is None:
        return (cost / float(n)).mean()
    return (cost / ln.to(device=cost.device, dtype=cost.dtype).clamp(1, n)).mean()


class _ExpansionPenalty(torch.autograd.Function):
    """rf_expansion_penalty / rf_expansion_penalty_grad: only dist carries a gradient, under the fixed tree, mean and
    indicator (a penalty on the long edges, not on the mean)."""

    @staticmethod
    def forward(ctx, xyz, primitive_size, alpha):
        dist, father, length, mean, info = _raw.expansion_penalty(xyz, primitive_size, alpha)
        ctx.save_for_backward(xyz, father, dist)
        ctx.primitive_size = primitive_size
        ctx.mark_non_differentiable(father, length, mean, info)
        return dist, father, length, mean, info

    @staticmethod
    def backward(ctx, grad_dist, *_):
        xyz, father, dist = ctx.saved_tensors
        return _raw.expansion_penalty_grad(xyz, ctx.primitive_size, father, dist, grad_dist.contiguous()), None, None


def expansion_penalty(pcd, primitive_size, alpha=1.5, return_info=False):
    """MSN's expansion penalty: pcd (b, n, 3) is n / primitive_size surface patches of consecutive rows, each of 2 to 4096
    points.  Every patch gets its minimum spanning tree; a tree edge longer than alpha times the patch's mean edge is
    penalised with its length -> (dist (b, n): the penalised length of the edge that joined each point, else 0;
    father (b, n) int32: the row each point hangs on; mean_mst (b, P): the mean edge per patch).  dist is differentiable
    in pcd with the tree, the mean and the indicator held constant.  return_info: also length (b, n), every tree edge,
    and info (b, P) (0 ok, 1: the patch holds a non-finite coordinate and is all zeros).  One launch, no host
    synchronisation: capturable in a graph."""
    dist, father, length, mean, info = _ExpansionPenalty.apply(pcd.contiguous(), int(primitive_size), float(alpha))
    return (dist, father, mean, length, info) if return_info else (dist, father, mean)


def expansion_loss(pcd, primitive_size, alpha=1.5):
    """The mean of expansion_penalty's dist over all points: MSN's reduction."""
    return expansion_penalty(pcd, primitive_size, alpha)[0].mean()


def minimum_density_sample(pcd, npoint, sigma, lengths=None, return_xyz=False):
    """MSN's minimum density sampling: thin pcd (b, n, 3), n <= 16384, to npoint rows -- FPS's sibling, even density where
    FPS gives even coverage.  The first sample is row 0; every further one is the row whose Gaussian density
    sum exp(-d^2 / (2 sigma^2)) under the rows chosen so far is smallest (ties to the smallest index) -> idx (b, npoint)
    int32, and with return_xyz also the rows themselves (b, npoint, 3), not differentiable (gather_point(pcd, idx) is).
    sigma: a float, or a (b,) tensor that stays on the device (expansion_penalty's mean_mst.mean(1) flows in without a
    sync); a sample whose sigma is not positive gets the first npoint rows.  lengths (b,): per-sample point counts; slots
    behind min(npoint, count) are zeros."""
    res = _raw.minimum_density_sample(pcd.detach(), npoint, sigma, lengths=lengths, return_xyz=return_xyz)
    return (res[0], res[2]) if return_xyz else res[0]


def earth_mover(pcd1, pcd2, lengths1=None, lengths2=None):
    """mean over the batch of cost_i / #points (vv_recon.py:392-399).  lengths1 / lengths2: per-sample point counts of a
    ragged batch (rf_earth_mover_lengths): the mean of cost_i / lengths1[i], the ragged form of the division by
    pcd1.shape[1]; padded rows get a zero gradient."""
    if lengths1 is None and lengths2 is None:
        assert pcd1.shape[1] == pcd2.shape[1]
        cost = earth_mover_cost(pcd1, pcd2)  # approx_match -> match_cost fused: match never hits HBM
        return (cost / float(pcd1.shape[1])).mean()
    cost = earth_mover_cost(pcd1, pcd2, lengths1=lengths1, lengths2=lengths2)
    b, n = pcd1.shape[0], pcd1.shape[1]
    l1 = _raw._check_lengths(lengths1, b, n, "lengths1")
    if l1 is None:
        return (cost / float(n)).mean()
    # (device counts as the kernels read them: clamped into [1, n])
    return (cost / l1.to(device=cost.device, dtype=cost.dtype).clamp(1, n)).mean()


def re_chamfer(gt, pred, part=8):
    """Mean of chamfer_big over `part` consecutive index slices of length ptnum(gt)//8 (the
    reference hard-codes 8 for the interval), the same slice of pred against gt
    (vv_recon.py:171-193).  The slices are contiguous, so slice i of sample s is batch element
    s*part + i of ONE (b*part, interval, 3) Chamfer instead of `part` separate ones."""
    b = gt.shape[0]
    interval = int(gt.shape[1] / 8)
    g = gt[:, :part * interval].reshape(b * part, interval, 3)
    p = pred[:, :part * interval].reshape(b * part, interval, 3)
    # mean over slices of (batch mean over b) == mean over all b*part pseudo-samples
    return chamfer_big(p, g)[0]


def groupin_near(ptmat):
    return (ptmat * ptmat).sum(-1).mean(-1).mean(-1).mean()


def zero_groupnear(ptcens, rawpts, outmat, sorted_cens=None, sorted_raw=None):
    """relu(groupin_near(outmat) - 0.4 * mean(dist2)) (vv_recon.py:410-419): direction 2 only.
    With SortedCloud handles of both sets the sweep runs straight on them."""
    if isinstance(ptcens, torch.Tensor) and (ptcens.requires_grad or rawpts.requires_grad):
        _, _, dist, _ = nn_distance(ptcens, rawpts)
    elif sorted_cens is not None and sorted_raw is not None:
        _, _, dist, _ = _raw.nn_distance_sorted(sorted_cens, sorted_raw, False, True)
    else:
        _, _, dist, _ = _raw.nn_distance_dir(ptcens, rawpts, False, True)
    return torch.relu(groupin_near(outmat) - 0.4 * dist.mean())
