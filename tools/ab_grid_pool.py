"""Grid pooling on a sparse voxel grid against the best route without the op, on one GPU (ms per call, device events):
  ours    rf_grid_cluster (one workgroup per sample: keys, the LDS sort, heads, scan), rf_grid_pool for the cell means of the
          points and of the features, rf_grid_unpool for the backward (glue.grid_pool)
  torch   int64 keys with the batch index folded in, ONE torch.unique(return_inverse, return_counts) over the whole batch -- a
          global radix sort whose number of cells comes back to the host -- then index_add_ / scatter_reduce_ into (cells, c) and
          autograd for the backward
Per shape: the clustering alone, the pooling forward (clustering + mean points + mean features), forward + backward (to the
points and the features), and max pooling forward + backward at c = 64.  Same device, same process, routes alternated round by
round (a round is `reps` back-to-back calls between two events, the calls rotating over two sets of inputs; the figure is the
median over the rounds with the spread next to it), then the library's own per-kernel device times (rf_profile_*).  Before
anything is timed the two routes are compared: the same number of cells and the same pooled rows as sets (torch orders the cells
of the whole batch by key, the op per sample; float atomics round differently).
python tools/ab_grid_pool.py [rounds] [output file]      (writes profiles/grid_pool_ab.txt)"""
import math
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw, glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

# (b, n): two cell sizes each, about 4 and about 30 points per cell on a uniform cube
SHAPES = [(32, 2048), (32, 16384), (1, 16384)]
PER_CELL = (4, 30)
CHANNELS = (3, 64, 256)
OUT = os.path.join(ROOT, "profiles", "grid_pool_ab.txt")


def say(s=""):
    """to the terminal and, line by line, to the profile: a run that ends early leaves what it measured"""
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k & 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=4):
    profile_enable(True)
    for k in range(reps):
        fn(k & 1)
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def ab(routes, rounds):
    """routes {name: fn(set)} -> {name: (median, min, max, reps)}, alternated round by round"""
    for fn in routes.values():
        fn(0), fn(1)  # warm-up: code objects, workspaces, the allocator, the libraries' choices
    torch.cuda.synchronize()
    reps = {k: max(2, min(50, int(math.ceil(200.0 / rounds / max(window(fn, 2), 1e-3))))) for k, fn in routes.items()}
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(window(fn, reps[k]))
    return {k: (float(np.median(v)), min(v), max(v), reps[k]) for k, v in times.items()}


# ---- the route without the op --------------------------------------------------------------------------------------------------
def torch_cluster(xyz, cell):
    b, n, _ = xyz.shape
    k = torch.floor((xyz - xyz.amin(1, keepdim=True)) / cell).long()
    key = (torch.arange(b, device=xyz.device)[:, None] << 48) | (k[..., 0] << 32) | (k[..., 1] << 16) | k[..., 2]
    _, inverse, counts = torch.unique(key.reshape(-1), return_inverse=True, return_counts=True)
    return inverse, counts  # (counts.numel() is a host number: the call synchronised)


def torch_pool(xyz, feat, cell, reduce):
    inverse, counts = torch_cluster(xyz.detach(), cell)
    M, c = counts.numel(), feat.shape[-1]
    den = counts[:, None].to(torch.float32)
    points = torch.zeros(M, 3, device=xyz.device).index_add_(0, inverse, xyz.reshape(-1, 3)) / den
    if reduce == "mean":
        pooled = torch.zeros(M, c, device=xyz.device).index_add_(0, inverse, feat.reshape(-1, c)) / den
    else:
        pooled = torch.full((M, c), -math.inf, device=xyz.device).scatter_reduce(0, inverse[:, None].expand(-1, c),
                                                                                  feat.reshape(-1, c), "amax")
    return points, pooled


def ours_pool(xyz, feat, cell, reduce):
    points, pooled, _, _ = glue.grid_pool(xyz, cell, feat, reduce=reduce)
    return points, pooled


def backward(route, xyz, feat, cell, reduce):
    x, f = xyz.detach().requires_grad_(), feat.detach().requires_grad_()
    points, pooled = route(x, f, cell, reduce)
    (points.sum() + pooled.sum()).backward()
    return x.grad, f.grad


def fmt(res, name):
    med, lo, hi, reps = res[name]
    return f"  {name:34s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)"


def pair(res, what):
    o, t = res[f"ours  {what}"], res[f"torch {what}"]
    say(fmt(res, f"ours  {what}"))
    say(fmt(res, f"torch {what}"))
    verdict = "LOSES" if o[0] > t[0] else "wins"
    say(f"  ours / torch (medians) {what}: {o[0] / t[0]:.3f}  {verdict}")


def one_shape(b, n, per_cell, rounds):
    cell = float((per_cell / n) ** (1.0 / 3.0))
    g = torch.Generator(device="cuda").manual_seed(n + per_cell)
    xs = [torch.rand(b, n, 3, device="cuda", generator=g) for _ in range(2)]
    info = _raw.grid_cluster(xs[0], cell)
    M = info["nclusters"].sum().item()
    say(f"\n## b = {b}, n = {n}, cell = {cell:.4f}: {M} cells, {b * n / M:.1f} points per occupied cell")
    _, counts = torch_cluster(xs[0], cell)
    sizes = np.diff(info["starts"].cpu().numpy().astype(np.int64), axis=1)
    same = sorted(counts.tolist()) == sorted(sizes[sizes > 0].tolist())
    say(f"  agreement: torch.unique finds {counts.numel()} cells (fp32 cell arithmetic there, double here); the cell sizes are "
        f"{'equal' if same else 'NOT equal'} as multisets")
    res = ab({"ours  cluster": lambda s: _raw.grid_cluster(xs[s], cell), "torch cluster": lambda s: torch_cluster(xs[s], cell)}, rounds)
    pair(res, "cluster")
    say(f"  kernels ours (ms per call) {kernels(lambda s: _raw.grid_cluster(xs[s], cell))}")
    for c in CHANNELS:
        fs = [torch.randn(b, n, c, device="cuda", generator=g) for _ in range(2)]
        po, pt = ours_pool(xs[0], fs[0], cell, "mean")[1], torch_pool(xs[0], fs[0], cell, "mean")[1]
        live = po[torch.arange(n, device="cuda")[None] < info["nclusters"][:, None]]
        err = float((live.sum(0) - pt.sum(0)).abs().max() / pt.abs().sum(0).max())
        say(f"  c = {c}: pooled rows {tuple(live.shape)} against {tuple(pt.shape)}, column sums agree to {err:.1e} (relative)")
        routes = {}
        for name, route in (("ours ", ours_pool), ("torch", torch_pool)):
            routes[f"{name} forward c={c}"] = lambda s, r=route: r(xs[s], fs[s], cell, "mean")
            routes[f"{name} fwd+bwd c={c}"] = lambda s, r=route: backward(r, xs[s], fs[s], cell, "mean")
            if c == 64:
                routes[f"{name} max fwd+bwd c={c}"] = lambda s, r=route: backward(r, xs[s], fs[s], cell, "max")
        res = ab(routes, rounds)
        for what in (f"forward c={c}", f"fwd+bwd c={c}") + ((f"max fwd+bwd c={c}",) if c == 64 else ()):
            pair(res, what)
        say(f"  kernels ours, fwd+bwd (ms per call) {kernels(routes[f'ours  fwd+bwd c={c}'])}")
        del fs, routes
        torch.cuda.empty_cache()


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# grid pooling A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call, medians with min and max")
    say("# ours = rf_grid_cluster + rf_grid_pool (+ rf_grid_unpool backward) ; torch = int64 keys, one torch.unique over the batch "
        "(host sync), index_add_ / scatter_reduce, autograd")
    for b, n in SHAPES:
        for per_cell in PER_CELL:
            one_shape(b, n, per_cell, rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
