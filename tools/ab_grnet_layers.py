"""Cubic Feature Sampling and Gridding Reverse against the best torch routes without them, on one GPU (ms per call, device events):
  sampling forward    _raw.cubic_feature_sampling            | torch: cell indices with torch ops, then a gather of (b, c, R^3)
  sampling backward   _raw.cubic_feature_sampling_grad       | torch: autograd of that gather -- scatter_add_ of 8 n c floats into zeros
  reverse forward     _raw.gridding_reverse(compact=True)    | torch: eight shifted views, the weighted mean, cumsum + scatter
  reverse backward    _raw.gridding_reverse_grad             | torch: autograd of that
same device, same process, alternated round by round (each round is `reps` back-to-back calls between two events, the calls rotating
over two sets of inputs; the figure is the median over the rounds, with the spread next to it), then the library's own per-kernel
device times (rf_profile_*).  For the sampling's backward also the bytes: its floor is the 4 b c R^3 bytes it must store; it reads
the 32 b n c bytes of grad_feat once per channel chunk that needs them and 8 b n bytes of records.  Before anything is timed the two
routes must agree; a difference ends the run.
python tools/ab_grnet_layers.py [rounds]      (writes profiles/grnet_layers_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

LO, HI, EPS = -0.5, 0.5, 1e-6
CFS_SHAPES = [(32, n, R, c) for n in (2048, 16384) for R, c in ((32, 32), (16, 64), (8, 128))] + [(1, 16384, 32, 32)]
REV_SHAPES = [(32, 2048, 64), (32, 16384, 64), (1, 16384, 64)]
HBM = 6.3e12  # achievable bytes per second (the streaming figure this project measures against)
OUT = os.path.join(ROOT, "profiles", "grnet_layers_ab.txt")


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
        fn(0), fn(1)  # warm-up: code objects, workspaces, the allocator
    torch.cuda.synchronize()
    reps = {k: max(2, min(50, int(np.ceil(200.0 / rounds / max(window(fn, 2), 1e-3))))) for k, fn in routes.items()}
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(window(fn, reps[k]))
    return {k: (float(np.median(v)), min(v), max(v), reps[k]) for k, v in times.items()}


def report(title, res, ours, theirs):
    say(title)
    for k in (ours, theirs):
        med, lo, hi, reps = res[k]
        say(f"  {k:14s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)")
    say(f"  ratio {ours} / {theirs} (medians): {res[ours][0] / res[theirs][0]:.4f}")


def torch_cells(x, R):
    """include/rfops.h's cell rule with torch ops -> (inside (b, n) bool, the eight vertex ids (b, n, 8) int64)"""
    inv_h = float(np.float32(np.float64(R - 1) / (np.float64(np.float32(HI)) - np.float64(np.float32(LO)))))
    u = (x - LO) * inv_h
    ins = ((u >= 0) & (u <= R - 1)).all(2)
    i = u.floor().clamp(0, R - 2).long()
    v = (i[..., 0] * R + i[..., 1]) * R + i[..., 2]
    off = torch.tensor([(d >> 2) * R * R + ((d >> 1) & 1) * R + (d & 1) for d in range(8)], device=x.device)
    return ins, v[..., None] + off


def torch_cfs(x, vol):
    b, c, R = vol.shape[:3]
    n = x.shape[1]
    ins, ids = torch_cells(x, R)
    got = vol.reshape(b, c, R ** 3).gather(2, ids.reshape(b, 1, n * 8).expand(b, c, n * 8))
    return got.reshape(b, c, n, 8).permute(0, 2, 3, 1).contiguous() * ins[..., None, None]


def sampling(rounds):
    for b, n, R, c in CFS_SHAPES:
        rng = np.random.RandomState(n + R + c)
        xs = [torch.from_numpy((rng.rand(b, n, 3) - 0.5).astype(np.float32)).cuda() for _ in range(2)]
        vols = [torch.randn(b, c, R, R, R, device="cuda").requires_grad_() for _ in range(2)]
        gs = [torch.randn(b, n, 8, c, device="cuda") for _ in range(2)]
        feats = [torch_cfs(xs[k], vols[k]) for k in range(2)]  # the graphs the torch backward walks
        ours = _raw.cubic_feature_sampling(xs[0], vols[0].detach(), LO, HI)[0]
        if not torch.equal(ours, feats[0].detach()):
            sys.exit(f"sampling {b} x {n}, R = {R}, c = {c}: the forward routes differ: not timed")
        gv = _raw.cubic_feature_sampling_grad(xs[0], gs[0], R, LO, HI)
        tv, = torch.autograd.grad(feats[0], vols[0], gs[0], retain_graph=True)
        err = float((gv - tv).abs().max() / tv.abs().max())
        if err > 1e-5:
            sys.exit(f"sampling {b} x {n}, R = {R}, c = {c}: the backward routes differ by {err:.3e} of the largest entry: not timed")
        fwd = {"rf forward": lambda k: _raw.cubic_feature_sampling(xs[k], vols[k].detach(), LO, HI),
               "torch forward": lambda k: torch_cfs(xs[k], vols[k].detach())}
        bwd = {"rf backward": lambda k: _raw.cubic_feature_sampling_grad(xs[k], gs[k], R, LO, HI),
               "torch backward": lambda k: torch.autograd.grad(feats[k], vols[k], gs[k], retain_graph=True)}
        say(f"\n## sampling b = {b}, n = {n}, R = {R}, c = {c}: backward max |difference| {err:.3e} of the largest entry")
        report("forward (ms)", ab(fwd, rounds), "rf forward", "torch forward")
        res = ab(bwd, rounds)
        report("backward (ms)", res, "rf backward", "torch backward")
        kern = kernels(bwd["rf backward"])
        floor, read = 4 * b * c * R ** 3, 32 * b * n * c + 8 * b * n
        t = res["rf backward"][0] * 1e-3
        say(f"  kernels rf backward (ms per call) {kern}")
        say(f"  bytes: {floor / 2**20:.1f} MiB stored (the floor: {floor / HBM * 1e3:.4f} ms at {HBM / 1e12:.1f} TB/s), "
            f"{read / 2**20:.1f} MiB read at least; stored / time {floor / t / 1e12:.3f} TB/s, (stored + read) / time "
            f"{(floor + read) / t / 1e12:.3f} TB/s = {(floor + read) / t / HBM:.1%} of the roof")
        say(f"  kernels rf forward (ms per call) {kernels(fwd['rf forward'])}")
        del xs, vols, gs, feats, ours, gv, tv, fwd, bwd
        torch.cuda.empty_cache()


def torch_reverse(grid):
    """eight shifted views, the weighted mean per cell, the valid cells to the front by cumsum + scatter -> (points, count)"""
    b, R = grid.shape[:2]
    C, M = R - 1, (R - 1) ** 3
    w = [grid[:, dx:dx + C, dy:dy + C, dz:dz + C] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    S = sum(w)
    T = (w[4] + w[5] + w[6] + w[7], w[2] + w[3] + w[6] + w[7], w[1] + w[3] + w[5] + w[7])
    valid = (S >= EPS).reshape(b, M)
    h = (HI - LO) / (R - 1)
    ar = torch.arange(C, device=grid.device, dtype=grid.dtype)
    idx = (ar[:, None, None], ar[None, :, None], ar[None, None, :])
    safe = torch.where(S >= EPS, S, torch.ones_like(S))
    p = torch.stack([LO + (idx[a] + T[a] / safe) * h for a in range(3)], -1).reshape(b, M, 3)
    dest = torch.where(valid, valid.cumsum(1) - 1, torch.full_like(valid, M, dtype=torch.long))
    out = torch.zeros(b, M + 1, 3, device=grid.device, dtype=grid.dtype)
    out = out.scatter(1, dest[..., None].expand(b, M, 3), p * valid[..., None])
    return out[:, :M], valid.sum(1).int()


def reverse(rounds):
    for b, n, R in REV_SHAPES:
        rng = np.random.RandomState(n + R)
        M = (R - 1) ** 3
        grids = [_raw.gridding(torch.from_numpy((rng.rand(b, n, 3) - 0.5).astype(np.float32)).cuda(), R, LO, HI)[0].requires_grad_()
                 for _ in range(2)]
        gps = [torch.randn(b, M, 3, device="cuda") for _ in range(2)]
        tp = [torch_reverse(g) for g in grids]
        rows = [_raw.gridding_reverse(g.detach(), LO, HI, EPS, True)[1] for g in grids]
        pts, _, cnt = _raw.gridding_reverse(grids[0].detach(), LO, HI, EPS, True)
        if not torch.equal(cnt, tp[0][1]) or float((pts - tp[0][0].detach()).abs().max()) > 1e-5:
            sys.exit(f"reverse {b} x {n}, R = {R}: the forward routes differ: not timed")
        gg = _raw.gridding_reverse_grad(grids[0].detach(), rows[0], gps[0], LO, HI)
        tg, = torch.autograd.grad(tp[0][0], grids[0], gps[0], retain_graph=True)
        err = float((gg - tg).abs().max() / tg.abs().max())
        if err > 1e-3:
            sys.exit(f"reverse {b} x {n}, R = {R}: the backward routes differ by {err:.3e} of the largest entry: not timed")
        fwd = {"rf forward": lambda k: _raw.gridding_reverse(grids[k].detach(), LO, HI, EPS, True),
               "torch forward": lambda k: torch_reverse(grids[k].detach())}
        bwd = {"rf backward": lambda k: _raw.gridding_reverse_grad(grids[k].detach(), rows[k], gps[k], LO, HI),
               "torch backward": lambda k: torch.autograd.grad(tp[k][0], grids[k], gps[k], retain_graph=True)}
        say(f"\n## reverse b = {b}, R = {R}, the grids of rf_gridding of {n} points: {int(cnt.min())} to {int(cnt.max())} valid cells of "
            f"{M}; backward max |difference| {err:.3e} of the largest entry (torch in float32)")
        report("forward, compact (ms)", ab(fwd, rounds), "rf forward", "torch forward")
        report("backward (ms)", ab(bwd, rounds), "rf backward", "torch backward")
        say(f"  kernels rf forward (ms per call) {kernels(fwd['rf forward'])}")
        say(f"  kernels rf backward (ms per call) {kernels(bwd['rf backward'])}")
        del grids, gps, tp, rows, fwd, bwd
        torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# Cubic Feature Sampling and Gridding Reverse A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call, "
        f"box [{LO}, {HI}]^3")
    say(f"# sampling backward: sub-bricks of {_raw.CFS_BRICK}^3 vertices x {_raw.CFS_CHUNK} channels; reverse: tiles of "
        f"{_raw.GREV_TILE} cells, eps {EPS}")
    sampling(rounds)
    reverse(rounds)


if __name__ == "__main__":
    main()
