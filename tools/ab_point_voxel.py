"""Average voxelization and trilinear devoxelization against the torch routes without them, on one GPU (ms per call, device events):
  voxelize forward     _raw.avg_voxelize                | torch: nearest-vertex ids with torch ops, then either index_add_ of the
                                                        | rows into (b R^3, c) and a transpose to (b, c, R^3), or scatter_add_
                                                        | straight into (b, c, R^3); bincount and a division
  voxelize backward    _raw.avg_voxelize_grad           | torch: autograd of those (a gather)
  devoxelize forward   _raw.trilinear_devoxelize        | torch: F.grid_sample(mode="bilinear", align_corners=True) on the 5-D volume
  devoxelize backward  _raw.trilinear_devoxelize_grad   | torch: its autograd, to the volume alone and to volume and points
same device, same process, alternated round by round (each round is `reps` back-to-back calls between two events, the calls rotating
over two sets of inputs; the figure is the median over the rounds, with the spread next to it), then the library's own per-kernel
device times (rf_profile_*).  For the two scatter kernels also the bytes: what they must store (4 b c R^3, and 4 b R^3 of counts)
plus what they must read at least once (4 b n c of features, 8 b n of records, 12 b n of coordinates for the weights) over the
time, against the HBM roof.  Before anything is timed the agreement of the two routes is reported, as a fraction of the largest entry
(forward: 1e-5 expected; gradients: 1e-6); a difference above 1e-3 ends the run.
python tools/ab_point_voxel.py [rounds]      (writes profiles/point_voxel_ab.txt)"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

LO, HI = -0.5, 0.5
SHAPES = [(32, n, R, c, "uniform") for n in (2048, 16384) for R, c in ((32, 64), (16, 128), (8, 256))] + \
         [(1, 16384, 32, 64, "uniform"), (32, 2048, 32, 64, "collapsed"), (32, 16384, 32, 64, "collapsed")]
HBM = 6.3e12  # achievable bytes per second (the streaming figure this project measures against)
OUT = os.path.join(ROOT, "profiles", "point_voxel_ab.txt")


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


def report(title, res, ours):
    say(title)
    for k, (med, lo, hi, reps) in res.items():
        say(f"  {k:24s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)")
    best = min((k for k in res if k != ours), key=lambda k: res[k][0])
    say(f"  ratio {ours} / {best} (medians): {res[ours][0] / res[best][0]:.4f}")


def agree(what, ours, theirs, bar):
    err = float((ours - theirs).abs().max() / theirs.abs().max())
    if err > 1e-3:
        sys.exit(f"{what}: the routes differ by {err:.3e} of the largest entry: not timed")
    return f"{what} {err:.2e}{'' if err <= bar else ' (above the expected ' + format(bar, '.0e') + ')'}"


def inv_h_of(R):
    return float(np.float32(np.float64(R - 1) / (np.float64(np.float32(HI)) - np.float64(np.float32(LO)))))


def torch_ids(x, R):
    """include/rfops.h's nearest-vertex rule with torch ops -> flat ids (b n,) into (b R^3)"""
    b = x.shape[0]
    u = (x - LO) * inv_h_of(R)
    i = u.floor().clamp(0, R - 2)
    k = (i + (u - i >= 0.5)).long()
    ids = (k[..., 0] * R + k[..., 1]) * R + k[..., 2]
    return (ids + torch.arange(b, device=x.device)[:, None] * R ** 3).reshape(-1)


def torch_vox_rows(x, f, R):
    b, n, c = f.shape
    ids = torch_ids(x, R)
    s = torch.zeros(b * R ** 3, c, device=f.device).index_add_(0, ids, f.reshape(b * n, c))
    cnt = torch.bincount(ids, minlength=b * R ** 3).clamp(min=1)
    return (s / cnt[:, None]).reshape(b, R ** 3, c).transpose(1, 2).contiguous().reshape(b, c, R, R, R)


def torch_vox_scatter(x, f, R):
    b, n, c = f.shape
    ids = torch_ids(x, R)
    local = (ids.reshape(b, n) - torch.arange(b, device=x.device)[:, None] * R ** 3)[:, None, :].expand(b, c, n)
    s = torch.zeros(b, c, R ** 3, device=f.device).scatter_add_(2, local, f.transpose(1, 2))
    cnt = torch.bincount(ids, minlength=b * R ** 3).clamp(min=1).reshape(b, 1, R ** 3)
    return (s / cnt).reshape(b, c, R, R, R)


def torch_devox(x, vol):
    """grid_sample takes (x, y, z) = (W, H, D) in [-1, 1]: the volume's last axis is our z"""
    b, n = x.shape[:2]
    g = ((x - LO) * (2.0 / (HI - LO)) - 1.0).flip(-1).reshape(b, 1, 1, n, 3)
    return F.grid_sample(vol, g, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(b, vol.shape[1], n).transpose(1, 2)


def clouds(kind, rng, b, n, R):
    if kind == "collapsed":  # every point of a sample in one cell
        cell = rng.randint(0, R - 1, (b, 1, 3))
        return ((cell + 0.02 + 0.96 * rng.rand(b, n, 3)) / (R - 1) - 0.5).astype(np.float32)
    return (rng.rand(b, n, 3) - 0.5).astype(np.float32)


def one_shape(b, n, R, c, kind, rounds):
    rng = np.random.RandomState(n + R + c)
    xs = [torch.from_numpy(clouds(kind, rng, b, n, R)).cuda().requires_grad_() for _ in range(2)]
    xd = [x.detach() for x in xs]
    fs = [torch.randn(b, n, c, device="cuda").requires_grad_() for _ in range(2)]
    vols = [torch.randn(b, c, R, R, R, device="cuda").requires_grad_() for _ in range(2)]
    gvs = [torch.randn(b, c, R, R, R, device="cuda") for _ in range(2)]
    say(f"\n## {kind} b = {b}, n = {n}, R = {R}, c = {c}")

    # ---- voxelization
    tv = [torch_vox_rows(xd[k], fs[k], R) for k in range(2)]  # the graphs the torch backward walks
    ts = [torch_vox_scatter(xd[k], fs[k], R) for k in range(2)]
    ov, cnt0, _ = _raw.avg_voxelize(xd[0], fs[0].detach(), R, LO, HI)
    cnts = [_raw.avg_voxelize(xd[k], fs[k].detach(), R, LO, HI)[1] for k in range(2)]
    og = _raw.avg_voxelize_grad(xd[0], cnt0, gvs[0], LO, HI)
    tg, = torch.autograd.grad(tv[0], fs[0], gvs[0], retain_graph=True)
    say("  agreement, of the largest entry: " + ", ".join((agree("voxelize forward", ov, tv[0].detach(), 1e-5),
                                                           agree("voxelize backward", og, tg, 1e-6))))
    fwd = {"rf forward": lambda k: _raw.avg_voxelize(xd[k], fs[k].detach(), R, LO, HI),
           "torch index_add_ forward": lambda k: torch_vox_rows(xd[k], fs[k].detach(), R),
           "torch scatter_add_ forward": lambda k: torch_vox_scatter(xd[k], fs[k].detach(), R)}
    bwd = {"rf backward": lambda k: _raw.avg_voxelize_grad(xd[k], cnts[k], gvs[k], LO, HI),
           "torch index_add_ backward": lambda k: torch.autograd.grad(tv[k], fs[k], gvs[k], retain_graph=True),
           "torch scatter_add_ backward": lambda k: torch.autograd.grad(ts[k], fs[k], gvs[k], retain_graph=True)}
    res = ab(fwd, rounds)
    report("voxelize forward (ms)", res, "rf forward")
    kern = kernels(fwd["rf forward"])
    say(f"  kernels rf forward (ms per call) {kern}")
    traffic(res["rf forward"][0], kern.get("voxelize_brick"), 4 * b * c * R ** 3 + 4 * b * R ** 3, 4 * b * n * c + 8 * b * n)
    report("voxelize backward (ms)", ab(bwd, rounds), "rf backward")
    say(f"  kernels rf backward (ms per call) {kernels(bwd['rf backward'])}")
    del tv, ts, fwd, bwd, og, tg, ov
    torch.cuda.empty_cache()

    # ---- devoxelization
    gfs = [torch.randn(b, n, c, device="cuda") for _ in range(2)]
    td = [torch_devox(xs[k], vols[k]) for k in range(2)]
    of = _raw.trilinear_devoxelize(xd[0], vols[0].detach(), LO, HI)[0]
    ogv, ogx = _raw.trilinear_devoxelize_grad(xd[0], vols[0].detach(), gfs[0], LO, HI)
    tgv, tgx = torch.autograd.grad(td[0], (vols[0], xs[0]), gfs[0], retain_graph=True)
    say("  agreement, of the largest entry: " + ", ".join((agree("devoxelize forward", of, td[0].detach(), 1e-5),
                                                           agree("grad_vol", ogv, tgv, 1e-6), agree("grad_xyz", ogx, tgx, 1e-6))))
    fwd = {"rf forward": lambda k: _raw.trilinear_devoxelize(xd[k], vols[k].detach(), LO, HI),
           "torch grid_sample forward": lambda k: torch_devox(xd[k], vols[k].detach())}
    bwd = {"rf backward": lambda k: _raw.trilinear_devoxelize_grad(xd[k], vols[k].detach(), gfs[k], LO, HI, want_xyz=False),
           "torch backward": lambda k: torch.autograd.grad(td[k], vols[k], gfs[k], retain_graph=True)}
    bwx = {"rf backward": lambda k: _raw.trilinear_devoxelize_grad(xd[k], vols[k].detach(), gfs[k], LO, HI),
           "torch backward": lambda k: torch.autograd.grad(td[k], (vols[k], xs[k]), gfs[k], retain_graph=True)}
    report("devoxelize forward (ms)", ab(fwd, rounds), "rf forward")
    say(f"  kernels rf forward (ms per call) {kernels(fwd['rf forward'])}")
    res = ab(bwd, rounds)
    report("devoxelize backward, to the volume (ms)", res, "rf backward")
    report("devoxelize backward, to the volume and the points (ms)", ab(bwx, rounds), "rf backward")
    kern = kernels(bwx["rf backward"])
    say(f"  kernels rf backward (ms per call) {kern}")
    traffic(res["rf backward"][0], kern.get("devoxelize_brick"), 4 * b * c * R ** 3, 4 * b * n * c + 8 * b * n + 12 * b * n)


def traffic(call_ms, kernel_ms, stored, read):
    t = (kernel_ms if kernel_ms else call_ms) * 1e-3
    say(f"  bytes of the scatter kernel: {stored / 2**20:.1f} MiB stored (the floor: {stored / HBM * 1e3:.4f} ms at {HBM / 1e12:.1f} TB/s), "
        f"{read / 2**20:.1f} MiB read at least; (stored + read) / kernel time {(stored + read) / t / 1e12:.3f} TB/s = "
        f"{(stored + read) / t / HBM:.1%} of the roof")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# Average voxelization and trilinear devoxelization A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call, "
        f"box [{LO}, {HI}]^3")
    say(f"# the scatter kernels: sub-bricks of {_raw.PV_BRICK}^3 vertices x {_raw.PV_CHUNK} channels")
    for b, n, R, c, kind in SHAPES:
        one_shape(b, n, R, c, kind, rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
