"""The Gridding loss with gradients, on one GPU (ms per forward + gradients, device events):
  gridding  _raw.gridding_loss(A, B, R, lo, hi, want_grad=True): one call, loss, inside counts and both gradients,
  torch     the best route without it: fp32 cell indices and trilinear weights with torch ops, eight scatter_add_ per cloud
            into (b, R^3) float grids, the L1 mean, backward of the sum by autograd -- same device, same process,
alternated round by round (each round is `reps` back-to-back steps between two events; the figure is the median over the
rounds, with the spread next to it), then the library's own per-kernel device times (rf_profile_*) and the workspace of both
routes.  Inputs are seeded uniform-cube clouds, and one pair of collapsed clouds (every point of a cloud in one place).  Before
anything is timed the two losses must agree within the quantisation bound of tests/test_gridding_host.py,
(I1 + I2) (12 / Q + 24 R 2^-22) / R^3, and the gradients are compared where no sign is at stake; a difference ends the run.
python tools/ab_gridding.py [rounds]      (writes profiles/gridding_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import lib, profile_collect, profile_enable  # noqa: E402

LO, HI = -0.5, 0.5
SHAPES = [(32, 2048, 16384, 64, "uniform"), (32, 2048, 16384, 128, "uniform"), (32, 16384, 16384, 64, "uniform"),
          (32, 16384, 16384, 128, "uniform"), (1, 16384, 16384, 64, "uniform"), (1, 65536, 65536, 64, "collapsed")]
OUT = os.path.join(ROOT, "profiles", "gridding_ab.txt")


def say(s=""):
    """to the terminal and, line by line, to the profile: a run that ends early leaves what it measured"""
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def cloud_pair(b, n, m, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "collapsed":
        A = np.broadcast_to(np.array([0.013, -0.207, 0.331], np.float32), (b, n, 3)).copy()
        B = np.broadcast_to(np.array([-0.411, 0.122, 0.018], np.float32), (b, m, 3)).copy()
    else:
        A = (rng.rand(b, n, 3) - 0.5).astype(np.float32)
        B = ((rng.rand(b, m, 3) - 0.5) * 0.9).astype(np.float32)
    return torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()


def torch_gridding_loss(A, B, R):
    """include/rfops.h's definitions with torch ops in fp32, unquantised; -> (loss, grad1, grad2)"""
    x, y = A.clone().requires_grad_(), B.clone().requires_grad_()
    inv_h = float(np.float32(np.float64(R - 1) / (np.float64(np.float32(HI)) - np.float64(np.float32(LO)))))

    def grid(p):
        b = p.shape[0]
        u = (p - LO) * inv_h
        ins = ((u >= 0) & (u <= R - 1)).all(2).to(u.dtype)
        i = u.detach().floor().clamp(0, R - 2)
        t = u - i
        il = i.long()
        w = (1.0 - t, t)
        G = torch.zeros(b, R ** 3, device=p.device, dtype=torch.float32)
        for d in range(8):
            dx, dy, dz = d >> 2, (d >> 1) & 1, d & 1
            idx = ((il[..., 0] + dx) * R + il[..., 1] + dy) * R + il[..., 2] + dz
            G.scatter_add_(1, idx, w[dx][..., 0] * w[dy][..., 1] * w[dz][..., 2] * ins)
        return G

    loss = (grid(x) - grid(y)).abs().mean(1)
    loss.sum().backward()
    return loss.detach(), x.grad, y.grad


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=4):
    profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def timing(rounds):
    for b, n, m, R, kind in SHAPES:
        A, B = cloud_pair(b, n, m, kind, n + m + R)
        out = {}

        def ours():
            out["ours"] = _raw.gridding_loss(A, B, R, LO, HI, want_grad=True)

        def theirs():
            out["torch"] = torch_gridding_loss(A, B, R)

        ours()
        theirs()
        torch.cuda.synchronize()
        loss, inside, g1, g2 = out["ours"]
        tl, t1, t2 = out["torch"]
        bound = inside.sum(1).double() * (12 / _raw.GR_Q + 24 * R * 2.0 ** -22) / R ** 3
        err = (loss.double() - tl.double()).abs()
        # the gradients agree except where the quantised and the float grid disagree on a sign: report the fraction of entries
        # within 1e-3 of the largest entry
        gd = [float(((g - t).abs() <= 1e-3 * t.abs().max()).double().mean()) for g, t in ((g1, t1), (g2, t2))]
        if not bool((err <= bound).all()):
            sys.exit(f"{b} x {n} x {m}, R = {R}, {kind}: the two losses differ by {float(err.max()):.3e}, above the bound "
                     f"{float(bound.min()):.3e}: not timed")
        once = {"gridding": window(ours, 1), "torch": window(theirs, 1)}
        reps = {k: max(1, min(50, int(np.ceil(200.0 / rounds / v)))) for k, v in once.items()}
        times = {"gridding": [], "torch": []}
        for _ in range(rounds):
            times["gridding"].append(window(ours, reps["gridding"]))
            times["torch"].append(window(theirs, reps["torch"]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        say(f"\n## b = {b}, n = {n}, m = {m}, R = {R}, {kind}: loss max |difference| {float(err.max()):.3e} (bound "
            f"{float(bound.min()):.3e}), gradient entries within 1e-3 of the largest: {gd[0]:.4f} / {gd[1]:.4f}")
        for k, v in times.items():
            say(f"{k:8s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}   ({rounds} rounds of {reps[k]} steps)")
        say(f"ratio gridding / torch (medians): {med['gridding'] / med['torch']:.4f}")
        say(f"kernels gridding (ms per call) {kernels(ours)}")
        only = lambda: _raw.gridding_loss(A, B, R, LO, HI)  # noqa: E731
        only()
        say(f"loss only: median {np.median([window(only, reps['gridding']) for _ in range(rounds)]):.4f}   kernels {kernels(only)}")
        say(f"workspace: rf_gridding_loss {lib.rf_gridding_loss_workspace_bytes(b, n, m, R, 1) / 2**20:.2f} MiB with gradients, "
            f"{lib.rf_gridding_loss_workspace_bytes(b, n, m, R, 0) / 2**20:.2f} MiB without; torch: "
            f"{2 * 2 * 4 * b * R ** 3 / 2**20:.1f} MiB of grids and their gradients, {8 * (8 + 4) * b * (n + m) / 2**20:.1f} MiB of "
            f"indices and weights kept for the backward")
        del out, A, B
        torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# Gridding loss A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per forward + gradients, COUNTS mode, "
        f"box [{LO}, {HI}]^3")
    say(f"# weight steps per axis {_raw.GR_Q}, brick edge {_raw.GR_BRICK} vertices")
    timing(rounds)


if __name__ == "__main__":
    main()
