"""The Sinkhorn divergence with gradients, on one GPU (ms per forward + gradients, device events):
  sinkhorn  _raw.sinkhorn(A, B, eps, p, want_grad=True): one call, loss, potentials, delta and both gradients,
  torch     the best route without it: the four cost matrices once (from coordinate differences: torch.cdist's matmul form
            moves the loss by 3e-4 and the gradients by 4e-3 of their largest entry, measured, and its exact form does not
            launch at these sizes), the batch in slices that fit the memory, the same Jacobi schedule with
            torch.logsumexp under no_grad, the final soft-min with autograd on, backward of the sum -- the same
            convention (the gradient through the last step only), same device, same process,
alternated round by round (each round is `reps` back-to-back steps between two events; the figure is the median over the
rounds, with the spread next to it), then the library's own per-kernel device times (rf_profile_*).  Inputs are seeded
uniform-cube clouds inside the unit ball.  Losses (rel 1e-4) and gradients (1e-3 of the largest entry) of the two routes
are compared before anything is timed, and a difference ends the run with an error.  For scale, glue.earth_mover with
gradients at the same shapes, same process.

Then quality at n = m = 2048, p = 1: S_eps with delta for blur 0.1 / 0.05 / 0.02 next to glue.emd_exact and
glue.earth_mover on the same clouds.
python tools/ab_sinkhorn.py [rounds]      (writes profiles/sinkhorn_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw, glue  # noqa: E402
from rfnet_amd._lib import lib, profile_collect, profile_enable  # noqa: E402

SHAPES = [(32, 2048, 2048), (32, 2048, 16384)]  # b, n, m
SCALINGS = [0.5, 0.9]
P, BLUR = 1, 0.05
OUT = os.path.join(ROOT, "profiles", "sinkhorn_ab.txt")


def say(s=""):
    """to the terminal and, line by line, to the profile: a run that ends early leaves what it measured"""
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def cloud_pair(b, n, m, seed):
    rng = np.random.RandomState(seed)
    A = torch.from_numpy((rng.rand(b, n, 3) - 0.5).astype(np.float32)).cuda()
    B = torch.from_numpy(((rng.rand(b, m, 3) - 0.5) * 0.9).astype(np.float32)).cuda()
    return A, B


TORCH_CHUNK_PAIRS = 1 << 30  # the torch route takes the batch in slices of at most this many pairs of the largest matrix


def torch_sinkhorn(A, B, eps, p):
    """include/rfops.h's iteration with torch ops; -> (loss, grad1, grad2).  The batch goes through in slices: at 32 x 16384^2
    one cost matrix is 34 GB and the final step keeps several of them for its backward."""
    big = max(A.shape[1], B.shape[1])
    step = max(1, min(A.shape[0], TORCH_CHUNK_PAIRS // (big * big)))
    parts = [_torch_sinkhorn(A[i:i + step], B[i:i + step], eps, p) for i in range(0, A.shape[0], step)]
    return tuple(torch.cat(t) for t in zip(*parts))


def _torch_sinkhorn(A, B, eps, p):
    x, y = A.clone().requires_grad_(), B.clone().requires_grad_()
    n, m = x.shape[1], y.shape[1]
    la, lb = -float(np.log(n)), -float(np.log(m))

    def cost(u, v):
        # from differences: torch.cdist's matmul form moves the loss by 3e-4 and the gradients by 4e-3 of their largest
        # entry (measured), and its exact form does not launch at these sizes ("invalid configuration argument")
        d2 = sum((u[:, :, None, k] - v[:, None, :, k]) ** 2 for k in range(3))
        return d2.clamp_min(1e-30).sqrt() if p == 1 else 0.5 * d2  # (the clamp: a zero gradient at distance 0, not NaN)

    def softmin(C, h, lw, e):
        return -e * torch.logsumexp((h[:, None, :] - C) / e + lw, dim=2)

    with torch.no_grad():
        Cxy, Cxx, Cyy = cost(x, y), cost(x, x), cost(y, y)
        Cyx = Cxy.transpose(1, 2)
        f, g, fx, gy = (torch.zeros_like(t[:, :, 0]) for t in (x, y, x, y))
        for e in eps:
            f, g, fx, gy = (0.5 * (f + softmin(Cxy, g, lb, e)), 0.5 * (g + softmin(Cyx, f, la, e)),
                            0.5 * (fx + softmin(Cxx, fx, la, e)), 0.5 * (gy + softmin(Cyy, gy, lb, e)))
        del Cxy, Cyx, Cxx, Cyy
    e = eps[-1]
    xd, yd = x.detach(), y.detach()  # the column arguments are held fixed
    loss = ((softmin(cost(x, yd), g, lb, e) - softmin(cost(x, xd), fx, la, e)).mean(1)
            + (softmin(cost(y, xd), f, la, e) - softmin(cost(y, yd), gy, lb, e)).mean(1))
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


def kernels(fn, reps=2):
    profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def timing(rounds):
    for b, n, m in SHAPES:
        A, B = cloud_pair(b, n, m, n + m)
        for scaling in SCALINGS:
            eps = glue.sinkhorn_schedule(P, BLUR, scaling)
            out = {}

            def ours():
                out["ours"] = _raw.sinkhorn(A, B, eps, P, want_grad=True)

            def theirs():
                out["torch"] = torch_sinkhorn(A, B, eps, P)

            ours()
            theirs()
            torch.cuda.synchronize()
            loss, pot, delta, g1, g2 = out["ours"]
            tl, t1, t2 = out["torch"]
            errs = [float(((loss.double() - tl.double()).abs() / tl.double().abs()).max()),
                    float((g1 - t1).abs().max() / t1.abs().max()), float((g2 - t2).abs().max() / t2.abs().max())]
            if not (errs[0] <= 1e-4 and max(errs[1:]) <= 1e-3):
                sys.exit(f"{b} x {n} x {m}, scaling {scaling}: the two routes differ (loss rel, grad1, grad2) {errs}: not timed")
            once = {"sinkhorn": window(ours, 1), "torch": window(theirs, 1)}
            reps = {k: max(1, min(20, int(np.ceil(300.0 / rounds / v)))) for k, v in once.items()}
            times = {"sinkhorn": [], "torch": []}
            for _ in range(rounds):
                times["sinkhorn"].append(window(ours, reps["sinkhorn"]))
                times["torch"].append(window(theirs, reps["torch"]))
            med = {k: float(np.median(v)) for k, v in times.items()}
            say(f"\n## b = {b}, n = {n}, m = {m}, p = {P}, blur {BLUR}, scaling {scaling}: {len(eps)} steps   the two routes: "
                f"loss max rel difference {errs[0]:.2e}, gradients {errs[1]:.2e} / {errs[2]:.2e} of the largest entry; "
                f"delta max {float(delta.max()):.3e}")
            for k, v in times.items():
                say(f"{k:8s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}   ({rounds} rounds of {reps[k]} steps)")
            say(f"ratio sinkhorn / torch (medians): {med['sinkhorn'] / med['torch']:.4f}")
            say(f"kernels sinkhorn (ms per call) {kernels(ours)}")
            del out
            torch.cuda.empty_cache()
        fn = lambda: _raw.earth_mover(A, B, with_grad=True)  # noqa: E731
        fn()
        em = [window(fn, 2) for _ in range(3)]
        say(f"for scale: earth_mover with gradients, b = {b}, n = {n}, m = {m}: median {np.median(em):.4f}  min {min(em):.4f}  "
            f"max {max(em):.4f}")
        say(f"workspace: rf_sinkhorn {lib.rf_sinkhorn_workspace_bytes(b, n, m) / 2**20:.1f} MiB; torch: "
            f"{4 * b * (2 * n * m + n * n + m * m) / 2**20:.1f} MiB of cost matrices, and as much again per logsumexp")
        del A, B
        torch.cuda.empty_cache()


def quality():
    b, n = 4, 2048
    A, B = cloud_pair(b, n, n, 77)
    exact = float(glue.emd_exact(A, B))
    approx = float(glue.earth_mover(A, B))
    say(f"\n## quality at b = {b}, n = m = {n}, p = 1 (batch means; cost per point)")
    say(f"emd_exact {exact:.6f}   earth_mover {approx:.6f} ({approx / exact:.4f} of exact)")
    for blur in (0.1, 0.05, 0.02):
        for scaling in SCALINGS:
            loss, info = glue.sinkhorn_divergence(A, B, p=1, blur=blur, scaling=scaling, return_info=True)
            s = float(loss.mean())
            say(f"blur {blur:<5} scaling {scaling}: S_eps {s:.6f} ({s / exact:.4f} of exact)   delta max {float(info['delta'].max()):.3e}")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# Sinkhorn divergence A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per forward + gradients")
    say(f"# column tile {_raw.SK_COL_TILE}, at most {_raw.SK_NSPLIT} column chunks per row")
    quality()
    timing(rounds)


if __name__ == "__main__":
    main()
