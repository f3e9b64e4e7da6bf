"""The sliced Wasserstein distance with gradients, on one GPU (ms per forward + gradients, device events):
  sliced  _raw.sliced_wasserstein(A, B, dirs, want_grad=True): one call, loss and both gradients,
  torch   the best route without it: (x @ dirs.T), torch.sort along the points, mean((s1 - s2)^2) per sample, and
          autograd's backward of the sum -- equal counts only, three (b, nproj, n) tensors per cloud,
alternated round by round in one process (each round is `reps` back-to-back steps between two events, sized so that a
side runs for at least half a second over the rounds; the figure is the median over the rounds, with the spread next to
it), then the library's own per-kernel device times (rf_profile_*).  Inputs are seeded uniform-cube clouds and unit
directions; losses (rel 1e-4) and gradients (1e-2 of the largest entry, 1e-3 in the L2 norm: where two projections of a
cloud are within an ulp, the two routes' fp32 projections order them differently and a point legitimately gets its
neighbour's partner) of the two routes are compared before anything is timed, and a difference ends the run with an
error.  One ragged row (random counts in [n / 4, n]) is the new call alone: the torch route has no ragged form.  For
scale, _raw.earth_mover(with_grad=True) at the same shapes, same process.
python tools/ab_sliced.py [rounds]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import lib, profile_collect, profile_enable  # noqa: E402

SHAPES = [(32, 2048, 2048, 128), (32, 16384, 16384, 128)]  # b, n, m, nproj


def routes(b, n, m, nproj, seed):
    rng = np.random.RandomState(seed)
    A = torch.from_numpy((rng.rand(b, n, 3) - 0.5).astype(np.float32)).cuda()
    B = torch.from_numpy((rng.rand(b, m, 3) - 0.5).astype(np.float32)).cuda()
    d = rng.randn(nproj, 3)
    D = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).cuda()
    l1 = torch.from_numpy(rng.randint(n // 4, n + 1, b).astype(np.int32)).cuda()
    l2 = torch.from_numpy(rng.randint(m // 4, m + 1, b).astype(np.int32)).cuda()
    out = {}

    def sliced():
        out["sliced"] = _raw.sliced_wasserstein(A, B, D, want_grad=True)

    def ragged():
        out["ragged"] = _raw.sliced_wasserstein(A, B, D, l1, l2, want_grad=True)

    def torch_route():
        x, y = A.clone().requires_grad_(), B.clone().requires_grad_()
        s1 = torch.sort((x @ D.t()).transpose(1, 2), dim=-1).values
        s2 = torch.sort((y @ D.t()).transpose(1, 2), dim=-1).values
        loss = ((s1 - s2) ** 2).mean(dim=(1, 2))
        loss.sum().backward()
        out["torch"] = (loss.detach(), x.grad, y.grad)

    def emd():
        out["emd"] = _raw.earth_mover(A, B, with_grad=True)

    return sliced, ragged, torch_route, emd, out


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=3):
    profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    torch.cuda.init()
    print(f"# Sliced Wasserstein A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per forward + gradients")
    print(f"# SW_DIR_CHUNK = {_raw.SW_DIR_CHUNK} directions per chunk")
    for b, n, m, nproj in SHAPES:
        sliced, ragged, torch_route, emd, out = routes(b, n, m, nproj, n + b)
        for _ in range(2):  # warm-up of both, and the check that they are the same loss and gradients
            sliced()
            torch_route()
        torch.cuda.synchronize()
        errs, l2 = [], []
        for k, (got, want) in enumerate(zip(out["sliced"], out["torch"])):
            got, want = got.double(), want.double()
            if k == 0:
                errs.append(float(((got - want).abs() / want.abs()).max()))
            else:
                errs.append(float((got - want).abs().max() / want.abs().max()))
                l2.append(float((got - want).norm() / want.norm()))
        if not (errs[0] <= 1e-4 and max(errs[1:]) <= 1e-2 and max(l2) <= 1e-3):
            sys.exit(f"{b} x {n} x {m}, {nproj} directions: the two routes differ (loss rel, grad1, grad2 max; L2) {errs} {l2}: not timed")
        once = {"sliced": window(sliced, 2), "torch": window(torch_route, 2)}
        reps = {k: max(1, int(np.ceil(500.0 / rounds / v))) for k, v in once.items()}  # >= 0.5 s per side over the rounds
        times = {"sliced": [], "torch": []}
        for _ in range(rounds):
            times["sliced"].append(window(sliced, reps["sliced"]))
            times["torch"].append(window(torch_route, reps["torch"]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"\n## b = {b}, n = {n}, m = {m}, nproj = {nproj}   the two routes: loss max rel difference {errs[0]:.2e}, "
              f"gradients {errs[1]:.2e} / {errs[2]:.2e} of the largest entry, {l2[0]:.2e} / {l2[1]:.2e} in the L2 norm")
        for k, v in times.items():
            print(f"{k:6s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}   ({rounds} rounds of {reps[k]} steps, "
                  f"{sum(v) * reps[k] / 1e3:.2f} s)")
        print(f"ratio sliced / torch (medians): {med['sliced'] / med['torch']:.4f}")
        ragged()
        rag = [window(ragged, reps["sliced"]) for _ in range(rounds)]
        print(f"ragged (the new call alone, counts in [n / 4, n]) median {np.median(rag):.4f}  min {min(rag):.4f}  max {max(rag):.4f}")
        emd()
        em = [window(emd, 2) for _ in range(3)]
        print(f"for scale: earth_mover with gradients, same shape: median {np.median(em):.4f}  min {min(em):.4f}  max {max(em):.4f}")
        print(f"workspace: sliced with gradients {lib.rf_sliced_wasserstein_workspace_bytes(b, n, m, nproj, 1) / 2**20:.1f} MiB, "
              f"loss only {lib.rf_sliced_wasserstein_workspace_bytes(b, n, m, nproj, 0) / 2**20:.1f} MiB; torch: "
              f"{16 * b * nproj * (n + m) / 2**20:.1f} MiB of (b, nproj, n) tensors (projections, sorted values, int64 indices, per cloud)")
        print("kernels sliced (ms per step)", kernels(sliced))
        print("kernels ragged (ms per step)", kernels(ragged))
        del out, sliced, ragged, torch_route, emd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
