"""The Chamfer matrix of two collections of clouds, on one GPU (ms per matrix, device events):
  cross   _raw.chamfer_cross(A, B): each collection sorted once, one pair-indexed sweep, nothing stored per point,
  rows    the best route without it: one sorted handle of B (_raw.nn_sort, made once, outside the timing) and then, per
          row i of the matrix, _raw.chamfer_loss(A[i:i+1].expand(r, n, 3).contiguous(), B, sorted2=handle),
alternated round by round in one process (each round is `reps` back-to-back matrices between two events, sized so that a
side runs for at least half a second over the rounds; the figure is the median over the rounds, with the spread next to
it), then the library's own per-kernel device times of either route (rf_profile_*).  Inputs are seeded uniform-cube clouds;
columns 0, 1 of the two routes are compared at rel 1e-5 before anything is timed, and a difference ends the run with an error.
python tools/ab_chamfer_cross.py [rounds]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import lib, profile_collect, profile_enable  # noqa: E402

SHAPES = [(32, 32, 2048, 2048), (8, 64, 16384, 16384)]  # s, r, n, m


def routes(s, r, n, m, seed):
    rng = np.random.RandomState(seed)
    A = torch.from_numpy((rng.rand(s, n, 3) - 0.5).astype(np.float32)).cuda()
    B = torch.from_numpy((rng.rand(r, m, 3) - 0.5).astype(np.float32)).cuda()
    handle = _raw.nn_sort(B)
    out = {}

    def cross():
        out["cross"] = _raw.chamfer_cross(A, B)

    def rows():
        out["rows"] = torch.stack([_raw.chamfer_loss(A[i:i + 1].expand(r, n, 3).contiguous(), B, sorted2=handle)[0]
                                   for i in range(s)])

    return cross, rows, out


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=5):
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
    print(f"# Chamfer matrix A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per (s, r) matrix")
    for s, r, n, m in SHAPES:
        cross, rows, out = routes(s, r, n, m, n + r)
        for _ in range(3):  # warm-up of both, and the check that they are the same matrix
            cross()
            rows()
        torch.cuda.synchronize()
        got, want = out["cross"][..., 0:2].double(), out["rows"][..., 0:2].double()
        err = float(((got - want).abs() / want.abs()).max())
        if not err <= 1e-5:
            sys.exit(f"{s} x {r} x {n} x {m}: columns 0, 1 of the two routes differ by rel {err:.3e}: not timed")
        once = {"cross": window(cross, 3), "rows": window(rows, 3)}
        reps = {k: max(1, int(np.ceil(500.0 / rounds / v))) for k, v in once.items()}  # >= 0.5 s per side over the rounds
        times = {"cross": [], "rows": []}
        for _ in range(rounds):
            times["cross"].append(window(cross, reps["cross"]))
            times["rows"].append(window(rows, reps["rows"]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"\n## s = {s}, r = {r}, n = {n}, m = {m}   columns 0, 1 of the two routes: max rel difference {err:.2e}")
        for k, v in times.items():
            print(f"{k:6s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}   ({rounds} rounds of {reps[k]} matrices, "
                  f"{sum(v) * reps[k] / 1e3:.2f} s)")
        print(f"ratio cross / rows (medians): {med['cross'] / med['rows']:.4f}")
        print(f"workspace: cross {lib.rf_chamfer_cross_workspace_bytes(s, r, n, m) / 2**20:.1f} MiB; rows, per call: "
              f"{lib.rf_chamfer_loss_workspace_bytes(r, n, m, 0, 1, 1, 1) / 2**20:.1f} MiB + dist / idx {8 * r * (n + m) / 2**20:.1f} MiB")
        print("kernels cross (ms per matrix)", kernels(cross))
        print("kernels rows  (ms per matrix)", kernels(rows))


if __name__ == "__main__":
    main()
