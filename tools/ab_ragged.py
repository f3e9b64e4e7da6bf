"""Ragged Chamfer batches on one GPU: the same seeded inputs timed three ways (ms per call, hipEvents via torch):
  ragged   one call with per-sample lengths (rf_nn_distance_lengths / rf_chamfer_loss_lengths + grad),
  full     the existing call on the same padded tensors at full size (what a caller pays today, wrong results aside),
  loop     a Python loop of existing per-sample calls on the unpadded slices.
Forward only (nn_distance; also with each route pinned) and forward + backward through glue.chamfer_per_sample, then the
library's per-kernel device times of the ragged and full calls.  Lengths are device tensors.
python tools/ab_ragged.py [reps]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw, glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

B = 32
# (label, n, m, lengths1 range, lengths2 range); None = all points
SHAPES = [
    ("fidelity 3000 x 16384, len1 in [1000, 3000]", 3000, 16384, (1000, 3000), None),
    ("16384 x 16384, both in [4096, 16384]", 16384, 16384, (4096, 16384), (4096, 16384)),
    ("2048 x 2048, both in [512, 2048]", 2048, 2048, (512, 2048), (512, 2048)),
    ("16384 x 16384, both in [1, 64]", 16384, 16384, (1, 64), (1, 64)),
    ("65536 x 65536, both in [1, 64]", 65536, 65536, (1, 64), (1, 64)),
]


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=10):
    """Per-kernel device time of one call (the library's own event brackets), ms."""
    fn()
    torch.cuda.synchronize()
    profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def lengths(rng, n, rng_range):
    if rng_range is None:
        return np.full(B, n, np.int32)
    lo, hi = rng_range
    return rng.randint(lo, hi + 1, size=B).astype(np.int32)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.init()
    print(f"# ragged Chamfer A/B on {torch.cuda.get_device_name(0)}, B={B}, {reps} reps per figure, ms per call")
    for label, n, m, r1, r2 in SHAPES:
        rng = np.random.RandomState(n + m)
        a = torch.from_numpy(rng.randn(B, n, 3).astype(np.float32)).cuda()
        c = torch.from_numpy(rng.randn(B, m, 3).astype(np.float32)).cuda()
        l1h, l2h = lengths(rng, n, r1), lengths(rng, m, r2)
        l1, l2 = torch.from_numpy(l1h).cuda(), torch.from_numpy(l2h).cuda()
        slices = [(a[i:i + 1, :l1h[i]].contiguous(), c[i:i + 1, :l2h[i]].contiguous()) for i in range(B)]
        route = "culled" if _raw.lib.rf_nn_distance_mode_workspace_bytes(B, n, m, 0) == \
            _raw.lib.rf_nn_distance_mode_workspace_bytes(B, n, m, 2) else "dense"
        print(f"\n## {label}  (AUTO route at full size: {route}; mean len1 {l1h.mean():.0f}, mean len2 {l2h.mean():.0f})")

        fwd = {
            "ragged": lambda: _raw.nn_distance(a, c, lengths1=l1, lengths2=l2),
            "full": lambda: _raw.nn_distance(a, c),
            "loop": lambda: [_raw.nn_distance(x, y) for x, y in slices],
        }
        for mode in ("dense", "culled"):
            fwd[f"ragged[{mode}]"] = (lambda md: lambda: _raw.nn_distance(a, c, mode=md, lengths1=l1, lengths2=l2))(mode)
            fwd[f"full[{mode}]"] = (lambda md: lambda: _raw.nn_distance(a, c, mode=md))(mode)
        for k, fn in fwd.items():
            print(f"forward          {k:16s} {timeit(fn, reps):9.3f}")
        for k in ("ragged", "full"):
            print(f"kernels forward  {k:16s} {kernels(fwd[k])}")

        ag = a.clone().requires_grad_(True)
        cg = c.clone().requires_grad_(True)
        sl = [(ag[i:i + 1, :l1h[i]], cg[i:i + 1, :l2h[i]]) for i in range(B)]

        def step_ragged():
            loss, _ = glue.chamfer_per_sample(ag, cg, lengths1=l1, lengths2=l2)
            loss.sum().backward()

        def step_full():
            loss, _ = glue.chamfer_per_sample(ag, cg)
            loss.sum().backward()

        def step_loop():
            tot = 0
            for x, y in sl:
                loss, _ = glue.chamfer_per_sample(x, y)
                tot = tot + loss.sum()
            tot.backward()

        for k, fn in (("ragged", step_ragged), ("full", step_full), ("loop", step_loop)):
            print(f"forward+backward {k:16s} {timeit(fn, max(reps // 2, 3)):9.3f}")
        for k, fn in (("ragged", step_ragged), ("full", step_full)):
            print(f"kernels step     {k:16s} {kernels(fn)}")


if __name__ == "__main__":
    main()
