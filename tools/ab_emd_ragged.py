"""Ragged EMD batches on one GPU: the same seeded padded inputs timed four ways (ms per call, hipEvents via torch):
  ragged   one call with per-sample lengths (rf_approxmatch_lengths + rf_matchcost_lengths, rf_earth_mover_lengths),
  auto     the existing call on the same padded tensors at full size, AUTO route (what a caller pays today, wrong results aside),
  swept    the same with the route pinned (RF_EMD_SWEPT: the route the ragged call always takes),
  loop     a Python loop of existing per-sample calls on the unpadded slices (AUTO route).
Three ops: approx_match + match_cost, earth_mover (cost alone) and earth_mover with gradients; then the library's
per-kernel device times of the ragged and full calls.  Lengths are device tensors.
python tools/ab_emd_ragged.py [reps]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

# (label, B, n = m, both counts' range, ops); the 16384^2 shape is fused only (match would be 4 GiB)
ALL = ("match", "emd", "emd_grad")
SHAPES = [
    ("2048 x 2048, both in [512, 2048]", 32, 2048, (512, 2048), ALL),
    ("2048 x 2048, both in [1536, 2048]", 32, 2048, (1536, 2048), ALL),
    ("2048 x 2048, all full", 32, 2048, (2048, 2048), ALL),
    ("256 x 256, both in [16, 256]", 32, 256, (16, 256), ALL),
    ("16384 x 16384, both in [4096, 16384]", 4, 16384, (4096, 16384), ("emd", "emd_grad")),
]


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=5):
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


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.cuda.init()
    print(f"# ragged EMD A/B on {torch.cuda.get_device_name(0)}, {reps} reps per figure, ms per call")
    for label, b, n, (lo, hi), ops in SHAPES:
        rng = np.random.RandomState(n + b)
        a = torch.from_numpy((rng.random_sample((b, n, 3)) - 0.5).astype(np.float32)).cuda()
        c = torch.from_numpy((rng.random_sample((b, n, 3)) - 0.5).astype(np.float32)).cuda()
        l1h = rng.randint(lo, hi + 1, size=b).astype(np.int32)
        l2h = rng.randint(lo, hi + 1, size=b).astype(np.int32)
        l1, l2 = torch.from_numpy(l1h).cuda(), torch.from_numpy(l2h).cuda()
        slices = [(a[i:i + 1, :l1h[i]].contiguous(), c[i:i + 1, :l2h[i]].contiguous()) for i in range(b)]
        print(f"\n## B = {b}, {label}  (mean len1 {l1h.mean():.0f}, mean len2 {l2h.mean():.0f})")
        rounds = max(2, reps // (4 if n >= 16384 else 1))
        for op in ops:
            if op == "match":
                def run(x, y, mode="auto", lengths1=None, lengths2=None):
                    mt = _raw.approx_match(x, y, mode=mode, lengths1=lengths1, lengths2=lengths2)
                    return _raw.match_cost(x, y, mt, lengths1=lengths1, lengths2=lengths2)
            else:
                grad = op == "emd_grad"

                def run(x, y, grad=grad, **kw):
                    return _raw.earth_mover(x, y, with_grad=grad, **kw)
            fns = {
                "ragged": lambda: run(a, c, lengths1=l1, lengths2=l2),
                "auto": lambda: run(a, c),
                "swept": lambda: run(a, c, mode="swept"),
                "loop": lambda: [run(x, y) for x, y in slices],
            }
            t = {k: timeit(fn, rounds) for k, fn in fns.items()}
            name = {"match": "approx_match+match_cost", "emd": "earth_mover", "emd_grad": "earth_mover+grad"}[op]
            print(f"{name:24s} " + "  ".join(f"{k} {v:8.3f}" for k, v in t.items())
                  + f"   ragged/loop {t['ragged'] / t['loop']:.3f}  ragged/swept {t['ragged'] / t['swept']:.3f}"
                  + f"  ragged/auto {t['ragged'] / t['auto']:.3f}")
            for k in ("ragged", "auto", "swept"):
                print(f"  kernels {k:7s} {kernels(fns[k], 3 if n >= 16384 else 5)}")


if __name__ == "__main__":
    main()
