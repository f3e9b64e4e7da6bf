"""What the metrics epilogue costs on top of the Chamfer sweep, on one GPU (ms per call, device events):
  loss     rf_chamfer_loss_lengths with NULL counts: the sweep + the sqrt-mean reduce (existing code, the baseline),
  metrics  rf_chamfer_metrics on the same inputs: the same sweep + histogram, counts and eleven columns,
both straight through the C ABI on caller-owned buffers, alternated round by round in one process (each round is `reps`
back-to-back calls between two events; the figure is the median over the rounds, with the spread next to it), then the
library's own per-kernel device times of either call (rf_profile_*: the epilogue kernel alone is
`chamfer_metrics_epilogue`, the reduce it replaces `chamfer_loss_reduce_len`).  Inputs are seeded; the two calls' dist / idx
are compared bit for bit before anything is timed, and a difference ends the run with an error.
python tools/ab_metrics.py [rounds] [reps]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd._lib import check, lib, profile_collect, profile_enable  # noqa: E402

SHAPES = [(32, 16384, 16384), (32, 2048, 16384)]
TAU, ALPHA = 0.01, 1000.0


def buffers(b, n, m, seed):
    rng = np.random.RandomState(seed)
    dev = "cuda"
    t = dict(a=torch.from_numpy((rng.rand(b, n, 3) - 0.5).astype(np.float32)).to(dev),
             c=torch.from_numpy((rng.rand(b, m, 3) - 0.5).astype(np.float32)).to(dev))
    for tag in ("loss", "met"):
        t[tag] = dict(d1=torch.empty(b, n, device=dev), i1=torch.empty(b, n, dtype=torch.int32, device=dev),
                      d2=torch.empty(b, m, device=dev), i2=torch.empty(b, m, dtype=torch.int32, device=dev))
    t["lossv"] = torch.empty(b, 2, device=dev)
    t["metv"] = torch.empty(b, 11, device=dev)
    t["c1"], t["c2"] = torch.empty(b, n, dtype=torch.int32, device=dev), torch.empty(b, m, dtype=torch.int32, device=dev)
    t["ws_loss"] = torch.empty(lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, 1, 1), dtype=torch.uint8, device=dev)
    t["ws_met"] = torch.empty(lib.rf_chamfer_metrics_workspace_bytes(b, n, m), dtype=torch.uint8, device=dev)
    return t


def calls(b, n, m, t):
    p = lambda x: x.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    o, q = t["loss"], t["met"]
    thr2 = float(np.float32(TAU) * np.float32(TAU))

    def loss():
        check(lib.rf_chamfer_loss_lengths(b, n, m, p(t["a"]), p(t["c"]), None, None, p(t["lossv"]), p(o["d1"]), p(o["i1"]),
                                          p(o["d2"]), p(o["i2"]), p(t["ws_loss"]), t["ws_loss"].numel(), s), "rf_chamfer_loss_lengths")

    def metrics():
        check(lib.rf_chamfer_metrics(b, n, m, p(t["a"]), p(t["c"]), None, None, thr2, ALPHA, p(t["metv"]), p(q["d1"]), p(q["i1"]),
                                     p(q["d2"]), p(q["i2"]), p(t["c1"]), p(t["c2"]), p(t["ws_met"]), t["ws_met"].numel(), s),
              "rf_chamfer_metrics")

    return loss, metrics


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=20):
    profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000  # ~0.3 s per window
    torch.cuda.init()
    print(f"# metrics epilogue A/B on {torch.cuda.get_device_name(0)}: {rounds} alternating rounds of {reps} calls, ms per call")
    for b, n, m in SHAPES:
        t = buffers(b, n, m, n + m)
        loss, metrics = calls(b, n, m, t)
        for _ in range(10):  # warm-up of both, and the check that they are the same sweep
            loss()
            metrics()
        torch.cuda.synchronize()
        same = all(torch.equal(t["loss"][k], t["met"][k]) for k in ("d1", "i1", "d2", "i2"))
        cd = torch.allclose(t["lossv"], t["metv"][:, 0:2], rtol=1e-5, atol=0)
        if not (same and cd):
            sys.exit(f"{b} x {n} x {m}: the two calls disagree (dist/idx identical: {same}, CD halves equal: {cd}): not timed")
        times = {"loss": [], "metrics": []}
        for _ in range(rounds):
            times["loss"].append(window(loss, reps))
            times["metrics"].append(window(metrics, reps))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"\n## {b} x {n} x {m}   dist/idx identical: {same}; columns 0, 1 equal the loss within 1e-5: {cd}")
        for k, v in times.items():
            print(f"{k:8s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
        print(f"ratio metrics / loss (medians): {med['metrics'] / med['loss']:.4f}   added per call: "
              f"{(med['metrics'] - med['loss']) * 1e3:.1f} us")
        print(f"bytes the epilogue needs (dist + idx read, count written, 4 B each): {12 * b * (n + m) / 1e6:.2f} MB")
        print("kernels loss    ", kernels(loss))
        print("kernels metrics ", kernels(metrics))


if __name__ == "__main__":
    main()
