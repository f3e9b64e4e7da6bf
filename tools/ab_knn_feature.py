"""k-nearest neighbours in feature space against the best route without the op, on one GPU (ms per call, device events), forward:
  ours        glue.knn_feature (rf_knn_feature: the squared norms, then the MFMA tiles with the lists in registers)
  torch       sq2[:, :, None] + sq1[:, None, :] - 2 bmm(feat2, feat1^T), then torch.topk(k, largest=False): the (b, m, n) matrix
              is written and read before topk starts
Same device, same process, routes alternated round by round (a round is `reps` back-to-back calls between two events, the calls
rotating over two sets of inputs; the figure is the median over the rounds with the spread next to it), then the library's own
per-kernel device times (rf_profile_*) and the main kernel's 2 b n m c FLOP over its time as a fraction of the 157.3 TF fp32
matrix peak.  Before anything is timed the agreement of the routes is reported: the two round differently, so indices may differ
at near-ties; the k-th distances must agree to 1e-3 of the largest or the run ends.
python tools/ab_knn_feature.py [rounds] [output file]      (writes profiles/knn_feature_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402

# (b, n candidates, m queries, c, k)
SHAPES = [(32, 2048, 2048, 64, 20), (32, 2048, 2048, 128, 20), (32, 2048, 2048, 256, 20), (32, 2048, 512, 128, 16),
          (8, 16384, 16384, 32, 16), (1, 2048, 2048, 64, 20)]
PEAK = 157.3e12  # fp32 matrix FLOP per second
OUT = os.path.join(ROOT, "profiles", "knn_feature_ab.txt")


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


def torch_route(k, f1, f2):
    d = (f2 * f2).sum(-1)[:, :, None] + (f1 * f1).sum(-1)[:, None, :] - 2 * torch.bmm(f2, f1.transpose(1, 2))
    val, idx = torch.topk(d, k, dim=-1, largest=False)
    return -val, idx


def one_shape(b, n, m, c, k, rounds):
    say(f"\n## b = {b}, n = {n} candidates, m = {m} queries, c = {c}, k = {k}")
    f1 = [torch.randn(b, n, c, device="cuda") for _ in range(2)]
    f2 = [torch.randn(b, m, c, device="cuda") for _ in range(2)]
    ov, oi = glue.knn_feature(k, f1[0], f2[0])
    tv, ti = torch_route(k, f1[0], f2[0])
    same = float((oi.long() == ti).float().mean())
    err = float((ov[..., -1] - tv[..., -1]).abs().max() / tv.abs().max())
    say(f"  agreement: {same:.5f} of the indices equal, k-th distances within {err:.2e} of the largest")
    if err > 1e-3:
        sys.exit("the routes disagree: not timed")
    del ov, oi, tv, ti
    torch.cuda.empty_cache()
    routes = {"ours": lambda s: glue.knn_feature(k, f1[s], f2[s]), "torch bmm + topk": lambda s: torch_route(k, f1[s], f2[s])}
    res = ab(routes, rounds)
    for name, (med, lo, hi, reps) in res.items():
        say(f"  {name:18s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)")
    say(f"  ratio ours / torch (medians): {res['ours'][0] / res['torch bmm + topk'][0]:.4f}")
    kern = kernels(routes["ours"])
    say(f"  kernels ours (ms per call) {kern}")
    main_ms = kern.get("knn_feature")
    if main_ms:
        flop = 2.0 * b * n * m * c
        say(f"  main kernel: {flop / 1e9:.1f} GFLOP in {main_ms:.4f} ms = {flop / (main_ms * 1e-3) / 1e12:.2f} TF = "
            f"{flop / (main_ms * 1e-3) / PEAK:.1%} of the {PEAK / 1e12:.1f} TF fp32 matrix peak")


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# knn_feature A/B on {torch.cuda.get_device_name(0)}: forward, alternating rounds, ms per call")
    say("# routes: ours = rf_knn_feature ; torch = sq2 + sq1 - 2 bmm, then topk over the (b, m, n) matrix")
    for shape in SHAPES:
        one_shape(*shape, rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
