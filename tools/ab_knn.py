#!/usr/bin/env python3
"""knn_point on one MI355X: the scan kernel (rf_knn), the boxed kernel with its own sort and on caller sort handles
(rf_knn_boxes), and the tensor expression it replaces (tf_grouping.py:64-73: the (b, m, n, 3) difference, sum, topk) -- same
process, same seeded inputs, alternated, device events after warm-up; torch.cuda.max_memory_allocated per path; the boxed
kernel's evaluated-pair fraction with --stats (a build with -DTB_STATS: knn_boxes_kernel then writes its 16-record block scans
per wave into idx[..., 0]; python tools/build_variant.py tbstats -DTB_STATS, RFOPS_LIB=rfnet_amd/variants/librfops_tbstats.so).
usage: python tools/ab_knn.py [--reps R] [--stats] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rfnet_amd import _raw as R  # noqa: E402

# (name, b, n, m, k): PointNet++ grouping, DGCNN-style self-kNN, a large batch of large clouds, one large sample
SHAPES = [
    ("pn2_k16", 32, 16384, 1024, 16), ("pn2_k32", 32, 16384, 1024, 32), ("pn2_k64", 32, 16384, 1024, 64),
    ("dgcnn_k20", 32, 2048, 2048, 20), ("b8_16k_k16", 8, 16384, 16384, 16), ("one_64k_k32", 1, 65536, 4096, 32),
    # around and below 1e8 pairs (where the form is chosen): small batches of the same workloads, and small clouds
    ("pn2_b8_k16", 8, 16384, 1024, 16), ("pn2_b8_k64", 8, 16384, 1024, 64), ("pn2_b4_k16", 4, 16384, 1024, 16),
    ("pn2_b4_k64", 4, 16384, 1024, 64), ("pn2_b1_k16", 1, 16384, 1024, 16), ("pn2_b1_k64", 1, 16384, 1024, 64),
    ("dgcnn_b16_k20", 16, 2048, 2048, 20), ("dgcnn_b8_k20", 8, 2048, 2048, 20), ("dgcnn_b1_k20", 1, 2048, 2048, 20),
    ("b4_4k_1k_k32", 4, 4096, 1024, 32), ("b1_1k_256_k16", 1, 1024, 256, 16), ("b8_512_512_k16", 8, 512, 512, 16),
    # where the boxed form can pay: many queries per sample
    ("b1_16k_k16", 1, 16384, 16384, 16), ("b4_16k_k16", 4, 16384, 16384, 16), ("b4_16k_k64", 4, 16384, 16384, 64),
    ("b8_16k_8k_k16", 8, 16384, 8192, 16), ("b2_64k_16k_k32", 2, 65536, 16384, 32), ("pn2_b64_k16", 64, 16384, 1024, 16),
]


def torch_expr(k, xyz1, xyz2):
    dist = ((xyz1.unsqueeze(1) - xyz2.unsqueeze(2)) ** 2).sum(-1)
    val, idx = torch.topk(-dist, k=int(k), dim=-1)
    return val, idx.to(torch.int32)


def timed(fn, reps):
    """-> (median ms over reps, peak bytes above what was allocated before)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
        del out
    ts.sort()
    return ts[len(ts) // 2], torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = []
    shapes = [s for s in SHAPES if not a.shapes or s[0] in a.shapes.split(",")]
    for name, b, n, m, k in shapes:
        g = torch.Generator(device=dev).manual_seed(b * 7 + n + m + k)
        x1 = torch.rand(b, n, 3, device=dev, generator=g)
        x2 = torch.rand(b, m, 3, device=dev, generator=g)
        if a.stats:
            _, idx = R.knn_point(k, x1, x2, form="boxes")
            # idx[..., 0] of every query = the block scans of its wave; a wave holds 64 queries and scans 16 records per block
            blocks = idx[..., 0].double().sum().item() / 64.0  # (each wave's count appears on its up to 64 queries)
            frac = blocks * 16 * 64 / (b * n * m)
            rec = {"shape": name, "b": b, "n": n, "m": m, "k": k, "evaluated_pair_fraction": round(frac, 5)}
        else:
            h1, h2 = R.nn_sort(x1), R.nn_sort(x2)
            paths = {
                "scan": lambda: R.knn_point(k, x1, x2, form="scan"),
                "boxes": lambda: R.knn_point(k, x1, x2, form="boxes"),
                "boxes_handles": lambda: R.knn_point(k, x1, x2, form="boxes", sorted1=h1.buf, sorted2=h2.buf),
                "auto": lambda: R.knn_point(k, x1, x2),
                "torch": lambda: torch_expr(k, x1, x2),
            }
            sv, si = paths["scan"]()
            for p in ("boxes", "boxes_handles", "auto"):
                v, i = paths[p]()
                assert torch.equal(i, si) and torch.equal(v.view(torch.int32), sv.view(torch.int32)), (name, p)
            tv, ti = paths["torch"]()
            same_sets = bool(torch.equal(torch.sort(ti, -1).values, torch.sort(si, -1).values))
            max_val_diff = float((tv - sv).abs().max())
            del tv, ti, v, i, sv, si
            for fn in paths.values():  # warm-up
                fn()
            ms = {p: [] for p in paths}
            mem = {}
            for r in range(a.reps):  # alternated: one call of every path per round
                for p, fn in paths.items():
                    t, pk = timed(fn, 1)
                    ms[p].append(t)
                    mem[p] = max(mem.get(p, 0), pk)
            med = {p: sorted(v)[len(v) // 2] for p, v in ms.items()}
            rec = {"shape": name, "b": b, "n": n, "m": m, "k": k, "pairs": b * n * m,
                   "ms": {p: round(v, 4) for p, v in med.items()},
                   "ms_min": {p: round(min(v), 4) for p, v in ms.items()},
                   "peak_mib": {p: round(v / 2**20, 1) for p, v in mem.items()},
                   "torch_same_sets": same_sets, "torch_max_val_diff": max_val_diff,
                   "auto_form": "boxes" if R.knn_auto_boxes(k, n, m) else "scan"}
            del h1, h2
        torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
