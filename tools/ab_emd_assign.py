"""The exact EMD (glue.emd_assignment: rf_emd_assign, a deterministic integer auction with a certificate) on one GPU, ms per
call from device events, next to what existed before it on the same inputs:
  exact      glue.emd_assignment forward, and forward + gradients (cost.sum().backward()),
  auction    _raw.auction_match: the port of the reference's sequential auction, until now the only device route to an
             assignment (no distances, no gradient, no bound),
  scipy      scipy.optimize.linear_sum_assignment on ONE sample's float64 distance matrix, on the CPU (wall clock),
and the figures the auction reports per sample (rounds, bids, the certified gap), and earth_mover's cost over the exact
cost: how far approx_match's ten-level annealing is from the optimum.  Shapes 32 x 1024 and 32 x 2048; inputs: uniform
clouds, and xyz2 = a permutation of xyz1 + 0.01 randn.  The figures are the median, min and max over `reps` calls after
one warm-up call.
python tools/ab_emd_assign.py [reps]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw, glue  # noqa: E402

SHAPES = [(32, 1024), (32, 2048)]


def inputs(kind, b, n, seed):
    rng = np.random.RandomState(seed)
    a = rng.rand(b, n, 3)
    if kind == "uniform":
        c = rng.rand(b, n, 3)
    else:
        c = np.stack([a[i, rng.permutation(n)] for i in range(b)]) + 0.01 * rng.randn(b, n, 3)
    return torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(c.astype(np.float32)).cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return f"median {np.median(ms):9.3f}  min {min(ms):9.3f}  max {max(ms):9.3f}", float(np.median(ms))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    print(f"# exact EMD A/B on {torch.cuda.get_device_name(0)}: ms per call, {reps} calls after one warm-up")
    for b, n in SHAPES:
        for kind in ("uniform", "noisy permuted copy"):
            A, B = inputs(kind, b, n, n + len(kind))
            print(f"\n## b = {b}, n = {n}, {kind}")

            def fwd():
                return glue.emd_assignment(A, B)

            def fwd_bwd():
                x, y = A.clone().requires_grad_(), B.clone().requires_grad_()
                glue.emd_assignment(x, y)["cost"].sum().backward()

            line, t_new = timed(fwd, reps)
            print(f"exact forward              {line}")
            print(f"exact forward + gradients  {timed(fwd_bwd, reps)[0]}")
            line, t_old = timed(lambda: _raw.auction_match(A, B), max(2, reps // 2))
            verdict = "the new op is SLOWER than auction_match here" if t_new > t_old else "the new op is faster than auction_match here"
            print(f"auction_match              {line}   exact / auction_match = {t_new / t_old:.3f}: {verdict}")
            d = (A[0].double()[:, None] - B[0].double()[None]).norm(dim=-1).cpu().numpy()
            from scipy.optimize import linear_sum_assignment
            t0 = time.perf_counter()
            rows, cols = linear_sum_assignment(d)
            t_cpu = (time.perf_counter() - t0) * 1e3
            out = fwd()
            torch.cuda.synchronize()
            cost, info = out["cost"].double().cpu().numpy(), out["info"].cpu().numpy()
            print(f"scipy linear_sum_assignment, ONE sample on the CPU: {t_cpu:.1f} ms; its optimum {d[rows, cols].sum():.6f}, "
                  f"exact cost of that sample {cost[0]:.6f}, certified bound {float(out['bound'][0]):.3e}")
            for name, col in (("rounds", 1), ("bids", 2)):
                v = info[:, col]
                print(f"{name:6s} per sample: min {v.min()}  median {int(np.median(v))}  max {v.max()}   ({np.median(v) / n:.2f} n)")
            print(f"status: {np.bincount(info[:, 0], minlength=3).tolist()} samples ok / capped / non-finite; "
                  f"gap (P - D) / S: max {float(out['gap'].max()):.3e}; bound / cost: max {float((out['bound'] / out['cost']).max()):.3e}")
            approx = _raw.earth_mover(A, B)
            approx = (approx[0] if isinstance(approx, (tuple, list)) else approx).double().cpu().numpy()
            ratio = approx / cost
            print(f"earth_mover cost / exact cost: min {ratio.min():.4f}  median {np.median(ratio):.4f}  max {ratio.max():.4f}")


if __name__ == "__main__":
    main()
