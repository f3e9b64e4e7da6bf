"""The expansion penalty and minimum density sampling, on one GPU (ms per forward + backward, device events):
  ours   glue.expansion_loss(x, S, alpha).backward()  -- rf_expansion_penalty + rf_expansion_penalty_grad, two launches;
         gather_point(x, glue.minimum_density_sample(x, m, sigma)).sum().backward()  -- rf_mds + gather + its scatter,
  torch  the best routes without the ops: Prim's algorithm batched over all patches on a dense (b P, S, S) matrix of squared
         distances (S - 1 dependent steps of a masked arg-min, a row gather and two selects), the lengths, the mean and the
         indicator with torch ops and autograd for the backward; the MDS loop with torch.exp (m - 1 dependent steps: a
         row gather, the squared distances, exp, add, a scatter and an arg-min), indexing and autograd for the gather
-- same device, same process, alternated round by round (each round is `reps` back-to-back steps between two events; the
figure is the median over the rounds, with the spread next to it), then the library's own per-kernel device times
(rf_profile_*).  Inputs are seeded uniform-cube clouds (no ties, so both Prims build the same tree).  Before anything is timed
the two penalties must agree (loss to 1e-4, gradient rows to 1e-5 of the largest entry; a difference ends the run).  The two
samplers are NOT the same function: the library's prescribed weight is exactly 0 from d^2 c = 64 on (below 2^-64) and a
polynomial within 2.6e-7 of exp2 before, so among points that far from every chosen one it takes the lowest index where
torch.exp still ranks 1e-38 against 1e-31 -- the choices part early.  The tool checks that both return distinct indices and
reports where they part; the work per step is the same.
python tools/ab_msn_ops.py [rounds]      (writes profiles/msn_ops_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402
from rfnet_amd.tf_ops.sampling.tf_sampling import gather_point  # noqa: E402

PENALTY = [(32, 16, 512, 1.5), (32, 2, 4096, 1.5)]  # b, patches, points per patch, alpha
MDS = [(32, 13192, 8192, 0.02), (32, 2048, 512, 0.05)]  # b, n, m, sigma
OUT = os.path.join(ROOT, "profiles", "msn_ops_ab.txt")


def say(s=""):
    """to the terminal and, line by line, to the profile: a run that ends early leaves what it measured"""
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def torch_penalty(x, S, alpha):
    """-> (loss, grad): Prim on the dense matrix, batched over the b P patches"""
    b, n, _ = x.shape
    X = x.reshape(-1, S, 3).clone().requires_grad_()
    Q = X.shape[0]
    ar = torch.arange(Q, device=x.device)
    with torch.no_grad():
        D = torch.zeros(Q, S, S, device=x.device)
        for a in range(3):
            d = X[:, :, None, a] - X[:, None, :, a]
            D += d * d
        key = D[:, 0].clone()
        father = torch.zeros(Q, S, dtype=torch.long, device=x.device)
        intree = torch.zeros(Q, S, dtype=torch.bool, device=x.device)
        intree[:, 0] = True
        for _ in range(S - 1):
            u = key.masked_fill(intree, float("inf")).argmin(1)
            intree[ar, u] = True
            d = D[ar, u]
            upd = ~intree & (d < key)
            key = torch.where(upd, d, key)
            father = torch.where(upd, u[:, None], father)
        del D
    length = (X - X.gather(1, father[:, :, None].expand(-1, -1, 3))).norm(dim=2)
    mean = length.detach()[:, 1:].mean(1, keepdim=True)
    loss = torch.where(length > alpha * mean, length, torch.zeros_like(length)).mean()
    loss.backward()
    return loss.detach(), X.grad.reshape(b, n, 3)


def our_penalty(x, S, alpha):
    X = x.clone().requires_grad_()
    loss = glue.expansion_loss(X, S, alpha)
    loss.backward()
    return loss.detach(), X.grad


def torch_mds(x, m, sigma):
    """-> (idx (b, m), grad of the gathered rows' sum)"""
    b, n, _ = x.shape
    X = x.clone().requires_grad_()
    ar = torch.arange(b, device=x.device)
    with torch.no_grad():
        dens = torch.zeros(b, n, device=x.device)
        idx = torch.zeros(b, m, dtype=torch.long, device=x.device)
        u = torch.zeros(b, dtype=torch.long, device=x.device)
        scale = -1.0 / (2.0 * sigma * sigma)
        for j in range(1, m):
            d = X - X[ar, u][:, None, :]
            dens += torch.exp((d * d).sum(2) * scale)
            dens[ar, u] = float("inf")
            u = dens.argmin(1)
            idx[:, j] = u
    X[ar[:, None], idx].sum().backward()
    return idx, X.grad


def our_mds(x, m, sigma):
    X = x.clone().requires_grad_()
    idx = glue.minimum_density_sample(X, m, sigma)
    gather_point(X, idx).sum().backward()
    return idx, X.grad


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


def alternate(ours, theirs, rounds):
    ours(), theirs()  # every shape warm
    torch.cuda.synchronize()
    once = {"ours": window(ours, 1), "torch": window(theirs, 1)}
    reps = {k: max(1, min(50, int(np.ceil(200.0 / rounds / v)))) for k, v in once.items()}
    times = {"ours": [], "torch": []}
    for _ in range(rounds):
        times["ours"].append(window(ours, reps["ours"]))
        times["torch"].append(window(theirs, reps["torch"]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        say(f"{k:6s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}   ({rounds} rounds of {reps[k]} steps)")
    say(f"ratio ours / torch (medians): {med['ours'] / med['torch']:.5f}")
    say(f"kernels ours (ms per call) {kernels(ours)}")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# expansion penalty and minimum density sampling A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per "
        f"forward + backward, uniform-cube clouds")
    for b, P, S, alpha in PENALTY:
        x = torch.from_numpy(np.random.RandomState(S).rand(b, P * S, 3).astype(np.float32)).cuda()
        (lo, go), (lt, gt) = our_penalty(x, S, alpha), torch_penalty(x, S, alpha)
        # an edge within a rounding of the bar may be penalised by one route and not by the other (the mean is a double sum here,
        # an fp32 reduction there): up to two such edges (four rows) are reported, more end the run
        dl = abs(float(lo) - float(lt))
        off = int(((go - gt).abs().amax(2) > 1e-5 * float(gt.abs().max())).sum())
        if not (dl <= 1e-4 * abs(float(lt)) and off <= 4):
            sys.exit(f"penalty {b} x {P} x {S}: the losses differ by {dl:.3e}, {off} gradient rows differ: not timed")
        say(f"\n## penalty b = {b}, {P} patches of {S} points, alpha {alpha}: loss {float(lo):.6e}, |difference| {dl:.2e}; "
            f"gradient rows more than 1e-5 of the largest entry apart: {off}; {int((go != 0).any(2).sum())} of {b * P * S} rows "
            f"with a gradient")
        alternate(lambda: our_penalty(x, S, alpha), lambda: torch_penalty(x, S, alpha), rounds)
        del x
        torch.cuda.empty_cache()
    for b, n, m, sigma in MDS:
        x = torch.from_numpy(np.random.RandomState(n).rand(b, n, 3).astype(np.float32)).cuda()
        (io, go), (it, gt) = our_mds(x, m, sigma), torch_mds(x, m, sigma)
        io, it = io.cpu().numpy(), it.cpu().numpy()
        for name, ix in (("ours", io), ("torch", it)):
            if any(len(set(row.tolist())) != m for row in ix):
                sys.exit(f"MDS {b} x {n} -> {m}: {name} returned an index twice: not timed")
        first = [int(np.flatnonzero(np.r_[io[i] != it[i], True])[0]) for i in range(b)]
        say(f"\n## MDS b = {b}, {n} -> {m}, sigma {sigma}: both return distinct indices; samples with all {m} choices equal: "
            f"{sum(f == m for f in first)} of {b}; the earliest choice that differs: {min(first)} (the weights differ by design: a cutoff at 2^-64)")
        alternate(lambda: our_mds(x, m, sigma), lambda: torch_mds(x, m, sigma), rounds)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
