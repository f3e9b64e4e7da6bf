"""Neighbour subtraction and neighbour aggregation against the routes without them, on one GPU (ms per call, device events):
  ours          glue.neighbor_subtraction / glue.neighbor_aggregation (rf_neighbor_sub, rf_neighbor_aggregate and their _grad entries)
  group_point   this library's group_point + the pos add + the broadcast multiply + sum (for the subtraction: + the broadcast
                subtraction), torch's autograd over them (group_point's gradient is the library's)
  torch gather  the same expressions over value[batch, idx]: advanced indexing, pure torch
each in forward and in forward + backward (the gradients to value, weight and pos; to both feature tensors for the subtraction).
Same device, same process, routes alternated round by round (a round is `reps` back-to-back calls between two events, the calls
rotating over two sets of inputs; the figure is the median over the rounds with the spread next to it), then the library's own
per-kernel device times (rf_profile_*) and, for each op, the bytes it must move at least once over its time against the project's
streaming figure.  Before anything is timed the agreement of the routes is reported as a fraction of the largest entry; a
difference above 1e-3 ends the run.
python tools/ab_vector_attention.py [rounds] [output file]      (writes profiles/vector_attention_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402
from rfnet_amd.tf_ops.grouping.tf_grouping import group_point  # noqa: E402

# (b, n, m, k, c, cw, hub)
SHAPES = [(32, 2048, 2048, 16, 64, 8, False), (32, 2048, 2048, 16, 64, 64, False), (32, 512, 2048, 8, 128, 128, False),
          (8, 16384, 16384, 16, 32, 4, False), (1, 16384, 16384, 16, 64, 8, False), (32, 2048, 2048, 16, 64, 8, True)]
HBM = 6.3e12  # achievable bytes per second (the streaming figure this project measures against)
OUT = os.path.join(ROOT, "profiles", "vector_attention_ab.txt")


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


def report(title, res, ours="ours"):
    say(title)
    for k, (med, lo, hi, reps) in res.items():
        say(f"  {k:24s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)")
    best = min((k for k in res if k != ours), key=lambda k: res[k][0])
    say(f"  ratio {ours} / {best} (medians): {res[ours][0] / res[best][0]:.4f}")
    return res[ours][0]


def agree(what, ours, theirs):
    err = float((ours - theirs).abs().max() / theirs.abs().max().clamp(min=1e-30))
    if err > 1e-3:
        sys.exit(f"{what}: the routes differ by {err:.3e} of the largest entry: not timed")
    return f"{what} {err:.2e}"


def traffic(what, ms, kernel_ms, nbytes):
    t = (kernel_ms if kernel_ms else ms) * 1e-3
    say(f"  bytes of {what}: {nbytes / 2**20:.1f} MiB moved at least once (the floor: {nbytes / HBM * 1e3:.4f} ms at {HBM / 1e12:.1f} TB/s); "
        f"over the {'kernels' if kernel_ms else 'call'}'s {t * 1e3:.4f} ms: {nbytes / t / 1e12:.3f} TB/s = {nbytes / t / HBM:.1%} of it")


def gathered(route, value, idx):
    if route == "group_point":
        return group_point(value, idx)
    return value[torch.arange(value.shape[0], device=value.device)[:, None, None], idx.long()]


def sub_route(route, q, src, idx):
    if route == "ours":
        return glue.neighbor_subtraction(q, src, idx)
    return q[:, :, None, :] - gathered(route, src, idx)


def agg_route(route, value, weight, idx, pos):
    if route == "ours":
        return glue.neighbor_aggregation(value, weight, idx, pos=pos)
    b, m, k, cw = weight.shape
    c = value.shape[2]
    s = (gathered(route, value, idx) + pos).view(b, m, k, c // cw, cw)
    return (s * weight[:, :, :, None, :]).sum(2).view(b, m, c)


ROUTES = ("ours", "group_point", "torch gather")


def one_shape(b, n, m, k, c, cw, hub, rounds):
    rng = np.random.RandomState(n + m + c + cw)
    say(f"\n## b = {b}, n = {n}, m = {m}, k = {k}, c = {c}, cw = {cw}" + (", every idx = 0 (the hub)" if hub else ", random idx"))
    idxs = [torch.zeros(b, m, k, dtype=torch.int32, device="cuda") if hub else
            torch.from_numpy(rng.randint(0, n, (b, m, k)).astype(np.int32)).cuda() for _ in range(2)]
    leaf = lambda *sh: [torch.randn(*sh, device="cuda").requires_grad_() for _ in range(2)]  # noqa: E731
    q, src, val, pos, w = leaf(b, m, c), leaf(b, n, c), leaf(b, n, c), leaf(b, m, k, c), leaf(b, m, k, cw)
    w = [torch.softmax(t.detach(), 2).requires_grad_() for t in w]  # what the attention hands over
    g4, g3 = [torch.randn(b, m, k, c, device="cuda") for _ in range(2)], [torch.randn(b, m, c, device="cuda") for _ in range(2)]
    det = lambda ts: [t.detach() for t in ts]  # noqa: E731
    qd, srcd, vald, posd, wd = det(q), det(src), det(val), det(pos), det(w)

    # ---- agreement, before anything is timed
    notes = []
    outs = {r: sub_route(r, q[0], src[0], idxs[0]) for r in ROUTES}
    grads = {r: torch.autograd.grad(outs[r], (q[0], src[0]), g4[0]) for r in ROUTES}
    for r in ROUTES[1:]:
        notes += [agree(f"sub vs {r}", outs["ours"].detach(), outs[r].detach()), agree("grad_q", grads["ours"][0], grads[r][0]),
                  agree("grad_src", grads["ours"][1], grads[r][1])]
    outs = {r: agg_route(r, val[0], w[0], idxs[0], pos[0]) for r in ROUTES}
    grads = {r: torch.autograd.grad(outs[r], (val[0], w[0], pos[0]), g3[0]) for r in ROUTES}
    for r in ROUTES[1:]:
        notes += [agree(f"aggregation vs {r}", outs["ours"].detach(), outs[r].detach()), agree("grad_value", grads["ours"][0], grads[r][0]),
                  agree("grad_weight", grads["ours"][1], grads[r][1]), agree("grad_pos", grads["ours"][2], grads[r][2])]
    say("  agreement, of the largest entry: " + ", ".join(notes))
    del outs, grads
    torch.cuda.empty_cache()

    # ---- the subtraction
    fwd = {r: (lambda s, r=r: sub_route(r, qd[s], srcd[s], idxs[s])) for r in ROUTES}
    both = {r: (lambda s, r=r: torch.autograd.grad(sub_route(r, q[s], src[s], idxs[s]), (q[s], src[s]), g4[s])) for r in ROUTES}
    ms = report("subtraction forward (ms)", ab(fwd, rounds))
    kern = kernels(fwd["ours"])
    say(f"  kernels ours forward (ms per call) {kern}")
    traffic("rf_neighbor_sub", ms, kern.get("neighbor_sub"), 4 * b * (m * k * c + m * c + n * c + m * k))
    report("subtraction forward + backward (ms)", ab(both, rounds))
    kern = kernels(both["ours"])
    say(f"  kernels ours forward + backward (ms per call) {kern}")
    back = sum(v for k_, v in kern.items() if k_.startswith("neighbor_sub_grad"))
    traffic("rf_neighbor_sub_grad", None, back, 4 * b * (m * k * c + m * c + n * c + 3 * m * k + n))
    torch.cuda.empty_cache()

    # ---- the aggregation
    fwd = {r: (lambda s, r=r: agg_route(r, vald[s], wd[s], idxs[s], posd[s])) for r in ROUTES}
    both = {r: (lambda s, r=r: torch.autograd.grad(agg_route(r, val[s], w[s], idxs[s], pos[s]), (val[s], w[s], pos[s]), g3[s]))
            for r in ROUTES}
    ms = report("aggregation forward (ms)", ab(fwd, rounds))
    kern = kernels(fwd["ours"])
    say(f"  kernels ours forward (ms per call) {kern}")
    traffic("rf_neighbor_aggregate", ms, kern.get("neighbor_agg"), 4 * b * (m * k * c + m * k * cw + m * k + n * c + m * c))
    report("aggregation forward + backward (ms)", ab(both, rounds))
    kern = kernels(both["ours"])
    say(f"  kernels ours forward + backward (ms per call) {kern}")
    back = sum(v for k_, v in kern.items() if k_.startswith("neighbor_agg_grad"))
    traffic("rf_neighbor_aggregate_grad", None, back, 4 * b * (2 * m * k * c + 2 * m * k * cw + 3 * m * k + 2 * n * c + m * c + n))


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# Neighbour subtraction and aggregation A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call")
    say("# routes: ours = rf_neighbor_* ; group_point = the library's group_point + torch broadcasts ; torch gather = advanced indexing")
    for shape in SHAPES:
        one_shape(*shape, rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
