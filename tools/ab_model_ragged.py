"""RFNet over a ragged batch on one GPU, one process: B = 32 partial clouds padded to N = 3000, counts uniform in [750, 3000]
(fixed seed), gt 32 x 16384.  The same seeded weights and inputs timed three ways, forward alone and forward + training_loss +
backward (ms, hipEvents via torch):
  ragged   net(pointcloud, lengths=counts)                                   -- counts on the device
  dense    net(pointcloud) on the same padded tensor (zeros behind the counts): what the call costs without counts, wrong
           results aside -- the figure the parent commit's forward gives
  loop     the per-sample loop a caller writes without counts: net(pointcloud[i:i+1, :counts[i]]) for every sample
The versions alternate inside every round (shared machine: a drift hits all of them); median of the rounds [min .. max].
Then the library's per-kernel device times (rf_profile_collect) of the poolings and merge_layer with FULL counts against their
dense entries, at the shapes the network calls them with.  Every timed step runs under a time limit of its own: a watchdog ends
the process when a step overruns (nothing else is started on the device after that).
python tools/ab_model_ragged.py [rounds] > profiles/model_ragged_ab.txt"""
import faulthandler
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402
from rfnet_amd.rfnet import RFNet, training_loss  # noqa: E402

B, N, NGT = 32, 3000, 16384
LO, HI = 750, 3000
STEP_LIMIT_S = 120  # one timed step (the loop leg is 32 forwards + backwards); a healthy one takes well under a second


def limited(fn, what):
    """fn() under the step's own time limit: on overrun the watchdog thread dumps the stacks and exits the process."""
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        return fn()
    except Exception:
        print(f"# step failed: {what}", flush=True)
        raise
    finally:
        faulthandler.cancel_dump_traceback_later()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(legs, rounds, warm=2):
    """{name: fn} -> {name: (median, min, max)} ms per call, the legs taken in turn inside every round."""
    for name, fn in legs.items():
        for _ in range(warm):
            limited(fn, name + " (warm-up)")
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(limited(lambda: timed(fn), name))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def show(title, res):
    print(f"\n## {title}")
    for name, (med, lo, hi) in res.items():
        print(f"  {name:7s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]")
    d = res["dense"][0]
    print(f"  ragged / dense {res['ragged'][0] / d:.3f}   loop / ragged {res['loop'][0] / res['ragged'][0]:.2f}")


def kernel_ms(fn, reps=20):
    """Per-launch-name device time of one call of fn (the library's own event brackets), ms."""
    limited(fn, "kernel warm-up")
    torch.cuda.synchronize()
    profile_collect()
    profile_enable(True)
    try:
        for _ in range(reps):
            limited(fn, "kernel times")
        torch.cuda.synchronize()
        prof = profile_collect()
    finally:
        profile_enable(False)
    return {k: v[0] / reps for k, v in sorted(prof.items())}


def kernel_table(counts_full):
    print("\n## kernels at FULL counts against the dense entries (ms per call, library event brackets; two alternated passes)")
    g = torch.Generator(device="cuda").manual_seed(1)
    dec = torch.tensor([0.07], device="cuda")
    raw = torch.rand(B, N, 3, device="cuda", generator=g) - 0.5
    cases = []
    for n, c in ((N, 256), (N + 64, 256), (N + 1024, 256), (N + 16384, 256)):  # the poolings of forward(): raw (+ generated)
        x = torch.randn(B, n, c, device="cuda", generator=g)
        full = torch.full((B,), n, dtype=torch.int32, device="cuda")
        cases.append((f"maxpool_points      {B} x {n} x {c}", lambda x=x: _raw.maxpool_points(x),
                      lambda x=x, full=full: _raw.maxpool_points(x, full)))
        cases.append((f"maxpool_points_idx  {B} x {n} x {c}", lambda x=x: _raw.maxpool_points_idx(x),
                      lambda x=x, full=full: _raw.maxpool_points_idx(x, full)))
    for m in (64, 1024, 16384):  # the three merge layers
        new = torch.rand(B, m, 3, device="cuda", generator=g) - 0.5
        go = torch.randn(B, m, 3, device="cuda", generator=g)
        idx = _raw.merge_layer(raw, new, dec)[1]
        cases.append((f"merge_layer         {B} x {N} x {m}", lambda new=new: _raw.merge_layer(raw, new, dec),
                      lambda new=new: _raw.merge_layer(raw, new, dec, lengths=counts_full)))
        cases.append((f"merge_layer_grad    {B} x {N} x {m}", lambda new=new, idx=idx, go=go: _raw.merge_layer_grad(raw, new, dec, idx, go),
                      lambda new=new, idx=idx, go=go: _raw.merge_layer_grad(raw, new, dec, idx, go, lengths=counts_full)))
    for label, dense, ragged in cases:
        rows = []
        for _ in range(2):
            rows.append((kernel_ms(dense), kernel_ms(ragged)))
        for tag, k in (("dense ", 0), ("counts", 1)):
            tot = [sum(r[k].values()) for r in rows]
            names = {n_: round(statistics.mean(r[k][n_] for r in rows), 4) for n_ in rows[0][k]}
            print(f"  {label}  {tag} total {tot[0]:.4f} / {tot[1]:.4f}   {names}")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    if not torch.cuda.is_available():
        raise SystemExit("ab_model_ragged.py measures on a HIP device: none is visible")
    torch.manual_seed(0)
    net = RFNet().cuda()
    with torch.no_grad():
        for p in net.biases.values():
            p.normal_(0.0, 0.05)
        for i, dn in enumerate(("decline_factor0", "decline_factor1", "decline_factor")):
            getattr(net, dn).fill_(0.05 + 0.03 * i)
    rng = np.random.RandomState(0)
    counts_h = rng.randint(LO, HI + 1, size=B).astype(np.int32)
    cloud = (rng.rand(B, N, 3) - 0.5).astype(np.float32)
    for i, ln in enumerate(counts_h):
        cloud[i, ln:] = 0.0
    cloud = torch.from_numpy(cloud).cuda()
    gt = torch.from_numpy((rng.rand(B, NGT, 3) - 0.5).astype(np.float32)).cuda()
    counts = torch.from_numpy(counts_h).cuda()
    slices = [cloud[i:i + 1, :int(counts_h[i])].contiguous() for i in range(B)]
    print(f"# RFNet ragged A/B on {torch.cuda.get_device_name(0)}: B={B}, N={N}, counts in [{LO}, {HI}] (mean {counts_h.mean():.0f}, "
          f"min {counts_h.min()}, max {counts_h.max()}), {rounds} alternated rounds, median [min .. max]")

    def fwd(x, **kw):
        with torch.no_grad():
            return net(x, **kw)

    show("forward", alternate({"ragged": lambda: fwd(cloud, lengths=counts), "dense": lambda: fwd(cloud),
                               "loop": lambda: [fwd(s) for s in slices]}, rounds))

    def step(x, g, **kw):
        net.zero_grad(set_to_none=True)
        col = {}
        outs = net(x, collect=col, **kw)
        training_loss(net, outs, col, g).backward()

    def loop_step():
        # gradients accumulate over the samples, as one batch's would (each sample's loss is its own batch mean)
        net.zero_grad(set_to_none=True)
        for i, s in enumerate(slices):
            col = {}
            outs = net(s, collect=col)
            training_loss(net, outs, col, gt[i:i + 1]).backward()

    show("forward + training_loss + backward", alternate({"ragged": lambda: step(cloud, gt, lengths=counts),
                                                            "dense": lambda: step(cloud, gt), "loop": loop_step}, rounds))
    kernel_table(torch.full((B,), N, dtype=torch.int32, device="cuda"))


if __name__ == "__main__":
    main()
