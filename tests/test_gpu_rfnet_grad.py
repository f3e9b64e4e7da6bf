"""GPU: the parameter gradients of the whole training step (RFNet forward, training_loss, backward) against the
float64 reference of tests/rfnet_grad_ref.py (checked on the CPU by tests/test_rfnet_grad_ref_host.py), variable by
variable, and the gradient of the input cloud.

The discrete choices are frozen: fps32 and the three merge layers' idx2 come from the GPU run (`collect`), as in
test_forward_and_training_loss_match_the_restatement_oracle, and their agreement with the C oracle's own choice on the
same fp32 tensors is asserted; the loss block's choices (FPS of gt, both arg-min sets of every Chamfer, the two match
matrices) are taken with the C oracle on the GPU run's own fp32 tensors.  None of them depends on the backward under test.

The bar is measured, per case, on the reference itself: the same restatement in float32 on the CPU with the same
choices gives err32[name] against the float64 run (ReLU-mask and arg-max flips of fp32 rounding included), and a
variable's bar is 8 x max(err32[name], median err32); the relative L2 error of the whole gradient has 8 x the float32
run's.  The GPU differs from that run in summation order and in exp / tanh: effects of err32's own size.  No bar is wider
than that.  A result that misses it is compared once more, under the same bar, with the one-sided float64 gradient
nearest to it: the reference re-run with those ReLU units of the small layers flipped whose float64 pre-activation lies
within fp32 rounding of zero and whose jump the result shows (rfnet_grad_ref.py, "Kinks").  Case b1_96 needs it: one
unit of refine_layer1/feat_refine1 sits at +1.4e-8, the MI355X's forward has it on the other side, and 52 variables
differ from the reference by up to 3.7 % -- and from the reference with that unit flipped by less than their bars.  Every wiring
error this file exists for is O(1) on some variable (test_mutations_stand_ten_times_above_the_bar).  The table of the
worst 20 variables is printed; with RFNET_GRAD_REF_TABLE=<file> the full tables are appended to that file
(profiles/rfnet_grad_ref.txt holds the measured ones, and what the first run showed)."""
import os
import zlib

import numpy as np
import pytest
import torch

import rfnet_grad_ref as R
from test_rfnet_model import _seeded_net

pytestmark = pytest.mark.gpu
F32 = np.float32

# every chain the model routes through RFNet.pooled: (points pooled over, as a function of the raw cloud's padded size n;
# channels of the chain's last layer).  The gate of RFNet.pooled sends a chain to _PooledChain when points > 2 * channels.
# A restatement by hand of the model's routing, there to assert that the row-sparse backward was (or was not) taken where
# a case is meant to take it: a chain added to or removed from the model needs its line here.
POOLED = (("init_mlp", lambda n: n, 256), ("cell", lambda n: n, 256), ("recover1", lambda n: n, 256),
          ("part_mlp", lambda n: n + 32, 256), ("refine_layer1", lambda n: 64, 128),
          ("cell_1", lambda n: n + 64, 256), ("recover2", lambda n: n + 64, 256), ("refine_layer2", lambda n: 1024, 128),
          ("cell_2", lambda n: n + 1024, 256), ("recover3", lambda n: n + 1024, 256),
          ("refine_layer_final", lambda n: 16384, 128))


def _clouds(sizes, equal=False):
    rng = np.random.RandomState(3)
    clouds = [(rng.rand(n, 3) - 0.5).astype(F32) for n in sizes]
    if equal:
        clouds = [clouds[0]] * len(sizes)
    gt = (rng.rand(1 if equal else len(sizes), 16384, 3) - 0.5).astype(F32)
    return clouds, np.concatenate([gt] * len(sizes)) if equal else gt


# name -> (per-sample sizes, how `lengths` is given (None: a dense batch), both samples equal)
CASES = {
    # every pooling over the raw cloud is past the gate (1100 > 2 * 256): the row-sparse backward runs in all ten of
    # them; refine_layer1 pools the 64 generated points, below its gate of 256 at any input size
    "b1_1100": ((1100,), None, False),
    # init_mlp, cell, recover1, part_mlp, cell_1, recover2 pool densely; 1024 and then 16384 generated points merge onto
    # 96 raw ones: the most contended scatter-add into the input gradient
    "b1_96": ((96,), None, False),
    # 33: one above the 32 FPS samples the graph draws
    "b2_ragged_list": ((300, 33), "list", False),
    "b2_ragged_cuda": ((300, 33), "cuda", False),
    # batch means of identical samples: every parameter gradient is the B = 1 gradient
    "b2_equal": ((300, 300), None, True),
}
_REFERENCES = {}


def _pooled_chain_nodes(root):
    seen, stack, count = set(), [root], 0
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        count += type(fn).__name__ == "_PooledChainBackward"
        stack.extend(f for f, _ in fn.next_functions)
    return count


def _gpu_step(sizes, lengths_kind, equal):
    from rfnet_amd.rfnet import training_loss
    clouds, gt = _clouds(sizes, equal)
    b, n = len(sizes), max(sizes)
    padded = np.full((b, n, 3), np.nan, F32)  # NaN behind every sample's count
    for i, c in enumerate(clouds):
        padded[i, :len(c)] = c
    net = _seeded_net().cuda()
    partial = torch.from_numpy(padded).cuda().requires_grad_(True)
    lengths = None if lengths_kind is None else list(sizes) if lengths_kind == "list" else \
        torch.tensor(sizes, dtype=torch.int32, device="cuda")
    col, terms = {}, {}
    outs = net(partial, collect=col, lengths=lengths)
    loss = training_loss(net, outs, col, torch.from_numpy(gt).cuda(), terms=terms)
    sparse = _pooled_chain_nodes(loss.grad_fn)
    loss.backward()
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy()
    return {"clouds": clouds, "gt": gt, "net": net, "loss": float(loss.detach()), "sparse_chains": sparse,
            "input_grad": host(partial.grad),
            "grads": {R.tf_name(k): None if p.grad is None else host(p.grad).astype(np.float64) for k, p in net.named_parameters()},
            "out": {"points1_pre": host(col["points1"]), "points2_pre": host(col["points2"]), "points3": host(outs[2]),
                    "points_final": host(outs[3])},
            "forward_choices": {k: host(col[k]) for k in ("fps32", "merge1", "merge2", "merge3")},
            "gt_fps": (host(terms["gt_fps64"]), host(terms["gt_fps1024"]))}


def _reference(orc, run):
    """The float64 and float32 reference runs for the choices of this GPU run; shared between GPU runs whose fp32 tensors and
    indices are the same bit for bit (the two ways of giving `lengths`)."""
    key = zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in
                              list(run["clouds"]) + [run["gt"]] + [run["out"][k] for k in sorted(run["out"])]
                              + [run["forward_choices"][k] for k in sorted(run["forward_choices"])]))
    if key not in _REFERENCES:
        choices = dict(run["forward_choices"])
        choices.update(R.loss_choices(orc, run["out"], run["gt"]))
        variables = run["net"].tf_state_dict()
        probe64, probe32 = {}, {}
        r64 = R.run(variables, run["clouds"], run["gt"], choices, probe=probe64)
        r32 = R.run(variables, run["clouds"], run["gt"], choices, dtype=torch.float32, probe=probe32)
        own = R.forward_choices(orc, run["clouds"], run["out"])
        _REFERENCES[key] = (choices, variables, own, r64, r32, R.kink_units(probe64, probe32))
    return _REFERENCES[key]


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_gradients_match_the_float64_reference(orc, case):
    sizes, lengths_kind, equal = CASES[case]
    run = _gpu_step(sizes, lengths_kind, equal)
    n = max(sizes)
    expected_sparse = sum(points(n) > 2 * channels for _, points, channels in POOLED)
    assert run["sparse_chains"] == expected_sparse, (run["sparse_chains"], expected_sparse)
    if case == "b1_1100":  # all but refine_layer1, whose 64 generated points stay below the gate at any input size
        assert run["sparse_chains"] == len(POOLED) - 1
    if case == "b1_96":
        assert run["sparse_chains"] == 4

    choices, variables, own, r64, r32, units = _reference(orc, run)
    # the discrete choices the run took against the C oracle's on the same fp32 tensors
    assert np.array_equal(own["fps32"], run["forward_choices"]["fps32"])
    for k in ("merge1", "merge2", "merge3"):
        agree = float((own[k] == run["forward_choices"][k]).mean())
        assert agree > 0.995, (k, agree)
    assert np.array_equal(run["gt_fps"][0], choices["gt_fps64"]) and np.array_equal(run["gt_fps"][1], choices["gt_fps1024"])

    ref_loss = r64["terms"]["loss"]
    print(f"{case}: loss {run['loss']!r} against {ref_loss!r}")
    assert abs(run["loss"] - ref_loss) <= 2e-4 * abs(ref_loss)

    # which variables have a gradient
    dead = {k for k, g in r64["grads"].items() if g is None or not g.any()}
    assert dead == {k for k in r64["grads"] if R.is_dead(k)} and len(dead) == 6 + 2 + 32
    assert {k for k, g in run["grads"].items() if g is None} == dead
    assert all(np.isfinite(g).all() and g.any() for g in run["grads"].values() if g is not None)

    # the input gradient: exactly zero behind a sample's count, the rest with the parameters under the bar
    for i, size in enumerate(sizes):
        assert not run["input_grad"][i, size:].any(), f"sample {i}: gradient on padded rows"
    got = {k: g.reshape(r64["grads"][k].shape) for k, g in run["grads"].items() if g is not None}
    got["input"] = np.concatenate([run["input_grad"][i, :size].reshape(-1) for i, size in enumerate(sizes)]).astype(np.float64)
    g64 = R.flat_gradient(r64)
    err32, rel32 = R.errors(R.flat_gradient(r32), g64)
    bar, rel_bar = R.bars(err32, rel32)

    def compare(ref, against):
        err, rel = R.errors(got, ref)
        worst = max(err, key=lambda k: err[k] / bar[k])
        noisiest = max(err, key=lambda k: err[k] / max(err32[k], 1e-300))
        head = [f"# {case}: B = {len(sizes)}, raw points {list(sizes)}, lengths {lengths_kind}, {run['sparse_chains']} row-sparse "
                f"chains; against {against}",
                f"# relative L2 of the whole gradient: float32 reference {rel32:.3e}, bar {rel_bar:.3e}, GPU {rel:.3e}",
                f"# median err32 {np.median(list(err32.values())):.3e}; worst GPU error / bar {err[worst] / bar[worst]:.3f} ({worst}); "
                f"largest GPU error / err32 {err[noisiest] / max(err32[noisiest], 1e-300):.2f} ({noisiest})"]
        print("\n".join(head + R.table(err32, bar, err, 20)))
        if os.environ.get("RFNET_GRAD_REF_TABLE"):
            with open(os.environ["RFNET_GRAD_REF_TABLE"], "a") as f:
                f.write("\n".join(head + R.table(err32, bar, err)) + "\n\n")
        return {k: (err[k], bar[k]) for k in err if err[k] > bar[k]}, worst, rel

    outside, worst, rel = compare(g64, "the float64 reference")
    if outside or rel > rel_bar:
        # Not inside the bar.  If units of the small layers sit within fp32 rounding of their kink, the GPU's forward may have
        # put some on the other side than float64 has them: the same bar, against the one-sided float64 gradient nearest to
        # the GPU's -- the reference re-run with those units' masks flipped, exact for the same loss at the same point
        names = lambda us: ", ".join(f"{'/'.join(str(x) for x in k)}:{i}" for k, i in us) or "none"
        chosen, flipped = R.one_sided_reference(variables, run["clouds"], run["gt"], choices, r64, units, got)
        print(f"{case}: {len(outside)} gradients outside their bar against the reference, worst {worst}: {outside.get(worst)}; "
              f"units within fp32 rounding of a kink: {names(units)}; nearest one-sided gradient: flipped {names(chosen)}")
        if chosen:
            assert abs(flipped["terms"]["loss"] - ref_loss) <= 1e-7 * abs(ref_loss)  # the same point: a kink, not another input
            outside, worst, rel = compare(R.flat_gradient(flipped), "the float64 reference with " + names(chosen) + " flipped")
    assert not outside, f"{len(outside)} gradients outside their bar, worst {worst}: {outside[worst]}"
    assert rel <= rel_bar, (rel, rel_bar)
