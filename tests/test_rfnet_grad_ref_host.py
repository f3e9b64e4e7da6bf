"""CPU: the training step's gradient reference (tests/rfnet_grad_ref.py) checked against things that are not the
product, before tests/test_gpu_rfnet_grad.py rests on it: its forward and every loss term against the float64
restatement oracle (oracle/rfnet_oracle.py) on the oracle's own discrete choices; its gradient against central
differences of its own float64 loss; the inventory of variables without a gradient; both zero_groupnear hinges, active
and clamped; and that each deliberate error (`mutate=`) stands far above the bar the GPU test uses.

One oracle run per case, shared through module-scoped fixtures (the oracle's loss block is serial C at 16384^2); the
C operators are memoised, so the choices the reference is handed cost no second sweep."""
import numpy as np
import pytest
import torch

import rfnet_grad_ref as R
from test_rfnet_model import _seeded_net

F32 = np.float32


class _Memo:
    """The C operator oracle with results remembered per (operator, arguments)."""

    def __init__(self, orc):
        self._orc, self._seen = orc, {}

    def __getattr__(self, name):
        fn = getattr(self._orc, name)

        def call(*args):
            key = (name,) + tuple((a.shape, a.dtype.str, hash(a.tobytes())) if isinstance(a, np.ndarray) else a for a in args)
            if key not in self._seen:
                self._seen[key] = fn(*args)
            return self._seen[key]
        return call


def _inputs(npts):
    rng = np.random.RandomState(3)  # the seed-3 inputs of test_forward_and_training_loss_match_the_restatement_oracle
    return (rng.rand(1, npts, 3) - 0.5).astype(F32), (rng.rand(1, 16384, 3) - 0.5).astype(F32)


@pytest.fixture(scope="module")
def morc(orc):
    return _Memo(orc)


@pytest.fixture(scope="module")
def variables():
    return _seeded_net().tf_state_dict()


def _case(variables, morc, npts, full_oracle_loss):
    from oracle.rfnet_oracle import RFNetOracle
    partial, gt = _inputs(npts)
    o = RFNetOracle(variables, morc)
    out = o.forward(partial)
    case = {"partial": partial, "gt": gt, "oracle": o, "oracle_out": out, "variables": variables}
    case["choices"] = R.forward_choices(morc, partial, out)
    case["choices"].update(R.loss_choices(morc, out, gt))  # (first: its sweeps run side by side and fill the memo)
    if full_oracle_loss:
        case["oracle_terms"] = o.training_loss(out, gt)
    probe64, probe32 = {}, {}
    case["r64"] = R.run(variables, partial, gt, case["choices"], probe=probe64)
    case["r32"] = R.run(variables, partial, gt, case["choices"], dtype=torch.float32, probe=probe32)
    g64 = R.flat_gradient(case["r64"])
    case["g64"] = g64
    case["err32"], case["rel32"] = R.errors(R.flat_gradient(case["r32"]), g64)
    case["units"] = R.kink_units(probe64, probe32)
    case["jumps"] = R.kink_jumps(variables, partial, gt, case["choices"], case["r64"], case["units"])
    case["bar"], case["rel_bar"] = R.bars(case["err32"], case["rel32"])  # the GPU test's bar
    return case


@pytest.fixture(scope="module")
def case96(variables, morc):
    return _case(variables, morc, 96, True)


MOVE_SCALE = 0.1
MOVE_LAYERS = ("decode_cell/points_out/weights", "decode_cell/points_out/Variable", "decode_cell_1/points_out/Variable")


@pytest.fixture(scope="module")
def clamped(variables, morc):
    """decode_cell's move layer (points_out: kernel and both applications' biases) scaled by MOVE_SCALE: the generated
    points move so little around their centres that mean |move|^2 falls below 0.4 mean dist2 in both zero_groupnear."""
    v = dict(variables)
    for k in MOVE_LAYERS:
        v[k] = (v[k] * F32(MOVE_SCALE)).astype(F32)
    return _case(v, morc, 96, False)


# ---- forward and loss terms against the oracle ---------------------------------------------------------------------------
def test_forward_equals_the_oracle(case96):
    for k in R.OUTPUTS:
        exp, got = case96["oracle_out"][k], case96["r64"]["out"][k]
        assert got.shape == exp.shape, k
        err = np.abs(got - exp).max() / np.abs(exp).max()
        print(f"{k}: max error / max = {err:.2e}")
        assert err <= 1e-10, (k, err)


def test_loss_terms_equal_the_oracle(case96):
    """The oracle takes its Chamfer and EMD values from the fp32 C operators; here they are recomputed in float64 from
    the same indices and match matrices: rel 1e-6 is that fp32 rounding (means of thousands of fp32 values)."""
    for k in R.TERMS:
        got, exp = case96["r64"]["terms"][k], float(case96["oracle_terms"][k])
        print(f"{k}: {got!r} vs {exp!r}")
        assert abs(got - exp) <= 1e-6 * abs(exp), (k, got, exp)


def test_earth_mover_distance_is_match_costs(orc):
    """earth_mover here against orc.match_cost (value) and orc.match_cost_grad (both gradients), any match matrix."""
    rng = np.random.RandomState(5)
    a, c = (rng.rand(2, 50, 3) - 0.5).astype(F32), (rng.rand(2, 50, 3) - 0.5).astype(F32)
    match = orc.approx_match(a, c)
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tc = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    val = R._Graph({}, None).earth_mover(ta, tc, match)
    exp = (orc.match_cost(a, c, match).astype(np.float64) / 50.0).mean()
    assert abs(float(val.detach()) - exp) <= 1e-6 * exp
    g1, g2 = torch.autograd.grad(val * 50.0 * 2, (ta, tc))  # d sum_b cost_b
    e1, e2 = orc.match_cost_grad(a, c, match)
    assert np.abs(g1.numpy() - e1).max() <= 1e-5 * np.abs(e1).max() and np.abs(g2.numpy() - e2).max() <= 1e-5 * np.abs(e2).max()


# ---- the gradient against central differences ----------------------------------------------------------------------------
H = (4e-6, 2e-6)
# a unit direction over the 288 input coordinates moves each by 0.06 h, one over the 3.8 M parameters by 5e-4 h: kinks
# come a hundred times sooner along the input (one lies inside h = 4e-6 for the direction below: 5.9e-4 relative)
H_INPUT = (1e-6, 5e-7)


def _directional(case, loss_at, ana, what, steps=H):
    """Central differences of the float64 loss at the steps H against <grad, direction> = ana.  The error of one
    estimate is c h^2 + r / h + (a term that does not shrink when a ReLU or arg-max kink lies inside (-h, h)).  At steps
    small enough that no kink lies inside, c h^2 is below the rounding term r / h (r <= |loss| 2^-52), so the h^2 law
    shows as: halving the step leaves at most a quarter of the error plus that rounding term.  A kink crossing breaks
    both assertions (measured: 1.7e-4 and 4.4e-5 relative at h = 1e-5 for two of these directions)."""
    loss = abs(case["r64"]["terms"]["loss"])
    errs = []
    for h in steps:
        fd = (loss_at(+h) - loss_at(-h)) / (2 * h)
        errs.append(abs(fd - ana))
        print(f"{what}: h = {h:g}: central difference {fd!r}, <grad, direction> {ana!r}, relative error {errs[-1] / abs(ana):.2e}")
        assert errs[-1] <= 1e-6 * abs(ana), (what, h, fd, ana)
    assert errs[1] <= errs[0] / 4 + loss * 2.0 ** -52 / steps[1], (what, errs)


@pytest.mark.parametrize("direction", range(4))
def test_parameter_gradient_against_central_differences(case96, direction):
    v = {k: np.asarray(x, np.float64) for k, x in case96["variables"].items()}
    rng = np.random.RandomState(70 + direction)
    u = {k: rng.randn(*x.shape) for k, x in v.items()}
    norm = np.sqrt(sum(float((x * x).sum()) for x in u.values()))
    u = {k: x / norm for k, x in u.items()}
    g = case96["r64"]["grads"]
    ana = sum(float((g[k] * u[k]).sum()) for k in u if g[k] is not None)

    def loss_at(h):
        return R.run({k: v[k] + h * u[k] for k in v}, case96["partial"], case96["gt"], case96["choices"], grad=False)["terms"]["loss"]
    _directional(case96, loss_at, ana, f"parameter direction {direction}")


def test_input_gradient_against_central_differences(case96):
    p = case96["partial"].astype(np.float64)
    u = np.random.RandomState(75).randn(*p.shape)
    u /= np.sqrt((u * u).sum())
    ana = float((case96["r64"]["input_grads"][0] * u[0]).sum())

    def loss_at(h):
        return R.run(case96["variables"], p + h * u, case96["gt"], case96["choices"], grad=False)["terms"]["loss"]
    _directional(case96, loss_at, ana, "input direction", H_INPUT)


# ---- which variables have a gradient -------------------------------------------------------------------------------------
def test_variables_without_a_gradient_are_the_dead_set(case96):
    g = case96["r64"]["grads"]
    none = {k for k, x in g.items() if x is None or not x.any()}
    dead = {k for k in g if R.is_dead(k)}
    assert none == dead, sorted(none ^ dead)
    assert len([k for k in dead if "refine_layer_final/feat_refine" in k]) == 6
    assert len([k for k in dead if k.startswith("decode_cell_1/state") and "expand" not in k]) == 2
    assert len([k for k in dead if k.startswith("decode_cell_1/state_expand")]) == 32
    assert all(np.isfinite(x).all() for x in g.values() if x is not None)
    assert case96["r64"]["input_grads"][0].any() and np.isfinite(case96["r64"]["input_grads"][0]).all()


def test_a_batch_of_two_equal_samples_has_the_single_samples_gradient(case96):
    """Every loss term is a batch mean: two copies of one sample give the B = 1 loss and parameter gradient, and each copy
    of the input half the B = 1 input gradient (what the GPU test's b2_equal case rests on)."""
    ch = {k: tuple(np.concatenate([x, x]) for x in v) if isinstance(v, tuple) else np.concatenate([v, v])
          for k, v in case96["choices"].items()}
    one = case96["r64"]
    two = R.run(case96["variables"], [case96["partial"][0]] * 2, np.concatenate([case96["gt"]] * 2), ch)
    assert abs(two["terms"]["loss"] - one["terms"]["loss"]) <= 1e-13 * abs(one["terms"]["loss"])
    for k, g in one["grads"].items():
        assert (g is None) == (two["grads"][k] is None), k
        if g is not None:
            assert np.abs(two["grads"][k] - g).max() <= 1e-11 * max(np.abs(g).max(), 1e-300), k
    for g in two["input_grads"]:
        assert np.abs(2 * g - one["input_grads"][0]).max() <= 1e-11 * np.abs(one["input_grads"][0]).max()


# ---- the hinge of zero_groupnear ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts", [96, 700])
def test_both_hinges_are_active_at_the_seeded_weights(variables, morc, case96, npts):
    """The oracle on _seeded_net() at B = 1, seed-3 inputs: loss_d1 ~ 9.9e-4, loss_d2 ~ 1.18e-3 (the move tensors come out
    of layers that do not see the raw cloud's size except through the code words)."""
    from oracle.rfnet_oracle import RFNetOracle
    if npts == 96:
        o, out, gt = case96["oracle"], case96["oracle_out"], case96["gt"]
    else:
        partial, gt = _inputs(npts)
        o = RFNetOracle(variables, morc)
        out = o.forward(partial)
    g = gt.astype(np.float64)
    gt1 = np.take_along_axis(g, morc.farthest_point_sample(64, gt)[..., None].astype(np.int64), 1)
    gt2 = np.take_along_axis(g, morc.farthest_point_sample(1024, gt)[..., None].astype(np.int64), 1)
    d1 = 0.05 * o.zero_groupnear(gt1, gt2, out["decode_move64"])
    d2 = 0.05 * o.zero_groupnear(gt2, g, out["decode_move1024"])
    print(f"{npts} partial points: loss_d1 {d1!r}, loss_d2 {d2!r}")
    assert 5e-4 < d1 < 2e-3 and 5e-4 < d2 < 2e-3
    if npts == 96:
        for term in ("loss_d1", "loss_d2"):  # an active hinge reaches the move layers
            r = R.run(variables, case96["partial"], gt, case96["choices"], term=term)
            assert r["terms"][term] > 0 and r["grads"]["decode_cell/points_out/weights"].any(), term


def test_a_clamped_hinge_passes_no_gradient(clamped):
    o, out = clamped["oracle"], clamped["oracle_out"]
    g = clamped["gt"].astype(np.float64)
    ch = clamped["choices"]
    gt1 = np.take_along_axis(g, ch["gt_fps64"][..., None].astype(np.int64), 1)
    gt2 = np.take_along_axis(g, ch["gt_fps1024"][..., None].astype(np.int64), 1)
    assert o.zero_groupnear(gt1, gt2, out["decode_move64"]) == 0.0       # the oracle says 0
    assert o.zero_groupnear(gt2, g, out["decode_move1024"]) == 0.0
    assert clamped["r64"]["terms"]["loss_d1"] == 0.0 and clamped["r64"]["terms"]["loss_d2"] == 0.0
    for term in ("loss_d1", "loss_d2"):
        r = R.run(clamped["variables"], clamped["partial"], clamped["gt"], ch, term=term)
        assert all(x is None or not x.any() for x in r["grads"].values()), term
        assert all(x is None or not x.any() for x in r["input_grads"]), term
        assert r["grads"]["decode_cell/points_out/weights"] is not None  # on the path, and exactly zero
        opened = R.run(clamped["variables"], clamped["partial"], clamped["gt"], ch, term=term, mutate="hinge_open")
        assert opened["grads"]["decode_cell/points_out/weights"].any(), "the mutation opens the hinge"


# ---- units on a kink ----------------------------------------------------------------------------------------------------
KINK_UNIT = (("refine_layer1", "feat_refine1", 0, 0), 38 * 128 + 100)


def test_a_unit_on_a_kink_is_found_and_its_flip_is_a_one_sided_gradient(case96):
    """At these inputs unit (row 38, channel 100) of refine_layer1/feat_refine1 has a float64 pre-activation inside fp32
    rounding of zero (+1.4e-8).  Flipping it leaves the forward where it is (the unit's value is ~0 on both sides) and moves
    the gradient by a finite amount, upstream of the unit only."""
    assert KINK_UNIT in case96["units"], case96["units"]
    assert KINK_UNIT in [u for u, _ in case96["jumps"]]
    print(f"{len(case96['units'])} units within fp32 rounding of a kink, {len(case96['jumps'])} of them move the gradient: "
          f"{[u for u, _ in case96['jumps']]}")
    one = case96["r64"]
    flipped = R.run(case96["variables"], case96["partial"], case96["gt"], case96["choices"], flip={KINK_UNIT[0]: [KINK_UNIT[1]]})
    for k in R.OUTPUTS:
        assert np.abs(flipped["out"][k] - one["out"][k]).max() <= 1e-7 * np.abs(one["out"][k]).max(), k
    assert abs(flipped["terms"]["loss"] - one["terms"]["loss"]) <= 1e-8 * abs(one["terms"]["loss"])
    jump, rel = R.errors(R.flat_gradient(flipped), case96["g64"])
    print(f"jump: relative L2 {rel:.3e}; " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(jump.items(), key=lambda t: -t[1])[:4]))
    assert jump["refine_layer1/feat_refine1/weights"] > 100 * case96["bar"]["refine_layer1/feat_refine1/weights"]
    downstream = ("refine_layer2/", "refine_layer_final/", "cell_1/", "cell_2/", "decode_cell_1/", "recover2/", "recover3/")
    assert all(v < 1e-6 for k, v in jump.items() if k.startswith(downstream))
    assert all(jump[k] > 1e-5 for k in ("refine_layer1/feat_refine0/weights", "init_mlp/ini_layer0/weights", "input"))


def test_the_nearest_one_sided_gradient_is_chosen_and_nothing_else(case96):
    """A float32 run with the unit on the other side, standing in for an fp32 forward that rounds the other way, misses the bar
    against the reference; choose_flips names exactly that unit, and against the reference with it flipped the run is inside
    the bar.  The unmutated float32 run is given no flip."""
    c = case96
    other = R.flat_gradient(R.run(c["variables"], c["partial"], c["gt"], c["choices"], dtype=torch.float32,
                                  flip={KINK_UNIT[0]: [KINK_UNIT[1]]}))
    err, _ = R.errors(other, c["g64"])
    assert any(err[k] > c["bar"][k] for k in err)
    assert R.choose_flips(c["jumps"], other, c["r64"]) == [KINK_UNIT]
    chosen, flipped = R.one_sided_reference(c["variables"], c["partial"], c["gt"], c["choices"], c["r64"], c["units"], other)
    assert chosen == [KINK_UNIT]
    err, rel = R.errors(other, R.flat_gradient(flipped))
    worst = max(err, key=lambda k: err[k] / c["bar"][k])
    print(f"against the flipped reference: worst {worst} at {err[worst] / c['bar'][worst]:.3f} of its bar, relative L2 {rel:.3e}")
    assert all(err[k] <= c["bar"][k] for k in err) and rel <= c["rel_bar"]
    assert R.choose_flips(c["jumps"], R.flat_gradient(c["r32"]), c["r64"]) == []


# ---- every deliberate error stands above the GPU test's bar ---------------------------------------------------------------
@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutations_stand_ten_times_above_the_bar(case96, clamped, mutate):
    """The float32 run of the mutated reference against the unmutated float64 run, under the bar the GPU test uses
    (R.bars of the unmutated float32 run): at least one variable must miss it by 10 x.  hinge_open changes nothing while
    the hinges are active, so it runs on the clamped case."""
    case = clamped if mutate == "hinge_open" else case96
    r = R.run(case["variables"], case["partial"], case["gt"], case["choices"], dtype=torch.float32, mutate=mutate)
    assert r["terms"]["loss"] == case["r32"]["terms"]["loss"], "a mutation changes gradients only"
    err, rel = R.errors(R.flat_gradient(r), case["g64"])
    worst = max(err, key=lambda k: err[k] / case["bar"][k])
    over = sum(err[k] > case["bar"][k] for k in err)
    print(f"{mutate}: worst {worst}: error {err[worst]:.3e} = {err[worst] / case['bar'][worst]:.1f} x its bar {case['bar'][worst]:.3e}; "
          f"{over} of {len(err)} gradients outside their bar; relative L2 {rel:.3e} against the bar {case['rel_bar']:.3e}")
    assert err[worst] >= 10 * case["bar"][worst], (mutate, worst, err[worst], case["bar"][worst])
    # ... and no flip of units on a kink brings it inside: against the nearest one-sided gradient it misses by as much
    chosen = R.choose_flips(case["jumps"], R.flat_gradient(r), case["r64"])
    if chosen:
        flipped = R.run(case["variables"], case["partial"], case["gt"], case["choices"], flip=R._flip_of(chosen))
        err, _ = R.errors(R.flat_gradient(r), R.flat_gradient(flipped))
        worst = max(err, key=lambda k: err[k] / case["bar"][k])
        print(f"{mutate}: against the reference with {chosen} flipped: worst {worst} at {err[worst] / case['bar'][worst]:.1f} x its bar")
        assert err[worst] >= 10 * case["bar"][worst], (mutate, chosen, worst, err[worst], case["bar"][worst])
