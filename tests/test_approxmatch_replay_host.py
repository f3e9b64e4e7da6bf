"""CPU: tests/approxmatch_replay.py held to itself before tests/test_gpu_emd_levels.py holds the kernels to it.

  self-consistency  the float64 schedule's own vectors replay with a ratio of at most 1e-6 (the replay restates the schedule
                    it is driven by), its `match` is _am64's and its cost the C oracle's to 1e-5;
  calibration       the float32 restatement of the schedule (rf::d2_fma's roundings, exp2 of the fp32 argument, fp32 sums)
                    replays with a ratio of at most 0.5 on every input of the GPU test: the reference measured against its own
                    float64, with a margin of 2 up to the GPU test's bar of 1.0 for hardware exp2 and other summation orders;
  mutation          on the same inputs every planted omission -- 16 columns out of P1's or P3's sum, 16 points out of P2's, a
                    level's term out of `match` -- gives a ratio of at least 10 in some comparison at every level where the
                    omitted points carry mass (approxmatch_replay.carried: at least MASS_MIN of a unit mass through them, for a
                    single well-conditioned point), and the inputs keep such mass at the sharpest, a middle and the last level.

The calibration maxima per comparison kind and the smallest mutation ratio are printed by the tests (-s) and quoted in
approxmatch_replay's docstring (MEASURED).  Mutations run at every level on the inputs of up to 4.5e5 pairs; the larger ones
(640 x 2048, 2048 x 640, 4100 x 520, 1000 x 1500) are calibrated only."""
import functools

import numpy as np
import pytest

import approxmatch_replay as R

REF = R.default_levels()
# The replay's bounds are at most N u of the mass in play per element (N <= 780 terms here: 4.6e-5), so an omission that moves
# 1e-3 of a unit mass at one well-conditioned point stands a factor 10 above them with room to spare.
MASS_MIN = 1e-3
MATCH_MIN = 1e-4  # (a `match` entry's bound is about 1e-6 of the entry)
BIG = 4.5e5       # pairs above which an input is calibrated only (the mutation runs cost 40 schedules per input)


SCHED = R.SCHEDULES


def _levels(name):
    return REF if SCHED[name] is None else SCHED[name]


def _inputs():
    """(id, n, m, kind, seed, sample, schedule name, counts or None) of every cloud pair the GPU test replays."""
    out = []
    for tn, tab in (("dense", R.DENSE), ("live", R.LIVE), ("sorted", R.SORTED), ("emd", R.EARTH_MOVER)):
        for idx, (b, n, m, kind) in enumerate(tab):
            for i in R.replayed_samples(b):
                out.append((f"{tn}-{b}x{n}x{m}-s{i}", n, m, kind, R.case_seed(tn, idx), i, "reference", None))
    for idx, (b, n, m, kind) in enumerate(R.SCHEDULE_SHAPES):
        for name in SCHED:
            out.append((f"schedule-{name}-{n}x{m}", n, m, kind, R.case_seed("schedule", idx), b - 1, name, None))
    b, n, m, kind, c1, c2 = R.RAGGED
    for i in range(b):
        out.append((f"ragged-s{i}", n, m, kind, R.case_seed("ragged", 0), i, "reference", (c1[i], c2[i])))
    return out


INPUTS = _inputs()
SMALL = [t for t in INPUTS if t[1] * t[2] <= BIG and t[6] == "reference"]


def _clouds(t):
    _, n, m, kind, seed, i, _, counts = t
    a, c = R.sample_clouds(seed, i, n, m, kind)
    if counts is not None:
        a, c = a[:counts[0]], c[:counts[1]]
    return a, c


_seen = {"cal": {}, "mut": [np.inf, None]}


@pytest.mark.parametrize("t", SMALL[::3], ids=lambda t: t[0])
def test_float64_schedule_replays_itself_and_is_the_oracles(orc, t):
    from test_gpu_memory_contract import _am64
    a, c = _clouds(t)
    s = R.schedule(a, c, REF, np.float64)
    res = R.replay(a, c, REF, s["RL"], s["RR"], s["rl_last"], s["rr_last"])
    worst = R.worst_ratio(res)
    assert worst[0] <= 1e-6, worst
    want = _am64(a[None], c[None], REF)[0]
    # (_am64 adds the double 1e-9 where the kernels, the oracle and this schedule add 1e-9f: 3e-8 of it, which a row that divides
    # by little else passes on)
    assert np.abs(s["match"] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    mt, mb = R.match_from_vectors(a, c, REF, s["RL"], s["RR"])
    assert (np.abs(mt - s["match"]) <= 1e-12 + 1e-9 * mb).all()
    # the gradient sums against a plain loop formulation on a few points
    g1, _, g2, _ = R.grads_from_vectors(a, c, mt, mb)
    for k in (0, len(a) - 1):
        d = a[k].astype(np.float64) - c.astype(np.float64)
        ref = (d * (mt[:, k] / np.sqrt(np.maximum((d ** 2).sum(1), 1e-20)))[:, None]).sum(0)
        assert np.allclose(g1[k], ref, rtol=1e-12, atol=1e-15)
    o1, o2 = orc.match_cost_grad(a[None], c[None], mt.astype(np.float32)[None])
    assert np.allclose(g1, o1[0], rtol=1e-3, atol=1e-4) and np.allclose(g2, o2[0], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("n,m", [(300, 257), (260, 780), (513, 700)])
def test_float64_schedule_has_the_oracles_cost(orc, n, m):
    """On uniform cubes, where the fp32 oracle's own chain is sound to 1e-5 (on the paired clouds its cost is 1.1e-5 off this
    float64 run at 300 x 257: the chain's ill-conditioning in fp32, tests/test_oracle_golden.py, not a difference of formula --
    `match` itself is compared with _am64 on those inputs above)."""
    rng = np.random.RandomState(n + m)
    a = (rng.random_sample((n, 3)) - 0.5).astype(np.float32)
    c = (rng.random_sample((m, 3)) - 0.5).astype(np.float32)
    s = R.schedule(a, c, REF, np.float64)
    mt, mb = R.match_from_vectors(a, c, REF, s["RL"], s["RR"])
    cost = R.cost_from_vectors(a, c, mt, mb)[0]
    oc = float(orc.match_cost(a[None], c[None], orc.approx_match(a[None], c[None]))[0])
    assert abs(cost - oc) <= 1e-5 * abs(oc), (cost, oc)
    assert R.worst_ratio(R.replay(a, c, REF, s["RL"], s["RR"], s["rl_last"], s["rr_last"]))[0] <= 1e-6


@pytest.mark.parametrize("t", INPUTS, ids=lambda t: t[0])
def test_float32_schedule_replays_within_half_the_bar(t):
    a, c = _clouds(t)
    lv = _levels(t[6])
    s = R.schedule(a, c, lv, np.float32)
    res = R.replay(a, c, lv, s["RL"], s["RR"], s["rl_last"], s["rr_last"])
    for key, (ratio, pos) in res.items():
        _seen["cal"][key[1]] = max(_seen["cal"].get(key[1], 0.0), ratio)
    worst = R.worst_ratio(res)
    print(f"{t[0]}: calibration worst {worst[0]:.3f} at {worst[1]} [{worst[2]}]; maxima so far {_seen['cal']}")
    assert worst[0] <= 0.5, worst
    if t[1] * t[2] <= BIG:
        mt, mb = R.match_from_vectors(a, c, lv, s["RL"], s["RR"])
        mr = R.ratio_of(s["match"], mt, mb)
        print(f"    match {mr[0]:.3f}")
        assert mr[0] <= 1.0, mr  # (numpy's own `match` chain, held to the GPU test's bar)


def test_read_vectors_slices_the_documented_layout():
    n, m, nlv, b = 300, 257, 3, 2
    npad, mpad, V, bstride = R.layout(n, m, nlv)
    cpad = R.kernel_constants()["CPAD"]
    assert npad % cpad == 0 and mpad % cpad == 0 and npad - n < cpad and V == npad + mpad and bstride == (1 + nlv) * V
    ws = np.zeros(b * bstride + 64, np.float32)
    for bi in range(b):
        for s in range(1 + nlv):
            o = bi * bstride + s * V
            ws[o:o + n] = 100 * bi + 10 * s + 1
            ws[o + npad:o + npad + m] = 100 * bi + 10 * s + 2
    vec = R.read_vectors(ws, b, n, m, nlv)
    assert (vec[1]["RL"][2] == 131).all() and (vec[1]["RR"][0] == 112).all() and vec[1]["RL"].shape == (nlv, n)
    assert (vec[0]["rl_last"] == 1).all() and (vec[1]["rr_last"] == 102).all() and vec[0]["rr_last"].shape == (m,)
    ws[bstride + V + n] = 1.0  # a padded entry of sample 1's ratioL_0
    with pytest.raises(AssertionError):
        R.read_vectors(ws, b, n, m, nlv)
    ws[bstride + V + n] = 0.0
    short = R.read_vectors(ws[:], b, n, m, nlv)[0]
    R.cheap_invariants(dict(RL=np.ones((2, 3), np.float32), RR=np.array([[1, 0.5, 0], [1, 0.25, 0]], np.float32),
                            rl_last=np.ones(3, np.float32), rr_last=np.array([0.5, 0.1, 0], np.float32)), 3, 3)
    with pytest.raises(AssertionError):  # a consumed column comes back to life
        R.cheap_invariants(dict(RL=np.ones((2, 3), np.float32), RR=np.array([[1, 0.5, 0], [1, 0.25, 0.1]], np.float32),
                                rl_last=np.ones(3, np.float32), rr_last=np.array([0.5, 0.1, 0], np.float32)), 3, 3)
    assert short["RL"].shape == (nlv, n)


def test_paired_clouds_keep_partners_in_range():
    for kind in ("jitter", "duplicates", "lopsided"):
        a, c = R.paired_clouds(np.random.RandomState(5), 301, 450, kind)
        d2 = R._d2(a, c, np.float64)
        assert np.sqrt(d2.min(0)).max() < R.SHARP_RANGE and np.sqrt(d2.min(1)).max() < R.SHARP_RANGE
        assert a.dtype == np.float32 and a.shape == (301, 3) and c.shape == (450, 3)
        if kind == "duplicates":
            assert (d2 == 0).sum() > 10


@functools.lru_cache(maxsize=None)
def _masses(tid):
    """The float64 run of a small input -> {kind: per level, the mass the omitted points carry}."""
    t = next(x for x in SMALL if x[0] == tid)
    a, c = _clouds(t)
    s64 = R.schedule(a, c, REF, np.float64)
    car = R.carried(a, c, REF, s64)
    d2 = R._d2(a, c, np.float64)
    car["match"] = np.zeros(len(REF))
    for v, lv in enumerate(REF):
        e = np.ones_like(d2) if lv == 0.0 else np.exp(lv * d2)
        low = s64["RL"][v] < np.median(s64["RL"][v])
        car["match"][v] = (e * s64["RL"][v][None, :] * s64["RR"][v][:, None])[:, low].max(initial=0.0)
    car["p3"][-1] = 0.0  # (P3 of the last level only updates remainL, which nothing reads: the kernels do not launch it)
    return car


def _matters(kind, mass):
    return mass >= (MATCH_MIN if kind == "match" else MASS_MIN)


@pytest.mark.parametrize("t", SMALL, ids=lambda t: t[0])
def test_planted_omissions_are_found_wherever_they_matter(t):
    a, c = _clouds(t)
    nlv = len(REF)
    car = _masses(t[0])
    clean = R.schedule(a, c, REF, np.float32)
    mt, mb = R.match_from_vectors(a, c, REF, clean["RL"], clean["RR"])
    for kind in R.FAULTS:
        for v in range(nlv):
            mass = float(car[kind][v])
            if not _matters(kind, mass):
                continue
            if kind == "match":
                f = R.schedule(a, c, REF, np.float32, fault=(v, kind))
                ratio = R.ratio_of(f["match"], mt, mb)[0]
            else:
                # (a schedule cut two levels behind the fault is a shorter call: its end comparisons hold as well)
                f = R.schedule(a, c, REF, np.float32, fault=(v, kind), upto=min(nlv, v + 2))
                ratio = R.worst_ratio(R.replay(a, c, REF, f["RL"], f["RR"], f["rl_last"], f["rr_last"]))[0]
            if ratio < _seen["mut"][0]:
                _seen["mut"] = [ratio, (t[0], kind, v, mass)]
            assert ratio >= 10, f"{t[0]}: {kind} at level {v} moves {mass:.2e} of a unit mass and shows as {ratio:.2f}"
    print(f"{t[0]}: smallest mutation ratio so far {_seen['mut']}")


def test_the_inputs_keep_mass_at_the_sharp_a_middle_and_the_last_level():
    """From the float64 runs alone: every kind of omission has inputs whose omitted points carry mass at the sharpest level, at
    a middle one and at the last (P3: the last one that is launched).  An input family that cannot show a fault is replaced
    in approxmatch_replay.py, not excused here."""
    last = len(REF) - 1
    for kind in R.FAULTS:
        got = {v for t in SMALL for v in range(len(REF)) if _matters(kind, float(_masses(t[0])[kind][v]))}
        want_last = last - 1 if kind == "p3" else last
        assert 0 in got and want_last in got and got & {3, 4, 5, 6}, (kind, sorted(got))
