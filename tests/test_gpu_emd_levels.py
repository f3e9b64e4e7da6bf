"""GPU: approx_match / earth_mover held LAUNCH BY LAUNCH to a float64 replay of their own stored vectors.

tests/test_gpu_emd.py compares `match` with the fp32 oracle over the whole annealing chain, which is ill-conditioned
(tests/test_oracle_golden.py::test_match_bar_is_ill_conditioned), so its bars are stray counts that a sweep which leaves out a
sub-chunk of columns still passes.  Here every call goes straight through the C ABI with this test's own workspace; the vector
region at its start (approxmatch.hip AmLayout) holds every level's ratioL / ratioR and the final remainL / remainR, and
tests/approxmatch_replay.py turns them into 3 * nlevels + 2 well-conditioned comparisons per sample, each with a derived bound
per element (its docstring) and each naming one launch:
    (v, "P2")  am_p2 of level v;   (v, "P1")  the P1 half of am_p1 / am_p3p1 of level v, in shipped mass;
    (v, "L")   remainL as that launch read it, i.e. the P3 half of am_p3p1 of level v (P3 of level v - 1);
    ("end", "rl" | "rr")  slot 0 after the call.
A ratio (error over bound) above 1.0 fails and names level, phase and element.  `match` is held entry by entry, and earth_mover's
cost and gradients, to what the stored vectors imply (match_from_vectors ...), again with bounds per element.  Every case asserts
from the library's own launch names (rf_profile_collect) that it ran on the route it is meant for.  For batches the first, the
middle and the last sample are replayed; every other sample's vectors pass approxmatch_replay.cheap_invariants.

The inputs are approxmatch_replay's paired clouds (mass alive at the omitted points through the last level) -- the ones
tests/test_approxmatch_replay_host.py calibrates (fp32 restatement: at most 0.5) and plants omissions in (at least 10).

Measured on the MI355X (approxmatch_replay's docstring, MEASURED, has all of it): the largest replay ratio is 0.26 (dense 0.24, live
sets 0.25, sorted / masked 0.26, swept 0.26, schedules 0.22, ragged 0.24, earth_mover 0.23); `match` entries reach 0.61 of their
bound, the cost 0.005, the gradients 0.063; v_exp_f32 is 1.39 u off at worst and flushes results below 2^-126."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import approxmatch_replay as R

pytestmark = pytest.mark.gpu

AUTO, SWEPT = 0, 1
REF = R.default_levels()
_worst = {}  # route -> [largest replay ratio, where]; printed as the cases run


def _lib():
    from rfnet_amd import _lib as L
    return L


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _f32_levels(name):
    lv = R.SCHEDULES[name]
    return None if lv is None else [float(np.float32(v)) for v in lv]


class Run:
    """One call through the C ABI with a poisoned workspace of this test's own -> outputs, the vector region, launch names."""

    def __init__(self, entry, a, c, levels=None, mode=AUTO, lengths=None, grad=False):
        L = _lib()
        lib = L.lib
        b, n, m = a.shape[0], a.shape[1], c.shape[1]
        self.b, self.n, self.m = b, n, m
        self.levels = REF if levels is None else levels
        nlv = 0 if levels is None else len(levels)
        ta, tc = cu(a), cu(c)
        lv = None if levels is None else (C.c_float * nlv)(*levels)
        l1 = l2 = None
        if lengths is not None:
            l1, l2 = cu(np.asarray(lengths[0], np.int32)), cu(np.asarray(lengths[1], np.int32))
        if entry == "approxmatch":
            need = (lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, nlv) if lengths is not None
                    else lib.rf_approxmatch_mode_workspace_bytes(b, n, m, nlv, mode))
        else:
            need = (lib.rf_earth_mover_lengths_workspace_bytes(b, n, m) if lengths is not None
                    else lib.rf_earth_mover_mode_workspace_bytes(b, n, m, mode))
        assert need > 0
        ws = torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda")  # (a vector entry nobody wrote shows)
        torch.cuda.synchronize()
        L.profile_collect()
        L.profile_enable(True)
        try:
            if entry == "approxmatch":
                self.match = torch.full((b, m, n), float("nan"), dtype=torch.float32, device="cuda")
                if lengths is not None:
                    st = lib.rf_approxmatch_lengths(b, n, m, ta.data_ptr(), tc.data_ptr(), l1.data_ptr(), l2.data_ptr(),
                                                    self.match.data_ptr(), lv, nlv, ws.data_ptr(), need, None)
                else:
                    st = lib.rf_approxmatch_mode(b, n, m, ta.data_ptr(), tc.data_ptr(), self.match.data_ptr(), lv, nlv,
                                                 ws.data_ptr(), need, None, mode)
            else:
                self.cost = torch.full((b,), float("nan"), dtype=torch.float32, device="cuda")
                self.g1 = torch.full((b, n, 3), float("nan"), dtype=torch.float32, device="cuda") if grad else None
                self.g2 = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device="cuda") if grad else None
                gp = (self.g1.data_ptr(), self.g2.data_ptr()) if grad else (None, None)
                if lengths is not None:
                    st = lib.rf_earth_mover_lengths(b, n, m, ta.data_ptr(), tc.data_ptr(), l1.data_ptr(), l2.data_ptr(),
                                                    self.cost.data_ptr(), gp[0], gp[1], ws.data_ptr(), need, None)
                else:
                    st = lib.rf_earth_mover_mode(b, n, m, ta.data_ptr(), tc.data_ptr(), self.cost.data_ptr(), gp[0], gp[1],
                                                 ws.data_ptr(), need, None, mode)
            torch.cuda.synchronize()
            self.names = {k: v[1] for k, v in L.profile_collect().items()}
        finally:
            L.profile_enable(False)
        assert st == 0, st
        nl = len(self.levels)
        region = ws[: b * R.layout(n, m, nl)[3]].cpu().numpy()
        self.vec = R.read_vectors(region, b, n, m, nl, lengths)  # (asserts the padding; NaN poison left in a real entry fails below)
        self.lengths = lengths


def _route(run, want, absent):
    for name in want:
        assert name in run.names, f"not on its route: no {name} launch among {sorted(run.names)}"
    for name in absent:
        assert name not in run.names, f"not on its route: a {name} launch among {sorted(run.names)}"
    assert "am_small" not in run.names


def _replay(route, run, a, c, samples=None, match=True):
    """The replayed samples against the float64 replay (and `match`); every sample's cheap invariants."""
    for bi in range(run.b):
        n1, m1 = (run.n, run.m) if run.lengths is None else (int(run.lengths[0][bi]), int(run.lengths[1][bi]))
        R.cheap_invariants(run.vec[bi], n1, m1)
    for bi in (R.replayed_samples(run.b) if samples is None else samples):
        v = run.vec[bi]
        n1, m1 = v["RL"].shape[1], v["RR"].shape[1]
        ai, ci = a[bi, :n1], c[bi, :m1]
        res = R.replay(ai, ci, run.levels, v["RL"], v["RR"], v["rl_last"], v["rr_last"])
        worst = R.worst_ratio(res)
        if worst[0] > _worst.get(route, [0.0])[0]:
            _worst[route] = [worst[0], f"{run.b}x{run.n}x{run.m} sample {bi} {worst[1]} element {worst[2]}"]
        print(f"[{route}] {run.b}x{run.n}x{run.m} sample {bi}: worst replay ratio {worst[0]:.3f} at {worst[1]} element {worst[2]}"
              f"; route maxima {_worst}")
        bad = {k: r for k, r in res.items() if not r[0] <= 1.0}
        assert not bad, f"sample {bi}: level / phase -> (ratio, element) above the bound: {bad}"
        if match and hasattr(run, "match"):
            mt, mb = R.match_from_vectors(ai, ci, run.levels, v["RL"], v["RR"])
            got = run.match[bi].cpu().numpy()
            mr = R.ratio_of(got[:m1, :n1], mt, mb)
            print(f"    match: worst entry ratio {mr[0]:.3f}")
            assert mr[0] <= 1.0, f"sample {bi}: match entry {divmod(mr[1], n1)} (l, k) is {mr[0]:.2f} bounds from its vectors' value"
            if run.lengths is not None:
                assert (got[m1:] == 0).all() and (got[:, n1:] == 0).all()


def _clouds(table, idx, b, n, m, kind):
    return R.batch_clouds(R.case_seed(table, idx), b, n, m, kind)


# ------------------------------------------------------------------------------------------------ the exponential
def test_exp2_error_is_within_the_replays_h():
    """v_exp_f32 through rf_probe_exp2 against float64 at 2e6 arguments over [-160, 0]: relative error where the result is a
    normal number, absolute below.  The replay's bounds take H_EXP2 = 2^-23 and E_FLOOR = 2^-126."""
    L = _lib()
    rng = np.random.RandomState(1)
    x = np.concatenate([np.linspace(-160.0, 0.0, 1000001), -rng.random_sample(1000000) * 160.0,
                        -np.arange(0, 161, dtype=np.float64)]).astype(np.float32)
    tx = cu(x)
    ty = torch.empty_like(tx)
    L.check(L.lib.rf_probe_exp2(tx.data_ptr(), ty.data_ptr(), tx.numel(), None), "rf_probe_exp2")
    y = ty.cpu().numpy().astype(np.float64)
    want = np.exp2(x.astype(np.float64))
    normal = want >= 2.0 ** -126
    rel = float((np.abs(y - want)[normal] / want[normal]).max())
    absl = float(np.abs(y - want)[~normal].max())
    print(f"v_exp_f32 over [-160, 0]: max relative error {rel:.3e} = {rel / 2.0 ** -24:.2f} u on normal results; "
          f"max absolute error {absl:.3e} = {absl / 2.0 ** -126:.3f} * 2^-126 below")
    assert rel <= R.H_EXP2 and absl <= R.E_FLOOR


# ------------------------------------------------------------------------------------------------ approx_match: the routes
@pytest.mark.parametrize("idx", range(len(R.DENSE)), ids=lambda i: "x".join(map(str, R.DENSE[i][:3])))
def test_dense_pipeline(idx):
    """A cloud in 257 .. 511: above the one-workgroup kernel, below the live sets -- the plain dense sweeps at every level."""
    b, n, m, kind = R.DENSE[idx]
    small = R.kernel_constants()["AM_SMALL"]
    assert max(n, m) > small and min(n, m) < 512
    a, c = _clouds("dense", idx, b, n, m, kind)
    run = Run("approxmatch", a, c)
    _route(run, ("am_init", "am_p1", "am_p3p1", "am_p2", "am_match"), ("am_compact", "nnp_sort"))
    assert run.names["am_p2"] == 10 and run.names["am_p3p1"] == 9
    _replay("dense", run, a, c)


@pytest.mark.parametrize("idx", range(len(R.LIVE)), ids=lambda i: "x".join(map(str, R.LIVE[i][:3])))
def test_live_sets(idx):
    """Both clouds >= 512: from the third level on the sweeps run over the packed live columns / rows (am_compact_kernel, am_rowk
    CMP, am_p2_live; 4100 x 520 takes am_p2_live's short row items, PL_ROWS_BIG, from the fifth level on)."""
    b, n, m, kind = R.LIVE[idx]
    a, c = _clouds("live", idx, b, n, m, kind)
    run = Run("approxmatch", a, c)
    _route(run, ("am_compact", "am_p1", "am_p3p1", "am_p2", "am_match"), ("nnp_sort",))
    assert run.names["am_compact"] == 1
    if idx == len(R.LIVE) - 1:
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rfnet_amd", "csrc", "approxmatch.hip")).read()
        assert n > int(re.search(r"PL_BIG_N\s*=\s*(\d+)", src).group(1))
    _replay("live", run, a, c)


@pytest.mark.parametrize("mode", [AUTO, SWEPT], ids=["auto", "swept"])
@pytest.mark.parametrize("idx", range(len(R.SORTED)), ids=lambda i: "x".join(map(str, R.SORTED[i][:3])))
def test_sorted_masked_sweeps(idx, mode):
    """From 6e7 pairs on the sharp levels take their rows in spatial order, skip columns and visit listed ones (am_rowk / am_rowl
    SKIP, MASK), then the live sets; RF_EMD_SWEPT pins the same batch to the plain dense sweeps."""
    b, n, m, kind = R.SORTED[idx]
    assert b * n * m >= 6.0e7
    a, c = _clouds("sorted", idx, b, n, m, kind)
    run = Run("approxmatch", a, c, mode=mode)
    if mode == AUTO:
        _route(run, ("nnp_sort", "am_compact", "am_match"), ())
    else:
        _route(run, ("am_p1", "am_p3p1", "am_p2", "am_match"), ("nnp_sort", "am_compact"))
    _replay("sorted" if mode == AUTO else "swept", run, a, c)


@pytest.mark.parametrize("name", list(R.SCHEDULES))
@pytest.mark.parametrize("idx", range(len(R.SCHEDULE_SHAPES)), ids=lambda i: "x".join(map(str, R.SCHEDULE_SHAPES[i][:3])))
def test_schedules(idx, name):
    """Schedules of 1 .. 50 levels on the live-set and on the dense route: the three ten-level materialisations (reference, off
    the quarter chain, non-zero last level), am_match_any's one to four groups of sixteen, its runs of five, a repeated
    multiplier (one exponential for P3 and P1) and a zero multiplier in the middle of the chain."""
    b, n, m, kind = R.SCHEDULE_SHAPES[idx]
    a, c = _clouds("schedule", idx, b, n, m, kind)
    lv = _f32_levels(name)
    run = Run("approxmatch", a, c, levels=lv)
    nlv = len(run.levels)
    _route(run, ("am_p1", "am_p2", "am_match"), ("nnp_sort",))
    assert run.names["am_p2"] == nlv and run.names.get("am_p3p1", 0) == nlv - 1 and run.names["am_match"] == 1
    live = min(n, m) >= 512 and nlv >= 4  # (the packed sets start at the third level and need two levels behind it)
    assert ("am_compact" in run.names) == live, (sorted(run.names), nlv)
    _replay(f"schedules-{n}x{m}", run, a, c, samples=[b - 1])


def test_ragged_batch():
    """rf_approxmatch_lengths: per-sample counts (700 | 513 | 257 against 600 | 300 | 599), NaN behind the counts; the replay runs
    on the slices with the multipliers of the counts, the vectors behind the counts are 0."""
    b, n, m, kind, c1, c2 = R.RAGGED
    a, c = _clouds("ragged", 0, b, n, m, kind)
    for i in range(b):
        a[i, c1[i]:] = np.nan
        c[i, c2[i]:] = np.nan
    run = Run("approxmatch", a, c, lengths=(c1, c2))
    _route(run, ("am_p1", "am_p3p1", "am_p2", "am_match"), ("nnp_sort", "am_compact"))
    _replay("ragged", run, a, c, samples=range(b))


# ------------------------------------------------------------------------------------------------ earth_mover
@pytest.mark.parametrize("form", ["cost", "grad", "swept", "lengths"])
@pytest.mark.parametrize("idx", range(len(R.EARTH_MOVER)), ids=lambda i: "x".join(map(str, R.EARTH_MOVER[i][:3])))
def test_earth_mover(idx, form):
    """rf_earth_mover_mode / _lengths: the level pipeline replayed from the fused op's own workspace, then the cost (the
    class-sorted cost-only form, the fused form with gradients, the pinned route, ragged counts) and both gradients against
    what the stored vectors imply."""
    b, n, m, kind = R.EARTH_MOVER[idx]
    a, c = _clouds("emd", idx, b, n, m, kind)
    lengths = None
    if form == "lengths":
        lengths = ([n, n - 44], [m - 3, m])
        a[1, n - 44:] = np.nan
        c[0, m - 3:] = np.nan
    grad = form != "cost"
    run = Run("earth_mover", a, c, mode=SWEPT if form == "swept" else AUTO, lengths=lengths, grad=grad)
    live = min(n, m) >= 512 and form in ("cost", "grad")
    _route(run, ("am_p1", "am_p3p1", "am_p2", "emd_pack_cols", "mc_final"), ("nnp_sort", "am_match"))
    assert ("am_compact" in run.names) == live
    if grad:
        assert run.names.get("emd_fused_grad") == 1 and "emd_fused" not in run.names
    else:
        assert run.names["emd_pack_cols"] == 2 and run.names.get("emd_fused") == 1  # (count + pack: the class-sorted columns)
    _replay(f"earth_mover-{form}", run, a, c, samples=range(b))
    cost = run.cost.cpu().numpy()
    for bi in range(b):
        v = run.vec[bi]
        n1, m1 = v["RL"].shape[1], v["RR"].shape[1]
        ai, ci = a[bi, :n1], c[bi, :m1]
        mt, mb = R.match_from_vectors(ai, ci, REF, v["RL"], v["RR"])
        want, bound = R.cost_from_vectors(ai, ci, mt, mb)
        cr = R.ratio_of(cost[bi:bi + 1], np.array([want]), np.array([bound]))[0]
        print(f"    sample {bi}: cost {cost[bi]:.6f} against {want:.6f}, ratio {cr:.3f} (bound {bound:.2e})")
        assert cr <= 1.0, (bi, float(cost[bi]), want, bound)
        if grad:
            g1, b1, g2, b2 = R.grads_from_vectors(ai, ci, mt, mb)
            got1, got2 = run.g1[bi].cpu().numpy(), run.g2[bi].cpu().numpy()
            r1, r2 = R.ratio_of(got1[:n1], g1, b1), R.ratio_of(got2[:m1], g2, b2)
            print(f"    sample {bi}: grad1 ratio {r1[0]:.3f}, grad2 ratio {r2[0]:.3f}")
            assert r1[0] <= 1.0 and r2[0] <= 1.0, (bi, r1, r2)
            assert (got1[n1:] == 0).all() and (got2[m1:] == 0).all()
