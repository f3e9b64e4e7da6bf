"""GPU: rf_nn_metrics / rf_chamfer_metrics / rf_chamfer_metrics_grad (rfnet_amd/csrc/chamfer_metrics.hip) against the
float64 restatement of include/rfops.h's definitions (tests/test_chamfer_metrics_host.py: metrics_ref, grad_weights_ref)
applied to the oracle's nn_distance outputs on each sample's unpadded slices.

Bars (the issue's): dist / idx / counts exact; columns 4-7 bit-exact (max and integer counts are order-free, one
correctly rounded fp32 division); column 8 rel 1e-6; columns 0-3 rel 1e-5 (the glue tolerance); columns 9, 10 rel 1e-5 +
abs 1e-6 (a term 1 - e/c at distance ~ 0 carries a few ulp of 1.0 ~ 2.4e-7; the floor is four times that); gradients
rel 1e-4 + abs 1e-5 (rfops.h's bar for fused gradients).

Shapes: each is the smallest that reaches its path.  The LDS histogram holds CM_LDS_BINS = 32768 bins
(chamfer_metrics.hip): "d" has 70001 bins in direction 1 (global atomics) and 300 in direction 2, "cap" / "cap1" sit
on either side of the cap, and test_nn_metrics_with_both_directions_beyond_the_lds_cap has both clouds above it."""
import numpy as np
import pytest
import torch

from conftest import assert_rel
from test_chamfer_metrics_host import NCOL, grad_weights_ref, metrics_ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
CM_LDS_BINS = 32768


def _unit(rng, *shape):
    return (rng.random_sample(shape) - 0.5).astype(F32)


def _inputs(name):
    """-> (xyz1, xyz2, len1 | None, len2 | None, tau, alpha)"""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "a":  # odd sizes, full counts
        return _unit(rng, 3, 301, 3), _unit(rng, 3, 257, 3), None, None, 0.1, 40.0
    if name == "b":  # ragged, counts 1 and full among them; hostile padding
        a, c = _unit(rng, 4, 700, 3), _unit(rng, 4, 1100, 3)
        l1, l2 = np.array([700, 1, 333, 64], I32), np.array([1100, 900, 1, 65], I32)
        a[1, 1:], c[1, 900:] = np.nan, np.inf
        a[2, 333:], c[2, 1:] = np.inf, np.nan
        a[3, 64:] = a[3, np.arange(700 - 64) % 64]  # copies of valid points: read, they would win and be counted
        c[3, 65:] = a[3, np.arange(1100 - 65) % 64]
        return a, c, l1, l2, 0.08, 60.0
    if name == "c":  # collisions and ties: every xyz1 point jittered around one of 40, duplicates in both clouds
        c = _unit(rng, 2, 40, 3)
        c[:, 30:] = c[:, :10]  # duplicated candidates: ties go to the lowest index, the copies get count 0
        a = np.stack([c[i, rng.randint(0, 40, 500)] for i in range(2)]) + (0.01 * rng.randn(2, 500, 3)).astype(F32)
        a[:, 400:] = c[:, rng.randint(0, 40, 100)]  # exact copies of candidates: zero distances
        a[:, 380:400] = a[:, 360:380]
        return a.astype(F32), c, None, None, 0.02, 1000.0
    if name == "d":  # bins beyond the LDS cap in direction 1, a tiny bin set in direction 2 (dense sweep, 2.1e7 pairs)
        return _unit(rng, 1, 300, 3), _unit(rng, 1, 70001, 3), None, None, 0.05, 200.0
    if name == "cap":  # the last size whose bins fit the LDS
        return _unit(rng, 1, 64, 3), _unit(rng, 1, CM_LDS_BINS, 3), None, None, 0.05, 200.0
    if name == "cap1":  # the first that does not, ragged: the global histogram with counts behind the valid range
        return _unit(rng, 2, 64, 3), _unit(rng, 2, CM_LDS_BINS + 1, 3), np.array([64, 7], I32), np.array([CM_LDS_BINS + 1, 5000], I32), 0.05, 200.0
    # "e" / "e_full": the culled sweep.  nn_distance.hip culled_pays: both clouds >= 512 points, n * m >= 2^21 and, for
    # clouds of at most 4096 points, b * n * m >= 2^24: with b = 2 that is n * m >= 2^23, first met on square clouds at
    # 2897^2 = 8392609 (2896^2 = 8386816 is dense).  "e" is ragged (the epilogue writes the padded slots there).
    a, c = _unit(rng, 2, 2897, 3), _unit(rng, 2, 2897, 3)
    if name == "e_full":
        return a, c, None, None, 0.03, 1000.0
    assert name == "e"
    a[1, 1500:], c[0, 2000:] = np.nan, c[0, :897]
    return a, c, np.array([2897, 1500], I32), np.array([2000, 2897], I32), 0.03, 1000.0


_CASES = {}


def case(name, orc):
    """Inputs and reference of a shape, computed once and shared (never modified)."""
    if name in _CASES:
        return _CASES[name]
    a, c, l1, l2, tau, alpha = _inputs(name)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    L1 = np.full(b, n, I32) if l1 is None else l1
    L2 = np.full(b, m, I32) if l2 is None else l2
    thr2 = float(F32(tau) * F32(tau))
    r = dict(a=a, c=c, l1=l1, l2=l2, L1=L1, L2=L2, tau=tau, alpha=alpha, thr2=thr2, b=b, n=n, m=m,
             d1=np.zeros((b, n), F32), i1=np.full((b, n), -1, I32), d2=np.zeros((b, m), F32), i2=np.full((b, m), -1, I32),
             c1=np.zeros((b, n), I32), c2=np.zeros((b, m), I32), met=np.zeros((b, NCOL)))
    for i in range(b):
        n_, m_ = L1[i], L2[i]
        e = orc.nn_distance(a[i:i + 1, :n_].copy(), c[i:i + 1, :m_].copy())
        r["d1"][i, :n_], r["i1"][i, :n_], r["d2"][i, :m_], r["i2"][i, :m_] = e[0][0], e[1][0], e[2][0], e[3][0]
        r["met"][i], r["c1"][i, :n_], r["c2"][i, :m_] = metrics_ref(e[0][0], e[1][0], e[2][0], e[3][0], thr2, alpha)
    _CASES[name] = r
    return r


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def check_metrics(got, exp, what):
    got, exp = np.asarray(got, F32), np.asarray(exp, np.float64)
    print(f"{what}: max rel err by column",
          " ".join("%.2e" % (np.abs(got[:, k] - exp[:, k]) / np.maximum(np.abs(exp[:, k]), 1e-300)).max() for k in range(NCOL)))
    assert np.array_equal(got[:, 4:8], exp[:, 4:8].astype(F32)), f"{what}: columns 4-7 are not bit-exact"
    assert_rel(got[:, 8], exp[:, 8], 1e-6, what=f"{what}: column 8")
    assert_rel(got[:, 0:4], exp[:, 0:4], 1e-5, what=f"{what}: columns 0-3")
    assert_rel(got[:, 9:11], exp[:, 9:11], 1e-5, 1e-6, what=f"{what}: columns 9, 10")


def run_fused(r, device_counts=False):
    from rfnet_amd import _raw
    l1 = None if r["l1"] is None else (_dev(r["l1"]) if device_counts else r["l1"].tolist())
    l2 = None if r["l2"] is None else (_dev(r["l2"]) if device_counts else r["l2"].tolist())
    out = _raw.chamfer_metrics(_dev(r["a"]), _dev(r["c"]), r["tau"], r["alpha"], lengths1=l1, lengths2=l2)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_fused(out, r, what):
    met, d1, i1, d2, i2, c1, c2 = out
    for k, g in (("d1", d1), ("i1", i1), ("d2", d2), ("i2", i2), ("c1", c1), ("c2", c2)):
        # (padded slots: dist +0, idx -1, count 0 -- they are in the expected arrays)
        assert np.array_equal(g, r[k]) and g.dtype == r[k].dtype, f"{what}: {k} differs from the oracle"
    assert not np.signbit(d1).any() and not np.signbit(d2).any()
    for i in range(r["b"]):  # a valid point's own neighbour always has a count >= 1
        assert (c2[i][i1[i, :r["L1"][i]]] >= 1).all() and (c1[i][i2[i, :r["L2"][i]]] >= 1).all()
        assert c2[i].sum() == r["L1"][i] and c1[i].sum() == r["L2"][i]
    check_metrics(met, r["met"], what)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "cap", "cap1", "e", "e_full"])
def test_fused_forward(orc, name):
    r = case(name, orc)
    from rfnet_amd._lib import lib
    # which sweep RF_NN_AUTO (mode 0) takes: its workspace is the pinned sweep's (1 dense, 2 culled), and the two differ
    ws = [lib.rf_nn_distance_mode_workspace_bytes(r["b"], r["n"], r["m"], mode) for mode in (0, 1, 2)]
    assert ws[1] != ws[2] and ws[0] == ws[2 if name.startswith("e") else 1], "not the sweep this shape is here for"
    out = run_fused(r)
    check_fused(out, r, name)
    again = run_fused(r, device_counts=True)  # counts as a device tensor; and a second call: identical bits everywhere
    for g, h in zip(out, again):
        assert g.tobytes() == h.tobytes(), f"{name}: two calls differ"


def test_nn_metrics_on_outputs_of_every_route(orc):
    """The epilogue alone on dist / idx the caller holds: the dense sweep's, the culled sweep's, sorted handles'."""
    from rfnet_amd import _raw
    r = case("e_full", orc)
    a, c = _dev(r["a"]), _dev(r["c"])
    routes = {"dense": _raw.nn_distance(a, c, mode="dense"), "culled": _raw.nn_distance(a, c, mode="culled"),
              "sorted": _raw.nn_distance_sorted(_raw.nn_sort(a), _raw.nn_sort(c))}
    first = None
    for k, (d1, i1, d2, i2) in routes.items():
        out = [t.cpu().numpy() for t in _raw.nn_metrics(d1, i1, d2, i2, r["tau"], r["alpha"])]
        check_metrics(out[0], r["met"], f"nn_metrics on {k}")
        assert np.array_equal(out[1], r["c1"]) and np.array_equal(out[2], r["c2"]), k
        first = first or out
        assert all(g.tobytes() == h.tobytes() for g, h in zip(first, out)), k
    # ragged: padded slots of dist / idx are not read (NaN / out-of-range there change nothing)
    r = case("b", orc)
    d1, i1, d2, i2 = r["d1"].copy(), r["i1"].copy(), r["d2"].copy(), r["i2"].copy()
    for i in range(r["b"]):
        d1[i, r["L1"][i]:], i1[i, r["L1"][i]:] = np.nan, 1 << 30
        d2[i, r["L2"][i]:], i2[i, r["L2"][i]:] = np.inf, -7
    out = [t.cpu().numpy() for t in _raw.nn_metrics(_dev(d1), _dev(i1), _dev(d2), _dev(i2), r["tau"], r["alpha"],
                                                   lengths1=r["l1"].tolist(), lengths2=_dev(r["l2"]))]
    check_metrics(out[0], r["met"], "nn_metrics ragged")
    assert np.array_equal(out[1], r["c1"]) and np.array_equal(out[2], r["c2"])


def test_nn_metrics_with_both_directions_beyond_the_lds_cap():
    """n and m above CM_LDS_BINS: no LDS histogram, both directions count with global atomics.  The epilogue alone on
    made-up dist / idx (a sweep of 1e9 pairs and its oracle would take too long here): skewed indices, so that some bins
    collect thousands of points and most none; ragged, with rubbish behind the counts."""
    from rfnet_amd import _raw
    rng = np.random.RandomState(11)
    b, n, m = 2, CM_LDS_BINS + 1, CM_LDS_BINS + 7
    L1, L2 = np.array([n, 20001], I32), np.array([m - 3, m], I32)
    d1, d2 = (rng.rand(b, n) ** 4 * 1e-2).astype(F32), (rng.rand(b, m) ** 4 * 1e-2).astype(F32)
    i1, i2 = np.zeros((b, n), I32), np.zeros((b, m), I32)
    exp, c1, c2 = np.zeros((b, NCOL)), np.zeros((b, n), I32), np.zeros((b, m), I32)
    tau, alpha = 0.03, 500.0
    for i in range(b):
        i1[i, :L1[i]] = (rng.rand(L1[i]) ** 3 * L2[i]).astype(I32)
        i2[i, :L2[i]] = (rng.rand(L2[i]) ** 3 * L1[i]).astype(I32)
        exp[i], c1[i, :L1[i]], c2[i, :L2[i]] = metrics_ref(d1[i, :L1[i]], i1[i, :L1[i]], d2[i, :L2[i]], i2[i, :L2[i]],
                                                          float(F32(tau) * F32(tau)), alpha)
        d1[i, L1[i]:], i1[i, L1[i]:], d2[i, L2[i]:], i2[i, L2[i]:] = np.nan, -5, np.inf, 1 << 29
    assert c2.max() > 100 and (c2 == 0).sum() > m // 2
    outs = [[t.cpu().numpy() for t in _raw.nn_metrics(_dev(d1), _dev(i1), _dev(d2), _dev(i2), tau, alpha,
                                                      lengths1=_dev(L1), lengths2=_dev(L2))] for _ in range(2)]
    check_metrics(outs[0][0], exp, "both beyond the cap")
    assert np.array_equal(outs[0][1], c1) and np.array_equal(outs[0][2], c2)
    assert all(g.tobytes() == h.tobytes() for g, h in zip(*outs))


def _abi_nn_metrics(r, thr2, alpha):
    from rfnet_amd._lib import lib
    b, n, m = r["b"], r["n"], r["m"]
    t = [_dev(r[k]) for k in ("d1", "i1", "d2", "i2")]
    met = torch.empty(b, NCOL, device="cuda")
    c1, c2 = torch.empty(b, n, dtype=torch.int32, device="cuda"), torch.empty(b, m, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.rf_nn_metrics_workspace_bytes(b, n, m), dtype=torch.uint8, device="cuda")
    st = lib.rf_nn_metrics(b, n, m, *[x.data_ptr() for x in t], None, None, thr2, alpha, met.data_ptr(), c1.data_ptr(),
                           c2.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    return met.cpu().numpy()


def test_threshold_edges(orc):
    from rfnet_amd import _raw
    r = case("a", orc)
    assert min(r["d1"].min(), r["d2"].min()) > 0
    # a threshold below every distance: nobody is inside, and the harmonic mean of (0, 0) is +0, not NaN
    tau = float(np.sqrt(min(r["d1"].min(), r["d2"].min()))) * 0.5
    met = _raw.chamfer_metrics(_dev(r["a"]), _dev(r["c"]), tau, r["alpha"])[0].cpu().numpy()
    assert not met[:, 6:9].any() and not np.signbit(met[:, 6:9]).any()
    rest = [0, 1, 2, 3, 4, 5, 9, 10]  # the threshold touches no other column
    assert np.array_equal(met[:, rest], _abi_nn_metrics(r, r["thr2"], r["alpha"])[:, rest])
    # thr2 = +inf through the C ABI: everybody; thr2 == 0: the compare is strict, nobody
    assert (_abi_nn_metrics(r, float("inf"), r["alpha"])[:, 6:9] == 1).all()
    assert not _abi_nn_metrics(r, 0.0, r["alpha"])[:, 6:9].any()
    # tau so small that float32(tau)^2 underflows to 0: a valid threshold of 0
    assert not _raw.chamfer_metrics(_dev(r["a"]), _dev(r["c"]), 1e-30, r["alpha"])[0].cpu().numpy()[:, 6:9].any()
    # thr2 exactly one of the distances: that point is outside
    d = np.sort(r["d1"][0])
    k = 100
    assert d[k - 1] < d[k]
    assert _abi_nn_metrics(r, float(d[k]), r["alpha"])[0, 6] == F32(k) / F32(r["n"])


def test_graph_capture_with_device_counts(orc):
    """No host synchronisation anywhere: the fused call is captured with device counts; replayed after inputs and
    counts changed in place it returns what the eager call returns on them, bit for bit."""
    from rfnet_amd import _host, _raw
    if not _host.graph_replay_ok():
        pytest.skip("this process started the HIP runtime without DEBUG_CLR_GRAPH_PACKET_CAPTURE=0: captured graphs "
                    "do not replay correctly")
    r = case("b", orc)
    a, c, l1, l2 = _dev(r["a"]), _dev(r["c"]), _dev(r["l1"]), _dev(r["l2"])
    args = (r["tau"], r["alpha"])
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        _raw.chamfer_metrics(a, c, *args, lengths1=l1, lengths2=l2)
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _raw.chamfer_metrics(a, c, *args, lengths1=l1, lengths2=l2)
    graph.replay()
    torch.cuda.synchronize()
    check_fused([t.cpu().numpy() for t in out], r, "replay on the captured inputs")
    # other inputs, in place: the clouds of sample 0 everywhere, and other counts
    a.copy_(a[0:1].expand_as(a).clone())
    c.copy_(c[0:1].expand_as(c).clone())
    l1.copy_(torch.tensor([5, 700, 699, 350], dtype=torch.int32))
    l2.copy_(torch.tensor([1100, 2, 1000, 129], dtype=torch.int32))
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out]
    eager = [t.cpu().numpy() for t in _raw.chamfer_metrics(a, c, *args, lengths1=l1, lengths2=l2)]
    for g, e in zip(got, eager):
        assert g.tobytes() == e.tobytes()
    assert (got[2][1, 700 - 1] >= 0) and (got[2][0, 5:] == -1).all() and (got[4][1, 2:] == -1).all()


# ---- backward ---------------------------------------------------------------------------------------------------
def _grad_ref(orc, r, gm):
    """float64 gd1 / gd2 from the formula, cast to fp32, through the oracle's NnDistanceGrad on the slices."""
    g1, g2 = np.zeros((r["b"], r["n"], 3), F32), np.zeros((r["b"], r["m"], 3), F32)
    for i in range(r["b"]):
        n_, m_ = r["L1"][i], r["L2"][i]
        d1, i1, d2, i2 = r["d1"][i, :n_], r["i1"][i, :n_], r["d2"][i, :m_], r["i2"][i, :m_]
        gd1 = grad_weights_ref(d1, i1, r["c2"][i], gm[i], 1, r["alpha"]).astype(F32)
        gd2 = grad_weights_ref(d2, i2, r["c1"][i], gm[i], 2, r["alpha"]).astype(F32)
        with np.errstate(invalid="ignore"):
            g = orc.nn_distance_grad(r["a"][i:i + 1, :n_].copy(), r["c"][i:i + 1, :m_].copy(), gd1[None], i1[None], gd2[None], i2[None])
        g1[i, :n_], g2[i, :m_] = g[0][0], g[1][0]
    return g1, g2


def _run_grad(r, gm):
    from rfnet_amd import _raw
    l1 = None if r["l1"] is None else _dev(r["l1"])
    l2 = None if r["l2"] is None else _dev(r["l2"])
    g = _raw.chamfer_metrics_grad(_dev(r["a"]), _dev(r["c"]), *[_dev(r[k]) for k in ("d1", "i1", "d2", "i2", "c1", "c2")],
                                  r["alpha"], _dev(gm), lengths1=l1, lengths2=l2)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in g]


def _check_grad(got, exp, r, what):
    for k, (g, e, L) in enumerate(zip(got, exp, (r["L1"], r["L2"]))):
        for i in range(r["b"]):  # rows behind a count: exactly +0
            assert not g[i, L[i]:].any() and not np.signbit(g[i, L[i]:]).any(), f"{what}: grad_xyz{k + 1} behind the count"
        fin = np.isfinite(e)  # (everywhere, except where a test says otherwise)
        assert np.isfinite(g[fin]).all(), f"{what}: grad_xyz{k + 1} is not finite where the reference is"
        print(f"{what}: grad_xyz{k + 1} max abs err {np.abs(g[fin] - e[fin]).max():.3e} of max {np.abs(e[fin]).max():.3e}")
        assert_rel(g[fin], e[fin], 1e-4, 1e-5, what=f"{what}: grad_xyz{k + 1}")


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_backward(orc, name):
    r = case(name, orc)
    gm = np.random.RandomState(77).randn(r["b"], NCOL).astype(F32)
    if name == "c":
        # zero distances (duplicated points): with CD-L1's upstream at exactly 0 its 1 / sqrt(0) is never formed
        gm[:, 0:2] = 0
        assert (r["d1"] == 0).any()
    exp = _grad_ref(orc, r, gm)
    got = _run_grad(r, gm)
    _check_grad(got, exp, r, name)
    if name == "c":
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # columns 4-8 carry no gradient whatever the upstream holds there
    gm2 = gm.copy()
    gm2[:, 4:9] = np.nan
    again = _run_grad(r, gm2)
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got, again)), "columns 4-8 of grad_metrics were read"


def test_backward_with_zero_distances_and_cd_l1_upstream(orc):
    """(c) with every column's upstream random: the CD-L1 term is infinite at a zero distance, as in rf_chamfer_loss_grad
    and in the reference's own sqrt: the bar holds wherever the reference gradient is finite."""
    r = case("c", orc)
    gm = np.random.RandomState(78).randn(r["b"], NCOL).astype(F32)
    _check_grad(_run_grad(r, gm), _grad_ref(orc, r, gm), r, "c, all columns")


def test_glue_autograd_agrees_with_the_raw_calls(orc):
    from rfnet_amd import glue
    r = case("b", orc)
    l1, l2 = r["l1"].tolist(), r["l2"].tolist()
    a, c = _dev(r["a"]).requires_grad_(True), _dev(r["c"]).requires_grad_(True)
    out = glue.chamfer_metrics(a, c, tau=r["tau"], alpha=r["alpha"], lengths1=l1, lengths2=l2)
    raw = out["raw"].detach().cpu().numpy()
    check_metrics(raw, r["met"], "glue")
    for key, exp in (("cd_l1", (raw[:, 0] + raw[:, 1]) / 2), ("cd_l2", raw[:, 2] + raw[:, 3]),
                     ("hausdorff", np.sqrt(np.maximum(raw[:, 4], raw[:, 5]))), ("precision", raw[:, 6]),
                     ("recall", raw[:, 7]), ("fscore", raw[:, 8]), ("dcd", (raw[:, 9] + raw[:, 10]) / 2)):
        assert out[key].shape == (r["b"],) and np.array_equal(out[key].detach().cpu().numpy(), exp.astype(F32)), key
    assert np.array_equal(out["idx1"].cpu().numpy(), r["i1"]) and not out["idx1"].requires_grad
    assert not out["fscore"].requires_grad and not out["hausdorff"].requires_grad and out["cd_l2"].requires_grad
    out["dcd"].sum().backward()
    gm = np.zeros((r["b"], NCOL), F32)
    gm[:, 9:11] = 0.5
    exp = _run_grad(r, gm)
    assert a.grad.cpu().numpy().tobytes() == exp[0].tobytes() and c.grad.cpu().numpy().tobytes() == exp[1].tobytes()
    # dcd_loss: the batch mean
    a2, c2 = _dev(r["a"]).requires_grad_(True), _dev(r["c"]).requires_grad_(True)
    loss = glue.dcd_loss(a2, c2, alpha=r["alpha"], lengths1=l1, lengths2=l2)
    assert_rel(float(loss.detach()), ((r["met"][:, 9] + r["met"][:, 10]) / 2).mean(), 1e-5, 1e-6, what="dcd_loss")
    loss.backward()
    exp = _run_grad(r, gm / r["b"])
    assert a2.grad.cpu().numpy().tobytes() == exp[0].tobytes() and c2.grad.cpu().numpy().tobytes() == exp[1].tobytes()
