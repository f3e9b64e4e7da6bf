"""GPU: rf_knn_feature (include/rfops.h, knn_feature.hip) against its numpy restatement, bit for bit.

tests/test_knn_feature_host.py restates the contract with an exact fp32 fma (`knn_feature_ref`) and holds that restatement to
an int64 brute force; here the kernels' val and idx are compared with it as bytes over the channel counts around the slab and
the matrix instruction's K, every list bucket's edges, tile edges, clustered and duplicate rows, non-finite values and ragged
batches.  One check goes round the restatement: float64 distances and the chain's own error bound.  Then determinism, the
independence of a sample from its batch, graph capture, and the gradients of glue.knn_feature against float64 autograd."""
import numpy as np
import pytest
import torch

from test_knn_feature_host import brute_int, int_features, knn_feature_ref

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def run(k, f1, f2, l1=None, l2=None):
    from rfnet_amd import _raw
    a = cu(f1)
    q = a if f2 is f1 else cu(f2)
    val, idx = _raw.knn_feature(k, a, q, None if l1 is None else cu(np.asarray(l1, I32)), None if l2 is None else cu(np.asarray(l2, I32)))
    assert val.shape == (f1.shape[0], f2.shape[1], k) and val.dtype == torch.float32 and idx.dtype == torch.int32
    return host(val), host(idx)


def same(got, want, what):
    (gv, gi), (wv, wi) = got, want
    bad = np.argwhere((gi != wi) | (gv.view(np.uint32) != wv.view(np.uint32)))
    if len(bad):
        s, j, t = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {gi.size} slots differ; first at sample {s} query {j} slot {t}: got "
                             f"({gv[s, j, t]!r}, {gi[s, j, t]}), want ({wv[s, j, t]!r}, {wi[s, j, t]})")


def features(kind, seed, b, n, m, c):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((b, n, c)).astype(F32), rng.standard_normal((b, m, c)).astype(F32)
    if kind == "clustered":  # cancellation, negative d, near-ties
        base = rng.standard_normal((b, 1, c)) * 3
        return ((base + 1e-4 * rng.standard_normal((b, n, c))).astype(F32), (base + 1e-4 * rng.standard_normal((b, m, c))).astype(F32))
    if kind == "duplicates":
        pool = rng.standard_normal((b, 7, c)).astype(F32)
        pick = lambda r: np.stack([pool[i, rng.integers(0, 7, r)] for i in range(b)])  # noqa: E731
        return pick(n), pick(m)
    raise KeyError(kind)


# ---- 1. bit equality with the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "clustered", "duplicates"])
@pytest.mark.parametrize("c", [1, 2, 3, 7, 32, 33, 64, 100])
def test_channels(c, kind):
    f1, f2 = features(kind, c, 2, 70, 45, c)
    same(run(20, f1, f2), knn_feature_ref(20, f1, f2), f"{kind}, c = {c}")


@pytest.mark.parametrize("k", [1, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_bucket_edges(k):
    for kind in ("normal", "clustered"):
        f1, f2 = features(kind, 40 + k, 2, 70, 45, 33)
        same(run(k, f1, f2), knn_feature_ref(k, f1, f2), f"{kind}, k = {k}")


@pytest.mark.parametrize("n,m,c,k", [(257, 129, 16, 20), (1, 1, 5, 1), (20, 33, 9, 20), (64, 64, 4, 64)])
def test_tile_edges_and_smallest_sizes(n, m, c, k):
    f1, f2 = features("normal", n, 2, n, m, c)
    same(run(k, f1, f2), knn_feature_ref(k, f1, f2), f"n = {n}, m = {m}, c = {c}, k = {k}")


def test_a_set_against_itself():
    for kind in ("normal", "clustered"):
        f1, _ = features(kind, 5, 2, 70, 1, 33)
        got = run(20, f1, f1)
        same(got, knn_feature_ref(20, f1, f1), f"feat1 is feat2, {kind}")
    assert (got[0] > 0).any(), "the clustered case must produce negative d"


# ---- 2. integers: exact everywhere ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 64, 130])
def test_integers_equal_the_brute_force(c):
    hi = 8 if c > 1 else 3
    f1, f2 = int_features(c, 2, 150, c, hi), int_features(50 + c, 2, 70, c, hi)
    f2[:, :20] = f1[:, 10:30]
    same(run(20, f1, f2), brute_int(20, f1, f2), f"integers, c = {c}")


def test_three_channels_of_integers_equal_knn_point():
    from rfnet_amd import _raw
    f1, f2 = int_features(3, 2, 300, 3, 4), int_features(4, 2, 140, 3, 4)
    val, idx = _raw.knn_point(16, cu(f1), cu(f2), form="scan")
    same(run(16, f1, f2), (host(val), host(idx)), "c = 3 against knn_point's scan")


# ---- 3. non-finite values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan candidate", "inf query", "overflow"])
def test_non_finite(what):
    f1, f2 = features("normal", 77, 3, 70, 45, 33)
    clean = run(20, f1, f2)
    if what == "nan candidate":
        f1[1, 13] = np.nan
        f1[1, 40, 32] = np.nan
    elif what == "inf query":
        f2[1, 7, 3] = np.inf
        f2[1, 9] = -np.inf
    else:
        f1[1, 22] = 2e19  # ip overflows against itself, sq1 is +inf
        f1[1, 23, 0] = 1.5e19
        f2[1, 5, 0] = 1.5e19  # sq2 + sq1 overflows, ip does not
        f2[1, 6, 0] = -3e19
    got = run(20, f1, f2)
    same(got, knn_feature_ref(20, f1, f2), what)
    for s in (0, 2):
        same((got[0][s:s + 1], got[1][s:s + 1]), (clean[0][s:s + 1], clean[1][s:s + 1]), f"{what}: sample {s} is untouched")
    assert not np.isfinite(got[0][1]).all()


# ---- 4. round the restatement: float64 distances and the chain's own bound -----------------------------------------
@pytest.mark.parametrize("kind,c", [("normal", 64), ("clustered", 33), ("normal", 100)])
def test_against_float64_within_the_chains_bound(kind, c):
    """Each of the c fmas of a chain, the sum sq2 + sq1 and the last fma round once, relative error 2^-24 of a partial result
    that is at most the sum of the magnitudes: |d - D| <= (c + 3) 2^-24 (sq1 + sq2 + 2 sum |q x|) =: E.  A returned val is
    within E of -D at its index, and a k-th neighbour cannot be farther than the true k-th by more than 2 E (the largest E
    of the row): whatever was left out had d >= the returned k-th's d."""
    k = 20
    f1, f2 = features(kind, 9, 2, 70, 45, c)
    val, idx = run(k, f1, f2)
    a, q = f1.astype(F64), f2.astype(F64)
    D = ((q[:, :, None, :] - a[:, None, :, :]) ** 2).sum(-1)
    E = (c + 3) * 2.0 ** -24 * ((a * a).sum(-1)[:, None, :] + (q * q).sum(-1)[:, :, None]
                                + 2 * (np.abs(q)[:, :, None, :] * np.abs(a)[:, None, :, :]).sum(-1))
    Dg, Eg = np.take_along_axis(D, idx.astype(np.int64), -1), np.take_along_axis(E, idx.astype(np.int64), -1)
    err = np.abs(-val.astype(F64) - Dg)
    print(f"max |val + D| / E = {(err / Eg).max():.3f}")
    assert (err <= Eg).all()
    kth = np.sort(D, -1)[..., k - 1]
    over = Dg[..., k - 1] - kth
    print(f"max (returned k-th - true k-th) / 2E = {(over / (2 * E.max(-1))).max():.3f}")
    assert (over <= 2 * E.max(-1)).all()
    assert all(len(set(r)) == k for r in idx.reshape(-1, k)) and idx.min() >= 0 and idx.max() < 70


# ---- 5. ragged batches ----------------------------------------------------------------------------------------------------------
def test_ragged_equals_the_calls_on_the_slices():
    from rfnet_amd import _raw
    k, n, m, c = 9, 70, 45, 33
    f1, f2 = features("clustered", 3, 4, n, m, c)
    L1, L2 = np.array([1, k - 1, k, n], I32), np.array([m, 1, 17, m], I32)
    for s in range(4):
        f1[s, L1[s]:] = np.nan
        f2[s, L2[s]:] = np.nan
    val, idx = run(k, f1, f2, L1, L2)
    same((val, idx), knn_feature_ref(k, f1, f2, L1, L2), "ragged against the restatement")
    for s in range(4):
        kv = min(k, L1[s])
        sv, si = run(kv, f1[s:s + 1, :L1[s]], f2[s:s + 1, :L2[s]])
        same((val[s:s + 1, :L2[s], :kv], idx[s:s + 1, :L2[s], :kv]), (sv, si), f"sample {s} against the dense call on its slices")
        assert not val[s, :, kv:].view(np.uint32).any() and not idx[s, :, kv:].any(), f"sample {s}: slots behind kv"
        assert not val[s, L2[s]:].view(np.uint32).any() and not idx[s, L2[s]:].any(), f"sample {s}: padded queries"
    hv, hi = _raw.knn_feature(k, cu(f1), cu(f2), L1.tolist(), torch.from_numpy(L2.astype(np.int64)))  # host counts
    same((host(hv), host(hi)), (val, idx), "host counts against device counts")
    one = run(k, f1, f2, L1, None)  # one count array alone
    same((one[0][3:], one[1][3:]), (val[3:], idx[3:]), "len2 = NULL")


# ---- 6. determinism, batch independence, capture --------------------------------------------------------------------------
def test_two_calls_and_a_sample_alone():
    f1, f2 = features("clustered", 8, 3, 257, 129, 16)
    first = run(20, f1, f2)
    same(run(20, f1, f2), first, "a second call")
    for s in range(3):
        same(run(20, f1[s:s + 1], f2[s:s + 1]), (first[0][s:s + 1], first[1][s:s + 1]), f"sample {s} alone")


def edge_ref(fq, fs, idx, L1, L2):
    b, m, k = idx.shape
    out = np.zeros((b, m, k, 2 * fq.shape[2]), F32)
    for s in range(b):
        kv = min(k, L1[s])
        rows = idx[s, :L2[s], :kv]
        out[s, :L2[s], :kv, :fq.shape[2]] = fs[s][rows] - fq[s, :L2[s], None, :]
        out[s, :L2[s], :kv, fq.shape[2]:] = fq[s, :L2[s], None, :]
    return out


def test_graph_and_edge_feature_eager_and_captured():
    from rfnet_amd import glue
    k, n, c = 8, 130, 12
    sets = []
    for v in range(2):
        f, _ = features("normal", 30 + v, 3, n, 1, c)
        L = np.array([[n, 5, 77], [64, n, 9]][v], I32)
        for s in range(3):
            f[s, L[s]:] = np.nan
        sets.append(dict(f=f, L=L))
    t = {nm: cu(x) for nm, x in sets[0].items()}

    def chain():
        val, idx = glue.knn_feature(k, t["f"], t["f"], t["L"], t["L"])
        return val, idx, glue.edge_feature(t["f"], t["f"], idx, t["L"], t["L"])

    def load(s):
        for nm, x in s.items():
            t[nm].copy_(cu(x))

    eager = []
    for s in (sets[1], sets[0]):
        load(s)
        eager.append([host(x).copy() for x in chain()])
    eager.reverse()
    for v, s in enumerate(sets):
        same((eager[v][0], eager[v][1]), knn_feature_ref(k, s["f"], s["f"], s["L"], s["L"]), f"set {v}: the graph's neighbours")
        want = edge_ref(s["f"], s["f"], eager[v][1], s["L"], s["L"])
        assert eager[v][2].shape == (3, n, k, 2 * c) and np.array_equal(eager[v][2].view(np.uint32), want.view(np.uint32)), f"set {v}: edge_feature"
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        chain()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for v in (0, 1):
        load(sets[v])  # inputs and counts change in place, on the device: nothing is read back
        graph.replay()
        torch.cuda.synchronize()
        for name, got, exp in zip(("val", "idx", "edge"), outs, eager[v]):
            assert host(got).tobytes() == exp.tobytes(), f"replay on set {v}: {name} differs from the eager bits"
    assert eager[0][1].tobytes() != eager[1][1].tobytes()


# ---- 7. gradients -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_gradients_against_float64_autograd(ragged):
    from rfnet_amd import glue
    b, n, m, c, k = 2, 40, 30, 12, 5
    f1, f2 = features("normal", 12, b, n, m, c)
    g = np.random.default_rng(13).standard_normal((b, m, k)).astype(F32)
    L1, L2 = (cu(np.array([n, 3], I32)), cu(np.array([7, m], I32))) if ragged else (None, None)
    a, q = cu(f1).requires_grad_(True), cu(f2).requires_grad_(True)
    val, idx = glue.knn_feature(k, a, q, L1, L2)
    assert val.requires_grad and not idx.requires_grad and idx.dtype == torch.int32
    val.backward(cu(g))
    a64, q64 = cu(f1).double().requires_grad_(True), cu(f2).double().requires_grad_(True)
    gathered = a64[torch.arange(b, device="cuda")[:, None, None], idx.long()]
    e = -((q64[:, :, None, :] - gathered) ** 2).sum(-1)
    live = torch.ones((b, m, k), dtype=torch.bool, device="cuda")
    if ragged:
        live = (torch.arange(k, device="cuda")[None, None, :] < L1[:, None, None]) & (torch.arange(m, device="cuda")[None, :, None] < L2[:, None, None])
    (e * live).backward(cu(g).double())
    for got, exp, name in ((a.grad, a64.grad, "grad_feat1"), (q.grad, q64.grad, "grad_feat2")):
        err = float((got.double() - exp).abs().max())
        print(f"{name}: max err {err:.3e}, max |exp| {float(exp.abs().max()):.3e}")
        assert err <= 1e-5 * float(exp.abs().max()), f"{name}: {err} against the float64 torch expression"
    only = cu(f2).requires_grad_(True)  # one input alone
    glue.knn_feature(k, cu(f1), only, L1, L2)[0].backward(cu(g))
    assert only.grad.cpu().numpy().tobytes() == q.grad.cpu().numpy().tobytes()
