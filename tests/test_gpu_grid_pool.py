"""GPU: rf_grid_cluster, rf_grid_pool and rf_grid_unpool against the numpy restatement of tests/grid_pool_ref.py AS BYTES, for
every output, over n in {1, 63, 64, 65, 1000, 2049, 4097, 8193, 16384} (b = 5, b = 2 above 1000; 2049, 4097 and 8193 are the
first n of the LDS sort's sizes 4096, 8192 and 16384, with lengths n // 2 + 1 beside them), the three orders, c in {1, 3, 5, 64, 130}
and the input families of the contract: everything in one cell, every point in its own cell, exact duplicates, points exactly
on cell faces (j / 64 with cell 1 / 16), cell 0.03 on random cubes, an explicit origin with negative cell indices, cells beyond
+-32768, rows of NaN / +-inf, -0, counts 0, 1 and n with NaN behind them, NaN features under max.  Then the properties: alone
equals in-batch, ragged equals sliced, two calls return the same bits, a permutation of exact-grid points changes nothing, the
gradients through glue as bytes, zero gradients for rows in no cell, no host synchronisation, graph capture."""
import numpy as np
import pytest
import torch

import grid_pool_ref as R
from grid_pool_ref import F32, I32

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 1000, 16384, 2049, 4097, 8193]  # (the last three: the first n of the sort sizes 4096, 8192 and 16384)
CS = [1, 3, 5, 64, 130]
CLUSTER_KEYS = ("origin", "inside", "nclusters", "order", "starts", "cluster", "coords", "code")


def batch_of(n):
    return 2 if n > 1000 else 5


# ---- the input families ------------------------------------------------------------------------------------------------------
def family(name, n, seed):
    rng = np.random.RandomState(seed)
    if name == "one_cell":
        return (rng.rand(n, 3) / 32).astype(F32) + F32(0.25)
    if name == "own_cell":  # a lattice of 32 x 32 x 16 cells of 1 / 16, shuffled
        i = rng.permutation(16384)[:n]
        return (np.stack([i % 32, (i // 32) % 32, i // 1024], 1) / 16.0).astype(F32)
    if name == "duplicates":
        base = (rng.randint(-128, 128, (max(1, n // 7), 3)) / 64.0).astype(F32)
        return base[rng.randint(0, len(base), n)]
    if name == "faces":  # exactly on cell faces: j / 64, cell = 1 / 16
        return (rng.randint(0, 256, (n, 3)) / 64.0).astype(F32)
    if name == "zeros_and_nonfinite":  # -0 among the minima, rows of NaN and +-inf
        x = (rng.randint(0, 64, (n, 3)) / 64.0).astype(F32)
        x[x == 0] = F32(-0.0)
        x[rng.rand(n, 3) < 0.2] = F32(-0.0)
        bad = rng.rand(n) < 0.15
        x[bad, rng.randint(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum())).astype(F32)
        return x
    if name == "cube":
        return (rng.rand(n, 3) - 0.5).astype(F32)
    if name == "beyond":  # cell 0.03: t up to +-50000, part of the rows beyond +-32768 cells
        return ((rng.rand(n, 3) - 0.5) * 3000).astype(F32)
    raise KeyError(name)


def config(cfg, n):
    """-> (xyz (b, n, 3), cell, lengths or None, origin or None)"""
    b = batch_of(n)
    if cfg == "grid":
        fams = ["own_cell", "one_cell", "duplicates", "faces", "zeros_and_nonfinite"][:b]
        return np.stack([family(f, n, 10 + i) for i, f in enumerate(fams)]), 1.0 / 16, None, None
    if cfg == "rand":
        xyz = np.stack([family("cube", n, 20 + i) for i in range(b)])
        lengths = np.array([0, 1, n, n // 2 + 1, max(n - 1, 1)] if b == 5 else [n // 2 + 1, n], I32)
        for i in range(b):
            xyz[i, max(int(lengths[i]), 1):] = np.nan
        return xyz, 0.03, lengths, None
    if cfg == "origin":
        fams = ["cube", "beyond", "zeros_and_nonfinite", "beyond", "cube"][:b]
        xyz = np.stack([family(f, n, 30 + i) for i, f in enumerate(fams)])
        origin = (np.random.RandomState(7).rand(b, 3) * 0.5 + 0.5).astype(F32)  # above every cube: k < 0
        return xyz, 0.03, None, origin
    raise KeyError(cfg)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_cluster(xyz, cell, order, lengths, origin):
    from rfnet_amd import _raw
    r = _raw.grid_cluster(dev(xyz), cell, order, dev(lengths), dev(origin), want_code=True)
    return {k: v.cpu().numpy() for k, v in r.items()}


def same_bytes(got, ref, what):
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        if got[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} places, first {bad[:3].tolist()}: got "
                                 f"{got[k][tuple(bad[0])]!r}, want {ref[k][tuple(bad[0])]!r}")


# ---- 1. the clustering ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["grid", "rand", "origin"])
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("n", NS)
def test_cluster_equals_the_restatement(n, order, cfg):
    xyz, cell, lengths, origin = config(cfg, n)
    ref = R.cluster_ref(xyz, cell, order, lengths, origin)
    got = gpu_cluster(xyz, cell, order, lengths, origin)
    same_bytes(got, ref, f"{cfg} n={n} {order}")
    again = gpu_cluster(xyz, cell, order, lengths, origin)
    same_bytes(again, got, "second call")
    if cfg == "origin" and n >= 63:
        assert (ref["coords"][0] < 0).any() and (ref["inside"][1] < n) and ref["inside"][1] > 0  # negative k; cells beyond
    if cfg == "grid" and n >= 63:
        assert ref["nclusters"][0] == n and ref["nclusters"][1] == 1


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("n", [65, 1000])
def test_alone_equals_in_batch_and_ragged_equals_sliced(n, order):
    xyz, cell, lengths, _ = config("rand", n)
    full = gpu_cluster(xyz, cell, order, lengths, None)
    for s in range(xyz.shape[0]):
        L = max(int(lengths[s]), 1)
        alone = gpu_cluster(xyz[s:s + 1], cell, order, lengths[s:s + 1], None)
        same_bytes(alone, {k: full[k][s:s + 1] for k in CLUSTER_KEYS}, f"alone {s}")
        cut = gpu_cluster(xyz[s:s + 1, :L], cell, order, None, None)
        want = {k: full[k][s:s + 1] for k in ("origin", "inside", "nclusters")}
        want.update({k: full[k][s:s + 1, :L] for k in ("order", "cluster", "coords", "code")})
        want["starts"] = full["starts"][s:s + 1, :L + 1]
        same_bytes(cut, want, f"sliced {s}")
        assert (full["cluster"][s, L:] == -1).all() and (full["code"][s, L:] == -1).all()


def test_a_permutation_of_exact_grid_points_changes_nothing():
    from rfnet_amd import _raw
    n, c = 1000, 5
    rng = np.random.RandomState(3)
    xyz = np.stack([family("faces", n, 40 + i) for i in range(3)])
    feat = rng.randint(-1000, 1000, (3, n, c)).astype(F32)  # integers: every sum is exact
    perm = rng.permutation(n)
    outs = []
    for x, f in ((xyz, feat), (xyz[:, perm], feat[:, perm])):
        r = gpu_cluster(x, 1.0 / 16, "hilbert", None, np.zeros((3, 3), F32))
        rows = [_raw.grid_pool(dev(t), dev(r["order"]), dev(r["starts"]), dev(r["nclusters"]), red)
                for t, red in ((x, "mean"), (f, "sum"), (f, "mean"))]
        mx = _raw.grid_pool(dev(f), dev(r["order"]), dev(r["starts"]), dev(r["nclusters"]), "max")[0]
        outs.append([r["coords"], np.diff(r["starts"]), r["nclusters"]] + [t.cpu().numpy() for t in rows + [mx]])
    for a, p in zip(*outs):
        assert a.tobytes() == p.tobytes()


# ---- 2. pool and unpool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_pool_and_unpool_equal_the_restatement(n, c):
    from rfnet_amd import _raw
    k = NS.index(n) + CS.index(c)
    cfg, order = ("grid", "rand", "origin")[k % 3], R.ORDERS[(k // 3) % 3]
    xyz, cell, lengths, origin = config(cfg, n)
    b = xyz.shape[0]
    ref = R.cluster_ref(xyz, cell, order, lengths, origin)
    od, ss, nc, cl = (dev(ref[key]) for key in ("order", "starts", "nclusters", "cluster"))
    rng = np.random.RandomState(100 + k)
    feat = (rng.randn(b, n, c) * 10).astype(F32)
    grad = rng.randn(b, n, c).astype(F32)
    for red in ("sum", "mean"):
        want = R.pool_ref(feat, ref["order"], ref["starts"], ref["nclusters"], red)
        got = _raw.grid_pool(dev(feat), od, ss, nc, red)
        same_bytes({"out": got.cpu().numpy()}, {"out": want}, f"{red} {cfg} n={n} c={c}")
        assert torch.equal(_raw.grid_pool(dev(feat), od, ss, nc, red).view(torch.int32), got.view(torch.int32))
        if red == "sum":  # unpool(pool_sum)
            same_bytes({"dst": _raw.grid_unpool(got, cl).cpu().numpy()}, {"dst": R.unpool_ref(want, ref["cluster"])}, "copy")
    same_bytes({"dst": _raw.grid_unpool(dev(grad), cl, starts=ss, mode="mean").cpu().numpy()},
               {"dst": R.unpool_ref(grad, ref["cluster"], starts=ref["starts"], mode="mean")}, "unpool mean")
    nanf = feat.copy()
    nanf[rng.rand(b, n, c) < 0.1] = np.nan  # NaN features under max
    for f in (feat, nanf):
        want, warg = R.pool_ref(f, ref["order"], ref["starts"], ref["nclusters"], "max")
        got, arg = _raw.grid_pool(dev(f), od, ss, nc, "max")
        same_bytes({"out": got.cpu().numpy(), "arg": arg.cpu().numpy()}, {"out": want, "arg": warg}, f"max {cfg} n={n} c={c}")
    same_bytes({"dst": _raw.grid_unpool(dev(grad), cl, arg=arg, mode="max").cpu().numpy()},
               {"dst": R.unpool_ref(grad, ref["cluster"], arg=warg, mode="max")}, "unpool max")


# ---- 3. glue: forward, every backward, zero gradients where there is no cell --------------------------------------------------
@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("n,c", [(65, 5), (1000, 64)])
def test_glue_forward_and_backward_equal_the_restatement(n, c, reduce):
    from rfnet_amd import glue
    xyz, _, lengths, _ = config("rand", n)
    cell = 0.15  # about three points per cell at n = 1000
    xyz = np.nan_to_num(xyz, nan=0.0)  # (autograd multiplies the padded rows too)
    xyz[2, 3] = 5000.0  # a row beyond +-32768 cells
    b = xyz.shape[0]
    rng = np.random.RandomState(n + c)
    feat, gp, gf = (rng.randn(b, n, c).astype(F32)), rng.randn(b, n, 3).astype(F32), rng.randn(b, n, c).astype(F32)
    ref = R.cluster_ref(xyz, cell, "z", lengths)
    tx, tf = dev(xyz).requires_grad_(), dev(feat).requires_grad_()
    points, pooled, lengths_out, info = glue.grid_pool(tx, cell, tf, reduce=reduce, order="z", lengths=dev(lengths))
    same_bytes({k: info[k].cpu().numpy() for k in CLUSTER_KEYS if k != "code"}, {k: ref[k] for k in CLUSTER_KEYS if k != "code"}, "info")
    assert lengths_out is info["nclusters"] and lengths_out.dtype == torch.int32 and lengths_out.is_cuda
    keys = (ref["order"], ref["starts"], ref["nclusters"])
    want_pts = R.pool_ref(xyz, *keys, "mean")
    want = R.pool_ref(feat, *keys, reduce)
    want, warg = want if reduce == "max" else (want, None)
    same_bytes({"points": points.detach().cpu().numpy(), "pooled": pooled.detach().cpu().numpy()}, {"points": want_pts, "pooled": want}, reduce)
    ((points * dev(gp)).sum() + (pooled * dev(gf)).sum()).backward()
    mode = {"sum": "copy", "mean": "mean", "max": "max"}[reduce]
    want_gx = R.unpool_ref(gp, ref["cluster"], starts=ref["starts"], mode="mean")
    want_gf = R.unpool_ref(gf, ref["cluster"], starts=ref["starts"], arg=warg, mode=mode)
    same_bytes({"grad pcd": tx.grad.cpu().numpy(), "grad feat": tf.grad.cpu().numpy()}, {"grad pcd": want_gx, "grad feat": want_gf}, reduce)
    out = ref["cluster"] < 0  # padded rows and the row outside
    assert out[2, 3] and out[1, 1:].all() and not tx.grad.cpu().numpy()[out].view(np.uint32).any()
    assert not tf.grad.cpu().numpy()[out].view(np.uint32).any()
    # only the gradients that are needed
    p2, f2, _, _ = glue.grid_pool(dev(xyz), cell, tf, reduce=reduce, order="z", lengths=dev(lengths))
    assert not p2.requires_grad and f2.requires_grad and torch.equal(f2, pooled)
    p3, f3, _, _ = glue.grid_pool(dev(xyz), cell, None, order="z", lengths=dev(lengths))
    assert f3 is None and torch.equal(p3, points)


@pytest.mark.parametrize("n,c", [(65, 5), (1000, 64)])
def test_glue_unpool_and_its_backward(n, c):
    from rfnet_amd import glue
    xyz, _, lengths, _ = config("rand", n)
    cell, b = 0.15, xyz.shape[0]
    rng = np.random.RandomState(n)
    src, g = rng.randn(b, n, c).astype(F32), rng.randn(b, n, c).astype(F32)
    ref = R.cluster_ref(xyz, cell, "hilbert", lengths)
    info = glue.grid_cluster(dev(xyz), cell, order="hilbert", lengths=dev(lengths))
    want, want_g = R.unpool_ref(src, ref["cluster"]), R.pool_ref(g, ref["order"], ref["starts"], ref["nclusters"], "sum")
    for args in ((info["cluster"], info["starts"]), (info["cluster"], info["starts"], info["order"], info["nclusters"])):
        t = dev(src).requires_grad_()
        out = glue.grid_unpool(t, *args)
        (out * dev(g)).sum().backward()
        same_bytes({"dst": out.detach().cpu().numpy(), "grad": t.grad.cpu().numpy()}, {"dst": want, "grad": want_g}, str(len(args)))


@pytest.mark.parametrize("order", R.ORDERS)
def test_serialize(order):
    from rfnet_amd import glue
    xyz, cell, lengths, _ = config("rand", 1000)
    xyz[3, 5] = np.inf
    ref = R.cluster_ref(xyz, cell, order, lengths)
    code, od, inv = (t.cpu().numpy() for t in glue.serialize(dev(xyz), cell, order=order, lengths=dev(lengths)))
    assert code.dtype == np.int64 and code.tobytes() == ref["code"].tobytes() and od.tobytes() == ref["order"].tobytes()
    for s in range(xyz.shape[0]):
        I = ref["inside"][s]
        want = np.full(1000, -1, I32)
        want[ref["order"][s, :I]] = np.arange(I)
        assert np.array_equal(inv[s], want)
        assert (np.diff(code[s][od[s, :I]]) >= 0).all()


# ---- 4. no host synchronisation; graph capture ----------------------------------------------------------------------------------
def test_grid_pool_then_fps_without_a_host_sync():
    from rfnet_amd import glue
    from rfnet_amd.tf_ops.sampling.tf_sampling import farthest_point_sample_lengths
    xyz, cell, lengths, _ = config("rand", 1000)
    tx, tl, tf = dev(xyz), dev(lengths), dev(np.random.RandomState(1).randn(5, 1000, 8).astype(F32))

    def run():
        points, pooled, lengths_out, _ = glue.grid_pool(tx, cell, tf, reduce="max", lengths=tl)
        return points, pooled, lengths_out, farthest_point_sample_lengths(16, points, lengths=lengths_out)
    first = run()  # (first use: library load, workspaces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    M = second[2].cpu().numpy()
    idx = second[3].cpu().numpy()
    assert M.tolist() == R.cluster_ref(xyz, cell, "xyz", lengths)["nclusters"].tolist()
    assert all((idx[s] < max(M[s], 1)).all() for s in range(5))  # samples only among the valid rows
    assert len(set(idx[2].tolist())) == 16


def test_graph_capture_with_new_inputs_and_device_counts():
    from rfnet_amd import _raw
    n, c = 1000, 8
    xyz, cell, lengths, _ = config("rand", n)
    xyz = np.nan_to_num(xyz, nan=0.125)  # (other counts below make padded rows valid)
    tx, tl = dev(xyz), dev(lengths)
    tf = dev(np.random.RandomState(2).randn(5, n, c).astype(F32))

    def call():
        r = _raw.grid_cluster(tx, cell, "hilbert", tl, want_code=True)
        out, arg = _raw.grid_pool(tf, r["order"], r["starts"], r["nclusters"], "max")
        mean = _raw.grid_pool(tx, r["order"], r["starts"], r["nclusters"], "mean")
        return [r[k] for k in CLUSTER_KEYS] + [out, arg, mean, _raw.grid_unpool(out, r["cluster"], arg=arg, mode="max")]

    def same(xs, ys):
        return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(xs, ys))
    eager = [t.clone() for t in call()]
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, eager)
    tx.copy_(dev(np.stack([family("cube", n, 77 + i) for i in range(5)])))
    tl.copy_(torch.tensor([700, 3, 64, 1000, 1], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, call()) and not same(out[1:3], eager[1:3])
