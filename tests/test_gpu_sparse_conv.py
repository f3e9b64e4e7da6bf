"""GPU: rf_sparse_conv_map, rf_sparse_conv (both modes) and rf_sparse_conv_grad_weight against the numpy restatement of
tests/sparse_conv_ref.py: the map as bytes, the fp32 results bit for bit after -0 -> +0 and with NaNs as a class (the latitude
the header gives to the realisation of absent slots).  Shapes are the smallest at which a path changes: n in {1, 33, 65, 331,
1000} (one wave with one row, a tile and a row, three waves, three workgroups, the sort's four sizes), 1100 rows for the weight
gradient's second chunk, cin in {1, 3, 5, 64, 256} (odd, below a slab, slabs, the scalar and the 16-byte loads), cout in {1, 7,
33, 64, 256} (one block, two, two passes), ks in {3, 5}, dilation in {1, 2}; a ragged batch with counts 0, 1, 77 and n, NaN
rows and garbage in nbr behind the counts, entries of nbr outside [0, M), a NaN and an inf feature row.  Then the properties:
symmetry of the map, alone equals in-batch, ragged equals sliced, glue and the layer, no host synchronisation, graph capture.

Section 5 repeats the comparisons on the size ladder of tests/sparse_sizes.py, n in {2049, 4097, 8193, 16384} with the counts
[n, n // 2 - 1, n // 4, 77]: each rung is the smallest n at which the shared LDS sort changes (2049: P = 4096, 1024 threads
of 4 words, two-stride passes, and a third chunk of the weight gradient; 4097: P = 8192 under 512 threads of 16 words,
four-stride passes with their r == 3 and r == 1 remainders; 8193: P = 16384 under 1024 threads; 16384: the contract's limit,
row numbers up to 16383 in the map's 16-bit field, V * K lookups of depth 14, 16 chunks), and the ragged counts run the sorts
of 128 ... 8192 words under the launch of the larger one.  The families there: "lattice" (every row live, 92 % of the slots
present at 16384), "spread", "cube" and "one" (n - 1 duplicates) for the map, "lattice" and "cube" for the convolutions with
few channels -- the rows are under test, the channel paths are covered above.  A kernel change that moves a threshold of the
sort, of the chunks or of the row field must keep the rung that reaches it."""
import functools

import numpy as np
import pytest
import torch

import sparse_conv_ref as R
import sparse_sizes as Z
from sparse_conv_ref import F32, F64, I32

pytestmark = pytest.mark.gpu


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def counts_of(n):
    return Z.counts_at(n) if n in Z.SIZES else np.array([0, 1, min(77, n), n], I32)


def full_of(n):
    """the sample that has all n rows"""
    return 0 if n in Z.SIZES else 3


def make_coords(kind, n, seed):
    """(4, n, 3) int32.  "cube": random cells of a small cube (neighbours and duplicates), sample 0 with rows at the edge of the
    range, out of range and a duplicate pair in front; "line": cells along z with gaps (three live slots at most); "lattice",
    "spread" and "one": the families of tests/sparse_sizes.py"""
    if kind in ("lattice", "spread", "one"):
        return Z.family(kind, n, seed)
    rng = np.random.RandomState(seed)
    if kind == "line":
        z = np.cumsum(rng.randint(1, 3, (4, n)), 1)
        return np.stack([np.full((4, n), 5), np.full((4, n), -3), z], -1).astype(I32)
    span = max(2, int(round((2.0 * n) ** (1 / 3) / 2)))  # about two rows per cell of the cube
    c = rng.randint(-span, span, (4, n, 3)).astype(I32)
    for s in range(4):  # the rows the count of 77 (or n) keeps
        if n >= 8:
            c[s, 1] = [40000, 0, 0]
            c[s, 2] = [32767, 32767, -32768]
            c[s, 3] = [32766, 32767, -32768]
            c[s, 4] = [0, -32769, 1]
            c[s, 6] = c[s, 7]
    return c


@functools.lru_cache(maxsize=None)
def case(n, cin, cout, ks, dilation, kind="cube"):
    """inputs and every reference of one shape, computed once"""
    seed = n * 7 + cin * 3 + cout + ks + dilation
    rng = np.random.RandomState(seed)
    K = ks ** 3
    coords, count = make_coords(kind, n, seed), counts_of(n)
    nbr = R.map_ref(coords, count, ks, dilation)
    feat = rng.randn(4, n, cin).astype(F32)
    gout = rng.randn(4, n, cout).astype(F32)
    weight = (rng.randn(K, cin, cout) / np.sqrt(cin)).astype(F32)
    if n >= 33:  # a NaN and an inf row among the live rows of the full sample
        full = full_of(n)
        feat[full, 0], feat[full, 9, 0] = np.nan, np.inf
        gout[full, 5] = np.nan
    hostile = nbr.copy()  # what the convolution must ignore: garbage behind the counts and outside [0, M) in absent slots
    for s in range(4):
        M = int(count[s])
        feat[s, M:], gout[s, M:] = np.nan, np.nan
        hostile[s, M:] = rng.randint(-5, n + 5, (n - M, K))
        hole = hostile[s, :M] == -1
        hostile[s, :M][hole] = rng.choice([-1, -2, M, n, n + 3, 1 << 30, -(1 << 31)], int(hole.sum()))
    return dict(coords=coords, count=count, nbr=nbr, hostile=hostile, feat=feat, gout=gout, weight=weight,
                out=R.conv_ref(feat, weight, nbr, count), gfeat=R.grad_input_ref(gout, weight, nbr, count),
                gweight=R.grad_weight_ref(feat, gout, nbr, count))


def assert_same(got, want, what):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not R.same_bits(got, want):
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: differs at {len(bad)} places, first {bad[:3].tolist()}: got {got[tuple(bad[0])]!r}, "
                             f"want {want[tuple(bad[0])]!r}")


# ---- 1. the map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ks,dilation", [(1, 3, 1), (33, 5, 1), (65, 3, 2), (331, 5, 2), (331, 3, 1), (1000, 3, 1)])
def test_map_equals_the_restatement(n, ks, dilation):
    from rfnet_amd import _raw
    coords, count = make_coords("cube", n, n + ks), counts_of(n)
    for cnt in (count, None):
        want = R.map_ref(coords, cnt, ks, dilation)
        got = host(_raw.sparse_conv_map(dev(coords), dev(cnt), ks, dilation))
        assert got.dtype == I32 and got.tobytes() == want.tobytes(), (n, ks, dilation, cnt is None)
    again = host(_raw.sparse_conv_map(dev(coords), None, ks, dilation))
    assert again.tobytes() == got.tobytes()  # two calls, the same bytes
    # the symmetry, on what the GPU returned
    K = ks ** 3
    live = R.live_rows(coords)
    assert (got[~live] == -1).all()
    for s in range(4):
        i, t = np.nonzero(got[s] >= 0)
        assert np.array_equal(got[s, got[s, i, t], K - 1 - t], i)


def test_map_of_a_full_block_and_of_isolated_cells():
    from rfnet_amd import _raw
    blk = (R.offsets(5, 1) + np.array([32767 - 2, -32768 + 2, 7])).astype(I32)  # a 5^3 block in a corner of the range
    iso = (np.arange(125)[:, None] * np.array([11, -13, 17])).astype(I32)   # no two within 2 * 2 cells
    coords = np.stack([blk, iso, blk[::-1], iso])
    for ks, dilation in ((5, 1), (3, 2)):
        got = host(_raw.sparse_conv_map(dev(coords), None, ks, dilation))
        assert got.tobytes() == R.map_ref(coords, None, ks, dilation).tobytes()
        K = ks ** 3
        assert np.array_equal(got[1, :, (K - 1) // 2], np.arange(125)) and (np.delete(got[1], (K - 1) // 2, 1) == -1).all()
    full = host(_raw.sparse_conv_map(dev(coords), None, 5, 1))
    assert np.array_equal(full[0, 62], np.arange(125)) and np.array_equal(full[2, 62], np.arange(125)[::-1])


@pytest.mark.parametrize("order", ["xyz", "z", "hilbert"])
def test_map_of_grid_cluster_coords_in_every_order(order):
    from rfnet_amd import _raw
    rng = np.random.RandomState(5)
    xyz = rng.rand(3, 331, 3).astype(F32)
    info = _raw.grid_cluster(dev(xyz), 0.11, order, dev(np.array([331, 77, 1], I32)))
    coords, ncl = host(info["coords"]), host(info["nclusters"])
    assert ncl[0] > 100
    got = host(_raw.sparse_conv_map(info["coords"], info["nclusters"], 3, 1))
    assert got.tobytes() == R.map_ref(coords, ncl, 3, 1).tobytes() and (got[0, :ncl[0], 13] == np.arange(ncl[0])).all()
    coarse = info["coords"] >> 1  # a coarser level: duplicates, the first of each cell is the live one
    got = host(_raw.sparse_conv_map(coarse, info["nclusters"], 3, 1))
    want = R.map_ref(host(coarse), ncl, 3, 1)
    assert got.tobytes() == want.tobytes() and (want[0, :ncl[0], 13] == -1).any()


# ---- 2. the convolution and its two gradients -----------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 3, 1, "cube"), (33, 3, 7, 3, 1, "cube"), (65, 5, 33, 3, 2, "cube"), (65, 64, 64, 3, 1, "cube"),
          (33, 64, 1, 5, 1, "cube"), (331, 5, 33, 5, 2, "cube"), (331, 4, 8, 3, 1, "cube"), (1000, 3, 7, 3, 1, "cube"),
          (1100, 3, 5, 3, 1, "line"), (33, 256, 256, 3, 1, "line")]


@pytest.mark.parametrize("n,cin,cout,ks,dilation,kind", SHAPES)
def test_conv_and_gradients_equal_the_restatement(n, cin, cout, ks, dilation, kind):
    from rfnet_amd import _raw
    c = case(n, cin, cout, ks, dilation, kind)
    conv_and_gradients(c, f"n={n} {cin}->{cout} ks={ks} d={dilation}", {name: dev(c[name]) for name in ("nbr", "hostile")})


def conv_and_gradients(c, what, maps):
    """forward, grad_input and grad_weight of a case under every map of `maps` (name -> device nbr), against its references"""
    from rfnet_amd import _raw
    n, full = c["feat"].shape[1], full_of(c["feat"].shape[1])
    cnt, feat, gout, weight = dev(c["count"]), dev(c["feat"]), dev(c["gout"]), dev(c["weight"])
    for name, nbr in maps.items():
        out = _raw.sparse_conv(feat, weight, nbr, cnt)
        assert_same(host(out), c["out"], f"forward {what} {name}")
        assert torch.equal(_raw.sparse_conv(feat, weight, nbr, cnt).view(torch.int32), out.view(torch.int32))
        gf = _raw.sparse_conv(gout, weight, nbr, cnt, "grad_input")
        assert_same(host(gf), c["gfeat"], f"grad_feat {what} {name}")
        gw = _raw.sparse_conv_grad_weight(feat, gout, nbr, cnt)
        assert_same(host(gw), c["gweight"], f"grad_weight {what} {name}")
        assert torch.equal(_raw.sparse_conv_grad_weight(feat, gout, nbr, cnt).view(torch.int32), gw.view(torch.int32))
    for s in range(4):  # rows behind the counts: +0 (zeros of either sign pass assert_same; these are the prescribed +0)
        M = int(c["count"][s])
        assert not host(out)[s, M:].view(np.uint32).any() and not host(gf)[s, M:].view(np.uint32).any()
    if n >= 33:  # the NaN row 0 and the inf row 9 of the full sample reach exactly the rows that name them
        named = (c["nbr"][full] == 0).any(1) | (c["nbr"][full] == 9).any(1)
        bad = ~np.isfinite(host(out)[full]).all(1)
        assert named[0] and np.array_equal(bad, named)


def test_alone_equals_in_batch_and_ragged_equals_sliced():
    alone_and_sliced(case(65, 5, 33, 3, 2), 3, 2, range(4))


def alone_and_sliced(c, ks, dilation, sliced):
    """every sample of a case alone, and the samples of `sliced` cut to their counts with no counts given"""
    from rfnet_amd import _raw
    weight = dev(c["weight"])
    for s in range(4):
        M = int(c["count"][s])
        one = slice(s, s + 1)
        cnt = dev(c["count"][one])
        nbr = _raw.sparse_conv_map(dev(c["coords"][one]), cnt, ks, dilation)
        assert host(nbr).tobytes() == c["nbr"][one].tobytes()
        assert_same(host(_raw.sparse_conv(dev(c["feat"][one]), weight, nbr, cnt)), c["out"][one], f"alone {s}")
        assert_same(host(_raw.sparse_conv(dev(c["gout"][one]), weight, nbr, cnt, "grad_input")), c["gfeat"][one], f"alone {s}")
        if M == 0 or s not in sliced:
            continue
        cut = _raw.sparse_conv_map(dev(c["coords"][one, :M]), None, ks, dilation)
        assert host(cut).tobytes() == c["nbr"][one, :M].tobytes()
        assert_same(host(_raw.sparse_conv(dev(c["feat"][one, :M]), weight, cut)), c["out"][one, :M], f"sliced {s}")
        assert_same(host(_raw.sparse_conv(dev(c["gout"][one, :M]), weight, cut, None, "grad_input")), c["gfeat"][one, :M], f"sliced {s}")


# ---- 3. glue and the layer ----------------------------------------------------------------------------------------------------
def test_glue_forward_and_backward_equal_the_restatement():
    from rfnet_amd import glue
    c = case(331, 4, 8, 3, 1)
    feat, gout = np.nan_to_num(c["feat"], nan=0.25, posinf=2.0), np.nan_to_num(c["gout"], nan=-0.5)  # (autograd multiplies padded rows)
    tf, tw = dev(feat).requires_grad_(), dev(c["weight"]).requires_grad_()
    cnt = dev(c["count"])
    nbr = glue.sparse_conv_map(dev(c["coords"]), cnt, 3, 1)
    assert host(nbr).tobytes() == c["nbr"].tobytes()
    out = glue.sparse_conv(tf, tw, nbr, cnt)
    assert_same(host(out), R.conv_ref(feat, c["weight"], c["nbr"], c["count"]), "glue forward")
    out.backward(dev(gout))
    assert_same(host(tf.grad), R.grad_input_ref(gout, c["weight"], c["nbr"], c["count"]), "glue grad feat")
    assert_same(host(tw.grad), R.grad_weight_ref(feat, gout, c["nbr"], c["count"]), "glue grad weight")
    # only the gradients that are needed
    o2 = glue.sparse_conv(dev(feat), tw, nbr, cnt)
    tw.grad = None
    o2.backward(dev(gout))
    assert_same(host(tw.grad), R.grad_weight_ref(feat, gout, c["nbr"], c["count"]), "weight only")
    tf.grad = None
    glue.sparse_conv(tf, dev(c["weight"]), nbr, cnt).backward(dev(gout))
    assert tf.grad is not None and not glue.sparse_conv(dev(feat), dev(c["weight"]), nbr, cnt).requires_grad


def gamma(L):
    u = 2.0 ** -24
    return L * u / (1 - L * u)


def test_layer_within_the_chain_bound_of_float64_im2col():
    """SubMConv3d against feat_pad[nbr] @ weight in float64.  A row's chain has (live slots) * cin fmaf steps: the error is at
    most gamma_L * sum |terms| (one rounding per step, from +0), plus one rounding of |out + bias| for the bias added by torch."""
    from rfnet_amd import glue
    torch.manual_seed(3)
    c = case(331, 4, 8, 3, 1)
    feat = np.nan_to_num(c["feat"], nan=0.25, posinf=2.0)
    layer = glue.SubMConv3d(4, 8).cuda()
    cnt = dev(c["count"])
    out = host(layer(dev(feat), dev(c["coords"]), cnt))
    assert_same(host(layer(dev(feat), dev(c["nbr"]), cnt)), out, "coords or nbr")
    w, bias = host(layer.weight).astype(F64), host(layer.bias).astype(F64)
    M = c["count"][:, None, None]
    use = (np.arange(331)[None, :, None] < M) & (c["nbr"] >= 0)
    pad = np.concatenate([feat, np.zeros((4, 1, 4), F32)], 1).astype(F64)
    col = pad[np.arange(4)[:, None, None], np.where(use, c["nbr"], 331)]
    exact = np.einsum("bnkc,kco->bno", col, w)
    mag = np.einsum("bnkc,kco->bno", np.abs(col), np.abs(w))
    rows = (np.arange(331)[None, :] < c["count"][:, None])[:, :, None]
    bound = gamma(use.sum(2) * 4 + 1)[:, :, None] * mag + 2.0 ** -24 * (np.abs(exact + bias) + mag * 1e-5) * rows
    err = np.abs(out.astype(F64) - (exact + bias * rows))
    assert (err <= bound).all() and err.max() > 0
    assert not out[0].view(np.uint32).any() and not out[2, 77:].view(np.uint32).any()  # rows behind a count: no bias either


# ---- 4. no host synchronisation; graph capture ----------------------------------------------------------------------------------
def test_cluster_map_conv_unpool_without_a_host_sync():
    from rfnet_amd import glue
    rng = np.random.RandomState(8)
    xyz, feat = dev(rng.rand(3, 331, 3).astype(F32)), dev(rng.randn(3, 331, 4).astype(F32))
    lengths = dev(np.array([331, 77, 1], I32))
    weight = dev((rng.randn(27, 4, 8) / 2).astype(F32))

    def run():
        points, pooled, ncl, info = glue.grid_pool(xyz, 0.11, feat, reduce="mean", order="z", lengths=lengths)
        nbr = glue.sparse_conv_map(info["coords"], ncl, 3, 1)
        out = glue.sparse_conv(pooled, weight, nbr, ncl)
        return nbr, out, glue.grid_unpool(out, info["cluster"], info["starts"], info["order"], ncl), info["coords"], ncl
    first = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    nbr, out, back, coords, ncl = (host(t) for t in second)
    assert nbr.tobytes() == R.map_ref(coords, ncl, 3, 1).tobytes()
    pooled = host(glue.grid_pool(xyz, 0.11, feat, reduce="mean", order="z", lengths=lengths)[1])
    assert_same(out, R.conv_ref(pooled, host(weight), nbr, ncl), "pipeline")
    assert back.shape == (3, 331, 8) and np.abs(back[0]).max() > 0 and not back[1, 77:].any()


def test_graph_capture_with_new_inputs_and_device_counts():
    from rfnet_amd import _raw
    c = case(331, 4, 8, 3, 1)
    feat, gout = np.nan_to_num(c["feat"], nan=0.25, posinf=2.0), np.nan_to_num(c["gout"], nan=-0.5)
    tc, tn, tf, tg, tw = dev(c["coords"]), dev(c["count"]), dev(feat), dev(gout), dev(c["weight"])

    def call():
        nbr = _raw.sparse_conv_map(tc, tn, 3, 1)
        return [nbr, _raw.sparse_conv(tf, tw, nbr, tn), _raw.sparse_conv(tg, tw, nbr, tn, "grad_input"),
                _raw.sparse_conv_grad_weight(tf, tg, nbr, tn)]

    def same(xs, ys):
        return all(host(x).tobytes() == host(y).tobytes() for x, y in zip(xs, ys))
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
    tc.copy_(dev(make_coords("cube", 331, 99)))
    tn.copy_(torch.tensor([331, 200, 3, 0], dtype=torch.int32))
    tf.copy_(dev(np.random.RandomState(4).randn(4, 331, 4).astype(F32)))
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, call()) and not same(out[:2], eager[:2])
    assert host(out[0]).tobytes() == R.map_ref(host(tc), host(tn), 3, 1).tobytes()


# ---- 5. the size ladder: 2049, 4097, 8193 and 16384 rows, counts [n, n // 2 - 1, n // 4, 77] -------------------------------------
def same_ints(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: differs at {len(bad)} places, first {bad[:3].tolist()}: got {got[tuple(bad[0])]!r}, "
                             f"want {want[tuple(bad[0])]!r}")


def family_is_alive(kind, coords, count):
    """a family that has quietly degenerated must not turn a case into a no-op"""
    live = R.live_rows(coords, count).sum(1)
    if kind in ("lattice", "spread"):
        assert np.array_equal(live, count), kind  # every row live
    elif kind == "one":
        assert (live == 1).all()
    else:  # "cube": about one row in five repeats an earlier one
        assert 0.1 * count[0] < count[0] - live[0] < 0.3 * count[0], (kind, live)


@pytest.mark.parametrize("kind", Z.FAMILIES)
@pytest.mark.parametrize("n", Z.SIZES)
def test_map_at_size_equals_the_restatement(n, kind):
    from rfnet_amd import _raw
    coords, count = make_coords(kind, n, n + 11), counts_of(n)
    family_is_alive(kind, coords, count)
    tc = dev(coords)
    for ks, dilation in ((3, 1), (5, 2)):
        K = ks ** 3
        for cnt in (count, None):
            want = R.map_ref(coords, cnt, ks, dilation)
            got = host(_raw.sparse_conv_map(tc, dev(cnt), ks, dilation))
            same_ints(got, want, f"{kind} n={n} ks={ks} d={dilation} counts={cnt is not None}")
            again = host(_raw.sparse_conv_map(tc, dev(cnt), ks, dilation))
            assert again.tobytes() == got.tobytes()  # two calls, the same bytes
        if kind == "lattice" and n == 16384 and ks == 3:
            assert (got[0] >= 0).mean() > 0.9  # a dense block: 92 % of the slots are present
        live = R.live_rows(coords)  # the symmetry, on what the GPU returned (all rows)
        assert (got[~live] == -1).all()
        for s in range(4):
            i, t = np.nonzero(got[s] >= 0)
            assert len(i) >= live[s].sum() and np.array_equal(got[s, got[s, i, t], K - 1 - t], i)


# (3 -> 33 on the "lattice" of 16384 rows is left out: its three references take 12 s on the CPU, the "cube" there takes 7 s)
AT_SIZE = [(n, cin, cout, kind) for n in Z.SIZES for cin, cout in ((3, 5), (4, 8), (3, 33)) for kind in ("lattice", "cube")
           if (n, cout, kind) != (16384, 33, "lattice")]


@pytest.mark.parametrize("n,cin,cout,kind", AT_SIZE)
def test_conv_and_gradients_at_size_equal_the_restatement(n, cin, cout, kind):
    """cin = 3: scalar loads, cin = 4: 16-byte loads, cout = 33: two output blocks.  Under the restatement's map, the hostile
    one and the map the GPU made of the same coordinates: the composition is what runs at size, and when it fails the first two
    say whether the map or the convolution did."""
    from rfnet_amd import _raw
    c = case(n, cin, cout, 3, 1, kind)
    family_is_alive(kind, c["coords"], c["count"])
    assert (c["nbr"][0, :, 13] >= 0).sum() > n // 2 and (kind == "cube" or c["nbr"][0, -1, 13] == n - 1)  # (the last chunk's row)
    maps = {name: dev(c[name]) for name in ("nbr", "hostile")}
    maps["gpu map"] = _raw.sparse_conv_map(dev(c["coords"]), dev(c["count"]), 3, 1)
    conv_and_gradients(c, f"n={n} {cin}->{cout} {kind}", maps)


@pytest.mark.parametrize("n", [8193, 16384])
def test_alone_equals_in_batch_and_ragged_equals_sliced_at_size(n):
    """sample 1 has n // 2 - 1 rows: sliced, it is sorted under its own launch; in the batch, under the launch of n rows"""
    alone_and_sliced(case(n, 3, 5, 3, 1, "lattice"), 3, 1, (1,))
