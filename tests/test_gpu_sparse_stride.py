"""GPU: rf_sparse_stride_map, rf_sparse_conv_strided (four modes) and rf_sparse_conv_strided_grad_weight (both modes) against
the numpy restatement of tests/sparse_stride_ref.py: the int outputs as bytes, the fp32 results bit for bit after -0 -> +0 and
with NaNs as a class.  Shapes are the smallest at which a path changes: n in {1, 33, 65, 331, 1000} for the map (the sort's
sizes, one wave of the scan and several); for the convolutions one row, a tile of 32 coarse rows and one more ("iso": every
fine row its own coarse cell), a workgroup of 128 and one more, odd widths, a second block of 32 output channels, full slabs,
a second pass of 64 output channels with a second reduction slab, and more than 1024 coarse rows for the weight gradient's
second chunk; a ragged batch with counts 0, 1, 77 and n, NaN rows and garbage in child / up behind the counts and in the
absent entries, a truncating n_coarse.  Then the properties: alone equals in-batch, ragged equals sliced, glue and the layers,
an encoder / decoder chain without a host synchronisation and under graph capture.

Section 5 repeats the comparisons on the size ladder of tests/sparse_sizes.py, n in {2049, 4097, 8193, 16384} with the counts
[n, n // 2 - 1, n // 4, 77]: each rung is the smallest n at which the shared LDS sort changes (2049: P = 4096, 1024 threads
of 4 words, two-stride passes; 4097: P = 8192 under 512 threads of 16 words, four-stride passes with their r == 3 and r == 1
remainders, and the map's head scan walks 16 steps over its two-deep totals; 8193: P = 16384 under 1024 threads, 16 steps
with all 16 waves; 16384: the contract's limit), and the ragged counts run the sorts of 128 ... 8192 words under the launch of
the larger one.  The families there: "spread" (every row alone in its coarse cell: n_coarse = n, at 16384 the fan-out form's
512 tiles of 32 coarse rows beside its 128 workgroups of fine rows, and 16 chunks of 1024 coarse rows in the weight
gradients), "lattice" (eight children per coarse cell), "cube" and "one" for the map.  A kernel change that moves a threshold
of the sort, of the scan, of the tiles or of the chunks must keep the rung that reaches it."""
import functools

import numpy as np
import pytest
import torch

import sparse_conv_ref as C
import sparse_sizes as Z
import sparse_stride_ref as R
from sparse_stride_ref import F32, I32

pytestmark = pytest.mark.gpu

MODES = {"down": R.DOWN, "up": R.UP, "down_grad_input": R.DOWN_GRAD_INPUT, "up_grad_input": R.UP_GRAD_INPUT}


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
    """(4, n, 3) int32.  "cube": random cells of a small cube round the origin (negative coordinates, several children per coarse
    cell, duplicates), every sample with rows at the edges of the range, out of range and a duplicate pair in front; "iso":
    every row a coarse cell of its own; "pairs": distinct cells, about two to a coarse cell, in a shuffled order; "lattice",
    "spread" and "one": the families of tests/sparse_sizes.py ("iso" leaves the range above 4681 rows)"""
    if kind in ("lattice", "spread", "one"):
        return Z.family(kind, n, seed)
    rng = np.random.RandomState(seed)
    if kind == "iso":
        i = np.stack([rng.permutation(n) for _ in range(4)])[..., None]
        return (i * np.array([3, -5, 7]) + rng.randint(0, 2, (4, n, 3))).astype(I32)
    if kind == "pairs":
        i = np.stack([rng.permutation(n) for _ in range(4)])
        return np.stack([i - n // 2, (i * 7) % 3, -((i >> 1) % 2)], -1).astype(I32)
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


def same_map(got, want):
    return all(got[k].dtype == I32 and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes() for k in want)


def gpu_map(coords, count=None, nc=None):
    from rfnet_amd import _raw
    return dict(zip(("coords", "count", "total", "child", "up"), (host(t) for t in _raw.sparse_stride_map(dev(coords), dev(count), nc))))


def hostile_maps(m, count, n, rng):
    """what the convolutions must ignore: garbage behind the counts, entries outside [0, M) in the absent slots of child,
    claims that child does not confirm in the dead rows of up"""
    child, up = m["child"].copy(), m["up"].copy()
    nc = child.shape[1]
    for s in range(len(count)):
        M, Mc = int(count[s]), int(m["count"][s])
        child[s, Mc:] = rng.randint(-5, n + 5, (nc - Mc, 8))
        hole = child[s, :Mc] == -1
        child[s, :Mc][hole] = rng.choice([-1, -2, M, n, n + 3, 1 << 30, -(1 << 31)], int(hole.sum()))
        up[s, M:] = rng.randint(-5, 8 * nc + 9, n - M)
        dead = up[s, :M] == -1
        up[s, :M][dead] = rng.choice([-1, -9, 8 * Mc, 8 * nc + 5, 1 << 30, -(1 << 31), 0, 9], int(dead.sum()))
    return child, up


@functools.lru_cache(maxsize=None)
def case(n, cin, cout, kind="cube", nc=None):
    """inputs and every reference of one shape, computed once"""
    seed = n * 7 + cin * 3 + cout + (nc or 0)
    rng = np.random.RandomState(seed)
    coords, count = make_coords(kind, n, seed), counts_of(n)
    m = R.map_ref(coords, count, nc)
    nc = m["child"].shape[1]
    fine_in, coarse_in = rng.randn(4, n, cin).astype(F32), rng.randn(4, nc, cin).astype(F32)
    fine_g, coarse_g = rng.randn(4, n, cout).astype(F32), rng.randn(4, nc, cout).astype(F32)
    weight = (rng.randn(8, cin, cout) / np.sqrt(cin)).astype(F32)
    if n >= 33:  # a NaN and an inf row among the live rows of the full sample
        full = full_of(n)
        fine_in[full, 0], fine_in[full, 9, 0] = np.nan, np.inf
        coarse_in[full, 0] = np.nan
    for s in range(4):
        M, Mc = int(count[s]), int(m["count"][s])
        fine_in[s, M:], fine_g[s, M:] = np.nan, np.nan
        coarse_in[s, Mc:], coarse_g[s, Mc:] = np.nan, np.nan
    hchild, hup = hostile_maps(m, count, n, rng)
    a = (m["child"], m["up"], n, count, m["count"])
    return dict(coords=coords, count=count, m=m, hchild=hchild, hup=hup, weight=weight,
                src=dict(down=fine_in, up=coarse_in, down_grad_input=coarse_g, up_grad_input=fine_g),
                out={k: R.conv_ref(v, dict(down=fine_in, up=coarse_in, down_grad_input=coarse_g, up_grad_input=fine_g)[k], weight, *a)
                     for k, v in MODES.items()},
                gw=dict(down=R.grad_weight_ref(R.DOWN, fine_in, coarse_g, m["child"], count, m["count"]),
                        up=R.grad_weight_ref(R.UP, fine_g, coarse_in, m["child"], count, m["count"])))


def assert_same(got, want, what):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not R.same_bits(got, want):
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: differs at {len(bad)} places, first {bad[:3].tolist()}: got {got[tuple(bad[0])]!r}, "
                             f"want {want[tuple(bad[0])]!r}")


# ---- 1. the map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(1, "cube"), (33, "iso"), (65, "cube"), (331, "cube"), (331, "pairs"), (1000, "cube")])
def test_map_equals_the_restatement(n, kind):
    coords, count = make_coords(kind, n, n + 2), counts_of(n)
    D = int(R.map_ref(coords)["total"].max())
    for nc in sorted({n, max(1, D // 3), min(n, D + 1), 1}):  # all rows; truncating; just enough
        for cnt in (count, None):
            want, got = R.map_ref(coords, cnt, nc), gpu_map(coords, cnt, nc)
            assert same_map(got, want), (n, kind, nc, cnt is None)
    assert same_map(gpu_map(coords, None, n), got)  # two calls, the same bytes (the last size is n)
    # up and child are inverse, on what the GPU returned at full size
    got = gpu_map(coords, count, n)
    live = R.live_rows(coords, count)
    for s in range(4):
        up, child = got["up"][s], got["child"][s]
        i = np.nonzero(up >= 0)[0]
        assert np.array_equal(i, np.nonzero(live[s])[0]) and np.array_equal(child[up[i] >> 3, up[i] & 7], i)


def test_map_of_a_full_block_and_of_isolated_cells():
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    blk = (g + np.array([32764, -32768, -4])).astype(I32)  # a 4^3 block in a corner of the range: 8 coarse cells of 8 children
    iso = (np.arange(64)[:, None] * np.array([11, -13, 17])).astype(I32)
    coords = np.stack([blk, iso, blk[::-1], iso[::-1]])
    got = gpu_map(coords)
    assert same_map(got, R.map_ref(coords))
    assert got["count"].tolist() == [8, 64, 8, 64] and (got["child"][0, :8] >= 0).all() and (got["child"][0, 8:] == -1).all()
    assert np.array_equal(got["child"][2, :8], 63 - got["child"][0, :8])
    assert ((got["child"][1] >= 0).sum(1) == 1).all() and np.array_equal(np.sort(got["up"][1] >> 3), np.arange(64))
    nxt = gpu_map(got["coords"], got["count"])  # the level goes into the next one as it is
    assert same_map(nxt, R.map_ref(got["coords"], got["count"])) and nxt["count"][0] == 1 and (nxt["child"][0, 0] == np.arange(8)).all()


@pytest.mark.parametrize("order", ["xyz", "z", "hilbert"])
def test_map_of_grid_cluster_coords_in_every_order(order):
    from rfnet_amd import _raw
    rng = np.random.RandomState(5)
    xyz = rng.rand(3, 331, 3).astype(F32)
    info = _raw.grid_cluster(dev(xyz), 0.11, order, dev(np.array([331, 77, 1], I32)))
    coords, ncl = host(info["coords"]), host(info["nclusters"])
    assert ncl[0] > 100
    got = dict(zip(("coords", "count", "total", "child", "up"), (host(t) for t in _raw.sparse_stride_map(info["coords"], info["nclusters"]))))
    assert same_map(got, R.map_ref(coords, ncl))
    assert 0 < got["count"][0] < ncl[0] and ((got["child"][0] >= 0).sum(1) > 1).any()
    if order == "xyz":  # the coarse cells are grid_cluster's at twice the edge (powers of two: the same floors), in its order
        lengths = dev(np.array([331, 77, 1], I32))
        fine = _raw.grid_cluster(dev(xyz), 0.125, "xyz", lengths)
        twice = _raw.grid_cluster(dev(xyz), 0.25, "xyz", lengths, fine["origin"])
        co, cn = (host(t) for t in _raw.sparse_stride_map(fine["coords"], fine["nclusters"])[:2])
        assert np.array_equal(host(twice["coords"]), co) and np.array_equal(host(twice["nclusters"]), cn) and cn[0] > 8


# ---- 2. the four modes and both weight gradients ---------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, "cube", None), (33, 3, 7, "iso", None), (129, 5, 33, "iso", None), (129, 5, 33, "cube", 20),
          (65, 64, 64, "cube", None), (65, 36, 96, "iso", None), (2100, 4, 4, "pairs", None)]


@pytest.mark.parametrize("n,cin,cout,kind,nc", SHAPES)
def test_modes_and_weight_gradients_equal_the_restatement(n, cin, cout, kind, nc):
    c = case(n, cin, cout, kind, nc)
    m = c["m"]
    if n == 2100:
        assert m["count"][3] > R.WGRAD_ROWS  # the weight gradient's second chunk
    if nc is not None:
        assert m["total"][3] > nc
    maps = {"maps": (dev(m["child"]), dev(m["up"])), "hostile": (dev(c["hchild"]), dev(c["hup"]))}
    modes_and_weight_gradients(c, f"n={n} {cin}->{cout} {kind} nc={nc}", maps, nc is not None)


def modes_and_weight_gradients(c, what, maps, truncated):
    """the four modes and both weight gradients of a case under every pair of `maps` (name -> device child, up), against its
    references"""
    from rfnet_amd import _raw
    m, n, full = c["m"], c["coords"].shape[1], full_of(c["coords"].shape[1])
    cnt, cntc, weight = dev(c["count"]), dev(m["count"]), dev(c["weight"])
    src = {k: dev(v) for k, v in c["src"].items()}
    for name, (child, up) in maps.items():
        out = {}
        for mode in MODES:
            out[mode] = _raw.sparse_conv_strided(src[mode], weight, child, up, cnt, cntc, mode)
            assert_same(host(out[mode]), c["out"][mode], f"{mode} {what} {name}")
            again = _raw.sparse_conv_strided(src[mode], weight, child, up, cnt, cntc, mode)
            assert torch.equal(again.view(torch.int32), out[mode].view(torch.int32))
        gwd = _raw.sparse_conv_strided_grad_weight(src["down"], src["down_grad_input"], child, cnt, cntc, "down")
        assert_same(host(gwd), c["gw"]["down"], f"grad_weight down {what} {name}")
        gwu = _raw.sparse_conv_strided_grad_weight(src["up_grad_input"], src["up"], child, cnt, cntc, "up")
        assert_same(host(gwu), c["gw"]["up"], f"grad_weight up {what} {name}")
        assert torch.equal(_raw.sparse_conv_strided_grad_weight(src["down"], src["down_grad_input"], child, cnt, cntc, "down").view(torch.int32),
                           gwd.view(torch.int32))
    for s in range(4):  # rows behind the counts, and fine rows that are not served: the prescribed +0
        M, Mc = int(c["count"][s]), int(m["count"][s])
        for mode in ("down", "up_grad_input"):
            assert not host(out[mode])[s, Mc:].view(np.uint32).any()
        for mode in ("up", "down_grad_input"):
            assert not host(out[mode])[s][m["up"][s] < 0].view(np.uint32).any()
    if n >= 33:  # the NaN row 0 and the inf row 9 of the full sample reach exactly the coarse rows that hold them
        named = np.isin(m["child"][full], [0, 9]).any(1) & (np.arange(m["child"].shape[1]) < m["count"][full])
        assert np.array_equal(~np.isfinite(host(out["down"])[full]).all(1), named) and (named.any() or truncated)
        kids = m["child"][full, 0][m["child"][full, 0] >= 0]  # the NaN coarse row 0 reaches exactly its children
        assert np.array_equal(np.nonzero(~np.isfinite(host(out["up"])[full]).all(1))[0], np.sort(kids))


def test_alone_equals_in_batch_and_ragged_equals_sliced():
    alone_and_sliced(case(129, 5, 33, "iso"), range(4))


def alone_and_sliced(c, sliced):
    """every sample of a case alone, and the samples of `sliced` cut to their counts with no counts given"""
    from rfnet_amd import _raw
    m, weight = c["m"], dev(c["weight"])
    for s in range(4):
        M, Mc = int(c["count"][s]), int(m["count"][s])
        one = slice(s, s + 1)
        alone = gpu_map(c["coords"][one], c["count"][one])
        assert same_map(alone, {k: v[one] for k, v in m.items()})
        cnt, cntc, child, up = dev(c["count"][one]), dev(alone["count"]), dev(alone["child"]), dev(alone["up"])
        for mode in MODES:
            got = _raw.sparse_conv_strided(dev(c["src"][mode][one]), weight, child, up, cnt, cntc, mode)
            assert_same(host(got), c["out"][mode][one], f"alone {s} {mode}")
        if M == 0 or s not in sliced:
            continue
        cut = gpu_map(c["coords"][one, :M])  # no counts: n = M rows, n_coarse = M
        assert cut["count"][0] == Mc and same_map({k: cut[k] for k in ("child", "coords")}, {k: m[k][one, :M] for k in ("child", "coords")})
        assert np.array_equal(cut["up"], m["up"][one, :M])
        child, up = dev(cut["child"][:, :Mc]), dev(cut["up"])  # and the coarse rows cut to Mc
        for mode in MODES:
            rows_in, rows_out = (M, Mc) if mode in ("down", "up_grad_input") else (Mc, M)
            got = _raw.sparse_conv_strided(dev(c["src"][mode][one, :rows_in]), weight, child, up, mode=mode)
            assert_same(host(got), c["out"][mode][one, :rows_out], f"sliced {s} {mode}")


# ---- 3. glue and the layers ----------------------------------------------------------------------------------------------------
def test_glue_forward_and_backward_equal_the_restatement():
    from rfnet_amd import glue
    c = case(331, 4, 8, "cube")
    m, w = c["m"], c["weight"]
    clean = {k: np.nan_to_num(v, nan=0.25, posinf=2.0) for k, v in c["src"].items()}  # (autograd multiplies padded rows)
    cnt = dev(c["count"])
    level = glue.sparse_stride_map(dev(c["coords"]), cnt)
    assert same_map({k: host(level[k]) for k in ("coords", "total", "child", "up")}, {k: m[k] for k in ("coords", "total", "child", "up")})
    assert np.array_equal(host(level["nclusters"]), m["count"])
    a = (m["child"], m["up"], 331, c["count"], m["count"])
    for fn, mode, gmode, x, g in ((glue.sparse_conv_down, "down", "down_grad_input", clean["down"], clean["down_grad_input"]),
                                  (glue.sparse_conv_up, "up", "up_grad_input", clean["up"], clean["up_grad_input"])):
        tx, tw = dev(x).requires_grad_(), dev(w).requires_grad_()
        out = fn(tx, tw, level, cnt)
        assert_same(host(out), R.conv_ref(MODES[mode], x, w, *a), f"glue {mode}")
        out.backward(dev(g))
        assert_same(host(tx.grad), R.conv_ref(MODES[gmode], g, w, *a), f"glue {mode} grad feat")
        fine, coarse = (x, g) if mode == "down" else (g, x)
        want_gw = R.grad_weight_ref(MODES[mode], fine, coarse, m["child"], c["count"], m["count"])
        assert_same(host(tw.grad), want_gw, f"glue {mode} grad weight")
        # only the gradients that are needed
        tw.grad = None
        fn(dev(x), tw, level, cnt).backward(dev(g))
        assert_same(host(tw.grad), want_gw, f"{mode}: weight only")
        tx.grad = None
        fn(tx, dev(w), level, cnt).backward(dev(g))
        assert tx.grad is not None and not fn(dev(x), dev(w), level, cnt).requires_grad


def test_layers_add_the_bias_in_front_of_the_counts_only():
    from rfnet_amd import glue
    torch.manual_seed(3)
    c = case(331, 4, 8, "cube")
    m = c["m"]
    x, y = np.nan_to_num(c["src"]["down"], nan=0.25, posinf=2.0), np.nan_to_num(c["src"]["up"], nan=0.25)
    cnt = dev(c["count"])
    a = (m["child"], m["up"], 331, c["count"], m["count"])
    down, up = glue.SparseConv3d(4, 8).cuda(), glue.SparseConvTranspose3d(4, 8).cuda()
    level = glue.sparse_stride_map(dev(c["coords"]), cnt)
    for layer, mode, src, live in ((down, R.DOWN, x, np.arange(331)[None, :] < m["count"][:, None]),
                                   (up, R.UP, y, np.arange(331)[None, :] < c["count"][:, None])):
        out = host(layer(dev(src), dev(c["coords"]), cnt))
        assert_same(host(layer(dev(src), level, cnt)), out, "coords or level")
        want = R.conv_ref(mode, src, host(layer.weight), *a) + live[:, :, None].astype(F32) * host(layer.bias)  # one fp32 add
        assert_same(out, want.astype(F32), f"layer {mode}")
        assert not out[0].view(np.uint32).any() and not out[2, 77:].view(np.uint32).any()  # rows behind a count: no bias either


# ---- 4. an encoder / decoder chain: no host synchronisation; graph capture -------------------------------------------------------
class _UNet(torch.nn.Module):
    def __init__(self):
        from rfnet_amd import glue
        super().__init__()
        self.sub0, self.down = glue.SubMConv3d(4, 8), glue.SparseConv3d(8, 16, bias=False)
        self.sub1, self.up = glue.SubMConv3d(16, 16), glue.SparseConvTranspose3d(16, 8, bias=False)

    def forward(self, xyz, feat, lengths, cell=0.11):
        from rfnet_amd import glue
        points, pooled, ncl, info = glue.grid_pool(xyz, cell, feat, reduce="mean", order="z", lengths=lengths)  # (grid_cluster)
        f0 = self.sub0(pooled, info["coords"], ncl)
        level = glue.sparse_stride_map(info["coords"], ncl)
        d = self.down(f0, level, ncl)
        f1 = self.sub1(d, glue.sparse_conv_map(level["coords"], level["nclusters"]), level["nclusters"])
        u = self.up(f1, level, ncl)
        back = glue.grid_unpool(torch.cat([f0, u], -1), info["cluster"], info["starts"], info["order"], ncl)
        return [info["coords"], ncl, level["coords"], level["nclusters"], level["child"], level["up"], f0, d, f1, u, pooled, back]


def _chain_inputs(seed):
    rng = np.random.RandomState(seed)
    return rng.rand(3, 331, 3).astype(F32), rng.randn(3, 331, 4).astype(F32)


def _check_chain(net, outs, lengths):
    coords, ncl, ccoords, cncl, child, up, f0, d, f1, u, pooled, back = (host(t) for t in outs)
    b, n = up.shape
    m = R.map_ref(coords, ncl)
    assert same_map(dict(coords=ccoords, count=cncl, child=child, up=up), {k: m[k] for k in ("coords", "count", "child", "up")})
    a = (child, up, n, ncl, cncl)
    assert_same(d, R.conv_ref(R.DOWN, f0, host(net.down.weight), *a), "chain down")
    assert_same(u, R.conv_ref(R.UP, f1, host(net.up.weight), *a), "chain up")
    assert back.shape == (b, n, 16) and np.abs(back[0, :, 8:]).max() > 0 and cncl[0] > 32
    assert not any(back[s, L:].any() for s, L in enumerate(lengths))  # points behind a length are in no cell


def _check_chain_submanifold(net, outs):
    """the two submanifold layers of the chain against the restatement of tests/sparse_conv_ref.py on the restatement's own map
    of the coordinates the chain produced, the bias as one fp32 add to the rows in front of the counts"""
    coords, ncl, ccoords, cncl, child, up, f0, d, f1, u, pooled, back = (host(t) for t in outs)
    for layer, src, cells, cnt, got, what in ((net.sub0, pooled, coords, ncl, f0, "chain sub0"), (net.sub1, d, ccoords, cncl, f1, "chain sub1")):
        live = (np.arange(cells.shape[1])[None, :] < cnt[:, None])[:, :, None].astype(F32)
        want = C.conv_ref(src, host(layer.weight), C.map_ref(cells, cnt, 3, 1), cnt) + live * host(layer.bias)
        assert_same(got, want.astype(F32), what)


def test_unet_chain_without_a_host_sync():
    torch.manual_seed(5)
    net = _UNet().cuda()
    xyz, feat = (dev(x) for x in _chain_inputs(8))
    lengths = dev(np.array([331, 77, 1], I32))
    with torch.no_grad():
        first = net(xyz, feat, lengths)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            second = net(xyz, feat, lengths)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    _check_chain(net, second, [331, 77, 1])
    # and it trains: every parameter gets a finite gradient through both strided layers
    net(xyz, feat, lengths)[-1].square().sum().backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_unet_chain_under_graph_capture_with_new_inputs_and_device_counts():
    torch.manual_seed(6)
    net = _UNet().cuda()
    xyz, feat = (dev(x) for x in _chain_inputs(9))
    lengths = dev(np.array([331, 77, 1], I32))

    def same(xs, ys):
        return all(host(x).tobytes() == host(y).tobytes() for x, y in zip(xs, ys))
    with torch.no_grad():
        eager = [t.clone() for t in net(xyz, feat, lengths)]
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            net(xyz, feat, lengths)  # warm-up off the capture
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(xyz, feat, lengths)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, eager)
        nx, nf = _chain_inputs(10)
        xyz.copy_(dev(nx))
        feat.copy_(dev(nf))
        lengths.copy_(torch.tensor([200, 331, 1], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, net(xyz, feat, lengths)) and not same(out[6:], eager[6:])
    ncl = host(out[1])
    assert ncl[2] == 1 and ncl[1] > ncl[0]
    _check_chain(net, out, [200, 331, 1])


# ---- 5. the size ladder: 2049, 4097, 8193 and 16384 rows, counts [n, n // 2 - 1, n // 4, 77] -------------------------------------
def assert_map(got, want, what):
    for k in want:
        assert got[k].dtype == I32 and got[k].shape == want[k].shape, (what, k)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} places, first {bad[:3].tolist()}: got "
                                 f"{got[k][tuple(bad[0])]!r}, want {want[k][tuple(bad[0])]!r}")


def family_is_alive(kind, coords, count, m):
    """a family that has quietly degenerated must not turn a case into a no-op; m is the restatement's map at n_coarse = n"""
    live, n = R.live_rows(coords, count).sum(1), coords.shape[1]
    if kind == "spread":  # every row alone in its coarse cell
        assert np.array_equal(live, count) and np.array_equal(m["count"], count)
    elif kind == "lattice":  # every row live, several children to a coarse cell, all eight at 16384
        assert np.array_equal(live, count) and 8 * m["count"][0] >= count[0] > 1.2 * m["count"][0]
        assert n < 16384 or (m["child"][0, :2048] >= 0).all()
    elif kind == "one":
        assert (live == 1).all() and (m["count"] == 1).all()
    else:  # "cube": about one row in five repeats an earlier one
        assert 0.1 * count[0] < count[0] - live[0] < 0.3 * count[0] and m["count"][0] > n // 8, (kind, live)


@pytest.mark.parametrize("kind", Z.FAMILIES)
@pytest.mark.parametrize("n", Z.SIZES)
def test_map_at_size_equals_the_restatement(n, kind):
    coords, count = make_coords(kind, n, n + 13), counts_of(n)
    whole = R.map_ref(coords, count)
    family_is_alive(kind, coords, count, whole)
    D = int(whole["total"].max())
    for nc in sorted({n, max(1, D // 3), D}):  # all rows; truncating; just enough
        want = whole if nc == n else R.map_ref(coords, count, nc)
        got = gpu_map(coords, count, nc)
        assert_map(got, want, f"{kind} n={n} nc={nc}")
        assert_map(gpu_map(coords, count, nc), got, "second call")  # two calls, the same bytes
    got = gpu_map(coords, None, n)  # and no counts: every sample sorts n rows
    assert_map(got, R.map_ref(coords, None, n), f"{kind} n={n} no counts")
    assert_map(gpu_map(coords, None, n), got, "second call")
    live = R.live_rows(coords)  # up and child are inverse, on what the GPU returned
    for s in range(4):
        up, child = got["up"][s], got["child"][s]
        i = np.nonzero(up >= 0)[0]
        assert np.array_equal(i, np.nonzero(live[s])[0]) and np.array_equal(child[up[i] >> 3, up[i] & 7], i)


AT_SIZE = [(n, cin, cout, kind, None) for n in Z.SIZES for cin, cout in ((3, 5), (4, 8)) for kind in ("spread", "lattice")]
AT_SIZE.append((16384, 3, 5, "lattice", 683))  # a third of the 2048 coarse cells of the full block


@pytest.mark.parametrize("n,cin,cout,kind,nc", AT_SIZE)
def test_modes_and_weight_gradients_at_size_equal_the_restatement(n, cin, cout, kind, nc):
    """cin = 3: scalar loads, cin = 4: 16-byte loads.  Under the restatement's maps, the hostile ones and the maps the GPU made
    of the same coordinates: the composition is what runs at size, and when it fails the first two say whether the map or the
    convolution did."""
    from rfnet_amd import _raw
    c = case(n, cin, cout, kind, nc)
    m = c["m"]
    if nc is None:
        family_is_alive(kind, c["coords"], c["count"], m)
        if kind == "spread":
            assert -(-m["count"][0] // R.WGRAD_ROWS) == -(-n // R.WGRAD_ROWS) >= 3  # the weight gradient's chunks: 3, 5, 9, 16
    else:
        assert m["total"][0] > nc == m["count"][0]
    made = _raw.sparse_stride_map(dev(c["coords"]), dev(c["count"]), nc)
    assert np.array_equal(host(made[1]), m["count"])
    maps = {"maps": (dev(m["child"]), dev(m["up"])), "hostile": (dev(c["hchild"]), dev(c["hup"])), "gpu maps": (made[3], made[4])}
    modes_and_weight_gradients(c, f"n={n} {cin}->{cout} {kind} nc={nc}", maps, nc is not None)


@pytest.mark.parametrize("n", [8193, 16384])
def test_alone_equals_in_batch_and_ragged_equals_sliced_at_size(n):
    """sample 1 has n // 2 - 1 rows: sliced, it is sorted under its own launch; in the batch, under the launch of n rows"""
    alone_and_sliced(case(n, 3, 5, "lattice"), (1,))


def test_unet_chain_at_16384_points_without_a_host_sync():
    """grid_pool -> sparse_conv_map -> SubMConv3d -> sparse_stride_map -> down -> SubMConv3d -> up -> grid_unpool on 16384 random
    points with more than 8192 occupied cells (a sort of 16384 words in every map), each layer against its restatement"""
    torch.manual_seed(7)
    net = _UNet().cuda()
    rng = np.random.RandomState(12)
    n, lens, cell = 16384, [16384, 4097], 0.03
    xyz, feat, lengths = dev(rng.rand(2, n, 3).astype(F32)), dev(rng.randn(2, n, 4).astype(F32)), dev(np.array(lens, I32))
    with torch.no_grad():
        first = net(xyz, feat, lengths, cell)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            second = net(xyz, feat, lengths, cell)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    ncl, cncl = host(second[1]), host(second[3])
    assert ncl[0] > 8192 and 1024 < cncl[0] < ncl[0] and ncl[1] > 2048
    _check_chain(net, second, lens)
    _check_chain_submanifold(net, second)
