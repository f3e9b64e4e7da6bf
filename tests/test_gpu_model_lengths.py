"""RFNet's forward over a ragged batch (per-sample partial-cloud sizes) and the two ragged entries it needs that the
earlier ragged operators did not bring: the poolings over the points axis (rf_maxpool_points_lengths /
rf_maxpool_points_idx_lengths) and merge_layer (rf_merge_layer_lengths / rf_merge_layer_grad_lengths).

The reference of every kernel check is the DENSE entry called on that sample's slice alone, bit for bit (the ragged merge_layer
is held to the float64 formula and torch autograd as well, since both forms are one kernel template); rows behind a count
are filled with values that would win if they were read (+inf / NaN for a max, copies of the query points for a nearest
neighbour search).  The network is checked against the float64 restatement oracle run per sample on the unpadded slice
(the bars of tests/test_rfnet_model.py) and against its own dense B = 1 call on the slice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POOL_COUNTS = [1, 255, 256, 257, 512, 600]  # n = 600: three strips of 256 rows


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ the pooling kernels --------------------------
def _poison_workspace(nbytes):
    """+inf into the cached scratch the next pooling call on this stream will be handed (a stale partial, if the fold
    read one, would win the max)."""
    from rfnet_amd import _host as H
    buf, _ = H.workspace(nbytes, torch.device("cuda", torch.cuda.current_device()), "maxpool")
    buf[: buf.numel() // 4 * 4].view(torch.float32).fill_(float("inf"))


def _pool_case(c, fill, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + c)
    x = torch.randn(6, 600, c, device="cuda", generator=g)
    x[:, 7] = x[:, 3]  # ties inside the valid rows: the lower index wins
    for i, ln in enumerate(POOL_COUNTS):
        x[i, ln:] = fill
    return x


@pytest.mark.parametrize("fill", [float("inf"), float("nan")])
@pytest.mark.parametrize("c", [4, 12, 64, 1024])
def test_pool_kernels_equal_the_dense_entries_on_slices(c, fill):
    from rfnet_amd import _raw
    from rfnet_amd._lib import lib
    x = _pool_case(c, fill)
    need = lib.rf_maxpool_points_idx_lengths_workspace_bytes(6, 600, c)
    ref = [_raw.maxpool_points_idx(x[i:i + 1, :ln].contiguous()) for i, ln in enumerate(POOL_COUNTS)]
    ref_v, ref_i = torch.cat([r[0] for r in ref]), torch.cat([r[1] for r in ref])
    assert torch.isfinite(ref_v).all()
    counts = {"list": POOL_COUNTS, "cpu": torch.tensor(POOL_COUNTS), "cuda32": torch.tensor(POOL_COUNTS, dtype=torch.int32).cuda(),
              "cuda64": torch.tensor(POOL_COUNTS).cuda(), "numpy": np.array(POOL_COUNTS, np.int32)}
    for kind, ln in counts.items():
        _poison_workspace(need)
        out = _raw.maxpool_points(x, ln)
        assert torch.equal(out, ref_v), kind
        _poison_workspace(need)
        out, idx = _raw.maxpool_points_idx(x, ln)
        assert torch.equal(out, ref_v) and torch.equal(idx, ref_i), kind
        assert bool((idx < torch.tensor(POOL_COUNTS, device="cuda").unsqueeze(1)).all()), kind
    # device counts outside [1, n] are held inside by the kernels: 0 -> 1, n + 7 -> n
    wild = torch.tensor([0, 255, 256, 257, 512, 607], dtype=torch.int32).cuda()
    held = [1, 255, 256, 257, 512, 600]
    xw = x.clone()
    xw[5] = torch.randn(600, c, device="cuda")
    out, idx = _raw.maxpool_points_idx(xw, wild)
    for i, ln in enumerate(held):
        ev, ei = _raw.maxpool_points_idx(xw[i:i + 1, :ln].contiguous())
        assert torch.equal(out[i:i + 1], ev) and torch.equal(idx[i:i + 1], ei), i


@pytest.mark.parametrize("c", [4, 64])
def test_pool_without_counts_is_the_dense_entry(c):
    from rfnet_amd import _raw
    x = torch.randn(6, 600, c, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    assert torch.equal(_raw.maxpool_points(x, None), _raw.maxpool_points(x))
    dv, di = _raw.maxpool_points_idx(x)
    full = [600] * 6
    for ln in (None, full, torch.tensor(full, dtype=torch.int32).cuda()):
        v, i = _raw.maxpool_points_idx(x, ln)
        assert torch.equal(v, dv) and torch.equal(i, di)
        assert torch.equal(_raw.maxpool_points(x, ln), dv)
    assert torch.equal(dv, x.amax(1, keepdim=True))


def test_pool_skips_nan_in_valid_rows_as_fmaxf_does():
    from rfnet_amd import _raw
    x = _pool_case(64, float("inf"), seed=9)
    x[1, 0:200:3, :] = float("nan")   # NaNs among the valid rows
    x[2, :256, 5] = float("nan")      # a channel that is NaN on every valid row: -inf, index 0, as the dense entry has it
    x[3, 256, :] = float("nan")       # the single row of the last written strip
    out, idx = _raw.maxpool_points_idx(x, POOL_COUNTS)
    val = _raw.maxpool_points(x, POOL_COUNTS)
    for i, ln in enumerate(POOL_COUNTS):
        ev, ei = _raw.maxpool_points_idx(x[i:i + 1, :ln].contiguous())
        assert torch.equal(out[i:i + 1], ev) and torch.equal(idx[i:i + 1], ei) and torch.equal(val[i:i + 1], ev), i
    assert float(out[2, 0, 5]) == float("-inf") and int(idx[2, 5]) == 0
    assert not torch.isnan(out).any()


# ------------------------------------------------------------------ the pooling Functions ------------------------
def test_maxpool_function_with_counts():
    from rfnet_amd.rfnet import _MaxPool, maxpool_points
    x = _pool_case(64, float("nan"), seed=3)
    up = torch.randn(6, 1, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    xr = x.clone().requires_grad_(True)
    out = maxpool_points(xr, POOL_COUNTS)
    assert out.grad_fn is not None
    (gin,) = torch.autograd.grad((out * up).sum(), xr)
    for i, ln in enumerate(POOL_COUNTS):
        xs = x[i:i + 1, :ln].clone().requires_grad_(True)
        os_ = _MaxPool.apply(xs)
        (gs,) = torch.autograd.grad((os_ * up[i:i + 1]).sum(), xs)
        assert torch.equal(out[i:i + 1], os_) and torch.equal(gin[i:i + 1, :ln], gs), i
        assert not gin[i, ln:].any(), i  # exactly zero on padded rows
    with torch.no_grad():
        assert torch.equal(maxpool_points(x, POOL_COUNTS), out)


def test_row_sparse_and_dense_pool_backward_agree_on_a_ragged_input():
    """_PooledChain with counts (backward recomputed on the arg-max rows, all of them below the count) against the dense
    backward through _MaxPool with counts; the bar of test_row_sparse_pool_backward_equals_the_dense_backward (2e-3 of the
    gradient's size).  Padded rows are finite here but far above the data: read, they would win every channel."""
    from rfnet_amd.rfnet import RFNet
    torch.manual_seed(0)
    net = RFNet().cuda()
    counts = [600, 513, 257, 40]
    g = torch.Generator(device="cuda").manual_seed(5)
    xyz = torch.rand(4, 600, 3, device="cuda", generator=g) - 0.5
    for i, ln in enumerate(counts):
        xyz[i, ln:] = 50.0
    up = torch.randn(4, 1, 256, device="cuda", generator=g)
    res = {}
    for sparse in (True, False):
        net.sparse_pool_backward = sparse
        net.zero_grad(set_to_none=True)
        xr = xyz.clone().requires_grad_(True)
        out = net.global_mlp("init_mlp", xr, counts)
        (out * up).sum().backward()
        res[sparse] = (out.detach(), xr.grad, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res[True][0], res[False][0])  # the forward is the same code
    for i, ln in enumerate(counts):
        with torch.no_grad():  # the sample alone: only the GEMM batch size differs (the C5 test's bar for that)
            alone = net.global_mlp("init_mlp", xyz[i:i + 1, :ln].contiguous())
        assert torch.allclose(res[True][0][i:i + 1], alone, rtol=1e-4, atol=1e-5), i
        assert not res[True][1][i, ln:].any() and not res[False][1][i, ln:].any(), i
    assert set(res[True][2]) == set(res[False][2]) and len(res[True][2]) == 6
    pairs = [("input", res[True][1], res[False][1])] + [(n, gs, res[False][2][n]) for n, gs in res[True][2].items()]
    for n, gs, gd in pairs:
        err = float((gs - gd).abs().max()) / (float(gd.abs().max()) + 1e-12)
        assert err < 2e-3, (n, err)


# ------------------------------------------------------------------ merge_layer -----------------------------------
DENSE_SHAPE = dict(b=3, n=300, m=257, len_raw=[1, 37, 300])
CULLED_SHAPE = dict(b=4, n=2048, m=2048, len_raw=[2048, 1301, 64, 1])
MERGE_CASES = [pytest.param(DENSE_SHAPE, None, "nn_sweep_len_1dir", id="dense-all-new"),
               pytest.param(DENSE_SHAPE, [257, 100, 1], "nn_sweep_len_1dir", id="dense-ragged-new"),
               pytest.param(CULLED_SHAPE, None, "nnp_sweep", id="culled-all-new"),
               pytest.param(CULLED_SHAPE, [2048, 700, 2048, 33], "nnp_sweep", id="culled-ragged-new")]


def _merge_case(shape, len_new):
    b, n, m, len_raw = shape["b"], shape["n"], shape["m"], shape["len_raw"]
    rng = np.random.RandomState(b * n + m)
    raw = (rng.rand(b, n, 3) - 0.5).astype(np.float32)
    new = (rng.rand(b, m, 3) - 0.5).astype(np.float32)
    for i, lr in enumerate(len_raw):
        # padded raw rows: copies of the sample's own new points, at distance 0 from them -- read, they win every search
        raw[i, lr:] = new[i, np.arange(n - lr) % m]
    ln = [m] * b if len_new is None else len_new
    return cu(raw), cu(new), len_raw, ln


def _profiled(fn):
    """fn() with the library's per-kernel event brackets on -> (result, {launch name: (ms, launches)})."""
    from rfnet_amd import _lib
    _lib.profile_collect()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, _lib.profile_collect()
    finally:
        _lib.profile_enable(False)


@pytest.mark.parametrize("shape,len_new,sweep", MERGE_CASES)
def test_merge_layer_equals_the_dense_entry_on_slices(shape, len_new, sweep):
    from rfnet_amd import _raw
    raw, new, lr, ln = _merge_case(shape, len_new)
    dec = torch.tensor([0.07], device="cuda")
    (refined, idx2), prof = _profiled(lambda: _raw.merge_layer(raw, new, dec, lengths=lr, lengths_new=len_new))
    # the route: the ragged dense sweep of one direction, or the culled sweep -- never the other, never the dense entry's
    other = "nnp_sweep" if sweep == "nn_sweep_len_1dir" else "nn_sweep_len_1dir"
    assert sweep in prof and other not in prof and "merge_pull_len" in prof and "merge_pull" not in prof, sorted(prof)
    for i in range(shape["b"]):
        er, ei = _raw.merge_layer(raw[i:i + 1, :lr[i]].contiguous(), new[i:i + 1, :ln[i]].contiguous(), dec)
        assert torch.equal(idx2[i:i + 1, :ln[i]], ei), i
        assert torch.equal(refined[i:i + 1, :ln[i]], er), i
        assert int(idx2[i].max()) < lr[i] and int(idx2[i].min()) >= 0, i
        assert not idx2[i, ln[i]:].any() and not refined[i, ln[i]:].any(), i  # padded new rows: index 0 ...
        assert not torch.signbit(refined[i, ln[i]:]).any(), i                  # ... and +0.0
    # counts as device tensors: the same call
    r2, i2 = _raw.merge_layer(raw, new, dec, lengths=torch.tensor(lr).cuda(),
                              lengths_new=None if len_new is None else torch.tensor(len_new, dtype=torch.int32).cuda())
    assert torch.equal(r2, refined) and torch.equal(i2, idx2)


@pytest.mark.parametrize("shape,len_new,sweep", MERGE_CASES)
def test_merge_layer_gradient_equals_the_dense_entry_on_slices(shape, len_new, sweep):
    """grad_newpts and grad_dec bit for bit; grad_raw is accumulated with atomics in both entries, so it is held to the
    bar the repository's numeric merge-layer gradient check uses (tests/test_gpu_chamfer_ext.py: rtol 1e-4, atol 1e-5 of
    the gradient's size; the check in tests/test_gpu_glue.py only asks for a non-zero gradient)."""
    from rfnet_amd import _raw
    raw, new, lr, ln = _merge_case(shape, len_new)
    b, n, m = shape["b"], shape["n"], shape["m"]
    dec = torch.tensor([0.07], device="cuda")
    _, idx2 = _raw.merge_layer(raw, new, dec, lengths=lr, lengths_new=len_new)
    go = torch.randn(b, m, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m))
    idx_in = idx2.clone()
    for i in range(b):  # what padded new rows hold must not matter
        go[i, ln[i]:] = float("nan")
        idx_in[i, ln[i]:] = 1 << 30
    gn, gd, gr = _raw.merge_layer_grad(raw, new, dec, idx_in, go, want_raw=True, lengths=lr, lengths_new=len_new)
    assert torch.isfinite(gn).all() and torch.isfinite(gd).all() and torch.isfinite(gr).all()
    for i in range(b):
        en, ed, er = _raw.merge_layer_grad(raw[i:i + 1, :lr[i]].contiguous(), new[i:i + 1, :ln[i]].contiguous(), dec,
                                           idx2[i:i + 1, :ln[i]].contiguous(), go[i:i + 1, :ln[i]].contiguous(), want_raw=True)
        assert torch.equal(gn[i:i + 1, :ln[i]], en) and torch.equal(gd[i:i + 1], ed), i
        assert torch.allclose(gr[i:i + 1, :lr[i]], er, rtol=1e-4, atol=1e-5 * float(er.abs().max())), i
        assert not gr[i, lr[i]:].any() and not gn[i, ln[i]:].any(), i
    gn2, gd2, none = _raw.merge_layer_grad(raw, new, dec, idx_in, go, lengths=lr, lengths_new=len_new)
    assert none is None and torch.equal(gn2, gn) and torch.equal(gd2, gd)


def test_merge_layer_ragged_against_the_float64_formula(orc):
    """The ragged entries against references that share no kernel with them (the two tests above compare one instantiation
    of the pull kernels with the other): per sample, on the slice, idx2 from the oracle's nn_distance, the reference's
    formula (vv_recon.py:132-139) in numpy float64, gradients from glue.merge_layer_unfused under torch autograd.  The bars
    are those of tests/test_gpu_chamfer_ext.py::test_merge_layer_fused_vs_reference_formula.  The new counts sit on both
    sides of the backward's 1024-thread stride and leave a zero-fill tail; padding is NaN on every input."""
    from rfnet_amd import _raw, glue
    b, n, m = 4, 300, 1100
    len_raw, len_new = [1, 64, 299, 300], [1, 1024, 1025, 1100]
    rng = np.random.RandomState(b * n + m)
    raw = (rng.rand(b, n, 3) - 0.5).astype(np.float32)
    new = (rng.rand(b, m, 3) - 0.5).astype(np.float32)
    w = rng.randn(b, m, 3).astype(np.float32)
    dec = np.float32(0.07)
    for i in range(b):
        raw[i, len_raw[i]:] = np.nan
        new[i, len_new[i]:] = np.nan
        w[i, len_new[i]:] = np.nan
    traw, tnew, tw = cu(raw), cu(new), cu(w)
    tdec = torch.tensor([dec], device="cuda")
    refined, idx2 = _raw.merge_layer(traw, tnew, tdec, lengths=len_raw, lengths_new=len_new)
    gn, gd, gr = _raw.merge_layer_grad(traw, tnew, tdec, idx2, tw, want_raw=True, lengths=len_raw, lengths_new=len_new)
    for i in range(b):
        lr, ln = len_raw[i], len_new[i]
        sraw, snew = raw[i:i + 1, :lr], new[i:i + 1, :ln]
        i2 = orc.nn_distance(sraw, snew)[3]
        assert np.array_equal(idx2[i:i + 1, :ln].cpu().numpy(), i2), i
        g = np.take_along_axis(sraw, i2[..., None].astype(np.int64), 1).astype(np.float64)
        diff = g - snew
        ratio = np.exp(-(diff * diff).sum(-1, keepdims=True) / (1e-8 + float(dec) ** 2))
        assert np.allclose(refined[i:i + 1, :ln].cpu().numpy(), snew + ratio * diff, rtol=1e-5, atol=1e-6), i
        # padded new rows: index 0 and refined with all bits zero
        assert not idx2[i, ln:].any() and not refined[i, ln:].view(torch.int32).any(), i
        uraw, unew = cu(sraw).requires_grad_(True), cu(snew).requires_grad_(True)
        udec = torch.tensor([dec], device="cuda", requires_grad=True)
        (glue.merge_layer_unfused(uraw, unew, udec) * tw[i:i + 1, :ln]).sum().backward()
        assert torch.allclose(gn[i:i + 1, :ln], unew.grad, rtol=1e-4, atol=1e-5 * float(unew.grad.abs().max())), i
        assert torch.allclose(gr[i:i + 1, :lr], uraw.grad, rtol=1e-4, atol=1e-5 * float(uraw.grad.abs().max())), i
        assert torch.allclose(gd[i:i + 1], udec.grad, rtol=1e-3, atol=1e-4 * float(udec.grad.abs().max()) + 1e-6), i
        assert not gn[i, ln:].any() and not gr[i, lr:].any(), i  # exactly zero behind the counts


def test_glue_merge_layer_and_sampling_take_the_counts():
    from rfnet_amd import _raw, glue
    raw, new, lr, _ = _merge_case(DENSE_SHAPE, None)
    tr, tn = raw.clone().requires_grad_(True), new.clone().requires_grad_(True)
    dec = torch.tensor([0.07], device="cuda", requires_grad=True)
    out, idx = glue.merge_layer(tr, tn, dec, return_idx=True, lengths=lr)
    er, ei = _raw.merge_layer(raw, new, dec.detach(), lengths=lr)
    assert torch.equal(out, er) and torch.equal(idx, ei)
    out.sum().backward()
    gn, gd, gr = _raw.merge_layer_grad(raw, new, dec.detach(), ei, torch.ones_like(er), want_raw=True, lengths=lr)
    assert torch.equal(tn.grad, gn) and torch.allclose(dec.grad, gd.sum().reshape(1))
    assert all(not tr.grad[i, ln:].any() for i, ln in enumerate(lr)) and float(tr.grad.abs().sum()) > 0
    cloud = torch.rand(3, 300, 3, device="cuda")
    counts = [300, 37, 64]
    for i, ln in enumerate(counts):
        cloud[i, ln:] = float("nan")
    fidx, fxyz = glue.sampling(32, cloud, lengths=counts)
    for i, ln in enumerate(counts):
        ei, ex = glue.sampling(32, cloud[i:i + 1, :ln].contiguous())
        assert torch.equal(fidx[i:i + 1], ei) and torch.equal(fxyz[i:i + 1], ex), i


# ------------------------------------------------------------------ the network ------------------------------------
NET_COUNTS = [3000, 1777, 300]


def _dead(n):
    """The parameters full_process leaves without a gradient (the rule of test_c5_size_forward_backward_properties)."""
    return ("refine_layer_final__feat_refine" in n or
            (n.startswith("biases.decode_cell_1__state") and "state_trans" not in n))


def _seeded_net(seed=0, bias_std=0.05):
    """As tests/test_rfnet_model.py: the reference's initialisation plus non-zero biases and decline factors of a useful
    size, so that the bias plumbing is under test."""
    from rfnet_amd.rfnet import RFNet
    torch.manual_seed(seed)
    net = RFNet()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.biases.values():
            p.copy_(bias_std * torch.randn(p.shape, generator=g))
        for i, dn in enumerate(("decline_factor0", "decline_factor1", "decline_factor")):
            getattr(net, dn).fill_(0.05 + 0.03 * i)
    return net


def _partial(nan_padding=True):
    rng = np.random.RandomState(3)
    partial = (rng.rand(3, 3000, 3) - 0.5).astype(np.float32)
    if nan_padding:
        for i, ln in enumerate(NET_COUNTS):
            partial[i, ln:] = np.nan
    return partial


@pytest.fixture(scope="module")
def ragged_run():
    """One ragged forward (B = 3, N = 3000, NaN padding), shared and left unchanged."""
    net = _seeded_net().cuda()
    partial = _partial()
    col = {}
    with torch.no_grad():
        outs = net(cu(partial), collect=col, lengths=NET_COUNTS)
    return net, partial, outs, col


def test_network_outputs_are_finite_and_fps_is_the_slice_s(ragged_run):
    from rfnet_amd import _raw
    net, partial, outs, col = ragged_run
    assert [tuple(t.shape) for t in outs] == [(3, 64, 3), (3, 1024, 3), (3, 16384, 3), (3, 16384, 3)]
    for t in list(outs) + [col[k] for k in ("points1", "points2", "refine_layer_final16384", "decode_cell64", "decode_cell1024")]:
        assert torch.isfinite(t).all()
    for i, ln in enumerate(NET_COUNTS):
        assert torch.equal(col["fps32"][i:i + 1], _raw.farthest_point_sample(32, cu(partial[i:i + 1, :ln]))), i
        for k in ("merge1", "merge2", "merge3"):
            assert int(col[k][i].max()) < ln and int(col[k][i].min()) >= 0, (k, i)


def test_network_matches_the_restatement_oracle_per_sample(ragged_run, orc):
    """Every sample of the ragged batch against the float64 restatement of full_process run on its unpadded slice, FPS and
    merge indices shared: the bars of test_forward_and_training_loss_match_the_restatement_oracle (1e-4 of the reference's
    scale, merge agreement above 0.995)."""
    from oracle.rfnet_oracle import RFNetOracle
    net, partial, outs, col = ragged_run
    o = RFNetOracle(net.tf_state_dict(), orc)
    for i, ln in enumerate(NET_COUNTS):
        shared = {k: col[k][i:i + 1].cpu().numpy() for k in ("fps32", "merge1", "merge2", "merge3")}
        ref = o.forward(partial[i:i + 1, :ln], shared=shared)
        assert ref["agreement"]["fps32"] == 1.0
        for k in ("merge1", "merge2", "merge3"):
            assert ref["agreement"][k] > 0.995, (i, ref["agreement"])

        def close(got, exp, what, rel=1e-4):
            got = got[i:i + 1].detach().cpu().numpy().astype(np.float64)
            scale, err = np.abs(exp).max(), np.abs(got - exp).max()
            assert err <= rel * scale, f"sample {i} {what}: max err {err:.3e} vs scale {scale:.3e}"

        for name, t in zip(("points1", "points2", "points3", "points_final"), outs):
            close(t, ref[name], name)
        close(col["points1"], ref["points1_pre"], "collection points1")
        close(col["points2"], ref["points2_pre"], "collection points2")
        close(col["refine_layer_final16384"], ref["refinemove3"], "refinemove3")
        close(col["decode_cell64"], ref["decode_move64"], "decode_cell64")
        close(col["decode_cell1024"], ref["decode_move1024"], "decode_cell1024")


def test_network_matches_its_own_dense_call_on_each_slice(ragged_run):
    """Sample i of the ragged batch against the dense B = 1 forward on pointcloud[i, :len]: allclose(rtol 1e-4, atol 1e-5),
    the bar test_c5_size_forward_backward_properties holds a sample of a batch to against the same sample alone (only the
    GEMM batch size differs) -- on the output points whose merge indices, their own and their ancestors', agree between the
    two runs (a near-tie may flip with the last bits of the network's output); at most 0.5 % of a sample's points may be
    left out that way (1 - 0.995, the agreement bar above)."""
    net, partial, outs, col = ragged_run
    for i, ln in enumerate(NET_COUNTS):
        c1 = {}
        with torch.no_grad():
            one = net(cu(partial[i:i + 1, :ln]), collect=c1)
        assert torch.equal(c1["fps32"], col["fps32"][i:i + 1])
        a1 = (c1["merge1"] == col["merge1"][i:i + 1])[0]
        a2 = (c1["merge2"] == col["merge2"][i:i + 1])[0] & a1.repeat_interleave(16)
        a3 = (c1["merge3"] == col["merge3"][i:i + 1])[0] & a2.repeat_interleave(16)
        for name, got, exp, ok in (("points1", outs[0], one[0], a1), ("points2", outs[1], one[1], a2),
                                   ("points3", outs[2], one[2], a2.repeat_interleave(16)), ("final", outs[3], one[3], a3)):
            assert float(ok.float().mean()) >= 0.995, (i, name, float(ok.float().mean()))
            assert torch.allclose(got[i][ok], exp[0][ok], rtol=1e-4, atol=1e-5), (i, name)


def test_network_full_counts_equal_no_counts():
    net = _seeded_net().cuda()
    x = cu(_partial(nan_padding=False))
    with torch.no_grad():
        dense, ragged = net(x), net(x, lengths=[3000] * 3)
    for a, b in zip(dense, ragged):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("sparse", [True, False])
def test_backward_through_the_ragged_forward(sparse):
    """training_loss on a fixed-size gt: a finite loss and a finite gradient on every live parameter, with NaN padding in the
    caller's tensor.  The dense pooled backward (sparse False) multiplies whole (B, N, C) activations into the weight
    gradients: a padded row that kept a NaN would show there as 0 * NaN."""
    from rfnet_amd.rfnet import training_loss
    net = _seeded_net().cuda()
    net.sparse_pool_backward = sparse
    rng = np.random.RandomState(5)
    gt = cu((rng.rand(3, 16384, 3) - 0.5).astype(np.float32))
    col = {}
    outs = net(cu(_partial()), collect=col, lengths=torch.tensor(NET_COUNTS, dtype=torch.int32).cuda())
    loss = training_loss(net, outs, col, gt)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(t).all() for t in outs)
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert all(_dead(n) for n in missing), [n for n in missing if not _dead(n)]
    bad = [n for n, p in net.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not bad, bad
    assert all(float(p.grad.abs().max()) > 0 for n, p in net.named_parameters() if n.startswith("weights.init_mlp"))


def test_ragged_forward_captures_into_a_graph():
    """Counts on the device: one ragged forward captured into a HIP graph (nothing reads the counts on the host) replays
    bit for bit, and again after the counts tensor was overwritten in place."""
    net = _seeded_net().cuda()
    clean = cu(_partial(nan_padding=False)[:2])
    first, second = [3000, 1777], [900, 3000]

    def padded(counts):
        t = clean.clone()
        for i, c in enumerate(counts):
            t[i, c:] = float("nan")
        return t

    x = padded(first)
    ln = torch.tensor(first, dtype=torch.int32).cuda()
    with torch.no_grad():
        eager = [t.clone() for t in net(x, lengths=ln)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x, lengths=ln)  # warm up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = net(x, lengths=ln)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
        x.copy_(padded(second))
        ln.copy_(torch.tensor(second, dtype=torch.int32).cuda())
        g.replay()
        torch.cuda.synchronize()
        again = net(x, lengths=torch.tensor(second, dtype=torch.int32).cuda())
        assert all(torch.isfinite(t).all() for t in out)
        assert all(torch.equal(a, b) for a, b in zip(out, again))
        assert not all(torch.equal(a, b) for a, b in zip(out, eager))
