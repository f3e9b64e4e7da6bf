"""GPU checks of the ragged-batch EMD entries (include/rfops.h rf_approxmatch_lengths, rf_matchcost_lengths,
rf_matchcost_grad_lengths, rf_earth_mover_lengths) and of the loss built on them (glue.earth_mover with lengths).

The oracle is the CPU reference on each sample's unpadded slices; the bars are tests/test_gpu_emd.py's."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_rel, strict_bar_report

pytestmark = pytest.mark.gpu

LEVELS7 = [-256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0]  # a non-reference schedule (am_match_any_kernel)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def clouds(b, n, m, seed):
    rng = np.random.RandomState(seed)
    a = (rng.random_sample((b, n, 3)) - 0.5).astype(np.float32)
    c = (rng.random_sample((b, m, 3)) - 0.5).astype(np.float32)
    return a, c


def counts(b, n, m, seed):
    """Random counts with a full one, a 1 (where the batch allows) and len1 != len2."""
    rng = np.random.RandomState(seed + 1)
    l1, l2 = rng.randint(1, n + 1, b), rng.randint(1, m + 1, b)
    l1[0] = n
    l2[b - 1] = m
    if b >= 2:
        l2[0] = 1
    if b >= 3:
        l1[1] = 1
    return l1.astype(np.int32), l2.astype(np.int32)


def hostile(a, l, fill):
    """A copy of `a` whose padding rows (beyond each sample's count) hold `fill`."""
    a = a.copy()
    for i, k in enumerate(l):
        a[i, k:] = fill
    return a


def check_padding_zero(t, l, axis, what):
    """Entries beyond each sample's count along `axis` (1: rows of (b, rows, ...), 2: columns of match) are exactly +0."""
    t = np.asarray(t)
    for i, k in enumerate(l):
        pad = t[i, k:] if axis == 1 else t[i, :, k:]
        assert (pad == 0).all() and not np.signbit(pad).any(), f"{what}: sample {i} has nonzero padding"


def bars(gm, om, what, big, lone=False):
    if lone:
        # one point against hundreds (a count of 1 facing a large one): every entry hangs on the single point's one row sum,
        # whose remaining mass max(0, remain - t) cancels at the broad levels -- the last-bit difference of that sum's segment
        # order against the oracle's sequential one comes out at up to ~1e-3 of an entry (~1).  The strict bar is reported.
        strict_bar_report(what, gm, om)
        assert np.abs(gm - om).max() < 1e-3, what
    elif big:  # the C4 bar (ten-level annealing amplifies 1-ulp exp differences), the strict one reported
        strict_bar_report(what, gm, om)
        assert np.abs(gm - om).max() < 2e-4, what
        assert (np.abs(gm - om) <= 1e-6 + 1e-4 * np.abs(om)).mean() > 0.9999, what
    else:
        assert_rel(gm, om, 1e-4, 1e-6, what=what)


# ---- 1. parity with the oracle on the slices ---------------------------------------------------------------------
@pytest.mark.parametrize("b,n,m", [(3, 64, 64), (2, 256, 200), (3, 300, 257), (2, 777, 130), (1, 130, 777),
                                   (4, 1000, 1300), (2, 2048, 2048)])
def test_parity_with_oracle(orc, b, n, m):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, 11 * n + m)
    l1, l2 = counts(b, n, m, n + 7 * m)
    ta, tc = cu(a), cu(c)
    match = _raw.approx_match(ta, tc, lengths1=l1, lengths2=l2)
    cost = _raw.match_cost(ta, tc, match, lengths1=l1, lengths2=l2).cpu().numpy()
    gm = match.cpu().numpy()
    check_padding_zero(gm, l2, 1, "match rows")
    check_padding_zero(gm, l1, 2, "match columns")
    om_pad = np.zeros((b, m, n), np.float32)
    ocost = np.zeros(b, np.float32)
    og1, og2 = np.zeros((b, n, 3), np.float32), np.zeros((b, m, 3), np.float32)
    for i in range(b):
        sa, sc = a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]]
        om = orc.approx_match(sa, sc)
        bars(gm[i, :l2[i], :l1[i]], om[0], f"match, sample {i} of ({b},{n},{m}), counts ({l1[i]},{l2[i]})", n >= 2048,
             min(l1[i], l2[i]) == 1 and max(l1[i], l2[i]) > 256)
        om_pad[i, :l2[i], :l1[i]] = om[0]
        ocost[i] = orc.match_cost(sa, sc, om)[0]
        o1, o2 = orc.match_cost_grad(sa, sc, om)
        og1[i, :l1[i]], og2[i, :l2[i]] = o1[0], o2[0]
    assert_rel(cost, ocost, 1e-5, what="cost")
    # the gradient kernels on the oracle's own match, zero-padded
    g1, g2 = _raw.match_cost_grad(ta, tc, cu(om_pad), lengths1=l1, lengths2=l2)
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    check_padding_zero(g1, l1, 1, "grad1")
    check_padding_zero(g2, l2, 1, "grad2")
    assert_rel(g1, og1, 1e-4, 1e-5, what="grad1")
    assert_rel(g2, og2, 1e-4, 1e-5, what="grad2")
    # the fused op, at test_earth_mover_fused_vs_oracle's bars with each sample's own mass
    fc = _raw.earth_mover(ta, tc, lengths1=l1, lengths2=l2).cpu().numpy()
    assert_rel(fc, ocost, 1e-5, what="fused cost")
    fcg, f1, f2 = _raw.earth_mover(ta, tc, with_grad=True, lengths1=l1, lengths2=l2)
    assert_rel(fcg.cpu().numpy(), ocost, 1e-5, what="fused cost (grad variant)")
    f1, f2 = f1.cpu().numpy(), f2.cpu().numpy()
    check_padding_zero(f1, l1, 1, "fused grad1")
    check_padding_zero(f2, l2, 1, "fused grad2")
    for i in range(b):
        # (built on the GPU's own match entries: their bar, 1e-4 -- 1e-3 for a lone point, see bars() -- times the row's mass)
        massL, massR = max(1, l2[i] // l1[i]), max(1, l1[i] // l2[i])
        e = 1e-3 if min(l1[i], l2[i]) == 1 and max(l1[i], l2[i]) > 256 else 1e-4
        assert_rel(f1[i], og1[i], 1e-4, e * massL, what=f"fused grad1, sample {i}")
        assert_rel(f2[i], og2[i], 1e-4, e * massR, what=f"fused grad2, sample {i}")


# ---- 2. padding never reaches a result ------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n,m", [(3, 64, 64), (3, 300, 257), (2, 777, 1300)])
@pytest.mark.parametrize("fill", [np.nan, np.inf, 1e30])
def test_hostile_padding(b, n, m, fill):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, 5 * n + m)
    l1, l2 = counts(b, n, m, 3 * n + m)
    a0, c0 = cu(hostile(a, l1, 0.0)), cu(hostile(c, l2, 0.0))
    ah, ch = cu(hostile(a, l1, fill)), cu(hostile(c, l2, fill))
    kw = dict(lengths1=l1, lengths2=l2)
    m0, mh = _raw.approx_match(a0, c0, **kw), _raw.approx_match(ah, ch, **kw)
    assert torch.equal(m0, mh)
    # match_cost{,_grad}: the padded entries of the caller's match are hostile too
    mt = m0.clone()
    for i in range(b):
        mt[i, l2[i]:, :] = fill
        mt[i, :, l1[i]:] = fill
    c_0 = _raw.match_cost(a0, c0, m0, **kw)
    assert torch.equal(c_0, _raw.match_cost(ah, ch, mt, **kw))
    g1a, g2a = _raw.match_cost_grad(a0, c0, m0, **kw)
    g1b, g2b = _raw.match_cost_grad(ah, ch, mt, **kw)
    for ga, gb, l, what in ((g1a, g1b, l1, "grad1"), (g2a, g2b, l2, "grad2")):
        gb = gb.cpu().numpy()
        check_padding_zero(gb, l, 1, what)
        assert np.isfinite(gb).all(), what
        assert_rel(gb, ga.cpu().numpy(), 1e-5, 1e-6, what=what)
    e0 = _raw.earth_mover(a0, c0, **kw)
    assert torch.equal(e0, _raw.earth_mover(ah, ch, **kw))
    ec0, e10, e20 = _raw.earth_mover(a0, c0, with_grad=True, **kw)
    ech, e1h, e2h = _raw.earth_mover(ah, ch, with_grad=True, **kw)
    assert torch.equal(ec0, ech)
    for ga, gb, l, what in ((e10, e1h, l1, "fused grad1"), (e20, e2h, l2, "fused grad2")):
        gb = gb.cpu().numpy()
        check_padding_zero(gb, l, 1, what)
        assert np.isfinite(gb).all(), what
        assert_rel(gb, ga.cpu().numpy(), 1e-5, 1e-6, what=what)


# ---- 3. full counts and batch invariance ----------------------------------------------------------------------------
def _approxmatch_null_counts(a, c, levels=None):
    """rf_approxmatch_lengths with both count arrays NULL, through the C ABI."""
    from rfnet_amd import _host as H
    from rfnet_amd._lib import check, lib
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    nlv = 0 if levels is None else len(levels)
    lv = None if levels is None else (ctypes.c_float * nlv)(*levels)
    match = torch.empty((b, m, n), dtype=torch.float32, device=a.device)
    ws = torch.empty(lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, nlv), dtype=torch.uint8, device=a.device)
    check(lib.rf_approxmatch_lengths(b, n, m, H.ptr(a), H.ptr(c), None, None, H.ptr(match), lv, nlv, H.ptr(ws), ws.numel(),
                                     H.stream(a.device)), "rf_approxmatch_lengths")
    return match


@pytest.mark.parametrize("b,n,m", [(3, 64, 64), (2, 777, 130), (3, 300, 1300), (2, 2048, 2048)])
def test_full_counts_are_the_swept_route(b, n, m):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, 2 * n + m)
    ta, tc = cu(a), cu(c)
    full1, full2 = np.full(b, n, np.int32), np.full(b, m, np.int32)
    for levels in (None, LEVELS7):
        ref = _raw.approx_match(ta, tc, levels=levels, mode="swept")
        assert torch.equal(_raw.approx_match(ta, tc, levels=levels, lengths1=full1, lengths2=full2), ref)
        assert torch.equal(_raw.approx_match(ta, tc, levels=levels, lengths1=full1), ref)  # len2 NULL
        assert torch.equal(_raw.approx_match(ta, tc, levels=levels, lengths2=torch.from_numpy(full2).cuda()), ref)
        assert torch.equal(_approxmatch_null_counts(ta, tc, levels), ref)
    ref = _raw.approx_match(ta, tc, mode="swept")
    assert torch.equal(_raw.match_cost(ta, tc, ref, lengths1=full1, lengths2=full2), _raw.match_cost(ta, tc, ref))
    sc, s1, s2 = _raw.earth_mover(ta, tc, with_grad=True, mode="swept")
    rc, r1, r2 = _raw.earth_mover(ta, tc, with_grad=True, lengths1=full1, lengths2=full2)
    assert_rel(rc.cpu().numpy(), sc.cpu().numpy(), 1e-5, what="fused cost")
    assert_rel(r1.cpu().numpy(), s1.cpu().numpy(), 1e-4, 1e-5, what="fused grad1")
    assert_rel(r2.cpu().numpy(), s2.cpu().numpy(), 1e-4, 1e-5, what="fused grad2")
    assert_rel(_raw.earth_mover(ta, tc, lengths1=full1).cpu().numpy(), _raw.earth_mover(ta, tc, mode="swept").cpu().numpy(),
               1e-5, what="fused cost alone")


@pytest.mark.parametrize("b,n,m", [(3, 64, 64), (4, 300, 257), (3, 1000, 1300)])
def test_batch_invariance(b, n, m):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, n + 3 * m)
    l1, l2 = counts(b, n, m, 9 * n + m)
    ta, tc = cu(a), cu(c)
    for levels in (None, LEVELS7):
        match = _raw.approx_match(ta, tc, levels=levels, lengths1=l1, lengths2=l2)
        for i in range(b):
            one = _raw.approx_match(ta[i:i + 1], tc[i:i + 1], levels=levels, lengths1=l1[i:i + 1], lengths2=l2[i:i + 1])
            assert torch.equal(match[i:i + 1], one), (levels, i)
    match = _raw.approx_match(ta, tc, lengths1=l1, lengths2=l2)
    cost = _raw.match_cost(ta, tc, match, lengths1=l1, lengths2=l2)
    fused = _raw.earth_mover(ta, tc, lengths1=l1, lengths2=l2)
    fused_g = _raw.earth_mover(ta, tc, with_grad=True, lengths1=l1, lengths2=l2)[0]
    for i in range(b):
        kw = dict(lengths1=l1[i:i + 1], lengths2=l2[i:i + 1])
        assert torch.equal(cost[i:i + 1], _raw.match_cost(ta[i:i + 1], tc[i:i + 1], match[i:i + 1], **kw)), i
        assert torch.equal(fused[i:i + 1], _raw.earth_mover(ta[i:i + 1], tc[i:i + 1], **kw)), i
        assert torch.equal(fused_g[i:i + 1], _raw.earth_mover(ta[i:i + 1], tc[i:i + 1], with_grad=True, **kw)[0]), i


# ---- 4. the small path: bit for bit the call on the slices ----------------------------------------------------------
@pytest.mark.parametrize("b,n,m", [(4, 64, 64), (3, 256, 200), (3, 100, 256)])
def test_small_path_matches_slices(b, n, m):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, 13 * n + m)
    l1, l2 = counts(b, n, m, n + m)
    ta, tc = cu(a), cu(c)
    for levels in (None, LEVELS7):
        match = _raw.approx_match(ta, tc, levels=levels, lengths1=l1, lengths2=l2)
        for i in range(b):
            one = _raw.approx_match(ta[i:i + 1, :l1[i]].contiguous(), tc[i:i + 1, :l2[i]].contiguous(), levels=levels)
            assert torch.equal(match[i:i + 1, :l2[i], :l1[i]], one), (levels, i)


# ---- 5. out-of-range device counts are clamped ----------------------------------------------------------------------
@pytest.mark.parametrize("b,n,m", [(3, 64, 48), (3, 300, 257)])
def test_device_counts_clamped(b, n, m):
    from rfnet_amd import _raw
    a, c = clouds(b, n, m, n + 5 * m)
    ta, tc = cu(a), cu(c)
    bad1 = torch.tensor([0, -3, n + 5], dtype=torch.int32, device="cuda")
    bad2 = torch.tensor([m + 5, 0, -3], dtype=torch.int32, device="cuda")
    ok1, ok2 = np.array([1, 1, n], np.int32), np.array([m, 1, 1], np.int32)
    assert torch.equal(_raw.approx_match(ta, tc, lengths1=bad1, lengths2=bad2),
                       _raw.approx_match(ta, tc, lengths1=ok1, lengths2=ok2))
    mt = _raw.approx_match(ta, tc, lengths1=ok1, lengths2=ok2)
    assert torch.equal(_raw.match_cost(ta, tc, mt, lengths1=bad1, lengths2=bad2),
                       _raw.match_cost(ta, tc, mt, lengths1=ok1, lengths2=ok2))
    assert torch.equal(_raw.earth_mover(ta, tc, lengths1=bad1, lengths2=bad2),
                       _raw.earth_mover(ta, tc, lengths1=ok1, lengths2=ok2))
    # int64 device counts beyond the int32 range are clamped before narrowing
    wide = torch.tensor([0, -(1 << 40), (1 << 40) + 3], dtype=torch.int64, device="cuda")
    assert torch.equal(_raw.earth_mover(ta, tc, lengths1=wide, lengths2=ok2),
                       _raw.earth_mover(ta, tc, lengths1=ok1, lengths2=ok2))


# ---- 6. the loss ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n,m", [(3, 64, 64), (4, 300, 280), (2, 1000, 1300)])
def test_glue_earth_mover_lengths(b, n, m):
    from rfnet_amd import glue
    from rfnet_amd.pc_distance.tf_approxmatch import earth_mover_cost
    a, c = clouds(b, n, m, 17 * n + m)
    l1, l2 = counts(b, n, m, 4 * n + m)
    ta, tc = cu(a).requires_grad_(), cu(c).requires_grad_()
    loss = glue.earth_mover(ta, tc, lengths1=l1, lengths2=l2)
    loss.backward()
    ga, gc = ta.grad.cpu().numpy(), tc.grad.cpu().numpy()
    check_padding_zero(np.abs(ga), l1, 1, "loss grad1")  # (a negative scale may leave -0: exactly zero either way)
    check_padding_zero(np.abs(gc), l2, 1, "loss grad2")
    total = 0.0
    for i in range(b):
        sa = cu(a[i:i + 1, :l1[i]]).requires_grad_()
        sc = cu(c[i:i + 1, :l2[i]]).requires_grad_()
        li = earth_mover_cost(sa, sc)[0] / float(l1[i]) / b
        li.backward()
        total += float(li.detach())
        assert_rel(ga[i, :l1[i]], sa.grad.cpu().numpy()[0], 1e-4, 1e-5, what=f"grad1, sample {i}")
        assert_rel(gc[i, :l2[i]], sc.grad.cpu().numpy()[0], 1e-4, 1e-5, what=f"grad2, sample {i}")
    assert_rel(float(loss.detach()), total, 1e-5, what="loss")
    # every count format gives the same loss and gradients
    formats = [list(map(int, l1)), np.asarray(l1, np.int64), torch.from_numpy(l1), torch.from_numpy(l1).cuda().long(),
               torch.from_numpy(l1).cuda()]
    for f in formats:
        xa, xc = cu(a).requires_grad_(), cu(c).requires_grad_()
        lf = glue.earth_mover(xa, xc, lengths1=f, lengths2=l2)
        lf.backward()
        assert torch.equal(lf.detach(), loss.detach()), type(f)
        assert_rel(xa.grad.cpu().numpy(), ga, 1e-5, 1e-7, what=f"grad1 with {type(f)}")
        assert_rel(xc.grad.cpu().numpy(), gc, 1e-5, 1e-7, what=f"grad2 with {type(f)}")


# ---- 7. graph capture ----------------------------------------------------------------------------------------------
def test_graph_capture_with_device_counts():
    from rfnet_amd import _raw
    b, n, m = 3, 300, 257
    a, c = clouds(b, n, m, 99)
    ta, tc = cu(a), cu(c)
    L1 = torch.tensor([300, 17, 200], dtype=torch.int32, device="cuda")
    L2 = torch.tensor([1, 257, 100], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture (workspaces, library load)
        _raw.approx_match(ta, tc, lengths1=L1, lengths2=L2)
        _raw.earth_mover(ta, tc, with_grad=True, lengths1=L1, lengths2=L2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gm = _raw.approx_match(ta, tc, lengths1=L1, lengths2=L2)
        gc, g1, g2 = _raw.earth_mover(ta, tc, with_grad=True, lengths1=L1, lengths2=L2)
    g.replay()
    torch.cuda.synchronize()
    old = [t.clone() for t in (gm, gc, g1, g2)]
    L1.copy_(torch.tensor([120, 300, 5], dtype=torch.int32))
    L2.copy_(torch.tensor([257, 64, 250], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    em = _raw.approx_match(ta, tc, lengths1=L1, lengths2=L2)
    ec, e1, e2 = _raw.earth_mover(ta, tc, with_grad=True, lengths1=L1, lengths2=L2)
    assert torch.equal(gm, em)
    assert torch.equal(gc, ec)
    assert_rel(g1.cpu().numpy(), e1.cpu().numpy(), 1e-5, 1e-7, what="grad1")
    assert_rel(g2.cpu().numpy(), e2.cpu().numpy(), 1e-5, 1e-7, what="grad2")
    assert not torch.equal(gm, old[0]) and not torch.equal(gc, old[1])
    assert not torch.equal(g1, old[2]) and not torch.equal(g2, old[3])


# ---- 8. larger shapes ----------------------------------------------------------------------------------------------
def test_c4_ragged(orc):
    """B = 32 at 2048^2 with counts in [512, 2048]: the oracle on two samples, mass properties where len1 == len2."""
    from rfnet_amd import _raw
    b, n = 32, 2048
    a, c = clouds(b, n, n, 2024)
    rng = np.random.RandomState(5)
    l1, l2 = rng.randint(512, n + 1, b).astype(np.int32), rng.randint(512, n + 1, b).astype(np.int32)
    l2[:6] = l1[:6]  # equal counts: a doubly stochastic block
    ta, tc = cu(a), cu(c)
    match = _raw.approx_match(ta, tc, lengths1=l1, lengths2=l2)
    cost = _raw.match_cost(ta, tc, match, lengths1=l1, lengths2=l2).cpu().numpy()
    for i in (2, 9):
        sa, sc = a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]]
        om = orc.approx_match(sa, sc)
        bars(match[i, :l2[i], :l1[i]].cpu().numpy(), om[0], f"C4 ragged match, sample {i}, counts ({l1[i]},{l2[i]})", True)
        assert_rel(cost[i:i + 1], orc.match_cost(sa, sc, om), 1e-5, what=f"cost[{i}]")
    for i in range(6):
        blk = match[i, :l2[i], :l1[i]]
        rows, cols = blk.sum(0).cpu().numpy(), blk.sum(1).cpu().numpy()
        assert_rel(rows, np.ones_like(rows), 1e-3, what=f"masses shipped, sample {i}")
        assert_rel(cols, np.ones_like(cols), 1e-3, what=f"masses received, sample {i}")
    assert (match >= 0).all()
    check_padding_zero(match.cpu().numpy(), l1, 2, "C4 match columns")
    fused = _raw.earth_mover(ta, tc, lengths1=l1, lengths2=l2).cpu().numpy()
    assert_rel(fused, cost, 1e-5, what="fused cost vs chain")


def test_16k_ragged_fused():
    """B = 4 at 16384^2 (match would be 4 GiB): the fused op against per-sample swept calls on the slices."""
    from rfnet_amd import _raw
    b, n = 4, 16384
    a, c = clouds(b, n, n, 16384)
    rng = np.random.RandomState(6)
    l1, l2 = rng.randint(4096, n + 1, b).astype(np.int32), rng.randint(4096, n + 1, b).astype(np.int32)
    ta, tc = cu(a), cu(c)
    cost = _raw.earth_mover(ta, tc, lengths1=l1, lengths2=l2).cpu().numpy()
    for i in range(b):
        one = _raw.earth_mover(ta[i:i + 1, :l1[i]].contiguous(), tc[i:i + 1, :l2[i]].contiguous(), mode="swept")
        assert_rel(cost[i:i + 1], one.cpu().numpy(), 1e-5, what=f"16k cost[{i}]")
