"""CPU: the references, bounds and route model of tests/chamfer_grad_ref.py, checked before the GPU tests rest on them.
Every reference function against an independent formulation (torch float64 autograd of the scalar function the
gradients belong to, at fixed indices); family A's proof fails when it should; an fp32 emulation of each route's
arithmetic stays inside the derived bound (the largest ratio per route is printed); the route model gives the routes
the GPU tests' shapes are named for."""
import numpy as np
import pytest
import torch

import chamfer_grad_ref as G

K = G.kernel_constants()
F32 = np.float32

ROUTES, STEP_ROUTES = G.GRAD_SHAPES, G.STEP_SHAPES


def test_route_model_at_the_shapes_of_the_gpu_tests():
    bad = [f"{s}: {G.grad_route(*s, K)} is not {r}" for s, r in ROUTES.items() if G.grad_route(*s, K) != r]
    bad += [f"{s}: {G.step_route(*s, K)} is not culled {r}" for s, r in STEP_ROUTES.items() if G.step_route(*s, K) != (True, r)]
    assert not bad, "shapes that no longer cover their route: " + "; ".join(bad)
    assert G.step_route(2, 300, 700, K)[0] is False and G.step_route(7, 1024, 2048, K)[0] is False
    assert K["GT"] * 3 // K["GTPB"] == 6 and K["RFP_GS_SEG"] == 1  # six elements per thread; the pre-sum is compiled in
    assert K["LR_TPB"] == 1024 and K["MG_TPB"] == 1024


def _case(rng, b, n, m, pattern="uniform", lens=False):
    a, c = G.clouds("randn", rng, b, n, m)
    l1 = rng.randint(1, n + 1, b) if lens else None
    l2 = rng.randint(1, m + 1, b) if lens else None
    i1 = G.indices(pattern, rng, b, n, m, l1, l2)
    i2 = G.indices(pattern, rng, b, m, n, l2, l1)
    return a, c, rng.randn(b, n).astype(F32), i1, rng.randn(b, m).astype(F32), i2, l1, l2


def _autograd(a, c, gd1, i1, gd2, i2, l1, l2):
    """d/da, d/dc of sum gd1 |a - c[idx1]|^2 + sum gd2 |c - a[idx2]|^2 over the valid rows, torch float64."""
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tc = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    c1, c2 = G.counts_of(l1, b, n), G.counts_of(l2, b, m)
    tot = 0.0
    for i in range(b):
        ni, mi = int(c1[i]), int(c2[i])
        if gd1 is not None:
            tot = tot + (torch.tensor(gd1[i, :ni], dtype=torch.float64)
                         * ((ta[i, :ni] - tc[i, torch.tensor(i1[i, :ni].astype(np.int64))]) ** 2).sum(-1)).sum()
        if gd2 is not None:
            tot = tot + (torch.tensor(gd2[i, :mi], dtype=torch.float64)
                         * ((tc[i, :mi] - ta[i, torch.tensor(i2[i, :mi].astype(np.int64))]) ** 2).sum(-1)).sum()
    tot.backward()
    return ta.grad.numpy(), tc.grad.numpy()


@pytest.mark.parametrize("pattern", G.PATTERNS)
@pytest.mark.parametrize("lens", [False, True])
def test_nn_grad_against_autograd(pattern, lens):
    rng = np.random.RandomState(11)
    a, c, gd1, i1, gd2, i2, l1, l2 = _case(rng, 3, 70, 45, pattern, lens)
    if lens:  # garbage behind the counts must not matter
        for x, ln in ((a, l1), (c, l2), (gd1, l1), (gd2, l2)):
            for i in range(3):
                x[i, ln[i]:] = np.nan
    g1, g2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2, l1, l2)
    e1, e2 = _autograd(a, c, gd1, i1, gd2, i2, l1, l2)
    assert np.all(np.abs(g1 - e1) <= 1e-12 * m1) and np.all(np.abs(g2 - e2) <= 1e-12 * m2)
    assert np.all(np.abs(g1) <= m1 * (1 + 1e-12)) and np.all(np.abs(g2) <= m2 * (1 + 1e-12))
    if lens:
        for g, ln in ((g1, l1), (g2, l2)):
            for i in range(3):
                assert not g[i, ln[i]:].any()


@pytest.mark.parametrize("dirs", [(True, True), (True, False), (False, True)])
def test_loss_and_loss_grad_against_autograd(dirs):
    rng = np.random.RandomState(12)
    a, c, _, i1, _, i2, l1, l2 = _case(rng, 3, 50, 33, "uniform", True)
    d1 = (10.0 ** rng.uniform(-8, 2, (3, 50))).astype(F32) if dirs[0] else None
    d2 = (10.0 ** rng.uniform(-8, 2, (3, 33))).astype(F32) if dirs[1] else None
    gl = rng.randn(3, 2).astype(F32)
    val, mag = G.loss(d1, d2, l1, l2)
    c1, c2 = G.counts_of(l1, 3, 50), G.counts_of(l2, 3, 33)
    for i in range(3):
        for col, (d, cnt) in enumerate(((d1, c1), (d2, c2))):
            exp = 0.0 if d is None else float(torch.sqrt(torch.tensor(d[i, :cnt[i]], dtype=torch.float64)).mean())
            assert abs(val[i, col] - exp) <= 1e-12 * max(mag[i, col], 1e-300)
    # the loss backward is nn_grad at gd = d loss / d dist: autograd of gl . mean sqrt(dist) with respect to dist
    gds = []
    for d, cnt, col in ((d1, c1, 0), (d2, c2, 1)):
        if d is None:
            gds.append(None)
            continue
        td = torch.tensor(d, dtype=torch.float64, requires_grad=True)
        sum(float(gl[i, col]) * torch.sqrt(td[i, :cnt[i]]).mean() for i in range(3)).backward()
        gds.append(td.grad.numpy())
    g1, g2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl, l1, l2)
    e1, e2 = _autograd(a, c, gds[0], i1, gds[1], i2, l1, l2)
    assert np.all(np.abs(g1 - e1) <= 1e-12 * m1) and np.all(np.abs(g2 - e2) <= 1e-12 * m2)


@pytest.mark.parametrize("dec", G.MERGE_DECS)
def test_merge_against_autograd(dec):
    rng = np.random.RandomState(13)
    b, n, m = 2, 40, 90
    lr, ln = np.array([40, 17]), np.array([90, 31])
    raw, new, idx, go = G.merge_case(rng, b, n, m, dec, "uniform", lr, ln)
    tr = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    tn = torch.tensor(new, dtype=torch.float64, requires_grad=True)
    td = torch.tensor(float(F32(dec)), dtype=torch.float64, requires_grad=True)
    outs = []
    for i in range(b):
        q = tn[i, :ln[i]]
        diff = tr[i, torch.tensor(idx[i, :ln[i]].astype(np.int64))] - q
        ratio = torch.exp(-(diff ** 2).sum(-1) / (G.C_EPS + td * td))
        outs.append(q + ratio[:, None] * diff)
    out, mag = G.merge_forward(raw, new, idx, dec, ln)
    for i in range(b):
        assert np.all(np.abs(out[i, :ln[i]] - outs[i].detach().numpy()) <= 1e-12 * mag[i, :ln[i]])
        assert not out[i, ln[i]:].any()
    sum((o * torch.tensor(go[i, :ln[i]], dtype=torch.float64)).sum() for i, o in enumerate(outs)).backward()
    (gn, gd, gr), (mn, md, mr) = G.merge_grad(raw, new, idx, dec, go, lr, ln)
    # grad_dec sums per sample in the op; autograd's is the sum over the samples
    assert abs(gd.sum() - float(td.grad)) <= 1e-11 * max(md.sum(), 1e-300)
    assert np.all(np.abs(gn - tn.grad.numpy()) <= 1e-12 * np.maximum(mn, 1e-300))
    assert np.all(np.abs(gr - tr.grad.numpy()) <= 1e-12 * np.maximum(mr, 1e-300))
    assert not gr[1, 17:].any() and not gn[1, 31:].any()


def test_family_a_proof_passes_and_fails_when_it_should():
    rng = np.random.RandomState(14)
    a, c = G.grid_clouds(rng, 2, 300, 500)
    gd1, gd2 = G.grid_gd(rng, (2, 300)), G.grid_gd(rng, (2, 500))
    i1, i2 = G.indices("uniform", rng, 2, 300, 500), G.indices("hub_last", rng, 2, 500, 300)
    e1, e2 = G.nn_grad_exact(a, c, gd1, i1, gd2, i2)
    g1, g2, _, _ = G.nn_grad(a, c, gd1, i1, gd2, i2)
    assert e1.dtype == F32 and np.array_equal(e1.astype(np.float64), g1) and np.array_equal(e2.astype(np.float64), g2)
    # a deliberately oversized hub: 200000 terms of up to 765 grid units each on one row
    a, c = G.grid_clouds(rng, 1, 4, 200000)
    with pytest.raises(AssertionError, match="could round"):
        G.nn_grad_exact(a, c, G.grid_gd(rng, (1, 4)), G.indices("uniform", rng, 1, 4, 200000),
                        G.grid_gd(rng, (1, 200000)), G.indices("hub_first", rng, 1, 200000, 4))
    # the hub of 16384 terms of the GPU tests: the coarser grid's proof decides
    a, c = G.grid_clouds(rng, 1, 7, 16384, step=2.0 ** -5, span=1.0)
    G.nn_grad_exact(a, c, G.grid_gd(rng, (1, 7)), G.indices("uniform", rng, 1, 7, 16384), G.grid_gd(rng, (1, 16384)),
                    G.indices("hub_last", rng, 1, 16384, 7), step=2.0 ** -5)
    with pytest.raises(AssertionError, match="not on the dyadic grid"):
        G.nn_grad_exact(a + F32(1e-3), c, G.grid_gd(rng, (1, 7)), G.indices("uniform", rng, 1, 7, 16384),
                        G.grid_gd(rng, (1, 16384)), G.indices("hub_last", rng, 1, 16384, 7), step=2.0 ** -5)


# ------------------------------------------------------------------ fp32 emulations of the routes ---------------------------
def _terms32(own, oth, gd, idx):
    """(own - other[idx]) * (gd + gd), each operation rounded to fp32: (rows, 3)."""
    return ((own - oth[idx.astype(np.int64)]) * (gd + gd)[:, None]).astype(F32)


def _emulate_dir(rng, dst, src, gd_d, idx_d, gd_s, idx_s, slices, presum):
    """One direction of one sample: the own term, the scatter into a float64 tile per slice (after the segmented fp32
    pre-sum of runs inside rows of 16 sources, if asked), the cast, the fp32 add of the own term, and a serial fp32
    sum of the slices' partials in a random order."""
    own = _terms32(dst, src, gd_d, idx_d)
    t = -_terms32(src, dst, gd_s, idx_s)
    ns = src.shape[0]
    per = -(-ns // slices)
    parts = []
    for s in range(slices):
        lo, hi = s * per, min(ns, (s + 1) * per)
        tile = np.zeros(dst.shape, np.float64)
        if presum:
            order = lo + np.argsort(idx_s[lo:hi], kind="stable")
            for r0 in range(0, len(order), 16):  # one 16-lane row: runs of equal destination summed in fp32, pairwise
                rows = order[r0:r0 + 16]
                for key in np.unique(idx_s[rows]):
                    v = [t[k] for k in rows if idx_s[k] == key]
                    while len(v) > 1:
                        v = [(v[i] + v[i + 1]).astype(F32) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
                    tile[key] += v[0]
        else:
            np.add.at(tile, idx_s[lo:hi].astype(np.int64), t[lo:hi].astype(np.float64))
        p = tile.astype(F32)
        parts.append((own + p).astype(F32) if s == 0 else p)
    out = np.zeros(dst.shape, F32)
    for s in rng.permutation(slices):
        out = (out + parts[s]).astype(F32)
    return out


@pytest.mark.parametrize("route,shape", [("unsliced", (1, 100, 4096)), ("unsliced", (1, 3000, 2049)), ("sliced", (1, 100, 4096)),
                                         ("sliced", (1, 3000, 2049)), ("sorted", (1, 600, 2500)), ("loss", (1, 3000, 2049))])
def test_fp32_emulation_stays_inside_the_bound(route, shape):
    b, n, m = shape
    worst = 0.0
    for pattern in ("uniform", "hub_last", "runs"):
        rng = np.random.RandomState(15)
        a, c, gd1, i1, gd2, i2, _, _ = _case(rng, b, n, m, pattern)
        r1, r2 = G.grad_route(b, n, m, K)
        s1, s2 = (r1[2], r2[2]) if route in ("sliced", "loss") else (1, 1)
        if route == "loss":  # the upstream gradients built in fp32: gl / count, times 0.5, over sqrtf(dist)
            d1, d2, gl = G.decade_dist(rng, (b, n)), G.decade_dist(rng, (b, m)), G.signed_gd(rng, (b, 2))
            g1, g2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl)
            gd1 = ((gl[:, :1] / F32(n)).astype(F32) * F32(0.5) / np.sqrt(d1)).astype(F32)
            gd2 = ((gl[:, 1:] / F32(m)).astype(F32) * F32(0.5) / np.sqrt(d2)).astype(F32)
        else:
            g1, g2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2)
        e1 = _emulate_dir(rng, a[0], c[0], gd1[0], i1[0], gd2[0], i2[0], s1, route == "sorted")
        e2 = _emulate_dir(rng, c[0], a[0], gd2[0], i2[0], gd1[0], i1[0], s2, route == "sorted")
        k1, k2 = {"sorted": (G.k_sorted(),) * 2, "loss": (G.k_loss(s1), G.k_loss(s2))}.get(route, (G.k_plain(s1), G.k_plain(s2)))
        worst = max(worst, G.worst_ratio(e1, g1[0], k1 * G.U * m1[0])[0], G.worst_ratio(e2, g2[0], k2 * G.U * m2[0])[0])
    print(f"emulation {route} {shape}: worst |fp32 - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


def _block_sum32(terms, tpb, unroll):
    """A workgroup's fp32 sum as chamfer_loss_reduce_kernel (unroll 4: four partials per thread, a tail loop into the
    first, (a0 + a1) + (a2 + a3)) and merge_pull_grad_kernel (unroll 1) take it."""
    cnt = len(terms)
    acc = np.zeros((unroll, tpb), F32)
    for t in range(min(tpb, cnt)):
        jj = t
        while jj + (unroll - 1) * tpb < cnt:
            for u in range(unroll):
                acc[u, t] = F32(acc[u, t] + terms[jj + u * tpb])
            jj += unroll * tpb
        while jj < cnt:
            acc[0, t] = F32(acc[0, t] + terms[jj])
            jj += tpb
    lane = acc[0] if unroll == 1 else ((acc[0] + acc[1]).astype(F32) + (acc[2] + acc[3]).astype(F32)).astype(F32)
    w = lane.reshape(tpb // 64, 64)
    for sh in (32, 16, 8, 4, 2, 1):  # butterfly: every lane ends with the wave's sum
        w = (w + w[:, np.arange(64) ^ sh]).astype(F32)
    tot = w[0, 0]
    for k in range(1, tpb // 64):
        tot = F32(tot + w[k, 0])
    return tot


@pytest.mark.parametrize("cnt", [1, 1023, 4097, 8193])
def test_fp32_emulation_of_the_loss_reduction(cnt):
    rng = np.random.RandomState(16)
    d = (10.0 ** rng.uniform(-8, 2, (1, cnt))).astype(F32)
    got = F32(_block_sum32(np.sqrt(d[0]).astype(F32), K["LR_TPB"], 4) / F32(cnt))
    val, _ = G.loss(d, None)
    ratio = abs(float(got) - val[0, 0]) / G.loss_bound(d, None)[0, 0]
    print(f"emulation loss forward cnt {cnt}: ratio {ratio:.3f} (K = {G.k_loss_forward(cnt)})")
    assert ratio <= 1.0


@pytest.mark.parametrize("n", [64, 3000])  # raw rows of ~40 terms; raw rows of mostly one term (tiny ones stand alone)
@pytest.mark.parametrize("dec", G.MERGE_DECS)
def test_fp32_emulation_of_merge_layer(dec, n):
    rng = np.random.RandomState(17)
    b, m = 1, 2500
    raw, new, idx, go = G.merge_case(rng, b, n, m, dec)
    g = np.take_along_axis(raw, idx[..., None].astype(np.int64), 1)
    decf = F32(dec)
    c = F32(F32(1e-8) + F32(decf * decf))
    d = (g - new).astype(F32)
    sq = (d * d).astype(F32)
    s = ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)
    with np.errstate(under="ignore"):
        ratio = np.exp((-s / c).astype(F32)).astype(F32)
        out = (new + (ratio[..., None] * d).astype(F32)).astype(F32)
        ref, _ = G.merge_forward(raw, new, idx, dec)
        worst = {"out": G.worst_ratio(out, ref, G.merge_forward_bound(raw, new, idx, dec))[0]}
        gd_ = (go * d).astype(F32)
        g_ratio = ((gd_[..., 0] + gd_[..., 1]).astype(F32) + gd_[..., 2]).astype(F32)
        k2 = (((F32(2) * ratio).astype(F32) * g_ratio).astype(F32) / c).astype(F32)
        f = ((ratio[..., None] * go).astype(F32) - (k2[..., None] * d).astype(F32)).astype(F32)
        gn = (go - f).astype(F32)
        w = ((((g_ratio * ratio).astype(F32) * s).astype(F32)) / F32(c * c)).astype(F32)
    gr = np.zeros((b, n, 3), F32)
    for j in rng.permutation(m):  # global fp32 atomics: any order
        gr[0, idx[0, j]] = (gr[0, idx[0, j]] + f[0, j]).astype(F32)
    gdec = F32(_block_sum32(w[0], K["MG_TPB"], 1) * F32(F32(2) * decf))
    r = G.merge_grad_all(raw, new, idx, dec, go)
    for name, got in (("grad_new", gn), ("grad_raw", gr), ("grad_dec", np.array([gdec]))):
        worst[name] = G.worst_ratio(got, r[name][0], r[name][1])[0]
    print(f"emulation merge_layer dec {dec} n {n}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
