#!/usr/bin/env python3
"""Measured |kernel - float64 reference| / bound of the Chamfer gradient kernels and the fused loss ops, family B, once per
launch route (references, bounds and routes: tests/chamfer_grad_ref.py; the asserting tests: tests/test_gpu_chamfer_grad.py),
and expf's measured worst error against float64 exp of the same fp32 argument.  Every ratio must be at most 1: above it
the kernel or the derivation is wrong.  usage: python tools/chamfer_grad_ratios.py > profiles/chamfer_grad_bounds.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_grad_ref as G  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from rfnet_amd import _raw as R  # noqa: E402

K = G.kernel_constants()
ROWS = []


def cu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def row(kernel, route, output, k, got, ref, bound):
    ratio, same = G.worst_ratio(got, ref, bound)
    ROWS.append(ratio)
    print(f"{kernel:<30} {route:<60} {output:<10} K {str(k):<6} worst ratio {ratio:6.3f}" + ("" if same else "   NaN MASKS DIFFER"))


def grad_routes():
    for shape, (r1, r2) in G.GRAD_SHAPES.items():
        b, n, m = shape
        for kind, pattern in (("randn", "uniform"), ("randn", "hub_last"), ("collapsed", "nn")):
            rng = np.random.RandomState(1)
            a, c = G.clouds(kind, rng, b, n, m)
            if pattern == "nn":
                e = ORC.nn_distance(a, c)
                i1, i2 = e[1], e[3]
            else:
                i1, i2 = G.indices(pattern, rng, b, n, m), G.indices(pattern, rng, b, m, n)
            gd1, gd2 = G.signed_gd(rng, (b, n)), G.signed_gd(rng, (b, m))
            g1, g2 = host(R.nn_distance_grad(cu(a), cu(c), cu(gd1), cu(i1), cu(gd2), cu(i2)))
            f1, f2, m1, m2 = G.nn_grad(a, c, gd1, i1, gd2, i2)
            for g, f, mg, r, name in ((g1, f1, m1, r1, "grad_xyz1"), (g2, f2, m2, r2, "grad_xyz2")):
                row("nn_grad_kernel<0>", f"{shape} gt {r[0]} tiles {r[1]} slices {r[2]} {kind}/{pattern}", name, G.k_plain(r[2]), g, f,
                    G.k_plain(r[2]) * G.U * mg)
        rng = np.random.RandomState(2)
        a, c = G.clouds("randn", rng, b, n, m)
        i1, i2 = G.indices("uniform", rng, b, n, m), G.indices("uniform", rng, b, m, n)
        d1, d2, gl = G.decade_dist(rng, (b, n)), G.decade_dist(rng, (b, m)), G.signed_gd(rng, (b, 2))
        g1, g2 = host(R.chamfer_loss_grad(cu(a), cu(c), cu(d1), cu(i1), cu(d2), cu(i2), cu(gl)))
        f1, f2, m1, m2 = G.loss_grad(a, c, d1, i1, d2, i2, gl)
        for g, f, mg, r, name in ((g1, f1, m1, r1, "grad_xyz1"), (g2, f2, m2, r2, "grad_xyz2")):
            row("nn_grad_kernel<1>", f"{shape} gt {r[0]} tiles {r[1]} slices {r[2]} randn/uniform", name, G.k_loss(r[2]), g, f,
                G.k_loss(r[2]) * G.U * mg)


def ragged_routes():
    for shape in ((1, 100, 4096), (2, 3000, 2049), (300, 70, 33)):
        b, n, m = shape
        r1, r2 = G.grad_route(b, n, m, K)
        rng = np.random.RandomState(7)
        l1, l2 = rng.randint(1, n + 1, b), rng.randint(1, m + 1, b)
        a, c = G.clouds("randn", rng, b, n, m)
        i1, i2 = G.indices("uniform", rng, b, n, m, l1, l2), G.indices("uniform", rng, b, m, n, l2, l1)
        gd1, gd2 = G.signed_gd(rng, (b, n)), G.signed_gd(rng, (b, m))
        d1, d2, gl = G.decade_dist(rng, (b, n)), G.decade_dist(rng, (b, m)), G.signed_gd(rng, (b, 2))
        got = host(R.nn_distance_grad(cu(a), cu(c), cu(gd1), cu(i1), cu(gd2), cu(i2), lengths1=l1, lengths2=l2))
        ref = G.nn_grad(a, c, gd1, i1, gd2, i2, l1, l2)
        lgot = host(R.chamfer_loss_grad(cu(a), cu(c), cu(d1), cu(i1), cu(d2), cu(i2), cu(gl), lengths1=l1, lengths2=l2))
        lref = G.loss_grad(a, c, d1, i1, d2, i2, gl, l1, l2)
        for j, (r, name) in enumerate(((r1, "grad_xyz1"), (r2, "grad_xyz2"))):
            route = f"{shape} lengths, gt {r[0]} tiles {r[1]} slices {r[2]} randn/uniform"
            row("nn_grad_kernel<0, per_sample>", route, name, G.k_plain(r[2]), got[j], ref[j], G.k_plain(r[2]) * G.U * ref[j + 2])
            row("nn_grad_kernel<1, per_sample>", route, name, G.k_loss(r[2]), lgot[j], lref[j], G.k_loss(r[2]) * G.U * lref[j + 2])


def step_routes():
    for shape, sets in G.STEP_SHAPES.items():
        b, n, m = shape
        for kind in ("randn", "collapsed", "same"):
            rng = np.random.RandomState(3)
            a, c = G.clouds(kind, rng, b, n, m)
            gd1, gd2 = G.signed_gd(rng, (b, n)), G.signed_gd(rng, (b, m))
            out = host(R.ChamferStep(b, n, m, "cuda")(cu(a), cu(c), cu(gd1), cu(gd2)))
            f1, f2, m1, m2 = G.nn_grad(a, c, gd1, out[1], gd2, out[3])
            for g, f, mg, st, name in ((out[4], f1, m1, sets[0], "grad_xyz1"), (out[5], f2, m2, sets[1], "grad_xyz2")):
                row("grad_tile", f"{shape} npad {st[0]} gt {st[2]} tiles {st[3]} {kind}", name, G.k_sorted(), g, f, G.k_sorted() * G.U * mg)


def loss_forward():
    t = K["LR_TPB"]
    for b, n, m in ((3, t - 1, 1), (3, t, 1), (2, 4 * t, 2), (2, 4 * t + 1, 2), (2, 8 * t + 1, 1)):
        rng = np.random.RandomState(4)
        a, c = G.clouds("randn", rng, b, n, m)
        got = host(R.chamfer_loss(cu(a), cu(c)))
        row("chamfer_loss_reduce_kernel", f"({b}, {n}, {m})", "loss", f"{G.k_loss_forward(n)}/{G.k_loss_forward(m)}", got[0],
            G.loss(got[1], got[3])[0], G.loss_bound(got[1], got[3]))


def merge():
    for shape in ((2, 64, 300), (2, 3000, 1024)):
        for dec in G.MERGE_DECS:
            rng = np.random.RandomState(5)
            raw, new, _, _ = G.merge_case(rng, *shape, dec)
            out, idx = host(R.merge_layer(cu(raw), cu(new), dec))
            row("merge_pull_kernel", f"{shape} dec {dec}", "refined", "-", out, G.merge_forward(raw, new, idx, dec)[0],
                G.merge_forward_bound(raw, new, idx, dec))
    for shape in ((3, 64, 1023), (2, 300, 1025), (2, 2048, 4097), (4, 7, 16384)):
        for dec in G.MERGE_DECS:
            for pattern in ("uniform", "hub_last"):
                rng = np.random.RandomState(6)
                raw, new, idx, go = G.merge_case(rng, *shape, dec, pattern)
                got = host(R.merge_layer_grad(cu(raw), cu(new), dec, cu(idx), cu(go), want_raw=True))
                r = G.merge_grad_all(raw, new, idx, dec, go, mg_tpb=K["MG_TPB"])
                for g, name in zip(got, ("grad_new", "grad_dec", "grad_raw")):
                    row("merge_pull_grad_kernel", f"{shape} dec {dec} {pattern}", name, "-", g, r[name][0], r[name][1])


def expf_error():
    """expf through merge_pull_grad_kernel: one raw point (dx, 0, 0) per new point at the origin and grad_out (0, 0, 1) make
    the z entry of grad_raw the kernel's ratio itself (g_ratio = 0, one atomic add onto 0: no other rounding), for the fp32
    argument -fl(fl(dx dx) / c), which numpy's fp32 arithmetic reproduces."""
    worst_n, worst_s, at_n, at_s = 0.0, 0.0, 0.0, 0.0
    for dec in (0.07, 1.0, 1e-4):
        decf = np.float32(dec)
        c = np.float32(np.float32(1e-8) + np.float32(decf * decf))
        m = 1 << 18
        x = np.linspace(0.0, 104.5, m)
        dx = np.sqrt(x * float(c)).astype(np.float32)
        raw = np.zeros((1, m, 3), np.float32)
        raw[0, :, 0] = dx
        new, go = np.zeros((1, m, 3), np.float32), np.zeros((1, m, 3), np.float32)
        go[..., 2] = 1.0
        gr = host(R.merge_layer_grad(cu(raw), cu(new), dec, cu(np.arange(m, dtype=np.int32)[None]), cu(go), want_raw=True))[2]
        arg = -((dx * dx).astype(np.float32) / c).astype(np.float32)
        ref = np.exp(arg.astype(np.float64))
        err = G.ulp_distance(gr[0, :, 2], ref)
        sub = ref < 2.0 ** -126
        for mask, which in ((~sub, "n"), (sub, "s")):
            if mask.any():
                j = int(np.argmax(np.where(mask, err, -1.0)))
                if which == "n" and err[j] > worst_n:
                    worst_n, at_n = float(err[j]), float(arg[j])
                if which == "s" and err[j] > worst_s:
                    worst_s, at_s = float(err[j]), float(arg[j])
    print(f"expf, {3 * (1 << 18)} arguments in [-104.5, 0]: worst error {worst_n:.3f} ulp where the result is normal (at {at_n!r}), "
          f"{worst_s:.3f} ulp (of 2^-149) where it is subnormal (at {at_s!r}); allowed in the bounds: {G.EXPF_ULP} ulp")
    return max(worst_n, worst_s)


if __name__ == "__main__":
    ORC = Oracle()
    print(f"# |kernel - float64 reference| / bound, family B, one run per route on {torch.cuda.get_device_name(0)}")
    print("# kernel, route, output, K (bound = K U mag; '-' = the composite bounds of merge_forward_bound / merge_grad_all), worst ratio")
    grad_routes()
    ragged_routes()
    step_routes()
    loss_forward()
    merge()
    e = expf_error()
    print(f"largest ratio of all rows: {max(ROWS):.3f}")
    sys.exit(0 if max(ROWS) <= 1.0 and e <= G.EXPF_ULP else 1)
