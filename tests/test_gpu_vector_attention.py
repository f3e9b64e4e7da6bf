"""GPU: the vector attention pair (include/rfops.h) against the numpy restatements of
tests/test_vector_attention_host.py.  The prescribed outputs -- both forwards, grad_q, grad_pos, grad_weight -- bit for bit on
float32 inputs of wide dynamic range; the two order-free scatters (grad_src, grad_value) bit for bit where the sums are exact
(integer values; the references' own three forms are first checked to agree) and inside the header's bar against math.fsum on
random values in float32's normal range (where the header states it), every element, the worst error / bar printed.  b = 3
throughout; the shapes run round a wave, a 256-thread workgroup, the scalar and the float4 paths and past one wave of float4s,
thinned so that no case builds a large reference."""
import numpy as np
import pytest
import torch

from test_vector_attention_host import (F32, F64, I32, INT_MAX, INT_MIN, agg_grad_ref, agg_ref, indices, ints, live_mask, normal,
                                        sub_grad_ref, sub_ref, va_tol, wide)

pytestmark = pytest.mark.gpu

B = 3
SIZES = (1, 63, 64, 65, 257)
KS = (1, 3, 16, 17, 64)
CS = (1, 3, 4, 8, 60, 64, 68, 260)
FAMILIES = ("random", "identity", "hub", "perm", "hostile")
MAX_ELEMENTS = 200_000  # m k c of a case: what the references (python sums per row and channel) stay quick at


def widths(c):
    """cw over 1, c and the divisors c / 2, c / 4 where they exist"""
    return sorted({1, c} | ({c // 2} if c % 2 == 0 else set()) | ({c // 4} if c % 4 == 0 else set()))


def cases():
    """(n, m, k, c, cw): every c with every one of its widths; m, n and k run through their values from case to case, and a case
    whose m k c is beyond MAX_ELEMENTS takes the next smaller k (the thinning of test_gpu_point_voxel.channels)"""
    out, j = [], 0
    for c in CS:
        for cw in widths(c):
            m, n, ki = SIZES[j % 5], SIZES[(2 * j + 1) % 5], (j + j // 5) % 5
            while m * KS[ki] * c > MAX_ELEMENTS:
                ki -= 1
            out.append((n, m, KS[ki], c, cw))
            j += 1
    return out


CASES = cases()
assert {s[0] for s in CASES} == set(SIZES) and {s[1] for s in CASES} == set(SIZES) and {s[2] for s in CASES} == set(KS)
assert {(s[3], s[4]) for s in CASES} == {(c, cw) for c in CS for cw in widths(c)}


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype} != {ref.shape} {ref.dtype}"
    bad = np.flatnonzero(got.view(np.uint32).ravel() != ref.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {bad[0]}: {got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def within(got, exact, tol, what):
    """every element inside the bar -> the worst error / bar"""
    err = np.abs(got.astype(F64) - exact)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    assert (err <= tol).all(), f"{what}: worst error / bar {worst:.3f}"
    return worst


def inputs(gen, seed, n, m, k, c, cw, kind):
    d = dict(q=gen(seed, B, m, c), src=gen(seed + 1, B, n, c), v=gen(seed + 2, B, n, c), pos=gen(seed + 3, B, m, k, c),
             w=gen(seed + 4, B, m, k, cw), g3=gen(seed + 5, B, m, c), g4=gen(seed + 6, B, m, k, c))
    d["idx"] = np.stack([indices(kind, seed + 7 + i, m, k, n) for i in range(B)])
    return d


def run(d, L1=None, L2=None, pos=True, sl=slice(None)):
    """all four entries on the samples `sl` of d -> numpy outputs"""
    from rfnet_amd import _raw
    t = {k_: cu(x[sl]) for k_, x in d.items()}
    l1, l2 = (None if L is None else cu(np.asarray(L, I32)[sl]) for L in (L1, L2))
    n, p = d["src"].shape[1], (t["pos"] if pos else None)
    o = dict(sub=_raw.neighbor_subtraction(t["q"], t["src"], t["idx"], l1, l2))
    o["gq"], o["gs"] = _raw.neighbor_subtraction_grad(t["idx"], t["g4"], n, l1, l2)
    o["out"] = _raw.neighbor_aggregation(t["v"], t["w"], t["idx"], p, l1, l2)
    o["gv"], o["gp"], o["gw"] = _raw.neighbor_aggregation_grad(t["v"], t["w"], t["idx"], t["g3"], p, l1, l2)
    return {k_: host(x) for k_, x in o.items()}


PRESCRIBED = ("sub", "gq", "out", "gp", "gw")


def refs(d, i, L1=None, L2=None, pos=True, **forms):
    """the restatements for sample i -> (prescribed outputs, (GS, A, K), (GV, A, K))"""
    a = (None if L1 is None else L1[i], None if L2 is None else L2[i])
    p = d["pos"][i] if pos else None
    gq, GS, As, Ks = sub_grad_ref(d["idx"][i], d["g4"][i], d["src"].shape[1], *a, **forms)
    GV, Av, Kv, gp, gw = agg_grad_ref(d["v"][i], d["w"][i], d["idx"][i], d["g3"][i], p, *a, **forms)
    pres = dict(sub=sub_ref(d["q"][i], d["src"][i], d["idx"][i], *a), gq=gq, out=agg_ref(d["v"][i], d["w"][i], d["idx"][i], p, *a),
                gp=gp, gw=gw)
    return pres, (GS, As, Ks), (GV, Av, Kv)


def exact_refs(d, i, L1=None, L2=None):
    """refs on integer inputs, after checking that the references' own sums are exact: plain, reversed and fsum agree"""
    three = [refs(d, i, L1, L2, **kw) for kw in (dict(), dict(reverse=True), dict(fsum=True))]
    for j in (1, 2):
        assert three[0][j][0].tobytes() == three[1][j][0].tobytes() == three[2][j][0].tobytes(), "the reference's sums are not exact"
    return three[0]


def check(n, m, k, c, cw, kind, seed, L1=None, L2=None, what=""):
    """-> the worst error / bar of the two scatters on random values"""
    what = f"{what} n = {n}, m = {m}, k = {k}, c = {c}, cw = {cw}, {kind}"
    dw, dr, di = (inputs(gen, seed, n, m, k, c, cw, kind) for gen in (wide, normal, ints))
    worst = 0.0
    for pos in (True, False) if seed % 2 else (True,):
        gw_, gr_, gi_ = run(dw, L1, L2, pos), run(dr, L1, L2, pos), run(di, L1, L2, pos)
        for i in range(B):
            pres = refs(dw, i, L1, L2, pos)[0]
            for name in PRESCRIBED:
                same_bits(gw_[name][i], pres[name], f"{what}, pos {pos}, sample {i}: {name}")
            _, (GS, As, Ks), (GV, Av, Kv) = refs(dr, i, L1, L2, pos, fsum=True)
            worst = max(worst, within(gr_["gs"][i], GS, va_tol(GS, As, Ks), f"{what}, sample {i}: grad_src"),
                        within(gr_["gv"][i], GV, va_tol(GV, Av, Kv), f"{what}, sample {i}: grad_value"))
            pres, (GS, _, _), (GV, _, _) = exact_refs(di, i, L1, L2) if pos else refs(di, i, L1, L2, pos)
            for name in PRESCRIBED:
                same_bits(gi_[name][i], pres[name], f"{what}, integers, pos {pos}, sample {i}: {name}")
            same_bits(gi_["gs"][i], GS.astype(F32), f"{what}, sample {i}: grad_src of integer gradients")
            same_bits(gi_["gv"][i], GV.astype(F32), f"{what}, pos {pos}, sample {i}: grad_value of integer gradients")
    return worst


# ---- 1. the shapes, a family each, and every family on three shapes ----------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[f"n{n}-m{m}-k{k}-c{c}-cw{cw}" for n, m, k, c, cw in CASES])
def test_shapes(ci):
    n, m, k, c, cw = CASES[ci]
    kind = FAMILIES[ci % 5]
    worst = check(n, m, k, c, cw, kind, 100 + ci)
    print(f"\n{kind}, n = {n}, m = {m}, k = {k}, c = {c}, cw = {cw}: scatters' worst error / bar {worst:.3f}")


@pytest.mark.parametrize("kind", FAMILIES)
def test_families(kind):
    """the scalar path, the float4 path with a scalar weight index (cw = 6), and past one wave of float4s with vector weights"""
    for j, (n, m, k, c, cw) in enumerate(((65, 64, 17, 3, 1), (63, 257, 16, 12, 6), (257, 65, 3, 260, 65), (64, 63, 64, 8, 8))):
        worst = check(n, m, k, c, cw, kind, 301 + 2 * j)
        print(f"\n{kind}, n = {n}, m = {m}, k = {k}, c = {c}, cw = {cw}: scatters' worst error / bar {worst:.3f}")


def test_second_pass_with_narrow_vector_weights():
    """c = 260 is 65 float4s, a second pass of a lane row with one live lane; widths(260) has no cw = 4: one vector of weights that
    65 channel groups share"""
    n, m, k, c, cw = 65, 63, 3, 260, 4
    worst = check(n, m, k, c, cw, "random", 401)
    print(f"\nrandom, n = {n}, m = {m}, k = {k}, c = {c}, cw = {cw}: scatters' worst error / bar {worst:.3f}")


def test_hub_of_a_large_sample():
    """a row named by every slot of 2048 queries (the walk of one lane row) next to rows nobody names"""
    n, m, k, c, cw = 257, 2048, 16, 8, 4
    d = inputs(ints, 9, n, m, k, c, cw, "hub")
    got = run(d)
    for i in range(B):
        pres, (GS, _, Ks), (GV, _, _) = exact_refs(d, i)
        assert Ks.max() == m * k and (Ks > 0).sum() == 1
        same_bits(got["gs"][i], GS.astype(F32), f"hub, sample {i}: grad_src")
        same_bits(got["gv"][i], GV.astype(F32), f"hub, sample {i}: grad_value")
        same_bits(got["gq"][i], pres["gq"], f"hub, sample {i}: grad_q")


# ---- 2. ragged batches ------------------------------------------------------------------------------------------------------------
def poisoned(d, L1, L2):
    """NaN in every padded row of every input and in the slots t >= len1, garbage in idx there"""
    d = {k_: x.copy() for k_, x in d.items()}
    garbage = np.array([INT_MIN, INT_MAX, -1, 7, 1 << 20], I32)
    for i in range(B):
        for name in ("src", "v"):
            d[name][i, L1[i]:] = np.nan
        for name in ("q", "g3", "pos", "w", "g4"):
            d[name][i, L2[i]:] = np.nan
        for name in ("pos", "w", "g4"):
            d[name][i, :, L1[i]:] = np.nan
        d["idx"][i, L2[i]:] = garbage[np.arange(d["idx"][i, L2[i]:].size) % 5].reshape(d["idx"][i, L2[i]:].shape)
        d["idx"][i, :, L1[i]:] = garbage[np.arange(d["idx"][i, :, L1[i]:].size) % 5].reshape(d["idx"][i, :, L1[i]:].shape)
    return d


@pytest.mark.parametrize("n,m,k,c,cw", [(65, 63, 17, 12, 4), (257, 64, 3, 68, 68), (16, 65, 64, 3, 1)])
def test_ragged_calls_are_the_sliced_calls(n, m, k, c, cw):
    """counts [full, 1, about half] over NaN padding and garbage indices: every output is the call on the sample's slices, bit for
    bit (integer inputs for the two scatters), and +0.0 bits elsewhere.  Sample 1 has len1 = 1 < k, in the last case sample 2 too."""
    L1, L2 = np.array([n, 1, n // 2], I32), np.array([m, 1, m // 2 + 1], I32)
    for gen, names in ((wide, PRESCRIBED), (ints, PRESCRIBED + ("gs", "gv"))):
        for kind in ("random", "hostile"):
            clean = inputs(gen, 40, n, m, k, c, cw, kind)
            for i in range(B):  # (live indices below the counts, so that the slices name rows they hold)
                clean["idx"][i] = np.where(clean["idx"][i] >= 0, clean["idx"][i] % L1[i], clean["idx"][i])
            d = poisoned(clean, L1, L2)
            full = run(d, L1, L2)
            again = run(d, L1, L2)
            for i in range(B):
                part = {k_: x[i:i + 1, :(L1[i] if k_ in ("src", "v") else L2[i])] for k_, x in d.items()}
                alone = run(part)
                for name in names:
                    what = f"{gen.__name__}, {kind}, sample {i}: {name}"
                    rows = L1[i] if name in ("gs", "gv") else L2[i]
                    same_bits(full[name][i, :rows], alone[name][0], what + " against the call on the slices")
                    assert not full[name][i, rows:].view(np.uint32).any(), what + ": padded rows are not +0.0"
                    if full[name].ndim == 4:
                        assert not full[name][i, :, L1[i]:].view(np.uint32).any(), what + ": slots behind len1 are not +0.0"
                    same_bits(again[name][i], full[name][i], what + " on a second call")
                lv = live_mask(d["idx"][i], n, L1[i], L2[i])
                assert not full["sub"][i][~lv].view(np.uint32).any() and np.isfinite(full["out"][i]).all()


def test_lengths_of_a_ragged_knn_pass_through():
    """knn_point's idx -- zeros behind a short sample's neighbours and in padded queries' rows -- and its counts, fed straight in"""
    from rfnet_amd import _raw
    n, m, k, c, cw = 65, 63, 16, 8, 2
    rng = np.random.RandomState(3)
    xyz1, xyz2 = rng.rand(B, n, 3).astype(F32), rng.rand(B, m, 3).astype(F32)
    L1, L2 = np.array([n, 5, 40], I32), np.array([m, 63, 1], I32)
    t1, t2 = cu(L1), cu(L2)
    _, idx = _raw.knn_point(k, cu(xyz1), cu(xyz2), lengths1=t1, lengths2=t2)
    d = inputs(normal, 5, n, m, k, c, cw, "random")
    d["idx"] = host(idx)
    assert live_mask(d["idx"][1], n, L1[1], L2[1]).sum() == 5 * 63 and live_mask(d["idx"][2], n, L1[2], L2[2]).sum() == 16
    d = poisoned(d, L1, L2)
    d["idx"] = host(idx)  # knn_point's own padding, not garbage
    got = run(d, L1, L2)
    for i in range(B):
        pres, (GS, As, Ks), (GV, Av, Kv) = refs(d, i, L1, L2, fsum=True)
        for name in PRESCRIBED:
            same_bits(got[name][i], pres[name], f"knn lengths, sample {i}: {name}")
        within(got["gs"][i], GS, va_tol(GS, As, Ks), f"knn lengths, sample {i}: grad_src")
        within(got["gv"][i], GV, va_tol(GV, Av, Kv), f"knn lengths, sample {i}: grad_value")


def test_a_samples_bits_do_not_depend_on_its_batch():
    n, m, k, c, cw = 64, 257, 17, 60, 15
    d = inputs(ints, 77, n, m, k, c, cw, "perm")
    full = run(d)
    for i in range(B):
        alone = run(d, sl=slice(i, i + 1))
        for name in full:
            same_bits(full[name][i], alone[name][0], f"sample {i}: {name} alone against in the batch")
    pair = run(d, sl=slice(1, 3))
    for name in full:
        same_bits(full[name][1:3], pair[name], f"{name} of samples 1, 2 as a batch of two")


def test_pos_none_is_pos_zero():
    n, m, k, c, cw = 63, 65, 16, 64, 16
    d = inputs(wide, 11, n, m, k, c, cw, "random")
    d["pos"] = np.zeros_like(d["pos"])
    with_zero, without = run(d, pos=True), run(d, pos=False)
    for name in ("out", "gw"):
        same_bits(with_zero[name], without[name], f"{name}: pos = None against pos = +0")
    di = inputs(ints, 11, n, m, k, c, cw, "random")
    di["pos"] = np.zeros_like(di["pos"])
    same_bits(run(di, pos=True)["gv"], run(di, pos=False)["gv"], "grad_value: pos = None against pos = +0")


# ---- 3. autograd ------------------------------------------------------------------------------------------------------------------
def test_glue_through_autograd():
    from rfnet_amd import _raw, glue
    n, m, k, c, cw = 65, 63, 16, 12, 4
    rng = np.random.RandomState(21)
    d = {k_: rng.randn(*x.shape).astype(F32) for k_, x in inputs(ints, 21, n, m, k, c, cw, "random").items() if k_ != "idx"}
    idx = cu(np.stack([indices("random", 21 + i, m, k, n) for i in range(B)]))
    L1, L2 = cu(np.array([n, 9, 33], I32)), cu(np.array([m, 63, 2], I32))
    leaf = lambda name: cu(d[name]).requires_grad_(True)  # noqa: E731
    # the subtraction
    q, src = leaf("q"), leaf("src")
    sub = glue.neighbor_subtraction(q, src, idx, L1, L2)
    sub.backward(cu(d["g4"]))
    gq, gs = _raw.neighbor_subtraction_grad(idx, cu(d["g4"]), n, L1, L2)
    same_bits(host(q.grad), host(gq), "glue grad_q")
    within(host(src.grad), host(gs).astype(F64), 1e-5 * float(gs.abs().max()) * np.ones(1), "glue grad_src against the raw call")
    q2 = leaf("q")
    sub2 = glue.neighbor_subtraction(q2, cu(d["src"]), idx, L1, L2)
    sub2.backward(cu(d["g4"]))
    same_bits(host(q2.grad), host(gq), "glue grad_q alone")
    src2 = leaf("src")
    assert glue.neighbor_subtraction(cu(d["q"]), src2, idx, L1, L2).requires_grad and not idx.requires_grad
    # the aggregation, every subset of the three gradients
    raw = _raw.neighbor_aggregation_grad(cu(d["v"]), cu(d["w"]), idx, cu(d["g3"]), cu(d["pos"]), L1, L2)
    for mask in range(1, 8):
        want = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]  # value, weight, pos
        v, w, p = (leaf(nm) if on else cu(d[nm]) for nm, on in zip(("v", "w", "pos"), want))
        out = glue.neighbor_aggregation(v, w, idx, pos=p, lengths1=L1, lengths2=L2)
        out.backward(cu(d["g3"]))
        for t, on, r, name in ((v, want[0], raw[0], "grad_value"), (w, want[1], raw[2], "grad_weight"), (p, want[2], raw[1], "grad_pos")):
            if not on:
                assert t.grad is None, f"{name} computed though not required (mask {mask})"
            elif name == "grad_value":
                within(host(t.grad), host(r).astype(F64), 1e-5 * float(r.abs().max()) * np.ones(1), f"glue {name} (mask {mask})")
            else:
                same_bits(host(t.grad), host(r), f"glue {name} (mask {mask})")
    v = leaf("v")
    glue.neighbor_aggregation(v, cu(d["w"]), idx).backward(cu(d["g3"]))  # without pos
    assert v.grad is not None and torch.isfinite(v.grad).all()
    # against the torch expression in float64, all slots live
    t64 = {k_: cu(x).double().requires_grad_(True) for k_, x in d.items() if k_ in ("q", "src", "v", "w", "pos")}
    bi = torch.arange(B, device="cuda")[:, None, None]
    rows = idx.long()
    e_sub = t64["q"][:, :, None, :] - t64["src"][bi, rows]
    e_out = ((t64["v"][bi, rows] + t64["pos"]) * t64["w"].repeat(1, 1, 1, c // cw)).sum(2)
    e_sub.backward(cu(d["g4"]).double())
    e_out.backward(cu(d["g3"]).double())
    q, src, v, w, p = (leaf(nm) for nm in ("q", "src", "v", "w", "pos"))
    sub = glue.neighbor_subtraction(q, src, idx)
    out = glue.neighbor_aggregation(v, w, idx, pos=p)
    sub.backward(cu(d["g4"]))
    out.backward(cu(d["g3"]))
    for got, exp, name in ((sub, e_sub, "sub"), (out, e_out, "out"), (q.grad, t64["q"].grad, "grad_q"), (src.grad, t64["src"].grad, "grad_src"),
                           (v.grad, t64["v"].grad, "grad_value"), (w.grad, t64["w"].grad, "grad_weight"), (p.grad, t64["pos"].grad, "grad_pos")):
        err = float((got.detach().double() - exp.detach()).abs().max())
        assert err <= 1e-5 * float(exp.detach().abs().max()), f"{name}: {err} against the float64 torch expression"


# ---- 4. the chain, eager and from a graph ---------------------------------------------------------------------------------------
def test_chain_eager_and_from_a_graph():
    """knn_point -> neighbor_subtraction -> neighbor_aggregation (the relative features as pos) and their backward, captured once
    and replayed on new inputs and counts.  Integer features in [-8, 8]: every sum is exact, so the scatters' bits are promised."""
    from rfnet_amd import _raw, glue
    n, m, k, c, cw = 257, 129, 16, 8, 4
    sets = []
    for v in range(2):
        rng = np.random.RandomState(60 + v)
        sets.append(dict(x1=rng.rand(B, n, 3).astype(F32), x2=rng.rand(B, m, 3).astype(F32),
                         L1=np.array([[n, 7, 100], [64, n, 20]][v], I32), L2=np.array([[m, 129, 1], [2, 77, m]][v], I32),
                         **{nm: rng.randint(-8, 9, sh).astype(F32) for nm, sh in (("q", (B, m, c)), ("src", (B, n, c)), ("v", (B, n, c)),
                                                                                  ("w", (B, m, k, cw)), ("go", (B, m, c)))}))
    t = {nm: cu(x) for nm, x in sets[0].items()}

    def chain():
        _, idx = _raw.knn_point(k, t["x1"], t["x2"], lengths1=t["L1"], lengths2=t["L2"])
        q, src, v, w = (t[nm].detach().requires_grad_(True) for nm in ("q", "src", "v", "w"))
        sub = glue.neighbor_subtraction(q, src, idx, t["L1"], t["L2"])
        out = glue.neighbor_aggregation(v, w, idx, pos=sub, lengths1=t["L1"], lengths2=t["L2"])
        return (idx, sub, out) + torch.autograd.grad(out, (q, src, v, w), t["go"])

    def load(s):
        for nm, x in s.items():
            t[nm].copy_(cu(x))

    eager = []
    for s in (sets[1], sets[0]):
        load(s)
        eager.append([host(x).copy() for x in chain()])
    eager.reverse()  # (the tensors now hold set 0)
    for v, s in enumerate(sets):  # the eager chain against the restatements
        for i in range(B):
            sub = sub_ref(s["q"][i], s["src"][i], eager[v][0][i], s["L1"][i], s["L2"][i])
            same_bits(eager[v][1][i], sub, f"set {v}, sample {i}: sub")
            same_bits(eager[v][2][i], agg_ref(s["v"][i], s["w"][i], eager[v][0][i], sub, s["L1"][i], s["L2"][i]), f"set {v}, sample {i}: out")
            GV = agg_grad_ref(s["v"][i], s["w"][i], eager[v][0][i], s["go"][i], sub, s["L1"][i], s["L2"][i])[0]
            same_bits(eager[v][5][i], GV.astype(F32), f"set {v}, sample {i}: grad_value")
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        chain()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    names = ("idx", "sub", "out", "grad_q", "grad_src", "grad_value", "grad_weight")
    for v in (0, 1, 0):
        load(sets[v])  # the inputs and the counts change in place, on the device: nothing is read back
        graph.replay()
        torch.cuda.synchronize()
        for name, got, exp in zip(names, outs, eager[v]):
            assert host(got).tobytes() == exp.tobytes(), f"replay on set {v}: {name} differs from the eager bits"
    assert eager[0][2].tobytes() != eager[1][2].tobytes()
