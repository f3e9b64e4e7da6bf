"""GPU: rf_gridding_loss, rf_gridding and rf_gridding_grad (include/rfops.h) against gr_ref, the numpy restatement
of the contract in tests/test_gridding_host.py.  The loss, the inside counts, the grid and the loss's gradients are BIT-EQUAL to the
reference: the contract leaves no rounding freedom there.  rf_gridding_grad is within 2^-23 |ref| + 2^-45 inv_h sum |terms| -- one
float32 rounding plus the double sum's own roundings.  The grids are the smallest with one cell, one brick and a brick seam
(R = 2, 3, E, E + 1, 2 E + 1 with E = 16 the brick edge), one at R = 64 and one at R = 256; the clouds have 1, 63, 64, 65 and 257
points, with one case at 2048 against 16384."""
import numpy as np
import pytest
import torch

from test_gridding_host import (BOUNDS, BRICK, COUNTS, DENSITY, F32, KINDS, Q3, family, gr_grid_grad_ref, gr_grid_ref, gr_ref,
                                pair)

pytestmark = pytest.mark.gpu

MODES = {COUNTS: "counts", DENSITY: "density"}
SIZES = ((1, 257), (63, 64), (64, 65), (65, 1), (257, 63))
E = BRICK


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def call(a, c, R, lo, hi, mode, l1=None, l2=None, grad=True):
    """a (b, n, 3), c (b, m, 3) numpy -> numpy (loss, inside, g1, g2) or (loss, inside)"""
    from rfnet_amd import _raw
    out = _raw.gridding_loss(cu(a), cu(c), R, lo, hi, MODES[mode], None if l1 is None else cu(l1, torch.int32),
                             None if l2 is None else cu(l2, torch.int32), want_grad=grad)
    return tuple(t.cpu().numpy() for t in out)


def check(a, c, R, lo, hi, mode, l1=None, l2=None, what=""):
    """every sample of the call against gr_ref, bit for bit, and the loss-only form against the form with gradients"""
    loss, inside, g1, g2 = call(a, c, R, lo, hi, mode, l1, l2)
    only = call(a, c, R, lo, hi, mode, l1, l2, grad=False)
    assert only[0].tobytes() == loss.tobytes() and only[1].tobytes() == inside.tobytes(), f"{what}: loss-only bits"
    for i in range(a.shape[0]):
        rl, ri, r1, r2 = gr_ref(a[i], c[i], R, lo, hi, mode, None if l1 is None else l1[i], None if l2 is None else l2[i])
        w = f"{what} sample {i}"
        assert inside[i].tolist() == ri.tolist(), f"{w}: inside {inside[i]} != {ri}"
        assert loss[i].tobytes() == rl.tobytes(), f"{w}: loss {loss[i]!r} != {rl!r}"
        for got, ref, name in ((g1[i], r1, "grad1"), (g2[i], r2, "grad2")):
            bad = np.flatnonzero(got.view(np.uint32).ravel() != ref.view(np.uint32).ravel())
            assert bad.size == 0, f"{w}: {name} differs in {bad.size} entries, first {bad[0]}: {got.ravel()[bad[0]]!r} != " \
                                  f"{ref.ravel()[bad[0]]!r}"
    return loss, inside, g1, g2


# ---- 1. the small grids: every family, both modes, both boxes, every size ----------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", [2, 3, E, E + 1, 2 * E + 1])
def test_bits_of_the_reference(R, kind):
    for k, (n, m) in enumerate(SIZES):
        lo, hi = BOUNDS[k % 2]
        for mode in (COUNTS, DENSITY):
            a, c = zip(*(pair(kind, 10 * k + s, n, m, R, lo, hi) for s in range(2)))
            check(np.stack(a), np.stack(c), R, lo, hi, mode, what=f"R = {R}, {kind}, {n} x {m}, mode {mode}, box {lo, hi}")
    # and the other box for the sizes above
    for k, (n, m) in enumerate(SIZES):
        lo, hi = BOUNDS[(k + 1) % 2]
        a, c = pair(kind, 77 + k, n, m, R, lo, hi)
        check(a[None], c[None], R, lo, hi, k % 2, what=f"R = {R}, {kind}, {n} x {m}, box {lo, hi}")


# ---- 2. the large cases ------------------------------------------------------------------------------------------------------------
def test_r64_2048_against_16384():
    lo, hi = BOUNDS[0]
    a = np.stack([family("uniform", 1, 2048, 64, lo, hi), family("outside", 2, 2048, 64, lo, hi), family("seams", 3, 2048, 64, lo, hi)])
    c = np.stack([family("uniform", 4, 16384, 64, lo, hi), family("uniform", 5, 16384, 64, lo, hi),
                  family("vertices", 6, 16384, 64, lo, hi)])
    for mode in (COUNTS, DENSITY):
        loss, inside, _, _ = check(a, c, 64, lo, hi, mode, what=f"R = 64, mode {mode}")
        assert (loss > 0).all() and inside[0].tolist() == [2048, 16384] and inside[1, 0] < 2048


def test_r256():
    lo, hi = BOUNDS[1]
    a, c = family("seams", 8, 257, 256, lo, hi)[None], family("uniform", 9, 2048, 256, lo, hi)[None]
    check(a, c, 256, lo, hi, COUNTS, what="R = 256")
    check(a, c, 256, lo, hi, DENSITY, what="R = 256")
    from rfnet_amd import _raw
    grid, inside = _raw.gridding(cu(c), 256, lo, hi)
    ref, ri, _ = gr_grid_ref(c[0], 256, lo, hi)
    assert int(inside[0]) == ri and bits(grid[0]) == ref.tobytes()


def test_collapsed_clouds_reach_the_int64_bound():
    """65536 points on one vertex against 65536 on another, DENSITY: |D| = 2^16 2^16 2^27 = 2^59 on each, sum |D| = 2^60 and the
    loss is exactly 2.  The second sample collapses inside a cell: eight LDS words take 65536 adds each."""
    R, (lo, hi) = 17, BOUNDS[0]
    n = 65536
    a = np.empty((2, n, 3), F32)
    c = np.empty((2, n, 3), F32)
    a[0], c[0] = (-0.5, 0.0, 0.5), (0.5, 0.0625, -0.5)
    a[1], c[1] = (0.01, 0.02, 0.03), (0.49, -0.49, 0.3)
    loss, inside, g1, g2 = check(a, c, R, lo, hi, DENSITY, what="collapsed")
    assert gr_ref(a[0], c[0], R, lo, hi, DENSITY, full=True)[4]["sum"] == 2 ** 60
    assert loss[0] == 2.0 and loss[1] == 2.0 and (inside == n).all()
    check(a, c, R, lo, hi, COUNTS, what="collapsed, counts")
    check(a, a, R, lo, hi, DENSITY, what="collapsed, self")


# ---- 3. purity -------------------------------------------------------------------------------------------------------------------
def ragged_case(R, lo, hi):
    n, m = 257, 130
    kinds = ("uniform", "seams", "outside", "nonfinite")
    a = np.stack([family(k, 30 + i, n, R, lo, hi) for i, k in enumerate(kinds)])
    c = np.stack([family(k, 40 + i, m, R, lo, hi) for i, k in enumerate(kinds)])
    l1, l2 = np.array([n, 1, 129, 64], np.int32), np.array([77, m, 1, 65], np.int32)
    for i in range(4):
        a[i, l1[i]:] = np.nan
        c[i, l2[i]:] = np.nan
    return a, c, l1, l2


@pytest.mark.parametrize("mode", [COUNTS, DENSITY])
def test_ragged_counts_over_nan_padding_are_the_sliced_calls(mode):
    R, (lo, hi) = 2 * E + 1, BOUNDS[1]
    a, c, l1, l2 = ragged_case(R, lo, hi)
    loss, inside, g1, g2 = check(a, c, R, lo, hi, mode, l1, l2, what="ragged")
    again = call(a, c, R, lo, hi, mode, l1, l2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((loss, inside, g1, g2), again)), "two calls differ"
    for i in range(4):
        sl = call(a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]], R, lo, hi, mode)
        assert sl[0].tobytes() == loss[i:i + 1].tobytes() and sl[1].tobytes() == inside[i:i + 1].tobytes(), f"sliced call {i}"
        assert sl[2][0].tobytes() == g1[i, :l1[i]].tobytes() and sl[3][0].tobytes() == g2[i, :l2[i]].tobytes(), f"sliced call {i}"
        assert not g1[i, l1[i]:].view(np.uint32).any() and not g2[i, l2[i]:].view(np.uint32).any()  # +0 behind the counts
        one = call(a[i:i + 1], c[i:i + 1], R, lo, hi, mode, l1[i:i + 1], l2[i:i + 1])  # the batch slice
        assert all(x.tobytes() == y[i:i + 1].tobytes() for x, y in zip(one, (loss, inside, g1, g2))), f"batch slice {i}"
    # counts outside [1, n] are clamped by the kernels
    wild = call(a, c, R, lo, hi, mode, np.array([9999, -5, 129, 64], np.int32), np.array([77, 2 ** 30, 0, 65], np.int32))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(wild, (loss, inside, g1, g2)))


@pytest.mark.parametrize("mode", [COUNTS, DENSITY])
def test_permutations_and_the_self_distance(mode):
    from rfnet_amd import _raw
    R, (lo, hi) = E + 1, BOUNDS[0]
    a = np.stack([family(k, 50 + i, 257, R, lo, hi) for i, k in enumerate(("uniform", "vertices", "nonfinite"))])
    c = np.stack([family(k, 60 + i, 65, R, lo, hi) for i, k in enumerate(("seams", "vertices", "outside"))])
    loss, inside, g1, g2 = call(a, c, R, lo, hi, mode)
    p1, p2 = np.random.RandomState(1).permutation(257), np.random.RandomState(2).permutation(65)
    got = call(a[:, p1], c[:, p2], R, lo, hi, mode)
    assert got[0].tobytes() == loss.tobytes() and got[1].tobytes() == inside.tobytes()
    assert got[2].tobytes() == g1[:, p1].tobytes() and got[3].tobytes() == g2[:, p2].tobytes()
    ga, gb = _raw.gridding(cu(a), R, lo, hi), _raw.gridding(cu(a[:, p1]), R, lo, hi)
    assert bits(ga[0]) == bits(gb[0]) and bits(ga[1]) == bits(gb[1])
    zero = call(a, a, R, lo, hi, mode)
    assert not zero[0].view(np.uint32).any() and not zero[2].view(np.uint32).any() and not zero[3].view(np.uint32).any()
    assert (zero[1][:, 0] == zero[1][:, 1]).all()


# ---- 4. the layer and its backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 3, E, E + 1, 2 * E + 1, 64])
def test_layer_and_its_backward(R):
    from rfnet_amd import _raw
    for k, kind in enumerate(KINDS):
        lo, hi = BOUNDS[k % 2]
        n = (257, 65, 64, 63, 1)[k] if R < 64 else 2048
        a = np.stack([family(kind, 70 + k + s, n, R, lo, hi) for s in range(3)])
        ln = np.array([n, 1, (n + 1) // 2], np.int32)
        gg = np.random.RandomState(R + k).randn(3, R, R, R).astype(F32)
        grid, inside = _raw.gridding(cu(a), R, lo, hi, cu(ln))
        grad = _raw.gridding_grad(cu(a), cu(gg), R, lo, hi, cu(ln)).cpu().numpy()
        for i in range(3):
            ref, ri, G = gr_grid_ref(a[i], R, lo, hi, ln[i])
            assert int(inside[i]) == ri and bits(grid[i]) == ref.tobytes(), f"R = {R}, {kind}, sample {i}: the grid"
            g, tol = gr_grid_grad_ref(a[i], gg[i], R, lo, hi, ln[i])
            err = np.abs(grad[i].astype(np.float64) - g)
            assert (err <= tol).all(), f"R = {R}, {kind}, sample {i}: worst error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3f}"
            assert not grad[i][tol[:, 0] == 0].view(np.uint32).any()  # +0 outside the box and behind the count
        sl = _raw.gridding(cu(a[1:2, :1]), R, lo, hi)
        assert bits(sl[0]) == bits(grid[1:2]) and bits(sl[1]) == bits(inside[1:2])


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------------
def test_graph_capture_with_device_counts():
    """No host synchronisation anywhere: the calls are captured with device counts, and a replay returns the eager bits -- also
    after the inputs and the counts changed in place."""
    from rfnet_amd import _raw
    R, (lo, hi) = 2 * E + 1, BOUNDS[1]
    a, c, l1, l2 = ragged_case(R, lo, hi)
    ta, tc, t1, t2 = cu(a), cu(c), cu(l1), cu(l2)

    def run():
        out = _raw.gridding_loss(ta, tc, R, lo, hi, "density", t1, t2, want_grad=True)
        return out + _raw.gridding(ta, R, lo, hi, t1)

    eager = [t.clone() for t in run()]
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()  # warm-up off the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(x) == bits(y) for x, y in zip(out, eager))
    ta.copy_(cu(np.roll(np.nan_to_num(a, nan=0.1), 1, 0)))
    tc.copy_(cu(np.roll(np.nan_to_num(c, nan=0.2), 2, 0)))
    t1.copy_(torch.tensor([7, 257, 64, 200], dtype=torch.int32))
    t2.copy_(torch.tensor([130, 3, 100, 1], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    again = run()
    assert all(bits(x) == bits(y) for x, y in zip(out, again))
    assert bits(out[0]) != bits(eager[0])


# ---- 6. glue ---------------------------------------------------------------------------------------------------------------------
def test_glue_losses_through_autograd():
    from rfnet_amd import _raw, glue
    R, (lo, hi) = 2 * E + 1, BOUNDS[1]
    a, c, l1, l2 = ragged_case(R, lo, hi)
    a, c = np.nan_to_num(a, nan=9.0, posinf=9.0, neginf=-9.0), np.nan_to_num(c, nan=-9.0, posinf=9.0, neginf=-9.0)
    a, c = np.clip(a, -9, 9), np.clip(c, -9, 9)  # (a non-finite value times a zero gradient would be NaN in autograd)
    for density in (False, True):
        ta, tc = cu(a).requires_grad_(), cu(c).requires_grad_()
        loss, info = glue.gridding_loss(ta, tc, resolution=R, bounds=(lo, hi), density=density, lengths1=l1, lengths2=l2,
                                        return_info=True)
        raw = _raw.gridding_loss(ta.detach(), tc.detach(), R, lo, hi, "density" if density else "counts", l1, l2, want_grad=True)
        assert loss.shape == (4,) and torch.equal(loss.detach(), raw[0]) and torch.equal(info["inside"], raw[1])
        assert not info["inside"].requires_grad
        w = torch.tensor([0.5, -2.0, 4.0, 1.0], device="cuda")
        (loss * w).sum().backward()
        assert torch.equal(ta.grad, w[:, None, None] * raw[2]) and torch.equal(tc.grad, w[:, None, None] * raw[3])
        assert ta.grad.abs().max() > 0 and tc.grad.abs().max() > 0
        one = glue.gridding_loss(ta, tc.detach(), resolution=R, bounds=(lo, hi), density=density, lengths1=l1, lengths2=l2)
        assert torch.equal(one, loss) and one.requires_grad
        none = glue.gridding_loss(ta.detach(), tc.detach(), resolution=R, bounds=(lo, hi), density=density, lengths1=l1, lengths2=l2)
        assert torch.equal(none, loss.detach()) and not none.requires_grad
    # the defaults: 64 vertices per axis over [-0.5, 0.5]; .sum().backward() is the raw gradient
    ta, tc = cu(a[:, :, :] * 0.05).requires_grad_(), cu(c * 0.05).requires_grad_()
    glue.gridding_loss(ta, tc).sum().backward()
    raw = _raw.gridding_loss(ta.detach(), tc.detach(), 64, -0.5, 0.5, want_grad=True)
    assert torch.equal(ta.grad, raw[2]) and torch.equal(tc.grad, raw[3]) and ta.grad.abs().max() > 0
    # numpy in, numpy out
    out = _raw.gridding_loss(a, c, R, lo, hi, lengths1=l1, lengths2=l2)
    assert isinstance(out[0], np.ndarray) and out[0].tobytes() == call(a, c, R, lo, hi, COUNTS, l1, l2, grad=False)[0].tobytes()
    assert torch.equal(glue.gridding_loss(a, c, resolution=R, bounds=(lo, hi), lengths1=l1, lengths2=l2),
                       torch.from_numpy(out[0]))


def test_glue_layer_through_autograd():
    from rfnet_amd import _raw, glue
    R, (lo, hi) = E + 1, BOUNDS[0]
    a = np.stack([family(k, 90 + i, 130, R, lo, hi) for i, k in enumerate(("uniform", "seams", "outside"))])
    ln = np.array([130, 1, 65], np.int32)
    ta = cu(a).requires_grad_()
    grid = glue.gridding(ta, resolution=R, bounds=(lo, hi), lengths=ln)
    raw, _ = _raw.gridding(ta.detach(), R, lo, hi, ln)
    assert grid.shape == (3, R, R, R) and torch.equal(grid.detach(), raw) and grid.requires_grad
    gg = torch.from_numpy(np.random.RandomState(5).randn(3, R, R, R).astype(F32)).cuda()
    (grid * gg).sum().backward()
    assert torch.equal(ta.grad, _raw.gridding_grad(ta.detach(), gg, R, lo, hi, ln)) and ta.grad.abs().max() > 0
    assert not ta.grad[1, 1:].any()
    # mass: every inside point adds 1
    assert abs(float(raw[0].double().sum()) - gr_grid_ref(a[0], R, lo, hi)[2].sum() / Q3) <= 130 * 2.0 ** -23
