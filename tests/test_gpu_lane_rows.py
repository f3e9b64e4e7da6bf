"""GPU: the edges of the lane-row geometry that group_point, three_interpolate and their gradients share (csrc/lane_rows.hpp): a
row of TX = 1 << tx_log2 lanes, at most a wave, walks the c / VEC channel vectors of its slot, so c > 256 sends the 4-wide path
through a second pass of the channel loop (c = 260: 65 vectors, one live lane in the second pass).  Every c runs once on tensors
as allocated and once through views 4 bytes off a 16-byte boundary, which take the scalar path also where c % 4 == 0; the row
counts (33 x 5 slots, 70 points) are no multiple of the rows per block.  Forwards bit for bit against the oracle, gradients
at rel 1e-5 with an abs floor of 1e-6 of the row scale (atomically accumulated: SURVEY 8(d), test_gpu_scatter_rows.py)."""
import numpy as np
import pytest
import torch

from conftest import assert_rel

pytestmark = pytest.mark.gpu

B, M, NS, N = 2, 33, 5, 70
CS = (1, 3, 4, 5, 64, 67, 256, 260)
_refs = {}


def cu(x, shifted=False):
    """x on the GPU; shifted: a contiguous view that starts 4 bytes behind a 16-byte boundary"""
    t = torch.from_numpy(np.array(x))  # (a copy: the shared references are read-only)
    if not shifted:
        return t.cuda()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def reference(orc, c):
    """inputs and oracle outputs for c channels, computed once and shared by the aligned and the shifted run"""
    if c not in _refs:
        rng = np.random.RandomState(1000 + c)
        d = dict(gp_pts=rng.randn(B, N, c).astype(np.float32), gp_idx=rng.randint(0, N, size=(B, M, NS)).astype(np.int32),
                 gp_go=rng.randn(B, M, NS, c).astype(np.float32), ti_pts=rng.randn(B, M, c).astype(np.float32),
                 ti_idx=rng.randint(0, M, size=(B, N, 3)).astype(np.int32), ti_w=rng.rand(B, N, 3).astype(np.float32),
                 ti_go=rng.randn(B, N, c).astype(np.float32))
        d["gp_idx"][:, :3] = 7  # a popular point
        d["ti_idx"][:, ::7, 1] = d["ti_idx"][:, ::7, 0]  # the same known point twice in a triple
        d["gp"] = orc.group_point(d["gp_pts"], d["gp_idx"])
        d["gp_grad"] = orc.group_point_grad(d["gp_pts"], d["gp_idx"], d["gp_go"])
        d["ti"] = orc.three_interpolate(d["ti_pts"], d["ti_idx"], d["ti_w"])
        d["ti_grad"] = orc.three_interpolate_grad(d["ti_pts"], d["ti_idx"], d["ti_w"], d["ti_go"])
        for v in d.values():
            v.setflags(write=False)
        _refs[c] = d
    return _refs[c]


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("c", CS)
def test_group_point_rows(orc, c, shifted):
    from rfnet_amd import _raw as R
    d = reference(orc, c)
    got = R.group_point(cu(d["gp_pts"], shifted), cu(d["gp_idx"])).cpu().numpy()
    assert np.array_equal(got, d["gp"])
    grad = R.group_point_grad(cu(d["gp_pts"]), cu(d["gp_idx"]), cu(d["gp_go"], shifted)).cpu().numpy()
    scale = max(1.0, float(np.abs(d["gp_grad"]).max()))
    assert_rel(grad, d["gp_grad"], 1e-5, 1e-6 * scale, what="group_point_grad")


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("c", CS)
def test_three_interpolate_rows(orc, c, shifted):
    from rfnet_amd import _raw as R
    d = reference(orc, c)
    got = R.three_interpolate(cu(d["ti_pts"], shifted), cu(d["ti_idx"]), cu(d["ti_w"])).cpu().numpy()
    assert np.array_equal(got, d["ti"])
    grad = R.three_interpolate_grad(cu(d["ti_pts"]), cu(d["ti_idx"]), cu(d["ti_w"]), cu(d["ti_go"], shifted)).cpu().numpy()
    scale = max(1.0, float(np.abs(d["ti_grad"]).max()))
    assert_rel(grad, d["ti_grad"], 1e-5, 1e-6 * scale, what="three_interpolate_grad")


# ---- the sorted-slots gather (scatter_rows.hip) at c = 260: the shapes above stay under its threshold of 2^22 gradient elements,
# so each op takes the smallest slot count that reaches it with b = 2 (2 x 8066 x 260 and 2 x 2689 x 3 x 260 >= 2^22)
@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
def test_group_point_grad_sorted_slots_second_pass(orc, shifted):
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    b, n, m, ns, c = B, N, 4033, 2, 260
    assert lib.rf_grouppoint_grad_workspace_bytes(b, n, c, m, ns) > 0, "shape is below the sorted-slots threshold: not the route under test"
    assert lib.rf_grouppoint_grad_workspace_bytes(b, n, c, m - 1, ns) == 0, "not the smallest such shape"
    rng = np.random.RandomState(5)
    idx = rng.randint(0, n, size=(b, m, ns)).astype(np.int32)
    go = rng.randn(b, m, ns, c).astype(np.float32)
    pts = np.zeros((b, n, c), np.float32)
    got = R.group_point_grad(cu(pts), cu(idx), cu(go, shifted)).cpu().numpy()
    want = orc.group_point_grad(pts, idx, go)
    assert_rel(got, want, 1e-5, 1e-6 * max(1.0, float(np.abs(want).max())), what="sorted slots vs oracle")


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
def test_three_interpolate_grad_sorted_slots_second_pass(orc, shifted):
    from rfnet_amd import _raw as R
    from rfnet_amd._lib import lib
    b, n, m, c = B, 2689, M, 260
    assert lib.rf_threeinterpolate_grad_workspace_bytes(b, n, c, m) > 0, "not the route under test"
    assert lib.rf_threeinterpolate_grad_workspace_bytes(b, n - 1, c, m) == 0, "not the smallest such shape"
    rng = np.random.RandomState(6)
    idx = rng.randint(0, m, size=(b, n, 3)).astype(np.int32)
    idx[:, ::7, 1] = idx[:, ::7, 0]
    w = rng.rand(b, n, 3).astype(np.float32)
    go = rng.randn(b, n, c).astype(np.float32)
    pts = np.zeros((b, m, c), np.float32)
    got = R.three_interpolate_grad(cu(pts), cu(idx), cu(w), cu(go, shifted)).cpu().numpy()
    want = orc.three_interpolate_grad(pts, idx, w, go)
    assert_rel(got, want, 1e-5, 1e-6 * max(1.0, float(np.abs(want).max())), what="sorted slots vs oracle")
