"""GPU checks of knn_point (knn.hip: rf_knn, rf_knn_boxes, rf_knn_grad): val / idx bit for bit against an in-test numpy
statement of the contract (the unfused fp32 distance, a stable sort by (distance, index), a NaN distance first), both forms,
ragged sizes, ties, degenerate and non-finite clouds; k = 3 against three_nn; caller sort handles; the routing of the public
op and its memory; the gradients; the rule that picks the form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ref_knn(k, xyz1, xyz2, chunk=256):
    """-> val (b,m,k) float32 = -d, idx (b,m,k): d = ((dx*dx)+(dy*dy))+(dz*dz) in float32, dx = x1 - x2; ascending by
    (d, index) with a NaN distance before every number."""
    b, m = xyz2.shape[0], xyz2.shape[1]
    val = np.empty((b, m, k), np.float32)
    idx = np.empty((b, m, k), np.int64)
    for bi in range(b):
        x1 = xyz1[bi]
        for j0 in range(0, m, chunk):
            q = xyz2[bi, j0:j0 + chunk]
            dx = x1[None, :, 0] - q[:, None, 0]
            dy = x1[None, :, 1] - q[:, None, 1]
            dz = x1[None, :, 2] - q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            key = np.where(np.isnan(d), np.float32(-1), d)
            o = np.argsort(key, axis=1, kind="stable")[:, :k]
            idx[bi, j0:j0 + chunk] = o
            val[bi, j0:j0 + chunk] = -np.take_along_axis(d, o, axis=1)
    return val, idx


def same_val(got, exp):
    """bit-equal for numbers, NaN where NaN"""
    got, exp = np.asarray(got), np.asarray(exp)
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), exp[~nan].view(np.int32))


def run(form, k, x1, x2, **kw):
    from rfnet_amd import _raw as R
    v, i = R.knn_point(k, cu(x1), cu(x2), form=form, **kw)
    return v.cpu().numpy(), i.cpu().numpy()


def check_both(k, x1, x2, what=""):
    ev, ei = ref_knn(k, x1, x2)
    for form in ("scan", "boxes"):
        v, i = run(form, k, x1, x2)
        assert np.array_equal(i, ei), (form, what)
        assert same_val(v, ev), (form, what)


@pytest.mark.parametrize("b,n,m,k", [
    (1, 1, 1, 1), (2, 70, 33, 3), (3, 100, 129, 1), (2, 1000, 250, 16), (2, 999, 301, 20), (2, 1111, 257, 32), (2, 513, 200, 33),
    (2, 777, 300, 64), (2, 64, 70, 64), (2, 20, 9, 20), (32, 300, 100, 16), (2, 5000, 700, 8),
])
def test_parity(b, n, m, k):
    rng = np.random.RandomState(n * 7 + m + k)
    x1 = rng.rand(b, n, 3).astype(np.float32)
    x2 = rng.rand(b, m, 3).astype(np.float32)
    check_both(k, x1, x2)


@pytest.mark.parametrize("b,n,m,k", [(2, 16384, 4096, 32), (1, 65536, 256, 16)])
def test_parity_large(b, n, m, k):
    rng = np.random.RandomState(n + m)
    x1 = rng.randn(b, n, 3).astype(np.float32)
    x2 = rng.randn(b, m, 3).astype(np.float32)
    check_both(k, x1, x2)


@pytest.mark.parametrize("kind", ["duplicates", "lattice", "queries_are_points", "identical", "flat"])
def test_ties_and_degenerate_clouds(kind):
    rng = np.random.RandomState(3)
    b, n, m = 2, 2000, 300
    if kind == "duplicates":
        x1 = rng.rand(b, n, 3).astype(np.float32)
        x1[:, 1000:1500] = x1[:, :500]
        x1[:, 1500:1600] = x1[:, 7:8]
        x2 = rng.rand(b, m, 3).astype(np.float32)
    elif kind == "lattice":
        g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25
        x1 = np.stack([g[rng.permutation(len(g))[:n]] for _ in range(b)])
        x2 = (np.floor(rng.rand(b, m, 3) * 13) * 0.25 + 0.125 * (rng.rand(b, m, 3) > 0.5)).astype(np.float32)
    elif kind == "queries_are_points":
        x1 = rng.rand(b, n, 3).astype(np.float32)
        x2 = x1[:, rng.choice(n, m, replace=False)].copy()
    elif kind == "identical":
        x1 = np.full((b, n, 3), 0.3, np.float32)
        x2 = rng.rand(b, m, 3).astype(np.float32)
    else:
        x1 = rng.rand(b, n, 3).astype(np.float32)
        x2 = rng.rand(b, m, 3).astype(np.float32)
        x1[..., 2] = 0
        x2[..., 2] = 0
    for k in (1, 5, 20, 64):
        check_both(k, x1, x2, (kind, k))
    if kind == "identical":
        for form in ("scan", "boxes"):
            _, i = run(form, 10, x1, x2)
            assert np.array_equal(i, np.broadcast_to(np.arange(10), i.shape)), form


def test_ten_identical_points_tie_to_the_lower_index():
    from tf_ops.grouping.tf_grouping import knn_point
    x1 = torch.full((1, 10, 3), 0.5, device="cuda")
    _, i = knn_point(5, x1, x1[:, :3])
    assert i.cpu().numpy().tolist() == [[[0, 1, 2, 3, 4]] * 3]


@pytest.mark.parametrize("where", ["candidates", "queries", "both"])
def test_non_finite_coordinates(where):
    rng = np.random.RandomState(11)
    b, n, m = 2, 3000, 400
    x1 = rng.rand(b, n, 3).astype(np.float32)
    x2 = rng.rand(b, m, 3).astype(np.float32)
    if where in ("candidates", "both"):
        x1[0, 17, 1] = np.nan
        x1[0, 2500, 0] = np.inf
        x1[1, 40:45, 2] = -np.inf
        x1[1, 900, :] = np.nan
    if where in ("queries", "both"):
        x2[0, 3, 0] = np.nan
        x2[0, 200, 2] = np.inf
        x2[1, 399, 1] = -np.inf
    for k in (1, 7, 32):
        check_both(k, x1, x2, (where, k))
        sv, si = run("scan", k, x1, x2)
        bv, bi = run("boxes", k, x1, x2)
        assert np.array_equal(si, bi) and np.array_equal(sv.view(np.int32), bv.view(np.int32)), (where, k)
    if where != "candidates":
        _, i = run("scan", 7, x1, x2)
        v, _ = run("scan", 7, x1, x2)
        assert np.array_equal(i[0, 3], np.arange(7)) and np.all(np.isnan(v[0, 3]))
    if where == "candidates":
        v, i = run("boxes", 3, x1, x2)
        assert np.all(i[0, :, 0] == 17) and np.all(i[1, :, 0] == 900)  # a NaN distance first
        assert np.all(np.isnan(v[:, :, 0])) and not np.any(np.isnan(v[:, :, 1:]))
        assert not np.any(i[0] == 2500)  # +inf after every finite distance


def test_k3_equals_three_nn():
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(5)
    for b, n, m in ((2, 5000, 3000), (3, 300, 64), (1, 20000, 2048)):
        known = rng.rand(b, n, 3).astype(np.float32)
        unknown = rng.rand(b, m, 3).astype(np.float32)
        known[:, 100:200] = known[:, :100]
        d, ti = R.three_nn(cu(unknown), cu(known), form="scan")
        for form in ("scan", "boxes"):
            v, i = R.knn_point(3, cu(known), cu(unknown), form=form)
            assert torch.equal(i, ti), form
            assert torch.equal(v.view(torch.int32), (-d).view(torch.int32)), form


def test_sort_handles():
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(9)
    b, n, m, k = 3, 6000, 2000, 24
    t1, t2 = cu(rng.randn(b, n, 3).astype(np.float32)), cu(rng.randn(b, m, 3).astype(np.float32))
    v0, i0 = R.knn_point(k, t1, t2, form="boxes")
    sv, si = R.knn_point(k, t1, t2, form="scan")
    assert torch.equal(i0, si) and torch.equal(v0.view(torch.int32), sv.view(torch.int32))
    h1, h2 = R.nn_sort(t1), R.nn_sort(t2)
    for kw in ({"sorted1": h1.buf}, {"sorted2": h2.buf}, {"sorted1": h1.buf, "sorted2": h2.buf}):
        v, i = R.knn_point(k, t1, t2, form="boxes", **kw)
        assert torch.equal(i, i0) and torch.equal(v.view(torch.int32), v0.view(torch.int32)), sorted(kw)


def old_knn(k, xyz1, xyz2):
    xyz1, xyz2 = torch.as_tensor(xyz1), torch.as_tensor(xyz2)
    dist = ((xyz1.unsqueeze(1) - xyz2.unsqueeze(2)) ** 2).sum(-1)
    val, idx = torch.topk(-dist, k=int(k), dim=-1)
    return val, idx.to(torch.int32)


def test_routing_memory():
    from rfnet_amd import _lib
    from rfnet_amd import _raw as R
    from tf_ops.grouping.tf_grouping import knn_point
    b, n, m, k = 4, 16384, 4096, 16
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.rand(b, n, 3, device="cuda", generator=g)
    x2 = torch.rand(b, m, 3, device="cuda", generator=g)
    v, i = knn_point(k, x1, x2)  # (warm: the HIP code objects, torch's caches)
    del v, i
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    v, i = knn_point(k, x1, x2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = b * m * k * 8
    workspace = int(_lib.lib.rf_knn_boxes_workspace_bytes(b, n, m))
    assert peak <= outputs + workspace + (64 << 20), peak
    sv, si = R.knn_point(k, x1, x2, form="scan")
    assert torch.equal(i, si) and torch.equal(v, sv)
    # the old expression's neighbour sets and values on this tie-free data (1e-6 absolute: torch's sum may round otherwise)
    ov, oi = old_knn(k, x1[:1, :4096], x2[:1, :512])
    nv, ni = knn_point(k, x1[:1, :4096].contiguous(), x2[:1, :512].contiguous())
    assert torch.equal(torch.sort(ni, -1).values, torch.sort(oi, -1).values)
    assert torch.allclose(nv, ov, rtol=0, atol=1e-6)


def test_routing_keeps_the_old_expression_elsewhere():
    from tf_ops.grouping.tf_grouping import knn_point
    rng = np.random.RandomState(2)
    a = rng.rand(2, 80, 3).astype(np.float32)
    q = rng.rand(2, 9, 3).astype(np.float32)
    cases = [
        (4, torch.from_numpy(a), torch.from_numpy(q)),  # CPU tensors
        (4, a, q),  # numpy arrays
        (4, cu(a).double(), cu(q).double()),  # float64
        (4, cu(rng.rand(2, 80, 4).astype(np.float32)), cu(rng.rand(2, 9, 4).astype(np.float32))),  # c = 4
    ]
    big = cu(rng.rand(2, 100, 3).astype(np.float32))
    cases.append((65, big, cu(q)))  # k > 64
    for k, x1, x2 in cases:
        v, i = knn_point(k, x1, x2)
        ov, oi = old_knn(k, x1, x2)
        assert type(v) is type(ov) and v.device == ov.device and v.dtype == ov.dtype
        assert torch.equal(v, ov) and torch.equal(i, oi)


def np_grads(x1, x2, idx, g):
    x1, x2, g = x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64)
    g1, g2 = np.zeros_like(x1), np.zeros_like(x2)
    b, m, k = idx.shape
    for bi in range(b):
        nb = x1[bi][idx[bi]]  # (m, k, 3)
        term = 2 * g[bi][..., None] * (nb - x2[bi][:, None, :])
        g2[bi] = term.sum(1)
        np.add.at(g1[bi], idx[bi].reshape(-1), -term.reshape(-1, 3))
    return g1, g2


@pytest.mark.parametrize("b,n,m,k", [(2, 3000, 500, 16), (3, 400, 1000, 33), (1, 20000, 4096, 8)])
def test_gradients(b, n, m, k):
    from tf_ops.grouping.tf_grouping import knn_point
    rng = np.random.RandomState(b + n + k)
    a = rng.rand(b, n, 3).astype(np.float32)
    q = rng.rand(b, m, 3).astype(np.float32)
    a[:, -1] = 1e3  # a row no slot names
    g = rng.randn(b, m, k).astype(np.float32)
    t1, t2 = cu(a).requires_grad_(True), cu(q).requires_grad_(True)
    v, i = knn_point(k, t1, t2)
    v.backward(cu(g))
    e1, e2 = np_grads(a, q, i.cpu().numpy(), g)
    g1, g2 = t1.grad.cpu().numpy(), t2.grad.cpu().numpy()
    assert np.allclose(g1, e1, rtol=1e-5, atol=1e-6) and np.allclose(g2, e2, rtol=1e-5, atol=1e-6)
    assert np.all(g1[:, -1] == 0)
    # the old expression's autograd on this tie-free data
    o1, o2 = cu(a).requires_grad_(True), cu(q).requires_grad_(True)
    ov, _ = old_knn(k, o1, o2)
    ov.backward(cu(g))
    assert torch.allclose(t1.grad, o1.grad, rtol=1e-4, atol=1e-5) and torch.allclose(t2.grad, o2.grad, rtol=1e-4, atol=1e-5)
    # only one input asks for the gradient
    t3 = cu(q).requires_grad_(True)
    v3, _ = knn_point(k, cu(a), t3)
    v3.backward(cu(g))
    assert torch.allclose(t3.grad, t2.grad, rtol=0, atol=0)


def test_gradient_hot_row():
    from rfnet_amd import _raw as R
    rng = np.random.RandomState(4)
    b, n, m, k = 2, 5000, 4096, 8
    dirs = rng.randn(b, n, 3)
    a = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True) * (10 + rng.rand(b, n, 1))).astype(np.float32)
    a[:, 123] = 0  # every query's nearest
    q = (rng.rand(b, m, 3) * 0.1).astype(np.float32)
    v, i = R.knn_point(k, cu(a), cu(q))
    ih = i.cpu().numpy()
    assert np.all(ih[..., 0] == 123)
    g = rng.randn(b, m, k).astype(np.float32)
    g1, g2 = R.knn_point_grad(cu(a), cu(q), i, cu(g))
    e1, e2 = np_grads(a, q, ih, g)
    assert np.allclose(g1.cpu().numpy(), e1, rtol=1e-5, atol=1e-5)
    assert np.allclose(g2.cpu().numpy(), e2, rtol=1e-5, atol=1e-6)


def test_auto_rule_takes_the_boxed_kernel():
    from rfnet_amd import _lib
    from rfnet_amd import _raw as R
    from tf_ops.grouping.tf_grouping import knn_point
    rng = np.random.RandomState(8)
    b, n, m, k = 4, 16384, 16384, 16
    assert R.knn_auto_boxes(k, n, m) and not R.knn_auto_boxes(k, n, 1024)
    x1, x2 = cu(rng.rand(b, n, 3).astype(np.float32)), cu(rng.rand(b, m, 3).astype(np.float32))
    _lib.profile_enable(True)
    try:
        _lib.profile_collect()
        v, i = knn_point(k, x1, x2)
        torch.cuda.synchronize()
        names = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    assert "knn_boxes" in names and "knn" not in names, names
    sv, si = R.knn_point(k, x1, x2, form="scan")
    assert torch.equal(i, si) and torch.equal(v.view(torch.int32), sv.view(torch.int32))
