"""CPU checks of the ragged-batch entries the network's forward needs (include/rfops.h: rf_maxpool_points_lengths,
rf_maxpool_points_idx_lengths, rf_merge_layer_lengths, rf_merge_layer_grad_lengths) and of their Python wrappers up to
RFNet.forward: the symbols are exported and bound, the workspace sizes are the documented ones, every argument error comes
back before any HIP call, and host-given counts are validated before any device work -- so these run without a device
(pointers here are never dereferenced)."""
import ctypes

import numpy as np
import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h

P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p((1 << 20) + 2)
W8 = ctypes.c_void_p((1 << 20) + 8)  # 4-byte aligned, not 16
BIG = 1 << 40

ENTRIES = ("rf_maxpool_points_lengths_workspace_bytes", "rf_maxpool_points_lengths",
           "rf_maxpool_points_idx_lengths_workspace_bytes", "rf_maxpool_points_idx_lengths",
           "rf_merge_layer_lengths_workspace_bytes", "rf_merge_layer_lengths")
GRAD = "rf_merge_layer_grad_lengths"


@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


def _align256(v):
    return (v + 255) // 256 * 256


def test_symbols_exported_and_bound(lib):
    from rfnet_amd import _lib
    header = open(__file__.replace("tests/test_model_lengths_host.py", "include/rfops.h")).read()
    for name in ENTRIES + (GRAD,):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name


def test_workspace_sizes(lib):
    mp, mpi, mg = (getattr(lib, n) for n in ENTRIES[0::2])
    for b, n, c in ((0, 100, 8), (2, 0, 8), (2, 100, 0), (-1, 10, 8)):
        assert mp(b, n, c) == 0 and mpi(b, n, c) == 0 and mg(b, n, c) == 0, (b, n, c)
    for b, n, c in ((1, 1, 4), (6, 600, 12), (3, 3000, 256), (32, 19384, 256), (2, 257, 1024)):
        assert mp(b, n, c) == lib.rf_maxpool_points_workspace_bytes(b, n, c) > 0, (b, n, c)
        assert mpi(b, n, c) == lib.rf_maxpool_points_idx_workspace_bytes(b, n, c) == 2 * mp(b, n, c), (b, n, c)
    # merge: the (b, m) distances, then the ragged sweep of direction 2 alone -- dense and culled shapes
    for b, n, m in ((3, 300, 257), (4, 2048, 2048), (32, 3000, 16384), (1, 1, 1)):
        sweep = lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, 0, 1)  # = ragged_workspace_bytes(AUTO, dirs = 2)
        assert sweep > 0 and mg(b, n, m) == _align256(b * m * 4) + sweep, (b, n, m)


@pytest.mark.parametrize("b,n,c", [(-1, 100, 8), (2, -5, 8), (2, 100, -4), (2, 0, 8)])
def test_pool_bad_sizes_are_einval(lib, b, n, c):
    assert lib.rf_maxpool_points_lengths(b, n, c, P, P, P, P, BIG, None) == RF_EINVAL
    assert lib.rf_maxpool_points_idx_lengths(b, n, c, P, P, P, P, P, BIG, None) == RF_EINVAL


@pytest.mark.parametrize("b,n,m", [(-1, 100, 10), (2, -5, 10), (2, 100, -5), (2, 0, 10)])
def test_merge_bad_sizes_are_einval(lib, b, n, m):
    assert lib.rf_merge_layer_lengths(b, n, m, P, P, P, P, P, P, P, P, BIG, None) == RF_EINVAL
    if min(b, n, m) < 0:
        assert lib.rf_merge_layer_grad_lengths(b, n, m, P, P, P, P, P, P, P, P, P, P, None) == RF_EINVAL


def test_empty_batch_is_ok(lib):
    assert lib.rf_maxpool_points_lengths(0, 100, 8, None, None, None, None, 0, None) == 0
    assert lib.rf_maxpool_points_idx_lengths(0, 100, 8, None, None, None, None, None, 0, None) == 0
    assert lib.rf_maxpool_points_lengths(2, 100, 0, None, None, None, None, 0, None) == 0
    assert lib.rf_merge_layer_lengths(0, 100, 10, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.rf_merge_layer_lengths(2, 100, 0, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.rf_merge_layer_grad_lengths(0, 100, 10, None, None, None, None, None, None, None, None, None, None, None) == 0


def _each(call, need, args, required, counts, workspace):
    """call(args, workspace_bytes): NULL in a required slot, a misaligned count array or workspace are RF_EINVAL; a NULL count
    array ("all") is not -- seen with a workspace one byte short, so that no call here ever gets as far as a launch (these
    tests run on machines with a device too)."""
    for k in required:
        a = list(args)
        a[k] = None
        assert call(a, need) == RF_EINVAL, ("NULL", k)
    for k in counts:
        a = list(args)
        a[k] = ODD
        assert call(a, need) == RF_EINVAL, ("misaligned count", k)
        a[k] = None  # "all"
        assert call(a, need - 1) == RF_EWORKSPACE, ("NULL count", k)
    a = list(args)
    a[workspace] = W8
    assert call(a, need) == RF_EINVAL, "misaligned workspace"
    assert call(list(args), need - 1) == RF_EWORKSPACE


def test_pool_argument_checks(lib):
    b, n, c = 6, 600, 64
    f, need = lib.rf_maxpool_points_lengths, lib.rf_maxpool_points_lengths_workspace_bytes(b, n, c)
    # x, len, out, workspace
    _each(lambda a, w: f(b, n, c, a[0], a[1], a[2], a[3], w, None), need, [P] * 4, required=(0, 2, 3), counts=(1,), workspace=3)
    g, gneed = lib.rf_maxpool_points_idx_lengths, lib.rf_maxpool_points_idx_lengths_workspace_bytes(b, n, c)
    # x, len, out, idx, workspace
    _each(lambda a, w: g(b, n, c, a[0], a[1], a[2], a[3], a[4], w, None), gneed, [P] * 5, required=(0, 2, 3, 4), counts=(1,),
          workspace=4)
    assert g(b, n, c, P, P, P, P, P, need, None) == RF_EWORKSPACE  # the values-only size is half of what idx needs
    # the dense entries' rules on the feature tensor: rows of c % 4 == 0 <= 1024 floats, 16-byte aligned
    for bad_c in (6, 1028, 2048):
        assert f(b, n, bad_c, P, P, P, P, BIG, None) == RF_EINVAL and g(b, n, bad_c, P, P, P, P, P, BIG, None) == RF_EINVAL
    assert f(b, n, c, W8, P, P, P, BIG, None) == RF_EINVAL and g(b, n, c, W8, P, P, P, P, BIG, None) == RF_EINVAL
    assert f(b, n, c, P, P, ODD, P, BIG, None) == RF_EINVAL and g(b, n, c, P, P, P, ODD, P, BIG, None) == RF_EINVAL
    assert f(65536, n, c, P, P, P, P, BIG, None) == RF_EINVAL
    # (1024 channels and a 4-byte aligned `out` are fine: what stops these is the short workspace)
    assert f(b, n, 1024, P, P, W8, P, 16, None) == RF_EWORKSPACE and g(b, n, 1024, P, P, W8, W8, P, 16, None) == RF_EWORKSPACE


@pytest.mark.parametrize("b,n,m", [(3, 300, 257), (4, 2048, 2048)])  # the dense sweep's shape, the culled sweep's
def test_merge_argument_checks(lib, b, n, m):
    f, need = lib.rf_merge_layer_lengths, lib.rf_merge_layer_lengths_workspace_bytes(b, n, m)
    # rawpts, newpts, len_raw, len_new, decfactor, refined, idx2, workspace
    _each(lambda a, w: f(b, n, m, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], w, None), need, [P] * 8,
          required=(0, 1, 4, 5, 6, 7), counts=(2, 3), workspace=7)
    assert f(b, n, m, P, P, None, None, P, P, P, P, _align256(b * m * 4), None) == RF_EWORKSPACE
    g = lib.rf_merge_layer_grad_lengths
    # rawpts, newpts, len_raw, len_new, decfactor, idx2, grad_refined, grad_newpts, grad_dec, grad_raw
    for k in (0, 1, 4, 5, 6, 7, 8):
        a = [P] * 10
        a[k] = None
        assert g(b, n, m, *a, None) == RF_EINVAL, ("NULL", k)
    for k in (2, 3):
        a = [P] * 10
        a[k] = ODD
        assert g(b, n, m, *a, None) == RF_EINVAL, ("misaligned count", k)


# ---- Python wrappers: host-side validation raises before any device work ------------------------------------------
def _wrappers(l_feat, l_raw, l_new):
    """Every wrapper on CPU arrays: `l_feat` counts the 40 rows of a (3, 40, 8) feature tensor, `l_raw` the 80 raw points,
    `l_new` the 25 new points."""
    import torch

    from rfnet_amd import _raw, glue
    from rfnet_amd import rfnet
    rng = np.random.RandomState(0)
    raw, new = rng.randn(3, 80, 3).astype(np.float32), rng.randn(3, 25, 3).astype(np.float32)
    x = torch.from_numpy(rng.randn(3, 40, 8).astype(np.float32))
    idx, go = np.zeros((3, 25), np.int32), np.ones((3, 25, 3), np.float32)
    calls = []
    if l_feat is not None:
        calls += [lambda: _raw.maxpool_points(x, l_feat), lambda: _raw.maxpool_points_idx(x, l_feat),
                  lambda: rfnet.maxpool_points(x, l_feat)]
    if l_raw is not None or l_new is not None:
        calls += [lambda: _raw.merge_layer(raw, new, 0.1, lengths=l_raw, lengths_new=l_new),
                  lambda: _raw.merge_layer_grad(raw, new, 0.1, idx, go, lengths=l_raw, lengths_new=l_new)]
    if l_raw is not None:
        calls += [lambda: glue.merge_layer(torch.from_numpy(raw), torch.from_numpy(new), 0.1, lengths=l_raw),
                  lambda: glue.sampling(25, torch.from_numpy(raw), lengths=l_raw)]
    return calls


@pytest.mark.parametrize("bad", [[1, 2], [1, 2, 3, 4], [0, 5, 5], [5, 81, 5], [-1, 5, 5], np.array([[1, 2, 3]]),
                                 [1.0, 2.0, 3.0], np.array([True, True, True])])
def test_host_counts_validated_first(bad):
    # ValueError from the argument check, not the missing-device RfopsError: nothing reached the GPU
    # ([5, 81, 5] is n + 1 for the raw cloud and beyond both other sizes)
    for call in _wrappers(bad, None, None) + _wrappers(None, bad, [25, 1, 3]) + _wrappers(None, None, bad):
        with pytest.raises(ValueError):
            call()


def test_counts_with_a_sorted_handle_rejected():
    import torch

    from rfnet_amd import _raw, glue
    rng = np.random.RandomState(0)
    raw, new = rng.randn(3, 80, 3).astype(np.float32), rng.randn(3, 25, 3).astype(np.float32)
    handle = object()  # never looked at: the combination itself is the error
    for kw in ({"lengths": [1, 2, 3]}, {"lengths_new": [1, 2, 3]}):
        with pytest.raises(ValueError, match="sorted"):
            _raw.merge_layer(raw, new, 0.1, sorted_raw=handle, **kw)
    with pytest.raises(ValueError, match="sorted"):
        glue.merge_layer(torch.from_numpy(raw), torch.from_numpy(new), 0.1, sorted_raw=handle, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="'r'"):
        glue.sampling(25, torch.from_numpy(raw), use_type="r", lengths=[80, 80, 80])


@pytest.mark.parametrize("bad", [[31, 100, 100], [100, 101, 100], [0, 100, 100], [100, 100], [50.0, 50.0, 50.0]])
def test_network_forward_validates_host_counts(bad):
    """The graph draws 32 FPS samples per cloud: 32 <= lengths[i] <= N, found before any layer runs (a CPU module here, which
    could not run the HIP operators at all)."""
    import torch

    from rfnet_amd.rfnet import RFNet
    net = RFNet()
    cloud = torch.zeros(3, 100, 3)
    for conv in (list, np.array, torch.tensor):
        with pytest.raises(ValueError):
            net(cloud, lengths=conv(bad))
    import inspect
    assert "lengths" in inspect.signature(RFNet.forward).parameters
    assert "lengths" in inspect.signature(RFNet.pooled).parameters
