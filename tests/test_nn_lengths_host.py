"""CPU checks of the ragged-batch Chamfer entries (include/rfops.h rf_nn_distance_lengths, rf_nn_distance_grad_lengths,
rf_chamfer_loss_lengths, rf_chamfer_loss_grad_lengths) and of their Python wrappers: the symbols are exported, the workspace
sizes follow the route, every argument error comes back before any HIP call, and host-given lengths are validated before any
device work -- so these run without a device (pointers here are never dereferenced)."""
import ctypes

import numpy as np
import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h
RF_NN_AUTO, RF_NN_DENSE, RF_NN_CULLED = 0, 1, 2

P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


def test_symbols_exported(lib):
    for name in ("rf_nn_distance_lengths_workspace_bytes", "rf_nn_distance_lengths", "rf_nn_distance_grad_lengths",
                 "rf_chamfer_loss_lengths_workspace_bytes", "rf_chamfer_loss_lengths", "rf_chamfer_loss_grad_lengths"):
        assert hasattr(lib, name), name


def test_workspace_sizes(lib):
    for b, n, m in ((0, 100, 10), (2, 0, 10), (2, 100, 0), (-1, 10, 10)):
        assert lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_AUTO) == 0, (b, n, m)
        assert lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, 1, 1) == 0, (b, n, m)
    assert lib.rf_nn_distance_lengths_workspace_bytes(2, 100, 10, 7) == 0  # unknown mode
    assert lib.rf_nn_distance_lengths_workspace_bytes(2, 65537, 10, RF_NN_CULLED) == 0  # beyond the culled sweep
    assert lib.rf_chamfer_loss_lengths_workspace_bytes(2, 100, 10, 0, 0) == 0  # no direction
    for b, n, m in ((1, 1, 1), (2, 999, 301), (32, 3000, 16384), (32, 16384, 16384), (1, 65536, 65536)):
        for mode in (RF_NN_AUTO, RF_NN_DENSE, RF_NN_CULLED):
            w = lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, mode)
            assert w > 0, (b, n, m, mode)
        # the dense route always re-packs the clouds: at least both padded copies
        assert lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_DENSE) >= 12 * b * (n + m)
        # the culled route: the culled sweep's own workspace (the padding is read as copies inside the sort)
        assert (lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_CULLED)
                == lib.rf_nn_distance_mode_workspace_bytes(b, n, m, RF_NN_CULLED))
        # AUTO routes by (n, m) exactly as rf_nn_distance does
        auto_culled = (lib.rf_nn_distance_mode_workspace_bytes(b, n, m, RF_NN_AUTO)
                       == lib.rf_nn_distance_mode_workspace_bytes(b, n, m, RF_NN_CULLED))
        pinned = RF_NN_CULLED if auto_culled else RF_NN_DENSE
        assert (lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_AUTO)
                == lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, pinned)), (b, n, m)
        # the loss needs no more than the forward of both directions
        for w1, w2 in ((1, 1), (1, 0), (0, 1)):
            lw = lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, w1, w2)
            assert 0 < lw <= lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_AUTO), (b, n, m, w1, w2)


@pytest.mark.parametrize("b,n,m", [(-1, 10, 10), (2, -5, 10), (2, 10, -5), (2, 0, 10), (2, 10, 0)])
def test_bad_sizes_are_einval(lib, b, n, m):
    assert lib.rf_nn_distance_lengths(b, n, m, P, P, P, P, P, P, P, P, P, BIG, None, RF_NN_AUTO) == RF_EINVAL
    assert lib.rf_nn_distance_grad_lengths(b, n, m, P, P, P, P, P, P, P, P, P, P, None) == RF_EINVAL
    assert lib.rf_chamfer_loss_lengths(b, n, m, P, P, P, P, P, P, P, P, P, P, BIG, None) == RF_EINVAL
    assert lib.rf_chamfer_loss_grad_lengths(b, n, m, P, P, P, P, P, P, P, P, P, P, P, None) == RF_EINVAL


def test_empty_batch_is_ok(lib):
    assert lib.rf_nn_distance_lengths(0, 10, 10, None, None, None, None, None, None, None, None, None, 0, None,
                                      RF_NN_AUTO) == 0
    assert lib.rf_chamfer_loss_lengths(0, 10, 10, None, None, None, None, None, None, None, None, None, None, 0,
                                       None) == 0


def test_pointer_alignment_and_workspace_checks(lib):
    b, n, m = 2, 999, 301
    need = lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, RF_NN_AUTO)
    lneed = lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, 1, 1)
    odd = ctypes.c_void_p((1 << 20) + 2)
    f = lib.rf_nn_distance_lengths
    # unknown mode, missing clouds, a half-given direction, no direction at all, no workspace
    assert f(b, n, m, P, P, P, P, P, P, P, P, P, need, None, 9) == RF_EINVAL
    assert f(b, n, m, None, P, P, P, P, P, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, None, P, P, P, P, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, None, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, None, None, None, None, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, P, P, None, need, None, RF_NN_AUTO) == RF_EINVAL
    # misaligned counts / outputs / workspace
    assert f(b, n, m, P, P, odd, P, P, P, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, odd, P, P, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, odd, P, P, P, P, need, None, RF_NN_AUTO) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, P, P, ctypes.c_void_p((1 << 20) + 8), need, None, RF_NN_AUTO) == RF_EINVAL
    # a short workspace
    assert f(b, n, m, P, P, P, P, P, P, P, P, P, need - 1, None, RF_NN_AUTO) == RF_EWORKSPACE
    assert f(b, n, m, P, P, None, None, P, P, None, None, P, 0, None, RF_NN_DENSE) == RF_EWORKSPACE
    # beyond the culled sweep's domain
    assert f(b, 65537, m, P, P, P, P, P, P, P, P, P, BIG, None, RF_NN_CULLED) == RF_EINVAL
    # the backward: every tensor needed (the counts may be NULL: "all points"), counts aligned
    g = lib.rf_nn_distance_grad_lengths
    for k in (0, 1, 4, 5, 6, 7, 8, 9):  # xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2, grad_xyz1, grad_xyz2
        args = [P] * 10
        args[k] = None
        assert g(b, n, m, *args, None) == RF_EINVAL, k
    assert g(b, n, m, P, P, odd, P, P, P, P, P, P, P, None) == RF_EINVAL
    # the loss
    L = lib.rf_chamfer_loss_lengths
    assert L(b, n, m, P, P, P, P, None, P, P, P, P, P, lneed, None) == RF_EINVAL  # no loss output
    assert L(b, n, m, P, P, P, P, P, None, None, None, None, P, lneed, None) == RF_EINVAL  # no direction
    assert L(b, n, m, P, P, P, P, P, P, P, P, P, None, lneed, None) == RF_EINVAL  # no workspace
    assert L(b, n, m, P, P, P, odd, P, P, P, P, P, P, lneed, None) == RF_EINVAL
    assert L(b, n, m, P, P, P, P, P, P, P, P, P, P, lneed - 1, None) == RF_EWORKSPACE
    G = lib.rf_chamfer_loss_grad_lengths
    assert G(b, n, m, P, P, P, P, P, P, P, P, None, P, P, None) == RF_EINVAL  # no grad_loss
    assert G(b, n, m, P, P, odd, P, P, P, P, P, P, P, P, None) == RF_EINVAL


# ---- Python wrappers: host-side validation raises before any device work ------------------------------------------
def _clouds(b=3, n=40, m=25):
    rng = np.random.RandomState(0)
    return rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


@pytest.mark.parametrize("bad", [[1, 2], [1, 2, 3, 4], [0, 5, 5], [5, 41, 5], [-1, 5, 5], np.array([[1, 2, 3]]),
                                 [1.0, 2.0, 3.0], np.array([True, True, True])])
def test_raw_host_lengths_validated_first(bad):
    from rfnet_amd import _raw
    a, c = _clouds()
    ok = [40, 1, 17]
    # ValueError from the argument check, not the missing-device RfopsError: nothing reached the GPU
    with pytest.raises(ValueError):
        _raw.nn_distance(a, c, lengths1=bad)
    with pytest.raises(ValueError):
        _raw.chamfer_loss(a, c, lengths1=bad, lengths2=[25, 1, 3])
    with pytest.raises(ValueError):
        _raw.chamfer_loss_grad(a, c, np.zeros((3, 40), np.float32), np.zeros((3, 40), np.int32), None, None,
                               np.ones((3, 2), np.float32), lengths1=bad)
    with pytest.raises(ValueError):
        _raw.nn_distance(a, c, lengths1=ok, lengths2=bad if np.asarray(bad).dtype.kind == "f" else [26, 1, 1])


def test_raw_lengths_with_sorted_handles_rejected():
    from rfnet_amd import _raw
    a, c = _clouds()
    handle = object()  # never looked at: the combination itself is the error
    with pytest.raises(ValueError, match="sorted"):
        _raw.chamfer_loss(a, c, handle, None, lengths1=[1, 2, 3])
    with pytest.raises(ValueError, match="sorted"):
        _raw.chamfer_loss(a, c, None, handle, lengths2=[1, 2, 3])


def test_raw_lengths_with_stats_rejected():
    from rfnet_amd import _raw
    a, c = _clouds()
    with pytest.raises(ValueError):
        _raw.nn_distance(a, c, stats=[], lengths1=[1, 2, 3])


@pytest.mark.parametrize("fmt", ["list", "tuple", "numpy32", "numpy64", "torch32", "torch64"])
def test_raw_host_length_formats_pass_validation(fmt):
    """Every host format is accepted by the check: what stops the call on a machine without a device is the missing
    device itself (RfopsError), raised only after the arguments were found valid."""
    import torch

    from rfnet_amd import _lib, _raw
    if torch.cuda.is_available():
        pytest.skip("this check is about the host-side path of a machine without a device")
    a, c = _clouds()
    v = [40, 1, 17]
    x = {"list": v, "tuple": tuple(v), "numpy32": np.array(v, np.int32), "numpy64": np.array(v, np.int64),
         "torch32": torch.tensor(v, dtype=torch.int32), "torch64": torch.tensor(v, dtype=torch.int64)}[fmt]
    with pytest.raises(_lib.RfopsError):
        _raw.nn_distance(a, c, lengths1=x)
