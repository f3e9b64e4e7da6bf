"""CPU checks of the knn_point C ABI (include/rfops.h rf_knn, rf_knn_boxes, rf_knn_grad): the symbols are exported, the
workspace sizes cover exactly the domain, and every argument error is returned before any HIP call -- so these run without a
device (pointers here are never dereferenced)."""
import ctypes

import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h


@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer


def test_symbols_exported(lib):
    for name in ("rf_knn", "rf_knn_boxes_workspace_bytes", "rf_knn_boxes", "rf_knn_grad_workspace_bytes", "rf_knn_grad"):
        assert hasattr(lib, name), name


def test_workspace_sizes(lib):
    for b, n, m in ((0, 100, 10), (2, 0, 10), (2, 100, 0), (2, 65537, 10), (2, 100, 65537), (65536, 10, 10)):
        assert lib.rf_knn_boxes_workspace_bytes(b, n, m) == 0, (b, n, m)
    assert lib.rf_knn_boxes_workspace_bytes(32, 16384, 1024) == lib.rf_nn_sort_bytes(32, 16384) + lib.rf_nn_sort_bytes(32, 1024)
    assert lib.rf_knn_boxes_workspace_bytes(1, 1, 1) > 0
    for b, n, m, k in ((2, 100, 10, 0), (2, 100, 10, 65), (2, 10, 10, 11), (2, 65537, 10, 4), (2, 100, 65537, 4), (0, 10, 10, 1)):
        assert lib.rf_knn_grad_workspace_bytes(b, n, m, k) == 0, (b, n, m, k)
    for b, n, m, k in ((1, 1, 1, 1), (32, 16384, 1024, 64), (1, 65536, 65536, 64)):
        assert lib.rf_knn_grad_workspace_bytes(b, n, m, k) > 0, (b, n, m, k)


@pytest.mark.parametrize("b,n,m,k", [(2, 100, 10, 0), (2, 100, 10, 65), (2, 10, 10, 11), (2, 65537, 10, 4),
                                     (2, 100, 65537, 4), (65536, 10, 10, 2), (-1, 10, 10, 2), (2, 100, 10, -3)])
def test_out_of_domain_is_einval(lib, b, n, m, k):
    big = 1 << 40
    assert lib.rf_knn(b, n, m, k, P, P, P, P, None) == RF_EINVAL
    assert lib.rf_knn_boxes(b, n, m, k, P, P, None, None, P, P, P, big, None) == RF_EINVAL
    assert lib.rf_knn_grad(b, n, m, k, P, P, P, P, P, P, P, big, None) == RF_EINVAL


def test_pointers_alignment_and_workspace(lib):
    b, n, m, k = 2, 500, 300, 16
    ws = 1 << 20
    need = lib.rf_knn_boxes_workspace_bytes(b, n, m)
    gneed = lib.rf_knn_grad_workspace_bytes(b, n, m, k)
    assert need > 0 and gneed > 0
    # NULL tensors
    assert lib.rf_knn(b, n, m, k, None, P, P, P, None) == RF_EINVAL
    assert lib.rf_knn(b, n, m, k, P, P, P, None, None) == RF_EINVAL
    # a short workspace
    assert lib.rf_knn_boxes(b, n, m, k, P, P, None, None, P, P, ws, need - 1, None) == RF_EWORKSPACE
    assert lib.rf_knn_grad(b, n, m, k, P, P, P, P, P, P, ws, gneed - 1, None) == RF_EWORKSPACE
    # a misaligned or missing workspace
    assert lib.rf_knn_boxes(b, n, m, k, P, P, None, None, P, P, ws + 4, need, None) == RF_EINVAL
    assert lib.rf_knn_boxes(b, n, m, k, P, P, None, None, P, P, None, need, None) == RF_EINVAL
    assert lib.rf_knn_grad(b, n, m, k, P, P, P, P, P, P, ws + 8, gneed, None) == RF_EINVAL
    assert lib.rf_knn_grad(b, n, m, k, P, P, P, P, P, P, None, gneed, None) == RF_EINVAL
    # a misaligned sort handle
    assert lib.rf_knn_boxes(b, n, m, k, P, P, ws + 8, None, P, P, ws, need, None) == RF_EINVAL
    assert lib.rf_knn_boxes(b, n, m, k, P, P, None, ws + 4, P, P, ws, need, None) == RF_EINVAL


def test_python_wrapper_rejects_out_of_domain_before_the_device():
    import torch
    from rfnet_amd import _raw as R
    x1, x2 = torch.zeros(1, 10, 3), torch.zeros(1, 4, 3)
    for k in (0, 11):
        with pytest.raises(ValueError):
            R.knn_point(k, x1, x2)
    with pytest.raises(ValueError):
        R.knn_point(3, torch.zeros(1, 10, 4), x2)
    with pytest.raises(ValueError):
        R.knn_point(3, x1, x2, form="dense")
