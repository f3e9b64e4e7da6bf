"""CPU checks of the ragged-batch entries of sampling, grouping and neighbour search (include/rfops.h:
rf_farthestpointsampling_lengths, rf_queryballpoint_lengths, rf_sample_and_group_lengths, rf_threenn_lengths, rf_knn_lengths,
rf_knn_grad_lengths) and of their Python wrappers: the symbols are exported and bound, the workspace sizes follow the route,
every argument error comes back before any HIP call, and host-given counts are validated before any device work -- so these
run without a device (pointers here are never dereferenced)."""
import ctypes

import numpy as np
import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h
AUTO, SCAN, BOXES = 0, 1, 2        # RF_GROUP_*

P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p((1 << 20) + 2)
W8 = ctypes.c_void_p((1 << 20) + 8)  # 4-byte aligned, not 16
BIG = 1 << 40

ENTRIES = ("rf_farthestpointsampling_lengths_workspace_bytes", "rf_farthestpointsampling_lengths",
           "rf_queryballpoint_lengths_workspace_bytes", "rf_queryballpoint_lengths",
           "rf_sample_and_group_lengths_workspace_bytes", "rf_sample_and_group_lengths",
           "rf_threenn_lengths_workspace_bytes", "rf_threenn_lengths",
           "rf_knn_lengths_workspace_bytes", "rf_knn_lengths", "rf_knn_grad_lengths_workspace_bytes", "rf_knn_grad_lengths")


@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


def test_symbols_exported_and_bound(lib):
    from rfnet_amd import _lib
    header = open(__file__.replace("tests/test_group_lengths_host.py", "include/rfops.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    for macro in ("RF_GROUP_AUTO 0", "RF_GROUP_SCAN 1", "RF_GROUP_BOXES 2"):
        assert "#define " + macro in header


def test_workspace_sizes(lib):
    fps, qb, sag, tn, kn, kg = (getattr(lib, n) for n in ENTRIES[0::2])
    for b, n, m in ((0, 100, 10), (2, 0, 10), (2, 100, 0), (-1, 10, 10)):
        assert fps(b, n, m) == 0 and qb(b, n, m, 32, BOXES) == 0 and tn(b, n, m, BOXES) == 0, (b, n, m)
        assert kn(b, n, m, 1, BOXES) == 0 and kg(b, n, m, 1) == 0, (b, n, m)
    assert sag(0, 100) == 0 and sag(2, 0) == 0 and sag(2, 63) == 0 and sag(2, 65537) == 0
    # FPS: the routes of rf_farthestpointsampling_ws on the padded sizes
    for b, n, m in ((2, 700, 64), (2, 3000, 512), (32, 16384, 1024), (2, 40000, 64), (2, 16384, 64)):
        assert fps(b, n, m) == lib.rf_farthestpointsampling_workspace_bytes(b, n, m), (b, n, m)
    assert fps(32, 16384, 1024) > 0 and fps(2, 40000, 64) == 4 * 2 * 40000 and fps(2, 700, 64) == 0
    # ball query: scratch for the boxed form only; auto takes it from 2048 dataset points on; outside its domain: nothing
    assert qb(2, 999, 301, 32, SCAN) == 0 and qb(2, 999, 301, 32, AUTO) == 0 and qb(2, 16384, 301, 32, SCAN) == 0
    assert qb(2, 999, 301, 32, BOXES) == lib.rf_queryballpoint_boxes_workspace_bytes(2, 999) > 0
    assert qb(2, 2048, 301, 32, AUTO) == qb(2, 2048, 301, 32, BOXES) > 0
    assert qb(2, 63, 301, 32, BOXES) == 0 and qb(2, 999, 301, 65, BOXES) == 0 and qb(2, 999, 301, 32, 7) == 0
    assert qb(2, 4096, 301, 65, AUTO) == 0  # (auto outside the boxed domain: the scan)
    assert sag(2, 999) == lib.rf_sample_and_group_workspace_bytes(2, 999) > 0
    # three_nn / knn: the two sorted sets for the boxed form
    assert tn(2, 999, 301, SCAN) == 0 and tn(2, 999, 301, AUTO) == 0 and tn(2, 999, 301, 7) == 0
    assert tn(2, 999, 301, BOXES) == lib.rf_threenn_boxes_workspace_bytes(2, 999, 301) > 0
    assert tn(32, 16384, 1024, AUTO) == tn(32, 16384, 1024, BOXES) > 0
    assert tn(2, 65537, 301, BOXES) == 0 and tn(65536, 10, 10, BOXES) == 0
    assert kn(2, 999, 301, 16, SCAN) == 0 and kn(2, 999, 301, 16, AUTO) == 0 and kn(2, 999, 301, 16, 7) == 0
    assert kn(2, 999, 301, 16, BOXES) == lib.rf_knn_boxes_workspace_bytes(2, 999, 301) > 0
    assert kn(8, 16384, 8192, 16, AUTO) == kn(8, 16384, 8192, 16, BOXES) > 0 and kn(8, 16384, 8192, 64, AUTO) == 0
    assert kn(2, 10, 301, 11, BOXES) == 0 and kn(2, 999, 301, 65, BOXES) == 0
    assert kg(2, 999, 301, 16) == lib.rf_knn_grad_workspace_bytes(2, 999, 301, 16) > 0


def _calls(lib, b, n, m):
    """Every entry on never-dereferenced pointers with ample workspaces."""
    return [lib.rf_farthestpointsampling_lengths(b, n, m, P, P, P, P, BIG, P, P, None),
            lib.rf_queryballpoint_lengths(b, n, m, 0.1, None, 16, P, P, P, P, P, P, P, BIG, None, AUTO),
            lib.rf_sample_and_group_lengths(b, n, m, 0.1, None, 16, P, P, P, P, P, P, P, P, P, BIG, None, None),
            lib.rf_threenn_lengths(b, n, m, P, P, P, P, P, P, P, BIG, None, AUTO),
            lib.rf_knn_lengths(b, n, m, 1, P, P, P, P, P, P, P, BIG, None, AUTO),
            lib.rf_knn_grad_lengths(b, n, m, 1, P, P, P, P, P, P, P, P, P, BIG, None)]


@pytest.mark.parametrize("b,n,m", [(-1, 100, 10), (2, -5, 10), (2, 100, -5), (2, 0, 10), (2, 100, 0)])
def test_bad_sizes_are_einval(lib, b, n, m):
    assert _calls(lib, b, n, m) == [RF_EINVAL] * 6


def test_empty_batch_is_ok(lib):
    assert lib.rf_farthestpointsampling_lengths(0, 100, 10, None, None, None, None, 0, None, None, None) == 0
    assert lib.rf_queryballpoint_lengths(0, 100, 10, 0.1, None, 16, None, None, None, None, None, None, None, 0, None, AUTO) == 0
    assert lib.rf_sample_and_group_lengths(0, 100, 10, 0.1, None, 16, None, None, None, None, None, None, None, None, None, 0,
                                           None, None) == 0
    assert lib.rf_threenn_lengths(0, 100, 10, None, None, None, None, None, None, None, 0, None, AUTO) == 0
    assert lib.rf_knn_lengths(0, 100, 10, 1, None, None, None, None, None, None, None, 0, None, AUTO) == 0
    assert lib.rf_knn_grad_lengths(0, 100, 10, 1, None, None, None, None, None, None, None, None, None, 0, None) == 0


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


def test_fps_argument_checks(lib):
    f = lib.rf_farthestpointsampling_lengths
    b, n, m = 2, 16384, 1024  # the sorted route: needs scratch
    need = lib.rf_farthestpointsampling_lengths_workspace_bytes(b, n, m)
    # inp, len, len_out, workspace, out, new_xyz
    _each(lambda a, w: f(b, n, m, a[0], a[1], a[2], a[3], w, a[4], a[5], None), need, [P] * 6, required=(0, 3, 4),
          counts=(1, 2), workspace=3)
    assert f(b, n, m, P, P, P, P, need - 1, P, None, None) == RF_EWORKSPACE  # new_xyz may be NULL
    assert f(2, 40000, 64, P, P, P, P, 4 * 2 * 40000 - 1, P, P, None) == RF_EWORKSPACE
    assert f(2, 40000, 64, P, P, P, None, 0, P, P, None) == RF_EINVAL
    assert f(b, n, m, ODD, P, P, P, need, P, P, None) == RF_EINVAL and f(b, n, m, P, P, P, P, need, ODD, P, None) == RF_EINVAL


def test_ball_query_argument_checks(lib):
    f = lib.rf_queryballpoint_lengths
    b, n, m, ns = 2, 4096, 301, 32
    need = lib.rf_queryballpoint_lengths_workspace_bytes(b, n, m, ns, BOXES)
    # xyz1, xyz2, len1, len2, idx, pts_cnt, workspace
    _each(lambda a, w: f(b, n, m, 0.1, None, ns, a[0], a[1], a[2], a[3], a[4], a[5], a[6], w, None, BOXES), need, [P] * 7,
          required=(0, 1, 4, 5, 6), counts=(2, 3), workspace=6)
    assert f(b, n, m, 0.1, None, ns, P, P, P, P, P, P, P, need - 1, None, AUTO) == RF_EWORKSPACE
    assert f(b, n, m, 0.1, ODD, ns, P, P, P, P, P, P, P, need, None, BOXES) == RF_EINVAL  # the device radius
    assert f(b, n, m, 0.1, None, 0, P, P, P, P, P, P, P, need, None, BOXES) == RF_EINVAL
    assert f(b, n, m, 0.1, None, ns, P, P, P, P, P, P, P, need, None, 9) == RF_EINVAL
    # boxes outside its domain
    assert f(b, 63, m, 0.1, None, ns, P, P, P, P, P, P, P, BIG, None, BOXES) == RF_EINVAL
    assert f(b, n, m, 0.1, None, 65, P, P, P, P, P, P, P, BIG, None, BOXES) == RF_EINVAL
    assert f(b, 65537, m, 0.1, None, ns, P, P, P, P, P, P, P, BIG, None, BOXES) == RF_EINVAL


def test_sample_and_group_argument_checks(lib):
    f = lib.rf_sample_and_group_lengths
    b, n, m, ns = 2, 4096, 301, 32
    need = lib.rf_sample_and_group_lengths_workspace_bytes(b, n)
    # xyz, len, len_out, fps_idx, new_xyz, idx, pts_cnt, grouped_xyz, workspace
    _each(lambda a, w: f(b, n, m, 0.1, None, ns, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], w, None, None), need,
          [P] * 9, required=(0, 3, 4, 5, 6, 7, 8), counts=(1, 2), workspace=8)
    for bad in ((b, 63, m, ns), (b, 65537, m, ns), (b, n, m, 65), (b, n, m, 0), (65536, n, m, ns)):
        assert f(bad[0], bad[1], bad[2], 0.1, None, bad[3], P, P, P, P, P, P, P, P, P, BIG, None, None) == RF_EINVAL, bad


def test_three_nn_argument_checks(lib):
    f = lib.rf_threenn_lengths
    b, n, m = 2, 4096, 301
    need = lib.rf_threenn_lengths_workspace_bytes(b, n, m, BOXES)
    # xyz1, xyz2, len1, len2, dist, idx, workspace
    _each(lambda a, w: f(b, n, m, a[0], a[1], a[2], a[3], a[4], a[5], a[6], w, None, BOXES), need, [P] * 7,
          required=(0, 1, 4, 5, 6), counts=(2, 3), workspace=6)
    assert f(b, n, m, P, P, P, P, P, P, P, need, None, 9) == RF_EINVAL
    assert f(b, 65537, m, P, P, P, P, P, P, P, BIG, None, BOXES) == RF_EINVAL
    assert f(65536, n, m, P, P, P, P, P, P, P, BIG, None, SCAN) == RF_EINVAL


def test_knn_argument_checks(lib):
    f = lib.rf_knn_lengths
    b, n, m, k = 2, 4096, 301, 16
    need = lib.rf_knn_lengths_workspace_bytes(b, n, m, k, BOXES)
    # xyz1, xyz2, len1, len2, val, idx, workspace
    _each(lambda a, w: f(b, n, m, k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], w, None, BOXES), need, [P] * 7,
          required=(0, 1, 4, 5, 6), counts=(2, 3), workspace=6)
    assert f(b, n, m, k, P, P, P, P, P, P, P, need, None, 9) == RF_EINVAL
    for bad in ((b, n, m, 0), (b, n, m, 65), (b, 10, m, 11), (b, 65537, m, k), (b, n, 65537, k), (65536, n, m, k)):
        assert f(bad[0], bad[1], bad[2], bad[3], P, P, P, P, P, P, P, BIG, None, SCAN) == RF_EINVAL, bad
    g = lib.rf_knn_grad_lengths
    gneed = lib.rf_knn_grad_lengths_workspace_bytes(b, n, m, k)
    # xyz1, xyz2, len1, len2, idx, grad_val, grad_xyz1, grad_xyz2, workspace
    _each(lambda a, w: g(b, n, m, k, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], w, None), gneed, [P] * 9,
          required=(0, 1, 4, 5, 6, 7, 8), counts=(2, 3), workspace=8)
    assert g(b, 10, m, 11, P, P, P, P, P, P, P, P, P, BIG, None) == RF_EINVAL


# ---- Python wrappers: host-side validation raises before any device work ------------------------------------------
def _clouds(b=3, n=80, m=25):
    rng = np.random.RandomState(0)
    return rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


def _wrappers(a, c, l1, l2):
    """Every wrapper with `l1` as the count of the (3, 80, 3) cloud and `l2` as the count of the 25 queries / samples."""
    from rfnet_amd import _raw
    idx = np.zeros((3, 25, 4), np.int32)
    return [lambda: _raw.farthest_point_sample(25, a, lengths=l1, npoints=l2),
            lambda: _raw.query_ball_point(0.3, 8, a, c, lengths1=l1, lengths2=l2),
            lambda: _raw.sample_and_group(25, 0.3, 8, a, lengths=l1, npoints=l2),
            lambda: _raw.three_nn(c, a, lengths1=l2, lengths2=l1),
            lambda: _raw.knn_point(4, a, c, lengths1=l1, lengths2=l2),
            lambda: _raw.knn_point_grad(a, c, idx, np.ones((3, 25, 4), np.float32), lengths1=l1, lengths2=l2)]


@pytest.mark.parametrize("bad", [[1, 2], [1, 2, 3, 4], [0, 5, 5], [5, 81, 5], [-1, 5, 5], np.array([[1, 2, 3]]),
                                 [1.0, 2.0, 3.0], np.array([True, True, True])])
def test_raw_host_counts_validated_first(bad):
    a, c = _clouds()
    # ValueError from the argument check, not the missing-device RfopsError: nothing reached the GPU
    for call in _wrappers(a, c, bad, [25, 1, 3]) + _wrappers(a, c, None, bad):
        with pytest.raises(ValueError):
            call()


def test_raw_counts_with_sorted_handles_rejected():
    from rfnet_amd import _raw
    a, c = _clouds()
    handle = object()  # never looked at: the combination itself is the error
    with pytest.raises(ValueError, match="sorted"):
        _raw.query_ball_point(0.3, 8, a, c, sorted1=handle, lengths1=[1, 2, 3])
    for kw in ({"sorted1": handle}, {"sorted2": handle}):
        with pytest.raises(ValueError, match="sorted"):
            _raw.three_nn(c, a, lengths1=[1, 2, 3], **kw)
        with pytest.raises(ValueError, match="sorted"):
            _raw.knn_point(4, a, c, lengths2=[1, 2, 3], **kw)


def test_drop_in_modules_take_the_counts():
    import inspect

    from rfnet_amd.tf_ops.grouping import tf_grouping
    from rfnet_amd.tf_ops.interpolation import tf_interpolate
    from rfnet_amd.tf_ops.sampling import tf_sampling
    # (the two signatures that tests/test_boundary.py pins to the reference's keep them: their ragged forms are siblings)
    assert {"lengths", "npoints"} <= set(inspect.signature(tf_sampling.farthest_point_sample_lengths).parameters)
    for fn in (tf_grouping.query_ball_point_lengths, tf_grouping.knn_point, tf_interpolate.three_nn):
        assert {"lengths1", "lengths2", "form"} <= set(inspect.signature(fn).parameters), fn
    a, c = _clouds()
    for call in (lambda: tf_sampling.farthest_point_sample_lengths(25, a, lengths=[0, 1, 1]),
                 lambda: tf_grouping.query_ball_point_lengths(0.3, 8, a, c, lengths1=[81, 1, 1]),
                 lambda: tf_interpolate.three_nn(c, a, lengths2=[1, 2]),
                 lambda: tf_grouping.knn_point(4, a, c, lengths1=[1, 2, 3])):  # (the tensor expression does not take counts)
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("fmt", ["list", "tuple", "numpy32", "numpy64", "torch32", "torch64"])
def test_raw_host_count_formats_pass_validation(fmt):
    """Every host format is accepted by the check: without a device what stops the call is the missing device itself
    (RfopsError), raised only after the arguments were found valid; with one, the call runs."""
    import torch

    from rfnet_amd import _lib
    a, c = _clouds()

    def conv(v):
        return {"list": v, "tuple": tuple(v), "numpy32": np.array(v, np.int32), "numpy64": np.array(v, np.int64),
                "torch32": torch.tensor(v, dtype=torch.int32), "torch64": torch.tensor(v, dtype=torch.int64)}[fmt]
    for call in _wrappers(a, c, conv([80, 1, 17]), conv([25, 1, 3])):
        if torch.cuda.is_available():
            call()
        else:
            with pytest.raises(_lib.RfopsError):
                call()
