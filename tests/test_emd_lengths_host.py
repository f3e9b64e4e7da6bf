"""CPU checks of the ragged-batch EMD entries (include/rfops.h rf_approxmatch_lengths, rf_matchcost_lengths,
rf_matchcost_grad_lengths, rf_earth_mover_lengths) and of their Python wrappers: the symbols are exported, the workspace
sizes follow the pinned route, every argument error comes back before any HIP call, and host-given lengths are validated
before any device work -- so these run without a device (pointers here are never dereferenced)."""
import ctypes

import numpy as np
import pytest

RF_EINVAL, RF_EWORKSPACE = -1, -2  # include/rfops.h
RF_EMD_SWEPT = 1

P = ctypes.c_void_p(1 << 20)  # a 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p((1 << 20) + 2)
ODD8 = ctypes.c_void_p((1 << 20) + 8)  # 4-byte but not 16-byte aligned
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from rfnet_amd import _lib
    return _lib.lib


def _levels(*v):
    return (ctypes.c_float * len(v))(*v)


def test_symbols_exported(lib):
    for name in ("rf_approxmatch_lengths_workspace_bytes", "rf_approxmatch_lengths", "rf_matchcost_lengths_workspace_bytes",
                 "rf_matchcost_lengths", "rf_matchcost_grad_lengths", "rf_earth_mover_lengths_workspace_bytes",
                 "rf_earth_mover_lengths"):
        assert hasattr(lib, name), name


def test_workspace_sizes(lib):
    for b, n, m in ((0, 100, 10), (2, 0, 10), (2, 100, 0), (-1, 10, 10)):
        assert lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, 0) == 0, (b, n, m)
        assert lib.rf_matchcost_lengths_workspace_bytes(b, n, m) == 0, (b, n, m)
        assert lib.rf_earth_mover_lengths_workspace_bytes(b, n, m) == 0, (b, n, m)
    assert lib.rf_approxmatch_lengths_workspace_bytes(2, 100, 10, -1) == 0  # no such schedule
    assert lib.rf_approxmatch_lengths_workspace_bytes(2, 100, 10, 65) == 0
    for b, n, m in ((1, 1, 1), (3, 64, 64), (2, 256, 200), (2, 777, 130), (32, 2048, 2048), (4, 16384, 16384)):
        for nl in (0, 10, 7, 50):
            w = lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, nl)
            # the pinned route's own workspace
            assert w > 0 and w == lib.rf_approxmatch_mode_workspace_bytes(b, n, m, nl, RF_EMD_SWEPT), (b, n, m, nl)
        assert lib.rf_matchcost_lengths_workspace_bytes(b, n, m) == lib.rf_matchcost_workspace_bytes(b, n, m) > 0
        assert (lib.rf_earth_mover_lengths_workspace_bytes(b, n, m)
                == lib.rf_earth_mover_mode_workspace_bytes(b, n, m, RF_EMD_SWEPT) > 0)


@pytest.mark.parametrize("b,n,m", [(-1, 10, 10), (2, -5, 10), (2, 10, -5), (2, 0, 10), (2, 10, 0), (65536, 10, 10)])
def test_bad_sizes_are_einval(lib, b, n, m):
    assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, None, 0, P, BIG, None) == RF_EINVAL
    assert lib.rf_matchcost_lengths(b, n, m, P, P, P, P, P, P, P, BIG, None) == RF_EINVAL
    assert lib.rf_matchcost_grad_lengths(b, n, m, P, P, P, P, P, P, P, None) == RF_EINVAL
    assert lib.rf_earth_mover_lengths(b, n, m, P, P, P, P, P, P, P, P, BIG, None) == RF_EINVAL


def test_empty_batch_is_ok(lib):
    assert lib.rf_approxmatch_lengths(0, 10, 10, None, None, None, None, None, None, 0, None, 0, None) == 0
    assert lib.rf_matchcost_lengths(0, 10, 10, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.rf_matchcost_grad_lengths(0, 10, 10, None, None, None, None, None, None, None, None) == 0
    assert lib.rf_earth_mover_lengths(0, 10, 10, None, None, None, None, None, None, None, None, 0, None) == 0


def test_approxmatch_argument_checks(lib):
    b, n, m = 2, 999, 301
    need = lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, 0)
    f = lib.rf_approxmatch_lengths
    for k in (0, 1, 4):  # xyz1, xyz2, match
        args = [P] * 5
        args[k] = None
        assert f(b, n, m, *args, None, 0, P, need, None) == RF_EINVAL, k
    assert f(b, n, m, P, P, P, P, P, None, 0, None, need, None) == RF_EINVAL  # no workspace
    assert f(b, n, m, P, P, ODD, P, P, None, 0, P, need, None) == RF_EINVAL  # misaligned counts
    assert f(b, n, m, P, P, P, ODD, P, None, 0, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, None, 0, ODD8, need, None) == RF_EINVAL  # misaligned workspace
    assert f(b, n, m, P, P, P, P, P, None, 0, P, need - 1, None) == RF_EWORKSPACE
    assert f(b, n, m, None, None, None, None, P, None, 0, P, need - 1, None) == RF_EINVAL  # (the tensors first)
    # NULL counts are "all points": valid arguments up to the workspace check
    assert f(b, n, m, P, P, None, None, P, None, 0, P, 0, None) == RF_EWORKSPACE


@pytest.mark.parametrize("levels", [(-4.0, 0.5, 0.0), (-4.0, float("nan")), (float("-inf"), 0.0), (float("inf"),), (1e-30,)])
def test_approxmatch_bad_schedules(lib, levels):
    b, n, m = 2, 999, 301
    lv = _levels(*levels)
    assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, lv, len(levels), P, BIG, None) == RF_EINVAL
    # (before the batch is looked at, as the existing entries check their schedule)
    assert lib.rf_approxmatch_lengths(0, n, m, P, P, P, P, P, lv, len(levels), P, BIG, None) == RF_EINVAL


def test_approxmatch_schedule_bounds(lib):
    b, n, m = 2, 300, 301
    assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, None, 3, P, BIG, None) == RF_EINVAL  # levels missing
    assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, _levels(*[-1.0] * 65), 65, P, BIG, None) == RF_EINVAL
    assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, _levels(-1.0), -1, P, BIG, None) == RF_EINVAL
    # admissible schedules reach the workspace check (0 and -0 are multipliers the reference uses)
    for lv in ((-16.0, -4.0, -0.0), (0.0,), tuple([-1.0] * 64)):
        assert lib.rf_approxmatch_lengths(b, n, m, P, P, P, P, P, _levels(*lv), len(lv), P, 0, None) == RF_EWORKSPACE, lv


def test_matchcost_argument_checks(lib):
    b, n, m = 2, 999, 301
    need = lib.rf_matchcost_lengths_workspace_bytes(b, n, m)
    f = lib.rf_matchcost_lengths
    for k in (0, 1, 4, 5, 6):  # xyz1, xyz2, match, cost, workspace
        args = [P] * 7
        args[k] = None
        assert f(b, n, m, *args, need, None) == RF_EINVAL, k
    assert f(b, n, m, P, P, ODD, P, P, P, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, ODD, P, P, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, ODD8, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, P, need - 1, None) == RF_EWORKSPACE
    g = lib.rf_matchcost_grad_lengths
    for k in (0, 1, 4, 5, 6):  # xyz1, xyz2, match, grad1, grad2: every one needed
        args = [P] * 7
        args[k] = None
        assert g(b, n, m, *args, None) == RF_EINVAL, k
    assert g(b, n, m, P, P, ODD, P, P, P, P, None) == RF_EINVAL
    assert g(b, n, m, P, P, P, ODD, P, P, P, None) == RF_EINVAL


def test_earth_mover_argument_checks(lib):
    b, n, m = 2, 999, 301
    need = lib.rf_earth_mover_lengths_workspace_bytes(b, n, m)
    f = lib.rf_earth_mover_lengths
    for k in (0, 1, 4, 7):  # xyz1, xyz2, cost, workspace
        args = [P] * 8
        args[k] = None
        assert f(b, n, m, *args, need, None) == RF_EINVAL, k
    assert f(b, n, m, P, P, P, P, P, P, None, P, need, None) == RF_EINVAL  # one gradient of the pair
    assert f(b, n, m, P, P, P, P, P, None, P, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, ODD, P, P, P, P, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, ODD, P, P, P, P, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, P, ODD8, need, None) == RF_EINVAL
    assert f(b, n, m, P, P, P, P, P, P, P, P, need - 1, None) == RF_EWORKSPACE
    assert f(b, n, m, P, P, P, P, P, None, None, P, need - 1, None) == RF_EWORKSPACE  # the cost alone
    assert f(4, 16384, 16384, P, P, P, P, P, P, P, P, 0, None) == RF_EWORKSPACE


# ---- Python wrappers: host-side validation raises before any device work ------------------------------------------
def _clouds(b=3, n=40, m=25):
    rng = np.random.RandomState(0)
    return rng.randn(b, n, 3).astype(np.float32), rng.randn(b, m, 3).astype(np.float32)


@pytest.mark.parametrize("bad", [[1, 2], [1, 2, 3, 4], [0, 5, 5], [5, 41, 5], [-1, 5, 5], np.array([[1, 2, 3]]),
                                 [1.0, 2.0, 3.0], np.array([True, True, True])])
def test_raw_host_lengths_validated_first(bad):
    from rfnet_amd import _raw
    a, c = _clouds()
    match = np.zeros((3, 25, 40), np.float32)
    # ValueError from the argument check, not the missing-device RfopsError: nothing reached the GPU
    with pytest.raises(ValueError):
        _raw.approx_match(a, c, lengths1=bad)
    with pytest.raises(ValueError):
        _raw.approx_match(a, c, levels=[-1.0, 0.0], mode="swept", lengths1=bad, lengths2=[25, 1, 3])
    with pytest.raises(ValueError):
        _raw.match_cost(a, c, match, lengths1=bad)
    with pytest.raises(ValueError):
        _raw.match_cost_grad(a, c, match, lengths1=bad, lengths2=[25, 1, 3])
    with pytest.raises(ValueError):
        _raw.earth_mover(a, c, lengths1=bad)
    with pytest.raises(ValueError):
        _raw.earth_mover(a, c, with_grad=True, lengths1=[40, 1, 17], lengths2=bad if np.asarray(bad).dtype.kind == "f"
                         else [26, 1, 1])


def test_raw_lengths_shape_checks_first():
    from rfnet_amd import _raw
    a, c = _clouds()
    with pytest.raises(ValueError):  # match of the wrong shape: the reference's own check, before the counts
        _raw.match_cost(a, c, np.zeros((3, 40, 25), np.float32), lengths1=[1, 2, 3])
    with pytest.raises(ValueError):
        _raw.approx_match(a, c, mode="fast", lengths1=[1, 2, 3])


def test_glue_and_module_validate_host_lengths():
    import torch

    from rfnet_amd import glue
    from rfnet_amd.pc_distance import tf_approxmatch
    a, c = (torch.from_numpy(x) for x in _clouds())
    with pytest.raises(ValueError):
        tf_approxmatch.earth_mover_cost(a, c, lengths1=[0, 1, 1])
    with pytest.raises(ValueError):
        glue.earth_mover(a, c, lengths2=[26, 1, 1])


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
        _raw.approx_match(a, c, lengths1=x)
    with pytest.raises(_lib.RfopsError):
        _raw.match_cost(a, c, np.zeros((3, 25, 40), np.float32), lengths1=x)
    with pytest.raises(_lib.RfopsError):
        _raw.match_cost_grad(a, c, np.zeros((3, 25, 40), np.float32), lengths1=x)
    with pytest.raises(_lib.RfopsError):
        _raw.earth_mover(a, c, with_grad=True, lengths1=x)
