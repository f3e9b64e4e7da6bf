"""Raw (non-differentiable) calls into librfops.so, one per reference OpKernel.

Each function validates shapes with the reference OpKernel's own checks and wording
(`OP_REQUIRES(... errors::InvalidArgument(msg))`, cited per function), allocates outputs and
scratch on the caller's GPU (what TF's allocate_output / allocate_temp did), and enqueues the
HIP kernels on torch's current stream through the C ABI.  No computation happens in Python.
"""
import ctypes as C

import numpy as np
import torch

from . import _host as H
from ._lib import check, lib

F32, I32 = torch.float32, torch.int32


def _shape3(t, last=None):
    return t.dim() == 3 and (last is None or t.shape[2] == last)


# ------------------------------------------------------------------ Chamfer ----------------
NN_MODES = {"auto": 0, "dense": 1, "culled": 2}


def _check_lengths(x, b, n, name):
    """A per-sample count argument of the ragged entries (include/rfops.h, rf_nn_distance_lengths) -> None or a
    (b,) integer tensor.  Host-given counts (list, tuple, numpy array, CPU tensor) are checked here -- shape (b,),
    range [1, n] -- before any GPU work; CUDA counts are only shape-checked (reading them would synchronise: the
    kernels clamp them into [1, n] instead)."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.detach()  # (integer counts carry no graph; a CUDA tensor is used as it is)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise H.invalid(f"{name} must hold integer point counts")
    if t.dim() != 1 or t.shape[0] != b:
        raise H.invalid(f"{name} must be of shape (batch,)")
    if not t.is_cuda and b > 0 and (int(t.min()) < 1 or int(t.max()) > n):
        raise H.invalid(f"{name} must lie in [1, {n}]")
    return t


def _lengths_up(t, dev, n):
    """Stage checked counts as a contiguous int32 tensor on `dev` (CUDA counts are converted there, on the
    current stream: no host round trip).  Wider integers are clamped into [1, n] before the narrowing cast, so
    that a device value beyond the int32 range cannot wrap into the domain (the kernels clamp the rest)."""
    if t is None:
        return None
    if t.is_cuda and t.dtype == I32 and t.device == dev and t.is_contiguous():
        return t  # the common case of a training loop: nothing to convert (each conversion is host time per call)
    if t.is_cuda and t.device != dev:
        raise ValueError(f"all GPU inputs of one op must live on the same device: got {dev} and {t.device}")
    t = t.to(device=dev)
    if t.dtype != I32:
        t = t.clamp(1, max(n, 1)).to(I32)
    return t.contiguous()


@H.on_input_device
def nn_distance(xyz1, xyz2, mode="auto", stats=None, lengths1=None, lengths2=None):
    """NnDistanceGpuOp::Compute, tf_ops/CD/tf_nndistance.cpp:172-204.

    `mode` pins the sweep ("dense": every pair; "culled": nn_pruned.hip) -- same outputs; `stats`
    (a list) receives the culled sweep's 8 counters (rfops.h).  `lengths1` / `lengths2`: per-sample point
    counts of a ragged batch (rf_nn_distance_lengths): padded slots come back as (0, -1)."""
    if lengths1 is not None or lengths2 is not None:
        return _nn_distance_lengths(xyz1, xyz2, mode, stats, lengths1, lengths2)
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    dev = st.device_()
    a, b_ = st.up(a, b_)
    d1, i1 = H.empty((b, n), F32, dev), H.empty((b, n), I32, dev)
    d2, i2 = H.empty((b, m), F32, dev), H.empty((b, m), I32, dev)
    ws, wsz = H.workspace(lib.rf_nn_distance_mode_workspace_bytes(b, n, m, NN_MODES[mode]), dev, "nn")
    cnt = (C.c_ulonglong * 32)() if stats is not None else None
    check(lib.rf_nn_distance_mode(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(d1), H.ptr(i1), H.ptr(d2),
                                  H.ptr(i2), H.ptr(ws), wsz, H.stream(dev), NN_MODES[mode],
                                  C.cast(cnt, C.c_void_p) if cnt is not None else None), "rf_nn_distance")
    if stats is not None:
        stats[:] = list(cnt)
    return tuple(st.give(t) for t in (d1, i1, d2, i2))


def _nn_distance_lengths(xyz1, xyz2, mode, stats, lengths1, lengths2):
    """rf_nn_distance_lengths: nn_distance over a ragged batch."""
    if stats is not None:
        raise H.invalid("nn_distance: the culled sweep's counters are not collected for ragged batches")
    if mode not in NN_MODES:
        raise H.invalid(f"nn_distance: mode must be one of {sorted(NN_MODES)}")
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    d1, i1 = H.empty((b, n), F32, dev), H.empty((b, n), I32, dev)
    d2, i2 = H.empty((b, m), F32, dev), H.empty((b, m), I32, dev)
    ws, wsz = H.workspace(lib.rf_nn_distance_lengths_workspace_bytes(b, n, m, NN_MODES[mode]), dev, "nn")
    check(lib.rf_nn_distance_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(d1), H.ptr(i1),
                                     H.ptr(d2), H.ptr(i2), H.ptr(ws), wsz, H.stream(dev), NN_MODES[mode]),
          "rf_nn_distance_lengths")
    return tuple(st.give(t) for t in (d1, i1, d2, i2))


@H.on_input_device
def nn_distance_grad(xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2, lengths1=None, lengths2=None):
    """NnDistanceGradGpuOp::Compute, tf_ops/CD/tf_nndistance.cpp:216-251.  With `lengths1` / `lengths2`
    (rf_nn_distance_grad_lengths) rows beyond a sample's count get a zero gradient."""
    st = H.Staged()
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    gd1, gd2 = st.take(grad_dist1, F32), st.take(grad_dist2, F32)
    i1, i2 = st.take(idx1, I32), st.take(idx2, I32)
    if a.dim() != 3:
        raise H.invalid("NnDistanceGrad requires xyz1 be of shape (batch,#points,3)")
    if a.shape[2] != 3:
        raise H.invalid("NnDistanceGrad only accepts 3d point set xyz1")
    if b_.dim() != 3:
        raise H.invalid("NnDistanceGrad requires xyz2 be of shape (batch,#points,3)")
    if b_.shape[2] != 3:
        raise H.invalid("NnDistanceGrad only accepts 3d point set xyz2")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid("NnDistanceGrad expects xyz1 and xyz2 have same batch size")
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    if tuple(gd1.shape) != (b, n):
        raise H.invalid("NnDistanceGrad requires grad_dist1 be of shape(batch,#points)")
    if tuple(i1.shape) != (b, n):
        raise H.invalid("NnDistanceGrad requires idx1 be of shape(batch,#points)")
    if tuple(gd2.shape) != (b, m):
        raise H.invalid("NnDistanceGrad requires grad_dist2 be of shape(batch,#points)")
    if tuple(i2.shape) != (b, m):
        raise H.invalid("NnDistanceGrad requires idx2 be of shape(batch,#points)")
    ragged = lengths1 is not None or lengths2 is not None
    if ragged:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_, gd1, gd2, i1, i2 = st.up(a, b_, gd1, gd2, i1, i2)
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    if ragged:
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        check(lib.rf_nn_distance_grad_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(gd1),
                                              H.ptr(i1), H.ptr(gd2), H.ptr(i2), H.ptr(g1), H.ptr(g2), H.stream(dev)),
              "rf_nn_distance_grad_lengths")
        return st.give(g1), st.give(g2)
    check(lib.rf_nn_distance_grad(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(gd1), H.ptr(i1), H.ptr(gd2),
                                  H.ptr(i2), H.ptr(g1), H.ptr(g2), H.stream(dev)),
          "rf_nn_distance_grad")
    return st.give(g1), st.give(g2)


def _nn_inputs(st, xyz1, xyz2, op="NnDistance"):
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if a.dim() != 3:
        raise H.invalid(f"{op} requires xyz1 be of shape (batch,#points,3)")
    if a.shape[2] != 3:
        raise H.invalid(f"{op} only accepts 3d point set xyz1")
    if b_.dim() != 3:
        raise H.invalid(f"{op} requires xyz2 be of shape (batch,#points,3)")
    if b_.shape[2] != 3:
        raise H.invalid(f"{op} only accepts 3d point set xyz2")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid(f"{op} expects xyz1 and xyz2 have same batch size")
    return a, b_


def _nn_outputs(b, n, m, dev, want1, want2):
    """(dist1, idx1, dist2, idx2) buffers of the wanted directions, None for a skipped one."""
    d1 = H.empty((b, n), F32, dev) if want1 else None
    i1 = H.empty((b, n), I32, dev) if want1 else None
    d2 = H.empty((b, m), F32, dev) if want2 else None
    i2 = H.empty((b, m), I32, dev) if want2 else None
    return d1, i1, d2, i2


@H.on_input_device
def nn_distance_dir(xyz1, xyz2, want1=True, want2=True):
    """nn_distance with only the direction(s) the caller uses (rf_nn_distance_dir): the reference's
    glue drops outputs -- merge_layer keeps idx2 (vv_recon.py:134-135), fidelity_loss dist1 (:386-390),
    zero_groupnear dist2 (:415-419).  -> (dist1, idx1, dist2, idx2) with None for a skipped direction."""
    if not (want1 or want2):
        raise H.invalid("nn_distance_dir needs at least one direction")
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    dev = st.device_()
    a, b_ = st.up(a, b_)
    d1, i1, d2, i2 = _nn_outputs(b, n, m, dev, want1, want2)
    ws, wsz = H.workspace(lib.rf_nn_distance_dir_workspace_bytes(b, n, m, int(want1), int(want2)), dev, "nn")
    check(lib.rf_nn_distance_dir(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(d1), H.ptr(i1), H.ptr(d2), H.ptr(i2),
                                 H.ptr(ws), wsz, H.stream(dev), int(want1), int(want2)), "rf_nn_distance_dir")
    return tuple(None if t is None else st.give(t) for t in (d1, i1, d2, i2))


class SortedCloud:
    """A batch of clouds in the culled sweep's space-filling-curve order (rf_nn_sort): sort once, use
    in any number of nn_distance_sorted / chamfer_loss / merge_layer calls while `xyz` is unchanged.
    The handle is this object's device buffer; the library itself keeps no state."""

    def __init__(self, xyz):
        st = H.Staged()
        t = st.take(xyz, F32)
        if not _shape3(t, 3):
            raise H.invalid("NnDistance requires xyz1 be of shape (batch,#points,3)")
        dev = st.device_()
        self.xyz, = st.up(t)
        self.b, self.n = int(t.shape[0]), int(t.shape[1])
        nbytes = lib.rf_nn_sort_bytes(self.b, self.n)
        if nbytes == 0:
            raise H.invalid("nn_sort handles clouds of 1..65536 points")
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.rf_nn_sort(self.b, self.n, H.ptr(self.xyz), H.ptr(self.buf), int(nbytes), H.stream(dev)),
                  "rf_nn_sort")

    @property
    def device(self):
        return self.buf.device


def nn_sort(xyz):
    return SortedCloud(xyz)


def nn_distance_sorted(s1, s2, want1=True, want2=True):
    """rf_nn_distance_sorted on two SortedCloud handles -> (dist1, idx1, dist2, idx2), None for a
    skipped direction.  Bit-identical to nn_distance(s1.xyz, s2.xyz)."""
    if s1.b != s2.b:
        raise H.invalid("NnDistance expects xyz1 and xyz2 have same batch size")
    if s1.device != s2.device:
        raise ValueError("all GPU inputs of one op must live on the same device")
    if not (want1 or want2):
        raise H.invalid("nn_distance_sorted needs at least one direction")
    dev, b, n, m = s1.device, s1.b, s1.n, s2.n
    with torch.cuda.device(dev):
        d1, i1, d2, i2 = _nn_outputs(b, n, m, dev, want1, want2)
        check(lib.rf_nn_distance_sorted(b, n, m, H.ptr(s1.buf), H.ptr(s2.buf), H.ptr(d1), H.ptr(i1), H.ptr(d2),
                                        H.ptr(i2), H.stream(dev)), "rf_nn_distance_sorted")
    return d1, i1, d2, i2


class ChamferStep:
    """nn_distance + nn_distance_grad of one shape as ONE C-ABI call on buffers allocated once
    (rf_chamfer_step): the host path of a training step is a single ctypes crossing with
    precomputed arguments -- no tensor allocation, no shape checks, no Python per-output work."""

    def __init__(self, b, n, m, device):
        dev = torch.device(device)
        self.dev, self.shape = dev, (b, n, m)
        self.dist1, self.idx1 = H.empty((b, n), F32, dev), H.empty((b, n), I32, dev)
        self.dist2, self.idx2 = H.empty((b, m), F32, dev), H.empty((b, m), I32, dev)
        self.grad1, self.grad2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
        nbytes = int(lib.rf_chamfer_step_workspace_bytes(b, n, m))
        self.ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self._tail = (H.ptr(self.dist1), H.ptr(self.idx1), H.ptr(self.dist2), H.ptr(self.idx2),
                      H.ptr(self.grad1), H.ptr(self.grad2), H.ptr(self.ws), nbytes)
        self._fn = lib.rf_chamfer_step

    def __call__(self, xyz1, xyz2, grad_dist1, grad_dist2):
        """Inputs: contiguous fp32 GPU tensors of the planned shape (not re-validated: this is the
        hot loop).  Returns (dist1, idx1, dist2, idx2, grad_xyz1, grad_xyz2) -- the plan's own buffers,
        overwritten by the next call."""
        b, n, m = self.shape
        st = self._fn(b, n, m, xyz1.data_ptr(), xyz2.data_ptr(), grad_dist1.data_ptr(), grad_dist2.data_ptr(),
                      *self._tail, torch.cuda.current_stream(self.dev).cuda_stream)
        if st:
            check(st, "rf_chamfer_step")
        return self.dist1, self.idx1, self.dist2, self.idx2, self.grad1, self.grad2


def _sorted_ptr(s, b, n, dev):
    if s is None:
        return None
    if (s.b, s.n) != (b, n) or s.device != dev:
        raise ValueError("sorted handle does not match its cloud (batch, points, device)")
    return H.ptr(s.buf)


@H.on_input_device
def chamfer_loss(xyz1, xyz2, sorted1=None, sorted2=None, want1=True, want2=True, lengths1=None, lengths2=None):
    """rf_chamfer_loss: per-sample mean sqrt(dist) both ways, (b, 2), next to the nn_distance outputs
    of the computed directions -> (loss, dist1, idx1, dist2, idx2).  `lengths1` / `lengths2`: per-sample
    counts of a ragged batch (rf_chamfer_loss_lengths: means over each sample's own count); they do not
    combine with sorted handles."""
    if not (want1 or want2):
        raise H.invalid("chamfer_loss needs at least one direction")
    if lengths1 is not None or lengths2 is not None:
        return _chamfer_loss_lengths(xyz1, xyz2, sorted1, sorted2, want1, want2, lengths1, lengths2)
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    dev = st.device_()
    a, b_ = st.up(a, b_)
    loss = H.empty((b, 2), F32, dev)
    d1, i1, d2, i2 = _nn_outputs(b, n, m, dev, want1, want2)
    p1, p2 = _sorted_ptr(sorted1, b, n, dev), _sorted_ptr(sorted2, b, m, dev)
    ws, wsz = H.workspace(lib.rf_chamfer_loss_workspace_bytes(b, n, m, int(want1), int(want2), int(p1 is not None),
                                                              int(p2 is not None)), dev, "nn")
    check(lib.rf_chamfer_loss(b, n, m, H.ptr(a), H.ptr(b_), p1, p2, H.ptr(loss), H.ptr(d1), H.ptr(i1), H.ptr(d2),
                              H.ptr(i2), H.ptr(ws), wsz, H.stream(dev)), "rf_chamfer_loss")
    return tuple(None if t is None else st.give(t) for t in (loss, d1, i1, d2, i2))


def _chamfer_loss_lengths(xyz1, xyz2, sorted1, sorted2, want1, want2, lengths1, lengths2):
    """rf_chamfer_loss_lengths: chamfer_loss over a ragged batch."""
    if sorted1 is not None or sorted2 is not None:
        raise H.invalid("chamfer_loss: per-sample lengths do not combine with sorted handles")
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    loss = H.empty((b, 2), F32, dev)
    d1, i1, d2, i2 = _nn_outputs(b, n, m, dev, want1, want2)
    ws, wsz = H.workspace(lib.rf_chamfer_loss_lengths_workspace_bytes(b, n, m, int(want1), int(want2)), dev, "nn")
    check(lib.rf_chamfer_loss_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(loss), H.ptr(d1),
                                      H.ptr(i1), H.ptr(d2), H.ptr(i2), H.ptr(ws), wsz, H.stream(dev)),
          "rf_chamfer_loss_lengths")
    return tuple(None if t is None else st.give(t) for t in (loss, d1, i1, d2, i2))


@H.on_input_device
def chamfer_loss_grad(xyz1, xyz2, dist1, idx1, dist2, idx2, grad_loss, lengths1=None, lengths2=None):
    """rf_chamfer_loss_grad -> (grad_xyz1, grad_xyz2); dist/idx of a direction that was not computed
    are None.  With `lengths1` / `lengths2` (rf_chamfer_loss_grad_lengths) the means are over each
    sample's own count and rows beyond it get a zero gradient."""
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2, "NnDistanceGrad")
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    gl = st.take(grad_loss, F32)
    if tuple(gl.shape) != (b, 2):
        raise H.invalid("chamfer_loss_grad requires grad_loss be of shape (batch,2)")
    opt = []
    for t, dt, shape in ((dist1, F32, (b, n)), (idx1, I32, (b, n)), (dist2, F32, (b, m)), (idx2, I32, (b, m))):
        if t is None:
            opt.append(None)
            continue
        t = st.take(t, dt)
        if tuple(t.shape) != shape:
            raise H.invalid("NnDistanceGrad requires idx/dist be of shape(batch,#points)")
        opt.append(t)
    ragged = lengths1 is not None or lengths2 is not None
    if ragged:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_, gl = st.up(a, b_, gl)
    opt = [None if t is None else st.up(t)[0] for t in opt]
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    if ragged:
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        check(lib.rf_chamfer_loss_grad_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(opt[0]),
                                               H.ptr(opt[1]), H.ptr(opt[2]), H.ptr(opt[3]), H.ptr(gl), H.ptr(g1),
                                               H.ptr(g2), H.stream(dev)), "rf_chamfer_loss_grad_lengths")
        return st.give(g1), st.give(g2)
    check(lib.rf_chamfer_loss_grad(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(opt[0]), H.ptr(opt[1]), H.ptr(opt[2]),
                                   H.ptr(opt[3]), H.ptr(gl), H.ptr(g1), H.ptr(g2), H.stream(dev)),
          "rf_chamfer_loss_grad")
    return st.give(g1), st.give(g2)


CM_NCOL = 11  # RF_CM_NCOL (include/rfops.h): columns of the metrics tensor


def _metric_args(tau, alpha, op):
    """(thr2, alpha) as the C ABI takes them: `tau` is a distance, the kernels compare squared distances with
    float32(tau) * float32(tau).  tau <= 0 or NaN, alpha negative or not finite: invalid, before any launch."""
    tau, alpha = float(tau), float(alpha)
    if not tau > 0.0:
        raise H.invalid(f"{op}: tau must be a positive distance")
    if not (alpha >= 0.0 and np.isfinite(alpha)):
        raise H.invalid(f"{op}: alpha must be finite and non-negative")
    with np.errstate(over="ignore"):
        return float(np.float32(tau) * np.float32(tau)), alpha


@H.on_input_device
def nn_metrics(dist1, idx1, dist2, idx2, tau, alpha, lengths1=None, lengths2=None):
    """rf_nn_metrics: the metrics epilogue on nn_distance outputs the caller holds (any route) ->
    (metrics (b, 11), count1 (b, n), count2 (b, m)); columns and counts as include/rfops.h defines them."""
    thr2, alpha = _metric_args(tau, alpha, "nn_metrics")
    st = H.Staged()
    d1, d2 = st.take(dist1, F32), st.take(dist2, F32)
    i1, i2 = st.take(idx1, I32), st.take(idx2, I32)
    if d1.dim() != 2 or d2.dim() != 2 or d1.shape[0] != d2.shape[0]:
        raise H.invalid("nn_metrics requires dist1 (batch,#points1) and dist2 (batch,#points2)")
    if i1.shape != d1.shape or i2.shape != d2.shape:
        raise H.invalid("nn_metrics requires idx1 / idx2 be of the shapes of dist1 / dist2")
    b, n, m = d1.shape[0], d1.shape[1], d2.shape[1]
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    d1, i1, d2, i2 = st.up(d1, i1, d2, i2)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    met = H.empty((b, CM_NCOL), F32, dev)
    c1, c2 = H.empty((b, n), I32, dev), H.empty((b, m), I32, dev)
    ws, wsz = H.workspace(lib.rf_nn_metrics_workspace_bytes(b, n, m), dev, "nn_metrics")
    check(lib.rf_nn_metrics(b, n, m, H.ptr(d1), H.ptr(i1), H.ptr(d2), H.ptr(i2), H.ptr(l1), H.ptr(l2), thr2, alpha,
                            H.ptr(met), H.ptr(c1), H.ptr(c2), H.ptr(ws), wsz, H.stream(dev)), "rf_nn_metrics")
    return tuple(st.give(t) for t in (met, c1, c2))


@H.on_input_device
def chamfer_metrics(xyz1, xyz2, tau, alpha, lengths1=None, lengths2=None):
    """rf_chamfer_metrics: the Chamfer sweep (both directions, padded slots (0, -1)) and the metrics epilogue in
    one call -> (metrics (b, 11), dist1, idx1, dist2, idx2, count1, count2)."""
    thr2, alpha = _metric_args(tau, alpha, "chamfer_metrics")
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    met = H.empty((b, CM_NCOL), F32, dev)
    d1, i1, c1 = H.empty((b, n), F32, dev), H.empty((b, n), I32, dev), H.empty((b, n), I32, dev)
    d2, i2, c2 = H.empty((b, m), F32, dev), H.empty((b, m), I32, dev), H.empty((b, m), I32, dev)
    ws, wsz = H.workspace(lib.rf_chamfer_metrics_workspace_bytes(b, n, m), dev, "nn")
    check(lib.rf_chamfer_metrics(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), thr2, alpha, H.ptr(met),
                                 H.ptr(d1), H.ptr(i1), H.ptr(d2), H.ptr(i2), H.ptr(c1), H.ptr(c2), H.ptr(ws), wsz,
                                 H.stream(dev)), "rf_chamfer_metrics")
    return tuple(st.give(t) for t in (met, d1, i1, d2, i2, c1, c2))


CX_NCOL = 6  # RF_CX_NCOL (include/rfops.h): columns of the Chamfer matrix
CX_MAX_CLOUDS, CX_MAX_POINTS = 65535, 65536


@H.on_input_device
def chamfer_cross(xyz1, xyz2=None, lengths1=None, lengths2=None):
    """rf_chamfer_cross: the Chamfer matrix of two collections of clouds, xyz1 (s, n, 3) against xyz2 (r, m, 3) ->
    (s, r, 6) float32: per pair (i, j) the means of sqrt(dist), the means of dist and the maxima of dist in both
    directions (columns 0-5 of chamfer_metrics).  Each collection is sorted once; nothing is stored per point.
    xyz2=None is the collection against itself (sorted once, `lengths2` must then be None too: lengths1 holds for
    both sides).  lengths1 (s,) / lengths2 (r,): per-cloud point counts.  The result carries no gradient."""
    st = H.Staged()
    a = st.take(xyz1, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid("chamfer_cross requires xyz1 be of shape (#clouds1,#points,3)")
    self_ = xyz2 is None
    if self_:
        if lengths2 is not None:
            raise H.invalid("chamfer_cross of a collection against itself takes lengths1 only")
        b_ = a
    else:
        b_ = st.take(xyz2, F32)
        if b_.dim() != 3 or b_.shape[2] != 3:
            raise H.invalid("chamfer_cross requires xyz2 be of shape (#clouds2,#points,3)")
    s, n, r, m = a.shape[0], a.shape[1], b_.shape[0], b_.shape[1]
    if s > 0 and r > 0 and (n < 1 or m < 1):
        raise H.invalid("chamfer_cross requires at least one point per cloud")
    if n > CX_MAX_POINTS or m > CX_MAX_POINTS:
        raise H.invalid(f"chamfer_cross takes clouds of up to {CX_MAX_POINTS} points")
    if s > CX_MAX_CLOUDS or r > CX_MAX_CLOUDS:
        raise H.invalid(f"chamfer_cross takes up to {CX_MAX_CLOUDS} clouds per collection: split the collection")
    l1 = _check_lengths(lengths1, s, n, "lengths1")
    l2 = l1 if self_ else _check_lengths(lengths2, r, m, "lengths2")
    dev = st.device_()
    if self_:
        (a,) = st.up(a)
        b_ = a
        l1 = l2 = _lengths_up(l1, dev, n)
    else:
        a, b_ = st.up(a, b_)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    out = H.empty((s, r, CX_NCOL), F32, dev)
    if s > 0 and r > 0:
        ws, wsz = H.workspace(lib.rf_chamfer_cross_workspace_bytes(s, r, n, m), dev, "chamfer_cross")
        check(lib.rf_chamfer_cross(s, r, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(out), H.ptr(ws), wsz,
                                   H.stream(dev)), "rf_chamfer_cross")
    return st.give(out)


SW_MAX_POINTS, SW_DIR_CHUNK = 16384, 16  # RF_SW_MAX_POINTS, RF_SW_DIR_CHUNK (include/rfops.h)


@H.on_input_device
def sliced_wasserstein(xyz1, xyz2, directions, lengths1=None, lengths2=None, want_grad=False):
    """rf_sliced_wasserstein: the sliced Wasserstein distance SW_2^2 of xyz1 (b, n, 3) and xyz2 (b, m, 3) over the
    rows of `directions` (nproj, 3), used as given -> loss (b,), or with `want_grad` (loss, grad_xyz1, grad_xyz2)
    from the same call.  n != m and per-sample counts lengths1 / lengths2 are exact (the quantile functions are
    merged); ties in a projection go to the lower index; rows behind a count get a gradient of exactly 0."""
    st = H.Staged()
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid("sliced_wasserstein requires xyz1 be of shape (batch,#points,3)")
    if b_.dim() != 3 or b_.shape[2] != 3:
        raise H.invalid("sliced_wasserstein requires xyz2 be of shape (batch,#points,3)")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid("sliced_wasserstein expects xyz1 and xyz2 have same batch size")
    d = st.take(directions, F32)
    if d.dim() != 2 or d.shape[1] != 3 or d.shape[0] < 1:
        raise H.invalid("sliced_wasserstein requires directions be of shape (#projections,3), at least one")
    b, n, m, nproj = a.shape[0], a.shape[1], b_.shape[1], d.shape[0]
    if b > 0 and (n < 1 or m < 1):
        raise H.invalid("sliced_wasserstein requires at least one point per cloud")
    if n > SW_MAX_POINTS or m > SW_MAX_POINTS:
        raise H.invalid(f"sliced_wasserstein takes clouds of up to {SW_MAX_POINTS} points")
    if b > 65535:
        raise H.invalid("sliced_wasserstein takes up to 65535 samples per call: split the batch")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_, d = st.up(a, b_, d)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    loss = H.empty((b,), F32, dev)
    g1 = H.empty((b, n, 3), F32, dev) if want_grad else None
    g2 = H.empty((b, m, 3), F32, dev) if want_grad else None
    if b > 0:
        ws, wsz = H.workspace(lib.rf_sliced_wasserstein_workspace_bytes(b, n, m, nproj, 1 if want_grad else 0), dev,
                              "sliced")
        check(lib.rf_sliced_wasserstein(b, n, m, nproj, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(d),
                                        H.ptr(loss), H.ptr(g1), H.ptr(g2), H.ptr(ws), wsz, H.stream(dev)),
              "rf_sliced_wasserstein")
    if want_grad:
        return st.give(loss), st.give(g1), st.give(g2)
    return st.give(loss)


SK_MAX_POINTS, SK_MAX_ITERS = 65536, 256  # RF_SK_MAX_POINTS, RF_SK_MAX_ITERS (include/rfops.h)
SK_COL_TILE, SK_NSPLIT = 256, 4  # sinkhorn.hip's column tile and the chunks a row's columns are spread over at most


def _sk_schedule(eps):
    """The eps schedule of rf_sinkhorn as a host float32 array, checked: 1 ... SK_MAX_ITERS positive finite values."""
    if isinstance(eps, torch.Tensor):
        if eps.is_cuda:
            raise H.invalid("sinkhorn expects eps on the host: the schedule is read when the call is made")
        eps = eps.detach().numpy()
    e = np.ascontiguousarray(np.asarray(eps, np.float64).reshape(-1)).astype(np.float32)
    if e.size < 1 or e.size > SK_MAX_ITERS:
        raise H.invalid(f"sinkhorn expects an eps schedule of 1 to {SK_MAX_ITERS} steps")
    if not (np.isfinite(e).all() and (e > 0).all()):
        raise H.invalid("sinkhorn expects every eps be positive and finite (in float32)")
    return e


@H.on_input_device
def sinkhorn(xyz1, xyz2, eps, p=1, lengths1=None, lengths2=None, want_grad=False):
    """rf_sinkhorn: the Sinkhorn divergence of xyz1 (b, n, 3) and xyz2 (b, m, 3) for the cost |x - y| (p = 1) or
    |x - y|^2 / 2 (p = 2) along the host schedule `eps` -> (loss (b,), pot (b, n + m) = the final potentials f1 | g1,
    delta (b,) = how far they moved in the last step), with `want_grad` also (grad_xyz1, grad_xyz2) of the same call.
    n != m and per-sample counts lengths1 / lengths2 are exact; slots and rows behind a count are +0."""
    st = H.Staged()
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid("sinkhorn requires xyz1 be of shape (batch,#points,3)")
    if b_.dim() != 3 or b_.shape[2] != 3:
        raise H.invalid("sinkhorn requires xyz2 be of shape (batch,#points,3)")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid("sinkhorn expects xyz1 and xyz2 have same batch size")
    if p not in (1, 2):
        raise H.invalid("sinkhorn expects p be 1 or 2")
    e = _sk_schedule(eps)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    if b > 0 and (n < 1 or m < 1):
        raise H.invalid("sinkhorn requires at least one point per cloud")
    if n > SK_MAX_POINTS or m > SK_MAX_POINTS:
        raise H.invalid(f"sinkhorn takes clouds of up to {SK_MAX_POINTS} points")
    if b > 65535:
        raise H.invalid("sinkhorn takes up to 65535 samples per call: split the batch")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    loss, pot, delta = H.empty((b,), F32, dev), H.empty((b, n + m), F32, dev), H.empty((b,), F32, dev)
    g1 = H.empty((b, n, 3), F32, dev) if want_grad else None
    g2 = H.empty((b, m, 3), F32, dev) if want_grad else None
    if b > 0:
        ws, wsz = H.workspace(lib.rf_sinkhorn_workspace_bytes(b, n, m), dev, "sinkhorn")
        check(lib.rf_sinkhorn(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), int(p), e.ctypes.data, int(e.size),
                              H.ptr(loss), H.ptr(pot), H.ptr(delta), H.ptr(g1), H.ptr(g2), H.ptr(ws), wsz, H.stream(dev)),
              "rf_sinkhorn")
    out = (loss, pot, delta) + ((g1, g2) if want_grad else ())
    return tuple(st.give(t) for t in out)


GR_Q, GR_MAX_RES, GR_MAX_POINTS = 512, 256, 65536  # RF_GR_Q, RF_GR_MAX_RES, RF_GR_MAX_POINTS (include/rfops.h)
GR_MODES = {"counts": 0, "density": 1}  # RF_GR_COUNTS, RF_GR_DENSITY
GR_BRICK = 16  # gridding.hip's brick edge, in vertices


def _gr_box(op, res, lo, hi):
    """The grid arguments of the gridding entries, checked -> (res, lo, hi) as an int and two floats that are fp32 values."""
    res = int(res)
    if res < 2 or res > GR_MAX_RES:
        raise H.invalid(f"{op} expects a resolution of 2 to {GR_MAX_RES} vertices per axis")
    with np.errstate(over="ignore"):
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise H.invalid(f"{op} expects finite bounds lo < hi (in float32)")
    return res, lo, hi


def _gr_cloud(op, st, xyz, name):
    a = st.take(xyz, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid(f"{op} requires {name} be of shape (batch,#points,3)")
    if a.shape[0] > 0 and a.shape[1] < 1:
        raise H.invalid(f"{op} requires at least one point per cloud")
    if a.shape[1] > GR_MAX_POINTS:
        raise H.invalid(f"{op} takes clouds of up to {GR_MAX_POINTS} points")
    if a.shape[0] > 65535:
        raise H.invalid(f"{op} takes up to 65535 samples per call: split the batch")
    return a


@H.on_input_device
def gridding_loss(xyz1, xyz2, res, lo, hi, mode="counts", lengths1=None, lengths2=None, want_grad=False):
    """rf_gridding_loss: the L1 difference of the trilinear grids of xyz1 (b, n, 3) and xyz2 (b, m, 3) on `res` vertices per
    axis over the box [lo, hi]^3 -> (loss (b,), inside (b, 2) int32), with `want_grad` also (grad_xyz1, grad_xyz2) of the same
    call.  mode "counts": the mean over the vertices of |G1 - G2|; "density": sum |G1 / L1 - G2 / L2|.  The sums are integers:
    the bits do not depend on the order of the points.  Points outside the box and rows behind a count contribute nothing and
    get a gradient of exactly 0."""
    st = H.Staged()
    a, b_ = _gr_cloud("gridding_loss", st, xyz1, "xyz1"), _gr_cloud("gridding_loss", st, xyz2, "xyz2")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid("gridding_loss expects xyz1 and xyz2 have same batch size")
    if mode not in GR_MODES:
        raise H.invalid("gridding_loss expects mode be 'counts' or 'density'")
    res, lo, hi = _gr_box("gridding_loss", res, lo, hi)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    loss, inside = H.empty((b,), F32, dev), H.empty((b, 2), I32, dev)
    g1 = H.empty((b, n, 3), F32, dev) if want_grad else None
    g2 = H.empty((b, m, 3), F32, dev) if want_grad else None
    if b > 0:
        ws, wsz = H.workspace(lib.rf_gridding_loss_workspace_bytes(b, n, m, res, 1 if want_grad else 0), dev, "gridding")
        check(lib.rf_gridding_loss(b, n, m, res, lo, hi, GR_MODES[mode], H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2),
                                   H.ptr(loss), H.ptr(inside), H.ptr(g1), H.ptr(g2), H.ptr(ws), wsz, H.stream(dev)),
              "rf_gridding_loss")
    out = (loss, inside) + ((g1, g2) if want_grad else ())
    return tuple(st.give(t) for t in out)


@H.on_input_device
def gridding(xyz, res, lo, hi, lengths=None):
    """rf_gridding: the Gridding layer -> (grid (b, res, res, res) fp32 with x slowest, inside (b,) int32): every point of xyz
    (b, n, 3) inside [lo, hi]^3 spreads a mass of 1 trilinearly over the eight vertices of its cell, in exact integer sums."""
    st = H.Staged()
    a = _gr_cloud("gridding", st, xyz, "xyz")
    res, lo, hi = _gr_box("gridding", res, lo, hi)
    b, n = a.shape[0], a.shape[1]
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    (a,) = st.up(a)
    ln = _lengths_up(ln, dev, n)
    grid, inside = H.empty((b, res, res, res), F32, dev), H.empty((b,), I32, dev)
    if b > 0:
        ws, wsz = H.workspace(lib.rf_gridding_workspace_bytes(b, n, res), dev, "gridding")
        check(lib.rf_gridding(b, n, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(grid), H.ptr(inside), H.ptr(ws), wsz,
                              H.stream(dev)), "rf_gridding")
    return st.give(grid), st.give(inside)


@H.on_input_device
def gridding_grad(xyz, grad_grid, res, lo, hi, lengths=None):
    """rf_gridding_grad: the backward of gridding -> grad_xyz (b, n, 3) from grad_grid (b, res, res, res); exactly 0 for points
    outside the box and rows behind the count."""
    st = H.Staged()
    a = _gr_cloud("gridding_grad", st, xyz, "xyz")
    res, lo, hi = _gr_box("gridding_grad", res, lo, hi)
    b, n = a.shape[0], a.shape[1]
    gg = st.take(grad_grid, F32)
    if tuple(gg.shape) != (b, res, res, res):
        raise H.invalid("gridding_grad requires grad_grid be of shape (batch,res,res,res)")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, gg = st.up(a, gg)
    ln = _lengths_up(ln, dev, n)
    out = H.empty((b, n, 3), F32, dev)
    if b > 0:
        check(lib.rf_gridding_grad(b, n, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(gg), H.ptr(out), H.stream(dev)),
              "rf_gridding_grad")
    return st.give(out)


CFS_MAX_CHANNELS = 1024  # RF_CFS_MAX_CHANNELS (include/rfops.h)
CFS_BRICK, CFS_CHUNK = 8, 8  # grnet_layers.hip: a backward workgroup's sub-brick edge in vertices, and its channels
GREV_TILE = 256  # grnet_layers.hip: cells per tile of Gridding Reverse's ordered compaction


def _cfs_volume(op, st, vol, name, b):
    v = st.take(vol, F32)
    if v.dim() != 5 or v.shape[0] != b or not (v.shape[2] == v.shape[3] == v.shape[4]):
        raise H.invalid(f"{op} requires {name} be of shape (batch,channels,res,res,res)")
    if v.shape[1] < 1 or v.shape[1] > CFS_MAX_CHANNELS:
        raise H.invalid(f"{op} takes 1 to {CFS_MAX_CHANNELS} channels")
    return v


@H.on_input_device
def cubic_feature_sampling(xyz, vol, lo, hi, lengths=None):
    """rf_cubic_feature_sampling: GRNet's Cubic Feature Sampling -> (feat (b, n, 8, c) fp32, inside (b,) int32): for every point
    of xyz (b, n, 3) inside [lo, hi]^3 the feature vectors of vol (b, c, R, R, R) at the eight vertices of its cell (dz fastest),
    copied bit for bit; +0 for points outside the box and rows behind the count."""
    st = H.Staged()
    a = _gr_cloud("cubic_feature_sampling", st, xyz, "xyz")
    b, n = a.shape[0], a.shape[1]
    v = _cfs_volume("cubic_feature_sampling", st, vol, "vol", b)
    c = v.shape[1]
    res, lo, hi = _gr_box("cubic_feature_sampling", v.shape[2], lo, hi)
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, v = st.up(a, v)
    ln = _lengths_up(ln, dev, n)
    feat, inside = H.empty((b, n, 8, c), F32, dev), H.empty((b,), I32, dev)
    if b > 0:
        check(lib.rf_cubic_feature_sampling(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(v), H.ptr(feat), H.ptr(inside),
                                            H.stream(dev)), "rf_cubic_feature_sampling")
    return st.give(feat), st.give(inside)


@H.on_input_device
def cubic_feature_sampling_grad(xyz, grad_feat, res, lo, hi, lengths=None):
    """rf_cubic_feature_sampling_grad: the backward of cubic_feature_sampling -> grad_vol (b, c, res, res, res) from grad_feat
    (b, n, 8, c): fp32 roundings of double sums, every element written once, no float atomics in memory.  The cells are
    recomputed from xyz."""
    st = H.Staged()
    a = _gr_cloud("cubic_feature_sampling_grad", st, xyz, "xyz")
    res, lo, hi = _gr_box("cubic_feature_sampling_grad", res, lo, hi)
    b, n = a.shape[0], a.shape[1]
    gf = st.take(grad_feat, F32)
    if gf.dim() != 4 or tuple(gf.shape[:3]) != (b, n, 8):
        raise H.invalid("cubic_feature_sampling_grad requires grad_feat be of shape (batch,#points,8,channels)")
    c = gf.shape[3]
    if c < 1 or c > CFS_MAX_CHANNELS:
        raise H.invalid(f"cubic_feature_sampling_grad takes 1 to {CFS_MAX_CHANNELS} channels")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, gf = st.up(a, gf)
    ln = _lengths_up(ln, dev, n)
    out = H.empty((b, c, res, res, res), F32, dev)
    if b > 0:
        ws, wsz = H.workspace(lib.rf_cubic_feature_sampling_grad_workspace_bytes(b, n, res), dev, "grnet_layers")
        check(lib.rf_cubic_feature_sampling_grad(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(gf), H.ptr(out), H.ptr(ws),
                                                 wsz, H.stream(dev)), "rf_cubic_feature_sampling_grad")
    return st.give(out)


def _grev_grid(op, st, grid):
    g = st.take(grid, F32)
    if g.dim() != 4 or not (g.shape[1] == g.shape[2] == g.shape[3]):
        raise H.invalid(f"{op} requires grid be of shape (batch,res,res,res)")
    if g.shape[0] > 65535:
        raise H.invalid(f"{op} takes up to 65535 samples per call: split the batch")
    return g


@H.on_input_device
def gridding_reverse(grid, lo, hi, eps=1e-6, compact=False):
    """rf_gridding_reverse: GRNet's Gridding Reverse -> (points (b, M, 3) fp32, row (b, M) int32, count (b,) int32) with
    M = (res - 1)^3: every cell of grid (b, res, res, res) whose eight corner weights sum to S >= eps (and < inf) gives one point,
    the weighted mean of its corners.  row[c] is the row cell c was written to (-1: invalid).  compact: the valid cells fill the
    rows 0 ... count - 1 in cell order and the rest is zeros -- a padded batch with device counts, without a host sync."""
    st = H.Staged()
    g = _grev_grid("gridding_reverse", st, grid)
    res, lo, hi = _gr_box("gridding_reverse", g.shape[1], lo, hi)
    with np.errstate(over="ignore"):
        eps = float(np.float32(eps))
    if not (np.isfinite(eps) and eps > 0):
        raise H.invalid("gridding_reverse expects a finite eps > 0 (in float32)")
    b, M = g.shape[0], (res - 1) ** 3
    dev = st.device_()
    (g,) = st.up(g)
    points, row, count = H.empty((b, M, 3), F32, dev), H.empty((b, M), I32, dev), H.empty((b,), I32, dev)
    if b > 0:
        ws, wsz = H.workspace(lib.rf_gridding_reverse_workspace_bytes(b, res), dev, "grnet_layers")
        check(lib.rf_gridding_reverse(b, res, lo, hi, eps, 1 if compact else 0, H.ptr(g), H.ptr(points), H.ptr(row),
                                      H.ptr(count), H.ptr(ws), wsz, H.stream(dev)), "rf_gridding_reverse")
    return st.give(points), st.give(row), st.give(count)


@H.on_input_device
def gridding_reverse_grad(grid, row, grad_points, lo, hi):
    """rf_gridding_reverse_grad: the backward of gridding_reverse -> grad_grid (b, res, res, res) from the forward's grid and row
    and grad_points (b, M, 3): a gather per vertex in double.  A row entry outside [0, M) counts as -1."""
    st = H.Staged()
    g = _grev_grid("gridding_reverse_grad", st, grid)
    res, lo, hi = _gr_box("gridding_reverse_grad", g.shape[1], lo, hi)
    b, M = g.shape[0], (res - 1) ** 3
    r, gp = st.take(row, I32), st.take(grad_points, F32)
    if tuple(r.shape) != (b, M):
        raise H.invalid("gridding_reverse_grad requires row be of shape (batch,(res-1)^3)")
    if tuple(gp.shape) != (b, M, 3):
        raise H.invalid("gridding_reverse_grad requires grad_points be of shape (batch,(res-1)^3,3)")
    dev = st.device_()
    g, r, gp = st.up(g, r, gp)
    out = H.empty((b, res, res, res), F32, dev)
    if b > 0:
        check(lib.rf_gridding_reverse_grad(b, res, lo, hi, H.ptr(g), H.ptr(r), H.ptr(gp), H.ptr(out), H.stream(dev)),
              "rf_gridding_reverse_grad")
    return st.give(out)


PV_BRICK, PV_CHUNK = 8, 8  # point_voxel.hip: a scatter workgroup's sub-brick edge in vertices, and its channels


def _pv_features(op, st, t, name, b, n):
    f = st.take(t, F32)
    if f.dim() != 3 or tuple(f.shape[:2]) != (b, n):
        raise H.invalid(f"{op} requires {name} be of shape (batch,#points,channels)")
    if f.shape[2] < 1 or f.shape[2] > CFS_MAX_CHANNELS:
        raise H.invalid(f"{op} takes 1 to {CFS_MAX_CHANNELS} channels")
    return f


@H.on_input_device
def avg_voxelize(xyz, feat, res, lo, hi, lengths=None):
    """rf_voxelize_mean: average voxelization -> (vol (b, c, res, res, res) fp32, cnt (b, res, res, res) int32, inside (b,)
    int32): the feature vectors feat (b, n, c) of the points of xyz (b, n, 3) inside [lo, hi]^3, averaged per nearest vertex of
    the grid (a tie goes up); fp32 roundings of double sums divided by the count, +0 where no point fell, no float atomics."""
    st = H.Staged()
    a = _gr_cloud("avg_voxelize", st, xyz, "xyz")
    res, lo, hi = _gr_box("avg_voxelize", res, lo, hi)
    b, n = a.shape[0], a.shape[1]
    f = _pv_features("avg_voxelize", st, feat, "feat", b, n)
    c = f.shape[2]
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, f = st.up(a, f)
    ln = _lengths_up(ln, dev, n)
    vol, cnt = H.empty((b, c, res, res, res), F32, dev), H.empty((b, res, res, res), I32, dev)
    inside = H.empty((b,), I32, dev)
    if b > 0:
        ws, wsz = H.workspace(lib.rf_voxelize_mean_workspace_bytes(b, n, res), dev, "point_voxel")
        check(lib.rf_voxelize_mean(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(f), H.ptr(vol), H.ptr(cnt), H.ptr(inside),
                                   H.ptr(ws), wsz, H.stream(dev)), "rf_voxelize_mean")
    return st.give(vol), st.give(cnt), st.give(inside)


@H.on_input_device
def avg_voxelize_grad(xyz, cnt, grad_vol, lo, hi, lengths=None):
    """rf_voxelize_mean_grad: the backward of avg_voxelize -> grad_feat (b, n, c) from the forward's cnt (b, res, res, res)
    and grad_vol (b, c, res, res, res): grad_vol at the point's nearest vertex over that vertex's count, +0 for points outside the
    box and rows behind the count.  The vertices are recomputed from xyz."""
    st = H.Staged()
    a = _gr_cloud("avg_voxelize_grad", st, xyz, "xyz")
    b, n = a.shape[0], a.shape[1]
    gv = _cfs_volume("avg_voxelize_grad", st, grad_vol, "grad_vol", b)
    c = gv.shape[1]
    res, lo, hi = _gr_box("avg_voxelize_grad", gv.shape[2], lo, hi)
    k = st.take(cnt, I32)
    if tuple(k.shape) != (b, res, res, res):
        raise H.invalid("avg_voxelize_grad requires cnt be of shape (batch,res,res,res)")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, k, gv = st.up(a, k, gv)
    ln = _lengths_up(ln, dev, n)
    out = H.empty((b, n, c), F32, dev)
    if b > 0:
        check(lib.rf_voxelize_mean_grad(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(k), H.ptr(gv), H.ptr(out),
                                        H.stream(dev)), "rf_voxelize_mean_grad")
    return st.give(out)


@H.on_input_device
def trilinear_devoxelize(xyz, vol, lo, hi, lengths=None):
    """rf_trilinear_devoxelize: trilinear devoxelization -> (feat (b, n, c) fp32, inside (b,) int32): vol (b, c, R, R, R)
    interpolated at every point of xyz (b, n, 3) inside [lo, hi]^3 from the eight vertices of its cell, in double with every
    rounding prescribed; +0 for points outside the box and rows behind the count."""
    st = H.Staged()
    a = _gr_cloud("trilinear_devoxelize", st, xyz, "xyz")
    b, n = a.shape[0], a.shape[1]
    v = _cfs_volume("trilinear_devoxelize", st, vol, "vol", b)
    c = v.shape[1]
    res, lo, hi = _gr_box("trilinear_devoxelize", v.shape[2], lo, hi)
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, v = st.up(a, v)
    ln = _lengths_up(ln, dev, n)
    feat, inside = H.empty((b, n, c), F32, dev), H.empty((b,), I32, dev)
    if b > 0:
        check(lib.rf_trilinear_devoxelize(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(v), H.ptr(feat), H.ptr(inside),
                                          H.stream(dev)), "rf_trilinear_devoxelize")
    return st.give(feat), st.give(inside)


@H.on_input_device
def trilinear_devoxelize_grad(xyz, vol, grad_feat, lo, hi, lengths=None, want_xyz=True):
    """rf_trilinear_devoxelize_grad: the backward of trilinear_devoxelize -> (grad_vol (b, c, R, R, R), grad_xyz (b, n, 3) or
    None without `want_xyz`) from grad_feat (b, n, c): grad_vol as fp32 roundings of double sums, every element written once, no
    float atomics in memory; grad_xyz a gather in double.  The cells and weights are recomputed from xyz."""
    st = H.Staged()
    a = _gr_cloud("trilinear_devoxelize_grad", st, xyz, "xyz")
    b, n = a.shape[0], a.shape[1]
    v = _cfs_volume("trilinear_devoxelize_grad", st, vol, "vol", b)
    c = v.shape[1]
    res, lo, hi = _gr_box("trilinear_devoxelize_grad", v.shape[2], lo, hi)
    gf = st.take(grad_feat, F32)
    if tuple(gf.shape) != (b, n, c):
        raise H.invalid("trilinear_devoxelize_grad requires grad_feat be of shape (batch,#points,channels)")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, v, gf = st.up(a, v, gf)
    ln = _lengths_up(ln, dev, n)
    gv = H.empty((b, c, res, res, res), F32, dev)
    gx = H.empty((b, n, 3), F32, dev) if want_xyz else None
    if b > 0:
        ws, wsz = H.workspace(lib.rf_trilinear_devoxelize_grad_workspace_bytes(b, n, res), dev, "point_voxel")
        check(lib.rf_trilinear_devoxelize_grad(b, n, c, res, lo, hi, H.ptr(a), H.ptr(ln), H.ptr(v), H.ptr(gf), H.ptr(gv),
                                               H.ptr(gx), H.ptr(ws), wsz, H.stream(dev)), "rf_trilinear_devoxelize_grad")
    return st.give(gv), (st.give(gx) if want_xyz else None)


# ---- the vector attention pair (include/rfops.h): neighbour subtraction and neighbour aggregation
VA_MAX_K, VA_MAX_CHANNELS = 64, 1024  # RF_VA_MAX_K, RF_VA_MAX_CHANNELS


def _va_index(op, st, idx):
    ix = st.take(idx, I32)
    if ix.dim() != 3:
        raise H.invalid(f"{op} requires idx be of shape (batch,#queries,k)")
    b, m, k = (int(v) for v in ix.shape)
    if not 1 <= k <= VA_MAX_K:
        raise H.invalid(f"{op} takes 1 to {VA_MAX_K} neighbours")
    if not 1 <= m <= 65536:
        raise H.invalid(f"{op} takes 1 to 65536 queries")
    if b > 65535:
        raise H.invalid(f"{op} takes at most 65535 samples")
    return ix, b, m, k


def _va_rows(op, st, t, name, b, rows=None, c=None, what="#points"):
    """a (batch, rows, channels) tensor; rows / c: what they must be where another argument has fixed them"""
    f = st.take(t, F32)
    if f.dim() != 3 or f.shape[0] != b or (rows is not None and f.shape[1] != rows) or (c is not None and f.shape[2] != c):
        raise H.invalid(f"{op} requires {name} be of shape (batch,{what},channels)")
    if not 1 <= f.shape[1] <= 65536:
        raise H.invalid(f"{op} takes 1 to 65536 points")
    if not 1 <= f.shape[2] <= VA_MAX_CHANNELS:
        raise H.invalid(f"{op} takes 1 to {VA_MAX_CHANNELS} channels")
    return f


def _va_slots(op, st, t, name, b, m, k, c=None):
    f = st.take(t, F32)
    if f.dim() != 4 or tuple(f.shape[:3]) != (b, m, k) or (c is not None and f.shape[3] != c):
        raise H.invalid(f"{op} requires {name} be of shape (batch,#queries,k,channels)")
    return f


def _va_sizes(op, n, m, k, c):
    if m * k * c >= 1 << 31 or n * c >= 1 << 31:
        raise H.invalid(f"{op} takes #queries * k * channels and #points * channels below 2^31")


def _va_weight(op, st, weight, b, m, k, c):
    w = _va_slots(op, st, weight, "weight", b, m, k)
    cw = int(w.shape[3])
    if cw < 1 or c % cw:
        raise H.invalid(f"{op} requires the channels of weight to divide those of value")
    return w, cw


@H.on_input_device
def neighbor_subtraction(feat_q, feat_src, idx, lengths1=None, lengths2=None):
    """rf_neighbor_sub (pointops' subtraction on padded batches) -> (b, m, k, c) fp32: feat_q (b, m, c) less the rows of feat_src
    (b, n, c) that idx (b, m, k) int32 names; +0 in dead slots -- queries behind lengths2, slots t >= lengths1 of a query, and
    slots naming a row outside [0, lengths1): the idx of a ragged knn_point and its two counts pass through unchanged."""
    op = "neighbor_subtraction"
    st = H.Staged()
    ix, b, m, k = _va_index(op, st, idx)
    q = _va_rows(op, st, feat_q, "feat_q", b, rows=m, what="#queries")
    c = int(q.shape[2])
    s = _va_rows(op, st, feat_src, "feat_src", b, c=c)
    n = int(s.shape[1])
    _va_sizes(op, n, m, k, c)
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    q, s, ix = st.up(q, s, ix)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    out = H.empty((b, m, k, c), F32, dev)
    if b > 0:
        check(lib.rf_neighbor_sub(b, n, m, k, c, H.ptr(q), H.ptr(s), H.ptr(ix), H.ptr(l1), H.ptr(l2), H.ptr(out), H.stream(dev)),
              "rf_neighbor_sub")
    return st.give(out)


@H.on_input_device
def neighbor_subtraction_grad(idx, grad_out, n, lengths1=None, lengths2=None, want_q=True, want_src=True):
    """rf_neighbor_sub_grad -> (grad_q (b, m, c) or None, grad_src (b, n, c) or None) from grad_out (b, m, k, c): grad_q the double
    sum over a query's live slots in ascending order, grad_src minus the double sum over the live slots naming a row -- a sort of
    the slots by row and a gather that stores every row once, no float atomics.  What is not wanted is not computed."""
    op = "neighbor_subtraction_grad"
    st = H.Staged()
    ix, b, m, k = _va_index(op, st, idx)
    g = _va_slots(op, st, grad_out, "grad_out", b, m, k)
    c, n = int(g.shape[3]), int(n)
    if not 1 <= c <= VA_MAX_CHANNELS:
        raise H.invalid(f"{op} takes 1 to {VA_MAX_CHANNELS} channels")
    if not 1 <= n <= 65536:
        raise H.invalid(f"{op} takes 1 to 65536 points")
    _va_sizes(op, n, m, k, c)
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    ix, g = st.up(ix, g)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    gq = H.empty((b, m, c), F32, dev) if want_q else None
    gs = H.empty((b, n, c), F32, dev) if want_src else None
    if b > 0 and (want_q or want_src):
        ws, wsz = H.workspace(lib.rf_neighbor_sub_grad_workspace_bytes(b, n, m, k), dev, "vector_attention") if want_src else (None, 0)
        check(lib.rf_neighbor_sub_grad(b, n, m, k, c, H.ptr(ix), H.ptr(l1), H.ptr(l2), H.ptr(g), H.ptr(gq), H.ptr(gs), H.ptr(ws), wsz,
                                       H.stream(dev)), "rf_neighbor_sub_grad")
    return (st.give(gq) if want_q else None), (st.give(gs) if want_src else None)


def _va_agg_inputs(op, st, value, weight, idx, pos):
    ix, b, m, k = _va_index(op, st, idx)
    v = _va_rows(op, st, value, "value", b)
    n, c = int(v.shape[1]), int(v.shape[2])
    w, cw = _va_weight(op, st, weight, b, m, k, c)
    p = None if pos is None else _va_slots(op, st, pos, "pos", b, m, k, c)
    _va_sizes(op, n, m, k, c)
    return ix, v, w, p, (b, n, m, k, c, cw)


@H.on_input_device
def neighbor_aggregation(value, weight, idx, pos=None, lengths1=None, lengths2=None):
    """rf_neighbor_aggregate (pointops' aggregation on padded batches) -> (b, m, c) fp32: the sum over a query's live slots, in
    ascending order and in double, of (value[idx] + pos) * weight[..., ch mod cw]; value (b, n, c), weight (b, m, k, cw) with cw
    dividing c (share_planes = c / cw), pos (b, m, k, c) or None.  Dead slots (neighbor_subtraction's rule) add nothing, whatever
    they hold; padded queries are +0."""
    op = "neighbor_aggregation"
    st = H.Staged()
    ix, v, w, p, (b, n, m, k, c, cw) = _va_agg_inputs(op, st, value, weight, idx, pos)
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    ix, v, w = st.up(ix, v, w)
    p = None if p is None else st.up(p)[0]
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    out = H.empty((b, m, c), F32, dev)
    if b > 0:
        check(lib.rf_neighbor_aggregate(b, n, m, k, c, cw, H.ptr(v), H.ptr(p), H.ptr(w), H.ptr(ix), H.ptr(l1), H.ptr(l2), H.ptr(out),
                                        H.stream(dev)), "rf_neighbor_aggregate")
    return st.give(out)


@H.on_input_device
def neighbor_aggregation_grad(value, weight, idx, grad_out, pos=None, lengths1=None, lengths2=None, want_value=True, want_pos=True,
                              want_weight=True):
    """rf_neighbor_aggregate_grad -> (grad_value (b, n, c), grad_pos (b, m, k, c), grad_weight (b, m, k, cw)), None for each that
    is not wanted (it is then not computed), from grad_out (b, m, c): grad_pos one fp32 product per element, grad_weight a double
    sum over the channel groups in ascending order, grad_value a sort of the slots by row and a gather that forms its terms from
    grad_out and weight on the fly and stores every row once -- no float atomics."""
    op = "neighbor_aggregation_grad"
    st = H.Staged()
    ix, v, w, p, (b, n, m, k, c, cw) = _va_agg_inputs(op, st, value, weight, idx, pos)
    g = _va_rows(op, st, grad_out, "grad_out", b, rows=m, c=c, what="#queries")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    ix, v, w, g = st.up(ix, v, w, g)
    p = None if p is None else st.up(p)[0]
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    gv = H.empty((b, n, c), F32, dev) if want_value else None
    gp = H.empty((b, m, k, c), F32, dev) if want_pos else None
    gw = H.empty((b, m, k, cw), F32, dev) if want_weight else None
    if b > 0 and (want_value or want_pos or want_weight):
        ws, wsz = (H.workspace(lib.rf_neighbor_aggregate_grad_workspace_bytes(b, n, m, k), dev, "vector_attention")
                   if want_value else (None, 0))
        check(lib.rf_neighbor_aggregate_grad(b, n, m, k, c, cw, H.ptr(v), H.ptr(p), H.ptr(w), H.ptr(ix), H.ptr(l1), H.ptr(l2),
                                             H.ptr(g), H.ptr(gv), H.ptr(gp), H.ptr(gw), H.ptr(ws), wsz, H.stream(dev)),
              "rf_neighbor_aggregate_grad")
    return tuple(st.give(t) if t is not None else None for t in (gv, gp, gw))


EA_MAX_POINTS = 4096  # RF_EA_MAX_POINTS (include/rfops.h)
EA_OK, EA_CAPPED, EA_NONFINITE = 0, 1, 2  # RF_EA_* status values
EA_TPB, EA_WAVE = 1024, 64  # emd_assign.hip's tiles: threads of the one workgroup per sample; lanes a bidder's scan strides by


def _ea_inputs(st, xyz1, xyz2, lengths, what):
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid(f"{what} requires xyz1 be of shape (batch,#points,3)")
    if b_.dim() != 3 or b_.shape[2] != 3:
        raise H.invalid(f"{what} requires xyz2 be of shape (batch,#points,3)")
    if b_.shape[0] != a.shape[0]:
        raise H.invalid(f"{what} expects xyz1 and xyz2 have same batch size")
    if b_.shape[1] != a.shape[1]:
        raise H.invalid(f"{what} expects xyz1 and xyz2 have same number of points")
    b, n = a.shape[0], a.shape[1]
    if b > 0 and n < 1:
        raise H.invalid(f"{what} requires at least one point per cloud")
    if n > EA_MAX_POINTS:
        raise H.invalid(f"{what} takes clouds of up to {EA_MAX_POINTS} points")
    if b > 65535:
        raise H.invalid(f"{what} takes up to 65535 samples per call: split the batch")
    return a, b_, _check_lengths(lengths, b, n, "lengths")


@H.on_input_device
def emd_assign(xyz1, xyz2, lengths=None, max_rounds=0):
    """rf_emd_assign: the optimal one-to-one assignment of xyz1 (b, n, 3) (persons) to xyz2 (b, n, 3) (objects) by the
    deterministic integer auction of include/rfops.h -> (match12 (b, n) int32, match21 (b, n) int32, dist (b, n),
    val (b, 3) = cost / gap / bound, cert (b, 2) int64 = P / D, info (b, 4) int32 = status / rounds / bids / k).
    `lengths` (b,): per-sample point counts shared by both clouds (slots behind a count are zeros); max_rounds = 0:
    64 L + 1024 rounds.  n <= 4096."""
    st = H.Staged()
    a, b_, ln = _ea_inputs(st, xyz1, xyz2, lengths, "emd_assign")
    max_rounds = int(max_rounds)
    if max_rounds < 0:
        raise H.invalid("emd_assign expects max_rounds >= 0 (0: 64 * #points + 1024)")
    b, n = a.shape[0], a.shape[1]
    dev = st.device_()
    a, b_ = st.up(a, b_)
    ln = _lengths_up(ln, dev, n)
    m12, m21, dist = H.empty((b, n), I32, dev), H.empty((b, n), I32, dev), H.empty((b, n), F32, dev)
    val, cert, info = H.empty((b, 3), F32, dev), H.empty((b, 2), torch.int64, dev), H.empty((b, 4), I32, dev)
    if b > 0:
        ws, wsz = H.workspace(lib.rf_emd_assign_workspace_bytes(b, n), dev, "emd_assign")
        check(lib.rf_emd_assign(b, n, H.ptr(a), H.ptr(b_), H.ptr(ln), max_rounds, H.ptr(m12), H.ptr(m21), H.ptr(dist),
                                H.ptr(val), H.ptr(cert), H.ptr(info), H.ptr(ws), wsz, H.stream(dev)), "rf_emd_assign")
    return tuple(st.give(t) for t in (m12, m21, dist, val, cert, info))


@H.on_input_device
def emd_assign_grad(xyz1, xyz2, match12, match21, grad_cost, lengths=None):
    """rf_emd_assign_grad -> (grad_xyz1, grad_xyz2), both (b, n, 3): the gradients of emd_assign's cost under the
    fixed assignment, scaled by grad_cost (b,); exactly 0 where a pair's distance is 0 and behind a count."""
    st = H.Staged()
    a, b_, ln = _ea_inputs(st, xyz1, xyz2, lengths, "emd_assign_grad")
    b, n = a.shape[0], a.shape[1]
    m12, m21, gc = st.take(match12, I32), st.take(match21, I32), st.take(grad_cost, F32)
    if tuple(m12.shape) != (b, n) or tuple(m21.shape) != (b, n):
        raise H.invalid("emd_assign_grad requires match12 and match21 be of shape (batch,#points)")
    if tuple(gc.shape) != (b,):
        raise H.invalid("emd_assign_grad requires grad_cost be of shape (batch,)")
    dev = st.device_()
    a, b_, m12, m21, gc = st.up(a, b_, m12, m21, gc)
    ln = _lengths_up(ln, dev, n)
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, n, 3), F32, dev)
    if b > 0:
        check(lib.rf_emd_assign_grad(b, n, H.ptr(a), H.ptr(b_), H.ptr(m12), H.ptr(m21), H.ptr(ln), H.ptr(gc), H.ptr(g1),
                                     H.ptr(g2), H.stream(dev)), "rf_emd_assign_grad")
    return st.give(g1), st.give(g2)


XP_MAX_PATCH = 4096  # RF_XP_MAX_PATCH (include/rfops.h)
XP_OK, XP_NONFINITE = 0, 1  # RF_XP_* status values
MDS_MAX_POINTS = 16384  # RF_MDS_MAX_POINTS
MDS_OK, MDS_BADSIGMA = 0, 1  # RF_MDS_* status values


def _xp_inputs(st, xyz, primitive_size, what):
    a = st.take(xyz, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid(f"{what} requires xyz be of shape (batch,#points,3)")
    S = int(primitive_size)
    if S < 2 or S > XP_MAX_PATCH:
        raise H.invalid(f"{what} takes a primitive size in [2, {XP_MAX_PATCH}]")
    b, n = a.shape[0], a.shape[1]
    if n < S or n % S != 0:
        raise H.invalid(f"{what} expects #points to be a positive multiple of the primitive size")
    if b * (n // S) > 2 ** 31 - 1:
        raise H.invalid(f"{what} takes up to 2^31 - 1 patches per call: split the batch")
    return a, S


@H.on_input_device
def expansion_penalty(xyz, primitive_size, alpha=1.5):
    """rf_expansion_penalty: xyz (b, n, 3) as n / primitive_size patches of consecutive rows; per patch the minimum
    spanning tree (Prim from the patch's first row, ties to the smallest index), its edges longer than alpha times the
    patch's mean edge penalised -> (dist (b, n), father (b, n) int32 cloud-level rows, length (b, n), mean (b, P),
    info (b, P) int32 status: 0 ok, 1 a non-finite coordinate in the patch)."""
    st = H.Staged()
    a, S = _xp_inputs(st, xyz, primitive_size, "expansion_penalty")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 3.4028234663852886e38:  # (a finite fp32)
        raise H.invalid("expansion_penalty expects a finite alpha >= 0")
    b, n = a.shape[0], a.shape[1]
    dev = st.device_()
    (a,) = st.up(a)
    dist, father, length = H.empty((b, n), F32, dev), H.empty((b, n), I32, dev), H.empty((b, n), F32, dev)
    mean, info = H.empty((b, n // S), F32, dev), H.empty((b, n // S), I32, dev)
    if b > 0:
        check(lib.rf_expansion_penalty(b, n, S, alpha, H.ptr(a), H.ptr(dist), H.ptr(father), H.ptr(length), H.ptr(mean),
                                       H.ptr(info), H.stream(dev)), "rf_expansion_penalty")
    return tuple(st.give(t) for t in (dist, father, length, mean, info))


@H.on_input_device
def expansion_penalty_grad(xyz, primitive_size, father, dist, grad_dist):
    """rf_expansion_penalty_grad -> grad_xyz (b, n, 3): the gradient of sum(grad_dist * dist) under the fixed tree, mean
    and indicator; summed in double in index order, exactly 0 where nothing contributes."""
    st = H.Staged()
    a, S = _xp_inputs(st, xyz, primitive_size, "expansion_penalty_grad")
    b, n = a.shape[0], a.shape[1]
    fa, d, g = st.take(father, I32), st.take(dist, F32), st.take(grad_dist, F32)
    if tuple(fa.shape) != (b, n) or tuple(d.shape) != (b, n):
        raise H.invalid("expansion_penalty_grad requires father and dist be of shape (batch,#points)")
    if tuple(g.shape) != (b, n):
        raise H.invalid("expansion_penalty_grad requires grad_dist be of shape (batch,#points)")
    dev = st.device_()
    a, fa, d, g = st.up(a, fa, d, g)
    out = H.empty((b, n, 3), F32, dev)
    if b > 0:
        check(lib.rf_expansion_penalty_grad(b, n, S, H.ptr(a), H.ptr(fa), H.ptr(d), H.ptr(g), H.ptr(out), H.stream(dev)),
              "rf_expansion_penalty_grad")
    return st.give(out)


@H.on_input_device
def minimum_density_sample(xyz, npoint, sigma, lengths=None, return_xyz=False):
    """rf_mds: thin xyz (b, n, 3), n <= 16384, to npoint rows; every step takes the valid row whose Gaussian density
    (scale sigma) under the rows chosen so far is smallest, ties to the smallest index; the first is row 0
    -> (idx (b, npoint) int32, info (b,) int32 status: 0 ok, 1 a sigma that is not positive or whose scale leaves fp32)
    and, with return_xyz, the chosen rows (b, npoint, 3).  sigma: a float, or (b,) values -- a CUDA tensor is used where
    it is.  `lengths` (b,): per-sample point counts; slots behind min(npoint, count) are zeros."""
    st = H.Staged()
    a = st.take(xyz, F32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise H.invalid("minimum_density_sample requires xyz be of shape (batch,#points,3)")
    b, n = a.shape[0], a.shape[1]
    m = int(npoint)
    if b > 0 and n < 1:
        raise H.invalid("minimum_density_sample requires at least one point per cloud")
    if n > MDS_MAX_POINTS:
        raise H.invalid(f"minimum_density_sample takes clouds of up to {MDS_MAX_POINTS} points")
    if m < 1:
        raise H.invalid("minimum_density_sample expects npoint >= 1")
    if isinstance(sigma, (int, float)):
        sg = None  # filled on the device below: no host-to-device copy, so the call stays capturable
    else:
        sg = sigma.detach() if isinstance(sigma, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(sigma)))
        if sg.dim() == 0:
            sg = sg.reshape(1).expand(b)
        if sg.dim() != 1 or sg.shape[0] != b:
            raise H.invalid("minimum_density_sample requires sigma be a number or of shape (batch,)")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    (a,) = st.up(a)
    if sg is None:
        sg = torch.full((b,), float(sigma), dtype=F32, device=dev)
    elif sg.is_cuda and sg.device != dev:
        raise ValueError(f"all GPU inputs of one op must live on the same device: got {dev} and {sg.device}")
    sg = sg.to(device=dev, dtype=F32).contiguous()
    ln = _lengths_up(ln, dev, n)
    out, info = H.empty((b, m), I32, dev), H.empty((b,), I32, dev)
    new_xyz = H.empty((b, m, 3), F32, dev) if return_xyz else None
    if b > 0:
        check(lib.rf_mds(b, n, m, H.ptr(a), H.ptr(sg), H.ptr(ln), H.ptr(out), H.ptr(info), H.ptr(new_xyz), H.stream(dev)),
              "rf_mds")
    res = (st.give(out), st.give(info))
    return res + (st.give(new_xyz),) if return_xyz else res


@H.on_input_device
def chamfer_metrics_grad(xyz1, xyz2, dist1, idx1, dist2, idx2, count1, count2, alpha, grad_metrics, lengths1=None,
                         lengths2=None):
    """rf_chamfer_metrics_grad -> (grad_xyz1, grad_xyz2): the backward of columns 0-3, 9 and 10 of the metrics
    (columns 4-8 of grad_metrics are not read; the counts are constants)."""
    _, alpha = _metric_args(1.0, alpha, "chamfer_metrics_grad")
    st = H.Staged()
    a, b_ = _nn_inputs(st, xyz1, xyz2, "NnDistanceGrad")
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    gm = st.take(grad_metrics, F32)
    if tuple(gm.shape) != (b, CM_NCOL):
        raise H.invalid(f"chamfer_metrics_grad requires grad_metrics be of shape (batch,{CM_NCOL})")
    per = []
    for t, dt, shape in ((dist1, F32, (b, n)), (idx1, I32, (b, n)), (dist2, F32, (b, m)), (idx2, I32, (b, m)),
                         (count1, I32, (b, n)), (count2, I32, (b, m))):
        t = st.take(t, dt)
        if tuple(t.shape) != shape:
            raise H.invalid("NnDistanceGrad requires idx/dist/count be of shape(batch,#points)")
        per.append(t)
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_, gm = st.up(a, b_, gm)
    d1, i1, d2, i2, c1, c2 = st.up(*per)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    ws, wsz = H.workspace(lib.rf_chamfer_metrics_grad_workspace_bytes(b, n, m), dev, "nn_metrics_grad")
    check(lib.rf_chamfer_metrics_grad(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(d1), H.ptr(i1),
                                      H.ptr(d2), H.ptr(i2), H.ptr(c1), H.ptr(c2), alpha, H.ptr(gm), H.ptr(g1),
                                      H.ptr(g2), H.ptr(ws), wsz, H.stream(dev)), "rf_chamfer_metrics_grad")
    return st.give(g1), st.give(g2)


@H.on_input_device
def merge_layer(rawpts, newpts, decfactor, sorted_raw=None, lengths=None, lengths_new=None):
    """rf_merge_layer (vv_recon.py:132-139) -> (refined (b,m,3), idx2 (b,m)).  `lengths` / `lengths_new`: per-sample
    counts of rawpts / newpts in a ragged batch (rf_merge_layer_lengths): idx2 points into the sample's own raw rows,
    padded new rows come back as idx2 = 0, refined = 0; they do not combine with a sorted handle."""
    ragged = lengths is not None or lengths_new is not None
    if ragged and sorted_raw is not None:
        raise H.invalid("merge_layer: per-sample lengths do not combine with a sorted handle")
    st = H.Staged()
    a, b_ = _nn_inputs(st, rawpts, newpts)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    if ragged:
        lr, ln = _check_lengths(lengths, b, n, "lengths"), _check_lengths(lengths_new, b, m, "lengths_new")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    dec = torch.as_tensor(decfactor, dtype=F32).detach().reshape(-1)[:1].to(dev).contiguous()
    out, i2 = H.empty((b, m, 3), F32, dev), H.empty((b, m), I32, dev)
    if ragged:
        lr, ln = _lengths_up(lr, dev, n), _lengths_up(ln, dev, m)
        ws, wsz = H.workspace(lib.rf_merge_layer_lengths_workspace_bytes(b, n, m), dev, "nn")
        check(lib.rf_merge_layer_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(lr), H.ptr(ln), H.ptr(dec), H.ptr(out),
                                         H.ptr(i2), H.ptr(ws), wsz, H.stream(dev)), "rf_merge_layer_lengths")
        return st.give(out), st.give(i2)
    ps = _sorted_ptr(sorted_raw, b, n, dev)
    ws, wsz = H.workspace(lib.rf_merge_layer_workspace_bytes(b, n, m, int(ps is not None)), dev, "nn")
    check(lib.rf_merge_layer(b, n, m, H.ptr(a), H.ptr(b_), ps, H.ptr(dec), H.ptr(out), H.ptr(i2), H.ptr(ws), wsz,
                             H.stream(dev)), "rf_merge_layer")
    return st.give(out), st.give(i2)


@H.on_input_device
def merge_layer_grad(rawpts, newpts, decfactor, idx2, grad_refined, want_raw=False, lengths=None, lengths_new=None):
    """rf_merge_layer_grad -> (grad_newpts (b,m,3), grad_dec (b,), grad_raw (b,n,3) or None).  With `lengths` /
    `lengths_new` (rf_merge_layer_grad_lengths) padded rows of either side get a zero gradient and grad_dec sums over
    each sample's own new points."""
    st = H.Staged()
    a, b_ = _nn_inputs(st, rawpts, newpts)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    ix, go = st.take(idx2, I32), st.take(grad_refined, F32)
    if tuple(ix.shape) != (b, m) or tuple(go.shape) != (b, m, 3):
        raise H.invalid("merge_layer_grad expects idx2 (batch,#new) and grad (batch,#new,3)")
    ragged = lengths is not None or lengths_new is not None
    if ragged:
        lr, ln = _check_lengths(lengths, b, n, "lengths"), _check_lengths(lengths_new, b, m, "lengths_new")
    dev = st.device_()
    a, b_, ix, go = st.up(a, b_, ix, go)
    dec = torch.as_tensor(decfactor, dtype=F32).detach().reshape(-1)[:1].to(dev).contiguous()
    gn, gd = H.empty((b, m, 3), F32, dev), H.empty((b,), F32, dev)
    gr = H.empty((b, n, 3), F32, dev) if want_raw else None
    if ragged:
        lr, ln = _lengths_up(lr, dev, n), _lengths_up(ln, dev, m)
        check(lib.rf_merge_layer_grad_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(lr), H.ptr(ln), H.ptr(dec), H.ptr(ix),
                                              H.ptr(go), H.ptr(gn), H.ptr(gd), H.ptr(gr), H.stream(dev)),
              "rf_merge_layer_grad_lengths")
        return st.give(gn), st.give(gd), (None if gr is None else st.give(gr))
    check(lib.rf_merge_layer_grad(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(dec), H.ptr(ix), H.ptr(go), H.ptr(gn),
                                  H.ptr(gd), H.ptr(gr), H.stream(dev)), "rf_merge_layer_grad")
    return st.give(gn), st.give(gd), (None if gr is None else st.give(gr))


# ------------------------------------------------------------------ EMD --------------------
def _emd_inputs(st, xyz1, xyz2, opname):
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if not _shape3(a, 3):
        raise H.invalid(f"{opname} expects (batch_size,num_points,3) xyz1 shape")
    if not (_shape3(b_, 3) and b_.shape[0] == a.shape[0]):
        raise H.invalid(f"{opname} expects (batch_size,num_points,3) xyz2 shape, and batch_size must match")
    return a, b_


# rf_approxmatch_mode / rf_earth_mover_mode (include/rfops.h): "swept" pins the route -- a sample's bits do not depend on the batch
EMD_MODES = {"auto": 0, "swept": 1}


@H.on_input_device
def approx_match(xyz1, xyz2, levels=None, mode="auto", lengths1=None, lengths2=None):
    """ApproxMatchGpuOp::Compute, pc_distance/tf_approxmatch.cpp:148-172 -> match (b,m,n).

    `levels` (optional, extension): explicit annealing schedule; default = the reference's 10.
    `mode` (extension): "auto" | "swept" (batch-invariant bits per sample, as the reference's per-sample loop).
    `lengths1` / `lengths2` (extension): per-sample point counts of a ragged batch (rf_approxmatch_lengths): entries
    outside a sample's counts come back as 0.  With counts, "auto" and "swept" both run the pinned (swept) route.
    """
    if mode not in EMD_MODES:
        raise H.invalid(f"ApproxMatch: mode must be one of {sorted(EMD_MODES)}")
    st = H.Staged()
    a, b_ = _emd_inputs(st, xyz1, xyz2, "ApproxMatch")
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    nlv = 0 if levels is None else len(levels)
    if lengths1 is not None or lengths2 is not None:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
        dev = st.device_()
        a, b_ = st.up(a, b_)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        match = H.empty((b, m, n), F32, dev)
        ws, wsz = H.workspace(lib.rf_approxmatch_lengths_workspace_bytes(b, n, m, nlv), dev, "am")
        lv = None if levels is None else (C.c_float * nlv)(*[float(v) for v in levels])
        check(lib.rf_approxmatch_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(match), lv, nlv,
                                         H.ptr(ws), wsz, H.stream(dev)), "rf_approxmatch_lengths")
        return st.give(match)
    dev = st.device_()
    a, b_ = st.up(a, b_)
    match = H.empty((b, m, n), F32, dev)
    if mode != "auto":
        ws, wsz = H.workspace(lib.rf_approxmatch_mode_workspace_bytes(b, n, m, nlv, EMD_MODES[mode]), dev, "am")
        lv = None if levels is None else (C.c_float * nlv)(*[float(v) for v in levels])
        check(lib.rf_approxmatch_mode(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(match), lv, nlv, H.ptr(ws), wsz, H.stream(dev),
                                      EMD_MODES[mode]), "rf_approxmatch_mode")
        return st.give(match)
    ws, wsz = H.workspace(lib.rf_approxmatch_workspace_bytes(b, n, m, nlv), dev, "am")
    if levels is None:
        check(lib.rf_approxmatch(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(match), H.ptr(ws), wsz,
                                 H.stream(dev)), "rf_approxmatch")
    else:
        lv = (C.c_float * nlv)(*[float(v) for v in levels])
        check(lib.rf_approxmatch_levels(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(match), lv, nlv,
                                        H.ptr(ws), wsz, H.stream(dev)), "rf_approxmatch_levels")
    return st.give(match)


def _match_check(mt, b, n, m):
    if not (mt.dim() == 3 and mt.shape[0] == b and mt.shape[1] == m and mt.shape[2] == n):
        raise H.invalid("MatchCost expects (batch_size,#query,#dataset) match shape")


@H.on_input_device
def match_cost(xyz1, xyz2, match, lengths1=None, lengths2=None):
    """MatchCostGpuOp::Compute, pc_distance/tf_approxmatch.cpp:204-230 -> cost (b).  With `lengths1` / `lengths2`
    (rf_matchcost_lengths) only each sample's valid pairs are read and summed."""
    st = H.Staged()
    a, b_ = _emd_inputs(st, xyz1, xyz2, "MatchCost")
    mt = st.take(match, F32)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    _match_check(mt, b, n, m)
    if lengths1 is not None or lengths2 is not None:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
        dev = st.device_()
        a, b_, mt = st.up(a, b_, mt)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        cost = H.empty((b,), F32, dev)
        ws, wsz = H.workspace(lib.rf_matchcost_lengths_workspace_bytes(b, n, m), dev, "mc")
        check(lib.rf_matchcost_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(mt), H.ptr(cost),
                                       H.ptr(ws), wsz, H.stream(dev)), "rf_matchcost_lengths")
        return st.give(cost)
    dev = st.device_()
    a, b_, mt = st.up(a, b_, mt)
    cost = H.empty((b,), F32, dev)
    ws, wsz = H.workspace(lib.rf_matchcost_workspace_bytes(b, n, m), dev, "mc")
    check(lib.rf_matchcost(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(mt), H.ptr(cost), H.ptr(ws), wsz,
                           H.stream(dev)), "rf_matchcost")
    return st.give(cost)


@H.on_input_device
def match_cost_grad(xyz1, xyz2, match, lengths1=None, lengths2=None):
    """MatchCostGradGpuOp::Compute, pc_distance/tf_approxmatch.cpp:265-295.  With `lengths1` / `lengths2`
    (rf_matchcost_grad_lengths) only the valid pairs enter, and rows beyond a sample's count get a zero gradient."""
    st = H.Staged()
    a, b_ = _emd_inputs(st, xyz1, xyz2, "MatchCostGrad")
    mt = st.take(match, F32)
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    _match_check(mt, b, n, m)
    if lengths1 is not None or lengths2 is not None:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
        dev = st.device_()
        a, b_, mt = st.up(a, b_, mt)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
        check(lib.rf_matchcost_grad_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(mt), H.ptr(g1),
                                            H.ptr(g2), H.stream(dev)), "rf_matchcost_grad_lengths")
        return st.give(g1), st.give(g2)
    dev = st.device_()
    a, b_, mt = st.up(a, b_, mt)
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    check(lib.rf_matchcost_grad(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(mt), H.ptr(g1), H.ptr(g2),
                                H.stream(dev)), "rf_matchcost_grad")
    return st.give(g1), st.give(g2)


@H.on_input_device
def earth_mover(xyz1, xyz2, with_grad=False, mode="auto", lengths1=None, lengths2=None):
    """Row f1: the fused form of `earth_mover`'s op chain (vv_recon.py:392-399):
    approx_match -> match_cost [-> MatchCostGrad], without materialising match.
    -> cost (b)  or  (cost, grad1 (b,n,3), grad2 (b,m,3)) with `with_grad`.
    mode="swept": cost[i] bit-identical whatever the batch around sample i (rf_earth_mover_mode).
    `lengths1` / `lengths2`: per-sample point counts of a ragged batch (rf_earth_mover_lengths): the cost of each
    sample's valid pairs, zero gradient rows beyond the counts.  With counts, "auto" and "swept" both run the pinned
    (swept) route."""
    if mode not in EMD_MODES:
        raise H.invalid(f"ApproxMatch: mode must be one of {sorted(EMD_MODES)}")
    st = H.Staged()
    a, b_ = _emd_inputs(st, xyz1, xyz2, "ApproxMatch")
    b, n, m = a.shape[0], a.shape[1], b_.shape[1]
    ragged = lengths1 is not None or lengths2 is not None
    if ragged:
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    cost = H.empty((b,), F32, dev)
    g1 = H.empty((b, n, 3), F32, dev) if with_grad else None
    g2 = H.empty((b, m, 3), F32, dev) if with_grad else None
    if ragged:
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        ws, wsz = H.workspace(lib.rf_earth_mover_lengths_workspace_bytes(b, n, m), dev, "emd")
        check(lib.rf_earth_mover_lengths(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(l1), H.ptr(l2), H.ptr(cost),
                                         H.ptr(g1) if with_grad else None, H.ptr(g2) if with_grad else None,
                                         H.ptr(ws), wsz, H.stream(dev)), "rf_earth_mover_lengths")
        if with_grad:
            return st.give(cost), st.give(g1), st.give(g2)
        return st.give(cost)
    ws, wsz = H.workspace(lib.rf_earth_mover_mode_workspace_bytes(b, n, m, EMD_MODES[mode]), dev, "emd")
    check(lib.rf_earth_mover_mode(b, n, m, H.ptr(a), H.ptr(b_), H.ptr(cost),
                                  H.ptr(g1) if with_grad else None, H.ptr(g2) if with_grad else None,
                                  H.ptr(ws), wsz, H.stream(dev), EMD_MODES[mode]), "rf_earth_mover_mode")
    if with_grad:
        return st.give(cost), st.give(g1), st.give(g2)
    return st.give(cost)


# ------------------------------------------------------------------ sampling ---------------
@H.on_input_device
def farthest_point_sample(npoint, inp, lengths=None, npoints=None, with_xyz=False, _pin_reg=False):
    """FarthestPointSampleGpuOp, tf_ops/sampling/tf_sampling.cpp:95-123 -> (b,npoint) int32.

    lengths / npoints: a ragged batch (rf_farthestpointsampling_lengths) -- lengths[i] valid points in cloud i, npoints[i]
    samples wanted from it (at most npoint); row i holds the samples of inp[i, :lengths[i]] and zeros behind npoints[i].
    with_xyz (ragged form only): also the samples' coordinates (b,npoint,3), zeros behind npoints[i].
    (_pin_reg: the kernels of the unsorted cloud whatever the size -- rf_farthestpointsampling; a measurement aid.)"""
    npoint = int(npoint)
    if npoint <= 0:
        raise H.invalid("FarthestPointSample expects positive npoint")
    st = H.Staged()
    p = st.take(inp, F32)
    if not _shape3(p, 3):
        raise H.invalid("FarthestPointSample expects (batch_size,num_points,3) inp shape")
    b, n = p.shape[0], p.shape[1]
    if lengths is not None or npoints is not None:
        if _pin_reg:
            raise H.invalid("FarthestPointSample: _pin_reg is a measurement aid of the plain op")
        if n == 0:
            raise H.invalid("FarthestPointSample: a ragged batch needs at least one point per cloud")
        ln, lo = _check_lengths(lengths, b, n, "lengths"), _check_lengths(npoints, b, npoint, "npoints")
        dev = st.device_()
        p, = st.up(p)
        ln, lo = _lengths_up(ln, dev, n), _lengths_up(lo, dev, npoint)
        out = H.empty((b, npoint), I32, dev)
        nx = H.empty((b, npoint, 3), F32, dev) if with_xyz else None
        ws, wsz = H.workspace(lib.rf_farthestpointsampling_lengths_workspace_bytes(b, n, npoint), dev, "fps")
        check(lib.rf_farthestpointsampling_lengths(b, n, npoint, H.ptr(p), H.ptr(ln), H.ptr(lo), H.ptr(ws), wsz, H.ptr(out),
                                                   H.ptr(nx), H.stream(dev)), "rf_farthestpointsampling_lengths")
        return (st.give(out), st.give(nx)) if with_xyz else st.give(out)
    if with_xyz:
        raise H.invalid("FarthestPointSample: with_xyz belongs to the ragged form (farthest_point_sample_sorted has its own)")
    dev = st.device_()
    p, = st.up(p)
    out = H.empty((b, npoint), I32, dev)
    if _pin_reg:
        nt = lib.rf_farthestpointsampling_temp_floats(b, n)
        temp = H.empty((nt,), F32, dev) if nt else None
        check(lib.rf_farthestpointsampling(b, n, npoint, H.ptr(p), H.ptr(temp), H.ptr(out),
                                           H.stream(dev)), "rf_farthestpointsampling")
        return st.give(out)
    ws, wsz = H.workspace(lib.rf_farthestpointsampling_workspace_bytes(b, n, npoint), dev, "fps")
    check(lib.rf_farthestpointsampling_ws(b, n, npoint, H.ptr(p), H.ptr(ws), wsz, H.ptr(out), H.stream(dev)),
          "rf_farthestpointsampling_ws")
    return st.give(out)


def farthest_point_sample_reg(npoint, inp):
    """farthest_point_sample pinned to the register-resident kernel of the unsorted cloud (measurement aid)."""
    return farthest_point_sample(npoint, inp, _pin_reg=True)


@H.on_input_device
def farthest_point_sample_sorted(npoint, inp, form=0, with_xyz=False):
    """farthest_point_sample over the spatially sorted cloud (sampling.hip fps_sorted_kernel): the same indices, for clouds of
    1025..16384 points.  -> idx (b, npoint) [, new_xyz (b, npoint, 3)]"""
    npoint = int(npoint)
    if npoint <= 0:
        raise H.invalid("FarthestPointSample expects positive npoint")
    st = H.Staged()
    p = st.take(inp, F32)
    if not _shape3(p, 3):
        raise H.invalid("FarthestPointSample expects (batch_size,num_points,3) inp shape")
    b, n = p.shape[0], p.shape[1]
    dev = st.device_()
    p, = st.up(p)
    out = H.empty((b, npoint), I32, dev)
    nx = H.empty((b, npoint, 3), F32, dev) if with_xyz else None
    ws, wsz = H.workspace(lib.rf_farthestpointsampling_sorted_workspace_bytes(b, n), dev, "fps")
    check(lib.rf_farthestpointsampling_sorted(b, n, npoint, int(form), H.ptr(p), H.ptr(ws), wsz, H.ptr(out), H.ptr(nx),
                                              H.stream(dev)), "rf_farthestpointsampling_sorted")
    if with_xyz:
        return st.give(out), st.give(nx)
    return st.give(out)


@H.on_input_device
def gather_point(inp, idx):
    """GatherPointGpuOp, tf_sampling.cpp:126-148 -> (b,m,3)."""
    st = H.Staged()
    p, ix = st.take(inp, F32), st.take(idx, I32)
    if not _shape3(p, 3):
        raise H.invalid("GatherPoint expects (batch_size,num_points,3) inp shape")
    if not (ix.dim() == 2 and ix.shape[0] == p.shape[0]):
        raise H.invalid("GatherPoint expects (batch_size,num_result) idx shape")
    b, n, m = p.shape[0], p.shape[1], ix.shape[1]
    dev = st.device_()
    p, ix = st.up(p, ix)
    out = H.empty((b, m, 3), F32, dev)
    check(lib.rf_gatherpoint(b, n, m, H.ptr(p), H.ptr(ix), H.ptr(out), H.stream(dev)),
          "rf_gatherpoint")
    return st.give(out)


@H.on_input_device
def gather_point_grad(inp, idx, out_g):
    """GatherPointGradGpuOp, tf_sampling.cpp:151-178 -> (b,n,3)."""
    st = H.Staged()
    p, ix, og = st.take(inp, F32), st.take(idx, I32), st.take(out_g, F32)
    if not _shape3(p, 3):
        raise H.invalid("GatherPointGradGpuOp expects (batch_size,num_points,3) inp")
    if not (ix.dim() == 2 and ix.shape[0] == p.shape[0]):
        raise H.invalid("GatherPointGradGpuOp expects (batch_size,num_result) idx shape")
    b, n, m = p.shape[0], p.shape[1], ix.shape[1]
    if tuple(og.shape) != (b, m, 3):
        raise H.invalid("GatherPointGradGpuOp expects (batch_size,num_result,3) out_g shape")
    dev = st.device_()
    p, ix, og = st.up(p, ix, og)
    g = H.empty((b, n, 3), F32, dev)
    check(lib.rf_scatteraddpoint(b, n, m, H.ptr(og), H.ptr(ix), H.ptr(g), H.stream(dev)),
          "rf_scatteraddpoint")
    return st.give(g)


# ------------------------------------------------------------------ grouping ---------------
QB_BOXES_MIN_N = 2048  # datasets from this size on take the boxed kernel (its sort costs ~20 us whatever the size)
GROUP_FORMS = {"auto": 0, "scan": 1, "boxes": 2}  # RF_GROUP_* (include/rfops.h): the `form` of the ragged entries


def _radius_arg(radius, dev):
    """-> (value, device tensor or None): a CUDA radius tensor is the reference's op input (tf_grouping.cpp:18,93-95)."""
    if isinstance(radius, torch.Tensor) and radius.is_cuda:
        if radius.device != dev:
            raise ValueError(f"all GPU inputs of one op must live on the same device: got {dev} and {radius.device}")
        return 0.0, radius.detach().reshape(-1)[:1].to(F32).contiguous()
    return float(np.float32(float(radius))), None


@H.on_input_device
def query_ball_point(radius, nsample, xyz1, xyz2, sorted1=None, form="auto", lengths1=None, lengths2=None):
    """QueryBallPointGpuOp, tf_ops/grouping/tf_grouping.cpp:68-110 -> idx (b,m,nsample), pts_cnt (b,m).

    Rows whose ball is empty are not written by the kernel (as in the reference, whose output
    buffer is then uninitialised); this wrapper allocates idx zero-filled so they read 0.
    form: "auto" (the boxed kernel for datasets of QB_BOXES_MIN_N points and more, the scan below that), "boxes",
    "scan" -- same results; sorted1: an rf_nn_sort handle of xyz1 (nn_sort), skips the boxed form's own sort.
    lengths1 / lengths2: a ragged batch (rf_queryballpoint_lengths) -- points per dataset, queries per sample; EVERY row is
    then written by the kernel: an empty ball and a padded query read idx 0, pts_cnt 0.  Not together with sorted1 (a handle
    was sorted without counts).
    """
    nsample = int(nsample)
    if nsample <= 0:
        raise H.invalid("QueryBallPoint expects positive nsample")
    ragged = lengths1 is not None or lengths2 is not None
    if ragged and sorted1 is not None:
        raise H.invalid("QueryBallPoint: lengths cannot be combined with a sorted handle (it was sorted without counts)")
    st = H.Staged()
    d, q = st.take(xyz1, F32), st.take(xyz2, F32)
    if not _shape3(d, 3):
        raise H.invalid("QueryBallPoint expects (batch_size, ndataset, 3) xyz1 shape.")
    if not _shape3(q, 3):
        raise H.invalid("QueryBallPoint expects (batch_size, npoint, 3) xyz2 shape.")
    b, n, m = d.shape[0], d.shape[1], q.shape[1]
    if ragged:
        if form not in GROUP_FORMS:
            raise H.invalid(f"QueryBallPoint: form must be one of {sorted(GROUP_FORMS)}")
        if q.shape[0] != b or n == 0 or m == 0:
            raise H.invalid("QueryBallPoint: a ragged batch needs one non-empty dataset and query set per sample")
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
        dev = st.device_()
        d, q = st.up(d, q)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        r, rt = _radius_arg(radius, dev)
        f = GROUP_FORMS[form]
        wsz = lib.rf_queryballpoint_lengths_workspace_bytes(b, n, m, nsample, f)
        if form == "boxes" and not wsz:
            raise H.invalid("QueryBallPoint: the boxed form takes datasets of 64..65536 points and nsample <= 64")
        idx, cnt = H.empty((b, m, nsample), I32, dev), H.empty((b, m), I32, dev)
        ws = H.empty((wsz // 4,), F32, dev) if wsz else None
        check(lib.rf_queryballpoint_lengths(b, n, m, r, H.ptr(rt), nsample, H.ptr(d), H.ptr(q), H.ptr(l1), H.ptr(l2),
                                            H.ptr(idx), H.ptr(cnt), H.ptr(ws), wsz, H.stream(dev), f),
              "rf_queryballpoint_lengths")
        return st.give(idx), st.give(cnt)
    dev = st.device_()
    d, q = st.up(d, q)
    idx = H.zeros((b, m, nsample), I32, dev)
    cnt = H.empty((b, m), I32, dev)
    r, rt = _radius_arg(radius, dev)
    wsz = lib.rf_queryballpoint_boxes_workspace_bytes(b, n) if nsample <= 64 and b <= 65535 else 0
    boxes = form == "boxes" or (form == "auto" and n >= QB_BOXES_MIN_N)
    if form == "boxes" and not wsz:
        raise H.invalid("QueryBallPoint: the boxed form takes datasets of 64..65536 points and nsample <= 64")
    if boxes and wsz and b * m > 0:
        ws = H.empty((wsz // 4,), F32, dev)
        check(lib.rf_queryballpoint_boxes(b, n, m, r, H.ptr(rt), nsample, H.ptr(d), H.ptr(q),
                                          H.ptr(sorted1) if sorted1 is not None else None, H.ptr(idx), H.ptr(cnt),
                                          H.ptr(ws), wsz, H.stream(dev)), "rf_queryballpoint_boxes")
    elif rt is not None:
        check(lib.rf_queryballpoint_dev(b, n, m, H.ptr(rt), nsample, H.ptr(d), H.ptr(q), H.ptr(idx),
                                        H.ptr(cnt), H.stream(dev)), "rf_queryballpoint_dev")
    else:
        check(lib.rf_queryballpoint(b, n, m, r, nsample, H.ptr(d), H.ptr(q), H.ptr(idx), H.ptr(cnt),
                                    H.stream(dev)), "rf_queryballpoint")
    return st.give(idx), st.give(cnt)


@H.on_input_device
def sample_and_group(npoint, radius, nsample, xyz, aux_stream=None, lengths=None, npoints=None):
    """rf_sample_and_group: farthest_point_sample -> gather_point -> query_ball_point -> group_point(xyz) as one call
    -> (fps_idx (b,npoint), new_xyz (b,npoint,3), idx (b,npoint,nsample), pts_cnt (b,npoint), grouped_xyz (b,npoint,nsample,3)),
    bit-identical to the four ops.  aux_stream: a torch.cuda.Stream on which the dataset's sort runs beside FPS.
    lengths / npoints: a ragged batch (rf_sample_and_group_lengths) -- points per cloud, samples wanted per cloud; the rows of
    samples behind npoints[i] are zeros in all five outputs."""
    npoint, nsample = int(npoint), int(nsample)
    if npoint <= 0:
        raise H.invalid("FarthestPointSample expects positive npoint")
    if nsample <= 0:
        raise H.invalid("QueryBallPoint expects positive nsample")
    st = H.Staged()
    p = st.take(xyz, F32)
    if not _shape3(p, 3):
        raise H.invalid("FarthestPointSample expects (batch_size,num_points,3) inp shape")
    b, n = p.shape[0], p.shape[1]
    ragged = lengths is not None or npoints is not None
    ln, lo = _check_lengths(lengths, b, n, "lengths"), _check_lengths(npoints, b, npoint, "npoints")
    dev = st.device_()
    p, = st.up(p)
    ln, lo = _lengths_up(ln, dev, n), _lengths_up(lo, dev, npoint)
    wsz = lib.rf_sample_and_group_workspace_bytes(b, n) if nsample <= 64 and b <= 65535 else 0
    if not wsz:
        raise H.invalid("sample_and_group takes clouds of 64..65536 points and nsample <= 64")
    rt = None
    if isinstance(radius, torch.Tensor) and radius.is_cuda:
        rt = radius.detach().reshape(-1)[:1].to(F32).contiguous()
        r = 0.0
    else:
        r = float(np.float32(float(radius)))
    fi = H.empty((b, npoint), I32, dev)
    nx = H.empty((b, npoint, 3), F32, dev)
    gi = H.empty((b, npoint, nsample), I32, dev)
    cnt = H.empty((b, npoint), I32, dev)
    gx = H.empty((b, npoint, nsample, 3), F32, dev)
    ws = H.empty((wsz // 4,), F32, dev)
    aux = aux_stream.cuda_stream if aux_stream is not None else None
    if ragged:
        check(lib.rf_sample_and_group_lengths(b, n, npoint, r, H.ptr(rt), nsample, H.ptr(p), H.ptr(ln), H.ptr(lo), H.ptr(fi),
                                              H.ptr(nx), H.ptr(gi), H.ptr(cnt), H.ptr(gx), H.ptr(ws), wsz, H.stream(dev), aux),
              "rf_sample_and_group_lengths")
    else:
        check(lib.rf_sample_and_group(b, n, npoint, r, H.ptr(rt), nsample, H.ptr(p), H.ptr(fi), H.ptr(nx), H.ptr(gi),
                                      H.ptr(cnt), H.ptr(gx), H.ptr(ws), wsz, H.stream(dev), aux), "rf_sample_and_group")
    if aux_stream is not None:
        ws.record_stream(aux_stream)  # the sort wrote the workspace on that stream
    return st.give(fi), st.give(nx), st.give(gi), st.give(cnt), st.give(gx)


@H.on_input_device
def group_point(points, idx):
    """GroupPointGpuOp, tf_grouping.cpp:147-175 -> (b,m,nsample,c)."""
    st = H.Staged()
    p, ix = st.take(points, F32), st.take(idx, I32)
    if p.dim() != 3:
        raise H.invalid("GroupPoint expects (batch_size, num_points, channel) points shape")
    if not (ix.dim() == 3 and ix.shape[0] == p.shape[0]):
        raise H.invalid("GroupPoint expects (batch_size, npoints, nsample) idx shape")
    b, n, c = p.shape
    m, ns = ix.shape[1], ix.shape[2]
    dev = st.device_()
    p, ix = st.up(p, ix)
    out = H.empty((b, m, ns, c), F32, dev)
    check(lib.rf_grouppoint(b, n, c, m, ns, H.ptr(p), H.ptr(ix), H.ptr(out), H.stream(dev)),
          "rf_grouppoint")
    return st.give(out)


@H.on_input_device
def group_point_grad(points, idx, grad_out, form="auto"):
    """GroupPointGradGpuOp, tf_grouping.cpp:178-212 -> (b,n,c).
    form: "auto" (rf_grouppoint_grad_ws: sorted slots where they pay) | "atomic" (the reference's form, rf_grouppoint_grad)."""
    st = H.Staged()
    p, ix, go = st.take(points, F32), st.take(idx, I32), st.take(grad_out, F32)
    if p.dim() != 3:
        raise H.invalid("GroupPointGrad expects (batch_size, num_points, channel) points shape")
    if not (ix.dim() == 3 and ix.shape[0] == p.shape[0]):
        raise H.invalid("GroupPointGrad expects (batch_size, npoints, nsample) idx shape")
    b, n, c = p.shape
    m, ns = ix.shape[1], ix.shape[2]
    if tuple(go.shape) != (b, m, ns, c):
        raise H.invalid("GroupPointGrad expects (batch_size, npoints, nsample, channel) grad_out shape")
    dev = st.device_()
    p, ix, go = st.up(p, ix, go)
    g = H.empty((b, n, c), F32, dev)
    if form == "atomic":
        check(lib.rf_grouppoint_grad(b, n, c, m, ns, H.ptr(go), H.ptr(ix), H.ptr(g), H.stream(dev)),
              "rf_grouppoint_grad")
        return st.give(g)
    ws, wsz = H.workspace(lib.rf_grouppoint_grad_workspace_bytes(b, n, c, m, ns), dev, "gpg")
    check(lib.rf_grouppoint_grad_ws(b, n, c, m, ns, H.ptr(go), H.ptr(ix), H.ptr(g), H.ptr(ws), wsz, H.stream(dev)),
          "rf_grouppoint_grad_ws")
    return st.give(g)


# ------------------------------------------------------------------ interpolation ----------
# three_nn: pairs per call from which sorting both sets is repaid (tools/ab_three_nn.py: the sort is ~25 us for sets of up to
# 16384 points -- one workgroup per cloud with the points in registers -- and ~270 us beyond)
TN_BOXES_MIN_PAIRS = 100_000_000
TN_BOXES_MIN_PAIRS_LARGE = 4_000_000_000
TN_BOXES_MIN_KNOWN = 512  # fewer known points: a handful of blocks, nothing to skip


@H.on_input_device
def three_nn(xyz1, xyz2, form="auto", sorted1=None, sorted2=None, lengths1=None, lengths2=None):
    """ThreeNNOp, tf_ops/interpolation/tf_interpolate.cpp:157-187 -> dist (b,n,3), idx (b,n,3).

    form: "auto" (the boxed kernel over sorted copies of the two sets from TN_BOXES_MIN_PAIRS pairs per call on, the scan
    below that), "boxes", "scan" -- same results, ties included; sorted1 / sorted2: rf_nn_sort handles of xyz1 / xyz2
    (nn_sort), which skip the boxed form's own sort of that set.
    lengths1 / lengths2: a ragged batch (rf_threenn_lengths) -- unknown / known points per sample; rows behind lengths1[i] come
    back as zeros.  Not together with sorted handles (they were sorted without counts)."""
    ragged = lengths1 is not None or lengths2 is not None
    if ragged and (sorted1 is not None or sorted2 is not None):
        raise H.invalid("ThreeNN: lengths cannot be combined with sorted handles (they were sorted without counts)")
    st = H.Staged()
    u, k = st.take(xyz1, F32), st.take(xyz2, F32)
    if not _shape3(u, 3):
        raise H.invalid("ThreeNN expects (b,n,3) xyz1 shape.")
    if not _shape3(k, 3):
        raise H.invalid("ThreeNN expects (b,m,3) xyz2 shape.")
    b, n, m = u.shape[0], u.shape[1], k.shape[1]
    if ragged:
        if form not in GROUP_FORMS:
            raise H.invalid(f"ThreeNN: form must be one of {sorted(GROUP_FORMS)}")
        if k.shape[0] != b or n == 0 or m == 0 or b > 65535:
            raise H.invalid("ThreeNN: a ragged batch needs one non-empty set of each kind per sample (b <= 65535)")
        l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
        dev = st.device_()
        u, k = st.up(u, k)
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        f = GROUP_FORMS[form]
        wsz = lib.rf_threenn_lengths_workspace_bytes(b, n, m, f)
        if form == "boxes" and not wsz:
            raise H.invalid("ThreeNN: the boxed form takes sets of 1..65536 points")
        dist, idx = H.empty((b, n, 3), F32, dev), H.empty((b, n, 3), I32, dev)
        ws = H.empty((wsz // 4,), F32, dev) if wsz else None
        check(lib.rf_threenn_lengths(b, n, m, H.ptr(u), H.ptr(k), H.ptr(l1), H.ptr(l2), H.ptr(dist), H.ptr(idx), H.ptr(ws),
                                     wsz, H.stream(dev), f), "rf_threenn_lengths")
        return st.give(dist), st.give(idx)
    dev = st.device_()
    u, k = st.up(u, k)
    dist, idx = H.empty((b, n, 3), F32, dev), H.empty((b, n, 3), I32, dev)
    wsz = lib.rf_threenn_boxes_workspace_bytes(b, n, m) if b * n * m > 0 else 0
    need = TN_BOXES_MIN_PAIRS if max(n if sorted1 is None else 0, m if sorted2 is None else 0) <= 16384 else TN_BOXES_MIN_PAIRS_LARGE
    if sorted1 is not None and sorted2 is not None:
        # nothing to sort: the boxed kernel alone wins from much smaller calls on (32 x 2048 x 512: 0.025 against 0.033 ms)
        boxes = form == "boxes" or (form == "auto" and n >= 1024 and m >= 256 and b * n * m >= TN_BOXES_MIN_PAIRS // 4)
    else:
        boxes = form == "boxes" or (form == "auto" and n >= 1024 and m >= TN_BOXES_MIN_KNOWN and
                                    (b * n * m >= need or (m >= 1536 and n >= 4096 and need == TN_BOXES_MIN_PAIRS)))
    # (the second clause: with few waves on the chip the scan is a chain of m candidates at ~0.05 us each whatever b -- 1 x 16384 x 2048:
    # 0.103 ms against 0.045 boxed)
    if form == "boxes" and not wsz:
        raise H.invalid("ThreeNN: the boxed form takes sets of 1..65536 points")
    if boxes and wsz:
        ws = H.empty((wsz // 4,), F32, dev)
        check(lib.rf_threenn_boxes(b, n, m, H.ptr(u), H.ptr(k), H.ptr(sorted1) if sorted1 is not None else None,
                                   H.ptr(sorted2) if sorted2 is not None else None, H.ptr(dist), H.ptr(idx), H.ptr(ws), wsz,
                                   H.stream(dev)), "rf_threenn_boxes")
    else:
        check(lib.rf_threenn(b, n, m, H.ptr(u), H.ptr(k), H.ptr(dist), H.ptr(idx), H.stream(dev)),
              "rf_threenn")
    return st.give(dist), st.give(idx)


# knn_point: where the boxed form (rf_knn_boxes) beats the scan (tools/ab_knn.py, profiles/knn_ab.txt).  The scan's time is that of
# one wave's chain over the n candidates, whatever b and m (1.02-1.11 ms at n = 16384, k = 16, from 1 x 1024 to 64 x 1024 queries);
# the boxed form pays when a sample has many queries, so that a wave's 64 queries sit close together: it won at every measured
# shape with m >= 8192, n >= 16384 and k <= 32 (0.40 against 1.02 ms at 1 x 16384 x 16384, k = 16; 0.51 against 1.04 at
# 8 x 16384 x 8192) and lost at every other (m <= 4096 whatever b: 1.51 against 1.04 ms at 64 x 16384 x 1024; n <= 4096; k = 64:
# 2.68 against 2.63 at 4 x 16384 x 16384).  Caller sort handles moved no shape across the line.
KNN_BOXES_MIN_QUERIES = 8192
KNN_BOXES_MIN_CANDIDATES = 16384
KNN_BOXES_MAX_K = 32
KNN_MAX_K = 64


def _knn_inputs(st, xyz1, xyz2, k, op):
    a, q = st.take(xyz1, F32), st.take(xyz2, F32)
    if not _shape3(a, 3):
        raise H.invalid(f"{op} expects (b,n,3) xyz1 shape")
    if not (_shape3(q, 3) and q.shape[0] == a.shape[0]):
        raise H.invalid(f"{op} expects (b,m,3) xyz2 shape, and batch_size must match")
    b, n, m = a.shape[0], a.shape[1], q.shape[1]
    if not 1 <= k <= min(n, KNN_MAX_K):
        raise H.invalid(f"{op} takes 1 <= k <= min(n, {KNN_MAX_K})")
    if not (1 <= b <= 65535 and 1 <= n <= 65536 and 1 <= m <= 65536):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and clouds of 1..65536 points")
    return a, q, b, n, m


def knn_supported(k, b, n, m):
    """The domain of the kernels (include/rfops.h rf_knn)."""
    return 1 <= k <= min(n, KNN_MAX_K) and 1 <= b <= 65535 and 1 <= n <= 65536 and 1 <= m <= 65536


def knn_auto_boxes(k, n, m):
    """form="auto" takes the boxed kernel (KNN_BOXES_* above)."""
    return m >= KNN_BOXES_MIN_QUERIES and n >= KNN_BOXES_MIN_CANDIDATES and k <= KNN_BOXES_MAX_K


@H.on_input_device
def knn_point(k, xyz1, xyz2, form="auto", sorted1=None, sorted2=None, lengths1=None, lengths2=None):
    """knn_point (tf_ops/grouping/tf_grouping.py:48-73) on the GPU -> val (b,m,k) = -d, idx (b,m,k) int32: per query of xyz2 the
    k points of xyz1 of smallest squared distance, ascending, ties to the lower index (tf.nn.top_k's rule).

    form: "auto" (the boxed kernel over sorted copies of the two sets where it measured faster -- m >= KNN_BOXES_MIN_QUERIES,
    n >= KNN_BOXES_MIN_CANDIDATES, k <= KNN_BOXES_MAX_K -- the scan elsewhere), "boxes", "scan" -- same results, bit for bit; sorted1 / sorted2: rf_nn_sort handles (nn_sort(...).buf) of
    xyz1 / xyz2, which skip the boxed form's own sort of that set.
    lengths1 / lengths2: a ragged batch (rf_knn_lengths) -- candidates / queries per sample.  Rows of padded queries come back
    as zeros; a sample with fewer candidates than k gets its lengths1[i] neighbours and zeros behind them.  Not together with
    sorted handles (they were sorted without counts)."""
    if form not in ("auto", "scan", "boxes"):
        raise H.invalid("knn_point: form must be one of auto, scan, boxes")
    ragged = lengths1 is not None or lengths2 is not None
    if ragged and (sorted1 is not None or sorted2 is not None):
        raise H.invalid("knn_point: lengths cannot be combined with sorted handles (they were sorted without counts)")
    k = int(k)
    st = H.Staged()
    a, q, b, n, m = _knn_inputs(st, xyz1, xyz2, k, "KnnPoint")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, q = st.up(a, q)
    val, idx = H.empty((b, m, k), F32, dev), H.empty((b, m, k), I32, dev)
    if ragged:
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        f = GROUP_FORMS[form]
        wsz = int(lib.rf_knn_lengths_workspace_bytes(b, n, m, k, f))
        ws = H.empty((wsz // 4,), F32, dev) if wsz else None
        check(lib.rf_knn_lengths(b, n, m, k, H.ptr(a), H.ptr(q), H.ptr(l1), H.ptr(l2), H.ptr(val), H.ptr(idx), H.ptr(ws), wsz,
                                 H.stream(dev), f), "rf_knn_lengths")
        return st.give(val), st.give(idx)
    boxes = form == "boxes" or (form == "auto" and knn_auto_boxes(k, n, m))
    if boxes:
        wsz = int(lib.rf_knn_boxes_workspace_bytes(b, n, m))
        ws = H.empty((wsz // 4,), F32, dev)
        check(lib.rf_knn_boxes(b, n, m, k, H.ptr(a), H.ptr(q), H.ptr(sorted1), H.ptr(sorted2), H.ptr(val), H.ptr(idx),
                               H.ptr(ws), wsz, H.stream(dev)), "rf_knn_boxes")
    else:
        check(lib.rf_knn(b, n, m, k, H.ptr(a), H.ptr(q), H.ptr(val), H.ptr(idx), H.stream(dev)), "rf_knn")
    return st.give(val), st.give(idx)


KNN_FEATURE_MAX_CHANNELS = 2048


@H.on_input_device
def knn_feature(k, feat1, feat2, lengths1=None, lengths2=None):
    """rf_knn_feature: knn_point in feature space (DGCNN's dynamic graph) -> val (b,m,k) = -d, idx (b,m,k) int32: per row of
    feat2 (b,m,c) the k rows of feat1 (b,n,c) of smallest d = |q|^2 + |x|^2 - 2 q.x, ascending by (d, index), ties to the lower
    index, a NaN distance first.  Every fp32 operation of d is prescribed (include/rfops.h) and the inner products come from the
    fp32 matrix instruction; no (b,m,n) tensor is formed.  d is the formula's value, not the rounded squared distance: it can be
    slightly negative, so a row that queries itself is not guaranteed slot 0 among near-duplicates.
    lengths1 / lengths2: a ragged batch, knn_point's rule -- candidates / queries per sample; rows of padded queries come back as
    zeros, a sample with fewer candidates than k gets its lengths1[i] neighbours and zeros behind them."""
    op = "KnnFeature"
    k = int(k)
    st = H.Staged()
    a, q = st.take(feat1, F32), st.take(feat2, F32)
    if not _shape3(a):
        raise H.invalid(f"{op} expects (b,n,c) feat1 shape")
    if not (_shape3(q, a.shape[2]) and q.shape[0] == a.shape[0]):
        raise H.invalid(f"{op} expects (b,m,c) feat2 shape, and batch_size and channels must match")
    b, n, c, m = a.shape[0], a.shape[1], a.shape[2], q.shape[1]
    if not 1 <= k <= min(n, KNN_MAX_K):
        raise H.invalid(f"{op} takes 1 <= k <= min(n, {KNN_MAX_K})")
    if not (1 <= b <= 65535 and 1 <= n <= 65536 and 1 <= m <= 65536):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1..65536 rows")
    if not 1 <= c <= KNN_FEATURE_MAX_CHANNELS:
        raise H.invalid(f"{op} takes 1 to {KNN_FEATURE_MAX_CHANNELS} channels")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, q = st.up(a, q)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    val, idx = H.empty((b, m, k), F32, dev), H.empty((b, m, k), I32, dev)
    ws, wsz = H.workspace(lib.rf_knn_feature_workspace_bytes(b, n, m, c, k), dev, "knn_feature")
    check(lib.rf_knn_feature(b, n, m, c, k, H.ptr(a), H.ptr(q), H.ptr(l1), H.ptr(l2), H.ptr(val), H.ptr(idx), H.ptr(ws), wsz,
                             H.stream(dev)), "rf_knn_feature")
    return st.give(val), st.give(idx)


PCA_MAX_K = 64  # RF_PCA_MAX_K (include/rfops.h)


@H.on_input_device
def local_pca(xyz, idx, lengths1=None, lengths2=None, viewpoint=None, want_axes=False):
    """rf_local_pca: per row of idx (b,m,k) the eigen-decomposition of the covariance of the rows of xyz (b,n,3) it names ->
    (normals (b,m,3), eigenvalues (b,m,3) ascending, axes (b,m,3,3) or None): cyclic Jacobi in double, every operation
    prescribed (include/rfops.h).  idx is what knn_point returned; lengths1 / lengths2: knn_point's own counts (source points /
    queries per sample) -- padded rows come back as zeros.  viewpoint (b,3): the normal is turned towards it."""
    op = "LocalPca"
    st = H.Staged()
    a, ix = st.take(xyz, F32), st.take(idx, I32)
    if not _shape3(a, 3):
        raise H.invalid(f"{op} expects (b,n,3) xyz shape")
    if not (_shape3(ix) and ix.shape[0] == a.shape[0]):
        raise H.invalid(f"{op} expects (b,m,k) idx shape, and batch_size must match")
    b, n, m, k = a.shape[0], a.shape[1], ix.shape[1], ix.shape[2]
    if not 1 <= k <= PCA_MAX_K:
        raise H.invalid(f"{op} takes 1 <= k <= {PCA_MAX_K}")
    if not (1 <= b <= 65535 and 1 <= n <= 65536 and 1 <= m <= 65536):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1..65536 points and queries")
    vp = None
    if viewpoint is not None:
        vp = st.take(viewpoint, F32)
        if tuple(vp.shape) != (b, 3):
            raise H.invalid(f"{op} expects (b,3) viewpoint shape")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, ix = st.up(a, ix)
    if vp is not None:
        vp, = st.up(vp)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    nrm, eig = H.empty((b, m, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    axes = H.empty((b, m, 3, 3), F32, dev) if want_axes else None
    check(lib.rf_local_pca(b, n, m, k, H.ptr(a), H.ptr(ix), H.ptr(l1), H.ptr(l2), H.ptr(vp), H.ptr(nrm), H.ptr(eig), H.ptr(axes),
                           H.stream(dev)), "rf_local_pca")
    return st.give(nrm), st.give(eig), None if axes is None else st.give(axes)


@H.on_input_device
def nn_normal_consistency(normals1, normals2, idx1, idx2, lengths1=None, lengths2=None):
    """rf_nn_normal_consistency: normals1 (b,n,3) / normals2 (b,m,3) and nn_distance's idx1 (b,n) / idx2 (b,m) -> (b,4):
    the means of |n1 . n2[idx1]| and |n2 . n1[idx2]|, then the two signed means (include/rfops.h)."""
    op = "NnNormalConsistency"
    st = H.Staged()
    a, c = st.take(normals1, F32), st.take(normals2, F32)
    i1, i2 = st.take(idx1, I32), st.take(idx2, I32)
    if not (_shape3(a, 3) and _shape3(c, 3) and a.shape[0] == c.shape[0]):
        raise H.invalid(f"{op} expects (b,n,3) normals1 and (b,m,3) normals2")
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    if tuple(i1.shape) != (b, n) or tuple(i2.shape) != (b, m):
        raise H.invalid(f"{op} expects (b,n) idx1 and (b,m) idx2")
    if not (1 <= b <= 65535 and n >= 1 and m >= 1):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and clouds of at least one point")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, c, i1, i2 = st.up(a, c, i1, i2)
    l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
    out = H.empty((b, 4), F32, dev)
    check(lib.rf_nn_normal_consistency(b, n, m, H.ptr(a), H.ptr(c), H.ptr(i1), H.ptr(i2), H.ptr(l1), H.ptr(l2), H.ptr(out),
                                       H.stream(dev)), "rf_nn_normal_consistency")
    return st.give(out)


GC_MAX_POINTS, GP_MAX_CHANNELS = 16384, 2048  # RF_GC_MAX_POINTS, RF_GP_MAX_CHANNELS (include/rfops.h)
GC_ORDERS = {"xyz": 0, "z": 1, "hilbert": 2}   # RF_GC_XYZ, RF_GC_Z, RF_GC_HILBERT
GP_REDUCES = {"sum": 0, "mean": 1, "max": 2}   # RF_GP_SUM, RF_GP_MEAN, RF_GP_MAX
GU_MODES = {"copy": 0, "mean": 1, "max": 2}    # RF_GU_COPY, RF_GU_MEAN, RF_GU_MAX


@H.on_input_device
def grid_cluster(xyz, cell, order="xyz", lengths=None, origin=None, want_code=False):
    """rf_grid_cluster: the occupied cells of edge `cell` of every cloud of xyz (b,n,3), n <= 16384, by a sort of integer cell
    keys along `order` ("xyz" row-major, "z" Morton, "hilbert") -> a dict of device tensors: "origin" (b,3) the origin used
    (`origin` (b,3), or the per-axis minimum of the sample), "inside" (b,) and "nclusters" (b,) int32, "order" (b,n) the inside
    points in key order, "starts" (b,n+1), "cluster" (b,n) with -1 for rows that are not inside, "coords" (b,n,3) int32 and,
    with want_code, "code" (b,n) int64 (include/rfops.h states every operation).  lengths: points per sample."""
    op = "GridCluster"
    st = H.Staged()
    a = st.take(xyz, F32)
    if not _shape3(a, 3):
        raise H.invalid(f"{op} expects (b,n,3) xyz shape")
    b, n = a.shape[0], a.shape[1]
    if not (1 <= b <= 65535 and 1 <= n <= GC_MAX_POINTS):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1 <= n <= {GC_MAX_POINTS} points")
    cell = float(np.float32(cell))
    if not (np.isfinite(cell) and cell > 0):
        raise H.invalid(f"{op} takes a finite cell > 0")
    if order not in GC_ORDERS:
        raise H.invalid(f"{op} takes order in {sorted(GC_ORDERS)}")
    og = None
    if origin is not None:
        og = st.take(origin, F32)
        if tuple(og.shape) != (b, 3):
            raise H.invalid(f"{op} expects (b,3) origin shape")
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = st.device_()
    a, = st.up(a)
    if og is not None:
        og, = st.up(og)
    ln = _lengths_up(ln, dev, n)
    r = {"origin": H.empty((b, 3), F32, dev), "inside": H.empty((b,), I32, dev), "nclusters": H.empty((b,), I32, dev),
         "order": H.empty((b, n), I32, dev), "starts": H.empty((b, n + 1), I32, dev), "cluster": H.empty((b, n), I32, dev),
         "coords": H.empty((b, n, 3), I32, dev)}
    if want_code:
        r["code"] = H.empty((b, n), torch.int64, dev)
    check(lib.rf_grid_cluster(b, n, cell, GC_ORDERS[order], H.ptr(a), H.ptr(ln), H.ptr(og), H.ptr(r["origin"]),
                              H.ptr(r["inside"]), H.ptr(r["nclusters"]), H.ptr(r["order"]), H.ptr(r["starts"]),
                              H.ptr(r["cluster"]), H.ptr(r["coords"]), H.ptr(r.get("code")), H.stream(dev)), "rf_grid_cluster")
    return {k: st.give(v) for k, v in r.items()}


def _gp_rows(op, st, t, name, dtype=F32):
    a = st.take(t, dtype)
    if not _shape3(a):
        raise H.invalid(f"{op} expects (b,n,c) {name} shape")
    b, n, c = a.shape
    if not (1 <= b <= 65535 and 1 <= n <= GC_MAX_POINTS and 1 <= c <= GP_MAX_CHANNELS):
        raise H.invalid(f"{op} takes 1 <= b <= 65535, 1 <= n <= {GC_MAX_POINTS} and 1 <= c <= {GP_MAX_CHANNELS}")
    return a


def _gp_index(op, st, t, name, shape):
    a = st.take(t, I32)
    if tuple(a.shape) != shape:
        raise H.invalid(f"{op} expects {name} of shape {shape}")
    return a


@H.on_input_device
def grid_pool(feat, order, starts, nclusters, reduce="mean"):
    """rf_grid_pool: feat (b,n,c) reduced per cluster of grid_cluster's order (b,n), starts (b,n+1) and nclusters (b,) ->
    out (b,n,c), rows behind the cluster count +0; reduce "sum" / "mean" (double sums, rounded once) or "max", which returns
    (out, arg (b,n,c) int32 the winning point index)."""
    op = "GridPool"
    st = H.Staged()
    f = _gp_rows(op, st, feat, "feat")
    b, n, c = f.shape
    if reduce not in GP_REDUCES:
        raise H.invalid(f"{op} takes reduce in {sorted(GP_REDUCES)}")
    od, ss = _gp_index(op, st, order, "order", (b, n)), _gp_index(op, st, starts, "starts", (b, n + 1))
    nc = _gp_index(op, st, nclusters, "nclusters", (b,))
    dev = st.device_()
    f, od, ss, nc = st.up(f, od, ss, nc)
    out = H.empty((b, n, c), F32, dev)
    arg = H.empty((b, n, c), I32, dev) if reduce == "max" else None
    check(lib.rf_grid_pool(b, n, c, GP_REDUCES[reduce], H.ptr(f), H.ptr(od), H.ptr(ss), H.ptr(nc), H.ptr(out), H.ptr(arg),
                           H.stream(dev)), "rf_grid_pool")
    return (st.give(out), st.give(arg)) if reduce == "max" else st.give(out)


@H.on_input_device
def grid_unpool(src, cluster, starts=None, arg=None, mode="copy"):
    """rf_grid_unpool: src (b,n,c) pooled rows back to the points -> (b,n,c): row i is row cluster[i] of src ("copy"), that row
    divided by the cluster's size from starts ("mean"), or its channels whose arg names point i ("max"); +0 where cluster[i] is
    -1.  The forward of an unpooling and the backward of grid_pool's three reductions."""
    op = "GridUnpool"
    st = H.Staged()
    s = _gp_rows(op, st, src, "src")
    b, n, c = s.shape
    if mode not in GU_MODES:
        raise H.invalid(f"{op} takes mode in {sorted(GU_MODES)}")
    cl = _gp_index(op, st, cluster, "cluster", (b, n))
    if mode == "mean" and starts is None:
        raise H.invalid(f"{op} needs starts for mode mean")
    if mode == "max" and arg is None:
        raise H.invalid(f"{op} needs arg for mode max")
    ss = _gp_index(op, st, starts, "starts", (b, n + 1)) if mode == "mean" else None
    ag = _gp_index(op, st, arg, "arg", (b, n, c)) if mode == "max" else None
    dev = st.device_()
    s, cl = st.up(s, cl)
    if ss is not None:
        ss, = st.up(ss)
    if ag is not None:
        ag, = st.up(ag)
    dst = H.empty((b, n, c), F32, dev)
    check(lib.rf_grid_unpool(b, n, c, GU_MODES[mode], H.ptr(s), H.ptr(cl), H.ptr(ss), H.ptr(ag), H.ptr(dst), H.stream(dev)),
          "rf_grid_unpool")
    return st.give(dst)


SC_MAX_CHANNELS, SC_MAX_DILATION, SC_WGRAD_ROWS = 256, 1024, 1024  # RF_SC_MAX_CHANNELS, RF_SC_MAX_DILATION, RF_SC_WGRAD_ROWS
SC_MODES = {"forward": 0, "grad_input": 1}  # RF_SC_FORWARD, RF_SC_GRAD_INPUT


def _sc_check_counts(x, b, n, name="nclusters"):
    """The cell counts of the sparse convolution entries -> None or a (b,) integer tensor, before any GPU work.  Unlike the
    point counts of the ragged entries a count may be 0 (a sample without a cell): host-given counts are checked into
    [0, n], device counts are only shape-checked (grid_cluster's nclusters: no host round trip; the kernels clamp them)."""
    if x is None:
        return None
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise H.invalid(f"{name} must hold integer cell counts")
    if t.dim() != 1 or t.shape[0] != b:
        raise H.invalid(f"{name} must be of shape (batch,)")
    if not t.is_cuda and (int(t.min()) < 0 or int(t.max()) > n):
        raise H.invalid(f"{name} must lie in [0, {n}]")
    return t


def _sc_counts_up(t, dev, n):
    """checked counts -> a contiguous int32 tensor on `dev` (a device int32 tensor stays as it is)"""
    if t is None:
        return None
    if t.is_cuda and t.device != dev:
        raise ValueError(f"all GPU inputs of one op must live on the same device: got {dev} and {t.device}")
    t = t.to(device=dev)
    if t.dtype != I32:
        t = t.clamp(0, n).to(I32)
    return t.contiguous()


def _sc_sizes(op, b, n, K=27, cin=1, cout=1):
    if not (1 <= b <= 65535 and 1 <= n <= GC_MAX_POINTS):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1 <= n <= {GC_MAX_POINTS} cells")
    if K not in (27, 125):
        raise H.invalid(f"{op} takes K = 27 or 125 slots (kernel_size 3 or 5)")
    if not (1 <= cin <= SC_MAX_CHANNELS and 1 <= cout <= SC_MAX_CHANNELS):
        raise H.invalid(f"{op} takes 1 to {SC_MAX_CHANNELS} channels")


@H.on_input_device
def sparse_conv_map(coords, nclusters=None, kernel_size=3, dilation=1):
    """rf_sparse_conv_map: coords (b,n,3) int32 cell indices (grid_cluster's "coords") and the cell counts nclusters (b,) ->
    nbr (b,n,K) int32, K = kernel_size^3: per live row the row of the cell at each of the K offsets, or -1 (include/rfops.h)."""
    op = "SparseConvMap"
    st = H.Staged()
    c = st.take(coords, I32)
    if not _shape3(c, 3):
        raise H.invalid(f"{op} expects (b,n,3) coords shape")
    b, n = c.shape[0], c.shape[1]
    _sc_sizes(op, b, n)
    ks, dilation = int(kernel_size), int(dilation)
    if ks not in (3, 5):
        raise H.invalid(f"{op} takes kernel_size 3 or 5")
    if not 1 <= dilation <= SC_MAX_DILATION:
        raise H.invalid(f"{op} takes 1 <= dilation <= {SC_MAX_DILATION}")
    cnt = _sc_check_counts(nclusters, b, n)
    dev = st.device_()
    c, = st.up(c)
    cnt = _sc_counts_up(cnt, dev, n)
    nbr = H.empty((b, n, ks ** 3), I32, dev)
    check(lib.rf_sparse_conv_map(b, n, ks, dilation, H.ptr(c), H.ptr(cnt), H.ptr(nbr), H.stream(dev)), "rf_sparse_conv_map")
    return st.give(nbr)


@H.on_input_device
def sparse_conv(feat, weight, nbr, nclusters=None, mode="forward"):
    """rf_sparse_conv: feat (b,n,cin), nbr (b,n,K) -> (b,n,cout).  mode "forward": weight (K,cin,cout); "grad_input": feat is
    grad_out, weight the forward's weight (K,cout,cin) and the result the gradient to the forward's features."""
    op = "SparseConv"
    st = H.Staged()
    f, w, nb = st.take(feat, F32), st.take(weight, F32), st.take(nbr, I32)
    if mode not in SC_MODES:
        raise H.invalid(f"{op} takes mode in {sorted(SC_MODES)}")
    if not _shape3(f):
        raise H.invalid(f"{op} expects (b,n,c) feat shape")
    b, n, cin = f.shape
    red = 1 if mode == "forward" else 2  # where weight holds this call's reduction width
    if not (_shape3(w) and w.shape[red] == cin):
        raise H.invalid(f"{op} expects (K,cin,cout) weight shape, and the channels must match feat")
    K, cout = w.shape[0], w.shape[3 - red]
    _sc_sizes(op, b, n, K, cin, cout)
    if tuple(nb.shape) != (b, n, K):
        raise H.invalid(f"{op} expects nbr of shape {(b, n, K)}")
    cnt = _sc_check_counts(nclusters, b, n)
    dev = st.device_()
    f, w, nb = st.up(f, w, nb)
    cnt = _sc_counts_up(cnt, dev, n)
    out = H.empty((b, n, cout), F32, dev)
    check(lib.rf_sparse_conv(b, n, K, cin, cout, SC_MODES[mode], H.ptr(f), H.ptr(w), H.ptr(nb), H.ptr(cnt), H.ptr(out),
                             H.stream(dev)), "rf_sparse_conv")
    return st.give(out)


@H.on_input_device
def sparse_conv_grad_weight(feat, grad_out, nbr, nclusters=None):
    """rf_sparse_conv_grad_weight: feat (b,n,cin), grad_out (b,n,cout), nbr (b,n,K) -> grad_weight (K,cin,cout): fmaf chains
    over chunks of 1024 rows, the chunks and the samples added in double, rounded once (include/rfops.h)."""
    op = "SparseConvGradWeight"
    st = H.Staged()
    f, g, nb = st.take(feat, F32), st.take(grad_out, F32), st.take(nbr, I32)
    if not _shape3(f):
        raise H.invalid(f"{op} expects (b,n,cin) feat shape")
    b, n, cin = f.shape
    if not (_shape3(g) and tuple(g.shape[:2]) == (b, n)):
        raise H.invalid(f"{op} expects (b,n,cout) grad_out shape")
    if not (nb.dim() == 3 and tuple(nb.shape[:2]) == (b, n)):
        raise H.invalid(f"{op} expects (b,n,K) nbr shape")
    cout, K = g.shape[2], nb.shape[2]
    _sc_sizes(op, b, n, K, cin, cout)
    cnt = _sc_check_counts(nclusters, b, n)
    dev = st.device_()
    f, g, nb = st.up(f, g, nb)
    cnt = _sc_counts_up(cnt, dev, n)
    gw = H.empty((K, cin, cout), F32, dev)
    ws, wsz = H.workspace(lib.rf_sparse_conv_grad_weight_workspace_bytes(b, K, cin, cout), dev, "sparse_conv_grad_weight")
    check(lib.rf_sparse_conv_grad_weight(b, n, K, cin, cout, H.ptr(f), H.ptr(g), H.ptr(nb), H.ptr(cnt), H.ptr(gw), H.ptr(ws), wsz,
                                         H.stream(dev)), "rf_sparse_conv_grad_weight")
    return st.give(gw)


SS_MODES = {"down": 0, "up": 1, "down_grad_input": 2, "up_grad_input": 3}  # RF_SS_DOWN ... RF_SS_UP_GRAD_INPUT


def _ss_sizes(op, b, n, nc, cin=1, cout=1):
    if not (1 <= b <= 65535 and 1 <= n <= GC_MAX_POINTS):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1 <= n <= {GC_MAX_POINTS} cells")
    if not 1 <= nc <= n:
        raise H.invalid(f"{op} takes 1 <= max_cells <= n coarse rows")
    if not (1 <= cin <= SC_MAX_CHANNELS and 1 <= cout <= SC_MAX_CHANNELS):
        raise H.invalid(f"{op} takes 1 to {SC_MAX_CHANNELS} channels")


@H.on_input_device
def sparse_stride_map(coords, nclusters=None, max_cells=None):
    """rf_sparse_stride_map: coords (b,n,3) int32 cell indices and the cell counts nclusters (b,) -> (coords_out (b,nc,3),
    count_out (b,), total_out (b,), child (b,nc,8), up (b,n)), all int32, nc = max_cells (default n): the level of the cells
    coords >> 1 (include/rfops.h)."""
    op = "SparseStrideMap"
    st = H.Staged()
    c = st.take(coords, I32)
    if not _shape3(c, 3):
        raise H.invalid(f"{op} expects (b,n,3) coords shape")
    b, n = c.shape[0], c.shape[1]
    nc = n if max_cells is None else int(max_cells)
    _ss_sizes(op, b, n, nc)
    cnt = _sc_check_counts(nclusters, b, n)
    dev = st.device_()
    c, = st.up(c)
    cnt = _sc_counts_up(cnt, dev, n)
    co, cn, tot = H.empty((b, nc, 3), I32, dev), H.empty((b,), I32, dev), H.empty((b,), I32, dev)
    child, up = H.empty((b, nc, 8), I32, dev), H.empty((b, n), I32, dev)
    check(lib.rf_sparse_stride_map(b, n, nc, H.ptr(c), H.ptr(cnt), H.ptr(co), H.ptr(cn), H.ptr(tot), H.ptr(child), H.ptr(up),
                                   H.stream(dev)), "rf_sparse_stride_map")
    return tuple(st.give(t) for t in (co, cn, tot, child, up))


def _ss_maps(op, st, child, up):
    ch, u = st.take(child, I32), st.take(up, I32)
    if not (ch.dim() == 3 and ch.shape[2] == 8 and u.dim() == 2 and u.shape[0] == ch.shape[0]):
        raise H.invalid(f"{op} expects child of shape (b,n_coarse,8) and up of shape (b,n)")
    return ch, u


@H.on_input_device
def sparse_conv_strided(src, weight, child, up, nclusters=None, nclusters_coarse=None, mode="down"):
    """rf_sparse_conv_strided: weight is the layer's (8,ci,co).  "down": src (b,n,ci) -> (b,nc,co); "up": src (b,nc,ci) ->
    (b,n,co); "down_grad_input": src the coarse grad_out (b,nc,co) -> (b,n,ci); "up_grad_input": src the fine grad_out (b,n,co) ->
    (b,nc,ci).  child (b,nc,8) and up (b,n) are `sparse_stride_map`'s, the counts those of the fine and of the coarse level."""
    op = "SparseConvStrided"
    st = H.Staged()
    f, w = st.take(src, F32), st.take(weight, F32)
    ch, u = _ss_maps(op, st, child, up)
    if mode not in SS_MODES:
        raise H.invalid(f"{op} takes mode in {sorted(SS_MODES)}")
    if not _shape3(f):
        raise H.invalid(f"{op} expects (b,rows,c) src shape")
    b, nc, n = ch.shape[0], ch.shape[1], u.shape[1]
    rows_in, rows_out = (n, nc) if mode in ("down", "up_grad_input") else (nc, n)
    if f.shape[0] != b or f.shape[1] != rows_in:
        raise H.invalid(f"{op} ({mode}) expects src of {rows_in} rows per sample, as child and up say")
    cin = f.shape[2]
    red = 1 if mode in ("down", "up") else 2  # where weight holds this call's reduction width
    if not (_shape3(w) and w.shape[0] == 8 and w.shape[red] == cin):
        raise H.invalid(f"{op} expects (8,ci,co) weight shape, and the channels must match src")
    cout = w.shape[3 - red]
    _ss_sizes(op, b, n, nc, cin, cout)
    cnt, cntc = _sc_check_counts(nclusters, b, n), _sc_check_counts(nclusters_coarse, b, nc, "nclusters_coarse")
    dev = st.device_()
    f, w, ch, u = st.up(f, w, ch, u)
    cnt, cntc = _sc_counts_up(cnt, dev, n), _sc_counts_up(cntc, dev, nc)
    out = H.empty((b, rows_out, cout), F32, dev)
    check(lib.rf_sparse_conv_strided(b, n, nc, cin, cout, SS_MODES[mode], H.ptr(f), H.ptr(w), H.ptr(ch), H.ptr(u), H.ptr(cnt),
                                     H.ptr(cntc), H.ptr(out), H.stream(dev)), "rf_sparse_conv_strided")
    return st.give(out)


@H.on_input_device
def sparse_conv_strided_grad_weight(fine, coarse, child, nclusters=None, nclusters_coarse=None, mode="down"):
    """rf_sparse_conv_strided_grad_weight -> (8,ci,co).  "down": fine is the forward's feat (b,n,ci), coarse grad_out (b,nc,co);
    "up": coarse is the forward's feat (b,nc,ci), fine grad_out (b,n,co).  fmaf chains over chunks of 1024 coarse rows, the
    chunks and the samples added in double, rounded once (include/rfops.h)."""
    op = "SparseConvStridedGradWeight"
    st = H.Staged()
    f, c, ch = st.take(fine, F32), st.take(coarse, F32), st.take(child, I32)
    if mode not in ("down", "up"):
        raise H.invalid(f"{op} takes mode 'down' or 'up'")
    if not (_shape3(f) and _shape3(c) and f.shape[0] == c.shape[0]):
        raise H.invalid(f"{op} expects (b,n,c) fine and (b,n_coarse,c) coarse shapes")
    b, n, nc = f.shape[0], f.shape[1], c.shape[1]
    if tuple(ch.shape) != (b, nc, 8):
        raise H.invalid(f"{op} expects child of shape {(b, nc, 8)}")
    cin, cout = (f.shape[2], c.shape[2]) if mode == "down" else (c.shape[2], f.shape[2])
    _ss_sizes(op, b, n, nc, cin, cout)
    cnt, cntc = _sc_check_counts(nclusters, b, n), _sc_check_counts(nclusters_coarse, b, nc, "nclusters_coarse")
    dev = st.device_()
    f, c, ch = st.up(f, c, ch)
    cnt, cntc = _sc_counts_up(cnt, dev, n), _sc_counts_up(cntc, dev, nc)
    gw = H.empty((8, cin, cout), F32, dev)
    ws, wsz = H.workspace(lib.rf_sparse_conv_strided_grad_weight_workspace_bytes(b, cin, cout), dev, "sparse_conv_strided_grad_weight")
    check(lib.rf_sparse_conv_strided_grad_weight(b, n, nc, cin, cout, SS_MODES[mode], H.ptr(f), H.ptr(c), H.ptr(ch), H.ptr(cnt),
                                                 H.ptr(cntc), H.ptr(gw), H.ptr(ws), wsz, H.stream(dev)),
          "rf_sparse_conv_strided_grad_weight")
    return st.give(gw)


def _sg_coords(op, st, t, name="coords"):
    c = st.take(t, I32)
    if not _shape3(c, 3):
        raise H.invalid(f"{op} expects (b,n,3) {name} shape")
    if not (1 <= c.shape[0] <= 65535 and 1 <= c.shape[1] <= GC_MAX_POINTS):
        raise H.invalid(f"{op} takes 1 <= b <= 65535 and 1 <= n <= {GC_MAX_POINTS} cells in {name}")
    return c


@H.on_input_device
def sparse_generate_map(coords, nclusters=None, max_cells=None):
    """rf_sparse_generate_map: coords (b,nc,3) int32 cells of the COARSE level and their counts nclusters (b,) -> (coords_out
    (b,nf,3), count_out (b,), total_out (b,), child (b,nc,8), up (b,nf)), all int32, nf = max_cells (default min(8 nc, 16384)):
    all eight children 2 c + bit of every live coarse row in [-16384, 16383], in row order (include/rfops.h)."""
    op = "SparseGenerateMap"
    st = H.Staged()
    c = _sg_coords(op, st, coords)
    b, nc = c.shape[0], c.shape[1]
    nf = min(8 * nc, GC_MAX_POINTS) if max_cells is None else int(max_cells)
    if not (8 <= nf <= GC_MAX_POINTS and nc <= nf):
        raise H.invalid(f"{op} takes max(8, n) <= max_cells <= {GC_MAX_POINTS} fine rows")
    cnt = _sc_check_counts(nclusters, b, nc)
    dev = st.device_()
    c, = st.up(c)
    cnt = _sc_counts_up(cnt, dev, nc)
    co, cn, tot = H.empty((b, nf, 3), I32, dev), H.empty((b,), I32, dev), H.empty((b,), I32, dev)
    child, up = H.empty((b, nc, 8), I32, dev), H.empty((b, nf), I32, dev)
    check(lib.rf_sparse_generate_map(b, nc, nf, H.ptr(c), H.ptr(cnt), H.ptr(co), H.ptr(cn), H.ptr(tot), H.ptr(child), H.ptr(up),
                                     H.stream(dev)), "rf_sparse_generate_map")
    return tuple(st.give(t) for t in (co, cn, tot, child, up))


@H.on_input_device
def sparse_prune_map(coords, keep, nclusters=None, max_cells=None):
    """rf_sparse_prune_map: coords (b,n,3) int32, keep (b,n) (bool / uint8 as they are, any other dtype as > 0) and the counts
    nclusters (b,) -> (coords_out (b,no,3), count_out (b,), total_out (b,), src (b,no), dst (b,n)), no = max_cells (default n):
    the selected rows in front, in their order (include/rfops.h)."""
    op = "SparsePruneMap"
    st = H.Staged()
    c = _sg_coords(op, st, coords)
    b, n = c.shape[0], c.shape[1]
    k = keep if isinstance(keep, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(keep)))
    if tuple(k.shape) != (b, n):
        raise H.invalid(f"{op} expects keep of shape {(b, n)}")
    if k.dtype not in (torch.bool, torch.uint8):
        k = k.detach() > 0
    k = st.take(k, torch.uint8)
    no = n if max_cells is None else int(max_cells)
    if not 1 <= no <= n:
        raise H.invalid(f"{op} takes 1 <= max_cells <= n rows")
    cnt = _sc_check_counts(nclusters, b, n)
    dev = st.device_()
    c, k = st.up(c, k)
    cnt = _sc_counts_up(cnt, dev, n)
    co, cn, tot = H.empty((b, no, 3), I32, dev), H.empty((b,), I32, dev), H.empty((b,), I32, dev)
    src, dst = H.empty((b, no), I32, dev), H.empty((b, n), I32, dev)
    check(lib.rf_sparse_prune_map(b, n, no, H.ptr(c), H.ptr(k), H.ptr(cnt), H.ptr(co), H.ptr(cn), H.ptr(tot), H.ptr(src), H.ptr(dst),
                                  H.stream(dev)), "rf_sparse_prune_map")
    return tuple(st.give(t) for t in (co, cn, tot, src, dst))


@H.on_input_device
def sparse_lookup(coords, table, nclusters=None, table_nclusters=None, shift=0):
    """rf_sparse_lookup: coords (b,n,3) and table (b,m,3) int32 with their counts -> idx (b,n) int32: the lowest usable row of
    table whose cell >> shift (the arithmetic shift) equals coords[i], or -1 (include/rfops.h)."""
    op = "SparseLookup"
    st = H.Staged()
    c, t = _sg_coords(op, st, coords), _sg_coords(op, st, table, "table")
    b, n, m = c.shape[0], c.shape[1], t.shape[1]
    if t.shape[0] != b:
        raise H.invalid(f"{op} expects coords and table of the same batch size")
    shift = int(shift)
    if not 0 <= shift <= 15:
        raise H.invalid(f"{op} takes 0 <= shift <= 15")
    cnt, tcnt = _sc_check_counts(nclusters, b, n), _sc_check_counts(table_nclusters, b, m, "table_nclusters")
    dev = st.device_()
    c, t = st.up(c, t)
    cnt, tcnt = _sc_counts_up(cnt, dev, n), _sc_counts_up(tcnt, dev, m)
    idx = H.empty((b, n), I32, dev)
    check(lib.rf_sparse_lookup(b, n, m, shift, H.ptr(c), H.ptr(cnt), H.ptr(t), H.ptr(tcnt), H.ptr(idx), H.stream(dev)),
          "rf_sparse_lookup")
    return st.give(idx)


@H.on_input_device
def sparse_take_rows(src, idx, nclusters=None):
    """rf_sparse_take_rows: src (b,n_src,c), idx (b,n_dst) int32 and the counts nclusters (b,) of the DESTINATION rows ->
    (b,n_dst,c): row r is a copy of row idx[r] of src where r is below the count and 0 <= idx[r] < n_src, +0 elsewhere."""
    op = "SparseTakeRows"
    st = H.Staged()
    s = _gp_rows(op, st, src, "src")
    b, ns, c = s.shape
    ix = st.take(idx, I32)
    if not (ix.dim() == 2 and ix.shape[0] == b and 1 <= ix.shape[1] <= GC_MAX_POINTS):
        raise H.invalid(f"{op} expects idx of shape (b,n_dst), 1 <= n_dst <= {GC_MAX_POINTS}")
    nd = ix.shape[1]
    cnt = _sc_check_counts(nclusters, b, nd)
    dev = st.device_()
    s, ix = st.up(s, ix)
    cnt = _sc_counts_up(cnt, dev, nd)
    dst = H.empty((b, nd, c), F32, dev)
    check(lib.rf_sparse_take_rows(b, ns, nd, c, H.ptr(s), H.ptr(ix), H.ptr(cnt), H.ptr(dst), H.stream(dev)), "rf_sparse_take_rows")
    return st.give(dst)


@H.on_input_device
def knn_point_grad(xyz1, xyz2, idx, grad_val, lengths1=None, lengths2=None):
    """The gradient of knn_point's val -> (grad_xyz1 (b,n,3), grad_xyz2 (b,m,3)) (rf_knn_grad).  lengths1 / lengths2: the counts
    of the ragged forward (rf_knn_grad_lengths): padded slots add nothing whatever they hold, padded rows are exactly 0."""
    st = H.Staged()
    ix, g = st.take(idx, I32), st.take(grad_val, F32)
    if ix.dim() != 3:
        raise H.invalid("KnnPointGrad expects (b,m,k) idx shape")
    a, q, b, n, m = _knn_inputs(st, xyz1, xyz2, int(ix.shape[2]), "KnnPointGrad")
    k = int(ix.shape[2])
    if tuple(ix.shape) != (b, m, k) or tuple(g.shape) != (b, m, k):
        raise H.invalid("KnnPointGrad expects (b,m,k) idx and grad_val shapes")
    l1, l2 = _check_lengths(lengths1, b, n, "lengths1"), _check_lengths(lengths2, b, m, "lengths2")
    dev = st.device_()
    a, q, ix, g = st.up(a, q, ix, g)
    g1, g2 = H.empty((b, n, 3), F32, dev), H.empty((b, m, 3), F32, dev)
    ws, wsz = H.workspace(lib.rf_knn_grad_workspace_bytes(b, n, m, k), dev, "knng")
    if l1 is not None or l2 is not None:
        l1, l2 = _lengths_up(l1, dev, n), _lengths_up(l2, dev, m)
        check(lib.rf_knn_grad_lengths(b, n, m, k, H.ptr(a), H.ptr(q), H.ptr(l1), H.ptr(l2), H.ptr(ix), H.ptr(g), H.ptr(g1),
                                      H.ptr(g2), H.ptr(ws), wsz, H.stream(dev)), "rf_knn_grad_lengths")
        return st.give(g1), st.give(g2)
    check(lib.rf_knn_grad(b, n, m, k, H.ptr(a), H.ptr(q), H.ptr(ix), H.ptr(g), H.ptr(g1), H.ptr(g2), H.ptr(ws), wsz,
                          H.stream(dev)), "rf_knn_grad")
    return st.give(g1), st.give(g2)


@H.on_input_device
def three_interpolate(points, idx, weight):
    """ThreeInterpolateOp, tf_interpolate.cpp:191-222 -> (b,n,c)."""
    st = H.Staged()
    p, ix, w = st.take(points, F32), st.take(idx, I32), st.take(weight, F32)
    if p.dim() != 3:
        raise H.invalid("ThreeInterpolate expects (b,m,c) points shape")
    b, m, c = p.shape
    if not (ix.dim() == 3 and ix.shape[0] == b and ix.shape[2] == 3):
        raise H.invalid("ThreeInterpolate expects (b,n,3) idx shape")
    n = ix.shape[1]
    if tuple(w.shape) != (b, n, 3):
        raise H.invalid("ThreeInterpolate expects (b,n,3) weight shape")
    dev = st.device_()
    p, ix, w = st.up(p, ix, w)
    out = H.empty((b, n, c), F32, dev)
    check(lib.rf_threeinterpolate(b, m, c, n, H.ptr(p), H.ptr(ix), H.ptr(w), H.ptr(out),
                                  H.stream(dev)), "rf_threeinterpolate")
    return st.give(out)


@H.on_input_device
def three_interpolate_grad(points, idx, weight, grad_out, form="auto"):
    """ThreeInterpolateGradOp, tf_interpolate.cpp:225-262 -> (b,m,c).
    form: "auto" (rf_threeinterpolate_grad_ws) | "inline" (rf_threeinterpolate_grad: the LDS tile, or atomics beyond it)."""
    st = H.Staged()
    p, ix, w, go = (st.take(points, F32), st.take(idx, I32), st.take(weight, F32),
                    st.take(grad_out, F32))
    if p.dim() != 3:
        raise H.invalid("ThreeInterpolateGrad expects (b,m,c) points shape")
    b, m, c = p.shape
    if not (ix.dim() == 3 and ix.shape[0] == b):
        raise H.invalid("ThreeInterpolateGrad expects (b,n,3) idx shape")
    n = ix.shape[1]
    if tuple(w.shape) != (b, n, 3):
        raise H.invalid("ThreeInterpolateGrad expects (b,n,3) weight shape")
    if tuple(go.shape) != (b, n, c):
        raise H.invalid("ThreeInterpolateGrad expects (b,n,c) grad_out shape")
    dev = st.device_()
    p, ix, w, go = st.up(p, ix, w, go)
    g = H.empty((b, m, c), F32, dev)
    if form == "inline":
        check(lib.rf_threeinterpolate_grad(b, n, c, m, H.ptr(go), H.ptr(ix), H.ptr(w), H.ptr(g),
                                           H.stream(dev)), "rf_threeinterpolate_grad")
        return st.give(g)
    ws, wsz = H.workspace(lib.rf_threeinterpolate_grad_workspace_bytes(b, n, c, m), dev, "tig")
    check(lib.rf_threeinterpolate_grad_ws(b, n, c, m, H.ptr(go), H.ptr(ix), H.ptr(w), H.ptr(g), H.ptr(ws), wsz,
                                          H.stream(dev)), "rf_threeinterpolate_grad_ws")
    return st.give(g)


# ------------------------------------------------------------------ import surface (f3) -----
@H.on_input_device
def auction_match(xyz1, xyz2):
    """AuctionMatchGpuOp, tf_ops/emd/tf_auctionmatch.cpp:27-58 -> matchl (b,n), matchr (b,n) int32."""
    st = H.Staged()
    a, b_ = st.take(xyz1, F32), st.take(xyz2, F32)
    if not _shape3(a, 3):
        raise H.invalid("ApproxMatch expects (batch_size,num_points,3) xyz1 shape")  # sic (reference wording)
    b, n = a.shape[0], a.shape[1]
    if n > 4096:
        raise H.invalid("AuctionMatch handles at most 4096 dataset points")
    if not (_shape3(b_, 3) and b_.shape[0] == b and b_.shape[1] == n):
        raise H.invalid("AuctionMatch expects (batch_size,num_points,3) xyz2 shape, and shape must match with xyz1")
    if n and not lib.rf_auctionmatch_supported(n):
        raise H.invalid("AuctionMatch is defined for n < 1024 or n in {1024, 2048, 4096}: for other n "
                        "the reference kernel reads out of bounds (tf_auctionmatch_g.cu:148,185)")
    dev = st.device_()
    a, b_ = st.up(a, b_)
    ml, mr = H.empty((b, n), I32, dev), H.empty((b, n), I32, dev)
    ws, wsz = H.workspace(lib.rf_auctionmatch_workspace_bytes(b, n), dev, "auction")
    check(lib.rf_auctionmatch(b, n, H.ptr(a), H.ptr(b_), H.ptr(ml), H.ptr(mr), H.ptr(ws), wsz,
                              H.stream(dev)), "rf_auctionmatch")
    return st.give(ml), st.give(mr)


@H.on_input_device
def select_top_k(k, dist):
    """SelectionSortGpuOp, tf_ops/grouping/tf_grouping.cpp:113-143 -> idx (b,m,n) int32, dist_out (b,m,n)."""
    k = int(k)
    if k <= 0:
        raise H.invalid("SelectionSort expects positive k")
    st = H.Staged()
    d = st.take(dist, F32)
    if d.dim() != 3:
        raise H.invalid("SelectionSort expects (b,m,n) dist shape.")
    b, m, n = d.shape
    if n > 16384:
        raise H.invalid("select_top_k handles rows of at most 16384 entries")
    dev = st.device_()
    d, = st.up(d)
    idx, out = H.empty((b, m, n), I32, dev), H.empty((b, m, n), F32, dev)
    check(lib.rf_selectionsort(b, n, m, k, H.ptr(d), H.ptr(idx), H.ptr(out), H.stream(dev)),
          "rf_selectionsort")
    return st.give(idx), st.give(out)


@H.on_input_device
def prob_sample(inp, inpr, return_cumsum=False):
    """ProbSampleGpuOp, tf_ops/sampling/tf_sampling.cpp:66-92 -> (b,m) int32 (and, on request, the
    op's temp tensor: the (b,n) cumulative sums)."""
    st = H.Staged()
    p, r = st.take(inp, F32), st.take(inpr, F32)
    if p.dim() != 2:
        raise H.invalid("ProbSample expects (batch_size,num_choices) inp shape")
    if not (r.dim() == 2 and r.shape[0] == p.shape[0]):
        raise H.invalid("ProbSample expects (batch_size,num_points) inpr shape")
    b, n, m = p.shape[0], p.shape[1], r.shape[1]
    dev = st.device_()
    p, r = st.up(p, r)
    temp, out = H.empty((b, n), F32, dev), H.empty((b, m), I32, dev)
    check(lib.rf_probsample(b, n, m, H.ptr(p), H.ptr(r), H.ptr(temp), H.ptr(out), H.stream(dev)),
          "rf_probsample")
    if return_cumsum:
        return st.give(out), st.give(temp)
    return st.give(out)


# ------------------------------------------------------------------ model graph helper (f2) --
_ACT = {None: 0, "none": 0, "relu": 1, "tanh": 2}


def point_affine(y, p, w, r, act="relu", out=None):
    """rf_point_affine: act(y + p @ w + r) in one pass.  y (b,n,c) or None, p (b,n,kp<=16) or None with
    w (kp,c), r (b,c) / (b,1,c) per sample or (c,) shared.  GPU tensors only (a model-graph helper,
    not one of the reference's ops)."""
    ref = y if y is not None else p
    b, n = ref.shape[0], ref.shape[1]
    c = r.shape[-1]
    kp = 0 if p is None else p.shape[-1]
    if not lib.rf_point_affine_supported(c, kp):
        raise H.invalid("point_affine: channels must be a multiple of 4 (<= 1024), narrow input <= 16 channels")
    dev = ref.device
    per_sample = r.dim() > 1 and r.shape[0] == b and r.numel() == b * c
    if not per_sample and r.numel() != c:
        raise H.invalid("point_affine: r must be (b,c), (b,1,c) or (c,)")
    y_ = None if y is None else y.contiguous()
    p_ = None if p is None else p.contiguous()
    w_ = None if p is None else w.contiguous()
    r_ = r.contiguous()
    if out is None:
        out = H.empty((b, n, c), F32, dev)
    with torch.cuda.device(dev):
        check(lib.rf_point_affine(b, n, c, H.ptr(y_), H.ptr(p_), kp, H.ptr(w_), H.ptr(r_), int(per_sample),
                                  _ACT[act], H.ptr(out), H.stream(dev)), "rf_point_affine")
    return out


def _maxpool_points(x, lengths, want_idx):
    """The four rf_maxpool_points* entries: `lengths` picks the ragged ones, want_idx the ones that also give positions."""
    b, n, c = x.shape
    ln = _check_lengths(lengths, b, n, "lengths")
    dev = x.device
    x_ = x.contiguous()
    out = H.empty((b, 1, c), F32, dev)
    idx = H.empty((b, c), I32, dev) if want_idx else None
    name = "rf_maxpool_points" + ("_idx" if want_idx else "") + ("_lengths" if ln is not None else "")
    with torch.cuda.device(dev):
        args = [b, n, c, H.ptr(x_)]
        if ln is not None:
            ln = _lengths_up(ln, dev, n)
            args.append(H.ptr(ln))
        args.append(H.ptr(out))
        if want_idx:
            args.append(H.ptr(idx))
        ws, wsz = H.workspace(getattr(lib, name + "_workspace_bytes")(b, n, c), dev, "maxpool")
        check(getattr(lib, name)(*args, H.ptr(ws), wsz, H.stream(dev)), name)
    return (out, idx) if want_idx else out


def maxpool_points_idx(x, lengths=None):
    """rf_maxpool_points_idx: max over the points axis of a (b, n, c) GPU tensor -> values (b, 1, c) and
    the point index of each maximum (b, c) int32 (lowest index among ties).  `lengths`: per-sample row counts of a
    ragged batch (rf_maxpool_points_idx_lengths): sample i pools x[i, :lengths[i]], idx < lengths[i]."""
    return _maxpool_points(x, lengths, True)


_ACT_GRAD = {None: 0, "none": 0, "relu": 1, "tanh": 2, "leaky_relu": 3}


def act_grad_colsum_supported(c):
    return c > 0 and c % 4 == 0 and c <= 1024


def act_grad_colsum(grad, out, act, inplace=False):
    """rf_act_grad_colsum: g = grad * act'(out) and sums[i,:] = sum_j g[i,j,:] for (b, n, c) GPU tensors,
    one pass.  `out` is the layer's OUTPUT (None with act None).  Returns (g (b,n,c), sums (b,c));
    with act None g is `grad` itself.  inplace: g overwrites grad."""
    b, n, c = grad.shape
    dev = grad.device
    a = _ACT_GRAD[act]
    grad_ = grad.contiguous()
    out_ = None if a == 0 else out.contiguous()
    g = grad_ if (a == 0 or inplace) else H.empty((b, n, c), F32, dev)
    sums = H.empty((b, c), F32, dev)
    with torch.cuda.device(dev):
        ws, wsz = H.workspace(lib.rf_act_grad_colsum_workspace_bytes(b, n, c), dev, "maxpool")
        check(lib.rf_act_grad_colsum(b, n, c, H.ptr(grad_), H.ptr(out_), a, H.ptr(g), H.ptr(sums), H.ptr(ws), wsz,
                                     H.stream(dev)), "rf_act_grad_colsum")
    return g, sums


def maxpool_points(x, lengths=None):
    """rf_maxpool_points: max over the points axis of a (b, n, c) GPU tensor -> (b, 1, c) (keepdim).  `lengths`:
    per-sample row counts of a ragged batch (rf_maxpool_points_lengths): sample i pools x[i, :lengths[i]]."""
    return _maxpool_points(x, lengths, False)
