"""3-nearest-neighbour interpolation: drop-in for the reference module
tf_ops/interpolation/tf_interpolate.py (three_nn :8-17, three_interpolate :19-28 + gradient
:29-34).  CPU-only ops in the reference; HIP kernels here."""
import torch

from ... import _raw


def three_nn(xyz1, xyz2, lengths1=None, lengths2=None, form="auto"):
    '''
    Input:
        xyz1: (b,n,3) float32 array, unknown points
        xyz2: (b,m,3) float32 array, known points
    Output:
        dist: (b,n,3) float32 array, SQUARED distances to the 3 nearest known points
        idx: (b,n,3) int32 array, indices to known points
    Ragged batches: lengths1 / lengths2 (b) -- unknown / known points per sample (lists, numpy arrays or tensors; on the device:
    no host synchronisation).  Rows behind lengths1[i] are zeros; the padding of xyz2 is nobody's neighbour.
    '''
    if lengths1 is None and lengths2 is None:
        return _raw.three_nn(xyz1, xyz2, form=form)
    return _raw.three_nn(xyz1, xyz2, form=form, lengths1=lengths1, lengths2=lengths2)


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, weight):
        ctx.save_for_backward(points, idx, weight)
        return _raw.three_interpolate(points, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        points, idx, weight = ctx.saved_tensors
        return _raw.three_interpolate_grad(points, idx, weight, grad_out.contiguous()), None, None


def three_interpolate(points, idx, weight):
    '''
    Input:
        points: (b,m,c) float32 array, known points
        idx: (b,n,3) int32 array, indices to known points
        weight: (b,n,3) float32 array, weights on known points
    Output:
        out: (b,n,c) float32 array, interpolated point values
    Ragged batches: the zero-filled rows that three_nn(..., lengths1=) leaves for padded unknown points are in range -- they read
    known point 0 with whatever weights the caller formed there; the counts say which rows mean something.
    '''
    if all(isinstance(t, torch.Tensor) for t in (points, idx, weight)) and points.requires_grad:
        return _ThreeInterpolate.apply(points, idx, weight)
    return _raw.three_interpolate(points, idx, weight)


def three_interpolate_grad(points, idx, weight, grad_out):
    """The reference's ThreeInterpolateGrad op (tf_interpolate.cpp:34-46)."""
    return _raw.three_interpolate_grad(points, idx, weight, grad_out)
