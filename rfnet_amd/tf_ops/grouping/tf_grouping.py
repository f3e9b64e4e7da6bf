"""Ball query and grouping: drop-in for the reference module tf_ops/grouping/tf_grouping.py
(query_ball_point :8-20, group_point :33-41 + gradient :42-46, knn_point :48-73;
select_top_k :22-31)."""
import torch
from torch.autograd.function import once_differentiable

from ... import _raw


def query_ball_point(radius, nsample, xyz1, xyz2):
    '''
    Input:
        radius: float32, ball search radius
        nsample: int32, number of points selected in each ball region
        xyz1: (batch_size, ndataset, 3) float32 array, input points
        xyz2: (batch_size, npoint, 3) float32 array, query points
    Output:
        idx: (batch_size, npoint, nsample) int32 array, indices to input points
        pts_cnt: (batch_size, npoint) int32 array, number of unique points in each local region
    '''
    return _raw.query_ball_point(radius, nsample, xyz1, xyz2)


def query_ball_point_lengths(radius, nsample, xyz1, xyz2, lengths1=None, lengths2=None, form="auto"):
    '''
    query_ball_point over a ragged batch (the reference's signature above is kept as it is: this is the extension).
    lengths1 / lengths2: (batch_size) int -- points per dataset, queries per sample (lists, numpy arrays or tensors; on the
    device: no host synchronisation; None = all).  Rows of queries behind lengths2[i] are idx 0, pts_cnt 0 (as are empty
    balls); the padding of xyz1 is in no ball.  form: "auto", "scan", "boxes" (same results).
    '''
    return _raw.query_ball_point(radius, nsample, xyz1, xyz2, form=form, lengths1=lengths1, lengths2=lengths2)


class _GroupPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        ctx.save_for_backward(points, idx)
        return _raw.group_point(points, idx)

    @staticmethod
    def backward(ctx, grad_out):
        points, idx = ctx.saved_tensors
        return _raw.group_point_grad(points, idx, grad_out.contiguous()), None


def group_point(points, idx):
    '''
    Input:
        points: (batch_size, ndataset, channel) float32 array, points to sample from
        idx: (batch_size, npoint, nsample) int32 array, indices to points
    Output:
        out: (batch_size, npoint, nsample, channel) float32 array, values sampled from points
    Ragged batches: the zero-filled rows that query_ball_point_lengths writes for padded queries are in range -- they
    gather point 0 (and the gradient adds there); pts_cnt and the counts say which rows mean something.
    '''
    if isinstance(points, torch.Tensor) and isinstance(idx, torch.Tensor) and points.requires_grad:
        return _GroupPoint.apply(points, idx)
    return _raw.group_point(points, idx)


def group_point_grad(points, idx, grad_out):
    """The reference's GroupPointGrad op (tf_grouping.cpp:56-64)."""
    return _raw.group_point_grad(points, idx, grad_out)


def _knn_on_gpu(k, xyz1, xyz2):
    if not (isinstance(xyz1, torch.Tensor) and isinstance(xyz2, torch.Tensor)):
        return False
    if not (xyz1.is_cuda and xyz2.is_cuda and xyz1.device == xyz2.device):
        return False
    if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32 or xyz1.dim() != 3 or xyz2.dim() != 3:
        return False
    if xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        return False
    return _raw.knn_supported(int(k), xyz1.shape[0], xyz1.shape[1], xyz2.shape[1])


class _KnnPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, xyz1, xyz2, form="auto", lengths1=None, lengths2=None):
        val, idx = _raw.knn_point(k, xyz1, xyz2, form=form, lengths1=lengths1, lengths2=lengths2)
        ctx.save_for_backward(xyz1, xyz2, idx)
        ctx.lengths = (lengths1, lengths2)  # (integer counts: kept for the backward as they came)
        ctx.mark_non_differentiable(idx)
        return val, idx

    @staticmethod
    @once_differentiable  # (the HIP gradient has no gradient of its own: no double backward on this path)
    def backward(ctx, grad_val, grad_idx):
        xyz1, xyz2, idx = ctx.saved_tensors
        if grad_val is None:
            return None, None, None, None, None, None
        l1, l2 = ctx.lengths
        g1, g2 = _raw.knn_point_grad(xyz1, xyz2, idx, grad_val.contiguous(), lengths1=l1, lengths2=l2)
        return None, g1 if ctx.needs_input_grad[1] else None, g2 if ctx.needs_input_grad[2] else None, None, None, None


def knn_point(k, xyz1, xyz2, lengths1=None, lengths2=None, form="auto"):
    '''
    Input:
        k: int32, number of k in k-nn search
        xyz1: (batch_size, ndataset, c) float32 array, input points
        xyz2: (batch_size, npoint, c) float32 array, query points
    Output:
        val: (batch_size, npoint, k) float32 array, NEGATED squared L2 distances (top_k of -dist)
        idx: (batch_size, npoint, k) int32 array, indices to input points
    Pure tensor ops in the reference (tf.nn.top_k of -dist, tf_grouping.py:64-73).  CUDA float32 tensors on one device with
    c = 3, 1 <= k <= min(n, 64) and b, n, m within the C ABI's limits go to the HIP kernels (rf_knn / rf_knn_boxes, no
    (b, m, n) tensor; ties to the lower index, tf.nn.top_k's rule), with the gradient to both inputs (rf_knn_grad, first order
    only: no double backward there); everything else is the tensor expression below.  val is the unfused fp32 distance
    ((dx*dx)+(dy*dy))+(dz*dz), which can differ from the expression's CUDA reduction in the last bits.
    Ragged batches: lengths1 / lengths2 (batch_size) -- candidates / queries per sample -- on the HIP path only (the tensor
    expression raises for them): rows of padded queries are zeros, a sample with fewer candidates than k gets its lengths1[i]
    neighbours and zeros behind, and the gradient ignores every padded slot.
    '''
    ragged = lengths1 is not None or lengths2 is not None
    if _knn_on_gpu(k, xyz1, xyz2):
        if xyz1.requires_grad or xyz2.requires_grad:
            return _KnnPoint.apply(int(k), xyz1, xyz2, form, lengths1, lengths2)
        return _raw.knn_point(int(k), xyz1, xyz2, form=form, lengths1=lengths1, lengths2=lengths2)
    if ragged:
        raise ValueError("knn_point: lengths need the HIP path (CUDA float32 (b,n,3) / (b,m,3) tensors on one device, "
                         "1 <= k <= min(n, 64)); the tensor expression does not take them")
    xyz1 = torch.as_tensor(xyz1)
    xyz2 = torch.as_tensor(xyz2)
    dist = ((xyz1.unsqueeze(1) - xyz2.unsqueeze(2)) ** 2).sum(-1)
    val, idx = torch.topk(-dist, k=int(k), dim=-1)
    return val, idx.to(torch.int32)


def select_top_k(k, dist):
    '''
    Input:
        k: int32, number of k SMALLEST elements selected
        dist: (b,m,n) float32 array, distance matrix, m query points, n dataset points
    Output:
        idx: (b,m,n) int32 array, first k in n are indices to the top k
        dist_out: (b,m,n) float32 array, first k in n are the top k
    '''
    return _raw.select_top_k(k, dist)
