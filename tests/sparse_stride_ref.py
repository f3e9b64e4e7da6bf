"""A numpy restatement of the strided sparse convolution contract of include/rfops.h (rf_sparse_stride_map,
rf_sparse_conv_strided, rf_sparse_conv_strided_grad_weight): the level map by np.unique over the coarse keys of the live rows,
the four modes as the prescribed fp32 fmaf chains on `fma32`, the weight gradient with its chunks of 1024 coarse rows and its
double sums.  `fma32`, `counts`, `live_rows` and `same_bits` are those of tests/sparse_conv_ref.py (imported, not copied).
tests/test_sparse_stride_host.py holds it to independent routes on the CPU, the GPU tests hold the kernels to it bit for bit
(zeros of either sign equal, NaNs as a class).  Not a test module itself."""
import numpy as np

from sparse_conv_ref import F32, F64, I32, I64, MAX_CHANNELS, MAX_POINTS, WGRAD_ROWS, counts, live_rows, same_bits  # noqa: F401
from test_knn_feature_host import fma32

DOWN, UP, DOWN_GRAD_INPUT, UP_GRAD_INPUT = 0, 1, 2, 3


def map_ref(coords, count=None, n_coarse=None):
    """-> dict(coords (b, nc, 3), count (b,), total (b,), child (b, nc, 8), up (b, n)), all int32"""
    coords = np.asarray(coords)
    b, n, _ = coords.shape
    nc = n if n_coarse is None else int(n_coarse)
    out = dict(coords=np.zeros((b, nc, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               child=np.full((b, nc, 8), -1, I32), up=np.full((b, n), -1, I32))
    live = live_rows(coords, count)
    for s in range(b):
        rows = np.nonzero(live[s])[0]
        if not len(rows):
            continue
        c = coords[s, rows].astype(I64)
        cc, t = c >> 1, (c[:, 0] & 1) * 4 + (c[:, 1] & 1) * 2 + (c[:, 2] & 1)  # (>> of a negative int64 is the floor)
        key = (cc[:, 0] + 16384) << 30 | (cc[:, 1] + 16384) << 15 | (cc[:, 2] + 16384)
        cells, first, rank = np.unique(key, return_index=True, return_inverse=True)  # ascending row-major
        D = len(cells)
        out["total"][s], out["count"][s] = D, min(D, nc)
        out["coords"][s, :min(D, nc)] = cc[first][:nc]
        kept = rank < nc
        out["child"][s, rank[kept], t[kept]] = rows[kept]
        out["up"][s, rows[kept]] = 8 * rank[kept] + t[kept]
    return out


def _gather(src, weight, child, M, Mc):
    """out[j][o], j < Mc: t ascending, i = child[j][t] in [0, M); ch ascending of src[i][ch] weight[t][ch][o]; +0 behind Mc"""
    b, n, cin = src.shape
    nc, cout = child.shape[1], weight.shape[2]
    flat = src.reshape(b * n, cin)
    acc = np.zeros((b * nc, cout), F32)
    row = np.arange(nc)[None, :]
    for t in range(8):
        i = child[:, :, t].astype(I64)
        use = ((row < Mc[:, None]) & (i >= 0) & (i < M[:, None])).reshape(-1)
        if not use.any():
            continue
        at = (i + np.arange(b)[:, None] * n).reshape(-1)[use]
        for ch in range(cin):
            acc[use] = fma32(flat[at, ch][:, None], weight[t, ch][None, :], acc[use])
    return acc.reshape(b, nc, cout)


def served_rows(child, up, M, Mc):
    """-> (sample, fine row, coarse row, slot) of the served fine rows: i < M, up[i] = 8 j + t, 0 <= j < Mc, child[j][t] == i"""
    b, n = up.shape
    u = up.astype(I64)
    j, t = u >> 3, u & 7
    ok = (np.arange(n)[None, :] < M[:, None]) & (u >= 0) & (j < Mc[:, None])
    s_i, i_i = np.nonzero(ok)
    hit = child[s_i, j[s_i, i_i], t[s_i, i_i]] == i_i
    s_i, i_i = s_i[hit], i_i[hit]
    return s_i, i_i, j[s_i, i_i], t[s_i, i_i]


def _fan(src, weight, child, up, M, Mc):
    """out[i][o] of a served fine row: ch ascending of src[j][ch] weight[t][ch][o]; every other row +0"""
    b, nc, cin = src.shape
    n, cout = up.shape[1], weight.shape[2]
    out = np.zeros((b, n, cout), F32)
    s_i, i_i, j_i, t_i = served_rows(child, up, M, Mc)
    acc = np.zeros((len(s_i), cout), F32)
    for ch in range(cin):
        acc = fma32(src[s_i, j_i, ch][:, None], weight[t_i, ch], acc)
    out[s_i, i_i] = acc
    return out


def conv_ref(mode, src, weight, child, up, n, count=None, count_coarse=None):
    """rf_sparse_conv_strided: weight is the layer's (8, ci, co); n is the fine level's row count"""
    src, weight = np.asarray(src, F32), np.asarray(weight, F32)
    child, up = np.asarray(child), np.asarray(up)
    b, nc = child.shape[:2]
    M, Mc = counts(count, b, n), counts(count_coarse, b, nc)
    if mode in (DOWN_GRAD_INPUT, UP_GRAD_INPUT):
        weight = np.ascontiguousarray(weight.transpose(0, 2, 1))  # weight[t][o][ch] where weight[t][ch][o] stands
    assert src.shape[1] == (n if mode in (DOWN, UP_GRAD_INPUT) else nc) and weight.shape[1] == src.shape[2]
    if mode in (DOWN, UP_GRAD_INPUT):
        return _gather(src, weight, child, M, Mc)
    return _fan(src, weight, child, up, M, Mc)


def grad_weight_ref(mode, fine, coarse, child, count=None, count_coarse=None):
    """rf_sparse_conv_strided_grad_weight -> (8, cin, cout): per sample and chunk of 1024 coarse rows an fmaf chain from +0 over
    the rows ascending, the chunks added in double, the samples added in double, rounded once.  DOWN: fine (b, n, cin), coarse
    (b, nc, cout); UP: coarse (b, nc, cin), fine (b, n, cout)."""
    fine, coarse, child = np.asarray(fine, F32), np.asarray(coarse, F32), np.asarray(child)
    b, n = fine.shape[:2]
    nc = coarse.shape[1]
    cin, cout = (fine.shape[2], coarse.shape[2]) if mode == DOWN else (coarse.shape[2], fine.shape[2])
    M, Mc = counts(count, b, n), counts(count_coarse, b, nc)
    i_all = child.astype(I64)
    use_all = (np.arange(nc)[None, :, None] < Mc[:, None, None]) & (i_all >= 0) & (i_all < M[:, None, None])
    ts = np.nonzero(use_all.any((0, 1)))[0]  # the slots anybody has: the others stay +0
    total = np.zeros((b, 8, cin, cout), F64)
    acc = np.zeros((b, len(ts), cin, cout), F32)
    bs = np.arange(b)[:, None]
    for j in range(int(Mc.max()) if b else 0):
        use = use_all[:, j][:, ts]  # (b, slots)
        if use.any():
            f = fine[bs, np.where(use, i_all[:, j][:, ts], 0)]  # (b, slots, c of the fine operand)
            if mode == DOWN:
                step = fma32(f[:, :, :, None], coarse[:, j][:, None, None, :], acc)
            else:
                step = fma32(coarse[:, j][:, None, :, None], f[:, :, None, :], acc)
            acc = np.where(use[:, :, None, None], step, acc)
        if (j + 1) % WGRAD_ROWS == 0:
            total[:, ts] += acc.astype(F64)
            acc = np.zeros_like(acc)
    total[:, ts] += acc.astype(F64)
    out = np.zeros((8, cin, cout), F64)
    for s in range(b):
        out = out + total[s]
    return out.astype(F32)
