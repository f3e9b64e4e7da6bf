"""A numpy restatement of the submanifold sparse convolution contract of include/rfops.h (rf_sparse_conv_map, rf_sparse_conv,
rf_sparse_conv_grad_weight): the kernel map by sorted keys and np.searchsorted, the convolution and both gradients as the
prescribed fp32 fmaf chains on `fma32` (the exact fused multiply-add of tests/test_knn_feature_host.py, imported, not copied),
the weight gradient with its chunks of 1024 rows and its double sums.  tests/test_sparse_conv_host.py holds it to independent
routes on the CPU, the GPU tests hold the kernels to it bit for bit (zeros of either sign equal, NaNs as a class).  Not a test
module itself."""
import numpy as np

from test_knn_feature_host import fma32

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
MAX_POINTS, MAX_CHANNELS, MAX_DILATION, WGRAD_ROWS = 16384, 256, 1024, 1024
LO, HI = -32768, 32767


def offsets(ks=3, dilation=1):
    """(K, 3): slot t = ((dx + r) ks + (dy + r)) ks + (dz + r) -> dilation (dx, dy, dz)"""
    r = ks // 2
    d = np.arange(-r, r + 1)
    return np.stack(np.meshgrid(d, d, d, indexing="ij"), -1).reshape(-1, 3).astype(I64) * dilation


def counts(count, b, n):
    return np.full(b, n, I64) if count is None else np.clip(np.asarray(count, I64), 0, n)


def _key(c):
    return (c[..., 0] + 32768) << 32 | (c[..., 1] + 32768) << 16 | (c[..., 2] + 32768)


def live_rows(coords, count=None):
    """(b, n) bool: below the count, in range, and no row of lower index with the same coordinates"""
    coords = np.asarray(coords)
    b, n, _ = coords.shape
    live = np.zeros((b, n), bool)
    for s, M in enumerate(counts(count, b, n)):
        c = coords[s, :M].astype(I64)
        ok = ((c >= LO) & (c <= HI)).all(1)
        _, first = np.unique(_key(c[ok]), return_index=True)
        live[s, np.nonzero(ok)[0][first]] = True
    return live


def map_ref(coords, count=None, ks=3, dilation=1):
    """-> nbr (b, n, K) int32"""
    coords = np.asarray(coords)
    b, n, _ = coords.shape
    off = offsets(ks, dilation)
    nbr = np.full((b, n, len(off)), -1, I32)
    live = live_rows(coords, count)
    for s in range(b):
        rows = np.nonzero(live[s])[0]
        if not len(rows):
            continue
        c = coords[s, rows].astype(I64)
        order = np.argsort(_key(c), kind="stable")
        keys, by_key = _key(c)[order], rows[order]  # distinct, ascending
        tgt = c[:, None, :] + off[None]
        ok = ((tgt >= LO) & (tgt <= HI)).all(2)
        want = np.where(ok, _key(np.clip(tgt, LO, HI)), -1)
        pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
        nbr[s, rows] = np.where(ok & (keys[pos] == want), by_key[pos], -1)
    return nbr


def conv_ref(feat, weight, nbr, count=None):
    """rf_sparse_conv, RF_SC_FORWARD: feat (b, n, cin), weight (K, cin, cout), nbr (b, n, K) -> (b, n, cout).  Absent slots are
    skipped; the samples' rows run side by side (the chain of a row does not know the others)."""
    feat, weight, nbr = np.asarray(feat, F32), np.asarray(weight, F32), np.asarray(nbr)
    b, n, cin = feat.shape
    K, _, cout = weight.shape
    M = counts(count, b, n)[:, None]
    row = np.arange(n)[None, :]
    flat = feat.reshape(b * n, cin)
    acc = np.zeros((b * n, cout), F32)
    for t in range(K):
        j = nbr[:, :, t].astype(I64)
        use = ((row < M) & (j >= 0) & (j < M)).reshape(-1)
        if not use.any():
            continue
        src = (j + np.arange(b)[:, None] * n).reshape(-1)[use]
        for ch in range(cin):
            acc[use] = fma32(flat[src, ch][:, None], weight[t, ch][None, :], acc[use])
    return acc.reshape(b, n, cout)


def grad_input_ref(grad_out, weight, nbr, count=None):
    """rf_sparse_conv, RF_SC_GRAD_INPUT: grad_out (b, n, cout), the forward's weight (K, cin, cout) -> grad_feat (b, n, cin): the
    forward chain with weight[K-1-t][o][ch] in place of weight[t][ch][o]"""
    return conv_ref(grad_out, np.ascontiguousarray(np.asarray(weight, F32)[::-1].transpose(0, 2, 1)), nbr, count)


def grad_weight_ref(feat, grad_out, nbr, count=None):
    """rf_sparse_conv_grad_weight -> (K, cin, cout): per sample and chunk of 1024 rows an fmaf chain from +0 over the rows
    ascending, the chunks added in double, the samples added in double, rounded once"""
    feat, grad_out, nbr = np.asarray(feat, F32), np.asarray(grad_out, F32), np.asarray(nbr)
    b, n, cin = feat.shape
    cout, K = grad_out.shape[2], nbr.shape[2]
    M = counts(count, b, n)
    j_all = nbr.astype(I64)
    use_all = (np.arange(n)[None, :, None] < M[:, None, None]) & (j_all >= 0) & (j_all < M[:, None, None])
    ts = np.nonzero(use_all.any((0, 1)))[0]  # the slots anybody has: the others stay +0
    total = np.zeros((b, K, cin, cout), F64)
    acc = np.zeros((b, len(ts), cin, cout), F32)
    bs = np.arange(b)[:, None]
    for i in range(int(M.max()) if b else 0):
        use = use_all[:, i][:, ts]  # (b, slots)
        if use.any():
            f = feat[bs, np.where(use, j_all[:, i][:, ts], 0)]  # (b, slots, cin)
            step = fma32(f[:, :, :, None], grad_out[:, i][:, None, None, :], acc)
            acc = np.where(use[:, :, None, None], step, acc)
        if (i + 1) % WGRAD_ROWS == 0:
            total[:, ts] += acc.astype(F64)
            acc = np.zeros_like(acc)
    total[:, ts] += acc.astype(F64)
    out = np.zeros((K, cin, cout), F64)
    for s in range(b):
        out = out + total[s]
    return out.astype(F32)


def same_bits(got, want):
    """equal as fp32 with zeros of either sign equal and NaNs as a class"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
