"""A numpy restatement of the grid pooling contract of include/rfops.h (rf_grid_cluster, rf_grid_pool, rf_grid_unpool): the
keys of the three orders (the Hilbert loop over the bit planes, vectorised over the points; encode AND decode), the sort, every
output, the three reductions with their prescribed order of operations, and the unpooling.  A plain module (no tests, no
fixtures): tests/test_grid_pool_host.py holds it to independent routes on the CPU, the GPU tests hold the kernels to it as
bytes."""
import numpy as np

F32, F64, I32, I64, U64 = np.float32, np.float64, np.int32, np.int64, np.uint64
MAX_POINTS, MAX_CHANNELS, BITS = 16384, 2048, 16
ORDERS = ("xyz", "z", "hilbert")


# ---- keys -------------------------------------------------------------------------------------------------------------------
def _u(v):
    return np.asarray(v).astype(U64)


def interleave(x, y, z, bits=BITS):
    """bit 3j+2 = bit j of x, 3j+1 of y, 3j of z"""
    x, y, z = _u(x), _u(y), _u(z)
    out = np.zeros(x.shape, U64)
    for j in range(bits):
        sj, one = U64(j), U64(1)
        out |= ((x >> sj) & one) << U64(3 * j + 2) | ((y >> sj) & one) << U64(3 * j + 1) | ((z >> sj) & one) << U64(3 * j)
    return out


def deinterleave(code, bits=BITS):
    code = _u(code)
    x, y, z = (np.zeros(code.shape, U64) for _ in range(3))
    for j in range(bits):
        sj, one = U64(j), U64(1)
        x |= ((code >> U64(3 * j + 2)) & one) << sj
        y |= ((code >> U64(3 * j + 1)) & one) << sj
        z |= ((code >> U64(3 * j)) & one) << sj
    return x, y, z


def morton(x, y, z, bits=BITS):
    return interleave(x, y, z, bits)


def hilbert_encode(x, y, z, bits=BITS):
    """Skilling's axes-to-transpose with X[0] = x, then the interleave of the Morton key."""
    X = [_u(x).copy(), _u(y).copy(), _u(z).copy()]
    q = 1 << (bits - 1)
    while q > 1:
        Q, P = U64(q), U64(q - 1)
        for i in range(3):
            hit = (X[i] & Q) != 0
            if i == 0:
                X[0] = np.where(hit, X[0] ^ P, X[0])
            else:
                t = (X[0] ^ X[i]) & P
                X[0], X[i] = np.where(hit, X[0] ^ P, X[0] ^ t), np.where(hit, X[i], X[i] ^ t)
        q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros(X[0].shape, U64)
    q = 1 << (bits - 1)
    while q > 1:
        t = np.where((X[2] & U64(q)) != 0, t ^ U64(q - 1), t)
        q >>= 1
    return interleave(X[0] ^ t, X[1] ^ t, X[2] ^ t, bits)


def hilbert_decode(code, bits=BITS):
    """Skilling's transpose-to-axes: the inverse of hilbert_encode -> (x, y, z)."""
    X = list(deinterleave(code, bits))
    t = X[2] >> U64(1)
    X[2] = X[2] ^ X[1]
    X[1] = X[1] ^ X[0]
    X[0] = X[0] ^ t
    q = 2
    while q != (1 << bits):
        Q, P = U64(q), U64(q - 1)
        for i in (2, 1, 0):
            hit = (X[i] & Q) != 0
            if i == 0:
                X[0] = np.where(hit, X[0] ^ P, X[0])
            else:
                t = (X[0] ^ X[i]) & P
                X[0], X[i] = np.where(hit, X[0] ^ P, X[0] ^ t), np.where(hit, X[i], X[i] ^ t)
        q <<= 1
    return X[0], X[1], X[2]


def key_of(u, order, bits=BITS):
    """u (.., 3) unsigned cell indices -> the key along `order`"""
    x, y, z = _u(u[..., 0]), _u(u[..., 1]), _u(u[..., 2])
    if order == "xyz":
        return x << U64(2 * bits) | y << U64(bits) | z
    return morton(x, y, z, bits) if order == "z" else hilbert_encode(x, y, z, bits)


# ---- rf_grid_cluster ----------------------------------------------------------------------------------------------------------
def counts_of(lengths, b, n):
    return np.full(b, n, I64) if lengths is None else np.clip(np.asarray(lengths, I64), 1, n)


def cells_of(xyz, cell, origin, L):
    """one sample: -> (inside (n,) bool, k (n, 3) int64, zeros where not inside)"""
    n = xyz.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (xyz.astype(F64) - origin.astype(F64)[None]) / F64(F32(cell))
        usable = np.isfinite(xyz).all(1) & (np.arange(n) < L)
        inside = usable & ((t >= -32768.0) & (t < 32768.0)).all(1)
        k = np.where(inside[:, None], np.floor(np.where(inside[:, None], t, 0.0)), 0.0).astype(I64)
    return inside, k


def origin_of(xyz, L):
    usable = np.isfinite(xyz).all(1) & (np.arange(xyz.shape[0]) < L)
    if not usable.any():
        return np.zeros(3, F32)
    return (xyz[usable].min(0) + F32(0.0)).astype(F32)  # (-0 + +0 = +0)


def cluster_ref(xyz, cell, order="xyz", lengths=None, origin=None):
    """-> dict of the outputs of rf_grid_cluster ("order" is point_order), "code" included"""
    xyz = np.asarray(xyz, F32)
    b, n, _ = xyz.shape
    Ls = counts_of(lengths, b, n)
    r = dict(origin=np.zeros((b, 3), F32), inside=np.zeros(b, I32), nclusters=np.zeros(b, I32), order=np.zeros((b, n), I32),
             starts=np.zeros((b, n + 1), I32), cluster=np.full((b, n), -1, I32), coords=np.zeros((b, n, 3), I32),
             code=np.full((b, n), -1, I64))
    for s in range(b):
        o = origin_of(xyz[s], Ls[s]) if origin is None else np.asarray(origin, F32)[s]
        r["origin"][s] = o
        inside, k = cells_of(xyz[s], cell, o, Ls[s])
        idx = np.nonzero(inside)[0]
        key = key_of(k[idx] + 32768, order)
        words = np.sort(key << U64(16) | idx.astype(U64))
        pts, skey = (words & U64(0xFFFF)).astype(I64), words >> U64(16)
        I = len(idx)
        head = np.ones(I, bool)
        head[1:] = skey[1:] != skey[:-1]
        rank = np.cumsum(head) - 1
        M = int(head.sum())
        r["inside"][s], r["nclusters"][s] = I, M
        r["order"][s, :I] = pts
        r["starts"][s, :M] = np.nonzero(head)[0]
        r["starts"][s, M:] = I
        r["cluster"][s, pts] = rank
        r["coords"][s, :M] = k[pts[head]]
        r["code"][s, pts] = skey.astype(I64)
    return r


# ---- rf_grid_pool ------------------------------------------------------------------------------------------------------------
def pool_ref(feat, order, starts, nclusters, reduce):
    """-> out (b, n, c) fp32, and arg (b, n, c) int32 for "max": every cluster's members one after the other (vectorised over
    the clusters, not over a cluster's members: the order of the operations is the contract)"""
    feat = np.asarray(feat, F32)
    b, n, c = feat.shape
    out, arg = np.zeros((b, n, c), F32), np.zeros((b, n, c), I32)
    for s in range(b):
        M = int(nclusters[s])
        if M == 0:
            continue
        beg, size = starts[s, :M].astype(I64), (starts[s, 1:M + 1] - starts[s, :M]).astype(I64)
        if reduce == "max":
            best, win = np.zeros((M, c), F32), np.zeros((M, c), I32)
            done = np.zeros((M, c), bool)
            for p in range(int(size.max())):
                js = np.nonzero(size > p)[0]
                i = order[s, beg[js] + p]
                v = feat[s, i]
                with np.errstate(invalid="ignore"):
                    take = ~done[js] & (np.isnan(v) | (v > best[js]) if p else np.ones_like(v, bool))
                best[js] = np.where(take, v, best[js])
                win[js] = np.where(take, i[:, None].astype(I32), win[js])
                done[js] |= take & np.isnan(v)
            out[s, :M], arg[s, :M] = best, win
        else:
            acc = np.zeros((M, c), F64)
            for p in range(int(size.max())):
                js = np.nonzero(size > p)[0]
                acc[js] = acc[js] + feat[s, order[s, beg[js] + p]].astype(F64)
            if reduce == "mean":
                acc = acc / size.astype(F64)[:, None]
            out[s, :M] = acc.astype(F32)
    return (out, arg) if reduce == "max" else out


# ---- rf_grid_unpool ----------------------------------------------------------------------------------------------------------
def unpool_ref(src, cluster, starts=None, arg=None, mode="copy"):
    src = np.asarray(src, F32)
    b, n, c = src.shape
    dst = np.zeros((b, n, c), F32)
    for s in range(b):
        live = np.nonzero(cluster[s] >= 0)[0]
        j = cluster[s, live].astype(I64)
        v = src[s, j]
        if mode == "mean":
            cnt = (starts[s, j + 1] - starts[s, j]).astype(F64)[:, None]
            v = (v.astype(F64) / cnt).astype(F32)
        elif mode == "max":
            v = np.where(arg[s, j] == live[:, None], v, F32(0.0))
        dst[s, live] = v
    return dst
