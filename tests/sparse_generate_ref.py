"""A numpy restatement of the decoder entries of include/rfops.h (rf_sparse_generate_map, rf_sparse_prune_map, rf_sparse_lookup,
rf_sparse_take_rows) as plain loops over samples and rows, in the words of the header.  The convolution onto the generated cells
is tests/sparse_stride_ref.py's (imported unchanged as `S`) fed with the generated child / up.  tests/test_sparse_generate_host.py
holds these loops to dictionary and set based routes on the CPU; the GPU tests hold the kernels to them byte for byte.  Not a
test module itself."""
import numpy as np

import sparse_stride_ref as S  # noqa: F401  (conv_ref, grad_weight_ref, UP, UP_GRAD_INPUT on the generated maps)
from sparse_conv_ref import F32, I32, I64, counts  # noqa: F401

LO, HI = -32768, 32767
PLO, PHI = -16384, 16383
MAX_POINTS, MAX_CHANNELS = 16384, 2048


def in_range(c, lo=LO, hi=HI):
    return all(lo <= int(v) <= hi for v in c)


def generate_ref(coords, count=None, n_fine=None):
    """-> dict(coords (b, nf, 3), count (b,), total (b,), child (b, nc, 8), up (b, nf)), all int32"""
    coords = np.asarray(coords)
    b, nc, _ = coords.shape
    nf = min(8 * nc, MAX_POINTS) if n_fine is None else int(n_fine)
    assert 8 <= nf <= MAX_POINTS and 1 <= nc <= nf
    out = dict(coords=np.zeros((b, nf, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               child=np.full((b, nc, 8), -1, I32), up=np.full((b, nf), -1, I32))
    M = counts(count, b, nc)
    for s in range(b):
        seen = set()
        r = 0  # parents of lower row index
        for j in range(int(M[s])):
            c = tuple(int(v) for v in coords[s, j])
            if not in_range(c) or c in seen:
                continue  # not live
            seen.add(c)
            if not in_range(c, PLO, PHI):
                continue  # live, no parent
            if r < nf // 8:
                for t in range(8):
                    out["child"][s, j, t] = 8 * r + t
                    out["up"][s, 8 * r + t] = 8 * j + t
                    out["coords"][s, 8 * r + t] = [2 * c[0] + ((t >> 2) & 1), 2 * c[1] + ((t >> 1) & 1), 2 * c[2] + (t & 1)]
            r += 1
        out["total"][s], out["count"][s] = 8 * r, 8 * min(r, nf // 8)
    return out


def prune_ref(coords, keep, count=None, n_out=None):
    """-> dict(coords (b, no, 3), count (b,), total (b,), src (b, no), dst (b, n)), all int32"""
    coords, keep = np.asarray(coords), np.asarray(keep)
    b, n, _ = coords.shape
    no = n if n_out is None else int(n_out)
    assert 1 <= no <= n and keep.shape == (b, n)
    out = dict(coords=np.zeros((b, no, 3), I32), count=np.zeros(b, I32), total=np.zeros(b, I32),
               src=np.full((b, no), -1, I32), dst=np.full((b, n), -1, I32))
    M = counts(count, b, n)
    for s in range(b):
        r = 0
        for i in range(int(M[s])):
            if keep[s, i] == 0:
                continue
            if r < no:
                out["src"][s, r], out["dst"][s, i] = i, r
                out["coords"][s, r] = coords[s, i]
            r += 1
        out["total"][s], out["count"][s] = r, min(r, no)
    return out


def lookup_ref(coords, table, count=None, tcount=None, shift=0):
    """-> idx (b, n) int32"""
    coords, table = np.asarray(coords), np.asarray(table)
    b, n, _ = coords.shape
    m = table.shape[1]
    assert 0 <= shift <= 15
    idx = np.full((b, n), -1, I32)
    M, Mt = counts(count, b, n), counts(tcount, b, m)
    for s in range(b):
        t = table[s, :int(Mt[s])].astype(I64)
        usable = ((t >= LO) & (t <= HI)).all(1)
        cell = t >> shift  # (>> of a negative int64 is the floor)
        for i in range(int(M[s])):
            c = coords[s, i].astype(I64)
            if not in_range(c):
                continue
            hit = np.nonzero(usable & (cell == c).all(1))[0]  # the scan over the table's rows, ascending
            if len(hit):
                idx[s, i] = hit[0]
    return idx


def take_ref(src, idx, count=None):
    """-> dst (b, n_dst, c) fp32, copies as bytes"""
    src, idx = np.asarray(src, F32), np.asarray(idx)
    b, ns, c = src.shape
    nd = idx.shape[1]
    dst = np.zeros((b, nd, c), F32)
    M = counts(count, b, nd)
    for s in range(b):
        for r in range(int(M[s])):
            if 0 <= int(idx[s, r]) < ns:
                dst[s, r] = src[s, int(idx[s, r])]
    return dst


def same_maps(got, want):
    """every tensor of `want` equals got's as int32 bytes"""
    return all(np.asarray(got[k]).dtype == I32 and np.asarray(got[k]).shape == want[k].shape
               and np.asarray(got[k]).tobytes() == want[k].tobytes() for k in want)
