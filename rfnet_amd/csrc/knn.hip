// knn.hip -- knn_point (tf_ops/grouping/tf_grouping.py:48-73) and its gradient for gfx950.
//
// The reference computes knn_point as tensor ops: dist = sum((xyz1 - xyz2)^2) over (b, m, n), then tf.nn.top_k(-dist, k), which
// breaks ties by the lower index.  Here no (b, m, n) tensor exists: every query keeps its k best candidates in registers.
//   - the distance is the UNFUSED fp32 expression ((dx*dx)+(dy*dy))+(dz*dz), dx = x1 - x2 (this file is compiled with
//     -ffp-contract=off, as interpolate.hip);
//   - a candidate is the 64-bit key (rank of d, index); the k smallest keys, ascending, are the result.  The rank is the bit
//     pattern of d plus one (d is never negative, so that orders as the float does, +inf last) and 0 for a NaN: a NaN distance
//     ranks before every number, as in torch.topk(-dist) -- so a query with a NaN coordinate gets indices 0..k-1;
//   - val = -d is written from the key (a NaN as -NaN).
//
// The list: KB >= k slots of 64-bit keys in registers, sorted ascending, constant-index and fully unrolled (a dynamically
// indexed register array would go to scratch), one kernel per bucket KB in {4, 8, 16, 32, 64}.  The first KB - k slots hold
// key 0, which no key is below, so they never move: the live list is the last k slots and its k-th best is always slot KB - 1.
// A candidate is first tested against the k-th best's distance as a float -- thr, NaN while the list is not full (every
// candidate passes), -inf once it is full of NaN distances (only NaNs pass) -- behind a wave-uniform __ballot branch, and only
// then keyed and inserted by exact 64-bit comparisons (KB compares, 4 KB selects); the scan first buffers what passes (below).
//
// knn_scan_kernel (rf_knn): one lane per query, the candidates wave-uniform through SGPRs in index order, as three_nn_kernel.
// In index order a tie never displaces the earlier index, so the float pre-test is strict ('d < thr').
//
// knn_boxes_kernel (rf_knn_boxes): both sets in rf_nn_sort order, as three_nn_boxes_kernel: a wave of 64 neighbouring queries
// visits the 16-record candidate blocks whose box bound is <= some lane's k-th distance, nearest superblock first.  Visits go
// in any order, so the pre-test admits ties ('d <= thr') and the keys settle them.  The bound is the same unfused expression
// on the per-axis gaps (box_bound.hpp), so it never exceeds a distance inside the box: the result is the scan's, bit for bit.
// Non-finite values break the bounds (the sort leaves such points out of the boxes, and a NaN distance ranks FIRST): a wave
// with a non-finite query, or a sample whose candidate set holds a non-finite coordinate (the sort's flag), visits every
// superblock without a test -- still the same keys, so still the scan's result.
//
// The gradient (rf_knn_grad): term(j, t) = 2 g[j, t] (x1[i] - x2[j]), i = idx[j, t]; grad_xyz2[j] = sum_t term, one lane per
// query; grad_xyz1[i] = -sum of the terms that name i, a scatter done as group_point's (scatter_rows.hip): the m k slots
// counting-sorted by i, then one lane per candidate sums its slots and writes its row once (zeros for a row nobody names).
// Sums in double on both sides.
#include "common.hpp"
#include "scatter_rows.hpp"
#include "nn_pruned.hpp"
#include "box_bound.hpp"

namespace {

typedef unsigned long long u64;

constexpr int KN_MAXK = 64;
constexpr int KN_TPB = 256;
constexpr int KN_SUB = 8;  // candidates per scalar-load sub-chunk

__device__ __forceinline__ u64 kn_key(float d, unsigned i) {
    const unsigned r = d != d ? 0u : __float_as_uint(d) + 1u;
    return ((u64)r << 32) | (u64)i;
}
// the float pre-test threshold of a k-th best key: NaN (not full: all pass), -inf (a NaN distance: only NaNs pass), else d
__device__ __forceinline__ float kn_thr(u64 key) {
    const unsigned r = (unsigned)(key >> 32);
    return r == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : (r == 0u ? -INFINITY : __uint_as_float(r - 1u));
}
__device__ __forceinline__ float kn_val(u64 key) {
    const unsigned r = (unsigned)(key >> 32);
    return r == 0u ? __uint_as_float(0xFFC00000u) : -__uint_as_float(r - 1u);
}

template <int KB>
__device__ __forceinline__ void kn_insert(u64 (&L)[KB], u64 key) {
    bool c[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) c[t] = key < L[t];
#pragma unroll
    for (int t = KB - 1; t > 0; t--) L[t] = c[t - 1] ? L[t - 1] : (c[t] ? key : L[t]);
    L[0] = c[0] ? key : L[0];
}

template <int KB>
__device__ __forceinline__ void kn_write(const u64 (&L)[KB], int k, float *__restrict__ val, int *__restrict__ idx) {
#pragma unroll
    for (int t = 0; t < KB; t++) {
        if (t >= KB - k) {
            val[t - (KB - k)] = kn_val(L[t]);
            idx[t - (KB - k)] = (int)(unsigned)L[t];
        }
    }
}

// Candidates that pass the pre-test are not inserted at once: each lane appends them to a buffer of its own in LDS, and the wave
// inserts only when some lane's buffer is full (or at the end of a run of candidates).  Inserting at once makes the whole wave run
// the KB-slot insertion whenever ANY of its 64 lanes admits a candidate -- nearly every candidate of the first 64 k -- while a
// flush costs as many insertions as the fullest buffer holds: the wave's insertions fall from ~ the union of its lanes' to ~ the
// largest lane's.  The threshold a lane tests against is then that of its last flush, never below the true one: nothing that
// belongs in the list is missed, and the exact keys decide.
constexpr int KN_BUF = 16;  // entries per lane
#define KN_FLUSH(BD, BI, TID)                                                                                        \
    {                                                                                                                \
        for (int f_ = 0; f_ < KN_BUF; f_++) {                                                                        \
            if (__ballot(f_ < cnt) == 0ull) break; /* wave-uniform */                                                \
            const unsigned i_ = f_ < cnt ? BI[f_][TID] : 0xFFFFFFFFu;                                                \
            kn_insert<KB>(L, i_ == 0xFFFFFFFFu ? ~0ull : kn_key(BD[f_][TID], i_));                                   \
        }                                                                                                            \
        cnt = 0;                                                                                                     \
        thr = kn_thr(L[KB - 1]);                                                                                     \
    }

// ---- scan: one lane per query, every candidate ----------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(KN_TPB) void knn_scan_kernel(int n, int m, int k, const float *__restrict__ xyz1,
                                                          const float *__restrict__ xyz2, float *__restrict__ val,
                                                          int *__restrict__ idx) {
    const int bi = blockIdx.y;
    const int j = blockIdx.x * KN_TPB + threadIdx.x;
    const float *__restrict__ C = xyz1 + (size_t)bi * n * 3;
    const float *__restrict__ Q = xyz2 + (size_t)bi * m * 3;
    const int jj = min(j, m - 1);
    const float x2 = Q[jj * 3], y2 = Q[jj * 3 + 1], z2 = Q[jj * 3 + 2];
    u64 L[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) L[t] = t < KB - k ? 0ull : ~0ull;
    float thr = __uint_as_float(0x7FC00000u);
    __shared__ float bd[KN_BUF][KN_TPB];
    __shared__ unsigned bx[KN_BUF][KN_TPB];
    const int tid = threadIdx.x;
    int cnt = 0;
    // (a macro, as TN_CONSIDER: the candidate's coordinates and index stay scalar operands)
#define KN_CONSIDER(cx, cy, cz, ci)                                                    \
    {                                                                                  \
        const float dx_ = (cx) - x2, dy_ = (cy) - y2, dz_ = (cz) - z2;                  \
        const float xx_ = dx_ * dx_, yy_ = dy_ * dy_, zz_ = dz_ * dz_;                  \
        const float d_ = (xx_ + yy_) + zz_;                                             \
        const bool in_ = !(d_ >= thr);                                                  \
        if (__ballot(in_) != 0ull) { /* wave-uniform */                                 \
            asm volatile("; some lane admits");                                         \
            if (in_) {                                                                  \
                bd[cnt][tid] = d_;                                                      \
                bx[cnt][tid] = (unsigned)(ci);                                          \
                cnt++;                                                                  \
            }                                                                           \
            if (__ballot(cnt == KN_BUF) != 0ull) KN_FLUSH(bd, bx, tid);                 \
        }                                                                               \
    }
    const int n_full = (n / KN_SUB) * KN_SUB;
    if (n_full > 0) {
        float pa[3 * KN_SUB], pb[3 * KN_SUB];
        auto fetch = [&](float (&dst)[3 * KN_SUB], int c0) {
            const float *cp = C + (size_t)min(c0, n - KN_SUB) * 3;  // uniform -> s_load; clamped in bounds
#pragma unroll
            for (int i = 0; i < 3 * KN_SUB; i++) dst[i] = cp[i];
        };
#define KN_SCAN8(c, c0) \
    _Pragma("unroll") for (int u = 0; u < KN_SUB; u++) KN_CONSIDER(c[u * 3], c[u * 3 + 1], c[u * 3 + 2], (c0) + u)
        fetch(pa, 0);
        for (int c0 = 0; c0 < n_full; c0 += 2 * KN_SUB) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): pa has arrived
            __builtin_amdgcn_sched_barrier(0);
            fetch(pb, c0 + KN_SUB);
            __builtin_amdgcn_sched_barrier(0);
            KN_SCAN8(pa, c0);
            if (c0 + KN_SUB >= n_full) break;
            __builtin_amdgcn_s_waitcnt(0xC07F);  // pb has arrived
            __builtin_amdgcn_sched_barrier(0);
            fetch(pa, c0 + 2 * KN_SUB);
            __builtin_amdgcn_sched_barrier(0);
            KN_SCAN8(pb, c0 + KN_SUB);
        }
#undef KN_SCAN8
    }
#pragma unroll 1
    for (int c = n_full; c < n; c++) KN_CONSIDER(C[c * 3], C[c * 3 + 1], C[c * 3 + 2], c);
#undef KN_CONSIDER
    KN_FLUSH(bd, bx, tid);
    if (j < m) kn_write<KB>(L, k, val + ((size_t)bi * m + j) * k, idx + ((size_t)bi * m + j) * k);
}

// ---- boxed: a wave of 64 sorted queries, the candidate blocks that can still matter -----------------------------------------
constexpr int KB_WAVES = 4;  // waves per workgroup, each on its own (no barrier)

template <int KB>
__global__ __launch_bounds__(64 * KB_WAVES) void knn_boxes_kernel(
    int b, int m, int k, int npq, int npc, const float *__restrict__ qxyz, const int *__restrict__ qorig,
    const float *__restrict__ qb64, const float *__restrict__ cxyz, const int *__restrict__ corig,
    const float *__restrict__ cb16, const float *__restrict__ cb64, const int *__restrict__ cflags,
    float *__restrict__ val, int *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int bpb = ((npq >> 6) + KB_WAVES - 1) / KB_WAVES;  // workgroups per sample
    const unsigned logical = rf::xcd_contiguous(blockIdx.x, gridDim.x);  // a sample's workgroups on one XCD
    const int bi = logical / bpb;
    const int group = (logical - bi * bpb) * KB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (group * 64 >= npq) return;  // (uniform)
    const int p = group * 64 + lane;
    const float *__restrict__ Q = qxyz + ((size_t)bi * npq + p) * 3;
    const float x2 = Q[0], y2 = Q[1], z2 = Q[2];
    const int oq = qorig[(size_t)bi * npq + p];
    const bool search = oq >= 0;  // (a padding record searches nothing)
    const u64 smask = __ballot(search);
    // every superblock, untested: a non-finite query in the wave, or one in the candidate set (the sort's flag, behind pos0)
    const bool full = __ballot(search && !(isfinite(x2) && isfinite(y2) && isfinite(z2))) != 0ull || cflags[2 * b + bi] != 0;
    u64 L[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) L[t] = (search && t >= KB - k) ? ~0ull : 0ull;
    float thr = search ? __uint_as_float(0x7FC00000u) : -INFINITY;
    const float *__restrict__ CX = cxyz + (size_t)bi * npc * 3;
    const int *__restrict__ CO = corig + (size_t)bi * npc;
    const int nsb = npc >> 6;
    const float *__restrict__ B16 = cb16 + (size_t)bi * nsb * 24;
    const float *__restrict__ B64 = cb64 + (size_t)bi * nsb * 8;
    // the lane's pruning distance: +inf while its list is not full (only in a finite wave: thr is then never -inf)
#define KB_PRUNE (thr != thr ? INFINITY : thr)

    // One candidate, inserted at once (a buffer as the scan's, flushed inside the visits, pushed this kernel into scratch; its
    // nearest-first order fills the lists early anyway).  A padding record (index -1, coordinates +inf) is keyed above everything
    // and never enters.  A lane that does not search admits nothing.
#define KB_CONSIDER(cx, cy, cz, oi)                                                               \
    {                                                                                             \
        const float dx_ = (cx) - x2, dy_ = (cy) - y2, dz_ = (cz) - z2;                             \
        const float xx_ = dx_ * dx_, yy_ = dy_ * dy_, zz_ = dz_ * dz_;                             \
        const float d_ = (xx_ + yy_) + zz_;                                                        \
        const bool in_ = !(d_ > thr) && search;                                                    \
        if (__ballot(in_) != 0ull) { /* wave-uniform */                                            \
            asm volatile("; some lane may insert");                                                \
            if (in_) {                                                                             \
                kn_insert<KB>(L, (oi) < 0 ? ~0ull : kn_key(d_, (unsigned)(oi)));                   \
                thr = kn_thr(L[KB - 1]);                                                           \
            }                                                                                      \
        }                                                                                         \
    }
#ifdef KB_STATS
    int nblk = 0;  // (uniform) 16-record block scans
#endif
    auto visit = [&](int sb, bool test) {
        unsigned hm = 0xFFu;  // the half-blocks to scan
        if (test) {
            const float *bx = B16 + (size_t)sb * 24;  // (uniform -> scalar loads)
            float bb[24];
#pragma unroll
            for (int i = 0; i < 24; i++) bb[i] = bx[i];
            hm = 0u;
            const float pr = KB_PRUNE;
#pragma unroll
            for (int blk = 0; blk < 4; blk++) {
                const float lb = tb_bound(bb[blk * 6], bb[blk * 6 + 1], bb[blk * 6 + 2], bb[blk * 6 + 3], bb[blk * 6 + 4],
                                          bb[blk * 6 + 5], x2, y2, z2, x2, y2, z2);
                if ((__ballot(lb <= pr) & smask) != 0ull) hm |= 3u << (2 * blk);  // (uniform)
            }
            if (hm == 0u) return;
        }
#ifdef KB_STATS
        nblk += __builtin_popcount(hm) >> 1;
#endif
        const float *cb = CX + (size_t)sb * 192;
        const int *ob = CO + sb * 64;
        float ca[24], cc[24];
        int oa[8], oc[8];
#define KB_FETCH(CC, O, H)                                              \
    {                                                                   \
        const float *cp_ = cb + (H) * 24;                               \
        const int *op_ = ob + (H) * 8;                                  \
        _Pragma("unroll") for (int i = 0; i < 24; i++) CC[i] = cp_[i];  \
        _Pragma("unroll") for (int i = 0; i < 8; i++) O[i] = op_[i];    \
    }
#define KB_SCAN8(CC, O) _Pragma("unroll") for (int u = 0; u < 8; u++) KB_CONSIDER(CC[u * 3], CC[u * 3 + 1], CC[u * 3 + 2], O[u])
        int h = __builtin_ctz(hm);
        hm &= hm - 1u;
        KB_FETCH(ca, oa, h);
        for (;;) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): set a has arrived
            __builtin_amdgcn_sched_barrier(0);
            const bool more_b = hm != 0u;
            if (more_b) {
                h = __builtin_ctz(hm);
                hm &= hm - 1u;
                KB_FETCH(cc, oc, h);
            }
            __builtin_amdgcn_sched_barrier(0);
            KB_SCAN8(ca, oa);
            if (!more_b) break;
            __builtin_amdgcn_s_waitcnt(0xC07F);  // set c has arrived
            __builtin_amdgcn_sched_barrier(0);
            const bool more_a = hm != 0u;
            if (more_a) {
                h = __builtin_ctz(hm);
                hm &= hm - 1u;
                KB_FETCH(ca, oa, h);
            }
            __builtin_amdgcn_sched_barrier(0);
            KB_SCAN8(cc, oc);
            if (!more_a) break;
        }
#undef KB_SCAN8
#undef KB_FETCH
    };

    if (full) {
        for (int sb = 0; sb < nsb; sb++) visit(sb, false);
    } else {
        // the wave's own box (its 64 queries are one superblock of their sorted set)
        const float *qb = qb64 + ((size_t)bi * (npq >> 6) + group) * 8;
        const float qlx = qb[0], qly = qb[1], qlz = qb[2], qhx = qb[4], qhy = qb[5], qhz = qb[6];
        // 1. the candidate superblock nearest to the wave's box goes first
        float best = INFINITY;
        int arg = 0;
        for (int r0 = 0; r0 < nsb; r0 += 64) {
            const int g = r0 + lane;
            float lb = INFINITY;
            if (g < nsb) {
                const float4 lo = *(const float4 *)(B64 + (size_t)g * 8), hi = *(const float4 *)(B64 + (size_t)g * 8 + 4);
                lb = tb_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
            }
            if (lb < best) best = lb, arg = g;
        }
        const float wmin = tb_wave_min(best);
        const u64 at = __ballot(best == wmin);
        const int seed = at != 0ull ? __builtin_amdgcn_readlane(arg, __builtin_ctzll(at)) : 0;
        visit(seed, false);
        // 2. every other superblock whose box is not beyond the wave's largest k-th distance (which shrinks as the visits go),
        //    nearest first, 64 superblocks at a time.  (No finite bound is skipped while a lane's list is not full: its
        //    pruning distance is +inf then.)
        float wk = tb_wave_max(search ? KB_PRUNE : -INFINITY);
        for (int r0 = 0; r0 < nsb; r0 += 64) {
            const int g = r0 + lane;
            float lb = INFINITY;
            if (g < nsb && g != seed) {
                const float4 lo = *(const float4 *)(B64 + (size_t)g * 8), hi = *(const float4 *)(B64 + (size_t)g * 8 + 4);
                lb = tb_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
            }
            bool pend = g < nsb && g != seed && lb <= wk;
            while (__ballot(pend) != 0ull) {  // (uniform)
                const float wmin2 = tb_wave_min(pend ? lb : INFINITY);
                if (!(wmin2 <= wk)) break;
                const int jn = __builtin_ctzll(__ballot(pend && lb == wmin2));
                pend = pend && lane != jn;
                visit(r0 + jn, true);
                wk = tb_wave_max(search ? KB_PRUNE : -INFINITY);
            }
        }
    }
#undef KB_CONSIDER
#undef KB_PRUNE
    if (search) {
        const size_t o = ((size_t)bi * m + oq) * k;
        kn_write<KB>(L, k, val + o, idx + o);
#ifdef KB_STATS
        idx[o] = nblk;
#endif
    }
}

// ---- gradient -----------------------------------------------------------------------------------------------------------
constexpr int KG_TPB = 256;

// grad_xyz2[j] = sum_t 2 g (x1[i] - x2[j]); slots whose index is outside [0, n) add nothing
__global__ __launch_bounds__(KG_TPB) void knn_grad_query_kernel(int n, int m, int k, const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, const int *__restrict__ idx,
                                                                const float *__restrict__ gval, float *__restrict__ grad2) {
    const int bi = blockIdx.y;
    const int j = blockIdx.x * KG_TPB + threadIdx.x;
    if (j >= m) return;
    const float *__restrict__ X1 = xyz1 + (size_t)bi * n * 3;
    const size_t q = (size_t)bi * m + j;
    const float x2 = xyz2[q * 3], y2 = xyz2[q * 3 + 1], z2 = xyz2[q * 3 + 2];
    const int *__restrict__ I = idx + q * k;
    const float *__restrict__ G = gval + q * k;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int t = 0; t < k; t++) {
        const int i = I[t];
        if (i < 0 || i >= n) continue;
        const double g2 = 2.0 * (double)G[t];
        ax += g2 * (double)(X1[i * 3] - x2);
        ay += g2 * (double)(X1[i * 3 + 1] - y2);
        az += g2 * (double)(X1[i * 3 + 2] - z2);
    }
    grad2[q * 3] = (float)ax;
    grad2[q * 3 + 1] = (float)ay;
    grad2[q * 3 + 2] = (float)az;
}

// grad_xyz1[i] = -sum over the slots s = j k + t that name i of 2 g[s] (x1[i] - x2[j]), the slots from the counting sort
__global__ __launch_bounds__(KG_TPB) void knn_grad_rows_kernel(int n, int m, int k, const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2, const float *__restrict__ gval,
                                                               const int *__restrict__ row_start, const int *__restrict__ perm,
                                                               float *__restrict__ grad1) {
    const int bi = blockIdx.y;
    const int i = blockIdx.x * KG_TPB + threadIdx.x;
    if (i >= n) return;
    const size_t S = (size_t)m * k;
    const int *__restrict__ RS = row_start + (size_t)bi * (n + 1);
    const int *__restrict__ P = perm + (size_t)bi * S;
    const float *__restrict__ X2 = xyz2 + (size_t)bi * m * 3;
    const float *__restrict__ G = gval + (size_t)bi * S;
    const size_t r = (size_t)bi * n + i;
    const float x1 = xyz1[r * 3], y1 = xyz1[r * 3 + 1], z1 = xyz1[r * 3 + 2];
    double ax = 0.0, ay = 0.0, az = 0.0;
    const int end = RS[i + 1];
    for (int p = RS[i]; p < end; p++) {
        const int s = P[p];
        const int j = s / k;
        const double g2 = 2.0 * (double)G[s];
        ax -= g2 * (double)(x1 - X2[j * 3]);
        ay -= g2 * (double)(y1 - X2[j * 3 + 1]);
        az -= g2 * (double)(z1 - X2[j * 3 + 2]);
    }
    grad1[r * 3] = (float)ax;
    grad1[r * 3 + 1] = (float)ay;
    grad1[r * 3 + 2] = (float)az;
}

bool kn_supported(int b, int n, int m, int k) {
    return b > 0 && b <= 65535 && n > 0 && m > 0 && n <= rfp::kMaxPoints && m <= rfp::kMaxPoints && k >= 1 && k <= KN_MAXK &&
           k <= n;
}

#define KN_DISPATCH(k, GO)                   \
    do {                                     \
        if ((k) <= 4) { GO(4); }             \
        else if ((k) <= 8) { GO(8); }        \
        else if ((k) <= 16) { GO(16); }      \
        else if ((k) <= 32) { GO(32); }      \
        else { GO(64); }                     \
    } while (0)

}  // namespace

extern "C" {

int rf_knn(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx, rf_stream_t stream) {
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!xyz1 || !xyz2 || !val || !idx) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(rf::ceil_div(m, KN_TPB), b);
#define KN_GO(KB) RF_LAUNCH("knn", knn_scan_kernel<KB>, grid, dim3(KN_TPB), 0, s, n, m, k, xyz1, xyz2, val, idx)
    KN_DISPATCH(k, KN_GO);
#undef KN_GO
    return RF_OK;
}

size_t rf_knn_boxes_workspace_bytes(int b, int n, int m) {
    if (!kn_supported(b, n, m, 1)) return 0;
    return rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m);
}

int rf_knn_boxes(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const void *sorted1, const void *sorted2,
                 float *val, int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!xyz1 || !xyz2 || !val || !idx || !workspace || !rf::aligned16(workspace)) return RF_EINVAL;
    if ((sorted1 && !rf::aligned16(sorted1)) || (sorted2 && !rf::aligned16(sorted2))) return RF_EINVAL;
    if (workspace_bytes < rf_knn_boxes_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    rfp::Sorted sv[2];
    sv[0] = rfp::sorted_view(b, n, sorted1 ? sorted1 : workspace);
    sv[1] = rfp::sorted_view(b, m, sorted2 ? sorted2 : (const char *)workspace + rfp::sorted_bytes(b, n));
    {  // the sets that came without a handle, in one launch
        int nn[2];
        const float *src[2];
        rfp::Sorted out[2];
        int c = 0;
        if (!sorted1) nn[c] = n, src[c] = xyz1, out[c] = sv[0], c++;
        if (!sorted2) nn[c] = m, src[c] = xyz2, out[c] = sv[1], c++;
        if (c > 0)
            if (int e = rfp::sort_sets(b, c, nn, src, out, s, nullptr)) return e;
    }
    const dim3 grid(rf::ceil_div(sv[1].npad / 64, KB_WAVES) * b);
#define KB_GO(KB)                                                                                                              \
    RF_LAUNCH("knn_boxes", knn_boxes_kernel<KB>, grid, dim3(64 * KB_WAVES), 0, s, b, m, k, sv[1].npad, sv[0].npad, sv[1].xyz, \
              sv[1].orig, sv[1].box64, sv[0].xyz, sv[0].orig, sv[0].box16, sv[0].box64, sv[0].pos0, val, idx)
    KN_DISPATCH(k, KB_GO);
#undef KB_GO
    return RF_OK;
}

size_t rf_knn_grad_workspace_bytes(int b, int n, int m, int k) {
    if (!kn_supported(b, n, m, k)) return 0;
    return rfs::rows_csr_workspace_bytes(b, n, (long)m * k);
}

int rf_knn_grad(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *idx, const float *grad_val,
                float *grad_xyz1, float *grad_xyz2, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!xyz1 || !xyz2 || !idx || !grad_val || !grad_xyz1 || !grad_xyz2 || !workspace || !rf::aligned16(workspace))
        return RF_EINVAL;
    if (workspace_bytes < rf_knn_grad_workspace_bytes(b, n, m, k)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    RF_LAUNCH("knn_grad_query", knn_grad_query_kernel, dim3(rf::ceil_div(m, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k, xyz1, xyz2,
              idx, grad_val, grad_xyz2);
    if (int e = rfs::rows_csr_sort(b, n, (long)m * k, idx, workspace, "knn_grad_sort", s)) return e;
    RF_LAUNCH("knn_grad_rows", knn_grad_rows_kernel, dim3(rf::ceil_div(n, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k, xyz1, xyz2,
              grad_val, (const int *)workspace, rfs::rows_csr_perm(b, n, workspace), grad_xyz1);
    return RF_OK;
}

}  // extern "C"
