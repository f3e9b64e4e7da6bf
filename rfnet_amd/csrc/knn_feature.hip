// knn_feature.hip -- k-nearest neighbours in feature space (rf_knn_feature, include/rfops.h): the graph DGCNN's EdgeConv
// rebuilds on the features of every layer.  knn.hip is three-dimensional; here a distance is |q|^2 + |x|^2 - 2 q.x over c
// channels, the inner products come from the fp32-input matrix instruction, and no (b, m, n) tensor exists.
//
// The arithmetic is the header's, operation for operation: ip is an fmaf chain over the channels in ascending order from +0
// (v_mfma_f32_32x32x2_f32 IS that chain, two channels per instruction, the accumulator carried from instruction to
// instruction; an odd c gets one channel of zeros), sq1 / sq2 the same chain on x * x (knn_feature_sq_kernel, into the
// workspace), d = fmaf(-2, ip, sq2 + sq1).  tests/test_knn_feature_host.py restates it in numpy and the GPU tests compare bits.
//
// knn_feature_kernel: a workgroup of KF_WAVES waves owns 64 KF_WAVES queries of one sample, a wave 64 of them.  For every tile of
// 32 candidates it runs over the channels in slabs of KF_KS: the slab of the 32 candidates and of the workgroup's queries is staged
// in LDS ([row][channel], row stride KF_KS + 1: the operand reads -- lane l takes row l & 31, channel 2 s + (l >> 5) -- touch 64
// different banks), and each wave issues two MFMAs per channel pair, candidates as A (rows), its queries 0..31 and 32..63 as
// the two B operands (columns).  The two accumulators live across the slabs, so the chain order is the contract's.  Staging
// goes through registers one slab ahead, so the global loads of the next slab fly while this one is multiplied.
// A 32x32 result has its column on lane & 31 and rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r: the two half-waves hold
// different candidates of the same queries.  The halves trade registers -- the lower half gives away its tile-1 registers and
// takes the upper half's tile-0 registers -- after which lane l holds all 32 candidates of query l of the wave: one list per
// lane, every lane busy, nothing to merge.
// The list is knn.hip's (knn_list.hpp): 64-bit keys (rank of d, index) in KB registers, a float pre-test against the k-th best
// behind a wave-uniform __ballot, what passes buffered per lane in LDS and inserted in batches.  A lane meets its candidates in
// index order, so the pre-test is strict as in knn.hip's scan.  d is signed here, so the rank is the order-preserving map of a
// signed float (kf_key).
#include "common.hpp"
#include "group_internal.hpp"
#include "knn_list.hpp"

namespace {

constexpr int KF_MAXC = 2048;
constexpr int KF_WAVES = 2;
constexpr int KF_TPB = 64 * KF_WAVES;  // one query per lane
constexpr int KF_TC = 32;              // candidates per tile: the rows of one MFMA
constexpr int KF_KS = 32;              // channels per slab
constexpr int KF_LD = KF_KS + 1;
constexpr int KF_BUF = 16;             // buffered candidates per lane
constexpr int KF_GROUP = 8;            // candidates between two looks at the buffers
constexpr int KF_SQ_TPB = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// rank of a distance: 0 for a NaN (before everything), else 1 + the order-preserving map of a signed float, -0 as +0:
// -inf -> 0x00800000, +0 -> 0x80000001, +inf -> 0xFF800001; 0xFFFFFFFF stays the empty slot's
__device__ __forceinline__ u64 kf_key(float d, unsigned i) {
    const unsigned u = __float_as_uint(d == 0.f ? 0.f : d);
    const unsigned r = d != d ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1u;
    return ((u64)r << 32) | (u64)i;
}
__device__ __forceinline__ float kf_dist(unsigned r) {  // of a rank that is neither 0 nor 0xFFFFFFFF
    const unsigned s = r - 1u;
    return __uint_as_float((s & 0x80000000u) ? (s & 0x7FFFFFFFu) : ~s);
}
// the float pre-test threshold of a k-th best key: NaN (not full: all pass), -inf (a NaN distance: only NaNs pass), else d
__device__ __forceinline__ float kf_thr(u64 key) {
    const unsigned r = (unsigned)(key >> 32);
    return r == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : (r == 0u ? -INFINITY : kf_dist(r));
}
__device__ __forceinline__ float kf_val(u64 key) {
    const unsigned r = (unsigned)(key >> 32);
    return r == 0u ? __uint_as_float(0xFFC00000u) : -kf_dist(r);
}

// sq[row] = the fmaf chain of x * x over the row's channels, ascending, from +0; rows = the b n rows of feat1, then the b m of feat2
__global__ __launch_bounds__(KF_SQ_TPB) void knn_feature_sq_kernel(long rows1, long rows2, int c, const float *__restrict__ feat1,
                                                                   const float *__restrict__ feat2, float *__restrict__ sq1,
                                                                   float *__restrict__ sq2) {
    const long r = (long)blockIdx.x * KF_SQ_TPB + threadIdx.x;
    if (r >= rows1 + rows2) return;
    const bool first = r < rows1;
    const float *__restrict__ x = first ? feat1 + (size_t)r * c : feat2 + (size_t)(r - rows1) * c;
    float acc = 0.f;
    for (int ch = 0; ch < c; ch++) acc = fmaf(x[ch], x[ch], acc);
    if (first) sq1[r] = acc;
    else sq2[r - rows1] = acc;
}

// insert what the lanes buffered (a wave's cost: its fullest buffer), empty the buffers, refresh the thresholds
template <int KB>
__device__ __forceinline__ void kf_flush(u64 (&L)[KB], int &cnt, float &thr, const float (*bd)[KF_TPB],
                                         const unsigned (*bx)[KF_TPB], int tid) {
#pragma unroll 1
    for (int f = 0; f < KF_BUF; f++) {
        if (__ballot(f < cnt) == 0ull) break;  // wave-uniform
        kn_insert<KB>(L, f < cnt ? kf_key(bd[f][tid], bx[f][tid]) : ~0ull);
    }
    cnt = 0;
    thr = kf_thr(L[KB - 1]);
}

// RAGGED: the candidates are the sample's first nv rows, the queries its first mv; the list is opened for kv = min(k, nv)
// neighbours, slots [kv, k) and the rows of padded queries are zeros (knn.hip's rule).  Rows behind the counts are never read.
// Occupancy: the lists of up to 16 slots fit two waves per SIMD and are held to that (without the hint the compiler spends the
// whole register file on scheduling freedom); the 32- and 64-slot lists, the prefetch registers and the accumulators need more
// than 256 registers and run one wave per SIMD, with the prefetch to cover the loads.
template <int KB, bool RAGGED>
__global__ __launch_bounds__(KF_TPB) __attribute__((amdgpu_waves_per_eu(KB <= 16 ? 2 : 1))) void knn_feature_kernel(
    int n, int m, int c, int k, const float *__restrict__ feat1, const float *__restrict__ feat2, const float *__restrict__ sq1,
    const float *__restrict__ sq2, float *__restrict__ val, int *__restrict__ idx, rfi::Counts<RAGGED> lens) {
    const int bi = blockIdx.y;
    const int q0 = blockIdx.x * KF_TPB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = q0 + tid;  // the lane's query, once the halves have traded
    const int nv = rfi::count1(lens, bi, n), mv = rfi::count2(lens, bi, m);
    const int kv = RAGGED ? min(k, nv) : k;
    float *__restrict__ V = val + ((size_t)bi * m + min(j, m - 1)) * k;
    int *__restrict__ I = idx + ((size_t)bi * m + min(j, m - 1)) * k;
    if (RAGGED && q0 >= mv) {  // (workgroup-uniform) padded queries only
        if (j < m) kn_zero(0, k, V, I);
        return;
    }
    const float *__restrict__ F1 = feat1 + (size_t)bi * n * c;
    const float *__restrict__ F2 = feat2 + (size_t)bi * m * c;
    const float *__restrict__ S1 = sq1 + (size_t)bi * n;
    const float s2 = sq2[(size_t)bi * m + min(j, mv - 1)];

    __shared__ float sa[KF_TC * KF_LD];
    __shared__ float sb[KF_TPB * KF_LD];
    __shared__ float bd[KF_BUF][KF_TPB];
    __shared__ unsigned bx[KF_BUF][KF_TPB];

    u64 L[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) L[t] = t < KB - kv ? 0ull : ~0ull;
    float thr = __uint_as_float(0x7FC00000u);
    int cnt = 0;

    const int cp = (c + 1) & ~1;  // the channels up to the MFMA's K of 2
    const int half = lane >> 5;
    const float *pa = sa + (lane & 31) * KF_LD + half;
    const float *pb0 = sb + (wv * 64 + (lane & 31)) * KF_LD + half;
    const float *pb1 = pb0 + 32 * KF_LD;

    // Staging goes through registers one slab ahead: the loads of the next slab are in flight while this one is multiplied.
    // Thread t owns channel t & 31 of rows (t >> 5) + 4 i of a slab.  With a single slab (c <= KF_KS) the queries' slab is the
    // same for every tile and is staged once.
    constexpr int KF_RA = KF_TC * KF_KS / KF_TPB, KF_RB = KF_TPB * KF_KS / KF_TPB;
    const int nslab = (c + KF_KS - 1) / KF_KS;
    const int sch = tid & (KF_KS - 1), srow = tid / KF_KS;
    float ra[KF_RA], rb[KF_RB];
    auto fetch = [&](int i0, int c0, bool with_b) __attribute__((always_inline)) {
        // every load is unconditional at a clamped, valid address (straight-line code, nothing waits for it here); what lies
        // outside the sample's rows and channels is zeroed when the registers go to LDS
        const unsigned chc = (unsigned)min(c0 + sch, c - 1);
#pragma unroll
        for (int i = 0; i < KF_RA; i++)
            ra[i] = F1[(unsigned)min(i0 + srow + i * (KF_TPB / KF_KS), nv - 1) * (unsigned)c + chc];
        if (with_b) {
#pragma unroll
            for (int i = 0; i < KF_RB; i++)
                rb[i] = F2[(unsigned)min(q0 + srow + i * (KF_TPB / KF_KS), mv - 1) * (unsigned)c + chc];
        }
    };
    fetch(0, 0, true);
    for (int i0 = 0; i0 < nv; i0 += KF_TC) {
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; r++) acc0[r] = 0.f, acc1[r] = 0.f;
        // sq1 of the tile's 32 candidates, one per lane; the candidate of a step is read from its lane (v_readlane)
        const float s1v = S1[min(i0 + (lane & 31), nv - 1)];
        for (int sl = 0; sl < nslab; sl++) {
            const int c0 = sl * KF_KS;
            const bool with_b = nslab > 1 || i0 == 0;
            const bool chan = c0 + sch < c;
            __syncthreads();  // the slab before this one has been consumed
#pragma unroll
            for (int i = 0; i < KF_RA; i++) {
                const int r = srow + i * (KF_TPB / KF_KS);
                sa[r * KF_LD + sch] = (chan && i0 + r < nv) ? ra[i] : 0.f;
            }
            if (with_b) {
#pragma unroll
                for (int i = 0; i < KF_RB; i++) {
                    const int r = srow + i * (KF_TPB / KF_KS);
                    sb[r * KF_LD + sch] = (chan && q0 + r < mv) ? rb[i] : 0.f;
                }
            }
            __syncthreads();
            {  // the next slab's loads, to land while this one is multiplied
                const bool last = sl + 1 == nslab;
                const int ni = last ? i0 + KF_TC : i0, nc = last ? 0 : c0 + KF_KS;
                if (ni < nv) fetch(ni, nc, nslab > 1);
            }
            const int steps = min(KF_KS, cp - c0) >> 1;
            if (steps == KF_KS / 2) {
#pragma unroll 4
                for (int s = 0; s < KF_KS / 2; s++) {
                    const float a = pa[2 * s], b0 = pb0[2 * s], b1 = pb1[2 * s];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
                }
            } else {
                for (int s = 0; s < steps; s++) {
                    const float a = pa[2 * s], b0 = pb0[2 * s], b1 = pb1[2 * s];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
                }
            }
        }
        // the halves trade: afterwards acc0[r] is row (r & 3) + 8 (r >> 2) of the tile for THIS lane's query, acc1[r] row + 4
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float got = __shfl_xor(half ? acc0[r] : acc1[r], 32);
            if (half) acc0[r] = got;
            else acc1[r] = got;
        }
#pragma unroll
        for (int g = 0; g < KF_TC / KF_GROUP; g++) {
#pragma unroll
            for (int t = 0; t < KF_GROUP; t++) {
                const int row = g * KF_GROUP + t, ci = i0 + row;  // ascending: the index order
                const float ip = (t & 4) ? acc1[4 * g + (t & 3)] : acc0[4 * g + (t & 3)];
                if (ci < nv) {  // (uniform)
                    const float s1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(s1v), row));
                    const float d = fmaf(-2.f, ip, s2 + s1);
                    const bool in = !(d >= thr);
                    if (__ballot(in) != 0ull) {  // wave-uniform
                        if (in) {
                            bd[cnt][tid] = d;
                            bx[cnt][tid] = (unsigned)ci;
                            cnt++;
                        }
                    }
                }
            }
            if (__ballot(cnt > KF_BUF - KF_GROUP) != 0ull) kf_flush<KB>(L, cnt, thr, bd, bx, tid);
        }
    }
    kf_flush<KB>(L, cnt, thr, bd, bx, tid);
    if (j < mv) {
#pragma unroll
        for (int t = 0; t < KB; t++) {
            if (t >= KB - kv) {
                V[t - (KB - kv)] = kf_val(L[t]);
                I[t - (KB - kv)] = (int)(unsigned)L[t];
            }
        }
    }
    if (RAGGED && j < m) kn_zero(j < mv ? kv : 0, k, V, I);
}

bool kf_supported(int b, int n, int m, int c, int k) {
    return b >= 1 && b <= 65535 && n >= 1 && n <= 65536 && m >= 1 && m <= 65536 && c >= 1 && c <= KF_MAXC && k >= 1 &&
           k <= KN_MAXK && k <= n;
}
struct KfLayout {
    size_t sq1, sq2, total;  // the squared norms of feat1's rows, of feat2's
};
KfLayout kf_layout(int b, int n, int m) {
    rf::Layout w;
    const size_t sq1 = w.add((size_t)b * n * sizeof(float)), sq2 = w.add((size_t)b * m * sizeof(float));
    return {sq1, sq2, w.total};
}

}  // namespace

extern "C" {

size_t rf_knn_feature_workspace_bytes(int b, int n, int m, int c, int k) {
    if (!kf_supported(b, n, m, c, k)) return 0;
    return kf_layout(b, n, m).total;
}

int rf_knn_feature(int b, int n, int m, int c, int k, const float *feat1, const float *feat2, const int *len1, const int *len2,
                   float *val, int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (!kf_supported(b, n, m, c, k)) return RF_EINVAL;
    if (!rf::tensors_ok({feat1, feat2, val, idx}, {len1, len2}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const KfLayout l = kf_layout(b, n, m);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *sq1 = (float *)((char *)workspace + l.sq1);
    float *sq2 = (float *)((char *)workspace + l.sq2);
    const long rows1 = (long)b * n, rows2 = (long)b * m;
    RF_LAUNCH("knn_feature_sq", knn_feature_sq_kernel, dim3(rf::ceil_div(rows1 + rows2, KF_SQ_TPB)), dim3(KF_SQ_TPB), 0, s, rows1,
              rows2, c, feat1, feat2, sq1, sq2);
    const dim3 grid(rf::ceil_div(m, KF_TPB), b);
    if (len1 || len2) {
        const rfi::Counts<true> lens{len1, len2};
#define KF_GO(KB) \
    RF_LAUNCH("knn_feature", (knn_feature_kernel<KB, true>), grid, dim3(KF_TPB), 0, s, n, m, c, k, feat1, feat2, sq1, sq2, val, idx, lens)
        KN_DISPATCH(k, KF_GO);
#undef KF_GO
    } else {
#define KF_GO(KB)                                                                                                             \
    RF_LAUNCH("knn_feature", (knn_feature_kernel<KB, false>), grid, dim3(KF_TPB), 0, s, n, m, c, k, feat1, feat2, sq1, sq2, val, \
              idx, rfi::Counts<false>{})
        KN_DISPATCH(k, KF_GO);
#undef KF_GO
    }
    return RF_OK;
}

}  // extern "C"
