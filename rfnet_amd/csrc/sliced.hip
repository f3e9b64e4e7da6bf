// sliced.hip -- the sliced Wasserstein distance SW_2^2 of two clouds with exact gradients: both clouds are projected on
// nproj directions, each projection is sorted (in 1-D optimal transport IS sorting), the two quantile step functions are
// merged with exact integer weights (unequal and ragged counts need no approximation) and the per-direction costs are
// averaged.  include/rfops.h states the contract; DESIGN.md 5.3i the measurements.
//
//   sort        one workgroup per (direction of the chunk, sample, cloud): projections -> 64-bit words (monotone key << 32 |
//               original index) in LDS, a bitonic network over the power of two that holds the sample's count, up to four
//               strides per pass with up to 16 words per thread in registers; sorted values and original indices go to the
//               workspace.  The index in the low half makes every word distinct: ties go to the lower index, whatever the
//               network does.
//   merge       one workgroup per (direction of the chunk, sample): a thread owns ranks of a cloud and walks the ranks of the
//               other cloud its quantile interval meets; the weights are integers (the 1 / (L1 L2) is applied once), all sums
//               are double in a fixed order.  With gradients every point's scalar coefficient is written at its ORIGINAL index
//               (each cloud walks its own ranks: no scatter-add).
//   accumulate  per (sample, point): acc += coefficient * direction over the chunk's directions in order, in double; one thread
//               per sample adds the chunk's costs in order.  The last chunk's launch scales, rounds to fp32 once and writes +0
//               behind the counts.
//
// Directions are processed in chunks of RF_SW_DIR_CHUNK so that the workspace does not grow with nproj.  No atomics anywhere.
#include "common.hpp"
#include "lds_sort.hpp"  // sw_at, sw_sort: the bitonic network over LDS words

namespace {

constexpr int SW_CHUNK = RF_SW_DIR_CHUNK;
constexpr int SW_SORT_TPB = 1024;  // at most (sw_sort_threads, lds_sort.hpp)
constexpr int SW_TPB = 256;        // accumulate, and the merge of small clouds
constexpr int SW_MERGE_MAX = 1024; // the merge of large ones: its walks are chains of dependent loads, so waves hide them
constexpr unsigned long long SW_PAD = ~0ull;

// fp32 bits <-> uint32 that orders as the floats do (negative: all bits flipped, else the sign bit set)
__device__ __forceinline__ unsigned sw_key(float p) {
    const unsigned u = __float_as_uint(p);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float sw_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// ---- the sort --------------------------------------------------------------------------------------------------------------
// grid (directions of the chunk, b, 2).  Every loop bound is P (a power of two from the clamped count) or the count itself.
__global__ __launch_bounds__(SW_SORT_TPB) void sliced_sort_kernel(int b, int n, int m, const float *__restrict__ xyz1,
                                                                   const float *__restrict__ xyz2, const int *__restrict__ len1,
                                                                   const int *__restrict__ len2, const float *__restrict__ dirs,
                                                                   float *__restrict__ val1, float *__restrict__ val2,
                                                                   int *__restrict__ idx1, int *__restrict__ idx2) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sw_words[];  // [P]
    const int c = blockIdx.x, s = blockIdx.y, second = blockIdx.z;
    const int full = second ? m : n;
    const int L = rf::ragged_count(second ? len2 : len1, s, full);
    const float *__restrict__ xyz = (second ? xyz2 : xyz1) + (size_t)s * full * 3;
    const size_t row = ((size_t)c * b + s) * full;
    float *__restrict__ val = (second ? val2 : val1) + row;
    int *__restrict__ idx = (second ? idx2 : idx1) + row;
    const float tx = dirs[c * 3], ty = dirs[c * 3 + 1], tz = dirs[c * 3 + 2];
    int P = 64;
    while (P < L) P <<= 1;  // <= 16384: L <= RF_SW_MAX_POINTS
    const int tid = threadIdx.x, nt = blockDim.x;

    for (int r = tid; r < P; r += nt) {
        unsigned long long w = SW_PAD;
        if (r < L) {
            const float p = fmaf(xyz[r * 3 + 2], tz, fmaf(xyz[r * 3], tx, xyz[r * 3 + 1] * ty)) + 0.0f;  // -0 sorts as +0
            w = ((unsigned long long)sw_key(p) << 32) | (unsigned)r;
        }
        sw_words[sw_at(r)] = w;
    }
    __syncthreads();

    sw_sort(sw_words, P, tid, nt);

    // a valid word is below every padding word (its index is below 2^32 - 1): the first L words are the sample's points
    for (int r = tid; r < L; r += nt) {
        const unsigned long long w = sw_words[sw_at(r)];
        val[r] = sw_unkey((unsigned)(w >> 32));
        idx[r] = (int)(unsigned)w;
    }
}

// ---- the merge -------------------------------------------------------------------------------------------------------------
// Rank i of a cloud of Lo points owns the quantile interval [i Lx, (i + 1) Lx) in units of 1 / (Lo Lx); rank j of the other
// cloud (Lx points) owns [j Lo, (j + 1) Lo).  The sums of w d and w d^2 over the ranks j the interval meets, d = own - other,
// w the integer length of the intersection.  All products are below 2^28.
__device__ __forceinline__ void sw_walk(int i, int Lo, int Lx, float own, const float *__restrict__ other, double &s1,
                                        double &s2) {
    const int lo = i * Lx, hi = lo + Lx;
    const int j0 = lo / Lo, j1 = (hi + Lo - 1) / Lo;  // j1 <= Lx
    s1 = 0.0, s2 = 0.0;
    for (int j = j0; j < j1; j++) {
        const int a = max(lo, j * Lo), e = min(hi, (j + 1) * Lo);
        const double d = (double)own - (double)other[j], wd = (double)(e - a) * d;
        s1 += wd;
        s2 += wd * d;
    }
}

// grid (directions of the chunk, b)
__global__ __launch_bounds__(SW_MERGE_MAX) void sliced_merge_kernel(int b, int n, int m, const int *__restrict__ len1,
                                                              const int *__restrict__ len2, const float *__restrict__ val1,
                                                              const float *__restrict__ val2, const int *__restrict__ idx1,
                                                              const int *__restrict__ idx2, double *__restrict__ coef1,
                                                              double *__restrict__ coef2, double *__restrict__ cost) {
    __shared__ double wsum[SW_MERGE_MAX / 64];
    const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int L1 = rf::ragged_count(len1, s, n), L2 = rf::ragged_count(len2, s, m);
    const size_t row1 = ((size_t)c * b + s) * n, row2 = ((size_t)c * b + s) * m;
    const float *__restrict__ u = val1 + row1, *__restrict__ v = val2 + row2;
    const double den = (double)L1 * (double)L2;  // exact; applied once, as a division
    const bool grad = coef1 != nullptr;
    const bool from2 = L2 > L1;  // the cost from the walk of the larger cloud: at most two partners per rank
    double part = 0.0;
    if (grad || !from2)
        for (int i = tid; i < L1; i += nt) {
            double s1, s2;
            sw_walk(i, L1, L2, u[i], v, s1, s2);
            if (!from2) part += s2;
            if (grad) coef1[row1 + idx1[row1 + i]] = s1 / den;
        }
    if (grad || from2)
        for (int j = tid; j < L2; j += nt) {
            double s1, s2;
            sw_walk(j, L2, L1, v[j], u, s1, s2);
            if (from2) part += s2;
            if (grad) coef2[row2 + idx2[row2 + j]] = s1 / den;
        }
    // fixed order: butterfly inside the wave, then the waves in order
    part = rf::wave_sum(part);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
        for (int w = 1; w < (nt >> 6); w++) t += wsum[w];
        cost[(size_t)c * b + s] = t / den;
    }
}

// ---- accumulate and finish -------------------------------------------------------------------------------------------------
struct SwAcc {
    int b, n, m, nproj, d0, cc, first, last;
    const int *len1, *len2;
    const float *dirs;
    const double *coef1, *coef2, *cost;
    double *acc, *lacc;
    float *loss, *grad1, *grad2;
};

// grid (ceil((n + m) / SW_TPB) with gradients, else 1; b)
__global__ __launch_bounds__(SW_TPB) void sliced_accumulate_kernel(SwAcc a) {
    const int s = blockIdx.y, k = blockIdx.x * SW_TPB + threadIdx.x;
    if (a.grad1 && k < a.n + a.m) {
        const bool second = k >= a.n;
        const int kk = second ? k - a.n : k, full = second ? a.m : a.n;
        const int L = rf::ragged_count(second ? a.len2 : a.len1, s, full);
        float *__restrict__ g = (second ? a.grad2 : a.grad1) + ((size_t)s * full + kk) * 3;
        if (kk < L) {
            double *__restrict__ ac = a.acc + ((size_t)s * (a.n + a.m) + k) * 3;
            const double *__restrict__ co = (second ? a.coef2 : a.coef1) + (size_t)s * full + kk;
            double ax = 0.0, ay = 0.0, az = 0.0;
            if (!a.first) ax = ac[0], ay = ac[1], az = ac[2];
            for (int c = 0; c < a.cc; c++) {
                const double w = co[(size_t)c * a.b * full];
                const float *__restrict__ th = a.dirs + (size_t)(a.d0 + c) * 3;
                ax += w * (double)th[0];
                ay += w * (double)th[1];
                az += w * (double)th[2];
            }
            if (a.last) {
                const double np = (double)a.nproj;
                g[0] = (float)(2.0 * ax / np), g[1] = (float)(2.0 * ay / np), g[2] = (float)(2.0 * az / np);
            } else {
                ac[0] = ax, ac[1] = ay, ac[2] = az;
            }
        } else if (a.last) {
            g[0] = 0.f, g[1] = 0.f, g[2] = 0.f;
        }
    }
    if (k == 0) {
        double t = a.first ? 0.0 : a.lacc[s];
        for (int c = 0; c < a.cc; c++) t += a.cost[(size_t)c * a.b + s];
        if (a.last) a.loss[s] = (float)(t / (double)a.nproj);
        else a.lacc[s] = t;
    }
}

struct SwLayout {
    size_t val, idx, cost, lacc, coef, acc, total;
};

SwLayout sw_layout(int b, int n, int m, int nproj, int want_grad) {
    const size_t cc = nproj < SW_CHUNK ? nproj : SW_CHUNK, pts = (size_t)n + (size_t)m, rows = cc * (size_t)b;
    SwLayout l;
    l.val = 0;
    l.idx = l.val + rf::align256(rows * pts * sizeof(float));
    l.cost = l.idx + rf::align256(rows * pts * sizeof(int));
    l.lacc = l.cost + rf::align256(rows * sizeof(double));
    l.coef = l.lacc + rf::align256((size_t)b * sizeof(double));
    l.acc = l.coef + (want_grad ? rf::align256(rows * pts * sizeof(double)) : 0);
    l.total = l.acc + (want_grad ? rf::align256((size_t)b * pts * 3 * sizeof(double)) : 0);
    return l;
}

}  // namespace

extern "C" {

size_t rf_sliced_wasserstein_workspace_bytes(int b, int n, int m, int nproj, int want_grad) {
    if (b <= 0 || n <= 0 || m <= 0 || nproj <= 0 || n > RF_SW_MAX_POINTS || m > RF_SW_MAX_POINTS || b > 65535) return 0;
    return sw_layout(b, n, m, nproj, want_grad).total;
}

int rf_sliced_wasserstein(int b, int n, int m, int nproj, const float *xyz1, const float *xyz2, const int *len1,
                          const int *len2, const float *dirs, float *loss, float *grad1, float *grad2, void *workspace,
                          size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || nproj < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || m < 1 || nproj < 1 || n > RF_SW_MAX_POINTS || m > RF_SW_MAX_POINTS || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, dirs, loss}, {grad1, grad2, len1, len2}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if ((grad1 == nullptr) != (grad2 == nullptr)) return RF_EINVAL;
    const int want_grad = grad1 != nullptr;
    const SwLayout l = sw_layout(b, n, m, nproj, want_grad);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    // workspace: sorted values | original indices (one chunk, cloud 1 then cloud 2) | the chunk's costs | one double per
    // sample | with gradients: the chunk's coefficients | the accumulators (b, n + m, 3)
    char *w = (char *)workspace;
    const size_t cc_max = nproj < SW_CHUNK ? nproj : SW_CHUNK, rows = cc_max * (size_t)b;
    float *val1 = (float *)(w + l.val), *val2 = val1 + rows * n;
    int *idx1 = (int *)(w + l.idx), *idx2 = idx1 + rows * n;
    double *cost = (double *)(w + l.cost), *lacc = (double *)(w + l.lacc);
    double *coef1 = want_grad ? (double *)(w + l.coef) : nullptr, *coef2 = want_grad ? coef1 + rows * n : nullptr;
    double *acc = want_grad ? (double *)(w + l.acc) : nullptr;

    const int big = n > m ? n : m;
    int P = 64;
    while (P < big) P <<= 1;
    const int sort_tpb = sw_sort_threads(P);
    const int merge_tpb = big > 4096 ? SW_MERGE_MAX : SW_TPB;
    RF_HIP(hipFuncSetAttribute((const void *)sliced_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    for (int d0 = 0; d0 < nproj; d0 += SW_CHUNK) {
        const int cc = nproj - d0 < SW_CHUNK ? nproj - d0 : SW_CHUNK;
        RF_LAUNCH("sliced_sort", sliced_sort_kernel, dim3(cc, b, 2), dim3(sort_tpb), (size_t)P * sizeof(unsigned long long),
                  st, b, n, m, xyz1, xyz2, len1, len2, dirs + (size_t)d0 * 3, val1, val2, idx1, idx2);
        RF_LAUNCH("sliced_merge", sliced_merge_kernel, dim3(cc, b), dim3(merge_tpb), 0, st, b, n, m, len1, len2, val1, val2, idx1,
                  idx2, coef1, coef2, cost);
        const SwAcc a{b,    n,     m,     nproj, d0,   cc,   d0 == 0, d0 + cc == nproj, len1,  len2,
                      dirs, coef1, coef2, cost,  acc,  lacc, loss,    grad1,            grad2};
        RF_LAUNCH("sliced_accumulate", sliced_accumulate_kernel, dim3(want_grad ? rf::ceil_div((long)n + m, SW_TPB) : 1, b),
                  dim3(SW_TPB), 0, st, a);
    }
    return RF_OK;
}

}  // extern "C"
