// chamfer_metrics.hip -- what a completion result is judged by, in one call on the Chamfer sweep's outputs:
// the two halves of CD-L1 and CD-L2, the squared directed Hausdorff distances, precision / recall / F-score at a
// threshold, and the density-aware Chamfer distance (DCD), next to the per-point counts DCD needs
// ("how many queries chose this point").  include/rfops.h states the contract; DESIGN.md 5.3g the measurements.
//
//   rf_nn_metrics            the epilogue alone, on nn_distance outputs the caller already holds
//   rf_chamfer_metrics       rf_nn_distance_lengths (RF_NN_AUTO, both directions) + the epilogue
//   rf_chamfer_metrics_grad  backward of columns 0-3, 9, 10: one elementwise kernel forms the per-point upstream
//                            gradients of dist1 / dist2, then NnDistanceGrad as it is (nn_distance.hip)
//
// The epilogue is one workgroup per (sample, direction): a histogram of the direction's idx over the other cloud's
// points with integer atomics (LDS when the bins fit, the zeroed count array in global memory otherwise), then the
// reductions with the counts gathered at idx.  Integer adds make the counts exact and order-free; every float sum
// takes chamfer_loss_reduce_kernel's fixed order (strided per-thread partials, the wave, waves in order), so two
// calls return the same bits.  No float atomics.
#include <initializer_list>

#include "common.hpp"
#include "nn_dense.hpp"

namespace {

constexpr int CM_TPB = 1024;
constexpr int CM_NW = CM_TPB / 64;
constexpr int CM_U = 8;  // points per thread and trip
// Bins (points of the other cloud) one workgroup's LDS histogram holds: 32768 ints = 128 KiB of the CU's 160 KiB.
// A direction with more bins counts with global atomics into its count array.  tests/test_gpu_chamfer_metrics.py
// cites this number for the shapes on either side of it.
constexpr int CM_LDS_BINS = 32768;

struct CmArgs {
    int n, m;
    float *dist1, *dist2;  // written only behind the counts, and only with `pad`
    int *idx1, *idx2;
    const int *len1, *len2;
    float thr2, alpha;
    float *metrics;
    int *count1, *count2;
    int pad;  // the culled sweep leaves the padded slots of dist / idx to this kernel: (0, -1)
};

// LDS_HIST: the histogram lives in `hist` (LDS, zeroed here); otherwise `hist` is the sample's row of the count
// array in global memory, zeroed by the host side before the launch, written with atomics that execute at L2 and
// read back with loads of the same scope (this workgroup is the row's only writer; the plain-load path through the
// CU's L1 is never used for it).  A stored index outside [0, nb) -- the sweeps never leave one in a valid slot, a
// caller of rf_nn_metrics might -- is not counted and weighs as a count of 1.
template <bool LDS_HIST>
__device__ __forceinline__ void cm_direction(const CmArgs &a, int bi, int dir, int *hist) {
    __shared__ float part[3][CM_NW];
    __shared__ float part_max[CM_NW];
    __shared__ int part_cnt[2][CM_NW];
    const int tid = threadIdx.x;
    const int full = dir ? a.m : a.n;  // this direction's points
    const int nb = dir ? a.n : a.m;    // its bins: the other cloud's points
    float *__restrict__ dfull = (dir ? a.dist2 : a.dist1) + (size_t)bi * full;
    int *__restrict__ ifull = (dir ? a.idx2 : a.idx1) + (size_t)bi * full;
    const float *__restrict__ d = dfull;
    const int *__restrict__ ix = ifull;
    const int L = rf::ragged_count(dir ? a.len2 : a.len1, bi, full);
    int *__restrict__ cnt_out = (dir ? a.count1 : a.count2) + (size_t)bi * nb;

    if (a.pad) {
        for (int k = L + tid; k < full; k += CM_TPB) {
            dfull[k] = 0.f;
            ifull[k] = -1;
        }
    }
    if constexpr (LDS_HIST) {  // (the dynamic LDS is sized to a multiple of four bins)
        int4 *__restrict__ h4 = reinterpret_cast<int4 *>(hist);
        for (int k = tid; k < (nb + 3) / 4; k += CM_TPB) h4[k] = make_int4(0, 0, 0, 0);
        __syncthreads();
    }
    // Pass 1: the histogram.  CM_U loads of a trip are in flight together (predicated, so that a tail costs no trips of
    // its own).  With one load per trip this pass is a chain of 16 dependent memory round trips at 16384 points: that
    // form of the kernel took 20.7 us at 32 x 16384^2, this one 17.0 (profiles/metrics_ab.txt).
    // Column 8 needs both directions' counts below the threshold.  They are integers, so direction 1's workgroup counts
    // direction 2's as well -- its loads ride in the same trips -- and gets exactly the number its neighbour workgroup
    // does: no second launch, nothing to order between workgroups.
    const float thr2 = a.thr2, nalpha = -a.alpha;
    const int Lo = rf::ragged_count(dir ? a.len1 : a.len2, bi, nb);
    const int Lr = dir == 0 ? Lo : 0;
    const float *__restrict__ dother = a.dist2 + (size_t)bi * a.m;  // read by direction 1's workgroup only
    int below_o = 0;
    for (int j = tid; j < (L > Lr ? L : Lr); j += CM_U * CM_TPB) {
        int k[CM_U];
        float w[CM_U];
#pragma unroll
        for (int u = 0; u < CM_U; u++) {
            const int jj = j + u * CM_TPB;
            k[u] = jj < L ? ix[jj] : -1;
            w[u] = jj < Lr ? dother[jj] : INFINITY;  // never below a threshold
        }
#pragma unroll
        for (int u = 0; u < CM_U; u++) {
            if ((unsigned)k[u] < (unsigned)nb) atomicAdd(&hist[k[u]], 1);
            below_o += w[u] < thr2;
        }
    }
    if constexpr (!LDS_HIST) __threadfence();
    __syncthreads();

    auto count_at = [&](int k) -> float {
        int c = 1;
        if ((unsigned)k < (unsigned)nb) {
            if constexpr (LDS_HIST) c = hist[k];
            else c = __hip_atomic_load(hist + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return (float)(c < 1 ? 1 : c);
    };
    // Pass 2: the reductions, CM_U points per trip into four independent partial sums per quantity and thread (as in
    // chamfer_loss_reduce_kernel): the loads of a trip (dist, idx, then the count at idx) are in flight together.  A
    // predicated-off slot contributes sqrt(0) = 0, 0, 1 - e^0 / 1 = 0 and max(., 0): nothing, exactly.
    float r[4] = {0.f, 0.f, 0.f, 0.f};  // sqrt(dist)
    float q[4] = {0.f, 0.f, 0.f, 0.f};  // dist
    float e[4] = {0.f, 0.f, 0.f, 0.f};  // 1 - exp(-alpha dist) / count
    float mx = 0.f;                     // distances are >= 0 and a sample has at least one point
    int below = 0;
    for (int j = tid; j < L; j += CM_U * CM_TPB) {
        float v[CM_U], c[CM_U];
        int k[CM_U];
#pragma unroll
        for (int u = 0; u < CM_U; u++) {
            const int jj = j + u * CM_TPB;
            v[u] = jj < L ? d[jj] : 0.f;
            k[u] = jj < L ? ix[jj] : -1;
        }
#pragma unroll
        for (int u = 0; u < CM_U; u++) c[u] = count_at(k[u]);
#pragma unroll
        for (int u = 0; u < CM_U; u++) {
            r[u & 3] += sqrtf(v[u]);
            q[u & 3] += v[u];
            e[u & 3] += 1.f - expf(nalpha * v[u]) / c[u];
            mx = fmaxf(mx, v[u]);
            below += (j + u * CM_TPB < L) & (v[u] < thr2);
        }
    }
    if constexpr (LDS_HIST) {
        for (int k = tid; k < nb; k += CM_TPB) cnt_out[k] = hist[k];
    }

    auto add = [](auto x, auto y) { return x + y; };
    const float sr = rf::wave_reduce((r[0] + r[1]) + (r[2] + r[3]), add);
    const float sq = rf::wave_reduce((q[0] + q[1]) + (q[2] + q[3]), add);
    const float se = rf::wave_reduce((e[0] + e[1]) + (e[2] + e[3]), add);
    mx = rf::wave_reduce(mx, [](float x, float y) { return fmaxf(x, y); });
    below = rf::wave_reduce(below, add);
    below_o = rf::wave_reduce(below_o, add);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        part[0][w] = sr;
        part[1][w] = sq;
        part[2][w] = se;
        part_max[w] = mx;
        part_cnt[0][w] = below;
        part_cnt[1][w] = below_o;
    }
    __syncthreads();
    if (tid == 0) {
        float t0 = part[0][0], t1 = part[1][0], t2 = part[2][0], tm = part_max[0];
        int nb0 = part_cnt[0][0], nb1 = part_cnt[1][0];
#pragma unroll
        for (int w = 1; w < CM_NW; w++) {
            t0 += part[0][w];
            t1 += part[1][w];
            t2 += part[2][w];
            tm = fmaxf(tm, part_max[w]);
            nb0 += part_cnt[0][w];
            nb1 += part_cnt[1][w];
        }
        float *__restrict__ M = a.metrics + (size_t)bi * RF_CM_NCOL;
        const float fl = (float)L;
        const float frac = (float)nb0 / fl;
        M[0 + dir] = t0 / fl;
        M[2 + dir] = t1 / fl;
        M[4 + dir] = tm;
        M[6 + dir] = frac;
        M[9 + dir] = t2 / fl;
        if (dir == 0) {
            const float frac_o = (float)nb1 / (float)Lo;
            const float s = frac + frac_o;
            M[8] = s == 0.f ? 0.f : 2.f * frac * frac_o / s;
        }
    }
}

__global__ __launch_bounds__(CM_TPB) void chamfer_metrics_kernel(CmArgs a) {
    extern __shared__ __attribute__((aligned(16))) int cm_hist[];  // [bins of the larger direction that fits, rounded up to 4]
    const int bi = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const int nb = dir ? a.n : a.m;
    if (nb <= CM_LDS_BINS) {
        cm_direction<true>(a, bi, dir, cm_hist);
    } else {
        cm_direction<false>(a, bi, dir, (dir ? a.count1 : a.count2) + (size_t)bi * nb);
    }
}

// gd_d[i][j], the upstream gradient of dist_d[i][j] (rfops.h): the three differentiable pairs of columns.  A term whose
// upstream value is exactly 0 is not formed, so a zero distance cannot turn 0 * inf into NaN when only DCD is trained.
// Slots behind a count get 0 (NnDistanceGrad does not read them).
__global__ void chamfer_metrics_gradw_kernel(int b, int n, int m, const int *__restrict__ len1,
                                             const int *__restrict__ len2, const float *__restrict__ dist1,
                                             const int *__restrict__ idx1, const float *__restrict__ dist2,
                                             const int *__restrict__ idx2, const int *__restrict__ count1,
                                             const int *__restrict__ count2, float alpha,
                                             const float *__restrict__ gm, float *__restrict__ gd1,
                                             float *__restrict__ gd2) {
    long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long t1 = (long)b * n;
    const int dir = g >= t1 ? 1 : 0;
    if (dir) g -= t1;
    const int full = dir ? m : n, nb = dir ? n : m;
    if (g >= (long)b * full) return;
    const int bi = (int)(g / full);
    float *__restrict__ out = dir ? gd2 : gd1;
    const int L = rf::ragged_count(dir ? len2 : len1, bi, full);
    if ((int)(g - (long)bi * full) >= L) {
        out[g] = 0.f;
        return;
    }
    const float v = (dir ? dist2 : dist1)[g];
    const float *__restrict__ u = gm + (size_t)bi * RF_CM_NCOL;
    const float u_l1 = u[0 + dir], u_l2 = u[2 + dir], u_dcd = u[9 + dir];
    const float fl = (float)L;
    float r = 0.f;
    if (u_l1 != 0.f) r += u_l1 * 0.5f / (fl * sqrtf(v));
    if (u_l2 != 0.f) r += u_l2 / fl;
    if (u_dcd != 0.f) {
        const int k = (dir ? idx2 : idx1)[g];
        int c = 1;
        if ((unsigned)k < (unsigned)nb) c = (dir ? count1 : count2)[(size_t)bi * nb + k];
        r += u_dcd * alpha * expf(-alpha * v) / ((float)(c < 1 ? 1 : c) * fl);
    }
    out[g] = r;
}

// the argument rules shared by the three entries (all before any HIP call); RF_OK with b == 0 is the caller's
int cm_check(int b, int n, int m, const int *len1, const int *len2, const void *workspace, float alpha) {
    if (b < 0 || n < 1 || m < 1 || b > 65535) return RF_EINVAL;
    if (!rf::workspace_ok(workspace) || !rf::all_aligned4({len1, len2})) return RF_EINVAL;
    if (!(alpha >= 0.f) || !isfinite(alpha)) return RF_EINVAL;
    return RF_OK;
}

int cm_epilogue(int b, int n, int m, float *dist1, int *idx1, float *dist2, int *idx2, const int *len1, const int *len2,
                float thr2, float alpha, float *metrics, int *count1, int *count2, int pad, hipStream_t s) {
    // a direction whose bins do not fit the LDS counts in global memory: its count array starts from zero
    if (n > CM_LDS_BINS) RF_ZERO(count1, sizeof(int) * (size_t)b * n, s);
    if (m > CM_LDS_BINS) RF_ZERO(count2, sizeof(int) * (size_t)b * m, s);
    // dynamic LDS: the larger of the directions whose bins fit (count1 has n bins, count2 m).  Both beyond the cap: no
    // LDS histogram at all, both directions count in global memory.
    const int fit1 = n <= CM_LDS_BINS ? n : 0, fit2 = m <= CM_LDS_BINS ? m : 0;
    const int lds_bins = fit1 > fit2 ? fit1 : fit2;
    const CmArgs a{n, m, dist1, dist2, idx1, idx2, len1, len2, thr2, alpha, metrics, count1, count2, pad};
    RF_HIP(hipFuncSetAttribute((const void *)chamfer_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               CM_LDS_BINS * (int)sizeof(int)));
    RF_LAUNCH("chamfer_metrics_epilogue", chamfer_metrics_kernel, dim3(2 * b), dim3(CM_TPB),
              sizeof(int) * (size_t)((lds_bins + 3) / 4 * 4), s, a);
    return RF_OK;
}

// rf_chamfer_metrics_grad's workspace: the per-point weights of the two directions, which nn_distance_grad then scatters
struct CmGradLayout {
    size_t gd1, gd2, total;
};
CmGradLayout cm_grad_layout(int b, int n, int m) {
    rf::Layout w;
    const size_t gd1 = w.add(sizeof(float) * (size_t)b * n), gd2 = w.add(sizeof(float) * (size_t)b * m);
    return {gd1, gd2, w.total};
}

}  // namespace

extern "C" {

// The epilogue's workspace is currently UNUSED: one workgroup per (sample, direction) needs no scratch.  The size is one
// 256-byte unit (positive, as every _workspace_bytes of the section is for positive sizes) and the pointer rules are
// checked, so that a caller written against this contract keeps working if a sample is ever split over workgroups.
size_t rf_nn_metrics_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return 256;
}

int rf_nn_metrics(int b, int n, int m, const float *dist1, const int *idx1, const float *dist2, const int *idx2,
                  const int *len1, const int *len2, float thr2, float alpha, float *metrics, int *count1, int *count2,
                  void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b == 0) return RF_OK;
    if (int e = cm_check(b, n, m, len1, len2, workspace, alpha)) return e;
    if (!(thr2 >= 0.f)) return RF_EINVAL;  // NaN or negative; +inf is "every point"
    if (!rf::tensors_ok({dist1, idx1, dist2, idx2, metrics, count1, count2})) return RF_EINVAL;
    if (workspace_bytes < rf_nn_metrics_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    // (pad = 0: nothing is written through the const inputs)
    return cm_epilogue(b, n, m, const_cast<float *>(dist1), const_cast<int *>(idx1), const_cast<float *>(dist2),
                       const_cast<int *>(idx2), len1, len2, thr2, alpha, metrics, count1, count2, 0,
                       (hipStream_t)stream);
}

size_t rf_chamfer_metrics_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return rfd::ragged_workspace_bytes(b, n, m, RF_NN_AUTO, 3);
}

int rf_chamfer_metrics(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                       float thr2, float alpha, float *metrics, float *dist1, int *idx1, float *dist2, int *idx2,
                       int *count1, int *count2, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b == 0) return RF_OK;
    if (int e = cm_check(b, n, m, len1, len2, workspace, alpha)) return e;
    if (!(thr2 >= 0.f)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, dist1, idx1, dist2, idx2, metrics, count1, count2})) return RF_EINVAL;
    if (workspace_bytes < rf_chamfer_metrics_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // the culled route leaves the padded slots to the epilogue (the dense sweep writes them itself)
    const bool culled = rfd::resolve_mode(b, n, m, RF_NN_AUTO) == RF_NN_CULLED;
    if (int e = rfd::ragged_nn_distance(b, n, m, xyz1, xyz2, len1, len2, dist1, idx1, dist2, idx2, workspace,
                                        workspace_bytes, s, RF_NN_AUTO, 3, !culled))
        return e;
    return cm_epilogue(b, n, m, dist1, idx1, dist2, idx2, len1, len2, thr2, alpha, metrics, count1, count2,
                       culled ? 1 : 0, s);
}

size_t rf_chamfer_metrics_grad_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return cm_grad_layout(b, n, m).total;
}

int rf_chamfer_metrics_grad(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                            const float *dist1, const int *idx1, const float *dist2, const int *idx2, const int *count1,
                            const int *count2, float alpha, const float *grad_metrics, float *grad_xyz1,
                            float *grad_xyz2, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b == 0) return RF_OK;
    if (int e = cm_check(b, n, m, len1, len2, workspace, alpha)) return e;
    if (!rf::tensors_ok({xyz1, xyz2, dist1, idx1, dist2, idx2, count1, count2, grad_metrics, grad_xyz1, grad_xyz2}))
        return RF_EINVAL;
    const CmGradLayout l = cm_grad_layout(b, n, m);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *gd1 = (float *)((char *)workspace + l.gd1);
    float *gd2 = (float *)((char *)workspace + l.gd2);
    const long total = (long)b * n + (long)b * m;
    RF_LAUNCH("chamfer_metrics_gradw", chamfer_metrics_gradw_kernel, dim3(rf::ceil_div(total, 256)), dim3(256), 0, s, b,
              n, m, len1, len2, dist1, idx1, dist2, idx2, count1, count2, alpha, grad_metrics, gd1, gd2);
    const rfd::GradSource g{gd1, gd2, nullptr, nullptr, nullptr};
    return rfd::nn_distance_grad(b, n, m, xyz1, xyz2, g, idx1, idx2, grad_xyz1, grad_xyz2, s, len1, len2);
}

}  // extern "C"
