// chamfer_ext.hip -- composite Chamfer entry points for gfx950: what the reference's loss / geometry
// glue (vv_recon.py:132-139 merge_layer, :381-390 chamfer_big / fidelity_loss, :414-419
// zero_groupnear) builds out of nn_distance + a handful of TensorFlow elementwise ops, as single
// calls into the library, plus the pieces a caller needs to stop paying twice for the same work:
//
//   rf_nn_distance_dir      one direction only (merge_layer uses idx2 alone, fidelity_loss dist1,
//                           zero_groupnear dist2): the other direction's half of the culled grid is
//                           not launched / the column half of the dense sweep is compiled out.
//   rf_nn_sort + rf_nn_distance_sorted
//                           a cloud that takes part in several Chamfers of a step (the model
//                           Chamfers `pointcloud` 3x and `gt` 5x per training step) is put in
//                           Hilbert order ONCE; the handle is a caller-owned buffer whose layout is
//                           a pure function of (b, n) -- no state in the library.
//   rf_chamfer_step         forward + backward of one Chamfer in one call on caller-owned buffers
//                           (the host path of a training step: one FFI crossing, no allocation).
//   rf_chamfer_loss(+grad)  per-sample mean of sqrt(dist) both ways (chamfer_big / fidelity_loss)
//                           with the 0.5/sqrt(d)/N backward folded into the scatter kernel.
//   rf_merge_layer(+grad)   direction-2 Chamfer + gather of the winner + Gaussian pull.
//
// The arithmetic of the Chamfer itself is the sweeps' (bit-exact dist / idx); the glue arithmetic
// follows the TensorFlow graph's expression order (unfused products and sums) and is held to the
// glue tolerance (rel 1e-5) against a numpy restatement of the reference's glue in the tests.
#include <type_traits>

#include "common.hpp"
#include "nn_dense.hpp"
#include "nn_pruned.hpp"

namespace {

// Sum of acc over a workgroup of TPB threads, valid in thread 0 only: the butterfly inside each wave, then thread 0 adds the
// waves' sums in ascending order -- a fixed order, so the float result is deterministic.
template <int TPB>
__device__ __forceinline__ float block_sum(float acc) {
    __shared__ float part[TPB / 64];
    acc = rf::wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
        t = part[0];
#pragma unroll
        for (int w = 1; w < TPB / 64; w++) t += part[w];
    }
    return t;
}

// loss[bi][dir] = mean_j sqrt(dist_dir[bi][j]): one workgroup per (sample, direction), fixed
// summation order (strided per-thread partials, DPP inside the wave, waves in order): deterministic.
// PER_SAMPLE (rf_chamfer_loss_lengths): the mean over the sample's own count (len1 / len2, NULL = all,
// clamped into [1, n] as in nn_distance.hip), in the order the sample alone would take.  pad_d* / pad_i*
// (PER_SAMPLE, may be NULL): the same rows' outputs, whose slots beyond the count get (0, -1) here -- on
// the culled route this replaces a launch of its own (nn_distance.hip pad_outputs_kernel).
constexpr int LR_TPB = 1024;
template <int PER_SAMPLE>
__global__ __launch_bounds__(LR_TPB) void chamfer_loss_reduce_kernel(int n, int m, const float *__restrict__ dist1,
                                                                     const float *__restrict__ dist2,
                                                                     float *__restrict__ loss,
                                                                     const int *__restrict__ len1,
                                                                     const int *__restrict__ len2,
                                                                     float *__restrict__ pad_d1, int *__restrict__ pad_i1,
                                                                     float *__restrict__ pad_d2,
                                                                     int *__restrict__ pad_i2) {
    const int bi = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const float *__restrict__ d = dir ? dist2 : dist1;
    int cnt = dir ? m : n;
    if (!d) {  // direction not computed
        if (threadIdx.x == 0) loss[bi * 2 + dir] = 0.f;
        return;
    }
    d += (size_t)bi * cnt;
    if constexpr (PER_SAMPLE != 0) {
        const int *__restrict__ len = dir ? len2 : len1;
        const int full = cnt;
        if (len) cnt = len[bi] < 1 ? 1 : (len[bi] > cnt ? cnt : len[bi]);
        float *__restrict__ pd = dir ? pad_d2 : pad_d1;
        int *__restrict__ pi = dir ? pad_i2 : pad_i1;
        if (pd) {
            for (int k = cnt + threadIdx.x; k < full; k += LR_TPB) {
                pd[(size_t)bi * full + k] = 0.f;
                pi[(size_t)bi * full + k] = -1;
            }
        }
    }
    // four independent partial sums per thread: the loads of a trip are all in flight together (one
    // running sum per thread made every trip wait a full memory latency: 22 us at 16384 points)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int j = threadIdx.x;
    for (; j + 3 * LR_TPB < cnt; j += 4 * LR_TPB) {
        const float v0 = d[j], v1 = d[j + LR_TPB], v2 = d[j + 2 * LR_TPB], v3 = d[j + 3 * LR_TPB];
        a0 += sqrtf(v0); a1 += sqrtf(v1); a2 += sqrtf(v2); a3 += sqrtf(v3);
    }
    for (; j < cnt; j += LR_TPB) a0 += sqrtf(d[j]);
    const float t = block_sum<LR_TPB>((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) loss[bi * 2 + dir] = t / (float)cnt;
}

// merge_layer's tail (vv_recon.py:135-138): g = raw[idx2]; diff = g - q;
// ratio = exp(-sum(diff^2) / (1e-8 + dec^2)); out = q + ratio * diff.  TensorFlow's expression
// order, nothing contracted (the file is compiled with -ffp-contract=off).
// RAGGED (rf_merge_layer_lengths / rf_merge_layer_grad_lengths, here and in the backward below): sample bi has len_raw[bi] raw
// points and len_new[bi] new points (device counts, clamped into [1, n] / [1, m] here; NULL = all).  Valid new rows get the
// dense arithmetic; a padded new row gets idx2 = 0 and refined = +0.0 whatever the sweep left in its slot ((0, -1) on the
// dense route, nothing on the culled one), so that gathers downstream need no special case.  Only that form writes idx2.
template <bool RAGGED>
__global__ void merge_pull_kernel(int n, int m, long total, const float *__restrict__ raw,
                                  const float *__restrict__ newpts,
                                  std::conditional_t<RAGGED, int, const int> *__restrict__ idx2,
                                  const float *__restrict__ decfactor, float *__restrict__ out,
                                  const int *__restrict__ len_new) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long bi = e / m;
    if constexpr (RAGGED) {
        if ((int)(e - bi * m) >= rf::ragged_count(len_new, (int)bi, m)) {
            idx2[e] = 0;
            out[e * 3 + 0] = 0.f;
            out[e * 3 + 1] = 0.f;
            out[e * 3 + 2] = 0.f;
            return;
        }
    }
    const float dec = decfactor[0];
    const float c = 1e-8f + dec * dec;
    const float *g = raw + (bi * n + idx2[e]) * 3;
    const float qx = newpts[e * 3 + 0], qy = newpts[e * 3 + 1], qz = newpts[e * 3 + 2];
    const float dx = g[0] - qx, dy = g[1] - qy, dz = g[2] - qz;
    const float s = (dx * dx + dy * dy) + dz * dz;
    const float ratio = expf(-s / c);
    out[e * 3 + 0] = qx + ratio * dx;
    out[e * 3 + 1] = qy + ratio * dy;
    out[e * 3 + 2] = qz + ratio * dz;
}

// Backward of the tail for one sample per workgroup: with go the upstream gradient of `out`,
//   g_ratio = go . diff;  g_diff = ratio * go - (2 ratio g_ratio / c) diff
//   grad_newpts = go - g_diff;   grad_raw[idx2] += g_diff  (optional, atomics on a zero-filled buffer)
//   grad_dec[bi] = sum_points g_ratio * ratio * s / c^2 * 2 dec     (fixed order: deterministic)
// idx2 carries no gradient (NnDistance's index outputs have none, tf_nndistance.py:26-32).
// RAGGED: the same strided loop and the same reduction over the sample's len_new valid rows (the order the dense form takes on
// that slice alone); padded rows get grad_newpts = 0 without their grad_out or idx2 being read.  A stored index is held inside
// [0, len_raw) before it addresses raw / grad_raw (the forward never leaves one outside), so grad_raw stays 0 behind the count
// whatever the caller kept in idx2.
constexpr int MG_TPB = 1024;
template <bool RAGGED>
__global__ __launch_bounds__(MG_TPB) void merge_pull_grad_kernel(int n, int m, const float *__restrict__ raw,
                                                                 const float *__restrict__ newpts,
                                                                 const int *__restrict__ idx2,
                                                                 const float *__restrict__ decfactor,
                                                                 const float *__restrict__ grad_out,
                                                                 float *__restrict__ grad_newpts,
                                                                 float *__restrict__ grad_dec,
                                                                 float *__restrict__ grad_raw,
                                                                 const int *__restrict__ len_raw,
                                                                 const int *__restrict__ len_new) {
    const int bi = blockIdx.x;
    int nl = n, ml = m;
    if constexpr (RAGGED) {
        nl = rf::ragged_count(len_raw, bi, n);
        ml = rf::ragged_count(len_new, bi, m);
    }
    const float dec = decfactor[0];
    const float c = 1e-8f + dec * dec;
    float acc = 0.f;
    for (int j = threadIdx.x; j < ml; j += MG_TPB) {
        const size_t e = (size_t)bi * m + j;
        int k = idx2[e];
        if constexpr (RAGGED) k = k < 0 ? 0 : (k >= nl ? nl - 1 : k);
        const float *g = raw + ((size_t)bi * n + k) * 3;
        const float qx = newpts[e * 3 + 0], qy = newpts[e * 3 + 1], qz = newpts[e * 3 + 2];
        const float dx = g[0] - qx, dy = g[1] - qy, dz = g[2] - qz;
        const float s = (dx * dx + dy * dy) + dz * dz;
        const float ratio = expf(-s / c);
        const float gx = grad_out[e * 3 + 0], gy = grad_out[e * 3 + 1], gz = grad_out[e * 3 + 2];
        const float g_ratio = (gx * dx + gy * dy) + gz * dz;
        const float k2 = 2.f * ratio * g_ratio / c;
        const float fx = ratio * gx - k2 * dx, fy = ratio * gy - k2 * dy, fz = ratio * gz - k2 * dz;
        grad_newpts[e * 3 + 0] = gx - fx;
        grad_newpts[e * 3 + 1] = gy - fy;
        grad_newpts[e * 3 + 2] = gz - fz;
        if (grad_raw) {
            float *gr = grad_raw + ((size_t)bi * n + k) * 3;
            atomicAdd(gr + 0, fx);
            atomicAdd(gr + 1, fy);
            atomicAdd(gr + 2, fz);
        }
        acc += g_ratio * ratio * s / (c * c);
    }
    if constexpr (RAGGED) {
        for (int j = ml * 3 + threadIdx.x; j < m * 3; j += MG_TPB) grad_newpts[(size_t)bi * m * 3 + j] = 0.f;
    }
    const float t = block_sum<MG_TPB>(acc);
    if (threadIdx.x == 0) grad_dec[bi] = t * (2.f * dec);
}

int dirs_of(int want1, int want2) { return (want1 ? 1 : 0) | (want2 ? 2 : 0); }

// Forward with optional sorted handles.  Culled when both handles are supplied or when the size rule
// says so (a missing handle is then sorted into the workspace), dense otherwise.
struct FwdPlan {
    bool culled;
    size_t off_s1, off_s2, off_dense, bytes;  // workspace regions
};
FwdPlan plan_forward(int b, int n, int m, int dirs, bool have1, bool have2) {
    FwdPlan p{};
    const bool can = rfp::pruned_supported(b, n, m);
    p.culled = can && ((have1 && have2) || rfd::resolve_mode(b, n, m, RF_NN_AUTO) == RF_NN_CULLED);
    size_t off = 0;
    if (p.culled) {
        p.off_s1 = off;
        if (!have1) off += rf::align256(rfp::sorted_bytes(b, n));
        p.off_s2 = off;
        if (!have2) off += rf::align256(rfp::sorted_bytes(b, m));
    } else {
        p.off_dense = off;
        off += rf::align256(rfd::dense_workspace_bytes(b, n, m, dirs));
    }
    p.bytes = off;
    return p;
}

int run_forward(int b, int n, int m, const float *xyz1, const float *xyz2, const void *sorted1, const void *sorted2,
                float *dist1, int *idx1, float *dist2, int *idx2, int dirs, void *workspace, size_t workspace_bytes,
                hipStream_t s) {
    const FwdPlan p = plan_forward(b, n, m, dirs, sorted1 != nullptr, sorted2 != nullptr);
    if (workspace_bytes < p.bytes || (p.bytes && !workspace)) return RF_EWORKSPACE;
    if (!rf::all_aligned16({workspace, sorted1, sorted2})) return RF_EINVAL;
    char *w = (char *)workspace;
    if (!p.culled)
        return rfd::dense_nn_distance(b, n, m, xyz1, xyz2, dist1, idx1, dist2, idx2, w + p.off_dense,
                                      workspace_bytes - p.off_dense, s, dirs);
    const rfp::Sorted s1 = rfp::sorted_view(b, n, sorted1 ? sorted1 : w + p.off_s1);
    const rfp::Sorted s2 = rfp::sorted_view(b, m, sorted2 ? sorted2 : w + p.off_s2);
    if (int e = rfp::sort_missing(b, n, m, xyz1, xyz2, s1, s2, sorted1 != nullptr, sorted2 != nullptr, s)) return e;
    return rfp::sweep_sorted(b, n, m, s1, s2, dist1, idx1, dist2, idx2, dirs, s, nullptr);
}

bool bad_sizes(int b, int n, int m) { return b < 0 || n < 0 || m < 0; }

// merge_layer's workspace starts with the b * m distances of direction 2 (they are not an output); the sweep's own follows
size_t merge_dist_bytes(int b, int m) { return rf::align256((size_t)b * m * sizeof(float)); }

// the tail of both merge_layer entries, once the sweep has left idx2
template <bool RAGGED>
int merge_pull(const char *name, int b, int n, int m, const float *rawpts, const float *newpts, int *idx2,
               const float *decfactor_dev, float *refined, const int *len_new, hipStream_t s) {
    const long total = (long)b * m;
    RF_LAUNCH(name, merge_pull_kernel<RAGGED>, dim3(rf::ceil_div(total, 256)), dim3(256), 0, s, n, m, total, rawpts, newpts,
              idx2, decfactor_dev, refined, len_new);
    return RF_OK;
}

// what both merge_layer gradients zero before their kernel: grad_raw (the kernel adds into it), and grad_dec where there is
// no pair to pull (`empty`: the caller returns then)
int merge_grad_zero(int b, int n, bool empty, float *grad_dec, float *grad_raw, hipStream_t s) {
    if (grad_raw && n) RF_ZERO(grad_raw, sizeof(float) * 3 * (size_t)b * n, s);
    if (empty) RF_ZERO(grad_dec, sizeof(float) * (size_t)b, s);
    return RF_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ one direction ----------
size_t rf_nn_distance_dir_workspace_bytes(int b, int n, int m, int want1, int want2) {
    if (b <= 0 || n <= 0 || m <= 0 || !(want1 || want2)) return 0;
    return plan_forward(b, n, m, dirs_of(want1, want2), false, false).bytes;
}

int rf_nn_distance_dir(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, int *idx1,
                       float *dist2, int *idx2, void *workspace, size_t workspace_bytes, rf_stream_t stream,
                       int want1, int want2) {
    if (bad_sizes(b, n, m) || !(want1 || want2)) return RF_EINVAL;
    if (b == 0 || (n == 0 && m == 0)) return RF_OK;
    if (n == 0 || m == 0) return RF_EINVAL;
    if (!xyz1 || !xyz2 || (want1 && (!dist1 || !idx1)) || (want2 && (!dist2 || !idx2))) return RF_EINVAL;
    return run_forward(b, n, m, xyz1, xyz2, nullptr, nullptr, dist1, idx1, dist2, idx2, dirs_of(want1, want2),
                       workspace, workspace_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------ sorted handles ---------
size_t rf_nn_sort_bytes(int b, int n) { return rfp::sorted_bytes(b, n); }

int rf_nn_sort(int b, int n, const float *xyz, void *sorted, size_t sorted_bytes, rf_stream_t stream) {
    if (b <= 0 || n <= 0 || n > rfp::kMaxPoints || !xyz || !rf::workspace_ok(sorted)) return RF_EINVAL;
    if (sorted_bytes < rfp::sorted_bytes(b, n)) return RF_EWORKSPACE;
    const rfp::Sorted v = rfp::sorted_view(b, n, sorted);
    return rfp::sort_sets(b, 1, &n, &xyz, &v, (hipStream_t)stream, nullptr);
}

int rf_nn_distance_sorted(int b, int n, int m, const void *sorted1, const void *sorted2, float *dist1, int *idx1,
                          float *dist2, int *idx2, rf_stream_t stream) {
    if (!rfp::pruned_supported(b, n, m) || !rf::workspace_ok(sorted1) || !rf::workspace_ok(sorted2)) return RF_EINVAL;
    const int dirs = dirs_of(dist1 && idx1, dist2 && idx2);
    if (!dirs) return RF_EINVAL;
    return rfp::sweep_sorted(b, n, m, rfp::sorted_view(b, n, sorted1), rfp::sorted_view(b, m, sorted2),
                             (dirs & 1) ? dist1 : nullptr, (dirs & 1) ? idx1 : nullptr, (dirs & 2) ? dist2 : nullptr,
                             (dirs & 2) ? idx2 : nullptr, dirs, (hipStream_t)stream, nullptr);
}

// ------------------------------------------------------------------ forward + backward -----
size_t rf_chamfer_step_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    if (rfd::resolve_mode(b, n, m, RF_NN_AUTO) == RF_NN_CULLED) return rfp::pruned_step_workspace_bytes(b, n, m);
    return rf_nn_distance_workspace_bytes(b, n, m);
}

int rf_chamfer_step(int b, int n, int m, const float *xyz1, const float *xyz2, const float *grad_dist1,
                    const float *grad_dist2, float *dist1, int *idx1, float *dist2, int *idx2, float *grad_xyz1,
                    float *grad_xyz2, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    // Large clouds (the culled sweep's sizes): the sweep leaves, per query and in sorted order, its winner's
    // sorted position and its upstream gradient, and the backward runs in sorted index space
    // (nnp_grad_sorted_kernel).  Other shapes: the two ops back to back.
    if (b > 0 && n > 0 && m > 0 && rfd::resolve_mode(b, n, m, RF_NN_AUTO) == RF_NN_CULLED) {
        if (!rf::all_given({xyz1, xyz2, dist1, idx1, dist2, idx2, workspace, grad_dist1, grad_dist2, grad_xyz1, grad_xyz2}))
            return RF_EINVAL;
        // A caller that sized the workspace with rf_nn_distance_workspace_bytes (rounds 1-2: the two sizes were equal)
        // still gets its step: the two ops back to back, same results -- not RF_EWORKSPACE.
        if (workspace_bytes >= rfp::pruned_step_workspace_bytes(b, n, m))
            return rfp::pruned_step(b, n, m, xyz1, xyz2, grad_dist1, grad_dist2, dist1, idx1, dist2, idx2, grad_xyz1,
                                    grad_xyz2, workspace, workspace_bytes, (hipStream_t)stream);
    }
    if (int e = rf_nn_distance(b, n, m, xyz1, xyz2, dist1, idx1, dist2, idx2, workspace, workspace_bytes, stream))
        return e;
    return rf_nn_distance_grad(b, n, m, xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2, grad_xyz1, grad_xyz2,
                               stream);
}

// ------------------------------------------------------------------ fused Chamfer loss -----
size_t rf_chamfer_loss_workspace_bytes(int b, int n, int m, int want1, int want2, int have_sorted1,
                                       int have_sorted2) {
    if (b <= 0 || n <= 0 || m <= 0 || !(want1 || want2)) return 0;
    return plan_forward(b, n, m, dirs_of(want1, want2), have_sorted1 != 0, have_sorted2 != 0).bytes;
}

int rf_chamfer_loss(int b, int n, int m, const float *xyz1, const float *xyz2, const void *sorted1,
                    const void *sorted2, float *loss, float *dist1, int *idx1, float *dist2, int *idx2,
                    void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n == 0 || m == 0 || !rf::all_given({xyz1, xyz2, loss})) return RF_EINVAL;
    const int dirs = dirs_of(dist1 && idx1, dist2 && idx2);
    if (!dirs) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (int e = run_forward(b, n, m, xyz1, xyz2, sorted1, sorted2, dist1, idx1, dist2, idx2, dirs, workspace,
                            workspace_bytes, s))
        return e;
    RF_LAUNCH("chamfer_loss_reduce", chamfer_loss_reduce_kernel<0>, dim3(2 * b), dim3(LR_TPB), 0, s, n, m,
              (const float *)((dirs & 1) ? dist1 : nullptr), (const float *)((dirs & 2) ? dist2 : nullptr), loss,
              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return RF_OK;
}

int rf_chamfer_loss_grad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *dist1,
                         const int *idx1, const float *dist2, const int *idx2, const float *grad_loss,
                         float *grad_xyz1, float *grad_xyz2, rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0 || (n == 0 && m == 0)) return RF_OK;
    if (!grad_loss) return RF_EINVAL;
    const rfd::GradSource g{nullptr, nullptr, dist1, dist2, grad_loss};
    return rfd::nn_distance_grad(b, n, m, xyz1, xyz2, g, dist1 ? idx1 : nullptr, dist2 ? idx2 : nullptr, grad_xyz1,
                                 grad_xyz2, (hipStream_t)stream);
}

// ------------------------------------------------------------------ fused loss, ragged -----
size_t rf_chamfer_loss_lengths_workspace_bytes(int b, int n, int m, int want1, int want2) {
    if (b <= 0 || n <= 0 || m <= 0 || !(want1 || want2)) return 0;
    return rfd::ragged_workspace_bytes(b, n, m, RF_NN_AUTO, dirs_of(want1, want2));
}

int rf_chamfer_loss_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                            const int *len2, float *loss, float *dist1, int *idx1, float *dist2, int *idx2,
                            void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n == 0 || m == 0 || !rf::all_given({xyz1, xyz2, loss, workspace})) return RF_EINVAL;
    const int dirs = dirs_of(dist1 && idx1, dist2 && idx2);
    if (!dirs) return RF_EINVAL;
    if (!rf::aligned16(workspace) || !rf::all_aligned4({len1, len2})) return RF_EINVAL;
    if (workspace_bytes < rfd::ragged_workspace_bytes(b, n, m, RF_NN_AUTO, dirs)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *d1 = (dirs & 1) ? dist1 : nullptr, *d2 = (dirs & 2) ? dist2 : nullptr;
    int *i1 = (dirs & 1) ? idx1 : nullptr, *i2 = (dirs & 2) ? idx2 : nullptr;
    // the culled route leaves the padded slots to the reduction (the dense sweep writes them itself)
    const bool culled = rfd::resolve_mode(b, n, m, RF_NN_AUTO) == RF_NN_CULLED;
    if (int e = rfd::ragged_nn_distance(b, n, m, xyz1, xyz2, len1, len2, d1, i1, d2, i2, workspace, workspace_bytes, s,
                                        RF_NN_AUTO, dirs, !culled))
        return e;
    RF_LAUNCH("chamfer_loss_reduce_len", chamfer_loss_reduce_kernel<1>, dim3(2 * b), dim3(LR_TPB), 0, s, n, m,
              (const float *)d1, (const float *)d2, loss, len1, len2, culled ? d1 : nullptr, culled ? i1 : nullptr,
              culled ? d2 : nullptr, culled ? i2 : nullptr);
    return RF_OK;
}

int rf_chamfer_loss_grad_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                                 const int *len2, const float *dist1, const int *idx1, const float *dist2,
                                 const int *idx2, const float *grad_loss, float *grad_xyz1, float *grad_xyz2,
                                 rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n == 0 || m == 0 || !grad_loss) return RF_EINVAL;
    if (!rf::all_aligned4({len1, len2})) return RF_EINVAL;
    const rfd::GradSource g{nullptr, nullptr, dist1, dist2, grad_loss};
    // both count arrays NULL: the kernel of rf_chamfer_loss_grad, same results
    return rfd::nn_distance_grad(b, n, m, xyz1, xyz2, g, dist1 ? idx1 : nullptr, dist2 ? idx2 : nullptr, grad_xyz1,
                                 grad_xyz2, (hipStream_t)stream, len1, len2);
}

// ------------------------------------------------------------------ merge_layer ------------
size_t rf_merge_layer_workspace_bytes(int b, int n, int m, int have_sorted_raw) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return merge_dist_bytes(b, m) + plan_forward(b, n, m, 2, have_sorted_raw != 0, false).bytes;
}

int rf_merge_layer(int b, int n, int m, const float *rawpts, const float *newpts, const void *sorted_raw,
                   const float *decfactor_dev, float *refined, int *idx2, void *workspace, size_t workspace_bytes,
                   rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0 || m == 0) return RF_OK;
    if (n == 0 || !rf::all_given({rawpts, newpts, decfactor_dev, refined, idx2, workspace})) return RF_EINVAL;
    const size_t dbytes = merge_dist_bytes(b, m);
    if (workspace_bytes < dbytes) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *dist2 = (float *)workspace;  // the distances themselves are not an output of merge_layer
    if (int e = run_forward(b, n, m, rawpts, newpts, sorted_raw, nullptr, nullptr, nullptr, dist2, idx2, 2,
                            (char *)workspace + dbytes, workspace_bytes - dbytes, s))
        return e;
    return merge_pull<false>("merge_pull", b, n, m, rawpts, newpts, idx2, decfactor_dev, refined, nullptr, s);
}

int rf_merge_layer_grad(int b, int n, int m, const float *rawpts, const float *newpts, const float *decfactor_dev,
                        const int *idx2, const float *grad_refined, float *grad_newpts, float *grad_dec,
                        float *grad_raw, rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!grad_dec) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool empty = m == 0 || n == 0;
    if (int e = merge_grad_zero(b, n, empty, grad_dec, grad_raw, s)) return e;
    if (empty) return RF_OK;
    if (!rf::all_given({rawpts, newpts, decfactor_dev, idx2, grad_refined, grad_newpts})) return RF_EINVAL;
    RF_LAUNCH("merge_pull_grad", merge_pull_grad_kernel<false>, dim3(b), dim3(MG_TPB), 0, s, n, m, rawpts, newpts, idx2,
              decfactor_dev, grad_refined, grad_newpts, grad_dec, grad_raw, nullptr, nullptr);
    return RF_OK;
}

// ------------------------------------------------------------------ merge_layer, ragged ----
size_t rf_merge_layer_lengths_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return merge_dist_bytes(b, m) + rfd::ragged_workspace_bytes(b, n, m, RF_NN_AUTO, 2);
}

int rf_merge_layer_lengths(int b, int n, int m, const float *rawpts, const float *newpts, const int *len_raw,
                           const int *len_new, const float *decfactor_dev, float *refined, int *idx2, void *workspace,
                           size_t workspace_bytes, rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0 || m == 0) return RF_OK;
    if (n == 0 || !rf::all_given({rawpts, newpts, decfactor_dev, refined, idx2, workspace})) return RF_EINVAL;
    if (!rf::aligned16(workspace) || !rf::all_aligned4({len_raw, len_new})) return RF_EINVAL;
    const size_t dbytes = merge_dist_bytes(b, m);
    if (workspace_bytes < rf_merge_layer_lengths_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *dist2 = (float *)workspace;  // the distances themselves are not an output of merge_layer
    // pad_culled = false: the pull kernel below writes every padded slot of idx2 itself, on either route
    if (int e = rfd::ragged_nn_distance(b, n, m, rawpts, newpts, len_raw, len_new, nullptr, nullptr, dist2, idx2,
                                        (char *)workspace + dbytes, workspace_bytes - dbytes, s, RF_NN_AUTO, 2, false))
        return e;
    return merge_pull<true>("merge_pull_len", b, n, m, rawpts, newpts, idx2, decfactor_dev, refined, len_new, s);
}

int rf_merge_layer_grad_lengths(int b, int n, int m, const float *rawpts, const float *newpts, const int *len_raw,
                                const int *len_new, const float *decfactor_dev, const int *idx2,
                                const float *grad_refined, float *grad_newpts, float *grad_dec, float *grad_raw,
                                rf_stream_t stream) {
    if (bad_sizes(b, n, m)) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!grad_dec || !rf::all_aligned4({len_raw, len_new})) return RF_EINVAL;
    const bool empty = m == 0 || n == 0;
    if (!empty && !rf::all_given({rawpts, newpts, decfactor_dev, idx2, grad_refined, grad_newpts})) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (int e = merge_grad_zero(b, n, empty, grad_dec, grad_raw, s)) return e;
    if (empty) return RF_OK;
    RF_LAUNCH("merge_pull_grad_len", merge_pull_grad_kernel<true>, dim3(b), dim3(MG_TPB), 0, s, n, m, rawpts, newpts, idx2,
              decfactor_dev, grad_refined, grad_newpts, grad_dec, grad_raw, len_raw, len_new);
    return RF_OK;
}

}  // extern "C"
