/*
 * rfops.h -- C ABI of librfops.so: RFNet's point-cloud operator hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  Each entry point replaces one of the reference's
 * C++-mangled "Launcher" functions that its TensorFlow OpKernels call (the native ABI
 * under tf_ops/ and pc_distance/); the reference interface each
 * one replaces is cited as file:line.  Conventions, identical to the reference's:
 *
 *   - all pointers are DEVICE pointers (HIP), row-major contiguous; xyz tensors are
 *     (b, npts, 3) float32, index tensors int32;
 *   - the caller owns every buffer (outputs, gradients, scratch); the library never
 *     allocates or frees device memory, and never synchronises the stream;
 *   - gradient outputs are zero-filled by the call itself (the reference's ops do the
 *     cudaMemset inside the launcher / OpKernel) -- by a kernel, never hipMemset*: every call can
 *     be captured into a HIP graph and replayed;
 *   - kernels are stateless and re-entrant; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).  The reference launches
 *     on the legacy default stream with no error checking; here every call returns a status.
 *     The library keeps no state between calls and reads no environment variables; the one
 *     exception is the opt-in measurement hook at the end of this file (rf_profile_*), which is
 *     process-global, thread-safe and off by default;
 *   - every call that launches work first checks that the calling thread's current HIP device
 *     is a gfx950 (the only code objects in the library) and returns RF_ENODEVICE otherwise;
 *   - `workspace` buffers and sorted-set handles (rf_nn_sort) must be 16-byte aligned -- the kernels read
 *     them with 16-byte vector loads at 256-byte-multiple offsets; any hipMalloc pointer is.  A misaligned
 *     one is RF_EINVAL (culled Chamfer paths, approx_match, earth_mover), not a fault inside a kernel.
 *     Tensor arguments need their element's natural alignment (4 bytes), except the (.., c) feature tensors of the
 *     model graph helpers, which are read and written in rows of c % 4 == 0 floats and need 16 bytes:
 *     rf_point_affine's y, w, r and out, rf_maxpool_points' and rf_maxpool_points_idx's x (their _lengths forms too), rf_act_grad_colsum's grad,
 *     out and g (their p, out / idx and sums need 4).  rf_grid_cluster's int64 code needs its own 8 bytes.  A less aligned
 *     one is RF_EINVAL before anything is launched.
 *
 * Status codes: 0 = success; > 0 = the hipError_t of the failing HIP call;
 *               < 0 = RF_EINVAL-style argument errors below.
 *
 * No torch / TensorFlow types appear here; bind with ctypes, cgo, JNI ... as needed
 * (INTEGRATION.md shows the reference-side stub).
 */
#ifndef RFOPS_H_
#define RFOPS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_OK 0
#define RF_EINVAL (-1)     /* negative size, NULL pointer with non-zero size, bad attribute, misaligned workspace */
#define RF_EWORKSPACE (-2) /* workspace smaller than rf_*_workspace_bytes() says            */
#define RF_ENODEVICE (-3)  /* no gfx950 device / code object could not be loaded            */

typedef void *rf_stream_t; /* hipStream_t */

const char *rf_version(void);
const char *rf_status_string(int status);
/* RF_OK when the calling thread's current HIP device is a gfx950, RF_ENODEVICE otherwise
 * (no device visible, or another architecture).  Every launching entry point makes this check. */
int rf_device_check(void);

/* ---------------------------------------------------------------- Chamfer (tf_ops/CD) --- */
/* Replaces NmDistanceKernelLauncher(b,n,xyz,m,xyz2,result,result_i,result2,result2_i)
 * (tf_ops/CD/tf_nndistance.cpp:168, tf_nndistance_g.cu:127-130; same op duplicated under
 * pc_distance/).  dist1[i,j] = min_k |xyz2[i,k]-xyz1[i,j]|^2, idx1 = lowest argmin;
 * dist2/idx2 symmetric.  `workspace`: per-split partial minima (dense sweep) or the sorted clouds
 * and their boxes (culled sweep); rf_nn_distance_workspace_bytes sizes it for the sweep that
 * rf_nn_distance picks for this shape. */
size_t rf_nn_distance_workspace_bytes(int b, int n, int m);
int rf_nn_distance(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1,
                   int *idx1, float *dist2, int *idx2, void *workspace, size_t workspace_bytes,
                   rf_stream_t stream);

/* Same call with the sweep pinned: RF_NN_DENSE evaluates all b*n*m pairs (nn_distance.hip),
 * RF_NN_CULLED sorts both clouds along a space-filling curve and skips blocks of candidates whose
 * bounding box is strictly farther than every query's current minimum (nn_pruned.hip; n, m <=
 * 65536) -- identical outputs, bit for bit, ties included.  RF_NN_AUTO (what rf_nn_distance
 * uses) picks by size.  `stats` (host pointer to 32 counters, or NULL; filled by the culled sweep
 * only): per direction d at [4d..4d+3] {waves, superblock steps, most steps of one wave, 16-candidate
 * block scans}, [8+d] most block scans of one wave, [12+d] directed pairs evaluated (summed by the kernel), [14+d] directed pairs per
 * counted block scan of the last wave of direction d to report (1024: 64 queries x 16 candidates; 16 where a query has four lanes of
 * its own, nn_pruned.hip sweep_tile16; a launch may mix both), [16..31] phase time stamps of the sort; a non-NULL
 * pointer synchronises the stream. */
#define RF_NN_AUTO 0
#define RF_NN_DENSE 1
#define RF_NN_CULLED 2
size_t rf_nn_distance_mode_workspace_bytes(int b, int n, int m, int mode);
int rf_nn_distance_mode(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1,
                        int *idx1, float *dist2, int *idx2, void *workspace, size_t workspace_bytes,
                        rf_stream_t stream, int mode, unsigned long long *stats);

/* Replaces NmDistanceGradKernelLauncher (tf_nndistance.cpp:208, tf_nndistance_g.cu:151-156).
 * grad_xyz1 (b,n,3) and grad_xyz2 (b,m,3) are zero-filled here, then accumulated. */
int rf_nn_distance_grad(int b, int n, int m, const float *xyz1, const float *xyz2,
                        const float *grad_dist1, const int *idx1, const float *grad_dist2,
                        const int *idx2, float *grad_xyz1, float *grad_xyz2, rf_stream_t stream);

/* ---- one direction, sorted-cloud handles, one-call step (Chamfer, continued) ------------- */
/* The same op with only the direction(s) a caller uses.  The reference's glue calls
 * nn_distance(xyz1, xyz2) and then drops outputs: merge_layer keeps idx2 alone
 * (vv_recon.py:134-135), fidelity_loss dist1 (:386-390), zero_groupnear dist2 (:415-419);
 * NmDistanceKernelLauncher (tf_nndistance_g.cu:127-130) is two independent kernel launches, one per
 * direction, so a TF-side op with a "directions" attribute maps onto this entry.  want1: dist1/idx1
 * (nearest neighbour of every xyz1 point in xyz2); want2: dist2/idx2.  Outputs of a direction that
 * is not wanted may be NULL and are not written.  Bit-identical to rf_nn_distance's. */
size_t rf_nn_distance_dir_workspace_bytes(int b, int n, int m, int want1, int want2);
int rf_nn_distance_dir(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1,
                       int *idx1, float *dist2, int *idx2, void *workspace, size_t workspace_bytes,
                       rf_stream_t stream, int want1, int want2);

/* A cloud that takes part in several Chamfers (the model Chamfers `pointcloud` 3x and `gt` 5x per
 * training step, vv_recon.py:213,225,238 and :484-498) can be put in space-filling-curve order
 * ONCE.  `sorted` is a caller-owned device buffer of rf_nn_sort_bytes(b, n) bytes whose layout is a
 * pure function of (b, n) (records, original indices and block boxes in key order): the library
 * keeps no state, the buffer IS the handle, valid for as long as the caller keeps it and xyz is
 * unchanged.  rf_nn_distance_sorted runs the culled exact sweep on two such buffers; a direction
 * whose outputs are NULL is skipped.  n, m <= 65536.  Same results as rf_nn_distance. */
size_t rf_nn_sort_bytes(int b, int n);
int rf_nn_sort(int b, int n, const float *xyz, void *sorted, size_t sorted_bytes, rf_stream_t stream);
int rf_nn_distance_sorted(int b, int n, int m, const void *sorted1, const void *sorted2, float *dist1,
                          int *idx1, float *dist2, int *idx2, rf_stream_t stream);

/* NnDistance followed by NnDistanceGrad on its own indices (what one training step of the
 * reference's Chamfer bench does, tf_ops/CD/tf_nndistance.py:35-61) in ONE call on caller-owned
 * buffers: one FFI crossing per step, nothing allocated.  Equivalent to rf_nn_distance +
 * rf_nn_distance_grad(..., grad_dist1, idx1, grad_dist2, idx2, ...): forward outputs bit-identical, gradients
 * within the backward's tolerance (fp32 add order of a scatter).  On shapes that take the culled sweep the
 * forward also leaves, in the workspace and in sorted query order, every query's winner position and own
 * gradient term, and the backward runs in sorted index space (nnp_grad_sorted_kernel): the
 * workspace is larger than rf_nn_distance's there (rf_chamfer_step_workspace_bytes says by how much). */
size_t rf_chamfer_step_workspace_bytes(int b, int n, int m);
int rf_chamfer_step(int b, int n, int m, const float *xyz1, const float *xyz2,
                    const float *grad_dist1, const float *grad_dist2, float *dist1, int *idx1,
                    float *dist2, int *idx2, float *grad_xyz1, float *grad_xyz2, void *workspace,
                    size_t workspace_bytes, rf_stream_t stream);

/* ---- ragged batches: per-sample point counts (Chamfer, continued) ----------------------- */
/* Clouds of different sizes in one padded batch.  len1 / len2 are DEVICE int32 arrays of b counts:
 * sample i uses xyz1[i, :len1[i]] and xyz2[i, :len2[i]]; the coordinates beyond a count are never read into
 * any result (they may hold anything: NaN, inf, copies of valid points).  Either array may be NULL ("all n",
 * "all m").  Domain 1 <= len <= n (m); the kernels read the counts themselves (no host synchronisation, so a
 * call can be captured in a HIP graph) and CLAMP a device value outside the domain into [1, n] (resp. m),
 * so a bad count can never make a kernel read or write past the tensors -- it just gives that sample's
 * results for the clamped count.
 *
 * rf_nn_distance_lengths: on the valid slots dist / idx are bit for bit what rf_nn_distance_mode returns
 * on the unpadded slices of that sample alone (ties to the lowest index, non-finite inputs included), and
 * a valid idx always points into the other cloud's valid range; padded slots get dist = 0.0f and idx = -1.
 * `mode` is RF_NN_AUTO (routes by (n, m) exactly as rf_nn_distance does), RF_NN_DENSE or RF_NN_CULLED
 * (n, m <= 65536, else RF_EINVAL).  The dense sweep takes the counts into its kernels, so its work shrinks
 * with them; the culled sweep's sort keys and boxes only a sample's first len points and the sweep skips the
 * padding behind them, so its work shrinks with the counts too.  A direction whose two output
 * pointers are NULL is skipped (one NULL of a pair is RF_EINVAL).  Pointers must be 4-byte aligned, the
 * workspace 16-byte aligned (RF_EINVAL); a workspace smaller than rf_nn_distance_lengths_workspace_bytes
 * (b, n, m, mode) is RF_EWORKSPACE -- both checked before any HIP call. */
size_t rf_nn_distance_lengths_workspace_bytes(int b, int n, int m, int mode);
int rf_nn_distance_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                           const int *len2, float *dist1, int *idx1, float *dist2, int *idx2, void *workspace,
                           size_t workspace_bytes, rf_stream_t stream, int mode);

/* NnDistanceGrad restricted to the valid slots: rows beyond a sample's count get a gradient of exactly 0
 * whatever grad_dist / idx hold there, valid rows are rf_nn_distance_grad's on the sample alone (within
 * the backward's fp32 add-order tolerance).  grad_xyz1 (b,n,3) / grad_xyz2 (b,m,3) fully overwritten. */
int rf_nn_distance_grad_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                                const int *len2, const float *grad_dist1, const int *idx1,
                                const float *grad_dist2, const int *idx2, float *grad_xyz1, float *grad_xyz2,
                                rf_stream_t stream);

/* rf_chamfer_loss on ragged batches: loss[i][0] = mean of sqrt(dist1) over the len1[i] valid points,
 * loss[i][1] likewise over len2[i] (0 for a direction whose dist/idx pointers are NULL), next to
 * rf_nn_distance_lengths' outputs of the computed directions (sweep chosen as RF_NN_AUTO).  No sorted handles:
 * the culled sweep sorts internally.  rf_chamfer_loss_grad_lengths is its backward, scaling by 1 / len
 * instead of 1 / n; rows beyond a count get exactly 0.  Before any HIP call: RF_EINVAL for a NULL tensor, a
 * misaligned count array or workspace, RF_EWORKSPACE for a workspace smaller than
 * rf_chamfer_loss_lengths_workspace_bytes(b, n, m, want1, want2). */
size_t rf_chamfer_loss_lengths_workspace_bytes(int b, int n, int m, int want1, int want2);
int rf_chamfer_loss_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                            const int *len2, float *loss, float *dist1, int *idx1, float *dist2, int *idx2,
                            void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_chamfer_loss_grad_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                                 const int *len2, const float *dist1, const int *idx1, const float *dist2,
                                 const int *idx2, const float *grad_loss, float *grad_xyz1, float *grad_xyz2,
                                 rf_stream_t stream);

/* ---- evaluation metrics on the sweep's outputs (Chamfer, continued) ---------------------- */
/* What a completion result is judged by, per sample, in one call: CD-L1, CD-L2, Hausdorff, F-score at a threshold
 * and the density-aware Chamfer distance (DCD), with the per-point counts DCD needs.  Conventions are
 * rf_nn_distance_lengths': len1 / len2 device int32 counts or NULL, read and clamped into [1, n] / [1, m] by the
 * kernels (no host synchronisation: a call can be captured in a HIP graph); L1, L2 below are the clamped counts.
 * Direction 1 is "points of xyz1 looking into xyz2" (dist1 / idx1 (b,n)), direction 2 the reverse ((b,m)).
 *
 *   count2[i][k] (b,m) = #{j < L1 : idx1[i][j] == k}      count1[i][j] (b,n) = #{k < L2 : idx2[i][k] == j}
 *   (exact integers; slots behind a count are 0; a valid point's own neighbour always has a count >= 1)
 *
 * metrics (b, RF_CM_NCOL), every sum over the valid slots only; direction d = 1, 2 in the even / odd column of a pair:
 *   0, 1   mean of sqrtf(dist_d)               the two halves of CD-L1 (rf_chamfer_loss_lengths' numbers)
 *   2, 3   mean of dist_d                      the halves of CD-L2
 *   4, 5   max of dist_d                       squared directed Hausdorff distances
 *   6, 7   (float)#{dist_d < thr2} / (float)L_d    strict fp32 compare with thr2 as given: pass the SQUARED threshold
 *   8      2 c6 c7 / (c6 + c7), +0 when c6 + c7 == 0    (F-score; c6 is the precision when xyz1 is the prediction)
 *   9, 10  mean_j (1 - expf(-alpha dist_d[j]) / (float)cnt),  cnt = the count of j's own neighbour
 *          (count2[idx1[j]] for d = 1, count1[idx2[k]] for d = 2): DCD with exponent 1 on the count and no
 *          set-size ratio factor
 * Columns 4-7 are exact (max and integer counts are order-free, one correctly rounded division); the float sums
 * take a fixed order, so two calls return identical bits; within rel 1e-5 (0-3), 1e-6 (8), rel 1e-5 + abs 1e-6
 * (9, 10) of the definitions in float64.  No float atomics.
 *
 * rf_nn_metrics: the epilogue alone on nn_distance outputs the caller holds (any route, sorted handles included);
 * padded slots of dist / idx are not read.  An index outside the other cloud is not counted and weighs as count 1.
 * Its workspace (256 bytes for positive sizes) is currently unused by the kernels; the pointer and size rules below
 * are checked all the same.
 * rf_chamfer_metrics: rf_nn_distance_lengths (RF_NN_AUTO, both directions: dist / idx bit for bit its outputs,
 * padded slots (0, -1)) and then the epilogue.  Inputs with non-finite coordinates never make a kernel read or
 * write out of bounds; the metric values for them are unspecified.
 * rf_chamfer_metrics_grad: columns 0-3, 9 and 10 are differentiable, columns 4-8 of grad_metrics are not read;
 * the counts are constants (a detached weight).  With g = grad_metrics[i]:
 *   gd_d[j] = g[d-1] 0.5 / (L_d sqrtf(dist_d[j])) + g[1+d] / L_d + g[8+d] alpha expf(-alpha dist_d[j]) / (cnt L_d)
 * where a term whose upstream value is exactly 0 is not formed (a zero distance then cannot turn 0 * inf into NaN
 * when only DCD is trained), followed by rf_nn_distance_grad_lengths: grad_xyz1 (b,n,3) / grad_xyz2 (b,m,3) fully
 * overwritten, rows behind a count exactly +0; within rel 1e-4 + abs 1e-5 as the other fused gradients.
 *
 * Argument rules, all checked before any HIP call: b == 0 is RF_OK; RF_EINVAL for n < 1 or m < 1, b > 65535, a NULL
 * tensor, a count array or tensor not 4-byte aligned, a workspace that is NULL or not 16-byte aligned, thr2 NaN or
 * negative (+inf is allowed), alpha negative or not finite; RF_EWORKSPACE for a workspace smaller than the matching
 * _workspace_bytes (0 for non-positive sizes, positive otherwise). */
#define RF_CM_NCOL 11
size_t rf_nn_metrics_workspace_bytes(int b, int n, int m);
int rf_nn_metrics(int b, int n, int m, const float *dist1, const int *idx1, const float *dist2, const int *idx2,
                  const int *len1, const int *len2, float thr2, float alpha, float *metrics, int *count1,
                  int *count2, void *workspace, size_t workspace_bytes, rf_stream_t stream);
size_t rf_chamfer_metrics_workspace_bytes(int b, int n, int m);
int rf_chamfer_metrics(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                       float thr2, float alpha, float *metrics, float *dist1, int *idx1, float *dist2, int *idx2,
                       int *count1, int *count2, void *workspace, size_t workspace_bytes, rf_stream_t stream);
size_t rf_chamfer_metrics_grad_workspace_bytes(int b, int n, int m);
int rf_chamfer_metrics_grad(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                            const int *len2, const float *dist1, const int *idx1, const float *dist2,
                            const int *idx2, const int *count1, const int *count2, float alpha,
                            const float *grad_metrics, float *grad_xyz1, float *grad_xyz2, void *workspace,
                            size_t workspace_bytes, rf_stream_t stream);

/* ---- the Chamfer matrix of two collections of clouds (Chamfer, continued) ----------------- */
/* What a set metric needs (minimal matching distance, MMD / coverage / 1-NN accuracy, nearest-shape retrieval): for
 * EVERY cloud i of xyz1 (s, n, 3) and EVERY cloud j of xyz2 (r, m, 3) the first six columns of rf_chamfer_metrics, in
 * out (s, r, RF_CX_NCOL).  Each collection is sorted once (s + r sorts, not s * r), nothing is stored per point, and no
 * index is tracked.  Conventions are rf_nn_distance_lengths': len1 (s) / len2 (r) device int32 counts or NULL, read and
 * clamped into [1, n] / [1, m] by the kernels; rows behind a count never reach a result.  No host synchronisation: a
 * call can be captured in a HIP graph.  With L1, L2 the clamped counts of cloud i of xyz1 and cloud j of xyz2:
 *
 *   d1[k] = min_{l < L2} d(xyz2[j][l], xyz1[i][k]), k < L1      d2[l] = min_{k < L1} d(xyz1[i][k], xyz2[j][l]), l < L2
 *   d = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) on "other - own": every d1 / d2 is bit for bit rf_nn_distance's value
 *
 *   0, 1   mean of sqrtf(d1), mean of sqrtf(d2)      within rel 1e-5 of the float64 mean of the fp32 values
 *   2, 3   mean of d1, mean of d2                    the same
 *   4, 5   max of d1, max of d2                      exact
 *
 * Guarantees:
 *   - No float atomics and no float sum at all: every sum is an exact INTEGER sum of the terms on a fixed-point grid
 *     that is a function of the pair alone, followed by one division: with D the squared diagonal of the joint box
 *     of the two clouds and P the power of two with P / 4 <= D < P / 2, the grid step is P 2^-111 for d and, with P'
 *     the power of two with sqrt(P) <= P' < 2 sqrt(P), P' 2^-111 for sqrtf(d).  Two calls return identical bits,
 *     whatever order the sort left the points in.  A term is truncated only below the step: the bar above holds
 *     whenever a mean is at least 2^-94 of P (of P'), and below that the absolute error stays under one step.  A
 *     direction with one valid point returns its sqrtf(d) and d exactly (d >= 2^-88 P).
 *   - Batch invariance: the six numbers of a pair depend only on that pair's two clouds and counts -- not on s, r,
 *     the position of the clouds in their collections or on what the other clouds hold.
 *   - Self-distance: with xyz1 == xyz2, len1 == len2, s == r and n == m the collection is sorted once and only one
 *     direction is swept (direction 2 of (i, j) is direction 1 of (j, i)); the results are the bits of the general call.
 *   - Memory safety: non-finite coordinates in valid rows never cause a read or write out of bounds -- every loop
 *     bound is a count, never a data value.  The numbers returned for such clouds are unspecified.
 *
 * Workspace, with sb(n) = (padded record count of a sorted cloud of n points) / 64 <= n / 64 + 2, each part rounded
 * up to 256 bytes:  rf_nn_sort_bytes(s, n) + rf_nn_sort_bytes(r, m) + 32 (s + r) + 48 s r sb(n) + 48 s r sb(m)
 * -- the two sorted collections, a box per cloud, and one 48-byte record per (i, j, 64 points) and direction; nothing
 * of size s r n or s r m.
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then s == 0 or r == 0 is RF_OK;
 * RF_EINVAL for n < 1 or m < 1, n or m above 65536, s or r above 65535, a NULL tensor, a tensor or count array not
 * 4-byte aligned, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a workspace smaller than
 * rf_chamfer_cross_workspace_bytes (0 for non-positive or unsupported sizes, positive otherwise).  All index
 * arithmetic is in size_t. */
#define RF_CX_NCOL 6
size_t rf_chamfer_cross_workspace_bytes(int s, int r, int n, int m);
int rf_chamfer_cross(int s, int r, int n, int m, const float *xyz1, const float *xyz2, const int *len1,
                     const int *len2, float *out, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* ---- the sliced Wasserstein distance of two clouds, with gradients ------------------------- */
/* A transport-type loss that is cheap at 16384 points and takes unequal and ragged counts exactly: both clouds are
 * projected on nproj directions, in 1-D optimal transport is sorting, and the per-direction costs are averaged.
 * xyz1 (b, n, 3), xyz2 (b, m, 3); dirs (nproj, 3) fp32 on the device, used as given (not normalised, no gradient).
 * len1 / len2: device int32 (b) or NULL with rf_nn_distance_lengths' conventions -- read and clamped into [1, n] /
 * [1, m] by the kernels, rows behind a count never reach a result.  No host synchronisation: a call can be captured in
 * a HIP graph.  Per sample and direction l = (tx, ty, tz), with L1, L2 the clamped counts:
 *
 *   1. p = fmaf(z, tz, fmaf(x, tx, y * ty)) + 0.0f for every valid point (the + 0.0f makes -0 sort as +0);
 *   2. each cloud's projections are ordered ascending by (value, original index) -- ties go to the lower index, which
 *      fixes the permutation and therefore the gradient: u[0..L1), v[0..L2) the sorted values, r1, r2 the ranks;
 *   3. c_l = sum_{i, j} w_ij (u_i - v_j)^2, w_ij the length of [i / L1, (i + 1) / L1) with [j / L2, (j + 1) / L2) cut out:
 *      (min((i + 1) L2, (j + 1) L1) - max(i L2, j L1)) / (L1 L2), the numerator an exact integer.  For L1 == L2 this
 *      is mean((u - v)^2).  Rank i meets the ranks floor(i L2 / L1) ... ceil((i + 1) L2 / L1) - 1.
 *
 *   loss[b]     = (1 / nproj) sum_l c_l
 *   grad1[b][k] =  (2 / nproj) sum_l dir_l sum_j w_{r1(k), j} (u_{r1(k)} - v_j)      k < L1, exactly +0 behind the count
 *   grad2[b][k] = -(2 / nproj) sum_l dir_l sum_i w_{i, r2(k)} (u_i - v_{r2(k)})      k < L2, exactly +0 behind the count
 *
 * grad1 (b, n, 3) and grad2 (b, m, 3) are either both given or both NULL (loss only).  Only the projection is fp32:
 * differences, weights, squares and every sum are double, in a fixed order (ranks within a direction, then the
 * directions 0 ... nproj - 1), with one rounding to fp32 at the end.  No atomics.
 *
 * Guarantees:
 *   - Two calls return identical bits.
 *   - Batch invariance: sample i's loss and gradients are bit for bit those of the call on [i : i + 1], for every b
 *     and position, whatever the other samples hold.
 *   - Memory safety: non-finite coordinates in valid rows never move a memory access -- every loop bound is a count
 *     and every index a rank or an original index below its count.  The numbers of such a sample are unspecified; the
 *     other samples are unaffected.
 *
 * Directions are processed RF_SW_DIR_CHUNK at a time and nothing in the workspace grows with nproj beyond a chunk.
 * With c = min(nproj, RF_SW_DIR_CHUNK) and each part rounded up to 256 bytes:
 *   4 c b (n + m)  sorted values       + 4 c b (n + m)  original indices   + 8 c b  costs   + 8 b  one double per sample
 *   and with gradients   + 8 c b (n + m)  per-point coefficients   + 24 b (n + m)  double accumulators.
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for
 * n, m or nproj < 1, n or m above RF_SW_MAX_POINTS, b above 65535, a NULL xyz1 / xyz2 / dirs / loss, exactly one of
 * grad1 / grad2 given, a tensor or count array not 4-byte aligned, a workspace that is NULL or not 16-byte aligned;
 * RF_EWORKSPACE for a workspace smaller than rf_sliced_wasserstein_workspace_bytes (0 for non-positive or unsupported
 * sizes, positive otherwise).  All index arithmetic is in size_t. */
#define RF_SW_MAX_POINTS 16384
#define RF_SW_DIR_CHUNK 16
size_t rf_sliced_wasserstein_workspace_bytes(int b, int n, int m, int nproj, int want_grad);
int rf_sliced_wasserstein(int b, int n, int m, int nproj, const float *xyz1, const float *xyz2, const int *len1,
                          const int *len2, const float *dirs, float *loss, float *grad1, float *grad2, void *workspace,
                          size_t workspace_bytes, rf_stream_t stream);

/* ---- the Sinkhorn divergence of two clouds: debiased entropic optimal transport, with gradients -- */
/* A transport-type loss that is differentiable, takes unequal and ragged counts at every size the other entries take, and
 * has a stated relation to optimal transport: S_eps(a, a) = 0, S_eps >= 0, and S_eps goes to the transport cost as eps -> 0
 * and to an energy distance as eps -> infinity.  xyz1 (b, n, 3), xyz2 (b, m, 3) fp32; len1 / len2: device int32 (b) or NULL
 * with rf_nn_distance_lengths' conventions -- read and clamped into [1, n] / [1, m] by the kernels, rows behind a count
 * never reach a result.  p: 1 or 2.  eps: a HOST array of T positive finite floats, 1 <= T <= RF_SK_MAX_ITERS, the
 * regularisation of every step (an annealing schedule ends at blur^p); it is read at call time, so a captured graph replays
 * the schedule it was captured with.  No host synchronisation, T + 2 launches on `stream`: a call can be captured.
 *
 * With L1, L2 the clamped counts, uniform weights a_i = 1 / L1, b_j = 1 / L2, and
 *   C(x, y) = sqrt(((dx dx) + (dy dy)) + (dz dz)) for p = 1 (unfused; the root from v_sqrt_f32, 1 ulp),  0.5f d^2 for p = 2
 *   softmin_e(C, h, w)_i = -e log sum_j w_j exp((h_j - C_ij) / e)
 * the iteration is Jacobi and averaged, from zero potentials: for t = 0 ... T - 1, e = eps[t], all four from the OLD values
 *   f  <- (f  + softmin_e(C_xy, g,  b)) / 2        g  <- (g  + softmin_e(C_yx, f,  a)) / 2
 *   fx <- (fx + softmin_e(C_xx, fx, a)) / 2        gy <- (gy + softmin_e(C_yy, gy, b)) / 2
 * and the final step at e = eps[T - 1] is not averaged:
 *   f1 = softmin_e(C_xy, g, b)   g1 = softmin_e(C_yx, f, a)   fx1 = softmin_e(C_xx, fx, a)   gy1 = softmin_e(C_yy, gy, b)
 *
 *   loss[b]  = sum_i a_i (f1_i - fx1_i) + sum_j b_j (g1_j - gy1_j): the differences added in double, a thread taking every
 *              1024th row in ascending order, the threads of a wave by a butterfly, the waves in order; one rounding to fp32
 *   pot[b]   (n + m): f1 then g1, slots behind a count +0
 *   delta[b] = max(max_i |f1_i - f_i|, max_j |g1_j - g_j|): how far the cross potentials still moved in the last step, in
 *              units of cost -- the convergence read-out (NaN when loss is NaN)
 *   grad1 (b, n, 3), grad2 (b, m, 3), both given or both NULL: the gradient of loss through the final step only, the
 *              potentials before it and the column arguments held fixed:
 *                grad1_i = a_i (sum_j pi_ij d1C(x_i, y_j) - sum_k pix_ik d1C(x_i, x_k)),
 *                pi_ij = b_j exp((f1_i + g_j - C_ij) / e) -- the rows sum to 1 by construction: the numerators are carried
 *              beside the final soft-min's running sum and divided by it once -- pix the same with fx1, fx, a; grad2 the
 *              mirror image.  d1C = (x - y) / C for p = 1 and 0 where C = 0 (as rf_emd_assign_grad), x - y for p = 2.  Rows
 *              behind a count are +0.
 * The exponent is formed as (h_j - C_ij) (log2(e) / eps) -- the difference first, which is where the terms that matter
 * cancel -- and the sums are base 2 (v_exp_f32, v_log_f32) under a running maximum renewed once per 8 columns.
 *
 * Guarantees:
 *   - Purity: a sample's numbers are a function of its own valid points, p and the schedule.  Two calls return identical
 *     bits; sample i is bit for bit the call on [i : i + 1]; a ragged call is bit for bit the call on the sliced clouds.  The
 *     column structure of every sum is a function of the valid column count L alone: tiles of 256 columns from column 0,
 *     ceil(ceil(L / 256) / 4) consecutive tiles to a chunk, the chunks merged in ascending order -- whichever workgroup
 *     computed them.  The loss-only form returns the bits of the form with gradients.
 *   - Self distance: with xyz1 == xyz2 and len1 == len2 the loss is +0 and both gradients are +0 in every slot: the four
 *     problems run through one code path.
 *   - Finite in, finite out, as long as C log2(e) / eps is finite in fp32 for the largest cost (C / eps below 2e38).
 *   - Memory safety: every loop bound is a count.  A non-finite coordinate in a valid row gives NaN in that sample only.
 *
 * Workspace, each part rounded up to 256 bytes, with r = 2 b (n + m):  2 * 4 r  potentials, double-buffered  + 2 * 32 r
 * (max, sum) partials of every (row, chunk), double-buffered  + 48 r  the gradient numerators of the final step.
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n or
 * m outside 1 ... RF_SK_MAX_POINTS, b above 65535, p not 1 or 2, T outside 1 ... RF_SK_MAX_ITERS, a NULL eps, an eps[t]
 * that is not positive and finite, a NULL xyz1 / xyz2 / loss / pot / delta, exactly one of grad1 / grad2 given, a tensor
 * or count array not 4-byte aligned, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a workspace smaller
 * than rf_sinkhorn_workspace_bytes (0 for non-positive or unsupported sizes, positive otherwise).  All index arithmetic is
 * in size_t. */
#define RF_SK_MAX_POINTS 65536
#define RF_SK_MAX_ITERS 256
size_t rf_sinkhorn_workspace_bytes(int b, int n, int m);
int rf_sinkhorn(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, int p,
                const float *eps, int T, float *loss, float *pot, float *delta, float *grad1, float *grad2, void *workspace,
                size_t workspace_bytes, rf_stream_t stream);

/* ---- the Gridding layer and the Gridding loss: trilinear voxel grids, exact sums, with gradients -- */
/* The occupancy family of completion losses (GRNet): every point spreads its mass trilinearly over the eight vertices of
 * its cell of a regular grid, and the loss is the L1 difference of the two grids.  No correspondence, linear in the point
 * count, and the cost of one cloud does not depend on the size of the other.  xyz1 (b, n, 3), xyz2 (b, m, 3) fp32; len1 /
 * len2: device int32 (b) or NULL with rf_nn_distance_lengths' conventions -- read and clamped into [1, n] / [1, m] by the
 * kernels.  No host synchronisation, at most three launches on `stream`: a call can be captured in a HIP graph.
 *
 * Grid: R = res vertices per axis, 2 <= R <= RF_GR_MAX_RES; lo < hi finite floats, the same box on all three axes; vertex k
 * sits at lo + k h, h = (hi - lo) / (R - 1); the library forms inv_h = (float)((double)(R - 1) / ((double)hi - (double)lo))
 * on the host.  Per point and axis, all in fp32:
 *   u = (x - lo) * inv_h                        a subtraction, then a multiplication: two roundings
 *   inside iff u >= 0 && u <= (float)(R - 1)    on all three axes; a NaN fails.  Points outside and rows behind the count
 *                                               contribute nothing and get a gradient of exactly +0
 *   i = min((int)floorf(u), R - 2),  t = u - (float)i      t is exact, in [0, 1], and 1 on the upper face
 *   q1 = (int)rintf(t * 512.0f),  q0 = RF_GR_Q - q1
 * For d in {0, 1}^3 the weight on vertex (ix + dx, iy + dy, iz + dz) is the INTEGER W_d = q_dx(x) q_dy(y) q_dz(z) <= 2^27;
 * the eight weights of a point sum to exactly Q^3.  G(v) = sum over the points of W is an exact integer and mass is conserved
 * exactly: sum_v G(v) = inside * Q^3.
 *
 * rf_gridding_loss: with (mu1, mu2) = (1, 1) for RF_GR_COUNTS and (L2, L1), the clamped counts, for RF_GR_DENSITY,
 *   D(v) = mu1 G1(v) - mu2 G2(v), an int64: |D(v)| <= 2^16 2^16 2^27 = 2^59 and sum_v |D(v)| <= 2^60
 *   loss[b]   = (float)((double)sum_v |D| / Q^3 / R^3)                  COUNTS: the mean over the vertices (GRNet's L1Loss)
 *             = (float)((double)sum_v |D| / Q^3 / ((double)L1 * L2))    DENSITY: sum_v |G1 / L1 - G2 / L2|, in [0, 2]
 *   inside[b] (2) int32: the inside counts of the two clouds
 *   grad1 (b, n, 3), grad2 (b, m, 3), both given or both NULL.  With s(v) = sign(D(v)) in {-1, 0, 1}, w_k(0) = 1.0f - t_k and
 *   w_k(1) = t_k in fp32, sigma_a(d) = +1 if d_a = 1 else -1:
 *     grad1[i][a] = (float)((sum_{d = 0..7, dz fastest} (s(v_i + d) sigma_a(d)) (prod_{k != a} (double)w_k(d_k))) ((double)inv_h c1))
 *   the sum in double from +0, c1 = 1 / (double)R^3 (COUNTS) or 1 / (double)L1 (DENSITY); grad2 the same with -s and c2 = 1 / R^3
 *   or 1 / L2.  This is the analytic gradient of the unquantised trilinear loss under the signs of the quantised grid, 0 where
 *   D(v) = 0.  Each product of two fp32 factors is exact in double, so a fused multiply-add could not change a bit.
 *
 * rf_gridding: the Gridding layer itself.  grid (b, R, R, R) fp32, x slowest: v = (ix R + iy) R + iz, the value
 * (float)((double)G(v) / Q^3); every element is written, zeros where nothing fell.  inside (b) int32.
 * rf_gridding_grad: its backward.  grad_xyz[i][a] = (float)((double)inv_h sum_d (sigma_a(d) (double)gg[v_i + d]) (prod_{k != a}
 * (double)w_k(d_k))), the same order of d, the sum in double from +0; +0 for outside points and rows behind the count.
 *
 * Guarantees:
 *   - Purity: two calls return identical bits; sample i is bit for bit the call on [i : i + 1]; a ragged call is bit for bit
 *     the call on the sliced clouds; loss, grid and inside are bit-identical under any permutation of a cloud's points (the
 *     sums are integers); the loss-only form returns the bits of the form with gradients.
 *   - Self distance: loss(x, x) is +0 with all-zero gradients.
 *   - Memory safety: a non-finite coordinate never moves a memory access -- it is simply outside.  Every loop bound is a count.
 *   - No float atomics anywhere; no call uses hipMemset.
 *
 * Workspace, each part rounded up to 256 bytes, with nb = ceil(R / 16) bricks per axis:
 *   rf_gridding_loss   4 * 2 b (nb^3 + 1)  list starts  + 8 b (n + m)  one record per point  + 8 b nb^3  one partial per brick,
 *                      and with gradients  + b R^3  one sign byte per vertex
 *   rf_gridding        4 b (nb^3 + 1)  + 8 b n
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n or m
 * outside 1 ... RF_GR_MAX_POINTS, res outside 2 ... RF_GR_MAX_RES, b above 65535, a non-finite lo or hi or lo >= hi, an unknown
 * mode, a NULL xyz / loss / grid / inside / grad_grid / grad_xyz, exactly one of grad1 / grad2 given, a tensor or count array
 * not 4-byte aligned, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a workspace smaller than the
 * _workspace_bytes function states (0 for non-positive or unsupported sizes, positive otherwise).  All index arithmetic is in
 * size_t. */
#define RF_GR_Q 512
#define RF_GR_MAX_RES 256
#define RF_GR_MAX_POINTS 65536
#define RF_GR_COUNTS 0
#define RF_GR_DENSITY 1
size_t rf_gridding_loss_workspace_bytes(int b, int n, int m, int res, int want_grad);
int rf_gridding_loss(int b, int n, int m, int res, float lo, float hi, int mode, const float *xyz1, const float *xyz2,
                     const int *len1, const int *len2, float *loss, int *inside, float *grad1, float *grad2, void *workspace,
                     size_t workspace_bytes, rf_stream_t stream);
size_t rf_gridding_workspace_bytes(int b, int n, int res);
int rf_gridding(int b, int n, int res, float lo, float hi, const float *xyz, const int *len, float *grid, int *inside,
                void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_gridding_grad(int b, int n, int res, float lo, float hi, const float *xyz, const int *len, const float *grad_grid,
                     float *grad_xyz, rf_stream_t stream);

/* ---- Gridding Reverse and Cubic Feature Sampling: from a voxel grid back to points, with gradients -- */
/* The two GRNet layers behind the Gridding layer (cloud -> grid -> 3-D CNN -> cloud -> per-point refinement).  The grid
 * geometry is the gridding section's, verbatim: R = res vertices per axis, 2 <= R <= RF_GR_MAX_RES, the box [lo, hi]^3,
 * inv_h = (float)((double)(R - 1) / ((double)hi - (double)lo)) formed on the host, per axis u = (x - lo) * inv_h in fp32,
 * inside iff 0 <= u <= (float)(R - 1) on all three axes (a NaN fails), the cell i = min((int)floorf(u), R - 2), the vertex
 * index v = (ix R + iy) R + iz, the corners d in {0, 1}^3 with dz fastest: v + d = v + (dx R + dy) R + dz.  The library is
 * built with -ffp-contract=off: the double arithmetic below has exactly the roundings written.  Counts are device int32 (b)
 * or NULL with rf_nn_distance_lengths' conventions, clamped into [1, n] by the kernels.  No host synchronisation, no
 * hipMemset, no float atomics in global memory, a fixed number of launches on `stream` (forward 1, its backward 2; reverse
 * 3, its backward 1): every call can be captured in a HIP graph.
 *
 * rf_cubic_feature_sampling: xyz (b, n, 3) fp32, 1 <= n <= RF_GR_MAX_POINTS; vol (b, c, R, R, R) fp32, channel-first and
 * contiguous (what a 3-D convolution returns), 1 <= c <= RF_CFS_MAX_CHANNELS.
 *   feat (b, n, 8, c) fp32: for an inside point feat[s][i][d][ch] = vol[s][ch][v_i + d], a copy bit for bit (NaN payloads
 *   included); for a point outside the box and a row behind the count all 8 c floats are +0.  Every element is written.
 *   inside (b) int32: how many points of the sample are inside.
 * rf_cubic_feature_sampling_grad: grad_vol (b, c, R, R, R) from grad_feat (b, n, 8, c); grad_vol[s][ch][v] is the sum of
 * grad_feat[s][i][d][ch] over the (i, d) with v_i + d = v, i inside and below the count.  Every element is written exactly
 * once, +0 where nothing fell; the value is the fp32 rounding of a DOUBLE sum of the contributions.  THE ORDER OF THE
 * ADDITIONS IS NOT FIXED (it is the order in which the points arrive at a workgroup).  The promise: identical bits, for
 * every call and batch, whenever the double sum is exact (for instance integer-valued gradients with sums below 2^53);
 * otherwise |got - exact| <= 2^-23 |exact| + k 2^-52 sum |terms| for k contributions -- one fp32 rounding plus the double
 * sum's own roundings -- and two calls may differ within that.  The points get no gradient: the op is piecewise constant
 * in xyz, as in GRNet.  The backward takes xyz and len again and recomputes the cells; it takes no index tensor, so no
 * corrupt index can move a store.  Only GRNet's neighborhood_size = 1 (the eight vertices of the cell) is provided: larger
 * neighbourhoods are out of scope; trilinear (PVCNN-style) devoxelisation is rf_trilinear_devoxelize, in the next section.
 *
 * rf_gridding_reverse: grid (b, R, R, R) fp32, eps fp32 finite and > 0, compact 0 or 1.  There are M = (R - 1)^3 cells,
 * cell = (ix (R - 1) + iy) (R - 1) + iz with its first vertex v = (ix R + iy) R + iz.  Per cell, all in double:
 *   w_d = (double)grid[v + d]
 *   S   = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7                left to right from w_0
 *   T_x = ((w_4 + w_5) + w_6) + w_7,  T_y = ((w_2 + w_3) + w_6) + w_7,  T_z = ((w_1 + w_3) + w_5) + w_7
 *   valid iff S >= (double)eps && S < +inf         a NaN anywhere makes the cell invalid; negative entries may pass
 *   f_a = T_a / S,   p_a = (float)((double)lo + ((double)i_a + f_a) * h_d)
 * with h_d = ((double)hi - (double)lo) / (double)(R - 1) formed on the host.
 *   points (b, M, 3) fp32, row (b, M) int32: the row cell c was written to, -1 for an invalid cell; count (b) int32: the
 *   number of valid cells.  compact = 0: cell c writes row c, invalid rows are (+0, +0, +0).  compact = 1: the valid cells
 *   occupy the rows 0 ... count - 1 IN INCREASING CELL ORDER (an ordered scan, no atomics: the placement is a pure function
 *   of the grid) and the rows from count on are zeros.  Every element of all three outputs is written.  points and count
 *   are a padded batch with device counts: what the _lengths entries take.
 * rf_gridding_reverse_grad: grad_grid (b, R, R, R) from grid, row and grad_points gp (b, M, 3), every element written once:
 *   grad_grid[v] = (float) sum over the <= 8 cells c with v = v_c + d and row[c] in [0, M) of
 *                  (h_d / S_c) (((d_x - f_x(c)) gp[row[c]][0] + (d_y - f_y(c)) gp[row[c]][1]) + (d_z - f_z(c)) gp[row[c]][2])
 * in double from +0 with d ascending, rounded once; S_c and f_a(c) are recomputed from grid as above.  row is the forward's:
 * an entry outside [0, M) is treated as -1 and never moves a load.
 *
 * Guarantees: two calls return identical bits, sample i is bit for bit the call on [i : i + 1], a ragged call is bit for
 * bit the call on the sliced clouds and rows behind a count are never read -- for rf_cubic_feature_sampling_grad as far as
 * its promise above goes.  A non-finite coordinate never moves a memory access; every loop bound is a count.
 *
 * Workspace, each part rounded up to 256 bytes, with nb = ceil(R / 16):
 *   rf_cubic_feature_sampling_grad   4 b (nb^3 + 1)  list starts  + 8 b n  one record per point (its cell and its index)
 *   rf_gridding_reverse              4 b ceil(M / 256)  the valid cells per tile of 256 cells
 *
 * Argument rules, all checked before any HIP call, as for rf_gridding: RF_EINVAL for a negative size; then b == 0 is RF_OK;
 * RF_EINVAL for n outside 1 ... RF_GR_MAX_POINTS, c outside 1 ... RF_CFS_MAX_CHANNELS, res outside 2 ... RF_GR_MAX_RES, b
 * above 65535, a non-finite lo or hi or lo >= hi, eps not finite or not > 0, compact not 0 or 1, a NULL tensor (len may be
 * NULL), a tensor or count array not 4-byte aligned, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a
 * workspace smaller than the _workspace_bytes function states (0 for non-positive or unsupported sizes, positive
 * otherwise).  All index arithmetic is in size_t. */
#define RF_CFS_MAX_CHANNELS 1024
int rf_cubic_feature_sampling(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len,
                              const float *vol, float *feat, int *inside, rf_stream_t stream);
size_t rf_cubic_feature_sampling_grad_workspace_bytes(int b, int n, int res);
int rf_cubic_feature_sampling_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len,
                                   const float *grad_feat, float *grad_vol, void *workspace, size_t workspace_bytes,
                                   rf_stream_t stream);
size_t rf_gridding_reverse_workspace_bytes(int b, int res);
int rf_gridding_reverse(int b, int res, float lo, float hi, float eps, int compact, const float *grid, float *points,
                        int *row, int *count, void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_gridding_reverse_grad(int b, int res, float lo, float hi, const float *grid, const int *row,
                             const float *grad_points, float *grad_grid, rf_stream_t stream);

/* ---- the point-voxel pair: average voxelization and trilinear devoxelization, with gradients -- */
/* The two ops of the point-voxel networks (PVCNN blocks, Point-Voxel Diffusion, SPVCNN-style refiners): per-point feature
 * vectors are averaged into the voxel nearest to each point, a 3-D CNN works on the volume, and the volume is interpolated
 * back at every point.  The grid geometry is the gridding section's, verbatim: R = res vertices per axis,
 * 2 <= R <= RF_GR_MAX_RES, the box [lo, hi]^3, inv_h = (float)((double)(R - 1) / ((double)hi - (double)lo)) formed on the
 * host, per axis u = (x - lo) * inv_h in fp32, inside iff 0 <= u <= (float)(R - 1) on all three axes (a NaN fails), the
 * cell i = min((int)floorf(u), R - 2), t = u - (float)i exact in [0, 1], the vertex index v = (ix R + iy) R + iz, the corners
 * d in {0, 1}^3 with dz fastest: v + d = v + (dx R + dy) R + dz.  The lattice points of PVCNN's voxel grid are these
 * vertices.  New here: the NEAREST VERTEX of an inside point is k_a = i_a + (t_a >= 0.5f ? 1 : 0) per axis, always in
 * 0 ... R - 1 (a tie goes up), k = (kx R + ky) R + kz.
 *
 * Layout: point features are (b, n, c) fp32, as in rf_group_point; volumes are channel-first (b, c, R, R, R) fp32 and
 * contiguous (what a 3-D convolution takes and returns); 1 <= c <= RF_CFS_MAX_CHANNELS, 1 <= n <= RF_GR_MAX_POINTS.  Counts
 * are device int32 (b) or NULL with rf_nn_distance_lengths' conventions, clamped into [1, n] by the kernels.  The library is
 * built with -ffp-contract=off: the double arithmetic below has exactly the roundings written.  No host synchronisation, no
 * hipMemset, no float atomics in global memory, a fixed number of launches on `stream` (rf_voxelize_mean 2, its backward 1;
 * rf_trilinear_devoxelize 1, its backward 2, and 3 with grad_xyz): every call can be captured in a HIP graph.
 *
 * rf_voxelize_mean: from xyz (b, n, 3), len and feat (b, n, c):
 *   cnt (b, R, R, R) int32: cnt[k] = the number of inside points below the count whose nearest vertex is k.
 *   vol (b, c, R, R, R): vol[ch][k] = (float)(S / (double)cnt[k]) with S a DOUBLE sum of (double)feat[i][ch] over those
 *   points; +0 where cnt[k] = 0.
 *   inside (b) int32: how many points of the sample are inside; it is the sum of cnt.
 * Every element of all three outputs is written exactly once.  THE ORDER OF THE ADDITIONS IS NOT FIXED (it is the order in
 * which the points arrive at a workgroup), as for rf_cubic_feature_sampling_grad, and the promise is the same: identical
 * bits, for every call and batch, whenever the double sum is exact (for instance integer-valued features with sums below
 * 2^53); otherwise, with exact = (sum of the terms) / cnt in real arithmetic,
 *   |got - exact| <= 2^-23 |exact| + 2^-52 sum |terms|                    (results in fp32's normal range)
 * and two calls may differ within that.  Derivation: the double sum of cnt terms makes cnt - 1 roundings, so it is off by at
 * most (cnt - 1) u (1 + O(cnt u)) sum |terms| with u = 2^-53; divided by cnt that is below u sum |terms|.  The double division
 * adds at most u |exact| (1 + ...) and the rounding to fp32 at most 2^-24 of the quotient.  Together: at most
 * (2^-24 + 2 u + O(u 2^-24)) |exact| + (1 + 2^-24 + O(cnt u)) u sum |terms|, and both parentheses are below twice their
 * leading term for every cnt <= 2^16: hence 2^-23 and 2^-52.
 *
 * rf_voxelize_mean_grad: grad_feat (b, n, c) from grad_vol (b, c, R, R, R), xyz, len and the forward's cnt:
 *   grad_feat[i][ch] = (float)((double)grad_vol[ch][k_i] / (double)cnt[k_i])   for an inside point below the count with
 *   cnt[k_i] >= 1, and +0 for every other element.  A pure gather with prescribed bits: two calls return identical bits.  k_i
 * is recomputed from xyz; there is no index tensor, and whatever cnt holds moves no access.  The points get no gradient:
 * the op is piecewise constant in xyz.
 *
 * rf_trilinear_devoxelize: from xyz, len and vol (b, c, R, R, R).  With w_a(0) = 1.0f - t_a and w_a(1) = t_a in fp32 and
 *   W_d = ((double)w_x(d_x) * (double)w_y(d_y)) * (double)w_z(d_z)          (the first product is exact, the second rounds)
 *   feat[i][ch] = (float)(sum_{d = 0..7 ascending} W_d * (double)vol[ch][v_i + d])
 * the sum in double from +0, one rounding per product and per addition, rounded once to fp32; +0 for points outside the
 * box and rows behind the count.  feat (b, n, c), every element written; inside (b) int32.  A pure function with every
 * rounding written down: a float64 restatement matches it bit for bit on arbitrary finite inputs.
 *
 * rf_trilinear_devoxelize_grad: from xyz, len, vol and grad_feat gf (b, n, c).
 *   grad_vol (b, c, R, R, R): grad_vol[ch][v] is the fp32 rounding of a DOUBLE sum of the terms W_d(i) * (double)gf[i][ch]
 *   (each term rounded once, as a double product) over the (i, d) with v_i + d = v, i inside and below the count.  Every
 *   element is stored exactly once, +0 where nothing fell.  The order of the additions is not fixed; the promise is
 *   rf_cubic_feature_sampling_grad's: identical bits whenever the sum of the terms is exact, otherwise
 *   |got - exact| <= 2^-23 |exact| + k 2^-52 sum |terms| for k terms, exact being the exact sum of the prescribed terms.
 *   grad_xyz (b, n, 3) or NULL (then it is not computed and one launch fewer is made): with
 *     g_d = sum_{ch ascending} (double)gf[i][ch] * (double)vol[ch][v_i + d]         (every product exact, the sum from +0)
 *     grad_xyz[i][a] = (float)((double)inv_h * sum_{d ascending} (sigma_a(d) g_d) * (prod_{k != a} (double)w_k(d_k)))
 *   sigma_a(d) = +1 if d_a = 1 else -1, the sum in double from +0 as in rf_gridding_grad; +0 for points outside the box and
 *   rows behind the count.  A gather with prescribed bits.
 *
 * Guarantees: sample i is the call on [i : i + 1], a ragged call is the call on the sliced clouds, and rows behind a count
 * are never read -- bit for bit for the prescribed outputs, and as far as the promises above go for vol and grad_vol.  A
 * non-finite coordinate never moves a memory access: it is simply outside.  Every loop bound is a count.
 *
 * Workspace, each part rounded up to 256 bytes, with nb = ceil(R / 16), for rf_voxelize_mean and
 * rf_trilinear_devoxelize_grad alike:  4 b (nb^3 + 1)  list starts  + 8 b n  one record per point (its vertex or cell and
 * its index).
 *
 * Argument rules, all checked before any HIP call, as for rf_gridding: RF_EINVAL for a negative size; then b == 0 is RF_OK;
 * RF_EINVAL for n outside 1 ... RF_GR_MAX_POINTS, c outside 1 ... RF_CFS_MAX_CHANNELS, res outside 2 ... RF_GR_MAX_RES, b
 * above 65535, a non-finite lo or hi or lo >= hi, a NULL tensor (len and grad_xyz may be NULL), a tensor or count array not
 * 4-byte aligned, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a workspace smaller than the
 * _workspace_bytes function states (0 for non-positive or unsupported sizes, positive otherwise).  All index arithmetic is
 * in size_t.  Out of scope: PVCNN's coordinate normalisation (torch ops in front of the call), non-cubic boxes, and bit
 * parity with PVCNN's CUDA ops (torch.round's ties to even, float atomics). */
size_t rf_voxelize_mean_workspace_bytes(int b, int n, int res);
int rf_voxelize_mean(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const float *feat,
                     float *vol, int *cnt, int *inside, void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_voxelize_mean_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const int *cnt,
                          const float *grad_vol, float *grad_feat, rf_stream_t stream);
int rf_trilinear_devoxelize(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len,
                            const float *vol, float *feat, int *inside, rf_stream_t stream);
size_t rf_trilinear_devoxelize_grad_workspace_bytes(int b, int n, int res);
int rf_trilinear_devoxelize_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len,
                                 const float *vol, const float *grad_feat, float *grad_vol, float *grad_xyz,
                                 void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* ---- the vector attention pair: neighbour subtraction and neighbour aggregation, with gradients -- */
/* The two ops that transformer-style point networks (Point Transformer, SnowflakeNet's skip-transformer, PoinTr / AdaPoinTr,
 * SeedFormer) run on their neighbourhoods behind a kNN search -- pointops' `subtraction` and `aggregation`, here padded-batch
 * with counts instead of packed with offsets:
 *   sub[i][t][:] = q[i][:] - src[idx[i][t]][:]                                        (b, m, k, c)
 *   out[i][ch]   = sum_t (value[idx[i][t]][ch] + pos[i][t][ch]) * weight[i][t][ch mod cw]   (b, m, c); share_planes = c / cw
 * Everything is fp32, channel-last and contiguous.  idx is (b, m, k) int32: m queries with k slots each, naming rows of a
 * (b, n, c) tensor.  len1 (b) = valid source rows, len2 (b) = valid queries: device int32 arrays or NULL (= n, m), clamped into
 * [1, n] and [1, m] by the kernels as every count of this header.
 *
 * LIVENESS, one rule for all four entries: slot (i, t) is live iff i < len2', t < len1' and 0 <= idx[i][t] < len1' (the
 * primes: the clamped counts).  It is the rule of rf_knn_grad_lengths, so the idx of a ragged rf_knn_lengths -- zeros behind
 * a short sample's len1' neighbours, zero rows for padded queries -- and its two count arrays pass through unchanged.  A dead
 * slot's pos, weight, grad_out and whatever row its idx names never enter a result (they are dropped by a select, never by
 * a product: NaN there reaches nothing), and every output element that a dead slot or a padded row owns is written as +0.0.
 * Any int32 is allowed in idx.  A live non-finite input gives non-finite results in the same places; NaN payloads are not
 * promised.  The library is built with -ffp-contract=off: the arithmetic below has exactly the roundings written.
 *
 * rf_neighbor_sub: out (b, m, k, c): one fp32 subtraction per element of a live slot.  Bit for bit.
 *
 * rf_neighbor_sub_grad, from grad_out g (b, m, k, c); the features themselves are not needed:
 *   grad_q (b, m, c) or NULL:   grad_q[i][ch] = (float)(sum over the live t, ascending, of (double)g[i][t][ch]), the sum in double
 *   from +0.0.  Prescribed, bit for bit.
 *   grad_src (b, n, c) or NULL: grad_src[r][ch] = (float)(the double sum from +0.0 of the terms -(double)g[i][t][ch] over the live
 *   slots with idx[i][t] = r).  ORDER-FREE (below).  Every row is stored exactly once; rows nobody names are +0.0, and so is an
 *   exact zero.
 *
 * rf_neighbor_aggregate: 1 <= cw, cw divides c.  pos (b, m, k, c) or NULL, weight (b, m, k, cw).  Per live slot
 *   s = fl32(value[idx[i][t]][ch] + pos[i][t][ch])  (value[...] itself when pos is NULL),   acc = acc + (double)s * (double)w
 *   with w = weight[i][t][ch mod cw]: the product of two floats is exact in double, so there is one rounding per addition; t
 *   ascending from acc = +0.0; out[i][ch] = (float)acc.  A pure function with every rounding written down: a float64
 *   restatement matches it bit for bit.
 *
 * rf_neighbor_aggregate_grad, from grad_out g (b, m, c) and the forward's inputs; each output may be NULL and is then not computed:
 *   grad_pos (b, m, k, c):     grad_pos[i][t][ch] = fl32(g[i][ch] * w[i][t][ch mod cw]), one fp32 product.  Bit for bit.
 *   grad_weight (b, m, k, cw): grad_weight[i][t][j] = (float)(sum over q = 0 ... c / cw - 1, ascending, of
 *   (double)g[i][j + q cw] * (double)s[i][t][j + q cw]), s as in the forward, the sum in double from +0.0.  Bit for bit.
 *   grad_value (b, n, c):      grad_value[r][ch] = (float)(the double sum from +0.0 of the exact products
 *   (double)g[i][ch] * (double)w[i][t][ch mod cw] over the live slots with idx[i][t] = r).  ORDER-FREE.  Every row is stored
 *   exactly once, rows nobody names are +0.0.
 *
 * The ORDER-FREE sums (grad_src, grad_value): the order of the additions is the order in which a counting sort leaves the
 * slots of a row, which is not fixed.  Promise: identical bits, for every call and batch, whenever the double sum is exact
 * (for instance integer-valued terms with sums below 2^53); otherwise, for an element with K terms,
 *   |got - exact| <= 2^-23 |exact| + K 2^-52 sum |terms|                    (results in fp32's normal range)
 * with exact the sum of the prescribed terms in real arithmetic, and two calls may differ within that.  Derivation: a recursive
 * double sum of K terms makes K - 1 roundings, each of at most u = 2^-53 of a partial sum that is itself at most
 * (1 + (K - 1) u) sum |terms|: the sum is off by at most (K - 1) u (1 + O(K u)) sum |terms|, below K 2^-53 sum |terms| with room
 * to spare for every K <= 2^22 (m k at its largest), and the statement doubles it.  The rounding to fp32 adds at most 2^-24 of
 * the computed sum, that is 2^-24 |exact| + 2^-24 K 2^-53 sum |terms|; 2^-23 |exact| and the doubled second term cover both.
 *
 * Guarantees: sample i is the call on [i : i + 1]; a ragged call is the call on each sample's slices [: len1'], [: len2'],
 * with +0.0 in every element beyond (bit for bit for the prescribed outputs, as far as the promise goes for the order-free
 * ones); rows and slots behind a count are never used.  No host synchronisation, no hipMemset, no float atomics in
 * global memory, a fixed number of launches on `stream` for a given set of NULL outputs (rf_neighbor_sub 1;
 * rf_neighbor_sub_grad 1 for grad_q + 2 for grad_src; rf_neighbor_aggregate 1; rf_neighbor_aggregate_grad 1 for grad_pos
 * + 1 for grad_weight + 2 for grad_value): every call can be captured in a HIP graph.
 *
 * Workspace of the two _grad entries, needed only when grad_src / grad_value is asked for (otherwise no sort runs, and
 * `workspace` is not looked at), each part rounded up to 256 bytes:
 *   4 b (n + 1)  the rows' list starts  +  4 b m k  the slots in row order.
 * The two _workspace_bytes functions return that, and 0 outside the domain of (b, n, m, k).
 *
 * Domain: 1 <= b <= 65535, 1 <= n, m <= 65536, 1 <= k <= RF_VA_MAX_K, 1 <= c <= RF_VA_MAX_CHANNELS, cw >= 1 with c % cw == 0,
 * m k c < 2^31 and n c < 2^31 (32-bit offsets inside a sample).  Argument rules, all checked before any HIP call: RF_EINVAL for
 * a negative size; then b == 0 is RF_OK; RF_EINVAL for sizes outside the domain, a NULL tensor (len1, len2, pos and the
 * outputs of the _grad entries may be NULL), a tensor or count array not 4-byte aligned, and, where grad_src / grad_value is
 * asked for, a workspace that is NULL or not 16-byte aligned; RF_EWORKSPACE for a workspace smaller than stated.  Tensors at
 * 16-byte alignment with c % 4 == 0 take the float4 kernels; the results do not depend on it.  Out of scope: the softmax over
 * k in front of the aggregation (torch code, as in pointops), bf16 / fp16 channels, and packed (offset) batches. */
#define RF_VA_MAX_K 64
#define RF_VA_MAX_CHANNELS 1024
int rf_neighbor_sub(int b, int n, int m, int k, int c, const float *feat_q, const float *feat_src, const int *idx,
                    const int *len1, const int *len2, float *out, rf_stream_t stream);
size_t rf_neighbor_sub_grad_workspace_bytes(int b, int n, int m, int k);
int rf_neighbor_sub_grad(int b, int n, int m, int k, int c, const int *idx, const int *len1, const int *len2,
                         const float *grad_out, float *grad_q, float *grad_src, void *workspace, size_t workspace_bytes,
                         rf_stream_t stream);
int rf_neighbor_aggregate(int b, int n, int m, int k, int c, int cw, const float *value, const float *pos,
                          const float *weight, const int *idx, const int *len1, const int *len2, float *out,
                          rf_stream_t stream);
size_t rf_neighbor_aggregate_grad_workspace_bytes(int b, int n, int m, int k);
int rf_neighbor_aggregate_grad(int b, int n, int m, int k, int c, int cw, const float *value, const float *pos,
                               const float *weight, const int *idx, const int *len1, const int *len2, const float *grad_out,
                               float *grad_value, float *grad_pos, float *grad_weight, void *workspace,
                               size_t workspace_bytes, rf_stream_t stream);

/* ---- the exact earth mover's distance: optimal assignment with a certificate and gradients -- */
/* The one-to-one assignment of minimal total distance between two clouds of EQUAL counts, by a deterministic Jacobi
 * auction with eps-scaling on an integer cost grid: a pure function of its inputs with a machine-checkable optimality
 * certificate (a dual lower bound in exact integers).  xyz1 (b, n, 3) are the persons, xyz2 (b, n, 3) the objects, both
 * fp32; 1 <= n <= RF_EA_MAX_POINTS.  len: device int32 (b) or NULL, shared by both clouds, with rf_nn_distance_lengths'
 * conventions -- read and clamped into [1, n] by the kernel; L below is the clamped count, rows behind it never reach a
 * result.  max_rounds: 0 means 64 L + 1024.  No host synchronisation, one launch: a call can be captured in a HIP graph.
 * One workgroup works on a sample: spreading a sample over several workgroups, n above RF_EA_MAX_POINTS and unequal
 * counts (n != m) are out of scope.  Per sample:
 *
 *   1. Grid.  lo / hi per axis over the 2 L valid points in fp32, E = the largest of the three hi - lo.  E NaN or
 *      infinite (any non-finite valid coordinate, or an extent that overflows): status RF_EA_NONFINITE, match12 =
 *      match21 = the identity, the numbers unspecified, rounds = bids = k = 0; the other samples are unaffected and no
 *      memory access depends on a data value.  Otherwise frexpf(E) = (., ex) with ex = 0 for E = 0,
 *      k = 19 - max(ex, -100) and S = 2^k.
 *   2. Costs.  d_ij = sqrtf(((x1 - x2)^2 + (y1 - y2)^2) + (z1 - z2)^2), unfused fp32 with a correctly rounded square
 *      root; c_ij = (int)rintf(fminf(d_ij S, 2^20)).  The product is exact and c_ij < 2^20 (the fminf acts only where the
 *      squares overflow fp32, E >= 2^63: memory-safe and terminating there, the numbers unspecified).  Costs are
 *      recomputed on the fly: nothing of size n^2 is stored anywhere.
 *   3. Phases.  eps = 2^17, 2^14, 2^11, 2^8, 2^5, 2^2, 1: always seven.  Prices p_j are int32, start at 0 and carry over;
 *      every phase starts with all persons unassigned and all objects free.
 *   4. One round works on the prices and the unassigned set U as they are at its start.  Every i in U forms
 *      v_j = c_ij + p_j; j* minimises (v_j, (j - i) mod L) lexicographically (the rotating tie rule keeps collapsed or
 *      duplicated clouds from costing L rounds per phase); w = min_{j != j*} v_j (v_j* when L = 1); the bid is
 *      beta_i = p_j* + (w - v_j*) + eps.  Every object that received bids goes to the highest beta, ties to the lowest i;
 *      its price becomes that beta and its previous owner becomes unassigned.  A phase ends when U is empty; `rounds`
 *      counts rounds over all phases, `bids` the bids (saturating at 2^31 - 1).
 *   5. Cap.  If rounds reaches max_rounds while someone is unassigned: status RF_EA_CAPPED, and the unassigned persons
 *      in ascending i take the free objects in ascending j -- the result is still a permutation.
 *   6. Prices and values stay below 2^26 (emd_assign.hip's header gives the argument), so int32 suffices.
 *
 * Outputs.  match12 (b, n), match21 (b, n) int32: inverse permutations of [0, L).  dist (b, n): the unquantised
 * d_{i, match12[i]}.  Slots behind L are zeros (index 0, +0.0f).  val (b, 3): cost = sum_i dist_i summed in double in
 * index order and rounded once; gap = (P - D) / S; bound = (P - D + L) / S.  cert (b, 2) long long:
 * P = sum_i c_{i, match12[i]} and D = sum_i min_j (c_ij + p_j) - sum_j p_j with the final prices and one more sweep.
 * info (b, 4) int32: status, rounds, bids, k.  The workspace receives the final prices, int32 (b, n), valid slots only:
 * with them anyone can recompute D.
 *
 * Guarantees:
 *   - D <= OPT_int <= P always, for any prices (weak duality), OPT_int the optimum on the integer grid.
 *   - With status RF_EA_OK, P - D <= L: every phase ends in eps-complementary slackness and the last eps is 1.
 *   - In true distances cost - EMD <= bound up to the fp32 rounding of cost: the L / S pays for the quantisation (at
 *     most 1 / (2 S) per pair on either side).
 *   - Two calls return identical bits; sample i's outputs are those of the call on [i : i + 1].  No float atomics (the
 *     only atomics are a 64-bit integer maximum and a list counter in LDS, and no result depends on their order).
 *   - The kernel ends on any input: every loop is bounded by a count or by max_rounds.
 *
 * rf_emd_assign_grad: the gradients of cost under the fixed assignment, scaled by gcost (b).  grad1[i] = gcost *
 * ((x_i - y_a(i)) / d_i), a = match12, d recomputed as above: exactly 0 where d_i == 0 and exactly +0 behind L;
 * grad2[j] is the negative of its partner's term, read through match21.  The assignment is a permutation, so there are no
 * atomics; an index outside [0, L) is clamped into it.  grad1, grad2 (b, n, 3) fully overwritten.
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for
 * n < 1, n above RF_EA_MAX_POINTS, b above 65535, a NULL tensor, a tensor or count array not 4-byte aligned (cert: 8
 * bytes), a workspace that is NULL or not 16-byte aligned, a negative max_rounds; RF_EWORKSPACE for a workspace smaller
 * than rf_emd_assign_workspace_bytes (4 b n rounded up to 256 bytes; 0 for non-positive or unsupported sizes).  All
 * index arithmetic is in size_t.  rf_emd_assign_supported(n): 1 for 1 <= n <= RF_EA_MAX_POINTS, else 0. */
#define RF_EA_MAX_POINTS 4096
#define RF_EA_OK 0
#define RF_EA_CAPPED 1
#define RF_EA_NONFINITE 2
int rf_emd_assign_supported(int n);
size_t rf_emd_assign_workspace_bytes(int b, int n);
int rf_emd_assign(int b, int n, const float *xyz1, const float *xyz2, const int *len, int max_rounds, int *match12,
                  int *match21, float *dist, float *val, long long *cert, int *info, void *workspace,
                  size_t workspace_bytes, rf_stream_t stream);
int rf_emd_assign_grad(int b, int n, const float *xyz1, const float *xyz2, const int *match12, const int *match21,
                       const int *len, const float *gcost, float *grad1, float *grad2, rf_stream_t stream);

/* ---- the expansion penalty and minimum density sampling (the ops of MSN-style completion networks) -- */
/* rf_expansion_penalty: the surface is generated as P patches of S points; every patch gets its minimum spanning tree,
 * and the tree edges longer than alpha times the patch's mean edge are the penalty.  xyz (b, n, 3) fp32, n = P S, patch
 * p of a sample is rows [p S, (p + 1) S); 2 <= S <= RF_XP_MAX_PATCH; alpha finite and >= 0.  One launch, no workspace,
 * no atomics, no host synchronisation: a call can be captured in a HIP graph.  One workgroup works on a patch; ragged
 * counts per patch and patches above RF_XP_MAX_PATCH are out of scope.  Per patch, as a pure function of its S rows
 * (indices below are local to the patch, root = 0):
 *
 *   1. Status.  If any of the 3 S coordinates is NaN or +-Inf (exponent bits all ones): status RF_XP_NONFINITE,
 *      father[v] = v, length = dist = +0, mean = 0; the other patches are unaffected and no address depends on a data
 *      value.  Otherwise status RF_XP_OK.
 *   2. Distances.  d2(u, v) = ((dx dx) + (dy dy)) + (dz dz), unfused fp32 -- rf_emd_assign's d_ij without the root;
 *      symmetric bit for bit, >= 0 or +inf, never NaN.  Nothing of size S^2 is stored.
 *   3. Tree.  Prim from vertex 0: key[v] = d2(0, v), father[v] = 0.  S - 1 times: the next vertex u minimises
 *      (bits(key[v]), v) lexicographically over the vertices outside the tree (the unsigned bit order is the float
 *      order); then, for every v still outside, key[v] and father[v] are replaced by d2(u, v) and u only where
 *      d2(u, v) < key[v] -- strictly, so the earliest tree vertex keeps a tie.  Ties, duplicates and lattices give one
 *      defined tree.
 *   4. Lengths.  length[v] = sqrtf(key[v]) with the key v joined with, correctly rounded; length[0] = +0, father[0] = 0.
 *   5. Mean.  mean64 = (sum over v = 1 .. S - 1 ascending of (double)length[v]) / (double)(S - 1); mean = (float)mean64.
 *   6. Penalty.  dist[v] = length[v] where (double)length[v] > (double)alpha * mean64, else +0.
 *
 * Outputs: dist (b, n), length (b, n) fp32; father (b, n) int32 as CLOUD-level row indices (p S + local: inside the own
 * patch); mean (b, P) fp32; info (b, P) int32 status.  Two calls return identical bits; a sample's outputs are those of
 * the call on [i : i + 1], a patch's those of the call on the patch alone (n = S) with father shifted by p S.
 *
 * rf_expansion_penalty_grad: the gradient of sum_v gdist[v] dist[v] with the tree, the mean and the indicator held
 * constant.  For v with dist[v] != 0: f = father[v] - p S clamped into [0, S), l_v = sqrtf(d2(v, f)) recomputed,
 * t_v = gdist[v] * ((x_v - x_f) / l_v) per component in fp32 (0 where l_v == 0).  grad[w] = (float)(0.0 + [dist[w] != 0]
 * t_w - sum over v with dist[v] != 0 and f(v) = w, ascending v, of t_v), summed in double in that order and rounded once:
 * exactly +0 where nothing contributes.  No atomics.  grad (b, n, 3) fully overwritten.
 *
 * rf_mds: minimum density sampling.  xyz (b, n, 3), 1 <= n <= RF_MDS_MAX_POINTS; m >= 1 samples per cloud; sigma (b)
 * fp32 on the device; len: device int32 (b) or NULL with rf_nn_distance_lengths' conventions (clamped into [1, n] by the
 * kernel), L the clamped count.  One launch, no workspace, capturable.  Per sample:
 *
 *   1. Scale.  c64 = 1.4426950408889634 / (2.0 * (double)sigma * (double)sigma), c = (float)c64.  If !(sigma > 0), or
 *      c is 0 or inf: status RF_MDS_BADSIGMA and out[j] = j for j < mo.  Otherwise RF_MDS_OK.
 *   2. Count.  mo = min(m, L).  out[0] = 0.  Slots j >= mo are 0 (coordinates +0).
 *   3. Density.  dens[v] = +0 in fp32.  After choosing u, every valid v gets dens[v] += w(d2(u, v)), in the order of
 *      the choices; d2 as above.  w: s = d2 * c; w = 0 if !(s < 64.0f) (NaN and inf included); else k = floorf(s),
 *      f = s - k (exact), p = the degree-5 polynomial for 2^-f of rfnet_amd/csrc/msn_poly.hpp in Horner form,
 *      p = p * f + c_i with a separate fp32 multiply and add at every step from c5 down to c0, and w = ldexpf(p, -k)
 *      (exact).
 *   4. Choice.  The next sample minimises (bits(dens[v]), v) over the valid v not chosen yet.
 *
 * Outputs: out (b, m) int32; info (b) int32 status; new_xyz (b, m, 3) or NULL: the chosen rows of xyz (gather_point
 * fused).  Two calls return identical bits; a sample's outputs are those of the call on [i : i + 1].
 *
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for
 * S outside [2, RF_XP_MAX_PATCH], n < S or n % S != 0, alpha negative or not finite, b (n / S) above 2^31 - 1; for n
 * outside [1, RF_MDS_MAX_POINTS] or m < 1; for a NULL tensor (len and new_xyz may be NULL) or a tensor or count array
 * not 4-byte aligned.  All index arithmetic is in size_t.  rf_expansion_penalty_supported(n, S) and rf_mds_supported(n)
 * return 1 for sizes inside these ranges, else 0. */
#define RF_XP_MAX_PATCH 4096
#define RF_XP_OK 0
#define RF_XP_NONFINITE 1
#define RF_MDS_MAX_POINTS 16384
#define RF_MDS_OK 0
#define RF_MDS_BADSIGMA 1
int rf_expansion_penalty_supported(int n, int S);
int rf_expansion_penalty(int b, int n, int S, float alpha, const float *xyz, float *dist, int *father, float *length,
                         float *mean, int *info, rf_stream_t stream);
int rf_expansion_penalty_grad(int b, int n, int S, const float *xyz, const int *father, const float *dist,
                              const float *gdist, float *grad, rf_stream_t stream);
int rf_mds_supported(int n);
int rf_mds(int b, int n, int m, const float *xyz, const float *sigma, const int *len, int *out, int *info,
           float *new_xyz, rf_stream_t stream);

/* ----------------------------------------------------------- EMD (pc_distance) ---------- */
/* Replaces approxmatchLauncher(b,n,m,xyz1,xyz2,match,temp) (pc_distance/tf_approxmatch.cpp:141,
 * tf_approxmatch.cu:180-182).  xyz1 (b,n,3) "dataset", xyz2 (b,m,3) "query" (b <= 65535 for
 * every entry point of this section: the batch is a grid dimension); match is
 * (b,m,n) (tf_approxmatch.cpp:164).  The reference's `temp` (b,2(n+m)) becomes `workspace`
 * (larger: it keeps the per-level ratio vectors so that match is written once). */
size_t rf_approxmatch_workspace_bytes(int b, int n, int m, int nlevels /* 0 = reference's 10 */);
int rf_approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                   void *workspace, size_t workspace_bytes, rf_stream_t stream);
/* Same with an explicit annealing schedule (host array of `nlevels` values, each the
 * multiplier of d^2 inside exp(); the reference's is {-4^7..-4^-1, 0}, tf_approxmatch.cu:21-25). */
int rf_approxmatch_levels(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                          const float *levels_host, int nlevels, void *workspace,
                          size_t workspace_bytes, rf_stream_t stream);

/* The same op with its route pinned.  The reference's kernel loops over the samples of a batch independently
 * (tf_approxmatch.cu:13), so a sample's match does not depend on the batch it is called in.  RF_EMD_AUTO (what rf_approxmatch /
 * rf_approxmatch_levels / rf_earth_mover pass) picks launch shapes and routes by the size of the WHOLE batch: from 6e7 pairs on
 * the sharp levels' sweeps take their rows in spatial order and skip columns, and the column segments of a sweep follow b --
 * every route within the op's tolerances, but the bits of sample i may differ between a call on the batch and a call on that
 * sample alone.  RF_EMD_SWEPT pins the route: every level a dense sweep over the clouds in the caller's order, launch shapes
 * those of a batch of one -- sample i's match (and rf_earth_mover_mode's cost) is bit-identical whatever the batch around it or
 * the shard it lands in (what a loss compared across differently sharded runs wants; C4 costs ~1.5x the time).
 * levels_host == NULL with nlevels == 0: the reference schedule. */
#define RF_EMD_AUTO 0
#define RF_EMD_SWEPT 1
size_t rf_approxmatch_mode_workspace_bytes(int b, int n, int m, int nlevels /* 0 = reference's 10 */, int mode);
int rf_approxmatch_mode(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                        const float *levels_host, int nlevels, void *workspace, size_t workspace_bytes,
                        rf_stream_t stream, int mode);

/* Replaces matchcostLauncher (tf_approxmatch.cpp:142, tf_approxmatch.cu:226-228): cost (b). */
size_t rf_matchcost_workspace_bytes(int b, int n, int m);
int rf_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                 float *cost, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* Replaces matchcostgradLauncher (tf_approxmatch.cpp:143, tf_approxmatch.cu:292-295):
 * grad1 (b,n,3), grad2 (b,m,3), fully overwritten. */
int rf_matchcost_grad(int b, int n, int m, const float *xyz1, const float *xyz2,
                      const float *match, float *grad1, float *grad2, rf_stream_t stream);

/* ------------------------------------------------------- sampling (tf_ops/sampling) ------ */
/* Replaces farthestpointsamplingLauncher(b,n,m,inp,temp,out) (tf_sampling.cpp:94,
 * tf_sampling_g.cu:203-205).  inp (b,n,3); out (b,m) int32; temp: caller scratch of
 * b*n floats, used only when n exceeds the register-resident limit (may be NULL otherwise,
 * see rf_farthestpointsampling_temp_floats). */
size_t rf_farthestpointsampling_temp_floats(int b, int n);
int rf_farthestpointsampling(int b, int n, int m, const float *inp, float *temp, int *out,
                             rf_stream_t stream);

/* The op with caller scratch of a stated size -- the entry point a binding should prefer: for clouds of 4097..16384 points from
 * 256 samples on (2049..4096 points: from 512) it sorts the cloud into the workspace and samples over the sorted cloud (rf_farthestpointsampling_sorted
 * below: the same indices, iterations a quarter shorter), otherwise it is rf_farthestpointsampling with `workspace` as `temp`.
 * workspace: rf_farthestpointsampling_workspace_bytes(b, n, m) bytes, 16-byte aligned (may be NULL when that is 0). */
size_t rf_farthestpointsampling_workspace_bytes(int b, int n, int m);
int rf_farthestpointsampling_ws(int b, int n, int m, const float *inp, void *workspace, size_t workspace_bytes, int *out,
                                rf_stream_t stream);

/* The same op (same indices, bit for bit) over the spatially sorted cloud: the call sorts the cloud into `workspace`
 * (rf_farthestpointsampling_sorted_workspace_bytes(b, n) bytes, 16-byte aligned) and a new sample then only re-scans the
 * regions it can still change (sampling.hip fps_sorted_kernel).  1024 < n <= 16384, m <= the kernel's capacity (1024 x 2, 4, 8 or 16 points: the power of two that holds n).  form: reserved (0).
 * new_xyz (b, m, 3), may be NULL: the samples' coordinates. */
size_t rf_farthestpointsampling_sorted_workspace_bytes(int b, int n);
int rf_farthestpointsampling_sorted(int b, int n, int m, int form, const float *inp, void *workspace,
                                    size_t workspace_bytes, int *out, float *new_xyz, rf_stream_t stream);

/* ---- ragged batches: per-sample point counts (sampling, grouping, neighbour search) --------
 * The conventions of rf_nn_distance_lengths, for the ops that run BEFORE the losses on the same padded clouds.  A count argument
 * (len, len1, len2, len_out) is a DEVICE int32 array of b values or NULL ("all"), 4-byte aligned; the kernels read it themselves
 * (no host synchronisation: every call captures into a HIP graph and a replay sees new counts) and CLAMP a value outside its
 * domain into [1, n] (resp. [1, m]), so a bad count can never make a kernel read or write outside the tensors.
 *   - Valid slots are bit for bit what the plain entry point returns when called on that sample's unpadded slices alone (ties,
 *     non-finite inputs and every documented quirk of the plain op included).
 *   - Nothing in the padding reaches a result, whatever it holds (NaN, inf, 1e30, copies of valid points).
 *   - PADDED OUTPUT SLOTS ARE ZEROS: index outputs 0, counts 0, floats +0.0f.  Deliberately not Chamfer's idx = -1: the index
 *     outputs of this family feed gathers that do not range-check (rf_grouppoint, rf_gatherpoint, rf_threeinterpolate), and the
 *     library already writes 0 for a row without a result (rf_sample_and_group's empty balls).  The counts say what is valid.
 *   - The work shrinks with the counts; with all counts NULL or full the results equal the plain op's.
 *   - Before any HIP call: RF_EINVAL for a negative or zero size (b == 0 is RF_OK), a NULL tensor, a misaligned count array,
 *     tensor (4 bytes) or workspace (16 bytes); RF_EWORKSPACE for a workspace smaller than the matching _workspace_bytes.
 *
 * rf_farthestpointsampling_lengths: len = valid points per cloud; len_out (may be NULL) = how many samples each cloud wants,
 * clamped into [1, m]: the cloud's chain of dependent iterations stops there (this is where ragged FPS saves time) and the tail
 * of its row is zeros.  FPS is prefix-stable, so out[i, :len_out[i]] are the first len_out[i] samples of rf_farthestpointsampling
 * on inp[i, :len[i]]; m > len[i] is legal and gives what the plain op gives there (point 0 repeated once every point is taken).
 * new_xyz (b, m, 3) or NULL: the samples' coordinates (zeros behind len_out).  Kernels and workspace are chosen by the padded
 * (n, m) exactly as rf_farthestpointsampling_ws chooses them; workspace may be NULL when the size query returns 0. */
size_t rf_farthestpointsampling_lengths_workspace_bytes(int b, int n, int m);
int rf_farthestpointsampling_lengths(int b, int n, int m, const float *inp, const int *len, const int *len_out,
                                     void *workspace, size_t workspace_bytes, int *out, float *new_xyz, rf_stream_t stream);

/* Replaces gatherpointLauncher (tf_sampling.cpp:125, tf_sampling_g.cu:206-208). */
int rf_gatherpoint(int b, int n, int m, const float *inp, const int *idx, float *out,
                   rf_stream_t stream);
/* Replaces scatteraddpointLauncher + the cudaMemset before it (tf_sampling.cpp:150,174). */
int rf_scatteraddpoint(int b, int n, int m, const float *out_g, const int *idx, float *inp_g,
                       rf_stream_t stream);

/* ------------------------------------------------------- grouping (tf_ops/grouping) ------ */
/* Replaces queryBallPointLauncher(b,n,m,radius*,nsample,xyz1,xyz2,idx,pts_cnt)
 * (tf_grouping.cpp:67, tf_grouping_g.cu:125-128).  xyz1 (b,n,3) dataset, xyz2 (b,m,3)
 * queries; idx (b,m,nsample), pts_cnt (b,m).  The reference passes `radius` as a device
 * pointer to one float (an op input tensor); here it is passed by value.  Rows with an
 * empty ball are left untouched, as in the reference. */
int rf_queryballpoint(int b, int n, int m, float radius, int nsample, const float *xyz1,
                      const float *xyz2, int *idx, int *pts_cnt, rf_stream_t stream);
/* The reference's exact signature: `radius_dev` is a DEVICE pointer to one float, the op's input
 * tensor (tf_grouping.cpp:18,93-95; queryBallPointLauncher(b,n,m,radius*,...), :67).  A TF-side
 * binder passes the tensor's buffer straight through: no D2H copy, no stream synchronisation.
 * Same results as rf_queryballpoint for the same radius value. */
int rf_queryballpoint_dev(int b, int n, int m, const float *radius_dev, int nsample,
                          const float *xyz1, const float *xyz2, int *idx, int *pts_cnt,
                          rf_stream_t stream);

/* The same op (same idx and pts_cnt, bit for bit) for datasets of 64 .. 65536 points and nsample <= 64, with
 * caller scratch: the dataset is put in sort-tile-recursive order once (or comes as an rf_nn_sort handle in
 * `sorted1`, NULL otherwise) and every query tests only the 64-record blocks whose box lies within the radius,
 * then keeps the nsample lowest ORIGINAL indices in ascending order (tf_grouping_g.cu:18-33); queries whose ball
 * reaches a large share of the cloud, non-finite queries and clouds with a non-finite point walk the cloud in index
 * order inside the same launch.  radius_dev: NULL (use `radius`) or the reference's device scalar (then `radius` is
 * ignored).  RF_EINVAL outside that domain: use rf_queryballpoint there.  A TF-side binder allocates the scratch
 * with allocate_temp, as tf_sampling.cpp:115 does for FPS. */
size_t rf_queryballpoint_boxes_workspace_bytes(int b, int n);
int rf_queryballpoint_boxes(int b, int n, int m, float radius, const float *radius_dev, int nsample,
                            const float *xyz1, const float *xyz2, const void *sorted1, int *idx, int *pts_cnt,
                            void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* query_ball_point over a ragged batch (the conventions of the "ragged batches" block of the sampling section): len1 = points per
 * dataset, len2 = queries per sample.  idx / pts_cnt on the valid queries are rf_queryballpoint's on xyz1[i, :len1[i]] and
 * xyz2[i, :len2[i]] -- except that, unlike rf_queryballpoint, EVERY row is written: an empty ball and a padded query are
 * idx = 0 ..., pts_cnt = 0.  radius_dev: NULL (use `radius`) or the reference's device scalar.  form: RF_GROUP_AUTO (the boxed
 * kernel for padded datasets of 2048 points and more inside its domain, what the Python wrapper applies to the plain op),
 * RF_GROUP_SCAN (every size; no workspace) or RF_GROUP_BOXES (64 <= n <= 65536, nsample <= 64, b <= 65535 on the PADDED sizes,
 * else RF_EINVAL; a count below 64 is fine); same results.  workspace: rf_queryballpoint_lengths_workspace_bytes(b, n, m,
 * nsample, form) bytes (0: may be NULL).  No sorted handle: a handle was sorted without counts. */
#define RF_GROUP_AUTO 0
#define RF_GROUP_SCAN 1
#define RF_GROUP_BOXES 2
size_t rf_queryballpoint_lengths_workspace_bytes(int b, int n, int m, int nsample, int form);
int rf_queryballpoint_lengths(int b, int n, int m, float radius, const float *radius_dev, int nsample, const float *xyz1,
                              const float *xyz2, const int *len1, const int *len2, int *idx, int *pts_cnt, void *workspace,
                              size_t workspace_bytes, rf_stream_t stream, int form);

/* The set-abstraction chain of BASELINE.json configs[2] as ONE call on caller buffers:
 *     fps_idx = farthest_point_sample(npoint, xyz)          (tf_sampling_g.cu:105-170)
 *     new_xyz = gather_point(xyz, fps_idx)                  (tf_sampling_g.cu:172-181)
 *     idx, pts_cnt = query_ball_point(radius, nsample, xyz, new_xyz)   (tf_grouping_g.cu:3-36)
 *     grouped_xyz = group_point(xyz, idx)                   (tf_grouping_g.cu:40-57)
 * with the results of the four separate entry points, bit for bit (rows of empty balls -- impossible for radius > 1e-20,
 * every sample lies in its own ball -- are written as index 0 instead of being left untouched, because the grouping reads
 * them).  xyz (b,n,3) with 64 <= n <= 65536, nsample <= 64; fps_idx (b,npoint) int32, new_xyz (b,npoint,3), idx
 * (b,npoint,nsample) int32, pts_cnt (b,npoint) int32, grouped_xyz (b,npoint,nsample,3).  radius_dev: NULL or the reference's
 * device scalar.  Two launches on `stream` (FPS writes new_xyz itself, the ball query writes grouped_xyz itself) plus the
 * dataset's sort, which runs on `aux_stream` beside FPS when one is given (NULL: on `stream`, before FPS); the call creates
 * and releases the two events that order the streams, keeps no state and is graph-capturable.  A TF-side op for a fused
 * "SampleAndGroup" would bind this with its four outputs from allocate_output and the scratch from allocate_temp. */
size_t rf_sample_and_group_workspace_bytes(int b, int n);
int rf_sample_and_group(int b, int n, int npoint, float radius, const float *radius_dev, int nsample, const float *xyz,
                        int *fps_idx, float *new_xyz, int *idx, int *pts_cnt, float *grouped_xyz, void *workspace,
                        size_t workspace_bytes, rf_stream_t stream, rf_stream_t aux_stream);

/* rf_sample_and_group over a ragged batch: rf_farthestpointsampling_lengths (len, len_out) and rf_queryballpoint_lengths (boxed
 * form, len1 = len, len2 = len_out) chained exactly as rf_sample_and_group chains the plain ops -- FPS writes new_xyz, the boxed
 * query writes grouped_xyz, one sort shared by both or beside FPS on aux_stream, graph-capturable; same domain on the PADDED
 * sizes (64 <= n <= 65536, nsample <= 64, b <= 65535).  Results: those of the two ragged entries called separately, bit for bit;
 * rows of samples behind len_out[i] are zeros in all five outputs (grouped_xyz +0.0f). */
size_t rf_sample_and_group_lengths_workspace_bytes(int b, int n);
int rf_sample_and_group_lengths(int b, int n, int npoint, float radius, const float *radius_dev, int nsample, const float *xyz,
                                const int *len, const int *len_out, int *fps_idx, float *new_xyz, int *idx, int *pts_cnt,
                                float *grouped_xyz, void *workspace, size_t workspace_bytes, rf_stream_t stream,
                                rf_stream_t aux_stream);

/* Replaces groupPointLauncher / groupPointGradLauncher (tf_grouping.cpp:146,177,208).
 * points (b,n,c); idx (b,m,nsample); out / grad_out (b,m,nsample,c); grad_points (b,n,c)
 * zero-filled here. */
int rf_grouppoint(int b, int n, int c, int m, int nsample, const float *points, const int *idx,
                  float *out, rf_stream_t stream);
int rf_grouppoint_grad(int b, int n, int c, int m, int nsample, const float *grad_out,
                       const int *idx, float *grad_points, rf_stream_t stream);
/* The gradient with caller scratch -- the entry point a binding should prefer.  The reference's form (one atomicAdd per element
 * into the zeroed tensor, tf_grouping_g.cu:61-78) is bound by the L2's float-atomic rate on this chip; given
 * rf_grouppoint_grad_workspace_bytes(b, n, c, m, nsample) bytes of 16-byte aligned scratch (0: the shape stays on the atomics, pass
 * NULL) the slots are counting-sorted by destination row and every row of grad_points is written once, from sums in double:
 * no zero fill, no atomics on memory, the same values to fp32 rounding whatever the order (scatter_rows.hip).  Slots whose index
 * is outside [0, n) add to no row.  With workspace == NULL or too small: rf_grouppoint_grad. */
size_t rf_grouppoint_grad_workspace_bytes(int b, int n, int c, int m, int nsample);
int rf_grouppoint_grad_ws(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                          float *grad_points, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* Replace knn_point (tf_ops/grouping/tf_grouping.py:48-73: dist = sum((xyz1 - xyz2)^2), then tf.nn.top_k(-dist, k), pure
 * TF ops in the reference).  xyz1 (b,n,3) candidates, xyz2 (b,m,3) queries; val (b,m,k) = -d float32 and idx (b,m,k) int32:
 * per query the k candidates of smallest d = ((dx*dx)+(dy*dy))+(dz*dz) (fp32, unfused, dx = x1 - x2), ascending by
 * (d, index) -- ties go to the lower index, top_k's rule.  A NaN distance ranks before every number and +inf after every
 * finite one (the order torch.topk(-dist) gives): a query with a NaN coordinate gets idx 0..k-1, val NaN.
 * Domain: 1 <= k <= min(n, 64), 1 <= n, m <= 65536, 1 <= b <= 65535; anything else is RF_EINVAL (checked before any HIP call).
 * rf_knn: every candidate against every query (knn.hip knn_scan_kernel). */
int rf_knn(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx, rf_stream_t stream);
/* The same op over spatially sorted copies of the two sets (rf_nn_sort), as rf_threenn_boxes: a wave of 64 neighbouring
 * queries visits only the 16-point candidate blocks whose box can still hold one of its k nearest.  val / idx bit-identical
 * to rf_knn, ties and non-finite values included (a sample with a non-finite coordinate is searched without the boxes).
 * sorted1 / sorted2: rf_nn_sort handles of xyz1 / xyz2 or NULL (sorted here, into the workspace), 16-byte aligned.
 * workspace: rf_knn_boxes_workspace_bytes(b, n, m) bytes, 16-byte aligned (0 = outside the domain); a shorter one is
 * RF_EWORKSPACE. */
size_t rf_knn_boxes_workspace_bytes(int b, int n, int m);
int rf_knn_boxes(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const void *sorted1, const void *sorted2,
                 float *val, int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream);
/* The gradient of val (tf_grouping.py:48-73 through top_k's gradient): with g = grad_val (b,m,k) and i = idx[b][j][t],
 * grad_xyz2[j] = sum_t 2 g (x1[i] - x2[j]) and grad_xyz1[i] = -(the same terms summed over the slots that name i).  Both are
 * fully overwritten (a candidate no slot names: zeros); the scatter is a counting sort of the m k slots by candidate, every row
 * written once from sums in double (scatter_rows.hip), so the values do not depend on the slots' order beyond fp32 rounding.
 * Slots whose index is outside [0, n) add nothing.  Same domain as rf_knn; workspace: rf_knn_grad_workspace_bytes(b, n, m, k)
 * bytes, 16-byte aligned. */
size_t rf_knn_grad_workspace_bytes(int b, int n, int m, int k);
int rf_knn_grad(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *idx, const float *grad_val,
                float *grad_xyz1, float *grad_xyz2, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* knn_point over a ragged batch (the conventions of the "ragged batches" block of the sampling section; RF_GROUP_* forms as
 * rf_queryballpoint_lengths, RF_GROUP_AUTO by the Python wrapper's thresholds on the padded sizes): len1 = candidates per
 * sample, len2 = queries.  k <= min(n, 64) is checked on the host against the PADDED n; a sample with len1[i] < k (only the
 * device knows) gets its len1[i] neighbours in slots [0, len1[i]) of every valid row, identical to rf_knn called with
 * k = len1[i] on the slices, and zeros behind; rows of padded queries are zeros (val +0.0f, idx 0).  rf_knn_grad_lengths: the
 * slots of padded queries, the slots t >= len1[i] and slots naming a candidate behind len1[i] contribute nothing, whatever idx
 * and grad_val hold there; rows of padded candidates and padded queries are exactly +0.0f; valid rows are rf_knn_grad's on the
 * slices (fp32 rounding of sums in double).  b == 0 is RF_OK. */
size_t rf_knn_lengths_workspace_bytes(int b, int n, int m, int k, int form);
int rf_knn_lengths(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *val,
                   int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream, int form);
size_t rf_knn_grad_lengths_workspace_bytes(int b, int n, int m, int k);
int rf_knn_grad_lengths(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                        const int *idx, const float *grad_val, float *grad_xyz1, float *grad_xyz2, void *workspace,
                        size_t workspace_bytes, rf_stream_t stream);

/* ---- k-nearest neighbours in FEATURE space: the dynamic graph of DGCNN's EdgeConv ------------
 * knn_point's argument order in c dimensions: feat1 (b,n,c) candidates, feat2 (b,m,c) queries; val (b,m,k) float32 and
 * idx (b,m,k) int32.  No (b,m,n) tensor is formed: the inner products come from the fp32-input matrix instruction
 * (v_mfma_f32_32x32x2_f32, an fp32 fmaf chain in ascending k) and every query keeps its k best in registers (knn_feature.hip).
 * The distance is the formula DGCNN uses, |q|^2 + |x|^2 - 2 q.x, every operation prescribed, all in fp32:
 *   ip[j][i]: acc = +0; for ch = 0 .. c-1 ascending: acc = fmaf(feat2[j][ch], feat1[i][ch], acc);
 *             the matrix instruction's K is 2, so an odd c is padded with one channel of zeros: acc = fmaf(+0, +0, acc);
 *   sq1[i], sq2[j]: acc = +0; for ch ascending: acc = fmaf(x[ch], x[ch], acc);
 *   d[j][i] = fmaf(-2, ip[j][i], sq2[j] + sq1[i]), the sum rounded to fp32 first.
 * d is NOT the rounded squared distance: under cancellation it can be slightly negative, so a row that queries itself is not
 * guaranteed slot 0 among near-duplicates (the formula's property, DGCNN's included).  d is never -0 (the sum is >= +0).
 * Result: per query the k smallest by (d, index), ascending -- ties go to the lower index; -0 orders as +0; a NaN distance
 * ranks before everything (knn_point's rule), -inf before the finite values and +inf after them.  val = -d, -NaN for a NaN.
 * Ragged batches, knn_point's rule exactly: len1 = candidates per sample, len2 = queries, device arrays of b ints clamped into
 * [1, n] / [1, m] (either may be NULL; both NULL: a dense batch), read on the device with no host synchronisation.  The list is
 * opened for kv = min(k, len1[i]); slots [kv, k) and the rows of padded queries are zeros (+0.0f, index 0); rows behind a count
 * may hold anything, NaN included.  The result is a pure function of a sample's own valid rows: two calls return the same bits, a
 * sample does not depend on its batch, a ragged call equals the call on the slices.
 * Domain: 1 <= k <= min(n, 64), 1 <= n, m <= 65536, 1 <= b <= 65535, 1 <= c <= 2048; anything else is RF_EINVAL before any HIP
 * call, as is a NULL tensor, a tensor or count array not 4-byte aligned and a NULL or not 16-byte aligned workspace.  workspace:
 * rf_knn_feature_workspace_bytes(b, n, m, c, k) bytes (the squared norms; 0 = outside the domain); a shorter one is
 * RF_EWORKSPACE and nothing is touched.  Two launches on `stream`. */
size_t rf_knn_feature_workspace_bytes(int b, int n, int m, int c, int k);
int rf_knn_feature(int b, int n, int m, int c, int k, const float *feat1, const float *feat2, const int *len1, const int *len2,
                   float *val, int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* ---- surface normals: PCA of every point's k-neighbourhood, and normal consistency -----------
 * rf_local_pca: per query the eigen-decomposition of the covariance of the points its idx row names (normals.hip).
 * xyz (b,n,3) the source points; idx (b,m,k) int32 what rf_knn* returned for m queries -- for one cloud knn_point of the
 * cloud against itself, the point itself included.  The query coordinates are not an argument: the covariance is taken about
 * the neighbourhood's own mean.  viewpoint (b,3) or NULL.  normals (b,m,3); eigenvalues (b,m,3) ascending; axes (b,m,3,3) or
 * NULL: the three eigenvectors as rows, in the order of the eigenvalues.
 * Ragged batches, knn_point's rule exactly: len1 = source points per sample, len2 = queries, device arrays of b ints clamped
 * into [1, n] / [1, m] (either may be NULL), read on the device.  kv = min(k, len1[i]) slots of a row are live; a live slot
 * whose index is outside [0, len1[i]) is skipped and does not count towards kv', the number of slots used; kv' == 0 is a
 * non-finite neighbourhood (below).  Rows j >= len2[i] are written as zeros and their idx rows are not read; source rows
 * behind len1[i] are not read.
 * The arithmetic per query, everything in double, every product, sum, quotient and root one separately rounded operation,
 * slots in ascending t:
 *   1. mean        s = +0.0; s = s + (double)x_t per axis; mu = s / (double)kv'.
 *   2. covariance  d_t = (double)x_t - mu; for the six entries of the upper triangle acc = +0.0; acc = acc + (d_a * d_b);
 *                  C_ab = acc / (double)kv'.  If any of the six is not finite the neighbourhood is NON-FINITE: eigenvalues =
 *                  three canonical quiet NaNs (0x7fc00000), normals and axes = +0, and nothing else is computed.
 *   3. cyclic Jacobi, exactly 6 sweeps from A = C, V = I; a sweep rotates the pairs (p,q) = (0,1), (0,2), (1,2) in that
 *      order; a pair with A_pq == 0 is skipped, otherwise
 *        theta = (A_qq - A_pp) / (2.0 * A_pq);  t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0))
 *        (no branch: theta * theta = inf gives t = +-0);  c = 1.0 / sqrt(t * t + 1.0);  s = t * c;  h = t * A_pq;
 *        A_pp = A_pp - h;  A_qq = A_qq + h;  A_pq = 0;  with r the third index
 *        (A_rp, A_rq) <- (c * A_rp - s * A_rq, s * A_rp + c * A_rq) from the old values, and for each row i of V
 *        (V_ip, V_iq) <- (c * V_ip - s * V_iq, s * V_ip + c * V_iq).
 *      (A numpy restatement leaves every off-diagonal entry exactly 0 after the sixth sweep on planes, lines, duplicates,
 *      balls and clouds scaled by 1e18 and 1e-30: tests/test_normals_host.py.)
 *   4. order       eigenvalue w is A_ww, its vector column w of V; ascending by (value, w).  A tiny negative smallest
 *                  eigenvalue is returned as it is.
 *   5. sign        every vector gets the canonical sign: its component of largest magnitude positive, a tie to the lowest
 *                  axis, a zero vector as it is (negation only: no rounding).  With a viewpoint v the NORMAL ONLY (vector 0)
 *                  is then negated when ((v_x - mu_x) * n_x + (v_y - mu_y) * n_y) + (v_z - mu_z) * n_z < 0; row 0 of axes
 *                  follows it.
 *   6. store       every output is the double rounded once to fp32.
 * One launch, no workspace, no host synchronisation (capturable); two calls return the same bits, a sample does not depend
 * on its batch, a ragged call equals the call on the slices.
 * Domain: 1 <= k <= 64, 1 <= n, m <= 65536, 1 <= b <= 65535 (b == 0 is RF_OK); anything else is RF_EINVAL before any HIP
 * call, as is a NULL tensor (len1, len2, viewpoint and axes may be NULL) and a tensor or count array not 4-byte aligned.
 *
 * rf_nn_normal_consistency: nrm1 (b,n,3) / nrm2 (b,m,3) the normals of two clouds, idx1 (b,n) / idx2 (b,m) the indices of
 * rf_nn_distance_lengths; len1 / len2 as there.  out (b,4), L1 / L2 the clamped counts:
 *   0  abs12    = (1/L1) sum_{j < L1} |n1[j] . n2[idx1[j]]|        1  abs21, the other direction (over L2)
 *   2  signed12 = (1/L1) sum_{j < L1}  n1[j] . n2[idx1[j]]         3  signed21
 * The dot is ((a_x b_x) + (a_y b_y)) + (a_z b_z) on the values widened to double; the sum is in double in one fixed order,
 * divided once and rounded once to fp32: two calls return the same bits and a sample does not depend on its batch.  Slots
 * behind a count are not read; a slot whose index is outside [0, L) of the other cloud contributes +0, and so does a pair
 * in which either normal is all zeros (a degenerate or padded row).  No atomics, no workspace, one launch (capturable).
 * Argument rules as rf_nn_metrics: b == 0 is RF_OK; RF_EINVAL for n < 1, m < 1, b > 65535, a NULL tensor (len1 / len2 may be
 * NULL), a tensor or count array not 4-byte aligned; all before any HIP call. */
#define RF_PCA_MAX_K 64
int rf_local_pca(int b, int n, int m, int k, const float *xyz, const int *idx, const int *len1, const int *len2,
                 const float *viewpoint, float *normals, float *eigenvalues, float *axes, rf_stream_t stream);
int rf_nn_normal_consistency(int b, int n, int m, const float *nrm1, const float *nrm2, const int *idx1, const int *idx2,
                             const int *len1, const int *len2, float *out, rf_stream_t stream);

/* ---- grid pooling on a sparse voxel grid, and the point order along a space-filling curve (grid_pool.hip) ----
 * rf_grid_cluster: xyz (b,n,3) -> per sample the occupied cells of an unbounded grid of edge `cell`, by a sort of integer
 * cell keys: which cell every point is in, the points in key order, where every cell's points begin.  One workgroup per
 * sample with its 64-bit words in LDS, hence 1 <= n <= RF_GC_MAX_POINTS (the cap RF_SW_MAX_POINTS has for the same reason),
 * b <= 65535.  One launch, no workspace, no atomics, no memset: every element of every output is written exactly once on
 * every call; the counts stay on the device (capturable).  Two calls return the same bits, a sample does not depend on its
 * batch, a ragged call equals the call on the slices.  Every operation is prescribed:
 *   usable   L = len[i] clamped into [1, n] (len NULL: n), read on the device.  A row below L is USABLE when its three
 *            coordinates are finite.  Rows behind L are not read and may hold anything.
 *   origin   origin (b,3) fp32 on the device, or NULL: then per axis the fp32 minimum over the sample's usable rows (exact,
 *            so free of any order), + 0.0f (-0 becomes +0), and +0 when no row is usable.  The origin used is written to
 *            origin_out (b,3).
 *   cell     per axis t = ((double)x - (double)o) / (double)cell, three separately rounded double operations, k = floor(t).
 *            A usable row is INSIDE when -32768 <= t < 32768 on all three axes, compared in double before any conversion to
 *            an integer (a NaN or infinite origin leaves no row inside).  u = k + 32768 in [0, 65535].
 *   key      48 bits.  RF_GC_XYZ: u_x << 32 | u_y << 16 | u_z.  RF_GC_Z (Morton): bit 3j+2 = bit j of u_x, 3j+1 of u_y, 3j of
 *            u_z.  RF_GC_HILBERT: Skilling's axes-to-transpose on 16 bits with X[0] = u_x, X[1] = u_y, X[2] = u_z -- for Q =
 *            2^15 down to 2 and i = 0, 1, 2: if X[i] & Q then X[0] ^= Q-1 else { t = (X[0] ^ X[i]) & (Q-1); X[0] ^= t;
 *            X[i] ^= t }; then X[1] ^= X[0]; X[2] ^= X[1]; then t = 0 and for Q = 2^15 down to 2: if X[2] & Q then t ^= Q-1;
 *            X[i] ^= t -- and X interleaved as for RF_GC_Z.  Both curves: a bijection with code 0 at cell (0,0,0) of the
 *            16-bit cube, code >> 3s is the code of the cell >> s on 16 - s bits (coarsening a code coarsens the cell), and
 *            consecutive Hilbert codes are face-adjacent cells.  Other axis conventions are a column permutation of xyz in
 *            front of the call.
 *   sort     words key << 16 | i (the point index i < 16384 in the low bits), ascending: the order is ascending (key, index).
 *   outputs  inside (b) int32: the inside count I.  nclusters (b) int32: the number of distinct keys M.
 *            point_order (b,n) int32: the inside points in sorted order, zeros from I on.
 *            starts (b,n+1) int32: entry j < M is where cluster j begins in point_order; every entry from M on holds I, so
 *            starts[j+1] - starts[j] is the size of cluster j and 0 behind M.
 *            cluster (b,n) int32: the rank of the point's cell among the sample's occupied cells in key order; -1 for a row
 *            that is not inside.
 *            coords (b,n,3) int32: k of each cluster, zeros behind M.
 *            code (b,n) int64 or NULL: the key per point, -1 for a row that is not inside.
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n
 * outside 1 ... RF_GC_MAX_POINTS, b above 65535, a cell that is not a finite fp32 > 0, an unknown order, a NULL tensor (len,
 * origin and code may be NULL), a tensor or count array not 4-byte aligned, a code not 8-byte aligned.
 *
 * rf_grid_pool: feat (b,n,c), 1 <= c <= RF_GP_MAX_CHANNELS, and rf_grid_cluster's point_order, starts and nclusters ->
 * out (b,n,c): row j < M reduces the rows of cluster j, point_order[starts[j] .. starts[j+1]), in that order (ascending
 * point index); rows behind M are +0.  RF_GP_SUM: acc = +0.0; acc = acc + (double)x; rounded to fp32 once.  RF_GP_MEAN: the
 * same sum divided by the count in double, rounded once.  RF_GP_MAX: the first member, replaced by a later one when it is
 * strictly greater; a NaN member is taken and ends the walk; arg (b,n,c) int32 receives the winning point index (0 behind M)
 * -- required for RF_GP_MAX, NULL otherwise.  The pooled coordinates are this entry with c = 3 and RF_GP_MEAN.  The arrays are
 * read defensively: nclusters is clamped into [0, n], a list's bounds into [0, n], a member outside [0, n) is skipped, an
 * empty list gives +0 -- nothing outside the tensors is touched whatever they hold.  One launch, no workspace.
 *
 * rf_grid_unpool: src (b,n,c) pooled rows, cluster (b,n) -> dst (b,n,c), row i from row cluster[i] of src; +0 where
 * cluster[i] is outside [0, n) (-1: not inside).  RF_GU_COPY: the row.  RF_GU_MEAN: (float)((double)src / count), count =
 * starts[cluster[i]+1] - starts[cluster[i]] (+0 when that is not positive); starts is required.  RF_GU_MAX: src[..][ch] where
 * arg[cluster[i]][ch] == i, else +0; arg (b,n,c) is required.  starts and arg may be NULL where they are not read.  This one
 * entry is the forward of an unpooling and the backward of all three reductions; the backward of RF_GU_COPY is rf_grid_pool
 * with RF_GP_SUM: no float atomics and no memset anywhere, so the gradients have prescribed bits too.  One launch.
 * Argument rules of both, before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n outside
 * 1 ... RF_GC_MAX_POINTS, c outside 1 ... RF_GP_MAX_CHANNELS, b above 65535, an unknown reduce / mode, a NULL tensor (those
 * named optional aside), arg given without RF_GP_MAX, a tensor not 4-byte aligned.  When c is a multiple of 4 and every
 * (b,n,c) tensor is 16-byte aligned the rows move as 16-byte vectors; the results are the same. */
#define RF_GC_MAX_POINTS 16384
#define RF_GP_MAX_CHANNELS 2048
#define RF_GC_XYZ 0
#define RF_GC_Z 1
#define RF_GC_HILBERT 2
#define RF_GP_SUM 0
#define RF_GP_MEAN 1
#define RF_GP_MAX 2
#define RF_GU_COPY 0
#define RF_GU_MEAN 1
#define RF_GU_MAX 2
int rf_grid_cluster(int b, int n, float cell, int order, const float *xyz, const int *len, const float *origin,
                    float *origin_out, int *inside, int *nclusters, int *point_order, int *starts, int *cluster, int *coords,
                    long long *code, rf_stream_t stream);
int rf_grid_pool(int b, int n, int c, int reduce, const float *feat, const int *point_order, const int *starts,
                 const int *nclusters, float *out, int *arg, rf_stream_t stream);
int rf_grid_unpool(int b, int n, int c, int mode, const float *src, const int *cluster, const int *starts, const int *arg,
                   float *dst, rf_stream_t stream);

/* ---- submanifold sparse convolution on the cells of that grid (sparse_conv.hip) ----
 * The output cells are the input cells; the strided form and its transpose are the next block (sparse_stride.hip).  A kernel of edge
 * ks in {3, 5} has K = ks^3 slots; with r = ks / 2, slot t = ((dx + r) ks + (dy + r)) ks + (dz + r) has the offset
 * dilation (dx, dy, dz), so offset[K-1-t] = -offset[t] and the centre is slot (K-1)/2.
 *
 * rf_sparse_conv_map: coords (b,n,3) int32 -- rf_grid_cluster's, in any order, or those of a coarser level -- and count (b)
 * -> nbr (b,n,K) int32.  M = count[i] clamped into [0, n] (NULL: n), read on the device; rows behind M are never read.  A
 * row below M is LIVE when (a) its three coordinates are in [-32768, 32767] and (b) no row of lower index has the same
 * coordinates; (c) a duplicate of an earlier row is not live: its row of nbr is all -1 and no row names it.  For a live row
 * i, nbr[i][t] is the live row j with coords[j] = coords[i] + offset[t] (the sum range-checked: a target outside
 * [-32768, 32767] is absent), or -1.  Every other row of nbr, the rows from M on included, is -1.  Hence for live i, j:
 * nbr[i][t] == j exactly when nbr[j][K-1-t] == i, on which the gradient below rests.  One workgroup per sample sorts
 * (48-bit key << 16 | row) in LDS, as rf_grid_cluster does, and answers every (row, slot) by a binary search: n <=
 * RF_GC_MAX_POINTS.  One launch, no workspace, no atomics, no memset, every element of nbr written once, capturable.
 * Argument rules, before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n outside
 * 1 ... RF_GC_MAX_POINTS, b above 65535, ks outside {3, 5}, dilation outside 1 ... RF_SC_MAX_DILATION, a NULL tensor (count
 * may be NULL), a tensor or count array not 4-byte aligned.
 *
 * rf_sparse_conv: feat (b,n,cin), weight, nbr (b,n,K), count (b) -> out (b,n,cout), K in {27, 125}, 1 <= cin, cout <=
 * RF_SC_MAX_CHANNELS.  RF_SC_FORWARD, weight (K,cin,cout): per row i < M and output channel o
 *     acc = +0; for t = 0 .. K-1 ascending: j = nbr[i][t]; if 0 <= j < M:
 *         for ch = 0 .. cin-1 ascending: acc = fmaf(feat[j][ch], weight[t][ch][o], acc)
 *     out[i][o] = acc
 * an fp32 fmaf chain (v_mfma_f32_32x32x2_f32 computes exactly that, subnormals kept).  Rows from M on are +0.  An entry of
 * nbr outside [0, M) is absent, so nothing outside the tensors is touched whatever nbr holds; a non-finite feature row
 * reaches exactly the outputs whose map names it.  An absent slot, and the padding of an odd cin to the instruction's two
 * channels, may be realised as skipped steps or as steps with zeros.  The two differ in this only: an accumulator that is
 * exactly -0 may become +0 -- zeros compare equal regardless of sign, NaNs as NaN regardless of payload -- and the weights
 * must be finite: a precondition that is not checked (nothing outside out is touched if it is broken).
 * RF_SC_GRAD_INPUT is the same kernel for the gradient to the features: feat is grad_out (b,n,cin), weight the forward's
 * weight, which is (K,cout,cin) in this call's sizes, out is grad_feat (b,n,cout), and weight[K-1-t][o][ch] stands where
 * weight[t][ch][o] stands above.  By the map's symmetry that mirrored gather chain is the gradient; it is prescribed as
 * such, not as a scatter: no atomics, every row stored once.  One launch, no workspace.
 *
 * rf_sparse_conv_grad_weight: feat (b,n,cin), grad_out (b,n,cout), nbr, count -> grad_weight (K,cin,cout),
 *     grad_weight[t][ci][co] = sum over samples and rows i < M with 0 <= j = nbr[i][t] < M of feat[j][ci] grad_out[i][co]:
 * per sample the rows in chunks of RF_SC_WGRAD_ROWS; inside a chunk acc = +0 and acc = fmaf(feat[j][ci], grad_out[i][co],
 * acc) over the chunk's rows ascending, absent slots skipped (or taken with zeros on both sides, with the same latitude for
 * -0); a sample's chunks added in double from +0.0 ascending, the samples' totals added in double from +0.0 ascending,
 * rounded to fp32 once.  The result is a sum over the batch and depends on nothing else.  Two launches (a double partial per
 * sample into the workspace, then the sum over the samples), no atomics, no memset, the same bits on every call.
 * workspace: rf_sparse_conv_grad_weight_workspace_bytes(b, K, cin, cout) bytes, 16-byte aligned (0 = outside the domain).
 * Argument rules of both, before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n outside
 * 1 ... RF_GC_MAX_POINTS, b above 65535, K outside {27, 125}, cin or cout outside 1 ... RF_SC_MAX_CHANNELS, an unknown mode,
 * a NULL tensor (count may be NULL), a tensor or count array not 4-byte aligned, a workspace that is NULL or not 16-byte
 * aligned; a workspace smaller than the query says is RF_EWORKSPACE.  When cin and cout are multiples of 4 and feat and
 * weight are 16-byte aligned, rf_sparse_conv loads rows as 16-byte vectors; the results are the same. */
#define RF_SC_MAX_CHANNELS 256
#define RF_SC_MAX_DILATION 1024
#define RF_SC_WGRAD_ROWS 1024
#define RF_SC_FORWARD 0
#define RF_SC_GRAD_INPUT 1
int rf_sparse_conv_map(int b, int n, int ks, int dilation, const int *coords, const int *count, int *nbr, rf_stream_t stream);
int rf_sparse_conv(int b, int n, int K, int cin, int cout, int mode, const float *feat, const float *weight, const int *nbr,
                   const int *count, float *out, rf_stream_t stream);
size_t rf_sparse_conv_grad_weight_workspace_bytes(int b, int K, int cin, int cout);
int rf_sparse_conv_grad_weight(int b, int n, int K, int cin, int cout, const float *feat, const float *grad_out, const int *nbr,
                               const int *count, float *grad_weight, void *workspace, size_t workspace_bytes,
                               rf_stream_t stream);

/* ---- strided sparse convolution and its transpose: the change of level on that grid (sparse_stride.hip) ----
 * Kernel 2, stride 2 only: a coarse cell (x >> 1, y >> 1, z >> 1) -- the arithmetic shift, a floor -- has up to eight children,
 * the child (x, y, z) in slot t = (x & 1) 4 + (y & 1) 2 + (z & 1).  Kernel 3 / stride 2 and other strides are not provided.  With
 * rf_sparse_stride_map's maps the transpose writes to the cells of the finer level it came from; with rf_sparse_generate_map's (the
 * next block) the same entries are the "generative" transposed convolution that creates cells.
 *
 * rf_sparse_stride_map: coords (b,n,3) int32 and count (b), read exactly as rf_sparse_conv_map reads them (the same LIVE rule:
 * below the clamped count M, in [-32768, 32767], no row of lower index with the same coordinates; any order) -> the coarse
 * level.  The coarse cells of a sample are the distinct coarse cells of its live rows in ascending row-major key order (the
 * order RF_GC_XYZ gives), D of them: total_out[s] = D, count_out[s] = min(D, n_coarse).  Cells of rank >= n_coarse are DROPPED:
 * they have no row, and their children count as not live for child and up.  coords_out (b,n_coarse,3) holds the cells, zeros
 * behind count_out.  child (b,n_coarse,8): child[j][t] is the live fine row in coarse cell j at slot t, or -1; rows behind
 * count_out are all -1.  up (b,n): 8 j + t for a live, kept fine row, -1 for every other row, the rows from M on included.
 * Hence up[i] == 8 j + t exactly when child[j][t] == i.  coords_out / count_out go as they are into rf_sparse_conv_map for the
 * coarse level's submanifold layers and into another rf_sparse_stride_map for the next level.  One workgroup per sample sorts
 * ((45-bit coarse key << 3 | t) << 16 | row) in LDS; a scan of the words at which the coarse key changes gives the rank.  n <=
 * RF_GC_MAX_POINTS, 1 <= n_coarse <= n, b <= 65535.  One launch, no workspace, no atomics, no memset, every element of every
 * output written exactly once, capturable.  Argument rules, before any HIP call: RF_EINVAL for a negative size; then b == 0 is
 * RF_OK; RF_EINVAL for n outside 1 ... RF_GC_MAX_POINTS, n_coarse outside 1 ... n, b above 65535, a NULL tensor (count may be
 * NULL), a tensor or count array not 4-byte aligned.
 *
 * rf_sparse_conv_strided: weight is always the layer's (8, ci, co) tensor; cin is the reduction width of this call and cout the
 * width of out, both in 1 ... RF_SC_MAX_CHANNELS; M and Mc are count and count_coarse clamped into [0, n] and [0, n_coarse]
 * (NULL: n, n_coarse).  Every sum is ONE fp32 fmaf chain from +0 in the stated order, with rf_sparse_conv's latitude for absent
 * slots and odd widths (-0 may become +0); weights must be finite.
 *   RF_SS_DOWN             src (b,n,cin) -> out (b,n_coarse,cout).  Per j < Mc and o: t ascending, skipping i = child[j][t]
 *                          outside [0, M); then ch ascending: acc = fmaf(src[i][ch], weight[t][ch][o], acc).  Rows from Mc on: +0.
 *   RF_SS_UP               the transposed convolution onto the fine cells: src (b,n_coarse,cin) -> out (b,n,cout).  A fine row i
 *                          is SERVED when i < M, up[i] = 8 j + t with 0 <= j < Mc, and child[j][t] == i; then out[i][o] is the
 *                          chain over ch ascending of src[j][ch] weight[t][ch][o].  A row that is not served is +0.
 *   RF_SS_DOWN_GRAD_INPUT  src is the coarse grad_out (b,n_coarse,cin) -> out (b,n,cout): as RF_SS_UP with weight[t][o][ch].
 *   RF_SS_UP_GRAD_INPUT    src is the fine grad_out (b,n,cin) -> out (b,n_coarse,cout): as RF_SS_DOWN with weight[t][o][ch].
 * The served rule makes the result well defined and keeps every store inside out with no two writers of a row, whatever child
 * and up hold: garbage in the maps is tolerated as rf_sparse_conv tolerates it in nbr.  DOWN and UP_GRAD_INPUT gather (a wave
 * owns 32 coarse rows and carries its accumulators over the eight slots); UP and DOWN_GRAD_INPUT fan out (a workgroup owns 32
 * coarse rows, each of its waves two slots: one chain per slot some row of the tile has, each accumulator row stored to the fine
 * row child[j][t] that up confirms; further workgroups of the same launch store +0 to the fine rows that are not served).  One launch, no workspace, no
 * atomics, no memset, every element of out written once.
 *
 * rf_sparse_conv_strided_grad_weight -> grad_weight (8,cin,cout), the layer's layout.  Both modes walk the coarse rows j < Mc
 * ascending with i = child[j][t] in [0, M), otherwise skipped.  RF_SS_DOWN: fine is the forward's feat (b,n,cin), coarse is
 * grad_out (b,n_coarse,cout), the terms are fine[i][ci] coarse[j][co].  RF_SS_UP: coarse is the forward's feat (b,n_coarse,cin),
 * fine is grad_out (b,n,cout), the terms are coarse[j][ci] fine[i][co].  The sum is rf_sparse_conv_grad_weight's: an fmaf chain
 * per chunk of RF_SC_WGRAD_ROWS coarse rows, the chunks added in double, a double partial per sample in the workspace, the
 * samples added in double in ascending order, rounded once.  Two launches, no atomics, no memset.
 * workspace: rf_sparse_conv_strided_grad_weight_workspace_bytes(b, cin, cout) bytes, 16-byte aligned (0 = outside the domain).
 * Argument rules of both, before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n outside
 * 1 ... RF_GC_MAX_POINTS, n_coarse outside 1 ... n, b above 65535, cin or cout outside 1 ... RF_SC_MAX_CHANNELS, an unknown mode
 * (the weight gradient takes RF_SS_DOWN and RF_SS_UP), a NULL tensor (count and count_coarse may be NULL), a tensor or count
 * array not 4-byte aligned, a workspace that is NULL or not 16-byte aligned; a workspace smaller than the query says is
 * RF_EWORKSPACE.  When cin and cout are multiples of 4 and src and weight are 16-byte aligned, rf_sparse_conv_strided loads rows
 * as 16-byte vectors; the results are the same. */
#define RF_SS_DOWN 0
#define RF_SS_UP 1
#define RF_SS_DOWN_GRAD_INPUT 2
#define RF_SS_UP_GRAD_INPUT 3
int rf_sparse_stride_map(int b, int n, int n_coarse, const int *coords, const int *count, int *coords_out, int *count_out,
                         int *total_out, int *child, int *up, rf_stream_t stream);
int rf_sparse_conv_strided(int b, int n, int n_coarse, int cin, int cout, int mode, const float *src, const float *weight,
                           const int *child, const int *up, const int *count, const int *count_coarse, float *out,
                           rf_stream_t stream);
size_t rf_sparse_conv_strided_grad_weight_workspace_bytes(int b, int cin, int cout);
int rf_sparse_conv_strided_grad_weight(int b, int n, int n_coarse, int cin, int cout, int mode, const float *fine,
                                       const float *coarse, const int *child, const int *count, const int *count_coarse,
                                       float *grad_weight, void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* ---- generative transposed convolution, pruning and cell lookup: the decoder's step on that grid (sparse_generate.hip) ----
 * A sparse completion decoder creates all eight children of every coarse cell, convolves onto them, classifies every new cell
 * and prunes the unoccupied ones (MinkowskiEngine's GenerativeConvolutionTranspose + MinkowskiPruning).  The convolution is the
 * block above: with child / up of rf_sparse_generate_map, count = its count_out and count_coarse = the coarse count, RF_SS_UP is
 * the generative transposed convolution, RF_SS_UP_GRAD_INPUT its gradient to the features and
 * rf_sparse_conv_strided_grad_weight(RF_SS_UP) its gradient to the weight.  The four entries here are one launch each, no
 * workspace, no atomics in memory, no memset, every element of every output stored exactly once on every call, every count read
 * on the device (capturable); b <= 65535 and every row count <= RF_GC_MAX_POINTS.  Counts are clamped into [0, rows] (NULL: all
 * rows); rows behind a count are never read.  LIVE is rf_sparse_conv_map's rule: below the clamped count, the three coordinates
 * in [-32768, 32767], no row of lower index with the same coordinates.
 *
 * rf_sparse_generate_map: coords (b,n_coarse,3), count (b) -> coords_out (b,n_fine,3), count_out (b), total_out (b), child
 * (b,n_coarse,8), up (b,n_fine), 8 <= n_fine <= RF_GC_MAX_POINTS, 1 <= n_coarse <= n_fine.  A coarse row is a PARENT when it is
 * live and its three coordinates are in [-16384, 16383] (its children 2 c + bit then stay in range).  The rank r of a parent is
 * the number of parents of lower ROW index (not key order: with no dead rows the fine row of parent j, slot t is 8 j + t and the
 * input order is kept).  Parents with r < n_fine / 8 (integer division) are KEPT: a parent gets all eight children or none.
 * For a kept parent j and slot t = 0 .. 7 (the slot rule of the block above, t = (x & 1) 4 + (y & 1) 2 + (z & 1) of the child):
 *     child[j][t] = 8 r + t,  up[8 r + t] = 8 j + t,  coords_out[8 r + t] = 2 coords[j] + ((t >> 2) & 1, (t >> 1) & 1, t & 1).
 * Every other row of child is all -1; behind count_out up is -1 and coords_out is 0.  total_out = 8 #parents, count_out =
 * 8 #kept.  Hence up[i] == 8 j + t exactly when child[j][t] == i, on which rf_sparse_conv_strided rests.  One workgroup per
 * sample sorts (48-bit key << 16 | row) in LDS to find the duplicates, marks the live rows in LDS and scans them in row order.
 * Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is RF_OK; RF_EINVAL for n_fine
 * outside 8 ... RF_GC_MAX_POINTS, n_coarse outside 1 ... n_fine, b above 65535, a NULL tensor (count may be NULL), a tensor or
 * count array not 4-byte aligned.
 *
 * rf_sparse_prune_map: coords (b,n,3), keep (b,n) uint8, count (b) -> coords_out (b,n_out,3), count_out (b), total_out (b), src
 * (b,n_out), dst (b,n), 1 <= n_out <= n <= RF_GC_MAX_POINTS.  Row i < M is SELECTED when keep[i] != 0; there is no liveness test,
 * rows are carried as they are; keep behind M is not read.  The rank r of a selected row is the number of selected rows of lower
 * index (the compaction is stable); it is KEPT when r < n_out: src[r] = i, dst[i] = r, coords_out[r] = coords[i].  Every other
 * entry of src and dst is -1, coords_out is 0 behind the count.  total_out = #selected, count_out = min(total_out, n_out).  One
 * workgroup per sample scans keep in row order.  Argument rules, all checked before any HIP call: RF_EINVAL for a negative size;
 * then b == 0 is RF_OK; RF_EINVAL for n outside 1 ... RF_GC_MAX_POINTS, n_out outside 1 ... n, b above 65535, a NULL tensor (count
 * may be NULL; keep may not), an int32 tensor or count array not 4-byte aligned.  keep has no alignment requirement.
 *
 * rf_sparse_lookup: coords (b,n,3), count (b), table (b,m,3), tcount (b), 0 <= shift <= 15 -> idx (b,n), 1 <= n, m <=
 * RF_GC_MAX_POINTS.  A table row is USABLE when it is below its clamped count and its coordinates are in [-32768, 32767]; its
 * cell is table >> shift, the arithmetic shift (a floor) per axis.  For a query row i below its clamped count with coordinates
 * in [-32768, 32767], idx[i] is the LOWEST usable table row whose shifted cell equals coords[i], or -1 when there is none; for
 * every other query row idx[i] is -1.  Query rows are not de-duplicated.  shift = 0 is the map between two cell sets of one
 * level (a skip connection); shift = s tells whether a cell of level s is occupied among the FINEST cells, with no pyramid of
 * the target.  One workgroup per sample sorts the table's (key << 16 | row) in LDS and answers every query by a lower-bound
 * binary search, as rf_sparse_conv_map does.  Argument rules, all checked before any HIP call: RF_EINVAL for a negative n, m or
 * b; then b == 0 is RF_OK; RF_EINVAL for n or m outside 1 ... RF_GC_MAX_POINTS, b above 65535, shift outside 0 ... 15, a NULL
 * tensor (count and tcount may be NULL), a tensor or count array not 4-byte aligned.
 *
 * rf_sparse_take_rows: src (b,n_src,c), idx (b,n_dst), count_dst (b) -> dst (b,n_dst,c), 1 <= c <= RF_GP_MAX_CHANNELS, 1 <=
 * n_src, n_dst <= RF_GC_MAX_POINTS.  dst[r] = src[idx[r]] bit for bit where r is below the clamped count and 0 <= idx[r] < n_src;
 * every other row is +0, so nothing outside the tensors is touched whatever idx holds; idx behind the count is not read.  It is
 * rf_grid_unpool's RF_GU_COPY with two row counts: features through a pruning (by src forward, by dst backward) and through a
 * skip (by the lookup's idx).  Argument rules, all checked before any HIP call: RF_EINVAL for a negative size; then b == 0 is
 * RF_OK; RF_EINVAL for n_src or n_dst outside 1 ... RF_GC_MAX_POINTS, c outside 1 ... RF_GP_MAX_CHANNELS, b above 65535, a NULL
 * tensor (count_dst may be NULL), a tensor or count array not 4-byte aligned.  When c is a multiple of 4 and src and dst are
 * 16-byte aligned the rows move as 16-byte vectors; the results are the same. */
int rf_sparse_generate_map(int b, int n_coarse, int n_fine, const int *coords, const int *count, int *coords_out, int *count_out,
                           int *total_out, int *child, int *up, rf_stream_t stream);
int rf_sparse_prune_map(int b, int n, int n_out, const int *coords, const unsigned char *keep, const int *count, int *coords_out,
                        int *count_out, int *total_out, int *src, int *dst, rf_stream_t stream);
int rf_sparse_lookup(int b, int n, int m, int shift, const int *coords, const int *count, const int *table, const int *tcount,
                     int *idx, rf_stream_t stream);
int rf_sparse_take_rows(int b, int n_src, int n_dst, int c, const float *src, const int *idx, const int *count_dst, float *dst,
                        rf_stream_t stream);

/* -------------------------------------------------- interpolation (tf_ops/interpolation) - */
/* Replace threenn_cpu / threeinterpolate_cpu / threeinterpolate_grad_cpu
 * (tf_interpolate.cpp:60-153; CPU-only ops in the reference).  xyz1 (b,n,3) unknown,
 * xyz2 (b,m,3) known; dist/idx (b,n,3).  points (b,m,c), weight (b,n,3), out (b,n,c);
 * grad_points (b,m,c) zero-filled here. */
int rf_threenn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx,
               rf_stream_t stream);
/* The same op over spatially sorted copies of the two sets (the Chamfer sweep's sort, rf_nn_sort): a wave of 64
 * neighbouring unknown points visits only the candidate blocks whose box can still hold one of its three nearest.
 * dist / idx bit-identical to rf_threenn (ties included: the three smallest by (distance, index), which is what
 * the scan's strict '<' insertion in index order yields, tf_interpolate.cpp:78-93).  1 <= n, m <= 65536,
 * b <= 65535 (else RF_EINVAL: use rf_threenn).  sorted1 / sorted2: rf_nn_sort handles of xyz1 / xyz2 or NULL
 * (sorted here, into the workspace).  workspace: rf_threenn_boxes_workspace_bytes(b, n, m) bytes, 16-byte
 * aligned (0 = outside the domain).  Pays from about 1e8 pairs per call on (the sort is ~25 us). */
size_t rf_threenn_boxes_workspace_bytes(int b, int n, int m);
int rf_threenn_boxes(int b, int n, int m, const float *xyz1, const float *xyz2, const void *sorted1,
                     const void *sorted2, float *dist, int *idx, void *workspace, size_t workspace_bytes,
                     rf_stream_t stream);
/* three_nn over a ragged batch (the conventions of the "ragged batches" block of the sampling section; RF_GROUP_* forms as
 * rf_queryballpoint_lengths): len1 = unknown points per sample, len2 = known points.  Rows [0, len1[i]) are rf_threenn's on
 * the slices -- with len2[i] < 3 what rf_threenn gives for m < 3, (+inf, 0) in the slots without a neighbour -- and the rows
 * behind len1[i] are zeros.  RF_GROUP_AUTO takes the boxed form where the Python wrapper takes it for the plain op, by the
 * padded sizes; RF_GROUP_BOXES outside rf_threenn_boxes' domain is RF_EINVAL.  rf_threeinterpolate and its gradient take the
 * result as it is: the zero-filled indices of padded rows are in range (they interpolate known point 0 with weight rows the
 * caller left there; the counts say which rows mean something). */
size_t rf_threenn_lengths_workspace_bytes(int b, int n, int m, int form);
int rf_threenn_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *dist,
                       int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream, int form);
int rf_threeinterpolate(int b, int m, int c, int n, const float *points, const int *idx,
                        const float *weight, float *out, rf_stream_t stream);
int rf_threeinterpolate_grad(int b, int n, int c, int m, const float *grad_out, const int *idx,
                             const float *weight, float *grad_points, rf_stream_t stream);
/* ... with caller scratch: where a sample's known points do not fit the LDS tile of the in-kernel form (more than 2048 at 8
 * channels per slice) the 3 n slots are counting-sorted by known point and every row of grad_points is written once
 * (scatter_rows.hip, as rf_grouppoint_grad_ws).  rf_threeinterpolate_grad_workspace_bytes = 0: no scratch needed, pass NULL. */
size_t rf_threeinterpolate_grad_workspace_bytes(int b, int n, int c, int m);
int rf_threeinterpolate_grad_ws(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                const float *weight, float *grad_points, void *workspace, size_t workspace_bytes,
                                rf_stream_t stream);

/* ------------------------------------------- rest of the import surface ("next" row f3) --- */
/* Replaces AuctionMatchLauncher(b,n,xyz1,xyz2,matchl,matchr,cost) (tf_ops/emd/tf_auctionmatch.cpp:25,
 * tf_auctionmatch_g.cu:292-294).  xyz1, xyz2 (b,n,3); matchl, matchr (b,n) int32: matchr[j] = the
 * xyz1 point assigned to xyz2 point j, matchl its inverse.  `workspace` is the reference's temp
 * cost matrix (b,n,n) floats.  Defined for n < 1024 or n in {1024, 2048, 4096}
 * (rf_auctionmatch_supported); the reference additionally caps n at 4096. */
int rf_auctionmatch_supported(int n);
size_t rf_auctionmatch_workspace_bytes(int b, int n);
int rf_auctionmatch(int b, int n, const float *xyz1, const float *xyz2, int *matchl, int *matchr,
                    void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* Replaces selectionSortLauncher(b,n,m,k,dist,outi,out) (tf_ops/grouping/tf_grouping.cpp:112,
 * tf_grouping_g.cu:129-132).  dist (b,m,n); outi (b,m,n) int32, out (b,m,n): per row a partial
 * selection sort, the first k entries are the k smallest in ascending order.  n <= 16384. */
int rf_selectionsort(int b, int n, int m, int k, const float *dist, int *outi, float *out,
                     rf_stream_t stream);

/* Replaces probsampleLauncher(b,n,m,inp_p,inp_r,temp,out) (tf_ops/sampling/tf_sampling.cpp:65,
 * tf_sampling_g.cu:198-201): inp_p (b,n) weights, inp_r (b,m) uniforms in [0,1), temp (b,n) floats
 * (receives the cumulative sums), out (b,m) int32 inverse-CDF indices. */
int rf_probsample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out,
                  rf_stream_t stream);

/* ------------------------------------------------------- loss glue as a fused op (row f1) --- */
/* The reference's `earth_mover` (vv_recon.py:392-399) is approx_match -> match_cost, with
 * MatchCostGrad behind it (pc_distance/tf_approxmatch.py:44-50; ApproxMatch itself is NoGradient,
 * so match is a constant in the backward).  rf_earth_mover computes the same cost (b) -- and,
 * when grad1/grad2 are non-NULL (both or neither), the same MatchCostGrad outputs grad1 (b,n,3),
 * grad2 (b,m,3) -- straight from the per-level ratio vectors, without materialising the
 * (b,m,n) match tensor (512 MiB at 32x2048x2048; 1 GiB per sample at 16384^2).  No reference
 * launcher corresponds to it: a TF-side maintainer would register it as one new op replacing
 * the three-op chain.  Reference 10-level schedule only.  The cost is the chain's within rel 1e-5 (north_star's bar), not its
 * bits: the cost-only form (grad1 == grad2 == NULL) sums a sample's columns in the order of their last live level and takes
 * sqrt(d2) from v_sqrt_f32 (1 ulp) -- a function of the sample alone, so RF_EMD_SWEPT's batch independence holds. */
size_t rf_earth_mover_workspace_bytes(int b, int n, int m);
int rf_earth_mover(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost,
                   float *grad1, float *grad2, void *workspace, size_t workspace_bytes,
                   rf_stream_t stream);
/* ... with the route pinned as rf_approxmatch_mode pins it (RF_EMD_SWEPT: cost[i] bit-identical whatever the batch). */
size_t rf_earth_mover_mode_workspace_bytes(int b, int n, int m, int mode);
int rf_earth_mover_mode(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost,
                        float *grad1, float *grad2, void *workspace, size_t workspace_bytes,
                        rf_stream_t stream, int mode);

/* ---- ragged batches: per-sample point counts (EMD) ------------------------------------------
 * The conventions of rf_nn_distance_lengths: sample i is xyz1[i, :len1[i]] against xyz2[i, :len2[i]]; len1 / len2 are DEVICE
 * int32 arrays of b counts or NULL ("all n" / "all m"), read by the kernels themselves (no host synchronisation: a call can be
 * captured in a HIP graph) and clamped into [1, n] / [1, m].  Nothing beyond a count reaches a result: neither the padded
 * coordinates of either cloud nor, in rf_matchcost{,_grad}_lengths, the padded entries of the caller's `match` (NaN, inf,
 * 1e30 there change no bit of match or cost).
 *   Multipliers per sample from the clamped counts, the reference's integer rule (am_multipliers): len1 >= len2 gives
 *   multiL = 1, multiR = len1 / len2, else multiL = len2 / len1, multiR = 1.
 *   match keeps the shape (b, m, n); every entry with l >= len2[i] or k >= len1[i] is exactly +0.  The cost sums the valid
 *   pairs only; gradient rows beyond a count are exactly +0.
 *   Route: always the pinned one (RF_EMD_SWEPT: dense sweeps in the caller's order, launch shapes of a batch of one), or
 *   am_small's one workgroup per sample when n, m <= 256 -- so sample i's match, cost and fused cost are bit-identical to the
 *   same ragged call on [i:i+1]; counts (n, m) or NULL give bit for bit rf_approxmatch_mode(..., RF_EMD_SWEPT) (any schedule)
 *   and rf_matchcost; and at n, m <= 256 the valid block of match is bit for bit rf_approxmatch on the unpadded slices.
 *   The work shrinks with the counts: row blocks beyond len1 (len2) exit at once, a sweep's column segment ends at the other
 *   count, and the match / cost / gradient kernels skip whole blocks beyond the counts (still writing match's zeros).  The
 *   column segments stay those of the padded width, so a sum can differ from a call on the slices in the last place.
 * Argument rules: b == 0 is RF_OK; n < 1, m < 1, b > 65535, a NULL tensor, a misaligned count array (4 bytes) or workspace
 * (16 bytes) are RF_EINVAL, as are (rf_approxmatch_lengths) a level multiplier that is positive or not finite; a workspace
 * smaller than the matching _workspace_bytes is RF_EWORKSPACE -- all before any HIP call.  Outputs fully overwritten. */
size_t rf_approxmatch_lengths_workspace_bytes(int b, int n, int m, int nlevels /* 0 = reference's 10 */);
int rf_approxmatch_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                           float *match, const float *levels_host, int nlevels, void *workspace, size_t workspace_bytes,
                           rf_stream_t stream);
size_t rf_matchcost_lengths_workspace_bytes(int b, int n, int m);
int rf_matchcost_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                         const float *match, float *cost, void *workspace, size_t workspace_bytes, rf_stream_t stream);
/* grad1 (b,n,3), grad2 (b,m,3): MatchCostGrad over the valid pairs (both required). */
int rf_matchcost_grad_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                              const float *match, float *grad1, float *grad2, rf_stream_t stream);
/* rf_earth_mover_mode(..., RF_EMD_SWEPT) on ragged batches (grad1 / grad2 both given or both NULL): within rel 1e-5 (cost) and
 * rel 1e-4 + abs 1e-5 (gradients) of it at full counts. */
size_t rf_earth_mover_lengths_workspace_bytes(int b, int n, int m);
int rf_earth_mover_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                           float *cost, float *grad1, float *grad2, void *workspace, size_t workspace_bytes,
                           rf_stream_t stream);

/* `chamfer_big` / `fidelity_loss` (vv_recon.py:381-390) are reduce_mean(sqrt(dist)) over the
 * nn_distance outputs.  rf_chamfer_loss returns the per-sample means loss (b, 2):
 * loss[i][0] = mean_j sqrt(dist1[i][j]), loss[i][1] = mean_k sqrt(dist2[i][k]) (0 for a direction
 * that is not computed) -- the batch means of the reference are the means of these columns -- next
 * to the nn_distance outputs of the computed directions (a direction whose dist/idx pointers are
 * NULL is skipped: fidelity_loss needs direction 1 only).  sorted1 / sorted2: optional rf_nn_sort
 * handles of xyz1 / xyz2 (NULL: sorted internally when the culled sweep is used).
 * rf_chamfer_loss_grad is its backward: NnDistanceGrad with
 * grad_dist_d[i][j] = grad_loss[i][d] / npts_d * 0.5 / sqrt(dist_d[i][j]) formed inside the scatter
 * kernel (no intermediate tensors); grad_xyz1 (b,n,3) / grad_xyz2 (b,m,3) fully overwritten. */
size_t rf_chamfer_loss_workspace_bytes(int b, int n, int m, int want1, int want2, int have_sorted1,
                                       int have_sorted2);
int rf_chamfer_loss(int b, int n, int m, const float *xyz1, const float *xyz2, const void *sorted1,
                    const void *sorted2, float *loss, float *dist1, int *idx1, float *dist2, int *idx2,
                    void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_chamfer_loss_grad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *dist1,
                         const int *idx1, const float *dist2, const int *idx2, const float *grad_loss,
                         float *grad_xyz1, float *grad_xyz2, rf_stream_t stream);

/* `merge_layer` (vv_recon.py:132-139): idx2 of nn_distance(rawpts, newpts), the winner gathered
 * (group_point with nsample = 1), and every new point pulled towards it:
 *   refined = newpts + exp(-|g - newpts|^2 / (1e-8 + decfactor^2)) * (g - newpts).
 * rawpts (b,n,3), newpts (b,m,3), decfactor_dev: DEVICE pointer to the one-element variable
 * (vv_recon.py:211), sorted_raw: optional rf_nn_sort handle of rawpts; refined (b,m,3), idx2 (b,m)
 * (kept for the backward).  rf_merge_layer_grad: grad_newpts (b,m,3), grad_dec (b) per-sample
 * partial derivatives wrt decfactor (their sum is the variable's gradient), grad_raw (b,n,3) or
 * NULL (rawpts is the network input in the model). */
size_t rf_merge_layer_workspace_bytes(int b, int n, int m, int have_sorted_raw);
int rf_merge_layer(int b, int n, int m, const float *rawpts, const float *newpts, const void *sorted_raw,
                   const float *decfactor_dev, float *refined, int *idx2, void *workspace,
                   size_t workspace_bytes, rf_stream_t stream);
int rf_merge_layer_grad(int b, int n, int m, const float *rawpts, const float *newpts,
                        const float *decfactor_dev, const int *idx2, const float *grad_refined,
                        float *grad_newpts, float *grad_dec, float *grad_raw, rf_stream_t stream);

/* merge_layer over a ragged batch: sample i merges newpts[i, :len_new[i]] into rawpts[i, :len_raw[i]].
 * The conventions of rf_nn_distance_lengths: len_raw / len_new are DEVICE int32[b] arrays, NULL = all rows, read by the
 * kernels (no host synchronisation: the calls can be captured into a graph), a value outside [1, n] / [1, m] is clamped
 * inside the kernels, and rows beyond a count may hold anything (NaN, inf, copies of valid points): they reach no result.
 * rf_merge_layer_lengths: direction 2 of rf_nn_distance_lengths (sweep chosen as RF_NN_AUTO on the padded sizes; no
 * sorted handle -- the culled sweep sorts internally) and the pull.  On the valid new rows idx2 and refined are bit for
 * bit rf_merge_layer's on that sample's slices alone, and idx2 < len_raw[i]; a padded new row gets idx2 = 0 and
 * refined = +0.0f.  rf_merge_layer_grad_lengths: grad_newpts as rf_merge_layer_grad on the valid rows and exactly 0 on
 * the padded ones, whatever grad_refined or idx2 hold there; grad_dec[i] sums over the valid new rows only, in
 * rf_merge_layer_grad's order on the slice; grad_raw (or NULL) is exactly 0 beyond len_raw[i].  Count arrays 4-byte
 * aligned, workspace 16-byte aligned (RF_EINVAL); a workspace smaller than rf_merge_layer_lengths_workspace_bytes(b, n, m)
 * is RF_EWORKSPACE; both are found before any HIP call. */
size_t rf_merge_layer_lengths_workspace_bytes(int b, int n, int m);
int rf_merge_layer_lengths(int b, int n, int m, const float *rawpts, const float *newpts, const int *len_raw,
                           const int *len_new, const float *decfactor_dev, float *refined, int *idx2,
                           void *workspace, size_t workspace_bytes, rf_stream_t stream);
int rf_merge_layer_grad_lengths(int b, int n, int m, const float *rawpts, const float *newpts, const int *len_raw,
                                const int *len_new, const float *decfactor_dev, const int *idx2,
                                const float *grad_refined, float *grad_newpts, float *grad_dec, float *grad_raw,
                                rf_stream_t stream);

/* ------------------------------------------------ model graph helper (row f2) ------------ */
/* The elementwise tail of RFNet's per-point dense layers in one pass.  The reference's conv2d
 * (vv_recon.py:47-65: conv + bias_add + activation) is mostly applied to
 * tf.concat([per-point features, tf.tile(global code word)]) (:101,127,144,148,280,288,299,317,343);
 * computed without the concatenation that is
 *     out[i,j,:] = act( y[i,j,:] + sum_{k<kp} p[i,j,k] w[k,:] + r[i,:] )
 * y (b,n,c): the GEMM of the wide per-point inputs, or NULL; p (b,n,kp), w (kp,c): a narrow
 * per-point input (the coordinates: kp = 3; kp <= 16) applied on the fly, or kp = 0; r: bias + code
 * word term, (b,c) with r_per_sample != 0, (c) otherwise; act: 0 none, 1 relu, 2 tanh.
 * c % 4 == 0, c <= 1024 (rf_point_affine_supported).  out may alias y.
 * Non-finite values pass through as the tensor ops pass them: with no activation and with relu a NaN in y, p or r
 * gives NaN (relu is `v < 0 ? 0 : v`, torch.relu's and tf.nn.relu's rule, not fmaxf, which would turn NaN into 0), +inf
 * stays +inf, relu(-inf) = 0; tanh(+-inf) = +-1 and tanh(NaN) = NaN.  relu(-0.0) may be either zero. */
/* tf.reduce_max(axis=1) of a (b, n, c) feature tensor -> (b, c) (global_mlp / encode_cell /
 * recover_cell / init_move_layer / refine_layer, vv_recon.py:90,107,129,151,286).  c % 4 == 0,
 * c <= 1024.  Two launches (strips, fold); exact and deterministic (max in any order).  NaNs are
 * skipped (fmaxf): a channel's maximum runs over its numbers, and a channel that holds nothing above -inf gives -inf.
 * (rf_point_affine's relu lets a NaN through, so a NaN can reach this pooling; it is skipped here all the same.) */
size_t rf_maxpool_points_workspace_bytes(int b, int n, int c);
int rf_maxpool_points(int b, int n, int c, const float *x, float *out, void *workspace,
                      size_t workspace_bytes, rf_stream_t stream);

/* The same with the point index of each maximum (idx (b, c) int32, the lowest index among ties): the
 * forward of the pooling when a backward follows (training: tf.gradients of reduce_max routes the
 * gradient to the arg-max rows). */
size_t rf_maxpool_points_idx_workspace_bytes(int b, int n, int c);
int rf_maxpool_points_idx(int b, int n, int c, const float *x, float *out, int *idx, void *workspace,
                          size_t workspace_bytes, rf_stream_t stream);

/* The two poolings over a ragged batch: for sample i the maximum runs over rows [0, len[i]) of x only.
 * len: DEVICE int32[b], NULL = all rows, read by the kernels (no host synchronisation), clamped into [1, n] inside them;
 * rows beyond a count may hold anything (NaN, +inf) and are never read.  out -- and idx, which is always < len[i] -- are
 * bit for bit what rf_maxpool_points / rf_maxpool_points_idx return for x[i, :len[i]] alone (lowest index among ties,
 * NaNs skipped as fmaxf skips them).  Work shrinks with the counts: a strip wholly behind a count is not read, and the
 * fold visits only the strips that were written, so the workspace (the dense entries' sizes) may arrive uninitialised.
 * Argument rules of the dense entries (c % 4 == 0, c <= 1024, x and workspace 16-byte aligned) plus len 4-byte aligned:
 * RF_EINVAL; a short workspace: RF_EWORKSPACE; all found before any HIP call. */
size_t rf_maxpool_points_lengths_workspace_bytes(int b, int n, int c);
int rf_maxpool_points_lengths(int b, int n, int c, const float *x, const int *len, float *out, void *workspace,
                              size_t workspace_bytes, rf_stream_t stream);
size_t rf_maxpool_points_idx_lengths_workspace_bytes(int b, int n, int c);
int rf_maxpool_points_idx_lengths(int b, int n, int c, const float *x, const int *len, float *out, int *idx,
                                  void *workspace, size_t workspace_bytes, rf_stream_t stream);

/* Backward of a layer tail (training step of the graph; conv2d's bias_add + activation,
 * vv_recon.py:47-65, differentiated):  g[i,j,:] = grad[i,j,:] * act'(out[i,j,:])  and
 * sums[i,:] = sum_j g[i,j,:]  (the bias gradient is the sum of `sums` over i; the gradient of a
 * per-sample row r of rf_point_affine is `sums` itself) in ONE pass over grad/out.  act: 0 none, 1 relu
 * (out > 0), 2 tanh (1 - out^2), 3 leaky relu with slope 0.2 (sign of out); `out` is the layer's
 * OUTPUT (NULL with act 0).  g may alias grad; g NULL (or act 0 with g == grad) writes nothing.
 * c % 4 == 0, c <= 1024.  Deterministic (fixed summation order). */
size_t rf_act_grad_colsum_workspace_bytes(int b, int n, int c);
int rf_act_grad_colsum(int b, int n, int c, const float *grad, const float *out, int act, float *g,
                       float *sums, void *workspace, size_t workspace_bytes, rf_stream_t stream);

int rf_point_affine_supported(int c, int kp);
int rf_point_affine(int b, int n, int c, const float *y, const float *p, int kp, const float *w,
                    const float *r, int r_per_sample, int act, float *out, rf_stream_t stream);

/* ------------------------------------------------------------------ runtime diagnostic --- */
/* hipMemsetAsync(p, 0, bytes) on `stream` -- the ONE place this library issues a memset, and only for
 * this purpose: on ROCm 7 with the graph "packet capture" on (the default; DEBUG_CLR_GRAPH_PACKET_CAPTURE=0
 * before the runtime starts turns it off) a memset node of a small buffer captured into a HIP graph writes
 * garbage on later launches of the graph -- harmless for this library, whose zero fills are kernels, fatal
 * for anything else in the same graph that does (PyTorch's reduction kernels clear their semaphores that
 * way).  A host that captures graphs captures this call in a small test graph first and checks the buffer
 * after every replay (rfnet_amd/_host.py:graph_replay_ok). */
int rf_probe_memset_async(void *p, size_t bytes, rf_stream_t stream);

/* y[i] = v_exp_f32(x[i]) for i < count, the instruction every EMD weight exp(level * d2) goes through
 * (pc_distance/tf_approxmatch.cu:49,77,110,146 use __expf = ex2.approx(x * log2e)).  The skipping sweeps of the sharp
 * levels leave out pairs whose argument is <= -160 on the ground that the instruction returns EXACTLY +0 there; this entry
 * point lets a host (and tests/test_gpu_emd.py) check that on the device it runs on. */
int rf_probe_exp2(const float *x, float *y, int count, rf_stream_t stream);

/* ------------------------------------------------------------------ measurement hooks --- */
/* When enabled, every kernel launch made by this library is bracketed by hipEvents recorded
 * on the launch stream.  rf_profile_collect() waits for them and returns the per-kernel sums
 * since the last collect.  Used by bench.py for roofline.achieved; off by default.
 * This is the library's only process-global state: one switch and one list of pending event
 * pairs for the whole process, shared by all threads and streams (both calls are thread-safe;
 * a collect() concurrent with launches simply leaves those launches for the next collect). */
void rf_profile_enable(int on);
/* Fills up to `cap` entries; returns the number of distinct kernel names seen.  names[i] is a
 * pointer to a static string; ms[i] the summed duration in milliseconds; launches[i] the count. */
int rf_profile_collect(const char **names, double *ms, long *launches, int cap);

#ifdef __cplusplus
}
#endif
#endif /* RFOPS_H_ */
