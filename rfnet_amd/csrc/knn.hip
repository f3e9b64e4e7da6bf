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
// knn_scan_kernel (rf_knn): one lane per query, the candidates wave-uniform through SGPRs in index order (box_bound.hpp
// ts_stream, shared with three_nn_kernel).  In index order a tie never displaces the earlier index, so the float pre-test is
// strict ('d < thr').
//
// knn_boxes_kernel (rf_knn_boxes): the boxed walk of box_bound.hpp (tb_walk, shared with three_nn_boxes_kernel) with knn's list,
// KnList: a wave of 64 neighbouring sorted queries visits the candidate blocks whose box bound is <= some lane's k-th distance,
// nearest superblock first.  Visits go in any order, so the pre-test admits ties ('d <= thr') and the keys settle them: the
// result is the scan's, bit for bit.  Non-finite values break the bounds (the sort leaves such points out of the boxes, and a
// NaN distance ranks FIRST): a wave with a non-finite query, or a sample whose candidate set holds a non-finite coordinate (the
// sort's flag), visits every superblock without a test -- still the same keys, so still the scan's result.
//
// The gradient (rf_knn_grad): term(j, t) = 2 g[j, t] (x1[i] - x2[j]), i = idx[j, t]; grad_xyz2[j] = sum_t term, one lane per
// query; grad_xyz1[i] = -sum of the terms that name i, a scatter done as group_point's (scatter_rows.hip): the m k slots
// counting-sorted by i, then one lane per candidate sums its slots and writes its row once (zeros for a row nobody names).
// Sums in double on both sides.
#include "common.hpp"
#include "scatter_rows.hpp"
#include "nn_pruned.hpp"
#include "box_bound.hpp"
#include "group_internal.hpp"
#include "knn_list.hpp"  // u64, KN_MAXK, kn_insert, kn_zero, KN_DISPATCH: shared with knn_feature.hip

namespace {

constexpr int KN_TPB = 256;

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
// belongs in the list is missed, and the exact keys decide.  The flush loop is unrolled for lists of up to 8 slots only
// (kn_flush_unroll, in the kernel): unrolled at every candidate, a 16-slot list's flush makes the kernel ten times longer.
constexpr int KN_BUF = 16;  // entries per lane
#define KN_FLUSH(BD, BI, TID)                                                                                        \
    {                                                                                                                \
        _Pragma("unroll kn_flush_unroll") for (int f_ = 0; f_ < KN_BUF; f_++) {                                      \
            if (__ballot(f_ < cnt) == 0ull) break; /* wave-uniform */                                                \
            const unsigned i_ = f_ < cnt ? BI[f_][TID] : 0xFFFFFFFFu;                                                \
            kn_insert<KB>(L, i_ == 0xFFFFFFFFu ? ~0ull : kn_key(BD[f_][TID], i_));                                   \
        }                                                                                                            \
        cnt = 0;                                                                                                     \
        thr = kn_thr(L[KB - 1]);                                                                                     \
    }

// ---- scan: one lane per query, every candidate (box_bound.hpp ts_stream) ----------------------------------------------------
// RAGGED (rf_knn_lengths; the counts arrive as rfi::Counts, group_internal.hpp): the candidates are the sample's first nv points,
// the queries its first mv.  The list is opened for kv = min(k, nv) neighbours -- a sample with fewer candidates than k could not
// fill k slots, and the unfilled ones would go out as the keys they start with -- so slots [0, kv) are the op's with k = kv,
// and slots [kv, k) and the rows of padded queries are written as zeros; a wave of padded queries writes them and leaves.
template <int KB, bool RAGGED = false>
__global__ __launch_bounds__(KN_TPB) void knn_scan_kernel(int n, int m, int k, const float *__restrict__ xyz1,
                                                          const float *__restrict__ xyz2, float *__restrict__ val,
                                                          int *__restrict__ idx, rfi::Counts<RAGGED> lens) {
    const int bi = blockIdx.y;
    const int j = blockIdx.x * KN_TPB + threadIdx.x;
    const float *__restrict__ C = xyz1 + (size_t)bi * n * 3;
    const float *__restrict__ Q = xyz2 + (size_t)bi * m * 3;
    const int nv = rfi::count1(lens, bi, n), mv = rfi::count2(lens, bi, m);
    const int kv = RAGGED ? min(k, nv) : k;
    if (RAGGED && (int)(blockIdx.x * KN_TPB + (threadIdx.x & ~63u)) >= mv) {  // (uniform) a wave of padded queries
        if (j < m) kn_zero(0, k, val + ((size_t)bi * m + j) * k, idx + ((size_t)bi * m + j) * k);
        return;
    }
    const int jj = min(j, m - 1);
    const float x2 = Q[jj * 3], y2 = Q[jj * 3 + 1], z2 = Q[jj * 3 + 2];
    u64 L[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) L[t] = t < KB - kv ? 0ull : ~0ull;
    float thr = __uint_as_float(0x7FC00000u);
    __shared__ float bd[KN_BUF][KN_TPB];
    __shared__ unsigned bx[KN_BUF][KN_TPB];
    const int tid = threadIdx.x;
    int cnt = 0;
    constexpr int kn_flush_unroll = KB <= 8 ? KN_BUF : 1;
    auto consider = [&](float cx, float cy, float cz, int ci) __attribute__((always_inline)) {
        const float dx = cx - x2, dy = cy - y2, dz = cz - z2;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float d = (xx + yy) + zz;
        const bool in = !(d >= thr);
        if (__ballot(in) != 0ull) {  // wave-uniform
            asm volatile("; some lane admits");
            if (in) {
                bd[cnt][tid] = d;
                bx[cnt][tid] = (unsigned)ci;
                cnt++;
            }
            if (__ballot(cnt == KN_BUF) != 0ull) KN_FLUSH(bd, bx, tid);
        }
    };
    ts_stream(C, nv, consider);
    KN_FLUSH(bd, bx, tid);
    if (j < mv) kn_write<KB>(L, kv, val + ((size_t)bi * m + j) * k, idx + ((size_t)bi * m + j) * k);
    if (RAGGED && j < m) kn_zero(j < mv ? kv : 0, k, val + ((size_t)bi * m + j) * k, idx + ((size_t)bi * m + j) * k);
}

// ---- boxed: the walk of box_bound.hpp with knn's list ----------------------------------------------------------------------
template <int KB>
struct KnList {
    // NaN ranks first and +inf is admitted while a list is not full: superblocks at +inf are visited, and a wave with a
    // non-finite query or candidate set (whose points the boxes leave out) walks every superblock untested
    static constexpr bool kNonFinite = true;
    u64 L[KB];
    float thr;
    bool search;
    __device__ __forceinline__ KnList(bool search_, int k) : search(search_) {
#pragma unroll
        for (int t = 0; t < KB; t++) L[t] = (search && t >= KB - k) ? ~0ull : 0ull;
        thr = search ? __uint_as_float(0x7FC00000u) : -INFINITY;
    }
    // +inf while the list is not full (thr NaN; only in a finite wave, where thr is never -inf); -inf in a lane that does not
    // search, which no bound is <=
    __device__ __forceinline__ float prune() const { return thr != thr ? INFINITY : thr; }
    // ties pass: visits go in any order and the keys settle them.  A lane that does not search admits nothing.
    __device__ __forceinline__ bool admit(float d) const { return !(d > thr) && search; }
    // at once (a buffer as the scan's, flushed inside the visits, pushed this kernel into scratch; the nearest-first order fills
    // the lists early anyway).  A padding record (index -1) is keyed above everything.
    __device__ __forceinline__ void insert(float d, int oi, bool in) {
        if (in) {
            kn_insert<KB>(L, oi < 0 ? ~0ull : kn_key(d, (unsigned)oi));
            thr = kn_thr(L[KB - 1]);
        }
    }
};

// RAGGED: both sets were sorted WITH their counts (records, boxes and the non-finite flag are those of the valid points).  The
// list is opened for kv = min(k, nv) neighbours as in the scan: while it is not full every superblock is visited, so the nv >= kv
// real records fill it and the padding records' keys (above everything) never enter.  Rows of padded queries belong to no
// record: the lane at sorted position p writes the zeros of row p where mv <= p < m (npq >= m), before the walk.
template <int KB, bool RAGGED = false>
__global__ __launch_bounds__(64 * TB_WAVES) void knn_boxes_kernel(
    int b, int m, int k, int npq, int npc, const float *__restrict__ qxyz, const int *__restrict__ qorig,
    const float *__restrict__ qb64, const float *__restrict__ cxyz, const int *__restrict__ corig,
    const float *__restrict__ cb16, const float *__restrict__ cb64, const int *__restrict__ cflags,
    float *__restrict__ val, int *__restrict__ idx, int n, rfi::Counts<RAGGED> lens) {
    const TbPlace w = tb_place(npq);
    if (w.group * 64 >= npq) return;  // (uniform)
    const int bi = w.bi;
    const int p = w.group * 64 + (threadIdx.x & 63);
    const int kv = RAGGED ? min(k, rfi::count1(lens, bi, n)) : k;
    if (RAGGED && p >= rfi::count2(lens, bi, m) && p < m) kn_zero(0, k, val + ((size_t)bi * m + p) * k, idx + ((size_t)bi * m + p) * k);
    const float *__restrict__ Q = qxyz + ((size_t)bi * npq + p) * 3;
    TbQuery q;
    q.x = Q[0], q.y = Q[1], q.z = Q[2];
    const int oq = qorig[(size_t)bi * npq + p];
    q.search = oq >= 0;  // (a padding record searches nothing)
    // every superblock, untested: a non-finite query in the wave, or one in the candidate set (the sort's flag, behind pos0)
    q.full = __ballot(q.search && !(isfinite(q.x) && isfinite(q.y) && isfinite(q.z))) != 0ull || cflags[2 * b + bi] != 0;
    q.qb = qb64 + ((size_t)bi * (npq >> 6) + w.group) * 8;
    const int nsb = npc >> 6;
    const TbCands c = {cxyz + (size_t)bi * npc * 3, corig + (size_t)bi * npc, cb16 + (size_t)bi * nsb * 24,
                       cb64 + (size_t)bi * nsb * 8, nsb};
    KnList<KB> L(q.search, kv);
    TbStats st;
    tb_walk(L, q, c, st);
    if (q.search) {
        const size_t o = ((size_t)bi * m + oq) * k;
        kn_write<KB>(L.L, kv, val + o, idx + o);
        if (RAGGED) kn_zero(kv, k, val + o, idx + o);
#ifdef TB_STATS
        idx[o] = st.scans;
#endif
    }
}

// ---- gradient -----------------------------------------------------------------------------------------------------------
constexpr int KG_TPB = 256;

// grad_xyz2[j] = sum_t 2 g (x1[i] - x2[j]); slots whose index is outside [0, n) add nothing
// RAGGED: slots behind the sample's neighbours (t >= nv), slots that name a padded candidate and the slots of padded queries add
// nothing, whatever idx and gval hold there; the rows of padded queries are +0.
template <bool RAGGED = false>
__global__ __launch_bounds__(KG_TPB) void knn_grad_query_kernel(int n, int m, int k, const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, const int *__restrict__ idx,
                                                                const float *__restrict__ gval, float *__restrict__ grad2,
                                                                rfi::Counts<RAGGED> lens) {
    const int bi = blockIdx.y;
    const int j = blockIdx.x * KG_TPB + threadIdx.x;
    if (j >= m) return;
    const float *__restrict__ X1 = xyz1 + (size_t)bi * n * 3;
    const size_t q = (size_t)bi * m + j;
    const int kstride = k;
    if (RAGGED) {
        n = rfi::count1(lens, bi, n);
        k = min(k, n);
        if (j >= rfi::count2(lens, bi, m)) {
            grad2[q * 3] = grad2[q * 3 + 1] = grad2[q * 3 + 2] = 0.f;
            return;
        }
    }
    const float x2 = xyz2[q * 3], y2 = xyz2[q * 3 + 1], z2 = xyz2[q * 3 + 2];
    const int *__restrict__ I = idx + q * kstride;
    const float *__restrict__ G = gval + q * kstride;
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

}  // namespace

extern "C" {

int rf_knn(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx, rf_stream_t stream) {
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!rf::all_given({xyz1, xyz2, val, idx})) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(rf::ceil_div(m, KN_TPB), b);
#define KN_GO(KB) RF_LAUNCH("knn", knn_scan_kernel<KB>, grid, dim3(KN_TPB), 0, s, n, m, k, xyz1, xyz2, val, idx, rfi::Counts<false>{})
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
    if (!rf::all_given({xyz1, xyz2, val, idx}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (!rf::all_aligned16({sorted1, sorted2})) return RF_EINVAL;
    if (workspace_bytes < rf_knn_boxes_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    rfp::Sorted sv[2];
    sv[0] = rfp::sorted_view(b, n, sorted1 ? sorted1 : workspace);
    sv[1] = rfp::sorted_view(b, m, sorted2 ? sorted2 : (const char *)workspace + rfp::sorted_bytes(b, n));
    if (int e = rfp::sort_missing(b, n, m, xyz1, xyz2, sv[0], sv[1], sorted1 != nullptr, sorted2 != nullptr, s)) return e;
    const dim3 grid(rf::ceil_div(sv[1].npad / 64, TB_WAVES) * b);
#define KB_GO(KB)                                                                                                              \
    RF_LAUNCH("knn_boxes", knn_boxes_kernel<KB>, grid, dim3(64 * TB_WAVES), 0, s, b, m, k, sv[1].npad, sv[0].npad, sv[1].xyz, \
              sv[1].orig, sv[1].box64, sv[0].xyz, sv[0].orig, sv[0].box16, sv[0].box64, sv[0].pos0, val, idx, n, rfi::Counts<false>{})
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
    if (!rf::all_given({xyz1, xyz2, idx, grad_val, grad_xyz1, grad_xyz2}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (workspace_bytes < rf_knn_grad_workspace_bytes(b, n, m, k)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    RF_LAUNCH("knn_grad_query", knn_grad_query_kernel<false>, dim3(rf::ceil_div(m, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k, xyz1,
              xyz2, idx, grad_val, grad_xyz2, rfi::Counts<false>{});
    if (int e = rfs::rows_csr_sort(b, n, (long)m * k, idx, workspace, "knn_grad_sort", s)) return e;
    RF_LAUNCH("knn_grad_rows", knn_grad_rows_kernel, dim3(rf::ceil_div(n, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k, xyz1, xyz2,
              grad_val, (const int *)workspace, rfs::rows_csr_perm(b, n, workspace), grad_xyz1);
    return RF_OK;
}

// ---- ragged batches (include/rfops.h).  auto: the boxed form where the Python wrapper takes it for the plain op
// (KNN_BOXES_* of rfnet_amd/_raw.py), by the PADDED sizes.
static int kn_lengths_form(int n, int m, int k, int form) {  // -> RF_GROUP_SCAN / RF_GROUP_BOXES, or -1
    if (form == RF_GROUP_SCAN || form == RF_GROUP_BOXES) return form;
    if (form != RF_GROUP_AUTO) return -1;
    return m >= 8192 && n >= 16384 && k <= 32 ? RF_GROUP_BOXES : RF_GROUP_SCAN;
}

size_t rf_knn_lengths_workspace_bytes(int b, int n, int m, int k, int form) {
    if (!kn_supported(b, n, m, k)) return 0;
    return kn_lengths_form(n, m, k, form) == RF_GROUP_BOXES ? rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m) : 0;
}

int rf_knn_lengths(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *val,
                   int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream, int form) {
    if (b == 0 && n >= 0 && m >= 0 && k >= 0) return RF_OK;
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, val, idx}, {len1, len2}) || !rf::aligned16(workspace)) return RF_EINVAL;
    const int route = kn_lengths_form(n, m, k, form);
    if (route < 0) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const rfi::Counts<true> lens{len1, len2};
    if (route == RF_GROUP_SCAN) {
        const dim3 grid(rf::ceil_div(m, KN_TPB), b);
#define KN_GO(KB) \
    RF_LAUNCH("knn_lengths", (knn_scan_kernel<KB, true>), grid, dim3(KN_TPB), 0, s, n, m, k, xyz1, xyz2, val, idx, lens)
        KN_DISPATCH(k, KN_GO);
#undef KN_GO
        return RF_OK;
    }
    if (!workspace) return RF_EINVAL;
    if (workspace_bytes < rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m)) return RF_EWORKSPACE;
    rfp::Sorted sv[2] = {rfp::sorted_view(b, n, workspace), rfp::sorted_view(b, m, (const char *)workspace + rfp::sorted_bytes(b, n))};
    const int nn[2] = {n, m};
    const float *src[2] = {xyz1, xyz2};
    const int *ls[2] = {len1, len2};
    if (int e = rfp::sort_sets(b, 2, nn, src, sv, s, nullptr, (len1 || len2) ? ls : nullptr)) return e;
    const dim3 grid(rf::ceil_div(sv[1].npad / 64, TB_WAVES) * b);
#define KB_GO(KB)                                                                                                               \
    RF_LAUNCH("knn_boxes_lengths", (knn_boxes_kernel<KB, true>), grid, dim3(64 * TB_WAVES), 0, s, b, m, k, sv[1].npad, sv[0].npad, \
              sv[1].xyz, sv[1].orig, sv[1].box64, sv[0].xyz, sv[0].orig, sv[0].box16, sv[0].box64, sv[0].pos0, val, idx, n, lens)
    KN_DISPATCH(k, KB_GO);
#undef KB_GO
    return RF_OK;
}

size_t rf_knn_grad_lengths_workspace_bytes(int b, int n, int m, int k) { return rf_knn_grad_workspace_bytes(b, n, m, k); }

int rf_knn_grad_lengths(int b, int n, int m, int k, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                        const int *idx, const float *grad_val, float *grad_xyz1, float *grad_xyz2, void *workspace,
                        size_t workspace_bytes, rf_stream_t stream) {
    if (b == 0 && n >= 0 && m >= 0 && k >= 0) return RF_OK;
    if (!kn_supported(b, n, m, k)) return RF_EINVAL;
    if (!rf::all_given({xyz1, xyz2, idx, grad_val, grad_xyz1, grad_xyz2}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (!rf::all_aligned4({len1, len2})) return RF_EINVAL;
    if (workspace_bytes < rf_knn_grad_lengths_workspace_bytes(b, n, m, k)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    RF_LAUNCH("knn_grad_query_lengths", knn_grad_query_kernel<true>, dim3(rf::ceil_div(m, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k,
              xyz1, xyz2, idx, grad_val, grad_xyz2, rfi::Counts<true>{len1, len2});
    if (int e = rfs::rows_csr_sort_masked(b, n, m, k, idx, len1, len2, workspace, "knn_grad_sort_lengths", s)) return e;
    // (a masked slot is in no row, so the rows kernel needs no counts: a padded candidate's row sums nothing and is written +0)
    RF_LAUNCH("knn_grad_rows", knn_grad_rows_kernel, dim3(rf::ceil_div(n, KG_TPB), b), dim3(KG_TPB), 0, s, n, m, k, xyz1, xyz2,
              grad_val, (const int *)workspace, rfs::rows_csr_perm(b, n, workspace), grad_xyz1);
    return RF_OK;
}

}  // extern "C"
