// interpolate.hip -- three_nn, three_interpolate and its gradient for gfx950.
//
// The reference has ONLY CPU kernels for these ops (threenn_cpu, threeinterpolate_cpu,
// threeinterpolate_grad_cpu: tf_ops/interpolation/tf_interpolate.cpp:60-153), so the parity
// target is the g++ x86-64 arithmetic: the squared distance is the UNFUSED float expression
// ((dx*dx)+(dy*dy))+(dz*dz), the interpolation is (p1*w1 + p2*w2) + p3*w3 with every product
// rounded.  This file is compiled with -ffp-contract=off and uses no fmaf(), so dist / idx /
// out are bit-exact with oracle/rfops_oracle.c (and with the reference CPU bodies).
//
// three_nn: one lane per unknown point; the known set is wave-uniform and streamed through SGPRs
// (box_bound.hpp ts_stream, shared with knn_scan_kernel).  A candidate enters the lane's sorted
// triple only if d < b3; that test is one compare, and the insertion chain sits behind a
// wave-uniform branch (taken for ~half of the candidates at m = 1024, ever more rarely as m
// grows), instead of being predicated over every pair.
//
// three_nn over SORTED clouds (three_nn_boxes_kernel, rf_threenn_boxes): the boxed walk of box_bound.hpp (tb_walk, shared with
// knn_boxes_kernel) with three_nn's list, TnList.  A wave takes 64 consecutive sorted unknown points and visits only the
// candidate blocks whose box can still hold a point at or inside some lane's third-best distance.  The scan visits candidates in
// index order and inserts on strict '<': its result is the three smallest by (distance, index); the boxed form visits them in
// any order and inserts by that pair -- the same triple, ties included.
#include "common.hpp"
#include "lane_rows.hpp"
#include "scatter_rows.hpp"
#include "nn_pruned.hpp"
#include "box_bound.hpp"
#include "group_internal.hpp"

namespace {

constexpr int TN_TPB = 256;

// RAGGED (rf_threenn_lengths; the counts arrive as rfi::Counts, group_internal.hpp): the unknown points are the sample's first
// nv, the known ones its first mv -- the stream ends there -- and the rows behind nv are written as zeros; a wave of padded
// rows writes them and leaves.
template <bool RAGGED = false>
__global__ __launch_bounds__(TN_TPB) void three_nn_kernel(int n, int m,
                                                          const float *__restrict__ xyz1,
                                                          const float *__restrict__ xyz2,
                                                          float *__restrict__ dist,
                                                          int *__restrict__ idx, rfi::Counts<RAGGED> lens) {
    const int bi = blockIdx.y;
    const int j = blockIdx.x * TN_TPB + threadIdx.x;
    const int nv = rfi::count1(lens, bi, n), mv = rfi::count2(lens, bi, m);
    if (RAGGED && (int)(blockIdx.x * TN_TPB + (threadIdx.x & ~63u)) >= nv) {  // (uniform) a wave of padded rows
        if (j < n) {
            const size_t o = ((size_t)bi * n + j) * 3;
            dist[o] = dist[o + 1] = dist[o + 2] = 0.f;
            idx[o] = idx[o + 1] = idx[o + 2] = 0;
        }
        return;
    }
    const float *__restrict__ U = xyz1 + (size_t)bi * n * 3;
    const float *__restrict__ K = xyz2 + (size_t)bi * m * 3;
    const int jj = min(j, n - 1);
    const float x1 = U[jj * 3], y1 = U[jj * 3 + 1], z1 = U[jj * 3 + 2];
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int i1 = 0, i2 = 0, i3 = 0;
    // One candidate.  The insertion is select-only (2 compares, 10 selects): strict '<' everywhere, so an earlier index keeps
    // its place on ties, exactly the reference's if / else-if chain (tf_interpolate.cpp:78-93).
    auto consider = [&](float cx, float cy, float cz, int kk) __attribute__((always_inline)) {
        const float dx = cx - x1, dy = cy - y1, dz = cz - z1;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float d = (xx + yy) + zz;
        const bool in = d < b3;
        if (__ballot(in) != 0ull) {  // wave-uniform
            asm volatile("; some lane inserts");  // keeps this a real branch (grouping.hip)
            if (in) {
                const bool c1 = d < b1, c2 = d < b2;
                b3 = c2 ? b2 : d;
                i3 = c2 ? i2 : kk;
                b2 = c1 ? b1 : (c2 ? d : b2);
                i2 = c1 ? i1 : (c2 ? kk : i2);
                b1 = c1 ? d : b1;
                i1 = c1 ? kk : i1;
            }
        }
    };
    ts_stream(K, mv, consider);
    if (j < nv) {
        size_t o = ((size_t)bi * n + j) * 3;
        dist[o] = b1; dist[o + 1] = b2; dist[o + 2] = b3;
        idx[o] = i1;  idx[o + 1] = i2;  idx[o + 2] = i3;
    } else if (RAGGED && j < n) {
        const size_t o = ((size_t)bi * n + j) * 3;
        dist[o] = dist[o + 1] = dist[o + 2] = 0.f;
        idx[o] = idx[o + 1] = idx[o + 2] = 0;
    }
}


// ---- three_nn over sorted clouds: the walk of box_bound.hpp with three_nn's list --------------------------------------------
// The three best as 64-bit keys (distance bits, index): a squared distance is never negative, so its bit pattern orders as the
// float does, a NaN above +inf; "smaller key" is then the scan's strict '<' in index order, ties included, in ONE comparison.
// Unfilled slots are (+inf, 0) as the op leaves them.
struct TnList {
    typedef unsigned long long u64;
    static constexpr u64 kInf = (u64)0x7f800000u << 32;
    // a key must be below (+inf, 0) to enter, so a non-finite distance never does (tf_interpolate.cpp:78-93: every comparison
    // fails): no superblock at +inf is visited, and there is no untested walk
    static constexpr bool kNonFinite = false;
    u64 k1, k2, k3;
    // a lane that does not search holds zeros -- no key is below them -- until the end
    __device__ __forceinline__ explicit TnList(bool search) : k1(search ? kInf : 0ull), k2(k1), k3(k1) {}
    // the third-best distance (0 in a lane that does not search: its point is padding or non-finite, at +inf from every box)
    __device__ __forceinline__ float prune() const { return __uint_as_float((unsigned)(k3 >> 32)); }
    __device__ __forceinline__ bool admit(float d) const { return d <= prune(); }
    // by the keys alone, in every lane (one whose pre-test failed has a key that is not below k3; a padding record, index -1 =
    // the largest unsigned, coordinates +inf, is not below (+inf, 0))
    __device__ __forceinline__ void insert(float d, int oi, bool) {
        const u64 key = ((u64)__float_as_uint(d) << 32) | (u64)(unsigned)oi;
        const bool c3 = key < k3, c2 = key < k2, c1 = key < k1;
        k3 = c3 ? (c2 ? k2 : key) : k3;
        k2 = c2 ? (c1 ? k1 : key) : k2;
        k1 = c1 ? key : k1;
    }
};

// RAGGED: both sets were sorted WITH their counts, so the records and boxes are those of the valid points and the walk needs
// nothing more.  The rows of padded unknown points belong to no record: the lane at sorted position p writes the zeros of row p
// where nv <= p < n (npq >= n: every such row has its lane) -- in this launch, before the walk, no fill pass.
template <bool RAGGED = false>
__global__ __launch_bounds__(64 * TB_WAVES) void three_nn_boxes_kernel(
    int n, int npq, int npc, const float *__restrict__ qxyz, const int *__restrict__ qorig, const float *__restrict__ qb64,
    const float *__restrict__ cxyz, const int *__restrict__ corig, const float *__restrict__ cb16,
    const float *__restrict__ cb64, float *__restrict__ dist, int *__restrict__ idx, rfi::Counts<RAGGED> lens) {
    const TbPlace w = tb_place(npq);
    if (w.group * 64 >= npq) return;  // (uniform)
    const int bi = w.bi;
    const int p = w.group * 64 + (threadIdx.x & 63);
    if (RAGGED && p >= rfi::count1(lens, bi, n) && p < n) {
        const size_t o = ((size_t)bi * n + p) * 3;
        dist[o] = dist[o + 1] = dist[o + 2] = 0.f;
        idx[o] = idx[o + 1] = idx[o + 2] = 0;
    }
    const float *__restrict__ Q = qxyz + ((size_t)bi * npq + p) * 3;
    TbQuery q;
    q.x = Q[0], q.y = Q[1], q.z = Q[2];
    const int oq = qorig[(size_t)bi * npq + p];
    // a point with a NaN or infinite coordinate is at a NaN or infinite distance from everything: nothing is ever inserted
    // (tf_interpolate.cpp:78-93: every comparison fails) and it takes no part in the search
    q.search = oq >= 0 && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    q.full = false;
    q.qb = qb64 + ((size_t)bi * (npq >> 6) + w.group) * 8;
    const int nsb = npc >> 6;
    const TbCands c = {cxyz + (size_t)bi * npc * 3, corig + (size_t)bi * npc, cb16 + (size_t)bi * nsb * 24,
                       cb64 + (size_t)bi * nsb * 8, nsb};
    TnList L(q.search);
    TbStats st;
    tb_walk(L, q, c, st);
    if (oq >= 0) {
        if (!q.search) L.k1 = L.k2 = L.k3 = TnList::kInf;
        const size_t o = ((size_t)bi * n + oq) * 3;
        dist[o] = __uint_as_float((unsigned)(L.k1 >> 32));
        dist[o + 1] = __uint_as_float((unsigned)(L.k2 >> 32));
        dist[o + 2] = __uint_as_float((unsigned)(L.k3 >> 32));
        idx[o] = (int)(unsigned)L.k1;
#ifdef TB_STATS
        idx[o + 1] = st.visits, idx[o + 2] = st.scans;
#else
        idx[o + 1] = (int)(unsigned)L.k2;
        idx[o + 2] = (int)(unsigned)L.k3;
#endif
    }
}

// ---- three_interpolate / its gradient, row-shaped --------------------------------------------------------------------------
// One element per thread (the kernels below) pays a 64-bit division per output element and six index / weight loads for four
// bytes of output: 1.7 TB/s forward, 0.5 TB/s backward at 32 x 16384 x 1024, c = 128.  Here a thread row owns an unknown point:
// its three indices and weights are loaded once, the channels go by as VEC-wide vectors over the row's lanes (32-bit
// arithmetic, no division).  Same expression per element: (p1*w1 + p2*w2) + p3*w3, every product rounded (-ffp-contract=off).
constexpr int TI_TPB = 256;
constexpr int TI_PP = 4;  // points per thread row and block

template <int VEC>
__global__ __launch_bounds__(TI_TPB) void three_interpolate_rows_kernel(int m, int c, int n, int tx_log2, int bpb /* blocks per sample */,
                                                                        const float *__restrict__ points,
                                                                        const int *__restrict__ idx,
                                                                        const float *__restrict__ weight,
                                                                        float *__restrict__ out) {
    typedef typename rf::LaneVec<VEC>::T V;
    // (a sample's blocks on ONE XCD: its rows of `points` then cross the fabric once instead of eight times -- FETCH_SIZE 71 -> 14 MB, 68 -> 57 us)
    int bi, bx;
    rf::place_1d(bpb, bi, bx);
    const rf::LaneRows<TI_TPB> g(tx_log2);
    const int cv = c / VEC;
    const V *__restrict__ P = (const V *)(points + (size_t)bi * m * c);
    V *__restrict__ O = (V *)(out + (size_t)bi * n * c);
    const int *__restrict__ I = idx + (size_t)bi * n * 3;
    const float *__restrict__ W = weight + (size_t)bi * n * 3;
    int r[TI_PP][3];
    float w[TI_PP][3];
    int jj[TI_PP];
#pragma unroll
    for (int u = 0; u < TI_PP; u++) {
        jj[u] = (bx * TI_PP + u) * g.TY + g.ly;
        const int j = min(jj[u], n - 1);
#pragma unroll
        for (int t = 0; t < 3; t++) {
            r[u][t] = I[j * 3 + t] * cv;
            w[u][t] = W[j * 3 + t];
        }
    }
    for (int l = g.lx; l < cv; l += g.TX) {
        V a[TI_PP], b2[TI_PP], d[TI_PP];
#pragma unroll
        for (int u = 0; u < TI_PP; u++) a[u] = P[r[u][0] + l], b2[u] = P[r[u][1] + l], d[u] = P[r[u][2] + l];
#pragma unroll
        for (int u = 0; u < TI_PP; u++) {
            if (jj[u] < n)  // (written once, read by another kernel: past the caches)
                __builtin_nontemporal_store((a[u] * w[u][0] + b2[u] * w[u][1]) + d[u] * w[u][2], &O[(size_t)jj[u] * cv + l]);
        }
    }
}

// The gradient: a workgroup owns a SLICE of cs channels of one sample's (m, c) gradient as an LDS tile of doubles -- ds_add_f64
// runs at 18 lane-operations per ns and CU against 0.8 for ds_add_f32 (tools/ubench/lds_atomic_rate.hip), and L2 atomics from
// every element (the kernel below) reach 0.3 per ns and CU -- and walks a part of the unknown points: grad_out is read once,
// cs * 4 bytes per point and workgroup; the tile leaves as plain stores (one part) or atomic adds (several).
#ifndef RFI_TG_WGS
#define RFI_TG_WGS 256
#endif
constexpr int TG_TPB = 1024;  // (128 KiB of LDS: one workgroup per CU -- its 16 waves are all the loads in flight there are)
constexpr int TG_U = 4;  // points per thread row in flight

template <int VEC, bool POW2>  // POW2: cs is a power of two (shifts instead of multiplications and a division)
__global__ __launch_bounds__(TG_TPB) void three_interpolate_grad_tile_kernel(int m, int c, int n, int cs, int tx_log2,
                                                                             int nslices, int parts,
                                                                             const float *__restrict__ grad_out,
                                                                             const int *__restrict__ idx,
                                                                             const float *__restrict__ weight,
                                                                             float *__restrict__ grad_points) {
    typedef typename rf::LaneVec<VEC>::T V;
    extern __shared__ __attribute__((aligned(16))) double ti_tile[];  // [m * cs]; cs = VEC << tx_log2, or (VEC == 1) any cs <= 1 << tx_log2
    // (a sample's slices and parts on ONE XCD: neighbouring slices share the cache lines of grad_out's rows)
    int bi, bx;
    rf::place_1d(nslices * parts /* workgroups per sample */, bi, bx);
    const int slice = bx % nslices, part = bx / nslices;
    const rf::LaneRows<TG_TPB> lr(tx_log2);
    const int TY = lr.TY, lx = lr.lx, ly = lr.ly;
    const bool lane_on = POW2 || lx * VEC < cs;  // (a slice of 3 or 13 channels leaves the last lanes of its rows idle)
    const int csl = POW2 ? 31 - __clz(cs) : 0;
    for (int e = threadIdx.x; e < m * cs; e += TG_TPB) ti_tile[e] = 0.0;
    const int per = (n + parts - 1) / parts;
    const int jbeg = part * per, jend = min(n, jbeg + per);
    const float *__restrict__ G = grad_out + (size_t)bi * n * c + slice * cs + (lane_on ? lx * VEC : 0);
    const int *__restrict__ I = idx + (size_t)bi * n * 3;
    const float *__restrict__ W = weight + (size_t)bi * n * 3;
    __syncthreads();
    // a point's cs sums sit v-major in the tile (channel lx * VEC + v at v * TX + lx): the lanes of a row then add to consecutive
    // doubles in every instruction; the next batch of points is loaded before this one is added (two waves per SIMD at 128 KiB
    // of LDS: nothing else hides the loads)
    const int rot = VEC == 4 ? (ly & 3) : 0;  // this row's first channel of four
    int voff[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) voff[k] = ((k + rot) & (VEC - 1)) << tx_log2;
    V g[TG_U], gn[TG_U];
    int r[TG_U][3], rn[TG_U][3];
    float w[TG_U][3], wn[TG_U][3];
#define TG_LOAD(GG, RR, WW, J0)                                                   \
    _Pragma("unroll") for (int u = 0; u < TG_U; u++) {                            \
        const int j = min((J0) + u * TY, jend - 1);                               \
        GG[u] = *(const V *)(G + (size_t)j * c);                                  \
        _Pragma("unroll") for (int t = 0; t < 3; t++) {                           \
            RR[u][t] = (POW2 ? I[j * 3 + t] << csl : I[j * 3 + t] * cs) + lx;     \
            WW[u][t] = W[j * 3 + t];                                              \
        }                                                                         \
    }
    if (jbeg + ly < jend) {
        TG_LOAD(g, r, w, jbeg + ly)
    }
    for (int j0 = jbeg + ly; j0 < jend; j0 += TY * TG_U) {
        const bool more = j0 + TY * TG_U < jend;
        if (more) {
            TG_LOAD(gn, rn, wn, j0 + TY * TG_U)
        }
        // (neighbouring rows start at different channels: in one instruction the rows of a wave would otherwise all add to the
        // same 8 banks of their points' 32)
        float gr[TG_U][VEC];
#pragma unroll
        for (int u = 0; u < TG_U; u++)
#pragma unroll
            for (int k = 0; k < VEC; k++) {
                float x = rf::lane_at(g[u], k);
                if (VEC == 4) {
                    const float y = rf::lane_at(g[u], (k + 1) & 3), z = rf::lane_at(g[u], (k + 2) & 3), q = rf::lane_at(g[u], (k + 3) & 3);
                    x = rot == 0 ? x : (rot == 1 ? y : (rot == 2 ? z : q));
                }
                gr[u][k] = x;
            }
#pragma unroll
        for (int u = 0; u < TG_U; u++) {
            if (j0 + u * TY < jend && lane_on) {
#pragma unroll
                for (int t = 0; t < 3; t++)
#pragma unroll
                    for (int k = 0; k < VEC; k++) atomicAdd(&ti_tile[r[u][t] + voff[k]], (double)(gr[u][k] * w[u][t]));
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < TG_U; u++) {
                g[u] = gn[u];
#pragma unroll
                for (int t = 0; t < 3; t++) r[u][t] = rn[u][t], w[u][t] = wn[u][t];
            }
        }
    }
#undef TG_LOAD
    __syncthreads();
    float *__restrict__ GP = grad_points + (size_t)bi * m * c + slice * cs;
    for (int e = threadIdx.x; e < m * cs; e += TG_TPB) {
        const int i = POW2 ? e >> csl : e / cs, ch = e - i * cs;
        const float v = (float)ti_tile[i * cs + (ch % VEC << tx_log2) + ch / VEC];
        if (parts == 1) {
            GP[(size_t)i * c + ch] = v;
        } else {
            atomicAdd(&GP[(size_t)i * c + ch], v);
        }
    }
}

__global__ void three_interpolate_kernel(int m, int c, int n, long total,
                                         const float *__restrict__ points,
                                         const int *__restrict__ idx,
                                         const float *__restrict__ weight, float *__restrict__ out) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    long bj = e / c;  // b*n + j
    int l = (int)(e - bj * c);
    long bi = bj / n;
    const float *P = points + bi * m * c;
    float a = P[(long)idx[bj * 3 + 0] * c + l] * weight[bj * 3 + 0];
    float b = P[(long)idx[bj * 3 + 1] * c + l] * weight[bj * 3 + 1];
    float d = P[(long)idx[bj * 3 + 2] * c + l] * weight[bj * 3 + 2];
    out[e] = (a + b) + d;
}

__global__ void three_interpolate_grad_kernel(int m, int c, int n, long total,
                                              const float *__restrict__ grad_out,
                                              const int *__restrict__ idx,
                                              const float *__restrict__ weight,
                                              float *__restrict__ grad_points) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    long bj = e / c;
    int l = (int)(e - bj * c);
    long bi = bj / n;
    float *G = grad_points + bi * m * c;
    float g = grad_out[e];
#pragma unroll
    for (int t = 0; t < 3; t++) atomicAdd(&G[(long)idx[bj * 3 + t] * c + l], g * weight[bj * 3 + t]);
}

}  // namespace

extern "C" {

int rf_threenn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx,
               rf_stream_t stream) {
    if (b < 0 || b > 65535 || n < 0 || m < 0) return RF_EINVAL;  // the batch is grid.y
    if (b == 0 || n == 0) return RF_OK;
    if (!xyz1 || !dist || !idx || (m > 0 && !xyz2)) return RF_EINVAL;
    RF_LAUNCH("three_nn", three_nn_kernel<false>, dim3(rf::ceil_div(n, TN_TPB), b), dim3(TN_TPB), 0,
              (hipStream_t)stream, n, m, xyz1, xyz2, dist, idx, rfi::Counts<false>{});
    return RF_OK;
}

// ---- the boxed form: needs scratch (the sorted copies of the two sets unless the caller hands rf_nn_sort handles over)
size_t rf_threenn_boxes_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || b > 65535 || !rfp::pruned_supported(b, n, m)) return 0;
    return rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m);
}

int rf_threenn_boxes(int b, int n, int m, const float *xyz1, const float *xyz2, const void *sorted1, const void *sorted2,
                     float *dist, int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0) return RF_EINVAL;
    if (b == 0 || n == 0) return RF_OK;
    if (b > 65535 || !rfp::pruned_supported(b, n, m)) return RF_EINVAL;  // (m = 0 and huge clouds: rf_threenn)
    if (!rf::all_given({xyz1, xyz2, dist, idx}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (!rf::all_aligned16({sorted1, sorted2})) return RF_EINVAL;
    if (workspace_bytes < rf_threenn_boxes_workspace_bytes(b, n, m)) return RF_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    rfp::Sorted sv[2];
    sv[0] = rfp::sorted_view(b, n, sorted1 ? sorted1 : workspace);
    sv[1] = rfp::sorted_view(b, m, sorted2 ? sorted2 : (const char *)workspace + rfp::sorted_bytes(b, n));
    if (int e = rfp::sort_missing(b, n, m, xyz1, xyz2, sv[0], sv[1], sorted1 != nullptr, sorted2 != nullptr, s)) return e;
    RF_LAUNCH("three_nn_boxes", three_nn_boxes_kernel<false>, dim3(rf::ceil_div(sv[0].npad / 64, TB_WAVES) * b), dim3(64 * TB_WAVES), 0, s,
              n, sv[0].npad, sv[1].npad, sv[0].xyz, sv[0].orig, sv[0].box64, sv[1].xyz, sv[1].orig, sv[1].box16, sv[1].box64,
              dist, idx, rfi::Counts<false>{});
    return RF_OK;
}

// ---- ragged batches (include/rfops.h).  auto: the boxed form where the Python wrapper takes it for the plain op without sort
// handles (TN_BOXES_* of rfnet_amd/_raw.py), by the PADDED sizes.
static int tn_lengths_form(int b, int n, int m, int form) {  // -> RF_GROUP_SCAN / RF_GROUP_BOXES, or -1
    const bool domain = b <= 65535 && rfp::pruned_supported(b, n, m);
    if (form == RF_GROUP_SCAN) return RF_GROUP_SCAN;
    if (form == RF_GROUP_BOXES) return domain ? RF_GROUP_BOXES : -1;
    if (form != RF_GROUP_AUTO) return -1;
    const double pairs = (double)b * n * m;
    const bool small = (n > m ? n : m) <= 16384;
    const bool pays = n >= 1024 && m >= 512 && (pairs >= (small ? 1e8 : 4e9) || (m >= 1536 && n >= 4096 && small));
    return domain && pays ? RF_GROUP_BOXES : RF_GROUP_SCAN;
}

size_t rf_threenn_lengths_workspace_bytes(int b, int n, int m, int form) {
    if (b <= 0 || b > 65535 || n <= 0 || m <= 0) return 0;
    return tn_lengths_form(b, n, m, form) == RF_GROUP_BOXES ? rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m) : 0;
}

int rf_threenn_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *dist,
                       int *idx, void *workspace, size_t workspace_bytes, rf_stream_t stream, int form) {
    if (b < 0 || b > 65535 || n < 0 || m < 0) return RF_EINVAL;  // the batch is grid.y
    if (b == 0) return RF_OK;
    if (n == 0 || m == 0) return RF_EINVAL;  // counts are at least 1
    if (!rf::tensors_ok({xyz1, xyz2, dist, idx}, {len1, len2}) || !rf::aligned16(workspace)) return RF_EINVAL;
    const int route = tn_lengths_form(b, n, m, form);
    if (route < 0) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const rfi::Counts<true> lens{len1, len2};
    if (route == RF_GROUP_SCAN) {
        RF_LAUNCH("three_nn_lengths", three_nn_kernel<true>, dim3(rf::ceil_div(n, TN_TPB), b), dim3(TN_TPB), 0, s, n, m, xyz1, xyz2,
                  dist, idx, lens);
        return RF_OK;
    }
    if (!workspace) return RF_EINVAL;
    if (workspace_bytes < rfp::sorted_bytes(b, n) + rfp::sorted_bytes(b, m)) return RF_EWORKSPACE;
    rfp::Sorted sv[2] = {rfp::sorted_view(b, n, workspace), rfp::sorted_view(b, m, (const char *)workspace + rfp::sorted_bytes(b, n))};
    const int nn[2] = {n, m};
    const float *src[2] = {xyz1, xyz2};
    const int *ls[2] = {len1, len2};
    if (int e = rfp::sort_sets(b, 2, nn, src, sv, s, nullptr, (len1 || len2) ? ls : nullptr)) return e;
    RF_LAUNCH("three_nn_boxes_lengths", three_nn_boxes_kernel<true>, dim3(rf::ceil_div(sv[0].npad / 64, TB_WAVES) * b),
              dim3(64 * TB_WAVES), 0, s, n, sv[0].npad, sv[1].npad, sv[0].xyz, sv[0].orig, sv[0].box64, sv[1].xyz, sv[1].orig,
              sv[1].box16, sv[1].box64, dist, idx, lens);
    return RF_OK;
}

int rf_threeinterpolate(int b, int m, int c, int n, const float *points, const int *idx,
                        const float *weight, float *out, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || c < 0) return RF_EINVAL;
    long total = (long)b * n * c;
    if (total == 0) return RF_OK;
    if (!rf::all_given({points, idx, weight, out})) return RF_EINVAL;
    if (b <= 65535 && (long)n * c < (1L << 31) && (long)m * c < (1L << 31) && (long)n * 3 < (1L << 31)) {
        const bool vec = rf::lane_rows_vec_ok(c, {points, out});
        const int tx_log2 = rf::lane_rows_tx_log2(vec ? c / 4 : c);
        const int ppb = (TI_TPB >> tx_log2) * TI_PP;  // points per block
        const long bpb = rf::ceil_div(n, ppb);
        if (bpb * b <= 0x7FFFFFFF) {
            const dim3 grid((unsigned)(bpb * b));
            if (vec) {
                RF_LAUNCH("three_interpolate", three_interpolate_rows_kernel<4>, grid, dim3(TI_TPB), 0, (hipStream_t)stream, m, c, n,
                          tx_log2, (int)bpb, points, idx, weight, out);
            } else {
                RF_LAUNCH("three_interpolate", three_interpolate_rows_kernel<1>, grid, dim3(TI_TPB), 0, (hipStream_t)stream, m, c, n,
                          tx_log2, (int)bpb, points, idx, weight, out);
            }
            return RF_OK;
        }
    }
    RF_LAUNCH("three_interpolate", three_interpolate_kernel, dim3(rf::ceil_div(total, 256)), dim3(256), 0,
              (hipStream_t)stream, m, c, n, total, points, idx, weight, out);
    return RF_OK;
}

// The LDS-tile form's slice: cs channels with m * cs doubles in 128 KiB -- cs a power of two dividing c (8..64), or, for c that has
// none (3, 6, 13 ...), all c <= 64 channels in one slice; 0: the sample's known points do not fit a tile
static int tig_tile_cs(int b, int n, int c, int m) {
    if (!(b <= 65535 && (long)n * c < (1L << 31) && (long)m * c < (1L << 31) && (long)n * 3 < (1L << 31))) return 0;
    for (int k = 6; k >= 3; k--)
        if (c % (1 << k) == 0 && ((long)m << k) <= 16384) return 1 << k;
    if (c <= 64 && (long)m * c <= 16384) return c;
    return 0;
}
// beyond the tile (more than 2048 known points at 8 channels per slice): the sorted-slots form of scatter_rows.hip, from this
// many gradient elements on (below: the atomics)
constexpr long TIG_CSR_MIN_ELEMS = 1L << 22;
static bool tig_csr(int b, int n, int c, int m) {
    return tig_tile_cs(b, n, c, m) == 0 && (long)b * n * 3 * c >= TIG_CSR_MIN_ELEMS && rfs::rows_csr_supported(b, m, c, (long)n * 3, 3);
}

size_t rf_threeinterpolate_grad_workspace_bytes(int b, int n, int c, int m) {
    if (b <= 0 || n <= 0 || c <= 0 || m <= 0) return 0;
    return tig_csr(b, n, c, m) ? rfs::rows_csr_workspace_bytes(b, m, (long)n * 3) : 0;
}

int rf_threeinterpolate_grad(int b, int n, int c, int m, const float *grad_out, const int *idx,
                             const float *weight, float *grad_points, rf_stream_t stream) {
    return rf_threeinterpolate_grad_ws(b, n, c, m, grad_out, idx, weight, grad_points, nullptr, 0, stream);
}

int rf_threeinterpolate_grad_ws(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                const float *weight, float *grad_points, void *workspace, size_t workspace_bytes,
                                rf_stream_t stream) {

    if (b < 0 || n < 0 || m < 0 || c < 0) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if ((size_t)b * m * c && !grad_points) return RF_EINVAL;
    long total = (long)b * n * c;
    if (total != 0 && m != 0 && (!grad_out || !idx || !weight)) return RF_EINVAL;
    const int cs = (total != 0 && m != 0) ? tig_tile_cs(b, n, c, m) : 0;
    if (cs == 0 && total != 0 && m != 0 && tig_csr(b, n, c, m) && workspace && rf::aligned16(workspace) &&
        workspace_bytes >= rf_threeinterpolate_grad_workspace_bytes(b, n, c, m))
        return rfs::rows_csr_scatter(b, m, c, (long)n * 3, 3, grad_out, idx, weight, grad_points, workspace, "three_interpolate_grad_sort",
                                     "three_interpolate_grad", s);
    if (cs > 0) {
        const bool pow2 = (cs & (cs - 1)) == 0 && cs >= 8;
        const bool vec = pow2 && rf::aligned16(grad_out);  // (rows of a slice start 16-byte aligned when the tensor does)
        const int nslices = c / cs;
        const int tx_log2 = rf::lane_rows_tx_log2(vec ? cs / 4 : cs);  // (cs <= 64: the rows cover the slice in one pass)
        // parts of the unknown points: a workgroup per CU (the tile leaves room for one), every part still thousands of points
        int parts = 1;
        while ((long)b * nslices * parts < RFI_TG_WGS && n / (parts * 2) >= 2048) parts *= 2;
        if (parts > 1) RF_ZERO(grad_points, sizeof(float) * (size_t)b * m * c, s);
        const size_t lds = sizeof(double) * (size_t)m * cs;
        const dim3 grid((unsigned)(nslices * parts * b));
#define TG_GO(KERNEL)                                                                                                      \
    RF_HIP(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));                 \
    RF_LAUNCH("three_interpolate_grad", KERNEL, grid, dim3(TG_TPB), lds, s, m, c, n, cs, tx_log2, nslices, parts, grad_out, idx, \
              weight, grad_points)
        if (vec) {
            TG_GO((three_interpolate_grad_tile_kernel<4, true>));
        } else if (pow2) {
            TG_GO((three_interpolate_grad_tile_kernel<1, true>));
        } else {
            TG_GO((three_interpolate_grad_tile_kernel<1, false>));
        }
#undef TG_GO
        return RF_OK;
    }
    if ((size_t)b * m * c) RF_ZERO(grad_points, sizeof(float) * (size_t)b * m * c, s);
    if (total == 0 || m == 0) return RF_OK;
    RF_LAUNCH("three_interpolate_grad", three_interpolate_grad_kernel, dim3(rf::ceil_div(total, 256)),
              dim3(256), 0, s, m, c, n, total, grad_out, idx, weight, grad_points);
    return RF_OK;
}

}  // extern "C"
