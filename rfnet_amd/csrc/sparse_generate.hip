// sparse_generate.hip -- the decoder's side of the sparse voxel grid: a level that CREATES cells, its pruning, and the lookup of
// one cell set in another (rf_sparse_generate_map, rf_sparse_prune_map, rf_sparse_lookup, rf_sparse_take_rows).  The
// convolution onto the created cells is sparse_stride.hip's RF_SS_UP on the maps made here, its gradients RF_SS_UP_GRAD_INPUT and
// the weight gradient of RF_SS_UP: no kernel of that file changes.  include/rfops.h states the contract; DESIGN.md 5.3v the
// measurements.
//
//   generate one workgroup per sample, as sparse_stride_map_kernel: 64-bit words (48-bit key << 16 | row) of the rows that can be
//            parents in LDS, the bitonic network of lds_sort.hpp; a word whose predecessor has another key is the lowest row of its
//            cell and marks a byte of its ROW in LDS; grid_cluster's workgroup scan over those bytes in row order is the parent's
//            rank, so the children keep the input order.  A row writes its eight entries of child and, when kept, the eight
//            rows of up and coords_out at 8 rank.
//   prune    the same scan over keep[i] != 0, no sort: src, dst and the compacted coords.
//   lookup   sparse_conv_map_kernel with two cell sets: the table's words sorted, every query row one lower-bound search.
//   take     grid_unpool's copy on the lane-row header with two row counts and a count on the destination.
// All four: one launch, no workspace, no atomics in memory, no memset, every output element stored once, counts read on the device.
#include "lane_rows.hpp"
#include "lds_sort.hpp"
#include "sparse_conv.hpp"

namespace {

constexpr int SG_NW = 1024 / 64;
constexpr int SG_TPB = 256;  // take_rows

// The exclusive rank of this thread's flag among the flags of the workgroup's step, plus `run`, the flags of the steps before;
// `run` then takes the step's total.  One barrier per step: the totals alternate between two rows of wtot.
__device__ __forceinline__ unsigned sg_rank(bool f, unsigned &run, unsigned (*wtot)[SG_NW], int it, int lane, int wave, int nw) {
    const unsigned incl = rf::wave_incl_scan(f ? 1u : 0u);
    if (lane == 63) wtot[it & 1][wave] = incl;
    __syncthreads();
    unsigned base = run;
    for (int q = 0; q < nw; q++) {
        const unsigned t = wtot[it & 1][q];
        base += q < wave ? t : 0u;
        run += t;
    }
    return base + incl - (f ? 1u : 0u);
}

__device__ __forceinline__ bool sg_parent_range(int x, int y, int z) {  // 2 c + bit stays in [-32768, 32767]
    return x >= -16384 && x <= 16383 && y >= -16384 && y <= 16383 && z >= -16384 && z <= 16383;
}

// ---- the generative level map --------------------------------------------------------------------------------------------------
// grid (b); dynamic LDS: the P words of the largest sample the launch admits and a byte per row behind them
__global__ __launch_bounds__(1024) void sparse_generate_map_kernel(int nc, int nf, const int *__restrict__ coords,
                                                                   const int *__restrict__ count, int *__restrict__ coords_out,
                                                                   int *__restrict__ count_out, int *__restrict__ total_out,
                                                                   int *__restrict__ child, int *__restrict__ up) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sg_words[];  // [P], then P bytes
    __shared__ unsigned wtot[2][SG_NW];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int M = sc_count(count, s, nc);
    const int *__restrict__ C = coords + (size_t)s * nc * 3;
    int *__restrict__ CO = coords_out + (size_t)s * nf * 3;
    int *__restrict__ CH = child + (size_t)s * nc * 8;
    int *__restrict__ UP = up + (size_t)s * nf;
    int P = 64;
    while (P < M) P <<= 1;
    unsigned char *__restrict__ flag = (unsigned char *)(sg_words + P);  // [P]: row i is a parent

    // 1. the words of the rows that can be parents (rows behind M are not read).  A row in [-32768, 32767] but outside the
    // parents' range has its duplicates outside it too, so the LIVE rule needs those rows in no comparison.
    for (int i = tid; i < P; i += nt) {
        unsigned long long w = SC_PAD;
        if (i < M) {
            const int x = C[i * 3], y = C[i * 3 + 1], z = C[i * 3 + 2];
            if (sg_parent_range(x, y, z)) w = sc_key(x, y, z) << 16 | (unsigned)i;
        }
        sg_words[sw_at(i)] = w;
        flag[i] = 0;
    }
    __syncthreads();

    // 2. the network: ascending (key, row), so the first word of a key is its lowest row, the live one
    sw_sort(sg_words, P, tid, nt);

    // 3. the first word of every key marks its row
    for (int r = tid; r < P; r += nt) {
        const unsigned long long w = sg_words[sw_at(r)];
        if (w != SC_PAD && (r == 0 || (sg_words[sw_at(r - 1)] >> 16) != (w >> 16))) flag[(unsigned)w & 0xFFFFu] = 1;
    }
    __syncthreads();

    // 4. the scan in row order and the write-out: every row of child here, a kept parent's eight rows of up and coords_out
    const int cap = nf >> 3;
    unsigned run = 0;
    for (int i0 = 0, it = 0; i0 < nc; i0 += nt, it++) {
        const int i = i0 + tid;
        const bool par = i < M && flag[i] != 0;
        const int r = (int)sg_rank(par, run, wtot, it, lane, wave, nw);
        if (i < nc) {
            const bool kept = par && r < cap;
            for (int t = 0; t < 8; t++) CH[i * 8 + t] = kept ? 8 * r + t : -1;
            if (kept) {
                const int x = 2 * C[i * 3], y = 2 * C[i * 3 + 1], z = 2 * C[i * 3 + 2];
                for (int t = 0; t < 8; t++) {
                    const int f = 8 * r + t;  // < 8 cap <= nf
                    UP[f] = 8 * i + t;
                    CO[f * 3] = x + ((t >> 2) & 1), CO[f * 3 + 1] = y + ((t >> 1) & 1), CO[f * 3 + 2] = z + (t & 1);
                }
            }
        }
    }
    const int D = (int)run, Dk = D < cap ? D : cap;
    for (int e = Dk * 8 + tid; e < nf; e += nt) UP[e] = -1;
    for (int e = Dk * 24 + tid; e < nf * 3; e += nt) CO[e] = 0;
    if (tid == 0) total_out[s] = 8 * D, count_out[s] = 8 * Dk;
}

// ---- the pruning compaction -----------------------------------------------------------------------------------------------------
// grid (b)
__global__ __launch_bounds__(1024) void sparse_prune_map_kernel(int n, int n_out, const int *__restrict__ coords,
                                                                const unsigned char *__restrict__ keep, const int *__restrict__ count,
                                                                int *__restrict__ coords_out, int *__restrict__ count_out,
                                                                int *__restrict__ total_out, int *__restrict__ src, int *__restrict__ dst) {
    __shared__ unsigned wtot[2][SG_NW];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int M = sc_count(count, s, n);
    const int *__restrict__ C = coords + (size_t)s * n * 3;
    const unsigned char *__restrict__ K = keep + (size_t)s * n;
    int *__restrict__ CO = coords_out + (size_t)s * n_out * 3;
    int *__restrict__ SRC = src + (size_t)s * n_out;
    int *__restrict__ DST = dst + (size_t)s * n;
    unsigned run = 0;
    for (int i0 = 0, it = 0; i0 < n; i0 += nt, it++) {
        const int i = i0 + tid;
        const bool sel = i < M && K[i] != 0;  // (rows behind M are not read)
        const int r = (int)sg_rank(sel, run, wtot, it, lane, wave, nw);
        if (i < n) {
            const bool kept = sel && r < n_out;
            DST[i] = kept ? r : -1;
            if (kept) {
                SRC[r] = i;
                CO[r * 3] = C[i * 3], CO[r * 3 + 1] = C[i * 3 + 1], CO[r * 3 + 2] = C[i * 3 + 2];
            }
        }
    }
    const int D = (int)run, Dk = D < n_out ? D : n_out;
    for (int e = Dk + tid; e < n_out; e += nt) SRC[e] = -1;
    for (int e = Dk * 3 + tid; e < n_out * 3; e += nt) CO[e] = 0;
    if (tid == 0) total_out[s] = D, count_out[s] = Dk;
}

// ---- the lookup -----------------------------------------------------------------------------------------------------------------
// grid (b); dynamic LDS: the P words of the largest table the launch admits
__global__ __launch_bounds__(1024) void sparse_lookup_kernel(int n, int m, int shift, const int *__restrict__ coords,
                                                             const int *__restrict__ count, const int *__restrict__ table,
                                                             const int *__restrict__ tcount, int *__restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sl_words[];  // [P]
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int M = sc_count(count, s, n), Mt = sc_count(tcount, s, m);
    const int *__restrict__ C = coords + (size_t)s * n * 3;
    const int *__restrict__ T = table + (size_t)s * m * 3;
    int *__restrict__ IDX = idx + (size_t)s * n;
    int P = 64;
    while (P < Mt) P <<= 1;

    // 1. the table's words: the cell >> shift (the arithmetic shift, a floor) of every usable row
    for (int i = tid; i < P; i += nt) {
        unsigned long long w = SC_PAD;
        if (i < Mt) {
            const int x = T[i * 3], y = T[i * 3 + 1], z = T[i * 3 + 2];
            if (sc_in_range(x, y, z)) w = sc_key(x >> shift, y >> shift, z >> shift) << 16 | (unsigned)i;
        }
        sl_words[sw_at(i)] = w;
    }
    __syncthreads();

    // 2. ascending (key, row): the first word of a key is the lowest row that has it
    sw_sort(sl_words, P, tid, nt);

    // 3. the valid words are the first V
    int V = 0;
    for (int step = P; step > 0; step >>= 1)
        if (V + step <= P && sl_words[sw_at(V + step - 1)] != SC_PAD) V += step;

    // 4. every query row: the first word >= (key << 16) among the V valid ones
    for (int i = tid; i < n; i += nt) {
        int j = -1;
        if (i < M) {
            const int x = C[i * 3], y = C[i * 3 + 1], z = C[i * 3 + 2];
            if (sc_in_range(x, y, z)) {
                const unsigned long long want = sc_key(x, y, z), lo_word = want << 16;
                int lo = 0;
                for (int len = V; len > 0;) {
                    const int hl = len >> 1;
                    if (sl_words[sw_at(lo + hl)] < lo_word) lo += hl + 1, len -= hl + 1;
                    else len = hl;
                }
                if (lo < V) {
                    const unsigned long long f = sl_words[sw_at(lo)];
                    if ((f >> 16) == want) j = (int)((unsigned)f & 0xFFFFu);
                }
            }
        }
        IDX[i] = j;
    }
}

// ---- rows by index ----------------------------------------------------------------------------------------------------------------
struct StArgs {
    int n_src, n_dst, c, tx_log2, bpb;
    const float *src;
    const int *idx, *count;
    float *dst;
};

template <int VEC>
__global__ __launch_bounds__(SG_TPB) void sparse_take_rows_kernel(StArgs a) {
    typedef typename rf::LaneVec<VEC>::T V;
    int bi, bx;
    rf::place_1d(a.bpb, bi, bx);
    const rf::LaneRows<SG_TPB> g(a.tx_log2);
    const int cv = a.c / VEC;
    const int r = bx * g.TY + g.ly;
    if (r >= a.n_dst) return;
    int ix = -1;
    if (r < sc_count(a.count, bi, a.n_dst)) ix = a.idx[(size_t)bi * a.n_dst + r];  // (idx behind the count is not read)
    const bool live = (unsigned)ix < (unsigned)a.n_src;
    const V *__restrict__ S = (const V *)(a.src + (size_t)bi * a.n_src * a.c) + (size_t)(live ? ix : 0) * cv;
    V *__restrict__ D = (V *)(a.dst + (size_t)bi * a.n_dst * a.c) + (size_t)r * cv;
    for (int l = g.lx; l < cv; l += g.TX) {
        V out;
#pragma unroll
        for (int k = 0; k < VEC; k++) rf::lane_set(out, k, 0.f);
        if (live) out = S[l];
        D[l] = out;
    }
}

int sg_pow2(int n) {
    int P = 64;
    while (P < n) P <<= 1;
    return P;
}

}  // namespace

extern "C" {

int rf_sparse_generate_map(int b, int n_coarse, int n_fine, const int *coords, const int *count, int *coords_out, int *count_out,
                           int *total_out, int *child, int *up, rf_stream_t stream) {
    if (b < 0 || n_coarse < 0 || n_fine < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n_fine < 8 || n_fine > RF_GC_MAX_POINTS || n_coarse < 1 || n_coarse > n_fine || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({coords, coords_out, count_out, total_out, child, up}, {count})) return RF_EINVAL;
    const int P = sg_pow2(n_coarse);
    if (int dv = rf::require_device()) return dv;
    // (144 KiB of words and row bytes at 16384 rows: with the scan's static LDS below the 160 KiB a workgroup may take)
    RF_HIP(hipFuncSetAttribute((const void *)sparse_generate_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 147456));
    RF_LAUNCH("sparse_generate_map", sparse_generate_map_kernel, dim3((unsigned)b), dim3(sw_sort_threads(P)),
              (size_t)P * (sizeof(unsigned long long) + 1), (hipStream_t)stream, n_coarse, n_fine, coords, count, coords_out, count_out,
              total_out, child, up);
    return RF_OK;
}

int rf_sparse_prune_map(int b, int n, int n_out, const int *coords, const unsigned char *keep, const int *count, int *coords_out,
                        int *count_out, int *total_out, int *src, int *dst, rf_stream_t stream) {
    if (b < 0 || n < 0 || n_out < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_GC_MAX_POINTS || n_out < 1 || n_out > n || b > 65535) return RF_EINVAL;
    if (!keep || !rf::tensors_ok({coords, coords_out, count_out, total_out, src, dst}, {count})) return RF_EINVAL;
    const int threads = n >= 1024 ? 1024 : rf::round_up(n, 64);
    RF_LAUNCH("sparse_prune_map", sparse_prune_map_kernel, dim3((unsigned)b), dim3(threads), 0, (hipStream_t)stream, n, n_out, coords,
              keep, count, coords_out, count_out, total_out, src, dst);
    return RF_OK;
}

int rf_sparse_lookup(int b, int n, int m, int shift, const int *coords, const int *count, const int *table, const int *tcount,
                     int *idx, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_GC_MAX_POINTS || m < 1 || m > RF_GC_MAX_POINTS || b > 65535 || shift < 0 || shift > 15) return RF_EINVAL;
    if (!rf::tensors_ok({coords, table, idx}, {count, tcount})) return RF_EINVAL;
    const int P = sg_pow2(m);
    if (int dv = rf::require_device()) return dv;
    RF_HIP(hipFuncSetAttribute((const void *)sparse_lookup_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RF_LAUNCH("sparse_lookup", sparse_lookup_kernel, dim3((unsigned)b), dim3(sw_sort_threads(P)), (size_t)P * sizeof(unsigned long long),
              (hipStream_t)stream, n, m, shift, coords, count, table, tcount, idx);
    return RF_OK;
}

int rf_sparse_take_rows(int b, int n_src, int n_dst, int c, const float *src, const int *idx, const int *count_dst, float *dst,
                        rf_stream_t stream) {
    if (b < 0 || n_src < 0 || n_dst < 0 || c < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n_src < 1 || n_src > RF_GC_MAX_POINTS || n_dst < 1 || n_dst > RF_GC_MAX_POINTS || c < 1 || c > RF_GP_MAX_CHANNELS || b > 65535)
        return RF_EINVAL;
    if (!rf::tensors_ok({src, idx, dst}, {count_dst})) return RF_EINVAL;
    const bool vec = rf::lane_rows_vec_ok(c, {src, dst});
    const int tx_log2 = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const int bpb = rf::ceil_div(n_dst, SG_TPB >> tx_log2);
    const StArgs a{n_src, n_dst, c, tx_log2, bpb, src, idx, count_dst, dst};
    const dim3 grid((unsigned)((long)bpb * b));
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        RF_LAUNCH("sparse_take_rows", sparse_take_rows_kernel<4>, grid, dim3(SG_TPB), 0, st, a);
    } else {
        RF_LAUNCH("sparse_take_rows", sparse_take_rows_kernel<1>, grid, dim3(SG_TPB), 0, st, a);
    }
    return RF_OK;
}

}  // extern "C"
