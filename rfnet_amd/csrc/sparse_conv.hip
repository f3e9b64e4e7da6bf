// sparse_conv.hip -- submanifold sparse convolution on the cells of grid_pool.hip's voxel grid (rf_sparse_conv_map,
// rf_sparse_conv, rf_sparse_conv_grad_weight): the output cells are the input cells, a cell sums over those of its ks^3
// offsets that are occupied.  include/rfops.h states the contract; DESIGN.md 5.3t the measurements.
//
//   map      one workgroup per sample, as grid_cluster: 64-bit words (48-bit row-major key of the cell << 16 | row) in LDS, the
//            bitonic network of lds_sort.hpp, a word whose predecessor has the same key is a duplicate, and every (row, slot)
//            is answered by a binary search among the words: nbr (b, n, K), every element written once, no atomics.
//   conv     the second matrix-shaped loop of the library (knn_feature.hip is the first) and the first whose reduction
//            dimension is gathered.  A wave owns 32 consecutive rows and blocks of 32 output channels as accumulators of
//            v_mfma_f32_32x32x2_f32, which IS the contract's fmaf chain: rows as A, the weight slab as B, two channels per
//            instruction, the accumulator carried over the slots in ascending order.  Per slot and slab of 32 channels the
//            wave gathers its 32 feature rows and the weight slab into LDS of its own, through registers one slab ahead, so
//            there is no workgroup barrier anywhere and a wave skips every slot none of its rows has (a ballot over the
//            wave's tile of the map, which sits in LDS as 16-bit row numbers, what lies outside [0, M) already absent).
//            The gradient to the features is the same kernel: the mirrored slot and the transposed weight.
//   wgrad    a wave owns one (sample, slot, 32 input channels, 32 output channels): gathered features as A, grad_out as B,
//            the row index as the instruction's K, pairs of rows of which neither has the slot skipped; an fmaf chain per
//            chunk of RF_SC_WGRAD_ROWS rows, the chunks added in double, a double partial per sample in the workspace, and a
//            second launch that adds the samples in ascending order and rounds once.
#include "lds_sort.hpp"
#include "sparse_conv.hpp"

namespace {

// ---- the kernel map --------------------------------------------------------------------------------------------------------
// grid (b); dynamic LDS: the P words of the largest sample the launch admits
__global__ __launch_bounds__(1024) void sparse_conv_map_kernel(int n, int ks, int dilation, const int *__restrict__ coords,
                                                               const int *__restrict__ count, int *__restrict__ nbr) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sc_words[];  // [P]
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int K = ks * ks * ks, r = ks >> 1;
    const int M = sc_count(count, s, n);
    const int *__restrict__ C = coords + (size_t)s * n * 3;
    int *__restrict__ NB = nbr + (size_t)s * n * K;
    int P = 64;
    while (P < M) P <<= 1;

    // 1. the words; a row behind M or out of range is finished here (rows behind M are not read)
    const int top = P > n ? P : n;
    for (int i = tid; i < top; i += nt) {
        unsigned long long w = SC_PAD;
        if (i < M) {
            const int x = C[i * 3], y = C[i * 3 + 1], z = C[i * 3 + 2];
            if (sc_in_range(x, y, z)) w = sc_key(x, y, z) << 16 | (unsigned)i;
        }
        if (i < P) sc_words[sw_at(i)] = w;
        if (i < n && w == SC_PAD)
            for (int t = 0; t < K; t++) NB[(size_t)i * K + t] = -1;
    }
    __syncthreads();

    // 2. the network: ascending (key, row), so the first word of a key is its lowest row, the live one
    sw_sort(sc_words, P, tid, nt);

    // 3. the valid words are the first V (a padding word is above every valid one)
    int V = 0;
    for (int step = P; step > 0; step >>= 1)  // the largest V <= P with words[V - 1] != PAD
        if (V + step <= P && sc_words[sw_at(V + step - 1)] != SC_PAD) V += step;

    // 4. every (sorted word, slot): a duplicate's row is all -1; a live row looks its neighbour up
    for (int e = tid; e < V * K; e += nt) {
        const int q = e / K, t = e - q * K;
        const unsigned long long w = sc_words[sw_at(q)], key = w >> 16;
        const bool head = q == 0 || (sc_words[sw_at(q - 1)] >> 16) != key;
        const int i = (int)((unsigned)w & 0xFFFFu);  // < M
        int j = -1;
        if (head) {
            const int dz = t % ks - r, dy = (t / ks) % ks - r, dx = t / (ks * ks) - r;
            // (a cell index is within +-32768 and dilation * r within 2048: the sums fit an int)
            const int x = (int)(unsigned)(key >> 32) - 32768 + dilation * dx, y = (int)((unsigned)(key >> 16) & 0xFFFFu) - 32768 + dilation * dy,
                      z = (int)((unsigned)key & 0xFFFFu) - 32768 + dilation * dz;
            if (sc_in_range(x, y, z)) {
                const unsigned long long want = sc_key(x, y, z), lo_word = want << 16;
                int lo = 0;  // the first word >= lo_word among the V valid ones
                for (int len = V; len > 0;) {
                    const int hl = len >> 1;
                    if (sc_words[sw_at(lo + hl)] < lo_word) lo += hl + 1, len -= hl + 1;
                    else len = hl;
                }
                if (lo < V) {
                    const unsigned long long f = sc_words[sw_at(lo)];
                    if ((f >> 16) == want) j = (int)((unsigned)f & 0xFFFFu);
                }
            }
        }
        NB[(size_t)i * K + t] = j;
    }
}

// ---- the convolution -------------------------------------------------------------------------------------------------------
struct ScArgs {
    int n, K, cin, cout;  // cin: the reduction (feat's channels), cout: out's channels, in either mode
    const float *feat, *weight;
    const int *nbr, *count;
    float *out;
};

// grid (ceil(n / 128), b); dynamic LDS: 4 * sc_wave_bytes(NB, K)
template <int MODE, int NB, bool VEC>
__global__ __launch_bounds__(SC_TPB) void sparse_conv_kernel(ScArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bi = blockIdx.y, i0 = blockIdx.x * SC_ROWS + wv * 32;
    const int n = a.n, K = a.K, cin = a.cin, cout = a.cout;
    if (i0 >= n) return;  // (wave-uniform)
    const int M = sc_count(a.count, bi, n);
    float *__restrict__ O = a.out + (size_t)bi * n * cout;
    if (i0 >= M) {  // rows behind the count only: +0
        const int rows = min(32, n - i0);
        for (int e = lane; e < rows * cout; e += 64) O[(size_t)i0 * cout + e] = 0.f;
        return;
    }
    constexpr int LDB = NB == 1 ? 32 : 96;
    constexpr int NQB = NB * 4;  // quads of a weight slab per lane
    float *sA = (float *)(sc_lds + (size_t)wv * sc_wave_bytes(NB, K));
    float *sB = sA + 32 * SC_LD;
    unsigned short *sN = (unsigned short *)(sB + sc_b_floats(NB));
    const float *__restrict__ F = a.feat + (size_t)bi * n * cin;
    const float *__restrict__ W = a.weight;

    // the wave's tile of the map, [row][slot]: a row number in [0, M) or ABSENT (rows behind M are not read)
    {
        const int *__restrict__ NBR = a.nbr + ((size_t)bi * n + i0) * K;
        const int have = min(32, M - i0) * K;
        for (int q = lane; q < 32 * K; q += 64) {
            const int v = q < have ? NBR[q] : -1;
            sN[q] = (unsigned)v < (unsigned)M ? (unsigned short)v : SC_ABSENT;
        }
    }
    sc_wave_sync();
    auto next_live = [&](int t) __attribute__((always_inline)) {  // the first slot >= t that a row of the wave has
        for (; t < K; t++)
            if (__ballot(sN[l31 * K + t] != SC_ABSENT) != 0ull) break;
        return t;
    };

    float4 ra[4], rb[NQB];
    for (int o0 = 0; o0 < cout; o0 += NB * 32) {
        auto fetch = [&](int t, int c0) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; i++) {  // 32 gathered rows x 8 quads
                const int q = lane + 64 * i, row = q >> 3, cq = (q & 7) * 4;
                const unsigned j = sN[row * K + t];
                ra[i] = sc_quad<VEC>(F + (size_t)(j == SC_ABSENT ? 0u : j) * cin + c0 + cq, j == SC_ABSENT ? 0 : cin - c0 - cq);
            }
#pragma unroll
            for (int i = 0; i < NQB; i++) {
                const int q = lane + 64 * i;
                if constexpr (MODE == RF_SC_FORWARD) {  // weight[t][c0 + red][o0 + col]: 32 rows of NB * 8 quads
                    const int red = q / (NB * 8), cq = (q % (NB * 8)) * 4;
                    const bool in = c0 + red < cin;
                    rb[i] = sc_quad<VEC>(W + ((size_t)t * cin + (in ? c0 + red : 0)) * cout + o0 + cq, in ? cout - o0 - cq : 0);
                } else {  // weight[K - 1 - t][o0 + col][c0 + red]: NB * 32 rows of 8 quads
                    const int col = q >> 3, rq = (q & 7) * 4;
                    const bool in = o0 + col < cout;
                    rb[i] = sc_quad<VEC>(W + ((size_t)(K - 1 - t) * cout + (in ? o0 + col : 0)) * cin + c0 + rq, in ? cin - c0 - rq : 0);
                }
            }
        };
        f32x16 acc[NB];
#pragma unroll
        for (int k = 0; k < NB; k++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[k][r] = 0.f;

        int t = next_live(0), c0 = 0;
        if (t < K) fetch(t, 0);
        while (t < K) {
            sc_wave_sync();  // the slab before this one has been consumed
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int q = lane + 64 * i;
                float *d = sA + (q >> 3) * SC_LD + (q & 7) * 4;
                d[0] = ra[i].x, d[1] = ra[i].y, d[2] = ra[i].z, d[3] = ra[i].w;
            }
#pragma unroll
            for (int i = 0; i < NQB; i++) {
                const int q = lane + 64 * i;
                if constexpr (MODE == RF_SC_FORWARD) {
                    float *d = sB + (q / (NB * 8)) * LDB + (q % (NB * 8)) * 4;
                    d[0] = rb[i].x, d[1] = rb[i].y, d[2] = rb[i].z, d[3] = rb[i].w;
                } else {
                    float *d = sB + (q >> 3) * SC_LD + (q & 7) * 4;
                    d[0] = rb[i].x, d[1] = rb[i].y, d[2] = rb[i].z, d[3] = rb[i].w;
                }
            }
            sc_wave_sync();
            // the next slab's loads, to land while this one is multiplied
            int tn = t, cn = c0 + SC_KS;
            if (cn >= cin) cn = 0, tn = next_live(t + 1);
            if (tn < K) fetch(tn, cn);
            const int steps = (min(SC_KS, cin - c0) + 1) >> 1;  // an odd width: one channel of zeros
            const float *pa = sA + l31 * SC_LD + half;
            for (int s = 0; s < steps; s++) {
                const float av = pa[2 * s];
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const float bv = MODE == RF_SC_FORWARD ? sB[(2 * s + half) * LDB + k * 32 + l31] : sB[(k * 32 + l31) * SC_LD + 2 * s + half];
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[k], 0, 0, 0);
                }
            }
            t = tn, c0 = cn;
        }
        // register r of a lane: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile, column lane & 31
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const int col = o0 + k * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gi = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (gi < n && col < cout) O[(size_t)gi * cout + col] = gi < M ? acc[k][r] : 0.f;
            }
        }
    }
}

// ---- the weight gradient ---------------------------------------------------------------------------------------------------
struct SwArgs {
    int b, n, K, cin, cout, CT, OT;
    const float *feat, *gout;
    const int *nbr, *count;
    double *part;  // (b, K, cin, cout)
};

// a wave per (sample, slot, tile of 32 input channels, tile of 32 output channels), the output tile fastest: the waves of
// a workgroup gather the same rows
__global__ __launch_bounds__(SC_TPB) void sparse_conv_wgrad_kernel(SwArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    long w = (long)blockIdx.x * (SC_TPB / 64) + wv;
    if (w >= (long)a.b * a.K * a.CT * a.OT) return;  // (wave-uniform)
    const int n = a.n, K = a.K, cin = a.cin, cout = a.cout;
    const int cot = (int)(w % a.OT);
    w /= a.OT;
    const int cit = (int)(w % a.CT);
    w /= a.CT;
    const int t = (int)(w % K), bi = (int)(w / K);
    const int M = sc_count(a.count, bi, n);
    const int ci = cit * 32 + l31, co = cot * 32 + l31;
    const bool ci_in = ci < cin, co_in = co < cout;
    const float *__restrict__ F = a.feat + (size_t)bi * n * cin + (ci_in ? ci : 0);
    const float *__restrict__ G = a.gout + (size_t)bi * n * cout + (co_in ? co : 0);
    const int *__restrict__ NBR = a.nbr + (size_t)bi * n * K + t;

    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; r++) sum[r] = 0.0;
    for (int ch0 = 0; ch0 < M; ch0 += RF_SC_WGRAD_ROWS) {
        const int end = min(M, ch0 + RF_SC_WGRAD_ROWS);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        for (int g0 = ch0; g0 < end; g0 += 64) {  // 64 rows: lane l holds row g0 + l's entry of the slot
            int j = -1;
            if (g0 + lane < end) {
                j = NBR[(size_t)(g0 + lane) * K];
                if ((unsigned)j >= (unsigned)M) j = -1;
            }
            const unsigned long long live = __ballot(j >= 0);
            // pairs of rows (the instruction's K of 2) of which at least one has the slot, in ascending order, four at a
            // time with their loads in front; an absent row of a pair is zeros on both sides
            unsigned long long pm = (live | live >> 1) & 0x5555555555555555ull;
            while (pm != 0ull) {
                float av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    av[u] = 0.f, bv[u] = 0.f;
                    if (pm != 0ull) {  // (uniform)
                        const int src = __builtin_ctzll(pm) + half;
                        pm &= pm - 1;
                        const int jj = __shfl(j, src, 64);
                        if (jj >= 0) {
                            if (ci_in) av[u] = F[(size_t)jj * cin];
                            if (co_in) bv[u] = G[(size_t)(g0 + src) * cout];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) sum[r] += (double)acc[r];
    }
    double *__restrict__ D = a.part + ((size_t)bi * K + t) * cin * cout;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = cit * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < cin && co_in) D[(size_t)row * cout + co] = sum[r];
    }
}

bool sc_sizes_ok(int b, int n, int K, int cin, int cout) {
    return b <= 65535 && n >= 1 && n <= RF_GC_MAX_POINTS && (K == 27 || K == 125) && cin >= 1 && cin <= RF_SC_MAX_CHANNELS && cout >= 1 &&
           cout <= RF_SC_MAX_CHANNELS;
}

template <int MODE, int NB, bool VEC>
int sc_launch(int b, const ScArgs &a, hipStream_t st) {
    const size_t lds = (size_t)(SC_TPB / 64) * sc_wave_bytes(NB, a.K);
    // (82 KiB at K = 125 with two blocks, above the 64 KiB a kernel gets without asking)
    RF_HIP(hipFuncSetAttribute((const void *)sparse_conv_kernel<MODE, NB, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, 98304));
    RF_LAUNCH("sparse_conv", (sparse_conv_kernel<MODE, NB, VEC>), dim3((unsigned)rf::ceil_div(a.n, SC_ROWS), (unsigned)b), dim3(SC_TPB), lds,
              st, a);
    return RF_OK;
}

}  // namespace

extern "C" {

int rf_sparse_conv_map(int b, int n, int ks, int dilation, const int *coords, const int *count, int *nbr, rf_stream_t stream) {
    if (b < 0 || n < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_GC_MAX_POINTS || b > 65535) return RF_EINVAL;
    if ((ks != 3 && ks != 5) || dilation < 1 || dilation > RF_SC_MAX_DILATION) return RF_EINVAL;
    if (!rf::tensors_ok({coords, nbr}, {count})) return RF_EINVAL;
    int P = 64;
    while (P < n) P <<= 1;
    if (int dv = rf::require_device()) return dv;
    RF_HIP(hipFuncSetAttribute((const void *)sparse_conv_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RF_LAUNCH("sparse_conv_map", sparse_conv_map_kernel, dim3((unsigned)b), dim3(sw_sort_threads(P)),
              (size_t)P * sizeof(unsigned long long), (hipStream_t)stream, n, ks, dilation, coords, count, nbr);
    return RF_OK;
}

int rf_sparse_conv(int b, int n, int K, int cin, int cout, int mode, const float *feat, const float *weight, const int *nbr,
                   const int *count, float *out, rf_stream_t stream) {
    if (b < 0 || n < 0 || cin < 0 || cout < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!sc_sizes_ok(b, n, K, cin, cout)) return RF_EINVAL;
    if (mode != RF_SC_FORWARD && mode != RF_SC_GRAD_INPUT) return RF_EINVAL;
    if (!rf::tensors_ok({feat, weight, nbr, out}, {count})) return RF_EINVAL;
    const bool vec = cin % 4 == 0 && cout % 4 == 0 && rf::all_aligned16({feat, weight});
    const ScArgs a{n, K, cin, cout, feat, weight, nbr, count, out};
    hipStream_t st = (hipStream_t)stream;
    if (int dv = rf::require_device()) return dv;
#define RF_SC_GO(MODE)                                                          \
    do {                                                                        \
        if (cout <= 32) return vec ? sc_launch<MODE, 1, true>(b, a, st) : sc_launch<MODE, 1, false>(b, a, st); \
        return vec ? sc_launch<MODE, 2, true>(b, a, st) : sc_launch<MODE, 2, false>(b, a, st);                 \
    } while (0)
    if (mode == RF_SC_FORWARD) RF_SC_GO(RF_SC_FORWARD);
    RF_SC_GO(RF_SC_GRAD_INPUT);
#undef RF_SC_GO
}

size_t rf_sparse_conv_grad_weight_workspace_bytes(int b, int K, int cin, int cout) {
    if (b < 1 || !sc_sizes_ok(b, 1, K, cin, cout)) return 0;
    rf::Layout w;
    w.add((size_t)b * K * cin * cout * sizeof(double));
    return w.total;
}

int rf_sparse_conv_grad_weight(int b, int n, int K, int cin, int cout, const float *feat, const float *grad_out, const int *nbr,
                               const int *count, float *grad_weight, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || cin < 0 || cout < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!sc_sizes_ok(b, n, K, cin, cout)) return RF_EINVAL;
    if (!rf::tensors_ok({feat, grad_out, nbr, grad_weight}, {count}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (workspace_bytes < rf_sparse_conv_grad_weight_workspace_bytes(b, K, cin, cout)) return RF_EWORKSPACE;
    const int CT = rf::ceil_div(cin, 32), OT = rf::ceil_div(cout, 32);
    const SwArgs a{b, n, K, cin, cout, CT, OT, feat, grad_out, nbr, count, (double *)workspace};
    hipStream_t st = (hipStream_t)stream;
    const long waves = (long)b * K * CT * OT, E = (long)K * cin * cout;
    RF_LAUNCH("sparse_conv_wgrad", sparse_conv_wgrad_kernel, dim3((unsigned)rf::ceil_div(waves, SC_TPB / 64)), dim3(SC_TPB), 0, st, a);
    RF_LAUNCH("sparse_conv_wsum", sparse_conv_wsum_kernel, dim3((unsigned)rf::ceil_div(E, 256)), dim3(256), 0, st, b, E,
              (const double *)workspace, grad_weight);
    return RF_OK;
}

}  // extern "C"
