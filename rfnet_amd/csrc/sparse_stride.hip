// sparse_stride.hip -- the change of level on the sparse voxel grid: the 2 x 2 x 2 stride-2 convolution and its transpose onto
// the finer level's cells (rf_sparse_stride_map, rf_sparse_conv_strided, rf_sparse_conv_strided_grad_weight).  The submanifold
// layers of a level are sparse_conv.hip's; include/rfops.h states the contract; DESIGN.md 5.3u the measurements.
//
//   map      one workgroup per sample, as sparse_conv_map_kernel and grid_cluster: 64-bit words ((45-bit row-major key of the
//            COARSE cell << 3 | slot) << 16 | row) in LDS, the bitonic network of lds_sort.hpp; a word whose predecessor has the
//            same 48 bits is a duplicate, a word whose predecessor has another coarse key is a head, and grid_cluster's workgroup
//            scan of the heads is the coarse cell's rank.  A word writes its own entry of child and of up and the -1 of the slots
//            between its predecessor's and its own; the last word of a cell writes the slots behind it.
//   conv     sparse_conv_kernel's wave: 32 COARSE rows, their tile of child in LDS as 16-bit fine rows, v_mfma_f32_32x32x2_f32
//            as the fmaf chain, slabs of 32 channels through registers one ahead, no workgroup barrier.  The gather form (down,
//            and the gradient of up to its features) carries the accumulators over the eight slots and stores coarse rows.
//            The fan-out form (up, and the gradient of down to its features) has the coarse rows themselves as A, runs a
//            chain per slot some row of the tile has and stores accumulator row r to the fine row child[j][t] -- which `up`
//            has confirmed, so a fine row has one writer; the four waves of a workgroup share 32 coarse rows and take two
//            slots each; further workgroups of the same launch walk `up` and store +0 to the fine rows nobody serves.
//   wgrad    sparse_conv_wgrad_kernel over the coarse rows, the gather on the operand of the fine level.
#include "lds_sort.hpp"
#include "sparse_conv.hpp"

namespace {

constexpr int SS_NW = 1024 / 64;

// ---- the level map ---------------------------------------------------------------------------------------------------------
// grid (b); dynamic LDS: the P words of the largest sample the launch admits
__global__ __launch_bounds__(1024) void sparse_stride_map_kernel(int n, int nc, const int *__restrict__ coords, const int *__restrict__ count,
                                                                 int *__restrict__ coords_out, int *__restrict__ count_out,
                                                                 int *__restrict__ total_out, int *__restrict__ child, int *__restrict__ up) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ss_words[];  // [P]
    __shared__ unsigned wtot[2][SS_NW];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int M = sc_count(count, s, n);
    const int *__restrict__ C = coords + (size_t)s * n * 3;
    int *__restrict__ CO = coords_out + (size_t)s * nc * 3;
    int *__restrict__ CH = child + (size_t)s * nc * 8;
    int *__restrict__ UP = up + (size_t)s * n;
    int P = 64;
    while (P < M) P <<= 1;

    // 1. the words; a row behind M or out of range is finished here (rows behind M are not read)
    const int top = P > n ? P : n;
    for (int i = tid; i < top; i += nt) {
        unsigned long long w = SC_PAD;
        if (i < M) {
            const int x = C[i * 3], y = C[i * 3 + 1], z = C[i * 3 + 2];
            if (sc_in_range(x, y, z)) {
                // (x + 32768) >> 1 = (x >> 1) + 16384: the shift of the biased index is the floor; its low bit is x & 1
                const unsigned ux = (unsigned)(x + 32768), uy = (unsigned)(y + 32768), uz = (unsigned)(z + 32768);
                const unsigned long long ckey = (unsigned long long)(ux >> 1) << 30 | (unsigned long long)(uy >> 1) << 15 | (uz >> 1);
                const unsigned t = (ux & 1u) << 2 | (uy & 1u) << 1 | (uz & 1u);
                w = (ckey << 3 | t) << 16 | (unsigned)i;
            }
        }
        if (i < P) ss_words[sw_at(i)] = w;
        if (i < n && w == SC_PAD) UP[i] = -1;
    }
    __syncthreads();

    // 2. the network: ascending (coarse key, slot, row), so the first word of a fine cell is its lowest row, the live one
    sw_sort(ss_words, P, tid, nt);

    // 3. heads, their scan and the write-out, nt sorted words per step (a valid word is below every padding word)
    unsigned run = 0;
    for (int r0 = 0, it = 0; r0 < P; r0 += nt, it++) {
        const int r = r0 + tid;  // < P: nt divides P or exceeds it
        const unsigned long long w = r < P ? ss_words[sw_at(r)] : SC_PAD;
        const unsigned long long prev = (r > 0 && r < P) ? ss_words[sw_at(r - 1)] : SC_PAD;
        const unsigned long long next = r + 1 < P ? ss_words[sw_at(r + 1)] : SC_PAD;
        const bool valid = w != SC_PAD;
        const bool first = r == 0 || (prev >> 19) != (w >> 19);  // of its coarse cell
        const bool head = valid && first;
        const unsigned incl = rf::wave_incl_scan(head ? 1u : 0u);
        if (lane == 63) wtot[it & 1][wave] = incl;
        __syncthreads();
        unsigned base = run;
        for (int q = 0; q < nw; q++) {
            const unsigned t = wtot[it & 1][q];
            base += q < wave ? t : 0u;
            run += t;
        }
        if (valid) {
            const int i = (int)((unsigned)w & 0xFFFFu);  // < M
            const int t = (int)((unsigned)(w >> 16) & 7u);
            const int j = (int)(base + incl) - 1;  // heads up to and including r, less one
            const bool dup = !first && (prev >> 16) == (w >> 16);
            const bool kept = j < nc;
            UP[i] = (!dup && kept) ? 8 * j + t : -1;
            if (kept) {
                if (!dup) {
                    CH[j * 8 + t] = i;
                    // (a predecessor in the cell has a lower slot: the 48 bits differ and the words ascend)
                    for (int e = first ? 0 : (int)((unsigned)(prev >> 16) & 7u) + 1; e < t; e++) CH[j * 8 + e] = -1;
                }
                if (next == SC_PAD || (next >> 19) != (w >> 19))  // the last word of the cell
                    for (int e = t + 1; e < 8; e++) CH[j * 8 + e] = -1;
                if (head) {
                    const unsigned long long ckey = w >> 19;
                    CO[j * 3] = (int)((unsigned)(ckey >> 30) & 0x7FFFu) - 16384;
                    CO[j * 3 + 1] = (int)((unsigned)(ckey >> 15) & 0x7FFFu) - 16384;
                    CO[j * 3 + 2] = (int)((unsigned)ckey & 0x7FFFu) - 16384;
                }
            }
        }
    }
    const int D = (int)run, Dk = D < nc ? D : nc;
    for (int e = Dk * 8 + tid; e < nc * 8; e += nt) CH[e] = -1;
    for (int e = Dk * 3 + tid; e < nc * 3; e += nt) CO[e] = 0;
    if (tid == 0) total_out[s] = D, count_out[s] = Dk;
}

// ---- the four convolutions ---------------------------------------------------------------------------------------------------
struct SsArgs {
    int n, nc, cin, cout, tiles;  // cin: the reduction (src's channels), cout: out's channels; tiles: workgroups of coarse rows
    const float *src, *weight;
    const int *child, *up, *count, *count_coarse;
    float *out;
};

// grid (ceil(n_coarse / 128), b), for FAN (ceil(n_coarse / 32) + ceil(n / 128), b); dynamic LDS: 4 * sc_wave_bytes(NB, 8).
// FAN: out has the fine rows; TRANS: weight[t][o][ch] stands for weight[t][ch][o]
template <bool FAN, bool TRANS, int NB, bool VEC>
__global__ __launch_bounds__(SC_TPB) void sparse_stride_kernel(SsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_lds[];
    constexpr int K = 8;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bi = blockIdx.y;
    const int n = a.n, nc = a.nc, cin = a.cin, cout = a.cout;
    const int M = sc_count(a.count, bi, n), Mc = sc_count(a.count_coarse, bi, nc);
    const int *__restrict__ CH = a.child + (size_t)bi * nc * K;
    float *__restrict__ O = a.out + (size_t)bi * (FAN ? n : nc) * cout;

    if constexpr (FAN) {
        if ((int)blockIdx.x >= a.tiles) {  // +0 to the fine rows nobody serves: 32 rows of `up` per wave
            const int i0 = ((int)blockIdx.x - a.tiles) * SC_ROWS + wv * 32, i = i0 + l31;
            if (i0 >= n) return;  // (wave-uniform)
            bool zero = false;
            if (half == 0 && i < n) {
                bool served = false;
                if (i < M) {
                    const int u = a.up[(size_t)bi * n + i];
                    served = u >= 0 && (u >> 3) < Mc && CH[u] == i;  // (u < 8 Mc <= 8 nc: inside child)
                }
                zero = !served;
            }
            unsigned long long todo = __ballot(zero);
            while (todo != 0ull) {
                const int r = __builtin_ctzll(todo);
                todo &= todo - 1;
                for (int e = lane; e < cout; e += 64) O[(size_t)(i0 + r) * cout + e] = 0.f;
            }
            return;
        }
    }
    // gather: a wave per 32 coarse rows, all eight slots; fan-out: a workgroup per 32 coarse rows, two slots per wave -- a chain
    // there is one slot long, and four times the waves is what fills the chip at a few hundred coarse rows per sample
    const int j0 = FAN ? blockIdx.x * 32 : blockIdx.x * SC_ROWS + wv * 32;
    const int t_lo = FAN ? 2 * wv : 0, t_hi = FAN ? 2 * wv + 2 : K;
    if (j0 >= nc) return;  // (wave-uniform)
    if (j0 >= Mc) {        // coarse rows behind the count only
        if constexpr (!FAN) {
            const int rows = min(32, nc - j0);
            for (int e = lane; e < rows * cout; e += 64) O[(size_t)j0 * cout + e] = 0.f;
        }
        return;
    }
    constexpr int LDB = NB == 1 ? 32 : 96;
    constexpr int NQB = NB * 4;  // quads of a weight slab per lane
    float *sA = (float *)(ss_lds + (size_t)wv * sc_wave_bytes(NB, K));
    float *sB = sA + 32 * SC_LD;
    unsigned short *sN = (unsigned short *)(sB + sc_b_floats(NB));
    const float *__restrict__ F = a.src + (size_t)bi * (FAN ? nc : n) * cin;
    const float *__restrict__ W = a.weight;

    // the wave's tile of child, [coarse row][slot] (FAN: its two slots of it): a fine row in [0, M) -- for FAN one whose `up`
    // names this entry -- or ABSENT (coarse rows behind Mc are not read)
    {
        const int *__restrict__ CT = CH + (size_t)j0 * K;
        const int have = min(32, Mc - j0) * K;
        for (int e = lane; e < 32 * (t_hi - t_lo); e += 64) {
            const int q = FAN ? (e >> 1) * K + t_lo + (e & 1) : e;
            int v = q < have ? CT[q] : -1;
            if ((unsigned)v >= (unsigned)M) v = -1;
            if constexpr (FAN) {
                if (v >= 0 && a.up[(size_t)bi * n + v] != j0 * K + q) v = -1;
            }
            sN[q] = v >= 0 ? (unsigned short)v : SC_ABSENT;
        }
    }
    sc_wave_sync();
    auto next_live = [&](int t) __attribute__((always_inline)) {  // the first slot >= t that a row of the wave has, or t_hi
        for (; t < t_hi; t++)
            if (__ballot(sN[l31 * K + t] != SC_ABSENT) != 0ull) break;
        return t;
    };

    float4 ra[4], rb[NQB];
    for (int o0 = 0; o0 < cout; o0 += NB * 32) {
        auto fetch = [&](int t, int c0) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; i++) {  // 32 source rows x 8 quads
                const int q = lane + 64 * i, row = q >> 3, cq = (q & 7) * 4;
                const unsigned j = sN[row * K + t];
                const unsigned from = FAN ? (unsigned)(j0 + row) : j;  // (FAN: j0 + row < Mc wherever the slot is there)
                ra[i] = sc_quad<VEC>(F + (size_t)(j == SC_ABSENT ? 0u : from) * cin + c0 + cq, j == SC_ABSENT ? 0 : cin - c0 - cq);
            }
#pragma unroll
            for (int i = 0; i < NQB; i++) {
                const int q = lane + 64 * i;
                if constexpr (!TRANS) {  // weight[t][c0 + red][o0 + col]: 32 rows of NB * 8 quads
                    const int red = q / (NB * 8), cq = (q % (NB * 8)) * 4;
                    const bool in = c0 + red < cin;
                    rb[i] = sc_quad<VEC>(W + ((size_t)t * cin + (in ? c0 + red : 0)) * cout + o0 + cq, in ? cout - o0 - cq : 0);
                } else {  // weight[t][o0 + col][c0 + red]: NB * 32 rows of 8 quads
                    const int col = q >> 3, rq = (q & 7) * 4;
                    const bool in = o0 + col < cout;
                    rb[i] = sc_quad<VEC>(W + ((size_t)t * cout + (in ? o0 + col : 0)) * cin + c0 + rq, in ? cin - c0 - rq : 0);
                }
            }
        };
        f32x16 acc[NB];
#pragma unroll
        for (int k = 0; k < NB; k++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[k][r] = 0.f;

        int t = next_live(t_lo), c0 = 0;
        if (t < t_hi) fetch(t, 0);
        while (t < t_hi) {
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
                if constexpr (!TRANS) {
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
            if (tn < t_hi) fetch(tn, cn);
            const int steps = (min(SC_KS, cin - c0) + 1) >> 1;  // an odd width: one channel of zeros
            const float *pa = sA + l31 * SC_LD + half;
            for (int s = 0; s < steps; s++) {
                const float av = pa[2 * s];
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const float bv = !TRANS ? sB[(2 * s + half) * LDB + k * 32 + l31] : sB[(k * 32 + l31) * SC_LD + 2 * s + half];
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[k], 0, 0, 0);
                }
            }
            // register r of a lane: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile, column lane & 31
            if constexpr (FAN) {
                if (tn != t) {  // the slot's chain ends here: its rows go to the fine rows, and the next slot starts from +0
#pragma unroll
                    for (int k = 0; k < NB; k++) {
                        const int col = o0 + k * 32 + l31;
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const unsigned i = sN[((r & 3) + 8 * (r >> 2) + 4 * half) * K + t];  // in [0, M), named by no other entry
                            if (i != SC_ABSENT && col < cout) O[(size_t)i * cout + col] = acc[k][r];
                            acc[k][r] = 0.f;
                        }
                    }
                }
            }
            t = tn, c0 = cn;
        }
        if constexpr (!FAN) {
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const int col = o0 + k * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int gj = j0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (gj < nc && col < cout) O[(size_t)gj * cout + col] = gj < Mc ? acc[k][r] : 0.f;
                }
            }
        }
    }
}

// ---- the weight gradient ---------------------------------------------------------------------------------------------------
struct SgArgs {
    int b, n, nc, cin, cout, CT, OT;
    const float *fine, *coarse;
    const int *child, *count, *count_coarse;
    double *part;  // (b, 8, cin, cout)
};

// a wave per (sample, slot, tile of 32 input channels, tile of 32 output channels), the output tile fastest.  UP: the input
// channels are the coarse rows', the output channels the fine rows'; otherwise the other way round.
template <bool UP>
__global__ __launch_bounds__(SC_TPB) void sparse_stride_wgrad_kernel(SgArgs a) {
    constexpr int K = 8;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    long w = (long)blockIdx.x * (SC_TPB / 64) + wv;
    if (w >= (long)a.b * K * a.CT * a.OT) return;  // (wave-uniform)
    const int n = a.n, nc = a.nc, cin = a.cin, cout = a.cout;
    const int cot = (int)(w % a.OT);
    w /= a.OT;
    const int cit = (int)(w % a.CT);
    w /= a.CT;
    const int t = (int)(w % K), bi = (int)(w / K);
    const int M = sc_count(a.count, bi, n), Mc = sc_count(a.count_coarse, bi, nc);
    const int ci = cit * 32 + l31, co = cot * 32 + l31;
    const bool ci_in = ci < cin, co_in = co < cout;
    // A: the operand with the input channels, B: the one with the output channels
    const float *__restrict__ PA = (UP ? a.coarse + (size_t)bi * nc * cin : a.fine + (size_t)bi * n * cin) + (ci_in ? ci : 0);
    const float *__restrict__ PB = (UP ? a.fine + (size_t)bi * n * cout : a.coarse + (size_t)bi * nc * cout) + (co_in ? co : 0);
    const int *__restrict__ CH = a.child + (size_t)bi * nc * K + t;

    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; r++) sum[r] = 0.0;
    for (int ch0 = 0; ch0 < Mc; ch0 += RF_SC_WGRAD_ROWS) {
        const int end = min(Mc, ch0 + RF_SC_WGRAD_ROWS);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        for (int g0 = ch0; g0 < end; g0 += 64) {  // 64 coarse rows: lane l holds row g0 + l's child in the slot
            int i = -1;
            if (g0 + lane < end) {
                i = CH[(size_t)(g0 + lane) * K];
                if ((unsigned)i >= (unsigned)M) i = -1;
            }
            const unsigned long long live = __ballot(i >= 0);
            // pairs of coarse rows (the instruction's K of 2) of which at least one has the slot, in ascending order, four at
            // a time with their loads in front; an absent row of a pair is zeros on both sides
            unsigned long long pm = (live | live >> 1) & 0x5555555555555555ull;
            while (pm != 0ull) {
                float av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    av[u] = 0.f, bv[u] = 0.f;
                    if (pm != 0ull) {  // (uniform)
                        const int src = __builtin_ctzll(pm) + half;
                        pm &= pm - 1;
                        const int ii = __shfl(i, src, 64);
                        if (ii >= 0) {
                            const int ra = UP ? g0 + src : ii, rb = UP ? ii : g0 + src;
                            if (ci_in) av[u] = PA[(size_t)ra * cin];
                            if (co_in) bv[u] = PB[(size_t)rb * cout];
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

bool ss_sizes_ok(int b, int n, int nc, int cin, int cout) {
    return b <= 65535 && n >= 1 && n <= RF_GC_MAX_POINTS && nc >= 1 && nc <= n && cin >= 1 && cin <= RF_SC_MAX_CHANNELS && cout >= 1 &&
           cout <= RF_SC_MAX_CHANNELS;
}

template <bool FAN, bool TRANS, int NB, bool VEC>
int ss_launch(int b, const SsArgs &a, hipStream_t st) {
    const size_t lds = (size_t)(SC_TPB / 64) * sc_wave_bytes(NB, 8);
    // (66.5 KiB with two blocks, above the 64 KiB a kernel gets without asking)
    RF_HIP(hipFuncSetAttribute((const void *)sparse_stride_kernel<FAN, TRANS, NB, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, 98304));
    const unsigned gx = (unsigned)(a.tiles + (FAN ? rf::ceil_div(a.n, SC_ROWS) : 0));
    RF_LAUNCH("sparse_conv_strided", (sparse_stride_kernel<FAN, TRANS, NB, VEC>), dim3(gx, (unsigned)b), dim3(SC_TPB), lds, st, a);
    return RF_OK;
}

template <bool FAN, bool TRANS>
int ss_go(int b, const SsArgs &a, bool vec, hipStream_t st) {
    if (a.cout <= 32) return vec ? ss_launch<FAN, TRANS, 1, true>(b, a, st) : ss_launch<FAN, TRANS, 1, false>(b, a, st);
    return vec ? ss_launch<FAN, TRANS, 2, true>(b, a, st) : ss_launch<FAN, TRANS, 2, false>(b, a, st);
}

}  // namespace

extern "C" {

int rf_sparse_stride_map(int b, int n, int n_coarse, const int *coords, const int *count, int *coords_out, int *count_out,
                         int *total_out, int *child, int *up, rf_stream_t stream) {
    if (b < 0 || n < 0 || n_coarse < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_GC_MAX_POINTS || n_coarse < 1 || n_coarse > n || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({coords, coords_out, count_out, total_out, child, up}, {count})) return RF_EINVAL;
    int P = 64;
    while (P < n) P <<= 1;
    if (int dv = rf::require_device()) return dv;
    RF_HIP(hipFuncSetAttribute((const void *)sparse_stride_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RF_LAUNCH("sparse_stride_map", sparse_stride_map_kernel, dim3((unsigned)b), dim3(sw_sort_threads(P)),
              (size_t)P * sizeof(unsigned long long), (hipStream_t)stream, n, n_coarse, coords, count, coords_out, count_out, total_out,
              child, up);
    return RF_OK;
}

int rf_sparse_conv_strided(int b, int n, int n_coarse, int cin, int cout, int mode, const float *src, const float *weight,
                           const int *child, const int *up, const int *count, const int *count_coarse, float *out, rf_stream_t stream) {
    if (b < 0 || n < 0 || n_coarse < 0 || cin < 0 || cout < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!ss_sizes_ok(b, n, n_coarse, cin, cout)) return RF_EINVAL;
    if (mode != RF_SS_DOWN && mode != RF_SS_UP && mode != RF_SS_DOWN_GRAD_INPUT && mode != RF_SS_UP_GRAD_INPUT) return RF_EINVAL;
    if (!rf::tensors_ok({src, weight, child, up, out}, {count, count_coarse})) return RF_EINVAL;
    const bool vec = cin % 4 == 0 && cout % 4 == 0 && rf::all_aligned16({src, weight});
    const bool fan = mode == RF_SS_UP || mode == RF_SS_DOWN_GRAD_INPUT;
    const SsArgs a{n, n_coarse, cin, cout, rf::ceil_div(n_coarse, fan ? 32 : SC_ROWS), src, weight, child, up, count, count_coarse, out};
    hipStream_t st = (hipStream_t)stream;
    if (int dv = rf::require_device()) return dv;
    if (mode == RF_SS_DOWN) return ss_go<false, false>(b, a, vec, st);
    if (mode == RF_SS_UP) return ss_go<true, false>(b, a, vec, st);
    if (mode == RF_SS_DOWN_GRAD_INPUT) return ss_go<true, true>(b, a, vec, st);
    return ss_go<false, true>(b, a, vec, st);
}

size_t rf_sparse_conv_strided_grad_weight_workspace_bytes(int b, int cin, int cout) {
    if (b < 1 || !ss_sizes_ok(b, 1, 1, cin, cout)) return 0;
    rf::Layout w;
    w.add((size_t)b * 8 * cin * cout * sizeof(double));
    return w.total;
}

int rf_sparse_conv_strided_grad_weight(int b, int n, int n_coarse, int cin, int cout, int mode, const float *fine, const float *coarse,
                                       const int *child, const int *count, const int *count_coarse, float *grad_weight,
                                       void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || n_coarse < 0 || cin < 0 || cout < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!ss_sizes_ok(b, n, n_coarse, cin, cout)) return RF_EINVAL;
    if (mode != RF_SS_DOWN && mode != RF_SS_UP) return RF_EINVAL;
    if (!rf::tensors_ok({fine, coarse, child, grad_weight}, {count, count_coarse}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (workspace_bytes < rf_sparse_conv_strided_grad_weight_workspace_bytes(b, cin, cout)) return RF_EWORKSPACE;
    const int CT = rf::ceil_div(cin, 32), OT = rf::ceil_div(cout, 32);
    const SgArgs a{b, n, n_coarse, cin, cout, CT, OT, fine, coarse, child, count, count_coarse, (double *)workspace};
    hipStream_t st = (hipStream_t)stream;
    const long waves = (long)b * 8 * CT * OT, E = (long)8 * cin * cout;
    const dim3 grid((unsigned)rf::ceil_div(waves, SC_TPB / 64));
    if (mode == RF_SS_UP) {
        RF_LAUNCH("sparse_conv_strided_wgrad", sparse_stride_wgrad_kernel<true>, grid, dim3(SC_TPB), 0, st, a);
    } else {
        RF_LAUNCH("sparse_conv_strided_wgrad", sparse_stride_wgrad_kernel<false>, grid, dim3(SC_TPB), 0, st, a);
    }
    RF_LAUNCH("sparse_conv_wsum", sparse_conv_wsum_kernel, dim3((unsigned)rf::ceil_div(E, 256)), dim3(256), 0, st, b, E,
              (const double *)workspace, grad_weight);
    return RF_OK;
}

}  // extern "C"
