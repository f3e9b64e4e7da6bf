// grid_pool.hip -- voxel-grid pooling on an unbounded, sparse grid ("one row per occupied cell of edge `cell`") and the point
// order along a space-filling curve, which is the same computation read out differently: a sort of integer cell keys.
// include/rfops.h states the contract; DESIGN.md 5.3s the measurements.
//
//   cluster   one workgroup per sample: the origin (the exact per-axis minimum, when it is not given), a 48-bit key per inside
//             point (row-major, Morton or Hilbert over 3 x 16 bits of cell index) -> 64-bit words (key << 16 | point index) in
//             LDS, the bitonic network of lds_sort.hpp, a head flag per sorted word, a workgroup scan of the flags, and all
//             outputs from LDS: every element once, no memset, no atomics, the counts stay on the device.
//   pool      a lane row per cluster: the cluster's members order[starts[j] .. starts[j + 1]) in ascending point index,
//             channels across the lanes as floats or float4; sum and mean in double rounded once, max with its argument.
//   unpool    a lane row per point: the row of the point's cluster copied, divided by the cluster's size, or masked by the
//             max's argument.  It is the forward of grid_unpool and the backward of all three reductions; the backward of
//             grid_unpool is pool's sum: no float atomics and no memset anywhere.
#include "common.hpp"
#include "lane_rows.hpp"
#include "lds_sort.hpp"

namespace {

constexpr int GC_MAX_TPB = 1024;
constexpr int GC_NW = GC_MAX_TPB / 64;
constexpr unsigned long long GC_PAD = ~0ull;
constexpr int GP_TPB = 256;

// ---- the key ---------------------------------------------------------------------------------------------------------------
// bit j of v -> bit 3 j (v < 2^16)
__device__ __forceinline__ unsigned long long gc_spread(unsigned v) {
    unsigned long long x = v;
    x = (x | x << 16) & 0x0000FF0000FFull;  // (a 24-bit gap pattern suffices: 16 bits in)
    x = (x | x << 8) & 0x00F00F00F00Full;
    x = (x | x << 4) & 0x0C30C30C30C3ull;
    x = (x | x << 2) & 0x249249249249ull;
    return x;
}
__device__ __forceinline__ unsigned long long gc_interleave(unsigned x, unsigned y, unsigned z) {
    return gc_spread(x) << 2 | gc_spread(y) << 1 | gc_spread(z);
}

// Skilling's axes-to-transpose on 16 bits (AIP Conf. Proc. 707, 2004), X[0] = x: the inverse undo from Q = 2^15 down to 2, the
// Gray encode, the t fix-up; the transpose is then interleaved as the Morton key is.
__device__ __forceinline__ unsigned long long gc_hilbert(unsigned x, unsigned y, unsigned z) {
    unsigned X[3] = {x, y, z};
#pragma unroll
    for (unsigned Q = 1u << 15; Q > 1; Q >>= 1) {
        const unsigned P = Q - 1;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (X[i] & Q) {
                X[0] ^= P;
            } else {
                const unsigned t = (X[0] ^ X[i]) & P;
                X[0] ^= t, X[i] ^= t;
            }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    unsigned t = 0;
#pragma unroll
    for (unsigned Q = 1u << 15; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    return gc_interleave(X[0] ^ t, X[1] ^ t, X[2] ^ t);
}

struct GcArgs {
    int n, order;
    float cell;
    const float *xyz, *origin;
    const int *len;
    float *origin_out;
    int *inside, *nclusters, *sorted, *starts, *cluster, *coords;
    long long *code;
};

// the cell of a row: false when the row is not inside (a non-finite coordinate, or a cell index outside 16 bits)
__device__ __forceinline__ bool gc_cell(const float *__restrict__ p, float ox, float oy, float oz, double cell, int &kx, int &ky,
                                        int &kz) {
    const float x = p[0], y = p[1], z = p[2];
    const double tx = floor(((double)x - (double)ox) / cell), ty = floor(((double)y - (double)oy) / cell),
                 tz = floor(((double)z - (double)oz) / cell);
    // (floor keeps the two bounds: t < 32768 iff floor(t) < 32768 and t >= -32768 iff floor(t) >= -32768; NaN fails both)
    const bool in = tx >= -32768.0 && tx < 32768.0 && ty >= -32768.0 && ty < 32768.0 && tz >= -32768.0 && tz < 32768.0 &&
                    isfinite(x) && isfinite(y) && isfinite(z);
    kx = in ? (int)tx : 0, ky = in ? (int)ty : 0, kz = in ? (int)tz : 0;
    return in;
}

// grid (b); dynamic LDS: the P words of the largest sample the launch admits
__global__ __launch_bounds__(GC_MAX_TPB) void grid_cluster_kernel(GcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long gc_words[];  // [P]
    __shared__ float omin[3][GC_NW];
    __shared__ unsigned wtot[2][GC_NW];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int n = a.n;
    const int L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    int P = 64;
    while (P < L) P <<= 1;  // <= 16384: L <= RF_GC_MAX_POINTS

    // 1. the origin
    float ox, oy, oz;
    if (a.origin) {
        ox = a.origin[s * 3], oy = a.origin[s * 3 + 1], oz = a.origin[s * 3 + 2];
    } else {
        const float inf = __builtin_inff();
        float mx = inf, my = inf, mz = inf;
        for (int i = tid; i < L; i += nt) {
            const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
            if (isfinite(x) && isfinite(y) && isfinite(z)) mx = fminf(mx, x), my = fminf(my, y), mz = fminf(mz, z);
        }
        mx = rf::wave_min_f32(mx), my = rf::wave_min_f32(my), mz = rf::wave_min_f32(mz);
        if (lane == 0) omin[0][wave] = mx, omin[1][wave] = my, omin[2][wave] = mz;
        __syncthreads();
        mx = omin[0][0], my = omin[1][0], mz = omin[2][0];
        for (int w = 1; w < nw; w++) mx = fminf(mx, omin[0][w]), my = fminf(my, omin[1][w]), mz = fminf(mz, omin[2][w]);
        // no usable row: +0; -0 becomes +0
        ox = (mx == inf ? 0.f : mx) + 0.0f, oy = (my == inf ? 0.f : my) + 0.0f, oz = (mz == inf ? 0.f : mz) + 0.0f;
    }
    if (tid < 3) a.origin_out[s * 3 + tid] = tid == 0 ? ox : (tid == 1 ? oy : oz);

    // 2. the words; a row that is not inside is finished here
    const double cell = (double)a.cell;
    int *__restrict__ cluster = a.cluster + (size_t)s * n;
    long long *__restrict__ code = a.code ? a.code + (size_t)s * n : nullptr;
    const int top = P > n ? P : n;
    for (int i = tid; i < top; i += nt) {
        unsigned long long w = GC_PAD;
        if (i < L) {
            int kx, ky, kz;
            if (gc_cell(xyz + (size_t)i * 3, ox, oy, oz, cell, kx, ky, kz)) {
                const unsigned ux = (unsigned)(kx + 32768), uy = (unsigned)(ky + 32768), uz = (unsigned)(kz + 32768);
                const unsigned long long key = a.order == RF_GC_XYZ ? ((unsigned long long)ux << 32 | (unsigned long long)uy << 16 | uz)
                                               : a.order == RF_GC_Z ? gc_interleave(ux, uy, uz)
                                                                    : gc_hilbert(ux, uy, uz);
                w = key << 16 | (unsigned)i;
            }
        }
        if (i < P) gc_words[sw_at(i)] = w;
        if (i < n && w == GC_PAD) {
            cluster[i] = -1;
            if (code) code[i] = -1;
        }
    }
    __syncthreads();

    // 3. the network
    sw_sort(gc_words, P, tid, nt);

    // 4-6. heads, their scan and the write-out, nt sorted words per step: a valid word is below every padding word, so the
    // inside points are the first I words.  One scan carries both counts: heads in the low half, valid words in the high half.
    int *__restrict__ sorted = a.sorted + (size_t)s * n;
    int *__restrict__ starts = a.starts + (size_t)s * (n + 1);
    int *__restrict__ coords = a.coords + (size_t)s * n * 3;
    unsigned run = 0;
    for (int r0 = 0, it = 0; r0 < P; r0 += nt, it++) {
        const int r = r0 + tid;  // < P: nt divides P or exceeds it
        const unsigned long long w = r < P ? gc_words[sw_at(r)] : GC_PAD;
        const unsigned long long prev = (r > 0 && r < P) ? gc_words[sw_at(r - 1)] : GC_PAD;
        const bool valid = w != GC_PAD;
        const bool head = valid && (r == 0 || (w >> 16) != (prev >> 16));
        const unsigned incl = rf::wave_incl_scan((head ? 1u : 0u) | (valid ? 0x10000u : 0u));
        if (lane == 63) wtot[it & 1][wave] = incl;
        __syncthreads();
        unsigned base = run;
        for (int q = 0; q < nw; q++) {
            const unsigned t = wtot[it & 1][q];
            base += q < wave ? t : 0u;
            run += t;
        }
        if (valid) {
            const int i = (int)((unsigned)w & 0xFFFFu);           // < L
            const int rank = (int)((base + incl) & 0xFFFFu) - 1;  // heads up to and including r, less one: < n
            sorted[r] = i;
            cluster[i] = rank;
            if (code) code[i] = (long long)(w >> 16);
            if (head) {
                int kx, ky, kz;
                gc_cell(xyz + (size_t)i * 3, ox, oy, oz, cell, kx, ky, kz);
                starts[rank] = r;
                coords[rank * 3] = kx, coords[rank * 3 + 1] = ky, coords[rank * 3 + 2] = kz;
            }
        }
    }
    const int M = (int)(run & 0xFFFFu), I = (int)(run >> 16);
    for (int r = I + tid; r < n; r += nt) sorted[r] = 0;
    for (int j = M + tid; j <= n; j += nt) {
        starts[j] = I;
        if (j < n) coords[j * 3] = 0, coords[j * 3 + 1] = 0, coords[j * 3 + 2] = 0;
    }
    if (tid == 0) a.inside[s] = I, a.nclusters[s] = M;
}

// ---- pool ------------------------------------------------------------------------------------------------------------------
struct GpArgs {
    int n, c, tx_log2, bpb;
    const float *feat;
    const int *sorted, *starts, *nclusters;
    float *out;
    int *arg;
};

// What the caller hands over is read defensively: the cluster count is clamped into [0, n], a list's bounds into [0, n], and a
// member outside [0, n) is skipped -- whatever the arrays hold, nothing outside the tensors is touched.
template <int VEC, int REDUCE>
__global__ __launch_bounds__(GP_TPB) void grid_pool_kernel(GpArgs a) {
    typedef typename rf::LaneVec<VEC>::T V;
    typedef int IV __attribute__((ext_vector_type(VEC)));
    int bi, bx;
    rf::place_1d(a.bpb, bi, bx);
    const rf::LaneRows<GP_TPB> g(a.tx_log2);
    const int n = a.n, cv = a.c / VEC;
    const int j = bx * g.TY + g.ly;
    if (j >= n) return;
    const int M = min(max(a.nclusters[bi], 0), n);
    const int *__restrict__ ST = a.starts + (size_t)bi * (n + 1);
    const int *__restrict__ O = a.sorted + (size_t)bi * n;
    const V *__restrict__ F = (const V *)(a.feat + (size_t)bi * n * a.c);
    int beg = 0, end = 0;
    if (j < M) {
        beg = min(max(ST[j], 0), n);
        end = min(max(ST[j + 1], beg), n);
    }
    for (int l = g.lx; l < cv; l += g.TX) {
        V out;
        if constexpr (REDUCE == RF_GP_MAX) {
            IV win;
            bool first[VEC], done[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) first[k] = true, done[k] = false, rf::lane_set(out, k, 0.f), win[k] = 0;
            int i = beg < end ? O[beg] : -1;
            for (int p = beg; p < end; p++) {
                const int nxt = p + 1 < end ? O[p + 1] : -1;
                if ((unsigned)i < (unsigned)n) {
                    const V v = F[(size_t)i * cv + l];
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float x = rf::lane_at(v, k);
                        // the first member; a later one when it is strictly greater; a NaN member is taken and ends the walk
                        const bool take = !done[k] && (first[k] || x != x || x > rf::lane_at(out, k));
                        if (take) rf::lane_set(out, k, x), win[k] = i;
                        done[k] = done[k] || (take && x != x);
                        first[k] = false;
                    }
                }
                i = nxt;
            }
            IV *__restrict__ A = (IV *)(a.arg + (size_t)bi * n * a.c);
            A[(size_t)j * cv + l] = win;
        } else {
            double acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) acc[k] = 0.0;
            int i = beg < end ? O[beg] : -1;
            for (int p = beg; p < end; p++) {
                const int nxt = p + 1 < end ? O[p + 1] : -1;
                if ((unsigned)i < (unsigned)n) {
                    const V v = F[(size_t)i * cv + l];
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc[k] += (double)rf::lane_at(v, k);
                }
                i = nxt;
            }
            const double cnt = (double)(end - beg);
#pragma unroll
            for (int k = 0; k < VEC; k++)
                rf::lane_set(out, k, end == beg ? 0.f : (REDUCE == RF_GP_MEAN ? (float)(acc[k] / cnt) : (float)acc[k]));
        }
        V *__restrict__ D = (V *)(a.out + (size_t)bi * n * a.c);
        D[(size_t)j * cv + l] = out;
    }
}

// ---- unpool ----------------------------------------------------------------------------------------------------------------
struct GuArgs {
    int n, c, tx_log2, bpb;
    const float *src;
    const int *cluster, *starts, *arg;
    float *dst;
};

template <int VEC, int MODE>
__global__ __launch_bounds__(GP_TPB) void grid_unpool_kernel(GuArgs a) {
    typedef typename rf::LaneVec<VEC>::T V;
    typedef int IV __attribute__((ext_vector_type(VEC)));
    int bi, bx;
    rf::place_1d(a.bpb, bi, bx);
    const rf::LaneRows<GP_TPB> g(a.tx_log2);
    const int n = a.n, cv = a.c / VEC;
    const int i = bx * g.TY + g.ly;
    if (i >= n) return;
    const int cl = a.cluster[(size_t)bi * n + i];
    const bool live = (unsigned)cl < (unsigned)n;  // -1: a row that is not inside (anything else outside [0, n) alike)
    const int jc = live ? cl : 0;
    const V *__restrict__ S = (const V *)(a.src + (size_t)bi * n * a.c) + (size_t)jc * cv;
    V *__restrict__ D = (V *)(a.dst + (size_t)bi * n * a.c) + (size_t)i * cv;
    double cnt = 1.0;
    bool some = live;
    if constexpr (MODE == RF_GU_MEAN) {
        const int *__restrict__ ST = a.starts + (size_t)bi * (n + 1);
        const int k = ST[jc + 1] - ST[jc];
        some = live && k > 0;
        cnt = (double)k;
    }
    for (int l = g.lx; l < cv; l += g.TX) {
        V out;
#pragma unroll
        for (int k = 0; k < VEC; k++) rf::lane_set(out, k, 0.f);
        if (some) {
            const V v = S[l];
            if constexpr (MODE == RF_GU_COPY) {
                out = v;
            } else if constexpr (MODE == RF_GU_MEAN) {
#pragma unroll
                for (int k = 0; k < VEC; k++) rf::lane_set(out, k, (float)((double)rf::lane_at(v, k) / cnt));
            } else {
                const IV w = ((const IV *)(a.arg + (size_t)bi * n * a.c) + (size_t)jc * cv)[l];
#pragma unroll
                for (int k = 0; k < VEC; k++) rf::lane_set(out, k, w[k] == i ? rf::lane_at(v, k) : 0.f);
            }
        }
        D[l] = out;
    }
}

bool gp_sizes_ok(int b, int n, int c) { return b <= 65535 && n >= 1 && n <= RF_GC_MAX_POINTS && c >= 1 && c <= RF_GP_MAX_CHANNELS; }

}  // namespace

extern "C" {

int rf_grid_cluster(int b, int n, float cell, int order, const float *xyz, const int *len, const float *origin, float *origin_out,
                    int *inside, int *nclusters, int *sorted, int *starts, int *cluster, int *coords, long long *code,
                    rf_stream_t stream) {
    if (b < 0 || n < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_GC_MAX_POINTS || b > 65535) return RF_EINVAL;
    if (!(cell > 0.f) || !isfinite(cell)) return RF_EINVAL;
    if (order != RF_GC_XYZ && order != RF_GC_Z && order != RF_GC_HILBERT) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, origin_out, inside, nclusters, sorted, starts, cluster, coords}, {len, origin}) || !rf::aligned8(code))
        return RF_EINVAL;
    int P = 64;
    while (P < n) P <<= 1;
    const GcArgs a{n, order, cell, xyz, origin, len, origin_out, inside, nclusters, sorted, starts, cluster, coords, code};
    if (int dv = rf::require_device()) return dv;
    // (128 KiB of words at 16384 points, above the 64 KiB a kernel gets without asking; with the scan's few hundred bytes of
    // static LDS below the 160 KiB a workgroup may take)
    RF_HIP(hipFuncSetAttribute((const void *)grid_cluster_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RF_LAUNCH("grid_cluster", grid_cluster_kernel, dim3((unsigned)b), dim3(sw_sort_threads(P)),
              (size_t)P * sizeof(unsigned long long), (hipStream_t)stream, a);
    return RF_OK;
}

int rf_grid_pool(int b, int n, int c, int reduce, const float *feat, const int *sorted, const int *starts, const int *nclusters,
                 float *out, int *arg, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gp_sizes_ok(b, n, c)) return RF_EINVAL;
    if (reduce != RF_GP_SUM && reduce != RF_GP_MEAN && reduce != RF_GP_MAX) return RF_EINVAL;
    if (!rf::tensors_ok({feat, sorted, starts, nclusters, out}, {arg})) return RF_EINVAL;
    if ((reduce == RF_GP_MAX) != (arg != nullptr)) return RF_EINVAL;
    const bool vec = rf::lane_rows_vec_ok(c, {feat, out, arg});
    const int tx_log2 = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const int bpb = rf::ceil_div(n, GP_TPB >> tx_log2);
    const GpArgs a{n, c, tx_log2, bpb, feat, sorted, starts, nclusters, out, arg};
    const dim3 grid((unsigned)((long)bpb * b));
    hipStream_t st = (hipStream_t)stream;
#define RF_GP_GO(VEC, R) RF_LAUNCH("grid_pool", (grid_pool_kernel<VEC, R>), grid, dim3(GP_TPB), 0, st, a)
    if (reduce == RF_GP_SUM) {
        if (vec) { RF_GP_GO(4, RF_GP_SUM); } else { RF_GP_GO(1, RF_GP_SUM); }
    } else if (reduce == RF_GP_MEAN) {
        if (vec) { RF_GP_GO(4, RF_GP_MEAN); } else { RF_GP_GO(1, RF_GP_MEAN); }
    } else {
        if (vec) { RF_GP_GO(4, RF_GP_MAX); } else { RF_GP_GO(1, RF_GP_MAX); }
    }
#undef RF_GP_GO
    return RF_OK;
}

int rf_grid_unpool(int b, int n, int c, int mode, const float *src, const int *cluster, const int *starts, const int *arg,
                   float *dst, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gp_sizes_ok(b, n, c)) return RF_EINVAL;
    if (mode != RF_GU_COPY && mode != RF_GU_MEAN && mode != RF_GU_MAX) return RF_EINVAL;
    if (!rf::tensors_ok({src, cluster, dst}, {starts, arg})) return RF_EINVAL;
    if ((mode == RF_GU_MEAN && !starts) || (mode == RF_GU_MAX && !arg)) return RF_EINVAL;
    const bool vec = rf::lane_rows_vec_ok(c, {src, dst, mode == RF_GU_MAX ? arg : nullptr});
    const int tx_log2 = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const int bpb = rf::ceil_div(n, GP_TPB >> tx_log2);
    const GuArgs a{n, c, tx_log2, bpb, src, cluster, starts, arg, dst};
    const dim3 grid((unsigned)((long)bpb * b));
    hipStream_t st = (hipStream_t)stream;
#define RF_GU_GO(VEC, R) RF_LAUNCH("grid_unpool", (grid_unpool_kernel<VEC, R>), grid, dim3(GP_TPB), 0, st, a)
    if (mode == RF_GU_COPY) {
        if (vec) { RF_GU_GO(4, RF_GU_COPY); } else { RF_GU_GO(1, RF_GU_COPY); }
    } else if (mode == RF_GU_MEAN) {
        if (vec) { RF_GU_GO(4, RF_GU_MEAN); } else { RF_GU_GO(1, RF_GU_MEAN); }
    } else {
        if (vec) { RF_GU_GO(4, RF_GU_MAX); } else { RF_GU_GO(1, RF_GU_MAX); }
    }
#undef RF_GU_GO
    return RF_OK;
}

}  // extern "C"
