// msn_ops.hip -- the two ops of MSN-style completion networks that the library lacked, for gfx950: the expansion penalty
// (per surface patch: the minimum spanning tree, its edges longer than alpha times the patch's mean edge penalised) with
// its gradient, and minimum density sampling (MDS: thin a cloud to m points, each step taking the point whose Gaussian
// density under the points chosen so far is smallest).  include/rfops.h states the contracts operation by operation,
// DESIGN.md 5.3n the design.
//
// Both are chains -- Prim's algorithm is S - 1 dependent arg-minima, MDS m - 1 -- so both take the shape of fps_reg_kernel
// (sampling.hip): ONE workgroup per patch / cloud, the points in registers (x, y, z and a key per point), and per step
//   scan      every lane updates its PPT points against the last winner and takes the smallest key word of them;
//   wave min  DPP row rotations + 4 v_readlane (rf::wave_min_u32); a lane owns PPT CONSECUTIVE points, so the lowest lane
//             holding the wave's minimum and, in it, the lowest slot is the winner under the tie order "smallest index";
//   exchange  (more than one wave) lane 0 publishes (word, index) in the wave's LDS slot, double-buffered: ONE barrier per
//             step; every 16-lane row re-reduces the <= 16 slots by DPP (smallest word, then smallest index).
// The keys are non-negative floats (or +inf), whose unsigned bit order is their order.  What may no longer win holds a word
// that no key can take: all ones for a vertex inside the tree (a NaN: the strict `d2 < key` that updates a key is false
// for it too, so a tree vertex needs no test of its own), +inf for an MDS point that is chosen or behind the count (a
// density is a sum of at most 16384 weights of at most 1 + 2^-20 each: never +inf, and inf + w stays inf).
//
// No address depends on a data value that is not bounded by construction: a winner's index is below the kernel's capacity
// (and clamped below the count before the one global read that uses it).  Every loop is bounded by a count.
#include "common.hpp"
#include "msn_poly.hpp"

namespace {

constexpr unsigned XP_INTREE = 0xFFFFFFFFu;  // a key word no d2 can take
constexpr int XG_TPB = 256;                  // the gradient kernel
constexpr float MDS_TAKEN = __builtin_huge_valf();

// ((dx dx) + (dy dy)) + (dz dz), unfused: emd_assign.hip's ea_dist without the root.  Symmetric bit for bit.
__device__ __forceinline__ float d2_unfused(float dx, float dy, float dz) { return ((dx * dx) + (dy * dy)) + (dz * dz); }
__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// The workgroup's arg-min of (word, index).  lm: the smallest word among the lane's PPT consecutive points
// (t * PPT + s), sidx: the lowest slot s holding it.  Returns the winner's index, uniform.  More than one wave: ONE barrier;
// call j uses buffer j & 1 (a wave can be one call ahead of another, never two: the barrier of call j + 1 is in between).
template <int NT, int PPT>
__device__ __forceinline__ int block_argmin(unsigned lm, int sidx, int wave, int lane, unsigned (*slot_w)[16],
                                            unsigned (*slot_v)[16], int buf) {
    const unsigned wm = rf::wave_min_u32(lm);
    const unsigned long long hl = __ballot(lm == wm);  // (never empty: wm is one of the lm)
    const int wl = hl ? __builtin_ctzll(hl) : 0;
    const int bs = __builtin_amdgcn_readlane(sidx, wl);
    const unsigned wv = (unsigned)((wave * 64 + wl) * PPT + bs);
    if (NT == 64) return (int)wv;
    if (lane == 0) {
        slot_w[buf][wave] = wm;
        slot_v[buf][wave] = wv;
    }
    __syncthreads();
    const unsigned sw = slot_w[buf][lane & 15];
    const unsigned sv = slot_v[buf][lane & 15];
    const unsigned gm = rf::row_allmin_u(sw);
    const unsigned gv = rf::row_allmin_u(sw == gm ? sv : 0xFFFFFFFFu);
    return (int)__builtin_amdgcn_readfirstlane(gv);
}

// ---- the expansion penalty ------------------------------------------------------------------------------------------
// One workgroup per patch (blockIdx.x = sample * P + patch; the patches of a batch are consecutive runs of S rows).  The
// patch's coordinates also sit in LDS: the winner's are read from there (a uniform address: a broadcast), and the same
// array carries the lengths to the one thread that sums them afterwards.
template <int NT, int PPT>
__global__ __launch_bounds__(NT) void xp_kernel(int S, int P, float alpha, const float *__restrict__ xyz,
                                                float *__restrict__ dist, int *__restrict__ father,
                                                float *__restrict__ length, float *__restrict__ mean,
                                                int *__restrict__ info) {
    constexpr int CAP = NT * PPT;
    __shared__ float sc[CAP * 3];
    __shared__ unsigned slot_w[2][16], slot_v[2][16];
    __shared__ double mean_sh;
    const size_t q = blockIdx.x;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *__restrict__ X = xyz + q * (size_t)S * 3;
    const size_t row0 = q * (size_t)S;
    const int fbase = (int)(q % (size_t)P) * S;

    float px[PPT], py[PPT], pz[PPT];
    unsigned kb[PPT], lk[PPT];  // the key's word (XP_INTREE once inside the tree); the key the vertex joined with
    int fa[PPT];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int v = t * PPT + s;
        px[s] = py[s] = pz[s] = 0.f;
        if (v < S) {
            px[s] = X[v * 3 + 0], py[s] = X[v * 3 + 1], pz[s] = X[v * 3 + 2];
            sc[v * 3 + 0] = px[s], sc[v * 3 + 1] = py[s], sc[v * 3 + 2] = pz[s];
            bad = bad || nonfinite(px[s]) || nonfinite(py[s]) || nonfinite(pz[s]);
        }
    }
    if (NT > 64 && t < 32) {  // unused slots never win
        slot_w[t >> 4][t & 15] = 0xFFFFFFFFu;
        slot_v[t >> 4][t & 15] = 0xFFFFFFFFu;
    }
    if (__syncthreads_or(bad)) {  // (uniform) the patch is reported, its neighbours never see it
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int v = t * PPT + s;
            if (v < S) dist[row0 + v] = 0.f, length[row0 + v] = 0.f, father[row0 + v] = fbase + v;
        }
        if (t == 0) mean[q] = 0.f, info[q] = RF_XP_NONFINITE;
        return;
    }

    float ux = sc[0], uy = sc[1], uz = sc[2];  // Prim from local vertex 0
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int v = t * PPT + s;
        const bool outside = v < S && v != 0;  // the root and the slots behind S are "inside" from the start
        kb[s] = outside ? __float_as_uint(d2_unfused(px[s] - ux, py[s] - uy, pz[s] - uz)) : XP_INTREE;
        lk[s] = 0u;
        fa[s] = 0;
    }
    for (int j = 1; j < S; j++) {
        unsigned lm = kb[0];
#pragma unroll
        for (int s = 1; s < PPT; s++) lm = min(lm, kb[s]);
        int sidx = 0;
#pragma unroll
        for (int s = PPT - 1; s >= 1; s--) sidx = kb[s] == lm ? s : sidx;
        if (PPT > 1) sidx = kb[0] == lm ? 0 : sidx;
        const int u = block_argmin<NT, PPT>(lm, sidx, wave, lane, slot_w, slot_v, j & 1);
        ux = sc[u * 3 + 0], uy = sc[u * 3 + 1], uz = sc[u * 3 + 2];
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const bool won = t * PPT + s == u;
            lk[s] = won ? kb[s] : lk[s];
            kb[s] = won ? XP_INTREE : kb[s];
            const float d = d2_unfused(px[s] - ux, py[s] - uy, pz[s] - uz);
            const bool upd = d < __uint_as_float(kb[s]);  // strict: the earliest tree vertex keeps a tie; false inside the tree
            kb[s] = upd ? __float_as_uint(d) : kb[s];
            fa[s] = upd ? u : fa[s];
        }
    }

    float len[PPT];
    __syncthreads();  // the last step's readers of sc are through
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int v = t * PPT + s;
        len[s] = sqrtf(__uint_as_float(lk[s]));
        if (v < S) sc[v] = len[s];
    }
    __syncthreads();
    if (t == 0) {  // one thread, one pass, ascending: the sum has one order
        double a = 0.0;
        for (int v = 1; v < S; v++) a += (double)sc[v];
        mean_sh = a / (double)(S - 1);
    }
    __syncthreads();
    const double mean64 = mean_sh, bar = (double)alpha * mean64;
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int v = t * PPT + s;
        if (v < S) {
            length[row0 + v] = len[s];
            father[row0 + v] = fbase + fa[s];
            dist[row0 + v] = (double)len[s] > bar ? len[s] : 0.f;
        }
    }
    if (t == 0) mean[q] = (float)mean64, info[q] = RF_XP_OK;
}

// ---- its gradient ---------------------------------------------------------------------------------------------------
// t_v = gdist[v] ((x_v - x_f) / l_v), f = father[v] clamped into the patch, l_v recomputed (0 where l_v = 0)
__device__ __forceinline__ void xg_term(const float *__restrict__ X, int v, int f, float g, float &tx, float &ty, float &tz) {
    const float dx = X[v * 3 + 0] - X[f * 3 + 0], dy = X[v * 3 + 1] - X[f * 3 + 1], dz = X[v * 3 + 2] - X[f * 3 + 2];
    const float l = sqrtf(d2_unfused(dx, dy, dz));
    tx = ty = tz = 0.f;
    if (l != 0.f) tx = g * (dx / l), ty = g * (dy / l), tz = g * (dz / l);
}

// One workgroup per patch.  The penalised vertices (dist != 0) are compacted IN INDEX ORDER into an LDS list of (father,
// term): a first pass counts them per chunk of 64 rows (one ballot), a second places them (the chunk's base + the lane's
// rank in the ballot).  Every thread then walks the list for each of its rows and sums in double in list order: no
// atomics, one order.  Dynamic LDS: 14 S bytes.
__global__ __launch_bounds__(XG_TPB) void xp_grad_kernel(int S, int P, const float *__restrict__ xyz,
                                                         const int *__restrict__ father, const float *__restrict__ dist,
                                                         const float *__restrict__ gdist, float *__restrict__ grad) {
    extern __shared__ __align__(16) unsigned char xg_lds[];
    float *__restrict__ tx = reinterpret_cast<float *>(xg_lds);
    float *__restrict__ ty = tx + S;
    float *__restrict__ tz = ty + S;
    unsigned short *__restrict__ lf = reinterpret_cast<unsigned short *>(tz + S);
    __shared__ int cnt[RF_XP_MAX_PATCH / 64];
    constexpr int NW = XG_TPB / 64;
    const size_t q = blockIdx.x;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *__restrict__ X = xyz + q * (size_t)S * 3;
    const size_t row0 = q * (size_t)S;
    const int fbase = (int)(q % (size_t)P) * S;
    const int chunks = (S + 63) / 64;

    for (int c = wave; c < chunks; c += NW) {
        const int v = c * 64 + lane;
        const unsigned long long pen = __ballot(v < S && dist[row0 + v] != 0.f);
        if (lane == 0) cnt[c] = __popcll(pen);
    }
    __syncthreads();
    int before = 0, seen = 0;  // penalised vertices in the chunks below `seen`
    for (int c = wave; c < chunks; c += NW) {
        for (; seen < c; seen++) before += cnt[seen];
        const int v = c * 64 + lane;
        const bool mine = v < S && dist[row0 + v] != 0.f;
        const unsigned long long pen = __ballot(mine);
        if (mine) {
            int f = father[row0 + v] - fbase;
            f = f < 0 ? 0 : (f >= S ? S - 1 : f);  // inside the patch whatever the index tensor holds
            const int at = before + __popcll(pen & ((1ull << lane) - 1ull));
            float ax, ay, az;
            xg_term(X, v, f, gdist[row0 + v], ax, ay, az);
            tx[at] = ax, ty[at] = ay, tz[at] = az;
            lf[at] = (unsigned short)f;
        }
    }
    for (; seen < chunks; seen++) before += cnt[seen];
    const int K = before;
    __syncthreads();
    for (int w = t; w < S; w += XG_TPB) {
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (dist[row0 + w] != 0.f) {
            int f = father[row0 + w] - fbase;
            f = f < 0 ? 0 : (f >= S ? S - 1 : f);
            float ox, oy, oz;
            xg_term(X, w, f, gdist[row0 + w], ox, oy, oz);
            ax += (double)ox, ay += (double)oy, az += (double)oz;
        }
        for (int k = 0; k < K; k++) {
            if (lf[k] == (unsigned short)w) ax -= (double)tx[k], ay -= (double)ty[k], az -= (double)tz[k];
        }
        float *__restrict__ G = grad + (row0 + w) * 3;
        G[0] = (float)ax, G[1] = (float)ay, G[2] = (float)az;
    }
}

// ---- minimum density sampling ---------------------------------------------------------------------------------------
// w(d2): 2^-(d2 c) for d2 c < 64, else 0 (NaN and inf included); c = log2(e) / (2 sigma^2).  floor and the subtraction are
// exact, the polynomial is msn_poly.hpp's in Horner form with separate multiplies and adds, the scaling by 2^-k is exact.
__device__ __forceinline__ float mds_weight(float d2, float c) {
    const float s = d2 * c;
    const bool near = s < 64.0f;
    const float sv = near ? s : 0.f;
    const float k = floorf(sv);
    const float f = sv - k;
    float p = RF_MDS_POLY_C5;
    p = p * f + RF_MDS_POLY_C4;
    p = p * f + RF_MDS_POLY_C3;
    p = p * f + RF_MDS_POLY_C2;
    p = p * f + RF_MDS_POLY_C1;
    p = p * f + RF_MDS_POLY_C0;
    return near ? ldexpf(p, -(int)k) : 0.f;
}

template <int NT, int PPT>
__global__ __launch_bounds__(NT) void mds_kernel(int n, int m, const float *__restrict__ xyz,
                                                 const float *__restrict__ sigma, const int *__restrict__ len,
                                                 int *__restrict__ out, int *__restrict__ info,
                                                 float *__restrict__ new_xyz) {
    __shared__ unsigned slot_w[2][16], slot_v[2][16];
    const int bi = blockIdx.x;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *__restrict__ P = xyz + (size_t)bi * n * 3;
    int *__restrict__ O = out + (size_t)bi * m;
    float *__restrict__ NX = new_xyz ? new_xyz + (size_t)bi * m * 3 : nullptr;
    const int L = rf::ragged_count(len, bi, n);
    const int mo = m < L ? m : L;
    const float sg = sigma[bi];
    const double c64 = 1.4426950408889634 / (2.0 * (double)sg * (double)sg);
    const float c = (float)c64;
    const bool bad = !(sg > 0.f) || c == 0.f || c == __builtin_huge_valf();

    for (int j = (bad ? 0 : mo) + t; j < m; j += NT) {  // a bad scale: the first mo points as they come; always: the tail is zeros
        const bool take = j < mo;
        O[j] = take ? j : 0;
        if (NX) {
            NX[j * 3 + 0] = take ? P[j * 3 + 0] : 0.f;
            NX[j * 3 + 1] = take ? P[j * 3 + 1] : 0.f;
            NX[j * 3 + 2] = take ? P[j * 3 + 2] : 0.f;
        }
    }
    if (t == 0) info[bi] = bad ? RF_MDS_BADSIGMA : RF_MDS_OK;
    if (bad) return;  // (uniform)

    float px[PPT], py[PPT], pz[PPT], dens[PPT];
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int v = t * PPT + s;
        px[s] = py[s] = pz[s] = 0.f;
        dens[s] = MDS_TAKEN;  // behind the count: never a candidate
        if (v < L) {
            px[s] = P[v * 3 + 0], py[s] = P[v * 3 + 1], pz[s] = P[v * 3 + 2];
            dens[s] = 0.f;
        }
    }
    if (NT > 64 && t < 32) {  // unused slots never win
        slot_w[t >> 4][t & 15] = 0xFFFFFFFFu;
        slot_v[t >> 4][t & 15] = 0xFFFFFFFFu;
    }
    __syncthreads();
    int u = 0;
    float ox = P[0], oy = P[1], oz = P[2];
    if (t == 0) {
        O[0] = 0;
        if (NX) NX[0] = ox, NX[1] = oy, NX[2] = oz;
    }
    for (int j = 1; j < mo; j++) {
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const float w = mds_weight(d2_unfused(px[s] - ox, py[s] - oy, pz[s] - oz), c);
            dens[s] = t * PPT + s == u ? MDS_TAKEN : dens[s] + w;
        }
        unsigned lm = __float_as_uint(dens[0]);
#pragma unroll
        for (int s = 1; s < PPT; s++) lm = min(lm, __float_as_uint(dens[s]));
        int sidx = 0;
#pragma unroll
        for (int s = PPT - 1; s >= 1; s--) sidx = __float_as_uint(dens[s]) == lm ? s : sidx;
        if (PPT > 1) sidx = __float_as_uint(dens[0]) == lm ? 0 : sidx;
        u = block_argmin<NT, PPT>(lm, sidx, wave, lane, slot_w, slot_v, j & 1);
        u = u < L ? u : L - 1;  // (it is: j < mo <= L leaves a candidate.  The read below is inside the cloud regardless)
        ox = P[u * 3 + 0];      // uniform address: scalar loads
        oy = P[u * 3 + 1];
        oz = P[u * 3 + 2];
        if (t == 0) {
            O[j] = u;
            if (NX) NX[j * 3 + 0] = ox, NX[j * 3 + 1] = oy, NX[j * 3 + 2] = oz;
        }
    }
}

bool alpha_ok(float alpha) { return alpha >= 0.f && alpha <= 3.402823466e38f; }

}  // namespace

extern "C" {

int rf_expansion_penalty_supported(int n, int S) { return S >= 2 && S <= RF_XP_MAX_PATCH && n >= S && n % S == 0; }

int rf_expansion_penalty(int b, int n, int S, float alpha, const float *xyz, float *dist, int *father, float *length,
                         float *mean, int *info, rf_stream_t stream) {
    if (b < 0 || n < 0 || S < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!rf_expansion_penalty_supported(n, S) || !alpha_ok(alpha)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, dist, father, length, mean, info})) return RF_EINVAL;
    const int P = n / S;
    const long long patches = (long long)b * P;
    if (patches > 2147483647LL) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define XP_GO(NT, PPT)                                                                                                  \
    do {                                                                                                                \
        RF_LAUNCH("expansion_penalty", (xp_kernel<NT, PPT>), dim3((unsigned)patches), dim3(NT), 0, s, S, P, alpha, xyz, \
                  dist, father, length, mean, info);                                                                    \
    } while (0)
    if (S <= 256) XP_GO(64, 4);
    else if (S <= 1024) XP_GO(256, 4);
    else XP_GO(1024, 4);
#undef XP_GO
    return RF_OK;
}

int rf_expansion_penalty_grad(int b, int n, int S, const float *xyz, const int *father, const float *dist,
                              const float *gdist, float *grad, rf_stream_t stream) {
    if (b < 0 || n < 0 || S < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!rf_expansion_penalty_supported(n, S)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, father, dist, gdist, grad})) return RF_EINVAL;
    const int P = n / S;
    const long long patches = (long long)b * P;
    if (patches > 2147483647LL) return RF_EINVAL;
    RF_LAUNCH("expansion_penalty_grad", xp_grad_kernel, dim3((unsigned)patches), dim3(XG_TPB), (size_t)S * 14,
              (hipStream_t)stream, S, P, xyz, father, dist, gdist, grad);
    return RF_OK;
}

int rf_mds_supported(int n) { return n >= 1 && n <= RF_MDS_MAX_POINTS; }

int rf_mds(int b, int n, int m, const float *xyz, const float *sigma, const int *len, int *out, int *info, float *new_xyz,
           rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!rf_mds_supported(n) || m < 1) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, sigma, out, info}, {len, new_xyz})) return RF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define MDS_GO(NT, PPT)                                                                                              \
    do {                                                                                                             \
        RF_LAUNCH("mds", (mds_kernel<NT, PPT>), dim3(b), dim3(NT), 0, s, n, m, xyz, sigma, len, out, info, new_xyz); \
    } while (0)
    if (n <= 256) MDS_GO(64, 4);
    else if (n <= 1024) MDS_GO(256, 4);
    else if (n <= 4096) MDS_GO(1024, 4);
    else if (n <= 8192) MDS_GO(1024, 8);
    else MDS_GO(1024, 16);
#undef MDS_GO
    return RF_OK;
}

}  // extern "C"
