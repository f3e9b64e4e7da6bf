// emd_assign.hip -- the earth mover's distance itself: the optimal one-to-one assignment of two clouds of equal counts by a
// deterministic Jacobi auction with eps-scaling on an INTEGER cost grid, with an optimality certificate (a dual lower bound
// in exact integers) and the gradients of the cost under the assignment.  include/rfops.h states the contract, DESIGN.md
// 5.3j the measurements.
//
//   grid      per sample: lo / hi per axis over the 2 L valid points, E = the largest extent, S = 2^k the power of two that
//             puts the costs c_ij = rint(d_ij S) below 2^20 (d_ij fp32, unfused, correctly rounded sqrt; d S is exact).
//   auction   ONE workgroup per sample (the rounds of an auction are a chain; no workgroup ever waits for another one).
//             Objects' coordinates, prices, owners and the per-object bid words live in LDS; costs are recomputed on the fly,
//             nothing of size n^2 exists anywhere.  A round works on the prices and the list of unassigned persons as they are
//             at its start: (A) every unassigned person scans all objects for the lowest and second lowest v = c + p, the
//             lowest by the 64-bit key (v, (j - i) mod L), and raises the object's bid word to (beta, ~i) with a 64-bit LDS
//             maximum -- the order in which bidders arrive cannot matter; (B) every bidder looks at its object's bid word: the
//             winner books price and owner and puts the previous owner on the next round's list, a loser puts itself there.
//             With 9 bidders or more a wave takes a bidder (EA_WAVES bidders side by side); in the long tail of rounds with
//             one to eight bidders a bidder's scan is spread over 2, 4, 8 or all 16 waves, whose partial (lowest, second
//             lowest) keys meet in LDS.  The lists' order depends on arrival, the SET does not, and nothing else is read.
//   finish    the capped fill when max_rounds ran out, match12 / match21 / dist, P and D by one more sweep, the cost summed in
//             double in index order by one thread, final prices to the workspace (with them anyone can recompute D).
//
// Range: prices and values stay below 2^26, so int32 suffices.  Within a phase, while an object exists that has had no bid in
// this phase, its price is still its price p0 <= M at the phase's start (M the highest price then).  A bidder i that does not
// bid for it has w <= c_i,j0 + p0, so its bid beta = w - c_i,j* + eps <= M + C + eps (C <= 2^20 the largest cost).  A bidder
// that takes the LAST such object has w <= C + (M + C + eps), so beta <= M + 2 (C + eps).  Once every object has had a bid in
// the phase every object is owned, every person is assigned and the phase is over.  So a phase raises the highest price by at
// most 2 (C + eps), and seven phases by 14 * 2^20 + 2 * (2^17 + 2^14 + ... + 1) < 2^25.  v = c + p < 2^26.
//
// Every loop is bounded by a count (L, the number of waves, seven phases) or by max_rounds, never by a data value: the kernel
// ends on any input.  Out of scope: a sample spread over several workgroups, n > RF_EA_MAX_POINTS, unequal counts.
#include "common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int EA_TPB = 1024;           // threads per workgroup
constexpr int EA_WAVES = EA_TPB / 64;  // bidders side by side in a round with many bidders
constexpr int EA_GTPB = 256;           // the gradient kernel
constexpr u64 EA_NOKEY = ~0ull;
constexpr float EA_CMAX = 1048576.0f;  // 2^20: reached only when the squares overflow fp32 (E >= 2^63)

__device__ __forceinline__ float ea_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
}
__device__ __forceinline__ int ea_cost(float d, float S) { return (int)rintf(fminf(d * S, EA_CMAX)); }

// (lowest, second lowest) of two disjoint sets of distinct keys
__device__ __forceinline__ void ea_merge(u64 &a1, u64 &a2, u64 b1, u64 b2) {
    const bool lt = a1 < b1;
    const u64 lo = lt ? a1 : b1, hi = lt ? b1 : a1, m2 = a2 < b2 ? a2 : b2;
    a1 = lo, a2 = hi < m2 ? hi : m2;
}
template <int FROM>
__device__ __forceinline__ void ea_reduce(u64 &k1, u64 &k2) {
#pragma unroll
    for (int o = FROM; o > 0; o >>= 1) {
        const u64 b1 = __shfl_xor(k1, o, 64), b2 = __shfl_xor(k2, o, 64);
        ea_merge(k1, k2, b1, b2);
    }
}

struct EaArgs {
    int b, n, max_rounds;
    const float *xyz1, *xyz2;
    const int *len;
    int *match12, *match21;
    float *dist, *val;
    long long *cert;
    int *info, *price_out;
};

// grid (b), EA_TPB threads; dynamic LDS: 34 bytes per point of the padded count (rounded up to a multiple of 4)
__global__ __launch_bounds__(EA_TPB) void emd_assign_kernel(EaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ea_lds[];
    __shared__ u64 part[2][EA_WAVES][2];
    __shared__ long long red[3][EA_WAVES];
    __shared__ float ext[7][EA_WAVES];
    __shared__ int cnt[2];

    const int s = blockIdx.x, n = a.n, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = (n + 3) & ~3;
    const int L = rf::ragged_count(a.len, s, n);
    u64 *__restrict__ bid = (u64 *)ea_lds;                         // per object: (beta << 32 | ~i), 0 = no bid
    float *__restrict__ ox = (float *)(bid + np), *__restrict__ oy = ox + np, *__restrict__ oz = oy + np;
    int *__restrict__ price = (int *)(oz + np), *__restrict__ owner = price + np;
    unsigned short *__restrict__ ul0 = (unsigned short *)(owner + np), *__restrict__ ul1 = ul0 + np;
    unsigned short *__restrict__ jstar = ul1 + np;                 // per list position: the object bid for
    const float *__restrict__ X1 = a.xyz1 + (size_t)s * n * 3, *__restrict__ X2 = a.xyz2 + (size_t)s * n * 3;

    // ---- the grid ----
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.f;
    for (int j = tid; j < L; j += EA_TPB) {
        const float p[3] = {X1[j * 3], X1[j * 3 + 1], X1[j * 3 + 2]}, q[3] = {X2[j * 3], X2[j * 3 + 1], X2[j * 3 + 2]};
        ox[j] = q[0], oy[j] = q[1], oz[j] = q[2];
        price[j] = 0, owner[j] = j, bid[j] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = fminf(lo[c], fminf(p[c], q[c]));
            hi[c] = fmaxf(hi[c], fmaxf(p[c], q[c]));
            if (!(p[c] - p[c] == 0.f) || !(q[c] - q[c] == 0.f)) bad = 1.f;  // NaN or infinite: fminf would skip a NaN
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
        }
        bad = fmaxf(bad, __shfl_xor(bad, o, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) ext[c][wave] = lo[c], ext[3 + c][wave] = hi[c];
        ext[6][wave] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < EA_WAVES; w++) {
#pragma unroll
        for (int c = 0; c < 3; c++) lo[c] = fminf(lo[c], ext[c][w]), hi[c] = fmaxf(hi[c], ext[3 + c][w]);
        bad = fmaxf(bad, ext[6][w]);
    }
    const float E = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    const bool nonfinite = bad != 0.f || !(E - E == 0.f);
    int k = 0;
    if (!nonfinite) {  // frexpf's exponent from the bits; a subnormal E is below the clamp anyway
        const int e8 = (int)((__float_as_uint(E) >> 23) & 0xFFu);
        const int ex = E == 0.f ? 0 : (e8 ? e8 - 126 : -126);
        k = 19 - (ex > -100 ? ex : -100);  // -109 ... 119
    }
    const float S = __uint_as_float((unsigned)(k + 127) << 23);

    // ---- the auction ----
    const int cap = a.max_rounds > 0 ? a.max_rounds : 64 * L + 1024;
    int rounds = 0, cur = 0;
    long long bids = 0;
    bool capped = false;
    for (int phase = 0; phase < 7 && !nonfinite && !capped; phase++) {
        const int eps = phase < 6 ? 1 << (17 - 3 * phase) : 1;
        unsigned short *__restrict__ ul = cur ? ul1 : ul0;
        __syncthreads();  // everyone has read the empty list's count that ended the previous phase
        for (int j = tid; j < L; j += EA_TPB) owner[j] = -1, ul[j] = (unsigned short)j;
        if (tid == 0) cnt[cur] = L;
        __syncthreads();
        for (int r = 0; r <= cap; r++) {  // (leaves through one of the two breaks: rounds <= cap)
            const int nU = cnt[cur];
            if (nU == 0) break;
            if (rounds >= cap) {
                capped = true;
                break;
            }
            const unsigned short *__restrict__ uc = cur ? ul1 : ul0;
            unsigned short *__restrict__ un = cur ? ul0 : ul1;
            if (tid == 0) cnt[cur ^ 1] = 0;
            // (A) the bids
            const int G = L <= 64 || nU >= 9 ? 1 : (nU >= 5 ? 2 : (nU >= 3 ? 4 : (nU == 2 ? 8 : 16)));
            const int ngroups = EA_WAVES / G, grp = wave / G, wig = wave - grp * G;
            const int iters = (nU + ngroups - 1) / ngroups, Q = 64 * G, q = wig * 64 + lane;
            for (int it = 0; it < iters; it++) {
                const int t = it * ngroups + grp;
                const bool on = t < nU;
                u64 k1 = EA_NOKEY, k2 = EA_NOKEY;
                int i = 0;
                if (on) {
                    i = uc[t];
                    const float ax = X1[i * 3], ay = X1[i * 3 + 1], az = X1[i * 3 + 2];
                    for (int j = q; j < L; j += Q) {
                        const unsigned v = (unsigned)(ea_cost(ea_dist(ax, ay, az, ox[j], oy[j], oz[j]), S) + price[j]);
                        const int rot = j - i + (j < i ? L : 0);
                        const u64 key = ((u64)v << 32) | (unsigned)rot;
                        if (key < k1) k2 = k1, k1 = key;
                        else if (key < k2) k2 = key;
                    }
                    ea_reduce<32>(k1, k2);
                }
                if (G > 1) {
                    if (lane == 0) part[it & 1][wave][0] = k1, part[it & 1][wave][1] = k2;
                    __syncthreads();
                    if (on && wig == 0) {
                        k1 = lane < G ? part[it & 1][wave + lane][0] : EA_NOKEY;
                        k2 = lane < G ? part[it & 1][wave + lane][1] : EA_NOKEY;
                        ea_reduce<8>(k1, k2);
                    }
                }
                if (on && wig == 0 && lane == 0) {
                    int js = (int)(unsigned)k1 + i;
                    js -= js >= L ? L : 0;
                    const int v1 = (int)(k1 >> 32), w = L == 1 ? v1 : (int)(k2 >> 32);
                    const int beta = price[js] + (w - v1) + eps;
                    atomicMax(&bid[js], ((u64)(unsigned)beta << 32) | (unsigned)~i);
                    jstar[t] = (unsigned short)js;
                }
            }
            __syncthreads();
            // (B) the sales
            for (int t = tid; t < nU; t += EA_TPB) {
                const int i = uc[t], js = jstar[t];
                const u64 top = bid[js];
                if ((unsigned)top == (unsigned)~i) {
                    const int old = owner[js];
                    owner[js] = i, price[js] = (int)(top >> 32), bid[js] = 0;
                    if (old >= 0) un[atomicAdd(&cnt[cur ^ 1], 1)] = (unsigned short)old;
                } else {
                    un[atomicAdd(&cnt[cur ^ 1], 1)] = (unsigned short)i;
                }
            }
            __syncthreads();
            rounds++, bids += nU, cur ^= 1;
        }
    }

    // ---- the capped fill: unassigned persons in ascending i take the free objects in ascending j ----
    int *__restrict__ flag = (int *)bid;  // every bid word is 0 between rounds
    if (capped) {
        __syncthreads();
        for (int j = tid; j < L; j += EA_TPB)
            if (owner[j] >= 0) flag[owner[j]] = 1;
        __syncthreads();
        if (tid == 0) {
            int j = 0;
            for (int i = 0; i < L; i++) {
                if (flag[i]) continue;
                for (; j < L && owner[j] >= 0; j++) {}
                if (j < L) owner[j++] = i;
            }
        }
    }
    __syncthreads();

    // ---- outputs, P, D ----
    float *__restrict__ sdist = (float *)ea_lds;  // (the flags are done with)
    int *__restrict__ M12 = a.match12 + (size_t)s * n, *__restrict__ M21 = a.match21 + (size_t)s * n;
    float *__restrict__ DI = a.dist + (size_t)s * n;
    int *__restrict__ PR = a.price_out + (size_t)s * n;
    long long sP = 0, sPrice = 0, sMin = 0;
    for (int j = tid; j < n; j += EA_TPB) {
        if (j < L) {
            const int i = owner[j];
            const float d = ea_dist(X1[i * 3], X1[i * 3 + 1], X1[i * 3 + 2], ox[j], oy[j], oz[j]);
            sP += ea_cost(d, S), sPrice += price[j];
            M21[j] = i, M12[i] = j, DI[i] = d, sdist[i] = d, PR[j] = price[j];
        } else {
            M21[j] = 0, M12[j] = 0, DI[j] = 0.f;
        }
    }
    for (int i = wave; i < L; i += EA_WAVES) {
        const float ax = X1[i * 3], ay = X1[i * 3 + 1], az = X1[i * 3 + 2];
        int m = 0x7FFFFFFF;
        for (int j = lane; j < L; j += 64) m = min(m, ea_cost(ea_dist(ax, ay, az, ox[j], oy[j], oz[j]), S) + price[j]);
        m = rf::wave_reduce(m, [](int x, int y) { return min(x, y); });
        if (lane == 0) sMin += m;
    }
    sP = rf::wave_sum(sP), sPrice = rf::wave_sum(sPrice), sMin = rf::wave_sum(sMin);
    if (lane == 0) red[0][wave] = sP, red[1][wave] = sPrice, red[2][wave] = sMin;
    __syncthreads();
    if (tid == 0) {
        long long P = 0, D = 0;
        for (int w = 0; w < EA_WAVES; w++) P += red[0][w], D += red[2][w] - red[1][w];
        double cost = 0.0;
        for (int i = 0; i < L; i++) cost += (double)sdist[i];
        const double Sd = (double)S;
        float *__restrict__ V = a.val + (size_t)s * 3;
        V[0] = (float)cost, V[1] = (float)((double)(P - D) / Sd), V[2] = (float)((double)(P - D + L) / Sd);
        a.cert[(size_t)s * 2] = P, a.cert[(size_t)s * 2 + 1] = D;
        int *__restrict__ I = a.info + (size_t)s * 4;
        I[0] = nonfinite ? RF_EA_NONFINITE : (capped ? RF_EA_CAPPED : RF_EA_OK);
        I[1] = rounds, I[2] = bids > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)bids, I[3] = k;
    }
}

// grid (ceil(n / EA_GTPB), b): slot k of both clouds
__global__ __launch_bounds__(EA_GTPB) void emd_assign_grad_kernel(int n, const float *__restrict__ xyz1,
                                                                   const float *__restrict__ xyz2,
                                                                   const int *__restrict__ match12,
                                                                   const int *__restrict__ match21,
                                                                   const int *__restrict__ len, const float *__restrict__ gcost,
                                                                   float *__restrict__ grad1, float *__restrict__ grad2) {
    const int s = blockIdx.y, k = blockIdx.x * EA_GTPB + threadIdx.x;
    if (k >= n) return;
    const int L = rf::ragged_count(len, s, n);
    const size_t row = (size_t)s * n;
    float *__restrict__ g1 = grad1 + (row + k) * 3, *__restrict__ g2 = grad2 + (row + k) * 3;
    if (k >= L) {
        g1[0] = 0.f, g1[1] = 0.f, g1[2] = 0.f, g2[0] = 0.f, g2[1] = 0.f, g2[2] = 0.f;
        return;
    }
    const float g = gcost[s];
    const float *__restrict__ X1 = xyz1 + row * 3, *__restrict__ X2 = xyz2 + row * 3;
#pragma unroll
    for (int second = 0; second < 2; second++) {
        int o = second ? match21[row + k] : match12[row + k];
        o = o < 0 ? 0 : (o >= L ? L - 1 : o);  // a partner is inside the sample whatever the index tensors hold
        const int i = second ? o : k, j = second ? k : o;
        const float dx = X1[i * 3] - X2[j * 3], dy = X1[i * 3 + 1] - X2[j * 3 + 1], dz = X1[i * 3 + 2] - X2[j * 3 + 2];
        const float d = sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
        float tx = 0.f, ty = 0.f, tz = 0.f;
        if (d != 0.f) tx = g * (dx / d), ty = g * (dy / d), tz = g * (dz / d);
        if (second) g2[0] = 0.f - tx, g2[1] = 0.f - ty, g2[2] = 0.f - tz;  // (0 - 0 = +0)
        else g1[0] = tx, g1[1] = ty, g1[2] = tz;
    }
}

size_t ea_lds_bytes(int n) { return (size_t)((n + 3) & ~3) * 34; }

}  // namespace

extern "C" {

int rf_emd_assign_supported(int n) { return n >= 1 && n <= RF_EA_MAX_POINTS; }

size_t rf_emd_assign_workspace_bytes(int b, int n) {
    if (b <= 0 || !rf_emd_assign_supported(n) || b > 65535) return 0;
    return rf::align256((size_t)b * (size_t)n * sizeof(int));
}

int rf_emd_assign(int b, int n, const float *xyz1, const float *xyz2, const int *len, int max_rounds, int *match12,
                  int *match21, float *dist, float *val, long long *cert, int *info, void *workspace,
                  size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_EA_MAX_POINTS || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, match12, match21, dist, val, cert, info}, {len})) return RF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(cert) & 7u) != 0) return RF_EINVAL;  // 64-bit words
    if (!rf::workspace_ok(workspace) || max_rounds < 0) return RF_EINVAL;
    if (workspace_bytes < rf_emd_assign_workspace_bytes(b, n)) return RF_EWORKSPACE;
    RF_HIP(hipFuncSetAttribute((const void *)emd_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)ea_lds_bytes(RF_EA_MAX_POINTS)));
    const EaArgs a{b, n, max_rounds, xyz1, xyz2, len, match12, match21, dist, val, cert, info, (int *)workspace};
    RF_LAUNCH("emd_assign", emd_assign_kernel, dim3(b), dim3(EA_TPB), ea_lds_bytes(n), (hipStream_t)stream, a);
    return RF_OK;
}

int rf_emd_assign_grad(int b, int n, const float *xyz1, const float *xyz2, const int *match12, const int *match21,
                       const int *len, const float *gcost, float *grad1, float *grad2, rf_stream_t stream) {
    if (b < 0 || n < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (n < 1 || n > RF_EA_MAX_POINTS || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, match12, match21, gcost, grad1, grad2}, {len})) return RF_EINVAL;
    RF_LAUNCH("emd_assign_grad", emd_assign_grad_kernel, dim3(rf::ceil_div(n, EA_GTPB), b), dim3(EA_GTPB), 0,
              (hipStream_t)stream, n, xyz1, xyz2, match12, match21, len, gcost, grad1, grad2);
    return RF_OK;
}

}  // extern "C"
