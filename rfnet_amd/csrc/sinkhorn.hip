// sinkhorn.hip -- the Sinkhorn divergence S_eps of two clouds (debiased entropy-regularised optimal transport) with the
// gradients of its last step.  include/rfops.h states the contract; DESIGN.md 5.3k the layout and the measurements.
//
//   sweep    one launch per step serves the four soft-min problems (xy, yx, xx, yy) of every sample: a workgroup is (problem,
//            sample, tile of SK_TPB rows, chunk of columns).  A lane owns a row.  The columns of the chunk pass through LDS a
//            tile of SK_CT at a time as (x, y, z, h): every lane reads the same address, so the reads are broadcasts.  The sum
//            is a log-sum-exp in the base-2 domain (v_exp_f32 / v_log_f32) with a running maximum that is renewed once per
//            block of SK_CB columns, not per pair; the step that feeds the gradients carries the three numerators
//            sum_j 2^z dC/dx beside the running sum and rescales them with it.
//   lazily   a step writes only the (max, sum) partial of every (row, chunk).  The NEXT launch finishes them while it stages its
//            columns: h' = (h + softmin) / 2, the chunks merged in ascending order; the workgroups of row tile 0 write h' back.
//            Potentials and partials are double-buffered in the workspace, so a launch never reads what it writes.  T steps,
//            the final soft-min and one finishing launch (loss, potentials, delta, gradients): T + 2 launches.
//   purity   the column structure of a sum -- tiles of SK_CT from column 0, ceil(tiles / SK_NSPLIT) consecutive tiles to a
//            chunk, chunks merged ascending -- is a function of the VALID column count alone: not of b, of the padded sizes or
//            of where a workgroup ran.  The four problems share every instruction, so S(x, x) is +0 bit for bit.
//
// No atomics, no float sum whose order is left open.  Every loop bound is a count.
#include "common.hpp"

namespace {

constexpr int SK_TPB = 256;      // rows of a workgroup: one per lane
constexpr int SK_CT = 256;       // columns staged in LDS at a time (4 KiB)
constexpr int SK_CB = 8;         // columns per renewal of the running maximum; divides SK_CT
constexpr int SK_NSPLIT = 4;     // chunks a row's columns are spread over at most: b = 1 at 2048 x 2048 still is 128 workgroups
constexpr int SK_FIN_TPB = 1024;
constexpr double SK_LOG2E = 1.4426950408889634, SK_LN2 = 0.6931471805599453;

__host__ __device__ __forceinline__ int sk_tiles(int L) { return (L + SK_CT - 1) / SK_CT; }
// tiles per chunk and chunks, from the valid column count alone
__host__ __device__ __forceinline__ int sk_tpc(int L) { return (sk_tiles(L) + SK_NSPLIT - 1) / SK_NSPLIT; }
__device__ __forceinline__ int sk_nch(int L) { return (sk_tiles(L) + sk_tpc(L) - 1) / sk_tpc(L); }

__device__ __forceinline__ float sk_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float sk_log2(float x) { return __builtin_amdgcn_logf(x); }

// Potentials and partials are rows of one table per sample: f (n) | g (m) | fx (n) | gy (m).  Problem k (0 xy, 1 yx, 2 xx,
// 3 yy) updates potential k; its columns carry potential 1, 0, 2, 3 and are points of cloud 2, 1, 1, 2.
__device__ __forceinline__ size_t sk_off(int q, int n, int m) {
    return q == 0 ? 0 : (q == 1 ? (size_t)n : (q == 2 ? (size_t)n + m : (size_t)2 * n + m));
}

// the (max, sum) of a row over all its columns: the chunk partials in ascending order
__device__ __forceinline__ void sk_fold(const float2 *__restrict__ p, int nch, float &M, float &S) {
    const float2 a = p[0];
    M = a.x, S = a.y;
    for (int c = 1; c < nch; c++) {
        const float2 q = p[c];
        const float Mn = fmaxf(M, q.x);
        S = S * sk_exp2(M - Mn) + q.y * sk_exp2(q.x - Mn);
        M = Mn;
    }
}
// ... with the gradient numerators beside the sum
__device__ __forceinline__ void sk_fold_grad(const float2 *__restrict__ p, const float *__restrict__ g, int nch, float &M,
                                             float &S, float &gx, float &gy, float &gz) {
    const float2 a = p[0];
    M = a.x, S = a.y, gx = g[0], gy = g[1], gz = g[2];
    for (int c = 1; c < nch; c++) {
        const float2 q = p[c];
        const float Mn = fmaxf(M, q.x);
        const float r0 = sk_exp2(M - Mn), r1 = sk_exp2(q.x - Mn);
        S = S * r0 + q.y * r1;
        gx = gx * r0 + g[c * 3] * r1, gy = gy * r0 + g[c * 3 + 1] * r1, gz = gz * r0 + g[c * 3 + 2] * r1;
        M = Mn;
    }
}
// softmin = -eps ln 2 (M + log2(S w)), w the uniform column weight
__device__ __forceinline__ float sk_softmin(float M, float S, float w, float k) { return -(M + sk_log2(S * w)) * k; }

struct SkStep {
    int b, n, m, t;  // t: how many updates the potentials have had (0: they are zero and nothing is read)
    const float *xyz1, *xyz2;
    const int *len1, *len2;
    const float *pot_old;    // after t - 1 updates (not read for t <= 1)
    float *pot_new;          // after t updates: written here, by the workgroups of row tile 0
    const float2 *part_old;  // step t - 1's partials
    float2 *part_new;
    float *gpart;            // GRAD: the numerators of every (row, chunk)
    float sc;                // log2(e) / eps of this sweep
    float kprev;             // eps ln 2 of the sweep that wrote part_old
};

// grid (row tiles of max(n, m) * SK_NSPLIT, b, 4)
template <int P, bool GRAD>
__global__ __launch_bounds__(SK_TPB) void sk_sweep_kernel(SkStep a) {
    __shared__ float4 col[SK_CT];
    const int k = blockIdx.z, s = blockIdx.y, tid = threadIdx.x;
    const int rt = blockIdx.x / SK_NSPLIT, ch = blockIdx.x % SK_NSPLIT;
    const int n = a.n, m = a.m;
    const int L1 = rf::ragged_count(a.len1, s, n), L2 = rf::ragged_count(a.len2, s, m);
    const bool rows2 = (k & 1) != 0, cols2 = k == 0 || k == 3;
    const int Lr = rows2 ? L2 : L1, Lc = cols2 ? L2 : L1;
    const int tpc = sk_tpc(Lc), tiles = sk_tiles(Lc), t0 = ch * tpc;
    if (rt * SK_TPB >= Lr || t0 >= tiles) return;  // (the whole workgroup)
    const int t1 = t0 + tpc < tiles ? t0 + tpc : tiles;
    const float *__restrict__ rows = rows2 ? a.xyz2 + (size_t)s * m * 3 : a.xyz1 + (size_t)s * n * 3;
    const float *__restrict__ cols = cols2 ? a.xyz2 + (size_t)s * m * 3 : a.xyz1 + (size_t)s * n * 3;
    const size_t R = 2 * ((size_t)n + m), base = (size_t)s * R;
    const int qc = k == 0 ? 1 : (k == 1 ? 0 : k);
    const size_t offc = base + sk_off(qc, n, m), offr = base + sk_off(k, n, m);
    // the column potential's own last step summed over the columns of problem qc
    const int Lp = (qc == 0 || qc == 3) ? L2 : L1, nchp = sk_nch(Lp);
    const float wp = 1.0f / (float)Lp;

    const int row = rt * SK_TPB + tid, rowc = row < Lr ? row : Lr - 1;
    const float xi = rows[(size_t)rowc * 3], yi = rows[(size_t)rowc * 3 + 1], zi = rows[(size_t)rowc * 3 + 2];
    const float sc = a.sc;
    float mx = -INFINITY, sum = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;

    for (int tile = t0; tile < t1; tile++) {
        const int j = tile * SK_CT + tid;
        float4 v = make_float4(0.f, 0.f, 0.f, -INFINITY);  // behind the count: 2^z = 0 exactly
        if (j < Lc) {
            float h = 0.f;
            if (a.t > 0) {
                float M, S;
                sk_fold(a.part_old + (offc + j) * SK_NSPLIT, nchp, M, S);
                const float old = a.t > 1 ? a.pot_old[offc + j] : 0.f;
                h = 0.5f * (old + sk_softmin(M, S, wp, a.kprev));
                if (rt == 0) a.pot_new[offc + j] = h;
            }
            v = make_float4(cols[(size_t)j * 3], cols[(size_t)j * 3 + 1], cols[(size_t)j * 3 + 2], h);
        }
        __syncthreads();
        col[tid] = v;
        __syncthreads();
        const int cnt = Lc - tile * SK_CT < SK_CT ? Lc - tile * SK_CT : SK_CT;
        for (int jj = 0; jj < cnt; jj += SK_CB) {
            float z[SK_CB], dx[SK_CB], dy[SK_CB], dz[SK_CB], rc[SK_CB];
#pragma unroll
            for (int u = 0; u < SK_CB; u++) {
                const float4 c = col[jj + u];
                dx[u] = xi - c.x, dy[u] = yi - c.y, dz[u] = zi - c.z;
                const float d2 = ((dx[u] * dx[u]) + (dy[u] * dy[u])) + (dz[u] * dz[u]);
                float C;
                if (P == 1) {
                    C = __builtin_amdgcn_sqrtf(d2);
                    if (GRAD) rc[u] = C > 0.f ? __builtin_amdgcn_rcpf(C) : 0.f;
                } else {
                    C = 0.5f * d2;
                }
                z[u] = (c.w - C) * sc;
            }
            const float zb = fmaxf(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])), fmaxf(fmaxf(z[4], z[5]), fmaxf(z[6], z[7])));
            const float mn = fmaxf(mx, zb);
            const float r = sk_exp2(mx - mn);
            float w[SK_CB];
#pragma unroll
            for (int u = 0; u < SK_CB; u++) w[u] = sk_exp2(z[u] - mn);
            sum = sum * r + (((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7])));
            if (GRAD) {
                gx *= r, gy *= r, gz *= r;
#pragma unroll
                for (int u = 0; u < SK_CB; u++) {
                    const float t = P == 1 ? w[u] * rc[u] : w[u];
                    gx = fmaf(t, dx[u], gx), gy = fmaf(t, dy[u], gy), gz = fmaf(t, dz[u], gz);
                }
            }
            mx = mn;
        }
    }
    if (row < Lr) {
        const size_t o = (offr + row) * SK_NSPLIT + ch;
        a.part_new[o] = make_float2(mx, sum);
        if (GRAD) a.gpart[o * 3] = gx, a.gpart[o * 3 + 1] = gy, a.gpart[o * 3 + 2] = gz;
    }
}

struct SkFin {
    int b, n, m;
    const int *len1, *len2;
    const float *pot;    // the potentials the final soft-min read
    const float2 *part;  // the final soft-min's partials
    const float *gpart;  // or nullptr
    float k;             // eps[T - 1] ln 2
    float *loss, *potout, *delta, *grad1, *grad2;
};

// grid (b).  A thread takes the rows tid, tid + SK_FIN_TPB, ... of a cloud in ascending order; the sums are double: the
// threads of a wave by a butterfly, then the waves in order.
__global__ __launch_bounds__(SK_FIN_TPB) void sk_finish_kernel(SkFin a) {
    __shared__ double wsum[2][SK_FIN_TPB / 64];
    __shared__ float wmax[SK_FIN_TPB / 64];
    const int s = blockIdx.x, tid = threadIdx.x, n = a.n, m = a.m;
    const int L1 = rf::ragged_count(a.len1, s, n), L2 = rf::ragged_count(a.len2, s, m);
    const size_t R = 2 * ((size_t)n + m), base = (size_t)s * R;
    const bool grad = a.gpart != nullptr;
    double acc[2] = {0.0, 0.0};
    float dl = 0.f;
    for (int side = 0; side < 2; side++) {
        const int nr = side ? m : n, Lr = side ? L2 : L1, Lo = side ? L1 : L2;
        const size_t offc = base + sk_off(side, n, m), offs = base + sk_off(2 + side, n, m);
        const int nchc = sk_nch(Lo), nchs = sk_nch(Lr);  // cross: the other cloud's columns; self: the cloud's own
        const float wc = 1.0f / (float)Lo, ws = 1.0f / (float)Lr;
        float *__restrict__ po = a.potout + (size_t)s * ((size_t)n + m) + (side ? n : 0);
        float *__restrict__ go = grad ? (side ? a.grad2 + (size_t)s * m * 3 : a.grad1 + (size_t)s * n * 3) : nullptr;
        for (int i = tid; i < nr; i += SK_FIN_TPB) {
            float f1 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (i < Lr) {
                float Mc, Sc, Ms, Ss;
                if (grad) {
                    float cx, cy, cz, sx, sy, sz;
                    sk_fold_grad(a.part + (offc + i) * SK_NSPLIT, a.gpart + (offc + i) * SK_NSPLIT * 3, nchc, Mc, Sc, cx, cy, cz);
                    sk_fold_grad(a.part + (offs + i) * SK_NSPLIT, a.gpart + (offs + i) * SK_NSPLIT * 3, nchs, Ms, Ss, sx, sy, sz);
                    const float L = (float)Lr;
                    g0 = (cx / Sc - sx / Ss) / L, g1 = (cy / Sc - sy / Ss) / L, g2 = (cz / Sc - sz / Ss) / L;
                } else {
                    sk_fold(a.part + (offc + i) * SK_NSPLIT, nchc, Mc, Sc);
                    sk_fold(a.part + (offs + i) * SK_NSPLIT, nchs, Ms, Ss);
                }
                f1 = sk_softmin(Mc, Sc, wc, a.k);
                const float fs = sk_softmin(Ms, Ss, ws, a.k);
                acc[side] += (double)f1 - (double)fs;
                dl = fmaxf(dl, fabsf(f1 - a.pot[offc + i]));
            }
            po[i] = f1;
            if (grad) go[(size_t)i * 3] = g0, go[(size_t)i * 3 + 1] = g1, go[(size_t)i * 3 + 2] = g2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc[0] += __shfl_xor(acc[0], o, 64);
        acc[1] += __shfl_xor(acc[1], o, 64);
        dl = fmaxf(dl, __shfl_xor(dl, o, 64));
    }
    if ((tid & 63) == 0) wsum[0][tid >> 6] = acc[0], wsum[1][tid >> 6] = acc[1], wmax[tid >> 6] = dl;
    __syncthreads();
    if (tid == 0) {
        double t0 = wsum[0][0], t1 = wsum[1][0];
        float d = wmax[0];
        for (int w = 1; w < SK_FIN_TPB / 64; w++) t0 += wsum[0][w], t1 += wsum[1][w], d = fmaxf(d, wmax[w]);
        const double l = t0 / (double)L1 + t1 / (double)L2;
        a.loss[s] = (float)l;
        a.delta[s] = l != l ? (float)l : d;  // (fmaxf drops a NaN: a sample that is NaN says so here too)
    }
}

struct SkLayout {
    size_t pot[2], part[2], gpart, total;
};

// the potentials (two buffers of b rows f | g | fx | gy) | the (max, sum) partials of every (row, chunk), two buffers | the
// gradient numerators of the final soft-min
SkLayout sk_layout(int b, int n, int m) {
    const size_t rows = (size_t)b * 2 * ((size_t)n + (size_t)m);
    rf::Layout w;
    SkLayout l;
    for (size_t &o : l.pot) o = w.add(rows * sizeof(float));
    for (size_t &o : l.part) o = w.add(rows * SK_NSPLIT * sizeof(float2));
    l.gpart = w.add(rows * SK_NSPLIT * 3 * sizeof(float));
    l.total = w.total;
    return l;
}

bool sk_sizes_ok(int b, int n, int m) {
    return b >= 1 && b <= 65535 && n >= 1 && m >= 1 && n <= RF_SK_MAX_POINTS && m <= RF_SK_MAX_POINTS;
}

}  // namespace

extern "C" {

size_t rf_sinkhorn_workspace_bytes(int b, int n, int m) {
    if (!sk_sizes_ok(b, n, m)) return 0;
    return sk_layout(b, n, m).total;
}

int rf_sinkhorn(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, int p,
                const float *eps, int T, float *loss, float *pot, float *delta, float *grad1, float *grad2, void *workspace,
                size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!sk_sizes_ok(b, n, m)) return RF_EINVAL;
    if (p != 1 && p != 2) return RF_EINVAL;
    if (T < 1 || T > RF_SK_MAX_ITERS || !eps) return RF_EINVAL;
    for (int t = 0; t < T; t++)
        if (!(eps[t] > 0.f) || !isfinite(eps[t])) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, loss, pot, delta}, {grad1, grad2, len1, len2})) return RF_EINVAL;
    if ((grad1 == nullptr) != (grad2 == nullptr) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const SkLayout l = sk_layout(b, n, m);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    float *potb[2] = {(float *)(w + l.pot[0]), (float *)(w + l.pot[1])};
    float2 *partb[2] = {(float2 *)(w + l.part[0]), (float2 *)(w + l.part[1])};
    float *gpart = grad1 ? (float *)(w + l.gpart) : nullptr;

    const int big = n > m ? n : m;
    const dim3 grid(rf::ceil_div(big, SK_TPB) * SK_NSPLIT, b, 4);
    for (int t = 0; t <= T; t++) {  // sweep t reads the potentials after t updates; sweep T is the final soft-min
        const float e = eps[t < T ? t : T - 1], eprev = eps[t > 0 ? t - 1 : 0];
        const bool fin = t == T;
        const SkStep a{b,    n,    m,    t,
                       xyz1, xyz2, len1, len2,
                       potb[(t + 1) & 1], potb[t & 1], partb[(t + 1) & 1], partb[t & 1],
                       fin ? gpart : nullptr, (float)(SK_LOG2E / (double)e), (float)((double)eprev * SK_LN2)};
        if (fin && gpart && p == 1) {
            RF_LAUNCH("sinkhorn_final", (sk_sweep_kernel<1, true>), grid, dim3(SK_TPB), 0, st, a);
        } else if (fin && gpart) {
            RF_LAUNCH("sinkhorn_final", (sk_sweep_kernel<2, true>), grid, dim3(SK_TPB), 0, st, a);
        } else if (p == 1) {
            RF_LAUNCH("sinkhorn_sweep", (sk_sweep_kernel<1, false>), grid, dim3(SK_TPB), 0, st, a);
        } else {
            RF_LAUNCH("sinkhorn_sweep", (sk_sweep_kernel<2, false>), grid, dim3(SK_TPB), 0, st, a);
        }
    }
    const SkFin f{b,  n,  m,  len1, len2, potb[T & 1], partb[T & 1], gpart, (float)((double)eps[T - 1] * SK_LN2),
                  loss, pot, delta, grad1, grad2};
    RF_LAUNCH("sinkhorn_finish", sk_finish_kernel, dim3(b), dim3(SK_FIN_TPB), 0, st, f);
    return RF_OK;
}

}  // extern "C"
