// vector_attention.hip -- the two ops that the transformer-style completion networks (Point Transformer, SnowflakeNet's
// skip-transformer, PoinTr / AdaPoinTr, SeedFormer) run on their (b, m, k, c) neighbourhood tensors behind a kNN search:
//   neighbour subtraction   sub[i][t][:] = q[i][:] - src[idx[i][t]][:]
//   neighbour aggregation   out[i][ch]   = sum_t (value[idx[i][t]][ch] + pos[i][t][ch]) * weight[i][t][ch mod cw]
// both with gradients.  include/rfops.h states the contract, DESIGN.md 5.3p the layout and the measurements.
//
// Three kernel shapes, all of them lane rows over the channels (lane_rows.hpp has the geometry, the vector type and the placement):
//   slot rows    a lane row per slot (i, t): the subtraction, grad_pos, grad_weight (there the lanes run over the WEIGHT channels
//                and every lane walks the c / cw channel groups in ascending order: the prescribed order, coalesced loads);
//   query rows   a lane row per query i walking its slots in ascending t with double accumulators: the aggregation and grad_q;
//   source rows  a lane row per row r of the gathered tensor walking the slots that name it: grad_src and grad_value, over
//                rows_csr_sort_masked's row_start / perm (scatter_rows.hpp).  The sort applies the liveness rule, every row is
//                stored once, nothing of size (b, m, k, c) is formed for the aggregation: its terms come from grad_out[i][:] and
//                weight[i][t][:] on the fly.  No float atomics in memory and no memset anywhere.
// The streamed (b, m, k, c) tensors go by non-temporal loads and stores, the gathered rows by plain loads (they are what the L2
// holds), and rf::place_2d puts a sample's workgroups on one XCD.  A dead slot's operands are loaded from addresses that are the
// call's own (its own slot of pos / weight / grad_out, row 0 of the gathered tensor) and dropped by a SELECT, never by a product:
// a NaN there reaches nothing, and several loads stay in flight without a branch.
#include "common.hpp"
#include "lane_rows.hpp"
#include "scatter_rows.hpp"

namespace {

constexpr int VA_TPB = 256;
constexpr int VA_PP = 4;    // slot rows: slots per lane row
constexpr int VA_TQ = 4;    // query rows: slots of the query in flight
constexpr int VA_RPT = 2;   // source rows: rows per lane row (their chains run side by side) ...
constexpr int VA_Q = 4;     // ... and slots of each in flight
constexpr int VA_MAXK = RF_VA_MAX_K, VA_MAXC = RF_VA_MAX_CHANNELS;
static_assert(VA_MAXK == 64, "KN_MAXK (knn.hip): what rf_knn writes is what these entries take");

// the liveness rule of include/rfops.h, cb_key's of scatter_rows.hip: nv valid source rows, mv valid queries
struct VaLive {
    int nv, mv;
};
__device__ __forceinline__ bool va_live(const VaLive &L, int i, int t, int row) {
    return i < L.mv && t < L.nv && (unsigned)row < (unsigned)L.nv;
}

// where the weights of the channels ch0 ... ch0 + VEC - 1 sit in a weight row of cw floats.  WV: cw % 4 == 0, one vector load.
template <int VEC, bool WV>
struct VaWOff {
    int o[WV || VEC == 1 ? 1 : VEC];
};
template <int VEC, bool WV>
__device__ __forceinline__ VaWOff<VEC, WV> va_woff(int ch0, int cw) {
    VaWOff<VEC, WV> w;
    if constexpr (WV || VEC == 1) {
        w.o[0] = ch0 % cw;
    } else {
#pragma unroll
        for (int j = 0; j < VEC; j++) w.o[j] = (ch0 + j) % cw;
    }
    return w;
}
template <int VEC, bool WV>
__device__ __forceinline__ typename rf::LaneVec<VEC>::T va_wload(const float *__restrict__ row, const VaWOff<VEC, WV> &w) {
    typedef typename rf::LaneVec<VEC>::T V;
    if constexpr (WV || VEC == 1) {
        return __builtin_nontemporal_load((const V *)(row + w.o[0]));
    } else {
        V v;
#pragma unroll
        for (int j = 0; j < VEC; j++) rf::lane_set(v, j, __builtin_nontemporal_load(row + w.o[j]));
        return v;
    }
}

struct VaArgs {
    int n, m, k, c, cw;
    const int *idx, *len1, *len2;
    const float *q;       // (b, m, c): feat_q | grad_out of the aggregation
    const float *src;     // (b, n, c): feat_src | value
    const float *pos;     // (b, m, k, c) or NULL | grad_out of the subtraction
    const float *weight;  // (b, m, k, cw)
    float *out;
};

// ------------------------------------------------------------------------------------------------ slot rows
// The PP slots of a lane row: js = (bx PP + u) TY + ly, clamped into the sample as jc (a slot behind the last loads the last
// slot's operands and stores nothing), its query qi, whether it is live and the row it gathers (row 0 for a dead slot).
// One text for va_slot_kernel and va_gweight_kernel, from their bx, L, I, k and S; a macro, because round an inlined function the
// compiler places the kernels' address arithmetic elsewhere, and the code of seventeen tuned kernels is to stay what it is.
#define VA_SLOTS(PP, G)                                            \
    int js[PP], jc[PP], qi[PP], row[PP];                           \
    bool live[PP];                                                 \
    _Pragma("unroll") for (int u = 0; u < PP; u++) {               \
        js[u] = (bx * PP + u) * G.TY + G.ly;                       \
        jc[u] = min(js[u], S - 1);                                 \
        qi[u] = jc[u] / k;                                         \
        const int r = I[jc[u]];                                    \
        live[u] = va_live(L, qi[u], jc[u] - qi[u] * k, r);         \
        row[u] = live[u] ? r : 0;                                  \
    }

// What a lane row computes for its slot.  SUB: q - src.  GPOS: fl32(g * w).
enum { VA_SUB = 0, VA_GPOS = 1 };

// grid (ceil(m k / (TY VA_PP)), b)
template <int VEC, int OP, bool WV>
__global__ __launch_bounds__(VA_TPB) void va_slot_kernel(VaArgs a, int tx_log2) {
    typedef typename rf::LaneVec<VEC>::T V;
    int bx, s;
    rf::place_2d<true>(bx, s);
    const rf::LaneRows<VA_TPB> g(tx_log2);
    const int c = a.c, cv = c / VEC, k = a.k, S = a.m * k;
    const VaLive L{rf::ragged_count(a.len1, s, a.n), rf::ragged_count(a.len2, s, a.m)};
    const int *__restrict__ I = a.idx + (size_t)s * S;
    const V *__restrict__ Q = (const V *)(a.q + (size_t)s * a.m * c);
    const V *__restrict__ P = (const V *)(a.src + (size_t)s * a.n * c);
    const float *__restrict__ W = a.weight + (size_t)s * S * a.cw;
    V *__restrict__ O = (V *)(a.out + (size_t)s * S * c);
    VA_SLOTS(VA_PP, g)
    for (int l = g.lx; l < cv; l += g.TX) {
        V x[VA_PP], y[VA_PP];
        if constexpr (OP == VA_SUB) {
#pragma unroll
            for (int u = 0; u < VA_PP; u++) x[u] = Q[(size_t)qi[u] * cv + l], y[u] = P[(size_t)row[u] * cv + l];
        } else {
            const VaWOff<VEC, WV> wo = va_woff<VEC, WV>(l * VEC, a.cw);
#pragma unroll
            for (int u = 0; u < VA_PP; u++)
                x[u] = Q[(size_t)qi[u] * cv + l], y[u] = va_wload<VEC, WV>(W + (size_t)jc[u] * a.cw, wo);
        }
#pragma unroll
        for (int u = 0; u < VA_PP; u++) {
            if (js[u] >= S) continue;
            V o;
#pragma unroll
            for (int j = 0; j < VEC; j++) {
                const float xa = rf::lane_at(x[u], j), ya = rf::lane_at(y[u], j);
                rf::lane_set(o, j, live[u] ? (OP == VA_SUB ? xa - ya : xa * ya) : 0.f);
            }
            __builtin_nontemporal_store(o, &O[(size_t)js[u] * cv + l]);
        }
    }
}

// grad_weight (b, m, k, cw): the lanes of a slot's row run over the weight channels j (VEC of them each), and every lane walks the
// c / cw channel groups q ascending: sum_q (double)g[i][j + q cw] * (double)s[i][t][j + q cw], s = fl32(value + pos).
// A row's lanes read 4 cw contiguous bytes of the slot's row of pos per group.  With narrow weights that is a fraction of a cache
// line, and the line's other groups are wanted UQ - 1 steps later: taken one group at a time the lines left the L2 in between
// (0.203 ms at 32 x 2048 x 16, c = 64, cw = 8, whose pos is 268 MB).  So the loads of UQ groups -- a whole 128-byte line where
// 4 cw UQ = 128 -- are issued together, and the sums then take them in ascending order as before.  PP slots per lane row.
// grid (ceil(m k / (TY PP)), b)
template <int VEC, bool HAS_POS, int UQ, int PP>
__global__ __launch_bounds__(VA_TPB) void va_gweight_kernel(VaArgs a, int tx_log2) {
    typedef typename rf::LaneVec<VEC>::T V;
    int bx, s;
    rf::place_2d<true>(bx, s);
    const rf::LaneRows<VA_TPB> lr(tx_log2);
    const int c = a.c, cv = c / VEC, cwv = a.cw / VEC, groups = c / a.cw, k = a.k, S = a.m * k;
    const VaLive L{rf::ragged_count(a.len1, s, a.n), rf::ragged_count(a.len2, s, a.m)};
    const int *__restrict__ I = a.idx + (size_t)s * S;
    const V *__restrict__ G = (const V *)(a.q + (size_t)s * a.m * c);
    const V *__restrict__ P = (const V *)(a.src + (size_t)s * a.n * c);
    const V *__restrict__ E = HAS_POS ? (const V *)(a.pos + (size_t)s * S * c) : nullptr;
    V *__restrict__ O = (V *)(a.out + (size_t)s * S * a.cw);
    VA_SLOTS(PP, lr)
    for (int l = lr.lx; l < cwv; l += lr.TX) {
        double acc[PP][VEC];
#pragma unroll
        for (int u = 0; u < PP; u++)
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[u][j] = 0.0;
        for (int q0 = 0; q0 < groups; q0 += UQ) {
            V g[UQ][PP], v[UQ][PP], e[UQ][PP];
#pragma unroll
            for (int h = 0; h < UQ; h++) {
                const int off = min(q0 + h, groups - 1) * cwv + l;
#pragma unroll
                for (int u = 0; u < PP; u++) {
                    g[h][u] = G[(size_t)qi[u] * cv + off];
                    v[h][u] = P[(size_t)row[u] * cv + off];
                    if constexpr (HAS_POS) e[h][u] = __builtin_nontemporal_load(&E[(size_t)jc[u] * cv + off]);
                }
            }
#pragma unroll
            for (int h = 0; h < UQ; h++) {
                const bool in = q0 + h < groups;  // (a select, not a branch: the loads above stay one batch; + 0.0 changes no bit)
#pragma unroll
                for (int u = 0; u < PP; u++)
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        const float sv = HAS_POS ? rf::lane_at(v[h][u], j) + rf::lane_at(e[h][u], j) : rf::lane_at(v[h][u], j);
                        const double term = (double)rf::lane_at(g[h][u], j) * (double)sv;
                        acc[u][j] += in ? term : 0.0;
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < PP; u++) {
            if (js[u] >= S) continue;
            V o;
#pragma unroll
            for (int j = 0; j < VEC; j++) rf::lane_set(o, j, live[u] ? (float)acc[u][j] : 0.f);
            __builtin_nontemporal_store(o, &O[(size_t)js[u] * cwv + l]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ query rows
// A lane row per query walks its slots in ascending t; a dead slot adds +0.0, which changes no bit of a sum begun at +0.0.
// AGG: acc += (double)s * (double)w with s = fl32(value + pos) | value; otherwise (grad_q) acc += (double)grad_out[i][t][ch].
// grid (ceil(m / TY), b)
template <int VEC, bool AGG, bool HAS_POS, bool WV>
__global__ __launch_bounds__(VA_TPB) void va_query_kernel(VaArgs a, int tx_log2) {
    typedef typename rf::LaneVec<VEC>::T V;
    int bx, s;
    rf::place_2d<true>(bx, s);
    const rf::LaneRows<VA_TPB> g(tx_log2);
    const int i = bx * g.TY + g.ly;
    if (i >= a.m) return;
    const int c = a.c, cv = c / VEC, k = a.k;
    const VaLive L{rf::ragged_count(a.len1, s, a.n), rf::ragged_count(a.len2, s, a.m)};
    const int kk = i < L.mv ? min(k, L.nv) : 0;  // the slots t >= nv are dead: the loop's bound is a count
    const int *__restrict__ I = a.idx + ((size_t)s * a.m + i) * k;
    const V *__restrict__ P = (const V *)(a.src + (size_t)s * a.n * c);
    const V *__restrict__ E = (const V *)(a.pos + ((size_t)s * a.m + i) * k * c);  // (not formed into an address when pos is NULL)
    const float *__restrict__ W = a.weight + ((size_t)s * a.m + i) * k * a.cw;
    V *__restrict__ O = (V *)(a.out + ((size_t)s * a.m + i) * c);
    for (int l = g.lx; l < cv; l += g.TX) {
        VaWOff<VEC, WV> wo;
        if constexpr (AGG) wo = va_woff<VEC, WV>(l * VEC, a.cw);
        double acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) acc[j] = 0.0;
        for (int t0 = 0; t0 < kk; t0 += VA_TQ) {
            int tc[VA_TQ], row[VA_TQ];
            bool live[VA_TQ];
            V v[VA_TQ], e[VA_TQ], w[VA_TQ];
#pragma unroll
            for (int u = 0; u < VA_TQ; u++) {
                tc[u] = min(t0 + u, kk - 1);
                const int r = I[tc[u]];
                live[u] = t0 + u < kk && (unsigned)r < (unsigned)L.nv;
                row[u] = live[u] ? r : 0;
            }
#pragma unroll
            for (int u = 0; u < VA_TQ; u++) {
                if constexpr (AGG) {
                    v[u] = P[(size_t)row[u] * cv + l];
                    if constexpr (HAS_POS) e[u] = __builtin_nontemporal_load(&E[(size_t)tc[u] * cv + l]);
                    w[u] = va_wload<VEC, WV>(W + (size_t)tc[u] * a.cw, wo);
                } else {
                    e[u] = __builtin_nontemporal_load(&E[(size_t)tc[u] * cv + l]);
                }
            }
#pragma unroll
            for (int u = 0; u < VA_TQ; u++)
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    double term;
                    if constexpr (AGG) {
                        const float sv = HAS_POS ? rf::lane_at(v[u], j) + rf::lane_at(e[u], j) : rf::lane_at(v[u], j);
                        term = (double)sv * (double)rf::lane_at(w[u], j);
                    } else {
                        term = (double)rf::lane_at(e[u], j);
                    }
                    acc[j] += live[u] ? term : 0.0;
                }
        }
        V o;
#pragma unroll
        for (int j = 0; j < VEC; j++) rf::lane_set(o, j, (float)acc[j]);
        O[(size_t)l] = o;
    }
}

// ------------------------------------------------------------------------------------------------ source rows
struct VaGather {
    int n, k, c, cw, S;
    const float *g;       // grad_out: (b, m, k, c) of the subtraction | (b, m, c) of the aggregation
    const float *weight;  // (b, m, k, cw), the aggregation's
    const int *row_start, *perm;
    float *dst;  // (b, n, c)
};

// rows_csr_gather_kernel's walk with the terms of this file.  dst row r = the double sum, from +0.0, over the slots p of the row's
// list of   -(double)g[p][ch]   (the subtraction: a sum of negated terms, so that an exact zero is +0.0 like an empty row)   or
// (double)g[p / k][ch] * (double)weight[p][ch mod cw]   (the aggregation; the product is exact).  Every row is stored once.
// grid (ceil(n / (TY VA_RPT)), b)
template <int VEC, bool AGG, bool WV>
__global__ __launch_bounds__(VA_TPB) void va_rows_kernel(VaGather a, int tx_log2) {
    typedef typename rf::LaneVec<VEC>::T V;
    int bx, s;
    rf::place_2d<true>(bx, s);
    const rf::LaneRows<VA_TPB> g(tx_log2);
    const int n = a.n, c = a.c, cv = c / VEC, k = a.k, S = a.S;
    const int *__restrict__ RS = a.row_start + (size_t)s * (n + 1);
    const int *__restrict__ P = a.perm + (size_t)s * S;
    const V *__restrict__ G = (const V *)(a.g + (size_t)s * (AGG ? S / k : S) * c);
    const float *__restrict__ W = AGG ? a.weight + (size_t)s * S * a.cw : nullptr;
    V *__restrict__ O = (V *)(a.dst + (size_t)s * n * c);
    int r[VA_RPT], beg[VA_RPT], end[VA_RPT];
#pragma unroll
    for (int u = 0; u < VA_RPT; u++) {
        r[u] = (bx * VA_RPT + u) * g.TY + g.ly;
        const int rr = min(r[u], n - 1);
        beg[u] = RS[rr];
        end[u] = r[u] < n ? RS[rr + 1] : beg[u];
    }
    for (int l = g.lx; l < cv; l += g.TX) {
        VaWOff<VEC, WV> wo;
        if constexpr (AGG) wo = va_woff<VEC, WV>(l * VEC, a.cw);
        double acc[VA_RPT][VEC];
#pragma unroll
        for (int u = 0; u < VA_RPT; u++)
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[u][j] = 0.0;
        int p[VA_RPT];
#pragma unroll
        for (int u = 0; u < VA_RPT; u++) p[u] = beg[u];
        while (true) {
            bool any = false;
#pragma unroll
            for (int u = 0; u < VA_RPT; u++) any = any || p[u] < end[u];
            if (!any) break;
            int sl[VA_RPT][VA_Q];
            V v[VA_RPT][VA_Q], w[VA_RPT][VA_Q];
#pragma unroll
            for (int u = 0; u < VA_RPT; u++)
#pragma unroll
                for (int q = 0; q < VA_Q; q++) sl[u][q] = p[u] + q < end[u] ? P[p[u] + q] : -1;
#pragma unroll
            for (int u = 0; u < VA_RPT; u++)
#pragma unroll
                for (int q = 0; q < VA_Q; q++) {
                    const int ss = max(sl[u][q], 0);  // (a slot of the list is below S: the sort wrote it)
                    if constexpr (AGG) {
                        v[u][q] = G[(size_t)(ss / k) * cv + l];
                        w[u][q] = va_wload<VEC, WV>(W + (size_t)ss * a.cw, wo);
                    } else {
                        v[u][q] = __builtin_nontemporal_load(&G[(size_t)ss * cv + l]);
                    }
                }
#pragma unroll
            for (int u = 0; u < VA_RPT; u++)
#pragma unroll
                for (int q = 0; q < VA_Q; q++)
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        double term;
                        if constexpr (AGG) {
                            term = (double)rf::lane_at(v[u][q], j) * (double)rf::lane_at(w[u][q], j);
                        } else {
                            term = -(double)rf::lane_at(v[u][q], j);
                        }
                        acc[u][j] += sl[u][q] < 0 ? 0.0 : term;
                    }
#pragma unroll
            for (int u = 0; u < VA_RPT; u++) p[u] += VA_Q;
        }
#pragma unroll
        for (int u = 0; u < VA_RPT; u++) {
            if (r[u] >= n) continue;
            V o;
#pragma unroll
            for (int j = 0; j < VEC; j++) rf::lane_set(o, j, (float)acc[u][j]);
            __builtin_nontemporal_store(o, &O[(size_t)r[u] * cv + l]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the host side
bool va_sizes_ok(int b, int n, int m, int k) {
    return b >= 1 && b <= 65535 && n >= 1 && n <= 65536 && m >= 1 && m <= 65536 && k >= 1 && k <= VA_MAXK;
}
bool va_channels_ok(int n, int m, int k, int c, int cw) {
    return c >= 1 && c <= VA_MAXC && cw >= 1 && c % cw == 0 && (long)m * k * c < (1L << 31) && (long)n * c < (1L << 31);
}

// the sort by source row and the gather over it
template <bool AGG>
int va_rows(int b, int n, int m, int k, int c, int cw, const float *g, const float *weight, const int *idx, const int *len1,
            const int *len2, float *dst, void *workspace, const char *sort_name, const char *rows_name, hipStream_t st) {
    if (int e = rfs::rows_csr_sort_masked(b, n, m, k, idx, len1, len2, workspace, sort_name, st)) return e;
    const bool vec = rf::lane_rows_vec_ok(c, {g, dst});
    const bool wv = vec && rf::lane_rows_vec_ok(cw, {weight});
    const int tx = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const dim3 grid(rf::ceil_div(n, (VA_TPB >> tx) * VA_RPT), b);
    const VaGather a{n, k, c, cw, m * k, g, weight, (const int *)workspace, rfs::rows_csr_perm(b, n, workspace), dst};
    if (!vec) {
        RF_LAUNCH(rows_name, (va_rows_kernel<1, AGG, false>), grid, dim3(VA_TPB), 0, st, a, tx);
    } else if (AGG && wv) {
        RF_LAUNCH(rows_name, (va_rows_kernel<4, AGG, true>), grid, dim3(VA_TPB), 0, st, a, tx);
    } else {
        RF_LAUNCH(rows_name, (va_rows_kernel<4, AGG, false>), grid, dim3(VA_TPB), 0, st, a, tx);
    }
    return RF_OK;
}

}  // namespace

extern "C" {

size_t rf_neighbor_sub_grad_workspace_bytes(int b, int n, int m, int k) {
    if (!va_sizes_ok(b, n, m, k)) return 0;
    return rfs::rows_csr_workspace_bytes(b, n, (long)m * k);
}

size_t rf_neighbor_aggregate_grad_workspace_bytes(int b, int n, int m, int k) {
    return rf_neighbor_sub_grad_workspace_bytes(b, n, m, k);
}

int rf_neighbor_sub(int b, int n, int m, int k, int c, const float *feat_q, const float *feat_src, const int *idx, const int *len1,
                    const int *len2, float *out, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || k < 0 || c < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!va_sizes_ok(b, n, m, k) || !va_channels_ok(n, m, k, c, 1)) return RF_EINVAL;
    if (!rf::tensors_ok({feat_q, feat_src, idx, out}, {len1, len2})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = rf::lane_rows_vec_ok(c, {feat_q, feat_src, out});
    const int tx = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const dim3 grid(rf::ceil_div((long)m * k, (VA_TPB >> tx) * VA_PP), b);
    const VaArgs a{n, m, k, c, 1, idx, len1, len2, feat_q, feat_src, nullptr, nullptr, out};
    if (vec) {
        RF_LAUNCH("neighbor_sub", (va_slot_kernel<4, VA_SUB, false>), grid, dim3(VA_TPB), 0, st, a, tx);
    } else {
        RF_LAUNCH("neighbor_sub", (va_slot_kernel<1, VA_SUB, false>), grid, dim3(VA_TPB), 0, st, a, tx);
    }
    return RF_OK;
}

int rf_neighbor_sub_grad(int b, int n, int m, int k, int c, const int *idx, const int *len1, const int *len2, const float *grad_out,
                         float *grad_q, float *grad_src, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || k < 0 || c < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!va_sizes_ok(b, n, m, k) || !va_channels_ok(n, m, k, c, 1)) return RF_EINVAL;
    // (grad_q and grad_src may be NULL: what is NULL is not computed)
    if (!rf::tensors_ok({idx, grad_out}, {len1, len2, grad_q, grad_src})) return RF_EINVAL;
    if (grad_src) {
        if (!rf::workspace_ok(workspace)) return RF_EINVAL;
        if (workspace_bytes < rf_neighbor_sub_grad_workspace_bytes(b, n, m, k)) return RF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (grad_q) {
        const bool vec = rf::lane_rows_vec_ok(c, {grad_out, grad_q});
        const int tx = rf::lane_rows_tx_log2(vec ? c / 4 : c);
        const dim3 grid(rf::ceil_div(m, VA_TPB >> tx), b);
        const VaArgs a{n, m, k, c, 1, idx, len1, len2, nullptr, nullptr, grad_out, nullptr, grad_q};
        if (vec) {
            RF_LAUNCH("neighbor_sub_grad_q", (va_query_kernel<4, false, true, false>), grid, dim3(VA_TPB), 0, st, a, tx);
        } else {
            RF_LAUNCH("neighbor_sub_grad_q", (va_query_kernel<1, false, true, false>), grid, dim3(VA_TPB), 0, st, a, tx);
        }
    }
    if (grad_src)
        return va_rows<false>(b, n, m, k, c, 1, grad_out, nullptr, idx, len1, len2, grad_src, workspace, "neighbor_sub_grad_sort",
                              "neighbor_sub_grad_rows", st);
    return RF_OK;
}

int rf_neighbor_aggregate(int b, int n, int m, int k, int c, int cw, const float *value, const float *pos, const float *weight,
                          const int *idx, const int *len1, const int *len2, float *out, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || k < 0 || c < 0 || cw < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!va_sizes_ok(b, n, m, k) || !va_channels_ok(n, m, k, c, cw)) return RF_EINVAL;
    // (pos may be NULL: the values are then taken as they are)
    if (!rf::tensors_ok({value, weight, idx, out}, {pos, len1, len2})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = rf::lane_rows_vec_ok(c, {value, pos, out});
    const bool wv = vec && rf::lane_rows_vec_ok(cw, {weight});
    const int tx = rf::lane_rows_tx_log2(vec ? c / 4 : c);
    const dim3 grid(rf::ceil_div(m, VA_TPB >> tx), b);
    const VaArgs a{n, m, k, c, cw, idx, len1, len2, nullptr, value, pos, weight, out};
#define VA_GO(VEC, POS, WV) RF_LAUNCH("neighbor_agg", (va_query_kernel<VEC, true, POS, WV>), grid, dim3(VA_TPB), 0, st, a, tx)
    if (pos) {
        if (!vec) { VA_GO(1, true, false); } else if (wv) { VA_GO(4, true, true); } else { VA_GO(4, true, false); }
    } else {
        if (!vec) { VA_GO(1, false, false); } else if (wv) { VA_GO(4, false, true); } else { VA_GO(4, false, false); }
    }
#undef VA_GO
    return RF_OK;
}

int rf_neighbor_aggregate_grad(int b, int n, int m, int k, int c, int cw, const float *value, const float *pos, const float *weight,
                               const int *idx, const int *len1, const int *len2, const float *grad_out, float *grad_value,
                               float *grad_pos, float *grad_weight, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || k < 0 || c < 0 || cw < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!va_sizes_ok(b, n, m, k) || !va_channels_ok(n, m, k, c, cw)) return RF_EINVAL;
    // (pos and each of the three outputs may be NULL)
    if (!rf::tensors_ok({value, weight, idx, grad_out}, {pos, len1, len2, grad_value, grad_pos, grad_weight})) return RF_EINVAL;
    if (grad_value) {
        if (!rf::workspace_ok(workspace)) return RF_EINVAL;
        if (workspace_bytes < rf_neighbor_aggregate_grad_workspace_bytes(b, n, m, k)) return RF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (grad_pos) {
        const bool vec = rf::lane_rows_vec_ok(c, {grad_out, grad_pos});
        const bool wv = vec && rf::lane_rows_vec_ok(cw, {weight});
        const int tx = rf::lane_rows_tx_log2(vec ? c / 4 : c);
        const dim3 grid(rf::ceil_div((long)m * k, (VA_TPB >> tx) * VA_PP), b);
        const VaArgs a{n, m, k, c, cw, idx, len1, len2, grad_out, nullptr, nullptr, weight, grad_pos};
        if (!vec) {
            RF_LAUNCH("neighbor_agg_grad_pos", (va_slot_kernel<1, VA_GPOS, false>), grid, dim3(VA_TPB), 0, st, a, tx);
        } else if (wv) {
            RF_LAUNCH("neighbor_agg_grad_pos", (va_slot_kernel<4, VA_GPOS, true>), grid, dim3(VA_TPB), 0, st, a, tx);
        } else {
            RF_LAUNCH("neighbor_agg_grad_pos", (va_slot_kernel<4, VA_GPOS, false>), grid, dim3(VA_TPB), 0, st, a, tx);
        }
    }
    if (grad_weight) {
        const bool vec = rf::lane_rows_vec_ok(cw, {grad_out, value, pos, grad_weight});
        const int tx = rf::lane_rows_tx_log2(vec ? cw / 4 : cw);
        const int uq = cw <= 4 ? 8 : (cw <= 8 ? 4 : (cw <= 16 ? 2 : 1));  // groups per 128-byte line, at most 8
        const int pp = uq == 8 ? 1 : 2;
        const dim3 grid(rf::ceil_div((long)m * k, (VA_TPB >> tx) * pp), b);
        const VaArgs a{n, m, k, c, cw, idx, len1, len2, grad_out, value, pos, nullptr, grad_weight};
#define VA_GO(VEC, POS, UQ, PP) \
    RF_LAUNCH("neighbor_agg_grad_weight", (va_gweight_kernel<VEC, POS, UQ, PP>), grid, dim3(VA_TPB), 0, st, a, tx)
#define VA_GO_UQ(VEC, POS)                         \
    do {                                           \
        if (uq == 8) { VA_GO(VEC, POS, 8, 1); }    \
        else if (uq == 4) { VA_GO(VEC, POS, 4, 2); } \
        else if (uq == 2) { VA_GO(VEC, POS, 2, 2); } \
        else { VA_GO(VEC, POS, 1, 2); }            \
    } while (0)
        if (pos) {
            if (vec) { VA_GO_UQ(4, true); } else { VA_GO_UQ(1, true); }
        } else {
            if (vec) { VA_GO_UQ(4, false); } else { VA_GO_UQ(1, false); }
        }
#undef VA_GO_UQ
#undef VA_GO
    }
    if (grad_value)
        return va_rows<true>(b, n, m, k, c, cw, grad_out, weight, idx, len1, len2, grad_value, workspace, "neighbor_agg_grad_sort",
                             "neighbor_agg_grad_rows", st);
    return RF_OK;
}

}  // extern "C"
