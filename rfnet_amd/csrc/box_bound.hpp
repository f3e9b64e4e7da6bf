// box_bound.hpp -- the k-nearest search shared by three_nn (interpolate.hip) and knn_point (knn.hip): the scalar candidate
// stream of their scans, and the boxed walk over sorted clouds with the point/box bound it tests (its wave minimum / maximum
// are rf::wave_min_f32 / rf::wave_max_f32, wave.hpp).  Each op brings its own candidate list (TnList, KnList), so the walk and
// the stream exist once.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace {

// squared distance from a point (or, with plo != phi, a box) to a box, per axis the gap max(lo - phi, plo - hi, 0): the
// unfused expression of the op itself, so that bound <= d in fp32 (below).  An empty box (lo = +inf, hi = -inf) is at +inf.
__device__ __forceinline__ float tb_gap(float a, float b) { return fmaxf(fmaxf(a, b), 0.f); }
__device__ __forceinline__ float tb_bound(float lx, float ly, float lz, float hx, float hy, float hz, float pxl, float pyl,
                                          float pzl, float pxh, float pyh, float pzh) {
    const float gx = tb_gap(lx - pxh, pxl - hx), gy = tb_gap(ly - pyh, pyl - hy), gz = tb_gap(lz - pzh, pzl - hz);
    return (gx * gx + gy * gy) + gz * gz;
}

// ---- the scans: one lane per query, every candidate ------------------------------------------------------------------------
// The candidate set is wave-uniform, so it is streamed through SGPRs by scalar loads (two register sets of TS_SUB candidates
// used alternately, as query_ball_lanes_kernel: the next set is on its way while this one is compared) and the VALU ops take
// the SGPR operands directly -- no LDS tile, no barrier.  consider(x, y, z, i) sees every candidate of C[0, n) in index order;
// it is inlined into the unrolled sets, so what it updates stays in registers as long as it indexes its list with constants.
constexpr int TS_SUB = 8;  // candidates per scalar-load set

template <class F>
__device__ __forceinline__ void ts_stream(const float *__restrict__ C, int n, F &consider) {
    const int n_full = (n / TS_SUB) * TS_SUB;
    if (n_full > 0) {
        float pa[3 * TS_SUB], pb[3 * TS_SUB];
        auto fetch = [&](float (&dst)[3 * TS_SUB], int c0) {
            const float *cp = C + (size_t)min(c0, n - TS_SUB) * 3;  // uniform -> s_load; clamped in bounds
#pragma unroll
            for (int i = 0; i < 3 * TS_SUB; i++) dst[i] = cp[i];
        };
#define TS_SCAN8(c, c0) \
    _Pragma("unroll") for (int u = 0; u < TS_SUB; u++) consider(c[u * 3], c[u * 3 + 1], c[u * 3 + 2], (c0) + u)
        fetch(pa, 0);
        for (int c0 = 0; c0 < n_full; c0 += 2 * TS_SUB) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): pa has arrived
            __builtin_amdgcn_sched_barrier(0);
            fetch(pb, c0 + TS_SUB);
            __builtin_amdgcn_sched_barrier(0);
            TS_SCAN8(pa, c0);
            if (c0 + TS_SUB >= n_full) break;
            __builtin_amdgcn_s_waitcnt(0xC07F);  // pb has arrived
            __builtin_amdgcn_sched_barrier(0);
            fetch(pa, c0 + 2 * TS_SUB);
            __builtin_amdgcn_sched_barrier(0);
            TS_SCAN8(pb, c0 + TS_SUB);
        }
#undef TS_SCAN8
    }
#pragma unroll 1
    for (int c = n_full; c < n; c++) consider(C[c * 3], C[c * 3 + 1], C[c * 3 + 2], c);
}

// ---- the boxed walk: both sets sorted, a wave of 64 neighbouring queries, the candidate blocks that can still matter --------
// Both sets in the spatial order of the Chamfer sweep's sort (nn_pruned.hip: 64-record superblocks and 16-record blocks with
// their boxes).  A wave takes 64 consecutive sorted queries -- a compact cell, one superblock of their set -- and visits only the
// candidate blocks whose box can still hold a point at or inside some lane's pruning distance (its k-th best), nearest
// superblock first.  The bound is the SAME unfused fp32 expression as the distance, evaluated on the per-axis gaps to the box:
// rounding is monotone, so bound <= distance holds in fp32 exactly and nothing that the scan would insert is skipped.  Visits
// go in any order, so a list ranks candidates by the 64-bit key (distance bits, index), which settles ties as the scan's index
// order does: the result is the scan's, bit for bit.
//
// The list is a policy of the op (TnList in interpolate.hip, KnList in knn.hip), which states what follows from its semantics:
//   kNonFinite        whether a non-finite distance can ever enter the list.  If it can, the walk visits superblocks whose bound
//                     is +inf, and a wave with q.full set visits every superblock without a test (non-finite values break the
//                     bounds: the sort leaves such points out of the boxes);
//   prune()           the lane's pruning distance; in a lane that does not search, one that no bound is <=;
//   admit(d)          the float pre-test of a distance, behind a wave-uniform branch;
//   insert(d, oi, in) the exact insertion by key, run by the whole wave when some lane admits (in: this lane's pre-test).
#ifndef RFI_TB_WAVES
#define RFI_TB_WAVES 4
#endif
constexpr int TB_WAVES = RFI_TB_WAVES;  // waves per workgroup, each on its own (no barrier)

// The sample bi and the superblock `group` of its sorted queries that this wave takes; a sample's workgroups on the XCD that
// sorted it (rf::xcd_contiguous, as nnp_sort): its records are still in that L2.  group * 64 >= npq: a wave past the end.
struct TbPlace {
    int bi, group;
};
__device__ __forceinline__ TbPlace tb_place(int npq) {
    const int bpb = ((npq >> 6) + TB_WAVES - 1) / TB_WAVES;  // workgroups per sample
    const unsigned logical = rf::xcd_contiguous(blockIdx.x, gridDim.x);
    const int bi = logical / bpb;
    return {bi, (int)(logical - bi * bpb) * TB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)};
}

// the lane's query and its wave's box (qb: lo xyz, -, hi xyz of the wave's superblock)
struct TbQuery {
    float x, y, z;
    bool search;  // the lane takes part (a padding record, or for three_nn a non-finite point, does not)
    bool full;    // (uniform) visit every superblock without a test (lists with kNonFinite only)
    const float *qb;
};
// one sample's sorted candidate set
struct TbCands {
    const float *xyz;
    const int *orig;
    const float *b16, *b64;
    int nsb;  // superblocks
};
// -DTB_STATS: the walk counts its superblock visits and 16-record block scans (uniform); the kernels write them into idx
struct TbStats {
    int visits = 0, scans = 0;
};

template <class List>
__device__ __forceinline__ void tb_walk(List &L, const TbQuery &q, const TbCands &c, TbStats &st) {
    const int lane = threadIdx.x & 63;
    // One candidate (uniform coordinates and original index, through scalar registers).  A padding record (index -1, coordinates
    // +inf) never enters: both lists key it above everything.
#define TB_CONSIDER(cx, cy, cz, oi)                                                   \
    {                                                                                 \
        const float dx_ = (cx) - q.x, dy_ = (cy) - q.y, dz_ = (cz) - q.z;              \
        const float xx_ = dx_ * dx_, yy_ = dy_ * dy_, zz_ = dz_ * dz_;                 \
        const float d_ = (xx_ + yy_) + zz_;                                            \
        const bool in_ = L.admit(d_);                                                  \
        if (__ballot(in_) != 0ull) { /* wave-uniform */                                \
            asm volatile("; some lane may insert"); /* keeps this a real branch */     \
            L.insert(d_, (oi), in_);                                                   \
        }                                                                             \
    }
    // one superblock: per 16-record block the lanes' bounds against their pruning distances (test), then the records of the
    // blocks some lane needs, eight at a time through two scalar register sets in turn (the next eight are on their way while
    // these are compared)
    auto visit = [&](int sb, bool test) {
#ifdef TB_STATS
        st.visits++;
#endif
        unsigned hm = 0xFFu;  // the half-blocks to scan
        if (test) {
            const float *bx = c.b16 + (size_t)sb * 24;  // (uniform -> scalar loads)
            float bb[24];
#pragma unroll
            for (int i = 0; i < 24; i++) bb[i] = bx[i];
            hm = 0u;
            const float pr = L.prune();
#pragma unroll
            for (int blk = 0; blk < 4; blk++) {
                const float lb = tb_bound(bb[blk * 6], bb[blk * 6 + 1], bb[blk * 6 + 2], bb[blk * 6 + 3], bb[blk * 6 + 4],
                                          bb[blk * 6 + 5], q.x, q.y, q.z, q.x, q.y, q.z);
                if (__ballot(lb <= pr) != 0ull) hm |= 3u << (2 * blk);  // (uniform)
            }
            if (hm == 0u) return;
        }
#ifdef TB_STATS
        st.scans += __builtin_popcount(hm) >> 1;
#endif
        const float *cb = c.xyz + (size_t)sb * 192;
        const int *ob = c.orig + sb * 64;
        float ca[24], cc[24];
        int oa[8], oc[8];
#define TB_FETCH(CC, O, H)                                              \
    {                                                                   \
        const float *cp_ = cb + (H) * 24;                               \
        const int *op_ = ob + (H) * 8;                                  \
        _Pragma("unroll") for (int i = 0; i < 24; i++) CC[i] = cp_[i];  \
        _Pragma("unroll") for (int i = 0; i < 8; i++) O[i] = op_[i];    \
    }
#define TB_SCAN8(CC, O) _Pragma("unroll") for (int u = 0; u < 8; u++) TB_CONSIDER(CC[u * 3], CC[u * 3 + 1], CC[u * 3 + 2], O[u])
        int h = __builtin_ctz(hm);
        hm &= hm - 1u;
        TB_FETCH(ca, oa, h);
        for (;;) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): set a has arrived
            __builtin_amdgcn_sched_barrier(0);
            const bool more_b = hm != 0u;
            if (more_b) {
                h = __builtin_ctz(hm);
                hm &= hm - 1u;
                TB_FETCH(cc, oc, h);
            }
            __builtin_amdgcn_sched_barrier(0);
            TB_SCAN8(ca, oa);
            if (!more_b) break;
            __builtin_amdgcn_s_waitcnt(0xC07F);  // set c has arrived
            __builtin_amdgcn_sched_barrier(0);
            const bool more_a = hm != 0u;
            if (more_a) {
                h = __builtin_ctz(hm);
                hm &= hm - 1u;
                TB_FETCH(ca, oa, h);
            }
            __builtin_amdgcn_sched_barrier(0);
            TB_SCAN8(cc, oc);
            if (!more_a) break;
        }
#undef TB_SCAN8
#undef TB_FETCH
    };
#undef TB_CONSIDER

    if (__ballot(q.search) == 0ull) return;  // (uniform) no lane to search for
    if (List::kNonFinite && q.full) {
        for (int sb = 0; sb < c.nsb; sb++) visit(sb, false);
        return;
    }
    const float qlx = q.qb[0], qly = q.qb[1], qlz = q.qb[2], qhx = q.qb[4], qhy = q.qb[5], qhz = q.qb[6];
    // 1. lanes <-> candidate superblocks: the one nearest to the wave's box goes first and fills the lists
    float best = INFINITY;
    int arg = 0;
    for (int r0 = 0; r0 < c.nsb; r0 += 64) {
        const int g = r0 + lane;
        float lb = INFINITY;
        if (g < c.nsb) {
            const float4 lo = *(const float4 *)(c.b64 + (size_t)g * 8), hi = *(const float4 *)(c.b64 + (size_t)g * 8 + 4);
            lb = tb_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
        }
        if (lb < best) best = lb, arg = g;
    }
    const float wmin = rf::wave_min_f32(best);
    const unsigned long long at = __ballot(best == wmin);
    const int seed = at != 0ull ? __builtin_amdgcn_readlane(arg, __builtin_ctzll(at)) : 0;
    visit(seed, false);
    // 2. every other superblock whose box is not beyond the wave's largest pruning distance (which shrinks as the visits go),
    //    64 superblocks at a time, nearest box first: the pruning distances shrink fastest that way, and the first box beyond
    //    the wave's largest ends the round.  (Where a lane's pruning distance is +inf, no finite bound is skipped.)
    float wk = rf::wave_max_f32(L.prune());
    for (int r0 = 0; r0 < c.nsb; r0 += 64) {
        const int g = r0 + lane;
        float lb = INFINITY;
        if (g < c.nsb && g != seed) {
            const float4 lo = *(const float4 *)(c.b64 + (size_t)g * 8), hi = *(const float4 *)(c.b64 + (size_t)g * 8 + 4);
            lb = tb_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
        }
        bool pend = g < c.nsb && g != seed && lb <= wk && (List::kNonFinite || lb != INFINITY);
        while (__ballot(pend) != 0ull) {  // (uniform)
            const float wmin2 = rf::wave_min_f32(pend ? lb : INFINITY);
            if (!(wmin2 <= wk)) break;
            const int jn = __builtin_ctzll(__ballot(pend && lb == wmin2));
            pend = pend && lane != jn;
            visit(r0 + jn, true);
            wk = rf::wave_max_f32(L.prune());
        }
    }
}

}  // namespace
