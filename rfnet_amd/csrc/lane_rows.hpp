// lane_rows.hpp -- the skeleton of the gather-by-index kernels (grouping.hip, interpolate.hip, scatter_rows.hip,
// vector_attention.hip; point_voxel.hip takes the placement): a workgroup of TPB threads is cut into TY lane rows of
// TX = 1 << tx_log2 lanes; a lane row owns a slot, a query or a destination row, and its lanes walk the channels as floats or
// 4-wide vectors, `for (l = lx; l < c / VEC; l += TX)`; the workgroup first takes its logical place, so that a sample's
// workgroups share one XCD's L2.  Structure only: how many rows a lane row takes, how many loads it keeps in flight, the block
// size and which loads are non-temporal are tuned -- and commented with their measurements -- where the kernels are.
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace rf {

// ---- the channel vector: float, or four floats in one 16-byte load (operators per component, every product rounded)
typedef float v4f __attribute__((ext_vector_type(4)));
template <int VEC>
struct LaneVec;
template <>
struct LaneVec<4> {
    typedef v4f T;
};
template <>
struct LaneVec<1> {
    typedef float T;
};
__device__ __forceinline__ float lane_at(float v, int) { return v; }
__device__ __forceinline__ float lane_at(const v4f &v, int j) { return v[j]; }
__device__ __forceinline__ void lane_set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void lane_set(v4f &v, int j, float x) { v[j] = x; }

// ---- the geometry, device side: this thread's lane lx of lane row ly
template <int TPB>
struct LaneRows {
    int TX, TY, lx, ly;
    __device__ __forceinline__ explicit LaneRows(int tx_log2)
        : TX(1 << tx_log2), TY(TPB >> tx_log2), lx(threadIdx.x & (TX - 1)), ly(threadIdx.x >> tx_log2) {}
};

// ---- the geometry, host side
// lanes per row: the power of two that covers `lanes` channel vectors, a wave at most (wider rows take further passes)
inline int lane_rows_tx_log2(int lanes) {
    int t = 0;
    while ((1 << t) < lanes && t < 6) t++;
    return t;
}
// the vector path: whole vectors per row, and every tensor read or written as vectors 16-byte aligned (NULL: an absent tensor)
inline bool lane_rows_vec_ok(int c, std::initializer_list<const void *> ps) {
    if (c % 4 != 0) return false;
    for (const void *p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}

// ---- the workgroup's logical place (xcd_contiguous, common.hpp: a speed-up only, any mapping is correct)
// a grid of bpb * b workgroups -> sample bi, workgroup bx of the sample
template <class B>
__device__ __forceinline__ void place_1d(int bpb, B &bi, int &bx) {
    const unsigned logical = xcd_contiguous(blockIdx.x, gridDim.x);
    bi = logical / bpb;
    bx = logical - (int)bi * bpb;
}
// an (x, sample) grid.  xcd_contiguous works on 32-bit ids, and the entries' size checks alone do not keep x * b below 2^32
// (rf_voxelize_mean admits 32^3 sub-bricks x 128 chunks x 65535 samples; the slot rows of vector attention 2^20 x 65535), though
// no memory holds the tensors of such a grid.  GUARD: from 2^32 workgroups on the ids are taken as they are instead of a mapping
// that wrapped.  vector_attention.hip has it; point_voxel.hip never had it and stays without: given the guard, its
// voxelize_brick measured 0.7 to 1.4 % slower, outside the parent's noise at four of five shapes (profiles/lane_rows_ab.txt).
template <bool GUARD>
__device__ __forceinline__ void place_2d(int &x, int &s) {
    if constexpr (GUARD) {
        const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
        if (total >> 32) {
            x = (int)blockIdx.x, s = (int)blockIdx.y;
            return;
        }
        const unsigned pos = xcd_contiguous(blockIdx.y * gridDim.x + blockIdx.x, (unsigned)total);
        s = (int)(pos / gridDim.x), x = (int)(pos - (unsigned)s * gridDim.x);
    } else {
        const unsigned pos = xcd_contiguous(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
        s = (int)(pos / gridDim.x), x = (int)(pos - (unsigned)s * gridDim.x);
    }
}

}  // namespace rf
