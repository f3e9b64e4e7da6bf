// wave.hpp -- the device helpers that every operator file of librfops.so needs, each of them ONCE: the ragged count, the
// 256-byte alignment of workspace sections, and the reductions / scans over a wave of 64 lanes.  Included by common.hpp.
// What is NOT here on purpose: the fused six-chain box reductions of nn_pruned.hip, wave_max_u64 and the v_max3 combine of
// sampling.hip, the reduce-scatter of nn_distance.hip, the bid trees of auction.hip and the shuffle loops inside the hot
// kernels of approxmatch.hip / nn_pruned.hip -- each is tuned to the one kernel it lives in.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rf {

// ---- ragged batches (the _lengths entries of include/rfops.h) ----
// A ragged batch's count of batch element bi (NULL = all n), clamped into [1, n]: the rule of include/rfops.h for every _lengths
// entry, so that no kernel reads past its tensor whatever the caller's lengths hold (the sort of nn_pruned.hip is given the same
// array and applies the same rule).  bi is uniform over a wave wherever this is called, so the load is scalar.
__device__ __forceinline__ int ragged_count(const int *__restrict__ len, int bi, int n) {
    if (!len) return n;
    const int v = len[bi];
    return v < 1 ? 1 : (v > n ? n : v);
}

// Sections of a workspace start at multiples of 256 bytes (boundary.hpp: workspace_ok, Layout).
__host__ __device__ inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// running minimum as ONE v_min3_f32.  Written as asm so that LLVM cannot re-associate the chain
// of minima over a chunk into a tree evaluated at the end of the chunk (minnum is exactly
// associative, so it does -- and then keeps all the distances of the chunk alive: spills).
__device__ __forceinline__ float min3_acc(float acc, float a, float b) {
    asm("v_min3_f32 %0, %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
    return acc;
}

// ---- xor butterflies: every lane ends with the result.  Offsets 32, 16, .., 1 in THAT order: float and double sums depend on it.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- DPP row steps: v = OP(v, v rotated by N lanes inside each row of 16 lanes), as the ONE instruction it is.  hipcc expands
// a float DPP reduction step written with builtins into mov / nop / mov_dpp / max / max (and wraps fminf / fmaxf in canonicalising
// v_max x, x).  The s_nop covers the VALU-write -> DPP-read hazard: neither the assembler nor the hazard recogniser looks inside
// asm.  Inputs of the float forms must not be NaN.  This is the form for a serial chain (FPS, the sort's boxes, the boxed walks);
// it is not faster everywhere: chamfer_cross.hip keeps a builtin form of its own (profiles/wave_primitives_ab.txt).
#define RF_DPP_ROW(OP, N) asm volatile("s_nop 1\n\t" OP " %0, %0, %0 row_ror:" #N " row_mask:0xf bank_mask:0xf" : "+v"(v))
#define RF_DPP_ROW4(OP) \
    RF_DPP_ROW(OP, 8);  \
    RF_DPP_ROW(OP, 4);  \
    RF_DPP_ROW(OP, 2);  \
    RF_DPP_ROW(OP, 1)
// every lane of a row ends with the row's result
__device__ __forceinline__ float row_allmax(float v) {
    RF_DPP_ROW4("v_max_f32_dpp");
    return v;
}
__device__ __forceinline__ float row_allmin(float v) {
    RF_DPP_ROW4("v_min_f32_dpp");
    return v;
}
__device__ __forceinline__ unsigned row_allmin_u(unsigned v) {
    RF_DPP_ROW4("v_min_u32_dpp");
    return v;
}
__device__ __forceinline__ unsigned row_allmax_u(unsigned v) {
    RF_DPP_ROW4("v_max_u32_dpp");
    return v;
}
#undef RF_DPP_ROW4
#undef RF_DPP_ROW

// uniform minimum / maximum over the wave: the row all-reduce, then the four row results through scalar registers
__device__ __forceinline__ float wave_min_f32(float v) {  // inputs not NaN
    v = row_allmin(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
__device__ __forceinline__ float wave_max_f32(float v) {  // inputs not NaN
    v = row_allmax(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = row_allmin_u(v);
    const unsigned r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const unsigned r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return min(min(r0, r1), min(r2, r3));
}
// maximum of floats that are +-inf or non-negative, never NaN: non-negative floats order as integers
__device__ __forceinline__ float wave_max_nonneg(float f) {
    // -inf (lanes that do not take part) maps to 0, which never exceeds a participant's value
    unsigned v = row_allmax_u(f < 0.f ? 0u : __float_as_uint(f));
    const unsigned r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const unsigned r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return __uint_as_float(max(max(r0, r1), max(r2, r3)));
}

// The same shape written with the DPP builtin, which the compiler may schedule and fold (off the serial chains, where the
// instruction count of a step does not matter): uniform sum (it must fit 32 bits) and uniform unsigned maximum.
__device__ __forceinline__ unsigned wave_add_u32(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);  // row_ror:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);  // row_ror:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);  // row_ror:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);  // row_ror:1
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}

// inclusive prefix sum over the wave in 6 DPP steps (row shifts, then the two row broadcasts)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return v;
}

}  // namespace rf
