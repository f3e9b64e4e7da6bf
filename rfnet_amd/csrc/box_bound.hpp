// box_bound.hpp -- the wave reductions and the point/box bound shared by the kernels that search sorted clouds box by box
// (interpolate.hip three_nn_boxes_kernel, knn.hip knn_boxes_kernel).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace {

#define TB_ROW(OP, N) asm volatile("s_nop 1\n\t" OP " %0, %0, %0 row_ror:" #N " row_mask:0xf bank_mask:0xf" : "+v"(v))
__device__ __forceinline__ float tb_wave_max(float v) {  // uniform result; inputs not NaN
    TB_ROW("v_max_f32_dpp", 8);
    TB_ROW("v_max_f32_dpp", 4);
    TB_ROW("v_max_f32_dpp", 2);
    TB_ROW("v_max_f32_dpp", 1);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
__device__ __forceinline__ float tb_wave_min(float v) {
    TB_ROW("v_min_f32_dpp", 8);
    TB_ROW("v_min_f32_dpp", 4);
    TB_ROW("v_min_f32_dpp", 2);
    TB_ROW("v_min_f32_dpp", 1);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
#undef TB_ROW

// squared distance from a point (or, with plo != phi, a box) to a box, per axis the gap max(lo - phi, plo - hi, 0): the
// unfused expression of the op itself, so that bound <= d in fp32 (header).  An empty box (lo = +inf, hi = -inf) is at +inf.
__device__ __forceinline__ float tb_gap(float a, float b) { return fmaxf(fmaxf(a, b), 0.f); }
__device__ __forceinline__ float tb_bound(float lx, float ly, float lz, float hx, float hy, float hz, float pxl, float pyl,
                                          float pzl, float pxh, float pyh, float pzh) {
    const float gx = tb_gap(lx - pxh, pxl - hx), gy = tb_gap(ly - pyh, pyl - hy), gz = tb_gap(lz - pzh, pzl - hz);
    return (gx * gx + gy * gy) + gz * gz;
}


}  // namespace
