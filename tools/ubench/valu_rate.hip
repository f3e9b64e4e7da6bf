// valu_rate.hip -- measures the fp32 VALU issue rates that bound the Chamfer / EMD sweeps on
// gfx950: v_fma_f32, v_pk_fma_f32, v_sub_f32, v_pk_add_f32, v_min3_f32, v_exp_f32 and the
// Chamfer pair mix, at 1..8 waves per SIMD.  Also reads the shader clock (s_memtime vs
// s_memrealtime).  Development aid: hipcc --offload-arch=gfx950 -O3 valu_rate.hip -o valu_rate
// `valu_rate sort` runs only the last section: the instruction classes the culled sort's phases are made of (integer select /
// mask / shift-or / multiply-add, the float-to-integer conversions, v_med3_f32, plain and self-canonicalising min / max) at the
// sort's residency of 4 waves per SIMD, and what v_cvt_pk_u8_f32 returns on the inputs a bin computation can meet
// (profiles/sort_issue_costs.txt).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float f2 __attribute__((ext_vector_type(2)));

#define REP8(x) x x x x x x x x

template <int MODE>
__global__ void k(float *out, int iters, unsigned long long *clk) {
    float a = threadIdx.x * 1e-3f, b = 1.0001f;
    float c0 = 0, c1 = 1, c2 = 2, c3 = 3, c4 = 4, c5 = 5, c6 = 6, c7 = 7;
    f2 p0 = {0, 1}, p1 = {2, 3}, p2 = {4, 5}, p3 = {6, 7}, p4 = {1, 1}, p5 = {2, 2}, p6 = {3, 3}, p7 = {4, 4};
    f2 pa = {a, a}, pb = {b, b};
    const float sa2 = __builtin_amdgcn_readfirstlane(a), sb2 = __builtin_amdgcn_readfirstlane(b);
    unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; i++) {
        if (MODE == 0) {  // v_fma_f32, 8 independent chains
            REP8(asm volatile("v_fma_f32 %0, %8, %9, %0\n v_fma_f32 %1, %8, %9, %1\n v_fma_f32 %2, %8, %9, %2\n v_fma_f32 %3, %8, %9, %3\n"
                              "v_fma_f32 %4, %8, %9, %4\n v_fma_f32 %5, %8, %9, %5\n v_fma_f32 %6, %8, %9, %6\n v_fma_f32 %7, %8, %9, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 1) {  // v_pk_fma_f32
            REP8(asm volatile("v_pk_fma_f32 %0, %8, %9, %0\n v_pk_fma_f32 %1, %8, %9, %1\n v_pk_fma_f32 %2, %8, %9, %2\n v_pk_fma_f32 %3, %8, %9, %3\n"
                              "v_pk_fma_f32 %4, %8, %9, %4\n v_pk_fma_f32 %5, %8, %9, %5\n v_pk_fma_f32 %6, %8, %9, %6\n v_pk_fma_f32 %7, %8, %9, %7\n"
                              : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(pa), "v"(pb));)
        } else if (MODE == 2) {  // v_sub_f32 (VOP2)
            REP8(asm volatile("v_sub_f32 %0, %8, %0\n v_sub_f32 %1, %8, %1\n v_sub_f32 %2, %8, %2\n v_sub_f32 %3, %8, %3\n"
                              "v_sub_f32 %4, %8, %4\n v_sub_f32 %5, %8, %5\n v_sub_f32 %6, %8, %6\n v_sub_f32 %7, %8, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 3) {  // v_pk_add_f32
            REP8(asm volatile("v_pk_add_f32 %0, %8, %0\n v_pk_add_f32 %1, %8, %1\n v_pk_add_f32 %2, %8, %2\n v_pk_add_f32 %3, %8, %3\n"
                              "v_pk_add_f32 %4, %8, %4\n v_pk_add_f32 %5, %8, %5\n v_pk_add_f32 %6, %8, %6\n v_pk_add_f32 %7, %8, %7\n"
                              : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(pa), "v"(pb));)
        } else if (MODE == 4) {  // v_min3_f32
            REP8(asm volatile("v_min3_f32 %0, %8, %9, %0\n v_min3_f32 %1, %8, %9, %1\n v_min3_f32 %2, %8, %9, %2\n v_min3_f32 %3, %8, %9, %3\n"
                              "v_min3_f32 %4, %8, %9, %4\n v_min3_f32 %5, %8, %9, %5\n v_min3_f32 %6, %8, %9, %6\n v_min3_f32 %7, %8, %9, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 5) {  // v_exp_f32
            REP8(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_exp_f32 %2, %2\n v_exp_f32 %3, %3\n"
                              "v_exp_f32 %4, %4\n v_exp_f32 %5, %5\n v_exp_f32 %6, %6\n v_exp_f32 %7, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 6) {  // Chamfer pair mix: 3 sub, mul, 2 fmac per pair + min3 per 2 pairs (13 instr per 2 pairs) x4
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n v_mul_f32 %1, %1, %1\n v_sub_f32 %2, %8, %6\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_sub_f32 %0, %9, %4\n v_sub_f32 %3, %8, %5\n v_mul_f32 %3, %3, %3\n v_sub_f32 %2, %9, %6\n v_fmac_f32 %3, %0, %0\n v_fmac_f32 %3, %2, %2\n"
                "v_min3_f32 %7, %7, %1, %3\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 7) {  // same pair mix with an SGPR candidate operand (scalar-load path)
            float sa = __builtin_amdgcn_readfirstlane(a), sb = __builtin_amdgcn_readfirstlane(b);
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n v_mul_f32 %1, %1, %1\n v_sub_f32 %2, %8, %6\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_sub_f32 %0, %9, %4\n v_sub_f32 %3, %8, %5\n v_mul_f32 %3, %3, %3\n v_sub_f32 %2, %9, %6\n v_fmac_f32 %3, %0, %0\n v_fmac_f32 %3, %2, %2\n"
                "v_min3_f32 %7, %7, %1, %3\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "s"(sa), "s"(sb));)
        } else if (MODE == 8) {  // EMD column: 3 sub, mul, 2 fmac, mul, exp, fmac -- ONE accumulator (x8 columns)
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n v_mul_f32 %1, %1, %1\n v_sub_f32 %2, %8, %6\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_mul_f32 %1, %9, %1\n v_exp_f32 %1, %1\n v_fmac_f32 %7, %8, %1\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "s"(sa2), "s"(sb2));)
        } else if (MODE == 9) {  // same, two columns interleaved with two accumulators (x4)
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n v_sub_f32 %2, %8, %6\n v_mul_f32 %1, %1, %1\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_mul_f32 %1, %9, %1\n v_exp_f32 %1, %1\n"
                "v_sub_f32 %0, %9, %4\n v_sub_f32 %2, %8, %5\n v_mul_f32 %2, %2, %2\n v_fmac_f32 %2, %0, %0\n v_sub_f32 %0, %9, %6\n v_fmac_f32 %2, %0, %0\n"
                "v_mul_f32 %2, %9, %2\n v_exp_f32 %2, %2\n v_fmac_f32 %7, %8, %1\n v_fmac_f32 %3, %8, %2\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "s"(sa2), "s"(sb2));)
        } else if (MODE == 10) {  // mode 8 + 2 SALU moves per column: is scalar issue free next to VALU?
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n s_mov_b32 s20, s21\n v_mul_f32 %1, %1, %1\n v_sub_f32 %2, %8, %6\n v_fmac_f32 %1, %0, %0\n s_mov_b32 s22, s23\n v_fmac_f32 %1, %2, %2\n"
                "v_mul_f32 %1, %9, %1\n v_exp_f32 %1, %1\n v_fmac_f32 %7, %8, %1\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "s"(sa2), "s"(sb2) : "s20", "s22");)
        } else if (MODE == 11) {  // chamfer pair mix with an SGPR operand + 1 SALU move per pair
            float sa = __builtin_amdgcn_readfirstlane(a), sb = __builtin_amdgcn_readfirstlane(b);
            REP8(asm volatile(
                "v_sub_f32 %0, %8, %4\n v_sub_f32 %1, %9, %5\n s_mov_b32 s20, s21\n v_mul_f32 %1, %1, %1\n v_sub_f32 %2, %8, %6\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_sub_f32 %0, %9, %4\n v_sub_f32 %3, %8, %5\n s_mov_b32 s22, s23\n v_mul_f32 %3, %3, %3\n v_sub_f32 %2, %9, %6\n v_fmac_f32 %3, %0, %0\n v_fmac_f32 %3, %2, %2\n"
                "v_min3_f32 %7, %7, %1, %3\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "s"(sa), "s"(sb) : "s20", "s22");)
        } else if (MODE == 12) {  // v_permlane32_swap (VOP1), 4 independent register pairs
            REP8(asm volatile("v_permlane32_swap_b32 %0, %1\n v_permlane32_swap_b32 %2, %3\n v_permlane32_swap_b32 %4, %5\n v_permlane32_swap_b32 %6, %7\n"
                              "v_permlane32_swap_b32 %0, %1\n v_permlane32_swap_b32 %2, %3\n v_permlane32_swap_b32 %4, %5\n v_permlane32_swap_b32 %6, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7));)
        } else if (MODE == 13) {  // v_permlane16_swap
            REP8(asm volatile("v_permlane16_swap_b32 %0, %1\n v_permlane16_swap_b32 %2, %3\n v_permlane16_swap_b32 %4, %5\n v_permlane16_swap_b32 %6, %7\n"
                              "v_permlane16_swap_b32 %0, %1\n v_permlane16_swap_b32 %2, %3\n v_permlane16_swap_b32 %4, %5\n v_permlane16_swap_b32 %6, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7));)
        } else if (MODE == 14) {  // v_min_f32_dpp row_ror:8, 8 independent chains (sources never just-written)
            REP8(asm volatile("v_min_f32_dpp %0, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n v_min_f32_dpp %1, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
                              "v_min_f32_dpp %2, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n v_min_f32_dpp %3, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
                              "v_min_f32_dpp %4, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n v_min_f32_dpp %5, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
                              "v_min_f32_dpp %6, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n v_min_f32_dpp %7, %8, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 15) {  // v_cndmask_b32_e64 with an SGPR-pair mask
            REP8(asm volatile("v_cndmask_b32_e64 %0, %8, %9, s[20:21]\n v_cndmask_b32_e64 %1, %8, %9, s[20:21]\n v_cndmask_b32_e64 %2, %8, %9, s[20:21]\n v_cndmask_b32_e64 %3, %8, %9, s[20:21]\n"
                              "v_cndmask_b32_e64 %4, %8, %9, s[20:21]\n v_cndmask_b32_e64 %5, %8, %9, s[20:21]\n v_cndmask_b32_e64 %6, %8, %9, s[20:21]\n v_cndmask_b32_e64 %7, %8, %9, s[20:21]\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "s20", "s21");)
        } else if (MODE == 16) {  // ds_bpermute_b32, 8 in flight
            REP8(asm volatile("ds_bpermute_b32 %0, %8, %0\n ds_bpermute_b32 %1, %8, %1\n ds_bpermute_b32 %2, %8, %2\n ds_bpermute_b32 %3, %8, %3\n"
                              "ds_bpermute_b32 %4, %8, %4\n ds_bpermute_b32 %5, %8, %5\n ds_bpermute_b32 %6, %8, %6\n ds_bpermute_b32 %7, %8, %7\n s_waitcnt lgkmcnt(0)\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 17) {  // v_cndmask_b32_e32 (VCC mask)
            REP8(asm volatile("v_cndmask_b32_e32 %0, %8, %9, vcc\n v_cndmask_b32_e32 %1, %8, %9, vcc\n v_cndmask_b32_e32 %2, %8, %9, vcc\n v_cndmask_b32_e32 %3, %8, %9, vcc\n"
                              "v_cndmask_b32_e32 %4, %8, %9, vcc\n v_cndmask_b32_e32 %5, %8, %9, vcc\n v_cndmask_b32_e32 %6, %8, %9, vcc\n v_cndmask_b32_e32 %7, %8, %9, vcc\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "vcc");)
        } else if (MODE == 18) {  // v_readlane_b32 + v_writelane_b32 pairs
            REP8(asm volatile("v_readlane_b32 s20, %0, 3\n v_writelane_b32 %1, s22, 5\n v_readlane_b32 s21, %2, 3\n v_writelane_b32 %3, s22, 5\n"
                              "v_readlane_b32 s20, %4, 3\n v_writelane_b32 %5, s22, 5\n v_readlane_b32 s21, %6, 3\n v_writelane_b32 %7, s22, 5\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : : "s20", "s21");)
        } else if (MODE == 19) {  // Chamfer pair mix, candidate coordinates as DPP row_newbcast source operands (sub-wave tile form)
            REP8(asm volatile(
                "v_sub_f32_dpp %0, %4, %8 row_newbcast:3 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %1, %5, %9 row_newbcast:3 row_mask:0xf bank_mask:0xf\n v_mul_f32 %1, %1, %1\n"
                "v_sub_f32_dpp %2, %6, %8 row_newbcast:3 row_mask:0xf bank_mask:0xf\n v_fmac_f32 %1, %0, %0\n v_fmac_f32 %1, %2, %2\n"
                "v_sub_f32_dpp %0, %4, %9 row_newbcast:4 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %3, %5, %8 row_newbcast:4 row_mask:0xf bank_mask:0xf\n v_mul_f32 %3, %3, %3\n"
                "v_sub_f32_dpp %2, %6, %9 row_newbcast:4 row_mask:0xf bank_mask:0xf\n v_fmac_f32 %3, %0, %0\n v_fmac_f32 %3, %2, %2\n"
                "v_min3_f32 %7, %7, %1, %3\n"
                : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 20) {  // v_sub_f32_dpp row_newbcast alone, 8 independent chains
            REP8(asm volatile("v_sub_f32_dpp %0, %8, %9 row_newbcast:1 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %1, %8, %9 row_newbcast:2 row_mask:0xf bank_mask:0xf\n"
                              "v_sub_f32_dpp %2, %8, %9 row_newbcast:3 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %3, %8, %9 row_newbcast:4 row_mask:0xf bank_mask:0xf\n"
                              "v_sub_f32_dpp %4, %8, %9 row_newbcast:5 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %5, %8, %9 row_newbcast:6 row_mask:0xf bank_mask:0xf\n"
                              "v_sub_f32_dpp %6, %8, %9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n v_sub_f32_dpp %7, %8, %9 row_newbcast:8 row_mask:0xf bank_mask:0xf\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 21) {  // v_mov_b32_dpp quad_perm broadcast (what a quad-shared query costs per exchanged value)
            REP8(asm volatile("v_mov_b32_dpp %0, %8 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %1, %8 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n"
                              "v_mov_b32_dpp %2, %8 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %3, %8 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n"
                              "v_mov_b32_dpp %4, %9 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %5, %9 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n"
                              "v_mov_b32_dpp %6, %9 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %7, %9 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 22) {  // v_cmp_lt_f32 feeding a v_cndmask_b32 (4 pairs, through vcc)
            REP8(asm volatile("v_cmp_lt_f32 vcc, %8, %0\n v_cndmask_b32_e32 %0, %8, %9, vcc\n v_cmp_lt_f32 vcc, %8, %1\n v_cndmask_b32_e32 %1, %8, %9, vcc\n"
                              "v_cmp_lt_f32 vcc, %8, %2\n v_cndmask_b32_e32 %2, %8, %9, vcc\n v_cmp_lt_f32 vcc, %8, %3\n v_cndmask_b32_e32 %3, %8, %9, vcc\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "vcc");)
        } else if (MODE == 23) {  // v_and_b32 (VOP2)
            REP8(asm volatile("v_and_b32 %0, %8, %0\n v_and_b32 %1, %8, %1\n v_and_b32 %2, %8, %2\n v_and_b32 %3, %8, %3\n"
                              "v_and_b32 %4, %8, %4\n v_and_b32 %5, %8, %5\n v_and_b32 %6, %8, %6\n v_and_b32 %7, %8, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 24) {  // v_lshl_or_b32 (VOP3)
            REP8(asm volatile("v_lshl_or_b32 %0, %0, 1, %8\n v_lshl_or_b32 %1, %1, 1, %8\n v_lshl_or_b32 %2, %2, 1, %8\n v_lshl_or_b32 %3, %3, 1, %8\n"
                              "v_lshl_or_b32 %4, %4, 1, %8\n v_lshl_or_b32 %5, %5, 1, %8\n v_lshl_or_b32 %6, %6, 1, %8\n v_lshl_or_b32 %7, %7, 1, %8\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 25) {  // v_and_or_b32 (VOP3)
            REP8(asm volatile("v_and_or_b32 %0, %0, %8, %9\n v_and_or_b32 %1, %1, %8, %9\n v_and_or_b32 %2, %2, %8, %9\n v_and_or_b32 %3, %3, %8, %9\n"
                              "v_and_or_b32 %4, %4, %8, %9\n v_and_or_b32 %5, %5, %8, %9\n v_and_or_b32 %6, %6, %8, %9\n v_and_or_b32 %7, %7, %8, %9\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 26) {  // v_mad_u32_u24 (VOP3)
            REP8(asm volatile("v_mad_u32_u24 %0, %0, %8, %9\n v_mad_u32_u24 %1, %1, %8, %9\n v_mad_u32_u24 %2, %2, %8, %9\n v_mad_u32_u24 %3, %3, %8, %9\n"
                              "v_mad_u32_u24 %4, %4, %8, %9\n v_mad_u32_u24 %5, %5, %8, %9\n v_mad_u32_u24 %6, %6, %8, %9\n v_mad_u32_u24 %7, %7, %8, %9\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 27) {  // v_cvt_i32_f32 (VOP1)
            REP8(asm volatile("v_cvt_i32_f32 %0, %0\n v_cvt_i32_f32 %1, %1\n v_cvt_i32_f32 %2, %2\n v_cvt_i32_f32 %3, %3\n"
                              "v_cvt_i32_f32 %4, %4\n v_cvt_i32_f32 %5, %5\n v_cvt_i32_f32 %6, %6\n v_cvt_i32_f32 %7, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 28) {  // v_cvt_pk_u8_f32 (VOP3): float -> byte 1 of the destination's old value
            REP8(asm volatile("v_cvt_pk_u8_f32 %0, %8, 1, %0\n v_cvt_pk_u8_f32 %1, %8, 1, %1\n v_cvt_pk_u8_f32 %2, %8, 1, %2\n v_cvt_pk_u8_f32 %3, %8, 1, %3\n"
                              "v_cvt_pk_u8_f32 %4, %8, 1, %4\n v_cvt_pk_u8_f32 %5, %8, 1, %5\n v_cvt_pk_u8_f32 %6, %8, 1, %6\n v_cvt_pk_u8_f32 %7, %8, 1, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 29) {  // v_med3_f32 (VOP3)
            REP8(asm volatile("v_med3_f32 %0, %0, %8, %9\n v_med3_f32 %1, %1, %8, %9\n v_med3_f32 %2, %2, %8, %9\n v_med3_f32 %3, %3, %8, %9\n"
                              "v_med3_f32 %4, %4, %8, %9\n v_med3_f32 %5, %5, %8, %9\n v_med3_f32 %6, %6, %8, %9\n v_med3_f32 %7, %7, %8, %9\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 30) {  // v_min_f32 / v_max_f32 alternating (VOP2)
            REP8(asm volatile("v_min_f32 %0, %8, %0\n v_max_f32 %1, %8, %1\n v_min_f32 %2, %8, %2\n v_max_f32 %3, %8, %3\n"
                              "v_min_f32 %4, %8, %4\n v_max_f32 %5, %8, %5\n v_min_f32 %6, %8, %6\n v_max_f32 %7, %8, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        } else if (MODE == 31) {  // v_max_f32 x, x, x: the canonicalisation the compiler puts in front of fminf / fmaxf
            REP8(asm volatile("v_max_f32 %0, %0, %0\n v_max_f32 %1, %1, %1\n v_max_f32 %2, %2, %2\n v_max_f32 %3, %3, %3\n"
                              "v_max_f32 %4, %4, %4\n v_max_f32 %5, %5, %5\n v_max_f32 %6, %6, %6\n v_max_f32 %7, %7, %7\n"
                              : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b));)
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7 + p0.x + p1.y + p2.x + p3.y + p4.x + p5.x + p6.x + p7.x;
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = t1 - t0; clk[1] = r1 - r0; }
}

template <int MODE>
void run(const char *name, int instr_per_iter, int waves_per_simd) {
    const int iters = 2000;
    int blocks = 256 * waves_per_simd;  // 256 threads = 4 waves = 1 per SIMD per block
    float *out; unsigned long long *clk;
    hipMalloc(&out, sizeof(float) * blocks * 256);
    hipMalloc(&clk, 16);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k<MODE><<<blocks, 256>>>(out, iters, clk);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int r = 0; r < 5; r++) k<MODE><<<blocks, 256>>>(out, iters, clk);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); ms /= 5;
    unsigned long long h[2]; hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
    double ghz = (double)h[0] / ((double)h[1] / 100e6) / 1e9;
    double winstr = (double)blocks * 4 * iters * instr_per_iter;  // wave-instructions
    double per_simd_cyc = ms * 1e-3 * ghz * 1e9 * 1024 / winstr;
    printf("%-14s waves/SIMD=%d  %.3f ms  clock %.2f GHz  %.2f cycles per wave-instruction per SIMD  (%.1f T wave-lane-ops/s)\n",
           name, waves_per_simd, ms, ghz, per_simd_cyc, winstr * 64 / (ms * 1e-3) / 1e12);
    hipFree(out); hipFree(clk);
}

// what the conversions return: v_cvt_pk_u8_f32 into byte 0 of 0 and into byte 2 of 0xAABBCCDD, beside the clamp-and-convert it
// would replace (v_med3_f32 to [0, 255], v_cvt_i32_f32, & 255)
__global__ void cvt_probe(const unsigned *in, unsigned *out, int n) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const float f = __uint_as_float(in[i]);
    out[3 * i] = __builtin_amdgcn_cvt_pk_u8_f32(f, 0, 0u);
    out[3 * i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(f, 2, 0xAABBCCDDu);
    out[3 * i + 2] = (unsigned)((int)__builtin_amdgcn_fmed3f(f, 0.f, 255.f) & 255);
}

void probe_cvt() {
    const unsigned bits[] = {
        0x7FC00000u, 0xFFC00000u, 0x7FA00000u, 0xFFA00001u,  // quiet NaN, -quiet NaN, signalling NaNs
        0x7F800000u, 0xFF800000u,                            // +inf, -inf
        0x80000000u, 0x00000001u, 0x80000001u,               // -0.0, smallest denormals
    };
    const float vals[] = {-1e30f, -300.f, -1.f, -0.75f, -0.5f, -0.25f, 0.f, 0.25f, 0.49999997f, 0.5f, 0.75f, 0.99999994f, 1.f, 1.5f, 2.5f, 3.5f,
                          126.5f, 127.5f, 253.5f, 254.5f, 254.99998f, 255.f, 255.25f, 255.5f, 255.75f, 255.99998f, 256.f, 256.5f, 300.f, 65536.f, 1e30f};
    std::vector<unsigned> h(bits, bits + sizeof(bits) / 4);
    for (float v : vals) h.push_back(*(const unsigned *)&v);
    const int n = (int)h.size();
    unsigned *din, *dout;
    hipMalloc(&din, n * 4); hipMalloc(&dout, n * 12);
    hipMemcpy(din, h.data(), n * 4, hipMemcpyHostToDevice);
    cvt_probe<<<1, 64>>>(din, dout, n);
    std::vector<unsigned> o(3 * n);
    hipMemcpy(o.data(), dout, n * 12, hipMemcpyDeviceToHost);
    printf("\nv_cvt_pk_u8_f32: input bits, value -> byte 0 of 0 | byte 2 of 0xAABBCCDD | med3(0,255) + cvt_i32 + &255\n");
    for (int i = 0; i < n; i++)
        printf("  0x%08X %-16.9g -> %3u | 0x%08X | %3u\n", h[i], *(const float *)&h[i], o[3 * i], o[3 * i + 1], o[3 * i + 2]);
    hipFree(din); hipFree(dout);
}

void sort_section() {
    printf("\nthe culled sort's instruction classes at its residency (4 waves per SIMD; v_fma_f32 as the yardstick)\n");
    const int w = 4;
    run<0>("(warm-up, clock rising)", 64, w);  // the first launches of a process run while the clock is still rising
    run<0>("(warm-up, clock rising)", 64, w);
    run<0>("v_fma_f32", 64, w);
    run<17>("v_cndmask_b32 vcc", 64, w);
    run<15>("v_cndmask_b32 sgpr", 64, w);
    run<22>("v_cmp+v_cndmask", 64, w);
    run<23>("v_and_b32", 64, w);
    run<24>("v_lshl_or_b32", 64, w);
    run<25>("v_and_or_b32", 64, w);
    run<26>("v_mad_u32_u24", 64, w);
    run<27>("v_cvt_i32_f32", 64, w);
    run<28>("v_cvt_pk_u8_f32", 64, w);
    run<29>("v_med3_f32", 64, w);
    run<30>("v_min/max_f32", 64, w);
    run<31>("v_max_f32 x,x,x", 64, w);
    run<0>("v_fma_f32 again", 64, w);
    probe_cvt();
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "sort")) {
        sort_section();
        return 0;
    }
    for (int w : {4, 8}) {
        run<0>("v_fma_f32", 64, w);
        run<1>("v_pk_fma_f32", 64, w);
        run<2>("v_sub_f32", 64, w);
        run<3>("v_pk_add_f32", 64, w);
        run<4>("v_min3_f32", 64, w);
        run<5>("v_exp_f32", 64, w);
        run<6>("chamfer mix", 104, w);
        run<7>("chamfer mix sgpr", 104, w);
        run<8>("emd col 1acc", 72, w);
        run<9>("emd col 2acc", 144, w);
        run<10>("emd col +2salu", 72, w);   // cycles per VALU instruction (the 16 SALU not counted)
        run<11>("chamfer +salu", 104, w);
        run<12>("permlane32_swap", 64, w);
        run<13>("permlane16_swap", 64, w);
        run<14>("v_min_f32_dpp", 64, w);
        run<15>("cndmask_e64 sgpr", 64, w);
        run<16>("ds_bpermute", 64, w);
        run<17>("cndmask_e32 vcc", 64, w);
        run<18>("readlane/writelane", 64, w);
        run<19>("chamfer mix dpp-bcast", 104, w);
        run<20>("v_sub_f32_dpp newbcast", 64, w);
        run<21>("v_mov_dpp quad_perm", 64, w);
    }
    sort_section();
    return 0;
}
