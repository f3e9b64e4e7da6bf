// sparse_conv.hpp -- what sparse_conv.hip (the submanifold convolution) and sparse_stride.hip (the strided convolution and its
// transpose) share, ONCE: the clamped count, the 16-bit cell range and its row-major key, the sizes of a wave's LDS tile, the
// guarded quad load, the wave-level LDS hand-over, and the second launch of both weight gradients.
#pragma once
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned long long SC_PAD = ~0ull;

__device__ __forceinline__ int sc_count(const int *__restrict__ count, int bi, int n) {  // clamped into [0, n]
    return count ? min(max(count[bi], 0), n) : n;
}
__device__ __forceinline__ bool sc_in_range(int x, int y, int z) {
    return x >= -32768 && x <= 32767 && y >= -32768 && y <= 32767 && z >= -32768 && z <= 32767;
}
__device__ __forceinline__ unsigned long long sc_key(int x, int y, int z) {  // of a cell in range
    return (unsigned long long)(unsigned)(x + 32768) << 32 | (unsigned long long)(unsigned)(y + 32768) << 16 |
           (unsigned long long)(unsigned)(z + 32768);
}

constexpr int SC_TPB = 256;                 // 4 waves, each on its own: no workgroup barrier
constexpr int SC_ROWS = 128;                // rows of a workgroup, 32 per wave
constexpr int SC_KS = 32;                   // channels per slab
constexpr int SC_LD = SC_KS + 1;            // row stride of a [row][channel] slab: the operand reads touch 64 banks
constexpr unsigned short SC_ABSENT = 0xFFFF;

// floats of a wave's weight slab: [channel][column] (row stride 32, or 96 for two blocks so that the half-waves, one channel
// apart, read different banks) in the forward, [column][channel] (SC_LD) in the gradient
__host__ __device__ constexpr int sc_b_floats(int nb) { return nb == 1 ? 32 * SC_LD : 32 * 96; }
__host__ __device__ constexpr int sc_wave_bytes(int nb, int K) {
    return (32 * SC_LD + sc_b_floats(nb)) * 4 + (64 * K + 15) / 16 * 16;
}

template <bool VEC>
__device__ __forceinline__ float4 sc_quad(const float *__restrict__ p, int avail) {  // p[0..3], zeros from `avail` on
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
        if (avail > 0) v = *(const float4 *)p;  // (channels are a multiple of 4: a quad is inside or outside)
    } else {
        if (avail > 0) v.x = p[0];
        if (avail > 1) v.y = p[1];
        if (avail > 2) v.z = p[2];
        if (avail > 3) v.w = p[3];
    }
    return v;
}

// what one lane wrote to LDS is read by another lane of its wave: LDS serves a wave's requests in order, the fences keep
// the compiler from moving one over the other
__device__ __forceinline__ void sc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the samples' totals in ascending order, in double, rounded once
__global__ __launch_bounds__(256) void sparse_conv_wsum_kernel(int b, long E, const double *__restrict__ part, float *__restrict__ gw) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double s = 0.0;
    for (int bi = 0; bi < b; bi++) s += part[(size_t)bi * E + e];
    gw[e] = (float)s;
}

}  // namespace
