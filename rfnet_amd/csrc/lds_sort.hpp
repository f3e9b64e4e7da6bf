// lds_sort.hpp -- the bitonic network over 64-bit words in LDS that sliced.hip (sorted projections) and grid_pool.hip (sorted
// cell keys) share, ONCE: the compare-exchange, where a word lives, one pass of up to four strides with the words in registers,
// and the stage loop.  The caller packs what it sorts by into the high bits and an index into the low bits, so that all words
// of a sort are distinct: the result is then the ascending order whatever the network does, ties to the lower index.
#pragma once
#include "common.hpp"

__device__ __forceinline__ void sw_cx(unsigned long long &a, unsigned long long &b) {  // ascending
    const bool lt = a < b;
    const unsigned long long lo = lt ? a : b, hi = lt ? b : a;
    a = lo, b = hi;
}

// Where word i lives in LDS: the low four bits are XORed with the next four, so that the 16 consecutive words a thread
// takes in the passes over the lowest strides fall on different banks from lane to lane.  A bijection inside each block of
// 256 words (of 64: P >= 64).
__device__ __forceinline__ int sw_at(int i) { return i ^ ((i >> 4) & 15); }

// One pass over the words: the R strides jl << (R - 1) ... jl of stage k, each thread 2^R words in registers.  The words of
// a group share every bit of their index above the strides, so they share the direction too (all strides are below k); a
// descending group is an ascending one on the complemented words, which keeps the direction out of the compare-exchanges
// (the sort is bound by their VALU work: a 64-bit compare and four selects each).
template <int R>
__device__ __forceinline__ void sw_pass(unsigned long long *__restrict__ w, int P, int k, int jl, int tid, int nt) {
    constexpr int E = 1 << R;
    for (int q = tid; q < (P >> R); q += nt) {
        const int lo = q & (jl - 1), i = ((q - lo) << R) | lo;
        const unsigned long long flip = (i & k) == 0 ? 0ull : ~0ull;
        unsigned long long a[E];
#pragma unroll
        for (int e = 0; e < E; e++) a[e] = w[sw_at(i + e * jl)] ^ flip;
#pragma unroll
        for (int t = R - 1; t >= 0; t--)
#pragma unroll
            for (int e = 0; e < E; e++)
                if (!(e & (1 << t))) sw_cx(a[e], a[e | (1 << t)]);
#pragma unroll
        for (int e = 0; e < E; e++) w[sw_at(i + e * jl)] = a[e] ^ flip;
    }
    __syncthreads();
}

// The network over the P words w[sw_at(0 .. P - 1)], P a power of two in 64 ... 16384, by the whole workgroup (tid of nt
// threads; the words are in place and a barrier has passed).  Stage k merges bitonic runs of k words with the strides
// k / 2 ... 1; a pass takes up to four of them (two below 8192 words, where the longer passes measured no faster).
__device__ __forceinline__ void sw_sort(unsigned long long *__restrict__ w, int P, int tid, int nt) {
    const int rmax = P >= 8192 ? 4 : 2;
    for (int s2 = 1; (1 << s2) <= P; s2++) {
        const int k = 1 << s2;
        for (int rem = s2; rem > 0;) {
            const int r = rem >= rmax ? rmax : rem, jl = 1 << (rem - r);
            if (r == 4) sw_pass<4>(w, P, k, jl, tid, nt);
            else if (r == 3) sw_pass<3>(w, P, k, jl, tid, nt);
            else if (r == 2) sw_pass<2>(w, P, k, jl, tid, nt);
            else sw_pass<1>(w, P, k, jl, tid, nt);
            rem -= r;
        }
    }
}

// threads for a sort of P words: a thread per 4 words below 8192 words, per 16 from there on (sw_sort's rmax), 64 ... 1024
inline int sw_sort_threads(int P) {
    const int per = P >= 8192 ? 16 : 4;
    return P / per < 64 ? 64 : (P / per > 1024 ? 1024 : P / per);
}
