// knn_list.hpp -- the register-resident k-best list shared by knn.hip (three dimensions) and knn_feature.hip (c dimensions).
//
// KB >= k slots of 64-bit keys (rank of the distance, index), sorted ascending, constant-index and fully unrolled (a dynamically
// indexed register array would go to scratch), one kernel per bucket KB in {4, 8, 16, 32, 64} (KN_DISPATCH).  The first KB - k
// slots hold key 0, which no key is below, so they never move: the live list is the last k slots and its k-th best is always
// slot KB - 1; an empty slot is ~0.  How a distance becomes a rank is the including file's (knn.hip: d >= 0; knn_feature.hip:
// signed).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef unsigned long long u64;

constexpr int KN_MAXK = 64;

// KB compares, 4 KB selects; a key that is below nothing (~0) leaves the list as it is
template <int KB>
__device__ __forceinline__ void kn_insert(u64 (&L)[KB], u64 key) {
    bool c[KB];
#pragma unroll
    for (int t = 0; t < KB; t++) c[t] = key < L[t];
#pragma unroll
    for (int t = KB - 1; t > 0; t--) L[t] = c[t - 1] ? L[t - 1] : (c[t] ? key : L[t]);
    L[0] = c[0] ? key : L[0];
}

// slots [from, k) of a row as zeros (ragged batches: behind a sample's neighbours, and the whole row of a padded query)
__device__ __forceinline__ void kn_zero(int from, int k, float *__restrict__ val, int *__restrict__ idx) {
    for (int t = from; t < k; t++) val[t] = 0.f, idx[t] = 0;
}

#define KN_DISPATCH(k, GO)                   \
    do {                                     \
        if ((k) <= 4) { GO(4); }             \
        else if ((k) <= 8) { GO(8); }        \
        else if ((k) <= 16) { GO(16); }      \
        else if ((k) <= 32) { GO(32); }      \
        else { GO(64); }                     \
    } while (0)

}  // namespace
