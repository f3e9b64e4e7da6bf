// group_internal.hpp -- launchers shared by the entry points of sampling.hip / grouping.hip and the one-call
// sample-and-group of sample_group.hip, and rfi::Counts, the argument through which a RAGGED kernel instantiation receives
// its per-sample counts.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "nn_pruned.hpp"
#include "wave.hpp"

namespace rfi {

// ---- ragged batches (the _lengths entries of include/rfops.h; the count of a batch element is rf::ragged_count, wave.hpp) ----
// How a kernel with a RAGGED instantiation receives the counts: as its LAST argument, a Counts<RAGGED> by value.  The plain
// instantiation's is EMPTY and count1 / count2 return the padded sizes themselves, so its code is what it was before the counts
// existed, instruction for instruction (checked on the disassembly); the ragged one carries the two device arrays
// (either may be NULL) and reads them through rf::ragged_count.
template <bool RAGGED>
struct Counts {
    const int *len1, *len2;
};
template <>
struct Counts<false> {};
__device__ __forceinline__ int count1(const Counts<false> &, int, int n) { return n; }
__device__ __forceinline__ int count2(const Counts<false> &, int, int m) { return m; }
__device__ __forceinline__ int count1(const Counts<true> &c, int bi, int n) { return rf::ragged_count(c.len1, bi, n); }
__device__ __forceinline__ int count2(const Counts<true> &c, int bi, int m) { return rf::ragged_count(c.len2, bi, m); }

// farthest_point_sample (sampling.hip).  new_xyz (b, m, 3): the samples' coordinates, written by the same launch (NULL: not
// wanted) -- gather_point(inp, out) fused: the kernel reloads every winner's coordinates anyway.  temp: b*n floats when
// n exceeds the register-resident limit (rf_farthestpointsampling_temp_floats), NULL otherwise.
int fps(int b, int n, int m, const float *inp, float *temp, int *out, float *new_xyz, hipStream_t s);

// The same op over a cloud that is already sorted (fps_sorted_kernel: clouds of 1025..16384 points): the same indices; a new
// sample only re-scans the regions it can still change.  fps_sorted_pays: from how many samples on the sort is repaid.
bool fps_sorted_pays(int n, int m);
int fps_sorted(int b, int n, int m, const float *inp, const rfp::Sorted &sv, int *out, float *new_xyz, hipStream_t s);

// Both over a ragged batch (rf_farthestpointsampling_lengths): len (b) valid points per cloud, len_out (b) samples wanted per
// cloud, device arrays or NULL; rows of `out` / `new_xyz` behind len_out are zeros.  fps_lengths takes every size (temp as
// fps), fps_sorted_lengths a cloud sorted WITH the same `len` (rfp::sort_sets' lens).
int fps_lengths(int b, int n, int m, const float *inp, const int *len, const int *len_out, float *temp, int *out,
                float *new_xyz, hipStream_t s);
int fps_sorted_lengths(int b, int n, int m, const float *inp, const int *len, const int *len_out, const rfp::Sorted &sv,
                       int *out, float *new_xyz, hipStream_t s);

// query_ball_point on a sorted dataset (grouping.hip, query_ball_boxes_kernel).  grouped_xyz (b, m, nsample, 3) or NULL:
// group_point(xyz1, idx) fused; zero_empty: rows of empty balls are written as index 0 instead of being left untouched.
// The caller has checked the domain (64 <= n <= 65536, nsample <= 64, b <= 65535).
// ragged (rf_queryballpoint_lengths): the dataset was sorted with len1, queries behind len2 get rows of zeros (len1 / len2 device
// arrays or NULL); every row is written whatever zero_empty says.
int ball_boxes(int b, int n, int m, float radius, const float *radius_dev, int nsample, const float *xyz1, const float *xyz2,
               const rfp::Sorted &so, int *idx, int *pts_cnt, float *grouped_xyz, int zero_empty, hipStream_t s,
               bool ragged = false, const int *len1 = nullptr, const int *len2 = nullptr);

}  // namespace rfi
