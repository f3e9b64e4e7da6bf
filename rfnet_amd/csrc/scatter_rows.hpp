// scatter_rows.hpp -- internal interface of scatter_rows.hip (the scatter-add gradients of group_point / three_interpolate as a
// counting sort of the slots by destination row + a gather that writes every destination row once).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rfs {

// dst (b, n, c)[idx (b, S)] += weight (b, S) * src (b, S / K, c)[slot / K]; K = 1 with weight == NULL, or K = 3 with weights.
bool rows_csr_supported(int b, int n, int c, long S, int K);
size_t rows_csr_workspace_bytes(int b, int n, long S);
// dst is fully overwritten (rows no slot names: zeros).  workspace: rows_csr_workspace_bytes, 16-byte aligned.
int rows_csr_scatter(int b, int n, int c, long S, int K, const float *src, const int *idx, const float *weight, float *dst,
                     void *workspace, const char *build_name, const char *gather_name, hipStream_t s);
// The counting sort alone, for gathers of their own: the workspace then holds row_start (b, n + 1) at its start and perm (b, S)
// at rows_csr_perm -- perm[row_start[r] .. row_start[r + 1]) are the slots s of a sample with idx[s] = r (any order).
int rows_csr_sort(int b, int n, long S, const int *idx, void *workspace, const char *build_name, hipStream_t s);
const int *rows_csr_perm(int b, int n, const void *workspace);
// The same sort of the S = m k slots of a ragged knn_point (idx (b, m, k); len1 (b) valid rows, len2 (b) valid queries, device
// arrays or NULL, clamped as every count): slots of queries behind len2, slots t >= len1 of a query and slots that name a row
// behind len1 are in no row, whatever idx holds there.
int rows_csr_sort_masked(int b, int n, int m, int k, const int *idx, const int *len1, const int *len2, void *workspace,
                         const char *build_name, hipStream_t s);

}  // namespace rfs
