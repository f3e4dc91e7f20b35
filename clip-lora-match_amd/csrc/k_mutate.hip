// In-place mutation of the resident index (gfx950): the row movers of clm_index_remove /
// clm_index_update. Both are HBM-bound copies of whole rows of three arrays -- the fp16 rows, the
// fp32 rows (when the index keeps them) and the fp32 inverse norms -- in 16-byte units (a padded
// row is dim % 64 == 0 elements: 128 B granules of fp16, 256 B of fp32, so every unit is aligned).
//
//   gather_rows:  removal. Source rows [s0, s0 + rows) of the arrays; `rem` holds the sorted,
//                 de-duplicated removed rows that lie inside that range and `c0` the number of
//                 removed rows below s0. Row r survives unless it is in rem; its slot in the
//                 packed output is (r - s0) - |{x in rem : x < r}| (one binary search per row gives
//                 both answers). The output pointers are either a staging buffer or -- when the
//                 host has shown the destination range to end at or below s0 -- the arrays' own
//                 rows from s0 - c0 on. The kernel never reads a row outside [s0, s0 + rows) nor
//                 writes a slot >= the chunk's survivor count, so it cannot race with itself.
//   scatter_rows: update. Staged row i replaces row ids[i] - offset (the host has checked the ids
//                 are inside the index and distinct, so no two rows write one slot).
//
// A group of G = 8 .. 64 threads moves one row (G = the fp16 row's 16-byte units, capped at a
// wave), so narrow rows still fill the lanes.
#include <algorithm>

#include "kernels.hpp"

namespace clm {

namespace {

__device__ __forceinline__ void move_row(const u16* s16, const float* s32, const float* sinv, u16* d16, float* d32,
                                         float* dinv, int64_t src, int64_t dst, int dim, int t, int G) {
  const uint4* a = (const uint4*)(s16 + src * dim);
  uint4* b = (uint4*)(d16 + dst * dim);
  for (int e = t; e < dim / 8; e += G) b[e] = a[e];
  if (s32) {
    const uint4* a4 = (const uint4*)(s32 + src * dim);
    uint4* b4 = (uint4*)(d32 + dst * dim);
    for (int e = t; e < dim / 4; e += G) b4[e] = a4[e];
  }
  if (t == 0) dinv[dst] = sinv[src];
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const u16* rows16, const float* rows32, const float* inv,
                                                          int64_t s0, int64_t rows, int dim, const int64_t* rem,
                                                          int64_t m, u16* out16, float* out32, float* out_inv,
                                                          int G) {
  const int t = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (i >= rows) return;
  const int64_t r = s0 + i;
  int64_t lo = 0, hi = m;   // lower bound of r in rem[0, m)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rem[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  if (lo < m && rem[lo] == r) return;   // removed
  move_row(rows16, rows32, inv, out16, out32, out_inv, r, i - lo, dim, t, G);
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const u16* src16, const float* src32, const float* src_inv,
                                                           const int64_t* ids, int64_t offset, int64_t n, int dim,
                                                           u16* rows16, float* rows32, float* inv, int G) {
  const int t = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (i >= n) return;
  move_row(src16, src32, src_inv, rows16, rows32, inv, i, ids[i] - offset, dim, t, G);
}

}  // namespace

hipError_t gather_rows(const u16* rows16, const float* rows32, const float* inv, int64_t s0, int64_t rows, int dim,
                       const int64_t* rem, int64_t m, u16* out16, float* out32, float* out_inv, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (dim <= 0 || dim % 64 || m < 0 || (m > 0 && !rem) || (rows32 && !out32)) return hipErrorInvalidValue;
  const int G = group_of(dim);
  const int64_t blocks = (rows + 256 / G - 1) / (256 / G);
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  gather_rows_kernel<<<(unsigned)blocks, 256, 0, s>>>(rows16, rows32, inv, s0, rows, dim, rem, m, out16, out32,
                                                      out_inv, G);
  return hipGetLastError();
}

hipError_t scatter_rows(const u16* src16, const float* src32, const float* src_inv, const int64_t* ids, int64_t offset,
                        int64_t n, int dim, u16* rows16, float* rows32, float* inv, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (dim <= 0 || dim % 64 || !ids || (src32 && !rows32)) return hipErrorInvalidValue;
  const int G = group_of(dim);
  const int64_t blocks = (n + 256 / G - 1) / (256 / G);
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  scatter_rows_kernel<<<(unsigned)blocks, 256, 0, s>>>(src16, src32, src_inv, ids, offset, n, dim, rows16, rows32, inv,
                                                       G);
  return hipGetLastError();
}

}  // namespace clm
