// Keyed search on the resident index (gfx950): the kernels of clm_index_search_keyed beside the index
// GEMM. Every index row carries one int32 key (the caller's, per call) and every query one inclusive
// key range [lo, hi]; row j is open to query y iff lo[y] <= keys[j] <= hi[y]. (The hot path, the keyed
// filter epilogue of the index GEMM, is EPI_FILTER_KEYS in gemm_common.hpp.)
//
//   key_fill:    mask_fill (k_mask.hip) with the per-query predicate: -inf into the entries of a window
//                of scores whose row is closed to the query, the sign bit of an open NaN cleared. The
//                exact route's windows (column j = row r0 + j) and the pass route's sample score matrix
//                (r0 = 0, keys = the sample's keys) both go through it;
//   key_sample:  S rows at positions floor(i * N / S) of the index: fp16 row, inverse norm and key, the
//                16-byte row mover of mask_gather without a position list.
// Every store is a plain vector store.
#include "kernels.hpp"

namespace clm {

namespace {

__global__ __launch_bounds__(256) void key_fill_kernel(float* scores, int64_t lds, int64_t C, int64_t r0,
                                                       const int32_t* keys, const int32_t* lo, const int32_t* hi) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  const int32_t key = keys[r0 + j];
  float* p = scores + (int64_t)blockIdx.y * lds + j;
  if (lo[blockIdx.y] <= key && key <= hi[blockIdx.y]) {
    // an open NaN keeps its place above every number, as in mask_fill
    const float v = *p;
    if (v != v) *p = __uint_as_float(__float_as_uint(v) & 0x7FFFFFFFu);
    return;
  }
  *p = -__builtin_inff();
}

__global__ __launch_bounds__(256) void key_sample_kernel(const u16* rows16, const float* inv, const int32_t* keys,
                                                         int dim, int64_t N, int64_t S, u16* out16, float* out_inv,
                                                         int32_t* out_keys, int G) {
  const int t = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (i >= S) return;
  // floor(i * N / S): i < S <= N < 2^31, so the product fits 64 bits
  const int64_t src = S == N ? i : (int64_t)(((uint64_t)i * (uint64_t)N) / (uint64_t)S);
  const uint4* a = (const uint4*)(rows16 + src * dim);
  uint4* b = (uint4*)(out16 + i * dim);
  for (int e = t; e < dim / 8; e += G) b[e] = a[e];
  if (t == 0) {
    out_inv[i] = inv[src];
    out_keys[i] = keys[src];
  }
}

}  // namespace

hipError_t key_fill(float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const int32_t* keys,
                    const int32_t* lo, const int32_t* hi, hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  if (!scores || !keys || !lo || !hi || r0 < 0 || nq > 65535 || (C + 255) / 256 > 0x7FFFFFFF)
    return hipErrorInvalidValue;
  key_fill_kernel<<<dim3((unsigned)((C + 255) / 256), (unsigned)nq), 256, 0, s>>>(scores, lds, C, r0, keys, lo, hi);
  return hipGetLastError();
}

hipError_t key_sample(const u16* rows16, const float* inv, const int32_t* keys, int dim, int64_t N, int64_t S,
                      u16* out16, float* out_inv, int32_t* out_keys, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (dim <= 0 || dim % 8 || S > N || N > 0x7FFFFFFF || !rows16 || !inv || !keys || !out16 || !out_inv || !out_keys)
    return hipErrorInvalidValue;
  const int G = group_of(dim);
  const int64_t blocks = (S + 256 / G - 1) / (256 / G);
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  key_sample_kernel<<<(unsigned)blocks, 256, 0, s>>>(rows16, inv, keys, dim, N, S, out16, out_inv, out_keys, G);
  return hipGetLastError();
}

}  // namespace clm
