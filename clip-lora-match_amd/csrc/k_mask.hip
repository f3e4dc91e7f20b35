// Filtered search on the resident index (gfx950): the bitset kernels of clm_index_search_masked.
// A mask is ceil(N / 32) little-endian u32 words, bit j & 31 of word j >> 5 set iff local row j is
// allowed. (The hot path, the masked filter epilogue of the index GEMM, is EPI_FILTER_MASK in
// gemm_common.hpp.)
//
//   mask_prepare:  the caller's words copied into the index's buffer with the bits at or past N
//                  cleared, and one popcount per block of MASK_BLOCK_WORDS words;
//   mask_scan:     exclusive prefix sums of the block counts (one workgroup, fixed order) + the total P;
//   mask_compact:  the ordered list of the set local rows: a thread owns one word, its slot is the
//                  block's offset + the prefix sum of the popcounts before it in the block -- no
//                  atomics, so the list is the allowed rows ascending whatever the schedule;
//   mask_fill:     -inf into the disallowed entries of a window of exact scores (and the sign bit of
//                  an allowed NaN cleared, so it sorts above every number);
//   map_ids:       list positions -> global ids, and the dead marker (-inf scores get id -1);
//   mask_gather:   whole rows (fp16, fp32, inverse norm) at list positions, 16-byte units as the
//                  movers of k_mutate.hip (gather_rows_kernel there walks a removal list, not a
//                  position list, so the row mover is restated here).
// Every store is a plain vector store.
#include <algorithm>

#include "kernels.hpp"

namespace clm {

namespace {

constexpr int MB = MASK_BLOCK_WORDS;   // threads per block = words per block
static_assert(MB == 256, "the block scans below assume 4 waves of 64");

// the exclusive prefix sum of v over the block's 256 threads (*total: the block's sum); lds: 4 ints
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned* lds, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) base += lds[i];
    tot += lds[i];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__device__ __forceinline__ unsigned live_word(const uint32_t* src, int64_t i, int64_t nw, int64_t N) {
  if (i >= nw) return 0u;
  unsigned w = src[i];
  const int64_t rest = N - i * 32;   // rows this word covers
  if (rest < 32) w &= (1u << (int)rest) - 1u;
  return w;
}

__global__ __launch_bounds__(MB) void mask_prepare_kernel(const uint32_t* src, int64_t N, int64_t nw, uint32_t* dst,
                                                          uint32_t* bcnt) {
  __shared__ unsigned lds[4];
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  const unsigned w = live_word(src, i, nw, N);
  if (i < nw) dst[i] = w;
  unsigned tot;
  (void)block_exclusive((unsigned)__popc(w), lds, &tot);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MB) void mask_scan_kernel(const uint32_t* bcnt, int64_t nblocks, int64_t* boff) {
  __shared__ unsigned lds[4];
  int64_t run = 0;
  for (int64_t b0 = 0; b0 < nblocks; b0 += MB) {
    const int64_t b = b0 + threadIdx.x;
    const unsigned v = b < nblocks ? bcnt[b] : 0u;
    unsigned tot;
    const unsigned ex = block_exclusive(v, lds, &tot);   // <= 256 * 8192 per round: 32 bits hold it
    if (b < nblocks) boff[b] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) boff[nblocks] = run;
}

__global__ __launch_bounds__(MB) void mask_compact_kernel(const uint32_t* words, int64_t nw, const int64_t* boff,
                                                          uint32_t* list) {
  __shared__ unsigned lds[4];
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  unsigned w = i < nw ? words[i] : 0u;   // prepared words: the tail bits are clear
  unsigned tot;
  const unsigned ex = block_exclusive((unsigned)__popc(w), lds, &tot);
  uint32_t* out = list + boff[blockIdx.x] + ex;
  const uint32_t row0 = (uint32_t)(i * 32);
  while (w) {
    const int b = __ffs((int)w) - 1;
    *out++ = row0 + (uint32_t)b;
    w &= w - 1;
  }
}

__global__ __launch_bounds__(256) void mask_fill_kernel(float* scores, int64_t lds, int64_t C, int64_t r0,
                                                        const uint32_t* words) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  const int64_t r = r0 + j;
  float* p = scores + (int64_t)blockIdx.y * lds + j;
  if ((words[r >> 5] >> (r & 31)) & 1u) {
    // an allowed NaN keeps its place above every number: the top-k orders scores by their bit
    // pattern, and a NaN with the sign bit set would sort below the -inf of the dead entries
    const float v = *p;
    if (v != v) *p = __uint_as_float(__float_as_uint(v) & 0x7FFFFFFFu);
    return;
  }
  *p = -__builtin_inff();
}

__global__ __launch_bounds__(256) void map_ids_kernel(const float* scores, int64_t* ids, int64_t n, const uint32_t* list,
                                                      int64_t offset) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  if (id < 0 || scores[i] == -__builtin_inff()) ids[i] = -1;
  else if (list) ids[i] = offset + (int64_t)list[id];
}

__global__ __launch_bounds__(256) void mask_gather_kernel(const u16* rows16, const float* rows32, const float* inv,
                                                          int dim, const uint32_t* list, int64_t P, int64_t S,
                                                          u16* out16, float* out32, float* out_inv, int G) {
  const int t = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (i >= S) return;
  // floor(i * P / S): i < S <= P < 2^32, so the product fits 64 bits
  const int64_t pos = S == P ? i : (int64_t)(((uint64_t)i * (uint64_t)P) / (uint64_t)S);
  const int64_t src = (int64_t)list[pos];
  const uint4* a = (const uint4*)(rows16 + src * dim);
  uint4* b = (uint4*)(out16 + i * dim);
  for (int e = t; e < dim / 8; e += G) b[e] = a[e];
  if (rows32) {
    const uint4* a4 = (const uint4*)(rows32 + src * dim);
    uint4* b4 = (uint4*)(out32 + i * dim);
    for (int e = t; e < dim / 4; e += G) b4[e] = a4[e];
  }
  if (t == 0) out_inv[i] = inv[src];
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* out, int64_t n, float value) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = value;
}

}  // namespace

hipError_t mask_prepare(const uint32_t* src, int64_t N, uint32_t* dst, uint32_t* bcnt, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (!src || !dst || !bcnt || mask_blocks(N) > 0x7FFFFFFF) return hipErrorInvalidValue;
  mask_prepare_kernel<<<(unsigned)mask_blocks(N), MB, 0, s>>>(src, N, mask_words(N), dst, bcnt);
  return hipGetLastError();
}

hipError_t mask_scan(const uint32_t* bcnt, int64_t nblocks, int64_t* boff, hipStream_t s) {
  if (nblocks < 0 || !bcnt || !boff) return hipErrorInvalidValue;
  mask_scan_kernel<<<1, MB, 0, s>>>(bcnt, nblocks, boff);
  return hipGetLastError();
}

hipError_t mask_compact(const uint32_t* words, int64_t N, const int64_t* boff, uint32_t* list, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (!words || !boff || !list || N > (int64_t)0xFFFFFFFF) return hipErrorInvalidValue;
  mask_compact_kernel<<<(unsigned)mask_blocks(N), MB, 0, s>>>(words, mask_words(N), boff, list);
  return hipGetLastError();
}

hipError_t mask_fill(float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const uint32_t* words,
                     hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  if (!scores || !words || r0 < 0 || nq > 65535 || (C + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
  mask_fill_kernel<<<dim3((unsigned)((C + 255) / 256), (unsigned)nq), 256, 0, s>>>(scores, lds, C, r0, words);
  return hipGetLastError();
}

hipError_t map_ids(const float* scores, int64_t* ids, int64_t n, const uint32_t* list, int64_t offset, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!scores || !ids || (n + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
  map_ids_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(scores, ids, n, list, offset);
  return hipGetLastError();
}

hipError_t mask_gather(const u16* rows16, const float* rows32, const float* inv, int dim, const uint32_t* list,
                       int64_t P, int64_t S, u16* out16, float* out32, float* out_inv, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (dim <= 0 || dim % 8 || S > P || !list || !rows16 || !inv || !out16 || !out_inv || (rows32 && !out32))
    return hipErrorInvalidValue;
  const int G = group_of(dim);
  const int64_t blocks = (S + 256 / G - 1) / (256 / G);
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  mask_gather_kernel<<<(unsigned)blocks, 256, 0, s>>>(rows16, rows32, inv, dim, list, P, S, out16, out32, out_inv, G);
  return hipGetLastError();
}

hipError_t fill_f32(float* out, int64_t n, float value, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!out || (n + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
  fill_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(out, n, value);
  return hipGetLastError();
}

}  // namespace clm
