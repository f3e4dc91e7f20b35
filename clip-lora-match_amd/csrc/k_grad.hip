// Streaming softmax gradients over the resident index (gfx950): the copy kernels of
// clm_index_softmax_grad. The weights W16 come from the EPI_SOFTW GEMM (gemm_common.hpp); the two
// accumulating GEMMs dq += W16 . R^T^T and dr += W16T . Q^T^T take K-contiguous fp16 operands, so the
// weights, the index chunk and the staged queries are each transposed once by transpose16, which
// also folds the inverse norms (rows appended as fp16 are stored unnormalised: their scale lives in
// the index's inv alone).
#include "kernels.hpp"

namespace clm {

namespace {
// One 64 x 64 tile per workgroup of 256 threads. Load: thread (r = t / 8, ch = t % 8) of each half
// reads 8 consecutive source columns of row r (one 16-byte load where the row is aligned, else
// element by element), scales in fp32, rounds to fp16 and writes 4 dwords into the row-major LDS
// tile. Rows are TLD = 66 halves = 33 dwords apart: a transposed read of 8 rows down one column by
// lanes (c = lane / 8, rg = lane % 8) touches dwords (rg * 8 + i) * 33 + c / 2, banks 8 rg + i + c / 2
// (mod 32) -- distinct over rg and c / 2, the two columns of a dword broadcast: conflict-free
// ds_read_u16. The dword writes (row * 33 + ch * 4 + k) are 2-way (rows r and r + 4 of neighbouring
// chunks): 4 writes against 8 reads per thread. Store: 8 rows of one destination row as one 16-byte
// store, a destination row's 128 bytes by 8 consecutive lanes.
constexpr int TT = 64, TLD = 66;

__global__ __launch_bounds__(256) void transpose16_kernel(const u16* __restrict__ src, int64_t lds, int64_t rows,
                                                         int64_t cols, const float* __restrict__ s,
                                                         u16* __restrict__ dst, int64_t ldd) {
  __shared__ uint32_t tile[TT * TLD / 2];
  const int64_t r0 = (int64_t)blockIdx.x * TT, c0 = (int64_t)blockIdx.y * TT;
  const int t = threadIdx.x;
  const bool src16 = (lds % 8) == 0 && ((uintptr_t)src & 15) == 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = h * 32 + t / 8, ch = t % 8;
    const int64_t gr = r0 + r, gc = c0 + ch * 8;
    u16 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0;
    if (gr < rows) {
      const u16* p = src + gr * lds + gc;
      if (src16 && gc + 8 <= cols) {
        const uint4 q = *(const uint4*)p;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (u16)(w[i / 2] >> (16 * (i & 1)));
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (gc + i < cols) v[i] = p[i];
      }
      if (s) {
        const float f = s[gr];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          // the fp32 product, then its rounding to fp16, as the contract states it: left to itself
          // the compiler fuses the two into v_fma_mixlo_f16, which rounds the exact product once and
          // differs from the two-step value in about one element of 2^13
          float p = f16_to_f32(v[i]) * f;
          asm volatile("" : "+v"(p));
          v[i] = f32_to_f16(p);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[r * (TLD / 2) + ch * 4 + k] = (uint32_t)v[2 * k] | ((uint32_t)v[2 * k + 1] << 16);
  }
  __syncthreads();
  const u16* th = (const u16*)tile;
  const bool dst16 = (ldd % 8) == 0 && ((uintptr_t)dst & 15) == 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = h * 32 + t / 8, rg = t % 8;
    const int64_t gc = c0 + c;
    if (gc >= cols) continue;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = (uint32_t)th[(rg * 8 + 2 * k) * TLD + c] | ((uint32_t)th[(rg * 8 + 2 * k + 1) * TLD + c] << 16);
    u16* o = dst + gc * ldd + r0 + rg * 8;   // r0 + rg * 8 + 7 < round_up(rows, 64) <= ldd
    if (dst16) {
      *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (u16)(w[i / 2] >> (16 * (i & 1)));
    }
  }
}

__global__ __launch_bounds__(256) void softw_offsets_kernel(const double* lse, int64_t n, double sub, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)(lse[i] * 1.4426950408889634 - sub);
}

__global__ __launch_bounds__(256) void scale_f32_kernel(float* v, int64_t n, float f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] *= f;
}
}  // namespace

hipError_t transpose16(const u16* src, int64_t lds, int64_t rows, int64_t cols, const float* s, u16* dst, int64_t ldd,
                       hipStream_t st) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  const int64_t tr = (rows + TT - 1) / TT, tc = (cols + TT - 1) / TT;
  if (!src || !dst || lds < cols || ldd < tr * TT || tr > 0x7FFFFFFF || tc > 65535) return hipErrorInvalidValue;
  transpose16_kernel<<<dim3((unsigned)tr, (unsigned)tc), 256, 0, st>>>(src, lds, rows, cols, s, dst, ldd);
  return hipGetLastError();
}

hipError_t softw_offsets(const double* lse, int64_t n, double sub, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  softw_offsets_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(lse, n, sub, out);
  return hipGetLastError();
}

hipError_t scale_f32(float* v, int64_t n, float f, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if ((n + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
  scale_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(v, n, f);
  return hipGetLastError();
}

}  // namespace clm
