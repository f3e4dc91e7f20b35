// Streaming log-sum-exp over the resident index (gfx950): the finishing kernels of clm_index_lse.
//
//   lse(q) = log sum_j exp(scale * s_j),   s_j = the exact score of row j (exact_cos.hpp)
//
// The exact route folds windows of exact scores into a running (maximum, sum) per query in fp64
// (lse_fold*). The fast route splits the rows at a head floor theta: the EPI_LSE GEMM lists the rows
// whose fp16-pass score reaches theta - margin (the band) and sums exp2((s - theta) * c) of all the
// others (the tail) into a slab of per-wave partials; here
//   lse_band_scores: the band rows re-scored exactly (rank_rescore's item plan);
//   lse_finish:      head (fixed point, so the list's slot order does not matter) + tail (slab in
//                    slot order) -> lse and a certified bound on its distance from the exact route.
// The reference route (clm_index_lse64) is the exact route without the rounding of s_j to fp32:
// lse_scores64 + the same fold on doubles, which also picks out the pair scores.
// Nothing here uses a floating-point atomic: two calls give the same bits.
#include <algorithm>

#include "exact_cos.hpp"
#include "kernels.hpp"

namespace clm {

namespace {
using namespace exact_cos;

constexpr int NT = 256;

__device__ __forceinline__ float fmax_t(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double fmax_t(double a, double b) { return fmax(a, b); }

// fixed-shape block reductions (every thread calls them; the result is valid on every thread)
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // sh may still be read from the previous reduction
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// maximum of the numbers (float or double); `bad` marks a NaN (a NaN anywhere makes the result NaN)
template <typename T>
__device__ __forceinline__ T block_max_nan(T v, bool bad, T* sh) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const T nan = (T)__builtin_nanf("");
  int nb = bad ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v = fmax_t(v, __shfl_xor(v, o, 64));
    nb |= __shfl_xor(nb, o, 64);
  }
  __syncthreads();
  if (lane == 0) sh[wid] = nb ? nan : v;
  __syncthreads();
  T r = sh[0];
  bool n = r != r;
  for (int w = 1; w < NT / 64; ++w) {
    n = n || sh[w] != sh[w];
    r = fmax_t(r, sh[w]);
  }
  return n ? nan : r;
}
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* sh) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void fold_init_kernel(double2* state, int64_t nq) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < nq) state[i] = make_double2(-INFINITY, 0.0);
}

// One workgroup per query over its row of the window: the window's maximum, then its terms
// exp(scale * (s - max)) summed per thread over columns t, t + 256, ... and by one fixed tree, then
// merged into the running state. The result depends on the window sizes (a function of the index
// size alone) and on nothing else: not on the other queries of the call, not on the route.
// S = float: the library's exact scores. S = double: the unrounded cosines of the reference route;
// there pair[row] takes the score of local row target[row] - base when the window [r0, r0 + C) holds it.
template <typename S>
__global__ __launch_bounds__(NT) void fold_kernel(const S* sc, int64_t lds, int64_t C, double scale, double2* state,
                                                  const int64_t* target, int64_t base, int64_t r0, double* pair) {
  __shared__ double shd[NT / 64];
  __shared__ S shf[NT / 64];
  const int64_t row = blockIdx.x;
  const S* s = sc + row * lds;
  S mx = (S)-INFINITY;
  bool bad = false;
  for (int64_t j = threadIdx.x; j < C; j += NT) {
    const S v = s[j];
    bad = bad || v != v;
    mx = fmax_t(mx, v);
  }
  const S wmax = block_max_nan<S>(mx, bad, shf);
  double sum = 0.0;
  if (wmax == wmax)
    for (int64_t j = threadIdx.x; j < C; j += NT) sum += exp(scale * ((double)s[j] - (double)wmax));
  const double wsum = block_sum(sum, shd);
  if (threadIdx.x == 0) {
    const double2 st = state[row];
    double2 o;
    if (!(wmax == wmax)) {
      o = make_double2(st.x, __builtin_nan(""));   // a NaN score: the sum is NaN from here on
    } else {
      const double M = fmax(st.x, (double)wmax);
      // the first window: st = (-inf, 0), and 0 * exp(-inf) = 0
      o = make_double2(M, st.y * exp(scale * (st.x - M)) + wsum * exp(scale * ((double)wmax - M)));
    }
    state[row] = o;
    if (target && pair) {
      const int64_t t = target[row] - base - r0;
      if (t >= 0 && t < C) pair[row] = (double)s[t];
    }
  }
}

// exact_scores (k_search.hip) without the rounding to fp32: out[qi, j] = dot / (|q| |row|) in fp64,
// one wave per row, queries looped
template <typename R>
__global__ __launch_bounds__(NT) void scores64_kernel(const float* q, const double* qn, int64_t nq, const R* rows,
                                                      int64_t rn, int dim, double* out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= rn) return;
  const R* r = rows + j * dim;
  for (int64_t qi = 0; qi < nq; ++qi) {
    double d, rr;
    dot_wave(q + qi * dim, r, dim, lane, d, rr);
    if (lane == 0) out[qi * ldo + j] = d / (qn[qi] * sqrt(rr));
  }
}

__global__ void fold_finish_kernel(const double2* state, int64_t nq, double scale, double* lse, float* err) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= nq) return;
  const double2 st = state[i];
  lse[i] = scale * st.x + log(st.y);
  if (err) err[i] = 0.f;
}

constexpr int BAND_GRID = 4096;

// rank_rescore_kernel's walk over the plan's items, one wave per listed row: the exact score goes
// to the slot of its index
template <typename R>
__global__ __launch_bounds__(NT) void band_scores_kernel(const int64_t* band, const int* cnt, int64_t cap,
                                                         const int* start, int nq, const float* q, const double* qn,
                                                         int dim, const R* rows, int64_t offset, float* band_s) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int total = start[nq];
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    int lo = 0, hi = nq - 1;   // the query of this item: the last one with start[q] <= item
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (start[mid] <= item) lo = mid;
      else hi = mid - 1;
    }
    const int64_t row = lo;
    const int chunk = item - start[lo];
    const int64_t c = cnt[row];
    const int64_t j0 = (int64_t)chunk * PLAN_CHUNK, j1 = min(c, j0 + PLAN_CHUNK);
    const float* qr = q + row * dim;
    const double qnr = qn[row];
    for (int64_t j = j0 + wid; j < j1; j += 4) {
      const int64_t ix = band[row * cap + j];
      double d, rr;
      dot_wave(qr, rows + (ix - offset) * dim, dim, lane, d, rr);
      if (lane == 0) band_s[row * cap + j] = cos_from(d, qnr, rr);
    }
  }
}

// One workgroup per query. With M = the largest band score, every band term v = exp(scale * (s - M))
// lies in (0, 1] and the largest is exactly 1; floor(v * 2^k) is added in 64-bit integers, k = 62 -
// ceil(log2(c + 1)) for c band rows (the total stays below 2^63), so the head H = total / 2^k does
// not depend on the order of the list and is short of the true sum by less than c * 2^-k. The error
// bound: DESIGN.md, "Streaming log-sum-exp".
__global__ __launch_bounds__(NT) void lse_finish_kernel(const float* band_s, const int* cnt, int64_t cap,
                                                        const float* part, int64_t slots, const float* theta,
                                                        double scale, double E, int64_t N, double* lse, float* err,
                                                        int* redo) {
  __shared__ double shd[NT / 64];
  __shared__ float shf[NT / 64];
  __shared__ unsigned long long shu[NT / 64];
  const int64_t row = blockIdx.x;
  const int64_t c = cnt[row];
  const float th = theta[row];
  if (c > cap || c <= 0 || !(fabsf(th) <= 3.4028235e38f)) {   // uniform over the workgroup
    if (threadIdx.x == 0) redo[row] = 1;
    return;
  }
  const float* bs = band_s + row * cap;
  float mx = -INFINITY;
  bool bad = false;
  for (int64_t j = threadIdx.x; j < c; j += NT) {
    const float v = bs[j];
    bad = bad || v != v;
    mx = fmaxf(mx, v);
  }
  const float Mf = block_max_nan<float>(mx, bad, shf);
  double tsum = 0.0;   // the slab: columns t, t + 256, ... per thread, then one fixed tree
  const float* pr = part + row * slots;
  for (int64_t j = threadIdx.x; j < slots; j += NT) tsum += (double)pr[j];
  const double tail = block_sum(tsum, shd);
  if (!(Mf == Mf) || !(tail >= 0.0 && tail <= 1.7976931348623157e308)) {   // uniform (block results)
    if (threadIdx.x == 0) redo[row] = 1;
    return;
  }
  int lg = 0;
  while (((int64_t)1 << lg) < c + 1) ++lg;
  const int k = 62 - lg;
  const double two_k = (double)((unsigned long long)1 << k);
  unsigned long long fx = 0;
  for (int64_t j = threadIdx.x; j < c; j += NT)
    fx += (unsigned long long)(exp(scale * ((double)bs[j] - (double)Mf)) * two_k);
  const unsigned long long tot = block_sum_u64(fx, shu);
  if (threadIdx.x != 0) return;
  const double M = (double)Mf;
  const double H = (double)tot / two_k;                       // >= 1: the largest term is 2^k
  const double w = exp(scale * ((double)th - M));             // tail units -> head units
  const double T = tail * w;
  const double total = H + T;
  const double out = scale * M + log(total);
  // certified bound: the tail's fp16-pass and fp32 errors, the head's fixed point, the
  // tail terms flushed to zero by v_exp_f32, fp64 rounding
  const double u = 5.9604644775390625e-8;                     // 2^-24
  const double D = 1.01 + fabs((double)th);                   // |s~ - theta| of any row
  const double rho_x = expm1(3.01 * u * scale * D);           // the exponent's three fp32 roundings
  const double rho = (1.0 + rho_x) * (1.0 + 2.0 * u) * (1.0 + 40.0 * u) - 1.0;   // + v_exp_f32 + <= 34 adds
  const double F = exp(scale * E) / (1.0 - rho);
  const double eta = (double)c / two_k;                       // head: relative fixed-point loss (H >= 1)
  const double flush = (double)N * 1.1754943508222875e-38 * w;
  const double slack = (double)(c + slots + 16) * 8.881784197001252e-16;   // 2^-50 per fp64 term
  const double e = (T / total) * (F - 1.0) + eta / (1.0 - eta) + flush / total + slack;
  if (!(rho < 1.0) || !(out == out) || !(e <= 3.0e38)) {
    redo[row] = 1;
    return;
  }
  lse[row] = out;
  err[row] = __double2float_ru(e * (1.0 + 1e-6));
}
}  // namespace

hipError_t lse_fold_init(double2* state, int64_t nq, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  fold_init_kernel<<<(unsigned)((nq + NT - 1) / NT), NT, 0, s>>>(state, nq);
  return hipGetLastError();
}

hipError_t lse_fold(const float* scores, int64_t lds, int64_t nq, int64_t C, double scale, double2* state,
                    hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  fold_kernel<float><<<(unsigned)nq, NT, 0, s>>>(scores, lds, C, scale, state, nullptr, 0, 0, nullptr);
  return hipGetLastError();
}

hipError_t lse_scores64(const float* q, const double* qn, int64_t nq, const void* rows, bool rows_f16, int64_t rn,
                        int dim, double* out, int64_t ldo, hipStream_t s) {
  if (nq <= 0 || rn <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((rn + 3) / 4);
  if (rows_f16) scores64_kernel<u16><<<grid, NT, 0, s>>>(q, qn, nq, (const u16*)rows, rn, dim, out, ldo);
  else scores64_kernel<float><<<grid, NT, 0, s>>>(q, qn, nq, (const float*)rows, rn, dim, out, ldo);
  return hipGetLastError();
}

hipError_t lse_fold64(const double* scores, int64_t lds, int64_t nq, int64_t C, double scale, double2* state,
                      const int64_t* target, int64_t base, int64_t r0, double* pair, hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  fold_kernel<double><<<(unsigned)nq, NT, 0, s>>>(scores, lds, C, scale, state, target, base, r0, pair);
  return hipGetLastError();
}

hipError_t lse_fold_finish(const double2* state, int64_t nq, double scale, double* lse, float* err, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  fold_finish_kernel<<<(unsigned)((nq + NT - 1) / NT), NT, 0, s>>>(state, nq, scale, lse, err);
  return hipGetLastError();
}

hipError_t lse_band_scores(const int64_t* band, const int* cnt, int64_t cap, const float* q, const double* qn, int dim,
                           const void* rows, bool rows_f16, int64_t offset, int64_t nq, int* plan, float* band_s,
                           hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  hipError_t e = rescore_plan(cnt, cap, nq, plan, s);
  if (e != hipSuccess) return e;
  if (rows_f16)
    band_scores_kernel<u16><<<BAND_GRID, NT, 0, s>>>(band, cnt, cap, plan, (int)nq, q, qn, dim, (const u16*)rows,
                                                     offset, band_s);
  else
    band_scores_kernel<float><<<BAND_GRID, NT, 0, s>>>(band, cnt, cap, plan, (int)nq, q, qn, dim, (const float*)rows,
                                                       offset, band_s);
  return hipGetLastError();
}

hipError_t lse_finish(const float* band_s, const int* cnt, int64_t cap, const float* part, int64_t slots,
                      const float* theta, double scale, double E, int64_t N, int64_t nq, double* lse, float* err,
                      int* redo, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (cap < 1 || slots < 1 || !err || !redo) return hipErrorInvalidValue;
  lse_finish_kernel<<<(unsigned)nq, NT, 0, s>>>(band_s, cnt, cap, part, slots, theta, scale, E, N, lse, err, redo);
  return hipGetLastError();
}

}  // namespace clm
