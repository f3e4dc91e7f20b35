// Exact retrieval ranks on the resident index (gfx950): the finishing kernels of
// clm_index_rank / clm_index_count_above.
//
// The rank of a target row is one plus the number of rows ahead of it in the search order (score
// desc, index asc, NaN above every number: rank_ahead in kernels.hpp). The EPI_RANK GEMM decides
// every row whose fp16-pass score is further than RANK_MARGIN from the target's exact score and
// lists the rest (the band); here
//   target_scores: t[q] = the exact score of (q, its target row);
//   rank_rescore:  the band rows re-scored exactly and counted, added with the GEMM's count;
//   count_rank:    the same count over a window of an exact score matrix (the exact route).
// Every exact score goes through exact_cos.hpp, the routine of exact_scores and rescore_select,
// so a row compares against the target with the same bits on every route.
#include <algorithm>

#include "exact_cos.hpp"
#include "kernels.hpp"

namespace clm {

namespace {
using namespace exact_cos;

// one wave per query
template <typename R>
__global__ __launch_bounds__(256) void target_scores_kernel(const float* q, const double* qn, int64_t nq, int dim,
                                                            const R* rows, int64_t offset, const int64_t* target,
                                                            float* t) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= nq) return;
  double d, rr;
  dot_wave(q + qi * dim, rows + (target[qi] - offset) * dim, dim, lane, d, rr);
  if (lane == 0) t[qi] = cos_from(d, qn[qi], rr);
}

// block-wide sum of per-thread counts (every thread calls it); thread 0 gets the total
__device__ __forceinline__ unsigned long long block_total(unsigned long long v, unsigned long long* wsum) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) wsum[wid] = v;
  __syncthreads();
  unsigned long long tot = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += wsum[w];
  return tot;
}

// The band re-score as a list of work items, one per (query, chunk of RESCORE_CHUNK band rows):
// band lengths are skewed (a target nearer the bulk of the scores has a band hundreds of times the
// median), so one workgroup per query left the device waiting for the longest list of each launch
// (687 us per 2560-query launch at a mean of 22 rows, profiles/rank_pass_kernel_stats_v1.txt), and
// a grid over every possible chunk spent as long dispatching workgroups that exit at once (190 us
// with 196 chunks per query, ..._v2.txt). rescore_plan gives every complete list max(1, chunks)
// items (start = their exclusive prefix sums, start[nq] = the total; an overflowed list gets none:
// the exact route serves it); a fixed grid then walks the items, one wave per listed row. Each item
// adds its count to out[q] (zeroed by the caller) with one integer atomicAdd, a query's first item
// the GEMM's count as well: the sum does not depend on the order.
constexpr int RESCORE_CHUNK = PLAN_CHUNK, RESCORE_GRID = 4096, PLAN_NT = 1024;

__global__ __launch_bounds__(PLAN_NT) void rescore_plan_kernel(const int* cnt, int64_t cap, int nq, int* start) {
  __shared__ int part[PLAN_NT];
  const int per = (nq + PLAN_NT - 1) / PLAN_NT;
  const int q0 = min(nq, (int)threadIdx.x * per), q1 = min(nq, q0 + per);
  auto items = [&](int q) {
    const int64_t c = cnt[q];
    return c > cap ? 0 : (int)max<int64_t>(1, (c + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
  };
  int sum = 0;
  for (int q = q0; q < q1; ++q) sum += items(q);
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < PLAN_NT; o <<= 1) {   // inclusive scan of the threads' sums
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - sum;
  for (int q = q0; q < q1; ++q) {
    start[q] = run;
    run += items(q);
  }
  if (threadIdx.x == PLAN_NT - 1) start[nq] = part[PLAN_NT - 1];
}

template <typename R>
__global__ __launch_bounds__(256) void rank_rescore_kernel(const int64_t* band, const int* cnt, int64_t cap,
                                                           const unsigned* above32, const int* start, int nq,
                                                           const float* q, const double* qn, int dim, const R* rows,
                                                           int64_t offset, const float* t, const int64_t* g,
                                                           unsigned long long* out) {
  __shared__ unsigned long long wsum[4];
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
    const int64_t j0 = (int64_t)chunk * RESCORE_CHUNK, j1 = min(c, j0 + RESCORE_CHUNK);
    const float* qr = q + row * dim;
    const double qnr = qn[row];
    const float tq = t[row];
    const int64_t gq = g[row];
    unsigned long long mine = 0;
    for (int64_t j = j0 + wid; j < j1; j += 4) {
      const int64_t ix = band[row * cap + j];
      double d, rr;
      dot_wave(qr, rows + (ix - offset) * dim, dim, lane, d, rr);
      if (lane == 0 && rank_ahead(cos_from(d, qnr, rr), ix, tq, gq)) ++mine;
    }
    unsigned long long tot = block_total(mine, wsum);
    if (threadIdx.x == 0) {
      if (chunk == 0) tot += above32[row];
      if (tot) atomicAdd(out + row, tot);
    }
    __syncthreads();   // wsum is rewritten by the next item
  }
}

// one workgroup per query over its row of the window
__global__ __launch_bounds__(256) void count_rank_kernel(const float* S, int64_t lds, int64_t C, int64_t base,
                                                         const float* t, const int64_t* g, int64_t* above) {
  __shared__ unsigned long long wsum[4];
  const int64_t row = blockIdx.x;
  const float* s = S + row * lds;
  const float tq = t[row];
  const int64_t gq = g[row];
  unsigned long long mine = 0;
  for (int64_t j = threadIdx.x; j < C; j += 256) mine += rank_ahead(s[j], base + j, tq, gq) ? 1u : 0u;
  const unsigned long long tot = block_total(mine, wsum);
  if (threadIdx.x == 0) above[row] += (int64_t)tot;
}

__global__ void rank_from_above_kernel(const int64_t* above, int64_t nq, int64_t* rank) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nq) rank[i] = above[i] + 1;
}
}  // namespace

hipError_t target_scores(const float* q, const double* qn, int64_t nq, int dim, const void* rows, bool rows_f16,
                         int64_t offset, const int64_t* target, float* t, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((nq + 3) / 4);
  if (rows_f16) target_scores_kernel<u16><<<grid, 256, 0, s>>>(q, qn, nq, dim, (const u16*)rows, offset, target, t);
  else target_scores_kernel<float><<<grid, 256, 0, s>>>(q, qn, nq, dim, (const float*)rows, offset, target, t);
  return hipGetLastError();
}

hipError_t rescore_plan(const int* cnt, int64_t cap, int64_t nq, int* plan, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (cap < 1 || !plan || nq * ((cap + RESCORE_CHUNK - 1) / RESCORE_CHUNK) > 0x7FFFFFFF) return hipErrorInvalidValue;
  rescore_plan_kernel<<<1, PLAN_NT, 0, s>>>(cnt, cap, (int)nq, plan);
  return hipGetLastError();
}

hipError_t rank_rescore(const int64_t* band, const int* cnt, int64_t cap, const unsigned* above32, const float* q,
                        const double* qn, int dim, const void* rows, bool rows_f16, int64_t offset, const float* t,
                        const int64_t* g, int64_t nq, int* plan, int64_t* out, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  // the items of one launch are counted in an int: nq * ceil(cap / chunk) must fit
  if (cap < 1 || !plan || nq * ((cap + RESCORE_CHUNK - 1) / RESCORE_CHUNK) > 0x7FFFFFFF) return hipErrorInvalidValue;
  rescore_plan_kernel<<<1, PLAN_NT, 0, s>>>(cnt, cap, (int)nq, plan);
  unsigned long long* o = (unsigned long long*)out;
  if (rows_f16)
    rank_rescore_kernel<u16><<<RESCORE_GRID, 256, 0, s>>>(band, cnt, cap, above32, plan, (int)nq, q, qn, dim,
                                                          (const u16*)rows, offset, t, g, o);
  else
    rank_rescore_kernel<float><<<RESCORE_GRID, 256, 0, s>>>(band, cnt, cap, above32, plan, (int)nq, q, qn, dim,
                                                            (const float*)rows, offset, t, g, o);
  return hipGetLastError();
}

hipError_t count_rank(const float* scores, int64_t lds, int64_t nq, int64_t C, int64_t base, const float* t,
                      const int64_t* g, int64_t* above, hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  count_rank_kernel<<<(unsigned)nq, 256, 0, s>>>(scores, lds, C, base, t, g, above);
  return hipGetLastError();
}

hipError_t rank_from_above(const int64_t* above, int64_t nq, int64_t* rank, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  rank_from_above_kernel<<<(unsigned)((nq + 255) / 256), 256, 0, s>>>(above, nq, rank);
  return hipGetLastError();
}

}  // namespace clm
