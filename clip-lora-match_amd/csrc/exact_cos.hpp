// The exact (fp64) cosine of one (query, row) pair, one wave per pair: the single device routine
// behind every exact score of the library (k_search.hip: exact_scores, rescore_select,
// rescore_wide; k_rank.hip: target_scores, rank_rescore). fp32 x fp32 products are exact in fp64;
// one fixed element -> lane mapping and reduction order, rounded once to fp32, so a pair scores
// bit-identically on every path.
#pragma once
#include "clm_common.hpp"

namespace clm {
namespace exact_cos {

template <typename R>
__device__ __forceinline__ float row_elem(const R* r, int64_t e) {
  if constexpr (sizeof(R) == 2) return f16_to_f32(r[e]);
  else return r[e];
}

// lane-partial fp64 sums over elements e = lane + 64 i, then one xor-tree over the wave
template <typename R>
__device__ __forceinline__ void dot_wave(const float* q, const R* r, int dim, int lane, double& dot, double& rr) {
  double a = 0.0, b = 0.0;
  for (int e = lane; e < dim; e += 64) {
    const double rv = (double)row_elem(r, e);
    a = fma((double)q[e], rv, a);
    b = fma(rv, rv, b);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  dot = a;
  rr = b;
}

__device__ __forceinline__ float cos_from(double dot, double qn, double rr) {
  return (float)(dot / (qn * sqrt(rr)));
}

}  // namespace exact_cos
}  // namespace clm
