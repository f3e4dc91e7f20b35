// Threshold search on the resident index (gfx950): the kernels that make clm_index_search_above's
// result ragged.
//
// The result of a query is every index row (s, id) for which rank_ahead(s, id, tau, INT64_MAX)
// holds -- exact score s >= tau, NaN above every number -- in the search order (score desc, id asc).
// Both routes hand over lists of unknown length; here
//   range_keep_count: per query, how many rows of its re-scored candidate list pass the rule;
//   range_emit:       those rows as 64-bit composites into the query's segment (slots by integer
//                     atomics: the order inside a segment is whatever the waves made it);
//   range_collect:    the same from a window of an exact score matrix (the exact route);
//   range_sort_runs / range_merge: every segment sorted descending -- runs of up to RANGE_RUN
//                     composites by one workgroup in LDS, longer segments by merge passes between
//                     two buffers -- which makes the order canonical: two calls return equal bits;
//   range_decode:     composites -> (score, global id) at the CSR position of the entry.
// A composite is (order key of the score << 32) | (0xFFFFFFFF - local row), as topk_any builds it:
// descending composites are (score desc, id asc), and distinct rows never compare equal.
// NaN scores lead (the rule) and come back as positive NaNs.
// Segment lengths differ by orders of magnitude (most queries keep a handful of rows, a few keep
// thousands), so every kernel walks a list of work items -- rescore_plan's chunks of a candidate
// list, or RangeItem records the host cuts from the segment lengths it has read -- instead of giving
// each query a workgroup that waits for the longest list.
#include <algorithm>

#include "kernels.hpp"

namespace clm {

namespace {
constexpr int64_t NO_TIE = 0x7FFFFFFFFFFFFFFFll;   // g of rank_ahead: ties with tau are kept

// A NaN score goes in with its sign cleared: float_key puts a positive NaN above +inf, where the rule
// has it, and a negative one (what 0 / 0 and inf / inf give in fp64 division here) below -inf.
__device__ __forceinline__ uint64_t composite(float s, int64_t local) {
  if (s != s) s = __uint_as_float(__float_as_uint(s) & 0x7FFFFFFFu);
  return ((uint64_t)float_key(s) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)local);
}

// the query of plan item `item`: the last one with start[q] <= item
__device__ __forceinline__ int plan_query(const int* start, int nq, int item) {
  int lo = 0, hi = nq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= item) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One wave per plan item (PLAN_CHUNK = 64 listed rows, one per lane). EMIT = false: len[q] += the
// rows that pass; EMIT = true: they are written at seg[src[q] + slot], slot from cursor[q].
template <bool EMIT>
__global__ __launch_bounds__(256) void keep_kernel(const float* band_s, const int64_t* band, const int* cnt,
                                                   int64_t cap, const int* start, int nq, const float* tau,
                                                   int64_t offset, int* len, int* cursor, const int64_t* src,
                                                   uint64_t* seg) {
  static_assert(PLAN_CHUNK == 64, "one lane per listed row of an item");
  const int lane = threadIdx.x & 63;
  const int total = start[nq];
  const int waves = (int)gridDim.x * 4;
  for (int item = (int)blockIdx.x * 4 + (threadIdx.x >> 6); item < total; item += waves) {
    const int row = plan_query(start, nq, item);
    const int64_t j = (int64_t)(item - start[row]) * PLAN_CHUNK + lane;
    bool keep = false;
    float s = 0.f;
    int64_t ix = 0;
    if (j < cnt[row]) {
      s = band_s[row * cap + j];
      ix = band[row * cap + j];
      keep = rank_ahead(s, ix, tau[row], NO_TIE);
    }
    const unsigned long long m = __ballot(keep);
    if (m == 0) continue;
    const int n = __popcll(m);
    if constexpr (!EMIT) {
      if (lane == 0) atomicAdd(len + row, n);
    } else {
      int base = 0;
      if (lane == 0) base = atomicAdd(cursor + row, n);
      base = __shfl(base, 0, 64);
      const int at = base + __popcll(m & ((1ull << lane) - 1));
      if (keep && at < len[row]) seg[src[row] + at] = composite(s, ix - offset);
    }
  }
}

// one workgroup per query over its row of the window; a wave's passing rows take consecutive slots
__global__ __launch_bounds__(256) void collect_kernel(const float* S, int64_t lds, int64_t C, int64_t r0,
                                                      const float* tau, unsigned long long* cursor,
                                                      const int64_t* end, uint64_t* seg) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const float* s = S + row * lds;
  const float t = tau[row];
  const int64_t lim = end[row];
  for (int64_t j0 = 0; j0 < C; j0 += 256) {
    const int64_t j = j0 + threadIdx.x;
    const float v = j < C ? s[j] : 0.f;
    const bool keep = j < C && rank_ahead(v, r0 + j, t, NO_TIE);
    const unsigned long long m = __ballot(keep);
    if (m == 0) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor + row, (unsigned long long)__popcll(m));
    base = __shfl(base, 0, 64);
    const int64_t at = (int64_t)base + __popcll(m & ((1ull << lane) - 1));
    if (keep && at < lim) seg[at] = composite(v, r0 + j);
  }
}

// in-place descending bitonic sort of n (a power of two) u64 in LDS, all threads of the block
// (k_search.hip's, 64-bit LDS reads and writes; from stride 32 on a wave's accesses are contiguous)
__device__ void bitonic_desc(uint64_t* a, int n) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < n / 2; t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint64_t x = a[lo], y = a[hi];
        if ((x < y) == desc) { a[lo] = y; a[hi] = x; }
      }
    }
  }
  __syncthreads();
}

// item: run [start, start + n), 2 <= n <= RANGE_RUN; padded in LDS with 0 (below every composite of
// a row) to a power of two
__global__ __launch_bounds__(1024) void sort_runs_kernel(uint64_t* seg, const RangeItem* items, int nitems) {
  __shared__ uint64_t a[RANGE_RUN];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    uint64_t* p = seg + items[it].start;
    const int n = (int)items[it].n;
    int np = 2;
    while (np < n) np <<= 1;
    for (int j = threadIdx.x; j < np; j += blockDim.x) a[j] = j < n ? p[j] : 0;
    bitonic_desc(a, np);   // starts and ends with a barrier
    for (int j = threadIdx.x; j < n; j += blockDim.x) p[j] = a[j];
    __syncthreads();
  }
}

// One pass over a segment of n > RANGE_RUN composites made of sorted runs of L (the last one
// shorter): runs 2i and 2i + 1 merge into dst, each element placed by a binary search of the other
// run (merge path; composites are distinct). A run without a partner is copied. item: segment at
// `start`, elements [aux, aux + RANGE_MERGE_CHUNK) of it.
__global__ __launch_bounds__(256) void merge_kernel(const uint64_t* src, uint64_t* dst, const RangeItem* items,
                                                    int nitems, int64_t L) {
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int64_t n = items[it].n, p1 = min(n, items[it].aux + RANGE_MERGE_CHUNK);
    const uint64_t* s = src + items[it].start;
    uint64_t* d = dst + items[it].start;
    for (int64_t p = items[it].aux + threadIdx.x; p < p1; p += 256) {
      const int64_t r = p / L, pos = p - r * L;
      const uint64_t x = s[p];
      const int64_t ob = (r ^ 1) * L, oe = min(n, ob + L);
      const bool b_side = r & 1;
      int64_t lo = 0, hi = max<int64_t>(0, oe - ob);   // elements of the other run that precede x
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t o = s[ob + mid];
        if (b_side ? o >= x : o > x) lo = mid + 1;
        else hi = mid;
      }
      d[(r & ~(int64_t)1) * L + pos + lo] = x;
    }
  }
}

// item: n composites from seg[start ..] to entries [aux, aux + n) of the result
__global__ __launch_bounds__(256) void decode_kernel(const uint64_t* seg, const RangeItem* items, int nitems,
                                                     int64_t offset, float* os, int64_t* oi) {
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const uint64_t* s = seg + items[it].start;
    const int64_t d = items[it].aux, n = items[it].n;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
      const uint64_t v = s[j];
      os[d + j] = key_float((unsigned)(v >> 32));
      oi[d + j] = offset + (int64_t)(0xFFFFFFFFu - (uint32_t)v);
    }
  }
}

unsigned item_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>(n, 1), 65535); }
}  // namespace

hipError_t range_keep_count(const float* band_s, const int64_t* band, const int* cnt, int64_t cap, const int* plan,
                            const float* tau, int64_t nq, int* len, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (cap < 1 || !plan || nq > 0x7FFFFFFF) return hipErrorInvalidValue;
  keep_kernel<false><<<RANGE_GRID, 256, 0, s>>>(band_s, band, cnt, cap, plan, (int)nq, tau, 0, len, nullptr, nullptr,
                                                nullptr);
  return hipGetLastError();
}

hipError_t range_emit(const float* band_s, const int64_t* band, const int* cnt, int64_t cap, const int* plan,
                      const float* tau, int64_t offset, int64_t nq, int* len, int* cursor, const int64_t* src,
                      uint64_t* seg, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (cap < 1 || !plan || nq > 0x7FFFFFFF) return hipErrorInvalidValue;
  keep_kernel<true><<<RANGE_GRID, 256, 0, s>>>(band_s, band, cnt, cap, plan, (int)nq, tau, offset, len, cursor, src, seg);
  return hipGetLastError();
}

hipError_t range_collect(const float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const float* tau,
                         int64_t* cursor, const int64_t* end, uint64_t* seg, hipStream_t s) {
  if (nq <= 0 || C <= 0) return hipSuccess;
  if (r0 < 0 || r0 + C > 0xFFFFFFFFll) return hipErrorInvalidValue;   // the composite holds 32 bits of row
  collect_kernel<<<(unsigned)nq, 256, 0, s>>>(scores, lds, C, r0, tau, (unsigned long long*)cursor, end, seg);
  return hipGetLastError();
}

hipError_t range_sort_runs(uint64_t* seg, const RangeItem* items, int64_t nitems, int64_t longest, hipStream_t s) {
  if (nitems <= 0) return hipSuccess;
  if (longest > RANGE_RUN || nitems > 0x7FFFFFFF) return hipErrorInvalidValue;
  // short runs (the common case: a handful of rows per query) do not need a thousand threads each
  const int nt = longest <= 512 ? 64 : longest <= 2048 ? 256 : 1024;
  sort_runs_kernel<<<item_grid(nitems), nt, 0, s>>>(seg, items, (int)nitems);
  return hipGetLastError();
}

hipError_t range_merge(const uint64_t* src, uint64_t* dst, const RangeItem* items, int64_t nitems, int64_t L,
                       hipStream_t s) {
  if (nitems <= 0) return hipSuccess;
  if (L < 1 || nitems > 0x7FFFFFFF) return hipErrorInvalidValue;
  merge_kernel<<<item_grid(nitems), 256, 0, s>>>(src, dst, items, (int)nitems, L);
  return hipGetLastError();
}

hipError_t range_decode(const uint64_t* seg, const RangeItem* items, int64_t nitems, int64_t offset, float* out_s,
                        int64_t* out_i, hipStream_t s) {
  if (nitems <= 0) return hipSuccess;
  if (nitems > 0x7FFFFFFF) return hipErrorInvalidValue;
  decode_kernel<<<item_grid(nitems), 256, 0, s>>>(seg, items, (int)nitems, offset, out_s, out_i);
  return hipGetLastError();
}

}  // namespace clm
