// What every unit of the C-ABI host layer shares (capi.cpp: context + encode, capi_index.cpp: the
// resident index, capi_search.cpp: search / rank / log-sum-exp, capi_ops.cpp: stand-alone ops and
// images): error reporting, device helpers, the workspace layout helper and the index itself.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>

#include "clm.h"
#include "kernels.hpp"

namespace clm {
namespace capi {

// sets the calling thread's clm_last_error text (one thread_local, in capi.cpp) and returns code
int fail(int code, const std::string& msg);

#define CLM_CHK_(x, pre)                                                                             \
  do {                                                                                               \
    hipError_t e_ = (x);                                                                             \
    if (e_ != hipSuccess) return fail(CLM_E_HIP, std::string(pre) + #x + ": " + hipGetErrorString(e_)); \
  } while (0)
#define HIPCHK(x) CLM_CHK_(x, "")
#define KCHK(x) CLM_CHK_(x, "kernel launch ")

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

bool is_device_ptr(const void* p);

// grow-only device buffer: at least `bytes`, contents not kept; CLM_E_OOM "<what> allocation failed"
int grow(void** p, size_t* cap, size_t bytes, const char* what = "search workspace");

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline size_t dtype_size(int dt) {
  switch (dt) {
    case CLM_F32: case CLM_I32: return 4;
    case CLM_F16: case CLM_BF16: return 2;
    case CLM_U8: return 1;
    case CLM_I64: return 8;
  }
  return 0;
}

inline float host_f16_to_f32(uint16_t v) {
  _Float16 h;
  std::memcpy(&h, &v, 2);
  return (float)h;
}

// Carves one workspace into buffers: take() returns each buffer's offset (256-byte aligned),
// total() the bytes to allocate -- the size and the carving come from the same calls.
struct Layout {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off = (size_t)round_up((int64_t)(off + bytes), 256); return o; }
  size_t total() const { return off; }
};

}  // namespace capi
}  // namespace clm

// The route counters of an index (clm_index::search_stats), in the order clm_index_stats2 reports them.
enum SearchStat {
  // queries served by the sampled bounded search / the bounded search with the chunked fp16 scan as
  // step 1 / the full exact scan / the overflow re-runs
  ST_BOUNDED_SAMPLED, ST_BOUNDED_SCAN, ST_EXACT_SCAN, ST_OVERFLOW,
  // queries whose filter pass ran on G2 256 x 192 / gemm_kernel 256 x 256 (dense blocks)
  ST_TILE_G2, ST_TILE_DENSE,
  ST_SMALL,   // queries served by the small-batch streaming search (search_small)
  // rank queries served by the EPI_RANK band pass / by the exact route, those of the latter whose
  // band list overflowed its capacity, band rows re-scored for the queries of ST_RANK_BAND
  ST_RANK_BAND, ST_RANK_EXACT, ST_RANK_OVERFLOW, ST_RANK_BAND_ROWS,
  // log-sum-exp queries served by the EPI_LSE pass / by the exact route, queries whose EPI_LSE band
  // list overflowed its capacity
  ST_LSE_FAST, ST_LSE_EXACT, ST_LSE_OVERFLOW,
  // threshold-search queries served by the EPI_FILTER pass / by the exact route, those whose
  // candidate list overflowed its capacity
  ST_RANGE_FAST, ST_RANGE_EXACT, ST_RANGE_OVERFLOW,
  // masked-search queries served by the pass route / the gather route / the exact route (a query of
  // the other two redone exactly counts in ST_MASK_EXACT)
  ST_MASK_PASS, ST_MASK_GATHER, ST_MASK_EXACT,
  // keyed-search queries served by the pass route / the exact route (a redone query counts in the latter)
  ST_KEY_PASS, ST_KEY_EXACT,
  // softmax-gradient queries served, and the (query block, row chunk) passes run for them
  ST_GRAD_QUERIES, ST_GRAD_PASSES,
  ST_COUNT
};

// Every device buffer below is owned by the index and released by index_free_buffers (after the
// struct), the one list of them: a new device buffer is added there.
struct clm_index {
  int dev = 0;
  int64_t cap = 0, n = 0, dim = 0, offset = 0;
  // MFMA-pass operands: fp16 rows (f16 appends: the rows as given; f32 appends: the rows
  // normalised in fp32, then rounded) + fp32 inverse norms of those fp16 rows
  u16* rows = nullptr;
  float* inv = nullptr;
  // the caller's fp32 rows, kept once any f32 rows were appended (f16 appends upcast into it):
  // the exact re-scoring reads these; without them the fp16 rows ARE the caller's rows
  float* rows32 = nullptr;
  // search workspaces (grown on demand): ws = query staging, ws2 = per-query-block buffers,
  // ws3 = chunked score matrices of the exact scans
  void* ws = nullptr; size_t ws_bytes = 0;
  void* ws2 = nullptr; size_t ws2_bytes = 0;
  void* ws3 = nullptr; size_t ws3_bytes = 0;
  // ws4 = the overflow passes' gathered queries / candidate lists (overflow_wide, exact re-scan)
  void* ws4 = nullptr; size_t ws4_bytes = 0;
  // strided row sample for the threshold pass, rebuilt when n changes
  u16* samp = nullptr; float* samp_inv = nullptr; int64_t samp_S = 0, samp_n = -1, samp_cap = 0;
  // order keys {min, max} of inv[0, n) for the filter GEMM's skip test, rebuilt with the sample
  unsigned* inv_keys = nullptr; int64_t inv_keys_n = -1;
  // staging of clm_index_remove / clm_index_update: MUTATE_STAGE_BYTES, allocated by the first of them
  void* mut = nullptr;
  int64_t search_stats[ST_COUNT] = {};
  // The held result of the last threshold search (clm_index_search_above / _rows): res_n entries
  // (exact score, global id) in CSR order, read by clm_index_search_above_read until the next
  // threshold search, reset, mutation or destroy (res_valid). rg_comp / rg_comp2: the composites it
  // is built from (the segmented sort's two buffers), rg_items: the sort / merge / decode work items.
  float* res_s = nullptr; int64_t* res_i = nullptr; int64_t res_cap = 0, res_n = 0; bool res_valid = false;
  uint64_t* rg_comp = nullptr; int64_t rg_comp_cap = 0;
  uint64_t* rg_comp2 = nullptr; int64_t rg_comp2_cap = 0;
  void* rg_items = nullptr; size_t rg_items_bytes = 0;
};

// Frees every device buffer of the index but those in `keep`: on loan or the caller's (the filtered
// search's gather route builds a temporary clm_index around gathered rows and lends it ws2 / ws3 / ws4)
inline void index_free_buffers(clm_index* x, std::initializer_list<const void*> keep = {}) {
  for (void* p : {(void*)x->rows, (void*)x->inv, (void*)x->rows32, x->ws, x->ws2, x->ws3, x->ws4, (void*)x->samp,
                  (void*)x->samp_inv, (void*)x->inv_keys, x->mut, (void*)x->res_s, (void*)x->res_i, (void*)x->rg_comp,
                  (void*)x->rg_comp2, x->rg_items})
    if (p && std::find(keep.begin(), keep.end(), p) == keep.end()) (void)hipFree(p);
}
