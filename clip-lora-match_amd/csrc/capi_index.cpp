// libclm C-ABI, the resident index: create / destroy, append, shard export / import, in-place
// removal and update, read-back and the route counters. Searching it is capi_search.cpp.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "capi_internal.hpp"

using namespace clm;
using namespace clm::capi;

extern "C" {

// ------------------------------------------------------------------ index ---
// HBM-resident cosine index behind TextSearchIndex / top_k_similar (src/embedding/search.py:
// 24-115, similarity.py:36-58). Search = an fp16 MFMA pass that bounds the candidates, then an
// exact fp64 re-score of the candidates against the caller's own rows (see clm_index_search).
int clm_index_create(int hip_device, int64_t capacity, int dim, clm_index** out) {
  if (!out || capacity < 0 || dim <= 0 || dim % 64 || dim > 65536)
    return fail(CLM_E_ARG, "bad capacity/dim (dim must be a multiple of 64, <= 65536)");
  DeviceGuard g(hip_device);
  clm_index* x = new clm_index();
  x->dev = hip_device;
  x->cap = std::max<int64_t>(capacity, 1);
  x->dim = dim;
  if (hipMalloc(&x->rows, (size_t)x->cap * dim * sizeof(u16)) != hipSuccess ||
      hipMalloc(&x->inv, (size_t)x->cap * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    if (x->rows) (void)hipFree(x->rows);
    delete x;
    return fail(CLM_E_OOM, "index allocation failed");
  }
  *out = x;
  return CLM_OK;
}

int clm_index_destroy(clm_index* x) {
  if (!x) return CLM_OK;
  DeviceGuard g(x->dev);
  (void)hipDeviceSynchronize();
  index_free_buffers(x);
  delete x;
  return CLM_OK;
}

static int index_grow(clm_index* x, int64_t need_rows) {
  if (need_rows <= x->cap) return CLM_OK;
  int64_t nc = std::max<int64_t>(need_rows, x->cap * 2);
  u16* nr = nullptr;
  float* ni = nullptr;
  float* n32 = nullptr;
  if (hipMalloc(&nr, (size_t)nc * x->dim * sizeof(u16)) != hipSuccess ||
      hipMalloc(&ni, (size_t)nc * sizeof(float)) != hipSuccess ||
      (x->rows32 && hipMalloc(&n32, (size_t)nc * x->dim * sizeof(float)) != hipSuccess)) {
    (void)hipGetLastError();
    if (nr) (void)hipFree(nr);
    if (ni) (void)hipFree(ni);
    return fail(CLM_E_OOM, "index grow failed");
  }
  HIPCHK(hipMemcpy(nr, x->rows, (size_t)x->n * x->dim * sizeof(u16), hipMemcpyDeviceToDevice));
  HIPCHK(hipMemcpy(ni, x->inv, (size_t)x->n * sizeof(float), hipMemcpyDeviceToDevice));
  if (n32) {
    HIPCHK(hipMemcpy(n32, x->rows32, (size_t)x->n * x->dim * sizeof(float), hipMemcpyDeviceToDevice));
    (void)hipFree(x->rows32);
    x->rows32 = n32;
  }
  (void)hipFree(x->rows);
  (void)hipFree(x->inv);
  x->rows = nr;
  x->inv = ni;
  x->cap = nc;
  return CLM_OK;
}

// the first fp32 rows (append, import, update): keep an fp32 copy from now on; the rows so far were
// fp16 as given
static int start_rows32(clm_index* x, hipStream_t st) {
  if (hipMalloc(&x->rows32, (size_t)x->cap * x->dim * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    x->rows32 = nullptr;
    return fail(CLM_E_OOM, "fp32 row copy allocation failed");
  }
  KCHK(f16_to_f32_rows(x->rows, x->n, (int)x->dim, x->rows32, st));
  return CLM_OK;
}

// rescore_select / topk_merge / topk_any order ties by a 32-bit image of the row's index inside
// its own index (the global offset is added after the selection, so any offset orders alike)
constexpr int64_t MAX_INDEX_ROWS = (int64_t)0xFFFFFFFF;
constexpr int64_t MAX_GLOBAL_OFFSET = (int64_t)1 << 62;

int clm_index_append(clm_index* x, const void* rows, int dtype, int64_t n, void* stream) {
  if (!x || n < 0 || (n > 0 && !rows)) return fail(CLM_E_ARG, "bad argument");
  if (dtype != CLM_F32 && dtype != CLM_F16) return fail(CLM_E_ARG, "rows must be f32 or f16");
  if (n == 0) return CLM_OK;
  if (x->n + n > MAX_INDEX_ROWS) return fail(CLM_E_ARG, "index append: one index holds fewer than 2^32 rows");
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));
  int r = index_grow(x, x->n + n);
  if (r) return r;
  x->samp_n = -1;   // the threshold sample is rebuilt from the new row set
  x->inv_keys_n = -1;
  x->res_valid = false;   // a held threshold-search result describes the previous rows
  if (dtype == CLM_F32 && !x->rows32 && (r = start_rows32(x, st))) return r;
  const size_t bytes = (size_t)n * x->dim * dtype_size(dtype);
  const void* src = rows;
  void* tmp = nullptr;
  if (!is_device_ptr(rows)) {
    if (hipMalloc(&tmp, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(CLM_E_OOM, "staging failed"); }
    HIPCHK(hipMemcpyAsync(tmp, rows, bytes, hipMemcpyHostToDevice, st));
    src = tmp;
  }
  hipError_t e = hipSuccess;
  if (x->rows32) {
    float* dst = x->rows32 + (size_t)x->n * x->dim;
    e = dtype == CLM_F32 ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)
                         : f16_to_f32_rows((const u16*)src, n, (int)x->dim, dst, st);
  }
  // fp16 MFMA operands: f32 rows are normalised first (no fp16 overflow / subnormal loss);
  // f16 rows are kept as given (exact) with the inverse norms of those rows
  if (e == hipSuccess)
    e = rows_to_f16(src, dtype == CLM_F32 ? 0 : 1, n, (int)x->dim, x->rows + (size_t)x->n * x->dim, x->inv + x->n,
                    st, dtype == CLM_F32 ? 2 : 0);
  if (tmp) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
  }
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("index append: ") + hipGetErrorString(e));
  x->n += n;
  return CLM_OK;
}

// Shard persistence (TextSearchIndex.save_shard / load_shard): the index's internal state as it
// is, so a reload skips the fp32 normalisation and fp16 rounding of every row and searches bit for
// bit as the index that was saved.
int clm_index_has_f32(const clm_index* x) { return x ? (x->rows32 != nullptr) : -1; }

static hipMemcpyKind copy_kind(const void* dst, const void* src) {
  const bool d = is_device_ptr(dst), s = is_device_ptr(src);
  return d ? (s ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) : (s ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
}

int clm_index_export(clm_index* x, int64_t start, int64_t n, uint16_t* rows16, float* inv, float* rows32,
                     void* stream) {
  if (!x || start < 0 || n < 0 || start + n > x->n || (n > 0 && (!rows16 || !inv)))
    return fail(CLM_E_ARG, "index export: bad range or null destination");
  if (rows32 && !x->rows32) return fail(CLM_E_STATE, "index export: the index keeps no fp32 rows");
  if (n == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const size_t cnt = (size_t)n * x->dim;
  HIPCHK(hipMemcpyAsync(rows16, x->rows + (size_t)start * x->dim, cnt * 2, copy_kind(rows16, x->rows), st));
  HIPCHK(hipMemcpyAsync(inv, x->inv + start, (size_t)n * 4, copy_kind(inv, x->inv), st));
  if (rows32)
    HIPCHK(hipMemcpyAsync(rows32, x->rows32 + (size_t)start * x->dim, cnt * 4, copy_kind(rows32, x->rows32), st));
  HIPCHK(hipStreamSynchronize(st));
  return CLM_OK;
}

int clm_index_import(clm_index* x, const uint16_t* rows16, const float* inv, const float* rows32, int64_t n,
                     void* stream) {
  if (!x || n < 0 || (n > 0 && (!rows16 || !inv))) return fail(CLM_E_ARG, "index import: bad argument");
  if (n == 0) return CLM_OK;
  if (x->n + n > MAX_INDEX_ROWS) return fail(CLM_E_ARG, "index import: one index holds fewer than 2^32 rows");
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));
  int r = index_grow(x, x->n + n);
  if (r) return r;
  x->samp_n = -1;
  x->inv_keys_n = -1;
  x->res_valid = false;   // a held threshold-search result describes the previous rows
  const size_t cnt = (size_t)n * x->dim;
  if (rows32 && !x->rows32 && (r = start_rows32(x, st))) return r;
  u16* d16 = x->rows + (size_t)x->n * x->dim;
  HIPCHK(hipMemcpyAsync(d16, rows16, cnt * 2, copy_kind(d16, rows16), st));
  HIPCHK(hipMemcpyAsync(x->inv + x->n, inv, (size_t)n * 4, copy_kind(x->inv, inv), st));
  if (x->rows32) {
    float* d32 = x->rows32 + (size_t)x->n * x->dim;
    if (rows32) HIPCHK(hipMemcpyAsync(d32, rows32, cnt * 4, copy_kind(d32, rows32), st));
    else KCHK(f16_to_f32_rows(d16, n, (int)x->dim, d32, st));   // fp16 rows are the caller's rows
  }
  HIPCHK(hipStreamSynchronize(st));
  x->n += n;
  return CLM_OK;
}

int64_t clm_index_size(const clm_index* x) { return x ? x->n : -1; }

int clm_index_reset(clm_index* x) {
  if (!x) return fail(CLM_E_ARG, "null index");
  x->n = 0;
  x->samp_n = -1;   // never reuse a sample of the previous rows
  x->inv_keys_n = -1;
  x->res_valid = false;   // a held threshold-search result describes the previous rows
  return CLM_OK;
}

int clm_index_set_offset(clm_index* x, int64_t off) {
  if (!x || off < 0 || off > MAX_GLOBAL_OFFSET) return fail(CLM_E_ARG, "index offset: 0 <= offset <= 2^62");
  x->offset = off;
  return CLM_OK;
}

// ---- in-place mutation (clm_index_remove / clm_index_update, k_mutate.hip) -------------------
// One staging buffer of a fixed size, whatever the index holds: removal moves the rows above the
// first removed one chunk by chunk through it, update converts the new rows into it batch by batch.
constexpr size_t MUTATE_STAGE_BYTES = (size_t)64 << 20;

static int mutate_stage(clm_index* x) {
  if (x->mut) return CLM_OK;
  if (hipMalloc(&x->mut, MUTATE_STAGE_BYTES) != hipSuccess) {
    (void)hipGetLastError();
    x->mut = nullptr;
    return fail(CLM_E_OOM, "index mutation: staging allocation failed");
  }
  return CLM_OK;
}

// rows per pass: what the staging buffer holds at row_bytes each, lowered by $CLM_MUTATE_CHUNK_ROWS
// (tests: chunk boundaries at a few thousand rows)
static int64_t mutate_chunk_rows(size_t row_bytes) {
  int64_t r = std::max<int64_t>(1, (int64_t)(MUTATE_STAGE_BYTES / row_bytes));
  const char* e = getenv("CLM_MUTATE_CHUNK_ROWS");
  if (e && atoll(e) >= 1) r = std::min<int64_t>(r, atoll(e));
  return r;
}

// the caller's global ids (host or device) as local rows on the host; CLM_E_ARG for one outside the index.
// Device ids are read in stream order on st (the caller's stream may still be writing them: a plain
// hipMemcpy runs on the null stream, which a non-blocking stream does not wait for); drains st.
static int mutate_local_ids(const clm_index* x, const int64_t* ids, int64_t n, std::vector<int64_t>& loc,
                            const char* what, hipStream_t st) {
  loc.resize((size_t)n);
  if (is_device_ptr(ids)) HIPCHK(hipMemcpyAsync(loc.data(), ids, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  else std::memcpy(loc.data(), ids, (size_t)n * 8);
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t& v : loc) {
    if (v < x->offset || v - x->offset >= x->n)
      return fail(CLM_E_ARG, std::string(what) + ": id " + std::to_string(v) + " is outside [offset, offset + size)");
    v -= x->offset;
  }
  return CLM_OK;
}

int clm_index_remove(clm_index* x, const int64_t* ids, int64_t n_ids, void* stream) {
  if (!x || n_ids < 0 || (n_ids > 0 && !ids)) return fail(CLM_E_ARG, "index remove: bad argument");
  if (n_ids == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> rem;
  int r = mutate_local_ids(x, ids, n_ids, rem, "index remove", st);
  if (r) return r;
  std::sort(rem.begin(), rem.end());
  rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
  const int64_t m = (int64_t)rem.size(), n = x->n, dim = x->dim;
  if ((r = mutate_stage(x))) return r;
  x->samp_n = -1;
  x->inv_keys_n = -1;
  x->res_valid = false;   // a held threshold-search result describes the previous rows
  int64_t* drem = nullptr;   // the sorted list on the device, for the gather's binary search
  if (hipMalloc(&drem, (size_t)m * 8) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CLM_E_OOM, "index remove: id list allocation failed");
  }
  hipError_t e = hipMemcpyAsync(drem, rem.data(), (size_t)m * 8, hipMemcpyHostToDevice, st);
  // Stable compaction of rows [rem[0], n) in stream order, R source rows at a time. A chunk's
  // survivors land at [d0, d0 + surv), d0 = s0 - (removed rows below s0): at or below their sources,
  // above every row an earlier chunk wrote and below every row a later chunk reads. Only the chunk's
  // own sources can overlap that range, so it is gathered into the staging buffer and copied down --
  // or straight to the destination once the range ends at or below s0.
  const bool has32 = x->rows32 != nullptr;
  const int64_t R = mutate_chunk_rows((size_t)dim * (has32 ? 6 : 2) + 4);
  u16* s16 = (u16*)x->mut;
  float* s32 = has32 ? (float*)((char*)x->mut + (size_t)R * dim * 2) : nullptr;
  float* sinv = (float*)((char*)x->mut + (size_t)R * dim * (has32 ? 6 : 2));
  int64_t c = 0;   // removed rows below s0
  for (int64_t s0 = rem[0]; s0 < n && e == hipSuccess; s0 += R) {
    const int64_t s1 = std::min(n, s0 + R);
    const int64_t c1 = std::lower_bound(rem.begin() + c, rem.end(), s1) - rem.begin();
    const int64_t surv = (s1 - s0) - (c1 - c), d0 = s0 - c;
    if (surv > 0) {
      u16* d16 = x->rows + (size_t)d0 * dim;
      float* d32 = has32 ? x->rows32 + (size_t)d0 * dim : nullptr;
      float* dinv = x->inv + d0;
      const bool direct = d0 + surv <= s0;
      e = gather_rows(x->rows, x->rows32, x->inv, s0, s1 - s0, (int)dim, drem + c, c1 - c, direct ? d16 : s16,
                      direct ? d32 : s32, direct ? dinv : sinv, st);
      if (!direct) {
        if (e == hipSuccess) e = hipMemcpyAsync(d16, s16, (size_t)surv * dim * 2, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && has32)
          e = hipMemcpyAsync(d32, s32, (size_t)surv * dim * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dinv, sinv, (size_t)surv * 4, hipMemcpyDeviceToDevice, st);
      }
    }
    c = c1;
  }
  const hipError_t es = hipStreamSynchronize(st);
  (void)hipFree(drem);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("index remove: ") + hipGetErrorString(e));
  x->n = n - m;
  return CLM_OK;
}

int clm_index_update(clm_index* x, const int64_t* ids, const void* rows, int dtype, int64_t n, void* stream) {
  if (!x || n < 0 || (n > 0 && (!ids || !rows))) return fail(CLM_E_ARG, "index update: bad argument");
  if (dtype != CLM_F32 && dtype != CLM_F16) return fail(CLM_E_ARG, "index update: rows must be f32 or f16");
  if (n == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> loc;
  int r = mutate_local_ids(x, ids, n, loc, "index update", st);
  if (r) return r;
  {
    std::vector<int64_t> s(loc);
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return fail(CLM_E_ARG, "index update: duplicate id");
  }
  const int64_t dim = x->dim;
  if ((r = mutate_stage(x))) return r;
  if (dtype == CLM_F32 && !x->rows32 && (r = start_rows32(x, st))) return r;
  x->samp_n = -1;   // n stays: nothing else would rebuild the sample and the order keys
  x->inv_keys_n = -1;
  x->res_valid = false;   // a held threshold-search result describes the previous rows
  // per batch of B rows, in the staging buffer: the rows as given (when they come from the host or
  // are not 16-byte aligned), their fp16 operands, their fp32 form (f16 rows into an index with the
  // fp32 copy), the local ids, the inverse norms -- converted by append's own routines, then scattered
  const bool has32 = x->rows32 != nullptr;
  const size_t esz = dtype_size(dtype);
  const int64_t B = mutate_chunk_rows((size_t)dim * 10 + 12);
  char* base = (char*)x->mut;
  void* ssrc = base;
  u16* s16 = (u16*)(base + (size_t)B * dim * 4);
  float* s32 = (float*)(base + (size_t)B * dim * 6);
  int64_t* sid = (int64_t*)(base + (size_t)B * dim * 10);
  float* sinv = (float*)(base + (size_t)B * dim * 10 + (size_t)B * 8);
  const bool dev_rows = is_device_ptr(rows);
  hipError_t e = hipSuccess;
  for (int64_t b0 = 0; b0 < n && e == hipSuccess; b0 += B) {
    const int64_t nb = std::min(B, n - b0);
    const void* src = (const char*)rows + (size_t)b0 * dim * esz;
    if (!dev_rows || ((uintptr_t)src & 15)) {
      e = hipMemcpyAsync(ssrc, src, (size_t)nb * dim * esz, dev_rows ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         st);
      src = ssrc;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(sid, loc.data() + b0, (size_t)nb * 8, hipMemcpyHostToDevice, st);
    const float* src32 = nullptr;
    if (e == hipSuccess && has32) {
      if (dtype == CLM_F32) src32 = (const float*)src;
      else {
        e = f16_to_f32_rows((const u16*)src, nb, (int)dim, s32, st);
        src32 = s32;
      }
    }
    if (e == hipSuccess)
      e = rows_to_f16(src, dtype == CLM_F32 ? 0 : 1, nb, (int)dim, s16, sinv, st, dtype == CLM_F32 ? 2 : 0);
    if (e == hipSuccess) e = scatter_rows(s16, src32, sinv, sid, 0, nb, (int)dim, x->rows, x->rows32, x->inv, st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("index update: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_index_read(clm_index* x, int64_t start, int64_t n, float* dst, void* stream) {
  if (!x || start < 0 || n < 0 || start + n > x->n || (n > 0 && !dst)) return fail(CLM_E_ARG, "bad range");
  if (n == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const size_t cnt = (size_t)n * x->dim;
  std::vector<float> f(cnt);
  if (x->rows32) {
    HIPCHK(hipMemcpyAsync(f.data(), x->rows32 + (size_t)start * x->dim, cnt * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    std::vector<u16> h(cnt);
    HIPCHK(hipMemcpyAsync(h.data(), x->rows + (size_t)start * x->dim, cnt * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 0; i < cnt; ++i) f[i] = host_f16_to_f32(h[i]);
  }
  if (is_device_ptr(dst)) {
    // on st, behind whatever the caller's stream wrote to dst before; f is freed on return
    HIPCHK(hipMemcpyAsync(dst, f.data(), cnt * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    std::memcpy(dst, f.data(), cnt * 4);
  }
  return CLM_OK;
}

int clm_index_stats(const clm_index* x, int64_t* filtered, int64_t* exact, int64_t* overflow) {
  if (!x) return fail(CLM_E_ARG, "null index");
  if (filtered) *filtered = x->search_stats[ST_BOUNDED_SAMPLED];
  if (exact) *exact = x->search_stats[ST_EXACT_SCAN] + x->search_stats[ST_BOUNDED_SCAN];
  if (overflow) *overflow = x->search_stats[ST_OVERFLOW];
  return CLM_OK;
}

int clm_index_stats2(const clm_index* x, int64_t* out, int n) {
  if (!x || !out || n < 0) return fail(CLM_E_ARG, "bad argument");
  for (int i = 0; i < n && i < ST_COUNT; ++i) out[i] = x->search_stats[i];
  return CLM_OK;
}

}  // extern "C"
