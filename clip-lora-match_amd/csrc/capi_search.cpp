// libclm C-ABI, searching the resident index: clm_index_search and its routes, the filtered, keyed
// and threshold searches, exact retrieval ranks, the streaming log-sum-exp and (last) the streaming
// softmax gradients with their two test hooks, after the plumbing
// they share: query staging (QueryStage), band query blocks, the exact routes' row windows, redoing
// a subset of the queries exactly (redo_subset), the overflowed lists' gathered groups (wide_groups);
// further down one row filter (RowFilter), one candidate pass (PassBufs, row_thresholds,
// sample_scores, candidate_pass), the top-k entry points' result staging
// (ResultStage) and the exact / fast router (whole_call_exact). The clm_* entry points have C linkage
// from their declarations in clm.h; the counters are named by SearchStat (capi_internal.hpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "capi_internal.hpp"

using namespace clm;
using namespace clm::capi;

namespace {

// environment knobs: set to a non-zero number / the number, or `def` when unset
bool env_flag(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
int64_t env_int(const char* name, int64_t def) { const char* e = getenv(name); return e ? atoll(e) : def; }

// the rows the exact re-scoring reads, from row r0 on: the caller's fp32 rows where the index keeps
// them, else its fp16 rows (which then ARE the caller's rows)
struct ExactRows { const void* p; bool f16; };
ExactRows exact_rows(const clm_index* x, int64_t r0 = 0) {
  return x->rows32 ? ExactRows{x->rows32 + r0 * x->dim, false} : ExactRows{x->rows + r0 * x->dim, true};
}

// result / input copies between a workspace buffer and the caller's host or device array
hipError_t copy_out(void* dst, const void* src, size_t bytes, hipStream_t st) {
  return hipMemcpyAsync(dst, src, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
}
hipError_t copy_in(void* dst, const void* src, size_t bytes, hipStream_t st) {
  return hipMemcpyAsync(dst, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
}

// The queries of one call on the device, in x->ws: as given (qsrc: uploaded when they come from the
// host), as fp32 rows (q32: qsrc itself for f32 queries, widened for f16 ones) with their fp64 norms
// (qn), room for the MFMA pass's operands (q16 / qinv, filled by stage_queries_f16 on the routes
// that run that pass), then `extra` bytes of the caller's own per-query buffers.
struct QueryStage {
  const void* qsrc; int q_dtype;
  const float* q32; double* qn;
  u16* q16; float* qinv;
  uint8_t* extra;
};
int stage_queries(clm_index* x, const void* q, int q_dtype, int64_t nq, size_t extra_bytes, hipStream_t st,
                  QueryStage* s) {
  const int dim = (int)x->dim;
  const bool q_dev = is_device_ptr(q), f32 = q_dtype == CLM_F32;
  const size_t q_src_bytes = (size_t)nq * dim * (f32 ? 4 : 2);
  Layout lay;
  const size_t o_qsrc = q_dev ? 0 : lay.take(q_src_bytes), o_q16 = lay.take((size_t)nq * dim * 2),
               o_qinv = lay.take((size_t)nq * 4), o_q32 = f32 ? 0 : lay.take((size_t)nq * dim * 4),
               o_qn = lay.take((size_t)nq * 8), o_extra = lay.take(extra_bytes);
  int r = grow(&x->ws, &x->ws_bytes, lay.total());
  if (r) return r;
  uint8_t* ws = (uint8_t*)x->ws;
  const void* qsrc = q;
  if (!q_dev) {
    HIPCHK(hipMemcpyAsync(ws + o_qsrc, q, q_src_bytes, hipMemcpyHostToDevice, st));
    qsrc = ws + o_qsrc;
  }
  const float* q32 = (const float*)qsrc;
  if (!f32) {
    KCHK(f16_to_f32_rows((const u16*)qsrc, nq, dim, (float*)(ws + o_q32), st));
    q32 = (const float*)(ws + o_q32);
  }
  *s = QueryStage{qsrc, q_dtype, q32, (double*)(ws + o_qn), (u16*)(ws + o_q16), (float*)(ws + o_qinv), ws + o_extra};
  KCHK(query_norms(s->q32, nq, dim, s->qn, st));
  return CLM_OK;
}

// fp16 operands of the MFMA pass: queries normalised, then rounded
int stage_queries_f16(const clm_index* x, const QueryStage& s, int64_t nq, hipStream_t st) {
  KCHK(rows_to_f16(s.qsrc, s.q_dtype == CLM_F32 ? 0 : 1, nq, (int)x->dim, s.q16, s.qinv, st, 2));
  return CLM_OK;
}

// Queries per block of a pass that streams the whole index once per block (the filter, rank and
// log-sum-exp GEMMs): fewer, larger blocks read the index fewer times (10 M x 512 fp16 = 10 GB per
// pass). At most $CLM_SEARCH_QB queries; with bytes_per_query > 0 the block's buffers also stay
// within $CLM_SEARCH_WS_MB (default 8192) and a quarter of the free HBM, but hold `floor` queries at
// least. Then balanced: the same number of blocks, equal sizes (multiples of 64 rows while that
// stays within the cap).
int64_t band_query_block(int64_t nq, int64_t bytes_per_query, int64_t floor) {
  static const int64_t ws_mb = env_int("CLM_SEARCH_WS_MB", 8192);
  // query-block cap ($CLM_SEARCH_QB, A/B): a block's fp16 queries are re-read from L2 by every
  // index tile; with the filter GEMM on G2 tiles 2560 beats 4096 (10 k queries: 100.5 k vs 97.7 k
  // QPS, profiles/r04_v7_search_qb_ab.txt), and the blocks are balanced (a cap of 4096 gives
  // 10 k = 3392 + 3392 + 3216 instead of 4096 + 4096 + 1808)
  static const int64_t qb_cap = std::max<int64_t>(64, env_int("CLM_SEARCH_QB", 2560));
  int64_t nqb = std::min<int64_t>(nq, qb_cap);
  if (bytes_per_query > 0) {
    size_t fr = 0, tot = 0;
    int64_t cap_b = ws_mb << 20;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) cap_b = std::min<int64_t>(cap_b, (int64_t)(fr / 4));
    else (void)hipGetLastError();
    nqb = std::min<int64_t>(nqb, std::max<int64_t>(floor, cap_b / bytes_per_query));
  }
  const int64_t nblk = (nq + nqb - 1) / nqb;
  const int64_t even = (nq + nblk - 1) / nblk;
  return std::min<int64_t>(nqb, round_up(even, 64));
}

// The exact routes' row windows (rank_exact, lse_exact; windowed as search_scan(exact) is, so no
// buffer grows with nq x N): x->ws3 holds `header` bytes of the caller's, then one [nqb, ch] window
// of esz-byte scores within a 512 MiB budget.
struct ExactWindows { int64_t ch, nqb; uint8_t* header; void* sc; };
int exact_windows(clm_index* x, int64_t nq, size_t esz, size_t header, ExactWindows* w) {
  const size_t budget = (size_t)512 << 20;
  w->ch = round_up(std::min<int64_t>(x->n, 1 << 17), 128);
  w->nqb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 4096), (int64_t)(budget / ((size_t)w->ch * esz))));
  Layout lay;
  const size_t o_head = lay.take(header), o_sc = lay.take((size_t)w->nqb * w->ch * esz);
  int r = grow(&x->ws3, &x->ws3_bytes, lay.total());
  if (r) return r;
  w->header = (uint8_t*)x->ws3 + o_head;
  w->sc = (uint8_t*)x->ws3 + o_sc;
  return CLM_OK;
}
// body(q0, nb, r0, rn, rows): queries [q0, q0 + nb) against index rows [r0, r0 + rn)
template <class Body>
int walk_exact_windows(const clm_index* x, const ExactWindows& w, int64_t nq, Body body) {
  for (int64_t q0 = 0; q0 < nq; q0 += w.nqb) {
    const int64_t nb = std::min(w.nqb, nq - q0);
    for (int64_t r0 = 0; r0 < x->n; r0 += w.ch)
      if (int r = body(q0, nb, r0, std::min(w.ch, x->n - r0), exact_rows(x, r0))) return r;
  }
  return CLM_OK;
}

// Queries `list` of a batch redone by an exact route: their rows of the `in` arrays {base, row
// bytes} are gathered into x->ws4, body(gathered in..., out...) computes the `out` arrays' rows
// there, and those are scattered back to rows `list` of the batch's arrays.
struct RowArray { const void* base; int64_t row_bytes; };
template <class Body>
int redo_subset(clm_index* x, const std::vector<int64_t>& list, std::initializer_list<RowArray> in,
                std::initializer_list<RowArray> out, const char* what, hipStream_t st, Body body) {
  if (list.empty()) return CLM_OK;
  const int64_t no = (int64_t)list.size();
  Layout lay;
  const size_t p_x = lay.take((size_t)no * 8);
  std::vector<size_t> offs;
  for (const RowArray& a : in) offs.push_back(lay.take((size_t)no * a.row_bytes));
  for (const RowArray& a : out) offs.push_back(lay.take((size_t)no * a.row_bytes));
  int r = grow(&x->ws4, &x->ws4_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws4;
  std::vector<void*> g;
  for (size_t o : offs) g.push_back(w + o);
  int64_t* gx = (int64_t*)(w + p_x);
  const RowArray *ai = in.begin(), *ao = out.begin();
  void* const* go = g.data() + in.size();
  hipError_t e = hipMemcpyAsync(gx, list.data(), (size_t)no * 8, hipMemcpyHostToDevice, st);
  for (size_t j = 0; j < in.size() && e == hipSuccess; ++j)
    e = gather_rows(ai[j].base, ai[j].row_bytes, gx, no, ai[j].row_bytes, g[j], ai[j].row_bytes, false, st);
  r = e == hipSuccess ? body(g.data(), go) : fail(CLM_E_HIP, std::string(what) + " gather: " + hipGetErrorString(e));
  for (size_t j = 0; j < out.size() && r == CLM_OK && e == hipSuccess; ++j)
    e = gather_rows(go[j], ao[j].row_bytes, gx, no, ao[j].row_bytes, const_cast<void*>(ao[j].base), ao[j].row_bytes, true, st);
  (void)hipStreamSynchronize(st);   // `list` (the source of gx) may go out of scope
  if (r) return r;
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string(what) + " scatter: " + hipGetErrorString(e));
  return CLM_OK;
}

// Overflowed candidate lists are rebuilt by one more pass with this capacity (headroom over the first
// pass's count: a different tile shape may round a score differently)
int64_t wide_capacity(int64_t count) { return count + count / 8 + 256; }
// ... in groups of at most G queries: their lists (12 B per slot, `cap` slots each) within 1 GiB,
// at most 4096. Per group the id list is uploaded (gx), the queries' rows of the `in` arrays are
// gathered into x->ws4 behind it and body(w, gathered in..., gx, g0, ng) runs; carve(lay, G) takes
// the body's own buffers from the same workspace (w + their offsets). body drains the stream before
// it returns CLM_OK (the next group rewrites gx and the buffers); every exit path drains it.
template <class Carve, class Body>
int wide_groups(clm_index* x, const std::vector<int64_t>& list, int64_t cap, std::initializer_list<RowArray> in,
                hipStream_t st, Carve carve, Body body) {
  const int64_t n = (int64_t)list.size();
  const int64_t G = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, 4096), ((int64_t)1 << 30) / (cap * 12)));
  Layout lay;
  const size_t p_x = lay.take((size_t)G * 8);
  std::vector<size_t> offs;
  for (const RowArray& a : in) offs.push_back(lay.take((size_t)G * a.row_bytes));
  carve(lay, G);
  if (int r = grow(&x->ws4, &x->ws4_bytes, lay.total())) return r;
  uint8_t* w = (uint8_t*)x->ws4;
  int64_t* gx = (int64_t*)(w + p_x);
  std::vector<void*> g;
  for (size_t o : offs) g.push_back(w + o);
  auto group = [&](int64_t g0, int64_t ng) -> int {
    HIPCHK(hipMemcpyAsync(gx, list.data() + g0, (size_t)ng * 8, hipMemcpyHostToDevice, st));
    size_t j = 0;
    for (const RowArray& a : in) KCHK(gather_rows(a.base, a.row_bytes, gx, ng, a.row_bytes, g[j++], a.row_bytes, false, st));
    return body(w, g.data(), gx, g0, ng);
  };
  int r = CLM_OK;
  for (int64_t g0 = 0; g0 < n && r == CLM_OK; g0 += G) r = group(g0, std::min(G, n - g0));
  (void)hipStreamSynchronize(st);   // `list` (the source of gx) may go out of scope
  return r;
}

}  // namespace

// The MFMA pass scores fp16 unit-rounded operands: |fp16-pass score - exact cosine| <= 2.05e-3
// (each side's rounding moves a cosine by <= 2u, u = 2^-11, plus fp32 accumulation of <= 1024
// products). Every row of the exact top-k therefore has an fp16-pass score within 2 x 2.05e-3 of
// the fp16-pass k-th best; the candidates are taken that wide (plus slack) and re-scored exactly.
constexpr float RESCORE_MARGIN = 5e-3f;
// ... while the fp32 accumulation error stays inside the slack: dim * 2^-24 <= 4.9e-4 for dim <= 8192
// (every score within 1.95e-3 + 4.9e-4 of the exact cosine, twice that < RESCORE_MARGIN). Wider
// rows are always searched by the exact scan.
constexpr int MARGIN_MAX_DIM = 8192;
constexpr int CAND_CAP = 2048;

// The rows a search may return: those of a filtered search's prepared mask words, or of a keyed
// search's keys [N] and per-query ranges lo / hi [nq]; empty: every row (the unfiltered search).
struct RowFilter {
  const uint32_t* words = nullptr;
  const int32_t *keys = nullptr, *lo = nullptr, *hi = nullptr;
  // exact scores [nb, rn] of the queries from q0 against the rows from r0: disallowed entries -> -inf
  hipError_t strike(float* sc, int64_t ld, int64_t q0, int64_t nb, int64_t r0, int64_t rn, hipStream_t st) const {
    if (words) return mask_fill(sc, ld, nb, rn, r0, words, st);
    if (keys) return key_fill(sc, ld, nb, rn, r0, keys, lo + q0, hi + q0, st);
    return hipSuccess;
  }
  // the filter pass of the query block from q0: its operands set in g, its epilogue returned
  int arm(GemmArgs& g, int64_t q0) const {
    if (words) { g.mask = words; return EPI_FILTER_MASK; }
    if (keys) { g.keys = keys; g.klo = lo + q0; g.khi = hi + q0; return EPI_FILTER_KEYS; }
    return EPI_FILTER;
  }
};

// Chunked scan: score chunks [nqb, ch] -- fp16 MFMA (EPI_SCORE GEMM) or exact fp64 cosines
// (exact_scores) -- radix top-k per chunk row, merge of the chunk lists. Any k <= 1024, any N.
// allow (exact scan only): the rows open to each query. Every window's disallowed entries become
// -inf before its top-k (RowFilter::strike), so they sort behind every allowed row
static int search_scan(clm_index* x, bool exact, const u16* q16, const float* qinv, const float* q32,
                       const double* qn, int64_t nq, int k, float* osc, int64_t* oix, hipStream_t st,
                       const RowFilter& allow = RowFilter{}) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  const size_t budget = (size_t)512 << 20;
  const int64_t max_chunks = std::max<int64_t>(1, 8192 / k);
  int64_t ch = 1;
  if (N > 0) {
    ch = std::max<int64_t>((N + max_chunks - 1) / max_chunks, std::min<int64_t>(N, 1 << 17));
    ch = round_up(ch, 128);
  }
  const int64_t nchunks = N > 0 ? (N + ch - 1) / ch : 0;
  int64_t nqb = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(budget / ((size_t)ch * 4))));
  nqb = std::min<int64_t>(nqb, 4096);
  Layout lay;
  const size_t o_sc = lay.take((size_t)nqb * ch * 4);
  const size_t o_cs = lay.take((size_t)nqb * std::max<int64_t>(nchunks, 1) * k * 4);
  const size_t o_ci = lay.take((size_t)nqb * std::max<int64_t>(nchunks, 1) * k * 8);
  int r = grow(&x->ws3, &x->ws3_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws3;
  float* sc = (float*)(w + o_sc);
  float* cs = (float*)(w + o_cs);
  int64_t* ci = (int64_t*)(w + o_ci);
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    if (N == 0) {
      KCHK(topk_rows(sc, 1, nb, 0, k, 0, osc + q0 * k, oix + q0 * k, k, st));
      continue;
    }
    for (int64_t c = 0; c < nchunks; ++c) {
      const int64_t r0 = c * ch, rn = std::min(ch, N - r0);
      if (exact) {
        const ExactRows er = exact_rows(x, r0);
        KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, sc, ch, st));
        KCHK(allow.strike(sc, ch, q0, nb, r0, rn, st));
      } else {
        GemmArgs ga{};
        ga.A = q16 + q0 * dim; ga.lda = dim; ga.W = x->rows + r0 * dim; ga.ldw = dim;
        ga.M = (int)nb; ga.N = (int)rn; ga.K = dim; ga.out = sc; ga.ldo = ch;
        ga.rscale = qinv + q0; ga.cscale = x->inv + r0;
        KCHK(gemm(false, EPI_SCORE, ga, st));
      }
      if (nchunks == 1) {
        KCHK(topk_rows(sc, ch, nb, rn, k, x->offset + r0, osc + q0 * k, oix + q0 * k, k, st));
      } else {
        KCHK(topk_rows(sc, ch, nb, rn, k, x->offset + r0, cs + c * k, ci + c * k, nchunks * k, st));
      }
    }
    if (nchunks > 1) KCHK(topk_merge(cs, ci, nb, (int)nchunks, k, k, osc + q0 * k, oix + q0 * k, st));
  }
  return CLM_OK;
}

// Exact scan for k > 1024 (torch.topk of search.py:98 / similarity.py:57 takes any k <= N): every
// row of a query block scored exactly into one [nqb, N] matrix, then topk_any (exact k-th key,
// collection, LDS run sort + merge passes). The block is sized so the scores and topk_any's
// workspace stay within a 1 GiB budget (at least one query).
static int search_scan_large(clm_index* x, const float* q32, const double* qn, int64_t nq, int k, float* osc,
                             int64_t* oix, hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  const size_t budget = (size_t)1 << 30;
  const size_t per_q = (size_t)std::max<int64_t>(N, 1) * 4 + topk_any_ws_bytes(1, k);
  int64_t nqb = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(budget / per_q)));
  nqb = std::min<int64_t>(nqb, 65535);
  Layout lay;
  const size_t o_sc = lay.take((size_t)nqb * std::max<int64_t>(N, 1) * 4);
  const size_t o_ws = lay.take(topk_any_ws_bytes(nqb, k));
  int r = grow(&x->ws3, &x->ws3_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws3;
  float* sc = (float*)(w + o_sc);
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    if (N > 0) {
      const ExactRows er = exact_rows(x);
      KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, N, dim, sc, N, st));
    }
    KCHK(topk_any(sc, std::max<int64_t>(N, 1), nullptr, 0, nb, N, k, x->offset, osc + q0 * k, oix + q0 * k, k,
                  w + o_ws, st));
  }
  return CLM_OK;
}

// The filter GEMM's cscale bounds (GemmArgs::cbound) for the current rows, computed once per row set
// on the stream; null when the 8 bytes cannot be had. (The rank and log-sum-exp routers read them
// to see a non-finite inverse norm.)
static const unsigned* inv_keys_get(clm_index* x, hipStream_t st) {
  if (!x->inv_keys && hipMalloc(&x->inv_keys, 2 * sizeof(unsigned)) != hipSuccess) {
    (void)hipGetLastError();
    x->inv_keys = nullptr;
    return nullptr;
  }
  if (x->inv_keys_n != x->n) {
    if (value_bounds(x->inv, x->n, x->inv_keys, st) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    x->inv_keys_n = x->n;
  }
  return x->inv_keys;
}
// ... for the search's filter passes: null (no skip test) when $CLM_FILTER_SKIP=0 (A/B)
static const unsigned* inv_keys_of(clm_index* x, hipStream_t st) {
  static const bool on = env_int("CLM_FILTER_SKIP", 1) != 0;
  return on ? inv_keys_get(x, st) : nullptr;
}

// Arguments of a GEMM that streams the whole index once for nb queries in M-fastest tile order
// (EPI_FILTER / _RANK / _LSE): fp16-pass scores against theta[q], the rows that pass appended to
// cand_i (capacity `cap` per query) and counted in cnt
static GemmArgs index_pass(const clm_index* x, const u16* q16, const float* qinv, int64_t nb, const float* theta,
                           int* cnt, int64_t* cand_i, int64_t cap) {
  GemmArgs g{};
  g.A = q16; g.lda = x->dim; g.W = x->rows; g.ldw = x->dim;
  g.M = (int)nb; g.N = (int)x->n; g.K = (int)x->dim;
  g.rscale = qinv; g.cscale = x->inv;
  g.theta = theta; g.theta_ld = 1;
  g.cnt = cnt; g.cand_i = cand_i; g.cap = (int)cap; g.base = x->offset;
  g.m_fastest = 1;
  return g;
}

// Whether every inverse norm of the index is finite and positive (NaN fails both tests): 0 is the
// inverse of an infinite norm (an fp16 row holding inf), whose fp16-pass score is NaN like a zero
// row's. *keys_out (if asked for): the device keys (inv_keys_get). Drains the stream: the callers'
// own reads queued before it are complete too.
static int inv_norms_finite(clm_index* x, hipStream_t st, bool* ok, const unsigned** keys_out = nullptr) {
  unsigned hkeys[2] = {0, 0};
  const unsigned* keys = inv_keys_get(x, st);
  if (keys) HIPCHK(hipMemcpyAsync(hkeys, keys, sizeof(hkeys), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *ok = keys && key_float(hkeys[0]) > 0.f && key_float(hkeys[1]) <= 3.4028235e38f;
  if (keys_out) *keys_out = keys;
  return CLM_OK;
}

// The tile config of a filter pass whose lists are long (overflowed, or estimated to): appends
// dominate such a pass, where gemm_kernel's 256 x 256 FILTER epilogue beats G2's (near-duplicate leg
// 73.7 k vs 66.0 k QPS, profiles/r04_v7_neardup_ab.txt); -1 (the heuristic's) under $CLM_GEMM_CFG
static int dense_cfg() { static const int cfg = getenv("CLM_GEMM_CFG") ? -1 : 1; return cfg; }

// Overflowed queries, wide path: their fp16 rows, inverse norms, fp32 rows, norms and filter
// thresholds are gathered (wide_groups), the EPI_FILTER GEMM streams the index once more for just
// them with a capacity of cap[j] (the first pass's count plus headroom), and rescore_wide + topk_merge
// pick the exact top k from the whole list; results are scattered back to the queries' rows. Queries
// whose list still exceeds its capacity are appended to `full` (the exact scan redoes them).
static int overflow_wide(clm_index* x, const std::vector<int64_t>& qs, const std::vector<int64_t>& cap,
                         const QueryStage& q, const float* th, int k, float* osc, int64_t* oix,
                         std::vector<int64_t>& full, hipStream_t st) {
  const int dim = (int)x->dim;
  const ExactRows xr = exact_rows(x);
  int64_t cap_max = 0;
  for (int64_t c : cap) cap_max = std::max(cap_max, c);
  cap_max = round_up(cap_max, RESCORE_WIDE_CHUNK);
  const int64_t nch = cap_max / RESCORE_WIDE_CHUNK;
  size_t p_cnt, p_cs, p_ci, p_ps, p_pi, p_s, p_i;
  return wide_groups(   // gathered: in[0] = q16, [1] = qinv, [2] = q32, [3] = qn, [4] = th
      x, qs, cap_max, {{q.q16, (int64_t)dim * 2}, {q.qinv, 4}, {q.q32, (int64_t)dim * 4}, {q.qn, 8}, {th, 4}}, st,
      [&](Layout& lay, int64_t G) {
        p_cnt = lay.take((size_t)G * 4); p_cs = lay.take((size_t)G * cap_max * 4); p_ci = lay.take((size_t)G * cap_max * 8);
        p_ps = lay.take((size_t)G * nch * k * 4); p_pi = lay.take((size_t)G * nch * k * 8);
        p_s = lay.take((size_t)G * k * 4); p_i = lay.take((size_t)G * k * 8);
      },
      [&](uint8_t* w, void* const* in, const int64_t* gx, int64_t g0, int64_t ng) -> int {
        int* cnt = (int*)(w + p_cnt);
        float* gs = (float*)(w + p_s);
        int64_t* gi = (int64_t*)(w + p_i);
        HIPCHK(hipMemsetAsync(cnt, 0, (size_t)ng * 4, st));
        GemmArgs gf = index_pass(x, (const u16*)in[0], (const float*)in[1], ng, (const float*)in[4], cnt,
                                 (int64_t*)(w + p_ci), cap_max);
        gf.cand_s = (float*)(w + p_cs);
        gf.cbound = inv_keys_of(x, st);
        KCHK(gemm_cfg(false, EPI_FILTER, dense_cfg(), gf, st));
        KCHK(rescore_wide((const int64_t*)(w + p_ci), cnt, cap_max, (const float*)in[2], (const double*)in[3], dim, xr.p,
                          xr.f16, x->offset, ng, k, (float*)(w + p_ps), (int64_t*)(w + p_pi), st));
        KCHK(topk_merge((const float*)(w + p_ps), (const int64_t*)(w + p_pi), ng, (int)nch, k, k, gs, gi, st));
        std::vector<int> hcnt(ng);
        HIPCHK(hipMemcpyAsync(hcnt.data(), cnt, (size_t)ng * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // scatter the complete lists' results; a list past its capacity goes to the exact scan
        std::vector<int64_t> rows_ok;
        for (int64_t j = 0; j < ng; ++j) {
          if (hcnt[j] > cap_max) full.push_back(qs[g0 + j]);
          else rows_ok.push_back(j);
        }
        if (rows_ok.size() == (size_t)ng) {
          KCHK(gather_rows(gs, (int64_t)k * 4, gx, ng, (int64_t)k * 4, osc, (int64_t)k * 4, true, st));
          KCHK(gather_rows(gi, (int64_t)k * 8, gx, ng, (int64_t)k * 8, oix, (int64_t)k * 8, true, st));
        } else {
          for (int64_t j : rows_ok) {
            const int64_t dst = qs[g0 + j];
            HIPCHK(hipMemcpyAsync(osc + dst * k, gs + j * k, (size_t)k * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(oix + dst * k, gi + j * k, (size_t)k * 8, hipMemcpyDeviceToDevice, st));
          }
        }
        HIPCHK(hipStreamSynchronize(st));   // gx is rewritten by the next group
        return CLM_OK;
      });
}

// Candidate lists that overflowed CAND_CAP (queries `overflow`, first-pass counts `ocount`): rebuilt
// whole by a second filter pass (overflow_wide) or redone by the exact scan (search_bounded,
// search_small). th: every query's filter threshold. `exact`: further queries for that one exact scan.
static int finish_overflow(clm_index* x, const std::vector<int64_t>& overflow, const std::vector<int64_t>& ocount,
                           const QueryStage& qs, const float* th, int k, float* osc, int64_t* oix, hipStream_t st,
                           const std::vector<int64_t>* exact = nullptr) {
  int r;
  // Candidate lists beyond CAND_CAP (near-duplicate rows inside the window). Lists of up to
  // (SORT_MAX / k) chunks are rebuilt whole by a second filter pass over just those queries and
  // re-scored chunk-wise (overflow_wide); longer ones are redone by the exact scan, all of them in
  // ONE scan (the index is streamed once per query block of search_scan, not once per query).
  x->search_stats[ST_OVERFLOW] += (int64_t)overflow.size();
  std::vector<int64_t> wide, wcount, full;
  if (exact) full = *exact;
  for (size_t j = 0; j < overflow.size(); ++j) {
    const int64_t cap2 = wide_capacity(ocount[j]);
    if ((cap2 + RESCORE_WIDE_CHUNK - 1) / RESCORE_WIDE_CHUNK * k <= 8192) {
      wide.push_back(overflow[j]);
      wcount.push_back(cap2);
    } else {
      full.push_back(overflow[j]);
    }
  }
  if (!wide.empty() && (r = overflow_wide(x, wide, wcount, qs, th, k, osc, oix, full, st))) return r;
  // the rest redone by the exact scan, all of them in ONE scan; their rows of osc / oix are replaced
  // (x->ws4: overflow_wide is done with it, it drains its stream)
  return redo_subset(x, full, {{qs.q32, x->dim * 4}, {qs.qn, 8}}, {{osc, (int64_t)k * 4}, {oix, (int64_t)k * 8}}, "overflow",
                     st, [&](void* const* in, void* const* out) -> int {
                       return search_scan(x, true, nullptr, nullptr, (const float*)in[0], (const double*)in[1],
                                          (int64_t)full.size(), k, (float*)out[0], (int64_t*)out[1], st);
                     });
}

// ---- what the candidate passes share (search_bounded, search_small, masked_pass, keyed_pass) ----
// $CLM_KTH_RADIX=1: the sampled thresholds through topk_rows (A/B, tests)
static const bool g_kth_radix = env_flag("CLM_KTH_RADIX");
// k-th values by one streaming pass (kth_thresholds and its fp16 variants)
static bool kth_one_pass(int k) { return k <= 8 && !g_kth_radix; }

// The buffers of a candidate pass over nq queries in blocks of nqb: a block's top-k scratch (ts / ti)
// and candidate lists (cs / ci, CAND_CAP slots per query), every query's threshold (the overflow pass
// reuses them) and count (read once, after the last block). take() from the Layout, bind() once grown.
struct PassBufs {
  size_t o_ts, o_ti, o_th, o_cnt, o_cs, o_ci;
  float* ts; int64_t* ti; float* th; int* cnt; float* cs; int64_t* ci;
  void take(Layout& lay, int64_t nq, int64_t nqb, int k) {
    o_ts = lay.take((size_t)nqb * k * 4); o_ti = lay.take((size_t)nqb * k * 8);
    o_th = lay.take((size_t)nq * 4); o_cnt = lay.take((size_t)nq * 4);
    o_cs = lay.take((size_t)nqb * CAND_CAP * 4); o_ci = lay.take((size_t)nqb * CAND_CAP * 8);
  }
  void bind(void* ws) {
    uint8_t* w = (uint8_t*)ws;
    ts = (float*)(w + o_ts); ti = (int64_t*)(w + o_ti); th = (float*)(w + o_th); cnt = (int*)(w + o_cnt);
    cs = (float*)(w + o_cs); ci = (int64_t*)(w + o_ci);
  }
};

// th[q] = (k-th largest of row q of the scores [nb, C], row stride ld) - RESCORE_MARGIN: one
// streaming pass (one_pass, where kth_one_pass(k)), else topk_rows into b's scratch + filter_thresholds
static int row_thresholds(const float* sc, int64_t ld, int64_t nb, int64_t C, int k, bool one_pass, const PassBufs& b,
                          float* th, hipStream_t st) {
  if (one_pass) {
    KCHK(kth_thresholds(sc, ld, nb, C, k, RESCORE_MARGIN, th, st));
  } else {
    KCHK(topk_rows(sc, ld, nb, C, k, 0, b.ts, b.ti, k, st));
    KCHK(filter_thresholds(b.ts, k, nb, k, RESCORE_MARGIN, th, st));
  }
  return CLM_OK;
}

// The threshold sample's size: the k-th best of S rows sampled from `rows` ranks ~k * rows / S = div
// among them, so ~div candidates per query; 8192 rows at least, a multiple of 256
static int64_t sample_size(int k, int64_t rows, int64_t div = 256) {
  return round_up(std::max<int64_t>(8192, (int64_t)k * rows / div), 256);
}
// whether the masked / keyed pass route can serve the call (fin: inv_norms_finite)
static bool filter_pass_ok(const clm_index* x, bool fin, int k) {
  return fin && k <= 256 && x->dim <= MARGIN_MAX_DIM && x->n <= 0x7FFFFFFF;
}

// fp16-pass scores [nb, S] (row stride ld) of the nb queries from q0 against S sample rows s16 with
// inverse norms sinv. out16: 0 fp32 scores, 1 fp16, 2 fp16 maxima of groups of 4 rows (config 1,
// 256 x 256: the group layout's tile)
static hipError_t sample_scores(const QueryStage& qs, int64_t q0, int64_t nb, int dim, const u16* s16, const float* sinv,
                                int64_t S, void* sc, int64_t ld, int out16, hipStream_t st) {
  GemmArgs ga{};
  ga.A = qs.q16 + q0 * dim; ga.lda = dim; ga.W = s16; ga.ldw = dim;
  ga.M = (int)nb; ga.N = (int)S; ga.K = dim; ga.out = sc; ga.ldo = ld; ga.out16 = out16;
  ga.rscale = qs.qinv + q0; ga.cscale = sinv;
  return gemm_cfg(false, EPI_SCORE, out16 == 2 ? 1 : -1, ga, st);
}

// The candidate pass over the staged queries, block by block behind one memset of the counts: the
// filter GEMM (index_pass against b.th, the filter's epilogue and operands, the tile config that
// cfg(q0, nb, args) returns) lists the block's candidates, rescore_select writes its exact top k.
// Then every count comes to the host (hcnt; drains the stream): what is overflowed or short is the caller's rule.
template <class Cfg>
static int candidate_pass(clm_index* x, const QueryStage& qs, int64_t nq, int64_t nqb, int k, const RowFilter& allow,
                          const PassBufs& b, float* osc, int64_t* oix, std::vector<int>& hcnt, hipStream_t st, Cfg cfg) {
  const int dim = (int)x->dim;
  const ExactRows xr = exact_rows(x);
  HIPCHK(hipMemsetAsync(b.cnt, 0, (size_t)nq * 4, st));
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    GemmArgs gf = index_pass(x, qs.q16 + q0 * dim, qs.qinv + q0, nb, b.th + q0, b.cnt + q0, b.ci, CAND_CAP);
    gf.cand_s = b.cs;
    gf.cbound = inv_keys_of(x, st);
    const int epi = allow.arm(gf, q0), config = cfg(q0, nb, gf);
    KCHK(gemm_cfg(false, epi, config, gf, st));
    KCHK(rescore_select(b.cs, b.ci, b.cnt + q0, CAND_CAP, qs.q32 + q0 * dim, qs.qn + q0, dim, xr.p, xr.f16, x->offset,
                        RESCORE_MARGIN, nb, k, osc + q0 * k, oix + q0 * k, st));
  }
  hcnt.resize(nq);
  HIPCHK(hipMemcpyAsync(hcnt.data(), b.cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return CLM_OK;
}
static int heuristic_cfg(int64_t, int64_t, GemmArgs&) { return -1; }

// Bounded search (large N), per block of queries:
//  1. theta[q] <= the fp16-pass k-th best score of q:
//     sampled (k <= 256, N >= 4S): the k-th best over a strided sample of S rows -- a subset
//       of the index, so never above the true fp16-pass k-th best;
//     otherwise: the chunked fp16 scan's k-th best itself.
//  2. the EPI_FILTER GEMM streams the whole index once (M-fastest tile order: each index tile
//     is read once and shared by all query tiles) and appends every (score, row) with
//     score >= theta[q] - RESCORE_MARGIN to q's candidate list (capacity CAND_CAP): a
//     superset of the exact top-k.
//  3. rescore_select: candidates within the margin of their k-th are re-scored exactly against
//     the caller's rows, sorted (score desc, index asc), top k written.
//  Lists that overflowed CAND_CAP are redone by the full exact scan.
static int search_bounded(clm_index* x, bool sampled, int64_t S, const QueryStage& qs, int64_t nq, int k, float* osc,
                          int64_t* oix, hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  int r;
  if (sampled && (x->samp_n != N || x->samp_S != S)) {
    if (x->samp_cap < S) {
      if (x->samp) (void)hipFree(x->samp);
      if (x->samp_inv) (void)hipFree(x->samp_inv);
      x->samp = nullptr; x->samp_inv = nullptr; x->samp_cap = 0;
      if (hipMalloc(&x->samp, (size_t)S * dim * 2) != hipSuccess || hipMalloc(&x->samp_inv, (size_t)S * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CLM_E_OOM, "sample allocation failed");
      }
      x->samp_cap = S;
    }
    KCHK(sample_rows(x->rows, x->inv, N, dim, S, x->samp, x->samp_inv, st));
    x->samp_n = N;
    x->samp_S = S;
  }
  // the sample-score rows' stride: S (a multiple of 256 floats, 1 KB) plus 256 B, so the score
  // GEMM's 16-row column stores do not land every row at the same power-of-two address offset
  // ($CLM_SAMPLE_PAD floats, A/B)
  static const int64_t spad = env_int("CLM_SAMPLE_PAD", 64);
  const int64_t ldS = S + spad;
  // the sampled path's block is bounded by its sample-score matrix (nqb x S fp32), 256 queries at least
  const int64_t nqb = band_query_block(nq, sampled ? ldS * 4 : 0, 256);
  Layout lay;
  // fp16 sample scores (rounded toward -inf: the k-th largest over them is <= the fp32 one, so
  // the thresholds only widen) where the one-pass k-th value path runs: half the bytes of the
  // phase's three passes ($CLM_SAMPLE_F32=1: fp32, A/B)
  static const bool s32_env = env_flag("CLM_SAMPLE_F32");
  const bool s16 = sampled && kth_one_pass(k) && !s32_env;
  // ... and stored as the maxima of groups of 4 sample rows (a subset of the scores: its k-th
  // largest is at most theirs, so θ stays a lower bound; 4x fewer bytes again). The dense-tile
  // estimate then counts groups, times 4 (an upper bound of the scores >= θ).
  // ($CLM_SAMPLE_GROUP=0: every score, A/B)
  static const bool grp_env = env_int("CLM_SAMPLE_GROUP", 1) != 0;
  const bool sgrp = s16 && grp_env && S % 256 == 0;
  const int64_t Sc = sgrp ? S / 4 : S;             // stored values per sample-score row
  const int64_t ldC = sgrp ? S / 4 + 64 : ldS;     // their row stride
  const size_t o_sc = sampled ? lay.take((size_t)nqb * ldC * (s16 ? 2 : 4)) : 0;
  const size_t o_est = lay.take((size_t)nq * 4);
  PassBufs b;
  b.take(lay, nq, nqb, k);
  if ((r = grow(&x->ws2, &x->ws2_bytes, lay.total()))) return r;
  b.bind(x->ws2);
  float* sc = (float*)((uint8_t*)x->ws2 + o_sc);
  int* est = (int*)((uint8_t*)x->ws2 + o_est);
  float* th = b.th;
  // Phase 1, every block: the per-query thresholds (and, sampled, the estimated candidate counts)
  // -- no host round trip between blocks
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    if (sampled) {
      KCHK(sample_scores(qs, q0, nb, dim, x->samp, x->samp_inv, S, sc, ldC, sgrp ? 2 : s16 ? 1 : 0, st));
      if (s16) {
        KCHK(kth_thresholds16((const u16*)sc, ldC, nb, Sc, k, RESCORE_MARGIN, th + q0, st));
        KCHK(count_ge16((const u16*)sc, ldC, nb, Sc, th + q0, est + q0, st));
      } else {
        if ((r = row_thresholds(sc, ldS, nb, S, k, kth_one_pass(k), b, th + q0, st))) return r;
        KCHK(count_ge(sc, ldS, nb, S, th + q0, est + q0, st));
      }
    } else {
      if ((r = search_scan(x, false, qs.q16 + q0 * dim, qs.qinv + q0, nullptr, nullptr, nb, k, b.ts, b.ti, st))) return r;
      KCHK(filter_thresholds(b.ts, k, nb, k, RESCORE_MARGIN, th + q0, st));
    }
  }
  // Filter tile per block, from the block's own data: when most of its queries' candidate windows
  // hold more than CAND_CAP rows (near-duplicate rows: the sampled count above the threshold,
  // scaled by N / S), the appends dominate the pass and gemm_kernel's 256 x 256 FILTER epilogue is
  // the faster one (dense_cfg); otherwise G2's 256 x 192 (same candidates either way)
  std::vector<int> hest, hcnt;
  if (sampled) {
    hest.resize(nq);
    HIPCHK(hipMemcpyAsync(hest.data(), est, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // never clm_debug_set / $CLM_GEMM_DEBUG (those drop epilogues: the candidate lists would be
  // empty and the top-k wrong); the filter pass's own timing knob is $CLM_SEARCH_EPI_DEBUG,
  // read by tools only, whose results are discarded
  static const int search_dbg = (int)env_int("CLM_SEARCH_EPI_DEBUG", 0) & 3;
  // Phase 2, every block: the filter pass and the exact re-score of its candidates
  r = candidate_pass(x, qs, nq, nqb, k, RowFilter{}, b, osc, oix, hcnt, st, [&](int64_t q0, int64_t nb, GemmArgs& gf) {
    bool dense = false;
    if (sampled) {
      int64_t over = 0;
      for (int64_t i = 0; i < nb; ++i) over += (double)hest[q0 + i] * (sgrp ? 4.0 : 1.0) * ((double)N / (double)S) > CAND_CAP;
      dense = 2 * over > nb;
    }
    gf.debug = search_dbg;
    x->search_stats[dense ? ST_TILE_DENSE : ST_TILE_G2] += nb;
    return dense ? dense_cfg() : -1;
  });
  if (r) return r;
  std::vector<int64_t> overflow, ocount;
  for (int64_t i = 0; i < nq; ++i)
    if (hcnt[i] > CAND_CAP) {
      overflow.push_back(i);
      ocount.push_back(hcnt[i]);
    }
  x->search_stats[sampled ? ST_BOUNDED_SAMPLED : ST_BOUNDED_SCAN] += nq - (int64_t)overflow.size();
  if (overflow.empty()) return CLM_OK;
  return finish_overflow(x, overflow, ocount, qs, th, k, osc, oix, st);
}

// Small query batches (nq <= 16) on a large index -- the reference's own pattern, one query per
// search_with_embedding call (search.py:93-99, seeker_service.py:183-186). The bounded search's
// MFMA filter pads such a batch to 256-row query tiles (>= 94 % padding) and its sampled-threshold
// phase adds a second GEMM; here the index is streamed ONCE (scan16: fp16-pass scores of every row
// into [N, ldq], ldq = nq rounded up to a power of two, + each 256-row chunk's maximum), then
//  1. th[q] = (k-th largest chunk maximum of q) - RESCORE_MARGIN: k chunks whose maxima are >= the
//     k-th largest hold k distinct rows, so it is <= the fp16-pass k-th best, a lower bound like
//     the sampled threshold (search_bounded step 1);
//  2. collect_ge appends every (score, row) >= th[q] (CAND_CAP per query; ~k + the rows within the
//     margin), 4 bytes per stored score read once;
//  3. rescore_select: exact fp64 re-score and (score desc, index asc) top k -- the same routine and
//     bits as every other path. Lists past CAND_CAP go through finish_overflow.
// Needs nchunk >= k (N >= 256 k) and the score matrix's offsets within one buffer descriptor.
// from this many rows on, a small batch takes search_small by default (below it the full exact
// scan is as fast: ~1.9 ms per query per 1 M rows at 512 dims against ~0.1 ms + launches)
constexpr int64_t SMALL_MIN_ROWS = 65536;
static bool search_small_fits(const clm_index* x, int64_t nq, int k) {
  const int64_t N = x->n, dim = x->dim;
  const int64_t nchunk = (N + 255) / 256;
  return nq >= 1 && nq <= 16 && k >= 1 && k <= 1024 && dim >= 64 && dim <= 1024 && dim % 64 == 0 && nchunk >= k &&
         (nq - 1) * nchunk * 4 + 4 <= 0x7FFFFFF0LL;
}

static int search_small(clm_index* x, const QueryStage& qs, int64_t nq, int k, float* osc, int64_t* oix,
                        hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  const int64_t nchunk = (N + 255) / 256;
  int64_t ldq = 1;   // scores per index row, a power of two >= nq
  while (ldq < nq) ldq *= 2;
  Layout lay;
  const size_t o_sc = lay.take((size_t)N * ldq * 4);
  const size_t o_cm = lay.take((size_t)nq * nchunk * 4);
  PassBufs b;   // one block of all nq queries
  b.take(lay, nq, nq, k);
  const int64_t W = scan16_waves(nchunk, dim);   // k <= 8: every wave's 8 largest chunk maxima
  const int64_t ldw = W * 8;
  const size_t o_wt = lay.take((size_t)nq * ldw * 4);
  int r = grow(&x->ws2, &x->ws2_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws2;
  b.bind(w);
  float* sc = (float*)(w + o_sc);
  float* cm = (float*)(w + o_cm);
  float* wt = (float*)(w + o_wt);
  Scan16Args a{};
  a.rows = x->rows; a.inv = x->inv; a.N = N; a.dim = dim;
  a.q16 = qs.q16; a.qinv = qs.qinv; a.nq = (int)nq;
  a.out = sc; a.ldo = ldq; a.cmax = cm; a.nchunk = nchunk;
  const bool wave_top = kth_one_pass(k) && W * 8 >= k;
  a.wtop = wave_top ? wt : nullptr; a.ldw = ldw;
  KCHK(scan16(a, st));
  // the k-th largest of the waves' top-8 lists = the k-th largest chunk maximum
  if ((r = wave_top ? row_thresholds(wt, ldw, nq, ldw, k, true, b, b.th, st)
                    : row_thresholds(cm, nchunk, nq, nchunk, k, false, b, b.th, st)))
    return r;
  HIPCHK(hipMemsetAsync(b.cnt, 0, (size_t)nq * 4, st));
  KCHK(collect_ge(sc, (int)ldq, (int)nq, N, b.th, b.cnt, CAND_CAP, b.cs, b.ci, x->offset, st));
  const ExactRows xr = exact_rows(x);
  KCHK(rescore_select(b.cs, b.ci, b.cnt, CAND_CAP, qs.q32, qs.qn, dim, xr.p, xr.f16, x->offset, RESCORE_MARGIN, nq, k,
                      osc, oix, st));
  std::vector<int> hcnt(nq);
  HIPCHK(hipMemcpyAsync(hcnt.data(), b.cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // fewer than k candidates although the index holds k rows (nchunk >= k): scores that are NaN (a
  // zero or non-finite query; fewer than k rows with a finite norm) never pass score >= th, and
  // no threshold describes such a top-k: the exact scan, which defines the result, serves it
  std::vector<int64_t> overflow, ocount, degenerate;
  for (int64_t i = 0; i < nq; ++i)
    if (hcnt[i] > CAND_CAP) {
      overflow.push_back(i);
      ocount.push_back(hcnt[i]);
    } else if (hcnt[i] < k) {
      degenerate.push_back(i);
    }
  x->search_stats[ST_SMALL] += nq - (int64_t)overflow.size() - (int64_t)degenerate.size();
  x->search_stats[ST_EXACT_SCAN] += (int64_t)degenerate.size();
  if (overflow.empty() && degenerate.empty()) return CLM_OK;
  return finish_overflow(x, overflow, ocount, qs, b.th, k, osc, oix, st, &degenerate);
}

// Top-k by EXACT cosine (the fp32-rounded fp64 cosine of the caller's query and rows), order
// (score desc, index asc). The reference ranks fp32 dot products of fp32-normalised rows
// (search.py:36,68,93,96-99), i.e. the same scores to within its own fp32 summation error.
//  * small problems (nq * N <= 2^24 dot products, or $CLM_SEARCH_FULL=1): the exact scan;
//  * otherwise (or $CLM_SEARCH_BOUNDED=1) search_bounded, sampled when the index is large
//    enough for sampling to pay ($CLM_SEARCH_EXACT=1 forces the chunked fp16 scan for step 1).
// (search_route: the routes, for queries already staged -- clm_index_search's, and the filtered
// search's gather route on its temporary index)
// small_max: up to this many dot products the exact scan serves the call (the gather route passes a
// lower bound for its temporary index)
constexpr double SMALL_PROBLEM = (double)(1 << 24);
static int search_route(clm_index* x, const QueryStage& qs, int64_t nq, int k, float* osc, int64_t* oix,
                        hipStream_t st, double small_max = SMALL_PROBLEM) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  int r;
  const bool e_full = env_flag("CLM_SEARCH_FULL"), e_exact = env_flag("CLM_SEARCH_EXACT");
  const bool force_bounded = env_flag("CLM_SEARCH_BOUNDED") && N > 0;   // tests: bounded search at any size
  // small batches on a large index: one streaming pass (search_small); $CLM_SEARCH_SMALLQ=1 takes
  // it at any size (tests), 0 never
  const int64_t small_mode = env_int("CLM_SEARCH_SMALLQ", -1);
  const bool small = small_mode != 0 && k <= 1024 && N > 0 && search_small_fits(x, nq, k) &&
                     (small_mode == 1 || (!force_bounded && !e_full && !e_exact && N >= SMALL_MIN_ROWS));
  if (small) {
    r = search_small(x, qs, nq, k, osc, oix, st);
  } else if (k > 1024) {
    // any k: the exact scan over whole rows (topk_rows / the candidate lists stop at 1024)
    r = search_scan_large(x, qs.q32, qs.qn, nq, k, osc, oix, st);
    x->search_stats[ST_EXACT_SCAN] += nq;
  } else if (e_full || N == 0 || dim > MARGIN_MAX_DIM ||
             (!force_bounded && (double)nq * (double)N <= small_max)) {
    r = search_scan(x, true, qs.q16, qs.qinv, qs.q32, qs.qn, nq, k, osc, oix, st);
    x->search_stats[ST_EXACT_SCAN] += nq;
  } else {
    // $CLM_SAMPLE_DIV replaces sample_size's 256: A/B only
    static const int64_t sdiv = std::max<int64_t>(16, env_int("CLM_SAMPLE_DIV", 256));
    const int64_t S = sample_size(k, N, sdiv);
    const bool sampled = !e_exact && k <= 256 && N >= 4 * S && S <= (1 << 18);
    r = search_bounded(x, sampled, S, qs, nq, k, osc, oix, st);
  }
  return r;
}

// every entry point's check of the query dtype (each keeps its own k range and messages)
static int check_query_dtype(int q_dtype) {
  return q_dtype == CLM_F32 || q_dtype == CLM_F16 ? CLM_OK : fail(CLM_E_ARG, "queries must be f32 or f16");
}

// Where a top-k call builds its results (osc / oix): the caller's arrays when both are on the
// device, else two buffers taken from the Layout that sizes QueryStage::extra; bind() once the
// queries are staged, finish() copies out (each array by where it lies) and drains the stream.
struct ResultStage {
  float* out_s; int64_t* out_i; size_t n; bool s_dev, i_dev, dev;
  size_t o_s = 0, o_i = 0;
  float* osc = nullptr; int64_t* oix = nullptr;
  ResultStage(Layout& lay, float* out_scores, int64_t* out_idx, int64_t nq, int k)
      : out_s(out_scores), out_i(out_idx), n((size_t)nq * k), s_dev(is_device_ptr(out_scores)),
        i_dev(is_device_ptr(out_idx)), dev(s_dev && i_dev) {
    if (!dev) { o_s = lay.take(n * 4); o_i = lay.take(n * 8); }
  }
  void bind(const QueryStage& qs) {
    osc = dev ? out_s : (float*)(qs.extra + o_s);
    oix = dev ? out_i : (int64_t*)(qs.extra + o_i);
  }
  int finish(hipStream_t st) const {
    if (!dev) {
      HIPCHK(hipMemcpyAsync(out_s, osc, n * 4, s_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out_i, oix, n * 8, i_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));   // workspaces are reused by the next call
    return CLM_OK;
  }
};

int clm_index_search(clm_index* x, const void* q, int q_dtype, int64_t nq, int k, float* out_scores,
                     int64_t* out_idx, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !out_scores || !out_idx))) return fail(CLM_E_ARG, "bad argument");
  if (int r = check_query_dtype(q_dtype)) return r;
  if (k < 1) return fail(CLM_E_ARG, "k must be >= 1");
  if (k > (1 << 26)) return fail(CLM_E_ARG, "k must be <= 2^26");
  if (nq == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  Layout lay;
  ResultStage res(lay, out_scores, out_idx, nq, k);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (!r) r = stage_queries_f16(x, qs, nq, st);
  if (r) return r;
  res.bind(qs);
  if ((r = search_route(x, qs, nq, k, res.osc, res.oix, st))) return r;
  return res.finish(st);
}

// ---- filtered search (clm_index_search_masked) ----------------------------------------------
// The first k of the ALLOWED rows in the search order. Three routes, the same bits on each (every
// score comes from the exact_cos.hpp routine, every order from (exact score desc, local row asc)):
//  A exact:  search_scan(exact) with every window's disallowed entries set to -inf (mask_fill);
//  B gather: the allowed rows gathered in order into a temporary index of clm_index_import's form,
//            searched by search_route, positions mapped back through the list (monotone: ties keep
//            their order);
//  C pass:   theta from a sample of the ALLOWED rows (a subset of them: its fp16-pass k-th best is
//            never above theirs), one EPI_FILTER_MASK pass, rescore_select; a query whose
//            list overflowed CAND_CAP or ended short of min(k, P) is redone by route A.
// -inf marks a dead entry everywhere (an exact cosine is finite or NaN); map_ids turns it into -1.

// device buffers of one call, released when it returns (the call keeps no state)
struct CallBufs {
  hipStream_t st;
  std::vector<void*> p;
  explicit CallBufs(hipStream_t s) : st(s) {}
  void* take(size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 256)) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    p.push_back(d);
    return d;
  }
  ~CallBufs() {
    if (p.empty()) return;
    (void)hipStreamSynchronize(st);
    for (void* d : p) (void)hipFree(d);
  }
};

// the gather route switches in at P * MASK_GATHER_DIV <= N (the pass route streams all N rows, the
// gather route moves and searches P of them). Measured at 1 M x 512, 4,096 queries, k = 5
// (profiles/masked_search_ab.txt): at P = N / 2 gather 6.2 / 4.3 ms (random / contiguous mask) against
// pass 6.4 / 5.4, at N / 8 2.2 / 1.7 against 5.6 / 4.6; at P = N pass 6.4 against gather 7.7
constexpr int64_t MASK_GATHER_DIV = 2;
// ... and for small batches (nq <= 16, the unmasked search's small-batch bound) at P * 8 <= N: one
// query pays the gather of P rows alone. 1 M rows: pass 0.38 / 0.36 ms at N / 2 and N / 8 against gather
// 0.72 / 0.58; 10 M rows: pass 2.35 / 2.30 against gather 3.88 / 1.64, and 0.46 at 1 %
constexpr int64_t MASK_GATHER_DIV_SMALL = 8;
// the temporary index of the gather route takes the exact scan up to this many dot products only
// (with the unmasked search's 2^24, 4,096 queries x 1,000 gathered rows took the fp64 scan: 10.1 ms,
// profiles/masked_search_ab.txt)
constexpr double MASK_GATHER_SMALL = (double)(1 << 20);

// Route A of the filtered and the keyed search: the exact scan under the filter, dead entries' ids -> -1
static int filtered_exact(clm_index* x, const float* q32, const double* qn, int64_t nq, int k, const RowFilter& allow,
                          float* osc, int64_t* oix, hipStream_t st) {
  int r = search_scan(x, true, nullptr, nullptr, q32, qn, nq, k, osc, oix, st, allow);
  if (r) return r;
  KCHK(map_ids(osc, oix, nq * k, nullptr, 0, st));
  return CLM_OK;
}

// queries `redo` of the batch served again by route A, their rows of osc / oix replaced (a keyed
// filter's ranges are gathered with the queries)
static int filtered_redo(clm_index* x, const QueryStage& qs, int k, const RowFilter& allow,
                         const std::vector<int64_t>& redo, float* osc, int64_t* oix, hipStream_t st) {
  const std::initializer_list<RowArray> plain = {{qs.q32, x->dim * 4}, {qs.qn, 8}},
                                        ranged = {{qs.q32, x->dim * 4}, {qs.qn, 8}, {allow.lo, 4}, {allow.hi, 4}};
  return redo_subset(x, redo, allow.keys ? ranged : plain, {{osc, (int64_t)k * 4}, {oix, (int64_t)k * 8}},
                     allow.keys ? "keyed redo" : "masked redo", st, [&](void* const* in, void* const* out) -> int {
                       RowFilter sub = allow;
                       if (allow.keys) { sub.lo = (const int32_t*)in[2]; sub.hi = (const int32_t*)in[3]; }
                       return filtered_exact(x, (const float*)in[0], (const double*)in[1], (int64_t)redo.size(), k, sub,
                                             (float*)out[0], (int64_t*)out[1], st);
                     });
}

static int masked_gather(clm_index* x, const QueryStage& qs, int64_t nq, int k, const uint32_t* words,
                         const uint32_t* list, int64_t P, float* osc, int64_t* oix, int64_t* n_redo,
                         hipStream_t st) {
  const int dim = (int)x->dim;
  CallBufs bufs(st);
  u16* t16 = (u16*)bufs.take((size_t)P * dim * 2);
  float* tinv = t16 ? (float*)bufs.take((size_t)P * 4) : nullptr;
  float* t32 = tinv && x->rows32 ? (float*)bufs.take((size_t)P * dim * 4) : nullptr;
  if (!t16 || !tinv || (x->rows32 && !t32))
    return fail(CLM_E_OOM, "masked search: the temporary index of " + std::to_string(P) + " rows cannot be allocated");
  KCHK(mask_gather(x->rows, x->rows32, x->inv, dim, list, P, P, t16, t32, tinv, st));
  // the temporary index: the gathered rows, offset 0 (ids = list positions), the parent's block
  // workspaces on loan (the staged queries live in x->ws, which no route touches)
  clm_index tmp;
  tmp.dev = x->dev; tmp.cap = P; tmp.n = P; tmp.dim = x->dim; tmp.offset = 0;
  tmp.rows = t16; tmp.inv = tinv; tmp.rows32 = t32;
  tmp.ws2 = x->ws2; tmp.ws2_bytes = x->ws2_bytes; tmp.ws3 = x->ws3; tmp.ws3_bytes = x->ws3_bytes;
  tmp.ws4 = x->ws4; tmp.ws4_bytes = x->ws4_bytes;
  int r = search_route(&tmp, qs, nq, k, osc, oix, st, MASK_GATHER_SMALL);
  x->ws2 = tmp.ws2; x->ws2_bytes = tmp.ws2_bytes; x->ws3 = tmp.ws3; x->ws3_bytes = tmp.ws3_bytes;
  x->ws4 = tmp.ws4; x->ws4_bytes = tmp.ws4_bytes;
  if (!r && map_ids(osc, oix, nq * k, list, x->offset, st) != hipSuccess) r = fail(CLM_E_HIP, "map_ids launch failed");
  // a list short of min(k, P) entries: a NaN-scoring (zero or non-finite) query, which the MFMA routes
  // of the unmasked search leave without candidates -- route A defines its result
  const int64_t need = std::min<int64_t>(k, P);
  std::vector<int64_t> last(nq);
  hipError_t e = r ? hipSuccess
                   : hipMemcpy2DAsync(last.data(), 8, oix + (need - 1), (size_t)k * 8, 8, (size_t)nq,
                                      hipMemcpyDeviceToHost, st);
  (void)hipStreamSynchronize(st);
  // everything the routes allocated lazily in the temporary index: not the gathered rows (bufs owns
  // them), not the workspaces on loan
  index_free_buffers(&tmp, {tmp.rows, tmp.inv, tmp.rows32, tmp.ws2, tmp.ws3, tmp.ws4});
  if (r) return r;
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("masked search: ") + hipGetErrorString(e));
  std::vector<int64_t> redo;
  for (int64_t i = 0; i < nq && k <= 1024; ++i)
    if (last[i] < 0) redo.push_back(i);
  *n_redo = (int64_t)redo.size();
  return filtered_redo(x, qs, k, RowFilter{words}, redo, osc, oix, st);
}

// The sampled thresholds and the candidate pass of the masked and the keyed search. The call's
// sample -- S rows with inverse norms and, for a keyed filter, keys, which sample(s16, sinv, skeys)
// fills -- is scored per query block, a keyed filter's closed entries are struck out, and th[q] =
// its k-th best - RESCORE_MARGIN (fewer sample rows than k: no threshold, -inf). Then candidate_pass
// under the filter; hcnt: every query's count, for the caller's rule of what is redone. The
// sample-score rows are padded as search_bounded's.
template <class Sample>
static int filtered_pass(clm_index* x, const QueryStage& qs, int64_t nq, int k, const RowFilter& allow, int64_t S,
                         float* osc, int64_t* oix, std::vector<int>& hcnt, hipStream_t st, Sample sample) {
  const int dim = (int)x->dim;
  int r;
  const int64_t ldS = round_up(S, 4) + 64;
  const int64_t nqb = band_query_block(nq, ldS * 4, 256);
  Layout lay;
  const size_t o_s16 = lay.take((size_t)S * dim * 2), o_si = lay.take((size_t)S * 4),
               o_sk = allow.keys ? lay.take((size_t)S * 4) : 0, o_sc = lay.take((size_t)nqb * ldS * 4);
  PassBufs b;
  b.take(lay, nq, nqb, k);
  if ((r = grow(&x->ws2, &x->ws2_bytes, lay.total()))) return r;
  uint8_t* w = (uint8_t*)x->ws2;
  b.bind(w);
  u16* s16 = (u16*)(w + o_s16);
  float* sinv = (float*)(w + o_si);
  int32_t* skeys = allow.keys ? (int32_t*)(w + o_sk) : nullptr;
  float* sc = (float*)(w + o_sc);
  KCHK(sample(s16, sinv, skeys));
  if (S < k) KCHK(fill_f32(b.th, nq, -INFINITY, st));
  for (int64_t q0 = 0; q0 < nq && S >= k; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    KCHK(sample_scores(qs, q0, nb, dim, s16, sinv, S, sc, ldS, 0, st));
    // fewer than k open sample rows: the k-th value is a struck-out -inf, and so is theta
    if (skeys) KCHK(key_fill(sc, ldS, nb, S, 0, skeys, allow.lo + q0, allow.hi + q0, st));
    if ((r = row_thresholds(sc, ldS, nb, S, k, kth_one_pass(k), b, b.th + q0, st))) return r;
  }
  return candidate_pass(x, qs, nq, nqb, k, allow, b, osc, oix, hcnt, st, heuristic_cfg);
}

static int masked_pass(clm_index* x, const QueryStage& qs, int64_t nq, int k, const uint32_t* words,
                       const uint32_t* list, int64_t P, int64_t S, float* osc, int64_t* oix, int64_t* n_redo,
                       hipStream_t st) {
  const RowFilter allow{words};
  std::vector<int> hcnt;
  // the sample: S rows at positions floor(i * P / S) of the allowed list, in buffers of this call
  int r = filtered_pass(x, qs, nq, k, allow, S, osc, oix, hcnt, st, [&](u16* s16, float* sinv, int32_t*) {
    return mask_gather(x->rows, nullptr, x->inv, (int)x->dim, list, P, S, s16, nullptr, sinv, st);
  });
  if (r) return r;
  // an overflowed list, or one short of min(k, P) (NaN scores pass no threshold): route A decides
  std::vector<int64_t> redo;
  const int64_t need = std::min<int64_t>(k, P);
  for (int64_t i = 0; i < nq; ++i)
    if (hcnt[i] > CAND_CAP || hcnt[i] < need) redo.push_back(i);
  *n_redo = (int64_t)redo.size();
  return filtered_redo(x, qs, k, allow, redo, osc, oix, st);
}

// The mask steps every filtered search starts with (clm_mask_rows runs them alone): the caller's words
// prepared -- tail bits cleared, one count per block --, the blocks' offsets, and the total P brought
// to the host (drains the stream).
static int mask_plan(const uint32_t* src, int64_t N, uint32_t* words, uint32_t* bcnt, int64_t* boff, int64_t* P,
                     hipStream_t st) {
  const int64_t nblk = mask_blocks(N);
  KCHK(mask_prepare(src, N, words, bcnt, st));
  KCHK(mask_scan(bcnt, nblk, boff, st));
  HIPCHK(hipMemcpyAsync(P, boff + nblk, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return CLM_OK;
}

static int search_masked(clm_index* x, const QueryStage& qs, int64_t nq, int k, const uint32_t* words,
                         const int64_t* boff, int64_t P, int flags, float* osc, int64_t* oix, hipStream_t st) {
  const int64_t N = x->n, dim = x->dim;
  int r;
  if (P == 0) {   // nothing is allowed: (-inf, -1) lists (counted with the exact route)
    x->search_stats[ST_MASK_EXACT] += nq;
    KCHK(fill_f32(osc, nq * k, -INFINITY, st));
    HIPCHK(hipMemsetAsync(oix, 0xFF, (size_t)nq * k * 8, st));
    return CLM_OK;
  }
  const bool exact_ok = k <= 1024;   // search_scan's lists
  // a zero or non-finite inverse norm: that row's scores are NaN, which the fp16 pass cannot list and
  // which the unmasked routes (the gather route's search) do not place above every number -- the
  // exact route does (mask_fill), so it serves such an index whenever its lists hold k
  bool fin = false;
  if ((r = inv_norms_finite(x, st, &fin))) return r;
  const bool pass_ok = filter_pass_ok(x, fin, k);
  const int64_t Sd = sample_size(k, P);
  enum { R_EXACT, R_GATHER, R_PASS } route;
  if (((flags & CLM_MASK_EXACT) || !fin) && exact_ok) route = R_EXACT;
  else if ((flags & CLM_MASK_PASS) && pass_ok) route = R_PASS;
  else if (flags & CLM_MASK_GATHER) route = R_GATHER;
  else if (exact_ok && (env_flag("CLM_SEARCH_FULL") || dim > MARGIN_MAX_DIM)) route = R_EXACT;
  else if (pass_ok && P >= 4 * Sd && Sd <= (1 << 18) && P * (nq <= 16 ? MASK_GATHER_DIV_SMALL : MASK_GATHER_DIV) > N)
    route = R_PASS;
  else route = R_GATHER;
  if (route == R_EXACT) {
    x->search_stats[ST_MASK_EXACT] += nq;
    return filtered_exact(x, qs.q32, qs.qn, nq, k, RowFilter{words}, osc, oix, st);
  }
  CallBufs bufs(st);
  uint32_t* list = (uint32_t*)bufs.take((size_t)P * 4);
  if (!list) return fail(CLM_E_OOM, "masked search: the list of " + std::to_string(P) + " allowed rows cannot be allocated");
  KCHK(mask_compact(words, N, boff, list, st));
  int64_t n_redo = 0;
  if (route == R_GATHER) {
    r = masked_gather(x, qs, nq, k, words, list, P, osc, oix, &n_redo, st);
    x->search_stats[ST_MASK_GATHER] += nq - n_redo;
    x->search_stats[ST_MASK_EXACT] += n_redo;
    return r;
  }
  r = masked_pass(x, qs, nq, k, words, list, P, std::min(std::min<int64_t>(Sd, 1 << 18), P), osc, oix, &n_redo, st);
  x->search_stats[ST_MASK_PASS] += nq - n_redo;
  x->search_stats[ST_MASK_EXACT] += n_redo;
  return r;
}

int clm_index_search_masked(clm_index* x, const void* q, int q_dtype, int64_t nq, int k, const uint32_t* allow,
                            int flags, float* out_scores, int64_t* out_idx, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !allow || !out_scores || !out_idx))) return fail(CLM_E_ARG, "bad argument");
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (k < 1) return fail(CLM_E_ARG, "k must be >= 1");
  if (k > (1 << 26)) return fail(CLM_E_ARG, "k must be <= 2^26");
  if (x->n == 0) return fail(CLM_E_ARG, "masked search: the index is empty");
  if (nq == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = x->n, nw = mask_words(N), nblk = mask_blocks(N);
  const bool a_dev = is_device_ptr(allow);
  Layout lay;   // the results' staging when they go to the host, then the mask's buffers
  ResultStage res(lay, out_scores, out_idx, nq, k);
  const size_t o_src = a_dev ? 0 : lay.take((size_t)nw * 4);
  const size_t o_words = lay.take((size_t)nw * 4), o_bcnt = lay.take((size_t)nblk * 4),
               o_boff = lay.take((size_t)(nblk + 1) * 8);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (!r) r = stage_queries_f16(x, qs, nq, st);
  if (r) return r;
  res.bind(qs);
  const uint32_t* src = allow;
  if (!a_dev) {
    HIPCHK(copy_in(qs.extra + o_src, allow, (size_t)nw * 4, st));
    src = (const uint32_t*)(qs.extra + o_src);
  }
  uint32_t* words = (uint32_t*)(qs.extra + o_words);
  uint32_t* bcnt = (uint32_t*)(qs.extra + o_bcnt);
  int64_t* boff = (int64_t*)(qs.extra + o_boff);
  int64_t P = 0;
  if ((r = mask_plan(src, N, words, bcnt, boff, &P, st))) return r;
  if ((r = search_masked(x, qs, nq, k, words, boff, P, flags, res.osc, res.oix, st))) return r;
  return res.finish(st);
}

int clm_mask_rows(int hip_device, const uint32_t* allow, int64_t N, uint32_t* words, uint32_t* bcnt, int64_t* boff,
                  uint32_t* list, int64_t* P_out, void* stream) {
  if (N < 1 || N > 0xFFFFFFFFll) return fail(CLM_E_ARG, "mask_rows: 1 <= N <= 2^32 - 1");
  if (!is_device_ptr(allow) || !is_device_ptr(words) || !is_device_ptr(bcnt) || !is_device_ptr(boff) ||
      (list && !is_device_ptr(list)))
    return fail(CLM_E_ARG, "mask_rows: device pointers");
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  int64_t P = 0;
  if (int r = mask_plan(allow, N, words, bcnt, boff, &P, st)) return r;
  if (list && P > 0) {
    KCHK(mask_compact(words, N, boff, list, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (P_out) *P_out = P;
  return CLM_OK;
}

// ---- keyed search (clm_index_search_keyed) --------------------------------------------------
// One int32 key per index row (the caller's, per call) and one inclusive key range per query: row j
// is open to query i iff lo[i] <= keys[j] <= hi[i]. Row i of the result is row 0 of the masked
// search of query i alone under the mask of its open rows. Two routes:
//  A exact:  search_scan(exact) with every window's closed entries set to -inf (key_fill);
//  C pass:   theta[i] from a strided sample of the index whose closed entries are struck out per
//            query (key_fill on the sample's score matrix): the k-th best of sample rows that are in
//            the index and open to the query is never above the k-th best of all its open rows, and a
//            query with fewer than k open sample rows gets -inf and lists every open row. Then one
//            EPI_FILTER_KEYS pass and rescore_select; a query whose list overflowed CAND_CAP or ended
//            short of what its range holds is redone by route A. Nothing rests on the sample but speed.

// hn_in: the caller's counts on the host, or null; hlo / hhi: the ranges on the host
static int keyed_pass(clm_index* x, const QueryStage& qs, int64_t nq, int k, const RowFilter& allow, const int32_t* hlo,
                      const int32_t* hhi, const int64_t* hn_in, int64_t S, float* osc, int64_t* oix, int64_t* n_redo,
                      hipStream_t st) {
  std::vector<int> hcnt;
  // the sample: S rows at positions floor(i * N / S) with their keys, in buffers of this call
  int r = filtered_pass(x, qs, nq, k, allow, S, osc, oix, hcnt, st, [&](u16* s16, float* sinv, int32_t* skeys) {
    return key_sample(x->rows, x->inv, allow.keys, (int)x->dim, x->n, S, s16, sinv, skeys, st);
  });
  if (r) return r;
  // an overflowed list, or one short of what the range holds (NaN scores pass no threshold; without
  // the caller's counts every list short of k): route A decides
  std::vector<int64_t> redo;
  for (int64_t i = 0; i < nq; ++i) {
    const int64_t open = hlo[i] > hhi[i] ? 0 : hn_in ? hn_in[i] : x->n;
    if (hn_in && hcnt[i] > open)
      return fail(CLM_E_ARG, "keyed search: query " + std::to_string(i) + " lists " + std::to_string(hcnt[i]) +
                                 " rows of its range, n_in says it holds " + std::to_string(open));
    if (hcnt[i] > CAND_CAP || hcnt[i] < std::min<int64_t>(k, open)) redo.push_back(i);
  }
  *n_redo = (int64_t)redo.size();
  return filtered_redo(x, qs, k, allow, redo, osc, oix, st);
}

int clm_index_search_keyed(clm_index* x, const void* q, int q_dtype, int64_t nq, int k, const int32_t* keys,
                           const int32_t* lo, const int32_t* hi, const int64_t* n_in, int flags, float* out_scores,
                           int64_t* out_idx, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !keys || !lo || !hi || !out_scores || !out_idx)))
    return fail(CLM_E_ARG, "bad argument");
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (k < 1 || k > 1024) return fail(CLM_E_ARG, "keyed search: 1 <= k <= 1024");
  if (flags & ~(CLM_MASK_EXACT | CLM_MASK_PASS)) return fail(CLM_E_ARG, "keyed search: flags are 0, CLM_MASK_EXACT or CLM_MASK_PASS");
  if (x->n == 0) return fail(CLM_E_ARG, "keyed search: the index is empty");
  if (nq == 0) return CLM_OK;
  DeviceGuard g(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = x->n;
  Layout lay;   // the results' staging when they go to the host, then the keys and the ranges
  ResultStage res(lay, out_scores, out_idx, nq, k);
  const size_t o_keys = lay.take((size_t)N * 4), o_lo = lay.take((size_t)nq * 4), o_hi = lay.take((size_t)nq * 4);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (r) return r;
  res.bind(qs);
  int32_t* dkeys = (int32_t*)(qs.extra + o_keys);
  int32_t* dlo = (int32_t*)(qs.extra + o_lo);
  int32_t* dhi = (int32_t*)(qs.extra + o_hi);
  HIPCHK(copy_in(dkeys, keys, (size_t)N * 4, st));
  HIPCHK(copy_in(dlo, lo, (size_t)nq * 4, st));
  HIPCHK(copy_in(dhi, hi, (size_t)nq * 4, st));
  const RowFilter allow{nullptr, dkeys, dlo, dhi};
  // a zero or non-finite inverse norm: that row's scores are NaN, which only the exact route places
  // (see search_masked). Drains the stream: the copies above are done
  bool fin = false;
  if ((r = inv_norms_finite(x, st, &fin))) return r;
  const int64_t Sd = sample_size(k, N);
  bool pass = filter_pass_ok(x, fin, k) && !(flags & CLM_MASK_EXACT);
  if (pass && !(flags & CLM_MASK_PASS)) pass = !env_flag("CLM_SEARCH_FULL") && N >= 4 * Sd;
  if (!pass) {
    x->search_stats[ST_KEY_EXACT] += nq;
    r = filtered_exact(x, qs.q32, qs.qn, nq, k, allow, res.osc, res.oix, st);
  } else {
    // the ranges and the caller's counts on the host: what each list must hold
    std::vector<int32_t> hlo(nq), hhi(nq);
    std::vector<int64_t> hn;
    HIPCHK(hipMemcpyAsync(hlo.data(), dlo, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hhi.data(), dhi, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    if (n_in) {
      hn.resize(nq);
      if (is_device_ptr(n_in)) HIPCHK(hipMemcpyAsync(hn.data(), n_in, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
      else std::memcpy(hn.data(), n_in, (size_t)nq * 8);
    }
    HIPCHK(hipStreamSynchronize(st));
    if ((r = stage_queries_f16(x, qs, nq, st))) return r;
    int64_t n_redo = 0;
    r = keyed_pass(x, qs, nq, k, allow, hlo.data(), hhi.data(), n_in ? hn.data() : nullptr,
                   std::min(std::min<int64_t>(Sd, 1 << 18), N), res.osc, res.oix, &n_redo, st);
    if (!r) {
      x->search_stats[ST_KEY_PASS] += nq - n_redo;
      x->search_stats[ST_KEY_EXACT] += n_redo;
    }
  }
  if (r) return r;
  return res.finish(st);
}

// Whether a whole rank / log-sum-exp / threshold call takes its exact route: asked for (force_exact:
// the call's flag or $CLM_SEARCH_FULL=1), a zero or non-finite inverse norm in the index (!inv_ok),
// rows the fp16-pass margins do not cover or the pass cannot number, or at most the 2^24 dot products
// below which clm_index_search takes its exact scan too -- unless the fast route is asked for
// (force_fast: the call's flag or, tests, $CLM_SEARCH_BOUNDED=1)
static bool whole_call_exact(const clm_index* x, int64_t nq, bool inv_ok, bool force_exact, bool force_fast) {
  return force_exact || !inv_ok || x->dim > MARGIN_MAX_DIM || x->n > 0x7FFFFFFF ||
         (!force_fast && (double)nq * (double)x->n <= SMALL_PROBLEM);
}

// ---- exact retrieval ranks (clm_index_rank / clm_index_count_above) ------------------------
// above(q) = #{rows ahead of the target (t, g) in the search order}. One EPI_RANK pass decides
// every row whose fp16-pass score s is further than RANK_MARGIN from t: RESCORE_MARGIN's comment
// bounds |s - exact cosine| by 1.95e-3 + 4.9e-4 = 2.44e-3 for dim <= MARGIN_MAX_DIM, so
// s > t + 2.5e-3 puts the exact score above t by more than 6e-5 and s < t - 2.5e-3 below it by
// as much; t's own fp32 rounding and that of t +- margin (6e-8 each) are inside the 6e-5. The
// comparison is one-sided but only one score of it (s) carries the fp16 error -- t is exact -- so
// half of RESCORE_MARGIN, which covers two such scores, is enough.
constexpr float RANK_MARGIN = RESCORE_MARGIN / 2;
// band slots per query: the capacity bits of a caller's band_cap, else max(2048, N / 8); N at most
static int64_t band_capacity(int band_cap, int64_t N) {
  const int64_t user = band_cap > 0 ? band_cap & CLM_RANK_CAP_MASK : 0;
  return std::min<int64_t>(N, user > 0 ? user : std::max<int64_t>(2048, N / 8));
}

// The exact route: exact scores in row windows [nqb, ch] (windowed as search_scan(exact) does:
// no buffer grows with nq x N) and count_rank per window. q32 / qn / t / g / above: device
// arrays of the nq queries.
static int rank_exact(clm_index* x, const float* q32, const double* qn, const float* t, const int64_t* g,
                      int64_t nq, int64_t* above, hipStream_t st) {
  const int dim = (int)x->dim;
  ExactWindows w;
  int r = exact_windows(x, nq, 4, 0, &w);
  if (r) return r;
  float* sc = (float*)w.sc;
  HIPCHK(hipMemsetAsync(above, 0, (size_t)nq * 8, st));
  return walk_exact_windows(x, w, nq, [&](int64_t q0, int64_t nb, int64_t r0, int64_t rn, ExactRows er) -> int {
    KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, sc, w.ch, st));
    KCHK(count_rank(sc, w.ch, nb, rn, x->offset + r0, t + q0, g + q0, above + q0, st));
    return CLM_OK;
  });
}

// The band route, per block of queries (blocks as search_bounded cuts them): the EPI_RANK GEMM
// streams the index once (above32 = the rows certainly ahead, the band list = the undecided ones,
// capacity `cap` per query), rank_rescore settles the band exactly. The band buffer (8 B per
// slot) is what band_query_block bounds: the query block shrinks, the capacity does not. Queries
// whose band overflowed are appended to `redo`.
static int rank_band(clm_index* x, const unsigned* keys, const u16* q16, const float* qinv, const float* q32,
                     const double* qn, const float* t, const int64_t* g, int64_t nq, int64_t cap, int64_t* above,
                     std::vector<int64_t>& redo, hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t nqb = band_query_block(nq, cap * 8, 1);
  Layout lay;
  const size_t o_up = lay.take((size_t)nq * 4), o_cnt = lay.take((size_t)nq * 4), o_plan = lay.take((size_t)(nqb + 1) * 4),
               o_band = lay.take((size_t)nqb * cap * 8);
  int r = grow(&x->ws2, &x->ws2_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws2;
  unsigned* above32 = (unsigned*)(w + o_up);
  int* cnt = (int*)(w + o_cnt);
  int64_t* band = (int64_t*)(w + o_band);
  const ExactRows xr = exact_rows(x);
  HIPCHK(hipMemsetAsync(above32, 0, (size_t)nq * 4, st));
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)nq * 4, st));
  HIPCHK(hipMemsetAsync(above, 0, (size_t)nq * 8, st));   // rank_rescore adds into it
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    GemmArgs gr = index_pass(x, q16 + q0 * dim, qinv + q0, nb, t + q0, cnt + q0, band, cap);
    gr.rank_margin = RANK_MARGIN;
    gr.above = above32 + q0;
    gr.cbound = keys;
    KCHK(gemm_cfg(false, EPI_RANK, -1, gr, st));
    KCHK(rank_rescore(band, cnt + q0, cap, above32 + q0, q32 + q0 * dim, qn + q0, dim, xr.p, xr.f16, x->offset,
                      t + q0, g + q0, nb, (int*)(w + o_plan), above + q0, st));
  }
  std::vector<int> hcnt(nq);
  HIPCHK(hipMemcpyAsync(hcnt.data(), cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < nq; ++i) {
    if (hcnt[i] > cap) redo.push_back(i);
    else x->search_stats[ST_RANK_BAND_ROWS] += hcnt[i];
  }
  return CLM_OK;
}

// Router of both entry points. tgt: the targets (rank: global row ids, validated; count_above: the
// tie-break ids g, any value); t_in: the target scores (count_above) or null (rank: computed here).
// A query takes the exact route when its band list overflowed or its t is NaN / infinite; the whole
// call does when the index holds a non-finite inverse norm (a zero row scores NaN in the fp16 pass
// as in the exact one, but only the latter is compared as the order defines), dim > MARGIN_MAX_DIM,
// CLM_RANK_EXACT / $CLM_SEARCH_FULL=1 ask for it, or nq x N is at most the 2^24 dot products below
// which clm_index_search takes its exact scan too (CLM_RANK_BAND / $CLM_SEARCH_BOUNDED=1: the band
// route at any size, tests). The counts do not depend on the route: both compare exact_cos scores.
static int rank_run(clm_index* x, const void* q, int q_dtype, int64_t nq, const float* t_in, const int64_t* tgt,
                    int64_t* out_i, float* out_s, int band_cap, void* stream) {
  const bool is_rank = t_in == nullptr;
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (nq == 0) return CLM_OK;
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  std::vector<int64_t> htgt(nq);
  if (is_device_ptr(tgt)) {
    HIPCHK(hipMemcpyAsync(htgt.data(), tgt, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    std::memcpy(htgt.data(), tgt, (size_t)nq * 8);
  }
  if (is_rank)
    for (int64_t i = 0; i < nq; ++i)
      if (htgt[i] < x->offset || htgt[i] - x->offset >= N)
        return fail(CLM_E_ARG, "target " + std::to_string(htgt[i]) + " of query " + std::to_string(i) +
                                   " is outside the index [" + std::to_string(x->offset) + ", " +
                                   std::to_string(x->offset + N) + ")");
  Layout lay;
  const size_t o_t = lay.take((size_t)nq * 4), o_g = lay.take((size_t)nq * 8), o_ab = lay.take((size_t)nq * 8),
               o_rk = lay.take((size_t)nq * 8);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (r) return r;
  const float* q32 = qs.q32;
  const double* qn = qs.qn;
  float* t = (float*)(qs.extra + o_t);
  int64_t* g = (int64_t*)(qs.extra + o_g);
  int64_t* above = (int64_t*)(qs.extra + o_ab);
  int64_t* rank = (int64_t*)(qs.extra + o_rk);
  const ExactRows xr = exact_rows(x);
  HIPCHK(hipMemcpyAsync(g, htgt.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  if (is_rank) KCHK(target_scores(q32, qn, nq, dim, xr.p, xr.f16, x->offset, g, t, st));
  else HIPCHK(copy_in(t, t_in, (size_t)nq * 4, st));
  std::vector<float> ht(nq);
  HIPCHK(hipMemcpyAsync(ht.data(), t, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  const unsigned* keys = nullptr;
  bool inv_ok = false;
  if ((r = inv_norms_finite(x, st, &inv_ok, &keys))) return r;
  const int flags = band_cap > 0 ? band_cap & (CLM_RANK_EXACT | CLM_RANK_BAND) : 0;
  const bool all_exact = whole_call_exact(x, nq, inv_ok, (flags & CLM_RANK_EXACT) || env_flag("CLM_SEARCH_FULL"),
                                         (flags & CLM_RANK_BAND) || env_flag("CLM_SEARCH_BOUNDED"));
  if (all_exact) {
    if ((r = rank_exact(x, q32, qn, t, g, nq, above, st))) return r;
    x->search_stats[ST_RANK_EXACT] += nq;
  } else {
    if ((r = stage_queries_f16(x, qs, nq, st))) return r;
    const int64_t cap = band_capacity(band_cap, N);
    std::vector<int64_t> redo;
    if ((r = rank_band(x, keys, qs.q16, qs.qinv, q32, qn, t, g, nq, cap, above, redo, st))) return r;
    x->search_stats[ST_RANK_OVERFLOW] += (int64_t)redo.size();
    std::vector<char> listed(nq, 0);
    for (int64_t i : redo) listed[i] = 1;
    for (int64_t i = 0; i < nq; ++i)
      if (!listed[i] && !(std::fabs(ht[i]) <= 3.4028235e38f)) redo.push_back(i);   // NaN or infinite t
    x->search_stats[ST_RANK_BAND] += nq - (int64_t)redo.size();
    x->search_stats[ST_RANK_EXACT] += (int64_t)redo.size();
    // their queries, norms and targets gathered, one exact pass, counts scattered back
    r = redo_subset(x, redo, {{q32, (int64_t)dim * 4}, {qn, 8}, {t, 4}, {g, 8}}, {{above, 8}}, "rank", st,
                    [&](void* const* in, void* const* out) -> int {
                      return rank_exact(x, (const float*)in[0], (const double*)in[1], (const float*)in[2],
                                        (const int64_t*)in[3], (int64_t)redo.size(), (int64_t*)out[0], st);
                    });
    if (r) return r;
  }
  const int64_t* res = above;
  if (is_rank) {
    KCHK(rank_from_above(above, nq, rank, st));
    res = rank;
  }
  HIPCHK(copy_out(out_i, res, (size_t)nq * 8, st));
  if (out_s) HIPCHK(copy_out(out_s, t, (size_t)nq * 4, st));
  HIPCHK(hipStreamSynchronize(st));   // workspaces are reused by the next call
  return CLM_OK;
}

int clm_index_count_above(clm_index* x, const void* q, int q_dtype, int64_t nq, const float* t_score,
                          const int64_t* t_index, int64_t* out_above, int band_cap, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !t_score || !t_index || !out_above))) return fail(CLM_E_ARG, "bad argument");
  return rank_run(x, q, q_dtype, nq, t_score, t_index, out_above, nullptr, band_cap, stream);
}

int clm_index_rank(clm_index* x, const void* q, int q_dtype, int64_t nq, const int64_t* target, int64_t* out_rank,
                   float* out_score, int band_cap, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !target || !out_rank))) return fail(CLM_E_ARG, "bad argument");
  return rank_run(x, q, q_dtype, nq, nullptr, target, out_rank, out_score, band_cap, stream);
}

// ---- streaming log-sum-exp (clm_index_lse) --------------------------------------------------
// lse(q) = log sum_j exp(scale * s_j) over the exact scores, in fp64. The fast route's certified
// bound rests on E >= |fp16-pass score - s_j|: RESCORE_MARGIN's comment gives 1.95e-3 + 4.9e-4 for
// dim <= MARGIN_MAX_DIM against the exact cosine; 1e-6 more covers the fp32 roundings of s_j itself
// and of the fp16-pass score's two scale products (6e-8 each).
constexpr double LSE_E = 1.95e-3 + 4.9e-4 + 1e-6;

// The exact route: exact scores in rank_exact's row windows, folded into a running (maximum, sum)
// per query. A query's result depends on the index alone, not on nq. q32 / qn / lse / err: device
// arrays of the nq queries (err may be null). f64: the reference route of clm_index_lse64, the same
// windows of unrounded fp64 cosines; pair[q] (device, or null) takes the cosine of row target[q].
static int lse_exact(clm_index* x, const float* q32, const double* qn, int64_t nq, double scale, double* lse,
                     float* err, hipStream_t st, bool f64 = false, const int64_t* target = nullptr,
                     double* pair = nullptr) {
  const int dim = (int)x->dim;
  ExactWindows w;
  int r = exact_windows(x, nq, f64 ? 8 : 4, (size_t)nq * sizeof(double2), &w);
  if (r) return r;
  double2* state = (double2*)w.header;
  void* sc = w.sc;
  const int64_t ch = w.ch;
  KCHK(lse_fold_init(state, nq, st));
  r = walk_exact_windows(x, w, nq, [&](int64_t q0, int64_t nb, int64_t r0, int64_t rn, ExactRows er) -> int {
    if (f64) {
      KCHK(lse_scores64(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, (double*)sc, ch, st));
      KCHK(lse_fold64((const double*)sc, ch, nb, rn, scale, state + q0, target ? target + q0 : nullptr, x->offset,
                      r0, pair ? pair + q0 : nullptr, st));
    } else {
      KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, (float*)sc, ch, st));
      KCHK(lse_fold((const float*)sc, ch, nb, rn, scale, state + q0, st));
    }
    return CLM_OK;
  });
  if (r) return r;
  KCHK(lse_fold_finish(state, nq, scale, lse, err, st));
  return CLM_OK;
}

// The fast route, per block of queries (rank_band's blocks): the EPI_LSE GEMM streams the index
// once (band list = the rows at or above theta - RANK_MARGIN, slab = the tail partials), then
// lse_band_scores re-scores the band and lse_finish combines. Band (8 + 4 B per slot) and slab
// (4 B per slot) are what band_query_block bounds: the query block shrinks. redo[q] = 1 (device)
// marks the queries left to the exact route; `overflowed` counts those whose band exceeded `cap`.
static int lse_band(clm_index* x, const u16* q16, const float* qinv, const float* q32, const double* qn,
                    const float* theta, int64_t nq, int64_t cap, double scale, double* lse, float* err, int* redo,
                    std::vector<int64_t>& redo_list, int64_t& overflowed, hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  const int64_t slots = lse_slots(N);
  const int64_t nqb = band_query_block(nq, cap * 12 + slots * 4, 1);
  Layout lay;
  const size_t o_cnt = lay.take((size_t)nq * 4), o_plan = lay.take((size_t)(nqb + 1) * 4),
               o_band = lay.take((size_t)nqb * cap * 8), o_bs = lay.take((size_t)nqb * cap * 4),
               o_slab = lay.take((size_t)nqb * slots * 4);
  int r = grow(&x->ws2, &x->ws2_bytes, lay.total());
  if (r) return r;
  uint8_t* w = (uint8_t*)x->ws2;
  int* cnt = (int*)(w + o_cnt);
  int64_t* band = (int64_t*)(w + o_band);
  float* band_s = (float*)(w + o_bs);
  float* slab = (float*)(w + o_slab);
  const ExactRows xr = exact_rows(x);
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)nq * 4, st));
  HIPCHK(hipMemsetAsync(redo, 0, (size_t)nq * 4, st));
  for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
    const int64_t nb = std::min(nqb, nq - q0);
    HIPCHK(hipMemsetAsync(slab, 0, (size_t)nb * slots * 4, st));   // the slots the chosen tiles do not use
    GemmArgs gr = index_pass(x, q16 + q0 * dim, qinv + q0, nb, theta + q0, cnt + q0, band, cap);
    gr.rank_margin = RANK_MARGIN;
    gr.lse_part = slab; gr.lse_ld = slots; gr.lse_c = (float)(scale * 1.4426950408889634);
    KCHK(gemm_cfg(false, EPI_LSE, -1, gr, st));
    KCHK(lse_band_scores(band, cnt + q0, cap, q32 + q0 * dim, qn + q0, dim, xr.p, xr.f16, x->offset, nb,
                         (int*)(w + o_plan), band_s, st));
    KCHK(lse_finish(band_s, cnt + q0, cap, slab, slots, theta + q0, scale, LSE_E, N, nb, lse + q0, err + q0,
                    redo + q0, st));
  }
  std::vector<int> hcnt(nq), hredo(nq);
  HIPCHK(hipMemcpyAsync(hcnt.data(), cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hredo.data(), redo, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < nq; ++i) {
    if (hredo[i]) redo_list.push_back(i);
    if (hcnt[i] > cap) ++overflowed;
  }
  return CLM_OK;
}

int clm_index_lse(clm_index* x, const void* q, int q_dtype, int64_t nq, double scale, const float* head_floor,
                  double* out_lse, float* out_err, int band_cap, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !out_lse))) return fail(CLM_E_ARG, "bad argument");
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (!(scale > 0.0 && scale <= 1.7976931348623157e308)) return fail(CLM_E_ARG, "scale must be finite and positive");
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (nq == 0) return CLM_OK;
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  Layout lay;
  const size_t o_th = lay.take((size_t)nq * 4), o_lse = lay.take((size_t)nq * 8), o_err = lay.take((size_t)nq * 4),
               o_redo = lay.take((size_t)nq * 4);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (r) return r;
  const float* q32 = qs.q32;
  const double* qn = qs.qn;
  float* theta = (float*)(qs.extra + o_th);
  double* lse = (double*)(qs.extra + o_lse);
  float* err = (float*)(qs.extra + o_err);
  int* redo = (int*)(qs.extra + o_redo);
  // as rank_run: every inverse norm finite and positive, or the whole call is exact
  bool inv_ok = false;
  if ((r = inv_norms_finite(x, st, &inv_ok))) return r;
  const int flags = band_cap > 0 ? band_cap & (CLM_LSE_EXACT | CLM_LSE_FAST) : 0;
  const bool all_exact = !head_floor || whole_call_exact(x, nq, inv_ok, (flags & CLM_LSE_EXACT) || env_flag("CLM_SEARCH_FULL"),
                                                        (flags & CLM_LSE_FAST) != 0);
  if (all_exact) {
    if ((r = lse_exact(x, q32, qn, nq, scale, lse, err, st))) return r;
    x->search_stats[ST_LSE_EXACT] += nq;
  } else {
    HIPCHK(copy_in(theta, head_floor, (size_t)nq * 4, st));
    if ((r = stage_queries_f16(x, qs, nq, st))) return r;
    const int64_t cap = band_capacity(band_cap, N);
    std::vector<int64_t> todo;
    int64_t overflowed = 0;
    if ((r = lse_band(x, qs.q16, qs.qinv, q32, qn, theta, nq, cap, scale, lse, err, redo, todo, overflowed, st))) return r;
    x->search_stats[ST_LSE_OVERFLOW] += overflowed;
    x->search_stats[ST_LSE_FAST] += nq - (int64_t)todo.size();
    x->search_stats[ST_LSE_EXACT] += (int64_t)todo.size();
    // their queries and norms gathered, one exact pass, results scattered back
    r = redo_subset(x, todo, {{q32, (int64_t)dim * 4}, {qn, 8}}, {{lse, 8}, {err, 4}}, "lse", st,
                    [&](void* const* in, void* const* out) -> int {
                      return lse_exact(x, (const float*)in[0], (const double*)in[1], (int64_t)todo.size(), scale,
                                       (double*)out[0], (float*)out[1], st);
                    });
    if (r) return r;
  }
  HIPCHK(copy_out(out_lse, lse, (size_t)nq * 8, st));
  if (out_err) HIPCHK(copy_out(out_err, err, (size_t)nq * 4, st));
  HIPCHK(hipStreamSynchronize(st));   // workspaces are reused by the next call
  return CLM_OK;
}

// The reference route: lse_exact on the unrounded fp64 cosines. Nothing here is rounded to fp32, so
// a loss built from out_lse and out_pair is the fp64 loss of the same rows to fp64 rounding.
int clm_index_lse64(clm_index* x, const void* q, int q_dtype, int64_t nq, double scale, const int64_t* target,
                    double* out_lse, double* out_pair, void* stream) {
  if (!x || nq < 0 || (nq > 0 && (!q || !out_lse || (out_pair && !target)))) return fail(CLM_E_ARG, "bad argument");
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (!(scale > 0.0 && scale <= 1.7976931348623157e308)) return fail(CLM_E_ARG, "scale must be finite and positive");
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (nq == 0) return CLM_OK;
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  Layout lay;
  const size_t o_lse = lay.take((size_t)nq * 8), o_pair = lay.take((size_t)nq * 8), o_tg = lay.take((size_t)nq * 8);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (r) return r;
  double* lse = (double*)(qs.extra + o_lse);
  double* pair = out_pair ? (double*)(qs.extra + o_pair) : nullptr;
  int64_t* tg = pair ? (int64_t*)(qs.extra + o_tg) : nullptr;
  if (pair) {
    HIPCHK(copy_in(tg, target, (size_t)nq * 8, st));
    HIPCHK(hipMemsetAsync(pair, 0xFF, (size_t)nq * 8, st));   // NaN: a target outside the index keeps it
  }
  if ((r = lse_exact(x, qs.q32, qs.qn, nq, scale, lse, nullptr, st, true, tg, pair))) return r;
  x->search_stats[ST_LSE_EXACT] += nq;
  HIPCHK(copy_out(out_lse, lse, (size_t)nq * 8, st));
  if (pair) HIPCHK(copy_out(out_pair, pair, (size_t)nq * 8, st));
  HIPCHK(hipStreamSynchronize(st));   // workspaces are reused by the next call
  return CLM_OK;
}

// ---- threshold search (clm_index_search_above / _rows / _read) -------------------------------
// result(q) = the rows (s, id) with rank_ahead(s, id, tau[q], INT64_MAX): exact score s >= tau[q],
// NaN above every number, in the search order. The fast route lists, per query, every row whose
// fp16-pass score reaches theta = tau - RANK_MARGIN (EPI_FILTER): tau is exact and only the fp16-pass
// score carries error, the case RANK_MARGIN's comment bounds, so a row with s >= tau is always
// listed. The listed rows are re-scored exactly (lse_band_scores), those that pass are counted,
// placed and emitted as composites; the exact route takes them from windows of exact scores. Either
// way a query owns one segment of x->rg_comp, and range_finish sorts the segments and decodes them
// into the held result in CSR order. Both routes compare exact_cos scores against the same tau, so
// the result does not depend on the route.
struct RangeBuild {   // where each query's segment lies in x->rg_comp
  std::vector<int64_t> src, len;
  int64_t total = 0;
  void place(int64_t q, int64_t n) { src[q] = total; len[q] = n; total += n; }
};

// room for `need` composites in x->rg_comp, the first `used` kept; amortised as the index rows are
static int range_reserve(clm_index* x, int64_t used, int64_t need, hipStream_t st) {
  if (need <= x->rg_comp_cap) return CLM_OK;
  HIPCHK(hipStreamSynchronize(st));
  int64_t nc = std::max<int64_t>(std::max<int64_t>(need, 2 * x->rg_comp_cap), 1 << 16);
  uint64_t* p = nullptr;
  if (hipMalloc(&p, (size_t)nc * 8) != hipSuccess) {
    (void)hipGetLastError();
    nc = need;
    if (hipMalloc(&p, (size_t)nc * 8) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLM_E_OOM, "threshold search: a result of " + std::to_string(need) + " entries cannot be allocated");
    }
  }
  hipError_t e = used > 0 ? hipMemcpyAsync(p, x->rg_comp, (size_t)used * 8, hipMemcpyDeviceToDevice, st) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return fail(CLM_E_HIP, std::string("threshold search: ") + hipGetErrorString(e));
  }
  if (x->rg_comp) (void)hipFree(x->rg_comp);
  x->rg_comp = p;
  x->rg_comp_cap = nc;
  return CLM_OK;
}

// the per-query buffers of one filter pass over nb queries with `cap` list slots each
struct RangeBufs {
  size_t o_cnt, o_len, o_cur, o_plan, o_src, o_band, o_bs;
  void take(Layout& lay, int64_t nb, int64_t cap) {
    o_cnt = lay.take((size_t)nb * 4); o_len = lay.take((size_t)nb * 4); o_cur = lay.take((size_t)nb * 4);
    o_plan = lay.take((size_t)(nb + 1) * 4); o_src = lay.take((size_t)nb * 8);
    o_band = lay.take((size_t)nb * cap * 8); o_bs = lay.take((size_t)nb * cap * 4);
  }
};

// One filter pass for nb queries (global query numbers qid[0, nb)): EPI_FILTER lists the rows at or
// above theta (their fp16-pass scores go to band_s, which lse_band_scores then overwrites with the
// exact ones), range_keep_count counts the rows that pass, the counts come to the host and place the
// segments, range_emit fills them. Queries whose list exceeded `cap` go to over / ocount.
static int range_pass(clm_index* x, const unsigned* keys, const u16* q16, const float* qinv, const float* q32,
                      const double* qn, const float* tau, const float* theta, int64_t nb, int64_t cap, int cfg,
                      uint8_t* w, const RangeBufs& b, const int64_t* qid, RangeBuild& rb, std::vector<int64_t>& over,
                      std::vector<int64_t>& ocount, hipStream_t st) {
  int* cnt = (int*)(w + b.o_cnt);
  int* len = (int*)(w + b.o_len);
  int* cursor = (int*)(w + b.o_cur);
  int* plan = (int*)(w + b.o_plan);
  int64_t* src = (int64_t*)(w + b.o_src);
  int64_t* band = (int64_t*)(w + b.o_band);
  float* band_s = (float*)(w + b.o_bs);
  const ExactRows xr = exact_rows(x);
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)nb * 4, st));
  HIPCHK(hipMemsetAsync(len, 0, (size_t)nb * 4, st));
  HIPCHK(hipMemsetAsync(cursor, 0, (size_t)nb * 4, st));
  GemmArgs gf = index_pass(x, q16, qinv, nb, theta, cnt, band, cap);
  gf.cand_s = band_s;
  gf.cbound = keys;
  KCHK(gemm_cfg(false, EPI_FILTER, cfg, gf, st));
  KCHK(lse_band_scores(band, cnt, cap, q32, qn, (int)x->dim, xr.p, xr.f16, x->offset, nb, plan, band_s, st));
  KCHK(range_keep_count(band_s, band, cnt, cap, plan, tau, nb, len, st));
  std::vector<int> hcnt(nb), hlen(nb);
  HIPCHK(hipMemcpyAsync(hcnt.data(), cnt, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hlen.data(), len, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int64_t> hsrc(nb, 0);
  const int64_t used = rb.total;
  for (int64_t i = 0; i < nb; ++i) {
    if (hcnt[i] > cap) {
      over.push_back(qid[i]);
      ocount.push_back(hcnt[i]);
    } else {
      hsrc[i] = rb.total;
      rb.place(qid[i], hlen[i]);
    }
  }
  if (rb.total == used) return CLM_OK;
  if (int r = range_reserve(x, used, rb.total, st)) return r;
  HIPCHK(hipMemcpyAsync(src, hsrc.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
  KCHK(range_emit(band_s, band, cnt, cap, plan, tau, x->offset, nb, len, cursor, src, x->rg_comp, st));
  HIPCHK(hipStreamSynchronize(st));   // hsrc goes out of scope; the next pass rewrites the buffers
  return CLM_OK;
}

// The exact route for nq queries (global query numbers qid[0, nq), or 0 .. nq - 1): one walk of the
// row windows with count_rank (g = INT64_MAX) gives the lengths, a second one collects each
// window's passing (score, row) composites at the query's cursor.
static int range_exact(clm_index* x, const float* q32, const double* qn, const float* tau, int64_t nq,
                       const int64_t* qid, RangeBuild& rb, hipStream_t st) {
  const int dim = (int)x->dim;
  Layout hl;
  const size_t o_g = hl.take((size_t)nq * 8), o_ab = hl.take((size_t)nq * 8), o_cur = hl.take((size_t)nq * 8),
               o_end = hl.take((size_t)nq * 8);
  ExactWindows w;
  int r = exact_windows(x, nq, 4, hl.total(), &w);
  if (r) return r;
  float* sc = (float*)w.sc;
  int64_t* g = (int64_t*)(w.header + o_g);
  int64_t* above = (int64_t*)(w.header + o_ab);
  int64_t* cursor = (int64_t*)(w.header + o_cur);
  int64_t* end = (int64_t*)(w.header + o_end);
  std::vector<int64_t> hg(nq, INT64_MAX), hab(nq), hcur(nq), hend(nq);
  HIPCHK(hipMemcpyAsync(g, hg.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(above, 0, (size_t)nq * 8, st));
  r = walk_exact_windows(x, w, nq, [&](int64_t q0, int64_t nb, int64_t r0, int64_t rn, ExactRows er) -> int {
    KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, sc, w.ch, st));
    KCHK(count_rank(sc, w.ch, nb, rn, x->offset + r0, tau + q0, g + q0, above + q0, st));
    return CLM_OK;
  });
  if (r) return r;
  HIPCHK(hipMemcpyAsync(hab.data(), above, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t used = rb.total;
  for (int64_t i = 0; i < nq; ++i) {
    hcur[i] = rb.total;
    rb.place(qid ? qid[i] : i, hab[i]);
    hend[i] = rb.total;
  }
  if (rb.total == used) return CLM_OK;
  if ((r = range_reserve(x, used, rb.total, st))) return r;
  HIPCHK(hipMemcpyAsync(cursor, hcur.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(end, hend.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  r = walk_exact_windows(x, w, nq, [&](int64_t q0, int64_t nb, int64_t r0, int64_t rn, ExactRows er) -> int {
    KCHK(exact_scores(q32 + q0 * dim, qn + q0, nb, er.p, er.f16, rn, dim, sc, w.ch, st));
    KCHK(range_collect(sc, w.ch, nb, rn, r0, tau + q0, cursor + q0, end + q0, x->rg_comp, st));
    return CLM_OK;
  });
  if (r) return r;
  HIPCHK(hipStreamSynchronize(st));   // the host arrays go out of scope
  return CLM_OK;
}

// The fast route. Blocks are cut by band_query_block on the list bytes (12 B per slot): the block
// shrinks, never the capacity. `skip` marks the queries the exact route must serve whatever their
// list holds (theta = +inf keeps their lists empty). Overflowed lists are redone with a capacity of
// count + count / 8 + 256, gathered and grouped as overflow_wide does within the same 1 GiB; a list
// that overflows again (or would not fit) is appended to `exact`.
static int range_band(clm_index* x, const unsigned* keys, const QueryStage& qs, const float* tau, const float* theta,
                      int64_t nq, int64_t cap, RangeBuild& rb, std::vector<int64_t>& exact, int64_t& overflowed,
                      hipStream_t st) {
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  int r;
  std::vector<int64_t> over, ocount, ids(nq);
  for (int64_t i = 0; i < nq; ++i) ids[i] = i;
  {
    const int64_t nqb = band_query_block(nq, cap * 12, 1);
    Layout lay;
    RangeBufs b;
    b.take(lay, nqb, cap);
    if ((r = grow(&x->ws2, &x->ws2_bytes, lay.total()))) return r;
    for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
      const int64_t nb = std::min(nqb, nq - q0);
      if ((r = range_pass(x, keys, qs.q16 + q0 * dim, qs.qinv + q0, qs.q32 + q0 * dim, qs.qn + q0, tau + q0,
                          theta + q0, nb, cap, -1, (uint8_t*)x->ws2, b, ids.data() + q0, rb, over, ocount, st)))
        return r;
    }
  }
  overflowed = (int64_t)over.size();
  if (over.empty()) return CLM_OK;
  std::vector<int64_t> wide;
  int64_t cap_max = 0;
  for (size_t j = 0; j < over.size(); ++j) {
    const int64_t cap2 = std::min<int64_t>(N, wide_capacity(ocount[j]));
    if (cap2 * 12 <= ((int64_t)1 << 30)) {
      wide.push_back(over[j]);
      cap_max = std::max(cap_max, cap2);
    } else {
      exact.push_back(over[j]);
    }
  }
  if (wide.empty()) return CLM_OK;
  RangeBufs b;
  return wide_groups(   // gathered: in[0] = q16, [1] = qinv, [2] = q32, [3] = qn, [4] = theta, [5] = tau
      x, wide, cap_max,
      {{qs.q16, (int64_t)dim * 2}, {qs.qinv, 4}, {qs.q32, (int64_t)dim * 4}, {qs.qn, 8}, {theta, 4}, {tau, 4}}, st,
      [&](Layout& lay, int64_t G) { b.take(lay, G, cap_max); },
      [&](uint8_t* w, void* const* in, const int64_t*, int64_t g0, int64_t ng) -> int {
        // these lists overflowed: dense_cfg, overflow_wide's choice. range_pass drains the stream
        std::vector<int64_t> ocount2;
        return range_pass(x, keys, (const u16*)in[0], (const float*)in[1], (const float*)in[2], (const double*)in[3],
                          (const float*)in[5], (const float*)in[4], ng, cap_max, dense_cfg(), w, b, wide.data() + g0, rb,
                          exact, ocount2, st);
      });
}

// Segmented sort of the placed segments and the decode into the held result, in CSR order.
static int range_finish(clm_index* x, const RangeBuild& rb, int64_t nq, int64_t* out_offsets, hipStream_t st) {
  std::vector<int64_t> off(nq + 1, 0);
  for (int64_t q = 0; q < nq; ++q) off[q + 1] = off[q] + rb.len[q];
  const int64_t total = off[nq];
  // work items: LDS runs, merge chunks of the segments longer than one run, decode chunks (the
  // short segments from the first buffer, the long ones from wherever the last merge pass left them)
  constexpr int64_t DECODE_CHUNK = 4096;
  std::vector<RangeItem> runs, merges, dec_a, dec_b;
  int64_t longest = 0, longest_run = 0;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t n = rb.len[q], s0 = rb.src[q];
    if (n <= 0) continue;
    const bool is_long = n > RANGE_RUN;
    for (int64_t a = 0; a < n; a += RANGE_RUN) {
      const int64_t m = std::min<int64_t>(RANGE_RUN, n - a);
      if (m >= 2) runs.push_back(RangeItem{s0 + a, 0, m});
      longest_run = std::max(longest_run, m);
    }
    if (is_long) {
      longest = std::max(longest, n);
      for (int64_t a = 0; a < n; a += RANGE_MERGE_CHUNK) merges.push_back(RangeItem{s0, a, n});
    }
    for (int64_t a = 0; a < n; a += DECODE_CHUNK)
      (is_long ? dec_b : dec_a).push_back(RangeItem{s0 + a, off[q] + a, std::min<int64_t>(DECODE_CHUNK, n - a)});
  }
  if (total > 0) {
    if (total > x->res_cap) {   // the held result's own arrays, 12 B per entry, amortised as the index rows are
      HIPCHK(hipStreamSynchronize(st));
      float* ns = nullptr;
      int64_t* ni = nullptr;
      auto alloc = [&](int64_t rows) {
        if (hipMalloc(&ns, (size_t)rows * 4) == hipSuccess && hipMalloc(&ni, (size_t)rows * 8) == hipSuccess) return true;
        (void)hipGetLastError();
        if (ns) (void)hipFree(ns);
        ns = nullptr; ni = nullptr;
        return false;
      };
      int64_t nc = std::max<int64_t>(total, 2 * x->res_cap);
      if (!alloc(nc)) {
        nc = total;
        if (!alloc(nc))
          return fail(CLM_E_OOM, "threshold search: a result of " + std::to_string(total) + " entries cannot be allocated");
      }
      if (x->res_s) (void)hipFree(x->res_s);
      if (x->res_i) (void)hipFree(x->res_i);
      x->res_s = ns; x->res_i = ni; x->res_cap = nc;
      x->res_valid = false;
    }
    if (longest > 0 && x->rg_comp2_cap < x->rg_comp_cap) {   // the merge passes' second buffer
      HIPCHK(hipStreamSynchronize(st));
      if (x->rg_comp2) (void)hipFree(x->rg_comp2);
      x->rg_comp2 = nullptr; x->rg_comp2_cap = 0;
      if (hipMalloc(&x->rg_comp2, (size_t)x->rg_comp_cap * 8) != hipSuccess) {
        (void)hipGetLastError();
        x->rg_comp2 = nullptr;
        return fail(CLM_E_OOM, "threshold search: a result of " + std::to_string(total) + " entries cannot be sorted");
      }
      x->rg_comp2_cap = x->rg_comp_cap;
    }
    const size_t isz = sizeof(RangeItem);
    Layout lay;
    const size_t o_runs = lay.take(runs.size() * isz), o_mer = lay.take(merges.size() * isz),
                 o_da = lay.take(dec_a.size() * isz), o_db = lay.take(dec_b.size() * isz);
    if (int r = grow(&x->rg_items, &x->rg_items_bytes, lay.total(), "threshold search work items")) return r;
    uint8_t* w = (uint8_t*)x->rg_items;
    auto up = [&](size_t o, const std::vector<RangeItem>& v) {
      return v.empty() ? hipSuccess : hipMemcpyAsync(w + o, v.data(), v.size() * isz, hipMemcpyHostToDevice, st);
    };
    HIPCHK(up(o_runs, runs));
    HIPCHK(up(o_mer, merges));
    HIPCHK(up(o_da, dec_a));
    HIPCHK(up(o_db, dec_b));
    x->res_valid = false;   // the held result is rewritten from here on
    KCHK(range_sort_runs(x->rg_comp, (const RangeItem*)(w + o_runs), (int64_t)runs.size(), longest_run, st));
    uint64_t *a = x->rg_comp, *b2 = x->rg_comp2;
    for (int64_t L = RANGE_RUN; L < longest; L <<= 1) {
      KCHK(range_merge(a, b2, (const RangeItem*)(w + o_mer), (int64_t)merges.size(), L, st));
      std::swap(a, b2);
    }
    KCHK(range_decode(x->rg_comp, (const RangeItem*)(w + o_da), (int64_t)dec_a.size(), x->offset, x->res_s, x->res_i, st));
    KCHK(range_decode(a, (const RangeItem*)(w + o_db), (int64_t)dec_b.size(), x->offset, x->res_s, x->res_i, st));
  }
  if (is_device_ptr(out_offsets)) HIPCHK(hipMemcpyAsync(out_offsets, off.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
  else std::memcpy(out_offsets, off.data(), (size_t)(nq + 1) * 8);
  HIPCHK(hipStreamSynchronize(st));   // the host vectors go out of scope; workspaces are reused by the next call
  x->res_n = total;
  x->res_valid = true;
  return CLM_OK;
}

// Router, as rank_run's: the whole call takes the exact route for a zero or non-finite inverse norm
// in the index, dim > MARGIN_MAX_DIM, N > 2^31 - 1, nq x N <= 2^24 (unless CLM_RANK_BAND /
// $CLM_SEARCH_BOUNDED=1), CLM_RANK_EXACT or $CLM_SEARCH_FULL=1; single queries do when their list
// overflows twice, when tau is not finite, or when the query's norm is zero, non-finite or outside
// [1e-30, 1e30] (its fp16 operand is then not a unit row and its exact scores may be NaN, which the
// fp16 pass never lists).
static int range_run(clm_index* x, const void* q, int q_dtype, int64_t nq, const float* threshold,
                     int64_t* out_offsets, int band_cap, void* stream) {
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (x->n > 0xFFFFFFFFll) return fail(CLM_E_ARG, "threshold search: at most 2^32 - 1 rows per index");
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  RangeBuild rb;
  rb.src.assign(nq, 0);
  rb.len.assign(nq, 0);
  if (nq == 0) return range_finish(x, rb, 0, out_offsets, st);
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  std::vector<float> htau(nq), hth(nq);
  if (is_device_ptr(threshold)) {
    HIPCHK(hipMemcpyAsync(htau.data(), threshold, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    std::memcpy(htau.data(), threshold, (size_t)nq * 4);
  }
  Layout lay;
  const size_t o_tau = lay.take((size_t)nq * 4), o_th = lay.take((size_t)nq * 4);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, lay.total(), st, &qs);
  if (r) return r;
  float* tau = (float*)(qs.extra + o_tau);
  float* theta = (float*)(qs.extra + o_th);
  HIPCHK(hipMemcpyAsync(tau, htau.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
  std::vector<double> hqn(nq);
  HIPCHK(hipMemcpyAsync(hqn.data(), qs.qn, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
  const unsigned* keys = nullptr;
  bool inv_ok = false;
  if ((r = inv_norms_finite(x, st, &inv_ok, &keys))) return r;   // drains the stream
  const int flags = band_cap > 0 ? band_cap & (CLM_RANK_EXACT | CLM_RANK_BAND) : 0;
  const bool all_exact = whole_call_exact(x, nq, inv_ok, (flags & CLM_RANK_EXACT) || env_flag("CLM_SEARCH_FULL"),
                                         (flags & CLM_RANK_BAND) || env_flag("CLM_SEARCH_BOUNDED"));
  int64_t n_fast = 0, n_exact = nq, n_over = 0;
  if (all_exact) {
    if ((r = range_exact(x, qs.q32, qs.qn, tau, nq, nullptr, rb, st))) return r;
  } else {
    std::vector<int64_t> exact;
    for (int64_t i = 0; i < nq; ++i) {
      const bool q_ok = hqn[i] >= 1e-30 && hqn[i] <= 1e30;
      if (q_ok && std::fabs(htau[i]) <= 3.4028235e38f) {
        hth[i] = htau[i] - RANK_MARGIN;
      } else {
        hth[i] = INFINITY;   // lists nothing: the exact route serves the query
        exact.push_back(i);
      }
    }
    HIPCHK(hipMemcpyAsync(theta, hth.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    if ((r = stage_queries_f16(x, qs, nq, st))) return r;
    if ((r = range_band(x, keys, qs, tau, theta, nq, band_capacity(band_cap, N), rb, exact, n_over, st))) return r;
    n_exact = (int64_t)exact.size();
    n_fast = nq - n_exact;
    // their queries, norms and thresholds gathered; one exact pass places and fills their segments
    r = redo_subset(x, exact, {{qs.q32, (int64_t)dim * 4}, {qs.qn, 8}, {tau, 4}}, {}, "threshold search", st,
                    [&](void* const* in, void* const*) -> int {
                      return range_exact(x, (const float*)in[0], (const double*)in[1], (const float*)in[2],
                                         (int64_t)exact.size(), exact.data(), rb, st);
                    });
    if (r) return r;
  }
  if ((r = range_finish(x, rb, nq, out_offsets, st))) return r;
  x->search_stats[ST_RANGE_FAST] += n_fast;
  x->search_stats[ST_RANGE_EXACT] += n_exact;
  x->search_stats[ST_RANGE_OVERFLOW] += n_over;
  return CLM_OK;
}

int clm_index_search_above(clm_index* x, const void* q, int q_dtype, int64_t nq, const float* threshold,
                           int64_t* out_offsets, int band_cap, void* stream) {
  if (!x || nq < 0 || !out_offsets || (nq > 0 && (!q || !threshold))) return fail(CLM_E_ARG, "bad argument");
  return range_run(x, q, q_dtype, nq, threshold, out_offsets, band_cap, stream);
}

int clm_index_search_above_rows(clm_index* x, int64_t row0, int64_t nrows, const float* threshold,
                                int64_t* out_offsets, int band_cap, void* stream) {
  if (!x || nrows < 0 || !out_offsets || (nrows > 0 && !threshold)) return fail(CLM_E_ARG, "bad argument");
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (row0 < x->offset || row0 - x->offset > x->n || nrows > x->n - (row0 - x->offset))
    return fail(CLM_E_ARG, "rows [" + std::to_string(row0) + ", " + std::to_string(row0) + " + " + std::to_string(nrows) +
                               ") are outside the index [" + std::to_string(x->offset) + ", " +
                               std::to_string(x->offset + x->n) + ")");
  const ExactRows er = exact_rows(x, row0 - x->offset);   // the queries stay where they are, in HBM
  return range_run(x, er.p, er.f16 ? CLM_F16 : CLM_F32, nrows, threshold, out_offsets, band_cap, stream);
}

int clm_index_search_above_read(clm_index* x, int64_t start, int64_t n, float* out_scores, int64_t* out_idx,
                                void* stream) {
  if (!x || (n > 0 && (!out_scores || !out_idx))) return fail(CLM_E_ARG, "bad argument");
  if (!x->res_valid) return fail(CLM_E_STATE, "no threshold-search result is held (none yet, or the index changed since)");
  if (start < 0 || n < 0 || start > x->res_n || n > x->res_n - start)
    return fail(CLM_E_STATE, "entries [" + std::to_string(start) + ", " + std::to_string(start) + " + " +
                                 std::to_string(n) + ") are outside the held result of " + std::to_string(x->res_n));
  if (n == 0) return CLM_OK;
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(copy_out(out_scores, x->res_s + start, (size_t)n * 4, st));
  HIPCHK(copy_out(out_idx, x->res_i + start, (size_t)n * 8, st));
  HIPCHK(hipStreamSynchronize(st));
  return CLM_OK;
}

// ---- streaming softmax gradients (clm_index_softmax_grad) -------------------------------------
// dq[i] = sum_j W_ij r^_j and dr[j] = sum_i W_ij q^_i with W_ij = wq exp(scale s_ij - q_lse[i]) + wr
// exp(scale s_ij - row_lse[j]) over the fp16-pass scores, per (row chunk, query block): the EPI_SOFTW
// GEMM writes the block's fp16 weights W16 [nb, C], transpose16 gives W16T [C, nb], and the two fp16
// GEMMs accumulate in fp32 into the outputs (EPI_RESID, or gemm_splitk_resid where the tiles are short
// of a round of the CUs). Their other operands are K-contiguous transposes made once per chunk / per
// call with the inverse norms folded in: R^T [dim, C] and Q^T [dim, nq]. Chunks outside, blocks inside:
// every output element is added to by launches in stream order, and no kernel uses a floating-point
// atomic, so a call's bits are a function of its arguments.
//
// Scaling: with a = wq / wmax, b = wr / wmax (wmax the larger weight) a stored weight is
// 2^p (a exp(..) + b exp(..)); an exponential is at most exp(2 scale E) for offsets within scale E of
// the true log-sum-exps (the fp16-pass score adds the other scale E), so 2^p = 65504 / ((a + b) exp(2
// scale E)) puts the largest possible weight on the largest fp16 and every weight above 2^-14 / 65504
// = 9.3e-10 of it in fp16's normal range. log2 a + p and log2 b + p go into the offset arrays, wmax 2^-p
// multiplies the fp32 results.
constexpr int64_t GRAD_CHUNK_ROWS = 4096;    // default C (profiles/loss_grad_ab.txt)
constexpr int64_t GRAD_QUERY_BLOCK = 32768;  // default cap of B

// K slices of an accumulating GEMM [M, N] (0: the plain EPI_RESID GEMM): its 128 x 128 tiles short of
// half the CUs' 2-per-CU slots, the largest divisor of K / 64 up to 8; $CLM_GRAD_SLICES overrides (A/B)
static int grad_slices(int64_t M, int64_t N, int64_t K) {
  static const int64_t forced = env_int("CLM_GRAD_SLICES", -1);
  const int64_t ksteps = K / 64;
  int64_t want = 8;
  if (forced >= 0) want = forced;
  else if (((M + 127) / 128) * ((N + 127) / 128) >= 256) return 0;
  for (int64_t s = std::min<int64_t>(want, ksteps); s >= 2; --s)
    if (ksteps % s == 0) return (int)s;
  return 0;
}

// out[M, N] += A[M, K] . W[N, K]^T, fp16 operands, fp32 accumulation into out (ldo = N)
static int grad_accumulate(const u16* A, int64_t lda, const u16* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                           float* out, int slices, float* part, hipStream_t st) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.out = out; g.ldo = N;
  if (slices >= 2) KCHK(gemm_splitk_resid(false, g, slices, part, st));
  else KCHK(gemm(false, EPI_RESID, g, st));
  return CLM_OK;
}

int clm_index_softmax_grad(clm_index* x, const void* q, int q_dtype, int64_t nq, double scale, const double* q_lse,
                           const double* row_lse, double wq, double wr, float* out_dq, float* out_dr,
                           int64_t chunk_rows, int64_t query_block, void* stream) {
  if (!x || nq < 0 || chunk_rows < 0 || query_block < 0 || (nq > 0 && (!q || !q_lse)))
    return fail(CLM_E_ARG, "bad argument");
  if (int rc = check_query_dtype(q_dtype)) return rc;
  if (!(scale > 0.0 && scale <= 1.7976931348623157e308)) return fail(CLM_E_ARG, "scale must be finite and positive");
  if (!(wq >= 0.0 && wq <= 1.7976931348623157e308) || !(wr >= 0.0 && wr <= 1.7976931348623157e308))
    return fail(CLM_E_ARG, "the weights must be finite and not negative");
  if (wr > 0.0 && !row_lse) return fail(CLM_E_ARG, "wr > 0 needs row_lse");
  if (x->n == 0) return fail(CLM_E_ARG, "the index is empty");
  if (x->dim > MARGIN_MAX_DIM) return fail(CLM_E_ARG, "softmax_grad: dim > 8192 is outside the fp16 pass's bound");
  if (x->n > 0x7FFFFFFF) return fail(CLM_E_ARG, "softmax_grad: more than 2^31 - 1 rows");
  if (nq == 0) return CLM_OK;
  DeviceGuard guard(x->dev);
  hipStream_t st = (hipStream_t)stream;
  const int dim = (int)x->dim;
  const int64_t N = x->n;
  const bool use_r = row_lse && wr > 0.0;

  Layout ql;
  const size_t o_lse = ql.take((size_t)nq * 8), o_lq = ql.take((size_t)nq * 4);
  QueryStage qs;
  int r = stage_queries(x, q, q_dtype, nq, ql.total(), st, &qs);
  if (r) return r;
  double* lse_d = (double*)(qs.extra + o_lse);
  float* lq = (float*)(qs.extra + o_lq);
  HIPCHK(copy_in(lse_d, q_lse, (size_t)nq * 8, st));
  if ((r = stage_queries_f16(x, qs, nq, st))) return r;
  std::vector<double> hqn((size_t)nq);
  HIPCHK(hipMemcpyAsync(hqn.data(), qs.qn, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
  bool inv_ok = false;
  if ((r = inv_norms_finite(x, st, &inv_ok))) return r;   // drains the stream: hqn is here too
  if (!inv_ok) return fail(CLM_E_ARG, "softmax_grad: the index holds a row whose norm is zero or not finite");
  for (int64_t i = 0; i < nq; ++i)
    if (!(hqn[i] > 0.0 && hqn[i] <= 1.7976931348623157e308))
      return fail(CLM_E_ARG, "softmax_grad: query " + std::to_string(i) + " has a zero or non-finite norm");

  // blocks and chunks: multiples of 64 (the GEMMs' K granule and the operands' 16-byte alignment)
  const int64_t nqp = round_up(nq, 64);
  int64_t C = std::min(round_up(chunk_rows > 0 ? chunk_rows : GRAD_CHUNK_ROWS, 64), round_up(N, 64));
  int64_t B = std::min(round_up(query_block > 0 ? query_block : GRAD_QUERY_BLOCK, 64), nqp);
  if (query_block == 0) {   // the two W buffers within the workspace budget (band_query_block's rule)
    size_t fr = 0, tot = 0;
    int64_t cap_b = env_int("CLM_SEARCH_WS_MB", 8192) << 20;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) cap_b = std::min<int64_t>(cap_b, (int64_t)(fr / 4));
    else (void)hipGetLastError();
    const int64_t fit = cap_b / (C * 2 * (out_dr ? 2 : 1)) / 64 * 64;
    B = std::max<int64_t>(64, std::min(B, fit));
  }
  const bool dq_direct = out_dq && is_device_ptr(out_dq), dr_direct = out_dr && is_device_ptr(out_dr);
  const int sl_q = out_dq ? grad_slices(B, dim, C) : 0, sl_r = out_dr ? grad_slices(C, dim, B) : 0;
  Layout lay;
  const size_t o_rlse = lay.take(use_r ? (size_t)N * 8 : 0), o_lr = lay.take(use_r ? (size_t)N * 4 : 0),
               o_qt = lay.take(out_dr ? (size_t)dim * nqp * 2 : 0), o_rt = lay.take(out_dq ? (size_t)dim * C * 2 : 0),
               o_w = lay.take((size_t)B * C * 2), o_wt = lay.take(out_dr ? (size_t)C * B * 2 : 0),
               o_dq = lay.take(out_dq && !dq_direct ? (size_t)nq * dim * 4 : 0),
               o_dr = lay.take(out_dr && !dr_direct ? (size_t)C * dim * 4 : 0),
               o_part = lay.take(std::max(sl_q ? gemm_splitk_ws_bytes((int)B, dim, sl_q) : 0,
                                          sl_r ? gemm_splitk_ws_bytes((int)C, dim, sl_r) : 0));
  if ((r = grow(&x->ws2, &x->ws2_bytes, lay.total()))) return r;
  uint8_t* w = (uint8_t*)x->ws2;
  float* lr = use_r ? (float*)(w + o_lr) : nullptr;
  u16 *QT = (u16*)(w + o_qt), *RT = (u16*)(w + o_rt), *W16 = (u16*)(w + o_w), *W16T = (u16*)(w + o_wt);
  float* dq = !out_dq ? nullptr : dq_direct ? out_dq : (float*)(w + o_dq);
  float* part = (float*)(w + o_part);

  const double a = use_r && wr > wq ? wq / wr : 1.0, b = !use_r ? 0.0 : wr > wq ? 1.0 : wr / wq;
  const double wmax = use_r && wr > wq ? wr : wq;
  if (wmax == 0.0) {   // no weight at all: the sums are zero
    if (dq_direct) HIPCHK(hipMemsetAsync(out_dq, 0, (size_t)nq * dim * 4, st));
    else if (out_dq) std::memset(out_dq, 0, (size_t)nq * dim * 4);
    if (dr_direct) HIPCHK(hipMemsetAsync(out_dr, 0, (size_t)N * dim * 4, st));
    else if (out_dr) std::memset(out_dr, 0, (size_t)N * dim * 4);
    HIPCHK(hipStreamSynchronize(st));
    return CLM_OK;
  }
  const double p = std::log2(65504.0) - std::log2(a + b) - 2.0 * scale * LSE_E * 1.4426950408889634;
  const float unscale = (float)(wmax * std::exp2(-p));
  // log2(0) = -inf makes the offsets of an absent term +inf: exp2(x - inf) = 0
  KCHK(softw_offsets(lse_d, nq, std::log2(a) + p, lq, st));
  if (use_r) {
    HIPCHK(copy_in(w + o_rlse, row_lse, (size_t)N * 8, st));
    KCHK(softw_offsets((const double*)(w + o_rlse), N, std::log2(b) + p, lr, st));
  }
  // every weight ever stored is finite (EPI_SOFTW clamps): zeros first, so the columns between a
  // ragged chunk's end and its K granule multiply the transposes' zero padding with finite values
  HIPCHK(hipMemsetAsync(W16, 0, (size_t)B * C * 2, st));
  if (out_dr) KCHK(transpose16(qs.q16, dim, nq, dim, qs.qinv, QT, nqp, st));
  if (out_dq) HIPCHK(hipMemsetAsync(dq, 0, (size_t)nq * dim * 4, st));

  int64_t passes = 0;
  for (int64_t r0 = 0; r0 < N; r0 += C) {
    const int64_t cn = std::min(C, N - r0), ck = round_up(cn, 64);
    float* drc = !out_dr ? nullptr : dr_direct ? out_dr + r0 * dim : (float*)(w + o_dr);
    if (out_dr) HIPCHK(hipMemsetAsync(drc, 0, (size_t)cn * dim * 4, st));
    if (out_dq) KCHK(transpose16(x->rows + r0 * dim, dim, cn, dim, x->inv + r0, RT, C, st));
    for (int64_t q0 = 0; q0 < nq; q0 += B, ++passes) {
      const int64_t nb = std::min(B, nq - q0), bk = round_up(nb, 64);
      GemmArgs g{};
      g.A = qs.q16 + q0 * dim; g.lda = dim; g.W = x->rows + r0 * dim; g.ldw = dim;
      g.M = (int)nb; g.N = (int)cn; g.K = dim;
      g.rscale = qs.qinv + q0; g.cscale = x->inv + r0;
      g.theta = lq + q0; g.theta_ld = 1; g.bias = lr ? lr + r0 : nullptr; g.lse_c = (float)(scale * 1.4426950408889634);
      g.out = W16; g.ldo = C;
      KCHK(gemm_cfg(false, EPI_SOFTW, -1, g, st));
      if (out_dq && (r = grad_accumulate(W16, C, RT, C, nb, dim, ck, dq + q0 * dim, sl_q && ck % (64 * sl_q) == 0 ? sl_q : 0, part, st)))
        return r;
      if (out_dr) {
        KCHK(transpose16(W16, C, nb, cn, nullptr, W16T, B, st));
        if ((r = grad_accumulate(W16T, B, QT + q0, nqp, cn, dim, bk, drc, sl_r && bk % (64 * sl_r) == 0 ? sl_r : 0, part, st)))
          return r;
      }
    }
    if (out_dr) {
      KCHK(scale_f32(drc, cn * dim, unscale, st));
      if (!dr_direct) HIPCHK(copy_out(out_dr + r0 * dim, drc, (size_t)cn * dim * 4, st));
    }
  }
  if (out_dq) {
    KCHK(scale_f32(dq, nq * dim, unscale, st));
    if (!dq_direct) HIPCHK(copy_out(out_dq, dq, (size_t)nq * dim * 4, st));
  }
  x->search_stats[ST_GRAD_QUERIES] += nq;
  x->search_stats[ST_GRAD_PASSES] += passes;
  HIPCHK(hipStreamSynchronize(st));   // workspaces are reused by the next call
  return CLM_OK;
}

// test hooks: the EPI_SOFTW epilogue and the transposing copy alone
int clm_gemm_softw(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N,
                   int K, const float* rscale, const float* cscale, const float* lq, const float* lr, float c,
                   void* out, int64_t ldo, void* stream) {
  if (config >= gemm_num_configs()) return fail(CLM_E_ARG, "bad config");
  if (M < 0 || N < 0 || K <= 0 || K % 64 || lda % 8 || ldw % 8 || lda < K || ldw < K || ldo < N)
    return fail(CLM_E_ARG, "bad shape (K % 64 == 0; lda, ldw multiples of 8 and >= K; ldo >= N)");
  if (M == 0 || N == 0) return CLM_OK;
  if (!A || !W || !lq || !out || ((uintptr_t)lr & 15)) return fail(CLM_E_ARG, "gemm_softw: null pointer or misaligned lr");
  DeviceGuard g(hip_device);
  GemmArgs a{};
  a.A = (const u16*)A; a.lda = lda; a.W = (const u16*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.rscale = rscale; a.cscale = cscale; a.theta = lq; a.theta_ld = 1; a.bias = lr; a.lse_c = c; a.out = out; a.ldo = ldo;
  hipError_t e = gemm_cfg(false, EPI_SOFTW, config, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_transpose16(int hip_device, const void* src, int64_t lds, int64_t rows, int64_t cols, const float* s,
                    void* dst, int64_t ldd, void* stream) {
  if (rows < 0 || cols < 0 || lds < cols || ldd < round_up(rows, 64))
    return fail(CLM_E_ARG, "transpose16: rows, cols >= 0, lds >= cols, ldd >= round_up(rows, 64)");
  if (rows == 0 || cols == 0) return CLM_OK;
  if (!src || !dst) return fail(CLM_E_ARG, "transpose16: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = transpose16((const u16*)src, lds, rows, cols, s, (u16*)dst, ldd, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("transpose16: ") + hipGetErrorString(e));
  return CLM_OK;
}
