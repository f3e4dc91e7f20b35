// libclm C-ABI, the stand-alone entry points: exact cosine scores, the search building blocks the
// tests and tools drive on their own (thresholds, scan16, collect_ge, top-k merge), row
// normalisation / fusion, and the image resize + crop with its synthetic-image generator.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "capi_internal.hpp"

using namespace clm;
using namespace clm::capi;

namespace {

// Grow-only per-device scratch for the entry points that stage host buffers (resize_crop,
// cosine_scores, topk_merge, l2_normalize, fuse_queries): no hipMalloc / hipFree per call -- hipFree
// synchronises the whole device, which stalled work queued on other streams (the concurrent tower
// stream) behind a single-image encode. A caller holds the device's lock until its stream has
// drained the scratch (every such entry point synchronises its stream before returning).
struct Scratch {
  std::mutex mu;
  void* p = nullptr;
  size_t bytes = 0;
};
// A call that needed more than SCRATCH_KEEP bytes (a one-off host-staged score matrix, a resize
// of large photos) frees its scratch once its stream has drained it, so that peak does not stay
// allocated for the life of the process (the caller holds scr.mu)
constexpr size_t SCRATCH_KEEP = (size_t)256 << 20;
void scratch_trim(Scratch& scr) {
  if (scr.bytes <= SCRATCH_KEEP) return;
  (void)hipFree(scr.p);
  (void)hipGetLastError();
  scr.p = nullptr;
  scr.bytes = 0;
}
Scratch& scratch_of_current_device() {
  static Scratch s[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
  return s[d & 63];
}
int scratch_grow(Scratch& scr, size_t bytes) { return grow(&scr.p, &scr.bytes, bytes); }
}  // namespace

extern "C" {

// similarity.cosine_similarity (similarity.py:10-33): every score exact (fp32-rounded fp64 cosine)
int clm_cosine_scores(int hip_device, const float* q, int64_t nq, const float* c, int64_t n, int dim, float* out,
                      void* stream) {
  if (nq < 0 || n < 0 || dim <= 0 || (nq * n > 0 && (!q || !c || !out)))
    return fail(CLM_E_ARG, "bad argument");
  if (nq == 0 || n == 0) return CLM_OK;
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  const bool qd = is_device_ptr(q), cd = is_device_ptr(c), od = is_device_ptr(out);
  Layout lay;
  const size_t o_qn = lay.take((size_t)nq * 8), o_q = qd ? 0 : lay.take((size_t)nq * dim * 4),
               o_c = cd ? 0 : lay.take((size_t)n * dim * 4), o_o = od ? 0 : lay.take((size_t)nq * n * 4);
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  if (int rg = scratch_grow(scr, lay.total())) return rg;
  uint8_t* w = (uint8_t*)scr.p;
  double* qn = (double*)(w + o_qn);
  const float* qs = q;
  const float* cs = c;
  float* os = od ? out : (float*)(w + o_o);
  int rc = CLM_OK;
  hipError_t e = hipSuccess;
  if (!qd) { float* t = (float*)(w + o_q); e = hipMemcpyAsync(t, q, (size_t)nq * dim * 4, hipMemcpyHostToDevice, st); qs = t; }
  if (e == hipSuccess && !cd) { float* t = (float*)(w + o_c); e = hipMemcpyAsync(t, c, (size_t)n * dim * 4, hipMemcpyHostToDevice, st); cs = t; }
  if (e == hipSuccess) e = query_norms(qs, nq, dim, qn, st);
  if (e == hipSuccess) e = exact_scores(qs, qn, nq, cs, false, n, dim, os, n, st);
  if (e == hipSuccess && !od) e = hipMemcpyAsync(out, os, (size_t)nq * n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  scratch_trim(scr);
  if (e != hipSuccess) rc = fail(CLM_E_HIP, std::string("cosine_scores: ") + hipGetErrorString(e));
  return rc;
}

int clm_topk_threshold(int hip_device, const float* scores, int64_t lds, int64_t nq, int64_t C, int k, float margin,
                       int method, float* th, void* stream) {
  if (nq < 0 || C < k || lds < C || k < 1 || k > (method == 0 ? 8 : 1024) || (method != 0 && method != 1))
    return fail(CLM_E_ARG, "bad threshold shape (k <= C <= lds; k <= 8 streaming, <= 1024 radix)");
  if (nq == 0) return CLM_OK;
  if (!is_device_ptr(scores) || !is_device_ptr(th)) return fail(CLM_E_ARG, "topk_threshold: device pointers");
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  if (method == 0) {
    KCHK(kth_thresholds(scores, lds, nq, C, k, margin, th, st));
    return CLM_OK;
  }
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  Layout lay;
  const size_t o_ts = lay.take((size_t)nq * k * 4), o_ti = lay.take((size_t)nq * k * 8);
  if (int rg = scratch_grow(scr, lay.total())) return rg;
  float* ts = (float*)((uint8_t*)scr.p + o_ts);
  int64_t* ti = (int64_t*)((uint8_t*)scr.p + o_ti);
  KCHK(topk_rows(scores, lds, nq, C, k, 0, ts, ti, k, st));
  KCHK(filter_thresholds(ts, k, nq, k, margin, th, st));
  HIPCHK(hipStreamSynchronize(st));   // the scratch is reused by the next call
  scratch_trim(scr);
  return CLM_OK;
}

int clm_scan16(int hip_device, const uint16_t* rows16, const float* inv, int64_t N, int dim, const uint16_t* q16,
               const float* qinv, int nq, float* out, int64_t ldo, float* cmax, float* wtop, int64_t ldw,
               void* stream) {
  if (N < 0 || nq < 0) return fail(CLM_E_ARG, "scan16: bad shape");
  if (N == 0 || nq == 0) return CLM_OK;
  if (!is_device_ptr(rows16) || !is_device_ptr(inv) || !is_device_ptr(q16) || !is_device_ptr(qinv) ||
      !is_device_ptr(out) || !is_device_ptr(cmax) || (wtop && !is_device_ptr(wtop)))
    return fail(CLM_E_ARG, "scan16: device pointers");
  DeviceGuard g(hip_device);
  Scan16Args a{};
  a.rows = rows16; a.inv = inv; a.N = N; a.dim = dim;
  a.q16 = q16; a.qinv = qinv; a.nq = nq;
  a.out = out; a.ldo = ldo; a.cmax = cmax; a.nchunk = (N + 255) / 256;
  a.wtop = wtop; a.ldw = ldw;
  const hipError_t e = scan16(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(CLM_E_ARG, "scan16: dim % 64 == 0 in [64, 1024], nq <= 16, ldo a power of two in [nq, 16], ldw >= 8 waves");
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("scan16: ") + hipGetErrorString(e));
  return CLM_OK;
}

int64_t clm_scan16_waves(int hip_device, int64_t N, int dim) {
  DeviceGuard g(hip_device);
  return scan16_waves((std::max<int64_t>(N, 0) + 255) / 256, dim);
}

int clm_collect_ge(int hip_device, const float* scores, int ldq, int nq, int64_t C, const float* th, int* cnt, int cap,
                   float* cand_s, int64_t* cand_i, int64_t base, void* stream) {
  if (nq < 0 || C < 0 || cap < 0) return fail(CLM_E_ARG, "collect_ge: bad shape");
  if (nq == 0 || C == 0) return CLM_OK;
  if (!is_device_ptr(scores) || !is_device_ptr(th) || !is_device_ptr(cnt) || !is_device_ptr(cand_s) ||
      !is_device_ptr(cand_i))
    return fail(CLM_E_ARG, "collect_ge: device pointers");
  DeviceGuard g(hip_device);
  const hipError_t e = collect_ge(scores, ldq, nq, C, th, cnt, cap, cand_s, cand_i, base, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(CLM_E_ARG, "collect_ge: ldq a power of two in [nq, 16], scores 16-byte aligned");
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("collect_ge: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_topk_any(int hip_device, const float* scores, int64_t lds, const int64_t* idx, int64_t ldi, int64_t nq,
                 int64_t C, int k, int64_t base, float* out_scores, int64_t* out_idx, void* stream) {
  if (k < 1 || k > (1 << 26) || nq < 0 || nq > 65535 || C < 0 || C > 0xFFFFFFFFll || lds < C || (idx && ldi < C))
    return fail(CLM_E_ARG, "bad topk_any shape (1 <= k <= 2^26, nq <= 65535, C <= 2^32 - 1, C <= lds, ldi)");
  if (nq == 0) return CLM_OK;
  if (!is_device_ptr(scores) || (idx && !is_device_ptr(idx)) || !is_device_ptr(out_scores) || !is_device_ptr(out_idx))
    return fail(CLM_E_ARG, "topk_any: device pointers");
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  if (int rg = scratch_grow(scr, topk_any_ws_bytes(nq, k))) return rg;
  KCHK(topk_any(scores, lds, idx, ldi, nq, C, k, base, out_scores, out_idx, k, scr.p, st));
  HIPCHK(hipStreamSynchronize(st));   // the scratch is reused by the next call
  scratch_trim(scr);
  return CLM_OK;
}

int clm_topk_merge(int hip_device, const float* scores, const int64_t* idx, int64_t nq, int parts, int k_in, int k,
                   float* out_scores, int64_t* out_idx, void* stream) {
  if (nq < 0 || parts <= 0 || k_in <= 0 || k <= 0 || (int64_t)parts * k_in > 0x7FFFFFFF)
    return fail(CLM_E_ARG, "bad merge shape");
  if (nq == 0) return CLM_OK;
  // one LDS sort per row (topk_merge) up to 8192 candidates and k <= 1024; beyond, topk_any
  const bool any = k > 1024 || (int64_t)parts * k_in > 8192;
  const int64_t any_rows = std::min<int64_t>(nq, 65535);
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  const bool in_d = is_device_ptr(scores) && is_device_ptr(idx);
  const bool out_d = is_device_ptr(out_scores) && is_device_ptr(out_idx);
  const size_t n_in = (size_t)nq * parts * k_in;
  uint8_t* w = nullptr;
  // the offsets and the size from the same Layout (a size computed apart once under-allocated 4
  // small buffers -- found by the host-sanitizer harness)
  Layout lay;
  const size_t o_si = in_d ? 0 : lay.take(n_in * 4), o_ii = in_d ? 0 : lay.take(n_in * 8),
               o_so = out_d ? 0 : lay.take((size_t)nq * k * 4), o_io = out_d ? 0 : lay.take((size_t)nq * k * 8),
               o_aws = any ? lay.take(topk_any_ws_bytes(any_rows, k)) : 0, o_mx = any ? lay.take(8) : 0;
  const size_t bytes = lay.total();
  Scratch& scr = scratch_of_current_device();
  std::unique_lock<std::mutex> lock(scr.mu, std::defer_lock);
  if (bytes > 0) {   // host lists: staged through the device scratch (the call drains its stream)
    lock.lock();
    if (int rg = scratch_grow(scr, bytes)) return rg;
    w = (uint8_t*)scr.p;
  }
  const float* s_in = scores;
  const int64_t* i_in = idx;
  float* s_out = out_d ? out_scores : (float*)(w + o_so);
  int64_t* i_out = out_d ? out_idx : (int64_t*)(w + o_io);
  hipError_t e = hipSuccess;
  if (!in_d) {
    float* a = (float*)(w + o_si);
    int64_t* b = (int64_t*)(w + o_ii);
    e = hipMemcpyAsync(a, scores, n_in * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b, idx, n_in * 8, hipMemcpyHostToDevice, st);
    s_in = a; i_in = b;
  }
  if (!any) {
    if (e == hipSuccess) e = topk_merge(s_in, i_in, nq, parts, k_in, k, s_out, i_out, st);
  } else {
    void* aws = w + o_aws;
    const int64_t n_row = (int64_t)parts * k_in;
    // past one LDS sort the selection keys hold the low 32 bits of an index: larger ones are refused
    int64_t* mx = (int64_t*)(w + o_mx);
    int64_t hmx = 0;
    if (e == hipSuccess) e = max_index(i_in, (int64_t)n_in, mx, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&hmx, mx, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && hmx > (int64_t)0xFFFFFFFF) {
      scratch_trim(scr);
      return fail(CLM_E_ARG, "topk_merge: more than 8192 candidates per query or k > 1024 needs indices below 2^32");
    }
    for (int64_t q0 = 0; e == hipSuccess && q0 < nq; q0 += any_rows)
      e = topk_any(s_in + q0 * n_row, n_row, i_in + q0 * n_row, n_row, std::min(any_rows, nq - q0), n_row, k, 0,
                   s_out + q0 * k, i_out + q0 * k, k, aws, st);
  }
  if (e == hipSuccess && !out_d) {
    e = hipMemcpyAsync(out_scores, s_out, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out_idx, i_out, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess && bytes > 0) e = hipStreamSynchronize(st);   // the scratch is free again
  if (bytes > 0) scratch_trim(scr);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("topk_merge: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_topk_distinct(int hip_device, const float* scores, const int64_t* idx, const int64_t* gid,
                      const int64_t* offsets, int64_t ld, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                      int64_t* out_gid, int32_t* out_found, void* stream) {
  if (nq < 0 || ld < 0 || k < 1 || k > 1024) return fail(CLM_E_ARG, "bad topk_distinct shape (nq, ld >= 0, 1 <= k <= 1024)");
  if (nq == 0) return CLM_OK;
  const bool reads = offsets || ld > 0;   // fixed-width lists of no entries read nothing
  if (!out_scores || !out_idx || !out_gid || !out_found) return fail(CLM_E_ARG, "topk_distinct: a null output");
  if (reads && (!scores || !idx || !gid)) return fail(CLM_E_ARG, "topk_distinct: a null list");
  if (!is_device_ptr(out_scores) || !is_device_ptr(out_idx) || !is_device_ptr(out_gid) || !is_device_ptr(out_found) ||
      (offsets && !is_device_ptr(offsets)) ||
      (reads && (!is_device_ptr(scores) || !is_device_ptr(idx) || !is_device_ptr(gid))))
    return fail(CLM_E_ARG, "topk_distinct: device pointers");
  DeviceGuard g(hip_device);
  KCHK(topk_distinct(scores, idx, gid, offsets, ld, nq, k, out_scores, out_idx, out_gid, out_found,
                     (hipStream_t)stream));
  return CLM_OK;
}

int clm_l2_normalize(int hip_device, float* rows, int64_t n, int dim, void* stream) {
  if (n < 0 || dim <= 0 || (n > 0 && !rows)) return fail(CLM_E_ARG, "bad argument");
  if (n == 0) return CLM_OK;
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  if (is_device_ptr(rows)) {
    KCHK(l2_normalize_rows(rows, n, dim, st));
    return CLM_OK;
  }
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  if (int rg = scratch_grow(scr, (size_t)n * dim * 4)) return rg;
  float* t = (float*)scr.p;
  hipError_t e = hipMemcpyAsync(t, rows, (size_t)n * dim * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = l2_normalize_rows(t, n, dim, st);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, t, (size_t)n * dim * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  scratch_trim(scr);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("l2_normalize: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_fuse_queries(int hip_device, const float* a, float w_a, const float* b, float w_b, int64_t n,
                     int dim, float* out, void* stream) {
  if (n < 0 || dim <= 0 || (n > 0 && (!a || !out))) return fail(CLM_E_ARG, "bad argument");
  if (n == 0) return CLM_OK;
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  const bool dev = is_device_ptr(a);
  if (dev != is_device_ptr(out) || (b && dev != is_device_ptr(b)))
    return fail(CLM_E_ARG, "fuse_queries: a, b and out must all be device or all host pointers");
  if (dev) {
    KCHK(fuse_rows(a, w_a, b, w_b, n, dim, out, st));
    return CLM_OK;
  }
  const size_t bytes = (size_t)n * dim * 4;
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  if (int rg = scratch_grow(scr, bytes * (b ? 2 : 1))) return rg;
  float* t = (float*)scr.p;
  float* tb = b ? t + (size_t)n * dim : nullptr;
  hipError_t e = hipMemcpyAsync(t, a, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && b) e = hipMemcpyAsync(tb, b, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = fuse_rows(t, w_a, tb, w_b, n, dim, t, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out, t, bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  scratch_trim(scr);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("fuse_queries: ") + hipGetErrorString(e));
  return CLM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- images ----
// Tap tables of PIL's 8-bit resampler (Pillow 12.2.0 src/libImaging/Resample.c precompute_coeffs +
// normalize_coeffs_8bpc, BICUBIC a = -0.5, support 2), the resize CLIPImageProcessor runs
// (models/clip_model.py:108-110); restated with the same double arithmetic and operation order as
// oracle/image_ref.py:coeffs. Contraction is off so no FMA can change a weight's last bit.
namespace {
#pragma clang fp contract(off)
double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// taps of output coordinates [first, first + count) of an in_size -> out_size resample:
// mins / ns [count] and fixed-point weights [count][ksize]; returns ksize
int pil_coeffs(int in_size, int out_size, int first, int count, std::vector<int32_t>& mins,
               std::vector<int32_t>& ns, std::vector<int32_t>& ks) {
  const double scale = (double)(float)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  mins.assign(count, 0);
  ns.assign(count, 0);
  ks.assign((size_t)count * ksize, 0);
  std::vector<double> w(ksize);
  for (int i = 0; i < count; ++i) {
    const int xx = first + i;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = pil_bicubic((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    for (int x = 0; x < xmax; ++x) {
      const double k = ww != 0.0 ? w[x] / ww : w[x];
      ks[(size_t)i * ksize + x] = k < 0 ? (int32_t)(-0.5 + k * (1 << 22)) : (int32_t)(0.5 + k * (1 << 22));
    }
    mins[i] = xmin;
    ns[i] = xmax;
  }
  return ksize;
}
#pragma clang fp contract(on)

}  // namespace

extern "C" int clm_resize_crop(int hip_device, const uint8_t* src, const int64_t* offs, const int32_t* hw,
                               int n, int S, uint8_t* out, void* stream) {
  if (n < 0 || S <= 0 || S > 4096 || (n > 0 && (!src || !offs || !hw || !out)))
    return fail(CLM_E_ARG, "resize_crop: bad argument");
  if (n == 0) return CLM_OK;
  std::vector<ResizeDesc> desc(n);
  std::vector<int32_t> coef;
  int64_t src_bytes = 0, tmp_bytes = 0;
  int max_rows = 0;
  std::vector<int32_t> xmin, xn, xk, ymin, yn, yk;
  for (int i = 0; i < n; ++i) {
    const int H = hw[2 * i], W = hw[2 * i + 1];
    if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 28) || offs[i] < 0)
      return fail(CLM_E_ARG, "resize_crop: image " + std::to_string(i) + " has a bad size or offset");
    src_bytes = std::max(src_bytes, offs[i] + (int64_t)H * W * 3);
    // get_resize_output_image_size(default_to_square=False): short -> S, long -> int(S * long / short)
    const int shrt = std::min(H, W), lng = std::max(H, W);
    // int(S * long / short) in double as transformers does; an extreme aspect ratio (a 1 x 10^7
    // strip) would overflow int -- undefined behaviour, PIL fails on it too: refuse
    const double nl = (double)((int64_t)S * lng) / shrt;
    if (!(nl < (double)(1 << 24)))
      return fail(CLM_E_ARG, "resize_crop: image " + std::to_string(i) + " resizes to a side over 2^24 pixels");
    const int new_long = (int)nl;
    const int nh = W <= H ? new_long : S, nw = W <= H ? S : new_long;
    const int top = (nh - S) / 2, left = (nw - S) / 2;   // center_crop; nh, nw >= S
    ResizeDesc& d = desc[i];
    d.src_off = offs[i];
    d.W = W;
    d.kh = pil_coeffs(W, nw, left, S, xmin, xn, xk);
    d.kv = pil_coeffs(H, nh, top, S, ymin, yn, yk);
    int r1 = 0;
    for (int y = 0; y < S; ++y) r1 = std::max(r1, ymin[y] + yn[y]);
    d.r0 = ymin[0];
    d.rows = r1 - d.r0;
    for (int y = 0; y < S; ++y) ymin[y] -= d.r0;
    d.tmp_off = tmp_bytes;
    tmp_bytes += round_up((int64_t)d.rows * S * 3, 256);
    max_rows = std::max(max_rows, d.rows);
    d.coef_off = (int32_t)coef.size();
    if ((int64_t)coef.size() + 4 * S + (int64_t)S * (d.kh + d.kv) > INT32_MAX)
      return fail(CLM_E_ARG, "resize_crop: tap tables too large");
    coef.insert(coef.end(), xmin.begin(), xmin.end());
    coef.insert(coef.end(), xn.begin(), xn.end());
    coef.insert(coef.end(), ymin.begin(), ymin.end());
    coef.insert(coef.end(), yn.begin(), yn.end());
    coef.insert(coef.end(), xk.begin(), xk.end());
    coef.insert(coef.end(), yk.begin(), yk.end());
  }
  DeviceGuard g(hip_device);
  hipStream_t st = (hipStream_t)stream;
  const bool sd = is_device_ptr(src), od = is_device_ptr(out);
  const size_t out_bytes = (size_t)n * S * S * 3;
  Layout lay;
  const size_t o_desc = lay.take(sizeof(ResizeDesc) * n), o_coef = lay.take(coef.size() * 4),
               o_tmp = lay.take((size_t)tmp_bytes), o_src = sd ? 0 : lay.take((size_t)src_bytes),
               o_out = od ? 0 : lay.take(out_bytes);
  Scratch& scr = scratch_of_current_device();
  std::lock_guard<std::mutex> lock(scr.mu);
  if (int rg = scratch_grow(scr, lay.total())) return rg;
  uint8_t* w = (uint8_t*)scr.p;
  ResizeDesc* d_desc = (ResizeDesc*)(w + o_desc);
  int32_t* d_coef = (int32_t*)(w + o_coef);
  uint8_t* d_tmp = w + o_tmp;
  const uint8_t* d_src = src;
  uint8_t* d_out = od ? out : w + o_out;
  hipError_t e = hipMemcpyAsync(d_desc, desc.data(), sizeof(ResizeDesc) * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !sd) {
    uint8_t* t = w + o_src;
    e = hipMemcpyAsync(t, src, (size_t)src_bytes, hipMemcpyHostToDevice, st);
    d_src = t;
  }
  if (e == hipSuccess) e = resize_crop(d_src, d_desc, n, S, max_rows, d_coef, d_tmp, d_out, st);
  if (e == hipSuccess && !od) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
  // the tables live in host vectors and the workspace is freed below: wait for the stream
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  scratch_trim(scr);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("resize_crop: ") + hipGetErrorString(e));
  return CLM_OK;
}

extern "C" int clm_synth_images(int hip_device, uint64_t seed, int64_t row0, int n, int S, uint8_t* out,
                                void* stream) {
  if (n < 0 || S <= 0 || row0 < 0 || ((int64_t)S * S * 3) % 16 || (n > 0 && !out))
    return fail(CLM_E_ARG, "synth_images: bad argument (S * S * 3 must be a multiple of 16)");
  if (n == 0) return CLM_OK;
  if (!is_device_ptr(out) || ((uintptr_t)out & 15)) return fail(CLM_E_ARG, "synth_images: out must be 16-B aligned device memory");
  DeviceGuard g(hip_device);
  KCHK(synth_images(seed, row0, n, S, out, (hipStream_t)stream));
  return CLM_OK;
}
