// libclm C-ABI (include/clm.h): context, weight packing, encode drivers, kernel test hooks. (The
// HBM index: capi_index.cpp, searching it: capi_search.cpp, stand-alone ops + images: capi_ops.cpp.)
//
// Host runtime behind the reference's Python API:
//   load_clip_model            models/clip_model.py:37-82     -> clm_ctx_create/_load_tensor/_finalize
//   PEFT LoRA (r, alpha/r)     models/lora_adapter.py:21-43    -> merged or K-extension packing
//   encode_image/encode_text   models/clip_model.py:89-150     -> clm_encode_image/_text
//   TextSearchIndex            src/embedding/search.py:24-115  -> clm_index_*
// Weights arrive by transformers / PEFT state-dict name; finalize() fuses q/k/v
// into one [3d, K] matrix (q rows pre-scaled by 64^-1/2), folds LoRA either into
// the weights (W + (alpha/r) B A, fp32 then cast) or as K-extension columns
// [W | (alpha/r) B] against activations [X | X A^T], and uploads everything in
// the compute dtype (bf16/fp16), keeping LayerNorm, biases, embeddings and the
// projections in fp32.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "capi_internal.hpp"

using namespace clm;
using namespace clm::capi;

namespace {
thread_local std::string g_err;   // clm_last_error: what any unit's fail() wrote on this thread
}  // namespace

int clm::capi::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

bool clm::capi::is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

int clm::capi::grow(void** p, size_t* cap, size_t bytes, const char* what) {
  if (*cap >= bytes) return CLM_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return fail(CLM_E_OOM, std::string(what) + " allocation failed");
  }
  *cap = bytes;
  return CLM_OK;
}

namespace {

// clm_debug_set / $CLM_GEMM_DEBUG: GemmArgs::debug of clm_gemm (micro-benchmarks only)
int g_gemm_debug = getenv("CLM_GEMM_DEBUG") ? atoi(getenv("CLM_GEMM_DEBUG")) : 0;

uint16_t host_f32_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
uint16_t host_f32_to_f16(float f) {
  _Float16 h = (_Float16)f;
  uint16_t r;
  std::memcpy(&r, &h, 2);
  return r;
}
float host_bf16_to_f32(uint16_t v) {
  uint32_t u = (uint32_t)v << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

struct LayerW {
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  // k_*: the weight's row stride and the K of GEMMs that need whole 64-wide K-steps (G2, split-K);
  // kl_*: the logical K, in + round_up(r, 32) in unmerged-LoRA mode (gemm_kernel and the fused
  // attention run the 32-wide last K-step), = k_* otherwise
  u16* w_qkv = nullptr; float* b_qkv = nullptr; int k_qkv = 0, kl_qkv = 0;
  u16* w_out = nullptr; float* b_out = nullptr; int k_out = 0, kl_out = 0;
  u16* w_fc1 = nullptr; float* b_fc1 = nullptr; int k_fc1 = 0, kl_fc1 = 0;
  u16* w_fc2 = nullptr; float* b_fc2 = nullptr; int k_fc2 = 0, kl_fc2 = 0;
  // unmerged LoRA: the stacked A of each GEMM input in the compute dtype, [RPAD, in] with zero rows
  // past r_* (the down-projection GEMM writes all RPAD extension columns: the pad ones get zeros)
  u16* a_qkv = nullptr; int r_qkv = 0;
  u16* a_out = nullptr; int r_out = 0;
  u16* a_fc1 = nullptr; int r_fc1 = 0;
  u16* a_fc2 = nullptr; int r_fc2 = 0;
};

struct Tower {
  bool vision = false;
  bool q_log2e = false;   // q_proj weights carry log2(e) (attention_folds_log2e)
  int d = 0, L = 0, H = 0, mlp = 0;
  std::vector<LayerW> layers;
  float *projT = nullptr, *fin_g = nullptr, *fin_b = nullptr;
  // vision
  u16* patch_w = nullptr; int kp = 0;
  float *cls = nullptr, *pos = nullptr, *pre_g = nullptr, *pre_b = nullptr, *lut = nullptr;
  // text
  float *tok = nullptr, *tpos = nullptr;
  // workspace
  int64_t maxM = 0;
  float* h = nullptr;
  u16 *X = nullptr, *QKV = nullptr, *O = nullptr, *Hm = nullptr, *P = nullptr;
  float* pooled = nullptr;  // [max_batch, proj_dim] un-normalised projections
  float* hc = nullptr;      // [max_batch, d] pooled residual rows of the pruned last layer
  u16* Oc = nullptr;        // [max_batch, ldo] their attention-output rows
  // varlen text plan (text_plan): per caption live rows / offsets, packed-row map, fused-attention
  // tiles, {live rows, tiles}; a sub-batch view at b0 uses lens / tiles + b0, offs / counts + 2 b0
  int *vl_lens = nullptr, *vl_offs = nullptr, *vl_rowmap = nullptr, *vl_tiles = nullptr, *vl_counts = nullptr;
  int64_t ldx = 0, ldo = 0, ldm = 0;
};

// K-extension width of the unmerged LoRA mode: the storage (weight columns, activation columns;
// rows stay whole 64-wide K-steps), of which GEMMs multiply round_up(sum r, 32) (LORA_GRANULE)
constexpr int RPAD = 64;
constexpr int LORA_GRANULE = 32;

}  // namespace

struct clm_ctx {
  int dev = 0;
  clm_model_desc desc{};
  bool finalized = false;
  bool lora_enabled = true;
  std::unordered_map<std::string, HostTensor> host;
  std::vector<void*> allocs;       // weights + workspace
  Tower vis, txt;
  // host<->device staging
  void* stage_in = nullptr; size_t stage_in_bytes = 0;
  void* stage_out = nullptr; size_t stage_out_bytes = 0;
  int32_t* ids_dev = nullptr;
  // two-tower concurrency + graph replay (clm_encode_pair)
  // Each tower's batch is cut into `split` sub-batches on their own streams (disjoint row
  // ranges of the tower workspace): one sub-batch's write-bound GEMM epilogues and
  // latency-bound LN/attention launches overlap another's MFMA main loops.
  static constexpr int MAX_SPLIT = 4;
  hipStream_t ps[2 * MAX_SPLIT] = {};
  hipEvent_t pev[2 * MAX_SPLIT] = {};
  hipEvent_t ev_fork = nullptr, ev_done = nullptr;
  typedef std::tuple<const void*, int, int, const void*, int, int, void*, void*, int, int, int> PairKey;
  std::map<PairKey, hipGraphExec_t> graphs;
  int last_pair_path = -1;   // clm_pair_path: 0 = two tower streams (-1: no encode_pair yet)
  // kernel timing (clm_prof_*): events recorded on the launch stream
  bool prof = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Rec { int cat; double work; size_t e0, e1; };
  std::vector<Rec> recs;

  // operand type of a tower's GEMMs / attention (CLM_COMPUTE_MIXED: bf16 vision, fp16 text)
  bool bf16(bool vision) const {
    return desc.compute_dtype == CLM_BF16 || (vision && desc.compute_dtype == CLM_COMPUTE_MIXED);
  }

  template <typename T>
  int dalloc(T** p, size_t count) {
    void* q = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLM_E_OOM, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes failed");
    }
    allocs.push_back(q);
    *p = (T*)q;
    return CLM_OK;
  }
  void drop_graphs() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
  }
  void free_all() {
    drop_graphs();
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    if (stage_in) (void)hipFree(stage_in);
    if (stage_out) (void)hipFree(stage_out);
    stage_in = stage_out = nullptr;
    stage_in_bytes = stage_out_bytes = 0;
    vis = Tower();
    txt = Tower();
    ids_dev = nullptr;
  }
};

namespace {

const HostTensor* find(const clm_ctx* c, const std::string& n) {
  auto it = c->host.find(n);
  return it == c->host.end() ? nullptr : &it->second;
}

int need(const clm_ctx* c, const std::string& n, int64_t numel, const HostTensor** out) {
  const HostTensor* t = find(c, n);
  if (!t) return fail(CLM_E_MISSING, "missing tensor '" + n + "'");
  if ((int64_t)t->data.size() != numel)
    return fail(CLM_E_ARG, "tensor '" + n + "' has " + std::to_string(t->data.size()) + " elements, expected " +
                               std::to_string(numel));
  *out = t;
  return CLM_OK;
}

int upload_f32(clm_ctx* c, const std::vector<float>& v, float** dst) {
  int r = c->dalloc(dst, v.size());
  if (r) return r;
  HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return CLM_OK;
}

int upload_16(clm_ctx* c, const std::vector<float>& v, u16** dst, bool bf) {
  std::vector<u16> h(v.size());
  if (bf)
    for (size_t i = 0; i < v.size(); ++i) h[i] = host_f32_to_bf16(v[i]);
  else
    for (size_t i = 0; i < v.size(); ++i) h[i] = host_f32_to_f16(v[i]);
  int r = c->dalloc(dst, h.size());
  if (r) return r;
  HIPCHK(hipMemcpy(*dst, h.data(), h.size() * sizeof(u16), hipMemcpyHostToDevice));
  return CLM_OK;
}

// the stacked LoRA A [r_ext, in] (fp32 host) as the [RPAD, in] 16-bit W operand of the
// down-projection GEMM, rows r_ext .. RPAD-1 zero
int upload_lora_a(clm_ctx* c, const std::vector<float>& A, int r_ext, int in, u16** dst, bool bf) {
  std::vector<float> pad((size_t)RPAD * in, 0.f);
  std::copy(A.begin(), A.begin() + (size_t)r_ext * in, pad.begin());
  return upload_16(c, pad, dst, bf);
}

int get_f32(clm_ctx* c, const std::string& n, int64_t numel, float** dst) {
  const HostTensor* t;
  int r = need(c, n, numel, &t);
  if (r) return r;
  return upload_f32(c, t->data, dst);
}

// A linear's weight block for a (possibly fused) GEMM: rows [row0, row0+out) of W,
// its LoRA pair (if targeted and enabled), and the extension offset for unmerged mode.
struct LinearSpec {
  std::string path;
  int in, out;
  bool lora;
};

// Build a fused [sum(out), K] weight (fp32 host) for linears sharing one input.
// merged: W += s * B A.  unmerged: K = in + RPAD, columns [in + off, in + off + r) = s * B.
// Also returns the stacked A [r_ext, in] for the unmerged mode.
int build_fused(clm_ctx* c, const std::vector<LinearSpec>& specs, float q_scale, std::vector<float>& W,
                std::vector<float>& bias, int& K, std::vector<float>& A_stack, int& r_ext, int& K_log) {
  const clm_model_desc& d = c->desc;
  const bool unmerged = d.lora_mode == CLM_LORA_UNMERGED;
  const int in = specs[0].in;
  int total_out = 0;
  r_ext = 0;
  for (auto& s : specs) {
    total_out += s.out;
    if (s.lora) r_ext += d.lora_r;
  }
  K = (unmerged && r_ext > 0) ? in + RPAD : in;
  K_log = (unmerged && r_ext > 0) ? in + (r_ext + LORA_GRANULE - 1) / LORA_GRANULE * LORA_GRANULE : in;
  if (r_ext > RPAD) return fail(CLM_E_ARG, "LoRA rank too large for the K-extension (sum r > 64)");
  W.assign((size_t)total_out * K, 0.f);
  bias.assign(total_out, 0.f);
  A_stack.assign((size_t)r_ext * in, 0.f);
  const float scaling = d.lora_r > 0 ? d.lora_alpha / (float)d.lora_r : 0.f;
  int row0 = 0, roff = 0;
  for (size_t si = 0; si < specs.size(); ++si) {
    const LinearSpec& s = specs[si];
    const HostTensor *w, *b;
    int r = need(c, s.path + ".weight", (int64_t)s.out * s.in, &w);
    if (r) return r;
    r = need(c, s.path + ".bias", s.out, &b);
    if (r) return r;
    const float qs = si == 0 ? q_scale : 1.0f;   // the first linear's scale (q_proj: see build_tower)
    for (int o = 0; o < s.out; ++o) {
      std::memcpy(&W[(size_t)(row0 + o) * K], &w->data[(size_t)o * s.in], s.in * sizeof(float));
      bias[row0 + o] = b->data[o];
    }
    if (s.lora) {
      const HostTensor *A, *B;
      const std::string base = "base_model.model." + s.path;
      r = need(c, base + ".lora_A.weight", (int64_t)d.lora_r * s.in, &A);
      if (r) return r;
      r = need(c, base + ".lora_B.weight", (int64_t)s.out * d.lora_r, &B);
      if (r) return r;
      if (!unmerged) {
        for (int o = 0; o < s.out; ++o) {
          float* wr = &W[(size_t)(row0 + o) * K];
          for (int j = 0; j < d.lora_r; ++j) {
            const float bj = scaling * B->data[(size_t)o * d.lora_r + j];
            const float* ar = &A->data[(size_t)j * s.in];
            for (int i = 0; i < s.in; ++i) wr[i] += bj * ar[i];
          }
        }
      } else {
        for (int o = 0; o < s.out; ++o)
          for (int j = 0; j < d.lora_r; ++j)
            W[(size_t)(row0 + o) * K + s.in + roff + j] = scaling * B->data[(size_t)o * d.lora_r + j];
        std::memcpy(&A_stack[(size_t)roff * in], A->data.data(), (size_t)d.lora_r * in * sizeof(float));
      }
      roff += d.lora_r;
    }
    if (qs != 1.0f) {
      for (int o = 0; o < s.out; ++o) {
        float* wr = &W[(size_t)(row0 + o) * K];
        for (int i = 0; i < K; ++i) wr[i] *= qs;
        bias[row0 + o] *= qs;
      }
    }
    row0 += s.out;
  }
  if (!unmerged) r_ext = 0;
  return CLM_OK;
}

int build_tower(clm_ctx* c, Tower& T, bool vision) {
  const clm_model_desc& d = c->desc;
  const clm_tower_desc& td = vision ? d.vision : d.text;
  T.vision = vision;
  T.d = td.hidden; T.L = td.layers; T.H = td.heads; T.mlp = td.mlp;
  if (T.d != T.H * 64) return fail(CLM_E_ARG, "head_dim must be 64");
  if (T.d % 128 || T.d > 1024 || T.mlp % 64) return fail(CLM_E_ARG, "hidden must be a multiple of 128 (<=1024), mlp of 64");
  const std::string pre = vision ? "vision_model" : "text_model";
  const bool lora_on = c->lora_enabled && d.lora_r > 0;
  const uint32_t tg = lora_on ? d.lora_targets : 0u;
  const bool unmerged = d.lora_mode == CLM_LORA_UNMERGED;
  // q_proj carries the 64^-1/2 score scale (head_dim 64: a power of two, bit-identical to scaling
  // the scores), and log2(e) too where the tower's attention kernel takes its scores in the log2
  // domain (attention_folds_log2e: the L/14 image tower's T = 577)
  const int Tseq = vision ? (d.image_size / d.patch) * (d.image_size / d.patch) + 1 : 0;
  T.q_log2e = vision && attention_folds_log2e(c->bf16(true), false, Tseq);
  const float qscale = T.q_log2e ? 0.125f * 1.4426950408889634f : 0.125f;
  int r;
  T.layers.resize(T.L);
  for (int l = 0; l < T.L; ++l) {
    LayerW& Lw = T.layers[l];
    const std::string p = pre + ".encoder.layers." + std::to_string(l);
    if ((r = get_f32(c, p + ".layer_norm1.weight", T.d, &Lw.ln1_g))) return r;
    if ((r = get_f32(c, p + ".layer_norm1.bias", T.d, &Lw.ln1_b))) return r;
    if ((r = get_f32(c, p + ".layer_norm2.weight", T.d, &Lw.ln2_g))) return r;
    if ((r = get_f32(c, p + ".layer_norm2.bias", T.d, &Lw.ln2_b))) return r;
    std::vector<float> W, b, A;
    int K, rext, KL;
    // q, k, v share the LN1 output: one fused GEMM
    std::vector<LinearSpec> qkv = {{p + ".self_attn.q_proj", T.d, T.d, (tg & CLM_LORA_Q) != 0},
                                   {p + ".self_attn.k_proj", T.d, T.d, (tg & CLM_LORA_K) != 0},
                                   {p + ".self_attn.v_proj", T.d, T.d, (tg & CLM_LORA_V) != 0}};
    if ((r = build_fused(c, qkv, qscale, W, b, K, A, rext, KL))) return r;
    if ((r = upload_16(c, W, &Lw.w_qkv, c->bf16(vision))) || (r = upload_f32(c, b, &Lw.b_qkv))) return r;
    Lw.k_qkv = K; Lw.kl_qkv = KL; Lw.r_qkv = rext;
    if (unmerged && rext && (r = upload_lora_a(c, A, rext, T.d, &Lw.a_qkv, c->bf16(vision)))) return r;

    std::vector<LinearSpec> outp = {{p + ".self_attn.out_proj", T.d, T.d, (tg & CLM_LORA_OUT) != 0}};
    if ((r = build_fused(c, outp, 1.0f, W, b, K, A, rext, KL))) return r;
    if ((r = upload_16(c, W, &Lw.w_out, c->bf16(vision))) || (r = upload_f32(c, b, &Lw.b_out))) return r;
    Lw.k_out = K; Lw.kl_out = KL; Lw.r_out = rext;
    if (unmerged && rext && (r = upload_lora_a(c, A, rext, T.d, &Lw.a_out, c->bf16(vision)))) return r;

    std::vector<LinearSpec> fc1 = {{p + ".mlp.fc1", T.d, T.mlp, (tg & CLM_LORA_FC1) != 0}};
    if ((r = build_fused(c, fc1, 1.0f, W, b, K, A, rext, KL))) return r;
    if ((r = upload_16(c, W, &Lw.w_fc1, c->bf16(vision))) || (r = upload_f32(c, b, &Lw.b_fc1))) return r;
    Lw.k_fc1 = K; Lw.kl_fc1 = KL; Lw.r_fc1 = rext;
    if (unmerged && rext && (r = upload_lora_a(c, A, rext, T.d, &Lw.a_fc1, c->bf16(vision)))) return r;

    std::vector<LinearSpec> fc2 = {{p + ".mlp.fc2", T.mlp, T.d, (tg & CLM_LORA_FC2) != 0}};
    if ((r = build_fused(c, fc2, 1.0f, W, b, K, A, rext, KL))) return r;
    if ((r = upload_16(c, W, &Lw.w_fc2, c->bf16(vision))) || (r = upload_f32(c, b, &Lw.b_fc2))) return r;
    Lw.k_fc2 = K; Lw.kl_fc2 = KL; Lw.r_fc2 = rext;
    if (unmerged && rext && (r = upload_lora_a(c, A, rext, T.mlp, &Lw.a_fc2, c->bf16(vision)))) return r;
  }
  // projection, transposed to [d, D] for coalesced reads in pool_project
  {
    const HostTensor* pw;
    const std::string pn = vision ? "visual_projection.weight" : "text_projection.weight";
    if ((r = need(c, pn, (int64_t)d.proj_dim * T.d, &pw))) return r;
    std::vector<float> pt((size_t)T.d * d.proj_dim);
    for (int j = 0; j < d.proj_dim; ++j)
      for (int i = 0; i < T.d; ++i) pt[(size_t)i * d.proj_dim + j] = pw->data[(size_t)j * T.d + i];
    if ((r = upload_f32(c, pt, &T.projT))) return r;
  }
  const int64_t B = d.max_batch;
  if (vision) {
    const int G = d.image_size / d.patch, Tn = G * G + 1;
    if ((r = get_f32(c, pre + ".post_layernorm.weight", T.d, &T.fin_g))) return r;
    if ((r = get_f32(c, pre + ".post_layernorm.bias", T.d, &T.fin_b))) return r;
    if ((r = get_f32(c, pre + ".pre_layrnorm.weight", T.d, &T.pre_g))) return r;
    if ((r = get_f32(c, pre + ".pre_layrnorm.bias", T.d, &T.pre_b))) return r;
    if ((r = get_f32(c, pre + ".embeddings.class_embedding", T.d, &T.cls))) return r;
    if ((r = get_f32(c, pre + ".embeddings.position_embedding.weight", (int64_t)Tn * T.d, &T.pos))) return r;
    const int kreal = d.channels * d.patch * d.patch;
    T.kp = (int)round_up(kreal, 64);
    const HostTensor* pw;
    if ((r = need(c, pre + ".embeddings.patch_embedding.weight", (int64_t)T.d * kreal, &pw))) return r;
    std::vector<float> wp((size_t)T.d * T.kp, 0.f);
    for (int o = 0; o < T.d; ++o) std::memcpy(&wp[(size_t)o * T.kp], &pw->data[(size_t)o * kreal], kreal * 4);
    if ((r = upload_16(c, wp, &T.patch_w, c->bf16(true)))) return r;
    // CLIPImageProcessor rescale (float64 multiply -> float32) then (x - mean) / std in float32
    std::vector<float> lut((size_t)d.channels * 256);
    for (int ch = 0; ch < d.channels; ++ch)
      for (int u = 0; u < 256; ++u) {
        const float x = (float)((double)u * (1.0 / 255.0));
        lut[(size_t)ch * 256 + u] = (x - d.mean[ch % 3]) / d.std[ch % 3];
      }
    if ((r = upload_f32(c, lut, &T.lut))) return r;
    T.maxM = B * Tn;
    if ((r = c->dalloc(&T.P, (size_t)B * G * G * T.kp))) return r;
  } else {
    if ((r = get_f32(c, pre + ".final_layer_norm.weight", T.d, &T.fin_g))) return r;
    if ((r = get_f32(c, pre + ".final_layer_norm.bias", T.d, &T.fin_b))) return r;
    if ((r = get_f32(c, pre + ".embeddings.token_embedding.weight", (int64_t)d.vocab * T.d, &T.tok))) return r;
    if ((r = get_f32(c, pre + ".embeddings.position_embedding.weight", (int64_t)d.max_pos * T.d, &T.tpos))) return r;
    T.maxM = B * d.max_pos;
  }
  T.ldx = T.d + RPAD;
  T.ldo = T.d + RPAD;
  T.ldm = T.mlp + RPAD;
  if ((r = c->dalloc(&T.h, (size_t)T.maxM * T.d))) return r;
  if ((r = c->dalloc(&T.X, (size_t)T.maxM * T.ldx))) return r;
  if ((r = c->dalloc(&T.QKV, (size_t)T.maxM * 3 * T.d))) return r;
  if ((r = c->dalloc(&T.O, (size_t)T.maxM * T.ldo))) return r;
  if ((r = c->dalloc(&T.Hm, (size_t)T.maxM * T.ldm))) return r;
  if ((r = c->dalloc(&T.pooled, (size_t)B * d.proj_dim))) return r;
  if ((r = c->dalloc(&T.hc, (size_t)B * T.d))) return r;
  if ((r = c->dalloc(&T.Oc, (size_t)B * T.ldo))) return r;
  if (!T.vision) {
    if ((r = c->dalloc(&T.vl_lens, (size_t)B))) return r;
    if ((r = c->dalloc(&T.vl_offs, (size_t)2 * B + 1))) return r;
    if ((r = c->dalloc(&T.vl_rowmap, (size_t)T.maxM))) return r;
    if ((r = c->dalloc(&T.vl_tiles, (size_t)B))) return r;
    if ((r = c->dalloc(&T.vl_counts, (size_t)2 * B))) return r;
  }
  return CLM_OK;
}

// time one launch when profiling is on: returns the event-pair slot or -1
struct ProfScope {
  clm_ctx* c; hipStream_t st; int cat; double work; size_t e0 = 0; bool on = false;
  ProfScope(clm_ctx* c_, hipStream_t st_, int cat_, double work_) : c(c_), st(st_), cat(cat_), work(work_) {
    if (!c->prof) return;
    if (c->ev_used + 2 > c->ev_pool.size()) {
      for (int i = 0; i < 256; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return; }
        c->ev_pool.push_back(e);
      }
    }
    e0 = c->ev_used;
    c->ev_used += 2;
    on = hipEventRecord(c->ev_pool[e0], st) == hipSuccess;
  }
  ~ProfScope() {
    if (!on) return;
    if (hipEventRecord(c->ev_pool[e0 + 1], st) == hipSuccess) c->recs.push_back({cat, work, e0, e0 + 1});
  }
};
#define PROF(cat, work) ProfScope prof_scope_##__LINE__(c, st, cat, work)

// LN into X for a layer's q/k/v (or fc1) GEMM input
LnArgs ln_into_x(clm_ctx* c, Tower& T, int64_t M, const float* g, const float* b, float* h = nullptr) {
  LnArgs a{};
  if (!h) h = T.h;
  a.mode = 0; a.src = h; a.lds = T.d; a.hf = h; a.ldh = T.d;
  a.g1 = g; a.b1 = b; a.y = T.X; a.ldy = T.ldx;
  a.M = (int)M; a.d = T.d; a.eps = c->desc.ln_eps;
  return a;
}

// Unmerged LoRA, the down-projection of a GEMM input (PEFT lora_A, models/clip_model.py:78):
// X[:, K : K + RPAD) = X[:, :K] . A^T as a skinny MFMA GEMM (N = RPAD, 64 x 64 tiles, fp32
// accumulate, rounded once to the compute dtype), so the consumer GEMM's K-extension
// [X | X A^T] . [W | (alpha/r) B]^T adds the low-rank update in its own main loop. The input's
// rows are read once more (19.7 MB for the vision q/k/v input at batch 256, ~3 us); the round-4
// VALU form (24 wave reductions per row inside the LayerNorm / a row-per-wave kernel) cost
// 1.6 ms per pair step (profiles/r05_v2_unmerged_trace.txt).
hipError_t lora_down_gemm(bool bf, u16* X, int64_t ldx, int M, int K, const u16* A, const int* mdev,
                          hipStream_t st) {
  GemmArgs g{};
  g.A = X; g.lda = ldx; g.W = A; g.ldw = K; g.M = M; g.N = RPAD; g.K = K;
  g.out = X + K; g.ldo = ldx; g.m_dev = mdev;
  static const int cfg = getenv("CLM_LORA_DOWN_CFG") ? atoi(getenv("CLM_LORA_DOWN_CFG")) : GEMM_CFG_SKINNY;   // A/B
  return gemm_cfg(bf, EPI_STORE, cfg, g, st);
}

// Last-layer pruning (default; $CLM_NO_PRUNE=1 runs every row): the encoders return only the
// pooled row of each item (vision CLS row 0, text first-EOS row: TF/models/clip/
// modeling_clip.py:558-580, 650), and after the last layer's attention every op is row-wise
// (out_proj, LN2, fc1, fc2 + their LoRA). So the last layer runs q/k/v and attention on all
// B*S rows, then out_proj .. fc2 on the B pooled rows only (gathered into T.hc / T.Oc): the
// pooled embeddings are the same rows through the same kernels.
bool prune_last_layer() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("CLM_NO_PRUNE");
    v = (e && atoi(e)) ? 0 : 1;
  }
  return v == 1 && !(g_gemm_debug & 8);   // clm_debug_set bit 8: every row (tests)
}

// Varlen text (default; $CLM_TEXT_VARLEN=0 or clm_debug_set bit 32: every padded row): the text
// tower is causal and pools each caption's first-EOS row, so rows after it cannot reach the
// output. Only each caption's live rows (through its first EOS) are packed and encoded; the
// embeddings are bit-identical to encoding all L rows (rows are independent in every kernel but
// attention, whose keys of a live query are all live; tests/test_gpu_encode.py). Needs the fused
// attention kernel (unmerged LoRA included: its down-projection GEMMs read the live row count too).
bool text_varlen_enabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("CLM_TEXT_VARLEN");
    v = (e && !atoi(e)) ? 0 : 1;
  }
  return v == 1 && !(g_gemm_debug & 32);
}

// q/k/v projection + attention fused into one launch for T <= 128 (k_gemm_attn.hip) unless
// $CLM_FUSED_ATTN=0 or clm_debug_set bit 16 (tests: the two-kernel path, bit-identical)
bool fused_attention(int T, int H, int d, int K) {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("CLM_FUSED_ATTN");
    v = (e && !atoi(e)) ? 0 : 1;
  }
  return v == 1 && !(g_gemm_debug & 16) && gemm_attn_supported(T, H, d, K);
}

// Per-call state of one tower's encoder pass (run_layers).
struct LayerRun {
  Tower* T;
  int B, S;
  bool causal, vl, bf;
  const int32_t* ids;
  const int* mdev;            // varlen: device-resident live row count (T.vl_counts)
  double Mx, attn_pairs;      // executed rows / attention pairs (profiling)
};

int make_run(clm_ctx* c, Tower& T, int B, int S, bool causal, const int32_t* ids, bool vl, hipStream_t st,
             LayerRun* r) {
  *r = LayerRun{&T, B, S, causal, vl, c->bf16(T.vision), ids, vl ? T.vl_counts : nullptr, (double)B * S,
                (double)B * S * S};
  // varlen (packed live text rows): the row-wise kernels read the live row count from
  // T.vl_counts; the profiled pass (no graph, may sync) counts the executed rows and attention pairs
  if (vl && c->prof) {
    std::vector<int> lens(B);
    HIPCHK(hipMemcpyAsync(lens.data(), T.vl_lens, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r->Mx = r->attn_pairs = 0;
    for (int v : lens) { r->Mx += v; r->attn_pairs += (double)v * v; }
  }
  return CLM_OK;
}

double attn_flops(const LayerRun& R, int l) {
  const Tower& T = *R.T;
  return 2.0 * R.Mx * 3 * T.d * T.layers[l].kl_qkv + 4.0 * T.H * R.attn_pairs * 64;
}

// layer l's q/k/v projection + attention of one tower: T.X -> T.O
int attn_step(clm_ctx* c, const LayerRun& R, int l, hipStream_t st) {
  Tower& T = *R.T;
  LayerW& Lw = T.layers[l];
  const bool bf = R.bf;
  GemmArgs g{};
  g.A = T.X; g.lda = T.ldx; g.M = R.B * R.S; g.N = 3 * T.d; g.K = Lw.kl_qkv; g.out = T.QKV; g.ldo = 3 * T.d;
  g.W = Lw.w_qkv; g.ldw = Lw.k_qkv; g.bias = Lw.b_qkv;
  if (R.vl) {   // packed live rows of variable-length captions
    PROF(CLM_PROF_GEMM, attn_flops(R, l));
    KCHK(gemm_attn_varlen(bf, R.causal, g.A, g.lda, g.W, g.ldw, g.bias, T.O, T.ldo, R.B, R.S, T.H, T.d, g.K,
                          T.vl_lens, T.vl_offs, T.vl_tiles, T.vl_counts, st));
  } else if (fused_attention(R.S, T.H, T.d, g.K)) {
    // one launch: the q/k/v GEMM's tiles attend their own sequences (GEMM + attention FLOPs)
    PROF(CLM_PROF_GEMM, attn_flops(R, l));
    KCHK(gemm_attn(bf, R.causal, g.A, g.lda, g.W, g.ldw, g.bias, T.O, T.ldo, R.B, R.S, T.H, T.d, g.K, st));
  } else {
    { PROF(CLM_PROF_GEMM, 2.0 * g.M * g.N * g.K); KCHK(gemm(bf, EPI_STORE, g, st)); }
    { PROF(CLM_PROF_ATTN, 4.0 * R.B * T.H * (double)R.S * R.S * 64);
      KCHK(attention(bf, R.causal, T.QKV, 3 * T.d, T.O, T.ldo, R.B, R.S, T.H, T.d, st, T.q_log2e)); }
  }
  return CLM_OK;
}

// the pruned last layer's residual GEMMs have only B (pooled) rows: K is split into slices of
// >= 4 K-steps (a fixed count per shape, so a row's bits do not depend on B), partials in the
// QKV workspace, which is idle by then (B * S rows * 3d 16-bit values); 75 µs of idle chip per
// launch before (profiles/r02_v5_pooled_splitk_ab.txt)
int pooled_resid(clm_ctx* c, const LayerRun& R, GemmArgs& g, hipStream_t st) {
  const int nk = g.K / 64;
  int slices = 1;
  for (int sl = nk / 4; sl >= 2; --sl)
    if (nk % sl == 0 && gemm_splitk_ws_bytes(1, g.N, sl) <= (size_t)R.S * 3 * R.T->d * 2) { slices = sl; break; }
  PROF(CLM_PROF_GEMM, 2.0 * g.M * g.N * g.K);
  if (slices > 1) KCHK(gemm_splitk_resid(R.bf, g, slices, (float*)R.T->QKV, st));
  else KCHK(gemm_cfg(R.bf, EPI_RESID, GEMM_CFG_SPLITK, g, st));
  return CLM_OK;
}

// The four row-wise GEMMs and two LayerNorms of layer l after its attention, as (M rows of) one
// tower: out_proj (+= h), LN2 -> X, fc1 (GELU) -> Hm, fc2 (+= h), next layer's LN1 -> X.
struct PostOps {
  GemmArgs out, fc1, fc2;
  LnArgs ln2, ln1;
  bool has_ln1;
  double rows;   // executed rows (profiling)
};
PostOps post_ops(clm_ctx* c, const LayerRun& R, int l, int64_t M, float* h, u16* O, bool pooled) {
  Tower& T = *R.T;
  LayerW& Lw = T.layers[l];
  const int* mdev = pooled ? nullptr : R.mdev;
  PostOps p{};
  p.rows = pooled ? (double)M : R.Mx;
  GemmArgs& g = p.out;
  // pooled rows: split-K over whole 64-wide K-steps (the extension's pad columns are zero on both sides)
  g.A = O; g.lda = T.ldo; g.W = Lw.w_out; g.ldw = Lw.k_out; g.M = (int)M; g.N = T.d; g.K = pooled ? Lw.k_out : Lw.kl_out;
  g.out = h; g.ldo = T.d; g.bias = Lw.b_out; g.m_dev = mdev;
  p.ln2 = ln_into_x(c, T, M, Lw.ln2_g, Lw.ln2_b, h);
  p.ln2.m_dev = mdev;
  GemmArgs& f = p.fc1;
  f.A = T.X; f.lda = T.ldx; f.M = (int)M; f.N = T.mlp; f.K = Lw.k_fc1; f.out = T.Hm; f.ldo = T.ldm;
  f.W = Lw.w_fc1; f.ldw = Lw.k_fc1; f.bias = Lw.b_fc1; f.m_dev = mdev;
  GemmArgs& f2 = p.fc2;
  f2.A = T.Hm; f2.lda = T.ldm; f2.W = Lw.w_fc2; f2.ldw = Lw.k_fc2; f2.M = (int)M; f2.N = T.d;
  f2.K = pooled ? Lw.k_fc2 : Lw.kl_fc2;
  f2.out = h; f2.ldo = T.d; f2.bias = Lw.b_fc2; f2.m_dev = mdev;
  p.has_ln1 = l + 1 < T.L;
  if (p.has_ln1) {
    LayerW& Ln = T.layers[l + 1];
    p.ln1 = ln_into_x(c, T, M, Ln.ln1_g, Ln.ln1_b);
    p.ln1.m_dev = mdev;
  }
  return p;
}

// layer l after its attention, one tower. The last layer is pruned to the pooled rows
// (prune_last_layer): they are gathered into T.hc / T.Oc first and *pooled_rows is set.
int post_attn_step(clm_ctx* c, const LayerRun& R, int l, bool* pooled_rows, hipStream_t st) {
  Tower& T = *R.T;
  LayerW& Lw = T.layers[l];
  const bool bf = R.bf;
  const bool pooled = prune_last_layer() && l + 1 == T.L;
  int64_t M = (int64_t)R.B * R.S;
  float* h = T.h;
  u16* O = T.O;
  if (pooled) {
    { PROF(CLM_PROF_OTHER, (double)R.B * T.d * 6.0);
      KCHK(gather_pooled(T.h, T.d, T.O, T.ldo, R.B, R.S, T.d, R.ids, c->desc.eos_token_id, T.hc, T.Oc, T.ldo, st,
                         R.vl ? T.vl_offs : nullptr)); }
    M = R.B;
    h = T.hc;
    O = T.Oc;
    *pooled_rows = true;
  }
  PostOps p = post_ops(c, R, l, M, h, O, pooled);
  const int* mdev = pooled ? nullptr : R.mdev;
  if (Lw.r_out) { PROF(CLM_PROF_GEMM, 2.0 * p.rows * RPAD * T.d);
    KCHK(lora_down_gemm(bf, O, T.ldo, (int)M, T.d, Lw.a_out, mdev, st)); }
  if (pooled) {
    int r = pooled_resid(c, R, p.out, st);
    if (r) return r;
  } else {
    PROF(CLM_PROF_GEMM, 2.0 * p.rows * p.out.N * p.out.K); KCHK(gemm(bf, EPI_RESID, p.out, st));
  }
  { PROF(CLM_PROF_LN, p.rows * T.d * 6.0); KCHK(layernorm(bf, p.ln2, st)); }
  if (Lw.r_fc1) { PROF(CLM_PROF_GEMM, 2.0 * p.rows * RPAD * T.d);
    KCHK(lora_down_gemm(bf, T.X, T.ldx, (int)M, T.d, Lw.a_fc1, mdev, st)); }
  { PROF(CLM_PROF_GEMM, 2.0 * p.rows * p.fc1.N * p.fc1.K);   // pooled rows: 128 x 64 tiles (4 waves) fill the chip
    KCHK(pooled ? gemm_cfg(bf, EPI_GELU, GEMM_CFG_SPLITK, p.fc1, st) : gemm(bf, EPI_GELU, p.fc1, st)); }
  if (Lw.r_fc2) { PROF(CLM_PROF_GEMM, 2.0 * p.rows * RPAD * T.mlp);
    KCHK(lora_down_gemm(bf, T.Hm, T.ldm, (int)M, T.mlp, Lw.a_fc2, mdev, st)); }
  if (pooled) {
    int r = pooled_resid(c, R, p.fc2, st);
    if (r) return r;
  } else {
    PROF(CLM_PROF_GEMM, 2.0 * p.rows * p.fc2.N * p.fc2.K); KCHK(gemm(bf, EPI_RESID, p.fc2, st));
  }
  if (p.has_ln1) {
    { PROF(CLM_PROF_LN, p.rows * T.d * 6.0); KCHK(layernorm(bf, p.ln1, st)); }
    const LayerW& Ln = T.layers[l + 1];
    if (Ln.r_qkv) { PROF(CLM_PROF_GEMM, 2.0 * p.rows * RPAD * T.d);
      KCHK(lora_down_gemm(bf, T.X, T.ldx, (int)M, T.d, Ln.a_qkv, mdev, st)); }
  }
  return CLM_OK;
}

// encoder layers on the residual stream T.h; the first layer's LN1 output must already be in T.X.
// Returns with the pooled rows in T.hc (pruned: *pooled_rows = true) or all rows in T.h.
// (LayerNorm folded into the next GEMM -- producer moments in the residual epilogue, consumer
// W diag(gamma) + epilogue correction -- was parity-green but 3 % slower end to end and was
// removed: profiles/r02_v2_ln_fold_ab.txt.)
int run_layers(clm_ctx* c, Tower& T, int B, int S, bool causal, const int32_t* ids, bool* pooled_rows,
               hipStream_t st, bool vl = false) {
  *pooled_rows = false;
  LayerRun R;
  int r = make_run(c, T, B, S, causal, ids, vl, st, &R);
  for (int l = 0; !r && l < T.L; ++l) {
    r = attn_step(c, R, l, st);
    if (!r) r = post_attn_step(c, R, l, pooled_rows, st);
  }
  return r;
}

// the tower with its workspace pointers moved to sub-batch b0 (items of `rows` sequence rows)
Tower ws_view(const Tower& T0, int b0, int rows, int patches, int proj_dim) {
  Tower T = T0;
  const int64_t r0 = (int64_t)b0 * rows;
  T.h += r0 * T.d; T.X += r0 * T.ldx; T.QKV += r0 * 3 * T.d; T.O += r0 * T.ldo; T.Hm += r0 * T.ldm;
  if (T.P) T.P += (int64_t)b0 * patches * T.kp;
  T.pooled += (int64_t)b0 * proj_dim;
  T.hc += (int64_t)b0 * T.d;
  T.Oc += (int64_t)b0 * T.ldo;
  if (T.vl_lens) {
    T.vl_lens += b0; T.vl_tiles += b0; T.vl_offs += 2 * b0; T.vl_counts += 2 * b0; T.vl_rowmap += r0;
  }
  return T;
}

// image tower up to the first layer: patchify -> patch GEMM (+pos) -> class rows -> pre-LN + LN1 -> T.X
int image_prologue(clm_ctx* c, Tower& T, const void* pix, int layout, int B, hipStream_t st) {
  const clm_model_desc& d = c->desc;
  const bool bf = c->bf16(T.vision);
  const int G = d.image_size / d.patch, Tn = G * G + 1;
  { PROF(CLM_PROF_OTHER, (double)B * G * G * T.kp * 2.0 + (double)B * d.image_size * d.image_size * d.channels);
    KCHK(patchify(bf, pix, layout, B, d.image_size, d.patch, d.channels, T.lut, T.P, T.kp, st)); }
  GemmArgs g{};
  g.A = T.P; g.lda = T.kp; g.W = T.patch_w; g.ldw = T.kp; g.M = B * G * G; g.N = T.d; g.K = T.kp;
  g.out = T.h; g.ldo = T.d; g.aux = T.pos; g.aux_ld = T.d; g.group = G * G;
  { PROF(CLM_PROF_GEMM, 2.0 * g.M * g.N * g.K); KCHK(gemm(bf, EPI_PATCH, g, st)); }
  { PROF(CLM_PROF_OTHER, (double)B * T.d * 4.0); KCHK(write_cls(T.h, T.d, B, Tn, T.d, T.cls, T.pos, st)); }
  LnArgs a = ln_into_x(c, T, (int64_t)B * Tn, T.pre_g, T.pre_b);
  a.g2 = T.layers[0].ln1_g; a.b2 = T.layers[0].ln1_b;  // pre_layrnorm (in place) then layer-0 LN1
  { PROF(CLM_PROF_LN, (double)B * Tn * T.d * 10.0); KCHK(layernorm(bf, a, st)); }
  if (T.layers[0].r_qkv) { PROF(CLM_PROF_GEMM, 2.0 * B * Tn * RPAD * T.d);
    KCHK(lora_down_gemm(bf, T.X, T.ldx, B * Tn, T.d, T.layers[0].a_qkv, nullptr, st)); }
  return CLM_OK;
}

// pooled class rows -> post-LN -> projection (-> L2 norm) -> out
int image_epilogue(clm_ctx* c, Tower& T, int B, bool pooled_rows, void* out, int out_dtype, int normalize,
                   hipStream_t st) {
  const clm_model_desc& d = c->desc;
  const int G = d.image_size / d.patch, Tn = G * G + 1;
  PROF(CLM_PROF_OTHER, (double)B * (T.d * 4.0 + d.proj_dim * 4.0) + (double)T.d * d.proj_dim * 4.0);
  KCHK(pool_project(pooled_rows ? T.hc : T.h, T.d, B, pooled_rows ? 1 : Tn, T.d, nullptr, d.eos_token_id, T.fin_g,
                    T.fin_b, d.ln_eps, T.projT, d.proj_dim, T.pooled, out, out_dtype == CLM_F32 ? 0 : 1, normalize,
                    st));
  return CLM_OK;
}

int encode_image_chunk(clm_ctx* c, Tower& T, const void* pix, int layout, int B, void* out, int out_dtype,
                       int normalize, hipStream_t st) {
  const int G = c->desc.image_size / c->desc.patch;
  int r = image_prologue(c, T, pix, layout, B, st);
  bool pooled_rows = false;
  if (!r) r = run_layers(c, T, B, G * G + 1, false, nullptr, &pooled_rows, st);
  if (!r) r = image_epilogue(c, T, B, pooled_rows, out, out_dtype, normalize, st);
  return r;
}

// text tower up to the first layer: varlen plan (text_plan) -> token + position gather -> LN1 -> T.X.
// *vl: whether the live rows are packed (varlen path)
int text_prologue(clm_ctx* c, Tower& T, const int32_t* ids_dev, int B, int L, bool* vl_out, hipStream_t st) {
  const clm_model_desc& d = c->desc;
  const bool bf = c->bf16(T.vision);
  LnArgs a{};
  a.mode = 1; a.ids = ids_dev; a.tok = T.tok; a.pos = T.tpos; a.L = L;
  a.hf = T.h; a.ldh = T.d; a.g1 = T.layers[0].ln1_g; a.b1 = T.layers[0].ln1_b;
  a.y = T.X; a.ldy = T.ldx; a.M = B * L; a.d = T.d; a.eps = d.ln_eps;
  bool vl = text_varlen_enabled() && T.vl_lens && B <= 4096 &&   // text_plan: <= 4096 captions per chunk
            fused_attention(L, T.H, T.d, T.layers.empty() ? 0 : T.layers[0].k_qkv);
  if (vl) {
    { PROF(CLM_PROF_OTHER, (double)B * L * 8.0);
      KCHK(text_plan(ids_dev, B, L, d.eos_token_id, T.vl_lens, T.vl_offs, T.vl_rowmap, T.vl_tiles, T.vl_counts, st)); }
    a.m_dev = T.vl_counts;
    a.rowmap = T.vl_rowmap;
  }
  *vl_out = vl;
  { PROF(CLM_PROF_LN, (double)B * L * T.d * 14.0); KCHK(layernorm(bf, a, st)); }
  if (T.layers[0].r_qkv) { PROF(CLM_PROF_GEMM, 2.0 * B * L * RPAD * T.d);
    KCHK(lora_down_gemm(bf, T.X, T.ldx, B * L, T.d, T.layers[0].a_qkv, vl ? T.vl_counts : nullptr, st)); }
  return CLM_OK;
}

// pooled first-EOS rows -> final LN -> projection (-> L2 norm) -> out
int text_epilogue(clm_ctx* c, Tower& T, const int32_t* ids_dev, int B, int L, bool vl, bool pooled_rows, void* out,
                  int out_dtype, int normalize, hipStream_t st) {
  const clm_model_desc& d = c->desc;
  PROF(CLM_PROF_OTHER, (double)B * (T.d * 4.0 + d.proj_dim * 4.0 + L * 4.0) + (double)T.d * d.proj_dim * 4.0);
  KCHK(pool_project(pooled_rows ? T.hc : T.h, T.d, B, pooled_rows ? 1 : L, T.d, pooled_rows ? nullptr : ids_dev,
                    d.eos_token_id, T.fin_g, T.fin_b, d.ln_eps, T.projT, d.proj_dim, T.pooled, out,
                    out_dtype == CLM_F32 ? 0 : 1, normalize, st, vl && !pooled_rows ? T.vl_offs : nullptr));
  return CLM_OK;
}

int encode_text_chunk(clm_ctx* c, Tower& T, const int32_t* ids_dev, int B, int L, void* out, int out_dtype,
                      int normalize, hipStream_t st) {
  bool vl = false, pooled_rows = false;
  int r = text_prologue(c, T, ids_dev, B, L, &vl, st);
  if (!r) r = run_layers(c, T, B, L, true, ids_dev, &pooled_rows, st, vl);
  if (!r) r = text_epilogue(c, T, ids_dev, B, L, vl, pooled_rows, out, out_dtype, normalize, st);
  return r;
}

}  // namespace

extern "C" {

const char* clm_last_error(void) { return g_err.c_str(); }
const char* clm_version(void) { return "clm 0.1.0 gfx950"; }
int32_t clm_model_desc_size(void) { return (int32_t)sizeof(clm_model_desc); }

int clm_gemm(int hip_device, int dtype, int epilogue, int config, const void* A, int64_t lda, const void* W,
             int64_t ldw, int M, int N, int K, void* out, int64_t ldo, const float* bias, const float* rscale,
             const float* cscale, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (epilogue != EPI_STORE && epilogue != EPI_GELU && epilogue != EPI_RESID && epilogue != EPI_SCORE)
    return fail(CLM_E_ARG, "bad epilogue");
  if (config >= gemm_num_configs()) return fail(CLM_E_ARG, "bad config");
  // K % 64 == 32 (the unmerged-LoRA granule): rows must be readable to round_up(K, 64)
  const int64_t kr = (K + 63) / 64 * 64;
  if (M < 0 || N < 0 || K <= 0 || K % 32 || (K % 64 && (lda < kr || ldw < kr)))
    return fail(CLM_E_ARG, "bad shape (K % 64 == 0, or K % 64 == 32 with lda, ldw >= round_up(K, 64))");
  DeviceGuard g(hip_device);
  GemmArgs a{};
  a.A = (const u16*)A; a.lda = lda; a.W = (const u16*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.out = out; a.ldo = ldo; a.bias = bias; a.rscale = rscale; a.cscale = cscale;
  a.debug = g_gemm_debug;
  hipError_t e = gemm_cfg(dtype == CLM_BF16, epilogue, config, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_gemm_num_configs(void) { return gemm_num_configs(); }

// The sampled search's score matrix forms (search_bounded): fp16 A / W, score = acc * rscale[m] *
// cscale[n] stored as fp16 rounded toward -inf (mode 1, [M, ldo] u16) or as the maxima of each
// group of 4 consecutive columns, rounded the same way (mode 2: [M, ldo >= N / 4] u16, a row's
// groups in a fixed permutation; config 1 and N % 256 == 0, as the search runs it).
int clm_gemm_scores16(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M,
                      int N, int K, const float* rscale, const float* cscale, void* out, int64_t ldo, int mode,
                      void* stream) {
  if (mode != 1 && mode != 2) return fail(CLM_E_ARG, "mode must be 1 (fp16 scores) or 2 (group maxima)");
  if (config >= gemm_num_configs()) return fail(CLM_E_ARG, "bad config");
  if (M < 0 || N < 0 || K <= 0 || K % 64) return fail(CLM_E_ARG, "bad shape (K % 64 == 0)");
  if (mode == 2 && (config != 1 || N % 256 || ldo < N / 4 || ldo % 8))
    return fail(CLM_E_ARG, "group maxima: config 1, N % 256 == 0, ldo >= N / 4, ldo % 8 == 0");
  if (mode == 1 && ldo < N) return fail(CLM_E_ARG, "ldo < N");
  DeviceGuard g(hip_device);
  GemmArgs a{};
  a.A = (const u16*)A; a.lda = lda; a.W = (const u16*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.out = out; a.ldo = ldo; a.rscale = rscale; a.cscale = cscale; a.out16 = mode;
  hipError_t e = gemm_cfg(false, EPI_SCORE, config, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hook: the index passes' selecting epilogues alone (EPI_FILTER / EPI_RANK / EPI_LSE /
// EPI_FILTER_MASK, gemm_common.hpp), with every GemmArgs field the search sets for them. Nothing is
// zeroed here: cnt, above and the slab are the caller's, as in the search. (clm_gemm_select_keyed
// below: EPI_FILTER_KEYS, whose keys and ranges clm_gemm_select's signature has no room for.)
static int gemm_select_run(int hip_device, int epilogue, int config, const void* A, int64_t lda, const void* W,
                           int64_t ldw, int M, int N, int K, const float* rscale, const float* cscale,
                           const float* theta, int64_t theta_ld, float margin, int* cnt, float* cand_s,
                           int64_t* cand_i, int cap, int64_t base, const uint32_t* cbound, uint32_t* above,
                           float* lse_part, int64_t lse_ld, float lse_c, const uint32_t* mask, const int32_t* keys,
                           const int32_t* klo, const int32_t* khi, int m_fastest, void* stream) {
  if (config >= gemm_num_configs()) return fail(CLM_E_ARG, "bad config");
  if (M < 0 || N < 0 || K <= 0 || K % 64 || lda % 8 || ldw % 8 || lda < K || ldw < K)
    return fail(CLM_E_ARG, "bad shape (K % 64 == 0; lda, ldw multiples of 8 and >= K)");
  if (cap < 1 || theta_ld < 1) return fail(CLM_E_ARG, "gemm_select: cap >= 1 and theta_ld >= 1");
  if (epilogue == EPI_LSE && lse_ld < lse_slots(N)) return fail(CLM_E_ARG, "gemm_select: lse_ld < N / 64 + 4");
  if (M == 0 || N == 0) return CLM_OK;
  if (!A || !W || !cscale || !theta || !cnt || !cand_i) return fail(CLM_E_ARG, "gemm_select: null pointer");
  if ((epilogue == EPI_FILTER || epilogue == EPI_FILTER_MASK || epilogue == EPI_FILTER_KEYS) && !cand_s)
    return fail(CLM_E_ARG, "gemm_select: FILTER / FILTER_MASK / FILTER_KEYS write cand_s");
  if (epilogue == EPI_RANK && !above) return fail(CLM_E_ARG, "gemm_select: RANK counts into above");
  if (epilogue == EPI_LSE && !lse_part) return fail(CLM_E_ARG, "gemm_select: LSE writes lse_part");
  if (epilogue == EPI_FILTER_MASK && !mask) return fail(CLM_E_ARG, "gemm_select: FILTER_MASK reads mask");
  if (epilogue == EPI_FILTER_KEYS && (!keys || !klo || !khi || ((uintptr_t)keys & 15)))
    return fail(CLM_E_ARG, "gemm_select: FILTER_KEYS reads keys (16-byte aligned), klo and khi");
  DeviceGuard g(hip_device);
  GemmArgs a{};
  a.A = (const u16*)A; a.lda = lda; a.W = (const u16*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.rscale = rscale; a.cscale = cscale; a.theta = theta; a.theta_ld = theta_ld; a.rank_margin = margin;
  a.cnt = cnt; a.cand_s = cand_s; a.cand_i = cand_i; a.cap = cap; a.base = base; a.cbound = cbound;
  a.above = above; a.lse_part = lse_part; a.lse_ld = lse_ld; a.lse_c = lse_c; a.mask = mask;
  a.keys = keys; a.klo = klo; a.khi = khi;
  a.m_fastest = m_fastest ? 1 : 0;
  a.debug = g_gemm_debug;
  hipError_t e = gemm_cfg(false, epilogue, config, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_gemm_select(int hip_device, int epilogue, int config, const void* A, int64_t lda, const void* W, int64_t ldw,
                    int M, int N, int K, const float* rscale, const float* cscale, const float* theta,
                    int64_t theta_ld, float margin, int* cnt, float* cand_s, int64_t* cand_i, int cap, int64_t base,
                    const uint32_t* cbound, uint32_t* above, float* lse_part, int64_t lse_ld, float lse_c,
                    const uint32_t* mask, int m_fastest, void* stream) {
  if (!epi_selects(epilogue) || epilogue == EPI_FILTER_KEYS)
    return fail(CLM_E_ARG, "gemm_select: epilogue must be FILTER, RANK, LSE or FILTER_MASK");
  return gemm_select_run(hip_device, epilogue, config, A, lda, W, ldw, M, N, K, rscale, cscale, theta, theta_ld, margin,
                         cnt, cand_s, cand_i, cap, base, cbound, above, lse_part, lse_ld, lse_c, mask, nullptr,
                         nullptr, nullptr, m_fastest, stream);
}

int clm_gemm_select_keyed(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M,
                          int N, int K, const float* rscale, const float* cscale, const float* theta,
                          int64_t theta_ld, int* cnt, float* cand_s, int64_t* cand_i, int cap, int64_t base,
                          const uint32_t* cbound, const int32_t* keys, const int32_t* klo, const int32_t* khi,
                          int m_fastest, void* stream) {
  return gemm_select_run(hip_device, EPI_FILTER_KEYS, config, A, lda, W, ldw, M, N, K, rscale, cscale, theta, theta_ld,
                         0.f, cnt, cand_s, cand_i, cap, base, cbound, nullptr, nullptr, 0, 0.f, nullptr, keys, klo, khi,
                         m_fastest, stream);
}

// test hook: the order keys of min / max cscale (value_bounds, k_search.hip), the cbound of the index passes
int clm_value_bounds(int hip_device, const float* v, int64_t n, uint32_t* keys, void* stream) {
  if (n < 0 || !keys || (n > 0 && !v)) return fail(CLM_E_ARG, "value_bounds: n >= 0, keys, and v where n > 0");
  DeviceGuard g(hip_device);
  hipError_t e = value_bounds(v, n, keys, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("value_bounds: ") + hipGetErrorString(e));
  return CLM_OK;
}

void clm_debug_set(int flags) { g_gemm_debug = flags; }

int clm_attention_ex(int hip_device, int dtype, int flags, const void* qkv, void* out, int64_t ldo, int B, int T,
                     int H, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (B < 0 || T < 0 || H <= 0) return fail(CLM_E_ARG, "bad shape");
  DeviceGuard g(hip_device);
  if (flags & ~(CLM_ATTN_CAUSAL | CLM_ATTN_Q_LOG2E)) return fail(CLM_E_ARG, "unknown attention flags");
  const bool bf = dtype == CLM_BF16, cz = (flags & CLM_ATTN_CAUSAL) != 0, l2e = (flags & CLM_ATTN_Q_LOG2E) != 0;
  if (l2e && !attention_folds_log2e(bf, cz, T))
    return fail(CLM_E_ARG, "CLM_ATTN_Q_LOG2E: the kernel for this dtype / mask / T takes q without log2(e)");
  hipError_t e = attention(bf, cz, (const u16*)qkv, 3LL * H * 64, (u16*)out, ldo, B, T, H, H * 64,
                           (hipStream_t)stream, l2e);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("attention: ") + hipGetErrorString(e));
  return CLM_OK;
}

// the original entry point: `causal` is a 0 / non-0 switch (any non-zero value is the causal mask)
int clm_attention(int hip_device, int dtype, int causal, const void* qkv, void* out, int64_t ldo, int B, int T,
                  int H, void* stream) {
  return clm_attention_ex(hip_device, dtype, causal ? CLM_ATTN_CAUSAL : 0, qkv, out, ldo, B, T, H, stream);
}

int clm_layernorm(int hip_device, int dtype, const float* src, int64_t lds, int64_t M, int d, const float* gamma,
                  const float* beta, float eps, void* y, int64_t ldy, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (M < 0 || M > 0x7FFFFFFF || d <= 0 || d % 128 || d > 1024 || lds < d || ldy < d || (lds % 4) || (ldy % 4))
    return fail(CLM_E_ARG, "bad shape");
  if (M == 0) return CLM_OK;
  DeviceGuard g(hip_device);
  LnArgs a{};
  a.mode = 0; a.src = src; a.lds = lds; a.hf = nullptr; a.ldh = 0;
  a.g1 = gamma; a.b1 = beta; a.y = (u16*)y; a.ldy = ldy; a.M = (int)M; a.d = d; a.eps = eps;
  hipError_t e = layernorm(dtype == CLM_BF16, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("layernorm: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hook: the varlen text plan alone (text_plan, k_ops.hip), as text_prologue launches it
int clm_text_plan(int hip_device, const int32_t* ids, int B, int L, int eos, int* lens, int* offs, int* rowmap,
                  int* tiles, int* counts, void* stream) {
  if (B < 0 || B > 4096 || L < 1 || L > 256) return fail(CLM_E_ARG, "text_plan: 0 <= B <= 4096, 1 <= L <= 256");
  if (B == 0) return CLM_OK;
  if (!ids || !lens || !offs || !rowmap || !tiles || !counts) return fail(CLM_E_ARG, "text_plan: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = text_plan(ids, B, L, eos, lens, offs, rowmap, tiles, counts, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("text_plan: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hook: the fused q/k/v projection + attention alone (k_gemm_attn.hip); the four plan pointers
// all null: gemm_attn (B sequences of T rows), all set: gemm_attn_varlen (T = the padded length L)
int clm_gemm_attn(int hip_device, int dtype, int flags, const void* X, int64_t ldx, const void* W, int64_t ldw,
                  const float* bias, void* out, int64_t ldo, int B, int T, int H, int K, const int* lens,
                  const int* offs, const int* tiles, const int* counts, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (flags & ~CLM_ATTN_CAUSAL) return fail(CLM_E_ARG, "unknown attention flags");
  if (B < 0 || T < 0 || H <= 0 || H > 0x7FFFFFFF / 64) return fail(CLM_E_ARG, "bad shape");
  const int plan = (lens != nullptr) + (offs != nullptr) + (tiles != nullptr) + (counts != nullptr);
  if (plan != 0 && plan != 4) return fail(CLM_E_ARG, "gemm_attn: lens, offs, tiles and counts go together");
  if (B == 0) return CLM_OK;
  if (!X || !W || !out) return fail(CLM_E_ARG, "gemm_attn: null pointer");
  // K % 64 == 32: rows must be readable to round_up(K, 64), as in clm_gemm
  const int64_t kr = ((int64_t)K + 63) / 64 * 64;
  if (K > 0 && K % 64 && (ldx < kr || ldw < kr))
    return fail(CLM_E_ARG, "gemm_attn: K % 64 == 32 needs ldx, ldw >= round_up(K, 64)");
  DeviceGuard g(hip_device);
  const bool bf = dtype == CLM_BF16, cz = (flags & CLM_ATTN_CAUSAL) != 0;
  const hipError_t e =
      plan ? gemm_attn_varlen(bf, cz, (const u16*)X, ldx, (const u16*)W, ldw, bias, (u16*)out, ldo, B, T, H, H * 64, K,
                              lens, offs, tiles, counts, (hipStream_t)stream)
           : gemm_attn(bf, cz, (const u16*)X, ldx, (const u16*)W, ldw, bias, (u16*)out, ldo, B, T, H, H * 64, K,
                       (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm_attn: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hook: every field of LnArgs (layernorm, k_ops.hip) -- the text-embedding gather (mode 1), the
// dual LayerNorm (g2 / b2, hf), packed rows (m_dev, rowmap)
int clm_layernorm_ex(int hip_device, int dtype, int mode, const float* src, int64_t lds, const int32_t* ids,
                     const float* tok, const float* pos, int L, float* hf, int64_t ldh, const float* g1,
                     const float* b1, const float* g2, const float* b2, float eps, void* y, int64_t ldy, int64_t M,
                     int d, const int* m_dev, const int* rowmap, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (mode != 0 && mode != 1) return fail(CLM_E_ARG, "layernorm_ex: mode must be 0 (rows) or 1 (token + position gather)");
  if (M < 0 || M > 0x7FFFFFFF || d <= 0 || d % 128 || d > 1024 || ldy < d || (ldy % 4))
    return fail(CLM_E_ARG, "bad shape");
  if (mode == 0 && (lds < d || (lds % 4))) return fail(CLM_E_ARG, "bad shape (lds)");
  if (hf && (ldh < d || (ldh % 4))) return fail(CLM_E_ARG, "bad shape (ldh)");
  if (mode == 1 && (!ids || !tok || !pos || !hf)) return fail(CLM_E_ARG, "layernorm_ex: mode 1 needs ids, tok, pos and hf");
  if (mode == 1 && L < 1) return fail(CLM_E_ARG, "layernorm_ex: mode 1 needs L >= 1");
  if ((g2 != nullptr) != (b2 != nullptr)) return fail(CLM_E_ARG, "layernorm_ex: g2 and b2 go together");
  if (g2 && !hf) return fail(CLM_E_ARG, "layernorm_ex: the dual LayerNorm writes hf");
  if (rowmap && mode != 1) return fail(CLM_E_ARG, "layernorm_ex: rowmap is mode 1's");
  if (M == 0) return CLM_OK;
  if ((mode == 0 && !src) || !g1 || !b1 || !y) return fail(CLM_E_ARG, "layernorm_ex: null pointer");
  DeviceGuard g(hip_device);
  LnArgs a{};
  a.mode = mode; a.src = src; a.lds = lds; a.ids = ids; a.tok = tok; a.pos = pos; a.L = L; a.hf = hf; a.ldh = ldh;
  a.g1 = g1; a.b1 = b1; a.g2 = g2; a.b2 = b2; a.y = (u16*)y; a.ldy = ldy; a.M = (int)M; a.d = d; a.eps = eps;
  a.m_dev = m_dev; a.rowmap = rowmap;
  hipError_t e = layernorm(dtype == CLM_BF16, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("layernorm: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hook: the GEMM forms only the towers run -- EPI_PATCH (aux / aux_ld / group), a device-resident
// row count (m_dev), and with slices >= 1 the few-row split-K residual GEMM (gemm_splitk_resid)
int clm_gemm_ex(int hip_device, int dtype, int epilogue, int config, const void* A, int64_t lda, const void* W,
                int64_t ldw, int M, int N, int K, void* out, int64_t ldo, const float* bias, const float* aux,
                int64_t aux_ld, int group, const int* m_dev, int slices, float* ws, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (epilogue != EPI_STORE && epilogue != EPI_GELU && epilogue != EPI_RESID && epilogue != EPI_PATCH)
    return fail(CLM_E_ARG, "gemm_ex: epilogue must be STORE, GELU, RESID or PATCH");
  if (config >= gemm_num_configs()) return fail(CLM_E_ARG, "bad config");
  const int64_t kr = ((int64_t)K + 63) / 64 * 64;
  if (M < 0 || N < 0 || K <= 0 || K % 32 || (K % 64 && (lda < kr || ldw < kr)) || lda < K || ldw < K || ldo < N)
    return fail(CLM_E_ARG, "bad shape (K % 64 == 0, or K % 64 == 32 with lda, ldw >= round_up(K, 64); ldo >= N)");
  if (epilogue == EPI_PATCH) {
    if (!aux || aux_ld < N || group < 1 || M % group)
      return fail(CLM_E_ARG, "gemm_ex: EPI_PATCH needs aux, aux_ld >= N, group >= 1 and M % group == 0");
  } else if (aux || aux_ld || group) {
    return fail(CLM_E_ARG, "gemm_ex: aux, aux_ld and group are EPI_PATCH's");
  }
  if (slices < 0 || (slices == 0 && ws)) return fail(CLM_E_ARG, "gemm_ex: ws goes with slices >= 1");
  if (slices > 0 && (epilogue != EPI_RESID || m_dev || (config >= 0 && config != GEMM_CFG_SPLITK)))
    return fail(CLM_E_ARG, "gemm_ex: split-K is EPI_RESID on the 128 x 64 tile, without m_dev");
  if (M == 0 || N == 0) return CLM_OK;
  if (!A || !W || !out) return fail(CLM_E_ARG, "gemm_ex: null pointer");
  DeviceGuard g(hip_device);
  GemmArgs a{};
  a.A = (const u16*)A; a.lda = lda; a.W = (const u16*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.out = out; a.ldo = ldo; a.bias = bias; a.aux = aux; a.aux_ld = aux_ld; a.group = group; a.m_dev = m_dev;
  const bool bf = dtype == CLM_BF16;
  const hipError_t e = slices > 0 ? gemm_splitk_resid(bf, a, slices, ws, (hipStream_t)stream)
                                  : gemm_cfg(bf, epilogue, config, a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gemm: ") + hipGetErrorString(e));
  return CLM_OK;
}

// test hooks: the image prologue's and the pooled tail's row ops (k_ops.hip), as the launchers take them
int clm_patchify(int hip_device, int dtype, const void* pix, int layout, int B, int S, int p, int C,
                 const float* lut, void* P, int Kp, void* stream) {
  if (dtype != CLM_BF16 && dtype != CLM_F16) return fail(CLM_E_ARG, "dtype must be bf16 or f16");
  if (layout != CLM_PIX_U8_HWC && layout != CLM_PIX_F32_CHW) return fail(CLM_E_ARG, "bad pixel layout");
  if (B < 0 || S < 1 || p < 1 || S % p || C < 1 || C > 4 || S > 4096)
    return fail(CLM_E_ARG, "patchify: B >= 0, 1 <= p, S % p == 0, S <= 4096, 1 <= C <= 4");
  if (Kp < C * p * p) return fail(CLM_E_ARG, "patchify: Kp < C * p * p");
  if (B == 0) return CLM_OK;
  if (!pix || !lut || !P) return fail(CLM_E_ARG, "patchify: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = patchify(dtype == CLM_BF16, pix, layout == CLM_PIX_U8_HWC ? 0 : 1, B, S, p, C, lut, (u16*)P, Kp,
                          (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("patchify: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_write_cls(int hip_device, float* h, int64_t ldh, int B, int T, int d, const float* cls, const float* pos,
                  void* stream) {
  if (B < 0 || T < 1 || d < 1 || ldh < d) return fail(CLM_E_ARG, "write_cls: B >= 0, T >= 1, 1 <= d <= ldh");
  if (B == 0) return CLM_OK;
  if (!h || !cls || !pos) return fail(CLM_E_ARG, "write_cls: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = write_cls(h, ldh, B, T, d, cls, pos, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("write_cls: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_gather_pooled(int hip_device, const float* h, int64_t ldh, const void* O, int64_t ldo, int B, int T, int d,
                      const int32_t* ids, int eos, float* hc, void* Oc, int64_t ldoc, const int* offs, void* stream) {
  if (B < 0 || T < 1 || d < 1 || ldh < d || ldo < d || ldoc < d)
    return fail(CLM_E_ARG, "gather_pooled: B >= 0, T >= 1, 1 <= d <= ldh, ldo, ldoc");
  if (B == 0) return CLM_OK;
  if (!h || !O || !hc || !Oc) return fail(CLM_E_ARG, "gather_pooled: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = gather_pooled(h, ldh, (const u16*)O, ldo, B, T, d, ids, eos, hc, (u16*)Oc, ldoc, (hipStream_t)stream,
                               offs);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("gather_pooled: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_pool_project(int hip_device, const float* h, int64_t ldh, int B, int T, int d, const int32_t* ids, int eos,
                     const float* gamma, const float* beta, float eps, const float* projT, int D, float* tmp,
                     void* out, int out_dtype, int normalize, const int* offs, void* stream) {
  if (out_dtype != CLM_F32 && out_dtype != CLM_F16) return fail(CLM_E_ARG, "out_dtype must be f32 or f16");
  if (B < 0 || T < 1 || d < 1 || d > 1024 || D < 1 || ldh < d)
    return fail(CLM_E_ARG, "pool_project: B >= 0, T >= 1, 1 <= d <= min(ldh, 1024), D >= 1");
  if (B == 0) return CLM_OK;
  if (!h || !gamma || !beta || !projT || !tmp || !out) return fail(CLM_E_ARG, "pool_project: null pointer");
  DeviceGuard g(hip_device);
  hipError_t e = pool_project(h, ldh, B, T, d, ids, eos, gamma, beta, eps, projT, D, tmp, out,
                              out_dtype == CLM_F32 ? 0 : 1, normalize, (hipStream_t)stream, offs);
  if (e != hipSuccess) return fail(CLM_E_HIP, std::string("pool_project: ") + hipGetErrorString(e));
  return CLM_OK;
}

int clm_prof_enable(clm_ctx* ctx, int enable) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  DeviceGuard g(ctx->dev);
  (void)hipDeviceSynchronize();
  ctx->prof = enable != 0;
  ctx->recs.clear();
  ctx->ev_used = 0;
  return CLM_OK;
}

int clm_prof_read(clm_ctx* ctx, int category, double* ms, double* work, int64_t* launches) {
  if (!ctx || category < 0 || category >= CLM_PROF_NCAT) return fail(CLM_E_ARG, "bad argument");
  DeviceGuard g(ctx->dev);
  double t = 0, w = 0;
  int64_t n = 0;
  for (auto& r : ctx->recs) {
    if (r.cat != category) continue;
    HIPCHK(hipEventSynchronize(ctx->ev_pool[r.e1]));
    float m = 0.f;
    HIPCHK(hipEventElapsedTime(&m, ctx->ev_pool[r.e0], ctx->ev_pool[r.e1]));
    t += m; w += r.work; ++n;
  }
  if (ms) *ms = t;
  if (work) *work = w;
  if (launches) *launches = n;
  return CLM_OK;
}

int clm_ctx_create(int hip_device, const clm_model_desc* desc, clm_ctx** out) {
  if (!desc || !out) return fail(CLM_E_ARG, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(CLM_E_HIP, "no HIP device available");
  }
  if (hip_device < 0 || hip_device >= ndev) return fail(CLM_E_ARG, "bad device index");
  if (desc->compute_dtype != CLM_BF16 && desc->compute_dtype != CLM_F16 && desc->compute_dtype != CLM_COMPUTE_MIXED)
    return fail(CLM_E_ARG, "compute_dtype must be CLM_BF16, CLM_F16 or CLM_COMPUTE_MIXED");
  if (desc->max_batch <= 0 || desc->patch <= 0 || desc->image_size % desc->patch)
    return fail(CLM_E_ARG, "bad max_batch / patch / image_size");
  if (desc->max_pos > 77 * 4 || desc->proj_dim > 1024) return fail(CLM_E_ARG, "bad max_pos / proj_dim");
  if (desc->lora_r < 0 || desc->lora_r > 64) return fail(CLM_E_ARG, "lora_r must be in [0, 64]");
  clm_ctx* c = new clm_ctx();
  c->dev = hip_device;
  c->desc = *desc;
  *out = c;
  return CLM_OK;
}

int clm_ctx_destroy(clm_ctx* ctx) {
  if (!ctx) return CLM_OK;
  DeviceGuard g(ctx->dev);
  (void)hipDeviceSynchronize();
  ctx->free_all();
  for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : {ctx->ev_fork, ctx->ev_done})
    if (e) (void)hipEventDestroy(e);
  for (int i = 0; i < 2 * clm_ctx::MAX_SPLIT; ++i) {
    if (ctx->pev[i]) (void)hipEventDestroy(ctx->pev[i]);
    if (ctx->ps[i]) (void)hipStreamDestroy(ctx->ps[i]);
  }
  delete ctx;
  return CLM_OK;
}

int clm_load_tensor(clm_ctx* ctx, const char* name, const void* host_ptr, int dtype, const int64_t* shape,
                    int ndim) {
  if (!ctx || !name || (!host_ptr && ndim > 0) || ndim < 0 || ndim > 8) return fail(CLM_E_ARG, "bad argument");
  int64_t n = 1;
  HostTensor t;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(CLM_E_ARG, "negative dim");
    n *= shape[i];
    t.shape.push_back(shape[i]);
  }
  t.data.resize(n);
  if (dtype == CLM_F32) {
    std::memcpy(t.data.data(), host_ptr, n * sizeof(float));
  } else if (dtype == CLM_F16) {
    const uint16_t* p = (const uint16_t*)host_ptr;
    for (int64_t i = 0; i < n; ++i) t.data[i] = host_f16_to_f32(p[i]);
  } else if (dtype == CLM_BF16) {
    const uint16_t* p = (const uint16_t*)host_ptr;
    for (int64_t i = 0; i < n; ++i) t.data[i] = host_bf16_to_f32(p[i]);
  } else {
    return fail(CLM_E_ARG, "tensor dtype must be f32/f16/bf16");
  }
  ctx->host[name] = std::move(t);
  ctx->finalized = false;
  return CLM_OK;
}

int clm_finalize(clm_ctx* ctx) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  DeviceGuard g(ctx->dev);
  (void)hipDeviceSynchronize();
  ctx->free_all();
  ctx->finalized = false;
  int r = build_tower(ctx, ctx->vis, true);
  if (!r) r = build_tower(ctx, ctx->txt, false);
  if (!r) r = ctx->dalloc(&ctx->ids_dev, (size_t)ctx->desc.max_batch * ctx->desc.max_pos);
  if (r) {
    ctx->free_all();
    return r;
  }
  ctx->finalized = true;
  return CLM_OK;
}

int clm_set_lora(clm_ctx* ctx, int r, float alpha, uint32_t targets) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  if (r < 0 || r > 64) return fail(CLM_E_ARG, "lora_r must be in [0, 64]");
  if (targets & ~(uint32_t)(CLM_LORA_Q | CLM_LORA_K | CLM_LORA_V | CLM_LORA_OUT | CLM_LORA_FC1 | CLM_LORA_FC2))
    return fail(CLM_E_ARG, "unknown LoRA target bits");
  ctx->desc.lora_r = r;
  ctx->desc.lora_alpha = alpha;
  ctx->desc.lora_targets = r > 0 ? targets : 0u;
  ctx->finalized = false;   // the adapter tensors are loaded next, then clm_finalize
  return CLM_OK;
}

int clm_set_lora_enabled(clm_ctx* ctx, int enabled) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  ctx->lora_enabled = enabled != 0;
  return clm_finalize(ctx);
}

int clm_encode_image(clm_ctx* ctx, const void* pixels, int pix_layout, int n, void* out, int out_dtype,
                     int normalize, void* stream) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  if (!ctx->finalized) return fail(CLM_E_STATE, "clm_finalize has not been called");
  if (n < 0 || (n > 0 && (!pixels || !out))) return fail(CLM_E_ARG, "bad pixels/out/n");
  if (pix_layout != CLM_PIX_U8_HWC && pix_layout != CLM_PIX_F32_CHW) return fail(CLM_E_ARG, "bad pix_layout");
  if (out_dtype != CLM_F32 && out_dtype != CLM_F16) return fail(CLM_E_ARG, "out_dtype must be f32 or f16");
  if (n == 0) return CLM_OK;
  DeviceGuard g(ctx->dev);
  hipStream_t st = (hipStream_t)stream;
  const clm_model_desc& d = ctx->desc;
  const size_t pix_bytes = (size_t)d.image_size * d.image_size * d.channels * (pix_layout == CLM_PIX_U8_HWC ? 1 : 4);
  const size_t out_row = (size_t)d.proj_dim * dtype_size(out_dtype);
  const bool in_dev = is_device_ptr(pixels), out_dev = is_device_ptr(out);
  const int mb = d.max_batch;
  if (!in_dev) {
    int r = grow(&ctx->stage_in, &ctx->stage_in_bytes, pix_bytes * mb, "staging");
    if (r) return r;
  }
  if (!out_dev) {
    int r = grow(&ctx->stage_out, &ctx->stage_out_bytes, out_row * mb, "staging");
    if (r) return r;
  }
  for (int i0 = 0; i0 < n; i0 += mb) {
    const int B = std::min(mb, n - i0);
    const void* src = (const uint8_t*)pixels + (size_t)i0 * pix_bytes;
    if (!in_dev) {
      HIPCHK(hipMemcpyAsync(ctx->stage_in, src, pix_bytes * B, hipMemcpyHostToDevice, st));
      src = ctx->stage_in;
    }
    void* dst = out_dev ? (void*)((uint8_t*)out + (size_t)i0 * out_row) : ctx->stage_out;
    int r = encode_image_chunk(ctx, ctx->vis, src, pix_layout, B, dst, out_dtype, normalize, st);
    if (r) return r;
    if (!out_dev) {
      HIPCHK(hipMemcpyAsync((uint8_t*)out + (size_t)i0 * out_row, ctx->stage_out, out_row * B, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    } else if (!in_dev) {
      HIPCHK(hipStreamSynchronize(st));  // staging buffer reused next chunk
    }
  }
  return CLM_OK;
}

int clm_encode_text(clm_ctx* ctx, const int32_t* ids, int n, int L, void* out, int out_dtype, int normalize,
                    void* stream) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  if (!ctx->finalized) return fail(CLM_E_STATE, "clm_finalize has not been called");
  const clm_model_desc& d = ctx->desc;
  if (n < 0 || (n > 0 && (!ids || !out))) return fail(CLM_E_ARG, "bad ids/out/n");
  if (L <= 0 || L > d.max_pos)
    return fail(CLM_E_ARG, "sequence length " + std::to_string(L) + " outside [1, " + std::to_string(d.max_pos) + "]");
  if (out_dtype != CLM_F32 && out_dtype != CLM_F16) return fail(CLM_E_ARG, "out_dtype must be f32 or f16");
  if (n == 0) return CLM_OK;
  DeviceGuard g(ctx->dev);
  hipStream_t st = (hipStream_t)stream;
  const size_t out_row = (size_t)d.proj_dim * dtype_size(out_dtype);
  const bool in_dev = is_device_ptr(ids), out_dev = is_device_ptr(out);
  const int mb = d.max_batch;
  if (!out_dev) {
    int r = grow(&ctx->stage_out, &ctx->stage_out_bytes, out_row * mb, "staging");
    if (r) return r;
  }
  for (int i0 = 0; i0 < n; i0 += mb) {
    const int B = std::min(mb, n - i0);
    const int32_t* src = ids + (size_t)i0 * L;
    if (!in_dev) {
      for (int64_t q = 0; q < (int64_t)B * L; ++q)
        if (src[q] < 0 || src[q] >= d.vocab) return fail(CLM_E_ARG, "token id out of range");
      HIPCHK(hipMemcpyAsync(ctx->ids_dev, src, sizeof(int32_t) * B * L, hipMemcpyHostToDevice, st));
      src = ctx->ids_dev;
    }
    void* dst = out_dev ? (void*)((uint8_t*)out + (size_t)i0 * out_row) : ctx->stage_out;
    int r = encode_text_chunk(ctx, ctx->txt, src, B, L, dst, out_dtype, normalize, st);
    if (r) return r;
    if (!out_dev) {
      HIPCHK(hipMemcpyAsync((uint8_t*)out + (size_t)i0 * out_row, ctx->stage_out, out_row * B, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    } else if (!in_dev) {
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  return CLM_OK;
}

// Sub-batch launches of one encode_pair on ps[0..2*split): images on ps[2j], captions on
// ps[2j+1]. `fork` has been recorded on ps[0]; every other stream waits on it, and ps[0]
// waits on every other stream's pev at the end (join).
static int pair_launch(clm_ctx* c, int split, hipEvent_t fork, const void* pixels, int layout, int n_img,
                       const int32_t* ids, int n_txt, int L, void* oi, void* ot, int out_dtype, int normalize) {
  const clm_model_desc& d = c->desc;
  const int Tn = d.image_size / d.patch * (d.image_size / d.patch) + 1;
  const size_t pix_bytes = (size_t)d.image_size * d.image_size * d.channels * (layout == CLM_PIX_U8_HWC ? 1 : 4);
  const size_t out_row = (size_t)d.proj_dim * dtype_size(out_dtype);
  for (int i = 1; i < 2 * split; ++i) HIPCHK(hipStreamWaitEvent(c->ps[i], fork, 0));
  struct Concurrent {   // tile heuristic hint for the duration of the launches (k_gemm.hip)
    explicit Concurrent(bool on) { gemm_set_concurrent(on); }
    ~Concurrent() { gemm_set_concurrent(false); }
  } conc(n_img > 0 && n_txt > 0);
  const int G = d.image_size / d.patch;
  for (int j = 0; j < split; ++j) {
    const int i0 = (int)((int64_t)n_img * j / split), i1 = (int)((int64_t)n_img * (j + 1) / split);
    const int t0 = (int)((int64_t)n_txt * j / split), t1 = (int)((int64_t)n_txt * (j + 1) / split);
    if (i1 > i0) {
      Tower T = ws_view(c->vis, i0, Tn, G * G, d.proj_dim);
      int r = encode_image_chunk(c, T, (const uint8_t*)pixels + i0 * pix_bytes, layout, i1 - i0,
                                 (uint8_t*)oi + i0 * out_row, out_dtype, normalize, c->ps[2 * j]);
      if (r) return r;
    }
    if (t1 > t0) {
      Tower T = ws_view(c->txt, t0, L, 0, d.proj_dim);
      int r = encode_text_chunk(c, T, ids + (int64_t)t0 * L, t1 - t0, L, (uint8_t*)ot + t0 * out_row, out_dtype,
                                normalize, c->ps[2 * j + 1]);
      if (r) return r;
    }
  }
  for (int i = 1; i < 2 * split; ++i) {
    HIPCHK(hipEventRecord(c->pev[i], c->ps[i]));
    HIPCHK(hipStreamWaitEvent(c->ps[0], c->pev[i], 0));
  }
  return CLM_OK;
}

int clm_pair_path(const clm_ctx* ctx) { return ctx ? ctx->last_pair_path : -1; }

int clm_encode_pair(clm_ctx* ctx, const void* pixels, int pix_layout, int n_img, const int32_t* ids, int n_txt,
                    int L, void* out_img, void* out_txt, int out_dtype, int normalize, int flags, void* stream) {
  if (!ctx) return fail(CLM_E_ARG, "null ctx");
  if (!ctx->finalized) return fail(CLM_E_STATE, "clm_finalize has not been called");
  const clm_model_desc& d = ctx->desc;
  if (n_img < 0 || n_txt < 0 || n_img > d.max_batch || n_txt > d.max_batch)
    return fail(CLM_E_ARG, "clm_encode_pair: 0 <= n <= max_batch per tower");
  if (pix_layout != CLM_PIX_U8_HWC && pix_layout != CLM_PIX_F32_CHW) return fail(CLM_E_ARG, "bad pix_layout");
  if (out_dtype != CLM_F32 && out_dtype != CLM_F16) return fail(CLM_E_ARG, "out_dtype must be f32 or f16");
  if (n_txt && (L <= 0 || L > d.max_pos)) return fail(CLM_E_ARG, "bad sequence length");
  if ((n_img && (!is_device_ptr(pixels) || !is_device_ptr(out_img))) ||
      (n_txt && (!is_device_ptr(ids) || !is_device_ptr(out_txt))))
    return fail(CLM_E_ARG, "clm_encode_pair needs device buffers");
  if (n_img == 0 && n_txt == 0) return CLM_OK;
  DeviceGuard g(ctx->dev);
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->ps[0]) {
    for (int i = 0; i < 2 * clm_ctx::MAX_SPLIT; ++i) {
      HIPCHK(hipStreamCreateWithFlags(&ctx->ps[i], hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ctx->pev[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming));
  }
  // sub-batches per tower: flags, else CLM_PAIR_SPLIT, else by batch size
  static const int env_split = getenv("CLM_PAIR_SPLIT") ? atoi(getenv("CLM_PAIR_SPLIT")) : 0;
  int split = (flags >> CLM_PAIR_SPLIT_SHIFT) & 15;
  // default 1: with persistent GEMM grids (one workgroup per CU slot) more concurrent
  // sub-batch streams only contend; measured 43.9k vs 41.3k (2) vs 38.2k (4) pairs/s at B=256
  if (!split) split = env_split > 0 ? env_split : 1;
  split = std::max(1, std::min({split, clm_ctx::MAX_SPLIT, std::max(n_img, n_txt)}));
  const bool use_graph = (flags & CLM_PAIR_GRAPH) && !ctx->prof;
  ctx->last_pair_path = 0;   // one stream per tower piece (the only path; round 5's grouped launches were removed)
  HIPCHK(hipEventRecord(ctx->ev_fork, st));
  HIPCHK(hipStreamWaitEvent(ctx->ps[0], ctx->ev_fork, 0));
  if (!use_graph) {
    int r = pair_launch(ctx, split, ctx->ev_fork, pixels, pix_layout, n_img, ids, n_txt, L, out_img, out_txt,
                        out_dtype, normalize);
    if (r) return r;
  } else {
    // the diagnostic flags change which kernels run (varlen / fused / pruned): part of the key
    clm_ctx::PairKey key(pixels, pix_layout, n_img, ids, n_txt, L, out_img, out_txt, out_dtype, normalize,
                         split | (g_gemm_debug << 8));
    auto it = ctx->graphs.find(key);
    if (it == ctx->graphs.end()) {
      if (ctx->graphs.size() >= 16) ctx->drop_graphs();
      // capture the pure kernel DAG on ps[0]; the fork edge from the origin stream is the
      // wait on ev_fork above (outside the capture); inside, ev_done is the fork point
      HIPCHK(hipStreamBeginCapture(ctx->ps[0], hipStreamCaptureModeRelaxed));
      hipError_t e1 = hipEventRecord(ctx->ev_done, ctx->ps[0]);
      int r = e1 == hipSuccess ? pair_launch(ctx, split, ctx->ev_done, pixels, pix_layout, n_img, ids, n_txt, L,
                                             out_img, out_txt, out_dtype, normalize)
                               : CLM_OK;
      hipGraph_t graph = nullptr;
      hipError_t e3 = hipStreamEndCapture(ctx->ps[0], &graph);
      if (r) { if (graph) (void)hipGraphDestroy(graph); return r; }
      if (e1 != hipSuccess || e3 != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return fail(CLM_E_HIP, std::string("graph capture: ") + hipGetErrorString(e3 != hipSuccess ? e3 : e1));
      }
      hipGraphExec_t exec = nullptr;
      hipError_t e4 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (e4 != hipSuccess) return fail(CLM_E_HIP, std::string("graph instantiate: ") + hipGetErrorString(e4));
      it = ctx->graphs.emplace(key, exec).first;
    }
    HIPCHK(hipGraphLaunch(it->second, ctx->ps[0]));
  }
  HIPCHK(hipEventRecord(ctx->ev_done, ctx->ps[0]));
  HIPCHK(hipStreamWaitEvent(st, ctx->ev_done, 0));
  return CLM_OK;
}

}  // extern "C"
