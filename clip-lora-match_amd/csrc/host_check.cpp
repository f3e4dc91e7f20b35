// Host-side sanitizer harness of the C-ABI (ASan / UBSan build of the C-ABI
// layer). Built by `make sanitize` with the HOST half of every translation unit under
// -fsanitize=address,undefined (device code is compiled normally: GPU sanitizers are not
// available on this pool), and run without Python, so no preload is needed.
//
//  * every run: argument validation of each entry point (null pointers, bad shapes, bad
//    dtypes), error strings, version / layout queries;
//  * with a HIP device: the resident-index lifecycle (create, f16 + f32 appends that grow the
//    capacity, search on the scan and bounded paths, ranks on every route and their argument
//    validation, the log-sum-exp on every route and its argument validation, read-back, offset,
//    reset, destroy), remove / update round trips against a freshly built index and their
//    argument validation,
//    clm_cosine_scores / clm_topk_merge / clm_l2_normalize / clm_fuse_queries on host buffers,
//    each checked against a scalar host reference.
// Exit code 0 = all checks passed (the sanitizers abort the process on their own findings).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "clm.h"

// leaks LeakSanitizer reports at exit from inside the ROCm runtime (HSA / HIP objects that
// live for the process) are not ours; anything allocated by libclm or this harness still counts
extern "C" const char* __lsan_default_suppressions() { return "leak:libhsa-runtime64\nleak:libamdhip64\n"; }

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, \
                   clm_last_error());                                            \
      ++failures;                                                                \
    }                                                                            \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float frand() {   // xorshift64*, uniform in [-1, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (float)((rng_state * 2685821657736338717ull) >> 40) / (float)(1ull << 23) - 1.0f;
}

static void argument_checks() {
  CHECK(clm_version() && std::strlen(clm_version()) > 0);
  CHECK(clm_model_desc_size() == (int32_t)sizeof(clm_model_desc));
  clm_ctx* ctx = nullptr;
  CHECK(clm_ctx_create(0, nullptr, &ctx) == CLM_E_ARG);
  CHECK(std::strlen(clm_last_error()) > 0);
  CHECK(clm_ctx_destroy(nullptr) == CLM_OK);
  CHECK(clm_load_tensor(nullptr, "x", nullptr, CLM_F32, nullptr, 0) == CLM_E_ARG);
  CHECK(clm_finalize(nullptr) != CLM_OK);
  CHECK(clm_encode_image(nullptr, nullptr, CLM_PIX_U8_HWC, 1, nullptr, CLM_F32, 1, nullptr) != CLM_OK);
  CHECK(clm_encode_text(nullptr, nullptr, 1, 77, nullptr, CLM_F32, 1, nullptr) != CLM_OK);
  clm_index* idx = nullptr;
  CHECK(clm_index_create(0, 16, 100, &idx) != CLM_OK);    // dim % 64 != 0
  CHECK(clm_index_create(0, 16, 131072, &idx) != CLM_OK);   // dim > 65536
  CHECK(clm_index_destroy(nullptr) == CLM_OK);
  CHECK(clm_index_size(nullptr) < 0);
  CHECK(clm_index_search(nullptr, nullptr, CLM_F32, 1, 1, nullptr, nullptr, nullptr) != CLM_OK);
  CHECK(clm_index_search_masked(nullptr, nullptr, CLM_F32, 1, 1, nullptr, 0, nullptr, nullptr, nullptr) == CLM_E_ARG);
  CHECK(clm_index_search_keyed(nullptr, nullptr, CLM_F32, 1, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                               nullptr) == CLM_E_ARG);
  int64_t st[4];
  CHECK(clm_index_stats2(nullptr, st, 4) != CLM_OK);
  CHECK(clm_gemm(0, 99, CLM_EPI_STORE, -1, nullptr, 64, nullptr, 64, 1, 1, 64, nullptr, 1, nullptr, nullptr, nullptr,
                 nullptr) == CLM_E_ARG);
  CHECK(clm_attention(0, 99, 0, nullptr, nullptr, 64, 1, 1, 1, nullptr) == CLM_E_ARG);
  CHECK(clm_layernorm(0, CLM_BF16, nullptr, 100, 4, 100, nullptr, nullptr, 1e-5f, nullptr, 100, nullptr) == CLM_E_ARG);
  {   // the text plan and fused-attention hooks: shapes, null pointers, a partial plan
    int one[2] = {0, 0};
    const int32_t id1[1] = {0};
    CHECK(clm_text_plan(0, id1, -1, 77, 1, one, one, one, one, one, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, id1, 4097, 77, 1, one, one, one, one, one, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, id1, 1, 0, 1, one, one, one, one, one, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, id1, 1, 257, 1, one, one, one, one, one, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, nullptr, 1, 77, 1, one, one, one, one, one, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, id1, 1, 77, 1, one, one, one, one, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_text_plan(0, nullptr, 0, 77, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == CLM_OK);
    uint16_t x[1] = {0};
    CHECK(clm_gemm_attn(0, 99, 0, x, 64, x, 64, nullptr, x, 64, 1, 1, 1, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) == CLM_E_ARG);   // dtype
    CHECK(clm_gemm_attn(0, CLM_F16, CLM_ATTN_Q_LOG2E, x, 64, x, 64, nullptr, x, 64, 1, 1, 1, 64, nullptr, nullptr,
                        nullptr, nullptr, nullptr) == CLM_E_ARG);   // a flag of clm_attention_ex only
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, x, 64, -1, 1, 1, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) == CLM_E_ARG);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, x, 64, 1, 1, 0, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) == CLM_E_ARG);   // H = 0
    CHECK(clm_gemm_attn(0, CLM_F16, 0, nullptr, 64, x, 64, nullptr, x, 64, 1, 1, 1, 64, nullptr, nullptr, nullptr,
                        nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, nullptr, 64, 1, 1, 1, 64, nullptr, nullptr, nullptr,
                        nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gemm_attn(0, CLM_F16, CLM_ATTN_CAUSAL, x, 64, x, 64, nullptr, x, 64, 1, 1, 1, 64, one, one, one, nullptr,
                        nullptr) == CLM_E_ARG);   // three of the four plan pointers
    CHECK(clm_gemm_attn(0, CLM_F16, CLM_ATTN_CAUSAL, x, 64, x, 64, nullptr, x, 64, 1, 1, 1, 64, nullptr, nullptr,
                        nullptr, one, nullptr) == CLM_E_ARG);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 96, x, 128, nullptr, x, 64, 1, 1, 1, 96, nullptr, nullptr, nullptr, nullptr,
                        nullptr) == CLM_E_ARG);   // K % 64 == 32 with ldx < round_up(K, 64)
    // refused by the launcher before anything is launched: T > 128, K % 32 != 0, ldx % 8 != 0, ldo < d
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, x, 64, 1, 129, 1, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) != CLM_OK);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, x, 64, 1, 1, 1, 48, nullptr, nullptr, nullptr, nullptr,
                        nullptr) != CLM_OK);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 68, x, 64, nullptr, x, 64, 1, 1, 1, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) != CLM_OK);
    CHECK(clm_gemm_attn(0, CLM_F16, 0, x, 64, x, 64, nullptr, x, 60, 1, 1, 1, 64, nullptr, nullptr, nullptr, nullptr,
                        nullptr) != CLM_OK);
    CHECK(clm_gemm_attn(0, CLM_F16, CLM_ATTN_CAUSAL, x, 64, x, 64, nullptr, x, 64, 65536, 16, 1, 64, one, one, one,
                        one, nullptr) != CLM_OK);   // varlen: B > 65535
    CHECK(clm_gemm_attn(0, CLM_F16, 0, nullptr, 64, nullptr, 64, nullptr, nullptr, 64, 0, 1, 1, 64, nullptr, nullptr,
                        nullptr, nullptr, nullptr) == CLM_OK);   // B = 0: nothing to do
  }
  {   // the encoder row-op and tower-GEMM hooks: every case is refused (or empty) before any launch
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    uint16_t x[1] = {0};
    const int32_t id1[1] = {0};
    int one[2] = {0, 0};
    // clm_layernorm_ex(dev, dtype, mode, src, lds, ids, tok, pos, L, hf, ldh, g1, b1, g2, b2, eps, y, ldy, M, d,
    //                  m_dev, rowmap, stream)
    CHECK(clm_layernorm_ex(0, CLM_F32, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // dtype
    CHECK(clm_layernorm_ex(0, CLM_F16, 2, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // mode
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 128, -1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);  // M < 0
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 100, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 100, 1, 100, nullptr, nullptr, nullptr) == CLM_E_ARG);   // d % 128
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 130, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // ldy % 4
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, nullptr, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr,
                           nullptr, 1e-5f, x, 128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // null src
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, nullptr, nullptr,
                           nullptr, 1e-5f, x, 128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // null beta
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, nullptr, f, f, 1, f, 128, f, f, nullptr, nullptr, 1e-5f, x,
                           128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // mode 1 without ids
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, id1, nullptr, f, 1, f, 128, f, f, nullptr, nullptr, 1e-5f, x,
                           128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // ... tok
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, id1, f, nullptr, 1, f, 128, f, f, nullptr, nullptr, 1e-5f, x,
                           128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // ... pos
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, id1, f, f, 1, nullptr, 0, f, f, nullptr, nullptr, 1e-5f, x,
                           128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // ... hf
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, id1, f, f, 0, f, 128, f, f, nullptr, nullptr, 1e-5f, x, 128, 1,
                           128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // L < 1
    CHECK(clm_layernorm_ex(0, CLM_F16, 1, nullptr, 0, id1, f, f, 1, f, 64, f, f, nullptr, nullptr, 1e-5f, x, 128, 1,
                           128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // ldh < d
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, f, 128, f, f, f, nullptr, 1e-5f, x,
                           128, 1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // g2 without b2
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, f, f, 1e-5f, x, 128,
                           1, 128, nullptr, nullptr, nullptr) == CLM_E_ARG);   // the dual LN without hf
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, f, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, f, f, nullptr, nullptr,
                           1e-5f, x, 128, 1, 128, nullptr, one, nullptr) == CLM_E_ARG);   // rowmap in mode 0
    CHECK(clm_layernorm_ex(0, CLM_F16, 0, nullptr, 128, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr,
                           nullptr, nullptr, 1e-5f, nullptr, 128, 0, 128, nullptr, nullptr, nullptr) == CLM_OK);   // M = 0
    // clm_gemm_ex(dev, dtype, epi, config, A, lda, W, ldw, M, N, K, out, ldo, bias, aux, aux_ld, group, m_dev,
    //             slices, ws, stream)
    CHECK(clm_gemm_ex(0, 99, CLM_EPI_STORE, -1, x, 64, x, 64, 1, 1, 64, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // dtype
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_SCORE, -1, x, 64, x, 64, 1, 1, 64, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // not an encoder epilogue
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, 99, x, 64, x, 64, 1, 1, 64, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // config
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 64, x, 64, -1, 1, 64, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // M < 0
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 64, x, 64, 1, 1, 48, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // K % 32
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 96, x, 128, 1, 1, 96, x, 1, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // K % 64 == 32 with lda < round_up(K, 64)
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 64, x, 64, 1, 8, 64, x, 4, nullptr, nullptr, 0, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // ldo < N
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, nullptr, 64, x, 64, 1, 1, 64, x, 1, nullptr, nullptr, 0, 0,
                      nullptr, 0, nullptr, nullptr) == CLM_E_ARG);   // null A
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 64, x, 64, 1, 1, 64, nullptr, 1, nullptr, nullptr, 0, 0,
                      nullptr, 0, nullptr, nullptr) == CLM_E_ARG);   // null out
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_PATCH, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 4, 2, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // PATCH without aux
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_PATCH, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, f, 4, 0, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // group < 1
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_PATCH, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, f, 4, 3, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // M % group
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_PATCH, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, f, 2, 2, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // aux_ld < N
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_PATCH, -1, x, 64, x, 64, 4, 4, 64, f, 4, f, f, 4, 2, nullptr, 0, nullptr,
                      nullptr) == CLM_E_HIP);   // PATCH with a bias: the launcher's rule, before any launch
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, f, 4, 2, nullptr, 0,
                      nullptr, nullptr) == CLM_E_ARG);   // aux / group with another epilogue
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 0, 0, nullptr, -1,
                      nullptr, nullptr) == CLM_E_ARG);   // slices < 0
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 0, 0, nullptr, 0,
                      f, nullptr) == CLM_E_ARG);   // a workspace without slices
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, x, 64, x, 64, 4, 4, 64, x, 4, nullptr, nullptr, 0, 0, nullptr, 1,
                      f, nullptr) == CLM_E_ARG);   // split-K is RESID's
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, 0, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 0, 0, nullptr, 1, f,
                      nullptr) == CLM_E_ARG);   // ... on config 2 only
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 0, 0, one, 1, f,
                      nullptr) == CLM_E_ARG);   // ... without m_dev
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 4, 64, f, 4, nullptr, nullptr, 0, 0, nullptr, 1,
                      nullptr, nullptr) == CLM_E_HIP);   // no workspace: the launcher's
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 128, x, 128, 4, 4, 128, f, 4, nullptr, nullptr, 0, 0, nullptr,
                      3, f, nullptr) == CLM_E_HIP);   // K % (64 slices)
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_RESID, -1, x, 64, x, 64, 4, 6, 64, f, 6, nullptr, nullptr, 0, 0, nullptr, 1, f,
                      nullptr) == CLM_E_HIP);   // N % 4
    CHECK(clm_gemm_ex(0, CLM_F16, CLM_EPI_STORE, -1, nullptr, 64, nullptr, 64, 0, 4, 64, nullptr, 4, nullptr, nullptr,
                      0, 0, nullptr, 0, nullptr, nullptr) == CLM_OK);   // M = 0
    {   // the selecting epilogues' hook and the cscale bounds: refused (or empty) before any launch
      int64_t ci[1] = {0};
      uint32_t u[2] = {0u, 0u};
      // clm_gemm_select(dev, epi, config, A, lda, W, ldw, M, N, K, rscale, cscale, theta, theta_ld, margin, cnt,
      //                 cand_s, cand_i, cap, base, cbound, above, lse_part, lse_ld, lse_c, mask, m_fastest, stream)
      auto sel = [&](int epi, int cfg, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N, int K,
                     const float* cs, const float* th, int64_t theta_ld, int* cnt, float* cand_s, int64_t* cand_i,
                     int cap, uint32_t* above, float* slab, int64_t lse_ld, const uint32_t* mask) {
        return clm_gemm_select(0, epi, cfg, A, lda, W, ldw, M, N, K, nullptr, cs, th, theta_ld, 0.f, cnt, cand_s, cand_i,
                               cap, 0, nullptr, above, slab, lse_ld, 1.f, mask, 1, nullptr);
      };
      CHECK(sel(CLM_EPI_SCORE, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // epilogue
      CHECK(sel(9, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);
      CHECK(sel(CLM_EPI_FILTER, 99, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // config
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, -1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);  // M < 0
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, -1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);  // N < 0
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 0, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);    // K <= 0
      CHECK(sel(CLM_EPI_FILTER, -1, x, 96, x, 96, 1, 1, 96, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // K % 64
      CHECK(sel(CLM_EPI_FILTER, -1, x, 68, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // lda % 8
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 68, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // ldw % 8
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 128, 1, 1, 128, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG); // lda < K
      CHECK(sel(CLM_EPI_FILTER, -1, x, 128, x, 64, 1, 1, 128, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG); // ldw < K
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 0, u, f, 4, u) == CLM_E_ARG);   // cap < 1
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, f, 0, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // theta_ld < 1
      CHECK(sel(CLM_EPI_LSE, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 3, u) == CLM_E_ARG);   // lse_ld < 4
      CHECK(sel(CLM_EPI_LSE, -1, x, 64, x, 64, 1, 640, 64, f, f, 1, one, f, ci, 1, u, f, 13, u) == CLM_E_ARG);   // < 640 / 64 + 4
      CHECK(sel(CLM_EPI_FILTER, -1, nullptr, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // A
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, nullptr, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // W
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, nullptr, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // cscale
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, nullptr, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_ARG);   // theta
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, nullptr, f, ci, 1, u, f, 4, u) == CLM_E_ARG);     // cnt
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, nullptr, 1, u, f, 4, u) == CLM_E_ARG);    // cand_i
      CHECK(sel(CLM_EPI_FILTER, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, nullptr, ci, 1, u, f, 4, u) == CLM_E_ARG);   // cand_s
      CHECK(sel(CLM_EPI_FILTER_MASK, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, nullptr, ci, 1, u, f, 4, u) == CLM_E_ARG);
      CHECK(sel(CLM_EPI_FILTER_MASK, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, f, ci, 1, u, f, 4, nullptr) == CLM_E_ARG);   // mask
      CHECK(sel(CLM_EPI_RANK, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, nullptr, ci, 1, nullptr, f, 4, u) == CLM_E_ARG);    // above
      CHECK(sel(CLM_EPI_LSE, -1, x, 64, x, 64, 1, 1, 64, f, f, 1, one, nullptr, ci, 1, u, nullptr, 4, u) == CLM_E_ARG);     // slab
      // what the launcher refuses, before any launch: a tile without the epilogue
      CHECK(sel(CLM_EPI_FILTER, 13, x, 128, x, 128, 1, 8, 128, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_HIP);
      CHECK(sel(CLM_EPI_FILTER, 14, x, 128, x, 128, 1, 8, 128, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_HIP);
      for (int cfg : {0, 2, 3, 4, 5, 6, 7, 12, 13, 14}) {
        CHECK(sel(CLM_EPI_RANK, cfg, x, 128, x, 128, 1, 8, 128, f, f, 1, one, nullptr, ci, 1, u, f, 4, u) == CLM_E_HIP);
        CHECK(sel(CLM_EPI_LSE, cfg, x, 128, x, 128, 1, 8, 128, f, f, 1, one, nullptr, ci, 1, u, f, 4, u) == CLM_E_HIP);
        CHECK(sel(CLM_EPI_FILTER_MASK, cfg, x, 128, x, 128, 1, 8, 128, f, f, 1, one, f, ci, 1, u, f, 4, u) == CLM_E_HIP);
      }
      {   // clm_gemm_select_keyed(dev, config, A, lda, W, ldw, M, N, K, rscale, cscale, theta, theta_ld, cnt, cand_s,
          //                       cand_i, cap, base, cbound, keys, klo, khi, m_fastest, stream)
        alignas(16) int32_t kk[4] = {0, 1, 2, 3};
        int32_t kr[1] = {0};
        auto keyed = [&](int cfg, const void* A, int64_t lda, int M, int N, int K, float* cand_s, int cap,
                         const int32_t* keys, const int32_t* klo, const int32_t* khi) {
          return clm_gemm_select_keyed(0, cfg, A, lda, x, 64, M, N, K, nullptr, f, f, 1, one, cand_s, ci, cap, 0, nullptr,
                                       keys, klo, khi, 1, nullptr);
        };
        CHECK(keyed(99, x, 64, 1, 1, 64, f, 1, kk, kr, kr) == CLM_E_ARG);        // config
        CHECK(keyed(-1, x, 64, -1, 1, 64, f, 1, kk, kr, kr) == CLM_E_ARG);       // M < 0
        CHECK(keyed(-1, x, 96, 1, 1, 96, f, 1, kk, kr, kr) == CLM_E_ARG);        // K % 64
        CHECK(keyed(-1, x, 64, 1, 1, 64, f, 0, kk, kr, kr) == CLM_E_ARG);        // cap < 1
        CHECK(keyed(-1, nullptr, 64, 1, 1, 64, f, 1, kk, kr, kr) == CLM_E_ARG);  // A
        CHECK(keyed(-1, x, 64, 1, 1, 64, nullptr, 1, kk, kr, kr) == CLM_E_ARG);  // cand_s
        CHECK(keyed(-1, x, 64, 1, 1, 64, f, 1, nullptr, kr, kr) == CLM_E_ARG);   // keys
        CHECK(keyed(-1, x, 64, 1, 1, 64, f, 1, kk + 1, kr, kr) == CLM_E_ARG);    // ... 16-byte aligned
        CHECK(keyed(-1, x, 64, 1, 1, 64, f, 1, kk, nullptr, kr) == CLM_E_ARG);   // klo
        CHECK(keyed(-1, x, 64, 1, 1, 64, f, 1, kk, kr, nullptr) == CLM_E_ARG);   // khi
        CHECK(keyed(-1, nullptr, 64, 0, 4, 64, nullptr, 1, nullptr, nullptr, nullptr) == CLM_OK);   // M == 0
      }
      // nothing to do: M == 0 or N == 0, whatever the pointers
      CHECK(sel(CLM_EPI_FILTER, -1, nullptr, 64, nullptr, 64, 0, 4, 64, nullptr, nullptr, 1, nullptr, nullptr, nullptr, 1,
                nullptr, nullptr, 0, nullptr) == CLM_OK);
      CHECK(sel(CLM_EPI_LSE, -1, nullptr, 64, nullptr, 64, 4, 0, 64, nullptr, nullptr, 1, nullptr, nullptr, nullptr, 1,
                nullptr, nullptr, 4, nullptr) == CLM_OK);
      // clm_value_bounds(dev, v, n, keys, stream)
      CHECK(clm_value_bounds(0, f, -1, u, nullptr) == CLM_E_ARG);
      CHECK(clm_value_bounds(0, f, 4, nullptr, nullptr) == CLM_E_ARG);
      CHECK(clm_value_bounds(0, nullptr, 4, u, nullptr) == CLM_E_ARG);
    }
    // clm_patchify(dev, dtype, pix, layout, B, S, p, C, lut, P, Kp, stream)
    CHECK(clm_patchify(0, CLM_F32, x, CLM_PIX_U8_HWC, 1, 16, 8, 3, f, x, 192, nullptr) == CLM_E_ARG);   // dtype
    CHECK(clm_patchify(0, CLM_F16, x, 7, 1, 16, 8, 3, f, x, 192, nullptr) == CLM_E_ARG);                // layout
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, -1, 16, 8, 3, f, x, 192, nullptr) == CLM_E_ARG);
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 0, 3, f, x, 192, nullptr) == CLM_E_ARG);   // p < 1
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 5, 3, f, x, 192, nullptr) == CLM_E_ARG);   // S % p
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 8, 0, f, x, 192, nullptr) == CLM_E_ARG);   // C < 1
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 8, 3, f, x, 128, nullptr) == CLM_E_ARG);   // Kp < C p^2
    CHECK(clm_patchify(0, CLM_F16, nullptr, CLM_PIX_U8_HWC, 1, 16, 8, 3, f, x, 192, nullptr) == CLM_E_ARG);
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_F32_CHW, 1, 16, 8, 3, nullptr, x, 192, nullptr) == CLM_E_ARG);   // no lut
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 8, 3, f, nullptr, 192, nullptr) == CLM_E_ARG);
    CHECK(clm_patchify(0, CLM_F16, x, CLM_PIX_U8_HWC, 1, 16, 8, 3, f, x, 196, nullptr) == CLM_E_HIP);   // Kp % 8
    CHECK(clm_patchify(0, CLM_F16, nullptr, CLM_PIX_U8_HWC, 0, 16, 8, 3, nullptr, nullptr, 192, nullptr) == CLM_OK);
    // clm_write_cls(dev, h, ldh, B, T, d, cls, pos, stream)
    CHECK(clm_write_cls(0, f, 4, -1, 1, 4, f, f, nullptr) == CLM_E_ARG);
    CHECK(clm_write_cls(0, f, 4, 1, 0, 4, f, f, nullptr) == CLM_E_ARG);
    CHECK(clm_write_cls(0, f, 2, 1, 1, 4, f, f, nullptr) == CLM_E_ARG);   // ldh < d
    CHECK(clm_write_cls(0, nullptr, 4, 1, 1, 4, f, f, nullptr) == CLM_E_ARG);
    CHECK(clm_write_cls(0, f, 4, 1, 1, 4, nullptr, f, nullptr) == CLM_E_ARG);
    CHECK(clm_write_cls(0, f, 4, 1, 1, 4, f, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_write_cls(0, nullptr, 4, 0, 1, 4, nullptr, nullptr, nullptr) == CLM_OK);
    // clm_gather_pooled(dev, h, ldh, O, ldo, B, T, d, ids, eos, hc, Oc, ldoc, offs, stream)
    CHECK(clm_gather_pooled(0, f, 4, x, 4, -1, 1, 4, nullptr, 2, f, x, 4, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gather_pooled(0, f, 4, x, 4, 1, 0, 4, nullptr, 2, f, x, 4, nullptr, nullptr) == CLM_E_ARG);   // T < 1
    CHECK(clm_gather_pooled(0, f, 4, x, 4, 1, 1, 8, nullptr, 2, f, x, 8, nullptr, nullptr) == CLM_E_ARG);   // ldh < d
    CHECK(clm_gather_pooled(0, f, 4, x, 4, 1, 1, 4, nullptr, 2, f, x, 2, nullptr, nullptr) == CLM_E_ARG);   // ldoc < d
    CHECK(clm_gather_pooled(0, nullptr, 4, x, 4, 1, 1, 4, nullptr, 2, f, x, 4, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gather_pooled(0, f, 4, nullptr, 4, 1, 1, 4, nullptr, 2, f, x, 4, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gather_pooled(0, f, 4, x, 4, 1, 1, 4, nullptr, 2, nullptr, x, 4, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gather_pooled(0, f, 4, x, 4, 1, 1, 4, nullptr, 2, f, nullptr, 4, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_gather_pooled(0, f, 6, x, 8, 1, 1, 4, nullptr, 2, f, x, 4, nullptr, nullptr) == CLM_E_HIP);   // ldh % 4
    CHECK(clm_gather_pooled(0, nullptr, 4, nullptr, 4, 0, 1, 4, nullptr, 2, nullptr, nullptr, 4, nullptr, nullptr) ==
          CLM_OK);
    // clm_pool_project(dev, h, ldh, B, T, d, ids, eos, gamma, beta, eps, projT, D, tmp, out, out_dtype, normalize,
    //                  offs, stream)
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_BF16, 1, nullptr, nullptr) ==
          CLM_E_ARG);   // out dtype
    CHECK(clm_pool_project(0, f, 16, -1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 16, 1, 0, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_ARG);   // T < 1
    CHECK(clm_pool_project(0, f, 8, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_ARG);   // ldh < d
    CHECK(clm_pool_project(0, f, 2048, 1, 1, 2048, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_ARG);   // d > 1024
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 0, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_ARG);   // D < 1
    CHECK(clm_pool_project(0, nullptr, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr,
                           nullptr) == CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, nullptr, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr,
                           nullptr) == CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, nullptr, 4, f, f, CLM_F32, 1, nullptr,
                           nullptr) == CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, nullptr, f, CLM_F32, 1, nullptr,
                           nullptr) == CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 16, 1, 1, 16, nullptr, 2, f, f, 1e-5f, f, 4, f, nullptr, CLM_F32, 1, nullptr,
                           nullptr) == CLM_E_ARG);
    CHECK(clm_pool_project(0, f, 24, 1, 1, 24, nullptr, 2, f, f, 1e-5f, f, 4, f, f, CLM_F32, 1, nullptr, nullptr) ==
          CLM_E_HIP);   // d % 16
    CHECK(clm_pool_project(0, nullptr, 16, 0, 1, 16, nullptr, 2, nullptr, nullptr, 1e-5f, nullptr, 4, nullptr, nullptr,
                           CLM_F32, 1, nullptr, nullptr) == CLM_OK);
  }
  CHECK(clm_topk_merge(0, nullptr, nullptr, 1, 0, 1, 1, nullptr, nullptr, nullptr) != CLM_OK);
  CHECK(clm_l2_normalize(0, nullptr, 1, 0, nullptr) != CLM_OK);
  // clm_topk_distinct: shape errors, null and host pointers are refused before anything runs
  {
    float hs[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t hi[4] = {0, 1, 2, 3}, ho[3] = {0, 2, 4};
    int32_t hf[2] = {0, 0};
    CHECK(clm_topk_distinct(0, nullptr, nullptr, nullptr, nullptr, 4, 0, 5, nullptr, nullptr, nullptr, nullptr, nullptr) == CLM_OK);
    CHECK(clm_topk_distinct(0, nullptr, nullptr, nullptr, nullptr, 4, 1, 5, nullptr, nullptr, nullptr, nullptr, nullptr) == CLM_E_ARG);
    CHECK(clm_topk_distinct(0, hs, hi, hi, nullptr, 4, 1, 0, hs, hi, hi, hf, nullptr) == CLM_E_ARG);
    CHECK(clm_topk_distinct(0, hs, hi, hi, nullptr, 4, 1, 1025, hs, hi, hi, hf, nullptr) == CLM_E_ARG);
    CHECK(clm_topk_distinct(0, hs, hi, hi, nullptr, 4, -1, 2, hs, hi, hi, hf, nullptr) == CLM_E_ARG);
    CHECK(clm_topk_distinct(0, hs, hi, hi, nullptr, -4, 1, 2, hs, hi, hi, hf, nullptr) == CLM_E_ARG);
    CHECK(clm_topk_distinct(0, hs, hi, hi, ho, 0, 2, 2, hs, hi, hi, hf, nullptr) == CLM_E_ARG);   // host memory
  }
  CHECK(clm_scan16(0, nullptr, nullptr, -1, 64, nullptr, nullptr, 1, nullptr, 1, nullptr, nullptr, 0, nullptr) ==
        CLM_E_ARG);
  CHECK(clm_scan16(0, nullptr, nullptr, 256, 64, nullptr, nullptr, 1, nullptr, 1, nullptr, nullptr, 0, nullptr) ==
        CLM_E_ARG);   // not device pointers
  CHECK(clm_collect_ge(0, nullptr, 1, -1, 1, nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr) == CLM_E_ARG);
  CHECK(clm_index_set_offset(nullptr, 0) == CLM_E_ARG);
  // ranks: null index / null pointers
  float rq[64] = {1.f}, rs[1] = {0.f};
  int64_t rt[1] = {0}, ro[1] = {0};
  CHECK(clm_index_rank(nullptr, rq, CLM_F32, 1, rt, ro, rs, 0, nullptr) == CLM_E_ARG);
  CHECK(clm_index_count_above(nullptr, rq, CLM_F32, 1, rs, rt, ro, 0, nullptr) == CLM_E_ARG);
  // log-sum-exp: null index
  double rl[1] = {0.0};
  CHECK(clm_index_lse(nullptr, rq, CLM_F32, 1, 100.0, rs, rl, rs, 0, nullptr) == CLM_E_ARG);
  CHECK(clm_index_lse(nullptr, rq, CLM_F32, 0, 100.0, nullptr, nullptr, nullptr, 0, nullptr) == CLM_E_ARG);
  CHECK(clm_index_lse64(nullptr, rq, CLM_F32, 1, 100.0, nullptr, rl, nullptr, nullptr) == CLM_E_ARG);
  // remove / update: null index, whatever else is passed
  CHECK(clm_index_remove(nullptr, rt, 1, nullptr) == CLM_E_ARG);
  CHECK(clm_index_remove(nullptr, nullptr, 0, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(nullptr, rt, rq, CLM_F32, 1, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(nullptr, nullptr, nullptr, CLM_F32, 0, nullptr) == CLM_E_ARG);
}

// the index's whole internal state, as clm_index_export gives it
struct IndexState {
  int64_t n = -1;
  int has32 = -1;
  std::vector<uint16_t> r16;
  std::vector<float> inv, r32;
  bool operator==(const IndexState& o) const {
    return n == o.n && has32 == o.has32 && r16 == o.r16 && r32 == o.r32 &&
           (inv.empty() || std::memcmp(inv.data(), o.inv.data(), inv.size() * 4) == 0);
  }
};
static IndexState state_of(clm_index* idx, int dim) {
  IndexState s;
  s.n = clm_index_size(idx);
  s.has32 = clm_index_has_f32(idx);
  s.r16.resize((size_t)s.n * dim);
  s.inv.resize((size_t)s.n);
  if (s.has32 == 1) s.r32.resize((size_t)s.n * dim);
  CHECK(clm_index_export(idx, 0, s.n, s.r16.data(), s.inv.data(), s.has32 == 1 ? s.r32.data() : nullptr, nullptr) ==
        CLM_OK);
  return s;
}

// remove / update round trips against a fresh index (one built by appending the final rows in
// order, each run in its final dtype), and their argument validation on a live index
static void mutate_checks() {
  const int dim = 128, n16 = 300, n32 = 700, n = n16 + n32;
  std::vector<float> rows((size_t)n * dim);
  for (auto& v : rows) v = frand();
  std::vector<uint16_t> h16((size_t)n16 * dim);
  for (size_t i = 0; i < h16.size(); ++i) {
    const _Float16 h = (_Float16)rows[i];
    std::memcpy(&h16[i], &h, 2);
  }
  clm_index* idx = nullptr;
  CHECK(clm_index_create(0, 8, dim, &idx) == CLM_OK);
  if (!idx) return;
  CHECK(clm_index_append(idx, h16.data(), CLM_F16, n16, nullptr) == CLM_OK);
  CHECK(clm_index_append(idx, rows.data() + (size_t)n16 * dim, CLM_F32, n32, nullptr) == CLM_OK);
  CHECK(clm_index_set_offset(idx, 1000) == CLM_OK);
  const IndexState before = state_of(idx, dim);
  // argument validation: nothing changes
  int64_t ids[4] = {1000, 1000 + n - 1, 1005, 1005};
  CHECK(clm_index_remove(idx, nullptr, 2, nullptr) == CLM_E_ARG);
  CHECK(clm_index_remove(idx, ids, -1, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(idx, nullptr, rows.data(), CLM_F32, 2, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(idx, ids, nullptr, CLM_F32, 2, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(idx, ids, rows.data(), CLM_F32, -1, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(idx, ids, rows.data(), CLM_BF16, 2, nullptr) == CLM_E_ARG);
  CHECK(clm_index_update(idx, ids, rows.data(), CLM_F32, 4, nullptr) == CLM_E_ARG);   // 1005 twice
  for (int64_t bad : {(int64_t)-1, (int64_t)999, (int64_t)1000 + n, (int64_t)1 << 40}) {
    int64_t b[2] = {1001, bad};
    CHECK(clm_index_remove(idx, b, 2, nullptr) == CLM_E_ARG);
    CHECK(clm_index_update(idx, b, rows.data(), CLM_F32, 2, nullptr) == CLM_E_ARG);
  }
  CHECK(clm_index_remove(idx, ids, 0, nullptr) == CLM_OK);
  CHECK(clm_index_update(idx, ids, rows.data(), CLM_F32, 0, nullptr) == CLM_OK);
  CHECK(state_of(idx, dim) == before);
  // remove: every 7th row, the first, the last, 1005 twice, unsorted; chunks of 64 rows
  setenv("CLM_MUTATE_CHUNK_ROWS", "64", 1);
  std::vector<int64_t> rem = {1000 + n - 1, 1005, 1000, 1005};
  for (int j = 7; j < n - 1; j += 7) rem.push_back(1000 + j);
  CHECK(clm_index_remove(idx, rem.data(), (int64_t)rem.size(), nullptr) == CLM_OK);
  std::vector<char> gone(n, 0);
  for (int64_t v : rem) gone[v - 1000] = 1;
  // update: three survivors, f32 rows (one in the fp16 run, so the fresh index appends it as f32)
  const int64_t upd[3] = {1000 + 400, 1000 + 2, 1000 + 150};
  std::vector<float> fresh_rows((size_t)3 * dim);
  for (auto& v : fresh_rows) v = 3.0f * frand();
  CHECK(clm_index_update(idx, upd, fresh_rows.data(), CLM_F32, 3, nullptr) == CLM_OK);
  unsetenv("CLM_MUTATE_CHUNK_ROWS");
  // the fresh index: the final rows in order, run by run
  clm_index* fr = nullptr;
  CHECK(clm_index_create(0, 8, dim, &fr) == CLM_OK);
  if (fr) {
    int64_t pos = 0;
    for (int j = 0; j < n; ++j) {
      if (gone[j]) continue;
      int u = -1;
      for (int t = 0; t < 3; ++t)
        if (upd[t] - 1000 == pos) u = t;
      if (u >= 0) CHECK(clm_index_append(fr, &fresh_rows[(size_t)u * dim], CLM_F32, 1, nullptr) == CLM_OK);
      else if (j < n16) CHECK(clm_index_append(fr, &h16[(size_t)j * dim], CLM_F16, 1, nullptr) == CLM_OK);
      else CHECK(clm_index_append(fr, &rows[(size_t)j * dim], CLM_F32, 1, nullptr) == CLM_OK);
      ++pos;
    }
    CHECK(clm_index_size(idx) == pos);
    CHECK(state_of(idx, dim) == state_of(fr, dim));
    CHECK(clm_index_destroy(fr) == CLM_OK);
  }
  CHECK(clm_index_destroy(idx) == CLM_OK);
}

static double cos64(const float* a, const float* b, int dim) {
  double ab = 0, aa = 0, bb = 0;
  for (int e = 0; e < dim; ++e) {
    ab += (double)a[e] * b[e];
    aa += (double)a[e] * a[e];
    bb += (double)b[e] * b[e];
  }
  return ab / std::sqrt(aa * bb);
}

static void device_checks() {
  const int dim = 128, nq = 5, k = 7;
  // index: f16 rows first (upcast into the fp32 copy when the f32 rows arrive), capacity grows
  clm_index* idx = nullptr;
  CHECK(clm_index_create(0, 8, dim, &idx) == CLM_OK);
  if (!idx) return;
  const int n16 = 300, n32 = 2000, n = n16 + n32;
  std::vector<float> rows((size_t)n * dim);
  for (auto& v : rows) v = frand();
  std::vector<uint16_t> h16((size_t)n16 * dim);
  for (size_t i = 0; i < h16.size(); ++i) {
    const _Float16 h = (_Float16)rows[i];
    std::memcpy(&h16[i], &h, 2);
    rows[i] = (float)h;   // the fp16 rows as given are the reference rows
  }
  CHECK(clm_index_append(idx, h16.data(), CLM_F16, n16, nullptr) == CLM_OK);
  CHECK(clm_index_append(idx, rows.data() + (size_t)n16 * dim, CLM_F32, n32, nullptr) == CLM_OK);
  CHECK(clm_index_size(idx) == n);
  std::vector<float> back((size_t)n * dim);
  CHECK(clm_index_read(idx, 0, n, back.data(), nullptr) == CLM_OK);
  CHECK(std::memcmp(back.data(), rows.data(), back.size() * 4) == 0);
  CHECK(clm_index_read(idx, n - 1, 2, back.data(), nullptr) != CLM_OK);   // past the end

  std::vector<float> q((size_t)nq * dim);
  for (auto& v : q) v = frand();
  std::vector<float> sc((size_t)nq * k);
  std::vector<int64_t> ix((size_t)nq * k);
  for (int pass = 0; pass < 2; ++pass) {   // exact scan, then the bounded path
    if (pass == 1) setenv("CLM_SEARCH_BOUNDED", "1", 1);
    CHECK(clm_index_search(idx, q.data(), CLM_F32, nq, k, sc.data(), ix.data(), nullptr) == CLM_OK);
    for (int i = 0; i < nq; ++i) {
      // host reference: exact cosines, (score desc, index asc)
      std::vector<std::pair<double, int64_t>> all(n);
      for (int j = 0; j < n; ++j) all[j] = {cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim), j};
      std::partial_sort(all.begin(), all.begin() + k, all.end(), [](const auto& a, const auto& b) {
        return a.first > b.first || (a.first == b.first && a.second < b.second);
      });
      for (int t = 0; t < k; ++t) {
        CHECK(ix[(size_t)i * k + t] == all[t].second);
        CHECK(sc[(size_t)i * k + t] == (float)all[t].first);
      }
    }
    unsetenv("CLM_SEARCH_BOUNDED");
  }
  {   // filtered search on host buffers (every third row allowed, garbage past n in the last word),
      // every route, against the host reference over the allowed rows
    std::vector<uint32_t> allow((size_t)(n + 31) / 32, 0u);
    for (int j = 0; j < n; j += 3) allow[j >> 5] |= 1u << (j & 31);
    if (n % 32) allow.back() |= ~0u << (n % 32);
    for (int flag : {0, (int)CLM_MASK_EXACT, (int)CLM_MASK_PASS, (int)CLM_MASK_GATHER}) {
      CHECK(clm_index_search_masked(idx, q.data(), CLM_F32, nq, k, allow.data(), flag, sc.data(), ix.data(), nullptr) == CLM_OK);
      for (int i = 0; i < nq; ++i) {
        std::vector<std::pair<double, int64_t>> all;
        for (int j = 0; j < n; j += 3) all.push_back({cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim), j});
        std::sort(all.begin(), all.end(), [](const auto& a, const auto& b) {
          return a.first > b.first || (a.first == b.first && a.second < b.second);
        });
        for (int t = 0; t < k; ++t) {
          if (t < (int)all.size()) CHECK(ix[(size_t)i * k + t] == all[t].second && sc[(size_t)i * k + t] == (float)all[t].first);
          else CHECK(ix[(size_t)i * k + t] == -1);
        }
      }
    }
    int64_t ms[20] = {0};
    CHECK(clm_index_stats2(idx, ms, 20) == CLM_OK && ms[17] + ms[18] + ms[19] == 4 * (int64_t)nq);
    CHECK(clm_index_search_masked(idx, q.data(), CLM_F32, nq, k, nullptr, 0, sc.data(), ix.data(), nullptr) == CLM_E_ARG);
    CHECK(clm_index_search_masked(idx, q.data(), CLM_BF16, nq, k, allow.data(), 0, sc.data(), ix.data(), nullptr) == CLM_E_ARG);
    CHECK(clm_index_search_masked(idx, q.data(), CLM_F32, nq, 0, allow.data(), 0, sc.data(), ix.data(), nullptr) == CLM_E_ARG);
  }
  {   // keyed search on host buffers: key = row number mod 7, one range per query (query 1's empty), both
      // routes, against the host reference over each query's open rows; then what the entry point refuses
    std::vector<int32_t> keys(n), lo(nq), hi(nq);
    std::vector<int64_t> n_in(nq, 0);
    for (int j = 0; j < n; ++j) keys[j] = j % 7;
    for (int i = 0; i < nq; ++i) {
      lo[i] = i % 4;
      hi[i] = i == 1 ? -1 : i % 4 + i % 3;
      for (int j = 0; j < n; ++j) n_in[i] += lo[i] <= keys[j] && keys[j] <= hi[i];
    }
    for (int flag : {0, (int)CLM_MASK_EXACT, (int)CLM_MASK_PASS}) {
      for (const int64_t* counts : {(const int64_t*)n_in.data(), (const int64_t*)nullptr}) {
        CHECK(clm_index_search_keyed(idx, q.data(), CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), counts, flag,
                                     sc.data(), ix.data(), nullptr) == CLM_OK);
        for (int i = 0; i < nq; ++i) {
          std::vector<std::pair<double, int64_t>> all;
          for (int j = 0; j < n; ++j)
            if (lo[i] <= keys[j] && keys[j] <= hi[i]) all.push_back({cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim), j});
          std::sort(all.begin(), all.end(), [](const auto& a, const auto& b) {
            return a.first > b.first || (a.first == b.first && a.second < b.second);
          });
          for (int t = 0; t < k; ++t) {
            if (t < (int)all.size()) CHECK(ix[(size_t)i * k + t] == all[t].second && sc[(size_t)i * k + t] == (float)all[t].first);
            else CHECK(ix[(size_t)i * k + t] == -1);
          }
        }
      }
    }
    int64_t ks[22] = {0};
    CHECK(clm_index_stats2(idx, ks, 22) == CLM_OK && ks[20] + ks[21] == 6 * (int64_t)nq);
    auto keyed = [&](const void* qq, int dt, int64_t m, int kk, const int32_t* ky, const int32_t* l, const int32_t* h,
                     int flag, float* os) {
      return clm_index_search_keyed(idx, qq, dt, m, kk, ky, l, h, nullptr, flag, os, ix.data(), nullptr);
    };
    CHECK(keyed(nullptr, CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, nullptr, lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, keys.data(), nullptr, hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, keys.data(), lo.data(), nullptr, 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_BF16, nq, k, keys.data(), lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, -1, k, keys.data(), lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, 0, keys.data(), lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, 1025, keys.data(), lo.data(), hi.data(), 0, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), CLM_MASK_GATHER, sc.data()) == CLM_E_ARG);
    CHECK(keyed(q.data(), CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), 1, sc.data()) == CLM_E_ARG);   // an unknown flag
    CHECK(keyed(nullptr, CLM_F32, 0, k, nullptr, nullptr, nullptr, 0, nullptr) == CLM_OK);                  // nq == 0
    std::vector<int64_t> wrong(nq, 0);   // counts that say every range is empty: the pass route sees more
    CHECK(clm_index_search_keyed(idx, q.data(), CLM_F32, nq, k, keys.data(), lo.data(), hi.data(), wrong.data(),
                                 CLM_MASK_PASS, sc.data(), ix.data(), nullptr) == CLM_E_ARG);
  }
  CHECK(clm_index_set_offset(idx, 1000) == CLM_OK);
  CHECK(clm_index_search(idx, q.data(), CLM_F32, 1, 1, sc.data(), ix.data(), nullptr) == CLM_OK);
  CHECK(ix[0] >= 1000);
  {   // ranks of global targets on host buffers, every route, against a host count
    std::vector<int64_t> tg(nq), rk(nq), ab(nq), want(nq);
    std::vector<float> ts(nq);
    for (int i = 0; i < nq; ++i) {
      tg[i] = 1000 + (i * 577) % n;
      const double t = cos64(&q[(size_t)i * dim], &rows[(size_t)(tg[i] - 1000) * dim], dim);
      want[i] = 1;
      for (int j = 0; j < n; ++j) want[i] += cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim) > t;
    }
    for (int flag : {0, (int)CLM_RANK_BAND, (int)CLM_RANK_BAND | 4, (int)CLM_RANK_EXACT}) {
      CHECK(clm_index_rank(idx, q.data(), CLM_F32, nq, tg.data(), rk.data(), ts.data(), flag, nullptr) == CLM_OK);
      CHECK(clm_index_count_above(idx, q.data(), CLM_F32, nq, ts.data(), tg.data(), ab.data(), flag, nullptr) == CLM_OK);
      for (int i = 0; i < nq; ++i) CHECK(rk[i] == want[i] && ab[i] == want[i] - 1);
    }
    // argument validation: null pointers, a dtype other than f32 / f16, targets outside [offset, offset + n)
    CHECK(clm_index_rank(idx, nullptr, CLM_F32, nq, tg.data(), rk.data(), ts.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_rank(idx, q.data(), CLM_F32, nq, nullptr, rk.data(), ts.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_rank(idx, q.data(), CLM_F32, nq, tg.data(), nullptr, ts.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_rank(idx, q.data(), CLM_F32, nq, tg.data(), rk.data(), nullptr, 0, nullptr) == CLM_OK);
    CHECK(clm_index_rank(idx, q.data(), CLM_BF16, nq, tg.data(), rk.data(), ts.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_rank(idx, q.data(), CLM_F32, -1, tg.data(), rk.data(), ts.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_count_above(idx, q.data(), CLM_F32, nq, nullptr, tg.data(), ab.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_count_above(idx, q.data(), CLM_F32, nq, ts.data(), nullptr, ab.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_count_above(idx, q.data(), CLM_F32, nq, ts.data(), tg.data(), nullptr, 0, nullptr) == CLM_E_ARG);
    for (int64_t bad : {(int64_t)-1, (int64_t)999, (int64_t)1000 + n, (int64_t)1 << 40}) {
      tg[nq - 1] = bad;
      CHECK(clm_index_rank(idx, q.data(), CLM_F32, nq, tg.data(), rk.data(), ts.data(), 0, nullptr) == CLM_E_ARG);
    }
  }
  {   // log-sum-exp on host buffers, every route, against a host fp64 sum; then argument validation
    const double scale = 1.0 / 0.07;
    std::vector<float> floor_(nq);
    std::vector<double> want(nq), got(nq);
    std::vector<float> er(nq);
    for (int i = 0; i < nq; ++i) {
      std::vector<float> s(n);
      for (int j = 0; j < n; ++j) s[j] = (float)cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim);
      double acc = 0;
      for (int j = 0; j < n; ++j) acc += std::exp(scale * (double)s[j]);
      want[i] = std::log(acc);
      std::nth_element(s.begin(), s.begin() + 15, s.end(), [](float a, float b) { return a > b; });
      floor_[i] = s[15];   // the 16th best score
    }
    for (int flag : {0, (int)CLM_LSE_FAST, (int)CLM_LSE_FAST | 4, (int)CLM_LSE_EXACT}) {
      CHECK(clm_index_lse(idx, q.data(), CLM_F32, nq, scale, floor_.data(), got.data(), er.data(), flag, nullptr) == CLM_OK);
      // 1e-6: the host cosines may differ from the library's in their last fp32 bit
      for (int i = 0; i < nq; ++i) CHECK(std::fabs(got[i] - want[i]) <= (double)er[i] + 1e-6);
    }
    CHECK(clm_index_lse(idx, q.data(), CLM_F32, nq, scale, nullptr, got.data(), nullptr, 0, nullptr) == CLM_OK);
    int64_t ls[14];
    CHECK(clm_index_stats2(idx, ls, 14) == CLM_OK && ls[11] >= nq && ls[12] >= 3 * nq && ls[13] >= nq);
    CHECK(clm_index_lse(idx, nullptr, CLM_F32, nq, scale, floor_.data(), got.data(), er.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_lse(idx, q.data(), CLM_F32, nq, scale, floor_.data(), nullptr, er.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_lse(idx, q.data(), CLM_BF16, nq, scale, floor_.data(), got.data(), er.data(), 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_lse(idx, q.data(), CLM_F32, -1, scale, floor_.data(), got.data(), er.data(), 0, nullptr) == CLM_E_ARG);
    for (double bad : {0.0, -1.0, (double)INFINITY, (double)NAN})
      CHECK(clm_index_lse(idx, q.data(), CLM_F32, nq, bad, floor_.data(), got.data(), er.data(), 0, nullptr) == CLM_E_ARG);
    {   // the reference route: unrounded cosines, and the pair scores of rows i
      std::vector<int64_t> tg(nq);
      std::vector<double> pr(nq);
      for (int i = 0; i < nq; ++i) tg[i] = 1000 + i % n;   // the offset set above
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, scale, tg.data(), got.data(), pr.data(), nullptr) == CLM_OK);
      for (int i = 0; i < nq; ++i) {
        double acc = 0;
        for (int j = 0; j < n; ++j) acc += std::exp(scale * cos64(&q[(size_t)i * dim], &rows[(size_t)j * dim], dim));
        CHECK(std::fabs(got[i] - std::log(acc)) <= 1e-10);
        CHECK(std::fabs(pr[i] - cos64(&q[(size_t)i * dim], &rows[(size_t)(tg[i] - 1000) * dim], dim)) <= 1e-12);
      }
      tg[0] = 1000 + n;   // a row the index does not hold
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, scale, tg.data(), got.data(), pr.data(), nullptr) == CLM_OK);
      CHECK(std::isnan(pr[0]) && !std::isnan(pr[nq - 1]));
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, scale, nullptr, got.data(), nullptr, nullptr) == CLM_OK);
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, scale, nullptr, got.data(), pr.data(), nullptr) == CLM_E_ARG);
      CHECK(clm_index_lse64(idx, nullptr, CLM_F32, nq, scale, nullptr, got.data(), nullptr, nullptr) == CLM_E_ARG);
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, scale, nullptr, nullptr, nullptr, nullptr) == CLM_E_ARG);
      CHECK(clm_index_lse64(idx, q.data(), CLM_BF16, nq, scale, nullptr, got.data(), nullptr, nullptr) == CLM_E_ARG);
      CHECK(clm_index_lse64(idx, q.data(), CLM_F32, nq, 0.0, nullptr, got.data(), nullptr, nullptr) == CLM_E_ARG);
    }
  }
  double st_lse = 0.0;
  int64_t st[4] = {-1, -1, -1, -1};
  CHECK(clm_index_stats2(idx, st, 4) == CLM_OK && st[0] >= 0);
  CHECK(clm_index_reset(idx) == CLM_OK && clm_index_size(idx) == 0);
  CHECK(clm_index_lse(idx, q.data(), CLM_F32, 1, 100.0, nullptr, &st_lse, nullptr, 0, nullptr) == CLM_E_ARG);   // empty
  CHECK(clm_index_search(idx, q.data(), CLM_F32, nq, 3, sc.data(), ix.data(), nullptr) == CLM_OK);
  CHECK(ix[0] == -1 && std::isinf(sc[0]));   // empty index: (-inf, -1) slots
  {   // ... which the keyed search refuses
    int32_t k0 = 0;
    CHECK(clm_index_search_keyed(idx, q.data(), CLM_F32, 1, 3, &k0, &k0, &k0, nullptr, 0, sc.data(), ix.data(),
                                 nullptr) == CLM_E_ARG);
  }
  {   // ... which has no ranks
    int64_t t0 = 1000, r0 = 0;
    float s0 = 0.f;
    CHECK(clm_index_rank(idx, q.data(), CLM_F32, 1, &t0, &r0, &s0, 0, nullptr) == CLM_E_ARG);
    CHECK(clm_index_count_above(idx, q.data(), CLM_F32, 1, &s0, &t0, &r0, 0, nullptr) == CLM_E_ARG);
  }
  CHECK(clm_index_destroy(idx) == CLM_OK);

  // near-duplicate rows: 3000 copies of one row (and 3000 others) overflow the bounded path's
  // 2048-candidate lists; those queries take the whole-list pass (overflow_wide), k = 7 and 1024
  {
    const int nd = 6000, ndup = 3000, nqd = 4;
    std::vector<float> drows((size_t)nd * dim);
    for (auto& v : drows) v = frand();
    for (int j = 1; j < ndup; ++j) std::memcpy(&drows[(size_t)(2 * j) * dim], &drows[0], dim * 4);   // even rows
    clm_index* di = nullptr;
    CHECK(clm_index_create(0, nd, dim, &di) == CLM_OK);
    if (di) {
      CHECK(clm_index_append(di, drows.data(), CLM_F32, nd, nullptr) == CLM_OK);
      std::vector<float> dq((size_t)nqd * dim);
      for (auto& v : dq) v = frand();
      std::memcpy(dq.data(), drows.data(), dim * 4);
      std::memcpy(dq.data() + 2 * dim, drows.data(), dim * 4);
      setenv("CLM_SEARCH_BOUNDED", "1", 1);
      for (int kk : {7, 1024}) {
        int64_t s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
        CHECK(clm_index_stats2(di, s0, 4) == CLM_OK);
        std::vector<float> dsc((size_t)nqd * kk);
        std::vector<int64_t> dix((size_t)nqd * kk);
        CHECK(clm_index_search(di, dq.data(), CLM_F32, nqd, kk, dsc.data(), dix.data(), nullptr) == CLM_OK);
        CHECK(clm_index_stats2(di, s1, 4) == CLM_OK && s1[3] - s0[3] >= 2);   // the two duplicate queries
        for (int i = 0; i < nqd; ++i) {
          std::vector<std::pair<double, int64_t>> all(nd);
          for (int j = 0; j < nd; ++j) all[j] = {cos64(&dq[(size_t)i * dim], &drows[(size_t)j * dim], dim), j};
          std::partial_sort(all.begin(), all.begin() + kk, all.end(), [](const auto& a, const auto& b) {
            return a.first > b.first || (a.first == b.first && a.second < b.second);
          });
          for (int t = 0; t < kk; ++t) {
            CHECK(dix[(size_t)i * kk + t] == all[t].second);
            CHECK(dsc[(size_t)i * kk + t] == (float)all[t].first);
          }
        }
      }
      unsetenv("CLM_SEARCH_BOUNDED");
      CHECK(clm_index_destroy(di) == CLM_OK);
    }
  }

  // exact cosine matrix on host buffers, any dim
  const int cd = 77, cn = 33;
  std::vector<float> cq((size_t)nq * cd), cc((size_t)cn * cd), cout((size_t)nq * cn);
  for (auto& v : cq) v = frand();
  for (auto& v : cc) v = frand();
  CHECK(clm_cosine_scores(0, cq.data(), nq, cc.data(), cn, cd, cout.data(), nullptr) == CLM_OK);
  for (int i = 0; i < nq; ++i)
    for (int j = 0; j < cn; ++j) CHECK(cout[(size_t)i * cn + j] == (float)cos64(&cq[(size_t)i * cd], &cc[(size_t)j * cd], cd));

  // two sorted lists per query merge into one
  const int parts = 2, kin = 4, km = 5;
  std::vector<float> ms = {0.9f, 0.5f, 0.4f, 0.1f, 0.8f, 0.5f, 0.3f, 0.2f};
  std::vector<int64_t> mi = {3, 9, 1, 7, 4, 2, 8, 6};
  std::vector<float> os(km);
  std::vector<int64_t> oi(km);
  CHECK(clm_topk_merge(0, ms.data(), mi.data(), 1, parts, kin, km, os.data(), oi.data(), nullptr) == CLM_OK);
  const int64_t want[km] = {3, 4, 2, 9, 1};
  for (int t = 0; t < km; ++t) CHECK(oi[t] == want[t]);

  // a merge past one LDS sort (topk_any): 5 lists of 3000 with ties and empty slots, k = 4500,
  // against a host sort by (score desc, index asc)
  {
    const int P = 5, KI = 3000, K = 4500, NQ = 2;
    std::vector<float> bs((size_t)NQ * P * KI);
    std::vector<int64_t> bi(bs.size());
    for (size_t j = 0; j < bs.size(); ++j) {
      bs[j] = (float)((int)(frand() * 64.f)) / 64.f;   // many exact ties
      bi[j] = (j % 997 == 5) ? -1 : (int64_t)((j * 7919) % 1000003);
    }
    std::vector<float> bos((size_t)NQ * K);
    std::vector<int64_t> boi((size_t)NQ * K);
    CHECK(clm_topk_merge(0, bs.data(), bi.data(), NQ, P, KI, K, bos.data(), boi.data(), nullptr) == CLM_OK);
    for (int q = 0; q < NQ; ++q) {
      std::vector<std::pair<float, int64_t>> v;
      for (int j = 0; j < P * KI; ++j) {
        const size_t o = (size_t)q * P * KI + j;
        if (bi[o] >= 0) v.push_back({bs[o], bi[o]});
      }
      std::sort(v.begin(), v.end(), [](const std::pair<float, int64_t>& x, const std::pair<float, int64_t>& y) {
        return x.first != y.first ? x.first > y.first : x.second < y.second;
      });
      int bad = 0;
      for (int t = 0; t < K; ++t) bad += (boi[(size_t)q * K + t] != v[t].second || bos[(size_t)q * K + t] != v[t].first);
      CHECK(bad == 0);
    }
  }

  // l2 normalise and query fusion in place on host rows
  std::vector<float> a((size_t)3 * dim), b((size_t)3 * dim);
  for (auto& v : a) v = frand();
  for (auto& v : b) v = frand();
  std::vector<float> fused(a.size());
  CHECK(clm_fuse_queries(0, a.data(), 0.7f, b.data(), 0.3f, 3, dim, fused.data(), nullptr) == CLM_OK);
  CHECK(clm_l2_normalize(0, a.data(), 3, dim, nullptr) == CLM_OK);
  for (int r = 0; r < 3; ++r) {
    double s2 = 0, f2 = 0;
    for (int e = 0; e < dim; ++e) {
      s2 += (double)a[(size_t)r * dim + e] * a[(size_t)r * dim + e];
      f2 += (double)fused[(size_t)r * dim + e] * fused[(size_t)r * dim + e];
    }
    CHECK(std::fabs(s2 - 1.0) < 1e-5 && std::fabs(f2 - 1.0) < 1e-5);
  }
}

int main() {
  argument_checks();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    device_checks();
    mutate_checks();
    std::printf("host_check: argument + device checks, %d failure(s)\n", failures);
  } else {
    (void)hipGetLastError();
    std::printf("host_check: argument checks (no HIP device), %d failure(s)\n", failures);
  }
  return failures ? 1 : 0;
}
