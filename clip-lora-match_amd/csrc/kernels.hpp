// Host-callable launchers of the gfx950 kernels in k_*.hip.
#pragma once
#include "clm_common.hpp"

namespace clm {

// ---------------------------------------------------------------- GEMM ------
// C[M,N] = A[M,K] . W[N,K]^T  (both operands K-contiguous, nn.Linear layout),
// bf16 or fp16 operands, fp32 accumulate, fused epilogue. K % 64 == 0, or K % 64 == 32 (gemm_kernel
// configs 0-7 without split-K, and gemm_attn): every operand row must then be readable (and finite)
// to round_up(K, 64) -- the last K-step's DMA moves 64 columns, its MFMAs use the first 32.
enum Epi {
  EPI_STORE = 0,  // out16[m,n] = acc + bias[n]
  EPI_GELU = 1,   // out16[m,n] = quick_gelu(acc + bias[n])
  EPI_RESID = 2,  // outf[m,n] += acc + bias[n]            (fp32 residual stream)
  EPI_PATCH = 3,  // outf[b*(G+1)+1+p, n] = acc + aux[(1+p)*aux_ld + n], m = b*G+p, G = group >= 1;
                  // no bias: gemm_cfg refuses one (hipErrorInvalidValue), as it does a null aux
  EPI_SCORE = 4,  // outf[m,n] = acc * rscale[m] * cscale[n]  (cosine scores)
  EPI_FILTER = 5,  // s = acc*rscale[m]*cscale[n]; if s >= theta[m]: append (s, base+n) to row m's
                   // candidate list (atomic slot in cnt[m], capacity cap)
  EPI_RANK = 6,    // s as above against the row's target score t = theta[m]: s > t + rank_margin is
                   // counted into above[m]; otherwise s >= t - rank_margin appends base+n to row m's
                   // band list cand_i (slot from cnt[m], capacity cap). fp16, configs 1 and 8-11 only
  EPI_LSE = 7,     // s as above against the row's head floor theta[m]: s >= theta - rank_margin appends
                   // base+n to row m's band list (cnt / cand_i / cap as EPI_RANK); every other s adds
                   // exp2((s - theta) * lse_c) to the wave's partial lse_part[m * lse_ld + slot], slot =
                   // (column tile) * (wave columns of the config) + wave column < lse_slots(N): every
                   // slot a config uses is written once per live row, the others keep the caller's
                   // zeros. fp16, configs 1 and 8-11 only
  EPI_FILTER_MASK = 8,    // EPI_FILTER over the rows a bitset allows: column n is tested only where
                          // bit n & 31 of mask[n >> 5] is set (bits at or past N clear:
                          // mask_prepare). fp16, configs 1 and 8-11 only
  EPI_FILTER_KEYS = 9,    // EPI_FILTER with one open test per (row, column): column n is tested for row m
                          // only where klo[m] <= keys[n] <= khi[m] (a row with klo > khi lists nothing).
                          // fp16, configs 1 and 8-11 only
  EPI_SOFTW = 10          // softmax weights (clm_index_softmax_grad): s as above, x = s * lse_c (lse_c = scale *
                          // log2 e as in EPI_LSE); out16[m,n] = fp16(min(exp2(x - theta[m]) + exp2(x - bias[n]),
                          // 65504)): theta = the per-row offsets (theta_ld apart), bias = the per-column offsets
                          // (16-byte aligned: a lane loads its 4 at once, as it does keys), the second term
                          // absent when bias is null (the caller folds log2 of the weights and the scaling
                          // exponent p into the offsets); out as u16 [M, ldo]. fp16, configs 0 and 1 only
};
// upper bound, over the configs EPI_LSE runs on, of the slab slots per row (wave column extents are
// 64, 96 or 128 index rows)
inline int64_t lse_slots(int64_t N) { return N / 64 + 4; }
constexpr bool epi_stores16(int e) { return e == EPI_STORE || e == EPI_GELU; }
constexpr bool epi_gelu(int e) { return e == EPI_GELU; }
// the index passes' selecting epilogues: they compare each score with theta[m] and append / count / sum
constexpr bool epi_selects(int e) {
  return e == EPI_FILTER || e == EPI_FILTER_MASK || e == EPI_FILTER_KEYS || e == EPI_RANK || e == EPI_LSE;
}

struct GemmArgs {
  const u16* A; int64_t lda;
  const u16* W; int64_t ldw;
  int M, N, K;
  void* out; int64_t ldo;
  const float* bias;
  const float* aux; int64_t aux_ld; int group;
  const float* rscale; const float* cscale;
  // EPI_FILTER
  const float* theta; int64_t theta_ld; int* cnt; float* cand_s; int64_t* cand_i; int cap; int64_t base;
  // optional: order keys {min, max} of cscale[0, N) (value_bounds); lets a wave whose largest
  // accumulator cannot reach any of its rows' thresholds skip the per-element filter
  const unsigned* cbound;
  // EPI_RANK (with theta = the target scores, cnt / cand_i / cap / base / cbound as EPI_FILTER)
  unsigned* above; float rank_margin;
  int m_fastest;   // tile order: 1 = consecutive workgroups walk M (share one W tile)
  // split-K (gemm_kernel configs only, EPI_SCORE as the fp32 partial store): ksplit > 1 cuts K
  // into ksplit equal slices; slice s of every tile writes out + s * split_stride
  int ksplit; int64_t split_stride;
  // EPI_SCORE: 1 = store the scores as fp16 rounded toward -inf (f16_down: never above the fp32
  // score, so a k-th largest taken over them bounds the fp32 one from below), out as u16 [M, ldo];
  // 2 (gemm_kernel config 1 only, N % 256 == 0) = one fp16 (rounded down) per 4 consecutive
  // columns, their maximum, out as u16 [M, ldo >= N / 4] in a per-tile permuted column order
  int out16;
  // varlen rows (packed text tower): if set, the row count is *m_dev (device-resident, <= M, which
  // sizes the grid), so a captured graph replays with data-dependent row counts
  const int* m_dev;
  int debug;       // diagnostics only: 1 = skip the epilogue (accumulators kept live), 2 = drop its
                   // stores, 4 = one tile per workgroup (non-persistent grid)
  // EPI_LSE (with theta = the head floors, rank_margin, cnt / cand_i / cap / base as EPI_RANK)
  float* lse_part; int64_t lse_ld; float lse_c;
  // EPI_FILTER_MASK (with the EPI_FILTER fields): ceil(N / 32) words, read by that epilogue only
  const uint32_t* mask;
  // EPI_FILTER_KEYS (with the EPI_FILTER fields): keys [N], one per column (16-byte aligned: the
  // vector epilogue loads a lane's 4 at once); klo / khi [M], the row's inclusive key range
  const int32_t* keys; const int32_t* klo; const int32_t* khi;
};

hipError_t gemm(bool bf16, int epi, const GemmArgs& g, hipStream_t s);
// Few-row residual GEMM (the pruned last layer: M = pooled rows): out[m,n] += acc + bias with K cut
// into `slices` (deterministic: the fp32 partials [slices][M][N] go to ws and are summed in slice
// order by one reduce kernel, so a row's result does not depend on M). slices must divide K / 64.
hipError_t gemm_splitk_resid(bool bf16, const GemmArgs& g, int slices, float* ws, hipStream_t s);
// fp32 workspace bytes gemm_splitk_resid needs
inline size_t gemm_splitk_ws_bytes(int M, int N, int slices) { return (size_t)slices * M * N * 4; }
// explicit tile configuration (config < 0: heuristic); configs: k_gemm.hip launch_id.
// GEMM_CFG_SPLITK: the 128 x 64 tile (4 waves), for few-row GEMMs (the pooled last layer)
constexpr int GEMM_CFG_SPLITK = 2;
// GEMM_CFG_SKINNY: 64 x 64 tiles (4 waves), for N <= 64 (the unmerged-LoRA down-projections): twice
// the workgroups of 128 x 64 over the same rows
constexpr int GEMM_CFG_SKINNY = 12;
hipError_t gemm_cfg(bool bf16, int epi, int config, const GemmArgs& g, hipStream_t s);
int gemm_num_configs();
// host-side hint for the tile heuristic of the calling thread: true while two towers are being
// launched on concurrent streams (clm_encode_pair). Then the RESID / PATCH GEMMs keep the
// 192x128 / 128x192 tiles, whose single round leaves ~20 % of the workgroup slots to the
// other stream; alone, the slot-filling 160x128 tiles are faster (profiles/r02_v4_gemm_160x128.txt)
void gemm_set_concurrent(bool on);

// ----------------------------------------------------------- row ops -------
// LayerNorm over rows of a fp32 matrix, one wave per row.
//   mode 0: x = src rows                         (src = h)
//   mode 1: x = tok[ids[r]] + pos[r % L]         (text embedding gather), h written
// If g2 != null: h_out = LN(x; g1,b1) is written to hf (fp32) and y = LN(h_out; g2,b2)
// else: (mode 1 writes hf = x) y = LN(x; g1,b1).
// y (compute dtype) gets row stride ldy.
struct LnArgs {
  int mode;
  const float* src; int64_t lds;       // mode 0 source rows
  const int32_t* ids; const float* tok; const float* pos; int L;   // mode 1
  float* hf; int64_t ldh;              // fp32 output rows (may alias src)
  const float* g1; const float* b1;
  const float* g2; const float* b2;
  u16* y; int64_t ldy;
  int M, d; float eps;
  // varlen rows (packed text tower): rows r < *m_dev only (M sizes the grid); mode 1 reads token
  // rowmap[r] = b * L + position of the padded [B, L] ids instead of r
  const int* m_dev; const int* rowmap;
};
hipError_t layernorm(bool bf16, const LnArgs& a, hipStream_t s);

// shortest-edge bicubic resize + centre crop (k_image.hip), PIL / CLIPImageProcessor arithmetic.
// Per image: source HWC RGB bytes at src + src_off (row stride 3 W); the crop needs source rows
// [r0, r0 + rows), whose horizontally resampled S columns go to tmp + tmp_off ([rows][S][3]).
// coef + coef_off holds int32 xmin[S] | xn[S] | ymin[S] (relative to r0) | yn[S] | xk[S][kh] |
// yk[S][kv] (22-bit fixed-point taps).
struct ResizeDesc {
  int64_t src_off;
  int64_t tmp_off;
  int32_t W, r0, rows, kh, kv, coef_off;
};
hipError_t resize_crop(const uint8_t* src, const ResizeDesc* desc, int n, int S, int max_rows,
                       const int32_t* coef, uint8_t* tmp, uint8_t* out, hipStream_t s);

// n synthetic uint8 [S, S, 3] images, image i's bytes a function of (seed, row0 + i) only
// (S * S * 3 % 16 == 0; out 16-B aligned)
hipError_t synth_images(uint64_t seed, int64_t row0, int n, int S, uint8_t* out, hipStream_t s);

// patchify + (u8 rescale/normalise via lut | f32 copy) -> P[B*G*G, Kp] (compute dtype)
hipError_t patchify(bool bf16, const void* pix, int layout, int B, int S, int p, int C,
                    const float* lut /*[C*256]*/, u16* P, int Kp, hipStream_t s);

// h[b*T + 0, :] = cls + pos[0]
hipError_t write_cls(float* h, int64_t ldh, int B, int T, int d, const float* cls,
                     const float* pos, hipStream_t s);

// pooled row -> LN -> projection (fp32, projT [d, D]) -> optional L2 norm -> out
//   ids == null: row b*T (CLS); else row b*T + (first eos in ids[b]) (argmax if eos==2)
//   tmp: [B, D] fp32 workspace
// Last-layer pruning: hc[b] = h[b*T + prow_b], Oc[b][:d] = O[b*T + prow_b][:d], prow_b the
// pooled row (0, or the first EOS of ids).
// offs (varlen packed text rows, see text_plan): item b's pooled row is offs[b + 1] - 1 (its last
// live row, the first EOS) instead of b * T + pooled_row(ids)
hipError_t gather_pooled(const float* h, int64_t ldh, const u16* O, int64_t ldo, int B, int T, int d,
                         const int32_t* ids, int eos, float* hc, u16* Oc, int64_t ldoc, hipStream_t s,
                         const int* offs = nullptr);
hipError_t pool_project(const float* h, int64_t ldh, int B, int T, int d, const int32_t* ids,
                        int eos, const float* g, const float* bta, float eps, const float* projT,
                        int D, float* tmp, void* out, int out_dtype, int normalize, hipStream_t s,
                        const int* offs = nullptr);
// Varlen text plan (causal text tower, CLIPTextTransformer pools the first EOS row: rows after it
// cannot reach the pooled output). Per caption b of ids [B, L]: lens[b] = pooled row + 1 live
// rows, offs[b] = their exclusive prefix sum (offs[B] = total), rowmap[offs[b] + p] = b * L + p,
// the fused-attention tiles (whole captions, <= 256 rows each; tiles[t] = first caption |
// captions << 16) and counts = {live rows, tiles}. Three launches (lengths: a wave per caption;
// prefix / tiles: one workgroup; row map: a workgroup per 16 captions); B <= 4096.
hipError_t text_plan(const int32_t* ids, int B, int L, int eos, int* lens, int* offs, int* rowmap, int* tiles,
                     int* counts, hipStream_t s);

// ----------------------------------------------------------- attention -----
// qkv [B*T, 3d] (q pre-scaled by head_dim^-0.5), out [B*T, ldo] compute dtype.
// q_log2e: q carries log2(e) as well (the scores arrive in the log2 domain); valid only where
// attention_folds_log2e(bf16, causal, T) -- the kernel chosen for that shape takes that form
// (k_attn.hip attn_long_dma_kernel<true, true>: bf16, non-causal, T > 128) -- else
// hipErrorInvalidValue. The engine folds log2 e into the q_proj weights of such towers.
bool attention_folds_log2e(bool bf16, bool causal, int T);
hipError_t attention(bool bf16, bool causal, const u16* qkv, int64_t ldq, u16* out, int64_t ldo,
                     int B, int T, int H, int d, hipStream_t s, bool q_log2e = false);
// fused q/k/v projection + attention (k_gemm_attn.hip), T <= 128: out = attention(X . Wqkv^T +
// bias) without materialising QKV; bit-identical to gemm(EPI_STORE) + attention()
bool gemm_attn_supported(int T, int H, int d, int K);
hipError_t gemm_attn(bool bf16, bool causal, const u16* X, int64_t ldx, const u16* W, int64_t ldw, const float* bias,
                     u16* out, int64_t ldo, int B, int T, int H, int d, int K, hipStream_t s);
// the same over packed variable-length sequences (text_plan's lens / offs / tiles / counts; B
// sequences of <= L <= 128 rows, rows X[offs[b] ..]); grid sized for the worst case
hipError_t gemm_attn_varlen(bool bf16, bool causal, const u16* X, int64_t ldx, const u16* W, int64_t ldw,
                            const float* bias, u16* out, int64_t ldo, int B, int L, int H, int d, int K,
                            const int* lens, const int* offs, const int* tiles, const int* counts, hipStream_t s);
// one fused q/k/v + attention problem (gemm_attn / gemm_attn_varlen); lens == null: fixed length T
struct AttnProblem {
  const u16* X; int64_t ldx; const u16* W; int64_t ldw; const float* bias; u16* out; int64_t ldo;
  int B, T, H, d, K;
  const int *lens, *offs, *tiles, *counts;   // varlen (text_plan) or null
};

// ----------------------------------------------------------- search --------
// rows f32|f16 [n, dim] -> fp16 dst + fp32 inverse norms of the fp16-rounded rows
// (norm_src = 0) or of the source rows (norm_src = 1); norm_src = 2: dst = fp16(v / ||v||)
// and the inverse norms of those rounded unit rows
hipError_t rows_to_f16(const void* src, int src_dtype, int64_t n, int dim, u16* dst,
                       float* inv_norm, hipStream_t s, int norm_src);
// per-row top-k over scores [nq, C] (row stride lds): out sorted by (score desc,
// idx asc); idx = base + column.
hipError_t topk_rows(const float* scores, int64_t lds, int64_t nq, int64_t C, int k,
                     int64_t base, float* out_s, int64_t* out_i, int64_t ldo, hipStream_t s);
// top-k of any k (k > 1024, or candidate lists longer than one LDS sort): exact k-th key by radix
// select, the k composites collected, sorted (LDS runs + merge passes), emitted. idx == null: the
// global index of column j is base + j (any base); else idx[row * ldi + j] (< 0: an empty slot, never
// taken before a score; the values must be below 2^32: ties are ordered by their low 32 bits). Rows with fewer than k entries end in (-inf, -1). nq <= 65535; ws of
// topk_any_ws_bytes(nq, k) device bytes.
size_t topk_any_ws_bytes(int64_t nq, int k);
hipError_t topk_any(const float* scores, int64_t lds, const int64_t* idx, int64_t ldi, int64_t nq, int64_t C, int k,
                    int64_t base, float* out_s, int64_t* out_i, int64_t ldo, void* ws, hipStream_t s);
// cnt[q] = number of scores in row q [C] (row stride lds) that are >= th[q]
hipError_t count_ge(const float* scores, int64_t lds, int64_t nq, int64_t C, const float* th, int* cnt, hipStream_t s);
// the same over fp16 scores (GemmArgs::out16 score matrices)
hipError_t count_ge16(const u16* scores, int64_t lds, int64_t nq, int64_t C, const float* th, int* cnt, hipStream_t s);
hipError_t kth_thresholds16(const u16* scores, int64_t lds, int64_t nq, int64_t C, int k, float margin, float* th,
                            hipStream_t s);
// merge `parts` candidate lists per row: in [nq, parts*k_in] -> out [nq, k] by (score desc, index
// asc); indices are any int64 >= 0 (< 0: an empty slot)
hipError_t topk_merge(const float* in_s, const int64_t* in_i, int64_t nq, int parts, int k_in,
                      int k, float* out_s, int64_t* out_i, hipStream_t s);
// the first k entries of each list that open a new group (k_group.hip): list q = entries [q * ld, q * ld +
// ld) of in_s / in_i / in_g, or [offsets[q], offsets[q + 1]) with offsets; an entry with id < 0 (or gid <
// 0) is skipped, an entry is kept iff no earlier position of its list has its gid. out_* [nq, k] = the
// first k kept entries in list order, then (-inf, -1, -1); out_found [nq] = how many were written.
// 1 <= k <= 1024; a pure function of the lists.
hipError_t topk_distinct(const float* in_s, const int64_t* in_i, const int64_t* in_g, const int64_t* offsets,
                         int64_t ld, int64_t nq, int k, float* out_s, int64_t* out_i, int64_t* out_g, int* out_found,
                         hipStream_t s);
// out[0] (device) = the largest index of idx[0, n), 0 if none is >= 0
hipError_t max_index(const int64_t* idx, int64_t n, int64_t* out, hipStream_t s);
hipError_t l2_normalize_rows(float* rows, int64_t n, int dim, hipStream_t s);
hipError_t fuse_rows(const float* a, float wa, const float* b, float wb, int64_t n, int dim, float* out,
                     hipStream_t s);
// strided row sample: out[s] = rows[s * n / S] (fp16 rows + fp32 inverse norms)
hipError_t sample_rows(const u16* rows, const float* inv, int64_t n, int dim, int64_t S, u16* out_rows,
                       float* out_inv, hipStream_t s);
hipError_t f32_to_f16_rows(const float* src, int64_t n, int dim, u16* dst, hipStream_t s);
hipError_t f16_to_f32_rows(const u16* src, int64_t n, int dim, float* dst, hipStream_t s);

// exact (fp64) cosine re-scoring (k_search.hip): every path scores a (query, row) pair through
// one device routine, so the exact scores are bit-identical across paths
hipError_t query_norms(const float* q, int64_t nq, int dim, double* qn, hipStream_t s);
// out[qi, j] = fp32(cos64(q[qi], rows[j])), rows f32 or f16 [rn, dim]
hipError_t exact_scores(const float* q, const double* qn, int64_t nq, const void* rows, bool rows_f16, int64_t rn,
                        int dim, float* out, int64_t ldo, hipStream_t s);
// per query: candidates (fp16-pass score, global index) [nq, cap] with counts cnt[nq] -> keep
// those within `margin` of the k-th, re-score exactly, emit top k by (score desc, index asc);
// queries with cnt > cap are left untouched
hipError_t rescore_select(const float* cand_s, const int64_t* cand_i, const int* cnt, int cap, const float* q,
                          const double* qn, int dim, const void* rows, bool rows_f16, int64_t offset, float margin,
                          int64_t nq, int k, float* out_s, int64_t* out_i, hipStream_t s);
// overflowed lists: candidates [nq, cap] (global indices; cnt[q] <= cap) -> per chunk of
// RESCORE_WIDE_CHUNK candidates the top k by (exact score desc, index asc), part_s / part_i
// [nq, ceil(cap / chunk) * k] (-inf / -1 padded), merged by topk_merge; ceil(cap / chunk) * k <= 8192
constexpr int RESCORE_WIDE_CHUNK = 4096;
hipError_t rescore_wide(const int64_t* cand_i, const int* cnt, int64_t cap, const float* q, const double* qn, int dim,
                        const void* rows, bool rows_f16, int64_t offset, int64_t nq, int k, float* part_s,
                        int64_t* part_i, hipStream_t s);
// dst row j = src row idx[j] (scatter: dst row idx[j] = src row j), row_bytes per row
hipError_t gather_rows(const void* src, int64_t src_stride, const int64_t* idx, int64_t n, int64_t row_bytes,
                       void* dst, int64_t dst_stride, bool scatter, hipStream_t s);
// th[q] = ts[q * ld + k - 1] - margin
hipError_t filter_thresholds(const float* ts, int64_t ld, int64_t nq, int k, float margin, float* th, hipStream_t s);
// th[q] = (k-th largest of scores row q [C], duplicates counted) - margin, bit-identical to
// topk_rows + filter_thresholds; k <= 8, C >= k
hipError_t kth_thresholds(const float* scores, int64_t lds, int64_t nq, int64_t C, int k, float margin, float* th,
                          hipStream_t s);
// keys[0] / keys[1] = order key (float_key) of min / max over v[0, n); a NaN anywhere makes the
// decoded min or max NaN. keys: 2 device u32
hipError_t value_bounds(const float* v, int64_t n, unsigned* keys, hipStream_t s);
// small-batch search scan (k_search.hip scan16_kernel): nq <= 16 unit-rounded fp16 queries q16
// [nq, dim] (inverse norms qinv) against the fp16 index rows [N, dim] (inverse norms inv), one
// streaming pass: out [N, ldo] = fp16-pass scores (acc * qinv * inv), row-major with the queries
// of a row contiguous (ldo = 1, 2, 4, 8 or 16 >= nq), cmax [nq, nchunk] = each 256-row chunk's
// largest score (nchunk = ceil(N / 256)); dim % 64 == 0, 64 <= dim <= 1024
// wtop (optional) [nq, ldw]: wave w's 8 largest chunk maxima per query at columns 8 w .. 8 w + 7
// (-inf padded); scan16_waves gives the wave count W (ldw >= 8 W)
struct Scan16Args {
  const u16* rows; const float* inv; int64_t N; int dim;
  const u16* q16; const float* qinv; int nq;
  float* out; int64_t ldo;
  float* cmax; int64_t nchunk;
  float* wtop; int64_t ldw;
};
hipError_t scan16(const Scan16Args& a, hipStream_t s);
void scan16_shape(int dim, int* nw, int* depth);
int scan16_grid(int64_t nchunk, int nw, int cus);
int64_t scan16_waves(int64_t nchunk, int dim);
// append every (score, base + row) of column q of scores [C rows, ldq] (ldq a power of two, 1..16,
// >= nq) at or above th[q] to q's candidate list [cap] (cnt[q] counts them all)
hipError_t collect_ge(const float* scores, int ldq, int nq, int64_t C, const float* th, int* cnt, int cap, float* cs,
                      int64_t* ci, int64_t base, hipStream_t s);

// ----------------------------------------------------------- rank (k_rank.hip) ---
// The order of the search, (score desc, index asc) with NaN above every number: is (s, idx)
// ahead of the target (t, g)?
__host__ __device__ inline bool rank_ahead(float s, int64_t idx, float t, int64_t g) {
  const bool sn = s != s, tn = t != t;
  if (sn || tn) return sn && (!tn || idx < g);
  return s > t || (s == t && idx < g);
}
// t[q] = exact score of (q, row target[q] - offset): the routine of exact_scores / rescore_select
hipError_t target_scores(const float* q, const double* qn, int64_t nq, int dim, const void* rows, bool rows_f16,
                         int64_t offset, const int64_t* target, float* t, hipStream_t s);
// per query: the band list (global indices [nq, cap], cnt[q] entries; cnt[q] > cap marks an
// incomplete list, left untouched) re-scored exactly; out[q] (zeroed by the caller) += above32[q] +
// #{listed rows ahead of the target (t[q], g[q])}; plan: nq + 1 device ints of scratch (the work
// items' prefix sums); nq * ceil(cap / 64) < 2^31
hipError_t rank_rescore(const int64_t* band, const int* cnt, int64_t cap, const unsigned* above32, const float* q,
                        const double* qn, int dim, const void* rows, bool rows_f16, int64_t offset, const float* t,
                        const int64_t* g, int64_t nq, int* plan, int64_t* out, hipStream_t s);
// the same count over a window of exact scores [nq, C] (row stride lds), column j being the global
// row base + j: above[q] += #{j : (scores[q, j], base + j) ahead of (t[q], g[q])}
hipError_t count_rank(const float* scores, int64_t lds, int64_t nq, int64_t C, int64_t base, const float* t,
                      const int64_t* g, int64_t* above, hipStream_t s);
// out[q] = in[q] + 1
hipError_t rank_from_above(const int64_t* above, int64_t nq, int64_t* rank, hipStream_t s);
// rank_rescore's item plan alone: every complete band list (cnt[q] <= cap) gets max(1, ceil(cnt[q] /
// PLAN_CHUNK)) items, plan[q] = their exclusive prefix sums, plan[nq] = the total
constexpr int PLAN_CHUNK = 64;
hipError_t rescore_plan(const int* cnt, int64_t cap, int64_t nq, int* plan, hipStream_t s);

// ----------------------------------------------------------- log-sum-exp (k_lse.hip) ---
// lse(q) = log sum_j exp(scale * s_j) over the exact scores s_j, in fp64.
// The exact route: state[q] = (running maximum M, sum of exp(scale * (s - M))) folded over windows
// of exact scores; lse_fold_init sets (-inf, 0), lse_fold adds the window scores [nq, C] (row
// stride lds), lse_fold_finish writes lse = scale * M + log(sum) and err = 0 (err may be null).
hipError_t lse_fold_init(double2* state, int64_t nq, hipStream_t s);
hipError_t lse_fold(const float* scores, int64_t lds, int64_t nq, int64_t C, double scale, double2* state,
                    hipStream_t s);
hipError_t lse_fold_finish(const double2* state, int64_t nq, double scale, double* lse, float* err, hipStream_t s);
// The reference route (clm_index_lse64): lse_scores64 is exact_scores without the rounding to fp32
// (out [nq, rn] fp64, row stride ldo); lse_fold64 folds such a window of local rows [r0, r0 + C) and,
// with target / pair given, copies the score of local row target[q] - base into pair[q] when the
// window holds it (pair is otherwise left as it is).
hipError_t lse_scores64(const float* q, const double* qn, int64_t nq, const void* rows, bool rows_f16, int64_t rn,
                        int dim, double* out, int64_t ldo, hipStream_t s);
hipError_t lse_fold64(const double* scores, int64_t lds, int64_t nq, int64_t C, double scale, double2* state,
                      const int64_t* target, int64_t base, int64_t r0, double* pair, hipStream_t s);
// The fast route after the EPI_LSE GEMM. lse_band_scores: the exact score of every listed band row
// (complete lists only) into band_s [nq, cap], beside its index (rescore_plan's items; plan: nq + 1
// ints). lse_finish, per query: head = the band rows' exp(scale * (s - M)) summed in 2^-k fixed
// point (order-free), tail = the slab's `slots` partials summed in slot order,
//   lse = scale * M + log(head + tail * exp(scale * (theta - M))),   err >= |lse - exact route's|
// (DESIGN.md derives err from E = the fp16 pass's score error bound and N = the index rows);
// redo[q] = 1 and lse / err untouched where the exact route must serve the query: band overflowed or
// empty, non-finite theta, tail or band score, or an err that is not finite.
hipError_t lse_band_scores(const int64_t* band, const int* cnt, int64_t cap, const float* q, const double* qn, int dim,
                           const void* rows, bool rows_f16, int64_t offset, int64_t nq, int* plan, float* band_s,
                           hipStream_t s);
hipError_t lse_finish(const float* band_s, const int* cnt, int64_t cap, const float* part, int64_t slots,
                      const float* theta, double scale, double E, int64_t N, int64_t nq, double* lse, float* err,
                      int* redo, hipStream_t s);

// ----------------------------------------------------------- softmax gradients (k_grad.hip) ---
// dst[c, r] = fp16(float(src[r, c]) * s[r]) for r < rows, c < cols (s null: 1), src fp16 [rows, lds], dst
// fp16 [cols, ldd]; the padding columns rows .. round_up(rows, 64) - 1 of every dst row are written as
// zeros (ldd >= round_up(rows, 64)): dst is the K-contiguous operand of a GEMM whose K is `rows`.
hipError_t transpose16(const u16* src, int64_t lds, int64_t rows, int64_t cols, const float* s, u16* dst, int64_t ldd,
                       hipStream_t st);
// EPI_SOFTW's offsets: out[i] = fp32(lse[i] * log2(e) - sub) for i < n (sub = log2 of the weight + p)
hipError_t softw_offsets(const double* lse, int64_t n, double sub, float* out, hipStream_t st);
// v[i] *= f for i < n
hipError_t scale_f32(float* v, int64_t n, float f, hipStream_t st);

// ----------------------------------------------------------- threshold search (k_range.hip) ---
// The result of query q under threshold tau[q]: the rows (s, id) with rank_ahead(s, id, tau[q],
// INT64_MAX) -- s >= tau, NaN above every number -- as 64-bit composites (float_key(s) << 32 |
// 0xFFFFFFFF - local row; descending composites = score desc, id asc) in one segment per query.
// A work item of the sort / merge / decode launches, cut by the host from the segment lengths:
//   range_sort_runs: the run of n composites (2 <= n <= RANGE_RUN) at `start`;
//   range_merge:     elements [aux, aux + RANGE_MERGE_CHUNK) of the segment of n composites at `start`;
//   range_decode:    n composites at `start` -> entries [aux, aux + n) of the result.
struct RangeItem { int64_t start, aux, n; };
constexpr int RANGE_RUN = 8192, RANGE_MERGE_CHUNK = 1024, RANGE_GRID = 4096;
// keep / count over the re-scored candidate lists (band [nq, cap] global ids beside their exact scores
// band_s, cnt[q] entries, complete lists only; plan: rescore_plan's items, as lse_band_scores leaves
// them): len[q] (zeroed by the caller) += the listed rows that pass
hipError_t range_keep_count(const float* band_s, const int64_t* band, const int* cnt, int64_t cap, const int* plan,
                            const float* tau, int64_t nq, int* len, hipStream_t s);
// emit: those rows' composites (local row = id - offset) into seg[src[q] ..), len[q] of them, slots from
// cursor[q] (zeroed by the caller; integer atomics: the order inside a segment is not defined)
hipError_t range_emit(const float* band_s, const int64_t* band, const int* cnt, int64_t cap, const int* plan,
                      const float* tau, int64_t offset, int64_t nq, int* len, int* cursor, const int64_t* src,
                      uint64_t* seg, hipStream_t s);
// window collect (the exact route): the passing entries of a window of exact scores [nq, C] (row
// stride lds; column j = local row r0 + j, r0 + C <= 2^32 - 1) appended at seg[cursor[q]++], never at
// or past end[q]
hipError_t range_collect(const float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const float* tau,
                         int64_t* cursor, const int64_t* end, uint64_t* seg, hipStream_t s);
// segmented sort, descending: every item's run sorted in LDS by one workgroup (longest: the largest
// item's n), then for the segments longer than one run log2 passes of range_merge with L = RANGE_RUN,
// 2 RANGE_RUN, ... between two buffers (a pass moves every element of its items' segments to dst)
hipError_t range_sort_runs(uint64_t* seg, const RangeItem* items, int64_t nitems, int64_t longest, hipStream_t s);
hipError_t range_merge(const uint64_t* src, uint64_t* dst, const RangeItem* items, int64_t nitems, int64_t L,
                       hipStream_t s);
// composites -> (exact score, global id = offset + local row)
hipError_t range_decode(const uint64_t* seg, const RangeItem* items, int64_t nitems, int64_t offset, float* out_s,
                        int64_t* out_i, hipStream_t s);

// ----------------------------------------------------------- index mutation (k_mutate.hip) ---
// Whole-row movers over the index's three arrays (fp16 rows, fp32 rows or null, fp32 inverse
// norms), 16-byte loads and stores. gather_rows: the rows of [s0, s0 + rows) that are not in rem
// (sorted, distinct, all inside that range; m of them) packed in order into out16 / out32 / out_inv
// (slot 0 = the first survivor). scatter_rows: staged row i -> row ids[i] - offset (ids distinct
// and inside the index: the caller's check).
hipError_t gather_rows(const u16* rows16, const float* rows32, const float* inv, int64_t s0, int64_t rows, int dim,
                       const int64_t* rem, int64_t m, u16* out16, float* out32, float* out_inv, hipStream_t s);
hipError_t scatter_rows(const u16* src16, const float* src32, const float* src_inv, const int64_t* ids, int64_t offset,
                        int64_t n, int dim, u16* rows16, float* rows32, float* inv, hipStream_t s);

// threads that move one row in the whole-row movers (k_mutate.hip, k_mask.hip): the largest power of
// two <= min(64, 16-byte units of one fp16 row)
inline int group_of(int dim) {
  int g = 8;
  while (g < 64 && g * 2 <= dim / 8) g *= 2;
  return g;
}

// ----------------------------------------------------------- filtered search (k_mask.hip) ---
// A mask: ceil(N / 32) little-endian u32 words, bit j & 31 of word j >> 5 set iff local row j is
// allowed. A block of the mask kernels covers MASK_BLOCK_WORDS words (MASK_BLOCK_WORDS * 32 rows).
constexpr int MASK_BLOCK_WORDS = 256;
inline int64_t mask_words(int64_t N) { return (N + 31) / 32; }
inline int64_t mask_blocks(int64_t N) { return (mask_words(N) + MASK_BLOCK_WORDS - 1) / MASK_BLOCK_WORDS; }
// dst = the caller's words with the bits at or past N cleared; bcnt[b] = block b's set bits
hipError_t mask_prepare(const uint32_t* src, int64_t N, uint32_t* dst, uint32_t* bcnt, hipStream_t s);
// boff[b] = the exclusive prefix sum of bcnt over the mask_blocks(N) blocks, boff[blocks] = the total
// P (int64: one workgroup, fixed order)
hipError_t mask_scan(const uint32_t* bcnt, int64_t nblocks, int64_t* boff, hipStream_t s);
// list[boff[b] ..) = block b's set local rows, ascending: the whole list is the allowed rows in order
// (prefix sums inside the block, no atomics)
hipError_t mask_compact(const uint32_t* words, int64_t N, const int64_t* boff, uint32_t* list, hipStream_t s);
// scores [nq, C] (row stride lds), column j = local row r0 + j: -inf where that row's bit is clear; an
// allowed NaN gets its sign bit cleared (the top-k kernels order scores by their bit pattern)
hipError_t mask_fill(float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const uint32_t* words,
                     hipStream_t s);
// result fix-up over n (score, id) entries. list != null: ids are positions of the allowed list, id =
// offset + list[id]; list == null: ids are kept. An id < 0 stays -1 and an entry whose score is -inf
// (the fill value: an exact cosine is finite or NaN) becomes -1.
hipError_t map_ids(const float* scores, int64_t* ids, int64_t n, const uint32_t* list, int64_t offset, hipStream_t s);
// out row i = row list[floor(i * P / S)] of the index's arrays (S <= P; S == P: every listed row in
// order): fp16 rows, inverse norms, and the fp32 rows where rows32 / out32 are given; dim % 8 == 0
hipError_t mask_gather(const u16* rows16, const float* rows32, const float* inv, int dim, const uint32_t* list,
                       int64_t P, int64_t S, u16* out16, float* out32, float* out_inv, hipStream_t s);
// ---- keyed search (k_keys.hip): one int32 key per index row, one inclusive key range per query
// mask_fill with the per-query predicate: scores [nq, C] (row stride lds), column j = local row
// r0 + j: -inf where keys[r0 + j] lies outside [lo[y], hi[y]] of query y; a NaN inside gets its sign
// bit cleared
hipError_t key_fill(float* scores, int64_t lds, int64_t nq, int64_t C, int64_t r0, const int32_t* keys,
                    const int32_t* lo, const int32_t* hi, hipStream_t s);
// the strided sample: out row i = row floor(i * N / S) of the index's arrays (S <= N): fp16 row,
// inverse norm and key; dim % 8 == 0
hipError_t key_sample(const u16* rows16, const float* inv, const int32_t* keys, int dim, int64_t N, int64_t S,
                      u16* out16, float* out_inv, int32_t* out_keys, hipStream_t s);
// out[i] = value for i < n (floats)
hipError_t fill_f32(float* out, int64_t n, float value, hipStream_t s);

__host__ __device__ inline unsigned float_key(float f) {
  const unsigned b = __builtin_bit_cast(unsigned, f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float key_float(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

}  // namespace clm
