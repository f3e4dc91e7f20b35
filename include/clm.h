/*
 * clm.h -- C-ABI of libclm.so, the MI355X (gfx950) CLIP+LoRA encode and
 * cosine top-k library. Plain pointers and sizes only; no torch types.
 *
 * Each entry point replaces one reference interface (file:line into
 * youngalip/clip-lora-match, /root/reference):
 *
 *   clm_ctx_create/_destroy   models/clip_model.py:37-82  load_clip_model
 *                              (device/dtype from _get_device :23-28, _get_dtype :31-34)
 *   clm_load_tensor            CLIPModel.from_pretrained (clip_model.py:59) and
 *                              PeftModel.from_pretrained (clip_model.py:78): tensors by
 *                              their transformers / PEFT state-dict names
 *   clm_finalize               model.eval() (clip_model.py:81): fuse q/k/v, merge or
 *                              pack LoRA (models/lora_adapter.py:21-43 scaling alpha/r)
 *   clm_encode_image           encode_image clip_model.py:89-118,
 *                              embed_images_batch src/embedding/embed_image.py:57-98
 *   clm_encode_text            encode_text clip_model.py:121-150,
 *                              embed_text src/embedding/embed_text.py:11-60
 *   clm_index_create/_append   TextSearchIndex.__init__ src/embedding/search.py:24-68
 *                              (rows re-normalised at load, :68)
 *   clm_index_search           TextSearchIndex.search_with_embedding search.py:70-115,
 *                              top_k_similar src/embedding/similarity.py:36-58
 *   clm_index_rank,            (new) the rank of each query's ground-truth row in the whole index,
 *   clm_index_count_above      what scripts/evaluate_model.py:60-103 (compute_recall_at_k / _mrr /
 *                              _map) reads off argsort positions of a full [nq, N] matrix
 *   clm_index_lse              (new) log sum_j exp(scale * score_j) per query over the whole index:
 *                              the row reduction of compute_clip_contrastive_loss
 *                              (scripts/train_lora.py:83-108, evaluated :213-241) and the
 *                              normaliser of softmax match probabilities, without a [nq, N] matrix
 *   clm_index_lse64            (new) the same reduction and the pair scores on unrounded fp64
 *                              cosines: that function on float64 tensors
 *   clm_index_softmax_grad     (new) the softmax-weighted sums over the index, both ways: what
 *                              loss.backward() of that function (scripts/train_lora.py:83-108 as
 *                              called from its training loop) delivers to the embeddings, without the
 *                              [N, N] logits
 *   clm_index_search_above     (new) every index row at or above a cosine, exactly: the relevant set
 *                              of scripts/evaluate.py:141-269 (evaluate_single_query: cosine >= 0.7),
 *                              "which reports describe the same item", near-duplicate listing
 *   clm_cosine_scores          cosine_similarity similarity.py:10-33
 *   clm_topk_merge             (new) merge of per-shard top-k lists for the
 *                              8-GPU sharded search
 *   clm_topk_distinct          (new) the first k entries of an ordered list that open a new group:
 *                              "the k best ITEMS" where an item owns several rows (the finder
 *                              stores a photo and a description per item; a CSV index lists one
 *                              image_path under several captions)
 *   clm_l2_normalize           v / ||v||_2 (clip_model.py:116,148; search.py:68,93)
 *   clm_index_remove/_update   (new) the second half of the lost-and-found lifecycle: an item handed
 *                              back stops matching, a corrected description replaces its row --
 *                              in place in HBM instead of FinderService's reload + re-save of
 *                              the whole index (finder_service.py:171-185)
 *   clm_index_export/_import   the index's .pt persistence (search.py:29-36,68;
 *                              finder_service.py:93-103) as a raw fp16 shard
 *   clm_resize_crop            CLIPProcessor's image resize + centre crop for inputs of any
 *                              size (clip_model.py:105-110, embed_image.py:36-41;
 *                              config/clip_config.yaml:7-9)
 *
 * Conventions
 *   - return 0 (CLM_OK) on success, a negative CLM_E_* code on error;
 *     clm_last_error() returns a thread-local message for the last failure.
 *   - pointers may be device (hipMalloc / torch cuda) or host memory; host
 *     buffers are staged through the context's device workspace.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream). Calls are
 *     asynchronous w.r.t. the host only when every buffer is device memory.
 *     Device inputs are read and device outputs written in stream order on
 *     `stream`: work queued on it before the call is seen, work queued after
 *     sees the results, and the caller needs no other synchronisation (a
 *     non-blocking stream included; tests/test_gpu_stream_order.py).
 *   - one context per device; calls on one context must be externally
 *     serialised; different contexts are independent.
 */
#ifndef CLM_H
#define CLM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CLM_OK = 0,
  CLM_E_ARG = -1,     /* bad argument / shape (Python: ValueError)         */
  CLM_E_OOM = -2,     /* device allocation failed                          */
  CLM_E_HIP = -3,     /* HIP runtime error                                 */
  CLM_E_STATE = -4,   /* call out of order (e.g. encode before finalize)   */
  CLM_E_MISSING = -5  /* a required tensor was never loaded                */
};

enum { CLM_F32 = 0, CLM_F16 = 1, CLM_BF16 = 2, CLM_U8 = 3, CLM_I32 = 4, CLM_I64 = 5 };

/* pixel layouts for clm_encode_image */
enum {
  CLM_PIX_U8_HWC = 0,  /* raw uint8 [n, S, S, 3]; rescale+normalise fused in-kernel */
  CLM_PIX_F32_CHW = 1  /* CLIPProcessor pixel_values float32 [n, 3, S, S]          */
};

/* LoRA target bits (PEFT target_modules, lora_config.yaml:3-7) */
enum {
  CLM_LORA_Q = 1, CLM_LORA_K = 2, CLM_LORA_V = 4, CLM_LORA_OUT = 8,
  CLM_LORA_FC1 = 16, CLM_LORA_FC2 = 32
};

enum { CLM_LORA_MERGED = 0, CLM_LORA_UNMERGED = 1 };
/* compute_dtype CLM_COMPUTE_MIXED: bf16 operands in the vision tower, fp16 in the text tower. The
 * text tower carries the bf16 error (64 + 64 parity set vs the fp32 reference: txt.txt scores 1.7e-3
 * in bf16, 2.8e-4 in fp16; img.img 4.8e-4 / 6.8e-5 -- profiles/r04_v2_bf16_tower_bisect.jsonl), so
 * this is the bf16 assignment that meets the path's 1e-3 score bar. */
enum { CLM_COMPUTE_MIXED = 0x12 };

typedef struct clm_ctx clm_ctx;
typedef struct clm_index clm_index;

typedef struct {
  int32_t hidden, layers, heads, mlp;
} clm_tower_desc;

typedef struct {
  clm_tower_desc vision, text;
  int32_t patch, image_size, channels;
  int32_t vocab, max_pos, proj_dim;
  int32_t eos_token_id;       /* 2 selects the legacy argmax(ids) pooling rule */
  float ln_eps;
  int32_t lora_r;             /* 0 = no LoRA */
  float lora_alpha;
  uint32_t lora_targets;      /* CLM_LORA_* bitmask */
  int32_t lora_mode;          /* CLM_LORA_MERGED | CLM_LORA_UNMERGED (K-extension) */
  int32_t compute_dtype;      /* CLM_BF16 | CLM_F16 | CLM_COMPUTE_MIXED: GEMM/attention operand type */
  int32_t max_batch;          /* workspace is sized for this many images/captions */
  float mean[3], std[3];      /* preprocess.normalize (clip_config.yaml:10-12) */
} clm_model_desc;

int clm_ctx_create(int hip_device, const clm_model_desc* desc, clm_ctx** out);
int clm_ctx_destroy(clm_ctx* ctx);

/* host tensor by transformers/PEFT name; dtype CLM_F32|CLM_F16|CLM_BF16.
 * Copied (as float32) into the context; device upload happens in finalize. */
int clm_load_tensor(clm_ctx* ctx, const char* name, const void* host_ptr, int dtype,
                    const int64_t* shape, int ndim);
int clm_finalize(clm_ctx* ctx);
/* re-finalize with LoRA on (enabled != 0) or off (the base model); tensors are kept */
int clm_set_lora_enabled(clm_ctx* ctx, int enabled);
/* attach (or replace) the LoRA configuration of a context in place -- PEFT get_peft_model on
 * the loaded model (models/lora_adapter.py:46-56): r (0 = none), alpha, CLM_LORA_* targets.
 * Load the adapter tensors (base_model.model.<path>.lora_{A,B}.weight) next, then clm_finalize. */
int clm_set_lora(clm_ctx* ctx, int r, float alpha, uint32_t targets);

/* n images -> out [n, proj_dim] (CLM_F32 or CLM_F16); normalize != 0 => unit rows */
int clm_encode_image(clm_ctx* ctx, const void* pixels, int pix_layout, int n, void* out,
                     int out_dtype, int normalize, void* stream);
/* Shortest-edge BICUBIC resize to S + centre crop S x S of n uint8 RGB images of any size
 * (H, W >= 1), with PIL's 8-bit resampling arithmetic (the CLIPImageProcessor the reference runs):
 * out is uint8 [n, S, S, 3], bit-identical to PIL Image.resize + transformers center_crop, and
 * feeds clm_encode_image(CLM_PIX_U8_HWC). Image i is HWC RGB bytes at src + offs[i] with
 * hw[2 i] = H, hw[2 i + 1] = W (offs, hw: host arrays). src / out: host or device. Synchronous. */
int clm_resize_crop(int hip_device, const uint8_t* src, const int64_t* offs, const int32_t* hw, int n,
                    int S, uint8_t* out, void* stream);

/* Synthetic benchmark / test images (BASELINE configs[2]): out uint8 [n, S, S, 3] (device,
 * 16-B aligned; S * S * 3 % 16 == 0) where every byte of image i is a hash of (seed, row0 + i,
 * byte index) -- any shard / batch split of a global row range regenerates the same pixels. */
int clm_synth_images(int hip_device, uint64_t seed, int64_t row0, int n, int S, uint8_t* out, void* stream);

/* ids int32 [n, L] (L <= max_pos; each row holds an EOS) -> out [n, proj_dim] */
int clm_encode_text(clm_ctx* ctx, const int32_t* ids, int n, int L, void* out, int out_dtype,
                    int normalize, void* stream);

/* One image batch and one caption batch (each <= max_batch, device pointers) encoded
 * concurrently: each tower's batch is cut into S sub-batches, and the 2*S pieces run on
 * context-owned streams forked from / joined to `stream` with events.
 * flags & CLM_PAIR_GRAPH: the whole launch DAG is captured once per (pointers, shapes, S)
 * into a hipGraph and replayed on later calls. S = (flags >> CLM_PAIR_SPLIT_SHIFT) & 15,
 * clamped to [1, 4]; 0 = env CLM_PAIR_SPLIT, else 2 when a tower has >= 128 items, else 1.
 * Results are identical (bit for bit) to clm_encode_image + clm_encode_text. */
enum { CLM_PAIR_GRAPH = 1, CLM_PAIR_SPLIT_SHIFT = 8 };
int clm_encode_pair(clm_ctx* ctx, const void* pixels, int pix_layout, int n_img, const int32_t* ids,
                    int n_txt, int L, void* out_img, void* out_txt, int out_dtype, int normalize,
                    int flags, void* stream);
/* How the last clm_encode_pair ran: 0 = one stream per tower piece (the only path; round 5's
 * opt-in grouped launches measured 11 % slower and were removed), -1 = no call yet. */
int clm_pair_path(const clm_ctx* ctx);

/* GPU-resident cosine index (dim % 64 == 0, <= 65536; rows wider than 8192 are always searched by
 * the exact scan, MARGIN_MAX_DIM in capi_search.cpp). Scores are the EXACT cosine of the
 * caller's query and rows (fp64 arithmetic, rounded once to fp32): an fp16 MFMA pass bounds the
 * candidates, which are then re-scored against the rows as given. */
int clm_index_create(int hip_device, int64_t capacity, int dim, clm_index** out);
int clm_index_destroy(clm_index* idx);
/* rows [n, dim] CLM_F32|CLM_F16, host or device. Kept: fp16 MFMA operands (f32 rows normalised
 * then rounded; f16 rows as given) + fp32 inverse norms, and -- once any f32 rows arrive -- an
 * fp32 copy of the rows as given (f16 rows upcast into it), read by the exact re-score. */
int clm_index_append(clm_index* idx, const void* rows, int dtype, int64_t n, void* stream);
int64_t clm_index_size(const clm_index* idx);
int clm_index_reset(clm_index* idx);
/* index of row 0 in the global (all-shard) numbering, for multi-GPU shards: any value in
 * [0, 2^62] (one index holds fewer than 2^32 rows; its searches order equal scores by the local
 * row, so results are the offset-0 results plus the offset) */
int clm_index_set_offset(clm_index* idx, int64_t global_offset);
/* In-place mutation of the resident index. ids (host or device) are the numbers a search returns:
 * global ids, clm_index_set_offset's offset included. Everything is validated before anything
 * changes: a null index, a null pointer with n > 0, a negative n, an id outside
 * [offset, offset + size) or a dtype other than CLM_F32 / CLM_F16 is CLM_E_ARG and leaves the index
 * bit for bit as it was; n == 0 is a no-op. Both synchronise the stream.
 *   remove: ids in any order, a duplicate counts once. The survivors keep their order: a
 *           survivor's new number is its old one minus the number of removed rows below it.
 *           Rows below the first removed one are not touched; the capacity stays.
 *   update: row ids[i] becomes rows[i] [n, dim] (host or device) through exactly the conversion of
 *           clm_index_append (the first f32 rows start the fp32 copy); a duplicate id is CLM_E_ARG.
 * The result equals, bit for bit, an index built by appending the final rows in order. */
int clm_index_remove(clm_index* idx, const int64_t* ids, int64_t n_ids, void* stream);
int clm_index_update(clm_index* idx, const int64_t* ids, const void* rows, int dtype, int64_t n, void* stream);
/* copy rows [start, start+n) back as fp32 (host or device dst) */
int clm_index_read(clm_index* idx, int64_t start, int64_t n, float* dst, void* stream);
/* Shard persistence (TextSearchIndex.save_shard / load_shard; the reference persists its index
 * as a .pt, search.py:29-36 / finder_service.py:93-103): export copies rows [start, start+n) of
 * the index's internal state -- fp16 MFMA operands rows16 [n, dim], their fp32 inverse norms
 * inv [n] and, when rows32 != NULL, the fp32 rows the index keeps (CLM_E_STATE if it keeps none;
 * clm_index_has_f32 says) -- to host or device memory. import appends n rows in exactly that
 * form (no normalisation or rounding), so the reloaded index searches bit for bit as the saved
 * one. Both synchronous. */
int clm_index_has_f32(const clm_index* idx);
int clm_index_export(clm_index* idx, int64_t start, int64_t n, uint16_t* rows16, float* inv, float* rows32,
                     void* stream);
int clm_index_import(clm_index* idx, const uint16_t* rows16, const float* inv, const float* rows32, int64_t n,
                     void* stream);
/* q [nq, dim] CLM_F32|CLM_F16 (normalised in-kernel); k in [1, 1024];
 * out_scores [nq, k] f32 = exact cosines, out_idx [nq, k] i64 (+ global offset);
 * order: score desc, index asc (CPU torch.topk, search.py:98-99, leaves ties unordered);
 * slots past the index size are filled with (-inf, -1). Replaces the reference's fp32
 * sims = q_hat @ E_hat^T + topk (search.py:93-99) on the same rows. */
int clm_index_search(clm_index* idx, const void* q, int q_dtype, int64_t nq, int k,
                     float* out_scores, int64_t* out_idx, void* stream);

/* Exact retrieval ranks. "Exact score" s_j of row j for query q is the score of clm_index_search:
 * fp32(cos64(q, row j)) of the rows as the index keeps them (the fp32 rows when it keeps them, else
 * the fp16 rows), from the device routine every exact score of the library comes from. For a
 * target with score t (fp32) and global index g (row 0 is index `global_offset`):
 *
 *     above(q) = #{ rows j : s_j > t  or  (s_j == t and global_index(j) < g) }
 *     rank(q)  = 1 + above(q)
 *
 * -- the search order (score desc, index asc), so rank == r means that clm_index_search with any
 * k >= r returns the target at position r - 1. A NaN score sorts above every number (torch.topk's
 * order, and the exact scan's); NaNs tie with each other and are ordered by index.
 *
 * clm_index_count_above is the primitive: out_above[i] = above(q_i) over this index's rows for the
 * given (t_score[i], t_index[i]); t_index is any int64 (the target may live in another shard: the
 * counts of row shards add up to the whole index's). clm_index_rank takes target[i], a global id in
 * [offset, offset + size), computes t as the exact score of (q_i, that row), counts, and writes
 * out_rank[i] = rank and out_score[i] = t (out_score may be NULL). q [nq, dim] CLM_F32|CLM_F16;
 * every pointer host or device, as in clm_index_search. One fp16 MFMA pass counts the rows whose
 * fp16-pass score is clearly above t and lists those within a margin of it (the band), which are
 * re-scored exactly; no buffer grows with nq x size. band_cap <= 0: the default band capacity per
 * query, min(size, max(2048, size / 8)); > 0: its low bits (CLM_RANK_CAP_MASK) cap the band list
 * (0 = default) -- a query whose band is longer is served by the exact route, windows of exact
 * scores and the same count -- and CLM_RANK_EXACT sends every query that way, CLM_RANK_BAND keeps
 * the MFMA pass even for problems small enough for the exact route (both for tests: the results do
 * not depend on the route). CLM_E_ARG: a target outside the index, an empty index, a null pointer,
 * a dtype other than f32 / f16. */
enum { CLM_RANK_EXACT = 1 << 30, CLM_RANK_BAND = 1 << 29, CLM_RANK_CAP_MASK = (1 << 29) - 1 };
int clm_index_count_above(clm_index* idx, const void* q, int q_dtype, int64_t nq, const float* t_score,
                          const int64_t* t_index, int64_t* out_above, int band_cap, void* stream);
int clm_index_rank(clm_index* idx, const void* q, int q_dtype, int64_t nq, const int64_t* target,
                   int64_t* out_rank, float* out_score, int band_cap, void* stream);

/* Streaming log-sum-exp. With s_j the exact score of row j (as above),
 *
 *     lse(q) = log sum_j exp(scale * s_j)
 *
 * evaluated in fp64, max-shifted, rows in index order; a NaN score makes the result NaN
 * (torch.logsumexp's behaviour). The exact route computes just that from windows of exact scores
 * folded into a running (maximum, sum) per query: bit-reproducible, err = 0.
 * The fast route takes a head floor per query, head_floor[i] (typically the k-th exact score of
 * clm_index_search): one fp16 MFMA pass lists the rows whose fp16-pass score is within a margin of
 * the floor or above it (re-scored exactly, summed in fp64) and sums exp(scale * (score - floor)) of
 * all the others on chip in fp32; out_err[i] >= |out_lse[i] - the exact route's result|, a certified
 * bound from the fp16 pass's score error and the fp32 arithmetic. No floating-point
 * atomics: two calls return the same bits. No buffer grows with nq x size.
 * The whole call takes the exact route when head_floor is NULL, the index holds a zero or non-finite
 * row norm, dim > 8192, size > 2^31 - 1, nq x size <= 2^24 (unless CLM_LSE_FAST), CLM_LSE_EXACT or
 * $CLM_SEARCH_FULL=1; a single query does when its band list overflowed the capacity or is empty
 * (a floor above every score) or its floor is not finite. band_cap: as in clm_index_rank (capacity
 * in the CLM_RANK_CAP_MASK bits, 0 = default). q [nq, dim] CLM_F32|CLM_F16; out_lse [nq] doubles,
 * out_err [nq] floats or NULL; every pointer host or device. scale is a double on purpose: 1 / 0.07
 * rounded to fp32 moves a loss by about 1e-7.
 * A row-sharded index is additive: lse of the whole = logaddexp over the shards' results, each shard
 * called with floors of its own, and the largest shard bound bounds the merged error.
 * CLM_E_ARG: an empty index, a null q or out_lse, a dtype other than f32 / f16, nq < 0, a scale that
 * is not finite and positive. */
enum { CLM_LSE_EXACT = 1 << 30, CLM_LSE_FAST = 1 << 29 };
int clm_index_lse(clm_index* idx, const void* q, int q_dtype, int64_t nq, double scale, const float* head_floor,
                  double* out_lse, float* out_err, int band_cap, void* stream);

/* The reference route. An exact score is an fp64 cosine rounded once to fp32, so clm_index_lse's
 * result is within scale * 2^-25 of the log-sum-exp of the unrounded cosines, and a loss built on it
 * and on clm_index_rank's scores sits a few 1e-9 from the same loss in float64. This call is
 * clm_index_lse's exact route (the same row windows, the same fold) with no rounding to fp32 at all:
 * out_lse[i] = log sum_j exp(scale * c_ij), c_ij = dot / (|q_i| |row_j|) in fp64, and, when out_pair
 * is given, out_pair[i] = c_ij of row target[i] (a global row id as in clm_index_rank; NaN when the
 * index does not hold it). Bit-reproducible; a NaN cosine makes the result NaN. The cost is that of
 * the exact route: for model selection by the reference's own number, not for serving.
 * q [nq, dim] CLM_F32|CLM_F16; target [nq] or NULL; out_lse [nq], out_pair [nq] or NULL; every pointer
 * host or device. CLM_E_ARG: as clm_index_lse, and out_pair without target. */
int clm_index_lse64(clm_index* idx, const void* q, int q_dtype, int64_t nq, double scale, const int64_t* target,
                    double* out_lse, double* out_pair, void* stream);

/* Softmax-weighted sums over the index, both ways: what the gradient of a softmax / InfoNCE loss over
 * the index needs, with nothing sized nq x size. With unit vectors q^_i, r^_j, s_ij = q^_i . r^_j and
 *   W_ij = wq * exp(scale * s_ij - q_lse[i]) + wr * exp(scale * s_ij - row_lse[j])
 * (the wr term absent when row_lse is NULL):
 *   out_dq[i] = sum_j W_ij r^_j   [nq, dim] fp32,      out_dr[j] = sum_i W_ij q^_i   [size, dim] fp32
 * in local row order; either output may be NULL. q_lse [nq] / row_lse [size] are log-sum-exps in
 * doubles as clm_index_lse returns them (q_lse of the queries over the index, row_lse of each index
 * row over the queries), expected within scale * E of the true ones, E = 2.441e-3 the fp16 pass's
 * score bound: weights far above what such offsets allow saturate at the fp16 maximum instead of
 * overflowing. The scores inside W are fp16-pass scores: per output row the 2-norm of the error is at
 * most rho times the row's weight mass plus tau, rho = expm1(scale * E) and about 2e-3 more for the fp16
 * roundings (DESIGN.md states every term: 0.038 at scale 1 / 0.07, 0.28 at 100 in the worst case;
 * measured values sit near 1e-3), tau = terms * 2^-14 * (wq + wr) * exp(2 scale E) / 65504 for the weights
 * below fp16's normal range. No floating-point atomics: two
 * identical calls return the same bits; the bits may depend on nq, chunk_rows and query_block.
 * chunk_rows / query_block: index rows / queries per pass, rounded up to multiples of 64; 0 = default
 * (bounded by $CLM_SEARCH_WS_MB and a quarter of the free device memory). Every pointer host or device.
 * CLM_E_ARG: an empty index, a null q or q_lse, a dtype other than f32 / f16, nq < 0, a scale that is
 * not finite and positive, a negative or non-finite weight, wr > 0 without row_lse, dim > 8192, size >
 * 2^31 - 1, an index row or a query whose norm is zero or not finite (the reference's gradient is NaN
 * there). nq == 0 returns at once. clm_index_stats2 entries 22 / 23 count the queries served and the
 * (query block, row chunk) passes run. */
int clm_index_softmax_grad(clm_index* idx, const void* q, int q_dtype, int64_t nq, double scale,
                           const double* q_lse, const double* row_lse, double wq, double wr, float* out_dq,
                           float* out_dr, int64_t chunk_rows, int64_t query_block, void* stream);

/* Threshold search: WHICH rows score at or above a threshold. With s_j the exact score of row j (as
 * clm_index_search returns it) and tau = threshold[i] (one fp32 per query), the result of query i is
 *
 *     { j : s_j >= tau, or s_j is NaN }        (rank_ahead(s_j, id_j, tau, INT64_MAX) of the rank order)
 *
 * ordered (score desc, global id asc), NaN above every number. So its length is
 * clm_index_count_above(q_i, tau, INT64_MAX), it equals bit for bit the first entries of
 * clm_index_search(q_i, k) for every k that holds it, and the results of row shards concatenate and
 * merge to the whole index's. tau = -inf returns every row, +inf (or 2.0) none but NaN-scoring rows, a
 * NaN tau only the NaN-scoring rows. NaN scores lead a result, in id order, and are returned with
 * their sign bit cleared (the sort key of a score is its bit pattern). Two calls return the same bits (integer atomics only; a sort
 * makes the order canonical).
 * Results are ragged, so the index holds them: out_offsets [nq + 1] (host or device) says that query
 * i owns entries [offsets[i], offsets[i + 1]) of the held result, clm_index_search_above_read copies
 * entries [start, start + n) -- exact scores f32, global ids i64, host or device -- until the next
 * threshold search, clm_index_reset, a mutation (append / import / remove / update) or destroy.
 * clm_index_search_above_rows takes the index's own rows [row0, row0 + nrows) as the queries (row0 a
 * global id; the fp32 rows where the index keeps them, else its fp16 rows) without moving them: the
 * self-join behind near-duplicate listing.
 * Fast route: one fp16 MFMA pass lists per query the rows whose fp16-pass score reaches tau minus the
 * rank margin, they are re-scored exactly, the rows that pass are sorted. Exact route: windows of
 * exact scores, counted, then collected. band_cap: as in clm_index_rank (list capacity per query in
 * the CLM_RANK_CAP_MASK bits, 0 = default; a list that overflows is redone with the capacity it
 * needs, then by the exact route); CLM_RANK_EXACT / CLM_RANK_BAND force a route. The whole call is
 * exact under clm_index_rank's conditions (a zero or non-finite row norm in the index, dim > 8192,
 * size > 2^31 - 1, nq x size <= 2^24, $CLM_SEARCH_FULL=1); a single query is when its tau or its norm
 * is not finite. Nothing is sized by nq x size; a low tau returns up to nq x size entries (12 B each,
 * 28 B while they are sorted), each re-scored exactly. At most 2^32 - 1 rows per index.
 * CLM_E_ARG: an empty index, a null pointer, a dtype other than f32 / f16, nq < 0, rows outside the
 * index. CLM_E_OOM: the result cannot be allocated (clm_last_error names the entry count); the index's
 * rows are untouched. clm_index_search_above_read: CLM_E_STATE when no result is held, when it was
 * invalidated, or when the range is outside it. */
int clm_index_search_above(clm_index* idx, const void* q, int q_dtype, int64_t nq, const float* threshold,
                           int64_t* out_offsets, int band_cap, void* stream);
int clm_index_search_above_rows(clm_index* idx, int64_t row0, int64_t nrows, const float* threshold,
                                int64_t* out_offsets, int band_cap, void* stream);
int clm_index_search_above_read(clm_index* idx, int64_t start, int64_t n, float* out_scores, int64_t* out_idx,
                                void* stream);

/* Filtered search: exact top-k over an allowed subset of the rows. allow: ceil(size / 32)
 * little-endian uint32 words, bit j & 31 of word j >> 5 set iff local row j (global id offset + j)
 * is allowed; bits at or past size in the last word are ignored. The result of query i is the first
 * k entries of the ALLOWED rows in the search order (exact score desc, global id asc, NaN above every
 * number), scores bit for bit clm_index_search's; slots past the number of allowed rows hold
 * (-inf, -1). So an all-ones mask returns what clm_index_search returns, the result equals
 * clm_index_search on an index holding only the allowed rows in order (positions mapped back to ids),
 * and the results of row shards merge with clm_topk_merge.
 * Three routes, the same bits on each: exact (windows of exact scores, disallowed entries set to
 * -inf, the exact scan's top-k; k <= 1024), gather (the allowed rows' operands gathered into a
 * temporary index of P x (6 dim + 4) bytes, P = the allowed rows, searched as clm_index_search does,
 * positions mapped back; any k) and pass (a sample of the allowed rows gives each query a threshold,
 * one fp16 MFMA pass lists the allowed rows that reach it, they are re-scored exactly; k <= 256, finite
 * row norms, dim <= 8192). flags: 0 = chosen by size, k and P; CLM_MASK_EXACT / _PASS / _GATHER ask
 * for a route, which is taken when its preconditions hold (clm_index_stats2 says which route served).
 * An index holding a zero or non-finite row norm (NaN scores) is served by the exact route while
 * k <= 1024, as is a single NaN-scoring query of the other routes; for k > 1024 NaN scores are placed
 * as clm_index_search places them. Mind the cost: the exact route computes all nq x size cosines in
 * fp64 (about 2 ms per query per 1 M rows of 512 dims), so one zero row in a large index makes every
 * filtered search of it that slow -- remove or replace such rows (clm_index_remove / _update).
 * Otherwise the exact scan over all rows is taken only on request, for dim > 8192 or under
 * $CLM_SEARCH_FULL=1; small problems go through the gather route, whose temporary index takes the
 * exact scan up to 2^20 cosines.
 * The call keeps no state: it leaves a held threshold-search result and the cached row sample of the
 * unmasked search as they are. q [nq, dim] CLM_F32|CLM_F16; every pointer host or device; k >= 1.
 * CLM_E_ARG: a null index, q, allow or output with nq > 0, a dtype other than f32 / f16, nq < 0, an
 * empty index. CLM_E_OOM: the gather route's buffers cannot be allocated (clm_last_error names the
 * row count). */
enum { CLM_MASK_EXACT = 1 << 30, CLM_MASK_PASS = 1 << 29, CLM_MASK_GATHER = 1 << 28 };
int clm_index_search_masked(clm_index* idx, const void* q, int q_dtype, int64_t nq, int k,
                            const uint32_t* allow, int flags, float* out_scores, int64_t* out_idx, void* stream);

/* Keyed search: exact top-k under one key range PER QUERY, in one batched pass. keys [size] holds one
 * int32 per index row in local row order (row j has global id offset + j), lo / hi [nq] one inclusive
 * range per query: row j is open to query i iff lo[i] <= keys[j] <= hi[i]. Row i of the result is bit
 * for bit row 0 of clm_index_search_masked(q_i, k, mask_i) with mask_i = the rows open to query i: the
 * same order (NaN first, exact score descending, global id ascending), the same exact scores and global
 * ids, (-inf, -1) past the number of open rows. An empty range (lo[i] > hi[i]) or one no key falls in
 * gives a row of pads. A timestamp bound, a category (lo == hi) and a price band take this form once the
 * values are mapped to their ranks; a key no range can hold (-1 below ranges that start at 0) closes a
 * row to every query, which is how a batch-wide mask combines with the ranges.
 * Two routes, the same bits on each. exact: windows of exact scores, the closed entries of each query set
 * to -inf, the exact scan's top-k. pass: a strided sample of min(size, 2^18, round_up(max(8192, k * size
 * / 256), 256)) rows, struck out per query, gives each query a threshold (-inf with fewer than k open
 * sample rows), one fp16 MFMA pass lists the open rows that reach it, they are re-scored exactly; a
 * query whose list overflowed 2,048 entries or ended short of min(k, n_in[i]) is redone by the exact
 * route. The sample only sets the cost: its open rows are rows of the index, so the threshold never
 * cuts below k of them. flags: 0 = the pass route unless the index holds a zero or non-finite row norm,
 * $CLM_SEARCH_FULL=1, dim > 8192, k > 256 or size < 4 * round_up(max(8192, k * size / 256), 256);
 * CLM_MASK_EXACT asks for the exact route, CLM_MASK_PASS for the pass route (taken with finite row
 * norms, k <= 256, dim <= 8192). clm_index_stats2 entries 20 / 21 say which route served.
 * n_in [nq] (or NULL): the number of rows in each query's range, which spares the exact redo of a query
 * whose range holds fewer than k rows (with NULL every list short of k is redone). The pass route checks
 * it from one side: a query that lists more rows than n_in[i] says its range holds is CLM_E_ARG.
 * keys are copied into the index's workspace on every call; keys, lo, hi, n_in and the outputs may each be
 * host or device pointers. q [nq, dim] CLM_F32|CLM_F16; 1 <= k <= 1024 (there is no gather route to serve
 * a larger k). The call keeps no state. CLM_E_ARG: a null index, q, keys, lo, hi or output with nq > 0, a
 * dtype other than f32 / f16, nq < 0, k outside [1, 1024], flags other than 0 / CLM_MASK_EXACT /
 * CLM_MASK_PASS (CLM_MASK_GATHER among them), an empty index. nq == 0 is CLM_OK. */
int clm_index_search_keyed(clm_index* idx, const void* q, int q_dtype, int64_t nq, int k, const int32_t* keys,
                           const int32_t* lo, const int32_t* hi, const int64_t* n_in, int flags,
                           float* out_scores, int64_t* out_idx, void* stream);

/* search-path counters since creation: queries served by the sampled single-pass bounded
 * search (`filtered`), by the exact scan or the fp16-scan-bounded search (`exact`), and
 * bounded queries whose candidate list overflowed (redone by a whole-list pass, or by the exact
 * scan when the list is longer than 8192 / k chunks of 4096) */
int clm_index_stats(const clm_index* idx, int64_t* filtered, int64_t* exact, int64_t* overflow);
/* out[0..n), n <= 24: sampled bounded, fp16-scan bounded, full exact scan, overflow re-runs, then the
 * sampled queries whose filter pass ran on the G2 256 x 192 tiles / on gemm_kernel 256 x 256 (chosen
 * per query block from the block's sampled candidate counts: near-duplicate blocks take the latter),
 * then the queries served by the small-batch streaming search (nq <= 16 on a large index: one pass
 * over the fp16 rows, thresholds from 256-row chunk maxima), then the rank / count_above queries
 * served by the band pass, by the exact route, those of the latter whose band list overflowed, and
 * the band rows re-scored for the band-served queries, then the clm_index_lse queries served by the
 * fast route, by the exact route (clm_index_lse64's among them), and those whose band list overflowed
 * its capacity, then the threshold-search queries served by the MFMA pass, by the exact route, and
 * those whose candidate list overflowed its capacity, then the clm_index_search_masked queries served
 * by the pass route, by the gather route and by the exact route (a pass-route query redone exactly
 * counts as exact), then (entries 20 / 21) the clm_index_search_keyed queries served by the pass route
 * and by the exact route (a redone query counts as exact), then (entries 22 / 23) the
 * clm_index_softmax_grad queries served and the (query block, row chunk) passes run for them */
int clm_index_stats2(const clm_index* idx, int64_t* out, int n);

/* full cosine matrix, exact: out [nq, n] f32 = fp32(cos64(q_i, c_j)), any dim */
int clm_cosine_scores(int hip_device, const float* q, int64_t nq, const float* c, int64_t n,
                      int dim, float* out, void* stream);

/* merge `parts` sorted candidate lists per query: scores/idx [nq, parts*k_in]
 * -> [nq, k] by (score desc, index asc); idx < 0 marks an empty slot. Indices are any int64 >= 0
 * while parts * k_in <= 8192 and k <= 1024 (one LDS sort per query); larger merges take indices
 * below 2^32 and return CLM_E_ARG for any other. */
int clm_topk_merge(int hip_device, const float* scores, const int64_t* idx, int64_t nq,
                   int parts, int k_in, int k, float* out_scores, int64_t* out_idx, void* stream);

/* rows [n, dim] f32 in place (device or host) */
int clm_l2_normalize(int hip_device, float* rows, int64_t n, int dim, void* stream);

/* query fusion, replaces SeekerService._build_query_embedding (src/embedding/seeker_service.py:84-157):
 * out[i] = v / ||v|| with v = w_a*a[i] + w_b*b[i], rows [n, dim] f32; b == NULL gives out = a / ||a||
 * (the single-modality branch, :149-152). a, b, out all device or all host; out may alias a. */
int clm_fuse_queries(int hip_device, const float* a, float w_a, const float* b, float w_b, int64_t n,
                     int dim, float* out, void* stream);

/* Kernel-level entry points (unit tests and micro-benchmarks of the hot kernels).
 * clm_gemm: C[M,N] = A[M,K] . W[N,K]^T with dtype CLM_BF16|CLM_F16 operands (device
 * pointers), K % 64 == 0, epilogue CLM_EPI_*; config < 0 picks the tile heuristically. */
enum { CLM_EPI_STORE = 0, CLM_EPI_GELU = 1, CLM_EPI_RESID = 2, CLM_EPI_SCORE = 4 };
int clm_gemm(int hip_device, int dtype, int epilogue, int config, const void* A, int64_t lda,
             const void* W, int64_t ldw, int M, int N, int K, void* out, int64_t ldo,
             const float* bias, const float* rscale, const float* cscale, void* stream);
int clm_gemm_num_configs(void);
/* the sampled search's fp16 score forms (fp16 A / W, device pointers): score = acc * rscale[m] *
 * cscale[n] rounded toward -inf to fp16 (mode 1, out [M, ldo] u16), or the maxima of each group of
 * 4 consecutive columns rounded the same way (mode 2, out [M, ldo >= N/4], a row's groups in a
 * fixed permutation; config 1, N % 256 == 0) */
int clm_gemm_scores16(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M,
                      int N, int K, const float* rscale, const float* cscale, void* out, int64_t ldo, int mode,
                      void* stream);
/* clm_gemm_select: the GEMM whose epilogue selects instead of storing, as every index pass runs it
 * (test hook; fp16 A [M, lda] / W [N, ldw], device pointers; every extent is the caller's to provide).
 * s = acc * rscale[m] * cscale[n] (rscale NULL: 1), t = theta[m * theta_ld], id = base + n:
 *   CLM_EPI_FILTER       s >= t: (s, id) appended to row m's list cand_s / cand_i [M, cap];
 *   CLM_EPI_FILTER_MASK  the same over the columns whose bit n & 31 of mask[n >> 5] is set; mask holds
 *                        ceil(N / 32) words; the bits at or past N of the last word are not read;
 *   CLM_EPI_RANK         s > t + margin counted into above[m]; otherwise s >= t - margin: id appended;
 *   CLM_EPI_LSE          s >= t - margin: id appended; every other column adds exp2((s - t) * lse_c) to
 *                        one slot of lse_part [M, lse_ld >= N / 64 + 4]: slot (n / BN) * WN + wave column
 *                        of the config's BN-wide tile with WN wave columns (config 1: 128 columns per
 *                        slot, 8: 96, 9 / 10 / 11: 64). The slots ceil(N / BN) * WN of a row m < M are
 *                        each stored once (a slot none of whose columns is below N holds 0), the others
 *                        are not touched. A NaN score makes its slot NaN.
 * Appends go to slot atomicAdd(cnt[m], 1) while that is below cap, in no fixed order; cnt[m] counts them
 * all, stored or not. cand_s is unused by RANK / LSE. A NaN score or threshold selects nothing (RANK:
 * neither counted nor listed). Nothing is zeroed: cnt, above and lse_part are the caller's, and rows at
 * or past M of every output are untouched.
 * cbound (or NULL: no skip test): the 2 keys of clm_value_bounds(cscale, N); FILTER / FILTER_MASK / RANK
 * then skip the 16 x 16 blocks whose largest possible score is below the threshold -- the selected
 * (s, id) sets are the same. m_fastest: 0 = the grouped tile order of clm_gemm, non-0 = the index passes'
 * (consecutive workgroups walk M); the results do not depend on it. config as clm_gemm (-1: heuristic):
 * FILTER runs on configs 0-12, the others on 1 and 8-11; anything else is CLM_E_HIP with nothing written.
 * CLM_E_ARG, before any launch: an epilogue outside the four, config >= clm_gemm_num_configs(), M or N < 0,
 * K <= 0 or K % 64, lda / ldw not a multiple of 8 or below K, cap < 1, theta_ld < 1, LSE with lse_ld <
 * N / 64 + 4, and with M, N > 0 a null A, W, cscale, theta, cnt, cand_i, or the epilogue's own cand_s /
 * above / lse_part / mask. M == 0 or N == 0 is CLM_OK. clm_debug_set applies as to clm_gemm.
 * clm_value_bounds: keys[0] / keys[1] (device) = the order key of min / max over v[0, n) (device), key(f)
 * = bits(f) ^ 0xFFFFFFFF for a set sign bit, bits(f) | 0x80000000 otherwise; a NaN anywhere makes the
 * decoded minimum (sign bit set) or maximum NaN. n == 0 gives {0xFFFFFFFF, 0}. CLM_E_ARG: n < 0, a null
 * keys, a null v with n > 0. */
enum { CLM_EPI_FILTER = 5, CLM_EPI_RANK = 6, CLM_EPI_LSE = 7, CLM_EPI_FILTER_MASK = 8 };
int clm_gemm_select(int hip_device, int epilogue, int config, const void* A, int64_t lda, const void* W,
                    int64_t ldw, int M, int N, int K, const float* rscale, const float* cscale,
                    const float* theta, int64_t theta_ld, float margin, int* cnt, float* cand_s, int64_t* cand_i,
                    int cap, int64_t base, const uint32_t* cbound, uint32_t* above, float* lse_part,
                    int64_t lse_ld, float lse_c, const uint32_t* mask, int m_fastest, void* stream);
int clm_value_bounds(int hip_device, const float* v, int64_t n, uint32_t* keys, void* stream);
/* clm_gemm_select_keyed: clm_gemm_select for CLM_EPI_FILTER_KEYS (test hook; clm_gemm_select itself refuses
 * that epilogue: it has no room for the arguments). CLM_EPI_FILTER with one open test per (row, column):
 * column n is tested for row m only where klo[m] <= keys[n] <= khi[m]; keys [N] (16-byte aligned), klo /
 * khi [M], device pointers. Row m's count and appended (s, id) set are bit for bit what
 * CLM_EPI_FILTER_MASK gives it under the mask of its open columns. Configs 1 and 8-11, -1 = heuristic;
 * cbound, m_fastest and the CLM_E_ARG cases as clm_gemm_select, plus null or misaligned keys, null klo / khi. */
enum { CLM_EPI_FILTER_KEYS = 9 };
int clm_gemm_select_keyed(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M,
                          int N, int K, const float* rscale, const float* cscale, const float* theta,
                          int64_t theta_ld, int* cnt, float* cand_s, int64_t* cand_i, int cap, int64_t base,
                          const uint32_t* cbound, const int32_t* keys, const int32_t* klo, const int32_t* khi,
                          int m_fastest, void* stream);
/* clm_gemm_softw: the softmax-weight epilogue alone (test hook; fp16 A [M, lda] / W [N, ldw], device
 * pointers). s = acc * rscale[m] * cscale[n] (either NULL: 1), x = s * c:
 *   out[m * ldo + n] = fp16(min(exp2(x - lq[m]) + exp2(x - lr[n]), 65504))   (lr NULL: the first term alone)
 * lq [M], lr [N] fp32 (lr 16-byte aligned); out u16 [M, ldo >= N]; rows at or past M and columns at or
 * past N are untouched. Configs 0 and 1 (-1: heuristic); any other is CLM_E_HIP with nothing written.
 * CLM_E_ARG: config >= clm_gemm_num_configs(), M or N < 0, K <= 0 or K % 64, lda / ldw not a multiple
 * of 8 or below K, ldo < N, and with M, N > 0 a null A, W, lq or out, or a misaligned lr.
 * clm_transpose16: dst[c * ldd + r] = fp16(float(src[r * lds + c]) * s[r]) for r < rows, c < cols (s
 * NULL: 1; fp16 src / dst, fp32 s, device pointers); columns rows .. round_up(rows, 64) - 1 of every dst
 * row are written as zeros. CLM_E_ARG: rows or cols < 0, lds < cols, ldd < round_up(rows, 64), and with
 * rows, cols > 0 a null src or dst. */
enum { CLM_EPI_SOFTW = 10 };
int clm_gemm_softw(int hip_device, int config, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N,
                   int K, const float* rscale, const float* cscale, const float* lq, const float* lr, float c,
                   void* out, int64_t ldo, void* stream);
int clm_transpose16(int hip_device, const void* src, int64_t lds, int64_t rows, int64_t cols, const float* s,
                    void* dst, int64_t ldd, void* stream);
/* diagnostic flags (micro-benchmarks and tests only; 0 in production), initialised from
 * $CLM_GEMM_DEBUG: for later clm_gemm / clm_gemm_select calls bit 0 = skip the epilogue (accumulators kept
 * live), bit 1 = run the epilogue but drop every store, bit 2 = one tile per workgroup
 * instead of the persistent grid; for later encodes bit 3 (value 8) = run the last encoder
 * layer on every row instead of only the pooled rows, bit 4 (16) = q/k/v GEMM and attention
 * as two kernels instead of the fused one, bit 5 (32) = encode every padded caption row
 * instead of each caption's live rows (all: same embeddings, for parity tests). */
void clm_debug_set(int flags);
/* sampled-search thresholds (the bounded search's step 1 over the sample-score rows):
 * th[q] = (k-th largest of scores[q, 0:C), duplicates counted) - margin, scores [nq, lds] f32,
 * device pointers. method 0: one streaming pass (k <= 8), 1: radix top-k select + gather (the
 * general path, k <= 1024); both give the same bits. */
int clm_topk_threshold(int hip_device, const float* scores, int64_t lds, int64_t nq, int64_t C, int k,
                       float margin, int method, float* th, void* stream);
/* the small-batch search's streaming scan (nq <= 16 fp16 queries q16 [nq, dim] against fp16 rows16
 * [N, dim], device pointers): out [N, ldo] f32 = acc * qinv[q] * inv[row], query q of a row in
 * column q (ldo = 1, 2, 4, 8 or 16, >= nq; columns of a group of four that starts at or past nq
 * are not written), cmax [nq, ceil(N / 256)] = each 256-row chunk's largest score (NaN ignored),
 * wtop (or NULL) [nq, ldw] = every wave's 8 largest chunk maxima at columns 8 w .. 8 w + 7 (-inf
 * padded), ldw >= 8 * clm_scan16_waves(N, dim). dim % 64 == 0 in [64, 1024]; else CLM_E_ARG.
 * The extents are the caller's to provide: out holds N * ldo floats, cmax nq * ceil(N / 256),
 * wtop nq * ldw. clm_scan16_waves means something only for a dim that clm_scan16 accepts. */
int clm_scan16(int hip_device, const uint16_t* rows16, const float* inv, int64_t N, int dim, const uint16_t* q16,
               const float* qinv, int nq, float* out, int64_t ldo, float* cmax, float* wtop, int64_t ldw,
               void* stream);
int64_t clm_scan16_waves(int hip_device, int64_t N, int dim);
/* ... and its candidate collection: every (score, base + row) of column q of scores [C, ldq]
 * (ldq a power of two in [nq, 16]) with score >= th[q] appended to q's list cand_s / cand_i
 * [nq, cap] in no fixed order; cnt[q] (zeroed by the caller) counts them all, stored or not. */
int clm_collect_ge(int hip_device, const float* scores, int ldq, int nq, int64_t C, const float* th, int* cnt, int cap,
                   float* cand_s, int64_t* cand_i, int64_t base, void* stream);
/* clm_topk_any: the top-k of any k (the search's path for k > 1024 and the merge's past one LDS sort), test
 * hook, device pointers. Row q of scores [nq, lds >= C] f32; idx (or NULL) [nq, ldi >= C]: an entry with
 * idx < 0 cannot be taken. out_scores / out_idx [nq, k]: the first k takeable entries by (order key of the
 * score desc -- key as clm_value_bounds: a positive NaN above +inf, a negative one below -inf, +0 above -0
 * --, low 32 bits of idx, or the column, asc), then (-inf, -1). The id is idx's value (below 2^32; base is
 * ignored), or base + column without idx. The workspace is the device scratch; the call drains the stream.
 * CLM_E_ARG, nothing written: k < 1, nq < 0 or > 65535, C < 0 or > 2^32 - 1, lds < C, ldi < C with idx, a
 * pointer that is not device memory. nq == 0 is CLM_OK. */
int clm_topk_any(int hip_device, const float* scores, int64_t lds, const int64_t* idx, int64_t ldi, int64_t nq,
                 int64_t C, int k, int64_t base, float* out_scores, int64_t* out_idx, void* stream);
/* clm_mask_rows: the mask steps of clm_index_search_masked, in its order (test hook, device pointers):
 * words [ceil(N / 32)] = allow's words with the bits at or past N cleared (allow is not written), bcnt
 * [blocks] = the set bits of each block of 8192 rows (blocks = ceil(N / 8192)), boff [blocks + 1] = their
 * exclusive prefix sums, boff[blocks] = P, list (or NULL: not built) [>= P, the caller's to size: N always
 * holds it] = the set rows ascending; *P_out (a host int64, or NULL) = P. The call drains the stream.
 * CLM_E_ARG, nothing written: N < 1 or > 2^32 - 1, a pointer that is not device memory. */
int clm_mask_rows(int hip_device, const uint32_t* allow, int64_t N, uint32_t* words, uint32_t* bcnt, int64_t* boff,
                  uint32_t* list, int64_t* P_out, void* stream);
/* clm_topk_distinct: the first k entries of a list that open a new group -- the selection step of the
 * grouped (collapse) search, CosineIndex.search_grouped and distributed.merge_grouped_gpu. Device pointers.
 * Query q owns a list of entries (scores f32, idx i64, gid i64), already in the search order: entries
 * [q * ld, (q + 1) * ld) of the three arrays (offsets == NULL: fixed width), or [offsets[q], offsets[q + 1])
 * with offsets [nq + 1] i64 (the shape clm_index_search_above returns). An entry with idx < 0 (a pad, or a
 * row the caller struck out) is skipped wherever it stands, as is one with gid < 0. An entry is KEPT iff no
 * earlier position of its list carries its gid. out_scores / out_idx / out_gid [nq, k] = the first k kept
 * entries in list order -- each with its score, idx and gid bit for bit as given --, then (-inf, -1, -1);
 * out_found [nq] i32 = the number of kept entries written (<= k).
 * gid is any int64 >= 0: the set of gids seen is a hash table in LDS keyed by the whole value, so values
 * that share a slot are still told apart. The result is a pure function of the lists: where several
 * positions carry a gid the lowest one wins (an integer minimum, not arrival order), and the output slots
 * are prefix sums in list order; two calls return the same bits. One workgroup per list walks it in chunks
 * of 1024 entries and stops at k kept; a list has any length (64-bit offsets). The call does not drain the
 * stream.
 * CLM_E_ARG, nothing written: k outside [1, 1024], nq < 0, ld < 0, and with nq > 0 a null output, a null
 * list array (unless offsets == NULL and ld == 0), or a pointer that is not device memory. nq == 0 is
 * CLM_OK. The extents are the caller's to provide: offsets must be non-decreasing and inside the arrays. */
int clm_topk_distinct(int hip_device, const float* scores, const int64_t* idx, const int64_t* gid,
                      const int64_t* offsets, int64_t ld, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                      int64_t* out_gid, int32_t* out_found, void* stream);
/* attention over qkv [B*T, 3*H*64] (q pre-scaled by 64^-1/2), out [B*T, ldo] (device
 * pointers); causal: 0 / non-0 switch (the text tower's mask). */
int clm_attention(int hip_device, int dtype, int causal, const void* qkv, void* out, int64_t ldo,
                  int B, int T, int H, void* stream);
/* the same with a flag word: CLM_ATTN_CAUSAL (1), CLM_ATTN_Q_LOG2E (2): q carries log2(e) as
 * well -- the form the engine uses where the kernel takes log2-domain scores (bf16, non-causal,
 * T > 128); CLM_E_ARG for any other shape or an unknown flag bit. */
#define CLM_ATTN_CAUSAL 1
#define CLM_ATTN_Q_LOG2E 2
int clm_attention_ex(int hip_device, int dtype, int flags, const void* qkv, void* out, int64_t ldo,
                     int B, int T, int H, void* stream);
/* LayerNorm of fp32 rows src [M, lds] over d columns (d a multiple of 128, <= 1024), eps, fp32
 * gamma / beta -> y [M, ldy] in dtype CLM_BF16|CLM_F16 (device pointers); the encoder's kernel
 * (TF/models/clip/modeling_clip.py:358,360 nn.LayerNorm) */
int clm_layernorm(int hip_device, int dtype, const float* src, int64_t lds, int64_t M, int d,
                  const float* gamma, const float* beta, float eps, void* y, int64_t ldy, void* stream);
/* the varlen text plan of ids [B, L] (device pointers): lens [B] = each caption's live rows (its
 * pooled row + 1: the first eos, or with eos == 2 the first largest id; row 0 if there is none),
 * offs [B + 1] = their exclusive prefix sums (offs[B] = the total), rowmap [B * L]: packed row
 * offs[b] + p -> b * L + p (the first `total` entries are written), tiles [B]: whole captions in
 * order, <= 256 rows per tile, tiles[t] = first caption | captions << 16 (the first counts[1]
 * entries are written), counts [2] = {total, tiles}. 0 <= B <= 4096, 1 <= L <= 256, else CLM_E_ARG;
 * B == 0 writes nothing. */
int clm_text_plan(int hip_device, const int32_t* ids, int B, int L, int eos, int* lens, int* offs, int* rowmap,
                  int* tiles, int* counts, void* stream);
/* fused q/k/v projection + attention, T <= 128 (device pointers): out [rows, ldo >= H*64] =
 * attention(X [rows, ldx] . W [3*H*64, ldw]^T + bias [3*H*64] or NULL), q rows of W pre-scaled by
 * 64^-1/2; the bits of clm_gemm(CLM_EPI_STORE) followed by clm_attention. flags: CLM_ATTN_CAUSAL.
 * K % 32 == 0 (K % 64 == 32: ldx, ldw >= round_up(K, 64), every row readable and finite that far),
 * ldx % 8 == 0, ldw % 8 == 0, ldo % 4 == 0. lens / offs / tiles / counts all NULL: B sequences of T
 * rows each; all set (clm_text_plan's outputs for B <= 65535 captions of padded length T): the packed
 * live rows, sequence b at rows offs[b] .. offs[b] + lens[b]. A mixture is CLM_E_ARG; a shape the
 * kernel does not take is an error and writes nothing. */
int clm_gemm_attn(int hip_device, int dtype, int flags, const void* X, int64_t ldx, const void* W, int64_t ldw,
                  const float* bias, void* out, int64_t ldo, int B, int T, int H, int K, const int* lens,
                  const int* offs, const int* tiles, const int* counts, void* stream);
/* Test hooks over the encoder's remaining launchers (device pointers; every extent is the caller's to
 * provide). Each checks its arguments (CLM_E_ARG) before anything is launched; what the launcher
 * itself refuses is CLM_E_HIP, with nothing written.
 *
 * clm_layernorm_ex: the LayerNorm kernel with every option (d, ldy, dtype as clm_layernorm).
 *   mode 0: x = src [M, lds] rows. mode 1 (text embeddings): x = tok[ids[s]] + pos[s % L], one fp32 add,
 *   s = r, or rowmap[r] where rowmap (clm_text_plan's; mode 1 only) is given; tok [vocab, d], pos [L, d],
 *   ids indexed by s; x is written to hf [M, ldh].
 *   g2 / b2 NULL: y = LN(x; g1, b1). Both set (the dual LayerNorm): hf = LN(x; g1, b1) in fp32 (hf may be
 *   src: in place) and y = LN(hf; g2, b2). hf is required by mode 1 and by g2, otherwise unused.
 *   m_dev (or NULL): only rows r < *m_dev (a device int, <= M) are computed; M sizes the grid, rows at
 *   or past *m_dev are untouched and *m_dev == 0 writes nothing.
 *   CLM_E_ARG: what clm_layernorm refuses; mode not 0 / 1; mode 1 with a null ids, tok, pos or hf or
 *   L < 1; ldh < d or ldh % 4 with hf; one of g2 / b2 alone; g2 without hf; rowmap in mode 0. M == 0 is
 *   CLM_OK. */
int clm_layernorm_ex(int hip_device, int dtype, int mode, const float* src, int64_t lds, const int32_t* ids,
                     const float* tok, const float* pos, int L, float* hf, int64_t ldh, const float* g1,
                     const float* b1, const float* g2, const float* b2, float eps, void* y, int64_t ldy, int64_t M,
                     int d, const int* m_dev, const int* rowmap, void* stream);
/* clm_gemm_ex: clm_gemm's STORE / GELU / RESID (operands and shapes as there, ldo >= N) plus
 *   CLM_EPI_PATCH: out (fp32) [b (group + 1) + 1 + p, n] = acc + aux[(1 + p) aux_ld + n] for row m =
 *   b group + p -- the patch embeddings written around each image's class row, which is not touched.
 *   aux [group + 1, aux_ld >= N] fp32, group >= 1, M % group == 0, and no bias: one given is refused by
 *   the launcher (CLM_E_HIP); configs 13 / 14 do not have this epilogue (CLM_E_HIP). aux, aux_ld and
 *   group are NULL / 0 / 0 for the other epilogues.
 *   m_dev (or NULL): the row count is *m_dev (a device int, <= M, which sizes the grid); rows at or
 *   past it are untouched, *m_dev == 0 writes nothing.
 *   slices >= 1 (CLM_EPI_RESID only, config -1 or 2, no m_dev): the few-row split-K form, out += acc +
 *   bias with K cut into `slices` (a divisor of K / 64) whose fp32 partials go to ws [slices * M * N]
 *   and are summed in slice order, so a row's bits do not depend on M; N % 4 == 0, ldo % 4 == 0.
 *   slices == 0: the plain GEMM, ws NULL. */
enum { CLM_EPI_PATCH = 3 };
int clm_gemm_ex(int hip_device, int dtype, int epilogue, int config, const void* A, int64_t lda, const void* W,
                int64_t ldw, int M, int N, int K, void* out, int64_t ldo, const float* bias, const float* aux,
                int64_t aux_ld, int group, const int* m_dev, int slices, float* ws, void* stream);
/* clm_patchify: pixels (CLM_PIX_U8_HWC [B, S, S, C] bytes through lut [C, 256], or CLM_PIX_F32_CHW
 *   [B, C, S, S] copied) -> P [B (S/p)^2, Kp] in dtype CLM_BF16|CLM_F16, row b G^2 + py G + px, column
 *   c p^2 + ky p + kx, columns [C p^2, Kp) zero. S % p == 0, 1 <= C <= 4, Kp >= C p^2 (CLM_E_ARG), Kp
 *   % 8 == 0 (the launcher's). lut is required for either layout. */
int clm_patchify(int hip_device, int dtype, const void* pix, int layout, int B, int S, int p, int C,
                 const float* lut, void* P, int Kp, void* stream);
/* clm_write_cls: h[b T, 0:d] = cls[0:d] + pos[0:d] for b < B, h fp32 with row stride ldh >= d */
int clm_write_cls(int hip_device, float* h, int64_t ldh, int B, int T, int d, const float* cls, const float* pos,
                  void* stream);
/* The pooled row of item b: offs[b + 1] - 1 where offs (clm_text_plan's) is given; else b T + t with t =
 * 0 where ids is NULL, else over ids[b, 0:T] the first t with ids == eos (0 if none), or with eos == 2 the
 * first largest id.
 * clm_gather_pooled: hc [B, d] fp32 = h's pooled rows, Oc [B, ldoc] = O's (16-bit values, columns
 *   0:d); d, ldh, ldo, ldoc multiples of 4 (the launcher's).
 * clm_pool_project: pooled row -> LayerNorm(gamma, beta, eps) -> . projT [d, D] (fp32) -> tmp [B, D] ->
 *   divided by its L2 norm if normalize -> out [B, D] in out_dtype CLM_F32|CLM_F16. d <= 1024, d % 16 ==
 *   0 (the launcher's). A row's bits depend on neither B nor its position in the batch. */
int clm_gather_pooled(int hip_device, const float* h, int64_t ldh, const void* O, int64_t ldo, int B, int T, int d,
                      const int32_t* ids, int eos, float* hc, void* Oc, int64_t ldoc, const int* offs, void* stream);
int clm_pool_project(int hip_device, const float* h, int64_t ldh, int B, int T, int d, const int32_t* ids, int eos,
                     const float* gamma, const float* beta, float eps, const float* projT, int D, float* tmp,
                     void* out, int out_dtype, int normalize, const int* offs, void* stream);

/* Kernel timing by category, measured with hipEvents recorded on the launch
 * stream around every kernel of clm_encode_* while enabled (adds event
 * overhead; keep it off in timed regions). categories: CLM_PROF_* */
enum { CLM_PROF_GEMM = 0, CLM_PROF_ATTN = 1, CLM_PROF_LN = 2, CLM_PROF_OTHER = 3, CLM_PROF_NCAT = 4 };
int clm_prof_enable(clm_ctx* ctx, int enable);   /* enabling also resets the counters */
/* sums since enable: kernel milliseconds, algorithmic FLOPs (GEMM/ATTN) or
 * algorithmic bytes (LN/OTHER), and launch count, for one category */
int clm_prof_read(clm_ctx* ctx, int category, double* ms, double* work, int64_t* launches);

const char* clm_last_error(void);
const char* clm_version(void);
/* sizeof(clm_model_desc), so bindings can verify their struct layout */
int32_t clm_model_desc_size(void);

#ifdef __cplusplus
}
#endif
#endif /* CLM_H */
