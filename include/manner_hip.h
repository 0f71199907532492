/*
 * manner_hip.h — C ABI of the MI355X (gfx950) MANNeR news-encoding + candidate-scoring hot path.
 *
 * The reference has no FFI: its "plugin boundary" for this path is a set of torch.nn.Module
 * classes imported by name.  Each entry point below states which reference
 * interface it replaces (paths relative to the reference repository root).  The Python mirror of
 * those classes (manner_amd/models/components/) binds these symbols through ctypes; see
 * INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - every pointer is CALLER-OWNED DEVICE memory unless marked "host"; nothing is retained past
 *     the call except by an encoder handle, which owns private packed copies of the weights;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and is asynchronous with respect to the host; no entry point allocates, frees or
 *     synchronises except *_create / *_destroy / manner_hip_encoder_status;
 *   - return value: 0 = ok, non-zero = MANNER_HIP_E_*; manner_hip_last_error() returns a
 *     thread-local message for the most recent failure.  No C++ exception crosses the ABI.
 */
#ifndef MANNER_HIP_H
#define MANNER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MANNER_HIP_ABI_VERSION 8

enum {
  MANNER_HIP_OK = 0,
  MANNER_HIP_E_INVALID = 1,     /* bad argument (shape, alignment, unsupported architecture) */
  MANNER_HIP_E_WORKSPACE = 2,   /* workspace too small */
  MANNER_HIP_E_RUNTIME = 3,     /* HIP runtime error */
  MANNER_HIP_E_INPUT = 4        /* device-side input validation failed (see encoder_status) */
};

/* Device-side input validation.  Kernels never fault on bad inputs: they raise one of these bits in a status word
 * (the encoder handle's own, or the caller-owned int32 `status` argument of the scoring entry points, which may be
 * NULL) and continue on a safe substitute.  The reference raises a Python exception in each of these cases. */
enum {
  MANNER_HIP_STATUS_MASK = 1,     /* attention_mask is not a right-padded 0/1 prefix with 1..MAX_LEN_INFER tokens (inference),
                                     1..MAX_LEN_TRAIN tokens (train_forward / _backward) or 1..MAX_LEN_FULL tokens ("full rows") */
  MANNER_HIP_STATUS_TOKEN = 2,    /* input id / position outside the embedding tables (IndexError in the reference) */
  MANNER_HIP_STATUS_FUSED = 4,    /* reserved (bounded-wait overflow of a fused kernel) */
  MANNER_HIP_STATUS_INDEX = 8,    /* news / entity index outside the table (IndexError in the reference) */
  MANNER_HIP_STATUS_LENGTHS = 16  /* host_lengths disagree with attention_mask (tokens beyond the chunk bound dropped) */
};

enum { MANNER_HIP_ARCH_BERT = 0, MANNER_HIP_ARCH_ROBERTA = 1 };

/* Arithmetic of the encoder GEMMs/attention.  F32: f32 operands on the f32 MFMA (exact f32 FMA
 * chains; the 1e-4 parity mode).  BF16: bf16 operands, f32 accumulation, f32 LayerNorm/softmax.
 * BF16X3: f32 activations and f32 attention / LayerNorm / erf-GeLU as in F32, but every GEMM runs on the bf16 MFMA
 * over split operands — x = hi + lo, W = hi + lo (bf16 each), x W^T ~ hi.hi + hi.lo + lo.hi as ONE bf16 GEMM of
 * depth 3K: 16-bit operand mantissas, f32 accumulation.  2.3x the F32 mode's speed at 3e-5 .. 1.1e-4 of the reference
 * (stated tolerance 2.5e-4; F32 remains THE 1e-4 parity mode).  Needs H and I multiples of 256.
 * F16: the BF16 schedule and kernels on IEEE half operands (v_mfma_f32_*_f16: same rate, same bytes): 11 mantissa
 * bits instead of 8 (~8x smaller error), f16's exponent range (max 65504) — the arithmetic the reference's own GPU
 * setting computes in (`precision: 16-mixed`, configs/trainer/default.yaml:12).
 * F16X3: BF16X3 with IEEE half splits — hi and lo carry 11 bits each, so the three products reproduce ~21 operand
 * bits (lo parts below 6e-5 fall into f16's subnormals and keep 3e-8 absolute): within 1e-4 of the reference like F32,
 * at the speed of BF16X3.  Needs H and I multiples of 256. */
enum { MANNER_HIP_PREC_F32 = 0, MANNER_HIP_PREC_BF16 = 1, MANNER_HIP_PREC_BF16X3 = 2, MANNER_HIP_PREC_F16 = 3,
       MANNER_HIP_PREC_F16X3 = 4 };

typedef void* manner_hip_stream_t;
typedef struct manner_hip_encoder* manner_hip_encoder_t;

typedef struct manner_hip_encoder_config {
  int32_t arch;         /* MANNER_HIP_ARCH_* : position-id rule */
  int32_t hidden;       /* H, multiple of 128 */
  int32_t layers;
  int32_t heads;        /* head_dim = H / heads must be 64 */
  int32_t intermediate; /* I, multiple of 128 */
  int32_t vocab;
  int32_t max_pos;
  int32_t type_vocab;
  int32_t pad_id;       /* RoBERTa: positions start at pad_id + 1 */
  float ln_eps;
} manner_hip_encoder_config;

/* Order of the fp32 device pointers in the `weights` table of manner_hip_encoder_create: the HF
 * BertModel/RobertaModel state_dict tensors that sit under
 * "news_encoder.text_encoder.plm_model." in a reference checkpoint, nn.Linear
 * layout [out, in].  5 embedding tensors, then 16 per layer. */
enum {
  MANNER_HIP_W_WORD_EMB = 0, MANNER_HIP_W_POS_EMB, MANNER_HIP_W_TYPE_EMB,
  MANNER_HIP_W_EMB_LN_G, MANNER_HIP_W_EMB_LN_B,
  MANNER_HIP_W_EMB_COUNT
};
enum {
  MANNER_HIP_WL_Q_W = 0, MANNER_HIP_WL_Q_B, MANNER_HIP_WL_K_W, MANNER_HIP_WL_K_B,
  MANNER_HIP_WL_V_W, MANNER_HIP_WL_V_B, MANNER_HIP_WL_AO_W, MANNER_HIP_WL_AO_B,
  MANNER_HIP_WL_ALN_G, MANNER_HIP_WL_ALN_B, MANNER_HIP_WL_FF1_W, MANNER_HIP_WL_FF1_B,
  MANNER_HIP_WL_FF2_W, MANNER_HIP_WL_FF2_B, MANNER_HIP_WL_OLN_G, MANNER_HIP_WL_OLN_B,
  MANNER_HIP_WL_COUNT
};

int manner_hip_abi_version(void);
const char* manner_hip_last_error(void);

/* ---------------------------------------------------------------- text encoder (K1-K7)
 * Replaces MannerTextEncoder.__init__/forward — manner/models/components/news_encoder.py:11-37 —
 * i.e. `AutoModel.from_pretrained(plm)(**tokenized).last_hidden_state[:, 0, :]`, eval mode. */

/* Pack the PLM weights (fp32 device pointers, table order above, MANNER_HIP_W_EMB_COUNT +
 * layers*MANNER_HIP_WL_COUNT entries) into the handle's private bf16 and/or fp32 GEMM layouts.
 * `precisions` is a bit mask (1 << MANNER_HIP_PREC_*) of the modes the handle must serve.
 * Synchronises `stream` before returning; the source tensors may be freed afterwards. */
int manner_hip_encoder_create(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/,
                              int32_t n_weights, uint32_t precisions, manner_hip_stream_t stream,
                              manner_hip_encoder_t* out /*host*/);
int manner_hip_encoder_destroy(manner_hip_encoder_t enc);

/* Bytes of scratch manner_hip_encode_cls needs to process `max_tokens` packed tokens and
 * `max_news` news per internal chunk. */
size_t manner_hip_encoder_workspace_bytes(manner_hip_encoder_t enc, int64_t max_news, int64_t max_tokens,
                                          int32_t precision);

/* CLS embeddings of `n_news` tokenised news.
 *   ids, mask : int64 [n_news, padded_len] row-major, exactly the tensors of the reference's
 *               BatchEncoding (manner/data/components/mind_rec_dataset.py:134-137); `mask` must be
 *               a right-padded 0/1 prefix mask with >= 1 real token per news (validated on device,
 *               see manner_hip_encoder_status); padded_len <= MANNER_HIP_MAX_LEN_INFER (512), and every news
 *               also within its model's position table (a longer row raises MANNER_HIP_STATUS_TOKEN, the
 *               reference's IndexError).  Rows of <= MANNER_HIP_MAX_LEN (128) tokens run the short-row kernels
 *               whatever the padded length or their neighbours; longer rows take the long-row attention;
 *   host_lengths : optional host int32 [n_news] copy of the row sums of `mask`.  With it the
 *               launch grids are exact; without it (NULL) grids cover n_news*padded_len tokens
 *               and surplus workgroups exit early.  No host synchronisation either way.  The lengths only
 *               size the chunks: the device derives its own from `mask`, and if the two disagree it raises
 *               MANNER_HIP_STATUS_LENGTHS and drops the tokens beyond the chunk's bound instead of writing
 *               past the workspace;
 *   out       : float32 [n_news, H].
 * News are processed in internal chunks that fit the workspace; padding tokens cost no FLOPs
 * (tokens are packed; SURVEY.md Q5 makes this equivalent to the padded reference computation). */
int manner_hip_encode_cls(manner_hip_encoder_t enc, const int64_t* ids, const int64_t* mask,
                          const int32_t* host_lengths /*host, nullable*/, int64_t n_news, int64_t padded_len,
                          int32_t precision, float* out, void* workspace, size_t workspace_bytes,
                          manner_hip_stream_t stream);

/* Hidden states after the first n_layers encoder layers — HF's hidden_states[n_layers] of the model built at
 * manner/models/components/news_encoder.py:20 (n_layers = 0: embedding output; = layers: last_hidden_state).
 * n_layers = 8 is the frozen / trainable boundary of the shipped configs (frozen_layers [0..7],
 * configs/model/cr_module.yaml:10; news_encoder.py:24-27): these activations do not change across training epochs and can
 * be cached per news — provided the embedding tables, which that name test does not freeze, are
 * not trained either.  Arguments as manner_hip_encode_cls; out [n_news, padded_len, H] of
 * out_dtype (0 = f32, 1 = bf16).  Rows of padded positions are written as zeros: HF computes throw-away values there
 * which never reach a real token (keys are masked) — feed the tensor with the same attention_mask.  padded_len up to
 * MANNER_HIP_MAX_LEN_INFER, as manner_hip_encode_cls. */
int manner_hip_encode_hidden(manner_hip_encoder_t enc, const int64_t* input_ids, const int64_t* attention_mask,
                             const int32_t* host_lengths, int64_t n_news, int64_t padded_len, int32_t precision,
                             int32_t n_layers, int32_t out_dtype, void* out, void* workspace, size_t workspace_bytes,
                             manner_hip_stream_t stream);

/* Blocking: synchronises `stream` and returns MANNER_HIP_E_INPUT if any encode_cls call on this
 * handle since the last status call saw an invalid mask (non-prefix, empty or longer than
 * MANNER_HIP_MAX_LEN_INFER) or token / position index; clears the flag. */
int manner_hip_encoder_status(manner_hip_encoder_t enc, manner_hip_stream_t stream);
/* Non-blocking form: enqueues a copy of the flag word into `host_flag` (pinned host int32) followed by its reset,
 * both on `stream`; the caller reads *host_flag once an event recorded after this call has completed.  This is how
 * the module mirror surfaces bad inputs of call k at call k+1 without a host synchronisation per forward. */
int manner_hip_encoder_status_async(manner_hip_encoder_t enc, int32_t* host_flag /*pinned host*/, manner_hip_stream_t stream);
/* Per-row token limits.  MANNER_HIP_MAX_LEN: the short-row attention tile (at most four 32-key tiles per wave).
 * MANNER_HIP_MAX_LEN_INFER: the inference entry points manner_hip_encode_cls / manner_hip_encode_hidden, whose rows of 129..512
 * tokens run the long-row attention kernels.  MANNER_HIP_MAX_LEN_TRAIN: manner_hip_train_forward / _backward, whose rows of
 * 129..512 tokens run the long-row training attention kernels (the rows of <= 128 tokens keep the short-row kernels and their bits).
 * MANNER_HIP_MAX_LEN_FULL: the "full rows" entry points (manner_hip_encode_full, manner_hip_train_full_*), padded_len <= 512; a
 * batch of more than 128 positions runs the row-block grid of the f32 attention kernels (fp32 mode) or the long-row matrix-pipe
 * kernels with a key count per news (f16 / bf16, head_dim 64); batches of <= 128 positions keep their kernels and their bits. */
#define MANNER_HIP_MAX_LEN 128
#define MANNER_HIP_MAX_LEN_INFER 512
#define MANNER_HIP_MAX_LEN_TRAIN 512
#define MANNER_HIP_MAX_LEN_FULL 512

/* ABI v8 — sampled fingerprint of a set of tensors, for hosts that cache copies of caller-owned parameters (the module mirror's
 * inference handle packs the PLM weights once; torch's version counters do not see a write through `p.data`).  out[i] = a 32-bit
 * hash of min(counts[i], samples) evenly strided 32-bit words of tensors[i] (first and last word included) mixed with counts[i]:
 * a bulk rewrite of a tensor (scaling, a copy, an optimiser step through .data) changes its word; a poke into single elements
 * between the samples does not — this is a tripwire, not a checksum.  tensors / counts / out are DEVICE arrays of n entries;
 * one launch, no host synchronisation. */
int manner_hip_fingerprint(const void* const* tensors /*device*/, const int64_t* counts /*device*/, int32_t n, int32_t samples,
                           uint32_t* out /*device*/, manner_hip_stream_t stream);

/* Optional per-kernel timing (the reference delegates profiling to Lightning's `profiler: simple`,
 * configs/trainer/default.yaml:21; this is the build's equivalent for the roofline report).
 * While enabled, every launch inside encode_cls is bracketed by hipEvents on the launch stream.
 * profile_read synchronises `stream`, adds the elapsed times into ms[MANNER_HIP_PROF_COUNT] and the
 * launch counts into launches[...] (host arrays, accumulated since the last read) and resets. */
enum {
  MANNER_HIP_PROF_LENGTHS = 0, MANNER_HIP_PROF_EMBED, MANNER_HIP_PROF_GEMM_QKV, MANNER_HIP_PROF_ATTENTION,
  MANNER_HIP_PROF_GEMM_OUT, MANNER_HIP_PROF_LAYERNORM, MANNER_HIP_PROF_GEMM_FFN1, MANNER_HIP_PROF_GEMM_FFN2,
  MANNER_HIP_PROF_GATHER, MANNER_HIP_PROF_CLS_TAIL /* last layer's [CLS]-row-only launches */,
  MANNER_HIP_PROF_COUNT
};
int manner_hip_encoder_profile(manner_hip_encoder_t enc, int32_t enable);
int manner_hip_encoder_profile_read(manner_hip_encoder_t enc, manner_hip_stream_t stream, double* ms /*host*/,
                                    int64_t* launches /*host*/);

/* ---------------------------------------------------------------- pooler (K11)
 * Replaces AdditiveAttention.forward — manner/models/components/attention.py:12-29 — and through
 * it NAMLUserEncoder.forward — manner/models/components/user_encoder.py:17-21.
 *   x [B,S,D] f32 contiguous; lin_w [Q,D]; lin_b [Q]; query [Q]; out [B,D] f32.
 * No padding mask, as in the reference.  scratch: B*S floats. */
int manner_hip_additive_pool(const float* x, const float* lin_w, const float* lin_b, const float* query,
                             int64_t B, int64_t S, int32_t D, int32_t Q, float* out, float* scratch,
                             manner_hip_stream_t stream);
/* ABI v5 — the same operator with ONE pass over x (csrc/pool.hip): the rows of x stay on the CU (registers, IEEE-half hi/lo pairs
 * under a power-of-two row scale = 22 significant bits) between the logits — split (x3) products on the f16 matrix pipe: W.hi x.hi +
 * W.hi x.lo + W.lo x.hi, f32 accumulation; tanh by exp / rcp — and the softmax-weighted sum; x is read from HBM once.  Pooled vectors
 * within 1e-4 of the reference (measured 2e-7 on tests/golden/additive_attention.npz incl. the zero-padded Q2 case, 1.1e-5 on a
 * peaked-softmax stress input).  Runs when D = 768 (S <= 128) or D = 1024 (S <= 64),
 * Q <= 320 and x / out are 16-byte aligned; otherwise — or with strict != 0, or MANNER_HIP_POOL_STRICT=1 in the environment — the
 * exact-f32 two-pass path of manner_hip_additive_pool runs (logits on the f32 matrix pipe, x read twice).
 *   workspace: manner_hip_additive_pool_workspace_bytes(B, S, D, Q) bytes, 256-byte aligned (packed W fragments / the logits). */
size_t manner_hip_additive_pool_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q);
int manner_hip_additive_pool_fused(const float* x, const float* lin_w, const float* lin_b, const float* query,
                                   int64_t B, int64_t S, int32_t D, int32_t Q, float* out, void* workspace,
                                   size_t workspace_bytes, int32_t strict, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- entity branch (K8)
 * manner_hip_entity_encode replaces MannerEntityEncoder.forward — manner/models/components/news_encoder.py:60-72:
 * Embedding -> nn.MultiheadAttention(D, heads) -> AdditiveAttention(D -> Q), eval mode.  BATCH-FAITHFUL
 * to the reference: the MHA is batch_first=False but receives [N, E, D], so attention
 * runs across the N news of the call at each entity slot, without key_padding_mask; the result for
 * a news depends on the other news of the call, exactly as in the reference.
 *   entity_ids int64 [N, E] (0 = padding slot, looked up like any other row); table f32 [n_entities, D];
 *   in_proj_w [3D, D], in_proj_b [3D], out_proj_w [D, D], out_proj_b [D] (nn.MultiheadAttention keys);
 *   pool_w [Q, D], pool_b [Q], pool_q [Q] (AdditiveAttention keys); out f32 [N, D].
 * manner_hip_linear replaces the nn.Linear(H + D -> H) on cat[text, entity] — news_encoder.py:109-113,
 * 122-124: y[R, O] = x[R, K] weight[O, K]^T + bias[O] (bias may be NULL). */
size_t manner_hip_entity_workspace_bytes(int64_t N, int64_t E, int32_t D);
int manner_hip_entity_encode(const int64_t* entity_ids, int64_t N, int64_t E, const float* table, int64_t n_entities,
                             int32_t D, int32_t heads, const float* in_proj_w, const float* in_proj_b,
                             const float* out_proj_w, const float* out_proj_b, const float* pool_w,
                             const float* pool_b, const float* pool_q, int32_t Q, float* out, void* workspace,
                             size_t workspace_bytes, int32_t* status /*device, nullable*/, manner_hip_stream_t stream);
int manner_hip_linear(const float* x, const float* weight, const float* bias, int64_t R, int32_t K, int32_t O,
                      float* y, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- scorer (K12, K9+K10+K12)
 * Replaces DotProduct.forward — manner/models/components/click_predictors.py:9-12:
 * out[b,c] = <user[b,:], cand[b,:,c]>.  `cand` is addressed with element strides so that the
 * reference call site's permuted view (manner/models/cr_module.py:127-129) is read in place. */
int manner_hip_dot(const float* user, const float* cand, int64_t B, int64_t C, int32_t D,
                   int64_t cand_stride_b, int64_t cand_stride_d, int64_t cand_stride_c,
                   float* out /*[B,C]*/, manner_hip_stream_t stream);

/* Fused late-fusion scorer over a news-embedding table: replaces the tail of CRModule.forward —
 * manner/models/cr_module.py:108-131 with late_fusion=True — and of
 * EnsembleModule._submodel_forward — manner/models/ensemble_module.py:116-135:
 * user_i = sum(table[hist_idx[hist_off[i]:hist_off[i+1]]]) / h_i ;
 * out[j] = <user_i, table[cand_idx[j]]> for j in [cand_off[i], cand_off[i+1]).
 * table f32 [n_rows, D] (D % 4 == 0, D <= 3072); idx int32; off int64 [B+1]; out f32 [cand_off[B]] (ragged order).
 * An index outside [0, n_rows) raises MANNER_HIP_STATUS_INDEX in *status (device int32, nullable) where the
 * reference's gather raises IndexError. */
int manner_hip_score_late_fusion(const float* table, int64_t n_rows, int32_t D,
                                 const int32_t* hist_idx, const int64_t* hist_off,
                                 const int32_t* cand_idx, const int64_t* cand_off, int64_t B,
                                 float* out, int32_t* status, manner_hip_stream_t stream);

/* The same scorer (same reference lines: cr_module.py:108-131, ensemble_module.py:116-135) over an IEEE-half copy of the
 * table, table16 [n_rows, D] (D % 8 == 0): half the bytes per gathered row, and a MIND-large table (161 013 x 768 = 247 MB)
 * that stays resident in the 256 MiB Infinity Cache.  Accumulation, the user vector and the scores are f32; only the
 * stored rows are rounded.  mean == NULL: table16 = half(T).  mean != NULL (f32 [D]): table16 = half(T - mean), the rows
 * centred on the table's column mean — the tables of one encoder are nearly collinear, so the deviations are an order of
 * magnitude smaller than the entries and the rounding error of the scores shrinks alike; the scores are reassembled
 * exactly (<mean + u', mean + c'> = <w, mean> + <w, c'>, w = mean + u').  For tables produced by the 16-bit encoder
 * modes; the fp32 parity mode keeps the f32 table.
 * manner_hip_table_to_f16 makes the copy; with mean != NULL it first computes the column mean into `mean` (workspace:
 * manner_hip_table_to_f16_workspace_bytes(D) bytes). */
int manner_hip_score_late_fusion_f16(const void* table16, const float* mean, int64_t n_rows, int32_t D,
                                     const int32_t* hist_idx, const int64_t* hist_off,
                                     const int32_t* cand_idx, const int64_t* cand_off, int64_t B,
                                     float* out, int32_t* status, manner_hip_stream_t stream);
size_t manner_hip_table_to_f16_workspace_bytes(int32_t D);
int manner_hip_table_to_f16(const float* table, int64_t n_rows, int32_t D, float* mean /*nullable*/, void* table16,
                            void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);

/* Same scorer with the user vectors given: the early-fusion tail of CRModule.forward —
 * manner/models/cr_module.py:125-129 (user_vector = user_encoder(...), then the click predictor) — on ragged
 * candidates: out[j] = <user[i, :], table[cand_idx[j]]> for j in [cand_off[i], cand_off[i+1]).  user f32 [B, D]. */
int manner_hip_score_user(const float* table, int64_t n_rows, int32_t D, const float* user,
                          const int32_t* cand_idx, const int64_t* cand_off, int64_t B, float* out,
                          int32_t* status, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- ragged -> dense (K9)
 * Replaces torch_geometric.utils.to_dense_batch at its call sites — manner/models/cr_module.py:108-110,114,142;
 * manner/models/ensemble_module.py:116-124,155-163: dense[b, j, :] = x[off[b] + j, :] for j < off[b+1] - off[b],
 * every other slot of row b = fill[b] (fill == NULL: 0, what to_dense_batch writes); mask[b, j] = 1 on real slots.
 * x f32 [off[B], D]; dense f32 [B, width, D]; mask uint8 [B, width] (nullable).  `width` comes from the caller
 * (the collate knows the batch maximum), so nothing is read back to the host; items beyond `width` are dropped.
 * `fill` carries the value the reference's dense ensemble matrix holds in padded slots (see zscore_fuse). */
int manner_hip_to_dense(const float* x, const int64_t* off, int64_t B, int64_t width, int32_t D, const float* fill,
                        float* dense, uint8_t* mask, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- ensemble (K13+K14)
 * Replaces the z-normalisation of EnsembleModule._submodel_forward —
 * manner/models/ensemble_module.py:138-149 — and the fusion of EnsembleModule.forward — :95-109:
 * out = z(scores[0]) + sum_{k>=1, w[k-1] != 0} w[k-1] * z(scores[k]), z per impression with the
 * unbiased std (c_i == 1 gives NaN, as torch.std does).
 * scores: K planes of f32 [total] at stride `plane_stride` elements; weights host f32 [K-1].
 * pad_value f32 [B] (nullable): the value the reference's dense [B, Cmax] result holds in the PADDED slots of row i —
 * its z-score runs over the whole zero-padded row (:145-149), so they become sum_k w_k (0 - mean_ik) / std_ik, not 0.
 * Feed it to manner_hip_to_dense as `fill` to reproduce the reference's matrix slot for slot. */
int manner_hip_zscore_fuse(const float* scores, int64_t plane_stride, int32_t K, const float* weights /*host*/,
                           const int64_t* cand_off, int64_t B, float* out, float* pad_value,
                           manner_hip_stream_t stream);

/* ---------------------------------------------------------------- ranking / nDCG (K15)
 * Replaces what RetrievalNormalizedDCG(top_k=k) computes per impression (constructed at
 * manner/models/cr_module.py:83-84, fed at :267-273): stable descending rank of each candidate.
 * topk_idx int32 [B,k]: position (within the impression) of the r-th ranked candidate, -1 padded.
 * ndcg f32 [B]: DCG@k/IDCG@k, 0 for impressions without a positive label.
 * mrr  f32 [B]: 1/(1 + rank of the best-ranked positive) over ALL candidates (RetrievalMRR, constructed at
 *               manner/models/cr_module.py:82), 0 without a positive.  Any output may be NULL. */
int manner_hip_rank_ndcg(const float* scores, const float* labels, const int64_t* cand_off, int64_t B,
                         int32_t k, int32_t* topk_idx, float* ndcg, float* mrr, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- Phase C in one launch (ABI v5)
 * EnsembleModule.forward over K per-module tables — manner/models/ensemble_module.py:95-151 — and the ranking consumer of
 * cr_module.py:267-273 in ONE kernel: for every impression gather-mean-dot against each active module's table (weights[k-1] == 0
 * skips module k as the reference does), per-impression z-score and weighted fusion (K == 1: the CR-Module's raw late-fusion scores,
 * cr_module.py:105-131), stable ranking, top-k, nDCG@k, MRR.  The K score planes stay in LDS.  BIT-IDENTICAL to
 * manner_hip_score_late_fusion x K -> manner_hip_zscore_fuse -> manner_hip_rank_ndcg (same code, same order of operations).
 *   tables: K HOST pointers to device tables f32 [n_rows, D] (D = 768 or 1024); weights: K-1 host floats; scores f32 [total_candidates]
 *   out; pad_value [B] or NULL; topk_idx int32 [B, k] or NULL; ndcg / mrr f32 [B] or NULL (need labels); workspace
 *   manner_hip_score_fuse_rank_workspace_bytes(K, total_candidates) bytes (touched only by impressions with more than 320 candidates). */
size_t manner_hip_score_fuse_rank_workspace_bytes(int32_t K, int64_t total_candidates);
int manner_hip_score_fuse_rank(const float* const* tables, int32_t K, const float* weights, int64_t n_rows, int32_t D,
                               const int32_t* hist_idx, const int64_t* hist_off, const int32_t* cand_idx, const int64_t* cand_off,
                               int64_t B, int64_t total_candidates, const float* labels, int32_t k, float* scores, float* pad_value,
                               int32_t* topk_idx, float* ndcg, float* mrr, void* workspace, size_t workspace_bytes, int32_t* status,
                               manner_hip_stream_t stream);

/* ---------------------------------------------------------------- aspect metrics
 * Replaces Diversity / Personalization @k — manner/metrics/functional.py:8-28, 31-62, 65-70 grouped per
 * impression as manner/metrics/base.py:92-129 and torchmetrics RetrievalMetric.compute do (constructed at
 * manner/models/ensemble_module.py:56-84).  topk_idx is the output of manner_hip_rank_ndcg for the same k.
 *   cand_aspect int32 [total candidates], hist_aspect int32 [total history] : class ids in [0, num_classes)
 *   diversity f32 [B]      : entropy of the class distribution of the top-k / ln(num_classes)
 *   personalization f32 [B]: generalised Jaccard of the top-k class counts vs the history class counts
 * Both are 0 for an impression whose candidate class ids sum to 0 (reference behaviour). Either may be NULL. */
int manner_hip_aspect_metrics(const int32_t* topk_idx, const int32_t* cand_aspect, const int32_t* hist_aspect,
                              const int64_t* cand_off, const int64_t* hist_off, int64_t B, int32_t k,
                              int32_t num_classes, float* diversity, float* personalization,
                              manner_hip_stream_t stream);

/* ---------------------------------------------------------------- global AUC
 * Replaces AUROC(task="binary") — constructed at manner/models/cr_module.py:81 (and ensemble_module.py), fed the
 * ragged preds / targets of every impression at cr_module.py:267-273; the arithmetic is torchmetrics'
 * (>=0.11.4, requirements.txt:4): ONE curve over all pairs of the run, not a per-impression mean.
 *   scores f32 [n], labels f32 [n] (positive iff > 0.5), n < 2^31.
 *   sigmoid_rule != 0 reproduces torchmetrics' format step: if any score lies outside [0, 1] every score is
 *   passed through the logistic function (f32) before thresholds are formed, so saturated scores tie.
 *   auc f64 [1] (device): (2U) / (2 P N), U = #(pos > neg) + #(pos == neg)/2, i.e. the trapezoid area through the
 *   distinct thresholds; 0 when there is no positive or no negative.
 *   counts int64 [3] (device, may be NULL): {2U, P, N} — exact integers, so ranks can be combined across
 *   shards only by re-running on the gathered scores (AUC does not decompose over impressions).
 * Either of auc / counts may be NULL, not both. */
size_t manner_hip_auc_workspace_bytes(int64_t n);
int manner_hip_auc(const float* scores, const float* labels, int64_t n, int32_t sigmoid_rule, void* workspace,
                   size_t workspace_bytes, double* auc, int64_t* counts, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- device-side collate
 * Replaces the per-step host work of MINDCollate.__call__ — manner/data/components/mind_rec_dataset.py:114-137
 * (pd.concat of the impressions' news rows + tokenizer call + padding) — and of MINDRecDatasetTest.__getitem__
 * (:87-99, DataFrame.loc per impression).  The news are tokenised ONCE into a device-resident store:
 *   store_ids int32 [n_news, Ls] (tokenizer output truncated to tokenizer_max_length), store_len int32 [n_news];
 *   store_ent int32 [n_news, Es] entity indices, store_cnt int32 [n_news]; category / sentiment int32 [n_news],
 *   sentiment_score f32 [n_news]  (columns of the parsed news frame, mind_dataframe.py:245-246).
 * `rows` int32 [M] are the store rows of the batch's concatenated history (or candidate) news.
 *   collate_segments: _make_batch_assignees (:171-174) — seg int64 [total] = repeat_interleave(arange(B), sizes)
 *                     from the int64 offsets [B+1] (this is MINDRecBatch.batch_hist / batch_cand).
 *   collate_text    : BatchEncoding of tokenizer(padding=True, truncation=True) (:134-137): ids / mask int64 [M, Lp],
 *                     Lp = longest news of the batch (the host knows the lengths), pad_id outside, mask 1/0.
 *   collate_entities: _tokenize_entities (:139-144): int64 [M, E], right-padded with 0 to the batch max E.
 *   collate_aspects : category / sentiment int64 [M], sentiment_score f32 [M] (:164-168); any output may be NULL. */
int manner_hip_collate_segments(const int64_t* off, int64_t B, int64_t total, int64_t* seg, manner_hip_stream_t stream);
int manner_hip_collate_text(const int32_t* store_ids, const int32_t* store_len, int64_t n_news, int32_t Ls,
                            const int32_t* rows, int64_t M, int32_t Lp, int32_t pad_id, int64_t* ids, int64_t* mask,
                            manner_hip_stream_t stream);
int manner_hip_collate_entities(const int32_t* store_ent, const int32_t* store_cnt, int64_t n_news, int32_t Es,
                                const int32_t* rows, int64_t M, int32_t E, int64_t* out, manner_hip_stream_t stream);
int manner_hip_collate_aspects(const int32_t* category, const int32_t* sentiment, const float* sentiment_score,
                               int64_t n_news, const int32_t* rows, int64_t M, int64_t* out_category,
                               int64_t* out_sentiment, float* out_score, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- training batches: negative sampling on the device
 * Replaces MINDRecDatasetTrain.__getitem__ / _sample_candidates — manner/data/components/mind_rec_dataset.py:13-77
 * (np.random.choice + np.random.permutation per impression, DataFrame.loc, pd.concat) — in front of the collate_* kernels.
 * The data set lives on the device as the CSR arrays of the behaviours: cand_rows int32 [total], labels f32 [total],
 * cand_off int64 [n_imp + 1] (history: hist_rows / hist_off alike), users int64 [n_imp].
 *
 * The sampling rule.  Positions 0..n-1 of an impression, P = positions with label == 1 (p of them), N = positions with
 * label == 0 (q of them; any other label is in neither set), m = ratio * p.  With 64-bit wrap-around arithmetic,
 *   mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *   key(stream, slot) = mix(mix(mix(seed + 0x9E3779B97F4A7C15 * (epoch + 1)) ^ imp) ^ (stream << 32 | slot))
 * where imp is the impression's index in the data set — so a sample depends on (seed, epoch, imp) only, never on the
 * batch, the place in it or the launch:
 *   m <= q: S = the m negatives with the smallest (key(0, position), position), in that order (without replacement);
 *   m >  q: draw t = 0..m-1 is the r-th negative in position order, r = ((key(1, t) >> 32) * q) >> 32 (with replacement);
 *   the list [P in position order, then S] is written in ascending order of (key(2, s), s), s = the element's place in it.
 *
 *   sample_candidates: one workgroup per batch impression b (imp_idx int64 [B], any order, repeats allowed) writes its
 *                      p * (1 + ratio) elements to out_rows / out_labels [out_off[b], out_off[b+1]) — out_off int64 [B + 1] is the
 *                      host's prefix sum, out_total = out_off[B] the length of the outputs.  out_pos (int32, may be NULL) receives
 *                      the chosen positions; users / out_users (int64 [n_imp] / [B], both or neither NULL) gather the impressions'
 *                      user indices in the same launch.  An imp_idx outside [0, n_imp) raises MANNER_HIP_STATUS_INDEX in *status; an
 *                      out_off segment that is not p * (1 + ratio) long or leaves [0, out_total], and p > 0 with q == 0 (where
 *                      np.random.choice raises), raise MANNER_HIP_STATUS_LENGTHS; such an impression writes nothing.
 *   gather_segments  : out[out_off[b] + k] = src[src_off[imp_idx[b]] + k] (src int32 [src_total], src_off int64 [n_seg + 1]); the f32
 *                      companion src_f / out_f is gathered alike (both NULL: none).  Flags as above (a segment whose length differs
 *                      from out_off's raises MANNER_HIP_STATUS_LENGTHS); a flagged element is written as 0.
 *   rows_max_len     : out_max[0] = max store_len[rows[r]], out_max[1] = max store_cnt[rows[r]] (0 for store_cnt == NULL or M == 0):
 *                      the padding=True widths of a sampled batch, for a caller that wants them exact.
 * status (device int32) may be NULL. */
int manner_hip_sample_candidates(const int32_t* cand_rows, const float* labels, const int64_t* cand_off, int64_t n_imp,
                                 int64_t total, const int64_t* users, const int64_t* imp_idx, int64_t B, const int64_t* out_off,
                                 int64_t out_total, int32_t ratio, uint64_t seed, uint64_t epoch, int32_t* out_rows,
                                 float* out_labels, int32_t* out_pos, int64_t* out_users, int32_t* status,
                                 manner_hip_stream_t stream);
int manner_hip_gather_segments(const int32_t* src, const float* src_f, const int64_t* src_off, int64_t n_seg, int64_t src_total,
                               const int64_t* imp_idx, int64_t B, const int64_t* out_off, int64_t out_total, int32_t* out,
                               float* out_f, int32_t* status, manner_hip_stream_t stream);
int manner_hip_rows_max_len(const int32_t* store_len, const int32_t* store_cnt, int64_t n_news, const int32_t* rows, int64_t M,
                            int32_t* out_max, manner_hip_stream_t stream);

/* ---------------------------------------------------------------- A-Module batches: M-per-class sampling on the device
 * Replaces pytorch_metric_learning's MPerClassSampler as MINDNewsDataModule uses it — manner/data/mind_news_datamodule.py:175-217,
 * MPerClassSampler(labels, m, batch_size, length_before_new_iter=len(data_train)) — in front of the collate_* kernels: a whole
 * epoch of news batches in one call.  The data set is N news with one aspect label each; the distinct labels in ascending value
 * are the classes 0..L-1 (class_label int64 [L]), class l has n_l = class_off[l+1] - class_off[l] members, and
 * class_members int32 [N] lists the data-set indices grouped by class, ascending inside a class (class_off int64 [L+1]);
 * rows int32 [N] maps a data-set index to its row of the news store.
 *
 * The sampling rule (documented behaviour of MPerClassSampler, not its random stream).  An epoch is nb batches of
 * B = k * m slots: k distinct classes chosen uniformly afresh for every batch, in random order, each filling a block of m
 * consecutive slots with m distinct members drawn uniformly — or, where the class has fewer than m members, with m draws with
 * replacement.  With key() of "training batches" above, its third argument now the batch or the unit, and two streams of its own:
 *   class choice of batch b: the k classes with the smallest (key(seed, epoch, b, 16, l), l), in that order;
 *   block j of batch b has unit = b * k + j, draws from its class of n members, h_t = key(seed, epoch, unit, 17, t) >> 32:
 *     n >= m (Floyd's subset algorithm): for t = 0..m-1: J = n - m + t, r = (h_t * (J + 1)) >> 32; append J if r was appended
 *             before, else r;
 *     n <  m: draw t is (h_t * n) >> 32;
 *   the block lists the drawn members in draw order.  That order is not a uniform permutation of the subset (Floyd's J can only
 *   appear at or after step t) and need not be: the supervised contrastive loss, the batch-coupled entity attention and the
 *   iid dropouts are equivariant to the order inside a batch.
 * A sample is a pure function of (seed, epoch, b, j) and the label array: no atomics, no stored keys, no dependence on the
 * launch geometry.
 *
 *   sample_m_per_class: out_idx int32 [nb * B] data-set indices, out_rows int32 [nb * B] their store rows, out_labels int64
 *                       [nb * B], out_width int32 [nb, 2] = per batch the longest stored token row and the longest entity list
 *                       among its rows (the padding=True widths; store_cnt == NULL: 0).  Bounds: 1 <= m <= 256,
 *                       1 <= k <= L <= 1024, 1 <= N < 2^31, nb * k * m < 2^31 — anything else is MANNER_HIP_E_INVALID before
 *                       any launch.  A rows entry outside [0, n_news), a member outside [0, N) or a class without members raises
 *                       MANNER_HIP_STATUS_INDEX in *status (device int32, may be NULL); the slot is then written with the index
 *                       clamped into its table. */
int manner_hip_sample_m_per_class(const int64_t* class_off, const int32_t* class_members, const int64_t* class_label, int32_t L,
                                  int64_t N, const int32_t* rows, const int32_t* store_len, const int32_t* store_cnt, int64_t n_news,
                                  int32_t m, int32_t k, int64_t nb, uint64_t seed, uint64_t epoch, int32_t* out_idx,
                                  int32_t* out_rows, int64_t* out_labels, int32_t* out_width, int32_t* status,
                                  manner_hip_stream_t stream);

/* ---------------------------------------------------------------- evaluation loss (val/loss, test/loss)
 * Replaces the loss of CRModule.model_step — manner/models/cr_module.py:140-171, run by validation_step and test_step
 * (:211-262) on every batch — per impression, on the ragged scores (no dense [B, Cmax] matrix, no host loops).
 *   mode 0 (supcon_loss: True, configs/model/cr_module.yaml:4): the reference's SupConLoss on the score matrix
 *           (manner/models/components/losses.py:12-40): losses[i] = -sum_{j positive}(s_j/T - logsumexp_{j real} s_j/T)
 *           / (n_pos + FLT_MIN); 0 for an impression without a positive.  The batch value is the reducer's job
 *           (pytorch_metric_learning default for SupConLoss: mean over the non-zero entries).
 *   mode 1 (supcon_loss: False): nn.CrossEntropyLoss(scores [B, c_max], y_true [B, c_max]) with probability targets —
 *           the c_max - c_i zero-padded scores of the dense row take part in the softmax, as in the reference;
 *           losses[i] = -sum_j y_ij log_softmax(row_i)_j, batch value = mean.  temperature is ignored (pass 1).
 * scores / labels f32 [cand_off[B]], cand_off int64 [B+1], losses f32 [B]. */
int manner_hip_eval_loss(const float* scores, const float* labels, const int64_t* cand_off, int64_t B, int32_t mode,
                         float temperature, int64_t c_max, float* losses, manner_hip_stream_t stream);

/* ---- the training path of MannerTextEncoder (train.hip) -------------------------------------------------
 * Replaces, for the CR-/A-Module training step (manner/models/cr_module.py:140-171 -> news_encoder.py:29-37 in train()
 * mode, then loss.backward()): the HF BertModel / RobertaModel forward WITH its dropouts (embeddings, attention
 * probabilities, attention output, FFN output: modeling_bert.py:107,140,183,351), MannerTextEncoder's own dropout on the
 * [CLS] vector (news_encoder.py:35), and the autograd backward down to the parameter gradients.
 *
 *   weights : HOST array of n_weights device pointers (f32, the order of manner_hip_encoder_create) — the live master
 *             parameters, read at every call (nothing is cached between optimiser steps);
 *   ids / mask / n_news / padded_len : as manner_hip_encode_cls, padded_len <= MANNER_HIP_MAX_LEN_TRAIN (512); every row must
 *             also fit the model's position table (MANNER_HIP_STATUS_TOKEN otherwise).  Rows of more than MANNER_HIP_MAX_LEN (128)
 *             tokens run the long-row attention kernels (one workgroup per news, head and block of queries or keys);
 *             `saved` and `workspace` stay per token (nothing of size tokens^2 is stored);
 *   m_bound : rows every activation buffer holds: a multiple of 256, >= the number of real tokens (n_news * padded_len
 *             rounded up always works; a device-side check raises MANNER_HIP_STATUS_LENGTHS otherwise);
 *   precision : MANNER_HIP_PREC_F32 (f32 MFMA GEMMs) or _F16 / _BF16 (GEMM operands rounded to 16 bits, f32 accumulation,
 *             f32 activations — "16-mixed"); activations, gradients and everything that is not a GEMM are f32;
 *   start_layer / prefix_hidden : 0 / NULL runs embeddings + all layers in training mode.  start_layer = f > 0 starts
 *             from prefix_hidden = hidden_states[f] ([n_news, padded_len, H] f32, e.g. manner_hip_encode_hidden of the
 *             frozen layers) — valid when no tensor below layer f receives a gradient;
 *   p_hidden / p_attn / p_out : hidden_dropout_prob, attention_probs_dropout_prob, MannerTextEncoder.dropout.p; 0 = off;
 *   seed    : dropout masks are a pure function of (seed, site, element index); the backward call must repeat the
 *             forward call's seed and probabilities.  manner_hip_dropout_mask returns the keep-bits of one site
 *             (site 0: embeddings over [m, H]; 1: [CLS] output over [n_news, H]; 8*(layer+1)+0: attention
 *             probabilities over [(m*heads + head)*256 + key] for a query row m of a news of <= 128 tokens, and — a stream
 *             of its own — site (8*(layer+1)) | 0x80000000 over [((m*heads + head) << 9) + key] for a news of 129..512 tokens;
 *             +1: attention output; +2: FFN output, over [m, H]);
 *   saved   : manner_hip_train_saved_bytes(cfg, n_news, m_bound, start_layer) bytes that carry the activations from the
 *             forward to the backward call;  workspace: manner_hip_train_workspace_bytes(cfg, m_bound) bytes of scratch;
 *   cls_out : f32 [n_news, H].
 * Backward: grad_cls f32 [n_news, H]; grads = HOST array of n_weights device pointers, NULL where no gradient is
 * wanted (requires_grad = False; a LayerNorm's weight and bias come together); each non-NULL tensor is OVERWRITTEN with
 * d loss / d parameter.  The activation gradient travels as far down as a requested gradient needs — through frozen
 * layers into the embedding tables when an embedding tensor is trainable, which is the reference's default
 * (news_encoder.py:24-27 freezes "layer.N." parameters only).  grad_prefix (optional, start_layer > 0): f32
 * [n_news, padded_len, H] gradient of prefix_hidden.  Embedding-table gradients: up to 8192 padded positions (n_news * padded_len — an
 * A-Module step) every table row is summed by one workgroup in position order, the same bits on every run; larger batches use f32
 * atomics (summation order, hence the last bits, vary between runs — as torch's CUDA embedding backward). */
size_t manner_hip_train_saved_bytes(const manner_hip_encoder_config* cfg, int64_t n_news, int64_t m_bound, int32_t start_layer);
size_t manner_hip_train_workspace_bytes(const manner_hip_encoder_config* cfg, int64_t m_bound);
/* ABI v7 — the bytes manner_hip_train_forward needs for `saved` IN THE GIVEN PRECISION (never more than the function above, which
 * stays valid for every mode).  Round 5: in the 16-bit modes the tensors that only GEMMs and the attention consume — Q | K | V, the
 * attention output, the FFN pre-activation and its gelu — are saved in the 16-bit type alone (what the reference's
 * `precision: 16-mixed` autocast keeps: configs/trainer/default.yaml:12), 31 instead of 49 KB per token and layer for bert-base.
 * Evaluate it right before the forward call: the layout follows the same rule the forward applies (matrix-pipe attention and fused
 * GeLU epilogues available for the shape; MANNER_HIP_TRAIN_SAVE16=0 keeps the f32 layout); a forward whose rule asks for more than
 * it was given fails with MANNER_HIP_E_WORKSPACE, it never overruns. */
size_t manner_hip_train_saved_bytes_for(const manner_hip_encoder_config* cfg, int64_t n_news, int64_t m_bound, int32_t start_layer,
                                        int32_t precision);
/* ABI v5 — optional cache of the 16-bit weight copies the 16-bit training modes make on every call (round 4).  Registers, for the NEXT
 * manner_hip_train_forward / _backward call of THIS thread (consumed by it; ignored in fp32 mode), 2 * n_weights caller-owned device
 * buffers (host array `slots`, entries may be NULL = not cached) and as many host flags `valid` (in / out):
 *   slot 2 i     the mode's 16-bit copy of weight i of the table, same layout          (read by the forward GEMMs)
 *   slot 2 i + 1 the 16-bit copy of its transpose                                      (read by the data-gradient GEMMs)
 *   at a layer's query weight: the packed [3H, H] Q | K | V copy / its [H, 3H] transpose; at its query bias, slot 2 i: f32 [3H] biases.
 * valid[s] == 0: the library fills slot s on first use and sets the flag; != 0: it reads the slot and launches nothing.  Meant for
 * FROZEN weights (reference news_encoder.py:24-27 freezes layers by name): the caller clears a flag when the weight's contents change
 * and keeps the buffers alive until the stream has passed the call.  slots == NULL: no cache (the default). */
int manner_hip_train_weight_cache(void* const* slots /*host*/, int32_t* valid /*host, in/out*/, int32_t n_slots);
int manner_hip_train_forward(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/, int32_t n_weights,
                             const int64_t* ids, const int64_t* mask, int64_t n_news, int64_t padded_len, int64_t m_bound,
                             int32_t precision, int32_t start_layer, const float* prefix_hidden, float p_hidden, float p_attn,
                             float p_out, uint64_t seed, float* cls_out, void* saved, size_t saved_bytes, void* workspace,
                             size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_train_backward(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/, int32_t n_weights,
                              const int64_t* ids, int64_t n_news, int64_t padded_len, int64_t m_bound, int32_t precision,
                              int32_t start_layer, float p_hidden, float p_attn, float p_out, uint64_t seed,
                              const float* grad_cls, void* saved, size_t saved_bytes, float* const* grads /*host*/,
                              float* grad_prefix, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
/* ABI v8 — the layout of `saved` travels WITH the call pair instead of being guessed.  manner_hip_train_layout_last() returns the
 * layout word of the most recent successful manner_hip_train_forward / _full_forward of THIS thread (bit 0: attention on the matrix
 * pipe with 16-bit Q | K | V, bit 1: 16-bit-only saved activations; -1: no forward yet); manner_hip_train_layout_next(word) hands it
 * to the NEXT manner_hip_train_backward / _full_backward of this thread (consumed by it, like manner_hip_train_weight_cache).  A host
 * keeps the word next to the saved buffer (the mirror: in the autograd ctx).  A backward that gets no word falls back to the
 * per-address record its forward left in this process image; one that finds neither FAILS with MANNER_HIP_E_INVALID rather than
 * deriving a layout from the environment of the moment (which may differ from the forward's and would plan other slot offsets). */
int32_t manner_hip_train_layout_last(void);
int manner_hip_train_layout_next(int32_t word);
int manner_hip_dropout_mask(uint64_t seed, uint32_t site, float p, int64_t n, uint8_t* keep, manner_hip_stream_t stream);

/* The same training path with "full rows" — the PLM inside PLMTextEncoder in train() mode (manner/models/components/
 * news_encoder.py:132-171: `self.plm_model(**tokenized_text)[0]` = HF last_hidden_state, whose PADDED positions the
 * reference's un-masked MultiheadAttention / AdditiveAttention mix into the result; trained by baselines/
 * nrms_plm_module.py:119-135): every position of the padded batch is a row (m = n_news * padded_len), the real tokens
 * of a news are its attention keys, padded positions embed the pad token (RoBERTa: at position pad_id) and still
 * produce outputs, no layer is pruned to the [CLS] rows.  hidden / grad_hidden: f32 [n_news * padded_len, H] (row
 * n * padded_len + t); padded_len <= MANNER_HIP_MAX_LEN_FULL (512), and every position must fit the model's position table
 * (MANNER_HIP_STATUS_TOKEN otherwise).  saved: manner_hip_train_saved_bytes(cfg, n_news, M, 0) (the upper bound of every layout),
 * workspace: manner_hip_train_workspace_bytes(cfg, M), M = n_news * padded_len rounded up to 256 — both per token, nothing of
 * size padded_len x padded_len is stored.  In f16 / bf16 a batch of more than 128 positions runs the long-row matrix-pipe
 * attention (queries = every position, keys = the real tokens; MANNER_HIP_TRAIN_ATTN_VALU=1 keeps the f32 kernels); the layout
 * word of the forward says which, and the backward follows it.  Dropout sites and the grads
 * table as in manner_hip_train_forward / _backward (there is no [CLS] dropout here: the caller owns what follows). */
int manner_hip_train_full_forward(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/, int32_t n_weights,
                                  const int64_t* ids, const int64_t* mask, int64_t n_news, int64_t padded_len, int32_t precision,
                                  float p_hidden, float p_attn, uint64_t seed, float* hidden, void* saved, size_t saved_bytes,
                                  void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_train_full_backward(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/, int32_t n_weights,
                                   const int64_t* ids, int64_t n_news, int64_t padded_len, int32_t precision, float p_hidden,
                                   float p_attn, uint64_t seed, const float* grad_hidden, void* saved, size_t saved_bytes,
                                   float* const* grads /*host*/, void* workspace, size_t workspace_bytes,
                                   manner_hip_stream_t stream);

/* The rest of the training step (cr_module.py:105-171), f32, ragged order:
 *  - late-fusion scorer on the vectors of every occurrence (training encodes x_hist / x_cand per impression, :107-113):
 *    user_i = mean(hist rows of i) (:116-123), scores_j = <user_i, cand_j> (:127-129); backward: d hist, d cand.
 *    hist f32 [hist_off[B], D], cand f32 [cand_off[B], D], user f32 [B, D] (kept for the backward), scores f32 [cand_off[B]];
 *  - DotProduct backward for the drop-in click predictor (click_predictors.py:9-12): grad_user [B, D], grad_cand
 *    CONTIGUOUS [B, D, C] (the shape of the permuted view the reference passes);
 *  - the loss of model_step (:140-171) with its gradient: mode / temperature / c_max as manner_hip_eval_loss;
 *    losses f32 [B]; loss_and_scale f32 [2] = {batch loss, reducer factor} — SupCon: mean over the non-zero
 *    per-impression losses (pytorch_metric_learning AvgNonZeroReducer); CE: mean; grad_scores f32 [cand_off[B]] =
 *    d loss / d scores (ragged order). */
int manner_hip_late_fusion_train_forward(const float* hist, const int64_t* hist_off, const float* cand, const int64_t* cand_off,
                                         int64_t B, int32_t D, float* user, float* scores, manner_hip_stream_t stream);
int manner_hip_late_fusion_train_backward(const float* grad_scores, const float* user, const int64_t* hist_off, const float* cand,
                                          const int64_t* cand_off, int64_t B, int32_t D, float* grad_hist, float* grad_cand,
                                          manner_hip_stream_t stream);
int manner_hip_dot_backward(const float* grad_out, const float* user, const float* cand, int64_t B, int64_t C, int32_t D,
                            int64_t cand_stride_b, int64_t cand_stride_d, int64_t cand_stride_c, float* grad_user,
                            float* grad_cand, manner_hip_stream_t stream);
int manner_hip_train_loss(const float* scores, const float* labels, const int64_t* cand_off, int64_t B, int32_t mode,
                          float temperature, int64_t c_max, float* losses, float* loss_and_scale, float* grad_scores,
                          manner_hip_stream_t stream);

/* The A-Module's loss (manner/models/a_module.py:73-75,102-108): pytorch_metric_learning (>= 2.1.1, requirements.txt:6 — not
 * vendored by the reference; restated) SupConLoss(temperature, distance=DotProductSimilarity(normalize_embeddings=False)) on the
 * news embeddings emb f32 [N, D] and their aspect labels int64 [N]: mat = emb emb^T / T; positives of anchor i = other news
 * with its label, negatives = news with another label; losses[i] = -sum_pos(m_ij - logsumexp_{j != i} m_ij) / (n_pos + FLT_MIN);
 * loss_and_scale = {mean over the losses > 0 (AvgNonZeroReducer), its factor}; all zero when the batch holds no positive or no
 * negative pair.  grad_emb f32 [N, D] = d loss / d emb.  workspace: manner_hip_supcon_embeddings_workspace_bytes(N). */
size_t manner_hip_supcon_embeddings_workspace_bytes(int64_t N);
int manner_hip_supcon_embeddings(const float* emb, const int64_t* labels, int64_t N, int32_t D, float temperature, float* losses,
                                 float* loss_and_scale, float* grad_emb, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);

/* The small operators of the training step (train_small.hip; f32): what autograd needs below and beside the text encoder
 * for the reference's default `use_entities: True` (configs/model/cr_module.yaml:13) and for early fusion —
 *  - manner_hip_linear_backward: nn.Linear (news_encoder.py:110-113 `linear` on cat[text, entity]; the projections of
 *    nn.MultiheadAttention; AdditiveAttention.linear): y = x W^T + b, x [R, K], W [O, K]; any of grad_x / grad_w /
 *    grad_b may be NULL; add_to_dx (nullable) [R, K] is added into grad_x;
 *  - manner_hip_additive_pool_backward: AdditiveAttention.forward (attention.py:21-27) — grad_x [B, S, D], grad_w [Q, D],
 *    grad_b [Q], grad_q [Q] from grad_out [B, D]; workspace manner_hip_additive_pool_backward_workspace_bytes;
 *  - manner_hip_axis0_attention(_backward): the attention core of nn.MultiheadAttention(batch_first=False) as the reference
 *    calls it (quirk Q1: along axis 0 of [L0, B1, E], per position B1 and head, no mask, no attention dropout) on projected
 *    qkv [L0, B1, 3E] = [q | k | v]; backward: grad_qkv [L0, B1, 3E] from grad_out [L0, B1, E], stats = L0*B1*heads*3 floats of scratch;
 *  - manner_hip_embedding(_backward): nn.Embedding.from_pretrained(..., freeze=False, padding_idx=0) (news_encoder.py:99-103):
 *    lookup, and grad_table [n_rows, D] (overwritten; row padding_idx receives no gradient; up to 8192 ids each row is summed in id
 *    order by one workgroup, the same bits on every run; more ids use f32 atomics);
 *  - manner_hip_dropout: out = keep ? x / (1 - p) : 0 over a flat tensor with the training path's generator (its own
 *    backward: apply it to the gradient with the same seed / site). */
int manner_hip_linear_backward(const float* x, const float* weight, const float* grad_y, int64_t R, int32_t K, int32_t O,
                               const float* add_to_dx, float* grad_x, float* grad_w, float* grad_b, manner_hip_stream_t stream);
size_t manner_hip_additive_pool_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q);
int manner_hip_additive_pool_backward(const float* x, const float* lin_w, const float* lin_b, const float* query, const float* grad_out,
                                      int64_t B, int64_t S, int32_t D, int32_t Q, float* grad_x, float* grad_w, float* grad_b,
                                      float* grad_q, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
int manner_hip_axis0_attention(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, manner_hip_stream_t stream);
int manner_hip_axis0_attention_backward(const float* qkv, const float* grad_out, int64_t L0, int64_t B1, int32_t E, int32_t heads,
                                        float* grad_qkv, float* stats, manner_hip_stream_t stream);
int manner_hip_embedding(const int64_t* ids, int64_t R, const float* table, int64_t n_rows, int32_t D, float* out, int32_t* status,
                         manner_hip_stream_t stream);
int manner_hip_embedding_backward(const int64_t* ids, int64_t R, const float* grad_out, int64_t n_rows, int32_t D, int64_t padding_idx,
                                  float* grad_table, manner_hip_stream_t stream);
int manner_hip_dropout(const float* x, float* out, int64_t n, uint64_t seed, uint32_t site, float p, manner_hip_stream_t stream);

/* ---- the PLM baseline encoders (f32 activations; not on the throughput path) ------------------------------
 * manner_hip_encode_full replaces `self.plm_model(**tokenized_text)[0]` of PLMTextEncoder.forward
 * (manner/models/components/news_encoder.py:158-160): HF last_hidden_state f32 [n_news, padded_len, H] INCLUDING the padded
 * positions — they embed the pad token (RoBERTa: at position pad_id), attend over the real keys only, and the consumer
 * below mixes them into real tokens.  weights / precision / status as manner_hip_train_forward; padded_len <=
 * MANNER_HIP_MAX_LEN_FULL (512), every position within the model's position table (MANNER_HIP_STATUS_TOKEN otherwise).  In
 * f16 / bf16 a batch of more than 128 positions takes the long-row matrix-pipe forward kernel of the training path (p = 0).
 * manner_hip_mha_axis0 replaces nn.MultiheadAttention(embed_dim=E, num_heads=heads) as the reference calls it —
 * batch_first=False on a [batch, seq, E] tensor, no masks (news_encoder.py:163-165; user_encoder.py:35-37): attention along
 * AXIS 0 of x [L0, B1, E] (across the news / users of the call, independently per position B1), in/out projections included.
 * in_proj_w [3E, E], in_proj_b [3E], out_proj_w [E, E], out_proj_b [E]; out [L0, B1, E]; eval mode (no dropout). */
size_t manner_hip_encode_full_workspace_bytes(const manner_hip_encoder_config* cfg, int64_t n_news, int64_t padded_len);
int manner_hip_encode_full(const manner_hip_encoder_config* cfg, const float* const* weights /*host*/, int32_t n_weights,
                           const int64_t* ids, const int64_t* mask, int64_t n_news, int64_t padded_len, int32_t precision,
                           float* hidden, void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
size_t manner_hip_mha_axis0_workspace_bytes(int64_t L0, int64_t B1, int32_t E);
int manner_hip_mha_axis0(const float* x, int64_t L0, int64_t B1, int32_t E, int32_t heads, const float* in_proj_w,
                         const float* in_proj_b, const float* out_proj_w, const float* out_proj_b, float* out, void* workspace,
                         size_t workspace_bytes, manner_hip_stream_t stream);

/* ---- the MINER baseline's operators (csrc/poly.hip; f32, forward and backward; additive exports) -------------------------------------
 * manner_hip_poly_attention replaces PolyAttention.forward (manner/models/components/attention.py:60-84): x [B, S, D],
 * mask uint8 / bool [B, S], lin_w [Q, D] (no bias), codes [K, Q], bias f32 [B, S, T] or NULL; out [B, K, D] =
 * softmax_s(tanh(x W^T) codes^T + mean_t bias) x.  As in the reference a masked slot's logit is 1e-30 (not -inf: it stays in the
 * softmax) and the bias mean runs over all T columns.  S <= 256, K <= 64, Q <= 512, D <= 1024 (MANNER_HIP_E_INVALID otherwise).
 * _backward: grad_x [B, S, D] (weighted-sum and projection routes), grad_w [Q, D], grad_codes [K, Q] from grad_out [B, K, D]; masked
 * slots' logits receive no gradient; no gradient for bias.
 * manner_hip_target_attention replaces TargetAwareAttention.forward (attention.py:102-116): query [B, K, D], key [B, C, D],
 * value [B, C, K], lin_w [D, D] (no bias); out [B, C] = sum_k softmax_k(key . gelu(query W^T)^T) value.  K <= 64, D <= 1024.
 * _backward: grad_query, grad_key, grad_value, grad_w from grad_out [B, C].
 * manner_hip_bmm is DotProduct.forward (click_predictors.py:9-12) for M > 1 rows, as MINERModule.forward calls it
 * (baselines/miner_module.py:195-198): out [B, M, N] = a [B, M, D] . b [B, D, N], b by element strides (read in place).
 * _backward: grad_a [B, M, D], grad_b CONTIGUOUS [B, D, N].
 * Every reduction across rows has a fixed order (no floating-point atomics).  Workspaces: the *_workspace_bytes queries. */
size_t manner_hip_poly_attention_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K);
int manner_hip_poly_attention(const float* x, const uint8_t* mask, const float* lin_w, const float* codes, const float* bias, int64_t T,
                              int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K, float* out, void* workspace, size_t workspace_bytes,
                              manner_hip_stream_t stream);
size_t manner_hip_poly_attention_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K);
int manner_hip_poly_attention_backward(const float* x, const uint8_t* mask, const float* lin_w, const float* codes, const float* bias, int64_t T,
                                       const float* grad_out, int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K, float* grad_x, float* grad_w,
                                       float* grad_codes, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_target_attention_workspace_bytes(int64_t B, int32_t K, int32_t D);
int manner_hip_target_attention(const float* query, const float* key, const float* value, const float* lin_w, int64_t B, int64_t C, int32_t K,
                                int32_t D, float* out, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_target_attention_backward_workspace_bytes(int64_t B, int32_t K, int32_t D);
int manner_hip_target_attention_backward(const float* query, const float* key, const float* value, const float* lin_w, const float* grad_out,
                                         int64_t B, int64_t C, int32_t K, int32_t D, float* grad_query, float* grad_key, float* grad_value,
                                         float* grad_w, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
int manner_hip_bmm(const float* a, const float* b, int64_t B, int64_t M, int64_t N, int32_t D, int64_t b_stride_b, int64_t b_stride_d,
                   int64_t b_stride_n, float* out, manner_hip_stream_t stream);
int manner_hip_bmm_backward(const float* grad_out, const float* a, const float* b, int64_t B, int64_t M, int64_t N, int32_t D, int64_t b_stride_b,
                            int64_t b_stride_d, int64_t b_stride_n, float* grad_a, float* grad_b, manner_hip_stream_t stream);

/* ---- MINERModule's own lines (csrc/miner.hip; f32; additive exports) --------------------------------------------------------------
 * What baselines/miner_module.py:153-242 computes between the operators above, without the [N_hist, N_cand] cosine matrix, the
 * [B, S, N_cand] dense bias, the per-impression host loop, the [B, C, K] product and the [B, K, K] Gram matrix.
 * manner_hip_miner_category_bias (miner_module.py:162-181 with attention.py:75): hist_cat int64 [N_hist], cand_cat int64 [T], the frozen
 * category table f32 [V, Dc], hist_off / cand_off int64 [B + 1]; bias f32 [B, S] (hand it to manner_hip_poly_attention as [B, S, 1],
 * T = 1) with bias[b, s] = (1 / T) sum over the candidates t of the batch that are NOT user b's own of cos(x_{b,s}, y_t) — T counts
 * ALL candidates, the own columns are zeroed and still counted, cos divides by the norms themselves (torchmetrics: no epsilon, so an
 * all-zero row gives NaN wherever it is summed), a padded slot s >= h_b and an empty exclusion set are exactly 0.  The unit candidate
 * rows outside the user's own are summed directly in ascending t, then one dot product per slot.  p > 0: nn.Dropout on the embedded
 * rows by the counter rule of the training path, element (row of its side) * Dc + d, history at (seed_hist, site_hist), candidates at
 * (seed_cand, site_cand).  Dc <= 1024, S <= 256 (MANNER_HIP_E_INVALID otherwise); a category id outside [0, V) is never read and raises
 * MANNER_HIP_STATUS_INDEX in `status` (may be NULL).  No gradient: the embedding is frozen.
 * manner_hip_miner_code_scores (miner_module.py:195-202): cand [N, D] ragged by cand_off [B + 1], user [B, K, D]; out [N] =
 * max_k (mode 0) or mean_k (mode 1) of cand[t] . user[b, k] — the dot products and the reduction in one kernel.  argmax int32 [N] (may be
 * NULL; mode 0) receives the winning code, ties to the LOWEST index (torch's max(dim) on the CPU).  _backward: grad_cand [N, D] and
 * grad_user [B, K, D] from grad_out [N]: to the argmax code (mode 0, `argmax` of the forward) or spread evenly over the K codes (mode
 * 1); grad_user is a sum over the user's candidates in ascending order.  K <= 64, D <= 1024.
 * manner_hip_disagreement_loss (miner_module.py:237-241, components/utils.py:4-31 with zero_diagonal=True, then .mean()): user
 * [B, K, D] -> loss [1] = (1 / (B K K)) sum_b sum_{i != j} u_i . u_j, u = x / (1e-8 + ||x||) (a zero row is 0).  workspace: 8-byte
 * aligned.  _backward: grad_user [B, K, D] from the DEVICE scalar grad_loss [1]; a zero row gets the finite gradient through 1 / 1e-8
 * that torch autograd gives.  K <= 64, D <= 1024.  Every reduction has a fixed order (no floating-point atomics). */
size_t manner_hip_miner_category_bias_workspace_bytes(int64_t n_hist, int64_t T, int64_t B, int32_t Dc);
int manner_hip_miner_category_bias(const int64_t* hist_cat, const int64_t* cand_cat, const float* table, int64_t V, int32_t Dc,
                                   const int64_t* hist_off, const int64_t* cand_off, int64_t n_hist, int64_t T, int64_t B, int64_t S, float p,
                                   uint64_t seed_hist, uint64_t seed_cand, uint32_t site_hist, uint32_t site_cand, float* bias, void* workspace,
                                   size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_miner_code_scores(const float* cand, const int64_t* cand_off, const float* user, int64_t N, int64_t B, int32_t K, int32_t D,
                                 int32_t mode, float* out, int32_t* argmax, manner_hip_stream_t stream);
int manner_hip_miner_code_scores_backward(const float* grad_out, const float* cand, const int64_t* cand_off, const float* user,
                                          const int32_t* argmax, int64_t N, int64_t B, int32_t K, int32_t D, int32_t mode, float* grad_cand,
                                          float* grad_user, manner_hip_stream_t stream);
size_t manner_hip_disagreement_loss_workspace_bytes(int64_t B);
int manner_hip_disagreement_loss(const float* user, int64_t B, int32_t K, int32_t D, float* loss, void* workspace, size_t workspace_bytes,
                                 manner_hip_stream_t stream);
int manner_hip_disagreement_loss_backward(const float* user, const float* grad_loss, int64_t B, int32_t K, int32_t D, float* grad_user,
                                          manner_hip_stream_t stream);

/* ---- the auxiliary heads and losses of TANR-PLM and SentiRec-PLM (csrc/aspect.hip; f32; additive exports) -------------------------
 * What baselines/tanr_plm_module.py:139-141,172-177 and baselines/sentirec_plm_module.py:141-143,174-193 compute over the news rows of a
 * batch, without the torch.cat, the one-hot matrix, the dense [B, Cmax] blocks and the per-impression host loop.
 * manner_hip_head_ce: x [N, D], w [O, D], b [O], target int64 [N] (plain class indices) -> loss [1] = the mean over the N rows of
 * -log softmax(x w^T + b)[target]: nn.Linear, the row softmax, the log and the row loss in ONE launch — the weight staged once per
 * workgroup (LDS, up to 128 KB; a larger one is read through L2) under a grid-stride walk of the rows — and one small launch for the
 * fixed-order mean.  `logits` (may be NULL) receives [N, O]; nothing of that size is written otherwise but `saved` [N, O] = p - y (may
 * be NULL when no backward follows).  The rows may come in any order with their targets in the same order: the mean is symmetric.
 * O <= 64, D <= 1024 (MANNER_HIP_E_INVALID otherwise); N == 0 is MANNER_HIP_E_INVALID (the mean of nothing).  A target outside [0, O)
 * — where F.one_hot raises — is never used as an index: it raises MANNER_HIP_STATUS_INDEX in `status` (may be NULL) and its row counts
 * as loss 0 and gradient 0.
 * manner_hip_head_ce_backward: from the DEVICE scalar grad_loss [1] and the forward's `saved`, grad_x [N, D], grad_w [O, D] and
 * grad_b [O]; each may be NULL (a frozen head, rows that need no gradient) and its work is then skipped.  grad_w / grad_b are partial
 * sums over chunks of ascending rows added in ascending chunk order; `workspace` (_backward_workspace_bytes) is read only for them.
 * manner_hip_head_l1 / _backward: the O == 1 case of the same row walk with nn.L1Loss: w [D], b [1], target f32 [N] -> loss [1] =
 * mean |x . w + b - target|; `saved` [N] = sign(residual) with sign(0) = 0 as torch: a row that meets its target exactly sends no
 * gradient.
 * manner_hip_senti_div (sentirec_plm_module.py:180-193): the RAGGED scores [T] and candidate sentiment scores [T], the history
 * sentiment scores [N_hist], hist_off / cand_off int64 [B + 1], c_max = the dense width Cmax -> loss [1] =
 * (1 / (B c_max)) sum_b sum_c relu(u_b s_bc score_bc), u_b = (the sum of user b's history scores, ascending) / its history length.
 * Padded slots add 0 and are counted in the divisor.  A user without history has u = 0 / 0: the loss is NaN as in the reference, and so
 * are the gradients of that user's candidates, and only those.  c_max < 1 or B c_max < T is MANNER_HIP_E_INVALID; a single impression
 * with more than c_max candidates is seen on the device only and raises MANNER_HIP_STATUS_LENGTHS in `status` (may be NULL).
 * workspace: 8-byte aligned.  _backward: grad_scores [T] from the DEVICE scalar grad_loss [1]: (g / (B c_max)) u_b s_t where the
 * product is > 0, exactly 0 where it is <= 0 (a neutral news with s = 0 included).  Every reduction has a fixed order (no
 * floating-point atomics) and every grid depends on the shape alone. */
size_t manner_hip_head_workspace_bytes(int64_t N);
size_t manner_hip_head_backward_workspace_bytes(int64_t N, int32_t D, int32_t O);
int manner_hip_head_ce(const float* x, const float* w, const float* b, const int64_t* target, int64_t N, int32_t D, int32_t O, float* loss,
                       float* saved, float* logits, void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_head_ce_backward(const float* grad_loss, const float* x, const float* w, const float* saved, int64_t N, int32_t D, int32_t O,
                                float* grad_x, float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
int manner_hip_head_l1(const float* x, const float* w, const float* b, const float* target, int64_t N, int32_t D, float* loss, float* saved,
                       void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
int manner_hip_head_l1_backward(const float* grad_loss, const float* x, const float* w, const float* saved, int64_t N, int32_t D, float* grad_x,
                                float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_senti_div_workspace_bytes(int64_t B);
int manner_hip_senti_div(const float* scores, const float* cand_score, const float* hist_score, const int64_t* hist_off, const int64_t* cand_off,
                         int64_t T, int64_t n_hist, int64_t B, int64_t c_max, float* loss, void* workspace, size_t workspace_bytes, int32_t* status,
                         manner_hip_stream_t stream);
int manner_hip_senti_div_backward(const float* grad_loss, const float* scores, const float* cand_score, const float* hist_score,
                                  const int64_t* hist_off, const int64_t* cand_off, int64_t T, int64_t n_hist, int64_t B, int64_t c_max,
                                  float* grad_scores, manner_hip_stream_t stream);

/* ---- SentiDebias-PLM's generator and discriminator lines (csrc/debias.hip; f32, forward and backward; additive exports) --------------
 * What baselines/senti_debias_plm_module.py:94-148,163-167,275-280 compute beside the leaf classes.  The sentiment encoder has only
 * C = num_sent_classes distinct outputs, the class table `table` [C, D] = tanh(linear(embedding.weight)) that the caller forms with
 * manner_hip_linear_tanh on C rows; `cls` int64 holds a row's class and the [N, D] sentiment rows are never written.  A class outside
 * [0, C) is never used as an index: it raises MANNER_HIP_STATUS_INDEX in `status` (may be NULL) and its row counts as 0, gradient 0.
 * Every reduction has a fixed order (no floating-point atomics), every grid depends on the shape alone; NULL gradient pointers skip
 * their kernels.  N < 2^31, C <= 64.
 * manner_hip_orth_loss: rows [N, D] (the first n_hist are the history's), user_free / user_aware [B, D] -> loss [1] =
 * |mean_{i < n_hist} cos(rows_i, table[cls_i])| + |mean_{i >= n_hist} cos(...)| + mean_b |cos(user_free_b, user_aware_b)| with
 * cos(a, b) = a . b / (1e-8 + |a| |b|); `means` [2] receives the two signed means (the backward's signs).  An empty segment is NaN.
 * D <= 1024 (a row in registers).  _backward: from the DEVICE scalar grad_loss [1], grad_rows [N, D], grad_user_free / _aware [B, D] and
 * grad_table [C, D], per-class sums over chunks of ascending rows added in ascending chunk order; a zero vector receives torch's zero
 * gradient through its norm.
 * manner_hip_class_dense: off int64 [B + 1] -> out [B, width, D] = to_dense_batch of table[cls], zero padding; B width >= N
 * (MANNER_HIP_E_INVALID otherwise; a single user with more than `width` rows raises MANNER_HIP_STATUS_LENGTHS).  _backward: grad_out
 * [B, width, D] -> grad_table by the same binned sums.
 * manner_hip_class_scores: user [B, D] -> out [N] = user_b . table[cls_t] for the ragged candidates t of user b (off [B + 1]), read
 * from the [B, C] products.  _backward: grad_user [B, D], grad_table [C, D] from the per-(user, class) sums of grad_out.
 * manner_hip_adv_loss: Discriminator.forward and adversarial_loss on both row sets: loss [1] = mean_{i < n_hist} CE_i +
 * mean_{i >= n_hist} CE_i, CE_i = -log softmax(w2 tanh(w1 rows_i + b1) + b2)[(cls_i - 1) mod O] (the module writes
 * y_true[i, t - 1] = 1: class 0 lands on the last column); cls is validated against [0, O).  w1 [H, D], w2 [O, H].  Layer 1 runs on
 * the f32 matrix cores, layer 2 with the softmax as a row walk under w2 staged in LDS (up to 128 KB, read through L2 past it).
 * `hidden` [N, H] receives the activation; `saved` [N, O] (may be NULL when no backward follows) (p - y) / rows of the segment.
 * O <= 64, H <= 1024 (a hidden row in registers), D <= 1024 (the rows are orth_loss's).  _backward: grad_rows through the matrix cores,
 * grad_w1 through manner_hip_wgrad_rows_f32, grad_b1 / grad_w2 / grad_b2 as chunked fixed-order sums; any subset may be NULL and the
 * others keep their bits. */
size_t manner_hip_orth_loss_workspace_bytes(int64_t N, int64_t B);
size_t manner_hip_orth_loss_backward_workspace_bytes(int64_t N, int32_t D, int32_t C);
int manner_hip_orth_loss(const float* rows, int64_t N, int64_t n_hist, const float* table, const int64_t* cls, const float* user_free,
                         const float* user_aware, int64_t B, int32_t D, int32_t C, float* loss, float* means, void* workspace, size_t workspace_bytes,
                         int32_t* status, manner_hip_stream_t stream);
int manner_hip_orth_loss_backward(const float* grad_loss, const float* means, const float* rows, int64_t N, int64_t n_hist, const float* table,
                                  const int64_t* cls, const float* user_free, const float* user_aware, int64_t B, int32_t D, int32_t C,
                                  float* grad_rows, float* grad_table, float* grad_user_free, float* grad_user_aware, void* workspace,
                                  size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_class_dense_backward_workspace_bytes(int64_t B, int64_t width, int32_t D, int32_t C);
int manner_hip_class_dense(const float* table, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int64_t width, int32_t D, int32_t C,
                           float* out, int32_t* status, manner_hip_stream_t stream);
int manner_hip_class_dense_backward(const float* grad_out, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int64_t width, int32_t D,
                                    int32_t C, float* grad_table, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_class_scores_workspace_bytes(int64_t B, int32_t C);
int manner_hip_class_scores(const float* user, const float* table, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int32_t D, int32_t C,
                            float* out, void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_class_scores_backward(const float* grad_out, const float* user, const float* table, const int64_t* cls, const int64_t* off, int64_t N,
                                     int64_t B, int32_t D, int32_t C, float* grad_user, float* grad_table, void* workspace, size_t workspace_bytes,
                                     manner_hip_stream_t stream);
size_t manner_hip_adv_loss_workspace_bytes(int64_t N);
size_t manner_hip_adv_loss_backward_workspace_bytes(int64_t N, int32_t D, int32_t H, int32_t O);
int manner_hip_adv_loss(const float* rows, int64_t N, int64_t n_hist, const float* w1, const float* b1, const float* w2, const float* b2,
                        const int64_t* cls, int32_t D, int32_t H, int32_t O, float* loss, float* hidden, float* saved, void* workspace,
                        size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream);
int manner_hip_adv_loss_backward(const float* grad_loss, const float* rows, int64_t N, const float* w1, const float* w2, const float* hidden,
                                 const float* saved, int32_t D, int32_t H, int32_t O, float* grad_rows, float* grad_w1, float* grad_b1, float* grad_w2,
                                 float* grad_b2, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);

/* ---- the CAUM baseline's operators (csrc/caum.hip; f32, forward and backward; additive exports) -------------------------------------
 * manner_hip_axis0_attention_any is manner_hip_axis0_attention at ANY head dim 1 <= E / heads <= 64 (CAUM ships 25 and 5): qkv
 * [L0, B1, 3E] -> out [L0, B1, E], attention along axis 0.  stats [L0 * B1 * heads * 3] (may be NULL in the forward) receives the
 * softmax {max, sum} of every (row, slot, head); _backward_q reads them with the forward's `out`, writes the q third of grad_qkv and
 * the third statistic (d out . out); _backward_kv, called after it, writes the k and v thirds.
 * manner_hip_caum_user_forward is CAUMUserEncoder.forward (manner/models/components/user_encoder.py:121-178) for one candidate per
 * user: x [B, S, D], c [B, D] with rows c_stride floats apart (the cand[:, i, :] view), out [B].  params: the 16 tensors linear1.weight
 * [F, 4D], .bias, linear2.weight [U, 2D], .bias, multihead_attention.in_proj_weight [3U, U], in_proj_bias, out_proj.weight [U, U],
 * .bias, linear3.weight [U, F + U], .bias, dense_att.linear.weight [H1, 2U], .bias, dense_att.linear2.weight [H2, H1], .bias,
 * dense_att.linear3.weight [1, H2], .bias, in that order.  p > 0: the three dropouts on the generator of manner_hip_dropout_mask at
 * the sites site0 (candidate, element b * D + d), site0 + 1 (clicked news, flat index) and site0 + 2 (cat[cnn, self], flat index over
 * [B S, F + U]).  The attention runs across the B users at each history slot and the softmax over all S slots, unmasked, as in the
 * reference.  S <= 256; D, F, U, H1, H2 <= 1024; U / heads <= 64; D == U (MANNER_HIP_E_INVALID otherwise).  `saved`
 * (manner_hip_caum_user_saved_bytes) keeps the activations for _backward, which fills grad_x [B, S, D], grad_c [B, D] (contiguous) and
 * the 16 parameter gradients; the K third of d in_proj_bias and d dense_att.linear3.bias, zero in exact arithmetic, are written as zeros.
 * manner_hip_relu / _backward: out = max(x, 0); grad_x = grad_out where x > 0.
 * Every reduction across rows has a fixed order (no floating-point atomics). */
int manner_hip_axis0_attention_any(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, float* stats,
                                   manner_hip_stream_t stream);
int manner_hip_axis0_attention_any_backward_q(const float* qkv, const float* out, const float* grad_out, int64_t L0, int64_t B1, int32_t E,
                                              int32_t heads, float* grad_qkv, float* stats, manner_hip_stream_t stream);
int manner_hip_axis0_attention_any_backward_kv(const float* qkv, const float* grad_out, const float* stats, int64_t L0, int64_t B1, int32_t E,
                                               int32_t heads, float* grad_qkv, manner_hip_stream_t stream);
size_t manner_hip_caum_user_saved_bytes(int64_t B, int64_t S, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads);
int manner_hip_caum_user_forward(const float* x, const float* c, int64_t c_stride, const float* const* params, int64_t B, int64_t S, int32_t D,
                                 int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, uint64_t seed, uint32_t site0, float* out,
                                 void* saved, size_t saved_bytes, manner_hip_stream_t stream);
size_t manner_hip_caum_user_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads);
int manner_hip_caum_user_backward(const float* const* params, const float* grad_out, int64_t B, int64_t S, int32_t D, int32_t F, int32_t U,
                                  int32_t H1, int32_t H2, int32_t heads, float p, uint64_t seed, uint32_t site0, void* saved, size_t saved_bytes,
                                  float* grad_x, float* grad_c, float* const* grads, void* workspace, size_t workspace_bytes,
                                  manner_hip_stream_t stream);
/* manner_hip_caum_scores_all is the candidate loop of CAUMPLMModule.forward (baselines/caum_plm_module.py:159-161) in one call, forward
 * only and without dropout (eval()): x [B, S, D], cand contiguous [B, C, D], the same 16 params -> out [B, C] with out[b, c] what
 * manner_hip_caum_user_forward returns for the column cand[:, c, :].  Every product whose operand depends on (b, s) alone or on (b, c)
 * alone is taken once; only attention -> linear3 -> the two tanh layers run over the B C S rows.  Those rows live in `workspace`, and the
 * entry walks the columns in passes of as many as `workspace_bytes` holds (_workspace_bytes(..., cols_per_pass) gives the bytes for a
 * pass width; the least workspace holds one column).  A column's bits do not depend on the pass width.  Limits and messages as
 * manner_hip_caum_user_forward; C == 0 or B == 0 writes nothing; C < 0 is MANNER_HIP_E_INVALID. */
size_t manner_hip_caum_scores_all_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads,
                                                  int64_t cols_per_pass);
int manner_hip_caum_scores_all(const float* x, const float* cand, const float* const* params, int64_t B, int64_t S, int64_t C, int32_t D, int32_t F,
                               int32_t U, int32_t H1, int32_t H2, int32_t heads, float* out, void* workspace, size_t workspace_bytes,
                               manner_hip_stream_t stream);
/* manner_hip_caum_train_all_forward / _backward are the candidate loop in one call WITH dropout and gradients (train()): x [B, S, D],
 * cand contiguous [B, C, D], the same 16 params, seeds a device array of C uint64 (may be NULL when p == 0) -> scores [B, C], column c
 * what manner_hip_caum_user_forward(x, cand[:, c, :], ..., p, seeds[c], site0) computes: the same three sites and element indices
 * (dropout1 b D + d, dropout2 (b S + s) D + d, dropout3 (b S + s)(F + U) + j), so the masks of column c are those of the per-column
 * call with that seed.  The reference draws a fresh mask of the clicked news per column, so nothing is shared between the columns:
 * the B C S rows run in (b, c, s) order through one launch per product — the f32 matrix-core linear forward and for the data
 * gradients, manner_hip_wgrad_rows_f32's kernel for the weight gradients (from 64 rows on; the per-column entry's below).  `saved` (_saved_bytes) keeps the activations for _backward,
 * which fills grad_x [B, S, D] (the columns' contributions added in ascending c, each through its own dropout2 mask),
 * grad_cand [B, C, D] and the 16 parameter gradients (the same two written as exact zeros); `workspace` as
 * _backward_workspace_bytes says.  Limits and messages as manner_hip_caum_user_forward under the prefixes caum_train_all /
 * caum_train_all_backward, and B C S < 2^31.  Forward: C == 0 or B == 0 writes nothing.  Backward: C == 0 or B == 0 zero-fills the
 * parameter gradients, and grad_x as well when C == 0.  C < 0 is MANNER_HIP_E_INVALID.
 * manner_hip_wgrad_rows_f32: dW[o, k] = sum_r dy[r, o] x[r, k] in true f32 on the matrix cores (dy rows ldy, x rows ldx, dW rows ldo
 * floats apart).  The rows are split into groups whose count depends on (R, K, O) alone; the partial sums live in `workspace`
 * (_workspace_bytes; 0 when one group takes all rows) and are added in ascending group order: no atomics, the same bits every run.
 * R == 0 writes zeros. */
size_t manner_hip_caum_train_all_saved_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads);
int manner_hip_caum_train_all_forward(const float* x, const float* cand, const float* const* params, int64_t B, int64_t S, int64_t C, int32_t D,
                                      int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, const uint64_t* seeds, uint32_t site0,
                                      float* scores, void* saved, size_t saved_bytes, manner_hip_stream_t stream);
size_t manner_hip_caum_train_all_backward_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2,
                                                          int32_t heads);
int manner_hip_caum_train_all_backward(const float* const* params, const float* grad_scores, int64_t B, int64_t S, int64_t C, int32_t D, int32_t F,
                                       int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, const uint64_t* seeds, uint32_t site0, void* saved,
                                       size_t saved_bytes, float* grad_x, float* grad_cand, float* const* grads, void* workspace,
                                       size_t workspace_bytes, manner_hip_stream_t stream);
size_t manner_hip_wgrad_rows_f32_workspace_bytes(int64_t R, int32_t K, int32_t O);
int manner_hip_wgrad_rows_f32(const float* dy, int32_t ldy, const float* x, int32_t ldx, int64_t R, int32_t K, int32_t O, float* dW, int32_t ldo,
                              void* workspace, size_t workspace_bytes, manner_hip_stream_t stream);
/* DenseAttention alone (attention.py:134-141): y [R, O] = tanh(x W^T + b), and grad_pre = grad_out (1 - y^2) for its backward */
int manner_hip_linear_tanh(const float* x, const float* weight, const float* bias, int64_t R, int32_t K, int32_t O, float* y,
                           manner_hip_stream_t stream);
int manner_hip_tanh_backward(const float* y, const float* grad_out, float* grad_pre, int64_t n, manner_hip_stream_t stream);
int manner_hip_relu(const float* x, float* out, int64_t n, manner_hip_stream_t stream);
int manner_hip_relu_backward(const float* x, const float* grad_out, float* grad_x, int64_t n, manner_hip_stream_t stream);

/* ---- the LSTUR baseline's operators (csrc/gru.hip; f32, forward and backward; additive exports) ------------------------------------
 * manner_hip_gru_forward is a one-layer nn.GRU over pack_padded_sequence(batch_first=True, enforce_sorted=False) returning
 * `last_hidden` (manner/models/components/user_encoder.py:78-88): out[b] = the hidden state of row b after its own lengths[b] steps.
 * x [B, S, I] is read in place at x + b x_stride_b + s x_stride_s (element strides, the features contiguous: a channel view of a wider
 * tensor needs no copy); slots s >= lengths[b] are never read and may hold anything.  lengths int64 [B] (device); w_ih [3H, I], w_hh
 * [3H, H], b_ih, b_hh [3H] in nn.GRU's gate order r | z | n, n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h; h0
 * [B, H] contiguous or NULL (zeros); out rows ldo floats apart (the first H columns of a wider buffer).  The input projection runs
 * once for all rows, then one plain launch per time step (no cooperative launch, no grid barrier); a row past its length keeps h by
 * selection.  1 <= S <= 256, 1 <= I, H <= 1024 (MANNER_HIP_E_INVALID otherwise, "gru: H=1028 unsupported (H <= 1024)").  A length
 * outside [1, S] raises MANNER_HIP_STATUS_LENGTHS in *status (device int32, nullable): such a row takes min(max(length, 0), S) steps
 * and nothing is read out of bounds.  workspace: manner_hip_gru_workspace_bytes (one size for forward and backward).  saved
 * (manner_hip_gru_saved_bytes; NULL = inference): the rows of x as read, h_{t-1}, and the gates r, z, n, W_hn h + b_hn of every (t, b).
 * manner_hip_gru_backward: from grad_out [B, H] (rows ldg apart) and `saved`, S plain launches in reverse, then grad_x [B, S, I]
 * (contiguous; exactly 0 at the slots s >= lengths[b]), grad_h0 [B, H] (nullable), grad_w_ih, grad_w_hh, grad_b_ih, grad_b_hh.
 * manner_hip_user_rows: out[b, :E] = m(b) src[row(b), :E] with row(b) = ids[b] (ids int64 [B] given: a gather from a table of n_rows
 * rows ld_src apart; an id outside it raises MANNER_HIP_STATUS_INDEX and writes zeros) or row(b) = b (ids NULL: the same mask on
 * gradient rows), m(b) = 0 or 1 / (1 - p) drawn per ROW b at (seed, site) of manner_hip_dropout_mask's generator — nn.Dropout2d on
 * [1, B, E] as LSTURUserEncoder applies it: a whole user is masked.  out rows ld_out apart.
 * Every reduction has a fixed order (no floating-point atomics). */
size_t manner_hip_gru_saved_bytes(int64_t B, int64_t S, int32_t I, int32_t H);
size_t manner_hip_gru_workspace_bytes(int64_t B, int64_t S, int32_t I, int32_t H);
int manner_hip_gru_forward(const float* x, int64_t x_stride_b, int64_t x_stride_s, const int64_t* lengths, const float* w_ih, const float* w_hh,
                           const float* b_ih, const float* b_hh, const float* h0, int64_t B, int64_t S, int32_t I, int32_t H, float* out,
                           int64_t ldo, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, int32_t* status,
                           manner_hip_stream_t stream);
int manner_hip_gru_backward(const float* w_ih, const float* w_hh, const int64_t* lengths, const float* grad_out, int64_t ldg, int64_t B, int64_t S,
                            int32_t I, int32_t H, void* saved, size_t saved_bytes, float* grad_x, float* grad_h0, float* grad_w_ih,
                            float* grad_w_hh, float* grad_b_ih, float* grad_b_hh, void* workspace, size_t workspace_bytes,
                            manner_hip_stream_t stream);
int manner_hip_user_rows(const int64_t* ids, const float* src, int64_t n_rows, int64_t ld_src, int64_t B, int32_t E, float p, uint64_t seed,
                         uint32_t site, float* out, int64_t ld_out, int32_t* status, manner_hip_stream_t stream);

/* ---- the MINS baseline's operators (csrc/mins.hip; f32, forward and backward; additive exports) -------------------------------------
 * manner_hip_channel_gru_forward is MINSUserEncoder's multi-channel GRU (manner/models/components/user_encoder.py:217-238): a one-layer
 * GRU over R = B C independent sequences that SHARE one w_ih [3H, I], w_hh [3H, H], b_ih, b_hh [3H] (gate order r | z | n, the formulas
 * of manner_hip_gru_forward, zero initial state).  Row r = b C + c reads x + b x_stride_b + t x_stride_s + c I (element strides: a
 * contiguous [B, S, C I] tensor is read in place, channel c = torch.chunk's c-th piece), takes lengths[b] steps (int64 [B], device) and
 * writes out[b, c H : (c + 1) H], rows ldo floats apart.  Slots t >= lengths[b] are never read and may hold anything; a row keeps h by
 * selection once its length is reached.  The input projection of all (b, t, c) rows is one launch and the WHOLE RECURRENCE IS ONE
 * LAUNCH: a workgroup of 3 x 128 threads holds W_hh in registers (thread = (gate, unit), one row of 128) and walks all S steps of its
 * tile of 8 rows with workgroup barriers only — no cooperative launch, no grid barrier, no inter-workgroup counter.
 * 1 <= S <= 256, 1 <= I <= 1024, 1 <= H <= 128, C >= 1, B C S within int32 (MANNER_HIP_E_INVALID otherwise, "channel_gru: H=129
 * unsupported (H <= 128)").  A length outside [1, S] raises MANNER_HIP_STATUS_LENGTHS in *status (device int32, nullable): such a row
 * takes min(max(length, 0), S) steps and nothing is read out of bounds.  workspace: manner_hip_channel_gru_workspace_bytes (one size
 * for forward and backward).  saved (manner_hip_channel_gru_saved_bytes; NULL = inference), all in (b, t, c) row order: the rows of x
 * as read, the state entering every step, and the gates r, z, n, W_hn h + b_hn of the steps taken.
 * manner_hip_channel_gru_backward: from grad_out [B, C H] (rows ldg apart) and `saved`, ONE launch walks t = S - 1 .. 0 (thread = (gate,
 * unit k) holds column k of W_g; the three partial products are added through LDS in the order r, z, n; dh_{t-1} = dh_t z + that sum),
 * then manner_hip_linear_backward over the B S C stacked rows gives grad_w_hh, grad_b_hh, grad_w_ih, grad_b_ih — one fixed-order row
 * sum over all channels — and grad_x [B, S, C I] (contiguous; exactly 0 at the slots t >= lengths[b]).
 * manner_hip_axis0_attention_wide / _wide_backward_q / _wide_backward_kv are the manner_hip_axis0_attention_any entries at head dims
 * 65 <= E / heads <= 128 (MINS ships 768 / 6 = 128): the same layouts, the same stats [L0 * B1 * heads * 3] protocol (_backward_q
 * before _backward_kv) and the same arithmetic, with the lanes of a wave along the head dim (a wave per query row; backward-kv: per key
 * row) and the other side's rows staged in LDS tiles.  Any other head dim: MANNER_HIP_E_INVALID, "axis0_attention_wide: head_dim 129
 * unsupported (65 <= head_dim <= 128)".
 * Every reduction has a fixed order (no floating-point atomics): the same inputs give the same bits. */
size_t manner_hip_channel_gru_saved_bytes(int64_t B, int64_t S, int32_t C, int32_t I, int32_t H);
size_t manner_hip_channel_gru_workspace_bytes(int64_t B, int64_t S, int32_t C, int32_t I, int32_t H);
int manner_hip_channel_gru_forward(const float* x, int64_t x_stride_b, int64_t x_stride_s, const int64_t* lengths, const float* w_ih,
                                   const float* w_hh, const float* b_ih, const float* b_hh, int64_t B, int64_t S, int32_t C, int32_t I, int32_t H,
                                   float* out, int64_t ldo, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                   int32_t* status, manner_hip_stream_t stream);
int manner_hip_channel_gru_backward(const float* w_ih, const float* w_hh, const int64_t* lengths, const float* grad_out, int64_t ldg, int64_t B,
                                    int64_t S, int32_t C, int32_t I, int32_t H, void* saved, size_t saved_bytes, float* grad_x, float* grad_w_ih,
                                    float* grad_w_hh, float* grad_b_ih, float* grad_b_hh, void* workspace, size_t workspace_bytes,
                                    manner_hip_stream_t stream);
int manner_hip_axis0_attention_wide(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, float* stats,
                                    manner_hip_stream_t stream);
int manner_hip_axis0_attention_wide_backward_q(const float* qkv, const float* out, const float* grad_out, int64_t L0, int64_t B1, int32_t E,
                                               int32_t heads, float* grad_qkv, float* stats, manner_hip_stream_t stream);
int manner_hip_axis0_attention_wide_backward_kv(const float* qkv, const float* grad_out, const float* stats, int64_t L0, int64_t B1, int32_t E,
                                                int32_t heads, float* grad_qkv, manner_hip_stream_t stream);

/* ---- content-addressed news-embedding cache (ABI v6, round 4; csrc/cache.hip) ----------------------------------------------
 * SURVEY.md §8(d) mode T ("each unique news encoded once per module") behind the unchanged drop-in call pattern: the reference
 * re-encodes every occurrence — manner/models/cr_module.py:107,113 call manner/models/components/news_encoder.py:29-37 per batch —
 * while in eval() the text encoder is a pure function of a row's real tokens and the weights.  The caller (MannerTextEncoder.forward,
 * opt-in) keys every row, looks the keys up and encodes only the rows whose state is not 0.
 * manner_hip_news_key128: keys uint64 [n_news, 2] of the tokens at mask != 0 (independent of padded_len; keys[n][0] != 0).
 * manner_hip_news_cache_lookup: open-addressing table in CALLER-OWNED device memory — slot_keys uint64 [2, n_slots] (zero-filled =
 *   empty; n_slots a power of two), slot_rows int32 [n_slots], row_count int32 [1] (rows handed out so far; may run past
 *   capacity_rows once the table is full), scratch int32 [2 n_news].  Per input row: rows_out int32 (row of the embedding table, -1 if
 *   none) and state_out int32: 0 = cached (or a duplicate of a key that is new in this call — its row is valid once the state-1
 *   occurrence has been encoded and stored), 1 = new: encode and store at rows_out, 2 = encode without storing (table full).
 *   Exactly one occurrence of a new key gets state 1.  One stream at a time per table. */
int manner_hip_news_key128(const int64_t* ids, const int64_t* mask, int64_t n_news, int64_t padded_len, uint64_t* keys,
                           manner_hip_stream_t stream);
int manner_hip_news_cache_lookup(const uint64_t* keys, int64_t n_news, uint64_t* slot_keys, int32_t* slot_rows, int64_t n_slots,
                                 int32_t* row_count, int32_t capacity_rows, int32_t* rows_out, int32_t* state_out, int32_t* scratch,
                                 manner_hip_stream_t stream);

/* ---- token-packed payload of the frozen-prefix cache (csrc/cache.hip) --------------------------------------------------------
 * The hidden states of a news after the frozen layers, kept by REAL tokens: a table row (the index manner_hip_news_cache_lookup hands
 * out) owns row_len tokens of `pool` f32 [pool_tokens, hidden] starting at token row_off, so a news costs len x hidden x 4 bytes at
 * any padded width up to MANNER_HIP_MAX_LEN_INFER.  Caller-owned device state beside the lookup's: pool, row_off int64 [capacity_rows],
 * row_len int32 [capacity_rows] (filled with -1 = empty; -2 = key known, the pool had no room: no payload, ever; >= 1 = tokens),
 * row_src int32 [capacity_rows] (scratch), tok_count uint64 [1] (zeroed; tokens handed out — it may come to rest past pool_tokens when
 * the pool fills, nothing is ever written or read past the pool).  pool, fresh and out are 16-byte aligned, hidden % 4 == 0.  One
 * stream at a time per table; no call reads anything back to the host.
 * manner_hip_prefix_resolve: after the lookup — a state-0 row whose key has no payload becomes state 2, row -1 (encode, do not store).
 * manner_hip_prefix_store: fresh [n_new, padded_len, hidden] = encode_hidden of the rows with state != 0; fresh row j is row index[j]
 *   of the call (index NULL: j; n_new <= n_news), whose rows / state / lens (real tokens) are [n_news].  Every state-1 row reserves
 *   its tokens with one device-scope atomic add (correct for any order of the workgroups) and its real tokens are copied; a row that
 *   does not fit gets row_len -2.  src_of int32 [n_news] receives j at index[j] (for the gather of the same call).
 * manner_hip_prefix_gather: out [n_news, padded_len, hidden] — a row with a payload: its tokens, zeros at every padded position
 *   (whatever width it was stored at); a row without one: copied from `fresh` (its own row for state != 0, the row of the state-1
 *   occurrence of its key for state 0) when `fresh` is given, left untouched for the caller when fresh is NULL. */
int manner_hip_prefix_resolve(int32_t* rows, int32_t* state, int64_t n_news, const int32_t* row_len, int32_t capacity_rows,
                              manner_hip_stream_t stream);
int manner_hip_prefix_store(const float* fresh, int64_t n_new, const int64_t* index, int64_t n_news, const int32_t* rows,
                            const int32_t* state, const int32_t* lens, int64_t padded_len, int32_t hidden, float* pool,
                            int64_t pool_tokens, int32_t capacity_rows, int64_t* row_off, int32_t* row_len, int32_t* row_src,
                            uint64_t* tok_count, int32_t* src_of, manner_hip_stream_t stream);
int manner_hip_prefix_gather(const int32_t* rows, const int32_t* state, int64_t n_news, int64_t padded_len, int32_t hidden,
                             const float* pool, int64_t pool_tokens, int32_t capacity_rows, const int64_t* row_off,
                             const int32_t* row_len, const int32_t* row_src, const float* fresh, int64_t n_fresh,
                             const int32_t* src_of, float* out, manner_hip_stream_t stream);

/* ---- the sentiment annotator's classifier (csrc/seqcls.hip; f32, inference only; an additive export) --------------------------------
 * manner_hip_seqcls_head is the head of a *ForSequenceClassification checkpoint and the labelling rule of the reference's
 * SentimentAnnotator.forward (manner/data/components/sentiment_annotator.py:25-38) over the [CLS] rows x [N, H] (rows ldx floats apart)
 * that manner_hip_encode_cls returns.  dense_w [H, H], dense_b [H]; out_w [L, H], out_b [L].  Per row, in f32:
 *   h = tanh(dense_w x + dense_b),  z = out_w h + out_b,  p = softmax(z) with the row maximum subtracted,
 *   a = argmax p, the lowest index at a tie (numpy.argmax),
 *   score = p[a] if a == pos_idx, -p[a] if a == neg_idx, else (1 - p[a]) (p[L-1] - p[0])
 * pos_idx / neg_idx: the ids the checkpoint's id2label names 'positive' / 'negative', -1 for none.  The last branch reads positions
 * L - 1 and 0 whatever those labels are named, as the reference does.  A row with a non-finite logit gets label -1, score NaN and NaN
 * probabilities.  probs [N, L] (may be NULL: not written), label int32 [N], score [N].
 * One launch: a workgroup owns a panel of rows (32 below 8192 rows, else 128) and walks all column tiles of the dense layer for it on
 * the f32 matrix cores; tanh and the out-projection are each tile's epilogue, and softmax, argmax and the rule finish in the same
 * workgroup.  The [N, H] hidden activation is never written; there is no workspace and no atomic.  A hidden feature is one k-ascending
 * fmaf chain, a logit one fmaf chain over the hidden features in ascending order starting from out_b: the bits of a row do not depend
 * on N, on the panel or on the row's place in the call.
 * 1 <= L <= 64; H a multiple of 4, H <= 1024; 0 <= N < 2^31 (N == 0 launches nothing and returns OK); ldx >= H; pos_idx, neg_idx in
 * [-1, L).  Anything else, or a null pointer other than probs (x, label and score may be NULL at N == 0), is MANNER_HIP_E_INVALID with a message that names the entry, before any
 * launch. */
int manner_hip_seqcls_head(const float* x, int64_t ldx, const float* dense_w, const float* dense_b, const float* out_w, const float* out_b,
                           int64_t N, int32_t H, int32_t L, int32_t pos_idx, int32_t neg_idx, float* probs, int32_t* label, float* score,
                           manner_hip_stream_t stream);

/* ---- t-SNE of the A-Module's embedding plots (csrc/tsne.hip; f32, f64 only in final fixed-order sums; additive exports) ---------------
 * The reference's AModule.on_validation_epoch_end / on_test_epoch_end (manner/models/a_module.py:150-173, 191-212) call
 * MulticoreTSNE(n_jobs=8).fit_transform on the CPU.  These five entries are the arithmetic of manner_amd.manifold.TSNE, the published
 * method (kNN affinities at 3 x perplexity neighbours, gains, momentum, early exaggeration) with EXACT repulsive forces: the Barnes-Hut
 * `angle` has no meaning here.  No floating-point atomic, no grid-wide barrier or counter; every grid comes from the shape alone: two
 * runs give the same bits.  Bounds of all five: 1 <= k <= 255, 0 <= N <= 2^20, N - 1 >= k (but for tsne_affinities, whose rows are searched
 * one by one, and tsne_repulsion, which has no k); N == 0 launches nothing and returns OK.  A bad
 * shape or a null pointer is MANNER_HIP_E_INVALID with a message that names the entry, before any launch.
 *
 * manner_hip_knn_rows_f32: x [N, D] (1 <= D <= 1024) -> idx int32 [N, k], d2 [N, k]: the k nearest OTHER rows of every row by squared
 *   Euclidean distance, ascending by (d2, idx) — equal distances resolve to the lower row index.  The search is exact; a distance is one
 *   fmaf chain of squared differences over the features in ascending order (not the Gram form).  A row whose distances are NaN leaves
 *   idx -1 in the places it could not fill.
 * manner_hip_tsne_affinities: d2 [N, k] -> p [N, k], beta [N].  Per row the binary search for the beta at which p_j ~ exp(-beta d2_j) has
 *   entropy log(perplexity) within 1e-5: from beta = 1, doubled or halved while the far bound is open, bisected afterwards, at most 200
 *   trips.  Distances are taken relative to the row's smallest (p and the entropy do not change; nothing underflows to an empty sum), so
 *   a row of equal or of zero distances is uniform; beta saturates at FLT_MAX.
 * manner_hip_tsne_repulsion: y [N, 2] -> part [split, N, 4] = per row and j slice (sum q^2 dx, sum q^2 dy, sum q, 0) over ALL j of the
 *   slice, q = 1 / (1 + |y_i - y_j|^2) by the hardware reciprocal; zpart f64 [split * ceil(N / 512)] = per workgroup the sum of its rows'
 *   sum q.  The self pair is not branched on: its q is exactly 1 and its force exactly 0, so Z = (sum of zpart) - N.  `split` must be the
 *   launcher's own function of N (manner_amd.hip.tsne_j_split); a row's partials are added in ascending slice order by the consumer.
 * manner_hip_tsne_step: one iteration.  dY_i = exaggeration sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_j q_ij^2 (y_i - y_j), P gathered
 *   from the directed edge list out_idx / out_p [N, k] (edge (i -> j, p) adds p / (2 N) to P_ij and to P_ji) and its transpose: the incoming
 *   edges of row i are in_src / in_p [in_off[i], in_off[i + 1]) (in_off int64 [N + 1], n_in edges in all), any number per row.  Then
 *   gains = sign(dY) != sign(u) ? gains + 0.2 : gains * 0.8, floored at 0.01 (sign(0) = 0); u = momentum u - learning_rate gains dY;
 *   y_out = y + u, less its column means (a second launch; ypart f64 [2 ceil(N / 64)] is its scratch).  u, gains [N, 2] in place; y_out
 *   must not be y.  An edge whose index is outside [0, N) is skipped.
 * manner_hip_tsne_kl: kl f64 [1] = sum P log(P / Q) over the non-zero entries of the symmetrised P, Q = q / Z, from y, the zpart of a
 *   repulsion call on the same y, and the outgoing edges; klpart f64 [ceil(N / 64)] is scratch. */
int manner_hip_knn_rows_f32(const float* x, int64_t N, int32_t D, int32_t k, int32_t* idx, float* d2, manner_hip_stream_t stream);
int manner_hip_tsne_affinities(const float* d2, int64_t N, int32_t k, float perplexity, float* p, float* beta, manner_hip_stream_t stream);
int manner_hip_tsne_repulsion(const float* y, int64_t N, int32_t split, float* part, double* zpart, manner_hip_stream_t stream);
int manner_hip_tsne_step(const float* y, const float* part, const double* zpart, int32_t split, const int32_t* out_idx, const float* out_p,
                         int32_t k, const int64_t* in_off, const int32_t* in_src, const float* in_p, int64_t n_in, int64_t N,
                         float exaggeration, float momentum, float learning_rate, float* u, float* gains, float* y_out, double* ypart,
                         manner_hip_stream_t stream);
int manner_hip_tsne_kl(const float* y, const double* zpart, int32_t split, const int32_t* out_idx, const float* out_p, int32_t k, int64_t N,
                       double* klpart, double* kl, manner_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MANNER_HIP_H */
