/*
 * chimeralm_hip.h -- C ABI of the MI355X (gfx950) inference engine for ChimeraLM's `predict` hot path.
 *
 * The drop-in boundary of the reference is the `net` module of `ClassificationLit`
 *   /root/reference/chimeralm/models/basic_module.py:14-22,38,67-77   (ClassificationLit.forward -> self.net)
 *   /root/reference/chimeralm/models/components/hyena.py:218-256      (HyenaDna.__init__ / forward)
 * i.e. `forward(input_ids int64[B,L], input_quals=None) -> logits fp32[B,2]`.  The reference is pure Python
 * on torch and has no FFI of its own; these entry points are what a ctypes binding behind
 * `HyenaDna.forward` binds (INTEGRATION.md shows the stub).  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative CLM_E_* code; `clm_last_error` gives the text.
 *     No exception crosses this boundary.
 *   - one handle per GPU; a handle is not re-entrant; different handles are independent.
 *   - `clm_forward` is asynchronous on the caller's HIP stream and performs no host synchronisation,
 *     PROVIDED the workspace is already large enough (`clm_reserve`); growing it synchronises the stream first.
 *   - weight memory is copied at `clm_load_weight`; the caller keeps ownership of `data`.
 */
#ifndef CHIMERALM_HIP_H
#define CHIMERALM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLM_ABI_VERSION 6

/* error codes */
#define CLM_OK 0
#define CLM_E_INVALID (-1)     /* bad argument / shape / unknown key            */
#define CLM_E_HIP (-2)         /* a HIP runtime call failed                      */
#define CLM_E_MISSING (-3)     /* clm_finalize: a required weight was not loaded */
#define CLM_E_UNSUPPORTED (-4) /* shape or mode outside what the kernels cover   */
#define CLM_E_STATE (-5)       /* call order (e.g. forward before finalize)      */

/* element types for clm_load_weight / token ids */
#define CLM_DT_F32 0
#define CLM_DT_F64 1
#define CLM_DT_BF16 2
#define CLM_DT_F16 3
#define CLM_DT_U8 4
#define CLM_DT_I32 5
#define CLM_DT_I64 6

/* arithmetic type of the dense projections (in_proj / out_proj / fc1 / fc2 / pooling score GEMM).
 * Accumulation, LayerNorm statistics, the residual stream, the long convolution (FFT) and the softmax are
 * fp32 in every mode.  F32 uses v_mfma_f32_32x32x2_f32 (exact fp32); BF16/F16 use v_mfma_f32_32x32x16_*. */
#define CLM_PREC_F32 0
#define CLM_PREC_BF16 1
#define CLM_PREC_F16 2
/* F16C: fp16 activations; the weights of in_proj, out_proj and the score layer held as hi + lo, hi = fp16(w) and lo = e4m3((w - hi)
 * * 2^17): per 64-deep group four fp16 MFMAs with hi and one block-scaled fp8 MFMA with lo (activations truncated to e5m2 in
 * registers), one fp32 accumulator; the two MLP products on plain fp16 weights (their rounding does not show in the logits).  The mode
 * that runs at 16-bit MFMA rate AND stays within the reference's 1e-3 logit tolerance (weight rounding is the error
 * that attention pooling cannot average out, tests/error_model.py); z / y are stored as fp16 like CLM_PREC_F16. */
#define CLM_PREC_F16C 3
/* F16X3 (ABI 4): near-exact at fp16 MFMA rate / 3.  Every operand of a dense projection is split into two halfs, x = hi + lo with
 * hi = fp16(x) and lo = fp16(x - hi) (~21 bits; weights pre-scaled by 2^10 so that their lo halfs stay normal), and a product is
 * three fp16 MFMAs into the fp32 accumulator: w_hi a_hi + w_lo a_hi + w_hi a_lo.  Everything else is the exact-fp32 engine (fp32
 * z / y / residual stream in HBM, fp32 convolution, score layer on the fp32 MFMA).  Logits within ~1e-5 of exact fp32 -- three
 * orders of magnitude inside the reference's 1e-3 -- at 2x its rate; unguarded by default (csrc/tail32.hip, AR_X3).  ABI 5: also
 * the arithmetic every 16-bit handle runs its short reads (clm_set_short_read_len) and its first fall-back level in. */
#define CLM_PREC_F16X3 4

typedef struct clm_handle clm_handle;

/* Mirrors the hyper-parameters fixed by the reference at
 *   chimeralm/models/lm.py:19-31 (head: 256 -> 512, 2 layers, attention pooling, gelu, residual) and by the
 *   HyenaDNA-small-32k config.  Only these values are accepted (checked in clm_create). */
typedef struct clm_config {
    int32_t struct_size;   /* = sizeof(clm_config), ABI guard                               */
    int32_t d_model;       /* 256                                                           */
    int32_t n_layer;       /* 4                                                             */
    int32_t d_inner;       /* 1024                                                          */
    int32_t vocab_rows;    /* 16  (vocab 12 padded to a multiple of 8)                      */
    int32_t filter_order;  /* 64                                                            */
    int32_t emb_dim;       /* 5                                                             */
    int32_t max_seq_len;   /* 32770 rows of pos_emb.z / pos_emb.t                           */
    int32_t head_hidden;   /* 512                                                           */
    int32_t n_classes;     /* 2                                                             */
    float ln_eps;          /* 1e-5                                                          */
    int32_t precision;     /* CLM_PREC_*                                                    */
    int32_t chunk_reads;   /* reads pushed through all layers together (default 256; the engine lowers it for long reads so that a
                              chunk holds at most 256 x 8,256 tokens in the 16-bit modes, 64 x 8,256 in exact fp32: workspace ~ chunk) */
} clm_config;

int clm_abi_version(void);
int clm_default_config(clm_config* cfg);

/* Replaces HyenaDna.__init__ (hyena.py:218-242): allocate an engine on HIP device `device`. */
int clm_create(const clm_config* cfg, int device, clm_handle** out);

/* Replaces the state_dict load of PyTorchModelHubMixin.from_pretrained / Lightning ckpt_path
 * (lm.py:17, __main__.py:317).  `key` is the reference checkpoint key with or without the `net.` prefix, e.g.
 * `net.backbone.backbone.layers.0.mixer.in_proj.weight`, `net.head.attention.0.weight`.
 * `data` may be host or device memory (hipMemcpyDefault); `shape[ndim]` is checked against the model.
 * Unknown keys return CLM_E_INVALID; the aliases `implicit_filter.{3,5}.freq` of the shared sine module are
 * accepted and ignored in favour of `.1.freq`. */
int clm_load_weight(clm_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);

/* Packs weights for the kernels (MFMA fragment order, compute dtype) and checks completeness.
 * May be called again after further clm_load_weight calls; everything derived from the weights (packings, filter spectra, [PAD]
 * tables, the fp16x3 range verdict) is rebuilt.  The switches are handle state, not weight state: the clm_set_fallback level,
 * clm_set_mlp_compensation and clm_set_short_read_len stay as they were set (chimeralm_amd/hyena.py resets them itself). */
int clm_finalize(clm_handle* h);

/* Grow the workspace for batches up to B reads of L tokens (optional; clm_forward does it on demand). */
int clm_reserve(clm_handle* h, int B, int L);

/* Replaces HyenaDna.forward(input_ids, input_quals=None) (hyena.py:244-256).
 *   ids        device pointer, [B, L] row-major with `ids_row_stride` elements between rows,
 *              dtype CLM_DT_I64 (what the reference's collator produces), CLM_DT_I32 or CLM_DT_U8.
 *   logits_out device pointer, fp32 [B, n_classes].
 *   stream     hipStream_t (NULL = default stream). */
int clm_forward(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L,
                float* logits_out, void* stream);

/* ---- batches that arrive in host memory ------------------------------------------------------------
 * Replaces the `batch["input_ids"].to(device)` Lightning performs before predict_step (basic_module.py:177-187 receives a
 * device batch).  Two device staging buffers per handle: clm_stage_ids enqueues the H2D copy of a batch on the HANDLE'S OWN
 * copy stream (so it overlaps the forward pass running on the compute stream) and returns which buffer it used;
 * clm_forward_staged makes the compute stream wait for exactly that copy and runs the forward on it; clm_stage_wait blocks
 * the host until the copy has left the host buffer (a pinned slot of the BAM feeder, chimeralm_feed.h, can then be
 * released).  A staging buffer is not overwritten before the forward that read it has finished (event-ordered).
 * `host_ids` should be page-locked for the copy to be asynchronous. */
int clm_stage_ids(clm_handle* h, const void* host_ids, int ids_dtype, int64_t ids_row_stride, int B, int L, int* staged);
int clm_forward_staged(clm_handle* h, int staged, float* logits_out, void* stream);
int clm_stage_wait(clm_handle* h, int staged);

/* ---- attention as an output -------------------------------------------------------------------------------------------
 * Replaces `save_attention` of the reference (chimeralm/models/lm.py:14,40; BinarySequenceClassifier keeps
 * `attention_weights = softmax(self.attention(x), dim=1)`, hyena.py:52,119,129-130) and what notebooks/attention.ipynb does with it
 * on the host (find_attention_peaks: np.argsort(weights)[-top_k:][::-1]; the mass of a window), for whole batches and without a
 * host synchronisation.  Per read b of L tokens with pooling scores s[b, t]:
 *   weights     w[b, t] = exp(s[b, t] - max_t s) / sum_t exp(s[b, t] - max_t s) over ALL L positions, [PAD] and [SEP] included (the
 *               reference's mask is always None, hyena.py:256): fp32, row b at weights + b * weights_row_stride.  The scores are
 *               those of the arithmetic the forward ran in (precision, fall-back level, short-read switch).
 *   summary     n_pad = length of the leading run of token id 4 ([PAD]); has_sep = the last token is id 1 ([SEP]); the BASES are the
 *               n_bases positions in between.  pad_weight / sep_weight / base_weight: the weight on each of the three.
 *   peaks       the n_peaks = min(top_k, n_bases) bases of largest weight, in descending weight, equal weights by lower position:
 *               peak_pos[b * top_k + k] is 0-based among the read's bases (token index = position + n_pad), peak_weight its
 *               weight; slots k >= n_peaks hold -1 / 0.  top_k is 1 ... 32.
 * A read whose scores hold a NaN or +-inf reports n_peaks = 0 and NaN masses (never a position outside the read).
 * `weights` may be NULL (summary and peaks only); `summary`, `peak_pos` and `peak_weight` may be NULL together (weights only); all
 * NULL is CLM_E_INVALID, as are a top_k outside 1 ... 32 with a summary and a weights_row_stride < L.  All are device pointers for
 * the B reads of the call: a batch larger than a chunk is written chunk by chunk at its rows.  One kernel per chunk behind the
 * head on `stream` (csrc/attn_weights.hip: one workgroup per read, the scores cross HBM once, no atomics -- bitwise the same from
 * run to run); L above 32,832 tokens is CLM_E_UNSUPPORTED.  Nothing else writes these buffers: not clm_selfcheck, not the
 * forwards the engine runs for itself.  With `attn` NULL the two calls ARE clm_forward / clm_forward_staged. */
typedef struct clm_attn_summary {
    int32_t n_pad, n_bases, has_sep, n_peaks;
    float pad_weight, sep_weight, base_weight;
    int32_t reserved;
} clm_attn_summary;
typedef struct clm_attn_out {
    int32_t struct_size;          /* = sizeof(clm_attn_out), ABI guard */
    int32_t top_k;
    float* weights;               /* fp32 [B][weights_row_stride] or NULL */
    int64_t weights_row_stride;   /* floats between rows, >= L */
    clm_attn_summary* summary;    /* [B] or NULL */
    int32_t* peak_pos;            /* [B][top_k] */
    float* peak_weight;           /* [B][top_k] */
} clm_attn_out;
int clm_forward_attn(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                     const clm_attn_out* attn, void* stream);
int clm_forward_staged_attn(clm_handle* h, int staged, float* logits_out, const clm_attn_out* attn, void* stream);

/* ---- the running verdict: prefix logits along a read from one forward ---------------------------------------------------
 * No counterpart in the reference.  The backbone is causal and the head (hyena.py:117-146) is a softmax-weighted sum over
 * positions followed by the classifier, so the logits the model would give if a row ENDED after its first n tokens follow from what
 * one forward of the whole row leaves behind: its per-tile pooling partials, merged prefix by prefix, then the classifier.
 *   points      a batch row of L tokens (its pads included) and a stride S (a multiple of 128 in 128 ... 4,096) have
 *               K = ceil(L / S) points; point k < K - 1 covers tokens [0, (k + 1) S), point K - 1 all L; n_k = tokens point k covers.
 *   trajectory  logits[b][k][:] = classifier(pool(ln_f(h[b, :n_k]))): the reference head applied to the first n_k rows of the
 *               final residual stream, the softmax normalised over those n_k positions only -- HyenaDna.forward(ids[b:b+1, :n_k]) up
 *               to the arithmetic's rounding.  fp32, row b at logits + b * point_stride * 2.  Point K - 1 is the call's own
 *               logits_out[b], copied bit for bit, not recomputed.
 *               A truncated row does not end in [SEP]: no point but the last shows the model a complete read.  Points inside the
 *               [PAD] prefix of a left-padded row describe pads only.  The values are those of the arithmetic the forward ran in
 *               (precision, fall-back level, short-read switch); a short prefix averages the roundings of fewer tokens than the
 *               read it comes from, so a 16-bit mode's interior points may be further from fp32 than its logits are.
 *   summary     per read, computed on the device, with gap_k = (double)logit1 - (double)logit0 of point k:
 *               n_pad, n_bases, has_sep as clm_attn_summary defines them; n_points = K;
 *               first_k   the first point with n_k > n_pad, min(n_pad / S, K - 1) (an all-[PAD] row: K - 1);
 *               label     gap_{K-1} > 0 (a tie is class 0); final_gap = gap_{K-1};
 *               onset_k   the smallest k >= first_k such that every point in [k, K - 1] has the final label;
 *               jump_k    the k in (first_k, K - 1] that maximises sgn * (gap_k - gap_{k-1}), sgn = +1 for label 1, -1 for label 0,
 *                         ties to the lowest k; jump_dgap is that value; first_k = K - 1: jump_k = -1, jump_dgap = 0;
 *               n_nonfinite   points >= first_k with a NaN or +-inf logit; if any, onset_k = jump_k = -1 and jump_dgap = 0.
 *               "Bases seen at point k" is clamp(n_k - n_pad, 0, n_bases).
 * `summary` may be NULL.  CLM_E_INVALID: a stride that is not such a multiple, point_stride < K, logits NULL, a struct_size
 * mismatch.  CLM_E_UNSUPPORTED: L above 32,832 tokens, a debug stop, the unfused exact path (CLM_DEBUG=unfused_fp32: its partials
 * have another form).  Device pointers for the B reads of the call, written chunk by chunk at their rows by three kernels behind
 * the head on `stream` (csrc/trajectory.hip: fixed order, no atomics -- bitwise the same from run to run); the workspace is the
 * handle's.  Nothing else writes these buffers: not clm_selfcheck, not the forwards the engine runs for itself.  `attn` and `traj`
 * may each be NULL; with both NULL the two calls ARE clm_forward / clm_forward_staged. */
typedef struct clm_traj_summary {
    int32_t n_pad, n_bases, has_sep, n_points;
    int32_t first_k, label, onset_k, jump_k;
    int32_t n_nonfinite, reserved;
    float jump_dgap, final_gap;
} clm_traj_summary;
typedef struct clm_traj_out {
    int32_t struct_size;          /* = sizeof(clm_traj_out), ABI guard */
    int32_t stride;               /* S: tokens between points */
    float* logits;                /* fp32 [B][point_stride][2] */
    int64_t point_stride;         /* points between rows, >= K */
    clm_traj_summary* summary;    /* [B] or NULL */
} clm_traj_out;
int clm_forward_traj(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                     const clm_attn_out* attn, const clm_traj_out* traj, void* stream);
int clm_forward_staged_traj(clm_handle* h, int staged, float* logits_out, const clm_attn_out* attn, const clm_traj_out* traj,
                            void* stream);

/* Errors a forward can only detect on the device after the call has returned: a token id outside [0, vocab_rows), for
 * which the reference's nn.Embedding raises IndexError inside HyenaDna.forward (hyena.py:249).  The id kernels clamp such an
 * id (no wild read) and flag the handle; the flag is reported ONCE, as CLM_E_INVALID with the message in clm_last_error,
 * by the next clm_forward / clm_forward_staged / clm_stage_wait, or by clm_check, which first waits for `stream`. */
int clm_check(clm_handle* h, void* stream);

/* ---- the 16-bit modes checked against, and replaced by, the reference's arithmetic -------------------------------------
 * The reference computes the whole forward in ONE precision, fp32 (hyena.py:244-256).  A 16-bit handle (CLM_PREC_F16C / F16 /
 * BF16) also holds the exact-fp32 packing of its weights and the exact-fp32 kernels, so the deviation of its mode from the
 * reference's arithmetic can be MEASURED on the weights that were loaded and on reads the caller chooses, instead of assumed
 * from other weights:
 *   clm_selfcheck   runs `ids` (device memory, as clm_forward) through the handle's mode AND through the exact-fp32 kernels
 *                   and returns the largest |logit difference| (`max_abs_diff`, host; +inf if anything is not finite) and the
 *                   number of reads whose argmax differs (`labels_differ`, may be NULL).  Synchronises `stream`.  Not affected
 *                   by clm_set_fallback; 0 for a CLM_PREC_F32 handle.  Lengths a CLM_PREC_F16C handle runs in its fp16x3 kernels
 *                   (clm_set_short_read_len) are measured like any other: fp16x3 against exact fp32.
 *   clm_set_fallback(h, level)   ABI 5: a LEVEL, not a switch -- the reference computes one precision always (hyena.py:244-256), so
 *                   the answer to "the fast mode is off" is the next-fastest arithmetic that is inside its tolerance, not the
 *                   slowest.  0 = the handle's own mode.  1 = every later clm_forward* runs in the next arithmetic inside the
 *                   gate: CLM_PREC_F16X3 on a 16-bit handle (fp32-class logits at about twice the exact-fp32 rate), exact fp32
 *                   on a CLM_PREC_F16X3 handle.  2 = exact fp32 on every handle.  (The caller's reaction to a self-check above its
 *                   threshold: chimeralm_amd/hyena.py uses level 1 at 5e-4, half the reference tolerance.)  No effect on a
 *                   CLM_PREC_F32 handle.  Other values: CLM_E_INVALID.
 *   clm_effective_precision  the CLM_PREC_* code reads of L tokens run in right now (CLM_PREC_F16X3 for the short reads of a
 *                   CLM_PREC_F16C handle and for a 16-bit handle at fall-back level 1).  fp16x3 packs weights x 2^10 as fp16 halfs,
 *                   which saturate at |w| >= 64: on a handle whose in_proj / out_proj / fc1 / fc2 / score weights reach that (or hold
 *                   a NaN; measured by clm_finalize) every read that would run fp16x3 runs exact fp32, and this says CLM_PREC_F32. */
int clm_selfcheck(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, void* stream,
                  float* max_abs_diff, int* labels_differ);
int clm_set_fallback(clm_handle* h, int level);
int clm_effective_precision(const clm_handle* h, int L);
/* The reduction both self-checks report (pure host arithmetic, no device needed): a, b = logits [B][n_classes] of the mode and of
 * the referee; *max_abs_diff = the largest |a - b|, +inf as soon as ANY difference is not finite (and it stays +inf: a NaN in read
 * 0 must not be overwritten by a finite difference of read 1); *labels_differ = reads whose argmax differs (may be NULL). */
int clm_logit_deviation(const float* a, const float* b, int B, int n_classes, float* max_abs_diff, int* labels_differ);
/* CLM_PREC_F16C only: reads shorter than `min_len` tokens run in the fp16x3 kernels inside the mode (ABI 5; exact fp32 before, and
 * still at fall-back level 2) -- default 2,048: the mode's error is a sum of per-token fp16 roundings that the attention pooling
 * averages like 1 / sqrt(L); below some length it no longer fits half the tolerance.  That length depends on the weights: the caller
 * may MEASURE it with clm_selfcheck(mode) on reads of decreasing length after clm_set_short_read_len(h, 1) (chimeralm_amd/hyena.py
 * does, at 1,024 / 512 / 256 tokens, and lowers the switch only with a margin of 2 under its threshold) and lower or raise it. */
int clm_set_short_read_len(clm_handle* h, int min_len);
/* CLM_PREC_F16C only (round 4): the two MLP products (fc1, fc2: two thirds of the dense FLOPs) run on plain fp16 weights by default
 * -- on most weights their rounding does not show in the logits -- and on hi + lo weights, like in_proj / out_proj / the score
 * layer, after clm_set_mlp_compensation(h, 1) (both packings are held; takes effect with the next forward; ~10 % slower).  The
 * caller decides with clm_selfcheck on the loaded weights: chimeralm_amd/hyena.py switches it on when the default form measures
 * above its threshold, and falls back to exact fp32 only if this form does too. */
int clm_set_mlp_compensation(clm_handle* h, int on);

/* ---- SequenceCNNTransformer -----------------------------------------------------------
 * Multi-head self-attention of nn.TransformerEncoderLayer as the reference builds it
 * (/root/reference/chimeralm/models/components/transformer.py:64-68,98: d_model 256, 8 heads of 32, no masks):
 *   qkv  device, [B, L, 768] 16-bit, the in_proj output q | k | v per token;  out  device, [B, L, 256] 16-bit, heads concatenated
 *   precision CLM_PREC_F16 or CLM_PREC_BF16 (element type of qkv / out; statistics and accumulation are fp32), or CLM_PREC_F16C:
 *   the attention of the transformer's fp16c mode -- qkv fp16, out 2 * B * L * 256 fp16 values, the plane hi = fp16(64 a) and then
 *   the plane lo = fp16(64 a - hi), so that a = (hi + lo) / 64 to ~2^-21.  CLM_PREC_F32 and CLM_PREC_F16X3 are CLM_E_INVALID here
 *   (clm_attention_exact_fwd).  qkv must be 16-byte aligned and out 8-byte aligned (the kernel's load and store widths), else
 *   CLM_E_INVALID and nothing is launched; likewise a shape whose ceil(L / 128) * 8 * B workgroups exceed 2^31 - 1, the most one
 *   launch takes.  Asynchronous on `stream`; writes nothing beyond out[B * L * 256] (F16C: twice that). */
int clm_attention_fwd(const void* qkv, void* out, int B, int L, int precision, void* stream);
/* The same attention in the arithmetic of the exact path (csrc/attention.hip; the kernels clm_tf_forward runs there): qkv device fp32
 * [B, L, 768], out device fp32 [B, L, 256]; precision CLM_PREC_F32 (fp32 products) or CLM_PREC_F16X3 (every operand as fp16 hi + lo,
 * three fp16 MFMAs per product).  qkv and out must be 16-byte aligned (the kernels read and write float4) and ceil(L / 128) * 8 * B
 * at most 2^31 - 1, else CLM_E_INVALID and nothing is launched.  Asynchronous on `stream`; writes nothing beyond out[B * L * 256]. */
int clm_attention_exact_fwd(const float* qkv, float* out, int B, int L, int precision, void* stream);

/* ---- the attention core for training (csrc/attention_train.hip; additive under ABI 6) ---------------
 * The same attention, exact fp32, forward with dropout on the probabilities and backward.  Stateless, no handle: the caller owns
 * every tensor.  Shape as above: qkv device fp32 [B, L, 768] (q | k | v), L positions, 8 heads of 32.
 *   forward    out [B, L, 256] = sum_j keep_ij p_ij v_j / (1 - dropout_p), p = softmax_j(q_i . k_j / sqrt(32)) (the row sum is taken
 *              over the undropped probabilities), and lse [B, 8, L] = log2 sum_j exp(q_i . k_j / sqrt(32)), in LOG2 units
 *              (torch.logsumexp of the scaled scores times log2 e: the exponent the kernels' exp2 takes).  With dropout_p == 0 out equals clm_attention_exact_fwd(CLM_PREC_F32)
 *              bit for bit.
 *   backward   dqkv [B, L, 768] (dq | dk | dv, every element written) of dout [B, L, 256], from qkv and the forward's out and lse,
 *              with the forward's dropout_p and seed.  P is recomputed as 2^(s log2 e - lse); delta_i = sum_d dout_id out_id goes to
 *              `workspace` (clm_attn_train_workspace_bytes(B, L) bytes: 4 * B * 8 * L rounded up to 16).  Two passes (dq per query
 *              tile over the keys, dk | dv per key tile over the queries); no floating-point atomics: two identical calls give
 *              identical bits, and a read's results do not depend on the other reads of the batch.
 *   keep mask  keep_ij = bits(seed, b * 8 + h, i, j) >= round(dropout_p * 2^32), with mix32 the xor-shift / multiply avalanche
 *              mixer  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  applied twice:
 *                  r    = mix32((uint32) seed ^ i * 0x9E3779B1)
 *                  bits = mix32((r ^ ((uint32)(seed >> 32) + (b * 8 + h) * 0x85EBCA77)) + j * 0xC2B2AE3D)      (mod 2^32)
 *              A pure function of those four values -- not of the tile shape, the launch geometry or B.  The backward
 *              regenerates it; clm_attn_train_mask writes it out as bytes keep [B, 8, L, L] (0 / 1) for the tests and is the only
 *              place a mask is ever stored.
 * CLM_E_INVALID, and nothing is launched: B < 1 or L < 1; dropout_p outside [0, 1) (NaN included); a pointer that is NULL or off 16
 * bytes; more than 2^31 - 1 workgroups in any launch (ceil(L / 128) * 8 * B for the passes, ceil(B * 8 * L * L / 256) for the mask).
 * clm_attn_train_workspace_bytes returns the (negative) code instead of a size.  Asynchronous on `stream`; nothing is written
 * beyond the stated extents. */
int64_t clm_attn_train_workspace_bytes(int B, int L);
int clm_attn_train_forward(const float* qkv, float* out, float* lse, int B, int L, float dropout_p, uint64_t seed, void* stream);
int clm_attn_train_backward(const float* qkv, const float* out, const float* lse, const float* dout, float* dqkv, void* workspace,
                            int B, int L, float dropout_p, uint64_t seed, void* stream);
int clm_attn_train_mask(uint8_t* keep, int B, int L, float dropout_p, uint64_t seed, void* stream);

/* ---- the Hyena operator's core for training (csrc/hyena_train.hip; additive under ABI 6) -------------
 * The causal 3-tap filter, the two gates and the long convolution with its skip term, forward and backward, exact fp32.
 * Stateless, no handle: the caller owns every tensor.  All tensors are device fp32, contiguous, channel-major, rows of exactly L
 * floats (no padded pitch; 4-byte alignment is all that is asked):
 *   zc [B, 768, L]   the raw in_proj output, rows x0 | x1 | v          sw [768, 3], sb [768]   short_filter weight and bias
 *   k  [256, L]      the modulated implicit filter                      D  [256]                filter_fn.bias
 *   c, y, dy [B, 256, L]
 *   forward    u_r[t] = sb[r] + sum_j sw[r, j] zc[r, t - 2 + j] (zc = 0 before t = 0; r = ch, 256 + ch, 512 + ch -> x0, x1, v),
 *              g = v x1,  c = causal_conv(g, k[ch]) + D[ch] g,  y = c x0.  Writes c_out and y_out.
 *   backward   from zc, the parameters, the forward's c and dy: dzc [B, 768, L], dsw [768, 3], dsb [768], dk [256, L], dD [256],
 *              every element written.  g, x0, x1, v are recomputed.
 * Covered: 1 <= L <= 8193 (one power-of-two transform of N = 2^logn >= 2 L - 2 points, logn 8 ... 14, held in LDS).  No
 * floating-point atomics: two identical calls give identical bits; dk, dsw, dsb and dD are added over the reads in read order;
 * c, y and dzc of a read do not depend on the other reads of the batch.
 * `workspace`: clm_hyena_train_workspace_bytes(B, L) bytes, with N as above,
 *       4 * (N + 512 * (N / 2 + 1) + B * 256 * L + B * 256 * 16)   rounded up to 16
 * (the twiddle table, the filter spectra -- computed once per call from k --, the per-read dk rows and the per-read parameter
 * partials; the forward uses the first two).  It holds nothing between calls.
 * CLM_E_INVALID, and nothing is launched: B < 1, L < 1 or B > 65535; a pointer that is NULL or off 4 bytes.  CLM_E_UNSUPPORTED:
 * L > 8193.  clm_hyena_train_workspace_bytes returns the (negative) code instead of a size.  Asynchronous on `stream`; nothing is
 * written beyond the stated extents. */
int64_t clm_hyena_train_workspace_bytes(int B, int L);
int clm_hyena_train_forward(const float* zc, const float* sw, const float* sb, const float* k, const float* D, int B, int L,
                            float* c_out, float* y_out, void* workspace, void* stream);
int clm_hyena_train_backward(const float* zc, const float* sw, const float* sb, const float* k, const float* D, const float* c,
                             const float* dy, int B, int L, float* dzc, float* dsw, float* dsb, float* dk, float* dD, void* workspace,
                             void* stream);

/* ---- the same core for reads of up to 32,769 tokens (csrc/hyena_longtrain.hip; additive under ABI 6) ----
 * The operator, the tensors, the outputs and the promises of clm_hyena_train_* above (no floating-point atomics, identical bits
 * from identical calls, sums over the reads in read order, c, y and dzc of a read independent of the other reads), computed as a
 * uniformly partitioned convolution: S = ceil(L / 8192) segments of P = 8192 tokens, overlap-save transforms of N = 16384 points
 * held in LDS, the spectra of the segments kept in the workspace and their products added per segment before one inverse.
 * Covered: every 1 <= L <= 32769 (S = 1 ... 5; a lone last token, L = 8192 n + 1, is a segment of its own).  The results agree
 * with clm_hyena_train_* to rounding where both cover L, not bit for bit.
 * `workspace`: clm_hyena_longtrain_workspace_bytes(B, L) bytes, with H = 8193 bins per spectrum,
 *       4 * (16384 + 512 * S * H + 1024 * B * S * H + B * 256 * L + B * 256 * 16)   rounded up to 16
 * (the twiddle table; the S filter spectra of the 256 channels, computed once per call from k; two spectra per (read, channel,
 * segment) -- the backward's FFT([dc_m ; dc_m+1]) and FFT([g_m ; 0]); the forward keeps one per channel there --; the per-read dk
 * rows; the per-read parameter partials).  It holds nothing between calls.
 * CLM_E_INVALID, and nothing is launched: B < 1, L < 1 or B > 65535; a pointer that is NULL or off 4 bytes.  CLM_E_UNSUPPORTED:
 * L > 32769.  clm_hyena_longtrain_workspace_bytes returns the (negative) code instead of a size.  Asynchronous on `stream`; nothing
 * is written beyond the stated extents. */
int64_t clm_hyena_longtrain_workspace_bytes(int B, int L);
int clm_hyena_longtrain_forward(const float* zc, const float* sw, const float* sb, const float* k, const float* D, int B, int L,
                                float* c_out, float* y_out, void* workspace, void* stream);
int clm_hyena_longtrain_backward(const float* zc, const float* sw, const float* sb, const float* k, const float* D, const float* c,
                                 const float* dy, int B, int L, float* dzc, float* dsw, float* dsb, float* dk, float* dD,
                                 void* workspace, void* stream);

/* The whole SequenceCNNTransformer forward (transformer.py:88-104; configuration of configs/model/transformer.yaml:3-12:
 * vocab 12, d_model 256, kernel 3, 8 heads, feed-forward 1024, `n_layers` encoder layers) behind the same `net` boundary as
 * HyenaDna: forward(input_ids[B, L], input_quals=None) -> logits fp32 [B, 2].  Same conventions as the clm_* calls above;
 * weights are loaded under the reference module's state_dict keys (with or without the `net.` prefix), the buffer
 * `pos_encoder.pe` [1, max_len, 256] included; fp32 tensors only.  L >= 8; L / 8 must not exceed max_len (the reference
 * asserts the same, transformer.py:21).  clm_tf_debug_fetch names: "hidden" fp32 [B, L/8, 256] (encoder output),
 * "scores" fp32 [B, L/8] (pooling scores before the softmax), "pooled" fp32 [B, 256]. */
typedef struct clm_tf_handle clm_tf_handle;
int clm_tf_create(int device, int precision /* CLM_PREC_F32 (exact, parity mode) | CLM_PREC_F16X3 (fp32-class, the module default) | CLM_PREC_F16C | CLM_PREC_F16 | CLM_PREC_BF16 */,
                  int n_layers, clm_tf_handle** out);
int clm_tf_load_weight(clm_tf_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
int clm_tf_finalize(clm_tf_handle* h);
int clm_tf_forward(clm_tf_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                   void* stream);
/* Round 3: the 16-bit mode on trial, as clm_selfcheck / clm_set_fallback for the Hyena engine.  A 16-bit handle keeps the raw fp32
 * tensors, so the exact-fp32 kernels (tf_fp32.hip) can run on the same handle: clm_tf_selfcheck runs `ids` through the handle's
 * mode and through them, synchronises `stream` and reports max |logit difference| and the number of reads whose label differs
 * (0 / 0 on an fp32 handle); clm_tf_set_fallback(h, level) has clm_set_fallback's levels: 1 = every later clm_tf_forward of a
 * 16-bit handle runs the fp32-path kernels on hi + lo halfs (fp16x3; exact fp32 on an fp16x3 handle), 2 = exact fp32. */
int clm_tf_selfcheck(clm_tf_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, void* stream,
                     float* max_abs_diff_out, int* labels_differ_out);
int clm_tf_set_fallback(clm_tf_handle* h, int level);
/* The CLM_PREC_* code clm_tf_forward runs in right now (after clm_tf_finalize; CLM_E_STATE before): the handle's 16-bit mode, or on
 * the fp32 path CLM_PREC_F16X3 / CLM_PREC_F32.  fp16x3 packs weights x 2^10 as fp16 halfs, which saturate at |w| >= 64: a handle
 * whose CNN-stem or encoder weights reach that (or hold a NaN) runs exact fp32 wherever it would run fp16x3 -- its own mode, fall-back
 * level 1 -- and says CLM_PREC_F32 here.  The Hyena engine does the same (clm_effective_precision). */
int clm_tf_effective_precision(const clm_tf_handle* h);
int clm_tf_debug_fetch(clm_tf_handle* h, const char* name, void* host_out, size_t bytes);
/* Test-only observability of the kernels between the ids and the logits (tests/test_gpu_tf_stages.py).  Off by default; with it off
 * a forward launches exactly what it launches without it (the cost is a host-side comparison per launch, no device code).
 * clm_tf_debug_stop_after(h, stage): every later clm_tf_forward of the handle returns right after the launch named `stage` and
 * launches nothing behind it, the pooling head included (logits_out is left untouched); stage < 0 ends that.  clm_tf_selfcheck always
 * runs whole forwards.  CLM_E_UNSUPPORTED on a handle created under CLM_DEBUG=unfused_fp32, CLM_E_INVALID for a stage the net
 * does not have.  The launches, in order:
 *   CLM_TF_STAGE_EMBED          exact path: the embedding rows (the 16-bit path has no such launch: it stops behind the ids conversion)
 *   CLM_TF_STAGE_CONV1 .. 3     a stem level: convolution + ReLU + max-pool
 *   CLM_TF_STAGE_PE_LN          + positional encoding, LayerNorm -> the residual stream
 *   CLM_TF_STAGE_IN_PROJ        layer 0's in_proj (the later layers' is the tail of the layer kernel before them)
 *   CLM_TF_STAGE_ATTENTION(i)   layer i's attention
 *   CLM_TF_STAGE_LAYER(i)       layer i's kernel: out_proj + LN1 + feed-forward + LN2 (+ layer i + 1's in_proj)
 * clm_tf_debug_fetch names beyond the three above, each in the type the kernels store it in (B, L of the last forward, M = B * (L/8)):
 *   exact path (fp32, fp16x3), fp32:   "x0" [B, L, 256] embedding rows, "x1" [B, L/2, 256], "x2" [B, L/4, 256], "x3" [M, 256] stem
 *                                      levels, "qkv" [M, 768], "att" [M, 256].  The stem ping-pongs between two buffers: "x0" lives
 *                                      until CONV2 has run, "x1" until CONV3 (fetch them from a forward stopped before that).
 *   16-bit path, raw fp16 / bf16 bits: "x1", "x2", "x3" as above, "hx" [M, 256] (the residual stream rounded once, the GEMM operand),
 *                                      "qkv" [M, 768], "att" [M, 256]; fp16c: "att" is [2][M, 256], the planes fp16(64 a), fp16(64 a - hi)
 *   both: "hidden" is the residual stream fp32 [M, 256] as the last launched stage left it (PE_LN: the encoder's input; LAYER(i): layer
 *   i's output; the layer kernel updates it in place), "qkv" / "att" those of the last in_proj / attention launched.
 * A name the last forward did not produce, or has overwritten since, is CLM_E_INVALID with a message ("scores" and "pooled" after a
 * stopped forward included; on a handle created under CLM_DEBUG=unfused_fp32, whose separate launches lay the workspace out
 * differently, every exact-path name but "hidden").  chimeralm_amd/transformer.py repeats the stage codes (TF_STOPS,
 * _STOP_ATTENTION0, _STOP_LAYER0); tests/test_tf_stage_host.py holds the two together. */
enum { CLM_TF_STAGE_EMBED = 0, CLM_TF_STAGE_CONV1 = 1, CLM_TF_STAGE_CONV2 = 2, CLM_TF_STAGE_CONV3 = 3, CLM_TF_STAGE_PE_LN = 4,
       CLM_TF_STAGE_IN_PROJ = 5 };
#define CLM_TF_STAGE_ATTENTION(i) (6 + 2 * (i))
#define CLM_TF_STAGE_LAYER(i) (7 + 2 * (i))
int clm_tf_debug_stop_after(clm_tf_handle* h, int stage);
/* Profiling taps of the 16-bit path (bench.py --net transformer): accumulated HIP-event time on the launch stream and number of
 * spans per stage -- 0 conv stack + positional encoding / LayerNorm, 1 attention, 2 encoder layer kernel (out_proj + LayerNorm-1
 * + feed-forward + LayerNorm-2 + next layer's QKV), 3 pooling head.  clm_tf_profile_read synchronises the device. */
int clm_tf_profile_enable(clm_tf_handle* h, int on);
int clm_tf_profile_read(clm_tf_handle* h, double* ms_out /*[4]*/, int64_t* spans_out /*[4]*/, int reset);
const char* clm_tf_last_error(const clm_tf_handle* h);
int clm_tf_destroy(clm_tf_handle* h);

/* ---- DNAConvNet (ABI 6) ----------------------------------------------------------------------------------------------
 * The reference's CNN classifier (/root/reference/chimeralm/models/components/cnn.py, configs/model/cnn.yaml: vocab 12, embedding 256,
 * three blocks of Conv1d(256, 256, 7, padding "same") + BatchNorm1d + GELU + MaxPool1d(4), mean over positions, Linear(256, 512) +
 * BatchNorm1d + GELU + Linear(512, 2)) in eval mode, behind the same `net` boundary: forward(input_ids[B, L]) -> logits fp32 [B, 2].
 * Same conventions as the clm_tf_* calls; weights under the reference module's state_dict keys (with or without `net.`), fp32
 * only; `*.num_batches_tracked` is accepted and ignored.
 *   precision   CLM_PREC_F32 (exact fp32 MFMA) or CLM_PREC_F16X3 (blocks 1 and 2 as three fp16 MFMAs on hi + lo halfs); anything
 *               else is CLM_E_INVALID.  The fp16x3 weight packing saturates for |w| >= 64: if a block-1 / block-2 weight is that
 *               large, clm_cnn_finalize packs that handle's weights for the exact-fp32 kernels instead.  Block 0 (an fp64 table of
 *               embedding x taps) and the head are fp32 in both modes.
 *   L >= 64     (three max-pools of 4; the reference raises for shorter reads), otherwise CLM_E_INVALID.
 *   ids         i64, i32 or u8; an id outside [0, 12) is clamped into it (no read outside the table; the reference's nn.Embedding
 *               would raise IndexError).
 * The forward is bitwise deterministic (no atomics) and a read's logits do not depend on the other reads of its batch.
 * clm_cnn_debug_fetch names (the last forward): "block0" fp32 [B, L/4, 256], "block1" fp32 [B, L/16, 256], "partial" fp32
 * [B, ceil((L/64) / 16), 256] (block 2's pooled rows summed per tile of 16; block 2 stores nothing else), "pooled" fp32 [B, 256]
 * (the mean of block 2's output: the partials added in order, over L/64). */
typedef struct clm_cnn_handle clm_cnn_handle;
int clm_cnn_create(int device, int precision, clm_cnn_handle** out);
int clm_cnn_load_weight(clm_cnn_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
int clm_cnn_finalize(clm_cnn_handle* h);
int clm_cnn_forward(clm_cnn_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                    void* stream);
int clm_cnn_debug_fetch(clm_cnn_handle* h, const char* name, void* host_out, size_t bytes);
const char* clm_cnn_last_error(const clm_cnn_handle* h); /* h may be NULL: error of the last failed clm_cnn_create */
int clm_cnn_destroy(clm_cnn_handle* h);

/* ---- DNAConvNet in training mode (ABI 6, additive; chimeralm_amd/cnntrain.py) ------------------------------------------------
 * Forward on batch statistics and the full backward of the three convolution blocks and the mean over positions, on the CALLER's
 * current fp32 parameters (device pointers); the classifier `fc` sees [B, 256] and is the caller's.  Exact fp32
 * (v_mfma_f32_32x32x2_f32) whatever the inference precision; no floating-point atomics and every reduction in a fixed order: the
 * same inputs give the same bits.  Rows are token-major [B, L_i, 256], L_0 = L, L_{i+1} = floor(L_i / 4); pads are ordinary tokens.
 *   block i:  z = conv1d_same(x_i; W_i, b_i) on all L_i positions (x_0 = embedding rows; zero outside [0, L_i));
 *             mu_c, v_c = mean and biased variance of z[:, :, c] over all B L_i positions (those past 4 L_{i+1} included);
 *             xh = (z - mu) / sqrt(v + 1e-5);  y = gelu_erf(g xh + beta);  p[b, j, c] = max_{r < 4} y[b, 4 j + r, c], routed in the
 *             backward to choice[b, j, c] = the LOWEST r that attains it (torch's rule);  x_{i+1} = p keep keep_scale
 *   pooled[b] = mean_j x_3[b, j, :]
 *   backward: dz = g rstd (dy - mean(dy) - xh mean(dy xh)), dg = sum dy xh, dbeta = sum dy, db_i = sum dz (0 in exact arithmetic;
 *             what the sum gives is returned), dW_i[co, ci, k] = sum_{b, t} dz[b, t, co] x_i[b, t + k - 3, ci], dx_i = the "same"
 *             convolution of dz with the taps flipped and ci / co exchanged, d embedding[tok] = sum of dx_0 over the positions
 *             holding tok, row 4 (padding_idx) zero.
 * params / grads: CLM_CNN_TRAIN_PARAMS pointers in the order embedding [12, 256], then per block i = 0, 1, 2: W_i [256, 256, 7],
 * b_i, g_i, beta_i [256]; all 16-byte aligned.
 * clm_cnn_train_create    workspace_limit_bytes = 0: 64 GiB.  BatchNorm couples the reads of a batch, so a batch is never computed
 *               in pieces: one whose workspace (clm_cnn_train_workspace_bytes) exceeds the limit is CLM_E_INVALID, bytes in the message.
 * clm_cnn_train_forward   ids as clm_cnn_forward takes them; keep: NULL (no dropout) or three byte masks [B, L_{i+1}, 256] (non-zero =
 *               keep) that must stay alive until the backward has run; keep_scale = 1 / (1 - p).  Writes pooled_out [B, 256] and the
 *               batch statistics mean_out, var_out [3, 256] (biased variance).  B >= 2 and L >= 64, otherwise CLM_E_INVALID; B > 65535
 *               or B L > 2^30 is CLM_E_UNSUPPORTED.  A refused call launches nothing and leaves the handle as it was.
 * clm_cnn_train_generation   moves with every forward on the handle (-1 for NULL).
 * clm_cnn_train_backward  dpooled [B, 256]; grads = beta * (what they hold) + the gradients, beta 0 or 1.  `generation` is the value
 *               after the forward to differentiate: CLM_E_STATE if no forward is pending (none ran, or its backward already did) or
 *               another forward ran on the handle since -- and nothing is launched.
 * Both are asynchronous on `stream` and do not synchronise (a forward that has to grow the workspace does, once).
 * clm_cnn_train_debug_fetch names (synchronises): "z0".."z2", "y0".."y2" fp32 [B, L_i, 256]; "choice0".."choice2" u8
 * [B, L_{i+1}, 256]; "dz0".."dz2" fp32 [B, L_i, 256] (after the backward, else CLM_E_STATE). */
#define CLM_CNN_TRAIN_PARAMS 13
typedef struct clm_cnn_train_handle clm_cnn_train_handle;
int clm_cnn_train_create(int device, size_t workspace_limit_bytes, clm_cnn_train_handle** out);
int64_t clm_cnn_train_workspace_bytes(int B, int L); /* < 0: CLM_E_INVALID (B < 1 or L < 64) */
int clm_cnn_train_forward(clm_cnn_train_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L,
                          const float* const* params, const unsigned char* const* keep, float keep_scale, float* pooled_out,
                          float* mean_out, float* var_out, void* stream);
int64_t clm_cnn_train_generation(const clm_cnn_train_handle* h);
int clm_cnn_train_backward(clm_cnn_train_handle* h, int64_t generation, const float* dpooled, float* const* grads, float beta,
                           void* stream);
int clm_cnn_train_debug_fetch(clm_cnn_train_handle* h, const char* name, void* host_out, size_t bytes);
const char* clm_cnn_train_last_error(const clm_cnn_train_handle* h); /* h may be NULL: the last failed clm_cnn_train_create */
int clm_cnn_train_destroy(clm_cnn_train_handle* h);

/* ---- Mamba2 classifiers (ABI 6, additive) -----------------------------------------------------------------------------
 * The reference's two Mamba nets (chimeralm/models/components/mamba.py) in eval mode, behind the same `net`
 * boundary: forward(input_ids[B, L], second argument) -> logits fp32 [B, 2].
 *   CLM_MAMBA_SEQ  MambaSequenceClassification (configs/model/mamba.yaml: d 256, 12 layers, d_state 16, expand 2):
 *                  LayerNorm(Linear(E[id] + pos_embedding[t])), then h += Mamba2(h) per layer; `mask` [B, L] (the reference's
 *                  `attention_mask`, optional) multiplies h after the front and after every residual add.  L > model_max_length
 *                  is CLM_E_INVALID.
 *   CLM_MAMBA_SP   MambaSequenceClassificationSP (configs/model/mambasp.yaml: d 512, 3 layers, d_state 128, expand 3): h = E[id];
 *                  `mask` is ignored, as the reference ignores its second argument; any L.
 * Both: pooled = (mean_t h + max_t h) / 2 over all L positions, pooler Linear + GELU, classifier Linear + GELU + Linear.  Mamba2 is
 * mamba_ssm 2.x's with its defaults (ngroups 1, gated RMSNorm after the gate, per-head D, no projection bias, conv bias, zero
 * initial state); tests/mamba_reference.py states its arithmetic.
 * Same conventions as the clm_cnn_* calls; weights under the reference module's state_dict keys (with or without `net.`), fp32 only.
 *   create      variant, precision, d_model (256 or 512), n_layers (>= 1), d_state (16, 32, 64 or 128), expand (d_inner = expand x
 *               d_model), headdim (64), model_max_length (CLM_MAMBA_SEQ: the positional table's length; ignored otherwise).
 *               Anything else is CLM_E_INVALID.
 *   precision   CLM_PREC_F32 (exact fp32 MFMA) or CLM_PREC_F16X3 (the projections as three fp16 MFMAs on hi + lo halfs).  The
 *               fp16x3 weight packing saturates for |w| >= 64 (out_proj counted with norm.weight folded in): then finalize packs
 *               that handle's weights for the exact-fp32 kernels.  An activation beyond fp16's range entering an fp16x3 projection
 *               makes that tile's outputs NaN (the caller reruns the batch on an fp32 handle).  The scan, the norms and the head
 *               are fp32 in both modes.
 *   ids         i64, i32 or u8; an id outside [0, 12) is clamped into it.
 *   mask        fp32 [B, mask_row_stride] device pointer or NULL.
 * Long batches run in chunks of whole reads (the in_proj output of one chunk is bounded at 4 GiB).  The forward is bitwise
 * deterministic (no atomics) and a read's logits do not depend on the other reads of its batch.
 * clm_mamba_debug_fetch names (the last forward): "front" fp32 [B, L, d] (the residual stream entering layer 0), "layer0" fp32
 * [B, L, d] (after layer 0) -- both only while B x L x d x 4 <= 256 MiB -- and "pooled" fp32 [B, d].  The workspace of the LAST
 * layer, as the forward left it and only when the batch ran as one chunk of reads (CLM_E_INVALID otherwise): "zx" fp32 [B, L,
 * n_in_pad] (in_proj output z | x | B | C | dt with softplus applied | zero padding; n_in_pad = 2 di + 2 N + H rounded up to a multiple
 * of 256), "xc" fp32 [B, L, di + 2 N] (conv + SiLU), "g" fp32 [B, L, di] (scan output, gated, before the RMS scale), "ssq" fp32 [B, L,
 * H] (per-head sums of g^2), "part" fp32 [B, ceil(L / 64), 2, d] (per 64-token tile: channel sums | maxima of the last layer's rows). */
#define CLM_MAMBA_SEQ 0
#define CLM_MAMBA_SP 1
typedef struct clm_mamba_handle clm_mamba_handle;
int clm_mamba_create(int device, int variant, int precision, int d_model, int n_layers, int d_state, int expand, int headdim,
                     int model_max_length, clm_mamba_handle** out);
int clm_mamba_load_weight(clm_mamba_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
int clm_mamba_finalize(clm_mamba_handle* h);
int clm_mamba_forward(clm_mamba_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, const float* mask,
                      int64_t mask_row_stride, float* logits_out, void* stream);
/* The running verdict of the Mamba nets (ABI 6, additive): clm_mamba_forward that also leaves the request of `traj`, the clm_traj_out
 * / clm_traj_summary of clm_forward_traj above with its points, its stride contract (a multiple of 128 in 128 ... 4,096) and its
 * summary, unchanged.  Both nets are causal end to end (embedding, positional term and mask per token, the causal 4-tap convolution,
 * the scan from a zero state, the per-token RMSNorm), and a prefix of their pooling is a running sum and a running maximum, so the
 * whole trajectory follows from the per-64-token partials one forward leaves behind.
 *   trajectory  logits[b][k] = head((mean + max) / 2 over h[b, :n_k]), head = pooler Linear + GELU, classifier Linear + GELU + Linear.
 *               The mean divides by n_k, pads and masked rows included (a masked row is a row of zeros: it counts in the mean and
 *               takes part in the maximum), because that is what the reference's forward of ids[b:b+1, :n_k] (and mask[b:b+1, :n_k])
 *               computes.  Point K - 1 is the call's own logits_out[b], copied bit for bit, not recomputed.  The values are those of
 *               the arithmetic the handle ran (fp32 or fp16x3).  As above, a truncated row does not end in [SEP]: no point but the
 *               last shows the model a complete read; points inside the [PAD] prefix of a left-padded row describe pads only.
 * CLM_E_INVALID, each with a message in clm_mamba_last_error: a stride that is not such a multiple, point_stride < K, traj->logits
 * NULL, a struct_size mismatch.  No length cap beyond the forward's own.  Device pointers for the B reads of the call, written chunk by
 * chunk at their rows by two kernels behind the head on `stream` (csrc/mamba_verdict.hip) and the summary kernel of
 * csrc/trajectory.hip: fixed order, no atomics -- bitwise the same from run to run; the workspace is the handle's and is reserved by
 * the first request.  With traj NULL this IS clm_mamba_forward. */
int clm_mamba_forward_traj(clm_mamba_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, const float* mask,
                           int64_t mask_row_stride, float* logits_out, const clm_traj_out* traj, void* stream);
int clm_mamba_debug_fetch(clm_mamba_handle* h, const char* name, void* host_out, size_t bytes);
const char* clm_mamba_last_error(const clm_mamba_handle* h); /* h may be NULL: error of the last failed clm_mamba_create */
int clm_mamba_destroy(clm_mamba_handle* h);

/* ---- The Mamba2 core in training form (ABI 6, additive; chimeralm_amd/mambatrain.py) ---------------------------------------------
 * What lies between in_proj and out_proj of one Mamba2 layer, forward and backward, on the CALLER's tensors (fp32 device pointers,
 * 16-byte aligned, contiguous, token-major rows).  With di = expand x d_model, H = di / 64, P = 64, N = d_state, conv_dim = di + 2 N:
 *   zxbcdt [B, L, 2 di + 2 N + H] = z | xBC | dt (the raw in_proj output)
 *   xc = silu(causal depthwise conv of xBC, 4 taps, + bias) = x | B | C, inside each read;  dt = softplus(raw + dt_bias)
 *   ys = scan(x, dt, A = -exp(A_log), B, C) + D x, from a zero state per read, in chunks of 64 tokens (tests/mamba_reference.py)
 *   out [B, L, di] = norm.weight g rsqrt(mean_c g^2 + 1e-5),  g = ys silu(z)          (what out_proj consumes)
 * Exact fp32 (products on v_mfma_f32_32x32x2_f32); no floating-point atomics and every reduction in a fixed order, partials of
 * different workgroups combined in fp64 in workgroup order: the same inputs give the same bits.  Pads are ordinary tokens.
 * params / dparams: CLM_MAMBA_TRAIN_PARAMS pointers in the order conv1d.weight [conv_dim, 1, 4], conv1d.bias [conv_dim], dt_bias [H],
 * A_log [H], D [H], norm.weight [di].
 * The op is stateless across calls: what the backward needs is written by the forward into buffers of the caller, who keeps them
 * (and zxbcdt) until the backward has run --
 *   xc [B, L, conv_dim], dt [B, L, H], ys [B, L, di], states [B, H, ceil(L / 64), N, 64] (every chunk's entry state).
 * clm_mamba_train_backward  dout [B, L, di] -> dzxbcdt (zxbcdt's shape; every element written) and the six parameter gradients
 *               (overwritten).  Its scratch belongs to the handle and is grown on demand (one synchronisation when it grows):
 *   clm_mamba_train_workspace_bytes = 4 x (B L (2 di + H + 2 N H) + B ceil(L / 64) (di + 5 conv_dim + H) + 2 B H)
 *               (dys, dx, ddt, the heads' dB | dC; the 64-row partials of norm.weight, conv1d.weight / bias and dt_bias; dA_log and dD
 *               per (read, head)).  A negative value is the refusal's code.
 * Calls on one handle are ordered by the caller (one stream at a time).  B < 1 or L < 1 is CLM_E_INVALID; d_model other than 256 /
 * 512, d_state other than 16 / 32 / 64 / 128, expand outside 1 ... 1024, or a batch beyond the index range (B L or a launch grid
 * >= 2^31) is CLM_E_UNSUPPORTED.  A refused call launches nothing.  Both calls are asynchronous on `stream`. */
#define CLM_MAMBA_TRAIN_PARAMS 6
typedef struct clm_mamba_train_handle clm_mamba_train_handle;
int clm_mamba_train_create(int device, clm_mamba_train_handle** out);
int64_t clm_mamba_train_workspace_bytes(int B, int L, int d_model, int expand, int d_state);
int clm_mamba_train_forward(clm_mamba_train_handle* h, const float* zxbcdt, const float* const* params, int B, int L, int d_model,
                            int expand, int d_state, float* xc, float* dt, float* ys, float* states, float* out, void* stream);
int clm_mamba_train_backward(clm_mamba_train_handle* h, const float* zxbcdt, const float* const* params, int B, int L, int d_model,
                             int expand, int d_state, const float* xc, const float* dt, const float* ys, const float* states,
                             const float* dout, float* dzxbcdt, float* const* dparams, void* stream);
const char* clm_mamba_train_last_error(const clm_mamba_train_handle* h); /* h may be NULL: the last failed clm_mamba_train_create */
int clm_mamba_train_destroy(clm_mamba_train_handle* h);

/* ---- test-stage metrics (ABI 6, additive) -----------------------------------------------------------------------------
 * What the reference's `test_step` feeds to torchmetrics on the host after a sync per batch (basic_module.py:153-175), summed on the
 * device instead: the logits of a batch never leave it and the host waits once, in clm_eval_read.
 *   create      n_classes must be 2 (binary F1 / precision / recall); `ignore_index` is the criterion's (torch's default -100).
 *               device -1 makes a host-only handle that needs no GPU: it totals results (merge, read, reset); update is CLM_E_STATE.
 *   update      logits fp32 [B, 2] contiguous and labels int64 [B], both device pointers; B >= 1.  One launch of one workgroup on
 *               `stream`, no atomics, a fixed reduction order: the sums are bitwise the same from run to run.  It does not
 *               synchronise.  Updates of one handle are ordered by the stream: use one stream per handle (the one the logits were
 *               produced on needs no event).
 *               Per row: label == ignore_index is skipped; otherwise a label outside {0, 1} counts in n_invalid_labels and a row
 *               with a NaN / inf logit in n_nonfinite, and neither enters any sum (the reference raises inside the loss / computes
 *               NaN).  A valid row adds loss = logsumexp(l0, l1) - l[label], in double from the fp32 logits with the maximum
 *               subtracted first, and one of tp / fp / tn / fn with prediction = 1 only if l1 > l0 (a tie is 0, as torch.argmax).
 *               A batch with at least one valid row adds its mean loss over its valid rows to sum_batch_mean_loss and 1 to
 *               n_batches (the reference's MeanMetric weights batches alike), its ignored rows to n_ignored.  A batch with no valid
 *               row adds 1 to n_empty_batches; of its rows only invalid labels and non-finite logits are still counted.
 *   read        copies the sums to the host behind everything queued on `stream` and waits for that copy: the one sync of the
 *               stage.  Sums merged in from other ranks are included.
 *   merge       adds another handle's result (another rank's) to this handle's, on the host.  Ranks that want the same bits each
 *               merge every rank's result, their own included, in rank order into a host-only handle.
 *   reset       zeroes device and merged sums, behind what is queued on `stream`. */
typedef struct clm_eval_handle clm_eval_handle;
typedef struct clm_eval_result {
    int64_t tp, fp, tn, fn;
    int64_t n_valid, n_ignored, n_batches, n_empty_batches, n_invalid_labels, n_nonfinite;
    double sum_batch_mean_loss, sum_loss;
} clm_eval_result;
int clm_eval_create(int device, int n_classes, int64_t ignore_index, clm_eval_handle** out);
int clm_eval_update(clm_eval_handle* h, const float* logits, const int64_t* labels, int B, void* stream);
int clm_eval_read(clm_eval_handle* h, clm_eval_result* out, void* stream);
int clm_eval_merge(clm_eval_handle* h, const clm_eval_result* other);
int clm_eval_reset(clm_eval_handle* h, void* stream);
const char* clm_eval_last_error(const clm_eval_handle* h); /* h may be NULL: error of the last failed clm_eval_create */
int clm_eval_destroy(clm_eval_handle* h);

/* ---- in-silico mutagenesis: per-base importance for every net (ABI 6, additive) ------------------------------------------
 * Replaces Mamba2Analyzer.get_position_importance of the reference (chimeralm/explain/motif.py:64-82): replace one base by N, run
 * the model again, report |p1(read) - p1(mutant)| per position -- one forward and one host wait per position there.  Here the
 * mutants of a read are built on the device in batches, the forward between "rows" and "scores" is the net's own on the uint8
 * rows (any of the clm_*_forward calls), and nothing waits on the host.  The calls are tied to no net.
 *
 * The read     n_bases base ids (A, C, G, T, N = 7 ... 11) followed by [SEP] (id 1), as `predict` tokenises it, no pads:
 *              L = n_bases + 1, 1 <= n_bases <= 32768.  (The reference feeds ord(c) and no [SEP] to a model trained on this
 *              tokenisation; that is a bug there and is not reproduced.)
 * Windows      window w >= 1, stride s with 1 <= s <= w: window k starts at base k * s and covers the bases
 *              [k * s, min(k * s + w, n_bases)); n_windows = ceil(n_bases / s).  [SEP] is never replaced.
 * Substitute   CLM_EXPLAIN_SUB_N: every base of the window becomes N; S = 1 column per window.
 *              CLM_EXPLAIN_SUB_ALL: saturation mutagenesis, needs w = s = 1; S = 4 columns A, C, G, T.  The column of the read's
 *              own base is exactly 0.0 and has no mutant (no forward is spent on it); a base that is N has all four.
 * A mutant     clm_explain_mutant: the first base of its window, the substitute id, and its slot k * S + column in dp1 / dgap.
 * Outputs      logits [M + 1, 2] fp32: row 0 the unmodified read, rows 1 ... M the mutants in plan order, as the net returned them.
 *              dp1, dgap [n_windows, S] fp32, signed, mutant minus read: p1 = softmax(logits)[1] in double from the fp32 logits with
 *              the maximum taken out first (as clm_eval_update), gap = l1 - l0 in double.  A mutant with a NaN / inf logit has NaN
 *              in both and counts in n_nonfinite.
 *              importance [n_bases] fp32: the maximum of |d| over the windows that cover the base and over the S columns, d being
 *              dp1 (the reference's number for w = s = 1 and N) or dgap (which does not vanish on confident reads); NaN if one of
 *              them is NaN.
 *              peak_pos int32 / peak_val fp32 [top_k], 1 <= top_k <= 32: the min(top_k, n_bases) bases of largest importance in
 *              descending order, equal values by the lower position (a total order, as for the attention peaks: the result does
 *              not depend on the shape of the reduction); positions 0-based among the bases; slots beyond hold -1 and 0.  A read
 *              with any NaN importance reports no peaks.
 *   plan       host only, needs no GPU and no handle: enumerates the mutants of `ids` [L] (host memory) in window order, columns
 *              ascending.  Writes at most `capacity` entries to `plan` (NULL: count only) and always the counts; more mutants than
 *              capacity, a token that is not a base, a missing [SEP] and bad options are CLM_E_INVALID (clm_explain_last_error of
 *              NULL has the text).  The caller uploads the plan once per read.
 *   rows       device: writes mutants m0 ... m0 + rows - 1 of the plan as uint8 rows of L ids to `out`, row r at out + r *
 *              row_stride.  16-byte stores: `ids` and `out` 16-byte aligned, row_stride a multiple of 16 and >= L; the bytes of a
 *              row between L and the next multiple of 16 are written as 0.  rows <= 65535.  ids [L], plan: device pointers.
 *   scores     device, one workgroup behind the forward of a batch: batch_logits [rows, 2] fp32 as the net wrote them.  With
 *              has_base = 1 (the read's first batch, m0 = 0) row 0 is the unmodified read and rows 1 ... the mutants 0 ...: its
 *              logits are kept in the handle for the read's later batches (ordered by the stream), all n_slots = n_windows * S
 *              entries of dp1 / dgap are zeroed and *n_nonfinite starts at 0.  With has_base = 0 the rows are mutants m0 ...  Fills
 *              logits_out rows, dp1 / dgap at the mutants' slots, and adds to *n_nonfinite (int32, device).
 *   reduce     device, one workgroup: importance and peaks from d = dp1 or dgap [n_windows, n_sub] (n_sub = S).
 * All three launches go to `stream` and do not synchronise; no atomics and fixed reduction orders, so results are bitwise the same
 * from run to run.  One read at a time per handle (the handle holds the read's base logits); use one stream per handle. */
#define CLM_EXPLAIN_SUB_N 0
#define CLM_EXPLAIN_SUB_ALL 1
typedef struct clm_explain_handle clm_explain_handle;
typedef struct clm_explain_mutant {
    int32_t start;    /* first base of the window                   */
    int32_t sub;      /* the id its bases are replaced by (7 ... 11) */
    int32_t slot;     /* index into dp1 / dgap: window * S + column  */
    int32_t reserved; /* 0                                          */
} clm_explain_mutant;
int clm_explain_plan(const unsigned char* ids, int L, int window, int stride, int substitute, clm_explain_mutant* plan, int capacity,
                     int* n_mutants, int* n_windows);
int clm_explain_create(int device, clm_explain_handle** out);
int clm_explain_rows(clm_explain_handle* h, const unsigned char* ids, int L, int window, const clm_explain_mutant* plan, int n_mutants,
                     int m0, int rows, unsigned char* out, int64_t row_stride, void* stream);
int clm_explain_scores(clm_explain_handle* h, const float* batch_logits, int rows, int has_base, const clm_explain_mutant* plan,
                       int n_mutants, int m0, int n_slots, float* logits_out, float* dp1, float* dgap, int* n_nonfinite, void* stream);
int clm_explain_reduce(clm_explain_handle* h, const float* d, int n_bases, int window, int stride, int n_sub, int top_k,
                       float* importance, int* peak_pos, float* peak_val, void* stream);
const char* clm_explain_last_error(const clm_explain_handle* h); /* h may be NULL: error of the last failed clm_explain_create / _plan */
int clm_explain_destroy(clm_explain_handle* h);

/* ---- reads longer than the model's context, in overlapping windows (ABI 6, additive) ------------------------------------------
 * The reference truncates a read to the tokenizer's 32,768 bases (chimeralm/data/bam.py:166-170); the rest reaches no net.  These
 * calls cut a long read into overlapping context-sized windows around the net's own forward (any of the clm_*_forward calls on the
 * uint8 rows) and reduce the windows' logits to one pair per read.  They are tied to no net; nothing waits on the host.
 *
 * Window       Wb >= 1 bases, C = Wb + 1 tokens (the product: Wb = 32768).  Overlap O, 0 <= O <= Wb / 2; step = Wb - O.
 * Cap          max_bases >= Wb: a longer read is cut to its first max_bases bases before anything else.
 * Windows of a read of n bases (after the cap): n <= Wb: one window, the read itself.  Otherwise K = 1 + ceil((n - Wb) / step)
 *              windows of exactly Wb bases; window k < K - 1 starts at base k * step, the last at n - Wb (it ends on the read's
 *              last base).  A window row is its Wb bases followed by [SEP] (id 1), no pads.
 * The batch    ids uint8 [B, L] with row stride row_stride: each row [PAD] (id 4) x (L - n_tokens), then the read's n_tokens tokens
 *              (its bases and one [SEP]), untruncated.  [PAD] never occurs inside a read.
 * Head batch   the first forward: L_out = min(L, C) tokens wide; a read that fits is right-aligned with [PAD] on its left, a long
 *              read appears as its window 0 -- byte for byte the batch the truncating path delivers.
 * Extra rows   the windows k >= 1 of the batch's long reads, C tokens wide, in read order, then window order.
 * A span       clm_longread_span, one per output row, the B head rows first, then the extra rows: the output row is
 *              [PAD] x (width - n_copy - sep), then n_copy bytes of source row `read` from column src_col, then [SEP] if sep
 *              (bit 0 of flags).  A short read's head row copies its tokens, its own [SEP] included, with sep = 0.
 * Reduction    gap_k = (double)logit1_k - (double)logit0_k from the fp32 logits.  The chosen window has the largest gap, equal gaps
 *              go to the lowest k; if a window has a non-finite logit the chosen window is the lowest such k.  The read's logits
 *              are the chosen window's two floats, bit for bit.  With no non-finite window: label = OR of the windows' labels.
 *   lengths    host only: n_tokens [B] of a left-padded batch in host memory, by a search per row (not a pass over the bytes);
 *              the boundary is verified.  A row that ends in [PAD] (all pads, or padded on the right) or whose boundary is not
 *              [PAD] followed by a token is CLM_E_INVALID.
 *   plan       host only, needs no GPU and no handle.  Writes L_out, first [B + 1] (may be NULL; read r's extra windows are extra
 *              rows first[r] ... first[r + 1] - 1, so K_r = 1 + first[r + 1] - first[r]), n_spans = B + first[B], and at most
 *              `capacity` spans with each span's first base in `starts` (may be NULL).  spans = NULL: count only.  More spans than
 *              capacity, 1 > n_tokens[r] or n_tokens[r] > L and bad options are CLM_E_INVALID (clm_longread_last_error of NULL has
 *              the text).
 *   rows       device: writes spans s0 ... s0 + rows - 1 as rows of `width` bytes (L_out for head rows, C for extra rows), row r at
 *              out + r * out_stride; the bytes between width and the next multiple of 16 are written as 0.  16-byte stores: `out`
 *              16-byte aligned, out_stride a multiple of 16 that holds width rounded up to 16.  The source of a row starts at an
 *              arbitrary byte; it is read with aligned 16-byte loads, all inside the batch: `ids` 16-byte aligned, row_stride a
 *              multiple of 16 and >= L, the buffer holds B * row_stride bytes.  Anything else is CLM_E_INVALID and launches
 *              nothing.  1 <= rows <= 65535.  ids, spans, out: device pointers.
 *   reduce     device, one thread per read: logits [B + n_extra, 2] fp32 (head rows, then extra rows), first [B + 1] int32 ->
 *              logits_out [B, 2], chosen int32 [B], gap fp32 [B + n_extra], nonfinite int32 [B] (windows of the read with a
 *              non-finite logit).
 * Both launches go to `stream` and do not synchronise; no atomics and no sums across threads: bitwise the same from run to run. */
#define CLM_LONGREAD_SEP 1
typedef struct clm_longread_handle clm_longread_handle;
typedef struct clm_longread_span {
    int32_t read;    /* source row in the batch                     */
    int32_t src_col; /* first source column                         */
    int32_t n_copy;  /* bytes copied                                */
    int32_t flags;   /* bit 0 (CLM_LONGREAD_SEP): [SEP] follows them */
} clm_longread_span;
int clm_longread_lengths(const unsigned char* ids, int64_t row_stride, int B, int L, int32_t* n_tokens);
int clm_longread_plan(const int32_t* n_tokens, int B, int L, int window, int overlap, int max_bases, int* L_out, int32_t* first,
                      clm_longread_span* spans, int32_t* starts, int capacity, int* n_spans);
int clm_longread_create(int device, clm_longread_handle** out);
int clm_longread_rows(clm_longread_handle* h, const unsigned char* ids, int64_t row_stride, int B, int L, const clm_longread_span* spans,
                      int n_spans, int s0, int rows, unsigned char* out, int64_t out_stride, int width, void* stream);
int clm_longread_reduce(clm_longread_handle* h, const float* logits, const int32_t* first, int B, float* logits_out, int32_t* chosen,
                        float* gap, int32_t* nonfinite, void* stream);
const char* clm_longread_last_error(const clm_longread_handle* h); /* h may be NULL: the last failed _lengths / _plan / _create */
int clm_longread_destroy(clm_longread_handle* h);

/* ---- length-bucketed predict: a read's row depends on the read alone (ABI 6, additive) -----------------------------------------
 * The reference pads a batch on the left to its longest read (chimeralm/data/tokenizer.py:152-159) and masks nothing: a read's
 * logits depend on its batch-mates, and a ragged file pays for the pads.  These calls regroup the reads of the incoming batches
 * into batches of one canonical length each, around the net's own forward.  They are tied to no net; the left pads differ from
 * the reference's, so this mode is not reference parity.
 *
 * Row          a read of n tokens is b = n - 1 bases and one trailing [SEP] (id 1), truncated as today: 1 <= n <= 32769.
 * Canonical    with m = steps_log2 (0 ... 5, the product: 3): e = max(6, floor(log2(max(b, 1))) - m), q = 2^e and
 * length         Lc(n) = min(32769, 1 + q * max(1, ceil(b / q))).
 *              Quantum 64 up to 1,024 bases, then 2^m steps per octave; the ladder is laid on bases, so 1025, 2049, ..., 32769
 *              tokens are class tops with no pad.  Lc >= max(n, 65), Lc is monotone in n and Lc - n <= max(64, b / 2^m).
 * Bucket row   [PAD] (id 4) x (Lc - n), then the read's n tokens: a function of the read alone.
 * Regrouping   reads are taken in the order they arrive and each goes to the staging slab of its class (its Lc).  A class that
 *              reaches batch_size rows is emitted as one batch, rows in arrival order; at the end of the input (`finish`) the
 *              classes that hold rows are emitted in ascending Lc.  No class is merged into another.
 * Pool         one slab of batch_size rows of round16(Lc) bytes per class, laid behind one another in the order the classes first
 *              appear.  clm_bucket_pool_bytes is the size with every class of the ladder present (m = 3: 56 classes, 406,400
 *              bytes x batch_size).
 * Steps        what a push or finish asks of the caller, in order.  CLM_BUCKET_SCATTER: spans first ... first + count - 1 are
 *              written (clm_bucket_scatter).  CLM_BUCKET_EMIT: the class `length` holds `count` rows at pool + offset, `stride`
 *              bytes apart, ready to forward; they are the reads reads[first ... first + count - 1] (indices counted over all
 *              pushes since create, from 0).  A scatter group closes at every emit: the emitted rows go through the forward
 *              before a later group refills their slab (one stream orders both).
 * A span       clm_bucket_span: n_copy bytes of source row src_row from column src_col become the last n_copy bytes of a row of
 *              dst_width bytes at pool + dst_offset; [PAD] before them, zeroes up to the next multiple of 16 behind them.
 *   length     Lc(n_tokens), or CLM_E_INVALID for n_tokens outside 1 ... 32769 or steps_log2 outside 0 ... 5.
 *   plan       host only, needs no GPU.  push takes the token counts n_tokens [B] of a left-padded batch L columns wide (every one
 *              in 1 ... min(L, 32769); clm_longread_lengths finds them) and leaves steps, spans and reads in the planner, where
 *              clm_bucket_plan_steps finds them until the next push, finish or destroy.  A refused push changes nothing.
 *   scatter    device: writes spans[s0 ... s0 + rows - 1] (HOST memory: they are checked, then copied to the device behind the
 *              stream's earlier work).  A thread owns 16 destination bytes and stores them once; the source is read with aligned
 *              16-byte loads, each issued only inside [0, B * row_stride), each store only inside [0, pool_bytes).  `ids` and
 *              `pool` 16-byte aligned, row_stride a multiple of 16 and >= L, every span inside its source row and, rounded up to
 *              16 bytes, inside the pool at a 16-byte offset, n_copy <= dst_width <= 32769, 1 <= rows <= 65535: anything else is
 *              CLM_E_INVALID and launches nothing.  ids, pool: device pointers.  Up to 4,096 spans go out per launch, through a ring
 *              of eight page-locked buffers that clm_bucket_create allocates; the launches go to `stream` and do not synchronise,
 *              the call waits only for the launch eight launches back, whose buffer it reuses.  No atomics: bitwise the same from
 *              run to run. */
#define CLM_BUCKET_SCATTER 0
#define CLM_BUCKET_EMIT 1
#define CLM_BUCKET_MAX_TOKENS 32769
typedef struct clm_bucket_handle clm_bucket_handle;
typedef struct clm_bucket_plan clm_bucket_plan;
typedef struct clm_bucket_span {
    int32_t src_row;    /* source row in the batch                       */
    int32_t src_col;    /* first source column                           */
    int32_t n_copy;     /* bytes copied: the read's tokens               */
    int32_t dst_width;  /* the class's Lc                                */
    int64_t dst_offset; /* bytes into the pool, a multiple of 16         */
} clm_bucket_span;
typedef struct clm_bucket_step {
    int32_t kind;   /* CLM_BUCKET_SCATTER | CLM_BUCKET_EMIT                              */
    int32_t first;  /* scatter: the first span; emit: the first entry of reads           */
    int32_t count;  /* scatter: spans; emit: rows                                        */
    int32_t length; /* emit: the class's Lc (scatter: 0)                                 */
    int64_t offset; /* emit: the slab's offset in the pool (scatter: 0)                  */
    int64_t stride; /* emit: bytes from row to row, round16(Lc) (scatter: 0)             */
} clm_bucket_step;
int clm_bucket_length(int n_tokens, int steps_log2);
int64_t clm_bucket_pool_bytes(int batch_size, int steps_log2); /* < 0: CLM_E_INVALID */
int clm_bucket_plan_create(int batch_size, int steps_log2, clm_bucket_plan** out);
int clm_bucket_plan_push(clm_bucket_plan* p, const int32_t* n_tokens, int B, int L);
int clm_bucket_plan_finish(clm_bucket_plan* p);
int clm_bucket_plan_steps(const clm_bucket_plan* p, const clm_bucket_step** steps, int* n_steps, const clm_bucket_span** spans,
                          int* n_spans, const int64_t** reads, int* n_reads);
const char* clm_bucket_plan_last_error(const clm_bucket_plan* p); /* p may be NULL: the last failed _length / _pool_bytes / _create */
int clm_bucket_plan_destroy(clm_bucket_plan* p);
int clm_bucket_create(int device, clm_bucket_handle** out);
int clm_bucket_scatter(clm_bucket_handle* h, const unsigned char* ids, int64_t row_stride, int B, int L, const clm_bucket_span* spans,
                       int n_spans, int s0, int rows, unsigned char* pool, int64_t pool_bytes, void* stream);
const char* clm_bucket_last_error(const clm_bucket_handle* h); /* h may be NULL: the last failed clm_bucket_create */
int clm_bucket_destroy(clm_bucket_handle* h);

/* ---- fine-tuning the head with the backbone frozen (chimeralm_amd/headtrain.py) -------------------
 * The backbone runs as in inference and leaves the final residual rows h fp32 [B, L, 256] (before ln_f) on the device; the attention
 * pooling -- the one part of the head that sees L tokens per read -- runs forward and backward here on the CALLER's current weights
 * (device pointers, fp32: attention.0.weight w1 [256, 256] and bias b1 [256], attention.2.weight w2 [256] and bias b2 [1]); ln_f and
 * its eps come from the finalized handle.  The classifier behind the pooling sees one 256-vector per read and is the caller's.
 *   per read, x_t = ln_f(h_t):  s_t = w2 . gelu(w1 x_t + b1) + b2,  a = softmax_t(s) over all L positions,  pooled = sum_t a_t x_t
 *
 * clm_rows      device pointer, reads and tokens of the rows the LAST forward on this handle left.  CLM_E_STATE if there was none
 *               (since the weights were loaded) or it ran more than one chunk (B > chunk_reads: only the last chunk's rows are left);
 *               CLM_E_UNSUPPORTED unless it ran the exact-fp32 or fp16x3 kernels.  The pointer is the handle's workspace: the next
 *               forward (or weight load) rewrites or frees it.  clm_rows_generation moves whenever that may have happened: compare
 *               it before reading rows taken earlier.
 * clm_pool_forward   rows [B, L, 256] (any device pointer) -> scores_out [B, L] (before the softmax), stats_out [B, 2] (max, sum of
 *               exp(s - max)), pooled_out [B, 256].
 * clm_pool_backward  with the forward's scores, stats and pooled and dpooled [B, 256] = dloss/dpooled:
 *               d_w1 [256, 256], d_b1 [256], d_w2 [256], d_b2 [1] = beta * (what they hold) + the gradients; beta is 0 (they are not
 *               read) or 1 (micro-batches accumulate).  Exact fp32 (v_mfma_f32_32x32x2_f32), no floating-point atomics: the same
 *               inputs give the same bits.  d_b2 is 0 in exact arithmetic (softmax is shift-invariant); what the sum gives is returned.
 * Both: asynchronous on `stream`; CLM_E_INVALID for B or L < 1, a null pointer, another beta, or rows / weights / scores / pooled /
 * dpooled that are not 16-byte aligned (the kernels read them 16 bytes at a time), CLM_E_STATE before clm_finalize,
 * CLM_E_UNSUPPORTED for B > 65535 or L > max_seq_len -- and nothing is launched.  One call at a time per handle (they share its
 * workspace, in stream order). */
/* Reads of L tokens the handle pushes through all layers as ONE chunk right now (chunk_reads, capped by tokens, even above one):
 * the largest B whose forward leaves all its rows for clm_rows.  After clm_finalize; otherwise, or for L < 1, CLM_E_INVALID. */
int clm_chunk_reads(const clm_handle* h, int L);
int clm_rows(clm_handle* h, const float** rows, int* B, int* L);
int64_t clm_rows_generation(const clm_handle* h); /* -1 for NULL */
int clm_pool_forward(clm_handle* h, const float* rows, int B, int L, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* scores_out, float* stats_out, float* pooled_out, void* stream);
int clm_pool_backward(clm_handle* h, const float* rows, int B, int L, const float* w1, const float* b1, const float* w2,
                      const float* scores, const float* stats, const float* pooled, const float* dpooled, float* d_w1, float* d_b1,
                      float* d_w2, float* d_b2, float beta, void* stream);

/* ---- test / measurement taps (not on the product path) -------------------------------------------- */

/* Copy a named intermediate of the LAST clm_forward to host memory (synchronises the device).  Names:
 *   "hidden"        fp32 [B, L, 256]  residual stream after the final block (before ln_f)
 *   "scores"        fp32 [B, L]       pooling scores before the softmax
 *   "pooled"        fp32 [B, 256]
 *   "filter.<i>"    fp32 [L, 256]     implicit long filter of layer i for the last L
 * Only data of the last processed chunk is meaningful for "hidden"/"scores" when B > chunk_reads. */
int clm_debug_fetch(clm_handle* h, const char* name, void* host_out, size_t bytes);
/* Make clm_forward return right after stage `stage` (CLM_STAGE_*) of block `layer` (-1 with CLM_STAGE_EMBED:
 * after the embedding); the raw buffers "h", "z" [B,768,Lp], "y" [B,256,Lp], "u" [B,L,1024] can then be
 * fetched (z/y/u in the activation storage type of the precision mode).  layer = -1, stage = -1 disables. */
int clm_debug_stop_after(clm_handle* h, int layer, int stage);

/* Per-stage device timing with HIP events on the forward stream.  Stage names: clm_profile_stage_name. */
#define CLM_STAGE_EMBED 0
#define CLM_STAGE_INPROJ 1
#define CLM_STAGE_CONV 2
#define CLM_STAGE_OUTPROJ 3
#define CLM_STAGE_FC1 4
#define CLM_STAGE_FC2 5
#define CLM_STAGE_SCORE 6
#define CLM_STAGE_POOL 7
#define CLM_STAGE_HEADMLP 8
#define CLM_STAGE_FILTER 9
#define CLM_STAGE_TAIL 10   /* profile only: fused out_proj + LN2 + fc1 + GELU + fc2 (16-bit modes) */
#define CLM_STAGE_MLP 11    /* profile only: fused LN2 + fc1 + GELU + fc2 (16-bit modes, CLM_DEBUG=split_tail) */
#define CLM_N_STAGES 12
int clm_profile_enable(clm_handle* h, int on);
/* Synchronises, then returns accumulated milliseconds and launch counts per stage since the last reset. */
int clm_profile_read(clm_handle* h, double* ms_out /*[CLM_N_STAGES]*/, int64_t* launches_out /*[CLM_N_STAGES]*/,
                     int reset);
const char* clm_profile_stage_name(int stage);

const char* clm_last_error(const clm_handle* h); /* h may be NULL: error of the last failed clm_create */
int clm_destroy(clm_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* CHIMERALM_HIP_H */
