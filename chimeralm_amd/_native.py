"""ctypes binding of the C ABI declared in include/chimeralm_hip.h (csrc/libchimeralm_hip.so).

There is no fallback: if the shared library is missing or does not export the full ABI, importing the
engine fails loudly.  Build it with `python -m chimeralm_amd.build` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

# CLM_LIB points development A/B runs at another build of the same ABI; the product default is the in-tree library
LIB_PATH = Path(os.environ.get("CLM_LIB") or Path(__file__).resolve().parent / "csrc" / "libchimeralm_hip.so")

# error codes / enums (mirror include/chimeralm_hip.h)
OK, E_INVALID, E_HIP, E_MISSING, E_UNSUPPORTED, E_STATE = 0, -1, -2, -3, -4, -5
DT_F32, DT_F64, DT_BF16, DT_F16, DT_U8, DT_I32, DT_I64 = range(7)
PREC_F32, PREC_BF16, PREC_F16, PREC_F16C, PREC_F16X3 = 0, 1, 2, 3, 4
BAM_INPUT_SAM, BAM_KEEP_UNPLACED = 1, 2
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "bf16": PREC_BF16, "fp16": PREC_F16, "f16": PREC_F16, "fp16c": PREC_F16C, "fp16x3": PREC_F16X3}
PREC_NAMES = {PREC_F32: "fp32", PREC_BF16: "bf16", PREC_F16: "fp16", PREC_F16C: "fp16c", PREC_F16X3: "fp16x3"}
STAGES = ["embed", "ln1_in_proj", "short_long_conv", "out_proj", "ln2_fc1_gelu", "fc2", "lnf_pool_score",
          "softmax_pool", "head_mlp", "filter", "out_proj_ln2_mlp", "ln2_mlp"]
N_STAGES = len(STAGES)
ABI_VERSION = 6
ATTN_MAX_TOP_K = 32                   # clm_attn_out.top_k: 1 ... 32
TRAJ_STRIDE_UNIT, TRAJ_STRIDE_MAX = 128, 4096   # clm_traj_out.stride: a multiple of 128 in 128 ... 4096
EXPLAIN_SUB_N, EXPLAIN_SUB_ALL = 0, 1   # clm_explain_plan substitutes (CLM_EXPLAIN_SUB_*)
EXPLAIN_MAX_BASES = 32768             # bases of one read the explain calls take
LONGREAD_SEP = 1                      # clm_longread_span.flags bit 0 (CLM_LONGREAD_SEP)
BUCKET_SCATTER, BUCKET_EMIT = 0, 1     # clm_bucket_step.kind (CLM_BUCKET_*)
BUCKET_MAX_TOKENS = 32769             # tokens of the longest row the bucket calls take (CLM_BUCKET_MAX_TOKENS)
X3_WEIGHT_LIMIT = 64.0                # |w| at which fp16x3's weight packing (w x 2^10 as fp16 hi + lo) saturates (clm_common.h)
MAMBA_SEQ, MAMBA_SP = 0, 1            # clm_mamba_create variants (CLM_MAMBA_SEQ, CLM_MAMBA_SP)


class ClmConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("d_model", C.c_int32), ("n_layer", C.c_int32), ("d_inner", C.c_int32),
        ("vocab_rows", C.c_int32), ("filter_order", C.c_int32), ("emb_dim", C.c_int32), ("max_seq_len", C.c_int32),
        ("head_hidden", C.c_int32), ("n_classes", C.c_int32), ("ln_eps", C.c_float), ("precision", C.c_int32),
        ("chunk_reads", C.c_int32),
    ]


class ClmFeederConfig(C.Structure):          # include/chimeralm_feed.h: struct clm_feeder_config
    _fields_ = [("struct_size", C.c_int32), ("batch_size", C.c_int32), ("max_tokens", C.c_int32), ("slots", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32), ("pad_left", C.c_int32), ("pinned", C.c_int32),
                ("max_reads", C.c_int64), ("inflate_threads", C.c_int32), ("reserved", C.c_int32)]


class ClmFeedBatch(C.Structure):              # include/chimeralm_feed.h: struct clm_feed_batch
    _fields_ = [("slot", C.c_int32), ("n_reads", C.c_int32), ("n_tokens", C.c_int32), ("reserved", C.c_int32),
                ("row_stride", C.c_int64), ("ids", C.c_void_p), ("names", C.c_void_p), ("first_index", C.c_int64)]


class ClmEvalResult(C.Structure):             # include/chimeralm_hip.h: struct clm_eval_result
    _fields_ = [(n, C.c_int64) for n in ("tp", "fp", "tn", "fn", "n_valid", "n_ignored", "n_batches", "n_empty_batches",
                                         "n_invalid_labels", "n_nonfinite")] + [("sum_batch_mean_loss", C.c_double),
                                                                                ("sum_loss", C.c_double)]


class ClmAttnSummary(C.Structure):            # include/chimeralm_hip.h: struct clm_attn_summary (one record per read)
    _fields_ = [("n_pad", C.c_int32), ("n_bases", C.c_int32), ("has_sep", C.c_int32), ("n_peaks", C.c_int32),
                ("pad_weight", C.c_float), ("sep_weight", C.c_float), ("base_weight", C.c_float), ("reserved", C.c_int32)]


class ClmAttnOut(C.Structure):                # include/chimeralm_hip.h: struct clm_attn_out
    _fields_ = [("struct_size", C.c_int32), ("top_k", C.c_int32), ("weights", C.c_void_p), ("weights_row_stride", C.c_int64),
                ("summary", C.c_void_p), ("peak_pos", C.c_void_p), ("peak_weight", C.c_void_p)]


class ClmTrajSummary(C.Structure):            # include/chimeralm_hip.h: struct clm_traj_summary (one record per read)
    _fields_ = [(n, C.c_int32) for n in ("n_pad", "n_bases", "has_sep", "n_points", "first_k", "label", "onset_k", "jump_k",
                                         "n_nonfinite", "reserved")] + [("jump_dgap", C.c_float), ("final_gap", C.c_float)]


class ClmTrajOut(C.Structure):                # include/chimeralm_hip.h: struct clm_traj_out
    _fields_ = [("struct_size", C.c_int32), ("stride", C.c_int32), ("logits", C.c_void_p), ("point_stride", C.c_int64),
                ("summary", C.c_void_p)]


class ClmLongreadSpan(C.Structure):           # include/chimeralm_hip.h: struct clm_longread_span
    _fields_ = [("read", C.c_int32), ("src_col", C.c_int32), ("n_copy", C.c_int32), ("flags", C.c_int32)]


class ClmBucketSpan(C.Structure):             # include/chimeralm_hip.h: struct clm_bucket_span
    _fields_ = [("src_row", C.c_int32), ("src_col", C.c_int32), ("n_copy", C.c_int32), ("dst_width", C.c_int32),
                ("dst_offset", C.c_int64)]


class ClmBucketStep(C.Structure):             # include/chimeralm_hip.h: struct clm_bucket_step
    _fields_ = [("kind", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("length", C.c_int32), ("offset", C.c_int64),
                ("stride", C.c_int64)]


class ClmExplainMutant(C.Structure):          # include/chimeralm_hip.h: struct clm_explain_mutant
    _fields_ = [("start", C.c_int32), ("sub", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/chimeralm_hip.h and include/chimeralm_feed.h declare: name -> (restype, argtypes)
_H = C.c_void_p
SYMBOLS = {
    "clm_abi_version": (C.c_int, []),
    "clm_default_config": (C.c_int, [C.POINTER(ClmConfig)]),
    "clm_create": (C.c_int, [C.POINTER(ClmConfig), C.c_int, C.POINTER(_H)]),
    "clm_load_weight": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "clm_finalize": (C.c_int, [_H]),
    "clm_reserve": (C.c_int, [_H, C.c_int, C.c_int]),
    "clm_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "clm_forward_attn": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(ClmAttnOut),
                                   C.c_void_p]),
    "clm_forward_staged_attn": (C.c_int, [_H, C.c_int, C.c_void_p, C.POINTER(ClmAttnOut), C.c_void_p]),
    "clm_forward_traj": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(ClmAttnOut),
                                   C.POINTER(ClmTrajOut), C.c_void_p]),
    "clm_forward_staged_traj": (C.c_int, [_H, C.c_int, C.c_void_p, C.POINTER(ClmAttnOut), C.POINTER(ClmTrajOut), C.c_void_p]),
    "clm_stage_ids": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "clm_forward_staged": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "clm_stage_wait": (C.c_int, [_H, C.c_int]),
    "clm_check": (C.c_int, [_H, C.c_void_p]),
    "clm_selfcheck": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                C.POINTER(C.c_int)]),
    "clm_logit_deviation": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float),
                                      C.POINTER(C.c_int)]),
    "clm_set_fallback": (C.c_int, [_H, C.c_int]),
    "clm_effective_precision": (C.c_int, [_H, C.c_int]),
    "clm_set_short_read_len": (C.c_int, [_H, C.c_int]),
    "clm_set_mlp_compensation": (C.c_int, [_H, C.c_int]),
    "clm_attention_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "clm_attention_exact_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "clm_attn_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "clm_attn_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p]),
    "clm_attn_train_backward": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p]),
    "clm_attn_train_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p]),
    "clm_hyena_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "clm_hyena_train_forward": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 4),
    "clm_hyena_train_backward": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 7),
    "clm_hyena_longtrain_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "clm_hyena_longtrain_forward": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 4),
    "clm_hyena_longtrain_backward": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 7),
    "clm_tf_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "clm_tf_load_weight": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "clm_tf_finalize": (C.c_int, [_H]),
    "clm_tf_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "clm_tf_selfcheck": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                   C.POINTER(C.c_int)]),
    "clm_tf_set_fallback": (C.c_int, [_H, C.c_int]),
    "clm_tf_effective_precision": (C.c_int, [_H]),
    "clm_tf_debug_fetch": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_size_t]),
    "clm_tf_debug_stop_after": (C.c_int, [_H, C.c_int]),
    "clm_tf_profile_enable": (C.c_int, [_H, C.c_int]),
    "clm_tf_profile_read": (C.c_int, [_H, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "clm_tf_last_error": (C.c_char_p, [_H]),
    "clm_tf_destroy": (C.c_int, [_H]),
    "clm_cnn_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_H)]),
    "clm_cnn_load_weight": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "clm_cnn_finalize": (C.c_int, [_H]),
    "clm_cnn_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "clm_cnn_debug_fetch": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_size_t]),
    "clm_cnn_last_error": (C.c_char_p, [_H]),
    "clm_cnn_destroy": (C.c_int, [_H]),
    "clm_cnn_train_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_H)]),
    "clm_cnn_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "clm_cnn_train_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clm_cnn_train_generation": (C.c_int64, [_H]),
    "clm_cnn_train_backward": (C.c_int, [_H, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_float, C.c_void_p]),
    "clm_cnn_train_debug_fetch": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_size_t]),
    "clm_cnn_train_last_error": (C.c_char_p, [_H]),
    "clm_cnn_train_destroy": (C.c_int, [_H]),
    "clm_mamba_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "clm_mamba_load_weight": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "clm_mamba_finalize": (C.c_int, [_H]),
    "clm_mamba_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p]),
    "clm_mamba_forward_traj": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.POINTER(ClmTrajOut), C.c_void_p]),
    "clm_mamba_debug_fetch": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_size_t]),
    "clm_mamba_last_error": (C.c_char_p, [_H]),
    "clm_mamba_destroy": (C.c_int, [_H]),
    "clm_mamba_train_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "clm_mamba_train_workspace_bytes": (C.c_int64, [C.c_int] * 5),
    "clm_mamba_train_forward": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_void_p] * 6),
    "clm_mamba_train_backward": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_void_p] * 6
                                 + [C.POINTER(C.c_void_p), C.c_void_p]),
    "clm_mamba_train_last_error": (C.c_char_p, [_H]),
    "clm_mamba_train_destroy": (C.c_int, [_H]),
    "clm_eval_create": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.POINTER(_H)]),
    "clm_eval_update": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "clm_eval_read": (C.c_int, [_H, C.POINTER(ClmEvalResult), C.c_void_p]),
    "clm_eval_merge": (C.c_int, [_H, C.POINTER(ClmEvalResult)]),
    "clm_eval_reset": (C.c_int, [_H, C.c_void_p]),
    "clm_eval_last_error": (C.c_char_p, [_H]),
    "clm_eval_destroy": (C.c_int, [_H]),
    "clm_explain_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "clm_explain_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "clm_explain_rows": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                   C.c_void_p]),
    "clm_explain_scores": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "clm_explain_reduce": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "clm_explain_last_error": (C.c_char_p, [_H]),
    "clm_explain_destroy": (C.c_int, [_H]),
    "clm_longread_lengths": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "clm_longread_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "clm_longread_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "clm_longread_rows": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int64, C.c_int, C.c_void_p]),
    "clm_longread_reduce": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clm_longread_last_error": (C.c_char_p, [_H]),
    "clm_longread_destroy": (C.c_int, [_H]),
    "clm_bucket_length": (C.c_int, [C.c_int, C.c_int]),
    "clm_bucket_pool_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "clm_bucket_plan_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_H)]),
    "clm_bucket_plan_push": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int]),
    "clm_bucket_plan_finish": (C.c_int, [_H]),
    "clm_bucket_plan_steps": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "clm_bucket_plan_last_error": (C.c_char_p, [_H]),
    "clm_bucket_plan_destroy": (C.c_int, [_H]),
    "clm_bucket_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "clm_bucket_scatter": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int64, C.c_void_p]),
    "clm_bucket_last_error": (C.c_char_p, [_H]),
    "clm_bucket_destroy": (C.c_int, [_H]),
    "clm_chunk_reads": (C.c_int, [_H, C.c_int]),
    "clm_rows": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "clm_rows_generation": (C.c_int64, [_H]),
    "clm_pool_forward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "clm_pool_backward": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_float, C.c_void_p]),
    "clm_debug_fetch": (C.c_int, [_H, C.c_char_p, C.c_void_p, C.c_size_t]),
    "clm_debug_stop_after": (C.c_int, [_H, C.c_int, C.c_int]),
    "clm_profile_enable": (C.c_int, [_H, C.c_int]),
    "clm_profile_read": (C.c_int, [_H, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "clm_profile_stage_name": (C.c_char_p, [C.c_int]),
    "clm_last_error": (C.c_char_p, [_H]),
    "clm_destroy": (C.c_int, [_H]),
    "clm_feeder_default_config": (C.c_int, [C.POINTER(ClmFeederConfig)]),
    "clm_feeder_open": (C.c_int, [C.c_char_p, C.POINTER(ClmFeederConfig), C.POINTER(_H)]),
    "clm_feeder_next": (C.c_int, [_H, C.POINTER(ClmFeedBatch)]),
    "clm_feeder_release": (C.c_int, [_H, C.c_int32]),
    "clm_feeder_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]),
    "clm_feeder_last_error": (C.c_char_p, [_H]),
    "clm_feeder_close": (C.c_int, [_H]),
    "clm_bam_filter": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int64, C.POINTER(C.c_int64),
                                 C.POINTER(C.c_int64)]),
    "clm_bam_filter_ex": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int64, C.c_int, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "clm_bam_sort_index": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "clm_bam_last_error": (C.c_char_p, []),
}



def upload_state_dict(items, load_weight, check) -> None:
    """Every `(key, tensor)` to an engine as contiguous fp32: `load_weight` is a `clm_*_load_weight` bound to its handle, `check` takes its code."""
    for k, t in items:
        t = t.detach().float().contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        check(load_weight(k.encode(), C.c_void_p(t.data_ptr()), DT_F32, shape, t.dim()))


_lib = None


def load() -> C.CDLL:
    """Load the engine library and bind every ABI symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: the ChimeraLM MI355X engine has no CPU or PyTorch fallback. "
            "Build it with `python -m chimeralm_amd.build` (needs hipcc, targets gfx950)."
        )
    # The process must hold ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64; if this library were opened first it
    # would pull in /opt/rocm's copy and device enumeration then fails in whichever runtime comes second
    # ("no such HIP device 0").  Importing torch first makes the dynamic loader resolve our dependency to the copy torch
    # has already mapped, whatever order the caller imports things in.
    import torch  # noqa: F401

    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild with `python -m chimeralm_amd.build --force`") from e
        fn.restype = res
        fn.argtypes = args
    if lib.clm_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.clm_abi_version()} != {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib
