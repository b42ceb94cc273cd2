"""ctypes binding of ``libripor_hip.so`` (C ABI in include/ripor_hip.h).

The product path has no CPU fallback: if the shared library is missing or no HIP device is
visible, every entry point raises (``RiporHipError``) instead of silently computing elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# RPR_DEV_LIB=1: the development build of the same sources (-DRPR_DEV_SWITCHES: the A/B switches of kernel routes and
# generations are live, csrc/common.h dev_getenv) — tools/ and the tests that compare kernel variants bit for bit. The
# product library reads none of those switches.
LIB_NAME = "libripor_hip_dev.so" if os.environ.get("RPR_DEV_LIB", "0") not in ("", "0") else "libripor_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

(K_GEMM, K_DEC_SELF_ATTN, K_DEC_CROSS_ATTN, K_ENC_ATTN, K_RMSNORM, K_SELECT, K_OTHER, K_GEMM_SMALL, K_TAIL_SELF_ATTN, K_FORK,
 K_COUNT) = range(11)
KERNEL_CLASS_NAMES = ["gemm", "dec_self_attn", "dec_cross_attn", "enc_attn", "rmsnorm", "select", "other", "gemm_small",
                      "tail_self_attn", "fork"]
STATUS_SATURATED, STATUS_EMPTY_QUERY, STATUS_TAIL_LEFTOVER, STATUS_SMALL_STREAM = 1, 2, 4, 8
# either one: the split-precision results since the last clear are not trustworthy and the call is repeated in exact fp32
STATUS_NEEDS_F32 = STATUS_SATURATED | STATUS_SMALL_STREAM
ABI_VERSION = 5

PREC_F32, PREC_F16X2, PREC_BF16 = 0, 1, 2
FLAG_LOG_SOFTMAX = 1
FLAG_NO_GRAPH = 2
# rpr_model_ext.ff_kind: wo(relu(wi x)) / wo(gelu_new(wi_0 x) * wi_1 x)
FF_RELU, FF_GATED_GELU = 0, 1


class RiporHipError(RuntimeError):
    pass


GRAD_BUCKET_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)
c_f32p = C.POINTER(C.c_float)
c_f32pp = C.POINTER(c_f32p)


class ModelDesc(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32), ("d_model", C.c_int32), ("d_kv", C.c_int32), ("d_ff", C.c_int32),
        ("num_heads", C.c_int32), ("num_layers", C.c_int32), ("num_decoder_layers", C.c_int32),
        ("rel_buckets", C.c_int32), ("rel_max_distance", C.c_int32), ("L", C.c_int32), ("V", C.c_int32),
        ("scaleup_output_hidden", C.c_int32), ("layer_norm_eps", C.c_float),
        ("shared", C.c_void_p), ("enc_rel_bias", C.c_void_p), ("dec_rel_bias", C.c_void_p),
        ("enc_final_ln", C.c_void_p), ("dec_final_ln", C.c_void_p), ("start_embed", C.c_void_p),
        ("in_embeds", C.c_void_p), ("out_embeds", C.c_void_p), ("dec_xkv", C.c_void_p),
        ("enc_ln0", C.POINTER(C.c_void_p)), ("enc_qkv", C.POINTER(C.c_void_p)), ("enc_o", C.POINTER(C.c_void_p)),
        ("enc_ln1", C.POINTER(C.c_void_p)), ("enc_wi", C.POINTER(C.c_void_p)), ("enc_wo", C.POINTER(C.c_void_p)),
        ("dec_ln0", C.POINTER(C.c_void_p)), ("dec_qkv", C.POINTER(C.c_void_p)), ("dec_o", C.POINTER(C.c_void_p)),
        ("dec_ln1", C.POINTER(C.c_void_p)), ("dec_xq", C.POINTER(C.c_void_p)), ("dec_xo", C.POINTER(C.c_void_p)),
        ("dec_ln2", C.POINTER(C.c_void_p)), ("dec_wi", C.POINTER(C.c_void_p)), ("dec_wo", C.POINTER(C.c_void_p)),
    ]


class ModelExt(C.Structure):
    """``rpr_model_ext``: what rpr_load_model_ext takes beside the (size-pinned) ModelDesc."""
    _fields_ = [("size", C.c_int32), ("ff_kind", C.c_int32)]


class DebugTaps(C.Structure):
    _fields_ = [("encoder_out", C.c_void_p), ("step_logits", C.c_void_p), ("step_scores", C.c_void_p),
                ("step_tokens", C.c_void_p), ("step_parent", C.c_void_p), ("step_valid", C.c_void_p)]


class KernelStats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("launches", C.c_int64), ("flops", C.c_double), ("bytes", C.c_double)]


class XencDesc(C.Structure):
    """``rpr_xenc_desc``: the cross-encoder's dimensions and device weight pointers (stacked per layer)."""
    _fields_ = ([(n, C.c_int32) for n in ("vocab_size", "hidden", "layers", "heads", "d_ff", "max_pos", "type_vocab")] +
                [("ln_eps", C.c_float)] +
                [(n, C.c_void_p) for n in ("word_emb", "pos_emb", "type_emb", "emb_ln_w", "emb_ln_b",
                                           "qkv_w", "qkv_b", "ao_w", "ao_b", "ln1_w", "ln1_b",
                                           "ff1_w", "ff1_b", "ff2_w", "ff2_b", "ln2_w", "ln2_b",
                                           "pool_w", "pool_b", "cls_w", "cls_b")])


def _op_struct(ptrs, i64s, i32s):
    return [(n, C.c_void_p) for n in ptrs] + [(n, C.c_int64) for n in i64s] + [(n, C.c_int32) for n in i32s]


class EncAttnOp(C.Structure):
    """``rpr_enc_attn_op`` (attention test hook; device pointers as integers)."""
    _fields_ = _op_struct(("qkv", "mask", "rel_bias", "offs", "lens", "out", "out_planes"), ("plane_stride",),
                          ("num_buckets", "max_distance", "Q", "Lq", "H", "dkv", "causal", "mfma"))


class DecSelfAttnOp(C.Structure):
    """``rpr_dec_self_attn_op``."""
    _fields_ = _op_struct(("q", "kcache", "vcache", "anc", "rel_bias", "nq_dev", "out", "out_planes"),
                          ("plane_stride", "q_stride", "h_stride", "pos_stride", "slot_stride"),
                          ("anc_ld", "num_buckets", "max_distance", "Q", "B", "H", "t", "dkv"))


class CrossAttnOp(C.Structure):
    """``rpr_cross_attn_op``."""
    _fields_ = _op_struct(("q", "xk", "xv", "mask", "offs", "nq_dev", "out", "out_planes"), ("plane_stride",),
                          ("site", "xld", "Q", "B", "H", "Lq", "dkv"))


class TailSelfAttnOp(C.Structure):
    """``rpr_tail_self_attn_op``."""
    _fields_ = _op_struct(("qkv", "kcache", "vcache", "anc", "flist", "kvq", "nseq_dev", "rel_bias", "out", "out_planes"),
                          ("plane_stride", "q_stride", "h_stride", "pos_stride", "slot_stride"),
                          ("anc_ld", "num_buckets", "max_distance", "nseq_cap", "B", "H", "T", "L", "dkv"))


class AttnDrop(C.Structure):
    """``rpr_attn_drop``: the dropout of the probabilities of a training attention hook (rate 0 = none)."""
    _fields_ = [("seed", C.c_uint64), ("step", C.c_uint64), ("rate", C.c_float), ("site", C.c_int32), ("L", C.c_int32)]


class TrainSelfAttnOp(C.Structure):
    """``rpr_train_self_attn_op`` (rpr_op_train_self_attn_bwd, rpr_op_train_self_attn_drop_fwd)."""
    _fields_ = ([(n, C.c_void_p) for n in ("qkv", "dO", "mask", "rel_bias", "dqkv", "dbias", "out")] + [("drop", AttnDrop)] +
                [(n, C.c_int32) for n in ("num_buckets", "max_distance", "S", "Ls", "H", "dkv", "causal")])


class TrainCrossAttnOp(C.Structure):
    """``rpr_train_cross_attn_op`` (rpr_op_train_cross_attn_bwd, rpr_op_train_cross_attn_drop_fwd)."""
    _fields_ = ([(n, C.c_void_p) for n in ("q", "dO", "xk", "xv", "mask", "dq", "dxk", "dxv", "out")] + [("drop", AttnDrop)] +
                [(n, C.c_int32) for n in ("xld", "bz", "n", "Lq", "H", "dkv")])


CROSS_SITE_BLOCK, CROSS_SITE_STEP, CROSS_SITE_TAIL = 0, 1, 2


class TrainRowsOp(C.Structure):
    """``rpr_train_rows_op`` (rpr_op_train_rows): one launcher of the training step's row-wise kernels."""
    _fields_ = [("src", C.c_void_p * 6), ("dst", C.c_void_p * 6), ("op", C.c_int32), ("dims", C.c_int32 * 11), ("f", C.c_float * 4)]


# RPR_TR_* of include/ripor_hip.h, in enum order
TRAIN_ROWS_OPS = {n: i for i, n in enumerate((
    "RMSNORM_BWD", "COLSUM_MULTI", "GOLD_SCORES", "GOLD_SCORE_BWD", "GOLD_ROWDOT", "MARGIN_MSE", "MARGIN_MSE_BWD", "DENSE_MSE_FWD",
    "DENSE_MSE_BWD", "RELU_BWD", "DEC_EMBED", "TRAIN_INDICES", "SCATTER_FIX", "FIX_FLUSH", "SUM_SELECTED", "S2S_HEAD_FWD",
    "S2S_HEAD_BWD", "ABSMAX2", "SPLIT_DYN", "SPLIT_DYN_T", "TO_BF16", "TO_BF16_T", "RMSNORM_BF16_T", "WEIGHTS_BF16", "TRANSPOSE_PAD"))}

# every symbol include/ripor_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "rpr_op_enc_attn": (C.c_int, [C.c_void_p, C.POINTER(EncAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_dec_self_attn": (C.c_int, [C.c_void_p, C.POINTER(DecSelfAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_cross_attn": (C.c_int, [C.c_void_p, C.POINTER(CrossAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_tail_self_attn": (C.c_int, [C.c_void_p, C.POINTER(TailSelfAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_train_self_attn_bwd": (C.c_int, [C.c_void_p, C.POINTER(TrainSelfAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_train_self_attn_drop_fwd": (C.c_int, [C.c_void_p, C.POINTER(TrainSelfAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_train_cross_attn_bwd": (C.c_int, [C.c_void_p, C.POINTER(TrainCrossAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_train_cross_attn_drop_fwd": (C.c_int, [C.c_void_p, C.POINTER(TrainCrossAttnOp), C.POINTER(C.c_int32), C.c_void_p]),
    "rpr_op_train_rows": (C.c_int, [C.c_void_p, C.POINTER(TrainRowsOp), C.c_void_p]),
    "rpr_attn_kernel_name": (C.c_char_p, [C.c_int]),
    "rpr_attn_kernel_count": (C.c_int, []),
    "rpr_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "rpr_free_ctx": (None, [C.c_void_p]),
    "rpr_last_error": (C.c_char_p, []),
    "rpr_abi_version": (C.c_int, []),
    "rpr_rel_bucket": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rpr_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "rpr_get_precision": (C.c_int, [C.c_void_p]),
    "rpr_load_model": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    "rpr_load_model_ext": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc), C.POINTER(ModelExt), C.POINTER(C.c_void_p)]),
    "rpr_free_model": (None, [C.c_void_p]),
    "rpr_op_gated_gelu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_op_gated_gelu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rpr_build_trie": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "rpr_free_trie": (None, [C.c_void_p]),
    "rpr_trie_num_rows": (C.c_int64, [C.c_void_p]),
    "rpr_trie_perm": (C.POINTER(C.c_int64), [C.c_void_p]),
    "rpr_trie_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rpr_trie_load": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "rpr_trie_build_file": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_char_p, C.c_int64, C.c_int64,
                                      C.c_int64, C.c_char_p]),
    "rpr_trie_file_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rpr_trie_file_validate": (C.c_int, [C.c_char_p]),
    "rpr_trie_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64)]),
    "rpr_trie_keys": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpr_trie_set_vocab": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_d2s_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rpr_d2s_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rpr_d2s_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_d2s_close": (None, [C.c_void_p]),
    "rpr_trie_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rpr_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                             C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(DebugTaps), C.c_void_p]),
    "rpr_search_margins": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(DebugTaps), C.c_void_p]),
    "rpr_search_prefixes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "rpr_lngknp_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "rpr_param_count": (C.c_int64, [C.c_void_p]),
    "rpr_param_total": (C.c_int64, [C.c_void_p]),
    "rpr_param_info": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rpr_lngknp_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_lngknp_backward_buckets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_seq2seq_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_seq2seq_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_seq2seq_backward_buckets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_dense_mse_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_dense_mse_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_dense_mse_backward_buckets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "rpr_set_train_dropout": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64]),
    "rpr_op_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_uint64,
                                 C.c_uint64, C.c_int32, C.c_void_p]),
    "rpr_get_status": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "rpr_status_words_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rpr_model_f32_only": (C.c_int, [C.c_void_p]),
    "rpr_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rpr_profile_reset": (C.c_int, [C.c_void_p]),
    "rpr_profile_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(KernelStats)]),
    "rpr_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "rpr_set_lane_split": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_lane_split": (C.c_int32, [C.c_void_p]),
    "rpr_set_l0_table": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_l0_table_bytes": (C.c_int64, [C.c_void_p, C.c_void_p]),
    "rpr_set_gemm_mfma16": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_gemm_mfma16": (C.c_int32, [C.c_void_p]),
    "rpr_set_forced_tail": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_forced_tail": (C.c_int32, [C.c_void_p]),
    "rpr_set_fork_depths": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "rpr_fork_depths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                  C.POINTER(C.c_int32)]),
    "rpr_trie_single_frac": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "rpr_trie_extra_mean": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "rpr_plan_forks": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rpr_set_tail_extras": (C.c_int, [C.c_void_p, C.c_int32]),
    "rpr_tail_extras": (C.c_int32, [C.c_void_p]),
    "rpr_last_fork_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rpr_op_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.c_void_p]),
    "rpr_op_linear_h2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_op_linear_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rpr_op_rmsnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                 C.c_void_p]),
    "rpr_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                             C.c_void_p]),
    "rpr_rq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "rpr_rq_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "rpr_rq_encode_beam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "rpr_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rpr_rq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rpr_flat_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rpr_xenc_load": (C.c_int, [C.c_void_p, C.POINTER(XencDesc), C.POINTER(C.c_void_p)]),
    "rpr_xenc_free": (None, [C.c_void_p]),
    "rpr_xenc_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                 C.c_void_p, C.c_void_p]),
    "rpr_xenc_set_precision": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rpr_xenc_get_precision": (C.c_int, [C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the library (once). Raises RiporHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RiporHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the search path.")
    # torch ships its own libamdhip64.so.7; the library must share that HIP runtime instance so
    # torch device pointers / streams are valid inside it. Importing torch first makes the
    # dynamic loader resolve our DT_NEEDED libamdhip64.so.7 to the copy torch already mapped.
    import torch  # noqa: F401
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        C.CDLL(hip_rt, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().rpr_last_error()
        raise RiporHipError(f"{what or 'libripor_hip'} failed (status {status}): "
                            f"{msg.decode('utf-8', 'replace') if msg else ''}")
