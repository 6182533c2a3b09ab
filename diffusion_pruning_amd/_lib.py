"""ctypes binding of libaptp_hip.so (C ABI declared in include/aptp_hip.h).

The library is the ONLY compute path of this package: there is no PyTorch/CPU fallback.  Loading fails loudly if
the shared object is missing (build it with ``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C diffusion_pruning_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# (APTP_LIB=<file> loads another build of the same ABI: A/B timing of kernel changes on one box)
LIB_PATH = os.environ.get("APTP_LIB") or os.path.join(_HERE, "csrc", "libaptp_hip.so")

ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU = 0, 1, 2, 3
ACT_QUICK_GELU = 5          # (4 is reserved: include/aptp_hip.h)
TILE_AUTO, TILE_128x128, TILE_128x160, TILE_64x128, TILE_64x160, TILE_128x64, TILE_64x64 = range(7)
(TILE_DMA_128x128, TILE_DMA_128x160, TILE_DMA_64x128, TILE_DMA_64x160, TILE_DMA_128x64, TILE_DMA_64x64) = range(7, 13)
(TILE_DMA3_128x128, TILE_DMA3_128x160, TILE_DMA3_64x128, TILE_DMA3_64x160, TILE_DMA3_128x64, TILE_DMA3_64x64) = range(13, 19)
# (past 18 only the ids host code names: launch_policy.py's lean set, the halo-in-LDS pair, the stream-K tiles it picks)
TILE_DMA4_64x128, TILE_DMA4_64x64, TILE_DMA4_128x64 = 24, 25, 26
TILE_HALO_128x160, TILE_HALO_128x128 = 43, 44
(TILE_DMA6_64x64, TILE_DMA8S_64x64, TILE_DMA6_64x128, TILE_DMA6_128x64, TILE_KU2S4_64x64, TILE_KU2S6_64x64, TILE_KU2S4_64x128,
 TILE_KU2S6_64x128, TILE_KU2S4_128x64) = range(45, 54)
TILE_SK_256x160, TILE_SK_256x128 = 64, 65


class ConvGemmParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64),
        ("B", c_int32), ("Hin", c_int32), ("Win", c_int32), ("Cin", c_int32),
        ("Hout", c_int32), ("Wout", c_int32),
        ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad", c_int32), ("ups", c_int32),
        ("w", c_void_p),
        ("N", c_int32), ("cin_pad", c_int32),
        ("bias", c_void_p),
        ("rowbias", c_void_p), ("ld_rowbias", c_int32),
        ("colgate", c_void_p), ("gate_group", c_int32), ("gate_B", c_int32),
        ("act", c_int32),
        ("corr", c_void_p), ("corr_B", c_int32),
        ("residual", c_void_p), ("ldres", c_int64),
        ("depth", c_void_p), ("depth_B", c_int32),
        ("depth_in", c_void_p), ("lddin", c_int64),
        ("y", c_void_p), ("ldy", c_int64),
        ("out_f32", c_int32), ("split_k", c_int32),
        ("workspace", c_void_p),
        ("tile", c_int32), ("order", c_int32),
        ("rowstat_out", c_void_p), ("rowstat_slots", c_int32),
        ("ln_stats", c_void_p), ("ln_slots", c_int32),
        ("ln_colsum", c_void_p), ("ln_eps", c_float), ("ln_C", c_int32),
        ("colstat_out", c_void_p), ("colstat_ld", c_int32),
        ("tile_counters", c_void_p),
        ("x2", c_void_p), ("ldx2", c_int64), ("Cin2", c_int32), ("cin2_pad", c_int32),
        ("prefetch", c_void_p), ("prefetch_bytes", c_int64),
        ("epilogue", c_int32),
        ("gn_gamma", c_void_p), ("gn_beta", c_void_p), ("gn_groups", c_int32), ("gn_C", c_int32), ("gn_silu", c_int32),
        ("gn_eps", c_float),
        ("io_f32", c_int32),
        ("ustat_out", c_void_p), ("ustat_unit", c_int32), ("ustat_units", c_int32), ("ustat_nrep", c_int32),
        ("pad_end", c_int32),
    ]


class GroupNormColStats(Structure):
    _fields_ = [("stats", c_void_p), ("ld", c_int32), ("rows_per_block", c_int32), ("C", c_int32),
                ("ustats", c_void_p), ("unit", c_int32), ("units", c_int32), ("nrep", c_int32)]


class GroupNormParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64),
        ("y", c_void_p), ("ldy", c_int64),
        ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("groups", c_int32),
        ("gamma", c_void_p), ("beta", c_void_p),
        ("eps", c_float), ("silu", c_int32),
        ("workspace", c_void_p), ("variant", c_int32),
        ("counters", c_void_p),
        ("colstats", GroupNormColStats * 2),
        ("io_f32", c_int32),
    ]


class LayerNormParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64),
        ("y", c_void_p), ("ldy", c_int64),
        ("rows", c_int32), ("C", c_int32),
        ("gamma", c_void_p), ("beta", c_void_p),
        ("eps", c_float),
        ("io_f32", c_int32),
    ]


class AttentionParams(Structure):
    _fields_ = [
        ("q", c_void_p), ("q_stride_b", c_int64), ("q_stride_l", c_int64),
        ("k", c_void_p), ("k_stride_b", c_int64), ("k_stride_l", c_int64),
        ("v", c_void_p), ("v_stride_b", c_int64), ("v_stride_l", c_int64),
        ("o", c_void_p), ("o_stride_b", c_int64), ("o_stride_l", c_int64),
        ("B", c_int32), ("heads", c_int32), ("Lq", c_int32), ("Lk", c_int32),
        ("scale", c_float),
        ("lse", c_void_p),
        ("variant", c_int32),
        ("io_f32", c_int32),
    ]


class GateBwdParams(Structure):
    _fields_ = [
        ("dy", c_void_p), ("lddy", c_int64), ("y0", c_void_p), ("ldy0", c_int64), ("dx", c_void_p), ("lddx", c_int64),
        ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("groups", c_int32),
        ("gate", c_void_p), ("gate_B", c_int32),
        ("dgate_partial", c_void_p),
        ("dgate", c_void_p),
    ]


class GegluParams(Structure):
    _fields_ = [
        ("hg", c_void_p), ("ldhg", c_int64), ("out", c_void_p), ("ldout", c_int64),
        ("dout", c_void_p), ("lddout", c_int64), ("dhg", c_void_p), ("lddhg", c_int64),
        ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("groups", c_int32),
        ("gate", c_void_p), ("gate_B", c_int32),
        ("dgate_partial", c_void_p),
        ("backward", c_int32),
        ("dgate", c_void_p),
    ]


class FfTailParams(Structure):
    _fields_ = [
        ("h", c_void_p), ("ldh", c_int64), ("x", c_void_p), ("ldx", c_int64), ("y", c_void_p), ("ldy", c_int64),
        ("w1", c_void_p), ("b1", c_void_p), ("cs1", c_void_p), ("n1", c_int32), ("ld1", c_int32),
        ("w2", c_void_p), ("b2", c_void_p), ("ld2", c_int32),
        ("w3", c_void_p), ("b3", c_void_p), ("ld3", c_int32),
        ("colstat", c_void_p), ("colstat_ld", c_int32),
        ("M", c_int32), ("C", c_int32),
        ("eps", c_float),
    ]


class WgradParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("dy", c_void_p), ("lddy", c_int64), ("dw", c_void_p),
        ("B", c_int32), ("H", c_int32), ("W", c_int32), ("C", c_int32), ("N", c_int32), ("KH", c_int32), ("KW", c_int32),
        ("split_m", c_int32), ("ld_dw", c_int32), ("db", c_void_p), ("slab_stride", c_int64), ("db_stride", c_int64),
        ("stride", c_int32), ("ups", c_int32),
    ]


class FoldRowsParams(Structure):
    _fields_ = [("partials", c_void_p), ("out", c_void_p), ("R", c_int32), ("n_rows", c_int32), ("C", c_int32), ("ld_out", c_int32),
                ("tail_out", c_void_p), ("tail_rows", c_int32), ("pair_split", c_int32), ("tail_n", c_int32)]


class PackDgradParams(Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("N", c_int32), ("C", c_int32), ("taps", c_int32), ("src_ld", c_int32),
                ("dst_ld", c_int32), ("dst_rows", c_int32)]


class DepthLerpParams(Structure):
    _fields_ = [
        ("x_in", c_void_p), ("ld_in", c_int64), ("x_out", c_void_p), ("ld_out", c_int64), ("y", c_void_p), ("ld_y", c_int64),
        ("dy", c_void_p), ("ld_dy", c_int64), ("d_in", c_void_p), ("ld_d_in", c_int64), ("d_out", c_void_p), ("ld_d_out", c_int64),
        ("B", c_int32), ("HW", c_int32), ("C", c_int32),
        ("d", c_void_p), ("d_B", c_int32),
        ("dd_partial", c_void_p),
        ("dd", c_void_p),
        ("backward", c_int32),
    ]


class AdamWItem(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("shadow", c_void_p), ("n", c_int64)]


class AdamWParams(Structure):
    _fields_ = [("items_dev", c_void_p), ("starts_dev", c_void_p), ("n_items", c_int32), ("total_blocks", c_int32),
                ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("step_dev", c_void_p), ("gate_dev", c_void_p), ("grad_scale", c_float), ("warmup_steps", c_float)]


class AdamW8Item(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m8", c_void_p), ("v8", c_void_p), ("absmax_m", c_void_p), ("absmax_v", c_void_p),
                ("shadow", c_void_p), ("n", c_int64)]


class AdamW8Params(Structure):
    _fields_ = AdamWParams._fields_ + [("qmap_signed_dev", c_void_p), ("qmap_unsigned_dev", c_void_p), ("items_host", c_void_p)]


class GroupAdamWItem(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("step", c_void_p), ("n", c_int64),
                ("group", c_int32)]


class AdamWGroup(Structure):
    _fields_ = [("lr", c_float), ("weight_decay", c_float), ("warmup_steps", c_float)]


class GroupAdamWParams(Structure):
    _fields_ = [("items_dev", c_void_p), ("starts_dev", c_void_p), ("n_items", c_int32), ("total_blocks", c_int32),
                ("groups_dev", c_void_p), ("n_groups", c_int32), ("counters_dev", c_void_p),
                ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("grad_scale", c_float), ("zero_grad", c_int32),
                ("gate_dev", c_void_p), ("items_host", c_void_p), ("grad_scale_dev", c_void_p)]


# kinds of aptp_lr_schedule, by the names of the recipes' `lr_scheduler` (transformers.optimization.SchedulerType)
LR_KINDS = {"constant": 0, "constant_with_warmup": 1, "linear": 2, "cosine": 3, "cosine_with_restarts": 4, "polynomial": 5}


class LrScheduleParams(Structure):
    _fields_ = [("kind", c_int32), ("warmup_steps", c_int32), ("training_steps", c_int32), ("n", c_int32),
                ("num_cycles", ctypes.c_double), ("power", ctypes.c_double), ("lr_end", ctypes.c_double), ("lr_init", ctypes.c_double),
                ("count_dev", c_void_p), ("base_dev", c_void_p), ("out_dev", c_void_p), ("out_stride", c_int32),
                ("mult_dev", c_void_p)]


class GradNormItem(Structure):
    _fields_ = [("g", c_void_p), ("n", c_int64)]


class GradNormParams(Structure):
    _fields_ = [("items_dev", c_void_p), ("starts_dev", c_void_p), ("n_items", c_int32), ("total_blocks", c_int32),
                ("partials_dev", c_void_p), ("grad_scale", c_float), ("max_norm_dev", c_void_p), ("gate_dev", c_void_p),
                ("out_dev", c_void_p)]


EMA_UPDATE, EMA_SWAP = 0, 1


class EmaItem(Structure):
    _fields_ = [("p", c_void_p), ("ema", c_void_p), ("shadow", c_void_p), ("n", c_int64)]


class EmaParams(Structure):
    _fields_ = [("items_dev", c_void_p), ("starts_dev", c_void_p), ("n_items", c_int32), ("total_blocks", c_int32),
                ("mode", c_int32), ("count_dev", c_void_p), ("gate_dev", c_void_p),
                ("decay", c_float), ("min_decay", c_float), ("update_after_step", c_int32), ("use_warmup", c_int32),
                ("inv_gamma", c_float), ("power", c_float), ("cur_decay_dev", c_void_p)]


GRAD_ACCUM_STORE, GRAD_ACCUM_ADD, GRAD_ACCUM_FINAL = 0, 1, 2


class GradAccumParams(Structure):
    _fields_ = [("acc", c_void_p), ("g", c_void_p), ("n", c_int64), ("mode", c_int32)]


class MseParams(Structure):
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64), ("b", c_void_p), ("ldb", c_int64),
        ("rows", c_int64), ("C", c_int32), ("f32", c_int32),
        ("partial", c_void_p), ("out", c_void_p),
        ("g", c_void_p), ("da", c_void_p), ("ldda", c_int64),
        ("backward", c_int32),
    ]


LOSS_TERMS_MAX = 16


class LossTerm(Structure):
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64), ("b", c_void_p), ("ldb", c_int64),
        ("rows", c_int64), ("rows_per_sample", c_int64),
        ("C", c_int32), ("a_f32", c_int32), ("b_f32", c_int32), ("group", c_int32),
        ("scale", c_float), ("reserved", c_int32),
    ]


class LossTermsParams(Structure):
    _fields_ = [
        ("terms", LossTerm * LOSS_TERMS_MAX),
        ("n_terms", c_int32), ("n_groups", c_int32),
        ("group_coef", c_float * LOSS_TERMS_MAX), ("group_div", c_float * LOSS_TERMS_MAX),
        ("w", c_void_p),
        ("partial", c_void_p), ("out", c_void_p), ("sample_out", c_void_p), ("running", c_void_p),
    ]


class LossStageTerm(Structure):
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64), ("b", c_void_p), ("ldb", c_int64),
        ("rows", c_int64), ("rows_per_sample", c_int64),
        ("C", c_int32), ("a_f32", c_int32), ("b_f32", c_int32), ("group", c_int32),
        ("scale", c_float), ("weighted", c_int32),
    ]


class LossStageGrad(Structure):
    _fields_ = [("grad_out", c_void_p), ("ldg", c_int64), ("term0", c_int32), ("term1", c_int32)]


LOSS_STAGE_MAX_B = 1024


class LossStageParams(Structure):
    _fields_ = [
        ("terms", LossStageTerm * LOSS_TERMS_MAX),
        ("n_terms", c_int32), ("n_groups", c_int32),
        ("group_coef", c_float * LOSS_TERMS_MAX), ("group_div", c_float * LOSS_TERMS_MAX),
        ("valid", c_void_p), ("w", c_void_p),
        ("partial", c_void_p), ("out", c_void_p), ("sample_out", c_void_p),
        ("grads", LossStageGrad * LOSS_TERMS_MAX),
        ("n_grads", c_int32), ("reserved", c_int32),
        ("g", c_void_p),
    ]


ROUTER_STAGE_MAX_B, ROUTER_STAGE_MAX_FEATURES, SINKHORN_MAX_K = 1024, 4096, 64
RESOURCE_TYPES = {"log": 0, "mae": 1, "mse": 2}


class SinkhornParams(Structure):
    _fields_ = [
        ("scores", c_void_p), ("ld", c_int64),
        ("valid", c_void_p), ("idx", c_void_p), ("q", c_void_p),
        ("B", c_int32), ("K", c_int32), ("iters", c_int32),
        ("eps", c_float),
    ]


class RouterStageParams(Structure):
    _fields_ = [
        ("text", c_void_p), ("ld_text", c_int64), ("arch", c_void_p), ("ld_arch", c_int64),
        ("ratios", c_void_p), ("valid", c_void_p), ("g", c_void_p),
        ("work", c_void_p), ("out", c_void_p),
        ("d_arch", c_void_p), ("ld_darch", c_int64), ("d_ratios", c_void_p),
        ("B", c_int32), ("E", c_int32), ("D", c_int32), ("resource_type", c_int32),
        ("tau_arch", c_float), ("tau_text", c_float), ("p", c_double),
        ("w_resource", c_float), ("w_contrastive", c_float), ("w_std", c_float), ("w_max", c_float),
    ]


GUMBEL_RELAX_MAX_R, GUMBEL_RELAX_MAX_E, GUMBEL_RELAX_MAX_SEG, GUMBEL_RELAX_MAX_ND = 65535, 4096, 1024, 64
ROUTER_ASSIGN_SUBDRAW, ROUTER_RELAX_SUBDRAW = 6, 7          # csrc/gumbel_relax.h: APTP_TN_ROUTER_ASSIGN / _RELAX


class GumbelRelaxParams(Structure):
    _fields_ = [
        ("z", c_void_p), ("out", c_void_p), ("dout", c_void_p), ("dz", c_void_p),
        ("seeds", c_void_p), ("draw", c_void_p),
        ("seg_start", c_void_p), ("depth_order", c_void_p),
        ("seg_start_host", c_void_p), ("depth_order_host", c_void_p),
        ("R", c_int32), ("nw", c_int32), ("nd", c_int32), ("n_seg", c_int32),
        ("sub", c_int32), ("codebook", c_int32), ("non_zero_width", c_int32), ("reserved", c_int32),
        ("T", c_float), ("base", c_float),
    ]


class PhiloxGumbelParams(Structure):
    _fields_ = [
        ("out", c_void_p), ("words", c_void_p), ("seeds", c_void_p), ("draw", c_void_p),
        ("n", c_int64), ("offset", c_int64),
        ("R", c_int32), ("sub", c_int32), ("codebook", c_int32), ("reserved", c_int32),
    ]


class GroupNormBwdParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("dy", c_void_p), ("lddy", c_int64), ("dx", c_void_p), ("lddx", c_int64),
        ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("groups", c_int32),
        ("gamma", c_void_p), ("beta", c_void_p),
        ("eps", c_float), ("silu", c_int32),
        ("fwd_stats", c_void_p),
        ("workspace", c_void_p),
        ("pgrad_partial", c_void_p),
        ("add", c_void_p), ("ldadd", c_int64),
    ]


class UnetPrologueParams(Structure):
    _fields_ = [
        ("sample", c_void_p), ("sample_bf16", c_int32), ("x", c_void_p),
        ("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32), ("cin_pad", c_int32),
        ("timesteps", c_void_p), ("freqs", c_void_p), ("half", c_int32), ("t_emb", c_void_p),
    ]


class UnetEpilogueParams(Structure):
    _fields_ = [
        ("y", c_void_p), ("ldy", c_int64), ("out", c_void_p), ("out_bf16", c_int32),
        ("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32),
    ]


class AttentionWideParams(Structure):
    _fields_ = [
        ("q", c_void_p), ("q_stride_b", c_int64), ("q_stride_l", c_int64),
        ("k", c_void_p), ("k_stride_b", c_int64), ("k_stride_l", c_int64),
        ("v", c_void_p), ("v_stride_b", c_int64), ("v_stride_l", c_int64),
        ("o", c_void_p), ("o_stride_b", c_int64), ("o_stride_l", c_int64),
        ("B", c_int32), ("Lq", c_int32), ("Lk", c_int32),
        ("scale", c_float),
        ("io_f32", c_int32),
    ]


class ImageOutParams(Structure):
    _fields_ = [
        ("y", c_void_p), ("ldy", c_int64), ("out", c_void_p), ("out_u8", c_int32),
        ("B", c_int32), ("H", c_int32), ("W", c_int32),
    ]


class ImageInParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("x_bf16", c_int32), ("out", c_void_p), ("out_f32", c_int32),
        ("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32),
    ]


class LatentDistParams(Structure):
    _fields_ = [
        ("y", c_void_p), ("ldy", c_int64), ("wq", c_void_p), ("bq", c_void_p), ("moments", c_void_p), ("eps", c_void_p),
        ("latents", c_void_p), ("latents_bf16", c_int32), ("scale", c_float),
        ("B", c_int32), ("H", c_int32), ("W", c_int32),
    ]


class AttentionCausalParams(Structure):
    _fields_ = [
        ("q", c_void_p), ("q_stride_b", c_int64), ("q_stride_l", c_int64),
        ("k", c_void_p), ("k_stride_b", c_int64), ("k_stride_l", c_int64),
        ("v", c_void_p), ("v_stride_b", c_int64), ("v_stride_l", c_int64),
        ("o", c_void_p), ("o_stride_b", c_int64), ("o_stride_l", c_int64),
        ("B", c_int32), ("heads", c_int32), ("L", c_int32),
        ("scale", c_float),
        ("io_f32", c_int32),
    ]


class TokenEmbedParams(Structure):
    _fields_ = [
        ("ids", c_void_p), ("tok", c_void_p), ("pos", c_void_p), ("out", c_void_p), ("ldo", c_int64),
        ("B", c_int32), ("L", c_int32), ("C", c_int32), ("vocab", c_int32), ("out_f32", c_int32), ("pos_rows", c_int32),
    ]


class AttentionBiasParams(Structure):
    _fields_ = [
        ("q", c_void_p), ("q_stride_b", c_int64), ("q_stride_l", c_int64),
        ("k", c_void_p), ("k_stride_b", c_int64), ("k_stride_l", c_int64),
        ("v", c_void_p), ("v_stride_b", c_int64), ("v_stride_l", c_int64),
        ("o", c_void_p), ("o_stride_b", c_int64), ("o_stride_l", c_int64),
        ("relbias", c_void_p), ("key_mask", c_void_p),
        ("B", c_int32), ("heads", c_int32), ("L", c_int32),
        ("scale", c_float),
        ("io_f32", c_int32),
    ]


class EmbedLnParams(Structure):
    _fields_ = [
        ("ids", c_void_p), ("word", c_void_p), ("pos", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
        ("out", c_void_p), ("ldo", c_int64),
        ("B", c_int32), ("L", c_int32), ("C", c_int32), ("vocab", c_int32), ("pos_rows", c_int32), ("pad_id", c_int32),
        ("out_f32", c_int32), ("eps", c_float),
    ]


class MaskedMeanParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("x_stride_b", c_int64), ("x_stride_l", c_int64), ("mask", c_void_p), ("out", c_void_p),
        ("B", c_int32), ("L", c_int32), ("C", c_int32), ("x_f32", c_int32),
    ]


class ColsumParams(Structure):
    _fields_ = [("x", c_void_p), ("ldx", c_int64), ("rows", c_int32), ("C", c_int32), ("partial", c_void_p), ("batch", c_int32)]


class LayerNormPgradParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("dy", c_void_p), ("lddy", c_int64),
        ("rows", c_int32), ("C", c_int32), ("eps", c_float), ("partial", c_void_p),
    ]


class LayerNormBwdParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("dy", c_void_p), ("lddy", c_int64), ("dx", c_void_p), ("lddx", c_int64),
        ("rows", c_int32), ("C", c_int32),
        ("gamma", c_void_p),
        ("eps", c_float),
        ("add", c_void_p), ("ldadd", c_int64),
    ]


class AttentionBwdParams(Structure):
    _fields_ = [
        ("q", c_void_p), ("q_stride_b", c_int64), ("q_stride_l", c_int64),
        ("k", c_void_p), ("k_stride_b", c_int64), ("k_stride_l", c_int64),
        ("v", c_void_p), ("v_stride_b", c_int64), ("v_stride_l", c_int64),
        ("o", c_void_p), ("o_stride_b", c_int64), ("o_stride_l", c_int64),
        ("dout", c_void_p), ("dout_stride_b", c_int64), ("dout_stride_l", c_int64),
        ("dq", c_void_p), ("dq_stride_b", c_int64), ("dq_stride_l", c_int64),
        ("dk", c_void_p), ("dk_stride_b", c_int64), ("dk_stride_l", c_int64),
        ("dv", c_void_p), ("dv_stride_b", c_int64), ("dv_stride_l", c_int64),
        ("lse", c_void_p), ("delta", c_void_p),
        ("B", c_int32), ("heads", c_int32), ("Lq", c_int32), ("Lk", c_int32),
        ("scale", c_float), ("q_split", c_int32), ("workspace", c_void_p),
    ]


class ImagePatchesParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("nchw", c_int32),
        ("B", c_int32), ("H", c_int32), ("W", c_int32),
        ("S", c_int32), ("P", c_int32),
        ("resize", c_int32),
        ("mean", c_float * 3), ("std", c_float * 3),
        ("out", c_void_p), ("ldo", c_int64),
        ("out_f32", c_int32),
    ]


class VitEmbedLnParams(Structure):
    _fields_ = [
        ("patches", c_void_p), ("ldp", c_int64),
        ("cls", c_void_p), ("pos", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
        ("out", c_void_p), ("ldo", c_int64),
        ("B", c_int32), ("T", c_int32), ("C", c_int32),
        ("out_f32", c_int32),
        ("eps", c_float),
    ]


class L2NormalizeParams(Structure):
    _fields_ = [("x", c_void_p), ("ldx", c_int64), ("out", c_void_p), ("ldo", c_int64), ("n", c_int32), ("D", c_int32)]


class MmdRbfParams(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64),
        ("y", c_void_p), ("ldy", c_int64),
        ("n", c_int32), ("m", c_int32), ("D", c_int32),
        ("sigma", c_float), ("scale", c_float),
        ("workspace", c_void_p),
        ("out", c_void_p),
    ]


class ImagePatchesPilParams(Structure):
    _fields_ = [
        ("x", c_void_p),
        ("B", c_int32), ("H", c_int32), ("W", c_int32),
        ("S", c_int32), ("P", c_int32),
        ("xbounds", c_void_p), ("xweights", c_void_p), ("xk", c_int32),
        ("ybounds", c_void_p), ("yweights", c_void_p), ("yk", c_int32),
        ("scratch", c_void_p),
        ("mean", c_float * 3), ("std", c_float * 3),
        ("out", c_void_p), ("ldo", c_int64),
        ("out_f32", c_int32),
    ]


EOS_ARGMAX, EOS_FIRST = 0, 1


class EosPoolLnParams(Structure):
    _fields_ = [
        ("ids", c_void_p),
        ("x", c_void_p), ("x_stride_b", c_int64), ("x_stride_l", c_int64),
        ("gamma", c_void_p), ("beta", c_void_p),
        ("out", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_int64),
        ("index_out", c_void_p),
        ("B", c_int32), ("L", c_int32), ("C", c_int32),
        ("eos_mode", c_int32), ("eos_token_id", c_int32),
        ("x_f32", c_int32), ("act_f32", c_int32),
        ("eps", c_float),
    ]


class PairedCosineParams(Structure):
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64),
        ("b", c_void_p), ("ldb", c_int64),
        ("cos_out", c_void_p),
        ("sum_out", c_void_p),
        ("n", c_int32), ("D", c_int32),
        ("accumulate", c_int32),
    ]


TRAIN_NO_TABLE = -1


class TrainImageDesc(Structure):
    _fields_ = [
        ("src_off", c_int64),
        ("scratch_off", c_int64),
        ("xtab_off", c_int64), ("ytab_off", c_int64),
        ("H", c_int32), ("W", c_int32),
        ("H1", c_int32), ("W1", c_int32),
        ("top", c_int32), ("left", c_int32), ("flip", c_int32),
        ("xk", c_int32), ("yk", c_int32),
        ("row0", c_int32), ("nrows", c_int32),
        ("reserved", c_int32),
    ]


class TrainImagesParams(Structure):
    _fields_ = [
        ("images", c_void_p), ("images_bytes", c_int64),
        ("desc", c_void_p),
        ("desc_dev", c_void_p),
        ("tables", c_void_p), ("tables_count", c_int64),
        ("scratch", c_void_p), ("scratch_bytes", c_int64),
        ("out", c_void_p),
        ("B", c_int32), ("R", c_int32),
        ("out_f32", c_int32),
    ]


STEP_NOISE_BF16, STEP_NOISE_F32 = 0, 1
STEP_DDIM, STEP_PNDM, STEP_DPMPP = 0, 1, 2
STEP_EPSILON, STEP_V_PREDICTION = 0, 1


class GuidedStepParams(Structure):
    _fields_ = [
        ("noise", c_void_p),
        ("sample", c_void_p),
        ("out", c_void_p),
        ("coef", c_void_p),
        ("slot", c_void_p),
        ("w", c_void_p),
        ("flags", c_void_p),
        ("E", c_void_p),
        ("saved", c_void_p),
        ("n", c_int64),
        ("b", c_int32), ("noise_rows", c_int32),
        ("noise_dtype", c_int32), ("scheduler", c_int32), ("prediction", c_int32), ("do_cfg", c_int32),
        ("guidance_scale", c_float), ("guidance_rescale", c_float),
    ]


PHILOX_F32, PHILOX_BF16, PHILOX_RAW = 0, 1, 2


class PhiloxNormalParams(Structure):
    _fields_ = [
        ("out", c_void_p),
        ("base", c_void_p),
        ("seeds_dev", c_void_p),
        ("draw_dev", c_void_p),
        ("scale_dev", c_void_p),
        ("n", c_int64), ("offset", c_int64), ("draw", c_int64),
        ("b", c_int32), ("out_kind", c_int32),
        ("scale", c_float),
    ]


TRAIN_NOISE_EPSILON, TRAIN_NOISE_V_PREDICTION = 0, 1


class TrainNoiseParams(Structure):
    _fields_ = [
        ("moments", c_void_p),
        ("latents_in", c_void_p),
        ("sqrt_table", c_void_p),
        ("seeds_dev", c_void_p),
        ("draw_dev", c_void_p),
        ("noisy", c_void_p),
        ("target", c_void_p),
        ("timesteps", c_void_p),
        ("latents_out", c_void_p),
        ("noise_out", c_void_p),
        ("draw", c_int64),
        ("B", c_int32), ("h", c_int32), ("w", c_int32), ("T", c_int32),
        ("prediction", c_int32),
        ("scale", c_float), ("noise_offset", c_float), ("input_perturbation", c_float),
    ]


# every symbol include/aptp_hip.h declares: (name, restype, argtypes)
EXPORTS = [
    ("aptp_conv_gemm", c_int, [POINTER(ConvGemmParams), c_void_p]),
    ("aptp_conv_gemm_workspace_bytes", c_int64, [POINTER(ConvGemmParams)]),
    ("aptp_conv_gemm_suggest_split_k", c_int, [POINTER(ConvGemmParams)]),
    ("aptp_conv_gemm_rowstat_slots", c_int, [POINTER(ConvGemmParams)]),
    ("aptp_conv_gemm_tiles", c_int, [POINTER(ConvGemmParams)]),
    ("aptp_conv_gemm_colstat_rows", c_int, [POINTER(ConvGemmParams)]),
    ("aptp_groupnorm", c_int, [POINTER(GroupNormParams), c_void_p]),
    ("aptp_groupnorm_nchunk", c_int, [c_int]),
    ("aptp_rows_nchunk", c_int, [c_int]),
    ("aptp_groupnorm_workspace_bytes", c_int64, [POINTER(GroupNormParams)]),
    ("aptp_layernorm", c_int, [POINTER(LayerNormParams), c_void_p]),
    ("aptp_attention", c_int, [POINTER(AttentionParams), c_void_p]),
    ("aptp_gate_bwd", c_int, [POINTER(GateBwdParams), c_void_p]),
    ("aptp_geglu", c_int, [POINTER(GegluParams), c_void_p]),
    ("aptp_depth_lerp", c_int, [POINTER(DepthLerpParams), c_void_p]),
    ("aptp_ff_tail_supported", c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    ("aptp_ff_tail", c_int, [POINTER(FfTailParams), c_void_p]),
    ("aptp_conv_wgrad_supported", c_int, [POINTER(WgradParams)]),
    ("aptp_conv_wgrad_suggest_split", c_int, [POINTER(WgradParams)]),
    ("aptp_conv_wgrad", c_int, [POINTER(WgradParams), c_void_p]),
    ("aptp_conv_wgrad_many_item_bytes", ctypes.c_int64, []),
    ("aptp_conv_wgrad_many_blocks", c_int, [POINTER(WgradParams)]),
    ("aptp_conv_wgrad_many_fill", c_int, [POINTER(WgradParams), c_void_p, ctypes.c_int32]),
    ("aptp_conv_wgrad_many", c_int, [c_void_p, c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_void_p]),
    ("aptp_fold_rows", c_int, [POINTER(FoldRowsParams), c_void_p]),
    ("aptp_pack_dgrad", c_int, [POINTER(PackDgradParams), c_void_p]),
    ("aptp_fold_rows_blocks", c_int, [POINTER(FoldRowsParams)]),
    ("aptp_fold_rows_many", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("aptp_pack_dgrad_blocks", c_int, [POINTER(PackDgradParams)]),
    ("aptp_pack_dgrad_many", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("aptp_adamw_blocks", c_int, [c_int64]),
    ("aptp_adamw_many", c_int, [POINTER(AdamWParams), c_void_p]),
    ("aptp_adamw_many_scaled", c_int, [POINTER(AdamWParams), c_void_p, c_void_p]),
    ("aptp_adamw_many_lr", c_int, [POINTER(AdamWParams), c_void_p, c_void_p, c_void_p]),
    ("aptp_adamw8_blocks", c_int, [c_int64]),
    ("aptp_adamw8_many", c_int, [POINTER(AdamW8Params), c_void_p, c_void_p]),
    ("aptp_adamw8_many_lr", c_int, [POINTER(AdamW8Params), c_void_p, c_void_p, c_void_p]),
    ("aptp_lr_schedule", c_int, [POINTER(LrScheduleParams), c_void_p]),
    ("aptp_ema_many", c_int, [POINTER(EmaParams), c_void_p]),
    ("aptp_group_adamw_blocks", c_int, [c_int64]),
    ("aptp_group_adamw", c_int, [POINTER(GroupAdamWParams), c_void_p]),
    ("aptp_grad_norm_blocks", c_int, [c_int64]),
    ("aptp_grad_norm", c_int, [POINTER(GradNormParams), c_void_p]),
    ("aptp_grad_accumulate_blocks", c_int, [c_int64]),
    ("aptp_grad_accumulate", c_int, [POINTER(GradAccumParams), c_void_p]),
    ("aptp_mse_nblocks", c_int, [c_int64, c_int32]),
    ("aptp_mse", c_int, [POINTER(MseParams), c_void_p]),
    ("aptp_loss_terms_nblocks", c_int, [POINTER(LossTermsParams)]),
    ("aptp_loss_terms_scratch_floats", c_int, [POINTER(LossTermsParams)]),
    ("aptp_loss_terms", c_int, [POINTER(LossTermsParams), c_void_p]),
    ("aptp_loss_stage_nblocks", c_int, [POINTER(LossStageParams)]),
    ("aptp_loss_stage_scratch_floats", c_int, [POINTER(LossStageParams)]),
    ("aptp_loss_stage", c_int, [POINTER(LossStageParams), c_void_p]),
    ("aptp_loss_stage_bwd_nblocks", c_int, [POINTER(LossStageParams)]),
    ("aptp_loss_stage_bwd", c_int, [POINTER(LossStageParams), c_void_p]),
    ("aptp_sinkhorn_assign", c_int, [POINTER(SinkhornParams), c_void_p]),
    ("aptp_router_stage_work_floats", c_int64, [c_int32, c_int32, c_int32]),
    ("aptp_router_stage", c_int, [POINTER(RouterStageParams), c_void_p]),
    ("aptp_router_stage_bwd", c_int, [POINTER(RouterStageParams), c_void_p]),
    ("aptp_gumbel_relax", c_int, [POINTER(GumbelRelaxParams), c_void_p]),
    ("aptp_gumbel_relax_bwd", c_int, [POINTER(GumbelRelaxParams), c_void_p]),
    ("aptp_philox_gumbel", c_int, [POINTER(PhiloxGumbelParams), c_void_p]),
    ("aptp_groupnorm_bwd", c_int, [POINTER(GroupNormBwdParams), c_void_p]),
    ("aptp_layernorm_bwd", c_int, [POINTER(LayerNormBwdParams), c_void_p]),
    ("aptp_attention_bwd", c_int, [POINTER(AttentionBwdParams), c_void_p]),
    ("aptp_attention_bwd_q_split", c_int, [POINTER(AttentionBwdParams)]),
    ("aptp_attention_bwd_workspace_bytes", c_size_t, [POINTER(AttentionBwdParams), c_int32]),
    ("aptp_colsum", c_int, [POINTER(ColsumParams), c_void_p]),
    ("aptp_layernorm_pgrad", c_int, [POINTER(LayerNormPgradParams), c_void_p]),
    ("aptp_unet_prologue", c_int, [POINTER(UnetPrologueParams), c_void_p]),
    ("aptp_unet_epilogue", c_int, [POINTER(UnetEpilogueParams), c_void_p]),
    ("aptp_attention_wide", c_int, [POINTER(AttentionWideParams), c_void_p]),
    ("aptp_image_out", c_int, [POINTER(ImageOutParams), c_void_p]),
    ("aptp_image_in", c_int, [POINTER(ImageInParams), c_void_p]),
    ("aptp_latent_dist", c_int, [POINTER(LatentDistParams), c_void_p]),
    ("aptp_attention_causal", c_int, [POINTER(AttentionCausalParams), c_void_p]),
    ("aptp_token_embed", c_int, [POINTER(TokenEmbedParams), c_void_p]),
    ("aptp_attention_bias", c_int, [POINTER(AttentionBiasParams), c_void_p]),
    ("aptp_embed_ln", c_int, [POINTER(EmbedLnParams), c_void_p]),
    ("aptp_masked_mean", c_int, [POINTER(MaskedMeanParams), c_void_p]),
    ("aptp_image_patches", c_int, [POINTER(ImagePatchesParams), c_void_p]),
    ("aptp_vit_embed_ln", c_int, [POINTER(VitEmbedLnParams), c_void_p]),
    ("aptp_l2_normalize", c_int, [POINTER(L2NormalizeParams), c_void_p]),
    ("aptp_mmd_rbf_workspace_bytes", c_int64, [c_int32, c_int32]),
    ("aptp_mmd_rbf", c_int, [POINTER(MmdRbfParams), c_void_p]),
    ("aptp_image_patches_pil_size", c_int, [c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                            POINTER(c_int32)]),
    ("aptp_image_patches_pil", c_int, [POINTER(ImagePatchesPilParams), c_void_p]),
    ("aptp_eos_pool_ln", c_int, [POINTER(EosPoolLnParams), c_void_p]),
    ("aptp_paired_cosine", c_int, [POINTER(PairedCosineParams), c_void_p]),
    ("aptp_train_images", c_int, [POINTER(TrainImagesParams), c_void_p]),
    ("aptp_guided_step", c_int, [POINTER(GuidedStepParams), c_void_p]),
    ("aptp_philox_normal", c_int, [POINTER(PhiloxNormalParams), c_void_p]),
    ("aptp_train_noise", c_int, [POINTER(TrainNoiseParams), c_void_p]),
    ("aptp_last_error", c_char_p, []),
    ("aptp_version", c_int, []),
]

_lib = None


class AptpError(RuntimeError):
    pass


def load():
    """Load libaptp_hip.so (once) and declare the prototypes.  Raises if the library is missing: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles the HIP runtime (torch/lib/libamdhip64.so), and the process must end up with ONE
    # runtime.  Loaded after torch, libaptp_hip.so's libamdhip64.so.7 dependency resolves to the copy torch already
    # mapped; loaded before it, /opt/rocm's copy comes in as a second runtime and every launch on a torch stream fails with
    # "no ROCm-capable device is detected" (seen with build() followed by smoke() in one process).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise AptpError(
            f"{LIB_PATH} not found: the HIP extension is the only compute path of diffusion_pruning_amd. "
            "Build it with `make -C diffusion_pruning_amd/csrc` (hipcc, --offload-arch=gfx950).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in EXPORTS:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().aptp_last_error()
        raise AptpError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


class BlockTable:
    """The device table of a launch whose workgroups find their item by bisection (csrc/packed_pass.h: item_of_block): a filled
    ctypes array of item descriptors and the number of workgroups each item takes ->
      items    the descriptors' bytes in device memory (uint8)
      starts   int32 [n + 1]: first workgroup of item i; starts[n] == total, the grid size
      host     the ctypes array itself (kept alive: aptp_group_adamw validates it on the host)
    The caller checks the operands where it fills an item."""

    def __init__(self, host, blocks, device):
        import torch
        self.host, self.blocks = host, [int(b) for b in blocks]
        assert len(self.blocks) == len(host) >= 1, "BlockTable: one block count per item"
        starts = [0]
        for nb in self.blocks:
            starts.append(starts[-1] + nb)
        self.n, self.total = len(self.blocks), starts[-1]
        self.items = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
        self.starts = torch.tensor(starts, dtype=torch.int32).to(device)

    def subset(self, indices):
        """a table of its own over items[i] for i in indices, in that order: the same descriptors, block prefixes of their own"""
        indices = list(indices)
        host = (self.host._type_ * len(indices))(*[self.host[i] for i in indices])
        return BlockTable(host, [self.blocks[i] for i in indices], self.items.device)

    def args(self):
        """(items_dev, starts_dev, n_items, total_blocks) as the C entry points take them"""
        return self.items.data_ptr(), self.starts.data_ptr(), self.n, self.total
