"""ctypes binding of libafm_hip.so (include/afm_hip.h) - the thin FFI layer between the
Python host code and the hand-written gfx950 kernels.

There is NO fallback: if the library is missing or a call fails, an exception is raised.
Tensors are passed as raw device pointers (``tensor.data_ptr()``) plus explicit sizes; work is
enqueued on torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libafm_hip.so")
_lib = None

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3
ARITH_DEFAULT, ARITH_F32, ARITH_BF16X1, ARITH_BF16X6, ARITH_BF16X9 = 0, 1, 3, 6, 9       # afm_linear_args.arith (include/afm_hip.h)
TUNE_NO_DMA, TUNE_TILE_SHIFT = 0x1, 4
CMDM_NO_L0_CACHE, CMDM_FUSED_LN, CMDM_NO_LN_FOLD, CMDM_ALL_QUERIES, CMDM_CLIP_X0, CMDM_NO_RIDERS, CMDM_PAIR_LAUNCH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
CDM_NO_GEN, CDM_CHAIN_SIDE, CDM_DEC_CHUNKS_SHIFT, CDM_CLIP_X0, CDM_PIPELINE = 0x2, 0x4, 12, 0x8, 0x10
ABI_VERSION = 7
MAX_LAYERS = 16

c_f32p = C.c_void_p
i32, i64, u64 = C.c_int32, C.c_int64, C.c_uint64


class AfmError(RuntimeError):
    pass


class LinearArgs(C.Structure):
    _fields_ = [
        ("A", c_f32p), ("lda", i64), ("W", c_f32p), ("ldw", i64), ("C", c_f32p), ("ldc", i64),
        ("M", i32), ("N", i32), ("K", i32),
        ("bias", c_f32p), ("scale", c_f32p), ("residual", c_f32p), ("ldr", i64),
        ("rowtab", c_f32p), ("rowtab_period", i32), ("act", i32), ("act_post", i32),
        ("a_grp", i32), ("a_stride", i32), ("a_off", i32),
        ("c_grp", i32), ("c_stride", i32), ("c_off", i32),
        ("ddpm_xt", c_f32p), ("ddpm_noise", c_f32p), ("ddpm_out", c_f32p), ("ldx", i64),
        ("ddpm_c1", c_f32p), ("ddpm_c2", c_f32p), ("ddpm_sigma", c_f32p), ("rows_per_sample", i32),
        # training hooks (ABI v2)
        ("preact", c_f32p), ("ldp", i64), ("dact_z", c_f32p), ("ldz", i64), ("dact", i32),
        ("drop_p", C.c_float), ("drop_seed", u64), ("drop_id", C.c_uint32), ("drop_after", i32),
        # arithmetic of the product + bit-neutral tuning (ABI v3: fields instead of a process-wide switch)
        ("arith", i32), ("arith_min_n", i32), ("tune", i32),
        # fused row-dot epilogue (ABI v4)
        ("rowdot_w", c_f32p), ("rowdot_out", c_f32p), ("rowdot_n", i32),
        # fused LayerNorm of the output rows (ABI v5)
        ("ln_gamma", c_f32p), ("ln_beta", c_f32p), ("ln_out", c_f32p), ("ldo", i64), ("ln_eps", C.c_float), ("ln_counters", C.c_void_p),
        # LayerNorm folded across kernel boundaries (ABI v5)
        ("stat_out", c_f32p), ("a_stat", c_f32p), ("a_stat_groups", i32), ("a_fold_g", c_f32p),
        ("res_stat", c_f32p), ("res_gamma", c_f32p), ("res_beta", c_f32p), ("ln_eps2", C.c_float),
        # a hole inside every group of the row remaps (ABI v6)
        ("a_skip_after", i32), ("a_skip", i32), ("c_skip_after", i32), ("c_skip", i32),
        ("ddpm_clip", i32),
        ("ddpm_out2", c_f32p), ("ldx2", i64),
        ("aux_src", c_f32p), ("aux_idx", C.c_void_p), ("aux_add", c_f32p), ("aux_dst", c_f32p), ("aux_dst_ld", i64),
        ("aux_rows", i32), ("aux_cols", i32), ("aux_idx_max", i32),
    ]


class WgradArgs(C.Structure):
    _fields_ = [
        ("dY", c_f32p), ("lddy", i64), ("X", c_f32p), ("ldx", i64), ("dW", c_f32p), ("lddw", i64), ("db", c_f32p),
        ("M", i32), ("N", i32), ("K", i32),
        ("dy_grp", i32), ("dy_stride", i32), ("dy_off", i32), ("x_grp", i32), ("x_stride", i32), ("x_off", i32),
        ("accumulate", i32), ("ws", C.c_void_p), ("ws_bytes", i64),
    ]


class PtAttentionArgs(C.Structure):
    _fields_ = [("p", c_f32p), ("qkv", c_f32p), ("knn_idx", C.c_void_p), ("out", c_f32p),
                ("n", i32), ("channels", i32), ("nsample", i32), ("share_planes", i32)] + \
               [(n, c_f32p) for n in ("lp0_w", "lp0_b", "lp_bn_scale", "lp_bn_shift", "lp3_w", "lp3_b", "w0_bn_scale",
                                      "w0_bn_shift", "w2_w", "w2_b", "w3_bn_scale", "w3_bn_shift", "w5_w", "w5_b",
                                      "out_scale", "out_shift")] + [("relu", i32)]


class Lin(C.Structure):
    _fields_ = [("w", c_f32p), ("b", c_f32p)]


class Ln(C.Structure):
    _fields_ = [("g", c_f32p), ("b", c_f32p)]


class MhaW(C.Structure):
    _fields_ = [("q", Lin), ("k", Lin), ("v", Lin), ("o", Lin)]


class MlpW(C.Structure):
    _fields_ = [("norm", Ln), ("fc1", Lin), ("fc2", Lin)]


class CdmWeights(C.Structure):
    _fields_ = [
        ("contact_dim", i32), ("feat_dim", i32), ("dq", i32), ("dkv", i32), ("enc_heads", i32), ("dec_heads", i32),
        ("n_self", i32), ("text_dim", i32), ("time_dim", i32), ("n_timesteps", i32),
        ("time_q0", c_f32p), ("time_u", c_f32p), ("time_cu", c_f32p),
        ("language_adapter", Lin), ("time_embedding_adapter", Lin), ("encoder_adapter", Lin), ("decoder_adapter", Lin),
        ("enc_q_norm", Ln), ("enc_kv_norm", Ln), ("enc_attn", MhaW), ("enc_mlp", MlpW),
        ("self_norm", Ln * 4), ("self_attn", MhaW * 4), ("self_mlp", MlpW * 4),
        ("dec_q_norm", Ln), ("dec_kv_norm", Ln), ("dec_attn", MhaW), ("dec_mlp", MlpW),
        ("contact_layer", Lin),
        ("gemm_arith", i32), ("gemm_arith_min_n", i32),
        # weight products of the folded sampling form (ABI v4; all five or none)
        ("fold_xu", c_f32p), ("fold_xv", c_f32p), ("fold_w2", c_f32p), ("flags", i32), ("fold_q", c_f32p), ("fold_c0", c_f32p),
        # generator tables of the two adapters (ABI v5; all three or none)
        ("gen_qe", c_f32p),
        ("dec_c", c_f32p), ("dec_twx", c_f32p), ("dec_qxx", c_f32p), ("dec_qdd", c_f32p),
        ("enc_ec", c_f32p), ("enc_qee", c_f32p), ("enc_wove", c_f32p), ("enc_c1", c_f32p),
        ("dec_dwq", c_f32p), ("dec_wqb", c_f32p), ("dec_wco", c_f32p), ("dec_wow", c_f32p), ("dec_wog", c_f32p), ("dec_xwo", c_f32p),
        ("lat_fold", C.c_void_p),
    ]


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", i64), ("total_ms", C.c_double), ("total_work", C.c_double)]


class EncoderLayerWeights(C.Structure):
    _fields_ = [(n, c_f32p) for n in (
        "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
        "norm1_w", "norm1_b", "norm2_w", "norm2_b", "lin1_wg", "lin1_g", "lin1_c", "in_proj_wg", "in_proj_g", "in_proj_c")]


class CmdmWeights(C.Structure):
    _fields_ = [
        ("d", i32), ("heads", i32), ("ff", i32), ("n_layers", i32), ("motion_dim", i32), ("n_cond", i32),
        ("motion_adapter_w", c_f32p), ("motion_adapter_b", c_f32p),
        ("motion_layer_w", c_f32p), ("motion_layer_b", c_f32p),
        ("time_table", c_f32p), ("n_timesteps", i32), ("pos_table", c_f32p),
        ("layer", EncoderLayerWeights * MAX_LAYERS),
        ("gemm_arith", i32), ("gemm_arith_min_n", i32), ("attn_group_waves", i32), ("flags", i32),
        ("motion_adapter_kpad", i32),
        ("motion_layer_wg", c_f32p), ("motion_layer_g", c_f32p), ("motion_layer_c", c_f32p),
    ]


class DdpmArgs(C.Structure):
    _fields_ = [("noise", c_f32p), ("x_next", c_f32p), ("c1", c_f32p), ("c2", c_f32p), ("sigma", c_f32p),
                ("seed", u64), ("sample_index0", i64), ("step", i32)]


class DdimRows(C.Structure):
    """afm_ddim_rows (v7-additive): device pointers of the five DDIM rows (a, b, c, d, sigma); sigma None = no noise term."""
    _fields_ = [("a", c_f32p), ("b", c_f32p), ("c", c_f32p), ("d", c_f32p), ("sigma", c_f32p)]


class DpmRows(C.Structure):
    """afm_dpm_rows (v7-additive): device pointers of the three DPM-Solver++(2M) rows (a, b, c)."""
    _fields_ = [("a", c_f32p), ("b", c_f32p), ("c", c_f32p)]


class CfgArgs(C.Structure):
    """afm_cfg_args (v7-additive): classifier-free guidance of the CMDM - device [B] scales, the dropped conditions, AFM_CFG_* flags."""
    _fields_ = [("scale", c_f32p), ("drop_text", i32), ("drop_pc", i32), ("flags", i32), ("branch_streams", C.POINTER(C.c_void_p))]


class CfgStepArgs(C.Structure):
    """afm_cfg_step_args (v7-additive): one guided sampling update from the two branches' pred_xstart."""
    _fields_ = [("x0_c", c_f32p), ("x0_u", c_f32p), ("scale", c_f32p), ("x_t", c_f32p), ("noise", c_f32p), ("x_next", c_f32p),
                ("c1", c_f32p), ("c2", c_f32p), ("sigma", c_f32p), ("ddim", C.POINTER(DdimRows)), ("clip", i32), ("B", i32),
                ("per_sample", i64), ("seed", u64), ("sample_index0", i64), ("step", i32)]


class ImputeStepArgs(C.Structure):
    """afm_impute_step_args (v7-additive): afm_cfg_step_args with known / mask, the unconditioned branch optional."""
    _fields_ = [("x0_c", c_f32p), ("x0_u", c_f32p), ("scale", c_f32p), ("known", c_f32p), ("mask", C.c_void_p), ("x_t", c_f32p),
                ("noise", c_f32p), ("x_next", c_f32p), ("c1", c_f32p), ("c2", c_f32p), ("sigma", c_f32p), ("ddim", C.POINTER(DdimRows)),
                ("clip", i32), ("B", i32), ("per_sample", i64), ("seed", u64), ("sample_index0", i64), ("step", i32)]


class Cfg2Args(C.Structure):
    """afm_cfg2_args (v7-additive): two-scale guidance of the CMDM - device [B] scales of the first and second condition, first: 0 = text,
    1 = pc, AFM_CFG_* flags."""
    _fields_ = [("scale_first", c_f32p), ("scale_second", c_f32p), ("first", i32), ("flags", i32)]


class Cfg2StepArgs(C.Structure):
    """afm_cfg2_step_args (v7-additive): one two-scale sampling update from the three branches' pred_xstart, known / mask optional."""
    _fields_ = [("x0_c", c_f32p), ("x0_a", c_f32p), ("x0_u", c_f32p), ("scale_first", c_f32p), ("scale_second", c_f32p), ("known", c_f32p),
                ("mask", C.c_void_p), ("x_t", c_f32p), ("noise", c_f32p), ("x_next", c_f32p), ("c1", c_f32p), ("c2", c_f32p), ("sigma", c_f32p),
                ("ddim", C.POINTER(DdimRows)), ("clip", i32), ("B", i32), ("per_sample", i64), ("seed", u64), ("sample_index0", i64), ("step", i32)]


class GuideStepArgs(C.Structure):
    """afm_guide_step_args (v7-additive): one sampling update with every optional ingredient - branches, known / mask, grad / gk."""
    _fields_ = [("x0_c", c_f32p), ("x0_a", c_f32p), ("x0_u", c_f32p), ("scale", c_f32p), ("scale2", c_f32p), ("known", c_f32p),
                ("mask", C.c_void_p), ("grad", c_f32p), ("gk", c_f32p), ("x_t", c_f32p), ("noise", c_f32p), ("x_next", c_f32p),
                ("x0_out", c_f32p), ("c1", c_f32p), ("c2", c_f32p), ("sigma", c_f32p), ("ddim", C.POINTER(DdimRows)),
                ("dpm", C.POINTER(DpmRows)), ("x0_prev", c_f32p), ("clip", i32), ("B", i32), ("per_sample", i64), ("seed", u64),
                ("sample_index0", i64), ("step", i32)]


GUIDE_MAX_JOINTS = 16
H3D_JOINTS = 22                   # joints of the HumanML3D skeleton
H3D_COLS = 67                     # the feature columns the joint recovery reads: 0..66
H3D_SCAN_ROWS = 7                 # per-frame LDS rows of the joint recovery and of its adjoint
GUIDE_LDS_BYTES = 60 * 1024       # the LDS the guidance kernels stage into


class H3dLayout(C.Structure):
    """afm_h3d_layout (v7-additive): the motion vector holds HumanML3D features - the joint index 0..21 of each guided joint and the
    scene transform [3][4] (NULL: identity) with its batch stride in floats (0: one shared matrix, 12: one per sample)."""
    _fields_ = [("joints", i32 * GUIDE_MAX_JOINTS), ("to_scene", c_f32p), ("to_scene_stride", i32)]


class ContactGuide(C.Structure):
    """afm_contact_guide (v7-additive): the contact-guidance description - scene points, target map, columns, de-normalisation, scale, and
    for the loops the gk rows [T][B] and the first guided executed step; ``h3d``: NULL, or the layout of a HumanML3D-feature motion."""
    _fields_ = [("q", c_f32p), ("c", c_f32p), ("mean", c_f32p), ("std", c_f32p), ("scale", c_f32p), ("gk", c_f32p),
                ("frame_mask", C.c_void_p), ("cols", i32 * GUIDE_MAX_JOINTS), ("K", i32), ("N", i32), ("sigma", C.c_double), ("first_guided", i32), ("t_start", i64),
                ("h3d", C.POINTER(H3dLayout))]


class JointTargets(C.Structure):
    """afm_joint_targets (v7-additive): the joint-target description - target positions [B][L][K][3], weights [B][L][K], scale,
    de-normalisation, the columns (or ``h3d``: the layout of a HumanML3D-feature motion), and for the loops the term's own first guided step."""
    _fields_ = [("target", c_f32p), ("weight", c_f32p), ("scale", c_f32p), ("mean", c_f32p), ("std", c_f32p), ("cols", i32 * GUIDE_MAX_JOINTS),
                ("K", i32), ("first_guided", i32), ("t_start", i64), ("h3d", C.POINTER(H3dLayout))]


class MotionGuide(C.Structure):
    """afm_motion_guide (v7-additive): the sum of the contact and the joint-target guidance (either may be NULL, not both) and, for the
    loops, the gk rows [T][B] and the guidance's frame mask."""
    _fields_ = [("contact", C.POINTER(ContactGuide)), ("targets", C.POINTER(JointTargets)), ("gk", c_f32p), ("frame_mask", C.c_void_p)]


CLEAR_WAVES = 8                   # waves per block of the clearance kernel: the spans of its summation order
CLEAR_TILE = 1024                 # points per LDS tile of the clearance kernel


class SceneClearance(C.Structure):
    """afm_scene_clearance (v7-additive): the scene-clearance description - scene points, point weights (or NULL), the contact map of
    the exemption (or NULL) with its column count and threshold, de-normalisation, scale, the columns (or ``h3d``), a radius per joint,
    the up axis and the floor height with its flag, and for the loops the term's own first guided step."""
    _fields_ = [("q", c_f32p), ("weight", c_f32p), ("c", c_f32p), ("mean", c_f32p), ("std", c_f32p), ("scale", c_f32p),
                ("cols", i32 * GUIDE_MAX_JOINTS), ("K", i32), ("N", i32), ("Kc", i32), ("exempt", i32), ("c_min", C.c_double),
                ("radius", C.c_double * GUIDE_MAX_JOINTS), ("up", i32), ("has_min_height", i32), ("min_height", C.c_double),
                ("first_guided", i32), ("t_start", i64), ("h3d", C.POINTER(H3dLayout))]


class SceneGuide(C.Structure):
    """afm_scene_guide (v7-additive): the sum of an afm_motion_guide (or NULL) and the scene clearance (or NULL) and, for the loops, the gk
    rows [T][B] and the guidance's frame mask."""
    _fields_ = [("terms", C.POINTER(MotionGuide)), ("clearance", C.POINTER(SceneClearance)), ("gk", c_f32p), ("frame_mask", C.c_void_p)]


GROUND_LABEL_COL = 259            # HumanML3D's foot-contact columns 259..262
GROUND_LABEL_SLOT = {7: 0, 10: 1, 8: 2, 11: 3}          # left foot (joints 7, 10) before the right one (8, 11)


class FootGrounding(C.Structure):
    """afm_foot_grounding (v7-additive): the foot-grounding description - de-normalisation, scale, the columns (or ``h3d``), the up axis,
    the labels switch, for the loops the term's own first guided step, the floor, a height per joint and the two weights."""
    _fields_ = [("mean", c_f32p), ("std", c_f32p), ("scale", c_f32p), ("cols", i32 * GUIDE_MAX_JOINTS), ("K", i32), ("up", i32),
                ("labels", i32), ("first_guided", i32), ("floor", C.c_double), ("height", C.c_double * GUIDE_MAX_JOINTS),
                ("floor_weight", C.c_double), ("skate_weight", C.c_double), ("t_start", i64), ("h3d", C.POINTER(H3dLayout))]


class GroundGuide(C.Structure):
    """afm_ground_guide (v7-additive): the sum of an afm_scene_guide (or NULL) and the foot grounding (or NULL) and, for the loops, the gk
    rows [T][B] and the guidance's frame mask."""
    _fields_ = [("terms", C.POINTER(SceneGuide)), ("feet", C.POINTER(FootGrounding)), ("gk", c_f32p), ("frame_mask", C.c_void_p)]


class Stitch(C.Structure):
    """afm_stitch (v7-additive): a batch of G * S overlapping windows of G long motions - windows per motion, shared frames of two
    neighbours, the device weight row [2][overlap] (wl then wr)."""
    _fields_ = [("windows", i32), ("overlap", i32), ("weights", c_f32p)]


class StitchStepArgs(C.Structure):
    """afm_stitch_step_args (v7-additive): one stitched sampling update - branches, known / mask, DDIM (eta = 0) or 2M rows."""
    _fields_ = [("x0_c", c_f32p), ("x0_a", c_f32p), ("x0_u", c_f32p), ("scale", c_f32p), ("scale2", c_f32p), ("known", c_f32p),
                ("mask", C.c_void_p), ("x_t", c_f32p), ("x_next", c_f32p), ("x0_out", c_f32p), ("ddim", C.POINTER(DdimRows)),
                ("dpm", C.POINTER(DpmRows)), ("x0_prev", c_f32p), ("stitch", C.POINTER(Stitch)), ("clip", i32), ("B", i32), ("L", i32),
                ("D", i32)]


class LongGuide(C.Structure):
    """afm_long_guide (v7-additive): the guidance of stitched long motions - the terms (scale rows [G], long-form targets, q / c per window),
    the stitch and the long motion's frames F."""
    _fields_ = [("terms", C.POINTER(MotionGuide)), ("stitch", Stitch), ("frames", i32)]


class LongSceneGuide(C.Structure):
    """afm_long_scene_guide (v7-additive): the long guidance with the scene clearance as a third term - the long description (its terms
    always set, possibly naming neither term) and the clearance (q / weight / c per window, scale [G]) or NULL."""
    _fields_ = [("base", C.POINTER(LongGuide)), ("clearance", C.POINTER(SceneClearance))]


CFG_FORCE_MASKED = 0x1

EXPORTS = {
    # name: (restype, argtypes)
    "afm_version": (C.c_int, []),
    "afm_linear": (C.c_int, [C.POINTER(LinearArgs), C.c_void_p]),
    "afm_linear_pair": (C.c_int, [C.POINTER(LinearArgs), C.POINTER(LinearArgs), C.c_void_p]),
    "afm_mha_fwd": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i32, i32, i32, i32, C.c_void_p]),
    "afm_mha_fwd_grouped": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_clamp": (C.c_int, [c_f32p, i64, C.c_float, C.c_float, C.c_void_p]),
    "afm_mha_fwd_rows": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i32, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_mha_fwd_arith": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i32, i32, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_mha_cross_fwd": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_layernorm": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, C.c_float, C.c_void_p]),
    "afm_layernorm_rows": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, C.c_float, i32, i32, i32, C.c_void_p]),
    "afm_ddpm_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i64, u64, i64, i32, C.c_void_p]),
    "afm_randn": (C.c_int, [c_f32p, i32, i64, u64, i64, i32, C.c_void_p]),
    "afm_ddim_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(DdimRows), i32, i64, u64, i64, i32, C.c_void_p]),
    "afm_ddim_sched_scratch_bytes": (i64, [i32, i32]),
    "afm_cmdm_ddim_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                           i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cdm_ddim_loop_range": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                          i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cfg_combine": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i64, C.c_void_p]),
    "afm_cfg_step": (C.c_int, [C.POINTER(CfgStepArgs), C.c_void_p]),
    "afm_cmdm_cfg_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32]),
    "afm_cmdm_cfg_forward": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(CfgArgs), c_f32p, c_f32p, c_f32p,
                                       i32, i32, C.c_void_p, i64, C.c_void_p]),
    "afm_cmdm_cfg_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs)]),
    "afm_cmdm_cfg_sample_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p,
                                                 C.POINTER(CfgArgs), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                                 C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cmdm_cfg_ddim_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                               C.POINTER(CfgArgs), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                               C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_impute": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, i64, C.c_void_p]),
    "afm_impute_step": (C.c_int, [C.POINTER(ImputeStepArgs), C.c_void_p]),
    "afm_cmdm_impute_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                             c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), c_f32p, C.c_void_p, i32, i32, u64, i64, i32, i32,
                                             C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cdm_impute_loop_range": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                            c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                            C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cdm_dpm_loop_workspace_bytes": (i64, [C.POINTER(CdmWeights), i32, i32, i32]),
    "afm_cdm_dpm_loop_range": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.POINTER(DpmRows), c_f32p,
                                         C.c_void_p, i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cfg2_combine": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i64, C.c_void_p]),
    "afm_cfg2_step": (C.c_int, [C.POINTER(Cfg2StepArgs), C.c_void_p]),
    "afm_cmdm_cfg2_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32]),
    "afm_cmdm_cfg2_forward": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(Cfg2Args), c_f32p, c_f32p, c_f32p,
                                        c_f32p, i32, i32, C.c_void_p, i64, C.c_void_p]),
    "afm_cmdm_cfg2_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(Cfg2Args)]),
    "afm_cmdm_cfg2_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                           c_f32p, c_f32p, c_f32p, C.POINTER(Cfg2Args), c_f32p, C.c_void_p, i32, i32, u64, i64, i32, i32,
                                           C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_dpm_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(DpmRows), i32, i64, C.c_void_p]),
    "afm_cmdm_dpm_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args)]),
    "afm_cmdm_dpm_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.POINTER(DpmRows), C.POINTER(CfgArgs),
                                          C.POINTER(Cfg2Args), c_f32p, C.c_void_p, i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                          C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_guide_step": (C.c_int, [C.POINTER(GuideStepArgs), C.c_void_p]),
    "afm_contact_guidance_workspace_bytes": (i64, [i32, i32, i32]),
    "afm_contact_guidance": (C.c_int, [C.POINTER(ContactGuide), c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, i64,
                                       C.c_void_p]),
    "afm_contact_guidance_h3d_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "afm_h3d_joints": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.POINTER(i32), i32, c_f32p, i32, c_f32p, i32, i32, i32, C.c_void_p]),
    "afm_motion_guidance_workspace_bytes": (i64, [C.POINTER(MotionGuide), i32, i32, i32]),
    "afm_motion_guidance": (C.c_int, [C.POINTER(MotionGuide), c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, i64,
                                      C.c_void_p]),
    "afm_cmdm_motion_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                         C.POINTER(MotionGuide)]),
    "afm_cmdm_motion_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                                   C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p,
                                                   C.c_void_p, C.POINTER(MotionGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                                   C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_ground_guidance_workspace_bytes": (i64, [C.POINTER(GroundGuide), i32, i32, i32]),
    "afm_ground_guidance": (C.c_int, [C.POINTER(GroundGuide), c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32,
                                      C.c_void_p, i64, C.c_void_p]),
    "afm_cmdm_ground_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                         C.POINTER(GroundGuide)]),
    "afm_cmdm_ground_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                                   C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p,
                                                   C.c_void_p, C.POINTER(GroundGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                                   C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_scene_guidance_workspace_bytes": (i64, [C.POINTER(SceneGuide), i32, i32, i32]),
    "afm_scene_guidance": (C.c_int, [C.POINTER(SceneGuide), c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p,
                                     i64, C.c_void_p]),
    "afm_cmdm_scene_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                        C.POINTER(SceneGuide)]),
    "afm_cmdm_scene_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                                  C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p,
                                                  C.c_void_p, C.POINTER(SceneGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                                  C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cmdm_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                  C.POINTER(ContactGuide)]),
    "afm_cmdm_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                            C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p, C.c_void_p,
                                            C.POINTER(ContactGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                            C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_stitch_blend": (C.c_int, [c_f32p, c_f32p, C.POINTER(Stitch), i32, i32, i32, C.c_void_p]),
    "afm_stitch_windows": (C.c_int, [c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_stitch_join": (C.c_int, [c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, C.c_void_p]),
    "afm_stitch_step": (C.c_int, [C.POINTER(StitchStepArgs), C.c_void_p]),
    "afm_cmdm_stitch_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                   C.POINTER(Stitch)]),
    "afm_cmdm_stitch_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                             C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p, C.c_void_p,
                                             C.POINTER(Stitch), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                             C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_long_guidance_workspace_bytes": (i64, [C.POINTER(LongGuide), i32, i32, i32]),
    "afm_long_guidance": (C.c_int, [C.POINTER(LongGuide), c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, i64, C.c_void_p]),
    "afm_stitch_guide_step": (C.c_int, [C.POINTER(StitchStepArgs), c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "afm_cmdm_long_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                       C.POINTER(LongGuide)]),
    "afm_cmdm_long_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                                 C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p, C.c_void_p,
                                                 C.POINTER(LongGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                                 C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_long_scene_guidance_workspace_bytes": (i64, [C.POINTER(LongSceneGuide), i32, i32, i32]),
    "afm_long_scene_guidance": (C.c_int, [C.POINTER(LongSceneGuide), c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, i64,
                                          C.c_void_p]),
    "afm_cmdm_long_scene_guide_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32, C.POINTER(CfgArgs), C.POINTER(Cfg2Args),
                                                             C.POINTER(LongSceneGuide)]),
    "afm_cmdm_long_scene_guide_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, C.POINTER(DdimRows),
                                                       C.POINTER(DpmRows), c_f32p, c_f32p, c_f32p, C.POINTER(CfgArgs), C.POINTER(Cfg2Args), c_f32p,
                                                       C.c_void_p, C.POINTER(LongSceneGuide), i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64,
                                                       i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_bn_fold": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_float, c_f32p, c_f32p, c_f32p, i32, C.c_void_p]),
    "afm_contact_glue": (C.c_int, [c_f32p, c_f32p, i64, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "afm_masked_mse": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, i32, i32, i32, C.c_void_p]),
    "afm_transpose": (C.c_int, [c_f32p, c_f32p, i32, i32, C.c_void_p]),
    "afm_linear_wgrad_workspace_bytes": (i64, [i32, i32, i32]),
    "afm_linear_wgrad": (C.c_int, [C.POINTER(WgradArgs), C.c_void_p]),
    "afm_layernorm_bwd_workspace_bytes": (i64, [i64, i32]),
    "afm_layernorm_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, C.c_float, C.c_float, u64,
                                    C.c_uint32, C.c_void_p, i64, C.c_void_p]),
    "afm_mha_fwd_train": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64, C.c_uint32, C.c_void_p]),
    "afm_mha_bwd": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64, C.c_uint32,
                              C.c_void_p, i64, C.c_void_p]),
    "afm_mha_cross_fwd_train": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, i32, i32, i32, i32, i32, C.c_float, u64, C.c_uint32, C.c_void_p]),
    "afm_mha_cross_bwd": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, C.c_float, u64,
                                   C.c_uint32, C.c_void_p, i64, C.c_void_p]),
    "afm_masked_mse_bwd": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, i32, i32, i32, C.c_void_p]),
    "afm_rowop": (C.c_int, [c_f32p, c_f32p, i32, c_f32p, i32, c_f32p, i64, i32, C.c_float, u64, C.c_uint32, C.c_void_p]),
    "afm_colstats_workspace_bytes": (i64, [i64, i32]),
    "afm_colstats": (C.c_int, [c_f32p, i64, i32, c_f32p, C.c_void_p, i64, C.c_void_p]),
    "afm_bn_finalize": (C.c_int, [c_f32p, i32, i64, c_f32p, c_f32p, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32,
                                  C.c_void_p]),
    "afm_colaffine": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i32, c_f32p, i64, i32, C.c_void_p]),
    "afm_bn_bwd_stats": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, c_f32p, C.c_void_p, i64, C.c_void_p]),
    "afm_bn_bwd_apply": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i64, c_f32p, c_f32p, i64, i32, C.c_void_p]),
    "afm_group_points": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, i64, i32, i32, C.c_void_p]),
    "afm_scatter_add_rows": (C.c_int, [c_f32p, i64, i32, C.c_void_p, c_f32p, i64, i32, C.c_void_p]),
    "afm_group_max": (C.c_int, [c_f32p, c_f32p, C.c_void_p, i64, i32, i32, C.c_void_p]),
    "afm_group_max_bwd": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i64, i32, i32, C.c_void_p]),
    "afm_scatter_plan_words": (C.c_int64, [i64, i64]),
    "afm_scatter_plan": (C.c_int, [C.c_void_p, i64, i64, C.c_void_p, C.c_void_p]),
    "afm_segment_sum_rows": (C.c_int, [c_f32p, i64, i32, i32, C.c_void_p, C.c_void_p, c_f32p, i64, i32, C.c_void_p]),
    "afm_group_sum": (C.c_int, [c_f32p, c_f32p, i64, i32, i32, C.c_float, C.c_void_p]),
    "afm_pt_w0": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, i32, C.c_void_p]),
    "afm_pt_aggregate": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, i32, i32, C.c_void_p]),
    "afm_pt_aggregate_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i64, i32, i32, i32, C.c_void_p]),
    "afm_xq_workspace_bytes": (i64, [i32, i32, i32]),
    "afm_xq_attention_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64, C.c_uint32, C.c_void_p, i64,
                                       C.c_void_p]),
    "afm_xq_attention_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64,
                                       C.c_uint32, C.c_void_p, i64, C.c_void_p]),
    "afm_xk_workspace_bytes": (i64, [i32, i32, i32]),
    "afm_xk_attention_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64, C.c_uint32, C.c_void_p]),
    "afm_xk_attention_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, C.c_float, u64, C.c_uint32,
                                       C.c_void_p, i64, C.c_void_p]),
    "afm_adamw_multi": (C.c_int, [C.c_void_p, i32, i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32, C.c_void_p]),
    "afm_adamw": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32, C.c_void_p]),
    "afm_fps": (C.c_int, [c_f32p, i32, i32, i32, C.c_void_p, C.c_void_p]),
    "afm_knn": (C.c_int, [i32, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, c_f32p, C.c_void_p]),
    "afm_knn_workspace_bytes": (C.c_int64, [i32, i32, i32, i32]),
    "afm_knn_ws": (C.c_int, [i32, c_f32p, c_f32p, i32, i32, i32, C.c_void_p, c_f32p, C.c_void_p, i64, C.c_void_p]),
    "afm_gather_rows": (C.c_int, [c_f32p, C.c_void_p, c_f32p, i64, i32, C.c_void_p]),
    "afm_interpolate": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, i64, i32, i32, C.c_void_p]),
    "afm_segment_mean": (C.c_int, [c_f32p, c_f32p, i32, i32, i32, C.c_void_p]),
    "afm_interpolate_bwd": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, i64, i64, i32, i32, C.c_void_p]),
    "afm_transition_down": (C.c_int, [c_f32p, c_f32p, i32, c_f32p, C.c_void_p, i32, c_f32p, i32, c_f32p, c_f32p, c_f32p,
                                      i32, C.c_void_p]),
    "afm_pt_attention": (C.c_int, [C.POINTER(PtAttentionArgs), C.c_void_p]),
    "afm_cdm_workspace_bytes": (i64, [C.POINTER(CdmWeights), i32, i32]),
    "afm_cdm_forward": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p,
                                  C.POINTER(DdpmArgs), i32, i32, C.c_void_p, i64, C.c_void_p]),
    "afm_cdm_forward_overlap": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p,
                                          C.POINTER(DdpmArgs), i32, i32, C.c_void_p, i64, C.c_void_p, C.c_void_p]),
    "afm_cdm_loop_workspace_bytes": (i64, [C.POINTER(CdmWeights), i32, i32, i32]),
    "afm_cdm_sample_loop": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p,
                                      i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cdm_sample_loop_range": (C.c_int, [C.POINTER(CdmWeights), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p,
                                            c_f32p, i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32, C.POINTER(C.c_void_p),
                                            C.c_void_p]),
    "afm_cdm_latent_tokens": (C.c_int, [C.POINTER(CdmWeights), i32, c_f32p, i32, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "afm_profile_enable": (C.c_int, [i32]),
    "afm_profile_read": (C.c_int, [C.POINTER(ProfileEntry), i32]),
    "afm_cmdm_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32]),
    "afm_cmdm_forward": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, C.c_void_p, c_f32p, C.c_void_p, c_f32p,
                                   C.POINTER(DdpmArgs), i32, i32, C.c_void_p, i64, C.c_void_p]),
    "afm_cmdm_sched_scratch_bytes": (i64, [i32, i32]),
    "afm_cmdm_loop_workspace_bytes": (i64, [C.POINTER(CmdmWeights), i32, i32, i32]),
    "afm_cmdm_sample_loop": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, c_f32p,
                                       c_f32p, c_f32p, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                       C.POINTER(C.c_void_p), C.c_void_p]),
    "afm_cmdm_sample_loop_range": (C.c_int, [C.POINTER(CmdmWeights), c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, c_f32p,
                                             c_f32p, c_f32p, i32, i32, u64, i64, i32, i32, C.c_void_p, C.c_void_p, i64, i32,
                                             C.POINTER(C.c_void_p), C.c_void_p]),
}


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load (once) and type every export.  Raises AfmError when the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise AfmError(f"{_LIB_PATH} not found: build it with `python afford-motion_amd/build_hip.py` "
                       "(the HIP path has no CPU or eager fallback)")
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = {-1: "bad argument", -2: "workspace too small", -3: "unsupported shape"}.get(rc, f"hipError {rc}")
        raise AfmError(f"{what} failed: {kind}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_of(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def sched_scratch(owner, n_steps: int, batch: int, device, *, ddim: bool = False) -> torch.Tensor:
    """The expanded-schedule scratch of a native sampling loop (afm_cmdm_sched_scratch_bytes), kept on `owner` (the model) across calls and
    grown geometrically from 1 MiB (1000 steps x 32 samples need 0.64 MB): a loop call allocates NOTHING after the first one, whatever its
    step count - a fresh device allocation inside a short loop call costs tens of milliseconds (tools/probe_k20_first.py: the first 20-step
    call 100 ms instead of 46).  Calls are stream-ordered, so the next call's expand kernel cannot overtake the previous call's readers."""
    fn = "afm_ddim_sched_scratch_bytes" if ddim else "afm_cmdm_sched_scratch_bytes"     # (the DDIM loops: float4 row records)
    need = int(getattr(load(), fn)(n_steps, batch))
    if need < 0:
        check(need, fn)
    cache = owner.__dict__.setdefault("_afm_sched", {})
    buf = cache.get(str(device))
    if buf is None or buf.numel() < need:
        size = 1 << 20
        while size < need:
            size *= 2
        buf = cache[str(device)] = torch.empty(size, dtype=torch.uint8, device=device)
    return buf


class LoopTables:
    """What one native sampling-loop call reads of the schedule: the `_DeviceTables` of ``diffusion`` on ``device``, the DDIM rows of
    ``ddim_eta`` or None, the DPM-Solver++ rows of ``dpm_order`` or None, and the expanded-schedule scratch (`sched_scratch` on ``owner``,
    the model).  It knows the ABI's ordering of the row arguments of a range call whose first timestep index is ``lo``, nothing else."""

    def __init__(self, owner, diffusion, B: int, device, ddim_eta=None, dpm_order=None):
        self.n = diffusion.num_timesteps
        self.tab = diffusion.tables(device)
        self.sched = sched_scratch(owner, self.n, B, device, ddim=ddim_eta is not None or dpm_order is not None)
        self.ddim = None if ddim_eta is None else diffusion.ddim_tables(device, ddim_eta)
        self.dpm = None if dpm_order is None else diffusion.dpm_tables(device, dpm_order)

    def tmap(self, lo: int) -> int:
        return self.tab.timestep_map[lo:].data_ptr()

    def rows(self, lo: int, every_form: bool = False) -> tuple:
        """(c1, c2, sigma) of a DDPM-only entry or (afm_ddim_rows*,) of a DDIM-only one; ``every_form``: the (rows, c1, c2, sigma) of an
        entry that runs both updates, the other kind NULL."""
        if self.ddim is not None:
            rows = C.byref(self.ddim.rows(lo))
            return (rows, None, None, None) if every_form else (rows,)
        ddpm = (self.tab.coef1[lo:].data_ptr(), self.tab.coef2[lo:].data_ptr(), self.tab.sigma[lo:].data_ptr())
        return (None,) + ddpm if every_form else ddpm

    def dpm_rows(self, lo: int):
        return C.byref(self.dpm.rows(lo))

    def named(self, lo: int) -> dict:
        """the one kind of rows this chain has, by the slot names of afm.cmdm.plan_loop_call"""
        if self.dpm is not None:
            return {"dpm_rows": self.dpm_rows(lo)}
        if self.ddim is not None:
            return {"ddim_rows": C.byref(self.ddim.rows(lo))}
        return dict(zip(("c1", "c2", "sigma"), self.rows(lo)))

    def keep(self) -> tuple:
        """what the caller holds until the stream has consumed the loop"""
        return (self.sched, self.ddim, self.dpm)


def workspace(cache: dict, key, sizer: str, *args, device, single: bool = False) -> torch.Tensor:
    """The byte buffer ``cache[key]`` of a native call, sized by the library's ``sizer(*args)`` (a negative size is its error code).
    ``single`` (the CMDM): the key fixes the size, a hit is returned unsized, and a miss replaces whatever the cache held - one buffer per
    model.  Otherwise (the CDM) every key stays and a cached buffer smaller than this call needs is re-allocated (one key covers the
    sampling forms, whose sizes differ)."""
    buf = cache.get(key)
    if buf is not None and single:
        return buf
    nbytes = int(getattr(load(), sizer)(*args))
    if nbytes < 0:
        check(nbytes, sizer)
    if buf is None or buf.numel() < nbytes:
        if single:
            cache.clear()
        buf = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def impute_ptrs(impute) -> tuple:
    """the (known, mask) pointer pair of an afm.diffusion.Impute, or two NULLs"""
    return (None, None) if impute is None else (impute.known.data_ptr(), impute.mask.data_ptr())


_HIP_RT = None


_STREAM_POOL = {}


def stream_pool(device, n: int):
    """The first `n` side streams of the PROCESS-WIDE pool of `device` (created on demand, never destroyed).  The HIP runtime multiplexes its
    streams onto a handful of hardware queues (four by default): kernels of two streams that share a queue run strictly one after the other,
    whatever the events between them say (round 6: the CDM pipeline with private streams per model - seven alive in the process - ran its
    "concurrent" latent chains serialised behind the point kernels, 2.7 k against 5.8 k steps/s).  Every loop of this package therefore
    takes its side streams from ONE pool, so that the streams alive in a sampling process stay at the null stream + at most three."""
    key = str(device)
    pool = _STREAM_POOL.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def cu_masked_stream(device, mask_words):
    """A HIP stream restricted to the compute units whose bits are set in `mask_words` (uint32 words, bit i = CU i as the runtime numbers
    them), wrapped so that torch sees it (`.cuda_stream`, events).  hipExtStreamCreateWithCUMask lives in the HIP runtime the process has
    already loaded (libamdhip64): the library of this package neither creates nor owns streams."""
    global _HIP_RT
    if _HIP_RT is None:
        _HIP_RT = C.CDLL("libamdhip64.so")
        _HIP_RT.hipExtStreamCreateWithCUMask.restype = C.c_int
        _HIP_RT.hipExtStreamCreateWithCUMask.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32)]
    words = [int(w) & 0xFFFFFFFF for w in mask_words]
    arr = (C.c_uint32 * len(words))(*words)
    handle = C.c_void_p()
    with torch.cuda.device(device):
        rc = _HIP_RT.hipExtStreamCreateWithCUMask(C.byref(handle), len(words), arr)
    if rc != 0 or not handle.value:
        raise AfmError(f"hipExtStreamCreateWithCUMask failed (hipError {rc})")
    return torch.cuda.ExternalStream(handle.value, device=device)


def require_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise AfmError("afford-motion_amd runs on the MI355X HIP path only; got a CPU tensor "
                           "(the CPU oracle lives in oracle/ and is test infrastructure)")


def f32c(t: torch.Tensor) -> torch.Tensor:
    """float32 + contiguous view/copy of ``t``."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def profile_enable(on: bool) -> None:
    check(load().afm_profile_enable(1 if on else 0), "afm_profile_enable")


def profile_read():
    """-> {kernel name: dict(launches, total_ms, total_work)} since the last read (synchronises)."""
    buf = (ProfileEntry * 32)()
    n = load().afm_profile_read(buf, 32)
    if n < 0:
        check(n, "afm_profile_read")
    return {buf[i].name.decode(): dict(launches=buf[i].launches, total_ms=buf[i].total_ms, total_work=buf[i].total_work)
            for i in range(n)}


def progress_slices(n_steps: int, progress: bool, slices: int = 50):
    """Executed-step ranges [(j0, j1), ...] of a native sampling loop: one range without a progress bar, ~`slices` ranges with one
    (the bar advances between native enqueues; gaussian_diffusion.py:520-523's tqdm over the step indices)."""
    if not progress:
        return [(0, n_steps)]
    per = max(1, -(-n_steps // slices))
    return [(j, min(j + per, n_steps)) for j in range(0, n_steps, per)]


def cut_slices(ranges, cuts):
    """Split the (j0, j1) ranges at every executed-step count in `cuts` (chained slices stay bit-identical to the whole loop)."""
    out = []
    for j0, j1 in ranges:
        for c in cuts:
            if j0 < c < j1:
                out.append((j0, c))
                j0 = c
        out.append((j0, j1))
    return out


def run_slices(ranges, enqueue, progress: bool, device):
    """Enqueue every slice; with a progress bar, advance it as the device finishes each slice (one event per slice, the next slice is
    already queued while the host waits, so the GPU never idles on the bar)."""
    import torch
    if not progress:
        for j0, j1 in ranges:
            enqueue(j0, j1)
        return
    from tqdm.auto import tqdm
    bar = tqdm(total=ranges[-1][1])
    pending = None
    for j0, j1 in ranges:
        enqueue(j0, j1)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        if pending is not None:
            pending[0].synchronize()
            bar.update(pending[1])
        pending = (ev, j1 - j0)
    pending[0].synchronize()
    bar.update(pending[1])
    bar.close()


def run_native_loop(x, n_steps: int, step_noise, progress: bool, snapshots, call):
    """The host side shared by the native sampling loops: `call(j0, j1, noise_ptr)` issues the native range call for the executed steps
    j0..j1-1.  ``step_noise`` ([n_steps, *x.shape] or None) is brought to x's device as contiguous float32 and returned - the caller keeps
    it alive until the stream has consumed it.  ``progress`` slices the chain for a tqdm bar.  ``snapshots`` = {executed step count: None}:
    the chain is cut at those counts and x is cloned there (stream-ordered device copies, no host synchronisation) - the intermediate
    states p_sample_loop_progressive would yield.  Chained slices are bit-identical to the whole loop."""
    if step_noise is not None:
        step_noise = f32c(step_noise.to(x.device))
        assert step_noise.shape == (n_steps,) + tuple(x.shape), step_noise.shape
    slices = progress_slices(n_steps, progress)
    if snapshots is not None:
        slices = cut_slices(slices, sorted(k for k in snapshots if 0 < k < n_steps))

    def enqueue(j0, j1):
        call(j0, j1, None if step_noise is None else step_noise[j0:j1].data_ptr())
        if snapshots is not None and j1 in snapshots:
            snapshots[j1] = x.clone()
    run_slices(slices, enqueue, progress, x.device)
    return step_noise
