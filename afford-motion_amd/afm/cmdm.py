"""CMDM / AMDM denoiser (`trans_enc`): drop-in for the reference's `models.cmdm.CMDM`
(reference models/cmdm.py:12-196) - same registry name, constructor, config keys, call
signature and state-dict keys - with the forward pass running on hand-written HIP kernels.

What differs from the reference (results identical, SURVEY.md section 7 "hard parts"):
  * the step-invariant condition tokens (text adapter, SceneMapEncoder + contact adapter and
    their positional encodings) are computed once per distinct set of condition tensors and
    cached; the reference recomputes them in every one of the 1000 steps (cmdm.py:134-156).
    ``model.hoist_conditions = False`` restores per-call recomputation ("faithful" timing).
  * TimestepEmbedder(t) depends on t only -> a [1000, d] table built once per weight version.
  * sampling can run as one native loop (afm_cmdm_sample_loop) with the DDPM update fused into
    the last GEMM's epilogue.
  * classifier-free guided sampling (`GuidedCMDM`, at the end of this file): both branches and
    the guided update inside the same native loops.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Mapping, NamedTuple, Optional

import torch
import torch.nn as nn

from . import autograd as AG
from . import ffi, fold, ops
from ._cache import HeldKey
from .base import Model
from .guidance import ContactGuidance, FootGrounding, JointTargets, LongGuidance, MotionGuidance, SceneClearance, scale_row, scale_value
from .scene import SceneMapEncoder, SceneMapEncoderDecoder
from .text import TextEncoderMixin, lang_feat_dim_type


def compute_repr_dimesion(data_repr: str) -> int:
    """Feature width per data representation (reference utils/misc.py:4-22; name kept as spelt there)."""
    table = {"smplx_no_hands": 69, "pos": 66, "pos_rot": 129, "contact_one_joints": 1, "contact_all_joints": 22,
             "contact_cont_joints": 6, "contact_pelvis": 1, "h3d": 263}
    if data_repr not in table:
        raise ValueError(f"Unknown data representation: {data_repr}")
    return table[data_repr]


def sinusoid_table(max_len: int, dim: int) -> torch.Tensor:
    """pe[pos, 2i] = sin(pos * w_i), pe[pos, 2i+1] = cos(pos * w_i), w_i = exp(-2i ln(1e4)/dim);
    stored [max_len, 1, dim] like the reference's buffers (models/modules.py:10-26)."""
    pos = torch.arange(max_len, dtype=torch.float32)[:, None]
    freq = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * (-math.log(10000.0) / dim))
    pe = torch.zeros(max_len, dim)
    pe[:, 0::2] = torch.sin(pos * freq)
    pe[:, 1::2] = torch.cos(pos * freq)
    return pe[:, None, :]


class TimestepEmbedder(nn.Module):
    """Parameter container: pe[t] -> Linear -> SiLU -> Linear (reference models/modules.py:38-53)."""

    def __init__(self, d_model: int, time_embed_dim: int, max_len: int = 5000):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(max_len, time_embed_dim))
        self.d_model, self.time_embed_dim = d_model, time_embed_dim
        self.time_embed = nn.Sequential(nn.Linear(time_embed_dim, d_model), nn.SiLU(), nn.Linear(d_model, d_model))

    def table(self) -> torch.Tensor:
        """Embedding of every timestep, [max_len, d_model], two HIP GEMMs (SiLU fused in the first)."""
        h = ops.linear(self.pe[:, 0, :], self.time_embed[0].weight, self.time_embed[0].bias, act=ffi.ACT_SILU)
        return ops.linear(h, self.time_embed[2].weight, self.time_embed[2].bias)

    def run(self, t_idx: torch.Tensor) -> torch.Tensor:
        """Embedding of the timesteps t_idx [B] (int64, on the device) -> [B, d_model] on the differentiable HIP operators."""
        h = AG.linear(self.pe[t_idx, 0, :], self.time_embed[0].weight, self.time_embed[0].bias, act=ffi.ACT_SILU)
        return AG.linear(h, self.time_embed[2].weight, self.time_embed[2].bias)

    def forward(self, timesteps):
        return self.table()[timesteps].unsqueeze(1)


class PositionalEncoding(nn.Module):
    """Buffer container for the sequence positional table (reference models/modules.py:28-36)."""

    def __init__(self, time_emb_dim, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.register_buffer("pe", sinusoid_table(max_len, time_emb_dim))


COND_SWITCHES = ("c_text_mask", "c_text_erase", "c_pc_mask", "c_pc_erase")


def _param_version(module: nn.Module) -> int:
    """Changes whenever a parameter / buffer of `module` is written in place (optimiser step, load_state_dict, synth.fill_module_) or
    replaced - the key of the weight packs and of the step-invariant caches.  The tensors are collected ONCE (the recursive
    `parameters()` walk costs 0.5 ms on the 282 tensors of the CMDM and ran three times per sampling call: most of a short loop's fixed
    cost) as (owning dict, name, tensor) triples; every call checks that each slot still holds the SAME tensor object at the same storage
    (a child's `.to()`, `load_state_dict(assign=True)` or `layer.weight = nn.Parameter(...)` replace tensors behind the top-level module's
    back: the list is rebuilt and the version jumps), then sums the in-place version counters."""
    flat = module.__dict__.get("_afm_flat")
    gen = module.__dict__.get("_afm_flat_gen", 0)
    if flat is not None:
        for owner, name, t, ptr in flat:
            if owner.get(name) is not t or t.data_ptr() != ptr:
                flat = None
                break
    if flat is None:
        flat = []
        for m in module.modules():
            for d in (m._parameters, m._buffers):
                for name, t in d.items():
                    if t is not None:
                        flat.append((d, name, t, t.data_ptr()))
        gen += 1
        module.__dict__["_afm_flat"], module.__dict__["_afm_flat_gen"] = flat, gen
    v = len(flat) + (gen << 40)
    for _, _, t, _ in flat:
        v += t._version
    return v


class _FlatParamsMixin:
    """Invalidates the cached tensor lists of `_param_version` (on this module and every submodule) when tensors may be replaced."""

    def _drop_flat_params(self):
        for m in self.modules():
            m.__dict__.pop("_afm_flat", None)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._drop_flat_params()
        if "_pack" in self.__dict__:
            self._pack = None                       # device pointers of the C-ABI weight pack are stale after .to() / .cuda()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._drop_flat_params()
        if "_pack" in self.__dict__:
            self._pack = None
        return out


def _dist_rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def drop_seed(initial_seed: int, drop_calls: int, rank: int = 0) -> int:
    """The 64-bit seed of one training forward's dropout masks: torch's initial seed, advanced per forward pass with dropout (every pass
    draws fresh masks) and per rank (every rank draws its own), modulo 2^64.  Pure: the masks of a pass are a function of this seed, the
    mask id and the element (csrc/common.h DropKey)."""
    return (initial_seed + 0x9E3779B97F4A7C15 * drop_calls + 0xD1B54A32D192ED03 * rank) & (2**64 - 1)


class LoopExtras(NamedTuple):
    """The ``_guidance`` of `CMDM.afm_native_loop`: what only this denoiser's native loop takes (a plain tuple in this order serves too).
    ``cfg`` / ``branch_streams``: GuidedCMDM's afm_cfg_args or afm_cfg2_args and its branch-stream switch.  ``guide``: an
    afm.diffusion.ContactGuidance (afm_cmdm_guide_loop_range), JointTargets or MotionGuidance (afm_cmdm_motion_guide_loop_range: the step's
    gradient the sum of the terms that have started), a SceneClearance or a MotionGuidance that carries one
    (afm_cmdm_scene_guide_loop_range), a FootGrounding or a MotionGuidance that carries one (afm_cmdm_ground_guide_loop_range; no stitched
    chain takes a grounding) - the gradient at every guided step's x_t is computed on the sub-batch's stream and
    enters the update launch; the loop runs in the separate-update form like an imputing one, and steps before the guidance starts launch
    what an imputing loop launches.  ``stitch``: an afm.diffusion.Stitch - the batch rows are overlapping windows of long motions and
    every step's update launch gives the frames two windows share one pred_xstart (afm_cmdm_stitch_loop_range, every deterministic
    form; the separate-update form; sub-batches are cut over long motions).  With ``stitch`` the one ``guide`` taken is an
    afm.diffusion.LongGuidance on the same geometry (afm_cmdm_long_guide_loop_range: the terms on the joined long motions; one that carries
    a SceneClearance: afm_cmdm_long_scene_guide_loop_range)."""
    cfg: object = None
    branch_streams: bool = False
    guide: object = None
    stitch: object = None


class LoopPlan(NamedTuple):
    """One form's native call by names: the C entry, its workspace sizer and the sizer's arguments behind (w, B, L, streams), the form's
    part of the workspace key, the entry's arguments between frame_mask and B.  A slot names a value of the call; None is a NULL."""
    entry: str
    sizer: str
    size_slots: tuple
    key: tuple
    slots: tuple


def plan_loop_call(update: str, guidance: str = "none", impute: bool = False, term: str = "none", stitch: bool = False) -> LoopPlan:
    """The entry a chain reaches: ``update`` "ddpm" / "ddim" / "dpm", ``guidance`` "none" / "cfg" (one scale) / "cfg2" (two), with or without
    ``impute``, ``term`` "none" / "contact" (a bare ContactGuidance) / "motion" (anything that carries targets) / "scene" (anything that carries a
    SceneClearance) / "ground" (anything that carries a FootGrounding) / "long" (a LongGuidance:
    only stitched, only with a deterministic update; the long description takes the guidance's slot and carries the stitch) / "long_scene" (a
    LongGuidance that carries a SceneClearance: the same slots, afm_cmdm_long_scene_guide_loop_range), stitched or not.  By
    priority: a term's entry, the stitched one, the 2M one (each runs every form it is asked for on a workspace of its own size: a history
    buffer, gradient buffers, sub-batches over long motions), then the entries of both updates (cfg2, impute), then one per update."""
    if term in ("long", "long_scene") and not stitch:
        raise ValueError(f"term {term!r} guides stitched windows: no such loop with stitch=False")
    if stitch and (update == "ddpm" or term not in ("none", "long", "long_scene")):
        raise ValueError(f"no stitched loop with update {update!r} and term {term!r}")
    base = {"none": "loop", "cfg": "cfg_loop", "cfg2": "cfg2_loop"}[guidance]
    cfgs = ("cfg" if guidance == "cfg" else None, "cfg2" if guidance == "cfg2" else None)
    known = ("known", "mask") if impute else (None, None)
    ddim = "ddim_rows" if update == "ddim" else None
    ddpm = ("c1", "c2", "sigma") if update == "ddpm" else (None, None, None)
    tail = ("n_steps", "first_step", "seed", "sample_index0")
    own = {"contact": "guide", "motion": "motion_guide", "scene": "scene_guide", "ground": "ground_guide", "long": "long_guide",
           "long_scene": "long_scene_guide"}.get(term, "stitch" if stitch else None)
    if own is not None:                 # both kinds of rows and the 2M rows, one of the three set
        last = ("stitch" if own == "stitch" else "term",)
        return LoopPlan(f"afm_cmdm_{own}_loop_range", f"afm_cmdm_{own}_loop_workspace_bytes", cfgs + last, (own, base),
                        ("noise", "tmap", ddim, "dpm_rows" if update == "dpm" else None) + ddpm + cfgs + known + last + tail)
    if update == "dpm":                 # no noise, no seed
        return LoopPlan("afm_cmdm_dpm_loop_range", "afm_cmdm_dpm_loop_workspace_bytes", cfgs, ("dpm", base),
                        ("tmap", "dpm_rows") + cfgs + known + tail[:2])
    sizer, size = f"afm_cmdm_{base}_workspace_bytes", tuple(c for c in cfgs if c)
    if guidance == "cfg2" or impute:    # both kinds of rows, then cfg (of the entry's own kind) or NULL, known and mask or NULLs
        return LoopPlan("afm_cmdm_cfg2_loop_range" if guidance == "cfg2" else "afm_cmdm_impute_loop_range", sizer, size, (None, base),
                        ("noise", "tmap", ddim) + ddpm + (cfgs[1] or cfgs[0],) + known + tail)
    name = ("cfg_" if size else "") + ("sample" if update == "ddpm" else "ddim")
    return LoopPlan(f"afm_cmdm_{name}_loop_range", sizer, size, (None, base), ("noise", "tmap") + (ddpm if ddim is None else (ddim,)) + size + tail)


def _refuse_loop(ex: LoopExtras, x, model_kwargs, step_noise, ddim_eta, dpm_order) -> None:
    """what `CMDM.afm_native_loop` refuses before it touches the device"""
    if ex.stitch is not None:
        if ddim_eta is None and dpm_order is None:
            raise ValueError("stitched windows need a deterministic update: the ancestral loop draws noise at every step, and the noise of "
                             "the frames two windows share would have to be shared (ddim_eta=0 or dpm_order)")
        if ddim_eta is not None and float(ddim_eta) != 0.0:
            raise ValueError(f"stitched windows need a deterministic update: with ddim_eta = {ddim_eta!r} the step noise of the frames two "
                             "windows share would have to be shared")
        if step_noise is not None:
            raise ValueError("stitched windows take no step_noise: the noise of the frames two windows share would have to be shared")
        if ex.guide is not None and not isinstance(ex.guide, LongGuidance):
            raise ValueError("a cond_fn guidance with stitch= is not built: per-window gradients disagree in the overlaps (LongGuidance "
                             "evaluates the terms on the joined long motion)")
        ex.stitch.check(x.shape[0], x.shape[1])          # (B % S, 2 * ov <= L, the frames)
        if ex.guide is not None and not ex.guide.same_geometry(ex.stitch):
            raise ValueError("the LongGuidance was built on another Stitch than the chain's (windows, overlap, frames, length)")
    elif isinstance(ex.guide, LongGuidance):
        raise ValueError("LongGuidance guides the windows of a stitched chain: pass its Stitch as stitch=")
    if any(k in model_kwargs for k in COND_SWITCHES):
        raise NotImplementedError("condition switches (c_*_mask / c_*_erase) are training-time augmentations; "
                                  "p_sample_loop samples them step by step (p_sample_loop_progressive)")
    if dpm_order is not None and (ddim_eta is not None or step_noise is not None):
        raise ValueError("the DPM-Solver++ loop is deterministic: it takes neither ddim_eta nor step_noise")


@Model.register()
class CMDM(_FlatParamsMixin, TextEncoderMixin, nn.Module):
    """`Model.get('CMDM')(cfg.model, device=...)` - see module docstring."""

    def __init__(self, cfg, *args, **kwargs):
        super().__init__()
        self.device = kwargs["device"] if "device" in kwargs else "cpu"
        self.motion_type = cfg.data_repr
        self.motion_dim = cfg.input_feats
        self.latent_dim = cfg.latent_dim
        self.mask_motion = cfg.mask_motion
        self.arch = cfg.arch
        if self.arch not in ("trans_enc", "trans_dec"):
            raise NotImplementedError(f"arch={self.arch!r}: 'trans_enc' or 'trans_dec' (cmdm.py:65-113)")
        self.time_emb_dim = cfg.time_emb_dim
        self.timestep_embedder = TimestepEmbedder(self.latent_dim, self.time_emb_dim, max_len=1000)

        self.contact_type = cfg.contact_model.contact_type
        self.contact_dim = compute_repr_dimesion(self.contact_type)
        self.planes = list(cfg.contact_model.planes)
        if self.arch == "trans_enc":
            self.contact_adapter = nn.Linear(self.planes[-1], self.latent_dim, bias=True)
        scene_module = SceneMapEncoder if self.arch == "trans_enc" else SceneMapEncoderDecoder
        self.contact_encoder = scene_module(point_feat_dim=self.contact_dim, planes=self.planes, blocks=list(cfg.contact_model.blocks),
                                            num_points=cfg.contact_model.num_points)

        self.text_model_name = cfg.text_model.version
        self.text_max_length = cfg.text_model.max_length
        self.text_feat_dim, self.text_feat_type = lang_feat_dim_type(self.text_model_name)
        self._init_text_encoder()
        self.language_adapter = nn.Linear(self.text_feat_dim, self.latent_dim, bias=True)

        self.motion_adapter = nn.Linear(self.motion_dim, self.latent_dim, bias=True)
        self.positional_encoder = PositionalEncoding(self.latent_dim, dropout=0.1, max_len=5000)
        self.num_layers = list(cfg.num_layers)
        self.num_heads = cfg.num_heads
        # parameter containers with torch's own key names (in_proj_weight, out_proj, linear1/2, norm1/2/3)
        enc_layer = lambda: nn.TransformerEncoderLayer(d_model=self.latent_dim, nhead=cfg.num_heads, dim_feedforward=cfg.dim_feedforward,
                                                       dropout=cfg.dropout, activation="gelu", batch_first=True)
        if self.arch == "trans_enc":
            self.self_attn_layer = nn.TransformerEncoder(enc_layer(), enable_nested_tensor=False, num_layers=sum(self.num_layers))
        else:                                               # trans_dec (cmdm.py:78-113): self-attention stacks interleaved with cross-attention
            self.self_attn_layers, self.kv_mappling_layers, self.cross_attn_layers = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
            for i, n in enumerate(self.num_layers):
                self.self_attn_layers.append(nn.TransformerEncoder(enc_layer(), num_layers=n, enable_nested_tensor=False))
                if i != len(self.num_layers) - 1:
                    self.kv_mappling_layers.append(nn.Sequential(nn.Linear(self.planes[-1 - i], self.latent_dim, bias=True),
                                                                 nn.LayerNorm(self.latent_dim)))
                    self.cross_attn_layers.append(nn.TransformerDecoderLayer(d_model=self.latent_dim, nhead=cfg.num_heads,
                                                                             dim_feedforward=cfg.dim_feedforward, dropout=cfg.dropout,
                                                                             activation="gelu", batch_first=True))
        self.motion_layer = nn.Linear(self.latent_dim, self.motion_dim, bias=True)

        if self.arch == "trans_dec":
            self.afm_native_loop = None      # the fused native sampling loop covers trans_enc; trans_dec samples step by step
        self.dropout_p = float(cfg.dropout)
        self._drop_calls = 0       # forward passes with dropout so far: every pass draws fresh masks
        self.hoist_conditions = True
        # Host-side tuning attributes (plain attributes of the instance; nothing is read from the environment).
        # sub-batches of the native sampling loop, each on its own HIP stream; `loop_streams_auto` caps them at B // 8 (below B = 16 a
        # second stream only adds launches), set it to False to take `loop_streams` literally
        self.loop_streams = 2
        self.loop_streams_auto = True
        self._side_streams: List[torch.cuda.Stream] = []
        self.gemm_tile = 0  # measurement: AFM_TUNE_TILE code forced on the wide encoder GEMMs (0 = library heuristic; bit-neutral)
        self.attn_group_waves = 0  # afm_mha_fwd_grouped workgroup shape (0 = library heuristic; results do not depend on it)
        self.no_l0_cache = False   # measurement: recompute layer 0's q | k | v rows of the condition tokens every step (passed in the pack)
        self.no_riders = False             # measurement: the per-step prologue launch instead of the riders on the step's first / last GEMM (bit-identical)
        self.all_queries = False           # measurement: the last layer's attention computes all T query rows (only the L motion rows are read)
        self.no_ln_fold = False            # measurement: separate LayerNorm launches instead of the statistics-carrying epilogues (afm_linear_args.a_stat ...)
        self.pair_launch = False           # native loop, two sub-batch streams: sub-batch A's out_proj + sub-batch B's linear1 as ONE 128 x 128-tile launch per layer (afm_linear_pair; bit-identical)
        self.fused_layernorm = False       # norm1 / norm2 inside the out_proj / linear2 GEMMs (bit-identical; measured slower on MI355X, profiles/r03_ln_fusion.md)
        self._pack = None          # (version, CmdmWeights, keep-alive tensors)
        self._cond_cache = None    # (key, cond_tokens)
        self._ws: Dict[tuple, torch.Tensor] = {}

    # ------------------------------------------------------------------ weight pack for the C-ABI
    def _weights(self) -> ffi.CmdmWeights:
        ver = (_param_version(self), self.training)
        if self._pack is not None and self._pack[0] == ver:
            return self._stamp(self._pack[1])
        dev = self.motion_adapter.weight.device
        if dev.type != "cuda":
            raise ffi.AfmError("CMDM parameters are on the CPU; move the model to the MI355X (`model.to('cuda')`)")
        keep: List[torch.Tensor] = []

        def P(t: torch.Tensor) -> int:
            t = ffi.f32c(t.detach())
            keep.append(t)
            return t.data_ptr()

        w = ffi.CmdmWeights()
        layers = self.self_attn_layer.layers
        w.d, w.heads, w.ff, w.n_layers = self.latent_dim, self.num_heads, layers[0].linear1.out_features, len(layers)
        w.motion_dim = self.motion_dim
        w.n_cond = 1 + self.contact_encoder.num_groups
        # K = motion_dim = 263 ('h3d') is not a multiple of 16: the weight is zero-padded once per weight version to K = 272 and the loop
        # keeps a padded copy of x_t, so the adapter runs on the bf16-split GEMM like every other layer (padding adds exact zeros)
        kpad = -(-self.motion_dim // 16) * 16
        w.motion_adapter_kpad = kpad if (kpad != self.motion_dim and kpad >= 128) else 0
        maw = self.motion_adapter.weight.detach()
        if w.motion_adapter_kpad:
            maw = torch.nn.functional.pad(maw, (0, kpad - self.motion_dim))
        w.motion_adapter_w, w.motion_adapter_b = P(maw), P(self.motion_adapter.bias)
        w.motion_layer_w, w.motion_layer_b = P(self.motion_layer.weight), P(self.motion_layer.bias)
        w.time_table, w.n_timesteps = P(self.timestep_embedder.table()), self.timestep_embedder.pe.shape[0]
        w.pos_table = P(self.positional_encoder.pe[:, 0, :])
        for i, l in enumerate(layers):
            lw = w.layer[i]
            lw.in_proj_w, lw.in_proj_b = P(l.self_attn.in_proj_weight), P(l.self_attn.in_proj_bias)
            lw.out_proj_w, lw.out_proj_b = P(l.self_attn.out_proj.weight), P(l.self_attn.out_proj.bias)
            lw.lin1_w, lw.lin1_b, lw.lin2_w, lw.lin2_b = P(l.linear1.weight), P(l.linear1.bias), P(l.linear2.weight), P(l.linear2.bias)
            lw.norm1_w, lw.norm1_b, lw.norm2_w, lw.norm2_b = P(l.norm1.weight), P(l.norm1.bias), P(l.norm2.weight), P(l.norm2.bias)
        if not self.training:
            # eval: LayerNorm folded into the linears it feeds (afm_encoder_layer_weights.lin1_wg ...): W' = W * gamma, g = row sums of W',
            # c = b + W beta (afm.fold.ln_fold, the CDM's lat_fold as well) - float64 products rounded once, on the HOST (once per weight
            # version: ~12 MB down, the same up - no eager ATen arithmetic and no vendor BLAS call in a sampling job)
            def ln_fold(lin_w, lin_b, norm):
                return tuple(P(t.float().contiguous().to(dev)) for t in fold.ln_fold(lin_w, lin_b, norm.weight, norm.bias))
            for i, l in enumerate(layers):
                lw = w.layer[i]
                lw.lin1_wg, lw.lin1_g, lw.lin1_c = ln_fold(l.linear1.weight, l.linear1.bias, l.norm1)
                if i > 0:
                    lw.in_proj_wg, lw.in_proj_g, lw.in_proj_c = ln_fold(l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, layers[i - 1].norm2)
            w.motion_layer_wg, w.motion_layer_g, w.motion_layer_c = ln_fold(self.motion_layer.weight, self.motion_layer.bias, layers[-1].norm2)
        self._pack = (ver, w, keep)
        return self._stamp(w)

    def _stamp(self, w: ffi.CmdmWeights) -> ffi.CmdmWeights:
        """Per-call settings of the pack: the host's GEMM arithmetic (afm.ops.set_gemm_split) and bit-neutral tuning fields."""
        w.gemm_arith, w.gemm_arith_min_n = ops.gemm_arith()
        w.attn_group_waves = int(self.attn_group_waves)
        w.flags = (ffi.CMDM_NO_L0_CACHE if self.no_l0_cache else 0) | (ffi.CMDM_FUSED_LN if self.fused_layernorm else 0) | \
            (ffi.CMDM_NO_LN_FOLD if self.no_ln_fold else 0) | (ffi.CMDM_ALL_QUERIES if self.all_queries else 0) | (ffi.CMDM_NO_RIDERS if self.no_riders else 0) | ((int(self.gemm_tile) & 0xF) << 8) | \
            (ffi.CMDM_PAIR_LAUNCH if self.pair_launch else 0)
        return w

    # ------------------------------------------------------------------ step-invariant conditions
    def condition_tokens(self, **kwargs) -> torch.Tensor:
        """[B, 1 + G, d]: language_adapter(text) and contact_adapter(SceneMapEncoder(xyz, contact)),
        positional encoding of sequence positions 1 .. 1+G already added (cmdm.py:134-156,161-162)."""
        tensors = [kwargs.get(k) for k in ("c_pc_xyz", "c_pc_contact", "c_text_feat", "c_cont_emb")]
        extra = (tuple(kwargs["c_text"]) if "c_text" in kwargs and "c_text_feat" not in kwargs else None, _param_version(self))
        if self.hoist_conditions and self._cond_cache is not None and self._cond_cache[0].matches(tensors, extra):
            return self._cond_cache[1]
        with torch.no_grad():           # sampling-side entry point (the training composition never calls it): always the fused inference kernels,
            return self._condition_tokens(tensors, extra, kwargs)      # also when the caller has not disabled autograd itself

    def _condition_tokens(self, tensors, extra, kwargs) -> torch.Tensor:
        text_feat = self.encode_text(kwargs)                                          # [B, text_dim]
        cont_emb = kwargs["c_cont_emb"] if "c_cont_emb" in kwargs else \
            self.contact_encoder(kwargs["c_pc_xyz"], kwargs["c_pc_contact"])           # [B, G, planes[-1]]
        B, G = cont_emb.shape[0], cont_emb.shape[1]
        pe = self.positional_encoder.pe[:, 0, :]
        tok = torch.empty(B, 1 + G, self.latent_dim, device=cont_emb.device, dtype=torch.float32)
        flat = tok.view(B * (1 + G), self.latent_dim)
        ops.linear(text_feat, self.language_adapter.weight, self.language_adapter.bias, rowtab=pe[1:2],
                   out=flat, c_map=(1, 1 + G, 0))
        ops.linear(cont_emb.reshape(B * G, -1), self.contact_adapter.weight, self.contact_adapter.bias, rowtab=pe[2:2 + G],
                   out=flat, c_map=(G, 1 + G, 1))
        self._cond_cache = (HeldKey(tensors, extra), tok) if self.hoist_conditions else None
        return tok

    # ------------------------------------------------------------------ forward
    def forward(self, x, timesteps, **kwargs):
        """x [B, L, motion_dim], timesteps [B] int64, kwargs = batch dict (x_mask, c_text | c_text_feat,
        c_pc_xyz, c_pc_contact, info_* ignored) -> predicted x_0, same shape as x."""
        if self.arch == "trans_dec":
            return self.forward_trans_dec(x, timesteps, **kwargs)
        if torch.is_grad_enabled() and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self.forward_train(x, timesteps, **kwargs)
        if any(k in kwargs for k in COND_SWITCHES):
            # training-time condition switches (datasets/transforms.py:50-106) change the key mask / the embeddings per
            # sample: evaluate through the per-operator composition, which implements them (no autograd, no dropout in eval)
            with torch.no_grad():
                return self.forward_train(x, timesteps, **kwargs)
        ffi.require_gpu(x)
        with torch.no_grad():
            lib = ffi.load()
            x = ffi.f32c(x)
            B, L, _ = x.shape
            w = self._weights()
            cond = self.condition_tokens(**kwargs)
            fm = None
            if self.mask_motion:
                fm = kwargs["x_mask"].to(device=x.device, dtype=torch.uint8).contiguous()
            out = torch.empty_like(x)
            ws = ffi.workspace(self._ws, (B, L, str(x.device)), "afm_cmdm_workspace_bytes", C.byref(w), B, L, device=x.device, single=True)
            t = timesteps.to(device=x.device, dtype=torch.int64).contiguous()
            ffi.check(lib.afm_cmdm_forward(C.byref(w), x.data_ptr(), t.data_ptr(), cond.data_ptr(), ffi.ptr(fm),
                                           out.data_ptr(), None, B, L, ws.data_ptr(), ws.numel(), ffi.stream_of(x)),
                      "afm_cmdm_forward")
        return out

    # ------------------------------------------------------------------ trans_dec variant (per-operator composition, inference)
    def _enc_layer(self, x, layer, key_mask):
        """Post-LN nn.TransformerEncoderLayer (GELU) on [B, T, d]."""
        B, T, d = x.shape
        flat = x.reshape(B * T, d)
        a = ops.mha(ops.linear(flat, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias).view(B, T, 3 * d), key_mask, self.num_heads)
        y = ops.layernorm(ops.linear(a.view(B * T, d), layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, residual=flat),
                          layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
        h = ops.linear(y, layer.linear1.weight, layer.linear1.bias, act=ffi.ACT_GELU)
        return ops.layernorm(ops.linear(h, layer.linear2.weight, layer.linear2.bias, residual=y), layer.norm2.weight, layer.norm2.bias,
                             layer.norm2.eps).view(B, T, d)

    def _dec_layer(self, x, layer, key_mask, kv, mem_mask):
        """Post-LN nn.TransformerDecoderLayer (GELU): self-attention, cross-attention over the memory (kv = its packed K | V
        projections, step-invariant), feed-forward."""
        B, T, d = x.shape
        flat = x.reshape(B * T, d)
        a = ops.mha(ops.linear(flat, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias).view(B, T, 3 * d), key_mask, self.num_heads)
        y = ops.layernorm(ops.linear(a.view(B * T, d), layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, residual=flat),
                          layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
        ca = layer.multihead_attn
        q = ops.linear(y, ca.in_proj_weight[:d], ca.in_proj_bias[:d]).view(B, T, d)
        c = ops.mha_cross(q, kv, mem_mask, self.num_heads)
        y = ops.layernorm(ops.linear(c.view(B * T, d), ca.out_proj.weight, ca.out_proj.bias, residual=y), layer.norm2.weight, layer.norm2.bias,
                          layer.norm2.eps)
        h = ops.linear(y, layer.linear1.weight, layer.linear1.bias, act=ffi.ACT_GELU)
        return ops.layernorm(ops.linear(h, layer.linear2.weight, layer.linear2.bias, residual=y), layer.norm3.weight, layer.norm3.bias,
                             layer.norm3.eps).view(B, T, d)

    def _trans_dec_memories(self, kwargs):
        """Step-invariant part of trans_dec: SceneMapEncoderDecoder features -> kv_mappling (Linear + LayerNorm) -> the packed
        K | V projections of every cross-attention layer; cached per scene batch like the trans_enc condition tokens."""
        tensors = [kwargs.get(k) for k in ("c_pc_xyz", "c_pc_contact", "c_pc_erase")]
        extra = ("trans_dec", _param_version(self))
        if self.hoist_conditions and self._cond_cache is not None and self._cond_cache[0].matches(tensors, extra):
            return self._cond_cache[1]
        feats = self.contact_encoder(kwargs["c_pc_xyz"], kwargs["c_pc_contact"])                     # [x4, x3, x2, x1]
        d, out = self.latent_dim, []
        for i, layer in enumerate(self.cross_attn_layers):
            mem = feats[i]
            if "c_pc_erase" in kwargs:
                mem = mem * (1.0 - kwargs["c_pc_erase"].to(mem.device).float().reshape(-1, 1, 1))
            B, n, c = mem.shape
            km = self.kv_mappling_layers[i]
            m = ops.layernorm(ops.linear(mem.reshape(B * n, c), km[0].weight, km[0].bias), km[1].weight, km[1].bias, km[1].eps)
            ca = layer.multihead_attn
            out.append(ops.linear(m, ca.in_proj_weight[d:], ca.in_proj_bias[d:]).view(B, n, 2 * d))
        self._cond_cache = (HeldKey(tensors, extra), out) if self.hoist_conditions else None
        return out

    def forward_trans_dec(self, x, timesteps, **kwargs):
        """CMDM.forward, `trans_dec` branch (cmdm.py:171-191): tokens [time | text | motion]; five self-attention stacks
        interleaved with four decoder layers whose memories are the multi-scale scene features (N/64 ... N points)."""
        ffi.require_gpu(x)
        if torch.is_grad_enabled() and (self.training or any(p.requires_grad for p in self.parameters())):
            return self._forward_trans_dec_train(x, timesteps, **kwargs)
        with torch.no_grad():
            x = ffi.f32c(x)
            B, L, _ = x.shape
            d, dev, T = self.latent_dim, x.device, 2 + L
            kvs = self._trans_dec_memories(kwargs)
            pe = self.positional_encoder.pe[:, 0, :]
            tok = torch.empty(B, T, d, device=dev, dtype=torch.float32)
            flat = tok.view(B * T, d)
            t_idx = timesteps.to(device=dev, dtype=torch.int64)
            tok[:, 0, :] = self.timestep_embedder.table()[t_idx] + pe[0]
            text = self.encode_text(kwargs)
            if "c_text_erase" in kwargs:
                text = text * (1.0 - kwargs["c_text_erase"].to(dev).float().reshape(B, 1))
            ops.linear(text, self.language_adapter.weight, self.language_adapter.bias, rowtab=pe[1:2], out=flat, c_map=(1, T, 1))
            ops.linear(x.view(B * L, -1), self.motion_adapter.weight, self.motion_adapter.bias, rowtab=pe[2:2 + L], out=flat, c_map=(L, T, 2))
            key_mask = None
            if self.mask_motion:
                tm = kwargs["c_text_mask"].to(dev).bool().reshape(B, 1) if "c_text_mask" in kwargs else torch.zeros(B, 1, dtype=torch.bool, device=dev)
                key_mask = torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev), tm, kwargs["x_mask"].to(dev).bool().reshape(B, L)], dim=1)
            for i, stack in enumerate(self.self_attn_layers):
                for layer in stack.layers:
                    tok = self._enc_layer(tok, layer, key_mask)
                if i != len(self.self_attn_layers) - 1:
                    mem_mask = None
                    if "c_pc_mask" in kwargs:
                        mem_mask = kwargs["c_pc_mask"].to(dev).bool().reshape(B, 1).repeat(1, kvs[i].shape[1])
                    tok = self._dec_layer(tok, self.cross_attn_layers[i], key_mask, kvs[i], mem_mask)
            return ops.linear(tok.view(B * T, d), self.motion_layer.weight, self.motion_layer.bias, a_map=(L, T, 2), rows=B * L).view(B, L, self.motion_dim)

    def _forward_trans_dec_train(self, x, timesteps, **kwargs):
        """The `trans_dec` branch under autograd (cmdm.py:171-191 reached from utils/training.py:140-152): the same graph from differentiable
        HIP operators - the multi-scale SceneMapEncoderDecoder, kv_mappling (Linear + LayerNorm), the self-attention stacks
        (AG.encoder_layer) and the decoder layers (AG.decoder_layer: self-attention, cross-attention over a memory, feed-forward).  Train
        mode applies the reference's dropouts with counter-hash masks."""
        x = ffi.f32c(x)
        B, L, _ = x.shape
        d, dev, T = self.latent_dim, x.device, 2 + L
        p_drop = self.dropout_p if self.training else 0.0
        p_pe = float(self.positional_encoder.dropout.p) if self.training else 0.0
        self._drop_calls += 1
        seed = drop_seed(torch.initial_seed(), self._drop_calls, _dist_rank())
        # memories: [x4, x3, x2, x1] -> kv_mappling (the K | V projections live inside the decoder layer operator)
        feats = self.contact_encoder(kwargs["c_pc_xyz"], kwargs["c_pc_contact"])
        mems = []
        for i in range(len(self.cross_attn_layers)):
            mem = feats[i]
            if "c_pc_erase" in kwargs:
                mem = mem * (1.0 - kwargs["c_pc_erase"].to(dev).float().reshape(-1, 1, 1))
            km = self.kv_mappling_layers[i]
            Bm, n, c = mem.shape
            mems.append(AG.layer_norm(AG.linear(mem.reshape(Bm * n, c), km[0].weight, km[0].bias), km[1]).view(Bm, n, d))
        # tokens [time | text | motion] + positional encoding (+ dropout)
        time_emb = self.timestep_embedder.run(timesteps.to(device=dev, dtype=torch.int64)).view(B, 1, d)
        text = self.encode_text(kwargs)
        if "c_text_erase" in kwargs:
            text = text * (1.0 - kwargs["c_text_erase"].to(dev).float().reshape(B, 1))
        text_emb = AG.linear(text, self.language_adapter.weight, self.language_adapter.bias).view(B, 1, d)
        h = AG.linear(x, self.motion_adapter.weight, self.motion_adapter.bias)
        tok = AG.posenc_dropout(torch.cat([time_emb, text_emb, h], dim=1), self.positional_encoder.pe[:T, 0, :], (p_pe, seed, 1))
        key_mask = None
        if self.mask_motion:
            tm = kwargs["c_text_mask"].to(dev).bool().reshape(B, 1) if "c_text_mask" in kwargs else torch.zeros(B, 1, dtype=torch.bool, device=dev)
            key_mask = torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev), tm, kwargs["x_mask"].to(dev).bool().reshape(B, L)], dim=1)
        did = 16
        for i, stack in enumerate(self.self_attn_layers):
            for layer in stack.layers:
                tok = AG.encoder_layer(tok, layer, key_mask, self.num_heads, (p_drop, seed, did))
                did += 4
            if i != len(self.self_attn_layers) - 1:
                mem_mask = None
                if "c_pc_mask" in kwargs:
                    mem_mask = kwargs["c_pc_mask"].to(dev).bool().reshape(B, 1).repeat(1, mems[i].shape[1])
                tok = AG.decoder_layer(tok, mems[i], self.cross_attn_layers[i], key_mask, mem_mask, self.num_heads, (p_drop, seed, did))
                did += 6
        out = AG.linear(tok.view(B * T, d), self.motion_layer.weight, self.motion_layer.bias, a_map=(L, T, 2), rows=B * L)
        return out.view(B, L, self.motion_dim)

    # ------------------------------------------------------------------ training forward (autograd tape over HIP kernels)
    def forward_train(self, x, timesteps, **kwargs):
        """Same function as `forward`, composed from differentiable HIP ops (afm.autograd) so that
        `diffusion.training_losses(...)['loss'].mean().backward()` (utils/training.py:140-152) fills `.grad` of the
        transformer trunk, the adapters and the TimestepEmbedder.  Train mode applies the reference's dropouts
        (PositionalEncoding 0.1, cfg.dropout inside every encoder layer incl. attention probabilities) with
        counter-hash masks; the SceneMapEncoder trains through afm.autograd_points (batch-statistics BatchNorm) unless
        its parameters are frozen, in which case the fused inference kernels compute it."""
        ffi.require_gpu(x)
        x = ffi.f32c(x)
        B, L, _ = x.shape
        d, dev = self.latent_dim, x.device
        p_drop = self.dropout_p if self.training else 0.0
        p_pe = float(self.positional_encoder.dropout.p) if self.training else 0.0
        self._drop_calls += 1
        seed = drop_seed(torch.initial_seed(), self._drop_calls, _dist_rank())

        # time token: pe[t] -> Linear -> SiLU -> Linear (modules.py:48-53)
        time_emb = self.timestep_embedder.run(timesteps.to(device=dev, dtype=torch.int64)).view(B, 1, d)
        masks = [torch.zeros(B, 1, dtype=torch.bool, device=dev)]
        # text token (cmdm.py:134-146)
        text_feat = self.encode_text(kwargs)
        text_mask = torch.zeros(B, 1, dtype=torch.bool, device=dev)
        if "c_text_mask" in kwargs:
            text_mask = text_mask | kwargs["c_text_mask"].to(dev).bool().reshape(B, 1)
        if "c_text_erase" in kwargs:
            text_feat = text_feat * (1.0 - kwargs["c_text_erase"].to(dev).float().reshape(B, 1))
        text_emb = AG.linear(text_feat, self.language_adapter.weight, self.language_adapter.bias).view(B, 1, d)
        masks.append(text_mask)
        # contact tokens (cmdm.py:148-156)
        # SceneMapEncoder: differentiable passes (batch-statistics BatchNorm in train mode) when it has trainable
        # parameters, the fused inference kernels when it is frozen
        cont = kwargs["c_cont_emb"] if "c_cont_emb" in kwargs else self.contact_encoder(kwargs["c_pc_xyz"], kwargs["c_pc_contact"])
        G = cont.shape[1]
        cont_mask = torch.zeros(B, G, dtype=torch.bool, device=dev)
        if "c_pc_mask" in kwargs:
            cont_mask = cont_mask | kwargs["c_pc_mask"].to(dev).bool().reshape(B, 1)
        if "c_pc_erase" in kwargs:
            cont = cont * (1.0 - kwargs["c_pc_erase"].to(dev).float().reshape(B, 1, 1))
        cont_emb = AG.linear(cont, self.contact_adapter.weight, self.contact_adapter.bias)
        masks.append(cont_mask)
        # motion tokens, concatenation, positional encoding + dropout (cmdm.py:159-162)
        h = AG.linear(x, self.motion_adapter.weight, self.motion_adapter.bias)
        T = 2 + G + L
        tok = torch.cat([time_emb, text_emb, cont_emb, h], dim=1)
        tok = AG.posenc_dropout(tok, self.positional_encoder.pe[:T, 0, :], (p_pe, seed, 1))
        key_mask = None
        if self.mask_motion:
            key_mask = torch.cat(masks + [kwargs["x_mask"].to(dev).bool().reshape(B, L)], dim=1)
        for i, layer in enumerate(self.self_attn_layer.layers):
            tok = AG.encoder_layer(tok, layer, key_mask, self.num_heads, (p_drop, seed, 16 + 4 * i))
        # output projection on the motion tokens only (cmdm.py:169,195)
        out = AG.linear(tok.view(B * T, d), self.motion_layer.weight, self.motion_layer.bias, a_map=(L, T, T - L), rows=B * L)
        return out.view(B, L, self.motion_dim)

    # ------------------------------------------------------------------ native sampling loop
    def afm_native_loop(self, diffusion, x, model_kwargs, *, step_noise=None, seed=0, sample_index0=0, progress=False, snapshots=None,
                        clip_denoised=False, ddim_eta: Optional[float] = None, impute=None, _guidance=None, dpm_order: Optional[int] = None):
        """Whole p_sample_loop on the device: x holds x_T on entry, returns the final sample.  ``clip_denoised``: pred_xstart clamped to
        [-1, 1] inside the fused DDPM update (the reference's default argument; test.py passes False).  ``ddim_eta`` not None: the
        ddim_sample_loop with that eta instead (afm_cmdm_ddim_loop_range: the same launches, the DDIM update in the same epilogue).  ``progress`` (test.py:85 passes
        True) splits the chain into ~50 native slices (afm_cmdm_sample_loop_range) and advances a tqdm bar between them; the
        result is bit-identical to the unsliced loop.  ``impute``: an afm.diffusion.Impute - its known values are written over every step's
        pred_xstart before the clamp, inside the loop's update launch (afm_cmdm_impute_loop_range, all four forms).  ``dpm_order`` (1 or
        2) not None: dpm_solver_sample_loop instead (afm_cmdm_dpm_loop_range, every form: the eta = 0 DDIM loop's launches with the
        DPM-Solver++ update and one history buffer per sub-batch in the workspace; no noise: ``step_noise`` is refused, ``seed`` unused;
        sliced chains stay bit-identical because every range call of one chain runs on the same workspace).  ``_guidance``: what only this
        denoiser's loops take (not a caller's argument; the public keywords are the CDM's, name for name) - a `LoopExtras`, or a tuple in
        its order.  What the loop refuses: `_refuse_loop`; which entry a form reaches and how its arguments lie: `plan_loop_call`."""
        ex = LoopExtras() if _guidance is None else LoopExtras(*_guidance)
        _refuse_loop(ex, x, model_kwargs, step_noise, ddim_eta, dpm_order)
        lib = ffi.load()
        ffi.require_gpu(x)
        with torch.no_grad():
            x = ffi.f32c(x)
            B, L, _ = x.shape
            if impute is not None:
                impute.check(x)
            w = self._weights()
            if clip_denoised:
                w.flags |= ffi.CMDM_CLIP_X0                  # per call: _stamp() rewrites the flags on the next _weights()
            cfg = ex.cfg
            term, term_keep, kind, kind_key = None, None, "none", None
            gk_of = None                    # the description whose gk rows a range call sets
            if ex.guide is not None:
                both = MotionGuidance(targets=ex.guide) if isinstance(ex.guide, JointTargets) else \
                    MotionGuidance(clearance=ex.guide) if isinstance(ex.guide, SceneClearance) else \
                    MotionGuidance(feet=ex.guide) if isinstance(ex.guide, FootGrounding) else ex.guide
                term, term_fm, term_keep = both.describe(x, model_kwargs, diffusion)
                gk_of = term
                if isinstance(both, ContactGuidance):      # a bare contact term keeps its own entry
                    kind, kind_key = "contact", (term.K, term.N, bool(term.h3d))
                else:                                                # anything that carries targets: the sum's entry (a LongGuidance: its own)
                    ct, tg = both.contact, both.targets
                    kind, kind_key = "motion", (None if ct is None else (ct.K, model_kwargs["c_pc_xyz"].shape[1]), None if tg is None else tg.K,
                                                (ct or tg or getattr(both, "clearance", None) or getattr(both, "feet", None)).joints is not None)
                    sc = getattr(both, "clearance", None)
                    if sc is not None:                               # anything that carries a clearance: the scene entry
                        kind, kind_key = "scene", kind_key + (sc.K, model_kwargs["c_pc_xyz"].shape[1])
                    ft = getattr(both, "feet", None)
                    if ft is not None:                               # anything that carries a grounding: the ground entry, a kind of its own
                        kind, kind_key = "ground", kind_key + (None if sc is None else "scene", ft.K)
                if isinstance(both, LongGuidance):         # no frame mask: validity is the geometry; gk rows per window, on its terms
                    base = term if both.clearance is None else term.base.contents          # (a clearance: the long description is the base)
                    kind, gk_of, long_key = "long" if both.clearance is None else "long_scene", base.terms.contents, kind_key + (base.frames,)
                else:
                    term.frame_mask = ffi.ptr(term_fm)      # the guidance masks by x_mask also where the model does not (mask_motion=False)
                gk_rows = diffusion.guidance_rows(x.device, "mean" if ddim_eta is None and dpm_order is None else "x0", B)
            cond = self.condition_tokens(**model_kwargs)
            if tuple(cond.shape[:2]) != (B, w.n_cond):       # (e.g. a cloud of fewer points than contact_model.num_points: the loop reads n_cond rows per sample)
                raise ValueError(f"the conditions give {tuple(cond.shape[:2])} tokens, the model's layout has ({B}, {w.n_cond})")
            fm = model_kwargs["x_mask"].to(device=x.device, dtype=torch.uint8).contiguous() if self.mask_motion else None
            tables = ffi.LoopTables(self, diffusion, B, x.device, ddim_eta, dpm_order)
            # sub-batch streams fill the wave-quantisation tails of B >= 16 launches; below that every launch is latency-bound and a
            # second stream only adds launches (B = 4: 1311 steps/s on one stream vs 1159 on two, profiles/r02_small_batch.md)
            nsub = max(1, min(int(self.loop_streams), B // 8 if self.loop_streams_auto else B))
            st = st_keep = None
            if ex.stitch is not None:          # sub-batches are cut over long motions: a window and its neighbour share one
                st, st_keep = ex.stitch.describe(x.device)
                nsub = max(1, min(nsub, B // ex.stitch.windows))
                kind_key = (st.windows, st.overlap) + (long_key if kind in ("long", "long_scene") else ())
            self._side_streams = ffi.stream_pool(x.device, nsub)          # process-wide pool (hardware queues are few: ffi.stream_pool)
            handles = (C.c_void_p * nsub)(*[s.cuda_stream for s in self._side_streams[:nsub]])
            # ex.cfg (GuidedCMDM only): the afm_cfg_args of a guided loop (afm_cmdm_cfg_*_loop_range; scales already [B] on the device)
            two = isinstance(cfg, ffi.Cfg2Args)             # one scale per condition: three branches (afm_cmdm_cfg2_loop_range)
            if two and ex.branch_streams:
                raise ValueError("branch streams are not built for the two-scale guided loop (three branches)")
            if ex.branch_streams:
                # the unconditioned branch of every sub-batch on a pool stream of its own: 2 * nsub <= 4 streams (the process has four hardware
                # queues; more streams than queues serialise, ffi.stream_pool)
                nsub = min(nsub, 2)
                pool = ffi.stream_pool(x.device, 2 * nsub)
                self._side_streams = pool
                handles = (C.c_void_p * nsub)(*[s.cuda_stream for s in pool[:nsub]])
                branch_handles = (C.c_void_p * nsub)(*[s.cuda_stream for s in pool[nsub:2 * nsub]])
                cfg.branch_streams = C.cast(branch_handles, C.POINTER(C.c_void_p))
            # the form's entry, sizer and argument layout, and the values its slots name.  The workspace key: the plan's, what of the
            # guidance and of the term / the windows sizes the buffer; every range call of a chain runs on the one buffer
            plan = plan_loop_call("dpm" if tables.dpm is not None else "ddpm" if tables.ddim is None else "ddim",
                                  "none" if cfg is None else "cfg2" if two else "cfg", impute is not None, kind, st is not None)
            cfg_key = () if cfg is None else (cfg.first, cfg.flags) if two else (cfg.drop_text, cfg.drop_pc, cfg.flags)
            ref = lambda s: None if s is None else C.byref(s)
            fill = lambda slots, v: [None if s is None else v[s] for s in slots]
            known, mask = ffi.impute_ptrs(impute)
            values = {"cfg": ref(cfg), "cfg2": ref(cfg), "known": known, "mask": mask, "term": ref(term), "stitch": ref(st),
                      "seed": seed & (2**64 - 1), "sample_index0": sample_index0}
            ws = ffi.workspace(self._ws, (plan.key, cfg_key, kind_key, B, L, nsub, str(x.device)), plan.sizer, C.byref(w), B, L, nsub,
                               *fill(plan.size_slots, values), device=x.device, single=True)
            head = (C.byref(w), x.data_ptr(), cond.data_ptr(), ffi.ptr(fm))
            tail = (B, L, tables.sched.data_ptr(), ws.data_ptr(), ws.numel(), nsub if nsub > 1 else 0, handles if nsub > 1 else None,
                    ffi.stream_of(x))
            n = tables.n

            def call(j0, j1, nz):       # executed steps j0..j1-1 = timestep indices n-j1 .. n-1-j0
                lo = n - j1
                if gk_of is not None:         # the gk rows of the slice
                    gk_of.gk = gk_rows[lo:].data_ptr()
                step = dict(values, noise=nz, tmap=tables.tmap(lo), n_steps=j1 - j0, first_step=j0, **tables.named(lo))
                ffi.check(getattr(lib, plan.entry)(*head, *fill(plan.slots, step), *tail), plan.entry)

            step_noise = ffi.run_native_loop(x, n, step_noise, progress, snapshots, call)
            # keep scratch alive until the stream has consumed it
            self._last_loop_scratch = (tables.keep(), step_noise, cond, fm, ex, impute, term_keep, st, st_keep)
        return x


# ---------------------------------------------------------------------- classifier-free guidance
GUIDANCE_DROPS = ("text", "pc")


class GuidedCMDM(nn.Module):
    """Classifier-free guided denoiser over a CMDM:  x0_guided = x0_u + scale[b] * (x0_c - x0_u)  (float32, this association).

    The reference trains every motion task with condition dropout (datasets/transforms.py:46-92 sets c_text_mask / c_pc_mask with
    probability 0.1; cmdm.py:142-166 turns them into key-padding masks), so a CMDM checkpoint is a guidance model.  ``x0_c`` is the ordinary
    forward, ``x0_u`` the forward of the same x_t, t, x_mask with the conditions named in ``drop`` masked as training masks them.
    ``scale``: a float or a [B] tensor.  Calling the wrapper is a denoiser (``wrapper(x, t, **kwargs) -> x0_guided``): both fused forwards and
    the combine kernel in one native call (afm_cmdm_cfg_forward), so ``diffusion.p_sample_loop(wrapper, shape, model_kwargs=...)`` and
    ``ddim_sample_loop`` work unchanged; it exposes ``afm_native_loop``, so they run the guided native loop under the conditions of the
    unguided one.  With every condition dropped the unconditioned branch runs in its compact form (no condition rows at all);
    ``force_masked=True`` (measurement) keeps the masked full-length form.  ``branch_streams=True`` (measurement; bit-identical) queues
    the unconditioned branch of a native loop on a second stream per sub-batch instead of behind the conditioned branch.

    One scale per condition: ``scale={"pc": 1.5, "text": 5.0}`` - a mapping with exactly the keys "text" and "pc", each value a float or a
    [B] tensor; the insertion order names (first, second).  Three evaluations, u (both dropped), a (only `first` kept), c (nothing dropped):

        x0_guided = (u + s_first[b] * (a - u)) + s_second[b] * (c - a)          (float32, this association)

    ``drop`` stays at its default, ``force_masked`` applies to u, branch streams are not built for three branches (ValueError).
    ``branches`` then returns (x0_c, x0_a, x0_u, x0_guided).  Equal scales are not bit-equal to the single-scale form."""

    def __init__(self, model: "CMDM", scale, drop=GUIDANCE_DROPS, *, force_masked: bool = False, branch_streams: bool = False):
        super().__init__()
        if not isinstance(model, CMDM):
            raise TypeError(f"GuidedCMDM wraps a CMDM, not {type(model).__name__} (the CDM never reads the condition switches)")
        if model.arch == "trans_dec":
            raise NotImplementedError("classifier-free guidance is built for arch='trans_enc' only")
        if not model.mask_motion:
            raise ValueError("classifier-free guidance needs mask_motion=True: with mask_motion=False the condition masks are no-ops (cmdm.py:165)")
        drop = (drop,) if isinstance(drop, str) else tuple(drop)
        if not drop:
            raise ValueError("GuidedCMDM: `drop` is empty - name at least one of " + repr(GUIDANCE_DROPS))
        unknown = [d for d in drop if d not in GUIDANCE_DROPS]
        if unknown:
            raise ValueError(f"GuidedCMDM: unknown condition(s) {unknown} in `drop`; valid names: {GUIDANCE_DROPS}")
        self.order = None                     # (first, second) with one scale per condition
        if isinstance(scale, Mapping):
            if len(scale) != len(GUIDANCE_DROPS) or set(scale) != set(GUIDANCE_DROPS):
                raise ValueError(f"GuidedCMDM: a `scale` mapping has exactly the keys {GUIDANCE_DROPS}, got {list(scale)}")
            if set(drop) != set(GUIDANCE_DROPS):
                raise ValueError(f"GuidedCMDM: with one scale per condition `drop` stays at its default {GUIDANCE_DROPS}, got {drop}")
            if branch_streams:
                raise ValueError("GuidedCMDM: branch streams are not built for one scale per condition (three branches)")
            self.order = tuple(scale)
            scale = {k: scale_value(v, "GuidedCMDM", "shape ") for k, v in scale.items()}
        else:
            scale = scale_value(scale, "GuidedCMDM", "shape ")
        self.model, self.scale, self.drop, self.force_masked = model, scale, tuple(sorted(set(drop))), bool(force_masked)
        self.branch_streams = bool(branch_streams)
        self._scales: Dict[tuple, torch.Tensor] = {}

    @property
    def motion_dim(self) -> int:
        return self.model.motion_dim

    def _scale_row(self, which, B: int, device) -> torch.Tensor:
        """the [B] scale tensor (`which`: a condition's name with one scale per condition, else None), built once per (B, device)"""
        key = (which, B, str(device))
        if key not in self._scales:
            self._scales[key] = scale_row(self.scale if which is None else self.scale[which], B, device, "GuidedCMDM",
                                          "`scale`" if which is None else f"`scale[{which!r}]`")
        return self._scales[key]

    def _cfg(self, B: int, device):
        """afm_cfg_args (one scale per condition: afm_cfg2_args) for a batch of B on `device`; the [B] scale tensors are kept on the wrapper."""
        flags = ffi.CFG_FORCE_MASKED if self.force_masked else 0
        if self.order is not None:
            first, second = self.order
            return ffi.Cfg2Args(self._scale_row(first, B, device).data_ptr(), self._scale_row(second, B, device).data_ptr(),
                                GUIDANCE_DROPS.index(first), flags)
        return ffi.CfgArgs(self._scale_row(None, B, device).data_ptr(), int("text" in self.drop), int("pc" in self.drop), flags)

    @staticmethod
    def _no_switches(kwargs) -> None:
        used = [k for k in COND_SWITCHES if k in kwargs]
        if used:
            raise ValueError(f"GuidedCMDM sets the condition masks itself: remove {used} from model_kwargs")

    def branches(self, x, timesteps, **kwargs):
        """(x0_c, x0_u, x0_guided) of one guided evaluation - afm_cmdm_cfg_forward: the conditioned branch is CMDM.forward's launches.
        One scale per condition: (x0_c, x0_a, x0_u, x0_guided) - afm_cmdm_cfg2_forward."""
        self._no_switches(kwargs)
        m = self.model
        if m.training:
            raise RuntimeError("GuidedCMDM samples in eval mode: call model.eval() first")
        ffi.require_gpu(x)
        with torch.no_grad():
            lib = ffi.load()
            x = ffi.f32c(x)
            B, L, _ = x.shape
            cfg = self._cfg(B, x.device)
            w = m._weights()
            cond = m.condition_tokens(**kwargs)
            fm = kwargs["x_mask"].to(device=x.device, dtype=torch.uint8).contiguous()
            two = self.order is not None
            name = "afm_cmdm_cfg2" if two else "afm_cmdm_cfg"
            out = torch.empty((4 if two else 3,) + tuple(x.shape), dtype=torch.float32, device=x.device)
            ws = ffi.workspace(m._ws, ("cfg2" if two else "cfg", B, L, str(x.device)), name + "_workspace_bytes", C.byref(w), B, L,
                               device=x.device, single=True)
            t = timesteps.to(device=x.device, dtype=torch.int64).contiguous()
            ffi.check(getattr(lib, name + "_forward")(C.byref(w), x.data_ptr(), t.data_ptr(), cond.data_ptr(), fm.data_ptr(), C.byref(cfg),
                                                      *[o.data_ptr() for o in out], B, L, ws.data_ptr(), ws.numel(), ffi.stream_of(x)),
                      name + "_forward")
        return tuple(out)

    def forward(self, x, timesteps, **kwargs):
        return self.branches(x, timesteps, **kwargs)[-1]

    def afm_native_loop(self, diffusion, x, model_kwargs, *, impute=None, dpm_order: Optional[int] = None, contact_guide=None, stitch=None,
                        **kw):
        """The guided native loop (afm_cmdm_cfg_sample_loop_range / afm_cmdm_cfg_ddim_loop_range; with ``impute``: the guided form of
        afm_cmdm_impute_loop_range; one scale per condition: afm_cmdm_cfg2_loop_range, every form; ``dpm_order``: the guided forms of
        afm_cmdm_dpm_loop_range; ``contact_guide``: the guided forms of afm_cmdm_guide_loop_range; ``stitch``: the guided forms of
        afm_cmdm_stitch_loop_range, each window combined with its own scales; with a LongGuidance as ``contact_guide``:
        afm_cmdm_long_guide_loop_range): CMDM.afm_native_loop's arguments."""
        self._no_switches(model_kwargs)
        if self.model.training:
            raise RuntimeError("GuidedCMDM samples in eval mode: call model.eval() first")
        cfg = self._cfg(x.shape[0], x.device)          # (a [B] scale of the wrong length is refused here)
        ffi.require_gpu(x)
        return self.model.afm_native_loop(diffusion, x, model_kwargs, _guidance=LoopExtras(cfg, self.branch_streams, contact_guide, stitch),
                                          impute=impute, dpm_order=dpm_order, **kw)
