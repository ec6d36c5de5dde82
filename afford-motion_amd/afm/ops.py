"""Tensor-level wrappers of the primitive C-ABI entry points (include/afm_hip.h).

Each function mirrors the PyTorch call the reference makes at that point of the path
(F.linear, F.layer_norm, the attention inside nn.TransformerEncoderLayer, the DDPM update),
takes/returns torch tensors on the GPU and enqueues the HIP kernel on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import ffi

RowMap = Tuple[int, ...]   # (group, stride, offset[, skip_after, skip]): row r -> (r // group) * stride + offset + j + (skip if j >= skip_after), j = r % group


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: int = ffi.ACT_NONE,
           act_post: int = ffi.ACT_NONE,
           scale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           rowtab: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           rows: Optional[int] = None, a_map: Optional[RowMap] = None, c_map: Optional[RowMap] = None,
           rowdot_w: Optional[torch.Tensor] = None, rowdot_out: Optional[torch.Tensor] = None, store: bool = True,
           ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None, ln_out: Optional[torch.Tensor] = None,
           ln_counters: Optional[torch.Tensor] = None, stat_out: Optional[torch.Tensor] = None,
           a_stat: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
           res_stat: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, ln_eps: float = 1e-5, defer: bool = False) -> torch.Tensor:
    """``act_post(act(scale * (x @ weight.T) + bias) + residual + rowtab[row % len(rowtab)])`` on f32 MFMA.

    x [..., K] (or a 2-D row pool when ``a_map`` gathers rows), weight [N, K] as in nn.Linear.
    With ``out`` given (2-D row pool [R, N]) and ``c_map``, rows are scattered into it.
    ``rowdot_w`` [R, N] + ``rowdot_out`` [rows, ceil(N / 64), R]: the fused row-dot epilogue (afm_linear_args.rowdot_*): per 64-column
    group, the dot of the output row with each of the R vectors; ``store=False`` then skips writing the output itself.
    ``ln`` = (gamma, beta, eps) + ``ln_out`` (same row layout as the output): the fused LayerNorm of the output rows (afm_linear_args.ln_*,
    the workgroup finishing the last column tile of a row block normalises it); ``ln_counters`` = zeroed int32 scratch of >= ceil(M / 32)
    words (allocated here when omitted).  Returns the (pre-LayerNorm) output; the normalised rows are in ``ln_out``.
    LayerNorm folded ACROSS launches (afm_linear_args.stat_out / a_stat / res_stat): ``stat_out`` [rows, N / 64, 2] receives (mean, M2) per
    output row and 64-column group; ``a_stat`` = (statistics of the raw input rows, g [N]) with ``weight`` = W * gamma and ``bias`` =
    b + W beta makes this call compute W LN(x) + b from the RAW x; ``res_stat`` = (statistics, gamma, beta) adds LayerNorm(residual)."""
    lib = ffi.load()
    ffi.require_gpu(x, weight)
    x = ffi.f32c(x)
    weight = ffi.f32c(weight)
    K = x.shape[-1]
    N = weight.shape[0]
    assert weight.shape[1] == K, (weight.shape, x.shape)
    M = rows if rows is not None else x.numel() // K
    if out is None:
        out = torch.empty(*(x.shape[:-1] if rows is None else (M,)), N, device=x.device, dtype=torch.float32)
    a = ffi.LinearArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = x.data_ptr(), x.stride(-2) if x.dim() > 1 else K, weight.data_ptr(), K, out.data_ptr(), N
    a.M, a.N, a.K = M, N, K
    keep = [x, weight, out]
    for name, t in (("bias", bias), ("scale", scale)):
        if t is not None:
            t = ffi.f32c(t)
            assert t.numel() == N
            keep.append(t)
            setattr(a, name, t.data_ptr())
    if residual is not None:
        residual = ffi.f32c(residual)
        keep.append(residual)
        a.residual, a.ldr = residual.data_ptr(), N
    if rowtab is not None:
        rowtab = ffi.f32c(rowtab)
        keep.append(rowtab)
        a.rowtab, a.rowtab_period = rowtab.data_ptr(), rowtab.shape[0]
    a.act, a.act_post = act, act_post
    if a_map:
        a.a_grp, a.a_stride, a.a_off = a_map[:3]
        if len(a_map) == 5:                       # (group, stride, offset, skip_after, skip): a hole of `skip` rows behind member skip_after - 1
            a.a_skip_after, a.a_skip = a_map[3:]
    if c_map:
        a.c_grp, a.c_stride, a.c_off = c_map[:3]
        if len(c_map) == 5:
            a.c_skip_after, a.c_skip = c_map[3:]
    if rowdot_w is not None:
        rowdot_w = ffi.f32c(rowdot_w)
        R = rowdot_w.shape[0]
        assert rowdot_w.shape[1] == N and 1 <= R <= 8, rowdot_w.shape
        assert rowdot_out is not None and rowdot_out.is_contiguous() and rowdot_out.dtype == torch.float32 and rowdot_out.device == x.device
        assert rowdot_out.numel() >= M * ((N + 63) // 64) * R, (rowdot_out.shape, M, N, R)      # [rows, ceil(N / 64), R]: an undersized buffer is written out of bounds
        keep += [rowdot_w, rowdot_out]
        a.rowdot_w, a.rowdot_out, a.rowdot_n = rowdot_w.data_ptr(), rowdot_out.data_ptr(), rowdot_w.shape[0]
        if not store:
            a.C = None
    if ln is not None:
        g, b, eps = ln
        g, b = ffi.f32c(g), ffi.f32c(b)
        assert ln_out is not None and ln_out.dtype == torch.float32 and ln_out.is_contiguous() and ln_out.shape[-1] == N and g.numel() == N and b.numel() == N
        if ln_counters is None:
            ln_counters = torch.zeros((M + 31) // 32, dtype=torch.int32, device=x.device)
        assert ln_counters.dtype == torch.int32 and ln_counters.numel() >= (M + 31) // 32
        keep += [g, b, ln_out, ln_counters]
        a.ln_gamma, a.ln_beta, a.ln_out, a.ldo, a.ln_eps, a.ln_counters = g.data_ptr(), b.data_ptr(), ln_out.data_ptr(), N, float(eps), ln_counters.data_ptr()
    if stat_out is not None:
        assert stat_out.dtype == torch.float32 and stat_out.is_contiguous() and stat_out.numel() >= out.numel() // N * (N // 64) * 2 and N % 64 == 0
        keep.append(stat_out)
        a.stat_out = stat_out.data_ptr()
    if a_stat is not None:
        st, g = a_stat
        st, g = ffi.f32c(st), ffi.f32c(g)
        assert g.numel() == N and K % 64 == 0
        keep += [st, g]
        a.a_stat, a.a_stat_groups, a.a_fold_g = st.data_ptr(), K // 64, g.data_ptr()
    if res_stat is not None:
        st, g, b = res_stat
        st, g, b = ffi.f32c(st), ffi.f32c(g), ffi.f32c(b)
        assert residual is not None and g.numel() == N and b.numel() == N
        keep += [st, g, b]
        a.res_stat, a.res_gamma, a.res_beta = st.data_ptr(), g.data_ptr(), b.data_ptr()
    if stat_out is not None or a_stat is not None or res_stat is not None:
        a.ln_eps2 = float(ln_eps)
        # the folded-LayerNorm epilogue reads its side inputs 16 bytes at a time and writes stat_out only from that branch: a
        # contiguous-but-offset view (bias[1:]) is refused here as afm_linear refuses it (AFM_E_BADARG), never silently mis-normalised
        for nm in ("C", "residual", "bias", "a_fold_g", "res_gamma", "res_beta"):
            ptr = getattr(a, nm)
            if ptr and ptr % 16:
                raise ffi.AfmError(f"afm_linear with folded LayerNorm statistics: `{nm}` is not 16-byte aligned")
    fill_arith(a)
    if defer:                                           # linear_pair: the argument block instead of the launch
        return a, out, keep
    ffi.check(lib.afm_linear(C.byref(a), ffi.stream_of(x)), "afm_linear")
    return out


def linear_pair(first: dict, second: dict) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two independent `linear` calls (keyword dicts of `linear`) as ONE launch of 128 x 128 tiles (afm_linear_pair): bit-identical to the
    two calls; raises AfmError (AFM_E_UNSUPPORTED) when the pair is not eligible (both on the bf16-split path, one arithmetic, K > 256)."""
    a0, out0, keep0 = linear(**first, defer=True)
    a1, out1, keep1 = linear(**second, defer=True)
    ffi.check(ffi.load().afm_linear_pair(C.byref(a0), C.byref(a1), ffi.stream_of(out0)), "afm_linear_pair")
    del keep0, keep1
    return out0, out1


# ---- arithmetic of the GEMMs: HOST state (this module), written into every afm_linear_args / weight pack that is built.
# The library itself has no switch and reads no environment (ABI v3).  Two settings:
#   sampling / inference operators (`linear`, `mha`, the CMDM / CDM weight packs): AFM_GEMM_SPLIT / AFM_GEMM_SPLIT_MIN_N in the environment of the
#     Python process, else SIX products of the three-way bf16 operand split on every eligible GEMM and in the attention (round 6: the
#     worst-case comparison of tests/test_gpu_arith.py for the GEMMs - six products are never above nine and both sit in the error class of
#     an f32 chain; for the attention the value families of tests/test_gpu_attention_edges.py, profiles/attention_edges_parity.json - large and
#     near-tied logits, wide-range V, the worst-mantissa operands: six and nine products within 1.7 x the float32 reference's own error);
#   training operators (afm.autograd: every forward and backward GEMM of the tape): AFM_GEMM_SPLIT_TRAIN, else all NINE products (exact f32
#     products) - gradients through ~40 serial batch-statistics BatchNorms are ill-conditioned in float32 (the reference's own f32 backward sits
#     2.8e-2 from its f64 backward on the CDM's PointTrans U-Net), so the tape keeps every bit the operands carry.
DEFAULT_PRODUCTS, DEFAULT_TRAIN_PRODUCTS = 6, 9


def _initial_split():
    import os
    p = os.environ.get("AFM_GEMM_SPLIT")
    products = int(p) if p is not None else DEFAULT_PRODUCTS
    if products not in (0, 1, 6, 9):
        products = 0
    n = os.environ.get("AFM_GEMM_SPLIT_MIN_N")
    return products, max(0, int(n)) if n is not None else 0


def _initial_train_split():
    import os
    p = os.environ.get("AFM_GEMM_SPLIT_TRAIN")
    products = int(p) if p is not None else DEFAULT_TRAIN_PRODUCTS
    return products if products in (0, 6, 9) else 0


_gemm_split = list(_initial_split())
_train_split = [_initial_train_split()]
_gemm_tune = 0
_ARITH = {9: ffi.ARITH_BF16X9, 6: ffi.ARITH_BF16X6, 1: ffi.ARITH_BF16X1}


def gemm_arith() -> Tuple[int, int]:
    """(arith, arith_min_n) for afm_linear_args / afm_c(m)dm_weights from the host setting."""
    products, min_n = _gemm_split
    if products == 0:
        return ffi.ARITH_F32, 0
    return _ARITH[products], min_n


def set_train_gemm_split(products: int) -> int:
    """Arithmetic of the TRAINING operators' GEMMs (afm.autograd): 9 (default, exact f32 products), 6 or 0 (native f32 MFMA).  Returns the previous value."""
    if int(products) not in (0, 6, 9):
        raise ffi.AfmError(f"set_train_gemm_split: products must be 0, 6 or 9 (got {products})")
    prev, _train_split[0] = _train_split[0], int(products)
    return prev


def get_train_gemm_split() -> int:
    return _train_split[0]


def fill_arith_train(a) -> None:
    """afm_linear_args of a training operator: the tape's arithmetic (see the note above), never the sampling setting."""
    a.arith, a.arith_min_n = (ffi.ARITH_F32, 0) if _train_split[0] == 0 else (_ARITH[_train_split[0]], 0)
    a.tune = _gemm_tune


def set_gemm_split(products: int, min_n: Optional[int] = None):
    """Arithmetic of `linear`'s GEMMs and of `mha`: the three-way bf16 operand split on the bf16 matrix pipe with the 6 largest cross products
    (default, every eligible GEMM: K >= 128, K % 16 == 0, aligned) or all 9 (exact f32 products), 0 = native f32 MFMA everywhere.  ``min_n`` moves the N threshold.
    Returns the previous setting in the same form (products, or (products, min_n) when ``min_n`` was given)."""
    if int(products) not in (0, 1, 6, 9):
        raise ffi.AfmError(f"set_gemm_split: products must be 0, 6 or 9 (or 1: plain bf16, informational only) (got {products})")
    if min_n is not None and int(min_n) < 0:
        raise ffi.AfmError(f"set_gemm_split: min_n must be >= 0 (got {min_n})")
    prev = tuple(_gemm_split)
    _gemm_split[0] = int(products)
    if min_n is None:
        return prev[0]
    _gemm_split[1] = int(min_n)
    return prev


def get_gemm_split():
    """Current (products, min_n) of the GEMM arithmetic."""
    return tuple(_gemm_split)


def set_gemm_tune(tune: int) -> int:
    """Bit-neutral performance knobs of afm_linear for experiments (afm_linear_args.tune, AFM_TUNE_*); returns the previous value."""
    global _gemm_tune
    prev, _gemm_tune = _gemm_tune, int(tune)
    return prev


def fill_arith(a) -> None:
    a.arith, a.arith_min_n = gemm_arith()
    a.tune = _gemm_tune


def mha(qkv: torch.Tensor, key_mask: Optional[torch.Tensor], heads: int, group_waves: int = 0, q_first: int = 0) -> torch.Tensor:
    """qkv [B, T, 3*d] (packed in_proj output) -> softmax(QK^T/sqrt(dh) + mask) V, [B, T, d].  ``group_waves``: workgroup shape of
    afm_mha_fwd_grouped (0 = the library's choice); results do not depend on it.  ``q_first`` > 0 (afm_mha_fwd_rows): only the query
    rows q_first .. T - 1 are computed, the leading rows of the result are zeros."""
    lib = ffi.load()
    ffi.require_gpu(qkv)
    qkv = ffi.f32c(qkv)
    B, T, d3 = qkv.shape
    d = d3 // 3
    km = None
    if key_mask is not None:
        km = key_mask.to(torch.uint8).contiguous()
        assert km.shape == (B, T)
    arith = gemm_arith()[0]                             # the attention follows the host's GEMM arithmetic (six products by default)
    if q_first:
        out = torch.zeros(B, T, d, device=qkv.device, dtype=torch.float32)
        ffi.check(lib.afm_mha_fwd_arith(qkv.data_ptr(), ffi.ptr(km), out.data_ptr(), B, T, heads, d // heads, int(q_first), int(group_waves), arith,
                                        ffi.stream_of(qkv)), "afm_mha_fwd_arith")
        return out
    out = torch.empty(B, T, d, device=qkv.device, dtype=torch.float32)
    ffi.check(lib.afm_mha_fwd_arith(qkv.data_ptr(), ffi.ptr(km), out.data_ptr(), B, T, heads, d // heads, 0, int(group_waves), arith,
                                    ffi.stream_of(qkv)), "afm_mha_fwd_arith")
    return out


def clamp_(x: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """In-place clamp of a float32 GPU tensor (afm_clamp): `process_xstart` with clip_denoised=True (gaussian_diffusion.py:289-294)."""
    ffi.require_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    ffi.check(ffi.load().afm_clamp(x.data_ptr(), x.numel(), float(lo), float(hi), ffi.stream_of(x)), "afm_clamp")
    return x


def mha_cross(q: torch.Tensor, kv: torch.Tensor, key_mask: Optional[torch.Tensor], heads: int) -> torch.Tensor:
    """q [B, Tq, d], kv [B, Tk, 2*d] (packed k | v), key_mask [B, Tk] (True = ignore) -> [B, Tq, d]."""
    lib = ffi.load()
    ffi.require_gpu(q, kv)
    q, kv = ffi.f32c(q), ffi.f32c(kv)
    B, Tq, d = q.shape
    Tk = kv.shape[1]
    assert kv.shape[2] == 2 * d
    out = torch.empty(B, Tq, d, device=q.device, dtype=torch.float32)
    km = None
    if key_mask is not None:
        km = key_mask.to(torch.uint8).contiguous()
        assert km.shape == (B, Tk)
    ffi.check(lib.afm_mha_cross_fwd(q.data_ptr(), kv.data_ptr(), ffi.ptr(km), out.data_ptr(), B, Tq, Tk, heads, d // heads, ffi.stream_of(q)),
              "afm_mha_cross_fwd")
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = ffi.load()
    ffi.require_gpu(x)
    x = ffi.f32c(x)
    out = torch.empty_like(x) if out is None else out
    dim = x.shape[-1]
    w, b = ffi.f32c(weight), ffi.f32c(bias)
    ffi.check(lib.afm_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), x.numel() // dim, dim, eps,
                                ffi.stream_of(x)), "afm_layernorm")
    return out


def ddpm_step(x0: torch.Tensor, x_t: torch.Tensor, noise: Optional[torch.Tensor], c1: torch.Tensor, c2: torch.Tensor,
              sigma: torch.Tensor, *, seed: int = 0, sample_index0: int = 0, step: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_{t-1} = (c1*x0 + c2*x_t) + sigma*noise, per-sample coefficients [B] (no fma contraction)."""
    lib = ffi.load()
    ffi.require_gpu(x0, x_t)
    x0, x_t = ffi.f32c(x0), ffi.f32c(x_t)
    B = x0.shape[0]
    per = x0.numel() // max(B, 1)
    out = torch.empty_like(x0) if out is None else out
    nz = None if noise is None else ffi.f32c(noise)
    c1, c2, sigma = ffi.f32c(c1), ffi.f32c(c2), ffi.f32c(sigma)
    ffi.check(lib.afm_ddpm_step(x0.data_ptr(), x_t.data_ptr(), ffi.ptr(nz), out.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                sigma.data_ptr(), B, per, seed & (2**64 - 1), sample_index0, step, ffi.stream_of(x0)),
              "afm_ddpm_step")
    return out


def ddim_step(x0: torch.Tensor, x_t: torch.Tensor, noise: Optional[torch.Tensor], a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
              d: torch.Tensor, sigma: Optional[torch.Tensor], *, seed: int = 0, sample_index0: int = 0, step: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DDIM update (afm_ddim_step): eps = (a*x_t - x0) / b, x_next = (x0*c + d*eps) + sigma*noise, per-sample rows [B], every operation
    rounded on its own.  sigma None: no noise term (ddim_reverse_sample); noise None: Philox keyed like ddpm_step."""
    lib = ffi.load()
    ffi.require_gpu(x0, x_t)
    x0, x_t = ffi.f32c(x0), ffi.f32c(x_t)
    B = x0.shape[0]
    per = x0.numel() // max(B, 1)
    out = torch.empty_like(x0) if out is None else out
    nz = None if noise is None or sigma is None else ffi.f32c(noise)
    keep = [ffi.f32c(r) for r in (a, b, c, d)] + ([] if sigma is None else [ffi.f32c(sigma)])
    rows = ffi.DdimRows(*[r.data_ptr() for r in keep[:4]], None if sigma is None else keep[4].data_ptr())
    ffi.check(lib.afm_ddim_step(x0.data_ptr(), x_t.data_ptr(), ffi.ptr(nz), out.data_ptr(), C.byref(rows), B, per, seed & (2**64 - 1),
                                sample_index0, step, ffi.stream_of(x0)), "afm_ddim_step")
    return out


def dpm_step(x0: torch.Tensor, x_t: torch.Tensor, prev: Optional[torch.Tensor], a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, *,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DPM-Solver++(2M) update (afm_dpm_step): x_next = a*x_t + b*x0 (``prev`` None: no history) or (a*x_t + b*x0) + c*prev, per-sample
    rows [B], float32, every operation rounded on its own.  No noise term.  ``out`` may be ``x_t``."""
    lib = ffi.load()
    ffi.require_gpu(x0, x_t, prev)
    x0, x_t = ffi.f32c(x0), ffi.f32c(x_t)
    pv = None if prev is None else ffi.f32c(prev)
    if x_t.shape != x0.shape or (pv is not None and pv.shape != x0.shape):
        raise ValueError(f"dpm_step: x0 {tuple(x0.shape)}, x_t {tuple(x_t.shape)} and prev must have one shape")
    B = x0.shape[0]
    per = x0.numel() // max(B, 1)
    out = torch.empty_like(x0) if out is None else out
    keep = [ffi.f32c(r) for r in (a, b, c)]
    if any(r.numel() != B for r in keep):
        raise ValueError(f"dpm_step: the rows hold one value per sample ({B})")
    rows = ffi.DpmRows(*[r.data_ptr() for r in keep])
    ffi.check(lib.afm_dpm_step(x0.data_ptr(), x_t.data_ptr(), ffi.ptr(pv), out.data_ptr(), C.byref(rows), B, per, ffi.stream_of(x0)),
              "afm_dpm_step")
    return out


def cfg_combine(x0_c: torch.Tensor, x0_u: torch.Tensor, scale: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Classifier-free guidance of an x_start prediction (afm_cfg_combine): x0_u + scale[b] * (x0_c - x0_u), float32, every operation
    rounded on its own; scale [B]."""
    lib = ffi.load()
    ffi.require_gpu(x0_c, x0_u, scale)
    x0_c, x0_u, scale = ffi.f32c(x0_c), ffi.f32c(x0_u), ffi.f32c(scale)
    B = x0_c.shape[0]
    if scale.numel() != B or x0_u.shape != x0_c.shape:
        raise ValueError(f"cfg_combine: scale must hold one value per sample ({B}), got {tuple(scale.shape)}; branches {tuple(x0_c.shape)} / {tuple(x0_u.shape)}")
    out = torch.empty_like(x0_c) if out is None else out
    ffi.check(lib.afm_cfg_combine(x0_c.data_ptr(), x0_u.data_ptr(), scale.data_ptr(), out.data_ptr(), B, x0_c.numel() // max(B, 1),
                                  ffi.stream_of(x0_c)), "afm_cfg_combine")
    return out


def _step_tail(a, x0, x_t, out, noise, ddpm, ddim, clip, seed, sample_index0, step) -> list:
    """The fields CfgStepArgs, ImputeStepArgs and Cfg2StepArgs share: x_t, x_next, noise, the DDPM or DDIM rows, clip, the sizes, the Philox
    key.  -> what must stay alive until the call returns (the contiguous noise and rows, the DdimRows struct ``a.ddim`` points to)."""
    B = x0.shape[0]
    nz = None if noise is None else ffi.f32c(noise)
    a.x_t, a.x_next, a.noise = x_t.data_ptr(), out.data_ptr(), ffi.ptr(nz)
    keep = [ffi.f32c(r) for r in (ddpm if ddpm is not None else ddim) if r is not None]
    if ddpm is not None:
        a.c1, a.c2, a.sigma = (r.data_ptr() for r in keep)
    else:
        rows = ffi.DdimRows(*[r.data_ptr() for r in keep[:4]], keep[4].data_ptr() if len(keep) > 4 else None)
        a.ddim = C.pointer(rows)
        keep.append(rows)
    a.clip, a.B, a.per_sample = int(bool(clip)), B, x0.numel() // max(B, 1)
    a.seed, a.sample_index0, a.step = seed & (2**64 - 1), sample_index0, step
    return keep + [nz]


def cfg_step(x0_c: torch.Tensor, x0_u: torch.Tensor, scale: torch.Tensor, x_t: torch.Tensor, noise: Optional[torch.Tensor], *,
             ddpm=None, ddim=None, clip: bool = False, seed: int = 0, sample_index0: int = 0, step: int = 0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One guided sampling update (afm_cfg_step): cfg_combine, the clamp to [-1, 1] if ``clip``, then the ddpm_step expression with
    ``ddpm`` = (c1, c2, sigma) per-sample rows or the ddim_step expression with ``ddim`` = (a, b, c, d, sigma | None).  noise None: Philox."""
    if (ddpm is None) == (ddim is None):
        raise ValueError("cfg_step: exactly one of ddpm= / ddim= rows")
    lib = ffi.load()
    ffi.require_gpu(x0_c, x0_u, x_t)
    x0_c, x0_u, scale, x_t = ffi.f32c(x0_c), ffi.f32c(x0_u), ffi.f32c(scale), ffi.f32c(x_t)
    B = x0_c.shape[0]
    if scale.numel() != B:
        raise ValueError(f"cfg_step: scale must hold one value per sample ({B}), got {tuple(scale.shape)}")
    out = torch.empty_like(x0_c) if out is None else out
    a = ffi.CfgStepArgs()
    a.x0_c, a.x0_u, a.scale = x0_c.data_ptr(), x0_u.data_ptr(), scale.data_ptr()
    keep = _step_tail(a, x0_c, x_t, out, noise, ddpm, ddim, clip, seed, sample_index0, step)
    ffi.check(lib.afm_cfg_step(C.byref(a), ffi.stream_of(x0_c)), "afm_cfg_step")
    return out


def impute(x0: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Imputation of known values into an x_start prediction (afm_impute): where(mask, known, x0), a select - ``known`` is not read where
    the mask is 0.  known float32 and mask uint8 / bool, both of x0's shape; ``out`` may be x0."""
    lib = ffi.load()
    ffi.require_gpu(x0, known, mask)
    x0, known = ffi.f32c(x0), ffi.f32c(known)
    mask = _mask_u8(mask)
    if known.shape != x0.shape or mask.shape != x0.shape:
        raise ValueError(f"impute: known {tuple(known.shape)} and mask {tuple(mask.shape)} must have x0's shape {tuple(x0.shape)}")
    out = torch.empty_like(x0) if out is None else out
    ffi.check(lib.afm_impute(x0.data_ptr(), known.data_ptr(), mask.data_ptr(), out.data_ptr(), x0.numel(), ffi.stream_of(x0)), "afm_impute")
    return out


def _mask_u8(mask: torch.Tensor) -> torch.Tensor:
    """a bool / uint8 mask as contiguous uint8 (bool storage is one byte of 0 / 1: a view, no kernel)"""
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise ValueError(f"mask must be bool or uint8, not {mask.dtype}")
    return mask.contiguous()


def impute_step(x0: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, x_t: torch.Tensor, noise: Optional[torch.Tensor], *,
                x0_u: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, ddpm=None, ddim=None, clip: bool = False,
                seed: int = 0, sample_index0: int = 0, step: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One imputing sampling update (afm_impute_step): x0 (with ``x0_u`` and ``scale``: cfg_combine(x0, x0_u, scale)), then impute, the clamp
    to [-1, 1] if ``clip``, then the ddpm_step expression with ``ddpm`` = (c1, c2, sigma) per-sample rows or the ddim_step expression with
    ``ddim`` = (a, b, c, d, sigma | None).  noise None: Philox."""
    if (ddpm is None) == (ddim is None):
        raise ValueError("impute_step: exactly one of ddpm= / ddim= rows")
    if (x0_u is None) != (scale is None):
        raise ValueError("impute_step: x0_u= and scale= go together")
    lib = ffi.load()
    ffi.require_gpu(x0, known, mask, x_t)
    x0, known, x_t = ffi.f32c(x0), ffi.f32c(known), ffi.f32c(x_t)
    mask = _mask_u8(mask)
    B = x0.shape[0]
    if known.shape != x0.shape or mask.shape != x0.shape:
        raise ValueError(f"impute_step: known {tuple(known.shape)} and mask {tuple(mask.shape)} must have x0's shape {tuple(x0.shape)}")
    out = torch.empty_like(x0) if out is None else out
    a = ffi.ImputeStepArgs()
    a.x0_c, a.known, a.mask = x0.data_ptr(), known.data_ptr(), mask.data_ptr()
    if x0_u is not None:
        x0_u, scale = ffi.f32c(x0_u), ffi.f32c(scale)
        if scale.numel() != B or x0_u.shape != x0.shape:
            raise ValueError(f"impute_step: scale must hold one value per sample ({B}), got {tuple(scale.shape)}; x0_u {tuple(x0_u.shape)}")
        a.x0_u, a.scale = x0_u.data_ptr(), scale.data_ptr()
    keep = _step_tail(a, x0, x_t, out, noise, ddpm, ddim, clip, seed, sample_index0, step)
    ffi.check(lib.afm_impute_step(C.byref(a), ffi.stream_of(x0)), "afm_impute_step")
    return out


def guide_step(x0: torch.Tensor, x_t: torch.Tensor, noise: Optional[torch.Tensor], *, grad: Optional[torch.Tensor] = None,
               gk: Optional[torch.Tensor] = None, x0_a: Optional[torch.Tensor] = None, x0_u: Optional[torch.Tensor] = None,
               scale: Optional[torch.Tensor] = None, scale2: Optional[torch.Tensor] = None, known: Optional[torch.Tensor] = None,
               mask: Optional[torch.Tensor] = None, ddpm=None, ddim=None, dpm=None, prev: Optional[torch.Tensor] = None, clip: bool = False,
               seed: int = 0, sample_index0: int = 0, step: int = 0, out: Optional[torch.Tensor] = None,
               x0_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One sampling update with a cond_fn gradient (afm_guide_step): x0 (with ``x0_u`` / ``scale``: cfg_combine; with ``x0_a`` / ``scale2``
    too: cfg2_combine), impute with ``known`` / ``mask``, the clamp to [-1, 1] if ``clip``, then with ``grad`` [B, ...] and its per-sample
    coefficient ``gk`` [B] (both or neither), in float32 with every operation rounded on its own:

        ddim= (a, b, c, d, sigma | None) or dpm= (a, b, c) with ``prev``:   m = gk[b] * grad;  x0' = x0 + m;  the ddim_step / dpm_step
                                                                             expression on x0' (``x0_out``, if given, receives x0')
        ddpm= (c1, c2, sigma):                                              m = gk[b] * grad;  x_next = ((c1*x0 + c2*x_t) + m) + sigma*noise

    Without ``grad`` nothing of it is read and the result is cfg_step / impute_step / cfg2_step / ddpm_step / ddim_step / dpm_step of
    the same arguments, bit for bit.  noise None: Philox.  ``out`` may be ``x_t``."""
    if sum(r is not None for r in (ddpm, ddim, dpm)) != 1:
        raise ValueError("guide_step: exactly one of ddpm= / ddim= / dpm= rows")
    if (known is None) != (mask is None):
        raise ValueError("guide_step: known= and mask= go together")
    lib = ffi.load()
    ffi.require_gpu(x0, x_t, grad, prev)
    x0, x_t = ffi.f32c(x0), ffi.f32c(x_t)
    B = x0.shape[0]
    out = torch.empty_like(x0) if out is None else out
    a = ffi.GuideStepArgs()
    keep = []

    def same(name, t):
        t = ffi.f32c(t)
        if t.shape != x0.shape:
            raise ValueError(f"guide_step: {name} {tuple(t.shape)} must have x0's shape {tuple(x0.shape)}")
        keep.append(t)
        return t.data_ptr()

    def row(name, t):
        t = ffi.f32c(t)
        if t.numel() != B:
            raise ValueError(f"guide_step: {name} must hold one value per sample ({B}), got {tuple(t.shape)}")
        keep.append(t)
        return t.data_ptr()
    a.x0_c = x0.data_ptr()
    if x_t.shape != x0.shape:
        raise ValueError(f"guide_step: x_t {tuple(x_t.shape)} must have x0's shape {tuple(x0.shape)}")
    for name, t in (("x0_a", x0_a), ("x0_u", x0_u), ("known", known), ("grad", grad), ("x0_prev", prev)):
        if t is not None:
            setattr(a, name, same(name, t))
    for name, t in (("scale", scale), ("scale2", scale2), ("gk", gk)):
        if t is not None:
            setattr(a, name, row(name, t))
    if mask is not None:
        mask = _mask_u8(mask)
        if mask.shape != x0.shape:
            raise ValueError(f"guide_step: mask {tuple(mask.shape)} must have x0's shape {tuple(x0.shape)}")
        a.mask = mask.data_ptr()
    if x0_out is not None:
        if x0_out.dtype != torch.float32 or x0_out.shape != x0.shape or not x0_out.is_contiguous() or x0_out.device != x0.device:
            raise ValueError(f"guide_step: x0_out must be a contiguous float32 tensor of x0's shape {tuple(x0.shape)} on {x0.device}")
        a.x0_out = x0_out.data_ptr()
    if dpm is not None:
        rows = [ffi.f32c(r) for r in dpm]
        drows = ffi.DpmRows(*[r.data_ptr() for r in rows])
        a.dpm = C.pointer(drows)
        keep += rows + [drows]
        a.x_t, a.x_next = x_t.data_ptr(), out.data_ptr()
        a.clip, a.B, a.per_sample = int(bool(clip)), B, x0.numel() // max(B, 1)
    else:
        keep += _step_tail(a, x0, x_t, out, noise, ddpm, ddim, clip, seed, sample_index0, step)
    ffi.check(lib.afm_guide_step(C.byref(a), ffi.stream_of(x0)), "afm_guide_step")
    return out


def contact_guidance(guide: "ffi.ContactGuide", x: torch.Tensor, frame_mask: Optional[torch.Tensor], t: Optional[torch.Tensor] = None, *,
                     grad: bool = True, energy: bool = False):
    """afm_contact_guidance of a filled description (afm.diffusion.ContactGuidance builds it): -> (grad [B, L, D] or None, energy [B] or
    None) of x [B, L, D]; ``frame_mask`` [B, L] (True / nonzero = padded) or None; ``t`` [B] int64 (samples with t >= guide.t_start get a
    zero gradient) or None.  Two launches (an h3d description: four), no atomics; the workspace is allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, frame_mask, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    fm = None if frame_mask is None else _mask_u8(frame_mask.reshape(B, L))
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    e = torch.empty(B, dtype=torch.float32, device=x.device) if energy else None
    if guide.h3d:
        sizer, nbytes = "afm_contact_guidance_h3d_workspace_bytes", int(lib.afm_contact_guidance_h3d_workspace_bytes(B, L, guide.N, guide.K))
    else:
        sizer, nbytes = "afm_contact_guidance_workspace_bytes", int(lib.afm_contact_guidance_workspace_bytes(B, guide.N, guide.K))
    if nbytes < 0:
        ffi.check(nbytes, sizer)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_contact_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(fm), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(e), B, L, D, ws.data_ptr(),
                                       ws.numel(), ffi.stream_of(x)), "afm_contact_guidance")
    return g, e


def motion_guidance(guide: "ffi.MotionGuide", x: torch.Tensor, frame_mask: Optional[torch.Tensor], t: Optional[torch.Tensor] = None, *,
                    grad: bool = True, energy: bool = False):
    """afm_motion_guidance of a filled sum (afm.diffusion.JointTargets / MotionGuidance build it): -> (grad [B, L, D] or None, the contact
    term's energy [B] or None, the targets' energy [B] or None) of x [B, L, D].  grad = grad_contact + grad_targets, each term the float32
    result of that guidance alone, one rounded addition per element; a term that is not set contributes nothing and has no energy.
    Launches: the contact term's 2 (h3d: 4) plus the targets' 1 (h3d: 3); no atomics; the workspace is allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, frame_mask, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    fm = None if frame_mask is None else _mask_u8(frame_mask.reshape(B, L))
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    ec = torch.empty(B, dtype=torch.float32, device=x.device) if energy and guide.contact else None
    et = torch.empty(B, dtype=torch.float32, device=x.device) if energy and guide.targets else None
    nbytes = int(lib.afm_motion_guidance_workspace_bytes(C.byref(guide), B, L, D))
    if nbytes < 0:
        ffi.check(nbytes, "afm_motion_guidance_workspace_bytes")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_motion_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(fm), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(ec), ffi.ptr(et), B, L, D,
                                      ws.data_ptr(), ws.numel(), ffi.stream_of(x)), "afm_motion_guidance")
    return g, ec, et


def scene_guidance(guide: "ffi.SceneGuide", x: torch.Tensor, frame_mask: Optional[torch.Tensor], t: Optional[torch.Tensor] = None, *,
                   grad: bool = True, energy: bool = False):
    """afm_scene_guidance of a filled sum (afm.diffusion.SceneClearance / MotionGuidance build it): -> (grad [B, L, D] or None, the contact
    term's energy [B] or None, the targets', the clearance's) of x [B, L, D].  grad = (grad_contact + grad_targets) + grad_clearance, each
    term the float32 result of that term alone, one rounded addition per element; a term that is not set contributes nothing and has no
    energy.  Launches: the terms' of afm_motion_guidance plus the clearance's 1 (h3d: 3); no atomics; the workspace is allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, frame_mask, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    fm = None if frame_mask is None else _mask_u8(frame_mask.reshape(B, L))
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    terms = guide.terms.contents if guide.terms else None
    new = lambda on: torch.empty(B, dtype=torch.float32, device=x.device) if energy and on else None
    ec, et, el = new(terms is not None and bool(terms.contact)), new(terms is not None and bool(terms.targets)), new(bool(guide.clearance))
    nbytes = int(lib.afm_scene_guidance_workspace_bytes(C.byref(guide), B, L, D))
    if nbytes < 0:
        ffi.check(nbytes, "afm_scene_guidance_workspace_bytes")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_scene_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(fm), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(ec), ffi.ptr(et), ffi.ptr(el), B, L, D,
                                     ws.data_ptr(), ws.numel(), ffi.stream_of(x)), "afm_scene_guidance")
    return g, ec, et, el


def ground_guidance(guide: "ffi.GroundGuide", x: torch.Tensor, frame_mask: Optional[torch.Tensor], t: Optional[torch.Tensor] = None, *,
                    grad: bool = True, energy: bool = False):
    """afm_ground_guidance of a filled sum (afm.diffusion.FootGrounding / MotionGuidance build it): -> (grad [B, L, D] or None, the contact
    term's energy [B] or None, the targets', the clearance's, the grounding's) of x [B, L, D].  grad = ((grad_contact + grad_targets) +
    grad_clearance) + grad_feet, each term the float32 result of that term alone, one rounded addition per element; a term that is not set
    contributes nothing and has no energy.  Launches: the terms' of afm_scene_guidance plus the grounding's 1 (h3d: 3); no atomics; the
    workspace is allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, frame_mask, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    fm = None if frame_mask is None else _mask_u8(frame_mask.reshape(B, L))
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    scene = guide.terms.contents if guide.terms else None
    terms = scene.terms.contents if scene is not None and scene.terms else None
    new = lambda on: torch.empty(B, dtype=torch.float32, device=x.device) if energy and on else None
    ec, et = new(terms is not None and bool(terms.contact)), new(terms is not None and bool(terms.targets))
    el, ef = new(scene is not None and bool(scene.clearance)), new(bool(guide.feet))
    nbytes = int(lib.afm_ground_guidance_workspace_bytes(C.byref(guide), B, L, D))
    if nbytes < 0:
        ffi.check(nbytes, "afm_ground_guidance_workspace_bytes")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_ground_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(fm), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(ec), ffi.ptr(et), ffi.ptr(el), ffi.ptr(ef),
                                      B, L, D, ws.data_ptr(), ws.numel(), ffi.stream_of(x)), "afm_ground_guidance")
    return g, ec, et, el, ef


def h3d_joint_list(joints, limit: int, who: str):
    """the joint list of a HumanML3D-feature motion as ints (None: all 22), checked: 1..limit joints, each 0..21, none twice"""
    joints = list(range(ffi.H3D_JOINTS)) if joints is None else [int(j) for j in joints]
    if not 1 <= len(joints) <= limit:
        raise ValueError(f"{who}: 1 to {limit} joints, got {len(joints)}")
    for i, j in enumerate(joints):
        if not 0 <= j < ffi.H3D_JOINTS:
            raise ValueError(f"{who}: joint {j} is outside 0..{ffi.H3D_JOINTS - 1}")
        if j in joints[:i]:
            raise ValueError(f"{who}: joint {j} is named twice")
    return joints


def h3d_to_scene(to_scene: Optional[torch.Tensor], who: str):
    """``to_scene`` checked apart from its device and batch: None, or a float32 [3, 4] / [B, 3, 4] tensor"""
    if to_scene is None:
        return None
    if not isinstance(to_scene, torch.Tensor) or to_scene.dtype != torch.float32 or to_scene.dim() not in (2, 3) or tuple(to_scene.shape[-2:]) != (3, 4):
        what = f"{tuple(to_scene.shape)} {to_scene.dtype}" if isinstance(to_scene, torch.Tensor) else type(to_scene).__name__
        raise ValueError(f"{who}: to_scene must be a float32 [3, 4] or [B, 3, 4] tensor, got {what}")
    return to_scene.detach()


def h3d_to_scene_on(to_scene: Optional[torch.Tensor], B: int, device, who: str):
    """(contiguous tensor or None, batch stride in floats) of a checked ``to_scene`` against a batch on ``device``"""
    if to_scene is None:
        return None, 0
    if to_scene.device != device:
        raise ValueError(f"{who}: to_scene is on {to_scene.device}, the sample on {device}")
    if to_scene.dim() == 3 and to_scene.shape[0] != B:
        raise ValueError(f"{who}: to_scene holds {to_scene.shape[0]} matrices for a batch of {B}")
    return to_scene.contiguous(), (12 if to_scene.dim() == 3 else 0)


def h3d_joints(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, *, x_mask: Optional[torch.Tensor] = None, joints=None,
               to_scene: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Joint positions [B, L, J, 3] of a HumanML3D-feature motion x [B, L, D >= 67] (afm_h3d_joints: the reference's recover_from_ric on
    the device, one launch).  ``mean`` / ``std`` [D] de-normalise x; ``joints``: the joint indices 0..21 wanted (None: all 22);
    ``x_mask`` [B, L] (True = padded): a padded frame's rotation and root velocities count as zero, so with valid frames first the valid
    frames come out as without a mask; ``to_scene`` [3, 4] or [B, 3, 4] float32 = [A|t] places the motion in the scene, p = A P + t
    (None: identity; y-up to z-up is A = [[1, 0, 0], [0, 0, -1], [0, 1, 0]])."""
    who = "h3d_joints"
    if x.dim() != 3 or x.shape[-1] < ffi.H3D_COLS:
        raise ValueError(f"{who}: x must be [B, L, D] with D >= {ffi.H3D_COLS} HumanML3D feature columns, got {tuple(x.shape)}")
    B, L, D = x.shape
    if mean.dim() != 1 or mean.shape[0] != D or std.shape != mean.shape:
        raise ValueError(f"{who}: mean and std must be [{D}], got {tuple(mean.shape)} and {tuple(std.shape)}")
    joints = h3d_joint_list(joints, ffi.H3D_JOINTS, who)
    ts, stride = h3d_to_scene_on(h3d_to_scene(to_scene, who), B, x.device, who)
    ffi.require_gpu(x, x_mask)
    lib = ffi.load()
    x = ffi.f32c(x)
    mean, std = ffi.f32c(mean.detach().to(x.device)), ffi.f32c(std.detach().to(x.device))
    fm = None if x_mask is None else _mask_u8(x_mask.reshape(B, L))
    out = torch.empty((B, L, len(joints), 3), dtype=torch.float32, device=x.device)
    if L == 0:
        return out
    jl = (C.c_int32 * len(joints))(*joints)
    ffi.check(lib.afm_h3d_joints(x.data_ptr(), mean.data_ptr(), std.data_ptr(), ffi.ptr(fm), jl, len(joints), ffi.ptr(ts), stride, out.data_ptr(),
                                 B, L, D, ffi.stream_of(x)), "afm_h3d_joints")
    return out


def cfg2_combine(x0_c: torch.Tensor, x0_a: torch.Tensor, x0_u: torch.Tensor, scale_first: torch.Tensor, scale_second: torch.Tensor, *,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two-scale guidance of an x_start prediction (afm_cfg2_combine): (x0_u + scale_first[b] * (x0_a - x0_u)) + scale_second[b] *
    (x0_c - x0_a), float32, every operation rounded on its own; both scales [B]."""
    lib = ffi.load()
    ffi.require_gpu(x0_c, x0_a, x0_u, scale_first, scale_second)
    x0_c, x0_a, x0_u, s1, s2 = (ffi.f32c(v) for v in (x0_c, x0_a, x0_u, scale_first, scale_second))
    B = x0_c.shape[0]
    if s1.numel() != B or s2.numel() != B or x0_a.shape != x0_c.shape or x0_u.shape != x0_c.shape:
        raise ValueError(f"cfg2_combine: each scale must hold one value per sample ({B}), got {tuple(s1.shape)} / {tuple(s2.shape)}; "
                         f"branches {tuple(x0_c.shape)} / {tuple(x0_a.shape)} / {tuple(x0_u.shape)}")
    out = torch.empty_like(x0_c) if out is None else out
    ffi.check(lib.afm_cfg2_combine(x0_c.data_ptr(), x0_a.data_ptr(), x0_u.data_ptr(), s1.data_ptr(), s2.data_ptr(), out.data_ptr(), B,
                                   x0_c.numel() // max(B, 1), ffi.stream_of(x0_c)), "afm_cfg2_combine")
    return out


def cfg2_step(x0_c: torch.Tensor, x0_a: torch.Tensor, x0_u: torch.Tensor, scale_first: torch.Tensor, scale_second: torch.Tensor,
              x_t: torch.Tensor, noise: Optional[torch.Tensor], *, known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              ddpm=None, ddim=None, clip: bool = False, seed: int = 0, sample_index0: int = 0, step: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One two-scale sampling update (afm_cfg2_step): cfg2_combine, impute with ``known`` / ``mask`` (both or neither), the clamp to
    [-1, 1] if ``clip``, then the ddpm_step expression with ``ddpm`` = (c1, c2, sigma) per-sample rows or the ddim_step expression with
    ``ddim`` = (a, b, c, d, sigma | None).  noise None: Philox."""
    if (ddpm is None) == (ddim is None):
        raise ValueError("cfg2_step: exactly one of ddpm= / ddim= rows")
    if (known is None) != (mask is None):
        raise ValueError("cfg2_step: known= and mask= go together")
    lib = ffi.load()
    ffi.require_gpu(x0_c, x0_a, x0_u, x_t)
    x0_c, x0_a, x0_u, s1, s2, x_t = (ffi.f32c(v) for v in (x0_c, x0_a, x0_u, scale_first, scale_second, x_t))
    B = x0_c.shape[0]
    if s1.numel() != B or s2.numel() != B or x0_a.shape != x0_c.shape or x0_u.shape != x0_c.shape:
        raise ValueError(f"cfg2_step: each scale must hold one value per sample ({B}), got {tuple(s1.shape)} / {tuple(s2.shape)}; "
                         f"branches {tuple(x0_c.shape)} / {tuple(x0_a.shape)} / {tuple(x0_u.shape)}")
    out = torch.empty_like(x0_c) if out is None else out
    a = ffi.Cfg2StepArgs()
    a.x0_c, a.x0_a, a.x0_u, a.scale_first, a.scale_second = x0_c.data_ptr(), x0_a.data_ptr(), x0_u.data_ptr(), s1.data_ptr(), s2.data_ptr()
    if known is not None:
        known, mask = ffi.f32c(known), _mask_u8(mask)
        if known.shape != x0_c.shape or mask.shape != x0_c.shape:
            raise ValueError(f"cfg2_step: known {tuple(known.shape)} and mask {tuple(mask.shape)} must have x0's shape {tuple(x0_c.shape)}")
        a.known, a.mask = known.data_ptr(), mask.data_ptr()
    keep = _step_tail(a, x0_c, x_t, out, noise, ddpm, ddim, clip, seed, sample_index0, step)
    ffi.check(lib.afm_cfg2_step(C.byref(a), ffi.stream_of(x0_c)), "afm_cfg2_step")
    return out


def randn(shape, device, *, seed: int, sample_index0: int = 0, step: int = 0) -> torch.Tensor:
    """Counter-based N(0,1) noise keyed by (seed, global sample index, step, element)."""
    lib = ffi.load()
    out = torch.empty(*shape, device=device, dtype=torch.float32)
    ffi.require_gpu(out)
    B = shape[0]
    ffi.check(lib.afm_randn(out.data_ptr(), B, out.numel() // max(B, 1), seed & (2**64 - 1), sample_index0, step,
                            ffi.stream_of(out)), "afm_randn")
    return out


def masked_mse(target: torch.Tensor, pred: torch.Tensor, frame_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Per-sample MSE over the un-padded frames: [B, L, D] x2 (+ [B, L] bool, True = padded) -> [B]."""
    lib = ffi.load()
    ffi.require_gpu(target, pred)
    target, pred = ffi.f32c(target), ffi.f32c(pred)
    B, D = target.shape[0], target.shape[-1]
    L = target.numel() // max(B * D, 1)
    km = None if frame_mask is None else frame_mask.reshape(B, L).to(torch.uint8).contiguous()
    out = torch.empty(B, device=target.device, dtype=torch.float32)
    ffi.check(lib.afm_masked_mse(target.data_ptr(), pred.data_ptr(), ffi.ptr(km), out.data_ptr(), B, L, D,
                                 ffi.stream_of(target)), "afm_masked_mse")
    return out


# ---------------------------------------------------------------------- long motions as overlapping windows (afm.diffusion.Stitch)
def _stitch_desc(stitch, x: torch.Tensor, who: str):
    """(afm_stitch of ``stitch`` on x's device, what must stay alive with it), x [B, L, D] checked against the geometry"""
    if x.dim() != 3:
        raise ValueError(f"{who}: the windows are [B, L, D], got {tuple(x.shape)}")
    stitch.check(x.shape[0], x.shape[1])
    return stitch.describe(x.device)


def stitch_blend(x0: torch.Tensor, stitch, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The blend of the frames neighbouring windows share (afm_stitch_blend): x0 [G * S, L, D]; for f < overlap, window w's frame
    L - overlap + f and window w + 1's frame f both become (wl[f] * left) + (wr[f] * right), float32, each operation rounded on its
    own; everything else is copied.  ``stitch``: an afm.diffusion.Stitch.  ``out`` may be x0.  No blend (one window, no overlap): the
    input's bits."""
    lib = ffi.load()
    ffi.require_gpu(x0)
    x0 = ffi.f32c(x0)
    st, keep = _stitch_desc(stitch, x0, "stitch_blend")
    out = torch.empty_like(x0) if out is None else out
    if out.shape != x0.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x0.device:
        raise ValueError(f"stitch_blend: out must be a contiguous float32 tensor of x0's shape {tuple(x0.shape)} on {x0.device}")
    B, L, D = x0.shape
    ffi.check(lib.afm_stitch_blend(x0.data_ptr(), out.data_ptr(), C.byref(st), B, L, D, ffi.stream_of(x0)), "afm_stitch_blend")
    return out


def stitch_windows(long_motion: torch.Tensor, windows: int, overlap: int, length: int) -> torch.Tensor:
    """[G, F, D] -> the windows [G * S, L, D] (afm_stitch_windows): window w holds the long frames w * (L - overlap) ..; frames at or
    behind F are zero.  Copies."""
    lib = ffi.load()
    ffi.require_gpu(long_motion)
    x = ffi.f32c(long_motion)
    if x.dim() != 3:
        raise ValueError(f"stitch_windows: the long motions are [G, F, D], got {tuple(x.shape)}")
    G, F, D = x.shape
    out = torch.empty(G * windows, length, D, dtype=torch.float32, device=x.device)
    ffi.check(lib.afm_stitch_windows(x.data_ptr(), out.data_ptr(), G, windows, overlap, length, D, F, ffi.stream_of(x)), "afm_stitch_windows")
    return out


def stitch_join(windows_: torch.Tensor, windows: int, overlap: int, frames: int) -> torch.Tensor:
    """The windows [G * S, L, D] -> [G, F, D] (afm_stitch_join): a shared frame is read from the later window.  Copies."""
    lib = ffi.load()
    ffi.require_gpu(windows_)
    x = ffi.f32c(windows_)
    if x.dim() != 3 or x.shape[0] % windows != 0:
        raise ValueError(f"stitch_join: the windows are [G * {windows}, L, D], got {tuple(x.shape)}")
    B, L, D = x.shape
    out = torch.empty(B // windows, frames, D, dtype=torch.float32, device=x.device)
    ffi.check(lib.afm_stitch_join(x.data_ptr(), out.data_ptr(), B // windows, windows, overlap, L, D, frames, ffi.stream_of(x)), "afm_stitch_join")
    return out


def stitch_step(x0: torch.Tensor, x_t: torch.Tensor, stitch, *, x0_a: Optional[torch.Tensor] = None, x0_u: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None, scale2: Optional[torch.Tensor] = None, known: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, ddim=None, dpm=None, prev: Optional[torch.Tensor] = None, clip: bool = False,
                out: Optional[torch.Tensor] = None, x0_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One stitched sampling update in one launch (afm_stitch_step): x0 (with ``x0_u`` / ``scale``: cfg_combine; with ``x0_a`` /
    ``scale2`` too: cfg2_combine - each window with its own scales), the blend of `stitch_blend` - the neighbour window's branches combined
    with the neighbour's scales - impute with ``known`` / ``mask``, the clamp to [-1, 1] if ``clip``, then the ddim_step expression with
    ``ddim`` = (a, b, c, d) (no noise term) or the dpm_step expression with ``dpm`` = (a, b, c) and ``prev``; ``x0_out`` (dpm only)
    receives the final x0.  Equal, bit for bit, to the chain of separate launches.  ``out`` may be ``x_t``."""
    return _stitch_update("stitch_step", x0, x_t, stitch, x0_a, x0_u, scale, scale2, known, mask, ddim, dpm, prev, clip, out, x0_out)


def stitch_guide_step(x0: torch.Tensor, x_t: torch.Tensor, stitch, *, grad: torch.Tensor, gk: torch.Tensor, x0_a: Optional[torch.Tensor] = None,
                      x0_u: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, scale2: Optional[torch.Tensor] = None,
                      known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, ddim=None, dpm=None,
                      prev: Optional[torch.Tensor] = None, clip: bool = False, out: Optional[torch.Tensor] = None,
                      x0_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`stitch_step` with a cond_fn gradient term, one launch (afm_stitch_guide_step): combine -> blend -> select -> clamp ->
    ``x0 += gk[b] * grad`` (the product rounded, then the sum) -> update.  ``grad`` [B, L, D] and ``gk`` [B] are both required; ``x0_out``
    (DDIM rows too) receives the shifted x0.  Equal, bit for bit, to `stitch_blend` -> `impute` -> clamp -> `guide_step`."""
    if grad is None or gk is None:
        raise ValueError("stitch_guide_step: grad= and gk= are both required")
    return _stitch_update("stitch_guide_step", x0, x_t, stitch, x0_a, x0_u, scale, scale2, known, mask, ddim, dpm, prev, clip, out, x0_out, grad, gk)


def _stitch_update(who, x0, x_t, stitch, x0_a, x0_u, scale, scale2, known, mask, ddim, dpm, prev, clip, out, x0_out, grad=None, gk=None):
    """what `stitch_step` and `stitch_guide_step` share: the checks, the afm_stitch_step_args and the launch"""
    if (ddim is None) == (dpm is None):
        raise ValueError(f"{who}: exactly one of ddim= / dpm= rows")
    if (known is None) != (mask is None):
        raise ValueError(f"{who}: known= and mask= go together")
    if ddim is not None and len(ddim) > 4 and ddim[4] is not None:
        raise ValueError(f"{who}: rows with a noise term are refused - the step noise of shared frames would have to be shared")
    lib = ffi.load()
    ffi.require_gpu(x0, x_t, prev, grad)
    x0, x_t = ffi.f32c(x0), ffi.f32c(x_t)
    st, keep = _stitch_desc(stitch, x0, who)
    keep = [keep]
    B, L, D = x0.shape
    if x_t.shape != x0.shape:
        raise ValueError(f"{who}: x_t {tuple(x_t.shape)} must have x0's shape {tuple(x0.shape)}")
    out = torch.empty_like(x0) if out is None else out
    a = ffi.StitchStepArgs()
    a.x0_c, a.x_t, a.x_next, a.stitch = x0.data_ptr(), x_t.data_ptr(), out.data_ptr(), C.pointer(st)
    extra = {}                      # grad / gk: arguments of afm_stitch_guide_step, not fields of the struct
    for name, t in (("x0_a", x0_a), ("x0_u", x0_u), ("known", known), ("x0_prev", prev), ("grad", grad)):
        if t is not None:
            t = ffi.f32c(t)
            if t.shape != x0.shape:
                raise ValueError(f"{who}: {name} {tuple(t.shape)} must have x0's shape {tuple(x0.shape)}")
            keep.append(t)
            if name == "grad":
                extra[name] = t.data_ptr()
            else:
                setattr(a, name, t.data_ptr())
    for name, t in (("scale", scale), ("scale2", scale2), ("gk", gk)):
        if t is not None:
            t = ffi.f32c(t)
            if t.numel() != B:
                raise ValueError(f"{who}: {name} must hold one value per sample ({B}), got {tuple(t.shape)}")
            keep.append(t)
            if name == "gk":
                extra[name] = t.data_ptr()
            else:
                setattr(a, name, t.data_ptr())
    if mask is not None:
        mask = _mask_u8(mask)
        if mask.shape != x0.shape:
            raise ValueError(f"{who}: mask {tuple(mask.shape)} must have x0's shape {tuple(x0.shape)}")
        a.mask = mask.data_ptr()
    if x0_out is not None:
        if dpm is None and grad is None:
            raise ValueError(f"{who}: x0_out goes with dpm= rows")
        if x0_out.dtype != torch.float32 or x0_out.shape != x0.shape or not x0_out.is_contiguous() or x0_out.device != x0.device:
            raise ValueError(f"{who}: x0_out must be a contiguous float32 tensor of x0's shape {tuple(x0.shape)} on {x0.device}")
        if dpm is not None:
            a.x0_out = x0_out.data_ptr()
    rows = [ffi.f32c(r) for r in (ddim[:4] if ddim is not None else dpm)]
    if any(r.numel() != B for r in rows):
        raise ValueError(f"{who}: the rows hold one value per sample ({B})")
    if ddim is not None:
        rr = ffi.DdimRows(*[r.data_ptr() for r in rows], None)
        a.ddim = C.pointer(rr)
    else:
        rr = ffi.DpmRows(*[r.data_ptr() for r in rows])
        a.dpm = C.pointer(rr)
    keep += rows + [rr]
    a.clip, a.B, a.L, a.D = int(bool(clip)), B, L, D
    if grad is not None:
        ffi.check(lib.afm_stitch_guide_step(C.byref(a), extra["grad"], extra["gk"], ffi.ptr(x0_out), ffi.stream_of(x0)), "afm_stitch_guide_step")
    else:
        ffi.check(lib.afm_stitch_step(C.byref(a), ffi.stream_of(x0)), "afm_stitch_step")
    return out


def long_guidance(guide: "ffi.LongGuide", x: torch.Tensor, t: Optional[torch.Tensor] = None, *, grad: bool = True, energy: bool = False):
    """afm_long_guidance of a filled description (afm.guidance.LongGuidance builds it): -> (grad [G * S, L, D] or None, the contact term's
    energy [G] or None, the targets' energy [G] or None) of the windows x [G * S, L, D]: the windows joined, the terms evaluated on the long
    motion, the gradient handed back to the windows.  ``t`` [G * S] int64 or None (long motion g has t[g * S]).  No atomics; the workspace is
    allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    G = B // max(int(guide.stitch.windows), 1)
    terms = guide.terms.contents
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    ec = torch.empty(G, dtype=torch.float32, device=x.device) if energy and terms.contact else None
    et = torch.empty(G, dtype=torch.float32, device=x.device) if energy and terms.targets else None
    nbytes = int(lib.afm_long_guidance_workspace_bytes(C.byref(guide), B, L, D))
    if nbytes < 0:
        ffi.check(nbytes, "afm_long_guidance_workspace_bytes")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_long_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(ec), ffi.ptr(et), B, L, D, ws.data_ptr(),
                                    ws.numel(), ffi.stream_of(x)), "afm_long_guidance")
    return g, ec, et


def long_scene_guidance(guide: "ffi.LongSceneGuide", x: torch.Tensor, t: Optional[torch.Tensor] = None, *, grad: bool = True, energy: bool = False):
    """afm_long_scene_guidance of a filled description (afm.guidance.LongGuidance with a clearance builds it): -> (grad [G * S, L, D] or None,
    the contact term's energy [G] or None, the targets', the clearance's) of the windows x [G * S, L, D].  grad_long = (grad_contact +
    grad_targets) + grad_clearance on the joined motion - the clearance per window against the window's own cloud, crossfaded per long frame
    - handed back to the windows.  ``t`` [G * S] int64 or None (long motion g has t[g * S]).  The clearance adds 2 launches (h3d: 4); no
    atomics; the workspace is allocated per call."""
    lib = ffi.load()
    ffi.require_gpu(x, t)
    x = ffi.f32c(x)
    B, L, D = x.shape
    base = guide.base.contents
    G = B // max(int(base.stitch.windows), 1)
    terms = base.terms.contents
    tt = None if t is None else t.to(dtype=torch.int64).contiguous()
    g = torch.empty_like(x) if grad else None
    new = lambda on: torch.empty(G, dtype=torch.float32, device=x.device) if energy and on else None
    ec, et, el = new(bool(terms.contact)), new(bool(terms.targets)), new(bool(guide.clearance))
    nbytes = int(lib.afm_long_scene_guidance_workspace_bytes(C.byref(guide), B, L, D))
    if nbytes < 0:
        ffi.check(nbytes, "afm_long_scene_guidance_workspace_bytes")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    ffi.check(lib.afm_long_scene_guidance(C.byref(guide), x.data_ptr(), ffi.ptr(tt), ffi.ptr(g), ffi.ptr(ec), ffi.ptr(et), ffi.ptr(el), B, L, D,
                                          ws.data_ptr(), ws.numel(), ffi.stream_of(x)), "afm_long_scene_guidance")
    return g, ec, et, el
