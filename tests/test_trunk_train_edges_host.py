"""Host side of tests/test_gpu_trunk_train_edges.py: the cases that take the transformer trunk's training path (csrc/train.hip, the training
epilogue of csrc/gemm_epilogue.h, afm_layernorm / afm_masked_mse of csrc/elementwise.hip, afm/autograd.py) to its dropout, dispatch, shape
and value edges, the plain restatements they are compared with (each run in float64 and in float32 on the CPU), and the proof - on the CPU -
that every case is the edge it claims to be and that every float32-class bound the GPU module uses is non-vacuous.

A. Train mode: oracle/denoiser_ref's layers and oracle/train_ref's loss take the keep-masks of oracle/rng_ref.keep_mask at the mask ids
   afm/autograd.py uses; a reference with ONE deliberate fault in one mask must leave the bound (the references have teeth).
B. afm_linear_wgrad: flat_plan / skinny_plan / wgrad_plan of csrc/train.hip are RESTATED here as small pure functions, to be checked
   against the source by eye; every case names the path it must take and the restated plans are asserted to put it there.
C. LayerNorm forward / backward at the edges of the MAXV arms, on the generic arm, past the block cap of ln_bwd_blocks, on value families.
D. masked MSE, afm_rowop, afm_transpose, the training epilogue of afm_linear.

Tolerances are the ones tests/test_gpu_train.py and tests/test_gpu_ops.py state for the same quantities (named below).  For a non-Gaussian
value family the stated tolerance is the Gaussian figure times (float32 reference error on the family / on the Gaussian family of the same
shape), rounded up to a power of two: family_tol.  It is computed from the references alone."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from afm import synth
from afm.cmdm import drop_seed
from conftest import golden
from oracle import denoiser_ref as dr
from oracle import diffusion_ref as df
from oracle import rng_ref
from oracle import shapes as sh
from oracle import train_ref as tr
from test_point_train_edges_host import f32_class_bound, partial_sum_size

MARGIN = 4.0
ULP32 = 2.0 ** -23
F32, F64 = torch.float32, torch.float64
LAYER_FWD_TOL, LAYER_GRAD_TOL = 5e-5, 1e-4                # test_encoder_layer_grads_vs_torch (gradients scaled by the tensor's maximum)
LOSS_TOL, MODEL_GRAD_TOL = 5e-5, 5e-4                     # test_training_losses_backward_with_encoder_and_full_shapes
WGRAD_TOL, LN_TOL = 2e-5, 2e-5                            # test_linear_wgrad, test_layernorm_backward (scaled)
MSE_TOL = 1e-5                                            # tests/test_gpu_ops.py test_masked_mse
GEMM_TOL = 2e-5                                           # tests/test_gpu_ops.py test_linear_thin_layers (here scaled by the maximum)
# an elementwise chain of at most 8 float32 roundings of an O(max) value: 8 * 2^-24 of the maximum (afm_rowop, afm_masked_mse_bwd, act')
ELEMENTWISE_TOL = 1e-6
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3       # afm.ffi.ACT_*
AFM_E_WORKSPACE, AFM_E_UNSUPPORTED = -2, -3


def g(name, shape, seed=synth.NOISE_SEED):
    return synth.gaussian(name, shape, seed=seed)


def pow2ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def max_err(a32, a64, div=1.0):
    return ((a32.double() - a64) / div).abs().max().item()


def family_tol(gauss_tol, err_family, err_gauss):
    """the stated tolerance of a non-Gaussian family (module docstring)"""
    return pow2ceil(gauss_tol * err_family / err_gauss)


def non_vacuous(name, a32, a64, tol, div=1.0, floor_at=None, select=None):
    """report_f32_class's first assertion, on the host: 4 max|ref32 - ref64| + floor < tol"""
    a32, a64 = a32.double() / div, a64 / div
    if select is not None:
        a32, a64 = a32[select], a64[select]
    bound = f32_class_bound(a32, a64, floor_at=floor_at)
    assert bound < tol, f"{name}: bound {bound:.3e} >= {tol:.1e} (vacuous)"
    return bound


def keep_share_ok(mask, p):
    share = (mask != 0).double().mean().item()
    assert abs(share - (1 - p)) < 0.02, (share, p)


# ================================================================================================ A. train mode against the same masks
LB, LH, LD, LFF = 2, 2, 128, 256                          # head dimension 64 (attention_bwd.hip refuses others)
LDH = LD // LH
ENC_ID0 = 16 + 4 * 3
ENC_CASES = {f"T{T}_p{p}_seed{i}": (T, p, seed) for T in (37, 70) for p in (0.1, 0.5) for i, seed in enumerate((1234567, 2 ** 63 + 5))}
DEC_T, DEC_N, DEC_P, DEC_SEED, DEC_ID0 = 37, 70, 0.1, 1234567, 16 + 4 * 3
ENC_IDS = dict(attn=0, drop1=1, ffn=2, drop2=3)
DEC_IDS = dict(attn=0, drop1=1, cross=2, drop2=3, ffn=4, drop3=5)
_ATT = lambda pre: [(pre + ".in_proj_weight", (3 * LD, LD)), (pre + ".in_proj_bias", (3 * LD,)), (pre + ".out_proj.weight", (LD, LD)),
                    (pre + ".out_proj.bias", (LD,))]
_FFN = [("linear1.weight", (LFF, LD)), ("linear1.bias", (LFF,)), ("linear2.weight", (LD, LFF)), ("linear2.bias", (LD,))]
_NORM = lambda i: [(f"norm{i}.weight", (LD,)), (f"norm{i}.bias", (LD,))]
ENC_PARAMS = _ATT("self_attn") + _FFN + _NORM(1) + _NORM(2)
DEC_PARAMS = _ATT("self_attn") + _ATT("multihead_attn") + _FFN + _NORM(1) + _NORM(2) + _NORM(3)


@functools.lru_cache(maxsize=None)
def layer_weights(kind):
    """name -> float32 tensor, by the state-dict names of nn.TransformerEncoderLayer / nn.TransformerDecoderLayer.  Matrices N(0, 1 / d):
    with the 2 / sqrt(d) of test_decoder_layer_fwd_bwd_vs_torch_float64 the float32 CPU reference of the decoder's forward is itself
    1.4e-5 off float64, and 4 x that is no bound below the 5e-5 stated for a layer's forward."""
    out = {}
    for name, shape in (ENC_PARAMS if kind == "enc" else DEC_PARAMS):
        w = g(f"tte_{kind}_{name}", shape) * (LD ** -0.5 if len(shape) > 1 else 0.1)
        out[name] = w + 1.0 if "norm" in name and name.endswith("weight") else w
    return out


@functools.lru_cache(maxsize=None)
def enc_inputs(T):
    km = torch.zeros(LB, T, dtype=torch.bool)
    km[1, T - T // 3:] = True                             # key padding on sample 1
    return dict(x=g(f"tte_enc_x_{T}", (LB, T, LD)), dy=g(f"tte_enc_dy_{T}", (LB, T, LD)), km=km)


@functools.lru_cache(maxsize=None)
def dec_inputs():
    T, n = DEC_T, DEC_N
    km = torch.zeros(LB, T, dtype=torch.bool); km[0, T - T // 3:] = True                # the masks of test_decoder_layer_fwd_bwd_vs_torch_float64
    mm = torch.zeros(LB, n, dtype=torch.bool); mm[LB - 1, n // 2:] = True
    return dict(x=g("tte_dec_x", (LB, T, LD)), mem=g("tte_dec_mem", (LB, n, LD)), dy=g("tte_dec_dy", (LB, T, LD)), km=km, mm=mm)


def with_fault(masks, fault, p, seed, id0, ids, dtype):
    """One deliberate fault in the masks of a layer: (kind, key).  neighbour_id: the mask of `key` drawn with the next site's id (the last
    site: the previous one's); transposed: row and column exchanged in the draw; no_inv_keep: kept elements not scaled; after_pv: the
    attention mask `key` (attn / cross) taken off the probabilities and applied, with the same id and rows, to the head output P V."""
    if fault is None:
        return masks
    kind, key = fault
    m = dict(masks)
    shape = tuple(m[key].shape)
    if kind == "neighbour_id":
        other = ids[key] + 1 if ids[key] + 1 < len(ids) else ids[key] - 1
        m[key] = dr.keep_scale(p, seed, id0 + other, shape, dtype)
    elif kind == "transposed":
        rows, cols = int(np.prod(shape[:-1])), shape[-1]
        keep, inv = rng_ref.keep_mask(p, seed, id0 + ids[key], cols, rows)
        m[key] = (torch.from_numpy(np.ascontiguousarray(keep.T)).to(dtype) * float(inv)).view(shape)
    elif kind == "no_inv_keep":
        m[key] = (m[key] != 0).to(dtype)
    elif kind == "after_pv":
        m[{"attn": "attn_out", "cross": "cross_out"}[key]] = dr.keep_scale(p, seed, id0 + ids[key], shape[:-1] + (LDH,), dtype)
        m[key] = None
    else:
        raise KeyError(kind)
    return m


def layer_faults(ids):
    return [(kind, key) for kind in ("neighbour_id", "transposed", "no_inv_keep") for key in ids] + \
           [("after_pv", key) for key in ids if key in ("attn", "cross")]


def run_layer(kind, i, masks, dtype):
    """forward, and the gradients of sum(out * dy) by autograd, of the oracle's layer in `dtype` -> {out, dx, (dmem,) d<param>}.  Decoder:
    the rows of padded queries (at most T // 3 rows of sample 0: nothing reads them) carry no dy and are left out of out and dx - the
    only exclusion."""
    leaf = {"L." + k: v.to(dtype).clone().requires_grad_(True) for k, v in layer_weights(kind).items()}
    x = i["x"].to(dtype).clone().requires_grad_(True)
    dy = i["dy"].to(dtype)
    if kind == "enc":
        out = dr.encoder_layer(leaf, "L", x, i["km"], LH, masks)
        (out * dy).sum().backward()
        res = dict(out=out.detach(), dx=x.grad)
    else:
        mem = i["mem"].to(dtype).clone().requires_grad_(True)
        out = dr.decoder_layer(leaf, "L", x, mem, i["km"], i["mm"], LH, masks)
        valid = ~i["km"]
        (out * dy * valid[..., None]).sum().backward()
        res = dict(out=out.detach()[valid], dx=x.grad[valid], dmem=mem.grad)
    res.update({"d" + k[2:]: v.grad for k, v in leaf.items()})
    return res


@functools.lru_cache(maxsize=None)
def enc_reference(name, dtype, fault=None):
    T, p, seed = ENC_CASES[name]
    masks = with_fault(dr.encoder_layer_masks(p, seed, ENC_ID0, LB, T, LD, LFF, LH, dtype), fault, p, seed, ENC_ID0, ENC_IDS, dtype)
    return run_layer("enc", enc_inputs(T), masks, dtype)


@functools.lru_cache(maxsize=None)
def dec_reference(dtype, fault=None):
    masks = with_fault(dr.decoder_layer_masks(DEC_P, DEC_SEED, DEC_ID0, LB, DEC_T, DEC_N, LD, LFF, LH, dtype), fault, DEC_P, DEC_SEED,
                       DEC_ID0, DEC_IDS, dtype)
    return run_layer("dec", dec_inputs(), masks, dtype)


def layer_checks(r64):
    """(key, tolerance, divisor) of every tensor of a layer case: the forward as it is, gradients scaled by their maximum"""
    return [(k, LAYER_FWD_TOL, 1.0) if k == "out" else (k, LAYER_GRAD_TOL, max(v.abs().max().item(), 1e-12)) for k, v in r64.items()]


# ---- the whole CMDM: the inputs of test_training_losses_backward_vs_reference_gradients, model.train(), torch.manual_seed(5), first pass
CMDM_P, CMDM_P_POS, CMDM_D, CMDM_FF, CMDM_H, CMDM_LAYERS = 0.1, 0.1, 512, 1024, 8, 5
CMDM_SEED_ARGS = (5, 1, 0)                                 # (torch.initial_seed(), _drop_calls after the pass's increment, rank)


@functools.lru_cache(maxsize=None)
def cmdm_inputs():
    gf, gg = golden("cmdm_forward_N1024_L16"), golden("cmdm_training_grads")
    return dict(sd=sh.weights(sh.cmdm()), x0=g("train_x0", (2, 16, 263)), noise=g("train_noise", (2, 16, 263)), t=gg["t"],
                text=gf["text_feat"], cont=gf["cont_emb"], x_mask=gf["x_mask"])


def cmdm_masks(dtype):
    i = cmdm_inputs()
    T = 2 + i["cont"].shape[1] + i["x0"].shape[1]
    return dr.cmdm_masks(CMDM_P, CMDM_P_POS, drop_seed(*CMDM_SEED_ARGS), i["x0"].shape[0], T, CMDM_D, CMDM_FF, CMDM_H, CMDM_LAYERS, dtype)


@functools.lru_cache(maxsize=None)
def cmdm_reference(dtype, with_masks=True):
    """-> (loss [B], {parameter name: gradient}) of oracle/train_ref in `dtype` with the model's masks"""
    i = cmdm_inputs()
    c = lambda v: v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v
    sd = {k: c(v) for k, v in i["sd"].items()}
    return tr.cmdm_loss_and_grads(sd, df.Schedule(1000), c(i["x0"]), i["t"], c(i["noise"]), c(i["text"]), c(i["cont"]), i["x_mask"],
                                  masks=cmdm_masks(dtype) if with_masks else None)


# ================================================================================================ B. afm_linear_wgrad
def flat_plan(M, N, K):
    """csrc/train.hip flat_plan -> (ok, tn, tk, nwg)"""
    tn, tk, big = (N + 31) // 32, (K + 31) // 32, max(N, K)
    if not (tn * tk <= 12 and big <= 256 and M >= 4096):
        return False, tn, tk, 0
    rb = min((2048 // big) & ~7, 512)
    nblk = (M + rb - 1) // rb
    pbytes = max(M * (N + K) // 2, 4 << 20)
    nwg = max(1, min(1024, pbytes // (N * K * 4)))
    nwg = min(nwg, nblk)
    per = (nblk + nwg - 1) // nwg
    return True, tn, tk, (nblk + per - 1) // per


def skinny_plan(M, N, K):
    """csrc/train.hip skinny_plan -> (ok, tn, tk, nwaves, rows_per_wave)"""
    tn, tk = (N + 31) // 32, (K + 31) // 32
    ok = (tn == 1 and tk in (1, 2, 4, 8)) or (tk == 1 and tn in (2, 4, 8)) or (tn == 2 and tk == 2)
    if tn == 1 and tk == 3: tk, ok = 4, True
    if tk == 1 and tn == 3: tn, ok = 4, True
    if tn == 1 and 4 < tk < 8: tk, ok = 8, True
    if tk == 1 and 4 < tn < 8: tn, ok = 8, True
    ok = ok and M >= 4096
    waves = min((M + 127) // 128, 16384, (64 << 20) // (N * K * 4))
    waves = (max(waves, 4) + 3) // 4 * 4
    return ok, tn, tk, waves, ((M + waves - 1) // waves + 15) // 16 * 16


def tiled_plan(M, N, K):
    """csrc/train.hip wgrad_plan -> (tiles, S, chunks)"""
    RB, WT = 16, 128
    tiles = ((N + WT - 1) // WT) * ((K + WT - 1) // WT)
    S = (768 + tiles - 1) // tiles
    maxS = (M + 4 * RB - 1) // (4 * RB)
    S = min(S, maxS)
    capS = (M * (N + K)) // (2 * N * K)
    if tiles <= 8 and S > capS:
        S = max(capS, 4)
    S = max(1, min(S, maxS, 1024))
    rps = max((((M + S - 1) // S) + RB - 1) // RB * RB, RB)
    return tiles, max(1, (M + rps - 1) // rps), max(1, min(256, (M + 63) // 64))


def wgrad_path(M, N, K, layout="dense", lddw_pad=0, maps=False):
    """afm_linear_wgrad's dispatch -> (path, what the path is, bytes of workspace THAT path asks for).  layout: dense (lddy = N, ldx = K,
    16-byte aligned), offset (dense, 4 bytes past a 16-byte boundary), strided (lddy = N + 3, ldx = K + 5)."""
    ok, tn, tk, nwg = flat_plan(M, N, K)
    if ok and not maps and not lddw_pad and layout == "dense":
        return "flat", (tn, tk), nwg * (N * K + N) * 4
    ok, tn, tk, waves, rpw = skinny_plan(M, N, K)
    if ok and not maps and not lddw_pad:
        return "skinny", (tn, tk), waves * (N * K + N) * 4
    tiles, S, chunks = tiled_plan(M, N, K)
    lddy, ldx = (N + 3, K + 5) if layout == "strided" else (N, K)
    vec = N % 4 == 0 and K % 4 == 0 and lddy % 4 == 0 and ldx % 4 == 0 and layout != "offset"
    return "tiled", ("vec" if vec else "scalar", "S1" if S == 1 else "S>1"), (S * N * K + chunks * N) * 4


def wgrad_workspace_bytes(M, N, K):
    """afm_linear_wgrad_workspace_bytes: the largest of what the three paths ask for, whatever the operands' layout"""
    fok, _, _, nwg = flat_plan(M, N, K)
    sok, _, _, waves, _ = skinny_plan(M, N, K)
    tiles, S, chunks = tiled_plan(M, N, K)
    return 4 * max(S * N * K + chunks * N, waves * (N * K + N) if sok else 0, nwg * (N * K + N) if fok else 0)


# name -> (M, N, K, layout, lddw_pad, maps, family, the path and the arm of it the case must take)
WG_MAPS = {"maps_300x264x512": (5, 60, 64, 3, 70, 10), "maps_300x263x64": (5, 60, 64, 3, 70, 10)}       # B, L, dY rows, off, X rows, off
WG_CASES = {
    # flat: dense, aligned, M >= 4096, tn tk <= 12
    "flat_4096x35x64": (4096, 35, 64, "dense", 0, False, "gaussian", ("flat", (2, 2))),
    "flat_4097x3x3": (4097, 3, 3, "dense", 0, False, "gaussian", ("flat", (1, 1))),
    "flat_4096x128x96": (4096, 128, 96, "dense", 0, False, "gaussian", ("flat", (4, 3))),
    "flat_refused_4096x129x96": (4096, 129, 96, "dense", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),      # 5 x 3 tiles > 12
    # skinny: the flat plan refuses the operands (4-byte offset views, strides), a skinny tile pair exists
    "offset_4096x35x64": (4096, 35, 64, "offset", 0, False, "gaussian", ("skinny", (2, 2))),
    "offset_4097x3x3": (4097, 3, 3, "offset", 0, False, "gaussian", ("skinny", (1, 1))),
    "offset_4096x128x96": (4096, 128, 96, "offset", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),           # no (4, 3) skinny pair
    "strided_4100x3x3": (4100, 3, 3, "strided", 0, False, "gaussian", ("skinny", (1, 1))),
    "strided_5000x64x64": (5000, 64, 64, "strided", 0, False, "gaussian", ("skinny", (2, 2))),
    "strided_4096x32x200": (4096, 32, 200, "strided", 0, False, "gaussian", ("skinny", (1, 8))),
    "strided_4096x200x32": (4096, 200, 32, "strided", 0, False, "gaussian", ("skinny", (8, 1))),
    "strided_4099x96x30": (4099, 96, 30, "strided", 0, False, "gaussian", ("skinny", (4, 1))),
    # tiled: by size, by lddw, by row maps; both load arms; one slice and several
    "tiled_4095x257x64": (4095, 257, 64, "dense", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_300x64x263": (300, 64, 263, "dense", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_4096x263x257": (4096, 263, 257, "dense", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_300x264x512": (300, 264, 512, "dense", 0, False, "gaussian", ("tiled", ("vec", "S>1"))),
    "tiled_offset_300x264x512": (300, 264, 512, "offset", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_offset_300x263x512": (300, 263, 512, "offset", 0, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_lddw_4096x35x64": (4096, 35, 64, "dense", 4, False, "gaussian", ("tiled", ("scalar", "S>1"))),
    "tiled_7x5x3": (7, 5, 3, "dense", 0, False, "gaussian", ("tiled", ("scalar", "S1"))),
    "tiled_lddw_7x5x3": (7, 5, 3, "dense", 4, False, "gaussian", ("tiled", ("scalar", "S1"))),
    "maps_300x264x512": (300, 264, 512, "dense", 0, True, "gaussian", ("tiled", ("vec", "S>1"))),
    "maps_300x263x64": (300, 263, 64, "dense", 0, True, "gaussian", ("tiled", ("scalar", "S>1"))),
}
WG_FAMILIES = ("gaussian", "offset", "alternating", "columns")
WG_FAMILY_SHAPES = {(20000, 35, 64): ("flat", (2, 2)), (300, 263, 64): ("tiled", ("scalar", "S>1"))}
for _shape, _path in WG_FAMILY_SHAPES.items():
    for _fam in WG_FAMILIES:
        WG_CASES["family_%s_%dx%dx%d" % ((_fam,) + _shape)] = _shape + ("dense", 0, False, _fam, _path)


@functools.lru_cache(maxsize=None)
def wg_inputs(name):
    """dY [M, N], X [M, K] (float32, the logical rows: the GPU module lays them out)"""
    M, N, K, _, _, _, fam, _ = WG_CASES[name]
    dy, x = g(f"tte_wg_dy_{M}_{N}", (M, N)), g(f"tte_wg_x_{M}_{K}", (M, K))
    if fam == "offset":
        dy = 1.0 + 0.01 * dy
    elif fam == "alternating":                            # terms +-(1 + small): they cancel to the size of one term
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
        dy, x = sign * (1.0 + 0.003 * dy), 1.0 + 0.003 * x
    elif fam == "columns":
        dy = dy * torch.logspace(-4, 3, N)[None, :]
    return dy.contiguous(), x.contiguous()


@functools.lru_cache(maxsize=None)
def wg_reference(name, dtype):
    dy, x = wg_inputs(name)
    return dict(dW=dy.to(dtype).t() @ x.to(dtype), db=dy.to(dtype).sum(0))


@functools.lru_cache(maxsize=None)
def wg_partial_sizes(name):
    """-> ([N] max over k and j of |sum_{m <= j} dY[m, n] X[m, k]|, [N] max over j of |sum_{m <= j} dY[m, n]|), float64"""
    dy, x = (t.double() for t in wg_inputs(name))
    pw = torch.stack([(dy[:, n: n + 1] * x).cumsum(0).abs().max() for n in range(dy.shape[1])])
    return pw, dy.cumsum(0).abs().max(0).values


def wg_divisors(name):
    """dW and db are compared after division by the tensor's float64 maximum; the `columns` family column by column (row n of dW, entry n
    of db), by the column's own maximum - for db[n], one number, by the size of its largest partial sum - so that a wrong small column
    cannot hide under a large one."""
    r64 = wg_reference(name, F64)
    if WG_CASES[name][6] == "columns":
        return dict(dW=r64["dW"].abs().max(1, keepdim=True).values.clamp_min(1e-300), db=wg_partial_sizes(name)[1].clamp_min(1e-300))
    return dict(dW=max(r64["dW"].abs().max().item(), 1e-12), db=max(r64["db"].abs().max().item(), 1e-12))


@functools.lru_cache(maxsize=None)
def wg_checks(name):
    """[(key, tolerance, divisor, floor_at)].  The value families state floor_at, the size of the largest partial sum in row order
    (tests/test_point_train_edges_host.py partial_sum_size) over the divisor; the Gaussian shape cases keep the plain floor."""
    M, N, K, _, _, _, fam, _ = WG_CASES[name]
    div = wg_divisors(name)
    if not name.startswith("family_"):
        return [("dW", WGRAD_TOL, div["dW"], None), ("db", WGRAD_TOL, div["db"], None)]
    pw, pb = wg_partial_sizes(name)
    floors = dict(dW=(pw / (div["dW"].flatten() if fam == "columns" else div["dW"])).max().item(),
                  db=(pb / div["db"]).max().item())
    out = []
    gauss = "family_gaussian_%dx%dx%d" % (M, N, K)
    for key in ("dW", "db"):
        tol = WGRAD_TOL
        if fam != "gaussian":
            e_f = max_err(wg_reference(name, F32)[key], wg_reference(name, F64)[key], div[key])
            e_g = max_err(wg_reference(gauss, F32)[key], wg_reference(gauss, F64)[key], wg_divisors(gauss)[key])
            tol = family_tol(WGRAD_TOL, e_f, e_g)
        out.append((key, tol, div[key], max(floors[key], 1.0)))
    return out


# ================================================================================================ C. LayerNorm
LN_EPS = 1e-5
LN_BOTH = (4, 252, 256, 260, 508, 512, 516, 1020, 1024)
LN_FWD_ONLY = (1028, 2044, 2048)
LN_GENERIC = (1, 3, 63, 65, 1023)
LN_ROWS = (1, 3, 4, 5, 8193)                              # and 0, which has no reference: dgamma = dbeta = 0
LN_ROW_DIMS = (256, 516, 63)
LN_FAMILIES = ("gaussian", "offset_100", "near_eps", "scale_1e4", "outlier", "constant_row")
LN_FAMILY_DIMS, LN_FAMILY_ROWS, LN_CONST_ROW, LN_CONST = (512, 260), 37, 5, 3.25
LN_EXACT_DIMS = (256, 512, 1024)                          # a constant row's sums are exact: y == beta


def ln_arm(dim, aligned=True):
    """afm_layernorm_rows / afm_layernorm_bwd: the generic kernels for dim % 4 != 0 or a pointer off a 16-byte boundary, else MAXV"""
    if dim % 4 or not aligned:
        return "generic"
    return 1 if dim <= 256 else 2 if dim <= 512 else 4 if dim <= 1024 else 8


def ln_bwd_trips(rows):
    """ln_bwd_blocks: min(512, ceil(rows / 16)) blocks of 4 waves, one row per wave and trip -> (trips, rows of the last trip)"""
    per = max(1, min(512, (rows + 15) // 16)) * 4
    trips = (rows + per - 1) // per
    return trips, rows - (trips - 1) * per


def ln_cases():
    """name -> (rows, dim, family, 4-byte offset views, has a backward)"""
    cases = {}
    for dim in LN_BOTH + LN_FWD_ONLY + LN_GENERIC:
        cases[f"shape_5x{dim}"] = (5, dim, "gaussian", False, dim <= 1024)
    cases["offset_view_5x512"] = (5, 512, "gaussian", True, True)
    for rows in LN_ROWS:
        for dim in LN_ROW_DIMS:
            cases[f"shape_{rows}x{dim}"] = (rows, dim, "gaussian", False, True)
    for dim in LN_FAMILY_DIMS:
        for fam in LN_FAMILIES:
            cases[f"family_{fam}_{LN_FAMILY_ROWS}x{dim}"] = (LN_FAMILY_ROWS, dim, fam, False, True)
    for dim in LN_EXACT_DIMS:
        cases[f"exact_constant_row_8x{dim}"] = (8, dim, "constant_row", False, True)
    return cases


@functools.lru_cache(maxsize=None)
def ln_inputs(name):
    rows, dim, fam, _, _ = ln_cases()[name]
    z = g(f"tte_ln_x_{rows}_{dim}", (rows, dim))
    x = {"gaussian": z, "offset_100": 100.0 + z, "near_eps": 3.0 + 1e-3 * z, "scale_1e4": 1e4 * z}.get(fam, z).clone()
    if fam == "outlier":
        x[torch.arange(rows), (7 * torch.arange(rows)) % dim] = 1e3
    if fam == "constant_row":
        x[LN_CONST_ROW] = LN_CONST
    return dict(x=x, gamma=1 + 0.1 * g(f"tte_ln_g_{dim}", (dim,)), beta=0.1 * g(f"tte_ln_b_{dim}", (dim,)), dy=g(f"tte_ln_dy_{rows}_{dim}", (rows, dim)))


def ln_restatement(x, gamma, beta, dy, dtype, variant=None):
    """y = (x - mean) rstd gamma + beta over the last dimension and the gradients of sum(y dy), in `dtype`.  variant: the two wrong
    forwards the host proofs tell from the right one - `one_pass` (variance as E[x^2] - mean^2), `no_eps`."""
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    if variant is None and x.shape[-1] == 1:              # (torch's own backward at width 1 returns a non-zero dx in float64; the composition does not)
        variant = "two_pass"
    if variant is None:
        y = F.layer_norm(x, (x.shape[-1],), gamma, beta, LN_EPS)
    else:
        mean = x.mean(-1, keepdim=True)
        var = (x * x).mean(-1, keepdim=True) - mean * mean if variant == "one_pass" else ((x - mean) ** 2).mean(-1, keepdim=True)
        y = (x - mean) / torch.sqrt(var + (0.0 if variant == "no_eps" else LN_EPS)) * gamma + beta
    (y * dy.to(dtype)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


@functools.lru_cache(maxsize=None)
def ln_reference(name, dtype):
    i = ln_inputs(name)
    return ln_restatement(i["x"], i["gamma"], i["beta"], i["dy"], dtype)


@functools.lru_cache(maxsize=None)
def ln_checks(name):
    """[(key, tolerance, divisor, floor_at)]: every quantity scaled by its float64 maximum; dgamma and dbeta, sums over the rows, with the
    size of their largest partial sum as floor_at.  Width 1 is exactly zero in dx and dgamma, and zero is the point: dgamma = sum dy xhat
    with xhat = 0 whatever the arithmetic keeps divisor 1e-12 (only an exactly zero result is in its class); dx = rstd (dy gamma -
    mean(dy gamma)) is what is left of two equal terms of size eps^-1/2 |dy gamma| after they cancel - a fused multiply-subtract leaves
    the rounding of the product -, so it is divided by the largest such term and its floor is one ulp of it."""
    rows, dim, fam, _, has_bwd = ln_cases()[name]
    i, r32, r64 = ln_inputs(name), ln_reference(name, F32), ln_reference(name, F64)
    x = i["x"].double()
    xhat = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + LN_EPS)
    psize = dict(dgamma=partial_sum_size(i["dy"].double() * xhat), dbeta=partial_sum_size(i["dy"]))
    out = []
    for key in ("y", "dx", "dgamma", "dbeta") if has_bwd else ("y",):
        div = max(r64[key].abs().max().item(), 1e-12)
        tol = LN_TOL
        if fam != "gaussian":
            gname = (f"family_gaussian_{rows}x{dim}" if name.startswith("family_") else f"shape_5x{dim}")
            gd = max(ln_reference(gname, F64)[key].abs().max().item(), 1e-12)
            tol = family_tol(LN_TOL, max_err(r32[key], r64[key], div), max_err(ln_reference(gname, F32)[key], ln_reference(gname, F64)[key], gd))
        floor_at = max(psize[key] / div, 1.0) if key in psize and div > 1e-12 else None
        if key == "dx" and dim == 1:
            div, floor_at = LN_EPS ** -0.5 * (i["dy"] * i["gamma"]).abs().max().item(), 1.0
        out.append((key, tol, div, floor_at))
    return out


LN_ROWS_MAPS = [(37, 256, (5, 9, 2)), (37, 516, (12, 12, 0)), (10, 1028, (3, 7, 4))]         # rows, dim, (grp, stride, off)


def mapped_rows(rows, grp, stride, off):
    r = torch.arange(rows)
    return (r // grp) * stride + off + r % grp


# ================================================================================================ D. loss, glue, epilogue
MSE_SHAPES = [(1, 1, 1), (3, 65, 263), (2, 257, 7)]
MSE_MASKS = ("none", "mixed", "one_valid", "full_sample")
MSE_DLOSS = (0.5, -1.25, 2.0)                             # a different number per sample


@functools.lru_cache(maxsize=None)
def mse_inputs(B, L, D, kind):
    gen = torch.Generator().manual_seed(7 + L + D)
    mask = None
    if kind != "none":
        mask = torch.rand(B, L, generator=gen) < 0.4
        mask[:, L // 2] = False                           # every sample keeps a frame
        if kind == "one_valid":
            mask[:] = True
            mask[torch.arange(B), (3 * torch.arange(B) + 1) % L] = False
        if kind == "full_sample":
            mask[B - 1] = True
    return dict(target=g(f"tte_mse_t_{B}_{L}_{D}", (B, L, D)), pred=g(f"tte_mse_p_{B}_{L}_{D}", (B, L, D)), mask=mask,
                dloss=torch.tensor(MSE_DLOSS[:B]))


def mse_restatement(i, dtype, dloss_index=None):
    """loss[b] = sum((t - p)^2 keep) / (sum(keep) D) (NaN for a sample without a frame, as the torch expression), dpred = 2 dloss[b]
    (p - t) keep / (sum(keep) D) with the rows of masked frames exactly 0.  dloss_index: the wrong backward that reads dloss[0] for
    every sample."""
    t, p = i["target"].to(dtype), i["pred"].to(dtype)
    keep = torch.ones(t.shape[:2], dtype=dtype) if i["mask"] is None else (~i["mask"]).to(dtype)
    cnt = keep.sum(1) * t.shape[-1]
    loss = ((t - p) ** 2 * keep[..., None]).sum((1, 2)) / cnt
    dl = i["dloss"].to(dtype) if dloss_index is None else i["dloss"].to(dtype)[dloss_index].expand(t.shape[0])
    coef = 2.0 * dl / cnt
    dpred = torch.where(keep[..., None] > 0, coef[:, None, None] * (p - t), torch.zeros((), dtype=dtype))
    return dict(loss=loss, dpred=dpred)


ROWOP_ROWS, ROWOP_PERIOD, ROWOP_COLS, ROWOP_DROP = 37, 5, 70, (0.25, 99, 7)
ROWOP_BIG = (4097, 256)                                    # rows cols = 4096 * 256 + cols: one row of a second grid-stride trip
ROWOP_COMBOS = [(tab, act, drop) for tab in (False, True) for act in (ACT_NONE, ACT_GELU, ACT_SILU, ACT_RELU) for drop in (False, True)]
ACT_LADDER = [0.0] + [s * v for v in (1e-30, 1.0, 5.0, 10.0, 40.0, 88.0, 100.0, 1e4) for s in (1.0, -1.0)]


def act_grad(z, act):
    """d act(z) / dz by torch's autograd in z's dtype"""
    z = z.clone().requires_grad_(True)
    {ACT_GELU: F.gelu, ACT_SILU: F.silu, ACT_RELU: F.relu}[act](z).sum().backward()
    return z.grad


@functools.lru_cache(maxsize=None)
def rowop_inputs(rows, cols):
    z = g(f"tte_ro_z_{rows}_{cols}", (rows, cols)) * 2.0
    z = torch.where(z.abs() < 1e-3, torch.full_like(z, 0.5), z)            # nothing on ReLU's kink but the exact zeros below
    z[::3, ::5] = 0.0
    return dict(x=g(f"tte_ro_x_{rows}_{cols}", (rows, cols)), tab=g(f"tte_ro_t_{cols}", (ROWOP_PERIOD, cols)), z=z)


def rowop_restatement(i, tab, act, drop, dtype):
    """out = (x + rowtab[row % period]) act'(z) keep, each part optional"""
    x = i["x"].to(dtype)
    rows, cols = x.shape
    v = x + i["tab"].to(dtype)[torch.arange(rows) % ROWOP_PERIOD] if tab else x
    if act:
        v = v * act_grad(i["z"].to(dtype), act)
    return v * dr.keep_scale(*ROWOP_DROP, (rows, cols), dtype) if drop else v


TRANSPOSE_SHAPES = [(1, 1), (1, 77), (77, 1), (31, 33), (32, 32), (33, 31), (65, 97)]

EPI_SHAPES = {(129, 192, 128): ("vector", (43, 50, 4)), (33, 263, 64): ("scalar", (11, 16, 3))}        # (M, N, K): arm, c_map (grp, stride, off)
EPI_VARIANTS = ("preact", "dact", "drop_before", "drop_after", "act_drop", "drop_dact", "c_map")
EPI_DROP = (0.25, 2 ** 63 + 5, 9)


@functools.lru_cache(maxsize=None)
def epi_inputs(M, N, K):
    z = g(f"tte_ep_z_{M}_{N}", (M, N)) * 2.0
    return dict(A=g(f"tte_ep_a_{M}_{K}", (M, K)), W=g(f"tte_ep_w_{N}_{K}", (N, K)) * (K ** -0.5), bias=0.1 * g(f"tte_ep_b_{N}", (N,)),
                res=g(f"tte_ep_r_{M}_{N}", (M, N)), z=z)


@functools.lru_cache(maxsize=None)
def epi_reference(M, N, K, variant, dtype):
    """The epilogue's order (csrc/gemm_epilogue.h): bias, preact store, act, drop (drop_after = 0), act'(dact_z), residual, drop
    (drop_after = 1) -> {out, (preact)}"""
    i = epi_inputs(M, N, K)
    v = i["A"].to(dtype) @ i["W"].to(dtype).t()
    keep = dr.keep_scale(*EPI_DROP, (M, N), dtype)
    if variant == "preact":
        v = v + i["bias"].to(dtype)
        return dict(out=F.gelu(v), preact=v)
    if variant == "dact":
        return dict(out=v * act_grad(i["z"].to(dtype), ACT_GELU))
    if variant == "drop_before":
        return dict(out=v * keep + i["res"].to(dtype))
    if variant == "drop_after":
        return dict(out=(v + i["res"].to(dtype)) * keep)
    if variant == "act_drop":
        return dict(out=F.gelu(v + i["bias"].to(dtype)) * keep)
    if variant == "drop_dact":
        return dict(out=v * keep * act_grad(i["z"].to(dtype), ACT_GELU))
    if variant == "c_map":
        grp, stride, off = EPI_SHAPES[M, N, K][1]
        out = torch.zeros((M + grp - 1) // grp * stride, N, dtype=dtype)
        out[mapped_rows(M, grp, stride, off)] = v
        return dict(out=out)
    raise KeyError(variant)


# ================================================================================================ the proofs
def test_seed_helper_returns_the_pinned_values():
    assert drop_seed(5, 1, 0) == 0x9E3779B97F4A7C1A
    assert drop_seed(0, 2, 0) == 0x3C6EF372FE94F82A                      # wraps modulo 2^64
    assert drop_seed(2 ** 64 - 1, 0, 1) == 0xD1B54A32D192ED02
    assert drop_seed(*CMDM_SEED_ARGS) == drop_seed(5, 1)


@pytest.mark.parametrize("name", sorted(ENC_CASES))
def test_encoder_layer_case_is_not_vacuous_and_its_reference_has_teeth(name):
    T, p, seed = ENC_CASES[name]
    for key, m in dr.encoder_layer_masks(p, seed, ENC_ID0, LB, T, LD, LFF, LH).items():
        keep_share_ok(m, p)
    r32, r64 = enc_reference(name, F32), enc_reference(name, F64)
    assert len(r64) == 2 + 12
    bounds = {}
    for key, tol, div in layer_checks(r64):
        assert r64[key].abs().max().item() > 0
        bounds[key] = non_vacuous(f"{name} {key}", r32[key], r64[key], tol, div)
    for fault in layer_faults(ENC_IDS):
        bad = enc_reference(name, F64, fault)
        assert any(max_err(bad[key], r64[key], div) > bounds[key] for key, _, div in layer_checks(r64)), f"{name}: {fault} stays in the bound"


def test_decoder_layer_case_is_not_vacuous_and_its_reference_has_teeth():
    i = dec_inputs()
    assert 0 < int(i["km"].sum()) <= DEC_T // 3 and int(i["km"][1:].sum()) == 0          # the excluded rows: at most T // 3 of one sample
    for key, m in dr.decoder_layer_masks(DEC_P, DEC_SEED, DEC_ID0, LB, DEC_T, DEC_N, LD, LFF, LH).items():
        keep_share_ok(m, DEC_P)
    r32, r64 = dec_reference(F32), dec_reference(F64)
    assert len(r64) == 3 + 18
    bounds = {}
    for key, tol, div in layer_checks(r64):
        assert r64[key].abs().max().item() > 0
        bounds[key] = non_vacuous(f"decoder {key}", r32[key], r64[key], tol, div)
    for fault in layer_faults(DEC_IDS):
        bad = dec_reference(F64, fault)
        assert any(max_err(bad[key], r64[key], div) > bounds[key] for key, _, div in layer_checks(r64)), f"decoder: {fault} stays in the bound"


def test_oracle_default_is_unchanged_by_the_mask_arguments():
    """masks that keep everything with inv_keep = 1 (p = 0) give the bits of the call without masks"""
    i, sd = enc_inputs(37), {"L." + k: v for k, v in layer_weights("enc").items()}
    ones = dr.encoder_layer_masks(0.0, 1, ENC_ID0, LB, 37, LD, LFF, LH)
    assert all((m == 1).all() for m in ones.values())
    assert torch.equal(dr.encoder_layer(sd, "L", i["x"], i["km"], LH, ones), dr.encoder_layer(sd, "L", i["x"], i["km"], LH))
    j, sdd = dec_inputs(), {"L." + k: v for k, v in layer_weights("dec").items()}
    ones = dr.decoder_layer_masks(0.0, 1, DEC_ID0, LB, DEC_T, DEC_N, LD, LFF, LH)
    assert torch.equal(dr.decoder_layer(sdd, "L", j["x"], j["mem"], j["km"], j["mm"], LH, ones),
                       dr.decoder_layer(sdd, "L", j["x"], j["mem"], j["km"], j["mm"], LH))
    c = cmdm_inputs()
    T = 2 + c["cont"].shape[1] + 16
    ones = dr.cmdm_masks(0.0, 0.0, 1, 2, T, CMDM_D, CMDM_FF, CMDM_H, CMDM_LAYERS)
    args = (c["sd"], c["x0"], c["t"], c["text"])
    assert torch.equal(dr.cmdm_forward(*args, x_mask=c["x_mask"], cont_emb=c["cont"], masks=ones),
                       dr.cmdm_forward(*args, x_mask=c["x_mask"], cont_emb=c["cont"]))


def test_cmdm_case_is_not_vacuous_and_the_masks_matter():
    m = cmdm_masks(F32)
    keep_share_ok(m["pos"], CMDM_P_POS)
    assert len(m["layers"]) == CMDM_LAYERS
    for lm in m["layers"]:
        for mask in lm.values():
            keep_share_ok(mask, CMDM_P)
    (l32, g32), (l64, g64) = cmdm_reference(F32), cmdm_reference(F64)
    assert len(g64) == 72 and set(g32) == set(g64)
    lb = non_vacuous("CMDM train-mode loss", l32, l64, LOSS_TOL)
    bounds = {}
    for k, v in g64.items():
        div = max(v.abs().max().item(), 1e-12)
        assert v.abs().max().item() > 0, k
        bounds[k] = non_vacuous(f"CMDM train-mode d{k}", g32[k], v, MODEL_GRAD_TOL, div)
    # eval mode (no masks) is far outside: the train-mode reference is not the one the suite already had
    l_eval, g_eval = cmdm_reference(F64, False)
    assert (l_eval - l64).abs().max().item() > 100 * lb
    assert all(max_err(g_eval[k], v, max(v.abs().max().item(), 1e-12)) > bounds[k] for k, v in g64.items() if "bias" not in k or "motion_layer" not in k)


def test_wgrad_every_case_takes_the_path_it_names():
    seen = set()
    for name, (M, N, K, layout, pad, maps, fam, want) in WG_CASES.items():
        path, arm, need = wgrad_path(M, N, K, layout, pad, maps)
        assert (path, arm) == want, (name, path, arm)
        assert need > 0
        seen.add((path, arm))
    assert {("flat", (1, 1)), ("flat", (2, 2)), ("flat", (4, 3))} <= seen
    assert {("skinny", t) for t in ((1, 1), (2, 2), (1, 8), (8, 1), (4, 1))} <= seen                  # (3 -> 4, 1) and (1, 7 -> 8) among them
    assert {("tiled", (a, s)) for a in ("vec", "scalar") for s in ("S1", "S>1")} - seen == {("tiled", ("vec", "S1"))}
    # the flat plan refuses 129 x 96 by its tile product alone
    assert flat_plan(4096, 129, 96)[:3] == (False, 5, 3) and flat_plan(4096, 128, 96)[0]
    # a last wave that holds no row: rows_per_wave * (nwaves - 1) >= M
    empty = [name for name, c in WG_CASES.items() if wgrad_path(*c[:6])[0] == "skinny" and
             skinny_plan(*c[:3])[4] * (skinny_plan(*c[:3])[3] - 1) >= c[0]]
    assert "strided_4100x3x3" in empty, empty
    for name, (B, L, ty, offy, tx, offx) in WG_MAPS.items():
        assert B * L == WG_CASES[name][0] and offy + L <= ty and offx + L <= tx and WG_CASES[name][5]


@pytest.mark.parametrize("name", sorted(WG_CASES))
def test_wgrad_bounds_are_not_vacuous(name):
    r32, r64 = wg_reference(name, F32), wg_reference(name, F64)
    fam = WG_CASES[name][6]
    for key, tol, div, floor_at in wg_checks(name):
        assert r64[key].abs().max().item() > 0
        non_vacuous(f"{name} {key}", r32[key], r64[key], tol, div, floor_at)
    if fam == "alternating":                              # the terms cancel to the size of one term
        pw, pb = wg_partial_sizes(name)
        assert r64["db"].abs().max().item() < 4.0 and r64["dW"].abs().max().item() < 4.0 and pw.max().item() < 4.0
    if fam == "columns":
        dy, _ = wg_inputs(name)
        top = dy.abs().max(0).values
        assert top[-1] / top[0] > 1e6
    if fam == "offset":
        assert (wg_inputs(name)[0].mean().item() - 1.0) < 1e-3


def test_layernorm_cases_reach_every_arm():
    cases = ln_cases()
    arm = {name: ln_arm(c[1], not c[3]) for name, c in cases.items()}
    for dim, want in ((4, 1), (252, 1), (256, 1), (260, 2), (508, 2), (512, 2), (516, 4), (1020, 4), (1024, 4), (1028, 8), (2044, 8), (2048, 8)):
        assert arm[f"shape_5x{dim}"] == want
    for dim in LN_GENERIC:
        assert arm[f"shape_5x{dim}"] == "generic"
    assert arm["offset_view_5x512"] == "generic"
    assert ln_bwd_trips(8193) == (5, 1) and ln_bwd_trips(8192) == (4, 2048) and ln_bwd_trips(5) == (2, 1)
    assert not any(cases[f"shape_5x{dim}"][4] for dim in LN_FWD_ONLY)
    for rows, dim, (grp, stride, off) in LN_ROWS_MAPS:
        rr = mapped_rows(rows, grp, stride, off)
        assert len(set(rr.tolist())) == rows and ln_arm(dim) != "generic"


@pytest.mark.parametrize("name", sorted(ln_cases()))
def test_layernorm_bounds_are_not_vacuous_and_families_are_what_they_claim(name):
    rows, dim, fam, _, has_bwd = ln_cases()[name]
    i, r32, r64 = ln_inputs(name), ln_reference(name, F32), ln_reference(name, F64)
    for key, tol, div, floor_at in ln_checks(name):
        assert dim == 1 or r64[key].abs().max().item() > 0
        non_vacuous(f"{name} {key}", r32[key], r64[key], tol, div, floor_at)
    x = i["x"].double()
    var = x.var(-1, unbiased=False)
    if fam == "near_eps":
        assert 0.05 < (var / LN_EPS).min().item() and (var / LN_EPS).max().item() < 0.2
    if fam == "constant_row":
        assert (i["x"][LN_CONST_ROW] == LN_CONST).all() and var[LN_CONST_ROW] == 0
        assert torch.equal(r32["y"][LN_CONST_ROW], i["beta"]) or name.startswith("family_")
    if fam == "outlier":
        assert ((i["x"] == 1e3).sum(1) == 1).all()


@pytest.mark.parametrize("dim", LN_FAMILY_DIMS)
def test_layernorm_families_have_teeth(dim):
    def fails(name, variant, dtype):
        i, r32, r64 = ln_inputs(name), ln_reference(name, F32), ln_reference(name, F64)
        bad = ln_restatement(i["x"], i["gamma"], i["beta"], i["dy"], dtype, variant)
        key, tol, div, floor_at = ln_checks(name)[0]
        assert key == "y"
        bound = f32_class_bound(r32["y"].double() / div, r64["y"] / div)
        return not torch.isfinite(bad["y"]).all() or max_err(bad["y"], r64["y"], div) > bound
    tag = f"{LN_FAMILY_ROWS}x{dim}"
    assert fails(f"family_offset_100_{tag}", "one_pass", F32), "a one-pass float32 variance stays in the bound at 100 + g"
    assert not fails(f"family_offset_100_{tag}", None, F32)
    assert fails(f"family_near_eps_{tag}", "no_eps", F64) and fails(f"family_constant_row_{tag}", "no_eps", F64)


@pytest.mark.parametrize("B,L,D", MSE_SHAPES)
@pytest.mark.parametrize("kind", MSE_MASKS)
def test_masked_mse_cases(B, L, D, kind):
    i = mse_inputs(B, L, D, kind)
    assert len(set(i["dloss"].tolist())) == B
    r32, r64 = mse_restatement(i, F32), mse_restatement(i, F64)
    live = torch.ones(B, dtype=torch.bool) if kind != "full_sample" else torch.arange(B) < B - 1
    if kind == "full_sample":
        assert i["mask"][B - 1].all() and torch.isnan(r64["loss"][B - 1]) and torch.isnan(r32["loss"][B - 1])
        assert (r64["dpred"][B - 1] == 0).all()
    if kind == "one_valid":
        assert ((~i["mask"]).sum(1) == 1).all()
    if kind == "mixed" and L > 1:
        assert i["mask"].any() and (~i["mask"]).any()
    if live.any():
        non_vacuous("masked mse loss", r32["loss"], r64["loss"], MSE_TOL, select=live)
        div = max(r64["dpred"][live].abs().max().item(), 1e-12)
        bound = non_vacuous("masked mse dpred", r32["dpred"], r64["dpred"], ELEMENTWISE_TOL, div, select=live)
        if B > 1 and live.sum() > 1:                      # dloss[0] for every sample leaves the bound
            bad = mse_restatement(i, F64, dloss_index=0)
            assert max_err(bad["dpred"][live], r64["dpred"][live], div) > 100 * bound


def test_rowop_and_activation_ladder_bounds():
    assert ROWOP_ROWS % ROWOP_PERIOD and ROWOP_BIG[0] * ROWOP_BIG[1] == 4096 * 256 + ROWOP_BIG[1]
    keep_share_ok(dr.keep_scale(*ROWOP_DROP, (ROWOP_ROWS, ROWOP_COLS)), ROWOP_DROP[0])
    i = rowop_inputs(ROWOP_ROWS, ROWOP_COLS)
    assert (i["z"] == 0).any() and (i["z"] > 0).any() and (i["z"] < 0).any()
    for tab, act, drop in ROWOP_COMBOS:
        r32, r64 = rowop_restatement(i, tab, act, drop, F32), rowop_restatement(i, tab, act, drop, F64)
        non_vacuous(f"rowop {tab} {act} {drop}", r32, r64, ELEMENTWISE_TOL, max(r64.abs().max().item(), 1e-12))
    z = torch.tensor(ACT_LADDER)
    assert len(ACT_LADDER) == 17
    for act in (ACT_GELU, ACT_SILU, ACT_RELU):
        d32, d64 = act_grad(z, act), act_grad(z.double(), act)
        assert torch.isfinite(d32).all() and torch.isfinite(d64).all()
        non_vacuous(f"act' {act} ladder", d32, d64, ELEMENTWISE_TOL)
    assert act_grad(z, ACT_RELU)[0] == 0


@pytest.mark.parametrize("M,N,K", sorted(EPI_SHAPES))
def test_epilogue_bounds_are_not_vacuous(M, N, K):
    arm, (grp, stride, off) = EPI_SHAPES[M, N, K]
    assert (arm == "vector") == (N % 4 == 0) and M % grp == 0 and off + grp <= stride
    keep = dr.keep_scale(*EPI_DROP, (M, N))
    keep_share_ok(keep, EPI_DROP[0])
    for variant in EPI_VARIANTS:
        r32, r64 = epi_reference(M, N, K, variant, F32), epi_reference(M, N, K, variant, F64)
        for key in r64:
            non_vacuous(f"epilogue {variant} {key}", r32[key], r64[key], GEMM_TOL, max(r64[key].abs().max().item(), 1e-12))
    # drop_before and drop_after differ where the mask drops (the residual survives one and not the other)
    a, b = epi_reference(M, N, K, "drop_before", F64)["out"], epi_reference(M, N, K, "drop_after", F64)["out"]
    assert ((a != b) | (keep != 0)).all() and (a[keep == 0] == epi_inputs(M, N, K)["res"].double()[keep == 0]).all() and (b[keep == 0] == 0).all()
