"""Host side of tests/test_gpu_point_infer_edges.py: the inference half of the scene branch (csrc/pointnet.hip: afm_transition_down and
afm_pt_attention; the non-training entry points of csrc/pointops.hip: afm_knn, afm_knn_ws, afm_fps, afm_segment_mean, afm_gather_rows;
afm_bn_fold of csrc/elementwise.hip) at its shape, dispatch and value edges.

This module builds the cases, holds the plain restatements they are compared with - functions of exactly what the C entry points take,
run in float64 and in float32 on the CPU - and proves on the CPU that
  * the two fused kernels' restatements ARE the reference's layers: through the goldens pt_block_c32_k8 / pt_block_c64_k16 (layer_out) and
    transition_down_s4 / transition_down_s8 (y), at the 2e-5 the oracle holds against the reference;
  * the dispatch rules of afm_pt_attention and the tile arithmetic of afm_transition_down, RESTATED here as small pure functions (to be
    checked against the source by eye), are reached in every arm by the lists of cases;
  * every value family is the edge it claims to be;
  * the extended oracle (oracle/pointops_ref.py::knn_query, "the kNN / FPS contract") changes nothing on finite input and, for an untouched
    query with at least k candidates at a finite distance, gives the neighbours of the sample with the offending points deleted."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from afm import synth
from conftest import golden
from oracle import pointops_ref as po, shapes as sh

F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
ULP32 = 2.0 ** -23
TOL = 2e-4                        # tests/test_gpu_points.py's absolute bar for both fused layers
GOLDEN_TOL = 2e-5                 # what the oracle holds against the reference's goldens (tests/test_oracle_golden.py)
BN_EPS = 1e-5


def g(name, shape, seed=synth.NOISE_SEED):
    return synth.gaussian(name, shape, seed=seed)


def f32_class_bound(want32, want64, margin=MARGIN):
    """gpu_util.report_f32_class's bound on max|got - want64|"""
    return margin * (want32.double() - want64).abs().max().item() + ULP32 * want64.abs().max().item()


# ================================================================================================ restatements
PT_WEIGHTS = ("lp0_w", "lp0_b", "lp_s", "lp_t", "lp3_w", "lp3_b", "w0_s", "w0_t", "w2_w", "w2_b", "w3_s", "w3_t", "w5_w", "w5_b")


def pt_attention_restatement(p, qkv, knn_idx, share, w, out_scale=None, out_shift=None, relu=False, dtype=F64):
    """afm_pt_attention's contract (include/afm_hip.h) in `dtype`: p [n, 3], qkv [n, 3C] = q | k | v, knn_idx [n, KN] global rows, `w` the
    fourteen small tensors of PT_WEIGHTS (BatchNorms folded to scale / shift), the optional folded BatchNorm + ReLU of the enclosing
    block.  -> dict(out [n, C], rel [n, KN, 3], w1 [n, KN, C], sw [n, KN, C / share], vp [n, KN, C],
    z the logits, t1 the first BatchNorm's product before its shift)"""
    T = lambda t: t.to(dtype)
    w = {k: T(v) for k, v in w.items()}
    p, qkv, idx = T(p), T(qkv), knn_idx.long()
    n, C, KN = p.shape[0], qkv.shape[1] // 3, idx.shape[1]
    q, k, v = qkv[:, :C], qkv[:, C: 2 * C], qkv[:, 2 * C:]
    rel = p[idx] - p[:, None, :]
    h = torch.relu((rel @ w["lp0_w"].T + w["lp0_b"]) * w["lp_s"] + w["lp_t"])
    pr = h @ w["lp3_w"].T + w["lp3_b"]
    t1 = ((k[idx] - q[:, None, :]) + pr) * w["w0_s"]
    w1 = torch.relu(t1 + w["w0_t"])
    u = torch.relu((w1 @ w["w2_w"].T + w["w2_b"]) * w["w3_s"] + w["w3_t"])
    z = u @ w["w5_w"].T + w["w5_b"]
    sw = torch.softmax(z, dim=1)
    vp = v[idx] + pr
    out = (vp.view(n, KN, share, C // share) * sw[:, :, None, :]).sum(1).reshape(n, C)
    if out_scale is not None:
        out = out * T(out_scale) + T(out_shift)
    if relu:
        out = torch.relu(out)
    return dict(out=out, rel=rel, w1=w1, sw=sw, vp=vp, z=z, t1=t1)


def transition_down_restatement(p, x, new_p, knn_idx, W, scale, shift, dtype=F64):
    """afm_transition_down's contract: out[i, o] = max_j ReLU(scale[o] (W[o, :] . [p[knn[i, j]] - new_p[i] ; x[knn[i, j]]]) + shift[o])
    -> dict(out [M, cout], pre [M, 16, cout] the pre-activations, rel [M, 16, 3])"""
    T = lambda t: t.to(dtype)
    idx = knn_idx.long()
    rel = T(p)[idx] - T(new_p)[:, None, :]
    grouped = torch.cat([rel, T(x)[idx]], -1)
    pre = (grouped @ T(W).T) * T(scale) + T(shift)
    return dict(out=torch.relu(pre).max(1).values, pre=pre, rel=rel)


def bn_fold_restatement(w, b, mean, var, eps, lin_bias=None, dtype=F64):
    """afm_bn_fold: scale = w / sqrt(var + eps), shift = b - mean scale (+ lin_bias scale), each operation rounded once in `dtype`"""
    T = lambda t: t.to(dtype)
    scale = T(w) / torch.sqrt(T(var) + torch.tensor(eps, dtype=dtype))
    shift = T(b) - T(mean) * scale
    if lin_bias is not None:
        shift = T(lin_bias) * scale + shift
    return scale, shift


def bn_fold_ieee32(w, b, mean, var, eps, lin_bias=None):
    """bn_fold_restatement in float32 with every operation - the sum, the square root, the quotient, the products, the differences -
    correctly rounded once (numpy: IEEE 754 instructions).  torch's float32 sqrt on the CPU is not that everywhere: on an AVX-512 host
    it returns sqrt(0x3727C5AD) - the radicand 1e-12 + 1e-5 - one ulp low, where numpy and the kernel's sqrtf agree."""
    w, b, mean, var = (t.numpy() for t in (w, b, mean, var))
    scale = w / np.sqrt(var + np.float32(eps))
    shift = b - mean * scale
    if lin_bias is not None:
        shift = lin_bias.numpy() * scale + shift
    return torch.from_numpy(scale), torch.from_numpy(shift)


def segment_mean_restatement(x, B, n, dtype=F64):
    return x.to(dtype).view(B, n, -1).mean(1)


def gather_rows_restatement(src, idx):
    return src[idx.long()]


def fold_sd(sd, pre, dtype=F64):
    """afm.scene._bn_fold's algebra on a state dict's BatchNorm, redone in `dtype`"""
    return bn_fold_restatement(sd[pre + ".weight"], sd[pre + ".bias"], sd[pre + ".running_mean"], sd[pre + ".running_var"], BN_EPS, dtype=dtype)


def pt_weights_of(sd, pre, dtype=F64):
    """The fourteen tensors afm.scene.PointTransformerLayer.run hands to afm_pt_attention, from a reference state dict"""
    lp_s, lp_t = fold_sd(sd, pre + ".linear_p.1", dtype)
    w0_s, w0_t = fold_sd(sd, pre + ".linear_w.0", dtype)
    w3_s, w3_t = fold_sd(sd, pre + ".linear_w.3", dtype)
    S = lambda k: sd[pre + k].to(dtype)
    return dict(lp0_w=S(".linear_p.0.weight"), lp0_b=S(".linear_p.0.bias"), lp_s=lp_s, lp_t=lp_t, lp3_w=S(".linear_p.3.weight"),
                lp3_b=S(".linear_p.3.bias"), w0_s=w0_s, w0_t=w0_t, w2_w=S(".linear_w.2.weight"), w2_b=S(".linear_w.2.bias"), w3_s=w3_s, w3_t=w3_t,
                w5_w=S(".linear_w.5.weight"), w5_b=S(".linear_w.5.bias"))


@pytest.mark.parametrize("c,k", [(32, 8), (64, 16)])
def test_pt_attention_restatement_is_the_reference_layer(c, k):
    gd = golden(f"pt_block_c{c}_k{k}")
    sd = sh.weights(sh.pt_block("", c))
    knn_idx = po.knn_query(k, gd["p"], gd["p"], gd["o"], gd["o"])[0]
    for dtype in (F64, F32):
        x = gd["x"].to(dtype)
        lin = lambda name: F.linear(x, sd[f"transformer2.{name}.weight"].to(dtype), sd[f"transformer2.{name}.bias"].to(dtype))
        qkv = torch.cat([lin("linear_q"), lin("linear_k"), lin("linear_v")], 1)
        out = pt_attention_restatement(gd["p"], qkv, knn_idx, 8, pt_weights_of(sd, "transformer2", dtype), dtype=dtype)["out"]
        err = (out.double() - gd["layer_out"].double()).abs().max().item()
        assert err <= GOLDEN_TOL, f"c{c} k{k} {dtype}: {err:.3e}"


@pytest.mark.parametrize("stride", [4, 8])
def test_transition_down_restatement_is_the_reference_layer(stride):
    gd = golden(f"transition_down_s{stride}")
    sd = sh.weights(sh.transition_down("", 32, 64, stride))
    counts = torch.diff(gd["o"], prepend=gd["o"].new_zeros(1))
    n_o = torch.cumsum(counts // stride, 0).to(torch.int32)
    knn_idx = po.knn_query(16, gd["p"], gd["n_p"], gd["o"], n_o)[0]
    for dtype in (F64, F32):
        scale, shift = fold_sd(sd, "bn", dtype)
        out = transition_down_restatement(gd["p"], gd["x"], gd["n_p"], knn_idx, sd["linear.weight"], scale, shift, dtype)["out"]
        err = (out.double() - gd["y"].double()).abs().max().item()
        assert err <= GOLDEN_TOL, f"stride {stride} {dtype}: {err:.3e}"


# ================================================================================================ dispatch rules, restated
PT_LDS_LIMIT = 160 * 1024                                     # LDS of one gfx950 workgroup (csrc/pointnet.hip: PT_LDS_LIMIT)
BADARG, UNSUPPORTED = "AFM_E_BADARG", "AFM_E_UNSUPPORTED"


def pt_dispatch(C, share, KN, lds_limit=None):
    """afm_pt_attention: (channels, share_planes, nsample) -> (CPL, KN, NE, waves per workgroup, w2 in LDS, dynamic LDS bytes), or the
    refusal.  CS = C / share weight channels must divide 64 (a wave holds 64 / CS neighbours per pass); CPL = channels per lane rounded up
    to an instantiation, NE = passes over the neighbours; C <= 256 runs four waves (points) per workgroup with linear_w.2 transposed into
    LDS, C > 256 one wave with that weight read from global memory, and nsample = 8 is not built for it."""
    if C <= 0 or share <= 0 or C % share:
        return BADARG
    CS = C // share
    if C > 512 or KN not in (8, 16) or CS > 64 or 64 % CS:
        return UNSUPPORTED
    cpl, ne = (C + 63) // 64, -(-KN // (64 // CS))
    w2_lds, nwv = C <= 256, (4 if C <= 256 else 1)
    if (ne > 4 or cpl > 4 or not w2_lds) if KN == 8 else (ne > 16 or cpl > 8):
        return UNSUPPORTED
    lds = ((C * CS if w2_lds else 0) + CS * CS + nwv * (KN * (C + 1) + 2 * KN * CS)) * 4
    if lds > (PT_LDS_LIMIT if lds_limit is None else lds_limit):
        return UNSUPPORTED
    if KN == 8:
        inst = (1, 8, 1) if cpl == 1 and ne <= 1 else (2, 8, 2) if cpl <= 2 and ne <= 2 else (4, 8, 4)
    else:
        inst = (1, 16, 2) if cpl == 1 and ne <= 2 else (2, 16, 4) if cpl <= 2 and ne <= 4 else (4, 16, 8) if cpl <= 4 and ne <= 8 else (8, 16, 16)
    return inst + (nwv, w2_lds, lds)


# (C, share, KN) -> the instantiation it is meant to reach
PT_ARMS = {
    (32, 8, 8): (1, 8, 1), (64, 8, 8): (1, 8, 1),
    (128, 8, 8): (2, 8, 2), (96, 6, 8): (2, 8, 2),                   # 96: lanes 32..63 of the second channel slot are idle
    (256, 8, 8): (4, 8, 4), (32, 1, 8): (4, 8, 4),
    (32, 8, 16): (1, 16, 2), (64, 8, 16): (1, 16, 2),
    (128, 8, 16): (2, 16, 4), (48, 3, 16): (2, 16, 4),
    (256, 8, 16): (4, 16, 8), (32, 1, 16): (4, 16, 8),
    (64, 1, 16): (8, 16, 16),                                        # w2 from LDS
    (512, 8, 16): (8, 16, 16),                                       # one wave, w2 from global memory
}
PT_SMALL_ONLY = {(96, 6, 8), (48, 3, 16)}                             # n = 37 only
PT_POINTS = (("1x37", 1, 37), ("2x50", 2, 50))                        # (tag, samples, points per sample)
PT_REFUSALS = {
    (512, 8, 8): UNSUPPORTED, (40, 8, 8): UNSUPPORTED, (40, 8, 16): UNSUPPORTED, (520, 8, 16): UNSUPPORTED, (32, 8, 4): UNSUPPORTED,
    (36, 8, 16): BADARG, (256, 4, 16): UNSUPPORTED,
}


def pt_over_budget():
    """every (C, share, KN) that passes the shape checks and asks for more LDS than a workgroup has"""
    out = []
    for C in range(1, 513):
        for share in range(1, C + 1):
            if C % share:
                continue
            for KN in (8, 16):
                d = pt_dispatch(C, share, KN, lds_limit=1 << 40)
                if isinstance(d, tuple) and d[5] > PT_LDS_LIMIT:
                    out.append((C, share, KN))
    return out


def pt_trips(n, C):
    """-> (workgroups, trips of the grid-stride loop over groups of `waves` points)"""
    nwv = 4 if C <= 256 else 1
    quads = (n + nwv - 1) // nwv
    grid = min(quads, 2048)
    return grid, (quads + grid - 1) // grid


PT_COUNTS = [(32, 8, 16, n) for n in (1, 2, 3, 4, 5)] + [(512, 8, 16, n) for n in (1, 2, 3, 4, 5)]
PT_SECOND_TRIP = [(32, 8, 16, 8197), (512, 8, 16, 2051)]


def test_pt_attention_dispatch_every_arm_and_refusal_is_reached():
    reached = {}
    for key, inst in PT_ARMS.items():
        d = pt_dispatch(*key)
        assert isinstance(d, tuple) and d[:3] == inst, (key, d)
        reached.setdefault((inst, d[4]), []).append(key)
    insts = {(1, 8, 1), (2, 8, 2), (4, 8, 4), (1, 16, 2), (2, 16, 4), (4, 16, 8), (8, 16, 16)}
    assert {i for i, _ in reached} == insts, "the seven instantiations"
    assert ((8, 16, 16), True) in reached and ((8, 16, 16), False) in reached, "w2 from LDS and from global memory"
    assert pt_dispatch(512, 8, 16)[3] == 1 and all(pt_dispatch(*k)[3] == 4 for k in PT_ARMS if k[0] <= 256)
    assert pt_dispatch(64, 1, 16)[5] > 64 * 1024, "(64, 1, 16) raises the kernel's dynamic-LDS attribute"
    for key, want in PT_REFUSALS.items():
        assert pt_dispatch(*key) == want, (key, pt_dispatch(*key))
    over = pt_over_budget()
    assert over == [(256, 4, 16)] and all(k in PT_REFUSALS for k in over), over
    assert (256 * 64 + 64 * 64 + 4 * (16 * 257 + 2 * 16 * 64)) * 4 == 180480
    # dead waves and lanes, the one-wave form, the second trip of the grid-stride loop
    for C, share, KN, n in PT_COUNTS:
        assert pt_trips(n, C) == ((n + 3) // 4 if C <= 256 else n, 1)
    assert pt_trips(8197, 32) == (2048, 2) and pt_trips(8192, 32) == (2048, 1)
    assert pt_trips(2051, 512) == (2048, 2) and pt_trips(2048, 512) == (2048, 1)


TD_C, TD_COUT, TD_M = (1, 6, 29, 30, 32, 61, 64), (1, 32, 63, 64, 65, 128), (1, 7, 8, 9, 17)


def td_tiles(c, cout, M):
    """transition_down_kernel's tiles: K = 3 + c against BK = 32, cout against 64-column blocks, M * 16 rows against 128-row blocks
    -> set of the tile kinds the launch holds"""
    K, rows = 3 + c, M * 16
    kinds = set()
    if K >= 32:
        kinds.add("full K tile")
    if K % 32:
        kinds.add("ragged K tile")
    if cout >= 64:
        kinds.add("full column block")
    if cout % 64:
        kinds.add("ragged column block")
    if rows >= 128:
        kinds.add("full row block")
    if rows % 128:
        kinds.add("ragged row block")
    return kinds


TD_KINDS = ("full K tile", "ragged K tile", "full column block", "ragged column block", "full row block", "ragged row block")
TD_FAMILY_SHAPES = [(32, 64, 17), (6, 32, 9)]


def test_transition_down_grid_reaches_every_tile_kind():
    assert [3 + c for c in TD_C] == [4, 9, 32, 33, 35, 64, 67]
    seen = {k: 0 for k in TD_KINDS}
    for c in TD_C:
        for cout in TD_COUT:
            for M in TD_M:
                for k in td_tiles(c, cout, M):
                    seen[k] += 1
    assert all(v >= 2 for v in seen.values()), seen
    assert td_tiles(29, 64, 8) == {"full K tile", "full column block", "full row block"}               # nothing ragged at all
    assert td_tiles(1, 1, 1) == {"ragged K tile", "ragged column block", "ragged row block"}           # nothing full
    assert td_tiles(61, 128, 17) >= {"full K tile", "full column block", "full row block", "ragged row block"} and (3 + 61) // 32 == 2
    assert td_tiles(64, 65, 9) == set(TD_KINDS)                                                        # three K tiles, the last of 3 columns
    for shape in TD_FAMILY_SHAPES:
        assert shape[0] in TD_C and shape[1] in TD_COUT and shape[2] in TD_M


# ================================================================================================ clouds and inputs
def cloud(B, n, seed, grid=False):
    """[B n, 3] scene cloud; grid=True: every coordinate a multiple of 2^-10 in (-4, 4), so that a translation by 1e3 is exact in float32"""
    p = synth.scene_cloud(B, n, seed=seed).reshape(B * n, 3)
    return torch.round(p * 1024.0) / 1024.0 if grid else p.contiguous()


def self_knn(p, B, n, k):
    o = torch.arange(1, B + 1, dtype=torch.int32) * n
    return po.knn_query(k, p, p, o, o)[0]


PT_FAMILIES = ("softmax_1", "softmax_8", "softmax_30", "softmax_uniform", "softmax_shift_1e4", "dead_relu", "far_cloud", "one_row", "bn_fold_1e3")
PT_FAMILY_SHAPES = [(64, 8, 16), (256, 8, 16)]
FAR = 1e3


@functools.lru_cache(maxsize=None)
def pt_inputs(C, share, KN, B, n, family="softmax_1"):
    """One afm_pt_attention call (float32 CPU tensors, shared: not to be written to): cloud, self-kNN of the oracle, Gaussian qkv, small
    weights with folded BatchNorms near the identity.  The families change exactly what their name says (see the proofs below)."""
    CS = C // share
    tag = f"pie_pt_{C}_{share}_{KN}"
    grid = family == "far_cloud"
    p = cloud(B, n, seed=41 + C + KN, grid=grid)
    knn_idx = self_knn(p, B, n, KN)
    if family == "far_cloud":
        p = p + FAR
    if family == "one_row":                                   # the n < k case taken to its end: every neighbour of a point is ONE row
        knn_idx = knn_idx[:, 3 % KN: 3 % KN + 1].expand(-1, KN).contiguous()
    qkv = g(tag + f"_qkv_{B}x{n}", (B * n, 3 * C))
    w = dict(lp0_w=0.5 * g(tag + "_lp0w", (3, 3)), lp0_b=0.1 * g(tag + "_lp0b", (3,)), lp_s=1 + 0.1 * g(tag + "_lps", (3,)), lp_t=0.1 * g(tag + "_lpt", (3,)),
             lp3_w=0.5 * g(tag + "_lp3w", (C, 3)), lp3_b=0.1 * g(tag + "_lp3b", (C,)), w0_s=1 + 0.1 * g(tag + "_w0s", (C,)), w0_t=0.1 * g(tag + "_w0t", (C,)),
             w2_w=g(tag + "_w2w", (CS, C)) / C ** 0.5, w2_b=0.1 * g(tag + "_w2b", (CS,)), w3_s=1 + 0.1 * g(tag + "_w3s", (CS,)), w3_t=0.1 * g(tag + "_w3t", (CS,)),
             w5_w=g(tag + "_w5w", (CS, CS)) / CS ** 0.5, w5_b=0.1 * g(tag + "_w5b", (CS,)))
    if family.startswith("softmax_") and family[8:].isdigit():
        w["w5_w"] = w["w5_w"] * float(family[8:])
    if family == "softmax_uniform":
        w["w5_w"] = torch.zeros_like(w["w5_w"])
    if family == "softmax_shift_1e4":
        w["w5_b"] = w["w5_b"] + 1e4
    if family == "dead_relu":
        w["w0_t"] = w["w0_t"] - 1e3
    if family == "bn_fold_1e3":
        # linear_w.0 as a BatchNorm whose running mean lies 1e3 sigma from 0, on pre-activations that lie around that mean: k carries it
        var = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(C))
        mean = 1e3 * var.sqrt()
        gamma, beta = 0.25 * (1 + 0.1 * g(tag + "_bng", (C,))), 0.1 * g(tag + "_bnb", (C,))
        w["w0_s"], w["w0_t"] = bn_fold_restatement(gamma, beta, mean, var, BN_EPS, dtype=F32)
        qkv = qkv.clone()
        qkv[:, C: 2 * C] += mean
    return dict(p=p, qkv=qkv, knn_idx=knn_idx, w=w, share=share)


@functools.lru_cache(maxsize=None)
def pt_reference(C, share, KN, B, n, family, dtype, fused=None):
    i = pt_inputs(C, share, KN, B, n, family)
    kw = {}
    if fused is not None:
        kw = dict(out_scale=pt_out_bn(C)[0], out_shift=pt_out_bn(C)[1], relu=fused)
    return pt_attention_restatement(i["p"], i["qkv"], i["knn_idx"], share, i["w"], dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def pt_out_bn(C):
    return 1 + 0.1 * g(f"pie_pt_outs_{C}", (C,)), 0.1 * g(f"pie_pt_outt_{C}", (C,))


LOGIT_SIZE, TERM_SIZE = 256.0, 8.0        # (a logit of 256 has a float32 spacing of 3e-5: times |v + p_r| of a few, that is TOL)


def pt_tol(C, share, KN, B, n, family, fused=None):
    """TOL = 2e-4 is stated for logits of size <= LOGIT_SIZE and BatchNorm products |x scale| <= TERM_SIZE (the model-level tests' inputs).
    A float32 logit of size L is resolved to 2^-24 L, and so are the probabilities; x scale + shift rounds each term at the term's own
    size before they cancel (tests/test_point_train_edges_host.py, bn_tol).  So the bar grows with both beyond those sizes: logits of
    1e4 have a float32 spacing of 1e-3.  It only says below WHAT the class bound must stay to mean something; the bound itself is the
    float32 restatement's own error."""
    r = pt_reference(C, share, KN, B, n, family, F64, fused)
    return TOL * max(1.0, r["z"].abs().max().item() / LOGIT_SIZE, r["t1"].abs().max().item() / TERM_SIZE)


def td_tol(c, cout, M, family):
    """the same rule for afm_transition_down's scale (W . g) + shift"""
    i, r = td_inputs(c, cout, M, family), td_reference(c, cout, M, family, F64)
    return TOL * max(1.0, (r["pre"] - i["shift"].double()).abs().max().item() / TERM_SIZE)


def _bound_holds(r32, r64, tol=TOL):
    return (r32.double() - r64).abs().max().item() < tol and f32_class_bound(r32, r64) < tol


@pytest.mark.parametrize("C,share,KN", PT_FAMILY_SHAPES)
def test_pt_attention_value_families_are_what_they_claim(C, share, KN):
    B, n = 1, 37
    base = pt_inputs(C, share, KN, B, n)
    for family in PT_FAMILIES:
        i = pt_inputs(C, share, KN, B, n, family)
        r32, r64 = pt_reference(C, share, KN, B, n, family, F32), pt_reference(C, share, KN, B, n, family, F64)
        assert torch.isfinite(r32["out"]).all()
        assert _bound_holds(r32["out"], r64["out"], pt_tol(C, share, KN, B, n, family)), (family, f32_class_bound(r32["out"], r64["out"]))
        if family not in ("softmax_shift_1e4", "bn_fold_1e3"):
            assert pt_tol(C, share, KN, B, n, family) == TOL
        top = r64["sw"].max(1).values
        if family == "softmax_30":
            assert (top > 0.999).float().mean().item() > 0.1, "the largest probability per row reaches > 0.999 at scale 30"
            assert top.mean().item() > pt_reference(C, share, KN, B, n, "softmax_8", F64)["sw"].max(1).values.mean().item() \
                > pt_reference(C, share, KN, B, n, "softmax_1", F64)["sw"].max(1).values.mean().item()
        if family == "softmax_uniform":
            for r in (r32, r64):
                assert (r["sw"] == 1.0 / KN).all(), "w5 = 0: the probabilities are exactly uniform"
            mean = r64["vp"].view(n, KN, share, C // share).mean(1).reshape(n, C)
            assert (mean - r64["out"]).abs().max().item() < 1e-12, "and the output is the plain neighbour mean"
        if family == "softmax_shift_1e4":
            ref = pt_reference(C, share, KN, B, n, "softmax_1", F64)
            assert (r64["sw"] - ref["sw"]).abs().max().item() < 1e-10, "softmax is invariant under a shift of its logits"
            assert torch.equal(i["w"]["w5_w"], base["w"]["w5_w"]) and (i["w"]["w5_b"] > 9990).all()
        if family == "dead_relu":
            for r in (r32, r64):
                assert (r["w1"] == 0).all(), "a shift of -1e3 kills every first ReLU of the weight MLP"
        if family == "far_cloud":
            near = pt_inputs(C, share, KN, B, n, "softmax_1")
            grid = cloud(B, n, seed=41 + C + KN, grid=True)
            assert torch.equal(i["p"] - FAR, grid) and torch.equal((i["p"].double() - FAR).float(), grid), "the translation is exact in float32"
            rel_near = grid[i["knn_idx"].long()] - grid[:, None, :]
            assert torch.equal(r32["rel"], rel_near), "relative positions bit-equal to the untranslated ones"
            assert torch.equal(i["knn_idx"], self_knn(grid, B, n, KN)) and near["p"].shape == i["p"].shape
            assert i["p"].min().item() > 990
        if family == "one_row":
            assert (i["knn_idx"] == i["knn_idx"][:, :1]).all() and KN == 16
            for r in (r32, r64):
                assert (r["sw"] == 1.0 / KN).all()
            assert (r64["vp"][:, 0] - r64["out"]).abs().max().item() < 1e-12, "sixteen copies of one row: the output is v + p_r of that row"
        if family == "bn_fold_1e3":
            pre = (i["qkv"][:, C: 2 * C][i["knn_idx"].long()] - i["qkv"][:, None, :C]).double()
            assert (pre.mean((0, 1)) / pre.std((0, 1))).min().item() > 300, "the BatchNorm's input lies hundreds of sigma from 0"
            assert (r64["w1"] > 0).float().mean().item() > 0.2 and (r64["w1"] == 0).float().mean().item() > 0.2, "and comes out on both sides of the ReLU"


def test_pt_attention_every_case_keeps_a_bound_below_the_tolerance():
    for (C, share, KN) in PT_ARMS:
        for tag, B, n in PT_POINTS[:1]:
            r32, r64 = pt_reference(C, share, KN, B, n, "softmax_1", F32)["out"], pt_reference(C, share, KN, B, n, "softmax_1", F64)["out"]
            assert _bound_holds(r32, r64), (C, share, KN, f32_class_bound(r32, r64))
            # a wrong answer leaves the bound by far: the last neighbour left out, and the weight channel taken as ch / share for ch % CS
            i = pt_inputs(C, share, KN, B, n)
            r = pt_reference(C, share, KN, B, n, "softmax_1", F64)
            CS = C // share
            drop = (r["vp"][:, :-1].view(n, KN - 1, share, CS) * r["sw"][:, :-1, None, :]).sum(1).reshape(n, C)
            assert (drop - r64).abs().max().item() > 100 * f32_class_bound(r32, r64)
            if share > 1 and CS > 1:
                swap = (r["vp"].view(n, KN, CS, share) * r["sw"][:, :, :, None]).sum(1).reshape(n, C)
                assert (swap - r64).abs().max().item() > 100 * f32_class_bound(r32, r64)


# ---- transition_down
TD_FAMILIES = ("gaussian", "all_negative", "far_cloud", "bn_fold_1e3")


@functools.lru_cache(maxsize=None)
def td_inputs(c, cout, M, family="gaussian"):
    """One afm_transition_down call: a cloud of one sample (two for an even M >= 8) with n = max(4 m, 24) points each, the M points the
    oracle's FPS samples and their 16 nearest neighbours by the oracle's kNN, Gaussian features, W ~ N(0, 1 / K)"""
    B = 2 if M % 2 == 0 and M >= 8 else 1
    m = M // B
    n = max(4 * m, 24)
    grid = family == "far_cloud"
    p = cloud(B, n, seed=53 + M, grid=grid)
    o, n_o = torch.arange(1, B + 1, dtype=torch.int32) * n, torch.arange(1, B + 1, dtype=torch.int32) * m
    fps = po.furthest_sampling(p, o, n_o)
    new_p = p[fps.long()].contiguous()
    knn_idx = po.knn_query(16, p, new_p, o, n_o)[0]
    if family == "far_cloud":
        p, new_p = p + FAR, new_p + FAR
    K = 3 + c
    x = g(f"pie_td_x_{n * B}_{c}", (B * n, c))
    W = g(f"pie_td_w_{cout}_{K}", (cout, K)) / K ** 0.5
    scale, shift = 1 + 0.1 * g(f"pie_td_s_{cout}", (cout,)), 0.1 * g(f"pie_td_t_{cout}", (cout,))
    if family == "all_negative":
        shift = shift - 1e3
    if family == "bn_fold_1e3":
        # the layer's BatchNorm with a running mean 1e3 sigma from 0, on products that lie around that mean: feature 0 is the constant 1
        # and W's column for it carries the mean
        var = 0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(cout))
        mean = 1e3 * var.sqrt()
        gamma, beta = 0.25 * (1 + 0.1 * g(f"pie_td_bng_{cout}", (cout,))), 0.1 * g(f"pie_td_bnb_{cout}", (cout,))
        scale, shift = bn_fold_restatement(gamma, beta, mean, var, BN_EPS, dtype=F32)
        x, W = x.clone(), W.clone()
        x[:, 0] = 1.0
        W[:, 3] = mean
    return dict(p=p, x=x, new_p=new_p, knn_idx=knn_idx, W=W, scale=scale, shift=shift, B=B, n=n, m=m)


@functools.lru_cache(maxsize=None)
def td_reference(c, cout, M, family, dtype):
    i = td_inputs(c, cout, M, family)
    return transition_down_restatement(i["p"], i["x"], i["new_p"], i["knn_idx"], i["W"], i["scale"], i["shift"], dtype)


@pytest.mark.parametrize("c,cout,M", TD_FAMILY_SHAPES)
def test_transition_down_value_families_are_what_they_claim(c, cout, M):
    for family in TD_FAMILIES:
        i = td_inputs(c, cout, M, family)
        r32, r64 = td_reference(c, cout, M, family, F32), td_reference(c, cout, M, family, F64)
        assert i["knn_idx"].shape == (M, 16) and i["new_p"].shape == (M, 3)
        assert _bound_holds(r32["out"], r64["out"], td_tol(c, cout, M, family)), (family, f32_class_bound(r32["out"], r64["out"]))
        assert family == "bn_fold_1e3" or family == "all_negative" or td_tol(c, cout, M, family) == TOL
        if family == "all_negative":
            for r in (r32, r64):
                assert (r["pre"] < -900).all() and (r["out"] == 0).all(), "every pre-activation negative: the restatement gives exactly 0"
        if family == "far_cloud":
            near = td_inputs(c, cout, M, "gaussian")
            gp = cloud(i["B"], i["n"], seed=53 + M, grid=True)
            assert torch.equal(i["p"] - FAR, gp) and torch.equal((i["p"].double() - FAR).float(), gp)
            gn = i["new_p"] - FAR
            assert torch.equal(r32["rel"], gp[i["knn_idx"].long()] - gn[:, None, :]), "relative positions bit-equal to the untranslated ones"
            assert near["p"].shape == i["p"].shape and i["p"].min().item() > 990
        if family == "bn_fold_1e3":
            acc = (r64["pre"] - i["shift"].double()) / i["scale"].double()
            assert (acc.mean((0, 1)) / acc.std((0, 1))).min().item() > 300
            assert (r64["pre"] > 0).float().mean().item() > 0.2 and (r64["pre"] < 0).float().mean().item() > 0.2
    # the grid's cases keep a bound too (checked at the corners of the grid: the product itself runs on the GPU)
    for cc in (TD_C[0], TD_C[-1]):
        for co in (TD_COUT[0], TD_COUT[-1]):
            for MM in (TD_M[0], TD_M[-1]):
                a, b = td_reference(cc, co, MM, "gaussian", F32)["out"], td_reference(cc, co, MM, "gaussian", F64)["out"]
                assert _bound_holds(a, b), (cc, co, MM)


# ---- BatchNorm fold
FOLD_C, FOLD_VAR = (1, 255, 256, 257, 513), (0.0, 1e-12, 1.0, 1e12)
FOLD_TOL = 1e-6                   # relative to the largest scale / shift: a handful of float32 roundings


@functools.lru_cache(maxsize=None)
def fold_inputs(C, var, with_bias):
    """gamma, beta, a running mean 1e3 sigma from 0, the constant running variance `var`, an optional Linear bias"""
    tag = f"pie_fold_{C}"
    v = torch.full((C,), var, dtype=F32)
    sigma = (v + BN_EPS).sqrt()
    return dict(w=1 + 0.1 * g(tag + "_w", (C,)), b=0.1 * g(tag + "_b", (C,)), mean=1e3 * sigma * (1 + 0.01 * g(tag + "_m", (C,))), var=v,
                lin_bias=g(tag + "_lb", (C,)) if with_bias else None)


def test_bn_fold_family_and_restatement():
    for C in FOLD_C:
        for var in FOLD_VAR:
            for with_bias in (False, True):
                i = fold_inputs(C, var, with_bias)
                s32, t32 = bn_fold_restatement(i["w"], i["b"], i["mean"], i["var"], BN_EPS, i["lin_bias"], F32)
                s64, t64 = bn_fold_restatement(i["w"], i["b"], i["mean"], i["var"], BN_EPS, i["lin_bias"], F64)
                assert torch.isfinite(s32).all() and torch.isfinite(t32).all()
                si, ti = bn_fold_ieee32(i["w"], i["b"], i["mean"], i["var"], BN_EPS, i["lin_bias"])
                assert si.dtype == F32 and ((si.double() - s64).abs() <= 2 * ULP32 * s64.abs()).all() and ((ti.double() - t64).abs() <= 8 * ULP32 * t64.abs().max()).all()
                assert ((s32.double() - s64).abs() <= 4 * ULP32 * s64.abs()).all() and ((t32.double() - t64).abs() <= 8 * ULP32 * t64.abs().max()).all()
                assert ((i["mean"].double() / (i["var"].double() + BN_EPS).sqrt()).abs() > 900).all(), "the running mean lies 1e3 sigma from 0"
                # the fold IS eval-mode BatchNorm: x scale + shift against F.batch_norm in float64
                x = g(f"pie_fold_x_{C}", (5, C)).double() * (var + BN_EPS) ** 0.5 + i["mean"].double()
                lb = 0 if i["lin_bias"] is None else i["lin_bias"].double()
                want = F.batch_norm(x + lb, i["mean"].double(), i["var"].double(), i["w"].double(), i["b"].double(), False, 0.0, BN_EPS)
                assert (x * s64 + t64 - want).abs().max().item() < 1e-9 * max(1.0, want.abs().max().item())


# ---- segment mean
SEG_CASES = [(1, 1, 1), (3, 16, 512), (2, 256, 32), (2, 2048, 32), (2, 8192, 32), (1, 8192, 257)]
SEG_FAMILIES = ("gauss", "relu", "mean50")
SEG_TOL = 1e-3


@functools.lru_cache(maxsize=None)
def seg_inputs(B, n, c, family):
    z = g(f"pie_seg_{B}_{n}_{c}", (B * n, c))
    return z if family == "gauss" else torch.relu(z) if family == "relu" else 50.0 + 0.5 * z


def blocked_f32_mean(x, B, n, chains=64):
    """csrc/pointops.hip, segment_mean_kernel, in numpy float32: row i goes to chain i % 64, a chain adds its rows in ascending order, the
    chains are combined by the tree s[p] += s[p + h], h = 32 ... 1, and the total is divided by n"""
    x = x.numpy().reshape(B, n, -1)
    acc = np.zeros((B, chains, x.shape[2]), dtype=np.float32)
    for i0 in range(0, n, chains):
        blk = x[:, i0: i0 + chains]
        acc[:, : blk.shape[1]] = acc[:, : blk.shape[1]] + blk
    h = chains // 2
    while h:
        acc[:, :h] = acc[:, :h] + acc[:, h: 2 * h]
        h //= 2
    return torch.from_numpy(acc[:, 0] / np.float32(n))


def serial_f32_mean(x, B, n):
    """the kernel's earlier form: one ascending float32 chain over the n rows"""
    x = x.numpy().reshape(B, n, -1)
    acc = np.zeros((B, x.shape[2]), dtype=np.float32)
    for i in range(n):
        acc = acc + x[:, i]
    return torch.from_numpy(acc / np.float32(n))


@pytest.mark.parametrize("B,n,c", SEG_CASES)
def test_segment_mean_bound_is_meaningful_and_the_blocked_order_is_inside_it(B, n, c):
    for family in SEG_FAMILIES:
        x = seg_inputs(B, n, c, family)
        r32, r64 = segment_mean_restatement(x, B, n, F32), segment_mean_restatement(x, B, n, F64)
        floor = ULP32 * r64.abs().max().item()
        bound = f32_class_bound(r32, r64)
        assert bound < SEG_TOL
        if n > 1:
            assert bound > floor, "the float32 reference's own error leaves the bound above one ulp of the largest mean"
        if family == "mean50":
            assert (r64 - 50).abs().max().item() < (3.0 if n < 256 else 0.2)
        if family == "relu":
            assert (x >= 0).all() and (x == 0).float().mean().item() > 0.3
        blocked = blocked_f32_mean(x, B, n)
        assert (blocked.double() - r64).abs().max().item() <= bound, "the kernel's order, restated on the host, is in the class"
        assert torch.equal(blocked[:1], blocked_f32_mean(x[:n], 1, n)), "a sample's mean is a function of its own rows"
        if n >= 2048 and c == 32:
            serial = (serial_f32_mean(x, B, n).double() - r64).abs().max().item()
            assert serial > bound, f"{family} n={n}: the serial chain ({serial:.2e}) was expected outside the class ({bound:.2e})"


# ---- gather rows
GATHER_CASES = [(1, 1), (300, 3), (1025, 35), (70000, 16)]


@functools.lru_cache(maxsize=None)
def gather_inputs(rows, c):
    n_src = max(1, rows // 3)
    idx = torch.randint(0, n_src, (rows,), generator=torch.Generator().manual_seed(rows + c), dtype=torch.int32)
    return g(f"pie_ga_{n_src}_{c}", (n_src, c)), idx


def test_gather_cases_pass_the_grid_cap():
    trips = lambda rows, c: -(-(rows * c) // (min(4096, -(-(rows * c) // 256)) * 256))
    assert [trips(r, c) for r, c in GATHER_CASES] == [1, 1, 1, 2]
    for rows, c in GATHER_CASES:
        src, idx = gather_inputs(rows, c)
        assert int(idx.min()) >= 0 and int(idx.max()) < src.shape[0] and gather_rows_restatement(src, idx).shape == (rows, c)


# ================================================================================================ kNN / FPS on non-finite coordinates
BAD_VALUES = (float("nan"), -float("nan"), float("inf"), -float("inf"), 3e19, -3e19)
NEG_NAN = torch.tensor([0xFFC00000 - (1 << 32)], dtype=torch.int32).view(F32).item()      # a NaN with the sign bit set


def spoil(p, B, n, count, seed):
    """A copy of the cloud [B n, 3] with `count` points per sample spoiled: one coordinate (sometimes all three) of each set to NaN, a NaN
    with the sign bit set, +-inf or +-3e19 (finite, but its squared distance to any ordinary point overflows) -> (cloud, spoiled mask)"""
    p = p.clone().view(B, n, 3)
    bad = torch.zeros(B, n, dtype=torch.bool)
    gen = torch.Generator().manual_seed(seed)
    vals = torch.tensor(BAD_VALUES, dtype=F32)
    vals[1] = NEG_NAN
    for b in range(B):
        rows = torch.randperm(n, generator=gen)[:count]
        for j, r in enumerate(rows.tolist()):
            v = vals[(j + b) % len(vals)]
            if j % 4 == 3:
                p[b, r, :] = v
            else:
                p[b, r, j % 3] = v
            bad[b, r] = True
    return p.reshape(B * n, 3).contiguous(), bad.reshape(B * n)


@functools.lru_cache(maxsize=None)
def knn_case(k, B, n, m, where, count, seed=0):
    """-> candidates [B n, 3], queries [B m, 3] (the candidates themselves when m == n and where != "queries-only"), spoiled masks.
    where: "none", "candidates", "queries", "both"; count: spoiled points per sample"""
    p = cloud(B, n, seed=61 + n + seed)
    self_search = m == n and where in ("none", "both")
    q = p if self_search else cloud(B, m, seed=67 + m + seed)
    pbad, qbad = torch.zeros(B * n, dtype=torch.bool), torch.zeros(B * m, dtype=torch.bool)
    if where in ("candidates", "both"):
        p, pbad = spoil(p, B, n, min(count, n), seed=71 + seed)
    if self_search:
        q, qbad = p, pbad
    elif where in ("queries", "both"):
        q, qbad = spoil(q, B, m, min(count, m), seed=73 + seed)
    return p, q, pbad, qbad


def knn_oracle(k, p, q, B, n, m):
    return po.knn_query(k, p, q, torch.arange(1, B + 1, dtype=torch.int32) * n, torch.arange(1, B + 1, dtype=torch.int32) * m)


def check_contract(idx, d2, k, B, n, m):
    """rule 1 and the shape of rules 3 and 4 on any output"""
    idx, d2 = idx.view(B, m, k).long(), d2.view(B, m, k)
    lo = (torch.arange(B) * n).view(B, 1, 1)
    assert ((idx >= lo) & (idx < lo + n)).all(), "an index outside its sample"
    none = torch.isinf(d2[..., 0])
    assert (torch.isfinite(d2) | none[..., None]).all() and not torch.isnan(d2).any()
    assert (idx[none] == lo.expand(B, m, 1)[none]).all() and (d2[none] == float("inf")).all(), "no neighbour: the sample's first row at +inf"
    assert (d2[..., 1:] >= d2[..., :-1]).all()


PLAIN_KNN = [(k, 2, n, m) for k in (3, 8, 16) for n in (5, 300) for m in (7, 300)]
SPOILED = [("candidates", 1), ("candidates", 5), ("queries", 1), ("queries", 5), ("both", 1), ("both", 5), ("candidates", -1), ("both", -1)]     # -1: all but k


def all_but_k(n, k, count):
    return max(n - k - 1, 0) if count < 0 else count


@pytest.mark.parametrize("k,B,n,m", PLAIN_KNN)
def test_extended_oracle_on_spoiled_clouds(k, B, n, m):
    # finite input: the rule changes nothing (n < k repeats the last, as before)
    p, q, _, _ = knn_case(k, B, n, m, "none", 0)
    idx, d2 = knn_oracle(k, p, q, B, n, m)
    check_contract(idx, d2, k, B, n, m)
    d = po._d2(q.view(B, m, 1, 3), p.view(B, 1, n, 3))
    order = torch.argsort(d, dim=2, stable=True)[..., : min(k, n)]
    assert torch.equal(idx.view(B, m, k)[..., : min(k, n)].long(), order + (torch.arange(B) * n).view(B, 1, 1)), "a stable argsort of the distances"
    if n < k:
        assert (idx.view(B, m, k)[..., n:] == idx.view(B, m, k)[..., n - 1: n]).all()
    for where, count in SPOILED:
        count = all_but_k(n, k, count)
        p, q, pbad, qbad = knn_case(k, B, n, m, where, count)
        idx, d2 = knn_oracle(k, p, q, B, n, m)
        check_contract(idx, d2, k, B, n, m)
        _deleted_sample_agrees(idx, d2, k, p, q, pbad, qbad, B, n, m)


def _deleted_sample_agrees(idx, d2, k, p, q, pbad, qbad, B, n, m):
    """For every untouched query: the oracle on the sample with the spoiled candidates deleted, mapped back to original rows, is the
    result on the spoiled sample (entries beyond the number of kept candidates repeat the last on both sides)."""
    for b in range(B):
        keep = torch.nonzero(~pbad[b * n: (b + 1) * n]).flatten()
        qs = torch.nonzero(~qbad[b * m: (b + 1) * m]).flatten()
        if keep.numel() == 0 or qs.numel() == 0:
            continue
        pi, pd = po.knn_query(k, p[b * n: (b + 1) * n][keep], q[b * m: (b + 1) * m][qs], torch.tensor([keep.numel()], dtype=torch.int32),
                              torch.tensor([qs.numel()], dtype=torch.int32))
        assert torch.equal(keep[pi.long()] + b * n, idx[b * m: (b + 1) * m][qs].long()), "indices differ from the sample with the spoiled points deleted"
        assert torch.equal(pd, d2[b * m: (b + 1) * m][qs])
    spoiled_q = torch.nonzero(qbad).flatten()
    if spoiled_q.numel():
        nonfinite_q = ~torch.isfinite(q[spoiled_q]).all(1)
        assert torch.isinf(d2[spoiled_q][nonfinite_q]).all(), "a query with a NaN or infinite coordinate has no neighbour"


def test_spoiled_values_are_what_they_claim():
    v = torch.tensor(BAD_VALUES, dtype=F32)
    v[1] = NEG_NAN
    assert torch.isnan(v[:2]).all() and v[:2].view(torch.int32)[0] > 0 > v[:2].view(torch.int32)[1], "a NaN of either sign"
    assert v[0:1].view(torch.int32).item() > torch.tensor([float("inf")]).view(torch.int32).item(), "positive NaN bits compare above +inf's"
    assert torch.isinf(v[2:4]).all() and torch.isfinite(v[4:]).all()
    d = po._d2(torch.tensor([[3e19, 0.0, 0.0]]), torch.tensor([[1.0, 2.0, 0.5]]))
    assert torch.isinf(d).all(), "3e19 is finite and its squared distance overflows"
    assert po._d2(torch.tensor([[3e19, 0.0, 0.0]]), torch.tensor([[3e19, 1.0, 0.0]])).item() == 1.0, "though not to another point at 3e19"
    p, bad = spoil(cloud(2, 300, seed=5), 2, 300, 64, seed=9)
    assert bad.view(2, 300).sum(1).tolist() == [64, 64] and torch.isnan(p).any() and torch.isinf(p).any() and (p.abs() == 3e19).any()
    assert torch.isfinite(p[~bad]).all() and (~torch.isfinite(p[bad]).all(1) | (p[bad].abs() > 1e19).any(1)).all()
    assert (torch.isnan(p) & torch.signbit(p)).any() and (torch.isnan(p) & ~torch.signbit(p)).any()


PRUNED_KNN = [(k, 2, 4096, 4096, count) for k in (8, 16) for count in (1, 64, -1)]


def test_pruned_shapes_take_the_pruned_form():
    applies = lambda k, n, m: k in (3, 8, 16) and 4096 <= n <= 8192 and n <= m <= 8192
    assert all(applies(k, n, m) for k, _, n, m, _ in PRUNED_KNN) and not any(applies(k, n, m) for k, _, n, m in PLAIN_KNN)
    assert all_but_k(4096, 16, -1) == 4096 - 16 - 1 and 4096 % 64 == 0 and (4096 - 17) // 64 > 60, "whole tiles of spoiled candidates"
