"""Host side of tests/test_gpu_point_train_edges.py: the input families that take the scene branch's training kernels
(csrc/pointnet_train.hip, afm_interpolate / its segmented backward) to their shape, dispatch and value edges, the plain restatements they are
compared with (one function per operator, run in float64 and in float32 on the CPU), and the proof - on the CPU - that every family is the
edge it claims to be and that every float32-class bound the GPU module uses is non-vacuous.

The dispatch rules of the BatchNorm statistics (launch_colstats / stat_plan) and of the vector-attention aggregation (afm_pt_aggregate /
afm_pt_aggregate_bwd) are RESTATED here as small pure functions, to be checked against the source by eye; every shape of the GPU module is
asserted to reach the arm it is meant to reach.

Tolerances are the ones tests/test_gpu_train.py states for the same operators.  BatchNorm's 2e-5 there is for inputs 1.5 N(0, 1) + 0.3, whose
affine terms |x scale| stay below BN_TERM = 8; y = x scale + shift rounds each term at the term's own size before they cancel, so bn_tol
grows with max|x scale| beyond that (a column of mean 1e3 and sigma 0.5 has terms of 2000: one float32 ulp of them is 1.2e-4)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from afm import synth

MARGIN = 4.0
EPS, MOMENTUM = 1e-5, 0.1
BN_TOL, BN_GRAD_TOL, BN_RUN_TOL, BN_TERM = 2e-5, 5e-5, 1e-5, 8.0          # test_batch_norm_train_forward_backward
SEG_TOL = 2e-6                                                            # test_scatter_adds_are_deterministic_segmented_sums (scaled)
AGG_TOL, AGG_GRAD_TOL = 1e-5, 2e-5                                        # test_vector_attention_glue_ops (gradients scaled)
KINK = 1e-4                                                               # no ReLU pre-activation of a float32-class case lies this close to 0
ULP32 = 2.0 ** -23


def g(name, shape, seed=synth.NOISE_SEED):
    return synth.gaussian(name, shape, seed=seed)


# ================================================================================================ dispatch rules, restated
def bn_arm(rows, C, aligned=True):
    """launch_colstats: 16-byte lanes (colstats4_kernel) for a power-of-two C in 16..512 on 16-byte aligned pointers, otherwise
    colstats_kernel<MODE, NC> with stat_plan's CW = the power of two >= C in 4..64, NC = ceil(C / CW) rounded up to 1, 2, 4 or 8."""
    if 16 <= C <= 512 and (C & (C - 1)) == 0 and aligned:
        return "colstats4"
    CW = 4
    while CW < C and CW < 64:
        CW <<= 1
    NC = (C + CW - 1) // CW
    return "NC1" if NC == 1 else "NC2" if NC == 2 else "NC4" if NC <= 4 else "NC8"


def bn_chunks(rows, C, aligned=True):
    """-> (chunks, rows per chunk, chunks that hold no row): stat_plan's >= 16 rows per row lane capped at 1024 chunks; the 16-byte arm
    takes >= 32 rows per row lane of its own RL = 1024 / C, capped at 2048 and at stat_plan's count."""
    CW = 4
    while CW < C and CW < 64:
        CW <<= 1
    RL = 256 // CW
    ch = max(1, min(1024, (rows + RL * 16 - 1) // (RL * 16)))
    if bn_arm(rows, C, aligned) == "colstats4":
        RL4 = 1024 // C
        ch = max(1, min(2048, ch, (rows + RL4 * 32 - 1) // (RL4 * 32)))
    rpc = (rows + ch - 1) // ch
    return ch, rpc, ch - (rows + rpc - 1) // rpc


def grid_trips(n, cap=8192, per_block=256):
    """trips of a grid-stride loop over n elements launched by grid_for (at most `cap` blocks of 256)"""
    blocks = max(1, min(cap, (n + per_block - 1) // per_block))
    return (n + blocks * per_block - 1) // (blocks * per_block)


def agg_arm(k, C, share, aligned=True, backward=False):
    """afm_pt_aggregate / afm_pt_aggregate_bwd -> ("fused", G) or ("two-pass", 0): G = min(64, 8192 / (k C)) points per workgroup, shrunk
    until the dynamic LDS (forward G (kC + kCs), backward G (kC + C + 2 kCs) floats) fits 64 KB; fused only for C % 4 == 0,
    (k Cs) % 4 == 0, 16-byte aligned pointers and G >= 1."""
    Cs = C // share
    lds = (lambda G: G * (k * C + C + 2 * k * Cs) * 4) if backward else (lambda G: G * (k * C + k * Cs) * 4)
    G = min(64, 8192 // (k * C)) if k * C <= 8192 else 0
    while G > 1 and lds(G) > 65536:
        G -= 1
    if C % 4 == 0 and (k * Cs) % 4 == 0 and aligned and G >= 1 and lds(G) <= 65536:
        return "fused", G
    return "two-pass", 0


def agg_trips(m, G):
    return (m + 4096 * G - 1) // (4096 * G)


# ================================================================================================ BatchNorm
BN_CS, BN_ROWS = (1, 3, 5, 16, 96, 160, 320, 511, 512), (2, 3, 63, 257, 4097)
BN_FAMILIES = ("mean_1e3", "first_row_K10", "first_row_K30", "first_row_K100", "first_row_zero", "constant_columns", "sigma_1e-4",
               "relu_nonpositive_columns", "relu_exact_zeros")
FIRST_ROW_K = {"first_row_K10": 10.0, "first_row_K30": 30.0, "first_row_K100": 100.0, "first_row_zero": 100.0}
CONST_COLS = {0: 3.25, 3: -0.75, 7: 100.5, 8: 0.0, 13: 0.40625, 21: -17.0, 30: 1.0, 31: 2.5}       # dyadic: the float32 column mean is exact
NONPOS_COLS, ZERO_COLS = (0, 5), (1, 2)


def bn_cases():
    """name -> (rows, C, family, relu, residual, 4-byte offset view)"""
    cases = {}
    for C in BN_CS:
        for rows in BN_ROWS:
            cases[f"shape_{rows}x{C}"] = (rows, C, "gaussian", C % 2 == 1 or C == 512, rows in (3, 257), False)
    cases["offset_view_4097x32"] = (4097, 32, "gaussian", True, False, True)
    cases["aligned_4097x32"] = (4097, 32, "gaussian", True, False, False)
    cases["large_70001x64"] = (70001, 64, "gaussian", True, True, False)
    cases["large_offset_view_70001x64"] = (70001, 64, "gaussian", True, True, True)
    for C in (32, 96):
        for fam in BN_FAMILIES:
            cases[f"{fam}_4097x{C}"] = (4097, C, fam, fam.startswith("relu"), fam == "relu_exact_zeros", False)
    return cases


def bn_restatement(x, gamma, beta, dy, res, relu, dtype, running=None):
    """BatchNorm1d as the kernels fold it, in `dtype` on the CPU: batch mean and biased variance (running statistics when `running` is
    given: eval), scale = gamma rstd, shift = beta - mean scale, y = relu?(x scale + shift + residual); gradients of sum(y dy) by autograd;
    the running statistics after one step from (0, 1) with the unbiased variance."""
    T = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    x, gamma, beta, res = T(x), T(gamma), T(beta), T(res)
    rows = x.shape[0]
    if running is None:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = running[0].to(dtype), running[1].to(dtype)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * rstd
    shift = beta - mean * scale
    pre = x * scale + shift
    if res is not None:
        pre = pre + res
    y = torch.relu(pre) if relu else pre
    (y * dy.to(dtype)).sum().backward()
    out = dict(y=y.detach(), pre=pre.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, mean=mean.detach(), rstd=rstd.detach(),
               scale=scale.detach(), shift=shift.detach())
    if res is not None:
        out["dres"] = res.grad
    if running is None:
        unbiased = var.detach() * (rows / (rows - 1.0)) if rows > 1 else var.detach()
        out["running_mean"] = MOMENTUM * mean.detach()
        out["running_var"] = (1.0 - MOMENTUM) + MOMENTUM * unbiased
    return out


def _bn_raw(name):
    rows, C, fam, relu, has_res, _ = bn_cases()[name]
    tag = f"pte_bn_{rows}_{C}_{fam}"
    z = g(tag + "_x", (rows, C))
    gamma, beta = 1 + 0.1 * g(tag + "_w", (C,)), 0.1 * g(tag + "_b", (C,))
    res = g(tag + "_r", (rows, C)) if has_res else None
    if fam == "gaussian":
        x = z * 1.5 + 0.3
    elif fam == "mean_1e3":
        x = 1e3 + 0.5 * z
    elif fam in FIRST_ROW_K:
        z[1:] = (z[1:] - z[1:].mean(0)) / z[1:].std(0, unbiased=False)           # the other rows: mean 0 and sigma 1 to rounding, so K is exact
        x = 50.0 + 0.5 * z
        x[0] = 0.0 if fam == "first_row_zero" else 50.0 + 0.5 * FIRST_ROW_K[fam]
    elif fam == "sigma_1e-4":
        x = 1.0 + 1e-4 * z
    else:
        x = z * 1.5 + 0.3
    if fam == "constant_columns":
        for c, v in CONST_COLS.items():
            x[:, c] = v
    if fam == "relu_nonpositive_columns":
        beta[list(NONPOS_COLS)] = -10.0
    if fam == "relu_exact_zeros":
        gamma[list(ZERO_COLS)] = 0.0
        beta[list(ZERO_COLS)] = 0.0
        r = res[:, list(ZERO_COLS)]
        r = torch.where(r.abs() < 0.01, torch.zeros_like(r), r)
        r[::2] = 0.0                                               # half the entries exactly on the kink, the rest on both sides of it
        res[:, list(ZERO_COLS)] = r
    return x, gamma, beta, res


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """x, gamma, beta, dy, residual of a case (float32, shared: not to be written to).  With a ReLU, entries whose float64 pre-activation -
    in train mode or in the eval pass that follows - lies within KINK of 0 are moved off it (the mask of a float32 evaluation is then the
    float64 one); the exact zeros of relu_exact_zeros sit on the kink on purpose, in columns whose pre-activation is exact."""
    rows, C, fam, relu, has_res, _ = bn_cases()[name]
    x, gamma, beta, res = _bn_raw(name)
    dy = g(f"pte_bn_{rows}_{C}_dy", (rows, C))
    if relu:
        free = torch.ones(C, dtype=torch.bool)
        if fam == "relu_exact_zeros":
            free[list(ZERO_COLS)] = False
        for _ in range(20):
            tr = bn_restatement(x, gamma, beta, dy, res, relu, torch.float64)
            ev = bn_restatement(x, gamma, beta, dy, res, relu, torch.float64, running=(tr["running_mean"], tr["running_var"]))
            near = ((tr["pre"].abs() < 4 * KINK) | (ev["pre"].abs() < 4 * KINK)) & free
            if not near.any():
                break
            x = torch.where(near, x + 0.03125, x)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, res=res)


@functools.lru_cache(maxsize=None)
def bn_reference(name, dtype, mode="train"):
    rows, C, fam, relu, has_res, _ = bn_cases()[name]
    i = bn_inputs(name)
    tr = bn_restatement(i["x"], i["gamma"], i["beta"], i["dy"], i["res"], relu, dtype)
    if mode == "train":
        return tr
    run64 = bn_reference(name, torch.float64)
    return bn_restatement(i["x"], i["gamma"], i["beta"], i["dy"], i["res"], relu, dtype, running=(run64["running_mean"], run64["running_var"]))


def bn_tol(name):
    i, r = bn_inputs(name), bn_reference(name, torch.float64)
    return BN_TOL * max(1.0, (i["x"].double() * r["scale"]).abs().max().item() / BN_TERM)


BN_CHECKED = ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")           # + dres where there is a residual


def bn_checks(name, mode="train"):
    """(key, tolerance, divisor, floor_at or None) of every quantity the GPU module puts through report_f32_class.  The gradients are compared after division
    by the size of their terms, as tests/test_gpu_train.py's rel() does: dbeta and dres by max|ref|; dgamma = sum g x rstd - mean rstd sum g by
    the size of those two terms, max|x rstd| max|dbeta|, where that is the larger; dx by max|gamma rstd| max|dy| -
    with two or three rows dx is what is left of terms of that size after they cancel (xhat is +-1 whatever x is), and max|dx| says nothing."""
    t = bn_tol(name)
    i, r = bn_inputs(name), bn_reference(name, torch.float64, mode)
    top = lambda key: max(r[key].abs().max().item(), 1e-12)
    relu = bn_cases()[name][3]
    gm = i["dy"].double() * (r["y"] > 0) if relu else i["dy"].double()
    xhat = (i["x"].double() - r["mean"]) * r["rstd"]
    dg_div = max(top("dgamma"), (i["x"].double() * r["rstd"]).abs().max().item() * top("dbeta"))
    out = [("y", t, 1.0, None), ("dx", BN_GRAD_TOL * t / BN_TOL, r["scale"].abs().max().item() * i["dy"].abs().max().item(), None),
           ("dgamma", BN_GRAD_TOL * t / BN_TOL, dg_div, partial_sum_size(gm * xhat) / dg_div),
           ("dbeta", BN_GRAD_TOL, top("dbeta"), partial_sum_size(gm) / top("dbeta"))]
    if i["res"] is not None:
        out.append(("dres", 1e-6, top("dres"), None))
    if mode == "train":
        out += [("running_mean", BN_RUN_TOL * t / BN_TOL, 1.0, None), ("running_var", BN_RUN_TOL, 1.0, None)]
    return out


def scaled(ref64, *ts):
    s = max(ref64.abs().max().item(), 1e-12)
    return [t / s for t in ts]


def f32_class_bound(want32, want64, margin=MARGIN, floor_at=None):
    """gpu_util.report_f32_class's bound on max|got - want64|"""
    return margin * (want32.double() - want64).abs().max().item() + ULP32 * (want64.abs().max().item() if floor_at is None else floor_at)


def partial_sum_size(terms):
    """max over columns and rows j of |sum_{r <= j} terms[r]| in float64: the size of the largest partial sum of a column sum taken in row
    order.  dbeta = sum_r g_r and dgamma = sum_r g_r xhat_r are sums of +-O(1) terms whose total can be far smaller than their partial
    sums (4097 x 1: dbeta 14.8, partial sums up to 35.0); a float32 evaluation rounds each partial sum to 2^-24 of ITS size, so one ulp of the
    total - report_f32_class's floor - is not the resolution of such a sum, and a reference whose single draw came out at 0.2 ulp (torch's
    pairwise sum on that case; the ascending float32 sum of the same terms is 13 ulp off) leaves no class to be in.  The floor of a column
    sum is therefore one ulp of partial_sum_size; nothing else about the bound changes."""
    return terms.double().cumsum(0).abs().max().item()


# ---- sync combination on one GPU: `world` equal row slices, rank r shifted by 10 r sigma
SYNC_CASES = [(2, 512, 32), (8, 512, 32), (2, 300, 96), (8, 300, 96)]               # (world, rows per rank, C): colstats4 and NC2


@functools.lru_cache(maxsize=None)
def sync_inputs(world, rows, C):
    x = (g(f"pte_sync_{world}_{rows}_{C}", (world, rows, C)) * 0.5 + 1.0)
    x = x + (10.0 * 0.5) * torch.arange(world, dtype=torch.float32)[:, None, None]
    return dict(x=x.reshape(world * rows, C).contiguous(), gamma=1 + 0.1 * g(f"pte_sync_w_{C}", (C,)), beta=0.1 * g(f"pte_sync_b_{C}", (C,)))


@functools.lru_cache(maxsize=None)
def sync_reference(world, rows, C, dtype):
    i = sync_inputs(world, rows, C)
    return bn_restatement(i["x"], i["gamma"], i["beta"], torch.zeros_like(i["x"]), None, False, dtype)


SYNC_CHECKED = ("mean", "rstd", "scale", "shift", "running_mean", "running_var")


def sync_tol(ref64):
    """BN_RUN_TOL = 1e-5 is for statistics of size <= 1; the shifted ranks take the mean to 18 and the variance to 130: it grows with them"""
    return BN_RUN_TOL * max(1.0, ref64.abs().max().item())


# ================================================================================================ scatter plan / segmented sum
BIG_DST = 262144 + 1025
# (n_dst, entries, kind).  The rank pass is quadratic in a segment's length, so 2_200_000 entries go to n_dst >= 1023 only; the list with
# every entry on ONE destination has 4096 entries.
PLAN_CASES = [(1, 0, "uniform"), (1, 7, "uniform"), (1023, 0, "uniform"), (1023, 7, "uniform"), (1024, 7, "uniform"), (1025, 7, "uniform"),
              (BIG_DST, 0, "uniform"), (BIG_DST, 7, "uniform"), (1023, 2_200_000, "uniform"), (1024, 2_200_000, "uniform"),
              (1025, 2_200_000, "uniform"), (BIG_DST, 2_200_000, "uniform"),
              (1025, 4096, "one_destination"), (1, 4096, "one_destination"), (1025, 5000, "descending"), (700, 5000, "out_of_range"),
              (BIG_DST, 300_000, "out_of_range")]
SEG_LAYOUTS = [(1, 2, 1), (3, 8, 4), (40, 43, 3)]                                   # (C, ld, column offset): ld > C


@functools.lru_cache(maxsize=None)
def plan_indices(n_dst, entries, kind):
    """int32 index list.  uniform: random over the first 7/8 of the destinations (the rest stay empty), the first quarter (at most 40000 entries) folded
    onto five destinations; out_of_range: every 5th entry is -1, every 7th n_dst, every 11th 2^31 - 1 (skipped by the plan)."""
    gen = torch.Generator().manual_seed(1000 + n_dst % 997 + entries % 991)
    if kind == "one_destination":
        return torch.full((entries,), n_dst - 1, dtype=torch.int32)
    hi = max(1, n_dst - n_dst // 8)
    idx = torch.randint(0, hi, (entries,), generator=gen, dtype=torch.int32)
    if kind == "descending":
        return torch.sort(idx, descending=True).values.contiguous()
    if n_dst >= 1024:
        fold = min(entries // 4, 40_000)
        idx[:fold] = idx[:fold] % 5 + (n_dst // 2)
    if kind == "out_of_range":
        idx[::5], idx[3::7], idx[1::11] = -1, n_dst, 2 ** 31 - 1
    return idx


def plan_reference(idx, n_dst):
    """-> (offsets [n_dst + 1], entries ascending per destination): a stable sort of the valid entries"""
    idx = idx.long()
    valid = torch.nonzero((idx >= 0) & (idx < n_dst)).flatten()
    order = valid[torch.sort(idx[valid], stable=True).indices]
    off = torch.zeros(n_dst + 1, dtype=torch.long)
    off[1:] = torch.cumsum(torch.bincount(idx[valid], minlength=n_dst), 0)
    return off, order


def ascending_f32_sum(src, col, C, off, ent, row_div=1):
    """dst[d] = ((0 + v_0) + v_1) + ... over destination d's entries in ascending order, in float32: a numpy loop over the position inside
    the segment, vectorised across destinations - the order and the arithmetic segment_sum_kernel's header claims."""
    src, off, ent = src.numpy(), off.numpy(), ent.numpy()
    n_dst = len(off) - 1
    acc = np.zeros((n_dst, C), dtype=np.float32)
    length = off[1:] - off[:-1]
    for p in range(int(length.max()) if n_dst and len(ent) else 0):
        sel = np.nonzero(length > p)[0]
        acc[sel] = acc[sel] + src[ent[off[sel] + p] // row_div, col: col + C]
    return torch.from_numpy(acc)


def group_ascending_f32_sum(x, n):
    """[B n, C] -> [B, C]: ((0 + x_0) + x_1) + ... in float32 (afm_group_sum with scale 1)"""
    x = x.numpy().reshape(-1, n, x.shape[1])
    acc = np.zeros((x.shape[0], x.shape[2]), dtype=np.float32)
    for j in range(n):
        acc = acc + x[:, j]
    return torch.from_numpy(acc)


# ================================================================================================ interpolation
INTERP_CASES = [(1, 3, 1), (1, 3, 32), (1, 3, 35), (5000, 300, 1), (5000, 300, 32), (5000, 300, 35)]        # (n fine, m coarse, c)
D2_ROWS = {"one_zero": (0.0, 0.3, 0.7), "two_zeros": (0.0, 0.0, 0.4), "three_zeros": (0.0, 0.0, 0.0), "tiny": (1e-30, 0.2, 0.5),
           "huge": (1e12, 0.6, 0.1), "zero_tiny_huge": (0.0, 1e-30, 1e12), "zero_at_epsilon": (0.0, 1e-16, 0.3),      # sqrt(1e-16) = the 1e-8 itself
           "epsilon_pair": (1e-16, 1e-14, 0.9)}


@functools.lru_cache(maxsize=None)
def interp_inputs(n, m, c):
    """idx [n, 3] int32 into m coarse points, d2 [n, 3]: random rows, with the rows of D2_ROWS (in every rotation) written over the first
    ones that exist; feat [m, c], base [n, c], dout [n, c]"""
    gen = torch.Generator().manual_seed(31 + n + c)
    idx = torch.randint(0, m, (n, 3), generator=gen, dtype=torch.int32)
    d2 = torch.rand(n, 3, generator=gen) + 1e-3
    rows = [tuple(np.roll(v, s)) for v in D2_ROWS.values() for s in range(3)]
    for r, v in enumerate(rows[: n] if n > 1 else [D2_ROWS["one_zero"]]):
        d2[r] = torch.tensor(v)
    return dict(idx=idx, d2=d2, feat=g(f"pte_ip_f_{m}_{c}", (m, c)), base=g(f"pte_ip_b_{n}_{c}", (n, c)), dout=g(f"pte_ip_d_{n}_{c}", (n, c)))


@functools.lru_cache(maxsize=None)
def interp_reference(n, m, c, dtype):
    """out = base + sum_j w_j feat[idx_j], w = r / sum r, r = 1 / (sqrt(d2) + 1e-8); dfeat = the scatter of w_j dout"""
    i = interp_inputs(n, m, c)
    r = 1.0 / (torch.sqrt(i["d2"].to(dtype)) + 1e-8)
    w = r / r.sum(1, keepdim=True)
    feat, dout = i["feat"].to(dtype), i["dout"].to(dtype)
    up = sum(feat[i["idx"][:, j].long()] * w[:, j: j + 1] for j in range(3))
    dfeat = torch.zeros(m, c, dtype=dtype)
    for j in range(3):
        dfeat.index_add_(0, i["idx"][:, j].long(), dout * w[:, j: j + 1])
    return dict(up=up, out=i["base"].to(dtype) + up, dfeat=dfeat, w=w)


# ================================================================================================ grouping
GROUP_MAX_CASES = [(37, k, C) for k in (1, 2, 16) for C in (1, 3, 35)] + [(70000, 2, 32)]


@functools.lru_cache(maxsize=None)
def tie_family(m, k, C):
    """[m k, C], all <= 0, more than half the entries exactly 0 (every third of them -0.0), every 4th group zero in all k entries: what
    max-pooling post-ReLU features meets, mirrored so that the zeros ARE the maximum"""
    z = g(f"pte_tie_{m}_{k}_{C}", (m, k, C))
    x = torch.where(z > -0.2, torch.zeros_like(z), z)
    x[::4] = 0.0
    flat = x.view(-1)
    zero = torch.nonzero(flat == 0).flatten()[::3]
    flat[zero] = -0.0
    return x.view(m * k, C)


def group_max_reference(x, dy, k):
    """values, argmax = the FIRST maximum (by value: -0.0 == +0.0), dx = dy copied to it"""
    m, C = x.shape[0] // k, x.shape[1]
    xv = x.view(m, k, C)
    mx = xv.max(1).values
    arg = (xv == mx[:, None, :]).to(torch.uint8).argmax(1)                # first True
    dx = torch.zeros(m, k, C, dtype=dy.dtype).scatter_(1, arg[:, None, :], dy[:, None, :])
    return mx, arg, dx.view(m * k, C)


# ================================================================================================ vector-attention aggregation
# name -> (m, k, C, share, w2 family, arm forward, arm backward)
AGG_CASES = {
    "two_pass_C6":        (130, 16, 6, 2, "scale_1", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_C6_m5":     (5, 16, 6, 2, "scale_8", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_kCs3":      (130, 3, 4, 4, "scale_30", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_kCs3_m5":   (5, 3, 4, 4, "scale_1", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_kC16384":   (130, 16, 1024, 8, "scale_1", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_kC16384_m5": (5, 16, 1024, 8, "scale_8", ("two-pass", 0), ("two-pass", 0)),
    "fused_G64_m1":       (1, 16, 8, 8, "scale_1", ("fused", 64), ("fused", 64)),
    "fused_G64_m193":     (193, 16, 8, 8, "scale_8", ("fused", 64), ("fused", 64)),
    "fused_G2_m1":        (1, 16, 256, 8, "scale_1", ("fused", 2), ("fused", 2)),
    "fused_G2_m11":       (11, 16, 256, 8, "scale_30", ("fused", 2), ("fused", 2)),
    "fused_G1_m1":        (1, 16, 512, 8, "scale_1", ("fused", 1), ("fused", 1)),
    "fused_G1_m6":        (6, 16, 512, 8, "scale_8", ("fused", 1), ("fused", 1)),
    "fused_k1":           (130, 1, 32, 8, "scale_1", ("fused", 64), ("fused", 64)),
    "fused_scale_1":      (130, 16, 32, 8, "scale_1", ("fused", 16), ("fused", 16)),
    "fused_scale_8":      (130, 16, 32, 8, "scale_8", ("fused", 16), ("fused", 16)),
    "fused_scale_30":     (130, 16, 32, 8, "scale_30", ("fused", 16), ("fused", 16)),
    "fused_uniform":      (130, 16, 32, 8, "uniform", ("fused", 16), ("fused", 16)),
    "fused_offset_1e4":   (130, 16, 32, 8, "offset_1e4", ("fused", 16), ("fused", 16)),
    "fused_spread_200":   (130, 16, 32, 8, "spread_200", ("fused", 16), ("fused", 16)),
    "two_pass_spread_200": (130, 16, 6, 2, "spread_200", ("two-pass", 0), ("two-pass", 0)),
    "two_pass_offset_1e4": (130, 16, 6, 2, "offset_1e4", ("two-pass", 0), ("two-pass", 0)),
}
ALIGN_CASE = (130, 16, 32, 8)                                     # fused when aligned, two-pass with every tensor at a 4-byte offset
SECOND_TRIP = (4099, 16, 512, 8, 7)                               # G = 1, 4096 workgroups: three points of a second trip; tiled from 7 points
UNDERFLOW = 104.0                                                 # exp(-104) < 2^-150: no float32 evaluation keeps such a probability


def w2_family(family, z):
    if family.startswith("scale_"):
        return z * float(family.split("_")[1])
    if family == "uniform":
        return torch.full_like(z, 0.7)
    if family == "offset_1e4":
        return z + 1e4
    if family == "spread_200":
        return z * 200.0 / (z.max() - z.min())
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def agg_inputs(m, k, C, share, family):
    tag = f"pte_agg_{m}_{k}_{C}_{share}"
    return dict(vg=g(tag + "_vg", (m * k, C)), pr=g(tag + "_pr", (m * k, C)), dout=g(tag + "_do", (m, C)),
                w2=w2_family(family, g(tag + "_w2", (m * k, C // share))))


def agg_restatement(vg, pr, w2, dout, k, share, dtype, drop_max=False, drop_neighbour=False):
    """sw = softmax over the k neighbours of w2[g, :, j] (exp(w - max) / sum); out[g, s Cs + j] = sum_t (vg + pr)[g, t, s Cs + j] sw[g, t, j];
    da = dout sw; dw2 = sw (dsw - sum_t sw dsw), dsw = sum_s dout (vg + pr).  drop_max / drop_neighbour: the two wrong results the host
    asserts a bound still tells from the right one (no max subtraction - NaN or a uniform row once exp overflows; the last neighbour left
    out of the sum)."""
    m, C = vg.shape[0] // k, vg.shape[1]
    Cs = C // share
    a = (vg.to(dtype) + pr.to(dtype)).view(m, k, share, Cs)
    w = w2.to(dtype).view(m, k, Cs)
    e = torch.exp(w if drop_max else w - w.max(1, keepdim=True).values)
    sw = e / e.sum(1, keepdim=True)
    if drop_neighbour and k > 1:
        sw = torch.cat([sw[:, :-1], torch.zeros_like(sw[:, -1:])], 1)
    d = dout.to(dtype).view(m, 1, share, Cs)
    out = (a * sw[:, :, None, :]).sum(1).view(m, C)
    da = (d * sw[:, :, None, :]).reshape(m * k, C)
    dsw = (d * a).sum(2)
    dw2 = sw * (dsw - (sw * dsw).sum(1, keepdim=True))
    return dict(out=out, sw=sw.reshape(m * k, Cs), da=da, dw2=dw2.reshape(m * k, Cs))


@functools.lru_cache(maxsize=None)
def agg_reference(name, dtype):
    m, k, C, share, family, _, _ = AGG_CASES[name]
    i = agg_inputs(m, k, C, share, family)
    return agg_restatement(i["vg"], i["pr"], i["w2"], i["dout"], k, share, dtype)


AGG_CHECKED = (("out", AGG_TOL, False), ("sw", AGG_TOL, False), ("da", AGG_GRAD_TOL, True), ("dw2", AGG_GRAD_TOL, True))


# ================================================================================================ the proofs
def test_dispatch_every_arm_is_reached():
    arms = {name: bn_arm(c[0], c[1], not c[5]) for name, c in bn_cases().items()}
    for C, arm in ((1, "NC1"), (3, "NC1"), (5, "NC1"), (16, "colstats4"), (96, "NC2"), (160, "NC4"), (320, "NC8"), (511, "NC8"), (512, "colstats4")):
        for rows in BN_ROWS:
            assert arms[f"shape_{rows}x{C}"] == arm, (rows, C, arms[f"shape_{rows}x{C}"])
    assert arms["offset_view_4097x32"] == "NC1" and arms["aligned_4097x32"] == "colstats4"
    assert arms["large_70001x64"] == "colstats4" and arms["large_offset_view_70001x64"] == "NC1"
    assert set(arms.values()) == {"NC1", "NC2", "NC4", "NC8", "colstats4"}
    for fam in BN_FAMILIES:
        assert arms[f"{fam}_4097x32"] == "colstats4" and arms[f"{fam}_4097x96"] == "NC2"
    for world, rows, C in SYNC_CASES:
        assert bn_arm(rows, C) == ("colstats4" if C == 32 else "NC2")
    # (70001, 64) at a 4-byte offset: the chunk cap, chunks that hold no row, and a second grid-stride trip of colaffine / bn_bwd_apply
    ch, rpc, empty = bn_chunks(70001, 64, aligned=False)
    assert ch == 1024 and empty > 0 and rpc * (ch - empty) >= 70001
    assert bn_chunks(70001, 64)[0] < 1024 and grid_trips(70001 * 64) == 3 and grid_trips(4097 * 512) == 2
    assert bn_chunks(2, 1) == (1, 2, 0)

    got = {}
    for name, (m, k, C, share, _, fwd, bwd) in AGG_CASES.items():
        assert agg_arm(k, C, share) == fwd and agg_arm(k, C, share, backward=True) == bwd, (name, agg_arm(k, C, share), agg_arm(k, C, share, backward=True))
        got.setdefault(fwd, []).append(m)
    assert {("two-pass", 0), ("fused", 64), ("fused", 2), ("fused", 1)} <= set(got)
    for G in (64, 2, 1):                                      # one point, and a ragged last workgroup after q full ones
        assert 1 in got[("fused", G)] and any(m > G and m % G == 1 or G == 1 and m > 1 for m in got[("fused", G)]), (G, got[("fused", G)])
    m, k, C, share = ALIGN_CASE
    assert agg_arm(k, C, share)[0] == agg_arm(k, C, share, backward=True)[0] == "fused"
    assert agg_arm(k, C, share, aligned=False)[0] == agg_arm(k, C, share, aligned=False, backward=True)[0] == "two-pass"
    m, k, C, share, _ = SECOND_TRIP
    assert agg_arm(k, C, share) == agg_arm(k, C, share, backward=True) == ("fused", 1) and agg_trips(m, 1) == 2 and agg_trips(m - 3, 1) == 1
    assert agg_arm(17, 32, 8)[0] == "fused"                   # nothing in the dispatch stops k = 17: the entry points reject it first

    # scatter plan: one and several blocks of 1024 counters, a second trip of the block scan (> 256 blocks), of count / fill / rank
    assert [(n + 1023) // 1024 for n in (1, 1023, 1024, 1025, BIG_DST)] == [1, 1, 1, 2, 258]
    assert grid_trips(2_200_000) == 2 and grid_trips(4096) == 1
    for m, k, C in GROUP_MAX_CASES:
        assert grid_trips(m * C) == (2 if m == 70000 else 1)


@pytest.mark.parametrize("fam", sorted(FIRST_ROW_K))
@pytest.mark.parametrize("C", [32, 96])
def test_first_row_family_lies_K_sigma_from_the_mean(fam, C):
    x = bn_inputs(f"{fam}_4097x{C}")["x"].double()
    rest = x[1:]              # the first row itself moves the column's mean and sigma: K is stated for the distribution of the other rows
    k = (x[0] - rest.mean(0)).abs() / rest.std(0, unbiased=False)
    assert (k / FIRST_ROW_K[fam] - 1).abs().max().item() < 0.01, (fam, k.min().item(), k.max().item())
    if fam == "first_row_zero":
        assert (x[0] == 0).all() and (rest.mean(0) - 50).abs().max() < 0.05


def test_bn_value_families_are_what_they_claim():
    for C in (32, 96):
        x = bn_inputs(f"mean_1e3_4097x{C}")["x"].double()
        assert (x.mean(0) - 1e3).abs().max() < 0.05 and (x.std(0) - 0.5).abs().max() < 0.03
        x = bn_inputs(f"sigma_1e-4_4097x{C}")["x"].double()
        assert (x.mean(0) - 1).abs().max() < 1e-5 and (x.std(0) / 1e-4 - 1).abs().max() < 0.1      # (float32 spacing at 1 is 1.2e-7: ~800 levels per sigma)
        i, r = bn_inputs(f"constant_columns_4097x{C}"), bn_reference(f"constant_columns_4097x{C}", torch.float64)
        for c, v in CONST_COLS.items():
            assert (i["x"][:, c] == v).all() and r["rstd"][c].item() == EPS ** -0.5
            assert bn_reference(f"constant_columns_4097x{C}", torch.float32)["mean"][c].item() == v
        name = f"relu_nonpositive_columns_4097x{C}"
        r = bn_reference(name, torch.float64)
        for c in NONPOS_COLS:
            assert (r["pre"][:, c] < -1.0).all() and (r["dx"][:, c] == 0).all() and r["dgamma"][c] == 0 and r["dbeta"][c] == 0
        name = f"relu_exact_zeros_4097x{C}"
        i = bn_inputs(name)
        for dtype in (torch.float64, torch.float32):
            r = bn_reference(name, dtype)
            for c in ZERO_COLS:
                assert torch.equal(r["pre"][:, c], i["res"][:, c].to(dtype))              # the pre-activation is the residual, exactly
                zero = i["res"][:, c] == 0
                assert zero.float().mean() >= 0.5 and (i["res"][:, c] > 0).any() and (i["res"][:, c] < 0).any()
                assert (r["dres"][zero, c] == 0).all() and (r["dx"][:, c] == 0).all()
                assert torch.equal(r["dres"][:, c], torch.where(i["res"][:, c] > 0, i["dy"][:, c], torch.zeros(())).to(dtype))


@pytest.mark.parametrize("name", sorted(bn_cases()))
def test_bn_bounds_are_not_vacuous_and_masks_are_settled(name):
    rows, C, fam, relu, has_res, _ = bn_cases()[name]
    for mode in ("train", "eval"):
        if mode == "eval" and not name.startswith("shape_"):
            continue
        r32, r64 = bn_reference(name, torch.float32, mode), bn_reference(name, torch.float64, mode)
        if relu:
            free = torch.ones(C, dtype=torch.bool)
            if fam == "relu_exact_zeros":
                free[list(ZERO_COLS)] = False
            assert (r64["pre"][:, free].abs() >= KINK).all(), "a pre-activation on the ReLU's kink"
            assert torch.equal(r32["y"] > 0, r64["y"] > 0), "the float32 reference takes another side of the ReLU"
        for key, tol, div, floor_at in bn_checks(name, mode):
            a32, a64 = r32[key].double() / div, r64[key] / div
            err = (a32 - a64).abs().max().item()
            assert err < tol, f"{name} {mode} {key}: the float32 reference alone misses the tolerance ({err:.3e} >= {tol:.1e})"
            bound = f32_class_bound(a32, a64, floor_at=floor_at)
            assert bound < tol, f"{name} {mode} {key}: bound {bound:.3e} >= {tol:.1e} (vacuous)"
            if key == "dbeta" and fam == "relu_exact_zeros":         # a mask of y >= 0 where y > 0 is meant still leaves the widened floor by far
                i = bn_inputs(name)
                wrong = (i["dy"].double() * (r64["y"] >= 0)).sum(0) / div
                assert (wrong - a64)[list(ZERO_COLS)].abs().min().item() > 100 * bound


@pytest.mark.parametrize("world,rows,C", SYNC_CASES)
def test_sync_family_shifts_every_rank_and_keeps_a_bound(world, rows, C):
    x = sync_inputs(world, rows, C)["x"].double().view(world, rows, C)
    step = (x[1:].mean(1) - x[:-1].mean(1)) / 0.5
    assert (step - 10).abs().max() < 0.5 and (x.std(1) / 0.5 - 1).abs().max() < 0.15
    r32, r64 = sync_reference(world, rows, C, torch.float32), sync_reference(world, rows, C, torch.float64)
    for key in SYNC_CHECKED:
        tol = sync_tol(r64[key])
        assert (r32[key].double() - r64[key]).abs().max().item() < tol and f32_class_bound(r32[key], r64[key]) < tol, (key, f32_class_bound(r32[key], r64[key]))
    # the two formulas under test leave the bound by far when they are wrong: the between-rank term dropped, count for count - 1
    n = world * rows
    within = x.var(1, unbiased=False).mean(0)
    assert ((1 / torch.sqrt(within + EPS)) - r64["rstd"]).abs().max().item() > 100 * f32_class_bound(r32["rstd"], r64["rstd"])
    biased = (1 - MOMENTUM) + MOMENTUM * x.reshape(n, C).var(0, unbiased=False)
    assert (biased - r64["running_var"]).abs().max().item() > 4 * f32_class_bound(r32["running_var"], r64["running_var"])


@pytest.mark.parametrize("n_dst,entries,kind", PLAN_CASES)
def test_index_lists_have_the_stated_segments(n_dst, entries, kind):
    idx = plan_indices(n_dst, entries, kind)
    assert idx.dtype == torch.int32 and idx.numel() == entries
    off, ent = plan_reference(idx, n_dst)
    length = off[1:] - off[:-1]
    bad = int(((idx < 0) | (idx >= n_dst)).sum())
    assert off[-1].item() == entries - bad == ent.numel()
    if kind == "out_of_range":
        assert (idx == -1).sum() >= entries // 8 and (idx == n_dst).sum() >= entries // 12 and (idx == 2 ** 31 - 1).sum() >= entries // 20
        assert bad > entries // 4 and off[-1].item() > entries // 2
    else:
        assert bad == 0
    if kind == "one_destination":
        assert length[n_dst - 1].item() == entries == 4096 and int((length > 0).sum()) == 1
    if kind == "descending":
        assert (idx[1:] <= idx[:-1]).all() and idx[0] > idx[-1]
    if kind in ("uniform", "out_of_range") and n_dst >= 1023:
        assert (length == 0).sum().item() >= n_dst // 8                       # empty destinations, the last ones among them
        assert length[-1].item() == 0
    if entries >= 5000 and n_dst >= 1024 and kind != "descending":
        assert length.max().item() > 40 * max(1, entries // n_dst) or length.max().item() >= 5000      # heavily shared destinations
    if entries:
        assert length.max().item() <= 12_000                                 # the rank pass is quadratic in this
    d = idx.long()[ent]
    assert (d[1:] >= d[:-1]).all() and ((d[1:] > d[:-1]) | (ent[1:] > ent[:-1])).all()      # by destination, ascending inside it


def test_ascending_sum_is_an_order_and_not_just_a_sum():
    """The host loop adds in ascending order and that order matters at float32: the same entries added in descending order give other bits."""
    idx = plan_indices(1025, 4096, "one_destination")
    off, ent = plan_reference(idx, 1025)
    src = g("pte_seg_src_4096", (4096, 8))
    up = ascending_f32_sum(src, 4, 3, off, ent)
    down = ascending_f32_sum(src.flip(0).contiguous(), 4, 3, off, ent)
    assert not torch.equal(up, down)
    assert (up[-1].double() - src[:, 4:7].double().sum(0)).abs().max() < 2e-3 and (up[:-1] == 0).all()
    x = g("pte_bc_513", (2 * 513, 5))
    assert (group_ascending_f32_sum(x, 513).double() - x.double().view(2, 513, 5).sum(1)).abs().max() < 1e-4


@pytest.mark.parametrize("n,m,c", INTERP_CASES)
def test_d2_family_has_rows_with_one_two_and_three_zeros(n, m, c):
    i = interp_inputs(n, m, c)
    zeros = (i["d2"] == 0).sum(1)
    if n > 1:
        assert {1, 2, 3} <= set(zeros.tolist()) and (zeros > 0).sum() == 3 * 5
        assert (i["d2"] == 1e-30).any() and (i["d2"] == 1e12).any() and (i["d2"] == 1e-16).any()
        for col in range(3):
            assert (i["d2"][:, col] == 0).any()                               # a zero in every neighbour slot
    else:
        assert zeros.tolist() == [1]
    r32, r64 = interp_reference(n, m, c, torch.float32), interp_reference(n, m, c, torch.float64)
    assert torch.isfinite(r32["out"]).all() and (r64["w"].sum(1) - 1).abs().max() < 1e-12
    assert (r64["w"][: min(n, 3)].max(1).values > 1 - 1e-7).all()             # one coincident point takes (almost) all the weight
    for key, tol, is_scaled in (("out", AGG_TOL, False), ("dfeat", SEG_TOL, True)):
        a32, a64 = scaled(r64[key], r32[key].double(), r64[key]) if is_scaled else (r32[key].double(), r64[key])
        assert (a32 - a64).abs().max().item() < tol and f32_class_bound(a32, a64) < tol, (key, f32_class_bound(a32, a64), tol)
    if n > 1:                                                                 # an epsilon of 1e-6 where 1e-8 is meant leaves the bound
        r = 1.0 / (torch.sqrt(i["d2"].double()) + 1e-6)
        w = r / r.sum(1, keepdim=True)
        wrong = torch.zeros(m, c, dtype=torch.float64)
        for j in range(3):
            wrong.index_add_(0, i["idx"][:, j].long(), i["dout"].double() * w[:, j: j + 1])
        a32, a64, aw = scaled(r64["dfeat"], r32["dfeat"].double(), r64["dfeat"], wrong)
        assert (aw - a64).abs().max().item() > 10 * f32_class_bound(a32, a64)


@pytest.mark.parametrize("m,k,C", GROUP_MAX_CASES)
def test_tie_family_ties_on_the_maximum(m, k, C):
    x = tie_family(m, k, C)
    mx, arg, _ = group_max_reference(x.double(), torch.ones(m, C, dtype=torch.float64), k)
    assert (x <= 0).all() and (mx <= 0).all()
    at_max_zero = (x.view(m, k, C) == 0) & (mx[:, None, :] == 0)
    assert at_max_zero.float().mean().item() >= 0.5                           # half the entries ARE a group maximum of exactly 0
    all_tied = (x.view(m, k, C) == 0).all(1)
    assert all_tied.any() and (m < 4 or all_tied[::4].all())
    neg_zero = (x == 0) & torch.signbit(x)
    assert neg_zero.any() and ((x == 0) & ~torch.signbit(x)).any()
    # torch's max_pool1d picks the same (first) maximum, in values and in where its gradient goes
    xr = x.double().view(m, k, C).permute(0, 2, 1).clone().requires_grad_(True)
    dy = g(f"pte_tie_dy_{m}_{C}", (m, C)).double()
    y = F.max_pool1d(xr, k).squeeze(-1)
    (y * dy).sum().backward()
    _, _, dx = group_max_reference(x.double(), dy, k)
    assert torch.equal(y.detach(), mx) and torch.equal(xr.grad.permute(0, 2, 1).reshape(m * k, C), dx)
    if k > 1:                                                                 # "last maximum wins" is another gradient on this family
        last = (k - 1) - (x.view(m, k, C).flip(1) == 0).to(torch.uint8).argmax(1)
        assert (last != arg).float().mean().item() > 0.25


@pytest.mark.parametrize("name", sorted(AGG_CASES))
def test_aggregation_families_and_bounds(name):
    m, k, C, share, family, _, _ = AGG_CASES[name]
    i = agg_inputs(m, k, C, share, family)
    r32, r64 = agg_reference(name, torch.float32), agg_reference(name, torch.float64)
    Cs = C // share
    w = i["w2"].double().view(m, k, Cs)
    gap = w.max(1, keepdim=True).values - w
    if family == "uniform":
        assert (r64["sw"] == 1.0 / k).all()
    if family == "spread_200":
        dead = (gap > UNDERFLOW).reshape(m * k, Cs)
        assert dead.any() and (r32["sw"][dead] == 0).all() and (r32["dw2"][dead] == 0).all() and gap.max().item() > 150
    if family == "offset_1e4":
        assert w.min().item() > 9990
    if family == "scale_30" and k > 1:
        assert (r64["sw"].view(m, k, Cs).max(1).values > 0.99).any()
    if k == 1:
        assert (r32["sw"] == 1).all() and (r32["dw2"] == 0).all()
    for key, tol, is_scaled in AGG_CHECKED:
        if k == 1 and key == "dw2":
            continue
        a32, a64 = scaled(r64[key], r32[key].double(), r64[key]) if is_scaled else (r32[key].double(), r64[key])
        assert (a32 - a64).abs().max().item() < tol and f32_class_bound(a32, a64) < tol, (name, key, f32_class_bound(a32, a64), tol)
    if k > 1 and family != "uniform":                                        # a neighbour left out of the sum leaves the bound
        bad = agg_restatement(i["vg"], i["pr"], i["w2"], i["dout"], k, share, torch.float64, drop_neighbour=True)
        assert (bad["out"] - r64["out"]).abs().max().item() > 10 * f32_class_bound(r32["out"], r64["out"])
    if family in ("offset_1e4", "spread_200"):                               # and so does a softmax without its max subtraction
        bad = agg_restatement(i["vg"], i["pr"], i["w2"], i["dout"], k, share, torch.float32, drop_max=True)
        assert not torch.isfinite(bad["out"]).all() or (bad["out"].double() - r64["out"]).abs().max().item() > 10 * f32_class_bound(r32["out"], r64["out"])
