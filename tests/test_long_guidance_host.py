"""Guidance of stitched long motions on the host (no GPU): the float64 restatement of afm.diffusion.LongGuidance (`long_guidance_reference`:
join -> positions -> per-window terms -> joined sums -> adjoint -> windows; the GPU tests import it with the fixtures) against autograd, the
margin of the GPU fixtures' nearest-frame decisions, the rule for the windows that hold a long frame, every refusal (raised before a device
is touched), the loop-call plan of term "long", and the C surface (declared, mirrored field for field, ABI version 7)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm import diffusion as gd
from afm.cmdm import CMDM, plan_loop_call
from afm.diffusion import ContactGuidance, JointTargets, LongGuidance, MotionGuidance, Stitch
from afm.pipeline import long_motion_sample
from conftest import ROOT
from test_ddim_host import _diffusion
from test_guidance_host import JOINTS, SIGMA, contact_reference, contact_terms
from test_h3d_guidance_host import _prev, _recover, _scan, _to_scene, h3d_contact_reference, h3d_joints_ref

NEW = {"afm_long_guidance_workspace_bytes", "afm_long_guidance", "afm_stitch_guide_step", "afm_cmdm_long_guide_loop_workspace_bytes",
       "afm_cmdm_long_guide_loop_range"}
S, L = 3, 8                       # three windows of eight frames: a middle window with two neighbours
DCOLS = 21                        # the column form's motion vector: seven triples, six of them guided
DUP = (0, 5, 7)                   # long motion 0: long frame 7 repeats the pose of frame 5 bit for bit (both inside the first overlap for
#                                   ov = 3 and ov = 4) - the first long frame must win, in both windows
# (form, ov, tail, N, K, G): every overlap with and without a padded tail at the largest point and joint counts (K * N = 780: four
# blocks, the last part-filled), the small counts at ov = 3, and one run of a single long motion
CASES = [(form, ov, tail, 130, 6, 2) for form in ("cols", "h3d") for ov in (3, 0, 4) for tail in (0, 2)] + \
        [(form, 3, 0, N, K, 2) for form in ("cols", "h3d") for N, K in ((1, 1), (1, 6), (130, 1))] + \
        [(form, 3, 2, 130, 6, 1) for form in ("cols", "h3d")]
# The seed of every case is checked on the CPU (test_fixture_margin): no nearest-frame decision of any window is closer than a relative
# 1e-4 in float64 and float32 picks the same frames.  A case that stops meeting it gets another seed here, never a looser condition.
SEEDS = {("cols", 3, 0, 130, 6, 2): 5, ("cols", 3, 2, 130, 6, 2): 5, ("cols", 0, 0, 130, 6, 2): 1, ("cols", 0, 2, 130, 6, 2): 1,
         ("cols", 4, 0, 130, 6, 2): 4, ("h3d", 3, 0, 130, 6, 2): 1, ("h3d", 3, 2, 130, 6, 2): 10, ("h3d", 0, 0, 130, 6, 2): 2,
         ("h3d", 4, 0, 130, 6, 2): 9, ("h3d", 4, 2, 130, 6, 2): 4, ("h3d", 3, 0, 130, 1, 2): 3}


def case_id(case):
    return "{}_ov{}_tail{}_N{}_K{}_G{}".format(*case)


def case_stitch(case) -> Stitch:
    _, ov, tail, _, _, _ = case
    return Stitch(S, ov, S * L - (S - 1) * ov - tail, length=L)


def windows_holding(f, S_, L_, ov):
    """the one or two windows of a long motion that hold long frame f, earlier first (the rule of the long pass 2)"""
    hop = L_ - ov
    w1 = min(f // hop, S_ - 1)
    return ([w1 - 1] if w1 > 0 and f - w1 * hop < ov else []) + [w1]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def long_positions(long, cols, joints, mean, std, to_scene, dtype):
    """P [G, F, K, 3] of the joined motion: the de-normalised columns, or the h3d recovery over all F frames"""
    if joints is not None:
        return h3d_joints_ref(long, None, mean, std, joints, to_scene, dtype)
    idx = torch.tensor([[col + a for a in range(3)] for col in cols])
    return long.to(dtype)[:, :, idx] * std.to(dtype)[idx] + mean.to(dtype)[idx]


def window_positions(P, st: Stitch):
    """(the windows' positions as a motion of absolute columns [G * S, L, 3 K], its columns, zero mean, unit std, the padded-tail mask)"""
    G, F, K, _ = P.shape
    flat = st.windows_of(P.reshape(G, F, 3 * K), st.length)
    mask = st.x_mask(G, "cpu", st.length)
    return flat, [3 * k for k in range(K)], torch.zeros(3 * K, dtype=P.dtype), torch.ones(3 * K, dtype=P.dtype), mask


def long_fstar(P, st, q, c, sigma, dtype):
    """(d2 [B, N, K, L] over the window's frames, inf in the padded tail; f* [B, N, K] as LONG frame indices)"""
    flat, cols, zero, one, mask = window_positions(P, st)
    _, d2, _, fstar = contact_terms(flat, mask, q, c, cols, zero, one, sigma, dtype)
    first = (torch.arange(flat.shape[0]) % st.windows) * (st.length - st.overlap)
    return d2, fstar + first.view(-1, 1, 1)


def joined_contact_sums(P, st, q, c, sigma, dtype):
    """(coef * S joined per long frame [G, F, K, 3] - a frame in two windows: earlier + later -, E_contact [G]: the windows' E_b in order)"""
    G, F, K, _ = P.shape
    flat, cols, zero, one, mask = window_positions(P, st)
    gp, eb = contact_reference(flat, mask, q, c, cols, zero, one, torch.ones(flat.shape[0]), sigma, dtype)
    gp = gp.view(G, st.windows, st.length, K, 3)
    out = torch.zeros(G, F, K, 3, dtype=dtype)
    for f in range(F):
        ws = windows_holding(f, st.windows, st.length, st.overlap)
        terms = [gp[:, w, f - w * (st.length - st.overlap)] for w in ws]
        out[:, f] = terms[0] if len(terms) == 1 else terms[0] + terms[1]
    energy = torch.zeros(G, dtype=dtype)
    for w in range(st.windows):
        energy = energy + eb.view(G, st.windows)[:, w]
    return out, energy


def h3d_adjoint_ref(long, Sx, joints, mean, std, scale, to_scene, dtype):
    """scale * std * (the adjoint of the recovery over the F frames applied to Sx [G, F, K, 3]) - the chain of h3d_contact_reference"""
    G, F, D = long.shape
    u, cc, ss, _, _, vx, vz = _recover(long, None, mean, std, dtype)
    A = _to_scene(to_scene, G, dtype)
    du = torch.zeros(G, F, D, dtype=dtype)
    gX, gZ, T = (torch.zeros(G, F, dtype=dtype) for _ in range(3))
    for k, j in enumerate(joints):
        Gx, Gy, Gz = (((A[:, 0, a, None] * Sx[:, :, k, 0] + A[:, 1, a, None] * Sx[:, :, k, 1]) + A[:, 2, a, None] * Sx[:, :, k, 2]) for a in range(3))
        gX, gZ = gX + Gx, gZ + Gz
        if j == 0:
            du[..., 3] = Gy
            continue
        col = 4 + 3 * (j - 1)
        lx, lz = u[..., col], u[..., col + 2]
        du[..., col], du[..., col + 1], du[..., col + 2] = Gx * cc + Gz * ss, Gy, -Gx * ss + Gz * cc
        T = T + (Gx * (-lx * ss - lz * cc) + Gz * (lx * cc - lz * ss))
    SX, SZ = _scan(gX, reverse=True), _scan(gZ, reverse=True)
    T = 2 * (T + SX * (-_prev(vx) * ss - _prev(vz) * cc) + SZ * (_prev(vx) * cc - _prev(vz) * ss))
    du[:, :-1, 1] = (SX * cc + SZ * ss)[:, 1:]
    du[:, :-1, 2] = (-SX * ss + SZ * cc)[:, 1:]
    du[..., 0] = _scan(T, reverse=True, exclusive=True)
    return scale.to(dtype).view(-1, 1, 1) * std.to(dtype) * du


def long_guidance_reference(x, st, q=None, c=None, cols=None, joints=None, mean=None, std=None, scale=None, to_scene=None, target=None,
                            weight=None, tscale=None, tjoints=None, sigma=SIGMA, dtype=torch.float64, long_grad=False):
    """(grad [G * S, L, D], E_contact [G] or None, E_targets [G] or None) of LongGuidance's docstring in ``dtype``, plain torch.  q / c: the
    contact term's (None: no contact term); target / weight / tscale: the targets' in the long form (None: none); ``cols`` or ``joints``
    name the form; ``tjoints``: the targets' own columns or joints (None: the contact term's).  ``long_grad``: the gradient per long frame [G, F, D] instead."""
    long = st.join(x)
    G, F, D = long.shape
    h3d = joints is not None                                 # (a targets-only h3d case names its joints in `joints` too)
    grad = torch.zeros(G, F, D, dtype=dtype)
    ec = et = None
    stdd = std.to(dtype)
    if q is not None:
        P = long_positions(long, cols, joints, mean, std, to_scene, dtype)
        cS, ec = joined_contact_sums(P, st, q, c, sigma, dtype)
        if joints is not None:
            grad = grad + h3d_adjoint_ref(long, cS, joints, mean, std, scale, to_scene, dtype)
        else:
            for k, col in enumerate(cols):
                grad[:, :, col:col + 3] = scale.to(dtype).view(-1, 1, 1) * stdd[col:col + 3] * cS[:, :, k]
    if target is not None:
        names = tjoints if tjoints is not None else (joints if joints is not None else cols)
        P = long_positions(long, None if h3d else names, names if h3d else None, mean, std, to_scene, dtype)
        tg, w = target.to(dtype), weight.to(dtype)
        d = P - torch.where(w[..., None] == 0, P, tg)           # (a target with w == 0 is not read: it may be NaN)
        et = (w * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])).sum((1, 2))
        tS = 2 * (w[..., None] * -d)
        if h3d:
            grad = grad + h3d_adjoint_ref(long, tS, names, mean, std, tscale, to_scene, dtype)
        else:
            tgrad = torch.zeros(G, F, D, dtype=dtype)
            for k, col in enumerate(names):
                tgrad[:, :, col:col + 3] = tscale.to(dtype).view(-1, 1, 1) * stdd[col:col + 3] * tS[:, :, k]
            grad = grad + tgrad
    return (grad if long_grad else st.windows_of(grad, st.length)), ec, et


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def long_case(case):
    """The inputs of one kernel case (CPU float32 tensors): the windows x of a random long motion (shared frames bit-identical, a zero
    padded tail), q / c per window, the joints, mean / std, per-motion scales and to_scene, long-form targets - with the planted edges."""
    form, ov, tail, N, K, G = case
    st = case_stitch(case)
    F, B = st.frames, G * S
    D = 263 if form == "h3d" else DCOLS
    tag = f"long_guide_{case_id(case)}_s{SEEDS.get(case, 0)}"
    long = synth.gaussian(tag + "_x", (G, F, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    cols = joints = to_scene = None
    if form == "h3d":
        joints = JOINTS[:K]
        mean[0:3] = 0.0
        std[0], std[1:3] = 0.05, 0.1
        long[DUP[0], DUP[1]:DUP[2], 0:3] = 0.0               # the root stands still from frame 5 to frame 7 ...
        long[DUP[0], DUP[2], 3:] = long[DUP[0], DUP[1], 3:]   # ... and frame 7 repeats frame 5's pose
        to_scene = torch.eye(3, 4).repeat(G, 1, 1) + 0.3 * synth.gaussian("long_guide_to_scene", (G, 3, 4))          # per motion, not orthogonal
    else:
        cols = [3 * j for j in range(1, K + 1)]               # (triple 0 stays unguided)
        long[DUP[0], DUP[2]] = long[DUP[0], DUP[1]]
    x = st.windows_of(long, L)
    q = 1.5 * synth.gaussian(tag + "_q", (B, N, 3))
    P = long_positions(long, cols, joints, mean, std, to_scene, torch.float32)
    q[1, 0] = P[0, L - ov + 1, 0]                             # a point of window 1 coincident with a joint: d2 = 0, chat = 1
    if N > 1:
        q[2, N - 1] = 100.0                                   # a far point: chat underflows to 0
    c = torch.rand((B, N, K), generator=torch.Generator().manual_seed(N * 100 + K)) * 0.999 + 0.001
    if N > 2:                                                 # a target of exactly chat: a zero term
        flat, pc, zero, one, mask = window_positions(P, st)
        c[0, 1] = contact_terms(flat, mask, q, c, pc, zero, one, SIGMA, torch.float32)[2][0, 1]
    scale = torch.tensor([1.0, 2.5])[:G]
    target = P + 0.5 * synth.gaussian(tag + "_target", (G, F, K, 3))
    weight = (synth.gaussian(tag + "_weight", (G, F, K)) > 0.5).float() * (0.5 + synth.gaussian(tag + "_wv", (G, F, K)).abs())
    target[weight == 0] = float("nan")                        # never read
    tscale = torch.tensor([0.75, 1.5])[:G]
    return dict(st=st, x=x, q=q, c=c, cols=cols, joints=joints, mean=mean, std=std, scale=scale, to_scene=to_scene, target=target,
                weight=weight, tscale=tscale)


def ref_args(g, contact=True, targets=True):
    """the arguments of long_guidance_reference of a case"""
    a = {k: g[k] for k in ("st", "x", "cols", "joints", "mean", "std", "to_scene")}
    if contact:
        a.update(q=g["q"], c=g["c"], scale=g["scale"])
    if targets:
        a.update(target=g["target"], weight=g["weight"], tscale=g["tscale"])
    return a


def guidance_of(g, contact=True, targets=True, move=lambda t: t):
    """the LongGuidance of a case (``move``: to the tensors' device)"""
    ct = tg = None
    ts = None if g["to_scene"] is None else move(g["to_scene"])
    if contact:
        ct = ContactGuidance.h3d(g["joints"], g["mean"], g["std"], to_scene=ts, sigma=SIGMA, scale=g["scale"]) if g["joints"] is not None else \
            ContactGuidance(g["cols"], g["mean"], g["std"], sigma=SIGMA, scale=g["scale"])
    if targets:
        kw = dict(target=g["target"], weight=g["weight"], scale=g["tscale"])
        tg = JointTargets.h3d(g["joints"], g["mean"], g["std"], to_scene=ct.to_scene if ct is not None else ts, **kw) if g["joints"] is not None else \
            JointTargets(g["cols"], g["mean"], g["std"], **kw)
    return LongGuidance(g["st"], ct, tg)


@pytest.mark.parametrize("case", [("cols", 3, 2, 130, 6, 2), ("h3d", 3, 2, 130, 6, 2), ("h3d", 4, 0, 130, 1, 2), ("cols", 0, 0, 1, 6, 2)], ids=case_id)
def test_float64_gradient_equals_autograd_of_the_float64_energy(case):
    """-autograd of sum_g scale_g E_contact + tscale_g E_targets with respect to the long motion, f* held fixed: 1e-12 relative."""
    g = long_case(case)
    st = g["st"]
    want, ec, et = long_guidance_reference(**ref_args(g), long_grad=True)
    long = st.join(g["x"]).double().requires_grad_(True)
    P = long_positions(long, g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float64)
    G, F, K, _ = P.shape
    with torch.no_grad():
        _, fstar = long_fstar(P, st, g["q"], g["c"], SIGMA, torch.float64)
    q, c = g["q"].double(), g["c"].double()
    grp = torch.arange(G * S) // S
    pn = P[grp[:, None, None], fstar, torch.arange(K)[None, None, :]]          # [B, N, K, 3]: the nearest frame's position
    d2 = ((pn - q[:, :, None, :]) ** 2).sum(-1)
    chat = torch.exp(-d2 / (2 * SIGMA ** 2))
    eb = ((chat - c) ** 2).mean((1, 2)).view(G, S)
    w = g["weight"].double()
    dt = P - torch.where(w[..., None] == 0, P.detach(), g["target"].double())
    etg = (w * (dt * dt).sum(-1)).sum((1, 2))
    total = (g["scale"].double() * eb.sum(1)).sum() + (g["tscale"].double() * etg).sum()
    (auto,) = torch.autograd.grad(total, long)
    err, big = (want + auto).abs().max().item(), auto.abs().max().item()
    print(f"[long guidance host] analytic vs autograd {case_id(case)}: max|diff| = {err:.3e} (max|grad| = {big:.3e})")
    assert err <= 1e-12 * max(1.0, big) and big > 0
    assert (eb.sum(1).detach() - ec).abs().max() <= 1e-12 and (etg.detach() - et).abs().max() <= 1e-12 * max(1.0, et.abs().max().item())
    # back in the windows: both copies of a shared frame hold the same values, the padded tail is zero
    gw = st.windows_of(want, L).view(G, S, L, -1)
    for k in range(S - 1):
        assert st.overlap == 0 or torch.equal(gw[:, k, L - st.overlap:], gw[:, k + 1, :st.overlap])
    pad = st.full(L) - st.frames
    assert pad == 0 or not gw[:, -1, L - pad:].any()


def test_one_window_is_the_single_window_reference():
    """S = 1: the long reference is contact_reference / h3d_contact_reference of the same x without a mask."""
    st = Stitch(1, 0, length=7)
    x = synth.gaussian("long_one_x", (2, 7, 263))
    mean, std = 0.3 * synth.gaussian("long_one_mean", (263,)), 0.5 + synth.gaussian("long_one_std", (263,)).abs()
    mean[0:3], std[0], std[1:3] = 0.0, 0.05, 0.1
    q, c = 1.5 * synth.gaussian("long_one_q", (2, 9, 3)), torch.rand(2, 9, 2, generator=torch.Generator().manual_seed(3))
    scale, none = torch.tensor([1.0, 2.5]), torch.zeros(2, 7, dtype=torch.bool)
    got, ec, _ = long_guidance_reference(x, st, q, c, joints=[0, 20], mean=mean, std=std, scale=scale)
    want, e = h3d_contact_reference(x, none, q, c, [0, 20], mean, std, scale)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max() and (ec - e).abs().max() <= 1e-15
    got, ec, _ = long_guidance_reference(x, st, q, c, cols=[4, 100], mean=mean, std=std, scale=scale)
    want, e = contact_reference(x, none, q, c, [4, 100], mean, std, scale)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max() and (ec - e).abs().max() <= 1e-15


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixture_margin(case):
    """Every nearest-frame decision of the GPU fixtures, in every window, is clear in float64 (relative gap > 1e-4) but for the planted
    duplicate pose, where the first long frame wins in both windows; float32 picks the same frames: the cap on what a comparison leaves
    out is zero."""
    g = long_case(case)
    st = g["st"]
    P64 = long_positions(st.join(g["x"]), g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float64)
    d2, fstar = long_fstar(P64, st, g["q"], g["c"], SIGMA, torch.float64)
    hop = L - st.overlap
    for w in windows_holding(DUP[2], S, L, st.overlap):       # the windows of long motion 0 that hold the duplicate
        assert DUP[1] - w * hop >= 0, "the first pose lies in every window that holds its duplicate"
        assert (fstar[w] != DUP[2]).all()
        d2[w, :, :, DUP[2] - w * hop] = float("inf")          # the planted exact tie leaves the comparison
    assert (fstar >= 0).all()
    two = d2.topk(2, dim=-1, largest=False).values
    gap = (two[..., 1] - two[..., 0]) / two[..., 1]
    print(f"[long guidance host] fixture margin {case_id(case)}: smallest relative gap {gap.min().item():.3e}")
    assert gap.min().item() > 1e-4
    P32 = long_positions(st.join(g["x"]), g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float32)
    assert torch.equal(long_fstar(P32, st, g["q"], g["c"], SIGMA, torch.float32)[1], fstar)
    if st.overlap >= 3:                                       # the duplicate lies in the first overlap: both windows see both poses
        assert windows_holding(DUP[1], S, L, st.overlap) == [0, 1] and windows_holding(DUP[2], S, L, st.overlap) == [0, 1]


# ---------------------------------------------------------------------------------------------------------------- the geometry
@pytest.mark.parametrize("S_", [1, 2, 3])
@pytest.mark.parametrize("ov", [0, 3, 4])
def test_windows_holding_a_long_frame(S_, ov):
    """the rule of the long pass 2 against the windows' own frame ranges, at the full length and with a padded tail"""
    L_ = 8
    full = S_ * L_ - (S_ - 1) * ov
    lo = (S_ - 1) * (L_ - ov) + (ov if S_ > 1 else 0)
    for F in sorted({full, max(lo + 1, full - 2)}):
        st = Stitch(S_, ov, F, length=L_)
        assert st.check(S_, L_) == F
        for f in range(F):
            want = [w for w in range(S_) if w * (L_ - ov) <= f < min(w * (L_ - ov) + L_, F)]
            assert windows_holding(f, S_, L_, ov) == want, (S_, ov, F, f)
            assert 1 <= len(want) <= 2
        marks = torch.arange(F, dtype=torch.float32).view(1, F, 1)
        wins = st.windows_of(marks, L_)                       # the frames the windows really hold
        for f in range(F):
            for w in windows_holding(f, S_, L_, ov):
                assert wins[w, f - w * (L_ - ov), 0] == f


# ---------------------------------------------------------------------------------------------------------------- refusals, on the host
def _terms(G=2, F=18, scale=1.0, tscale=1.0, D=DCOLS, K=2):
    mean, std = torch.zeros(D), torch.ones(D)
    ct = ContactGuidance([3, 6][:K], mean, std, scale=scale)
    tg = JointTargets([3, 6][:K], mean, std, target=torch.zeros(G, F, K, 3), weight=torch.ones(G, F, K), scale=tscale)
    return ct, tg


def test_refusals_are_raised_before_a_device_is_touched():
    st = Stitch(S, 3, length=L)                               # F = 18
    x, t = torch.zeros(2 * S, L, DCOLS), torch.zeros(2 * S, dtype=torch.int64)
    kw = dict(c_pc_xyz=torch.zeros(2 * S, 5, 3), c_pc_contact=torch.zeros(2 * S, 5, 2))
    ct, tg = _terms()
    with pytest.raises(TypeError, match="must be a Stitch"):
        LongGuidance((3, 3), ct)
    with pytest.raises(ValueError, match="at least one of"):
        LongGuidance(st)
    with pytest.raises(ValueError, match="different mean / std"):
        LongGuidance(st, ct, JointTargets([3], torch.ones(DCOLS), torch.ones(DCOLS), target=torch.zeros(2, 18, 1, 3), weight=torch.ones(2, 18, 1)))
    lg = LongGuidance(st, ct, tg)
    for call in (lambda v: lg(v, t, **kw), lambda v: lg.energies(v, **kw), lambda v: lg.describe(v, kw)):
        with pytest.raises(ValueError, match="no multiple of 3 windows"):          # the batch
            call(torch.zeros(7, L, DCOLS))
        with pytest.raises(ValueError, match="the windows have 8 frames"):         # L
            call(torch.zeros(2 * S, 9, DCOLS))
        with pytest.raises(ValueError, match="describe 21 columns"):
            call(torch.zeros(2 * S, L, 24))
    with pytest.raises(ValueError, match="long-form"):                             # per-window targets
        LongGuidance(st, None, _terms(G=2 * S, F=L)[1])(x, t, **kw)
    with pytest.raises(ValueError, match="long-form"):                             # another F
        LongGuidance(st, None, _terms(F=16)[1])(x, t, **kw)
    for bad in (_terms(scale=torch.ones(2 * S))[0], None), (None, _terms(tscale=torch.ones(2 * S))[1]):
        with pytest.raises(ValueError, match="one value per window"):              # a per-window scale
            LongGuidance(st, *bad)(x, t, **kw)
    with pytest.raises(ValueError, match="3 values for 2 long motions"):
        LongGuidance(st, _terms(scale=torch.ones(3))[0])(x, t, **kw)
    with pytest.raises(ValueError, match=r"c_pc_xyz must be \[6, N, 3\]"):           # the maps are per window
        lg(x, t, c_pc_xyz=torch.zeros(2, 5, 3), c_pc_contact=torch.zeros(2, 5, 2))
    # h3d: to_scene per long motion, and F bounded by the 7 * F floats of the recovery's LDS
    mean, std = torch.zeros(263), torch.ones(263)
    with pytest.raises(ValueError, match="6 matrices for 2 long motions"):
        LongGuidance(st, ContactGuidance.h3d([0], mean, std, to_scene=torch.zeros(2 * S, 3, 4)))(torch.zeros(2 * S, L, 263), t, **kw)
    big = Stitch(3, 0, length=800)                             # F = 2400 > 61440 / 28
    with pytest.raises(ValueError, match="LDS"):
        LongGuidance(big, ContactGuidance.h3d([0], mean, std))(torch.zeros(3, 800, 263), t[:3], c_pc_xyz=torch.zeros(3, 5, 3),
                                                               c_pc_contact=torch.zeros(3, 5, 1))
    assert ffi.H3D_SCAN_ROWS * 2400 * 4 > ffi.GUIDE_LDS_BYTES >= ffi.H3D_SCAN_ROWS * 2194 * 4
    hdr = open(os.path.join(ROOT, "afford-motion_amd", "csrc", "guidance.hip")).read()
    assert re.search(r"GUIDE_LDS_BYTES = 60 \* 1024;", hdr) and re.search(r"H3D_SCAN_ROWS = 7;", hdr)          # the host's copy of the bound


class _Stub(torch.nn.Module):
    arch, mask_motion = "trans_enc", True

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.got = None

    def forward(self, x, t, **kw):
        return x * 0.5

    def afm_native_loop(self, diffusion, x, model_kwargs, *, stitch=None, contact_guide=None, impute=None, dpm_order=None, **kw):
        self.got = dict(stitch=stitch, contact_guide=contact_guide, dpm_order=dpm_order, **kw)
        return x


def test_samplers_take_a_long_guidance_on_the_chains_geometry_and_nothing_else():
    d = _diffusion(1000, "ddim5")
    st, shape, x = Stitch(S, 3, length=L), (2 * S, L, DCOLS), torch.zeros(2 * S, L, DCOLS)
    ct, tg = _terms()
    lg = LongGuidance(st, ct, tg)
    check = gd.GaussianDiffusion._check_stitch
    check(st, _Stub(), shape, lg)                              # accepted
    check(Stitch(S, 3, length=L), _Stub(), shape, lg)          # an equal geometry
    with pytest.raises(ValueError, match="another Stitch"):
        check(Stitch(S, 2, length=L), _Stub(), shape, lg)
    for per_window in (ct, tg, MotionGuidance(ct, tg), lambda x, t, **kw: x):          # every other cond_fn keeps its refusal
        with pytest.raises(ValueError, match="disagree in the overlaps"):
            check(st, _Stub(), shape, per_window)
    for loop in (d.ddim_sample_loop, d.dpm_solver_sample_loop):
        m = _Stub()
        loop(m, shape, noise=x, cond_fn=lg, model_kwargs={}, stitch=st)
        assert m.got is not None and m.got["contact_guide"] is lg and m.got["stitch"] is st          # handed on as the guide
        m = _Stub()
        with pytest.raises(ValueError, match="pass its Stitch as stitch="):
            loop(m, shape, noise=x, cond_fn=lg, model_kwargs={})
        with pytest.raises(ValueError, match="another Stitch"):
            loop(m, shape, noise=x, cond_fn=lg, model_kwargs={}, stitch=Stitch(S, 0, length=L))
        assert m.got is None
    with pytest.raises(ValueError, match="would have to be shared"):
        d.ddim_sample_loop(_Stub(), shape, noise=x, cond_fn=lg, model_kwargs={}, stitch=st, eta=0.5)
    with pytest.raises(ValueError, match="every ancestral step draws noise"):
        d.p_sample_loop(_Stub(), shape, noise=x, cond_fn=lg, stitch=st)
    # the native loop's own refusals, before it touches the device
    for guide, kw, why in ((object(), dict(ddim_eta=0.0), "a cond_fn guidance with stitch= is not built"),
                           (ct, dict(dpm_order=2), "a cond_fn guidance with stitch= is not built"),
                           (MotionGuidance(ct, tg), dict(ddim_eta=0.0), "a cond_fn guidance with stitch= is not built"),
                           (lg, dict(), "ancestral"), (lg, dict(ddim_eta=0.5), "ddim_eta = 0.5")):
        with pytest.raises(ValueError, match=why):
            CMDM.afm_native_loop(None, d, x, {}, _guidance=(None, False, guide, st), **kw)
    with pytest.raises(ValueError, match="another Stitch"):
        CMDM.afm_native_loop(None, d, x, {}, ddim_eta=0.0, _guidance=(None, False, lg, Stitch(S, 2, length=L)))
    with pytest.raises(ValueError, match="pass its Stitch as stitch="):
        CMDM.afm_native_loop(None, d, x, {}, ddim_eta=0.0, _guidance=(None, False, lg, None))
    # the pipeline: a deterministic sampler, long-form targets - refused before the first stage runs
    args = dict(text_feat=torch.zeros(2, S, 4), xyz=torch.zeros(2, 5, 3), frames=18, overlap=3, contact_guidance=ct)
    with pytest.raises(ValueError, match="'dpm\\+\\+' or 'ddim'"):
        long_motion_sample(None, None, None, None, sampler="ddpm", joint_targets=tg, **args)
    with pytest.raises(ValueError, match="joint_targets is the long form"):
        long_motion_sample(None, None, _Stub(), None, joint_targets=_terms(G=2 * S, F=L)[1], **args)


# ---------------------------------------------------------------------------------------------------------------- the loop call
@pytest.mark.parametrize("update", ["ddim", "dpm"])
@pytest.mark.parametrize("guidance", ["none", "cfg", "cfg2"])
@pytest.mark.parametrize("impute", [False, True])
def test_plan_loop_call_of_a_long_term(update, guidance, impute):
    plan = plan_loop_call(update, guidance, impute, "long", True)
    assert plan.entry == "afm_cmdm_long_guide_loop_range" and plan.sizer == "afm_cmdm_long_guide_loop_workspace_bytes"
    types = ffi.EXPORTS[plan.entry][1]
    assert len(plan.slots) == len(types) - 4 - 8                # between (w, x, cond, frame_mask) and (B, L, scratch, ws, bytes, n, streams, stream)
    assert types[4 + plan.slots.index("term")] == ctypes.POINTER(ffi.LongGuide) and "stitch" not in plan.slots
    assert len(plan.size_slots) == len(ffi.EXPORTS[plan.sizer][1]) - 4 and plan.size_slots[-1] == "term"
    assert ffi.EXPORTS[plan.sizer][1][-1] == ctypes.POINTER(ffi.LongGuide)
    rows = {"ddim": "ddim_rows", "dpm": "dpm_rows"}[update]
    assert rows in plan.slots and not any(s in plan.slots for s in ("c1", "c2", "sigma") + tuple(set(("ddim_rows", "dpm_rows")) - {rows}))
    assert (plan.slots[plan.slots.index("term") - 2:plan.slots.index("term")] == ("known", "mask")) == impute
    want = {"none": (None, None), "cfg": ("cfg", None), "cfg2": (None, "cfg2")}[guidance]
    assert plan.slots[7:9] == want and plan.size_slots[:2] == want
    # a workspace key of its own
    others = {plan_loop_call(update, guidance, impute, "none", True).key, plan_loop_call(update, guidance, impute, "motion", False).key,
              plan_loop_call(update, guidance, impute, "contact", False).key}
    assert plan.key not in others


def test_plan_loop_call_refuses_what_a_long_term_cannot_be():
    with pytest.raises(ValueError):
        plan_loop_call("ddpm", "none", False, "long", True)
    for update in ("ddim", "dpm", "ddpm"):
        with pytest.raises(ValueError):
            plan_loop_call(update, "none", False, "long", False)
        for term in ("contact", "motion"):                    # what the stitched loop refused, it still refuses
            with pytest.raises(ValueError, match="no stitched loop"):
                plan_loop_call(update, "none", False, term, True)


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_exports_declared_and_structs_mirrored(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert ffi.ABI_VERSION == 7 and re.search(r"#define AFM_ABI_VERSION\s+7\b", hdr)
    # the loop entry is the guided loop's signature with the description swapped, the sizer likewise
    long, guide = ffi.EXPORTS["afm_cmdm_long_guide_loop_range"][1], ffi.EXPORTS["afm_cmdm_guide_loop_range"][1]
    assert long[:15] == guide[:15] and long[16:] == guide[16:] and long[15] == ctypes.POINTER(ffi.LongGuide)
    assert ffi.EXPORTS["afm_cmdm_long_guide_loop_workspace_bytes"][1][:6] == ffi.EXPORTS["afm_cmdm_guide_loop_workspace_bytes"][1][:6]
    assert ffi.EXPORTS["afm_long_guidance"][1][0] == ctypes.POINTER(ffi.LongGuide) and len(ffi.EXPORTS["afm_long_guidance"][1]) == 12
    assert ffi.EXPORTS["afm_stitch_guide_step"][1][0] == ctypes.POINTER(ffi.StitchStepArgs) and len(ffi.EXPORTS["afm_stitch_guide_step"][1]) == 5
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NEW)
    if os.path.exists(ffi.lib_path()):
        lib = ffi.load()
        assert lib.afm_version() == 7 and all(hasattr(lib, n) for n in NEW)
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_long_guide", ffi.LongGuide), ("afm_motion_guide", ffi.MotionGuide), ("afm_stitch", ffi.Stitch),
             ("afm_stitch_step_args", ffi.StitchStepArgs))          # (the step's struct did not change)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "long_layout.c", tmp_path / "long_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert ctypes.sizeof(ffi.StitchStepArgs) == 14 * 8 + 4 * 4          # as callers laid it out


def test_the_new_entries_refuse_before_they_enqueue():
    """AFM_E_BADARG / AFM_E_UNSUPPORTED from the entries' own checks: nothing is dereferenced on the device and nothing is launched."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    P, R = 4096, ctypes.byref
    cg = ffi.ContactGuide()
    cg.q = cg.c = cg.mean = cg.std = cg.scale = P
    cg.K, cg.N, cg.sigma = 2, 5, 0.8
    cg.cols[0], cg.cols[1] = 3, 6
    m = ffi.MotionGuide()
    m.contact = ctypes.pointer(cg)

    def guide(S_=3, ov=3, F=18, terms=m):
        g = ffi.LongGuide()
        g.terms, g.stitch, g.frames = (ctypes.pointer(terms) if terms is not None else None), ffi.Stitch(S_, ov, P), F
        return g
    run = lambda g, B=6, L_=8, D=21, x=P, grad=P: lib.afm_long_guidance(R(g), x, None, grad, None, None, B, L_, D, P, 1 << 30, None)
    assert run(guide(F=13)) == -1 and run(guide(F=19)) == -1            # F outside (S-1) hop + ov < F <= S L - (S-1) ov
    assert run(guide(ov=5)) == -1 and run(guide(S_=0)) == -1 and run(guide(terms=None)) == -1
    assert run(guide(), B=7) == -1 and run(guide(), x=None) == -1 and run(guide(), grad=None) == -1
    assert run(guide(), D=7) == -1                                      # a column triple outside D
    assert lib.afm_long_guidance_workspace_bytes(R(guide()), 7, 8, 21) == -1 and lib.afm_long_guidance_workspace_bytes(R(guide(F=19)), 6, 8, 21) == -1
    assert lib.afm_long_guidance_workspace_bytes(R(guide()), 6, 8, 21) > 0
    lay = ffi.H3dLayout()
    lay.joints[1] = 1
    cg.h3d = ctypes.pointer(lay)                                        # h3d: 7 * F floats of LDS
    assert run(guide(S_=3, ov=0, F=2400), B=3, L_=800, D=263) == -3 and lib.afm_long_guidance_workspace_bytes(R(guide(S_=3, ov=0, F=2400)), 3, 800, 263) == -1
    cg.h3d = None
    w = ffi.CmdmWeights()
    ddim, noisy, dpm = ffi.DdimRows(P, P, P, P, None), ffi.DdimRows(P, P, P, P, P), ffi.DpmRows(P, P, P)

    def loop(g=guide(), step_noise=None, rows=R(ddim), dpm_=None, c1=None, B=6, first=0, known=None):
        return lib.afm_cmdm_long_guide_loop_range(R(w), P, P, None, step_noise, P, rows, dpm_, c1, c1, c1, None, None, known, None,
                                                  R(g) if g is not None else None, 5, first, 0, 0, B, 8, P, P, 1 << 20, 0, None, None)
    assert loop(c1=P, rows=None) == -1 and loop(c1=P) == -1 and loop(rows=R(noisy)) == -1 and loop(step_noise=P) == -1
    assert loop(B=7) == -1 and loop(g=None) == -1 and loop(first=-1) == -1 and loop(known=P) == -1
    assert loop(rows=None) == -1 and loop(dpm_=R(dpm)) == -1 and loop(g=guide(terms=None)) == -1
    assert lib.afm_cmdm_long_guide_loop_workspace_bytes(R(w), 6, 8, 0, None, None, None) == -1
    a = ffi.StitchStepArgs()
    st = ffi.Stitch(3, 3, P)
    a.x0_c, a.x_t, a.x_next, a.stitch, a.B, a.L, a.D, a.ddim = P, P, P + 64, ctypes.pointer(st), 6, 8, 21, ctypes.pointer(ddim)
    assert lib.afm_stitch_guide_step(R(a), None, P, None, None) == -1 and lib.afm_stitch_guide_step(R(a), P, None, None, None) == -1
    assert lib.afm_stitch_guide_step(None, P, P, None, None) == -1
    a.B = 7
    assert lib.afm_stitch_guide_step(R(a), P, P, None, None) == -1       # B % S != 0
    a.B, a.ddim = 6, ctypes.pointer(noisy)
    assert lib.afm_stitch_guide_step(R(a), P, P, None, None) == -1       # a noise term
