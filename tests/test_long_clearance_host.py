"""Scene clearance of stitched long motions on the host (no GPU): the restatement of `LongGuidance(stitch, clearance=...)` in plain torch
(`long_clearance_reference`: join -> positions -> per window the clearance sums of its own frames against its own cloud -> the crossfade of
the two windows' sums per long frame -> columns or the adjoint -> windows; the GPU tests import it with the fixtures) against autograd of the
omega-weighted energy, the conditions the GPU fixtures meet, every refusal (raised before a device is touched), the loop-call plan of term
"long_scene", and the C surface (declared, mirrored field for field, ABI version 7)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm import diffusion as gd
from afm.cmdm import CMDM, plan_loop_call
from afm.diffusion import ContactGuidance, JointTargets, LongGuidance, SceneClearance, Stitch
from afm.pipeline import long_motion_sample
from conftest import ROOT
from test_clearance_host import RADIUS, _coef, clearance_reference, clearance_sums, h3d_clearance_reference, obstacle_weight
from test_ddim_host import _diffusion
from test_long_guidance_host import L, S, _Stub, case_id, case_stitch, h3d_adjoint_ref, long_positions, windows_holding

NEW = {"afm_long_scene_guidance_workspace_bytes", "afm_long_scene_guidance", "afm_cmdm_long_scene_guide_loop_workspace_bytes",
       "afm_cmdm_long_scene_guide_loop_range"}
LONG_GUIDE_FIELDS = ["terms", "stitch", "frames"]          # afm_long_guide as every earlier caller laid it out
DCOLS = 36                        # the column form's motion vector: twelve triples, the first and the last never guided
H3D_JOINTS = [0, 10, 11, 12, 20, 21, 5, 7, 15, 3]
EXEMPT = 0.8
# (form, ov, tail, N, K, G): every overlap with and without a padded tail; N = 1100 crosses the 1024-point tile and K = 10 gives 6 frames
# per block, so a window of 8 frames is one full block and one part-filled block; the smallest counts; one run of a single long motion
CASES = [(form, ov, tail, 130, 6, 2) for form in ("cols", "h3d") for ov in (3, 0, 4) for tail in (0, 2)] + \
        [("cols", 3, 2, 1100, 10, 2), ("h3d", 3, 2, 130, 10, 2)] + [(form, 3, 0, 1, 1, 2) for form in ("cols", "h3d")] + \
        [(form, 3, 2, 130, 6, 1) for form in ("cols", "h3d")]
# The seed of every case is checked on the CPU in float64 (test_fixture_conditions).  A case that stops meeting a condition gets another
# seed here, never a looser condition.
SEEDS = {("cols", 3, 0, 1, 1, 2): 3, ("h3d", 3, 0, 1, 1, 2): 1}


def case_options(case):
    """what besides the cloud decides a point's weight, by case: a per-window weight row where ov = 3, the floor where ov = 4, and the
    exemption by each window's own map everywhere but at N = 1 (one point per window: it stays an obstacle)"""
    form, ov, tail, N, K, G = case
    o = {}
    if N > 1:
        o["exempt_contact"] = EXEMPT
    if ov == 3 and N > 1:
        gen = torch.Generator().manual_seed(N + 11 * K + tail)
        w = 0.25 + 1.75 * torch.rand((G * S, N), generator=gen)
        w[torch.rand((G * S, N), generator=gen) < 0.25] = 0.0
        o["weight"] = w
    if ov == 4:
        o.update(min_height=-1.0, up=1)
    return o


def case_radius(case):
    """a radius per joint (0.5 .. 0.8); one point per window: a radius that reaches more than one frame"""
    form, ov, tail, N, K, G = case
    return [1.6] * K if N == 1 else [RADIUS + 0.06 * (k % 6) for k in range(K)]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def frame_weights(st: Stitch, dtype):
    """omega [S, L]: 1 outside the overlaps, wl[i] in an earlier window's last ov frames, wr[i] in a later window's first ov - the device
    row (float64 rounded to float32 once), as ``dtype``"""
    Sn, Lw, ov = st.windows, st.length, st.overlap
    om = torch.ones(Sn, Lw, dtype=dtype)
    if ov > 0:
        wl, wr = st.weights("cpu").to(dtype)
        for w in range(Sn):
            if w + 1 < Sn:
                om[w, Lw - ov:] = wl
            if w > 0:
                om[w, :ov] = wr
    return om


def window_sums(P, st: Stitch, q, radius, dtype, **options):
    """(S_b [G, S, L, K, 3], e_b [G, S, L, K]) of every window's own frames of the joined motion's positions P [G, F, K, 3] against its own
    cloud - `clearance_sums` of tests/test_clearance_host.py on the windows' positions -, zero at and behind F"""
    G, F, K, _ = P.shape
    Sn, Lw = st.windows, st.length
    flat = st.windows_of(P.reshape(G, F, 3 * K), Lw).view(G * Sn, Lw, K, 3)
    gone = st.x_mask(G, "cpu", Lw)
    w = obstacle_weight(q, options.get("weight"), options.get("up", 2), options.get("min_height"), options.get("c"), options.get("exempt_contact"))
    Sb, eb, u = clearance_sums(flat, q, w, radius, dtype)
    zero = torch.zeros((), dtype=dtype)
    Sb, eb = torch.where(gone[..., None, None], zero, Sb), torch.where(gone[..., None], zero, eb)
    hit = ((u > 0) & (w[:, None, None, :] != 0)).any(-1)          # [B, L, K]: an obstacle point inside the radius
    return Sb.view(G, Sn, Lw, K, 3), eb.view(G, Sn, Lw, K), hit, ~gone


def crossfade(Sb, st: Stitch, F, dtype):
    """J [G, F, K, 3]: a frame in one window takes that window's sum as it is, a frame in two (wl[i] * S_earlier) + (wr[i] * S_later)"""
    G, Sn, Lw, K, _ = Sb.shape
    hop = Lw - st.overlap
    wts = st.weights("cpu").to(dtype)
    rows = []
    for f in range(F):
        ws = windows_holding(f, Sn, Lw, st.overlap)
        if len(ws) == 1:
            rows.append(Sb[:, ws[0], f - ws[0] * hop])
        else:
            i = f - ws[1] * hop
            rows.append(wts[0, i] * Sb[:, ws[0], f - ws[0] * hop] + wts[1, i] * Sb[:, ws[1], i])
    return torch.stack(rows, 1)


def long_clearance_reference(x, st, q, cols=None, joints=None, mean=None, std=None, scale=None, to_scene=None, radius=RADIUS, weight=None, up=2,
                             min_height=None, c=None, exempt_contact=None, t=None, t_start=None, dtype=torch.float64, long_grad=False, long=None):
    """(grad [G * S, L, D], E_clearance [G]) of `LongGuidance(stitch, clearance=...)` in ``dtype``, plain torch.  q / weight / c are per
    window [G * S, ...]; scale and to_scene per long motion; ``t`` [G * S] (long motion g has t[g * S]).  ``long_grad``: the gradient per
    long frame [G, F, D] instead; ``long``: the joined motion itself (autograd differentiates with respect to it)."""
    long = st.join(x) if long is None else long
    G, F, D = long.shape
    Sn, Lw = st.windows, st.length
    P = long_positions(long, cols, joints, mean, std, to_scene, dtype)
    K = P.shape[2]
    Sb, eb, _, _ = window_sums(P, st, q, radius, dtype, weight=weight, up=up, min_height=min_height, c=c, exempt_contact=exempt_contact)
    J = crossfade(Sb, st, F, dtype)
    coef = _coef(radius, K, dtype).to(dtype)
    if joints is not None:
        grad = h3d_adjoint_ref(long, coef.view(1, 1, -1, 1) * J, joints, mean, std, scale, to_scene, dtype)
    else:
        idx = torch.tensor([[col + a for a in range(3)] for col in cols])
        grad = torch.zeros(G, F, D, dtype=dtype)
        grad[:, :, idx] = ((scale.to(dtype).view(-1, 1, 1, 1) * coef.view(1, 1, -1, 1)) * std.to(dtype)[idx]) * J
    if t is not None and t_start is not None:
        grad = torch.where((t.view(G, Sn)[:, 0] >= t_start).view(G, 1, 1), torch.zeros((), dtype=dtype), grad)
    om = frame_weights(st, dtype)
    energy = torch.zeros(G, dtype=dtype)
    for w in range(Sn):                                       # the windows' E_b added in window order
        energy = energy + (om[w].view(1, Lw, 1) * eb[:, w]).sum((1, 2))
    return (grad if long_grad else st.windows_of(grad, Lw)), energy


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def long_clear_case(case):
    """The inputs of one kernel case (CPU float32 tensors): the windows x of a random long motion (shared frames bit-identical, a zero
    padded tail), a cloud, an exemption map and (by case) a weight row PER WINDOW, the joints with a radius each, mean / std, per-motion
    scales and to_scene.  A share of each window's points is scattered around joint positions of its own frames, the rest over the room."""
    form, ov, tail, N, K, G = case
    st = case_stitch(case)
    F, B = st.frames, G * S
    D = 263 if form == "h3d" else DCOLS
    tag = f"long_clear_{case_id(case)}_s{SEEDS.get(case, 0)}"
    long = synth.gaussian(tag + "_x", (G, F, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    cols = joints = to_scene = None
    if form == "h3d":
        joints = H3D_JOINTS[:K]
        mean[0:3] = 0.0
        std[0], std[1:3] = 0.05, 0.1
        to_scene = torch.eye(3, 4).repeat(G, 1, 1) + 0.3 * synth.gaussian("long_clear_to_scene", (G, 3, 4))          # per motion, not orthogonal
    else:
        cols = [3 * j for j in range(1, K + 1)]               # (triples 0 and 11 stay unguided)
    x = st.windows_of(long, L)
    P = long_positions(long, cols, joints, mean, std, to_scene, torch.float32)
    near = max(1, (3 * N) // 10)                              # the points scattered around a joint-frame of the window
    q = 2.0 * synth.gaussian(tag + "_q", (B, N, 3))
    pick = torch.Generator().manual_seed(1000 + N + K + ov + tail + 7 * SEEDS.get(case, 0))
    hop = L - ov
    for b in range(B):
        g, w = divmod(b, S)
        n_w = min(L, F - w * hop)
        fs = torch.randint(0, n_w, (near,), generator=pick) + w * hop
        ks = torch.randint(0, K, (near,), generator=pick)
        if N == 1:                                            # the one point of a window: next to a frame it shares with a neighbour
            fs[0] = (hop if w == 0 else w * hop) + 1
        q[b, :near] = P[g, fs, ks] + (0.5 if N == 1 else 0.3) * q[b, :near] / 2.0
    c = torch.rand((B, N, 2), generator=torch.Generator().manual_seed(N * 100 + K))
    scale = torch.tensor([1.0, 2.5])[:G]
    return dict(st=st, x=x, q=q, c=c, cols=cols, joints=joints, mean=mean, std=std, scale=scale, to_scene=to_scene, radius=case_radius(case),
                options=case_options(case))


def ref_args(g):
    """the arguments of long_clearance_reference of a case"""
    a = {k: g[k] for k in ("st", "x", "q", "cols", "joints", "mean", "std", "scale", "to_scene", "radius")}
    o = dict(g["options"])
    if "exempt_contact" in o:
        o["c"] = g["c"]
    return dict(a, **o)


def clearance_of(g, move=lambda t: t, **kw):
    """the SceneClearance of a case (``move``: to the tensors' device)"""
    o = dict(radius=g["radius"], scale=g["scale"], **g["options"])
    o.update(kw)
    if g["joints"] is not None:
        ts = None if g["to_scene"] is None else move(g["to_scene"])
        return SceneClearance.h3d(g["joints"], g["mean"], g["std"], to_scene=ts, **o)
    return SceneClearance(g["cols"], g["mean"], g["std"], **o)


def guidance_of(g, move=lambda t: t, **kw):
    return LongGuidance(g["st"], clearance=clearance_of(g, move, **kw))


def fixture_report(case):
    """per window (share of its valid joint-frames with an obstacle inside the radius, how many have none) and, for ov > 0, how many
    overlap joint-frames have nonzero, different sums from their two windows - float64"""
    g = long_clear_case(case)
    st, a = g["st"], ref_args(g)
    P = long_positions(st.join(g["x"]), g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float64)
    opts = {k: a[k] for k in ("weight", "up", "min_height", "c", "exempt_contact") if k in a}
    Sb, eb, hit, valid = window_sums(P, st, g["q"], g["radius"], torch.float64, **opts)
    cover = [(hit[b][valid[b]].double().mean().item(), int((~hit[b][valid[b]]).sum())) for b in range(hit.shape[0])]
    differ = 0
    hop = L - st.overlap
    for w in range(1, S if st.overlap > 0 else 0):
        for i in range(st.overlap):
            e, l = Sb[:, w - 1, hop + i], Sb[:, w, i]          # [G, K, 3]
            differ += int((e.abs().amax(-1).gt(0) & l.abs().amax(-1).gt(0) & (e != l).any(-1)).sum())
    return cover, differ


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixture_conditions(case):
    """In every window at least a quarter of the valid joint-frames have an obstacle inside the radius and at least one has none; with
    ov > 0 at least one overlap frame has nonzero, different sums from its two windows."""
    cover, differ = fixture_report(case)
    print(f"[long clearance host] {case_id(case)}: per window (share with an obstacle, count without) {[(round(s, 2), n) for s, n in cover]}, "
          f"overlap joint-frames with two different nonzero sums {differ}")
    assert all(share >= 0.25 and none >= 1 for share, none in cover)
    assert case[1] == 0 or differ >= 1


# ---------------------------------------------------------------------------------------------------------------- against autograd
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_float64_gradient_equals_autograd_of_the_weighted_energy(case):
    """-autograd of sum_g scale_g E_clearance[g] with respect to the long motion - E the omega-weighted energy - is the gradient: 1e-12
    relative, both forms."""
    g = long_clear_case(case)
    st, a = g["st"], ref_args(g)
    want, e = long_clearance_reference(**a, long_grad=True)
    long = st.join(g["x"]).double().requires_grad_(True)
    e_auto = long_clearance_reference(**a, long=long)[1]
    (auto,) = torch.autograd.grad((g["scale"].double() * e_auto).sum(), long)
    err, big = (want + auto).abs().max().item(), auto.abs().max().item()
    print(f"[long clearance host] analytic vs autograd {case_id(case)}: max|diff| = {err:.3e} (max|grad| = {big:.3e})")
    assert err <= 1e-12 * max(1.0, big) and big > 0 and torch.equal(e, e_auto.detach()) and (e > 0).all()
    # back in the windows: both copies of a shared frame hold the same values, the padded tail and the unnamed columns are zero
    G = case[5]
    gw = st.windows_of(want, L).view(G, S, L, -1)
    for k in range(S - 1):
        assert st.overlap == 0 or torch.equal(gw[:, k, L - st.overlap:], gw[:, k + 1, :st.overlap])
    pad = st.full(L) - st.frames
    assert pad == 0 or not gw[:, -1, L - pad:].any()
    named = torch.zeros(want.shape[-1], dtype=torch.bool)
    if g["joints"] is not None:
        named[:67] = True
    else:
        for col in g["cols"]:
            named[col:col + 3] = True
    assert not want[..., ~named].any()
    # t of long motion g is t[g * S]
    t = torch.zeros(G * S, dtype=torch.int64)
    t[0], t[1:S] = 10, 0
    late = long_clearance_reference(**a, t=t, t_start=10, long_grad=True)[0]
    assert not late[0].any() and torch.equal(late[1:], want[1:])


@pytest.mark.parametrize("form", ["cols", "h3d"])
def test_one_window_is_the_single_window_reference(form):
    """S = 1, F = L: the long reference is clearance_reference / h3d_clearance_reference of the same x without a mask."""
    g = long_clear_case((form, 3, 2, 130, 6, 2))
    F = g["st"].frames
    one = Stitch(1, 0, length=F)
    long = g["st"].join(g["x"])
    a = ref_args(g)
    a.update(st=one, x=long, q=g["q"][::S], c=g["c"][::S], weight=a["weight"][::S])
    got, e = long_clearance_reference(**a)
    names = dict(joints=a.pop("joints"), to_scene=a.pop("to_scene")) if form == "h3d" else dict(cols=a.pop("cols"))
    for k in ("st", "joints", "to_scene", "cols"):
        a.pop(k, None)
    single = h3d_clearance_reference if form == "h3d" else clearance_reference
    want, e1 = single(x_mask=None, **a, **names)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max() and (e - e1).abs().max() <= 1e-12 * e1.abs().max() and want.abs().max() > 0


def test_identical_clouds_give_the_single_scene_push_and_an_exemption_fades():
    """What the crossfade is for: with the same cloud in both windows an overlap frame gets wl * S + wr * S - the single-scene push up to
    rounding (ov = 3: the weights are quarters, wl + wr == 1 exactly), not twice it; and a point only the earlier window's map exempts
    pushes with wr[i] alone."""
    g = long_clear_case(("cols", 3, 0, 130, 6, 2))
    st, a = g["st"], ref_args(g)
    F = st.frames
    a.update(q=g["q"][::S].repeat_interleave(S, 0), weight=None, exempt_contact=None, c=None)
    J, _ = long_clearance_reference(**a, long_grad=True)
    one = Stitch(1, 0, length=F)
    a1 = dict(a, st=one, x=st.join(g["x"]), q=g["q"][::S])
    want, _ = long_clearance_reference(**a1)
    assert (J - want).abs().max() <= 1e-12 * want.abs().max() and want.abs().max() > 0
    # the exemption of the earlier window alone: the overlap frames get wr[i] times the later window's push
    c = torch.zeros(2 * S, 130, 2)
    c[0::S] = 1.0                                             # window 0 of every long motion exempts every point
    a.update(c=c, exempt_contact=0.5)
    faded, _ = long_clearance_reference(**a, long_grad=True)
    hop, wr = L - st.overlap, st.weights("cpu")[1].double()
    assert not faded[:, :hop].any()
    for i in range(st.overlap):
        assert (faded[:, hop + i] - wr[i] * want[:, hop + i]).abs().max() <= 1e-12 * want.abs().max()
    rest = slice(hop + st.overlap, 2 * hop)                   # window 1 alone: the push as it is
    assert (faded[:, rest] - want[:, rest]).abs().max() <= 1e-12 * want.abs().max() and faded[:, rest].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------- refusals, on the host
def _clear(G=2, N=5, D=DCOLS, **kw):
    return SceneClearance([3, 6], torch.zeros(D), torch.ones(D), radius=0.5, **kw)


def test_refusals_are_raised_before_a_device_is_touched():
    st = Stitch(S, 3, length=L)                               # F = 18
    B = 2 * S
    x, t = torch.zeros(B, L, DCOLS), torch.zeros(B, dtype=torch.int64)
    kw = dict(c_pc_xyz=torch.zeros(B, 5, 3), c_pc_contact=torch.zeros(B, 5, 2))
    with pytest.raises(TypeError, match="must be a SceneClearance"):
        LongGuidance(st, clearance=ContactGuidance([3], torch.zeros(DCOLS), torch.ones(DCOLS)))
    with pytest.raises(ValueError, match="at least one of"):
        LongGuidance(st, None, None, None)
    calls = lambda lg: (lambda v: lg(v, t, **kw), lambda v: lg.clearance_energy(v, **kw), lambda v: lg.describe(v, kw))
    for call in calls(LongGuidance(st, clearance=_clear())):
        with pytest.raises(ValueError, match="no multiple of 3 windows"):
            call(torch.zeros(7, L, DCOLS))
        with pytest.raises(ValueError, match="the windows have 8 frames"):
            call(torch.zeros(B, 9, DCOLS))
        with pytest.raises(ValueError, match="describe 36 columns"):
            call(torch.zeros(B, L, 24))
    for call in calls(LongGuidance(st, clearance=_clear(scale=torch.ones(B)))):          # a per-window scale
        with pytest.raises(ValueError, match="one value per window"):
            call(x)
    with pytest.raises(ValueError, match="3 values for 2 long motions"):
        LongGuidance(st, clearance=_clear(scale=torch.ones(3)))(x, t, **kw)
    for call in calls(LongGuidance(st, clearance=_clear(weight=torch.ones(2, 5)))):      # a weight per long motion
        with pytest.raises(ValueError, match="weight is per window"):
            call(x)
    with pytest.raises(ValueError, match=r"weight is \(6, 4\), the scene needs \[6, 5\]"):          # another N
        LongGuidance(st, clearance=_clear(weight=torch.ones(B, 4)))(x, t, **kw)
    with pytest.raises(ValueError, match=r"c_pc_xyz must be \[6, N, 3\]"):           # the clouds are per window
        LongGuidance(st, clearance=_clear())(x, t, c_pc_xyz=torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="exempt_contact reads c_pc_contact"):
        LongGuidance(st, clearance=_clear(exempt_contact=0.5))(x, t, c_pc_xyz=kw["c_pc_xyz"])
    with pytest.raises(ValueError, match=r"c_pc_contact must be \[6, 5, J\]"):       # the exemption maps too
        LongGuidance(st, clearance=_clear(exempt_contact=0.5))(x, t, c_pc_xyz=kw["c_pc_xyz"], c_pc_contact=torch.zeros(2, 5, 2))
    # terms that disagree
    ct = ContactGuidance([3, 6], torch.zeros(DCOLS), torch.ones(DCOLS))
    with pytest.raises(ValueError, match="different mean / std"):
        LongGuidance(st, ct, None, SceneClearance([3], torch.ones(DCOLS), torch.ones(DCOLS), radius=0.5))
    m263, s263 = torch.zeros(263), torch.ones(263)
    with pytest.raises(ValueError, match="HumanML3D features"):
        LongGuidance(st, ContactGuidance([3], m263, s263), None, SceneClearance.h3d([0], m263, s263, radius=0.5))
    with pytest.raises(ValueError, match="different to_scene"):
        LongGuidance(st, ContactGuidance.h3d([0], m263, s263, to_scene=torch.eye(3, 4)), None,
                     SceneClearance.h3d([0], m263, s263, radius=0.5, to_scene=2 * torch.eye(3, 4)))
    # h3d: to_scene per long motion, and F bounded by the 7 * F floats of the recovery's LDS
    with pytest.raises(ValueError, match="6 matrices for 2 long motions"):
        LongGuidance(st, clearance=SceneClearance.h3d([0], m263, s263, radius=0.5, to_scene=torch.zeros(B, 3, 4)))(torch.zeros(B, L, 263), t, **kw)
    big = Stitch(3, 0, length=800)                             # F = 2400 > 61440 / 28
    with pytest.raises(ValueError, match="LDS"):
        LongGuidance(big, clearance=SceneClearance.h3d([0], m263, s263, radius=0.5))(torch.zeros(3, 800, 263), t[:3], c_pc_xyz=torch.zeros(3, 5, 3))
    # the energies of the other two terms keep their 2-tuple; the clearance has its own
    assert LongGuidance(st, clearance=_clear()).energies(x, **kw) == (None, None)
    with pytest.raises(ValueError, match="needs a clearance"):
        LongGuidance(st, ct).clearance_energy(x, **kw)
    assert LongGuidance(st, ct, None, _clear(t_start=300)).t_start is None and LongGuidance(st, clearance=_clear(t_start=300)).t_start == 300
    d = _diffusion(1000, "ddim5")
    both = LongGuidance(st, ContactGuidance([3, 6], torch.zeros(DCOLS), torch.ones(DCOLS), t_start=d.timestep_map[1] + 1), None,
                        _clear(t_start=d.timestep_map[3] + 1))
    assert both.first_guided(d) == 1 and both.clearance.first_guided(d) == 1 and both.contact.first_guided(d) == 3


def test_samplers_take_a_long_guidance_with_a_clearance_on_the_chains_geometry_and_nothing_else():
    d = _diffusion(1000, "ddim5")
    st, shape, x = Stitch(S, 3, length=L), (2 * S, L, DCOLS), torch.zeros(2 * S, L, DCOLS)
    clear = _clear()
    lg = LongGuidance(st, clearance=clear)
    check = gd.GaussianDiffusion._check_stitch
    check(st, _Stub(), shape, lg)                              # accepted
    check(Stitch(S, 3, length=L), _Stub(), shape, lg)          # an equal geometry
    with pytest.raises(ValueError, match="another Stitch"):   # another Stitch geometry
        check(Stitch(S, 2, length=L), _Stub(), shape, lg)
    with pytest.raises(ValueError, match="LongGuidance"):     # a bare clearance keeps its refusal, which names what carries one
        check(st, _Stub(), shape, clear)
    for loop in (d.ddim_sample_loop, d.dpm_solver_sample_loop):
        m = _Stub()
        loop(m, shape, noise=x, cond_fn=lg, model_kwargs={}, stitch=st)
        assert m.got is not None and m.got["contact_guide"] is lg and m.got["stitch"] is st          # handed on as the guide
        m = _Stub()
        with pytest.raises(ValueError, match="pass its Stitch as stitch="):          # an unstitched chain
            loop(m, shape, noise=x, cond_fn=lg, model_kwargs={})
        with pytest.raises(ValueError, match="another Stitch"):
            loop(m, shape, noise=x, cond_fn=lg, model_kwargs={}, stitch=Stitch(S, 0, length=L))
        with pytest.raises(ValueError, match="LongGuidance"):
            loop(m, shape, noise=x, cond_fn=clear, model_kwargs={}, stitch=st)
        assert m.got is None
    # the native loop's own refusals, before it touches the device
    for guide, kw, why in ((clear, dict(ddim_eta=0.0), "a cond_fn guidance with stitch= is not built"), (lg, dict(), "ancestral"),
                           (lg, dict(ddim_eta=0.5), "ddim_eta = 0.5")):
        with pytest.raises(ValueError, match=why):
            CMDM.afm_native_loop(None, d, x, {}, _guidance=(None, False, guide, st), **kw)
    with pytest.raises(ValueError, match="another Stitch"):
        CMDM.afm_native_loop(None, d, x, {}, ddim_eta=0.0, _guidance=(None, False, lg, Stitch(S, 2, length=L)))
    with pytest.raises(ValueError, match="pass its Stitch as stitch="):
        CMDM.afm_native_loop(None, d, x, {}, ddim_eta=0.0, _guidance=(None, False, lg, None))
    # the pipeline: shapes that do not fit are refused before the first stage runs (the models are never touched)
    assert inspect.signature(long_motion_sample).parameters["clearance"].default is None
    args = dict(text_feat=torch.zeros(2, S, 4), xyz=torch.zeros(2, 5, 3), frames=18, overlap=3)
    with pytest.raises(ValueError, match="weight is per window"):
        long_motion_sample(None, None, _Stub(), None, clearance=_clear(weight=torch.ones(2, 5)), **args)
    with pytest.raises(ValueError, match="6 values for 2 long motions"):
        long_motion_sample(None, None, _Stub(), None, clearance=_clear(scale=torch.ones(2 * S)), **args)
    with pytest.raises(ValueError, match="different mean / std"):
        long_motion_sample(None, None, _Stub(), None, contact_guidance=ContactGuidance([3], torch.ones(DCOLS), torch.ones(DCOLS)), clearance=clear, **args)
    with pytest.raises(ValueError, match="'dpm\\+\\+' or 'ddim'"):
        long_motion_sample(None, None, None, None, sampler="ddpm", clearance=clear, **args)


# ---------------------------------------------------------------------------------------------------------------- the loop call
@pytest.mark.parametrize("update", ["ddim", "dpm"])
@pytest.mark.parametrize("guidance", ["none", "cfg", "cfg2"])
@pytest.mark.parametrize("impute", [False, True])
def test_plan_loop_call_of_a_long_scene_term(update, guidance, impute):
    plan = plan_loop_call(update, guidance, impute, "long_scene", True)
    assert plan.entry == "afm_cmdm_long_scene_guide_loop_range" and plan.sizer == "afm_cmdm_long_scene_guide_loop_workspace_bytes"
    types = ffi.EXPORTS[plan.entry][1]
    assert len(plan.slots) == len(types) - 4 - 8                # between (w, x, cond, frame_mask) and (B, L, scratch, ws, bytes, n, streams, stream)
    assert types[4 + plan.slots.index("term")] == ctypes.POINTER(ffi.LongSceneGuide) and "stitch" not in plan.slots
    assert len(plan.size_slots) == len(ffi.EXPORTS[plan.sizer][1]) - 4 and ffi.EXPORTS[plan.sizer][1][-1] == ctypes.POINTER(ffi.LongSceneGuide)
    long = plan_loop_call(update, guidance, impute, "long", True)
    assert plan.slots == long.slots and plan.size_slots == long.size_slots          # the slots equal the "long" plan's
    assert plan.key != long.key and long.entry == "afm_cmdm_long_guide_loop_range"          # a workspace key of its own; "long" as it was


def test_plan_loop_call_refuses_what_a_long_scene_term_cannot_be():
    with pytest.raises(ValueError):
        plan_loop_call("ddpm", "none", False, "long_scene", True)
    for update in ("ddim", "dpm", "ddpm"):
        with pytest.raises(ValueError, match="stitch=False"):
            plan_loop_call(update, "none", False, "long_scene", False)
        with pytest.raises(ValueError, match="no stitched loop"):          # the single-window scene term stays unstitched
            plan_loop_call(update, "none", False, "scene", True)


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_exports_declared_structs_mirrored_and_the_abi_kept(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert ffi.ABI_VERSION == 7 and re.search(r"#define AFM_ABI_VERSION\s+7\b", hdr)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NEW) and "afm_long_scene_guide" in integration
    # the loop entry is the long loop's signature with the description swapped, the sizer likewise; the call has one more energy
    new, old = ffi.EXPORTS["afm_cmdm_long_scene_guide_loop_range"][1], ffi.EXPORTS["afm_cmdm_long_guide_loop_range"][1]
    assert new[:15] == old[:15] and new[16:] == old[16:] and new[15] == ctypes.POINTER(ffi.LongSceneGuide) and old[15] == ctypes.POINTER(ffi.LongGuide)
    sz, osz = ffi.EXPORTS["afm_cmdm_long_scene_guide_loop_workspace_bytes"][1], ffi.EXPORTS["afm_cmdm_long_guide_loop_workspace_bytes"][1]
    assert sz[:6] == osz[:6] and sz[6] == ctypes.POINTER(ffi.LongSceneGuide)
    call, ocall = ffi.EXPORTS["afm_long_scene_guidance"][1], ffi.EXPORTS["afm_long_guidance"][1]
    assert call[0] == ctypes.POINTER(ffi.LongSceneGuide) and len(call) == len(ocall) + 1 == 13 and call[1:4] == ocall[1:4] and call[7:] == ocall[6:]
    assert [f for f, _ in ffi.LongGuide._fields_] == LONG_GUIDE_FIELDS          # afm_long_guide's field list is unchanged
    assert [f for f, _ in ffi.LongSceneGuide._fields_] == ["base", "clearance"]
    if os.path.exists(ffi.lib_path()):
        lib = ffi.load()
        assert lib.afm_version() == 7 and all(hasattr(lib, n) for n in NEW)
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_long_scene_guide", ffi.LongSceneGuide), ("afm_long_guide", ffi.LongGuide), ("afm_scene_clearance", ffi.SceneClearance),
             ("afm_motion_guide", ffi.MotionGuide))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "long_scene_layout.c", tmp_path / "long_scene_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert ctypes.sizeof(ffi.LongSceneGuide) == 16 and ctypes.sizeof(ffi.LongGuide) == 32


def test_the_new_entries_refuse_before_they_enqueue():
    """AFM_E_BADARG / AFM_E_UNSUPPORTED from the entries' own checks: nothing is dereferenced on the device and nothing is launched."""
    assert os.path.exists(ffi.lib_path()), "libafm_hip.so is not built (python afford-motion_amd/build_hip.py)"
    lib = ffi.load()
    P, R = 4096, ctypes.byref
    held = []

    def clear(K=2, radius=0.5, up=2, exempt=0, c=None, mean=P, h3d=None):
        a = ffi.SceneClearance()
        a.q = a.std = a.scale = P
        a.mean, a.K, a.N, a.up, a.exempt, a.c, a.Kc = mean, K, 5, up, exempt, c, 2
        a.cols[0], a.cols[1] = 3, 6
        a.radius[0] = a.radius[1] = radius
        if h3d is not None:
            a.h3d = ctypes.pointer(h3d)
        held.append(a)
        return a

    def terms(contact=False, h3d=None):
        m = ffi.MotionGuide()
        if contact:
            cg = ffi.ContactGuide()
            cg.q = cg.c = cg.mean = cg.std = cg.scale = P
            cg.K, cg.N, cg.sigma = 2, 5, 0.8
            cg.cols[0], cg.cols[1] = 3, 6
            if h3d is not None:
                cg.h3d = ctypes.pointer(h3d)
            m.contact = ctypes.pointer(cg)
            held.append(cg)
        held.append(m)
        return m

    def guide(a="default", S_=3, ov=3, F=18, m="default", weights=P):
        g = ffi.LongGuide()
        m = terms() if m == "default" else m
        g.terms, g.stitch, g.frames = (ctypes.pointer(m) if m is not None else None), ffi.Stitch(S_, ov, weights), F
        s = ffi.LongSceneGuide()
        a = clear() if a == "default" else a
        s.base, s.clearance = ctypes.pointer(g), (ctypes.pointer(a) if a is not None else None)
        held.extend([g, s])
        return s
    run = lambda g, B=6, L_=8, D=21, x=P, grad=P: lib.afm_long_scene_guidance(R(g), x, None, grad, None, None, None, B, L_, D, P, 1 << 30, None)
    size = lambda g, B=6, L_=8, D=21: lib.afm_long_scene_guidance_workspace_bytes(R(g), B, L_, D)
    assert size(guide()) > 0 and size(guide(m=terms(contact=True))) > size(guide())
    assert run(guide(F=13)) == -1 and run(guide(F=19)) == -1            # F outside (S-1) hop + ov < F <= S L - (S-1) ov
    assert run(guide(ov=5)) == -1 and run(guide(S_=0)) == -1 and run(guide(m=None)) == -1
    assert run(guide(a=None)) == -1                                     # no term at all
    assert run(guide(), B=7) == -1 and run(guide(), x=None) == -1 and run(guide(), grad=None) == -1
    assert run(guide(), D=7) == -1                                      # a column triple outside D
    assert run(guide(clear(radius=0.0))) == -1 and run(guide(clear(radius=-1.0))) == -1 and run(guide(clear(up=3))) == -1
    assert run(guide(clear(exempt=1))) == -1                            # an exemption without c
    assert run(guide(weights=None)) == -1                               # the crossfade's row is missing
    assert run(guide(clear(mean=P + 64), m=terms(contact=True))) == -1  # terms that disagree on mean
    lay = ffi.H3dLayout()
    lay.joints[1] = 1
    assert run(guide(clear(h3d=lay), m=terms(contact=True)), D=263) == -1          # ... on the form
    lay2 = ffi.H3dLayout()
    lay2.joints[1], lay2.to_scene = 1, P
    assert run(guide(clear(h3d=lay), m=terms(contact=True, h3d=lay2)), D=263) == -1          # ... on to_scene
    assert lib.afm_long_scene_guidance(R(guide(S_=3, ov=0, F=2400, a=clear(h3d=lay))), P, None, P, None, None, None, 3, 800, 263, P, 1 << 30, None) == -3
    assert lib.afm_long_scene_guidance(R(guide()), P, None, P, P, None, None, 6, 8, 21, P, 1 << 30, None) == -1          # an energy of a term not set
    assert size(guide(), B=7) == -1 and size(guide(F=19)) == -1 and size(guide(a=None)) == -1
    assert lib.afm_long_scene_guidance(None, P, None, P, None, None, None, 6, 8, 21, P, 1 << 30, None) == -1
    w = ffi.CmdmWeights()
    ddim, noisy, dpm = ffi.DdimRows(P, P, P, P, None), ffi.DdimRows(P, P, P, P, P), ffi.DpmRows(P, P, P)

    def loop(g="default", step_noise=None, rows=R(ddim), dpm_=None, c1=None, B=6, first=0, known=None):
        g = guide() if g == "default" else g
        return lib.afm_cmdm_long_scene_guide_loop_range(R(w), P, P, None, step_noise, P, rows, dpm_, c1, c1, c1, None, None, known, None,
                                                        R(g) if g is not None else None, 5, first, 0, 0, B, 8, P, P, 1 << 20, 0, None, None)
    assert loop(c1=P, rows=None) == -1 and loop(c1=P) == -1 and loop(rows=R(noisy)) == -1 and loop(step_noise=P) == -1
    assert loop(B=7) == -1 and loop(g=None) == -1 and loop(first=-1) == -1 and loop(known=P) == -1
    assert loop(rows=None) == -1 and loop(dpm_=R(dpm)) == -1 and loop(g=guide(m=None)) == -1
    assert lib.afm_cmdm_long_scene_guide_loop_workspace_bytes(R(w), 6, 8, 0, None, None, None) == -1
