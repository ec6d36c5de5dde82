"""Foot grounding on the host (no GPU): the plain-torch restatement of FootGrounding's energy and gradient in both forms
(`grounding_reference`, `h3d_grounding_reference`; the GPU tests import them with the fixtures) against autograd of its own float64 energy
with the pair weights detached; that the fixtures are not trivial; the descent case; the Python refusals; the C surface; the loop call plan
and the routing of the samplers."""
import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm.cmdm import plan_loop_call
from afm.diffusion import ContactGuidance, FootGrounding, JointTargets, MotionGuidance, SceneClearance
from afm.guidance import LongGuidance, Stitch
from conftest import ROOT

from test_guidance_host import SCATTERED, _Bundle, _Names, _NamesNot, _diffusion
from test_h3d_guidance_host import ZUP, h3d_joints_ref

NEW = {"afm_ground_guidance", "afm_ground_guidance_workspace_bytes", "afm_cmdm_ground_guide_loop_range", "afm_cmdm_ground_guide_loop_workspace_bytes"}
B = 3                             # sample 0: every frame valid; sample 1: a padded tail; sample 2: every frame padded
FEET = [7, 10, 8, 11]             # HumanML3D: left ankle, left toes, right ankle, right toes
SLOT = {7: 0, 10: 1, 8: 2, 11: 3}
LABEL_COL = 259


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _heights(height, K):
    return [float(height)] * K if not hasattr(height, "__len__") else [float(h) for h in height]


def _const(v, dtype):
    """a constant formed in float64 and rounded once to ``dtype``"""
    return torch.tensor(v, dtype=torch.float64).to(dtype)


def ground_terms(p, valid, lab, floor, height, up, floor_weight, skate_weight, dtype):
    """(m [B, L, K, 3], E [B], s [B, L-1, K], pen [B, L, K]) of the positions p [B, L, K, 3] in ``dtype``, operation by operation as the
    definition has it.  ``valid`` [B, L] bool; ``lab`` [B, L, K] the clamped labels in ``dtype`` (contact="labels") or None.  The pair
    weights s enter as constants (detached): m is -dE/dp with s held."""
    K = p.shape[2]
    ih = _const([1.0 / h for h in _heights(height, K)], dtype)
    fw, sw = _const(float(floor_weight), dtype), _const(float(skate_weight), dtype)
    cf, cs = _const(2.0 * float(floor_weight), dtype), _const(2.0 * float(skate_weight), dtype)
    h = p[..., up] - _const(float(floor), dtype)
    pen = torch.clamp(-h, min=0)
    gate = torch.clamp(1 - h * ih, min=0, max=1)
    pair = (valid[:, :-1] & valid[:, 1:])[..., None]                         # [B, L-1, 1]
    s = (gate[:, :-1] * gate[:, 1:]) if lab is None else lab[:, :-1]
    s = torch.where(pair, s, torch.zeros((), dtype=dtype)).detach()
    a, b = [ax for ax in range(3) if ax != up]
    dl = p[:, 1:][..., [a, b]] - p[:, :-1][..., [a, b]]                       # [B, L-1, K, 2]
    skate = sw * (s * (dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]))
    zero = torch.zeros_like(pen[:, :1])
    item = fw * (pen * pen) + torch.cat([skate, zero], 1)
    E = torch.where(valid[..., None], item, torch.zeros((), dtype=dtype)).sum((1, 2))
    sd = s[..., None] * dl                                                    # s[f] * dl[f]
    pad2 = torch.zeros_like(p[:, :1][..., :2])
    mab = cs * (torch.cat([sd, pad2], 1) - torch.cat([pad2, sd], 1))          # s[f] dl[f] - s[f-1] dl[f-1]
    m = torch.zeros_like(p)
    m[..., up], m[..., a], m[..., b] = cf * pen, mab[..., 0], mab[..., 1]
    m = torch.where(valid[..., None, None], m, torch.zeros((), dtype=dtype))
    return m, E, s, pen


def _valid(x, x_mask):
    return torch.ones(x.shape[:2], dtype=torch.bool) if x_mask is None else ~x_mask


def grounding_reference(x, x_mask, cols, mean, std, scale, floor=0.0, height=0.05, up=2, floor_weight=1.0, skate_weight=1.0, t=None, t_start=None,
                        dtype=torch.float64):
    """(-scale * dE/dx [B, L, D] with s held, E [B]) of the column form in ``dtype``, plain torch: p = x * std, + mean;
    grad[b,f,cols[k]+a] = (scale * std_a) * m_a"""
    idx = torch.tensor([[col + a for a in range(3)] for col in cols])
    xs, mean, std = x.to(dtype), mean.to(dtype), std.to(dtype)
    p = xs[:, :, idx] * std[idx] + mean[idx]                    # [B, L, K, 3]
    m, E, _, _ = ground_terms(p, _valid(x, x_mask), None, floor, height, up, floor_weight, skate_weight, dtype)
    grad = torch.zeros(x.shape, dtype=dtype)
    grad[:, :, idx] = (scale.to(dtype).view(-1, 1, 1, 1) * std[idx]) * m.detach()
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, E


def _labels(x, mean, std, joints, dtype):
    cols = [LABEL_COL + SLOT[j] for j in joints]
    return torch.clamp(x.detach()[..., cols].to(dtype) * std[cols].to(dtype) + mean[cols].to(dtype), min=0, max=1)


def h3d_grounding_reference(x, x_mask, joints, mean, std, scale, to_scene=None, floor=0.0, height=0.05, up=2, floor_weight=1.0,
                            skate_weight=1.0, contact="height", t=None, t_start=None, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D] with s held, E [B]) of FootGrounding.h3d in ``dtype``: m on the positions of the float recovery of
    tests/test_h3d_guidance_host.py, carried back to the features by torch.autograd on that recovery (a vector-Jacobian product with m)"""
    xs = x.detach().to(dtype).requires_grad_(True)
    p = h3d_joints_ref(xs, x_mask, mean, std, joints, to_scene, dtype)
    lab = _labels(x, mean, std, joints, dtype) if contact == "labels" else None
    m, E, _, _ = ground_terms(p.detach(), _valid(x, x_mask), lab, floor, height, up, floor_weight, skate_weight, dtype)
    (du,) = torch.autograd.grad(p, xs, m)
    grad = scale.to(dtype).view(-1, 1, 1) * du
    if x_mask is not None:
        grad = torch.where(x_mask[..., None], torch.zeros_like(grad), grad)
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, E


def reference(g, **kw):
    """either form's restatement of a case"""
    return (h3d_grounding_reference if "joints" in g else grounding_reference)(**{**g, **kw})


# ---------------------------------------------------------------------------------------------------------------- the fixtures
OPTIONS = {"plain": {}, "up1": dict(up=1), "floor only": dict(skate_weight=0.0), "skate only": dict(floor_weight=0.0),
           "heights": dict(height=[0.6, 1.2, 0.9, 1.5]), "weights": dict(floor_weight=0.7, skate_weight=2.5)}
# (form, L, K, D, mask) of the kernel cases.  L = 7 is the main shape; L = 1 has no pair, L = 2 has one.  mask "tail": sample 1's last two
# frames padded (L = 2: its last; L = 1: none); "middle": also an interior padded frame in sample 0, which takes both pairs around it (the
# h3d recovery assumes valid-frames-first and does not get it).  Sample 2 is padded throughout.
COLUMN_CASES = [("pos", 7, K, D, "tail") for K in (1, 4) for D in (66, 263)] + [("pos", 7, 4, 66, "middle"), ("pos", 1, 4, 66, "tail"),
                                                                                  ("pos", 2, 1, 263, "tail")]
H3D_CASES = [("h3d", 7, K, 263, "tail") for K in (1, 4)] + [("h3d", 1, 4, 263, "tail"), ("h3d", 2, 4, 263, "tail")]
MAIN = [c for c in COLUMN_CASES + H3D_CASES if c[1] == 7]
FLOOR, HEIGHT = 0.1, 1.0
# the seed of a case is the smallest at which its inputs meet `nontrivial` (chosen on the CPU; test_the_fixtures_are_not_trivial asserts
# it): a case that stops meeting it gets another seed here, never a looser condition
# (L = 1, 2: the smallest at which sample 0 has a joint below the floor under every variant, so that the floor term acts)
SEEDS = {("pos", 7, 1, 66, "tail"): 1, ("pos", 7, 1, 263, "tail"): 17, ("h3d", 7, 1, 263, "tail"): 1, ("pos", 1, 4, 66, "tail"): 1,
         ("h3d", 1, 4, 263, "tail"): 3}


def case_id(case):
    return "{}-L{}-K{}-D{}-{}".format(*case)


def case_mask(L, kind):
    mask = torch.zeros(B, L, dtype=torch.bool)
    if L >= 2:
        mask[1, L - (2 if L >= 4 else 1):] = True
    if kind == "middle":
        mask[0, 3] = True
    mask[2, :] = True
    return mask


@functools.lru_cache(maxsize=None)
def _base(case):
    form, L, K, D, kind = case
    tag = f"ground_{case_id(case)}_s{SEEDS.get(case, 0)}"
    x = synth.gaussian(tag + "_x", (B, L, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    g = dict(x=x, x_mask=case_mask(L, kind), mean=mean, std=std, scale=torch.tensor([1.0, 2.5, 0.5]))
    if form == "h3d":
        mean[0:3] = 0.0
        std[0], std[1:3] = 0.05, 0.1
        return dict(g, joints=FEET[:K] if K > 1 else [10], to_scene=ZUP.clone())
    return dict(g, cols=[3 * j for j in FEET[:K]] if D == 66 else SCATTERED[:K])


def ground_case(case, name="plain", **more):
    """The inputs of one kernel case (CPU float32 tensors; shared, read-only) with the options of a named variant"""
    o = dict(OPTIONS[name]) if name != "labels" else dict(contact="labels")
    if "height" in o:
        o["height"] = o["height"][:case[2]]
    return {**_base(case), "floor": FLOOR, "height": HEIGHT, **o, **more}


def positions(g, dtype=torch.float64):
    if "joints" in g:
        return h3d_joints_ref(g["x"], g["x_mask"], g["mean"], g["std"], g["joints"], g["to_scene"], dtype)
    idx = torch.tensor([[col + a for a in range(3)] for col in g["cols"]])
    return g["x"].to(dtype)[:, :, idx] * g["std"].to(dtype)[idx] + g["mean"].to(dtype)[idx]


def terms64(g):
    lab = _labels(g["x"], g["mean"], g["std"], g["joints"], torch.float64) if g.get("contact") == "labels" else None
    return ground_terms(positions(g), _valid(g["x"], g["x_mask"]), lab, g["floor"], g["height"], g.get("up", 2), g.get("floor_weight", 1.0),
                        g.get("skate_weight", 1.0), torch.float64)


def coverage(g):
    """per sample with a valid frame: (share of its valid pairs with s > 0, valid pairs with s == 0, valid joint-frames below the floor,
    valid joint-frames not below it), on the float64 restatement"""
    _, _, s, pen = terms64(g)
    valid = _valid(g["x"], g["x_mask"])
    out = {}
    for b in range(B):
        if not valid[b].any():
            continue
        pairs = (valid[b, :-1] & valid[b, 1:])
        sb, pb = s[b][pairs], pen[b][valid[b]]
        out[b] = ((sb > 0).double().mean().item() if sb.numel() else 0.0, int((sb == 0).sum()), int((pb > 0).sum()), int((pb == 0).sum()))
    return out


def nontrivial(g):
    cov = coverage(g)
    return set(cov) == {0, 1} and all(share >= 0.25 and zero >= 1 and below >= 1 and above >= 1 for share, zero, below, above in cov.values())


@pytest.mark.parametrize("case", MAIN, ids=case_id)
def test_the_fixtures_are_not_trivial(case):
    names = ["plain", "heights"] + (["labels"] if case[0] == "h3d" else [])
    for name in names:
        g = ground_case(case, name)
        print(f"[grounding host] {case_id(case)} {name}: (share of pairs with s > 0, pairs with s == 0, joint-frames below, not below) {coverage(g)}")
        assert nontrivial(g), (case, name)


# ---------------------------------------------------------------------------------------------------------------- against autograd
def _autograd(g):
    """-d(sum_b scale[b] E[b])/dx by torch.autograd on the restatement's own float64 energy, the pair weights detached"""
    x = g["x"].double().requires_grad_(True)
    valid = _valid(g["x"], g["x_mask"])
    if "joints" in g:
        p = h3d_joints_ref(x, g["x_mask"], g["mean"], g["std"], g["joints"], g["to_scene"], torch.float64)
        lab = _labels(g["x"], g["mean"], g["std"], g["joints"], torch.float64) if g.get("contact") == "labels" else None
    else:
        idx = torch.tensor([[col + a for a in range(3)] for col in g["cols"]])
        p, lab = x[:, :, idx] * g["std"].double()[idx] + g["mean"].double()[idx], None
    E = ground_terms(p, valid, lab, g["floor"], g["height"], g.get("up", 2), g.get("floor_weight", 1.0), g.get("skate_weight", 1.0), torch.float64)[1]
    (auto,) = torch.autograd.grad((E * g["scale"].double()).sum(), x)
    return -auto, E.detach()


VARIANTS = [(case, name) for case in COLUMN_CASES + H3D_CASES for name in list(OPTIONS) + (["labels"] if case[0] == "h3d" else [])]


@pytest.mark.parametrize("case,name", VARIANTS, ids=lambda v: case_id(v) if isinstance(v, tuple) else v.replace(" ", "_"))
def test_gradient_equals_autograd_of_the_float64_energy_with_the_weights_held(case, name):
    g = ground_case(case, name)
    want, e = reference(g)
    auto, e_auto = _autograd(g)
    err = (want - auto).abs().max().item()
    print(f"[grounding host] {case_id(case)} {name}: analytic vs autograd max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item()) and torch.equal(e, e_auto)
    zero = lambda v: torch.equal(v, torch.zeros_like(v))
    assert zero(want[2]) and zero(want[g["x_mask"]]) and e[2] == 0 and (e[0] > 0 or (case[1] == 1 and name == "skate only"))
    if "cols" in g:
        named = torch.zeros(case[3], dtype=torch.bool)
        for col in g["cols"]:
            named[col:col + 3] = True
        assert zero(want[..., ~named])
    else:
        assert zero(want[..., 67:])
    if case[1] == 7:
        assert want[0].abs().max() > 0 and want[1].abs().max() > 0
        late = reference(g, t=torch.tensor([500, 499, 0]), t_start=500)[0]
        assert zero(late[0]) and torch.equal(late[1:], want[1:])
        if name != "plain" and case[2] == 4:                     # the option acts (one joint: a height may leave every gate saturated)
            assert not torch.equal(want, reference(ground_case(case))[0])
    if case[1] == 1:                                             # no pair: only the floor
        assert torch.equal(want, reference({**g, "skate_weight": 7.0})[0]) and (name != "skate only" or zero(want))


def test_an_interior_padded_frame_takes_both_pairs_around_it():
    g = ground_case(("pos", 7, 4, 66, "middle"))
    _, _, s, _ = terms64(g)
    assert not s[0, 2].any() and not s[0, 3].any() and s[0, [0, 1, 4, 5]].any()
    want = reference(g)[0]
    assert not want[0, 3].any()


# ---------------------------------------------------------------------------------------------------------------- descent
EPS = 0.2                         # the step of the descent case: chosen on the CPU so that the float64 energy falls by at least 10 %


def effect_case():
    """A foot below `height` that slides at constant horizontal speed, two of its frames under the floor (samples 0 and 1, sample 1 at
    twice the speed with its last two frames padded; sample 2 stands still above `height`: E = 0).  Column form, D = 6, identity
    de-normalisation: column triple 3 is the foot."""
    L = 8
    x = torch.zeros(B, L, 6)
    f = torch.arange(L, dtype=torch.float32)
    for b, speed in ((0, 0.05), (1, 0.1)):
        x[b, :, 3], x[b, :, 4], x[b, :, 5] = speed * f, 0.5 * speed * f, 0.02
        x[b, 3:5, 5] = -0.03
    x[2, :, 5] = 0.5
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, L - 2:] = True
    return dict(x=x, x_mask=mask, cols=[3], mean=torch.zeros(6), std=torch.ones(6), scale=torch.ones(B), floor=0.0, height=0.1, up=2,
                floor_weight=1.0, skate_weight=1.0)


def descent64(g, eps=EPS):
    """(E before, E after one step x + eps * guide(x)) in float64"""
    grad, e0 = grounding_reference(**g)
    return e0, grounding_reference(**{**g, "x": g["x"].double() + eps * grad})[1]


def test_one_step_along_the_guidance_lowers_the_float64_energy_by_a_tenth():
    g = effect_case()
    e0, e1 = descent64(g)
    print(f"[grounding descent host] eps = {EPS}: energy {e0.tolist()} -> {e1.tolist()} (ratio {(e1[:2] / e0[:2]).tolist()})")
    pen = terms64(g)[3]
    assert int((pen[0] > 0).sum()) == 2 and (e0[:2] > 0).all() and e0[2] == 0 and e1[2] == 0
    assert (e1[:2] <= 0.9 * e0[:2]).all()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals():
    mean, std = torch.zeros(66), torch.ones(66)
    m263, s263 = torch.zeros(263), torch.ones(263)
    for bad in (0.0, -1.0, [0.5, 0.0], float("inf")):
        with pytest.raises(ValueError, match="^FootGrounding: .*height"):
            FootGrounding([0, 3], mean, std, height=bad)
    with pytest.raises(ValueError, match="height must be a positive float or 2 of them, got 3"):
        FootGrounding([0, 3], mean, std, height=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match=r"^FootGrounding\.h3d: every height must be positive"):
        FootGrounding.h3d([7, 10], m263, s263, height=-0.5)
    for up in (3, -1):
        with pytest.raises(ValueError, match="up names a coordinate 0..2"):
            FootGrounding([0, 3], mean, std, up=up)
    for kw in (dict(floor_weight=-1.0), dict(skate_weight=-0.5), dict(floor_weight=float("nan"))):
        with pytest.raises(ValueError, match="must be >= 0"):
            FootGrounding([0, 3], mean, std, **kw)
    with pytest.raises(ValueError, match="both 0"):
        FootGrounding([0, 3], mean, std, floor_weight=0.0, skate_weight=0.0)
    with pytest.raises(ValueError, match="floor must be a finite height"):
        FootGrounding([0, 3], mean, std, floor=float("nan"))
    with pytest.raises(ValueError, match="contact must be 'height' or 'labels'"):
        FootGrounding([0, 3], mean, std, contact="velocity")
    with pytest.raises(ValueError, match="needs FootGrounding.h3d"):          # labels on the column form
        FootGrounding([0, 3], m263, s263, contact="labels")
    with pytest.raises(ValueError, match="reads columns 259..262, the motion vector has 67"):
        FootGrounding.h3d([7, 10], m263[:67], s263[:67], contact="labels")
    with pytest.raises(ValueError, match=r"labels for the joints 7, 10, 8 and 11 only, got \[0\]"):
        FootGrounding.h3d([7, 0], m263, s263, contact="labels")
    with pytest.raises(ValueError, match="^FootGrounding: 1 to 16 guided joints, got 0$"):
        FootGrounding([], mean, std)
    with pytest.raises(ValueError, match="^FootGrounding: 1 to 16 guided joints, got 17$"):
        FootGrounding(list(range(0, 51, 3)), mean, std)
    with pytest.raises(ValueError):
        FootGrounding.h3d([], m263, s263)
    with pytest.raises(ValueError):
        FootGrounding.h3d(list(range(17)), m263, s263)
    with pytest.raises(ValueError, match="overlaps"):
        FootGrounding([0, 2], mean, std)
    with pytest.raises(ValueError, match="leaves the motion vector"):
        FootGrounding([0, 64], mean, std)
    with pytest.raises(ValueError, match="named twice"):
        FootGrounding.h3d([7, 7], m263, s263)
    x, t = torch.zeros(2, 5, 66), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="holds 3 values for a batch of 2"):
        FootGrounding([0, 3], mean, std, scale=torch.ones(3))(x, t)
    with pytest.raises(ValueError, match="x_mask covers 4 frames"):
        FootGrounding([0, 3], mean, std)(x, t, x_mask=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="describe 66 columns"):
        FootGrounding([0, 3], mean, std)(torch.zeros(2, 5, 67), t)
    with pytest.raises(ValueError, match=r"keeps \(3 K \+ 1\) \* L floats in LDS"):
        FootGrounding(list(range(0, 48, 3)), mean, std)(torch.zeros(1, 400, 66), t[:1])
    with pytest.raises(ffi.AfmError):                           # callables over HIP: the CPU has no path
        FootGrounding([0, 3], mean, std)(x, t)
    with pytest.raises(ffi.AfmError):
        FootGrounding([0, 3], mean, std).energy(x)
    d = _diffusion("ddim50")
    g = FootGrounding.h3d([7, 10], m263, s263, height=[0.05, 0.08], t_start=300, contact="labels")
    assert g.joints == [7, 10] and g.K == 2 and g.height == [0.05, 0.08] and g.first_guided(d) == sum(t >= 300 for t in d.timestep_map) == 35
    plain = FootGrounding([0, 3], mean, std, height=1)
    assert plain.height == [1.0, 1.0] and plain.first_guided(d) == 0 and (plain.floor, plain.up, plain.contact) == (0.0, 2, "height")
    assert (plain.floor_weight, plain.skate_weight) == (1.0, 1.0)
    # the sum: every existing positional call unchanged, the grounding the fourth term; terms that disagree
    tw = dict(target=torch.zeros(2, 5, 2, 3), weight=torch.ones(2, 5, 2))
    contact, targets, clear = ContactGuidance([0, 3], mean, std), JointTargets([0, 3], mean, std, **tw), SceneClearance([6], mean, std, radius=0.5)
    four = MotionGuidance(contact, targets, clear, plain)
    assert (four.contact, four.targets, four.clearance, four.feet) == (contact, targets, clear, plain) and four.t_start is None
    assert MotionGuidance(contact, targets, clear).feet is None and MotionGuidance(feet=plain).clearance is None
    with pytest.raises(ValueError, match="at least one"):
        MotionGuidance()
    with pytest.raises(TypeError, match="feet must be a FootGrounding"):
        MotionGuidance(feet=clear)
    with pytest.raises(TypeError):
        MotionGuidance(contact, targets, plain)                 # the third place is the clearance's
    with pytest.raises(ValueError, match="different mean / std"):
        MotionGuidance(contact, feet=FootGrounding([0, 3], mean + 1, std))
    with pytest.raises(ValueError, match="HumanML3D features"):
        MotionGuidance(ContactGuidance([0, 3], m263, s263), feet=FootGrounding.h3d([7, 10], m263, s263))
    for a, b in ((None, ZUP), (ZUP, None), (ZUP, ZUP + 1)):
        with pytest.raises(ValueError, match="different to_scene"):
            MotionGuidance(clearance=SceneClearance.h3d([0, 10], m263, s263, radius=0.5, to_scene=a), feet=FootGrounding.h3d([7], m263, s263, to_scene=b))
    late = MotionGuidance(ContactGuidance([0, 3], mean, std, t_start=300), feet=FootGrounding([6], mean, std, t_start=700))
    assert late.first_guided(d) == sum(t >= 700 for t in d.timestep_map) == 15 and late.t_start == 700
    with pytest.raises(ValueError, match="feet_energy needs a grounding"):
        MotionGuidance(contact).feet_energy(x)
    assert MotionGuidance(feet=plain).energies(x) == (None, None)
    # stitched chains: out of scope, refused by name
    with pytest.raises(ValueError, match="LongGuidance: a FootGrounding is not evaluated on the joined long motion"):
        LongGuidance(Stitch(2, 1), clearance=plain)
    with pytest.raises(ValueError, match="FootGrounding"):
        LongGuidance(Stitch(2, 1), plain)
    assert "feet" not in inspect.signature(LongGuidance.__init__).parameters


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_exports_declared_structs_mirrored_and_the_abi_kept(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NEW | {"afm_foot_grounding", "afm_ground_guide"})
    assert int(re.search(r"#define AFM_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert [f for f, _ in ffi.FootGrounding._fields_] == ["mean", "std", "scale", "cols", "K", "up", "labels", "first_guided", "floor", "height",
                                                          "floor_weight", "skate_weight", "t_start", "h3d"]
    assert [f for f, _ in ffi.GroundGuide._fields_] == ["terms", "feet", "gk", "frame_mask"]
    assert [f for f, _ in ffi.SceneGuide._fields_] == ["terms", "clearance", "gk", "frame_mask"]          # untouched
    assert [f for f, _ in ffi.MotionGuide._fields_] == ["contact", "targets", "gk", "frame_mask"]
    # the loop entry: afm_cmdm_scene_guide_loop_range's list with the description swapped; afm_ground_guidance: one more energy
    assert ffi.EXPORTS["afm_cmdm_ground_guide_loop_range"][1][:15] == ffi.EXPORTS["afm_cmdm_scene_guide_loop_range"][1][:15]
    assert ffi.EXPORTS["afm_cmdm_ground_guide_loop_range"][1][16:] == ffi.EXPORTS["afm_cmdm_scene_guide_loop_range"][1][16:]
    assert ffi.EXPORTS["afm_cmdm_ground_guide_loop_range"][1][15] is ctypes.POINTER(ffi.GroundGuide)
    assert ffi.EXPORTS["afm_cmdm_ground_guide_loop_workspace_bytes"][1][:6] == ffi.EXPORTS["afm_cmdm_scene_guide_loop_workspace_bytes"][1][:6]
    a, s = ffi.EXPORTS["afm_ground_guidance"][1], ffi.EXPORTS["afm_scene_guidance"][1]
    assert a[0] is ctypes.POINTER(ffi.GroundGuide) and a[1:8] == s[1:8] and a[8] is ffi.c_f32p and a[9:] == s[8:]
    assert ffi.GROUND_LABEL_COL == LABEL_COL and ffi.GROUND_LABEL_SLOT == SLOT
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_foot_grounding", ffi.FootGrounding), ("afm_ground_guide", ffi.GroundGuide), ("afm_scene_clearance", ffi.SceneClearance),
             ("afm_scene_guide", ffi.SceneGuide), ("afm_motion_guide", ffi.MotionGuide), ("afm_h3d_layout", ffi.H3dLayout))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "grounding_layout.c", tmp_path / "grounding_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_the_library_reports_abi_version_7():
    assert ffi.load().afm_version() == 7


# ---------------------------------------------------------------------------------------------------------------- the call plan, routing
@pytest.mark.parametrize("impute", [False, True])
@pytest.mark.parametrize("guidance", ["none", "cfg", "cfg2"])
@pytest.mark.parametrize("update", ["ddpm", "ddim", "dpm"])
def test_the_ground_term_reaches_its_entry_in_every_form(update, guidance, impute):
    plan = plan_loop_call(update, guidance, impute, term="ground")
    assert plan.entry == "afm_cmdm_ground_guide_loop_range" and plan.sizer == "afm_cmdm_ground_guide_loop_workspace_bytes"
    assert len(plan.slots) + 4 + 8 == len(ffi.EXPORTS[plan.entry][1]) and len(plan.size_slots) + 4 == len(ffi.EXPORTS[plan.sizer][1])
    scene = plan_loop_call(update, guidance, impute, term="scene")
    assert plan.slots == scene.slots and plan.size_slots == scene.size_slots and plan.key != scene.key          # the same loop, the description swapped
    # every sum without a grounding plans the entry it plans today
    assert scene.entry == "afm_cmdm_scene_guide_loop_range" and scene.sizer == "afm_cmdm_scene_guide_loop_workspace_bytes"
    assert plan_loop_call(update, guidance, impute, term="motion").entry == "afm_cmdm_motion_guide_loop_range"
    assert plan_loop_call(update, guidance, impute, term="contact").entry == "afm_cmdm_guide_loop_range"
    assert "guide" not in plan_loop_call(update, guidance, impute).entry
    if update != "ddpm":
        assert plan_loop_call(update, guidance, impute, term="long", stitch=True).entry == "afm_cmdm_long_guide_loop_range"
        assert plan_loop_call(update, guidance, impute, term="long_scene", stitch=True).entry == "afm_cmdm_long_scene_guide_loop_range"
        with pytest.raises(ValueError, match="no stitched loop"):
            plan_loop_call(update, guidance, impute, term="ground", stitch=True)


def test_sample_loop_goes_native_with_a_grounding(monkeypatch):
    from afm import diffusion as dm
    from afm.pipeline import two_stage_sample
    assert inspect.signature(two_stage_sample).parameters["grounding"].default is None
    assert dm.FootGrounding is FootGrounding
    d = _diffusion("ddim5")
    mean, std = torch.zeros(66), torch.ones(66)
    shape, x = (2, 4, 66), torch.zeros(2, 4, 66)
    feet = FootGrounding([0, 3], mean, std)
    guides = (feet, MotionGuidance(feet=feet), MotionGuidance(ContactGuidance([0, 3], mean, std), feet=feet))
    stepped = []
    monkeypatch.setattr(dm.GaussianDiffusion, "_progressive", lambda self, *a, **k: stepped.append(a[0].__name__) or iter([{"sample": x}]))
    monkeypatch.setattr(dm.GaussianDiffusion, "dpm_solver_sample_loop_progressive",
                        lambda self, *a, **k: stepped.append("dpm") or iter([{"sample": x}]))
    loops = (("p_sample", lambda m, fn: d.p_sample_loop(m, shape, noise=x, cond_fn=fn, model_kwargs={})),
             ("ddim_sample", lambda m, fn: d.ddim_sample_loop(m, shape, noise=x, cond_fn=fn, model_kwargs={})),
             ("dpm", lambda m, fn: d.dpm_solver_sample_loop(m, shape, noise=x, cond_fn=fn, model_kwargs={})))
    for name, run in loops:
        for guide in guides:
            for cls in (_Names, _Bundle):                       # by name (GuidedCMDM) and in the private bundle (the plain CMDM)
                m = cls()
                run(m, guide)
                assert m.got is not None and m.got["contact_guide"] is guide and not stepped, (name, cls, type(guide))
            m = _NamesNot()
            run(m, guide)                                       # a loop that does not name the keyword: step by step through __call__
            assert m.got is None and stepped == [name], (name, type(guide))
            stepped.clear()
    with pytest.raises(ValueError, match="LongGuidance"):       # stitched chains take no grounding
        d.ddim_sample_loop(_Names(), (2, 4, 66), noise=torch.zeros(2, 4, 66), cond_fn=feet, model_kwargs={}, stitch=Stitch(2, 1))
