"""Scene clearance on the host (no GPU): the plain-torch restatement of SceneClearance's energy and gradient in both forms
(`clearance_reference`, `h3d_clearance_reference`; the GPU tests import them with the fixtures) against autograd of the float64 energy; how
many joint-frames of the fixtures have an obstacle inside their radius; the Python refusals; the C surface; the loop call plan; and the
effect on the energy, in float64 with the identity denoiser."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from afm import ffi, synth
from afm.cmdm import plan_loop_call
from afm.diffusion import ContactGuidance, JointTargets, MotionGuidance, SceneClearance
from conftest import ROOT

from test_guidance_host import _Bundle, _Names, _NamesNot, _diffusion, guide_case
from test_h3d_guidance_host import ZUP, h3d_case, h3d_joints_ref
from test_joint_targets_host import CONTACT_GUIDE_FIELDS, effect_inputs, h3d_adjoint_ref, linear_ddim5

NEW = {"afm_scene_guidance", "afm_scene_guidance_workspace_bytes", "afm_cmdm_scene_guide_loop_range", "afm_cmdm_scene_guide_loop_workspace_bytes"}
RADIUS = 0.5
H3D_CASE = (7, 130, 6, 263, "small", "per_sample")          # the h3d contact fixture of tests/test_h3d_guidance_host.py
H3D_RADII = (0.25, 0.5, 1.0, 2.0)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def obstacle_weight(q, weight=None, up=2, min_height=None, c=None, exempt_contact=None):
    """w [B, N] float64 of the issue's rule: weight (1 where None), 0 below min_height, 0 where the contact map's largest value reaches
    exempt_contact.  The comparisons are exact: the float32 values as doubles against the Python floats."""
    w = torch.ones(q.shape[:2], dtype=torch.float64) if weight is None else weight.double().clone()
    if min_height is not None:
        w[q[..., up].double() < float(min_height)] = 0.0
    if exempt_contact is not None:
        w[c.double().max(-1).values >= float(exempt_contact)] = 0.0
    return w


def _radii(radius, K):
    return [float(radius)] * K if not hasattr(radius, "__len__") else [float(r) for r in radius]


def clearance_sums(p, q, w, radius, dtype):
    """(S [B, L, K, 3], e [B, L, K], u [B, L, K, N]) of the positions p [B, L, K, 3] in ``dtype``, operation by operation:
    d2 = (dx*dx + dy*dy) + dz*dz;  u = max(0, 1 - d2 * ir2);  wu = w * u;  S = sum_n wu * d;  e = sum_n wu * u.  ir2 = 1 / r^2 in float64,
    rounded once to float32 for the float32 restatement (the kernel's own constant)."""
    r = torch.tensor(_radii(radius, p.shape[2]), dtype=torch.float64)
    ir2 = 1.0 / (r * r)
    ir2 = ir2.float() if dtype == torch.float32 else ir2
    d = p.to(dtype)[:, :, :, None, :] - q.to(dtype)[:, None, None, :, :]          # [B, L, K, N, 3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    u = torch.clamp(1 - d2 * ir2.to(dtype)[None, None, :, None], min=0)
    wu = w.to(dtype)[:, None, None, :] * u
    return (wu[..., None] * d).sum(3), (wu * u).sum(3), u


def _coef(radius, K, dtype):
    r = torch.tensor(_radii(radius, K), dtype=torch.float64)
    c = 4.0 / (r * r)
    return c.float() if dtype == torch.float32 else c


def _pad(x, x_mask):
    return torch.zeros(x.shape[:2], dtype=torch.bool) if x_mask is None else x_mask


def clearance_reference(x, x_mask, q, cols, mean, std, scale, radius=RADIUS, weight=None, up=2, min_height=None, c=None, exempt_contact=None,
                        t=None, t_start=None, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D], E [B]) of the column form in ``dtype``, plain torch:
    p = x * std, + mean;  grad[b,f,cols[k]+a] = ((scale * coef_k) * std_a) * S_a;  E = sum over valid frames of e"""
    idx = torch.tensor([[col + a for a in range(3)] for col in cols])
    xs, mean, std = x.to(dtype), mean.to(dtype), std.to(dtype)
    p = xs[:, :, idx] * std[idx] + mean[idx]                    # [B, L, K, 3]
    S, e, _ = clearance_sums(p, q, obstacle_weight(q, weight, up, min_height, c, exempt_contact), radius, dtype)
    pad = _pad(x, x_mask)
    ks = scale.to(dtype).view(-1, 1, 1, 1) * _coef(radius, len(cols), dtype).to(dtype).view(1, 1, -1, 1)
    term = torch.where(pad[..., None, None], torch.zeros((), dtype=dtype), (ks * std[idx]) * S)
    grad = torch.zeros(x.shape, dtype=dtype)
    grad[:, :, idx] = term
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, torch.where(pad[..., None], torch.zeros((), dtype=dtype), e).sum((1, 2))


def h3d_clearance_reference(x, x_mask, q, joints, mean, std, scale, to_scene=None, radius=RADIUS, weight=None, up=2, min_height=None, c=None,
                            exempt_contact=None, t=None, t_start=None, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D], E [B]) of SceneClearance.h3d in ``dtype``: coef_k * S (zero in a padded frame) on the recovered positions,
    carried through the adjoint of the recovery with scale alone"""
    p = h3d_joints_ref(x, x_mask, mean, std, joints, to_scene, dtype)
    S, e, _ = clearance_sums(p, q, obstacle_weight(q, weight, up, min_height, c, exempt_contact), radius, dtype)
    pad = _pad(x, x_mask)
    S = torch.where(pad[..., None, None], torch.zeros((), dtype=dtype), _coef(radius, len(joints), dtype).to(dtype).view(1, 1, -1, 1) * S)
    du = h3d_adjoint_ref(S, x, x_mask, joints, mean, std, to_scene, dtype)
    grad = scale.to(dtype).view(-1, 1, 1) * std.to(dtype) * du
    grad = torch.where(pad[..., None], torch.zeros_like(grad), grad)
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, torch.where(pad[..., None], torch.zeros((), dtype=dtype), e).sum((1, 2))


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def clear_case(N, K, D, **options):
    """the contact fixture `guide_case(N, K, D)` as a clearance case: its x, x_mask, q, cols, mean, std, scale, and the options"""
    g = guide_case(N, K, D)
    case = {k: g[k] for k in ("x", "x_mask", "q", "cols", "mean", "std", "scale")}
    if "exempt_contact" in options:
        case["c"] = g["c"]
    return dict(case, **{"radius": RADIUS, **options})


def h3d_clear_case(**options):
    g = h3d_case(H3D_CASE)
    case = {k: g[k] for k in ("x", "x_mask", "q", "joints", "mean", "std", "scale", "to_scene")}
    if "exempt_contact" in options:
        case["c"] = g["c"]
    return dict(case, **options)


def coverage(case):
    """per sample with a valid frame: (the share of its valid joint-frames with an obstacle point inside the radius, how many have none),
    on the float64 restatement"""
    if "joints" in case:
        p = h3d_joints_ref(case["x"], case["x_mask"], case["mean"], case["std"], case["joints"], case["to_scene"], torch.float64)
    else:
        idx = torch.tensor([[col + a for a in range(3)] for col in case["cols"]])
        p = case["x"].double()[:, :, idx] * case["std"].double()[idx] + case["mean"].double()[idx]
    w = obstacle_weight(case["q"], case.get("weight"), case.get("up", 2), case.get("min_height"), case.get("c"), case.get("exempt_contact"))
    u = clearance_sums(p, case["q"], w, case.get("radius", RADIUS), torch.float64)[2]
    hit = ((u > 0) & (w[:, None, None, :] != 0)).any(-1)       # [B, L, K]
    out = {}
    for b in range(case["x"].shape[0]):
        valid = ~_pad(case["x"], case["x_mask"])[b]
        if valid.any():
            out[b] = (hit[b][valid].double().mean().item(), int((~hit[b][valid]).sum()))
    return out


def nontrivial(case):
    """the issue's condition: in each sample with a valid frame at least a quarter of the valid joint-frames have an obstacle point inside
    the radius and at least one has none"""
    cov = coverage(case)
    return bool(cov) and all(share >= 0.25 and none >= 1 for share, none in cov.values())


MIN_HEIGHT_1100 = 0.25            # removes enough of the 1100 points to leave joint-frames without an obstacle


def h3d_radius():
    """the smallest radius of H3D_RADII at which at least a quarter of the h3d fixture's valid joint-frames have an obstacle inside"""
    for r in H3D_RADII:
        if all(share >= 0.25 for share, _ in coverage(h3d_clear_case(radius=r)).values()):
            return r
    raise AssertionError("no radius of H3D_RADII reaches a quarter")


def test_the_fixtures_are_not_trivial():
    small, big = coverage(clear_case(130, 6, 66)), coverage(clear_case(1100, 3, 66))
    floor = coverage(clear_case(1100, 3, 66, min_height=MIN_HEIGHT_1100))
    r = h3d_radius()
    h3d = coverage(h3d_clear_case(radius=r))
    print(f"[clearance host] joint-frames with an obstacle inside the radius (share, count without): N=130 {small}, N=1100 {big}, "
          f"N=1100 min_height={MIN_HEIGHT_1100} {floor}, h3d radius {r} {h3d}")
    assert set(small) == set(big) == set(h3d) == {0, 1}          # sample 2 has no valid frame
    assert nontrivial(clear_case(130, 6, 66)) and nontrivial(clear_case(1100, 3, 66, min_height=MIN_HEIGHT_1100)) and nontrivial(h3d_clear_case(radius=r))
    assert all(share >= 0.9 for share, _ in big.values())


# ---------------------------------------------------------------------------------------------------------------- against autograd
OPTIONS = {"plain": {}, "weight": "weight", "min_height": dict(min_height=-0.5, up=1), "exempt": dict(exempt_contact=0.8),
           "radii": dict(radius=[0.3, 0.5, 0.8, 1.1, 0.45, 0.6])}


def case_options(name, N, K):
    """the options of a named variant for a scene of N points and K joints (`weight`: a third of the points weigh 0, the others 0.25 .. 2)"""
    if name == "weight":
        gen = torch.Generator().manual_seed(N + 7)
        w = 0.25 + 1.75 * torch.rand((3, N), generator=gen)
        w[torch.rand((3, N), generator=gen) < 0.33] = 0.0
        return dict(weight=w)
    o = dict(OPTIONS[name])
    if "radius" in o:
        o["radius"] = o["radius"][:K]
    return o


@pytest.mark.parametrize("name", list(OPTIONS))
@pytest.mark.parametrize("N,K,D", [(130, 6, 66), (1100, 3, 66)])
def test_column_form_gradient_equals_autograd_of_the_float64_energy(N, K, D, name):
    g = clear_case(N, K, D, **case_options(name, N, K))
    want, e = clearance_reference(**g)
    x = g["x"].double().requires_grad_(True)
    e_auto = clearance_reference(**{**g, "x": x})[1]
    (auto,) = torch.autograd.grad((e_auto * g["scale"].double()).sum(), x)
    err = (want + auto).abs().max().item()
    print(f"[clearance host] columns N={N} K={K} {name}: analytic vs autograd max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item()) and torch.equal(e, e_auto.detach())
    named = torch.zeros(D, dtype=torch.bool)
    for col in g["cols"]:
        named[col:col + 3] = True
    zero = lambda v: torch.equal(v, torch.zeros_like(v))
    assert zero(want[..., ~named]) and zero(want[2]) and zero(want[g["x_mask"]]) and e[2] == 0 and want[0].abs().max() > 0 and (e[:2] > 0).all()
    late = clearance_reference(**g, t=torch.tensor([500, 499, 0]), t_start=500)[0]
    assert zero(late[0]) and torch.equal(late[1:], want[1:])
    if name != "plain":                                          # the option acts
        assert not torch.equal(want, clearance_reference(**clear_case(N, K, D))[0])


@pytest.mark.parametrize("name", ["plain", "exempt", "radii"])
def test_h3d_form_gradient_equals_autograd_of_the_float64_energy(name):
    g = h3d_clear_case(**{"radius": h3d_radius(), **case_options(name, 130, 6)})
    want, e = h3d_clearance_reference(**g)
    x = g["x"].double().requires_grad_(True)
    e_auto = h3d_clearance_reference(**{**g, "x": x})[1]
    (auto,) = torch.autograd.grad((e_auto * g["scale"].double()).sum(), x)
    err = (want + auto).abs().max().item()
    print(f"[clearance host] h3d {name}: analytic vs autograd max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item())
    zero = lambda v: torch.equal(v, torch.zeros_like(v))
    assert zero(want[2]) and zero(want[g["x_mask"]]) and zero(want[..., 67:]) and e[2] == 0 and want[0].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals():
    mean, std = torch.zeros(66), torch.ones(66)
    m263, s263 = torch.zeros(263), torch.ones(263)
    for bad in (0.0, -1.0, [0.5, 0.0], float("inf")):
        with pytest.raises(ValueError, match="radius"):
            SceneClearance([0, 3], mean, std, radius=bad)
    with pytest.raises(ValueError, match="radius"):
        SceneClearance([0, 3], mean, std, radius=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="radius"):
        SceneClearance.h3d([0, 3], m263, s263, radius=-0.5)
    with pytest.raises(ValueError, match="guided joints"):
        SceneClearance(list(range(0, 51, 3)), mean, std, radius=0.5)          # K = 17
    with pytest.raises(ValueError, match="overlaps"):
        SceneClearance([0, 2], mean, std, radius=0.5)
    with pytest.raises(ValueError, match="leaves the motion vector"):
        SceneClearance([0, 64], mean, std, radius=0.5)
    with pytest.raises(ValueError, match="up names"):
        SceneClearance([0, 3], mean, std, radius=0.5, up=3)
    with pytest.raises(ValueError, match="weight must be"):
        SceneClearance([0, 3], mean, std, radius=0.5, weight=torch.ones(2, 9, 1))
    with pytest.raises(ValueError, match="named twice"):
        SceneClearance.h3d([3, 3], m263, s263, radius=0.5)
    x, t = torch.zeros(2, 5, 66), torch.zeros(2, dtype=torch.int64)
    q = torch.zeros(2, 9, 3)
    with pytest.raises(ValueError, match="c_pc_xyz"):
        SceneClearance([0, 3], mean, std, radius=0.5)(x, t)
    with pytest.raises(ValueError, match="c_pc_xyz"):
        SceneClearance([0, 3], mean, std, radius=0.5)(x, t, c_pc_xyz=torch.zeros(2, 9, 2))
    with pytest.raises(ValueError, match="exempt_contact reads c_pc_contact"):          # an exemption without a map
        SceneClearance([0, 3], mean, std, radius=0.5, exempt_contact=0.5)(x, t, c_pc_xyz=q)
    with pytest.raises(ValueError, match="exempt_contact reads c_pc_contact"):
        SceneClearance([0, 3], mean, std, radius=0.5, exempt_contact=0.5).energy(x, c_pc_xyz=q)
    with pytest.raises(ValueError, match="c_pc_contact must be"):
        SceneClearance([0, 3], mean, std, radius=0.5, exempt_contact=0.5)(x, t, c_pc_xyz=q, c_pc_contact=torch.zeros(2, 8, 6))
    with pytest.raises(ValueError, match="the scene needs"):
        SceneClearance([0, 3], mean, std, radius=0.5, weight=torch.ones(2, 8))(x, t, c_pc_xyz=q)
    with pytest.raises(ValueError, match="holds 3 values for a batch of 2"):
        SceneClearance([0, 3], mean, std, radius=0.5, scale=torch.ones(3))(x, t, c_pc_xyz=q)
    with pytest.raises(ValueError, match="x_mask covers 4 frames"):
        SceneClearance([0, 3], mean, std, radius=0.5)(x, t, c_pc_xyz=q, x_mask=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ffi.AfmError):                           # callables over HIP: the CPU has no path
        SceneClearance([0, 3], mean, std, radius=0.5)(x, t, c_pc_xyz=q)
    with pytest.raises(ffi.AfmError):                           # (no map is read without exempt_contact)
        SceneClearance([0, 3], mean, std, radius=0.5).energy(x, c_pc_xyz=q)
    d = _diffusion("ddim50")
    g = SceneClearance.h3d([0, 10], m263, s263, radius=[0.5, 0.25], t_start=300)
    assert g.joints == [0, 10] and g.K == 2 and g.radius == [0.5, 0.25] and g.first_guided(d) == sum(t >= 300 for t in d.timestep_map) == 35
    assert SceneClearance([0, 3], mean, std, radius=1).radius == [1.0, 1.0] and SceneClearance([0, 3], mean, std, radius=1).first_guided(d) == 0
    # the sum: terms that disagree
    tw = dict(target=torch.zeros(2, 5, 2, 3), weight=torch.ones(2, 5, 2))
    contact, targets = ContactGuidance([0, 3], mean, std), JointTargets([0, 3], mean, std, **tw)
    with pytest.raises(ValueError, match="at least one"):
        MotionGuidance()
    with pytest.raises(TypeError):
        MotionGuidance(clearance=contact)
    with pytest.raises(TypeError):
        MotionGuidance(contact, SceneClearance([0, 3], mean, std, radius=0.5))          # the second place is the targets'
    with pytest.raises(ValueError, match="different mean / std"):
        MotionGuidance(contact, clearance=SceneClearance([0, 3], mean + 1, std, radius=0.5))
    with pytest.raises(ValueError, match="different mean / std"):
        MotionGuidance(targets=targets, clearance=SceneClearance([0, 3], m263, s263, radius=0.5))
    with pytest.raises(ValueError, match="HumanML3D features"):
        MotionGuidance(ContactGuidance([0, 3], m263, s263), clearance=SceneClearance.h3d([0, 10], m263, s263, radius=0.5))
    with pytest.raises(ValueError, match="HumanML3D features"):
        MotionGuidance(ContactGuidance.h3d([0, 3], m263, s263), None, SceneClearance([0, 3], m263, s263, radius=0.5))
    for a, b in ((None, ZUP), (ZUP, None), (ZUP, ZUP + 1), (ZUP, ZUP.repeat(2, 1, 1))):
        with pytest.raises(ValueError, match="different to_scene"):
            MotionGuidance(ContactGuidance.h3d([0, 3], m263, s263, to_scene=a), clearance=SceneClearance.h3d([0, 10], m263, s263, radius=0.5, to_scene=b))
    three = MotionGuidance(ContactGuidance([0, 3], mean, std, t_start=300), JointTargets([0, 3], mean, std, t_start=500, **tw),
                           SceneClearance([6], mean, std, radius=0.5, t_start=700))
    assert three.first_guided(d) == sum(t >= 700 for t in d.timestep_map) == 15 and three.t_start == 700
    assert MotionGuidance(contact, targets, SceneClearance([6], mean, std, radius=0.5)).t_start is None
    assert MotionGuidance(contact, targets).clearance is None and MotionGuidance(clearance=three.clearance).contact is None


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_exports_declared_structs_mirrored_and_the_abi_kept(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert int(re.search(r"#define AFM_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert [f for f, _ in ffi.ContactGuide._fields_] == CONTACT_GUIDE_FIELDS          # untouched
    assert [f for f, _ in ffi.JointTargets._fields_] == ["target", "weight", "scale", "mean", "std", "cols", "K", "first_guided", "t_start", "h3d"]
    assert [f for f, _ in ffi.MotionGuide._fields_] == ["contact", "targets", "gk", "frame_mask"]
    assert [f for f, _ in ffi.SceneGuide._fields_] == ["terms", "clearance", "gk", "frame_mask"]
    assert ffi.EXPORTS["afm_cmdm_scene_guide_loop_range"][1][:15] == ffi.EXPORTS["afm_cmdm_motion_guide_loop_range"][1][:15]
    assert ffi.EXPORTS["afm_cmdm_scene_guide_loop_range"][1][16:] == ffi.EXPORTS["afm_cmdm_motion_guide_loop_range"][1][16:]
    assert ffi.CLEAR_WAVES == int(re.search(r"#define AFM_CLEAR_WAVES (\d+)", hdr).group(1))
    assert ffi.CLEAR_TILE == int(re.search(r"#define AFM_CLEAR_TILE (\d+)", hdr).group(1)) and ffi.CLEAR_TILE % ffi.CLEAR_WAVES == 0
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_scene_clearance", ffi.SceneClearance), ("afm_scene_guide", ffi.SceneGuide), ("afm_joint_targets", ffi.JointTargets),
             ("afm_motion_guide", ffi.MotionGuide), ("afm_contact_guide", ffi.ContactGuide), ("afm_h3d_layout", ffi.H3dLayout))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "clearance_layout.c", tmp_path / "clearance_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


# ---------------------------------------------------------------------------------------------------------------- the call plan, routing
@pytest.mark.parametrize("impute", [False, True])
@pytest.mark.parametrize("guidance", ["none", "cfg", "cfg2"])
@pytest.mark.parametrize("update", ["ddpm", "ddim", "dpm"])
def test_the_scene_term_reaches_its_entry_in_every_form(update, guidance, impute):
    plan = plan_loop_call(update, guidance, impute, term="scene")
    assert plan.entry == "afm_cmdm_scene_guide_loop_range" and plan.sizer == "afm_cmdm_scene_guide_loop_workspace_bytes"
    assert len(plan.slots) + 4 + 8 == len(ffi.EXPORTS[plan.entry][1]) and len(plan.size_slots) + 4 == len(ffi.EXPORTS[plan.sizer][1])
    motion = plan_loop_call(update, guidance, impute, term="motion")
    assert plan.slots == motion.slots and plan.size_slots == motion.size_slots and plan.key != motion.key          # the same loop, the description swapped
    assert motion.entry == "afm_cmdm_motion_guide_loop_range"
    assert plan_loop_call(update, guidance, impute, term="contact").entry == "afm_cmdm_guide_loop_range"
    assert "guide" not in plan_loop_call(update, guidance, impute).entry
    if update != "ddpm":
        assert plan_loop_call(update, guidance, impute, term="long", stitch=True).entry == "afm_cmdm_long_guide_loop_range"
        with pytest.raises(ValueError, match="no stitched loop"):
            plan_loop_call(update, guidance, impute, term="scene", stitch=True)


def test_sample_loop_goes_native_with_a_clearance(monkeypatch):
    from afm import diffusion as dm
    from afm.pipeline import two_stage_sample
    assert inspect.signature(two_stage_sample).parameters["clearance"].default is None
    assert dm.SceneClearance is SceneClearance
    d = _diffusion("ddim5")
    mean, std = torch.zeros(66), torch.ones(66)
    shape, x = (2, 4, 66), torch.zeros(2, 4, 66)
    clear = SceneClearance([0, 3], mean, std, radius=0.5)
    guides = (clear, MotionGuidance(clearance=clear), MotionGuidance(ContactGuidance([0, 3], mean, std), clearance=clear))
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
    from afm.guidance import Stitch
    with pytest.raises(ValueError, match="LongGuidance"):       # stitched chains stay as they are
        d.ddim_sample_loop(_Names(), (2, 4, 66), noise=torch.zeros(2, 4, 66), cond_fn=clear, model_kwargs={}, stitch=Stitch(2, 1))


# ---------------------------------------------------------------------------------------------------------------- the effect
EFFECT_RADIUS, EFFECT_SCALE = 0.75, 0.02


def effect_scene():
    """the effect inputs of tests/test_joint_targets_host.py with a scene for them: 96 obstacle points scattered around the guided joints'
    positions of the start motion (samples 0 and 1; sample 2's points lie far away - its unguided E is 0)"""
    g = effect_inputs()
    idx = torch.tensor([[c + a for a in range(3)] for c in g["cols"]])
    p = g["start"][:, :, idx] * g["std"][idx] + g["mean"][idx]          # [3, 16, 2, 3]
    q = p.reshape(3, -1, 3).repeat(1, 3, 1) + 0.4 * synth.gaussian("clear_effect_q", (3, 96, 3))
    q[2] += 50.0
    return dict(g, q=q)


def _chain64(g, scale):
    """the eta = 0 DDIM chain with the identity denoiser in float64: x0 = x_t, x0' = x0 + gk * grad(x_t) below t_start"""
    x = g["start"].double()
    for t, a, ap in linear_ddim5():
        x0 = x
        if scale is not None and t < g["t_start"]:
            grad, _ = clearance_reference(x, None, g["q"], g["cols"], g["mean"], g["std"], torch.full((x.shape[0],), float(scale)), EFFECT_RADIUS)
            x0 = x0 + (1 - a) / a ** 0.5 * grad
        eps = ((1 / a) ** 0.5 * x - x0) / (1 / a - 1) ** 0.5
        x = ap ** 0.5 * x0 + (1 - ap) ** 0.5 * eps
    return x


def test_the_guided_float64_chain_ends_below_the_unguided_chain():
    g = effect_scene()
    energy = lambda x: clearance_reference(x, None, g["q"], g["cols"], g["mean"], g["std"], torch.ones(3), EFFECT_RADIUS)[1]
    e_plain, e_guided = energy(_chain64(g, None)), energy(_chain64(g, EFFECT_SCALE))
    print(f"[clearance effect host] energy at the start {energy(g['start'].double()).tolist()}, unguided {e_plain.tolist()}, "
          f"scale {EFFECT_SCALE} {e_guided.tolist()}")
    assert (e_plain[:2] > 0).all() and e_plain[2] == 0 and e_guided[2] == 0
    assert (e_guided[:2] < e_plain[:2]).all()
