"""Joint-position targets on the host (no GPU): the plain-torch restatement of JointTargets' energy and gradient in both forms
(`targets_reference`, `h3d_targets_reference`; the GPU tests import them with the fixtures) against autograd of the float64 energy; the
exact zeros; the root's path into the velocity columns; the C surface; the Python refusals; the routing of `_sample_loop`; and the effect
on the energy, in float64 with the identity denoiser."""
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
from afm.diffusion import ContactGuidance, JointTargets, MotionGuidance, _takes
from conftest import ROOT

from test_guidance_host import SCATTERED, _Bundle, _Names, _NamesNot, _diffusion
from test_h3d_guidance_host import ZUP, _prev, _recover, _scan, _to_scene, h3d_joints_ref

NEW = {"afm_motion_guidance", "afm_motion_guidance_workspace_bytes", "afm_cmdm_motion_guide_loop_range",
       "afm_cmdm_motion_guide_loop_workspace_bytes"}
B = 3                             # sample 1: an interior padded frame and (L >= 4) padded trailing frames; sample 2: every frame padded
CONTACT_GUIDE_FIELDS = ["q", "c", "mean", "std", "scale", "gk", "frame_mask", "cols", "K", "N", "sigma", "first_guided", "t_start", "h3d"]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _valid(x_mask, weight):
    pad = torch.zeros(weight.shape[:2], dtype=torch.bool) if x_mask is None else x_mask
    return ~pad[..., None] & (weight != 0)


def _energy(p, target, weight, valid, dtype):
    """E[b] = sum over valid (f, k) of w * ((dx*dx + dy*dy) + dz*dz), d = p - target; a target without weight is never used"""
    g = torch.where(valid[..., None], target.to(dtype), torch.zeros((), dtype=dtype))
    d = p - g
    e = weight.to(dtype) * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return torch.where(valid, e, torch.zeros((), dtype=dtype)).sum((1, 2))


def _S(p, target, weight, valid, dtype):
    """w * (target - p), zero where w == 0 or the frame is padded (the target there may be NaN)"""
    g = torch.where(valid[..., None], target.to(dtype), p)
    return torch.where(valid[..., None], weight.to(dtype)[..., None] * (g - p), torch.zeros((), dtype=dtype))


def targets_reference(x, x_mask, cols, mean, std, target, weight, scale, t=None, t_start=None, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D], E [B]) of the column form in ``dtype``, plain torch, the issue's expression operation by operation:
    p = x * std, + mean;  d = target - p;  m = w * d;  grad = ((scale * 2) * std) * m"""
    idx = torch.tensor([[col + a for a in range(3)] for col in cols])
    xs, mean, std = x.to(dtype), mean.to(dtype), std.to(dtype)
    p = xs[:, :, idx] * std[idx] + mean[idx]                    # [B, L, K, 3]
    valid = _valid(x_mask, weight)
    m = _S(p, target, weight, valid, dtype)
    ks = scale.to(dtype).view(-1, 1, 1, 1) * 2
    grad = torch.zeros(x.shape, dtype=dtype)
    grad[:, :, idx] = (ks * std[idx]) * m
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, _energy(p, target, weight, valid, dtype)


def h3d_adjoint_ref(S, x, x_mask, joints, mean, std, to_scene, dtype):
    """S [B, L, K, 3] (d/dp of something, per guided joint) carried back to the features u: the adjoint of h3d_joints_ref, the six scans of
    tests/test_h3d_guidance_host.py::h3d_contact_reference in the same order -> du [B, L, D]"""
    Bn, L, D = x.shape
    u, cc, ss, _, _, vx, vz = _recover(x, x_mask, mean, std, dtype)
    A = _to_scene(to_scene, Bn, dtype)
    du = torch.zeros(Bn, L, D, dtype=dtype)
    gX, gZ, T = (torch.zeros(Bn, L, dtype=dtype) for _ in range(3))
    for k, j in enumerate(joints):
        Gx, Gy, Gz = (((A[:, 0, a, None] * S[:, :, k, 0] + A[:, 1, a, None] * S[:, :, k, 1]) + A[:, 2, a, None] * S[:, :, k, 2]) for a in range(3))
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
    return du


def h3d_targets_reference(x, x_mask, joints, mean, std, target, weight, scale, to_scene=None, t=None, t_start=None, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D], E [B]) of JointTargets.h3d in ``dtype``: S = w * (target - p) on the recovered positions, carried through
    the adjoint with coef = 2"""
    p = h3d_joints_ref(x, x_mask, mean, std, joints, to_scene, dtype)
    valid = _valid(x_mask, weight)
    du = h3d_adjoint_ref(_S(p, target, weight, valid, dtype), x, x_mask, joints, mean, std, to_scene, dtype)
    grad = (scale.to(dtype).view(-1, 1, 1) * 2) * std.to(dtype) * du
    if x_mask is not None:
        grad = torch.where(x_mask[..., None], torch.zeros_like(grad), grad)
    if t is not None and t_start is not None:
        grad[t >= t_start] = 0
    return grad, _energy(p, target, weight, valid, dtype)


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def case_mask(L):
    mask = torch.zeros(B, L, dtype=torch.bool)
    if L >= 3:
        mask[1, 1] = True                                       # interior
    if L >= 4:
        mask[1, L - 2:] = True
    mask[2, :] = True
    return mask


def _plant(tag, target, weight):
    """weights in (0.5, 1.5), a third of them exactly zero with NaN targets behind them (never read)"""
    Bn, L, K = weight.shape
    off = torch.rand((Bn, L, K), generator=torch.Generator().manual_seed(L * 100 + K)) < 1 / 3
    if L * K > 1:
        off[0, 0, 0] = False                                    # sample 0 keeps a target at the first frame
        off.view(Bn, -1)[:, -1] = False                         #   and every sample one at the last frame's last joint
        off[1, 0, 0] = True                                     # a zero weight in a valid frame, whatever the draw
        off[0, L - 1, 0] = K > 1                                # a zero weight in the last frame (one joint: its target there stays)
    else:
        off[:] = False                                          # one item: it keeps its target
    weight = torch.where(off, torch.zeros(()), weight)
    target = torch.where(off[..., None], torch.full((), float("nan")), target)
    return target, weight


def cols_case(L, K, D):
    """The inputs of one column-form case (CPU float32 tensors).  D = 66: the `pos` layout's columns 3 j; D = 263: scattered triples."""
    tag = f"targets_{L}_{K}_{D}"
    cols = [3 * j for j in range(K)] if D == 66 else (SCATTERED + [20, 29, 38, 47, 56, 70, 79, 88, 110, 120])[:K]
    x = synth.gaussian(tag + "_x", (B, L, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    std[cols[0] + 1] = 0.0                                      # a zero entry: that coordinate is the mean, its gradient zero
    target, weight = _plant(tag, 1.5 * synth.gaussian(tag + "_g", (B, L, K, 3)), 0.5 + torch.rand((B, L, K), generator=torch.Generator().manual_seed(K)))
    return dict(x=x, x_mask=case_mask(L), cols=cols, mean=mean, std=std, target=target, weight=weight, scale=torch.tensor([1.0, 2.5, 0.5]))


H3D_JOINT_SETS = {"root": [0], "mixed": [0, 10, 11, 12, 20, 21], "limbs": [21, 7]}
# (L, joints, to_scene) of the h3d cases: L = 1, 2 the scans' edges, 70 crosses one wave of frames, 196 the workload's maximum, 300 the
# 256-stride loops; the root alone (the suffix scans and column 3 only), mixed joints, joints without the root; a per-sample to_scene
H3D_CASES = [(1, "mixed", None), (2, "root", "zup"), (7, "mixed", "per_sample"), (7, "root", None), (70, "mixed", "zup"), (70, "limbs", "per_sample"),
             (196, "root", "per_sample"), (196, "mixed", None), (300, "mixed", "zup")]


def h3d_case_id(case):
    return "L{}_{}_{}".format(*case)


def h3d_targets_case(case):
    L, which, scene = case
    tag = f"h3d_targets_{h3d_case_id(case)}"
    joints, D = H3D_JOINT_SETS[which], 263
    K = len(joints)
    x = synth.gaussian(tag + "_x", (B, L, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    mean[0:3] = 0.0
    std[0], std[1:3] = 0.05, 0.1
    to_scene = None if scene is None else ZUP.clone() if scene == "zup" else torch.eye(3, 4).repeat(B, 1, 1) + 0.3 * synth.gaussian(tag + "_ts", (B, 3, 4))
    target, weight = _plant(tag, 1.5 * synth.gaussian(tag + "_g", (B, L, K, 3)), 0.5 + torch.rand((B, L, K), generator=torch.Generator().manual_seed(K)))
    return dict(x=x, x_mask=case_mask(L), joints=joints, mean=mean, std=std, target=target, weight=weight, scale=torch.tensor([1.0, 2.5, 0.5]),
                to_scene=to_scene)


# ---------------------------------------------------------------------------------------------------------------- against autograd
def _autograd(g, positions):
    x = g["x"].double().requires_grad_(True)
    p = positions(x)
    valid = _valid(g["x_mask"], g["weight"])
    energy = _energy(p, g["target"], g["weight"], valid, torch.float64)
    (auto,) = torch.autograd.grad((energy * g["scale"].double()).sum(), x)
    return auto, energy.detach()


@pytest.mark.parametrize("L,K,D", [(7, 2, 66), (7, 16, 263), (1, 1, 66)])
def test_column_form_gradient_equals_autograd_of_the_float64_energy(L, K, D):
    g = cols_case(L, K, D)
    want, e = targets_reference(**g)
    idx = torch.tensor([[col + a for a in range(3)] for col in g["cols"]])
    auto, e_auto = _autograd(g, lambda x: x[:, :, idx] * g["std"].double()[idx] + g["mean"].double()[idx])
    err = (want + auto).abs().max().item()
    print(f"[targets host] columns L={L} K={K} D={D}: analytic vs autograd max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item()) and (e - e_auto).abs().max().item() <= 1e-12 * max(1.0, e.abs().max().item())
    assert torch.isfinite(want).all() and torch.isfinite(e).all() and g["target"].isnan().any() == (L * K > 1)
    named = torch.zeros(D, dtype=torch.bool)
    named[idx.flatten()] = True
    zero = lambda v: torch.equal(v, torch.zeros_like(v))
    assert zero(want[..., ~named]) and zero(want[2]) and zero(want[g["x_mask"]]) and zero(want[..., g["cols"][0] + 1]) and e[2] == 0
    off = (g["weight"] == 0)[..., None].expand(-1, -1, -1, 3)
    assert zero(want[:, :, idx][off]) and (L * K == 1 or want[0].abs().max() > 0)
    late = targets_reference(**g, t=torch.tensor([500, 499, 0]), t_start=500)[0]
    assert zero(late[0]) and torch.equal(late[1:], want[1:])


@pytest.mark.parametrize("case", [H3D_CASES[0], H3D_CASES[1], H3D_CASES[2], H3D_CASES[3], H3D_CASES[5]], ids=h3d_case_id)
def test_h3d_form_gradient_equals_autograd_of_the_float64_energy(case):
    g = h3d_targets_case(case)
    want, e = h3d_targets_reference(**g)
    auto, e_auto = _autograd(g, lambda x: h3d_joints_ref(x, g["x_mask"], g["mean"], g["std"], g["joints"], g["to_scene"], torch.float64))
    err = (want + auto).abs().max().item()
    print(f"[targets host] h3d {h3d_case_id(case)}: analytic vs autograd max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item()) and (e - e_auto).abs().max().item() <= 1e-12 * max(1.0, e.abs().max().item())
    zero = lambda v: torch.equal(v, torch.zeros_like(v))
    assert zero(want[2]) and zero(want[g["x_mask"]]) and zero(want[..., 67:]) and e[2] == 0
    if g["x_mask"][1].any():                                    # the interior padded frame: zero row, its neighbours not
        assert zero(want[1, 1]) and want[1, 0].abs().max() > 0


def test_a_zero_weight_and_an_interior_padded_frame_give_exact_zeros():
    g = h3d_targets_case(H3D_CASES[2])
    g["weight"][0, 3, :] = 0.0
    g["target"][0, 3] = float("nan")
    want, e = h3d_targets_reference(**g)
    assert torch.isfinite(want).all() and torch.isfinite(e).all()
    local = [c for j in g["joints"] if j for c in range(4 + 3 * (j - 1), 7 + 3 * (j - 1))] + [3]
    assert torch.equal(want[0, 3, local], torch.zeros(len(local), dtype=torch.float64))          # no term in the frame's own columns
    assert want[0, 3, :3].abs().min() > 0                       # but later frames' targets still reach its velocities
    assert g["x_mask"][1, 1] and torch.equal(want[1, 1], torch.zeros(263, dtype=torch.float64))


def test_a_root_target_at_the_last_frame_reaches_the_velocities_of_every_earlier_frame():
    L = 7
    g = h3d_targets_case((L, "root", None))
    g["x_mask"] = torch.zeros(B, L, dtype=torch.bool)
    g["weight"] = torch.zeros(B, L, 1)
    g["weight"][:, L - 1, 0] = 1.0
    g["target"] = torch.full((B, L, 1, 3), float("nan"))
    g["target"][:, L - 1, 0] = torch.tensor([1.0, 0.5, -2.0])
    want, _ = h3d_targets_reference(**g)
    assert (want[:, :L - 1, 1:3] != 0).all() and (want[:, :L - 1, 0] != 0).all()          # planar velocities and the rotation, every earlier frame
    assert torch.equal(want[:, L - 1, :3], torch.zeros(B, 3, dtype=torch.float64))       # the last frame's velocities move nothing
    assert (want[:, L - 1, 3] != 0).all() and torch.equal(want[:, :L - 1, 3], torch.zeros(B, L - 1, dtype=torch.float64))
    assert torch.equal(want[..., 4:], torch.zeros(B, L, 259, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_exports_declared_structs_mirrored_and_the_abi_kept(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert int(re.search(r"#define AFM_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert [f for f, _ in ffi.ContactGuide._fields_] == CONTACT_GUIDE_FIELDS          # untouched
    assert [f for f, _ in ffi.H3dLayout._fields_] == ["joints", "to_scene", "to_scene_stride"]
    assert {"target", "weight", "scale", "mean", "std", "cols", "K", "t_start", "first_guided", "h3d"} == {f for f, _ in ffi.JointTargets._fields_}
    assert [f for f, _ in ffi.MotionGuide._fields_] == ["contact", "targets", "gk", "frame_mask"]
    assert ffi.EXPORTS["afm_cmdm_motion_guide_loop_range"][1][:15] == ffi.EXPORTS["afm_cmdm_guide_loop_range"][1][:15]
    assert ffi.EXPORTS["afm_cmdm_motion_guide_loop_range"][1][16:] == ffi.EXPORTS["afm_cmdm_guide_loop_range"][1][16:]
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_joint_targets", ffi.JointTargets), ("afm_motion_guide", ffi.MotionGuide), ("afm_contact_guide", ffi.ContactGuide),
             ("afm_h3d_layout", ffi.H3dLayout))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "targets_layout.c", tmp_path / "targets_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _tw(Bn=2, L=5, K=2):
    return dict(target=torch.zeros(Bn, L, K, 3), weight=torch.ones(Bn, L, K))


def test_python_refusals():
    mean, std = torch.zeros(66), torch.ones(66)
    m263, s263 = torch.zeros(263), torch.ones(263)
    with pytest.raises(ValueError, match="leaves the motion vector"):
        JointTargets([0, 64], mean, std, **_tw())
    with pytest.raises(ValueError, match="overlaps"):
        JointTargets([0, 2], mean, std, **_tw())
    with pytest.raises(ValueError, match="guided joints"):
        JointTargets(list(range(0, 51, 3)), mean, std, **_tw(K=17))
    with pytest.raises(ValueError, match="mean and std"):
        JointTargets([0, 3], mean, torch.ones(65), **_tw())
    for bad in (dict(target=torch.zeros(2, 5, 2), weight=torch.ones(2, 5, 2)), dict(target=torch.zeros(2, 5, 3, 3), weight=torch.ones(2, 5, 3)),
                dict(target=torch.zeros(2, 5, 2, 3), weight=torch.ones(2, 5)), dict(target=torch.zeros(2, 5, 2, 3), weight=torch.ones(2, 4, 2)),
                dict(target=torch.zeros(2, 5, 2, 3, dtype=torch.int64), weight=torch.ones(2, 5, 2)), dict(target=None, weight=torch.ones(2, 5, 2))):
        with pytest.raises(ValueError, match="target must be"):
            JointTargets([0, 3], mean, std, **bad)
        with pytest.raises(ValueError, match="target must be"):
            JointTargets.h3d([0, 10], m263, s263, **bad)
    with pytest.raises(ValueError, match="float or a floating"):
        JointTargets([0, 3], mean, std, scale=torch.ones(2, 2), **_tw())
    with pytest.raises(ValueError, match="outside 0..21"):
        JointTargets.h3d([0, 22], m263, s263, **_tw())
    with pytest.raises(ValueError, match="named twice"):
        JointTargets.h3d([3, 3], m263, s263, **_tw())
    with pytest.raises(ValueError, match="columns 0..66"):
        JointTargets.h3d([0, 1], mean, std, **_tw())
    with pytest.raises(ValueError, match="to_scene must be a float32"):
        JointTargets.h3d([0, 1], m263, s263, to_scene=torch.zeros(4, 3), **_tw())
    # against a sample: another batch, L or K; the scale; the columns; the x_mask
    x, t = torch.zeros(2, 5, 66), torch.zeros(2, dtype=torch.int64)
    for other in (_tw(Bn=3), _tw(L=4)):
        with pytest.raises(ValueError, match="the sample needs"):
            JointTargets([0, 3], mean, std, **other)(x, t)
        with pytest.raises(ValueError, match="the sample needs"):
            JointTargets([0, 3], mean, std, **other).energy(x)
        with pytest.raises(ValueError, match="the sample needs"):
            JointTargets.h3d([0, 10], m263, s263, **other)(torch.zeros(2, 5, 263), t)
    with pytest.raises(ValueError, match="the sample is"):
        JointTargets([0, 3], mean, std, **_tw())(torch.zeros(2, 5, 69), t)
    with pytest.raises(ValueError, match="holds 3 values for a batch of 2"):
        JointTargets([0, 3], mean, std, scale=torch.ones(3), **_tw())(x, t)
    with pytest.raises(ValueError, match="x_mask covers 4 frames"):
        JointTargets([0, 3], mean, std, **_tw())(x, t, x_mask=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="3 matrices for a batch of 2"):
        JointTargets.h3d([0, 10], m263, s263, to_scene=torch.zeros(3, 3, 4), **_tw())(torch.zeros(2, 5, 263), t)
    with pytest.raises(ffi.AfmError):                           # callables over HIP: the CPU has no path
        JointTargets([0, 3], mean, std, **_tw())(x, t)
    with pytest.raises(ffi.AfmError):
        JointTargets.h3d([0, 10], m263, s263, **_tw()).energy(torch.zeros(2, 5, 263))
    g = JointTargets.h3d([0, 10], m263, s263, t_start=300, **_tw())
    d = _diffusion("ddim50")
    assert g.joints == [0, 10] and g.K == 2 and g.first_guided(d) == sum(t >= 300 for t in d.timestep_map) == 35
    assert JointTargets([0, 3], mean, std, **_tw()).joints is None and JointTargets([0, 3], mean, std, **_tw()).first_guided(d) == 0
    # the sum: terms that disagree
    contact = ContactGuidance([0, 3], mean, std)
    with pytest.raises(ValueError, match="at least one"):
        MotionGuidance()
    with pytest.raises(TypeError):
        MotionGuidance(JointTargets([0, 3], mean, std, **_tw()))          # the first place is the contact term's
    with pytest.raises(TypeError):
        MotionGuidance(contact, contact)
    with pytest.raises(ValueError, match="different mean / std"):
        MotionGuidance(contact, JointTargets([0, 3], mean + 1, std, **_tw()))
    with pytest.raises(ValueError, match="different mean / std"):
        MotionGuidance(ContactGuidance([0, 3], m263, s263), JointTargets([0, 3], mean, std, **_tw()))
    with pytest.raises(ValueError, match="HumanML3D features"):
        MotionGuidance(ContactGuidance([0, 3], m263, s263), JointTargets.h3d([0, 10], m263, s263, **_tw()))
    with pytest.raises(ValueError, match="HumanML3D features"):
        MotionGuidance(ContactGuidance.h3d([0, 3], m263, s263), JointTargets([0, 3], m263, s263, **_tw()))
    for a, b in ((None, ZUP), (ZUP, None), (ZUP, ZUP + 1), (ZUP, ZUP.repeat(2, 1, 1))):
        with pytest.raises(ValueError, match="different to_scene"):
            MotionGuidance(ContactGuidance.h3d([0, 3], m263, s263, to_scene=a), JointTargets.h3d([0, 10], m263, s263, to_scene=b, **_tw()))
    both = MotionGuidance(ContactGuidance.h3d([0, 3], m263, s263, to_scene=ZUP, t_start=300), JointTargets.h3d([5], m263, s263, to_scene=ZUP.clone(), t_start=500, **_tw(K=1)))
    assert both.first_guided(d) == sum(t >= 500 for t in d.timestep_map) == 25 and both.t_start == 500
    assert MotionGuidance(contact, JointTargets([0, 3], mean, std, **_tw())).t_start is None


# ---------------------------------------------------------------------------------------------------------------- routing
def test_sample_loop_goes_native_for_all_three_classes(monkeypatch):
    from afm import diffusion as dm
    from afm.pipeline import two_stage_sample
    assert inspect.signature(two_stage_sample).parameters["joint_targets"].default is None
    d = _diffusion("ddim5")
    mean, std = torch.zeros(66), torch.ones(66)
    shape, x = (2, 4, 66), torch.zeros(2, 4, 66)
    contact, targets = ContactGuidance([0, 3], mean, std), JointTargets([0, 3], mean, std, **_tw(L=4))
    guides = (contact, targets, MotionGuidance(contact, targets), MotionGuidance(targets=targets), MotionGuidance(contact))
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


# ---------------------------------------------------------------------------------------------------------------- the effect
def effect_inputs():
    """The column-form inputs of the effect tests (CPU float32): B = 3, L = 16, K = 2 on D = 66, weights in {0, 1}, std up to about 2.8."""
    Bn, L, K, D = 3, 16, 2, 66
    cols = [0, 30]
    mean, std = 0.3 * synth.gaussian("targets_effect_mean", (D,)), 0.5 + synth.gaussian("targets_effect_std", (D,)).abs()
    known = 0.5 * synth.gaussian("targets_effect_motion", (Bn, L, D))
    idx = torch.tensor([[c + a for a in range(3)] for c in cols])
    target = known[:, :, idx] * std[idx] + mean[idx]
    weight = (torch.rand((Bn, L, K), generator=torch.Generator().manual_seed(11)) < 0.5).float()
    weight[:, L - 1] = 1.0                                      # every sample has targets
    start = known + 0.5 * synth.gaussian("targets_effect_noise", (Bn, L, D))
    return dict(cols=cols, mean=mean, std=std, target=target, weight=weight, start=start, t_start=601)


def linear_ddim5():
    """(timesteps high to low, abar, abar_prev) of the 5-step spaced process on 1000 linear betas, float64"""
    abar = np.cumprod(1.0 - np.linspace(1e-4, 0.02, 1000, dtype=np.float64))
    ts = list(range(0, 1000, 200))[::-1]
    return [(t, abar[t], abar[t - 200] if t >= 200 else 1.0) for t in ts]


def _chain64(g, scale):
    """the eta = 0 DDIM chain with the identity denoiser in float64: x0 = x_t, x0' = x0 + gk * grad(x_t) below t_start"""
    x = g["start"].double()
    for t, a, ap in linear_ddim5():
        x0 = x
        if scale is not None and t < g["t_start"]:
            grad, _ = targets_reference(x, None, g["cols"], g["mean"], g["std"], g["target"], g["weight"], torch.full((x.shape[0],), float(scale)))
            x0 = x0 + (1 - a) / a ** 0.5 * grad
        eps = ((1 / a) ** 0.5 * x - x0) / (1 / a - 1) ** 0.5
        x = ap ** 0.5 * x0 + (1 - ap) ** 0.5 * eps
    return x


def test_the_guided_float64_chain_ends_far_below_the_unguided_chain():
    g = effect_inputs()
    assert 2.5 < g["std"].max().item() < 3.1 and set(g["weight"].unique().tolist()) == {0.0, 1.0}
    energy = lambda x: targets_reference(x, None, g["cols"], g["mean"], g["std"], g["target"], g["weight"], torch.ones(3))[1]
    e_plain, e_guided, e_big = energy(_chain64(g, None)), energy(_chain64(g, 0.1)), energy(_chain64(g, 1.0))
    print(f"[targets effect host] energy at the start {energy(g['start'].double()).tolist()}, unguided {e_plain.tolist()}, "
          f"scale 0.1 {e_guided.tolist()}, scale 1.0 {e_big.tolist()}")
    assert (e_guided < 0.1 * e_plain).all()
    # scale = 1 steps past 2 / curvature (the curvature of E along a guided column is 2 w std^2): the chain diverges
    assert (e_big > e_plain).all()
