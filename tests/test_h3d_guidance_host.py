"""Contact guidance and joint recovery for HumanML3D features on the host (no GPU): the plain-torch restatement of the recovery
(`h3d_joints_ref`) and of the energy and its gradient through the recovery (`h3d_contact_reference`; the GPU tests import both, with the
fixtures) against the reference's own recover_from_ric (tests/golden/h3d_recover_from_ric.npz, tools/make_h3d_golden.py) and against
autograd; the mask rule; the margin of the GPU fixtures' nearest-frame decisions; the C surface and the Python refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, ops, synth
from afm.diffusion import ContactGuidance
from conftest import ROOT, golden

from test_guidance_host import JOINTS, SIGMA, contact_reference, contact_terms

NEW = {"afm_h3d_joints", "afm_contact_guidance_h3d_workspace_bytes"}
B = 3                             # sample 1: trailing frames masked where L allows; sample 2: every frame masked
DUP = (0, 2, 4)                   # sample 0 (L >= 5): frame 4 repeats the pose of frame 2 bit for bit - the first index must win
ZUP = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]])          # y-up to z-up
# (L, N, K, D, rotation, to_scene) of the kernel cases.  L = 1, 2: the scans' edges; 70 crosses one wave of frames; 196 is the workload's
# maximum and ends in a partial wave; N = 1, 63, 130: the point loops' edges.  rotation "turns": a std of the rotation velocity that takes
# 2 th through several full turns; "small": realistic values.  D = 67: joint 21 alone, whose triple ends at the last column.
CASES = [(1, 63, 6, 263, "small", None), (2, 1, 1, 263, "small", "zup"), (7, 130, 6, 263, "small", "per_sample"),
         (70, 63, 6, 263, "turns", None), (196, 130, 6, 263, "small", "zup"), (196, 63, 1, 263, "small", None),
         (7, 63, 1, 67, "small", "zup")]
# The seed of every case is checked on the CPU: no nearest-frame decision is closer than a relative 1e-4 in float64 and float32 picks the
# same frames (test_fixture_margin asserts it), so no (n, k) pair has to be left out of a comparison.  Seed 0 meets the condition at every
# case as the fixtures stand; a case that stops meeting it gets another seed here, never a looser condition.
SEEDS = {}


def case_id(case):
    return "L{}_N{}_K{}_D{}_{}_{}".format(*case)


def case_joints(case):
    return [21] if case[3] == 67 else JOINTS[:case[2]]


def zero_column(joints):
    return 2 if joints[-1] == 0 else 4 + 3 * (joints[-1] - 1) + 1


def _scan(v, *, reverse=False, exclusive=False):
    """the running sum of v [B, L] over the frames, one rounded addition per frame in frame order (reverse: from the last frame down) -
    written as the chain it is, so that float32 means float32 (torch.cumsum may accumulate wider)"""
    order = range(v.shape[1] - 1, -1, -1) if reverse else range(v.shape[1])
    acc, out = torch.zeros_like(v[:, 0]), [None] * v.shape[1]
    for f in order:
        if exclusive:
            out[f] = acc
            acc = acc + v[:, f]
        else:
            acc = acc + v[:, f]
            out[f] = acc
    return torch.stack(out, 1)


def _prev(v):
    """v of the frame before; zero at frame 0"""
    return torch.cat([torch.zeros_like(v[:, :1]), v[:, :-1]], 1)


def _to_scene(to_scene, Bn, dtype):
    """[Bn, 3, 4] of None (identity), [3, 4] or [Bn, 3, 4]"""
    if to_scene is None:
        to_scene = torch.eye(3, 4)
    return to_scene.to(dtype).expand(Bn, 3, 4)


def _recover(x, x_mask, mean, std, dtype):
    """u [B, L, 67], c, s, X, Z, and the masked vx, vz [B, L] of the issue's formulas"""
    u = x[..., :67].to(dtype) * std[:67].to(dtype) + mean[:67].to(dtype)
    pad = torch.zeros(x.shape[:2], dtype=torch.bool) if x_mask is None else x_mask
    w, vx, vz = (torch.where(pad, torch.zeros_like(u[..., i]), u[..., i]) for i in range(3))
    th = _scan(w, exclusive=True)
    c, s = torch.cos(2 * th), torch.sin(2 * th)
    first = torch.arange(x.shape[1]) == 0
    dX = torch.where(first, torch.zeros_like(c), _prev(vx) * c - _prev(vz) * s)
    dZ = torch.where(first, torch.zeros_like(c), _prev(vx) * s + _prev(vz) * c)
    return u, c, s, _scan(dX), _scan(dZ), vx, vz


def h3d_joints_ref(x, x_mask, mean, std, joints=None, to_scene=None, dtype=torch.float64):
    """Positions [B, L, J, 3] of the joints `joints` (None: all 22) of the HumanML3D-feature motion x [B, L, D >= 67] in ``dtype``, plain
    torch: the reference's recover_from_ric written out, a padded frame's velocity columns counted as zero, then p = A P + t."""
    joints = list(range(22)) if joints is None else list(joints)
    u, c, s, X, Z, _, _ = _recover(x, x_mask, mean, std, dtype)
    A = _to_scene(to_scene, x.shape[0], dtype)
    out = []
    for j in joints:
        if j == 0:
            P = (X, u[..., 3], Z)
        else:
            lx, ly, lz = (u[..., 4 + 3 * (j - 1) + a] for a in range(3))
            P = ((lx * c - lz * s) + X, ly, (lx * s + lz * c) + Z)
        out.append(torch.stack([((A[:, r, 0, None] * P[0] + A[:, r, 1, None] * P[1]) + A[:, r, 2, None] * P[2]) + A[:, r, 3, None] for r in range(3)], -1))
    return torch.stack(out, 2)


def _as_columns(pos):
    """positions [B, L, K, 3] as a motion of absolute columns for contact_terms / contact_reference: (x, cols, mean, std)"""
    Bn, L, K, _ = pos.shape
    return pos.reshape(Bn, L, 3 * K), [3 * k for k in range(K)], torch.zeros(3 * K, dtype=pos.dtype), torch.ones(3 * K, dtype=pos.dtype)


def h3d_terms(x, x_mask, q, c, joints, mean, std, to_scene, sigma, dtype):
    """contact_terms of tests/test_guidance_host.py on the recovered positions: (p [B,L,K,3], d2 [B,N,K,L], chat [B,N,K], f* [B,N,K])"""
    flat, cols, zero, one = _as_columns(h3d_joints_ref(x, x_mask, mean, std, joints, to_scene, dtype))
    return contact_terms(flat, x_mask, q, c, cols, zero, one, sigma, dtype)


def h3d_contact_reference(x, x_mask, q, c, joints, mean, std, scale, to_scene=None, sigma=SIGMA, dtype=torch.float64):
    """(-scale * dE/dx [B, L, D], E [B]) of ContactGuidance.h3d in ``dtype``, plain torch: contact_reference on the recovered positions gives
    coef * S[b,f,k,:] (unit scale, unit std), the issue's adjoint carries it back to the features."""
    Bn, L, D = x.shape
    u, cc, ss, _, _, vx, vz = _recover(x, x_mask, mean, std, dtype)
    flat, cols, zero, one = _as_columns(h3d_joints_ref(x, x_mask, mean, std, joints, to_scene, dtype))
    gp, energy = contact_reference(flat, x_mask, q, c, cols, zero, one, torch.ones(Bn), sigma, dtype)
    S = gp.view(Bn, L, len(joints), 3)
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
    grad = scale.to(dtype).view(-1, 1, 1) * std.to(dtype) * du
    if x_mask is not None:
        grad = torch.where(x_mask[..., None], torch.zeros_like(grad), grad)
    return grad, energy


def case_to_scene(kind):
    if kind is None:
        return None
    if kind == "zup":
        return ZUP.clone()
    m = torch.eye(3, 4).repeat(B, 1, 1) + 0.3 * synth.gaussian("h3d_guide_to_scene", (B, 3, 4))          # per sample, not orthogonal
    return m


def h3d_case(case):
    """The inputs of one kernel case (CPU float32 tensors): x, x_mask, q, c, joints, mean, std, scale, to_scene - with the planted edges."""
    L, N, K, D, rotation, scene = case
    tag = f"h3d_guide_{case_id(case)}_s{SEEDS.get(case, 0)}"
    joints = case_joints(case)
    x = synth.gaussian(tag + "_x", (B, L, D))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    mean[0:3] = 0.0
    std[0] = 3.0 if rotation == "turns" else 0.05            # turns: 2 th moves by several radians per frame
    std[1:3] = 0.1
    # a zero entry: that feature is its mean, its gradient zero (a local height; the root alone: a planar velocity - not the root's height,
    # which is all that tells the root's frames 2, 3 and 4 apart)
    std[zero_column(joints)] = 0.0
    if L > DUP[2]:                                           # the root stands still over frames 2, 3 and frame 4 repeats frame 2's pose
        x[DUP[0], DUP[1]:DUP[2], 0:3] = 0.0
        x[DUP[0], DUP[2], 3:] = x[DUP[0], DUP[1], 3:]
    mask = torch.zeros(B, L, dtype=torch.bool)
    if L >= 2:
        mask[1, L - (2 if L >= 4 else 1):] = True
    mask[2, :] = True
    to_scene = case_to_scene(scene)
    q = 1.5 * synth.gaussian(tag + "_q", (B, N, 3))
    p = h3d_joints_ref(x, mask, mean, std, joints, to_scene, torch.float32)
    q[0, 0] = p[0, min(1, L - 1), 0]                         # a point coincident with a joint: d2 = 0, chat = 1
    if N > 1:
        q[1, N - 1] = 100.0                                  # a far point: chat underflows to 0
    c = torch.rand((B, N, K), generator=torch.Generator().manual_seed(N * 100 + K)) * 0.999 + 0.001
    if N > 2:                                                # a target of exactly chat: a zero term
        c[0, 1] = h3d_terms(x, mask, q, c, joints, mean, std, to_scene, SIGMA, torch.float32)[2][0, 1]
    scale = torch.tensor([1.0, 2.5, 0.5])
    return dict(x=x, x_mask=mask, q=q, c=c, joints=joints, mean=mean, std=std, scale=scale, to_scene=to_scene)


# ---------------------------------------------------------------------------------------------------------------- the golden
def test_restatement_equals_the_reference_recover_from_ric():
    """float64: to 1e-12 max|P|.  float32: within 4 x the golden's own float32-minus-float64 error plus one ulp of the largest entry."""
    g = golden("h3d_recover_from_ric")
    u, p32, p64 = g["u"], g["pos32"], g["pos64"]
    assert u.shape == (2, 9, 263) and p64.shape == (2, 9, 22, 3) and p32.dtype == torch.float32 and p64.dtype == torch.float64
    one, zero = torch.ones(263, dtype=torch.float64), torch.zeros(263, dtype=torch.float64)
    big = p64.abs().max().item()
    got64 = h3d_joints_ref(u, None, zero, one, None, None, torch.float64)
    e64 = (got64 - p64).abs().max().item()
    got32 = h3d_joints_ref(u.float(), None, zero.float(), one.float(), None, None, torch.float32)
    assert got32.dtype == torch.float32
    e32, own = (got32.double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
    print(f"[h3d host] restatement vs recover_from_ric: f64 max|diff| {e64:.3e}; f32 max|diff| {e32:.3e}, the golden's own f32 error {own:.3e} "
          f"(max|P| {big:.3f})")
    assert e64 <= 1e-12 * big
    assert e32 <= 4.0 * own + 2.0 ** -23 * big
    assert torch.equal(h3d_joints_ref(u, None, zero, one, [5, 0, 21], None, torch.float64), got64[:, :, [5, 0, 21]])


# ---------------------------------------------------------------------------------------------------------------- the adjoint
def _autograd_of_the_energy(g):
    with torch.no_grad():
        fstar = h3d_terms(g["x"], g["x_mask"], g["q"], g["c"], g["joints"], g["mean"], g["std"], g["to_scene"], SIGMA, torch.float64)[3]
    x = g["x"].double().requires_grad_(True)
    p = h3d_joints_ref(x, g["x_mask"], g["mean"], g["std"], g["joints"], g["to_scene"], torch.float64)          # [B, L, K, 3]
    d = p[:, None] - g["q"].double()[:, :, None, None, :]
    d2 = (d * d).sum(-1).permute(0, 1, 3, 2)                   # [B, N, K, L]
    mn = d2.gather(-1, fstar.clamp(min=0)[..., None])[..., 0]
    chat = torch.where(fstar < 0, torch.zeros_like(mn), torch.exp(-mn / (2 * SIGMA ** 2)))
    energy = ((chat - g["c"].double()) ** 2).mean((1, 2))
    (auto,) = torch.autograd.grad((energy * g["scale"].double()).sum(), x)
    return auto, energy.detach()


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[6]], ids=case_id)
def test_float64_gradient_equals_autograd_of_the_float64_energy(case):
    """with f* held fixed; CASES[2] has the non-orthogonal per-sample to_scene, every case the mask pattern of the GPU tests"""
    g = h3d_case(case)
    want, e = h3d_contact_reference(**g)
    auto, e_auto = _autograd_of_the_energy(g)
    err = (want + auto).abs().max().item()
    print(f"[h3d host] analytic vs autograd {case_id(case)}: max|diff| = {err:.3e} (max|grad| = {auto.abs().max().item():.3e})")
    assert err <= 1e-12 * max(1.0, auto.abs().max().item())
    assert (e - e_auto).abs().max().item() <= 1e-12
    assert torch.equal(want[2], torch.zeros_like(want[2])) and torch.equal(want[g["x_mask"]], torch.zeros_like(want[g["x_mask"]]))
    assert torch.equal(want[..., 67:], torch.zeros_like(want[..., 67:])) and want[0, 0, :3].abs().min() > 0


def test_an_interior_masked_frame_counts_as_zero_velocity_and_gets_no_gradient():
    g = h3d_case(CASES[2])
    g["x_mask"] = torch.zeros(B, 7, dtype=torch.bool)
    g["x_mask"][0, 3] = True                                   # interior
    g["x_mask"][1, 5:] = True
    want, _ = h3d_contact_reference(**g)
    auto, _ = _autograd_of_the_energy(g)
    assert (want + auto).abs().max().item() <= 1e-12 * max(1.0, auto.abs().max().item())
    assert torch.equal(want[0, 3], torch.zeros(263, dtype=torch.float64)) and want[0, 2].abs().max() > 0
    still = g["x"].clone()
    still[0, 3, 0:3] = 0.0                                     # (mean[0:3] is zero in the fixtures: these velocities are exactly zero)
    a = h3d_joints_ref(g["x"], g["x_mask"], g["mean"], g["std"], None, g["to_scene"])
    b = h3d_joints_ref(still, torch.zeros_like(g["x_mask"]), g["mean"], g["std"], None, g["to_scene"])
    assert torch.equal(a[0], b[0])


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=case_id)
def test_valid_frames_first_masks_leave_the_valid_frames_as_unmasked(case):
    g = h3d_case(case)
    masked = h3d_joints_ref(g["x"], g["x_mask"], g["mean"], g["std"], None, g["to_scene"])
    plain = h3d_joints_ref(g["x"], None, g["mean"], g["std"], None, g["to_scene"])
    valid = ~g["x_mask"]
    assert g["x_mask"][1].any() and torch.equal(masked[valid], plain[valid])


# ---------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixture_margin(case):
    """Every nearest-frame decision of the GPU fixtures is clear in float64 (relative gap > 1e-4) but for the planted duplicate pose, where
    the first index wins, and float32 picks the same frames: no (n, k) pair is excluded from any comparison."""
    g = h3d_case(case)
    L = case[0]
    args = (g["x"], g["x_mask"], g["q"], g["c"], g["joints"], g["mean"], g["std"], g["to_scene"], SIGMA)
    p, d2, _, fstar = h3d_terms(*args, torch.float64)
    assert (fstar[2] == -1).all() and (fstar[:2] >= 0).all() and not g["x_mask"][0].any() and g["x_mask"][2].all()
    assert g["x_mask"][1].any() == (L >= 2) and not g["x_mask"][1, 0]
    d2 = d2.clone()
    if L > DUP[2]:
        assert torch.equal(p[DUP[0], DUP[1]], p[DUP[0], DUP[2]]) and (fstar[DUP[0]] != DUP[2]).all()
        p32 = h3d_joints_ref(g["x"], g["x_mask"], g["mean"], g["std"], g["joints"], g["to_scene"], torch.float32)
        assert torch.equal(p32[DUP[0], DUP[1]], p32[DUP[0], DUP[2]])
        d2[DUP[0], :, :, DUP[2]] = float("inf")                # the planted exact tie: the duplicate leaves the comparison
    f32 = h3d_terms(*args, torch.float32)[3]
    assert torch.equal(f32, fstar)
    valid = (~g["x_mask"]).sum(1)
    for b in range(2):
        if valid[b] - (1 if b == DUP[0] and L > DUP[2] else 0) < 2:
            continue                                            # one candidate frame: nothing to decide
        two = d2[b].topk(2, dim=-1, largest=False).values
        gap = (two[..., 1] - two[..., 0]) / two[..., 1]
        print(f"[h3d host] fixture margin {case_id(case)} sample {b}: smallest relative gap {gap.min().item():.3e}")
        assert gap.min().item() > 1e-4
    if case[4] == "turns":                                      # 2 th does pass through several full turns
        th2 = 2 * _scan(g["x"][..., 0].double() * g["std"][0].double(), exclusive=True)
        assert (th2[0].max() - th2[0].min()).item() > 4 * 3.141592653589793


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_h3d_exports_declared_structs_mirrored_and_the_abi_version_kept(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert int(re.search(r"#define AFM_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert ffi.H3D_JOINTS == int(re.search(r"#define AFM_H3D_JOINTS (\d+)", hdr).group(1)) == 22 and ffi.H3D_COLS == 4 + 3 * 21
    assert [f for f, _ in ffi.ContactGuide._fields_][-1] == "h3d"          # appended: every earlier field keeps its offset
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_h3d_layout", ffi.H3dLayout), ("afm_contact_guide", ffi.ContactGuide))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "h3d_layout.c", tmp_path / "h3d_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_python_refusals():
    mean, std = torch.zeros(263), torch.ones(263)
    x = torch.zeros(2, 5, 263)
    for build in (lambda **kw: ContactGuidance.h3d(kw.pop("joints", [0, 10]), kw.pop("mean", mean), kw.pop("std", std), **kw),
                  lambda **kw: ops.h3d_joints(kw.pop("x", x), kw.pop("mean", mean), kw.pop("std", std), **kw)):
        with pytest.raises(ValueError, match="outside 0..21"):
            build(joints=[0, 22])
        with pytest.raises(ValueError, match="outside 0..21"):
            build(joints=[-1])
        with pytest.raises(ValueError, match="named twice"):
            build(joints=[3, 7, 3])
        with pytest.raises(ValueError, match="joints, got 0"):
            build(joints=[])
        for bad in (torch.zeros(4, 3), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 2, 3, 4), [[0.0] * 4] * 3):
            with pytest.raises(ValueError, match="to_scene must be a float32"):
                build(to_scene=bad)
    with pytest.raises(ValueError, match="columns"):            # D < 67
        ContactGuidance.h3d([0], torch.zeros(66), torch.ones(66))
    with pytest.raises(ValueError, match="67"):
        ops.h3d_joints(torch.zeros(2, 5, 66), torch.zeros(66), torch.ones(66))
    with pytest.raises(ValueError, match="mean and std"):
        ContactGuidance.h3d([0], torch.zeros(263), torch.ones(262))
    with pytest.raises(ValueError, match="mean and std"):
        ops.h3d_joints(x, torch.zeros(67), torch.ones(67))
    with pytest.raises(ValueError, match=f"1 to {ffi.GUIDE_MAX_JOINTS} joints"):          # the guidance takes 16 joints, the recovery all 22
        ContactGuidance.h3d(list(range(ffi.GUIDE_MAX_JOINTS + 1)), mean, std)
    with pytest.raises(ValueError, match="1 to 22 joints"):
        ops.h3d_joints(x, mean, std, joints=list(range(22)) + [0])
    # against a batch: the device and the count of a per-sample to_scene
    kw = dict(c_pc_xyz=torch.zeros(2, 9, 3), c_pc_contact=torch.zeros(2, 9, 2))
    t = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="to_scene is on meta"):
        ContactGuidance.h3d([0, 10], mean, std, to_scene=torch.zeros(3, 4, device="meta"))(x, t, **kw)
    with pytest.raises(ValueError, match="to_scene is on meta"):
        ops.h3d_joints(x, mean, std, to_scene=torch.zeros(3, 4, device="meta"))
    with pytest.raises(ValueError, match="3 matrices for a batch of 2"):
        ContactGuidance.h3d([0, 10], mean, std, to_scene=torch.zeros(3, 3, 4)).energy(x, **kw)
    with pytest.raises(ValueError, match="3 matrices for a batch of 2"):
        ops.h3d_joints(x, mean, std, to_scene=torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="c_pc_contact"):       # K is the joint list's
        ContactGuidance.h3d([0, 10, 11], mean, std)(x, t, **kw)
    with pytest.raises(ValueError, match="the sample is"):
        ContactGuidance.h3d([0, 10], mean, std)(torch.zeros(2, 5, 67), t, **kw)
    with pytest.raises(ffi.AfmError):                           # callables over HIP: the CPU has no path
        ContactGuidance.h3d([0, 10], mean, std)(x, t, **kw)
    with pytest.raises(ffi.AfmError):
        ops.h3d_joints(x, mean, std)
    # the column form keeps its checks and texts
    with pytest.raises(ValueError, match="leaves the motion vector"):
        ContactGuidance([0, 64], torch.zeros(66), torch.ones(66))
    g = ContactGuidance.h3d([0, 10], mean, std, t_start=300)
    assert g.joints == [0, 10] and g.t_start == 300 and ContactGuidance([0], mean, std).joints is None
