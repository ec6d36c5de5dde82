"""Imputation of known motion values on the host (no GPU): the C ABI declares, exports and mirrors the new surface; the reference goldens
(tools/make_goldens_impute.py) are self-consistent; the CPU oracle wrapped with the same select reproduces them; afm.diffusion.Impute
broadcasts its mask and refuses what does not fit."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm.diffusion import Impute
from oracle import diffusion_ref as df
from oracle import shapes as sh

from conftest import ROOT, golden
from test_cfg_host import AMP, DROPS, guided_oracle
from test_ddim_host import _diffusion, _update
from test_oracle_golden import _cmdm_model

NEW = {"afm_impute", "afm_impute_step", "afm_cmdm_impute_loop_range"}
SHAPE = (2, 16, 263)
SCALE = (2.5, 7.5)
# golden tag -> (guided, clip_denoised) of the DDPM loops at respacing "5"; -> (guided, eta) of the DDIM loops at "ddim50"
DDPM_LOOPS = {"r5": (False, False), "r5_clip": (False, True), "cfg_r5": (True, False)}
DDIM_LOOPS = {"eta0": (False, 0.0), "eta1": (False, 1.0), "cfg_eta0": (True, 0.0)}


def impute_mask(B=2, L=16, D=263):
    """The mask of tools/make_goldens_impute.py, restated: sample 0 knows frames {0, 1, 2, 15} on all features (in-betweening), sample 1
    knows features 0..3 on all frames (root trajectory)."""
    m = torch.zeros(B, L, D, dtype=torch.bool)
    m[0, [0, 1, 2, 15], :] = True
    m[1, :, 0:4] = True
    return m


def impute_known():
    return synth.gaussian("impute_known", SHAPE)


def imputed(model, known=None, mask=None):
    """a denoiser with the select behind it, in the dtype of its output"""
    known = impute_known() if known is None else known
    mask = impute_mask() if mask is None else mask
    return lambda x, t, **kw: (lambda o: torch.where(mask, known.to(o.dtype), o))(model(x, t, **kw))


def oracle_model(guided, f64=False):
    """the oracle's CMDM (or the guided composition of tests/test_cfg_host.py) on the goldens' case, float32 or its float64 twin"""
    from gpu_util import to_f64
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    scale = torch.tensor(SCALE)
    if f64:
        g, sd, scale = to_f64(g), to_f64(sd), scale.double()
    return guided_oracle(sd, g, scale, DROPS["both"]) if guided else _cmdm_model(g, sd)


def ddim_loop_ref(model, x_T, step_noise, eta, clip_denoised=False):
    """ddim_sample_loop at respacing "ddim50" on the CPU: the update expression of tests/test_ddim_host.py (`_update`, which reproduces the
    reference's ddim_sample bit for bit on the product's float32 rows) around ``model``; in float64 when x_T is."""
    d = _diffusion(1000, "ddim50")
    rows, tmap = d.ddim_tables("cpu", eta), torch.tensor(d.timestep_map)
    img = x_T
    with torch.no_grad():
        for j, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
            x0 = model(img, tmap[torch.tensor([i] * x_T.shape[0])])
            if clip_denoised:
                x0 = x0.clamp(-1, 1)
            img = _update(x0, img, step_noise[j], rows, i)
    return img


def loop_inputs(prefix, n):
    return synth.gaussian(f"{prefix}_xT", SHAPE), [synth.gaussian(f"{prefix}_{j}", SHAPE) for j in range(n)]


def _err(name, got, want):
    err = (got.double() - want.double()).abs().max().item()
    print(f"[impute host] {name}: max|diff| = {err:.3e} (max|ref| = {want.abs().max().item():.3e})")
    return err


def test_impute_exports_declared_and_struct_mirrored(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert "#define AFM_ABI_VERSION 7" in hdr and ffi.ABI_VERSION == 7           # additive: the version stays
    if os.path.exists(ffi.lib_path()):
        lib = ctypes.CDLL(ffi.lib_path())
        for name in NEW:
            assert hasattr(lib, name), name
        assert ffi.load().afm_version() == 7
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pairs = (("afm_impute_step_args", ffi.ImputeStepArgs), ("afm_cfg_step_args", ffi.CfgStepArgs))      # (the second: left alone)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "impute_layout.c", tmp_path / "impute_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_entry_points_refuse_a_known_without_a_mask():
    """AFM_E_BADARG before anything is looked at or launched (no GPU needed: the checks come first)."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    buf = torch.zeros(8)
    mk = torch.zeros(8, dtype=torch.uint8)
    assert lib.afm_impute(buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), 8, None) == -1
    assert lib.afm_impute(buf.data_ptr(), None, mk.data_ptr(), buf.data_ptr(), 8, None) == -1
    assert lib.afm_impute(buf.data_ptr(), buf.data_ptr(), mk.data_ptr(), buf.data_ptr(), -1, None) == -1
    assert lib.afm_impute(None, None, None, None, 0, None) == 0                   # nothing to do
    assert lib.afm_impute_step(None, None) == -1
    a = ffi.ImputeStepArgs()
    a.x0_c = a.x_t = a.x_next = a.known = a.c1 = a.c2 = a.sigma = a.noise = buf.data_ptr()
    a.B, a.per_sample = 2, 4
    assert lib.afm_impute_step(ctypes.byref(a), None) == -1                       # known without mask
    a.known, a.mask = None, mk.data_ptr()
    assert lib.afm_impute_step(ctypes.byref(a), None) == -1                       # mask without known
    a.known, a.x0_u = buf.data_ptr(), buf.data_ptr()
    assert lib.afm_impute_step(ctypes.byref(a), None) == -1                       # x0_u without scale
    a.x0_u, a.c1 = None, None
    assert lib.afm_impute_step(ctypes.byref(a), None) == -1                       # neither kind of rows
    args = [None] * 25
    args[13:19] = [1, 0, 0, 0, 2, 4]
    args[19], args[21], args[22] = None, 0, 0
    args[11] = buf.data_ptr()
    assert lib.afm_cmdm_impute_loop_range(*args) == -1                            # known without mask, in front of every other check


# ---------------------------------------------------------------------------------------------------------------- goldens
def test_goldens_are_self_consistent():
    """The last step writes pred_xstart into the sample unchanged (DDPM: c1 = 1, c2 = 0, sigma = 0; DDIM: c = 1, d = 0), so every chain
    ends on `known` where the mask is set - exactly, in the reference's float32 arithmetic: 1 * k + 0 * x + 0 * z == k and
    k * 1 + 0 * eps == k for finite x, z, eps."""
    known, mask = impute_known(), impute_mask()
    assert known.abs().max() > 1 and (known[mask].abs() > 1).any()               # the clip case tests the order: denoised_fn, then clamp
    assert mask[0].all(1).nonzero().flatten().tolist() == [0, 1, 2, 15] and mask[1].all(0).nonzero().flatten().tolist() == [0, 1, 2, 3]
    ps = golden("cmdm_impute_p_sample_t500")
    assert ps["pred_xstart"].dtype == torch.float32 and torch.equal(ps["pred_xstart"][mask], known[mask])
    plain = golden("cmdm_p_sample_t500")          # the same inputs without the hook: untouched where nothing is known
    assert torch.equal(ps["pred_xstart"][~mask], plain["pred_xstart"][~mask]) and torch.equal(ps["sample"][~mask], plain["sample"][~mask])
    assert not torch.equal(ps["sample"][mask], plain["sample"][mask])
    for tag, (_, clip) in DDPM_LOOPS.items():
        s = golden(f"cmdm_impute_loop_{tag}")["sample"]
        assert torch.equal(s[mask], (known.clamp(-1, 1) if clip else known)[mask]), tag
        assert torch.isfinite(s).all() and not torch.equal(s[~mask], golden("cmdm_loop_r5")["sample"][~mask])     # the rest does react
    for tag in DDIM_LOOPS:
        s = golden(f"cmdm_impute_ddim_loop_ddim50_{tag}")["sample"]
        assert torch.equal(s[mask], known[mask]), tag
        assert torch.isfinite(s).all()


def test_oracle_with_the_select_reproduces_the_p_sample_golden():
    g, ps = golden("cmdm_forward_N1024_L16"), golden("cmdm_impute_p_sample_t500")
    out = df.p_sample(df.Schedule(1000), imputed(oracle_model(False)), g["x"], torch.tensor([500, 500]),
                      synth.gaussian("p_sample_noise_500", SHAPE))
    assert torch.equal(out["pred_xstart"][impute_mask()], ps["pred_xstart"][impute_mask()])
    assert _err("oracle p_sample pred_xstart", out["pred_xstart"], ps["pred_xstart"]) <= BOUND_PSAMPLE["pred_xstart"]
    assert _err("oracle p_sample sample", out["sample"], ps["sample"]) <= BOUND_PSAMPLE["sample"]


@pytest.mark.parametrize("tag", list(DDPM_LOOPS))
def test_oracle_with_the_select_reproduces_the_ddpm_loop_goldens(tag):
    guided, clip = DDPM_LOOPS[tag]
    s = df.Schedule(1000, "cosine", "5")
    xT, nz = loop_inputs("loop_r5", s.num_timesteps)
    out = df.p_sample_loop(s, imputed(oracle_model(guided)), xT, nz, clip_denoised=clip)
    assert _err(f"oracle DDPM loop {tag}", out, golden(f"cmdm_impute_loop_{tag}")["sample"]) <= BOUND_LOOP[tag]


@pytest.mark.parametrize("tag", list(DDIM_LOOPS))
def test_oracle_with_the_select_reproduces_the_ddim_loop_goldens(tag):
    guided, eta = DDIM_LOOPS[tag]
    xT, nz = loop_inputs("ddim_loop_ddim50", 50)
    out = ddim_loop_ref(imputed(oracle_model(guided)), xT, nz, eta)
    assert _err(f"oracle DDIM loop {tag}", out, golden(f"cmdm_impute_ddim_loop_ddim50_{tag}")["sample"]) <= BOUND_DDIM[tag]


# Measured on the CPU (beside each bound); a bound is at most 20x its measurement and never above the ceiling of the matching host test:
# 2e-5 for p_sample and 1e-4 for a loop (tests/test_oracle_golden.py: test_p_sample, test_p_sample_loop; the DDIM loops have no host test
# of their own and take the loop ceiling), times AMP for the guided cases (tests/test_cfg_host.py).  The select amplifies nothing.
BOUND_PSAMPLE = {"pred_xstart": 2e-5,      # 3.0e-6: 20x is above the ceiling, so the ceiling
                 "sample": 4.8e-6}         # 2.4e-7 (coef1 is small at t = 500)
BOUND_LOOP = {"r5": 6.4e-5,                # 3.2e-6
              "r5_clip": 6.3e-5,           # 3.2e-6
              "cfg_r5": 1e-4 * AMP}        # 1.3e-4: 20x is above the ceiling 1.4e-3, so the ceiling
BOUND_DDIM = {"eta0": 5.2e-5,              # 2.6e-6
              "eta1": 5.8e-5,              # 2.9e-6
              "cfg_eta0": 9.4e-4}          # 4.7e-5
assert max(BOUND_PSAMPLE.values()) <= 2e-5 and all(b <= 1e-4 * (AMP if "cfg" in k else 1) for k, b in {**BOUND_LOOP, **BOUND_DDIM}.items())


# ---------------------------------------------------------------------------------------------------------------- Impute
@pytest.mark.parametrize("mshape", [(2, 16, 263), (16, 263), (2, 16, 1), (2, 1, 263), (263,), (1, 1, 1)])
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_impute_broadcasts_its_mask_once(mshape, dtype):
    known = impute_known()
    m = (synth.gaussian("impute_mask_bits", mshape) > 0).to(dtype)
    imp = Impute(known, m)
    assert imp.mask.dtype == torch.uint8 and imp.mask.shape == known.shape and imp.mask.is_contiguous()
    assert imp.known.dtype == torch.float32 and imp.known.is_contiguous() and imp.shape == SHAPE
    assert torch.equal(imp.mask.bool(), m.bool().expand(SHAPE))
    part = imp.narrow(1, 1)
    assert isinstance(part, Impute) and part.shape == (1, 16, 263) and torch.equal(part.mask, imp.mask[1:2]) and torch.equal(part.known, known[1:2])
    assert part.known.is_contiguous() and part.mask.is_contiguous() and part.known.data_ptr() == known[1:2].data_ptr()      # a view: no copy


def test_impute_refuses_what_does_not_fit():
    known = impute_known()
    for bad in [(3, 16, 263), (2, 16, 2), (16,), (1, 2, 16, 263)]:
        with pytest.raises(ValueError, match="broadcast"):
            Impute(known, torch.zeros(bad, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        Impute(known, torch.zeros(SHAPE))
    with pytest.raises(ValueError, match=r"\[B, L, D\]"):
        Impute(known[0], torch.zeros(16, 263, dtype=torch.bool))
    imp = Impute(known, impute_mask())
    with pytest.raises(ValueError, match="sample is"):
        imp.check(torch.zeros(2, 15, 263))
    with pytest.raises(ValueError, match="narrow"):
        imp.narrow(1, 2)
    with pytest.raises(ffi.AfmError):           # a callable over HIP: the CPU has no path (the oracle is the CPU implementation)
        imp(torch.zeros(SHAPE))


def test_sampling_entry_points_take_the_imputation():
    from afm.base import create_gaussian_diffusion, create_model
    from afm.cdm import CDM
    from afm.cmdm import CMDM, GuidedCMDM
    from afm.diffusion import _takes
    from afm.pipeline import two_stage_sample
    from test_cfg_host import _cfg
    assert inspect.signature(two_stage_sample).parameters["motion_impute"].default is None
    assert all(_takes(cls.afm_native_loop, "impute") for cls in (CMDM, GuidedCMDM, CDM))
    # shape and device are checked against x before the native loop is entered
    m, d = create_model(_cfg(), device="cpu").eval(), create_gaussian_diffusion(_cfg())
    imp = Impute(impute_known(), impute_mask())
    with pytest.raises(ValueError, match="sample is"):
        d.p_sample_loop(m, (2, 15, 263), noise=torch.zeros(2, 15, 263), denoised_fn=imp, model_kwargs={})
    # trans_dec has no native loop: the generic path takes the same object as a plain denoised_fn
    assert create_model(_cfg(arch="trans_dec"), device="cpu").afm_native_loop is None
