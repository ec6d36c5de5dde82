"""Classifier-free guidance on the host (no GPU): the C ABI declares, exports and mirrors the guided surface; the reference goldens
(tools/make_goldens_cfg.py) are self-consistent; the CPU oracle composed into a guided callable reproduces them; the wrapper refuses
what it cannot do."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.config import to_config
from oracle import denoiser_ref as dr
from oracle import diffusion_ref as df
from oracle import shapes as sh

from conftest import ROOT, golden

DROPS = {"both": ("text", "pc"), "text": ("text",), "pc": ("pc",)}
NEW = {"afm_cfg_combine", "afm_cfg_step", "afm_cmdm_cfg_workspace_bytes", "afm_cmdm_cfg_forward", "afm_cmdm_cfg_loop_workspace_bytes",
       "afm_cmdm_cfg_sample_loop_range", "afm_cmdm_cfg_ddim_loop_range"}
# |s| + |1 - s| of the largest scale: how far the combination can amplify the branches' errors
AMP = 7.5 + 6.5


def _cfg(arch="trans_enc", mask_motion=True):
    return to_config(dict(
        model=dict(name="CMDM", input_feats=263, data_repr="h3d", time_emb_dim=512,
                   contact_model=dict(contact_type="contact_cont_joints", contact_joints=[0, 10, 11, 12, 20, 21],
                                      planes=[32, 64, 128, 256], num_points=1024, blocks=[2, 2, 2, 2]),
                   text_model=dict(version="ViT-B/32", max_length=20), arch=arch, latent_dim=512,
                   mask_motion=mask_motion, num_layers=[1, 1, 1, 1, 1], num_heads=8, dropout=0.1, dim_feedforward=1024),
        diffusion=dict(predict_xstart=True, steps=1000, noise_schedule="cosine", timestep_respacing="5",
                       rescale_timesteps=False, loss_type="MSE", learn_sigma=False, sigma_small=True)))


def guided_oracle(sd, g, scale, drop):
    """The oracle's CMDM twice per call, combined in float32 torch in the association the product fixes."""
    def model(x, t, **kw):
        B = x.shape[0]
        ones = torch.ones(B, 1, dtype=torch.bool)
        sw = {}
        if "text" in drop:
            sw["c_text_mask"] = ones
        if "pc" in drop:
            sw["c_pc_mask"] = ones
        c = dr.cmdm_forward(sd, x, t, g["text_feat"], x_mask=g["x_mask"], cont_emb=g["cont_emb"])
        u = dr.cmdm_forward(sd, x, t, g["text_feat"], x_mask=g["x_mask"], cont_emb=g["cont_emb"], **sw)
        return u + scale.view(B, 1, 1) * (c - u)
    return model


def _err(name, got, want):
    err = (got.double() - want.double()).abs().max().item()
    print(f"[cfg host] {name}: max|diff| = {err:.3e} (max|ref| = {want.abs().max().item():.3e})")
    return err


def test_cfg_exports_declared_and_structs_mirrored(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert "#define AFM_ABI_VERSION 7" in hdr and ffi.ABI_VERSION == 7
    assert f"#define AFM_CFG_FORCE_MASKED 0x{ffi.CFG_FORCE_MASKED:x}" in hdr
    if os.path.exists(ffi.lib_path()):
        lib = ctypes.CDLL(ffi.lib_path())
        for name in NEW:
            assert hasattr(lib, name), name
        assert ffi.load().afm_version() == 7
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pairs = (("afm_cfg_args", ffi.CfgArgs), ("afm_cfg_step_args", ffi.CfgStepArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "cfg_layout.c", tmp_path / "cfg_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


@pytest.mark.parametrize("tt", [999, 500, 0])
def test_goldens_are_self_consistent(tt):
    gs = {k: golden(f"cmdm_cfg_forward_{k}_t{tt}") for k in DROPS}
    for k, g in gs.items():
        s = g["scale"].view(2, 1, 1)
        assert g["scale"].tolist() == [2.5, 7.5] and g["x0_c"].dtype == torch.float32
        assert torch.equal(g["guided"], g["x0_u"] + s * (g["x0_c"] - g["x0_u"])), k
        assert torch.equal(g["x0_c"], gs["both"]["x0_c"])
    # the synthetic weights do exercise the guidance term
    assert (gs["both"]["x0_c"] - gs["both"]["x0_u"]).abs().max() > 1.0 and (gs["text"]["x0_c"] - gs["text"]["x0_u"]).abs().max() > 0.05


@pytest.mark.parametrize("tt", [999, 500, 0])
def test_guided_oracle_reproduces_the_forward_goldens(tt):
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    for k, drop in DROPS.items():
        gg = golden(f"cmdm_cfg_forward_{k}_t{tt}")
        out = guided_oracle(sd, g, gg["scale"], drop)(g["x"], torch.tensor([tt, tt]))
        # measured on the CPU: <= 3.0e-5 over the three timesteps and drop sets; 20x that is above the ceiling (2e-5 of the unguided
        # test_cmdm_forward per branch, times AMP), so the ceiling is the bound
        assert _err(f"guided oracle forward t={tt} drop={k}", out, gg["guided"]) <= 2e-5 * AMP


def test_guided_oracle_reproduces_the_p_sample_golden():
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    gs = golden("cmdm_cfg_p_sample_t500")
    out = df.p_sample(df.Schedule(1000), guided_oracle(sd, g, gs["scale"], DROPS["both"]), g["x"], torch.tensor([500, 500]),
                      synth.gaussian("p_sample_noise_500", (2, 16, 263)))
    assert _err("guided oracle p_sample pred_xstart", out["pred_xstart"], gs["pred_xstart"]) <= 2e-5 * AMP       # measured 2.7e-5
    assert _err("guided oracle p_sample sample", out["sample"], gs["sample"]) <= 4.8e-6                          # measured 2.4e-7


@pytest.mark.parametrize("tag,drop,clip", [("r5", "both", False), ("r5_clip", "both", True), ("r5_text", "text", False)])
def test_guided_oracle_reproduces_the_ddpm_loop_goldens(tag, drop, clip):
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    gl = golden(f"cmdm_cfg_loop_{tag}")
    s = df.Schedule(1000, "cosine", "5")
    nz = [synth.gaussian(f"loop_r5_{j}", (2, 16, 263)) for j in range(s.num_timesteps)]
    xT = synth.gaussian("loop_r5_xT", (2, 16, 263))
    model = guided_oracle(sd, g, gl["scale"], DROPS[drop])
    out = df.p_sample_loop(s, model, xT, nz, clip_denoised=clip)
    err = _err(f"guided oracle loop {tag}", out, gl["sample"])
    assert err <= BOUND_LOOP[tag]
    if clip:
        # the clamp is live in the clipped golden: guided x_start reaches ~18 at s = 7.5 with these weights
        assert (df.p_sample_loop(s, model, xT, nz) - gl["sample"]).abs().max() > 1e-2


# measured on the CPU: r5 6.8e-5, r5_clip 4.2e-5, r5_text 3.7e-5; each bound <= 20x its measurement and <= 1e-4 * AMP = 1.4e-3
# (1e-4: the unguided test_p_sample_loop of tests/test_oracle_golden.py)
BOUND_LOOP = {"r5": 1.3e-3, "r5_clip": 8e-4, "r5_text": 7e-4}
assert all(b <= 1e-4 * AMP for b in BOUND_LOOP.values())


# ---------------------------------------------------------------------------------------------------------------- errors, loud
def _model(**kw):
    return create_model(_cfg(**kw), device="cpu").eval()


def test_wrapper_refuses_what_it_cannot_do():
    m = _model()
    with pytest.raises(ValueError, match="mask_motion"):
        GuidedCMDM(_model(mask_motion=False), 2.5)
    with pytest.raises(ValueError, match="unknown"):
        GuidedCMDM(m, 2.5, drop=("text", "scene"))
    with pytest.raises(ValueError, match="empty"):
        GuidedCMDM(m, 2.5, drop=())
    with pytest.raises(NotImplementedError, match="trans_enc"):
        GuidedCMDM(_model(arch="trans_dec"), 2.5)
    with pytest.raises(TypeError):
        GuidedCMDM(torch.nn.Linear(2, 2), 2.5)
    with pytest.raises(ValueError, match="scale"):
        GuidedCMDM(m, torch.ones(2, 2))
    w = GuidedCMDM(m, torch.tensor([2.5, 7.5, 1.0]), drop="text")
    assert w.drop == ("text",) and w.motion_dim == 263
    with pytest.raises(ValueError, match="3 values for a batch of 2"):
        w._cfg(2, torch.device("cpu"))
    cfg = GuidedCMDM(m, 2.5)._cfg(2, torch.device("cpu"))
    assert (cfg.drop_text, cfg.drop_pc, cfg.flags) == (1, 1, 0)
    assert GuidedCMDM(m, 2.5, force_masked=True)._cfg(2, torch.device("cpu")).flags == ffi.CFG_FORCE_MASKED


@pytest.mark.parametrize("switch", ["c_text_mask", "c_pc_mask", "c_text_erase", "c_pc_erase"])
def test_wrapper_refuses_user_supplied_condition_switches(switch):
    w = GuidedCMDM(_model(), 2.5)
    x, kw = torch.zeros(2, 16, 263), {switch: torch.ones(2, 1, dtype=torch.bool), "x_mask": torch.zeros(2, 16, dtype=torch.bool)}
    with pytest.raises(ValueError, match=switch):
        w(x, torch.tensor([1, 2]), **kw)
    d = create_gaussian_diffusion(_cfg())
    with pytest.raises(ValueError, match=switch):          # the sampling entry points: the switches route to the step-by-step path, which refuses
        d.p_sample_loop(w, (2, 16, 263), noise=x, model_kwargs=kw)
    with pytest.raises(ValueError, match=switch):
        w.afm_native_loop(d, x, kw)


def test_unguided_model_keeps_refusing_the_switches_in_its_native_loop():
    m = _model()
    with pytest.raises(NotImplementedError):
        m.afm_native_loop(create_gaussian_diffusion(_cfg()), torch.zeros(2, 16, 263), {"c_text_mask": torch.ones(2, 1, dtype=torch.bool)})


def test_two_stage_sample_takes_the_guidance_arguments():
    import inspect
    from afm.pipeline import two_stage_sample
    p = inspect.signature(two_stage_sample).parameters
    assert p["guidance_scale"].default is None and p["guidance_drop"].default == ("text", "pc")
