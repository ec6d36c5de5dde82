"""Two-scale classifier-free guidance (one scale per condition) on the host (no GPU): the C ABI declares, exports and mirrors the new
surface and refuses bad arguments before any launch; the reference goldens (tools/make_goldens_cfg2.py) are self-consistent; the CPU
oracle composed three times per call reproduces them; the wrapper and the two-stage pipeline refuse what they cannot do."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi, synth
from afm.base import create_gaussian_diffusion
from afm.cmdm import GuidedCMDM
from oracle import denoiser_ref as dr
from oracle import diffusion_ref as df
from oracle import shapes as sh

from conftest import ROOT, golden
from test_cfg_host import AMP, _cfg, _model
from test_impute_host import ddim_loop_ref, impute_known, impute_mask, imputed, loop_inputs

NEW = {"afm_cfg2_combine", "afm_cfg2_step", "afm_cmdm_cfg2_workspace_bytes", "afm_cmdm_cfg2_forward", "afm_cmdm_cfg2_loop_workspace_bytes",
       "afm_cmdm_cfg2_loop_range"}
SHAPE = (2, 16, 263)
SCALES = {"pc": (1.5, 2.5), "text": (2.5, 7.5)}          # per sample
ORDERS = {"pc_text": ("pc", "text"), "text_pc": ("text", "pc")}          # golden tag -> (first, second)
SWITCH = {"text": "c_text_mask", "pc": "c_pc_mask"}
# how far the combination (1 - s1) u + (s1 - s2) a + s2 c can amplify the branches' errors: the AMP of the single-scale tests
assert all(max(abs(1 - a) + abs(a - b) + abs(b) for a, b in zip(SCALES[f], SCALES[s])) == AMP for f, s in ORDERS.values())


def scale_rows(order, dtype=torch.float32):
    return tuple(torch.tensor(SCALES[k], dtype=dtype) for k in order)


def branches_oracle(sd, g, order):
    """(c, a, u) of the oracle's CMDM: a keeps only the first condition of `order`, u keeps none"""
    first, second = order

    def branches(x, t):
        ones = torch.ones(x.shape[0], 1, dtype=torch.bool)
        run = lambda **sw: dr.cmdm_forward(sd, x, t, g["text_feat"], x_mask=g["x_mask"], cont_emb=g["cont_emb"], **sw)
        return run(), run(**{SWITCH[second]: ones}), run(**{SWITCH[first]: ones, SWITCH[second]: ones})
    return branches


def combine2(c, a, u, s1, s2):
    """the fixed expression, in the dtype of its operands, every torch operation rounded on its own"""
    g1 = u + s1.view(-1, 1, 1) * (a - u)
    return g1 + s2.view(-1, 1, 1) * (c - a)


def guided2_oracle(sd, g, order, dtype=torch.float32):
    """The oracle's CMDM three times per call, combined in torch in the association the product fixes."""
    s1, s2 = scale_rows(order, dtype)
    br = branches_oracle(sd, g, order)
    return lambda x, t, **kw: combine2(*br(x, t), s1, s2)


def _case():
    return golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())


def _err(name, got, want):
    err = (got.double() - want.double()).abs().max().item()
    print(f"[cfg2 host] {name}: max|diff| = {err:.3e} (max|ref| = {want.abs().max().item():.3e})")
    return err


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_cfg2_exports_declared_and_structs_mirrored(tmp_path):
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
    pairs = (("afm_cfg2_args", ffi.Cfg2Args), ("afm_cfg2_step_args", ffi.Cfg2StepArgs), ("afm_cfg_args", ffi.CfgArgs),      # (the last two: left alone)
             ("afm_cfg_step_args", ffi.CfgStepArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "cfg2_layout.c", tmp_path / "cfg2_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """AFM_E_BADARG (-1) with host pointers and no GPU: the checks come before anything is read or enqueued."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    buf, mk = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    p = buf.data_ptr()
    # the stand-alone combine: every tensor and both scales
    assert lib.afm_cfg2_combine(p, p, p, p, None, p, 2, 4, None) == -1
    assert lib.afm_cfg2_combine(p, p, p, None, p, p, 2, 4, None) == -1
    assert lib.afm_cfg2_combine(p, None, p, p, p, p, 2, 4, None) == -1
    assert lib.afm_cfg2_combine(p, p, p, p, p, p, 0, 4, None) == 0               # nothing to do
    # the step: a middle branch without both scales, or without the unconditioned branch; known without mask and the reverse
    assert lib.afm_cfg2_step(None, None) == -1

    def step_args():
        a = ffi.Cfg2StepArgs()
        a.x0_c = a.x0_a = a.x0_u = a.scale_first = a.scale_second = a.x_t = a.x_next = a.c1 = a.c2 = a.sigma = a.noise = p
        a.B, a.per_sample = 2, 4
        return a
    for field in ("scale_first", "scale_second", "x0_u", "x0_a"):
        a = step_args()
        setattr(a, field, None)
        assert lib.afm_cfg2_step(ctypes.byref(a), None) == -1, field
    a = step_args()
    a.known = p
    assert lib.afm_cfg2_step(ctypes.byref(a), None) == -1                         # known without mask
    a.known, a.mask = None, mk.data_ptr()
    assert lib.afm_cfg2_step(ctypes.byref(a), None) == -1                         # mask without known
    a = step_args()
    a.c1 = None
    assert lib.afm_cfg2_step(ctypes.byref(a), None) == -1                         # neither kind of rows
    # the loop: a missing frame_mask and known without mask, in front of every other check (the weight pack is never looked at)
    cfg = ffi.Cfg2Args(p, p, 1, 0)
    args = [None] * 25
    args[13:19] = [1, 0, 0, 0, 2, 4]
    args[21], args[22] = 0, 0
    args[10] = ctypes.byref(cfg)
    assert lib.afm_cmdm_cfg2_loop_range(*args) == -1                              # no frame_mask
    args[3], args[11] = mk.data_ptr(), p
    assert lib.afm_cmdm_cfg2_loop_range(*args) == -1                              # known without mask
    args[11], args[12] = None, mk.data_ptr()
    assert lib.afm_cmdm_cfg2_loop_range(*args) == -1                              # mask without known
    args[12], args[10] = None, None
    assert lib.afm_cmdm_cfg2_loop_range(*args) == -1                              # no afm_cfg2_args
    for bad in (ffi.Cfg2Args(p, None, 1, 0), ffi.Cfg2Args(None, p, 1, 0), ffi.Cfg2Args(p, p, 2, 0)):
        args[10] = ctypes.byref(bad)
        assert lib.afm_cmdm_cfg2_loop_range(*args) == -1                          # a scale row missing; `first` neither 0 nor 1


# ---------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("tt", [999, 500, 0])
def test_goldens_are_self_consistent(tt):
    single = golden(f"cmdm_cfg_forward_both_t{tt}")
    for tag, order in ORDERS.items():
        g = golden(f"cmdm_cfg2_forward_{tag}_t{tt}")
        s1, s2 = scale_rows(order)
        assert torch.equal(g["scale_first"], s1) and torch.equal(g["scale_second"], s2) and g["guided"].dtype == torch.float32
        assert torch.equal(g["guided"], combine2(g["x0_c"], g["x0_a"], g["x0_u"], s1, s2)), tag
        assert torch.equal(g["x0_c"], single["x0_c"]) and torch.equal(g["x0_u"], single["x0_u"])
        # the middle branch is the single-scale goldens' partial drop of the second condition
        assert torch.equal(g["x0_a"], golden(f"cmdm_cfg_forward_{order[1]}_t{tt}")["x0_u"])
        # the synthetic weights do exercise both guidance terms
        for p, q in (("x0_c", "x0_a"), ("x0_a", "x0_u"), ("x0_c", "x0_u")):
            assert (g[p] - g[q]).abs().max() > 0.05, (tag, p, q)
    a, b = (golden(f"cmdm_cfg2_forward_{tag}_t{tt}") for tag in ORDERS)
    assert (a["guided"] - b["guided"]).abs().max() > 0.05          # the order of the mapping matters


def test_loop_goldens_are_self_consistent():
    known, mask = impute_known(), impute_mask()
    plain, clip, imp = (golden(f"cmdm_cfg2_loop_{tag}")["sample"] for tag in ("r5", "r5_clip", "impute_r5"))
    assert (plain - clip).abs().max() > 1e-2                        # the clamp is live
    assert torch.equal(imp[mask], known[mask]) and not torch.equal(imp[~mask], plain[~mask])
    assert (plain - golden("cmdm_cfg_loop_r5")["sample"]).abs().max() > 1e-2       # not the single-scale loop
    e0, e1 = (golden(f"cmdm_cfg2_ddim_loop_ddim50_eta{e}")["sample"] for e in (0, 1))
    assert torch.isfinite(e0).all() and torch.isfinite(e1).all() and not torch.equal(e0, e1)


@pytest.mark.parametrize("tt", [999, 500, 0])
def test_composed_oracle_reproduces_the_forward_goldens(tt):
    g, sd = _case()
    for tag, order in ORDERS.items():
        gg = golden(f"cmdm_cfg2_forward_{tag}_t{tt}")
        out = guided2_oracle(sd, g, order)(g["x"], torch.tensor([tt, tt]))
        assert _err(f"composed oracle forward t={tt} {tag}", out, gg["guided"]) <= BOUND_FWD


def test_composed_oracle_reproduces_the_p_sample_golden():
    g, sd = _case()
    gs = golden("cmdm_cfg2_p_sample_t500")
    out = df.p_sample(df.Schedule(1000), guided2_oracle(sd, g, ORDERS["pc_text"]), g["x"], torch.tensor([500, 500]),
                      synth.gaussian("p_sample_noise_500", SHAPE))
    assert _err("composed oracle p_sample pred_xstart", out["pred_xstart"], gs["pred_xstart"]) <= BOUND_FWD
    assert _err("composed oracle p_sample sample", out["sample"], gs["sample"]) <= BOUND_PSAMPLE


@pytest.mark.parametrize("tag", ["r5", "r5_clip", "impute_r5"])
def test_composed_oracle_reproduces_the_ddpm_loop_goldens(tag):
    g, sd = _case()
    s = df.Schedule(1000, "cosine", "5")
    xT, nz = loop_inputs("loop_r5", s.num_timesteps)
    model = guided2_oracle(sd, g, ORDERS["pc_text"])
    if tag == "impute_r5":
        model = imputed(model)
    out = df.p_sample_loop(s, model, xT, nz, clip_denoised=tag == "r5_clip")
    assert _err(f"composed oracle DDPM loop {tag}", out, golden(f"cmdm_cfg2_loop_{tag}")["sample"]) <= BOUND_LOOP[tag]


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_composed_oracle_reproduces_the_ddim_loop_goldens(eta):
    g, sd = _case()
    xT, nz = loop_inputs("ddim_loop_ddim50", 50)
    out = ddim_loop_ref(guided2_oracle(sd, g, ORDERS["pc_text"]), xT, nz, eta)
    assert _err(f"composed oracle DDIM loop eta={eta}", out, golden(f"cmdm_cfg2_ddim_loop_ddim50_eta{int(eta)}")["sample"]) <= BOUND_DDIM[eta]


# Measured on the CPU (beside each bound); a bound is at most 20x its measurement and never above the project's ceiling: 2e-5 for a forward
# or p_sample, 1e-4 for a loop (tests/test_oracle_golden.py), each times AMP (tests/test_cfg_host.py).
BOUND_FWD = 2e-5 * AMP             # forwards 2.4e-5 (pc first), 2.5e-5 (text first), p_sample pred_xstart 2.3e-5: 20x is above the ceiling, so the ceiling
BOUND_PSAMPLE = 4.8e-6             # 2.4e-7 (coef1 is small at t = 500)
BOUND_LOOP = {"r5": 5.9e-4,        # 3.0e-5
              "r5_clip": 5.3e-4,   # 2.7e-5
              "impute_r5": 7.2e-4} # 3.6e-5
BOUND_DDIM = {0.0: 6.2e-4,         # 3.1e-5
              1.0: 6.8e-4}         # 3.4e-5
assert max(BOUND_FWD, BOUND_PSAMPLE) <= 2e-5 * AMP and all(b <= 1e-4 * AMP for b in list(BOUND_LOOP.values()) + list(BOUND_DDIM.values()))


# ---------------------------------------------------------------------------------------------------------------- errors, loud
def test_wrapper_takes_a_mapping_and_refuses_what_it_cannot_do():
    m = _model()
    w = GuidedCMDM(m, {"pc": 1.5, "text": 5.0}, force_masked=True)
    assert w.order == ("pc", "text") and w.drop == ("pc", "text") and w.motion_dim == 263
    cfg = w._cfg(2, torch.device("cpu"))
    assert isinstance(cfg, ffi.Cfg2Args) and (cfg.first, cfg.flags) == (1, ffi.CFG_FORCE_MASKED)
    assert w._scale_row("pc", 2, "cpu").tolist() == [1.5, 1.5] and w._scale_row("text", 2, "cpu").tolist() == [5.0, 5.0]
    cfg = GuidedCMDM(m, {"text": torch.tensor([2.5, 7.5]), "pc": 1.5})._cfg(2, torch.device("cpu"))
    assert (cfg.first, cfg.flags) == (0, 0)
    for bad in ({"text": 2.5}, {"pc": 1.5}, {}, {"text": 2.5, "pc": 1.5, "scene": 1.0}, {"text": 2.5, "scene": 1.0}):
        with pytest.raises(ValueError, match="exactly the keys"):
            GuidedCMDM(m, bad)
    for drop in ("text", ("pc",)):
        with pytest.raises(ValueError, match="`drop` stays at its default"):
            GuidedCMDM(m, {"pc": 1.5, "text": 5.0}, drop=drop)
    with pytest.raises(ValueError, match="branch streams"):
        GuidedCMDM(m, {"pc": 1.5, "text": 5.0}, branch_streams=True)
    with pytest.raises(ValueError, match="scale"):
        GuidedCMDM(m, {"pc": 1.5, "text": torch.ones(2, 2)})
    with pytest.raises(ValueError, match="scale"):
        GuidedCMDM(m, {"pc": torch.ones(2, dtype=torch.int64), "text": 5.0})
    w = GuidedCMDM(m, {"pc": 1.5, "text": torch.tensor([2.5, 7.5, 1.0])})
    with pytest.raises(ValueError, match=r"scale\['text'\]` holds 3 values for a batch of 2"):
        w._cfg(2, torch.device("cpu"))
    with pytest.raises(ValueError, match="3 values for a batch of 2"):           # at call time, before anything runs
        w.afm_native_loop(create_gaussian_diffusion(_cfg()), torch.zeros(SHAPE), {"x_mask": torch.zeros(2, 16, dtype=torch.bool)})
    # what the single-scale wrapper refuses stays refused
    with pytest.raises(ValueError, match="mask_motion"):
        GuidedCMDM(_model(mask_motion=False), {"pc": 1.5, "text": 5.0})
    with pytest.raises(NotImplementedError, match="trans_enc"):
        GuidedCMDM(_model(arch="trans_dec"), {"pc": 1.5, "text": 5.0})
    w = GuidedCMDM(m, {"pc": 1.5, "text": 5.0})
    kw = {"c_pc_mask": torch.ones(2, 1, dtype=torch.bool), "x_mask": torch.zeros(2, 16, dtype=torch.bool)}
    with pytest.raises(ValueError, match="c_pc_mask"):
        w(torch.zeros(SHAPE), torch.tensor([1, 2]), **kw)
    with pytest.raises(ValueError, match="c_pc_mask"):
        w.afm_native_loop(create_gaussian_diffusion(_cfg()), torch.zeros(SHAPE), kw)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        w(torch.zeros(SHAPE), torch.tensor([1, 2]), x_mask=kw["x_mask"])


def test_two_stage_sample_refuses_a_contradictory_guidance_drop():
    from afm.pipeline import two_stage_sample
    m = _model()
    args = dict(text_feat=torch.zeros(2, 512), xyz=torch.zeros(2, 1024, 3), frames=16)
    for drop in (("text",), "pc", ()):
        with pytest.raises(ValueError, match="contradicts"):                     # before the first stage runs
            two_stage_sample(None, None, m, None, guidance_scale={"pc": 1.5, "text": 5.0}, guidance_drop=drop, **args)
