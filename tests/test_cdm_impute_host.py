"""Imputation of known contact values in the CDM's native loops, on the host (no GPU): the C ABI declares and exports the new entry and
refuses a `known` without a `mask`; the Python surface is the one native loop with ``impute=`` and `contact_impute`; the reference goldens
(tools/make_goldens_cdm_impute.py) are self-consistent; the CPU oracle's CDM wrapped with the same select reproduces them.  The float64
twins of those loops are built here for tests/test_gpu_cdm_impute.py to import."""
import ctypes
import functools
import inspect
import os
import re

import pytest
import torch

from afm import ffi, synth
from oracle import denoiser_ref as dr
from oracle import diffusion_ref as df
from oracle import shapes as sh

from conftest import ROOT, golden
from test_ddim_host import _diffusion, _update

ENTRY = "afm_cdm_impute_loop_range"
SHAPE = (2, 256, 6)
DDPM_LOOPS = {"r5": False, "r5_clip": True}               # golden tag -> clip_denoised, respacing "5" of T = 500
DDIM_LOOPS = {"eta05": 0.5, "eta0": 0.0}                  # golden tag -> eta, respacing "ddim5" of T = 500


def contact_mask():
    """The mask of tools/make_goldens_cdm_impute.py, restated: sample 0 pins every joint on the points 0..95 (a chosen object), sample 1
    pins joints 0 and 3 on every point and every joint on the points 200..255 (a region to keep clear)."""
    m = torch.zeros(SHAPE, dtype=torch.bool)
    m[0, 0:96, :] = True
    m[1, :, 0] = True
    m[1, :, 3] = True
    m[1, 200:256, :] = True
    return m


def contact_known():
    return synth.gaussian("cdm_impute_known", SHAPE)


def imputed(model, known=None, mask=None):
    """a denoiser with the select behind it, in the dtype of its output"""
    known = contact_known() if known is None else known
    mask = contact_mask() if mask is None else mask
    return lambda x, t, **kw: (lambda o: torch.where(mask, known.to(o.dtype), o))(model(x, t, **kw))


def oracle_cdm(f64=False):
    """the oracle's CDM Perceiver on the goldens' case (text and scene of cdm_forward_N256), float32 or its float64 twin"""
    from gpu_util import to_f64
    g, sd = golden("cdm_forward_N256"), sh.weights(sh.cdm())
    if f64:
        g, sd = to_f64(g), to_f64(sd)
    return lambda x, t, **kw: dr.cdm_forward(sd, x, t, g["text_feat"], g["xyz"])


def ddim_loop_ref(model, x_T, step_noise, eta, clip_denoised=False):
    """ddim_sample_loop at respacing "ddim5" of T = 500 on the CPU: the update expression of tests/test_ddim_host.py around ``model``; in
    float64 when x_T is."""
    d = _diffusion(500, "ddim5")
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


def p_sample_inputs():
    g = golden("cdm_forward_N256")
    return g["x"], g["t"], synth.gaussian("cdm_impute_p_sample_noise", SHAPE)


def _err(name, got, want):
    err = (got.double() - want.double()).abs().max().item()
    print(f"[cdm impute host] {name}: max|diff| = {err:.3e} (max|ref| = {want.abs().max().item():.3e})")
    return err


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entry_is_declared_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert ENTRY in declared and ENTRY in ffi.EXPORTS
    assert "#define AFM_ABI_VERSION 7" in hdr and ffi.ABI_VERSION == 7           # additive: the version stays
    # the arguments of afm_cdm_ddim_loop_range with the three DDPM rows, known and mask behind `rows`
    ddim, samp, imp = (ffi.EXPORTS[n][1] for n in ("afm_cdm_ddim_loop_range", "afm_cdm_sample_loop_range", ENTRY))
    assert imp[:9] == ddim[:9] and imp[9:12] == samp[8:11] and imp[14:] == ddim[9:] and len(imp) == len(ddim) + 5
    proto = re.search(r"int\s+" + ENTRY + r"\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(imp) and "const float* known, const uint8_t* mask" in proto
    assert "afm_ddpm_args" not in proto
    if os.path.exists(ffi.lib_path()):
        assert hasattr(ctypes.CDLL(ffi.lib_path()), ENTRY) and ffi.load().afm_version() == 7


def test_entry_refuses_a_known_without_a_mask():
    """AFM_E_BADARG in front of every other check (no GPU needed: nothing is looked at or launched)."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    buf, mk = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    args = [None] * 26
    args[14:20] = [1, 0, 0, 0, 2, 4]              # n_steps, first_step, seed, sample_index0, B, N
    args[22], args[23] = 0, 0                     # workspace_bytes, n_sub
    for known, mask in ((buf.data_ptr(), None), (None, mk.data_ptr())):
        args[12], args[13] = known, mask
        assert getattr(lib, ENTRY)(*args) == -1
    args[12], args[13] = buf.data_ptr(), mk.data_ptr()
    assert getattr(lib, ENTRY)(*args) == -1       # both: the ordinary checks (no weights)
    args[12], args[13] = None, None
    assert getattr(lib, ENTRY)(*args) == -1       # neither: the existing loop's checks


LOOP_PARAMS = ["self", "diffusion", "x", "model_kwargs", "step_noise", "seed", "sample_index0", "progress", "snapshots", "clip_denoised",
               "ddim_eta", "impute", "dpm_order"]
LOOP_DEFAULTS = dict(step_noise=None, seed=0, sample_index0=0, progress=False, snapshots=None, clip_denoised=False, ddim_eta=None, impute=None,
                     dpm_order=None)


def check_one_native_loop():
    """The CDM's native-loop surface (tests/test_cdm_dpm_host.py pins the same): one method with the CMDM's protocol, found by
    `_sample_loop` through its keywords, and no second or third one."""
    from afm.cdm import CDM
    from afm.cmdm import CMDM
    from afm.diffusion import GaussianDiffusion, _takes
    loop = inspect.signature(CDM.afm_native_loop).parameters
    assert list(loop) == LOOP_PARAMS                                             # the old eleven names, then impute, dpm_order
    for name in LOOP_PARAMS[:4]:
        assert loop[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and loop[name].default is inspect.Parameter.empty, name
    for name in LOOP_PARAMS[4:]:                  # everything after model_kwargs: keyword-only, with these defaults
        assert loop[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert repr(loop[name].default) == repr(LOOP_DEFAULTS[name]), name
    cmdm = {k: v for k, v in inspect.signature(CMDM.afm_native_loop).parameters.items() if k != "_guidance"}
    assert sorted(loop) == sorted(cmdm)
    for name, par in cmdm.items():                # name for name, kind for kind, default for default
        assert loop[name].kind is par.kind and repr(loop[name].default) == repr(par.default), name
    assert _takes(CDM.afm_native_loop, "impute") and _takes(CDM.afm_native_loop, "dpm_order")
    src = inspect.getsource(GaussianDiffusion._sample_loop)
    for gone in ("afm_native_impute_loop", "afm_native_dpm_loop"):
        assert not hasattr(CDM, gone) and gone not in src, gone


def test_python_surface():
    from afm.diffusion import Impute
    from afm.pipeline import two_stage_sample
    check_one_native_loop()
    ts = inspect.signature(two_stage_sample).parameters
    assert ts["contact_impute"].default is None and ts["motion_impute"].default is None
    assert "normalised contact" in two_stage_sample.__doc__ and "[B, N, J]" in Impute.__doc__


class _Recorder(torch.nn.Module):
    """a denoiser with the one native loop, recording what a sampling call hands it (tests/test_cdm_dpm_host.py imports it)"""
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, x, t, **kw):
        self.calls.append("forward")
        return x

    def afm_native_loop(self, diffusion, x, model_kwargs, *, step_noise=None, seed=0, sample_index0=0, progress=False, snapshots=None,
                        clip_denoised=False, ddim_eta=None, impute=None, dpm_order=None):
        self.calls.append((impute, clip_denoised, ddim_eta, dpm_order, seed, sample_index0, progress, snapshots, step_noise is None))
        return x


class _NarrowRecorder(_Recorder):
    """a denoiser whose native loop names neither ``impute`` nor ``dpm_order``"""
    def afm_native_loop(self, diffusion, x, model_kwargs, *, step_noise=None, seed=0, sample_index0=0, progress=False, snapshots=None,
                        clip_denoised=False, ddim_eta=None):
        self.calls.append("narrow loop")
        return x


class Stop(Exception):
    pass


def samples_step_by_step(monkeypatch, model, sample):
    """``sample()`` reaches the denoiser's forward (stopped there) and never its native loop"""
    def stop(*a, **k):
        raise Stop
    monkeypatch.setattr(model, "forward", stop)
    with pytest.raises(Stop):
        sample()
    assert getattr(model, "calls", []) == []


def test_sample_loop_hands_an_impute_to_the_native_loop(monkeypatch):
    from afm.diffusion import Impute
    d, seeds = _diffusion(500, "ddim5"), _diffusion(500, "ddim5")
    shape = (2, 4, 6)
    imp = Impute(torch.zeros(shape), torch.ones(shape, dtype=torch.bool))
    xT = torch.zeros(shape)
    m = _Recorder()
    d.p_sample_loop(m, shape, noise=xT, clip_denoised=True, denoised_fn=imp)
    d.ddim_sample_loop(m, shape, noise=xT, clip_denoised=False, denoised_fn=imp, eta=0.5)
    d.p_sample_loop(m, shape, noise=xT, clip_denoised=False)
    s = [seeds._fresh_seed("_sample_calls") for _ in range(3)]                  # no seed given: the diffusion's own, call by call
    assert m.calls == [(imp, True, None, None, s[0], 0, False, None, True), (imp, False, 0.5, None, s[1], 0, False, None, True),
                       (None, False, None, None, s[2], 0, False, None, True)]
    with pytest.raises(ValueError):               # impute.check(x) first
        d.p_sample_loop(m, (2, 5, 6), noise=torch.zeros(2, 5, 6), denoised_fn=imp)
    assert len(m.calls) == 3
    # any other callable, and an Impute on a denoiser whose loop does not name ``impute``, sample step by step
    for model, fn in ((_Recorder(), lambda x0: x0), (_NarrowRecorder(), imp)):
        samples_step_by_step(monkeypatch, model, lambda: d.p_sample_loop(model, shape, noise=xT, clip_denoised=False, denoised_fn=fn))
    narrow = _NarrowRecorder()                    # (which still samples natively without one)
    d.p_sample_loop(narrow, shape, noise=xT, clip_denoised=False)
    assert narrow.calls == ["narrow loop"]


def test_native_loop_refuses_early():
    """before anything touches the library: on CPU tensors"""
    from afm import base
    from afm.config import load_config
    from afm.diffusion import Impute
    cdm = base.create_model(load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.scene_model.use_scene_model=False",
                                                                                "model.arch=Perceiver"]), device="cpu")
    d, x, kw = _diffusion(500, "ddim5"), torch.zeros(2, 4, 6), {}
    with pytest.raises(ValueError, match="neither ddim_eta nor step_noise"):
        cdm.afm_native_loop(d, x, kw, dpm_order=2, ddim_eta=0.0)
    with pytest.raises(ValueError, match="neither ddim_eta nor step_noise"):
        cdm.afm_native_loop(d, x, kw, dpm_order=2, step_noise=torch.zeros(5, 2, 4, 6))
    with pytest.raises(ValueError, match="sample is"):
        cdm.afm_native_loop(d, x, kw, impute=Impute(torch.zeros(2, 5, 6), torch.ones(2, 5, 6, dtype=torch.bool)))


# ---------------------------------------------------------------------------------------------------------------- goldens
def test_goldens_are_self_consistent():
    """The last step writes pred_xstart into the sample unchanged (DDPM: c1 = 1, c2 = 0, sigma = 0; DDIM: c = 1, d = 0), so every chain
    ends on `known` where the mask is set - exactly, in the reference's float32 arithmetic."""
    known, mask = contact_known(), contact_mask()
    assert (known[mask].abs() > 1).any()                                         # the clip case tests the order: denoised_fn, then clamp
    assert 0 < mask[0].sum() < mask[0].numel() and mask[1, :, 0].all() and not mask[1, :199, 1].any()
    ps, plain = golden("cdm_impute_p_sample"), golden("cdm_forward_N256")
    assert ps["pred_xstart"].dtype == torch.float32 and torch.equal(ps["pred_xstart"][mask], known[mask])
    # untouched where nothing is known: the plain forward golden of the same inputs (made on another CPU: tests/test_oracle_golden.py's 2e-5)
    assert (ps["pred_xstart"][~mask] - plain["out"][~mask]).abs().max() <= 2e-5 and (ps["pred_xstart"][mask] - plain["out"][mask]).abs().max() > 1
    for tag, clip in DDPM_LOOPS.items():
        s = golden(f"cdm_impute_loop_{tag}")["sample"]
        assert torch.equal(s[mask], (known.clamp(-1, 1) if clip else known)[mask]) and torch.isfinite(s).all(), tag
    assert not torch.equal(golden("cdm_impute_loop_r5")["sample"][~mask], golden("cdm_impute_loop_r5_clip")["sample"][~mask])
    for tag, eta in DDIM_LOOPS.items():
        g = golden(f"cdm_impute_ddim_loop_ddim5_{tag}")
        assert float(g["eta"]) == eta and torch.equal(g["sample"][mask], known[mask]) and torch.isfinite(g["sample"]).all(), tag


@functools.lru_cache(maxsize=None)
def twin64(tag):
    """The float64 twin of a golden - the oracle's CDM with the select under the same loop, everything in float64 - computed once per process
    and shared (tests/test_gpu_cdm_impute.py imports it).  tag: "p_sample" (a dict), a DDPM_LOOPS tag or "ddim_" + a DDIM_LOOPS tag."""
    model = imputed(oracle_cdm(f64=True))
    if tag == "p_sample":
        x, t, nz = p_sample_inputs()
        return df.p_sample(df.Schedule(500), model, x.double(), t, nz.double())
    if tag in DDPM_LOOPS:
        xT, nz = loop_inputs("cdm_impute_loop", 5)
        return df.p_sample_loop(df.Schedule(500, "cosine", "5"), model, xT.double(), [z.double() for z in nz], clip_denoised=DDPM_LOOPS[tag])
    xT, nz = loop_inputs("cdm_impute_ddim_loop", 5)
    return ddim_loop_ref(model, xT.double(), [z.double() for z in nz], DDIM_LOOPS[tag[len("ddim_"):]])


def _reproduces(name, out, want32, want64):
    """The oracle runs the reference's own torch operators in the reference's order, so on the CPU that made the goldens it reproduces them
    bit for bit: measured 0 for all six goldens, at 1, 2, 4 and 16 threads.  Twenty times that measurement would be a bound of 0, which
    holds only on a CPU whose GEMM blocking and vector math library round like that one's (the CMDM figures of tests/test_impute_host.py
    move in their second digit between machines).  The bound is therefore the reference's own float32 error, by the project's rule for
    "the same float32 arithmetic in another association" (gpu_util.report_f32_class): against the float64 twin the oracle may err at
    most 4 x what the float32 golden itself errs, plus one float32 ulp of the largest output.  Measured: golden vs twin 2.7e-6 (p_sample)
    to 5.3e-6 (loops), i.e. bounds of 1.1e-5 to 2.2e-5, below the 2e-5 / 1e-4 ceilings of tests/test_oracle_golden.py's CDM tests."""
    assert want64.dtype == torch.float64 and out.dtype == torch.float32
    direct = _err(f"{name}: oracle vs golden", out, want32)
    e_ref, e_got = _err(f"{name}: golden vs float64 twin", want32, want64), _err(f"{name}: oracle vs float64 twin", out, want64)
    bound = 4.0 * e_ref + 2.0 ** -23 * want64.abs().max().item()
    assert e_got <= bound and direct <= e_got + e_ref, (name, direct, e_got, bound)


def test_oracle_with_the_select_reproduces_the_p_sample_golden():
    x, t, nz = p_sample_inputs()
    ps, w64 = golden("cdm_impute_p_sample"), twin64("p_sample")
    out = df.p_sample(df.Schedule(500), imputed(oracle_cdm()), x, t, nz)
    assert torch.equal(out["pred_xstart"][contact_mask()], ps["pred_xstart"][contact_mask()])
    for k in ("pred_xstart", "sample"):
        _reproduces(f"p_sample {k}", out[k], ps[k], w64[k])


@pytest.mark.parametrize("tag", list(DDPM_LOOPS))
def test_oracle_with_the_select_reproduces_the_ddpm_loop_goldens(tag):
    s = df.Schedule(500, "cosine", "5")
    xT, nz = loop_inputs("cdm_impute_loop", s.num_timesteps)
    out = df.p_sample_loop(s, imputed(oracle_cdm()), xT, nz, clip_denoised=DDPM_LOOPS[tag])
    _reproduces(f"DDPM loop {tag}", out, golden(f"cdm_impute_loop_{tag}")["sample"], twin64(tag))


@pytest.mark.parametrize("tag", list(DDIM_LOOPS))
def test_oracle_with_the_select_reproduces_the_ddim_loop_goldens(tag):
    xT, nz = loop_inputs("cdm_impute_ddim_loop", 5)
    out = ddim_loop_ref(imputed(oracle_cdm()), xT, nz, DDIM_LOOPS[tag])
    _reproduces(f"DDIM loop {tag}", out, golden(f"cdm_impute_ddim_loop_ddim5_{tag}")["sample"], twin64("ddim_" + tag))


def test_float64_twins_keep_the_known_values():
    """the twins the GPU tests import: float64, and `known` (clamped where the loop clips) under the mask"""
    known, mask = contact_known().double(), contact_mask()
    for tag in list(DDPM_LOOPS) + ["ddim_" + t for t in DDIM_LOOPS]:
        w = twin64(tag)
        assert w.dtype == torch.float64 and torch.equal(w[mask], (known.clamp(-1, 1) if tag == "r5_clip" else known)[mask]), tag
    assert torch.equal(twin64("p_sample")["pred_xstart"][mask], known[mask])
