"""DPM-Solver++(2M) in the CDM's native loops, on the host (no GPU): the C ABI declares and exports the two new entries and refuses NULL
rows and a `known` without a `mask`; `dpm_solver_sample_loop` reaches the CDM's `afm_native_loop` with ``dpm_order=``, under the conditions
of every native loop.  The float32 / float64 twins of the loop - the 2M update restated
around the CPU oracle's CDM - are built here for tests/test_gpu_cdm_dpm.py to import.

    x_next = a x_t + b x0                       the first executed step (no history)
    x_next = (a x_t + b x0) + c x0_prev         x0 / x0_prev: the final predictions (after the imputation select and the clamp)"""
import ctypes
import functools
import os
import re

import pytest
import torch

from afm import ffi
from conftest import ROOT
from test_cdm_impute_host import (SHAPE, _NarrowRecorder, _Recorder, check_one_native_loop, contact_known, contact_mask, imputed, loop_inputs,
                                  oracle_cdm, samples_step_by_step)
from test_ddim_host import _diffusion

ENTRY, SIZER = "afm_cdm_dpm_loop_range", "afm_cdm_dpm_loop_workspace_bytes"
CASES = {"plain": (False, False), "clip": (False, True), "impute": (True, False), "impute+clip": (True, True)}      # name -> (Impute, clip_denoised)


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entries_are_declared_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert {ENTRY, SIZER} <= declared and {ENTRY, SIZER} <= set(ffi.EXPORTS)
    assert "#define AFM_ABI_VERSION 7" in hdr and ffi.ABI_VERSION == 7           # additive: the version stays
    # the arguments of afm_cdm_ddim_loop_range: the 2M rows for the DDIM rows, no step noise and no seed, known and mask behind the rows
    ddim, dpm = ffi.EXPORTS["afm_cdm_ddim_loop_range"][1], ffi.EXPORTS[ENTRY][1]
    assert dpm[:6] == ddim[:6] and dpm[6] == ddim[7] and dpm[7] is ctypes.POINTER(ffi.DpmRows) and dpm[10:12] == ddim[9:11]
    assert dpm[12:] == ddim[13:] and len(dpm) == len(ddim) - 3 + 2
    assert ffi.EXPORTS[SIZER] == ffi.EXPORTS["afm_cdm_loop_workspace_bytes"]
    proto = re.search(r"int\s+" + ENTRY + r"\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(dpm) and "const afm_dpm_rows* rows, const float* known" in proto and "const uint8_t* mask" in proto
    assert "step_noise" not in proto and "seed" not in proto and "afm_ddpm_args" not in proto
    sizer = re.search(r"int64_t\s+" + SIZER + r"\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(sizer.split(",")) == 4
    if os.path.exists(ffi.lib_path()):
        lib = ctypes.CDLL(ffi.lib_path())
        assert hasattr(lib, ENTRY) and hasattr(lib, SIZER) and ffi.load().afm_version() == 7


def test_entry_refuses_null_rows_and_a_known_without_a_mask():
    """AFM_E_BADARG in front of every other check (no GPU needed: nothing is looked at or launched)."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    buf, mk = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    rows = ffi.DpmRows(buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    args = [None] * 20
    args[10:14] = [1, 0, 2, 4]                    # n_steps, first_step, B, N
    args[16], args[17] = 0, 0                     # workspace_bytes, n_sub
    assert getattr(lib, ENTRY)(*args) == -1       # NULL rows
    args[7] = ctypes.byref(ffi.DpmRows(buf.data_ptr(), None, buf.data_ptr()))
    assert getattr(lib, ENTRY)(*args) == -1       # a NULL row
    args[7] = ctypes.byref(rows)
    for known, mask in ((buf.data_ptr(), None), (None, mk.data_ptr())):
        args[8], args[9] = known, mask
        assert getattr(lib, ENTRY)(*args) == -1
    args[8], args[9] = buf.data_ptr(), mk.data_ptr()
    assert getattr(lib, ENTRY)(*args) == -1       # both: the ordinary checks (no weights)
    args[8], args[9] = None, None
    assert getattr(lib, ENTRY)(*args) == -1       # neither: the same
    args[11] = -1
    assert getattr(lib, ENTRY)(*args) == -1       # a negative first_step
    assert getattr(lib, SIZER)(None, 2, 4, 0) == -1


def test_python_surface():
    from afm.diffusion import GaussianDiffusion
    from afm.pipeline import two_stage_sample
    check_one_native_loop()
    doc = two_stage_sample.__doc__
    assert "normalised contact" in doc and "afm_cdm_dpm_loop_range" in doc and "no native form" not in doc
    assert "never the CDM" not in GaussianDiffusion._sample_loop.__doc__


def test_dpm_solver_sample_loop_hands_the_order_to_the_native_loop(monkeypatch):
    from afm.diffusion import Impute
    d, seeds = _diffusion(500, "ddim5"), _diffusion(500, "ddim5")
    shape = (2, 4, 6)
    imp = Impute(torch.zeros(shape), torch.ones(shape, dtype=torch.bool))
    xT = torch.zeros(shape)
    m = _Recorder()
    snaps = {1: None}
    d.dpm_solver_sample_loop(m, shape, noise=xT, clip_denoised=True, denoised_fn=imp, seed=3, sample_index0=5)
    d.dpm_solver_sample_loop(m, shape, noise=xT, clip_denoised=False, order=1, seed=4, progress=False, snapshots=snaps)
    d.ddim_sample_loop(m, shape, noise=xT, clip_denoised=False, eta=0.0)          # the other samplers go where they went
    d.p_sample_loop(m, shape, noise=xT, clip_denoised=False, denoised_fn=imp)
    s = [seeds._fresh_seed("_sample_calls") for _ in range(2)]                  # no seed given: the diffusion's own, call by call
    assert m.calls == [(imp, True, None, 2, 3, 5, False, None, True), (None, False, None, 1, 4, 0, False, snaps, True),
                       (None, False, 0.0, None, s[0], 0, False, None, True), (imp, False, None, None, s[1], 0, False, None, True)]
    with pytest.raises(ValueError):               # impute.check(x) first
        d.dpm_solver_sample_loop(m, (2, 5, 6), noise=torch.zeros(2, 5, 6), denoised_fn=imp)
    assert len(m.calls) == 4
    # a plain callable, rescale_timesteps, a condition switch, and a denoiser whose loop does not name ``dpm_order`` - with and without an
    # Impute - sample step by step
    rescaled = _diffusion(500, "ddim5")
    rescaled.rescale_timesteps = True
    switch = dict(c_text_mask=torch.zeros(2, 1, dtype=torch.bool))
    for diff, model, fn, kw in ((d, _Recorder(), lambda x0: x0, None), (rescaled, _Recorder(), None, None), (d, _Recorder(), None, switch),
                                (d, _NarrowRecorder(), imp, None), (d, _NarrowRecorder(), None, None)):
        samples_step_by_step(monkeypatch, model, lambda: diff.dpm_solver_sample_loop(model, shape, noise=xT, clip_denoised=False, denoised_fn=fn,
                                                                                     model_kwargs=kw))


def test_only_the_perceiver_cdm_has_the_native_loop(monkeypatch):
    """a non-Perceiver CDM has no native loop, so dpm_solver_sample_loop drives its forward step by step; the Perceiver's names both
    keywords"""
    from afm import base
    from afm.config import load_config
    from afm.diffusion import _takes
    cfg = lambda *extra: load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.scene_model.use_scene_model=False", *extra])
    for arch in ("MLP", "PointTrans"):
        m = base.create_model(cfg(f"model.arch={arch}", "task.dataset.num_points=1024"), device="cpu")
        assert m.arch == arch and m.afm_native_loop is None
        samples_step_by_step(monkeypatch, m, lambda: _diffusion(500, "ddim5").dpm_solver_sample_loop(m, (1, 1024, 6), noise=torch.zeros(1, 1024, 6),
                                                                                                     clip_denoised=False))
    p = base.create_model(cfg("model.arch=Perceiver"), device="cpu")
    assert callable(p.afm_native_loop) and _takes(p.afm_native_loop, "impute") and _takes(p.afm_native_loop, "dpm_order")


# ---------------------------------------------------------------------------------------------------------------- the twins
def dpm_loop_ref(model, x_T, order=2, clip_denoised=False, respacing="ddim5"):
    """dpm_solver_sample_loop at ``respacing`` of T = 500 on the CPU around ``model``: the product's float32 rows, promoted with x_T (in
    float64 when x_T is), one rounded operation at a time."""
    d = _diffusion(500, respacing)
    tab, tmap = d.dpm_tables("cpu", order), torch.tensor(d.timestep_map)
    a, b, c = (r.to(x_T.dtype) for r in (tab.a, tab.b, tab.c))
    img, prev = x_T, None
    with torch.no_grad():
        for i in range(d.num_timesteps - 1, -1, -1):
            x0 = model(img, tmap[torch.tensor([i] * x_T.shape[0])])
            if clip_denoised:
                x0 = x0.clamp(-1, 1)
            two = a[i] * img + b[i] * x0
            img = two if prev is None else two + c[i] * prev
            prev = x0
    return img


def twin_x_T():
    return loop_inputs("cdm_dpm_loop", 0)[0]


@functools.lru_cache(maxsize=None)
def twin(case, f64):
    """The 2M loop ("ddim5" of T = 500, order 2) around the oracle's CDM on the goldens' scene, with the select of
    tests/test_cdm_impute_host.py in the imputing cases: float32, or its float64 twin.  Computed once per process and shared."""
    with_imp, clip = CASES[case]
    model = oracle_cdm(f64=f64)
    if with_imp:
        model = imputed(model)
    xT = twin_x_T()
    return dpm_loop_ref(model, xT.double() if f64 else xT, clip_denoised=clip)


def test_twins_keep_the_known_values_and_the_history_term_is_live():
    known, mask = contact_known(), contact_mask()
    assert (known[mask].abs() > 1).any()                                         # the clip case tests the order: select, then clamp
    for case, (with_imp, clip) in CASES.items():
        w32, w64 = twin(case, False), twin(case, True)
        assert w32.dtype == torch.float32 and w64.dtype == torch.float64 and w32.shape == SHAPE and torch.isfinite(w64).all()
        if with_imp:                              # the last row is (0, 1, 0): the sample is the final pred_xstart
            assert torch.equal(w32[mask], (known.clamp(-1, 1) if clip else known)[mask])
            assert torch.equal(w64[mask], (known.double().clamp(-1, 1) if clip else known.double())[mask])
        else:
            assert not torch.equal(w32[mask], known[mask])
        err = (w32.double() - w64).abs().max().item()
        print(f"[cdm dpm host] {case}: float32 oracle vs float64 twin {err:.3e} (max|ref| = {w64.abs().max().item():.3e})")
        assert err <= 1e-4                        # (1.3e-5 .. 2.7e-5 on the machines it ran on; the GPU test takes 4 x this figure as its bound)
    first = dpm_loop_ref(oracle_cdm(), twin_x_T(), order=1)
    assert not torch.equal(first, twin("plain", False))
