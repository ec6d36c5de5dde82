"""`-m gpu`: DPM-Solver++(2M) sampling (dpm_solver_sample / dpm_solver_sample_loop, afm_dpm_step, afm_cmdm_dpm_loop_range): the update
kernel against the CPU float32 expression (bit for bit), the native CMDM loop in every form against the step-by-step loop (bit for bit)
and against the loop restated around the CPU oracle, the solver's order on an ideal denoiser on the device, the pipeline, the refusals.

    x_next = a x_t + b x0                       no history (first executed step; callers without prev_xstart)
    x_next = (a x_t + b x0) + c x0_prev         x0 / x0_prev: the final predictions (after guidance, imputation, clamp)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.diffusion import Impute
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report, report_f32_class
from test_gpu_cdm import cdm_cfg
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _check, _device_kernel_names
from test_impute_host import oracle_model

pytestmark = pytest.mark.gpu
SHAPE = (2, 16, 263)
ODD = (2, 15, 263)          # 3945 values per sample: the update's last quad and its K-padded row copy end on a partial quad
D = lambda t: t.to(dev())


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def _last(gen):
    out = None
    for out in gen:
        pass
    return out["sample"]


def _diffusion(resp="ddim5", schedule="cosine"):
    cfg = cmdm_cfg(steps=1000, respacing=resp)
    cfg.diffusion.noise_schedule = schedule
    return create_gaussian_diffusion(cfg)


def _cpu_update(x0, x, prev, tab, t):
    """the float32 torch expression, one rounded operation at a time, on the product's float32 rows of timestep index t"""
    a, b, c = (r.cpu()[t] for r in (tab.a, tab.b, tab.c))
    two = a * x + b * x0
    return two if prev is None else two + c * prev


# ---------------------------------------------------------------------------------------------------------------- the kernel, exact
@pytest.mark.parametrize("resp", ["ddim5", "logsnr20"])
@pytest.mark.parametrize("shape", [SHAPE, (3, 5, 263)])          # (3, 5, 263): 1315 values per sample, the last quad is partial
def test_dpm_step_kernel_equals_the_cpu_expression(resp, shape):
    d = _diffusion(resp)
    n = d.num_timesteps
    x0, x, prev = (synth.gaussian(f"dpm_step_{k}_{shape[0]}", shape) for k in ("x0", "x", "prev"))
    for order in (1, 2):
        tab = d.dpm_tables(dev(), order)
        for tt in (n - 1, n // 2, 1, 0):
            t = torch.full((shape[0],), tt, device=dev())
            rows = (tab.a[t], tab.b[t], tab.c[t])
            for pv in (None, prev):
                want = _cpu_update(x0, x, pv, tab, tt)
                got = ops.dpm_step(D(x0), D(x), None if pv is None else D(pv), *rows)
                assert torch.equal(got.cpu(), want), (resp, shape, order, tt, pv is None)
                xt = D(x).clone()                            # out aliasing x_t: one thread reads then writes an element
                assert ops.dpm_step(D(x0), xt, None if pv is None else D(pv), *rows, out=xt) is xt and torch.equal(xt.cpu(), want)
    # rows per sample: every sample at a timestep of its own
    t = torch.tensor([n - 1, 1, 0][:shape[0]], device=dev())
    tab = d.dpm_tables(dev(), 2)
    got = ops.dpm_step(D(x0), D(x), D(prev), tab.a[t], tab.b[t], tab.c[t]).cpu()
    for b, tt in enumerate(t.tolist()):
        assert torch.equal(got[b], _cpu_update(x0[b], x[b], prev[b], tab, tt))


# ---------------------------------------------------------------------------------------------------------------- loops, native = step by step
def _impute(shape):
    """a prefix mask: the first five frames of every sample are known"""
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[:, :5, :] = True
    return Impute(D(synth.gaussian(f"dpm_impute_known_L{shape[1]}", shape)), D(mask))


def _kw_for(shape, g):
    if shape == SHAPE:
        return _kw(g)
    B, L = shape[0], shape[1]
    return dict(c_text_feat=D(g["text_feat"]), c_cont_emb=D(g["cont_emb"]), x_mask=D(synth.frame_mask(B, L, min_len=8)))


FORMS = {                   # name -> (guidance scale or None, clip_denoised, impute)
    "plain": (None, False, False),
    "clip": (None, True, False),
    "impute": (None, False, True),
    "guided": (2.5, False, False),
    "guided2": ({"pc": 1.5, "text": 5.0}, False, False),
    "guided+impute+clip": (2.5, True, True),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", [SHAPE, ODD])
def test_native_loop_equals_the_step_by_step_loop(cmdm, form, shape):
    """"ddim5": one two-term step, three three-term steps and the final step.  The same kernels must give the same bits."""
    scale, clip, imp = FORMS[form]
    d = _diffusion("ddim5")
    g = golden("cmdm_forward_N1024_L16")
    model = cmdm if scale is None else GuidedCMDM(cmdm, scale)
    xT = D(synth.gaussian(f"dpm_loop_xT_L{shape[1]}", shape))
    if clip:
        xT = 2.0 * xT
    args = dict(noise=xT, clip_denoised=clip, denoised_fn=_impute(shape) if imp else None, model_kwargs=_kw_for(shape, g))
    native = d.dpm_solver_sample_loop(model, shape, **args)
    assert torch.isfinite(native).all()
    outs = list(d.dpm_solver_sample_loop_progressive(model, shape, **args))
    report(f"CMDM 2M native vs step by step, {form} L={shape[1]}", native, outs[-1]["sample"], 0.0)
    if imp:
        m, known = args["denoised_fn"].mask.bool(), args["denoised_fn"].known
        known = known.clamp(-1, 1) if clip else known                            # (the select comes before the clamp)
        assert torch.equal(native[m], known[m])                                  # the last step returns the final pred_xstart
    if form in ("plain", "guided") and shape == SHAPE:
        assert torch.equal(native, d.dpm_solver_sample_loop(model, shape, progress=True, **args))
        snaps = {1: None, 4: None}
        assert torch.equal(native, d.dpm_solver_sample_loop(model, shape, snapshots=snaps, **args))
        assert torch.equal(snaps[1], outs[0]["sample"]) and torch.equal(snaps[4], outs[3]["sample"])
        first = d.dpm_solver_sample_loop(model, shape, order=1, **args)      # the history term is live: order 1 differs
        assert not torch.equal(first, native)
        assert torch.equal(first, _last(d.dpm_solver_sample_loop_progressive(model, shape, order=1, **args)))


@pytest.mark.parametrize("form", ["plain", "guided"])
def test_sub_batch_streams_are_bit_identical(cmdm, form):
    d = _diffusion("ddim5")
    B, L = 3, 16
    kw = dict(c_text_feat=D(synth.text_feature(B)), c_cont_emb=D(synth.gaussian("dpm_streams_cont", (B, 16, 256))),
              x_mask=D(synth.frame_mask(B, L, min_len=8)))
    model = cmdm if form == "plain" else GuidedCMDM(cmdm, 2.5)
    run = lambda: d.dpm_solver_sample_loop(model, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=4).clone()
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto = 1, False
        one = run()
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
        two = run()
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    assert torch.isfinite(one).all() and torch.equal(one, two)
    assert torch.equal(one, _last(d.dpm_solver_sample_loop_progressive(model, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=4)))


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def _loop_ref(model, x_T, tab, tmap):
    """the 2M loop restated around a CPU denoiser, in the dtype of x_T (the product's float32 rows, promoted with it)"""
    n = tmap.shape[0]
    a, b, c = (r.cpu().to(x_T.dtype) for r in (tab.a, tab.b, tab.c))
    img, prev = x_T, None
    with torch.no_grad():
        for i in range(n - 1, -1, -1):
            x0 = model(img, tmap[torch.tensor([i] * x_T.shape[0])])
            two = a[i] * img + b[i] * x0
            img = two if prev is None else two + c[i] * prev
            prev = x0
    return img


def test_native_loop_vs_the_oracle(cmdm):
    d = _diffusion("ddim5")
    g = golden("cmdm_forward_N1024_L16")
    xT = synth.gaussian("dpm_loop_xT_L16", SHAPE)
    native = d.dpm_solver_sample_loop(cmdm, SHAPE, noise=D(xT), clip_denoised=False, model_kwargs=_kw(g))
    tab, tmap = d.dpm_tables(dev(), 2), torch.tensor(d.timestep_map)
    want32 = _loop_ref(oracle_model(False), xT, tab, tmap)
    want64 = _loop_ref(oracle_model(False, f64=True), xT.double(), tab, tmap)
    report("CMDM 2M native loop ddim5 vs oracle", native, want32, 1e-3)
    report_f32_class("CMDM 2M native loop ddim5 vs oracle", native, want32, want64, old_tol=1e-3, margin=4.0)


# ---------------------------------------------------------------------------------------------------------------- the solver on the device
class IdealDenoiser(nn.Module):
    """E[x0 | x_t] of data N(0, s2): alpha s2 / (alpha^2 s2 + sigma^2) x_t.  No afm_native_loop: the generic path."""

    def __init__(self, acp_full, s2):
        super().__init__()
        al = torch.tensor(np.sqrt(acp_full))
        self.coef = nn.Parameter((al * s2 / (al * al * s2 + (1.0 - al * al))).float(), requires_grad=False)

    def forward(self, x, t, **kw):
        return self.coef[t].view(-1, 1, 1) * x


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_second_order_on_the_device(schedule):
    s2, shape = 4.0, (1, 8, 512)
    d = _diffusion("logsnr20", schedule)
    from afm.diffusion import get_named_beta_schedule
    acp_full = np.cumprod(1.0 - get_named_beta_schedule(schedule, 1000))
    model = IdealDenoiser(acp_full, s2).to(dev())
    xT = synth.gaussian("dpm_ideal_xT", shape)
    aT = d.alphas_cumprod[-1]
    exact = xT.double() * np.sqrt(s2) / np.sqrt(aT * s2 + 1.0 - aT)
    args = dict(noise=D(xT), clip_denoised=False)
    ddim = d.ddim_sample_loop(model, shape, eta=0.0, **args).cpu()
    second = d.dpm_solver_sample_loop(model, shape, **args).cpu()
    first = d.dpm_solver_sample_loop(model, shape, order=1, **args).cpu()
    e_ddim, e_2m = ((v.double() - exact).abs().max().item() for v in (ddim, second))
    print(f"[dpm] ideal denoiser {schedule} s2={s2} logsnr20 ({d.num_timesteps} steps): DDIM eta=0 error {e_ddim:.4g}, 2M error {e_2m:.4g}, "
          f"ratio {e_ddim / e_2m:.2f}")
    assert e_2m <= 0.25 * e_ddim
    # order 1 IS DDIM eta = 0 in another float32 association: the float64 twin of that one function, restated on the float64 rows
    t1 = d.dpm_tables("cpu", 1)
    coef = model.coef.double().cpu()
    x = xT.double()
    for i in range(d.num_timesteps - 1, -1, -1):
        x = t1.a64[i] * x + t1.b64[i] * (coef[d.timestep_map[i]] * x)
    report_f32_class(f"order 1 vs DDIM eta=0, ideal denoiser {schedule}", first, ddim, x, old_tol=1e-3, margin=4.0)


# ---------------------------------------------------------------------------------------------------------------- launches, pipeline, refusals
def test_second_native_loop_launches_no_eager_arithmetic(cmdm):
    d = _diffusion("ddim5")
    kw = _kw(golden("cmdm_forward_N1024_L16"))
    d.dpm_solver_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=kw, seed=2)       # first call builds the rows and scratch
    torch.cuda.synchronize()
    _check(_device_kernel_names(lambda: d.dpm_solver_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=kw, seed=3)), "CMDM 2M")


def test_two_stage_dpm_equals_the_stages_by_hand(cmdm, cdm):
    from afm import dist as adist
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="ddim5"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    B, N, L = 2, 1024, 16          # (the cloud of the CMDM's scene encoder: num_points = 1024, as in the DDIM twin of this test)
    text, xyz = D(synth.text_feature(B)), D(synth.scene_cloud(B, N, seed=14))
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9, sampler="dpm++")
    contact = d_adm.dpm_solver_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), seed=9)
    cond = adist.adm_to_amdm_condition(contact, sigma=0.8, mean=0.0, std=1.0)
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=cond, x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    motion = d_amdm.dpm_solver_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=10)
    assert torch.isfinite(got["motion"]).all()
    assert torch.equal(got["contact"], contact) and torch.equal(got["cond"], cond) and torch.equal(got["motion"], motion)
    with pytest.raises(ValueError):
        two_stage_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9, sampler="dpm++", eta=0.5)
    # the CDM samples this solver step by step, an Impute applied as the plain denoised_fn it also is
    mask = torch.zeros(B, N, 6, dtype=torch.bool)
    mask[:, :32, :] = True
    imp = Impute(D(synth.gaussian("dpm_cdm_known", (B, N, 6))), D(mask))
    ckw = dict(clip_denoised=False, denoised_fn=imp, model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), seed=9)
    pinned = d_adm.dpm_solver_sample_loop(cdm, (B, N, 6), **ckw)
    assert torch.equal(pinned, _last(d_adm.dpm_solver_sample_loop_progressive(cdm, (B, N, 6), **ckw)))
    assert torch.equal(pinned[D(mask)], imp.known[D(mask)])


def test_refusals(cmdm):
    d = _diffusion("ddim5")
    kw = _kw(golden("cmdm_forward_N1024_L16"))
    nz = torch.zeros((d.num_timesteps,) + SHAPE, device=dev())
    with pytest.raises(ValueError):
        d.dpm_solver_sample_loop(cmdm, SHAPE, model_kwargs=kw, step_noise=nz)
    with pytest.raises(ValueError):
        next(d.dpm_solver_sample_loop_progressive(cmdm, SHAPE, model_kwargs=kw, step_noise=nz))
    with pytest.raises(NotImplementedError):
        d.dpm_solver_sample_loop(cmdm, SHAPE, model_kwargs=kw, cond_fn=lambda *a, **k: None)
    with pytest.raises(NotImplementedError):
        d.dpm_solver_sample(cmdm, torch.zeros(SHAPE, device=dev()), torch.tensor([1, 1], device=dev()), model_kwargs=kw, cond_fn=lambda *a: None)
    with pytest.raises(ValueError):
        d.dpm_solver_sample_loop(cmdm, SHAPE, model_kwargs=kw, order=3)
    # the C entry: cfg together with cfg2, a workspace one byte short
    lib = ffi.load()
    B, L = SHAPE[0], SHAPE[1]
    w = cmdm._weights()
    x = torch.zeros(SHAPE, device=dev())
    cond = cmdm.condition_tokens(**kw)
    fm = kw["x_mask"].to(device=dev(), dtype=torch.uint8).contiguous()
    tab, rows = d.tables(dev()), d.dpm_tables(dev(), 2)
    sched = ffi.sched_scratch(cmdm, d.num_timesteps, B, dev(), ddim=True)
    scale = torch.full((B,), 2.5, device=dev())
    cfg, cfg2 = ffi.CfgArgs(scale.data_ptr(), 1, 1, 0), ffi.Cfg2Args(scale.data_ptr(), scale.data_ptr(), 0, 0)
    assert lib.afm_cmdm_dpm_loop_workspace_bytes(C.byref(w), B, L, 0, C.byref(cfg), C.byref(cfg2)) == -1
    need = lib.afm_cmdm_dpm_loop_workspace_bytes(C.byref(w), B, L, 0, None, None)
    per = B * L * 263 * 4
    assert need >= lib.afm_cmdm_loop_workspace_bytes(C.byref(w), B, L, 0) + per          # the history buffer is this loop's alone
    ws = torch.empty(need, dtype=torch.uint8, device=dev())

    def call(c1, c2, nbytes):
        return lib.afm_cmdm_dpm_loop_range(C.byref(w), x.data_ptr(), cond.data_ptr(), fm.data_ptr(), tab.timestep_map.data_ptr(), C.byref(rows.rows()),
                                           c1, c2, None, None, d.num_timesteps, 0, B, L, sched.data_ptr(), ws.data_ptr(), nbytes, 0, None,
                                           ffi.stream_of(x))
    assert call(C.byref(cfg), C.byref(cfg2), need) == -1          # AFM_E_BADARG
    assert call(None, None, need - 1) == -2                      # AFM_E_WORKSPACE
    assert call(None, None, need) == 0
    torch.cuda.synchronize()
