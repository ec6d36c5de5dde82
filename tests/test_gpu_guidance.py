"""`-m gpu`: cond_fn guidance.  The added term of the sampling update against the CPU float32 expression (bit for bit); the contact-guidance
kernels (afm_contact_guidance) against the float64 restatement of tests/test_guidance_host.py, bounded by the error of the same expression
in float32 torch; the natively guided loops (afm_cmdm_guide_loop_range) against the step-by-step loops with the same ContactGuidance (bit
for bit); a generic callable against the float64 rule; the effect on the energy; launches; argument errors."""
import ctypes as C

import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.diffusion import ContactGuidance, Impute
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import PARITY_ROWS, ULP32, dev, load_named_weights, report, write_parity_table
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_guidance_host import CASES, SCATTERED, SIGMA, contact_reference, contact_terms, guide_case
from test_impute_host import SHAPE

pytestmark = pytest.mark.gpu
ODD = (3, 5, 263)               # 1315 values per sample: a partial last quad
SHAPE3 = (3, 16, 263)           # the loops' batch: three samples split 2 + 1 over two streams
N_PTS = 130
D = lambda t: t.to(dev())


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


def _kw3():
    """the golden conditions for three samples (the third repeats the first), with a small scene of its own for the guidance: the model
    takes its contact embedding from c_cont_emb, the guidance reads c_pc_xyz / c_pc_contact"""
    g = golden("cmdm_forward_N1024_L16")
    kw = {k: (torch.cat([v, v[:1]], 0) if isinstance(v, torch.Tensor) else v) for k, v in _kw(g).items()}
    kw["info_dummy"] = [0, 1, 2]
    kw["c_pc_xyz"] = D(1.5 * synth.gaussian("guide_loop_q", (3, N_PTS, 3)))
    kw["c_pc_contact"] = D(torch.rand((3, N_PTS, 6), generator=torch.Generator().manual_seed(5)) * 0.999 + 0.001)
    return kw


def _guide(**kw):
    mean, std = 0.3 * synth.gaussian("guide_loop_mean", (263,)), 0.5 + synth.gaussian("guide_loop_std", (263,)).abs()
    kw.setdefault("scale", torch.tensor([1.0, 2.5, 0.5]))
    return ContactGuidance(SCATTERED, mean, std, sigma=SIGMA, **kw)


# ---------------------------------------------------------------------------------------------------------------- the update term, exact
def _cpu_x0(c, u, s, k, m, clip):
    v = c if u is None else u + s.view(-1, 1, 1) * (c - u)
    if m is not None:
        v = torch.where(m, k, v)
    return v.clamp(-1, 1) if clip else v


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_update_term_equals_the_cpu_expression(clip, guided, imputing):
    d = create_gaussian_diffusion(cmdm_cfg())
    tab, dpm = d.tables(dev()), d.dpm_tables(dev(), 2)
    gk_mean, gk_x0 = d.guidance_rows(dev(), "mean"), d.guidance_rows(dev(), "x0")
    v = lambda r: r.cpu().view(-1, 1, 1)
    for shape in (ODD, SHAPE):
        Bn = shape[0]
        c, u, x, nz, k, gr, pv = (synth.gaussian(f"guide_k_{n}_{Bn}", shape) for n in ("c", "u", "x", "nz", "known", "grad", "prev"))
        s = torch.tensor([2.5, 7.5, 0.0][:Bn])
        m = synth.gaussian(f"guide_bits_{Bn}", shape) > 0.3
        base = {}
        if guided:
            base.update(x0_u=D(u), scale=D(s))
        if imputing:
            base.update(known=D(k), mask=D(m))
        x0 = _cpu_x0(c, u if guided else None, s, k, m if imputing else None, clip)
        for tt in (999, 500, 1, 0):
            t = torch.tensor([tt, 3, 0][:Bn], device=dev())
            forms = {"ddpm": dict(ddpm=(tab.coef1[t], tab.coef2[t], tab.sigma[t])), "2m": dict(dpm=(dpm.a[t], dpm.b[t], dpm.c[t]), prev=D(pv)),
                     "2m_first": dict(dpm=(dpm.a[t], dpm.b[t], dpm.c[t]))}
            for eta in (0.0, 1.0):
                rows = d.ddim_tables(dev(), eta)
                forms[f"ddim{eta:g}"] = dict(ddim=(rows.a[t], rows.b[t], rows.c[t], rows.d[t], None if rows.sigma is None else rows.sigma[t]))
            for name, f in forms.items():
                gk = (gk_mean if name == "ddpm" else gk_x0)[t]
                m_ = v(gk) * gr                                  # m = gk * grad, rounded; then the addition, rounded
                if name == "ddpm":
                    c1, c2, sg = f["ddpm"]
                    want, shifted = ((v(c1) * x0 + v(c2) * x) + m_) + v(sg) * nz, None
                else:
                    shifted = x0 + m_
                    if "ddim" in f:
                        a, b, cc, dd, sg = f["ddim"]
                        want = shifted * v(cc) + v(dd) * ((v(a) * x - shifted) / v(b))
                        want = want if sg is None else want + v(sg) * nz
                    else:
                        a, b, cc = f["dpm"]
                        want = v(a) * x + v(b) * shifted
                        want = want if "prev" not in f else want + v(cc) * pv
                args = dict(clip=clip, **base, **f)
                keep = torch.empty(shape, device=dev()) if shifted is not None else None
                got = ops.guide_step(D(c), D(x), D(nz), grad=D(gr), gk=gk, x0_out=keep, **args)
                assert torch.equal(got.cpu(), want), (name, tt, shape)
                assert shifted is None or torch.equal(keep.cpu(), shifted), (name, tt, shape)
                # a gradient of zeros: today's update exactly; no gradient: the existing entry points, and grad is never read
                plain = ops.guide_step(D(c), D(x), D(nz), **args)
                assert torch.equal(plain, ops.guide_step(D(c), D(x), D(nz), grad=torch.zeros(shape, device=dev()), gk=gk, **args)), (name, tt)
                if name == "ddpm" and imputing:
                    old = ops.impute_step(D(c), D(k), D(m), D(x), D(nz), ddpm=f["ddpm"], clip=clip, **({} if not guided else dict(x0_u=D(u), scale=D(s))))
                elif name.startswith("ddim") and guided and not imputing:
                    old = ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddim=f["ddim"], clip=clip)
                elif name.startswith("2m") and not guided and not imputing and not clip:
                    old = ops.dpm_step(D(c), D(x), f.get("prev"), *f["dpm"])
                else:
                    old = None
                assert old is None or torch.equal(plain, old), (name, tt)
                out = D(x).clone()                               # in place on x_t, as the loops run it
                ops.guide_step(D(c), out, D(nz), grad=D(gr), gk=gk, out=out, **args)
                assert torch.equal(out, got), (name, tt)
        with pytest.raises(ValueError, match="x0_out"):          # the shifted prediction's buffer is checked like every other tensor
            ops.guide_step(D(c), D(x), D(nz), grad=D(gr), gk=gk_x0[t], x0_out=torch.empty(shape[:2], device=dev()), **forms["ddim0"])
        with pytest.raises(ValueError, match="x0_out"):
            ops.guide_step(D(c), D(x), D(nz), grad=D(gr), gk=gk_x0[t], x0_out=torch.empty(shape, device=dev()).transpose(0, 1), **forms["ddim0"])
        # one of grad / gk without the other: AFM_E_BADARG
        a = ffi.GuideStepArgs()
        bufs = [D(c), D(x), D(gr), torch.empty(shape, device=dev()), tab.coef1[t].contiguous()]
        a.x0_c, a.x_t, a.noise, a.x_next = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[1].data_ptr(), bufs[3].data_ptr()
        a.c1 = a.c2 = a.sigma = bufs[4].data_ptr()
        a.B, a.per_sample = Bn, shape[1] * shape[2]
        lib = ffi.load()
        a.grad = bufs[2].data_ptr()
        assert lib.afm_guide_step(C.byref(a), ffi.stream_of(bufs[0])) == -1
        a.grad, a.gk = None, bufs[4].data_ptr()
        assert lib.afm_guide_step(C.byref(a), ffi.stream_of(bufs[0])) == -1
        a.gk = None
        assert lib.afm_guide_step(C.byref(a), ffi.stream_of(bufs[0])) == 0
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the gradient kernels
def _bound_row(name, got, want32, want64):
    """|got - f64| <= 4 x |f32 torch - f64| + 4 ulp of the largest entry (max norm).  The factor covers another summation order over the
    points, not another algorithm; the floor covers results whose float32 twin happens to be exact."""
    e_got, e_ref = (got.double().cpu() - want64).abs().max().item(), (want32.double() - want64).abs().max().item()
    floor = 4 * ULP32 * want64.abs().max().item()
    ratio = e_got / (e_ref + floor / 4.0) if e_ref + floor > 0 else 0.0
    print(f"[guidance parity] {name}: f32 torch max {e_ref:.3e} | hip max {e_got:.3e} | ratio {ratio:.2f} (floor {floor:.1e})")
    PARITY_ROWS.append(dict(name=name, max_ref=e_ref, max_got=e_got, ratio_max=ratio, margin=4.0, floor=floor))
    assert e_got <= 4.0 * e_ref + floor, f"{name}: max|hip - f64| = {e_got:.3e} > 4 x {e_ref:.3e} + {floor:.1e}"


@pytest.mark.parametrize("case", CASES)
def test_contact_guidance_kernels_vs_float64(case):
    N, K, Dm = case
    g = guide_case(*case)
    guide = ContactGuidance(g["cols"], g["mean"], g["std"], sigma=SIGMA, scale=g["scale"])
    kw = dict(c_pc_xyz=D(g["q"]), c_pc_contact=D(g["c"]), x_mask=D(g["x_mask"]))
    t = torch.zeros(3, dtype=torch.int64, device=dev())
    got, energy = guide(D(g["x"]), t, **kw), guide.energy(D(g["x"]), **kw)
    want64, e64 = contact_reference(**g)
    want32, e32 = contact_reference(**g, dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (3,)
    _bound_row(f"contact guidance grad N={N} K={K} D={Dm}", got, want32, want64)
    _bound_row(f"contact guidance energy N={N} K={K} D={Dm}", energy, e32, e64)
    # exact zeros: outside the named columns, in masked frames, in the sample without a valid frame, at the zero std
    named = torch.zeros(Dm, dtype=torch.bool)
    for col in g["cols"]:
        named[col:col + 3] = True
    gc = got.cpu()
    assert not gc[..., ~named].any() and not gc[2].any() and not gc[1, -2:].any() and not gc[..., g["cols"][0] + 1].any()
    assert gc[1].abs().max() > 0 and (N == 1 or gc[0].abs().max() > 0)          # (N = 1: sample 0's only point sits on the joint)
    fstar = contact_terms(g["x"], g["x_mask"], g["q"], g["c"], g["cols"], g["mean"], g["std"], SIGMA, torch.float64)[3]
    hit = torch.zeros(3, 7, dtype=torch.bool)
    for b in range(2):
        hit[b, fstar[b].unique()] = True
    assert not gc[~hit].any() and not gc[0, 4].any()          # frames no point is nearest to; the duplicate frame: the first index won
    # the same bits run to run, and sample b of the batch is the sample computed alone
    assert torch.equal(got, guide(D(g["x"]), t, **kw)) and torch.equal(energy, guide.energy(D(g["x"]), **kw))
    for b in range(3):
        alone = ContactGuidance(g["cols"], g["mean"], g["std"], sigma=SIGMA, scale=g["scale"][b:b + 1])
        kwb = {k: v[b:b + 1] for k, v in kw.items()}
        assert torch.equal(alone(D(g["x"][b:b + 1]), t[:1], **kwb), got[b:b + 1]) and torch.equal(alone.energy(D(g["x"][b:b + 1]), **kwb), energy[b:b + 1])
    pair = ContactGuidance(g["cols"], g["mean"], g["std"], sigma=SIGMA, scale=g["scale"][1:])
    assert torch.equal(pair(D(g["x"][1:]), t[1:], **{k: v[1:] for k, v in kw.items()}), got[1:])
    # t_start: a sample at or above it gets zeros, the others what they got
    late = ContactGuidance(g["cols"], g["mean"], g["std"], sigma=SIGMA, scale=g["scale"], t_start=500)
    part = late(D(g["x"]), torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(part[1:], got[1:])


# ---------------------------------------------------------------------------------------------------------------- native loops, exact
FORMS = {"ddpm": ("5", "p"), "ddim": ("ddim5", "ddim"), "2m": ("ddim5", "dpm")}
GUIDANCE = {"unguided": None, "one scale": torch.tensor([2.5, 7.5, 1.0]), "two scales": {"pc": 1.5, "text": 5.0}}


def _sampler(form):
    """(diffusion, loop(model, shape, **kw), progressive(model, shape, **kw)) of a form: 5 steps"""
    respacing, kind = FORMS[form]
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=respacing))
    if kind == "p":
        return d, d.p_sample_loop, d.p_sample_loop_progressive
    if kind == "ddim":
        return d, (lambda *a, **k: d.ddim_sample_loop(*a, eta=0.0, **k)), (lambda *a, **k: d.ddim_sample_loop_progressive(*a, eta=0.0, **k))
    return d, (lambda *a, **k: d.dpm_solver_sample_loop(*a, order=2, **k)), (lambda *a, **k: d.dpm_solver_sample_loop_progressive(*a, order=2, **k))


def _model(cmdm, how):
    scale = GUIDANCE[how]
    if scale is None:
        return cmdm
    return GuidedCMDM(cmdm, D(scale) if isinstance(scale, torch.Tensor) else scale)


def _imp3():
    return Impute(D(synth.gaussian("guide_known", SHAPE3)), D(synth.gaussian("guide_known_bits", SHAPE3) > 0.6))


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("how", list(GUIDANCE))
@pytest.mark.parametrize("form", list(FORMS))
def test_native_guided_loop_equals_the_step_by_step_loop(cmdm, form, how, imputing):
    d, loop, progressive = _sampler(form)
    t_mid = d.timestep_map[2] + 1                               # the two first executed steps run unguided, the last three guided
    guide = _guide(t_start=t_mid)
    assert guide.first_guided(d) == 2
    model = _model(cmdm, how)
    args = dict(clip_denoised=imputing, denoised_fn=_imp3() if imputing else None, cond_fn=guide, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        native = loop(model, SHAPE3, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": None}))
        # a range-sliced call: the progress bar's slices, and snapshots cut inside the unguided and the guided part
        assert torch.equal(native, loop(model, SHAPE3, progress=True, **args))
        snaps = {1: None, 3: None}
        assert torch.equal(native, loop(model, SHAPE3, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
        steps = list(progressive(model, SHAPE3, **args))
        assert torch.equal(snaps[1], steps[0]["sample"]) and torch.equal(snaps[3], steps[2]["sample"])
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False      # two streams: sub-batches of 2 + 1
        assert torch.equal(native, loop(model, SHAPE3, **args))
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


@pytest.mark.parametrize("form", list(FORMS))
def test_the_guidance_masks_padded_frames_where_the_model_does_not(form):
    """mask_motion=False: the denoiser has no frame mask, the guidance still takes x_mask from model_kwargs - padded frames never attain the
    minimum and get no gradient, natively as step by step."""
    cfg = cmdm_cfg()
    cfg.model.mask_motion = False
    model = create_model(cfg, device=dev())
    load_named_weights(model)
    model = model.to(dev()).eval()
    assert not model.mask_motion
    d, loop, progressive = _sampler(form)
    kw = _kw3()
    kw["x_mask"] = torch.zeros(3, 16, dtype=torch.bool, device=dev())
    kw["x_mask"][1, 9:] = True                                  # one padded sample
    args = dict(clip_denoised=False, cond_fn=_guide(), model_kwargs=kw, seed=4)
    native = loop(model, SHAPE3, **args)
    assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
    assert not torch.equal(native, loop(model, SHAPE3, **{**args, "model_kwargs": {**kw, "x_mask": torch.zeros_like(kw["x_mask"])}}))
    # the gradient the loop computes is the masked one: a guided first step moves no padded frame off the unguided step
    one = {1: None}
    loop(model, SHAPE3, snapshots=one, **args)
    plain = {1: None}
    loop(model, SHAPE3, snapshots=plain, **{**args, "cond_fn": _guide(scale=0.0)})          # (the same separate-update form, a gradient of zeros)
    moved = (one[1] != plain[1]).flatten(2).any(-1)
    assert not moved[1, 9:].any() and moved[1, :9].any() and moved[0].any()


@pytest.mark.parametrize("form,how", [("ddpm", "unguided"), ("ddpm", "one scale"), ("ddim", "unguided"), ("ddim", "two scales"),
                                      ("2m", "unguided"), ("2m", "one scale")])
def test_zero_scale_and_a_late_start_reproduce_the_unguided_loop(cmdm, form, how):
    """scale = 0 and a t_start below every timestep give the unguided loop of the same form.  The guided loops run in the separate-update
    form; the plain native DDPM loop alone runs the contracted update fused into its last GEMM (it may differ from every separate-update
    form in the last bit, as tests/test_gpu_impute.py notes), so for ("ddpm", "unguided") the unguided loop of the same form is the
    step-by-step one."""
    d, loop, progressive = _sampler(form)
    model = _model(cmdm, how)
    args = dict(clip_denoised=False, model_kwargs=_kw3(), seed=4)
    plain = _last(progressive(model, SHAPE3, **args)) if (form, how) == ("ddpm", "unguided") else loop(model, SHAPE3, **args)
    for guide in (_guide(scale=0.0), _guide(t_start=0), _guide(scale=torch.zeros(3))):
        assert torch.equal(loop(model, SHAPE3, cond_fn=guide, **args), plain)
        assert torch.equal(_last(progressive(model, SHAPE3, cond_fn=guide, **args)), plain)


def test_unguided_steps_never_read_the_gradient_buffer(cmdm):
    """NaNs planted in the loop's gradient buffer (in the workspace: behind the history, in front of the guidance workspace, as
    include/afm_hip.h lays it out) are never read on a step without the term; a guided step overwrites them first."""
    d, loop, _ = _sampler("ddim")
    args = dict(clip_denoised=False, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True
    try:
        plain = loop(cmdm, SHAPE3, **args)
        mid = loop(cmdm, SHAPE3, cond_fn=_guide(t_start=d.timestep_map[2] + 1), **args)
        (ws,) = cmdm._ws.values()
        a256 = lambda n: (n + 255) & ~255
        tail = a256(int(ffi.load().afm_contact_guidance_workspace_bytes(3, N_PTS, 6)))
        nbytes = a256(3 * 16 * 263 * 4)
        region = ws[ws.numel() - tail - nbytes: ws.numel() - tail - nbytes + 3 * 16 * 263 * 4].view(torch.float32)
        region.fill_(float("nan"))
        assert torch.equal(loop(cmdm, SHAPE3, cond_fn=_guide(t_start=0), **args), plain) and region.isnan().all()
        assert torch.equal(loop(cmdm, SHAPE3, cond_fn=_guide(t_start=d.timestep_map[2] + 1), **args), mid) and not region.isnan().any()
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved


# ---------------------------------------------------------------------------------------------------------------- a generic callable
def test_a_generic_callable_follows_the_float64_rule(cmdm):
    """A lambda returning a fixed tensor: p_sample (condition_mean) and ddim_sample (condition_score) against the float64 rule applied to
    the unguided step's own outputs.  Bounds: those tests/test_gpu_ddim.py states for one step (pred_xstart 8e-5, sample 5.5e-5)."""
    g = golden("cmdm_forward_N1024_L16")
    d = create_gaussian_diffusion(cmdm_cfg())
    grad = 0.1 * synth.gaussian("guide_generic_grad", SHAPE)
    fn = lambda x, t, **kw: D(grad)
    x, nz, t = D(g["x"]), D(synth.gaussian("guide_generic_nz", SHAPE)), torch.tensor([500, 500], device=dev())
    seen = []
    spy = lambda x_, t_, **kw: seen.append((x_, t_, sorted(kw))) or D(grad)
    base = d.p_sample(cmdm, x, t, clip_denoised=False, model_kwargs=_kw(g), noise=nz)
    out = d.p_sample(cmdm, x, t, clip_denoised=False, cond_fn=spy, model_kwargs=_kw(g), noise=nz)
    assert torch.equal(seen[0][0], x) and torch.equal(seen[0][1], t) and "c_text_feat" in seen[0][2]          # evaluated at x_t, the model's t
    var = float(d.posterior_variance[500])
    assert torch.equal(out["pred_xstart"], base["pred_xstart"])
    report("generic cond_fn p_sample t=500 sample", out["sample"], base["sample"].double().cpu() + var * grad.double(), 5.5e-5)
    zero = d.p_sample(cmdm, x, torch.tensor([0, 0], device=dev()), clip_denoised=False, cond_fn=fn, model_kwargs=_kw(g), noise=nz)
    assert torch.equal(zero["sample"], d.p_sample(cmdm, x, torch.tensor([0, 0], device=dev()), clip_denoised=False, model_kwargs=_kw(g), noise=nz)["sample"])
    for eta in (0.0, 1.0):
        base = d.ddim_sample(cmdm, x, t, clip_denoised=False, model_kwargs=_kw(g), eta=eta, noise=nz)
        out = d.ddim_sample(cmdm, x, t, clip_denoised=False, cond_fn=fn, model_kwargs=_kw(g), eta=eta, noise=nz)
        acp, acp_prev = float(d.alphas_cumprod[500]), float(d.alphas_cumprod_prev[500])
        x0 = base["pred_xstart"].double().cpu() + (1 - acp) / acp ** 0.5 * grad.double()
        eps = ((1 / acp) ** 0.5 * g["x"].double() - x0) / (1 / acp - 1) ** 0.5
        sigma = eta * ((1 - acp_prev) / (1 - acp)) ** 0.5 * (1 - acp / acp_prev) ** 0.5
        want = x0 * acp_prev ** 0.5 + (1 - acp_prev - sigma ** 2) ** 0.5 * eps + sigma * nz.double().cpu()
        report(f"generic cond_fn ddim_sample eta={eta:g} t=500 pred_xstart", out["pred_xstart"], x0, 8e-5)
        report(f"generic cond_fn ddim_sample eta={eta:g} t=500 sample", out["sample"], want, 5.5e-5)
    # a generic callable keeps the loop step by step, and the loop's result is the chain of the steps
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    args = dict(clip_denoised=False, cond_fn=fn, model_kwargs=_kw(g), seed=3)
    assert torch.equal(d5.dpm_solver_sample_loop(cmdm, SHAPE, **args), _last(d5.dpm_solver_sample_loop_progressive(cmdm, SHAPE, **args)))


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_guidance_lowers_the_energy_of_every_sample():
    """A target map made from a known motion, the chain started from that motion plus noise: the guided chain ends at a lower energy than
    the unguided chain, for every sample.  Two runs compared; no threshold.

    The denoiser is the identity (pred_xstart = x_t), for which the effect follows from the update itself: a DDIM eta = 0 step is then
    x_next = A x_t + B gk g(x_t) with g = -scale dE/dx at the very point the step starts from, A > 0 and
    B = sqrt(abar_prev) - sqrt(abar_t) sqrt(1 - abar_prev) / sqrt(1 - abar_t) > 0 (abar_prev > abar_t): the unguided chain's step plus
    one gradient-descent step on E.  Guidance starts at model timestep 600, where gk = (1 - abar) / sqrt(abar) is about 1.1: with
    scale = 20 the step length stays far below 2 / (the largest curvature of E), about 2 / (2 / (K L)) = K L.  (The synthetic weights of
    the golden CMDM make its prediction all but independent of x_t, so its final sample - the last step's prediction - cannot show the
    effect of a gradient that acts through x_t: measured there, the final energies of the guided and the unguided native chains agree
    to 6 digits, [0.1364410, 0.1114841, 0.1288183] against [0.1364402, 0.1114846, 0.1288176].)"""
    kw = _kw3()
    guide = _guide(scale=20.0, t_start=601)
    known = 0.5 * synth.gaussian("guide_effect_motion", SHAPE3)
    chat = contact_terms(known, kw["x_mask"].cpu(), kw["c_pc_xyz"].cpu(), kw["c_pc_contact"].cpu(), SCATTERED, guide.mean.cpu(), guide.std.cpu(),
                         SIGMA, torch.float32)[2]
    kw = dict(c_pc_xyz=kw["c_pc_xyz"], c_pc_contact=D(chat), x_mask=kw["x_mask"])
    assert guide.energy(D(known), **kw).max().item() < 1e-10          # the known motion reproduces its own map
    start = D(known + 0.5 * synth.gaussian("guide_effect_noise", SHAPE3))
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    identity = lambda x, t, **_: x
    args = dict(noise=start, clip_denoised=False, model_kwargs=kw, eta=0.0, device=dev())
    plain, guided = d.ddim_sample_loop(identity, SHAPE3, **args), d.ddim_sample_loop(identity, SHAPE3, cond_fn=guide, **args)
    e_start, e_plain, e_guided = guide.energy(start, **kw), guide.energy(plain, **kw), guide.energy(guided, **kw)
    print(f"[guidance effect] energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
    assert (e_guided < e_plain).all()


# ---------------------------------------------------------------------------------------------------------------- launches
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_guided_jobs_launch_no_eager_arithmetic_and_the_derived_launch_counts(cmdm, cdm):
    n = 6
    kw = _kw3()
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    dp = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=str(n)))
    guide = _guide(t_start=dd.timestep_map[3] + 1)              # 2 unguided steps, 4 guided ones (both processes keep 6 timesteps)
    assert guide.first_guided(dd) == 2
    gp = _guide(t_start=dp.timestep_map[3] + 1)
    assert gp.first_guided(dp) == 2
    # (every launch but torch's movers; the gradient's second pass has "gather" in its name and is no mover)
    kernels = lambda names: sum(c for k, c in names.items() if "guide_gather_kernel" in k or not _MOVERS.search(k))
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    # the loop of the same (separate-update) form without guidance: an imputing loop that knows nothing
    none = Impute(D(synth.gaussian("guide_known", SHAPE3)), torch.zeros(SHAPE3, dtype=torch.bool, device=dev()))
    sep = lambda fn: none if fn is None else None
    runs = {"ddim": lambda fn: dd.ddim_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5),
            "2m": lambda fn: dd.dpm_solver_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5),
            "ddpm": lambda fn: dp.p_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5)}
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        for name, run in runs.items():
            fn = gp if name == "ddpm" else guide
            run(fn), run(None)                                    # (weight pack, workspaces, rows and streams exist before anything is counted)
            torch.cuda.synchronize()
            with_g, without = _device_kernel_names(lambda: run(fn)), _device_kernel_names(lambda: run(None))
            _check(with_g, f"contact-guided native loop ({name})")
            print(f"[guidance launches] {name}: kernels with {kernels(with_g)}, without {kernels(without)}")
            # per guided step: the two gradient launches on top of the separate-update loop of the form; every step: one update launch
            assert count(with_g, "guide_nearest_kernel") == count(with_g, "guide_gather_kernel") == 4
            assert count(with_g, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
            assert kernels(with_g) == kernels(without) + 2 * 4
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # both stages, the motion stage guided towards the first stage's own map
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    B, N, L = 2, 1024, 16
    args = dict(text_feat=D(synth.text_feature(B)), xyz=D(synth.scene_cloud(B, N, seed=14)), frames=L, sigma=SIGMA, seed=9, sampler="ddim")
    g2 = _guide(scale=2.0)
    two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args))
    _check(names, "two_stage_sample(contact_guidance=...)")
    assert count(names, "guide_nearest_kernel") == count(names, "guide_gather_kernel") == n
    base = two_stage_sample(cdm, d_adm, cmdm, dd, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"]) and not torch.equal(got["motion"], base["motion"])
    kw2 = dict(c_text_feat=args["text_feat"], c_pc_xyz=args["xyz"], c_pc_contact=base["cond"], x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    by_hand = dd.ddim_sample_loop(cmdm, (B, L, 263), clip_denoised=False, cond_fn=g2, model_kwargs=kw2, seed=10)
    assert torch.equal(got["motion"], by_hand)


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _GuideLoopProbe:
    """The loaded library with afm_cmdm_guide_loop_range wrapped: in front of every real call, the same call without the description,
    with a negative first_step, with no rows at all, with two kinds of rows, with a mask but no known values, and with a description whose
    column triple leaves the motion vector / that has no gk rows - AFM_E_BADARG each, returned before anything is enqueued."""
    ROWS, DPM, C1, C2, SIGMA_, KNOWN, MASK, GUIDE, FIRST_STEP = 6, 7, 8, 9, 10, 13, 14, 15, 17

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_guide_loop_range":
            return fn

        def call(*args):
            some = args[1]                                      # a valid device pointer
            two_m = ffi.DpmRows(some, some, some)
            both = {self.C1: some, self.C2: some, self.SIGMA_: some} if args[self.C1] is None else {self.DPM: C.byref(two_m)}
            for change in ({self.GUIDE: None}, {self.FIRST_STEP: -1}, {self.ROWS: None, self.DPM: None, self.C1: None, self.C2: None, self.SIGMA_: None},
                           both, {self.KNOWN: None, self.MASK: some}):
                bad = list(args)
                for i, val in change.items():
                    bad[i] = val
                assert fn(*bad) == -1, change
            real = args[self.GUIDE]._obj
            for field, val in (("cols", None), ("gk", None), ("K", 0), ("sigma", 0.0), ("first_guided", -1)):
                broken = ffi.ContactGuide.from_buffer_copy(real)
                if field == "cols":
                    broken.cols[0] = 262
                else:
                    setattr(broken, field, val)
                bad = list(args)
                bad[self.GUIDE] = C.byref(broken)
                assert fn(*bad) == -1, field
            self.calls += 1
            return fn(*args)
        return call


def test_loop_argument_errors_leave_the_next_call_untouched(cmdm, monkeypatch):
    guide, imp = _guide(), _imp3()
    runs = []
    for form in FORMS:
        _, loop, _ = _sampler(form)
        for m in (cmdm, _model(cmdm, "one scale")):
            runs.append(lambda m=m, loop=loop: loop(m, SHAPE3, clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=_kw3(), seed=4))
    want = [run().clone() for run in runs]
    probe = _GuideLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == 6 and all(torch.equal(a, b) for a, b in zip(want, got))


def test_zz_write_parity_table():
    """Not a check: stores the ratios measured so far (gpu_util.write_parity_table; committed as profiles/contact_guidance_parity.json),
    with the rule `_bound_row` applied in place of the writer's general one."""
    import json
    path = write_parity_table()
    if path and any("contact guidance" in r["name"] for r in PARITY_ROWS):
        table = json.load(open(path))
        table["rule"] = ("rows named 'contact guidance ...': max|hip - f64| <= 4 * max|f32 torch - f64| + 4 * 2^-23 max|f64| (max norm only, no "
                         "rms); ratio_max = e_hip / (e_ref + floor / 4), floor = 4 * 2^-23 max|f64|")
        json.dump(table, open(path, "w"), indent=1)
