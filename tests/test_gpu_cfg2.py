"""`-m gpu`: two-scale classifier-free guidance of the CMDM, one scale per condition (afm.cmdm.GuidedCMDM with a mapping, afm_cfg2_*,
afm_cmdm_cfg2_*): the kernels against the CPU float32 expression (bit for bit), the reference goldens of tools/make_goldens_cfg2.py and
the composed oracle, the product's own forms against each other (bit for bit), the launches of a two-scale job.

    g1 = u + s_first * (a - u);   x0 = g1 + s_second * (c - a)          u: both dropped, a: only `first` kept, c: nothing dropped

Bounds against the reference: at most 20x the error measured on the MI355X (in the comment beside each), and never above the bound of the
matching unguided test times AMP = |1 - s1| + |s1 - s2| + |s2| = 14 for the largest scales (1 - 2.5, 2.5 - 7.5, 7.5).  Beside every
report() against a golden stands report_f32_class against the float64 twin of the composed oracle, margin 4."""
import pytest
import torch

from afm import ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.diffusion import Impute
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report, report_f32_class, to_f64, write_parity_table
from test_cfg2_host import ORDERS, SCALES, SHAPE, branches_oracle, combine2, guided2_oracle, scale_rows
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import AMP, DDIM_LOOP, FWD, LOOP, _last
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_impute_host import ddim_loop_ref, impute_known, impute_mask, imputed

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


def _scales(order=ORDERS["pc_text"]):
    """the goldens' per-sample scales as the wrapper's mapping, in `order`"""
    return {k: torch.tensor(SCALES[k], device=dev()) for k in order}


def _loop_inputs(resp, prefix):
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=resp))
    nz = D(torch.stack([synth.gaussian(f"{prefix}_{j}", SHAPE) for j in range(d.num_timesteps)]))
    return d, nz, D(synth.gaussian(f"{prefix}_xT", SHAPE))


def _twin():
    from oracle import shapes as sh
    return to_f64(sh.weights(sh.cmdm())), to_f64(golden("cmdm_forward_N1024_L16"))


# ---------------------------------------------------------------------------------------------------------------- kernels, exact
@pytest.mark.parametrize("clip", [False, True])
def test_combine_and_update_kernels_equal_the_cpu_expression(clip):
    """afm_cfg2_combine and afm_cfg2_step against float32 torch on the CPU, and against the launches of the step-by-step path."""
    g = golden("cmdm_cfg2_forward_pc_text_t500")
    assert torch.equal(ops.cfg2_combine(D(g["x0_c"]), D(g["x0_a"]), D(g["x0_u"]), D(g["scale_first"]), D(g["scale_second"])).cpu(), g["guided"])
    d = create_gaussian_diffusion(cmdm_cfg())
    tab = d.tables(dev())
    # (3, 5, 263): 1315 values per sample - the last quad of a sample is partial and the mask bases of samples 1, 2 are not 4-aligned
    odd = (3, 5, 263)
    c, a, u, x, nz, k = (synth.gaussian(f"cfg2_odd_{n}", odd) for n in ("c", "a", "u", "x", "nz", "k"))
    s1, s2 = torch.tensor([1.5, 2.5, 0.0]), torch.tensor([2.5, 7.5, 1.0])
    m = synth.gaussian("cfg2_odd_mask", odd) > 0
    m[1], m[2] = False, True                                   # an all-zero sample and an all-one sample
    knan = torch.where(m, k, torch.full_like(k, float("nan")))  # a select: known is not read where the mask is 0
    guided = combine2(c, a, u, s1, s2)
    assert torch.equal(ops.cfg2_combine(D(c), D(a), D(u), D(s1), D(s2)).cpu(), guided)
    br = (D(c), D(a), D(u), D(s1), D(s2))
    v = lambda r: r.cpu().view(-1, 1, 1)
    for mask in (None, m):
        imp = {} if mask is None else dict(known=D(k), mask=D(mask))
        x0 = guided if mask is None else torch.where(mask, k, guided)
        x0 = x0.clamp(-1, 1) if clip else x0
        x0d = ops.cfg2_combine(*br)                             # the launches of the step-by-step path: combine, impute, clamp_, step
        if mask is not None:
            x0d = ops.impute(x0d, D(k), D(mask))
        if clip:
            x0d = ops.clamp_(x0d, -1.0, 1.0)
        assert torch.equal(x0d.cpu(), x0)
        for tt in (999, 500, 1, 0):
            t = torch.tensor([tt, 3, 0], device=dev())
            c1, c2, sg = tab.coef1[t], tab.coef2[t], tab.sigma[t]
            want = (v(c1) * x0 + v(c2) * x) + v(sg) * nz
            got = ops.cfg2_step(*br, D(x), D(nz), ddpm=(c1, c2, sg), clip=clip, **imp)
            assert torch.equal(got.cpu(), want), ("ddpm", tt, mask is not None)
            assert torch.equal(got, ops.ddpm_step(x0d, D(x), D(nz), c1, c2, sg))
            if mask is not None:
                nan = ops.cfg2_step(*br, D(x), D(nz), ddpm=(c1, c2, sg), clip=clip, known=D(knan), mask=D(mask))
                assert torch.equal(got, nan) and torch.isfinite(nan).all()
            for eta in (0.0, 1.0):                              # without and with a noise term
                rows = d.ddim_tables(dev(), eta)
                ra, rb, rc, rd = (r[t] for r in (rows.a, rows.b, rows.c, rows.d))
                sgd = None if rows.sigma is None else rows.sigma[t]
                eps = (v(ra) * x - x0) / v(rb)
                want = x0 * v(rc) + v(rd) * eps
                if sgd is not None:
                    want = want + v(sgd) * nz
                got = ops.cfg2_step(*br, D(x), D(nz), ddim=(ra, rb, rc, rd, sgd), clip=clip, **imp)
                assert torch.equal(got.cpu(), want), ("ddim", tt, eta, mask is not None)
                assert torch.equal(got, ops.ddim_step(x0d, D(x), D(nz), ra, rb, rc, rd, sgd))
        for rows in (dict(ddpm=(c1, c2, sg)), dict(ddim=(ra, rb, rc, rd, sgd))):
            out = D(x).clone()                                  # x_next aliasing x_t, as the loops run it
            ops.cfg2_step(*br, out, D(nz), clip=clip, out=out, **rows, **imp)
            assert torch.equal(out, ops.cfg2_step(*br, D(x), D(nz), clip=clip, **rows, **imp))
        phil = ops.cfg2_step(*br, D(x), None, ddpm=(c1, c2, sg), clip=clip, seed=11, sample_index0=3, step=7, **imp)
        given = ops.randn(odd, dev(), seed=11, sample_index0=3, step=7)
        assert torch.equal(phil, ops.cfg2_step(*br, D(x), given, ddpm=(c1, c2, sg), clip=clip, **imp))


# ---------------------------------------------------------------------------------------------------------------- reference goldens
@pytest.mark.parametrize("tt", [999, 500, 0])
def test_forward_vs_reference_golden(cmdm, tt):
    g = golden("cmdm_forward_N1024_L16")
    x, t = D(g["x"]), torch.tensor([tt, tt], device=dev())
    with torch.no_grad():
        plain = cmdm(x, t, **_kw(g))
    sd64, g64 = _twin()
    for tag, order in ORDERS.items():
        gg = golden(f"cmdm_cfg2_forward_{tag}_t{tt}")
        w = GuidedCMDM(cmdm, _scales(order))
        c, a, u, gd = w.branches(x, t, **_kw(g))
        assert torch.equal(c, plain)                            # the conditioned branch IS the unguided forward
        assert torch.equal(gd, ops.cfg2_combine(c, a, u, *_scales(order).values())) and torch.equal(gd, w(x, t, **_kw(g)))
        # the other two ARE the single-scale wrapper's unconditioned branches: the partial drop of `second`, the compact drop of both
        assert torch.equal(a, GuidedCMDM(cmdm, 1.0, (order[1],)).branches(x, t, **_kw(g))[1])
        assert torch.equal(u, GuidedCMDM(cmdm, 1.0).branches(x, t, **_kw(g))[1])
        c64, a64, u64 = branches_oracle(sd64, g64, order)(g64["x"], t.cpu())
        gd64 = combine2(c64, a64, u64, *scale_rows(order, torch.float64))
        for name, got, want64, tol in (("x0_c", c, c64, TOL_FWD_BRANCH), ("x0_a", a, a64, TOL_FWD_BRANCH), ("x0_u", u, u64, TOL_FWD_BRANCH),
                                       ("guided", gd, gd64, TOL_FWD_GUIDED)):
            report(f"two-scale forward t={tt} {tag}: {name}", got, gg[name], tol)
            report_f32_class(f"two-scale forward t={tt} {tag}: {name}", got, gg[name], want64, tol)
        # force_masked applies to u: another place of the attention's key blocks, the same function (not bit-equal)
        cm, am, um, gm = GuidedCMDM(cmdm, _scales(order), force_masked=True).branches(x, t, **_kw(g))
        assert torch.equal(cm, c) and torch.equal(am, a)
        report(f"two-scale forward t={tt} {tag}: x0_u, masked form", um, gg["x0_u"], TOL_FWD_BRANCH)
        report(f"two-scale forward t={tt} {tag}: guided, masked u", gm, gg["guided"], TOL_FWD_GUIDED)
        report_f32_class(f"two-scale forward t={tt} {tag}: guided, masked u", gm, gg["guided"], gd64, TOL_FWD_GUIDED)


def test_p_sample_vs_reference_golden(cmdm):
    g, gs = golden("cmdm_forward_N1024_L16"), golden("cmdm_cfg2_p_sample_t500")
    d = create_gaussian_diffusion(cmdm_cfg())
    out = d.p_sample(GuidedCMDM(cmdm, _scales()), D(g["x"]), torch.tensor([500, 500], device=dev()), clip_denoised=False,
                     model_kwargs=_kw(g), noise=D(synth.gaussian("p_sample_noise_500", SHAPE)))
    report("two-scale p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], TOL_FWD_GUIDED)
    report("two-scale p_sample t=500 sample", out["sample"], gs["sample"], TOL_PSAMPLE)
    from oracle import diffusion_ref as df
    sd64, g64 = _twin()
    w64 = df.p_sample(df.Schedule(1000), guided2_oracle(sd64, g64, ORDERS["pc_text"], torch.float64), g64["x"], torch.tensor([500, 500]),
                      synth.gaussian("p_sample_noise_500", SHAPE).double())
    report_f32_class("two-scale p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], w64["pred_xstart"], TOL_FWD_GUIDED)
    report_f32_class("two-scale p_sample t=500 sample", out["sample"], gs["sample"], w64["sample"], TOL_PSAMPLE)


@pytest.mark.parametrize("tag", ["r5", "r5_clip", "impute_r5"])
def test_ddpm_loop_vs_reference_golden(cmdm, tag):
    """The native two-scale loop (afm_cmdm_cfg2_loop_range) against the reference, and bit for bit against the step-by-step loop through
    wrapper.forward + p_sample, its sliced form and its masked-u form (within the golden's bound)."""
    d, nz, xT = _loop_inputs("5", "loop_r5")
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_cfg2_loop_{tag}")["sample"]
    clip = tag == "r5_clip"
    imp = Impute(D(impute_known()), D(impute_mask())) if tag == "impute_r5" else None
    args = dict(noise=xT, clip_denoised=clip, denoised_fn=imp, model_kwargs=_kw(g), step_noise=nz)
    w = GuidedCMDM(cmdm, _scales())
    native = d.p_sample_loop(w, SHAPE, **args)
    report(f"two-scale native DDPM loop {tag}", native, want, TOL_LOOP[tag])
    from oracle import diffusion_ref as df
    sd64, g64 = _twin()
    model64 = guided2_oracle(sd64, g64, ORDERS["pc_text"], torch.float64)
    if imp is not None:
        model64 = imputed(model64)
        assert torch.equal(native.cpu()[impute_mask()], impute_known()[impute_mask()])
    want64 = df.p_sample_loop(df.Schedule(1000, "cosine", "5"), model64, xT.cpu().double(), list(nz.cpu().double()), clip_denoised=clip)
    report_f32_class(f"two-scale native DDPM loop {tag}", native, want, want64, TOL_LOOP[tag])
    assert torch.equal(native, _last(d.p_sample_loop_progressive(w, SHAPE, **args)))      # the same kernels compute the same bits
    assert torch.equal(native, d.p_sample_loop(w, SHAPE, progress=True, **args))
    snaps = {1: None, d.num_timesteps - 1: None}
    assert torch.equal(native, d.p_sample_loop(w, SHAPE, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
    wm = GuidedCMDM(cmdm, _scales(), force_masked=True)
    masked = d.p_sample_loop(wm, SHAPE, **args)
    report(f"two-scale native DDPM loop {tag}, masked u", masked, want, TOL_LOOP[tag])
    report_f32_class(f"two-scale native DDPM loop {tag}, masked u", masked, want, want64, TOL_LOOP[tag])
    assert torch.equal(masked, _last(d.p_sample_loop_progressive(wm, SHAPE, **args)))
    if tag == "r5":             # L = 15: 3945 values per sample, the update's last quad and its K-padded row copy end on a partial quad
        odd = (2, 15, 263)
        kw = dict(c_text_feat=D(g["text_feat"]), c_cont_emb=D(g["cont_emb"]), x_mask=D(synth.frame_mask(2, 15, min_len=8)))
        oargs = dict(noise=D(synth.gaussian("loop_r5_L15_xT", odd)), clip_denoised=clip, model_kwargs=kw,
                     step_noise=D(torch.stack([synth.gaussian(f"loop_r5_L15_{j}", odd) for j in range(d.num_timesteps)])))
        assert torch.equal(d.p_sample_loop(w, odd, **oargs), _last(d.p_sample_loop_progressive(w, odd, **oargs)))


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_loop_vs_reference_golden(cmdm, eta):
    d, nz, xT = _loop_inputs("ddim50", "ddim_loop_ddim50")
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_cfg2_ddim_loop_ddim50_eta{int(eta)}")["sample"]
    w = GuidedCMDM(cmdm, _scales())
    args = dict(noise=xT, clip_denoised=False, model_kwargs=_kw(g), eta=eta, step_noise=nz)
    native = d.ddim_sample_loop(w, SHAPE, **args)
    report(f"two-scale native DDIM loop ddim50 eta={eta}", native, want, TOL_DDIM[eta])
    sd64, g64 = _twin()
    want64 = ddim_loop_ref(guided2_oracle(sd64, g64, ORDERS["pc_text"], torch.float64), xT.cpu().double(), list(nz.cpu().double()), eta)
    report_f32_class(f"two-scale native DDIM loop ddim50 eta={eta}", native, want, want64, TOL_DDIM[eta])
    assert torch.equal(native, _last(d.ddim_sample_loop_progressive(w, SHAPE, **args)))
    assert torch.equal(native, d.ddim_sample_loop(w, SHAPE, progress=True, **args))


# Measured on the MI355X (max over the parametrised cases), each bound <= 20x its measurement and <= its ceiling:
TOL_FWD_BRANCH = 8e-5              # x0_c 4.1e-6, x0_a 3.6e-6, x0_u 3.3e-6 (masked form 3.6e-6); ceiling FWD = 2e-4
TOL_FWD_GUIDED = 5.9e-4            # guided forward 3.0e-5 (masked u 2.8e-5), p_sample pred_xstart 2.8e-5; ceiling FWD * AMP = 2.8e-3
TOL_PSAMPLE = 4.7e-6               # p_sample sample at t = 500: 2.4e-7 (coef1 is small there)
TOL_LOOP = {"r5": 5.9e-4,          # 3.0e-5, masked u 2.8e-5; ceiling LOOP * AMP = 1.4e-2
            "r5_clip": 5.8e-4,     # 2.9e-5, masked u 2.6e-5
            "impute_r5": 6.1e-4}   # 3.1e-5, masked u 2.8e-5
TOL_DDIM = {0.0: 5.1e-4,           # 2.6e-5; ceiling DDIM_LOOP * AMP = 8.4e-4
            1.0: 5.8e-4}           # 2.9e-5
assert TOL_FWD_BRANCH <= FWD and max(TOL_FWD_GUIDED, TOL_PSAMPLE) <= FWD * AMP and all(b <= LOOP * AMP for b in TOL_LOOP.values()) \
    and all(b <= DDIM_LOOP * AMP for b in TOL_DDIM.values())


# ---------------------------------------------------------------------------------------------------------------- forms, exact
def _batch3():
    B, L = 3, 16
    kw = dict(c_text_feat=D(synth.text_feature(B)), c_cont_emb=D(synth.gaussian("cfg2_shard_cont", (B, 16, 256))),
              x_mask=D(synth.frame_mask(B, L, min_len=8)))
    scales = {"pc": torch.tensor([1.5, 2.5, 0.0], device=dev()), "text": torch.tensor([2.5, 7.5, 1.0], device=dev())}      # (zero and one: no shortcut)
    return B, L, kw, scales


def test_one_sub_batch_stream_equals_two_at_an_uneven_split(cmdm):
    """B = 3: sub-batches of 2 + 1 on two streams against one stream; AFM_CMDM_PAIR_LAUNCH is ignored (the loop runs unpaired)."""
    B, L, kw, scales = _batch3()
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    imp = Impute(D(synth.gaussian("cfg2_b3_known", (B, L, 263))), D(synth.gaussian("cfg2_b3_mask", (B, L, 263)) > 0))
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        for order in ORDERS.values():
            w = GuidedCMDM(cmdm, {k: scales[k] for k in order})
            runs = (lambda: d5.p_sample_loop(w, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=4),
                    lambda: d5.p_sample_loop(w, (B, L, 263), clip_denoised=True, denoised_fn=imp, model_kwargs=kw, seed=4),
                    lambda: dd.ddim_sample_loop(w, (B, L, 263), clip_denoised=True, model_kwargs=kw, eta=1.0, seed=4))
            for run in runs:
                cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
                one = run()
                cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
                two = run()
                cmdm.pair_launch = True
                assert torch.equal(one, two) and torch.equal(one, run()), order
                cmdm.pair_launch = False
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved
    w.branch_streams = True                                     # (set behind the constructor's refusal: the loop refuses it too)
    with pytest.raises(ValueError, match="branch streams"):
        d5.p_sample_loop(w, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=4)


@pytest.mark.parametrize("form", ["two_scale", "one_scale_compact", "one_scale_masked"])
def test_every_guided_form_at_an_uneven_split_and_a_partial_quad(cmdm, form):
    """B = 3, L = 15 (sub-batches of 2 + 1; 3945 values per sample: the update's last quad and the K-padded row copy end on a partial
    quad), {DDPM, DDIM eta = 0.5} x {no imputation, Impute}: two sub-batch streams and the step-by-step loop through the same wrapper
    are the native one-stream loop bit for bit - what a wrong branch order, workspace alias or stream would break."""
    B, L = 3, 15
    _, _, kw, scales = _batch3()
    kw = dict(kw, x_mask=D(synth.frame_mask(B, L, min_len=8)))
    w = GuidedCMDM(cmdm, scales) if form == "two_scale" else GuidedCMDM(cmdm, scales["text"], force_masked=form == "one_scale_masked")
    imp = Impute(D(synth.gaussian("cfg2_b3_L15_known", (B, L, 263))), D(synth.gaussian("cfg2_b3_L15_mask", (B, L, 263)) > 0))
    loops = {"ddpm": (create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5")), "p_sample_loop", {}),
             "ddim": (create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5")), "ddim_sample_loop", {"eta": 0.5})}
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        for name, (d, loop, extra) in loops.items():
            args = dict(noise=D(synth.gaussian(f"cfg2_b3_L15_{name}_xT", (B, L, 263))), clip_denoised=True, model_kwargs=kw,
                        step_noise=D(torch.stack([synth.gaussian(f"cfg2_b3_L15_{name}_{j}", (B, L, 263)) for j in range(d.num_timesteps)])), **extra)
            for fn in (None, imp):
                cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
                one = getattr(d, loop)(w, (B, L, 263), denoised_fn=fn, **args)
                assert torch.equal(one, _last(getattr(d, loop + "_progressive")(w, (B, L, 263), denoised_fn=fn, **args))), (name, fn)
                cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
                assert torch.equal(one, getattr(d, loop)(w, (B, L, 263), denoised_fn=fn, **args)), (name, fn)
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


def test_a_batch_of_three_equals_its_samples_run_in_shards(cmdm):
    B, L, kw, scales = _batch3()
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    full = d.p_sample_loop(GuidedCMDM(cmdm, scales), (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=21)
    parts = [d.p_sample_loop(GuidedCMDM(cmdm, {k: v[lo:hi] for k, v in scales.items()}), (hi - lo, L, 263), clip_denoised=False,
                             model_kwargs={k: v[lo:hi] for k, v in kw.items()}, seed=21, sample_index0=lo) for lo, hi in ((0, 2), (2, 3))]
    assert torch.equal(torch.cat(parts, 0), full)
    assert not torch.equal(full, d.p_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=21))


def test_equal_scales_are_the_single_scale_function_but_not_its_bits(cmdm):
    """s_pc = s_text = s: u + s (a - u) + s (c - a) is u + s (c - u) in exact arithmetic, and c itself at s = 1.  The product takes no
    shortcut, so the results agree to the roundings of the two expressions on the same branches, and nothing claims more.  Every rounding
    is at most half an ulp of a value no larger than (2 s + 1) max|branch|, that is 2^-23 (2 s + 1) max|branch|."""
    g = golden("cmdm_forward_N1024_L16")
    x, t = D(g["x"]), torch.tensor([500, 500], device=dev())
    s = torch.tensor([2.5, 7.5], device=dev())
    c, a, u, gd2 = GuidedCMDM(cmdm, {"pc": s, "text": s}).branches(x, t, **_kw(g))
    top = max(v.abs().max().item() for v in (c, a, u))
    gd1 = GuidedCMDM(cmdm, s)(x, t, **_kw(g))
    report("equal scales vs the single-scale wrapper", gd2, gd1, (6 + 3) * 2.0 ** -23 * (2 * 7.5 + 1) * top)      # 6 + 3 roundings
    one = GuidedCMDM(cmdm, {"pc": 1.0, "text": 1.0})(x, t, **_kw(g))
    report("both scales 1 vs the conditioned branch", one, c, 4 * 2.0 ** -23 * 2 * top)                            # 4 roundings (s * v is exact)


# ---------------------------------------------------------------------------------------------------------------- launches
def test_two_scale_jobs_launch_no_eager_arithmetic_and_the_derived_launch_counts(cmdm):
    g = golden("cmdm_forward_N1024_L16")
    n = 6
    dd = {k: create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{k}")) for k in (n, n // 2)}
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=str(n)))
    dens = {"unguided": cmdm, "one_scale": GuidedCMDM(cmdm, 2.5), "two_scales": GuidedCMDM(cmdm, {"pc": 1.5, "text": 5.0})}
    count = lambda names, pat: sum(c for k, c in names.items() if pat in k)
    kernels = lambda names: sum(c for k, c in names.items() if not _MOVERS.search(k))
    fused = ("cfg_combine_kernel", "cfg2_combine_kernel", "impute_kernel", "clamp_kernel")
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        names = {}
        for k, den in dens.items():                              # eta = 0: no noise launches - forwards, updates and the schedule rows only
            for steps, d in dd.items():
                run = lambda: d.ddim_sample_loop(den, SHAPE, clip_denoised=True, model_kwargs=_kw(g), eta=0.0, seed=5)
                run()                                            # (weight pack, workspaces and streams exist before anything is counted)
                torch.cuda.synchronize()
                names[k, steps] = _device_kernel_names(run)
                _check(names[k, steps], f"native DDIM loop ({k}, {steps} steps)")
        # kernels per step, from loops of n and n / 2 steps (what a loop launches once - rows, the first step's prologue - drops out)
        per_step = {k: (kernels(names[k, n]) - kernels(names[k, n // 2])) / (n - n // 2) for k in dens}
        updates = {k: (count(names[k, n], "sampling_update_kernel") - count(names[k, n // 2], "sampling_update_kernel")) / (n - n // 2) for k in dens}
        print(f"[cfg2 launches] kernels per step {per_step}, update launches per step {updates}, "
              f"per loop of {n}: {({k: kernels(names[k, n]) for k in dens})}")
        forward = per_step["unguided"] - updates["unguided"]     # the launches of one forward inside a loop, derived from the unguided loop
        assert forward > 0 and per_step["two_scales"] == per_step["one_scale"] + forward
        for k in dens:
            assert count(names[k, n], "sampling_update_kernel") == n, k
        for pat in fused:
            assert count(names["two_scales", n], pat) == 0, pat  # combination, select and clamp ride in the update launch
        # the DDPM loop with imputation, noise drawn by the loop
        imp = Impute(D(impute_known()), D(impute_mask()))
        run = lambda: d5.p_sample_loop(dens["two_scales"], SHAPE, clip_denoised=True, denoised_fn=imp, model_kwargs=_kw(g), seed=5)
        run()
        torch.cuda.synchronize()
        ddpm = _device_kernel_names(run)
        _check(ddpm, "two-scale imputing DDPM loop")
        assert count(ddpm, "sampling_update_kernel") == n and not any(p in k for k in ddpm for p in fused), ddpm
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # the single forward: three forwards and the stand-alone combine launch
    torch.cuda.synchronize()
    fwd = _device_kernel_names(lambda: dens["two_scales"](D(g["x"]), torch.tensor([1, 2], device=dev()), **_kw(g)))
    _check(fwd, "two-scale forward")
    assert count(fwd, "cfg2_combine_kernel") == 1 and count(fwd, "sampling_update_kernel") == 0


# ---------------------------------------------------------------------------------------------------------------- two stages
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_two_stage_sample_with_a_scale_per_condition(cmdm, cdm):
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    B, N, L = 2, 1024, 16
    text, xyz = D(synth.text_feature(B)), D(synth.scene_cloud(B, N, seed=14))
    args = dict(text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9)
    base = two_stage_sample(cdm, d_adm, cmdm, d_amdm, **args)
    scales = {"pc": 1.5, "text": torch.tensor([2.5, 7.5], device=dev())}
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=scales, **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"])
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=base["cond"], x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    by_hand = d_amdm.p_sample_loop(GuidedCMDM(cmdm, scales), (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=10)
    assert torch.equal(got["motion"], by_hand) and not torch.equal(got["motion"], base["motion"])
    swapped = two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=dict(reversed(list(scales.items()))), guidance_drop=("pc", "text"), **args)
    assert not torch.equal(swapped["motion"], got["motion"])    # the order of the mapping names (first, second)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=scales, sampler="ddim", eta=0.5, **args))
    _check(names, "two-scale two-stage (ddim)")
    assert any("sampling_update_kernel" in n for n in names)


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table -> profiles/cfg2_parity.json)."""
    write_parity_table()
