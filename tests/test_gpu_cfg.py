"""`-m gpu`: classifier-free guided sampling of the CMDM (afm.cmdm.GuidedCMDM, the guided native loops) against the CPU float32
expression, the product's own forms against each other (bit for bit), the reference goldens of tools/make_goldens_cfg.py and the oracle.

Bounds against the reference: at most 20x the error measured on the MI355X (in the comment beside each), and never above the bound of the
matching unguided test times AMP = |s| + |1 - s| = 14 for the largest scale, 7.5.  Beside every report() against a reference golden or an
oracle loop stands report_f32_class (tests/gpu_util.py): the HIP error against the float64 twin of the guided oracle
(tests/test_cfg_host.py::guided_oracle on float64 weights and inputs) is at most 4 x the float32 reference's own error against that
twin, plus one float32 ulp of the largest output - the guidance amplifies both sides alike."""
import pytest
import torch

from afm import ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report, report_f32_class, to_f64, write_parity_table
from test_cfg_host import guided_oracle
from test_gpu_cdm import cdm_cfg
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _check, _device_kernel_names

pytestmark = pytest.mark.gpu
SHAPE = (2, 16, 263)
DROPS = {"both": ("text", "pc"), "text": ("text",), "pc": ("pc",)}
AMP = 7.5 + 6.5
FWD, LOOP, DDIM_LOOP = 2e-4, 1e-3, 6e-5          # the unguided bounds: test_gpu_cmdm.py forward / p_sample, DDPM loops; test_gpu_ddim.py loops


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


def _scale():
    return torch.tensor([2.5, 7.5], device=dev())


def _loop_inputs(resp, prefix):
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=resp))
    nz = torch.stack([synth.gaussian(f"{prefix}_{j}", SHAPE) for j in range(d.num_timesteps)]).to(dev())
    return d, nz, synth.gaussian(f"{prefix}_xT", SHAPE).to(dev())


def _last(gen):
    out = None
    for out in gen:
        pass
    return out["sample"]


# ---------------------------------------------------------------------------------------------------------------- kernels, exact
def _cpu_guided(c, u, s, clip):
    g = u + s.view(-1, 1, 1) * (c - u)
    return g.clamp(-1, 1) if clip else g


@pytest.mark.parametrize("clip", [False, True])
def test_combine_and_guided_update_kernels_equal_the_cpu_expression(clip):
    g = golden("cmdm_cfg_forward_both_t500")
    D = lambda t: t.to(dev())
    assert torch.equal(ops.cfg_combine(D(g["x0_c"]), D(g["x0_u"]), D(g["scale"])).cpu(), g["guided"])
    d = create_gaussian_diffusion(cmdm_cfg())
    tab = d.tables(dev())
    # (3, 5, 263): 1315 values per sample, not a multiple of 4 - the last quad of a sample is partial
    odd = (3, 5, 263)
    cases = ((g["x0_c"], g["x0_u"], g["scale"], synth.gaussian("cmdm_x", SHAPE), synth.gaussian("p_sample_noise_500", SHAPE)),
             (*(synth.gaussian(f"cfg_odd_{n}", odd) for n in ("c", "u")), torch.tensor([2.5, 7.5, 0.0]),
              *(synth.gaussian(f"cfg_odd_{n}", odd) for n in ("x", "nz"))))
    for c, u, s, x, nz in cases:
        shape = tuple(x.shape)
        assert torch.equal(ops.cfg_combine(D(c), D(u), D(s)).cpu(), _cpu_guided(c, u, s, False))
        x0 = _cpu_guided(c, u, s, clip)
        for tt in (999, 500, 1, 0):
            t = torch.tensor([tt, 3, 0][:shape[0]], device=dev())
            c1, c2, sg = tab.coef1[t], tab.coef2[t], tab.sigma[t]
            v = lambda r: r.cpu().view(-1, 1, 1)
            want = (v(c1) * x0 + v(c2) * x) + v(sg) * nz
            got = ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip)
            assert torch.equal(got.cpu(), want), ("ddpm", tt, shape)
            # the three-launch composition of the step-by-step path gives the same bits
            x0d = ops.cfg_combine(D(c), D(u), D(s))
            if clip:
                x0d = ops.clamp_(x0d, -1.0, 1.0)
            assert torch.equal(got, ops.ddpm_step(x0d, D(x), D(nz), c1, c2, sg))
            phil = ops.cfg_step(D(c), D(u), D(s), D(x), None, ddpm=(c1, c2, sg), clip=clip, seed=11, sample_index0=3, step=7)
            given = ops.randn(shape, dev(), seed=11, sample_index0=3, step=7)
            assert torch.equal(phil, ops.cfg_step(D(c), D(u), D(s), D(x), given, ddpm=(c1, c2, sg), clip=clip))
            for eta in (0.0, 1.0):
                rows = d.ddim_tables(dev(), eta)
                a, b, cc, dd = (r[t] for r in (rows.a, rows.b, rows.c, rows.d))
                sgd = None if rows.sigma is None else rows.sigma[t]
                eps = (v(a) * x - x0) / v(b)
                want = x0 * v(cc) + v(dd) * eps
                if sgd is not None:
                    want = want + v(sgd) * nz
                got = ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddim=(a, b, cc, dd, sgd), clip=clip)
                assert torch.equal(got.cpu(), want), ("ddim", tt, eta, shape)
                assert torch.equal(got, ops.ddim_step(x0d, D(x), D(nz), a, b, cc, dd, sgd))
        out = D(x).clone()                                       # in place on x_t, as the loops run it
        ops.cfg_step(D(c), D(u), D(s), out, D(nz), ddpm=(c1, c2, sg), clip=clip, out=out)
        assert torch.equal(out, ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip))


# ---------------------------------------------------------------------------------------------------------------- reference goldens
def _twin():
    """Float64 state dict and conditions of the goldens' case, for guided_oracle and the oracle's branches."""
    from oracle import shapes as sh
    return to_f64(sh.weights(sh.cmdm())), to_f64(golden("cmdm_forward_N1024_L16"))


def _branches64(sd64, g64, x, t, drop):
    from oracle import denoiser_ref as dr
    ones = torch.ones(x.shape[0], 1, dtype=torch.bool)
    sw = {f"c_{k}_mask": ones for k in drop}
    base = dict(x_mask=g64["x_mask"], cont_emb=g64["cont_emb"])
    return dr.cmdm_forward(sd64, x, t, g64["text_feat"], **base), dr.cmdm_forward(sd64, x, t, g64["text_feat"], **base, **sw)


@pytest.mark.parametrize("tt", [999, 500, 0])
def test_guided_forward_vs_reference_golden(cmdm, tt):
    g = golden("cmdm_forward_N1024_L16")
    t = torch.tensor([tt, tt], device=dev())
    with torch.no_grad():                                     # (the fused inference forward, as p_sample calls the denoiser)
        plain = cmdm(g["x"].to(dev()), t, **_kw(g))
    for k, drop in DROPS.items():
        gg = golden(f"cmdm_cfg_forward_{k}_t{tt}")
        w = GuidedCMDM(cmdm, _scale(), drop)
        c, u, gd = w.branches(g["x"].to(dev()), t, **_kw(g))
        assert torch.equal(c, plain)                          # the conditioned branch IS the unguided forward
        assert torch.equal(gd, ops.cfg_combine(c, u, _scale())) and torch.equal(gd, w(g["x"].to(dev()), t, **_kw(g)))
        report(f"guided forward t={tt} drop={k}: x0_c", c, gg["x0_c"], TOL_FWD_BRANCH)
        report(f"guided forward t={tt} drop={k}: x0_u", u, gg["x0_u"], TOL_FWD_BRANCH)
        report(f"guided forward t={tt} drop={k}: guided", gd, gg["guided"], TOL_FWD_GUIDED)
        sd64, g64 = _twin()
        c64, u64 = _branches64(sd64, g64, g64["x"], t.cpu(), drop)
        gd64 = guided_oracle(sd64, g64, _scale().cpu().double(), drop)(g64["x"], t.cpu())
        report_f32_class(f"guided forward t={tt} drop={k}: x0_c", c, gg["x0_c"], c64, TOL_FWD_BRANCH)
        report_f32_class(f"guided forward t={tt} drop={k}: x0_u", u, gg["x0_u"], u64, TOL_FWD_BRANCH)
        report_f32_class(f"guided forward t={tt} drop={k}: guided", gd, gg["guided"], gd64, TOL_FWD_GUIDED)
        if k == "both":                                       # the masked full-length form of the same branch
            um = GuidedCMDM(cmdm, _scale(), drop, force_masked=True).branches(g["x"].to(dev()), t, **_kw(g))[1]
            report(f"guided forward t={tt}: x0_u, masked form", um, gg["x0_u"], TOL_FWD_BRANCH)
            report_f32_class(f"guided forward t={tt}: x0_u, masked form", um, gg["x0_u"], u64, TOL_FWD_BRANCH)
            report(f"guided forward t={tt}: compact vs masked form", u, um, TOL_FWD_FORMS)


def test_guided_p_sample_vs_reference_golden(cmdm):
    g, gs = golden("cmdm_forward_N1024_L16"), golden("cmdm_cfg_p_sample_t500")
    d = create_gaussian_diffusion(cmdm_cfg())
    out = d.p_sample(GuidedCMDM(cmdm, _scale()), g["x"].to(dev()), torch.tensor([500, 500], device=dev()), clip_denoised=False,
                     model_kwargs=_kw(g), noise=synth.gaussian("p_sample_noise_500", SHAPE).to(dev()))
    report("guided p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], TOL_FWD_GUIDED)
    report("guided p_sample t=500 sample", out["sample"], gs["sample"], TOL_PSAMPLE)
    from oracle import diffusion_ref as df
    sd64, g64 = _twin()
    w64 = df.p_sample(df.Schedule(1000), guided_oracle(sd64, g64, _scale().cpu().double(), DROPS["both"]), g64["x"], torch.tensor([500, 500]),
                      synth.gaussian("p_sample_noise_500", SHAPE).double())
    report_f32_class("guided p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], w64["pred_xstart"], TOL_FWD_GUIDED)
    report_f32_class("guided p_sample t=500 sample", out["sample"], gs["sample"], w64["sample"], TOL_PSAMPLE)


@pytest.mark.parametrize("tag,drop,clip", [("r5", "both", False), ("r5_clip", "both", True), ("r5_text", "text", False)])
def test_guided_ddpm_loop_vs_reference_golden(cmdm, tag, drop, clip):
    """Native guided loop (afm_cmdm_cfg_sample_loop_range) and the step-by-step loop through the same wrapper against the reference."""
    d, nz, xT = _loop_inputs("5", "loop_r5")
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_cfg_loop_{tag}")["sample"]
    w = GuidedCMDM(cmdm, _scale(), DROPS[drop])
    native = d.p_sample_loop(w, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz)
    report(f"guided native DDPM loop {tag}", native, want, TOL_LOOP[tag])
    from oracle import diffusion_ref as df
    sd64, g64 = _twin()
    want64 = df.p_sample_loop(df.Schedule(1000, "cosine", "5"), guided_oracle(sd64, g64, _scale().cpu().double(), DROPS[drop]), xT.cpu().double(),
                              list(nz.cpu().double()), clip_denoised=clip)
    report_f32_class(f"guided native DDPM loop {tag}", native, want, want64, TOL_LOOP[tag])
    generic = _last(d.p_sample_loop_progressive(w, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz))
    assert torch.equal(native, generic)                       # the same kernels and forms compute the same bits
    assert torch.equal(native, d.p_sample_loop(w, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz, progress=True))
    snaps = {1: None, d.num_timesteps - 1: None}
    assert torch.equal(native, d.p_sample_loop(w, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz, snapshots=snaps))
    assert all(v is not None for v in snaps.values())
    if tag == "r5":             # L = 15: 3945 values per sample, the update's last quad and its K-padded row copy end on a partial quad
        odd = (2, 15, 263)
        kw = dict(c_text_feat=g["text_feat"].to(dev()), c_cont_emb=g["cont_emb"].to(dev()), x_mask=synth.frame_mask(2, 15, min_len=8).to(dev()))
        onz = torch.stack([synth.gaussian(f"loop_r5_L15_{j}", odd) for j in range(d.num_timesteps)]).to(dev())
        oxT = synth.gaussian("loop_r5_L15_xT", odd).to(dev())
        assert torch.equal(d.p_sample_loop(w, odd, noise=oxT, clip_denoised=clip, model_kwargs=kw, step_noise=onz),
                           _last(d.p_sample_loop_progressive(w, odd, noise=oxT, clip_denoised=clip, model_kwargs=kw, step_noise=onz)))
    if drop == "both":                                        # the masked form: another place of the attention's key blocks, the same function
        wm = GuidedCMDM(cmdm, _scale(), DROPS[drop], force_masked=True)
        masked = d.p_sample_loop(wm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz)
        report(f"guided native DDPM loop {tag}, masked form", masked, want, TOL_LOOP[tag])
        report_f32_class(f"guided native DDPM loop {tag}, masked form", masked, want, want64, TOL_LOOP[tag])
        assert torch.equal(masked, _last(d.p_sample_loop_progressive(wm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), step_noise=nz)))


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_guided_ddim_loop_vs_reference_golden(cmdm, eta):
    d, nz, xT = _loop_inputs("ddim50", "ddim_loop_ddim50")
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_cfg_ddim_loop_ddim50_eta{int(eta)}")["sample"]
    w = GuidedCMDM(cmdm, _scale())
    native = d.ddim_sample_loop(w, SHAPE, noise=xT, clip_denoised=False, model_kwargs=_kw(g), eta=eta, step_noise=nz)
    report(f"guided native DDIM loop ddim50 eta={eta}", native, want, TOL_DDIM[eta])
    generic = _last(d.ddim_sample_loop_progressive(w, SHAPE, noise=xT, clip_denoised=False, model_kwargs=_kw(g), eta=eta, step_noise=nz))
    assert torch.equal(native, generic)
    assert torch.equal(native, d.ddim_sample_loop(w, SHAPE, noise=xT, clip_denoised=False, model_kwargs=_kw(g), eta=eta, step_noise=nz, progress=True))
    clipped = d.ddim_sample_loop(w, SHAPE, noise=xT, clip_denoised=True, model_kwargs=_kw(g), eta=eta, step_noise=nz)
    assert torch.equal(clipped, _last(d.ddim_sample_loop_progressive(w, SHAPE, noise=xT, clip_denoised=True, model_kwargs=_kw(g), eta=eta,
                                                                       step_noise=nz)))
    assert not torch.equal(clipped, native)


# Measured on the MI355X (max over the parametrised cases), each bound <= 20x its measurement and <= its ceiling:
TOL_FWD_BRANCH = 8e-5              # x0_c 4.1e-6, x0_u 3.6e-6 (compact and masked forms); ceiling FWD = 2e-4
TOL_FWD_FORMS = 4e-5               # compact vs masked form of x0_u, L = 16: 2.1e-6; ceiling FWD
TOL_FWD_GUIDED = 6e-4              # guided forward / p_sample pred_xstart 3.2e-5; ceiling FWD * AMP = 2.8e-3
TOL_PSAMPLE = 4.8e-6               # guided p_sample sample at t = 500: 2.4e-7 (coef1 is small there)
TOL_LOOP = {"r5": 2.0e-3,          # compact 1.0e-4, masked 1.2e-4; ceiling LOOP * AMP = 1.4e-2
            "r5_clip": 8.8e-4,     # compact 5.2e-5, masked 4.4e-5
            "r5_text": 6.9e-4}     # 3.5e-5
TOL_DDIM = {0.0: DDIM_LOOP * AMP,  # 8.3e-5: 20x is above the ceiling DDIM_LOOP * AMP = 8.4e-4, so the ceiling
            1.0: DDIM_LOOP * AMP}  # 1.9e-4
TOL_COMPACT_FULL = 4.4e-5          # compact vs masked x0_u at T = 326: 2.2e-6; ceiling FWD
TOL_FULL_LOOP = 3.8e-3             # 20-step guided loop at T = 326 vs the oracle: 1.9e-4; ceiling LOOP * AMP


# ---------------------------------------------------------------------------------------------------------------- forms, exact
def test_sub_batch_streams_are_bit_identical(cmdm):
    g = golden("cmdm_forward_N1024_L16")
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        for drop in DROPS.values():
            w = GuidedCMDM(cmdm, _scale(), drop)
            runs = (lambda: d5.p_sample_loop(w, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=4),
                    lambda: dd.ddim_sample_loop(w, SHAPE, clip_denoised=True, model_kwargs=_kw(g), eta=1.0, seed=4))
            for run in runs:
                cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
                one = run()
                cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
                two = run()
                cmdm.pair_launch = True                       # ignored by a guided loop: it runs unpaired
                assert torch.equal(one, two) and torch.equal(one, run())
                cmdm.pair_launch = False
                w.branch_streams = True                       # the other placement: the unconditioned branch on a stream of its own
                try:
                    assert torch.equal(one, run())            # two sub-batches, four streams
                    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True
                    assert torch.equal(one, run())            # one sub-batch, two streams
                finally:
                    w.branch_streams = False
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


def test_guided_loop_without_riders_is_bit_identical(cmdm):
    """no_riders: the prologue (and behind it the key-mask launch of the masked form) runs in every step instead of the first only."""
    g = golden("cmdm_forward_N1024_L16")
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    saved = cmdm.no_riders
    try:
        for drop in DROPS.values():
            w = GuidedCMDM(cmdm, _scale(), drop)
            cmdm.no_riders = False
            riders = d.p_sample_loop(w, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=8)
            cmdm.no_riders = True
            assert torch.equal(riders, d.p_sample_loop(w, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=8)), drop
    finally:
        cmdm.no_riders = saved


def test_a_batch_of_four_equals_its_samples_run_alone(cmdm):
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    B, L = 4, 16
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_cont_emb=synth.gaussian("cfg_shard_cont", (B, 16, 256)).to(dev()),
              x_mask=synth.frame_mask(B, L, min_len=8).to(dev()))
    scale = torch.tensor([2.5, 7.5, 0.0, 1.0], device=dev())
    for drop in (DROPS["both"], DROPS["pc"]):
        full = d.p_sample_loop(GuidedCMDM(cmdm, scale, drop), (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=21)
        alone = [d.p_sample_loop(GuidedCMDM(cmdm, scale[i:i + 1], drop), (1, L, 263), clip_denoised=False,
                                 model_kwargs={k: v[i:i + 1] for k, v in kw.items()}, seed=21, sample_index0=i) for i in range(B)]
        assert torch.equal(torch.cat(alone, 0), full), drop
    # scale 1 is the conditioned branch up to the rounding of u + (c - u); scale 0 is the unconditioned branch exactly
    plain = d.p_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=21)
    report("scale = 1 vs the unguided loop", full[3:], plain[3:], 1e-5)


def test_in_kernel_philox_noise_equals_the_same_noise_passed_in(cmdm):
    g = golden("cmdm_forward_N1024_L16")
    w = GuidedCMDM(cmdm, _scale())
    for d, loop, extra in ((create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="20")), "p_sample_loop", {}),
                           (create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim20")), "ddim_sample_loop", {"eta": 1.0})):
        xT = ops.randn(SHAPE, dev(), seed=6, sample_index0=5, step=-1)
        nz = torch.stack([ops.randn(SHAPE, dev(), seed=6, sample_index0=5, step=j) for j in range(d.num_timesteps)])
        a = getattr(d, loop)(w, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=6, sample_index0=5, **extra)
        b = getattr(d, loop)(w, SHAPE, noise=xT, clip_denoised=False, model_kwargs=_kw(g), step_noise=nz, **extra)
        assert torch.equal(a, b), loop


@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_two_stage_sample_with_and_without_guidance(cmdm, cdm):
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    B, N, L = 2, 1024, 16
    text, xyz = synth.text_feature(B).to(dev()), synth.scene_cloud(B, N, seed=14).to(dev())
    args = dict(text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9)
    base = two_stage_sample(cdm, d_adm, cmdm, d_amdm, **args)
    none = two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=None, **args)
    assert all(torch.equal(base[k], none[k]) for k in base)
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=2.5, guidance_drop=("text",), **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"])
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=base["cond"], x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    by_hand = d_amdm.p_sample_loop(GuidedCMDM(cmdm, 2.5, ("text",)), (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=10)
    assert torch.equal(got["motion"], by_hand) and not torch.equal(got["motion"], base["motion"])
    for sampler in ("ddpm", "ddim"):
        torch.cuda.synchronize()
        names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, d_amdm, guidance_scale=7.5, sampler=sampler, eta=0.5, **args))
        _check(names, f"guided two-stage ({sampler})")
        assert any("sampling_update_kernel" in n for n in names) or not names


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _LoopArgumentProbe:
    """The loaded library with its loop entry points wrapped: in front of every real call of one, the same call with a workspace one byte
    too small (AFM_E_WORKSPACE = -2) and with a NULL timestep map (AFM_E_BADARG = -1).  Both return before anything is enqueued.  The two
    entry points without `first_step` get the same pair of calls with the arguments of their `_range` form."""
    TMAP = {"afm_cmdm": 5, "afm_cdm_": 7}            # position of d_timestep_map; workspace_bytes is the fourth argument from the end
    FIRST_STEP = {"afm_cmdm_sample_loop_range": 10, "afm_cdm_sample_loop_range": 12}

    def __init__(self, lib):
        self.lib, self.seen = lib, set()

    def _errors(self, name, args):
        small, no_map = list(args), list(args)
        small[-4] -= 1
        no_map[self.TMAP[name[:8]]] = None
        assert getattr(self.lib, name)(*small) == -2, name
        assert getattr(self.lib, name)(*no_map) == -1, name
        self.seen.add(name)

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if "loop_range" not in name:
            return fn

        def call(*args):
            self._errors(name, args)
            if name in self.FIRST_STEP:
                i = self.FIRST_STEP[name]
                self._errors(name[:-len("_range")], args[:i] + args[i + 1:])
            return fn(*args)
        return call


def test_loop_argument_errors_leave_the_next_call_untouched(cmdm, cdm, monkeypatch):
    """Every loop entry point: a workspace one byte short -> AFM_E_WORKSPACE, a NULL schedule pointer -> AFM_E_BADARG, and the correct
    call behind them on the same process gives the result of a call without them, bit for bit."""
    from afm import ffi
    g = golden("cmdm_forward_N1024_L16")
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    dc = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    ckw = dict(c_text_feat=synth.text_feature(2).to(dev()), c_pc_xyz=synth.scene_cloud(2, 1024, seed=14).to(dev()))
    guided = GuidedCMDM(cmdm, _scale())
    runs = (lambda: d5.p_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=4),
            lambda: d5.ddim_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=_kw(g), eta=1.0, seed=4),
            lambda: d5.p_sample_loop(guided, SHAPE, clip_denoised=False, model_kwargs=_kw(g), seed=4),
            lambda: d5.ddim_sample_loop(guided, SHAPE, clip_denoised=False, model_kwargs=_kw(g), eta=1.0, seed=4),
            lambda: dc.p_sample_loop(cdm, (2, 1024, 6), clip_denoised=False, model_kwargs=ckw, seed=4),
            lambda: dc.ddim_sample_loop(cdm, (2, 1024, 6), clip_denoised=False, model_kwargs=ckw, eta=1.0, seed=4))
    want = [run().clone() for run in runs]
    probe = _LoopArgumentProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.seen == {"afm_cmdm_sample_loop", "afm_cmdm_sample_loop_range", "afm_cmdm_ddim_loop_range", "afm_cmdm_cfg_sample_loop_range",
                          "afm_cmdm_cfg_ddim_loop_range", "afm_cdm_sample_loop", "afm_cdm_sample_loop_range", "afm_cdm_ddim_loop_range"}
    assert all(torch.equal(a, b) for a, b in zip(want, got))


# ---------------------------------------------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def full():
    model = create_model(cmdm_cfg(num_points=8192), device=dev())
    load_named_weights(model)
    B, L = 2, 196
    text, cont, mask = synth.text_feature(B), synth.gaussian("full_cont", (B, 128, 256)), synth.frame_mask(B, L, seed=3)
    return model.to(dev()).eval(), text, cont, mask


def test_compact_form_against_masked_form_at_full_size(full):
    """L = 196, 128 contact tokens, T = 326: the unconditioned branch on 197 rows per sample against the same branch on all 326 rows with
    the 129 condition tokens key-masked.  They differ only in where the flash attention's key blocks fall."""
    model, text, cont, mask = full
    x, t = synth.gaussian("full_x", (2, 196, 263)).to(dev()), torch.tensor([999, 17], device=dev())
    kw = dict(c_text_feat=text.to(dev()), c_cont_emb=cont.to(dev()), x_mask=mask.to(dev()))
    c1, u1, g1 = GuidedCMDM(model, _scale()).branches(x, t, **kw)
    c2, u2, g2 = GuidedCMDM(model, _scale(), force_masked=True).branches(x, t, **kw)
    assert torch.equal(c1, c2)
    report("x0_u at T = 326: compact vs masked form", u1, u2, TOL_COMPACT_FULL)
    assert (c1 - u1).abs().max() > 0.1                        # the branches do differ


def test_full_size_guided_loop_vs_oracle(full):
    """B = 2, L = 196, T = 326, 20 respaced DDPM steps, shared explicit noise, default (benchmark) arithmetic: the native guided loop
    against the CPU oracle composed into a guided callable."""
    from oracle import denoiser_ref as dr, diffusion_ref as df, shapes as sh
    model, text, cont, mask = full
    B, L = 2, 196
    d = create_gaussian_diffusion(cmdm_cfg(num_points=8192, steps=1000, respacing="20"))
    xT = synth.gaussian("cfg_full_xT", (B, L, 263))
    nz = [synth.gaussian(f"cfg_full_nz{j}", (B, L, 263)) for j in range(20)]
    sd, s = sh.weights(sh.cmdm()), _scale().cpu().view(B, 1, 1)
    ones = torch.ones(B, 1, dtype=torch.bool)

    def guided(x, t, **k):
        c = dr.cmdm_forward(sd, x, t, text, x_mask=mask, cont_emb=cont)
        u = dr.cmdm_forward(sd, x, t, text, x_mask=mask, cont_emb=cont, c_text_mask=ones, c_pc_mask=ones)
        return u + s * (c - u)
    want = df.p_sample_loop(df.Schedule(1000, "cosine", "20"), guided, xT, nz)
    got = d.p_sample_loop(GuidedCMDM(model, _scale()), (B, L, 263), noise=xT.to(dev()), clip_denoised=False, step_noise=torch.stack(nz).to(dev()),
                          model_kwargs=dict(c_text_feat=text.to(dev()), c_cont_emb=cont.to(dev()), x_mask=mask.to(dev())))
    report("full-size 20-step guided loop vs oracle", got, want, TOL_FULL_LOOP)
    sd64, s64, text64, cont64 = to_f64(sd), s.double(), text.double(), cont.double()

    def guided64(x, t, **k):
        c = dr.cmdm_forward(sd64, x, t, text64, x_mask=mask, cont_emb=cont64)
        u = dr.cmdm_forward(sd64, x, t, text64, x_mask=mask, cont_emb=cont64, c_text_mask=ones, c_pc_mask=ones)
        return u + s64 * (c - u)
    want64 = df.p_sample_loop(df.Schedule(1000, "cosine", "20"), guided64, xT.double(), to_f64(nz))
    report_f32_class("full-size 20-step guided loop vs oracle", got, want, want64, TOL_FULL_LOOP)


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table -> profiles/r07_parity_f32_class.json)."""
    write_parity_table()
