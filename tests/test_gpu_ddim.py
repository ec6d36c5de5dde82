"""`-m gpu`: DDIM sampling (ddim_sample / ddim_reverse_sample / ddim_sample_loop) on the HIP path vs the reference's goldens
(tools/make_goldens_ddim.py), the CPU float32 expression, and the product's own forms against each other."""
import pytest
import torch

from afm import ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.config import to_config
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report
from test_gpu_cdm import cdm_cfg
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _check, _device_kernel_names

pytestmark = pytest.mark.gpu
SHAPE = (2, 16, 263)


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


def _cpu_update(x0, x, noise, rows, t):
    a, b, c, d = (r.cpu()[t] for r in (rows.a, rows.b, rows.c, rows.d))
    eps = (a * x - x0) / b
    mean = x0 * c + d * eps
    return mean if rows.sigma is None else mean + rows.sigma.cpu()[t] * noise


def _loop_inputs(resp):
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=resp))
    nz = torch.stack([synth.gaussian(f"ddim_loop_{resp}_{j}", SHAPE) for j in range(d.num_timesteps)]).to(dev())
    return d, nz, synth.gaussian(f"ddim_loop_{resp}_xT", SHAPE).to(dev())


@pytest.mark.parametrize("tt", [999, 500, 1, 0])
def test_ddim_step_kernel_equals_the_cpu_expression(tt):
    d = create_gaussian_diffusion(cmdm_cfg())
    g = golden(f"cmdm_ddim_sample_t{tt}")
    # (3, 5, 263): 1315 values per sample, not a multiple of 4 - the last quad of a sample is partial
    odd = tuple(synth.gaussian(f"ddim_odd_{n}", (3, 5, 263)) for n in ("x0", "x", "nz"))
    for x0, x, nz in ((g["pred_xstart"], g["x"], g["noise"]), odd):
        t = torch.full((x.shape[0],), tt, device=dev())
        for eta in (0.0, 0.5, 1.0):
            rows = d.ddim_tables(dev(), eta)
            sg = None if rows.sigma is None else rows.sigma[t]
            got = ops.ddim_step(x0.to(dev()), x.to(dev()), nz.to(dev()), rows.a[t], rows.b[t], rows.c[t], rows.d[t], sg).cpu()
            assert torch.equal(got, _cpu_update(x0, x, nz, rows, tt)), (tt, eta, x.shape)
            if sg is not None:          # noise=NULL: the in-kernel Philox draw equals afm_randn of the same keying
                phil = ops.ddim_step(x0.to(dev()), x.to(dev()), None, rows.a[t], rows.b[t], rows.c[t], rows.d[t], sg, seed=11, sample_index0=3, step=7)
                given = ops.randn(tuple(x.shape), dev(), seed=11, sample_index0=3, step=7)
                assert torch.equal(phil, ops.ddim_step(x0.to(dev()), x.to(dev()), given, rows.a[t], rows.b[t], rows.c[t], rows.d[t], sg,
                                                       seed=11, sample_index0=3, step=7))
        rows = d.ddim_tables(dev(), reverse=True)
        got = ops.ddim_step(x0.to(dev()), x.to(dev()), None, rows.a[t], rows.b[t], rows.c[t], rows.d[t], None).cpu()
        assert torch.equal(got, _cpu_update(x0, x, None, rows, tt))


@pytest.mark.parametrize("tt", [999, 500, 1, 0])
def test_ddim_sample_vs_reference_golden(cmdm, tt):
    d = create_gaussian_diffusion(cmdm_cfg())
    g, gs = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_ddim_sample_t{tt}")
    out = d.ddim_sample(cmdm, gs["x"].to(dev()), torch.tensor([tt, tt], device=dev()), clip_denoised=False, model_kwargs=_kw(g),
                        eta=float(gs["eta"]), noise=gs["noise"].to(dev()))
    report(f"ddim_sample t={tt} pred_xstart", out["pred_xstart"], gs["pred_xstart"], 8e-5)      # measured <= 4.1e-6
    report(f"ddim_sample t={tt} sample", out["sample"], gs["sample"], 5.5e-5)                   # measured <= 2.9e-6
    if tt == 500:
        gr = golden("cmdm_ddim_reverse_t500")
        rev = d.ddim_reverse_sample(cmdm, gr["x"].to(dev()), torch.tensor([500, 500], device=dev()), clip_denoised=False, model_kwargs=_kw(g))
        report("ddim_reverse_sample t=500 sample", rev["sample"], gr["sample"], 1.4e-5)        # measured 7.2e-7
        with pytest.raises(AssertionError):
            d.ddim_reverse_sample(cmdm, gr["x"].to(dev()), torch.tensor([500, 500], device=dev()), model_kwargs=_kw(g), eta=0.5)


@pytest.mark.parametrize("resp,eta,clip,tag", [("ddim50", 0.0, False, "ddim50_eta0"), ("ddim50", 1.0, False, "ddim50_eta1"),
                                               ("ddim5", 0.5, True, "ddim5_clip")])
def test_cmdm_ddim_loop_vs_reference_golden(cmdm, resp, eta, clip, tag):
    """Native loop (afm_cmdm_ddim_loop_range) and the generic step-by-step loop against the reference's ddim_sample_loop."""
    d, nz, xT = _loop_inputs(resp)
    if clip:
        xT = 2.0 * xT
    g = golden("cmdm_forward_N1024_L16")
    want = golden(f"cmdm_ddim_loop_{tag}")["sample"]
    native = d.ddim_sample_loop(cmdm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), eta=eta, step_noise=nz)
    report(f"CMDM native DDIM loop {tag}", native, want, 6e-5)            # measured <= 3.3e-6 (the DDPM loop tests allow 1e-3)
    generic = None
    for out in d.ddim_sample_loop_progressive(cmdm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), eta=eta, step_noise=nz):
        generic = out["sample"]
    report(f"CMDM generic DDIM loop {tag}", generic, want, 6e-5)
    report(f"CMDM native vs generic DDIM {tag}", native, generic, 0.0)          # measured 0: the same kernels compute the same bits
    sliced = d.ddim_sample_loop(cmdm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), eta=eta, step_noise=nz, progress=True)
    assert torch.equal(native, sliced)
    snaps = {1: None, d.num_timesteps - 1: None}
    snapped = d.ddim_sample_loop(cmdm, SHAPE, noise=xT, clip_denoised=clip, model_kwargs=_kw(g), eta=eta, step_noise=nz, snapshots=snaps)
    assert torch.equal(native, snapped) and all(v is not None for v in snaps.values())
    if resp == "ddim5":         # L = 15: 3945 values per sample, the update's last quad and its K-padded row copy end on a partial quad
        odd = (2, 15, 263)
        kw = dict(c_text_feat=g["text_feat"].to(dev()), c_cont_emb=g["cont_emb"].to(dev()), x_mask=synth.frame_mask(2, 15, min_len=8).to(dev()))
        onz = torch.stack([synth.gaussian(f"ddim_loop_L15_{j}", odd) for j in range(d.num_timesteps)]).to(dev())
        oxT = synth.gaussian("ddim_loop_L15_xT", odd).to(dev())
        native = d.ddim_sample_loop(cmdm, odd, noise=oxT, clip_denoised=clip, model_kwargs=kw, eta=eta, step_noise=onz)
        for out in d.ddim_sample_loop_progressive(cmdm, odd, noise=oxT, clip_denoised=clip, model_kwargs=kw, eta=eta, step_noise=onz):
            generic = out["sample"]
        assert torch.equal(native, generic)


def test_cdm_ddim_loop_in_every_sampling_form(cdm):
    """The DDIM update in the row-less, folded-rows and layer-by-layer forms against the reference and the step-by-step composition."""
    g = golden("cdm_forward_N256")
    want = golden("cdm_ddim_loop_ddim5")
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="ddim5"))
    nz = torch.stack([synth.gaussian(f"cdm_ddim_loop_{j}", (2, 256, 6)) for j in range(d.num_timesteps)]).to(dev())
    xT = synth.gaussian("cdm_ddim_loop_xT", (2, 256, 6)).to(dev())
    kw = dict(c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=g["xyz"].to(dev()))
    eta = float(want["eta"])
    outs = {}
    try:
        for form, attrs in (("row-less", {}), ("folded rows", dict(no_gen=True)), ("layer by layer", dict(no_fold=True))):
            for k, v in attrs.items():
                setattr(cdm, k, v)
            outs[form] = d.ddim_sample_loop(cdm, (2, 256, 6), noise=xT, clip_denoised=False, model_kwargs=kw, eta=eta, step_noise=nz).clone()
            cdm.no_gen = cdm.no_fold = False
    finally:
        cdm.no_gen = cdm.no_fold = False
    step = None
    for out in d.ddim_sample_loop_progressive(cdm, (2, 256, 6), noise=xT, clip_denoised=False, model_kwargs=kw, eta=eta, step_noise=list(nz)):
        step = out["sample"]
    report("CDM DDIM step-by-step vs reference", step, want["sample"], 1.4e-4)        # measured 7.0e-6
    # bounds per form, each <= 20x its measured error: vs the reference 7.0e-6 / 8.2e-6 / 1.1e-5; vs the step-by-step composition and
    # vs the row-less form 0 / 3.6e-6 / 7.2e-6 (the row-less loop runs the step-by-step path's kernels: bit-identical)
    ref_tol = {"row-less": 1.4e-4, "folded rows": 1.6e-4, "layer by layer": 2.2e-4}
    form_tol = {"row-less": 0.0, "folded rows": 7e-5, "layer by layer": 1.4e-4}
    for form, o in outs.items():
        report(f"CDM DDIM {form} vs reference", o, want["sample"], ref_tol[form])
        report(f"CDM DDIM {form} vs step-by-step", o, step, form_tol[form])
        report(f"CDM DDIM {form} vs row-less", o, outs["row-less"], form_tol[form])


def test_sub_batch_streams_are_bit_identical(cmdm, cdm):
    d, nz, xT = _loop_inputs("ddim5")
    g = golden("cmdm_forward_N1024_L16")
    run = lambda: d.ddim_sample_loop(cmdm, SHAPE, noise=xT, clip_denoised=False, model_kwargs=_kw(g), eta=1.0, seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto = 1, True
        one = run()
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
        two = run()
        cmdm.pair_launch = True
        paired = run()
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved
    assert torch.equal(one, two) and torch.equal(one, paired)
    gc = golden("cdm_forward_N256")
    dc = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="ddim5"))
    kw = dict(c_text_feat=gc["text_feat"].to(dev()), c_pc_xyz=gc["xyz"].to(dev()))
    xc = synth.gaussian("cdm_ddim_loop_xT", (2, 256, 6)).to(dev())
    runc = lambda: dc.ddim_sample_loop(cdm, (2, 256, 6), noise=xc, clip_denoised=False, model_kwargs=kw, eta=1.0, seed=4)
    saved = cdm.loop_sub_batches
    try:
        cdm.loop_sub_batches = 1
        c1 = runc()
        cdm.loop_sub_batches = 2
        c2 = runc()
    finally:
        cdm.loop_sub_batches = saved
    assert torch.equal(c1, c2)


def test_sharding_invariance_with_philox_noise(cmdm):
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    B, L = 4, 16
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_cont_emb=synth.gaussian("ddim_shard_cont", (B, 16, 256)).to(dev()),
              x_mask=synth.frame_mask(B, L, min_len=8).to(dev()))
    half = lambda i: {k: v[2 * i:2 * i + 2] for k, v in kw.items()}
    full = d.ddim_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, eta=1.0, seed=21)
    parts = [d.ddim_sample_loop(cmdm, (2, L, 263), clip_denoised=False, model_kwargs=half(i), eta=1.0, seed=21, sample_index0=2 * i)
             for i in range(2)]
    report("CMDM DDIM eta=1 sharded vs whole", torch.cat(parts, 0), full, 0.0)


def test_second_ddim_loop_launches_no_eager_arithmetic(cmdm):
    d, _, _ = _loop_inputs("ddim5")
    g = golden("cmdm_forward_N1024_L16")
    kw = _kw(g)
    d.ddim_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=kw, eta=0.5, seed=2)     # first call builds the rows and scratch
    torch.cuda.synchronize()
    _check(_device_kernel_names(lambda: d.ddim_sample_loop(cmdm, SHAPE, clip_denoised=False, model_kwargs=kw, eta=0.5, seed=3)), "CMDM DDIM")


def test_two_stage_ddim_equals_the_stages_by_hand(cmdm, cdm):
    from afm import dist as adist
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="ddim5"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    B, N, L = 2, 1024, 16
    text, xyz = synth.text_feature(B).to(dev()), synth.scene_cloud(B, N, seed=14).to(dev())
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9, sampler="ddim", eta=0.5)
    contact = d_adm.ddim_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), eta=0.5, seed=9)
    cond = adist.adm_to_amdm_condition(contact, sigma=0.8, mean=0.0, std=1.0)
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=cond, x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    motion = d_amdm.ddim_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, eta=0.5, seed=10)
    assert torch.equal(got["contact"], contact) and torch.equal(got["cond"], cond) and torch.equal(got["motion"], motion)


def test_cmdm_ddim_loop_with_a_narrow_feed_forward():
    """dim_feedforward = 64: the loop's pred_xstart [B][L][motion_dim] (4208 floats per sample) is larger than the encoder's hidden rows
    (T * ff = 34 * 64 = 2176 per sample) - it has a workspace region of its own, so the Philox noise of the next steps stays intact and
    the native loop equals the step-by-step composition at eta = 1."""
    cfg = cmdm_cfg(steps=1000, respacing="ddim5")
    cfg.model.dim_feedforward = 64
    m = create_model(cfg, device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    assert m.self_attn_layer.layers[0].linear1.out_features == 64
    d = create_gaussian_diffusion(cfg)
    g = golden("cmdm_forward_N1024_L16")
    native = d.ddim_sample_loop(m, SHAPE, clip_denoised=False, model_kwargs=_kw(g), eta=1.0, seed=31)
    generic = None
    for out in d.ddim_sample_loop_progressive(m, SHAPE, clip_denoised=False, model_kwargs=_kw(g), eta=1.0, seed=31):
        generic = out["sample"]
    report("CMDM ff=64 native vs generic DDIM eta=1", native, generic, 0.0)


def test_cdm_ddim_row_less_humanise_variant():
    """The NKS = 11 instantiation of dec_point_kernel's DDIM form (41 input channels: 32 scene features per point): native row-less loop
    against the step-by-step composition, eta = 1 with Philox noise."""
    m = create_model(cdm_cfg(point_feats=True), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    d = create_gaussian_diffusion(cdm_cfg(point_feats=True, steps=500, respacing="ddim5"))
    gc, g2 = golden("cdm_forward_N256"), golden("cdm_forward_feat32")
    kw = dict(c_text_feat=gc["text_feat"].to(dev()), c_pc_xyz=gc["xyz"].to(dev()), c_pc_feat=g2["pc_feat"].to(dev()))
    native = d.ddim_sample_loop(m, (2, 256, 6), clip_denoised=False, model_kwargs=kw, eta=1.0, seed=12)
    step = None
    for out in d.ddim_sample_loop_progressive(m, (2, 256, 6), clip_denoised=False, model_kwargs=kw, eta=1.0, seed=12):
        step = out["sample"]
    report("CDM HUMANISE (NKS = 11) row-less DDIM vs step-by-step", native, step, 0.0)        # measured 0
