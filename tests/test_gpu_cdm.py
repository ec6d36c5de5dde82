"""`-m gpu`: CDM / ContactPerceiver denoiser on the HIP path vs the reference goldens and the CPU oracle.
The encoder/decoder cross-attentions are evaluated in folded form (no K/V over the N points), i.e. a
re-association of the same f32 arithmetic: report() keeps the absolute bars (2e-4 on O(1) outputs, loops 1e-3); the bound that bites is
report_f32_class (tests/gpu_util.py): the HIP error against the float64 twin of the oracle is at most 4 x the float32 reference's own
error against that twin, plus one float32 ulp of the largest output, as maximum and as rms."""
import pytest
import torch

from afm import synth
from afm.base import create_gaussian_diffusion, create_model
from afm.config import to_config
from conftest import golden
from gpu_util import dev, grad_forms, load_named_weights, report, report_f32_class, to_f64, write_parity_table

pytestmark = pytest.mark.gpu


def cdm_cfg(num_points=256, point_feats=False, steps=500, respacing="", point_feat_dim=32):
    sm = dict(name="PointTransformerSeg", use_scene_model=point_feats, use_color=False, use_openscene=point_feats,
              num_points=num_points, point_feat_dim=point_feat_dim, pretrained_weight="", freeze=True)
    return to_config(dict(
        model=dict(name="CDM", input_feats=6, data_repr="contact_cont_joints", time_emb_dim=128,
                   text_model=dict(version="ViT-B/32", max_length=20), scene_model=sm, arch="Perceiver",
                   arch_perceiver=dict(last_dim=256, point_pos_emb=True, encoder_q_input_channels=512, encoder_kv_input_channels=256,
                                       encoder_num_heads=8, encoder_widening_factor=1, encoder_dropout=0.1, encoder_residual_dropout=0.0,
                                       encoder_self_attn_num_layers=2, decoder_q_input_channels=256, decoder_kv_input_channels=512,
                                       decoder_num_heads=8, decoder_widening_factor=1, decoder_dropout=0.1, decoder_residual_dropout=0.0)),
        diffusion=dict(predict_xstart=True, steps=steps, noise_schedule="cosine", timestep_respacing=respacing,
                       rescale_timesteps=False, loss_type="MSE", learn_sigma=False, sigma_small=True)))


@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def _sd64(**kw):
    from oracle import shapes as sh
    return to_f64(sh.weights(sh.cdm(**kw)))


def test_forward_vs_reference_golden(cdm):
    from oracle import denoiser_ref as dr
    g = golden("cdm_forward_N256")
    g64 = to_f64(g)
    want64 = dr.cdm_forward(_sd64(), g64["x"], g["t"], g64["text_feat"], g64["xyz"])
    for form, out in grad_forms(lambda: cdm(g["x"].to(dev()), g["t"].to(dev()), c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=g["xyz"].to(dev()))):
        report("CDM forward N=256 vs reference" + form, out, g["out"], 2e-4)
        report_f32_class("CDM forward N=256 vs reference" + form, out, g["out"], want64, 2e-4)


def test_loop_vs_reference_golden(cdm):
    g = golden("cdm_forward_N256")
    diff = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="4"))
    nz = torch.stack([synth.gaussian(f"cdm_loop_{j}", (2, 256, 6)) for j in range(diff.num_timesteps)]).to(dev())
    xT = synth.gaussian("cdm_loop_xT", (2, 256, 6)).to(dev())
    kw = dict(c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=g["xyz"].to(dev()))
    out = diff.p_sample_loop(cdm, (2, 256, 6), noise=xT, clip_denoised=False, model_kwargs=kw, step_noise=nz)
    report("CDM 4-step loop vs reference", out, golden("cdm_loop_r4")["sample"], 1e-3)
    from oracle import denoiser_ref as dr, diffusion_ref as df
    sd64, g64 = _sd64(), to_f64(g)
    want64 = df.p_sample_loop(df.Schedule(500, "cosine", "4"), lambda x, t, **k: dr.cdm_forward(sd64, x, t, g64["text_feat"], g64["xyz"]),
                              xT.cpu().double(), list(nz.cpu().double()))
    report_f32_class("CDM 4-step loop vs reference", out, golden("cdm_loop_r4")["sample"], want64, 1e-3)


def test_clip_denoised_in_every_sampling_form(cdm):
    """clip_denoised=True (the reference's default argument): the clamp of pred_xstart rides inside the fused DDPM update of the row-less,
    the folded-rows and the layer-by-layer form; each native loop against the step-by-step composition (model -> afm_clamp -> DDPM kernel)
    on the same recorded noise, and the three forms against each other."""
    g = golden("cdm_forward_N256")
    diff = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="4"))
    nz = torch.stack([synth.gaussian(f"cdm_loop_{j}", (2, 256, 6)) for j in range(diff.num_timesteps)]).to(dev())
    xT = 2.0 * synth.gaussian("cdm_loop_xT", (2, 256, 6)).to(dev())
    kw = dict(c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=g["xyz"].to(dev()))
    outs = {}
    try:
        for form, attrs in (("row-less", {}), ("folded rows", dict(no_gen=True)), ("layer by layer", dict(no_fold=True))):
            for k, v in attrs.items():
                setattr(cdm, k, v)
            outs[form] = diff.p_sample_loop(cdm, (2, 256, 6), noise=xT, model_kwargs=kw, step_noise=nz).clone()        # default: clip on
            cdm.no_gen = cdm.no_fold = False
    finally:
        cdm.no_gen = cdm.no_fold = False
    step = None
    for out in diff.p_sample_loop_progressive(cdm, (2, 256, 6), noise=xT, clip_denoised=True, model_kwargs=kw, step_noise=list(nz)):
        step = out
    assert step["pred_xstart"].abs().max().item() <= 1.0
    for form, o in outs.items():
        report(f"CDM clip_denoised, {form}: native loop vs step-by-step", o, step["sample"], 5e-5)
    unclipped = diff.p_sample_loop(cdm, (2, 256, 6), noise=xT, clip_denoised=False, model_kwargs=kw, step_noise=nz)
    assert (unclipped - outs["row-less"]).abs().max().item() > 1e-2


def test_forward_with_point_features_vs_reference_golden():
    g, g2 = golden("cdm_forward_N256"), golden("cdm_forward_feat32")
    m = create_model(cdm_cfg(point_feats=True), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    from oracle import denoiser_ref as dr
    g64 = to_f64(g)
    want64 = dr.cdm_forward(_sd64(point_feat_dim=32), g64["x"], g["t"], g64["text_feat"], g64["xyz"], pc_emb=g2["pc_feat"].double())
    for form, out in grad_forms(lambda: m(g["x"].to(dev()), g["t"].to(dev()), c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=g["xyz"].to(dev()),
                                          c_pc_feat=g2["pc_feat"].to(dev()))):
        report("CDM forward with 32-d point features vs reference" + form, out, g2["out"], 2e-4)
        report_f32_class("CDM forward with 32-d point features vs reference" + form, out, g2["out"], want64, 2e-4)


def test_full_size_vs_oracle():
    """BASELINE configs[2] shape (B = 2 here): N = 8192 points."""
    from oracle import denoiser_ref as dr, shapes as sh
    m = create_model(cdm_cfg(num_points=8192), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    B, N = 2, 8192
    x = synth.gaussian("cdm_full_x", (B, N, 6)); xyz = synth.scene_cloud(B, N, seed=51); text = synth.text_feature(B)
    t = torch.tensor([499, 3])
    want = dr.cdm_forward(sh.weights(sh.cdm()), x, t, text, xyz)
    want64 = dr.cdm_forward(_sd64(), x.double(), t, text.double(), xyz.double())
    for form, got in grad_forms(lambda: m(x.to(dev()), t.to(dev()), c_text_feat=text.to(dev()), c_pc_xyz=xyz.to(dev()))):
        report("CDM forward N=8192 vs oracle" + form, got, want, 2e-4)
        report_f32_class("CDM forward N=8192 vs oracle" + form, got, want, want64, 2e-4)


def test_two_stage_adm_to_amdm_pipeline_vs_oracle():
    """BASELINE configs[4] in miniature: ADM loop -> in-HBM glue -> AMDM loop (contact encoder included),
    explicit noise, vs the CPU oracle doing the same two loops."""
    from afm.pipeline import two_stage_sample
    from oracle import denoiser_ref as dr, diffusion_ref as df, shapes as sh
    from test_gpu_cmdm import cmdm_cfg
    B, N, L = 2, 1024, 12
    adm = create_model(cdm_cfg(num_points=N), device=dev()); load_named_weights(adm); adm = adm.to(dev()).eval()
    amdm = create_model(cmdm_cfg(num_points=N), device=dev()); load_named_weights(amdm); amdm = amdm.to(dev()).eval()
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="3"))
    text, xyz = synth.text_feature(B), synth.scene_cloud(B, N, seed=61)
    a_xT, a_nz = synth.gaussian("p_axT", (B, N, 6)) * 0.3 + 0.5, [synth.gaussian(f"p_anz{j}", (B, N, 6)) * 0.1 for j in range(3)]
    m_xT, m_nz = synth.gaussian("p_mxT", (B, L, 263)), [synth.gaussian(f"p_mnz{j}", (B, L, 263)) for j in range(3)]
    out = two_stage_sample(adm, d_adm, amdm, d_amdm, text_feat=text.to(dev()), xyz=xyz.to(dev()), frames=L, sigma=0.8,
                           adm_noise=dict(x_T=a_xT.to(dev()), steps=torch.stack(a_nz).to(dev())),
                           amdm_noise=dict(x_T=m_xT.to(dev()), steps=torch.stack(m_nz).to(dev())))
    sd_a, sd_m = sh.weights(sh.cdm()), sh.weights(sh.cmdm())
    c_ref = df.p_sample_loop(df.Schedule(500, "cosine", "3"), lambda x, t, **k: dr.cdm_forward(sd_a, x, t, text, xyz), a_xT, a_nz)
    cond_ref = torch.exp(-0.5 * (torch.sqrt(-2 * torch.log(c_ref.clamp(1e-20, 1.0)) * 0.8 ** 2)) ** 2 / 0.8 ** 2)
    mask = torch.zeros(B, L, dtype=torch.bool)
    m_ref = df.p_sample_loop(df.Schedule(1000, "cosine", "3"),
                             lambda x, t, **k: dr.cmdm_forward(sd_m, x, t, text, xyz, cond_ref, mask), m_xT, m_nz)
    report("two-stage: ADM contact", out["contact"], c_ref, 1e-4)
    report("two-stage: glue", out["cond"], cond_ref, 1e-4)
    report("two-stage: AMDM motion", out["motion"], m_ref, 1e-3)
    # the float64 twin of the same two loops and of the glue between them
    sd_a64, sd_m64, text64, xyz64 = to_f64(sd_a), to_f64(sd_m), text.double(), xyz.double()
    c64 = df.p_sample_loop(df.Schedule(500, "cosine", "3"), lambda x, t, **k: dr.cdm_forward(sd_a64, x, t, text64, xyz64), a_xT.double(), to_f64(a_nz))
    cond64 = torch.exp(-0.5 * (torch.sqrt(-2 * torch.log(c64.clamp(1e-20, 1.0)) * 0.8 ** 2)) ** 2 / 0.8 ** 2)
    m64 = df.p_sample_loop(df.Schedule(1000, "cosine", "3"),
                           lambda x, t, **k: dr.cmdm_forward(sd_m64, x, t, text64, xyz64, cond64, mask), m_xT.double(), to_f64(m_nz))
    report_f32_class("two-stage: ADM contact", out["contact"], c_ref, c64, 1e-4)
    report_f32_class("two-stage: glue", out["cond"], cond_ref, cond64, 1e-4)
    report_f32_class("two-stage: AMDM motion", out["motion"], m_ref, m64, 1e-3)


@pytest.mark.parametrize("arch,tag", [("PointTrans", "cdm_pointtrans_N1024"), ("PointTransV2", "cdm_pointtransv2_N1024")])
def test_pointtrans_archs_forward_vs_reference_golden(arch, tag):
    """`model.arch=PointTrans` / `PointTransV2` (cdm.py:190-410): a Point Transformer U-Net over the contact map per step."""
    from afm.config import load_config
    from afm.base import create_model
    cfg = load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.scene_model.use_scene_model=False", f"model.arch={arch}",
                                                           "task.dataset.num_points=1024", "model.text_model.max_length=20"])
    model = create_model(cfg, device=dev())
    load_named_weights(model)
    model = model.to(dev()).eval()
    gp, g = golden(tag), golden("cdm_forward_N256")
    x, xyz = synth.gaussian("cdm_pt_x", (2, 1024, 6)).to(dev()), synth.scene_cloud(2, 1024, seed=16).to(dev())
    with torch.no_grad():
        out = model(x, gp["t"].to(dev()), c_text_feat=g["text_feat"].to(dev()), c_pc_xyz=xyz)
    report(f"CDM {arch} forward vs reference", out[:, gp["rows"].to(dev())], gp["out_rows"], 5e-4)
    from oracle import denoiser_ref as dr, shapes as sh
    want64 = dr.cdm_pointtrans_forward(to_f64(sh.weights(sh.cdm_pointtrans(v2=arch == "PointTransV2"))), x.cpu().double(), gp["t"],
                                       g["text_feat"].double(), xyz.cpu().double(), v2=arch == "PointTransV2")
    report_f32_class(f"CDM {arch} forward vs reference", out[:, gp["rows"].to(dev())], gp["out_rows"], want64[:, gp["rows"]], 5e-4)
    s = out.double().abs().sum().item()
    assert abs(s - gp["out_abs_sum"].item()) <= 1e-4 * gp["out_abs_sum"].item()


def test_native_loop_matches_stepwise_and_is_sub_batch_invariant(cdm):
    """afm_cdm_sample_loop (Philox noise, DDPM update fused into the last GEMM, sub-batch stream pairs) vs the step-by-step
    path, and bit-identical results for 1 / 2 / 3 sub-batches (samples are independent)."""
    d8 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="8"))
    B, N = 5, 512
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_pc_xyz=synth.scene_cloud(B, N, seed=4).to(dev()))
    outs = []
    for nsub in (1, 2, 3):
        cdm.loop_sub_batches = nsub
        outs.append(d8.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=11, sample_index0=7))
    cdm.loop_sub_batches = 1
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    step = None
    for o in d8.p_sample_loop_progressive(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=11, sample_index0=7):
        step = o["sample"]
    report("CDM native loop vs step-by-step (8 steps)", outs[0], step, 1e-4)
    # test.py's call pattern (progress=True, non-tensor info_* entries): sliced native loop, bit-identical to the unsliced one
    d60 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="60"))
    kwi = dict(kw, info_index=list(range(B)), c_text=["walk"] * B)
    whole = d60.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, noise=None, model_kwargs=kwi, seed=3, sample_index0=7)
    sliced = d60.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, noise=None, model_kwargs=kwi, seed=3, sample_index0=7, progress=True)
    assert torch.equal(whole, sliced)
    # sharding invariance: samples 2..4 computed alone with their global indices give the same rows
    kw2 = {k: v[2:] for k, v in kw.items()}
    part = d8.p_sample_loop(cdm, (3, N, 6), clip_denoised=False, model_kwargs=kw2, seed=11, sample_index0=9)
    assert torch.equal(part, outs[0][2:])


def test_config4_full_size_properties():
    """VERDICT r1 #4c - BASELINE configs[4] at its real size: one text + one scene, k_sample = 32 flattened into the batch, N = 8192 points,
    L = 196 frames, ADM (Perceiver) -> in-HBM glue -> AMDM (trans_enc incl. the SceneMapEncoder over the generated contact maps).  The CPU
    oracle cannot run this size inside a test, so size-independent properties are checked on respaced chains (50 ADM + 100 AMDM steps):
    finite outputs, the glue's range, run-to-run determinism, and invariance to how the 32 samples are sharded (1 x 32 vs 2 x 16 vs
    4 x 8 - what ranks of an 8-GPU node do, with Philox noise keyed by the global sample index), bit for bit."""
    from afm.pipeline import two_stage_sample
    from test_gpu_cmdm import cmdm_cfg
    K, N, L = 32, 8192, 196
    adm = create_model(cdm_cfg(num_points=N), device=dev()); load_named_weights(adm); adm = adm.to(dev()).eval()
    amdm = create_model(cmdm_cfg(num_points=N), device=dev()); load_named_weights(amdm); amdm = amdm.to(dev()).eval()
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="50"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="100"))
    text = synth.text_feature(1).repeat(K, 1).contiguous().to(dev())
    xyz = synth.scene_cloud(1, N, seed=71).repeat(K, 1, 1).contiguous().to(dev())

    def run(lo, hi):
        return two_stage_sample(adm, d_adm, amdm, d_amdm, text_feat=text[lo:hi].contiguous(), xyz=xyz[lo:hi].contiguous(), frames=L,
                                sigma=0.8, seed=5, sample_index0=lo)

    whole = run(0, K)
    for name in ("contact", "cond", "motion"):
        assert torch.isfinite(whole[name]).all(), name
    assert whole["contact"].shape == (K, N, 6) and whole["motion"].shape == (K, L, 263)
    cond = whole["cond"]
    assert cond.min().item() >= 0.9999e-20 and cond.max().item() <= 1.0      # exp(-d^2 / 2 sigma^2) of a contact map clipped to [1e-20, 1] (the log -> exp round trip is not exact)
    # the k samples share text and scene but not noise: they must differ from each other
    assert (whole["motion"][0] - whole["motion"][1]).abs().max().item() > 1e-3
    again = run(0, K)
    for name in ("contact", "cond", "motion"):
        assert torch.equal(again[name], whole[name]), f"{name}: two identical runs differ"
    for shards in (2, 4):
        per = K // shards
        parts = [run(r * per, (r + 1) * per) for r in range(shards)]
        for name in ("contact", "cond", "motion"):
            got = torch.cat([p[name] for p in parts])
            assert torch.equal(got, whole[name]), f"{name}: {shards} shards of {per} samples differ from the single batch of {K}"


def test_openscene_text_similarity_feature():
    """cdm.py:500-503: with scene_model.use_openscene and point_feat_dim = 1, wide per-point features are reduced to ONE channel - their inner
    product with the sample's text feature (einsum 'b n d, b m d -> b n m').  Here: one afm_linear per sample, cached while the same tensors
    are passed; the denoiser's input block and a forward agree with the einsum in float64 / with the same model fed the reduced channel."""
    B, N = 3, 512
    m = create_model(cdm_cfg(num_points=N, point_feats=True, point_feat_dim=1), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    wide = synth.gaussian("os_feat", (B, N, 512)).to(dev())
    text = synth.text_feature(B).to(dev())
    want = torch.einsum("bnd,bd->bn", wide.double(), text.double()).unsqueeze(-1)
    x, t = synth.gaussian("os_x", (B, N, 6)).to(dev()), torch.tensor([5, 250, 499], device=dev())
    kw = dict(c_text_feat=text, c_pc_xyz=synth.scene_cloud(B, N, seed=8).to(dev()), c_pc_feat=wide)
    feat = m._features(x, kw)
    assert feat.shape == (B, N, 6 + 1 + 3)
    report("openscene text similarity channel", feat[..., 6:7], want, 2e-4)
    assert m._features(x, kw)[..., 6:7].data_ptr() != 0 and m._sim_cache is not None          # second call: served from the cache
    out = m(x, t, **kw)
    out_ref = m(x, t, **dict(kw, c_pc_feat=feat[..., 6:7].contiguous()))
    assert torch.isfinite(out).all()
    report("forward with the wide features vs the reduced channel", out, out_ref, 1e-5)


def test_pipelined_sub_batches_are_bit_identical():
    """Round 6: AFM_CDM_PIPELINE - the point kernels of all sub-batches in round-robin order on ONE stream, every sub-batch's latent chain on its
    own side stream between two events (a fixed-phase software pipeline instead of free-running sub-batch streams).  Samples are
    independent and a point's arithmetic does not depend on the sub-batching or on dec_chunks: the result must equal the single-stream
    loop's bit for bit, for 2 / 3 / 4 sub-batches, uneven splits, more steps than one noise block (16), and repeated runs."""
    N = 2048
    adm = create_model(cdm_cfg(num_points=N), device=dev()); load_named_weights(adm); adm = adm.to(dev()).eval()
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="40"))
    for K in (32, 7):
        kw = dict(c_text_feat=synth.text_feature(K).to(dev()), c_pc_xyz=synth.scene_cloud(K, N, seed=72).to(dev()))

        def run(nsub, pipeline, chunks=0):
            adm.loop_sub_batches, adm.pipeline, adm.dec_chunks = nsub, pipeline, chunks
            return d.p_sample_loop(adm, (K, N, 6), clip_denoised=False, model_kwargs=kw, seed=6, sample_index0=3).clone()
        try:
            ref = run(1, False)
            assert torch.isfinite(ref).all()
            for nsub, chunks in ((2, 0), (3, 0), (3, 23), (4, 32)):
                for r in range(3):
                    out = run(nsub, True, chunks)
                    bad = (out != ref).flatten(1).any(1).nonzero().flatten().tolist()
                    assert not bad, f"K={K} nsub={nsub} chunks={chunks} run {r}: samples {bad} differ (max {(out - ref).abs().max().item():.2e})"
        finally:
            adm.loop_sub_batches, adm.pipeline, adm.dec_chunks = 1, False, 0


def test_two_sub_batch_loop_repeats():
    """Round 2 regression (profiles/r02_decfold_nondeterminism.md): at configs[4]'s ADM size the native loop runs as two sub-batches on
    their own streams.  A build of lat_decfold_kernel that was correct on one stream lost single products in single waves in ~1/4 of
    50-step loops once the second stream was active - invisible to a single run-twice check.  Twelve loops with the two streams against
    the single-stream result, bit for bit (the failing build passed this with probability ~0.03)."""
    K, N = 32, 8192
    adm = create_model(cdm_cfg(num_points=N), device=dev()); load_named_weights(adm); adm = adm.to(dev()).eval()
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="50"))
    kw = dict(c_text_feat=synth.text_feature(1).repeat(K, 1).contiguous().to(dev()),
              c_pc_xyz=synth.scene_cloud(1, N, seed=71).repeat(K, 1, 1).contiguous().to(dev()))

    def run(nsub):
        adm.loop_sub_batches = nsub
        return d.p_sample_loop(adm, (K, N, 6), clip_denoised=False, model_kwargs=kw, seed=5).clone()

    ref = run(1)
    assert torch.isfinite(ref).all()
    for r in range(12):
        junk = torch.randn(64 << 20, device=dev()) if r % 2 else None      # vary allocator state and stream timing between the loops
        out = run(2)
        del junk
        bad = (out != ref).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"loop {r}: samples {bad} differ from the single-stream result (max {(out - ref).abs().max().item():.2e})"


def test_adm_to_amdm_glue_kernel_vs_reference_golden():
    """afm_contact_glue (the in-HBM ADM -> AMDM hand-off) against the golden generated from the real reference's two file-format halves."""
    from afm import dist as adist
    g = golden("adm_to_amdm_glue")
    cond = adist.adm_to_amdm_condition(g["sample"].to(dev()), sigma=float(g["sigma"]), mean=float(g["mean"]), std=float(g["std"]))
    report("ADM -> AMDM glue kernel vs reference golden", cond, g["cond"].float(), 1e-6)
    big = synth.gaussian("glue_big", (3, 1000, 6)).to(dev()) * 2.0
    from oracle import glue_ref
    report("glue kernel vs oracle (clipped tails)", adist.adm_to_amdm_condition(big, sigma=0.8, mean=0.1, std=0.7),
           glue_ref.adm_to_amdm_condition(big.cpu(), sigma=0.8, mean=0.1, std=0.7), 1e-6)


def test_native_loop_snapshots(cdm):
    """`p_sample_loop(..., snapshots={k: None})`: the ADM's native loop cuts the chain at the requested step counts and clones x
    there - the states p_sample_loop_progressive would have yielded, bit for bit equal to running the chain only that far."""
    d8 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="8"))
    B, N = 3, 256
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_pc_xyz=synth.scene_cloud(B, N, seed=8).to(dev()))
    snaps = {3: None, 6: None}
    full = d8.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=17, snapshots=snaps)
    assert torch.equal(full, d8.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=17))
    states = [o["sample"] for o in d8.p_sample_loop_progressive(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=17)]
    for k in (3, 6):
        report(f"CDM snapshot after {k} steps vs step-by-step", snaps[k], states[k - 1].cpu(), 1e-4)


def test_two_stream_loop_soak():
    """Round 3: the soak harness of profiles/r02_decfold_nondeterminism.md inside the suite - 50 two-stream 50-step loops of
    the ADM at configs[4]'s size against the single-stream result, bit for bit (the failing round-2 build differed in ~1/4 of such loops)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    from loop_determinism_probe import probe_cdm
    bad = probe_cdm(50, dev())
    assert not bad, f"{len(bad)} of 50 two-stream loops differ from the single-stream result: {bad[:4]}"


@pytest.fixture(scope="module")
def cdm_feat():
    m = create_model(cdm_cfg(point_feats=True), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


@pytest.mark.parametrize("B,N,feats", [(3, 1000, False), (1, 37, False), (9, 272, False), (3, 1000, True), (2, 53, True), (5, 4096, True)])
def test_row_less_form_on_ragged_shapes(cdm, cdm_feat, B, N, feats):
    """The row-less sampling form (enc_point / lat_head / lat_dectables / dec_point) against the layer-by-layer form where its tiling is ragged:
    N not a multiple of the 16-point tiles or of the per-wave ranges, a last token block of fewer than 16 latent tokens, one sample; both
    instantiations of the kernels (12 inputs: the H3D variant; 44 inputs: 32 scene features per point, the HUMANISE variant)."""
    cdm = cdm_feat if feats else cdm
    xyz, text = synth.scene_cloud(B, N, seed=B + N), synth.text_feature(B)
    kw = dict(c_text_feat=text.to(dev()), c_pc_xyz=xyz.to(dev()))
    if feats:
        kw["c_pc_feat"] = synth.gaussian(f"ragged_feat_{B}_{N}", (B, N, 32)).to(dev())
    x = synth.gaussian(f"ragged_x_{B}_{N}", (B, N, 6))
    t = torch.arange(B) * 53 % 500
    d4 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="4"))
    out = {}
    try:
        for tag, no_fold in (("default", False), ("layered", True)):
            cdm.no_fold = no_fold
            with torch.no_grad():
                out[tag] = (cdm(x.to(dev()), t.to(dev()), **kw), d4.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=7))
    finally:
        cdm.no_fold = False
    assert torch.isfinite(out["default"][0]).all() and torch.isfinite(out["default"][1]).all()
    report(f"CDM forward B={B} N={N}: row-less vs layered", out["default"][0], out["layered"][0].cpu(), 2e-5)
    from oracle import denoiser_ref as dr, shapes as sh
    sd = sh.weights(sh.cdm(point_feat_dim=32 if feats else 0))
    emb = kw["c_pc_feat"].cpu() if feats else None
    want = dr.cdm_forward(sd, x, t, text, xyz, pc_emb=emb)
    want64 = dr.cdm_forward(to_f64(sd), x.double(), t, text.double(), xyz.double(), pc_emb=to_f64(emb))
    for tag in ("default", "layered"):
        report(f"CDM forward B={B} N={N} feats={feats} ({tag}) vs oracle", out[tag][0], want, 2e-4)
        report_f32_class(f"CDM forward B={B} N={N} feats={feats} ({tag}) vs oracle", out[tag][0], want, want64, 2e-4)
    report(f"CDM 4-step loop B={B} N={N}: row-less vs layered", out["default"][1], out["layered"][1].cpu(), 1e-4)


@pytest.mark.parametrize("pfd", [3, 8, 34])
def test_row_less_form_with_partly_filled_input_tiles(pfd):
    """Feature widths between the two instantiations of the row-less kernels: feat_dim + 1 = 13 (the first width that needs K = 44), 18, and 44
    (every input used) - the unused inputs are zero columns of the host's tables, the loads of a tile are clamped to the sample's last float."""
    m = create_model(cdm_cfg(point_feats=True, point_feat_dim=pfd), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    assert m.contact_model.feat_dim + 1 == 6 + pfd + 3 + 1
    B, N = 3, 333
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_pc_xyz=synth.scene_cloud(B, N, seed=pfd).to(dev()),
              c_pc_feat=synth.gaussian(f"partly_feat_{pfd}", (B, N, pfd)).to(dev()))
    x, t = synth.gaussian(f"partly_x_{pfd}", (B, N, 6)).to(dev()), (torch.arange(B) * 97 % 500).to(dev())
    d4 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="4"))
    out = {}
    for tag, no_fold in (("default", False), ("layered", True)):
        m.no_fold = no_fold
        with torch.no_grad():
            out[tag] = (m(x, t, **kw), d4.p_sample_loop(m, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=11))
    report(f"CDM forward, {pfd} point features: row-less vs layered", out["default"][0], out["layered"][0].cpu(), 2e-5)
    report(f"CDM 4-step loop, {pfd} point features: row-less vs layered", out["default"][1], out["layered"][1].cpu(), 1e-4)


def test_sampling_forms_agree_with_each_other_and_the_oracle(cdm):
    """The CDM samples in one of three forms, all re-associations of the same f32 arithmetic:
      default   no per-point rows (round 3): a point is its 12 inputs [x_t | xyz | 1] and the decoder's 16 attention weights between the
                nonlinearities - the encoder reduction accumulates 16 x 12 numbers per wave, the whole decoder of a point is one kernel with
                linear1 as a K = 28 product; neither adapter output, nor h1, z or the hidden row is materialised;
      no_gen    round 2's folded form (step-invariant adapter parts materialised once per loop, per-point rows, linear1 as a GEMM);
      layered   the layer-by-layer form (what a training-mode forward runs).
    Against the CPU oracle a forward agrees to 2e-4 (measured ~5e-6); among each other to 2e-5, an 8-step loop to 1e-4."""
    from oracle import denoiser_ref as dr, shapes as sh
    B, N = 5, 512
    xyz, text = synth.scene_cloud(B, N, seed=4), synth.text_feature(B)
    kw = dict(c_text_feat=text.to(dev()), c_pc_xyz=xyz.to(dev()))
    x = synth.gaussian("fold_x", (B, N, 6))
    t = torch.tensor([3, 77, 250, 499, 0])
    d8 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="8"))
    res = {}
    try:
        for tag, (no_fold, no_gen) in dict(default=(False, False), no_gen=(False, True), layered=(True, False)).items():
            cdm.no_fold, cdm.no_gen = no_fold, no_gen
            with torch.no_grad():
                f = cdm(x.to(dev()), t.to(dev()), **kw)
            res[tag] = (f, d8.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, model_kwargs=kw, seed=5))
    finally:
        cdm.no_fold = cdm.no_gen = False
    w = cdm._weights()
    assert w.fold_xu and w.fold_w2 and w.fold_q and w.gen_qe and w.dec_twx and w.dec_wow and w.enc_wove, "eval-mode pack carries the folded products and the row-less tables"
    want = dr.cdm_forward(sh.weights(sh.cdm()), x, t, text, xyz)
    want64 = dr.cdm_forward(_sd64(), x.double(), t, text.double(), xyz.double())
    for tag, (f, _) in res.items():
        report(f"CDM forward ({tag}) vs oracle", f, want, 2e-4)
        report_f32_class(f"CDM forward ({tag}) vs oracle", f, want, want64, 2e-4)
    for tag in ("no_gen", "layered"):
        report(f"CDM forward: default vs {tag}", res["default"][0], res[tag][0].cpu(), 2e-5)
        report(f"CDM 8-step loop: default vs {tag}", res["default"][1], res[tag][1].cpu(), 1e-4)
    assert not torch.equal(res["default"][0], res["no_gen"][0]) and not torch.equal(res["default"][0], res["layered"][0])      # other code really ran
    cdm.train()
    try:
        assert not cdm._weights().fold_xu, "training mode keeps the layer-by-layer form (weights change every step)"
    finally:
        cdm.eval()


def test_batched_latent_chain_with_more_than_one_token_block(cdm):
    """B = 40 samples are 80 latent tokens: two 64-token blocks per stage of the batched chain (the second one partly filled), and a
    sub-batched loop whose parts are 1 / 2 / 37 samples wide; checked against the CPU oracle and per sample."""
    B, N = 40, 128
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_pc_xyz=synth.scene_cloud(B, N, seed=9).to(dev()))
    x = synth.gaussian("tb_x", (B, N, 6)).to(dev())
    t = (torch.arange(B, device=dev()) * 12) % 500
    try:
        with torch.no_grad():
            got = cdm(x, t, **kw)
    finally:
        pass
    from oracle import denoiser_ref as dr, shapes as sh
    want = dr.cdm_forward(sh.weights(sh.cdm()), x.cpu(), t.cpu(), kw["c_text_feat"].cpu(), kw["c_pc_xyz"].cpu())
    report("CDM forward B=40 (two token blocks) vs oracle", got, want, 2e-4)
    with torch.no_grad():
        parts = torch.cat([cdm(x[a:b], t[a:b], **{k: v[a:b] for k, v in kw.items()}) for a, b in ((0, 1), (1, 3), (3, 40))])
    assert torch.equal(parts, got), "a sample's result must not depend on which batch it is computed in"


def test_eval_pack_carries_the_fold_tables_bit_for_bit():
    """Every table afm.fold.cdm_tables names is in the default eval pack, behind its field's pointer, as the float32 rounding of the host's
    float64 table (tests/test_cdm_fold_host.py pins those to their identities); a training-mode pack and a no_fold pack carry none."""
    import ctypes as C
    from afm import fold
    m = create_model(cdm_cfg(num_points=64), device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    tables = fold.cdm_tables(m.contact_model, m.contact_layer, m.contact_dim)
    slots = tables.pop("lat_fold")
    assert len(tables) == 20 and len(slots) == 19
    w = m._weights()
    by_ptr = {t.data_ptr(): t for t in m._pack[2] if isinstance(t, torch.Tensor)}

    def same(ptr, want, what):
        got = by_ptr[ptr]
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.cpu(), want.float()), what
    for name, t in tables.items():
        same(getattr(w, name), t, name)
    ptrs = C.cast(w.lat_fold, C.POINTER(C.c_void_p))
    for s, trip in enumerate(slots):
        for j in range(3):
            if trip is None:
                assert not ptrs[3 * s + j], f"lat_fold slot {s} of a layer the model does not have"
            else:
                same(ptrs[3 * s + j], trip[j], f"lat_fold[{3 * s + j}]")
    try:
        for training, no_fold in ((True, False), (False, True)):
            m.train(training)
            m.no_fold = no_fold
            w = m._weights()
            assert not any(getattr(w, name) for name in tables) and not w.lat_fold, f"training={training} no_fold={no_fold}: a table is set"
    finally:
        m.eval()
        m.no_fold = False


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table -> profiles/r07_parity_f32_class.json)."""
    write_parity_table()
