"""`-m gpu`: imputation of known contact values inside the CDM's native loops (CDM.afm_native_loop with impute=, afm_cdm_impute_loop_range).

Bit for bit: the default (row-less) form against the step-by-step loop with the same afm.diffusion.Impute - the select fused into
dec_point's update, the DDPM update uncontracted - and against itself over sub-batches, the pipelined and chain-side forms, slices and
shards.  The folded-rows and layer-by-layer forms against the row-less one, and every form against the reference goldens of
tools/make_goldens_cdm_impute.py: report() with a bound of at most 20x the error measured on the MI355X (beside each) and never above the
tolerance the non-imputing CDM test of that kind states, report_f32_class beside it against the float64 twin of
tests/test_cdm_impute_host.py.  Shapes: the golden's (2, 256, 6); (3, 251, 6) - a partial 16-point tile, 1506 values per sample so that
the mask bases of samples 1 and 2 are not 4-aligned, an uneven split over two sub-batches; (2, 1024, 6) - two 512-point chunks per
sample; and the 44-input HUMANISE variant (NKS = 11)."""
import pytest
import torch

from afm import synth
from afm.base import create_gaussian_diffusion, create_model
from afm.diffusion import Impute
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report, report_f32_class, write_parity_table
from test_cdm_impute_host import DDIM_LOOPS, DDPM_LOOPS, SHAPE, contact_known, contact_mask, loop_inputs, p_sample_inputs, twin64
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())
FORMS = (("row-less", {}), ("folded rows", dict(no_gen=True)), ("layer by layer", dict(no_fold=True)))


@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


@pytest.fixture(scope="module")
def cdm_feat():
    m = create_model(cdm_cfg(point_feats=True), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


class _Form:
    """a sampling form of the CDM for the length of a `with` block"""
    KEYS = ("no_gen", "no_fold", "loop_sub_batches", "pipeline", "chain_side")

    def __init__(self, model, **attrs):
        self.model, self.attrs = model, attrs

    def __enter__(self):
        self.saved = {k: getattr(self.model, k) for k in self.KEYS}
        for k, v in self.attrs.items():
            setattr(self.model, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.model, k, v)


def _golden_imp():
    return Impute(D(contact_known()), D(contact_mask()))


def _golden_kw():
    g = golden("cdm_forward_N256")
    return dict(c_text_feat=D(g["text_feat"]), c_pc_xyz=D(g["xyz"]))


def _case(cdm, cdm_feat, name):
    """(model, shape, model_kwargs, Impute) of a shape case: random known values (beyond +-1) under a random per-element mask"""
    B, N, feats = {"golden": (2, 256, False), "ragged": (3, 251, False), "two chunks": (2, 1024, False), "humanise": (2, 256, True)}[name]
    shape = (B, N, 6)
    kw = dict(c_text_feat=D(synth.text_feature(B)), c_pc_xyz=D(synth.scene_cloud(B, N, seed=14)))
    if feats:
        kw["c_pc_feat"] = D(synth.gaussian(f"cdm_imp_feat_{N}", (B, N, 32)))
    imp = Impute(D(synth.gaussian(f"cdm_imp_known_{B}_{N}", shape)), D(synth.gaussian(f"cdm_imp_bits_{B}_{N}", shape) > 0.3))
    return (cdm_feat if feats else cdm), shape, kw, imp


def _sampler(eta, respacing=5):
    """(diffusion, loop(model, shape, **kw), progressive(model, shape, **kw)): the DDPM loop (eta None) or the DDIM loop, `respacing` steps of T = 500"""
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing=str(respacing) if eta is None else f"ddim{respacing}"))
    if eta is None:
        return d, d.p_sample_loop, d.p_sample_loop_progressive
    return d, (lambda *a, **k: d.ddim_sample_loop(*a, eta=eta, **k)), (lambda *a, **k: d.ddim_sample_loop_progressive(*a, eta=eta, **k))


SAMPLERS = {"ddpm": None, "ddim_eta0": 0.0, "ddim_eta1": 1.0}


# ---------------------------------------------------------------------------------------------------------------- row-less form, exact
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("case", ["golden", "ragged", "two chunks", "humanise"])
def test_row_less_imputing_loop_equals_the_step_by_step_loop(cdm, cdm_feat, case, sampler, clip):
    model, shape, kw, imp = _case(cdm, cdm_feat, case)
    d, loop, progressive = _sampler(SAMPLERS[sampler])
    xT = D(synth.gaussian(f"cdm_imp_xT_{case}", shape))
    nz = D(torch.stack([synth.gaussian(f"cdm_imp_nz_{case}_{j}", shape) for j in range(d.num_timesteps)]))
    given = dict(noise=xT, clip_denoised=clip, denoised_fn=imp, model_kwargs=kw, step_noise=nz)
    seeded = dict(clip_denoised=clip, denoised_fn=imp, model_kwargs=kw, seed=4, sample_index0=3)          # Philox noise, x_T included
    sel = imp.mask.bool()
    want = imp.known.clamp(-1, 1) if clip else imp.known
    for args in (given, seeded):
        native = loop(model, shape, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, shape, **args)))
        assert torch.equal(native[sel], want[sel])                                   # what a user relies on: the known values, bit for bit
        assert torch.equal(native, loop(model, shape, progress=True, **args))         # sliced: one native call per step
        snaps = {1: None, d.num_timesteps - 1: None}
        assert torch.equal(native, loop(model, shape, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
    # a NaN wherever nothing is known is never read
    knan = Impute(torch.where(sel, imp.known, torch.full_like(imp.known, float("nan"))), imp.mask)
    assert torch.equal(native, loop(model, shape, **{**seeded, "denoised_fn": knan}))
    # nothing known: the DDIM loop is the existing native DDIM loop exactly; the DDPM loop is the STEP-BY-STEP loop without a denoised_fn
    # exactly (the existing native DDPM loop's update is contracted and may differ in the last bit)
    none = Impute(imp.known, torch.zeros(shape, dtype=torch.bool, device=dev()))
    empty, plain = loop(model, shape, **{**given, "denoised_fn": none}), {**given, "denoised_fn": None}
    assert torch.equal(empty, _last(progressive(model, shape, **plain)))
    if sampler != "ddpm":
        assert torch.equal(empty, loop(model, shape, **plain))
    assert not torch.equal(empty, loop(model, shape, **given))


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_sub_batches_pipeline_chain_side_and_shards_are_bit_identical(cdm, cdm_feat, sampler):
    """B = 3: two sub-batches split 2 + 1 (both pointers offset by sb.start * per, 1506 values: an odd mask base); the pipelined and the
    chain-side forms of the sub-batches; a batch against its shards through Impute.narrow and sample_index0."""
    model, shape, kw, imp = _case(cdm, cdm_feat, "ragged")
    _, loop, _ = _sampler(SAMPLERS[sampler], respacing=20)                            # more steps than one block of Philox noise (16)
    args = dict(clip_denoised=False, denoised_fn=imp, model_kwargs=kw, seed=21)
    one = loop(model, shape, **args)
    for attrs in (dict(loop_sub_batches=2), dict(loop_sub_batches=3), dict(loop_sub_batches=2, pipeline=True), dict(loop_sub_batches=2, chain_side=True)):
        with _Form(model, **attrs):
            assert torch.equal(one, loop(model, shape, **args)), attrs
    parts = [loop(model, (c, shape[1], 6), **{**args, "denoised_fn": imp.narrow(s, c), "model_kwargs": {k: v[s:s + c] for k, v in kw.items()}},
                  sample_index0=s) for s, c in ((0, 2), (2, 1))]
    assert torch.equal(torch.cat(parts, 0), one)
    sel = imp.mask.bool()
    assert torch.equal(one[sel], imp.known[sel])


# ---------------------------------------------------------------------------------------------------------------- the other two forms
# against the row-less form and against the step-by-step loop (row-less kernels: the same bits as the row-less native loop), on the
# golden's case.  Measured on the MI355X over the six (sampler, clip) cases, against either partner (the same bits): a bound is 20x the
# SMALLEST of its form's six figures, and never above what test_cdm_ddim_loop_in_every_sampling_form allows the same pair of forms
# (7e-5 / 1.4e-4).
FORM_TOL = {"folded rows": 5.0e-5,            # 2.6e-6 .. 4.1e-6
            "layer by layer": 5.8e-5}         # 2.9e-6 .. 4.8e-6
assert FORM_TOL["folded rows"] <= 7e-5 and FORM_TOL["layer by layer"] <= 1.4e-4


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_folded_rows_and_layer_by_layer_forms(cdm, sampler, clip):
    d, loop, progressive = _sampler(SAMPLERS[sampler])
    imp, kw = _golden_imp(), _golden_kw()
    xT, nz = loop_inputs("cdm_impute_loop", d.num_timesteps)
    args = dict(noise=D(xT), clip_denoised=clip, denoised_fn=imp, model_kwargs=kw, step_noise=D(torch.stack(nz)))
    outs = {}
    for form, attrs in FORMS:
        with _Form(cdm, **attrs):
            outs[form] = loop(cdm, SHAPE, **args).clone()
            if form != "row-less":                  # two sub-batches of one sample each: the update launch of every sub-batch offsets both pointers
                with _Form(cdm, loop_sub_batches=2):
                    assert torch.equal(outs[form], loop(cdm, SHAPE, **args)), form
    step = _last(progressive(cdm, SHAPE, **args))
    sel, want = imp.mask.bool(), (imp.known.clamp(-1, 1) if clip else imp.known)
    for form, o in outs.items():
        assert torch.equal(o[sel], want[sel]), form
        tol = 0.0 if form == "row-less" else FORM_TOL[form]
        report(f"imputing CDM {sampler} clip={clip}, {form} vs step-by-step", o, step, tol)
        report(f"imputing CDM {sampler} clip={clip}, {form} vs row-less", o, outs["row-less"], tol)
    assert not torch.equal(outs["row-less"], outs["folded rows"]) and not torch.equal(outs["row-less"], outs["layer by layer"])      # other code really ran


# ---------------------------------------------------------------------------------------------------------------- reference goldens
# Bounds per form, each <= 20x the error measured on the MI355X (beside it) and never above the tolerance of the non-imputing CDM test of
# that kind: 2e-4 for a forward / p_sample (test_forward_vs_reference_golden), 1e-3 for a DDPM loop (test_loop_vs_reference_golden),
# 1.4e-4 / 1.6e-4 / 2.2e-4 per form for a DDIM loop (test_cdm_ddim_loop_in_every_sampling_form).
FWD, LOOP, DDIM_LOOP = 2e-4, 1e-3, {"row-less": 1.4e-4, "folded rows": 1.6e-4, "layer by layer": 2.2e-4}
TOL_PSAMPLE = {("pred_xstart", "row-less"): 5.6e-5,            # 2.8e-6
               ("pred_xstart", "folded rows"): 5.7e-5,         # 2.9e-6
               ("pred_xstart", "layer by layer"): 7.8e-5,      # 3.9e-6
               ("sample", "row-less"): 1.0e-5,                 # 5.4e-7 (coef1 is small at t = 499 and the noise term is exact)
               ("sample", "folded rows"): 9.5e-6,              # 4.8e-7
               ("sample", "layer by layer"): 1.1e-5}           # 6.0e-7
TOL_LOOP = {("r5", "row-less"): 1.3e-4,                        # 6.7e-6
            ("r5", "folded rows"): 1.4e-4,                     # 7.2e-6
            ("r5", "layer by layer"): 1.0e-4,                  # 5.5e-6
            ("r5_clip", "row-less"): 1.0e-4,                   # 5.4e-6
            ("r5_clip", "folded rows"): 8.8e-5,                # 4.4e-6
            ("r5_clip", "layer by layer"): 1.4e-4}             # 7.4e-6
TOL_DDIM = {("eta05", "row-less"): 1.1e-4,                     # 5.9e-6
            ("eta05", "folded rows"): 1.2e-4,                  # 6.2e-6
            ("eta05", "layer by layer"): 1.5e-4,               # 7.6e-6
            ("eta0", "row-less"): 1.2e-4,                      # 6.2e-6
            ("eta0", "folded rows"): 1.3e-4,                   # 6.6e-6
            ("eta0", "layer by layer"): 1.1e-4}                # 5.7e-6
assert max(TOL_PSAMPLE.values()) <= FWD and max(TOL_LOOP.values()) <= LOOP and all(b <= DDIM_LOOP[f] for (_, f), b in TOL_DDIM.items())


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
def test_p_sample_vs_reference_golden(cdm, form):
    gs, w64 = golden("cdm_impute_p_sample"), twin64("p_sample")
    x, t, nz = p_sample_inputs()
    d = create_gaussian_diffusion(cdm_cfg(steps=500))
    with _Form(cdm, **dict(FORMS)[form]):
        out = d.p_sample(cdm, D(x), D(t), clip_denoised=False, denoised_fn=_golden_imp(), model_kwargs=_golden_kw(), noise=D(nz))
    assert torch.equal(out["pred_xstart"].cpu()[contact_mask()], contact_known()[contact_mask()])
    for k in ("pred_xstart", "sample"):
        report(f"imputing CDM p_sample {k}, {form}", out[k], gs[k], TOL_PSAMPLE[k, form])
        report_f32_class(f"imputing CDM p_sample {k}, {form}", out[k], gs[k], w64[k], TOL_PSAMPLE[k, form])


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("tag", list(DDPM_LOOPS))
def test_ddpm_loop_vs_reference_golden(cdm, tag, form):
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="5"))
    xT, nz = loop_inputs("cdm_impute_loop", d.num_timesteps)
    want = golden(f"cdm_impute_loop_{tag}")["sample"]
    with _Form(cdm, **dict(FORMS)[form]):
        native = d.p_sample_loop(cdm, SHAPE, noise=D(xT), clip_denoised=DDPM_LOOPS[tag], denoised_fn=_golden_imp(), model_kwargs=_golden_kw(),
                                 step_noise=D(torch.stack(nz)))
    report(f"imputing native CDM DDPM loop {tag}, {form}", native, want, TOL_LOOP[tag, form])
    report_f32_class(f"imputing native CDM DDPM loop {tag}, {form}", native, want, twin64(tag), TOL_LOOP[tag, form])


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("tag", list(DDIM_LOOPS))
def test_ddim_loop_vs_reference_golden(cdm, tag, form):
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="ddim5"))
    xT, nz = loop_inputs("cdm_impute_ddim_loop", d.num_timesteps)
    want = golden(f"cdm_impute_ddim_loop_ddim5_{tag}")["sample"]
    with _Form(cdm, **dict(FORMS)[form]):
        native = d.ddim_sample_loop(cdm, SHAPE, noise=D(xT), clip_denoised=False, denoised_fn=_golden_imp(), model_kwargs=_golden_kw(),
                                    eta=DDIM_LOOPS[tag], step_noise=D(torch.stack(nz)))
    report(f"imputing native CDM DDIM loop ddim5 {tag}, {form}", native, want, TOL_DDIM[tag, form])
    report_f32_class(f"imputing native CDM DDIM loop ddim5 {tag}, {form}", native, want, twin64("ddim_" + tag), TOL_DDIM[tag, form])


# ---------------------------------------------------------------------------------------------------------------- launches
def test_imputing_cdm_jobs_launch_what_the_plain_loops_launch(cdm):
    """A second imputing job launches no ATen arithmetic; in the row-less form no impute_kernel and no sampling_update_kernel either - the
    select rides in dec_point - and exactly as many kernels as the loop without imputation.  The other two forms store pred_xstart and add
    the update launch: one per step (layer by layer: for DDPM only, its DDIM loop has that launch already)."""
    n = 6
    imp, kw = _golden_imp(), _golden_kw()
    d5 = create_gaussian_diffusion(cdm_cfg(steps=500, respacing=str(n)))
    dd = create_gaussian_diffusion(cdm_cfg(steps=500, respacing=f"ddim{n}"))
    kernels = lambda names: sum(c for k, c in names.items() if not _MOVERS.search(k))
    named = lambda names, what: sum(c for k, c in names.items() if what in k)
    runs = {"ddpm": lambda fn: d5.p_sample_loop(cdm, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=kw, seed=5),
            "ddim": lambda fn: dd.ddim_sample_loop(cdm, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=kw, eta=0.0, seed=5)}
    count = {}
    for form, attrs in FORMS:
        with _Form(cdm, **attrs):
            for name, run in runs.items():
                run(imp), run(None)                                   # (weight pack, workspaces and streams exist before anything is counted)
                torch.cuda.synchronize()
                with_imp, without = _device_kernel_names(lambda: run(imp)), _device_kernel_names(lambda: run(None))
                _check(with_imp, f"imputing native CDM loop ({name}, {form})")
                assert not named(with_imp, "impute_kernel"), with_imp
                count[form, name] = (kernels(with_imp), kernels(without), named(with_imp, "sampling_update_kernel"),
                                     named(without, "sampling_update_kernel"), named(with_imp, "dec_point_imputing_kernel"))
    print(f"[cdm impute launches] {n} steps, (kernels with, without, update launches with, without, imputing dec_point): {count}")
    for name in runs:
        k_with, k_without, u_with, u_without, dp = count["row-less", name]
        assert k_with == k_without and u_with == 0 and u_without == 0 and dp == n, (name, count["row-less", name])
        assert count["folded rows", name][0] == count["folded rows", name][1] + n and count["folded rows", name][2:4] == (n, 0)
    assert count["layer by layer", "ddpm"][0] == count["layer by layer", "ddpm"][1] + n and count["layer by layer", "ddpm"][2:4] == (n, 0)
    assert count["layer by layer", "ddim"][0] == count["layer by layer", "ddim"][1] and count["layer by layer", "ddim"][2:4] == (n, n)


# ---------------------------------------------------------------------------------------------------------------- two stages
def test_two_stage_sample_imputes_the_contact_stage(cdm):
    from afm import dist as adist
    from test_gpu_cmdm import cmdm_cfg
    from test_impute_host import impute_known, impute_mask
    cmdm = create_model(cmdm_cfg(), device=dev())
    load_named_weights(cmdm)
    cmdm = cmdm.to(dev()).eval()
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="3"))
    B, N, L = 2, 1024, 16
    text, xyz = D(synth.text_feature(B)), D(synth.scene_cloud(B, N, seed=14))
    args = dict(text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9)
    known = D(synth.gaussian("impute_cdm_known", (B, N, 6)))
    cimp = Impute(known, D(synth.gaussian("impute_cdm_bits", (N, 1)) > 0.5))          # whole points pinned, the same ones in both samples
    mimp = Impute(D(impute_known()), D(impute_mask()))
    sel = cimp.mask.bool()
    base = two_stage_sample(cdm, d_adm, cmdm, d_amdm, **args)
    for extra in ({}, dict(sampler="ddim", eta=0.5)):
        ref = base if not extra else two_stage_sample(cdm, d_adm, cmdm, d_amdm, **extra, **args)
        got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, contact_impute=cimp, **extra, **args)
        assert torch.equal(got["contact"][sel], known[sel]), extra                   # pinned: bit for bit
        assert not torch.equal(got["contact"][~sel], ref["contact"][~sel]), extra    # and the free points react to it
        assert not torch.equal(got["motion"], ref["motion"])
    # the two stages by hand, with the same seeds
    contact = d_adm.p_sample_loop(cdm, (B, N, 6), clip_denoised=False, denoised_fn=cimp, model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), seed=9)
    cond = adist.adm_to_amdm_condition(contact, sigma=0.8, mean=0.0, std=1.0)
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=cond, x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    motion = d_amdm.p_sample_loop(cmdm, (B, L, 263), clip_denoised=False, denoised_fn=mimp, model_kwargs=kw, seed=10)
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, contact_impute=cimp, motion_impute=mimp, **args)
    assert torch.equal(got["contact"], contact) and torch.equal(got["cond"], cond) and torch.equal(got["motion"], motion)
    # motion_impute alone leaves the contact stage what it was
    only = two_stage_sample(cdm, d_adm, cmdm, d_amdm, motion_impute=mimp, **args)
    assert torch.equal(only["contact"], base["contact"]) and torch.equal(only["cond"], base["cond"])


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table; committed as profiles/cdm_impute_parity.json)."""
    write_parity_table()
