"""`-m gpu`: imputation of known motion values (afm.diffusion.Impute, ops.impute / ops.impute_step, the imputing native loops of
afm_cmdm_impute_loop_range) against the CPU float32 expression (bit for bit), the product's own forms against each other (bit for bit),
and the reference goldens of tools/make_goldens_impute.py.

Bounds against the reference follow tests/test_gpu_cfg.py: at most 20x the error measured on the MI355X (in the comment beside each) and
never above a ceiling - 2e-4 for a forward or p_sample, 1e-3 for a DDPM loop, 6e-5 for a DDIM loop, times AMP = 14 for the guided cases.
The select amplifies nothing, so there is no new ceiling.  Beside every report() stands report_f32_class (tests/gpu_util.py) against the
float64 twin of the oracle wrapped with the same select (tests/test_impute_host.py)."""
import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.diffusion import Impute
from afm.pipeline import two_stage_sample
from conftest import golden
from gpu_util import dev, load_named_weights, report, report_f32_class, write_parity_table
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import AMP, DDIM_LOOP, FWD, LOOP, _last
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_impute_host import (DDIM_LOOPS, DDPM_LOOPS, SCALE, SHAPE, ddim_loop_ref, impute_known, impute_mask, imputed, loop_inputs,
                              oracle_model)

pytestmark = pytest.mark.gpu
ODD = (3, 5, 263)               # 1315 values per sample: a partial last quad, sample bases of the mask not 4-aligned
D = lambda t: t.to(dev())


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


def _imp():
    return Impute(D(impute_known()), D(impute_mask()))


def _model(cmdm, guided):
    return GuidedCMDM(cmdm, torch.tensor(SCALE, device=dev())) if guided else cmdm


# ---------------------------------------------------------------------------------------------------------------- kernels, exact
def _masks(shape):
    """a random mask, and one with an all-zero and an all-one sample (a third sample stays random)"""
    rnd = synth.gaussian(f"impute_bits_{shape[0]}", shape) > 0.3
    edge = rnd.clone()
    edge[0], edge[1] = False, True
    return {"random": rnd, "zero/one": edge, "none": torch.zeros(shape, dtype=torch.bool)}


def _cpu_x0(c, u, s, k, m, clip):
    v = c if u is None else u + s.view(-1, 1, 1) * (c - u)
    v = torch.where(m, k, v)
    return v.clamp(-1, 1) if clip else v


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_impute_kernels_equal_the_cpu_expression(guided, clip):
    d = create_gaussian_diffusion(cmdm_cfg())
    tab = d.tables(dev())
    v = lambda r: r.cpu().view(-1, 1, 1)
    for shape in (SHAPE, ODD):
        B = shape[0]
        c, u, x, nz, k = (synth.gaussian(f"impute_k_{n}_{B}", shape) for n in ("c", "u", "x", "nz", "known"))
        s = torch.tensor([2.5, 7.5, 0.0][:B])
        if not guided:
            u, s = None, None
        g = {} if not guided else dict(x0_u=D(u), scale=D(s))
        plain = c if not guided else _cpu_x0(c, u, s, k, torch.zeros(shape, dtype=torch.bool), False)
        for mname, m in _masks(shape).items():
            # the select alone (on the combined x0 when guided), out of place and in place on x0
            assert torch.equal(ops.impute(D(plain), D(k), D(m)).cpu(), torch.where(m, k, plain)), (mname, shape)
            assert torch.equal(ops.impute(D(plain), D(k), D(m).to(torch.uint8) * 7).cpu(), torch.where(m, k, plain))       # nonzero = known
            buf = D(plain).clone()
            assert ops.impute(buf, D(k), D(m), out=buf) is buf and torch.equal(buf.cpu(), torch.where(m, k, plain))
            x0 = _cpu_x0(c, u, s, k, m, clip)
            knan = torch.where(m, k, torch.full_like(k, float("nan")))          # NaN wherever nothing is known: must never be read
            assert torch.equal(ops.impute(D(plain), D(knan), D(m)).cpu(), torch.where(m, k, plain))
            for tt in (999, 500, 1, 0):
                t = torch.tensor([tt, 3, 0][:B], device=dev())
                c1, c2, sg = tab.coef1[t], tab.coef2[t], tab.sigma[t]
                want = (v(c1) * x0 + v(c2) * x) + v(sg) * nz
                got = ops.impute_step(D(c), D(k), D(m), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip, **g)
                assert torch.equal(got.cpu(), want), ("ddpm", mname, tt, shape)
                assert torch.equal(got, ops.impute_step(D(c), D(knan), D(m), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip, **g)) \
                    and torch.isfinite(got).all(), ("nan", mname, tt)
                # the launches of the step-by-step path give the same bits: (cfg_combine,) impute, clamp_, ddpm_step
                x0d = ops.impute(ops.cfg_combine(D(c), D(u), D(s)) if guided else D(c), D(k), D(m))
                if clip:
                    x0d = ops.clamp_(x0d, -1.0, 1.0)
                assert torch.equal(got, ops.ddpm_step(x0d, D(x), D(nz), c1, c2, sg))
                phil = ops.impute_step(D(c), D(k), D(m), D(x), None, ddpm=(c1, c2, sg), clip=clip, seed=11, sample_index0=3, step=7, **g)
                given = ops.randn(shape, dev(), seed=11, sample_index0=3, step=7)
                assert torch.equal(phil, ops.impute_step(D(c), D(k), D(m), D(x), given, ddpm=(c1, c2, sg), clip=clip, **g))
                if mname == "none":         # nothing known: the update without imputation, exactly
                    ref = ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip) if guided else \
                        ops.ddpm_step(ops.clamp_(D(c).clone(), -1.0, 1.0) if clip else D(c), D(x), D(nz), c1, c2, sg)
                    assert torch.equal(got, ref)
                for eta in (0.0, 1.0):
                    rows = d.ddim_tables(dev(), eta)
                    a, b, cc, dd = (r[t] for r in (rows.a, rows.b, rows.c, rows.d))
                    sgd = None if rows.sigma is None else rows.sigma[t]
                    eps = (v(a) * x - x0) / v(b)
                    want = x0 * v(cc) + v(dd) * eps
                    if sgd is not None:
                        want = want + v(sgd) * nz
                    got = ops.impute_step(D(c), D(k), D(m), D(x), D(nz), ddim=(a, b, cc, dd, sgd), clip=clip, **g)
                    assert torch.equal(got.cpu(), want), ("ddim", mname, tt, eta, shape)
                    assert torch.equal(got, ops.impute_step(D(c), D(knan), D(m), D(x), D(nz), ddim=(a, b, cc, dd, sgd), clip=clip, **g))
                    assert torch.equal(got, ops.ddim_step(x0d, D(x), D(nz), a, b, cc, dd, sgd))
                    if mname == "none":
                        ref = ops.cfg_step(D(c), D(u), D(s), D(x), D(nz), ddim=(a, b, cc, dd, sgd), clip=clip) if guided else \
                            ops.ddim_step(ops.clamp_(D(c).clone(), -1.0, 1.0) if clip else D(c), D(x), D(nz), a, b, cc, dd, sgd)
                        assert torch.equal(got, ref)
            out = D(x).clone()                                       # in place on x_t, as the loops run it
            ops.impute_step(D(c), D(k), D(m), out, D(nz), ddpm=(c1, c2, sg), clip=clip, out=out, **g)
            assert torch.equal(out, ops.impute_step(D(c), D(k), D(m), D(x), D(nz), ddpm=(c1, c2, sg), clip=clip, **g))


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _ImputeLoopProbe:
    """The loaded library with afm_cmdm_impute_loop_range wrapped: in front of every real call, the same call with `known` but no `mask`,
    with a negative first_step, and with neither kind of rows - AFM_E_BADARG each, returned before anything is enqueued."""
    ROWS, C1, KNOWN, MASK, FIRST_STEP = 6, 7, 11, 12, 14

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_impute_loop_range":
            return fn

        def call(*args):
            for change in ({self.MASK: None}, {self.KNOWN: None}, {self.FIRST_STEP: -1}, {self.ROWS: None, self.C1: None}):
                bad = list(args)
                for i, val in change.items():
                    bad[i] = val
                assert fn(*bad) == -1, change
            self.calls += 1
            return fn(*args)
        return call


def test_loop_argument_errors_leave_the_next_call_untouched(cmdm, monkeypatch):
    g = golden("cmdm_forward_N1024_L16")
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    imp = _imp()
    runs = [lambda m=m, loop=loop: getattr(d5, loop)(m, SHAPE, clip_denoised=False, denoised_fn=imp, model_kwargs=_kw(g), seed=4)
            for m in (cmdm, _model(cmdm, True)) for loop in ("p_sample_loop", "ddim_sample_loop")]
    want = [run().clone() for run in runs]
    probe = _ImputeLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == 4 and all(torch.equal(a, b) for a, b in zip(want, got))


# ---------------------------------------------------------------------------------------------------------------- reference goldens
def test_p_sample_vs_reference_golden(cmdm):
    g, gs = golden("cmdm_forward_N1024_L16"), golden("cmdm_impute_p_sample_t500")
    d = create_gaussian_diffusion(cmdm_cfg())
    nz = synth.gaussian("p_sample_noise_500", SHAPE)
    out = d.p_sample(cmdm, D(g["x"]), torch.tensor([500, 500], device=dev()), clip_denoised=False, denoised_fn=_imp(), model_kwargs=_kw(g),
                     noise=D(nz))
    assert torch.equal(out["pred_xstart"].cpu()[impute_mask()], impute_known()[impute_mask()])
    report("imputing p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], TOL_PSAMPLE["pred_xstart"])
    report("imputing p_sample t=500 sample", out["sample"], gs["sample"], TOL_PSAMPLE["sample"])
    from oracle import diffusion_ref as df
    w64 = df.p_sample(df.Schedule(1000), imputed(oracle_model(False, f64=True)), g["x"].double(), torch.tensor([500, 500]), nz.double())
    report_f32_class("imputing p_sample t=500 pred_xstart", out["pred_xstart"], gs["pred_xstart"], w64["pred_xstart"], TOL_PSAMPLE["pred_xstart"])
    report_f32_class("imputing p_sample t=500 sample", out["sample"], gs["sample"], w64["sample"], TOL_PSAMPLE["sample"])


@pytest.mark.parametrize("tag", list(DDPM_LOOPS))
def test_ddpm_loop_vs_reference_golden(cmdm, tag):
    guided, clip = DDPM_LOOPS[tag]
    from oracle import diffusion_ref as df
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    xT, nz = loop_inputs("loop_r5", d.num_timesteps)
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_impute_loop_{tag}")["sample"]
    native = d.p_sample_loop(_model(cmdm, guided), SHAPE, noise=D(xT), clip_denoised=clip, denoised_fn=_imp(), model_kwargs=_kw(g),
                             step_noise=D(torch.stack(nz)))
    report(f"imputing native DDPM loop {tag}", native, want, TOL_LOOP[tag])
    want64 = df.p_sample_loop(df.Schedule(1000, "cosine", "5"), imputed(oracle_model(guided, f64=True)), xT.double(), [z.double() for z in nz],
                              clip_denoised=clip)
    report_f32_class(f"imputing native DDPM loop {tag}", native, want, want64, TOL_LOOP[tag])


@pytest.mark.parametrize("tag", list(DDIM_LOOPS))
def test_ddim_loop_vs_reference_golden(cmdm, tag):
    guided, eta = DDIM_LOOPS[tag]
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim50"))
    xT, nz = loop_inputs("ddim_loop_ddim50", d.num_timesteps)
    g, want = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_impute_ddim_loop_ddim50_{tag}")["sample"]
    native = d.ddim_sample_loop(_model(cmdm, guided), SHAPE, noise=D(xT), clip_denoised=False, denoised_fn=_imp(), model_kwargs=_kw(g), eta=eta,
                                step_noise=D(torch.stack(nz)))
    report(f"imputing native DDIM loop ddim50 {tag}", native, want, TOL_DDIM[tag])
    want64 = ddim_loop_ref(imputed(oracle_model(guided, f64=True)), xT.double(), [z.double() for z in nz], eta)
    report_f32_class(f"imputing native DDIM loop ddim50 {tag}", native, want, want64, TOL_DDIM[tag])


# Measured on the MI355X, each bound <= 20x its measurement and <= its ceiling:
TOL_PSAMPLE = {"pred_xstart": 6.6e-5,           # 3.3e-6; ceiling FWD = 2e-4
               "sample": 4.8e-6}                # 2.4e-7 (coef1 is small at t = 500)
TOL_LOOP = {"r5": 7.4e-5,                       # 3.7e-6; ceiling LOOP = 1e-3
            "r5_clip": 6.8e-5,                  # 3.4e-6
            "cfg_r5": 2.0e-3}                   # 1.0e-4; ceiling LOOP * AMP = 1.4e-2
TOL_DDIM = {"eta0": DDIM_LOOP,                  # 3.8e-6: 20x is above the ceiling DDIM_LOOP = 6e-5, so the ceiling
            "eta1": DDIM_LOOP,                  # 3.7e-6: likewise
            "cfg_eta0": DDIM_LOOP * AMP}        # 5.1e-5: 20x is above the ceiling DDIM_LOOP * AMP = 8.4e-4, so the ceiling
assert max(TOL_PSAMPLE.values()) <= FWD and all(b <= LOOP * (AMP if "cfg" in k else 1) for k, b in TOL_LOOP.items()) \
    and all(b <= DDIM_LOOP * (AMP if "cfg" in k else 1) for k, b in TOL_DDIM.items())


# ---------------------------------------------------------------------------------------------------------------- forms, exact
FORMS = {"ddpm": (False, None), "ddim_eta0": (False, 0.0), "ddim_eta1": (False, 1.0), "cfg_ddpm": (True, None), "cfg_ddim": (True, 0.0)}


def _sampler(form):
    """(diffusion, loop(model, shape, **kw), progressive(model, shape, **kw)) of a form: 5 steps"""
    _, eta = FORMS[form]
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5" if eta is None else "ddim5"))
    if eta is None:
        return d, d.p_sample_loop, d.p_sample_loop_progressive
    return d, (lambda *a, **k: d.ddim_sample_loop(*a, eta=eta, **k)), (lambda *a, **k: d.ddim_sample_loop_progressive(*a, eta=eta, **k))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
def test_native_imputing_loop_in_every_form(cmdm, form, clip):
    guided = FORMS[form][0]
    d, loop, progressive = _sampler(form)
    g, imp, model = golden("cmdm_forward_N1024_L16"), _imp(), _model(cmdm, guided)
    xT, nz = loop_inputs("loop_r5", d.num_timesteps)
    args = dict(noise=D(xT), clip_denoised=clip, denoised_fn=imp, model_kwargs=_kw(g), step_noise=D(torch.stack(nz)))
    native = loop(model, SHAPE, **args)
    assert torch.isfinite(native).all()
    assert torch.equal(native, _last(progressive(model, SHAPE, **args)))          # the same kernels and forms compute the same bits
    assert torch.equal(native, loop(model, SHAPE, progress=True, **args))
    snaps = {1: None, d.num_timesteps - 1: None}
    assert torch.equal(native, loop(model, SHAPE, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
    want = impute_known().clamp(-1, 1) if clip else impute_known()
    assert torch.equal(native.cpu()[impute_mask()], want[impute_mask()])           # what a user relies on: the known values, bit for bit
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        seeded = dict(clip_denoised=clip, denoised_fn=imp, model_kwargs=_kw(g), seed=4)          # Philox noise drawn by the loop
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        one = loop(model, SHAPE, **seeded)
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False
        assert torch.equal(one, loop(model, SHAPE, **seeded))
        cmdm.pair_launch = True                                 # ignored by an imputing loop: it runs unpaired
        assert torch.equal(one, loop(model, SHAPE, **seeded))
        cmdm.pair_launch = False
        if guided:
            model.branch_streams = True                         # two sub-batches, four streams; then one sub-batch, two streams
            assert torch.equal(one, loop(model, SHAPE, **seeded))
            cmdm.loop_streams, cmdm.loop_streams_auto = 1, True
            assert torch.equal(one, loop(model, SHAPE, **seeded))
            model.branch_streams = False
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved
    # L = 15: 3945 values per sample, the update's last quad and its K-padded row copy end on a partial quad, the mask bases are odd
    odd = (2, 15, 263)
    kw = dict(c_text_feat=D(g["text_feat"]), c_cont_emb=D(g["cont_emb"]), x_mask=D(synth.frame_mask(2, 15, min_len=8)))
    oimp = Impute(D(synth.gaussian("impute_known_L15", odd)), D(synth.gaussian("impute_bits_L15", odd) > 0.3))
    oargs = dict(noise=D(synth.gaussian("loop_r5_L15_xT", odd)), clip_denoised=clip, denoised_fn=oimp, model_kwargs=kw,
                 step_noise=D(torch.stack([synth.gaussian(f"loop_r5_L15_{j}", odd) for j in range(d.num_timesteps)])))
    assert torch.equal(loop(model, odd, **oargs), _last(progressive(model, odd, **oargs)))
    # nothing known: the DDIM and guided loops are the existing native loops exactly; the DDPM loop is the STEP-BY-STEP unguided loop
    # exactly (the native unguided DDPM loop runs the contracted update fused into its last GEMM and may differ in the last bit)
    none = Impute(D(impute_known()), torch.zeros(SHAPE, dtype=torch.bool, device=dev()))
    empty = loop(model, SHAPE, **{**args, "denoised_fn": none})
    plain = {**args, "denoised_fn": None}
    assert torch.equal(empty, _last(progressive(model, SHAPE, **plain)))
    if form != "ddpm":
        assert torch.equal(empty, loop(model, SHAPE, **plain))
    assert not torch.equal(empty, native)


def test_sharded_imputation_equals_the_whole_batch(cmdm):
    """Impute.narrow: the samples of a rank, with Philox noise keyed by the global sample index."""
    g, imp = golden("cmdm_forward_N1024_L16"), _imp()
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    full = d.p_sample_loop(cmdm, SHAPE, clip_denoised=False, denoised_fn=imp, model_kwargs=_kw(g), seed=21)
    kw = {k: v for k, v in _kw(g).items() if k != "info_dummy"}
    parts = [d.p_sample_loop(cmdm, (1, 16, 263), clip_denoised=False, denoised_fn=imp.narrow(i, 1), model_kwargs={k: v[i:i + 1] for k, v in kw.items()},
                             seed=21, sample_index0=i) for i in range(2)]
    assert torch.equal(torch.cat(parts, 0), full)


# ---------------------------------------------------------------------------------------------------------------- launches
def test_imputing_jobs_launch_no_eager_arithmetic_and_the_derived_launch_counts(cmdm):
    g, imp = golden("cmdm_forward_N1024_L16"), _imp()
    n = 6
    d5 = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=str(n)))
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    guided = _model(cmdm, True)
    kernels = lambda names: sum(c for k, c in names.items() if not _MOVERS.search(k))
    updates = lambda names: sum(c for k, c in names.items() if "sampling_update_kernel" in k)
    runs = {"ddpm": lambda fn: d5.p_sample_loop(cmdm, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=_kw(g), seed=5),
            "ddim": lambda fn: dd.ddim_sample_loop(cmdm, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=_kw(g), eta=0.0, seed=5),
            "cfg": lambda fn: d5.p_sample_loop(guided, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=_kw(g), seed=5)}
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        count = {}
        for name, run in runs.items():
            run(imp), run(None)                                   # (weight pack, workspaces and streams exist before anything is counted)
            torch.cuda.synchronize()
            with_imp, without = _device_kernel_names(lambda: run(imp)), _device_kernel_names(lambda: run(None))
            _check(with_imp, f"imputing native loop ({name})")
            assert not any("impute_kernel" in k for k in with_imp), with_imp          # the select rides in the update launch
            count[name] = (kernels(with_imp), kernels(without), updates(with_imp), updates(without))
        print(f"[impute launches] {n} steps, (kernels with, without, update launches with, without): {count}")
        assert count["ddim"][0] == count["ddim"][1] and count["ddim"][2:] == (n, n)
        assert count["cfg"][0] == count["cfg"][1] and count["cfg"][2:] == (n, n)
        assert count["ddpm"][0] == count["ddpm"][1] + n and count["ddpm"][2:] == (n, 0)
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # the step-by-step path: the Impute is a denoised_fn whose select is afm_impute
    torch.cuda.synchronize()
    step = _device_kernel_names(lambda: d5.p_sample(cmdm, D(g["x"]), torch.tensor([1, 2], device=dev()), clip_denoised=True, denoised_fn=imp,
                                                    model_kwargs=_kw(g), seed=5))
    _check(step, "imputing p_sample")
    assert any("impute_kernel" in k for k in step)


# ---------------------------------------------------------------------------------------------------------------- two stages
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_two_stage_sample_imputes_the_motion_stage_only(cmdm, cdm):
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="5"))
    B, N, L = 2, 1024, 16
    text, xyz = D(synth.text_feature(B)), D(synth.scene_cloud(B, N, seed=14))
    args = dict(text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9)
    imp = _imp()
    base = two_stage_sample(cdm, d_adm, cmdm, d_amdm, **args)
    for extra in ({}, dict(sampler="ddim", eta=0.5), dict(guidance_scale=2.5)):
        ref = base if not extra else two_stage_sample(cdm, d_adm, cmdm, d_amdm, **extra, **args)
        got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, motion_impute=imp, **extra, **args)
        assert torch.equal(got["contact"], ref["contact"]) and torch.equal(got["cond"], ref["cond"]), extra          # the contact stage: untouched
        assert torch.equal(got["motion"].cpu()[impute_mask()], impute_known()[impute_mask()]), extra
        assert not torch.equal(got["motion"], ref["motion"])
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=base["cond"], x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    by_hand = d_amdm.p_sample_loop(cmdm, (B, L, 263), clip_denoised=False, denoised_fn=imp, model_kwargs=kw, seed=10)
    assert torch.equal(two_stage_sample(cdm, d_adm, cmdm, d_amdm, motion_impute=imp, **args)["motion"], by_hand)


def test_cdm_takes_the_same_impute_step_by_step(cdm):
    """The CDM's native loops are out of scope: an Impute is a plain denoised_fn there, on the step-by-step path, still without ATen math."""
    d = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    shape = (2, 1024, 6)
    kw = dict(c_text_feat=D(synth.text_feature(2)), c_pc_xyz=D(synth.scene_cloud(2, 1024, seed=14)))
    known, mask = D(synth.gaussian("impute_cdm_known", shape)), D(synth.gaussian("impute_cdm_bits", (1024, 1)) > 0.5)
    imp = Impute(known, mask)
    out = d.p_sample_loop(cdm, shape, clip_denoised=False, denoised_fn=imp, model_kwargs=kw, seed=4)
    sel = imp.mask.bool()
    assert torch.equal(out[sel], known[sel]) and torch.isfinite(out).all()
    assert torch.equal(out, d.p_sample_loop(cdm, shape, clip_denoised=False, denoised_fn=lambda x0: ops.impute(x0, known, imp.mask), model_kwargs=kw,
                                            seed=4))


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table; committed as profiles/impute_parity.json)."""
    write_parity_table()
