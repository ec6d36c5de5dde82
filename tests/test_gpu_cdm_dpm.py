"""`-m gpu`: DPM-Solver++(2M) sampling inside the CDM's native loops (CDM.afm_native_loop with dpm_order=, afm_cdm_dpm_loop_range).

Bit for bit: the default (row-less) form - update, imputation select and the history of the previous step's final pred_xstart fused into
dec_point (dec_point_dpm_kernel) - against the step-by-step loop (CDM.forward, the Impute, the clamp, afm_dpm_step per step), sliced one
range call per step so that the history crosses calls, and against itself over sub-batches, the pipelined and chain-side forms and
shards.  The folded-rows and layer-by-layer forms against the row-less one, and every form against the loop restated around the CPU
oracle (tests/test_cdm_dpm_host.py): report() with a bound derived from the float32 oracle's own error and never above what
test_cdm_ddim_loop_in_every_sampling_form allows, report_f32_class against the float64 twin.  Shapes as the imputing tests
(tests/test_gpu_cdm_impute.py): the golden's (2, 256, 6); (3, 251, 6) - a partial 16-point tile, 1506 values per sample so that the
history, mask and known bases of samples 1 and 2 are not 16-byte aligned, an uneven split over two sub-batches; (2, 1024, 6) - two
512-point chunks per sample; and the 44-input HUMANISE variant (NKS = 11)."""
import ctypes as C

import pytest
import torch

from afm import ffi, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.diffusion import Impute
from afm.pipeline import two_stage_sample
from gpu_util import dev, load_named_weights, report, report_f32_class, write_parity_table
from test_cdm_dpm_host import CASES, twin, twin_x_T
from test_cdm_impute_host import SHAPE
from test_gpu_cdm import cdm_cfg
from test_gpu_cdm_impute import FORMS, _case, _Form, _golden_imp, _golden_kw
from test_gpu_cfg import _last
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())


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


def _diffusion(respacing="ddim5"):
    return create_gaussian_diffusion(cdm_cfg(steps=500, respacing=respacing))


# ---------------------------------------------------------------------------------------------------------------- row-less form, exact
@pytest.mark.parametrize("with_imp", [False, True], ids=["plain", "impute"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("case", ["golden", "ragged", "two chunks", "humanise"])
def test_row_less_2m_loop_equals_the_step_by_step_loop(cdm, cdm_feat, case, order, clip, with_imp):
    """"ddim5": one two-term step, three three-term steps (order 2) and the final step.  The same expressions must give the same bits."""
    model, shape, kw, imp = _case(cdm, cdm_feat, case)
    d = _diffusion()
    loop = lambda *a, **k: d.dpm_solver_sample_loop(*a, order=order, **k)
    progressive = lambda *a, **k: d.dpm_solver_sample_loop_progressive(*a, order=order, **k)
    fn = imp if with_imp else None
    given = dict(noise=D(synth.gaussian(f"cdm_dpm_xT_{case}", shape)), clip_denoised=clip, denoised_fn=fn, model_kwargs=kw)
    seeded = dict(clip_denoised=clip, denoised_fn=fn, model_kwargs=kw, seed=4, sample_index0=3)          # x_T from Philox
    sel = imp.mask.bool()
    want = imp.known.clamp(-1, 1) if clip else imp.known
    for args in (given, seeded):
        native = loop(model, shape, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, shape, **args)))
        if with_imp:
            assert torch.equal(native[sel], want[sel])                               # the known values, bit for bit
        assert torch.equal(native, loop(model, shape, progress=True, **args))         # one range call per step: the history crosses calls
        snaps = {1: None, d.num_timesteps - 1: None}
        assert torch.equal(native, loop(model, shape, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
    native = loop(model, shape, **given)
    plain = loop(model, shape, **{**given, "denoised_fn": None})
    if with_imp:
        # a NaN wherever nothing is known is never read
        knan = Impute(torch.where(sel, imp.known, torch.full_like(imp.known, float("nan"))), imp.mask)
        assert torch.equal(native, loop(model, shape, **{**given, "denoised_fn": knan}))
        # nothing known: the loop without an Impute
        none = Impute(imp.known, torch.zeros(shape, dtype=torch.bool, device=dev()))
        assert torch.equal(plain, loop(model, shape, **{**given, "denoised_fn": none}))
        assert not torch.equal(plain, native)
    elif order == 2:
        # the history term really ran: not the native DDIM eta = 0 loop, not the first-order solver
        assert not torch.equal(native, d.ddim_sample_loop(model, shape, eta=0.0, **given))
        assert not torch.equal(native, d.dpm_solver_sample_loop(model, shape, order=1, **given))


@pytest.mark.parametrize("with_imp", [False, True], ids=["plain", "impute"])
def test_sub_batches_pipeline_chain_side_and_shards_are_bit_identical(cdm, cdm_feat, with_imp):
    """B = 3: two sub-batches split 2 + 1 (the history, known and mask pointers offset by sb.start * 1506 values); the pipelined and the
    chain-side routes to dec_point; a batch against its shards through Impute.narrow and sample_index0.  "logsnr20": 17 steps."""
    model, shape, kw, imp = _case(cdm, cdm_feat, "ragged")
    d = _diffusion("logsnr20")
    fn = imp if with_imp else None
    args = dict(clip_denoised=False, denoised_fn=fn, model_kwargs=kw, seed=21)
    one = d.dpm_solver_sample_loop(model, shape, **args)
    assert torch.isfinite(one).all()
    for attrs in (dict(loop_sub_batches=2), dict(loop_sub_batches=3), dict(loop_sub_batches=2, pipeline=True), dict(loop_sub_batches=2, chain_side=True)):
        with _Form(model, **attrs):
            assert torch.equal(one, d.dpm_solver_sample_loop(model, shape, **args)), attrs
    parts = [d.dpm_solver_sample_loop(model, (c, shape[1], 6), **{**args, "denoised_fn": imp.narrow(s, c) if with_imp else None,
                                                                  "model_kwargs": {k: v[s:s + c] for k, v in kw.items()}}, sample_index0=s)
             for s, c in ((0, 2), (2, 1))]
    assert torch.equal(torch.cat(parts, 0), one)
    if with_imp:
        sel = imp.mask.bool()
        assert torch.equal(one[sel], imp.known[sel])


# ---------------------------------------------------------------------------------------------------------------- the other two forms, the oracle
_NATIVE = {}


def _native(cdm, case):
    """{form: the native 5-step 2M loop of a CASES case on the goldens' scene}, run once per process"""
    if case not in _NATIVE:
        with_imp, clip = CASES[case]
        args = dict(noise=D(twin_x_T()), clip_denoised=clip, denoised_fn=_golden_imp() if with_imp else None, model_kwargs=_golden_kw())
        d, outs = _diffusion(), {}
        for form, attrs in FORMS:
            with _Form(cdm, **attrs):
                outs[form] = d.dpm_solver_sample_loop(cdm, SHAPE, **args).clone()
                if form != "row-less":              # two sub-batches of one sample each: the update launch of every sub-batch offsets its history
                    with _Form(cdm, loop_sub_batches=2):
                        assert torch.equal(outs[form], d.dpm_solver_sample_loop(cdm, SHAPE, **args)), form
        outs["step by step"] = _last(d.dpm_solver_sample_loop_progressive(cdm, SHAPE, **args))
        _NATIVE[case] = outs
    return _NATIVE[case]


# Against the row-less form and against the step-by-step loop (the same bits: both partners give one figure), on the goldens' scene.
# Measured on the MI355X over the four cases (beside each bound).  A bound is 20x the SMALLEST of its form's four figures, and never above
# what test_cdm_ddim_loop_in_every_sampling_form allows the same pair of forms (7e-5 / 1.4e-4): here 20x the smallest figure is 1.1e-4 /
# 2.4e-4, so the caps are the bounds.
FORM_TOL = {"folded rows": 7.0e-5,            # 5.7e-6 (impute+clip), 9.5e-6 (plain), 1.2e-5 (clip), 2.3e-5 (impute)
            "layer by layer": 1.4e-4}         # 1.2e-5 (plain), 1.2e-5 (impute), 1.3e-5 (impute+clip), 1.7e-5 (clip)


@pytest.mark.parametrize("case", list(CASES))
def test_folded_rows_and_layer_by_layer_forms(cdm, case):
    outs = _native(cdm, case)
    with_imp, clip = CASES[case]
    imp = _golden_imp()
    sel, want = imp.mask.bool(), (imp.known.clamp(-1, 1) if clip else imp.known)
    for form, _ in FORMS:
        o = outs[form]
        if with_imp:
            assert torch.equal(o[sel], want[sel]), form
        tol = 0.0 if form == "row-less" else FORM_TOL[form]
        report(f"CDM 2M {case}, {form} vs step-by-step", o, outs["step by step"], tol)
        report(f"CDM 2M {case}, {form} vs row-less", o, outs["row-less"], tol)
    assert not torch.equal(outs["row-less"], outs["folded rows"]) and not torch.equal(outs["row-less"], outs["layer by layer"])      # other code really ran


# Against the loop restated around the CPU oracle.  old_tol of report_f32_class: the caps of the DDIM loops per form
# (test_cdm_ddim_loop_in_every_sampling_form).  The bound of report() against the float32 twin is not a measured figure but follows from
# the project's standing rule: with e_ref = max|float32 twin - float64 twin| (the reference's own error, computed here: it depends
# on the CPU's float32 GEMM, 1.3e-5 .. 1.6e-5 on one machine and 1.8e-5 .. 2.7e-5 on another, at max|ref| 6.9) and the HIP error against
# the float64 twin allowed 4 e_ref + one float32 ulp of the largest output, the triangle inequality gives max|hip - float32 twin| <=
# 5 e_ref + ulp: 6.5e-5 .. 1.4e-4 - and never above the cap.  (Measured HIP error against the float64 twin: 6.1e-6 .. 2.0e-5.)
DDIM_LOOP = {"row-less": 1.4e-4, "folded rows": 1.6e-4, "layer by layer": 2.2e-4}


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("case", list(CASES))
def test_native_loop_vs_the_oracle(cdm, case, form):
    native = _native(cdm, case)[form]
    want32, want64 = twin(case, False), twin(case, True)
    e_ref = (want32.double() - want64).abs().max().item()
    tol = min(5.0 * e_ref + 2.0 ** -23 * want64.abs().max().item(), DDIM_LOOP[form])
    report(f"native CDM 2M loop ddim5 {case}, {form} vs oracle", native, want32, tol)
    report_f32_class(f"native CDM 2M loop ddim5 {case}, {form}", native, want32, want64, old_tol=DDIM_LOOP[form], margin=4.0)


# ---------------------------------------------------------------------------------------------------------------- launches
def test_2m_cdm_jobs_launch_what_the_ddim_loops_launch(cdm):
    """A second native 2M job launches no ATen arithmetic.  Row-less form: no sampling_update_kernel and no impute_kernel, with and without
    an Impute - update, select and history ride in dec_point - and exactly the kernels of the native DDIM eta = 0 loop of the same step
    count, one dec_point_dpm_kernel per step.  Folded rows: its DDIM loop's count plus one update launch per step.  Layer by layer: its
    DDIM loop's count (that loop has the update launch already)."""
    n = 6
    imp, kw = _golden_imp(), _golden_kw()
    d = _diffusion(f"ddim{n}")
    kernels = lambda names: sum(c for k, c in names.items() if not _MOVERS.search(k))
    named = lambda names, what: sum(c for k, c in names.items() if what in k)
    dpm = lambda fn: d.dpm_solver_sample_loop(cdm, SHAPE, clip_denoised=False, denoised_fn=fn, model_kwargs=kw, seed=5)
    ddim = lambda: d.ddim_sample_loop(cdm, SHAPE, clip_denoised=False, model_kwargs=kw, eta=0.0, seed=5)
    count = {}
    for form, attrs in FORMS:
        with _Form(cdm, **attrs):
            dpm(imp), dpm(None), ddim()                               # (weight pack, workspaces and streams exist before anything is counted)
            torch.cuda.synchronize()
            with_imp, without, base = (_device_kernel_names(f) for f in (lambda: dpm(imp), lambda: dpm(None), ddim))
            for names, what in ((with_imp, "imputing"), (without, "plain")):
                _check(names, f"native CDM 2M loop ({what}, {form})")
                assert not named(names, "impute_kernel"), names
            count[form] = dict(base=kernels(base), with_imp=kernels(with_imp), without=kernels(without),
                               upd_with=named(with_imp, "sampling_update_kernel"), upd_without=named(without, "sampling_update_kernel"),
                               upd_base=named(base, "sampling_update_kernel"), dpm_with=named(with_imp, "dec_point_dpm_kernel"),
                               dpm_without=named(without, "dec_point_dpm_kernel"))
    print(f"[cdm dpm launches] {n} steps: {count}")
    c = count["row-less"]
    assert c["with_imp"] == c["without"] == c["base"] and c["upd_with"] == c["upd_without"] == 0 and c["dpm_with"] == c["dpm_without"] == n, c
    c = count["folded rows"]
    assert c["with_imp"] == c["without"] == c["base"] + n and c["upd_with"] == c["upd_without"] == n and c["upd_base"] == 0, c
    c = count["layer by layer"]
    assert c["with_imp"] == c["without"] == c["base"] and c["upd_with"] == c["upd_without"] == c["upd_base"] == n, c
    assert count["folded rows"]["dpm_with"] == count["layer by layer"]["dpm_without"] == 0


# ---------------------------------------------------------------------------------------------------------------- two stages
def test_two_stage_dpm_imputes_the_contact_stage(cdm):
    from afm import dist as adist
    from test_gpu_cmdm import cmdm_cfg
    cmdm = create_model(cmdm_cfg(), device=dev())
    load_named_weights(cmdm)
    cmdm = cmdm.to(dev()).eval()
    d_adm = _diffusion("ddim5")
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    B, N, L = 2, 1024, 16
    text, xyz = D(synth.text_feature(B)), D(synth.scene_cloud(B, N, seed=14))
    args = dict(text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=9, sampler="dpm++")
    known = D(synth.gaussian("impute_cdm_known", (B, N, 6)))
    cimp = Impute(known, D(synth.gaussian("impute_cdm_bits", (N, 1)) > 0.5))          # whole points pinned, the same ones in both samples
    sel = cimp.mask.bool()
    ref = two_stage_sample(cdm, d_adm, cmdm, d_amdm, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, d_amdm, contact_impute=cimp, **args)
    assert torch.isfinite(got["motion"]).all()
    assert torch.equal(got["contact"][sel], known[sel])                              # pinned: bit for bit
    assert not torch.equal(got["contact"][~sel], ref["contact"][~sel])               # and the free points react to it
    assert not torch.equal(got["motion"], ref["motion"])
    # the two stages by hand, with the same seeds
    contact = d_adm.dpm_solver_sample_loop(cdm, (B, N, 6), clip_denoised=False, denoised_fn=cimp, model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), seed=9)
    cond = adist.adm_to_amdm_condition(contact, sigma=0.8, mean=0.0, std=1.0)
    kw = dict(c_text_feat=text, c_pc_xyz=xyz, c_pc_contact=cond, x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev()))
    motion = d_amdm.dpm_solver_sample_loop(cmdm, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=10)
    assert torch.equal(got["contact"], contact) and torch.equal(got["cond"], cond) and torch.equal(got["motion"], motion)
    # and the contact stage is the step-by-step loop's, bit for bit
    assert torch.equal(contact, _last(d_adm.dpm_solver_sample_loop_progressive(cdm, (B, N, 6), clip_denoised=False, denoised_fn=cimp,
                                                                             model_kwargs=dict(c_text_feat=text, c_pc_xyz=xyz), seed=9)))


# ---------------------------------------------------------------------------------------------------------------- the C entry
def test_c_entry_workspace(cdm):
    lib = ffi.load()
    d = _diffusion()
    B, N, J = SHAPE
    kw = _golden_kw()
    w = cdm._weights()
    x = D(twin_x_T()).clone()
    feat = cdm._features(x, kw)
    tq0, tu, tcu = cdm._text_latent(w, kw, dev())
    tab, rows = d.tables(dev()), d.dpm_tables(dev(), 2)
    sched = ffi.sched_scratch(cdm, d.num_timesteps, B, dev(), ddim=True)
    for nsub in (0, 2):
        need = lib.afm_cdm_dpm_loop_workspace_bytes(C.byref(w), B, N, nsub)
        assert need >= lib.afm_cdm_loop_workspace_bytes(C.byref(w), B, N, nsub) + B * N * J * 4      # the history buffers are this loop's alone
    need = lib.afm_cdm_dpm_loop_workspace_bytes(C.byref(w), B, N, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())

    def call(nbytes, r=rows.rows()):
        return lib.afm_cdm_dpm_loop_range(C.byref(w), x.data_ptr(), feat.data_ptr(), tq0.data_ptr(), tu.data_ptr(), tcu.data_ptr(),
                                          tab.timestep_map.data_ptr(), C.byref(r), None, None, d.num_timesteps, 0, B, N, sched.data_ptr(),
                                          ws.data_ptr(), nbytes, 0, None, ffi.stream_of(x))
    assert call(need - 1) == -2                  # AFM_E_WORKSPACE, as every loop of the library refuses a short workspace
    assert call(lib.afm_cdm_loop_workspace_bytes(C.byref(w), B, N, 0)) == -2      # the other loops' size is not enough
    assert torch.equal(x, D(twin_x_T()))         # a refused call touched nothing
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, _native(cdm, "plain")["row-less"])


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table; committed as profiles/cdm_dpm_parity.json)."""
    write_parity_table()
