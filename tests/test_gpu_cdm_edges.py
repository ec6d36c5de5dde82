"""`-m gpu`: the CDM's three sampling forms (row-less: csrc/perceiver_points.hip; folded rows: csrc/perceiver_rows.hip; layer by layer,
and the training composition an autograd forward runs) against float64 at the softmax and value edges tests/test_cdm_edges_host.py builds
and proves on the host: encoder and decoder softmaxes that one point or one latent carries, x_T-sized noise, coordinates in metres, a scene
20 m from the origin, large scene features - at N = 1100, where the encoder reductions have waves with two tiles, with a ragged tile and
with no point.  Everything goes through the model (create_model, no_gen, no_fold, grad_forms); nothing here knows how a kernel is built.

Every forward is bounded by the float32 oracle's OWN error against its float64 twin (gpu_util.report_f32_class, margin 4); the absolute
tolerance is the project's 2e-4 (loops: 1e-3) for outputs up to 5, growing with the outputs.  The figures go to
profiles/cdm_edges_parity.json."""
import contextlib

import pytest
import torch

from afm.base import create_model
from afm.cmdm import _param_version
from gpu_util import dev, grad_forms, load_named_weights, report, report_f32_class, write_parity_table
from test_cdm_edges_host import (B_EDGE, CHAOTIC_LOOP_FAMILY, LOOP_FAMILIES, LOOP_TOL, N_EDGE, SHIFT_FAMILY, SHIFTS, SMALL_B, SMALL_NS, VARIANTS, cases, diffusion,
                                 loop_inputs, loop_reference, old_tol, reference, solver_reference, weight_edits)
from test_gpu_cdm import cdm_cfg

pytestmark = pytest.mark.gpu
FORMS = (("row-less", {}), ("folded rows", dict(no_gen=True)), ("layer by layer", dict(no_fold=True)))


@pytest.fixture(scope="module")
def models():
    out = {}
    for variant, feats in VARIANTS.items():
        m = create_model(cdm_cfg(num_points=64, point_feats=feats), device=dev())
        load_named_weights(m)
        out[variant] = m.to(dev()).eval()
    return out


@contextlib.contextmanager
def edited(model, family):
    """The family's weight edits applied in place to the product model (and taken back): the packs and step-invariant caches are keyed by
    _param_version, which must move."""
    params = dict(model.named_parameters())
    saved = {key: params[key].detach().clone() for key in weight_edits(family)}
    before = _param_version(model)
    try:
        with torch.no_grad():
            for key, factor in weight_edits(family).items():
                params[key].mul_(factor)
        assert not saved or _param_version(model) != before, "an in-place edit must change the parameter version"
        yield model
    finally:
        with torch.no_grad():
            for key, w in saved.items():
                params[key].copy_(w)
        model.no_gen = model.no_fold = False


def forward_in_every_form(model, inp):
    """{form name: result}: the three sampling forms under no_grad (the inference kernels) and each with autograd enabled (the training
    composition).  The pack a form ran on was built for the current parameter version."""
    kw = dict(c_text_feat=inp["text"].to(dev()), c_pc_xyz=inp["xyz"].to(dev()))
    if inp["feat"] is not None:
        kw["c_pc_feat"] = inp["feat"].to(dev())
    x, t = inp["x"].to(dev()), inp["t"].to(dev())
    out = {}
    for form, attrs in FORMS:
        model.no_gen, model.no_fold = bool(attrs.get("no_gen")), bool(attrs.get("no_fold"))
        for suffix, got in grad_forms(lambda: model(x, t, **kw)):
            out[form + suffix] = got.detach().clone()
        assert model._pack is not None and model._pack[0][0] == _param_version(model), "the weight pack was not rebuilt for the edited weights"
    model.no_gen = model.no_fold = False
    return out


GRAD, NO_GRAD = "", " [no_grad: inference kernels]"           # gpu_util.grad_forms' suffixes


def check_forms(what, outs, want32, want64, tol, distinct=True):
    """The three inference forms and the training composition, each in the float32 class.  With autograd enabled no_gen and no_fold
    choose nothing (the per-operator tape runs the layer-by-layer kernels): that is asserted bit for bit and measured once."""
    for form, _ in FORMS[1:]:
        assert torch.equal(outs[form + GRAD], outs[FORMS[0][0] + GRAD]), f"{what}: the training composition depends on {form}"
    rows = [(form, outs[form + NO_GRAD]) for form, _ in FORMS] + [("training composition", outs[FORMS[0][0] + GRAD])]
    for form, got in rows:
        assert torch.isfinite(got).all(), f"{what} ({form}): non-finite values"
        report(f"{what} ({form}) vs oracle", got, want32, tol)
        report_f32_class(f"{what} ({form}) vs oracle", got, want32, want64, tol)
    assert not distinct or not torch.equal(rows[0][1], rows[1][1]) and not torch.equal(rows[0][1], rows[2][1]), f"{what}: other code really ran"


@pytest.mark.parametrize("family,variant", cases())
def test_value_families_stay_in_the_float32_class(models, family, variant):
    inp, want32, want64 = reference(family, variant, B_EDGE, N_EDGE)
    with edited(models[variant], family) as m:
        outs = forward_in_every_form(m, inp)
    check_forms(f"CDM edges {family} {variant} N={N_EDGE}", outs, want32, want64, old_tol(want64))


@pytest.mark.parametrize("shift", SHIFTS)
def test_dominant_point_at_every_partition_edge(models, shift):
    """The cloud rolled by `shift`: the point that carries the most peaked encoder row sits on another edge of the reductions' partition
    (test_cdm_edges_host.py:test_shifts_visit_every_partition_edge).  Both forms with an encoder reduction of their own against the oracle AT
    the rolled cloud; rolled back, the result lies within the absolute tolerance of the unshifted one (equivariance - not bit-identity:
    the points meet other partials)."""
    m = models["k12"]
    inp, want32, want64 = reference(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE, shift)
    base = reference(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE)[0]
    tol = old_tol(want64)
    with edited(m, SHIFT_FAMILY):
        for form, attrs in FORMS[:2]:
            m.no_gen = bool(attrs.get("no_gen"))
            with torch.no_grad():
                got = m(inp["x"].to(dev()), inp["t"].to(dev()), c_text_feat=inp["text"].to(dev()), c_pc_xyz=inp["xyz"].to(dev())).clone()
                unshifted = m(base["x"].to(dev()), base["t"].to(dev()), c_text_feat=base["text"].to(dev()), c_pc_xyz=base["xyz"].to(dev())).clone()
            what = f"CDM edges {SHIFT_FAMILY} rolled by {shift} ({form})"
            report(f"{what} vs oracle", got, want32, tol)
            report_f32_class(f"{what} vs oracle", got, want32, want64, tol)
            report(f"{what} rolled back vs unshifted", torch.roll(got, -shift, 1), unshifted, tol)


@pytest.mark.parametrize("N", SMALL_NS)
def test_small_clouds_with_peaked_softmax(models, N):
    """Fewer points than the 64 partials of a sample: most partials carry m = -inf and no sum, a workgroup's later waves have no point."""
    inp, want32, want64 = reference("both_peaked_30", "k12", SMALL_B, N)
    with edited(models["k12"], "both_peaked_30") as m:
        outs = forward_in_every_form(m, inp)
    check_forms(f"CDM edges both_peaked_30 N={N}", outs, want32, want64, old_tol(want64), distinct=N > 1)      # one point: both softmaxes are trivial


def _native_loops(m, family, snapshots=None):
    """{name: (result, snapshots)} of the native 4-step loops: DDPM on recorded noise in every form, DDIM (eta = 0) and DPM-Solver++(2M) in
    the default form"""
    d = diffusion()
    inp, xT, nz = loop_inputs(family, B_EDGE, N_EDGE)
    shape = (B_EDGE, N_EDGE, 6)
    kw = dict(c_text_feat=inp["text"].to(dev()), c_pc_xyz=inp["xyz"].to(dev()))
    snap = lambda: None if snapshots is None else {k: None for k in snapshots}
    outs = {}
    with edited(m, family):
        for form, attrs in FORMS:
            m.no_gen, m.no_fold = bool(attrs.get("no_gen")), bool(attrs.get("no_fold"))
            sn = snap()
            outs["ddpm, " + form] = (d.p_sample_loop(m, shape, noise=xT.to(dev()), clip_denoised=False, model_kwargs=kw,
                                                     step_noise=torch.stack(nz).to(dev()), snapshots=sn).clone(), sn)
        m.no_gen = m.no_fold = False
        sn = snap()
        outs["ddim, row-less"] = (d.ddim_sample_loop(m, shape, noise=xT.to(dev()), clip_denoised=False, model_kwargs=kw, eta=0.0, snapshots=sn).clone(), sn)
        sn = snap()
        outs["dpm++, row-less"] = (d.dpm_solver_sample_loop(m, shape, noise=xT.to(dev()), clip_denoised=False, model_kwargs=kw, snapshots=sn).clone(), sn)
    return outs


def _loop_reference(family, name, steps=None):
    sampler = name.split(",")[0]
    return loop_reference(family, steps) if sampler == "ddpm" else solver_reference(family, sampler, steps)


CHAOTIC = pytest.mark.xfail(strict=True, reason="four steps through both softmaxes at factor 30 amplify one rounding error beyond any float32 evaluation, the oracle's "
                                                "included: DESIGN.md 4.5 'A 4-step loop of both_peaked_30'; test_cdm_edges_host.py::test_the_both_peaked_loop_is_beyond_float32")


@pytest.mark.parametrize("family", [pytest.param(f, marks=CHAOTIC) if f == CHAOTIC_LOOP_FAMILY else f for f in LOOP_FAMILIES])
def test_four_step_loops_at_the_edges(models, family):
    """Native 4-step loops, where dec_point writes the x_{t-1} the next step's encoder reduction reads, against the same loops around the
    oracle in float32 and float64.  Every loop is measured (and its row recorded) before the first failure is raised."""
    outs = _native_loops(models["k12"], family)
    failures = []
    for name, (got, _) in outs.items():
        want32, want64 = _loop_reference(family, name)
        tol = old_tol(want64, LOOP_TOL)
        for check in (lambda: report_f32_class(f"CDM edges 4-step loop {family} ({name}) vs oracle", got, want32, want64, tol),
                      lambda: report(f"CDM edges 4-step loop {family} ({name}) vs oracle", got, want32, tol)):
            try:
                check()
            except AssertionError as e:
                failures.append(str(e))
    assert not torch.equal(outs["ddpm, row-less"][0], outs["ddpm, folded rows"][0]) and not torch.equal(outs["ddpm, row-less"][0], outs["ddpm, layer by layer"][0])
    assert not failures, "\n".join(failures)


def test_first_step_of_the_both_peaked_loops(models):
    """What IS well-posed under both_peaked_30: the state after one step of each native loop (the fused update behind the peaked decoder,
    taken from the loop's own snapshot) lies in the float32 class of the oracle's one step, and the four steps end finite."""
    for name, (got, snaps) in _native_loops(models["k12"], CHAOTIC_LOOP_FAMILY, snapshots=(1,)).items():
        assert torch.isfinite(got).all(), name
        want32, want64 = _loop_reference(CHAOTIC_LOOP_FAMILY, name, 1)
        tol = old_tol(want64, LOOP_TOL)
        report(f"CDM edges first loop step {CHAOTIC_LOOP_FAMILY} ({name}) vs oracle", snaps[1], want32, tol)
        report_f32_class(f"CDM edges first loop step {CHAOTIC_LOOP_FAMILY} ({name}) vs oracle", snaps[1], want32, want64, tol)


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (committed as profiles/cdm_edges_parity.json)."""
    write_parity_table()
