"""`-m gpu`: foot grounding (FootGrounding, MotionGuidance with a grounding).  The gradient and the energy of both forms against the
float64 restatement of tests/test_grounding_host.py, bounded by the error of the same expressions in float32 torch (`_bound_row` of
tests/test_gpu_guidance.py); every option; the exact zeros; bit-identity run to run and against the sample alone; the sum with the other
three terms, bit for bit; the natively guided loops (afm_cmdm_ground_guide_loop_range) against the step-by-step loops; zero scale and a
late start; the descent step; launches; the pipeline; argument errors.  All kernel cases run at B = 3 and L = 7, 2 or 1."""
import ctypes as C
import functools

import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion
from afm.diffusion import FootGrounding, Impute, MotionGuidance
from afm.pipeline import two_stage_sample
from gpu_util import PARITY_ROWS, dev, write_parity_table
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_clearance import _loop_clearance, _sum_clearance
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import FORMS, SHAPE3, _bound_row, _imp3, _kw3, _model, _sampler, cdm, cmdm          # noqa: F401 (cmdm, cdm: fixtures)
from test_gpu_guidance import _guide as _pos_contact
from test_gpu_h3d_guidance import _guide as _h3d_contact
from test_gpu_joint_targets import _loop_targets, _sum_case
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_grounding_host import (COLUMN_CASES, EPS, H3D_CASES, VARIANTS, case_id, coverage, descent64, effect_case, ground_case, nontrivial, reference,
                                 terms64)
from test_guidance_host import SCATTERED, SIGMA
from test_h3d_guidance_host import ZUP

pytestmark = pytest.mark.gpu
D = lambda t: None if t is None else t.to(dev())
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)
B = 3
# DESIGN.md 4.4, per guided step and sub-batch: the grounding's launches, alone or behind the other terms'
GROUND_KERNELS = {"pos": ("ground_kernel",), "h3d": ("h3d_recover_kernel", "ground_kernel", "h3d_adjoint")}
OWN = ("floor", "height", "up", "floor_weight", "skate_weight", "contact")


def _feet(g, sl=slice(None), **kw):
    """the FootGrounding of a case (its samples `sl`)"""
    args = dict({k: g[k] for k in OWN if k in g}, scale=g["scale"][sl], **kw)
    if "joints" in g:
        return FootGrounding.h3d(g["joints"], g["mean"], g["std"], to_scene=D(g["to_scene"]), **args)
    return FootGrounding(g["cols"], g["mean"], g["std"], **args)


def _kw(g, sl=slice(None)):
    return dict(x_mask=D(g["x_mask"][sl]))


@functools.lru_cache(maxsize=None)
def _case(case, name):
    """the case's inputs and its float64 / float32 restatements, computed once and shared (read-only)"""
    g = ground_case(case, name)
    return g, reference(g), reference(g, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------- both forms against float64
@pytest.mark.parametrize("case,name", VARIANTS, ids=lambda v: case_id(v) if isinstance(v, tuple) else v.replace(" ", "_"))
def test_grounding_vs_float64(case, name):
    form, L, K, Dm, kind = case
    g, (want64, e64), (want32, e32) = _case(case, name)
    tag = f"{case_id(case)} {name}"
    if L == 7 and name in ("plain", "heights", "labels"):
        print(f"[grounding] {tag}: (share of pairs with s > 0, pairs with s == 0, joint-frames below the floor, not below) {coverage(g)}")
        assert nontrivial(g)
    guide = _feet(g)
    x, kw = D(g["x"]), _kw(g)
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    got, energy = guide(x, t, **kw), guide.energy(x, **kw)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (B,)
    _bound_row(f"grounding grad {tag}", got, want32, want64)
    _bound_row(f"grounding energy {tag}", energy, e32, e64)
    # the exact zeros: every column that is not named, padded frames, the sample without a valid frame, a joint-frame left alone
    gc = got.cpu()
    named = torch.zeros(Dm, dtype=torch.bool)
    if form == "h3d":
        named[:67] = True
        guided = [c for j in g["joints"] for c in range(4 + 3 * (j - 1), 7 + 3 * (j - 1))]
        assert not gc[..., [c for c in range(3, 67) if c not in guided]].any()          # joints that are not guided, the root's height
    else:
        for col in g["cols"]:
            named[col:col + 3] = True
        idx = torch.tensor([[col + a for a in range(3)] for col in g["cols"]])
        alone = (terms64(g)[0] == 0).all(-1)                     # [B, L, K]: neither below the floor nor in a pair with s > 0
        assert not gc[:, :, idx][alone].any()
    assert torch.isfinite(gc).all() and not gc[..., ~named].any() and not gc[g["x_mask"]].any() and not gc[2].any() and energy[2].item() == 0.0
    if L == 7:
        assert gc[0].abs().max() > 0 and gc[1].abs().max() > 0 and (energy[:2] > 0).all()
    # the same bits run to run, for each sample alone and for a pair of samples at another place in another batch
    assert torch.equal(bits(got), bits(guide(x, t, **kw))) and torch.equal(bits(energy), bits(guide.energy(x, **kw)))
    for b in range(B):
        alone_b, kwb = _feet(g, slice(b, b + 1)), _kw(g, slice(b, b + 1))
        assert torch.equal(bits(alone_b(x[b:b + 1], t[:1], **kwb)), bits(got[b:b + 1]))
        assert torch.equal(bits(alone_b.energy(x[b:b + 1], **kwb)), bits(energy[b:b + 1]))
    pair = _feet(g, slice(1, 3))
    assert torch.equal(bits(pair(x[1:], t[1:], **_kw(g, slice(1, 3)))), bits(got[1:]))
    # t_start: a sample at or above it gets zeros, the others keep their bits
    part = _feet(g, t_start=500)(x, torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(bits(part[1:]), bits(got[1:]))
    if form == "pos" and kind == "tail" and L == 7:             # without a mask the padded frames are guided too
        open_ = {**g, "x_mask": torch.zeros_like(g["x_mask"])}
        free = guide(x, t)
        _bound_row(f"grounding grad {tag} no mask", free, reference(open_, dtype=torch.float32)[0], reference(open_)[0])


# ---------------------------------------------------------------------------------------------------------------- the sum
def _sum_feet(form, **kw):
    """a grounding on the motion of `_sum_case(form)` (tests/test_gpu_joint_targets.py): joints of its own"""
    from test_guidance_host import guide_case
    from test_h3d_guidance_host import h3d_case
    kw = dict(floor=0.1, height=[1.0, 0.7], floor_weight=0.8, skate_weight=1.5, scale=torch.tensor([0.7, 1.0, 3.0]), **kw)
    if form == "h3d":
        c = h3d_case((7, 130, 6, 263, "small", "per_sample"))
        return FootGrounding.h3d([10, 8], c["mean"], c["std"], to_scene=D(c["to_scene"]), contact="labels", **kw)
    c = guide_case(130, 6, 66 if form == "pos66" else 263)
    return FootGrounding([c["cols"][1], 21 if form == "pos66" else 150], c["mean"], c["std"], **kw)


@pytest.mark.parametrize("form", ["pos66", "pos263", "h3d"])
def test_the_sum_equals_the_terms_added_bit_for_bit(form):
    mk_c, mk_t, x, kw = _sum_case(form)
    t = torch.tensor([500, 499, 0], device=dev())
    for tc, tt, ts, tf in ((None, None, None, None), (500, None, None, 300), (None, 500, 300, None), (None, None, None, 500), (500, 300, 500, 500),
                           (0, 0, 0, 0)):
        contact, targets, clear, feet = mk_c(t_start=tc), mk_t(t_start=tt), _sum_clearance(form, t_start=ts), _sum_feet(form, t_start=tf)
        a, b, c, d = contact(x, t, **kw), targets(x, t, **kw), clear(x, t, **kw), feet(x, t, **kw)
        four = MotionGuidance(contact, targets, clear, feet)
        got = four(x, t, **kw)
        assert torch.equal(bits(got), bits(a + b + c + d)), (form, tc, tt, ts, tf)
        assert torch.equal(bits(got), bits(four(x, t, **kw)))
        # each subset that contains the grounding, in the stated order
        assert torch.equal(bits(MotionGuidance(contact, targets, feet=feet)(x, t, **kw)), bits(a + b + d))
        assert torch.equal(bits(MotionGuidance(contact, clearance=clear, feet=feet)(x, t, **kw)), bits(a + c + d))
        assert torch.equal(bits(MotionGuidance(targets=targets, clearance=clear, feet=feet)(x, t, **kw)), bits(b + c + d))
        assert torch.equal(bits(MotionGuidance(contact, feet=feet)(x, t, **kw)), bits(a + d))
        assert torch.equal(bits(MotionGuidance(targets=targets, feet=feet)(x, t, **kw)), bits(b + d))
        assert torch.equal(bits(MotionGuidance(clearance=clear, feet=feet)(x, t, **kw)), bits(c + d))
        assert torch.equal(bits(MotionGuidance(feet=feet)(x, t, **kw)), bits(d))
        # every subset without it: today's description, today's bits
        three, two = MotionGuidance(contact, targets, clear), MotionGuidance(contact, targets)
        assert isinstance(three.describe(x, kw)[0], ffi.SceneGuide) and isinstance(two.describe(x, kw)[0], ffi.MotionGuide)
        assert isinstance(MotionGuidance(clearance=clear).describe(x, kw)[0], ffi.SceneGuide)
        assert torch.equal(bits(three(x, t, **kw)), bits(a + b + c)) and torch.equal(bits(two(x, t, **kw)), bits(a + b))
        if tf == 500:
            assert not d[0].any() and torch.equal(got[0], (a + b + c)[0])          # (values: adding the zeros turns a -0 into +0)
        if tc is None and tt is None and ts is None and tf is None:
            assert all(v[1].abs().max() > 0 for v in (a, b, c, d)) and d[0].abs().max() > 0
        # the energies of one afm_ground_guidance call equal the terms' own
        g, fm, keep = four.describe(x, kw)
        assert isinstance(g, ffi.GroundGuide)
        _, ec, et, el, ef = ops.ground_guidance(g, x, fm, grad=False, energy=True)
        assert torch.equal(bits(ec), bits(contact.energy(x, **kw))) and torch.equal(bits(et), bits(targets.energy(x, **kw)))
        assert torch.equal(bits(el), bits(clear.energy(x, **kw))) and torch.equal(bits(ef), bits(feet.energy(x, **kw)))
        assert torch.equal(bits(four.feet_energy(x, **kw)), bits(ef))
        e2 = four.energies(x, **kw)
        assert torch.equal(bits(e2[0]), bits(ec)) and torch.equal(bits(e2[1]), bits(et))
    assert MotionGuidance(feet=feet).energies(x, **kw) == (None, None)


# ---------------------------------------------------------------------------------------------------------------- native loops, exact
def _loop_feet(repr_, **kw):
    """a grounding for the loops' batch SHAPE3 on the model's 263 columns: three joints on columns; the four foot joints with the motion's
    own contact labels on h3d"""
    kw.setdefault("scale", torch.tensor([0.5, 1.0, 0.25]))
    kw.setdefault("height", 1.0)
    if repr_ == "h3d":
        c = _h3d_contact()
        kw.setdefault("to_scene", D(ZUP))
        kw.setdefault("contact", "labels")
        return FootGrounding.h3d([7, 10, 8, 11], c.mean, c.std, **kw)
    c = _pos_contact()
    return FootGrounding([150, SCATTERED[3], 200], c.mean, c.std, **kw)


def _loop_guide(repr_, terms, d, **kw):
    """the grounding alone (guided from executed step 1 on), or contact (from step 3) + targets (from step 2) + clearance (from step 2) +
    grounding"""
    feet = _loop_feet(repr_, t_start=d.timestep_map[3] + 1, **kw)
    if terms == "grounding":
        return feet
    contact = (_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=d.timestep_map[1] + 1)
    return MotionGuidance(contact, _loop_targets(repr_, t_start=d.timestep_map[2] + 1), _loop_clearance(repr_, t_start=d.timestep_map[2] + 1), feet)


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("how", ["unguided", "one scale"])
@pytest.mark.parametrize("terms", ["grounding", "all four"])
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
@pytest.mark.parametrize("form", list(FORMS))
def test_native_guided_loop_equals_the_step_by_step_loop(cmdm, form, repr_, terms, how, imputing):
    d, loop, progressive = _sampler(form)
    guide = _loop_guide(repr_, terms, d)
    assert guide.first_guided(d) == 1 and (terms == "grounding" or (guide.contact.first_guided(d), guide.targets.first_guided(d)) == (3, 2))
    model = _model(cmdm, how)
    args = dict(clip_denoised=imputing, denoised_fn=_imp3() if imputing else None, cond_fn=guide, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        native = loop(model, SHAPE3, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": None}))
        if terms != "grounding":                                # the grounding acts next to the other three
            assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": MotionGuidance(guide.contact, guide.targets, guide.clearance)}))
        snaps = {1: None, 2: None, 3: None}                     # a range-sliced call, cut where the terms start
        assert torch.equal(native, loop(model, SHAPE3, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False      # two streams: sub-batches of 2 + 1
        assert torch.equal(native, loop(model, SHAPE3, **args))
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


@pytest.mark.parametrize("repr_", ["pos", "h3d"])
@pytest.mark.parametrize("form,how", [("ddpm", "unguided"), ("ddim", "one scale"), ("2m", "unguided")])
def test_zero_scale_and_a_late_start_reproduce_the_unguided_loop(cmdm, form, how, repr_):
    """as tests/test_gpu_guidance.py has it for the contact term: for ("ddpm", "unguided") the unguided loop of the same (separate-update)
    form is the step-by-step one"""
    d, loop, progressive = _sampler(form)
    model = _model(cmdm, how)
    args = dict(clip_denoised=False, model_kwargs=_kw3(), seed=4)
    plain = _last(progressive(model, SHAPE3, **args)) if (form, how) == ("ddpm", "unguided") else loop(model, SHAPE3, **args)
    for guide in (_loop_feet(repr_, scale=0.0), _loop_feet(repr_, t_start=0), _loop_feet(repr_, scale=torch.zeros(3))):
        assert torch.equal(loop(model, SHAPE3, cond_fn=guide, **args), plain)
        assert torch.equal(_last(progressive(model, SHAPE3, cond_fn=guide, **args)), plain)


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_one_step_along_the_guidance_lowers_the_energy_on_the_device():
    """the descent case of tests/test_grounding_host.py and its recorded step: on the device the energy falls by at least half of what the
    float64 restatement shows"""
    g = effect_case()
    e0_64, e1_64 = descent64(g)
    guide = _feet(g)
    x, kw = D(g["x"]), _kw(g)
    step = guide(x, torch.zeros(B, dtype=torch.int64, device=dev()), **kw)
    e0, e1 = guide.energy(x, **kw).double().cpu(), guide.energy(x + EPS * step, **kw).double().cpu()
    print(f"[grounding descent] eps = {EPS}: float64 {e0_64.tolist()} -> {e1_64.tolist()}, device {e0.tolist()} -> {e1.tolist()}")
    assert (e0_64[:2] - e1_64[:2] >= 0.1 * e0_64[:2]).all()
    assert ((e0 - e1)[:2] >= 0.5 * (e0_64 - e1_64)[:2]).all() and e0[2] == 0 and e1[2] == 0


# ---------------------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
def test_guided_jobs_launch_no_eager_arithmetic_and_the_documented_launch_counts(cmdm, repr_):
    n = 6
    kw = _kw3()
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    kernels = lambda names: sum(c for k, c in names.items() if "guide_gather_kernel" in k or not _MOVERS.search(k))
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    assert not any(_MOVERS.search(k) for ks in GROUND_KERNELS.values() for k in ks)
    none = Impute(D(synth.gaussian("guide_known", SHAPE3)), torch.zeros(SHAPE3, dtype=torch.bool, device=dev()))
    sep = lambda fn: none if fn is None else None              # the loop of the same (separate-update) form without guidance
    run = lambda fn: dd.ddim_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5)
    per_step = len(GROUND_KERNELS[repr_])
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        # the grounding from executed step 2 on (4 guided steps: no grounding kernel before), the contact term from step 3 on (3)
        feet = _loop_feet(repr_, t_start=dd.timestep_map[3] + 1)
        both = MotionGuidance((_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=dd.timestep_map[2] + 1), feet=feet)
        assert feet.first_guided(dd) == 2 and both.contact.first_guided(dd) == 3
        run(feet), run(both), run(None)                           # (weight pack, workspaces, rows and streams exist before anything is counted)
        torch.cuda.synchronize()
        with_f, with_b, without = (_device_kernel_names(lambda fn=fn: run(fn)) for fn in (feet, both, None))
        _check(with_f, f"grounding-guided native loop ({repr_})")
        _check(with_b, f"contact- and grounding-guided native loop ({repr_})")
        print(f"[grounding launches] {repr_}: kernels grounding {kernels(with_f)}, contact + grounding {kernels(with_b)}, without {kernels(without)}")
        assert count(with_f, "sampling_update_kernel") == count(with_b, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
        assert kernels(with_f) == kernels(without) + per_step * 4
        assert kernels(with_b) == kernels(without) + per_step * 4 + (4 if repr_ == "h3d" else 2) * 3
        assert count(with_f, "ground_kernel") == count(with_b, "ground_kernel") == 4 and count(without, "ground_kernel") == 0
        for names in (with_f, with_b):
            assert not any(part in k for k in names for part in ("clear_kernel", "target_cols_kernel", "target_h3d_kernel"))
        if repr_ == "h3d":
            assert count(with_f, "h3d_recover_kernel") == 4 and count(with_b, "h3d_recover_kernel") == 4 + 3          # once per term
            assert count(with_f, "h3d_adjoint_kernel") == 4 and count(with_f, "h3d_adjoint_add_kernel") == 0
            assert count(with_b, "h3d_adjoint_add_kernel") == 3 and count(with_b, "h3d_adjoint_kernel") == 1 + 3
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved


def test_the_entries_a_guidance_reaches(cmdm, monkeypatch):
    """anything that carries a grounding: afm_cmdm_ground_guide_loop_range alone; sums without one keep the entries they reach today"""
    seen = []

    class Spy:
        def __init__(self, lib):
            self.lib = lib

        def __getattr__(self, name):
            if name.endswith("guide_loop_range"):
                seen.append(name)
            return getattr(self.lib, name)

    spy = Spy(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: spy)
    d, loop, _ = _sampler("ddim")
    run = lambda fn: loop(cmdm, SHAPE3, clip_denoised=False, cond_fn=fn, model_kwargs=_kw3(), seed=4)
    a = run(_loop_feet("pos"))
    b = run(MotionGuidance(feet=_loop_feet("pos")))
    run(MotionGuidance(_pos_contact(), _loop_targets("pos"), _loop_clearance("pos"), _loop_feet("pos")))
    run(MotionGuidance(_pos_contact(), feet=_loop_feet("pos")))
    assert set(seen) == {"afm_cmdm_ground_guide_loop_range"} and len(seen) == 4 and torch.equal(a, b)
    seen.clear()
    run(_pos_contact())
    run(MotionGuidance(_pos_contact(), _loop_targets("pos")))
    run(MotionGuidance(_pos_contact(), _loop_targets("pos"), _loop_clearance("pos")))
    run(_loop_clearance("pos"))
    assert seen == ["afm_cmdm_guide_loop_range", "afm_cmdm_motion_guide_loop_range", "afm_cmdm_scene_guide_loop_range", "afm_cmdm_scene_guide_loop_range"]


# ---------------------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
def test_two_stage_sample_with_a_grounding_equals_the_chain_called_by_hand(cmdm, cdm, repr_):
    n = 6
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    Bn, N, L = 2, 1024, 16
    args = dict(text_feat=D(synth.text_feature(Bn)), xyz=D(synth.scene_cloud(Bn, N, seed=14)), frames=L, sigma=SIGMA, seed=9, sampler="ddim")
    f2 = _loop_feet(repr_, scale=2.0)
    c2 = (_h3d_contact if repr_ == "h3d" else _pos_contact)(scale=2.0)
    s2 = _loop_clearance(repr_, scale=2.0, exempt_contact=0.6)
    t2 = None
    base = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, clearance=s2, **args)
    only = two_stage_sample(cdm, d_adm, cmdm, dd, grounding=f2, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, joint_targets=t2, clearance=s2, grounding=f2, **args)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, clearance=s2, grounding=f2, **args))
    _check(names, "two_stage_sample(contact_guidance=..., clearance=..., grounding=...)")
    assert sum(c for k, c in names.items() if "ground_kernel" in k) == n
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"])
    assert not torch.equal(got["motion"], base["motion"]) and not torch.equal(got["motion"], only["motion"])
    kw2 = dict(c_text_feat=args["text_feat"], c_pc_xyz=args["xyz"], c_pc_contact=base["cond"], x_mask=torch.zeros(Bn, L, dtype=torch.bool, device=dev()))
    by_hand = dd.ddim_sample_loop(cmdm, (Bn, L, 263), clip_denoised=False, cond_fn=MotionGuidance(c2, clearance=s2, feet=f2), model_kwargs=kw2, seed=10)
    assert torch.equal(got["motion"], by_hand)
    alone = dd.ddim_sample_loop(cmdm, (Bn, L, 263), clip_denoised=False, cond_fn=f2, model_kwargs=kw2, seed=10)
    assert torch.equal(only["motion"], alone)


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _GroundLoopProbe:
    """The loaded library with afm_cmdm_ground_guide_loop_range wrapped: in front of every real call, the same call with a description that
    must be refused - AFM_E_BADARG each, returned before anything is enqueued."""
    GUIDE = 15

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_ground_guide_loop_range":
            return fn

        def call(*args):
            real = args[self.GUIDE]._obj
            some = args[1]                                      # a valid device pointer, not the one the terms name
            keep = []

            def variant(change):
                g = ffi.GroundGuide.from_buffer_copy(real)
                s = ffi.FootGrounding.from_buffer_copy(real.feet.contents)
                lay = ffi.H3dLayout.from_buffer_copy(s.h3d.contents) if s.h3d else None
                change(g, s, lay)
                if lay is not None and s.h3d:
                    s.h3d = C.pointer(lay)
                if g.feet:
                    g.feet = C.pointer(s)
                keep.append((g, s, lay))
                return g

            def neither(g, s, lay): g.terms, g.feet = None, None
            def k0(g, s, lay): s.K = 0
            def k17(g, s, lay): s.K = 17
            def no_gk(g, s, lay): g.gk = None
            def neg(g, s, lay): s.first_guided = -1
            def no_mean(g, s, lay): s.mean = None
            def h0(g, s, lay): s.height[1] = 0.0
            def hneg(g, s, lay): s.height[0] = -0.5
            def up3(g, s, lay): s.up = 3
            def upneg(g, s, lay): s.up = -1
            def wneg(g, s, lay): s.skate_weight = -1.0
            def wzero(g, s, lay): s.floor_weight, s.skate_weight = 0.0, 0.0
            changes = [neither, k0, k17, no_gk, neg, no_mean, h0, hneg, up3, upneg, wneg, wzero]
            if real.feet.contents.h3d:
                def out_of_range(g, s, lay): lay.joints[1] = 22
                def twice(g, s, lay): lay.joints[1] = lay.joints[0]
                def stride(g, s, lay): lay.to_scene_stride = 5
                def no_label(g, s, lay): s.labels, lay.joints[0] = 1, 0
                changes += [out_of_range, twice, stride, no_label]
            else:
                def leaves(g, s, lay): s.cols[0] = 262
                def overlaps(g, s, lay): s.cols[1] = s.cols[0] + 2
                def labels_on_columns(g, s, lay): s.labels = 1
                changes += [leaves, overlaps, labels_on_columns]
            if real.terms:
                def other_mean(g, s, lay): s.mean = some
                def other_std(g, s, lay): s.std = some
                changes += [other_mean, other_std]
                if real.feet.contents.h3d:
                    def other_scene(g, s, lay): lay.to_scene = some
                    def other_form(g, s, lay): s.h3d = None
                    changes += [other_scene, other_form]
            for change in changes:
                bad = list(args)
                bad[self.GUIDE] = C.byref(variant(change))
                assert fn(*bad) == -1, change.__name__
            bad = list(args)
            bad[self.GUIDE] = None
            assert fn(*bad) == -1
            self.calls += 1
            return fn(*args)
        return call


def test_argument_errors_leave_the_next_call_untouched(cmdm, monkeypatch):
    imp = _imp3()
    runs = []
    for form in FORMS:
        d, loop, _ = _sampler(form)
        for repr_, terms in (("pos", "grounding"), ("h3d", "all four"), ("pos", "all four"), ("h3d", "grounding")):
            guide = _loop_guide(repr_, terms, d)
            runs.append(lambda loop=loop, guide=guide: loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=_kw3(), seed=4))
    want = [run().clone() for run in runs]
    probe = _GroundLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == len(runs) and all(torch.equal(a, b) for a, b in zip(want, got))
    monkeypatch.undo()
    # afm_ground_guidance itself: labels with D < 263, an energy of a term that is not set, a workspace too small; nothing is enqueued
    lib = ffi.load()
    g = _case(("h3d", 7, 4, 263, "tail"), "labels")[0]
    x = D(g["x"])
    L = x.shape[1]
    guide = MotionGuidance(feet=_feet(g))
    desc, fm, keep = guide.describe(x, _kw(g))
    need = int(lib.afm_ground_guidance_workspace_bytes(C.byref(desc), B, L, 263))
    assert need > 0 and lib.afm_ground_guidance_workspace_bytes(None, B, L, 263) == -1
    assert lib.afm_ground_guidance_workspace_bytes(C.byref(desc), B, L, 262) == -1          # labels: the columns 259..262 must exist
    ws, grad, e = torch.empty(need, dtype=torch.uint8, device=dev()), torch.full_like(x, 7.0), torch.full((B,), 7.0, device=dev())
    x262 = x[..., :262].contiguous()
    call = lambda xx, Dm, nbytes, ec=None, el=None: lib.afm_ground_guidance(C.byref(desc), xx.data_ptr(), fm.data_ptr(), None, grad.data_ptr(), ec, None, el,
                                                                           e.data_ptr(), B, L, Dm, ws.data_ptr(), nbytes, ffi.stream_of(x))
    assert call(x262, 262, need) == -1 and call(x, 263, need, ec=e.data_ptr()) == -1 and call(x, 263, need, el=e.data_ptr()) == -1
    assert call(x, 263, 64) == -2
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (e == 7.0).all()
    assert call(x, 263, need) == 0
    t0 = torch.zeros(B, dtype=torch.int64, device=dev())
    assert torch.equal(grad, guide(x, t0, **_kw(g))) and torch.equal(e, guide.feet_energy(x, **_kw(g)))
    big = MotionGuidance(feet=FootGrounding(list(range(0, 48, 3)), g["mean"], g["std"]))          # 16 joints: L = 400 is beyond the LDS
    with pytest.raises(ValueError, match="LDS"):
        big(torch.zeros(1, 400, 263, device=dev()), t0[:1])


def test_zz_write_parity_table():
    """Not a check: stores the ratios measured so far (gpu_util.write_parity_table; committed as profiles/grounding_parity.json), with the
    rule `_bound_row` applied in place of the writer's general one."""
    import json
    path = write_parity_table()
    if path and any("grounding" in r["name"] for r in PARITY_ROWS):
        table = json.load(open(path))
        table["rule"] = ("rows named 'grounding ...': max|hip - f64| <= 4 * max|f32 torch - f64| + 4 * 2^-23 max|f64| (max norm only, no "
                         "rms); ratio_max = e_hip / (e_ref + floor / 4), floor = 4 * 2^-23 max|f64|")
        json.dump(table, open(path, "w"), indent=1)
