"""`-m gpu`: scene clearance (SceneClearance, MotionGuidance with a clearance).  The gradient and the energy of both forms against the
float64 restatement of tests/test_clearance_host.py, bounded by the error of the same expressions in float32 torch (`_bound_row` of
tests/test_gpu_guidance.py); every option; the exact zeros; bit-identity run to run and against the sample alone; the sum with the contact
and the target guidance, bit for bit; the natively guided loops (afm_cmdm_scene_guide_loop_range) against the step-by-step loops; zero
scale and a late start; the effect on the energy; launches; argument errors.  All kernel cases run at B = 3, L = 7."""
import ctypes as C
import functools

import pytest
import torch

from afm import ffi, synth
from afm.base import create_gaussian_diffusion
from afm.diffusion import ContactGuidance, Impute, JointTargets, MotionGuidance, SceneClearance
from afm.pipeline import two_stage_sample
from gpu_util import PARITY_ROWS, dev, write_parity_table
from test_clearance_host import (EFFECT_RADIUS, EFFECT_SCALE, MIN_HEIGHT_1100, OPTIONS, case_options, clear_case, clearance_reference, coverage,
                                 effect_scene, h3d_clear_case, h3d_clearance_reference, h3d_radius, nontrivial)
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import FORMS, SHAPE3, _bound_row, _imp3, _kw3, _model, _sampler, cdm, cmdm          # noqa: F401 (cmdm, cdm: fixtures)
from test_gpu_guidance import _guide as _pos_contact
from test_gpu_h3d_guidance import _guide as _h3d_contact
from test_gpu_joint_targets import _loop_targets, _sum_case
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_guidance_host import SCATTERED, SIGMA
from test_h3d_guidance_host import ZUP

pytestmark = pytest.mark.gpu
D = lambda t: None if t is None else t.to(dev())
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)
B = 3
# DESIGN.md 4.4, per guided step and sub-batch: the clearance's launches, alone or behind the other terms'
CLEAR_KERNELS = {"pos": ("clear_kernel",), "h3d": ("h3d_recover_kernel", "clear_kernel", "h3d_adjoint")}
COLUMN_CASES = [(130, 6, 66), (1100, 3, 66)]          # N is no multiple of 64; 1100 crosses the 1024-point tile
VARIANTS = list(OPTIONS) + ["floor"]                    # floor: the min_height that leaves the 1100-point case joint-frames without an obstacle


def _options(name, N, K):
    return dict(min_height=MIN_HEIGHT_1100) if name == "floor" else case_options(name, N, K)


def _clear(g, sl=slice(None), **kw):
    """the SceneClearance of a case (its samples `sl`)"""
    args = dict(radius=g["radius"], scale=g["scale"][sl], up=g.get("up", 2), min_height=g.get("min_height"), exempt_contact=g.get("exempt_contact"),
                weight=None if g.get("weight") is None else g["weight"][sl], **kw)
    if "joints" in g:
        ts = g["to_scene"]
        return SceneClearance.h3d(g["joints"], g["mean"], g["std"], to_scene=D(ts[sl] if ts is not None and ts.dim() == 3 else ts), **args)
    return SceneClearance(g["cols"], g["mean"], g["std"], **args)


def _kw(g, sl=slice(None)):
    kw = dict(c_pc_xyz=D(g["q"][sl]), x_mask=D(g["x_mask"][sl]))
    if "c" in g:
        kw["c_pc_contact"] = D(g["c"][sl])
    return kw


@functools.lru_cache(maxsize=None)
def _column(case, name):
    """the case's inputs and its float64 / float32 restatements, computed once and shared (read-only)"""
    g = clear_case(*case, **_options(name, case[0], case[1]))
    return g, clearance_reference(**g), clearance_reference(**g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _h3d(name):
    g = h3d_clear_case(**{"radius": h3d_radius(), **case_options(name, 130, 6)})
    return g, h3d_clearance_reference(**g), h3d_clearance_reference(**g, dtype=torch.float32)


def _kernel_checks(tag, g, want64, e64, want32, e32, named):
    """what both forms share: the bound, the exact zeros, the same bits run to run and for the sample alone, t_start"""
    guide = _clear(g)
    x, kw = D(g["x"]), _kw(g)
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    got, energy = guide(x, t, **kw), guide.energy(x, **kw)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (B,)
    _bound_row(f"clearance grad {tag}", got, want32, want64)
    _bound_row(f"clearance energy {tag}", energy, e32, e64)
    gc = got.cpu()
    assert torch.isfinite(gc).all() and not gc[..., ~named].any() and not gc[g["x_mask"]].any() and not gc[2].any() and energy[2].item() == 0.0
    assert gc[0].abs().max() > 0 and gc[1].abs().max() > 0 and (energy[:2] > 0).all()
    assert torch.equal(bits(got), bits(guide(x, t, **kw))) and torch.equal(bits(energy), bits(guide.energy(x, **kw)))
    for b in range(B):
        alone, kwb = _clear(g, slice(b, b + 1)), _kw(g, slice(b, b + 1))
        assert torch.equal(bits(alone(x[b:b + 1], t[:1], **kwb)), bits(got[b:b + 1]))
        assert torch.equal(bits(alone.energy(x[b:b + 1], **kwb)), bits(energy[b:b + 1]))
    pair = _clear(g, slice(1, 3))                               # another place in another batch
    assert torch.equal(bits(pair(x[1:], t[1:], **_kw(g, slice(1, 3)))), bits(got[1:]))
    part = _clear(g, t_start=500)(x, torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(bits(part[1:]), bits(got[1:]))
    return got, energy


# ---------------------------------------------------------------------------------------------------------------- the column form
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("case", COLUMN_CASES, ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_column_clearance_vs_float64(case, name):
    N, K, Dm = case
    g, (want64, e64), (want32, e32) = _column(case, name)
    if (N, name) in ((130, "plain"), (1100, "floor")):          # a quarter of the joint-frames pushed, at least one left alone
        print(f"[clearance] N={N} {name}: joint-frames with an obstacle inside the radius {coverage(g)}")
        assert nontrivial(g)
    named = torch.zeros(Dm, dtype=torch.bool)
    for col in g["cols"]:
        named[col:col + 3] = True
    got, energy = _kernel_checks(f"columns N={N} K={K} {name}", g, want64, e64, want32, e32, named)
    # a joint-frame without an obstacle point inside its radius: exactly zero
    idx = torch.tensor([[col + a for a in range(3)] for col in g["cols"]])
    alone = (want64[:, :, idx] == 0).all(-1)                    # [B, L, K]: the float64 sums are exactly zero there
    assert not got.cpu()[:, :, idx][alone].any() and (nontrivial(g) is False or alone[:2][~g["x_mask"][:2]].any())
    if name != "plain":                                          # the option changes the result as the reference says
        plain = _clear(_column(case, "plain")[0])(D(g["x"]), torch.zeros(B, dtype=torch.int64, device=dev()), **_kw(g))
        assert not torch.equal(got, plain) and not torch.equal(want64, _column(case, "plain")[1][0])
    # without a mask the padded frames are guided too
    open_ = {**g, "x_mask": torch.zeros_like(g["x_mask"])}
    free = _clear(g)(D(g["x"]), torch.zeros(B, dtype=torch.int64, device=dev()), **{k: v for k, v in _kw(g).items() if k != "x_mask"})
    _bound_row(f"clearance grad columns N={N} K={K} {name} no mask", free, clearance_reference(**open_, dtype=torch.float32)[0], clearance_reference(**open_)[0])


# ---------------------------------------------------------------------------------------------------------------- the h3d form
@pytest.mark.parametrize("name", list(OPTIONS))
def test_h3d_clearance_vs_float64(name):
    g, (want64, e64), (want32, e32) = _h3d(name)
    if name == "plain":
        r = h3d_radius()
        print(f"[clearance] h3d radius {r}: joint-frames with an obstacle inside the radius {coverage(g)}")
        assert nontrivial(g) and all(not all(s >= 0.25 for s, _ in coverage(h3d_clear_case(radius=q)).values()) for q in (0.25, 0.5, 1.0, 2.0) if q < r)
    named = torch.zeros(263, dtype=torch.bool)
    named[:67] = True
    got, _ = _kernel_checks(f"h3d {name}", g, want64, e64, want32, e32, named)
    guided = [c for j in g["joints"] if j for c in range(4 + 3 * (j - 1), 7 + 3 * (j - 1))] + ([3] if 0 in g["joints"] else [])
    assert not got.cpu()[..., [c for c in range(3, 67) if c not in guided]].any()          # joints that are not guided
    if name != "plain":
        plain = _clear(_h3d("plain")[0])(D(g["x"]), torch.zeros(B, dtype=torch.int64, device=dev()), **_kw(g))
        assert not torch.equal(got, plain)


# ---------------------------------------------------------------------------------------------------------------- the sum
def _sum_clearance(form, **kw):
    """a clearance on the motion of `_sum_case(form)` (tests/test_gpu_joint_targets.py): joints of its own, an exemption by the case's map"""
    from test_guidance_host import guide_case
    from test_h3d_guidance_host import h3d_case
    kw = dict(radius=[0.5, 0.8, 0.6], scale=torch.tensor([2.0, 0.4, 1.0]), exempt_contact=0.9, **kw)
    if form == "h3d":
        c = h3d_case((7, 130, 6, 263, "small", "per_sample"))
        return SceneClearance.h3d([0, 12, 7], c["mean"], c["std"], to_scene=D(c["to_scene"]), **kw)
    c = guide_case(130, 6, 66 if form == "pos66" else 263)
    return SceneClearance(c["cols"][1:3] + [6 if form == "pos66" else 200], c["mean"], c["std"], **kw)


@pytest.mark.parametrize("form", ["pos66", "pos263", "h3d"])
def test_the_sum_equals_the_terms_added_bit_for_bit(form):
    mk_c, mk_t, x, kw = _sum_case(form)
    t = torch.tensor([500, 499, 0], device=dev())
    for tc, tt, ts in ((None, None, None), (500, None, None), (None, 500, 300), (None, None, 500), (500, 300, 500), (0, 0, 0)):
        contact, targets, clear = mk_c(t_start=tc), mk_t(t_start=tt), _sum_clearance(form, t_start=ts)
        a, b, c = contact(x, t, **kw), targets(x, t, **kw), clear(x, t, **kw)
        three = MotionGuidance(contact, targets, clear)
        got = three(x, t, **kw)
        assert torch.equal(bits(got), bits(a + b + c)), (form, tc, tt, ts)
        assert torch.equal(bits(got), bits(three(x, t, **kw)))
        assert torch.equal(bits(MotionGuidance(contact, clearance=clear)(x, t, **kw)), bits(a + c))
        assert torch.equal(bits(MotionGuidance(targets=targets, clearance=clear)(x, t, **kw)), bits(b + c))
        assert torch.equal(bits(MotionGuidance(clearance=clear)(x, t, **kw)), bits(c))
        if ts == 500:
            assert not c[0].any() and torch.equal(got[0], (a + b)[0])          # (values: adding the zeros turns a -0 into +0)
        if tc is None and tt is None and ts is None:
            assert a[1].abs().max() > 0 and b[1].abs().max() > 0 and c[1].abs().max() > 0 and c[0].abs().max() > 0
        ec, et = three.energies(x, **kw)
        assert torch.equal(bits(ec), bits(contact.energy(x, **kw))) and torch.equal(bits(et), bits(targets.energy(x, **kw)))
        g, fm, keep = three.describe(x, kw)
        from afm import ops
        _, ec3, et3, el3 = ops.scene_guidance(g, x, fm, grad=False, energy=True)          # the three energies of one call
        assert torch.equal(bits(ec3), bits(ec)) and torch.equal(bits(et3), bits(et)) and torch.equal(bits(el3), bits(clear.energy(x, **kw)))
    assert MotionGuidance(clearance=clear).energies(x, **kw) == (None, None)


# ---------------------------------------------------------------------------------------------------------------- native loops, exact
def _loop_clearance(repr_, **kw):
    """a clearance for the loops' batch SHAPE3 on the model's 263 columns, on the scene of `_kw3`: three joints, radius 1"""
    kw.setdefault("scale", torch.tensor([0.5, 1.0, 0.25]))
    kw.setdefault("radius", [1.0, 0.8, 1.2])
    if repr_ == "h3d":
        c = _h3d_contact()
        kw.setdefault("to_scene", D(ZUP))
        return SceneClearance.h3d([0, 20, 5], c.mean, c.std, **kw)
    c = _pos_contact()
    return SceneClearance([SCATTERED[1] - 3, 150, SCATTERED[3]], c.mean, c.std, **kw)


def _loop_guide(repr_, terms, d, **kw):
    """the clearance alone (guided from executed step 1 on), or contact (from step 3) + targets (from step 2) + clearance"""
    clear = _loop_clearance(repr_, t_start=d.timestep_map[3] + 1, **kw)
    if terms == "clearance":
        return clear
    contact = (_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=d.timestep_map[1] + 1)
    return MotionGuidance(contact, _loop_targets(repr_, t_start=d.timestep_map[2] + 1), clear)


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("how", ["unguided", "one scale", "two scales"])
@pytest.mark.parametrize("terms", ["clearance", "all three"])
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
@pytest.mark.parametrize("form", list(FORMS) + ["ddim1"])
def test_native_guided_loop_equals_the_step_by_step_loop(cmdm, form, repr_, terms, how, imputing):
    if form == "ddim1":                                         # DDIM with eta = 1: the noise term next to the gradient term
        d = _sampler("ddim")[0]
        loop = lambda *a, **k: d.ddim_sample_loop(*a, eta=1.0, **k)
        progressive = lambda *a, **k: d.ddim_sample_loop_progressive(*a, eta=1.0, **k)
    else:
        d, loop, progressive = _sampler(form)
    guide = _loop_guide(repr_, terms, d)
    assert guide.first_guided(d) == 1 and (terms == "clearance" or (guide.contact.first_guided(d), guide.targets.first_guided(d)) == (3, 2))
    model = _model(cmdm, how)
    args = dict(clip_denoised=imputing, denoised_fn=_imp3() if imputing else None, cond_fn=guide, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        native = loop(model, SHAPE3, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": None}))
        if terms != "clearance":                                # the clearance acts next to the other two
            assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": MotionGuidance(guide.contact, guide.targets)}))
        assert torch.equal(native, loop(model, SHAPE3, progress=True, **args))
        snaps = {1: None, 2: None, 3: None}                     # a range-sliced call, cut where each term starts
        assert torch.equal(native, loop(model, SHAPE3, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False      # two streams: sub-batches of 2 + 1
        assert torch.equal(native, loop(model, SHAPE3, **args))
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


@pytest.mark.parametrize("repr_", ["pos", "h3d"])
@pytest.mark.parametrize("form,how", [("ddpm", "unguided"), ("ddim", "two scales"), ("2m", "unguided")])
def test_zero_scale_and_a_late_start_reproduce_the_unguided_loop(cmdm, form, how, repr_):
    """as tests/test_gpu_guidance.py has it for the contact term: for ("ddpm", "unguided") the unguided loop of the same (separate-update)
    form is the step-by-step one"""
    d, loop, progressive = _sampler(form)
    model = _model(cmdm, how)
    args = dict(clip_denoised=False, model_kwargs=_kw3(), seed=4)
    plain = _last(progressive(model, SHAPE3, **args)) if (form, how) == ("ddpm", "unguided") else loop(model, SHAPE3, **args)
    for guide in (_loop_clearance(repr_, scale=0.0), _loop_clearance(repr_, t_start=0), _loop_clearance(repr_, scale=torch.zeros(3))):
        assert torch.equal(loop(model, SHAPE3, cond_fn=guide, **args), plain)
        assert torch.equal(_last(progressive(model, SHAPE3, cond_fn=guide, **args)), plain)


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_clearance_lowers_the_energy_of_every_sample_that_has_one():
    """The effect inputs of tests/test_joint_targets_host.py with the scene tests/test_clearance_host.py adds to them (linear betas, ddim5,
    t_start = 601, the identity denoiser: a DDIM eta = 0 step is the unguided chain's step plus one gradient-descent step on E).  The guided
    chain ends at a lower energy than the unguided one for every sample whose unguided energy is > 0.  Two runs compared; no threshold."""
    g = effect_scene()
    guide = SceneClearance(g["cols"], g["mean"], g["std"], radius=EFFECT_RADIUS, scale=EFFECT_SCALE, t_start=g["t_start"])
    cfg = cmdm_cfg(steps=1000, respacing="ddim5")
    cfg.diffusion.noise_schedule = "linear"
    d = create_gaussian_diffusion(cfg)
    assert list(d.timestep_map) == [0, 200, 400, 600, 800] and guide.first_guided(d) == 1
    shape = tuple(g["start"].shape)
    identity = lambda x, t, **_: x
    kw = dict(c_pc_xyz=D(g["q"]))
    args = dict(noise=D(g["start"]), clip_denoised=False, model_kwargs=kw, eta=0.0, device=dev())
    plain, guided = d.ddim_sample_loop(identity, shape, **args), d.ddim_sample_loop(identity, shape, cond_fn=guide, **args)
    e_start, e_plain, e_guided = guide.energy(D(g["start"]), **kw), guide.energy(plain, **kw), guide.energy(guided, **kw)
    print(f"[clearance effect] energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
    has = e_plain > 0
    assert has[:2].all() and (e_guided[has] < e_plain[has]).all() and (e_guided[~has] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
def test_guided_jobs_launch_no_eager_arithmetic_and_the_documented_launch_counts(cmdm, cdm, repr_):
    n = 6
    kw = _kw3()
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    kernels = lambda names: sum(c for k, c in names.items() if "guide_gather_kernel" in k or not _MOVERS.search(k))
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    assert not any(_MOVERS.search(k) for ks in CLEAR_KERNELS.values() for k in ks)
    none = Impute(D(synth.gaussian("guide_known", SHAPE3)), torch.zeros(SHAPE3, dtype=torch.bool, device=dev()))
    sep = lambda fn: none if fn is None else None              # the loop of the same (separate-update) form without guidance
    run = lambda fn: dd.ddim_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5)
    per_step = len(CLEAR_KERNELS[repr_])
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        # the clearance from executed step 1 on (5 guided steps), the contact term from step 2 on (4)
        clear = _loop_clearance(repr_, t_start=dd.timestep_map[4] + 1)
        both = MotionGuidance((_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=dd.timestep_map[3] + 1), clearance=clear)
        assert clear.first_guided(dd) == 1 and both.contact.first_guided(dd) == 2
        run(clear), run(both), run(None)                          # (weight pack, workspaces, rows and streams exist before anything is counted)
        torch.cuda.synchronize()
        with_s, with_b, without = (_device_kernel_names(lambda fn=fn: run(fn)) for fn in (clear, both, None))
        _check(with_s, f"clearance-guided native loop ({repr_})")
        _check(with_b, f"contact- and clearance-guided native loop ({repr_})")
        print(f"[clearance launches] {repr_}: kernels clearance {kernels(with_s)}, contact + clearance {kernels(with_b)}, without {kernels(without)}")
        assert count(with_s, "sampling_update_kernel") == count(with_b, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
        assert kernels(with_s) == kernels(without) + per_step * 5
        assert kernels(with_b) == kernels(without) + per_step * 5 + (4 if repr_ == "h3d" else 2) * 4
        assert count(with_s, "clear_kernel") == count(with_b, "clear_kernel") == 5
        if repr_ == "h3d":
            assert count(with_s, "h3d_recover_kernel") == 5 and count(with_b, "h3d_recover_kernel") == 5 + 4          # once per term
            assert count(with_s, "h3d_adjoint_kernel") == 5 and count(with_s, "h3d_adjoint_add_kernel") == 0
            assert count(with_b, "h3d_adjoint_add_kernel") == 4 and count(with_b, "h3d_adjoint_kernel") == 1 + 4
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # both stages, the motion stage guided by the first stage's own map and pushed off the scene, the marked points exempt
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    Bn, N, L = 2, 1024, 16
    args = dict(text_feat=D(synth.text_feature(Bn)), xyz=D(synth.scene_cloud(Bn, N, seed=14)), frames=L, sigma=SIGMA, seed=9, sampler="ddim")
    s2 = _loop_clearance(repr_, scale=2.0, exempt_contact=0.6)
    c2 = (_h3d_contact if repr_ == "h3d" else _pos_contact)(scale=2.0)
    two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, clearance=s2, **args)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, clearance=s2, **args))
    _check(names, "two_stage_sample(contact_guidance=..., clearance=...)")
    assert count(names, "clear_kernel") == n
    base = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, **args)
    only = two_stage_sample(cdm, d_adm, cmdm, dd, clearance=s2, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, clearance=s2, **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"])
    assert not torch.equal(got["motion"], base["motion"]) and not torch.equal(got["motion"], only["motion"])
    kw2 = dict(c_text_feat=args["text_feat"], c_pc_xyz=args["xyz"], c_pc_contact=base["cond"], x_mask=torch.zeros(Bn, L, dtype=torch.bool, device=dev()))
    by_hand = dd.ddim_sample_loop(cmdm, (Bn, L, 263), clip_denoised=False, cond_fn=MotionGuidance(c2, clearance=s2), model_kwargs=kw2, seed=10)
    assert torch.equal(got["motion"], by_hand)


def test_the_entries_a_guidance_reaches(cmdm, monkeypatch):
    """anything that carries a clearance: afm_cmdm_scene_guide_loop_range alone; sums without one keep the entries they reach today"""
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
    a = run(_loop_clearance("pos"))
    b = run(MotionGuidance(clearance=_loop_clearance("pos")))
    run(MotionGuidance(_pos_contact(), _loop_targets("pos"), _loop_clearance("pos")))
    assert set(seen) == {"afm_cmdm_scene_guide_loop_range"} and torch.equal(a, b)
    seen.clear()
    run(_pos_contact())
    run(MotionGuidance(_pos_contact(), _loop_targets("pos")))
    assert seen == ["afm_cmdm_guide_loop_range", "afm_cmdm_motion_guide_loop_range"]


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _SceneLoopProbe:
    """The loaded library with afm_cmdm_scene_guide_loop_range wrapped: in front of every real call, the same call with a description that
    must be refused - AFM_E_BADARG each, returned before anything is enqueued."""
    GUIDE = 15

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_scene_guide_loop_range":
            return fn

        def call(*args):
            real = args[self.GUIDE]._obj
            some = args[1]                                      # a valid device pointer, not the one the terms name
            keep = []

            def variant(change):
                g = ffi.SceneGuide.from_buffer_copy(real)
                s = ffi.SceneClearance.from_buffer_copy(real.clearance.contents)
                lay = ffi.H3dLayout.from_buffer_copy(s.h3d.contents) if s.h3d else None
                change(g, s, lay)
                if lay is not None and s.h3d:
                    s.h3d = C.pointer(lay)
                if g.clearance:
                    g.clearance = C.pointer(s)
                keep.append((g, s, lay))
                return g

            def neither(g, s, lay): g.terms, g.clearance = None, None
            def k0(g, s, lay): s.K = 0
            def k17(g, s, lay): s.K = 17
            def no_gk(g, s, lay): g.gk = None
            def neg(g, s, lay): s.first_guided = -1
            def no_q(g, s, lay): s.q = None
            def n0(g, s, lay): s.N = 0
            def r0(g, s, lay): s.radius[1] = 0.0
            def rneg(g, s, lay): s.radius[0] = -0.5
            def up3(g, s, lay): s.up = 3
            def upneg(g, s, lay): s.up = -1
            def exempt_no_c(g, s, lay): s.exempt, s.c = 1, None
            changes = [neither, k0, k17, no_gk, neg, no_q, n0, r0, rneg, up3, upneg, exempt_no_c]
            if real.clearance.contents.h3d:
                def out_of_range(g, s, lay): lay.joints[1] = 22
                def twice(g, s, lay): lay.joints[1] = lay.joints[0]
                def stride(g, s, lay): lay.to_scene_stride = 5
                changes += [out_of_range, twice, stride]
            else:
                def leaves(g, s, lay): s.cols[0] = 262
                def overlaps(g, s, lay): s.cols[1] = s.cols[0] + 2
                changes += [leaves, overlaps]
            if real.terms:
                def other_mean(g, s, lay): s.mean = some
                def other_std(g, s, lay): s.std = some
                changes += [other_mean, other_std]
                if real.clearance.contents.h3d:
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
        for repr_, terms in (("pos", "clearance"), ("h3d", "all three"), ("pos", "all three"), ("h3d", "clearance")):
            guide = _loop_guide(repr_, terms, d)
            runs.append(lambda loop=loop, guide=guide: loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=_kw3(), seed=4))
    want = [run().clone() for run in runs]
    probe = _SceneLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == len(runs) and all(torch.equal(a, b) for a, b in zip(want, got))
    monkeypatch.undo()
    # afm_scene_guidance itself: D < 67 with h3d, an energy of a term that is not set, a workspace too small; nothing is enqueued
    lib = ffi.load()
    g = _h3d("plain")[0]
    x = D(g["x"])
    L = x.shape[1]
    guide = MotionGuidance(clearance=_clear(g))
    desc, fm, keep = guide.describe(x, _kw(g))
    need = int(lib.afm_scene_guidance_workspace_bytes(C.byref(desc), B, L, 263))
    assert need > 0 and lib.afm_scene_guidance_workspace_bytes(C.byref(desc), B, L, 66) == -1 and lib.afm_scene_guidance_workspace_bytes(None, B, L, 263) == -1
    ws, grad, e = torch.empty(need, dtype=torch.uint8, device=dev()), torch.full_like(x, 7.0), torch.full((B,), 7.0, device=dev())
    call = lambda Dm, nbytes, ec=None: lib.afm_scene_guidance(C.byref(desc), x.data_ptr(), fm.data_ptr(), None, grad.data_ptr(), ec, None, e.data_ptr(), B, L,
                                                              Dm, ws.data_ptr(), nbytes, ffi.stream_of(x))
    assert call(66, need) == -1 and call(263, need, e.data_ptr()) == -1 and call(263, 64) == -2
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (e == 7.0).all()
    assert call(263, need) == 0
    t0 = torch.zeros(B, dtype=torch.int64, device=dev())
    assert torch.equal(grad, guide(x, t0, **_kw(g))) and torch.equal(e, guide.clearance.energy(x, **_kw(g)))


def test_zz_write_parity_table():
    """Not a check: stores the ratios measured so far (gpu_util.write_parity_table; committed as profiles/clearance_parity.json), with the
    rule `_bound_row` applied in place of the writer's general one."""
    import json
    path = write_parity_table()
    if path and any("clearance" in r["name"] for r in PARITY_ROWS):
        table = json.load(open(path))
        table["rule"] = ("rows named 'clearance ...': max|hip - f64| <= 4 * max|f32 torch - f64| + 4 * 2^-23 max|f64| (max norm only, no "
                         "rms); ratio_max = e_hip / (e_ref + floor / 4), floor = 4 * 2^-23 max|f64|")
        json.dump(table, open(path, "w"), indent=1)
