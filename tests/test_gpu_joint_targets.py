"""`-m gpu`: joint-position targets (JointTargets, MotionGuidance).  The column-form gradient against the float32 torch CPU expression, bit
for bit; the energies and the h3d gradient against the float64 restatement of tests/test_joint_targets_host.py, bounded by the error of
the same expressions in float32 torch (`_bound_row` of tests/test_gpu_guidance.py); the sum with the contact guidance, bit for bit; the
natively guided loops (afm_cmdm_motion_guide_loop_range) against the step-by-step loops; zero scale and a late start; the effect on the
energy; launches; argument errors."""
import ctypes as C
import functools

import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion
from afm.diffusion import ContactGuidance, Impute, JointTargets, MotionGuidance
from afm.pipeline import two_stage_sample
from gpu_util import PARITY_ROWS, dev, write_parity_table
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import FORMS, SHAPE3, _bound_row, _imp3, _kw3, _model, _sampler, cdm, cmdm          # noqa: F401 (cmdm, cdm: fixtures)
from test_gpu_guidance import _guide as _pos_contact
from test_gpu_h3d_guidance import _guide as _h3d_contact
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_guidance_host import JOINTS, SCATTERED, SIGMA, guide_case
from test_h3d_guidance_host import ZUP
from test_h3d_guidance_host import h3d_case as h3d_contact_case
from test_joint_targets_host import (B, H3D_CASES, cols_case, effect_inputs, h3d_case_id, h3d_targets_case, h3d_targets_reference,
                                     targets_reference)

pytestmark = pytest.mark.gpu
D = lambda t: None if t is None else t.to(dev())
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)
# DESIGN.md 4.4, per guided step and sub-batch: the targets' launches, alone or behind the contact term's (2, h3d 4)
TARGET_KERNELS = {"pos": ("target_cols_kernel",), "h3d": ("h3d_recover_kernel", "target_h3d_kernel", "h3d_adjoint")}
CONTACT_LAUNCHES = {"pos": 2, "h3d": 4}


def _ts(g, sl=slice(None)):
    ts = g.get("to_scene")
    return D(ts[sl] if ts is not None and ts.dim() == 3 else ts)


def _targets(g, sl=slice(None), **kw):
    args = dict(target=g["target"][sl], weight=g["weight"][sl], scale=g["scale"][sl], **kw)
    if "joints" in g:
        return JointTargets.h3d(g["joints"], g["mean"], g["std"], to_scene=_ts(g, sl), **args)
    return JointTargets(g["cols"], g["mean"], g["std"], **args)


# ---------------------------------------------------------------------------------------------------------------- the column form, exact
@pytest.mark.parametrize("L", [1, 2, 7, 300])
@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("Dm", [66, 263])
def test_column_gradient_equals_the_cpu_expression_bit_for_bit(Dm, K, L):
    g = cols_case(L, K, Dm)
    guide = _targets(g)
    x, kw = D(g["x"]), dict(x_mask=D(g["x_mask"]))
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    got, energy = guide(x, t, **kw), guide.energy(x, **kw)
    want32, e32 = targets_reference(**g, dtype=torch.float32)
    want64, e64 = targets_reference(**g)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (B,) and want32.dtype == torch.float32
    assert torch.equal(bits(got), bits(want32))                  # elementwise, so exact - the zeros' signs included
    assert g["x_mask"][2].all() and not got[2].any() and energy[2].item() == 0.0          # the fully padded sample
    assert torch.isfinite(got).all() and (L * K == 1 or g["target"].isnan().any())      # NaN targets under zero weights were never read
    _bound_row(f"joint targets energy columns L={L} K={K} D={Dm}", energy, e32, e64)
    # the same bits run to run, and sample b of the batch is the sample computed alone
    assert torch.equal(bits(got), bits(guide(x, t, **kw))) and torch.equal(bits(energy), bits(guide.energy(x, **kw)))
    for b in range(B):
        alone = _targets(g, slice(b, b + 1))
        kwb = dict(x_mask=kw["x_mask"][b:b + 1])
        assert torch.equal(bits(alone(x[b:b + 1], t[:1], **kwb)), bits(got[b:b + 1]))
        assert torch.equal(bits(alone.energy(x[b:b + 1], **kwb)), bits(energy[b:b + 1]))
    # t_start: a sample at or above it gets zeros, the others what they got; without a mask the padded frames are guided too
    part = _targets(g, t_start=500)(x, torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(bits(part[1:]), bits(got[1:]))
    open_ = {**g, "x_mask": None}
    assert torch.equal(bits(guide(x, t)), bits(targets_reference(**open_, dtype=torch.float32)[0]))


# ---------------------------------------------------------------------------------------------------------------- the h3d form
@functools.lru_cache(maxsize=None)
def _h3d(case):
    """the case's inputs and its float64 / float32 restatements, computed once and shared (read-only)"""
    g = h3d_targets_case(case)
    return g, h3d_targets_reference(**g), h3d_targets_reference(**g, dtype=torch.float32)


@pytest.mark.parametrize("case", H3D_CASES, ids=h3d_case_id)
def test_h3d_targets_vs_float64(case):
    L = case[0]
    g, (want64, e64), (want32, e32) = _h3d(case)
    guide = _targets(g)
    x, kw = D(g["x"]), dict(x_mask=D(g["x_mask"]))
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    got, energy = guide(x, t, **kw), guide.energy(x, **kw)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (B,)
    _bound_row(f"h3d joint targets grad {h3d_case_id(case)}", got, want32, want64)
    _bound_row(f"h3d joint targets energy {h3d_case_id(case)}", energy, e32, e64)
    gc = got.cpu()
    assert torch.isfinite(gc).all() and not gc[..., 67:].any() and not gc[g["x_mask"]].any() and not gc[2].any() and energy[2].item() == 0.0
    guided = [c for j in g["joints"] if j for c in range(4 + 3 * (j - 1), 7 + 3 * (j - 1))] + ([3] if 0 in g["joints"] else [])
    assert not gc[..., [c for c in range(3, 67) if c not in guided]].any()          # joints that are not guided
    off = (g["weight"] == 0).all(-1)
    assert not gc[..., guided][off].any()                       # a frame without a target: no term in its own columns
    if L >= 2:                                                  # the adjoint reaches the rotation and root velocities of the first frame
        assert gc[0, 0, 0] != 0 and gc[0, 0, 1] != 0
    else:
        assert not gc[..., :3].any()
    # the same bits run to run; sample b alone
    assert torch.equal(bits(got), bits(guide(x, t, **kw))) and torch.equal(bits(energy), bits(guide.energy(x, **kw)))
    for b in range(B):
        alone = _targets(g, slice(b, b + 1))
        kwb = dict(x_mask=kw["x_mask"][b:b + 1])
        assert torch.equal(bits(alone(x[b:b + 1], t[:1], **kwb)), bits(got[b:b + 1]))
        assert torch.equal(bits(alone.energy(x[b:b + 1], **kwb)), bits(energy[b:b + 1]))
    part = _targets(g, t_start=500)(x, torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(bits(part[1:]), bits(got[1:]))


# ---------------------------------------------------------------------------------------------------------------- the sum
def _sum_case(form):
    """(contact, targets builders taking t_start, x, kw) on one motion: the contact fixtures of the existing kernel tests, targets on them"""
    if form == "h3d":
        c = h3d_contact_case((7, 130, 6, 263, "small", "per_sample"))
        joints = [0, 21, 5]                                     # another joint list than the contact term's
        mk_c = lambda **k: ContactGuidance.h3d(c["joints"], c["mean"], c["std"], to_scene=D(c["to_scene"]), sigma=SIGMA, scale=c["scale"], **k)
        mk_t = lambda tw, **k: JointTargets.h3d(joints, c["mean"], c["std"], to_scene=D(c["to_scene"]), scale=torch.tensor([0.3, 1.0, 2.0]), **tw, **k)
        K = len(joints)
    else:
        c = guide_case(130, 6, 66 if form == "pos66" else 263)
        cols = c["cols"][:2] + [3 if form == "pos66" else 150]          # two triples shared with the contact term, one of its own
        mk_c = lambda **k: ContactGuidance(c["cols"], c["mean"], c["std"], sigma=SIGMA, scale=c["scale"], **k)
        mk_t = lambda tw, **k: JointTargets(cols, c["mean"], c["std"], scale=torch.tensor([0.3, 1.0, 2.0]), **tw, **k)
        K = len(cols)
    L = c["x"].shape[1]
    tw = dict(target=1.5 * synth.gaussian(f"sum_{form}_g", (3, L, K, 3)), weight=(torch.rand((3, L, K), generator=torch.Generator().manual_seed(3)) < 0.7).float())
    kw = dict(c_pc_xyz=D(c["q"]), c_pc_contact=D(c["c"]), x_mask=D(c["x_mask"]))
    return mk_c, functools.partial(mk_t, tw), D(c["x"]), kw


@pytest.mark.parametrize("form", ["pos66", "pos263", "h3d"])
def test_the_sum_equals_the_terms_added_bit_for_bit(form):
    mk_c, mk_t, x, kw = _sum_case(form)
    t = torch.tensor([500, 499, 0], device=dev())
    for tc, tt in ((None, None), (500, None), (None, 500), (500, 300), (0, 0)):          # a late term contributes zeros
        contact, targets = mk_c(t_start=tc), mk_t(t_start=tt)
        both = MotionGuidance(contact, targets)
        a, b = contact(x, t, **kw), targets(x, t, **kw)
        got = both(x, t, **kw)
        assert torch.equal(bits(got), bits(a + b)), (form, tc, tt)
        assert torch.equal(bits(got), bits(both(x, t, **kw)))
        if tc == 500:
            assert not a[0].any() and torch.equal(got[0], b[0])
        if tt == 500:
            assert not b[0].any() and torch.equal(got[0], a[0])
        if tc is None and tt is None:
            assert a[1].abs().max() > 0 and b[1].abs().max() > 0 and not torch.equal(a, b)
        ec, et = both.energies(x, **kw)
        assert torch.equal(bits(ec), bits(contact.energy(x, **kw))) and torch.equal(bits(et), bits(targets.energy(x, **kw)))
    assert MotionGuidance(contact).energies(x, **kw)[1] is None and MotionGuidance(targets=targets).energies(x, **kw)[0] is None
    assert torch.equal(bits(MotionGuidance(mk_c())(x, t, **kw)), bits(mk_c()(x, t, **kw)))


# ---------------------------------------------------------------------------------------------------------------- native loops, exact
def _loop_targets(repr_, **kw):
    """targets for the loops' batch SHAPE3 on the model's 263 columns: three joints (h3d: the root among them), half of the frames"""
    K = 3
    target = 1.5 * synth.gaussian(f"targets_loop_{repr_}_g", (3, SHAPE3[1], K, 3))
    weight = (torch.rand((3, SHAPE3[1], K), generator=torch.Generator().manual_seed(21)) < 0.5).float() * 0.02
    target = torch.where((weight == 0)[..., None], torch.full((), float("nan")), target)
    kw.setdefault("scale", torch.tensor([1.0, 2.5, 0.5]))
    if repr_ == "h3d":
        c = _h3d_contact()
        kw.setdefault("to_scene", D(ZUP))
        return JointTargets.h3d([0, 21, 5], c.mean, c.std, target=target, weight=weight, **kw)
    c = _pos_contact()
    return JointTargets([SCATTERED[0], 150, SCATTERED[2]], c.mean, c.std, target=target, weight=weight, **kw)


def _loop_guide(repr_, terms, d, **kw):
    """targets alone (guided from executed step 1 on) or contact + targets (the contact term from step 2 on)"""
    targets = _loop_targets(repr_, t_start=d.timestep_map[3] + 1, **kw)
    if terms == "targets":
        return targets
    contact = (_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=d.timestep_map[2] + 1)
    return MotionGuidance(contact, targets)


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("how", ["unguided", "two scales"])
@pytest.mark.parametrize("terms", ["targets", "contact+targets"])
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
@pytest.mark.parametrize("form", list(FORMS))
def test_native_guided_loop_equals_the_step_by_step_loop(cmdm, form, repr_, terms, how, imputing):
    d, loop, progressive = _sampler(form)
    guide = _loop_guide(repr_, terms, d)
    assert guide.first_guided(d) == 1 and (terms == "targets" or guide.contact.first_guided(d) == 2)
    model = _model(cmdm, how)
    args = dict(clip_denoised=imputing, denoised_fn=_imp3() if imputing else None, cond_fn=guide, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        native = loop(model, SHAPE3, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": None}))
        if terms != "targets":                                  # both terms act
            assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": guide.contact}))
            assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": guide.targets}))
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
    contact0 = (_h3d_contact if repr_ == "h3d" else _pos_contact)(scale=0.0)
    for guide in (_loop_targets(repr_, scale=0.0), _loop_targets(repr_, t_start=0), _loop_targets(repr_, scale=torch.zeros(3)),
                  MotionGuidance(contact0, _loop_targets(repr_, scale=0.0))):
        assert torch.equal(loop(model, SHAPE3, cond_fn=guide, **args), plain)
        assert torch.equal(_last(progressive(model, SHAPE3, cond_fn=guide, **args)), plain)


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_targets_lower_the_energy_of_every_sample():
    """The inputs tests/test_joint_targets_host.py has shown to work in float64 (linear betas, ddim5, t_start = 601, scale = 0.1, weights
    in {0, 1}, B = 3, L = 16, K = 2) with the identity denoiser (pred_xstart = x_t: a DDIM eta = 0 step is the unguided chain's step plus
    one gradient-descent step on E at the point the step starts from).  The guided chain ends at a lower energy than the unguided one for
    every sample.  Two runs compared; no threshold."""
    g = effect_inputs()
    guide = JointTargets(g["cols"], g["mean"], g["std"], target=g["target"], weight=g["weight"], scale=0.1, t_start=g["t_start"])
    cfg = cmdm_cfg(steps=1000, respacing="ddim5")
    cfg.diffusion.noise_schedule = "linear"
    d = create_gaussian_diffusion(cfg)
    assert list(d.timestep_map) == [0, 200, 400, 600, 800] and guide.first_guided(d) == 1
    shape = tuple(g["start"].shape)
    identity = lambda x, t, **_: x
    args = dict(noise=D(g["start"]), clip_denoised=False, model_kwargs={}, eta=0.0, device=dev())
    plain, guided = d.ddim_sample_loop(identity, shape, **args), d.ddim_sample_loop(identity, shape, cond_fn=guide, **args)
    e_start, e_plain, e_guided = guide.energy(D(g["start"])), guide.energy(plain), guide.energy(guided)
    print(f"[joint targets effect] energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
    assert (e_guided < e_plain).all()


# ---------------------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("repr_", ["pos", "h3d"])
def test_guided_jobs_launch_no_eager_arithmetic_and_the_documented_launch_counts(cmdm, cdm, repr_):
    n = 6
    kw = _kw3()
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    dp = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=str(n)))
    kernels = lambda names: sum(c for k, c in names.items() if "guide_gather_kernel" in k or not _MOVERS.search(k))
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    assert not any(_MOVERS.search(k) for ks in TARGET_KERNELS.values() for k in ks)
    none = Impute(D(synth.gaussian("guide_known", SHAPE3)), torch.zeros(SHAPE3, dtype=torch.bool, device=dev()))
    sep = lambda fn: none if fn is None else None              # the loop of the same (separate-update) form without guidance
    runs = {"ddim": (lambda fn: dd.ddim_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), dd),
            "2m": (lambda fn: dd.dpm_solver_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), dd),
            "ddpm": (lambda fn: dp.p_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), dp)}
    per_step = len(TARGET_KERNELS[repr_])
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        for name, (run, d) in runs.items():
            # the targets from executed step 1 on (5 guided steps), the contact term from step 2 on (4)
            targets = _loop_targets(repr_, t_start=d.timestep_map[4] + 1)
            both = MotionGuidance((_h3d_contact if repr_ == "h3d" else _pos_contact)(t_start=d.timestep_map[3] + 1), targets)
            assert targets.first_guided(d) == 1 and both.contact.first_guided(d) == 2
            run(targets), run(both), run(None)                    # (weight pack, workspaces, rows and streams exist before anything is counted)
            torch.cuda.synchronize()
            with_t, with_b, without = (_device_kernel_names(lambda fn=fn: run(fn)) for fn in (targets, both, None))
            _check(with_t, f"target-guided native loop ({repr_}, {name})")
            _check(with_b, f"contact- and target-guided native loop ({repr_}, {name})")
            print(f"[joint targets launches] {repr_} {name}: kernels targets {kernels(with_t)}, contact + targets {kernels(with_b)}, without {kernels(without)}")
            assert count(with_t, "sampling_update_kernel") == count(with_b, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
            assert kernels(with_t) == kernels(without) + per_step * 5
            assert kernels(with_b) == kernels(without) + per_step * 5 + CONTACT_LAUNCHES[repr_] * 4
            if repr_ == "pos":
                assert count(with_t, "target_cols_kernel") == count(with_b, "target_cols_kernel") == 5
                assert count(with_b, "guide_nearest_kernel") == count(with_b, "guide_gather_kernel") == 4
            else:
                assert count(with_t, "target_h3d_kernel") == count(with_b, "target_h3d_kernel") == 5
                assert count(with_t, "h3d_recover_kernel") == 5 and count(with_b, "h3d_recover_kernel") == 5 + 4          # once per term
                assert count(with_t, "h3d_adjoint_kernel") == 5 and count(with_t, "h3d_adjoint_add_kernel") == 0
                # alone (step 1) the targets run the plain adjoint; behind the contact term the adding one
                assert count(with_b, "h3d_adjoint_add_kernel") == 4 and count(with_b, "h3d_adjoint_kernel") == 1 + 4
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # both stages, the motion stage guided by the first stage's own map and by targets
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    Bn, N, L = 2, 1024, 16
    args = dict(text_feat=D(synth.text_feature(Bn)), xyz=D(synth.scene_cloud(Bn, N, seed=14)), frames=L, sigma=SIGMA, seed=9, sampler="ddim")
    full = _loop_targets(repr_)
    t2 = (JointTargets.h3d(full.joints, full.mean, full.std, target=full.target[:Bn], weight=full.weight[:Bn], to_scene=D(ZUP), scale=2.0) if repr_ == "h3d"
          else JointTargets(full.cols, full.mean, full.std, target=full.target[:Bn], weight=full.weight[:Bn], scale=2.0))
    c2 = (_h3d_contact if repr_ == "h3d" else _pos_contact)(scale=2.0)
    two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, joint_targets=t2, **args)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, joint_targets=t2, **args))
    _check(names, "two_stage_sample(contact_guidance=..., joint_targets=...)")
    assert count(names, TARGET_KERNELS[repr_][-2 if repr_ == "h3d" else 0]) == n
    base = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, **args)
    only = two_stage_sample(cdm, d_adm, cmdm, dd, joint_targets=t2, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=c2, joint_targets=t2, **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"])
    assert not torch.equal(got["motion"], base["motion"]) and not torch.equal(got["motion"], only["motion"])
    kw2 = dict(c_text_feat=args["text_feat"], c_pc_xyz=args["xyz"], c_pc_contact=base["cond"], x_mask=torch.zeros(Bn, L, dtype=torch.bool, device=dev()))
    by_hand = dd.ddim_sample_loop(cmdm, (Bn, L, 263), clip_denoised=False, cond_fn=MotionGuidance(c2, t2), model_kwargs=kw2, seed=10)
    assert torch.equal(got["motion"], by_hand)


def test_a_bare_contact_guidance_keeps_its_entry(cmdm, monkeypatch):
    """ContactGuidance alone: afm_cmdm_guide_loop_range, never the sum's entry; anything with targets: the sum's entry alone"""
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
    run(_pos_contact())
    assert set(seen) == {"afm_cmdm_guide_loop_range"}
    seen.clear()
    a = run(_loop_targets("pos"))
    b = run(MotionGuidance(targets=_loop_targets("pos")))
    run(MotionGuidance(_pos_contact(), _loop_targets("pos")))
    assert set(seen) == {"afm_cmdm_motion_guide_loop_range"} and torch.equal(a, b)
    seen.clear()
    assert torch.equal(run(MotionGuidance(_pos_contact())), run(_pos_contact()))          # the sum of one contact term is that term
    assert seen == ["afm_cmdm_motion_guide_loop_range", "afm_cmdm_guide_loop_range"]


# ---------------------------------------------------------------------------------------------------------------- argument errors
class _MotionLoopProbe:
    """The loaded library with afm_cmdm_motion_guide_loop_range wrapped: in front of every real call, the same call with a description that
    must be refused - AFM_E_BADARG each, returned before anything is enqueued."""
    GUIDE = 15

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_motion_guide_loop_range":
            return fn

        def call(*args):
            real = args[self.GUIDE]._obj
            some = args[1]                                      # a valid device pointer, not the one the terms name
            keep = []

            def variant(change):
                m = ffi.MotionGuide.from_buffer_copy(real)
                t = ffi.JointTargets.from_buffer_copy(real.targets.contents)
                c = ffi.ContactGuide.from_buffer_copy(real.contact.contents) if real.contact else None
                lay = ffi.H3dLayout.from_buffer_copy(t.h3d.contents) if t.h3d else None
                change(m, t, c, lay)
                if lay is not None and t.h3d:
                    t.h3d = C.pointer(lay)
                if m.targets:
                    m.targets = C.pointer(t)
                if c is not None and m.contact:
                    m.contact = C.pointer(c)
                keep.append((m, t, c, lay))
                return m

            def neither(m, t, c, lay): m.contact, m.targets = None, None
            def k0(m, t, c, lay): t.K = 0
            def k17(m, t, c, lay): t.K = 17
            def no_gk(m, t, c, lay): m.gk = None
            def neg(m, t, c, lay): t.first_guided = -1
            def no_target(m, t, c, lay): t.target = None
            changes = [neither, k0, k17, no_gk, neg, no_target]
            if real.targets.contents.h3d:
                def out_of_range(m, t, c, lay): lay.joints[1] = 22
                def twice(m, t, c, lay): lay.joints[1] = lay.joints[0]
                def stride(m, t, c, lay): lay.to_scene_stride = 5
                changes += [out_of_range, twice, stride]
            else:
                def leaves(m, t, c, lay): t.cols[0] = 262
                def overlaps(m, t, c, lay): t.cols[1] = t.cols[0] + 2
                changes += [leaves, overlaps]
            if real.contact:
                def other_mean(m, t, c, lay): t.mean = some
                def other_std(m, t, c, lay): t.std = some
                def neg_c(m, t, c, lay): c.first_guided = -1
                changes += [other_mean, other_std, neg_c]
                if real.targets.contents.h3d:
                    def other_scene(m, t, c, lay): lay.to_scene = some
                    def other_form(m, t, c, lay): t.h3d = None
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
        for repr_, terms in (("pos", "targets"), ("h3d", "contact+targets"), ("pos", "contact+targets"), ("h3d", "targets")):
            guide = _loop_guide(repr_, terms, d)
            runs.append(lambda loop=loop, guide=guide: loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=_kw3(), seed=4))
    want = [run().clone() for run in runs]
    probe = _MotionLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == len(runs) and all(torch.equal(a, b) for a, b in zip(want, got))
    monkeypatch.undo()
    # afm_motion_guidance itself: D < 67 with h3d, an energy of a term that is not set, a workspace too small; nothing is enqueued
    lib = ffi.load()
    g = _h3d(H3D_CASES[2])[0]
    x = D(g["x"])
    L = x.shape[1]
    guide = MotionGuidance(targets=_targets(g))
    desc, fm, keep = guide.describe(x, dict(x_mask=D(g["x_mask"])))
    need = int(lib.afm_motion_guidance_workspace_bytes(C.byref(desc), B, L, 263))
    assert need > 0 and lib.afm_motion_guidance_workspace_bytes(C.byref(desc), B, L, 66) == -1 and lib.afm_motion_guidance_workspace_bytes(None, B, L, 263) == -1
    ws, grad, e = torch.empty(need, dtype=torch.uint8, device=dev()), torch.full_like(x, 7.0), torch.full((B,), 7.0, device=dev())
    call = lambda Dm, nbytes, ec=None: lib.afm_motion_guidance(C.byref(desc), x.data_ptr(), fm.data_ptr(), None, grad.data_ptr(), ec, e.data_ptr(), B, L, Dm,
                                                               ws.data_ptr(), nbytes, ffi.stream_of(x))
    assert call(66, need) == -1 and call(263, need, e.data_ptr()) == -1 and call(263, 64) == -2
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (e == 7.0).all()
    assert call(263, need) == 0
    t0 = torch.zeros(B, dtype=torch.int64, device=dev())
    assert torch.equal(grad, guide(x, t0, x_mask=D(g["x_mask"]))) and torch.equal(e, guide.energies(x, x_mask=D(g["x_mask"]))[1])


def test_zz_write_parity_table():
    """Not a check: stores the ratios measured so far (gpu_util.write_parity_table; committed as profiles/joint_targets_parity.json), with
    the rule `_bound_row` applied in place of the writer's general one."""
    import json
    path = write_parity_table()
    if path and any("joint targets" in r["name"] for r in PARITY_ROWS):
        table = json.load(open(path))
        table["rule"] = ("rows named '... joint targets ...': max|hip - f64| <= 4 * max|f32 torch - f64| + 4 * 2^-23 max|f64| (max norm only, no "
                         "rms); ratio_max = e_hip / (e_ref + floor / 4), floor = 4 * 2^-23 max|f64|")
        json.dump(table, open(path, "w"), indent=1)
