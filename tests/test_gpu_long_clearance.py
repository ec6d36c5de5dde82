"""`-m gpu`: scene clearance of stitched long motions (afm.diffusion.LongGuidance(stitch, contact, targets, clearance);
ops.long_scene_guidance; afm_cmdm_long_scene_guide_loop_range; afm.pipeline.long_motion_sample(clearance=)).

Against float64: the gradient and `clearance_energy` of every fixture of tests/test_long_clearance_host.py, bounded by the project's rule
for these kernels (`_bound_row`: 4 x the float32-torch error of the same expressions plus 4 ulp of the largest entry).  Bit for bit: the two
copies of a shared frame, the zeros, run to run, a long motion alone against the batch, one window against `SceneClearance`, the sum
against the terms added, the native loop against the step-by-step loop after every step, chained range calls against one call, zero scale
against the unguided stitched chain."""
import pytest
import torch

from afm import synth
from afm.base import create_gaussian_diffusion, create_model
from afm.diffusion import ContactGuidance, JointTargets, LongGuidance, SceneClearance, Stitch
from afm.pipeline import long_motion_sample
from gpu_util import dev, load_named_weights
from test_clearance_host import EFFECT_RADIUS, EFFECT_SCALE, effect_scene
from test_gpu_cdm import cdm_cfg
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import _bound_row
from test_gpu_long_guidance import _impute, _loops
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_gpu_stitch import cmdm, conds, d5, guided_model, shared_frames_agree          # noqa: F401 (fixtures)
from test_guidance_host import JOINTS, SCATTERED, SIGMA
from test_long_clearance_host import (CASES, case_id, clearance_of, guidance_of, long_clear_case, long_clearance_reference, ref_args,
                                      window_sums)
from test_long_guidance_host import L, S, long_case, long_positions, windows_holding
from test_long_guidance_host import guidance_of as terms_of

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())
bits = lambda t: t.contiguous().view(torch.int32)
N = 1024
# the gradient launches of one guided step: join + windows, the contact term's 2 (h3d: 4), the targets' 1 (h3d: 3) and the
# clearance's 2 - the long pass and the join of the windows' sums - (h3d: 4 - recovery, long pass, join, adjoint)
LAUNCHES = {("cols", "clearance"): 4, ("h3d", "clearance"): 6, ("cols", "all three"): 7, ("h3d", "all three"): 13}
CLEAR_KERNELS = ("long_clear_kernel", "long_clear_join_kernel")
LONG_KERNELS = ("long_", "stitch_join_kernel", "stitch_windows_kernel", "h3d_recover_kernel", "h3d_adjoint", "target_")


def _kw(g):
    kw = dict(c_pc_xyz=D(g["q"]))
    if "exempt_contact" in g["options"]:
        kw["c_pc_contact"] = D(g["c"])
    return kw


def _alone(g, i):
    """long motion i of a case as a case of its own"""
    one = dict(g, options=dict(g["options"]))
    for k in ("x", "q", "c"):
        one[k] = g[k][i * S:(i + 1) * S]
    if "weight" in one["options"]:
        one["options"]["weight"] = g["options"]["weight"][i * S:(i + 1) * S]
    for k in ("scale", "to_scene"):
        one[k] = None if g[k] is None else g[k][i:i + 1]
    return one


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_long_clearance_kernels_vs_float64(case):
    form, ov, tail, Np, K, G = case
    g = long_clear_case(case)
    st, x, kw = g["st"], D(g["x"]), _kw(g)
    B, F = G * S, st.frames
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    guide = guidance_of(g, D)
    got, e = guide(x, t, **kw), guide.clearance_energy(x, **kw)
    want64, e64 = long_clearance_reference(**ref_args(g))
    want32, e32 = long_clearance_reference(**ref_args(g), dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == x.shape and e.shape == (G,) and guide.energies(x, **kw) == (None, None)
    _bound_row(f"long clearance grad {case_id(case)}", got, want32, want64)
    _bound_row(f"long clearance energy {case_id(case)}", e, e32, e64)
    # exact: the two copies of every shared frame, the padded tail, the columns the term does not name
    gc = got.cpu()
    named = torch.zeros(x.shape[2], dtype=torch.bool)
    if form == "h3d":
        named[:67] = True
    else:
        for col in g["cols"]:
            named[col:col + 3] = True
    assert shared_frames_agree(st, got) and gc.abs().max() > 0 and (e > 0).all()
    assert tail == 0 or not gc.view(G, S, L, -1)[:, -1, L - tail:].any()
    assert not gc[..., ~named].any()
    # a joint-frame with no obstacle point inside its radius in any window that holds it (float64, by a margin): exactly zero in the
    # columns that are its own (the position triple; h3d: the local triple of a joint other than the root)
    a = ref_args(g)
    P = long_positions(st.join(g["x"]), g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float64)
    opts = {k: a[k] for k in ("weight", "up", "min_height", "c", "exempt_contact") if k in a}
    far = [r * 1.001 for r in g["radius"]]                    # (no point within 1.001 r: none within r in float32 either)
    hit = window_sums(P, st, g["q"], far, torch.float64, **opts)[2].view(G, S, L, K)
    glong, alone = st.join(got).cpu(), 0
    for f in range(F):
        ws = windows_holding(f, S, L, ov)
        for k in range(K):
            own = None if form != "h3d" else (None if g["joints"][k] == 0 else 4 + 3 * (g["joints"][k] - 1))
            own = g["cols"][k] if form != "h3d" else own
            for gi in range(G):
                if own is not None and not any(hit[gi, w, f - w * (L - ov), k] for w in ws):
                    alone += 1
                    assert not glong[gi, f, own:own + 3].any(), (gi, f, k)
    assert alone > 0 or (form == "h3d" and all(j == 0 for j in g["joints"]))          # (the root has no triple of its own)
    # the same bits run to run; a long motion alone is the same motion inside the batch
    assert torch.equal(bits(got), bits(guide(x, t, **kw))) and torch.equal(bits(e), bits(guide.clearance_energy(x, **kw)))
    for i in range(G if G > 1 else 0):
        one = _alone(g, i)
        solo = guidance_of(one, D)
        assert torch.equal(bits(solo(D(one["x"]), t[:S], **_kw(one))), bits(got[i * S:(i + 1) * S])), i
        assert torch.equal(bits(solo.clearance_energy(D(one["x"]), **_kw(one))), bits(e[i:i + 1])), i
    # t_start per long motion: one whose first window's t is at or above it gets zeros, the others what they got
    late = guidance_of(g, D, t_start=10)
    tt = t.clone()
    tt[0] = 10                                                # long motion 0 (t of its other windows is not read)
    tt[1:S] = 0
    part = late(x, tt, **kw)
    assert not part[:S].any() and torch.equal(bits(part[S:]), bits(got[S:]))
    tt[0], tt[1:S] = 0, 10
    assert torch.equal(bits(late(x, tt, **kw)), bits(got))


@pytest.mark.parametrize("form", ["cols", "h3d"])
def test_one_window_is_scene_clearance(form):
    """Stitch(1, 0, L) against `SceneClearance` on the same x: the same bits, gradient and energy"""
    g = long_clear_case((form, 3, 2, 130, 6, 2))
    long = D(g["st"].join(g["x"]))
    one = Stitch(1, 0, length=long.shape[1])
    g1 = dict(g, options=dict(g["options"], weight=g["options"]["weight"][::S].contiguous()))
    clr = clearance_of(g1, D)
    kw = dict(c_pc_xyz=D(g["q"][::S].contiguous()), c_pc_contact=D(g["c"][::S].contiguous()))
    for t in (torch.zeros(2, dtype=torch.int64, device=dev()), torch.tensor([10, 9], device=dev())):
        for ts in (None, 10):
            clr.t_start = ts
            lg = LongGuidance(one, clearance=clr)
            got, want = lg(long, t, **kw), clr(long, t, **kw)
            assert torch.equal(bits(got), bits(want)) and want.abs().max() > 0
    assert torch.equal(bits(lg.clearance_energy(long, **kw)), bits(clr.energy(long, **kw)))


def _sum_clearance(g, form, **kw):
    """a clearance on the motion of `long_case` (tests/test_long_guidance_host.py): joints of its own, an exemption by each window's map"""
    kw = dict(radius=[0.9, 1.2, 0.7], scale=torch.tensor([2.0, 0.4]), exempt_contact=0.9, **kw)
    if form == "h3d":
        return SceneClearance.h3d([0, 12, 7], g["mean"], g["std"], **kw)
    return SceneClearance(g["cols"][1:3] + [0], g["mean"], g["std"], **kw)


@pytest.mark.parametrize("form", ["cols", "h3d"])
def test_the_sum_equals_the_terms_added_bit_for_bit(form):
    g = long_case((form, 3, 2, 130, 6, 2))
    st, x = g["st"], D(g["x"])
    kw = dict(c_pc_xyz=D(g["q"]), c_pc_contact=D(g["c"]))
    t = torch.tensor([500] * S + [499] * S, device=dev())
    for tc, tt, ts in ((None, None, None), (500, None, None), (None, 500, 300), (None, None, 500), (500, 300, 500), (0, 0, 0)):
        two = terms_of(g, True, True, D)
        two.contact.t_start, two.targets.t_start = tc, tt
        clr = _sum_clearance(g, form, t_start=ts, **({"to_scene": two.contact.to_scene} if form == "h3d" else {}))
        three = LongGuidance(st, two.contact, two.targets, clr)
        a, c = two(x, t, **kw), LongGuidance(st, clearance=clr)(x, t, **kw)
        got = three(x, t, **kw)
        assert torch.equal(bits(got), bits(a + c)), (form, tc, tt, ts)
        assert torch.equal(bits(got), bits(three(x, t, **kw))) and shared_frames_agree(st, got)
        ca, ta = LongGuidance(st, two.contact)(x, t, **kw), LongGuidance(st, None, two.targets)(x, t, **kw)
        assert torch.equal(bits(LongGuidance(st, two.contact, None, clr)(x, t, **kw)), bits(ca + c))
        assert torch.equal(bits(LongGuidance(st, None, two.targets, clr)(x, t, **kw)), bits(ta + c))
        if ts == 500:
            assert not c[:S].any() and torch.equal(got[:S], a[:S])          # (values: adding the zeros turns a -0 into +0)
        if tc is None and tt is None and ts is None:
            assert a[S:].abs().max() > 0 and c[:S].abs().max() > 0 and c[S:].abs().max() > 0
        ec, et = three.energies(x, **kw)
        e2 = two.energies(x, **kw)
        assert torch.equal(bits(ec), bits(e2[0])) and torch.equal(bits(et), bits(e2[1]))
        assert torch.equal(bits(three.clearance_energy(x, **kw)), bits(LongGuidance(st, clearance=clr).clearance_energy(x, **kw)))
        assert three.t_start == (None if None in (tc, tt, ts) else max(tc, tt, ts))


# ---------------------------------------------------------------------------------------------------------------- the loops, exact
def loop_clearance(G, form, **kw):
    """a clearance for the loops on the CMDM's 263 columns, against each window's own cloud of `conds`: three joints, a scale per long motion,
    the exemption by each window's own map"""
    mean, std = 0.3 * synth.gaussian("long_loop_mean", (263,)), 0.5 + synth.gaussian("long_loop_std", (263,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    kw.setdefault("scale", torch.tensor([0.5, 1.0, 0.25, 0.75])[:G])
    kw.setdefault("radius", [1.0, 0.8, 1.2])
    kw.setdefault("exempt_contact", 0.9)
    if form == "h3d":
        return SceneClearance.h3d([0, 20, 5], mean, std, **kw)
    return SceneClearance([SCATTERED[1] - 3, 150, SCATTERED[3]], mean, std, **kw)


def loop_guide(st, G, form, terms, d=None, **kw):
    """the clearance alone, or contact + targets + clearance.  ``d``: the clearance guides from executed step 1 on, the contact term from
    step 3, the targets from step 2; else ``t_start`` (if given) is every term's"""
    every = {"t_start": kw.pop("t_start")} if "t_start" in kw else {}
    start = lambda j: every if d is None else dict(t_start=d.timestep_map[len(d.timestep_map) - 1 - j] + 1)
    F = st.check(G * st.windows, st.length)
    if form == "h3d":
        kw["to_scene"] = D(torch.eye(3, 4).repeat(G, 1, 1) + 0.2 * synth.gaussian("long_loop_to_scene", (G, 3, 4)))
    clear = loop_clearance(G, form, **start(1), **kw)
    if terms == "clearance":
        return LongGuidance(st, clearance=clear)
    target = 0.5 * synth.gaussian("long_loop_target", (G, F, 2, 3))
    weight = (synth.gaussian("long_loop_weight", (G, F, 2)) > 0.0).float()
    cs, tsc = torch.tensor([1.0, 2.5, 0.5, 1.5])[:G], torch.tensor([0.5, 0.25, 1.0, 0.125])[:G]
    if form == "h3d":
        ct = ContactGuidance.h3d(JOINTS, clear.mean, clear.std, to_scene=clear.to_scene, sigma=SIGMA, scale=cs, **start(3))
        tg = JointTargets.h3d([0, 20], clear.mean, clear.std, target=target, weight=weight, to_scene=clear.to_scene, scale=tsc, **start(2))
    else:
        ct = ContactGuidance(SCATTERED, clear.mean, clear.std, sigma=SIGMA, scale=cs, **start(3))
        tg = JointTargets(SCATTERED[:2], clear.mean, clear.std, target=target, weight=weight, scale=tsc, **start(2))
    return LongGuidance(st, ct, tg, clear)


LOOP_ST = Stitch(S, 3, S * L - 2 * 3 - 2, length=L)          # G = 2, S = 3, L = 8, ov = 3, a padded tail of two frames
LOOP_SHAPE = (2 * S, L, 263)


@pytest.mark.parametrize("terms", ["clearance", "all three"])
@pytest.mark.parametrize("form", ["pos", "h3d"])
@pytest.mark.parametrize("sampler,guided", [("ddim", "two"), ("ddim", "plain"), ("dpm", "one"), ("dpm", "plain")])
def test_native_loop_equals_the_step_by_step_loop(cmdm, d5, sampler, guided, form, terms):
    st, shape = LOOP_ST, LOOP_SHAPE
    B = shape[0]
    model, kw = guided_model(cmdm, guided, B), conds(B, L, st)
    loop, progressive = _loops(d5, sampler)
    n = d5.num_timesteps
    guide = loop_guide(st, 2, form, terms, d5)
    assert guide.first_guided(d5) == 1 and (terms == "clearance" or (guide.contact.first_guided(d5), guide.targets.first_guided(d5)) == (3, 2))
    for fn in (None, _impute(st, shape)):
        args = dict(clip_denoised=fn is not None, denoised_fn=fn, cond_fn=guide, model_kwargs=kw, seed=21, stitch=st)
        snaps = {j: None for j in range(1, n)}
        native = loop(model, shape, snapshots=snaps, **args)          # (range calls cut at every step, on one workspace)
        steps = [o["sample"].clone() for o in progressive(model, shape, **args)]
        assert len(steps) == n and torch.isfinite(native).all()
        for j in range(1, n):
            assert torch.equal(snaps[j], steps[j - 1]), (sampler, guided, form, terms, fn is not None, j)
            assert shared_frames_agree(st, snaps[j]), (sampler, guided, form, j)
        assert torch.equal(native, steps[-1]) and shared_frames_agree(st, native), (sampler, guided, form, fn is not None)
        assert torch.equal(native, loop(model, shape, **args))          # one call
        cut = {2: None}                                                 # a chain split into two range calls
        assert torch.equal(native, loop(model, shape, snapshots=cut, **args)) and cut[2] is not None and torch.equal(cut[2], snaps[2])
        assert not torch.equal(native, loop(model, shape, **{**args, "cond_fn": None}))          # the guidance acts
        if terms != "clearance":                                        # the clearance acts next to the other two
            assert not torch.equal(native, loop(model, shape, **{**args, "cond_fn": LongGuidance(st, guide.contact, guide.targets)}))


def test_two_streams_equal_one(cmdm, d5):
    G, st = 4, Stitch(S, 3, length=L)
    shape, kw = (G * S, L, 263), conds(G * S, L, st)
    guide = loop_guide(st, G, "h3d", "all three")
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    try:
        for sampler in ("ddim", "dpm"):
            loop = _loops(d5, sampler)[0]
            cmdm.loop_streams, cmdm.loop_streams_auto = 1, False
            one = loop(cmdm, shape, clip_denoised=False, cond_fn=guide, model_kwargs=kw, seed=8, stitch=st).clone()
            cmdm.loop_streams, cmdm.loop_streams_auto = 2, False          # sub-batches of two long motions each
            two = loop(cmdm, shape, clip_denoised=False, cond_fn=guide, model_kwargs=kw, seed=8, stitch=st).clone()
            assert torch.equal(one, two) and shared_frames_agree(st, two), sampler
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved


@pytest.mark.parametrize("form", ["pos", "h3d"])
def test_a_late_start_launches_no_clearance_kernel_before_it(cmdm, d5, form):
    """The launches of a guided step are DESIGN.md's; steps in front of the clearance's first_guided launch none of its kernels (and, alone,
    exactly the unguided stitched loop's); no ATen arithmetic kernel anywhere."""
    st, shape = LOOP_ST, LOOP_SHAPE
    kw = conds(shape[0], L, st)
    n = d5.num_timesteps
    t_mid = d5.timestep_map[2] + 1                            # the two first executed steps run unguided, the last three guided
    ours = lambda names: {k: c for k, c in names.items() if not _MOVERS.search(k) or any(p in k for p in LONG_KERNELS)}          # (not ATen's movers)
    kernels = lambda names: sum(ours(names).values())
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        for sampler in ("ddim", "dpm"):
            loop = _loops(d5, sampler)[0]
            run = lambda fn: loop(cmdm, shape, clip_denoised=False, cond_fn=fn, model_kwargs=kw, seed=5, stitch=st)
            for terms in ("clearance", "all three"):
                guide = loop_guide(st, 2, form, terms, t_start=t_mid)          # every term from executed step 2 on
                assert guide.first_guided(d5) == 2
                run(guide), run(None)
                torch.cuda.synchronize()
                with_, without = _device_kernel_names(lambda: run(guide)), _device_kernel_names(lambda: run(None))
                _check(with_, f"long-scene-guided stitched native loop ({sampler}, {form}, {terms})")
                per_step = LAUNCHES[("cols" if form == "pos" else "h3d", terms)]
                print(f"[long clearance launches] {sampler} {form} {terms}: kernels guided {kernels(with_)}, unguided {kernels(without)}, "
                      f"{per_step} a guided step")
                for k, cnt in ours(without).items():
                    assert with_.get(k, 0) == cnt + (3 if "stitch_windows_kernel" in k else 0), (k, sampler, form, terms)
                new = set(ours(with_)) - set(ours(without))
                assert new and all(any(p in k for p in LONG_KERNELS) for k in new), new
                assert kernels(with_) == kernels(without) + per_step * 3
                assert count(with_, "stitch_join_kernel") == 3 and count(with_, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
                assert all(count(with_, k) == 3 for k in CLEAR_KERNELS) and not any(count(without, k) for k in CLEAR_KERNELS)
                assert not any("clear_kernel" in k and "long_clear" not in k for k in with_)          # (the single-window kernel is not the long one)
            # the clearance starts later than the other two: in front of it a step launches what `LongGuidance(st, contact, targets)` launches
            full = loop_guide(st, 2, form, "all three")
            full.clearance.t_start = d5.timestep_map[1] + 1   # from executed step 3 on: two guided steps
            front = LongGuidance(st, full.contact, full.targets)
            run(full), run(front)
            torch.cuda.synchronize()
            with_, without = _device_kernel_names(lambda: run(full)), _device_kernel_names(lambda: run(front))
            per_clear = 2 if form == "pos" else 4
            assert all(count(with_, k) == 2 for k in CLEAR_KERNELS) and kernels(with_) == kernels(without) + per_clear * 2
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved


@pytest.mark.parametrize("sampler,guided", [("ddim", "two"), ("dpm", "plain")])
def test_zero_scale_and_a_start_at_zero_reproduce_the_unguided_stitched_chain(cmdm, d5, sampler, guided):
    st, shape = LOOP_ST, LOOP_SHAPE
    model, kw = guided_model(cmdm, guided, shape[0]), conds(shape[0], L, st)
    loop, progressive = _loops(d5, sampler)
    args = dict(clip_denoised=False, model_kwargs=kw, seed=4, stitch=st)
    plain = loop(model, shape, **args)
    for form in ("pos", "h3d"):
        for guide in (loop_guide(st, 2, form, "clearance", scale=0.0), loop_guide(st, 2, form, "clearance", t_start=0),
                      loop_guide(st, 2, form, "clearance", scale=torch.zeros(2))):
            assert torch.equal(loop(model, shape, cond_fn=guide, **args), plain), (form,)
            steps = [o["sample"] for o in progressive(model, shape, cond_fn=guide, **args)]
            assert torch.equal(steps[-1], plain), (form,)


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_clearance_lowers_the_energy_of_every_long_motion_that_has_one():
    """The effect scene of tests/test_clearance_host.py, its start motion cut into stitched windows and its cloud repeated per window,
    with the identity denoiser (a DDIM eta = 0 step is the unguided chain's step plus one gradient-descent step on E): the guided chain
    ends at a lower clearance energy than the unguided one for every long motion whose unguided energy is > 0.  Two runs compared; no threshold."""
    g = effect_scene()
    G, F, _ = g["start"].shape                                # 3 long motions of 16 frames: S = 3 windows of 8 sharing 4
    st = Stitch(3, 4, F)
    assert st.length == 8
    guide = LongGuidance(st, clearance=SceneClearance(g["cols"], g["mean"], g["std"], radius=EFFECT_RADIUS, scale=EFFECT_SCALE, t_start=g["t_start"]))
    cfg = cmdm_cfg(steps=1000, respacing="ddim5")
    cfg.diffusion.noise_schedule = "linear"
    d = create_gaussian_diffusion(cfg)
    assert list(d.timestep_map) == [0, 200, 400, 600, 800] and guide.first_guided(d) == 1
    start = D(st.windows_of(g["start"]))
    identity = lambda x, t, **_: x
    kw = dict(c_pc_xyz=D(g["q"].repeat_interleave(3, 0)))
    args = dict(noise=start, clip_denoised=False, model_kwargs=kw, eta=0.0, device=dev(), stitch=st)
    plain, guided = d.ddim_sample_loop(identity, tuple(start.shape), **args), d.ddim_sample_loop(identity, tuple(start.shape), cond_fn=guide, **args)
    e_start, e_plain, e_guided = (guide.clearance_energy(v, **kw) for v in (start, plain, guided))
    print(f"[long clearance effect] energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
    has = e_plain > 0
    assert shared_frames_agree(st, guided) and has[:2].all() and (e_guided[has] < e_plain[has]).all() and (e_guided[~has] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- two stages
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


@pytest.mark.parametrize("form", ["pos", "h3d"])
@pytest.mark.parametrize("sampler", ["dpm++", "ddim"])
def test_long_motion_sample_takes_a_clearance(cmdm, cdm, sampler, form):
    """long_motion_sample(clearance=...) on both samplers and both forms: finite, shared frames agree, the term's two kernels run at every
    guided step and nothing eager does, the group's cloud is cleared per window (a weight row per window, the exemption by the stage's own
    cond), shapes that do not fit are refused.  (The effect on the effect scene - D = 66, 96 points: no input of these models - is the
    identity-denoiser chain above, as tests/test_gpu_clearance.py has it for the single window.)"""
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    G, F, ov = 2, 35, 4                                       # L = 15, a padded tail of 2 frames in the last window
    text, xyz = D(synth.text_feature(G * S)).view(G, S, -1), D(synth.scene_cloud(G, N, seed=14))
    st = Stitch(S, ov, F)
    gen = torch.Generator().manual_seed(3)
    weight = 0.25 + 1.75 * torch.rand((G * S, N), generator=gen)
    weight[torch.rand((G * S, N), generator=gen) < 0.25] = 0.0
    mean, std = 0.3 * synth.gaussian("long_loop_mean", (263,)), 0.5 + synth.gaussian("long_loop_std", (263,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    mk = lambda **kw: SceneClearance.h3d([0, 20, 5], mean, std, radius=EFFECT_RADIUS, **kw) if form == "h3d" else \
        SceneClearance([SCATTERED[1] - 3, 150, SCATTERED[3]], mean, std, radius=EFFECT_RADIUS, **kw)
    run = lambda **kw: long_motion_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=F, overlap=ov, seed=9, sampler=sampler, **kw)
    clear = mk(weight=weight, scale=torch.tensor([EFFECT_SCALE, 2 * EFFECT_SCALE]), exempt_contact=0.5, t_start=d_amdm.timestep_map[-2] + 1)
    plain, out = run(), run(clearance=clear)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: run(clearance=clear))
    _check(names, f"long_motion_sample(clearance=) ({sampler}, {form})")
    guided_steps = d_amdm.num_timesteps - clear.first_guided(d_amdm)
    assert guided_steps == d_amdm.num_timesteps - 1
    assert all(sum(c for k, c in names.items() if part in k) == guided_steps for part in CLEAR_KERNELS)
    assert out["motion"].shape == (G, F, 263) and out["windows"].shape == (G * S, st.length, 263) and torch.isfinite(out["motion"]).all()
    assert shared_frames_agree(st, out["windows"]) and torch.equal(out["motion"], st.join(out["windows"]))
    assert torch.equal(plain["contact"], out["contact"]) and not torch.equal(plain["motion"], out["motion"])
    # the exemption reads the stage's own cond per window: without it the push is another one
    other = run(clearance=mk(weight=weight, scale=torch.tensor([EFFECT_SCALE, 2 * EFFECT_SCALE]), t_start=d_amdm.timestep_map[-2] + 1))
    assert torch.isfinite(other["motion"]).all() and not torch.equal(other["motion"], out["motion"])
    # next to the other terms
    ct = ContactGuidance.h3d(JOINTS, mean, std, sigma=SIGMA) if form == "h3d" else ContactGuidance(SCATTERED, mean, std, sigma=SIGMA)
    both = run(contact_guidance=ct, clearance=clear)
    assert torch.isfinite(both["motion"]).all() and shared_frames_agree(st, both["windows"]) and not torch.equal(both["motion"], out["motion"])
    with pytest.raises(ValueError, match="weight is per window"):
        run(clearance=mk(weight=weight[:G]))
    with pytest.raises(ValueError, match="6 values for 2 long motions"):
        run(clearance=mk(scale=torch.ones(G * S)))
