"""`-m gpu`: guidance of stitched long motions (afm.diffusion.LongGuidance; ops.long_guidance / stitch_guide_step; afm_cmdm_long_guide_loop_range;
afm.pipeline.long_motion_sample(contact_guidance=, joint_targets=)).

Against float64: the gradient and both energies of every fixture of tests/test_long_guidance_host.py, bounded by the project's rule for
these kernels (4 x the float32-torch error of the same expressions plus 4 ulp of the largest entry).  Bit for bit: the two copies of a
shared frame, the zeros, run to run, a long motion alone against the batch, the targets against `JointTargets` on the joined motion, one
window against `MotionGuidance`, the one-launch update against the chain of separate launches, the native loop against the step-by-step
loop after every step, chained range calls against one call, zero scale against the unguided stitched chain."""
import pytest
import torch

from afm import ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.diffusion import ContactGuidance, JointTargets, LongGuidance, MotionGuidance, Stitch
from afm.pipeline import long_motion_sample
from gpu_util import dev, load_named_weights
from test_gpu_cdm import cdm_cfg
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import _bound_row
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_gpu_stitch import cmdm, conds, d5, guided_model, shared_frames_agree          # noqa: F401 (fixtures)
from test_guidance_host import JOINTS, SCATTERED, SIGMA, contact_terms
from test_long_guidance_host import (CASES, DUP, L, S, case_id, guidance_of, long_case, long_guidance_reference, long_positions, ref_args,
                                     window_positions, windows_holding)

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())
N = 1024
# the gradient launches of one guided step: join + the contact term's 2 (h3d: 4) + the targets' 1 (h3d: 3) + windows
LAUNCHES = {("cols", "contact"): 4, ("cols", "targets"): 3, ("cols", "both"): 5, ("h3d", "contact"): 6, ("h3d", "targets"): 5, ("h3d", "both"): 9}
LONG_KERNELS = ("long_", "stitch_join_kernel", "stitch_windows_kernel", "h3d_recover_kernel", "h3d_adjoint", "target_")


def _kw(g):
    return dict(c_pc_xyz=D(g["q"]), c_pc_contact=D(g["c"]))


def _alone(g, i):
    """long motion i of a case as a case of its own"""
    one = dict(g)
    for k in ("x", "q", "c"):
        one[k] = g[k][i * S:(i + 1) * S]
    for k in ("scale", "tscale", "target", "weight", "to_scene"):
        one[k] = None if g[k] is None else g[k][i:i + 1]
    return one


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_long_guidance_kernels_vs_float64(case):
    form, ov, tail, Np, K, G = case
    g = long_case(case)
    st, x, kw = g["st"], D(g["x"]), _kw(g)
    B, F = G * S, st.frames
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    named = torch.zeros(x.shape[2], dtype=torch.bool)
    if form == "h3d":
        named[:67] = True
    else:
        for col in g["cols"]:
            named[col:col + 3] = True
    for terms in ("both", "contact", "targets"):
        ct, tg = terms != "targets", terms != "contact"
        guide = guidance_of(g, ct, tg, D)
        got, (ec, et) = guide(x, t, **kw), guide.energies(x, **kw)
        want64, ec64, et64 = long_guidance_reference(**ref_args(g, ct, tg))
        want32, ec32, et32 = long_guidance_reference(**ref_args(g, ct, tg), dtype=torch.float32)
        assert got.dtype == torch.float32 and got.shape == x.shape and (ec is None) == (not ct) and (et is None) == (not tg)
        _bound_row(f"long guidance {terms} grad {case_id(case)}", got, want32, want64)
        if ct:
            assert ec.shape == (G,)
            _bound_row(f"long guidance {terms} E_contact {case_id(case)}", ec, ec32, ec64)
        if tg:
            assert et.shape == (G,)
            _bound_row(f"long guidance {terms} E_targets {case_id(case)}", et, et32, et64)
        # exact: the two copies of every shared frame, the padded tail, the columns no term names
        gc = got.cpu()
        assert shared_frames_agree(st, got) and gc.abs().max() > 0
        assert tail == 0 or not gc.view(G, S, L, -1)[:, -1, L - tail:].any()
        assert not gc[..., ~named].any()
        if terms == "contact":                                # the duplicate pose: the first long frame won, in both windows
            for w in windows_holding(DUP[2], S, L, ov):
                row = gc[w, DUP[2] - w * (L - ov)]
                assert not (row[3:] if form == "h3d" else row).any(), (terms, w)
        # the same bits run to run; a long motion alone is the same motion inside the batch
        again, (ec2, et2) = guide(x, t, **kw), guide.energies(x, **kw)
        assert torch.equal(got, again) and (not ct or torch.equal(ec, ec2)) and (not tg or torch.equal(et, et2))
        for i in range(G if G > 1 else 0):
            one = _alone(g, i)
            alone = guidance_of(one, ct, tg, D)
            assert torch.equal(alone(D(one["x"]), t[:S], **_kw(one)), got[i * S:(i + 1) * S]), (terms, i)
            e1 = alone.energies(D(one["x"]), **_kw(one))
            assert (not ct or torch.equal(e1[0], ec[i:i + 1])) and (not tg or torch.equal(e1[1], et[i:i + 1])), (terms, i)
    # t_start: a long motion whose first window's t is at or above it gets zeros from that term, the others what they got
    guide = guidance_of(g, True, False, D)
    late = guidance_of(g, True, False, D)
    late.contact.t_start = 10
    tt = t.clone()
    tt[0] = 10                                                # long motion 0 (t of its other windows is not read)
    tt[1:S] = 0
    got, base = late(x, tt, **kw), guide(x, t, **kw)
    assert not got[:S].any() and torch.equal(got[S:], base[S:])


@pytest.mark.parametrize("form", ["cols", "h3d"])
def test_targets_are_the_targets_of_the_joined_motion_and_one_window_is_motion_guidance(form):
    g = long_case((form, 3, 2, 130, 6, 2))
    st, x, kw = g["st"], D(g["x"]), _kw(g)
    G = 2
    t = torch.zeros(G * S, dtype=torch.int64, device=dev())
    lg = guidance_of(g, False, True, D)
    long = st.join(x)
    want = st.windows_of(lg.targets(long, t[:G]), L)
    assert torch.equal(lg(x, t, **kw), want) and torch.equal(lg.energies(x, **kw)[1], lg.targets.energy(long))
    # S = 1: the long motion as its one window, each with its first window's map
    one = Stitch(1, 0, length=st.frames)
    kw1 = dict(c_pc_xyz=kw["c_pc_xyz"][::S].contiguous(), c_pc_contact=kw["c_pc_contact"][::S].contiguous())
    both = guidance_of(g, True, True, D)
    single, plain = LongGuidance(one, both.contact, both.targets), MotionGuidance(both.contact, both.targets)
    assert torch.equal(single(long, t[:G], **kw1), plain(long, t[:G], **kw1))
    e1, e2 = single.energies(long, **kw1), plain.energies(long, **kw1)
    assert torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1])


def test_a_target_in_the_last_window_moves_the_root_of_the_first():
    """The root carry: on h3d a target that only the last window holds reaches the root velocities of frame 0 of window 0 - which no
    per-window `JointTargets` on the same windows can do."""
    g = long_case(("h3d", 3, 0, 130, 6, 2))
    st, x = g["st"], D(g["x"])
    G, F = 2, st.frames
    weight = torch.zeros(G, F, 6)
    weight[:, F - 2, 0] = 1.0                                 # the root, at a frame of the last window alone
    assert windows_holding(F - 2, S, L, st.overlap) == [S - 1]
    target = torch.nan_to_num(g["target"], nan=0.0)
    ts = D(g["to_scene"])
    t = torch.zeros(G * S, dtype=torch.int64, device=dev())
    lg = LongGuidance(st, None, JointTargets.h3d(g["joints"], g["mean"], g["std"], target=target, weight=weight, to_scene=ts))
    got = lg(x, t).view(G, S, L, -1)
    assert (got[:, 0, 0, 0:3] != 0).all() and (got[:, 1, 0, 0:3] != 0).all()          # columns 0..2 of frame 0 of the earlier windows
    per_window = JointTargets.h3d(g["joints"], g["mean"], g["std"], target=st.windows_of(target.view(G, F, 18), L).view(G * S, L, 6, 3),
                                  weight=st.windows_of(weight, L), to_scene=D(g["to_scene"].repeat_interleave(S, 0)))
    alone = per_window(x, t).view(G, S, L, -1)
    assert not alone[:, :S - 1].any() and not torch.equal(alone, got)


# ---------------------------------------------------------------------------------------------------------------- the update, exact
@pytest.mark.parametrize("guided", ["plain", "one", "two"])
@pytest.mark.parametrize("geometry", [(3, 3, 8, 2, 2), (2, 3, 7, 0, 3), (1, 0, 8, 0, 2), (3, 4, 8, 0, 1)])
def test_stitch_guide_step_equals_the_separate_launches(geometry, guided):
    Sn, ov, Ln, tail, G = geometry
    st = Stitch(Sn, ov, Sn * Ln - (Sn - 1) * ov - tail, length=Ln)
    shape = (G * Sn, Ln, 263)
    B = shape[0]
    d = create_gaussian_diffusion(cmdm_cfg())
    name = "_".join(map(str, geometry))
    c, a, u, x, k, pv, gr = (D(synth.gaussian(f"long_step_{n}_{name}", shape)) for n in ("c", "a", "u", "x", "known", "prev", "grad"))
    s1, s2 = D(torch.linspace(0.5, 7.5, B)), D(torch.linspace(3.0, 1.25, B))
    m = D(synth.gaussian(f"long_step_bits_{name}", shape) > 0.3)
    t = D(torch.tensor(([999, 500, 1, 0, 250, 750, 3, 100, 900])[:B]))
    gk = d.guidance_rows(dev(), "x0")[t]
    br = {} if guided == "plain" else dict(x0_u=u, scale=s1) if guided == "one" else dict(x0_a=a, x0_u=u, scale=s1, scale2=s2)
    comb = c if guided == "plain" else ops.cfg_combine(c, u, s1) if guided == "one" else ops.cfg2_combine(c, a, u, s1, s2)
    rows = d.ddim_tables(dev(), 0.0)
    ddim = tuple(r[t] for r in (rows.a, rows.b, rows.c, rows.d))
    dp = d.dpm_tables(dev(), 2)
    dpm = tuple(r[t] for r in (dp.a, dp.b, dp.c))
    for impute in (False, True):
        for clip in (False, True):
            ik = dict(known=k, mask=m) if impute else {}
            x0 = ops.stitch_blend(comb, st)                   # the chain of separate launches: blend -> select -> clamp -> guide_step
            if impute:
                x0 = ops.impute(x0, k, m)
            if clip:
                x0 = ops.clamp_(x0.clone(), -1.0, 1.0)
            for rws in (dict(ddim=ddim), dict(dpm=dpm), dict(dpm=dpm, prev=pv)):
                keep, keep2 = torch.empty(shape, device=dev()), torch.empty(shape, device=dev())
                want = ops.guide_step(x0, x, None, grad=gr, gk=gk, x0_out=keep, **({"ddim": ddim + (None,)} if "ddim" in rws else rws))
                got = ops.stitch_guide_step(c, x, st, grad=gr, gk=gk, clip=clip, x0_out=keep2, **rws, **br, **ik)
                assert torch.equal(got, want) and torch.equal(keep2, keep), (geometry, guided, impute, clip, list(rws))
                assert not torch.equal(got, ops.stitch_step(c, x, st, clip=clip, **rws, **br, **ik))          # the term acts
                out = x.clone()                                # in place on x_t, as the loop runs it
                ops.stitch_guide_step(c, out, st, grad=gr, gk=gk, clip=clip, out=out, **rws, **br, **ik)
                assert torch.equal(out, want)
    with pytest.raises(ValueError, match="both required"):
        ops.stitch_guide_step(c, x, st, grad=gr, gk=None, ddim=ddim)
    with pytest.raises(ValueError, match="would have to be shared"):
        ops.stitch_guide_step(c, x, st, grad=gr, gk=gk, ddim=ddim + (ddim[0],))


# ---------------------------------------------------------------------------------------------------------------- the loops, exact
def loop_guide(st, G, form, **kw):
    """a LongGuidance on the CMDM's 263 columns: six contact joints against each window's own map, two target joints, a scale and a
    to_scene per long motion"""
    F = st.check(G * st.windows, st.length)
    mean, std = 0.3 * synth.gaussian("long_loop_mean", (263,)), 0.5 + synth.gaussian("long_loop_std", (263,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    target = 0.5 * synth.gaussian("long_loop_target", (G, F, 2, 3))
    weight = (synth.gaussian("long_loop_weight", (G, F, 2)) > 0.0).float()
    cs, tsc = kw.pop("scale", torch.tensor([1.0, 2.5])[:G]), kw.pop("tscale", torch.tensor([0.5, 0.25])[:G])
    if form == "h3d":
        ts = D(torch.eye(3, 4).repeat(G, 1, 1) + 0.2 * synth.gaussian("long_loop_to_scene", (G, 3, 4)))
        ct = ContactGuidance.h3d(JOINTS, mean, std, to_scene=ts, sigma=SIGMA, scale=cs, **kw)
        tg = JointTargets.h3d([0, 20], mean, std, target=target, weight=weight, to_scene=ts, scale=tsc, **kw)
    else:
        ct = ContactGuidance(SCATTERED, mean, std, sigma=SIGMA, scale=cs, **kw)
        tg = JointTargets(SCATTERED[:2], mean, std, target=target, weight=weight, scale=tsc, **kw)
    return LongGuidance(st, ct, tg)


def _loops(d, sampler):
    if sampler == "ddim":
        return d.ddim_sample_loop, d.ddim_sample_loop_progressive
    return d.dpm_solver_sample_loop, d.dpm_solver_sample_loop_progressive


def _impute(st, shape):
    B, Ln, Dm = shape
    G, F = B // st.windows, st.check(B, Ln)
    known = synth.gaussian("long_loop_known", (G, F, Dm))
    mask = torch.zeros(G, F, Dm, dtype=torch.bool)
    mask[:, [0, Ln - 2, F - 1]] = True
    mask[:, :, 3] = True
    return st.impute(D(known), D(mask))


LOOP_ST = Stitch(S, 3, S * L - 2 * 3 - 2, length=L)          # G = 2, S = 3, L = 8, ov = 3, a padded tail of two frames
LOOP_SHAPE = (2 * S, L, 263)


@pytest.mark.parametrize("guided", ["plain", "one", "two"])
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_native_loop_equals_the_step_by_step_loop(cmdm, d5, sampler, guided):
    st, shape = LOOP_ST, LOOP_SHAPE
    B = shape[0]
    model, kw = guided_model(cmdm, guided, B), conds(B, L, st)
    loop, progressive = _loops(d5, sampler)
    n = d5.num_timesteps
    for form in ("pos", "h3d"):
        guide = loop_guide(st, 2, form)
        for fn in (None, _impute(st, shape)):
            args = dict(clip_denoised=fn is not None, denoised_fn=fn, cond_fn=guide, model_kwargs=kw, seed=21, stitch=st)
            snaps = {j: None for j in range(1, n)}
            native = loop(model, shape, snapshots=snaps, **args)          # (range calls cut at every step, on one workspace)
            steps = [o["sample"].clone() for o in progressive(model, shape, **args)]
            assert len(steps) == n and torch.isfinite(native).all()
            for j in range(1, n):
                assert torch.equal(snaps[j], steps[j - 1]), (sampler, guided, form, fn is not None, j)
                assert shared_frames_agree(st, snaps[j]), (sampler, guided, form, j)
            assert torch.equal(native, steps[-1]) and shared_frames_agree(st, native), (sampler, guided, form, fn is not None)
            assert torch.equal(native, loop(model, shape, **args))          # one call
            cut = {2: None}                                                 # a chain split into two range calls
            assert torch.equal(native, loop(model, shape, snapshots=cut, **args)) and cut[2] is not None and torch.equal(cut[2], snaps[2])
            assert not torch.equal(native, loop(model, shape, **{**args, "cond_fn": None}))          # the guidance acts


def test_two_streams_equal_one_and_a_long_motion_alone_equals_its_rows(cmdm, d5):
    G, st = 4, Stitch(S, 3, length=L)
    shape, kw = (G * S, L, 263), conds(G * S, L, st)
    guide = loop_guide(st, G, "h3d", scale=torch.tensor([1.0, 2.5, 0.5, 1.5]), tscale=torch.tensor([0.5, 0.25, 1.0, 0.125]))
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
def test_a_late_start_launches_the_unguided_loop_until_it_starts(cmdm, d5, form):
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
            for terms in ("both", "contact", "targets"):
                full = loop_guide(st, 2, form, t_start=t_mid)
                guide = full if terms == "both" else LongGuidance(st, full.contact if terms == "contact" else None, full.targets if terms == "targets" else None)
                assert guide.first_guided(d5) == 2
                run(guide), run(None)
                torch.cuda.synchronize()
                with_, without = _device_kernel_names(lambda: run(guide)), _device_kernel_names(lambda: run(None))
                _check(with_, f"long-guided stitched native loop ({sampler}, {form}, {terms})")
                per_step = LAUNCHES[("cols" if form == "pos" else "h3d", terms)]
                print(f"[long guidance launches] {sampler} {form} {terms}: kernels guided {kernels(with_)}, unguided {kernels(without)}, "
                      f"{per_step} a guided step")
                # before first_guided: the unguided stitched loop's kernels; from then on the stated count a step
                for k, cnt in ours(without).items():
                    assert with_.get(k, 0) == cnt + (3 if "stitch_windows_kernel" in k else 0), (k, sampler, form, terms)
                new = set(ours(with_)) - set(ours(without))
                assert new and all(any(p in k for p in LONG_KERNELS) for k in new), new
                assert kernels(with_) == kernels(without) + per_step * 3
                assert count(with_, "stitch_join_kernel") == 3 and count(with_, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
                assert count(with_, "long_nearest") == (3 if terms != "targets" else 0)
                assert not any("guide_nearest" in k or "guide_gather" in k or "guide_sums" in k for k in with_)
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
        for guide in (loop_guide(st, 2, form, scale=0.0, tscale=0.0), loop_guide(st, 2, form, t_start=0),
                      loop_guide(st, 2, form, scale=torch.zeros(2), tscale=torch.zeros(2))):
            assert torch.equal(loop(model, shape, cond_fn=guide, **args), plain), (form,)
            steps = [o["sample"] for o in progressive(model, shape, cond_fn=guide, **args)]
            assert torch.equal(steps[-1], plain), (form,)


# ---------------------------------------------------------------------------------------------------------------- the effect
@pytest.mark.parametrize("form", ["cols", "h3d"])
def test_guidance_lowers_the_energies_of_every_long_motion(form):
    """The identity denoiser of tests/test_gpu_guidance.py::test_guidance_lowers_the_energy_of_every_sample on stitched windows: maps and
    targets made from a known long motion, the chain started from that motion plus noise; for the same start the guided chain ends at
    lower energies than the unguided one, for every long motion.  Two runs compared; no threshold."""
    g = long_case((form, 3, 2, 130, 6, 2))
    st = g["st"]
    G, F = 2, st.frames
    known = 0.5 * st.join(g["x"])
    P = long_positions(known, g["cols"], g["joints"], g["mean"], g["std"], g["to_scene"], torch.float32)
    flat, pc, zero, one, mask = window_positions(P, st)
    g["c"] = contact_terms(flat, mask, g["q"], g["c"], pc, zero, one, SIGMA, torch.float32)[2]          # each window's own map of the known motion
    g["target"], g["weight"] = P, (synth.gaussian("long_effect_weight", (G, F, 6)) > 0.0).float()
    kw = _kw(g)
    start = D(st.windows_of(known + 0.5 * synth.gaussian("long_effect_noise", tuple(known.shape)), L))
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    identity = lambda x, t, **_: x
    args = dict(noise=start, clip_denoised=False, model_kwargs=kw, eta=0.0, device=dev(), stitch=st)
    g["scale"], g["tscale"] = torch.tensor([20.0, 20.0]), torch.tensor([0.05, 0.05])
    both = guidance_of(g, True, True, D)
    e_known = both.energies(D(st.windows_of(known, L)), **kw)
    assert e_known[0].max().item() < 1e-10 and e_known[1].max().item() < 1e-8          # the known motion reproduces its maps and targets
    plain = d.ddim_sample_loop(identity, tuple(start.shape), **args)
    for terms in ("contact", "targets"):
        guide = guidance_of(g, terms == "contact", terms == "targets", D)
        (guide.contact or guide.targets).t_start = 601
        guided = d.ddim_sample_loop(identity, tuple(start.shape), cond_fn=guide, **args)
        i = 0 if terms == "contact" else 1
        e_start, e_plain, e_guided = (both.energies(v, **kw)[i] for v in (start, plain, guided))
        print(f"[long guidance effect] {form} {terms}: energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
        assert shared_frames_agree(st, guided) and (e_guided < e_plain).all()


# ---------------------------------------------------------------------------------------------------------------- two stages
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_long_motion_sample_takes_the_terms(cmdm, cdm):
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    G, F, ov = 2, 35, 4                                       # L = 15, a padded tail of 2 frames in the last window
    text, xyz = D(synth.text_feature(G * S)).view(G, S, -1), D(synth.scene_cloud(G, N, seed=14))
    st = Stitch(S, ov, F)
    full = loop_guide(st, G, "h3d")
    args = dict(text_feat=text, xyz=xyz, frames=F, overlap=ov, seed=9)
    for sampler in ("dpm++", "ddim"):
        run = lambda **kw: long_motion_sample(cdm, d_adm, cmdm, d_amdm, sampler=sampler, **args, **kw)
        terms = dict(contact_guidance=full.contact, joint_targets=full.targets)
        out = run(**terms)
        torch.cuda.synchronize()
        names = _device_kernel_names(lambda: run(**terms))
        _check(names, f"long_motion_sample(contact_guidance=, joint_targets=) ({sampler})")
        assert sum(c for k, c in names.items() if "long_nearest_h3d_kernel" in k) == d_amdm.num_timesteps
        assert out["motion"].shape == (G, F, 263) and out["windows"].shape == (G * S, st.length, 263) and torch.isfinite(out["motion"]).all()
        assert shared_frames_agree(st, out["windows"]) and torch.equal(out["motion"], st.join(out["windows"]))
        assert torch.equal(st.windows_of(out["motion"])[:, :st.length - 2], out["windows"][:, :st.length - 2])
        base = run()
        assert torch.equal(base["contact"], out["contact"]) and not torch.equal(base["motion"], out["motion"])
        only = run(joint_targets=full.targets)
        assert not torch.equal(only["motion"], out["motion"]) and not torch.equal(only["motion"], base["motion"])
    for bad in ("ddpm", "ancestral"):
        with pytest.raises(ValueError, match="deterministic"):
            long_motion_sample(cdm, d_adm, cmdm, d_amdm, sampler=bad, contact_guidance=full.contact, **args)
    with pytest.raises(ValueError, match="long form"):
        per_window = JointTargets.h3d([0], full.contact.mean, full.contact.std, target=torch.zeros(G * S, st.length, 1, 3),
                                      weight=torch.zeros(G * S, st.length, 1))
        long_motion_sample(cdm, d_adm, cmdm, d_amdm, joint_targets=per_window, **args)
