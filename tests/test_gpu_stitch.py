"""`-m gpu`: long motions sampled as overlapping windows stitched in the native loops (afm.diffusion.Stitch; ops.stitch_blend /
stitch_step / stitch_windows / stitch_join; afm_cmdm_stitch_loop_range; afm.pipeline.long_motion_sample).

Bit for bit: the kernels against the CPU float32 expression and against the chain of separate launches; the native loop against the
step-by-step loop in every form; the frames two windows share against each other after every step; the loop identities.  Against the
oracle: the stitched ddim5 and 2M loops and the oracle model run through the restated chain of tests/test_stitch_host.py, in float32 and
in its float64 twin, compared with report_f32_class (margin 4, the project's figure) under the DDIM-loop ceiling of tests/test_gpu_cfg.py
(6e-5), times its AMP = 14 for the guided case.  A convex blend amplifies nothing, so there is no new ceiling."""
import json
import os

import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion, create_model
from afm.cmdm import GuidedCMDM
from afm.diffusion import Impute, Stitch
from afm.pipeline import long_motion_sample
from conftest import golden
from gpu_util import PARITY_ROWS, dev, load_named_weights, report, report_f32_class
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import AMP, DDIM_LOOP
from test_gpu_cmdm import _kw, cmdm_cfg
from test_gpu_no_eager_math import _check, _device_kernel_names
from test_impute_host import SCALE, oracle_model
from test_stitch_host import SHAPES, blend_ref, stitch_of, stitched_chain_ref

pytestmark = pytest.mark.gpu
D = lambda t: t.to(dev())
N = 1024
GUIDED = ("plain", "one", "two")


@pytest.fixture(scope="module")
def cmdm():
    model = create_model(cmdm_cfg(), device=dev())
    load_named_weights(model)
    return model.to(dev()).eval()


@pytest.fixture(scope="module")
def d5():
    return create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))


_CONDS = {}


def conds(B, L, st=None, first=0):
    """the conditions of B windows of L frames (rows first .. first + B of one deterministic set): a text and a contact map per window"""
    key = (first + B, L)
    if key not in _CONDS:
        n = first + B
        _CONDS[key] = dict(c_text_feat=D(synth.text_feature(n)), c_pc_xyz=D(synth.scene_cloud(n, N)), c_pc_contact=D(synth.contact_map(n, N)))
    kw = {k: v[first:first + B] for k, v in _CONDS[key].items()}
    kw["x_mask"] = torch.zeros(B, L, dtype=torch.bool, device=dev()) if st is None else st.x_mask(B // st.windows, dev(), L)
    return kw


def scales(B):
    """a scale per window, different in neighbouring windows"""
    return torch.linspace(0.5, 7.5, B), torch.linspace(3.0, 1.25, B)


def guided_model(cmdm, guided, B):
    s1, s2 = scales(B)
    if guided == "one":
        return GuidedCMDM(cmdm, D(s1))
    if guided == "two":
        return GuidedCMDM(cmdm, {"pc": D(s2), "text": D(s1)})
    return cmdm


def consistent_impute(st, shape, name):
    """an Impute over the windows built from the long form: a few whole frames (shared ones among them) and the root columns"""
    B, L, Dm = shape
    G, F = B // st.windows, st.check(B, L)
    known = synth.gaussian(f"stitch_known_{name}", (G, F, Dm))
    mask = torch.zeros(G, F, Dm, dtype=torch.bool)
    mask[:, [0, L - 2, L - 1, F - 1]] = True
    mask[:, :, 0:4] = True
    return st.impute(D(known), D(mask))


def shared_frames_agree(st, x):
    B, L, Dm = x.shape
    S, ov = st.windows, st.overlap
    v = x.view(B // S, S, L, Dm)
    return all(torch.equal(v[:, k, L - ov:], v[:, k + 1, :ov]) for k in range(S - 1))


# ---------------------------------------------------------------------------------------------------------------- kernels, exact
@pytest.mark.parametrize("name", list(SHAPES))
def test_blend_windows_and_join_equal_the_cpu_expression(name):
    st, shape = stitch_of(name)
    B, L, Dm = shape
    x = synth.gaussian(f"stitch_blend_{name}", shape)
    want = blend_ref(x, st)
    got = ops.stitch_blend(D(x), st)
    assert torch.equal(got.cpu(), want), name
    if st.windows == 1 or st.overlap == 0:
        assert torch.equal(got.cpu(), x)                      # no blend: the input's bits
    else:
        assert not torch.equal(want, x) and shared_frames_agree(st, got)
    buf = D(x).clone()
    assert ops.stitch_blend(buf, st, out=buf) is buf and torch.equal(buf, got)          # in place equals out of place
    assert torch.equal(ops.stitch_blend(got, st), D(blend_ref(want, st)))                # (not idempotent: a blend of equal values rounds again)
    G, F = B // st.windows, st.check(B, L)
    long = synth.gaussian(f"stitch_long_{name}", (G, F, Dm))
    w = st.windows_of(D(long))                                # afm_stitch_windows / afm_stitch_join against the host's slices
    assert torch.equal(w.cpu(), st.windows_of(long)) and torch.equal(st.join(w).cpu(), long)


def _cpu_combine(c, a, u, s1, s2, guided):
    v = lambda r: r.view(-1, 1, 1)
    if guided == "one":
        return u + v(s1) * (c - u)
    if guided == "two":
        return (u + v(s1) * (a - u)) + v(s2) * (c - a)
    return c


@pytest.mark.parametrize("guided", GUIDED)
@pytest.mark.parametrize("name", ["middle", "odd", "ov1", "all_shared", "short", "one_window"])
def test_stitch_step_equals_the_cpu_expression_and_the_separate_launches(name, guided):
    st, shape = stitch_of(name)
    B = shape[0]
    d = create_gaussian_diffusion(cmdm_cfg())
    c, a, u, x, k, pv = (synth.gaussian(f"stitch_step_{n}_{name}", shape) for n in ("c", "a", "u", "x", "known", "prev"))
    s1, s2 = scales(B)
    m = synth.gaussian(f"stitch_step_bits_{name}", shape) > 0.3
    t = torch.tensor(([999, 500, 1, 0, 250, 750, 3, 100, 900])[:B])
    v = lambda r: r.cpu().view(-1, 1, 1)
    g = {} if guided == "plain" else dict(x0_u=D(u), scale=D(s1)) if guided == "one" else dict(x0_a=D(a), x0_u=D(u), scale=D(s1), scale2=D(s2))
    combined = _cpu_combine(c, a, u, s1, s2, guided)
    dcomb = D(c) if guided == "plain" else ops.cfg_combine(D(c), D(u), D(s1)) if guided == "one" else ops.cfg2_combine(D(c), D(a), D(u), D(s1), D(s2))
    assert torch.equal(dcomb.cpu(), combined)
    rows = d.ddim_tables(dev(), 0.0)
    ra, rb, rc, rd = (r[D(t)] for r in (rows.a, rows.b, rows.c, rows.d))
    dp = d.dpm_tables(dev(), 2)
    pa, pb, pc = (r[D(t)] for r in (dp.a, dp.b, dp.c))
    for impute in (False, True):
        for clip in (False, True):
            x0 = blend_ref(combined, st)
            if impute:
                x0 = torch.where(m, k, x0)
            if clip:
                x0 = x0.clamp(-1, 1)
            ik = dict(known=D(k), mask=D(m)) if impute else {}
            # the chain of separate launches: (cfg_combine / cfg2_combine) -> stitch_blend -> impute -> clamp_
            x0d = ops.stitch_blend(dcomb, st)
            if impute:
                x0d = ops.impute(x0d, D(k), D(m))
            if clip:
                x0d = ops.clamp_(x0d.clone(), -1.0, 1.0)
            assert torch.equal(x0d.cpu(), x0), (name, guided, impute, clip)
            eps = (v(ra) * x - x0) / v(rb)
            want = x0 * v(rc) + v(rd) * eps
            got = ops.stitch_step(D(c), D(x), st, ddim=(ra, rb, rc, rd), clip=clip, **g, **ik)
            assert torch.equal(got.cpu(), want), ("ddim", name, guided, impute, clip)
            assert torch.equal(got, ops.ddim_step(x0d, D(x), None, ra, rb, rc, rd, None))
            for prev in (None, pv):
                two = v(pa) * x + v(pb) * x0
                want = two if prev is None else two + v(pc) * prev
                keep = torch.empty(shape, device=dev())
                got = ops.stitch_step(D(c), D(x), st, dpm=(pa, pb, pc), prev=None if prev is None else D(prev), clip=clip, x0_out=keep, **g, **ik)
                assert torch.equal(got.cpu(), want), ("dpm", name, guided, impute, clip, prev is None)
                assert torch.equal(keep.cpu(), x0)            # the history keeps the blended value
                assert torch.equal(got, ops.dpm_step(x0d, D(x), None if prev is None else D(prev), pa, pb, pc))
            out = D(x).clone()                                # in place on x_t, as the loop runs it
            ops.stitch_step(D(c), out, st, ddim=(ra, rb, rc, rd), clip=clip, out=out, **g, **ik)
            assert torch.equal(out, ops.stitch_step(D(c), D(x), st, ddim=(ra, rb, rc, rd), clip=clip, **g, **ik))
    with pytest.raises(ValueError, match="would have to be shared"):
        ops.stitch_step(D(c), D(x), st, ddim=(ra, rb, rc, rd, ra))
    cd = D(c)
    with pytest.raises(ffi.AfmError):                         # x_next on an x0 buffer: another thread still reads it
        ops.stitch_step(cd, D(x), st, ddim=(ra, rb, rc, rd), out=cd)


# ---------------------------------------------------------------------------------------------------------------- the loops, exact
def _loops(d, sampler):
    if sampler == "ddim":
        return d.ddim_sample_loop, d.ddim_sample_loop_progressive
    return d.dpm_solver_sample_loop, d.dpm_solver_sample_loop_progressive


@pytest.mark.parametrize("guided", GUIDED)
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
@pytest.mark.parametrize("name", ["middle", "odd"])
def test_native_loop_equals_the_step_by_step_loop(cmdm, d5, name, sampler, guided):
    st, shape = stitch_of(name)
    B, L, _ = shape
    model, kw = guided_model(cmdm, guided, B), conds(B, L, st)
    loop, progressive = _loops(d5, sampler)
    n = d5.num_timesteps
    imp = consistent_impute(st, shape, name)
    x_T = st.x_T(B, L, shape[2], dev(), 21)
    assert torch.equal(x_T, st.windows_of(ops.randn((B // st.windows, st.full(L), shape[2]), dev(), seed=21, step=-1))) and shared_frames_agree(st, x_T)
    for fn in (None, imp):
        for clip in (False, True):
            snaps = {j: None for j in range(1, n)}
            native = loop(model, shape, clip_denoised=clip, denoised_fn=fn, model_kwargs=kw, seed=21, stitch=st, snapshots=snaps)
            steps = [o["sample"].clone() for o in progressive(model, shape, clip_denoised=clip, denoised_fn=fn, model_kwargs=kw, seed=21, stitch=st)]
            assert len(steps) == n and torch.isfinite(native).all()
            for j in range(1, n):
                assert torch.equal(snaps[j], steps[j - 1]), (name, sampler, guided, fn is not None, clip, j)
                assert shared_frames_agree(st, snaps[j]), (name, sampler, guided, j)
            assert torch.equal(native, steps[-1]), (name, sampler, guided, fn is not None, clip)
            assert shared_frames_agree(st, native)
            if fn is not None:
                sel = imp.mask.bool()
                known = imp.known[sel].clamp(-1, 1) if clip else imp.known[sel]          # (the select stands before the clamp)
                assert torch.equal(native[sel], known)
    free = loop(model, shape, clip_denoised=False, model_kwargs=kw, noise=x_T)          # unstitched from the same noise: the windows drift apart
    assert not shared_frames_agree(st, free)


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
@pytest.mark.parametrize("name", ["ov1", "all_shared", "short", "middle"])
def test_shared_frames_stay_bit_identical_and_join_reads_the_same_from_either_side(cmdm, d5, name, sampler):
    st, shape = stitch_of(name)
    B, L, Dm = shape
    S, ov, G = st.windows, st.overlap, B // st.windows
    n = d5.num_timesteps
    snaps = {j: None for j in range(1, n)}
    out = _loops(d5, sampler)[0](cmdm, shape, clip_denoised=False, model_kwargs=conds(B, L, st), seed=33, stitch=st, snapshots=snaps)
    for x in list(snaps.values()) + [out]:
        assert torch.isfinite(x).all() and shared_frames_agree(st, x), (name, sampler)
        long, v = st.join(x), x.view(G, S, L, Dm)
        F = long.shape[1]
        assert F == st.check(B, L)
        for w in range(S):                                    # every window's valid frames are the long motion's, shared ones from either side
            a = w * (L - ov)
            nfr = min(L, F - a)
            assert torch.equal(long[:, a:a + nfr], v[:, w, :nfr]), (name, sampler, w)


def test_one_window_is_the_imputing_form_loop_with_nothing_known(cmdm, d5):
    st, shape = stitch_of("one_window")
    B, L, _ = shape
    kw = conds(B, L)
    x_T = D(synth.gaussian("stitch_s1_xT", shape))
    nothing = Impute(torch.zeros(shape, device=dev()), torch.zeros(shape, dtype=torch.bool, device=dev()))
    for sampler in ("ddim", "dpm"):
        loop = _loops(d5, sampler)[0]
        for model in (cmdm, guided_model(cmdm, "one", B)):
            got = loop(model, shape, noise=x_T, clip_denoised=False, model_kwargs=kw, stitch=st)
            assert torch.equal(got, loop(model, shape, noise=x_T, clip_denoised=False, denoised_fn=nothing, model_kwargs=kw)), sampler
            assert torch.equal(got, loop(model, shape, noise=x_T, clip_denoised=False, model_kwargs=kw, stitch=Stitch(2, 0))), sampler


@pytest.mark.parametrize("GS", [(4, 2), (3, 3)])
def test_one_stream_equals_two_streams_and_a_group_alone_equals_its_rows(cmdm, d5, GS):
    G, S = GS
    st, L, Dm = Stitch(S, 4, length=16), 16, 263
    B = G * S
    shape, kw = (B, L, Dm), conds(B, L, st)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    try:
        for sampler in ("ddim", "dpm"):
            loop = _loops(d5, sampler)[0]
            cmdm.loop_streams, cmdm.loop_streams_auto = 1, False
            one = loop(cmdm, shape, clip_denoised=False, model_kwargs=kw, seed=8, stitch=st).clone()
            cmdm.loop_streams, cmdm.loop_streams_auto = 2, False          # sub-batches of whole long motions: 2 + 2, or 2 + 1
            two = loop(cmdm, shape, clip_denoised=False, model_kwargs=kw, seed=8, stitch=st).clone()
            assert torch.equal(one, two) and shared_frames_agree(st, two), (GS, sampler)
            g = G - 1                                         # the last group alone, keyed by its global index
            alone = loop(cmdm, (S, L, Dm), clip_denoised=False, model_kwargs=conds(S, L, st, first=g * S), seed=8, sample_index0=g, stitch=st)
            assert torch.equal(alone, one[g * S:]), (GS, sampler)
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved


def test_sliced_2m_chain_equals_the_unsliced_chain(cmdm, d5):
    st, shape = stitch_of("middle")
    B, L, _ = shape
    model, kw = guided_model(cmdm, "one", B), conds(B, L, st)
    whole = d5.dpm_solver_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=5, stitch=st).clone()
    sliced = d5.dpm_solver_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=5, stitch=st, progress=True)
    assert torch.equal(whole, sliced)


def test_second_stitched_loop_launches_no_eager_arithmetic(cmdm, d5):
    st, shape = stitch_of("middle")
    B, L, _ = shape
    model, kw = guided_model(cmdm, "two", B), conds(B, L, st)
    imp = consistent_impute(st, shape, "middle")
    run = lambda: d5.dpm_solver_sample_loop(model, shape, clip_denoised=True, denoised_fn=imp, model_kwargs=kw, seed=5, stitch=st)
    run()
    torch.cuda.synchronize()
    names = _device_kernel_names(run)
    _check(names, "stitched native loop")
    assert sum(c for k, c in names.items() if "sampling_update_kernel" in k) == d5.num_timesteps          # one update launch per step
    assert not any("stitch_blend_kernel" in k for k in names) and any("stitch_windows_kernel" in k for k in names)      # the blend rides in it


# ---------------------------------------------------------------------------------------------------------------- two stages
@pytest.fixture(scope="module")
def cdm():
    m = create_model(cdm_cfg(), device=dev())
    load_named_weights(m)
    return m.to(dev()).eval()


def test_long_motion_sample_equals_the_stages_by_hand(cmdm, cdm):
    from afm import dist as adist
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="5"))
    d_amdm = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    G, S, F, ov = 2, 3, 35, 4                                 # L = 15, a padded tail of 2 frames in the last window
    text, xyz = D(synth.text_feature(G * S)).view(G, S, -1), D(synth.scene_cloud(G, N, seed=14))
    for sampler in ("dpm++", "ddim"):
        for scale in (None, torch.linspace(1.0, 6.0, G * S)):
            out = long_motion_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=F, overlap=ov, sampler=sampler, guidance_scale=scale, seed=9)
            st = Stitch(S, ov, F)
            L = st.length
            assert L == 15 and out["contact"].shape == (G, S, N, 6) and out["motion"].shape == (G, F, 263) and out["windows"].shape == (G * S, L, 263)
            loop = (lambda d, *a, **k: d.ddim_sample_loop(*a, eta=0.0, **k)) if sampler == "ddim" else (lambda d, *a, **k: d.dpm_solver_sample_loop(*a, **k))
            flat, cloud = text.reshape(G * S, -1), xyz[:, None].expand(G, S, N, 3).reshape(G * S, N, 3)
            contact = loop(d_adm, cdm, (G * S, N, 6), clip_denoised=False, model_kwargs=dict(c_text_feat=flat, c_pc_xyz=cloud), seed=9)
            assert torch.equal(out["contact"].reshape(G * S, N, 6), contact)
            cond = adist.adm_to_amdm_condition(contact, sigma=0.8, mean=0.0, std=1.0)
            assert torch.equal(out["cond"], cond)
            kw = dict(c_text_feat=flat, c_pc_xyz=cloud, c_pc_contact=cond, x_mask=st.x_mask(G, dev()))
            model = cmdm if scale is None else GuidedCMDM(cmdm, scale)
            windows = loop(d_amdm, model, (G * S, L, 263), clip_denoised=False, model_kwargs=kw, seed=10, stitch=st)
            assert torch.equal(out["windows"], windows) and torch.equal(out["motion"], st.join(windows)) and shared_frames_agree(st, windows)
    args = dict(text_feat=text, xyz=xyz, frames=F, overlap=ov)
    with pytest.raises(ValueError, match="deterministic"):
        long_motion_sample(cdm, d_adm, cmdm, d_amdm, sampler="ddpm", **args)
    with pytest.raises(ValueError, match="at most two windows"):
        long_motion_sample(cdm, d_adm, cmdm, d_amdm, **dict(args, overlap=12))
    with pytest.raises(ValueError, match="text_feat is"):
        long_motion_sample(cdm, d_adm, cmdm, d_amdm, **dict(args, text_feat=text.reshape(G * S, -1)))
    with pytest.raises(ValueError, match="long form"):
        long_motion_sample(cdm, d_adm, cmdm, d_amdm, motion_impute=Impute(torch.zeros(G * S, 15, 263, device=dev()),
                                                                         torch.zeros(G * S, 15, 263, dtype=torch.bool, device=dev())), **args)
    known = D(synth.gaussian("stitch_long_known", (G, F, 263)))
    mask = torch.zeros(G, F, 1, dtype=torch.bool, device=dev())
    mask[:, [0, 12, F - 1]] = True
    got = long_motion_sample(cdm, d_adm, cmdm, d_amdm, motion_impute=Impute(known, mask), seed=9, **args)
    sel = mask.expand(G, F, 263)
    assert torch.equal(got["motion"][sel], known[sel]) and torch.isfinite(got["motion"]).all()


# ---------------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_stitched_loop_vs_the_oracle_chain(cmdm, d5, sampler, guided):
    """G = 1, S = 2, L = 16, ov = 4 on the goldens' case (guided: scales 2.5 and 7.5, different in the two windows)."""
    g = golden("cmdm_forward_N1024_L16")
    st, shape = Stitch(2, 4, length=16), (2, 16, 263)
    x_T = st.windows_of(synth.gaussian("stitch_chain_xT", (1, st.full(16), 263)))
    model = GuidedCMDM(cmdm, torch.tensor(SCALE, device=dev())) if guided else cmdm
    native = _loops(d5, sampler)[0](model, shape, noise=D(x_T), clip_denoised=False, model_kwargs=_kw(g), stitch=st)
    want32 = stitched_chain_ref(oracle_model(guided), st, x_T, d5, sampler)
    want64 = stitched_chain_ref(oracle_model(guided, f64=True), st, x_T.double(), d5, sampler)
    tol = DDIM_LOOP * (AMP if guided else 1.0)
    tag = f"stitched {sampler} loop ddim5{' guided' if guided else ''}"
    assert shared_frames_agree(st, native) and shared_frames_agree(st, want32)
    report(tag, native, want32, tol)
    report_f32_class(tag, native, want32, want64, tol)


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures of the stitched loops measured so far (committed as profiles/stitch_parity.json)."""
    rows = [r for r in PARITY_ROWS if r["name"].startswith("stitched ")]
    if not rows:
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.abspath(os.environ.get("AFM_PARITY_OUT") or os.path.join(root, "build", "parity"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "stitch_parity.json"), "w") as f:
        json.dump({"rule": "max|hip - f64| <= margin * max|ref32 - f64| + 2^-23 max|f64|, the same for the rms; "
                           "ratio = e_hip / (e_ref + floor / margin)", "rows": rows}, f, indent=1)
