"""`-m gpu`: contact guidance and joint recovery for HumanML3D features.  The recovery kernel (afm_h3d_joints) and the four-launch gradient
(afm_contact_guidance with an afm_h3d_layout) against the float64 restatement of tests/test_h3d_guidance_host.py, bounded by the error of
the same expressions in float32 torch (`_bound_row` of tests/test_gpu_guidance.py); the natively guided loops against the step-by-step
loops with the same ContactGuidance.h3d (bit for bit); zero scale and a late start; the effect on the energy; launches; refusals."""
import ctypes as C
import functools

import pytest
import torch

from afm import ffi, ops, synth
from afm.base import create_gaussian_diffusion
from afm.diffusion import ContactGuidance, Impute
from afm.pipeline import two_stage_sample
from gpu_util import PARITY_ROWS, dev, write_parity_table
from test_gpu_cdm import cdm_cfg
from test_gpu_cfg import _last
from test_gpu_cmdm import cmdm_cfg
from test_gpu_guidance import FORMS, SHAPE3, _bound_row, _imp3, _kw3, _model, _sampler, cdm, cmdm          # noqa: F401 (cmdm, cdm: fixtures)
from test_gpu_guidance import _guide as _pos_guide
from test_gpu_no_eager_math import _MOVERS, _check, _device_kernel_names
from test_guidance_host import JOINTS, SIGMA
from test_h3d_guidance_host import B, CASES, DUP, ZUP, case_id, h3d_case, h3d_contact_reference, h3d_joints_ref, h3d_terms, zero_column

pytestmark = pytest.mark.gpu
D = lambda t: None if t is None else t.to(dev())
H3D_KERNELS = ("h3d_recover_kernel", "guide_nearest_h3d_kernel", "guide_sums_h3d_kernel", "h3d_adjoint_kernel")
H3D_LAUNCHES_PER_GUIDED_STEP = len(H3D_KERNELS)          # recovery, pass 1, pass 2, adjoint - whatever B, L, N, K


@functools.lru_cache(maxsize=None)
def _case(case):
    """the case's inputs and its float64 / float32 restatements, computed once and shared (read-only)"""
    g = h3d_case(case)
    return g, h3d_contact_reference(**g), h3d_contact_reference(**g, dtype=torch.float32)


def _guidance(g, sl=slice(None), **kw):
    ts = g["to_scene"]
    if ts is not None and ts.dim() == 3:
        ts = ts[sl]
    return ContactGuidance.h3d(g["joints"], g["mean"], g["std"], to_scene=D(ts), sigma=SIGMA, scale=g["scale"][sl], **kw)


# ---------------------------------------------------------------------------------------------------------------- the recovery kernel
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_h3d_joints_vs_float64(case):
    g = _case(case)[0]
    x, mask, ts = g["x"], g["x_mask"], g["to_scene"]
    for joints in (None, g["joints"], [21, 0, 7]):
        got = ops.h3d_joints(D(x), g["mean"], g["std"], x_mask=D(mask), joints=joints, to_scene=D(ts))
        want64 = h3d_joints_ref(x, mask, g["mean"], g["std"], joints, ts, torch.float64)
        want32 = h3d_joints_ref(x, mask, g["mean"], g["std"], joints, ts, torch.float32)
        assert got.dtype == torch.float32 and got.shape == want64.shape == (B, case[0], 22 if joints is None else len(joints), 3)
        _bound_row(f"h3d joints {case_id(case)} J={got.shape[2]}", got, want32, want64)
        assert torch.equal(got, ops.h3d_joints(D(x), g["mean"], g["std"], x_mask=D(mask), joints=joints, to_scene=D(ts)))          # run to run
        for b in range(B):                                      # sample b of the batch is the sample computed alone
            tb = ts[b:b + 1] if ts is not None and ts.dim() == 3 else ts
            alone = ops.h3d_joints(D(x[b:b + 1]), g["mean"], g["std"], x_mask=D(mask[b:b + 1]), joints=joints, to_scene=D(tb))
            assert torch.equal(alone, got[b:b + 1]), (b, joints)
    # a list is the rows of the full answer; without a mask the valid frames of a valid-frames-first mask come out the same
    full = ops.h3d_joints(D(x), g["mean"], g["std"], x_mask=D(mask), to_scene=D(ts))
    assert torch.equal(ops.h3d_joints(D(x), g["mean"], g["std"], x_mask=D(mask), joints=[21, 0, 7], to_scene=D(ts)), full[:, :, [21, 0, 7]])
    plain = ops.h3d_joints(D(x), g["mean"], g["std"], to_scene=D(ts))
    assert torch.equal(plain[~D(mask)], full[~D(mask)])
    if case[0] > DUP[2]:
        assert torch.equal(full[DUP[0], DUP[1]], full[DUP[0], DUP[2]])          # the planted duplicate pose is one on the device too


# ---------------------------------------------------------------------------------------------------------------- the gradient kernels
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_h3d_contact_guidance_kernels_vs_float64(case):
    L, N, K, Dm = case[:4]
    g, (want64, e64), (want32, e32) = _case(case)
    guide = _guidance(g)
    kw = dict(c_pc_xyz=D(g["q"]), c_pc_contact=D(g["c"]), x_mask=D(g["x_mask"]))
    t = torch.zeros(B, dtype=torch.int64, device=dev())
    x = D(g["x"])
    got, energy = guide(x, t, **kw), guide.energy(x, **kw)
    assert got.dtype == torch.float32 and got.shape == g["x"].shape and energy.shape == (B,)
    _bound_row(f"h3d contact guidance grad {case_id(case)}", got, want32, want64)
    _bound_row(f"h3d contact guidance energy {case_id(case)}", energy, e32, e64)
    # exact zeros: columns 67 and above, padded frames, the sample without a valid frame, the zero std
    gc = got.cpu()
    assert not gc[..., 67:].any() and not gc[g["x_mask"]].any() and not gc[2].any() and not gc[..., zero_column(g["joints"])].any()
    assert gc[1].abs().max() > 0 or N == 1
    if L >= 2 and N > 1:                                        # the adjoint reaches the rotation and root velocities of an early frame
        assert gc[0, 0, 0] != 0 and gc[0, 0, 1] != 0
    if L == 1:                                                  # one frame: no later frame depends on its velocities
        assert not gc[..., :3].any()
    fstar = h3d_terms(g["x"], g["x_mask"], g["q"], g["c"], g["joints"], g["mean"], g["std"], g["to_scene"], SIGMA, torch.float64)[3]
    local = [c for j in g["joints"] if j for c in range(4 + 3 * (j - 1), 7 + 3 * (j - 1))] + ([3] if 0 in g["joints"] else [])
    hit = torch.zeros(B, L, dtype=torch.bool)
    for b in range(2):
        hit[b, fstar[b].unique()] = True
    assert not gc[..., local][~hit].any()                       # frames no point is nearest to: no term in their own columns
    other = [c for c in range(3, 67) if c not in local]
    assert not gc[..., other].any()                             # joints that are not guided
    # the same bits run to run; sample b alone, a pair, the full batch
    assert torch.equal(got, guide(x, t, **kw)) and torch.equal(energy, guide.energy(x, **kw))
    for b in range(B):
        alone = _guidance(g, slice(b, b + 1))
        kwb = {k: v[b:b + 1] for k, v in kw.items()}
        assert torch.equal(alone(x[b:b + 1], t[:1], **kwb), got[b:b + 1]) and torch.equal(alone.energy(x[b:b + 1], **kwb), energy[b:b + 1])
    pair = _guidance(g, slice(1, None))
    assert torch.equal(pair(x[1:], t[1:], **{k: v[1:] for k, v in kw.items()}), got[1:])
    # t_start: a sample at or above it gets zeros, the others what they got
    part = _guidance(g, t_start=500)(x, torch.tensor([500, 499, 0], device=dev()), **kw)
    assert not part[0].any() and torch.equal(part[1:], got[1:])


@pytest.mark.parametrize("L,N,K", [(7, 300, 2), (1, 1, 1)])
def test_the_h3d_energy_is_the_column_energy_of_the_recovered_positions(L, N, K):
    """The two forms' pass 1 is one computation on the positions: the h3d energy of x equals, bit for bit, the column-form energy (mean 0,
    std 1: x * 1 + 0 is exact) of the motion whose 3 K columns hold ops.h3d_joints(x) - the same [K][L][3] tile staged, the same search,
    partials and serial sum.  N K = 600: three blocks, the last part-filled; a padded tail frame in sample 0 (L = 7); sample 2 has no
    valid frame."""
    Bn, joints, tag = 3, JOINTS[:K], f"h3d_one_body_L{L}_N{N}_K{K}"
    x = D(synth.gaussian(tag + "_x", (Bn, L, 263)))
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (263,)), 0.5 + synth.gaussian(tag + "_std", (263,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    ts = D(ZUP.repeat(Bn, 1, 1) + 0.2 * synth.gaussian(tag + "_to_scene", (Bn, 3, 4)))
    mask = torch.zeros(Bn, L, dtype=torch.bool)
    mask[0, max(L - 1, 1):] = True
    mask[2] = True
    c = torch.rand((Bn, N, K), generator=torch.Generator().manual_seed(N * 100 + K)) * 0.999 + 0.001
    kw = dict(c_pc_xyz=D(1.5 * synth.gaussian(tag + "_q", (Bn, N, 3))), c_pc_contact=D(c), x_mask=D(mask))
    pos = ops.h3d_joints(x, mean, std, x_mask=kw["x_mask"], joints=joints, to_scene=ts)
    assert pos.shape == (Bn, L, K, 3)
    h3d = ContactGuidance.h3d(joints, mean, std, to_scene=ts, sigma=SIGMA)
    cols = ContactGuidance([3 * k for k in range(K)], torch.zeros(3 * K), torch.ones(3 * K), sigma=SIGMA)
    e_h3d, e_cols = h3d.energy(x, **kw), cols.energy(pos.reshape(Bn, L, 3 * K), **kw)
    print(f"[h3d one body] L={L} N={N} K={K}: h3d {e_h3d.tolist()}, columns {e_cols.tolist()}")
    assert torch.isfinite(e_h3d).all() and (e_h3d > 0).all() and torch.equal(e_h3d, e_cols)


# ---------------------------------------------------------------------------------------------------------------- native loops, exact
def _guide(**kw):
    mean, std = 0.3 * synth.gaussian("h3d_loop_mean", (263,)), 0.5 + synth.gaussian("h3d_loop_std", (263,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    kw.setdefault("scale", torch.tensor([1.0, 2.5, 0.5]))
    kw.setdefault("to_scene", D(ZUP))
    return ContactGuidance.h3d(JOINTS, mean, std, sigma=SIGMA, **kw)


@pytest.mark.parametrize("imputing", [False, True])
@pytest.mark.parametrize("how", ["unguided", "two scales"])
@pytest.mark.parametrize("form", list(FORMS))
def test_native_guided_loop_equals_the_step_by_step_loop(cmdm, form, how, imputing):
    d, loop, progressive = _sampler(form)
    t_mid = d.timestep_map[2] + 1                               # the two first executed steps run unguided, the last three guided
    guide = _guide(t_start=t_mid)
    assert guide.first_guided(d) == 2
    model = _model(cmdm, how)
    args = dict(clip_denoised=imputing, denoised_fn=_imp3() if imputing else None, cond_fn=guide, model_kwargs=_kw3(), seed=4)
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch)
    try:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = 1, True, False
        native = loop(model, SHAPE3, **args)
        assert torch.isfinite(native).all()
        assert torch.equal(native, _last(progressive(model, SHAPE3, **args)))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": None}))
        assert not torch.equal(native, loop(model, SHAPE3, **{**args, "cond_fn": _guide(t_start=t_mid, to_scene=None)}))          # the transform acts
        snaps = {1: None, 3: None}                              # a range-sliced call, cut inside the unguided and the guided part
        assert torch.equal(native, loop(model, SHAPE3, snapshots=snaps, **args)) and all(v is not None for v in snaps.values())
        per_sample = D(ZUP.repeat(3, 1, 1) + 0.2 * synth.gaussian("h3d_loop_to_scene", (3, 3, 4)))          # one matrix per sample, all different
        args_ps = {**args, "cond_fn": _guide(t_start=t_mid, to_scene=per_sample)}
        native_ps = loop(model, SHAPE3, **args_ps)
        assert not torch.equal(native_ps, native) and torch.equal(native_ps, _last(progressive(model, SHAPE3, **args_ps)))
        cmdm.loop_streams, cmdm.loop_streams_auto = 2, False      # two streams: sub-batches of 2 + 1, each with its own samples' matrices
        assert torch.equal(native, loop(model, SHAPE3, **args)) and torch.equal(native_ps, loop(model, SHAPE3, **args_ps))
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto, cmdm.pair_launch = saved


@pytest.mark.parametrize("form,how", [("ddpm", "unguided"), ("ddim", "two scales"), ("2m", "unguided")])
def test_zero_scale_and_a_late_start_reproduce_the_unguided_loop(cmdm, form, how):
    """as tests/test_gpu_guidance.py has it for the column form: for ("ddpm", "unguided") the unguided loop of the same (separate-update)
    form is the step-by-step one"""
    d, loop, progressive = _sampler(form)
    model = _model(cmdm, how)
    args = dict(clip_denoised=False, model_kwargs=_kw3(), seed=4)
    plain = _last(progressive(model, SHAPE3, **args)) if (form, how) == ("ddpm", "unguided") else loop(model, SHAPE3, **args)
    for guide in (_guide(scale=0.0), _guide(t_start=0), _guide(scale=torch.zeros(3))):
        assert torch.equal(loop(model, SHAPE3, cond_fn=guide, **args), plain)
        assert torch.equal(_last(progressive(model, SHAPE3, cond_fn=guide, **args)), plain)


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_guidance_lowers_the_energy_of_every_sample():
    """The identity denoiser of tests/test_gpu_guidance.py::test_guidance_lowers_the_energy_of_every_sample (pred_xstart = x_t: a DDIM
    eta = 0 step is the unguided chain's step plus one gradient-descent step on E at the point the step starts from): a target map made
    from a known h3d motion, the chain started from that motion plus noise; the guided chain ends at a lower energy than the unguided
    one for every sample that has a valid frame.  Two runs compared; no threshold."""
    kw = _kw3()
    guide = _guide(scale=20.0, t_start=601)
    known = 0.5 * synth.gaussian("h3d_effect_motion", SHAPE3)
    mask = kw["x_mask"].cpu()
    chat = h3d_terms(known, mask, kw["c_pc_xyz"].cpu(), kw["c_pc_contact"].cpu(), JOINTS, guide.mean.cpu(), guide.std.cpu(), ZUP, SIGMA,
                     torch.float32)[2]
    kw = dict(c_pc_xyz=kw["c_pc_xyz"], c_pc_contact=D(chat), x_mask=kw["x_mask"])
    assert guide.energy(D(known), **kw).max().item() < 1e-10          # the known motion reproduces its own map
    start = D(known + 0.5 * synth.gaussian("h3d_effect_noise", SHAPE3))
    d = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing="ddim5"))
    identity = lambda x, t, **_: x
    args = dict(noise=start, clip_denoised=False, model_kwargs=kw, eta=0.0, device=dev())
    plain, guided = d.ddim_sample_loop(identity, SHAPE3, **args), d.ddim_sample_loop(identity, SHAPE3, cond_fn=guide, **args)
    e_start, e_plain, e_guided = guide.energy(start, **kw), guide.energy(plain, **kw), guide.energy(guided, **kw)
    print(f"[h3d guidance effect] energy at the start {e_start.tolist()}, unguided {e_plain.tolist()}, guided {e_guided.tolist()}")
    has_valid = ~kw["x_mask"].all(1)
    assert has_valid.all() and (e_guided < e_plain)[has_valid].all()


# ---------------------------------------------------------------------------------------------------------------- launches
def test_guided_h3d_jobs_launch_no_eager_arithmetic_and_four_gradient_kernels_a_step(cmdm, cdm):
    n = 6
    kw = _kw3()
    dd = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=f"ddim{n}"))
    dp = create_gaussian_diffusion(cmdm_cfg(steps=1000, respacing=str(n)))
    t_mid = {"dd": dd.timestep_map[3] + 1, "dp": dp.timestep_map[3] + 1}          # 2 unguided steps, 4 guided ones
    kernels = lambda names: sum(c for k, c in names.items() if "guide_gather_kernel" in k or not _MOVERS.search(k))
    count = lambda names, part: sum(c for k, c in names.items() if part in k)
    assert not any(_MOVERS.search(k) for k in H3D_KERNELS)
    none = Impute(D(synth.gaussian("guide_known", SHAPE3)), torch.zeros(SHAPE3, dtype=torch.bool, device=dev()))
    sep = lambda fn: none if fn is None else None              # the loop of the same (separate-update) form without guidance
    runs = {"ddim": (lambda fn: dd.ddim_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), "dd"),
            "2m": (lambda fn: dd.dpm_solver_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), "dd"),
            "ddpm": (lambda fn: dp.p_sample_loop(cmdm, SHAPE3, clip_denoised=False, denoised_fn=sep(fn), cond_fn=fn, model_kwargs=kw, seed=5), "dp")}
    saved = (cmdm.loop_streams, cmdm.loop_streams_auto)
    cmdm.loop_streams, cmdm.loop_streams_auto = 1, True          # one sub-batch: one update launch per step
    try:
        for name, (run, which) in runs.items():
            h3d, pos = _guide(t_start=t_mid[which]), _pos_guide(t_start=t_mid[which])
            assert h3d.first_guided(dd if which == "dd" else dp) == 2
            run(h3d), run(pos), run(None)                         # (weight pack, workspaces, rows and streams exist before anything is counted)
            torch.cuda.synchronize()
            with_h, with_p, without = (_device_kernel_names(lambda fn=fn: run(fn)) for fn in (h3d, pos, None))
            _check(with_h, f"h3d contact-guided native loop ({name})")
            print(f"[h3d guidance launches] {name}: kernels h3d-guided {kernels(with_h)}, pos-guided {kernels(with_p)}, without {kernels(without)}")
            for k in H3D_KERNELS:
                assert count(with_h, k) == 4 and count(with_p, k) == 0 and count(without, k) == 0, (name, k)
            assert count(with_h, "guide_nearest_kernel") == count(with_h, "guide_gather_kernel") == 0
            assert count(with_h, "sampling_update_kernel") == n == count(without, "sampling_update_kernel")
            assert kernels(with_h) == kernels(without) + H3D_LAUNCHES_PER_GUIDED_STEP * 4
            # a pos-guided job still launches exactly two
            assert count(with_p, "guide_nearest_kernel") == count(with_p, "guide_gather_kernel") == 4
            assert kernels(with_p) == kernels(without) + 2 * 4
    finally:
        cmdm.loop_streams, cmdm.loop_streams_auto = saved
    # both stages, the h3d motion stage guided towards the first stage's own map
    d_adm = create_gaussian_diffusion(cdm_cfg(steps=500, respacing="3"))
    Bn, N, L = 2, 1024, 16
    args = dict(text_feat=D(synth.text_feature(Bn)), xyz=D(synth.scene_cloud(Bn, N, seed=14)), frames=L, sigma=SIGMA, seed=9, sampler="ddim")
    g2 = _guide(scale=2.0)
    two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args)
    torch.cuda.synchronize()
    names = _device_kernel_names(lambda: two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args))
    _check(names, "two_stage_sample(contact_guidance=ContactGuidance.h3d(...))")
    assert all(count(names, k) == n for k in H3D_KERNELS)
    base = two_stage_sample(cdm, d_adm, cmdm, dd, **args)
    got = two_stage_sample(cdm, d_adm, cmdm, dd, contact_guidance=g2, **args)
    assert torch.equal(got["contact"], base["contact"]) and torch.equal(got["cond"], base["cond"]) and not torch.equal(got["motion"], base["motion"])


# ---------------------------------------------------------------------------------------------------------------- refusals
class _H3dLoopProbe:
    """The loaded library with afm_cmdm_guide_loop_range wrapped: in front of every real call, the same call with a layout whose joint is out
    of range, named twice, or whose to_scene stride is neither 0 nor 12 - AFM_E_BADARG each, returned before anything is enqueued."""
    GUIDE = 15

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "afm_cmdm_guide_loop_range":
            return fn

        def call(*args):
            real = args[self.GUIDE]._obj
            assert real.h3d
            for field, val in (("joints", 22), ("joints", -1), ("joints", None), ("to_scene_stride", 5)):
                lay = ffi.H3dLayout.from_buffer_copy(real.h3d.contents)
                if field == "joints":
                    lay.joints[1] = lay.joints[0] if val is None else val
                else:
                    setattr(lay, field, val)
                broken = ffi.ContactGuide.from_buffer_copy(real)
                broken.h3d = C.pointer(lay)
                bad = list(args)
                bad[self.GUIDE] = C.byref(broken)
                assert fn(*bad) == -1, (field, val)
            self.calls += 1
            return fn(*args)
        return call


def test_refusals_leave_the_next_call_untouched(cmdm, monkeypatch):
    guide, imp = _guide(), _imp3()
    runs = []
    for form in FORMS:
        _, loop, _ = _sampler(form)
        for m in (cmdm, _model(cmdm, "one scale")):
            runs.append(lambda m=m, loop=loop: loop(m, SHAPE3, clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=_kw3(), seed=4))
    want = [run().clone() for run in runs]
    probe = _H3dLoopProbe(ffi.load())
    monkeypatch.setattr(ffi, "load", lambda: probe)
    got = [run().clone() for run in runs]
    assert probe.calls == 6 and all(torch.equal(a, b) for a, b in zip(want, got))
    monkeypatch.undo()
    # the C entries themselves: D < 67, a joint out of range or named twice, a workspace of the column form's size
    lib = ffi.load()
    g = _case(CASES[2])[0]
    x, mean, std = D(g["x"]), D(g["mean"]), D(g["std"])
    L = x.shape[1]
    out = torch.full((B, L, 22, 3), 7.0, device=dev())
    call = lambda joints, J, Dm: lib.afm_h3d_joints(x.data_ptr(), mean.data_ptr(), std.data_ptr(), None, joints, J, None, 0, out.data_ptr(), B, L, Dm,
                                                     ffi.stream_of(x))
    i32s = lambda *v: (C.c_int32 * len(v))(*v)
    assert call(None, 0, 66) == -1 and call(i32s(0, 22), 2, 263) == -1 and call(i32s(4, 4), 2, 263) == -1 and call(i32s(0), 0, 263) == -1
    assert call(i32s(*range(22)), 23, 263) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                   # nothing was enqueued
    kw = dict(c_pc_xyz=D(g["q"]), c_pc_contact=D(g["c"]), x_mask=D(g["x_mask"]))
    guide = _guidance(g)
    desc, fm, keep = guide.describe(x, kw)
    small = int(lib.afm_contact_guidance_workspace_bytes(B, desc.N, desc.K))
    need = int(lib.afm_contact_guidance_h3d_workspace_bytes(B, L, desc.N, desc.K))
    assert need > small > 0 and lib.afm_contact_guidance_h3d_workspace_bytes(B, 0, desc.N, desc.K) == -1
    ws, grad = torch.empty(need, dtype=torch.uint8, device=dev()), torch.full_like(x, 7.0)
    args = (C.byref(desc), x.data_ptr(), fm.data_ptr(), None, grad.data_ptr(), None, B, L)
    assert lib.afm_contact_guidance(*args, 263, ws.data_ptr(), small, ffi.stream_of(x)) == -2          # AFM_E_WORKSPACE
    assert lib.afm_contact_guidance(*args, 66, ws.data_ptr(), need, ffi.stream_of(x)) == -1            # D < 67
    torch.cuda.synchronize()
    assert (grad == 7.0).all()
    assert lib.afm_contact_guidance(*args, 263, ws.data_ptr(), need, ffi.stream_of(x)) == 0
    assert torch.equal(grad, guide(x, torch.zeros(B, dtype=torch.int64, device=dev()), **kw))


def test_zz_write_parity_table():
    """Not a check: stores the ratios measured so far (gpu_util.write_parity_table; committed as profiles/h3d_guidance_parity.json), with
    the rule `_bound_row` applied in place of the writer's general one."""
    import json
    path = write_parity_table()
    if path and any(r["name"].startswith("h3d ") for r in PARITY_ROWS):
        table = json.load(open(path))
        table["rule"] = ("rows named 'h3d ...': max|hip - f64| <= 4 * max|f32 torch - f64| + 4 * 2^-23 max|f64| (max norm only, no rms); "
                         "ratio_max = e_hip / (e_ref + floor / 4), floor = 4 * 2^-23 max|f64|")
        json.dump(table, open(path, "w"), indent=1)
