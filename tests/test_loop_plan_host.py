"""How a CMDM native-loop call is planned, on the host (no GPU): `afm.cmdm.plan_loop_call` over every form the loop runs - the entry and
sizer of the dispatch table, an argument list of the entry's declared length and types with a NULL in every slot the form does not use,
workspace keys shared only where entry, sizer and sizer arguments are shared; `LoopExtras` against the plain tuples callers pass and the
loop's refusals under either; the condition classes under afm.guidance and afm.diffusion, their shared base and its messages."""
import ctypes as C
import itertools
import subprocess
import sys

import pytest
import torch

from afm import ffi
from afm.cmdm import CMDM, LoopExtras, plan_loop_call
from conftest import PKG
from test_ddim_host import _diffusion

UPDATES, GUIDANCES, TERMS = ("ddpm", "ddim", "dpm"), ("none", "cfg", "cfg2"), ("none", "contact", "motion")
FORMS = [f for f in itertools.product(UPDATES, GUIDANCES, (False, True), TERMS, (False, True))
         if not (f[4] and (f[0] == "ddpm" or f[3] != "none"))]          # the loop refuses a stitched ancestral chain and a term on windows


def _table(update, guidance, impute, term, stitch):
    """(entry, sizer) by the dispatch table, in its priority order"""
    plain = {"none": "afm_cmdm_loop_workspace_bytes", "cfg": "afm_cmdm_cfg_loop_workspace_bytes", "cfg2": "afm_cmdm_cfg2_loop_workspace_bytes"}
    if term == "contact":
        return "afm_cmdm_guide_loop_range", "afm_cmdm_guide_loop_workspace_bytes"
    if term == "motion":
        return "afm_cmdm_motion_guide_loop_range", "afm_cmdm_motion_guide_loop_workspace_bytes"
    if stitch:
        return "afm_cmdm_stitch_loop_range", "afm_cmdm_stitch_loop_workspace_bytes"
    if update == "dpm":
        return "afm_cmdm_dpm_loop_range", "afm_cmdm_dpm_loop_workspace_bytes"
    if guidance == "cfg2":
        return "afm_cmdm_cfg2_loop_range", plain["cfg2"]
    if impute:
        return "afm_cmdm_impute_loop_range", plain[guidance]
    if guidance == "cfg":
        return ("afm_cmdm_cfg_sample_loop_range" if update == "ddpm" else "afm_cmdm_cfg_ddim_loop_range"), plain["cfg"]
    return ("afm_cmdm_sample_loop_range" if update == "ddpm" else "afm_cmdm_ddim_loop_range"), plain["none"]


# the C type a slot's value is declared with (a term's and the windows' description: by the entry)
SLOT_TYPES = {"noise": ffi.c_f32p, "tmap": C.c_void_p, "ddim_rows": C.POINTER(ffi.DdimRows), "dpm_rows": C.POINTER(ffi.DpmRows), "c1": ffi.c_f32p,
              "c2": ffi.c_f32p, "sigma": ffi.c_f32p, "cfg": C.POINTER(ffi.CfgArgs), "cfg2": C.POINTER(ffi.Cfg2Args), "known": ffi.c_f32p,
              "mask": C.c_void_p, "stitch": C.POINTER(ffi.Stitch), "n_steps": ffi.i32, "first_step": ffi.i32, "seed": ffi.u64, "sample_index0": ffi.i64}
HEAD, TAIL = 4, 8          # (w, x, cond_tokens, frame_mask) in front of the planned arguments, (B, L, scratch, workspace, bytes, streams x 2, stream) behind


def test_plan_reaches_the_tables_entry_with_a_full_argument_list_for_every_form():
    assert len(FORMS) == 3 * 3 * 2 * 3 + 2 * 3 * 2          # every unstitched form, the stitched deterministic ones without a term
    plans = {}
    for form in FORMS:
        update, guidance, impute, term, stitch = form
        p = plans[form] = plan_loop_call(*form)
        assert (p.entry, p.sizer) == _table(*form), form
        argtypes = ffi.EXPORTS[p.entry][1]
        assert len(p.slots) + HEAD + TAIL == len(argtypes), form
        assert len(p.size_slots) + 4 == len(ffi.EXPORTS[p.sizer][1]), form
        # exactly what the form uses is named, once each; every other slot is a NULL - and a NULL only ever stands for a pointer
        used = {"tmap", "n_steps", "first_step"} | {"ddpm": {"c1", "c2", "sigma"}, "ddim": {"ddim_rows"}, "dpm": {"dpm_rows"}}[update]
        used |= set() if guidance == "none" else {guidance}
        used |= ({"known", "mask"} if impute else set()) | (set() if term == "none" else {"term"}) | ({"stitch"} if stitch else set())
        if p.entry != "afm_cmdm_dpm_loop_range":          # (the 2M entry has no noise and no seed)
            used |= {"noise", "seed", "sample_index0"}
        named = [s for s in p.slots if s is not None]
        assert sorted(named) == sorted(used), form
        types = dict(SLOT_TYPES, term=C.POINTER(ffi.ContactGuide if term == "contact" else ffi.MotionGuide))
        for slot, ctype in zip(p.slots, argtypes[HEAD:]):
            if slot is None:
                assert ctype in (ffi.c_f32p, C.c_void_p) or issubclass(ctype, C._Pointer), (form, ctype)
            else:
                assert ctype is types[slot], (form, slot)
        # the sizer takes the guidance it sizes by (and the term / the windows), NULLs where the form has none
        want = [g if g == guidance else None for g in ("cfg", "cfg2")] + (["term"] if term != "none" else ["stitch"] if stitch else [])
        assert list(p.size_slots) == (want if len(p.size_slots) >= 2 else [w for w in want if w]), form
    # Two forms share a workspace key only if they share sizer and sizer arguments (what fixes the buffer's size) and the entry - but for
    # the three buffers of the plain / one-scale / two-scale sizers, each of which has always served the entries sized by it (sample,
    # ddim and impute; cfg_sample, cfg_ddim and impute; cfg2): there the keys are what they were, so a model keeps one buffer across
    # them.  Forms whose keys differ differ in entry, sizer or sizer arguments.
    for a, b in itertools.combinations(FORMS, 2):
        pa, pb = plans[a], plans[b]
        if pa.key == pb.key:
            assert (pa.sizer, pa.size_slots) == (pb.sizer, pb.size_slots), (a, b)
            assert pa.entry == pb.entry or (pa.key[0] is None and pa.sizer == _table("ddpm", a[1], False, "none", False)[1]), (a, b)
        else:
            assert (pa.entry, pa.sizer, pa.size_slots) != (pb.entry, pb.sizer, pb.size_slots), (a, b)
    for refused in (("ddpm", "none", False, "none", True), ("ddim", "cfg", False, "contact", True), ("dpm", "none", True, "motion", True)):
        with pytest.raises(ValueError):
            plan_loop_call(*refused)


def test_loop_extras_is_the_tuple_callers_pass_and_the_loop_refuses_alike_under_both():
    from afm.diffusion import Stitch
    cfg, guide, st = object(), object(), Stitch(3, 4, length=16)
    for t in ((cfg, True), (None, False, guide), (None, False, None, st), (cfg, False, guide, st)):
        ex = LoopExtras(*t)
        assert tuple(ex)[:len(t)] == t and tuple(ex)[len(t):] == (None, False, None, None)[len(t):]
        assert (ex.cfg, ex.branch_streams, ex.guide, ex.stitch) == (ex[0], ex[1], ex[2], ex[3])
    assert LoopExtras() == (None, False, None, None) and LoopExtras(guide=guide, stitch=st) == (None, False, guide, st)
    d, x = _diffusion(1000, "ddim5"), torch.zeros(6, 16, 8)
    cases = ((dict(), "ancestral", st, None), (dict(ddim_eta=0.5), "ddim_eta = 0.5", st, None), (dict(ddim_eta=0.0, step_noise=x), "no step_noise", st, None),
             (dict(dpm_order=2, step_noise=x), "no step_noise", st, None), (dict(ddim_eta=0.0), "cond_fn guidance with stitch=", st, guide),
             (dict(dpm_order=2), "cond_fn guidance with stitch=", st, guide), (dict(ddim_eta=0.0), "at most two windows", Stitch(3, 9), None))
    for kw, why, stitch, term in cases:
        for bundle in ((None, False, term, stitch), LoopExtras(guide=term, stitch=stitch), LoopExtras(cfg, False, term, stitch)):
            with pytest.raises(ValueError, match=why):
                CMDM.afm_native_loop(None, d, x, {}, _guidance=bundle, **kw)          # (refused before `self` or the device is touched)
    for bundle in ((None, False, None, st), LoopExtras(stitch=st)):
        with pytest.raises(ValueError, match="no multiple of 3 windows"):
            CMDM.afm_native_loop(None, d, torch.zeros(7, 16, 8), {}, ddim_eta=0.0, _guidance=bundle)


MOVED = ("Impute", "Stitch", "CondFnError", "ContactGuidance", "JointTargets", "MotionGuidance", "_guide_mask")


def test_condition_classes_live_in_afm_guidance_and_share_one_base():
    from afm import diffusion, guidance
    from afm.guidance import ContactGuidance, JointTargets
    for name in MOVED:
        assert getattr(diffusion, name) is getattr(guidance, name), name
    assert diffusion._takes.__module__ == "afm.diffusion" and not hasattr(guidance, "_takes")
    # afm.guidance stands below both: a fresh interpreter imports it without them
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import afm.guidance; "
            "print(sorted(m for m in ('afm.diffusion', 'afm.cmdm') if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code, PKG], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[]"
    base = guidance._JointTerm
    assert issubclass(ContactGuidance, base) and issubclass(JointTargets, base) and ContactGuidance.__mro__[1] is JointTargets.__mro__[1] is base
    for attr in ("K", "first_guided", "_init", "_fill", "_on"):          # what they share is the base's, not two copies
        assert attr not in vars(ContactGuidance) and attr not in vars(JointTargets) and attr in vars(base), attr
    # one column case and one h3d case: both refuse a bad scale, a bad triple / joint and a mean / std mismatch, each under its own name
    mean, std = torch.zeros(66), torch.ones(66)
    tw = dict(target=torch.zeros(2, 16, 2, 3), weight=torch.ones(2, 16, 2))
    makers = {"ContactGuidance": (lambda cols, m, s, **kw: ContactGuidance(cols, m, s, **kw), "contact"),
              "JointTargets": (lambda cols, m, s, **kw: JointTargets(cols, m, s, **tw, **kw), "guided")}
    for who, (make, noun) in makers.items():
        assert make([0, 3], mean, std).K == 2
        with pytest.raises(ValueError, match=rf"^{who}: `scale` must be a float or a floating \[B\] tensor, got \(2,\) torch.int64$"):
            make([0, 3], mean, std, scale=torch.tensor([1, 2]))
        with pytest.raises(ValueError, match=rf"^{who}: the column triple 64\.\.66 leaves the motion vector of 66 columns$"):
            make([0, 64], mean, std)
        with pytest.raises(ValueError, match=rf"^{who}: the column triple at 2 overlaps another one$"):
            make([0, 2], mean, std)
        with pytest.raises(ValueError, match=rf"^{who}: 1 to 16 {noun} joints, got 0$"):
            make([], mean, std)
        with pytest.raises(ValueError, match=rf"^{who}: mean and std must be \[D\] and alike, got \(66,\) and \(65,\)$"):
            make([0, 3], mean, std[:65])
    mean, std = torch.zeros(263), torch.ones(263)
    h3d = {"ContactGuidance": (lambda j, m, s, **kw: ContactGuidance.h3d(j, m, s, **kw), "ContactGuidance"),
           "JointTargets": (lambda j, m, s, **kw: JointTargets.h3d(j, m, s, **tw, **kw), r"JointTargets\.h3d")}
    for who, (make, scale_who) in h3d.items():
        g = make([0, 10], mean, std)
        assert g.K == 2 and g.joints == [0, 10] and g.cols == []
        with pytest.raises(ValueError, match=rf"^{scale_who}: `scale` must be a float or a floating \[B\] tensor, got \(2, 1\) torch.float32$"):
            make([0, 10], mean, std, scale=torch.ones(2, 1))
        with pytest.raises(ValueError, match=rf"^{who}\.h3d: joint 22 is outside 0\.\.21$"):
            make([0, 22], mean, std)
        with pytest.raises(ValueError, match=rf"^{who}\.h3d: mean and std must be \[D\] and alike, got \(263,\) and \(262,\)$"):
            make([0, 10], mean, std[:262])
        with pytest.raises(ValueError, match=rf"^{who}\.h3d: the joint recovery reads columns 0\.\.66, the motion vector has 66$"):
            make([0, 10], mean[:66], std[:66])
