"""Long motions as overlapping windows on the host (no GPU): the geometry of afm.diffusion.Stitch and what it refuses, the round trip
long form -> windows -> long form, the weight row against its float64 formula, the C ABI (declared, mirrored, version 7, the loop entry's
refusals - all returned before anything is enqueued), the samplers' refusals and routing, and a CPU float32 restatement of the stitched
DDIM and DPM-Solver++(2M) chains on the oracle model, which keeps the frames two windows share bit-equal in both after every step."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from afm import ffi, synth
from afm import diffusion as gd
from afm.diffusion import Impute, Stitch
from conftest import ROOT
from test_ddim_host import _diffusion, _update
from test_impute_host import oracle_model

NEW = {"afm_stitch_blend", "afm_stitch_windows", "afm_stitch_join", "afm_stitch_step", "afm_cmdm_stitch_loop_workspace_bytes",
       "afm_cmdm_stitch_loop_range"}
# (G, S, L, ov, D, frames or None): the smallest shapes at which each thing can still go wrong (tests/test_gpu_stitch.py runs the same)
SHAPES = {
    "middle": (2, 3, 16, 4, 263, None),           # a middle window with two neighbours
    "odd": (3, 2, 15, 7, 263, None),              # 3945 values per sample: partial last quad, quads straddling the overlap edge, uneven groups
    "ov1": (2, 3, 16, 1, 263, None),
    "all_shared": (1, 3, 16, 8, 263, None),       # 2 * ov == L: every frame of the middle window is shared
    "one_window": (2, 1, 16, 4, 263, None),
    "no_overlap": (2, 3, 16, 0, 263, None),
    "short": (2, 3, 16, 4, 263, 3 * 16 - 2 * 4 - 5),          # a short last window (full - 5)
}


def stitch_of(name):
    G, S, L, ov, D, F = SHAPES[name]
    return Stitch(S, ov, F, length=L), (G * S, L, D)


def blend_ref(x0, st: Stitch):
    """the blend in CPU torch of x0's dtype: each product rounded, then the sum"""
    B, L, D = x0.shape
    S, ov = st.windows, st.overlap
    out = x0.clone()
    if S == 1 or ov == 0:
        return out
    w = torch.from_numpy(st.weights64()).float().to(x0.dtype)          # (float32 row, cast up for the float64 twin)
    wl, wr = w[0].view(1, ov, 1), w[1].view(1, ov, 1)
    v = x0.view(B // S, S, L, D)
    o = out.view(B // S, S, L, D)
    for k in range(S - 1):
        b = (wl * v[:, k, L - ov:]) + (wr * v[:, k + 1, :ov])
        o[:, k, L - ov:] = b
        o[:, k + 1, :ov] = b
    return out


def stitched_chain_ref(model, st: Stitch, x_T, d, sampler, imp=None, clip=False, each=None):
    """The stitched chain on the CPU in x_T's dtype: model -> blend -> select -> clamp -> the DDIM (eta = 0) update of
    tests/test_ddim_host.py or the 2M update (a * x + b * x0) + c * prev on the product's rows.  ``each(j, x0, x)`` sees every step."""
    tmap = torch.tensor(d.timestep_map)
    rows = d.ddim_tables("cpu", 0.0) if sampler == "ddim" else d.dpm_tables("cpu", 2)
    img, prev = x_T, None
    with torch.no_grad():
        for j, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
            x0 = blend_ref(model(img, tmap[torch.tensor([i] * x_T.shape[0])]), st)
            if imp is not None:
                x0 = torch.where(imp[1], imp[0].to(x0.dtype), x0)
            if clip:
                x0 = x0.clamp(-1, 1)
            if sampler == "ddim":
                img = _update(x0, img, None, rows, i)
            else:
                two = rows.a[i] * img + rows.b[i] * x0
                img = two if prev is None else two + rows.c[i] * prev
                prev = x0
            if each is not None:
                each(j, x0, img)
    return img


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_geometry_and_its_refusals():
    st = Stitch(3, 4)
    assert (st.windows, st.overlap, st.frames, st.length) == (3, 4, None, None) and st.full(16) == 40 and st.check(6, 16) == 40
    assert Stitch(4, 20).full(196) == 4 * 196 - 3 * 20
    st = Stitch(3, 4, 35)                         # F names L: ov + ceil((F - ov) / S)
    assert st.length == 15 and st.full(15) == 37 and st.check(6, 15) == 35
    assert Stitch(3, 4, 40).length == 16 and Stitch(3, 4, 38).length == 16 and Stitch(3, 4, 37).length == 15 and Stitch(1, 0, 9).length == 9
    held = 0
    for F in range(9, 200):                       # a derived L holds F with a tail in the last window only - or the F is refused (it would
        for S, ov in ((2, 7), (3, 4), (4, 1), (5, 0)):          # leave the last window nothing of its own: fewer windows hold it)
            try:
                L = Stitch(S, ov, F).length
            except ValueError:
                continue
            held += 1
            assert 2 * ov <= L and (S - 1) * (L - ov) + ov < F <= S * L - (S - 1) * ov, (F, S, ov, L)
    assert held > 700
    with pytest.raises(ValueError, match="padded tail in the last window only"):
        Stitch(4, 1, 10)                          # L = 4: three windows already hold 10 frames
    with pytest.raises(ValueError, match="at least one window"):
        Stitch(0, 4)
    with pytest.raises(ValueError, match="overlap must be >= 0"):
        Stitch(2, -1)
    with pytest.raises(ValueError, match="at most two windows"):
        Stitch(3, 9, length=16)
    with pytest.raises(ValueError, match="at most two windows"):
        Stitch(3, 9).check(6, 16)
    with pytest.raises(ValueError, match="padded tail in the last window only"):
        Stitch(3, 4, 28, length=16)               # 28 = (S-1)(L-ov) + ov: the last window would hold shared frames only
    with pytest.raises(ValueError, match="padded tail in the last window only"):
        Stitch(3, 4, 41, length=16)
    assert Stitch(3, 4, 29, length=16).check(3, 16) == 29
    with pytest.raises(ValueError, match="no multiple of 3 windows"):
        Stitch(3, 4).check(7, 16)
    with pytest.raises(ValueError, match="the sample has 15"):
        Stitch(3, 4, length=16).check(6, 15)
    with pytest.raises(ValueError, match="do not reach past the first overlap"):
        Stitch(3, 4, 4)
    with pytest.raises(ValueError, match="window length is not known"):
        Stitch(3, 4).x_mask(2, "cpu")
    # 2 * ov == L and the degenerate forms are geometry like any other
    assert Stitch(3, 8).check(3, 16) == 32 and Stitch(1, 4).check(5, 16) == 16 and Stitch(3, 0).check(3, 16) == 48


@pytest.mark.parametrize("name", list(SHAPES))
def test_join_of_windows_is_the_long_form(name):
    st, (B, L, D) = stitch_of(name)
    G, F = B // st.windows, st.check(B, L)
    x = synth.gaussian(f"stitch_long_{name}", (G, F, D))
    w = st.windows_of(x)
    assert w.shape == (B, L, D) and torch.equal(st.join(w), x)
    S, ov = st.windows, st.overlap
    v = w.view(G, S, L, D)
    for k in range(S - 1):                        # the shared frames are the same long frames
        assert torch.equal(v[:, k, L - ov:], v[:, k + 1, :ov])
    pad = st.full(L) - F
    m = st.x_mask(G, "cpu")
    assert m.shape == (B, L) and m.dtype == torch.bool and int(m.sum()) == G * pad
    if pad:
        assert m.view(G, S, L)[:, -1, L - pad:].all() and not m.view(G, S, L)[:, :-1].any() and pad <= L - ov      # never inside an overlap
        assert (v[:, -1, L - pad:] == 0).all()
    u8 = (x > 0.3).to(torch.uint8)                # a mask travels the same way
    assert torch.equal(st.join(st.windows_of(u8)), u8)


def test_x_mask_refuses_a_model_that_does_not_mask():
    class M:
        mask_motion = False
    st, (B, L, D) = stitch_of("short")
    with pytest.raises(ValueError, match="mask_motion=True"):
        st.x_mask(2, "cpu", model=M())
    assert not Stitch(3, 4, length=16).x_mask(2, "cpu", model=M()).any()          # nothing padded: nothing to refuse


def test_impute_over_the_windows_agrees_in_the_overlaps():
    st, (B, L, D) = stitch_of("short")
    G, F, S, ov = B // st.windows, st.check(B, L), st.windows, st.overlap
    known = synth.gaussian("stitch_known_long", (G, F, D))
    mask = torch.zeros(G, F, 1, dtype=torch.bool)
    mask[:, [0, 11, 12, 13, 24, F - 1]] = True                  # frames 12..15 and 24..27 are shared
    imp = st.impute(known, mask)
    assert isinstance(imp, Impute) and imp.shape == (B, L, D) and imp.mask.dtype == torch.uint8
    k, m = imp.known.view(G, S, L, D), imp.mask.view(G, S, L, D)
    for w in range(S - 1):
        assert torch.equal(k[:, w, L - ov:], k[:, w + 1, :ov]) and torch.equal(m[:, w, L - ov:], m[:, w + 1, :ov])
    assert torch.equal(st.join(imp.known), known) and torch.equal(st.join(imp.mask), mask.expand(G, F, D).to(torch.uint8))
    assert not imp.mask.view(G, S, L, D)[:, -1, L - (st.full(L) - F):].any()          # the padded tail knows nothing


@pytest.mark.parametrize("ov", [1, 4, 7, 8, 20])
def test_weight_row_is_the_float64_formula_rounded_once(ov):
    st = Stitch(2, ov)
    w = st.weights("cpu")
    assert w.shape == (2, ov) and w.dtype == torch.float32 and w.is_contiguous()
    f = np.arange(ov, dtype=np.float64)
    wr = (f + 1.0) / (ov + 1.0)
    wl = 1.0 - wr
    assert np.array_equal(w[1].numpy(), wr.astype(np.float32)) and np.array_equal(w[0].numpy(), wl.astype(np.float32))
    assert st.weights("cpu") is w                 # built once per device
    assert (w > 0).all() and (w < 1).all()        # a convex blend: it amplifies nothing


# ---------------------------------------------------------------------------------------------------------------- the C surface
def test_stitch_exports_declared_and_structs_mirrored(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert NEW <= declared and NEW <= set(ffi.EXPORTS)
    assert ffi.ABI_VERSION == 7 and re.search(r"#define AFM_ABI_VERSION\s+7\b", hdr)
    # the loop entry is the guided loop's signature with the description swapped
    assert ffi.EXPORTS["afm_cmdm_stitch_loop_range"][1][:15] == ffi.EXPORTS["afm_cmdm_guide_loop_range"][1][:15]
    assert ffi.EXPORTS["afm_cmdm_stitch_loop_range"][1][16:] == ffi.EXPORTS["afm_cmdm_guide_loop_range"][1][16:]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NEW)
    if shutil.which("gcc") is None:
        return
    pairs = (("afm_stitch", ffi.Stitch), ("afm_stitch_step_args", ffi.StitchStepArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, py in pairs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "stitch_layout.c", tmp_path / "stitch_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(out[f"{cname}.size"]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_the_loop_entry_refuses_before_it_enqueues():
    """DDPM rows, rows with a noise term, a step_noise, B % S != 0 and 2 * ov > L: AFM_E_BADARG, returned from the entry's own checks -
    nothing is dereferenced on the device and nothing is launched, so the refusals run without a GPU."""
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ffi.load()
    assert lib.afm_version() == 7
    P = 4096                                      # a non-NULL stand-in for device pointers the refused calls never read
    w = ffi.CmdmWeights()
    ddim, noisy, dpm = ffi.DdimRows(P, P, P, P, None), ffi.DdimRows(P, P, P, P, P), ffi.DpmRows(P, P, P)
    st = ffi.Stitch(3, 4, P)
    R = ctypes.byref

    def call(step_noise=None, rows=R(ddim), dpm_=None, c1=None, c2=None, sg=None, stitch=R(st), B=6, L=16, first=0, known=None, mask=None):
        return lib.afm_cmdm_stitch_loop_range(R(w), P, P, None, step_noise, P, rows, dpm_, c1, c2, sg, None, None, known, mask, stitch, 5, first, 0, 0,
                                              B, L, P, P, 1 << 20, 0, None, None)
    assert call(c1=P, c2=P, sg=P, rows=None) == -1                         # DDPM rows
    assert call(c1=P, c2=P, sg=P) == -1                                    # ... also beside DDIM rows
    assert call(rows=R(noisy)) == -1                                       # a noise term (eta != 0)
    assert call(step_noise=P) == -1
    assert call(B=7) == -1 and call(B=4) == -1                             # B % S != 0
    assert call(L=7) == -1                                                 # 2 * ov > L
    assert call(stitch=R(ffi.Stitch(3, 9, P))) == -1 and call(stitch=R(ffi.Stitch(0, 0, P))) == -1 and call(stitch=R(ffi.Stitch(3, -1, P))) == -1
    assert call(stitch=None) == -1 and call(rows=None) == -1 and call(dpm_=R(dpm)) == -1          # no description; no rows; both kinds
    assert call(first=-1) == -1 and call(known=P) == -1 and call(mask=P) == -1
    assert lib.afm_cmdm_stitch_loop_workspace_bytes(R(w), 6, 16, 0, None, None, None) == -1
    assert lib.afm_cmdm_stitch_loop_workspace_bytes(R(w), 6, 16, 0, None, None, R(ffi.Stitch(3, 9, None))) == -1
    # the small entries: the same geometry, checked before the launch
    assert lib.afm_stitch_blend(P, P, R(st), 7, 16, 263, None) == -1 and lib.afm_stitch_blend(P, P, R(st), 6, 7, 263, None) == -1
    assert lib.afm_stitch_blend(P, P, None, 6, 16, 263, None) == -1 and lib.afm_stitch_blend(P, P, R(ffi.Stitch(3, 4, None)), 6, 16, 263, None) == -1
    assert lib.afm_stitch_windows(P, P, 2, 3, 4, 16, 263, 28, None) == -1 and lib.afm_stitch_windows(P, P, 2, 3, 4, 16, 263, 41, None) == -1
    assert lib.afm_stitch_join(P, P, 2, 3, 9, 16, 263, 30, None) == -1 and lib.afm_stitch_join(P, P, 2, 3, 4, 16, 263, 28, None) == -1
    a = ffi.StitchStepArgs()
    assert lib.afm_stitch_step(R(a), None) == -1 and lib.afm_stitch_step(None, None) == -1
    a.x0_c, a.x_t, a.x_next, a.stitch, a.B, a.L, a.D = P, P, P + 64, ctypes.pointer(st), 6, 16, 263
    assert lib.afm_stitch_step(R(a), None) == -1                           # no rows
    a.ddim = ctypes.pointer(noisy)
    assert lib.afm_stitch_step(R(a), None) == -1                           # a noise term
    a.ddim, a.B = ctypes.pointer(ddim), 7
    assert lib.afm_stitch_step(R(a), None) == -1                           # B % S != 0


# ---------------------------------------------------------------------------------------------------------------- the samplers
class _Stub(torch.nn.Module):
    arch, mask_motion = "trans_enc", True

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.got = None

    def forward(self, x, t, **kw):
        return x * 0.5


class _Names(_Stub):
    def afm_native_loop(self, diffusion, x, model_kwargs, *, stitch=None, impute=None, dpm_order=None, **kw):
        self.got = dict(stitch=stitch, dpm_order=dpm_order, **kw)
        return x


class _Bundle(_Stub):
    def afm_native_loop(self, diffusion, x, model_kwargs, *, _guidance=None, impute=None, dpm_order=None, **kw):
        self.got = dict(stitch=None if _guidance is None else _guidance[3], **kw)
        return x


class _NamesNot(_Stub):
    def afm_native_loop(self, diffusion, x, model_kwargs, *, impute=None, dpm_order=None, **kw):
        self.got = kw
        return x


def test_samplers_refuse_what_a_stitched_chain_cannot_be():
    d = _diffusion(1000, "ddim5")
    st, shape, x = Stitch(3, 4), (6, 16, 8), torch.zeros(6, 16, 8)
    m = _Names()
    with pytest.raises(ValueError, match="every ancestral step draws noise"):
        d.p_sample_loop(m, shape, noise=x, stitch=st)
    with pytest.raises(ValueError, match="would have to be shared"):
        d.ddim_sample_loop(m, shape, noise=x, eta=1.0, stitch=st)
    with pytest.raises(ValueError, match="would have to be shared"):
        d.ddim_sample_loop(m, shape, noise=x, step_noise=torch.zeros(5, 6, 16, 8), stitch=st)
    with pytest.raises(ValueError):
        d.dpm_solver_sample_loop(m, shape, noise=x, step_noise=torch.zeros(5, 6, 16, 8), stitch=st)
    for loop in (d.ddim_sample_loop, d.dpm_solver_sample_loop):
        with pytest.raises(ValueError, match="disagree in the overlaps"):
            loop(m, shape, noise=x, cond_fn=lambda x, t, **kw: x, stitch=st)
        with pytest.raises(ValueError, match="no multiple of 3 windows"):
            loop(m, (7, 16, 8), noise=torch.zeros(7, 16, 8), stitch=st)
        with pytest.raises(ValueError, match="at most two windows"):
            loop(m, shape, noise=x, stitch=Stitch(3, 9))
        with pytest.raises(ValueError, match="afm.diffusion.Stitch"):
            loop(m, shape, noise=x, stitch=(3, 4))
        dec = _Names()
        dec.arch = "trans_dec"
        with pytest.raises(ValueError, match="trans_dec"):
            loop(dec, shape, noise=x, stitch=st)
        nomask = _Names()
        nomask.mask_motion = False
        with pytest.raises(ValueError, match="mask_motion=True"):
            loop(nomask, shape, noise=x, stitch=Stitch(3, 4, 35, length=16))
        assert m.got is None and dec.got is None and nomask.got is None          # refused before the loop is entered
    with pytest.raises(ValueError, match="would have to be shared"):
        d.ddim_sample(m, x, torch.zeros(6, dtype=torch.int64), eta=0.5, stitch=st)
    with pytest.raises(ValueError, match="disagree in the overlaps"):
        d.dpm_solver_sample(m, x, torch.zeros(6, dtype=torch.int64), cond_fn=lambda x, t, **kw: x, stitch=st)
    # the native loop's own refusals (reached by a caller of afm_native_loop), before it touches the device
    from afm.cmdm import CMDM
    for kw, why in ((dict(), "ancestral"), (dict(ddim_eta=0.5), "ddim_eta = 0.5"), (dict(ddim_eta=0.0, step_noise=x), "no step_noise"),
                    (dict(ddim_eta=0.0, _guidance=(None, False, object(), st)), "cond_fn guidance")):
        bundle = kw.pop("_guidance", (None, False, None, st))
        with pytest.raises(ValueError, match=why):
            CMDM.afm_native_loop(None, d, x, {}, _guidance=bundle, **kw)
    with pytest.raises(ValueError, match="no multiple of 3 windows"):
        CMDM.afm_native_loop(None, d, torch.zeros(7, 16, 8), {}, ddim_eta=0.0, _guidance=(None, False, None, st))


def test_sample_loop_goes_native_exactly_when_the_loop_takes_stitch(monkeypatch):
    from afm.cdm import CDM
    from afm.cmdm import CMDM, GuidedCMDM
    from afm.diffusion import _takes
    assert _takes(GuidedCMDM.afm_native_loop, "stitch") and _takes(CMDM.afm_native_loop, "_guidance")
    assert not any(_takes(CDM.afm_native_loop, k) for k in ("stitch", "_guidance"))
    d = _diffusion(1000, "ddim5")
    st, shape, x = Stitch(3, 4), (6, 16, 8), torch.zeros(6, 16, 8)
    stepped = []
    monkeypatch.setattr(gd.GaussianDiffusion, "_progressive",
                        lambda self, *a, **k: stepped.append((a[0].__name__, a[-1].get("stitch"))) or iter([{"sample": x}]))
    monkeypatch.setattr(gd.GaussianDiffusion, "dpm_solver_sample_loop_progressive",
                        lambda self, *a, **k: stepped.append(("dpm", k.get("stitch"))) or iter([{"sample": x}]))
    loops = (("ddim_sample", lambda m, s: d.ddim_sample_loop(m, shape, noise=x, model_kwargs={}, stitch=s)),
             ("dpm", lambda m, s: d.dpm_solver_sample_loop(m, shape, noise=x, model_kwargs={}, stitch=s)))
    for name, run in loops:
        for cls in (_Names, _Bundle):
            m = cls()
            run(m, st)
            assert m.got is not None and m.got["stitch"] is st and not stepped, (name, cls)
        m = _Names()
        run(m, None)
        assert m.got is not None and m.got["stitch"] is None and "_guidance" not in m.got and not stepped, name
        m = _NamesNot()
        run(m, st)                                # a loop that takes it neither way: step by step, the generator handed the stitch
        assert m.got is None and stepped == [(name, st)], name
        stepped.clear()
        m = _NamesNot()
        run(m, None)
        assert m.got is not None and not stepped, name


# ---------------------------------------------------------------------------------------------------------------- the chain, restated
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_restated_chain_keeps_shared_frames_bit_equal(sampler, guided):
    """G = 1, S = 2, L = 16, ov = 4 on the oracle model (guided: scales 2.5 and 7.5 - different in the two windows): after every step the
    blended pred_xstart and x agree bit for bit on the four shared frames, and the long motion reads the same from either side."""
    st = Stitch(2, 4, length=16)
    d = _diffusion(1000, "ddim5")
    x_T = st.windows_of(synth.gaussian("stitch_chain_xT", (1, st.full(16), 263)))
    seen = []

    def each(j, x0, x):
        for v in (x0, x):
            assert torch.equal(v[0, 12:], v[1, :4]), (sampler, guided, j)
        seen.append(j)
    out = stitched_chain_ref(oracle_model(guided), st, x_T, d, sampler, each=each)
    assert seen == list(range(d.num_timesteps)) and torch.isfinite(out).all()
    long = st.join(out)
    assert torch.equal(long[0, :16], out[0]) and torch.equal(long[0, 12:], out[1])
    # without the blend the windows drift apart: the test above is not vacuous
    free = stitched_chain_ref(oracle_model(guided), Stitch(2, 0, length=16), x_T, d, sampler)
    assert not torch.equal(free[0, 12:], free[1, :4])
