"""Cost of contact guidance in the CMDM's sampling loops on one MI355X, printed as ONE JSON line (and as a markdown table with --md).

    python tools/bench_contact_guidance.py [--repr pos|h3d] [--targets] [--reps 5] [--parent-lib PATH] [--md PATH]

L = 196, N = 8192 contact points, K = 6 contact joints, the benchmark's synthetic weights, at B = 1 and at B = 32, for DDIM (eta = 0) at
"ddim50" and DPM-Solver++(2M) at "logsnr20".  Arms, ms per sample call (the loop call and the final synchronise):

    unguided        the native loop without a cond_fn
    native_guided   the same loop with a ContactGuidance as cond_fn (afm_cmdm_guide_loop_range)
    step_guided     the step-by-step loop with the same ContactGuidance (the progressive generator, consumed)
    parent          --parent-lib: the unguided loop of a libafm_hip.so built from the parent commit, in a fresh child process

--repr pos (the default) guides absolute-position columns (two gradient launches a step).  --repr h3d guides the same D = 263 vector as
HumanML3D features with ContactGuidance.h3d and the y-up to z-up transform (four launches: recovery, the two passes, adjoint), the same
L, N, K and batches, and adds the arm

    pos_guided      the native loop with the absolute-column ContactGuidance of --repr pos, for the cost of the two extra launches

--targets measures joint-position targets (afm.diffusion.JointTargets, K = 6 joints, every second frame of every joint weighted) at
"ddim50" alone, pos or h3d, with the arms

    unguided, contact_guided                    the native loops without a cond_fn and with the ContactGuidance of the plain mode
    targets_guided, both_guided                 the native loops with the JointTargets and with MotionGuidance(contact, targets)
    step_targets, step_both                     the step-by-step loops with the same two guidances
    parent_unguided, parent_contact_guided      --parent-lib: the first two arms on the parent commit's library, in a fresh child process

and the ratios guided step / unguided step, native / step by step, and this build / the parent's for the two arms the parent has.

A timed window is as many back-to-back loop calls as fill 100 ms (a single B = 1 call of 7 - 27 ms is too short a window), reported per
call.  The arms alternate inside every repetition and every repetition is kept (median, best, spread (max - min) / median), as the other
bench tools do; the parent's child process runs between the repetitions of this one.  The condition tokens of a batch are computed before
its arms, so that no arm pays for them.  Exit status 1 unless the native guided loop beats the step-by-step one in every cell.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

L, N, D = 196, 8192, 263
BATCHES = (1, 32)
SAMPLERS = {"ddim50": ("ddim50", "ddim"), "dpm2m_logsnr20": ("logsnr20", "dpm")}
JOINTS = [0, 10, 11, 12, 20, 21]
NEW_TARGETS = ("afm_motion_guidance", "afm_motion_guidance_workspace_bytes", "afm_cmdm_motion_guide_loop_range",
               "afm_cmdm_motion_guide_loop_workspace_bytes")
NEW = ("afm_guide_step", "afm_contact_guidance", "afm_contact_guidance_workspace_bytes", "afm_cmdm_guide_loop_range",
       "afm_cmdm_guide_loop_workspace_bytes", "afm_contact_guidance_h3d_workspace_bytes", "afm_h3d_joints")


def _setup(dev, lib=None, targets=False):
    from afm import ffi
    if lib:
        ffi._LIB_PATH = os.path.abspath(lib)          # (before the first load(): the parent build has none of the guidance entry points)
        for name in NEW_TARGETS + (() if targets else NEW):          # (--targets: the parent has the contact guidance, not the targets)
            ffi.EXPORTS.pop(name, None)
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    cfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263",
                                                                                "model.text_model.max_length=20", "diffusion.steps=1000",
                                                                                f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg("ddim50"), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    diffs = {k: create_gaussian_diffusion(cfg(resp)) for k, (resp, _) in SAMPLERS.items()}
    kws = {b: dict(c_text_feat=synth.text_feature(b).to(dev), c_pc_xyz=synth.scene_cloud(b, N).to(dev),
                   c_pc_contact=synth.contact_map(b, N).to(dev), x_mask=torch.zeros(b, L, dtype=torch.bool, device=dev)) for b in BATCHES}
    return model, diffs, kws


MIN_WINDOW_S = 0.1              # a timed window holds as many loop calls as fill it: a 7 ms call alone is too short to carry a 3 % claim


def _timed(fn, calls=1):
    """seconds per call over one window of `calls` back-to-back calls and the final synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _calls(fn):
    """warm-up (weight packs, condition tokens, workspaces, rows), then the calls per window from one timed call"""
    fn()
    fn()
    return max(1, math.ceil(MIN_WINDOW_S / _timed(fn)))


def _runner(model, diffs, kws, sampler, b, guide=None, step_by_step=False):
    d, kind = diffs[sampler], SAMPLERS[sampler][1]
    args = dict(clip_denoised=False, cond_fn=guide, model_kwargs=kws[b], seed=1)
    if kind == "ddim":
        loop = d.ddim_sample_loop_progressive if step_by_step else d.ddim_sample_loop
        args["eta"] = 0.0
    else:
        loop = d.dpm_solver_sample_loop_progressive if step_by_step else d.dpm_solver_sample_loop
    if not step_by_step:
        return lambda: loop(model, (b, L, D), **args)

    def consume():
        for _ in loop(model, (b, L, D), **args):
            pass
    return consume


def worker(lib, reps, targets=False, repr_="pos"):
    """Child process: the unguided loops of another build's library, `reps` timed runs per cell -> one JSON line of seconds.
    `targets`: "ddim50" alone, and the contact-guided loop of that library too."""
    dev = torch.device("cuda:0")
    model, diffs, kws = _setup(dev, lib, targets)
    out = {}
    for b in BATCHES:
        for s in (TARGET_SAMPLERS if targets else SAMPLERS):
            run = _runner(model, diffs, kws, s, b)
            n = _calls(run)
            model.condition_tokens(**kws[b])
            out[f"{s}/{b}"] = [_timed(run, n) for _ in range(reps)]
            if targets:
                run = _runner(model, diffs, kws, s, b, guide=_guides(repr_, dev, b)["contact_guided"])
                n = _calls(run)
                out[f"{s}/{b}/contact"] = [_timed(run, n) for _ in range(reps)]
    print("WORKER " + json.dumps(out), flush=True)


TARGET_SAMPLERS = ("ddim50",)
TARGET_SCALE = 1e-3


def _guides(repr_, dev, b):
    """the guidances of the --targets arms for a batch of b: contact, targets, both (K = 6 joints each, the same mean / std and transform).
    The targets' scale is small on purpose: the un-normalised energy times the early steps' coefficient (gk is about 20 at t = 980) would
    otherwise drive the synthetic model's samples to inf, and a chip at its power limit runs non-finite data faster than real data - every
    guided arm's final sample is checked to be finite ("finite" in the JSON line)."""
    from afm import synth
    from afm.diffusion import ContactGuidance, JointTargets, MotionGuidance
    mean, std = torch.zeros(D), torch.ones(D)
    K = len(JOINTS)
    target = 1.5 * synth.gaussian(f"bench_targets_{b}", (b, L, K, 3))
    weight = torch.zeros(b, L, K)
    weight[:, ::2] = 0.01
    if repr_ == "h3d":
        zup = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]], device=dev)
        contact = ContactGuidance.h3d(JOINTS, mean, std, to_scene=zup, sigma=0.8, scale=1.0)
        targets = JointTargets.h3d(JOINTS, mean, std, to_scene=zup, target=target, weight=weight, scale=TARGET_SCALE)
    else:
        contact = ContactGuidance([3 * j for j in JOINTS], mean, std, sigma=0.8, scale=1.0)
        targets = JointTargets([3 * j for j in JOINTS], mean, std, target=target, weight=weight, scale=TARGET_SCALE)
    return {"contact_guided": contact, "targets_guided": targets, "both_guided": MotionGuidance(contact, targets)}


def _markdown_targets(out):
    lines = [f"# Joint-position targets in the CMDM sampling loops ({out['repr']})", "",
             f"`tools/bench_contact_guidance.py --targets --repr {out['repr']}`, {out['device']}, L = {L}, N = {N}, K = {len(JOINTS)}, ddim50, {out['reps']} "
             "repetitions, arms alternating inside every repetition, a timed window = the loop calls that fill 100 ms.  ms per sample call "
             "(median; spread = (max - min) / median).  "
             f"Every guided arm's final sample finite: {all(out['finite'].values())}.", "", "| B | arm | ms / call | ms / step | spread |", "|---|---|---|---|---|"]
    for b in BATCHES:
        for arm, v in out["ddim50"][f"B{b}"].items():
            if isinstance(v, dict):
                lines.append(f"| {b} | {arm} | {v['ms_per_sample_call']} | {v['ms_per_step']} | {v['spread']} |")
    names = ("targets_over_unguided", "both_over_unguided", "contact_over_unguided", "step_over_native_targets", "step_over_native_both",
             "unguided_over_parent", "contact_over_parent")
    lines += ["", "| B | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]
    for b in BATCHES:
        o = out["ddim50"][f"B{b}"]
        lines.append(f"| {b} | " + " | ".join(str(o.get(n, "n/a")) for n in names) + " |")
    return "\n".join(lines) + "\n"


def main_targets(args):
    dev = torch.device("cuda:0")
    model, diffs, kws = _setup(dev)
    s = TARGET_SAMPLERS[0]
    runs = {}
    for b in BATCHES:
        g = _guides(args.repr, dev, b)
        runs[(b, "unguided")] = _runner(model, diffs, kws, s, b)
        for arm, guide in g.items():
            runs[(b, arm)] = _runner(model, diffs, kws, s, b, guide=guide)
        runs[(b, "step_targets")] = _runner(model, diffs, kws, s, b, guide=g["targets_guided"], step_by_step=True)
        runs[(b, "step_both")] = _runner(model, diffs, kws, s, b, guide=g["both_guided"], step_by_step=True)
    calls = {k: _calls(fn) for k, fn in runs.items()}
    finite = {f"B{b}/{arm}": bool(torch.isfinite(fn()).all()) for (b, arm), fn in runs.items() if arm.endswith("_guided")}
    times = {k: [] for k in runs}
    parent = {}
    for _ in range(args.reps):
        if args.parent_lib:                                   # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "1", "--targets", "--repr", args.repr],
                               capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            for key, ts in json.loads(line[0][7:]).items():
                parent.setdefault(key, []).extend(ts)
        for b in BATCHES:
            model.condition_tokens(**kws[b])
            for (bb, arm), fn in runs.items():
                if bb == b:
                    times[(b, arm)].append(_timed(fn, calls[(b, arm)]))
    out = {"tool": "bench_contact_guidance --targets", "repr": args.repr, "device": torch.cuda.get_device_name(0), "L": L, "N": N, "reps": args.reps,
           "finite": finite, s: {}}
    steps = diffs[s].num_timesteps
    ok = all(finite.values())
    for b in BATCHES:
        o = {arm: _stats(ts, steps) for (bb, arm), ts in times.items() if bb == b}
        ms = lambda arm: o[arm]["ms_per_sample_call"]
        if f"{s}/{b}" in parent:
            o["parent_unguided"], o["parent_contact_guided"] = _stats(parent[f"{s}/{b}"], steps), _stats(parent[f"{s}/{b}/contact"], steps)
            o["unguided_over_parent"] = round(ms("unguided") / ms("parent_unguided"), 4)
            o["contact_over_parent"] = round(ms("contact_guided") / ms("parent_contact_guided"), 4)
        for arm in ("targets", "both", "contact"):
            o[f"{arm}_over_unguided"] = round(ms(f"{arm}_guided") / ms("unguided"), 4)
        o["step_over_native_targets"] = round(ms("step_targets") / ms("targets_guided"), 4)
        o["step_over_native_both"] = round(ms("step_both") / ms("both_guided"), 4)
        ok = ok and o["step_over_native_targets"] > 1.0 and o["step_over_native_both"] > 1.0
        out[s][f"B{b}"] = o
    print(json.dumps(out))
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(_markdown_targets(out))
    return 0 if ok else 1


def _stats(ts, steps):
    med = statistics.median(ts)
    return {"ms_per_sample_call": round(1e3 * med, 3), "ms_per_step": round(1e3 * med / steps, 4), "best_ms": round(1e3 * min(ts), 3),
            "spread": round((max(ts) - min(ts)) / med, 4), "all_ms": [round(1e3 * t, 3) for t in ts]}


def _markdown(out):
    h3d = out.get("repr") == "h3d"
    lines = ["# Contact guidance in the CMDM sampling loops" + (" on HumanML3D features" if h3d else ""), "",
             f"`tools/bench_contact_guidance.py{' --repr h3d' if h3d else ''}`, {out['device']}, L = {L}, N = {N}, K = {len(JOINTS)}, {out['reps']} repetitions, arms alternating "
             "inside every repetition, a timed window = the loop calls that fill 100 ms.  ms per sample call (median; spread = (max - min) / median).", "",
             "| sampler | B | arm | ms / call | ms / step | spread |", "|---|---|---|---|---|---|"]
    for s in SAMPLERS:
        for b in BATCHES:
            for arm, v in out[s][f"B{b}"].items():
                if isinstance(v, dict):
                    lines.append(f"| {s} | {b} | {arm} | {v['ms_per_sample_call']} | {v['ms_per_step']} | {v['spread']} |")
    extra = ("guided step / pos-guided step | ", "---|") if h3d else ("", "")
    lines += ["", f"| sampler | B | guided step / unguided step | {extra[0]}step-by-step guided / native guided | unguided / parent unguided |",
              f"|---|---|---|{extra[1]}---|---|"]
    for s in SAMPLERS:
        for b in BATCHES:
            o = out[s][f"B{b}"]
            mid = f"{o['guided_over_pos_guided']} | " if h3d else ""
            lines.append(f"| {s} | {b} | {o['guided_over_unguided']} | {mid}{o['step_over_native']} | {o.get('unguided_over_parent', 'n/a')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repr", choices=("pos", "h3d"), default="pos", help="what the motion vector holds: absolute positions or HumanML3D features")
    ap.add_argument("--targets", action="store_true", help="measure joint-position targets, alone and summed with the contact guidance (ddim50)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps, args.targets, args.repr)
    if args.targets:
        return main_targets(args)
    dev = torch.device("cuda:0")
    model, diffs, kws = _setup(dev)
    from afm.diffusion import ContactGuidance
    guide = pos_guide = ContactGuidance([3 * j for j in JOINTS], torch.zeros(D), torch.ones(D), sigma=0.8, scale=1.0)
    if args.repr == "h3d":
        zup = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]], device=dev)
        guide = ContactGuidance.h3d(JOINTS, torch.zeros(D), torch.ones(D), to_scene=zup, sigma=0.8, scale=1.0)
    arms = {"unguided": dict(), "native_guided": dict(guide=guide), "step_guided": dict(guide=guide, step_by_step=True)}
    if args.repr == "h3d":
        arms["pos_guided"] = dict(guide=pos_guide)
    runs = {(s, b, arm): _runner(model, diffs, kws, s, b, **kw) for s in SAMPLERS for b in BATCHES for arm, kw in arms.items()}
    calls = {k: _calls(fn) for k, fn in runs.items()}
    times = {k: [] for k in runs}
    parent = {}
    for _ in range(args.reps):
        if args.parent_lib:                                   # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "1"], capture_output=True,
                               text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            for key, ts in json.loads(line[0][7:]).items():
                parent.setdefault(key, []).extend(ts)
        for b in BATCHES:
            model.condition_tokens(**kws[b])
            for s in SAMPLERS:
                for arm in arms:
                    times[(s, b, arm)].append(_timed(runs[(s, b, arm)], calls[(s, b, arm)]))
    out = {"tool": "bench_contact_guidance", "repr": args.repr, "device": torch.cuda.get_device_name(0), "L": L, "N": N, "reps": args.reps}
    ok = True
    for s in SAMPLERS:
        out[s] = {}
        steps = diffs[s].num_timesteps
        for b in BATCHES:
            o = {arm: _stats(times[(s, b, arm)], steps) for arm in arms}
            if f"{s}/{b}" in parent:
                o["parent"] = _stats(parent[f"{s}/{b}"], steps)
                o["unguided_over_parent"] = round(o["unguided"]["ms_per_sample_call"] / o["parent"]["ms_per_sample_call"], 4)
            o["guided_over_unguided"] = round(o["native_guided"]["ms_per_sample_call"] / o["unguided"]["ms_per_sample_call"], 4)
            o["step_over_native"] = round(o["step_guided"]["ms_per_sample_call"] / o["native_guided"]["ms_per_sample_call"], 4)
            if "pos_guided" in o:
                o["guided_over_pos_guided"] = round(o["native_guided"]["ms_per_sample_call"] / o["pos_guided"]["ms_per_sample_call"], 4)
            ok = ok and o["step_over_native"] > 1.0
            out[s][f"B{b}"] = o
    print(json.dumps(out))
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(_markdown(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
