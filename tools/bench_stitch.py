"""What stitching costs: long motions sampled as overlapping windows in the native loop (afm.diffusion.Stitch, afm_cmdm_stitch_loop_range).

    python tools/bench_stitch.py [--reps 5] [--parent-lib PATH] [--bench-steps 200] [--md PATH]

Cells: DPM-Solver++(2M) on "logsnr20" and DDIM (eta = 0) on "ddim50", G = 1 and G = 8 long motions of S = 4 windows, L = 196, ov = 20
(724 frames each), N = 8192 scene points, D = 263.  Per cell two arms on the same G * S rows, from the same x_T, alternated inside one
process:

    stitched        ddim_sample_loop / dpm_solver_sample_loop(..., stitch=Stitch(4, 20))
    imputing_form   the same rows in the imputing-form loop (an `Impute` that knows nothing) without stitching: the same launches - stored
                    pred_xstart, one update launch per sub-batch and step - minus the blend, which isolates the blend's cost

reported as ms per long motion and ms per step (median of --reps windows, with the spread), and their ratio.  A timed window holds as many
loop calls as fill 0.1 s.  With --parent-lib (a libafm_hip.so built from the parent commit) `bench.py --gpus 1 --steps K --warmup 20` runs
on this build and on the parent's, alternated, each in a fresh child process while this one idles: bench.py's loops are untouched, so its
figure should lie inside the parent's own call-to-call spread.  One JSON line at the end; --md also writes the table as markdown.

    python tools/bench_stitch.py --guided [contact|targets|both] --repr [pos|h3d] [--parent-lib PATH] [--md profiles/long_guidance_bench.md]

What guiding a stitched chain costs (afm.diffusion.LongGuidance, afm_cmdm_long_guide_loop_range): the same cells, the arms "guided"
(stitch= and the LongGuidance as cond_fn; every step guided) and "stitched" (the same chain without it) alternated in one call, as ms per
long motion, with the guided step's gradient-launch count taken from torch.profiler (device kernels of a guided chain minus those of the
unguided one, per step and sub-batch, counted at G = 1).  With --parent-lib the unguided stitched chain of every cell is also run on the parent's library in a fresh child
process and compared bit for bit (sha256 of the result).

    python tools/bench_stitch.py --clearance [--guided contact|targets|both] --repr [pos|h3d] [--parent-lib PATH] [--md profiles/long_clearance_bench.md]

What a SceneClearance costs on a stitched chain (LongGuidance(stitch, contact, targets, clearance), afm_cmdm_long_scene_guide_loop_range):
K = 16 joints, radius 0.5, every window against its own cloud of N points.  Arms, alternated inside every repetition: "clearance" (the
guided arm with the term added - or, without --guided, the term alone), "guided" (only with --guided: the same LongGuidance without it) and
"stitched" (unguided).  With --parent-lib the "guided" and "stitched" arms also run on the parent commit's library, one timed window each
in a fresh child process in front of every repetition: their code path is the parent's.  --md appends a section to the file.

    python tools/bench_stitch.py --clearance --kernel --repr [pos|h3d] --groups G [--calls 20]

only gradient evaluations of the term on G long motions, for a kernel trace (rocprofv3 --kernel-trace --stats)."""
import argparse
import hashlib
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

S, L, OV, N, D = 4, 196, 20, 8192, 263
GROUPS = (1, 8)
SAMPLERS = {"dpm2m_logsnr20": ("logsnr20", "dpm"), "ddim50": ("ddim50", "ddim")}
NEW = ("afm_stitch_blend", "afm_stitch_windows", "afm_stitch_join", "afm_stitch_step", "afm_cmdm_stitch_loop_workspace_bytes",
       "afm_cmdm_stitch_loop_range")
LONG_NEW = ("afm_long_guidance_workspace_bytes", "afm_long_guidance", "afm_stitch_guide_step", "afm_cmdm_long_guide_loop_workspace_bytes",
            "afm_cmdm_long_guide_loop_range")
LONG_SCENE_NEW = ("afm_long_scene_guidance_workspace_bytes", "afm_long_scene_guidance", "afm_cmdm_long_scene_guide_loop_workspace_bytes",
                  "afm_cmdm_long_scene_guide_loop_range")
CLEAR_K, CLEAR_RADIUS, CLEAR_SCALE = 16, 0.5, 1e-3          # tools/bench_clearance.py's term: a small scale keeps the synthetic model's samples finite
JOINTS = [0, 10, 11, 12, 20, 21]          # the six contact joints of the h3d skeleton
COLS = [4, 259, 100, 7, 193, 64]          # --repr pos: six column triples of the 263-column vector read as absolute positions
MIN_WINDOW_S = 0.1


def _timed(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _stats(ts, steps, groups):
    med = statistics.median(ts)
    return {"ms_per_long_motion": round(med * 1e3 / groups, 3), "ms_per_step": round(med * 1e3 / steps, 4),
            "spread_pct": round(100.0 * (max(ts) - min(ts)) / med, 2), "windows": len(ts)}


def bench_child(lib):
    """Child process: bench.py on another build's library (the entry points it lacks are not bound)."""
    from afm import ffi
    ffi._LIB_PATH = os.path.abspath(lib)
    for name in NEW + LONG_NEW + LONG_SCENE_NEW:
        ffi.EXPORTS.pop(name, None)
    import runpy
    runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")


def _bench_once(lib, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] if lib is None else [sys.executable, os.path.abspath(__file__), "--bench-child", lib]
    r = subprocess.run(cmd + ["--gpus", "1", "--steps", str(steps), "--warmup", "20"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-800:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)["value"]


def _setup():
    """(the CMDM on synthetic weights, its config factory, the device)"""
    from afm import synth
    from afm.base import create_model
    from afm.config import load_config
    dev = torch.device("cuda:0")
    cfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263",
                                                                                "model.text_model.max_length=20", "diffusion.steps=1000",
                                                                                f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg("ddim50"), device=dev)
    synth.fill_module_(model)
    return model.to(dev).eval(), cfg, dev


def _cells(model, cfg, dev):
    """every (sampler, G) cell: (key, diffusion, loop, G, B, model_kwargs, x_T, stitch)"""
    from afm import synth
    from afm.base import create_gaussian_diffusion
    from afm.diffusion import Stitch
    st = Stitch(S, OV, length=L)
    for name, (resp, kind) in SAMPLERS.items():
        d = create_gaussian_diffusion(cfg(resp))
        loop = d.ddim_sample_loop if kind == "ddim" else d.dpm_solver_sample_loop
        for G in GROUPS:
            B = G * S
            kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev),
                      c_pc_contact=synth.contact_map(B, N).to(dev), x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev))
            yield f"{name}/G{G}", d, loop, G, B, kw, st.x_T(B, L, D, dev, 1), st


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hash_child(lib):
    """Child process: the unguided stitched chain of every cell on another build's library; one JSON line of sha256 digests."""
    from afm import ffi
    ffi._LIB_PATH = os.path.abspath(lib)
    for name in LONG_NEW + LONG_SCENE_NEW:
        ffi.EXPORTS.pop(name, None)
    model, cfg, dev = _setup()
    out = {}
    for key, d, loop, G, B, kw, x_T, st in _cells(model, cfg, dev):
        out[key] = _sha(loop(model, (B, L, D), noise=x_T, clip_denoised=False, model_kwargs=kw, stitch=st))
    print(json.dumps(out))


def _long_guide(st, G, terms, form, dev, clearance=False):
    """the LongGuidance of the guided arm: six contact joints against each window's own map, the root's path as targets at every
    tenth long frame, one scale per long motion; ``clearance``: with a SceneClearance on 16 joints as the third term (terms None: alone)"""
    from afm import synth
    from afm.diffusion import ContactGuidance, JointTargets, LongGuidance, SceneClearance
    F = st.full(L)
    mean, std = 0.3 * synth.gaussian("bench_long_mean", (D,)), 0.5 + synth.gaussian("bench_long_std", (D,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    target = synth.gaussian("bench_long_target", (G, F, 1, 3))
    weight = torch.zeros(G, F, 1)
    weight[:, ::10] = 1.0
    scale = torch.full((G,), 2.0)
    ct = tg = None
    if terms in ("contact", "both"):
        ct = ContactGuidance.h3d(JOINTS, mean, std, scale=scale) if form == "h3d" else ContactGuidance(COLS, mean, std, scale=scale)
    if terms in ("targets", "both"):
        kw = dict(target=target, weight=weight, scale=0.1 * scale)
        tg = JointTargets.h3d(JOINTS[:1], mean, std, **kw) if form == "h3d" else JointTargets(COLS[:1], mean, std, **kw)
    clr = None
    if clearance:
        kw = dict(radius=CLEAR_RADIUS, scale=CLEAR_SCALE)
        clr = SceneClearance.h3d(list(range(CLEAR_K)), mean, std, **kw) if form == "h3d" else SceneClearance([3 * j for j in range(CLEAR_K)], mean, std, **kw)
    return LongGuidance(st, ct, tg, clr)


def _kernel_count(fn):
    """device kernels of one call of fn, ATen's movers left out (torch.profiler)"""
    import re
    from torch.profiler import ProfilerActivity, profile
    movers = re.compile(r"(FillFunctor|fill_kernel|copy|Copy|memcpy|Memcpy|memset|Memset)")
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and not movers.search(ev.name))


def _clear_arms(args, model, loop, B, kw, x_T, st, G, dev):
    """the arms of one --clearance cell"""
    run = lambda guide: (lambda: loop(model, (B, L, D), noise=x_T, clip_denoised=False, cond_fn=guide, model_kwargs=kw, stitch=st))
    arms = {"clearance": run(_long_guide(st, G, args.guided, args.repr, dev, clearance=True))}
    if args.guided:
        arms["guided"] = run(_long_guide(st, G, args.guided, args.repr, dev))
    arms["stitched"] = run(None)
    return arms


def time_child(args):
    """Child process: one timed window of the "guided" and "stitched" arms of every --clearance cell on another build's library"""
    from afm import ffi
    ffi._LIB_PATH = os.path.abspath(args.time_child)
    for name in LONG_SCENE_NEW:
        ffi.EXPORTS.pop(name, None)
    model, cfg, dev = _setup()
    out = {}
    for key, d, loop, G, B, kw, x_T, st in _cells(model, cfg, dev):
        arms = _clear_arms(args, model, loop, B, kw, x_T, st, G, dev)
        for arm in ("guided", "stitched"):
            if arm in arms:
                fn = arms[arm]
                fn()
                fn()
                out[f"{key}/{arm}"] = _timed(fn, max(1, math.ceil(MIN_WINDOW_S / _timed(fn))))
    print("CHILD " + json.dumps(out), flush=True)


def clearance_kernel(args):
    """only gradient evaluations of the term on --groups long motions (a kernel trace reads the kernels' own times)"""
    from afm import synth
    from afm.diffusion import Stitch
    dev = torch.device("cuda:0")
    st, G = Stitch(S, OV, length=L), args.groups
    guide = _long_guide(st, G, None, args.repr, dev, clearance=True)
    x = st.windows_of(synth.gaussian(f"bench_long_clear_x_{G}", (G, st.full(L), D)).to(dev), L)
    kw = dict(c_pc_xyz=synth.scene_cloud(G * S, N).to(dev))
    t = torch.zeros(G * S, dtype=torch.int64, device=dev)
    for _ in range(args.calls):
        g = guide(x, t, **kw)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "bench_stitch --clearance --kernel", "repr": args.repr, "G": G, "S": S, "L": L, "F": st.full(L), "K": CLEAR_K, "N": N,
                      "calls": args.calls, "pairs_per_call": G * S * L * CLEAR_K * N, "finite": bool(torch.isfinite(g).all()), "nonzero": bool(g.any())}))


def clearance_main(args):
    model, cfg, dev = _setup()
    what = f"{args.guided} + clearance" if args.guided else "clearance alone"
    out = {"clearance": what, "repr": args.repr, "shape": {"S": S, "L": L, "overlap": OV, "N": N, "D": D, "K": CLEAR_K, "radius": CLEAR_RADIUS},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "cells": {}}
    cells = list(_cells(model, cfg, dev))
    arms, calls, ts, finite, launches, parent = {}, {}, {}, {}, {}, {}
    for key, d, loop, G, B, kw, x_T, st in cells:
        out["shape"]["frames"] = st.full(L)
        arms[key] = _clear_arms(args, model, loop, B, kw, x_T, st, G, dev)
        for arm, fn in arms[key].items():
            fn()
            last = fn()
            calls[key, arm], ts[key, arm] = max(1, math.ceil(MIN_WINDOW_S / _timed(fn))), []
            if arm == "clearance":
                finite[key] = bool(torch.isfinite(last).all())
        if G == GROUPS[0]:          # the launch count, per sub-batch: taken where the chain is one sub-batch
            launches[key.split("/")[0]] = (_kernel_count(arms[key]["clearance"]) - _kernel_count(arms[key]["guided" if args.guided else "stitched"])) / d.num_timesteps
    for _ in range(args.reps):
        if args.parent_lib:          # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            cmd = [sys.executable, os.path.abspath(__file__), "--time-child", args.parent_lib, "--clearance", "--repr", args.repr]
            r = subprocess.run(cmd + (["--guided", args.guided] if args.guided else []), capture_output=True, text=True, cwd=ROOT, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"the parent library's child failed ({r.returncode}): {r.stderr[-800:]}")
            for k, v in json.loads(line[0][6:]).items():
                parent.setdefault(k, []).append(v)
        for key, *_ in cells:          # alternated: a drift of the chip's clocks lands on every arm
            for arm, fn in arms[key].items():
                ts[key, arm].append(_timed(fn, calls[key, arm]))
    for key, d, loop, G, B, kw, x_T, st in cells:
        steps = d.num_timesteps
        cell = {arm: _stats(ts[key, arm], steps, G) for arm in arms[key]}
        for arm in ("guided", "stitched"):
            if f"{key}/{arm}" in parent:
                cell[f"parent_{arm}"] = _stats(parent[f"{key}/{arm}"], steps, G)
                cell[f"{arm}_over_parent"] = round(statistics.median(ts[key, arm]) / statistics.median(parent[f"{key}/{arm}"]), 4)
        base = "guided" if args.guided else "stitched"
        cell["steps"], cell["rows"], cell["finite"] = steps, B, finite[key]
        cell["clearance_over_" + base] = round(statistics.median(ts[key, "clearance"]) / statistics.median(ts[key, base]), 4)
        cell["added_ms_per_step"] = round((statistics.median(ts[key, "clearance"]) - statistics.median(ts[key, base])) * 1e3 / steps, 4)
        cell["added_launches_per_guided_step"] = launches[key.split("/")[0]]
        out["cells"][key] = cell
        print(f"[long clearance bench] {key}: {cell}", flush=True)
    if args.md:
        f = out["shape"]["frames"]
        lines = [f"## {what}, `{args.repr}`: S = {S}, L = {L}, ov = {OV} ({f} frames), N = {N}, K = {CLEAR_K}, radius {CLEAR_RADIUS}, {out['device']}", "",
                 f"`tools/bench_stitch.py --clearance{' --guided ' + args.guided if args.guided else ''} --repr {args.repr}`, {args.reps} repetitions, the arms "
                 "alternated inside every repetition, a timed window = the loop calls that fill 100 ms; ms per long motion (median; spread = (max - min) / median, %).  "
                 f"Every step guided.  Final samples of the clearance arm finite: {all(finite.values())}.", "",
                 "| sampler | G | rows | steps | arm | ms / long motion | ms / step | spread % |", "|---|---|---|---|---|---|---|---|"]
        for key, c in out["cells"].items():
            s_, g = key.split("/G")
            for arm in ("stitched", "parent_stitched", "guided", "parent_guided", "clearance"):
                if arm in c:
                    lines.append(f"| {s_} | {g} | {c['rows']} | {c['steps']} | {arm} | {c[arm]['ms_per_long_motion']} | {c[arm]['ms_per_step']} | {c[arm]['spread_pct']} |")
        base = "guided" if args.guided else "stitched"
        lines += ["", f"| sampler | G | clearance / {base} | added ms / step | added launches / guided step and sub-batch (counted at G = 1) | stitched / parent's | guided / parent's |",
                  "|---|---|---|---|---|---|---|"]
        for key, c in out["cells"].items():
            s_, g = key.split("/G")
            lines.append(f"| {s_} | {g} | {c['clearance_over_' + base]} | {c['added_ms_per_step']} | {c['added_launches_per_guided_step']:g} | "
                         f"{c.get('stitched_over_parent', 'n/a')} | {c.get('guided_over_parent', 'n/a')} |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "a") as fh:
            fh.write("\n".join(lines) + "\n\n")
    print(json.dumps(out))
    return 0 if all(finite.values()) else 1


def guided_main(args):
    model, cfg, dev = _setup()
    out = {"guided": args.guided, "repr": args.repr, "shape": {"S": S, "L": L, "overlap": OV, "N": N, "D": D},
           "device": torch.cuda.get_device_name(0), "cells": {}}
    hashes, launches = {}, {}
    for key, d, loop, G, B, kw, x_T, st in _cells(model, cfg, dev):
        out["shape"]["frames"] = st.full(L)
        steps = d.num_timesteps
        guide = _long_guide(st, G, args.guided, args.repr, dev)
        arms = {"guided": lambda: loop(model, (B, L, D), noise=x_T, clip_denoised=False, cond_fn=guide, model_kwargs=kw, stitch=st),
                "stitched": lambda: loop(model, (B, L, D), noise=x_T, clip_denoised=False, model_kwargs=kw, stitch=st)}
        calls = {}
        for arm, fn in arms.items():
            fn()
            fn()
            calls[arm] = max(1, math.ceil(MIN_WINDOW_S / _timed(fn)))
        hashes[key] = _sha(arms["stitched"]())
        ts = {arm: [] for arm in arms}
        for _ in range(args.reps):
            for arm, fn in arms.items():
                ts[arm].append(_timed(fn, calls[arm]))
        cell = {arm: _stats(ts[arm], steps, G) for arm in arms}
        cell["steps"], cell["rows"] = steps, B
        cell["guided_over_stitched"] = round(statistics.median(ts["guided"]) / statistics.median(ts["stitched"]), 4)
        # the launch count, per sub-batch: taken where the chain is one sub-batch (G = 1; the profiler drops events of the long G = 8 chains)
        if G == GROUPS[0]:
            launches[key.split("/")[0]] = (_kernel_count(arms["guided"]) - _kernel_count(arms["stitched"])) / steps
        cell["gradient_launches_per_guided_step"] = launches[key.split("/")[0]]
        out["cells"][key] = cell
        print(f"[long guidance bench] {key}: {cell}", flush=True)
    if args.parent_lib:
        del model
        torch.cuda.empty_cache()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hash-child", args.parent_lib], capture_output=True, text=True, cwd=ROOT, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"the parent's chain failed ({r.returncode}): {r.stderr[-800:]}")
        parent = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        out["unguided_chain_equals_parent"] = {k: parent.get(k) == v for k, v in hashes.items()}
        print(f"[long guidance bench] unguided stitched chain, this build == parent's library: {out['unguided_chain_equals_parent']}", flush=True)
    if args.md:
        lines = [f"# Guided stitched long motions ({args.guided}, {args.repr}): S = {S}, L = {L}, ov = {OV} ({out['shape']['frames']} frames), "
                 f"N = {N}, {out['device']}", "",
                 "Every step guided; both arms alternated in one call, median of the timed windows.", "",
                 "| sampler | G | rows | steps | guided ms / long motion | unguided stitched ms / long motion | guided / unguided | gradient launches / guided step and sub-batch (counted at G = 1) | spread % (guided, unguided) |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for key, c in out["cells"].items():
            s_, g = key.split("/G")
            lines.append(f"| {s_} | {g} | {c['rows']} | {c['steps']} | {c['guided']['ms_per_long_motion']} | {c['stitched']['ms_per_long_motion']} | "
                         f"{c['guided_over_stitched']} | {c['gradient_launches_per_guided_step']:g} | {c['guided']['spread_pct']}, {c['stitched']['spread_pct']} |")
        if "unguided_chain_equals_parent" in out:
            same = out["unguided_chain_equals_parent"]
            lines += ["", "The unguided stitched chain of every cell, this build against the parent commit's library in a fresh process (sha256 of "
                      f"the result): {'bit-identical in every cell' if all(same.values()) else 'DIFFERS: ' + str(same)}."]
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=None)
    ap.add_argument("--bench-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--hash-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--guided", choices=("contact", "targets", "both"), default=None)
    ap.add_argument("--repr", choices=("pos", "h3d"), default="h3d")
    ap.add_argument("--clearance", action="store_true")
    ap.add_argument("--kernel", action="store_true", help="with --clearance: only gradient evaluations of the term, for a kernel trace")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--time-child", default=None, help=argparse.SUPPRESS)
    args, rest = ap.parse_known_args()
    if args.bench_child:
        sys.argv = [os.path.join(ROOT, "bench.py")] + rest
        return bench_child(args.bench_child)
    if args.hash_child:
        return hash_child(args.hash_child)
    if args.time_child:
        return time_child(args)
    if args.clearance:
        return clearance_kernel(args) if args.kernel else clearance_main(args)
    if args.guided:
        return guided_main(args)

    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    from afm.diffusion import Impute, Stitch
    dev = torch.device("cuda:0")
    cfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263",
                                                                                "model.text_model.max_length=20", "diffusion.steps=1000",
                                                                                f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg("ddim50"), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    st = Stitch(S, OV, length=L)
    out = {"shape": {"S": S, "L": L, "overlap": OV, "frames": st.full(L), "N": N, "D": D}, "device": torch.cuda.get_device_name(0), "cells": {}}
    for name, (resp, kind) in SAMPLERS.items():
        d = create_gaussian_diffusion(cfg(resp))
        steps = d.num_timesteps
        loop = d.ddim_sample_loop if kind == "ddim" else d.dpm_solver_sample_loop
        for G in GROUPS:
            B = G * S
            kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev),
                      c_pc_contact=synth.contact_map(B, N).to(dev), x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev))
            x_T = st.x_T(B, L, D, dev, 1)
            nothing = Impute(torch.zeros(B, L, D, device=dev), torch.zeros(B, L, D, dtype=torch.bool, device=dev))
            arms = {"stitched": lambda: loop(model, (B, L, D), noise=x_T, clip_denoised=False, model_kwargs=kw, stitch=st),
                    "imputing_form": lambda: loop(model, (B, L, D), noise=x_T, clip_denoised=False, denoised_fn=nothing, model_kwargs=kw)}
            calls = {}
            for arm, fn in arms.items():          # warm-up (weight packs, condition tokens, workspaces, rows), then the calls per window
                fn()
                fn()
                calls[arm] = max(1, math.ceil(MIN_WINDOW_S / _timed(fn)))
            ts = {arm: [] for arm in arms}
            for _ in range(args.reps):             # alternated: a drift of the chip's clocks lands on both arms
                for arm, fn in arms.items():
                    ts[arm].append(_timed(fn, calls[arm]))
            cell = {arm: _stats(ts[arm], steps, G) for arm in arms}
            cell["steps"], cell["rows"] = steps, B
            cell["stitched_over_imputing_form"] = round(statistics.median(ts["stitched"]) / statistics.median(ts["imputing_form"]), 4)
            out["cells"][f"{name}/G{G}"] = cell
            print(f"[stitch bench] {name} G={G}: {cell}", flush=True)
    if args.parent_lib:
        this, parent = [], []
        for _ in range(args.bench_rounds):
            this.append(_bench_once(None, args.bench_steps))
            parent.append(_bench_once(args.parent_lib, args.bench_steps))
        spread = lambda v: round(100.0 * (max(v) - min(v)) / statistics.median(v), 2)
        out["bench_py"] = {"steps_per_s_this": this, "steps_per_s_parent": parent, "median_this": statistics.median(this),
                           "median_parent": statistics.median(parent), "this_over_parent": round(statistics.median(this) / statistics.median(parent), 4),
                           "spread_pct_this": spread(this), "spread_pct_parent": spread(parent)}
        print(f"[stitch bench] bench.py: {out['bench_py']}", flush=True)
    if args.md:
        lines = [f"# Stitched long motions: S = {S}, L = {L}, ov = {OV} ({st.full(L)} frames), N = {N}, {out['device']}", "",
                 "| sampler | G | rows | steps | stitched ms / long motion | stitched ms / step | imputing-form ms / step | stitched / imputing-form | spread % (stitched, imputing-form) |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for key, c in out["cells"].items():
            s, g = key.split("/G")
            lines.append(f"| {s} | {g} | {c['rows']} | {c['steps']} | {c['stitched']['ms_per_long_motion']} | {c['stitched']['ms_per_step']} | "
                         f"{c['imputing_form']['ms_per_step']} | {c['stitched_over_imputing_form']} | {c['stitched']['spread_pct']}, {c['imputing_form']['spread_pct']} |")
        if "bench_py" in out:
            b = out["bench_py"]
            lines += ["", f"`bench.py --gpus 1 --steps {args.bench_steps} --warmup 20`, this build and the parent's library alternated in fresh processes:", "",
                      f"* this build: {b['steps_per_s_this']} steps/s (median {b['median_this']}, spread {b['spread_pct_this']} %)",
                      f"* parent: {b['steps_per_s_parent']} steps/s (median {b['median_parent']}, spread {b['spread_pct_parent']} %)",
                      f"* this / parent = {b['this_over_parent']}"]
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
