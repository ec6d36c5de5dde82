"""Cost of scene-clearance guidance in the CMDM's sampling loops on one MI355X, printed as ONE JSON line (and as a markdown table with --md).

    python tools/bench_clearance.py [--reps 5] [--parent-lib PATH] [--md PATH]
    python tools/bench_clearance.py --kernel [--repr pos|h3d] [--batch 32] [--calls 20]

L = 196, N = 8192 scene points, K = 16 joints, radius 0.5, the benchmark's synthetic weights, at B = 1 and at B = 32, for DDIM (eta = 0) at
"ddim50" and DPM-Solver++(2M) at "logsnr20", on absolute-position columns (pos) and on HumanML3D features (h3d).  Arms, ms per sample call
(the loop call and the final synchronise):

    unguided          the native loop without a cond_fn
    clearance_pos     the same loop with a SceneClearance on 16 column triples as cond_fn (afm_cmdm_scene_guide_loop_range; one launch a step)
    clearance_h3d     with SceneClearance.h3d on 16 joints and the y-up to z-up transform (three launches: recovery, clearance, adjoint)
    parent            --parent-lib: the unguided loop of a libafm_hip.so built from the parent commit, in a fresh child process

and the ratios guided / unguided and this build's unguided / the parent's.  Timing follows tools/bench_contact_guidance.py: a timed window
is as many back-to-back loop calls as fill 100 ms, the arms alternate inside every repetition, every repetition is kept (median, best,
spread), the parent's child process runs between the repetitions of this one.

--kernel runs nothing but `--calls` gradient evaluations of the clearance at one batch size, for a kernel trace of their own: the
clearance kernel's time per call gives pair evaluations per second, B * L * K * N pairs a call.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_contact_guidance as base          # noqa: E402

L, N, D, K = base.L, base.N, base.D, 16
RADIUS, SCALE = 0.5, 1e-3          # a small scale: the synthetic model's samples stay finite (every guided arm's final sample is checked)
NEW_SCENE = ("afm_scene_guidance", "afm_scene_guidance_workspace_bytes", "afm_cmdm_scene_guide_loop_range",
             "afm_cmdm_scene_guide_loop_workspace_bytes")


def _guides(dev):
    from afm.diffusion import SceneClearance
    mean, std = torch.zeros(D), torch.ones(D)
    zup = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]], device=dev)
    return {"clearance_pos": SceneClearance([3 * j for j in range(K)], mean, std, radius=RADIUS, scale=SCALE),
            "clearance_h3d": SceneClearance.h3d(list(range(K)), mean, std, radius=RADIUS, to_scene=zup, scale=SCALE)}


def worker(lib, reps):
    """Child process: the unguided loops of the parent build's library (it has none of the scene entry points)"""
    from afm import ffi
    for name in NEW_SCENE:
        ffi.EXPORTS.pop(name, None)
    ffi._LIB_PATH = os.path.abspath(lib)
    dev = torch.device("cuda:0")
    model, diffs, kws = base._setup(dev)
    out = {}
    for b in base.BATCHES:
        for s in base.SAMPLERS:
            run = base._runner(model, diffs, kws, s, b)
            n = base._calls(run)
            model.condition_tokens(**kws[b])
            out[f"{s}/{b}"] = [base._timed(run, n) for _ in range(reps)]
    print("WORKER " + json.dumps(out), flush=True)


def kernel_only(args):
    dev = torch.device("cuda:0")
    from afm import synth
    b = args.batch
    guide = _guides(dev)["clearance_" + args.repr]
    x = synth.gaussian(f"bench_clear_x_{b}", (b, L, D)).to(dev)
    kw = dict(c_pc_xyz=synth.scene_cloud(b, N).to(dev))
    t = torch.zeros(b, dtype=torch.int64, device=dev)
    for _ in range(args.calls):
        g = guide(x, t, **kw)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "bench_clearance --kernel", "repr": args.repr, "B": b, "L": L, "K": K, "N": N, "calls": args.calls,
                      "pairs_per_call": b * L * K * N, "finite": bool(torch.isfinite(g).all()), "nonzero": bool(g.any())}))
    return 0


def _markdown(out):
    lines = ["# Scene-clearance guidance in the CMDM sampling loops", "",
             f"`tools/bench_clearance.py`, {out['device']}, L = {L}, N = {N}, K = {K}, radius {RADIUS}, {out['reps']} repetitions, arms alternating inside "
             "every repetition, a timed window = the loop calls that fill 100 ms.  ms per sample call of the motion stage (median; spread = "
             f"(max - min) / median).  Every guided arm's final sample finite: {all(out['finite'].values())}.", "",
             "| sampler | B | arm | ms / call | ms / step | spread |", "|---|---|---|---|---|---|"]
    for s in base.SAMPLERS:
        for b in base.BATCHES:
            for arm, v in out[s][f"B{b}"].items():
                if isinstance(v, dict):
                    lines.append(f"| {s} | {b} | {arm} | {v['ms_per_sample_call']} | {v['ms_per_step']} | {v['spread']} |")
    lines += ["", "| sampler | B | pos guided / unguided | h3d guided / unguided | unguided / parent unguided |", "|---|---|---|---|---|"]
    for s in base.SAMPLERS:
        for b in base.BATCHES:
            o = out[s][f"B{b}"]
            lines.append(f"| {s} | {b} | {o['pos_over_unguided']} | {o['h3d_over_unguided']} | {o.get('unguided_over_parent', 'n/a')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    ap.add_argument("--kernel", action="store_true", help="only gradient evaluations of the clearance, for a kernel trace")
    ap.add_argument("--repr", choices=("pos", "h3d"), default="pos")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps)
    if args.kernel:
        return kernel_only(args)
    dev = torch.device("cuda:0")
    model, diffs, kws = base._setup(dev)
    guides = _guides(dev)
    arms = {"unguided": None, **guides}
    runs = {(s, b, arm): base._runner(model, diffs, kws, s, b, guide=g) for s in base.SAMPLERS for b in base.BATCHES for arm, g in arms.items()}
    calls = {k: base._calls(fn) for k, fn in runs.items()}
    finite = {f"{s}/B{b}/{arm}": bool(torch.isfinite(fn()).all()) for (s, b, arm), fn in runs.items() if arm != "unguided"}
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
        for b in base.BATCHES:
            model.condition_tokens(**kws[b])
            for s in base.SAMPLERS:
                for arm in arms:
                    times[(s, b, arm)].append(base._timed(runs[(s, b, arm)], calls[(s, b, arm)]))
    out = {"tool": "bench_clearance", "device": torch.cuda.get_device_name(0), "L": L, "N": N, "K": K, "reps": args.reps, "finite": finite}
    for s in base.SAMPLERS:
        out[s] = {}
        steps = diffs[s].num_timesteps
        for b in base.BATCHES:
            o = {arm: base._stats(times[(s, b, arm)], steps) for arm in arms}
            ms = lambda arm: o[arm]["ms_per_sample_call"]
            if f"{s}/{b}" in parent:
                o["parent"] = base._stats(parent[f"{s}/{b}"], steps)
                o["unguided_over_parent"] = round(ms("unguided") / ms("parent"), 4)
            o["pos_over_unguided"] = round(ms("clearance_pos") / ms("unguided"), 4)
            o["h3d_over_unguided"] = round(ms("clearance_h3d") / ms("unguided"), 4)
            out[s][f"B{b}"] = o
    print(json.dumps(out))
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(_markdown(out))
    return 0 if all(finite.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
