"""Cost of foot-grounding guidance in the CMDM's sampling loops on one MI355X, printed as ONE JSON line (and as a markdown table with --md).

    python tools/bench_grounding.py [--reps 5] [--md profiles/grounding_bench.md]
    python tools/bench_grounding.py --kernel [--repr pos|h3d] [--batch 32] [--calls 20]

L = 196, K = 4 joints (the feet: 7, 10, 8, 11), floor 0, height 0.05, the benchmark's synthetic weights, at B = 1 and at B = 32, for DDIM
(eta = 0) at "ddim50" and DPM-Solver++(2M) at "logsnr20", on absolute-position columns (pos) and on HumanML3D features (h3d).  Arms, ms per
sample call (the loop call and the final synchronise):

    unguided          the native loop without a cond_fn
    grounding_pos     the same loop with a FootGrounding on 4 column triples as cond_fn (afm_cmdm_ground_guide_loop_range; one launch a step)
    grounding_h3d     with FootGrounding.h3d on the 4 foot joints and the y-up to z-up transform (three launches: recovery, grounding, adjoint)
    targets_pos / targets_h3d     a JointTargets on the same joints, every second frame weighted (afm_cmdm_motion_guide_loop_range): the
                                  term of the same class (B x L x K items) the grounding is reported next to

and per cell the ratios guided / unguided and the added cost per step of the grounding over the targets'.  Timing follows
tools/bench_contact_guidance.py: a timed window is as many back-to-back loop calls as fill 100 ms, the arms alternate inside every
repetition, every repetition is kept (median, best, spread).

--kernel runs nothing but `--calls` gradient evaluations of the grounding at one batch size, for a kernel trace of their own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_contact_guidance as base          # noqa: E402

L, D = base.L, base.D
FEET = [7, 10, 8, 11]
K = len(FEET)
FLOOR, HEIGHT, SCALE = 0.0, 0.05, 1e-3          # a small scale: the synthetic model's samples stay finite (every guided arm's final sample is checked)


def _guides(dev, b):
    from afm import synth
    from afm.diffusion import FootGrounding, JointTargets
    mean, std = torch.zeros(D), torch.ones(D)
    zup = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]], device=dev)
    cols = [3 * j for j in FEET]
    target = 1.5 * synth.gaussian(f"bench_ground_targets_{b}", (b, L, K, 3))
    weight = torch.zeros(b, L, K)
    weight[:, ::2] = 0.01
    own = dict(floor=FLOOR, height=HEIGHT, scale=SCALE)
    return {"grounding_pos": FootGrounding(cols, mean, std, **own),
            "grounding_h3d": FootGrounding.h3d(FEET, mean, std, to_scene=zup, **own),
            "targets_pos": JointTargets(cols, mean, std, target=target, weight=weight, scale=SCALE),
            "targets_h3d": JointTargets.h3d(FEET, mean, std, to_scene=zup, target=target, weight=weight, scale=SCALE)}


def kernel_only(args):
    dev = torch.device("cuda:0")
    from afm import synth
    b = args.batch
    guide = _guides(dev, b)["grounding_" + args.repr]
    x = synth.gaussian(f"bench_ground_x_{b}", (b, L, D)).to(dev)
    t = torch.zeros(b, dtype=torch.int64, device=dev)
    for _ in range(args.calls):
        g = guide(x, t)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "bench_grounding --kernel", "repr": args.repr, "B": b, "L": L, "K": K, "calls": args.calls,
                      "items_per_call": b * L * K, "finite": bool(torch.isfinite(g).all()), "nonzero": bool(g.any())}))
    return 0


def _markdown(out):
    lines = ["# Foot-grounding guidance in the CMDM sampling loops", "",
             f"`tools/bench_grounding.py`, {out['device']}, L = {L}, K = {K}, floor {FLOOR}, height {HEIGHT}, {out['reps']} repetitions, arms "
             "alternating inside every repetition, a timed window = the loop calls that fill 100 ms.  ms per sample call of the motion stage "
             f"(median; spread = (max - min) / median).  Every guided arm's final sample finite: {all(out['finite'].values())}.", "",
             "| sampler | B | arm | ms / call | ms / step | spread |", "|---|---|---|---|---|---|"]
    for s in base.SAMPLERS:
        for b in base.BATCHES:
            for arm, v in out[s][f"B{b}"].items():
                if isinstance(v, dict):
                    lines.append(f"| {s} | {b} | {arm} | {v['ms_per_sample_call']} | {v['ms_per_step']} | {v['spread']} |")
    lines += ["", "Guided / unguided step, and the grounding's added cost per step over the targets' (added = guided - unguided, ms per step):", "",
              "| sampler | B | grounding pos | targets pos | added pos: grounding / targets | grounding h3d | targets h3d | added h3d: grounding / targets |",
              "|---|---|---|---|---|---|---|---|"]
    for s in base.SAMPLERS:
        for b in base.BATCHES:
            o = out[s][f"B{b}"]
            lines.append(f"| {s} | {b} | {o['grounding_pos_over_unguided']} | {o['targets_pos_over_unguided']} | {o['added_pos_grounding_over_targets']} | "
                         f"{o['grounding_h3d_over_unguided']} | {o['targets_h3d_over_unguided']} | {o['added_h3d_grounding_over_targets']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    ap.add_argument("--kernel", action="store_true", help="only gradient evaluations of the grounding, for a kernel trace")
    ap.add_argument("--repr", choices=("pos", "h3d"), default="pos")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if args.kernel:
        return kernel_only(args)
    dev = torch.device("cuda:0")
    model, diffs, kws = base._setup(dev)
    arms = {b: {"unguided": None, **_guides(dev, b)} for b in base.BATCHES}
    names = list(arms[base.BATCHES[0]])
    runs = {(s, b, arm): base._runner(model, diffs, kws, s, b, guide=arms[b][arm]) for s in base.SAMPLERS for b in base.BATCHES for arm in names}
    calls = {k: base._calls(fn) for k, fn in runs.items()}
    finite = {f"{s}/B{b}/{arm}": bool(torch.isfinite(fn()).all()) for (s, b, arm), fn in runs.items() if arm != "unguided"}
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for b in base.BATCHES:
            model.condition_tokens(**kws[b])
            for s in base.SAMPLERS:
                for arm in names:
                    times[(s, b, arm)].append(base._timed(runs[(s, b, arm)], calls[(s, b, arm)]))
    out = {"tool": "bench_grounding", "device": torch.cuda.get_device_name(0), "L": L, "K": K, "reps": args.reps, "finite": finite}
    for s in base.SAMPLERS:
        out[s] = {}
        steps = diffs[s].num_timesteps
        for b in base.BATCHES:
            o = {arm: base._stats(times[(s, b, arm)], steps) for arm in names}
            ms = lambda arm: o[arm]["ms_per_sample_call"]
            for arm in names[1:]:
                o[f"{arm}_over_unguided"] = round(ms(arm) / ms("unguided"), 4)
            for r in ("pos", "h3d"):
                added = (ms(f"grounding_{r}") - ms("unguided")) / max(ms(f"targets_{r}") - ms("unguided"), 1e-9)
                o[f"added_{r}_grounding_over_targets"] = round(added, 3)
            out[s][f"B{b}"] = o
    print(json.dumps(out))
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(_markdown(out))
    return 0 if all(finite.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
