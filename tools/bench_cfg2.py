"""Two-scale guided sampling throughput of the CMDM (one scale per condition) on one MI355X, printed as ONE JSON line.

    python tools/bench_cfg2.py [--reps 3] [--scale 2.5] [--scale-pc 1.5] [--scale-text 5.0] [--parent-lib PATH]

The workload of tools/bench_cfg.py (B = 32, L = 196, N = 8192 contact points, the 1000-step DDPM chain and `ddim50`, eta = 0): denoising
steps/s of the unguided native loop, the single-scale guided loop (compact unconditioned branch) and the two-scale loop (pc first),
alternating in one process, every repetition kept.  --parent-lib: a libafm_hip.so built from the parent commit; its unguided AND
single-scale guided loops (and its two-scale loop, if it exports one) are timed in a fresh child process between the repetitions of this one, so that `two-scale / parent unguided`
and the no-regression ratios come from one call.  Three full unguided evaluations per step are the trivial implementation: the ratio
must be at least 1/3 less the spread of the unguided repetitions; by GEMM rows the ideal is 326 / (326 + 326 + 197) = 0.38.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_cfg as bc  # noqa: E402  (the skeleton: _setup, _timed, _runner, the workload constants)


def worker(lib, reps, scale, scale_pc, scale_text):
    """Child process: the unguided and single-scale guided loops of another build's library, and its two-scale loop if it has one
    -> one JSON line of seconds."""
    import ctypes
    from afm import ffi
    ffi._LIB_PATH = os.path.abspath(lib)                          # (before the first load(): the library of another build)
    has = ctypes.CDLL(ffi._LIB_PATH)
    two = all(hasattr(has, n) for n in ffi.EXPORTS if "cfg2" in n)
    for name in [n for n in ffi.EXPORTS if "cfg2" in n and not two]:         # a build from before the two-scale entry points
        del ffi.EXPORTS[name]
    model, diffs, kw = bc._setup(torch.device("cuda:0"))
    from afm.cmdm import GuidedCMDM
    dens = {"unguided": model, "guided_compact": GuidedCMDM(model, scale)}
    if two:
        dens["two_scale"] = GuidedCMDM(model, {"pc": scale_pc, "text": scale_text})
    out = {s: {k: [] for k in dens} for s in bc.SAMPLERS}
    for s in bc.SAMPLERS:                                         # warm-up, then alternating like the parent process does
        for den in dens.values():
            bc._runner(diffs, kw, s, den)()
    for _ in range(reps):
        for s in bc.SAMPLERS:
            for k, den in dens.items():
                out[s][k].append(bc._timed(bc._runner(diffs, kw, s, den)))
    print("WORKER " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=2.5)
    ap.add_argument("--scale-pc", type=float, default=1.5)
    ap.add_argument("--scale-text", type=float, default=5.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps, args.scale, args.scale_pc, args.scale_text)
    dev = torch.device("cuda:0")
    model, diffs, kw = bc._setup(dev)
    from afm.cmdm import GuidedCMDM
    dens = {"unguided": model, "guided_compact": GuidedCMDM(model, args.scale),
            "two_scale": GuidedCMDM(model, {"pc": args.scale_pc, "text": args.scale_text})}
    times = {s: {k: [] for k in dens} for s in bc.SAMPLERS}
    parent = {s: {} for s in bc.SAMPLERS}
    for s in bc.SAMPLERS:                                         # warm-up: weight packs, workspaces, rows
        for den in dens.values():
            bc._runner(diffs, kw, s, den)()
    for _ in range(args.reps):
        if args.parent_lib:                                       # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "1", "--scale", str(args.scale),
                                "--scale-pc", str(args.scale_pc), "--scale-text", str(args.scale_text)],
                               capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            for s, by in json.loads(line[0][7:]).items():
                for k, ts in by.items():
                    parent[s].setdefault(k, []).extend(ts)
        for s in bc.SAMPLERS:
            for k, den in dens.items():
                times[s][k].append(bc._timed(bc._runner(diffs, kw, s, den)))
    out = {"tool": "bench_cfg2", "device": torch.cuda.get_device_name(0), "B": bc.B, "L": bc.L, "scale": args.scale,
           "scales": {"pc": args.scale_pc, "text": args.scale_text}, "reps": args.reps}
    for s in bc.SAMPLERS:
        n = diffs[s].num_timesteps
        rate = lambda ts: [round(n / t, 2) for t in ts]
        o = {k: {"steps_per_s": max(rate(ts)), "all": rate(ts)} for k, ts in times[s].items()}
        ung = o["unguided"]["all"]
        o["unguided_spread"] = round((max(ung) - min(ung)) / max(ung), 4)
        base = o["unguided"]["steps_per_s"]
        if parent[s]:
            for k, ts in parent[s].items():
                o["parent_" + k] = {"steps_per_s": max(rate(ts)), "all": rate(ts)}
                o[k + "_over_parent"] = round(o[k]["steps_per_s"] / o["parent_" + k]["steps_per_s"], 4)
            base = o["parent_unguided"]["steps_per_s"]
        o["two_scale_over_unguided"] = round(o["two_scale"]["steps_per_s"] / base, 4)
        o["two_scale_over_guided_compact"] = round(o["two_scale"]["steps_per_s"] / o["guided_compact"]["steps_per_s"], 4)
        o["floor"] = round(1 / 3 - o["unguided_spread"], 4)
        o["floor_held"] = o["two_scale_over_unguided"] >= o["floor"]
        out[s] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()
