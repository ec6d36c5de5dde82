"""Time per sample and per step of the CMDM's deterministic samplers on one MI355X, printed as ONE JSON line.

    python tools/bench_samplers.py [--reps 5] [--parent-lib PATH]

L = 196, N = 8192 contact points, the benchmark's synthetic weights, at B = 1 and at B = 32: ddim_sample_loop(eta = 0) at "ddim50" against
dpm_solver_sample_loop (DPM-Solver++(2M)) at "logsnr20" and "logsnr10".  A timed run is the loop call and the final synchronise; the
condition tokens of the batch are computed before its arms (the model holds one set: CMDM.condition_tokens), so that no arm pays for
them.  The arms alternate inside every repetition; every repetition is kept (the
median, the best and the spread (max - min) / median of each arm).  --parent-lib: a libafm_hip.so built from the parent commit; its
"ddim50" loop is timed in a fresh child process between the repetitions of this one, so that the per-step figures of this build can be
compared with the parent's DDIM loop inside one call.

The expectation the figures are read against: a 2M step is a DDIM step plus one [B, L, D] read and one write in the update launch.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

L, N = 196, 8192
BATCHES = (1, 32)
ARMS = {"ddim50": ("ddim50", "ddim"), "dpm2m_logsnr20": ("logsnr20", "dpm"), "dpm2m_logsnr10": ("logsnr10", "dpm")}


def _setup(dev, lib=None):
    from afm import ffi
    if lib:
        ffi._LIB_PATH = os.path.abspath(lib)          # (before the first load(): the library of another build, its DDIM loop only -
        for name in [n for n in ffi.EXPORTS if "_dpm_" in n]:      # a parent build has none of the 2M entry points)
            del ffi.EXPORTS[name]
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    cfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263",
                                                                                "model.text_model.max_length=20", "diffusion.steps=1000",
                                                                                f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg("ddim50"), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    diffs = {k: create_gaussian_diffusion(cfg(resp)) for k, (resp, _) in ARMS.items() if not lib or k == "ddim50"}
    kws = {b: dict(c_text_feat=synth.text_feature(b).to(dev), c_pc_xyz=synth.scene_cloud(b, N).to(dev),
                   c_pc_contact=synth.contact_map(b, N).to(dev), x_mask=torch.zeros(b, L, dtype=torch.bool, device=dev)) for b in BATCHES}
    return model, diffs, kws


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _runner(model, diffs, kws, arm, b):
    d, kind = diffs[arm], ARMS[arm][1]
    if kind == "ddim":
        return lambda: d.ddim_sample_loop(model, (b, L, 263), clip_denoised=False, model_kwargs=kws[b], eta=0.0, seed=1)
    return lambda: d.dpm_solver_sample_loop(model, (b, L, 263), clip_denoised=False, model_kwargs=kws[b], seed=1)


def worker(lib, reps):
    """Child process: the "ddim50" loop of another build's library, `reps` timed runs per batch -> one JSON line of seconds."""
    dev = torch.device("cuda:0")
    model, diffs, kws = _setup(dev, lib)
    out = {}
    for b in BATCHES:
        run = _runner(model, diffs, kws, "ddim50", b)
        run()
        run()
        model.condition_tokens(**kws[b])
        out[str(b)] = [_timed(run) for _ in range(reps)]
    print("WORKER " + json.dumps(out), flush=True)


def _stats(ts, steps, b):
    med = statistics.median(ts)
    return {"steps": steps, "ms_per_sample_call": round(1e3 * med, 3), "ms_per_step": round(1e3 * med / steps, 4),
            "best_ms_per_step": round(1e3 * min(ts) / steps, 4), "spread": round((max(ts) - min(ts)) / med, 4),
            "samples_per_s": round(b / med, 2), "all_ms": [round(1e3 * t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps)
    dev = torch.device("cuda:0")
    model, diffs, kws = _setup(dev)
    runs = {(arm, b): _runner(model, diffs, kws, arm, b) for b in BATCHES for arm in ARMS}
    for fn in runs.values():                                  # warm-up: weight packs, condition tokens, workspaces, rows
        fn()
        fn()
    times = {k: [] for k in runs}
    parent = {b: [] for b in BATCHES}
    for _ in range(args.reps):
        if args.parent_lib:                                   # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "1"], capture_output=True,
                               text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            for b, ts in json.loads(line[0][7:]).items():
                parent[int(b)] += ts
        for b in BATCHES:
            model.condition_tokens(**kws[b])
            for arm in ARMS:
                times[(arm, b)].append(_timed(runs[(arm, b)]))
    out = {"tool": "bench_samplers", "device": torch.cuda.get_device_name(0), "L": L, "reps": args.reps}
    for b in BATCHES:
        o = {arm: _stats(times[(arm, b)], diffs[arm].num_timesteps, b) for arm in ARMS}
        if parent[b]:
            o["parent_ddim50"] = _stats(parent[b], diffs["ddim50"].num_timesteps, b)
        base = o["ddim50"]["ms_per_step"]
        for arm in ARMS:
            if arm != "ddim50":
                o[arm + "_step_over_ddim_step"] = round(o[arm]["ms_per_step"] / base, 4)
                o[arm + "_sample_over_ddim_sample"] = round(o[arm]["ms_per_sample_call"] / o["ddim50"]["ms_per_sample_call"], 4)
        out[f"B{b}"] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()
