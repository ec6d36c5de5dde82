"""Classifier-free guided sampling throughput of the CMDM on one MI355X, printed as ONE JSON line.

    python tools/bench_cfg.py [--reps 3] [--scale 2.5] [--parent-lib PATH]

B = 32, L = 196, N = 8192 contact points, the 1000-step DDPM chain and `ddim50` (eta = 0): denoising steps/s of the unguided native loop,
the guided loop (compact unconditioned branch), the guided loop with the masked full-length branch forced and the compact form with the
unconditioned branch on a second stream per sub-batch (four streams), alternating in one process,
every repetition kept (best, and the spread of the repetitions).  --parent-lib: a libafm_hip.so built from the parent commit; its unguided
loop is timed in a fresh child process between the repetitions of this one, so that `guided / parent unguided` comes from one call.
Two full unguided evaluations per step are the trivial implementation: the ratio must be at least 0.5 less the spread.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

B, L, N = 32, 196, 8192
SAMPLERS = {"ddpm1000": ("", None), "ddim50": ("ddim50", 0.0)}


def _setup(dev, lib=None):
    from afm import ffi
    if lib:
        ffi._LIB_PATH = os.path.abspath(lib)          # (before the first load(): the library of another build, unguided loop only -
        for name in [n for n in ffi.EXPORTS if "_cfg_" in n]:      # a parent build has none of the guided entry points)
            del ffi.EXPORTS[name]
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    cfgs = {k: load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263", "model.text_model.max_length=20",
                                                                        "diffusion.steps=1000", f"diffusion.timestep_respacing='{resp}'"])
            for k, (resp, _) in SAMPLERS.items()}
    model = create_model(cfgs["ddpm1000"], device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    diffs = {k: create_gaussian_diffusion(c) for k, c in cfgs.items()}
    kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev),
              c_pc_contact=synth.contact_map(B, N).to(dev), x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev))
    return model, diffs, kw


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _runner(diffs, kw, sampler, den):
    d, (_, eta) = diffs[sampler], SAMPLERS[sampler]
    if eta is None:
        return lambda: d.p_sample_loop(den, (B, L, 263), clip_denoised=False, model_kwargs=kw, seed=1)
    return lambda: d.ddim_sample_loop(den, (B, L, 263), clip_denoised=False, model_kwargs=kw, eta=eta, seed=1)


def worker(lib, reps):
    """Child process: the unguided loop of another build's library, `reps` timed runs per sampler -> one JSON line of seconds."""
    dev = torch.device("cuda:0")
    model, diffs, kw = _setup(dev, lib)
    out = {}
    for s in SAMPLERS:
        run = _runner(diffs, kw, s, model)
        run()
        out[s] = [_timed(run) for _ in range(reps)]
    print("WORKER " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=2.5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps)
    dev = torch.device("cuda:0")
    model, diffs, kw = _setup(dev)
    from afm.cmdm import GuidedCMDM
    dens = {"unguided": model, "guided_compact": GuidedCMDM(model, args.scale), "guided_masked": GuidedCMDM(model, args.scale, force_masked=True),
            "guided_compact_branch_streams": GuidedCMDM(model, args.scale, branch_streams=True)}
    times = {s: {k: [] for k in dens} for s in SAMPLERS}
    parent = {s: [] for s in SAMPLERS}
    for s in SAMPLERS:                                        # warm-up: weight packs, workspaces, rows
        for den in dens.values():
            _runner(diffs, kw, s, den)()
    for _ in range(args.reps):
        if args.parent_lib:                                   # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "1"], capture_output=True,
                               text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            for s, ts in json.loads(line[0][7:]).items():
                parent[s] += ts
        for s in SAMPLERS:
            for k, den in dens.items():
                times[s][k].append(_timed(_runner(diffs, kw, s, den)))
    out = {"tool": "bench_cfg", "device": torch.cuda.get_device_name(0), "B": B, "L": L, "scale": args.scale, "reps": args.reps}
    for s in SAMPLERS:
        n = diffs[s].num_timesteps
        rate = lambda ts: [round(n / t, 2) for t in ts]
        o = {k: {"steps_per_s": max(rate(ts)), "all": rate(ts)} for k, ts in times[s].items()}
        ung = o["unguided"]["all"]
        o["unguided_spread"] = round((max(ung) - min(ung)) / max(ung), 4)
        base = o["unguided"]["steps_per_s"]
        if parent[s]:
            o["parent_unguided"] = {"steps_per_s": max(rate(parent[s])), "all": rate(parent[s])}
            base = o["parent_unguided"]["steps_per_s"]
            o["unguided_over_parent"] = round(o["unguided"]["steps_per_s"] / base, 4)
        for k in ("guided_compact", "guided_masked", "guided_compact_branch_streams"):
            o[k + "_over_unguided"] = round(o[k]["steps_per_s"] / base, 4)
        o["compact_over_masked"] = round(o["guided_compact"]["steps_per_s"] / o["guided_masked"]["steps_per_s"], 4)
        out[s] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()
