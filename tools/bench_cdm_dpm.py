"""DPM-Solver++(2M) sampling of the CDM Perceiver on one MI355X: the native loop against the step-by-step loop, printed as ONE JSON line.

    python tools/bench_cdm_dpm.py [--reps 5] [--parent-lib PATH]

The shape of BASELINE configs[2]: N = 8192 points, the H3D variant (9 input channels), T = 500, at B = 32 and B = 1, on `logsnr20`
(17 steps on the cosine schedule).  Four arms, alternating inside every repetition, every repetition kept (median, best, spread =
(max - min) / median): the native DDIM loop at eta = 0, the native 2M loop (afm_cdm_dpm_loop_range: update and history fused into
dec_point), the step-by-step 2M loop (dpm_solver_sample_loop_progressive: CDM.forward, a clone and an afm_dpm_step launch per step,
driven from Python - what the library ran before it had the native loop) and the native 2M loop with an Impute that pins every joint
on the first 1024 points.
Pass / fail: the native 2M loop is faster than the step-by-step one at both batch sizes, and its time per step is not above the native
DDIM loop's by more than that arm's own spread in the call.
Also the whole B = 1 job `two_stage_sample(sampler="dpm++")` on `logsnr20` for both stages (N = 8192, L = 196); with --parent-lib (a
libafm_hip.so built from the parent commit, which has no native 2M loop of the CDM) the same job on that library - its contact stage
step by step - in a child process between the repetitions.
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

N, J, L = 8192, 6, 196
BATCHES = (32, 1)
RESP = "logsnr20"
CDM_ONLY = ("afm_cdm_dpm_loop_range", "afm_cdm_dpm_loop_workspace_bytes")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _last(gen):
    out = None
    for out in gen:
        pass
    return out["sample"]


def _models(dev, lib=None):
    from afm import ffi
    if lib:                                       # (before the first load(): a parent build has neither entry of the CDM's 2M loop)
        ffi._LIB_PATH = os.path.abspath(lib)
        for name in CDM_ONLY:
            del ffi.EXPORTS[name]
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    ccfg = lambda resp: load_config("text_to_motion_contact_gen", "cdm",
                                    ["model.arch=Perceiver", "model.scene_model.use_scene_model=False", "model.input_feats=6",
                                     "model.text_model.max_length=20", "diffusion.steps=500", f"diffusion.timestep_respacing='{resp}'"])
    mcfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm",
                                    ["model.data_repr=h3d", "model.input_feats=263", "model.text_model.max_length=20", "diffusion.steps=1000",
                                     f"diffusion.timestep_respacing='{resp}'"])
    cdm = create_model(ccfg(""), device=dev)
    synth.fill_module_(cdm)
    cdm = cdm.to(dev).eval()
    if lib:
        cdm.afm_native_loop = None                # the parent's route: dpm_solver_sample_loop samples the CDM step by step (this worker runs "dpm++" only)
    cmdm = create_model(mcfg(RESP), device=dev)
    synth.fill_module_(cmdm)
    cmdm = cmdm.to(dev).eval()
    return cdm, create_gaussian_diffusion(ccfg(RESP)), cmdm, create_gaussian_diffusion(mcfg(RESP))


def _two_stage(dev, cdm, d_adm, cmdm, d_amdm):
    from afm import synth
    from afm.pipeline import two_stage_sample
    text, xyz = synth.text_feature(1).to(dev), synth.scene_cloud(1, N).to(dev)
    return lambda: two_stage_sample(cdm, d_adm, cmdm, d_amdm, text_feat=text, xyz=xyz, frames=L, sigma=0.8, seed=1, sampler="dpm++")


def worker(lib, reps):
    """Child process: the two-stage job on another build's library, `reps` timed runs -> one JSON line of seconds."""
    dev = torch.device("cuda:0")
    run = _two_stage(dev, *_models(dev, lib))
    run()
    run()
    print("WORKER " + json.dumps([_timed(run) for _ in range(reps)]), flush=True)


def _stats(ts, steps=None):
    med = statistics.median(ts)
    o = {"ms": round(1e3 * med, 3), "best_ms": round(1e3 * min(ts), 3), "spread": round((max(ts) - min(ts)) / med, 4),
         "all_ms": [round(1e3 * t, 3) for t in ts]}
    if steps:
        o["ms_per_step"] = round(1e3 * med / steps, 4)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps)
    dev = torch.device("cuda:0")
    from afm import synth
    from afm.diffusion import Impute
    cdm, d_adm, cmdm, d_amdm = _models(dev)
    steps = d_adm.num_timesteps
    runs = {}
    for b in BATCHES:
        kw = dict(c_text_feat=synth.text_feature(b).to(dev), c_pc_xyz=synth.scene_cloud(b, N).to(dev))
        mask = torch.zeros(b, N, J, dtype=torch.bool)
        mask[:, :1024] = True
        imp = Impute(synth.gaussian("bench_cdm_dpm_known", (b, N, J)).to(dev), mask.to(dev))
        common = dict(clip_denoised=False, model_kwargs=kw, seed=1)
        shape = (b, N, J)
        runs[b] = {
            "native_ddim": lambda shape=shape, common=common: d_adm.ddim_sample_loop(cdm, shape, eta=0.0, **common),
            "native_2m": lambda shape=shape, common=common: d_adm.dpm_solver_sample_loop(cdm, shape, **common),
            "stepwise_2m": lambda shape=shape, common=common: _last(d_adm.dpm_solver_sample_loop_progressive(cdm, shape, **common)),
            "native_2m_impute": lambda shape=shape, common=common, imp=imp: d_adm.dpm_solver_sample_loop(cdm, shape, denoised_fn=imp, **common)}
        got = {k: run() for k, run in runs[b].items()}           # warm-up: weight pack, workspaces, rows; and what the loop promises
        got = {k: run() for k, run in runs[b].items()}
        sel = imp.mask.bool()
        assert torch.equal(got["native_2m"], got["stepwise_2m"]) and torch.equal(got["native_2m_impute"][sel], imp.known[sel]), b
    job = _two_stage(dev, cdm, d_adm, cmdm, d_amdm)
    job()
    job()
    times = {b: {k: [] for k in runs[b]} for b in BATCHES}
    job_ts, parent_ts = [], []
    for _ in range(args.reps):
        if args.parent_lib:                                   # a fresh process (this one has the GPU open; it idles meanwhile)
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", args.parent_lib, "--reps", "3"], capture_output=True,
                               text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"parent-library worker failed ({r.returncode}): {r.stderr[-800:]}")
            parent_ts += json.loads(line[0][7:])
        for b in BATCHES:
            for k, run in runs[b].items():
                times[b][k].append(_timed(run))
        job_ts += [_timed(job) for _ in range(3)]
    out = {"tool": "bench_cdm_dpm", "device": torch.cuda.get_device_name(0), "N": N, "respacing": RESP, "steps": steps, "reps": args.reps}
    ok = True
    for b in BATCHES:
        o = {k: _stats(ts, steps) for k, ts in times[b].items()}
        o["native_over_stepwise"] = round(o["stepwise_2m"]["ms"] / o["native_2m"]["ms"], 4)
        o["impute_over_stepwise"] = round(o["stepwise_2m"]["ms"] / o["native_2m_impute"]["ms"], 4)
        o["step_2m_over_ddim"] = round(o["native_2m"]["ms_per_step"] / o["native_ddim"]["ms_per_step"], 4)
        o["ddim_spread"] = o["native_ddim"]["spread"]
        ok = ok and o["native_over_stepwise"] > 1.0 and o["step_2m_over_ddim"] <= 1.0 + o["ddim_spread"]
        out[f"B{b}"] = o
    out["two_stage_B1"] = {"frames": L, "motion_steps": d_amdm.num_timesteps, "this": _stats(job_ts)}
    if parent_ts:
        out["two_stage_B1"]["parent"] = _stats(parent_ts)
        out["two_stage_B1"]["parent_over_this"] = round(out["two_stage_B1"]["parent"]["ms"] / out["two_stage_B1"]["this"]["ms"], 4)
    out["pass"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
