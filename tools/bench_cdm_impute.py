"""Throughput of the imputing sampling loops of the CDM Perceiver on one MI355X, printed as ONE JSON line.

    python tools/bench_cdm_impute.py [--reps 5] [--ddpm-steps 200]

The shape of BASELINE configs[2]: B = 32, N = 8192 points, the H3D variant (9 input channels), T = 500.  Per sampler - the DDPM chain
respaced to --ddpm-steps and `ddim50` at eta = 0 - three arms, alternating in one process, every repetition kept (best, and all): the
native loop without imputation, the native imputing loop (afm_cdm_impute_loop_range: the select fused into dec_point) and the
step-by-step loop with the same Impute (one host round trip, one afm_impute launch and one update launch per step).  The mask pins every
joint on the first 1024 points of every sample (a chosen object: 12.5 % of the values).
Pass / fail: every native imputing loop is faster than the step-by-step loop (`native_over_stepwise` > 1) and not slower than its twin
without imputation by more than that twin's own spread in the call (`impute_over_native` >= 1 - `native_spread`).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

B, N, J = 32, 8192, 6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ddpm-steps", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    from afm.diffusion import Impute
    cfg = lambda resp: load_config("text_to_motion_contact_gen", "cdm",
                                   ["model.arch=Perceiver", "model.scene_model.use_scene_model=False", "model.input_feats=6",
                                    "model.text_model.max_length=20", "diffusion.steps=500", f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg(""), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev))
    mask = torch.zeros(B, N, J, dtype=torch.bool)
    mask[:, :1024] = True
    imp = Impute(synth.gaussian("bench_cdm_impute_known", (B, N, J)).to(dev), mask.to(dev))
    d_ddpm = create_gaussian_diffusion(cfg(str(args.ddpm_steps)))
    d_ddim = create_gaussian_diffusion(cfg("ddim50"))
    common = dict(clip_denoised=False, model_kwargs=kw, seed=1)
    shape = (B, N, J)
    samplers = {          # name: (steps, {arm: run})
        "ddpm": (d_ddpm.num_timesteps, {
            "native": lambda: d_ddpm.p_sample_loop(model, shape, **common),
            "native_impute": lambda: d_ddpm.p_sample_loop(model, shape, denoised_fn=imp, **common),
            "stepwise_impute": lambda: _last(d_ddpm.p_sample_loop_progressive(model, shape, denoised_fn=imp, **common))}),
        "ddim50": (d_ddim.num_timesteps, {
            "native": lambda: d_ddim.ddim_sample_loop(model, shape, eta=0.0, **common),
            "native_impute": lambda: d_ddim.ddim_sample_loop(model, shape, eta=0.0, denoised_fn=imp, **common),
            "stepwise_impute": lambda: _last(d_ddim.ddim_sample_loop_progressive(model, shape, eta=0.0, denoised_fn=imp, **common))}),
    }
    out = {"tool": "bench_cdm_impute", "device": torch.cuda.get_device_name(0), "B": B, "N": N, "reps": args.reps,
           "known_fraction": round(mask.float().mean().item(), 4)}
    times = {s: {k: [] for k in arms} for s, (_, arms) in samplers.items()}
    sel = imp.mask.bool()
    for s, (_, arms) in samplers.items():          # warm-up: weight pack, workspaces, rows; and the property the loops exist for
        got = {k: run() for k, run in arms.items()}
        assert torch.equal(got["native_impute"][sel], imp.known[sel]) and torch.equal(got["native_impute"], got["stepwise_impute"]), s
    for _ in range(args.reps):
        for s, (_, arms) in samplers.items():
            for k, run in arms.items():
                times[s][k].append(_timed(run))
    ok = True
    for s, (n, arms) in samplers.items():
        rate = lambda ts: [round(n / t, 2) for t in ts]
        o = {k: {"steps_per_s": max(rate(ts)), "all": rate(ts)} for k, ts in times[s].items()}
        for k in arms:
            o[k]["spread"] = round((max(o[k]["all"]) - min(o[k]["all"])) / max(o[k]["all"]), 4)
        o["native_spread"] = o["native"]["spread"]
        o["impute_over_native"] = round(o["native_impute"]["steps_per_s"] / o["native"]["steps_per_s"], 4)
        o["native_over_stepwise"] = round(o["native_impute"]["steps_per_s"] / o["stepwise_impute"]["steps_per_s"], 4)
        ok = ok and o["native_over_stepwise"] > 1.0 and o["impute_over_native"] >= 1.0 - o["native_spread"]
        out[s] = o
    out["pass"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
