"""Throughput of the imputing sampling loops of the CMDM on one MI355X, printed as ONE JSON line.

    python tools/bench_impute.py [--reps 3] [--ddpm-steps 200] [--scale 2.5]

B = 32, L = 196, N = 8192 contact points.  Per sampler - the DDPM chain respaced to --ddpm-steps, `ddim50` at eta = 0, the guided DDPM
chain - three arms, alternating in one process, every repetition kept (best, and all): the native loop without imputation, the native
imputing loop (afm_cmdm_impute_loop_range) and the step-by-step loop with the same Impute (what a `denoised_fn` meant before: one host
round trip, one afm_impute launch and one more [B, L, D] copy per step).  The DDIM loop at eta = 1 over the DDPM chain's steps is timed
too: it has the launch count of the imputing DDPM loop.  The mask: the first and last 10 frames and the four root features of every frame.
The one pass / fail: every native imputing loop is faster than the step-by-step loop (`native_over_stepwise` > 1).
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

B, L, N = 32, 196, 8192


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ddpm-steps", type=int, default=200)
    ap.add_argument("--scale", type=float, default=2.5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.cmdm import GuidedCMDM
    from afm.config import load_config
    from afm.diffusion import Impute
    cfg = lambda resp: load_config("text_to_motion_contact_motion_gen", "cmdm",
                                   ["model.data_repr=h3d", "model.input_feats=263", "model.text_model.max_length=20", "diffusion.steps=1000",
                                    f"diffusion.timestep_respacing='{resp}'"])
    model = create_model(cfg(""), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    guided = GuidedCMDM(model, args.scale)
    kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev),
              c_pc_contact=synth.contact_map(B, N).to(dev), x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev))
    mask = torch.zeros(B, L, 263, dtype=torch.bool)
    mask[:, :10], mask[:, -10:], mask[:, :, :4] = True, True, True
    imp = Impute(synth.gaussian("bench_impute_known", (B, L, 263)).to(dev), mask.to(dev))
    d_ddpm = create_gaussian_diffusion(cfg(str(args.ddpm_steps)))
    d_eta1 = create_gaussian_diffusion(cfg(f"ddim{args.ddpm_steps}"))
    d_ddim = create_gaussian_diffusion(cfg("ddim50"))
    common = dict(clip_denoised=False, model_kwargs=kw, seed=1)
    shape = (B, L, 263)
    samplers = {          # name: (steps, {arm: run})
        "ddpm": (d_ddpm.num_timesteps, {
            "native": lambda: d_ddpm.p_sample_loop(model, shape, **common),
            "native_impute": lambda: d_ddpm.p_sample_loop(model, shape, denoised_fn=imp, **common),
            "stepwise_impute": lambda: _last(d_ddpm.p_sample_loop_progressive(model, shape, denoised_fn=imp, **common)),
            "ddim_eta1": lambda: d_eta1.ddim_sample_loop(model, shape, eta=1.0, **common)}),
        "ddim50": (d_ddim.num_timesteps, {
            "native": lambda: d_ddim.ddim_sample_loop(model, shape, eta=0.0, **common),
            "native_impute": lambda: d_ddim.ddim_sample_loop(model, shape, eta=0.0, denoised_fn=imp, **common),
            "stepwise_impute": lambda: _last(d_ddim.ddim_sample_loop_progressive(model, shape, eta=0.0, denoised_fn=imp, **common))}),
        "cfg_ddpm": (d_ddpm.num_timesteps, {
            "native": lambda: d_ddpm.p_sample_loop(guided, shape, **common),
            "native_impute": lambda: d_ddpm.p_sample_loop(guided, shape, denoised_fn=imp, **common),
            "stepwise_impute": lambda: _last(d_ddpm.p_sample_loop_progressive(guided, shape, denoised_fn=imp, **common))}),
    }
    out = {"tool": "bench_impute", "device": torch.cuda.get_device_name(0), "B": B, "L": L, "reps": args.reps, "scale": args.scale,
           "known_fraction": round(mask.float().mean().item(), 4)}
    times = {s: {k: [] for k in arms} for s, (_, arms) in samplers.items()}
    for s, (_, arms) in samplers.items():          # warm-up: weight packs, workspaces, rows; and the property the loops exist for
        for k, run in arms.items():
            x = run()
            if "impute" in k:
                assert torch.equal(x[imp.mask.bool()], imp.known[imp.mask.bool()]), (s, k)
    for _ in range(args.reps):
        for s, (_, arms) in samplers.items():
            for k, run in arms.items():
                times[s][k].append(_timed(run))
    ok = True
    for s, (n, arms) in samplers.items():
        rate = lambda ts: [round(n / t, 2) for t in ts]
        o = {k: {"steps_per_s": max(rate(ts)), "all": rate(ts)} for k, ts in times[s].items()}
        nat = o["native"]["all"]
        o["native_spread"] = round((max(nat) - min(nat)) / max(nat), 4)
        o["impute_over_native"] = round(o["native_impute"]["steps_per_s"] / o["native"]["steps_per_s"], 4)
        o["native_over_stepwise"] = round(o["native_impute"]["steps_per_s"] / o["stepwise_impute"]["steps_per_s"], 4)
        if "ddim_eta1" in o:
            o["impute_over_ddim_eta1"] = round(o["native_impute"]["steps_per_s"] / o["ddim_eta1"]["steps_per_s"], 4)
        ok = ok and o["native_over_stepwise"] > 1.0
        out[s] = o
    out["every_native_imputing_loop_beats_stepwise"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
