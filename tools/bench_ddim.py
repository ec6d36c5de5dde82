"""DDIM vs DDPM sampling throughput on one MI355X, printed as ONE JSON line.

    python tools/bench_ddim.py [--steps 50] [--reps 3] [--latency-runs 10]

For the CMDM (B = 32, L = 196, N = 8192 contact points) and the CDM Perceiver of configs[2] (B = 32, N = 8192): denoising steps/s of
ddim_sample_loop at eta = 0 and eta = 1 and of p_sample_loop over the same number of steps, measured interleaved in one process (best
repetition of each), and the p50 wall time of a full B = 1 `ddim50` sample at eta = 0 (condition tokens + loop + final synchronise).
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

from afm import synth  # noqa: E402
from afm.base import create_model_and_diffusion  # noqa: E402
from afm.config import load_config  # noqa: E402


def _cmdm(dev, resp):
    cfg = load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263", "model.text_model.max_length=20",
                                                                   "diffusion.steps=1000", f"diffusion.timestep_respacing='{resp}'"])
    model, diff = create_model_and_diffusion(cfg, device=dev)
    synth.fill_module_(model)
    return model.to(dev).eval(), diff


def _cdm(dev, resp):
    cfg = load_config("text_to_motion_contact_gen", "cdm", ["model.arch=Perceiver", "model.scene_model.use_scene_model=False", "model.input_feats=6",
                                                           "model.text_model.max_length=20", "diffusion.steps=500", f"diffusion.timestep_respacing='{resp}'"])
    model, diff = create_model_and_diffusion(cfg, device=dev)
    synth.fill_module_(model)
    return model.to(dev).eval(), diff


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _interleaved(diff, model, shape, kw, reps):
    """steps/s of ddim_sample_loop at eta = 0 (no noise term: no noise drawn), at eta = 1 (Philox noise every step, as DDPM) and of
    p_sample_loop on the same spaced process, alternating, best of `reps` each."""
    runs = {"ddim_eta0": lambda: diff.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, eta=0.0, seed=1),
            "ddim_eta1": lambda: diff.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, eta=1.0, seed=1),
            "ddpm": lambda: diff.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, seed=1)}
    for fn in runs.values():                                  # warm-up: weight packs, workspaces, rows
        fn()
    best = {k: float("inf") for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            best[k] = min(best[k], _timed(fn))
    n = diff.num_timesteps
    out = {f"{k}_steps_per_s": round(n / t, 2) for k, t in best.items()}
    out.update(ddim_eta0_over_ddpm=round(best["ddpm"] / best["ddim_eta0"], 4), ddim_eta1_over_ddpm=round(best["ddpm"] / best["ddim_eta1"], 4),
               steps_per_call=n)
    return out


def _p50_b1(model, diff, shape, kw_fn, runs):
    kw = kw_fn(1)
    run = lambda: diff.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=kw, eta=0.0, seed=2)
    run()
    ts = sorted(_timed(run) for _ in range(runs))
    return round(1e3 * ts[len(ts) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="spaced steps of both samplers in the throughput comparison (ddim<steps>)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--latency-runs", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, N = 32, 196, 8192
    resp = f"ddim{args.steps}"
    out = {"tool": "bench_ddim", "respacing": resp, "device": torch.cuda.get_device_name(0)}

    model, diff = _cmdm(dev, resp)
    cmdm_kw = lambda b: dict(c_text_feat=synth.text_feature(b).to(dev), c_pc_xyz=synth.scene_cloud(b, N).to(dev),
                             c_pc_contact=synth.contact_map(b, N).to(dev), x_mask=torch.zeros(b, L, dtype=torch.bool, device=dev))
    out["cmdm_B32"] = _interleaved(diff, model, (B, L, 263), cmdm_kw(B), args.reps)
    model1, diff50 = _cmdm(dev, "ddim50")
    out["cmdm_B1_ddim50_p50_ms"] = _p50_b1(model1, diff50, (1, L, 263), cmdm_kw, args.latency_runs)
    del model, model1

    model, diff = _cdm(dev, resp)
    cdm_kw = lambda b: dict(c_text_feat=synth.text_feature(b).to(dev), c_pc_xyz=synth.scene_cloud(b, N).to(dev))
    out["cdm_B32"] = _interleaved(diff, model, (B, N, 6), cdm_kw(B), args.reps)
    model1, diff50 = _cdm(dev, "ddim50")
    out["cdm_B1_ddim50_p50_ms"] = _p50_b1(model1, diff50, (1, N, 6), cdm_kw, args.latency_runs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
