"""One native CMDM chain per row of the loop's dispatch table, hashed: run it on two checkouts and compare the columns.

    python tools/loop_plan_identity.py            # prints one `case sha256` line per chain

The model is the tests' random-weight CMDM (tests/test_gpu_cmdm.py::cmdm_cfg, synth.fill_module_), the shape the tests' small one: B = 4
samples (stitched: 2 long motions x 2 windows sharing 4 frames), L = 16, D = 263, N = 1024 points, 5 steps, fixed seeds.  Only public
names are used, so the script runs unchanged on a checkout from before the loop call was planned by `afm.cmdm.plan_loop_call`."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

B, L, D, N = 4, 16, 263, 1024
COLS = [0, 5, 11, 40, 100, 200]          # six non-overlapping column triples: one per contact channel


def main():
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.cmdm import GuidedCMDM
    from afm.config import to_config
    from afm.diffusion import ContactGuidance, Impute, JointTargets, MotionGuidance, Stitch
    dev = torch.device("cuda:0")
    cfg = lambda resp: to_config(dict(
        model=dict(name="CMDM", input_feats=D, data_repr="h3d", time_emb_dim=512,
                   contact_model=dict(contact_type="contact_cont_joints", contact_joints=[0, 10, 11, 12, 20, 21], planes=[32, 64, 128, 256],
                                      num_points=N, blocks=[2, 2, 2, 2]),
                   text_model=dict(version="ViT-B/32", max_length=20), arch="trans_enc", latent_dim=512, mask_motion=True,
                   num_layers=[1, 1, 1, 1, 1], num_heads=8, dropout=0.1, dim_feedforward=1024),
        diffusion=dict(predict_xstart=True, steps=1000, noise_schedule="cosine", timestep_respacing=resp, rescale_timesteps=False,
                       loss_type="MSE", learn_sigma=False, sigma_small=True)))
    model = create_model(cfg("5"), device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    one = GuidedCMDM(model, torch.tensor([2.5, 7.5, 1.0, 4.0], device=dev))
    two = GuidedCMDM(model, {"pc": 1.5, "text": 5.0})
    d5, dd5 = create_gaussian_diffusion(cfg("5")), create_gaussian_diffusion(cfg("ddim5"))
    kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev), c_pc_contact=synth.contact_map(B, N).to(dev),
              x_mask=torch.zeros(B, L, dtype=torch.bool, device=dev))
    kw["x_mask"][1, 13:] = True
    mean, std = 0.3 * synth.gaussian("identity_mean", (D,)), 0.5 + synth.gaussian("identity_std", (D,)).abs()
    t_mid = dd5.timestep_map[2] + 1          # the two first executed steps unguided, the last three guided
    contact = ContactGuidance(COLS, mean, std, sigma=0.8, scale=torch.tensor([1.0, 2.5, 0.5, 1.5]), t_start=t_mid)
    targets = JointTargets(COLS[:3], mean, std, target=synth.gaussian("identity_target", (B, L, 3, 3)).to(dev),
                           weight=(synth.gaussian("identity_weight", (B, L, 3)) > 0).float().to(dev), scale=0.7)
    imp = lambda: Impute(synth.gaussian("identity_known", (B, L, D)).to(dev), (synth.gaussian("identity_bits", (B, L, D)) > 0.6).to(dev))
    st = Stitch(2, 4, length=L)
    p = lambda m, **k: d5.p_sample_loop(m, (B, L, D), clip_denoised=False, model_kwargs=kw, seed=4, **k)
    ddim = lambda m, **k: dd5.ddim_sample_loop(m, (B, L, D), clip_denoised=False, model_kwargs=kw, seed=4, eta=0.0, **k)
    dpm = lambda m, **k: dd5.dpm_solver_sample_loop(m, (B, L, D), clip_denoised=False, model_kwargs=kw, seed=4, order=2, **k)
    cases = {          # by the table's rows, top to bottom
        "guide (bare contact, ddim)": lambda: ddim(model, cond_fn=contact),
        "guide (bare contact, one scale, ddpm, sliced)": lambda: p(one, cond_fn=contact, progress=True),
        "motion_guide (targets, ddim)": lambda: ddim(model, cond_fn=targets),
        "motion_guide (contact + targets, two scales, 2M, impute)": lambda: dpm(two, cond_fn=MotionGuidance(contact, targets), denoised_fn=imp()),
        "stitch (2M)": lambda: dpm(model, stitch=st),
        "stitch (one scale, ddim, impute)": lambda: ddim(one, stitch=st, denoised_fn=imp()),
        "dpm (plain)": lambda: dpm(model),
        "dpm (one scale, impute, sliced)": lambda: dpm(one, denoised_fn=imp(), progress=True),
        "cfg2 (ddpm)": lambda: p(two),
        "cfg2 (ddim, impute)": lambda: ddim(two, denoised_fn=imp()),
        "impute (plain, ddim)": lambda: ddim(model, denoised_fn=imp()),
        "impute (one scale, ddpm)": lambda: p(one, denoised_fn=imp()),
        "cfg_sample (ddpm)": lambda: p(one),
        "cfg_ddim": lambda: ddim(one),
        "sample (ddpm)": lambda: p(model),
        "ddim": lambda: ddim(model),
        "ddim (eta 0.5, clipped)": lambda: dd5.ddim_sample_loop(model, (B, L, D), clip_denoised=True, model_kwargs=kw, seed=4, eta=0.5),
    }
    for name, run in cases.items():
        x = run()
        torch.cuda.synchronize()
        assert torch.isfinite(x).all(), name
        print(f"{name}\t{hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
