"""What the guidance kernels of csrc/guidance.hip compute, hashed: run it on two checkouts and compare.

    python tools/guidance_identity.py            # prints one `item<TAB>sha256` line per item

Items: gradient (every sample guided, and with sample 1 at t >= t_start) and energy of ContactGuidance, JointTargets and the
MotionGuidance of both, each on absolute-position columns (`pos`) and on HumanML3D features (`h3d`, one to_scene matrix per sample), on
seeded inputs with B = 3 at (L, N, K) = (1, 1, 1), (7, 300, 2) and (196, 8192, 6): sample 0 ends in a padded frame (L > 1), sample 2 has
no valid frame.  Then the final sample of a 6-step native guided DDIM loop (B = 3, L = 16, N = 8192, K = 6, the benchmark's synthetic
CMDM) per representation, guided by the contact term alone and by the sum, on one and on two sub-batch streams.  The script uses the
public Python API alone, so it runs unchanged on any checkout that has the joint targets."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "afford-motion_amd"))

B, D = 3, 263
JOINTS = [0, 10, 11, 12, 20, 21]
SIGMA = 0.8
T_START = 500
CASES = ((1, 1, 1), (7, 300, 2), (196, 8192, 6))
ZUP = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0]])


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(name, value):
    print(f"{name}\t{value}", flush=True)


def guides(repr_, tag, L, K, dev, *, target_scale=torch.tensor([1.0, 2.5, 0.5]), t_start=None):
    """(contact, targets, both) on K joints of a [B, L, 263] motion, the same mean / std and transform"""
    from afm import synth
    from afm.diffusion import ContactGuidance, JointTargets, MotionGuidance
    mean, std = 0.3 * synth.gaussian(tag + "_mean", (D,)), 0.5 + synth.gaussian(tag + "_std", (D,)).abs()
    std[0], std[1:3] = 0.05, 0.1
    target = 1.5 * synth.gaussian(tag + "_target", (B, L, K, 3))
    weight = torch.zeros(B, L, K)
    weight[:, ::2] = 0.5
    scale = torch.tensor([1.0, 2.5, 0.5])
    if repr_ == "h3d":
        ts = (ZUP.repeat(B, 1, 1) + 0.2 * synth.gaussian(tag + "_to_scene", (B, 3, 4))).to(dev)
        contact = ContactGuidance.h3d(JOINTS[:K], mean, std, to_scene=ts, sigma=SIGMA, scale=scale, t_start=t_start)
        targets = JointTargets.h3d(JOINTS[:K], mean, std, to_scene=ts, target=target, weight=weight, scale=target_scale, t_start=t_start)
    else:
        cols = [3 * j for j in JOINTS[:K]]
        contact = ContactGuidance(cols, mean, std, sigma=SIGMA, scale=scale, t_start=t_start)
        targets = JointTargets(cols, mean, std, target=target, weight=weight, scale=target_scale, t_start=t_start)
    return contact, targets, MotionGuidance(contact, targets)


def kernels(dev):
    from afm import synth
    for L, N, K in CASES:
        tag = f"guidance_identity_L{L}_N{N}_K{K}"
        x = synth.gaussian(tag + "_x", (B, L, D)).to(dev)
        mask = torch.zeros(B, L, dtype=torch.bool)
        mask[0, max(L - 1, 1):] = True
        mask[2] = True
        kw = dict(c_pc_xyz=(1.5 * synth.gaussian(tag + "_q", (B, N, 3))).to(dev), c_pc_contact=synth.contact_map(B, N, K).to(dev),
                  x_mask=mask.to(dev))
        t_all, t_late = torch.zeros(B, dtype=torch.int64, device=dev), torch.tensor([0, T_START, 0], device=dev)
        for repr_ in ("pos", "h3d"):
            contact, targets, both = guides(repr_, tag, L, K, dev, t_start=T_START)
            for name, g in (("contact", contact), ("targets", targets), ("both", both)):
                head = f"L{L} N{N} K{K} {repr_} {name}"
                line(head + ": grad", sha(g(x, t_all, **kw)))
                line(head + ": grad, sample 1 at t_start", sha(g(x, t_late, **kw)))
                if name == "both":
                    ec, et = g.energies(x, **kw)
                    line(head + ": energy (contact)", sha(ec))
                    line(head + ": energy (targets)", sha(et))
                else:
                    line(head + ": energy", sha(g.energy(x, **kw)))


def loops(dev):
    from afm import synth
    from afm.base import create_gaussian_diffusion, create_model
    from afm.config import load_config
    L, N, K = 16, 8192, 6                       # (N: the model's contact encoder is laid out for the benchmark's cloud)
    cfg = load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263", "model.text_model.max_length=20",
                                                                    "diffusion.steps=1000", "diffusion.timestep_respacing='ddim6'"])
    model = create_model(cfg, device=dev)
    synth.fill_module_(model)
    model = model.to(dev).eval()
    d = create_gaussian_diffusion(cfg)
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, L - 3:] = True
    kw = dict(c_text_feat=synth.text_feature(B).to(dev), c_pc_xyz=synth.scene_cloud(B, N).to(dev), c_pc_contact=synth.contact_map(B, N, K).to(dev),
              x_mask=mask.to(dev))
    for repr_ in ("pos", "h3d"):
        contact, _, both = guides(repr_, "guidance_identity_loop", L, K, dev, target_scale=1e-3)
        for name, g in (("contact", contact), ("both", both)):
            for streams in (1, 2):
                model.loop_streams, model.loop_streams_auto = streams, False
                x = d.ddim_sample_loop(model, (B, L, D), clip_denoised=False, cond_fn=g, model_kwargs=kw, seed=1, eta=0.0)
                torch.cuda.synchronize()
                assert torch.isfinite(x).all(), (repr_, name, streams)
                line(f"6-step guided DDIM loop, {repr_} {name}, {streams} stream{'s' * (streams > 1)}", sha(x))


def main():
    dev = torch.device("cuda:0")
    kernels(dev)
    loops(dev)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
