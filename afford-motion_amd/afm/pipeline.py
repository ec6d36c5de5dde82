"""Two-stage sampling ADM (contact map over the scene) -> AMDM (motion) in ONE process.

The reference runs the stages as two `test.py` invocations that communicate through files:
`ContactHumanML3DEvaluator.evaluate` writes `H3D/pred_contact/{name}-{caption}.npy` = sqrt(-2 ln(c) sigma^2)
(utils/evaluate.py:41-82) and `ContactMotionHumanML3DDataset.__getitem__` reads it back and applies
exp(-d^2 / (2 sigma^2)) (datasets/humanml3d.py:763-774), looping `for k in range(k_samples)` sequentially
(test.py:88-101).  Here the k samples are the batch dimension, the hand-off stays in HBM
(`afm.dist.adm_to_amdm_condition`), and with several ranks the batch is sharded with one gather at the end.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional

import torch

from . import dist as adist
from .cmdm import GuidedCMDM
from .guidance import LongGuidance, MotionGuidance, Stitch


def two_stage_sample(adm, adm_diffusion, amdm, amdm_diffusion, *, text_feat: torch.Tensor, xyz: torch.Tensor, frames: int,
                     x_mask: Optional[torch.Tensor] = None, sigma: float = 0.8, contact_mean: float = 0.0,
                     contact_std: float = 1.0, seed: int = 0, sample_index0: int = 0,
                     adm_noise: Optional[Dict[str, torch.Tensor]] = None,
                     amdm_noise: Optional[Dict[str, torch.Tensor]] = None, sampler: str = "ddpm",
                     eta: float = 0.0, guidance_scale=None, guidance_drop=("text", "pc"), motion_impute=None,
                     contact_impute=None, contact_guidance=None, joint_targets=None, clearance=None, grounding=None) -> Dict[str, torch.Tensor]:
    """text_feat [B, text_dim], xyz [B, N, 3] (B = scenes x k_sample, already flattened) ->
    {"contact": [B, N, J] ADM sample, "cond": [B, N, J] AMDM condition, "motion": [B, frames, D]}.

    ``*_noise`` = optional {"x_T": ..., "steps": [T, ...]} explicit noise (parity tests); otherwise Philox
    keyed by (seed, sample_index0 + b), stage 2 uses seed + 1.  ``sampler`` = "ddpm" (p_sample_loop) or "ddim" (ddim_sample_loop with
    ``eta``) for both stages; DDIM runs the spaced process of each diffusion (e.g. timestep_respacing="ddim50").  ``sampler`` = "dpm++":
    DPM-Solver++(2M) (dpm_solver_sample_loop, deterministic; ``eta`` must be 0, explicit step noise is refused) on the spaced process of each
    diffusion (e.g. timestep_respacing="logsnr20"): both stages run in their native loops (the motion stage in
    afm_cmdm_dpm_loop_range, the contact stage in afm_cdm_dpm_loop_range; a non-Perceiver CDM samples step by step).
    ``guidance_scale`` (a float or a [B] tensor; None = unguided): classifier-free guidance of the MOTION stage, dropping the conditions named
    in ``guidance_drop`` (afm.cmdm.GuidedCMDM; the CDM of the first stage never reads the condition switches).  A mapping
    ``{"pc": s_pc, "text": s_text}`` (insertion order = first, second) gives every condition a scale of its own; ``guidance_drop`` must
    then name exactly the mapping's keys.
    ``contact_impute`` / ``motion_impute``: an afm.diffusion.Impute handed to stage 1 / stage 2 as ``denoised_fn`` (both stay in their native
    loops).  The contact stage is the one to steer: ``contact_impute.known`` [B, N, J] lives in the CDM's own sample space, the
    normalised contact (exp(-d^2 / 2 sigma^2) - mean) / std - pin it on the points of a chosen object, or to the value of zero contact
    on a region to keep clear.  ``motion_impute.known`` [B, frames, D] lives in the normalised motion space.
    ``contact_guidance``: an afm.diffusion.ContactGuidance handed to the motion stage as ``cond_fn`` (the stage stays in its native loop):
    the ``c_pc_contact`` it reads is the stage's own ``cond``, so the generated joints are pulled to the points the first stage marked.  A motion model on HumanML3D features (``data_repr`` "h3d",
    D = 263) takes ``ContactGuidance.h3d(joints, mean, std, to_scene=...)``, one on absolute positions ``ContactGuidance(cols, mean, std)``.
    ``joint_targets``: an afm.diffusion.JointTargets (or ``JointTargets.h3d``) - joints pulled to given scene positions at given frames - as
    the motion stage's ``cond_fn``; with ``contact_guidance`` too the stage is guided by their sum (afm.diffusion.MotionGuidance), still in
    its native loop.  ``clearance``: an afm.diffusion.SceneClearance (or ``SceneClearance.h3d``) - joints pushed off the obstacle points of
    ``xyz`` - summed with ``contact_guidance`` / ``joint_targets`` when given; the ``c_pc_contact`` its ``exempt_contact`` reads is the
    stage's own ``cond``.  ``grounding``: an afm.diffusion.FootGrounding (or ``FootGrounding.h3d``) - no joint below the floor, no planted
    foot sliding - summed with the other three terms when they are given."""
    if sampler not in ("ddpm", "ddim", "dpm++"):
        raise ValueError(f"sampler must be 'ddpm', 'ddim' or 'dpm++', not {sampler!r}")
    if sampler == "dpm++" and float(eta) != 0.0:
        raise ValueError(f"sampler 'dpm++' is deterministic: eta must be 0, not {eta!r}")
    if isinstance(guidance_scale, Mapping):          # (refused before the first stage runs)
        dropped = {guidance_drop} if isinstance(guidance_drop, str) else set(guidance_drop)
        if dropped != set(guidance_scale):
            raise ValueError(f"guidance_drop {sorted(dropped)} contradicts the conditions of the guidance_scale mapping {list(guidance_scale)}")

    def loop(diffusion, *args, **kw):
        if sampler == "ddim":
            return diffusion.ddim_sample_loop(*args, eta=eta, **kw)
        if sampler == "dpm++":
            if kw.pop("step_noise") is not None:
                raise ValueError("sampler 'dpm++' has no noise term: remove the \"steps\" noise")
            return diffusion.dpm_solver_sample_loop(*args, **kw)
        return diffusion.p_sample_loop(*args, **kw)

    B, N = xyz.shape[0], xyz.shape[1]
    dev = xyz.device
    adm_kw = dict(c_text_feat=text_feat, c_pc_xyz=xyz)
    an = adm_noise or {}
    contact = loop(adm_diffusion, adm, (B, N, adm.contact_dim), noise=an.get("x_T"), clip_denoised=False,
                   denoised_fn=contact_impute, model_kwargs=adm_kw, step_noise=an.get("steps"), seed=seed, sample_index0=sample_index0)
    cond = adist.adm_to_amdm_condition(contact, sigma=sigma, mean=contact_mean, std=contact_std)
    if x_mask is None:
        x_mask = torch.zeros(B, frames, dtype=torch.bool, device=dev)
    amdm_kw = dict(c_text_feat=text_feat, c_pc_xyz=xyz, c_pc_contact=cond, x_mask=x_mask)
    mn = amdm_noise or {}
    cond_fn = contact_guidance
    if joint_targets is not None:
        cond_fn = joint_targets if contact_guidance is None else MotionGuidance(contact_guidance, joint_targets)
    if clearance is not None:
        cond_fn = clearance if cond_fn is None else MotionGuidance(contact_guidance, joint_targets, clearance)
    if grounding is not None:
        cond_fn = grounding if cond_fn is None else MotionGuidance(contact_guidance, joint_targets, clearance, grounding)
    if guidance_scale is not None:
        amdm = GuidedCMDM(amdm, guidance_scale, guidance_drop)
    motion = loop(amdm_diffusion, amdm, (B, frames, amdm.motion_dim), noise=mn.get("x_T"), clip_denoised=False,
                  denoised_fn=motion_impute, cond_fn=cond_fn, model_kwargs=amdm_kw, step_noise=mn.get("steps"), seed=seed + 1, sample_index0=sample_index0)
    return {"contact": contact, "cond": cond, "motion": motion}


def long_motion_sample(adm, adm_diffusion, amdm, amdm_diffusion, *, text_feat: torch.Tensor, xyz: torch.Tensor, frames: int, overlap: int,
                       sampler: str = "dpm++", guidance_scale=None, guidance_drop=("text", "pc"), motion_impute=None, sigma: float = 0.8,
                       contact_mean: float = 0.0, contact_std: float = 1.0, seed: int = 0,
                       sample_index0: int = 0, contact_guidance=None, joint_targets=None, clearance=None) -> Dict[str, torch.Tensor]:
    """One scene, one thing after another: G long motions of ``frames`` frames, each S windows with a text of its own, sampled as
    ``G * S`` overlapping windows stitched inside the native loop (afm.diffusion.Stitch; "walk to the sofa, sit down, stand up again" is
    S = 3).  text_feat [G, S, text_dim], xyz [G, N, 3] ->
    {"contact": [G, S, N, J] ADM samples, "cond": [G * S, N, J] the motion stage's condition, "motion": [G, frames, D] the long motions,
    "windows": [G * S, L, D] the windows they were joined from}.

    Stage 1 runs as `two_stage_sample`'s on G * S rows - each window's text on its group's cloud - and the hand-off is unchanged.
    Stage 2 is stitched: window length ``L = overlap + ceil((frames - overlap) / S)``, neighbouring windows share ``overlap`` frames
    (``2 * overlap <= L``), x_T is the windows of one Philox draw per long motion keyed (seed + 1, sample_index0 + g), and the padded tail
    of a last window, if any, is masked.  ``sampler``: "dpm++" (dpm_solver_sample_loop) or "ddim" (ddim_sample_loop, eta = 0) on the spaced
    process of each diffusion - both deterministic, which is what keeps shared frames bit-identical in both windows.
    ``guidance_scale``: as `two_stage_sample`'s, a [G * S] tensor giving every window a scale of its own.  ``motion_impute``: an
    afm.diffusion.Impute in the LONG form ([G, frames, D]); it is cut into windows consistently (`Stitch.impute`).
    ``contact_guidance`` (a `ContactGuidance`) / ``joint_targets`` (a `JointTargets` in the LONG form, target [G, frames, K, 3]): wrapped
    into one afm.diffusion.LongGuidance on this call's Stitch and handed to stage 2 as its ``cond_fn`` - the terms are evaluated on the
    joined long motion against the stage's own ``cond``, each window with its own contact map; their scales are floats or [G] tensors.
    ``clearance``: an afm.diffusion.SceneClearance (or ``SceneClearance.h3d``) wrapped into the same `LongGuidance` as its third term - every
    window's frames are pushed off the group's cloud, expanded per window as for the other conditions; ``exempt_contact`` reads the stage's
    own ``cond`` per window (the window "sit down" exempts the sofa its contact map marks, the window "walk" does not); its ``weight`` is None
    or [G * S, N], row g * S + w; its scale a float or a [G] tensor.  Shapes that do not fit are refused before stage 1 runs."""
    if sampler not in ("dpm++", "ddim"):
        raise ValueError(f"long_motion_sample: sampler must be 'dpm++' or 'ddim' (a deterministic update), not {sampler!r}")
    if text_feat.dim() != 3 or xyz.dim() != 3 or xyz.shape[0] != text_feat.shape[0] or xyz.shape[2] != 3:
        raise ValueError(f"long_motion_sample: text_feat is [G, S, text_dim] and xyz [G, N, 3], got {tuple(text_feat.shape)} and {tuple(xyz.shape)}")
    if isinstance(guidance_scale, Mapping):
        dropped = {guidance_drop} if isinstance(guidance_drop, str) else set(guidance_drop)
        if dropped != set(guidance_scale):
            raise ValueError(f"guidance_drop {sorted(dropped)} contradicts the conditions of the guidance_scale mapping {list(guidance_scale)}")
    G, S, N = text_feat.shape[0], text_feat.shape[1], xyz.shape[1]
    stitch = Stitch(S, overlap, frames)
    guide = None if contact_guidance is None and joint_targets is None and clearance is None else \
        LongGuidance(stitch, contact_guidance, joint_targets, clearance)
    L, B, dev = stitch.length, G * S, xyz.device
    if motion_impute is not None and tuple(motion_impute.shape[:2]) != (G, frames):          # (refused before the first stage runs)
        raise ValueError(f"long_motion_sample: motion_impute is the long form [{G}, {frames}, D], got {motion_impute.shape}")
    if joint_targets is not None and tuple(joint_targets.target.shape[:2]) != (G, frames):          # (likewise)
        raise ValueError(f"long_motion_sample: joint_targets is the long form, target [{G}, {frames}, K, 3], got {tuple(joint_targets.target.shape)}")
    if clearance is not None:          # (likewise)
        if clearance.weight is not None and tuple(clearance.weight.shape) != (B, N):
            raise ValueError(f"long_motion_sample: the clearance's weight is per window, [{B}, {N}] (row g * {S} + w), got {tuple(clearance.weight.shape)}")
        if isinstance(clearance.scale, torch.Tensor) and clearance.scale.numel() != G:
            raise ValueError(f"long_motion_sample: the clearance's scale holds {clearance.scale.numel()} values for {G} long motions")
    x_mask = stitch.x_mask(G, dev, model=amdm)
    text = text_feat.reshape(B, text_feat.shape[2])
    cloud = xyz[:, None].expand(G, S, N, 3).reshape(B, N, 3)

    def loop(diffusion, *args, **kw):
        if sampler == "ddim":
            return diffusion.ddim_sample_loop(*args, eta=0.0, **kw)
        return diffusion.dpm_solver_sample_loop(*args, **kw)

    contact = loop(adm_diffusion, adm, (B, N, adm.contact_dim), clip_denoised=False, model_kwargs=dict(c_text_feat=text, c_pc_xyz=cloud),
                   seed=seed, sample_index0=sample_index0 * S)
    cond = adist.adm_to_amdm_condition(contact, sigma=sigma, mean=contact_mean, std=contact_std)
    amdm_kw = dict(c_text_feat=text, c_pc_xyz=cloud, c_pc_contact=cond, x_mask=x_mask)
    imp = None if motion_impute is None else stitch.impute(motion_impute.known, motion_impute.mask)
    if guidance_scale is not None:
        amdm = GuidedCMDM(amdm, guidance_scale, guidance_drop)
    windows = loop(amdm_diffusion, amdm, (B, L, amdm.motion_dim), clip_denoised=False, denoised_fn=imp, cond_fn=guide, model_kwargs=amdm_kw,
                   seed=seed + 1, sample_index0=sample_index0, stitch=stitch)
    return {"contact": contact.reshape(G, S, N, -1), "cond": cond, "motion": stitch.join(windows), "windows": windows}
