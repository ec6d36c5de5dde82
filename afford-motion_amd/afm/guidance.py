"""What a sampling chain is conditioned on besides the denoiser's own inputs: known values (`Impute`), overlapping windows of a long
motion (`Stitch`), and the analytic ``cond_fn`` guidance terms (`ContactGuidance`, `JointTargets`, `SceneClearance`, `FootGrounding`, their sum `MotionGuidance`, and
`LongGuidance`, the terms on the joined long motion of a stitched chain).  The
samplers of afm.diffusion take them, the native loops of afm.cmdm / afm.cdm read their descriptions; afm.diffusion re-exports every name
(``afm.diffusion.Stitch is afm.guidance.Stitch``).  This module imports `ffi` and `ops` only: of a diffusion object it reads
``timestep_map`` and nothing else."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import ffi, ops


class Impute:
    """Known values imputed into every pred_xstart of a sampling chain - motion (editing: keyframes to in-between, a root trajectory, a
    prefix to continue) or contact (steering the first stage: contact pinned on the points of a chosen object, zero contact on a region
    to keep clear): ``x0 = where(mask, known, x0)`` after the denoiser and before the clamp - what the reference's ``denoised_fn``
    hook of p_mean_variance exists for (gaussian_diffusion.py:289-294).  A select, never a blend: where the mask is 0 nothing of ``known``
    reaches the result (a NaN there does not propagate).

    ``known``: float32 [B, L, D] in the model's normalised motion space, or [B, N, J] in the CDM's sample space (normalised contact,
    (exp(-d^2 / 2 sigma^2) - mean) / std).  ``mask``: bool or uint8 (nonzero = known), broadcastable to it
    ([L, D], [B, L, 1], [B, 1, D], ...); expanded ONCE to a contiguous uint8 of known's shape on known's device.

    The object is a callable ``imp(x0) -> ops.impute(x0, known, mask)`` (afm_impute, HIP), so it IS a ``denoised_fn`` wherever one is
    accepted - p_sample, ddim_sample, the progressive generators, the CDM; handed to p_sample_loop / ddim_sample_loop /
    dpm_solver_sample_loop of a denoiser whose ``afm_native_loop`` names ``impute`` (CMDM `trans_enc`, GuidedCMDM:
    afm_cmdm_impute_loop_range; the CDM Perceiver: afm_cdm_impute_loop_range) the whole chain stays in the native loop."""

    def __init__(self, known: torch.Tensor, mask: torch.Tensor):
        if known.dim() != 3:
            raise ValueError(f"Impute: known must be [B, L, D], got {tuple(known.shape)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"Impute: mask must be bool or uint8, not {mask.dtype}")
        if mask.dim() > 3:
            raise ValueError(f"Impute: mask {tuple(mask.shape)} does not broadcast to known {tuple(known.shape)}")
        try:
            full = torch.broadcast_shapes(tuple(mask.shape), tuple(known.shape))
        except RuntimeError:
            full = None
        if full != tuple(known.shape):
            raise ValueError(f"Impute: mask {tuple(mask.shape)} does not broadcast to known {tuple(known.shape)}")
        self.known = ffi.f32c(known.detach())
        # bool storage is one byte of 0 / 1 and the kernels read "nonzero": the expansion is one copy, no arithmetic
        m = mask.detach().to(device=self.known.device).expand(full).contiguous()
        self.mask = m.view(torch.uint8) if m.dtype == torch.bool else m

    @classmethod
    def _of(cls, known: torch.Tensor, mask: torch.Tensor) -> "Impute":
        imp = cls.__new__(cls)
        imp.known, imp.mask = known, mask
        return imp

    @property
    def shape(self):
        return tuple(self.known.shape)

    def __call__(self, x0: torch.Tensor) -> torch.Tensor:
        self.check(x0)
        return ops.impute(x0, self.known, self.mask)

    def check(self, x: torch.Tensor) -> None:
        """shape and device against a sample tensor"""
        if tuple(x.shape) != self.shape:
            raise ValueError(f"Impute: known is {self.shape}, the sample is {tuple(x.shape)}")
        if x.device != self.known.device:
            raise ValueError(f"Impute: known is on {self.known.device}, the sample on {x.device}")

    def narrow(self, start: int, count: int) -> "Impute":
        """the samples [start, start + count) - the slice of one rank of a sharded job (afm.dist.sharded_sample's sample_fn)"""
        if start < 0 or count < 0 or start + count > self.known.shape[0]:
            raise ValueError(f"Impute.narrow({start}, {count}) of a batch of {self.known.shape[0]}")
        return Impute._of(self.known[start:start + count], self.mask[start:start + count])


class Stitch:
    """G long motions sampled as ``B = G * S`` overlapping windows, batch row ``g * S + w`` window ``w`` of motion ``g`` (DoubleTake /
    DiffCollage / MultiDiffusion style): the windows are denoised side by side, each with its own text and contact map, and at every
    step the frames two windows share get one common pred_xstart.  Window ``w`` holds the long frames ``w * (L - ov) .. w * (L - ov) + L -
    1``; ``2 * ov <= L``, so a frame lies in at most two windows.  ``windows == 1`` or ``overlap == 0``: no blend.

    ``frames`` = F is the long motion's length, ``(S-1)(L-ov) + ov < F <= S*L - (S-1)*ov``; None: the full length.  A shorter F leaves
    a padded tail in the LAST window only, never inside an overlap - `x_mask` builds the mask for it (the model must have
    ``mask_motion=True``).  The window length L is the sample's; given ``frames`` it is known up front, ``ov + ceil((F - ov) / S)``
    (``length=`` states it where neither is given).

    The blend, for f = 0 .. ov-1, of the left element (w, L - ov + f) and the right element (w + 1, f):

        wr[f] = (f + 1) / (ov + 1),  wl[f] = 1 - wr[f]        float64 on the host, rounded to float32 once (a device row [2][ov])
        v = (wl[f] * x0_left) + (wr[f] * x0_right)            float32, three roundings, this order, no contraction

    Both windows evaluate the same expression on the same operands and get the same bits: with shared frames starting from shared noise
    (`x_T`) and a deterministic update (DDIM eta = 0, DPM-Solver++(2M)) the shared frames stay bit-identical in both windows at every
    step, and `join` of the result is the long motion read from either side.  Order inside a step: the guidance combine (each window its
    own scales) -> blend -> ``denoised_fn`` / `Impute` -> clamp -> ``x0 += gk * grad`` (a `LongGuidance` as ``cond_fn``) -> update.

    ``ddim_sample_loop(..., stitch=)`` and ``dpm_solver_sample_loop(..., stitch=)`` take it; a CMDM `trans_enc` or a GuidedCMDM runs the
    whole chain natively (afm_cmdm_stitch_loop_range).  A per-window `Impute` built by hand that disagrees in an overlap is the caller's
    error - `impute` builds a consistent one from the long form."""

    def __init__(self, windows: int, overlap: int, frames: Optional[int] = None, *, length: Optional[int] = None):
        S, ov = int(windows), int(overlap)
        if S < 1:
            raise ValueError(f"Stitch: at least one window, got {windows!r}")
        if ov < 0:
            raise ValueError(f"Stitch: overlap must be >= 0, got {overlap!r}")
        self.windows, self.overlap = S, ov
        self.frames = None if frames is None else int(frames)
        self.length = None if length is None else int(length)
        if self.length is None and self.frames is not None:
            if self.frames <= (ov if S > 1 else 0):
                raise ValueError(f"Stitch: {self.frames} frames do not reach past the first overlap of {ov}")
            self.length = self.frames if S == 1 else ov + -(-(self.frames - ov) // S)
        if self.length is not None:
            self._geometry(self.length)
        self._w: Dict[str, torch.Tensor] = {}

    # ---- geometry
    def _geometry(self, L: int) -> int:
        """checks the geometry at window length L; -> the long motion's frames"""
        S, ov = self.windows, self.overlap
        if L <= 0 or 2 * ov > L:
            raise ValueError(f"Stitch: 2 * overlap <= L - a frame lies in at most two windows - but overlap = {ov}, L = {L}")
        full = S * L - (S - 1) * ov
        F = full if self.frames is None else self.frames
        lo = (S - 1) * (L - ov) + (ov if S > 1 else 0)
        if not lo < F <= full:
            raise ValueError(f"Stitch: {S} windows of {L} frames sharing {ov} hold long motions of {lo + 1}..{full} frames (a padded tail "
                             f"in the last window only), not {F}")
        return F

    def full(self, L: int) -> int:
        """the long frames S windows of L frames cover"""
        return self.windows * L - (self.windows - 1) * self.overlap

    def check(self, B: int, L: int) -> int:
        """a batch of B windows of L frames against the geometry (ValueError); -> the long motion's frames F"""
        if B % self.windows != 0:
            raise ValueError(f"Stitch: the batch holds whole long motions - {B} rows are no multiple of {self.windows} windows")
        if self.length is not None and L != self.length:
            raise ValueError(f"Stitch: the windows have {self.length} frames, the sample has {L}")
        return self._geometry(L)

    def _resolve(self, length: Optional[int], F: Optional[int] = None) -> int:
        L = self.length if self.length is not None else length
        if L is None and F is not None:          # a full-length long motion names its window length
            S, ov = self.windows, self.overlap
            if (F - ov) % S == 0 and F > ov:
                L = ov + (F - ov) // S
        if L is None:
            raise ValueError("Stitch: the window length is not known - pass length= (or frames= to the constructor)")
        return int(L)

    # ---- the weight row
    def weights64(self) -> np.ndarray:
        """[2, ov] float64: wl then wr"""
        wr = (np.arange(self.overlap, dtype=np.float64) + 1.0) / (self.overlap + 1.0)
        return np.stack([1.0 - wr, wr], 0)

    def weights(self, device) -> torch.Tensor:
        """the float32 row [2, ov] on ``device``: `weights64` rounded once"""
        key = str(torch.device(device))
        if key not in self._w:
            self._w[key] = torch.from_numpy(self.weights64()).float().contiguous().to(device)
        return self._w[key]

    def describe(self, device) -> tuple:
        """(afm_stitch on ``device``, what must stay alive with it)"""
        w = self.weights(device)
        return ffi.Stitch(self.windows, self.overlap, w.data_ptr() if self.overlap > 0 else None), w

    # ---- long form <-> windows (copies; float32 on the GPU: afm_stitch_windows / afm_stitch_join)
    def windows_of(self, long: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
        """[G, F, D] -> [G * S, L, D]; frames at or behind F (the padded tail) are zero.  F: the long motion's frames or the full length."""
        if long.dim() != 3:
            raise ValueError(f"Stitch.windows_of: the long form is [G, F, D], got {tuple(long.shape)}")
        G, F, D = long.shape
        S, ov = self.windows, self.overlap
        L = self._resolve(length, F)
        self._geometry(L)
        lo = (S - 1) * (L - ov) + (ov if S > 1 else 0)
        if not lo < F <= self.full(L):
            raise ValueError(f"Stitch.windows_of: {F} frames do not fill {S} windows of {L} sharing {ov}")
        if long.is_cuda and long.dtype == torch.float32:
            return ops.stitch_windows(long, S, ov, L)
        out = long.new_zeros(G, S, L, D)
        for w in range(S):
            a = w * (L - ov)
            n = max(0, min(L, F - a))
            out[:, w, :n] = long[:, a:a + n]
        return out.reshape(G * S, L, D)

    def join(self, windows: torch.Tensor) -> torch.Tensor:
        """[G * S, L, D] -> [G, F, D]; a shared frame is read from the later window (after a stitched chain both hold the same bits)"""
        if windows.dim() != 3:
            raise ValueError(f"Stitch.join: the windows are [G * S, L, D], got {tuple(windows.shape)}")
        B, L, D = windows.shape
        F = self.check(B, L)
        S, ov = self.windows, self.overlap
        if windows.is_cuda and windows.dtype == torch.float32:
            return ops.stitch_join(windows, S, ov, F)
        v = windows.reshape(B // S, S, L, D)
        parts = [v[:, w, :(L - ov if w + 1 < S else F - w * (L - ov))] for w in range(S)]
        return torch.cat(parts, 1)

    def x_mask(self, G: int, device, length: Optional[int] = None, model=None) -> torch.Tensor:
        """bool [G * S, L], True = padded frame: the tail of every long motion's last window.  ``model``: checked for mask_motion."""
        L = self._resolve(length)
        F = self._geometry(L)
        pad = self.full(L) - F
        if pad > 0 and model is not None and not getattr(getattr(model, "model", model), "mask_motion", True):
            raise ValueError("Stitch: a long motion shorter than its windows pads the last window, which needs a model with mask_motion=True")
        m = torch.zeros(G, self.windows, L, dtype=torch.bool)
        if pad > 0:
            m[:, -1, L - pad:] = True
        return m.reshape(G * self.windows, L).to(device)

    def impute(self, known_long: torch.Tensor, mask_long: torch.Tensor, length: Optional[int] = None) -> Impute:
        """the `Impute` over the windows of a long-form known [G, F, D] / mask (broadcastable to it): consistent in the overlaps by
        construction (padded frames know nothing)"""
        imp = Impute(known_long, mask_long)          # (the long form checked and expanded like any other)
        return Impute._of(self.windows_of(imp.known, length), self.windows_of(imp.mask, length))

    def x_T(self, B: int, L: int, D: int, device, seed: int, sample_index0: int = 0) -> torch.Tensor:
        """x_T of a stitched chain: the windows of ONE Philox draw [G, S*L - (S-1)*ov, D] keyed (seed, sample_index0 + g) - shared frames
        start from shared noise, and a long motion's noise does not depend on the batch around it"""
        self.check(B, L)
        return self.windows_of(ops.randn((B // self.windows, self.full(L), D), device, seed=seed, sample_index0=sample_index0, step=-1), L)


class CondFnError(ValueError, NotImplementedError):
    """A ``cond_fn`` that does not implement the protocol ``cond_fn(x, t, **model_kwargs) -> float32 tensor of x's shape on x's device``: it
    cannot be called that way, or what it returns does not fit.  It is a ValueError, which is what such a callable deserves.  The second
    base, NotImplementedError, and the `inspect.signature(...).bind` check in `_cond_grad` exist for one reason: before ``cond_fn`` was
    opened every sampler refused it with NotImplementedError, and tests/test_gpu_dpm.py::test_refusals still expects that from
    ``dpm_solver_sample(_loop)`` for ``lambda *a: None`` and ``lambda *a, **k: None``.  When that test is brought up to date, drop the
    second base and the bind check."""


# ---------------------------------------------------------------------- scales: one float or one value per sample
def scale_value(scale, who: str, got: str = ""):
    """a guidance scale as its owner keeps it: a float, or a private float32 [B] copy of a floating tensor (``who`` leads the message)"""
    if isinstance(scale, torch.Tensor):
        if scale.dim() > 1 or not scale.is_floating_point():
            raise ValueError(f"{who}: `scale` must be a float or a floating [B] tensor, got {got}{tuple(scale.shape)} {scale.dtype}")
        return scale.detach().clone().float().reshape(-1)
    return float(scale)


def scale_fits(scale, B: int, who: str, name: str = "`scale`") -> None:
    if isinstance(scale, torch.Tensor) and scale.numel() != B:
        raise ValueError(f"{who}: {name} holds {scale.numel()} values for a batch of {B}")


def scale_row(scale, B: int, device, who: str, name: str = "`scale`") -> torch.Tensor:
    """the float32 [B] row of a `scale_value` on ``device``"""
    scale_fits(scale, B, who, name)
    return scale.to(device).contiguous() if isinstance(scale, torch.Tensor) else torch.full((B,), scale, dtype=torch.float32, device=device)


def _guide_mask(x: torch.Tensor, model_kwargs, who: str):
    """x_mask of ``model_kwargs`` as the guidance kernels take it: uint8 [B, L] on x's device, or None"""
    fm = model_kwargs.get("x_mask")
    if fm is None:
        return None
    fm = fm.to(device=x.device).reshape(x.shape[0], -1)
    if fm.shape[1] != x.shape[1]:
        raise ValueError(f"{who}: x_mask covers {fm.shape[1]} frames, the sample has {x.shape[1]}")
    return (fm.view(torch.uint8) if fm.dtype == torch.bool else fm.to(torch.uint8)).contiguous()


class _JointTerm:
    """What `ContactGuidance`, `JointTargets`, `SceneClearance` and `FootGrounding` share: K joints named as column triples of absolute positions or (``.h3d``) as joints of
    HumanML3D features placed by ``to_scene``, the mean / std that de-normalise the motion, a scale per sample, ``t_start`` - and, per
    call, the pieces of the C description both fill the same way."""
    _NOUN = "guided"            # "1 to 16 <noun> joints" (_NAME: the class's name in its messages)
    _H3D_NAME = True            # an h3d object's messages say "<name>.h3d" behind the constructor's own checks too

    def _init(self, cols, joints, to_scene, mean: torch.Tensor, std: torch.Tensor, scale, t_start: Optional[int], **own) -> None:
        who = self._NAME + ("" if joints is None else ".h3d")
        if joints is None:
            cols = [int(c) for c in cols]
            if not 1 <= len(cols) <= ffi.GUIDE_MAX_JOINTS:
                raise ValueError(f"{who}: 1 to {ffi.GUIDE_MAX_JOINTS} {self._NOUN} joints, got {len(cols)}")
        else:
            joints = ops.h3d_joint_list([int(j) for j in joints], ffi.GUIDE_MAX_JOINTS, who)
        if mean.dim() != 1 or std.shape != mean.shape:
            raise ValueError(f"{who}: mean and std must be [D] and alike, got {tuple(mean.shape)} and {tuple(std.shape)}")
        D = mean.shape[0]
        for i, c in enumerate(cols if joints is None else []):          # (an h3d layout names joints: there are no columns to check)
            if c < 0 or c + 3 > D:
                raise ValueError(f"{who}: the column triple {c}..{c + 2} leaves the motion vector of {D} columns")
            if any(abs(c - o) < 3 for o in cols[:i]):
                raise ValueError(f"{who}: the column triple at {c} overlaps another one")
        if joints is not None:
            if D < ffi.H3D_COLS:
                raise ValueError(f"{who}: the joint recovery reads columns 0..{ffi.H3D_COLS - 1}, the motion vector has {D}")
            to_scene = ops.h3d_to_scene(to_scene, who)
            cols, who = [], who if self._H3D_NAME else self._NAME
        self.cols, self.joints, self.to_scene, self.D, self._who = cols, joints, to_scene, D, who
        self.mean, self.std = ffi.f32c(mean.detach()), ffi.f32c(std.detach())
        self._host = (self.mean, self.std) + tuple(self._own(**own))          # what `_on` copies to a device, once
        self.scale = scale_value(scale, who)
        self.t_start = None if t_start is None else int(t_start)
        self._dev: Dict[str, tuple] = {}

    @property
    def K(self) -> int:
        return len(self.cols if self.joints is None else self.joints)

    def _check_sample(self, x: torch.Tensor) -> None:
        if x.dim() != 3 or x.shape[-1] != self.D:
            raise ValueError(f"{self._who}: mean / std describe {self.D} columns, the sample is {tuple(x.shape)}")

    def _to_scene_on(self, B: int, device) -> tuple:
        return (None, 0) if self.joints is None else ops.h3d_to_scene_on(self.to_scene, B, device, self._NAME + ".h3d")

    def _on(self, device) -> tuple:
        """the term's own tensors (mean, std, ...) on ``device``, copied once per device"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in self._host)
        return self._dev[key]

    def _fill(self, g, mean, std, scale, ts, stride, diffusion):
        """the fields every term's description has (``diffusion`` given: first_guided of a chain on it); -> its afm_h3d_layout or None"""
        g.first_guided = 0 if diffusion is None else self.first_guided(diffusion)
        g.mean, g.std, g.scale, g.K = mean.data_ptr(), std.data_ptr(), scale.data_ptr(), self.K
        g.cols[:len(self.cols)] = self.cols
        g.t_start = 2**62 if self.t_start is None else self.t_start
        if self.joints is None:
            return None
        lay = ffi.H3dLayout()
        lay.joints[:self.K], lay.to_scene, lay.to_scene_stride = self.joints, ffi.ptr(ts), stride
        g.h3d = C.pointer(lay)
        return lay

    def first_guided(self, diffusion) -> int:
        """the first executed step of a chain on ``diffusion`` that carries this term: the count of its timesteps >= t_start"""
        return 0 if self.t_start is None else sum(1 for t in diffusion.timestep_map if t >= self.t_start)


class ContactGuidance(_JointTerm):
    """A ``cond_fn`` that pulls the contact joints of a generated motion towards the points its contact map marks - the analytic gradient
    of an energy between the map the motion implies and the map it was given (afm_contact_guidance, HIP; no second network, no autograd).

    ``cols``: K ints (K <= 16), each the column of the x coordinate of one contact joint in the motion vector, y and z the next two
    columns.  The columns must hold ABSOLUTE joint positions (``data_repr`` "pos" / "pos_rot": ``3 * j`` for joint j).  "h3d" has no such
    columns - it integrates root velocities over the frames: ``ContactGuidance.h3d(joints, mean, std)`` builds the guidance for it, the
    same energy on the joints the features imply (below).  The triples lie inside D and do not overlap.
    ``mean`` / ``std`` [D] de-normalise the motion.  ``sigma``: the contact map's.  ``scale``: a float or a [B] tensor.  ``t_start``: only
    steps whose model timestep is < t_start are guided (None: all).

    With q = c_pc_xyz [B, N, 3], c = c_pc_contact [B, N, K] (un-normalised exp(-d^2 / 2 sigma^2), as the motion model receives it) and
    x_mask [B, L] (True = padded frame) taken from ``model_kwargs``:

        p[b,f,k,:] = x[b,f,cols[k]:cols[k]+3] * std + mean
        d2[b,n,k]  = min over frames f with not x_mask[b,f] of |p[b,f,k,:] - q[b,n,:]|^2,   f* the FIRST frame that attains it
        chat       = exp(-d2 / (2 sigma^2))          (no valid frame: 0)
        E[b]       = 1/(N K) sum_{n,k} (chat - c)^2
        dE/dx[b,f,cols[k]+a] = sum_{n: f*(b,n,k) = f} (2/(N K)) (chat - c) chat (-(p_a - q_a) / sigma^2) std_a

    ``guide(x, t, **model_kwargs)`` returns -scale[b] * dE/dx [B, L, D] float32 (zero outside the named columns, in padded frames, in a
    sample without a valid frame or with t >= t_start); ``guide.energy(x, **model_kwargs)`` returns E [B] (a score for picking the best
    of several samples).  float32 order of the kernel: d2 = (dx*dx + dy*dy) + dz*dz; w = (chat - c) * chat; S_a = sum of w * (p_a - q_a)
    over the frame's points (lane l of a wave takes n = l, l + 64, ..., then a fixed butterfly); result = ((scale * coef) * std_a) * S_a
    with coef = 2 / (N K sigma^2) rounded once from float64.  No atomics: bit-identical run to run, and a sample's result does not depend
    on the batch around it.

    Handed as ``cond_fn`` to p_sample_loop / ddim_sample_loop / dpm_solver_sample_loop of a denoiser whose ``afm_native_loop`` names
    ``contact_guide`` (GuidedCMDM) or takes it in its private ``_guidance`` bundle (CMDM `trans_enc`, whose public keywords stay the
    CDM's) - afm_cmdm_guide_loop_range - the whole chain stays in the native loop; any other
    denoiser samples step by step through ``__call__``.  A skipped step natively launches no gradient kernel; step by step it adds a
    gradient of zeros (the same values).

    HumanML3D features: ``ContactGuidance.h3d(joints, mean, std, to_scene=None, ...)`` with ``joints`` the K joint indices 0..21.  With
    u = x * std + mean (columns 0..66 are read) and the velocity columns 0..2 of a padded frame counted as zero, p is the reference's
    recover_from_ric placed in the scene:

        th_f = sum_{g<f} u[g,0];  c_f, s_f = cos, sin(2 th_f);  X_f = sum_{1<=h<=f} (u[h-1,1] c_h - u[h-1,2] s_h),  Z_f likewise with
        (u[h-1,1] s_h + u[h-1,2] c_h);  joint 0: P = (X_f, u[f,3], Z_f);  joint j, l = u[f, 4+3(j-1):7+3(j-1)]:
        P = (l_x c_f - l_z s_f + X_f, l_y, l_x s_f + l_z c_f + Z_f);  p = A P + t,  to_scene = [A|t]

    ``to_scene`` is a float32 [3, 4] or [B, 3, 4] tensor (None: identity).  The reference does not fix how an h3d motion is placed in
    its scene, so the transform is an argument and not a constant; y-up to z-up is A = [[1, 0, 0], [0, 0, -1], [0, 1, 0]], t = 0.  The
    energy is the one above on these p; the gradient is its exact adjoint through the recovery (afm_contact_guidance with an
    afm_h3d_layout: four launches - recovery, the two passes, adjoint - every scan over the frames one lane's serial chain in frame order,
    no atomics), nonzero only in columns 0..66 of valid frames.  Everything else - ``__call__``, ``energy``, ``first_guided``, the
    native loops of GuidedCMDM and the plain CMDM, ``two_stage_sample(contact_guidance=...)`` - works as for the column form."""
    _NAME, _NOUN, _H3D_NAME = "ContactGuidance", "contact", False

    def __init__(self, cols, mean: torch.Tensor, std: torch.Tensor, *, sigma: float = 0.8, scale=1.0, t_start: Optional[int] = None):
        self._init(cols, None, None, mean, std, scale, t_start, sigma=sigma)

    @classmethod
    def h3d(cls, joints, mean: torch.Tensor, std: torch.Tensor, *, to_scene: Optional[torch.Tensor] = None, sigma: float = 0.8, scale=1.0,
            t_start: Optional[int] = None) -> "ContactGuidance":
        """The guidance of a HumanML3D-feature motion (``data_repr`` "h3d", D >= 67): ``joints`` are joint indices 0..21, ``to_scene`` a
        float32 [3, 4] or [B, 3, 4] tensor [A|t] on the samples' device (None: identity).  See the class docstring."""
        self = cls.__new__(cls)
        self._init(None, joints, to_scene, mean, std, scale, t_start, sigma=sigma)
        return self

    def _own(self, sigma) -> tuple:
        if not float(sigma) > 0.0:
            raise ValueError(f"{self._who}: sigma must be positive, got {sigma!r}")
        self.sigma = float(sigma)
        return ()

    def describe(self, x: torch.Tensor, model_kwargs, diffusion=None, *, long=None) -> tuple:
        """(afm_contact_guide of this sample tensor and these conditions, x_mask as uint8 or None, what must stay alive with it).  With
        ``diffusion``: first_guided set for a chain on it (the loops).  ``long`` = (G, F), `LongGuidance`'s: x holds the windows of G long
        motions - q / c stay per window, scale and to_scene are per long motion, x_mask is not read."""
        self._check_sample(x)
        for name in ("c_pc_xyz", "c_pc_contact"):
            if name not in model_kwargs:
                raise ValueError(f"ContactGuidance reads {name} from model_kwargs")
        B, K = x.shape[0], self.K
        q, c = model_kwargs["c_pc_xyz"], model_kwargs["c_pc_contact"]
        if q.dim() != 3 or q.shape[0] != B or q.shape[2] != 3 or tuple(c.shape) != (B, q.shape[1], K):
            raise ValueError(f"ContactGuidance: c_pc_xyz must be [{B}, N, 3] and c_pc_contact [{B}, N, {K}], got {tuple(q.shape)} and {tuple(c.shape)}")
        rows = B if long is None else long[0]
        scale_fits(self.scale, rows, self._who)
        ts, stride = self._to_scene_on(rows, x.device)
        ffi.require_gpu(x, q, c)
        scale = scale_row(self.scale, rows, x.device, self._who)
        q, c = ffi.f32c(q), ffi.f32c(c)
        mean, std = self._on(x.device)
        fm = _guide_mask(x, model_kwargs, self._who) if long is None else None
        g = ffi.ContactGuide()
        lay = self._fill(g, mean, std, scale, ts, stride, diffusion)
        g.q, g.c, g.N, g.sigma = q.data_ptr(), c.data_ptr(), q.shape[1], self.sigma
        return g, fm, (q, c, mean, std, scale, fm, lay, ts)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        g, fm, keep = self.describe(x, model_kwargs)
        return ops.contact_guidance(g, x, fm, None if self.t_start is None else t.to(x.device))[0]

    def energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        g, fm, keep = self.describe(x, model_kwargs)
        return ops.contact_guidance(g, x, fm, grad=False, energy=True)[1]


class JointTargets(_JointTerm):
    """A ``cond_fn`` that pulls named joints to given places in the scene at given frames: a root path through the room, a hand on a handle
    at frame 120, a pose at the last frame (afm_motion_guidance, HIP; no network, no autograd).

    ``cols``: K ints (K <= 16), the column of the x coordinate of each guided joint in a motion vector of ABSOLUTE positions (``data_repr``
    "pos" / "pos_rot"), as for `ContactGuidance`; ``JointTargets.h3d(joints, mean, std, ...)`` names joints 0..21 of a HumanML3D-feature
    motion instead (joint 0 is the root) and takes the ``to_scene`` of `ContactGuidance.h3d`.  ``target`` [B, L, K, 3] float32 holds scene
    coordinates, ``weight`` [B, L, K] their weights: 0 means no target, and the target value there is never read (it may be NaN).
    ``scale``: a float or a [B] tensor.  ``t_start``: only steps whose model timestep is < t_start are guided (None: all).  ``x_mask`` is
    read from ``model_kwargs`` as `ContactGuidance` reads it; nothing else is.

    With p[b,f,k,:] the positions `ContactGuidance` computes (x * std rounded, + mean rounded; h3d: the recovery kernel's output):

        E[b] = sum over valid frames f and joints k of  w * ((dx*dx + dy*dy) + dz*dz),   d = p - target

    not normalised - the weights are the caller's.  Order of the sum: the items e = f * K + k of a sample are dealt to the 256 threads of one
    block, thread i adds e = i, i + 256, ... in that order, then a fixed wave butterfly and ((r0 + r1) + r2) + r3 over the four waves: a
    function of the sample alone.  ``guide(x, t, **model_kwargs)`` returns -scale[b] * dE/dx:

        columns:  d = target_a - p_a;  m = w * d;  grad[b,f,cols[k]+a] = ((scale[b] * 2) * std_a) * m                       (one launch)
        h3d:      S[b,f,k,:] = w * (target - p), carried through the adjoint of the recovery with coef = 2 - the kernel and the six
                  serial scans `ContactGuidance.h3d` uses (three launches: recovery, targets, adjoint)

    exactly zero in every other column, in padded frames, where w == 0 and in samples with t >= t_start.  ``guide.energy(x, **model_kwargs)``
    returns E [B].  Handed as ``cond_fn`` it stays in the native loops wherever a `ContactGuidance` does (afm_cmdm_motion_guide_loop_range);
    `MotionGuidance` sums it with a `ContactGuidance`."""
    _NAME = "JointTargets"

    def __init__(self, cols, mean: torch.Tensor, std: torch.Tensor, *, target: torch.Tensor, weight: torch.Tensor, scale=1.0,
                 t_start: Optional[int] = None):
        self._init(cols, None, None, mean, std, scale, t_start, target=target, weight=weight)

    @classmethod
    def h3d(cls, joints, mean: torch.Tensor, std: torch.Tensor, *, target: torch.Tensor, weight: torch.Tensor,
            to_scene: Optional[torch.Tensor] = None, scale=1.0, t_start: Optional[int] = None) -> "JointTargets":
        """The targets of a HumanML3D-feature motion (``data_repr`` "h3d", D >= 67): ``joints`` are joint indices 0..21 (0: the root),
        ``to_scene`` a float32 [3, 4] or [B, 3, 4] tensor [A|t] on the samples' device (None: identity).  See the class docstring."""
        self = cls.__new__(cls)
        self._init(None, joints, to_scene, mean, std, scale, t_start, target=target, weight=weight)
        return self

    def _own(self, target, weight) -> tuple:
        K = self.K
        if not isinstance(target, torch.Tensor) or not isinstance(weight, torch.Tensor) or target.dim() != 4 or target.shape[2:] != (K, 3) or \
                tuple(weight.shape) != tuple(target.shape[:3]) or not target.is_floating_point() or not weight.is_floating_point():
            raise ValueError(f"{self._who}: target must be a floating [B, L, {K}, 3] tensor and weight [B, L, {K}], got "
                             f"{tuple(getattr(target, 'shape', ()))} and {tuple(getattr(weight, 'shape', ()))}")
        self.target, self.weight = ffi.f32c(target.detach()), ffi.f32c(weight.detach())
        return self.target, self.weight

    def describe(self, x: torch.Tensor, model_kwargs, diffusion=None, *, shared=None, long=None) -> tuple:
        """(afm_joint_targets of this sample tensor, x_mask as uint8 or None, what must stay alive with it).  ``shared``: the (mean, std,
        to_scene, stride) device tensors of the contact term this one is summed with - a sum names one set of them.  ``long`` = (G, F),
        `LongGuidance`'s: x holds the windows of G long motions of F frames, which is what target / weight / scale / to_scene describe;
        x_mask is not read."""
        who = self._who
        self._check_sample(x)
        B, L, K = (x.shape[0], x.shape[1], self.K) if long is None else (long[0], long[1], self.K)
        if tuple(self.target.shape) != (B, L, K, 3):
            raise ValueError(f"{who}: target is {tuple(self.target.shape)} and weight {tuple(self.weight.shape)}, the sample needs "
                             f"[{B}, {L}, {K}, 3] and [{B}, {L}, {K}]")
        scale_fits(self.scale, B, who)
        fm = _guide_mask(x, model_kwargs, who) if long is None else None
        ts, stride = self._to_scene_on(B, x.device)          # (checked against the batch before anything touches the device)
        ffi.require_gpu(x)
        mean, std, target, weight = self._on(x.device)
        scale = scale_row(self.scale, B, x.device, who)
        if shared is not None:
            mean, std = shared[0], shared[1]
            if self.joints is not None:
                ts, stride = shared[2], shared[3]
        g = ffi.JointTargets()
        lay = self._fill(g, mean, std, scale, ts, stride, diffusion)
        g.target, g.weight = target.data_ptr(), weight.data_ptr()
        return g, fm, (target, weight, mean, std, scale, fm, lay, ts)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        return MotionGuidance(targets=self)(x, t, **model_kwargs)

    def energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        return MotionGuidance(targets=self).energies(x, **model_kwargs)[1]


class SceneClearance(_JointTerm):
    """A ``cond_fn`` that pushes joints off the obstacle points of the scene cloud - the one term that pushes: `ContactGuidance` and
    `JointTargets` pull, this one keeps the skeleton out of the furniture (afm_scene_guidance, HIP; no network, no autograd).

    ``cols``: K ints (K <= 16) as for `ContactGuidance`; ``SceneClearance.h3d(joints, mean, std, to_scene=None, ...)`` names joints 0..21
    of a HumanML3D-feature motion instead.  ``radius``: a positive float or K of them - a joint is pushed by the points closer than its
    radius.  ``weight`` [B, N] float (None: every point weighs 1).  ``up`` (0..2) and ``min_height``: points with ``q[up] < min_height``
    weigh 0 - that takes the floor out.  ``exempt_contact``: points whose largest ``c_pc_contact`` value over the map's joints is >= it
    weigh 0 - what the contact map marks stays reachable.  ``scale``: a float or a [B] tensor.  ``t_start`` as for the other terms.
    Read from ``model_kwargs``: ``c_pc_xyz`` [B, N, 3], ``x_mask``, and ``c_pc_contact`` [B, N, J] only with ``exempt_contact``.

    With p[b,f,k,:] the positions the other terms compute, q the scene points and w[b,n] the obstacle weight, float32, each operation
    rounded on its own, ir2[k] = float32(1 / r_k^2) and coef_k = float32(4 / r_k^2) formed in float64 and rounded once:

        d = p - q_n;  d2 = (dx*dx + dy*dy) + dz*dz;  u = max(0, 1 - d2 * ir2[k]);  wu = w * u
        E[b]       = sum over valid frames f, joints k, points n of  wu * u          (not normalised)
        S[b,f,k,:] = sum_n wu * d
        columns:  grad[b,f,cols[k]+a] = ((scale[b] * coef_k) * std_a) * S_a                                             (one launch)
        h3d:      coef_k * S, rounded, carried through the adjoint of the recovery with scale[b] (three launches: recovery, clearance, adjoint)

    ``guide(x, t, **model_kwargs)`` returns -scale[b] * dE/dx - u * u and its derivative both vanish at d = r, so the gradient is
    continuous - exactly zero in every other column, in padded frames, in a sample with t >= t_start and in a joint-frame with no obstacle
    point inside its radius.  ``guide.energy(x, **model_kwargs)`` returns E [B]; a sample whose frames are all padded has E = 0.

    Order of the sums (no atomics; a function of the sample alone): the kernel runs 8 waves on tiles of 1024 points; for one joint-frame
    wave v adds, from 0 and in ascending n, the points with (n mod 1024) // 128 == v, then S = ((((((s_0 + s_1) + s_2) + s_3) + s_4) + s_5)
    + s_6) + s_7.  E[b]: blocks of 64 // K whole frames, lane i = (f - f0) * K + k adds its joint-frame's e over the blocks in order, then
    a fixed wave butterfly.  Handed as ``cond_fn`` it stays in the native loops wherever the other terms do
    (afm_cmdm_scene_guide_loop_range); `MotionGuidance` sums it with them."""
    _NAME = "SceneClearance"

    def __init__(self, cols, mean: torch.Tensor, std: torch.Tensor, *, radius, scale=1.0, t_start: Optional[int] = None, weight=None,
                 up: int = 2, min_height: Optional[float] = None, exempt_contact: Optional[float] = None):
        self._init(cols, None, None, mean, std, scale, t_start, radius=radius, weight=weight, up=up, min_height=min_height,
                   exempt_contact=exempt_contact)

    @classmethod
    def h3d(cls, joints, mean: torch.Tensor, std: torch.Tensor, *, radius, to_scene: Optional[torch.Tensor] = None, scale=1.0,
            t_start: Optional[int] = None, weight=None, up: int = 2, min_height: Optional[float] = None,
            exempt_contact: Optional[float] = None) -> "SceneClearance":
        """The clearance of a HumanML3D-feature motion (``data_repr`` "h3d", D >= 67): ``joints`` are joint indices 0..21, ``to_scene`` a
        float32 [3, 4] or [B, 3, 4] tensor [A|t] on the samples' device (None: identity).  See the class docstring."""
        self = cls.__new__(cls)
        self._init(None, joints, to_scene, mean, std, scale, t_start, radius=radius, weight=weight, up=up, min_height=min_height,
                   exempt_contact=exempt_contact)
        return self

    def _own(self, radius, weight, up, min_height, exempt_contact) -> tuple:
        who, K = self._who, self.K
        try:
            r = [float(radius)] * K if not hasattr(radius, "__len__") else [float(v) for v in radius]
        except (TypeError, ValueError):
            raise ValueError(f"{who}: radius must be a positive float or {K} of them, got {radius!r}") from None
        if len(r) != K:
            raise ValueError(f"{who}: radius must be a positive float or {K} of them, got {len(r)}")
        if not all(v > 0.0 and v < float("inf") for v in r):
            raise ValueError(f"{who}: every radius must be positive, got {r}")
        if int(up) not in (0, 1, 2):
            raise ValueError(f"{who}: up names a coordinate 0..2, got {up!r}")
        if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dim() != 2 or not weight.is_floating_point()):
            raise ValueError(f"{who}: weight must be a floating [B, N] tensor, got {tuple(getattr(weight, 'shape', ()))}")
        self.radius, self.up = r, int(up)
        self.min_height = None if min_height is None else float(min_height)
        self.exempt_contact = None if exempt_contact is None else float(exempt_contact)
        self.weight = None if weight is None else ffi.f32c(weight.detach())
        return () if self.weight is None else (self.weight,)

    def describe(self, x: torch.Tensor, model_kwargs, diffusion=None, *, shared=None, long=None) -> tuple:
        """(afm_scene_clearance of this sample tensor and these conditions, x_mask as uint8 or None, what must stay alive with it).
        ``shared``: the (mean, std, to_scene, stride) device tensors of the term in front of it in a sum - a sum names one set of them.
        ``long`` = (G, F), `LongGuidance`'s: x holds the windows of G long motions - q / weight / c stay per window, scale and to_scene are
        per long motion, x_mask is not read."""
        who = self._who
        self._check_sample(x)
        if "c_pc_xyz" not in model_kwargs:
            raise ValueError("SceneClearance reads c_pc_xyz from model_kwargs")
        B, q, c = x.shape[0], model_kwargs["c_pc_xyz"], None
        if q.dim() != 3 or q.shape[0] != B or q.shape[2] != 3:
            raise ValueError(f"SceneClearance: c_pc_xyz must be [{B}, N, 3], got {tuple(q.shape)}")
        N = q.shape[1]
        if self.exempt_contact is not None:
            if model_kwargs.get("c_pc_contact") is None:
                raise ValueError("SceneClearance: exempt_contact reads c_pc_contact from model_kwargs")
            c = model_kwargs["c_pc_contact"]
            if c.dim() != 3 or tuple(c.shape[:2]) != (B, N) or c.shape[2] < 1:
                raise ValueError(f"SceneClearance: c_pc_contact must be [{B}, {N}, J], got {tuple(c.shape)}")
        if self.weight is not None and tuple(self.weight.shape) != (B, N):
            raise ValueError(f"{who}: weight is {tuple(self.weight.shape)}, the scene needs [{B}, {N}]")
        rows = B if long is None else long[0]
        scale_fits(self.scale, rows, who)
        fm = _guide_mask(x, model_kwargs, who) if long is None else None
        ts, stride = self._to_scene_on(rows, x.device)
        ffi.require_gpu(x, q, c)
        own = self._on(x.device)
        mean, std, weight = own[0], own[1], own[2] if len(own) > 2 else None
        scale = scale_row(self.scale, rows, x.device, who)
        q, c = ffi.f32c(q), None if c is None else ffi.f32c(c)
        if shared is not None:
            mean, std = shared[0], shared[1]
            if self.joints is not None:
                ts, stride = shared[2], shared[3]
        g = ffi.SceneClearance()
        lay = self._fill(g, mean, std, scale, ts, stride, diffusion)
        g.q, g.weight, g.N, g.up = q.data_ptr(), ffi.ptr(weight), N, self.up
        g.radius[:self.K] = self.radius
        if c is not None:
            g.c, g.Kc, g.exempt, g.c_min = c.data_ptr(), c.shape[2], 1, self.exempt_contact
        if self.min_height is not None:
            g.has_min_height, g.min_height = 1, self.min_height
        return g, fm, (q, c, weight, mean, std, scale, fm, lay, ts)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        return MotionGuidance(clearance=self)(x, t, **model_kwargs)

    def energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        g, fm, keep = MotionGuidance(clearance=self).describe(x, model_kwargs)
        return ops.scene_guidance(g, x, fm, grad=False, energy=True)[3]


class FootGrounding(_JointTerm):
    """A ``cond_fn`` that keeps the feet honest: no joint below the floor, no planted foot sliding over it - the one term that couples
    frame f with frame f + 1 (afm_ground_guidance, HIP; no network, no autograd).  The harder the other terms pull or push, the more a
    planted foot skates; this term holds it.

    ``cols``: K ints (K <= 16) as for `ContactGuidance`; ``FootGrounding.h3d(joints, mean, std, to_scene=None, ...)`` names joints 0..21
    of a HumanML3D-feature motion instead (the feet are 7, 10 - left ankle, left toes - and 8, 11).  ``floor``: the floor's height along
    ``up`` (0..2).  ``height``: a positive float or K of them - a joint counts as planted at the floor and as free at ``floor + height``.
    ``floor_weight`` / ``skate_weight``: both >= 0, not both 0.  ``contact``: "height" (the pair weights come from the joints' heights) or
    "labels" (``.h3d`` only: they are the motion's own foot-contact columns).  ``scale``: a float or a [B] tensor.  ``t_start`` as for the
    other terms.  Read from ``model_kwargs``: ``x_mask``.

    With p[b,f,k,:] the positions the other terms compute, float32, each operation rounded on its own, ih[k] = float32(1 / height_k),
    fw / sw = float32 of the weights, cf = float32(2 * floor_weight) and cs = float32(2 * skate_weight) formed in float64 and rounded once,
    a < b the two axes that are not ``up``:

        h      = p[b,f,k,up] - float32(floor);   pen = max(0, -h);   g = min(1, max(0, 1 - h * ih[k]))
        s[f,k] = g[f,k] * g[f+1,k]  if the frames f and f + 1 are both valid, else 0                           (contact="height")
        s[f,k] = min(1, max(0, x[b,f,259+slot(k)] * std + mean))  under the same validity rule                 (contact="labels")
        dl_a   = p[b,f+1,k,a] - p[b,f,k,a]
        E[b]   = sum over valid f, k of  fw * (pen * pen) + sw * (s[f,k] * (dl_a * dl_a + dl_b * dl_b))
        m[f,k,up] = cf * pen;   m[f,k,a] = cs * (s[f,k] * dl_a[f] - s[f-1,k] * dl_a[f-1])    (a missing or invalid pair contributes 0)
        columns:  grad[b,f,cols[k]+a] = (scale[b] * std_a) * m_a                                                (one launch)
        h3d:      m, carried through the adjoint of the recovery with scale[b] (three launches: recovery, grounding, adjoint)

    ``guide(x, t, **model_kwargs)`` returns -scale[b] * dE/dx WITH THE PAIR WEIGHTS s HELD CONSTANT.  That is on purpose: differentiating
    s would lift a sliding foot out of contact to escape the penalty; with s held the foot is slowed down where it is.  The floor part is
    the exact gradient.  The result is exactly zero in every other column, in padded frames, in a sample with t >= t_start, in a sample
    without a valid frame and in a joint-frame that neither penetrates the floor nor belongs to a pair with s > 0.
    ``guide.energy(x, **model_kwargs)`` returns E [B]; a sample whose frames are all padded has E = 0.

    ``contact="labels"``: HumanML3D's feature layout puts the left foot (joints 7 and 10) before the right one (8 and 11) in its
    foot-contact columns 259..262, so slot = {7: 0, 10: 1, 8: 2, 11: 3}; the label of frame f describes the step f -> f + 1, which is why
    it weights that pair.  The convention is HumanML3D's own and is NOT pinned by the reference project, which holds no code that reads
    these columns.  It needs the ``.h3d`` form, D >= 263 and joints out of {7, 10, 8, 11}.

    Every element of the gradient is one expression of the sample's own values (no sum across threads).  Order of the energy's sum (no
    atomics; bit-identical run to run; a function of the sample alone): one block of 256 threads per sample, thread i adds from 0 the
    items e = f * K + k = i, i + 256, ... in that order (a padded frame's item is skipped), then the fixed butterfly of each wave and
    ((r0 + r1) + r2) + r3 over the four waves.  Handed as ``cond_fn`` it stays in the native loops wherever
    the other terms do (afm_cmdm_ground_guide_loop_range); `MotionGuidance` sums it with them.  Stitched chains (`LongGuidance`) do not
    take it yet."""
    _NAME = "FootGrounding"

    def __init__(self, cols, mean: torch.Tensor, std: torch.Tensor, *, floor: float = 0.0, height=0.05, up: int = 2, floor_weight: float = 1.0,
                 skate_weight: float = 1.0, contact: str = "height", scale=1.0, t_start: Optional[int] = None):
        self._init(cols, None, None, mean, std, scale, t_start, floor=floor, height=height, up=up, floor_weight=floor_weight,
                   skate_weight=skate_weight, contact=contact)

    @classmethod
    def h3d(cls, joints, mean: torch.Tensor, std: torch.Tensor, *, to_scene: Optional[torch.Tensor] = None, floor: float = 0.0, height=0.05,
            up: int = 2, floor_weight: float = 1.0, skate_weight: float = 1.0, contact: str = "height", scale=1.0,
            t_start: Optional[int] = None) -> "FootGrounding":
        """The grounding of a HumanML3D-feature motion (``data_repr`` "h3d", D >= 67; ``contact="labels"``: D >= 263): ``joints`` are joint
        indices 0..21, ``to_scene`` a float32 [3, 4] or [B, 3, 4] tensor [A|t] on the samples' device (None: identity; ``up`` names an axis
        of the scene).  See the class docstring."""
        self = cls.__new__(cls)
        self._init(None, joints, to_scene, mean, std, scale, t_start, floor=floor, height=height, up=up, floor_weight=floor_weight,
                   skate_weight=skate_weight, contact=contact)
        return self

    def _own(self, floor, height, up, floor_weight, skate_weight, contact) -> tuple:
        who, K = self._who, self.K
        try:
            h = [float(height)] * K if not hasattr(height, "__len__") else [float(v) for v in height]
        except (TypeError, ValueError):
            raise ValueError(f"{who}: height must be a positive float or {K} of them, got {height!r}") from None
        if len(h) != K:
            raise ValueError(f"{who}: height must be a positive float or {K} of them, got {len(h)}")
        if not all(v > 0.0 and v < float("inf") for v in h):
            raise ValueError(f"{who}: every height must be positive, got {h}")
        if int(up) not in (0, 1, 2):
            raise ValueError(f"{who}: up names a coordinate 0..2, got {up!r}")
        fw, sw, fl = float(floor_weight), float(skate_weight), float(floor)
        if not (0.0 <= fw < float("inf") and 0.0 <= sw < float("inf")):
            raise ValueError(f"{who}: floor_weight and skate_weight must be >= 0, got {floor_weight!r} and {skate_weight!r}")
        if fw == 0.0 and sw == 0.0:
            raise ValueError(f"{who}: floor_weight and skate_weight are both 0 - the term would do nothing")
        if fl != fl or abs(fl) == float("inf"):
            raise ValueError(f"{who}: floor must be a finite height, got {floor!r}")
        if contact not in ("height", "labels"):
            raise ValueError(f"{who}: contact must be 'height' or 'labels', got {contact!r}")
        if contact == "labels":
            if self.joints is None:
                raise ValueError(f"{who}: contact='labels' reads HumanML3D's foot-contact columns - it needs FootGrounding.h3d")
            if self.D < ffi.GROUND_LABEL_COL + 4:
                raise ValueError(f"{who}: contact='labels' reads columns {ffi.GROUND_LABEL_COL}..{ffi.GROUND_LABEL_COL + 3}, the motion vector "
                                 f"has {self.D}")
            bad = [j for j in self.joints if j not in ffi.GROUND_LABEL_SLOT]
            if bad:
                raise ValueError(f"{who}: contact='labels' has labels for the joints 7, 10, 8 and 11 only, got {bad}")
        self.floor, self.height, self.up, self.floor_weight, self.skate_weight, self.contact = fl, h, int(up), fw, sw, contact
        return ()

    def describe(self, x: torch.Tensor, model_kwargs, diffusion=None, *, shared=None) -> tuple:
        """(afm_foot_grounding of this sample tensor and these conditions, x_mask as uint8 or None, what must stay alive with it).
        ``shared``: the (mean, std, to_scene, stride) device tensors of the term in front of it in a sum - a sum names one set of them."""
        who = self._who
        self._check_sample(x)
        B, L = x.shape[0], x.shape[1]
        if ((3 * self.K + 1) * L) * 4 > ffi.GUIDE_LDS_BYTES:
            raise ValueError(f"{who}: the kernel keeps (3 K + 1) * L floats in LDS - {L} frames of {self.K} joints are beyond "
                             f"{ffi.GUIDE_LDS_BYTES} bytes")
        scale_fits(self.scale, B, who)
        fm = _guide_mask(x, model_kwargs, who)
        ts, stride = self._to_scene_on(B, x.device)
        ffi.require_gpu(x)
        mean, std = self._on(x.device)
        scale = scale_row(self.scale, B, x.device, who)
        if shared is not None:
            mean, std = shared[0], shared[1]
            if self.joints is not None:
                ts, stride = shared[2], shared[3]
        g = ffi.FootGrounding()
        lay = self._fill(g, mean, std, scale, ts, stride, diffusion)
        g.up, g.labels, g.floor, g.floor_weight, g.skate_weight = self.up, int(self.contact == "labels"), self.floor, self.floor_weight, self.skate_weight
        g.height[:self.K] = self.height
        return g, fm, (None, None, mean, std, scale, fm, lay, ts)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        return MotionGuidance(feet=self)(x, t, **model_kwargs)

    def energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        return MotionGuidance(feet=self).feet_energy(x, **model_kwargs)


class MotionGuidance:
    """The sum of a `ContactGuidance`, a `JointTargets`, a `SceneClearance` and a `FootGrounding` as one ``cond_fn`` (each may be None, not all):
    grad = ((grad_contact + grad_targets) + grad_clearance) + grad_feet in that order, each term the float32 result of that guidance alone,
    joined by one rounded addition per element - ``MotionGuidance(contact, targets)(x, t, **kw)`` equals ``contact(x, t, **kw) +
    targets(x, t, **kw)`` bit for bit, with a clearance ``... + clearance(x, t, **kw)`` and with a grounding ``... + feet(x, t, **kw)``.
    Each term keeps its
    own ``scale`` and ``t_start``: a sample (step by step) or a step (native loops) a term does not guide gets exactly zero from it.  The
    terms describe one motion: the same ``mean`` / ``std``, all on columns or all on HumanML3D features, the same ``to_scene`` -
    ValueError otherwise.  The joint lists may differ; an h3d motion is recovered once per term.  Launches per guided step: the contact
    term's 2 (h3d: 4) plus the targets' 1 (h3d: 3) plus the clearance's 1 (h3d: 3) plus the grounding's 1 (h3d: 3).  ``energies(x, **kw)``
    returns (E_contact or None, E_targets or None); the clearance's value is ``guide.clearance.energy(x, **kw)``, the grounding's
    ``guide.feet_energy(x, **kw)``.  A sum without a grounding reaches the entry it reached before there was one."""

    def __init__(self, contact: Optional[ContactGuidance] = None, targets: Optional[JointTargets] = None,
                 clearance: Optional[SceneClearance] = None, feet: Optional["FootGrounding"] = None):
        if contact is None and targets is None and clearance is None and feet is None:
            raise ValueError("MotionGuidance: at least one of contact / targets / clearance / feet")
        if feet is not None and not isinstance(feet, FootGrounding):
            raise TypeError(f"MotionGuidance: feet must be a FootGrounding, not {type(feet).__name__}")
        if contact is not None and not isinstance(contact, ContactGuidance):
            raise TypeError(f"MotionGuidance: contact must be a ContactGuidance, not {type(contact).__name__}")
        if targets is not None and not isinstance(targets, JointTargets):
            raise TypeError(f"MotionGuidance: targets must be a JointTargets, not {type(targets).__name__}")
        if clearance is not None and not isinstance(clearance, SceneClearance):
            raise TypeError(f"MotionGuidance: clearance must be a SceneClearance, not {type(clearance).__name__}")
        terms = [g for g in (contact, targets, clearance, feet) if g is not None]
        for first, other in zip(terms, terms[1:]):
            if first.D != other.D or not torch.equal(first.mean.cpu(), other.mean.cpu()) or not torch.equal(first.std.cpu(), other.std.cpu()):
                raise ValueError("MotionGuidance: the two terms de-normalise the motion with different mean / std")
            if (first.joints is None) != (other.joints is None):
                raise ValueError("MotionGuidance: one term names columns of absolute positions, the other joints of HumanML3D features")
            a, b = first.to_scene, other.to_scene
            if (a is None) != (b is None) or (a is not None and a is not b and (a.shape != b.shape or a.device != b.device or not torch.equal(a.cpu(), b.cpu()))):          # (compared on the host: no device arithmetic)
                raise ValueError("MotionGuidance: the two terms place the motion in the scene with different to_scene transforms")
        self.contact, self.targets, self.clearance, self.feet = contact, targets, clearance, feet

    def _terms(self) -> list:
        return [g for g in (self.contact, self.targets, self.clearance, self.feet) if g is not None]

    @property
    def t_start(self):
        """None if any term guides every step, else the latest start"""
        ts = [g.t_start for g in self._terms()]
        return None if any(t is None for t in ts) else max(ts)

    def describe(self, x: torch.Tensor, model_kwargs, diffusion: Optional["GaussianDiffusion"] = None) -> tuple:
        """(afm_motion_guide - with a clearance: afm_scene_guide, with a grounding: afm_ground_guide - of this sample tensor and these
        conditions, x_mask as uint8 or None, what must stay alive with it).  With ``diffusion``: each term's first_guided set for a chain on it (the loops)."""
        cg = tg = fm = shared = None
        keep = []
        if self.contact is not None:
            cg, fm, ck = self.contact.describe(x, model_kwargs, diffusion)
            keep.append((cg, ck))
            shared = (ck[2], ck[3], ck[7], cg.h3d.contents.to_scene_stride if cg.h3d else 0)
        if self.targets is not None:
            tg, fm, tk = self.targets.describe(x, model_kwargs, diffusion, shared=shared)
            keep.append((tg, tk))
            shared = (tk[2], tk[3], tk[7], tg.h3d.contents.to_scene_stride if tg.h3d else 0)
        g = ffi.MotionGuide()
        if cg is not None:
            g.contact = C.pointer(cg)
        if tg is not None:
            g.targets = C.pointer(tg)
        if self.clearance is None and self.feet is None:
            return g, fm, keep
        s = None
        if self.clearance is not None:
            sg, fm, sk = self.clearance.describe(x, model_kwargs, diffusion, shared=shared)
            keep.append((sg, sk, g))
            shared = (sk[3], sk[4], sk[8], sg.h3d.contents.to_scene_stride if sg.h3d else 0)
            s = ffi.SceneGuide()
            s.clearance = C.pointer(sg)
            if cg is not None or tg is not None:
                s.terms = C.pointer(g)
        elif cg is not None or tg is not None:
            s = ffi.SceneGuide()
            s.terms = C.pointer(g)
        if self.feet is None:
            return s, fm, keep
        fg, fm, fk = self.feet.describe(x, model_kwargs, diffusion, shared=shared)
        keep.append((fg, fk, g, s))
        r = ffi.GroundGuide()
        r.feet = C.pointer(fg)
        if s is not None:
            r.terms = C.pointer(s)
        return r, fm, keep

    def first_guided(self, diffusion: "GaussianDiffusion") -> int:
        """the first executed step of a chain on ``diffusion`` that carries any term"""
        return min(g.first_guided(diffusion) for g in self._terms())

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        g, fm, keep = self.describe(x, model_kwargs)
        timed = any(q.t_start is not None for q in self._terms())
        run = ops.ground_guidance if self.feet is not None else ops.motion_guidance if self.clearance is None else ops.scene_guidance
        return run(g, x, fm, t.to(x.device) if timed else None)[0]

    def energies(self, x: torch.Tensor, **model_kwargs) -> tuple:
        if self.contact is None and self.targets is None:
            return None, None
        g, fm, keep = MotionGuidance(self.contact, self.targets).describe(x, model_kwargs)
        return ops.motion_guidance(g, x, fm, grad=False, energy=True)[1:]

    def feet_energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        """E_feet [B] of the grounding term (see `FootGrounding`)"""
        if self.feet is None:
            raise ValueError("MotionGuidance: feet_energy needs a grounding term")
        g, fm, keep = MotionGuidance(feet=self.feet).describe(x, model_kwargs)
        return ops.ground_guidance(g, x, fm, grad=False, energy=True)[4]


class LongGuidance:
    """A ``cond_fn`` for chains that run with ``stitch=``: a `ContactGuidance`, a `JointTargets` and / or a `SceneClearance` evaluated on the JOINED long motion
    (afm_long_guidance, HIP), so a long motion is pulled to its own contact maps, and a root path or a target may lie beyond the first
    window - on HumanML3D features the root is integrated from long frame 0, not from each window's own origin.  In a stitched chain the
    shared frames are bit-identical in both windows at every step, so the windows join into one long x_t; the gradient goes back to the
    windows as one value per long frame, both copies of a shared frame receive the same bits and the stitching invariant survives.

    ``stitch``: a `Stitch` with S windows, overlap ov and F frames; hop = L - ov.  Window w of long motion g is batch row b = g * S + w and
    holds the long frames a_w = w * hop .. a_w + L - 1, clipped to < F.  ``contact``: a `ContactGuidance`, column form or ``.h3d``.
    ``targets``: a `JointTargets` whose ``target`` / ``weight`` are in the long form [G, F, K, 3] / [G, F, K].  The two terms must agree as
    `MotionGuidance` requires (same mean / std, same form, same ``to_scene``).  ``scale`` of each term is a float or a [G] tensor, one per
    long motion - a [G * S] tensor is a ValueError.  ``to_scene`` is [3, 4] or [G, 3, 4].  ``x_mask`` is not read: validity is the geometry
    - long frames 0 .. F-1 are valid, and the padded tail of a last window does not exist in the long form.  ``c_pc_xyz`` [G * S, N, 3] and
    ``c_pc_contact`` [G * S, N, K] are read from ``model_kwargs`` per window: each window keeps its own map.

    ``guide(x, t, **model_kwargs)`` takes x [G * S, L, D] and returns grad [G * S, L, D] float32:

      1. long = `Stitch.join` (x) [G, F, D]; the join rule stands: a shared frame is read from the later window.
      2. P[g,f,k,:] are the positions of ``long`` exactly as the existing kernels compute them - the de-normalised columns, or the h3d
         recovery over all F frames.  float32, every operation in its present order.
      3. Targets term: the existing afm_motion_guidance targets launches on (long, B = G, L = F) - by definition ``targets(long, ...)``.
      4. Contact term, for each window b: d2[b,n,k] = min over the window's long frames f of |P[g,f,k] - q[b,n]|^2, summed
         (dx*dx + dy*dy) + dz*dz; f* the first such frame, stored as a long frame index; chat and w as `ContactGuidance`;
         E_b = sum (chat - c)^2 / (N K) with the existing partial and serial sums; S_b[f,k,:] = sum over {n: f*(b,n,k) = f} of w * (p - q)
         in the existing frame_sum order.
      5. Per long frame the windows' sums are joined: a frame in one window takes that window's sum as is, a frame in two windows takes
         S_earlier + S_later - one rounded addition, earlier window first.
      6. Column form: grad_long[g,f,col+a] = ((scale[g] * coef) * std_a) * S.  h3d form: the joined S goes through the existing adjoint
         kernel on (B = G, L = F) with scale[g].
      7. The targets' launch adds its complete result to what the contact term wrote, as `MotionGuidance` does.
      8. grad = `Stitch.windows_of` (grad_long): the padded tail is exact zeros, both copies of a shared frame hold the same bits.

    ``energies(x, **kw)`` returns (E_contact [G], E_targets [G]) (None for a term that is not set); E_contact[g] is the serial sum of its
    windows' E_b in window order.  ``t_start`` and ``first_guided`` work per term as in `MotionGuidance`; t of long motion g is t[g * S].
    ValueError before anything runs: a batch or L that does not match ``stitch``, long-form shapes that do not match, F beyond what 7 * F
    floats of LDS allow for the h3d recovery, a term with a per-window scale.

    ``clearance``: a `SceneClearance` (column form or ``.h3d``) as a third term (afm_long_scene_guidance, HIP).  Each window clears ITS OWN
    frames of the joined motion against ITS OWN scene: ``c_pc_xyz`` [G * S, N, 3], the term's ``weight`` [G * S, N] (row g * S + w) and - with
    ``exempt_contact`` - ``c_pc_contact`` [G * S, N, J] are per window, so the window "sit down" exempts the sofa its contact map marks and the
    window "walk" does not; ``scale`` is a float or [G], ``to_scene`` [3, 4] or [G, 3, 4].  Per window b and each of its long frames f, with
    p = P[g,f,k,:], d, d2, u and wu are formed exactly as `SceneClearance` forms them and

        S_b[f,k,:] = sum_n wu * d,   e_b[f,k] = sum_n wu * u          (the clearance kernel's order: eight spans of 128 of every 1024 points)

    Per long frame the windows' sums are crossfaded with the stitch's own weight row: with w1 = min(f // hop, S - 1), the earlier window
    w1 - 1 also holds f iff w1 > 0 and i = f - w1 * hop < ov;

        one window:   J[g,f,k,:] = S_b[f,k,:]                                  (the bits as they are)
        two windows:  J[g,f,k,:] = (wl[i] * S_earlier) + (wr[i] * S_later)     float32, each product rounded, then the sum

    (the contact term's plain sum would push twice as hard inside every overlap of one room; identical clouds in both windows give the
    single-scene push up to rounding; an exemption fades out as the next action fades in).  Column form:
    grad_long[g,f,cols[k]+a] = ((scale[g] * coef_k) * std_a) * J_a; h3d form: coef_k * J_a, rounded, goes through the adjoint kernel on
    (B = G, L = F) with scale[g].  With S == 1, F == L and no mask this is `SceneClearance` on the one window, bit for bit.  The sum is
    grad_long = (grad_contact + grad_targets) + grad_clearance - the clearance's last launch adds its complete result to what the terms in
    front of it wrote, one rounded addition per element - then step 8.  Exact zeros: every unnamed column, the padded tail, a long motion
    with t >= t_start, a joint-frame with no obstacle point inside its radius in any window that holds it.
    ``clearance_energy(x, **kw)`` returns E_clearance [G] with grad = -scale * dE/dx: a joint-frame's e_b times its frame weight (1 outside
    overlaps, wl[i] / wr[i] in the earlier / later window), summed per window as `SceneClearance` sums a sample (blocks of 64 // K whole
    frames, a frame at or behind F counting 0), the windows' values added in window order.  ``energies`` keeps its 2-tuple.  Also a
    ValueError before anything runs: a clearance ``weight`` whose rows are not the windows'.

    Handed as ``cond_fn`` to ``ddim_sample_loop(..., stitch=)`` / ``dpm_solver_sample_loop(..., stitch=)`` with the same `Stitch` geometry; a
    CMDM `trans_enc` or a GuidedCMDM runs the whole chain natively (afm_cmdm_long_guide_loop_range; with a clearance:
    afm_cmdm_long_scene_guide_loop_range).  Launches per guided step: join + the contact term's 2 (h3d: 4) + the targets' 1 (h3d: 3) + the
    clearance's 2 (h3d: 4) + windows."""

    def __init__(self, stitch: Stitch, contact: Optional[ContactGuidance] = None, targets: Optional[JointTargets] = None,
                 clearance: Optional[SceneClearance] = None):
        if not isinstance(stitch, Stitch):
            raise TypeError(f"LongGuidance: stitch must be a Stitch, not {type(stitch).__name__}")
        for term in (contact, targets, clearance):
            if isinstance(term, FootGrounding):
                raise ValueError("LongGuidance: a FootGrounding is not evaluated on the joined long motion yet - stitched chains take contact, "
                                 "targets and clearance only")
        self.stitch = stitch
        self._sum = MotionGuidance(contact, targets, clearance)          # (the terms' types and their agreement, checked once)
        self.contact, self.targets, self.clearance = contact, targets, clearance

    @property
    def t_start(self):
        return self._sum.t_start

    def first_guided(self, diffusion) -> int:
        return self._sum.first_guided(diffusion)

    def same_geometry(self, stitch: Stitch) -> bool:
        """whether a chain's `Stitch` cuts the long motions as this guidance's does"""
        a, b = self.stitch, stitch
        return a is b or (a.windows, a.overlap, a.frames, a.length) == (b.windows, b.overlap, b.frames, b.length)

    def check(self, x: torch.Tensor) -> tuple:
        """the windows x [G * S, L, D] against the stitch and the terms, on the host (ValueError); -> (G, F)"""
        who = "LongGuidance"
        if x.dim() != 3:
            raise ValueError(f"{who}: the windows are [G * S, L, D], got {tuple(x.shape)}")
        B, L, _ = x.shape
        F = self.stitch.check(B, L)
        S = self.stitch.windows
        G = B // S
        for term in (self.contact, self.targets, self.clearance):
            if term is None:
                continue
            term._check_sample(x)
            if isinstance(term.scale, torch.Tensor) and term.scale.numel() != G:
                if S > 1 and term.scale.numel() == B:
                    raise ValueError(f"{who}: the {term._NAME}'s `scale` holds one value per window ({B}); a long motion has one scale, [{G}]")
                raise ValueError(f"{who}: the {term._NAME}'s `scale` holds {term.scale.numel()} values for {G} long motions")
            if term.joints is not None and ffi.H3D_SCAN_ROWS * F * 4 > ffi.GUIDE_LDS_BYTES:
                raise ValueError(f"{who}: the joint recovery keeps {ffi.H3D_SCAN_ROWS} * F floats in LDS - {F} frames are beyond "
                                 f"{ffi.GUIDE_LDS_BYTES // (4 * ffi.H3D_SCAN_ROWS)}")
            if term.to_scene is not None and term.to_scene.dim() == 3 and term.to_scene.shape[0] != G:
                raise ValueError(f"{who}: to_scene holds {term.to_scene.shape[0]} matrices for {G} long motions")
        tg = self.targets
        if tg is not None and tuple(tg.target.shape) != (G, F, tg.K, 3):
            raise ValueError(f"{who}: the targets are long-form - target [{G}, {F}, {tg.K}, 3] and weight [{G}, {F}, {tg.K}], got "
                             f"{tuple(tg.target.shape)} and {tuple(tg.weight.shape)}")
        sc = self.clearance
        if sc is not None and sc.weight is not None and sc.weight.shape[0] != B:
            raise ValueError(f"{who}: the SceneClearance's weight is per window, [{B}, N] - row g * {S} + w weighs window w's cloud -, got "
                             f"{tuple(sc.weight.shape)}")
        return G, F

    def describe(self, x: torch.Tensor, model_kwargs, diffusion=None) -> tuple:
        """(afm_long_guide - with a clearance: afm_long_scene_guide - of these windows and conditions, None - no frame mask is read -,
        what must stay alive with it).  With ``diffusion``: each term's first_guided set for a chain on it (the loops)."""
        long = self.check(x)
        cg = tg = shared = None
        keep = []
        if self.contact is not None:
            cg, _, ck = self.contact.describe(x, model_kwargs, diffusion, long=long)
            keep.append((cg, ck))
            shared = (ck[2], ck[3], ck[7], cg.h3d.contents.to_scene_stride if cg.h3d else 0)
        if self.targets is not None:
            tg, _, tk = self.targets.describe(x, model_kwargs, diffusion, shared=shared, long=long)
            keep.append((tg, tk))
            shared = (tk[2], tk[3], tk[7], tg.h3d.contents.to_scene_stride if tg.h3d else 0)
        m = ffi.MotionGuide()
        if cg is not None:
            m.contact = C.pointer(cg)
        if tg is not None:
            m.targets = C.pointer(tg)
        st, st_keep = self.stitch.describe(x.device)
        g = ffi.LongGuide()
        g.terms, g.stitch, g.frames = C.pointer(m), st, long[1]
        if self.clearance is None:
            return g, None, (m, keep, st_keep)
        sg, _, sk = self.clearance.describe(x, model_kwargs, diffusion, shared=shared, long=long)
        s = ffi.LongSceneGuide()
        s.base, s.clearance = C.pointer(g), C.pointer(sg)
        return s, None, (m, keep, st_keep, g, sg, sk)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        g, _, keep = self.describe(x, model_kwargs)
        run = ops.long_guidance if self.clearance is None else ops.long_scene_guidance
        return run(g, x, t.to(x.device) if self._timed() else None)[0]

    def _timed(self) -> bool:
        return any(q is not None and q.t_start is not None for q in (self.contact, self.targets, self.clearance))

    def energies(self, x: torch.Tensor, **model_kwargs) -> tuple:
        if self.contact is None and self.targets is None:
            return None, None
        g, _, keep = LongGuidance(self.stitch, self.contact, self.targets).describe(x, model_kwargs)
        return ops.long_guidance(g, x, grad=False, energy=True)[1:]

    def clearance_energy(self, x: torch.Tensor, **model_kwargs) -> torch.Tensor:
        """E_clearance [G] of the windows x: the windows' omega-weighted energies added in window order (see the class docstring)"""
        if self.clearance is None:
            raise ValueError("LongGuidance: clearance_energy needs a clearance term")
        g, _, keep = LongGuidance(self.stitch, clearance=self.clearance).describe(x, model_kwargs)
        return ops.long_scene_guidance(g, x, grad=False, energy=True)[3]
