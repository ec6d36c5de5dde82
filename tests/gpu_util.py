"""Helpers shared by the `-m gpu` parity tests (HIP path vs the CPU oracle)."""
import json
import os

import torch

from afm import synth


def dev():
    return torch.device("cuda:0")


def to_dev(sd):
    return {k: v.to(dev()) for k, v in sd.items()}


def report(name, got, want, tol):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    print(f"[parity] {name}: max|diff|={err:.3e} (max|ref|={ref:.3e}, tol={tol:.1e})")
    assert err <= tol, f"{name}: max abs err {err:.3e} > {tol:.1e}"
    return err


def grad_forms(fn):
    """fn() the two ways a caller reaches a model's forward: with autograd enabled, where a model whose parameters require grad runs its
    training composition (the per-operator tape, afm.autograd), and under torch.no_grad(), where it runs the fused inference kernels the
    sampling loops run.  Yields (name suffix, result)."""
    yield "", fn()
    with torch.no_grad():
        out = fn()
    yield " [no_grad: inference kernels]", out


PARITY_ROWS = []          # one dict per report_f32_class call of this process, in call order (written by write_parity_table)
ULP32 = 2.0 ** -23


def to_f64(v):
    """The float64 twin of an oracle argument: floating-point tensors (and the values of a state dict / golden) cast up; integer
    timesteps, boolean masks, index tensors and everything else unchanged."""
    if isinstance(v, dict):
        return {k: to_f64(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(to_f64(x) for x in v)
    return v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v


def report_f32_class(name, got, want32, want64, old_tol, margin=4.0, select=None, record=True, floor_at=None):
    """The HIP result must lie in the error class of the float32 reference itself: with e_ref = want32 - want64 (the reference's own
    float32 rounding error against the same function in float64) and e_got = got - want64, both taken in float64 on `select`,

        max|e_got| <= margin * max|e_ref| + floor      and      rms(e_got) <= margin * rms(e_ref) + floor,

    floor = 2^-23 * max|want64|: one float32 ulp of the largest output (`got` is stored in float32); for a SUM whose partial sums exceed
    its total the caller states `floor_at`, the size of the largest partial sum in the order of the terms (every float32 evaluation rounds
    partial sums of that size at least once: tests/test_point_train_edges_host.py).  margin = 4 is the project's figure
    for "the same f32 arithmetic in another association" (test_linear_layernorm_folded_across_launches).  The bound must also lie below
    the absolute tolerance `old_tol` the calling test states for report(), otherwise it says nothing new: that is asserted first.
    Prints one `[parity-f32]` line, appends the figures to PARITY_ROWS and returns (ratio_max, ratio_rms), where
    ratio = e_got / (e_ref + floor / margin): the assertion holds exactly when both ratios are <= margin."""
    assert want64.dtype == torch.float64, f"{name}: the float64 twin is {want64.dtype}"
    got, want32, want64 = got.detach().cpu(), want32.detach().cpu(), want64.detach().cpu()
    assert got.shape == want32.shape == want64.shape, (name, got.shape, want32.shape, want64.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    if select is not None:
        select = select.cpu()
        got, want32, want64 = got[select], want32[select], want64[select]
    e_ref, e_got = want32.double() - want64, got.double() - want64
    max_ref, max_got = e_ref.abs().max().item(), e_got.abs().max().item()
    rms_ref, rms_got = e_ref.pow(2).mean().sqrt().item(), e_got.pow(2).mean().sqrt().item()
    floor = ULP32 * (want64.abs().max().item() if floor_at is None else float(floor_at))
    # (an exactly zero reference - a gradient under a saturated softmax - has no error and no floor: only an exactly zero result is in its class)
    ratio = lambda e, d: e / d if d > 0.0 else (0.0 if e == 0.0 else float("inf"))
    ratio_max, ratio_rms = ratio(max_got, max_ref + floor / margin), ratio(rms_got, rms_ref + floor / margin)
    print(f"[parity-f32] {name}: ref max {max_ref:.3e} rms {rms_ref:.3e} | hip max {max_got:.3e} rms {rms_got:.3e} | "
          f"ratio max {ratio_max:.2f} rms {ratio_rms:.2f} (margin {margin:g}, floor {floor:.1e}, old tol {old_tol:.1e})")
    if record:
        PARITY_ROWS.append(dict(name=name, max_ref=max_ref, rms_ref=rms_ref, max_got=max_got, rms_got=rms_got, ratio_max=ratio_max,
                                ratio_rms=ratio_rms, margin=margin, old_tol=old_tol))
    assert margin * max_ref + floor < old_tol, \
        f"{name}: the f32-class bound {margin * max_ref + floor:.3e} is not below the stated tolerance {old_tol:.1e} (vacuous)"
    assert max_got <= margin * max_ref + floor, \
        f"{name}: max|hip - f64| = {max_got:.3e} > {margin:g} x {max_ref:.3e} + {floor:.1e} (ratio {ratio_max:.2f})"
    assert rms_got <= margin * rms_ref + floor, \
        f"{name}: rms(hip - f64) = {rms_got:.3e} > {margin:g} x {rms_ref:.3e} + {floor:.1e} (ratio {ratio_rms:.2f})"
    return ratio_max, ratio_rms


def write_parity_table():
    """Stores what report_f32_class measured so far in this process as parity_f32_class.json (committed as
    profiles/r07_parity_f32_class.json) in the directory AFM_PARITY_OUT names, by default build/parity of the repository (not under version
    control).  Called by the last test of every module that measures; the last call holds every row."""
    if not PARITY_ROWS:
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.abspath(os.environ.get("AFM_PARITY_OUT") or os.path.join(root, "build", "parity"))
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "parity_f32_class.json")
    with open(path, "w") as f:
        json.dump({"rule": "max|hip - f64| <= margin * max|ref32 - f64| + 2^-23 max|f64|, the same for the rms; "
                           "ratio = e_hip / (e_ref + floor / margin)", "rows": PARITY_ROWS}, f, indent=1)
    return path


def load_named_weights(module, seed=synth.WEIGHT_SEED):
    """Fill a product nn.Module with the name-keyed deterministic weights (same values the oracle's
    shape tables produce for the same keys)."""
    synth.fill_module_(module, seed)
    return module
