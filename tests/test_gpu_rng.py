"""`-m gpu`: the noise generator (afm_randn, the in-kernel draw of the sampling update) and the dropout keep-mask (afm_rowop, the
attention kernels) against the numpy restatements of oracle/rng_ref.py, which tests/test_rng_host.py pins to the published Philox vectors
and to the normal / binomial laws.  The integer stages must agree exactly (a wiring fault moves values by O(1)); the float stage of the
noise is held to the error class of the float32 numpy chain (gpu_util.report_f32_class).

Margin 16, not the project's 4: the kernel evaluates the logarithm and the sine / cosine with the hardware approximations (__logf,
__sincosf), whose error on this chain nobody had measured; the float32 numpy chain's own max error is about 6e-7, the float32 range
reduction of an angle up to 2 pi alone allows about 4 x that at |r| = 6.8, and any wiring fault gives errors of 1e-2 and up: three decades
of headroom.  The measured ratios are committed as profiles/rng_adamw_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from afm import autograd as AG
from afm import ffi, ops
from gpu_util import dev, report_f32_class, write_parity_table
from oracle import rng_ref as R

pytestmark = pytest.mark.gpu

OLD_TOL, MARGIN = 1e-4, 16
Z_MAX = 6.764                    # sqrt(-2 ln 2^-33) = 6.7638: the largest radius the generator can produce
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rng_edges.json")
GUARD = 64                     # floats behind the output that must stay untouched


def guarded(B, per):
    """A [B, per] view at the head of a NaN-filled buffer GUARD floats longer: a store behind the last element is seen, and stays in bounds."""
    buf = torch.full((B * per + GUARD,), float("nan"), device=dev())
    return buf, buf[:B * per].view(B, per)


def check_randn(B, per, seed, sample0, step):
    buf, out = guarded(B, per)
    ffi.check(ffi.load().afm_randn(out.data_ptr(), B, per, seed, sample0, step, ffi.stream_of(out)), "afm_randn")
    assert torch.isnan(buf[B * per:]).all(), "afm_randn stored behind its output"
    assert torch.equal(ops.randn((B, per), dev(), seed=seed, sample_index0=sample0, step=step), out)
    got = out.cpu()
    z32, z64 = R.normals(seed, sample0, step, B, per)
    name = f"afm_randn ({B}, {per}) seed {seed} sample0 {sample0} step {step}"
    report_f32_class(name, got, torch.from_numpy(z32), torch.from_numpy(z64), OLD_TOL, margin=MARGIN)
    return got


# ------------------------------------------------------------------------------------------------ afm_randn
@pytest.mark.parametrize("B,per", [(3, 1315), (1, 1), (1, 3), (2, 5), (1, 4),
                                   (2, 1049779)])          # 262445 quads per sample over a grid of 262144 threads: a second pass, a partial quad
def test_randn_matches_the_restatement_at_every_shape(B, per):
    got = check_randn(B, per, 7, 0, 3)
    if per < 1315:          # a short sample is the head of a long one: the layout does not depend on per_sample
        assert torch.equal(got[0], ops.randn((1, 1315), dev(), seed=7, sample_index0=0, step=3).cpu()[0, :per])


@pytest.mark.parametrize("seed", [0, 7, 1 << 32, (1 << 64) - 1])
def test_randn_matches_the_restatement_for_every_seed_word(seed):
    check_randn(3, 1315, seed, 0, 3)


@pytest.mark.parametrize("step", [-1, 0, 999, (1 << 31) - 1])
def test_randn_matches_the_restatement_for_every_step(step):
    check_randn(3, 1315, 7, 0, step)


@pytest.mark.parametrize("B,sample0", [(3, 0), (3, 5), (4, (1 << 32) - 2)])          # the last batch crosses the 32-bit boundary of the index
def test_randn_matches_the_restatement_for_every_sample_word(B, sample0):
    check_randn(B, 1315, 7, sample0, 3)


def test_randn_at_the_ends_of_the_uniform_range():
    """The quads of tests/golden/rng_edges.json (oracle/find_rng_edges.py): a radius word below 2^10 (far tail), a radius word that rounds to
    2^32 (only the clamp keeps u below 1), an angle word that rounds to 2^32 (the angle is the float32 2 pi), a radius word whose + 0.5f
    rounds.  Each is the LAST quad of its call."""
    with open(EDGES) as f:
        tuples = json.load(f)["tuples"]
    got, w32, w64 = [], [], []
    for t in tuples:
        q = t["q"]
        out = ops.randn((1, 4 * (q + 1)), dev(), seed=t["seed"], sample_index0=t["sample"], step=t["step"])
        last = out[0, 4 * q:].cpu()
        z32, z64 = R.normal_quads(t["seed"], t["sample"], t["step"], np.array([q], np.uint64))
        print(f"[rng-edge] {''.join(t['classes'])} {t['counters']}: hip {last.tolist()} f64 {z64[0].tolist()}")
        assert torch.isfinite(last).all(), t
        assert last.abs().max().item() <= Z_MAX * (1 + 2.0 ** -20), t
        got.append(last); w32.append(torch.from_numpy(z32[0])); w64.append(torch.from_numpy(z64[0]))
        report_f32_class(f"afm_randn edge quad {''.join(t['classes'])} (seed {t['seed']} sample {t['sample']} step {t['step']} q {q})",
                         last, w32[-1], w64[-1], OLD_TOL, margin=MARGIN, record=False)
    report_f32_class("afm_randn edge quads (all)", torch.stack(got), torch.stack(w32), torch.stack(w64), OLD_TOL, margin=MARGIN)


# ------------------------------------------------------------------------------------------------ the in-kernel draw
@pytest.mark.parametrize("B,per,sample0", [(2, 1049779, 0), (4, 1315, (1 << 32) - 2)])
def test_in_kernel_draw_is_afm_randn(B, per, sample0):
    """afm_ddpm_step without a noise tensor: (0 * 0 + 0 * 0) + 1 * z is the draw of sampling_update_kernel itself."""
    zeros, one = torch.zeros(B, per, device=dev()), torch.ones(B, device=dev())
    buf, out = guarded(B, per)
    got = ops.ddpm_step(zeros, zeros, None, 0 * one, 0 * one, one, seed=7, sample_index0=sample0, step=3, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.isnan(buf[B * per:]).all(), "the sampling update stored behind its output"
    assert torch.equal(got, ops.randn((B, per), dev(), seed=7, sample_index0=sample0, step=3))


# ------------------------------------------------------------------------------------------------ the keep-mask through the kernels
@pytest.mark.parametrize("rows,cols", [(300, 512), (70001, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9, 2.0 ** -31, 0.99999994])
def test_rowop_keep_mask_is_the_restatement(rows, cols, p):
    ones = torch.ones(rows, cols, device=dev())
    for seed in (99, (1 << 64) - 1):
        for mask_id in (0, 7, (1 << 32) - 1):
            out = AG._rowop(ones, drop=(p, seed, mask_id)).cpu()
            keep, inv_keep = R.keep_mask(p, seed, mask_id, rows, cols)
            assert torch.isfinite(out).all()
            assert np.array_equal((out != 0).numpy(), keep), (p, seed, mask_id, (out != 0).float().mean().item(), keep.mean())
            assert np.array_equal(out.numpy(), np.where(keep, inv_keep, np.float32(0.0))), (p, seed, mask_id, inv_keep)


def test_attention_hands_row_and_key_to_the_mask():
    """afm_mha_fwd_train, qkv [B*T, 3*H*dh] packed q | k | v: with q = k = 0 every probability is 1/T, and with V of every head the T x T
    identity (T = dh = 64) column j of a head's output is the dropped probability of key j: keep(row = (b*H + h)*T + query, col = key) *
    inv_keep / 64."""
    B, T, H, dh, p, seed, mask_id = 2, 64, 2, 64, 0.5, 99, 7
    qkv = torch.zeros(B, T, 3 * H * dh)
    for h in range(H):
        qkv[:, :, 2 * H * dh + h * dh: 2 * H * dh + (h + 1) * dh] = torch.eye(T)
    out = AG.self_attention(qkv.to(dev()), H, (p, seed, mask_id)).cpu()
    keep, inv_keep = R.keep_mask(p, seed, mask_id, B * H * T, T)
    keep = torch.from_numpy(keep).view(B, H, T, T).permute(0, 2, 1, 3).reshape(B, T, H * T)          # [b, query, h * 64 + key]
    assert not torch.equal(keep.view(B, T, H, T)[:, :, 0], keep.view(B, T, H, T)[:, :, 0].transpose(1, 2))          # the check can see a transpose
    assert torch.isfinite(out).all()
    assert torch.equal(out != 0, keep), ((out != 0).float().mean().item(), keep.float().mean().item())
    want = keep.float() * float(inv_keep) / T
    assert (out - want).abs().max().item() <= 1e-6


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table; committed as profiles/rng_adamw_parity.json)."""
    write_parity_table()
