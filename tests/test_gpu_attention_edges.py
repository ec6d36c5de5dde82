"""`-m gpu`: the attention kernels (csrc/attention.hip, csrc/attention_bwd.hip) against float64 at the mask, shape and value edges of their
case analysis.  Everything goes through afm.ops and the C entry points; nothing here knows how a kernel is built.

  masks    tests/test_attention_ref_host.py builds the key masks (and checks on the host which block flags they produce): leading runs, a
           whole key segment masked, only the upper / lower 16 keys of every block valid, every other key, Bernoulli(1/2), the unconditional
           branch of guided sampling, ONE valid key, and one sample with no valid key among three.  The samples of a launch carry different
           masks.
  shapes   T = 1 .. 289 (1 .. 10 key blocks: no merge, SEG2's idle trip at three blocks, one key in the tail block), H = 3 (a grid that is
           no multiple of 8: the remainder branch of the XCD remap) and 8, every workgroup form and q_first, B H >= 128 (the library's own
           12-wave choice), the cross form down its LDS ladder (4 / 2 / 1 waves) and its refusal.
  values   logits up to 140, near-tied keys, a spiked key late in either segment, V over 2^+-60 and around 1e20, the worst-mantissa operands
           of tests/test_gpu_arith.py - bounded by the float32 reference's OWN error (gpu_util.report_f32_class, margin 4), in all three
           arithmetics; the figures go to profiles/attention_edges_parity.json.
  training afm_mha_fwd_train / afm_mha_bwd and the cross pair over the same masks against float64 autograd."""
import contextlib
import math

import numpy as np
import pytest
import torch

from afm import ffi, ops
from gpu_util import PARITY_ROWS, dev, report, report_f32_class, write_parity_table
from oracle import attention_ref as AR
from test_attention_ref_host import LADDER, TRAIN_LAST_T, TS, batches, f32_bound, gaussian_qkv, lse_bound, patterns, single_key_mask, single_keys
from test_gpu_arith import _rng, _worst_mantissa
from test_gpu_train import _attn_ref, _mha_bwd, _mha_train, rel

pytestmark = pytest.mark.gpu

ARITHS = (("x6", 6), ("x9", 9), ("f32", 0))                      # ops.set_gemm_split: six products, nine, AFM_ARITH_F32
FORMS = (1, 2, 4, 6, 8, 12, 102, 104)                            # group_waves; a launch collapses them to the smallest group covering the query blocks
SENTINEL = 12345.0
TOL = 2e-5                                                       # the project's figure for Gaussian inputs


@contextlib.contextmanager
def arithmetic(products):
    prev = ops.set_gemm_split(products)
    try:
        yield ops.gemm_arith()[0]
    finally:
        ops.set_gemm_split(prev)


def pack(q, k, v):
    """[B, H, T, 64] x 3 -> the packed in_proj layout [B, T, 3 * 64 H]"""
    return torch.cat([AR.merge_heads(q), AR.merge_heads(k), AR.merge_heads(v)], -1).contiguous()


def pack_kv(k, v):
    return torch.cat([AR.merge_heads(k), AR.merge_heads(v)], -1).contiguous()


def mha_into(out, qkv, km, H, q_first, group_waves, arith):
    """afm_mha_fwd_arith straight into `out` (a view of a larger buffer)."""
    B, T, d3 = qkv.shape
    ffi.check(ffi.load().afm_mha_fwd_arith(qkv.data_ptr(), ffi.ptr(km), out.data_ptr(), B, T, H, d3 // 3 // H, int(q_first), int(group_waves), int(arith),
                                           ffi.stream_of(qkv)), "afm_mha_fwd_arith")


def u8(mask):
    return mask.to(torch.uint8).to(dev())


# ------------------------------------------------------------------------------------------------ 2. masks and shapes, inference kernel
@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("T", TS)
def test_mask_patterns_parity_and_bit_identity_across_forms(T, H):
    """Per mask batch and arithmetic: the library's choice against float64 at 2e-5; every group_waves form, every q_first (rows in front
    untouched) and - at the default arithmetic - ops.mha_cross on the same data repacked as q and k|v bit-identical to it."""
    B, d = 3, 64 * H
    q, k, v = gaussian_qkv(B, H, T, T, 1000 + T)
    qd = pack(q, k, v).to(dev())
    q_only, kv_only = qd[..., :d].contiguous(), qd[..., d:].contiguous()
    for names, mask in batches(T):
        want = AR.merge_heads(AR.attention64(q, k, v, mask)[0])
        km = u8(mask)
        for tag, products in ARITHS:
            with arithmetic(products) as arith:
                what = f"T={T} H={H} {'/'.join(names)} {tag}"
                base = ops.mha(qd, mask.to(dev()), H)
                report(f"attention {what}", base, want, TOL)
                for gw in FORMS:
                    assert torch.equal(ops.mha(qd, km, H, group_waves=gw), base), f"{what}: group_waves={gw} differs from the library's choice"
                for qf in sorted({x for x in (1, 31, 32, T - 1) if 0 < x < T}):
                    for gw in (0, 1, 104):
                        out = torch.full((B, T, d), SENTINEL, device=dev())
                        mha_into(out, qd, km, H, qf, gw, arith)
                        assert torch.equal(out[:, qf:], base[:, qf:]), f"{what}: q_first={qf} group_waves={gw} differs on the rows it computes"
                        assert bool((out[:, :qf] == SENTINEL).all()), f"{what}: q_first={qf} group_waves={gw} wrote in front of its first row"
                if products == ops.DEFAULT_PRODUCTS:
                    assert torch.equal(ops.mha_cross(q_only, kv_only, km, H), base), f"{what}: the cross form differs"
    with arithmetic(ops.DEFAULT_PRODUCTS):                        # no mask pointer at all == a mask of zeros
        none = ops.mha(qd, None, H)
        report(f"attention T={T} H={H} key_mask=None", none, AR.merge_heads(AR.attention64(q, k, v, None)[0]), TOL)
        assert torch.equal(none, ops.mha(qd, torch.zeros(B, T, dtype=torch.bool, device=dev()), H))


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("T", TS)
def test_one_valid_key_returns_its_value_row_bit_for_bit(T, H):
    """P is exactly 1 (its lower split terms are zero: no kept or dropped product rounds) and every other probability exactly 0: every query
    row is that key's V row, in all three arithmetics and every form; the three samples keep different keys."""
    B, d = 3, 64 * H
    q, k, v = gaussian_qkv(B, H, T, T, 2000 + T)
    qkv = pack(q, k, v)
    qd = qkv.to(dev())
    keys = single_keys(T)
    for j in range(len(keys)):
        mine = [keys[(j + b) % len(keys)] for b in range(B)]
        mask = torch.stack([single_key_mask(T, key) for key in mine])
        want = torch.stack([qkv[b, mine[b], 2 * d:].expand(T, d) for b in range(B)]).to(dev())
        km = u8(mask)
        for tag, products in ARITHS:
            with arithmetic(products):
                for gw in (0,) + FORMS:
                    assert torch.equal(ops.mha(qd, km, H, group_waves=gw), want), f"T={T} H={H} valid keys {mine} {tag} group_waves={gw}"
        assert torch.equal(ops.mha_cross(qd[..., :d].contiguous(), qd[..., d:].contiguous(), km, H), want), f"T={T} H={H} valid keys {mine} cross form"


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("T", TS)
def test_fully_masked_sample_is_nan_and_leaves_its_neighbours_alone(T, H):
    """One sample with no valid key between two ordinary ones: its rows are NaN in every element (0 / 0, as torch.softmax gives), the other
    two samples are bit-identical to a launch of those two alone."""
    B, d = 3, 64 * H
    q, k, v = gaussian_qkv(B, H, T, T, 3000 + T)
    qd = pack(q, k, v).to(dev())
    pats = list(patterns(T).values())
    mask = torch.stack([pats[-1], torch.ones(T, dtype=torch.bool), pats[len(pats) // 2]])
    km, keep = u8(mask), [0, 2]
    want = AR.merge_heads(AR.attention64(q, k, v, mask)[0])
    assert torch.isnan(want[1]).all()
    for tag, products in ARITHS:
        with arithmetic(products):
            alone = ops.mha(qd[keep].contiguous(), km[keep].contiguous(), H)
            report(f"attention next to a fully masked sample T={T} H={H} {tag}", alone, want[keep], TOL)
            for gw in (0,) + FORMS:
                out = ops.mha(qd, km, H, group_waves=gw)
                assert bool(torch.isnan(out[1]).all()), f"T={T} H={H} {tag} group_waves={gw}: the fully masked sample is not NaN everywhere"
                assert torch.equal(out[keep], alone), f"T={T} H={H} {tag} group_waves={gw}: a neighbour of the fully masked sample changed"
    out = ops.mha_cross(qd[..., :d].contiguous(), qd[..., d:].contiguous(), km, H)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[keep]).all())


def test_large_batch_takes_the_librarys_own_twelve_wave_choice():
    """B H = 128 at T = 289: the library picks one 12-wave workgroup per (sample, head) by itself; masks cycle through every pattern and the
    one-valid-key masks.  float64 parity and bit identity with the small forms."""
    B, H, T = 16, 8, 289
    q, k, v = gaussian_qkv(B, H, T, T, 4000)
    rows = list(patterns(T).values()) + [single_key_mask(T, key) for key in single_keys(T)]
    mask = torch.stack([rows[b % len(rows)] for b in range(B)])
    want = AR.merge_heads(AR.attention64(q, k, v, mask)[0])
    qd, km = pack(q, k, v).to(dev()), u8(mask)
    for tag, products in ARITHS:
        with arithmetic(products):
            base = ops.mha(qd, km, H)
            report(f"attention B={B} H={H} T={T} {tag}", base, want, TOL)
            for gw in (1, 4, 12, 104):
                assert torch.equal(ops.mha(qd, km, H, group_waves=gw), base), f"{tag}: group_waves={gw}"


@pytest.mark.parametrize("products", [6, 9])
def test_guard_rows_around_the_output_survive(products):
    """afm_mha_fwd_arith and afm_mha_cross_fwd write straight into a buffer with 64 sentinel rows in front of and behind the output; T, Tq and
    Tk are no multiples of 32 (the last query block is ragged, the loads behind the last key are clamped)."""
    B, H, T, Tq, Tk, G = 3, 3, 97, 70, 130, 64
    d = 64 * H
    lib = ffi.load()
    q, k, v = gaussian_qkv(B, H, T, T, 5000)
    mask = batches(T)[-1][1]
    qd, km = pack(q, k, v).to(dev()), u8(mask)
    with arithmetic(products) as arith:
        for gw in (0, 1, 4, 104):
            for qf in (0, 33):
                buf = torch.full((G + B * T + G, d), SENTINEL, device=dev())
                out = buf[G:G + B * T].view(B, T, d)
                mha_into(out, qd, km, H, qf, gw, arith)
                torch.cuda.synchronize()
                assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + B * T:] == SENTINEL).all()), f"group_waves={gw} q_first={qf}: guard rows overwritten"
                assert torch.equal(out[:, qf:], ops.mha(qd, km, H)[:, qf:])
    qx, kx, vx = gaussian_qkv(B, H, Tq, Tk, 5001)
    maskx = batches(Tk)[-1][1]
    qxd, kvd, kmx = AR.merge_heads(qx).contiguous().to(dev()), pack_kv(kx, vx).to(dev()), u8(maskx)
    buf = torch.full((G + B * Tq + G, d), SENTINEL, device=dev())
    out = buf[G:G + B * Tq].view(B, Tq, d)
    ffi.check(lib.afm_mha_cross_fwd(qxd.data_ptr(), kvd.data_ptr(), kmx.data_ptr(), out.data_ptr(), B, Tq, Tk, H, 64, ffi.stream_of(qxd)), "afm_mha_cross_fwd")
    torch.cuda.synchronize()
    assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + B * Tq:] == SENTINEL).all()), "cross form: guard rows overwritten"
    report("cross-attention into a guarded buffer (Tq=70, Tk=130)", out, AR.merge_heads(AR.attention64(qx, kx, vx, maskx)[0]), TOL)


# ------------------------------------------------------------------------------------------------ 3. value families
FAMILIES = ["logit_25", "logit_55", "logit_140", "near_tied_keys", "spike_late_in_segment1", "spike_late_in_segment0", "v_range_2pm60", "v_1e20",
            "worst_mantissa_qk_one_sign", "worst_mantissa_qk_signed", "worst_mantissa_v_one_sign", "worst_mantissa_v_signed"]


def _scale_logits(q, k, target):
    """q scaled so that max |q k^T / 8| = target (natural units)."""
    s = (q.double() @ k.double().transpose(-1, -2)).abs().max().item() / 8.0
    return q * (target / s)


def family(name, B, H, T):
    """-> q, k, v [B, H, T, 64] float32."""
    rng = _rng(f"attention {name} {T}")
    g = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    wm = lambda: torch.from_numpy(_worst_mantissa(rng, (B, H, T, 64)))
    sign = lambda: torch.from_numpy(np.where(rng.random((B, H, T, 64)) < 0.5, np.float32(-1), np.float32(1)))
    q, k, v = g(B, H, T, 64), g(B, H, T, 64), g(B, H, T, 64)
    n0, _ = AR.segments(T)
    if name.startswith("logit_"):
        q = _scale_logits(q, k, float(name.split("_")[1]))
    elif name == "near_tied_keys":
        k = g(B, H, 1, 64) + 1e-3 * g(B, H, T, 64)
        q = _scale_logits(q, k, 55.0)
    elif name == "spike_late_in_segment1":
        k[:, :, T - 2] *= 20.0                                      # logits of +-20 on one key: half of the queries are taken over by it late in the walk
    elif name == "spike_late_in_segment0":
        k[:, :, 32 * n0 - 2] *= 20.0
    elif name == "v_range_2pm60":
        v = v * torch.from_numpy(np.exp2(rng.integers(-60, 61, size=(B, H, T, 1))).astype(np.float32))
    elif name == "v_1e20":
        v = v * 1e20
    elif name.startswith("worst_mantissa_qk"):
        q, k = wm(), wm()
        if name.endswith("signed"):
            q, k = q * sign(), k * sign()
        # a power of two keeps every mantissa (the split terms the pool was searched for): the largest |logit| lands in (8, 16]
        s = (q.double() @ k.double().transpose(-1, -2)).abs().max().item() / 8.0
        q = q * 2.0 ** -math.ceil(math.log2(s / 16.0))
    elif name.startswith("worst_mantissa_v"):
        v = wm()
        if name.endswith("signed"):
            v = v * sign()
    else:
        raise KeyError(name)
    return q.contiguous(), k.contiguous(), v.contiguous()


def _family_mask(T, B):
    p = patterns(T)
    rows = [p["lead_inside_block"], p["bernoulli"]] if T == 97 else [p["unconditional_branch"], p["every_other"]]
    return torch.stack(rows[:B])


def _references(q, k, v, mask):
    """(want64, want32, both lse) - want32 = whichever of torch's float32 and the blocked float32 restatement has the LARGER max error."""
    o64, l64 = AR.attention64(q, k, v, mask)
    ot, lt = AR.attention32_torch(q, k, v, mask)
    ob, lb = AR.attention32_blocked(q, k, v, mask)
    pick = lambda a, b, w: a if (a.double() - w).abs().max() >= (b.double() - w).abs().max() else b
    return o64, pick(ot, ob, o64), l64, pick(lt, lb, l64)


def _all_arithmetics(name, run):
    """run(tag) -> (ratio_max, ratio_rms) for every arithmetic, all measured before any failure is raised; records x6 / x9."""
    ratios, failures = {}, []
    for tag, products in ARITHS:
        with arithmetic(products):
            try:
                ratios[tag] = run(tag)
            except AssertionError as e:
                failures.append(str(e))
                ratios[tag] = (PARITY_ROWS[-1]["ratio_max"], PARITY_ROWS[-1]["ratio_rms"]) if PARITY_ROWS and PARITY_ROWS[-1]["name"].endswith(tag) else None
    if ratios.get("x6") and ratios.get("x9"):
        row = dict(name=f"{name} x6/x9", x6_over_x9_max=ratios["x6"][0] / max(ratios["x9"][0], 1e-30), x6_over_x9_rms=ratios["x6"][1] / max(ratios["x9"][1], 1e-30))
        print(f"[parity-f32] {row['name']}: max {row['x6_over_x9_max']:.3f} rms {row['x6_over_x9_rms']:.3f}")
        PARITY_ROWS.append(row)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name,T", [(n, 97) for n in FAMILIES] + [("logit_55", 289)])
def test_value_families_stay_in_the_float32_class(name, T):
    """max and rms error against float64 within margin 4 of the float32 reference's own (the worse of torch's float32 softmax-attention and
    attention32_blocked), in all three arithmetics.  old_tol is no invented figure: the first-order worst case of a float32 evaluation of
    these inputs (test_attention_ref_host.f32_bound), which the class bound must stay below."""
    B, H = 2, 3
    q, k, v = family(name, B, H, T)
    mask = _family_mask(T, B)
    o64, o32, _, _ = _references(q, k, v, mask)
    assert torch.isfinite(o32).all()
    qd, km = pack(q, k, v).to(dev()), u8(mask)
    tol = f32_bound(q, k, v)
    _all_arithmetics(f"attention {name} T={T}",
                     lambda tag: report_f32_class(f"attention {name} T={T} {tag}", AR.split_heads(ops.mha(qd, km, H).cpu(), H), o32, o64, tol))


# ------------------------------------------------------------------------------------------------ 4. training forward and backward
def _xattn_train(q, kv, km, H):
    B, Tq, d = q.shape
    out, lse = torch.empty(B, Tq, d, device=q.device), torch.empty(B, H, Tq, device=q.device)
    ffi.check(ffi.load().afm_mha_cross_fwd_train(q.data_ptr(), kv.data_ptr(), ffi.ptr(km), out.data_ptr(), lse.data_ptr(), B, Tq, kv.shape[1], H, d // H,
                                                 0.0, 0, 0, ffi.stream_of(q)), "afm_mha_cross_fwd_train")
    return out, lse


def _xattn_bwd(q, kv, km, out, dout, lse, H):
    B, Tq, d = q.shape
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    ws = torch.empty(B * H * Tq, device=q.device)
    ffi.check(ffi.load().afm_mha_cross_bwd(q.data_ptr(), kv.data_ptr(), ffi.ptr(km), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                           dkv.data_ptr(), B, Tq, kv.shape[1], H, d // H, 0.0, 0, 0, ws.data_ptr(), ws.numel() * 4, ffi.stream_of(q)),
              "afm_mha_cross_bwd")
    return dq, dkv


def _train_batches(T):
    keys = single_keys(T)
    # (one ordinary sample in the middle: a batch of one-valid-key samples alone has dQ = dK = 0, which a scaled comparison cannot take)
    return batches(T) + [((f"only_key_{keys[1]}", "none", f"only_key_{keys[-1]}"),
                          torch.stack([single_key_mask(T, keys[1]), torch.zeros(T, dtype=torch.bool), single_key_mask(T, keys[-1])]))]


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("T", [33, 97, 130, 289])
def test_training_forward_backward_over_the_mask_patterns(T, H):
    """afm_mha_fwd_train + afm_mha_bwd: out and lse at 2e-5, dQ / dK / dV against float64 autograd at the existing scaled 5e-5, dK and dV of every
    masked key exactly zero (as autograd gives), a second call the same bits."""
    B, d = 3, 64 * H
    q, k, v = gaussian_qkv(B, H, T, T, 6000 + T)
    qkv = pack(q, k, v)
    dout = AR.merge_heads(gaussian_qkv(B, H, T, T, 6500 + T)[0]).contiguous()
    qd, dd = qkv.to(dev()), dout.to(dev())
    for names, mask in _train_batches(T):
        what = f"T={T} H={H} {'/'.join(names)}"
        qr = qkv.double().requires_grad_(True)
        o_ref, lse_ref = _attn_ref(qr, mask, H)
        o_ref.backward(dout.double())
        km = u8(mask)
        out, lse = _mha_train(qd, km, H)
        report(f"train attention out {what}", out, o_ref, TOL)
        report(f"train attention lse {what}", lse, lse_ref, TOL)
        dqkv = _mha_bwd(qd, km, out, dd, lse, H)
        for i, n in enumerate("QKV"):
            rel(f"train attention d{n} {what}", dqkv[..., i * d:(i + 1) * d], qr.grad[..., i * d:(i + 1) * d], 5e-5)
        assert bool((qr.grad[..., d:][mask] == 0).all())
        assert bool((dqkv[..., d:][mask.to(dev())] == 0).all()), f"{what}: dK / dV of a masked key is not exactly zero"
        out2, lse2 = _mha_train(qd, km, H)
        assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, _mha_bwd(qd, km, out, dd, lse, H)), f"{what}: not deterministic"


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("Tk", [33, 130])
def test_cross_training_forward_backward_over_the_mask_patterns(Tk, H):
    """afm_mha_cross_fwd_train + afm_mha_cross_bwd, Tq = 70 queries over Tk keys: the same checks."""
    B, Tq, d = 3, 70, 64 * H
    q, k, v = gaussian_qkv(B, H, Tq, Tk, 7000 + Tk)
    q2, kv = AR.merge_heads(q).contiguous(), pack_kv(k, v)
    dout = AR.merge_heads(gaussian_qkv(B, H, Tq, Tk, 7500 + Tk)[0]).contiguous()
    qd, kvd, dd = q2.to(dev()), kv.to(dev()), dout.to(dev())
    for names, mask in _train_batches(Tk):
        what = f"Tq={Tq} Tk={Tk} H={H} {'/'.join(names)}"
        qr, kvr = q2.double().requires_grad_(True), kv.double().requires_grad_(True)
        o_ref, lse_ref = AR.attention64(AR.split_heads(qr, H), AR.split_heads(kvr[..., :d], H), AR.split_heads(kvr[..., d:], H), mask)
        o_ref = AR.merge_heads(o_ref)
        o_ref.backward(dout.double())
        km = u8(mask)
        out, lse = _xattn_train(qd, kvd, km, H)
        report(f"train cross-attention out {what}", out, o_ref, TOL)
        report(f"train cross-attention lse {what}", lse, lse_ref, TOL)
        dq, dkv = _xattn_bwd(qd, kvd, km, out, dd, lse, H)
        rel(f"train cross-attention dQ {what}", dq, qr.grad, 5e-5)
        rel(f"train cross-attention dK {what}", dkv[..., :d], kvr.grad[..., :d], 5e-5)
        rel(f"train cross-attention dV {what}", dkv[..., d:], kvr.grad[..., d:], 5e-5)
        assert bool((kvr.grad[mask] == 0).all())
        assert bool((dkv[mask.to(dev())] == 0).all()), f"{what}: dK / dV of a masked key is not exactly zero"
        dq2, dkv2 = _xattn_bwd(qd, kvd, km, out, dd, lse, H)
        out2, lse2 = _xattn_train(qd, kvd, km, H)
        assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dq, dq2) and torch.equal(dkv, dkv2), f"{what}: not deterministic"


def test_training_forward_pair_with_large_logits_stays_in_the_float32_class():
    """logit_55 through afm_mha_fwd_train and afm_mha_cross_fwd_train (f32 MFMA, natural-unit exp): out AND lse within margin 4 of the float32
    reference's own error.  old_tol of the lse: test_attention_ref_host.lse_bound (the logit error itself plus the roundings of the sum)."""
    B, H, T, Tq = 2, 3, 97, 70
    q, k, v = family("logit_55", B, H, T)
    mask = _family_mask(T, B)
    o64, o32, l64, l32 = _references(q, k, v, mask)
    out, lse = _mha_train(pack(q, k, v).to(dev()), u8(mask), H)
    r = [report_f32_class("train attention logit_55 out", AR.split_heads(out.cpu(), H), o32, o64, f32_bound(q, k, v)),
         report_f32_class("train attention logit_55 lse", lse.cpu(), l32, l64, lse_bound(q, k, l64))]
    qx = q[:, :, :Tq].contiguous()
    o64, o32, l64, l32 = _references(qx, k, v, mask)
    out, lse = _xattn_train(AR.merge_heads(qx).contiguous().to(dev()), pack_kv(k, v).to(dev()), u8(mask), H)
    r += [report_f32_class("train cross-attention logit_55 out", AR.split_heads(out.cpu(), H), o32, o64, f32_bound(qx, k, v)),
          report_f32_class("train cross-attention logit_55 lse", lse.cpu(), l32, l64, lse_bound(qx, k, l64))]
    assert len(r) == 4


# ------------------------------------------------------------------------------------------------ 5. the cross form's LDS ladder
@pytest.mark.parametrize("Tq,Tk,nw", LADDER)
def test_cross_form_down_its_lds_ladder(Tq, Tk, nw):
    """ops.mha_cross against float64 at the last key counts that fit 4, 2 and 1 waves and the first ones on the next rung (sizes derived in
    test_attention_ref_host.test_ladder_sizes_are_the_edges_of_split_mha_lds), with masked keys in the last block."""
    B, H = 1, 2
    q, k, v = gaussian_qkv(B, H, Tq, Tk, 8000 + Tk)
    mask = torch.zeros(B, Tk, dtype=torch.bool)
    mask[:, Tk - 20:Tk - 3] = True
    want = AR.merge_heads(AR.attention64(q, k, v, mask)[0])
    got = ops.mha_cross(AR.merge_heads(q).contiguous().to(dev()), pack_kv(k, v).to(dev()), mask.to(dev()), H)
    report(f"cross-attention Tq={Tq} Tk={Tk} ({nw} waves by split_mha_lds)", got, want, TOL)


def test_unsupported_key_counts_are_refused_and_write_nothing():
    """One key past the last rung (Tk = 23521) afm_mha_cross_fwd, and one block past its own LDS limit afm_mha_fwd_train, return
    AFM_E_UNSUPPORTED (AfmError) and leave a sentinel-filled output untouched."""
    B, H, Tq, Tk = 1, 2, 70, 23521
    d = 64 * H
    lib = ffi.load()
    qd, kvd = torch.randn(B, Tq, d, device=dev()), torch.randn(B, Tk, 2 * d, device=dev())
    out = torch.full((B, Tq, d), SENTINEL, device=dev())
    with pytest.raises(ffi.AfmError, match="unsupported shape"):
        ffi.check(lib.afm_mha_cross_fwd(qd.data_ptr(), kvd.data_ptr(), None, out.data_ptr(), B, Tq, Tk, H, 64, ffi.stream_of(qd)), "afm_mha_cross_fwd")
    with pytest.raises(ffi.AfmError, match="unsupported shape"):
        ops.mha_cross(qd, kvd, None, H)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    T = TRAIN_LAST_T + 1
    qkv = torch.randn(1, T, 3 * 64, device=dev())
    out, lse = torch.full((1, T, 64), SENTINEL, device=dev()), torch.full((1, 1, T), SENTINEL, device=dev())
    with pytest.raises(ffi.AfmError, match="unsupported shape"):
        ffi.check(lib.afm_mha_fwd_train(qkv.data_ptr(), None, out.data_ptr(), lse.data_ptr(), 1, T, 1, 64, 0.0, 0, 0, ffi.stream_of(qkv)), "afm_mha_fwd_train")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((lse == SENTINEL).all())


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table; committed as profiles/attention_edges_parity.json)."""
    write_parity_table()
