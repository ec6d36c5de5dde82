"""Host restatement of the attention kernels (csrc/attention.hip): softmax(Q K^T / sqrt(64) + key mask) V over [B, H, T, 64] operands.

    attention64           the function itself in float64 (differentiable: the training tests take its autograd gradients)
    attention32_torch     the same lines in float32 (torch's softmax): the "other float32 evaluation"
    attention32_blocked   float32 in the inference kernel's ASSOCIATION: logits in base-2 units (q * log2(e) / 8), 32-key blocks with the fully
                          masked ones skipped, an online softmax per key segment, two segments split at ceil(nkb / 2) and merged the way seg_merge
                          does.  It has no bf16 operand split - that is what the tests put under test.
    block_bits            the three flags the kernel keeps per 32-key block, computed from a mask row

A key mask is [B, Tk] bool, True = ignore the key.  A sample whose keys are all masked gives NaN rows in all three, as torch.softmax does."""
import math

import torch

DH, KB = 64, 32
LOG2E_F32 = 1.4426950408889634


def split_heads(x, H):
    """[B, T, H * 64] -> [B, H, T, 64]"""
    B, T, d = x.shape
    return x.view(B, T, H, d // H).transpose(1, 2)


def merge_heads(x):
    """[B, H, T, 64] -> [B, T, H * 64]"""
    B, H, T, dh = x.shape
    return x.transpose(1, 2).reshape(B, T, H * dh)


def _plain(q, k, v, mask):
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.softmax(s, -1) @ v, torch.logsumexp(s, -1)


def attention64(q, k, v, mask=None):
    """q [B, H, Tq, 64], k / v [B, H, Tk, 64] (any float type), mask [B, Tk] bool or None -> (out [B, H, Tq, 64], lse [B, H, Tq]) in float64;
    lse = log-sum-exp of the scaled, masked logits in natural units (what afm_mha_fwd_train saves)."""
    return _plain(q.double(), k.double(), v.double(), mask)


def attention32_torch(q, k, v, mask=None):
    return _plain(q.float(), k.float(), v.float(), mask)


def block_bits(mask_row, T=None):
    """The flags of mha_fwd_split_kernel per 32-key block of one sample: bit 0 = the block has a valid key, bit 1 = it has a masked key (the
    padding behind key T - 1 of the last block counts as masked), bit 2 = it has a valid key among its keys 16 .. 31.  -> list of ints."""
    T = int(mask_row.numel()) if T is None else T
    nkb = (T + KB - 1) // KB
    bits = [0] * nkb
    for i in range(nkb * KB):
        ok = i < T and not bool(mask_row[i])
        bits[i // KB] |= (1 | (4 if i & 16 else 0)) if ok else 2
    return bits


def segments(T):
    """(n0, n1): key blocks of segment 0 / 1 (n0 = ceil(nkb / 2); n1 == 0: one segment, no merge)."""
    nkb = (T + KB - 1) // KB
    n0 = (nkb + 1) // 2
    return n0, nkb - n0


def _fma(a, b, c):
    """fl32(a * b + c) with one rounding: the product of two float32 is exact in float64 (the sum then rounds to 53 bits before it rounds to
    24 - a double rounding that differs from a true fma only on exact ties of the 53-bit sum)."""
    return (a.double() * b.double() + c.double()).float()


def _exp2(x, key0, ulp):
    p = torch.exp2(x)
    if ulp:
        # the hardware's exp2 is documented to one ulp: move every (positive, finite) result one float32 ulp, up on odd keys, down on even
        odd = ((torch.arange(x.shape[-1]) + key0) & 1).bool().expand(x.shape)
        moved = torch.where(odd, torch.nextafter(p, torch.full_like(p, math.inf)), torch.nextafter(p, torch.zeros_like(p)))
        p = torch.where((p > 0) & torch.isfinite(moved), moved, p)
    return p


def attention32_blocked(q, k, v, mask=None, exp2_ulp=False):
    """float32 in the inference kernel's association (see the module docstring) -> (out, lse) float32.  exp2_ulp: every exp2 result of the
    probabilities is moved one ulp (up on odd keys, down on even): the reference widened by the hardware exp2's documented error."""
    q, k, v = q.float(), k.float(), v.float()
    B, H, Tq, dh = q.shape
    Tk = k.shape[2]
    assert dh == DH
    nkb = (Tk + KB - 1) // KB
    n0, n1 = segments(Tk)
    scale2 = torch.tensor(LOG2E_F32, dtype=torch.float32) * torch.tensor(1.0 / 8.0, dtype=torch.float32)
    neg_inf = float("-inf")
    out = torch.empty(B, H, Tq, dh, dtype=torch.float32)
    lse = torch.empty(B, H, Tq, dtype=torch.float32)
    for b in range(B):
        valid = torch.ones(Tk, dtype=torch.bool) if mask is None else ~mask[b]
        qs = q[b] * scale2                                                                   # [H, Tq, 64], pre-scaled as the kernel does

        def walk(kb0, kb1):
            m = torch.full((H, Tq), neg_inf, dtype=torch.float32)
            l = torch.zeros(H, Tq, dtype=torch.float32)
            o = torch.zeros(H, Tq, dh, dtype=torch.float32)
            for kb in range(kb0, kb1):
                lo, hi = kb * KB, min(kb * KB + KB, Tk)
                if not bool(valid[lo:hi].any()):
                    continue                                                                 # fully masked block: skipped
                s = qs @ k[b, :, lo:hi].transpose(-1, -2)                                    # [H, Tq, keys]
                s = s.masked_fill(~valid[lo:hi], neg_inf)
                m_new = torch.maximum(m, s.amax(-1))
                m_safe = torch.where(m_new == neg_inf, torch.zeros_like(m_new), m_new)
                alpha = torch.exp2(m - m_safe)
                p = _exp2(s - m_safe[..., None], lo, exp2_ulp)
                l = l * alpha + p.sum(-1)
                o = o * alpha[..., None] + p @ v[b, :, lo:hi]
                m = m_new
            return m, l, o

        m, l, o = walk(0, n0)
        if n1 > 0:
            m1, l1, o1 = walk(n0, nkb)
            mm = torch.maximum(m, m1)
            ms = torch.where(mm == neg_inf, torch.zeros_like(mm), mm)
            a0, a1 = torch.exp2(m - ms), torch.exp2(m1 - ms)
            l = _fma(l, a0, l1 * a1)                                                         # seg_merge: fma(x0, a0, x1 * a1)
            o = _fma(o, a0[..., None], o1 * a1[..., None])
            m = mm
        out[b] = o * (1.0 / l)[..., None]
        lse[b] = (m + torch.log2(l)) * math.log(2.0)
    return out, lse
