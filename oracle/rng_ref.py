"""TEST INFRASTRUCTURE ONLY - numpy restatements of the library's two counter-based generators, written from their definitions and
independent of the library (nothing here imports afm or torch):

  * the noise of afm_randn / the in-kernel draw of the sampling update: Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as
    easy as 1, 2, 3"; the Random123 known-answer vectors are pinned in tests/test_rng_host.py) keyed as csrc/common.h's philox_normal4
    keys it, then Box-Muller;
  * the dropout keep-mask of csrc/common.h (mix32, DropKey).

The integer stages are exact.  The float stage is bit-exact up to the transcendental calls: every float32 operation before them is a
single rounded operation (u32 -> f32 conversion to nearest even, + 0.5f, * 2^-32, fminf, 6.2831855f * u), reproduced with np.float32.  From
those exact float32 radius uniforms and angles `box_muller` returns the float64 value (the reference) and the same chain with every
operation in float32 (the float32 reference of tests/gpu_util.report_f32_class).
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
GOLDEN32 = 0x9E3779B1                     # the multiplier of the sample index (philox_normal4) and of the mask id / row (DropKey)
KEY1_XOR = 0x85EBCA6B
TWO_PI_F32 = np.float32(6.2831855)
U_MAX = np.float32(0.99999994)            # 1 - 2^-24, the clamp of the radius uniforms
S32 = np.float32(2.0 ** -32)


def _u64(x):
    """uint64 array holding the low 32 bits of x (Python ints of any sign, or integer arrays)."""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & 0xFFFFFFFF)
    return np.asarray(x).astype(np.uint64) & M32


# ------------------------------------------------------------------------------------------------ integer stage
def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: four uint64 arrays (or scalars) holding 32-bit words, broadcast against each other; key: two.
    Returns the four output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in counter])
    k0, k1 = _u64(key[0]), _u64(key[1])
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & M32, (k1 + np.uint64(PHILOX_W1)) & M32
    return c0, c1, c2, c3


def noise_key(seed, sample):
    """(k0, k1) of philox_normal4: k0 = seed_lo ^ (uint32(sample) * 0x9E3779B1), k1 = seed_hi ^ 0x85EBCA6B.  seed: uint64 values, sample:
    int64 values (Python ints or arrays)."""
    if isinstance(seed, (int, np.integer)):
        seed_lo, seed_hi = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    else:
        seed = np.asarray(seed).astype(np.uint64)
        seed_lo, seed_hi = seed & M32, seed >> np.uint64(32)
    k0 = seed_lo ^ ((_u64(sample) * np.uint64(GOLDEN32)) & M32)
    return k0, seed_hi ^ np.uint64(KEY1_XOR)


def noise_counters(seed, sample, step, q):
    """The four Philox output words of quad(s) q of (seed, sample, step): counter = (q low, q high, uint32(step), sample >> 32)."""
    q = np.asarray(q, dtype=np.uint64)
    sample_hi = np.uint64((int(sample) >> 32) & 0xFFFFFFFF)          # arithmetic shift of the int64, then its low word
    return philox4x32_10((q & M32, q >> np.uint64(32), _u64(int(step)), sample_hi), noise_key(int(seed), int(sample)))


# ------------------------------------------------------------------------------------------------ float stage
def uniforms(c):
    """The exact float32 (u0, angle0, u2, angle1) of philox_normal4 from its four counter words: radius uniforms from c[0] and c[2]
    ((float(c) + 0.5f) * 2^-32, clamped to 1 - 2^-24), angles 6.2831855f * (float(c) * 2^-32) from c[1] and c[3]."""
    f = [np.asarray(x).astype(np.int64).astype(np.float32) for x in c]          # exact int64, one rounding to nearest even
    half = np.float32(0.5)
    u0 = np.minimum((f[0] + half) * S32, U_MAX)
    u2 = np.minimum((f[2] + half) * S32, U_MAX)
    return u0, TWO_PI_F32 * (f[1] * S32), u2, TWO_PI_F32 * (f[3] * S32)


def box_muller(u0, a0, u2, a1):
    """(z32, z64), each [..., 4] = (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) with r = sqrt(-2 ln u): z64 in float64 from the float32
    inputs, z32 with every operation in float32."""
    for x in (u0, a0, u2, a1):
        assert x.dtype == np.float32
    out = []
    for dt in (np.float32, np.float64):
        u0d, a0d, u2d, a1d = (x.astype(dt) for x in (u0, a0, u2, a1))
        r0, r1 = np.sqrt(dt(-2.0) * np.log(u0d)), np.sqrt(dt(-2.0) * np.log(u2d))
        z = np.stack([r0 * np.cos(a0d), r0 * np.sin(a0d), r1 * np.cos(a1d), r1 * np.sin(a1d)], axis=-1)
        assert z.dtype == dt
        out.append(z)
    return out[0], out[1]


def normal_quads(seed, sample, step, q):
    """(z32, z64) [len(q), 4] of the quads q of one (seed, sample, step)."""
    return box_muller(*uniforms(noise_counters(seed, sample, step, q)))


def normals(seed, sample_index0, step, B, per_sample):
    """(z32, z64) in the layout of afm_randn: [B, per_sample], row b = sample sample_index0 + b, element e of it = value e % 4 of quad
    e // 4 (the last quad cut where per_sample is no multiple of 4)."""
    nq = (per_sample + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    z32, z64 = np.empty((B, per_sample), np.float32), np.empty((B, per_sample), np.float64)
    for b in range(B):
        a32, a64 = normal_quads(seed, sample_index0 + b, step, q)
        z32[b], z64[b] = a32.reshape(-1)[:per_sample], a64.reshape(-1)[:per_sample]
    return z32, z64


# ------------------------------------------------------------------------------------------------ dropout keep-mask
def mix32(x):
    """The murmur3 finaliser on uint64 arrays holding 32-bit words."""
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13)); x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def drop_threshold(p):
    """(thresh, inv_keep) of DropKey: thresh = uint32(float32(p) * 2^32), saturating at 2^32 - 1 from 4294967040 on (the largest float32
    below 2^32); inv_keep = 1 / (1 - p) in float32."""
    p = np.float32(p)
    t = p * np.float32(4294967296.0)
    thresh = 0xFFFFFFFF if t >= np.float32(4294967040.0) else int(t)
    return thresh, np.float32(1.0) / (np.float32(1.0) - p)


def drop_draws(seed, mask_id, rows, cols):
    """The 32-bit draw of every (row, col) of mask (seed, mask_id): [rows, cols] uint64 < 2^32."""
    seed, mask_id = int(seed) & (2 ** 64 - 1), int(mask_id) & 0xFFFFFFFF
    k0 = np.uint64((seed & 0xFFFFFFFF) ^ ((mask_id * GOLDEN32) & 0xFFFFFFFF))
    k1 = np.uint64(((seed >> 32) + mask_id * 0x7FEB352D + 0x632BE5AB) & 0xFFFFFFFF)
    row = np.arange(rows, dtype=np.uint64)[:, None] & M32
    col = np.arange(cols, dtype=np.uint64)[None, :] & M32
    return mix32((mix32(col ^ k0) + ((row * np.uint64(GOLDEN32)) & M32) + k1) & M32)


def keep_mask(p, seed, mask_id, rows, cols):
    """(keep, inv_keep): keep [rows, cols] bool, True where DropKey(p, seed, mask_id)(row, col) keeps the element (draw >= thresh);
    inv_keep the float32 factor a kept element is scaled by."""
    thresh, inv_keep = drop_threshold(p)
    return drop_draws(seed, mask_id, rows, cols) >= np.uint64(thresh), inv_keep
