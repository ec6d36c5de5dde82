"""Host tests of oracle/attention_ref.py and of the key-mask patterns tests/test_gpu_attention_edges.py puts through the attention kernels.

The patterns are built here (and imported by the GPU tests) so that what they claim to hit is checked where it costs nothing: the three
flags mha_fwd_split_kernel keeps per 32-key block (has a valid key / has a masked key / has a valid key in its upper 16) are recomputed from
every mask on the host, and every combination the kernel distinguishes, an empty first segment and an empty second segment must occur at
every tested T with two or more key blocks."""
import pytest
import torch

from oracle import attention_ref as AR

TS = [1, 31, 32, 33, 65, 97, 130, 161, 225, 289]           # 1 .. 10 key blocks; T = 289: one key in the tail block
GAMMA = 66 * 2.0 ** -24                                      # 64 products, the scale, the subtraction of the maximum


def patterns(T):
    """name -> [T] bool key mask (True = ignore), every pattern with at least one valid key; patterns that do not exist at this T (a segment
    to mask when there is one key block, ...) or that coincide with `none` are left out."""
    nkb = (T + 31) // 32
    n0, n1 = AR.segments(T)
    i = torch.arange(T)
    p = {"none": torch.zeros(T, dtype=torch.bool)}
    c = min(T - 1, 32 * ((nkb - 1) // 2) + 11)
    p["lead_inside_block"] = i < c                            # a leading run that ends inside a block (whole leading blocks first when nkb >= 3)
    if 32 * max(1, nkb // 3) < T:
        p["lead_to_block_edge"] = i < 32 * max(1, nkb // 3)   # a leading run that ends on a block edge
    if n1 > 0:
        p["segment0_masked"] = i < 32 * n0
        p["segment1_masked"] = i >= 32 * n0
    if T > 16:
        p["upper16_valid"] = (i & 16) == 0                    # only keys with (i & 16) != 0 valid
    p["lower16_valid"] = (i & 16) != 0                        # only keys with (i & 16) == 0 valid: no block has a valid key in its upper half
    p["every_other"] = (i & 1) == 1
    bern = torch.rand(T, generator=torch.Generator().manual_seed(1234 + T)) < 0.5
    if bool(bern.all()):
        bern[0] = False
    p["bernoulli"] = bern
    if T >= 3:
        p["unconditional_branch"] = (i >= 1) & (i <= min(129, T - 2))      # key 0 valid, keys 1 .. min(129, T - 2) masked (guided sampling: 326 -> 1..129)
    out = {}
    for name, m in p.items():
        assert not bool(m.all()), (name, T)
        if name != "none" and not bool(m.any()):
            continue
        out[name] = m
    return out


def single_keys(T):
    """Positions of the one-valid-key masks: 0, 15, 16, 31, 32 and T - 1 where they exist."""
    return sorted({k for k in (0, 15, 16, 31, 32, T - 1) if 0 <= k < T})


def single_key_mask(T, key):
    m = torch.ones(T, dtype=torch.bool)
    m[key] = False
    return m


def batches(T, B=3):
    """The patterns of T in groups of B rows -> [(names, mask [B, T])]: the samples of a launch carry DIFFERENT masks (the batch indexing of
    key_mask is under test too); the last group is filled up from the front."""
    items = list(patterns(T).items())
    out = []
    for s in range(0, len(items), B):
        grp = [items[(s + j) % len(items)] for j in range(B)]
        out.append((tuple(n for n, _ in grp), torch.stack([m for _, m in grp])))
    return out


def gaussian_qkv(B, H, Tq, Tk, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, Tq, 64, generator=g), torch.randn(B, H, Tk, 64, generator=g), torch.randn(B, H, Tk, 64, generator=g))


def f32_bound(q, k, v):
    """First-order worst case of a float32 evaluation of softmax(q k^T / 8) v, from the inputs in float64:
    2 gamma max_{q,k} sum_i |q_i k_i| / 8 * max|v| + 2^-22 max|v| (a logit is wrong by at most gamma sum|q_i k_i| / 8, a probability by that
    relative amount, numerator and denominator both carry it; the normalisation and the output rounding add 2^-22 max|v|)."""
    s = (q.double().abs() @ k.double().abs().transpose(-1, -2)).max().item() / 8.0
    vmax = v.double().abs().max().item()
    return 2 * GAMMA * s * vmax + 2.0 ** -22 * vmax


def lse_bound(q, k, lse64):
    """The same for the log-sum-exp: the logit error itself plus the rounding of the sum, its logarithm and the result."""
    s = (q.double().abs() @ k.double().abs().transpose(-1, -2)).max().item() / 8.0
    return 2 * GAMMA * s + 2.0 ** -22 * max(lse64.abs().max().item(), 1.0)


@pytest.mark.parametrize("T", TS)
def test_float32_restatements_sit_in_the_float32_class_of_float64(T):
    """attention32_blocked (the kernel's association) and torch's float32 softmax-attention against attention64 over every mask pattern: both
    below the first-order float32 bound of the inputs, and neither more than the project's margin 4 (the same f32 arithmetic in another
    association, gpu_util.report_f32_class) above the other, with its floor of one ulp of the largest output."""
    B, H, Tq = 3, 2, min(T, 70)
    for names, mask in batches(T):
        q, k, v = gaussian_qkv(B, H, Tq, T, 7 * T)
        o64, l64 = AR.attention64(q, k, v, mask)
        ot, lt = AR.attention32_torch(q, k, v, mask)
        ob, lb = AR.attention32_blocked(q, k, v, mask)
        assert torch.isfinite(ob).all() and torch.isfinite(lb).all(), names
        et, eb = (ot.double() - o64).abs().max().item(), (ob.double() - o64).abs().max().item()
        floor = 2.0 ** -23 * o64.abs().max().item()
        bound = f32_bound(q, k, v)
        print(f"[attention-ref] T={T} {names}: torch f32 {et:.2e}, blocked f32 {eb:.2e}, bound {bound:.2e}")
        assert et <= bound and eb <= bound, (names, et, eb, bound)
        assert eb <= 4 * et + floor and et <= 4 * eb + floor, (names, et, eb)
        elt, elb = (lt.double() - l64).abs().max().item(), (lb.double() - l64).abs().max().item()
        assert max(elt, elb) <= lse_bound(q, k, l64), (names, elt, elb)
        ou, _ = AR.attention32_blocked(q, k, v, mask, exp2_ulp=True)          # the widened reference stays a float32-class evaluation
        assert (ou.double() - o64).abs().max().item() <= bound


@pytest.mark.parametrize("T", TS)
def test_one_valid_key_gives_its_value_row_exactly(T):
    """P is exactly 1 for the one valid key and exactly 0 for every other: both float32 evaluations return that key's V row bit for bit."""
    B, H, Tq = 1, 2, min(T, 40)
    q, k, v = gaussian_qkv(B, H, Tq, T, 11 * T)
    for key in single_keys(T):
        mask = single_key_mask(T, key)[None]
        want = v[:, :, key:key + 1, :].expand(B, H, Tq, 64)
        for fn in (AR.attention32_torch, AR.attention32_blocked):
            out, lse = fn(q, k, v, mask)
            assert torch.equal(out, want), (fn.__name__, T, key)
        o64, _ = AR.attention64(q, k, v, mask)
        assert torch.equal(o64, want.double())


@pytest.mark.parametrize("T", [1, 33, 97])
def test_fully_masked_sample_is_nan_like_torch_softmax(T):
    B, H = 3, 2
    q, k, v = gaussian_qkv(B, H, T, T, 13 * T)
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[1] = True
    assert torch.isnan(torch.softmax(torch.full((T,), float("-inf")), -1)).all()
    for fn in (AR.attention64, AR.attention32_torch, AR.attention32_blocked):
        out, _ = fn(q, k, v, mask)
        assert torch.isnan(out[1]).all(), fn.__name__
        assert torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all(), fn.__name__


@pytest.mark.parametrize("T", TS)
def test_patterns_hit_the_block_flags_they_claim(T):
    """The flags per block: 5 = all keys valid (no mask addition), 7 = valid and masked keys with a valid key in the upper 16, 3 = valid and
    masked keys, none valid in the upper 16 (the second K16 step of P V is skipped), 2 = no valid key (the block is skipped)."""
    nkb = (T + 31) // 32
    n0, n1 = AR.segments(T)
    pats = patterns(T)
    bits = {name: AR.block_bits(m, T) for name, m in pats.items()}
    assert all(len(b) == nkb and any(x & 1 for x in b) for b in bits.values())
    seen = {x for b in bits.values() for x in b}
    assert seen <= {2, 3, 5, 7}, seen                                        # nothing else can occur
    # single patterns do what their names say
    if T >= 32:
        assert bits["none"][0] == 5
    if T % 32:
        assert bits["none"][-1] & 2                                          # the padding of the tail block counts as masked
    if "lower16_valid" in pats:                                              # (T <= 16: the same mask as `none`)
        assert all(not (x & 4) for x in bits["lower16_valid"])
        assert any(x == 3 for x in bits["lower16_valid"])
    if T > 16:
        assert all(x in (2, 7) for x in bits["upper16_valid"]) and 7 in bits["upper16_valid"]
    if "unconditional_branch" in pats and T >= 130:
        assert bits["unconditional_branch"][:4] == [3, 2, 2, 2]              # one valid key in block 0, three empty blocks
    if "lead_inside_block" in pats:
        lead = bits["lead_inside_block"]
        first = next(j for j, x in enumerate(lead) if x & 1)
        assert all(x == 2 for x in lead[:first]) and (lead[first] & 2) and first == (nkb - 1) // 2
    if nkb >= 2:
        assert seen == {2, 3, 5, 7}, (T, seen)                               # every combination the kernel distinguishes
        assert n1 > 0
        assert all(x == 2 for x in bits["segment0_masked"][:n0]) and any(x & 1 for x in bits["segment0_masked"][n0:])
        assert all(x == 2 for x in bits["segment1_masked"][n0:]) and any(x & 1 for x in bits["segment1_masked"][:n0])
        assert bits["lead_to_block_edge"][0] == 2
    if nkb >= 3:
        assert lead[0] == 2                                                  # a masked LEADING block in front of a partly masked one
    # the one-valid-key masks: exactly one block with bit 0, upper-half flag only for keys 16 .. 31 of their block
    for key in single_keys(T):
        b = AR.block_bits(single_key_mask(T, key), T)
        assert [j for j, x in enumerate(b) if x & 1] == [key // 32]
        assert bool(b[key // 32] & 4) == bool(key & 16)
    # every pattern sits in exactly one batch slot, every batch has three different rows when there are three patterns
    names = [n for grp, _ in batches(T) for n in grp]
    assert set(names) == set(pats)


# ---- the LDS ladder of the cross form (csrc/attention.hip: split_mha_lds, mha_fwd_launch), restated to derive the key counts the GPU tests use
KVSTAGE, PARK_BYTES, LDS_CAP = 3 * 32 * 144 + 3 * 64 * 80, (32 * 64 + 64) * 4, 160 * 1024


def split_mha_lds(nkb, nw):
    """csrc/attention.hip split_mha_lds, sequential form: two K / V stages + additive mask + block flags (+ 8448 B of parked state per wave)."""
    return 2 * KVSTAGE + nkb * 32 * 4 + (nkb + 3) // 4 * 4 * 4 + (nw * PARK_BYTES if nkb > 1 else 0)


def last_fit(nw):
    nkb = 1
    while split_mha_lds(nkb + 1, nw) <= LDS_CAP:
        nkb += 1
    return nkb


def waves_after_ladder(Tq, Tk):
    """The cross form's wave count: the smallest group covering the query blocks, stepped down 12 -> 8 -> 6 -> 4 -> 2 -> 1 while the LDS
    does not fit; None = refused."""
    nqb, nkb = (Tq + 31) // 32, (Tk + 31) // 32
    nw = 4 if nqb <= 4 else (6 if nqb <= 6 else (8 if nqb <= 8 else 12))
    while split_mha_lds(nkb, nw) > LDS_CAP and nw > 1:
        nw = 8 if nw > 8 else (6 if nw > 6 else (4 if nw > 4 else nw // 2))
    return nw if split_mha_lds(nkb, nw) <= LDS_CAP else None


LADDER = [(70, 17376, 4), (70, 17377, 2), (70, 21472, 2), (70, 21473, 1), (70, 23520, 1), (289, 9185, 6)]


def _train_lds(nkb):
    return (2 * 32 * 68 + 2 * 32 * 64 + nkb * 32) * 4 + nkb * 4


TRAIN_LAST_T = 32 * max(n for n in range(1, 2000) if _train_lds(n) <= LDS_CAP)


def test_ladder_sizes_are_the_edges_of_split_mha_lds():
    """Host arithmetic: split_mha_lds(nkb, nw) = 58368 + 132 nkb (nkb a multiple of 4) + 8448 nw <= 163840 gives nkb <= 543 / 671 / 735 for
    4 / 2 / 1 waves, i.e. Tk = 17376 / 21472 / 23520 are the last sizes that fit them and 23521 is the first that fits none; with 10 query
    blocks (Tq = 289) 12 waves fit nkb <= 31 and 8 waves nkb <= 287 = Tk 9184, so 9185 is the first size on 6 waves.  afm_mha_fwd_train:
    (2 * 32 * 68 + 2 * 32 * 64) * 4 + 132 nkb <= 163840 gives nkb <= 985 = T 31520."""
    assert [32 * last_fit(4), 32 * last_fit(2), 32 * last_fit(1), 32 * last_fit(8)] == [17376, 21472, 23520, 9184]
    for Tq, Tk, nw in LADDER:
        assert waves_after_ladder(Tq, Tk) == nw, (Tq, Tk)
    assert waves_after_ladder(289, 9184) == 8 and waves_after_ladder(70, 23521) is None
    assert TRAIN_LAST_T == 31520
