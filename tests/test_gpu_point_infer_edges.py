"""`-m gpu`: the inference half of the scene branch - afm_pt_attention and afm_transition_down (csrc/pointnet.hip), afm_knn, afm_knn_ws,
afm_fps, afm_segment_mean and afm_gather_rows (csrc/pointops.hip), afm_bn_fold (csrc/elementwise.hip) - against the float64 restatements of
tests/test_point_infer_edges_host.py, at the shapes, dispatch arms and values that module builds and proves on the host.

Every inexact quantity is bounded by the float32 restatement's OWN error against its float64 twin (gpu_util.report_f32_class, margin 4,
nothing excluded); what is an exact function of its inputs - an index list, a copy, a sum in a stated order, one correctly rounded float32
operation after another - is asserted bit for bit.  The figures go to profiles/point_infer_edges_parity.json.

Non-finite coordinates.  The clouds with NaN, +-inf and 3e19 entries go ONLY to afm_knn, afm_knn_ws and afm_fps; their output is compared
and never used as a gather address.  Why those three may be given any coordinate values (read in csrc/pointops.hip):
  * every global and LDS address and every trip count in knn_kernel, knn_sort_kernel, knn_pruned_kernel and the FPS kernels is a function of
    n, m, k, the block / thread numbers and of INDICES the kernels made themselves; a coordinate only ever enters comparisons and selects;
  * knn_kernel keeps a candidate on `d < kth` - false for a NaN and for +inf against the initial +inf - and its append buffer is
    addressed by a count that the drain bounds (at most 8 appends between drains); slots never filled keep index -1, which the epilogue
    now replaces (rules 3 and 4) before `b n + index` is formed;
  * knn_sort_kernel: the sample's box comes from fminf / fmaxf, which drop a NaN; the quantisation `(x - lo) scale` may be NaN or +-inf,
    and is now clamped to [0, 1023] AS A FLOAT (fmaxf(NaN, 0) = 0) before the conversion, so the Morton key is a 30-bit number whatever x
    is; the bitonic sort orders (key, index) pairs and its trip counts depend on n alone: the sorted list is a permutation of 0 .. n-1
    followed by the 0xFFFFFFFF padding (whose key lies above every 30-bit key), and only that permutation is used as an address;
  * tile and query boxes are fminf / fmaxf reductions: a NaN coordinate is left out of its box (its point is never a neighbour), an
    infinite one widens it (a smaller lower bound: more tiles scanned, never fewer).  The box distance is max(lo - q, q - hi, 0) per
    axis: fmaxf against 0 makes it a number in [0, +inf] even for a NaN query, so `lb <= kth` is a plain comparison; a query that still
    lacks k neighbours has kth = +inf and scans every tile.  The walk over tiles runs t = 0 .. nt-1 regardless;
  * knn_pruned_kernel orders 64-bit keys (distance bits << 32 | index).  Positive NaN bits compare above +inf's, NaN bits with the sign
    set above those: with the empty slot at (+inf, 0), `key < kth` takes no candidate whose distance is not finite, and no padding entry
    of a ragged tile.  The merged list of a query is written to its rank (< k), then EVERY output entry is written from it (rules 3, 4);
  * the FPS kernels keep running minima as unsigned bits under v_min_u32 against the initial 1e10: the bits of a NaN or of +inf are
    larger and never stored, so every key the arg-max sees is an ordinary number and its index one of the sample's points."""
import ctypes as C

import pytest
import torch

from afm import ffi, pointops
from gpu_util import dev, report_f32_class, write_parity_table
import test_point_infer_edges_host as H

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SENTINEL = -12345.0


def cls(name, got, want32, want64, tol):
    return report_f32_class("point-infer edges " + name, got.detach().cpu(), want32, want64, tol, margin=H.MARGIN, select=None)


def D(t):
    return None if t is None else t.to(dev())


# ================================================================================================ afm_pt_attention
def pt_call(p, qkv, knn_idx, out, channels, share, w, out_scale=None, out_shift=None, relu=False, nsample=None):
    """afm_pt_attention on device tensors as they are, `out` given by the caller -> the return code"""
    a = ffi.PtAttentionArgs()
    a.p, a.qkv, a.knn_idx, a.out = p.data_ptr(), qkv.data_ptr(), knn_idx.data_ptr(), out.data_ptr()
    a.n, a.channels, a.nsample, a.share_planes = p.shape[0], channels, knn_idx.shape[1] if nsample is None else nsample, share
    for name, key in (("lp0_w", "lp0_w"), ("lp0_b", "lp0_b"), ("lp_bn_scale", "lp_s"), ("lp_bn_shift", "lp_t"), ("lp3_w", "lp3_w"), ("lp3_b", "lp3_b"),
                      ("w0_bn_scale", "w0_s"), ("w0_bn_shift", "w0_t"), ("w2_w", "w2_w"), ("w2_b", "w2_b"), ("w3_bn_scale", "w3_s"),
                      ("w3_bn_shift", "w3_t"), ("w5_w", "w5_w"), ("w5_b", "w5_b")):
        setattr(a, name, w[key].data_ptr())
    a.out_scale = None if out_scale is None else out_scale.data_ptr()
    a.out_shift = None if out_shift is None else out_shift.data_ptr()
    a.relu = 1 if relu else 0
    return ffi.load().afm_pt_attention(C.byref(a), ffi.stream_of(p))


def run_pt(i, C_, **kw):
    w = {k: D(v) for k, v in i["w"].items()}
    return pointops.pt_attention(D(i["p"]), D(i["qkv"]), D(i["knn_idx"]), C_, i["share"], *(w[k] for k in H.PT_WEIGHTS), **kw)


def check_knn_is_the_oracles(i, KN, B, n):
    p = D(i["p"])
    got, _ = pointops.knn(KN, p, p, B, n, n)
    assert torch.equal(got.cpu(), i["knn_idx"]), "pointops.knn differs from the oracle's neighbours"


@pytest.mark.parametrize("tag,B,n", H.PT_POINTS)
@pytest.mark.parametrize("C_,share,KN", sorted(H.PT_ARMS))
def test_pt_attention_every_dispatch_arm(C_, share, KN, tag, B, n):
    if (C_, share, KN) in H.PT_SMALL_ONLY and tag != "1x37":
        return                                                          # (these two arms take n = 37 only)
    i = H.pt_inputs(C_, share, KN, B, n)
    check_knn_is_the_oracles(i, KN, B, n)
    got = run_pt(i, C_)
    r32, r64 = H.pt_reference(C_, share, KN, B, n, "softmax_1", F32), H.pt_reference(C_, share, KN, B, n, "softmax_1", F64)
    cls(f"pt_attention arm C={C_} share={share} k={KN} n={tag}", got, r32["out"], r64["out"], H.TOL)
    assert torch.equal(got, run_pt(i, C_)), "two runs differ"
    if B == 2:                                                          # the second sample launched alone, its neighbours re-based
        alone = dict(i, p=i["p"][n:], qkv=i["qkv"][n:], knn_idx=i["knn_idx"][n:] - n)
        assert torch.equal(run_pt(alone, C_), got[n:]), "a shard of the points differs from the whole launch"


@pytest.mark.parametrize("C_,share,KN", sorted(H.PT_REFUSALS))
def test_pt_attention_refusals_leave_the_output_untouched(C_, share, KN):
    n, width = 3, 3 * 520
    p, qkv = torch.zeros(n, 3, device=dev()), torch.zeros(n, width, device=dev())
    knn_idx = torch.zeros(n, 16, dtype=torch.int32, device=dev())
    big = torch.zeros(520 * 64, device=dev())
    out = torch.full((n, 520), SENTINEL, device=dev())
    rc = pt_call(p, qkv, knn_idx, out, C_, share, {k: big for k in H.PT_WEIGHTS}, nsample=KN)
    want = H.PT_REFUSALS[(C_, share, KN)]
    assert rc == {H.BADARG: -1, H.UNSUPPORTED: -3}[want], (rc, want)
    with pytest.raises(ffi.AfmError, match="bad argument" if want == H.BADARG else "unsupported shape"):
        ffi.check(rc, "afm_pt_attention")
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call wrote to its output"


@pytest.mark.parametrize("C_,share,KN,n", H.PT_COUNTS + H.PT_SECOND_TRIP)
def test_pt_attention_point_counts(C_, share, KN, n):
    """n = 1 .. 5: dead waves of the four-wave form, the one-wave form, and n < k neighbour lists (the last neighbour repeated);
    8197 points at four waves and 2051 at one are a second trip of the grid-stride loop"""
    i = H.pt_inputs(C_, share, KN, 1, n)
    check_knn_is_the_oracles(i, KN, 1, n)
    if n < KN:
        assert (i["knn_idx"][:, n:] == i["knn_idx"][:, n - 1: n]).all()
    got = run_pt(i, C_)
    r32, r64 = H.pt_reference(C_, share, KN, 1, n, "softmax_1", F32), H.pt_reference(C_, share, KN, 1, n, "softmax_1", F64)
    cls(f"pt_attention points C={C_} n={n}", got, r32["out"], r64["out"], H.TOL)
    if n > 2048:
        # the points of the second trip launched alone: they come first, the rows their neighbour lists name follow (a point's own row
        # must sit at its own position); those extra rows' own lists point at row 0 where they leave the subset, and their output is unused
        first = 2048 * (4 if C_ <= 256 else 1)
        tail = torch.arange(first, n)
        named = torch.unique(i["knn_idx"][tail].long())
        order = torch.cat([tail, named[named < first]])
        remap = torch.zeros(n, dtype=torch.long)
        remap[order] = torch.arange(order.numel())
        sub = dict(i, p=i["p"][order], qkv=i["qkv"][order], knn_idx=remap[i["knn_idx"][order].long()].to(torch.int32))
        assert torch.equal(run_pt(sub, C_)[: tail.numel()], got[first:]), "the second trip differs from the same points launched alone"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C_,share,KN", H.PT_FAMILY_SHAPES)
def test_pt_attention_fused_output_batchnorm(C_, share, KN, relu):
    B, n = 1, 37
    i = H.pt_inputs(C_, share, KN, B, n)
    s, t = H.pt_out_bn(C_)
    got = run_pt(i, C_, out_scale=D(s), out_shift=D(t), relu=relu)
    r32, r64 = H.pt_reference(C_, share, KN, B, n, "softmax_1", F32, relu), H.pt_reference(C_, share, KN, B, n, "softmax_1", F64, relu)
    cls(f"pt_attention C={C_} fused BN relu={relu}", got, r32["out"], r64["out"], H.TOL)
    # the unfused composition: the plain launch, then the BatchNorm (and ReLU) as separate float32 operations
    plain = run_pt(i, C_) * D(s) + D(t)
    plain = torch.relu(plain) if relu else plain
    cls(f"pt_attention C={C_} unfused BN relu={relu}", plain, r32["out"], r64["out"], H.TOL)
    if relu:
        assert (got >= 0).all() and (got == 0).any()


@pytest.mark.parametrize("family", H.PT_FAMILIES)
@pytest.mark.parametrize("C_,share,KN", H.PT_FAMILY_SHAPES)
def test_pt_attention_value_families(C_, share, KN, family):
    B, n = 1, 37
    i = H.pt_inputs(C_, share, KN, B, n, family)
    got = run_pt(i, C_)
    r32, r64 = H.pt_reference(C_, share, KN, B, n, family, F32), H.pt_reference(C_, share, KN, B, n, family, F64)
    tol = H.pt_tol(C_, share, KN, B, n, family)
    cls(f"pt_attention C={C_} {family}", got, r32["out"], r64["out"], tol)
    CS = C_ // share
    if family == "softmax_uniform":                                     # the plain neighbour mean
        mean = lambda r: r["vp"].view(n, KN, share, CS).mean(1).reshape(n, C_)
        cls(f"pt_attention C={C_} uniform softmax = neighbour mean", got, mean(r32), mean(r64), tol)
    if family == "one_row":                                             # v + p_r of the one row
        cls(f"pt_attention C={C_} one row = v + p_r", got, r32["vp"][:, 0], r64["vp"][:, 0], tol)
    if family == "far_cloud":                                           # bit-equal relative positions: bit-equal output
        near = dict(i, p=i["p"] - H.FAR)
        assert torch.equal(got, run_pt(near, C_)), "the translated cloud gives other bits than the untranslated one"


# ================================================================================================ afm_transition_down
def run_td(i, knn_idx=None, new_p=None):
    return pointops.transition_down(D(i["p"]), D(i["x"]), D(i["new_p"] if new_p is None else new_p), D(i["knn_idx"] if knn_idx is None else knn_idx),
                                    D(i["W"]), D(i["scale"]), D(i["shift"]))


@pytest.mark.parametrize("c", H.TD_C)
def test_transition_down_every_tile_tail(c):
    """the whole grid: every c against every cout and every M (K, column and row tails in every combination)"""
    worst = 0.0
    for cout in H.TD_COUT:
        for M in H.TD_M:
            i = H.td_inputs(c, cout, M)
            got = run_td(i)
            assert got.shape == (M, cout)
            r32, r64 = H.td_reference(c, cout, M, "gaussian", F32), H.td_reference(c, cout, M, "gaussian", F64)
            record = cout in (63, 128) and M in (9, 17)
            ratio = report_f32_class(f"point-infer edges transition_down c={c} cout={cout} M={M}", got.cpu(), r32["out"], r64["out"], H.TOL,
                                     margin=H.MARGIN, select=None, record=record)
            worst = max(worst, ratio[0])
            assert torch.equal(got, run_td(i)), "two runs differ"
            if M > 1:                                                   # the last points launched alone: other rows of other row blocks
                j = M // 2
                assert torch.equal(run_td(i, knn_idx=i["knn_idx"][j:].contiguous(), new_p=i["new_p"][j:].contiguous()), got[j:]), "a shard differs"
    print(f"[parity-f32] point-infer edges transition_down c={c}: worst ratio of the grid {worst:.2f}")


def test_transition_down_sample_shard_and_knn():
    c, cout, M = 32, 64, 8
    i = H.td_inputs(c, cout, M)
    assert i["B"] == 2
    n, m = i["n"], i["m"]
    got_idx, _ = pointops.knn(16, D(i["p"]), D(i["new_p"]), 2, n, m)
    assert torch.equal(got_idx.cpu(), i["knn_idx"])
    got = run_td(i)
    alone = dict(i, p=i["p"][n:], x=i["x"][n:], new_p=i["new_p"][m:], knn_idx=i["knn_idx"][m:] - n)
    assert torch.equal(run_td(alone), got[m:]), "the second sample launched alone differs"


def test_transition_down_refuses_other_neighbour_counts():
    i = H.td_inputs(6, 32, 9)
    out = torch.full((9, 32), SENTINEL, device=dev())
    t = {k: D(i[k]) for k in ("p", "x", "new_p", "knn_idx", "W", "scale", "shift")}
    for k in (8, 15, 17):
        rc = ffi.load().afm_transition_down(t["p"].data_ptr(), t["x"].data_ptr(), 6, t["new_p"].data_ptr(), t["knn_idx"].data_ptr(), k, t["W"].data_ptr(), 32,
                                            t["scale"].data_ptr(), t["shift"].data_ptr(), out.data_ptr(), 9, None)
        with pytest.raises(ffi.AfmError, match="unsupported shape"):
            ffi.check(rc, "afm_transition_down")
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("family", H.TD_FAMILIES)
@pytest.mark.parametrize("c,cout,M", H.TD_FAMILY_SHAPES)
def test_transition_down_value_families(c, cout, M, family):
    i = H.td_inputs(c, cout, M, family)
    got = run_td(i)
    r32, r64 = H.td_reference(c, cout, M, family, F32), H.td_reference(c, cout, M, family, F64)
    if family == "all_negative":
        assert (got == 0).all(), "every pre-activation is negative: exactly 0"
        return
    cls(f"transition_down c={c} cout={cout} M={M} {family}", got, r32["out"], r64["out"], H.td_tol(c, cout, M, family))
    if family == "far_cloud":
        near = dict(i, p=i["p"] - H.FAR, new_p=i["new_p"] - H.FAR)
        assert torch.equal(got, run_td(near)), "the translated cloud gives other bits than the untranslated one"


# ================================================================================================ afm_segment_mean
@pytest.mark.parametrize("family", H.SEG_FAMILIES)
@pytest.mark.parametrize("B,n,c", H.SEG_CASES)
def test_segment_mean_is_in_the_class_and_a_function_of_the_sample(B, n, c, family):
    """Against torch.mean in float32 and float64, margin 4.  One ascending float32 chain over the n rows - the kernel this test was written
    against - leaves the class from n = 2048 on: ratio max 6.0 / 5.3 / 11.5 (gauss / relu / mean50) at (2, 2048, 32), 12.1 / 21.5 / 22.4 at
    (2, 8192, 32), 16.3 / 18.3 / 21.8 at (1, 8192, 257), measured on the MI355X with that library.  The fixed-order blocked sum: at most 1.37."""
    x = H.seg_inputs(B, n, c, family)
    xd = D(x)
    got = pointops.segment_mean(xd, B, n)
    r32, r64 = H.segment_mean_restatement(x, B, n, F32), H.segment_mean_restatement(x, B, n, F64)
    cls(f"segment_mean B={B} n={n} c={c} {family}", got, r32, r64, H.SEG_TOL)
    assert torch.equal(got, pointops.segment_mean(xd, B, n)), "two runs differ"
    for b in sorted({0, B - 1}):                                        # a sample's mean does not depend on B or on its place in the batch
        assert torch.equal(pointops.segment_mean(xd[b * n: (b + 1) * n], 1, n)[0], got[b]), f"sample {b} launched alone differs"
    assert torch.equal(got.cpu(), H.blocked_f32_mean(x, B, n)), "not the stated order: 64 interleaved ascending chains, the tree, one division"


# ================================================================================================ afm_bn_fold
def bn_fold_call(i, C_, eps, scale, shift):
    t = {k: D(i[k]) for k in ("w", "b", "mean", "var", "lin_bias")}
    rc = ffi.load().afm_bn_fold(t["w"].data_ptr(), t["b"].data_ptr(), t["mean"].data_ptr(), t["var"].data_ptr(), eps, ffi.ptr(t["lin_bias"]),
                                scale.data_ptr(), shift.data_ptr(), C_, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("C_", H.FOLD_C)
def test_bn_fold_is_the_float32_expression_bit_for_bit(C_, with_bias):
    """Bit for bit against the float32 expression with every operation correctly rounded (H.bn_fold_ieee32, numpy).  Against torch's
    float32 evaluation of the same expression only the class is asserted: torch's CPU sqrt is not correctly rounded on every host (measured
    on the MI355X machine's AVX-512 CPU: var = 1e-12 came out one ulp low in 393 of 513 scales, the kernel agreeing with numpy)."""
    for var in H.FOLD_VAR:
        i = H.fold_inputs(C_, var, with_bias)
        scale, shift = torch.full((C_ + 3,), SENTINEL, device=dev()), torch.full((C_ + 3,), SENTINEL, device=dev())
        assert bn_fold_call(i, C_, H.BN_EPS, scale, shift) == 0
        si, ti = H.bn_fold_ieee32(i["w"], i["b"], i["mean"], i["var"], H.BN_EPS, i["lin_bias"])
        for name, got, want in (("scale", scale[:C_].cpu(), si), ("shift", shift[:C_].cpu(), ti)):
            ulps = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs()
            print(f"[identity] bn_fold C={C_} var={var:g} bias={with_bias} {name}: {int((ulps > 0).sum())} of {C_} differ, at most {int(ulps.max())} ulp")
        assert torch.equal(scale[:C_].cpu(), si) and torch.equal(shift[:C_].cpu(), ti), f"C={C_} var={var}: not the float32 expression"
        assert (scale[C_:] == SENTINEL).all() and (shift[C_:] == SENTINEL).all(), "written past C"
        s32, t32 = H.bn_fold_restatement(i["w"], i["b"], i["mean"], i["var"], H.BN_EPS, i["lin_bias"], F32)
        s64, t64 = H.bn_fold_restatement(i["w"], i["b"], i["mean"], i["var"], H.BN_EPS, i["lin_bias"], F64)
        record = C_ == 513
        for name, got, r32, r64 in (("scale", scale[:C_], s32, s64), ("shift", shift[:C_], t32, t64)):
            div = r64.abs().max().item()
            report_f32_class(f"point-infer edges bn_fold C={C_} var={var:g} bias={with_bias} {name}", got.cpu() / div, r32 / div, r64 / div, H.FOLD_TOL,
                             margin=H.MARGIN, select=None, record=record)


def test_bn_fold_refusals_and_the_empty_call():
    i = H.fold_inputs(257, 1.0, True)
    scale, shift = torch.full((257,), SENTINEL, device=dev()), torch.full((257,), SENTINEL, device=dev())
    for eps in (-1e-5, float("nan")):
        with pytest.raises(ffi.AfmError, match="bad argument"):
            ffi.check(bn_fold_call(i, 257, eps, scale, shift), "afm_bn_fold")
    assert bn_fold_call(i, 0, H.BN_EPS, scale, shift) == 0
    assert (scale == SENTINEL).all() and (shift == SENTINEL).all()


# ================================================================================================ afm_gather_rows
@pytest.mark.parametrize("rows,c", H.GATHER_CASES)
def test_gather_rows_is_indexing(rows, c):
    src, idx = H.gather_inputs(rows, c)
    got = pointops.gather_rows(D(src), D(idx))
    assert torch.equal(got.cpu(), H.gather_rows_restatement(src, idx))


# ================================================================================================ the kNN / FPS contract
def knn_entry(k, p, q, B, n, m, ws=False):
    """afm_knn, or afm_knn_ws with its workspace, into sentinel-filled outputs -> (idx, dist2) on the host"""
    lib = ffi.load()
    idx = torch.full((B * m, k), -7, dtype=torch.int32, device=dev())
    d2 = torch.full((B * m, k), SENTINEL, device=dev())
    if ws:
        nbytes = int(lib.afm_knn_workspace_bytes(k, B, n, m))
        space = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
        rc = lib.afm_knn_ws(k, p.data_ptr(), q.data_ptr(), B, n, m, idx.data_ptr(), d2.data_ptr(), space.data_ptr() if nbytes else None, nbytes, None)
    else:
        rc = lib.afm_knn(k, p.data_ptr(), q.data_ptr(), B, n, m, idx.data_ptr(), d2.data_ptr(), None)
    ffi.check(rc, "afm_knn_ws" if ws else "afm_knn")
    torch.cuda.synchronize()
    return idx.cpu(), d2.cpu()


def check_knn(k, p, q, B, n, m, pruned):
    """both entry points against the extended oracle, bit for bit; rule 1 and `every entry written` on each output"""
    want_i, want_d = H.knn_oracle(k, p, q, B, n, m)
    pd = D(p)
    qd = pd if q is p else D(q)
    nbytes = int(ffi.load().afm_knn_workspace_bytes(k, B, n, m))
    assert (nbytes > 0) == pruned
    outs = {"afm_knn": knn_entry(k, pd, qd, B, n, m), "afm_knn_ws": knn_entry(k, pd, qd, B, n, m, ws=True)}
    for name, (gi, gd) in outs.items():
        assert (gi != -7).all() and (gd != SENTINEL).all(), f"{name}: an entry was not written"
        H.check_contract(gi, gd, k, B, n, m)
        assert torch.equal(gi, want_i), f"{name}: {(gi != want_i).sum().item()} of {gi.numel()} indices differ from the oracle"
        assert torch.equal(gd.view(torch.int32), want_d.view(torch.int32)), f"{name}: dist2 differs from the oracle"
    assert torch.equal(outs["afm_knn"][0], outs["afm_knn_ws"][0]) and torch.equal(outs["afm_knn"][1].view(torch.int32), outs["afm_knn_ws"][1].view(torch.int32))


@pytest.mark.parametrize("k,B,n,m", H.PLAIN_KNN)
def test_knn_contract_plain_kernel(k, B, n, m):
    p, q, _, _ = H.knn_case(k, B, n, m, "none", 0)
    check_knn(k, p, q, B, n, m, pruned=False)                            # finite input, n < k among it
    for where, count in H.SPOILED:
        p, q, _, _ = H.knn_case(k, B, n, m, where, H.all_but_k(n, k, count))
        check_knn(k, p, q, B, n, m, pruned=False)


@pytest.mark.parametrize("k,B,n,m,count", H.PRUNED_KNN)
def test_knn_contract_pruned_form(k, B, n, m, count):
    """self-search (the candidates are the queries: the spoiled points are spoiled queries too) and a separate query cloud"""
    count = H.all_but_k(n, k, count)
    p, q, _, _ = H.knn_case(k, B, n, m, "both", count)
    assert q is p
    check_knn(k, p, q, B, n, m, pruned=True)
    p, q, _, _ = H.knn_case(k, B, n, m, "candidates", count, seed=1)
    check_knn(k, p, q, B, n, m, pruned=True)


def test_knn_contract_pruned_form_spoiled_queries():
    k, B, n = 16, 2, 4096
    p, q, _, qbad = H.knn_case(k, B, n, n, "queries", 64)
    assert qbad.sum().item() == 128
    check_knn(k, p, q, B, n, n, pruned=True)


@pytest.mark.parametrize("n,m", [(300, 40), (4096, 64)])
@pytest.mark.parametrize("value", ["nan", "inf"])
def test_fps_writes_indices_of_its_sample_whatever_the_coordinates(value, n, m):
    """rule 1 only: one plain-kernel and one pruned-kernel shape (csrc/fps_plan.h), a NaN or an infinite point in each sample"""
    B = 2
    p = H.cloud(B, n, seed=83).view(B, n, 3).clone()
    v = float(value)
    p[0, 7, 1] = v
    p[1, n - 3, :] = v
    p[1, 11, 2] = -v
    idx = torch.full((B * m,), -7, dtype=torch.int32, device=dev())
    pd = D(p.reshape(B * n, 3).contiguous())
    ffi.check(ffi.load().afm_fps(pd.data_ptr(), B, n, m, idx.data_ptr(), None), "afm_fps")
    torch.cuda.synchronize()
    got = idx.cpu().view(B, m).long()
    lo = (torch.arange(B) * n).view(B, 1)
    assert (got != -7).all() and ((got >= lo) & (got < lo + n)).all(), "an FPS index outside its sample"
    assert (got[:, 0] == lo[:, 0]).all()


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (committed as profiles/point_infer_edges_parity.json)."""
    write_parity_table()
