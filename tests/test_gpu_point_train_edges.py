"""`-m gpu`: the scene branch's training kernels (csrc/pointnet_train.hip: BatchNorm statistics / affine / backward, the scatter plan and the
segmented sum, group max, grouping, the vector-attention aggregation in its fused and its two-pass form; afm_interpolate and its segmented
backward) against the float64 restatements of tests/test_point_train_edges_host.py, at the shapes, dispatch arms and values that module
builds and proves on the host.

Every inexact quantity is bounded by the float32 restatement's OWN error against its float64 twin (gpu_util.report_f32_class, margin 4);
the absolute tolerances are the ones tests/test_gpu_train.py states for the same operators.  What is an exact function of its inputs - the
plan, a sum in a fixed order, a maximum, a copy, a single float32 operation - is asserted bit for bit.  The figures go to
profiles/point_train_edges_parity.json.

Index lists with out-of-range entries go ONLY to the plan and the segmented sum, which skip them; the gathers and the atomic scatter-adds
do not check their indices and never see such a list here."""
import ctypes as C

import pytest
import torch

from afm import autograd_points as AP
from afm import ffi
from gpu_util import dev, report, report_f32_class, write_parity_table
import test_point_train_edges_host as H

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
AFM_E_BADARG = -1


def offset_view(t):
    """The same values on the device, contiguous, starting 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def cls(name, got, want32, want64, tol, div=1.0, floor_at=None):
    got = got.detach().cpu()
    report(name, got / div, want64 / div, tol)
    return report_f32_class(name, got / div, want32 / div, want64 / div, tol, floor_at=floor_at)


# ================================================================================================ BatchNorm
def run_bn(name, offset=False, mode="train", bn=None):
    rows, Cn, fam, relu, has_res, _ = H.bn_cases()[name]
    i = H.bn_inputs(name)
    put = offset_view if offset else (lambda t: t.to(dev()))
    if bn is None:
        bn = torch.nn.BatchNorm1d(Cn, eps=H.EPS, momentum=H.MOMENTUM)
        with torch.no_grad():
            bn.weight.copy_(i["gamma"]); bn.bias.copy_(i["beta"])
        bn = bn.to(dev())
    bn.train(mode == "train")
    bn.weight.grad = bn.bias.grad = None
    x = put(i["x"]).requires_grad_(True)
    res = None if i["res"] is None else put(i["res"]).requires_grad_(True)
    y = AP.batch_norm(x, bn, relu=relu, residual=res)
    (y * put(i["dy"])).sum().backward()
    out = dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad.clone(), dbeta=bn.bias.grad.clone(), running_mean=bn.running_mean.clone(),
               running_var=bn.running_var.clone())
    if res is not None:
        out["dres"] = res.grad
    return out, bn


def check_bn(name, got, mode="train", label=None):
    r32, r64 = H.bn_reference(name, F32, mode), H.bn_reference(name, F64, mode)
    worst = 0.0
    for key, tol, div, floor_at in H.bn_checks(name, mode):
        worst = max(worst, cls(f"point-train edges BN {label or name} {mode} {key}", got[key], r32[key].double(), r64[key], tol, div, floor_at)[0])
    return worst


@pytest.mark.parametrize("rows", H.BN_ROWS)
@pytest.mark.parametrize("Cn", H.BN_CS)
def test_batch_norm_every_lane_arm_and_row_count(Cn, rows):
    name = f"shape_{rows}x{Cn}"
    got, bn = run_bn(name)
    check_bn(name, got)
    assert int(bn.num_batches_tracked) == 1
    # frozen (eval): the float64 reference's running statistics are the constants; the module's own are within the class of them (above)
    with torch.no_grad():
        r64 = H.bn_reference(name, F64)
        bn.running_mean.copy_(r64["running_mean"]); bn.running_var.copy_(r64["running_var"])
    got, _ = run_bn(name, mode="eval", bn=bn)
    check_bn(name, got, "eval")


@pytest.mark.parametrize("name", ["4097x32", "70001x64"])
def test_batch_norm_scalar_arm_on_an_offset_view_agrees_with_the_aligned_launch(name):
    """A power-of-two C on pointers 4 bytes off a 16-byte boundary takes colstats_kernel<MODE, 1>; (70001, 64) there also meets the cap of
    1024 chunks with chunks that hold no row, and both launches a second and third grid-stride trip of colaffine / bn_bwd_apply."""
    al, off = ("aligned_" if name == "4097x32" else "large_") + name, ("offset_view_" if name == "4097x32" else "large_offset_view_") + name
    a, _ = run_bn(al)
    b, _ = run_bn(off, offset=True)
    check_bn(al, a)
    check_bn(off, b)
    for key in ("dres",) if "dres" in a else ():
        assert torch.equal(a[key], b[key])                              # the masked dy: no statistics in it


@pytest.mark.parametrize("Cn", [32, 96])
@pytest.mark.parametrize("fam", H.BN_FAMILIES)
def test_batch_norm_value_families(fam, Cn):
    name = f"{fam}_4097x{Cn}"
    got, _ = run_bn(name)
    check_bn(name, got)
    if fam == "constant_columns":
        for c, v in H.CONST_COLS.items():
            kept = (torch.tensor(1.0) - torch.tensor(H.MOMENTUM, dtype=F32)).item()              # (1 - momentum) * 1 + momentum * 0, in float32
            assert got["running_var"][c].item() == kept, "the variance of a constant column is exactly 0"
    if fam == "relu_nonpositive_columns":
        for c in H.NONPOS_COLS:
            assert (got["y"][:, c] == 0).all() and (got["dx"][:, c] == 0).all() and got["dgamma"][c] == 0 and got["dbeta"][c] == 0
    if fam == "relu_exact_zeros":
        i = H.bn_inputs(name)
        for c in H.ZERO_COLS:
            r, dy = i["res"][:, c].to(dev()), i["dy"][:, c].to(dev())
            assert torch.equal(got["y"][:, c], torch.relu(r)) and (got["dx"][:, c] == 0).all()
            assert torch.equal(got["dres"][:, c], torch.where(r > 0, dy, torch.zeros_like(dy))), "an output of exactly 0 passes no gradient"


@pytest.mark.parametrize("world,rows,Cn", H.SYNC_CASES)
def test_batch_norm_sync_combination_of_rank_statistics(world, rows, Cn):
    """afm_colstats on `world` equal row slices, the [world][3C] blocks through afm_bn_finalize: the parallel-variance combination and the
    unbiased count - 1, against BatchNorm over all rows.  No process group."""
    lib = ffi.load()
    i = H.sync_inputs(world, rows, Cn)
    x, gamma, beta = i["x"].to(dev()), i["gamma"].to(dev()), i["beta"].to(dev())
    stats = torch.empty(world, 3 * Cn, device=dev())
    ws = torch.empty(max(16, lib.afm_colstats_workspace_bytes(rows, Cn)), dtype=torch.uint8, device=dev())
    for r in range(world):
        part = x[r * rows: (r + 1) * rows]
        ffi.check(lib.afm_colstats(part.data_ptr(), rows, Cn, stats[r].data_ptr(), ws.data_ptr(), ws.numel(), None), "afm_colstats")
    out = {k: torch.empty(Cn, device=dev()) for k in ("mean", "rstd", "scale", "shift")}
    out["running_mean"], out["running_var"] = torch.zeros(Cn, device=dev()), torch.ones(Cn, device=dev())
    ffi.check(lib.afm_bn_finalize(stats.data_ptr(), world, rows, gamma.data_ptr(), beta.data_ptr(), H.EPS, H.MOMENTUM, out["running_mean"].data_ptr(),
                                  out["running_var"].data_ptr(), out["mean"].data_ptr(), out["rstd"].data_ptr(), out["scale"].data_ptr(),
                                  out["shift"].data_ptr(), Cn, None), "afm_bn_finalize")
    r32, r64 = H.sync_reference(world, rows, Cn, F32), H.sync_reference(world, rows, Cn, F64)
    for key in H.SYNC_CHECKED:
        cls(f"point-train edges BN sync world={world} {rows}x{Cn} {key}", out[key], r32[key].double(), r64[key], H.sync_tol(r64[key]))


# ================================================================================================ scatter plan / segmented sum
@pytest.mark.parametrize("n_dst,entries,kind", H.PLAN_CASES)
def test_scatter_plan_and_segmented_sum_are_exact(n_dst, entries, kind):
    idx = H.plan_indices(n_dst, entries, kind)
    off, ent = H.plan_reference(idx, n_dst)
    idx_d = idx.to(dev())
    plan = AP.scatter_plan(idx_d, n_dst)
    got_off = plan[: n_dst + 1].cpu().long()
    assert got_off[n_dst].item() == ent.numel(), "off[n_dst] is the number of valid entries"
    assert torch.equal(got_off, off), "the offsets are the exclusive prefix of the bincount"
    assert torch.equal(plan[n_dst + 1: n_dst + 1 + ent.numel()].cpu().long(), ent), "the plan is the stable sort of the valid entries"
    rows = max(entries, 1)
    layouts = H.SEG_LAYOUTS if entries <= 300_000 else H.SEG_LAYOUTS[:2]
    for Cn, ld, col in layouts:
        src = H.g(f"pte_seg_src_{rows}_{ld}", (rows, ld))
        want = H.ascending_f32_sum(src, col, Cn, off, ent)
        src_d = src.to(dev())
        outs = [AP._segment_sum(src_d, col, idx_d, n_dst, Cn) for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "repeats differ"
        assert torch.equal(outs[0].cpu(), want), f"C={Cn} ld={ld} offset={col}: not the ascending float32 sum"


def test_gather_and_broadcast_rows_are_exact():
    n, Cn = 500, 35
    idx = H.plan_indices(n, 7000, "uniform")
    feat, dy = H.g("pte_ga_f", (n, Cn)), H.g("pte_ga_dy", (7000, Cn))
    f = feat.to(dev()).requires_grad_(True)
    out = AP.gather(f, idx.to(dev()))
    assert torch.equal(out.detach().cpu(), feat[idx.long()])
    (out * dy.to(dev())).sum().backward()
    off, ent = H.plan_reference(idx, n)
    assert torch.equal(f.grad.cpu(), H.ascending_f32_sum(dy, 0, Cn, off, ent))
    for n_rep in (1, 2, 513):
        rows, dyb = H.g("pte_bc_rows", (4, 24)), H.g(f"pte_bc_dy_{n_rep}", (4 * n_rep, 24))
        r = rows.to(dev()).requires_grad_(True)
        got = AP.broadcast_rows(r, n_rep)
        assert torch.equal(got.detach().cpu(), rows.repeat_interleave(n_rep, 0))
        (got * dyb.to(dev())).sum().backward()
        assert torch.equal(r.grad.cpu(), H.group_ascending_f32_sum(dyb, n_rep)), f"broadcast_rows backward n={n_rep}"


# ================================================================================================ interpolation
@pytest.mark.parametrize("n,m,c", H.INTERP_CASES)
def test_interpolation_at_coincident_points(n, m, c):
    """afm_interpolate reads 16-byte lanes: c % 4 != 0 is AFM_E_BADARG (asserted), and those widths reach the segmented backward alone."""
    lib = ffi.load()
    i = H.interp_inputs(n, m, c)
    r32, r64 = H.interp_reference(n, m, c, F32), H.interp_reference(n, m, c, F64)
    idx, d2, feat, base, dout = (i[k].to(dev()) for k in ("idx", "d2", "feat", "base", "dout"))
    if c % 4:
        out = torch.empty(n, c, device=dev())
        assert lib.afm_interpolate(feat.data_ptr(), idx.data_ptr(), d2.data_ptr(), None, out.data_ptr(), n, c, 3, None) == AFM_E_BADARG
        grads = [AP._segment_sum(dout, 0, idx, m, c, row_div=3, d2=d2) for _ in range(3)]
    else:
        grads = []
        for with_base in (True, False, True):
            f = feat.clone().requires_grad_(True)
            b = base.clone().requires_grad_(True) if with_base else None
            out = AP._InterpolateFn.apply(f, b, idx, d2)
            key = "out" if with_base else "up"
            cls(f"point-train edges interpolate n={n} c={c} {key}", out, r32[key].double(), r64[key], H.AGG_TOL)
            (out * dout).sum().backward()
            grads.append(f.grad)
            assert b is None or torch.equal(b.grad, dout)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2]), "the segmented backward differs between repeats"
    div = max(r64["dfeat"].abs().max().item(), 1e-12)
    cls(f"point-train edges interpolate n={n} c={c} dfeat", grads[0], r32["dfeat"].double(), r64["dfeat"], H.SEG_TOL, div)


# ================================================================================================ grouping
@pytest.mark.parametrize("m,k,Cn", H.GROUP_MAX_CASES)
def test_group_max_ties_go_to_the_first_maximum(m, k, Cn):
    x, dy = H.tie_family(m, k, Cn), H.g(f"pte_tie_dy_{m}_{Cn}", (m, Cn))
    mx, _, dx = H.group_max_reference(x, dy, k)
    xg = x.to(dev()).requires_grad_(True)
    y = AP.group_max(xg, k)
    assert (y.detach().cpu() == mx).all(), "group max (by value: -0.0 == +0.0)"
    (y * dy.to(dev())).sum().backward()
    assert (xg.grad.cpu() == dx).all(), "the gradient goes to the first maximum, and only there"


@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("Cn", [0, 35])
def test_group_points_and_w0_are_single_float32_operations(Cn, k):
    n, m = 300, 37
    xyz, idx = H.g("pte_gp_xyz", (n, 3)), H.plan_indices(n, m * k, "uniform")
    new_xyz = H.g("pte_gp_new", (m, 3))
    feat = H.g("pte_gp_f", (n, Cn)) if Cn else None
    got = AP.group_points(xyz.to(dev()), new_xyz.to(dev()), None if feat is None else feat.to(dev()), idx.to(dev()), k)
    want = xyz[idx.long()] - new_xyz.repeat_interleave(k, 0)
    want = want if feat is None else torch.cat([want, feat[idx.long()]], 1)
    assert torch.equal(got.cpu(), want)
    Cw = max(Cn, 3)
    kg, pr, q = H.g("pte_w0_kg", (m * k, Cw)), H.g("pte_w0_pr", (m * k, Cw)), H.g("pte_w0_q", (m, Cw))
    w0 = AP.pt_w0(kg.to(dev()), q.to(dev()), pr.to(dev()), k)
    assert torch.equal(w0.cpu(), (kg - q.repeat_interleave(k, 0)) + pr)


# ================================================================================================ vector-attention aggregation
def run_aggregate(vg, pr, w2, dout, k, share, expect=0):
    """afm_pt_aggregate + afm_pt_aggregate_bwd on device tensors as they are (no copy: an offset view stays one) -> out, sw, da, dw2"""
    lib = ffi.load()
    Cn, m = vg.shape[1], vg.shape[0] // k
    like = offset_view if vg.data_ptr() % 16 else (lambda t: t)
    out, sw, da, dw2 = like(torch.zeros(m, Cn, device=dev())), like(torch.zeros_like(w2)), like(torch.zeros_like(vg)), like(torch.zeros_like(w2))
    rc = lib.afm_pt_aggregate(vg.data_ptr(), pr.data_ptr(), w2.data_ptr(), out.data_ptr(), sw.data_ptr(), m, k, Cn, share, None)
    rc2 = lib.afm_pt_aggregate_bwd(vg.data_ptr(), pr.data_ptr(), sw.data_ptr(), dout.data_ptr(), da.data_ptr(), dw2.data_ptr(), m, k, Cn, share, None)
    assert rc == expect and rc2 == expect, (rc, rc2)
    return dict(out=out, sw=sw, da=da, dw2=dw2)


@pytest.mark.parametrize("name", sorted(H.AGG_CASES))
def test_aggregation_in_both_arms_and_at_the_softmax_edges(name):
    m, k, Cn, share, family, _, _ = H.AGG_CASES[name]
    i = H.agg_inputs(m, k, Cn, share, family)
    r32, r64 = H.agg_reference(name, F32), H.agg_reference(name, F64)
    got = run_aggregate(*(i[key].to(dev()) for key in ("vg", "pr", "w2", "dout")), k, share)
    Cs = Cn // share
    if k == 1:
        assert (got["sw"] == 1).all() and (got["dw2"] == 0).all(), "one neighbour: the softmax is exactly 1 and carries no gradient"
    if family == "spread_200":
        w = i["w2"].view(m, k, Cs)
        dead = ((w.max(1, keepdim=True).values - w) > H.UNDERFLOW).reshape(m * k, Cs).to(dev())
        assert (got["sw"][dead] == 0).all() and (got["dw2"][dead] == 0).all(), "a probability that underflows is exactly 0, and so is its gradient"
    for key, tol, is_scaled in H.AGG_CHECKED:
        if k == 1 and key == "dw2":
            continue
        div = max(r64[key].abs().max().item(), 1e-12) if is_scaled else 1.0
        cls(f"point-train edges pt_aggregate {name} {key}", got[key], r32[key].double(), r64[key], tol, div)
    # the autograd wrapper hands out the same numbers
    t = {key: i[key].to(dev()).requires_grad_(key != "dout") for key in ("vg", "pr", "w2", "dout")}
    out = AP.pt_aggregate(t["vg"], t["pr"], t["w2"], k, share)
    (out * t["dout"]).sum().backward()
    assert torch.equal(out.detach(), got["out"]) and torch.equal(t["vg"].grad, got["da"]) and torch.equal(t["pr"].grad, got["da"]) and torch.equal(t["w2"].grad, got["dw2"])


def test_aggregation_two_pass_arm_by_alignment_matches_the_fused_arm():
    """Every tensor 4 bytes off a 16-byte boundary takes the two-pass kernels on a shape the fused kernels take when aligned; the source
    says the arms share arithmetic and order: out, sw, da and dw2 are compared bit for bit (and both with float64)."""
    m, k, Cn, share = H.ALIGN_CASE
    i = H.agg_inputs(m, k, Cn, share, "scale_8")
    args = [i[key] for key in ("vg", "pr", "w2", "dout")]
    fused = run_aggregate(*(t.to(dev()) for t in args), k, share)
    two = run_aggregate(*(offset_view(t) for t in args), k, share)
    r32 = H.agg_restatement(*args, k, share, F32)
    r64 = H.agg_restatement(*args, k, share, F64)
    for key, tol, is_scaled in H.AGG_CHECKED:
        div = max(r64[key].abs().max().item(), 1e-12) if is_scaled else 1.0
        for arm, got in (("fused", fused), ("two-pass (offset views)", two)):
            cls(f"point-train edges pt_aggregate alignment {arm} {key}", got[key], r32[key].double(), r64[key], tol, div)
    differ = {key: int((fused[key] != two[key]).sum()) for key in ("out", "sw", "da", "dw2")}
    print(f"[identity] fused vs two-pass, elements that differ: {differ}")
    assert not any(differ.values()), f"the two arms differ: {differ}"


def test_aggregation_rejects_more_than_sixteen_neighbours():
    m, k, Cn, share = 5, 17, 32, 8
    t = [torch.zeros(m * k, Cn, device=dev()), torch.zeros(m * k, Cn, device=dev()), torch.zeros(m * k, Cn // share, device=dev()), torch.zeros(m, Cn, device=dev())]
    run_aggregate(*t, k, share, expect=AFM_E_BADARG)


def test_aggregation_second_grid_trip():
    """(C, share, k) = (512, 8, 16): one point per workgroup and 4096 workgroups, so the last 3 of 4099 points are a second trip.  Inputs
    tiled on the device from 7 points; the last 3 points equal the same 3 launched alone bit for bit, a 64-point sample float64."""
    m, k, Cn, share, period = H.SECOND_TRIP
    i = H.agg_inputs(period, k, Cn, share, "scale_8")
    reps = (m + period - 1) // period
    tile = lambda t, rows: t.to(dev()).view(period, rows, -1).repeat(reps, 1, 1)[:m].reshape(m * rows, -1).contiguous()
    vg, pr, w2, dout = tile(i["vg"], k), tile(i["pr"], k), tile(i["w2"], k), tile(i["dout"], 1)
    got = run_aggregate(vg, pr, w2, dout, k, share)
    tail = run_aggregate(vg[-3 * k:].clone(), pr[-3 * k:].clone(), w2[-3 * k:].clone(), dout[-3:].clone(), k, share)
    for key, rows in (("out", 1), ("sw", k), ("da", k), ("dw2", k)):
        assert torch.equal(got[key][-3 * rows:], tail[key]), f"{key}: the second trip differs from the same points launched alone"
    pts = torch.cat([torch.arange(0, 4096, 67)[:61], torch.tensor([4096, 4097, 4098])])
    r32 = H.agg_restatement(i["vg"], i["pr"], i["w2"], i["dout"], k, share, F32)
    r64 = H.agg_restatement(i["vg"], i["pr"], i["w2"], i["dout"], k, share, F64)
    for key, tol, is_scaled in H.AGG_CHECKED:
        rows = 1 if key == "out" else k
        pick = lambda t, mod: t.view(-1, rows, t.shape[-1])[pts % mod if mod else pts].reshape(len(pts) * rows, -1)
        want32, want64 = pick(r32[key], period).double(), pick(r64[key], period)
        div = max(want64.abs().max().item(), 1e-12) if is_scaled else 1.0
        cls(f"point-train edges pt_aggregate second trip {key}", pick(got[key].cpu(), 0), want32, want64, tol, div)


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (committed as profiles/point_train_edges_parity.json)."""
    write_parity_table()
