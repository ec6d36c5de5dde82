"""`-m gpu`: the transformer trunk's training path on the HIP kernels against the float64 restatements of
tests/test_trunk_train_edges_host.py, on the cases that module builds and proves on the host.

A. AG.encoder_layer, AG.decoder_layer and the whole CMDM in TRAIN mode against the oracle evaluated with the same keep-masks
   (oracle/rng_ref.keep_mask at the ids afm/autograd.py uses): a backward that regenerated another mask than its forward - another id, row
   and column exchanged, inv_keep left out - leaves the bound, as the host module proves on the reference.  Every one of the four
   (encoder) and six (decoder) mask sites is covered by test_encoder_layer_train_mode / test_decoder_layer_train_mode.  No dropped tensor
   of a layer is an output (a LayerNorm follows each), so the bit-for-bit zeros are asserted where they can be seen: dx_drop (C) and
   the epilogue (D).
B. afm_linear_wgrad on every path - wgrad_flat_kernel, wgrad_skinny_kernel (all tile pairs), wgrad_kernel<true / false> - with db = NULL,
   accumulate = 1, lddw != K, row maps, a workspace one byte short, and on value families: test_linear_wgrad_every_path_and_argument.
C. afm_layernorm / afm_layernorm_rows / afm_layernorm_bwd (layernorm_bwd_kernel<1 / 2 / 4>, layernorm_bwd_generic_kernel) at the edges of
   their arms, past the block cap, on value families, with dropout: test_layernorm_*.
D. afm_masked_mse(_bwd), afm_rowop with act' on a ladder, afm_transpose, the training epilogue of afm_linear.

Every inexact quantity is bounded by the float32 CPU run's OWN error against float64 (gpu_util.report_f32_class, margin 4) below the
tolerance the host module states; what is an exact function of its inputs is asserted bit for bit.  The figures are committed as
profiles/trunk_train_edges_parity.json (500 rows); worst ratio e_hip / (e_ref + floor / 4) per group there, against the margin 4:
encoder layer 1.58, decoder layer 1.32, CMDM 1.80, wgrad shapes 1.88 and families 1.24, LayerNorm shapes 1.75, families 1.32 and mapped
rows 0.87, masked MSE 2.49, rowop 0.88, act' 0.87, epilogue 0.93."""
import ctypes as C

import pytest
import torch

from afm import autograd as AG
from afm import ffi
from afm.base import create_model_and_diffusion
from gpu_util import dev, load_named_weights, report, report_f32_class, write_parity_table
from oracle import denoiser_ref as dr
from oracle import rng_ref
from test_gpu_cmdm import cmdm_cfg
import test_trunk_train_edges_host as H

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SENTINEL = -777.25


def offset_view(t):
    """The same values on the device, contiguous, starting 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def cls(name, got, want32, want64, tol, div=1.0, floor_at=None, select=None):
    got = got.detach().cpu().double()
    if select is not None:
        got, want32, want64 = got[select], want32[select], want64[select]
    report(name, got / div, want64 / div, tol)
    return report_f32_class(name, got / div, want32.double() / div, want64 / div, tol, floor_at=floor_at)


def st(t):
    return ffi.stream_of(t)


# ================================================================================================ A. train mode
def make_layer(kind):
    ctor = torch.nn.TransformerEncoderLayer if kind == "enc" else torch.nn.TransformerDecoderLayer
    layer = ctor(d_model=H.LD, nhead=H.LH, dim_feedforward=H.LFF, dropout=0.0, activation="gelu", batch_first=True)
    layer.load_state_dict(H.layer_weights(kind))
    return layer.to(dev())


def check_layer(tag, got, r32, r64):
    assert set(got) == set(r64)
    for key, tol, div in H.layer_checks(r64):
        cls(f"trunk-train edges {tag} {key}", got[key], r32[key], r64[key], tol, div)


@pytest.mark.parametrize("name", sorted(H.ENC_CASES))
def test_encoder_layer_train_mode(name):
    """forward, dx and the twelve parameter gradients with the four dropouts on (ids id0 .. id0 + 3), T = 70 across a 64-key block"""
    T, p, seed = H.ENC_CASES[name]
    i, layer = H.enc_inputs(T), make_layer("enc")
    x = i["x"].to(dev()).requires_grad_(True)
    y = AG.encoder_layer(x, layer, i["km"].to(dev()), H.LH, (p, seed, H.ENC_ID0))
    (y * i["dy"].to(dev())).sum().backward()
    got = dict(out=y.detach(), dx=x.grad, **{"d" + n: q.grad for n, q in layer.named_parameters()})
    check_layer(f"encoder layer {name}", got, H.enc_reference(name, F32), H.enc_reference(name, F64))


def test_decoder_layer_train_mode():
    """forward, dx, dmem and the eighteen parameter gradients with the six dropouts on (ids id0 .. id0 + 5).  The rows of padded queries
    (at most T // 3 rows of sample 0; nothing reads them) are left out of the output and of dx: the only exclusion."""
    i, layer = H.dec_inputs(), make_layer("dec")
    valid = ~i["km"]
    x, mem = i["x"].to(dev()).requires_grad_(True), i["mem"].to(dev()).requires_grad_(True)
    y = AG.decoder_layer(x, mem, layer, i["km"].to(dev()), i["mm"].to(dev()), H.LH, (H.DEC_P, H.DEC_SEED, H.DEC_ID0))
    (y * (i["dy"] * valid[..., None]).to(dev())).sum().backward()
    got = dict(out=y.detach().cpu()[valid], dx=x.grad.cpu()[valid], dmem=mem.grad, **{"d" + n: q.grad for n, q in layer.named_parameters()})
    check_layer("decoder layer", got, H.dec_reference(F32), H.dec_reference(F64))


def test_cmdm_train_mode_loss_and_gradients():
    """model.train(): loss [B] and the 72 trunk gradients against oracle/train_ref run with the model's masks - id 1 on the positional
    encoding, ids 16 + 4 i .. + 3 in layer i, the seed afm.cmdm.drop_seed gives the first pass after torch.manual_seed(5)."""
    model, diff = create_model_and_diffusion(cmdm_cfg(), device=dev())
    load_named_weights(model)
    model = model.to(dev())
    model.contact_encoder.requires_grad_(False)
    model.train()
    assert model.dropout_p == H.CMDM_P and float(model.positional_encoder.dropout.p) == H.CMDM_P_POS
    assert len(model.self_attn_layer.layers) == H.CMDM_LAYERS and model.num_heads == H.CMDM_H
    i = H.cmdm_inputs()
    kw = dict(c_text_feat=i["text"].to(dev()), c_cont_emb=i["cont"].to(dev()), x_mask=i["x_mask"].to(dev()))
    torch.manual_seed(H.CMDM_SEED_ARGS[0])
    model._drop_calls = 0
    model.zero_grad()
    terms = diff.training_losses(model, i["x0"].to(dev()), i["t"].to(dev()), model_kwargs=kw, noise=i["noise"].to(dev()))
    terms["loss"].mean().backward()
    assert model._drop_calls == H.CMDM_SEED_ARGS[1]
    (l32, g32), (l64, g64) = H.cmdm_reference(F32), H.cmdm_reference(F64)
    cls("trunk-train edges CMDM train-mode loss", terms["loss"], l32, l64, H.LOSS_TOL)
    params = dict(model.named_parameters())
    assert len(g64) == 72
    for k, want in g64.items():
        assert params[k].grad is not None, k
        cls(f"trunk-train edges CMDM train-mode d{k}", params[k].grad, g32[k], want, H.MODEL_GRAD_TOL, max(want.abs().max().item(), 1e-12))


# ================================================================================================ B. afm_linear_wgrad
def wg_operands(name):
    """-> (dY, lddy, X, ldx, dy_map, x_map) on the device in the case's layout; what the kernels must not read is NaN"""
    M, N, K, layout, pad, maps, fam, _ = H.WG_CASES[name]
    dy, x = H.wg_inputs(name)
    if maps:
        B, L, ty, offy, tx, offx = H.WG_MAPS[name]
        by, bx = torch.full((B * ty, N), float("nan")), torch.full((B * tx, K), float("nan"))
        by[H.mapped_rows(M, L, ty, offy)], bx[H.mapped_rows(M, L, tx, offx)] = dy, x
        return by.to(dev()), N, bx.to(dev()), K, (L, ty, offy), (L, tx, offx)
    if layout == "strided":
        by, bx = torch.full((M, N + 3), float("nan")), torch.full((M, K + 5), float("nan"))
        by[:, :N], bx[:, :K] = dy, x
        return by.to(dev()), N + 3, bx.to(dev()), K + 5, None, None
    put = offset_view if layout == "offset" else (lambda t: t.to(dev()))
    return put(dy), N, put(x), K, None, None


def run_wgrad(name, ops, *, want_db=True, prior=None, short=False):
    """One afm_linear_wgrad call with exactly the workspace bytes the case's path asks for (one less: short) -> (rc, dW [N, lddw], db)"""
    lib = ffi.load()
    M, N, K, layout, pad, maps, fam, _ = H.WG_CASES[name]
    dY, lddy, X, ldx, dy_map, x_map = ops
    need = H.wgrad_path(M, N, K, layout, pad, maps)[2]
    total = int(lib.afm_linear_wgrad_workspace_bytes(M, N, K))
    assert 0 < need <= total == H.wgrad_workspace_bytes(M, N, K), "the restated plans are not the library's"
    ws = torch.empty(total, dtype=torch.uint8, device=dev())              # the buffer itself is never short
    dW, db = torch.full((N, K + pad), SENTINEL, device=dev()), torch.full((N,), SENTINEL, device=dev())
    if prior is not None:
        dW[:, :K], db[:] = prior
    a = ffi.WgradArgs()
    a.dY, a.lddy, a.X, a.ldx, a.dW, a.lddw = dY.data_ptr(), lddy, X.data_ptr(), ldx, dW.data_ptr(), K + pad
    a.db = db.data_ptr() if want_db else None
    a.M, a.N, a.K = M, N, K
    if dy_map:
        a.dy_grp, a.dy_stride, a.dy_off = dy_map
    if x_map:
        a.x_grp, a.x_stride, a.x_off = x_map
    a.accumulate = 0 if prior is None else 1
    a.ws, a.ws_bytes = ws.data_ptr(), need - 1 if short else need
    rc = lib.afm_linear_wgrad(C.byref(a), st(dY))
    torch.cuda.synchronize()
    return rc, dW, db


@pytest.mark.parametrize("name", sorted(H.WG_CASES))
def test_linear_wgrad_every_path_and_argument(name):
    """The path each case takes is the one H.WG_CASES names (flat: wgrad_flat_kernel; skinny: wgrad_skinny_kernel; tiled: wgrad_kernel<VEC>,
    asserted on the host against the restated plans)."""
    M, N, K, layout, pad, maps, fam, path = H.WG_CASES[name]
    ops = wg_operands(name)
    rc, dW, db = run_wgrad(name, ops)
    assert rc == 0, rc
    r32, r64 = H.wg_reference(name, F32), H.wg_reference(name, F64)
    got = dict(dW=dW[:, :K], db=db)
    for key, tol, div, floor_at in H.wg_checks(name):
        cls(f"trunk-train edges wgrad {name} [{path[0]}] {key}", got[key], r32[key], r64[key], tol, div, floor_at)
    if pad:
        assert (dW[:, K:] == SENTINEL).all(), "the guard columns of dW (lddw > K) were written"
    # two runs give identical bits
    rc, dW2, db2 = run_wgrad(name, ops)
    assert rc == 0 and torch.equal(dW, dW2) and torch.equal(db, db2), "not deterministic"
    # db = NULL: dW unchanged in bits, db untouched
    rc, dW3, db3 = run_wgrad(name, ops, want_db=False)
    assert rc == 0 and torch.equal(dW, dW3) and (db3 == SENTINEL).all()
    # accumulate = 1: one finished sum added per element
    pw, pb = H.g(f"tte_wg_prior_w_{N}_{K}", (N, K)).to(dev()), H.g(f"tte_wg_prior_b_{N}", (N,)).to(dev())
    rc, dW4, db4 = run_wgrad(name, ops, prior=(pw, pb))
    assert rc == 0 and torch.equal(dW4[:, :K], pw + dW[:, :K]) and torch.equal(db4, pb + db), "accumulate != prior + plain"
    assert not pad or (dW4[:, K:] == SENTINEL).all()
    # a workspace one byte short
    rc, dW5, db5 = run_wgrad(name, ops, short=True)
    assert rc == H.AFM_E_WORKSPACE and (dW5 == SENTINEL).all() and (db5 == SENTINEL).all()


# ================================================================================================ C. LayerNorm
def ln_forward(x, gamma, beta, y=None, rows=None, row_map=(0, 0, 0), expect=0):
    dim = x.shape[-1]
    y = torch.empty_like(x) if y is None else y
    rc = ffi.load().afm_layernorm_rows(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), x.numel() // dim if rows is None else rows,
                                       dim, H.LN_EPS, *row_map, st(x))
    assert rc == expect, rc
    return y


def ln_backward(x, gamma, dy, drop=None, put=None, expect=0):
    """-> dx, dx_drop (None without dropout), dgamma, dbeta; outputs pre-filled with the sentinel; put: how outputs are allocated"""
    lib = ffi.load()
    put = put or (lambda t: t.to(dev()))
    rows, dim = x.shape
    dx, dg, db = put(torch.full((rows, dim), SENTINEL)), torch.full((dim,), SENTINEL, device=dev()), torch.full((dim,), SENTINEL, device=dev())
    dxd = put(torch.full((rows, dim), SENTINEL)) if drop else None
    ws = torch.empty(max(int(lib.afm_layernorm_bwd_workspace_bytes(rows, dim)), 16), dtype=torch.uint8, device=dev())
    p, seed, did = drop or (0.0, 0, 0)
    rc = lib.afm_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.data_ptr(), ffi.ptr(dxd), dg.data_ptr(), db.data_ptr(), rows, dim,
                               H.LN_EPS, p, seed, did, ws.data_ptr(), ws.numel(), st(x))
    assert rc == expect, rc
    return dx, dxd, dg, db


@pytest.mark.parametrize("name", sorted(H.ln_cases()))
def test_layernorm_forward_backward_every_arm_and_family(name):
    rows, dim, fam, offset, has_bwd = H.ln_cases()[name]
    i, r32, r64 = H.ln_inputs(name), H.ln_reference(name, F32), H.ln_reference(name, F64)
    put = offset_view if offset else (lambda t: t.to(dev()))
    x, gamma, beta, dy = (put(i[k]) for k in ("x", "gamma", "beta", "dy"))
    got = dict(y=ln_forward(x, gamma, beta, put(torch.empty(rows, dim))))
    if has_bwd:
        got["dx"], _, got["dgamma"], got["dbeta"] = ln_backward(x, gamma, dy, put=put)
    else:                                                 # wider than 1024: no backward kernel, and nothing is written
        dx, _, dg, db = ln_backward(x, gamma, dy, expect=H.AFM_E_UNSUPPORTED)
        assert (dx == SENTINEL).all() and (dg == SENTINEL).all() and (db == SENTINEL).all()
    for key, tol, div, floor_at in H.ln_checks(name):
        cls(f"trunk-train edges LayerNorm {name} {key}", got[key], r32[key], r64[key], tol, div, floor_at)
    if name.startswith("exact_constant_row"):
        assert torch.equal(got["y"][H.LN_CONST_ROW].cpu(), i["beta"]), "a constant row's sums are exact at this width: y == beta"
    if fam == "constant_row":
        assert torch.isfinite(got["dx"]).all()


@pytest.mark.parametrize("dim", [63, 512])
def test_layernorm_backward_of_an_empty_batch(dim):
    lib = ffi.load()
    dg, db = torch.full((dim,), SENTINEL, device=dev()), torch.full((dim,), SENTINEL, device=dev())
    assert lib.afm_layernorm_bwd(None, None, None, None, None, dg.data_ptr(), db.data_ptr(), 0, dim, H.LN_EPS, 0.0, 0, 0, None, 0, st(dg)) == 0
    assert (dg == 0).all() and (db == 0).all()
    assert lib.afm_layernorm_rows(None, None, None, None, 0, dim, H.LN_EPS, 0, 0, 0, st(dg)) == 0


@pytest.mark.parametrize("rows,dim,row_map", H.LN_ROWS_MAPS)
def test_layernorm_rows_writes_the_mapped_rows_only(rows, dim, row_map):
    grp, stride, off = row_map
    total = (rows + grp - 1) // grp * stride + off
    x, gamma, beta = H.g(f"tte_lnr_x_{dim}", (total, dim)), 1 + 0.1 * H.g(f"tte_lnr_g_{dim}", (dim,)), 0.1 * H.g(f"tte_lnr_b_{dim}", (dim,))
    rr = H.mapped_rows(rows, grp, stride, off)
    y = ln_forward(x.to(dev()), gamma.to(dev()), beta.to(dev()), torch.full((total, dim), SENTINEL, device=dev()), rows, row_map).cpu()
    other = torch.ones(total, dtype=torch.bool)
    other[rr] = False
    assert other.any() and (y[other] == SENTINEL).all(), "a row outside the map was written"
    zero = torch.zeros(rows, dim)
    r32, r64 = (H.ln_restatement(x[rr], gamma, beta, zero, dt)["y"] for dt in (F32, F64))
    cls(f"trunk-train edges LayerNorm rows {rows}x{dim} map {row_map}", y[rr], r32, r64, H.LN_TOL, r64.abs().max().item())


@pytest.mark.parametrize("rows,dim", [(37, 256), (37, 260), (37, 512), (37, 1024), (8193, 256)])
def test_layernorm_backward_dropout_output_is_one_float32_multiply(rows, dim):
    """dx_drop == where(keep, dx * inv_keep, 0) bit for bit against oracle/rng_ref.keep_mask; dx itself is what the call without dropout
    gives.  (8193 rows: every block makes a fifth trip of one row - the row index of the mask is the row, not the trip.)"""
    drop = (0.25, 2 ** 63 + 5, 31)
    x, gamma, dy = (H.g(f"tte_lnd_{k}_{rows}_{dim}", s).to(dev()) for k, s in (("x", (rows, dim)), ("g", (dim,)), ("dy", (rows, dim))))
    dx, dxd, dg, db = ln_backward(x, gamma, dy, drop)
    dx0, _, dg0, db0 = ln_backward(x, gamma, dy)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    keep, inv = rng_ref.keep_mask(*drop, rows, dim)
    H.keep_share_ok(torch.from_numpy(keep), drop[0])
    keep = torch.from_numpy(keep).to(dev())
    want = torch.where(keep, dx * float(inv), torch.zeros_like(dx))
    assert torch.equal(dxd, want), f"{int((dxd != want).sum())} elements of dx_drop differ"
    assert (dxd[~keep] == 0).all()


@pytest.mark.parametrize("dim,offset", [(63, False), (512, True)])
def test_layernorm_backward_generic_arm_refuses_dropout(dim, offset):
    put = offset_view if offset else (lambda t: t.to(dev()))
    x, gamma, dy = put(H.g("tte_lng_x", (5, dim))), put(H.g("tte_lng_g", (dim,))), put(H.g("tte_lng_dy", (5, dim)))
    ln_backward(x, gamma, dy, (0.25, 1, 2), put=put, expect=H.AFM_E_UNSUPPORTED)


# ================================================================================================ D. loss, glue, epilogue
@pytest.mark.parametrize("kind", H.MSE_MASKS)
@pytest.mark.parametrize("B,L,D", H.MSE_SHAPES)
def test_masked_mse_forward_backward(B, L, D, kind):
    lib = ffi.load()
    i = H.mse_inputs(B, L, D, kind)
    r32, r64 = H.mse_restatement(i, F32), H.mse_restatement(i, F64)
    t, p, dl = i["target"].to(dev()), i["pred"].to(dev()), i["dloss"].to(dev())
    km = None if i["mask"] is None else i["mask"].to(torch.uint8).to(dev())
    loss, dpred = torch.full((B,), SENTINEL, device=dev()), torch.full((B, L, D), SENTINEL, device=dev())
    assert lib.afm_masked_mse(t.data_ptr(), p.data_ptr(), ffi.ptr(km), loss.data_ptr(), B, L, D, st(t)) == 0
    assert lib.afm_masked_mse_bwd(t.data_ptr(), p.data_ptr(), ffi.ptr(km), dl.data_ptr(), dpred.data_ptr(), B, L, D, st(t)) == 0
    live = torch.ones(B, dtype=torch.bool)
    if kind == "full_sample":                             # NaN forward, as the torch expression; its dpred rows exactly zero
        live[B - 1] = False
        assert torch.isnan(loss[B - 1]) and (dpred[B - 1] == 0).all()
    if i["mask"] is not None:
        assert (dpred.cpu()[i["mask"]] == 0).all(), "a masked frame's gradient is exactly zero"
    if live.any():
        cls(f"trunk-train edges masked mse {B}x{L}x{D} {kind} loss", loss, r32["loss"], r64["loss"], H.MSE_TOL, select=live)
        div = max(r64["dpred"][live].abs().max().item(), 1e-12)
        cls(f"trunk-train edges masked mse {B}x{L}x{D} {kind} dpred", dpred, r32["dpred"], r64["dpred"], H.ELEMENTWISE_TOL, div, select=live)


def test_masked_mse_of_an_empty_batch_returns_zero_from_both_entry_points():
    """The decision: B == 0 is an empty batch, not a bad argument - both entry points return 0 and touch nothing, null pointers included
    (as afm_layernorm_rows and afm_rowop treat rows == 0)."""
    lib = ffi.load()
    assert lib.afm_masked_mse(None, None, None, None, 0, 4, 3, None) == 0
    assert lib.afm_masked_mse_bwd(None, None, None, None, None, 0, 4, 3, None) == 0


@pytest.mark.parametrize("tab,act,drop", H.ROWOP_COMBOS)
def test_rowop_every_combination(tab, act, drop):
    i = H.rowop_inputs(H.ROWOP_ROWS, H.ROWOP_COLS)
    r32, r64 = H.rowop_restatement(i, tab, act, drop, F32), H.rowop_restatement(i, tab, act, drop, F64)
    out = AG._rowop(i["x"].to(dev()), rowtab=i["tab"].to(dev()) if tab else None, z=i["z"].to(dev()) if act else None, act=act,
                    drop=H.ROWOP_DROP if drop else None).cpu()
    cls(f"trunk-train edges rowop tab={tab} act={act} drop={drop}", out, r32, r64, H.ELEMENTWISE_TOL, r64.abs().max().item())
    if not act:
        assert torch.equal(out, r32), "an add and a multiply by inv_keep or 0: exact"
    if drop:
        assert (out[dr.keep_scale(*H.ROWOP_DROP, out.shape) == 0] == 0).all()
    if act == H.ACT_RELU:
        assert (out[i["z"] <= 0] == 0).all()


def test_rowop_second_grid_trip():
    rows, cols = H.ROWOP_BIG
    i = H.rowop_inputs(rows, cols)
    r32, r64 = (H.rowop_restatement(i, True, H.ACT_GELU, True, dt) for dt in (F32, F64))
    out = AG._rowop(i["x"].to(dev()), rowtab=i["tab"].to(dev()), z=i["z"].to(dev()), act=H.ACT_GELU, drop=H.ROWOP_DROP).cpu()
    cls("trunk-train edges rowop second grid trip", out, r32, r64, H.ELEMENTWISE_TOL, r64.abs().max().item())
    assert (out[dr.keep_scale(*H.ROWOP_DROP, out.shape) == 0] == 0).all()


@pytest.mark.parametrize("act", [H.ACT_GELU, H.ACT_SILU, H.ACT_RELU])
def test_activation_derivative_on_the_ladder(act):
    z = torch.tensor([H.ACT_LADDER])
    out = AG._rowop(torch.ones_like(z).to(dev()), z=z.to(dev()), act=act).cpu()
    print(f"[act'] act={act}: {out.flatten().tolist()}")
    assert torch.isfinite(out).all()
    cls(f"trunk-train edges act' act={act} ladder", out, H.act_grad(z, act), H.act_grad(z.double(), act), H.ELEMENTWISE_TOL)
    if act == H.ACT_RELU:
        assert out[0, 0] == 0 and torch.equal(out, (z > 0).float())


@pytest.mark.parametrize("rows,cols", H.TRANSPOSE_SHAPES)
def test_transpose_is_exact(rows, cols):
    w = H.g("tte_tr", (rows, cols))
    assert torch.equal(AG._transpose(w.to(dev())).cpu(), w.t().contiguous())


@pytest.mark.parametrize("variant", H.EPI_VARIANTS)
@pytest.mark.parametrize("M,N,K", sorted(H.EPI_SHAPES))
def test_training_epilogue_of_linear(M, N, K, variant):
    i = H.epi_inputs(M, N, K)
    r32, r64 = H.epi_reference(M, N, K, variant, F32), H.epi_reference(M, N, K, variant, F64)
    A, W, bias, res, z = (i[k].to(dev()) for k in ("A", "W", "bias", "res", "z"))
    out, got = torch.empty(M, N, device=dev()), {}
    keep = dr.keep_scale(*H.EPI_DROP, (M, N))
    if variant == "preact":
        got["preact"] = torch.empty(M, N, device=dev())
        AG._gemm(A, W, out, M, N, K, bias=bias, act=ffi.ACT_GELU, preact=got["preact"])
    elif variant == "dact":
        AG._gemm(A, W, out, M, N, K, dact=ffi.ACT_GELU, dact_z=z)
    elif variant in ("drop_before", "drop_after"):
        AG._gemm(A, W, out, M, N, K, residual=res, drop=H.EPI_DROP, drop_after=int(variant == "drop_after"))
    elif variant == "act_drop":
        AG._gemm(A, W, out, M, N, K, bias=bias, act=ffi.ACT_GELU, drop=H.EPI_DROP)
    elif variant == "drop_dact":                          # as the encoder backward launches it
        AG._gemm(A, W, out, M, N, K, drop=H.EPI_DROP, dact=ffi.ACT_GELU, dact_z=z)
    else:
        out = torch.zeros(r64["out"].shape, device=dev())
        AG._gemm(A, W, out, M, N, K, c_map=H.EPI_SHAPES[M, N, K][1])
        other = torch.ones(out.shape[0], dtype=torch.bool)
        other[H.mapped_rows(M, *H.EPI_SHAPES[M, N, K][1])] = False
        assert other.any() and (out.cpu()[other] == 0).all(), "an unmapped row was written"
    got["out"] = out
    for key in r64:
        cls(f"trunk-train edges epilogue {M}x{N}x{K} {variant} {key}", got[key], r32[key], r64[key], H.GEMM_TOL, r64[key].abs().max().item())
    o = out.cpu()
    if variant in ("drop_after", "act_drop", "drop_dact"):
        assert (o[keep == 0] == 0).all(), "a dropped element is exactly zero"
    if variant == "drop_before":
        assert torch.equal(o[keep == 0], i["res"][keep == 0]), "a dropped element is exactly its residual"


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (committed as profiles/trunk_train_edges_parity.json)."""
    write_parity_table()
