"""Folded-weight tables of the sampling forms: the definition of `afm_cdm_weights.fold_*`, `gen_qe`, `enc_*`, `dec_*` and `lat_fold`
(include/afm_hip.h), and the LayerNorm fold the CMDM's pack uses as well.

Pure host algebra: parameters in, float64 CPU tensors out - products in float64, rounded to float32 once by the caller that uploads
them.  Nothing here touches the GPU or another module of the package, so tests/test_cdm_fold_host.py pins every table to the identity
it is documented with.  Names as in the header: G_enc / G_dec are the two adapters as maps of the K inputs [x_t | features | 1 | 0 ...]
of a point, Xc the centred rows of G_dec with the decoder attention's output bias on the constant's row, Woc = dec_attn.o.w minus its
column means."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch


def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().double()


def _centred(rows: torch.Tensor) -> torch.Tensor:
    return rows - rows.mean(1, keepdim=True)


def ln_fold(weight, bias, gamma, beta) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """linear(LayerNorm(x)) = rstd (wg x - mean g) + c  with  wg = weight * gamma, g = row sums of wg, c = bias + weight beta."""
    w, gamma = _f64(weight), _f64(gamma)
    wg = w * gamma[None, :]
    return wg, wg.sum(1), _f64(bias) + w @ _f64(beta)


def operand_order(q: torch.Tensor, K: int) -> torch.Tensor:
    """[K, K] -> [K, 16 NT], NT = ceil(K / 16), the order the MFMA reads a quadratic form's matrix in:
    entry (k, 16 t + i) = q[4 (4 t + (i & 3)) + (i >> 2)][k], 0 where that index is >= K."""
    c = torch.arange(16 * ((K + 15) // 16))
    t, i = c // 16, c % 16
    src = 4 * (4 * t + (i & 3)) + (i >> 2)
    o = torch.zeros(K, c.numel(), dtype=torch.float64)
    o[:, src < K] = q[src[src < K], :].t()
    return o


def cdm_fold_level(contact_dim: int, feat_dim: int, dkv: int) -> int:
    """Which tables the CDM's shapes allow: 0 none, 1 the folded form (fold_*) and lat_fold, 2 the row-less form's tables as well."""
    if not (contact_dim <= 8 and feat_dim > contact_dim and dkv % 64 == 0):
        return 0
    return 2 if feat_dim + 1 <= 44 else 1


def _fold_tables(cm, contact_layer, cd: int) -> Dict[str, torch.Tensor]:
    """enc_kv = C + x_t fold_xu and dec_q = D + x_t fold_xv with C = encoder_adapter(row with x_t = 0), D = decoder_adapter(C) - only the
    contact columns of a row change between steps - and
    contact_layer(fc2(h) + dec_q + o_proj(a)) = fold_w2 h + fold_q x_t + contact_layer.w (D + o_proj.w a) + fold_c0."""
    we, wd, wc = _f64(cm.encoder_adapter.weight), _f64(cm.decoder_adapter.weight), _f64(contact_layer.weight)
    fc2, bo = cm.decoder_cross_attn[1].module[3], _f64(cm.decoder_cross_attn[0].module.attention.o_proj.bias)
    xv = (wd @ we[:, :cd]).t().contiguous()
    return dict(fold_xu=we[:, :cd].t().contiguous(), fold_xv=xv, fold_w2=wc @ _f64(fc2.weight), fold_q=wc @ xv.t(),
                fold_c0=wc @ (_f64(fc2.bias) + bo) + _f64(contact_layer.bias))


def _input_maps(cm, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """inp G_enc = encoder_adapter(row), inp G_dec = decoder_adapter(encoder_adapter(row)) for inp = [row | 1 | 0 ...] of width K."""
    we, wd, be, bd = (_f64(t) for t in (cm.encoder_adapter.weight, cm.decoder_adapter.weight, cm.encoder_adapter.bias, cm.decoder_adapter.bias))
    F = cm.feat_dim
    g_enc, g_dec = torch.zeros(K, cm.dkv, dtype=torch.float64), torch.zeros(K, cm.dkv, dtype=torch.float64)
    g_enc[:F], g_enc[F] = we.t(), be
    g_dec[:F], g_dec[F] = (wd @ we).t(), wd @ be + bd
    return g_enc, g_dec


def _generator_tables(contact_layer, g_dec) -> Dict[str, torch.Tensor]:
    """gen_qe inp = contact_layer.w decoder_adapter(encoder_adapter(row)) (no contact_layer bias)."""
    return dict(gen_qe=_f64(contact_layer.weight) @ g_dec.t())


def _encoder_tables(cm, g_enc, K: int) -> Dict[str, torch.Tensor]:
    """inp enc_ec = the centred encoder_adapter row e, inp Qe inp^T = var(e) (enc_qee: Qe in operand order), and with
    s_h = sum_n p_hn rstd_n inp_n:  sum_h s_h enc_wove[K h : K h + K] + enc_c1 = o_proj(attention output over v_proj(LayerNorm_kv(e)))."""
    ea = cm.encoder_cross_attn[0].module
    gk, bk = _f64(ea.kv_norm.weight), _f64(ea.kv_norm.bias)
    wv, bv, wo, bo = (_f64(t) for t in (ea.attention.v_proj.weight, ea.attention.v_proj.bias, ea.attention.o_proj.weight, ea.attention.o_proj.bias))
    ec = _centred(g_enc)
    wve = (ec * gk[None, :]) @ wv.t()                   # [K, dq]: v_proj.w (gamma * Ec[k])
    hd = cm.dq // 8                                     # 8 encoder heads: what enc_point_kernel accumulates and every reference config has
    wove = torch.zeros(8 * K, cm.dq, dtype=torch.float64)
    for h in range(8):
        blk = slice(h * hd, (h + 1) * hd)
        wove[K * h:K * h + K] = wve[:, blk] @ wo[:, blk].t()
    return dict(enc_ec=ec, enc_qee=operand_order(ec @ ec.t() / cm.dkv, K), enc_wove=wove, enc_c1=bo + wo @ (wv @ bk + bv))


def _mlp_rows(cm, g_dec) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Xc, fc1.w * norm.w) of the decoder MLP: Xc = centred rows of G_dec with dec_attn.o.b added on the constant's row."""
    mlp = cm.decoder_cross_attn[1].module
    tx = g_dec.clone()
    tx[cm.feat_dim] += _f64(cm.decoder_cross_attn[0].module.attention.o_proj.bias)
    return _centred(tx), _f64(mlp[1].weight) * _f64(mlp[0].weight)[None, :]


def _decoder_input_tables(cm, g_dec, K: int) -> Dict[str, torch.Tensor]:
    """With y = dec_q + o_proj(a): fc1(LayerNorm_mlp(y)) = rstd_y (inp dec_twx + a dec_wow) + dec_c, the inp-only part of var(y) is
    inp dec_qxx inp^T, and var(dec_q) = inp Qd inp^T (dec_qdd: Qd in operand order)."""
    mlp = cm.decoder_cross_attn[1].module
    xc, w1g = _mlp_rows(cm, g_dec)
    dc = _centred(g_dec)
    return dict(dec_c=_f64(mlp[1].bias) + _f64(mlp[1].weight) @ _f64(mlp[0].bias), dec_twx=xc @ w1g.t(), dec_qxx=xc @ xc.t() / cm.dkv,
                dec_qdd=operand_order(dc @ dc.t() / cm.dkv, K))


def _decoder_latent_tables(cm, contact_layer, g_dec, cd: int) -> Dict[str, torch.Tensor]:
    """q_proj(LayerNorm_q(dec_q)) = rstd (inp dec_dwq) + dec_wqb;  var(y) = inp dec_qxx inp^T + 2 inp dec_xwo a^T + a dec_wog a^T;
    dec_wco = contact_layer.w dec_attn.o.w in its first contact_dim rows, zero below (dec_wow: see the input side)."""
    da = cm.decoder_cross_attn[0].module
    gq, bq_n = _f64(da.q_norm.weight), _f64(da.q_norm.bias)
    wq, bq, wo = _f64(da.attention.q_proj.weight), _f64(da.attention.q_proj.bias), _f64(da.attention.o_proj.weight)
    xc, w1g = _mlp_rows(cm, g_dec)
    woc = wo - wo.mean(0, keepdim=True)
    wco = torch.zeros(8, cm.dkv, dtype=torch.float64)
    wco[:cd] = _f64(contact_layer.weight) @ wo
    return dict(dec_dwq=(_centred(g_dec) * gq[None, :]) @ wq.t(), dec_wqb=wq @ bq_n + bq, dec_wco=wco, dec_wow=woc.t() @ w1g.t(),
                dec_wog=woc.t() @ woc / cm.dkv, dec_xwo=xc @ woc / cm.dkv)


def _lat_fold(cm) -> List[Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]]:
    """19 slots of ln_fold triples: 0 enc_mlp.fc1; 1 + 4 l .. 3 + 4 l the q / k / v projections of self-attention layer l, 4 + 4 l its
    MLP's fc1; 17 / 18 dec_attn.k / dec_attn.v (dec_kv_norm).  None where the model has no such layer."""
    slots: List[Optional[tuple]] = [None] * 19

    def put(slot, lin, norm):
        slots[slot] = ln_fold(lin.weight, lin.bias, norm.weight, norm.bias)
    put(0, cm.encoder_cross_attn[1].module[1], cm.encoder_cross_attn[1].module[0])
    for l, layer in enumerate(cm.encoder_self_attn):
        sa, mlp = layer[0].module, layer[1].module
        put(1 + 4 * l, sa.attention.q_proj, sa.norm); put(2 + 4 * l, sa.attention.k_proj, sa.norm)
        put(3 + 4 * l, sa.attention.v_proj, sa.norm); put(4 + 4 * l, mlp[1], mlp[0])
    da = cm.decoder_cross_attn[0].module
    put(17, da.attention.k_proj, da.kv_norm); put(18, da.attention.v_proj, da.kv_norm)
    return slots


def cdm_tables(contact_model, contact_layer, contact_dim: int) -> dict:
    """Every table of `afm_cdm_weights` that `cdm_fold_level` allows, by field name, in the header's order ("lat_fold": the 19 slots)."""
    cm = contact_model
    level = cdm_fold_level(contact_dim, cm.feat_dim, cm.dkv)
    if level == 0:
        return {}
    tables = _fold_tables(cm, contact_layer, contact_dim)
    if level == 2:
        K = 12 if cm.feat_dim + 1 <= 12 else 44          # inputs of the row-less kernels, padded (RowLess<3> / RowLess<11> in perceiver.hip)
        g_enc, g_dec = _input_maps(cm, K)
        tables.update(_generator_tables(contact_layer, g_dec))
        tables.update(_encoder_tables(cm, g_enc, K))
        tables.update(_decoder_input_tables(cm, g_dec, K))
        tables.update(_decoder_latent_tables(cm, contact_layer, g_dec, contact_dim))
    tables["lat_fold"] = _lat_fold(cm)
    return tables
