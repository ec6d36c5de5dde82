"""The CDM's folded-weight tables (afm.fold), identity by identity, on the host in float64: the left side of every check is computed
from a ContactPerceiver's own parameters layer by layer, the right side from the tables alone, on random rows
inp = [x_t | features | 1 | 0 ...], random positive attention weights and random attention outputs `a`.

Every parameter is random (LayerNorm weights and biases included: the default 1 / 0 would hide half the terms).  Shapes: the input
widths at which the row-less kernels' padding changes (feat_dim + 1 = 10, 12 -> K = 12; 13, 44 -> K = 44; 46 -> no row-less tables),
contact_dim 1 and 8, 1 and 4 self-attention layers, and a model the fold does not apply to.  Bound: 1e-9 of the largest reference
value - float64 sums of at most 64^2 products of O(1) values err below ~5e-13; the margin is for the cancellation in the variances."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from afm import ffi, fold
from afm.cdm import ContactPerceiver

D, HEADS, N = 64, 8, 5          # dq = dkv, heads of both attentions, points per check
FOLD = {"fold_xu", "fold_xv", "fold_w2", "fold_q", "fold_c0"}
ROW_LESS = {"gen_qe", "enc_ec", "enc_qee", "enc_wove", "enc_c1", "dec_c", "dec_twx", "dec_qxx", "dec_qdd", "dec_dwq", "dec_wqb", "dec_wco",
            "dec_wow", "dec_wog", "dec_xwo"}
# (contact_dim, point_feat_dim, n_self, K): feat_dim + 1 = contact_dim + point_feat_dim + 3 + 1 inputs, padded to K by the row-less kernels
LEVEL2 = {"K12_padded": (6, 0, 2, 12), "K12_full": (8, 0, 1, 12), "K44_first": (1, 8, 4, 44), "K44_full": (6, 34, 1, 44),
          "K12_one_contact": (1, 5, 1, 12)}
LEVEL1 = (8, 34, 4, None)       # feat_dim + 1 = 46


def _model(contact_dim, point_feat_dim, n_self, pos=True, seed=0):
    cfg = SimpleNamespace(encoder_widening_factor=1, decoder_widening_factor=1, point_pos_emb=pos, encoder_q_input_channels=D,
                          encoder_kv_input_channels=D, decoder_q_input_channels=D, decoder_kv_input_channels=D, encoder_num_heads=HEADS,
                          decoder_num_heads=HEADS, encoder_self_attn_num_layers=n_self)
    cm = ContactPerceiver(cfg, contact_dim=contact_dim, point_feat_dim=point_feat_dim, text_feat_dim=16, time_emb_dim=16).double()
    cl = torch.nn.Linear(D, contact_dim).double()
    g = torch.Generator().manual_seed(1000 * seed + 100 * contact_dim + point_feat_dim)
    with torch.no_grad():
        for m in list(cm.modules()) + [cl]:
            for name, p in m.named_parameters(recurse=False):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.5 if p.dim() == 1 else 0.3))
                if isinstance(m, torch.nn.LayerNorm) and name == "weight":
                    p.add_(1.7)
    return cm, cl, g


class Case:
    """A model, its tables and random inputs."""

    def __init__(self, contact_dim, point_feat_dim, n_self, K):
        self.cd, self.K = contact_dim, K
        self.cm, self.cl, g = _model(contact_dim, point_feat_dim, n_self)
        self.t = fold.cdm_tables(self.cm, self.cl, contact_dim)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        self.row = rnd(N, self.cm.feat_dim)
        self.a, self.h, self.q0 = rnd(N, D), rnd(N, D), rnd(D)
        self.p = torch.rand(HEADS, N, generator=g, dtype=torch.float64) + 0.05
        self.p /= self.p.sum(1, keepdim=True)
        if K is not None:
            self.inp = torch.zeros(N, self.K, dtype=torch.float64)
            self.inp[:, :self.cm.feat_dim], self.inp[:, self.cm.feat_dim] = self.row, 1.0
        self.enc_kv = self.cm.encoder_adapter(self.row)
        self.dec_q = self.cm.decoder_adapter(self.enc_kv)
        self.dec_attn = self.cm.decoder_cross_attn[0].module
        self.dec_mlp = self.cm.decoder_cross_attn[1].module
        self.y = self.dec_q + self.dec_attn.attention.o_proj(self.a)


@pytest.fixture(scope="module", params=sorted(LEVEL2))
def case(request):
    with torch.no_grad():
        return Case(*LEVEL2[request.param])


def close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    bound = 1e-9 * want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= bound, f"max|diff| = {err:.3e} > {bound:.3e}"


def stats(x, norm):
    """mean, biased variance and rstd of the rows, as LayerNorm takes them"""
    var = x.var(1, unbiased=False)
    return x.mean(1), var, (var + norm.eps).rsqrt()


def from_operand_order(o, K):
    """inverse of fold.operand_order: column 16 t + i of the table holds row 4 (4 t + (i & 3)) + (i >> 2) of the matrix"""
    assert o.shape == (K, 16 * ((K + 15) // 16))
    q = torch.zeros(K, K, dtype=torch.float64)
    for c in range(o.shape[1]):
        t, i = divmod(c, 16)
        src = 4 * (4 * t + (i & 3)) + (i >> 2)
        if src < K:
            q[src] = o[:, c]
        else:
            assert not o[:, c].any(), "columns past the K-th row are zero"
    return q


def quad(x, q, y=None):
    return torch.einsum("nk,kl,nl->n", x, q, x if y is None else y)


# ---------------------------------------------------------------------------------------------------------------- levels and keys
def test_fold_level_conditions():
    assert fold.cdm_fold_level(6, 9, 256) == 2 and fold.cdm_fold_level(8, 43, 64) == 2
    assert fold.cdm_fold_level(6, 44, 256) == 1                                  # feat_dim + 1 = 45 > 44
    assert fold.cdm_fold_level(9, 12, 256) == 0 and fold.cdm_fold_level(6, 6, 256) == 0 and fold.cdm_fold_level(6, 9, 96) == 0


def test_keys_are_the_pack_fields(case):
    assert set(case.t) == FOLD | ROW_LESS | {"lat_fold"}
    fields = {n for n, _ in ffi.CdmWeights._fields_}
    assert set(case.t) <= fields
    assert case.t["enc_ec"].shape == (case.K, D) and case.t["dec_twx"].shape == (case.K, D) and case.t["gen_qe"].shape == (case.cd, case.K)
    assert all(t.dtype == torch.float64 and t.device.type == "cpu" for k, t in case.t.items() if k != "lat_fold")


@torch.no_grad()
def test_level_one_has_the_folded_form_only():
    c = Case(*LEVEL1)
    assert c.cm.feat_dim + 1 == 46 and set(c.t) == FOLD | {"lat_fold"}
    check_fold_tables(c)
    check_lat_fold(c)


def test_level_zero_is_empty():
    cm, cl, _ = _model(6, 0, 2, pos=False)
    assert cm.feat_dim == 6 and fold.cdm_tables(cm, cl, 6) == {}


# ---------------------------------------------------------------------------------------------------------------- ln_fold, operand order
def test_ln_fold_identity():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    w, b, gamma, beta, x = rnd(7, 13), rnd(7), 1.7 + 0.5 * rnd(13), rnd(13), rnd(4, 13)
    wg, gs, c = fold.ln_fold(w, b, gamma, beta)
    mean, _, rstd = stats(x, SimpleNamespace(eps=1e-5))
    close(rstd[:, None] * (x @ wg.t() - mean[:, None] * gs[None, :]) + c, F.linear(F.layer_norm(x, (13,), gamma, beta, 1e-5), w, b))


@pytest.mark.parametrize("K", [12, 44])
def test_operand_order_round_trip(K):
    q = torch.arange(K * K, dtype=torch.float64).reshape(K, K) + 1
    o = fold.operand_order(q, K)
    assert torch.equal(from_operand_order(o, K), q)
    assert o[3, 6] == q[4 * 2 + 1, 3]                                            # t = 0, i = 6 -> row 4 (i & 3) + (i >> 2) = 9, as the header spells it


# ---------------------------------------------------------------------------------------------------------------- the table groups
def check_fold_tables(c):
    cm, t, cd = c.cm, c.t, c.cd
    we, wd = cm.encoder_adapter.weight, cm.decoder_adapter.weight
    close(t["fold_xu"], we[:, :cd].t())
    close(t["fold_xv"], (wd @ we[:, :cd]).t())
    x_t, rest = c.row[:, :cd], c.row.clone()
    rest[:, :cd] = 0
    C0 = cm.encoder_adapter(rest)
    D0 = cm.decoder_adapter(C0)
    close(C0 + x_t @ t["fold_xu"], c.enc_kv)
    close(D0 + x_t @ t["fold_xv"], c.dec_q)
    o_w = c.dec_attn.attention.o_proj.weight
    want = c.cl(c.dec_mlp[3](c.h) + c.y)
    close(c.h @ t["fold_w2"].t() + x_t @ t["fold_q"].t() + (D0 + c.a @ o_w.t()) @ c.cl.weight.t() + t["fold_c0"], want)


def check_lat_fold(c):
    cm, slots = c.cm, c.t["lat_fold"]
    want = {0: (cm.encoder_cross_attn[1].module[1], cm.encoder_cross_attn[1].module[0]),
            17: (c.dec_attn.attention.k_proj, c.dec_attn.kv_norm), 18: (c.dec_attn.attention.v_proj, c.dec_attn.kv_norm)}
    for l, layer in enumerate(cm.encoder_self_attn):
        sa, mlp = layer[0].module, layer[1].module
        want.update({1 + 4 * l: (sa.attention.q_proj, sa.norm), 2 + 4 * l: (sa.attention.k_proj, sa.norm),
                     3 + 4 * l: (sa.attention.v_proj, sa.norm), 4 + 4 * l: (mlp[1], mlp[0])})
    assert len(slots) == 19 and {s for s, trip in enumerate(slots) if trip is not None} == set(want)
    x = c.h + 0.3                                                                # rows with a mean
    for s, (lin, norm) in want.items():
        wg, g, cc = slots[s]
        mean, _, rstd = stats(x, norm)
        close(rstd[:, None] * (x @ wg.t() - mean[:, None] * g[None, :]) + cc, lin(norm(x)))


@torch.no_grad()
def test_fold_tables(case):
    check_fold_tables(case)


@torch.no_grad()
def test_lat_fold_slots(case):
    check_lat_fold(case)


@torch.no_grad()
def test_encoder_rows_and_their_variance(case):
    c = case
    close(c.inp @ c.t["enc_ec"], c.enc_kv - c.enc_kv.mean(1, keepdim=True))
    close(quad(c.inp, from_operand_order(c.t["enc_qee"], c.K)), c.enc_kv.var(1, unbiased=False))


@torch.no_grad()
def test_head_of_the_latent_chain(case):
    c = case
    ea = c.cm.encoder_cross_attn[0].module
    v = ea.attention.v_proj(ea.kv_norm(c.enc_kv))                                # [N, dq]
    hd = D // HEADS
    attn = torch.cat([c.p[h] @ v[:, h * hd:(h + 1) * hd] for h in range(HEADS)])
    want = c.q0 + ea.attention.o_proj(attn)
    _, _, rstd = stats(c.enc_kv, ea.kv_norm)
    s = (c.p * rstd[None, :]) @ c.inp                                            # [heads, K]
    assert c.t["enc_wove"].shape == (HEADS * c.K, D)
    close(c.q0 + sum(s[h] @ c.t["enc_wove"][c.K * h:c.K * h + c.K] for h in range(HEADS)) + c.t["enc_c1"], want)


@torch.no_grad()
def test_generator_and_query_variance(case):
    c = case
    close(c.inp @ c.t["gen_qe"].t(), c.dec_q @ c.cl.weight.t())
    close(quad(c.inp, from_operand_order(c.t["dec_qdd"], c.K)), c.dec_q.var(1, unbiased=False))


@torch.no_grad()
def test_decoder_query_projection(case):
    c = case
    _, _, rstd = stats(c.dec_q, c.dec_attn.q_norm)
    close(rstd[:, None] * (c.inp @ c.t["dec_dwq"]) + c.t["dec_wqb"], c.dec_attn.attention.q_proj(c.dec_attn.q_norm(c.dec_q)))


@torch.no_grad()
def test_decoder_mlp_input(case):
    c, t = case, case.t
    _, var, rstd = stats(c.y, c.dec_mlp[0])
    close(rstd[:, None] * (c.inp @ t["dec_twx"] + c.a @ t["dec_wow"]) + t["dec_c"], c.dec_mlp[1](c.dec_mlp[0](c.y)))
    close(quad(c.inp, t["dec_qxx"]) + 2 * quad(c.inp, t["dec_xwo"], c.a) + quad(c.a, t["dec_wog"]), var)


@torch.no_grad()
def test_output_rows_of_the_attention_values(case):
    c = case
    wco = c.t["dec_wco"]
    assert wco.shape == (8, D) and not wco[c.cd:].any()
    close(wco[:c.cd], c.cl.weight @ c.dec_attn.attention.o_proj.weight)
