"""`-m gpu`: the 128 x 128 bf16-split tile on 512 threads (AFM_TUNE_TILE code 14: 4 x 2 waves, a 32 x 64 tile per wave) against the
256-thread 128 x 128 tile (code 5) and the 64 x 64 tile (code 3).  Same tile program, same products in the same order, same K-segment sums:
every output bit must agree, for ragged row counts, every K the sampling loop runs (272: the motion adapter; 512; 1024: linear2) and every
epilogue the loop uses - plain, residual + row statistics, folded LayerNorm of A, fused LayerNorm output, the DDPM update, the aux rider."""
import ctypes as C
import math

import pytest
import torch

from afm import ffi, ops, synth
from gpu_util import dev

pytestmark = pytest.mark.gpu

TILES = (14, 5, 3)


def _per_tile(products, fn):
    """fn() once per tile code, with the bf16-split arithmetic of `products`; -> list of results in TILES order."""
    saved, saved_tune = ops.get_gemm_split(), ops.set_gemm_tune(0)
    try:
        ops.set_gemm_split(products, 0)
        outs = []
        for tile in TILES:
            ops.set_gemm_tune(tile << ffi.TUNE_TILE_SHIFT)
            outs.append(fn())
        return outs
    finally:
        ops.set_gemm_split(*saved)
        ops.set_gemm_tune(saved_tune)


def _assert_same(outs, what):
    for tile, o in zip(TILES[1:], outs[1:]):
        for a, b in zip(outs[0], o):
            assert torch.isfinite(a).all(), f"{what}: tile 14 produced non-finite values"
            assert torch.equal(a, b), f"{what}: tile 14 differs from tile {tile}, max diff {(a - b).abs().max().item():.3e}"


def _g(name, *shape):
    return synth.gaussian(f"w8_{name}", shape).to(dev())


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("M,N,K", [(5216, 1536, 512), (777, 512, 512), (3136, 512, 272), (1304, 512, 1024), (5000, 1024, 512), (129, 256, 1024)])
def test_w8_plain_and_residual_statistics(products, M, N, K):
    x, w, b, r = _g("x", M, K), _g("w", N, K) / math.sqrt(K), _g("b", N), _g("r", M, N)

    def run():
        plain = ops.linear(x, w, b, act=ffi.ACT_GELU)
        st = torch.full((M, N // 64, 2), float("nan"), device=dev())
        res = ops.linear(x, w, b, residual=r, stat_out=st)
        return plain, res, st
    _assert_same(_per_tile(products, run), f"plain / residual+stat_out x{products} {M}x{N}x{K}")


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("M,N,K", [(5216, 1024, 512), (1001, 1536, 512), (2608, 512, 1024)])
def test_w8_folded_layernorm_of_a(products, M, N, K):
    """linear1 / in_proj of the loop: raw A rows, (mean, M2) per row and 64-column group, gamma folded into W; linear2 with res_stat."""
    x, w, b, fold = _g("fx", M, K) * 1.5 + 0.3, _g("fw", N, K) / math.sqrt(K), _g("fb", N), _g("fg", N)
    grp = x.view(M, K // 64, 64)
    st = torch.stack([grp.mean(-1), ((grp - grp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).contiguous()
    r = _g("fr", M, N)
    rgrp = r.view(M, N // 64, 64)
    rst = torch.stack([rgrp.mean(-1), ((rgrp - rgrp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).contiguous()
    rg, rb = _g("frg", N) * 0.2 + 1.0, _g("frb", N) * 0.1

    def run():
        h = ops.linear(x, w, b, act=ffi.ACT_GELU, a_stat=(st, fold))
        st2 = torch.full((M, N // 64, 2), float("nan"), device=dev())
        t = ops.linear(x, w, b, residual=r, res_stat=(rst, rg, rb), stat_out=st2)
        return h, t, st2
    _assert_same(_per_tile(products, run), f"folded LayerNorm x{products} {M}x{N}x{K}")


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("M,N,K", [(5216, 512, 512), (1303, 512, 1024), (300, 256, 272)])
def test_w8_fused_layernorm_output(products, M, N, K):
    x, w, b, r = _g("lx", M, K), _g("lw", N, K) / math.sqrt(K), _g("lb", N), _g("lr", M, N)
    gm, be = _g("lg", N) * 0.2 + 1.0, _g("lbe", N) * 0.1

    def run():
        ln_out = torch.full((M, N), float("nan"), device=dev())
        cnt = torch.zeros((M + 31) // 32, dtype=torch.int32, device=dev())
        c = ops.linear(x, w, b, residual=r, ln=(gm, be, 1e-5), ln_out=ln_out, ln_counters=cnt)
        assert int(cnt.abs().sum()) == 0                    # every launch leaves its tickets at zero
        return c, ln_out
    _assert_same(_per_tile(products, run), f"fused LayerNorm x{products} {M}x{N}x{K}")


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("B,L,N,K", [(5, 196, 263, 512), (16, 196, 512, 512), (3, 131, 640, 1024)])
def test_w8_ddpm_epilogue(products, B, L, N, K):
    """The output layer's fused DDPM update (scalar epilogue branch, x_next = (c1 * pred + c2 * x_t) + sigma * noise, clip, K-padded copy)."""
    M = B * L
    x, w, b = _g("dx", M, K), _g("dw", N, K) / math.sqrt(K), _g("db", N)
    xt, nz = _g("dxt", M, N), _g("dnz", M, N)
    c1, c2, sg = _g("dc1", B) * 0.1 + 0.5, _g("dc2", B) * 0.1 + 0.9, _g("dsg", B).abs() * 0.1
    ldx2 = N + 9
    lib = ffi.load()

    def run():
        out = torch.full((M, N), float("nan"), device=dev())
        xn = torch.full((M, N), float("nan"), device=dev())
        xn2 = torch.zeros((M, ldx2), device=dev())
        a, c, keep = ops.linear(x, w, b, out=out, defer=True)
        a.ddpm_xt, a.ddpm_noise, a.ddpm_out, a.ldx = xt.data_ptr(), nz.data_ptr(), xn.data_ptr(), N
        a.ddpm_c1, a.ddpm_c2, a.ddpm_sigma, a.rows_per_sample = c1.data_ptr(), c2.data_ptr(), sg.data_ptr(), L
        a.ddpm_clip = 1
        a.ddpm_out2, a.ldx2 = xn2.data_ptr(), ldx2
        ffi.check(lib.afm_linear(C.byref(a), ffi.stream_of(x)), "afm_linear")
        torch.cuda.synchronize()
        return c, xn, xn2
    _assert_same(_per_tile(products, run), f"DDPM epilogue x{products} B={B} L={L} N={N} K={K}")


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("B,L,K", [(16, 196, 272), (7, 60, 512)])
def test_w8_aux_rider(products, B, L, K):
    """The motion adapter's rider: the first aux_rows workgroups copy one time-token row each (table row of t[r] + positional row 0)."""
    d, T, n_t = 512, L + 2, 1000
    M = B * L
    x, w, b = _g("ax", M, K), _g("aw", d, K) / math.sqrt(K), _g("ab", d)
    table, pos = _g("atab", n_t, d), _g("apos", d)
    t = torch.tensor([(37 * i + 11) % n_t for i in range(B)], dtype=torch.int64, device=dev())
    t[0] = n_t + 5                                          # clamped to the last row
    lib = ffi.load()
    assert B <= ((M + 127) // 128) * ((d + 127) // 128)

    def run():
        seq = torch.zeros((B * T, d), device=dev())
        a, c, keep = ops.linear(x, w, b, out=seq, rows=M, c_map=(L, T, 2), defer=True)
        a.aux_src, a.aux_idx, a.aux_add, a.aux_dst = table.data_ptr(), t.data_ptr(), pos.data_ptr(), seq.data_ptr()
        a.aux_dst_ld, a.aux_rows, a.aux_cols, a.aux_idx_max = T * d, B, d, n_t
        ffi.check(lib.afm_linear(C.byref(a), ffi.stream_of(x)), "afm_linear")
        torch.cuda.synchronize()
        return (seq,)
    outs = _per_tile(products, run)
    _assert_same(outs, f"aux rider x{products} B={B} L={L} K={K}")
    seq = outs[0][0].view(B, T, d)
    want = table[t.clamp(0, n_t - 1)] + pos
    assert torch.equal(seq[:, 0], want)
    assert float(seq[:, 1].abs().sum()) == 0.0              # the row between the time token and the mapped rows is untouched


def test_w8_row_mapped_a():
    """A rows gathered through a row map (the 32-bit offsets of code 14 go through the same map)."""
    M, N, K, L, T = 2000, 512, 512, 100, 103
    x, w = _g("mx", (M // L) * T, K), _g("mw", N, K) / math.sqrt(K)

    def run():
        return (ops.linear(x, w, None, rows=M, a_map=(L, T, 3)),)
    _assert_same(_per_tile(6, run), "row-mapped A")


@pytest.mark.parametrize("products", [0, 1])
def test_w8_code_on_other_arithmetics(products):
    """Code 14 on the arithmetics other than six / nine products: the native f32 kernels (products 0) run their one 128 x 128 form, the
    one-product kernels the 512-thread tile; both bit-identical to code 5."""
    M, N, K = 3000, 512, 512
    x, w, b, r = _g("ox", M, K), _g("ow", N, K) / math.sqrt(K), _g("ob", N), _g("or", M, N)
    saved, saved_tune = ops.get_gemm_split(), ops.set_gemm_tune(0)
    try:
        ops.set_gemm_split(products, 0)
        outs = []
        for tile in (14, 5):
            ops.set_gemm_tune(tile << ffi.TUNE_TILE_SHIFT)
            outs.append(ops.linear(x, w, b, act=ffi.ACT_GELU, residual=r))
    finally:
        ops.set_gemm_split(*saved)
        ops.set_gemm_tune(saved_tune)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("products,min_n", [(0, 0), (9, 0), (9, 1024), (6, 1024), (6, 0), (1, 0)])
def test_w8_sampling_loop_every_arithmetic(products, min_n):
    """The two-stream sampling loop at B = 32 (sub-batches of 16 x 326 rows: the loop forces code 14 on its wide GEMMs) with every arithmetic
    setting the benchmark reports: it runs, and every bit equals the same loop forced to code 5."""
    from afm.base import create_model_and_diffusion
    from afm.config import load_config
    cfg = load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263", "diffusion.steps=1000",
                                                                    "diffusion.timestep_respacing='3'"])
    model, diff = create_model_and_diffusion(cfg, device=dev())
    synth.fill_module_(model)
    model = model.to(dev()).eval()
    B, L = 32, 196
    x_T = synth.gaussian("w8_loop_xT", (B, L, 263)).to(dev())
    kw = dict(c_text_feat=synth.text_feature(B).to(dev()), c_cont_emb=synth.gaussian("w8_loop_cont", (B, 128, 256)).to(dev()),
              x_mask=synth.frame_mask(B, L, min_len=8).to(dev()))
    saved = ops.get_gemm_split()
    outs = []
    try:
        ops.set_gemm_split(products, min_n)
        for tile in (0, 5):                                  # 0: the loop's own choice (code 14 here)
            model.gemm_tile = tile
            outs.append(diff.p_sample_loop(model, (B, L, 263), noise=x_T, clip_denoised=False, model_kwargs=kw, seed=5))
    finally:
        ops.set_gemm_split(*saved)
        model.gemm_tile = 0
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), f"x{products} min_n {min_n}: loop with code 14 differs from code 5"
