"""`-m gpu`: the streamed epilogue of the 512-thread 128 x 128 bf16-split tile (AFM_TUNE_TILE code 14: every global load of the tile's
epilogue issued before its first store, eight unrolled trips) against the same tile program with the shared epilogue (code 15) and the
64 x 64 tile (code 3).  The three run the same products in the same order and the same epilogue expressions: outputs and statistics must be
equal, for every input combination the streamed form serves, on ragged rows at the trip granularity of 16 (M = 129: seven of the second
row tile's eight trips run wholly on clamped rows), ragged column tiles (N = 64, 192), row maps with a hole, and for the inputs it declines
(scale, preact: the fall-back to the shared epilogue).  Buffers are pre-filled with NaN and carry guard rows behind the last mapped row:
a clamped prefetch address must never turn into a store.

Tile 14 is also compared with a float64 host evaluation, with the bound of test_linear_split_bf16_mode: e = max |got - f64| / scale
<= max(1.5 e_f32, 3e-7), scale = the sum of the magnitudes of the terms of an output element (sum |a||w| + |bias| there).  e_f32 there is
the native f32 MFMA kernel's error; those kernels carry no folded-LayerNorm statistics, so here e_f32 is the error of the same expression
evaluated in float32 on the host, for every combination alike.  The statistics records are checked against float64 sums of the stored
float32 outputs: |mean - mean64| <= 8 eps mean|v| (six additions and one scaling, one rounding each), and with M2 taken in float64 about
the RECORDED mean, |M2 - M2_64| <= 16 eps M2_64 + tiny (one rounding in each difference, counted twice in its square, the square, the
three-level sum inside a lane and the four butterfly levels: 10 roundings), eps = 2^-24."""
import ctypes as C
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from afm import ffi, ops, synth
from gpu_util import dev

pytestmark = pytest.mark.gpu

TILES = (14, 15, 3)
GUARD = 5                # rows behind the last mapped row of every output / statistics buffer
EPS = 2.0 ** -24
LN_EPS = 1e-5
FLAGS = ("a_stat", "bias", "gelu", "residual", "res_stat", "stat_out", "rowtab")
PERIOD = 50              # row table period: does not divide 128


def _combos():
    """Every valid subset of the folded-LayerNorm inputs, and every subset of the plain inputs with a row table (which the folded forms refuse)."""
    out = []
    for bits in itertools.product((False, True), repeat=len(FLAGS)):
        f = dict(zip(FLAGS, bits))
        if f["res_stat"] and not f["residual"]:
            continue
        if f["rowtab"] and (f["a_stat"] or f["res_stat"] or f["stat_out"]):
            continue
        out.append(f)
    return out


def _g(name, *shape):
    return synth.gaussian(f"e128_{name}", shape)


def _group_stats(t):
    """(mean, M2) per row and 64-column group, float32, as a producer launch records them."""
    g = t.view(t.shape[0], t.shape[1] // 64, 64)
    m = g.mean(-1)
    return torch.stack([m, ((g - m.unsqueeze(-1)) ** 2).sum(-1)], -1).contiguous()


def _row_norm(st, dtype):
    """(mean, rstd) of a row from its group records (Chan's combination), evaluated in `dtype`."""
    st = st.to(dtype)
    groups = st.shape[1]
    mean = st[..., 0].sum(-1) / groups
    m2 = (st[..., 1] + 64.0 * (st[..., 0] - mean.unsqueeze(-1)) ** 2).sum(-1)
    return mean.unsqueeze(-1), 1.0 / torch.sqrt(m2 / (64.0 * groups) + LN_EPS)[:, None]


class _Problem:
    """One GEMM with every side input; rows optionally gathered / scattered through row maps."""

    def __init__(self, M, N, K, a_map=None, c_map=None, a_rows=None, c_rows=None):
        self.M, self.N, self.K, self.a_map, self.c_map = M, N, K, a_map, c_map
        self.a_rows = a_rows if a_rows is not None else M       # rows of the A pool / of the C pool (before the guard rows)
        self.c_rows = c_rows if c_rows is not None else M
        tag = f"{M}_{N}_{K}_{int(a_map is not None)}"
        self.x = _g("x" + tag, self.a_rows, K) * 1.5 + 0.3
        self.x[::7] *= 50.0                                      # mixed magnitudes, as test_linear_split_bf16_mode
        self.w, self.b = _g("w" + tag, N, K) / math.sqrt(K), _g("b" + tag, N)
        self.fold_g = _g("fg" + tag, N)
        self.r = _g("r" + tag, self.c_rows + GUARD, N)
        self.rg, self.rb = _g("rg" + tag, N) * 0.2 + 1.0, _g("rb" + tag, N) * 0.1
        self.tab = _g("tab" + tag, PERIOD, N)
        self.a_idx = self._rows(a_map)
        self.c_idx = self._rows(c_map)
        self.xst = _group_stats(self.x)
        self.rst = _group_stats(self.r) if N % 64 == 0 else None
        self.d = {k: getattr(self, k).to(dev()) for k in ("x", "w", "b", "fold_g", "r", "rg", "rb", "tab", "xst")}
        if self.rst is not None:
            self.d["rst"] = self.rst.to(dev())
        self._acc = {}

    def _rows(self, m):
        r = torch.arange(self.M)
        if m is None:
            return r
        grp, stride, off = m[:3]
        after, skip = (m[3], m[4]) if len(m) == 5 else (0, 0)
        j = r % grp
        return (r // grp) * stride + off + j + (j >= after).long() * skip

    def launch(self, f, scale=None, preact=False):
        """-> (C pool, stat_out pool or None[, preact pool]); NaN wherever the launch wrote nothing."""
        d = self.d
        out = torch.full((self.c_rows + GUARD, self.N), float("nan"), device=dev())
        st = torch.full((self.c_rows + GUARD, self.N // 64, 2), float("nan"), device=dev()) if f["stat_out"] else None
        kw = dict(out=out, rows=self.M, a_map=self.a_map, c_map=self.c_map, act=ffi.ACT_GELU if f["gelu"] else ffi.ACT_NONE, stat_out=st, scale=scale)
        if f["residual"]:
            kw["residual"] = d["r"]
        if f["a_stat"]:
            kw["a_stat"] = (d["xst"], d["fold_g"])
        if f["res_stat"]:
            kw["res_stat"] = (d["rst"], d["rg"], d["rb"])
        if f["rowtab"]:
            kw["rowtab"] = d["tab"]
        if not preact:
            ops.linear(d["x"], d["w"], d["b"] if f["bias"] else None, **kw)
            return out, st
        pre = torch.full((self.c_rows + GUARD, self.N), float("nan"), device=dev())
        a, _, keep = ops.linear(d["x"], d["w"], d["b"] if f["bias"] else None, defer=True, **kw)
        a.preact, a.ldp = pre.data_ptr(), self.N
        ffi.check(ffi.load().afm_linear(C.byref(a), ffi.stream_of(out)), "afm_linear")
        torch.cuda.synchronize()
        del keep
        return out, st, pre

    def host(self, f, dtype):
        """-> (the output rows evaluated on the host in `dtype`, sum of the magnitudes of the terms)."""
        if dtype not in self._acc:
            x, w = self.x[self.a_idx].to(dtype), self.w.to(dtype)
            self._acc[dtype] = (x @ w.t(), x.abs() @ w.abs().t())
        v, mag = self._acc[dtype]
        if f["a_stat"]:
            mu, rs = _row_norm(self.xst[self.a_idx], dtype)
            g = self.fold_g.to(dtype)
            v, mag = rs * (v - mu * g), rs * (mag + (mu * g).abs())
        if f["bias"]:
            v, mag = v + self.b.to(dtype), mag + self.b.to(dtype).abs()
        if f["gelu"]:
            v = F.gelu(v)                                        # |gelu(v)| <= |v|: the magnitudes stay
        if f["residual"]:
            t = self.r[self.c_idx].to(dtype)
            if f["res_stat"]:
                mu, rs = _row_norm(self.rst[self.c_idx], dtype)
                t, tm = (t - mu) * rs * self.rg.to(dtype) + self.rb.to(dtype), (t.abs() + mu.abs()) * rs * self.rg.to(dtype).abs() + self.rb.to(dtype).abs()
            else:
                tm = t.abs()
            v, mag = v + t, mag + tm
        if f["rowtab"]:
            t = self.tab[torch.arange(self.M) % PERIOD].to(dtype)
            v, mag = v + t, mag + t.abs()
        return v, mag


def _per_tile(products, fn):
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


def _check_tiles(pb, outs, what):
    """Tile 14 == 15 == 3 on the mapped rows; every other row of every buffer still NaN (guard rows, the holes of the row map)."""
    idx = pb.c_idx.to(dev())
    other = torch.ones(pb.c_rows + GUARD, dtype=torch.bool, device=dev())
    other[idx] = False
    for tile, o in zip(TILES, outs):
        for k, buf in enumerate(o):
            if buf is None:
                continue
            assert torch.isfinite(buf[idx]).all(), f"{what}: tile {tile} buffer {k} has non-finite values in its rows"
            assert torch.isnan(buf[other]).all(), f"{what}: tile {tile} wrote buffer {k} outside its rows"
            assert torch.equal(buf[idx], outs[0][k][idx]), \
                f"{what}: buffer {k} of tile 14 differs from tile {tile}, max diff {(buf[idx] - outs[0][k][idx]).abs().max().item():.3e}"


def _check_host(pb, f, out, st, what):
    idx = pb.c_idx.to(dev())
    got = out[idx].double().cpu()
    ref, mag = pb.host(f, torch.float64)
    r32, _ = pb.host(f, torch.float32)
    scale = mag + 1e-30
    e_got, e_f32 = ((got - ref).abs() / scale).max().item(), ((r32.double() - ref).abs() / scale).max().item()
    print(f"{what}: max err / sum of magnitudes = {e_got:.2e} (float32 host evaluation {e_f32:.2e})")
    assert e_got <= max(1.5 * e_f32, 3e-7), f"{what}: {e_got:.3e} > max(1.5 x {e_f32:.3e}, 3e-7)"
    if st is not None:
        grp = got.view(pb.M, pb.N // 64, 64)
        rec = st[idx].double().cpu()
        mean64 = grp.mean(-1)
        e_mean = ((rec[..., 0] - mean64).abs() - 8 * EPS * grp.abs().mean(-1)).max().item()
        m2_64 = ((grp - rec[..., 0].unsqueeze(-1)) ** 2).sum(-1)
        e_m2 = ((rec[..., 1] - m2_64).abs() - 16 * EPS * m2_64 - 1e-30).max().item()
        print(f"{what}: statistics: mean excess {e_mean:.2e}, M2 excess {e_m2:.2e} (<= 0 passes)")
        assert e_mean <= 0.0, f"{what}: a recorded mean is off by more than 8 eps mean|v| (excess {e_mean:.3e})"
        assert e_m2 <= 0.0, f"{what}: a recorded M2 is off by more than 16 eps M2 (excess {e_m2:.3e})"


def _name(f):
    return "+".join(k for k in FLAGS if f[k]) or "plain"


_PROBLEMS = {}


def _problem(*key):
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(*key)
    return _PROBLEMS[key]


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("M,N,K", [(129, 192, 128), (145, 64, 128), (255, 192, 128), (145, 192, 512)])
def test_streamed_epilogue_every_input_combination(products, M, N, K):
    pb = _problem(M, N, K)
    for f in _combos():
        what = f"x{products} {M}x{N}x{K} {_name(f)}"
        outs = _per_tile(products, lambda: pb.launch(f))
        _check_tiles(pb, outs, what)
        _check_host(pb, f, outs[0][0], outs[0][1], what)


@pytest.mark.parametrize("products", [6, 9])
def test_streamed_epilogue_row_maps_with_a_hole(products):
    """C, the residual and both statistics through one row map (group, stride, offset, a hole behind the first member), A through another
    - the shapes of test_linear_row_maps_with_a_hole, reduced: 3 samples of 1 + 50 rows, 153 rows = a ragged second row tile."""
    B, L = 3, 50
    pb = _problem(B * (1 + L), 192, 128, (1 + L, 55, 1, 3, 2), (1 + L, 60, 2, 1, 7), B * 55, B * 60)
    for f in _combos():
        if not (f["residual"] or f["stat_out"] or f["a_stat"]):
            continue                                             # the combinations that index a side buffer through a map
        what = f"x{products} row maps {_name(f)}"
        outs = _per_tile(products, lambda: pb.launch(f))
        _check_tiles(pb, outs, what)
        _check_host(pb, f, outs[0][0], outs[0][1], what)


@pytest.mark.parametrize("products", [6, 9])
@pytest.mark.parametrize("declined", ["scale", "preact"])
def test_streamed_epilogue_declined_inputs_fall_back(products, declined):
    """Inputs the streamed form does not serve take the shared epilogue inside the same kernel: equal across 14, 15 and 3."""
    pb = _problem(145, 192, 128)
    f = dict.fromkeys(FLAGS, False)
    f.update(bias=True, gelu=True, residual=True)
    scale = (_g("scale", 192) * 0.2 + 1.0).to(dev()) if declined == "scale" else None
    outs = _per_tile(products, lambda: pb.launch(f, scale=scale, preact=declined == "preact"))
    _check_tiles(pb, outs, f"x{products} declined input {declined}")
