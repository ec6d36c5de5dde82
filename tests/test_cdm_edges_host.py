"""Host side of tests/test_gpu_cdm_edges.py: the weight and input families that take the CDM's three sampling forms to the edges of their
softmax reductions and of their folded LayerNorms, and the proof - on the CPU, in float64 - that every case is the edge it claims to be.

The families are named edits of the synthetic weights (N(0, 1 / sqrt(fan_in)): a nearly uniform softmax everywhere) and of the O(1) inputs;
their scales are fixed here and were not tuned against the kernels.  Checked below, for every family and shape the GPU module runs:

  peakedness   the float64 attention probabilities (oracle.denoiser_ref.cdm_attention_probs) are as concentrated as the family's name says;
  the bound    gpu_util.report_f32_class's bound, margin * max|ref32 - ref64| + 2^-23 max|ref64|, lies below the absolute tolerance the
               GPU test states (OLD_TOL scaled by the size of the outputs): the reference's own float32 error stays small at the edges;
  partition    the encoder reductions split a sample's N points over NPART = 64 partials; at N = 1100 there are waves with two tiles (the
               in-wave rescale by alpha), a ragged last tile (the -inf masking) and no point at all (a partial with m = -inf);
  loops        the 4-step DDPM / DDIM / DPM-Solver++ loops of `combined` keep a bound below their tolerance; those of `both_peaked_30` do
               not, in any float32 evaluation (test_the_both_peaked_loop_is_beyond_float32) - their first step does;
  shifts       rolling the cloud by SHIFTS moves the dominant point of the most peaked softmax row to the first and the last point, to
               both sides of a tile, a wave and a workgroup boundary and into a ragged tile.

The partition is restated from the kernels' documented constants: csrc/perceiver_points.hip (EP_WAVES = 8, EP_SPLIT = NPART / 8) and
csrc/perceiver_rows.hip (ERM_WAVES = 8, ERM_SPLIT = NPART / 8, "as in the VALU form"; 16 x 4 was the first enc_reduce kernel's split,
see NPART in perceiver_internal.h).  Both are kept as entries of PARTITIONS so that a change of either shows."""
import functools

import pytest
import torch

from afm import synth
from oracle import denoiser_ref as dr, diffusion_ref as df, shapes as sh

T_STEPS = 500
B_EDGE, N_EDGE = 2, 1100                                   # the forward tests of the GPU module
SMALL_B, SMALL_NS = 3, (1, 15, 17, 37)                      # fewer points than partials
OLD_TOL, LOOP_TOL, MARGIN = 2e-4, 1e-3, 4.0                 # the project's figures (tests/test_gpu_cdm.py) for outputs of the gaussian family's size (max 4.9)
ENC_K = "contact_model.encoder_cross_attn.0.module.attention.k_proj.weight"
DEC_K = "contact_model.decoder_cross_attn.0.module.attention.k_proj.weight"

# family -> (weight edits {key: factor}, factor of x_t, (factor, offset) of xyz, factor of the scene features, t = T - 1 first)
FAMILIES = {
    "gaussian":       ({}, 1.0, (1.0, 0.0), 1.0, False),
    "enc_peaked_8":   ({ENC_K: 8.0}, 1.0, (1.0, 0.0), 1.0, False),
    "enc_peaked_30":  ({ENC_K: 30.0}, 1.0, (1.0, 0.0), 1.0, False),
    "dec_peaked_8":   ({DEC_K: 8.0}, 1.0, (1.0, 0.0), 1.0, False),
    "dec_peaked_30":  ({DEC_K: 30.0}, 1.0, (1.0, 0.0), 1.0, False),
    "both_peaked_30": ({ENC_K: 30.0, DEC_K: 30.0}, 1.0, (1.0, 0.0), 1.0, False),
    "noise_tail":     ({}, 3.0, (1.0, 0.0), 1.0, True),
    "metres":         ({}, 1.0, (10.0, 0.0), 1.0, False),
    "offset":         ({}, 1.0, (1.0, 20.0), 1.0, False),
    "feat_large":     ({}, 1.0, (1.0, 0.0), 10.0, False),
    "combined":       ({ENC_K: 30.0, DEC_K: 30.0}, 3.0, (10.0, 0.0), 1.0, True),
}
VARIANTS = {"k12": False, "k44": True}                       # the two instantiations of the row-less kernels: 12 inputs / 44 (32 scene features)
LOOP_FAMILIES = ("both_peaked_30", "combined")               # the issue's two
CHAOTIC_LOOP_FAMILY = "both_peaked_30"                       # its 4-step loops are beyond ANY float32 evaluation (test_the_both_peaked_loop_is_beyond_float32): a strict xfail on the GPU, its first step checked instead
# Data seeds, chosen from the oracle alone before any kernel ran.  With one dominant point per encoder row (single_out_dominant_points) the
# oracle's own bound is at most 0.4 of the tolerance in every forward case on the CPU these were measured on; its float32 rounding differs
# between CPU models and torch builds (the same inputs gave 0.4 .. 2.5 x the error elsewhere).  Should test_the_f32_class_bound_is_not_vacuous
# (or the same assertion inside report_f32_class on the GPU machine) fail with no change to the product, the oracle's float32 arithmetic has
# moved, not a kernel: pick the next seed for which the host tests of this module pass - never widen the tolerance or the margin.
EDGE_SEED, SMALL_SEED, LOOP_SEED = 1057, 13, 7


def cases():
    """(family, variant) of the forward tests: feat_large exists only where there are scene features."""
    return [(f, v) for v in VARIANTS for f in FAMILIES if not (f == "feat_large" and not VARIANTS[v])]


def weight_edits(family):
    return dict(FAMILIES[family][0])


def edge_weights(family, point_feat_dim=0):
    """The oracle's float32 state dict with the family's edits."""
    sd = dict(sh.weights(sh.cdm(point_feat_dim=point_feat_dim)))
    for key, factor in weight_edits(family).items():
        sd[key] = sd[key] * factor
    return sd


def edge_inputs(family, B, N, feats, seed=None):
    """x_t [B, N, 6], t [B] (0 and T - 1 among them whenever B >= 2), the text feature, xyz and the scene features (None without).
    Built once per case and shared: not to be written to."""
    return dict(_edge_inputs(family, B, N, feats, (SMALL_SEED if N < 64 else EDGE_SEED) if seed is None else seed))


@functools.lru_cache(maxsize=None)
def _edge_inputs(family, B, N, feats, seed):
    _, fx, (fxyz, oxyz), ff, tail = FAMILIES[family]
    ts = [0, T_STEPS - 1, 250, 77, 3]
    if tail:
        ts[0], ts[1] = ts[1], ts[0]
    t = torch.tensor([ts[b % len(ts)] for b in range(B)])
    x = synth.gaussian(f"cdm_edge_x_{B}_{N}", (B, N, 6), seed=seed) * fx
    xyz = synth.scene_cloud(B, N, seed=seed + B + N) * fxyz + oxyz
    feat = synth.gaussian(f"cdm_edge_feat_{B}_{N}", (B, N, 32), seed=seed) * ff if feats else None
    inp = dict(x=x, t=t, text=synth.text_feature(B, seed=seed), xyz=xyz, feat=feat)
    return single_out_dominant_points(family, inp) if family in ENC_SATURATED else inp


ENC_SATURATED = ("enc_peaked_30", "both_peaked_30", "combined")
PEAK_TARGET = 0.92                                           # the construction's aim; the assertion is the issue's 0.9


def single_out_dominant_points(family, inp):
    """Among ~1000 random logits the two largest of a row are seldom 2.2 apart, and never in all 16 rows of a sample at once; a row with two
    or three rivals is the mixed regime enc_peaked_8 covers.  For the saturated families the cloud is therefore thinned of rivals: while a
    (b, head, latent) row's largest float64 probability is below PEAK_TARGET, the RUNNER-UP point of that row is replaced by a fresh draw
    from the cloud's distribution (a point's key depends on that point alone, so the other logits stay).  Deterministic, from the oracle's
    probabilities alone; a handful of the B N points change."""
    _, fx, (fxyz, oxyz), ff, _ = FAMILIES[family]
    feats = inp["feat"] is not None
    sd = f64(edge_weights(family, 32 if feats else 0))
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    gen = torch.Generator().manual_seed(20240 + inp["x"].shape[1])
    for _ in range(400):
        d = f64(inp)
        pe, _none = dr.cdm_attention_probs(sd, d["x"], d["t"], d["text"], d["xyz"], pc_emb=d["feat"], encoder_only=True)
        if pe.shape[-1] < 2 or pe.max(-1).values.min().item() >= PEAK_TARGET:
            return inp
        top = pe.topk(2, -1)
        for b, h, i in (top.values[..., 0] < PEAK_TARGET).nonzero().tolist():
            n = int(top.indices[b, h, i, 1])
            inp["x"][b, n] = torch.randn(6, generator=gen) * fx
            u = torch.rand(3, generator=gen)
            inp["xyz"][b, n] = torch.stack([4 * u[0] - 2, 4 * u[1] - 2, 2 * u[2]]) * fxyz + oxyz
            if feats:
                inp["feat"][b, n] = torch.randn(32, generator=gen) * ff
    raise AssertionError(f"{family}: the cloud did not reach one dominant point per row")


def f64(v):
    if isinstance(v, dict):
        return {k: f64(x) for k, x in v.items()}
    return v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v


def roll(inp, s):
    """The cloud's points s positions further on: a permutation of the points, under which the function is equivariant."""
    return {k: (torch.roll(v, s, 1) if k in ("x", "xyz", "feat") and v is not None else v) for k, v in inp.items()}


def oracle(sd, inp):
    return dr.cdm_forward(sd, inp["x"], inp["t"], inp["text"], inp["xyz"], pc_emb=inp["feat"])


@functools.lru_cache(maxsize=None)
def reference(family, variant, B, N, shift=0):
    """(inputs, oracle in float32, its float64 twin) of a forward case: computed once per process and shared, not to be written to."""
    feats = VARIANTS[variant]
    sd = edge_weights(family, 32 if feats else 0)
    inp = roll(edge_inputs(family, B, N, feats), shift)
    return inp, oracle(sd, inp), oracle(f64(sd), f64(inp))


@functools.lru_cache(maxsize=None)
def probabilities(family, variant, B, N, shift=0):
    """float64: encoder probabilities [B, H, 2, N], decoder probabilities [B, H, N, 2]"""
    feats = VARIANTS[variant]
    inp = f64(roll(edge_inputs(family, B, N, feats), shift))
    return dr.cdm_attention_probs(f64(edge_weights(family, 32 if feats else 0)), inp["x"], inp["t"], inp["text"], inp["xyz"], pc_emb=inp["feat"])


def old_tol(want64, base=OLD_TOL):
    """The absolute tolerance of the GPU test: the project's figure for outputs of the gaussian family's size, growing with the outputs."""
    return base * max(1.0, want64.abs().max().item() / 5.0)


def f32_class_bound(want32, want64):
    return MARGIN * (want32.double() - want64).abs().max().item() + 2.0 ** -23 * want64.abs().max().item()


# ------------------------------------------------------------------------------------------------ the loops
def loop_noise(B, N, steps=4):
    return (synth.gaussian(f"cdm_edge_loop_xT_{B}_{N}", (B, N, 6), seed=LOOP_SEED),
            [synth.gaussian(f"cdm_edge_loop_{j}_{B}_{N}", (B, N, 6), seed=LOOP_SEED) for j in range(steps)])


def loop_inputs(family, B, N):
    """The conditions of a loop (text, xyz) and its start: x_T carries the family's factor of x_t."""
    inp = edge_inputs(family, B, N, False)
    xT, nz = loop_noise(B, N)
    return inp, xT * FAMILIES[family][1], nz


def oracle_denoiser(family, double):
    sd = edge_weights(family)
    inp = edge_inputs(family, B_EDGE, N_EDGE, False)
    if double:
        sd, inp = f64(sd), f64(inp)
    return lambda x, t, **k: dr.cdm_forward(sd, x, t, inp["text"], inp["xyz"])


@functools.lru_cache(maxsize=None)
def loop_reference(family, steps=None):
    """The 4-step DDPM loop (oracle.diffusion_ref.p_sample, as p_sample_loop chains it) on the recorded noise in float32 and float64;
    ``steps``: only the first so many executed steps."""
    _, xT, nz = loop_inputs(family, B_EDGE, N_EDGE)
    s = df.Schedule(T_STEPS, "cosine", "4")

    def run(double):
        model, img = oracle_denoiser(family, double), (xT.double() if double else xT)
        with torch.no_grad():
            for j, i in enumerate(range(s.num_timesteps - 1, -1, -1)):
                if steps is not None and j >= steps:
                    break
                img = df.p_sample(s, model, img, torch.tensor([i] * img.shape[0]), nz[j].to(img.dtype))["sample"]
        return img
    return run(False), run(True)


def diffusion():
    """The product's 4-step schedule (its DDIM and DPM-Solver++ rows are built on the host)."""
    from afm.base import create_gaussian_diffusion
    from test_gpu_cdm import cdm_cfg
    return create_gaussian_diffusion(cdm_cfg(steps=T_STEPS, respacing="4"))


@functools.lru_cache(maxsize=None)
def solver_reference(family, sampler, steps=None):
    """The deterministic 4-step loops - "ddim" (eta = 0) and "dpm++" (2M) - restated around the oracle on the product's float32 rows,
    promoted with x (as tests/test_gpu_dpm.py:_loop_ref does), in float32 and float64."""
    d = diffusion()
    tmap = torch.tensor(d.timestep_map)
    rows = d.ddim_tables("cpu", 0.0) if sampler == "ddim" else d.dpm_tables("cpu", 2)
    _, xT, _ = loop_inputs(family, B_EDGE, N_EDGE)

    def run(double):
        model, img, prev = oracle_denoiser(family, double), (xT.double() if double else xT), None
        cast = lambda r: r.to(img.dtype)
        with torch.no_grad():
            for i in range(d.num_timesteps - 1, -1 if steps is None else d.num_timesteps - 1 - steps, -1):
                x0 = model(img, tmap[torch.tensor([i] * img.shape[0])])
                if sampler == "ddim":
                    eps = (cast(rows.a)[i] * img - x0) / cast(rows.b)[i]
                    img = x0 * cast(rows.c)[i] + cast(rows.d)[i] * eps
                else:
                    two = cast(rows.a)[i] * img + cast(rows.b)[i] * x0
                    img, prev = (two if prev is None else two + cast(rows.c)[i] * prev), x0
        return img
    return run(False), run(True)


# ------------------------------------------------------------------------------------------------ the partition of the encoder reductions
NPART, TILE = 64, 16
PARTITIONS = {"row-less": (8, 8), "folded rows": (8, 8)}     # (workgroups per sample, waves per workgroup): enc_point_kernel / enc_reduce_mfma_kernel


def ranges(N, form):
    """[(workgroup, wave, w0, w1)]: the points [w0, w1) of every wave of a sample's encoder reduction (w0 >= w1: none), as the kernels
    compute them: per = ceil(N / workgroups), wper = ceil(per / waves) rounded up to whole 16-point tiles."""
    nwg, nw = PARTITIONS[form]
    assert nwg * nw == NPART
    per = (N + nwg - 1) // nwg
    wper = ((per + nw - 1) // nw + TILE - 1) // TILE * TILE
    out = []
    for wg in range(nwg):
        n0, n1 = wg * per, min(N, wg * per + per)
        for wave in range(nw):
            w0 = n0 + wave * wper
            out.append((wg, wave, w0, min(n1, w0 + wper)))
    return out


def edges_at(N, form, p):
    """The partition edges point p of a sample sits on."""
    kinds = set()
    if p == 0:
        kinds.add("first point")
    if p == N - 1:
        kinds.add("last point")
    live = [r for r in ranges(N, form) if r[2] < r[3]]
    j = next(i for i, (_, _, w0, w1) in enumerate(live) if w0 <= p < w1)
    wg, wave, w0, w1 = live[j]
    tile0 = w0 + (p - w0) // TILE * TILE
    if min(w1, tile0 + TILE) - tile0 < TILE:
        kinds.add("ragged tile")
    if p == tile0 + TILE - 1 and p + 1 < w1:
        kinds.add("below a tile boundary")
    if p == tile0 and p > w0:
        kinds.add("above a tile boundary")
    if p == w1 - 1 and j + 1 < len(live):
        kinds.add("below a wave boundary" if live[j + 1][0] == wg else "below a workgroup boundary")
    if p == w0 and j > 0:
        kinds.add("above a wave boundary" if live[j - 1][0] == wg else "above a workgroup boundary")
    return kinds


EDGE_KINDS = {"first point", "last point", "ragged tile", "below a tile boundary", "above a tile boundary", "below a wave boundary",
              "above a wave boundary", "below a workgroup boundary", "above a workgroup boundary"}
SHIFT_FAMILY = "enc_peaked_30"
DOMINANT = 315                                               # the point the most peaked encoder row of SHIFT_FAMILY sits on at shift 0 (asserted below)
# positions 0, 15, 16, 31, 32 (tile and wave boundary of workgroup 0), 133 (its ragged tile), 137 | 138 (workgroup boundary), 600, 1099
SHIFTS = [0] + [(p - DOMINANT) % N_EDGE for p in (0, 15, 16, 31, 32, 133, 137, 138, 600, 1093, 1099)]


def dominant(p_enc):
    """(b, head, latent, point) of the encoder row with the largest maximum probability"""
    mx, arg = p_enc.max(-1)
    b, h, i = (int(v) for v in torch.unravel_index(mx.argmax(), mx.shape))
    return b, h, i, int(arg[b, h, i])


# ------------------------------------------------------------------------------------------------ the checks
@pytest.mark.parametrize("family,variant", cases())
def test_families_are_as_peaked_as_their_names_say(family, variant):
    p_enc, p_dec = probabilities(family, variant, B_EDGE, N_EDGE)
    assert p_enc.shape == (B_EDGE, 8, 2, N_EDGE) and p_dec.shape == (B_EDGE, 8, N_EDGE, 2)
    assert torch.allclose(p_enc.sum(-1), torch.ones(()).double()) and torch.allclose(p_dec.sum(-1), torch.ones(()).double())
    emax, dmax = p_enc.max(-1).values, p_dec.max(-1).values
    print(f"[cdm-edges] {family} {variant}: encoder row max {emax.min().item():.3f} .. {emax.max().item():.3f}, "
          f"decoder max > 0.99 for {(dmax > 0.99).double().mean().item():.2f} of the points")
    if family == "gaussian":
        assert emax.max().item() < 0.05 and dmax.max().item() < 0.99      # the regime the suite had: nothing concentrates
    if family in ("enc_peaked_30", "both_peaked_30", "combined"):
        assert emax.min().item() >= 0.9                       # every (b, head, latent) row: single_out_dominant_points
    if family == "enc_peaked_8":
        assert 0.5 < emax.max().item() < 1.0 and emax.min().item() < 0.5      # mixed: several tiles carry weight
    if family in ("dec_peaked_30", "both_peaked_30", "combined"):
        assert (dmax > 0.99).double().mean().item() >= 0.5


@pytest.mark.parametrize("family,variant", cases())
def test_the_f32_class_bound_is_not_vacuous(family, variant):
    _, want32, want64 = reference(family, variant, B_EDGE, N_EDGE)
    bound, tol = f32_class_bound(want32, want64), old_tol(want64)
    print(f"[cdm-edges] {family} {variant}: bound {bound:.2e} < tolerance {tol:.2e} (max|ref64| {want64.abs().max().item():.2f})")
    assert torch.isfinite(want32).all() and bound < tol


@pytest.mark.parametrize("N", SMALL_NS)
def test_the_bound_is_not_vacuous_for_small_clouds(N):
    _, want32, want64 = reference("both_peaked_30", "k12", SMALL_B, N)
    assert torch.isfinite(want32).all() and f32_class_bound(want32, want64) < old_tol(want64)
    assert N < NPART                                          # fewer points than partials


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_bound_is_not_vacuous_at_the_shifts(shift):
    _, want32, want64 = reference(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE, shift)
    assert f32_class_bound(want32, want64) < old_tol(want64)
    base = reference(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE)[2]
    assert (torch.roll(want64, -shift, 1) - base).abs().max().item() < 1e-9      # the oracle is equivariant


@pytest.mark.parametrize("family", [f for f in LOOP_FAMILIES if f != CHAOTIC_LOOP_FAMILY])
def test_the_bound_is_not_vacuous_for_the_loops(family):
    want32, want64 = loop_reference(family)
    bound, tol = f32_class_bound(want32, want64), old_tol(want64, LOOP_TOL)
    print(f"[cdm-edges] 4-step loop {family}: bound {bound:.2e} < tolerance {tol:.2e} (max|ref64| {want64.abs().max().item():.2f})")
    assert torch.isfinite(want32).all() and bound < tol
    for sampler in ("ddim", "dpm++"):
        want32, want64 = solver_reference(family, sampler)
        bound, tol = f32_class_bound(want32, want64), old_tol(want64, LOOP_TOL)
        print(f"[cdm-edges] 4-step {sampler} loop {family}: bound {bound:.2e} < tolerance {tol:.2e} (max|ref64| {want64.abs().max().item():.2f})")
        assert torch.isfinite(want32).all() and bound < tol


def test_the_both_peaked_loop_is_beyond_float32():
    """Why tests/test_gpu_cdm_edges.py expects its 4-step loops of `both_peaked_30` to miss the issue's bound (a strict xfail, derivation in
    DESIGN.md 4.5): four steps through both softmaxes at factor 30 amplify a rounding error of the first step (a near-tie that tips) so
    far that the float32 ORACLE itself misses its float64 twin by several times the loops' tolerance - bound / tolerance 2.7 .. 30 over 48
    noise seeds at N = 1100, 1.1 .. 36 at N = 37, 150 and 333, for DDPM, DDIM and 2M alike.  `combined` (the same weights, outputs to 27)
    stays below 0.9.  What is well-posed, and checked on the GPU in the float32 class, is the state after ONE step of each loop."""
    want32, want64 = loop_reference(CHAOTIC_LOOP_FAMILY)
    assert f32_class_bound(want32, want64) > old_tol(want64, LOOP_TOL)
    for sampler in ("ddim", "dpm++"):
        want32, want64 = solver_reference(CHAOTIC_LOOP_FAMILY, sampler)
        assert f32_class_bound(want32, want64) > old_tol(want64, LOOP_TOL)
    for want32, want64 in (loop_reference(CHAOTIC_LOOP_FAMILY, 1), solver_reference(CHAOTIC_LOOP_FAMILY, "ddim", 1), solver_reference(CHAOTIC_LOOP_FAMILY, "dpm++", 1)):
        bound, tol = f32_class_bound(want32, want64), old_tol(want64, LOOP_TOL)
        print(f"[cdm-edges] first step of a {CHAOTIC_LOOP_FAMILY} loop: bound {bound:.2e} < tolerance {tol:.2e}")
        assert torch.isfinite(want32).all() and bound < tol


@pytest.mark.parametrize("form", list(PARTITIONS))
def test_partition_has_every_kind_of_wave(form):
    """N = 1100, 8 x 8: per = 138, wper = 32 - waves 0 .. 3 of a workgroup hold two tiles, wave 4 holds 10 points (6 in the last
    workgroup), waves 5 .. 7 none."""
    r = ranges(N_EDGE, form)
    assert len(r) == NPART
    live = [(w0, w1) for _, _, w0, w1 in r if w0 < w1]
    assert live[0][0] == 0 and live[-1][1] == N_EDGE and all(a[1] == b[0] for a, b in zip(live, live[1:]))      # a partition of the points
    assert any(w1 - w0 >= 2 * TILE for w0, w1 in live), "no wave with two tiles: the in-wave rescale never runs"
    assert any((w1 - w0) % TILE for w0, w1 in live), "no ragged tile"
    assert any(w0 >= w1 for _, _, w0, w1 in r), "no wave without points"
    if PARTITIONS[form] == (8, 8):
        assert [(w1 - w0) for _, _, w0, w1 in r[:8]] == [32, 32, 32, 32, 10, -22, -54, -86]
    for n in SMALL_NS:                                        # small clouds: most partials empty
        assert sum(w0 < w1 for _, _, w0, w1 in ranges(n, form)) <= min(n, 8)
    assert max(w1 - w0 for _, _, w0, w1 in ranges(1000, form)) == TILE      # the suite's N = 1000 has one tile per wave


def test_shifts_visit_every_partition_edge():
    p_enc, _ = probabilities(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE)
    b, h, i, n = dominant(p_enc)
    assert n == DOMINANT and p_enc[b, h, i, n].item() > 0.99, (b, h, i, n, p_enc[b, h, i, n].item())
    assert len(set(SHIFTS)) == len(SHIFTS) == 12
    seen = {form: set() for form in PARTITIONS}
    for s in SHIFTS:
        pe, _ = probabilities(SHIFT_FAMILY, "k12", B_EDGE, N_EDGE, s)
        assert dominant(pe) == (b, h, i, (n + s) % N_EDGE)    # from the float64 probabilities at the rolled cloud
        for form in PARTITIONS:
            seen[form] |= edges_at(N_EDGE, form, (n + s) % N_EDGE)
    for form in PARTITIONS:
        assert seen[form] == EDGE_KINDS, (form, EDGE_KINDS - seen[form])


# ------------------------------------------------------------------------------------------------ the training-path attention (tests/test_gpu_train.py)
def _xattn_cases():
    import test_gpu_train as TT
    return [(kind, shape, qs) for kind, shapes in (("fq", TT.XQ_EDGE_SHAPES), ("fk", TT.XK_EDGE_SHAPES)) for shape in shapes for qs in TT.PEAKED]


@pytest.mark.parametrize("kind,shape,qscale", _xattn_cases())
def test_the_bound_is_not_vacuous_for_the_peaked_training_attention(kind, shape, qscale):
    """Forward, dQ, dK and dV of the peaked few-query / few-key cases: the float32 autograd reference stays so close to float64 that margin x
    its error + one ulp lies below the existing tolerances - and the softmax is as concentrated as the case claims."""
    import test_gpu_train as TT
    q, k, v, dO = TT.xattn_inputs(kind, *shape, qscale)
    H = shape[2]
    want32, want64 = TT.xattn_reference(q, k, v, dO, H, torch.float32), TT.xattn_reference(q, k, v, dO, H, torch.float64)
    for what, w32, w64, tol in zip(("out", "dQ", "dK", "dV"), want32, want64, TT.xattn_tolerances(want64)):
        bound = f32_class_bound(w32, w64)
        print(f"[cdm-edges] {kind} {shape} q x {qscale:g} {what}: bound {bound:.2e} < tolerance {tol:.2e}")
        assert torch.isfinite(w32).all() and bound < tol
    _, p = TT._xattn_ref(q.double(), k.double(), v.double(), H)
    pmax = p.max(-1).values
    if kind == "fk" and qscale == 30.0:
        assert (pmax > 0.99).double().mean().item() >= 0.5               # saturated to {1, 0} for most (point, head) pairs
    if kind == "fq" and qscale == 30.0 and shape[1] > 3:
        assert pmax.max().item() > 0.99 and pmax.median().item() > 0.5 and pmax.min().item() > 0.25      # one key carries most rows, two or three the others
