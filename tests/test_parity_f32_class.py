"""The yardstick of the model-level `-m gpu` parity tests, checked without a GPU: the float64 twin of every oracle function those tests
use (tests/gpu_util.py::to_f64 of the state dict and of the floating-point inputs, nothing else changed) runs, returns float64 and stays
within test_oracle_golden.py's TOL of the float32 reference - it is the same function - and report_f32_class accepts what is in the
reference's error class and rejects an error of a tenth of the tolerances those tests stated before (2e-5 on a 2e-4 bar)."""
import pytest
import torch

from afm import synth
from oracle import denoiser_ref as dr
from oracle import diffusion_ref as df
from oracle import scene_ref as sr
from oracle import shapes as sh

from conftest import golden
from gpu_util import report, report_f32_class, to_f64

TOL = 1e-5              # tests/test_oracle_golden.py


def both(fn, *args, **kw):
    """fn in float32 and its float64 twin."""
    return fn(*args, **kw), fn(*to_f64(args), **to_f64(kw))


def _cmdm_model(sd, g):
    return lambda x, t, **k: dr.cmdm_forward(sd, x, t, g["text_feat"], x_mask=g["x_mask"], cont_emb=g["cont_emb"])


def cmdm_forward_golden():
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    w64 = dr.cmdm_forward(to_f64(sd), g["x"].double(), g["t"], g["text_feat"].double(), x_mask=g["x_mask"], cont_emb=g["cont_emb"].double())
    return g["out"], w64, None, 2e-4


def cmdm_forward_full_size():
    B, L = 2, 196
    x, t = synth.gaussian("full_x", (B, L, 263)), torch.tensor([999, 17])
    cont, text, mask = synth.gaussian("full_cont", (B, 128, 256)), synth.text_feature(B), synth.frame_mask(B, L, seed=3)
    w32, w64 = both(dr.cmdm_forward, sh.weights(sh.cmdm()), x, t, text, x_mask=mask, cont_emb=cont)
    return w32, w64, ~mask, 3e-4


def cmdm_100_step_loop():
    B, L = 4, 60
    text, cont, mask = synth.text_feature(B), synth.gaussian("c0_cont", (B, 128, 256)), synth.frame_mask(B, L, seed=9)
    xT, nz = synth.gaussian("c0_xT", (B, L, 263)), [synth.gaussian(f"c0_nz{j}", (B, L, 263)) for j in range(100)]

    def loop(sd, text, cont, xT, nz):
        return df.p_sample_loop(df.Schedule(100), lambda x, t, **k: dr.cmdm_forward(sd, x, t, text, x_mask=mask, cont_emb=cont), xT, nz)
    w32, w64 = both(loop, sh.weights(sh.cmdm()), text, cont, xT, nz)
    return w32, w64, None, 1e-3


def cdm_forward_golden():
    g = golden("cdm_forward_N256")
    w64 = dr.cdm_forward(to_f64(sh.weights(sh.cdm())), g["x"].double(), g["t"], g["text_feat"].double(), g["xyz"].double())
    return g["out"], w64, None, 2e-4


def cdm_forward_full_size():
    B, N = 2, 8192
    x, xyz, text = synth.gaussian("cdm_full_x", (B, N, 6)), synth.scene_cloud(B, N, seed=51), synth.text_feature(B)
    w32, w64 = both(dr.cdm_forward, sh.weights(sh.cdm()), x, torch.tensor([499, 3]), text, xyz)
    return w32, w64, None, 2e-4


def scene_map_encoder_full_size():
    sd = {k: v for k, v in sh.weights(sh.cmdm()).items() if k.startswith("contact_encoder.")}
    xyz, contact = synth.scene_cloud(1, 8192, seed=77), synth.contact_map(1, 8192, seed=77)
    (w32, a32), (w64, a64) = both(sr.scene_map_encoder, sd, "contact_encoder", xyz, contact, blocks=(2, 2, 2, 2), return_aux=True)
    for l32, l64 in zip(a32, a64):                 # the float64 run walks the same discrete path
        assert torch.equal(l32["p"], l64["p"].float()) and torch.equal(l32["self_knn_idx"], l64["self_knn_idx"])
    return w32, w64, None, 2e-4


def cmdm_forward_with_encoder_golden():
    g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
    w64 = dr.cmdm_forward(to_f64(sd), g["x"].double(), g["t"], g["text_feat"].double(), g["xyz"].double(), g["contact"].double(), g["x_mask"])
    return g["out"], w64, None, 3e-4


def p_sample_golden(tt, key):
    def case():
        g, gs, sd = golden("cmdm_forward_N1024_L16"), golden(f"cmdm_p_sample_t{tt}"), sh.weights(sh.cmdm())
        out = df.p_sample(df.Schedule(1000), _cmdm_model(to_f64(sd), to_f64(g)), gs["x"].double(), torch.tensor([tt, tt]), gs["noise"].double())
        return gs[key], out[key], None, 2e-4
    return case


def loop_golden(steps, resp, tag, clip):
    def case():
        g, sd = golden("cmdm_forward_N1024_L16"), sh.weights(sh.cmdm())
        s = df.Schedule(steps, "cosine", resp)
        nz = [synth.gaussian(f"loop_{tag}_{j}", (2, 16, 263)).double() for j in range(s.num_timesteps)]
        xT = synth.gaussian(f"loop_{tag}_xT", (2, 16, 263)).double() * (2.0 if clip else 1.0)
        w64 = df.p_sample_loop(s, _cmdm_model(to_f64(sd), to_f64(g)), xT, nz, clip_denoised=clip)
        return golden(f"cmdm_loop_{tag}{'_clip' if clip else ''}")["sample"], w64, None, 1e-3
    return case


def trans_dec_golden():
    g = golden("cmdm_forward_N1024_L16")
    w64 = dr.cmdm_trans_dec_forward(to_f64(sh.weights(sh.cmdm_trans_dec())), g["x"].double(), g["t"], g["text_feat"].double(), g["xyz"].double(),
                                    g["contact"].double(), g["x_mask"])
    return golden("cmdm_trans_dec_N1024_L16")["out"], w64, ~g["x_mask"], 5e-4


def transition_down_golden(stride):
    def case():
        g = golden(f"transition_down_s{stride}")
        sd = {"td." + k: v for k, v in sh.weights(sh.transition_down("", 32, 64, stride)).items()}
        n_p, y, _, aux = sr.transition_down(to_f64(sd), "td", g["p"].double(), g["x"].double(), g["o"], stride, 16)
        assert torch.equal(n_p.float(), g["n_p"])                      # the sampled coordinates of the float32 reference run
        return g["y"], y, None, 2e-4
    return case


def pt_block_golden(c, k):
    def case():
        g = golden(f"pt_block_c{c}_k{k}")
        sd = {"b." + kk: v for kk, v in sh.weights(sh.pt_block("", c)).items()}
        return g["y"], sr.point_transformer_block(to_f64(sd), "b", g["p"].double(), g["x"].double(), g["o"], k), None, 2e-4
    return case


def scene_map_encoder_golden():
    g = golden("scene_map_encoder_N1024")
    return g["out"], sr.scene_map_encoder(to_f64(sh.weights(sh.scene_map_encoder(""))), "", g["xyz"].double(), g["contact"].double()), None, 3e-4


def point_transformer_seg_all_rows():
    g = golden("point_transformer_seg_N4096")
    w32, w64 = both(sr.point_transformer_seg, sh.weights(sh.point_transformer_seg("")), "", g["xyz"], g["color"])
    return w32, w64, None, 3e-4


CASES = {
    "cmdm_forward_golden": cmdm_forward_golden,
    "cmdm_forward_full_size": cmdm_forward_full_size,
    "cmdm_100_step_loop": cmdm_100_step_loop,
    "cdm_forward_golden": cdm_forward_golden,
    "cdm_forward_full_size": cdm_forward_full_size,
    "scene_map_encoder_full_size": scene_map_encoder_full_size,
    "cmdm_forward_with_encoder_golden": cmdm_forward_with_encoder_golden,
    "p_sample_t999_sample": p_sample_golden(999, "sample"),
    "p_sample_t999_pred_xstart": p_sample_golden(999, "pred_xstart"),
    "p_sample_t0_sample": p_sample_golden(0, "sample"),
    "loop_T20": loop_golden(20, "", "T20", False),
    "loop_r5_clip": loop_golden(1000, "5", "r5", True),
    "trans_dec_golden": trans_dec_golden,
    "transition_down_s4": transition_down_golden(4),
    "transition_down_s8": transition_down_golden(8),
    "pt_block_c32": pt_block_golden(32, 8),
    "pt_block_c64": pt_block_golden(64, 16),
    "scene_map_encoder_golden": scene_map_encoder_golden,
    "point_transformer_seg_all_rows": point_transformer_seg_all_rows,
}


@pytest.mark.parametrize("name", list(CASES))
def test_float64_twin_and_the_helper_on(name):
    with torch.no_grad():
        want32, want64, select, old_tol = CASES[name]()
    # (a) the float64 twin is the same function
    assert want32.dtype == torch.float32 and want64.dtype == torch.float64 and want32.shape == want64.shape
    d = want32.double() - want64
    if select is not None:
        d = d[select]
    print(f"[f64 twin] {name}: max|want32 - want64| = {d.abs().max().item():.3e}, rms {d.pow(2).mean().sqrt().item():.3e}")
    assert d.abs().max().item() <= TOL
    # (b) accepted: the reference itself, and the correctly rounded float64 result
    kw = dict(select=select, record=False)
    report_f32_class(f"{name}: got = want32", want32, want32, want64, old_tol, **kw)
    r = report_f32_class(f"{name}: got = float32(want64)", want64.float(), want32, want64, old_tol, **kw)
    assert max(r) <= 1.0
    # (c) rejected: a tenth of the 2e-4 bar, which report() lets through
    g = torch.randn(want32.shape, generator=torch.Generator().manual_seed(7))
    off = want32 + 2e-5 * g
    report(f"{name}: want32 + 2e-5 g", off if select is None else off[select], want32 if select is None else want32[select], old_tol)
    with pytest.raises(AssertionError, match="hip - f64"):
        report_f32_class(f"{name}: got = want32 + 2e-5 g", off, want32, want64, old_tol, **kw)
    # (d) a reference that is itself 1e-3 off makes the bound vacuous: refused
    with pytest.raises(AssertionError, match="vacuous"):
        report_f32_class(f"{name}: want32 1e-3 off", want32, want32 + 1e-3, want64, old_tol, **kw)


def test_helper_refuses_a_float32_twin_and_a_shape_mismatch():
    a = torch.zeros(4, 3)
    with pytest.raises(AssertionError, match="float64 twin"):
        report_f32_class("f32 twin", a, a, a, 2e-4, record=False)
    with pytest.raises(AssertionError):
        report_f32_class("shape", a, a, a.double()[:2], 2e-4, record=False)
