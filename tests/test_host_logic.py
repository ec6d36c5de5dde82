"""CPU tests of the host layer: registry / config / diffusion tables / state-dict surface / C-ABI exports.
No kernel is launched here (no GPU in the build container)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from afm import base, ffi
from afm import diffusion as gd
from afm.config import load_config, to_config
from afm.registry import Registry
from conftest import GOLDEN, ROOT, golden


def test_registry_behaviour():
    reg = Registry("thing")

    @reg.register()
    class A:
        pass

    class B:
        pass
    reg.register(B)
    assert reg.get("A") is A and reg.get("B") is B and "A" in reg
    with pytest.raises(AssertionError):
        reg.register(A)
    with pytest.raises(KeyError):
        reg.get("missing")
    assert dict(iter(reg)) == {"A": A, "B": B}


def test_drop_in_import_paths_register_models():
    import models                                   # noqa: F401  side-effect registration like the reference
    from models.base import Model, create_model_and_diffusion  # noqa: F401
    from diffusion import gaussian_diffusion as g2
    from diffusion.respace import SpacedDiffusion, space_timesteps  # noqa: F401
    from utils.misc import compute_repr_dimesion
    assert "CMDM" in Model and "CDM" in Model
    assert compute_repr_dimesion("h3d") == 263 and compute_repr_dimesion("pos") == 66
    assert compute_repr_dimesion("contact_cont_joints") == 6
    assert g2.get_named_beta_schedule is gd.get_named_beta_schedule


def test_config_composition_and_overrides():
    cfg = load_config("text_to_motion_contact_motion_gen", "cmdm",
                      ["model.data_repr=h3d", "model.text_model.max_length=20", "diffusion.steps=500"])
    assert cfg.model.contact_model.num_points == 8192           # ${task.dataset.num_points}
    assert cfg.diffusion.steps == 500 and cfg.model.text_model.max_length == 20
    assert cfg.model.num_layers == [1, 1, 1, 1, 1]
    cdm = load_config("text_to_motion_contact_gen", "cdm", ["model.arch=Perceiver", "model.scene_model.use_scene_model=False"])
    assert cdm.model.scene_model.use_color is False and cdm.model.arch_perceiver.encoder_q_input_channels == 512


@pytest.mark.parametrize("T,resp", [(1000, ""), (500, ""), (1000, "5"), (1000, "50")])
def test_diffusion_tables_match_reference(T, resp):
    g = golden(f"schedule_T{T}_r{resp or 'none'}")
    cfg = to_config(dict(diffusion=dict(predict_xstart=True, steps=T, noise_schedule="cosine", timestep_respacing=resp,
                                        rescale_timesteps=False, loss_type="MSE", learn_sigma=False, sigma_small=True)))
    d = base.create_gaussian_diffusion(cfg)
    assert isinstance(d, gd.SpacedDiffusion) and d.timestep_map == g["timestep_map"].tolist()
    idx = g["probe"].numpy()
    for k in ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_variance",
              "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        np.testing.assert_allclose(getattr(d, k)[idx], g[k].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(getattr(d, k).sum(), g[k + "_sum"].numpy(), rtol=1e-12)


def test_space_timesteps_and_errors():
    assert gd.space_timesteps(300, [10, 15, 20]) == gd.space_timesteps(300, "10,15,20")
    assert len(gd.space_timesteps(1000, "ddim50")) == 50
    with pytest.raises(ValueError):
        gd.space_timesteps(10, [20])
    with pytest.raises(NotImplementedError):
        gd.get_named_beta_schedule("sigmoid", 10)
    with pytest.raises(NotImplementedError):      # dead configurations are rejected loudly, not silently mis-sampled
        gd.GaussianDiffusion(betas=[0.1], model_mean_type=gd.ModelMeanType.EPSILON,
                             model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def _cmdm_cfg():
    return load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263"])


def test_cmdm_state_dict_keys_match_reference():
    model = base.create_model(_cmdm_cfg(), device="cpu")
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {}
    for line in open(os.path.join(GOLDEN, "cmdm_state_dict_keys.txt")):
        k, shp = line.strip().split(" ", 1)
        want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
    # the golden listing was dumped at num_points=1024: same keys / shapes (weights do not depend on N)
    assert have == want
    assert sum(p.numel() for p in model.parameters()) == 12204111


def test_cmdm_trans_dec_state_dict_keys_match_reference():
    model = base.create_model(load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263",
                                                                                       "model.arch=trans_dec"]), device="cpu")
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {}
    for line in open(os.path.join(GOLDEN, "cmdm_trans_dec_state_dict_keys.txt")):
        k, shp = line.strip().split(" ", 1)
        want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
    assert have == want, set(have) ^ set(want)


def test_cdm_state_dict_keys_match_reference():
    cfg = load_config("text_to_motion_contact_gen", "cdm", ["model.arch=Perceiver", "model.scene_model.use_scene_model=False",
                                                           "model.input_feats=6"])
    model = base.create_model(cfg, device="cpu")
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {}
    for line in open(os.path.join(GOLDEN, "cdm_state_dict_keys.txt")):
        k, shp = line.strip().split(" ", 1)
        want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
    assert have == want
    assert sum(p.numel() for p in model.parameters()) == 5431814
    seg = base.create_model(load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.arch=Perceiver",
                                        "model.scene_model.pretrained_weight=''", "task.dataset.use_color=True"]), device="cpu")
    have = {k[len("scene_model."):]: tuple(v.shape) for k, v in seg.state_dict().items() if k.startswith("scene_model.")}
    want = {}
    for line in open(os.path.join(GOLDEN, "seg_state_dict_keys.txt")):
        k, shp = line.strip().split(" ", 1)
        want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
    assert have == want                                                      # frozen scene backbone: reference key names
    mlp = base.create_model(load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "task.dataset.use_openscene=True"]),
                            device="cpu")                                    # yaml default arch: 'MLP' (configs/model/cdm.yaml)
    have = {k: tuple(v.shape) for k, v in mlp.state_dict().items()}
    want = {}
    for line in open(os.path.join(GOLDEN, "cdm_mlp_state_dict_keys.txt")):
        k, shp = line.strip().split(" ", 1)
        want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
    assert have == want
    for arch, listing in (("PointTrans", "cdm_pointtrans_state_dict_keys.txt"), ("PointTransV2", "cdm_pointtransv2_state_dict_keys.txt")):
        m = base.create_model(load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.scene_model.use_scene_model=False",
                                                                               f"model.arch={arch}", "task.dataset.num_points=1024"]), device="cpu")
        have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        want = {}
        for line in open(os.path.join(GOLDEN, listing)):
            k, shp = line.strip().split(" ", 1)
            want[k] = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
        assert have == want, (arch, set(have) ^ set(want))
    with pytest.raises(NotImplementedError):                                 # unknown variants fail loudly
        base.create_model(load_config("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.arch=Nope", "model.scene_model.pretrained_weight=''"]), device="cpu")


def test_product_path_refuses_cpu_tensors():
    model = base.create_model(_cmdm_cfg(), device="cpu").eval()
    with pytest.raises(ffi.AfmError):
        with torch.no_grad():
            model(torch.zeros(1, 8, 263), torch.zeros(1, dtype=torch.long), c_text_feat=torch.zeros(1, 512),
                  c_cont_emb=torch.zeros(1, 128, 256), x_mask=torch.zeros(1, 8, dtype=torch.bool))
    with pytest.raises(ffi.AfmError):              # the training path is HIP-only as well: loud, no eager fallback
        model.train()(torch.zeros(1, 8, 263), torch.zeros(1, dtype=torch.long), c_text_feat=torch.zeros(1, 512),
                      c_cont_emb=torch.zeros(1, 128, 256), x_mask=torch.zeros(1, 8, dtype=torch.bool))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "afford-motion_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_c_abi_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    assert declared == set(ffi.EXPORTS), declared ^ set(ffi.EXPORTS)
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    lib = ctypes.CDLL(ffi.lib_path())
    for name in declared:
        assert hasattr(lib, name), f"missing export {name}"
    assert ffi.load().afm_version() == ffi.ABI_VERSION == 7     # pure host call, no GPU needed


def test_ctypes_mirrors_match_the_c_structs(tmp_path):
    """Every ctypes.Structure of afm/ffi.py against the struct it mirrors in include/afm_hip.h: total size and the offset of every field, as gcc
    lays them out (a field added on one side only shifts everything behind it silently - the library would read garbage pointers)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pairs = {"afm_linear_args": ffi.LinearArgs, "afm_linear_wgrad_args": ffi.WgradArgs, "afm_pt_attention_args": ffi.PtAttentionArgs,
             "afm_lin": ffi.Lin, "afm_ln": ffi.Ln, "afm_mha_w": ffi.MhaW, "afm_mlp_w": ffi.MlpW, "afm_cdm_weights": ffi.CdmWeights,
             "afm_profile_entry": ffi.ProfileEntry, "afm_encoder_layer_weights": ffi.EncoderLayerWeights, "afm_cmdm_weights": ffi.CmdmWeights,
             "afm_ddpm_args": ffi.DdpmArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(out[cname]) == ctypes.sizeof(cls), (cname, out[cname], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_gemm_arithmetic_switches_are_host_state():
    """ABI v3: the GEMM arithmetic is a field of afm_linear_args / the weight packs; the switch lives in the Python host (afm.ops),
    initialised from AFM_GEMM_SPLIT* in the host's environment.  The library exports no setter and reads no environment."""
    from afm import ops
    want = (int(os.environ.get("AFM_GEMM_SPLIT", "6")), int(os.environ.get("AFM_GEMM_SPLIT_MIN_N", "0")))      # round 6: six products for sampling
    assert ops.get_train_gemm_split() == int(os.environ.get("AFM_GEMM_SPLIT_TRAIN", "9"))                        # ... nine on the training tape
    la = ffi.LinearArgs(); ops.fill_arith_train(la)
    assert la.arith == ffi.ARITH_BF16X9 or "AFM_GEMM_SPLIT_TRAIN" in os.environ
    assert ops.set_train_gemm_split(6) == ops.DEFAULT_TRAIN_PRODUCTS or "AFM_GEMM_SPLIT_TRAIN" in os.environ
    ops.fill_arith_train(la)
    assert la.arith == ffi.ARITH_BF16X6 and ops.set_train_gemm_split(int(os.environ.get("AFM_GEMM_SPLIT_TRAIN", "9"))) == 6
    with pytest.raises(ffi.AfmError):
        ops.set_train_gemm_split(1)
    saved = ops.get_gemm_split()
    assert saved == want
    try:
        assert ops.set_gemm_split(6, 0) == saved and ops.get_gemm_split() == (6, 0) and ops.gemm_arith() == (ffi.ARITH_BF16X6, 0)
        assert ops.set_gemm_split(0) == 6 and ops.get_gemm_split() == (0, 0) and ops.gemm_arith() == (ffi.ARITH_F32, 0)
        with pytest.raises(ffi.AfmError):
            ops.set_gemm_split(7)
        with pytest.raises(ffi.AfmError):
            ops.set_gemm_split(9, -1)
        assert ops.get_gemm_split() == (0, 0)
        ops.set_gemm_split(9, 1024)
        a = ffi.LinearArgs()
        ops.fill_arith(a)
        assert (a.arith, a.arith_min_n, a.tune) == (ffi.ARITH_BF16X9, 1024, 0)
    finally:
        ops.set_gemm_split(*saved)
    if os.path.exists(ffi.lib_path()):
        import subprocess
        syms = subprocess.run(["nm", "-D", "--defined-only", ffi.lib_path()], capture_output=True, text=True).stdout
        assert "afm_linear_set_split" not in syms                      # no process-wide switch left in the library
        imports = subprocess.run(["nm", "-D", "--undefined-only", ffi.lib_path()], capture_output=True, text=True).stdout
        assert " getenv" not in imports and "secure_getenv" not in imports, "libafm_hip.so must not read the environment"
        assert ffi.load().afm_version() == ffi.ABI_VERSION == 7


def _build_hip_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("afm_build_hip", os.path.join(ROOT, "afford-motion_amd", "build_hip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_isa_scan_flags_the_known_bad_kernel_form(tmp_path):
    """Round 3: packed-f32 VALU instructions are fenced - two kernels lost values in lanes 48..63 inside them whenever a
    second stream was active (round 2's lat_decfold, round 3's statistics-carrying GEMM epilogue; profiles/r03_packed_f32_defect.md).  The
    library is compiled with the `packed-fp32-ops` target feature off, and the build scans every code object: ANY v_pk_mul / v_pk_fma /
    v_pk_add _f32 rejects it.  Round 2's failing kernel form (tools/probes/decfold_scalar_form.hip), compiled for gfx950 here WITH the
    feature (no GPU needed), must be flagged - with the narrower round-2 shape recognised -, every object of the library must be clean."""
    import glob
    import shutil
    import subprocess
    bh = _build_hip_module()
    # unit level: the disassembly parser on a hand-written listing (hi half read + SGPR->SGPR copy = hit; literal move or low-half broadcast = clean)
    bad = "0000000000001000 <k>:\n\ts_mov_b32 s31, s40   // 0\n\tv_pk_mul_f32 v[36:37], v[30:31], s[30:31] op_sel:[1,0] op_sel_hi:[0,1] // 1\n"
    lit = "0000000000001000 <k>:\n\ts_mov_b32 s35, 0.5   // 0\n\tv_pk_mul_f32 v[24:25], v[24:25], s[34:35] // 1\n"
    low = "0000000000001000 <k>:\n\ts_mov_b32 s13, s40   // 0\n\tv_pk_fma_f32 v[0:1], s[12:13], v[2:3], v[0:1] op_sel_hi:[0,1,1] // 1\n"
    assert len(bh.scan_disassembly(bad)) == 1 and "lat_decfold" in bh.scan_disassembly(bad)[0][2]
    assert len(bh.scan_disassembly(lit)) == 1 and "lat_decfold" not in bh.scan_disassembly(lit)[0][2] and len(bh.scan_disassembly(low)) == 1
    assert bh.scan_disassembly("0000000000001000 <k>:\n\tv_fma_f32 v0, v0, v2, s2 // 0\n\tv_pk_add_u16 v0, v1, v2 // 1\n") == []
    if shutil.which("hipcc") is None or not os.path.exists(bh.OBJDUMP):
        pytest.skip("hipcc / llvm-objdump not available")
    obj = str(tmp_path / "decfold_bad.o")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", os.path.join(ROOT, "tools", "probes", "decfold_scalar_form.hip"), "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    hits = bh.scan_object(obj)
    assert hits and all(h[0] == "decfold_scalar_form" for h in hits) and any("lat_decfold" in h[2] for h in hits), hits[:3]
    clean = str(tmp_path / "decfold_nopk.o")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + bh.NO_PACKED_F32 + ["-c", os.path.join(ROOT, "tools", "probes", "decfold_scalar_form.hip"), "-o", clean],
                       capture_output=True, text=True)
    assert r.returncode == 0 and bh.scan_object(clean) == [], "the build flag removes every packed-f32 instruction"
    objs = glob.glob(os.path.join(ROOT, "afford-motion_amd", "build", "*.o"))
    if not objs:
        pytest.skip("library objects not built")
    for o in objs:
        assert bh.scan_object(o) == [], f"{os.path.basename(o)} contains the fenced instruction shape"


def test_progress_slices_cover_the_chain():
    """`progress=True` (test.py:94-101) runs the native loop as chained slices: contiguous, complete, ~50 of them."""
    assert ffi.progress_slices(1000, False) == [(0, 1000)]
    for n in (1, 7, 50, 51, 500, 1000):
        sl = ffi.progress_slices(n, True)
        assert sl[0][0] == 0 and sl[-1][1] == n and len(sl) <= 50
        assert all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and all(j1 > j0 for j0, j1 in sl)


def test_evaluator_file_formats_round_trip(tmp_path):
    """ADM -> file -> AMDM hand-off (utils/evaluate.py:41-82, datasets/humanml3d.py:763-774) and the motion pickle; the glue
    values are pinned by the reference-generated golden."""
    from afm import io as aio
    g = golden("adm_to_amdm_glue")
    raw, mean, std, sigma = g["sample"], float(g["mean"]), float(g["std"]), float(g["sigma"])
    path = aio.save_pred_contact(str(tmp_path), "000021", 3, raw[0], mean=mean, std=std, sigma=sigma)
    assert path.endswith("H3D/pred_contact/000021-3.npy")
    stored = np.load(path)
    assert stored.shape == (1, 64, 6) and stored.dtype == np.float32
    np.testing.assert_allclose(stored[0], g["dist"].numpy()[0], rtol=1e-6, atol=1e-7)
    cond = aio.load_pred_contact(str(tmp_path), "M_000021", 3, sigma=sigma)          # dataset strips the mirror prefix
    np.testing.assert_allclose(cond[0], g["cond"].numpy()[0], rtol=1e-5, atol=1e-7)
    aio.save_pred_contact(str(tmp_path), "000022", 0, raw, mean=mean, std=std, sigma=sigma)   # k samples stay (k, N, J)
    assert np.load(os.path.join(tmp_path, "H3D/pred_contact/000022-0.npy")).shape == (2, 64, 6)
    motion = torch.randn(16, 263)
    x_mask = torch.zeros(16, dtype=torch.bool); x_mask[12:] = True
    p = aio.save_motion_sample(str(tmp_path), "000021", 3, text="a person walks", tokens=["a/DET"], motion=motion, x_mask=x_mask,
                               mean=torch.ones(263), std=torch.full((263,), 2.0))
    rec = aio.load_motion_sample(p)
    assert set(rec) == {"name", "text", "tokens", "motion", "m_len"} and rec["m_len"] == 12
    np.testing.assert_allclose(rec["motion"], motion.numpy() * 2.0 + 1.0, rtol=1e-6)


def test_all_four_task_configs_compose():
    """configs/task/*.yaml mirror the reference's four tasks (HumanML3D + HUMANISE, ADM + AMDM) with the keys the path reads."""
    for task, model, ov in (("contact_gen", "cdm", ["model.input_feats=6", "model.arch=Perceiver", "model.scene_model.pretrained_weight=''"]),
                            ("contact_motion_gen", "cmdm", ["model.data_repr=pos", "model.input_feats=66"]),
                            ("text_to_motion_contact_gen", "cdm", ["model.input_feats=6", "model.arch=Perceiver", "model.scene_model.use_scene_model=False"]),
                            ("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263"])):
        cfg = load_config(task, model, ov)
        assert float(cfg.task.train.lr) == 1e-4 and cfg.task.train.batch_size == 32 and cfg.task.dataset.num_points == 8192
        m = base.create_model(cfg, device="cpu")
        assert sum(p.numel() for p in m.parameters()) > 0
    humanise = load_config("contact_gen", "cdm", ["model.input_feats=6", "model.arch=Perceiver", "model.scene_model.pretrained_weight=''"])
    assert humanise.model.scene_model.use_color is True and hasattr(base.create_model(humanise, device="cpu"), "scene_model")


def test_shim_packages_fall_through_to_a_reference_checkout(tmp_path):
    """`utils` / `diffusion` / `models` shadow the reference's directories; modules that are NOT on the hot path (utils.io,
    utils.training, diffusion.resample ...) must still resolve to the reference checkout that follows on sys.path, and so must
    NAMES the shim modules do not define (`utils.misc.smplx_neutral_model` for utils/evaluate.py:15).  A fake checkout stands in
    for /root/reference (which does not exist on the GPU box)."""
    import subprocess
    import sys
    fake = tmp_path / "ref"
    for pkg, mod, body in (("utils", "io", "MARK = 'ref-utils-io'"), ("diffusion", "resample", "MARK = 'ref-resample'"),
                           ("utils", "misc", "MARK = 'ref-misc'\ncompute_repr_dimesion = 'must-not-win'\n"
                                             "def get_meshes_from_smplx():\n    return 'ref-meshes'"),
                           ("diffusion", "gaussian_diffusion", "def _extract_into_tensor(*a):\n    return 'reference code ran'\nMARK = 'ref-gd'"),
                           ("diffusion", "respace", "class _WrappedModel:\n    pass"),
                           ("utils", "registry", "OTHER = 1"),
                           ("models", "modules", "class CrossAttentionLayer:\n    pass\nclass NotAThing:\n    pass")):
        (fake / pkg).mkdir(parents=True, exist_ok=True)
        (fake / pkg / f"{mod}.py").write_text(body + "\n")
    code = ("import utils.io, diffusion.resample, utils.misc, models.base, diffusion.gaussian_diffusion as gd;"
            "assert utils.io.MARK == 'ref-utils-io' and diffusion.resample.MARK == 'ref-resample';"
            "assert callable(utils.misc.compute_repr_dimesion) and utils.misc.compute_repr_dimesion('h3d') == 263;"
            "from utils.misc import get_meshes_from_smplx; assert get_meshes_from_smplx() == 'ref-meshes';"
            "from models.modules import CrossAttentionLayer; assert CrossAttentionLayer.__module__ == 'models._reference_modules';"
            # negative cases: only the allow-listed, non-hot-path names may resolve to the checkout - a hot-path name the shim does not
            # define (or a typo) raises instead of silently running the reference's code
            "import diffusion.respace, utils.registry, models.modules\n"
            "for mod, name in ((gd, '_extract_into_tensor'), (gd, 'MARK'), (diffusion.respace, '_WrappedModel'), (utils.misc, 'MARK'),"
            " (utils.registry, 'OTHER'), (models.modules, 'NotAThing'), (models.modules, 'SceneMapEncoderX')):\n"
            "    try:\n        getattr(mod, name); raise SystemExit(f'{mod.__name__}.{name} resolved')\n"
            "    except AttributeError as e:\n        assert 'allow-list' in str(e), e\n"
            "assert 'afford-motion_amd' in models.base.__file__ and 'afford-motion_amd' in gd.__file__ and 'afford-motion_amd' in utils.misc.__file__;"
            "from models.modules import PositionalEncoding, TimestepEmbedder; print('fall-through ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "afford-motion_amd"), str(fake)]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and "fall-through ok" in r.stdout, r.stdout + r.stderr
    # without any checkout a missing name is a clear ImportError, not a crash at import of the shim
    code = ("import utils.misc\ntry:\n    from utils.misc import smplx_neutral_model\nexcept ImportError as e:\n    print('clean', e)")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "afford-motion_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout + r.stderr


def test_step_invariant_cache_keys_hold_their_tensors():
    """a cache keyed on (address, version, shape) alone matches the NEXT batch when the allocator recycles the
    freed address.  HeldKey keeps the keyed tensors alive, so an equal address always means the same live storage."""
    from afm._cache import HeldKey
    recycled = 0
    for _ in range(20):
        a = torch.randn(4, 64, 3)
        key = HeldKey((a, None), ("v", 1))
        assert key.matches((a, None), ("v", 1)) and key.matches((a.view(4, 64, 3), None), ("v", 1))     # same storage, same layout
        assert not key.matches((a, None), ("v", 2)) and not key.matches((a[:2], None), ("v", 1))
        ptr = a.data_ptr()
        del a                                   # the caller drops its batch; the key still owns it
        b = torch.randn(4, 64, 3)               # "next batch": same shape, fresh version counter
        recycled += int(b.data_ptr() == ptr)
        assert not key.matches((b, None), ("v", 1))
        b.add_(1.0)
        key2 = HeldKey((b,), ())
        b.mul_(2.0)                             # in-place edits invalidate through the version counter
        assert not key2.matches((b,), ())
    assert recycled == 0                        # the address cannot come back while the key lives


def test_default_noise_seed_is_fresh_per_call():
    """with seed=None (how test.py:95-102 calls p_sample_loop inside its k_sample loop) every call must draw new noise,
    reproducibly from torch.manual_seed, and identically on every rank (no per-process hash randomisation)."""
    cfg = load_config("text_to_motion_contact_motion_gen", "cmdm", [])
    torch.manual_seed(2023)
    d1 = base.create_gaussian_diffusion(cfg)
    s = [d1._fresh_seed("_sample_calls") for _ in range(4)] + [d1._fresh_seed("_loss_calls")]
    assert len(set(s)) == 5 and all(0 <= v < 2**63 for v in s)
    torch.manual_seed(2023)
    d2 = base.create_gaussian_diffusion(cfg)
    assert [d2._fresh_seed("_sample_calls") for _ in range(4)] + [d2._fresh_seed("_loss_calls")] == s
    torch.manual_seed(7)
    assert base.create_gaussian_diffusion(cfg)._fresh_seed("_sample_calls") != s[0]


def test_missing_pretrained_scene_weights_raise(tmp_path):
    """reference pointtransformer.py:203-205 raises when the frozen backbone's weights are missing."""
    ov = ["model.input_feats=6", "model.arch=Perceiver", "task.dataset.use_color=True"]
    with pytest.raises(FileNotFoundError, match="pretrained point-transformer"):
        base.create_model(load_config("text_to_motion_contact_gen", "cdm", ov + [f"model.scene_model.pretrained_weight={tmp_path}/nope.pth"]),
                          device="cpu")


def test_clip_text_model_is_not_a_submodule(tmp_path, monkeypatch):
    """the lazily loaded CLIP model must not change state_dict() keys after the first text encode."""
    import sys
    import types
    fake = types.ModuleType("clip")

    class _Clip(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb = torch.nn.Embedding(50000, 512)

        def encode_text(self, tok):
            return self.emb(tok.clamp(max=49999)).mean(1)

    fake.load = lambda name, device="cpu", jit=False: (_Clip(), None)
    fake.tokenize = lambda texts, context_length=77, truncate=True: torch.ones(len(texts), context_length, dtype=torch.long)
    monkeypatch.setitem(sys.modules, "clip", fake)
    model = base.create_model(load_config("text_to_motion_contact_motion_gen", "cmdm", ["model.data_repr=h3d", "model.input_feats=263"]), device="cpu")
    before = set(model.state_dict())
    feat = model.encode_text({"c_text": ["a person walks", "sits down"]})
    assert feat.shape == (2, 512)
    assert set(model.state_dict()) == before and not any("clip" in n for n, _ in model.named_modules())


def test_param_version_sees_tensors_replaced_through_a_child_module():
    """the weight packs and condition caches are keyed by `_param_version`, whose tensor list is cached.  In-place writes bump
    `_version`; tensors REPLACED behind the top-level module (a child's `.to()` / `.double()`, `load_state_dict(assign=True)`,
    `layer.weight = nn.Parameter(...)`) must change the version too."""
    import torch.nn as nn
    from afm.cmdm import _param_version
    m = nn.Sequential(nn.Linear(4, 4), nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4)))
    seen = [_param_version(m)]
    assert _param_version(m) == seen[0]

    def changed(what):
        v = _param_version(m)
        assert v not in seen, what
        assert _param_version(m) == v
        seen.append(v)
    with torch.no_grad():
        m[0].weight.add_(1)
    changed("in-place write")
    m[1][0].weight = nn.Parameter(torch.zeros(4, 4))
    changed("parameter object replaced on a child")
    m[1].double()
    changed("child moved / cast")
    m[1].load_state_dict({k: v.clone() for k, v in m[1].state_dict().items()}, assign=True)
    changed("load_state_dict(assign=True) on a child")
