"""DDIM on the host (no GPU): the product's DDIM rows reproduce the reference's ddim_sample / ddim_reverse_sample goldens bit for bit
when put through the update expression in CPU float32; the C ABI declares and mirrors the new DDIM surface; the API matches the
reference's signatures."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from afm import ffi
from afm import diffusion as gd
from conftest import ROOT, golden


def _diffusion(steps=1000, respacing=None):
    return gd.SpacedDiffusion(use_timesteps=gd.space_timesteps(steps, respacing or [steps]),
                              betas=gd.get_named_beta_schedule("cosine", steps), model_mean_type=gd.ModelMeanType.START_X,
                              model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def _update(x0, x, noise, rows, t):
    """The reference's float32 expression (gaussian_diffusion.py:569-585), one operation at a time, on the product's rows of timestep t."""
    a, b, c, d = (r[t] for r in (rows.a, rows.b, rows.c, rows.d))
    eps = (a * x - x0) / b
    mean = x0 * c + d * eps
    return mean if rows.sigma is None else mean + rows.sigma[t] * noise


@pytest.mark.parametrize("tt", [999, 500, 1, 0])
def test_ddim_rows_reproduce_the_reference_step(tt):
    g = golden(f"cmdm_ddim_sample_t{tt}")
    rows = _diffusion().ddim_tables("cpu", float(g["eta"]))
    got = _update(g["pred_xstart"], g["x"], g["noise"], rows, tt)
    assert torch.equal(got, g["sample"]), (got - g["sample"]).abs().max()


def test_ddim_reverse_rows_reproduce_the_reference_step():
    g = golden("cmdm_ddim_reverse_t500")
    rows = _diffusion().ddim_tables("cpu", reverse=True)
    assert rows.sigma is None
    got = _update(g["pred_xstart"], g["x"], None, rows, 500)
    assert torch.equal(got, g["sample"]), (got - g["sample"]).abs().max()


def test_ddim_rows_without_noise_term_at_eta_zero():
    d = _diffusion(1000, "ddim50")
    assert d.ddim_tables("cpu", 0.0).sigma is None
    s = d.ddim_tables("cpu", 1.0).sigma
    assert s[0] == 0 and bool((s[1:] > 0).all())
    assert d.ddim_tables("cpu", 1.0) is d.ddim_tables("cpu", 1.0)          # built once per (device, eta)


def test_ddim_exports_declared_and_struct_mirrored(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(afm_\w+)\s*\(", hdr, re.M))
    new = {"afm_ddim_step", "afm_ddim_sched_scratch_bytes", "afm_cmdm_ddim_loop_range", "afm_cdm_ddim_loop_range"}
    assert new <= declared and new <= set(ffi.EXPORTS)
    assert "#define AFM_ABI_VERSION 7" in hdr
    if os.path.exists(ffi.lib_path()):
        lib = ctypes.CDLL(ffi.lib_path())
        for name in new:
            assert hasattr(lib, name), name
        assert ffi.load().afm_ddim_sched_scratch_bytes(50, 32) > ffi.load().afm_cmdm_sched_scratch_bytes(50, 32) > 0
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(afm_ddim_rows));']
    lines += [f'  printf("{f} %zu\\n", offsetof(afm_ddim_rows, {f}));' for f, _ in ffi.DdimRows._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "ddim_layout.c", tmp_path / "ddim_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(ffi.DdimRows)
    for f, _ in ffi.DdimRows._fields_:
        assert int(out[f]) == getattr(ffi.DdimRows, f).offset, f


def test_ddim_api_signatures_match_the_reference():
    """Positional / keyword parameters and defaults of the four DDIM methods equal the reference's (read from its source, not imported:
    importing it would replace the product's `models` / `diffusion` packages in this process).  The product's keyword-only extras are
    p_sample_loop's (step_noise, seed, sample_index0, snapshots)."""
    import ast
    ref = "/root/reference/diffusion/gaussian_diffusion.py"
    if not os.path.exists(ref):
        pytest.skip("reference checkout not present")
    tree = ast.parse(open(ref).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GaussianDiffusion")
    methods = {f.name: f for f in cls.body if isinstance(f, ast.FunctionDef)}
    for name in ("ddim_sample", "ddim_reverse_sample", "ddim_sample_loop", "ddim_sample_loop_progressive"):
        args = methods[name].args
        names = [a.arg for a in args.args]
        defaults = [inspect.Parameter.empty] * (len(names) - len(args.defaults)) + [ast.literal_eval(d) for d in args.defaults]
        got = [p for p in inspect.signature(getattr(gd.GaussianDiffusion, name)).parameters.values() if p.kind != p.KEYWORD_ONLY]
        assert [(p.name, p.default) for p in got] == list(zip(names, defaults)), name
