"""The CMDM workspace-size functions on the host (no GPU): pure host code, pinned byte for byte to a table.

tests/cmdm_workspace_bytes.json was written by a library built from commit a0a3f5a ("Impute known contact values inside the native CDM
sampling loops"), the parent of the commit that folded the guided branches into one list - not by the code under test.  A workspace byte
that moves shows up here before any GPU run."""
import ctypes
import json
import os

import pytest
import torch

from afm import ffi

from conftest import ROOT

SHAPES = ((0, 16), (1, 1), (3, 15), (3, 16), (32, 196))
STREAMS = (0, 2, 3)
# the model's pack (configs/model/cmdm.yaml, 'h3d' motion): what the sizes depend on, every tensor a dummy non-null pointer
PACK = dict(d=512, heads=8, ff=1024, n_layers=5, motion_dim=263, n_cond=129, n_timesteps=1000, motion_adapter_kpad=272)
CFG = {"cfg_compact": (1, 1, 0), "cfg_force_masked": (1, 1, ffi.CFG_FORCE_MASKED), "cfg_text": (1, 0, 0), "cfg_pc": (0, 1, 0)}      # drop_text, drop_pc, flags
CFG2 = {"cfg2_first0": (0, 0), "cfg2_first1": (1, 0), "cfg2_first0_force_masked": (0, ffi.CFG_FORCE_MASKED),
        "cfg2_first1_force_masked": (1, ffi.CFG_FORCE_MASKED)}                                                                          # first, flags


def pack(p):
    w = ffi.CmdmWeights()
    for k, v in PACK.items():
        setattr(w, k, v)
    w.motion_adapter_w = w.motion_layer_w = w.time_table = w.pos_table = p
    return w


def sizes(lib):
    """every size function over the grid -> {"single": {"B,L": [plain, cfg, cfg2]}, "loop": {"B,L,n_streams": {form: bytes}}}"""
    buf = torch.zeros(8)
    p = buf.data_ptr()
    w = ctypes.byref(pack(p))
    out = {"single": {}, "loop": {}}
    for B, L in SHAPES:
        out["single"][f"{B},{L}"] = [lib.afm_cmdm_workspace_bytes(w, B, L), lib.afm_cmdm_cfg_workspace_bytes(w, B, L),
                                     lib.afm_cmdm_cfg2_workspace_bytes(w, B, L)]
        for n in STREAMS:
            row = {"unguided": lib.afm_cmdm_loop_workspace_bytes(w, B, L, n)}
            for name, (dt, dp, fl) in CFG.items():
                row[name] = lib.afm_cmdm_cfg_loop_workspace_bytes(w, B, L, n, ctypes.byref(ffi.CfgArgs(p, dt, dp, fl, None)))
            for name, (first, fl) in CFG2.items():
                row[name] = lib.afm_cmdm_cfg2_loop_workspace_bytes(w, B, L, n, ctypes.byref(ffi.Cfg2Args(p, p, first, fl)))
            out["loop"][f"{B},{L},{n}"] = row
    return out


def test_workspace_sizes_match_the_parent_builds_table():
    if not os.path.exists(ffi.lib_path()):
        pytest.skip("libafm_hip.so not built (run python afford-motion_amd/build_hip.py)")
    want = json.load(open(os.path.join(ROOT, "tests", "cmdm_workspace_bytes.json")))
    got = sizes(ffi.load())
    assert set(got["single"]) == set(want["single"]) and set(got["loop"]) == set(want["loop"])
    for key, row in want["single"].items():
        assert got["single"][key] == row, key
    for key, row in want["loop"].items():
        assert got["loop"][key] == row, key
    # the table is not degenerate: no error code in it (an empty batch needs 0 bytes), and the forms differ where the layouts do
    big = want["loop"]["32,196,2"]
    assert all(v >= 0 for row in want["loop"].values() for v in row.values()) and all(v >= 0 for row in want["single"].values() for v in row)
    assert big["unguided"] < big["cfg_compact"] < big["cfg_force_masked"] == big["cfg_text"] == big["cfg_pc"] < big["cfg2_first0"]
    assert big["cfg2_first0"] == big["cfg2_first1"] < big["cfg2_first0_force_masked"]
