"""Writes tests/golden/h3d_recover_from_ric.npz: the reference's own recover_from_ric on seeded HumanML3D-style features.

    python tools/make_h3d_golden.py /path/to/reference

Runs on the development machine only (it needs a checkout of the reference; no test imports it).  The reference keeps `qinv`, `qrot`,
`recover_root_rot_pos` and `recover_from_ric` in utils/visualize.py, a module whose other imports (renderers, mesh libraries) are not
needed here and may be absent: the four function definitions are cut out of the parsed file and compiled on their own, with `torch` as
their only global.  They are evaluated in float32 and - with torch's default dtype switched, since they allocate with torch.zeros - in
float64, on the same de-normalised features u [2, 9, 263].  The file holds `u` (float64, every value a float32), `pos32` and `pos64`
[2, 9, 22, 3]."""
import ast
import os
import sys

import numpy as np
import torch

WANTED = ("qinv", "qrot", "recover_root_rot_pos", "recover_from_ric")
SHAPE = (2, 9, 263)
SEED = 20240607
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "h3d_recover_from_ric.npz")


def load_functions(reference_root):
    path = os.path.join(reference_root, "utils", "visualize.py")
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    if sorted(d.name for d in defs) != sorted(WANTED):
        raise SystemExit(f"{path}: expected the functions {WANTED}, found {[d.name for d in defs]}")
    scope = {"torch": torch}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), scope)
    return scope["recover_from_ric"]


def features():
    """realistic magnitudes: a rotation velocity of a few hundredths of a radian per frame, root velocities of centimetres, a root height
    near one metre, local joint offsets within a metre; the remaining columns (never read by the recovery) plain noise"""
    g = torch.Generator().manual_seed(SEED)
    u = torch.randn(SHAPE, generator=g, dtype=torch.float32)
    u[..., 0] *= 0.05
    u[..., 1:3] *= 0.03
    u[..., 3] = 0.9 + 0.05 * u[..., 3]
    u[..., 4:67] *= 0.4
    return u


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    recover = load_functions(sys.argv[1])
    u = features()
    out = {}
    for name, dtype in (("pos32", torch.float32), ("pos64", torch.float64)):
        saved = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            out[name] = recover(u.to(dtype).clone(), 22).numpy()
        finally:
            torch.set_default_dtype(saved)
        assert out[name].dtype == (np.float32 if dtype == torch.float32 else np.float64) and out[name].shape == SHAPE[:2] + (22, 3)
    np.savez(OUT, u=u.double().numpy(), **out)
    err = np.abs(out["pos32"].astype(np.float64) - out["pos64"]).max()
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): max|pos64| = {np.abs(out['pos64']).max():.4f}, max|pos32 - pos64| = {err:.3e}")


if __name__ == "__main__":
    main()
