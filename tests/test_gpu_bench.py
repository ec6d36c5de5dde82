"""bench.py at N = 1: the plain run (headline only) and `--dump-outputs`, whose file must be the same on every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(args, timeout=600):
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, cwd=ROOT, timeout=timeout)


@pytest.mark.parametrize("args", [["--steps", "1"], ["--warmup", "-2"]])
def test_bench_rejects_step_counts_no_schedule_can_hold(args):
    r = _bench(args, timeout=120)
    assert r.returncode == 2 and ("--steps" in r.stderr or "--warmup" in r.stderr), r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_bench_dumps_the_same_outputs_every_run(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        out = tmp_path / f"run{i}"
        r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out)])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
        found = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(found) == 1, r.stdout[-3000:]
        lines.append(json.loads(found[0]))
        assert sorted(os.listdir(out)) == ["sample.npy"]
        dumps.append(np.load(out / "sample.npy"))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["unit"] == "steps/s" and line["dtype"] == "f32"
        assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-2
        for key in ("roofline", "cpu_baseline", "sample_latency", "alt_gemm_modes", "other_scaling_mode", "secondary", "final_all_gather"):
            assert line[key] is None, key                   # measured with --full only
    a, b = dumps
    assert a.dtype == np.float32 and a.shape == (32, 196, 263) and np.isfinite(a).all()
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_bench_times_more_steps_than_one_schedule_holds(tmp_path):
    """K > 1000 (the diffusion's own step count) runs as chained loop calls: the line still reports exactly K timed steps."""
    r = _bench(["--gpus", "1", "--steps", "1001", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 1001 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-2
    x = np.load(tmp_path / "sample.npy")
    assert x.shape == (32, 196, 263) and np.isfinite(x).all()
