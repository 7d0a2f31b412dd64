"""bench.py on one GPU, the default workload: a plain run prints the headline and nothing that takes runs of its own;
--full adds the per-kernel times, the roofline and the std layer (the other configs and the CPU baseline, minutes of work,
are left out here), and both compute the same layer output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _run(tmp_path, name, extra):
    env = dict(os.environ, EGC_BENCH_DETAIL=str(tmp_path / f"{name}_detail.json"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--dump-outputs", str(tmp_path / name)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in CONTRACT:
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["warmup"] == 2 and line["unit"] == "edges/s"
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / line["config"]["e_eff"] - 1) < 1e-4
    out = np.load(tmp_path / name / "layer_out_rows_sample.npy")
    ids = np.load(tmp_path / name / "layer_out_row_ids.npy")
    assert out.shape == (len(ids), 128) and out.dtype == np.float32 and np.isfinite(out).all()
    return line, out


def test_plain_run_is_the_headline_and_full_adds_the_side_figures(tmp_path):
    plain, out_plain = _run(tmp_path, "plain", [])
    assert plain["roofline"] is None and plain["cpu_baseline"] is None
    for k in ("kernels_ms", "layer_frac", "ms_per_step_median_of_5_regions", "std_layer", "other_configs"):
        assert k not in plain, k

    full, out_full = _run(tmp_path, "full", ["--full", "--no-other-configs", "--no-cpu-baseline"])
    assert full["roofline"]["achieved"] > 0 and full["roofline"]["frac"] > 0
    assert set(full["kernels_ms"]) >= {"basis_gemm", "aggregate_combine", "layer_forward"}
    assert full["ms_per_step_median_of_5_regions"] > 0 and "error" not in full["std_layer"]
    assert "other_configs" not in full and full["cpu_baseline"] is None
    np.testing.assert_allclose(out_full, out_plain, rtol=0, atol=1e-5 * max(1.0, float(np.abs(out_plain).max())))
