"""bench.py end to end on a small mesh: a plain run prints the headline of exactly --steps timed V-cycles and nothing of
--full, and --dump-outputs writes the iterate of the last timed cycle, which is not degenerate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_and_dump(tmp_path):
    cells, steps = 32, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--cells", str(cells), "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == steps and line["dtype"] == "f64" and line["unit"] == "DoF/s" and line["higher_is_better"]
    n = (cells + 1) ** 3
    assert line["config"]["global_dofs"] == n
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / n - 1) < 1e-9
    for key in ("roofline", "other_kernels", "cpu_baseline", "north_star_512cubed_smoother"):
        assert key not in line
    x = np.load(tmp_path / "out" / "x.npy")
    assert x.dtype == np.float64 and x.shape == (n,) and np.all(np.isfinite(x))
    # the right-hand side is a load f in [0, 1): the iterate approaches the discrete solution of -div grad u = f (max ~0.03),
    # it does not decay to zero
    assert 1e-3 < np.abs(x).max() < 1.0
