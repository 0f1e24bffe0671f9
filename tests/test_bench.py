"""bench.py's plain run on the GPU: exactly --steps timed frames, the headline only, and --dump-outputs writing the
last timed frame's results (float32, at most 64 MB) identically from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("log_odds", "occupancy", "occupancy_grid", "hits", "miss", "bbox_id")


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_bench_plain_run_times_the_given_steps_and_dumps_the_last_frame(tmp_path):
    line = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2 and line["repetitions"]["n"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 1.0) < 1e-6
    assert "stage_ms" not in line and "with_h2d" not in line and line["cpu_baseline"] is None   # --full only
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in OUTPUTS}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in OUTPUTS)
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in OUTPUTS) <= 64 << 20
    assert got["hits"].sum() > 0 and (got["bbox_id"] >= 0).any() and np.isfinite(got["log_odds"]).all()
    _plain_run(tmp_path / "b")
    for n in OUTPUTS:
        assert np.array_equal(np.load(tmp_path / "b" / f"{n}.npy"), got[n]), n
