"""bench.py at N = 1: a plain run prints the headline line only, and --dump-outputs writes the last timed step's
top-k, the same from run to run (seeded inputs, exact top-k)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def _bench(steps, dump_dir):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", "32", "--gallery", "100000", "--dump-outputs", str(dump_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_headline_and_dumped_outputs(tmp_path):
    d = _bench(3, tmp_path / "a")
    assert set(d) == HEADLINE, sorted(set(d) ^ HEADLINE)      # the side measurements only run with --full
    assert d["steps"] == 3 and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["config"]["query_batch_per_gpu"] == 32 and d["config"]["gallery_rows"] == 100000
    assert abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    val = np.load(tmp_path / "a" / "topk_values.npy")
    idx = np.load(tmp_path / "a" / "topk_indices.npy")
    assert val.dtype == np.float32 and idx.dtype == np.float64 and val.shape == idx.shape == (32, 10)
    assert np.all(np.isfinite(val)) and np.all(np.abs(val) <= 1.0 + 1e-5) and np.all(np.diff(val, axis=1) <= 0)
    assert np.all(idx == np.round(idx)) and idx.min() >= 0 and idx.max() < 100000
    assert all(len(set(row)) == 10 for row in idx.tolist())
    # same arguments but the step count: same inputs, so the last step computes the same result
    _bench(1, tmp_path / "b")
    for name in ("topk_values.npy", "topk_indices.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
