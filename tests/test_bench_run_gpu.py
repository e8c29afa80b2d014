"""A plain `python bench.py` run: the headline line alone, --steps timed steps, and --dump-outputs writing what the last
timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(util.REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "training commits/sec (FIRA default config)" and line["unit"] == "commits/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 32 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]   # batch 32 per step
    for k in ("roofline", "decode", "cpu_baseline", "kernel_time_ms_per_step", "detail"):   # --full only
        assert k not in line, k

    assert sorted(os.listdir(out)) == ["loss.npy"]
    arr = np.load(out / "loss.npy")
    assert arr.dtype == np.float64 and arr.shape == (3,) and np.isfinite(arr).all()
    loss, loss_sum, n_tok = arr.tolist()
    assert n_tok > 0 and abs(loss - loss_sum / n_tok) <= 1e-6 * loss
    assert abs(loss - line["config"]["loss"]) <= 1e-5 * loss
