"""bench.py as the driver runs it: a plain run (no --full) prints the headline line and nothing it has to measure separately,
and --dump-outputs writes what the timed path returned, from the same seeded inputs in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _plain_run(out_dir, steps=3):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "S", "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
        assert not {"roofline", "roofline_mfma", "cpu_baseline", "parity", "other_configs"} & set(line)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["dpv.npy", "refined_dpv.npy"] and files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and x.shape[1] == 64 and np.isfinite(x).all()
        # same arguments, same inputs: two runs agree to the parity gate (tests/conftest.py MAX_ABS_TOL)
        assert np.abs(x - y).max() <= 1e-3
