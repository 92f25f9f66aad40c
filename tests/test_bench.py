"""bench.py's plain run: the result line's headline fields, no leg of --full, and --dump-outputs writing the last timed step's outputs, the same
from one run to the next (fixed engine seed and action pool)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    # a fresh child process per run (never an exec of this one, which may have touched the GPU)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    r = _bench(tmp_path / "a")
    assert r["steps"] == 7 and r["warmup"] == 3 and r["n_gpus"] == 1
    assert r["unit"] == "env-steps/s" and r["higher_is_better"] is True and r["dtype"] == "f32" and "horizontal-locomotion" in r["metric"]
    assert r["ms_per_step"] > 0 and abs(r["value"] - 4096 / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-6
    assert "cpu_baseline" not in r and r["config"]["vec_env_step_env_steps_per_s"] is None and "manipulation_env_steps_per_s" not in r["config"]
    shapes = {"obs": (4096, 64), "states": (4096, 93), "rew": (4096,), "resets": (4096,), "extras": (13,)}
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in shapes}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in shapes)
    for k, s in shapes.items():
        assert a[k].shape == s and a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
    assert np.abs(a["obs"]).max() <= 5.0 and a["obs"].std() > 0 and set(np.unique(a["resets"])) <= {0.0, 1.0}
    _bench(tmp_path / "b")
    for k in shapes:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy")), k
