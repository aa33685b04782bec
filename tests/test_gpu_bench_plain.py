"""A plain `bench.py` run (no --full) on the GPU box: exactly K timed steps, the result line's headline fields and nothing of the side
passes; `--dump-outputs DIR` writes the packed detections of the last timed step, the same arrays from two runs with the same flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--clips", "2", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.lstrip().startswith("{") and '"metric"' in l]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    d = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]
    assert not {"roofline", "roofline_im2col", "extras", "cpu_baseline", "parity"} & set(d)     # --full only
    a = np.load(tmp_path / "a" / "detections.npy")
    assert a.dtype == np.float32 and a.shape[0] == 2 and a.shape[2] == 40 and np.isfinite(a).all()
    assert int((a[..., 7] > 0).sum()) == d["config"]["detections_last_step"]
    _bench(tmp_path / "b")
    assert np.array_equal(a, np.load(tmp_path / "b" / "detections.npy"))          # seeded inputs: same flags, same outputs
