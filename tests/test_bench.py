"""GPU: bench.py's plain run and ``--dump-outputs`` on a small workload (config[1], a 1080p m1 frame)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_map(tmp_path):
    """a plain run prints the headline line without what ``--full`` adds; ``--dump-outputs`` writes the last timed step's depth map
    and coarse prediction as float32, and a second process with the same arguments writes the same arrays"""
    maps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "v1_dav2s_1080p_m1", "--steps", "2",
                            "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][-1])
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "depth maps/s"
        assert not {"roofline", "cpu_baseline", "alt", "operating_point"} & set(line), sorted(line)
        depth, coarse = np.load(d / "depth.npy"), np.load(d / "coarse_prediction.npy")
        assert depth.dtype == coarse.dtype == np.float32 and list(depth.shape) == line["config"]["out_shape"], (depth.dtype, depth.shape)
        assert np.isfinite(depth).all() and depth.max() > 0
        maps.append((depth, coarse))
    for a, b in zip(*maps):
        np.testing.assert_array_equal(a, b)
