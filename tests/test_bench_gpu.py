"""bench.py's plain line and --dump-outputs on the GPU: a plain run prints the headline alone, --steps sets the number of
timed steps, and two runs with the same arguments write the same outputs of their last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.stdout[-1000:], r.stderr[-1000:])
    return json.loads(lines[-1])


def test_plain_line_and_its_dumped_outputs_repeat(tmp_path):
    runs = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for out in runs:
        assert out["steps"] == 3 and out["n_gpus"] == 1 and out["refused_frac"] == 0.0 and out["ms_per_step"] > 0
        assert abs(out["value"] - 8192 * 3 / (out["ms_per_step"] * 3e-3)) / out["value"] < 1e-3
        assert not {"secondary", "cpu_baseline", "bit_exact_vs_oracle", "gather"} & set(out), sorted(out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["imdct_status.npy", "overlap.npy", "pcm.npy", "status.npy"]
    total = 0
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64), (name, x.dtype)
        assert np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64e6
    pcm = np.load(tmp_path / "a" / "pcm.npy")
    assert pcm.shape == (2048, 4096) and np.abs(pcm).max() > 0
    assert not np.load(tmp_path / "a" / "status.npy").any() and not np.load(tmp_path / "a" / "imdct_status.npy").any()
