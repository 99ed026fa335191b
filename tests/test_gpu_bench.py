"""GPU test of bench.py's plain run: `--steps` timed steps and nothing beside
them, a result line with the headline fields only, and `--dump-outputs DIR`
writing the masks the last timed step computed — bitwise what the same
frames give through Session.segment_frames (same kernels, same weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"median_step_ms", "roofline", "kernels", "batch_sweep", "latency", "cpu_baseline", "mask_max_abs_err",
             "post", "host_path", "ts_path"}


def test_plain_run_prints_the_headline_and_dumps_the_last_step(pkg, synthetic, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    steps, warmup = 6, 5  # more steps than slots: the last step's buffer is not the first one written
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert HEADLINE <= set(d), sorted(d)
    assert not FULL_ONLY & set(d), sorted(FULL_ONLY & set(d))
    assert d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "frames/s" and d["higher_is_better"]
    # value and ms_per_step describe the same window: 8 frames per step
    assert d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / 8 - 1) < 1e-2, (d["value"], d["ms_per_step"])
    assert os.listdir(tmp_path) == ["masks.npy"]
    got = np.load(tmp_path / "masks.npy")
    assert got.dtype == np.float32 and got.shape == (8, 144 * 256)
    with pkg.Session(max_batch=8, max_frame_h=480, max_frame_w=640) as s:
        want, _, _ = s.segment_frames(synthetic.make_batch(8, 480, 640, 3))
    assert np.array_equal(got, want)
