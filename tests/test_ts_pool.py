"""The post chain over many streams through the TypeScript host (PostPool in
ts/segment.ts) over the Node-API addon: the same bytes as the Python host."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = os.path.join(ROOT, "video-stream-segmenetation_amd", "ts")
NODE = shutil.which("node")


@pytest.fixture(scope="module")
def addon_built(pkg):
    if not NODE or not os.path.isdir("/usr/include/node"):
        pytest.skip("node / node headers not available")
    pkg.build()
    subprocess.run(["make", "-s", "-C", os.path.join(TS, "addon")], check=True)


@pytest.mark.gpu
def test_node_pool_matches_python_host(addon_built, pkg, synthetic, tmp_path):
    """Three calls over streams 3, 0, 1, a reset of one stream, then reset() and a
    knob change: PostPool.segment (TS) == PostPool.segment (Python), bit for bit."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h, w = 240, 320
    frames = np.stack([synthetic.make_frame(880 + i, h, w, 3) for i in range(5)])
    fp, op = tmp_path / "frames.bin", tmp_path / "pool"
    frames.tofile(fp)
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "run_pool.js"), str(fp), str(h), str(w), "3",
                          str(op), "bf16x2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info == {"width": 256, "height": 144, "count": 8, "dupRejected": True, "rangeRejected": True,
                    "countRejected": True}
    got_a = np.fromfile(str(op) + ".f32", np.float32).reshape(8, 144 * 256)
    got_u = np.fromfile(str(op) + ".u8", np.uint8).reshape(8, 144 * 256)
    with pkg.Session(dtype="bf16x2", max_batch=3, max_frame_h=h, max_frame_w=w) as s, pkg.PostPool(s, 4) as pool:
        parts = [pool.segment([3, 0, 1], frames[0:3]), pool.segment([1, 3], frames[3:5])]
        pool.reset(3)
        parts.append(pool.segment([3], frames[0:1]))
        with pytest.raises(pkg.VssError):
            pool.segment([2, 2], frames[0:2])
        pool.reset()
        pool.set_config(USE_BILATERAL=0, GAMMA=1.0)
        parts.append(pool.segment([0, 2], frames[1:3]))
    want_a = np.concatenate([p[0] for p in parts])
    want_u = np.concatenate([p[1] for p in parts])
    assert np.array_equal(got_u, want_u), f"{(got_u != want_u).sum()} alpha bytes differ"
    assert np.array_equal(got_a, want_a)
    assert np.array_equal(got_u[0], got_u[5])  # stream 3 after its reset: frame 0 is a first frame again
