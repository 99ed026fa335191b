"""Virtual backgrounds through the TypeScript host (Background and
PostChain.backgroundFrames in ts/segment.ts) over the Node-API addon: the same
bytes as the Python host."""
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
def test_node_backgrounds_match_python_host(addon_built, pkg, synthetic, tmp_path):
    """Colour and blur, n=4 at 240x320, each from the first frame of a stream:
    Background / backgroundFrames (TS) == Background / replace_background (Python)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, h, w = 4, 240, 320
    frames = np.stack([synthetic.make_frame(720 + i, h, w, 3) for i in range(n)])
    fp, op = tmp_path / "frames.bin", tmp_path / "bg"
    frames.tofile(fp)
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "run_background.js"), str(fp), str(n), str(h),
                          str(w), "3", str(op), "bf16x2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info == {"width": w, "height": h, "count": n, "badBlurRejected": True}
    with pkg.Session(dtype="bf16x2", max_batch=n, max_frame_h=h, max_frame_w=w) as s:
        chain = pkg.PostChain(s)
        bg = pkg.Background(s)
        bg.set_color(10, 200, 90)
        want_colour = chain.replace_background(frames, bg)
        chain.reset()
        bg.set_blur(7, 2.5)
        want_blur = chain.replace_background(frames, bg)
    for name, want in (("colour", want_colour), ("blur", want_blur)):
        got = np.fromfile(f"{op}_{name}.u8", np.uint8).reshape(n, h, w, 4)
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"
    assert np.all(want_colour[..., 3] == 255) and not np.array_equal(want_colour, want_blur)
