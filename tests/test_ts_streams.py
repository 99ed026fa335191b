"""Many streams to finished frames through the TypeScript host
(PostPool.replaceBackgrounds and Video.processStreams in ts/segment.ts) over the
Node-API addon: the same bytes as the Python host."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_ref as ref  # noqa: E402

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
def test_node_streams_match_python_host(addon_built, pkg, synthetic, tmp_path):
    """Two calls over streams 3, 0, 1 with a shared colour, a shared blur and a refined
    colour, as RGB frames and as NV12: replaceBackgrounds and processStreams (TS) ==
    replace_backgrounds and process_streams (Python), bit for bit."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h, w = 240, 320
    frames = np.stack([synthetic.make_frame(890 + i, h, w, 3) for i in range(5)])
    y, uv = ref.pack(ref.BT709_LIMITED, frames)
    fp, yp, uvp, op = tmp_path / "frames.bin", tmp_path / "y.bin", tmp_path / "uv.bin", tmp_path / "streams"
    frames.tofile(fp)
    y.tofile(yp)
    uv.tofile(uvp)
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "run_streams.js"), str(fp), str(yp), str(uvp),
                          str(h), str(w), str(op), "bf16x2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info == {"dupRejected": True, "countRejected": True, "nvCountRejected": True}
    got_rgba = np.fromfile(str(op) + "_rgba.u8", np.uint8).reshape(5, h, w, 4)
    got_y = np.fromfile(str(op) + "_y.u8", np.uint8).reshape(5, h, w)
    got_uv = np.fromfile(str(op) + "_uv.u8", np.uint8).reshape(5, h // 2, w)
    with pkg.Session(dtype="bf16x2", max_batch=3, max_frame_h=h, max_frame_w=w) as s, \
            pkg.PostPool(s, 4) as rgb_pool, pkg.PostPool(s, 4) as nv_pool:
        colour, blur, refined = pkg.Background(s), pkg.Background(s), pkg.Background(s)
        colour.set_color(10, 200, 90)
        blur.set_blur(5, 2.0)
        refined.set_color(200, 30, 60)
        refined.set_refine(2, 16.0)
        video = pkg.Video(s, "bt709")
        rgba, ys, uvs = [], [], []
        for ids, bgs, a, b in (([3, 0, 1], [colour, blur, colour], 0, 3), ([1, 3], [refined, blur], 3, 5)):
            rgba.append(rgb_pool.replace_backgrounds(ids, frames[a:b], bgs))
            oy, ouv = video.process_streams(y[a:b], uv[a:b], nv_pool, ids, bgs)
            ys.append(oy)
            uvs.append(ouv)
        with pytest.raises(pkg.VssError):
            rgb_pool.replace_backgrounds([2, 2], frames[0:2], [colour, blur])
    want_rgba, want_y, want_uv = np.concatenate(rgba), np.concatenate(ys), np.concatenate(uvs)
    assert np.array_equal(got_rgba, want_rgba), f"{(got_rgba != want_rgba).sum()} RGBA bytes differ"
    assert np.array_equal(got_y, want_y), f"{(got_y != want_y).sum()} Y bytes differ"
    assert np.array_equal(got_uv, want_uv), f"{(got_uv != want_uv).sum()} UV bytes differ"
    assert not np.array_equal(got_rgba[..., :3], frames)  # backgrounds were put in
