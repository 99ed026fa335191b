"""Branding layers through the TypeScript host (Background.setLayers /
setPrivacy in ts/segment.ts) over the Node-API addon: the same bytes as the C
path behind the Python host."""
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


def test_ts_host_declares_the_layer_calls():
    """No GPU: the generated module carries the methods and the addon's source the entry points."""
    js = open(os.path.join(TS, "segment.js")).read()
    cc = open(os.path.join(TS, "addon", "vss_napi.cc")).read()
    for name in ("setLayers", "setPrivacy"):
        assert f"  {name}(" in js
    for name in ("backgroundSetLayers", "backgroundSetPrivacy"):
        assert f"addon.{name}(" in js and f'"{name}"' in cc


@pytest.mark.gpu
def test_node_layers_match_the_c_path(addon_built, pkg, synthetic, tmp_path):
    """One blur case (level 'medium') and one image case (level 'high'), n=2 at
    120x160, each from the first frame of a stream."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, h, w = 2, 120, 160
    rng = np.random.default_rng(5)
    frames = np.stack([synthetic.make_frame(730 + i, h, w, 3) for i in range(n)])
    sprite = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    image = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    fp, sp, ip, op = tmp_path / "frames.bin", tmp_path / "sprite.bin", tmp_path / "image.bin", tmp_path / "out"
    frames.tofile(fp)
    sprite.tofile(sp)
    image.tofile(ip)
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "run_layers.js"), str(fp), str(n), str(h), str(w),
                          "3", str(sp), "9", "13", str(ip), "30", "40", str(op), "bf16x2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info == {"width": w, "height": h, "count": n, "rejected": 2}
    L = pkg.Layer
    layers = [L("rect", "low", 50, 90, 1100, 280, radius=20, color=(0, 0, 0, 64)),
              L("image", "medium", 300, 200, 900, 500, pixels=sprite,
                shadow={"color": (0, 0, 0, 179), "blur": 40, "dx": 20, "dy": 20}),
              L("rect", "high", 1300, 60, 580, 350, radius=60, color=(250, 10, 20, 200))]
    with pkg.Session(dtype="bf16x2", max_batch=n, max_frame_h=h, max_frame_w=w) as s:
        chain = pkg.PostChain(s)
        bg = pkg.Background(s)
        bg.set_blur(7, 2.5)
        plain = chain.replace_background(frames, bg)
        chain.reset()
        bg.set_layers(layers)
        want_blur = chain.replace_background(frames, bg)
        chain.reset()
        bg.set_image(image)
        bg.set_privacy("high")
        want_image = chain.replace_background(frames, bg)
    for name, want in (("blur", want_blur), ("image", want_image)):
        got = np.fromfile(f"{op}_{name}.u8", np.uint8).reshape(n, h, w, 4)
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"
    assert not np.array_equal(plain, want_blur) and not np.array_equal(want_blur, want_image)
