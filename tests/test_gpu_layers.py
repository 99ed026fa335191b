"""GPU parity of the branding layers (csrc/vss_layers.hip, the layered forms in
csrc/vss_background.hip) through the C ABI against the numpy reference
(tests/layers_ref.py).  Every comparison is BIT-EXACT.  The frames are small:
45 x 150 spans 2 x 3 blur tiles with a width that is no multiple of 4, 37 x 53
is odd in both directions (the per-pixel tail of the quad stores); the batch is 2, so the plate
is shared over the batch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref  # noqa: E402
import layers_ref as ref  # noqa: E402
import video_ref  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = [(45, 150), (37, 53)]
H, W = 32, 48  # the mask: no larger than either frame, so that refinement applies
REFINE = (2, 16.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def sess(pkg, torch_cuda):
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=2, autotune=False) as s:
        yield s


def _sprite(seed, h, w):
    """RGBA noise with partial alpha, a transparent band and an opaque one."""
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[: h // 3, :, 3] = 0
    px[-(h // 3):, :, 3] = 255
    return px


@pytest.fixture(scope="module")
def inputs():
    """Per frame size: noise frames (3 channels at the first size, 4 at the second) and
    random alpha bytes with 0 and 255 regions; built once."""
    out = {}
    for i, (fh, fw) in enumerate(FRAMES):
        rng = np.random.default_rng(500 + i)
        a = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
        a[:, : H // 4] = 0
        a[:, -H // 4:] = 255
        out[(fh, fw)] = (rng.integers(0, 256, (2, fh, fw, 3 + i), dtype=np.uint8), a)
    return out


def _cases(pkg, cw, ch):
    """The plates of the issue's list, in units of the canvas cw x ch."""
    L = pkg.Layer
    u, v = cw / 100.0, ch / 100.0

    def r(x, y, w, h, color, radius=0, privacy=1, shadow=None):
        return L("rect", privacy, int(x * u), int(y * v), int(w * u), int(h * v), radius=int(radius * u), color=color,
                 shadow=shadow)

    def img(x, y, w, h, px, privacy=1, shadow=None):
        return L("image", privacy, int(x * u), int(y * v), int(w * u), int(h * v), pixels=px, shadow=shadow)

    sh = lambda blur, dx=3, dy=4, color=(10, 20, 30, 200): {"color": color, "blur": blur, "dx": dx, "dy": dy}  # noqa: E731
    return {
        "plain rect": [r(10, 20, 55, 47, (200, 100, 50, 180))],
        "capsule": [r(5, 30, 80, 40, (0, 255, 128, 255), radius=90)],
        "rounded": [r(12, 8, 70, 80, (90, 10, 250, 140), radius=11)],
        "negative x": [r(-20, 10, 50, 60, (255, 255, 0, 99), radius=9)],
        "off the frame": [r(120, 10, 30, 30, (1, 2, 3, 255)), r(10, -50, 30, 40, (1, 2, 3, 255)),
                          r(10, 10, 0, 30, (1, 2, 3, 255))],
        "sprite up": [img(10, 5, 85, 90, _sprite(1, 7, 9))],
        "sprite down": [img(-8, 20, 60, 55, _sprite(2, 90, 201))],
        "shadow blur 30": [r(30, 30, 40, 40, (255, 255, 255, 255), radius=6, shadow=sh(30, 2, 2))],
        "shadow blur 0": [img(20, 20, 50, 50, _sprite(3, 12, 12), shadow=sh(0, int(6 * u), int(-5 * v)))],
        "shadow blur 1": [r(20, 25, 45, 40, (5, 6, 7, 128), radius=8, shadow=sh(1, int(-4 * u), int(3 * v)))],
        "shadow off the edge": [r(80, 70, 30, 40, (50, 60, 70, 255), shadow=sh(12, int(5 * u), int(5 * v)))],
        "three overlapping": [r(5, 10, 60, 60, (255, 0, 0, 128), radius=10),
                              img(30, 25, 55, 60, _sprite(4, 10, 14), shadow=sh(8, int(2 * u), int(2 * v))),
                              r(45, 5, 40, 70, (0, 0, 255, 200), radius=25, shadow=sh(4, int(-2 * u), int(3 * v),
                                                                                     (0, 0, 0, 255)))],
    }


def _same(tag, got, want):
    assert got.shape == want.shape, f"{tag}: shape {got.shape} != {want.shape}"
    bad = int((got != want).sum())
    assert bad == 0, f"{tag}: {bad} of {want.size} bytes differ (max |d| = " \
                     f"{int(np.abs(got.astype(int) - want.astype(int)).max())})"


CASE_NAMES = ["plain rect", "capsule", "rounded", "negative x", "off the frame", "sprite up", "sprite down",
              "shadow blur 30", "shadow blur 0", "shadow blur 1", "shadow off the edge", "three overlapping"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plate_bitexact(pkg, torch_cuda, sess, oracle, name):
    """vss_background_overlay_device at both frame sizes, on the reference's canvas and
    on a canvas equal to the frame (blur 30 there: sigma 15, the radius clamps to 32;
    blur 1 on 1920: vss_blur_weights refuses, B = P)."""
    bg = pkg.Background(sess)
    try:
        for fh, fw in FRAMES:
            for canvas in ((1920, 1080), (fw, fh)):
                layers = _cases(pkg, *canvas)[name]
                bg.set_layers(layers, canvas)
                want = ref.overlay(oracle, pkg, layers, 2, canvas, fh, fw)
                _same(f"{name} {fh}x{fw} canvas {canvas}", bg.overlay(fh, fw), want)
                assert want.any() == (name != "off the frame")
    finally:
        bg.close()


def test_shadow_cases_take_the_paths_they_name(pkg):
    import math
    sigma = 30 * 150 / (2.0 * 150)
    assert min(32, math.ceil(3 * sigma)) == 32 < math.ceil(3 * sigma)
    sigma = 1 * 53 / (2.0 * 1920)
    assert math.ceil(3 * sigma) == 1
    with pytest.raises(pkg.VssError):
        pkg.blur_weights(1, sigma)


def _run(torch, pkg, s, bg, frames, alpha, pad_out=8):
    """background_composite_device into a 0xAB-filled buffer with padded rows -> RGBA [n,fh,fw,4]."""
    n, fh, fw, c = frames.shape
    ors = fw * 4 + pad_out
    df = torch.from_numpy(frames).cuda()
    da = torch.from_numpy(alpha).cuda()
    do = torch.full((n, fh, ors), 0xAB, dtype=torch.uint8, device="cuda")
    pkg.background_composite_device(s, bg, df.data_ptr(), n, fh, fw, c, fw * c, fh * fw * c, da.data_ptr(),
                                    do.data_ptr(), ors, fh * ors, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    assert np.all(got[:, :, fw * 4:] == 0xAB), "row padding was written"
    return got[:, :, :fw * 4].reshape(n, fh, fw, 4)


IMAGE = np.random.default_rng(77).integers(0, 256, (20, 31, 3), dtype=np.uint8)
IMAGE2 = np.random.default_rng(78).integers(0, 256, (60, 40, 4), dtype=np.uint8)
BLUR = (5, 2.0)
CANVAS = (1920, 1080)


def _want(pkg, oracle, mode, frames, alpha, layers, level, refine, canvas=CANVAS, color=(32, 32, 32), image=IMAGE):
    """The reference for a state, built from scratch."""
    n, fh, fw, _ = frames.shape
    if mode == "colour":
        bgv = np.array(color)
    elif mode == "image":
        bgv = background_ref.scale_image(oracle, image, fh, fw)
    else:
        bgv = background_ref.blur(frames, pkg.blur_weights(*BLUR))
    O = ref.overlay(oracle, pkg, layers, level, canvas, fh, fw)
    return ref.composite(oracle, frames, alpha, bgv, O, refine)


def _set_mode(bg, mode):
    if mode == "image":
        bg.set_image(IMAGE)
    elif mode == "blur":
        bg.set_blur(*BLUR)


@pytest.mark.parametrize("refine", [None, REFINE], ids=["plain", "refine"])
@pytest.mark.parametrize("mode", ["colour", "image", "blur"])
def test_composite_bitexact(pkg, torch_cuda, sess, oracle, inputs, mode, refine):
    """O between the background and the person in every mode, refinement off and on,
    at both frame sizes in turn through one object (the plate follows the size)."""
    layers = _cases(pkg, *CANVAS)["three overlapping"]
    bg = pkg.Background(sess)
    try:
        _set_mode(bg, mode)
        if refine:
            bg.set_refine(*refine)
        bg.set_layers(layers)
        for size in FRAMES + FRAMES[:1]:
            frames, alpha = inputs[size]
            got = _run(torch_cuda, pkg, sess, bg, frames, alpha)
            _same(f"{mode} {size}", got, _want(pkg, oracle, mode, frames, alpha, layers, 2, refine))
        plain = _want(pkg, oracle, mode, frames, alpha, [], 2, refine)
        assert not np.array_equal(got, plain)  # the layers show
    finally:
        bg.close()


@pytest.mark.parametrize("mode", ["colour", "image", "blur"])
def test_invalidation(pkg, torch_cuda, sess, oracle, inputs, mode):
    """After a privacy change, new layers, a new frame size, a new colour, a new image
    and set_layers([]) the next composite equals the reference of the new state."""
    cases = _cases(pkg, *CANVAS)
    layers = cases["three overlapping"]
    layers[0].privacy, layers[1].privacy, layers[2].privacy = 1, 2, 3
    a, b = FRAMES
    bg, fresh = pkg.Background(sess), pkg.Background(sess)
    try:
        _set_mode(bg, mode)
        _set_mode(fresh, mode)
        state = {"layers": layers, "level": 2, "color": (32, 32, 32), "image": IMAGE, "mode": mode}

        def check(tag, size):
            frames, alpha = inputs[size]
            got = _run(torch_cuda, pkg, sess, bg, frames, alpha)
            want = _want(pkg, oracle, state["mode"], frames, alpha, state["layers"], state["level"], None,
                         color=state["color"], image=state["image"])
            _same(f"{mode}: {tag}", got, want)
            return got

        bg.set_layers(layers)
        first = check("layers set", a)
        for level in (1, 3, 2):
            bg.set_privacy(level)
            state["level"] = level
            got = check(f"privacy {level}", a)
        _same("back at level 2", got, first)
        state["layers"] = cases["sprite down"] + cases["rounded"]
        bg.set_layers(state["layers"])
        check("new layers", a)
        check("new frame size", b)
        check("and back", a)
        if mode == "colour":
            bg.set_color(200, 10, 99)
            state["color"] = (200, 10, 99)
            check("new colour", a)
        if mode == "image":
            bg.set_image(IMAGE2)
            state["image"] = IMAGE2
            check("new image", a)
            bg.set_color(1, 2, 3)
            state["mode"], state["color"] = "colour", (1, 2, 3)
            check("colour after image", a)
            bg.set_mode(pkg.VSS_BG_IMAGE)
            state["mode"] = "image"
            check("back to the image", a)
        bg.set_layers([])
        state["layers"] = []
        got = check("no layers", a)
        if mode == "colour":
            fresh.set_color(*state["color"])
        if mode == "image":
            fresh.set_image(IMAGE2)
        frames, alpha = inputs[a]
        _same("set_layers([]) vs a fresh background", got, _run(torch_cuda, pkg, sess, fresh, frames, alpha))
    finally:
        bg.close()
        fresh.close()


def _device_bytes(pkg, s):
    info = pkg._Info()
    assert pkg.lib().vss_get_info(s._h, ctypes.byref(info)) == pkg.VSS_OK
    return info.device_bytes


def test_device_bytes_are_counted_and_released(pkg, torch_cuda, sess, inputs):
    frames, alpha = inputs[FRAMES[0]]
    layers = _cases(pkg, *CANVAS)["three overlapping"]
    before = _device_bytes(pkg, sess)
    bg = pkg.Background(sess)
    bg.set_blur(*BLUR)
    _run(torch_cuda, pkg, sess, bg, frames, alpha)
    with_blur = _device_bytes(pkg, sess)
    for mode in ("blur", "colour"):
        if mode == "colour":
            bg.set_color(5, 6, 7)
        bg.set_layers(layers)
        assert _device_bytes(pkg, sess) > with_blur  # the sprites
        _run(torch_cuda, pkg, sess, bg, frames, alpha)
        fh, fw = FRAMES[0]
        assert _device_bytes(pkg, sess) >= with_blur + 4 * fh * fw + 10 * 14 * 4  # the plate and the sprite
        bg.set_layers([])
        assert _device_bytes(pkg, sess) == with_blur
    bg.set_layers(layers)
    _run(torch_cuda, pkg, sess, bg, frames, alpha)
    bg.close()
    assert _device_bytes(pkg, sess) == before


def test_invalid_arguments_change_nothing(pkg, torch_cuda, oracle, inputs):
    torch = torch_cuda
    lib = pkg.lib()
    frames, alpha = inputs[FRAMES[1]]
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=2, autotune=False) as s1, \
            pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=2, autotune=False) as s2:
        bg = pkg.Background(s1)
        bg.set_blur(*BLUR)
        good = _cases(pkg, *CANVAS)["three overlapping"]
        bg.set_layers(good)
        want = _run(torch, pkg, s1, bg, frames, alpha)
        _same("before", want, _want(pkg, oracle, "blur", frames, alpha, good, 2, None))
        px = np.zeros((4, 4, 4), np.uint8)

        def one(**kw):
            l = pkg._Layer()
            l.type, l.privacy, l.width, l.height = pkg.VSS_LAYER_ROUNDED_RECT, 1, 10, 10
            l.pixels, l.src_h, l.src_w, l.row_stride = px.ctypes.data, 4, 4, 16
            for k, v in kw.items():
                setattr(l, k, v)
            return (pkg._Layer * 1)(l)

        ok = one()
        IMG = pkg.VSS_LAYER_IMAGE
        calls = {
            "n < 0": lambda: lib.vss_background_set_layers(bg._bg, ok, -1, 1920, 1080),
            "n > 32": lambda: lib.vss_background_set_layers(bg._bg, (pkg._Layer * 33)(), 33, 1920, 1080),
            "canvas_w": lambda: lib.vss_background_set_layers(bg._bg, ok, 1, 0, 1080),
            "canvas_h": lambda: lib.vss_background_set_layers(bg._bg, ok, 1, 1920, -5),
            "canvas with n = 0": lambda: lib.vss_background_set_layers(bg._bg, None, 0, 0, 0),
            "null array": lambda: lib.vss_background_set_layers(bg._bg, None, 1, 1920, 1080),
            "type": lambda: lib.vss_background_set_layers(bg._bg, one(type=2), 1, 1920, 1080),
            "privacy 0": lambda: lib.vss_background_set_layers(bg._bg, one(privacy=0), 1, 1920, 1080),
            "privacy 4": lambda: lib.vss_background_set_layers(bg._bg, one(privacy=4), 1, 1920, 1080),
            "width": lambda: lib.vss_background_set_layers(bg._bg, one(width=-1), 1, 1920, 1080),
            "height": lambda: lib.vss_background_set_layers(bg._bg, one(height=-1), 1, 1920, 1080),
            "radius": lambda: lib.vss_background_set_layers(bg._bg, one(radius=-1), 1, 1920, 1080),
            "shadow_blur": lambda: lib.vss_background_set_layers(bg._bg, one(has_shadow=1, shadow_blur=-1), 1, 1920,
                                                                 1080),
            "null sprite": lambda: lib.vss_background_set_layers(bg._bg, one(type=IMG, pixels=None), 1, 1920, 1080),
            "src_h 0": lambda: lib.vss_background_set_layers(bg._bg, one(type=IMG, src_h=0), 1, 1920, 1080),
            "src_w 4097": lambda: lib.vss_background_set_layers(bg._bg, one(type=IMG, src_w=4097, row_stride=1 << 20),
                                                                1, 1920, 1080),
            "row_stride": lambda: lib.vss_background_set_layers(bg._bg, one(type=IMG, row_stride=15), 1, 1920, 1080),
            "level 0": lambda: lib.vss_background_set_privacy(bg._bg, 0),
            "level 4": lambda: lib.vss_background_set_privacy(bg._bg, 4),
        }
        for tag, call in calls.items():
            assert call() == pkg.VSS_E_INVALID_ARG, tag
            assert lib.vss_last_error(s1._h), tag
            _same(f"after a refused call ({tag})", _run(torch, pkg, s1, bg, frames, alpha), want)
        out = torch.zeros((37, 53, 4), dtype=torch.uint8, device="cuda")
        assert lib.vss_background_overlay_device(s2._h, bg._bg, 37, 53, out.data_ptr(), 53 * 4,
                                                 None) == pkg.VSS_E_INVALID_ARG  # an object of another handle
        assert b"background" in lib.vss_last_error(s2._h)
        assert lib.vss_background_overlay_device(s1._h, bg._bg, 37, 53, out.data_ptr(), 53 * 4 - 1,
                                                 None) == pkg.VSS_E_INVALID_ARG
        _same("after the refused overlays", _run(torch, pkg, s1, bg, frames, alpha), want)
        with pytest.raises(pkg.VssError):
            bg.set_privacy(7)
        with pytest.raises(pkg.VssError):
            bg.set_layers([pkg.Layer("rect", 1, 0, 0, -1, 5)])


def test_video_path_carries_the_layers(pkg, torch_cuda, synthetic, oracle):
    """vss_video_process_device over a layered blur background ==
    pack(composite(unpack(in))), the alpha from the post chain's own device calls."""
    torch = torch_cuda
    std = video_ref.BT709_LIMITED
    n, fh, fw = 2, 44, 150
    rgb = np.stack([synthetic.make_frame(40 + i, fh, fw, 3) for i in range(n)])
    y, uv = video_ref.pack(std, rgb)
    layers = _cases(pkg, *CANVAS)["three overlapping"]
    with pkg.Session(model_h=H, model_w=W, dtype="f32", autotune=False) as s:
        bg = pkg.Background(s)
        bg.set_blur(*BLUR)
        bg.set_layers(layers)
        st = torch.cuda.current_stream().cuda_stream
        v, staged = pkg.Video(s, std), pkg.PostChain(s)
        dy, duv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
        oy, ouv = torch.zeros_like(dy), torch.zeros_like(duv)
        for chain in (pkg.PostChain(s), pkg.PostChain(s)):  # the second call reuses the plate (and what the seam replays)
            v.process_device(chain, bg, dy.data_ptr(), fw, fw * fh, duv.data_ptr(), fw, fw * fh // 2, n, fh, fw,
                             oy.data_ptr(), fw, fw * fh, ouv.data_ptr(), fw, fw * fh // 2, st)
        torch.cuda.synchronize()
        rgba_np = video_ref.unpack(std, y, uv)
        rgba = torch.from_numpy(rgba_np).cuda()
        masks = torch.empty((n, s.mask_h * s.mask_w), dtype=torch.float32, device="cuda")
        alpha = torch.empty((n, s.mask_h, s.mask_w), dtype=torch.uint8, device="cuda")
        s.segment_device(rgba.data_ptr(), n, fh, fw, 4, fw * 4, fh * fw * 4, masks.data_ptr(), st)
        staged.process_device(rgba.data_ptr(), n, fh, fw, 4, fw * 4, fh * fw * 4, masks.data_ptr(), 0,
                              alpha.data_ptr(), st)
        torch.cuda.synchronize()
        want = _want(pkg, oracle, "blur", rgba_np, alpha.cpu().numpy(), layers, 2, None)
        want_y, want_uv = video_ref.pack(std, want)
        _same("Y", oy.cpu().numpy(), want_y)
        _same("UV", ouv.cpu().numpy(), want_uv)
        plain_y, _ = video_ref.pack(std, _want(pkg, oracle, "blur", rgba_np, alpha.cpu().numpy(), [], 2, None))
        assert not np.array_equal(want_y, plain_y)
