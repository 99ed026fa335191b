"""What the tests of the calls over many streams share (include/vss_streams.h):
a background's settings as a dict, applied to a Background object and restated
per frame through the numpy references of the single-object calls
(background_ref, layers_ref, matte_ref).  Nothing here runs the pooled path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref as bref  # noqa: E402
import layers_ref as lref  # noqa: E402
import matte_ref as mref  # noqa: E402

CANVAS = (1920, 1080)
IMAGE = np.random.default_rng(177).integers(0, 256, (20, 31, 3), dtype=np.uint8)
IMAGE2 = np.random.default_rng(178).integers(0, 256, (33, 27, 4), dtype=np.uint8)


def spec(mode, color=(32, 32, 32), image=None, blur=None, layers=(), level=2, refine=None):
    """mode: 'colour' | 'image' | 'blur'; blur = (radius, sigma); refine = (radius, eps) or None."""
    return {"mode": mode, "color": tuple(color), "image": image, "blur": blur, "layers": list(layers), "level": level,
            "refine": refine}


def layers(pkg):
    """A rounded rectangle with a shadow and a sprite: visible at level 2, partial alpha, off-centre."""
    px = np.random.default_rng(179).integers(0, 256, (9, 13, 4), dtype=np.uint8)
    px[:3, :, 3] = 0
    px[-3:, :, 3] = 255
    L = pkg.Layer
    return [L("rect", 1, 150, 200, 900, 500, radius=120, color=(200, 100, 50, 180),
              shadow={"color": (10, 20, 30, 200), "blur": 40, "dx": 30, "dy": 40}),
            L("image", 2, 800, 100, 700, 600, pixels=px)]


def apply(pkg, bg, sp):
    """The settings of `sp` on the Background bg (a fresh object or one set before)."""
    if sp["mode"] == "colour":
        bg.set_color(*sp["color"])
    elif sp["mode"] == "image":
        bg.set_image(sp["image"])
    else:
        bg.set_blur(*sp["blur"])
    bg.set_layers(sp["layers"], CANVAS)
    bg.set_privacy(sp["level"])
    bg.set_refine(*(sp["refine"] or (0, 0.0)))
    return bg


def want(pkg, oracle, sp, frame, alpha):
    """frame [fh,fw,3|4] u8 and alpha bytes [H,W] u8 -> that frame over `sp`, RGBA [fh,fw,4]."""
    f, a = np.ascontiguousarray(frame[None]), np.ascontiguousarray(alpha[None])
    _, fh, fw, _ = f.shape
    if sp["mode"] == "colour":
        bgv = np.array(sp["color"])
    elif sp["mode"] == "image":
        bgv = bref.scale_image(oracle, sp["image"], fh, fw)
    else:
        bgv = bref.blur(f, pkg.blur_weights(*sp["blur"]))
    if sp["layers"]:
        O = lref.overlay(oracle, pkg, sp["layers"], sp["level"], CANVAS, fh, fw)
        return lref.composite(oracle, f, a, bgv, O, sp["refine"])[0]
    if sp["refine"]:
        return mref.composite(oracle, f, a, bgv, *sp["refine"])[0]
    return bref.composite(oracle, f, a, bgv)[0]


def want_all(pkg, oracle, specs, frames, alpha):
    return np.stack([want(pkg, oracle, sp, frames[t], alpha[t]) for t, sp in enumerate(specs)])


def alpha_bytes(seed, n, H, W):
    """Random alpha bytes with a 0 band and a 255 band."""
    a = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    a[:, : H // 4] = 0
    a[:, -(H // 4):] = 255
    return a


def same(tag, got, want_):
    assert got.shape == want_.shape, f"{tag}: shape {got.shape} != {want_.shape}"
    bad = int((got != want_).sum())
    assert bad == 0, f"{tag}: {bad} of {want_.size} bytes differ (max |d| = " \
                     f"{int(np.abs(got.astype(int) - want_.astype(int)).max())})"
