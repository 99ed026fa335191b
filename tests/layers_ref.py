"""Numpy reference of the branding layers (include/vss_layers.h): the canvas
mapping, the rounded rectangle's 4 x 4 coverage, the sprite scaling (the
oracle's compositing upscale per premultiplied channel, as
background_ref.scale_image), the drop shadow, premultiplied source-over into
the overlay plate O, and O between the background and the person.  Exact
integers (or the oracle's own f32 recipe), so every comparison against it is
bit-exact.

A layer here is a dict: type "rect" | "image", privacy 1..3, x, y, width,
height, and for a rect color (r, g, b, a) and radius, for an image pixels
(RGBA u8 [h,w,4], not premultiplied); optionally shadow = {"color": (r, g, b,
a), "blur", "dx", "dy"}.  Objects with the same attributes (vss_amd.Layer)
serve as well."""
import math

import numpy as np

import background_ref
import matte_ref


def lmap(v: int, canvas: int, frame: int) -> int:
    """map(v, canvas, frame) = floor((2*v*frame + canvas) / (2*canvas)), Python integers."""
    return (2 * int(v) * int(frame) + int(canvas)) // (2 * int(canvas))


def _get(layer, key, default=None):
    if isinstance(layer, dict):
        return layer.get(key, default)
    return getattr(layer, key, default)


def _privacy(layer) -> int:
    p = _get(layer, "privacy")
    return {"low": 1, "medium": 2, "high": 3}[p] if isinstance(p, str) else int(p)


def rect_coverage(X0, Y0, X1, Y1, R, xs, ys) -> np.ndarray:
    """n in 0..16 for the pixels ys x xs (inside the rectangle) -> int64 [len(ys), len(xs)]."""
    n = np.zeros((len(ys), len(xs)), np.int64)
    x = np.asarray(xs, np.int64)[None, :]
    y = np.asarray(ys, np.int64)[:, None]
    for j in range(4):
        sy = 8 * y + 2 * j + 1
        for i in range(4):
            sx = 8 * x + 2 * i + 1
            inside = (sx > 8 * X0) & (sx < 8 * X1) & (sy > 8 * Y0) & (sy < 8 * Y1)
            # the corner squares: dx, dy from the square's inner vertex (the arc's centre)
            dx = np.where(sx < 8 * (X0 + R), 8 * (X0 + R) - sx, np.where(sx > 8 * (X1 - R), sx - 8 * (X1 - R), -1))
            dy = np.where(sy < 8 * (Y0 + R), 8 * (Y0 + R) - sy, np.where(sy > 8 * (Y1 - R), sy - 8 * (Y1 - R), -1))
            corner = (dx >= 0) & (dy >= 0)
            ok = ~corner | (dx * dx + dy * dy <= (8 * R) ** 2)
            n += (inside & ok).astype(np.int64)
    return n


def premultiply(rgba: np.ndarray) -> np.ndarray:
    p = np.asarray(rgba).astype(np.int64)
    out = p.copy()
    out[..., :3] = (p[..., :3] * p[..., 3:4] + 127) // 255
    return out.astype(np.uint8)


def scale_sprite(oracle, pm: np.ndarray, h: int, w: int) -> np.ndarray:
    """Premultiplied RGBA [sh,sw,4] -> [h,w,4]: background_ref.scale_image's recipe
    on four channels, then c = min(c, a)."""
    dummy = np.zeros((1, h, w, 3), np.uint8)
    s = np.stack([oracle.composite(dummy, np.ascontiguousarray(pm[None, :, :, c]))[0, :, :, 3] for c in range(4)],
                 axis=-1)
    s[..., :3] = np.minimum(s[..., :3], s[..., 3:4])
    return s


def layer_sample(oracle, layer, cw, ch, fh, fw):
    """The layer's premultiplied samples over its UNCLIPPED rectangle:
    (X0, Y0, S int64 [Y1-Y0, X1-X0, 4]) or None when the rectangle is empty."""
    x, y = _get(layer, "x"), _get(layer, "y")
    X0, X1 = lmap(x, cw, fw), lmap(x + _get(layer, "width"), cw, fw)
    Y0, Y1 = lmap(y, ch, fh), lmap(y + _get(layer, "height"), ch, fh)
    if X1 <= X0 or Y1 <= Y0:
        return None
    if _get(layer, "type") in ("rect", 1):
        r, g, b, a = (int(v) for v in _get(layer, "color"))
        R = min(lmap(_get(layer, "radius", 0), cw, fw), (X1 - X0) // 2, (Y1 - Y0) // 2)
        n = rect_coverage(X0, Y0, X1, Y1, R, range(X0, X1), range(Y0, Y1))
        sa = (a * n + 8) >> 4
        S = np.stack([(c * sa + 127) // 255 for c in (r, g, b)] + [sa], axis=-1)
    else:
        S = scale_sprite(oracle, premultiply(_get(layer, "pixels")), Y1 - Y0, X1 - X0).astype(np.int64)
    return X0, Y0, S


def _place(S, X0, Y0, fh, fw):
    """S (unclipped, at X0, Y0) on a zero frame-size canvas [fh,fw,...]."""
    out = np.zeros((fh, fw) + S.shape[2:], np.int64)
    h, w = S.shape[:2]
    x0, x1, y0, y1 = max(X0, 0), min(X0 + w, fw), max(Y0, 0), min(Y0 + h, fh)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = S[y0 - Y0:y1 - Y0, x0 - X0:x1 - X0]
    return out


def source_over(O, S):
    """O' = min(255, S + (O*(255 - S.a) + 127) // 255), per channel, alpha included."""
    return np.minimum(255, S + (O * (255 - S[..., 3:4]) + 127) // 255)


def _blur_zero(P, w, axis):
    r = (len(w) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(P, pad)
    acc = np.full(P.shape, 32768, np.int64)
    for k in range(2 * r + 1):
        acc += int(w[k]) * np.take(p, np.arange(k, k + P.shape[axis]), axis=axis)
    return acc >> 16


def shadow_sample(pkg, layer, sample, cw, ch, fh, fw):
    """The shadow's premultiplied sample on the frame, int64 [fh,fw,4]; pkg supplies vss_blur_weights."""
    sh = _get(layer, "shadow")
    X0, Y0, S = sample
    P = _place(S[..., 3], X0 + lmap(sh["dx"], cw, fw), Y0 + lmap(sh["dy"], ch, fh), fh, fw)
    sigma = sh["blur"] * fw / (2.0 * cw)
    r = min(32, int(math.ceil(3 * sigma)))
    B = P
    if r >= 1:
        try:
            w = pkg.blur_weights(r, sigma).astype(np.int64)
            B = _blur_zero(_blur_zero(P, w, 1), w, 0)
        except pkg.VssError:
            pass  # vss_blur_weights refuses: B = P
    r_, g_, b_, a_ = (int(v) for v in sh["color"])
    a_s = (a_ * B + 127) // 255
    return np.stack([(c * a_s + 127) // 255 for c in (r_, g_, b_)] + [a_s], axis=-1)


def overlay(oracle, pkg, layers, level, canvas, fh, fw) -> np.ndarray:
    """The plate O, premultiplied RGBA u8 [fh,fw,4]."""
    cw, ch = canvas
    O = np.zeros((fh, fw, 4), np.int64)
    for layer in layers:
        if _privacy(layer) > level:
            continue
        sample = layer_sample(oracle, layer, cw, ch, fh, fw)
        if sample is None:
            continue
        if _get(layer, "shadow") is not None:
            O = source_over(O, shadow_sample(pkg, layer, sample, cw, ch, fh, fw))
        O = source_over(O, _place(sample[2], sample[0], sample[1], fh, fw))
    return O.astype(np.uint8)


def under(bg, O) -> np.ndarray:
    """bg' = min(255, O.c + (bg.c*(255 - O.a) + 127) // 255); bg broadcastable to [..., fh, fw, 3]."""
    O = np.asarray(O).astype(np.int64)
    bg = np.asarray(bg).astype(np.int64)
    return np.minimum(255, O[..., :3] + (bg * (255 - O[..., 3:4]) + 127) // 255).astype(np.uint8)


def composite(oracle, frames, alpha_u8, bg, O, refine=None) -> np.ndarray:
    """The person over bg' = O over bg -> opaque RGBA [n,fh,fw,4]; refine = (radius, eps) or None."""
    frames = np.asarray(frames)
    n, fh, fw, _ = frames.shape
    bgp = under(np.broadcast_to(np.asarray(bg), (n, fh, fw, 3)), O)
    if refine:
        return matte_ref.composite(oracle, frames, alpha_u8, bgp, refine[0], refine[1])
    return background_ref.composite(oracle, frames, alpha_u8, bgp)
