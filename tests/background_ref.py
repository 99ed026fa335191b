"""Numpy reference of the virtual backgrounds (include/vss.h): the integer
blend, the fixed-point separable blur with replicated edges, and the background
image's scaling through the oracle's compositing upscale.  Exact integers (or
the oracle's own f32 recipe), so every comparison against it is bit-exact."""
import numpy as np


def numpy_blur_weights(radius: int, sigma: float) -> np.ndarray:
    """The definition of vss_blur_weights in numpy doubles, int64 [2r+1]."""
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    w = np.floor(65536.0 * g / g.sum() + 0.5).astype(np.int64)
    w[radius] = 0
    w[radius] = 65536 - w.sum()
    return w


def blend(fg, bg, a):
    """(fg*A + bg*(255-A) + 127) // 255 on broadcastable integer arrays -> u8."""
    fg, bg, a = (np.asarray(v).astype(np.int64) for v in (fg, bg, a))
    return ((fg * a + bg * (255 - a) + 127) // 255).astype(np.uint8)


def _blur_axis(img: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    r = (len(w) - 1) // 2
    pad = [(0, 0)] * img.ndim
    pad[axis] = (r, r)
    p = np.pad(img.astype(np.int64), pad, mode="edge")
    size = img.shape[axis]
    acc = np.full(img.shape, 32768, np.int64)
    for k in range(2 * r + 1):
        acc += int(w[k]) * np.take(p, np.arange(k, k + size), axis=axis)
    return (acc >> 16).astype(np.uint8)


def blur(frames: np.ndarray, w: np.ndarray) -> np.ndarray:
    """frames [n,h,w,c>=3] u8 -> blurred RGB [n,h,w,3]: the horizontal pass stored
    as u8, then the vertical pass over it; w = the 2r+1 taps (from vss_blur_weights)."""
    rgb = np.asarray(frames)[..., :3]
    return _blur_axis(_blur_axis(rgb, w, 2), w, 1)


def scale_image(oracle, image: np.ndarray, fh: int, fw: int) -> np.ndarray:
    """image [h,w,3|4] u8 -> RGB [fh,fw,3]: per channel, the alpha byte of the
    oracle's compositing upscale of that channel (the definition of the scaling)."""
    image = np.asarray(image)
    dummy = np.zeros((1, fh, fw, 3), np.uint8)
    return np.stack([oracle.composite(dummy, np.ascontiguousarray(image[None, :, :, c]))[0, :, :, 3]
                     for c in range(3)], axis=-1)


def composite(oracle, frames: np.ndarray, alpha_u8: np.ndarray, bg) -> np.ndarray:
    """frames [n,fh,fw,3|4], alpha bytes [n,H,W], bg broadcastable to [n,fh,fw,3]
    -> opaque RGBA [n,fh,fw,4]; A = the 4th byte of the unchanged oracle.composite."""
    frames = np.asarray(frames)
    n, fh, fw, _ = frames.shape
    A = oracle.composite(frames, alpha_u8)[..., 3:4]
    out = np.full((n, fh, fw, 4), 255, np.uint8)
    out[..., :3] = blend(frames[..., :3], np.broadcast_to(np.asarray(bg), (n, fh, fw, 3)), A)
    return out
