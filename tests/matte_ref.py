"""Numpy reference of the edge-aware matte (include/vss.h, guided-filter
refinement): linear coefficients of the alpha against the
frame's luma fitted at mask resolution, box-meaned, upsampled with the
oracle's own f32 recipe and applied to the luma at frame resolution.  Integers,
doubles in one prescribed order and that f32 recipe only, so every comparison
against it is bit-exact."""
import numpy as np

import background_ref

MAX_RADIUS = 8


def luma(frames: np.ndarray) -> np.ndarray:
    """frames [n,fh,fw,3|4] u8 -> Y = (77 R + 150 G + 29 B + 128) >> 8, int64 0..255."""
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def guide(Y: np.ndarray, H: int, W: int) -> np.ndarray:
    """Y [n,fh,fw] -> L [n,H,W]: the area mean over rows [i*fh//H, (i+1)*fh//H) and
    columns [j*fw//W, (j+1)*fw//W), rounded half up."""
    n, fh, fw = Y.shape
    assert fh >= H and fw >= W, "the guide needs a frame no smaller than the mask"
    r = np.arange(H + 1, dtype=np.int64) * fh // H
    c = np.arange(W + 1, dtype=np.int64) * fw // W
    s = np.add.reduceat(np.add.reduceat(Y.astype(np.int64), r[:-1], axis=1), c[:-1], axis=2)
    cnt = np.diff(r)[:, None] * np.diff(c)[None, :]
    return (s + cnt // 2) // cnt


def box_sum(x: np.ndarray, r: int) -> np.ndarray:
    """Sum of x [n,H,W] (int64) over [i-r, i+r] x [j-r, j+r] clipped to the plane."""
    _, H, W = x.shape
    c = np.zeros((x.shape[0], H + 1, W + 1), np.int64)
    c[:, 1:, 1:] = x.cumsum(1).cumsum(2)
    i, j = np.arange(H), np.arange(W)
    i0, i1 = np.maximum(i - r, 0), np.minimum(i + r, H - 1) + 1
    j0, j1 = np.maximum(j - r, 0), np.minimum(j + r, W - 1) + 1
    return (c[:, i1][:, :, j1] - c[:, i0][:, :, j1] - c[:, i1][:, :, j0] + c[:, i0][:, :, j0])


def coefficients(L: np.ndarray, p: np.ndarray, radius: int, eps: float):
    """L, p [n,H,W] integers 0..255 -> the mean planes (abar, bbar) f32 [n,H,W]."""
    assert 1 <= radius <= MAX_RADIUS and 1.0 <= eps <= 65025.0
    L, p = np.asarray(L).astype(np.int64), np.asarray(p).astype(np.int64)
    N = box_sum(np.ones_like(L), radius)
    S_L, S_p, S_Lp, S_LL = (box_sum(v, radius) for v in (L, p, L * p, L * L))
    assert max(S_Lp.max(), S_LL.max()) < 2 ** 32
    cov = N * S_Lp - S_L * S_p
    var = N * S_LL - S_L * S_L
    assert var.min() >= 0
    a = cov.astype(np.float64) / (var.astype(np.float64) + np.float64(eps) * (N * N).astype(np.float64))
    prod = a * S_L.astype(np.float64)  # rounded before the subtraction
    b = (S_p.astype(np.float64) - prod) / N.astype(np.float64)
    a_f, b_f = np.floor(a * 65536.0 + 0.5), np.floor(b * 256.0 + 0.5)
    lim = float(2 ** 31) / (2 * MAX_RADIUS + 1) ** 2  # the 289-term sums fit int32
    assert np.abs(a_f).max() < lim and np.abs(b_f).max() < lim
    a_q, b_q = a_f.astype(np.int64), b_f.astype(np.int64)
    abar = (box_sum(a_q, radius).astype(np.float64) / (N * 65536).astype(np.float64)).astype(np.float32)
    bbar = (box_sum(b_q, radius).astype(np.float64) / (N * 256).astype(np.float64)).astype(np.float32)
    return abar, bbar


def apply(oracle, abar: np.ndarray, bbar: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """A = floor(clamp(abar_up * Y + bbar_up, 0, 255) + 0.5) in f32, the product
    rounded before the sum; the planes upsampled by oracle.upsample_mask."""
    n, fh, fw = Y.shape
    au, bu = oracle.upsample_mask(abar, fh, fw), oracle.upsample_mask(bbar, fh, fw)
    prod = au * Y.astype(np.float32)
    q = prod + bu
    q = np.minimum(np.maximum(q, np.float32(0)), np.float32(255))
    return np.floor(q + np.float32(0.5)).astype(np.uint8)


def refine_guided(oracle, L, p, Y, radius: int, eps: float) -> np.ndarray:
    """Steps 3-7 on a given low-resolution guide L."""
    abar, bbar = coefficients(L, p, radius, eps)
    return apply(oracle, abar, bbar, Y)


def alpha(oracle, frames: np.ndarray, alpha_u8: np.ndarray, radius: int, eps: float) -> np.ndarray:
    """frames [n,fh,fw,3|4] u8, alpha bytes [n,H,W] u8 -> refined alpha [n,fh,fw] u8."""
    _, H, W = alpha_u8.shape
    Y = luma(frames)
    return refine_guided(oracle, guide(Y, H, W), alpha_u8, Y, radius, eps)


def plain_alpha(oracle, frames: np.ndarray, alpha_u8: np.ndarray) -> np.ndarray:
    """Refinement off: the 4th byte of the oracle's composite."""
    return oracle.composite(np.asarray(frames), alpha_u8)[..., 3]


def composite(oracle, frames: np.ndarray, alpha_u8: np.ndarray, bg, radius: int, eps: float) -> np.ndarray:
    """The refined alpha through the existing blend -> opaque RGBA [n,fh,fw,4]."""
    frames = np.asarray(frames)
    n, fh, fw, _ = frames.shape
    A = alpha(oracle, frames, alpha_u8, radius, eps)[..., None]
    out = np.full((n, fh, fw, 4), 255, np.uint8)
    out[..., :3] = background_ref.blend(frames[..., :3], np.broadcast_to(np.asarray(bg), (n, fh, fw, 3)), A)
    return out
