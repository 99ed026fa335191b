"""The NV12 colour conversion of include/vss_video.h, restated in numpy: the
definition the GPU kernels (csrc/vss_video.hip) must match bit for bit.

All arithmetic is in signed integers, `>> 8` is the floor division by 256 and
clip clamps to 0..255.  NV12: y [n, fh, fw] u8 and uv [n, fh/2, fw] u8 with
(U, V) interleaved, one pair per 2x2 pixel block; fh and fw even."""
import numpy as np

BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = 0, 1, 2, 3
STANDARDS = (BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL)
LIMITED = (BT601_LIMITED, BT709_LIMITED)

# std: (y0, cy, rv, gu, gv, bu, Y(r,g,b), U(r,g,b), V(r,g,b))
TABLE = {
    BT601_LIMITED: (16, 298, 409, -100, -208, 516, (66, 129, 25), (-38, -74, 112), (112, -94, -18)),
    BT709_LIMITED: (16, 298, 459, -55, -136, 541, (47, 157, 16), (-26, -86, 112), (112, -102, -10)),
    BT601_FULL: (0, 256, 359, -88, -183, 454, (77, 150, 29), (-43, -85, 128), (128, -107, -21)),
    BT709_FULL: (0, 256, 403, -48, -120, 475, (54, 183, 19), (-29, -99, 128), (128, -116, -12)),
}


def _clip(v):
    return np.clip(v, 0, 255)


def unpack(std, y, uv):
    """NV12 -> RGBA u8 [n, fh, fw, 4]: each chroma pair replicated over its 2x2 block, A = 255."""
    y0, cy, rv, gu, gv, bu = TABLE[std][:6]
    y = np.asarray(y).astype(np.int32)
    uv = np.asarray(uv).astype(np.int32)
    n, fh, fw = y.shape
    assert fh % 2 == 0 and fw % 2 == 0 and uv.shape == (n, fh // 2, fw)
    u = np.repeat(np.repeat(uv[:, :, 0::2], 2, axis=1), 2, axis=2)
    v = np.repeat(np.repeat(uv[:, :, 1::2], 2, axis=1), 2, axis=2)
    c, d, e = cy * (y - y0), u - 128, v - 128
    out = np.empty((n, fh, fw, 4), np.uint8)
    out[..., 0] = _clip((c + rv * e + 128) >> 8)
    out[..., 1] = _clip((c + gu * d + gv * e + 128) >> 8)
    out[..., 2] = _clip((c + bu * d + 128) >> 8)
    out[..., 3] = 255
    return out


def block_mean(rgb):
    """[n, fh, fw, C] ints -> the rounded mean of each 2x2 block, [n, fh/2, fw/2, C]."""
    p = np.asarray(rgb).astype(np.int32)
    return (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2


def chroma_unclipped(std, m):
    """(U, V) of block means m [..., 3] before the clamp (the full standards reach 256)."""
    U, V = TABLE[std][7], TABLE[std][8]
    m = np.asarray(m).astype(np.int32)
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    return (((U[0] * r + U[1] * g + U[2] * b + 128) >> 8) + 128,
            ((V[0] * r + V[1] * g + V[2] * b + 128) >> 8) + 128)


def pack(std, rgba):
    """RGBA (or RGB) u8 [n, fh, fw, 3|4] -> (y [n, fh, fw], uv [n, fh/2, fw]) u8; alpha ignored."""
    y0 = TABLE[std][0]
    Y = TABLE[std][6]
    p = np.asarray(rgba).astype(np.int32)
    n, fh, fw = p.shape[:3]
    assert fh % 2 == 0 and fw % 2 == 0
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = _clip(((Y[0] * r + Y[1] * g + Y[2] * b + 128) >> 8) + y0).astype(np.uint8)
    u, v = chroma_unclipped(std, block_mean(p[..., :3]))
    uv = np.empty((n, fh // 2, fw), np.uint8)
    uv[:, :, 0::2] = _clip(u)
    uv[:, :, 1::2] = _clip(v)
    return y, uv
