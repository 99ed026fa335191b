"""Properties of the NV12 conversion's definition (tests/video_ref.py,
include/vss_video.h), which the GPU must match bit for bit, and the parts of
the video ABI that need no GPU.  CPU only."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lattice(step=3):
    """The RGB lattice of that step plus 255 on every axis, as one frame [1, 2, K, 3]
    whose 2x2 blocks are uniform (so the block mean is the colour itself)."""
    ax = np.unique(np.append(np.arange(0, 256, step), 255))
    rgb = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return np.repeat(np.repeat(rgb[None, None], 2, axis=1), 2, axis=2).astype(np.uint8)


def test_video_abi_is_declared_exported_and_bound(pkg):
    """Every entry point include/vss_video.h declares is reachable through
    include/vss.h, exported by the library and has a ctypes signature."""
    assert '#include "vss_video.h"' in open(os.path.join(ROOT, "include", "vss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vss_video.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vss_[a-z0-9_]+)\s*\(", src)))
    assert names == ["vss_nv12_to_rgba_device", "vss_rgba_to_nv12_device", "vss_video_create", "vss_video_destroy",
                     "vss_video_process", "vss_video_process_device", "vss_video_set_standard"]
    L = pkg.lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature in lib()"
    for i, name in enumerate(("VSS_CSC_BT601_LIMITED", "VSS_CSC_BT709_LIMITED", "VSS_CSC_BT601_FULL",
                              "VSS_CSC_BT709_FULL")):
        assert re.search(rf"#define {name} {i}\b", src) and getattr(pkg, name) == i == getattr(ref, name[8:])


def test_header_table_is_the_reference_table():
    """The table in vss_video.h's comment, row by row, is video_ref.TABLE."""
    text = open(os.path.join(ROOT, "include", "vss_video.h")).read()
    for std, name in enumerate(("BT601_LIMITED", "BT709_LIMITED", "BT601_FULL", "BT709_FULL")):
        row = re.search(rf"\*\s+{name}\s+((?:-?\d+\s+){{14}}-?\d+)\s*$", text, flags=re.M)
        assert row, name
        v = [int(t) for t in row.group(1).split()]
        t = ref.TABLE[std]
        assert v == list(t[:6]) + list(t[6]) + list(t[7]) + list(t[8]), name


@pytest.mark.parametrize("std", ref.STANDARDS)
def test_row_sums(std):
    Y, U, V = ref.TABLE[std][6:]
    assert sum(Y) == (220 if std in ref.LIMITED else 256)
    assert sum(U) == 0 and sum(V) == 0


@pytest.mark.parametrize("std", ref.STANDARDS)
def test_greys_have_neutral_chroma(std):
    g = np.arange(256, dtype=np.uint8)
    rgb = np.repeat(np.repeat(np.repeat(g[None, None, :, None], 3, axis=3), 2, axis=1), 2, axis=2)
    y, uv = ref.pack(std, rgb)
    assert np.all(uv == 128)
    assert np.all(np.diff(y[0, 0].astype(int)) >= 0)
    assert (y.min(), y.max()) == ((16, 235) if std in ref.LIMITED else (0, 255))


@pytest.mark.parametrize("std", [ref.BT601_FULL, ref.BT709_FULL])
def test_full_range_chroma_needs_the_clamp(std):
    """Pure blue's U and pure red's V are 256 before the clamp and 255 after it."""
    px = np.zeros((1, 2, 4, 3), np.uint8)
    px[0, :, 0:2] = (0, 0, 255)
    px[0, :, 2:4] = (255, 0, 0)
    u, v = ref.chroma_unclipped(std, ref.block_mean(px))
    assert u[0, 0, 0] == 256 and v[0, 0, 1] == 256
    _, uv = ref.pack(std, px)
    assert uv[0, 0, 0] == 255 and uv[0, 0, 3] == 255
    # nothing else on the lattice leaves 0..255, and only at these two ends
    u, v = ref.chroma_unclipped(std, _lattice()[:, :1, 0::2])
    assert u.min() >= 0 and v.min() >= 0 and u.max() == 256 and v.max() == 256


@pytest.mark.parametrize("std", ref.LIMITED)
def test_limited_ranges(std):
    y, uv = ref.pack(std, _lattice())
    assert (y.min(), y.max()) == (16, 235)
    assert (uv.min(), uv.max()) == (16, 240)
    u, v = ref.chroma_unclipped(std, _lattice()[:, :1, 0::2])
    assert u.min() == 16 and u.max() == 240 and v.min() == 16 and v.max() == 240  # the clamp never acts


@pytest.mark.parametrize("std", ref.STANDARDS)
def test_round_trip_bound(std):
    """RGB -> NV12 -> RGB over the greys and the lattice (uniform blocks): within
    3 per channel for the limited standards, 2 for the full ones."""
    g = np.arange(256, dtype=np.uint8)
    greys = np.repeat(np.repeat(np.repeat(g[None, None, :, None], 3, axis=3), 2, axis=1), 2, axis=2)
    bound = 3 if std in ref.LIMITED else 2
    for rgb in (greys, _lattice()):
        back = ref.unpack(std, *ref.pack(std, rgb))
        assert np.all(back[..., 3] == 255)
        err = int(np.abs(back[..., :3].astype(int) - rgb.astype(int)).max())
        print(f"std {std}: round trip max error {err}")
        assert err <= bound


def test_chroma_is_taken_from_the_rounded_block_mean():
    """Four different pixels, BT.601 limited, by hand.
    means: R (107+29+116+156+2)>>2 = 102, G (132+108+198+197+2)>>2 = 159, B (74+159+92+234+2)>>2 = 140
    U = ((-38*102 - 74*159 + 112*140 + 128) >> 8) + 128 = (166 >> 8) + 128 = 0 + 128 = 128
    V = ((112*102 - 94*159 - 18*140 + 128) >> 8) + 128 = (-5914 >> 8) + 128 = -24 + 128 = 104
    Y00 = ((66*107 + 129*132 + 25*74 + 128) >> 8) + 16 = (26068 >> 8) + 16 = 101 + 16 = 117
    Converting each pixel and averaging afterwards gives V = (121+90+100+107+2)>>2 = 105."""
    px = np.array([[[[107, 132, 74, 9], [29, 108, 159, 99]], [[116, 198, 92, 0], [156, 197, 234, 255]]]], np.uint8)
    assert ref.block_mean(px[..., :3]).tolist() == [[[[102, 159, 140]]]]
    y, uv = ref.pack(ref.BT601_LIMITED, px)
    assert uv.tolist() == [[[128, 104]]]
    assert y[0, 0, 0] == 117
    _, v4 = ref.chroma_unclipped(ref.BT601_LIMITED, px[..., :3])
    assert v4.tolist() == [[[121, 90], [100, 107]]] and (int(v4.sum()) + 2) >> 2 == 105
    # the alpha byte is ignored
    px2 = px.copy()
    px2[..., 3] = 77
    y2, uv2 = ref.pack(ref.BT601_LIMITED, px2)
    assert np.array_equal(y, y2) and np.array_equal(uv, uv2)


def test_unpack_replicates_chroma_over_the_block():
    y = np.full((1, 4, 4), 128, np.uint8)
    uv = np.array([[[90, 200, 128, 128], [30, 40, 240, 16]]], np.uint8)
    out = ref.unpack(ref.BT709_LIMITED, y, uv)
    for by in range(2):
        for bx in range(2):
            blk = out[0, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2].reshape(4, 4)
            assert np.all(blk == blk[0])
    # by hand, block (0, 0): c = 298*112 = 33376, d = -38, e = 72
    #   R = (33376 + 459*72 + 128) >> 8 = 66552 >> 8 = 259 -> 255
    #   G = (33376 + 55*38 - 136*72 + 128) >> 8 = 25802 >> 8 = 100
    #   B = (33376 - 541*38 + 128) >> 8 = 12946 >> 8 = 50
    assert out[0, 0, 0].tolist() == [255, 100, 50, 255]


def test_host_validation_without_a_gpu(pkg):
    """What is rejected before any device is touched: null objects in the C ABI
    and malformed arrays or names in the Python host."""
    L = pkg.lib()
    out = ctypes.c_void_p(0x1)
    assert L.vss_video_create(None, 1, ctypes.byref(out)) == pkg.VSS_E_INVALID_ARG
    assert L.vss_video_set_standard(None, 1) == pkg.VSS_E_INVALID_ARG
    L.vss_video_destroy(None)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.vss_nv12_to_rgba_device(None, 1, p, 2, 4, p, 2, 2, 1, 2, 2, p, 8, 16, None) == pkg.VSS_E_INVALID_ARG
    assert L.vss_rgba_to_nv12_device(None, 1, p, 8, 16, 1, 2, 2, p, 2, 4, p, 2, 2, None) == pkg.VSS_E_INVALID_ARG
    assert L.vss_video_process_device(None, None, None, p, 2, 4, p, 2, 2, 1, 2, 2, p, 2, 4, p, 2, 2,
                                      None) == pkg.VSS_E_INVALID_ARG
    assert L.vss_video_process(None, None, None, p, p, 1, 2, 2, p, p) == pkg.VSS_E_INVALID_ARG
    assert not buf.any()
    with pytest.raises(pkg.VssError):
        pkg._csc("bt2020")
    assert pkg._csc("bt709") == 1 and pkg._csc("bt601-full") == 2 and pkg._csc(3) == 3
    y, uv = np.zeros((2, 4, 6), np.uint8), np.zeros((2, 2, 6), np.uint8)
    ya, ua = pkg._as_nv12(y, uv)
    assert ya.shape == (2, 4, 6) and ua.shape == (2, 2, 6)
    for bad_y, bad_uv in ((y.astype(np.int32), uv), (y[0], uv[0]), (y, uv[:, :1]), (y[:, :3], uv[:, :1]),
                          (y[:, :, :5], uv[:, :, :5]), (y[:, :0], uv[:, :0])):
        with pytest.raises(pkg.VssError):
            pkg._as_nv12(bad_y, bad_uv)
