"""Properties of the edge-aware matte's definition (tests/matte_ref.py,
include/vss.h): what the numpy reference, which the GPU must match bit for bit,
does on inputs whose true frame-resolution edge is known.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_ref as ref  # noqa: E402


def test_matte_abi_is_declared_exported_and_bound(pkg):
    """Every entry point include/vss_matte.h declares is reachable through
    include/vss.h, exported by the library and has a ctypes signature."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '#include "vss_matte.h"' in open(os.path.join(root, "include", "vss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vss_matte.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vss_[a-z_]+)\s*\(", src)))
    assert names == ["vss_background_alpha_device", "vss_background_alpha_device_at", "vss_background_set_refine"]
    L = pkg.lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature in lib()"


def _grey(img):
    """[fh,fw] grey levels -> one RGB frame [1,fh,fw,3] (its luma is the grey level)."""
    return np.repeat(np.asarray(img, np.uint8)[None, :, :, None], 3, axis=3)


def test_luma_of_grey_is_grey():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(ref.luma(_grey(g))[0], g)


def test_guide_footprints():
    """Non-integer ratios: every frame pixel belongs to exactly one footprint, and
    the mean rounds half up."""
    Y = np.arange(45 * 100, dtype=np.int64).reshape(1, 45, 100) % 256
    L = ref.guide(Y, 12, 16)
    for i, j in ((0, 0), (5, 7), (11, 15)):
        blk = Y[0, i * 45 // 12:(i + 1) * 45 // 12, j * 100 // 16:(j + 1) * 100 // 16]
        assert L[0, i, j] == int(np.floor(blk.sum() / blk.size + 0.5))
    assert np.array_equal(ref.guide(Y, 45, 100), Y)  # ratio 1: one pixel per footprint


def test_box_sum_clips_at_every_edge():
    x = np.arange(5 * 7, dtype=np.int64).reshape(1, 5, 7)
    for r in (1, 3, 8):
        want = np.array([[x[0, max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1].sum() for j in range(7)]
                         for i in range(5)])
        assert np.array_equal(ref.box_sum(x, r)[0], want)


@pytest.mark.parametrize("c", [0, 173, 255])
def test_constant_alpha_is_kept(oracle, c):
    frames = np.random.default_rng(c).integers(0, 256, (2, 45, 100, 3), dtype=np.uint8)
    p = np.full((2, 12, 16), c, np.uint8)
    for r in (1, 4, 8):
        for eps in (1.0, 16.0, 650.0):
            A = ref.alpha(oracle, frames, p, r, eps)
            assert np.all(A == c), f"c={c} r={r} eps={eps}: {np.unique(A)}"


def test_step_edge_is_placed_where_the_frame_has_it(oracle):
    """A vertical edge at frame column 53, inside mask column 8 (columns 50..55):
    the low-resolution alpha is the antialiased edge, the refined alpha puts the
    step back on column 53; the plain upscale cannot."""
    fh, fw, H, W = 45, 100, 12, 16
    img = np.full((fh, fw), 30, np.uint8)
    img[:, 53:] = 220
    frames = _grey(img)
    ideal = np.where(img == 220, 255, 0).astype(np.int64)
    L = ref.guide(ref.luma(frames), H, W)
    p = np.clip(np.floor((L - 30) * 255 / 190 + 0.5), 0, 255).astype(np.uint8)
    for r, eps in ((1, 1.0), (2, 16.0), (4, 16.0), (8, 16.0)):
        A = ref.alpha(oracle, frames, p, r, eps)[0].astype(np.int64)
        err = int(np.abs(A - ideal).max())
        print(f"step r={r} eps={eps}: max |A - ideal| = {err}")
        assert err <= 4
    plain = int(np.abs(ref.plain_alpha(oracle, frames, p)[0].astype(np.int64) - ideal).max())
    print(f"step plain upscale: max error = {plain}")
    assert plain >= 100


def test_disc(oracle):
    """A disc of grey 200 on grey 40; p = the area mean of the true alpha."""
    fh, fw, H, W = 270, 480, 36, 64
    y, x = np.mgrid[0:fh, 0:fw]
    inside = (y - 130.3) ** 2 + (x - 241.7) ** 2 <= 90.5 ** 2
    frames = _grey(np.where(inside, 200, 40))
    ideal = np.where(inside, 255, 0).astype(np.int64)
    p = ref.guide(ideal[None], H, W).astype(np.uint8)
    perr = np.abs(ref.plain_alpha(oracle, frames, p)[0].astype(np.int64) - ideal)
    print(f"disc plain: max {perr.max()} mean {perr.mean():.3f} over32 {(perr > 32).sum()}")
    for r, eps in ((2, 16.0), (4, 16.0)):
        err = np.abs(ref.alpha(oracle, frames, p, r, eps)[0].astype(np.int64) - ideal)
        print(f"disc r={r}: max {err.max()} mean {err.mean():.3f}")
        assert err.max() <= 32
        assert err.mean() <= perr.mean() / 4


def test_range_on_checkerboards(oracle):
    """The steepest fit the definition allows: L a 0/255 checkerboard, p its
    inverse, eps = 1.  The reference's int32 range asserts hold."""
    H, W, fh, fw = 12, 16, 45, 100
    i, j = np.mgrid[0:H, 0:W]
    L = np.where((i + j) % 2 == 0, 255, 0)[None]
    p = 255 - L
    Y = np.random.default_rng(5).integers(0, 256, (1, fh, fw))
    for r in (1, 4, 8):
        abar, bbar = ref.coefficients(L, p, r, 1.0)
        assert np.abs(abar).max() <= 64.0
        A = ref.apply(oracle, abar, bbar, Y)
        assert A.dtype == np.uint8 and A.shape == (1, fh, fw)  # clamped to 0..255 by definition
        assert A.min() == 0 and A.max() == 255  # and the clamp is reached at both ends
