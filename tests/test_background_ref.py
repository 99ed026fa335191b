"""CPU tests of the virtual backgrounds: the host-only weight table of the blur
(vss_blur_weights), the numpy reference's own arithmetic (tests/background_ref.py)
and the ctypes surface.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WEIGHT_CASES = [(1, 0.5), (3, 1.0), (8, 3.0), (16, 5.5), (32, 10.0), (32, 40.0)]


@pytest.mark.parametrize("radius,sigma", WEIGHT_CASES)
def test_blur_weights(pkg, radius, sigma):
    """The table sums to 65536, is symmetric, non-increasing away from the
    centre, every off-centre tap within 1 of numpy's, the centre = 65536 - rest.

    At (32, 40.0) plain rounding leaves the centre at 1116 between two taps of
    1120 (the 64 rounded taps sum to 64420); the library then lowers the two
    innermost tap pairs by 1, which is what the tolerance of 1 is there for."""
    w = pkg.blur_weights(radius, sigma).astype(np.int64)
    want = ref.numpy_blur_weights(radius, sigma)
    print(f"r={radius} sigma={sigma}: sum={w.sum()} min={w.min()} centre={w[radius]} (numpy {want[radius]}) "
          f"neighbour={w[radius + 1]} max|w - numpy|={np.abs(w - want).max()}")
    assert w.shape == (2 * radius + 1,)
    assert w.sum() == 65536
    assert np.array_equal(w, w[::-1])
    off = np.arange(2 * radius + 1) != radius
    assert np.abs(w - want)[off].max() <= 1
    assert w[radius] == 65536 - w[off].sum()
    assert np.all(np.diff(w[radius:]) <= 0), f"not non-increasing from the centre: {w[radius:radius + 4]}"


def test_blur_weights_bad_arguments(pkg):
    L = pkg.lib()
    w = (ctypes.c_uint16 * 65)()
    for radius, sigma in [(0, 1.0), (33, 1.0), (3, 0.0), (3, -2.0), (3, float("nan"))]:
        assert L.vss_blur_weights(radius, sigma, w) == pkg.VSS_E_INVALID_ARG, (radius, sigma)
        with pytest.raises(pkg.VssError):
            pkg.blur_weights(radius, sigma)
    assert b"sigma" in L.vss_last_error(None)  # the last failure on this thread: the NaN
    assert L.vss_blur_weights(3, 1.0, None) == pkg.VSS_E_INVALID_ARG
    assert L.vss_blur_weights(3, 1.0, w) == pkg.VSS_OK


def test_blend_equals_u2frameproc_for_all_triples():
    """(fg*A + bg*(255-A) + 127) // 255 == Math.round((a*s/255 + (1-a)*b/255)*255),
    a = A/255, in JS doubles, for all 256^3 (A, fg, bg)."""
    s = np.arange(256, dtype=np.float64)[:, None]
    b = np.arange(256, dtype=np.float64)[None, :]
    mism = 0
    for A in range(256):
        a = A / 255
        js = np.floor((a * s / 255 + (1 - a) * b / 255) * 255 + 0.5)  # Math.round: ties toward +inf
        got = ref.blend(s, b, A)
        mism += int((js != got).sum())
    assert mism == 0


def test_blend_endpoints():
    v = np.arange(256)
    assert np.array_equal(ref.blend(v[:, None], v[None, :], 0), np.broadcast_to(v[None, :], (256, 256)))
    assert np.array_equal(ref.blend(v[:, None], v[None, :], 255), np.broadcast_to(v[:, None], (256, 256)))


@pytest.mark.parametrize("radius,sigma", [(1, 0.5), (7, 2.5), (32, 10.0)])
def test_blur_of_a_constant_is_the_constant(radius, sigma):
    w = ref.numpy_blur_weights(radius, sigma)
    for v in (0, 1, 127, 254, 255):
        img = np.full((1, 9, 11, 3), v, np.uint8)
        assert np.all(ref.blur(img, w) == v)


def test_blur_replicates_edges():
    w = ref.numpy_blur_weights(2, 1.0)
    img = np.zeros((1, 1, 6, 3), np.uint8)
    img[0, 0, 0] = 255  # the left edge's value also stands left of the image
    h = ref.blur(img, w)[0, 0, :, 0].astype(np.int64)
    first = (255 * int(w[:3].sum()) + 32768) >> 16  # taps -2, -1, 0 all read pixel 0 (one row: the vertical pass
    assert h[0] == (first * 65536 + 32768) >> 16    # sees the same value on every tap)
    assert h[3] == 0


def test_scaling_to_the_same_size_is_the_identity(oracle):
    rng = np.random.default_rng(5)
    for shape in [(7, 5, 3), (37, 53, 4)]:
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(ref.scale_image(oracle, img, shape[0], shape[1]), img[..., :3])


def test_new_abi_names_have_ctypes_signatures(pkg):
    src = open(os.path.join(ROOT, "include", "vss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = [s for s in set(re.findall(r"\b(vss_[a-z_]+)\s*\(", src)) if "background" in s or "blur" in s]
    assert len(names) == 9, sorted(names)
    L = pkg.lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature in lib()"
