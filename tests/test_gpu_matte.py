"""GPU parity of the edge-aware matte (csrc/vss_matte.hip and the REFINE forms of
k_bg_composite) through the C ABI against the numpy reference
(tests/matte_ref.py).  Every comparison is BIT-EXACT: integers, doubles in one
prescribed order and the oracle's own f32 upscale recipe."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref as bref  # noqa: E402
import matte_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, fh, fw, c, H, W, r, pad_in, pad_out)
GEOMS = [
    (2, 45, 100, 3, 12, 16, 1, 0, 0),       # non-integer ratios in both axes
    (3, 100, 150, 4, 48, 64, 4, 40, 10),    # RGBA, padded input rows, width no multiple of 4
    (1, 64, 64, 3, 64, 64, 8, 0, 0),        # ratio 1: every footprint is one pixel
    (2, 37, 53, 3, 5, 7, 8, 0, 3),          # mask < window: every window clipped on all four sides; frame < tile
    (2, 480, 640, 3, 144, 256, 2, 0, 0),    # the product's shape
    (1, 1080, 1920, 3, 144, 256, 4, 0, 0),
    (2, 61, 78, 3, 48, 64, 3, 2, 2),       # RGB rows on dwords (the guide's 4-pixel loads) with a 2-pixel tail
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _alpha(seed, n, H, W):
    a = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    a[:, : H // 4] = 0
    a[:, -(H // 4):] = 255
    return a


_inputs = {}


def _geom_inputs(synthetic, gi):
    """Frames (synthetic scenes for the odd geometries, noise for the even ones, so
    that both smooth and busy guides are fitted) and alpha bytes; built once."""
    if gi not in _inputs:
        n, fh, fw, c, H, W = GEOMS[gi][:6]
        if gi % 2:
            frames = np.stack([synthetic.make_frame(300 + 10 * gi + i, fh, fw, c) for i in range(n)])
        else:
            frames = np.random.default_rng(200 + gi).integers(0, 256, (n, fh, fw, c), dtype=np.uint8)
        _inputs[gi] = (frames, _alpha(50 + gi, n, H, W))
    return _inputs[gi]


def _session(pkg, H, W, max_batch=4):
    """A handle for an H x W mask; masks that are no multiple of 16 (which no handle
    has as its model size) go through the explicit-size entry point instead."""
    own = H % 16 == 0 and W % 16 == 0
    s = pkg.Session(model_h=H if own else 48, model_w=W if own else 64, dtype="f32", max_batch=max_batch,
                    autotune=False)
    return s, (None if own else (H, W))


def _upload(torch, frames, alpha, pad_in):
    n, fh, fw, c = frames.shape
    rs = fw * c + pad_in
    padded = np.zeros((n, fh, rs), np.uint8)
    padded[:, :, :fw * c] = frames.reshape(n, fh, fw * c)
    return torch.from_numpy(padded).cuda(), torch.from_numpy(alpha).cuda(), rs


def _run_alpha(torch, pkg, s, bg, frames, alpha, pad_in=0, pad_out=0, mask_hw=None):
    """background_alpha_device into a 0xAB-filled padded buffer -> [n,fh,fw] u8."""
    n, fh, fw, c = frames.shape
    df, da, rs = _upload(torch, frames, alpha, pad_in)
    ors = fw + pad_out
    do = torch.full((n, fh, ors), 0xAB, dtype=torch.uint8, device="cuda")
    pkg.background_alpha_device(s, bg, df.data_ptr(), n, fh, fw, c, rs, fh * rs, da.data_ptr(), do.data_ptr(), ors,
                                fh * ors, torch.cuda.current_stream().cuda_stream, mask_hw=mask_hw)
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    assert np.all(got[:, :, fw:] == 0xAB), "row padding was written"
    return got[:, :, :fw]


def _run_composite(torch, pkg, s, bg, frames, alpha, pad_in=0, pad_out=0):
    n, fh, fw, c = frames.shape
    df, da, rs = _upload(torch, frames, alpha, pad_in)
    ors = fw * 4 + pad_out
    do = torch.full((n, fh, ors), 0xAB, dtype=torch.uint8, device="cuda")
    pkg.background_composite_device(s, bg, df.data_ptr(), n, fh, fw, c, rs, fh * rs, da.data_ptr(), do.data_ptr(),
                                    ors, fh * ors, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    assert np.all(got[:, :, fw * 4:] == 0xAB), "row padding was written"
    return got[:, :, :fw * 4].reshape(n, fh, fw, 4)


def _same(tag, got, want):
    bad = int((got != want).sum())
    assert bad == 0, f"{tag}: {bad} of {want.size} bytes differ (max |d| = " \
                     f"{int(np.abs(got.astype(int) - want.astype(int)).max())})"


@pytest.mark.parametrize("eps", [1.0, 16.0])
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_alpha_plane_bitexact(pkg, torch_cuda, synthetic, oracle, gi, eps):
    n, fh, fw, c, H, W, r, pad_in, pad_out = GEOMS[gi]
    frames, alpha = _geom_inputs(synthetic, gi)
    want = ref.alpha(oracle, frames, alpha, r, eps)
    s, mask_hw = _session(pkg, H, W)
    with s:
        bg = pkg.Background(s)
        bg.set_refine(r, eps)
        got = _run_alpha(torch_cuda, pkg, s, bg, frames, alpha, pad_in, pad_out, mask_hw)
    _same(f"alpha geom {gi} eps {eps}", got, want)


def test_every_other_radius(pkg, torch_cuda, synthetic, oracle):
    """The fit kernels are compiled per radius: the ones no geometry above uses."""
    n, fh, fw, c, H, W, _, pad_in, pad_out = GEOMS[6]
    frames, alpha = _geom_inputs(synthetic, 6)
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        for r in (5, 6, 7):
            bg.set_refine(r, 650.0)
            _same(f"radius {r}", _run_alpha(torch_cuda, pkg, s, bg, frames, alpha, pad_in, pad_out),
                  ref.alpha(oracle, frames, alpha, r, 650.0))


@pytest.mark.parametrize("gi", [1, 4])
def test_composite_refined_bitexact(pkg, torch_cuda, synthetic, oracle, gi):
    """Colour, image and blur (radius 7, sigma 2.5) with refinement on ==
    blend(frame, bg, A_ref), output alpha 255."""
    n, fh, fw, c, H, W, r, pad_in, _ = GEOMS[gi]
    frames, alpha = _geom_inputs(synthetic, gi)
    image = np.random.default_rng(17).integers(0, 256, (60, 90, 3), dtype=np.uint8)
    w = pkg.blur_weights(7, 2.5)
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        bg.set_refine(r, 16.0)
        bg.set_color(255, 0, 77)
        _same("colour", _run_composite(torch_cuda, pkg, s, bg, frames, alpha, pad_in, 24),
              ref.composite(oracle, frames, alpha, np.array([255, 0, 77]), r, 16.0))
        bg.set_image(image)
        _same("image", _run_composite(torch_cuda, pkg, s, bg, frames, alpha, pad_in, 24),
              ref.composite(oracle, frames, alpha, bref.scale_image(oracle, image, fh, fw), r, 16.0))
        bg.set_blur(7, 2.5)
        _same("blur", _run_composite(torch_cuda, pkg, s, bg, frames, alpha, pad_in, 24),
              ref.composite(oracle, frames, alpha, bref.blur(frames, w), r, 16.0))


def test_off_is_off(pkg, torch_cuda, synthetic, oracle):
    """Refinement on, a composite, off again: the next composite is today's bytes,
    and the alpha plane with refinement off is k_composite's alpha."""
    n, fh, fw, c, H, W, r, pad_in, _ = GEOMS[1]
    frames, alpha = _geom_inputs(synthetic, 1)
    plain = bref.composite(oracle, frames, alpha, np.array([32, 32, 32]))
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        bg.set_refine(4, 16.0)
        on = _run_composite(torch_cuda, pkg, s, bg, frames, alpha, pad_in)
        assert not np.array_equal(on, plain)
        bg.set_refine(0, 0.0)
        _same("composite after off", _run_composite(torch_cuda, pkg, s, bg, frames, alpha, pad_in), plain)
        _same("alpha plane, off", _run_alpha(torch_cuda, pkg, s, bg, frames, alpha, pad_in, 10),
              oracle.composite(frames, alpha)[..., 3])


def test_state_growth_and_sizes(pkg, torch_cuda, synthetic, oracle):
    """One object at n = 1 then n = 3 (the planes grow), at two frame sizes in turn
    and back; device_bytes grows when refinement first runs."""
    H, W = 48, 64
    fa, aa = _geom_inputs(synthetic, 1)  # 3 x 100 x 150 RGBA
    fb = np.random.default_rng(9).integers(0, 256, (2, 61, 77, 3), dtype=np.uint8)
    ab = _alpha(9, 2, H, W)

    def device_bytes(s):
        info = pkg._Info()
        assert pkg.lib().vss_get_info(s._h, ctypes.byref(info)) == pkg.VSS_OK
        return info.device_bytes

    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        _run_alpha(torch_cuda, pkg, s, bg, fa[:1], aa[:1])
        before = device_bytes(s)
        bg.set_refine(2, 16.0)
        assert device_bytes(s) == before  # nothing until it runs
        want_a, want_b = ref.alpha(oracle, fa, aa, 2, 16.0), ref.alpha(oracle, fb, ab, 2, 16.0)
        _same("n=1", _run_alpha(torch_cuda, pkg, s, bg, fa[:1], aa[:1]), want_a[:1])
        one = device_bytes(s)
        assert one > before
        _same("n=3", _run_alpha(torch_cuda, pkg, s, bg, fa, aa), want_a)
        assert device_bytes(s) > one
        _same("size b", _run_alpha(torch_cuda, pkg, s, bg, fb, ab), want_b)
        _same("back to size a", _run_alpha(torch_cuda, pkg, s, bg, fa, aa), want_a)
        _same("n=1 again", _run_alpha(torch_cuda, pkg, s, bg, fa[1:2], aa[1:2]), want_a[1:2])


def test_refine_errors(pkg, torch_cuda):
    torch = torch_cuda
    L = pkg.lib()
    with pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=2, autotune=False) as s:
        bg = pkg.Background(s)
        for radius, eps in [(-1, 16.0), (9, 16.0), (4, 0.5), (4, 70000.0), (4, float("nan")), (4, float("inf"))]:
            with pytest.raises(pkg.VssError) as e:
                bg.set_refine(radius, eps)
            assert e.value.code == pkg.VSS_E_INVALID_ARG and ("radius" in str(e.value) or "eps" in str(e.value))
        df = torch.zeros((1, 40, 80, 3), dtype=torch.uint8, device="cuda")  # 40 < 48 rows
        da = torch.zeros((1, 48, 64), dtype=torch.uint8, device="cuda")
        do = torch.zeros((1, 40, 80, 4), dtype=torch.uint8, device="cuda")

        def composite():
            return L.vss_background_composite_device(s._h, bg._bg, df.data_ptr(), 1, 40, 80, 3, 240, 9600,
                                                     da.data_ptr(), do.data_ptr(), 320, 12800, None)

        def plane():
            return L.vss_background_alpha_device(s._h, bg._bg, df.data_ptr(), 1, 40, 80, 3, 240, 9600,
                                                 da.data_ptr(), do.data_ptr(), 80, 3200, None)

        assert composite() == pkg.VSS_OK  # the failed setters left refinement off
        bg.set_refine(4, 16.0)
        assert composite() == pkg.VSS_E_INVALID_ARG
        assert b"smaller" in L.vss_last_error(s._h)
        assert plane() == pkg.VSS_E_INVALID_ARG
        bg.set_refine(0, 0.0)
        assert composite() == pkg.VSS_OK and plane() == pkg.VSS_OK
        torch.cuda.synchronize()
        assert np.all(do.cpu().numpy().reshape(-1)[:3200] == 0)  # alpha 0 everywhere


def test_replace_background_refined_end_to_end(pkg, torch_cuda, synthetic, oracle):
    """Seam + post chain + refined background in one call, two consecutive batches
    of one stream == the reference over the oracle's post alpha."""
    with pkg.Session(dtype="bf16x2", max_batch=4, max_frame_h=480, max_frame_w=640) as s:
        chain = pkg.PostChain(s)
        bg = pkg.Background(s)
        bg.set_color(10, 200, 90)
        bg.set_refine(2, 16.0)
        st = oracle.PostState(s.mask_h, s.mask_w)
        for call in range(2):
            frames = np.stack([synthetic.make_frame(130 + 4 * call + i, 240, 320, 4) for i in range(4)])
            masks = s.segment_frames(frames)[0].reshape(4, s.mask_h, s.mask_w)
            got = chain.replace_background(frames, bg)
            _, want_u = oracle.post(masks, frames, st)
            _same(f"call {call}", got, ref.composite(oracle, frames, want_u, np.array([10, 200, 90]), 2, 16.0))
