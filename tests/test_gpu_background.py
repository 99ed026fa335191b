"""GPU parity of the virtual backgrounds (csrc/vss_background.hip) through the C
ABI against the numpy reference (tests/background_ref.py): colour, image and
blur compositing and vss_segment_background.  Every comparison is BIT-EXACT:
the blend and the blur are integer arithmetic, the alpha and the image scaling
are the oracle's own f32 recipe."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _frames(syn, seeds, h, w, c=3):
    return np.stack([syn.make_frame(int(s), h, w, c) for s in seeds])


def _alpha(seed, n, H, W):
    a = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    a[:, : H // 4] = 0
    a[:, -H // 4:] = 255
    return a


def _run(torch, pkg, s, bg, frames, alpha, pad_in=0, pad_out=0):
    """background_composite_device on padded rows into a 0xAB-filled buffer -> RGBA [n,fh,fw,4]."""
    n, fh, fw, c = frames.shape
    rs, ors = fw * c + pad_in, fw * 4 + pad_out
    padded = np.zeros((n, fh, rs), np.uint8)
    padded[:, :, :fw * c] = frames.reshape(n, fh, fw * c)
    df = torch.from_numpy(padded).cuda()
    da = torch.from_numpy(alpha).cuda()
    do = torch.full((n, fh, ors), 0xAB, dtype=torch.uint8, device="cuda")
    pkg.background_composite_device(s, bg, df.data_ptr(), n, fh, fw, c, rs, fh * rs, da.data_ptr(), do.data_ptr(),
                                    ors, fh * ors, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    assert np.all(got[:, :, fw * 4:] == 0xAB), "row padding was written"
    return got[:, :, :fw * 4].reshape(n, fh, fw, 4)


def _same(tag, got, want):
    bad = int((got != want).sum())
    assert bad == 0, f"{tag}: {bad} of {want.size} bytes differ"


@pytest.mark.parametrize("geom", [(2, 480, 640, 3, 144, 256, 0, 0), (3, 100, 150, 4, 48, 64, 40, 24),
                                  (2, 7, 5, 3, 48, 64, 0, 8), (1, 1080, 1920, 3, 144, 256, 0, 0)])
def test_colour_bitexact(pkg, torch_cuda, synthetic, oracle, geom):
    """The default (32, 32, 32) and a set colour; padded input rows, a width that
    is no multiple of 4, output rows that are not 16-byte aligned, a frame
    smaller than the mask and than one tile, 1080p."""
    n, fh, fw, c, H, W, pad_in, pad_out = geom
    frames = _frames(synthetic, range(80, 80 + n), fh, fw, c)
    alpha = _alpha(fh, n, H, W)
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        got = _run(torch_cuda, pkg, s, bg, frames, alpha, pad_in, pad_out)
        _same("default colour", got, ref.composite(oracle, frames, alpha, np.array([32, 32, 32])))
        bg.set_color(255, 0, 77)
        got = _run(torch_cuda, pkg, s, bg, frames, alpha, pad_in, pad_out)
        _same("set colour", got, ref.composite(oracle, frames, alpha, np.array([255, 0, 77])))


def test_image_bitexact_and_cache(pkg, torch_cuda, synthetic, oracle):
    """Upscaled, downscaled (RGBA, padded rows) and frame-sized images; one object
    at two frame sizes in turn and back (the cached scaled image is rebuilt per
    size); a new image and a colour each show in the next call."""
    H, W = 48, 64
    rng = np.random.default_rng(11)
    geoms = {"a": (2, 100, 150, 4, 40, 24), "b": (2, 37, 53, 3, 0, 8)}
    frames = {k: _frames(synthetic, range(60, 60 + g[0]), g[1], g[2], g[3]) for k, g in geoms.items()}
    alpha = {k: _alpha(g[1], g[0], H, W) for k, g in geoms.items()}
    up = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    wide = rng.integers(0, 256, (300, 500 * 4 + 20), dtype=np.uint8)
    down = wide[:, :2000].reshape(300, 500, 4)  # a view: rows 2020 bytes apart
    same = rng.integers(0, 256, (100, 150, 3), dtype=np.uint8)
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=2, autotune=False) as s:
        bg = pkg.Background(s)

        def check(tag, k, want_bg):
            g = geoms[k]
            got = _run(torch_cuda, pkg, s, bg, frames[k], alpha[k], g[4], g[5])
            _same(tag, got, ref.composite(oracle, frames[k], alpha[k], want_bg))

        bg.set_mode(pkg.VSS_BG_IMAGE)
        with pytest.raises(pkg.VssError) as e:  # image mode, no image yet
            _run(torch_cuda, pkg, s, bg, frames["b"], alpha["b"])
        assert e.value.code == pkg.VSS_E_INVALID_ARG and "no image" in str(e.value)
        for name, img in (("up", up), ("down", down)):
            bg.set_image(img)
            scaled = {k: ref.scale_image(oracle, img, geoms[k][1], geoms[k][2]) for k in geoms}
            for k in ("a", "b", "a"):
                check(f"{name} image at size {k}", k, scaled[k])
        bg.set_image(same)
        assert np.array_equal(ref.scale_image(oracle, same, 100, 150), same)
        check("frame-sized image", "a", same)
        bg.set_color(1, 2, 3)
        check("colour after image", "a", np.array([1, 2, 3]))
        bg.set_mode(pkg.VSS_BG_IMAGE)  # the image is still there
        check("back to the image", "b", ref.scale_image(oracle, same, 37, 53))


BLUR_GEOMS = [(2, 7, 5, 3, 0, 0), (3, 100, 150, 4, 40, 24), (2, 150, 270, 3, 0, 0)]


@pytest.fixture(scope="module")
def blur_inputs():
    """Noise frames (every tap matters), different per batch index; built once."""
    out = []
    for i, (n, fh, fw, c, _, _) in enumerate(BLUR_GEOMS):
        rng = np.random.default_rng(100 + i)
        out.append((rng.integers(0, 256, (n, fh, fw, c), dtype=np.uint8), _alpha(fh, n, 48, 64)))
    return out


@pytest.mark.parametrize("gi", range(len(BLUR_GEOMS)))
@pytest.mark.parametrize("radius,sigma", [(1, 0.5), (7, 2.5), (32, 10.0)])
def test_blur_bitexact(pkg, torch_cuda, oracle, blur_inputs, radius, sigma, gi):
    """A frame smaller than the radius, RGBA with padded rows, and several tiles in
    both directions with halos across tile borders and the frame's edges; the
    weights come from vss_blur_weights, so exp() rounding plays no part."""
    n, fh, fw, c, pad_in, pad_out = BLUR_GEOMS[gi]
    frames, alpha = blur_inputs[gi]
    want = ref.composite(oracle, frames, alpha, ref.blur(frames, pkg.blur_weights(radius, sigma)))
    with pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        bg.set_blur(radius, sigma)
        got = _run(torch_cuda, pkg, s, bg, frames, alpha, pad_in, pad_out)
    _same(f"blur r={radius}", got, want)


def test_blur_two_gpu_streams_without_a_host_wait(pkg, torch_cuda, oracle, blur_inputs):
    """One frame on one GPU stream, then two frames on another, nothing waited for in
    between: the horizontal pass's buffer has to grow for the second call while the
    first may still read it, and the second call's stream is ordered after the first's."""
    torch = torch_cuda
    _, fh, fw, c, _, _ = BLUR_GEOMS[2]
    frames, alpha = blur_inputs[2]
    w = pkg.blur_weights(7, 2.5)
    dev = [(torch.from_numpy(frames[:n]).cuda(), torch.from_numpy(alpha[:n]).cuda(),
            torch.zeros((n, fh, fw, 4), dtype=torch.uint8, device="cuda")) for n in (1, 2)]
    gpu_streams = (torch.cuda.Stream(), torch.cuda.Stream())
    with pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=4, autotune=False) as s:
        bg = pkg.Background(s)
        bg.set_blur(7, 2.5)
        torch.cuda.synchronize()
        for (df, da, do), st in zip(dev, gpu_streams):
            n = df.shape[0]
            pkg.background_composite_device(s, bg, df.data_ptr(), n, fh, fw, c, fw * c, fh * fw * c, da.data_ptr(),
                                            do.data_ptr(), fw * 4, fh * fw * 4, st.cuda_stream)
        torch.cuda.synchronize()
        got = [do.cpu().numpy() for _, _, do in dev]
    for n, g in zip((1, 2), got):
        _same(f"blur, {n} frame(s) on their own GPU stream", g,
              ref.composite(oracle, frames[:n], alpha[:n], ref.blur(frames[:n], w)))


def test_replace_background_end_to_end(pkg, torch_cuda, synthetic, oracle):
    """Seam + post chain + background in one call == oracle.post on the GPU's own
    masks, then the reference composite; two calls of one stream per mode."""
    image = np.random.default_rng(3).integers(0, 256, (90, 160, 3), dtype=np.uint8)
    with pkg.Session(dtype="bf16x2", max_batch=4, max_frame_h=480, max_frame_w=640) as s:
        bytes_before = s.device_bytes
        for mode in ("blur", "image"):
            chain = pkg.PostChain(s)
            bg = pkg.Background(s)
            if mode == "blur":
                bg.set_blur(7, 2.5)
            else:
                bg.set_image(image)
            st = oracle.PostState(s.mask_h, s.mask_w)
            for call in range(2):
                frames = _frames(synthetic, range(90 + 4 * call, 94 + 4 * call), 240, 320, 4)
                masks = s.segment_frames(frames)[0].reshape(4, s.mask_h, s.mask_w)
                got = chain.replace_background(frames, bg)
                _, want_u = oracle.post(masks, frames, st)
                want_bg = (ref.blur(frames, pkg.blur_weights(7, 2.5)) if mode == "blur"
                           else ref.scale_image(oracle, image, 240, 320))
                _same(f"{mode} call {call}", got, ref.composite(oracle, frames, want_u, want_bg))
            with pytest.raises(pkg.VssError):  # more output than the handle holds
                chain.replace_background(np.zeros((4, 1080, 1920, 3), np.uint8), bg)
        import ctypes
        info = pkg._Info()
        assert pkg.lib().vss_get_info(s._h, ctypes.byref(info)) == pkg.VSS_OK
        assert info.device_bytes > bytes_before  # the backgrounds' buffers are counted


def test_background_errors(pkg, torch_cuda):
    torch = torch_cuda
    L = pkg.lib()
    with pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=2, autotune=False) as s1, \
            pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=2, autotune=False) as s2:
        bg = pkg.Background(s1)
        chain2 = pkg.PostChain(s2)
        df = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
        da = torch.zeros((1, 48, 64), dtype=torch.uint8, device="cuda")
        do = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda")

        def device_call(sess, channels=3, row_stride=24):
            return L.vss_background_composite_device(sess._h, bg._bg, df.data_ptr(), 1, 8, 8, channels, row_stride,
                                                     8 * row_stride, da.data_ptr(), do.data_ptr(), 32, 256, None)

        assert device_call(s2) == pkg.VSS_E_INVALID_ARG  # a background of another handle
        assert b"background" in L.vss_last_error(s2._h)
        f = np.zeros((1, 8, 8, 3), np.uint8)
        out = np.zeros((1, 8, 8, 4), np.uint8)
        assert L.vss_segment_background(s2._h, chain2._st, bg._bg, f.ctypes.data, 1, 8, 8, 3, 24,
                                        out.ctypes.data) == pkg.VSS_E_INVALID_ARG
        assert device_call(s1, channels=2, row_stride=16) == pkg.VSS_E_INVALID_ARG
        assert b"channels" in L.vss_last_error(s1._h)
        assert device_call(s1) == pkg.VSS_OK
        torch.cuda.synchronize()
        for rgb in [(-1, 0, 0), (0, 256, 0), (0, 0, 1000)]:
            with pytest.raises(pkg.VssError) as e:
                bg.set_color(*rgb)
            assert e.value.code == pkg.VSS_E_INVALID_ARG and "colour" in str(e.value)
        img = np.zeros((4, 4, 2), np.uint8)
        assert L.vss_background_set_image(bg._bg, img.ctypes.data, 4, 4, 2, 8) == pkg.VSS_E_INVALID_ARG
        assert b"channels" in L.vss_last_error(s1._h)
        for radius, sigma in [(0, 1.0), (33, 1.0), (4, 0.0), (4, -1.0), (4, float("nan"))]:
            with pytest.raises(pkg.VssError) as e:
                bg.set_blur(radius, sigma)
            assert e.value.code == pkg.VSS_E_INVALID_ARG and ("radius" in str(e.value) or "sigma" in str(e.value))
        with pytest.raises(pkg.VssError):
            bg.set_mode(3)
        assert device_call(s1) == pkg.VSS_OK  # the failed setters changed nothing
        torch.cuda.synchronize()
        assert np.all(do.cpu().numpy()[..., :3] == 32)
