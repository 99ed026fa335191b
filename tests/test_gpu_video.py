"""GPU parity of the NV12 video I/O (csrc/vss_video.hip and the vss_video_* calls
of include/vss_video.h) through the C ABI against the numpy reference
(tests/video_ref.py).  Every comparison is BIT-EXACT over whole buffers: the
expected buffer holds 0xAB wherever nothing may be written."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_ref as bg_ref  # noqa: E402
import video_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, fh, fw)
GEOMS = [
    (1, 2, 2),          # one block
    (2, 4, 6),          # only the scalar tail runs
    (2, 100, 150),      # width no multiple of 8: vector footprints and a tail, several row groups
    (2, 480, 640),      # several workgroups in x and y
    (1, 1080, 1920),
]
FILL = 0xAB


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def sess(pkg, torch_cuda):
    with pkg.Session(model_h=48, model_w=64, dtype="f32", autotune=False) as s:
        yield s


class Layout:
    """Where a batch's planes sit in their buffers: tight, or with padded pitches,
    gaps between frames and base pointers off every vector alignment."""

    def __init__(self, n, fh, fw, padded):
        self.n, self.fh, self.fw = n, fh, fw
        if padded:
            self.yp, self.up, self.rs = fw + 13, fw + 6, 4 * fw + 8
            self.yfs, self.ufs, self.fs = self.yp * fh + 3, self.up * (fh // 2) + 5, self.rs * fh + 4
            self.off, self.roff = 1, 4
        else:
            self.yp, self.up, self.rs = fw, fw, 4 * fw
            self.yfs, self.ufs, self.fs = fw * fh, fw * (fh // 2), 4 * fw * fh
            self.off, self.roff = 0, 0

    def _place(self, a, off, pitch, fs, rows, rowbytes):
        buf = np.full(off + self.n * fs, FILL, np.uint8)
        for t in range(self.n):
            v = buf[off + t * fs: off + t * fs + rows * pitch].reshape(rows, pitch)
            v[:, :rowbytes] = a[t].reshape(rows, rowbytes)
        return buf

    def y_buf(self, y):
        return self._place(y, self.off, self.yp, self.yfs, self.fh, self.fw)

    def uv_buf(self, uv):
        return self._place(uv, self.off, self.up, self.ufs, self.fh // 2, self.fw)

    def rgba_buf(self, rgba):
        return self._place(rgba, self.roff, self.rs, self.fs, self.fh, 4 * self.fw)

    def blank(self, kind):
        size = {"y": self.off + self.n * self.yfs, "uv": self.off + self.n * self.ufs,
                "rgba": self.roff + self.n * self.fs}[kind]
        return np.full(size, FILL, np.uint8)


_cache = {}


def _nv12_input(gi):
    """Random bytes plus, block by block from the top left, the saturated corners:
    Y in {0, 16, 235, 255} x U, V in {0, 16, 128, 240, 255} (as many as the frame holds)."""
    key = ("nv12", gi)
    if key not in _cache:
        n, fh, fw = GEOMS[gi]
        rng = np.random.default_rng(900 + gi)
        y = rng.integers(0, 256, (n, fh, fw), dtype=np.uint8)
        uv = rng.integers(0, 256, (n, fh // 2, fw), dtype=np.uint8)
        corners = [(a, b, c) for a in (0, 16, 235, 255) for b in (0, 16, 128, 240, 255) for c in (0, 16, 128, 240, 255)]
        for i, (a, b, c) in enumerate(corners[:(fh // 2) * (fw // 2)]):
            by, bx = divmod(i, fw // 2)
            y[:, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = a
            uv[:, by, 2 * bx] = b
            uv[:, by, 2 * bx + 1] = c
        _cache[key] = (y, uv)
    return _cache[key]


def _rgba_input(gi):
    """Random RGBA plus the eight corners of the RGB cube as uniform blocks (pure
    blue and pure red reach the pack's clamp in the full-range standards)."""
    key = ("rgba", gi)
    if key not in _cache:
        n, fh, fw = GEOMS[gi]
        px = np.random.default_rng(950 + gi).integers(0, 256, (n, fh, fw, 4), dtype=np.uint8)
        corners = [(0, 0, 255), (255, 0, 0)] + [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
        for i, c in enumerate(corners[:(fh // 2) * (fw // 2)]):
            by, bx = divmod(i, fw // 2)
            px[:, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2, :3] = c
        _cache[key] = px
    return _cache[key]


def _want(kind, gi, std):
    key = (kind, gi, std)
    if key not in _cache:
        _cache[key] = ref.unpack(std, *_nv12_input(gi)) if kind == "unpack" else ref.pack(std, _rgba_input(gi))
    return _cache[key]


def _same(tag, got, want):
    bad = int((got != want).sum())
    assert bad == 0, f"{tag}: {bad} of {want.size} bytes differ (max |d| = " \
                     f"{int(np.abs(got.astype(int) - want.astype(int)).max())})"


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("std", ref.STANDARDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_unpack_bitexact(pkg, torch_cuda, sess, gi, std, padded):
    torch = torch_cuda
    n, fh, fw = GEOMS[gi]
    y, uv = _nv12_input(gi)
    L = Layout(n, fh, fw, padded)
    dy, duv = torch.from_numpy(L.y_buf(y)).cuda(), torch.from_numpy(L.uv_buf(uv)).cuda()
    do = torch.from_numpy(L.blank("rgba")).cuda()
    pkg.nv12_to_rgba_device(sess, std, dy.data_ptr() + L.off, L.yp, L.yfs, duv.data_ptr() + L.off, L.up, L.ufs,
                            n, fh, fw, do.data_ptr() + L.roff, L.rs, L.fs, _stream(torch))
    torch.cuda.synchronize()
    _same(f"unpack std {std}", do.cpu().numpy(), L.rgba_buf(_want("unpack", gi, std)))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("std", ref.STANDARDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_pack_bitexact(pkg, torch_cuda, sess, gi, std, padded):
    torch = torch_cuda
    n, fh, fw = GEOMS[gi]
    L = Layout(n, fh, fw, padded)
    di = torch.from_numpy(L.rgba_buf(_rgba_input(gi))).cuda()
    dy, duv = torch.from_numpy(L.blank("y")).cuda(), torch.from_numpy(L.blank("uv")).cuda()
    pkg.rgba_to_nv12_device(sess, std, di.data_ptr() + L.roff, L.rs, L.fs, n, fh, fw, dy.data_ptr() + L.off, L.yp,
                            L.yfs, duv.data_ptr() + L.off, L.up, L.ufs, _stream(torch))
    torch.cuda.synchronize()
    wy, wuv = _want("pack", gi, std)
    _same(f"pack std {std} Y", dy.cpu().numpy(), L.y_buf(wy))
    _same(f"pack std {std} UV", duv.cpu().numpy(), L.uv_buf(wuv))
    if gi >= 2 and std in (ref.BT601_FULL, ref.BT709_FULL):  # the clamp was reached: pure blue's U, pure red's V
        assert wuv[0, 0, 0] == 255 and wuv[0, 0, 3] == 255


def _video_frames(synthetic, n, fh, fw, std, start):
    """Scenes with a person (so the alpha has an inside, an outside and an edge) as NV12."""
    rgb = np.stack([synthetic.make_frame(start + i, fh, fw, 3) for i in range(n)])
    return ref.pack(std, rgb)


def _process_device(torch, v, chain, bg, y, uv, padded=False):
    """Video.process_device on device copies of (y, uv) -> host (y, uv); whole output buffers checked for padding."""
    n, fh, fw = y.shape
    L = Layout(n, fh, fw, padded)
    dy, duv = torch.from_numpy(L.y_buf(y)).cuda(), torch.from_numpy(L.uv_buf(uv)).cuda()
    oy, ouv = torch.from_numpy(L.blank("y")).cuda(), torch.from_numpy(L.blank("uv")).cuda()
    v.process_device(chain, bg, dy.data_ptr() + L.off, L.yp, L.yfs, duv.data_ptr() + L.off, L.up, L.ufs, n, fh, fw,
                     oy.data_ptr() + L.off, L.yp, L.yfs, ouv.data_ptr() + L.off, L.up, L.ufs, _stream(torch))
    torch.cuda.synchronize()
    gy, guv = oy.cpu().numpy(), ouv.cpu().numpy()
    got_y = np.stack([gy[L.off + t * L.yfs: L.off + t * L.yfs + fh * L.yp].reshape(fh, L.yp)[:, :fw] for t in range(n)])
    got_uv = np.stack([guv[L.off + t * L.ufs: L.off + t * L.ufs + (fh // 2) * L.up].reshape(fh // 2, L.up)[:, :fw]
                       for t in range(n)])
    _same("output Y padding", gy, L.y_buf(got_y))
    _same("output UV padding", guv, L.uv_buf(got_uv))
    return got_y, got_uv


def _staged(torch, pkg, s, bg, std, y, uv):
    """The definition of the one-call path, run through the existing device entry
    points on the reference's unpacked RGBA, with a post state of its own."""
    n, fh, fw = y.shape
    st = _stream(torch)
    rgba = torch.from_numpy(ref.unpack(std, y, uv)).cuda()
    masks = torch.empty((n, s.mask_h * s.mask_w), dtype=torch.float32, device="cuda")
    alpha = torch.empty((n, s.mask_h * s.mask_w), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, fh, fw, 4), dtype=torch.uint8, device="cuda")
    chain = pkg.PostChain(s)
    s.segment_device(rgba.data_ptr(), n, fh, fw, 4, fw * 4, fh * fw * 4, masks.data_ptr(), st)
    chain.process_device(rgba.data_ptr(), n, fh, fw, 4, fw * 4, fh * fw * 4, masks.data_ptr(), 0, alpha.data_ptr(), st)
    pkg.background_composite_device(s, bg, rgba.data_ptr(), n, fh, fw, 4, fw * 4, fh * fw * 4, alpha.data_ptr(),
                                    out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    chain.close()
    return ref.pack(std, out.cpu().numpy())


@pytest.mark.parametrize("mode", ["colour", "blur", "image+refine"])
def test_one_call_equals_the_staged_calls(pkg, torch_cuda, sess, synthetic, mode):
    torch = torch_cuda
    std = {"colour": ref.BT709_LIMITED, "blur": ref.BT601_FULL, "image+refine": ref.BT601_LIMITED}[mode]
    y, uv = _video_frames(synthetic, 2, 100, 150, std, 40)
    bg = pkg.Background(sess)
    if mode == "colour":
        bg.set_color(10, 200, 90)
    elif mode == "blur":
        bg.set_blur(3, 1.5)
    else:
        bg.set_image(np.random.default_rng(4).integers(0, 256, (30, 40, 3), dtype=np.uint8))
        bg.set_refine(2, 16.0)
    v = pkg.Video(sess, std)
    chain = pkg.PostChain(sess)
    got_y, got_uv = _process_device(torch, v, chain, bg, y, uv, padded=(mode != "colour"))
    want_y, want_uv = _staged(torch, pkg, sess, bg, std, y, uv)
    _same(f"{mode} Y", got_y, want_y)
    _same(f"{mode} UV", got_uv, want_uv)
    assert not np.array_equal(got_y, y)  # a background was put in
    for o in (v, chain, bg):
        o.close()


def test_stream_state_carries_across_calls(pkg, torch_cuda, sess, synthetic):
    """Two calls of n = 2 on one stream and one post state == one call of n = 4."""
    torch = torch_cuda
    y, uv = _video_frames(synthetic, 4, 100, 150, ref.BT709_LIMITED, 60)
    bg = pkg.Background(sess)
    bg.set_color(0, 120, 255)
    v = pkg.Video(sess)
    one = pkg.PostChain(sess)
    want_y, want_uv = _process_device(torch, v, one, bg, y, uv)
    two = pkg.PostChain(sess)
    a = _process_device(torch, v, two, bg, y[:2], uv[:2])
    b = _process_device(torch, v, two, bg, y[2:], uv[2:])
    _same("Y", np.concatenate([a[0], b[0]]), want_y)
    _same("UV", np.concatenate([a[1], b[1]]), want_uv)
    # and the state matters: frames 2..3 from a fresh state are another result
    fresh = pkg.PostChain(sess)
    c = _process_device(torch, v, fresh, bg, y[2:], uv[2:])
    assert not (np.array_equal(c[0], b[0]) and np.array_equal(c[1], b[1]))
    for o in (v, one, two, fresh, bg):
        o.close()


def test_two_gpu_streams_without_a_host_wait(pkg, torch_cuda, sess, synthetic, oracle):
    """One frame on one GPU stream, then the stream's next two frames on another,
    nothing waited for in between: the RGBA scratch has to grow for the second call
    while the first may still use it, and the post state's prevAlpha goes from the
    first call to the second.  Against pack(composite(unpack(in))) on the CPU, the
    alpha from the oracle's post chain over the seam's masks of the unpacked frames."""
    torch = torch_cuda
    std, colour = ref.BT709_LIMITED, (10, 200, 90)
    fh, fw = 100, 150
    y, uv = _video_frames(synthetic, 3, fh, fw, std, 50)
    rgba = ref.unpack(std, y, uv)
    d_rgba = torch.from_numpy(rgba).cuda()
    d_masks = torch.empty((3, sess.mask_h, sess.mask_w), dtype=torch.float32, device="cuda")
    sess.segment_device(d_rgba.data_ptr(), 3, fh, fw, 4, fw * 4, fh * fw * 4, d_masks.data_ptr(), _stream(torch))
    calls = (slice(0, 1), slice(1, 3))
    dev = [(torch.from_numpy(y[c]).cuda(), torch.from_numpy(uv[c]).cuda(),
            torch.zeros(y[c].shape, dtype=torch.uint8, device="cuda"),
            torch.zeros(uv[c].shape, dtype=torch.uint8, device="cuda")) for c in calls]
    gpu_streams = (torch.cuda.Stream(), torch.cuda.Stream())
    bg, chain, v = pkg.Background(sess), pkg.PostChain(sess), pkg.Video(sess, std)
    bg.set_color(*colour)
    torch.cuda.synchronize()
    for (dy, duv, oy, ouv), st in zip(dev, gpu_streams):
        v.process_device(chain, bg, dy.data_ptr(), fw, fw * fh, duv.data_ptr(), fw, fw * fh // 2, dy.shape[0], fh, fw,
                         oy.data_ptr(), fw, fw * fh, ouv.data_ptr(), fw, fw * fh // 2, st.cuda_stream)
    torch.cuda.synchronize()
    masks = d_masks.cpu().numpy()
    state = oracle.PostState(sess.mask_h, sess.mask_w)
    for c, (_, _, oy, ouv) in zip(calls, dev):
        _, alpha = oracle.post(masks[c], rgba[c], state)
        want_y, want_uv = ref.pack(std, bg_ref.composite(oracle, rgba[c], alpha, np.array(colour)))
        _same(f"frames {c.start}..{c.stop - 1} Y", oy.cpu().numpy(), want_y)
        _same(f"frames {c.start}..{c.stop - 1} UV", ouv.cpu().numpy(), want_uv)
    for o in (v, chain, bg):
        o.close()


def test_steady_state_replays_the_graph(pkg, torch_cuda, sess, synthetic):
    """After the first call of a shape, three more calls build and patch nothing."""
    torch = torch_cuda
    n, fh, fw = 2, 60, 88
    y, uv = _video_frames(synthetic, n, fh, fw, ref.BT709_LIMITED, 70)
    dy, duv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    oy, ouv = torch.empty_like(dy), torch.empty_like(duv)
    bg, chain, v = pkg.Background(sess), pkg.PostChain(sess), pkg.Video(sess)

    def call():
        v.process_device(chain, bg, dy.data_ptr(), fw, fw * fh, duv.data_ptr(), fw, fw * fh // 2, n, fh, fw,
                         oy.data_ptr(), fw, fw * fh, ouv.data_ptr(), fw, fw * fh // 2, _stream(torch))

    builds0 = sess.graph_builds
    call()
    torch.cuda.synchronize()
    builds, patches = sess.graph_builds, sess.graph_patches
    assert builds == builds0 + 1  # the seam runs as a graph, built by this shape's first call
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert (sess.graph_builds, sess.graph_patches) == (builds, patches)
    for o in (v, chain, bg):
        o.close()


def test_host_path_equals_device_path(pkg, torch_cuda, sess, synthetic):
    torch = torch_cuda
    y, uv = _video_frames(synthetic, 2, 100, 150, ref.BT601_LIMITED, 80)
    bg = pkg.Background(sess)
    bg.set_blur(2, 1.0)
    v = pkg.Video(sess, "bt601")
    c1, c2 = pkg.PostChain(sess), pkg.PostChain(sess)
    want = _process_device(torch, v, c1, bg, y, uv)
    for call in range(2):  # the second call reuses the host call's planes
        c2.reset()
        got = v.process(y, uv, c2, bg)
        _same(f"host Y call {call}", got[0], want[0])
        _same(f"host UV call {call}", got[1], want[1])
    v.set_standard("bt601-full")
    c2.reset()
    other = v.process(y, uv, c2, bg)
    assert not np.array_equal(other[0], want[0])
    for o in (v, c1, c2, bg):
        o.close()


def test_video_errors(pkg, torch_cuda, sess):
    """Each rejected argument: VSS_E_INVALID_ARG, a message, and the 0xAB outputs untouched."""
    torch = torch_cuda
    L = pkg.lib()
    E = pkg.VSS_E_INVALID_ARG
    n, fh, fw = 1, 48, 64  # the mask's own size
    with pkg.Session(model_h=48, model_w=64, dtype="f32", max_batch=2, autotune=False) as other:
        bg, chain, v = pkg.Background(sess), pkg.PostChain(sess), pkg.Video(sess)
        obg, ochain, ov = pkg.Background(other), pkg.PostChain(other), pkg.Video(other)
        dy = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        duv = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        drgba = torch.zeros(16384, dtype=torch.uint8, device="cuda")
        outs = [torch.full((16384,), FILL, dtype=torch.uint8, device="cuda") for _ in range(3)]
        oy, ouv, orgba = (o.data_ptr() for o in outs)
        Y, UV, RGBA = dy.data_ptr(), duv.data_ptr(), drgba.data_ptr()

        def unpack(std=1, y=Y, yp=fw, yfs=fw * fh, uv=UV, up=fw, ufs=fw * fh // 2, n=n, h=fh, w=fw, out=orgba,
                   rs=4 * fw, fs=4 * fw * fh, s=sess):
            return L.vss_nv12_to_rgba_device(s._h, std, y or None, yp, yfs, uv or None, up, ufs, n, h, w, out or None,
                                             rs, fs, None)

        def pack(std=1, src=RGBA, rs=4 * fw, fs=4 * fw * fh, n=n, h=fh, w=fw, y=oy, yp=fw, yfs=fw * fh, uv=ouv, up=fw,
                 ufs=fw * fh // 2):
            return L.vss_rgba_to_nv12_device(sess._h, std, src or None, rs, fs, n, h, w, y or None, yp, yfs,
                                             uv or None, up, ufs, None)

        def process(v=v, chain=chain, bg=bg, y=Y, yp=fw, yfs=fw * fh, uv=UV, up=fw, ufs=fw * fh // 2, n=n, h=fh, w=fw,
                    o_y=oy, oyp=fw, oyfs=fw * fh, o_uv=ouv, oup=fw, oufs=fw * fh // 2):
            return L.vss_video_process_device(v._v if v else None, chain._st if chain else None,
                                              bg._bg if bg else None, y or None, yp, yfs, uv or None, up, ufs, n, h, w,
                                              o_y or None, oyp, oyfs, o_uv or None, oup, oufs, None)

        bad = [
            dict(w=fw - 1), dict(h=fh - 1), dict(w=0), dict(h=0),   # odd or sub-2 sizes
            dict(yp=fw - 1), dict(up=fw - 2),                     # a pitch below width
            dict(yfs=fw * fh - 1), dict(ufs=fw * fh // 2 - 1),    # a frame stride below pitch * rows
            dict(y=0), dict(uv=0),                                # null pointers
            dict(n=0), dict(n=sess.max_batch + 1),                # n outside the handle's batch capacity
        ]
        for fn in (unpack, process):
            for kw in bad:
                assert fn(**kw) == E, (fn.__name__, kw)
                assert L.vss_last_error(sess._h), (fn.__name__, kw)
        for kw in (dict(std=-1), dict(std=4), dict(out=0), dict(rs=4 * fw - 4), dict(fs=4 * fw * fh - 4)):
            assert unpack(**kw) == E, kw
        for kw in (dict(std=-1), dict(std=4), dict(src=0), dict(y=0), dict(uv=0), dict(w=fw - 1), dict(rs=4 * fw - 2),
                   dict(h=3),
                   dict(yp=fw - 1), dict(up=fw - 1), dict(yfs=fw * fh - 1), dict(ufs=fw * fh // 2 - 1),
                   dict(n=sess.max_batch + 1)):
            assert pack(**kw) == E, kw
        for kw in (dict(o_y=0), dict(o_uv=0), dict(oyp=fw - 1), dict(oup=fw - 1), dict(oyfs=fw * fh - 1),
                   dict(oufs=fw * fh // 2 - 1), dict(v=None), dict(chain=None), dict(bg=None),
                   dict(v=ov), dict(chain=ochain), dict(bg=obg)):   # ... and objects of another handle
            assert process(**kw) == E, kw
        out = ctypes.c_void_p()
        for std in (-1, 4):
            assert L.vss_video_create(sess._h, std, ctypes.byref(out)) == E and not out.value
            assert b"std" in L.vss_last_error(sess._h)
            assert L.vss_video_set_standard(v._v, std) == E
            with pytest.raises(pkg.VssError):
                pkg.Video(sess, std)
        hy, huv = np.zeros((1, 8, 8), np.uint8), np.zeros((1, 4, 8), np.uint8)
        ho = [np.full(64, FILL, np.uint8), np.full(32, FILL, np.uint8)]
        assert L.vss_video_process(v._v, chain._st, bg._bg, hy.ctypes.data, huv.ctypes.data, 1, 8, 7, ho[0].ctypes.data,
                                   ho[1].ctypes.data) == E
        assert L.vss_video_process(v._v, chain._st, obg._bg, hy.ctypes.data, huv.ctypes.data, 1, 8, 8,
                                   ho[0].ctypes.data, ho[1].ctypes.data) == E
        assert L.vss_video_process(v._v, chain._st, bg._bg, None, huv.ctypes.data, 1, 8, 8, ho[0].ctypes.data,
                                   ho[1].ctypes.data) == E
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == FILL).all()), "a rejected call wrote its output"
        assert np.all(ho[0] == FILL) and np.all(ho[1] == FILL)
        # the rejected calls changed nothing: the same objects still work
        assert process() == pkg.VSS_OK and unpack() == pkg.VSS_OK and pack() == pkg.VSS_OK
        torch.cuda.synchronize()
        assert not bool((outs[0][:fw] == FILL).all())
        for o in (v, chain, bg):
            o.close()


def test_scratch_is_counted_and_released(pkg, torch_cuda, sess, synthetic):
    def device_bytes():
        info = pkg._Info()
        assert pkg.lib().vss_get_info(sess._h, ctypes.byref(info)) == pkg.VSS_OK
        return info.device_bytes

    y, uv = _video_frames(synthetic, 2, 100, 150, ref.BT709_LIMITED, 90)
    before = device_bytes()
    bg, chain = pkg.Background(sess), pkg.PostChain(sess)
    v = pkg.Video(sess)
    assert device_bytes() == before  # sized on first use
    v.process(y, uv, chain, bg)
    first = device_bytes()
    px = 2 * 100 * 150
    assert first - before >= 8 * px + 3 * px  # RGBA in and out, the host call's four NV12 planes
    v.process(y, uv, chain, bg)
    assert device_bytes() == first  # the same shape: nothing regrown
    v.process(y[:1], uv[:1], chain, bg)
    assert device_bytes() == first  # a smaller one neither
    v.close()
    assert device_bytes() == before
    chain.close()
    bg.close()
