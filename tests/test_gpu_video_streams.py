"""GPU parity of the NV12 calls over many streams (include/vss_streams.h):
vss_video_process_streams_device / vss_video_process_streams and
vss_segment_background_streams.  Expected output, on the CPU:
  pack(std, composite_ref(unpack(std, in), alpha bytes of oracle.post over that stream's PostState))
with the seam's masks of the unpacked frames, one PostState per stream and the
numpy restatements of the single-object composite (tests/streams_ref.py).
Every comparison is BIT-EXACT.  Masks 48 x 80 (16 x 48 for the host paths),
frames 100 x 150."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streams_ref as sr  # noqa: E402
import video_ref as vref  # noqa: E402

pytestmark = pytest.mark.gpu

FH, FW = 100, 150
LIVE = (4, 0, 2)      # the live streams of a pool of capacity 5
CAPACITY = 5
PER_STREAM = 3        # frames per stream
FILL = 0xAB
SPECS = {4: sr.spec("colour", color=(10, 200, 90)), 0: sr.spec("blur", blur=(3, 1.5)),
         2: sr.spec("image", image=sr.IMAGE, refine=(2, 16.0))}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def sessions(pkg, torch_cuda):
    made = {}

    def get(H, W):
        if (H, W) not in made:
            made[(H, W)] = pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False)
        return made[(H, W)]

    yield get
    for s in made.values():
        s.close()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


_data = {}


def _stream_data(torch, synthetic, s, std):
    """Per live stream: PER_STREAM scenes with a person as NV12, their unpacked RGBA and the
    seam's masks of it (the GPU's, as in test_gpu_video.py and test_gpu_post_pool.py); built once."""
    key = (s.mask_h, s.mask_w, std)
    if key not in _data:
        out = {}
        for k, i in enumerate(LIVE):
            rgb = np.stack([synthetic.make_frame(500 + 20 * k + j, FH, FW, 3) for j in range(PER_STREAM)])
            y, uv = vref.pack(std, rgb)
            rgba = vref.unpack(std, y, uv)
            d_rgba = torch.from_numpy(rgba).cuda()
            d_masks = torch.empty((PER_STREAM, s.mask_h, s.mask_w), dtype=torch.float32, device="cuda")
            s.segment_device(d_rgba.data_ptr(), PER_STREAM, FH, FW, 4, FW * 4, FH * FW * 4, d_masks.data_ptr(),
                             _stream(torch))
            torch.cuda.synchronize()
            out[i] = (y, uv, rgba, d_masks.cpu().numpy())
        _data[key] = out
    return _data[key]


def _take(data, ids, used):
    """The next frame of every stream in ids -> (y, uv, rgba, masks) of the call; `used` advances."""
    pick = [(i, used[i]) for i in ids]
    for i in ids:
        used[i] += 1
    return tuple(np.stack([data[i][part][j] for i, j in pick]) for part in range(4))


def _want(pkg, oracle, std, states, ids, rgba, masks, faces=None):
    """Each stream's alpha from its own PostState, its frame over its own background, packed."""
    out = []
    for t, i in enumerate(ids):
        _, alpha = oracle.post(masks[t:t + 1], rgba[t:t + 1], states[i], None, [faces[t]] if faces is not None else None)
        out.append(sr.want(pkg, oracle, SPECS[i], rgba[t], alpha[0]))
    return vref.pack(std, np.stack(out))


class _Planes:
    """A call's NV12 planes on the device with padded pitches, gaps between the frames and
    base pointers off every vector alignment; the outputs 0xAB-filled."""

    def __init__(self, torch, y, uv):
        self.torch = torch
        self.n = n = y.shape[0]
        self.yp, self.up, self.off = FW + 13, FW + 6, 1
        self.yfs, self.ufs = self.yp * FH + 3, self.up * (FH // 2) + 5
        self.dy = torch.from_numpy(self._place(y, self.yp, self.yfs, FH)).cuda()
        self.duv = torch.from_numpy(self._place(uv, self.up, self.ufs, FH // 2)).cuda()
        self.oy = torch.full((self.off + n * self.yfs,), FILL, dtype=torch.uint8, device="cuda")
        self.ouv = torch.full((self.off + n * self.ufs,), FILL, dtype=torch.uint8, device="cuda")

    def _place(self, a, pitch, fs, rows):
        buf = np.full(self.off + self.n * fs, FILL, np.uint8)
        for t in range(self.n):
            buf[self.off + t * fs: self.off + t * fs + rows * pitch].reshape(rows, pitch)[:, :FW] = a[t]
        return buf

    def args(self, width=FW):
        o = self.off
        return (self.dy.data_ptr() + o, self.yp, self.yfs, self.duv.data_ptr() + o, self.up, self.ufs, self.n, FH, width,
                self.oy.data_ptr() + o, self.yp, self.yfs, self.ouv.data_ptr() + o, self.up, self.ufs)

    def fetch(self):
        """-> (y, uv) of the outputs; everything outside them still 0xAB."""
        gy, guv = self.oy.cpu().numpy(), self.ouv.cpu().numpy()
        y = np.stack([gy[self.off + t * self.yfs:][:FH * self.yp].reshape(FH, self.yp)[:, :FW] for t in range(self.n)])
        uv = np.stack([guv[self.off + t * self.ufs:][:(FH // 2) * self.up].reshape(FH // 2, self.up)[:, :FW]
                       for t in range(self.n)])
        sr.same("output Y padding", gy, self._place(y, self.yp, self.yfs, FH))
        sr.same("output UV padding", guv, self._place(uv, self.up, self.ufs, FH // 2))
        return y, uv

    def untouched(self):
        return bool((self.oy == FILL).all().item() and (self.ouv == FILL).all().item())


def _device_call(torch, v, pool, ids, bgs, y, uv, faces=None):
    planes = _Planes(torch, y, uv)
    dfaces = None
    if faces is not None:
        dfaces = torch.frombuffer(bytearray(bytes((type(faces[0]) * len(faces))(*faces))), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    v.process_streams_device(pool, ids, bgs, *planes.args(), _stream(torch),
                             dfaces.data_ptr() if dfaces is not None else 0)
    torch.cuda.synchronize()
    return planes.fetch()


def _backgrounds(pkg, s):
    return {i: sr.apply(pkg, pkg.Background(s), sp) for i, sp in SPECS.items()}


@pytest.mark.parametrize("std", [vref.BT709_LIMITED, vref.BT601_FULL], ids=["bt709", "bt601-full"])
def test_interleaved_streams(pkg, torch_cuda, sessions, synthetic, oracle, std):
    """Streams 4, 0 and 2 of a pool of 5 over the schedule [4,0,2], [2,4], [0], [0,2,4], one
    background per stream (colour, blur, image with refinement)."""
    s = sessions(48, 80)
    data = _stream_data(torch_cuda, synthetic, s, std)
    states = {i: oracle.PostState(s.mask_h, s.mask_w) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    bgs = _backgrounds(pkg, s)
    v = pkg.Video(s, std)
    try:
        with pkg.PostPool(s, CAPACITY) as pool:
            for call, ids in enumerate(([4, 0, 2], [2, 4], [0], [0, 2, 4])):
                y, uv, rgba, masks = _take(data, ids, used)
                got_y, got_uv = _device_call(torch_cuda, v, pool, ids, [bgs[i] for i in ids], y, uv)
                want_y, want_uv = _want(pkg, oracle, std, states, ids, rgba, masks)
                sr.same(f"call {call} ids {ids} Y", got_y, want_y)
                sr.same(f"call {call} ids {ids} UV", got_uv, want_uv)
                assert not np.array_equal(got_y, y)  # backgrounds were put in
    finally:
        for o in [v] + list(bgs.values()):
            o.close()


def test_a_refused_call_moves_no_stream(pkg, torch_cuda, sessions, synthetic, oracle):
    """After a good call: a background in image mode without an image (at the last
    index, behind two good ones), an id twice, and an odd width are refused and write
    nothing; the next good call equals the oracle with the states advanced by the good
    calls only — the backgrounds are checked before the pool flips a stream's plane."""
    torch, std = torch_cuda, vref.BT709_LIMITED
    s = sessions(48, 80)
    data = _stream_data(torch, synthetic, s, std)
    states = {i: oracle.PostState(s.mask_h, s.mask_w) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    bgs = _backgrounds(pkg, s)
    bad = pkg.Background(s)
    bad.set_mode(pkg.VSS_BG_IMAGE)
    v = pkg.Video(s, std)
    ids = [4, 0, 2]
    try:
        with pkg.PostPool(s, CAPACITY) as pool:
            def good(tag):
                y, uv, rgba, masks = _take(data, ids, used)
                got = _device_call(torch, v, pool, ids, [bgs[i] for i in ids], y, uv)
                want = _want(pkg, oracle, std, states, ids, rgba, masks)
                sr.same(f"{tag} Y", got[0], want[0])
                sr.same(f"{tag} UV", got[1], want[1])

            good("first call")
            y, uv = data[4][0][:3], data[4][1][:3]  # any three frames: nothing of them may be used
            planes = _Planes(torch, y, uv)
            torch.cuda.synchronize()
            ok = [bgs[i] for i in ids]
            refusals = {"image mode without an image": (ids, ok[:2] + [bad], FW),
                        "an id twice": ([4, 0, 4], ok, FW),
                        "odd width": (ids, ok, FW - 1)}
            for tag, (rids, rbgs, width) in refusals.items():
                with pytest.raises(pkg.VssError) as e:
                    v.process_streams_device(pool, rids, rbgs, *planes.args(width), _stream(torch))
                assert e.value.code == pkg.VSS_E_INVALID_ARG, tag
            torch.cuda.synchronize()
            assert planes.untouched(), "a refused call wrote output"
            good("after the refusals")
    finally:
        for o in [v, bad] + list(bgs.values()):
            o.close()


def test_host_paths_equal_the_device_paths(pkg, torch_cuda, sessions, synthetic):
    """vss_video_process_streams == the device call, and vss_segment_background_streams ==
    the seam, the pool and the pooled composite enqueued by hand; two calls each, so that
    the streams' state is carried.  Masks 16 x 48."""
    torch, std = torch_cuda, vref.BT601_LIMITED
    s = sessions(16, 48)
    data = _stream_data(torch, synthetic, s, std)
    bgs = _backgrounds(pkg, s)
    v = pkg.Video(s, std)
    P = s.mask_h * s.mask_w
    try:
        with pkg.PostPool(s, CAPACITY) as dev_pool, pkg.PostPool(s, CAPACITY) as host_pool, \
                pkg.PostPool(s, CAPACITY) as rgba_dev, pkg.PostPool(s, CAPACITY) as rgba_host:
            used = dict.fromkeys(LIVE, 0)
            for call, ids in enumerate(([0, 2, 4], [4, 2])):
                y, uv, rgba, _ = _take(data, ids, used)
                n, bl = len(ids), [bgs[i] for i in ids]
                want = _device_call(torch, v, dev_pool, ids, bl, y, uv)
                got = v.process_streams(y, uv, host_pool, ids, bl)
                sr.same(f"call {call} host Y", got[0], want[0])
                sr.same(f"call {call} host UV", got[1], want[1])
                # RGB frames through the host convenience against the three device calls
                rgb = np.ascontiguousarray(rgba[..., :3])
                out = rgba_host.replace_backgrounds(ids, rgb, bl)
                d_rgb = torch.from_numpy(rgb).cuda()
                d_masks = torch.empty((n, P), dtype=torch.float32, device="cuda")
                d_alpha = torch.empty((n, P), dtype=torch.uint8, device="cuda")
                d_out = torch.empty((n, FH, FW, 4), dtype=torch.uint8, device="cuda")
                st = _stream(torch)
                s.segment_device(d_rgb.data_ptr(), n, FH, FW, 3, FW * 3, FH * FW * 3, d_masks.data_ptr(), st)
                rgba_dev.process_device(ids, d_rgb.data_ptr(), n, FH, FW, 3, FW * 3, FH * FW * 3, d_masks.data_ptr(), 0,
                                        d_alpha.data_ptr(), st)
                pkg.composite_streams_device(s, bl, d_rgb.data_ptr(), n, FH, FW, 3, FW * 3, FH * FW * 3,
                                             d_alpha.data_ptr(), d_out.data_ptr(), stream=st)
                torch.cuda.synchronize()
                sr.same(f"call {call} replace_backgrounds", out, d_out.cpu().numpy())
                assert not np.array_equal(out[..., :3], rgb)
    finally:
        for o in [v] + list(bgs.values()):
            o.close()


def test_faces_are_forwarded(pkg, torch_cuda, sessions, synthetic, oracle):
    """d_faces with an affine and a box on stream 4, a box on stream 0 and neither on
    stream 2, two calls: against the oracle's post chain given the same faces."""
    torch, std = torch_cuda, vref.BT709_LIMITED
    s = sessions(48, 80)
    data = _stream_data(torch, synthetic, s, std)
    states = {i: oracle.PostState(s.mask_h, s.mask_w) for i in LIVE}
    plain = {i: oracle.PostState(s.mask_h, s.mask_w) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    bgs = _backgrounds(pkg, s)
    v = pkg.Video(s, std)

    def faces_of(ids, make):
        th = np.deg2rad(3.0)
        affine = (np.cos(th), -np.sin(th), 9.5, np.sin(th), np.cos(th), -2.25)
        per = {4: make(affine=affine, box=(40.0, 15.0, 105.0, 80.0), video_wh=(FW, FH)),
               0: make(box=(20.5, 30.0, 70.0, 90.25), video_wh=(FW, FH)), 2: make()}
        return [per[i] for i in ids]

    try:
        with pkg.PostPool(s, CAPACITY) as pool:
            differs = False
            for call, ids in enumerate(([4, 0, 2], [2, 4, 0])):
                y, uv, rgba, masks = _take(data, ids, used)
                got = _device_call(torch, v, pool, ids, [bgs[i] for i in ids], y, uv,
                                   faces=faces_of(ids, pkg.FaceFrame.make))
                want = _want(pkg, oracle, std, states, ids, rgba, masks, faces=faces_of(ids, oracle.Face.make))
                sr.same(f"faces call {call} Y", got[0], want[0])
                sr.same(f"faces call {call} UV", got[1], want[1])
                without = _want(pkg, oracle, std, plain, ids, rgba, masks)
                differs |= not np.array_equal(without[0], want[0])
            assert differs, "the face box changed nothing: the case does not test the forwarding"
    finally:
        for o in [v] + list(bgs.values()):
            o.close()
