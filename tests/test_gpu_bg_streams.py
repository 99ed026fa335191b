"""GPU parity of vss_background_composite_streams_device (include/vss_streams.h;
k_bg_streams_*, k_blur_h_streams, k_matte_*_streams): one frame per stream, each
over its own background.  Every comparison is BIT-EXACT, frame by frame, against
the numpy restatements of the single-object call (tests/streams_ref.py); the
pooled path is never its own reference.  Masks 48 x 80, frames 100 x 150: even,
no multiple of a mask side, a width that is no multiple of 4, 2 x 3 (at radius
32: the whole frame inside every halo) blur tiles and 25 flat-form rows of workgroups."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streams_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 48, 80
FH, FW = 100, 150
MAX_BATCH = 8
PAD_IN = 8    # bytes after each input row
PAD_OUT = 12  # bytes after each output row: with the base offset 4, rows 3, 7, ... start on 16 bytes, the others do not
OUT_OFF = 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def sess(pkg, torch_cuda):
    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=MAX_BATCH, autotune=False) as s:
        yield s


@pytest.fixture(scope="module")
def inputs():
    """8 noise frames with 4 channels (the 3-channel runs drop the last) and 8 alpha planes; built once."""
    return (np.random.default_rng(900).integers(0, 256, (MAX_BATCH, FH, FW, 4), dtype=np.uint8),
            sr.alpha_bytes(901, MAX_BATCH, H, W))


def _device_bytes(pkg, s):
    info = pkg._Info()
    assert pkg.lib().vss_get_info(s._h, ctypes.byref(info)) == pkg.VSS_OK
    return info.device_bytes


def _upload(torch, frames, alpha):
    n, fh, fw, c = frames.shape
    rs = fw * c + PAD_IN
    padded = np.zeros((n, fh, rs), np.uint8)
    padded[:, :, :fw * c] = frames.reshape(n, fh, fw * c)
    return torch.from_numpy(padded).cuda(), torch.from_numpy(np.ascontiguousarray(alpha)).cuda(), rs


class _Call:
    """One call's device buffers, uploaded and 0xAB-filled by stage(); issue() enqueues the call
    and waits for nothing, so that several staged calls can go out back to back."""

    def __init__(self, torch, frames, alpha):
        self.n, self.fh, self.fw, self.c = frames.shape
        self.df, self.da, self.rs = _upload(torch, frames, alpha)
        self.ors = self.fw * 4 + PAD_OUT
        self.do = torch.full((OUT_OFF + self.n * self.fh * self.ors,), 0xAB, dtype=torch.uint8, device="cuda")

    def issue(self, pkg, s, bgs, st, single=False):
        """The pooled call on the GPU stream handle st (single: n calls of
        vss_background_composite_device with n = 1 instead)."""
        n, fh, fw, c, rs, ors = self.n, self.fh, self.fw, self.c, self.rs, self.ors
        if single:
            for t in range(n):
                pkg.background_composite_device(s, bgs[t], self.df.data_ptr() + t * fh * rs, 1, fh, fw, c, rs, fh * rs,
                                                self.da.data_ptr() + t * H * W,
                                                self.do.data_ptr() + OUT_OFF + t * fh * ors, ors, fh * ors, st)
        else:
            pkg.composite_streams_device(s, bgs, self.df.data_ptr(), n, fh, fw, c, rs, fh * rs, self.da.data_ptr(),
                                         self.do.data_ptr() + OUT_OFF, ors, fh * ors, st)

    def fetch(self):
        """After a synchronise: [n,fh,fw,4], everything around it still 0xAB."""
        got = self.do.cpu().numpy()
        assert np.all(got[:OUT_OFF] == 0xAB), "bytes before the output were written"
        got = got[OUT_OFF:].reshape(self.n, self.fh, self.ors)
        assert np.all(got[:, :, self.fw * 4:] == 0xAB), "row padding was written"
        return got[:, :, :self.fw * 4].reshape(self.n, self.fh, self.fw, 4)


def _run(torch, pkg, s, bgs, frames, alpha, single=False):
    call = _Call(torch, frames, alpha)
    torch.cuda.synchronize()
    call.issue(pkg, s, bgs, torch.cuda.current_stream().cuda_stream, single)
    torch.cuda.synchronize()
    return call.fetch()


class _Objects:
    """Background objects made from specs, closed at the end of the test."""

    def __init__(self, pkg, s):
        self.pkg, self.s, self.made = pkg, s, []

    def __call__(self, sp):
        bg = sr.apply(self.pkg, self.pkg.Background(self.s), sp)
        self.made.append(bg)
        return bg

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for bg in self.made:
            bg.close()


def _check_frames(tag, pkg, oracle, specs, frames, alpha, got):
    for t, sp in enumerate(specs):
        sr.same(f"{tag}: frame {t} ({sp['mode']})", got[t], sr.want(pkg, oracle, sp, frames[t], alpha[t]))


@pytest.mark.parametrize("channels", [3, 4])
def test_every_mode_in_one_call(pkg, torch_cuda, sess, oracle, inputs, channels):
    """Colour, blur r=3, image, blur r=32, colour under layers, image under layers with
    refinement: the blur frames are neither first nor adjacent, so a descriptor indexed
    by a list position instead of the frame shows."""
    L = sr.layers(pkg)
    specs = [sr.spec("colour", color=(200, 10, 99)), sr.spec("blur", blur=(3, 1.5)), sr.spec("image", image=sr.IMAGE),
             sr.spec("blur", blur=(32, 12.0)), sr.spec("colour", color=(1, 2, 3), layers=L),
             sr.spec("image", image=sr.IMAGE2, layers=L, refine=(2, 16.0))]
    frames, alpha = inputs[0][:6, :, :, :channels], inputs[1][:6]
    with _Objects(pkg, sess) as make:
        got = _run(torch_cuda, pkg, sess, [make(sp) for sp in specs], frames, alpha)
    _check_frames(f"{channels} channels", pkg, oracle, specs, frames, alpha, got)
    plain = sr.want(pkg, oracle, sr.spec("colour", color=(1, 2, 3)), frames[4], alpha[4])
    assert not np.array_equal(got[4], plain)  # the layers show


def test_one_object_for_several_frames(pkg, torch_cuda, sess, oracle, inputs):
    """One blur object for frames 0 and 2, one refined image object for frames 1 and 3,
    with different frame contents: a scratch slot shared by the frames of an object shows."""
    blur, img = sr.spec("blur", blur=(5, 2.0)), sr.spec("image", image=sr.IMAGE, refine=(3, 16.0))
    specs = [blur, img, blur, img]
    frames, alpha = inputs[0][:4], inputs[1][:4]
    with _Objects(pkg, sess) as make:
        a, b = make(blur), make(img)
        bgs = [a, b, a, b]
        got = _run(torch_cuda, pkg, sess, bgs, frames, alpha)
        single = _run(torch_cuda, pkg, sess, bgs, frames, alpha, single=True)
    _check_frames("shared objects", pkg, oracle, specs, frames, alpha, got)
    sr.same("pooled vs n = 1 calls", got, single)
    assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[1], got[3])


def test_radii_in_one_call(pkg, torch_cuda, sess, oracle, inputs):
    """Refinement radius 1 and 8 and an unrefined frame, blur radius 1 and 32: the LDS is
    sized by the call's largest radius and every frame uses its own."""
    specs = [sr.spec("colour", color=(9, 200, 30), refine=(1, 1.0)), sr.spec("blur", blur=(1, 0.8)),
             sr.spec("image", image=sr.IMAGE, refine=(8, 400.0)), sr.spec("colour", color=(90, 20, 30)),
             sr.spec("blur", blur=(32, 40.0), refine=(8, 16.0))]
    frames, alpha = inputs[0][3:8, :, :, :3], inputs[1][3:8]
    with _Objects(pkg, sess) as make:
        got = _run(torch_cuda, pkg, sess, [make(sp) for sp in specs], frames, alpha)
    _check_frames("radii", pkg, oracle, specs, frames, alpha, got)


def test_degenerate_lists(pkg, torch_cuda, sess, oracle, inputs):
    """No blur frame, only blur frames, n = 1 in each form, and n = max_batch = 8 with 8 distinct objects."""
    frames, alpha = inputs
    flat = [sr.spec("colour", color=(5, 6, 7)), sr.spec("image", image=sr.IMAGE2)]
    blurs = [sr.spec("blur", blur=(2, 1.0)), sr.spec("blur", blur=(7, 3.0), refine=(2, 16.0))]
    eight = [sr.spec("colour", color=(10 * i, 255 - 10 * i, i)) for i in range(3)] + \
            [sr.spec("blur", blur=(1 + 4 * i, 1.0 + i)) for i in range(3)] + \
            [sr.spec("image", image=sr.IMAGE), sr.spec("colour", refine=(4, 16.0))]
    cases = {"no blur": flat, "only blur": blurs, "n = 1 flat": flat[1:], "n = 1 blur": blurs[1:], "n = 8": eight}
    with _Objects(pkg, sess) as make:
        for tag, specs in cases.items():
            n = len(specs)
            got = _run(torch_cuda, pkg, sess, [make(sp) for sp in specs], frames[:n], alpha[:n])
            _check_frames(tag, pkg, oracle, specs, frames[:n], alpha[:n], got)


def test_settings_between_calls(pkg, torch_cuda, sess, oracle, inputs):
    """set_color, set_mode, set_privacy and set_refine(0) on one object between calls: the
    next call follows them and the other frames do not change; then another frame size,
    where the caches are rebuilt, and back."""
    L = sr.layers(pkg)
    moving = sr.spec("image", image=sr.IMAGE, layers=L, refine=(2, 16.0))
    specs = [sr.spec("blur", blur=(4, 2.0), layers=L), moving, sr.spec("image", image=sr.IMAGE2)]
    frames, alpha = inputs[0][:3], inputs[1][:3]
    small = np.ascontiguousarray(frames[:, :62, :98])  # 62 x 98: even, above the mask, width no multiple of 4
    with _Objects(pkg, sess) as make:
        bgs = [make(sp) for sp in specs]
        first = _run(torch_cuda, pkg, sess, bgs, frames, alpha)
        _check_frames("before", pkg, oracle, specs, frames, alpha, first)
        steps = [("set_color", lambda b: b.set_color(7, 8, 9), {"mode": "colour", "color": (7, 8, 9)}),
                 ("set_mode", lambda b: b.set_mode(pkg.VSS_BG_IMAGE), {"mode": "image"}),
                 ("set_privacy", lambda b: b.set_privacy(1), {"level": 1}),
                 ("set_refine(0)", lambda b: b.set_refine(0), {"refine": None})]
        for tag, setter, change in steps:
            setter(bgs[1])
            moving = dict(moving, **change)
            specs[1] = moving
            got = _run(torch_cuda, pkg, sess, bgs, frames, alpha)
            sr.same(f"{tag}: frame 1", got[1], sr.want(pkg, oracle, moving, frames[1], alpha[1]))
            sr.same(f"{tag}: frame 0", got[0], first[0])
            sr.same(f"{tag}: frame 2", got[2], first[2])
        bgs[1].set_refine(2, 16.0)
        specs[1] = dict(moving, refine=(2, 16.0))
        _check_frames("another frame size", pkg, oracle, specs, small, alpha,
                      _run(torch_cuda, pkg, sess, bgs, small, alpha))
        _check_frames("and back", pkg, oracle, specs, frames, alpha, _run(torch_cuda, pkg, sess, bgs, frames, alpha))


def test_two_gpu_streams_share_an_object(pkg, torch_cuda, sess, oracle, inputs):
    """Two calls on two GPU streams name the same blur object (slot 0 of its horizontal
    pass in both).  Both calls' buffers are uploaded first and the device is idle; then
    the calls go out back to back with no host wait between them, so the second is
    ordered after the first by the object's event alone.  Run once."""
    torch = torch_cuda
    blur = sr.spec("blur", blur=(9, 4.0))
    one, two = [blur, sr.spec("colour", color=(1, 200, 3))], [sr.spec("colour", color=(250, 0, 30)), blur]
    frames, alpha = inputs
    with _Objects(pkg, sess) as make:
        shared = make(blur)
        bgs1, bgs2 = [shared, make(one[1])], [make(two[0]), shared]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        call1, call2 = _Call(torch, frames[0:2], alpha[0:2]), _Call(torch, frames[2:4], alpha[2:4])
        torch.cuda.synchronize()
        call1.issue(pkg, sess, bgs1, s1.cuda_stream)
        call2.issue(pkg, sess, bgs2, s2.cuda_stream)
        torch.cuda.synchronize()
        got1, got2 = call1.fetch(), call2.fetch()
    _check_frames("first stream", pkg, oracle, one, frames[0:2], alpha[0:2], got1)
    _check_frames("second stream", pkg, oracle, two, frames[2:4], alpha[2:4], got2)


@pytest.mark.parametrize("second", [0, 1])
def test_followed_event_rerecorded_and_outlived(pkg, torch_cuda, sess, oracle, inputs, second):
    """A call over two blur objects records one event, the first object's by address, and
    the other follows it.  Then, on three more GPU streams and with no host wait
    anywhere: a call over object `second` alone, a call over the other alone, and a call
    over both again; then `second` is destroyed and the survivor used.  Which object
    leads is decided by address, so both orders run.  Where `second` is the leader, its
    event is recorded again while the follower still points at it, the follower then
    waits on it from another stream, and at the end the follower outlives the object
    whose event it follows.  Every frame against the references.  Run once per case."""
    torch = torch_cuda
    specs = [sr.spec("blur", blur=(9, 4.0)), sr.spec("blur", blur=(4, 2.0), refine=(2, 16.0))]
    frames, alpha = inputs
    first = 1 - second
    with _Objects(pkg, sess) as make:
        objs = [make(sp) for sp in specs]
        plan = [([0, 1], slice(0, 2)), ([second], slice(2, 3)), ([first], slice(3, 4)), ([1, 0], slice(4, 6))]
        streams = [torch.cuda.Stream() for _ in plan]
        calls = [_Call(torch, frames[sl], alpha[sl]) for _, sl in plan]
        torch.cuda.synchronize()
        for call, (who, _), st in zip(calls, plan, streams):
            call.issue(pkg, sess, [objs[k] for k in who], st.cuda_stream)
        torch.cuda.synchronize()
        for i, (call, (who, sl)) in enumerate(zip(calls, plan)):
            _check_frames(f"call {i}", pkg, oracle, [specs[k] for k in who], frames[sl], alpha[sl], call.fetch())
        # both objects' latest call is the last one, which one event covers: destroy one, use the other
        last, last_stream = _Call(torch, frames[6:8], alpha[6:8]), torch.cuda.Stream()
        torch.cuda.synchronize()
        objs[second].close()
        last.issue(pkg, sess, [objs[first], objs[first]], last_stream.cuda_stream)
        torch.cuda.synchronize()
        _check_frames("after the other object was destroyed", pkg, oracle, [specs[first]] * 2, frames[6:8], alpha[6:8],
                      last.fetch())


def test_refusals_leave_everything_intact(pkg, torch_cuda, sess, oracle, inputs):
    """Every refusal of include/vss_streams.h returns VSS_E_INVALID_ARG with a message;
    the good call after them equals the references; the objects' scratch is counted into
    device_bytes and released with them."""
    torch = torch_cuda
    frames, alpha = inputs[0][:3], inputs[1][:3]
    start = _device_bytes(pkg, sess)
    blur, refined = sr.spec("blur", blur=(6, 2.5)), sr.spec("colour", color=(40, 50, 60), refine=(2, 16.0))
    specs = [blur, refined, blur]
    df, da, rs = _upload(torch, frames, alpha)
    ors = FW * 4
    do = torch.zeros((3 * FH * ors,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(bgs, n=3, fp=df.data_ptr(), ap=da.data_ptr(), op=do.data_ptr(), fh=FH, fw=FW, c=4, row=rs, s=sess):
        pkg.composite_streams_device(s, bgs, fp, n, fh, fw, c, row, fh * row, ap, op, fw * 4, fh * fw * 4, 0)

    with pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=2, autotune=False) as other, \
            _Objects(pkg, sess) as make, _Objects(pkg, other) as make_other:
        a, b = make(blur), make(refined)
        good = [a, b, a]
        no_image, no_blur, foreign = pkg.Background(sess), pkg.Background(sess), make_other(refined)
        make.made += [no_image, no_blur]
        no_image.set_mode(pkg.VSS_BG_IMAGE)
        no_blur.set_mode(pkg.VSS_BG_BLUR)
        refusals = {
            "null frames": lambda: call(good, fp=0),
            "null alpha": lambda: call(good, ap=0),
            "null output": lambda: call(good, op=0),
            "null background": lambda: call([a, None, a]),
            "another handle's background": lambda: call([a, b, foreign]),
            "n = 0": lambda: call([], n=0),
            "n above max_batch": lambda: call([a] * (MAX_BATCH + 1), n=MAX_BATCH + 1),
            "5 channels": lambda: call(good, c=5),
            "row stride below the row": lambda: call(good, row=FW * 4 - 1),
            "zero height": lambda: call(good, fh=0),
            "image mode without an image, last frame": lambda: call([a, b, no_image]),
            "blur mode without a blur": lambda: call([no_blur, b, a]),
            "refinement with a frame below the mask": lambda: call(good, fh=H - 2),
        }
        for tag, refused in refusals.items():
            with pytest.raises(pkg.VssError) as e:
                refused()
            assert e.value.code == pkg.VSS_E_INVALID_ARG, tag
            assert len(str(e.value)) > len(f"vss error {pkg.VSS_E_INVALID_ARG}: "), f"{tag}: no message"
        torch.cuda.synchronize()
        assert not do.any().item(), "a refused call wrote output"
        before = _device_bytes(pkg, sess)
        got = _run(torch, pkg, sess, good, frames, alpha)
        _check_frames("after the refusals", pkg, oracle, specs, frames, alpha, got)
        # the blur object serves 2 frames (its horizontal pass), the refined one 1 (17 B per mask pixel)
        assert _device_bytes(pkg, sess) - before == 2 * FH * FW * 4 + 1 * H * W * 17
    assert _device_bytes(pkg, sess) == start
