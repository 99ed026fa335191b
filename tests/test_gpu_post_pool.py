"""GPU parity of the post chain over many streams (include/vss_pool.h,
k_post_pool in csrc/vss_post.hip): one frame of each of several streams per
call, against the CPU oracle's `post` with one oracle.PostState per stream fed
that stream's frames one at a time.  Never against the pool itself.

Bar, as tests/test_gpu_post.py: u8 alpha bytes BIT-EXACT; f32 refinedAlpha
max |gpu - oracle| <= 1e-6 (the only inexact operation is pow(), whose last-ulp
double result may differ between the device math library and glibc before the
f32 store; measured differences are printed).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA_TOL = 1e-6
FH, FW = 100, 150  # frames: no multiple of any mask size used here


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Streams:
    """`count` synthetic streams of `length` frames each and the seam's masks of
    every frame, computed once per (model size, channels) and left unchanged."""

    def __init__(self, syn, session, count, length, c=3, fh=FH, fw=FW, seed0=300):
        self.H, self.W = session.mask_h, session.mask_w
        self.frames = np.stack([np.stack([syn.make_frame(seed0 + k * length + j, fh, fw, c) for j in range(length)])
                                for k in range(count)])  # [count][length][fh][fw][c]
        flat = self.frames.reshape(-1, fh, fw, c)
        mb = session.max_batch
        masks = [session.segment_frames(flat[i:i + mb])[0] for i in range(0, len(flat), mb)]
        self.masks = np.concatenate(masks).reshape(count, length, self.H, self.W)
        self.frames.setflags(write=False)
        self.masks.setflags(write=False)


@pytest.fixture(scope="module")
def sessions(pkg):
    """One f32, autotune-off session per model size, shared by the module's tests."""
    made = {}

    def get(H, W, max_batch=4):
        key = (H, W, max_batch)
        if key not in made:
            made[key] = pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=max_batch, autotune=False)
        return made[key]

    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def stream_data(sessions, synthetic):
    made = {}

    def get(H, W, c=3, count=3, length=4):
        key = (H, W, c, count, length)
        if key not in made:
            made[key] = Streams(synthetic, sessions(H, W), count, length, c)
        return made[key]

    return get


def _ocfg(oracle, config):
    ocfg = oracle.PostConfig.default()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(config, f))
    return ocfg


def _enqueue(torch, pool, ids, frames, masks, faces=None, pad=0):
    """One pooled call on torch's current stream, not waited for: returns the device
    tensors (outputs first), which the caller keeps alive until it synchronises."""
    n, fh, fw, c = frames.shape
    _, H, W = masks.shape
    rs = fw * c + pad
    padded = np.zeros((n, fh, rs), np.uint8)
    padded[:, :, :fw * c] = frames.reshape(n, fh, fw * c)
    df = torch.from_numpy(padded).cuda()
    dm = torch.from_numpy(np.ascontiguousarray(masks, np.float32)).cuda()
    da = torch.full((n, H, W), -1.0, dtype=torch.float32, device="cuda")
    du = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")
    dfaces = None
    if faces is not None:
        raw = bytes((type(faces[0]) * n)(*faces))
        dfaces = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    pool.process_device(ids, df.data_ptr(), n, fh, fw, c, rs, fh * rs, dm.data_ptr(), da.data_ptr(), du.data_ptr(),
                        torch.cuda.current_stream().cuda_stream, dfaces.data_ptr() if dfaces is not None else 0)
    return da, du, df, dm, dfaces


def _call(torch, pool, ids, frames, masks, faces=None, pad=0):
    da, du, *_ = _enqueue(torch, pool, ids, frames, masks, faces, pad)
    torch.cuda.synchronize()
    return da.cpu().numpy(), du.cpu().numpy()


def _want(oracle, states, ids, frames, masks, cfg=None, faces=None):
    """The oracle's outputs of one call: frame t through stream ids[t]'s own state."""
    outs = [oracle.post(masks[t:t + 1], frames[t:t + 1], states[i], cfg,
                        [faces[t]] if faces is not None else None) for t, i in enumerate(ids)]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def _cmp(tag, a, u, want_a, want_u):
    err = float(np.abs(a - want_a).max())
    mism = int((u != want_u).sum())
    print(f"{tag}: alpha max|d|={err:.3g} u8 mismatches={mism}")
    assert err <= ALPHA_TOL
    assert mism == 0


# capacity 5, live streams 4, 0 and 2; every call in another order, stream 0 skips
# the second call, the third call has n = 1
LIVE = (4, 0, 2)
SCHEDULE = ([4, 0, 2], [2, 4], [0], [0, 2, 4])


def _take(data, live, ids, used):
    """The next frame and mask of every stream of a call; `used` counts per stream."""
    k = [live.index(i) for i in ids]
    j = [used[i] for i in ids]
    for i in ids:
        used[i] += 1
    return data.frames[k, j], data.masks[k, j]


@pytest.mark.parametrize("H,W,c,pad", [(48, 80, 3, 0), (16, 48, 3, 0), (48, 80, 4, 40)])
def test_interleaved_streams_vs_oracle(pkg, torch_cuda, sessions, stream_data, oracle, H, W, c, pad):
    s, data = sessions(H, W), stream_data(H, W, c)
    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    with pkg.PostPool(s, 5) as pool:
        for call, ids in enumerate(SCHEDULE):
            frames, masks = _take(data, LIVE, ids, used)
            a, u = _call(torch_cuda, pool, ids, frames, masks, pad=pad)
            want_a, want_u = _want(oracle, states, ids, frames, masks)
            _cmp(f"{H}x{W} c={c} call {call} ids {ids}", a, u, want_a, want_u)


def test_pool_equals_per_stream_chains(pkg, torch_cuda, sessions, stream_data):
    """The same streams through three PostChain objects, n = 1 calls."""
    torch = torch_cuda
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    used = dict.fromkeys(LIVE, 0)
    chains = {i: pkg.PostChain(s) for i in LIVE}
    with pkg.PostPool(s, 5) as pool:
        for call, ids in enumerate(SCHEDULE):
            frames, masks = _take(data, LIVE, ids, used)
            a, u = _call(torch, pool, ids, frames, masks)
            for t, i in enumerate(ids):
                df = torch.from_numpy(np.ascontiguousarray(frames[t])).cuda()
                dm = torch.from_numpy(np.ascontiguousarray(masks[t])).cuda()
                da = torch.empty((H, W), dtype=torch.float32, device="cuda")
                du = torch.empty((H, W), dtype=torch.uint8, device="cuda")
                chains[i].process_device(df.data_ptr(), 1, FH, FW, 3, FW * 3, FH * FW * 3, dm.data_ptr(),
                                         da.data_ptr(), du.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                _cmp(f"call {call} stream {i} vs its chain", a[t], u[t], da.cpu().numpy(), du.cpu().numpy())
    for ch in chains.values():
        ch.close()


def test_faces_mixed_in_one_call(pkg, torch_cuda, sessions, stream_data, oracle):
    """One stream with an affine (3 degrees, about 9.5 mask pixels of translation:
    its warped taps land in other tiles) and a box, one with a box only, one with
    neither, in one call; three calls."""
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    th = np.deg2rad(3.0)
    affine = (np.cos(th), -np.sin(th), 9.5, np.sin(th), np.cos(th), -2.25)
    box_a, box_b = (40.0, 15.0, 105.0, 80.0), (20.5, 30.0, 70.0, 90.25)

    def faces_of(ids, make):
        per = {4: make(affine=affine, box=box_a, video_wh=(FW, FH)), 0: make(box=box_b, video_wh=(FW, FH)), 2: make()}
        return [per[i] for i in ids]

    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    with pkg.PostPool(s, 5) as pool:
        for call, ids in enumerate(([4, 0, 2], [2, 4, 0], [0, 2, 4])):
            frames, masks = _take(data, LIVE, ids, used)
            a, u = _call(torch_cuda, pool, ids, frames, masks, faces=faces_of(ids, pkg.FaceFrame.make))
            want_a, want_u = _want(oracle, states, ids, frames, masks, faces=faces_of(ids, oracle.Face.make))
            _cmp(f"faces call {call} ids {ids}", a, u, want_a, want_u)


def test_reset_without_a_wait(pkg, torch_cuda, sessions, stream_data, oracle):
    """Call A, reset(id), call B, and only then a synchronise: A is unaffected, B's
    frame of `id` is a first frame, the others continue; reset() restarts all."""
    torch = torch_cuda
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    ids = list(LIVE)
    with pkg.PostPool(s, 5) as pool:
        f0, m0 = _take(data, LIVE, ids, used)
        _call(torch, pool, ids, f0, m0)  # every stream has a prevAlpha
        _want(oracle, states, ids, f0, m0)
        fa, ma = _take(data, LIVE, ids, used)
        fb, mb = _take(data, LIVE, ids, used)
        keep_a = _enqueue(torch, pool, ids, fa, ma)
        pool.reset(0)
        keep_b = _enqueue(torch, pool, ids, fb, mb)
        torch.cuda.synchronize()
        want = _want(oracle, states, ids, fa, ma)
        _cmp("A (before the reset)", keep_a[0].cpu().numpy(), keep_a[1].cpu().numpy(), *want)
        states[0] = oracle.PostState(H, W)
        want = _want(oracle, states, ids, fb, mb)
        _cmp("B (stream 0 restarted)", keep_b[0].cpu().numpy(), keep_b[1].cpu().numpy(), *want)
        pool.reset()
        fc, mc = _take(data, LIVE, ids, used)
        a, u = _call(torch, pool, ids, fc, mc)
        fresh = {i: oracle.PostState(H, W) for i in LIVE}
        _cmp("after reset()", a, u, *_want(oracle, fresh, ids, fc, mc))


def test_two_gpu_streams_without_a_host_wait(pkg, torch_cuda, sessions, stream_data, oracle):
    """The same stream ids on one GPU stream, then on another, nothing waited for in
    between: the second call reads the prevAlpha planes the first one writes, so the
    pool itself has to order the two streams."""
    torch = torch_cuda
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    ids = list(LIVE)
    host = [_take(data, LIVE, ids, used) for _ in range(2)]
    dev = [(torch.from_numpy(np.ascontiguousarray(f)).cuda(),
            torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda(),
            torch.full((3, H, W), -1.0, dtype=torch.float32, device="cuda"),
            torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")) for f, m in host]
    gpu_streams = (torch.cuda.Stream(), torch.cuda.Stream())
    with pkg.PostPool(s, 5) as pool:
        torch.cuda.synchronize()
        for (df, dm, da, du), st in zip(dev, gpu_streams):
            pool.process_device(ids, df.data_ptr(), 3, FH, FW, 3, FW * 3, FH * FW * 3, dm.data_ptr(), da.data_ptr(),
                                du.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        for k, ((f, m), (_, _, da, du)) in enumerate(zip(host, dev)):
            _cmp(f"call {k} on its own GPU stream", da.cpu().numpy(), du.cpu().numpy(),
                 *_want(oracle, states, ids, f, m))


def test_many_streams(pkg, torch_cuda, sessions, synthetic, oracle):
    """Capacity 64 at max_batch 8: two rounds of 8 calls, each round over all 64 ids
    in a shuffled order (plane index and parity bookkeeping beyond n)."""
    H, W, cap = 16, 16, 64
    s = sessions(H, W, 8)
    data = Streams(synthetic, s, cap, 2, fh=40, fw=56, seed0=900)
    states = [oracle.PostState(H, W) for _ in range(cap)]
    rng = np.random.default_rng(11)
    worst, mism = 0.0, 0
    with pkg.PostPool(s, cap) as pool:
        for rnd in range(2):
            order = rng.permutation(cap)
            for call in range(8):
                ids = [int(i) for i in order[call * 8:call * 8 + 8]]
                frames, masks = data.frames[ids, rnd], data.masks[ids, rnd]
                a, u = _call(torch_cuda, pool, ids, frames, masks)
                want_a, want_u = _want(oracle, states, ids, frames, masks)
                worst = max(worst, float(np.abs(a - want_a).max()))
                mism += int((u != want_u).sum())
    print(f"64 streams: alpha max|d|={worst:.3g} u8 mismatches={mism}")
    assert worst <= ALPHA_TOL
    assert mism == 0


@pytest.mark.parametrize("knobs", [dict(USE_BILATERAL=0), dict(EMA=0.9, NOISE_CUTOFF=0.2, HIGH_THRESHOLD=0.7)])
def test_config_variants_set_between_calls(pkg, torch_cuda, sessions, stream_data, oracle, knobs):
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    with pkg.PostPool(s, 5) as pool:
        for call, ids in enumerate(([4, 0, 2], [0, 4, 2], [2, 0, 4])):
            if call == 1:
                pool.set_config(**knobs)
            frames, masks = _take(data, LIVE, ids, used)
            a, u = _call(torch_cuda, pool, ids, frames, masks)
            want_a, want_u = _want(oracle, states, ids, frames, masks, _ocfg(oracle, pool.config))
            _cmp(f"{knobs} call {call}", a, u, want_a, want_u)


def test_errors_leave_the_pool_intact(pkg, torch_cuda, sessions, stream_data, oracle):
    torch = torch_cuda
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    L = pkg.lib()
    states = {i: oracle.PostState(H, W) for i in LIVE}
    used = dict.fromkeys(LIVE, 0)
    ids = list(LIVE)

    def refused(rc, handle):
        assert rc == pkg.VSS_E_INVALID_ARG
        assert L.vss_last_error(handle), "no message"

    out = ctypes.c_void_p()
    refused(L.vss_post_pool_create(s._h, None, 0, ctypes.byref(out)), s._h)  # capacity < 1
    with pkg.PostPool(s, 5) as pool, \
            pkg.Session(model_h=H, model_w=W, dtype="f32", max_batch=4, autotune=False) as other:
        f0, m0 = _take(data, LIVE, ids, used)
        _cmp("before the refusals", *_call(torch, pool, ids, f0, m0), *_want(oracle, states, ids, f0, m0))
        f1, m1 = _take(data, LIVE, ids, used)
        df = torch.from_numpy(np.ascontiguousarray(f1)).cuda()
        dm = torch.from_numpy(np.ascontiguousarray(m1)).cuda()
        da = torch.empty((3, H, W), dtype=torch.float32, device="cuda")

        def dev(pool_p, id_list, n, frames_p, masks_p):
            arr = (ctypes.c_int * len(id_list))(*id_list) if id_list is not None else None
            return L.vss_post_pool_process_device(pool_p, arr, n, frames_p, FH, FW, 3, FW * 3, FH * FW * 3, masks_p,
                                                  None, da.data_ptr(), None, None)

        fp, mp = df.data_ptr(), dm.data_ptr()
        refused(dev(None, ids, 3, fp, mp), None)          # null pool
        refused(dev(pool._p, None, 3, fp, mp), s._h)      # null ids
        refused(dev(pool._p, ids, 3, fp, None), s._h)     # null masks
        refused(dev(pool._p, ids, 3, None, mp), s._h)     # null frames with use_bilateral on
        refused(dev(pool._p, ids, 0, fp, mp), s._h)       # n < 1
        refused(dev(pool._p, [0, 1, 2, 3, 4], 5, fp, mp), s._h)  # n above the session's max_batch
        refused(dev(pool._p, [4, -1, 2], 3, fp, mp), s._h)       # id below the range
        refused(dev(pool._p, [4, 0, 5], 3, fp, mp), s._h)        # id == capacity
        refused(dev(pool._p, [4, 0, 4], 3, fp, mp), s._h)        # the same id twice
        refused(L.vss_post_pool_reset(pool._p, 5), s._h)
        host_f = np.ascontiguousarray(f1)
        host_a = np.empty((3, H * W), np.float32)
        arr = (ctypes.c_int * 3)(*ids)
        refused(L.vss_segment_post_pool(other._h, pool._p, arr, host_f.ctypes.data, 3, FH, FW, 3, FW * 3,
                                        host_a.ctypes.data, None), other._h)  # a pool of another handle
        refused(L.vss_segment_post_pool(s._h, pool._p, arr, host_f.ctypes.data, 3, FH, FW, 3, FW * 3, None, None),
                s._h)                                                          # both outputs null
        with pytest.raises(pkg.VssError):
            pool.set_config(BILATERAL_SIGMA_RANGE=0.0)
        # no refusal enqueued anything or moved a stream's state
        _cmp("after the refusals", *_call(torch, pool, ids, f1, m1), *_want(oracle, states, ids, f1, m1))


def test_memory_is_counted_and_released(pkg, torch_cuda, sessions):
    H, W, cap = 48, 80, 37
    s = sessions(H, W)

    def device_bytes():
        info = pkg._Info()
        assert pkg.lib().vss_get_info(s._h, ctypes.byref(info)) == pkg.VSS_OK
        return info.device_bytes

    before = device_bytes()
    pool = pkg.PostPool(s, cap)
    grown = device_bytes() - before
    planes, table = cap * 2 * H * W * 4, (3 * 255 * 255 + 1) * 8
    print(f"pool of {cap}: {grown} bytes = {planes} (planes) + {grown - planes}")
    assert planes <= grown <= planes + table + 4096  # two planes per stream and O(1): the table
    pool.close()
    assert device_bytes() == before


def test_host_call_equals_device_path(pkg, torch_cuda, sessions, stream_data):
    H, W = 48, 80
    s, data = sessions(H, W), stream_data(H, W)
    used_h, used_d = dict.fromkeys(LIVE, 0), dict.fromkeys(LIVE, 0)
    with pkg.PostPool(s, 5) as host_pool, pkg.PostPool(s, 5) as dev_pool:
        for ids in ([0, 4, 2], [2, 0]):
            frames, masks = _take(data, LIVE, ids, used_h)
            _take(data, LIVE, ids, used_d)
            a, u, mw, mh = host_pool.segment(ids, frames)
            assert (mw, mh) == (W, H)
            da, du = _call(torch_cuda, dev_pool, ids, frames, masks)
            assert np.array_equal(a.reshape(da.shape), da)
            assert np.array_equal(u.reshape(du.shape), du)
