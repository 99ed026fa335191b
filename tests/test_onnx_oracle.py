"""CPU tests of the ONNX oracle (oracle/onnx_ref.py) — the checker of the GPU
ONNX sessions: its operator implementations pinned against PyTorch's
functional ops, the writer/reader round trip, and the real-weight fixtures
(tests/golden/mediapipe_*.npz) reproducing from their stored graphs (and
from the reference's own model files when /root/reference is present)."""
import os

import numpy as np
import pytest

import onnx_models as M
import onnx_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ASSETS = "/root/reference/client/src/assets"


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("k,s,pads,g,d", [(5, 2, [1, 1, 2, 2], 1, 1), (3, 1, [1, 1, 1, 1], 8, 1),
                                            (3, 2, [0, 0, 2, 2], 8, 1), (1, 1, [0, 0, 0, 0], 1, 1),
                                            (3, 1, [2, 2, 2, 2], 2, 2), (3, 2, [0, 1, 1, 0], 4, 1)])
def test_conv_matches_torch(k, s, pads, g, d):
    torch = _torch()
    F = torch.nn.functional
    rng = np.random.default_rng(k * 100 + s * 10 + g)
    x = rng.standard_normal((2, 8, 13, 17)).astype(np.float32)
    w = rng.standard_normal((16, 8 // g, k, k)).astype(np.float32)
    b = rng.standard_normal(16).astype(np.float32)
    got = R.conv2d(x, w, b, {"strides": [s, s], "pads": pads, "group": g, "dilations": [d, d]})
    xt = F.pad(torch.from_numpy(x).double(), (pads[1], pads[3], pads[0], pads[2]))
    want = F.conv2d(xt, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=s, groups=g,
                    dilation=d).float().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("model", ["conv_tile_matrix", "conv_up_matrix"])
def test_tile_matrix_models_evaluate(model):
    """The k_conv_tile matrix models (tests/test_gpu_conv_tile_matrix.py) load
    and evaluate in the oracle, and every Conv of theirs — 520 channels at
    5x5, the 45-channel Concat input, stride 2 on the odd 37x70 and 21x27
    planes, the upsampled inputs — equals torch.nn.functional.conv2d in
    float64 on the same input, within one float32 rounding of the result
    (both sum in float64, in different orders, and round once)."""
    torch = _torch()
    F = torch.nn.functional
    shapes = {"conv_tile_matrix": M.CONV_TILE_MATRIX_FEEDS, "conv_up_matrix": M.CONV_UP_MATRIX_FEEDS}[model]
    m = R.load(getattr(M, model)())
    feeds = M.matrix_feeds(shapes, 7)
    out = R.run(m, feeds)
    assert len(out) == len(m.outputs)
    for (name, _, dims), v in zip(m.outputs, out.values()):
        assert v.dtype == np.float32 and list(v.shape) == list(dims) and np.isfinite(v).all(), name
        assert np.abs(v).max() > 0, name
    half = R.run(m, feeds, conv_operands="bf16")  # the 16-bit sessions' oracle: rounds, so differs
    assert all(np.isfinite(v).all() for v in half.values())
    assert any(not np.array_equal(half[k], out[k]) for k in out)
    convs = [nd for nd in m.nodes if nd["op"] == "Conv"]
    assert len(convs) == (21 if model == "conv_tile_matrix" else 10)
    vals = R.run(m, feeds, want=[nd["inputs"][0] for nd in convs] + [nd["outputs"][0] for nd in convs])
    seen = set()
    for nd in convs:
        x, w, b = vals[nd["inputs"][0]], m.inits[nd["inputs"][1]], m.inits[nd["inputs"][2]]
        a = nd["attrs"]
        seen.add((x.shape[1], w.shape[2], a["strides"][0]))
        pt, pl, pb, pr = a["pads"]
        xt = F.pad(torch.from_numpy(x).double(), (pl, pr, pt, pb))
        want = F.conv2d(xt, torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                        stride=a["strides"][0]).float().numpy()
        got = vals[nd["outputs"][0]]
        assert got.shape == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all(), nd["outputs"]
    if model == "conv_tile_matrix":
        assert {(520, 5, 1), (45, 3, 1), (72, 3, 2), (200, 5, 1)} <= seen


def test_round_operand_matches_torch():
    """onnx_ref.round_operand (the 16-bit sessions' operand rounding in the
    oracle) is bitwise torch's float32 -> bfloat16 / float16 -> float32:
    random values over the exponent range, exact ties of both parities, values
    that round up into the next binade, subnormals of the 16-bit type and of
    float32, +-0, the largest finite values (float32's rounds to inf in both
    types), +-inf.  NaN is not compared: float16 keeps it a NaN (numpy's
    cast); the bfloat16 integer rounding keeps a NaN whose low 16 bits do not
    carry out of the mantissa (the default quiet NaN among them) and turns one
    that does — mantissa bits all set — into a zero.  No convolution operand
    of the tests is a NaN."""
    torch = _torch()
    rng = np.random.default_rng(3)
    rnd = (rng.standard_normal(4096) * 10.0 ** rng.integers(-42, 38, 4096)).astype(np.float32)
    f32 = lambda bits: np.array(bits, np.uint32).view(np.float32)
    # bf16 keeps the top 16 bits: ties are low halves of exactly 0x8000
    bf_ties = f32([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F818001,
                   0x3FFF8000, 0x3FFFFFFF, 0x407F8000,          # up into the next binade
                   0x00008000, 0x00018000, 0x00000001, 0x007F8000, 0x007FFFFF, 0x80008000,  # float32 subnormals
                   0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF])
    # f16 has 10 mantissa bits: ties at 2^-11 steps of [1, 2); subnormals below 2^-14, spaced 2^-24
    h_ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),
                       1 + 2.0 ** -11 + 2.0 ** -23, 2 - 2.0 ** -11, 2 - 2.0 ** -12, 4 - 2.0 ** -10,
                       2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 5 * 2.0 ** -25, 2.0 ** -14,
                       2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 6.1e-5, 1e-8, -2.0 ** -25,
                       65504.0, 65519.0, 65519.996, 65520.0, -65520.0, 70000.0], np.float32)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, np.finfo(np.float32).tiny], np.float32)
    v = np.concatenate([rnd, bf_ties, h_ties, edge])
    assert np.isfinite(rnd).all() and not np.isnan(v).any()
    for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        got = R.round_operand(v, mode)
        want = torch.from_numpy(v).to(dt).float().numpy()
        assert got.dtype == np.float32
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, (mode, v[bad][:8], got[bad][:8], want[bad][:8])
        # and rounding did something: ties went to even, the largest float32 overflowed
        assert np.isinf(got[np.abs(v) == np.finfo(np.float32).max]).all()
    assert R.round_operand(f32([0x3F808000, 0x3F818000]), "bf16").view(np.uint32).tolist() == [0x3F800000, 0x3F820000]
    assert R.round_operand(np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], np.float32), "f16").tolist() == \
        [1.0, 1 + 2.0 ** -9]
    assert np.isnan(R.round_operand(np.array([np.nan], np.float32), "bf16")).all()  # (the default quiet NaN stays one)
    assert np.isnan(R.round_operand(np.array([np.nan], np.float32), "f16")).all()


def test_pool_resize_norm_match_torch():
    torch = _torch()
    F = torch.nn.functional
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 12, 15)).astype(np.float32)
    xt = torch.from_numpy(x).double()
    got = R._pool(x, {"kernel_shape": [2, 2], "strides": [2, 2]}, "max")
    assert np.array_equal(got, F.max_pool2d(xt, 2, 2).float().numpy())
    got = R._pool(x, {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1], "count_include_pad": 1}, "avg")
    want = F.avg_pool2d(xt, 3, 2, padding=1, count_include_pad=True).float().numpy()
    assert np.abs(got - want).max() < 1e-6
    got = R._pool(x, {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]}, "avg")
    want = F.avg_pool2d(xt, 3, 2, padding=1, count_include_pad=False).float().numpy()
    assert np.abs(got - want).max() < 1e-6
    got = R._resize(x, [1, 1, 2, 2], None, {"mode": "linear", "coordinate_transformation_mode": "half_pixel"})
    want = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False).float().numpy()
    assert np.abs(got - want).max() < 1e-6
    got = R._resize(x, None, [2, 3, 24, 30], {"mode": "linear", "coordinate_transformation_mode": "align_corners"})
    want = F.interpolate(xt, size=(24, 30), mode="bilinear", align_corners=True).float().numpy()
    assert np.abs(got - want).max() < 1e-6
    got = R._resize(x, [1, 1, 2, 2], None, {"mode": "nearest", "coordinate_transformation_mode": "asymmetric",
                                            "nearest_mode": "floor"})
    want = F.interpolate(xt, scale_factor=2, mode="nearest").float().numpy()
    assert np.array_equal(got, want)
    m = R.load(R.make_model([R.make_node("InstanceNormalization", ["x", "s", "b"], ["y"], epsilon=1e-5)],
                            {"s": np.linspace(0.5, 2, 3, dtype=np.float32), "b": np.arange(3, dtype=np.float32)},
                            [("x", [2, 3, 12, 15])], [("y", [2, 3, 12, 15])]))
    got = R.run(m, {"x": x})["y"]
    want = F.instance_norm(xt, weight=torch.linspace(0.5, 2, 3).double(), bias=torch.arange(3).double(),
                           eps=1e-5).float().numpy()
    assert np.abs(got - want).max() < 1e-5


def test_writer_reader_round_trip():
    for name, (fn, _) in M.MODELS.items():
        data = fn()
        m = R.load(data)
        assert m.nodes and m.inputs and m.outputs, name
        if name == "q4f16_like":  # int4 initializers read back as int8 arrays: checked below instead
            continue
        # re-encode what was read: the same bytes come back
        re = R.make_model([R.make_node(n["op"], n["inputs"], n["outputs"], domain=n["domain"], **n["attrs"])
                           for n in m.nodes],
                          m.inits, [(a, d, e) for a, e, d in m.inputs], [(a, d, e) for a, e, d in m.outputs],
                          opset=m.opset)
        assert re == data, name


@pytest.mark.parametrize("name", list(M.MODELS))
def test_synthetic_models_evaluate(name):
    fn, _ = M.MODELS[name]
    m = R.load(fn())
    out = R.run(m, M.feeds_for(name))
    for k, v in out.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), (name, k)
        assert np.abs(v).max() > 0, (name, k)


@pytest.mark.parametrize("key", ["mediapipe_face_detector", "mediapipe_face_landmarks"])
def test_golden_fixture_reproduces(key):
    model, feeds, want, meta = M.load_golden(os.path.join(GOLDEN, key + ".npz"))
    got = R.run(R.load(model), feeds)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    src = os.path.join("/root/reference", meta["source"])
    if os.path.exists(src):  # the build container: the fixture is the reference's own model
        import hashlib
        data = open(src, "rb").read()
        assert hashlib.sha256(data).hexdigest() == meta["sha256"]
        orig = R.run(R.load(data), feeds)
        for k in want:
            assert np.array_equal(orig[k], want[k]), k


def test_q4f16_operators():
    """The q4f16 operators against direct restatements: int4 packing, blocked
    DequantizeLinear, MatMulNBits (nibble order, packed zero points, partial
    last block, bias) and the float16 Cast."""
    rng = np.random.default_rng(11)
    q = rng.integers(-8, 8, (4, 6, 2, 2))
    scale = (rng.random((4, 2, 2, 2)) * 0.1).astype(np.float16)
    m = R.load(R.make_model([R.make_node("DequantizeLinear", ["q", "s"], ["y"], axis=1, block_size=4)],
                            {"q": R.Packed4(q, signed=True), "s": scale}, [], [("y", [4, 6, 2, 2])], opset=21))
    assert np.array_equal(m.inits["q"], q)
    y = R.run(m, {})["y"]
    want = np.empty(q.shape, np.float64)
    for c in range(6):
        want[:, c] = q[:, c] * scale[:, c // 4].astype(np.float64)
    assert y.dtype == np.float16 and np.array_equal(y, want.astype(np.float32).astype(np.float16))
    # MatMulNBits: K = 40 in blocks of 16 (last block partial), N = 3
    K, N, bs = 40, 3, 16
    kb = 3
    B = rng.integers(0, 256, (N, kb, bs // 2), dtype=np.uint8)
    sc = (rng.random(N * kb) * 0.1).astype(np.float32)
    zp = rng.integers(0, 256, (N * 2,), dtype=np.uint8)
    bias = rng.standard_normal(N).astype(np.float32)
    A = rng.standard_normal((2, K)).astype(np.float32)
    m = R.load(R.make_model([R.make_node("MatMulNBits", ["a", "b", "s", "z", "", "bias"], ["y"], domain="com.microsoft",
                                         K=K, N=N, bits=4, block_size=bs)],
                            {"b": B, "s": sc, "z": zp, "bias": bias}, [("a", [2, K])], [("y", [2, N])]))
    y = R.run(m, {"a": A})["y"]
    W = np.zeros((N, K))
    for n in range(N):
        for k in range(K):
            blk, j = divmod(k, bs)
            nib = (B[n, blk, j // 2] >> (4 * (j % 2))) & 15
            z = (zp[n * 2 + blk // 2] >> (4 * (blk % 2))) & 15
            W[n, k] = np.float32((int(nib) - int(z)) * np.float64(sc[n * kb + blk]))
    assert np.allclose(y, A.astype(np.float64) @ W.T + bias, rtol=1e-6, atol=1e-6)
    # Cast to float16 rounds to nearest even half
    v = np.array([1 + 2 ** -11, 1 + 3 * 2 ** -11, 65519.0, 65520.0, 2 ** -25, 3 * 2 ** -25], np.float32)
    m = R.load(R.make_model([R.make_node("Cast", ["v"], ["y"], to=R.DT_FLOAT16)], {}, [("v", [6])], [("y", [6])]))
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).astype(np.float32)
    assert np.array_equal(R.run(m, {"v": v})["y"].astype(np.float32), want)


def test_modnet_instance_norm_conditioning():
    """The seeded MODNet's InstanceNormalization inputs on the GPU tests' frame
    (tests/test_gpu_onnx.py::modnet_cases): every channel's variance is far
    above the export's epsilon (1e-5), so the 16-bit GPU cases run the graph as
    exported without the norm amplifying operand rounding."""
    import onnx_models as M
    m = R.load(M.modnet(q4f16=True, in_eps=1e-5))
    x = np.random.default_rng(21).random((1, 3, 288, 512), dtype=np.float32)
    nodes = [nd for nd in m.nodes if nd["op"] == "InstanceNormalization"]
    assert len(nodes) == 16
    assert all(abs(nd["attrs"].get("epsilon", 1e-5) - 1e-5) < 1e-12 for nd in nodes)
    got = R.run(m, {"input": x}, want=[nd["inputs"][0] for nd in nodes])
    worst = min(float(v.astype(np.float64).var(axis=(2, 3)).min()) for v in got.values())
    print(f"smallest InstanceNorm input variance {worst:.4g} (eps 1e-5)")
    assert worst >= 100 * 1e-5
