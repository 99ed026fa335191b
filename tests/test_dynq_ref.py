"""The reference for dynamically quantised graphs (tests/onnx_ref_dynq.py),
on the CPU: ConvInteger / MatMulInteger against an independent statement
(torch.nn.functional.conv2d on x - zx and w - zw in float64), the four-term
identity the GPU kernels compute by,

    sum (x - zx)(w - zw[m]) = acc[m][pix] - zx' Sw[m] - zw'[m] Sx[pix] + K zx' zw'[m]

(x' = x - 128 padded by zx', w' = w - 128, K padding as zero weights, in
wrapping 32-bit arithmetic), DynamicQuantizeLinear against a float64 statement
away from ties, and the conditions the case table (tests/op_cases_dynq.py) and
the two models (tests/onnx_models_dynq.py) are built on."""
import zlib

import numpy as np
import pytest
import torch

import onnx_models_dynq as MD
import onnx_ref as R
import onnx_ref_dynq as RD
import op_cases_dynq as DC

U8, S8 = np.uint8, np.int8

# (name, x shape, w shape, x type, weight type, attrs): padded, strided, dilated, grouped, K no multiple of 64
GEOMETRIES = [
    ("3x3_pad1", (2, 3, 9, 11), (5, 3, 3, 3), U8, U8, {"pads": [1, 1, 1, 1]}),
    ("3x3_s2_pad1", (2, 16, 17, 33), (8, 16, 3, 3), U8, U8, {"pads": [1, 1, 1, 1], "strides": [2, 2]}),
    ("3x3_d2_pad2", (2, 16, 12, 13), (8, 16, 3, 3), U8, S8, {"pads": [2, 2, 2, 2], "dilations": [2, 2]}),
    ("5x5_K200_asym", (2, 8, 9, 11), (5, 8, 5, 5), S8, U8, {"pads": [2, 0, 1, 3]}),
    ("1x1_K64", (2, 64, 5, 7), (70, 64, 1, 1), U8, U8, {}),
    ("same_upper_s2", (2, 3, 12, 13), (5, 3, 3, 3), S8, S8, {"auto_pad": "SAME_UPPER", "strides": [2, 2]}),
    ("g2_3x3", (2, 8, 9, 11), (6, 4, 3, 3), U8, U8, {"pads": [1, 1, 1, 1], "group": 2}),
]


def _operands(name, xs, ws, xt, wt, per_channel):
    r = np.random.default_rng(zlib.crc32(name.encode()))
    info_x, info_w = np.iinfo(xt), np.iinfo(wt)
    x = r.integers(info_x.min, info_x.max + 1, size=xs).astype(xt)
    w = r.integers(info_w.min, info_w.max + 1, size=ws).astype(wt)
    zx = xt(r.integers(info_x.min, info_x.max + 1))
    zw = r.integers(info_w.min, info_w.max + 1, size=ws[0] if per_channel else ()).astype(wt)
    return x, w, zx, zw


def _torch_pads(attrs, x, w):
    st, dl = attrs.get("strides", [1, 1]), attrs.get("dilations", [1, 1])
    return RD._pads(attrs, w.shape[2:], x.shape[2:], st, dl), st, dl


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_conv_integer_is_torch_conv2d(geo, per_channel):
    name, xs, ws, xt, wt, attrs = geo
    x, w, zx, zw = _operands(name, xs, ws, xt, wt, per_channel)
    got = RD.conv_integer(x, w, zx, zw, attrs)
    (pt, pl, pb, pr), st, dl = _torch_pads(attrs, x, w)
    xd = torch.from_numpy(x.astype(np.float64) - float(zx))
    wd = torch.from_numpy(w.astype(np.float64) - zw.astype(np.float64).reshape(-1, 1, 1, 1))
    want = torch.nn.functional.conv2d(torch.nn.functional.pad(xd, (pl, pr, pt, pb)), wd, stride=st, dilation=dl,
                                      groups=attrs.get("group", 1)).numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got.astype(np.float64), want)  # (every sum below 2^53: float64 is exact)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("geo", [g for g in GEOMETRIES if g[5].get("group", 1) == 1], ids=lambda g: g[0])
def test_four_term_identity(geo, per_channel):
    """What k_iconv_tile computes: signed bytes x' and w', the window gathered with zx' outside the image, K padded
    to a multiple of 64 with zero weights (and zero activations), the four terms in wrapping uint32."""
    name, xs, ws, xt, wt, attrs = geo
    x, w, zx, zw = _operands(name, xs, ws, xt, wt, per_channel)
    want = RD.conv_integer(x, w, zx, zw, attrs)
    offx, offw = (128 if xt is U8 else 0), (128 if wt is U8 else 0)
    xp, zxp = x.astype(np.int64) - offx, int(zx) - offx
    wp = w.astype(np.int64) - offw
    zwp = np.broadcast_to(zw.astype(np.int64) - offw, (ws[0],))
    (pt, pl, pb, pr), st, dl = _torch_pads(attrs, x, w)
    xpad = np.pad(xp, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=zxp)
    n, c, _, _ = xs
    m, _, kh, kw = ws
    ho, wo = want.shape[2:]
    K = c * kh * kw
    Kp = -(-K // 64) * 64
    cols = np.zeros((n, ho, wo, Kp), np.int64)  # the staged activations: (c, ky, kx) order, 0 past K
    for ci in range(c):
        for ky in range(kh):
            for kx in range(kw):
                cols[..., (ci * kh + ky) * kw + kx] = xpad[:, ci, ky * dl[0]:ky * dl[0] + (ho - 1) * st[0] + 1:st[0],
                                                           kx * dl[1]:kx * dl[1] + (wo - 1) * st[1] + 1:st[1]]
    wrow = np.zeros((m, Kp), np.int64)
    wrow[:, :K] = wp.reshape(m, K)
    assert np.abs(cols).max() <= 128 and np.abs(wrow).max() <= 128
    u = lambda a: np.asarray(a, np.int64).astype(np.uint32)
    acc = u(np.einsum("nhwk,mk->nmhw", cols, wrow))
    sw, sx = u(wrow.sum(axis=1)).reshape(1, m, 1, 1), u(cols.sum(axis=3))[:, None]
    zwu = u(zwp).reshape(1, m, 1, 1)
    with np.errstate(over="ignore"):
        v = acc - u(zxp) * sw - zwu * sx + u(K) * u(zxp) * zwu
    assert np.array_equal(v.astype(np.uint32).view(np.int32).reshape(want.shape), want)


@pytest.mark.parametrize("per_column", [False, True])
def test_matmul_integer_is_float64_matmul(per_column):
    r = np.random.default_rng(5)
    a = r.integers(0, 256, size=(2, 33, 200)).astype(U8)
    b = r.integers(0, 256, size=(200, 100)).astype(U8)
    za, zb = U8(113), r.integers(0, 256, size=100 if per_column else ()).astype(U8)
    got = RD.matmul_integer(a, b, za, zb)
    want = (a.astype(np.float64) - 113.0) @ (b.astype(np.float64) - zb.astype(np.float64))
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.float64), want)


def test_dynamic_quantize_linear_statement():
    """The float32 statement against the operator text in float64: the same scale and zero point to float32
    precision, y equal except within 1e-4 of a tie; and the cases the text leaves to the implementation."""
    x = (np.random.default_rng(3).standard_normal((2, 5, 70, 100)) * 3.7).astype(np.float32)
    y, sc, zp = RD.dynamic_quantize_linear(x)
    assert y.dtype == U8 and sc.dtype == np.float32 and sc.shape == () and zp.dtype == U8 and zp.shape == ()
    mn, mx = min(0.0, float(x.min())), max(0.0, float(x.max()))
    s64 = (mx - mn) / 255.0
    assert abs(float(sc) - s64) <= 2.0 ** -23 * s64 and int(zp) == int(np.clip(np.rint(-mn / s64), 0, 255))
    v = x.astype(np.float64) / s64 + float(zp)
    far = np.abs(np.abs(v - np.floor(v)) - 0.5) > 1e-4
    assert far.mean() > 0.99 and np.array_equal(y[far], np.clip(np.rint(v), 0, 255)[far].astype(U8))
    y0, s0, z0 = RD.dynamic_quantize_linear(np.zeros((3, 4), np.float32))
    assert not y0.any() and float(s0) == 1.0 and int(z0) == 0
    yp, sp, zpp = RD.dynamic_quantize_linear(np.asarray([2.0, 8.0], np.float32))  # all positive: the range starts at 0
    assert int(zpp) == 0 and float(sp) == np.float32(8.0) / np.float32(255.0) and yp.tolist() == [64, 255]
    yn, _, zn = RD.dynamic_quantize_linear(np.asarray([-2.0, -8.0], np.float32))
    assert int(zn) == 255 and yn.tolist() == [191, 0]
    # ties round to even: 0.5 and 1.5 steps of a planted range of 255 / 32
    t = np.asarray([0.0, 255.0 / 32, 0.5 / 32, 1.5 / 32, 2.5 / 32], np.float32)
    assert RD.dynamic_quantize_linear(t)[0].tolist() == [0, 255, 0, 2, 2]


# ---- the case table's own conditions ---------------------------------------------------------------
@pytest.fixture(scope="module")
def families():
    out = {}
    for fam, cases in DC.groups().items():
        data, feeds, built = DC.build(cases)
        out[fam] = (cases, built, RD.run_all(R.load(data), feeds))
    return out


def test_table_accumulators_below_2_24(families):
    """Every integer result of the table converts to float32 exactly (with room for a dyadic bias of 40 quanta)."""
    for cases, built, env in families.values():
        for cs in cases:
            for a in built[cs.name].acc:
                assert np.abs(env[a].astype(np.int64)).max() < DC.ACC_MAX - 64, cs.name


def test_table_zero_points_and_scales(families):
    """The planted ranges give the zero points 0, 255 and mid-range the cases are named for, and the dyadic ones
    x_scale = 2^-4 exactly."""
    zps = set()
    for cases, built, env in families.values():
        for cs in cases:
            for z, v in built[cs.name].expect_zp.items():
                assert int(env[z]) == v and env[z].dtype == U8, cs.name
                zps.add(v)
            for s, v in built[cs.name].expect_scale.items():
                assert float(env[s]) == v, cs.name
    assert zps == {0, 100, 255}


def test_table_dql_patterns(families):
    cases, built, env = families[DC.F_DQL]
    for cs in cases:
        (y, sc, zp) = built[cs.name].outs
        if cs.name.endswith("_zero"):
            assert float(env[sc]) == 1.0 and int(env[zp]) == 0 and not env[y].any()
        elif cs.name.endswith("_pos"):
            assert int(env[zp]) == 0 and env[y].max() == 255
        elif cs.name.endswith("_neg"):
            assert int(env[zp]) == 255 and env[y].min() == 0
        elif cs.name.endswith("_ties"):
            (x,) = built[cs.name].feeds.values()
            steps = x.astype(np.float64) / float(env[sc])
            assert float(env[sc]) == 2.0 ** -5 and (np.abs(steps - np.floor(steps) - 0.5) == 0).mean() > 0.1
        elif env[y].size == 1:  # (one element: the range is [0, x] or [x, 0])
            assert int(env[zp]) in (0, 255)
        else:
            assert 0 < int(env[zp]) < 255 and env[y].min() == 0 and env[y].max() == 255


def test_table_general_chains_hold_their_bound(families):
    """The reference itself (one float32 rounding per node) lies within the general chains' bound, and the clipped
    cases keep a share of their values strictly between the bounds."""
    n = 0
    for cases, built, env in families.values():
        for cs in cases:
            for o, rule in built[cs.name].outs.items():
                if isinstance(rule, str):
                    continue
                v, bound = DC.general_bound(rule, env)
                assert (np.abs(env[o].astype(np.float64) - v) <= bound).all(), cs.name
                if rule["hi"] is not None:
                    assert ((v > rule["lo"]) & (v < rule["hi"])).mean() > 0.2, cs.name
                n += 1
    assert n >= 10


def test_refused_cases_the_reference_sees():
    """The refusals that are about one node's operands are the reference's too; the others are rules on the graph
    (what may read an int32 tensor, a zero point, a quantised tensor), which the reference simply evaluates."""
    graph_rules = {"refuse_int32_graph_output", "refuse_int32_read_by_Relu", "refuse_zero_point_read_by_Cast",
                   "refuse_y_read_by_Relu"}
    assert graph_rules <= {cs.name for cs in DC.REFUSED_CASES}
    for cs in DC.REFUSED_CASES:
        data, feeds, _ = DC.build([cs])
        if cs.name in graph_rules:
            RD.run_all(R.load(data), feeds)
        else:
            with pytest.raises(ValueError, match=cs.op):
                RD.run_all(R.load(data), feeds)


# ---- the two models ---------------------------------------------------------------------------------
def test_segmenter_is_built_exact():
    """Every clipped layer reaches both ends, so every DynamicQuantizeLinear behind the image's gives x_scale = 2^-4
    and zero point 0; every value before the Sigmoid is a multiple of 2^-12 below 2^12: exact in float32."""
    data, names, clipped, launches, fused = MD.dynq_segmenter()
    m = R.load(data)
    env = RD.run_all(m, MD.segmenter_feeds())
    for c in clipped:
        assert env[c].min() == 0.0 and env[c].max() == np.float32(MD.ACT_MAX), c
    scales = [(float(env[nd["outputs"][1]]), int(env[nd["outputs"][2]])) for nd in m.nodes if nd["op"] == "DynamicQuantizeLinear"]
    assert scales[0] == (2.0 ** -8, 0) and set(scales[1:]) == {(2.0 ** -4, 0)} and len(scales) == fused == 8
    for k in ("head", "feat", "stem", "up"):
        v = env[names[k]].astype(np.float64) * 2.0 ** 12
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() < 2.0 ** 24, k
    for nd in m.nodes:
        if nd["op"] == "ConvInteger":
            assert np.abs(env[nd["outputs"][0]].astype(np.int64)).max() < 2 ** 24


def _f32_layer_norm(x, g, b, eps):
    x = x.astype(np.float32)
    mu = x.mean(axis=-1, keepdims=True, dtype=np.float32)
    d = x - mu
    var = (d * d).mean(axis=-1, keepdims=True, dtype=np.float32)
    return (d / np.sqrt(var + np.float32(eps)) * g + b).astype(np.float32)


def test_transformer_leaves_the_bar_room():
    """No element entering a DynamicQuantizeLinear lies within TIE_MARGIN steps of a rounding tie, and evaluating
    the LayerNormalization in float32 instead of float64 moves the output by less than a tenth of the 1e-4 bar:
    the reference's own float32-vs-float64 spread."""
    data, out, dq_inputs = MD.dynq_transformer()
    m = R.load(data)
    feeds = MD.transformer_feeds()
    env = RD.run_all(m, feeds)
    for name in dq_inputs:
        _, sc, zp = RD.dynamic_quantize_linear(env[name])
        steps = env[name].astype(np.float64) / float(sc)
        margin = np.abs(np.abs(steps - np.floor(steps)) - 0.5).min()
        print(f"{name}: nearest tie {margin:.2e} steps")
        assert margin > MD.TIE_MARGIN, name
    ln = next(nd for nd in m.nodes if nd["op"] == "LayerNormalization")
    g, b = (env[i] for i in ln["inputs"][1:3])
    env32 = RD.run_all(m, feeds, override={ln["outputs"][0]: lambda v: _f32_layer_norm(feeds["x"], g, b, ln["attrs"]["epsilon"])})
    assert not np.array_equal(env32[ln["outputs"][0]], env[ln["outputs"][0]])  # (the float32 evaluation does differ)
    spread = np.abs(env32[out].astype(np.float64) - env[out].astype(np.float64)) / np.maximum(1.0, np.abs(env[out]))
    print(f"float32-vs-float64 spread {float(spread.max()):.2e}")
    assert spread.max() < 1e-5
