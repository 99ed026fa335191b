"""Two small dynamically quantised models (test infrastructure), in the form
onnxruntime's quantize_dynamic writes: every quantised layer is

    xq, x_scale, x_zp = DynamicQuantizeLinear(x)
    y = Mul(Cast(ConvInteger | MatMulInteger(xq, Wq, x_zp, w_zp)), Mul(x_scale, w_scale)) [+ bias] [Clip]

with uint8 weights.

dynq_segmenter — a MobileNet-style person segmenter:

    image [2, 3, 32, 48] -> stem 3x3 s2 (3 -> 16)
      -> 2 x inverted residual (1x1 16 -> 32, 3x3 depthwise, 1x1 32 -> 16, float residual Add, Clip)
      -> Resize (linear, 2x) -> head 3x3 (16 -> 1) -> Sigmoid

Built to be exact: every activation is Clip(0, 255 * 2^-4) and reaches both
ends (tests/test_dynq_ref.py asserts it), so every DynamicQuantizeLinear sees
min 0 and max 255 * 2^-4 and gives x_scale = 2^-4, zero point 0; the weights
are small integers, the weight scales powers of two, the biases multiples of
the products' quantum; the image is pixels j / 256 with 0 and 255 present
(x_scale 2^-8).  Every value before the Sigmoid is then a small multiple of a
power of two, exact in float32 and float64 alike — through the Resize too —
and a session's tensors there must equal the reference's.

dynq_transformer — one transformer block on [2, 40, 32]:

    x -> LayerNormalization -> DynamicQuantizeLinear -> 3 x MatMulInteger Linear (Q, K, V share the one)
      -> the float attention core (2 heads of 16) -> DynamicQuantizeLinear -> MatMulInteger projection -> + x

with general (seeded) scales.  Its input is chosen so that no element entering
a DynamicQuantizeLinear lies within TIE_MARGIN steps of a rounding tie (again
asserted on the CPU): the float32 roundings of the LayerNormalization and the
attention core in front cannot move a quantised value.
"""
from __future__ import annotations

import numpy as np

import onnx_models as M
import onnx_ref as R

MINMAX, DYNQ, TILE, DIRECT = "k_dyn_minmax(", "k_dyn_quantize(", "k_iconv_tile(", "k_iconv_direct("
SHAPE = (2, 3, 32, 48)
ACT_MAX = 255 * 2.0 ** -4
F32, U8 = np.float32, np.uint8


class _B(M.Builder):
    def qlayer(self, x, kind, wq, zw, w_scale, bias=None, clip=None, xq=None, **attrs):
        """One quantised layer on float `x` (xq: an earlier DynamicQuantizeLinear of it): (output, xq)."""
        xq = xq or self.op("DynamicQuantizeLinear", [x], n_out=3)
        y, sc, zp = xq
        acc = self.op(kind, [y, self.const(wq), zp, self.const(zw)], **attrs)
        f = self.op("Cast", [acc], to=R.DT_FLOAT)
        s = self.op("Mul", [sc, self.const(np.asarray(w_scale, F32))])
        t = self.op("Mul", [f, s])
        if bias is not None:
            t = self.op("Add", [t, self.const(bias)])
        if clip is not None:
            t = self.op("Clip", [t, self.const(F32(clip[0])), self.const(F32(clip[1]))])
        return t, xq

    def qconv(self, x, cin, cout, k, j, stride=1, group=1, wmax=3, clip=True, xs=2.0 ** -4):
        """A quantised convolution with w_scale = 2^-j, uint8 weights 128 + [-wmax, wmax], a bias that is a multiple
        of x_scale * w_scale, and Clip(0, ACT_MAX)."""
        wq = (128 + self.rng.integers(-wmax, wmax + 1, size=(cout, cin // group, k, k))).astype(U8)
        bias = (self.rng.integers(-32, 97, size=cout) * (xs * 2.0 ** -j) * 4).astype(F32).reshape(1, cout, 1, 1)
        y, _ = self.qlayer(x, "ConvInteger", wq, U8(128), 2.0 ** -j, bias, (0.0, ACT_MAX) if clip else None,
                           kernel_shape=[k, k], strides=[stride, stride], pads=[k // 2] * 4, group=group)
        return y


def dynq_segmenter(shape=SHAPE, width=16, float_model=False):
    """(model bytes, {"matte", "head", "feat", "stem", "up": graph outputs' names}, the clipped values' names, a
    session's launches in order, the number of fused launches among them).  float_model: the same topology with
    float Conv layers of the dequantised weights (the benchmark's yardstick)."""
    b = _B(21)
    n, _, h, w = shape
    c, e = width, 2 * width
    launches, clipped = [], []

    def conv(t, cin, cout, k, j, kernel, **kw):
        if float_model:
            y = b.conv(t, cin, cout, k, stride=kw.get("stride", 1), group=kw.get("group", 1))
            return b.op("Clip", [y, b.const(F32(0)), b.const(F32(ACT_MAX))]) if kw.get("clip", True) else y
        launches.extend([MINMAX, DYNQ, kernel])
        return b.qconv(t, cin, cout, k, j, **kw)

    t = conv("image", 3, c, 3, -1, TILE, stride=2, wmax=4, xs=2.0 ** -8)
    stem = t
    clipped.append(t)
    for _ in range(2):
        x1 = conv(t, c, e, 1, 2, TILE)
        x2 = conv(x1, e, e, 3, 2, DIRECT, group=e)
        x3 = conv(x2, e, c, 1, 3, TILE)
        t = b.op("Clip", [b.op("Add", [x3, t]), b.const(F32(0)), b.const(F32(ACT_MAX))])
        launches += ["k_binary", "k_unary("]
        clipped += [x1, x2, x3, t]
    feat = t
    up = b.op("Resize", [t, "", b.const(np.asarray([1, 1, 2, 2], F32))], mode="linear",
              coordinate_transformation_mode="half_pixel")
    launches.append("k_resize<")
    clipped.append(up)
    head = conv(up, c, 1, 3, 5, TILE, clip=False)
    matte = b.op("Sigmoid", [head])
    launches.append("k_unary(")
    names = {"matte": matte, "head": head, "feat": feat, "stem": stem, "up": up}
    outs = [(matte, [n, 1, h, w]), (head, [n, 1, h, w]), (feat, [n, c, h // 2, w // 2]), (stem, [n, c, h // 2, w // 2]),
            (up, [n, c, h, w])]
    fused = sum(k in (TILE, DIRECT) for k in launches)
    return b.model([("image", list(shape))], outs), names, clipped, launches, fused


def segmenter_feeds(shape=SHAPE):
    """Pixels j / 256, 0 and 255 present."""
    a = np.random.default_rng(22).integers(0, 256, size=shape)
    a.reshape(-1)[:2] = (0, 255)
    return {"image": (a / 256.0).astype(F32)}


def to_dynamic(data):
    """A float model with every Conv of constant weights rewritten to the dynamic form, as quantize_dynamic does:
    uint8 weights about 128 with one scale per tensor, one DynamicQuantizeLinear per quantised input (shared by
    the layers that read it), the bias a float Add.  Everything else is kept as it is."""
    m = R.load(data)
    b = _B(0)
    b.inits = dict(m.inits)
    b.k = 10 ** 6  # (new names clear of the model's own)
    dq = {}
    for nd in m.nodes:
        ins = nd["inputs"]
        if nd["op"] != "Conv" or ins[1] not in m.inits or (len(ins) > 2 and ins[2] and ins[2] not in m.inits):
            b.nodes.append(R.make_node(nd["op"], ins, nd["outputs"], domain=nd["domain"], **nd["attrs"]))
            continue
        w = m.inits[ins[1]].astype(np.float64)
        ws = max(float(np.abs(w).max()), 1e-12) / 127.0
        wq = np.clip(np.rint(w / ws) + 128, 0, 255).astype(U8)
        if ins[0] not in dq:
            dq[ins[0]] = b.op("DynamicQuantizeLinear", [ins[0]], n_out=3)
        y, sc, zp = dq[ins[0]]
        f = b.op("Cast", [b.op("ConvInteger", [y, b.const(wq), zp, b.const(U8(128))], **nd["attrs"])], to=R.DT_FLOAT)
        s = b.op("Mul", [sc, b.const(F32(ws))])
        has_bias = len(ins) > 2 and ins[2]
        out = nd["outputs"][0]
        scaled = b.name("scaled") if has_bias else out
        b.nodes.append(R.make_node("Mul", [f, s], [scaled]))
        if has_bias:
            b.nodes.append(R.make_node("Add", [scaled, b.const(m.inits[ins[2]].astype(F32).reshape(1, -1, 1, 1))], [out]))
    return R.make_model(b.nodes, b.inits, [(n, d, e) for n, e, d in m.inputs], [(n, d, e) for n, e, d in m.outputs],
                        opset=max(m.opset, 11))


# ---- the transformer block ---------------------------------------------------------------------------
T_SHAPE, HEADS, HEAD_D = (2, 40, 32), 2, 16
TIE_MARGIN = 2e-4   # steps: no element entering a DynamicQuantizeLinear lies nearer to a rounding tie
T_SEED = 38         # the input's seed, chosen for that (test_dynq_ref.py checks the margin)


def dynq_transformer():
    """(model bytes, the output's name, the float32 values entering the two DynamicQuantizeLinear nodes)."""
    b = _B(31)
    _, ntok, c = T_SHAPE
    i64 = lambda *v: b.const(np.asarray(v, np.int64))

    def linear(t, cin, cout, xq=None):
        wq = np.clip(128 + np.rint(b.rng.standard_normal((cin, cout)) * 40), 0, 255).astype(U8)
        ws = (0.0043 * (1.0 + np.arange(cout) / 11.0)).astype(F32)
        return b.qlayer(t, "MatMulInteger", wq, U8(128), ws, (b.rng.standard_normal(cout) * 0.1).astype(F32), xq=xq)

    def heads(t):  # [B, N, n d] -> [B, n, N, d]
        return b.op("Transpose", [b.op("Reshape", [t, i64(0, -1, HEADS, HEAD_D)])], perm=[0, 2, 1, 3])

    g = b.const((1.0 + 0.1 * b.rng.standard_normal(c)).astype(F32))
    be = b.const((0.1 * b.rng.standard_normal(c)).astype(F32))
    n1 = b.op("LayerNormalization", ["x", g, be], axis=-1, epsilon=1e-6)
    q, xq = linear(n1, c, c)
    k, _ = linear(n1, c, c, xq)
    v, _ = linear(n1, c, c, xq)
    kt = b.op("Transpose", [heads(k)], perm=[0, 1, 3, 2])
    sm = b.op("Softmax", [b.op("Mul", [b.op("MatMul", [heads(q), kt]), b.const(F32(HEAD_D ** -0.5))])], axis=-1)
    a = b.op("Reshape", [b.op("Transpose", [b.op("MatMul", [sm, heads(v)])], perm=[0, 2, 1, 3]), i64(0, -1, c)])
    proj, _ = linear(a, c, c)
    b.nodes.append(R.make_node("Add", ["x", proj], ["y"]))
    return b.model([("x", list(T_SHAPE))], [("y", list(T_SHAPE))], opset=17), "y", [n1, a]


def transformer_feeds(seed=T_SEED):
    return {"x": np.random.default_rng(1000 + seed).standard_normal(T_SHAPE).astype(F32)}
