"""A small statically quantised (QDQ) MobileNet-style person segmenter (test
infrastructure), in the form onnxruntime's quantize_static writes: every
activation between two layers is QuantizeLinear -> DequantizeLinear, every
weight DequantizeLinear of an int8 initializer, every bias DequantizeLinear of
an int32 one with the scale sx * sw.

    image [2, 3, 32, 48] -> Q -> stem 3x3 s2 (3 -> 16) Relu
      -> 2 x inverted residual (1x1 16 -> 32 Relu, 3x3 depthwise Relu, 1x1 32 -> 16, quantised residual Add)
      -> DQ -> Resize (linear, 2x) -> Q           (no fused form: the fallback in the middle of a fused graph)
      -> head 3x3 (16 -> 1) -> DQ -> Sigmoid

Outputs: the float matte, the head's uint8 tensor, the second block's int8
output.  Every scale is a power of two and the weights are small integers, so
each accumulator stays below 2^24 and a session's quantised tensors must equal
the reference's exactly (tests/op_cases_quant.py, "dyadic").
"""
from __future__ import annotations

import numpy as np

import onnx_models as M
import onnx_ref as R

Q, DQ, QCONV, QDW, QADD = "k_quantize(", "k_dequantize(", "k_qconv_tile(", "k_qconv_dw(", "k_qadd("
SHAPE = (2, 3, 32, 48)


class _B(M.Builder):
    """A quantised tensor is (name, scale, zero point)."""

    def q(self, x, scale, zp):
        return (self.op("QuantizeLinear", [x, self.const(np.float32(scale)), self.const(zp)]), scale, zp)

    def dq(self, t):
        return self.op("DequantizeLinear", [t[0], self.const(np.float32(t[1])), self.const(t[2])])

    def qconv(self, t, cin, cout, k, ys, yz, stride=1, group=1, relu=True, wmax=3, sw=2.0 ** -4):
        """DQ(t) -> Conv(DQ(Wq), DQ(Bq)) [-> Relu] -> Q."""
        wq = self.rng.integers(-wmax, wmax + 1, size=(cout, cin // group, k, k)).astype(np.int8)
        bq = self.rng.integers(-64, 65, size=cout).astype(np.int32)
        w = self.op("DequantizeLinear", [self.const(wq), self.const(np.float32(sw)), self.const(np.int8(0))])
        b = self.op("DequantizeLinear", [self.const(bq), self.const(np.float32(t[1] * sw))])
        y = self.op("Conv", [self.dq(t), w, b], kernel_shape=[k, k], strides=[stride, stride], pads=[k // 2] * 4,
                    group=group)
        if relu:
            y = self.op("Relu", [y])
        return self.q(y, ys, yz)


def qdq_segmenter(shape=SHAPE):
    """(model bytes, {"matte", "head_q", "feat_q": the graph outputs' names}, a session's launches in order, the
    number of fused launches among them)."""
    b = _B(11)
    u8, s8 = np.uint8, np.int8
    s_act = 2.0 ** -4
    t = b.q("image", 2.0 ** -8, u8(0))
    launches = [Q]
    t = b.qconv(t, 3, 16, 3, s_act, u8(0), stride=2, wmax=60)
    launches.append(QCONV)
    for blk in range(2):
        e = b.qconv(t, 16, 32, 1, s_act, u8(0), wmax=2)
        d = b.qconv(e, 32, 32, 3, s_act, u8(0), group=32, wmax=3)
        p = b.qconv(d, 32, 16, 1, s_act, s8(-3), relu=False, wmax=2)
        # the quantised residual connection; the second block's output is int8 (and a graph output)
        t = b.q(b.op("Add", [b.dq(p), b.dq(t)]), t[1] * 2, u8(128) if blk == 0 else s8(5))
        launches += [QCONV, QDW, QCONV, QADD]
    feat = t
    launches.append(DQ)  # feat_q is a graph output: its exact integers in float32
    # no fused form: DequantizeLinear, the float kernel, QuantizeLinear in the middle of a fused graph
    up = b.op("Resize", [b.dq(feat), "", b.const(np.asarray([1, 1, 2, 2], np.float32))], mode="linear",
              coordinate_transformation_mode="half_pixel")
    uq = b.q(up, feat[1], u8(128))
    launches += [DQ, "k_resize<", Q]
    head = b.qconv(uq, 16, 1, 3, 2.0 ** -3, u8(128), relu=False, wmax=2)
    launches += [QCONV, DQ]  # the head; head_q is a graph output
    matte = b.op("Sigmoid", [b.dq(head)])
    launches += [DQ, "k_unary("]
    n, _, h, w = shape
    outs = [(matte, [n, 1, h, w], R.DT_FLOAT), (head[0], [n, 1, h, w], R.DT_UINT8), (feat[0], [n, 16, h // 2, w // 2], R.DT_INT8)]
    names = {"matte": matte, "head_q": head[0], "feat_q": feat[0]}
    fused = sum(k in (QCONV, QDW, QADD) for k in launches)
    return b.model([("image", list(shape))], outs), names, launches, fused


def feeds():
    """An image in [0, 1): multiples of 1 / 512, so a share of the input quantisation's roundings are exact ties."""
    rng = np.random.default_rng(12)
    return {"image": (rng.integers(0, 512, size=SHAPE) / 512.0).astype(np.float32)}
