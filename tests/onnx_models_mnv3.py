"""A small recurrent matting net in the reference's RVM calling convention
(test infrastructure; client/src/core/frameProcessorRVM.ts feeds r1i..r4i and
takes r1o..r4o back): MobileNetV3-style blocks, a ConvGRU per scale and a
transposed-convolution decoder, built with tests/onnx_models.py's Builder from
seeded weights.

    src [1,3,H,W], r1i [1,16,H/2,W/2], r2i [1,24,H/4,W/4]  ->  pha [1,1,H,W], r1o, r2o

  stem     Conv 3x3 s2 3 -> 16, hard-swish                               (H/2)
  block 1  1x1 16 -> 48 hs, depthwise 3x3 s2 hs, squeeze-and-excite with
           ReduceMean(axes 2, 3), 1x1 48 -> 24                           (H/4)
  block 2  1x1 24 -> 72 hs, depthwise 3x3 hs, squeeze-and-excite with
           GlobalAveragePool, 1x1 72 -> 24, + its input
  gru 2    ConvGRU on block 2's output and r2i -> r2o
  up       ConvTranspose k4 s2 p1 24 -> 16 (k_deconv_tile), Concat with the
           stem's output, Conv 3x3 32 -> 16, Relu                        (H/2)
  gru 1    ConvGRU on that and r1i -> r1o
  head     ConvTranspose k2 s2 16 -> 1 (k_deconv_direct), Sigmoid         (H)

Squeeze-and-excite: mean -> 1x1 -> Relu -> 1x1 -> HardSigmoid -> Mul.  ConvGRU:
Concat(x, h) -> 3x3 -> Sigmoid -> Split (r, z) -> Concat(x, r h) -> 3x3 -> Tanh
(c) -> (1 - z) h + z c.  hard-swish is the HardSwish operator at opset 14 and
Mul(x, HardSigmoid(x; 1/6, 0.5)) at opset 13: the two builds hold the same
weights and differ in nothing else.
"""
from __future__ import annotations

import numpy as np

import onnx_models as M

C1, C2 = 16, 24  # the channels of the two scales (and of their recurrent states)


def rvm_like(opset=14, h=32, w=48, seed=11):
    """(model bytes, {input: shape}, [outputs]) of the net above."""
    assert opset in (13, 14) and h % 4 == 0 and w % 4 == 0
    b = M.Builder(seed)

    def hs(t):
        if opset >= 14:
            return b.op("HardSwish", [t])
        return b.op("Mul", [t, b.op("HardSigmoid", [t], alpha=1.0 / 6.0, beta=0.5)])

    def se(t, c, mean):
        m = b.op("ReduceMean", [t], axes=[2, 3], keepdims=1) if mean == "ReduceMean" else b.op("GlobalAveragePool", [t])
        g = b.op("Relu", [b.conv(m, c, c // 4, 1)])
        return b.op("Mul", [t, b.op("HardSigmoid", [b.conv(g, c // 4, c, 1)])])

    def block(t, cin, cout, e, stride, mean, res):
        u = hs(b.conv(t, cin, e, 1))
        u = hs(b.conv(u, e, e, 3, stride=stride, group=e))
        u = b.conv(se(u, e, mean), e, cout, 1)
        return b.op("Add", [u, t]) if res else u

    def gru(t, hprev, c):
        rz = b.op("Sigmoid", [b.conv(b.op("Concat", [t, hprev], axis=1), 2 * c, 2 * c, 3)])
        r, z = b.op("Split", [rz], n_out=2, axis=1)
        cand = b.op("Tanh", [b.conv(b.op("Concat", [t, b.op("Mul", [r, hprev])], axis=1), 2 * c, c, 3)])
        keep = b.op("Mul", [b.op("Sub", [b.const(np.ones(1, np.float32)), z]), hprev])
        return keep, b.op("Mul", [z, cand])  # (the caller adds them into the state's output name)

    def deconv(t, cin, cout, k, stride, pad):
        taps = (-(-k // stride)) ** 2
        return b.op("ConvTranspose", [t, b.w(cin, cout, k, k, scale=(cin * taps) ** -0.5), b.w(cout, scale=0.1)],
                    kernel_shape=[k, k], strides=[stride, stride], pads=[pad] * 4)

    f1 = hs(b.conv("src", 3, C1, 3, stride=2))
    f2 = block(f1, C1, C2, 48, 2, "ReduceMean", False)
    f2 = block(f2, C2, C2, 72, 1, "GlobalAveragePool", True)
    b.nodes.append(M.R.make_node("Add", list(gru(f2, "r2i", C2)), ["r2o"]))
    up = b.op("Concat", [deconv("r2o", C2, C1, 4, 2, 1), f1], axis=1)
    d1 = b.op("Relu", [b.conv(up, 2 * C1, C1, 3)])
    b.nodes.append(M.R.make_node("Add", list(gru(d1, "r1i", C1)), ["r1o"]))
    b.nodes.append(M.R.make_node("Sigmoid", [deconv("r1o", C1, 1, 2, 2, 0)], ["pha"]))
    shapes = {"src": (1, 3, h, w), "r1i": (1, C1, h // 2, w // 2), "r2i": (1, C2, h // 4, w // 4)}
    outs = ["pha", "r1o", "r2o"]
    return b.model([(k, list(v)) for k, v in shapes.items()], [(o, []) for o in outs], opset=opset), shapes, outs


def frames(n, shape, seed=3):
    """n source frames: a slowly moving pattern plus noise, values of an image normalised to about [-1, 1]."""
    rng = np.random.default_rng(seed)
    _, c, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        base = np.stack([np.sin(0.3 * xx + 0.5 * t + k) * np.cos(0.2 * yy - 0.3 * t) for k in range(c)])
        out.append((base + 0.25 * rng.standard_normal((c, h, w)))[None].astype(np.float32))
    return out
