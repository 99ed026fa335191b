"""A small mix-transformer segmentation net for the GPU ONNX sessions (test
infrastructure), built with onnx_models.Builder from seeded weights: the
layout of SegFormer (Xie et al., 2021) at two stages, 64 x 96 input, batch 2.

Per stage: an overlapping patch embedding Conv (7x7 stride 4, then 3x3 stride
2) and a LayerNorm over the channels of the [B, N, C] tokens; one block —
LayerNorm, efficient self-attention (Q from the tokens; K and V from the
tokens reduced by a strided 2x2 Conv and a LayerNorm, so Nq = 4 Nk; heads 1
and 2 of d = 32; Linear projections with biases), a residual Add, LayerNorm,
Mix-FFN (Linear -> 3x3 depthwise Conv -> GELU -> Linear), a residual Add — and
the stage's LayerNorm.  Behind the stages the all-MLP decode head: a Linear
per stage, the coarser one resized x2 (linear), Concat, a 1x1 fuse Conv + Relu,
a 1x1 classifier, Resize x4 and a Sigmoid matte.

Two exports of the same weights:
  opset 17  LayerNormalization nodes, the erf form of GELU;
  opset 13  LayerNorm decomposed as PyTorch exports it below 17 (ReduceMean,
            Sub, Pow, ReduceMean, Add, Sqrt, Div, Mul, Add), the same GELU.
A session must plan both as the same launch list.
"""
from __future__ import annotations

import numpy as np

import onnx_models as M

H, W, BATCH = 64, 96, 2
STAGES = ((32, 1, 7, 4, 3), (64, 2, 3, 2, 1))  # channels, heads, patch kernel, stride, pad
SR, EMBED, HEAD_D = 2, 32, 32
BLOCKS = len(STAGES)                 # attention blocks (one per stage)
NORMS = BLOCKS * 5                   # LayerNorms: embedding, two of the block, the reduction's, the stage's


def segformer(opset=17, seed=11):
    """(model bytes, input shape, output names) of the net as an opset-17 or an opset-13 export."""
    assert opset in (13, 17)
    b = M.Builder(seed)
    i64 = lambda *v: b.const(np.asarray(v, np.int64))
    f32 = lambda v: b.const(np.float32(v))

    def layer_norm(t, c):
        g = b.const((1.0 + 0.1 * b.rng.standard_normal(c)).astype(np.float32))
        be = b.const((0.1 * b.rng.standard_normal(c)).astype(np.float32))
        if opset >= 17:
            return b.op("LayerNormalization", [t, g, be], axis=-1, epsilon=1e-6)
        d = b.op("Sub", [t, b.op("ReduceMean", [t], axes=[-1], keepdims=1)])
        var = b.op("ReduceMean", [b.op("Pow", [d, f32(2.0)])], axes=[-1], keepdims=1)
        y = b.op("Div", [d, b.op("Sqrt", [b.op("Add", [var, f32(1e-6)])])])
        return b.op("Add", [b.op("Mul", [y, g]), be])

    def linear(t, cin, cout):
        w = b.const((b.rng.standard_normal((cin, cout)) * cin ** -0.5).astype(np.float32))
        return b.op("Add", [b.op("MatMul", [t, w]), b.w(cout, scale=0.1)])

    def gelu(t):
        e = b.op("Erf", [b.op("Div", [t, f32(np.sqrt(2.0))])])
        return b.op("Mul", [b.op("Mul", [t, b.op("Add", [e, f32(1.0)])]), f32(0.5)])

    def tokens(t, c):  # [B, C, h, w] -> [B, h w, C]
        return b.op("Transpose", [b.op("Reshape", [t, i64(0, c, -1)])], perm=[0, 2, 1])

    def plane(t, c, h, w):  # [B, h w, C] -> [B, C, h, w]
        return b.op("Reshape", [b.op("Transpose", [t], perm=[0, 2, 1]), i64(0, c, h, w)])

    def heads(t, n):  # [B, N, n d] -> [B, n, N, d]
        return b.op("Transpose", [b.op("Reshape", [t, i64(0, -1, n, HEAD_D)])], perm=[0, 2, 1, 3])

    t, cin, h, w = "x", 3, H, W
    feats = []
    for c, nh, k, s, p in STAGES:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        x = layer_norm(tokens(b.conv(t, cin, c, k, stride=s, pads=[p] * 4), c), c)
        # efficient self-attention: K and V from the spatially reduced tokens
        n1 = layer_norm(x, c)
        q = heads(linear(n1, c, c), nh)
        red = b.conv(plane(n1, c, h, w), c, c, SR, stride=SR, pads=[0] * 4)
        kv = layer_norm(tokens(red, c), c)
        kt = b.op("Transpose", [heads(linear(kv, c, c), nh)], perm=[0, 1, 3, 2])
        v = heads(linear(kv, c, c), nh)
        sm = b.op("Softmax", [b.op("Mul", [b.op("MatMul", [q, kt]), f32(HEAD_D ** -0.5)])], axis=-1)
        a = b.op("Reshape", [b.op("Transpose", [b.op("MatMul", [sm, v])], perm=[0, 2, 1, 3]), i64(0, -1, c)])
        x = b.op("Add", [x, linear(a, c, c)])
        # Mix-FFN
        f = plane(linear(layer_norm(x, c), c, 4 * c), 4 * c, h, w)
        f = gelu(b.conv(f, 4 * c, 4 * c, 3, group=4 * c))
        x = b.op("Add", [x, linear(tokens(f, 4 * c), 4 * c, c)])
        t, cin = plane(layer_norm(x, c), c, h, w), c
        feats.append((t, c, h, w))
    # the all-MLP decode head
    (f1, c1, h1, w1), (f2, c2, h2, w2) = feats
    d1 = plane(linear(tokens(f1, c1), c1, EMBED), EMBED, h1, w1)
    d2 = plane(linear(tokens(f2, c2), c2, EMBED), EMBED, h2, w2)
    up = b.op("Resize", [d2, "", b.const(np.array([1, 1, 2, 2], np.float32))], mode="linear",
              coordinate_transformation_mode="half_pixel")
    fuse = b.op("Relu", [b.conv(b.op("Concat", [up, d1], axis=1), 2 * EMBED, EMBED, 1)])
    logit = b.op("Resize", [b.conv(fuse, EMBED, 1, 1), "", b.const(np.array([1, 1, 4, 4], np.float32))], mode="linear",
                 coordinate_transformation_mode="half_pixel")
    b.nodes.append(M.R.make_node("Sigmoid", [logit], ["matte"]))
    b.nodes.append(M.R.make_node("Identity", [f2], ["stage2"]))
    outs = [("matte", [BATCH, 1, H, W]), ("stage2", [BATCH, c2, h2, w2])]
    return b.model([("x", [BATCH, 3, H, W])], outs, opset=opset), (BATCH, 3, H, W), [o for o, _ in outs]


def feeds(seed=3):
    return {"x": np.random.default_rng(seed).standard_normal((BATCH, 3, H, W)).astype(np.float32)}
