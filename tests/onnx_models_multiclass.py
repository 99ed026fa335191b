"""A small multiclass segmentation net for the GPU ONNX sessions (test
infrastructure), built with onnx_models.Builder from seeded weights: the
ending of SegFormer, DeepLab / LR-ASPP and MediaPipe's multiclass selfie
model.  64 x 96 input, batch 2: three 3x3 convolutions with Relu (strides 2,
2 and 1: the features at 1/4 of the frame), a 1x1 classifier to 21 classes at
16 x 24, a linear Resize x4 to frame size, and three outputs behind it:

  person  Softmax over the classes -> Gather(15): the person probability;
  labels  ArgMax over the classes, declared int64;
  mask    ArgMax -> Equal(15) -> Cast(FLOAT): 1.0 where the label is the person.

Two exports of the same weights:
  shared    one Resize read by all three heads — the exporter's form.  A near
            miss: the full-size logits are materialised by k_resize and each
            head runs on its plain form;
  per_head  one Resize per output: three fused heads, no full-size logits.
"""
from __future__ import annotations

import numpy as np

import onnx_models as M

H, W, BATCH, CLASSES, PERSON = 64, 96, 2, 21, 15
OUTPUTS = ("person", "labels", "mask")
R = M.R


def multiclass(export="shared", seed=23):
    """(model bytes, input shape, output names) of the net as the `shared` or the `per_head` export."""
    assert export in ("shared", "per_head")
    b = M.Builder(seed)
    t = b.op("Relu", [b.conv("x", 3, 16, 3, stride=2)])
    t = b.op("Relu", [b.conv(t, 16, 32, 3, stride=2)])
    t = b.op("Relu", [b.conv(t, 32, 32, 3, stride=1)])
    # (weights of ~3 / sqrt(fan_in): logits a few units apart, as a trained classifier's)
    logits = b.op("Conv", [t, b.w(CLASSES, 32, 1, 1, scale=3.0 * 32 ** -0.5), b.w(CLASSES, scale=0.5)], kernel_shape=[1, 1])
    scales = b.const(np.array([1, 1, 4, 4], np.float32))

    def full():
        return b.op("Resize", [logits, "", scales], mode="linear", coordinate_transformation_mode="half_pixel")

    shared = full() if export == "shared" else None
    sm = b.op("Softmax", [shared or full()], axis=1)
    b.nodes.append(R.make_node("Gather", [sm, b.const(np.asarray(PERSON, np.int64))], ["person"], axis=1))
    b.nodes.append(R.make_node("ArgMax", [shared or full()], ["labels"], axis=1, keepdims=0))
    am = b.op("ArgMax", [shared or full()], axis=1, keepdims=1)
    eq = b.op("Equal", [am, b.const(np.asarray(PERSON, np.int64))])
    b.nodes.append(R.make_node("Cast", [eq], ["mask"], to=R.DT_FLOAT))
    outs = [("person", [BATCH, H, W], R.DT_FLOAT), ("labels", [BATCH, H, W], R.DT_INT64),
            ("mask", [BATCH, 1, H, W], R.DT_FLOAT)]
    return b.model([("x", [BATCH, 3, H, W])], outs), (BATCH, 3, H, W), list(OUTPUTS)


def feeds(seed=5):
    return {"x": np.random.default_rng(seed).standard_normal((BATCH, 3, H, W)).astype(np.float32)}
