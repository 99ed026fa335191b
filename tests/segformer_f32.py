"""A float32 evaluation of tests/onnx_models_segformer.py's models (test
infrastructure): every node in float32 as one GPU launch would compute it —
PyTorch's float32 convolutions and resizes, numpy float32 for the rest, the
fused kernels by the restatements of tests/test_attn_ref.py's kind
(LayerNormalization: the mean, then the variance about it).  What separates
it from the float64 reference is float32 rounding alone: the share of the bar
the net's depth costs before any kernel is wrong."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

_erf = np.frompyfunc(math.erf, 1, 1)
f = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f))


def run(model, feeds):
    """{graph output: float32 array} of an onnx_ref.Model of the segformer builder's operators."""
    env = {k: np.asarray(v) for k, v in model.inits.items()}
    env.update(feeds)
    for nd in model.nodes:
        op, a = nd["op"], nd["attrs"]
        i = [env[n] if n else None for n in nd["inputs"]]
        x = i[0]
        if op == "Conv":
            p = a["pads"]
            assert p[0] == p[2] and p[1] == p[3]
            y = F.conv2d(_t(x), _t(i[1]), _t(i[2]), stride=a["strides"], padding=(p[0], p[1]), groups=a.get("group", 1)).numpy()
        elif op == "Reshape":
            shp = [x.shape[k] if d == 0 else int(d) for k, d in enumerate(i[1])]
            y = x.reshape(shp)
        elif op == "Transpose":
            y = np.ascontiguousarray(x.transpose(a["perm"]))
        elif op == "LayerNormalization":
            mean = x.mean(axis=-1, keepdims=True, dtype=f)
            c = x - mean
            var = (c * c).mean(axis=-1, keepdims=True, dtype=f)
            y = c * (f(1.0) / np.sqrt(var + f(a["epsilon"]))) * i[1] + i[2]
        elif op == "ReduceMean":
            y = x.mean(axis=-1, keepdims=True, dtype=f)
        elif op in ("Add", "Sub", "Mul", "Div"):
            y = {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": np.divide}[op](x, i[1])
        elif op == "Pow":
            y = np.power(x, i[1])
        elif op == "Sqrt":
            y = np.sqrt(x)
        elif op == "Erf":
            y = _erf(x.astype(np.float64)).astype(f)
        elif op == "MatMul":
            y = np.matmul(x, i[1])
        elif op == "Softmax":
            e = np.exp(x - x.max(axis=-1, keepdims=True))
            y = e / e.sum(axis=-1, keepdims=True, dtype=f)
        elif op == "Resize":
            s = i[2]
            y = F.interpolate(_t(x), scale_factor=(float(s[2]), float(s[3])), mode="bilinear", align_corners=False).numpy()
        elif op == "Concat":
            y = np.concatenate(i, axis=a["axis"])
        elif op == "Relu":
            y = np.maximum(x, f(0))
        elif op == "Sigmoid":
            y = f(1.0) / (f(1.0) + np.exp(-x))
        elif op == "Identity":
            y = x
        else:
            raise ValueError(op)
        assert y.dtype == f, (op, y.dtype)
        env[nd["outputs"][0]] = y
    return {o[0]: env[o[0]] for o in model.outputs}
