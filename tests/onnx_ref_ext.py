"""The reference for ConvTranspose, HardSigmoid, HardSwish and ReduceMean
(test infrastructure): run() walks a model's nodes in order, evaluates these
four itself in float64 from the ONNX operator definitions (rounded to float32
once per node, as oracle/onnx_ref.py does) and hands every other node to
onnx_ref.run as a one-node model, so the two cannot drift apart.

ConvTranspose is the scatter form of the definition: every input pixel adds
x * w into a zero canvas of the unpadded output size, which the pads then
crop — not the per-phase gather the GPU kernels compute.  Where ONNX leaves a
choice to its text (how an odd total padding is split under auto_pad or
output_shape), the operator text is the authority: SAME_UPPER puts total // 2
at the beginning, every other setting total - total // 2.  The geometries the
sessions refuse raise ValueError here.
"""
from __future__ import annotations

import numpy as np

import onnx_ref as R

OWN = ("ConvTranspose", "HardSigmoid", "HardSwish", "ReduceMean")


def conv_transpose_geometry(x_shape, w_shape, attrs):
    """(pads [top, left, bottom, right], (Ho, Wo), strides, dilations, output_padding) of a 2-D ConvTranspose."""
    if len(x_shape) != 4 or len(w_shape) != 4:
        raise ValueError(f"ConvTranspose: 2D only (input {x_shape}, weights {w_shape})")
    g = attrs.get("group", 1)
    if g < 1 or w_shape[0] != x_shape[1] or x_shape[1] % g:
        raise ValueError(f"ConvTranspose: channel/group mismatch (input {x_shape}, weights {w_shape}, group {g})")
    s = list(attrs.get("strides", [1, 1]))
    d = list(attrs.get("dilations", [1, 1]))
    op = list(attrs.get("output_padding", [0, 0]))
    pads = list(attrs.get("pads", [0, 0, 0, 0]))
    osz = attrs.get("output_shape")
    for name, v, want in (("strides", s, 2), ("dilations", d, 2), ("output_padding", op, 2), ("pads", pads, 4)):
        if len(v) != want:
            raise ValueError(f"ConvTranspose: {name} must have {want} values")
    if osz is not None and len(osz) != 2:
        raise ValueError("ConvTranspose: output_shape must have 2 values")
    ap = attrs.get("auto_pad", "NOTSET")
    if ap not in ("NOTSET", "VALID", "SAME_UPPER", "SAME_LOWER"):
        raise ValueError(f"ConvTranspose: auto_pad {ap}")
    begin, end, out = [0, 0], [0, 0], [0, 0]
    for a in range(2):
        if s[a] < 1 or d[a] < 1:
            raise ValueError("ConvTranspose: strides and dilations must be positive")
        if not 0 <= op[a] < max(s[a], d[a]):
            raise ValueError("ConvTranspose: output_padding must be below max(stride, dilation)")
        full = s[a] * (x_shape[2 + a] - 1) + op[a] + (w_shape[2 + a] - 1) * d[a] + 1
        if osz is not None or ap in ("SAME_UPPER", "SAME_LOWER"):
            total = full - (osz[a] if osz is not None else x_shape[2 + a] * s[a])
            if total < 0:
                raise ValueError("ConvTranspose: the output size asks for negative pads")
            begin[a] = total // 2 if ap == "SAME_UPPER" else total - total // 2
            end[a] = total - begin[a]
        elif ap == "NOTSET":
            begin[a], end[a] = pads[a], pads[a + 2]
            if begin[a] < 0 or end[a] < 0:
                raise ValueError("ConvTranspose: pads must not be negative")
        out[a] = full - begin[a] - end[a]
        if out[a] < 1:
            raise ValueError(f"ConvTranspose: empty output ({out})")
    return [begin[0], begin[1], end[0], end[1]], tuple(out), s, d, op


def conv_transpose(x, w, b, attrs):
    """ONNX ConvTranspose on NCHW in float64, scatter form; float32 out."""
    (pt, pl, pb, pr), (ho, wo), s, d, op = conv_transpose_geometry(x.shape, w.shape, attrs)
    x = x.astype(np.float64)
    w = w.astype(np.float64)
    n, c, h, wd = x.shape
    _, mg, kh, kw = w.shape
    g = attrs.get("group", 1)
    cg = c // g
    if b is not None and b.shape != (mg * g,):
        raise ValueError(f"ConvTranspose: bias must be [M] ({b.shape})")
    canvas = np.zeros((n, mg * g, ho + pt + pb, wo + pl + pr), np.float64)
    for gi in range(g):
        xs = x[:, gi * cg:(gi + 1) * cg]
        for ky in range(kh):
            for kx in range(kw):
                # every input pixel (iy, ix) adds x * w[ky, kx] at (iy s + ky d, ix s + kx d)
                add = np.tensordot(xs, w[gi * cg:(gi + 1) * cg, :, ky, kx], axes=([1], [0])).transpose(0, 3, 1, 2)
                y0, x0 = ky * d[0], kx * d[1]
                canvas[:, gi * mg:(gi + 1) * mg, y0:y0 + s[0] * (h - 1) + 1:s[0], x0:x0 + s[1] * (wd - 1) + 1:s[1]] += add
    out = canvas[:, :, pt:pt + ho, pl:pl + wo]
    if b is not None:
        out = out + b.astype(np.float64)[None, :, None, None]
    return out.astype(np.float32)


def hard_sigmoid(x, attrs):
    v = attrs.get("alpha", 0.2) * x.astype(np.float64) + attrs.get("beta", 0.5)
    return np.maximum(0.0, np.minimum(1.0, v)).astype(np.float32)


def hard_swish(x):
    x = x.astype(np.float64)
    return (x * np.maximum(0.0, np.minimum(1.0, x / 6.0 + 0.5))).astype(np.float32)


def reduce_mean(x, axes, attrs):
    """ReduceMean as the sessions take it: rank 4, over exactly H and W."""
    if x.ndim != 4:
        raise ValueError(f"ReduceMean: rank-4 input only ({x.shape})")
    axes = [] if axes is None else [int(a) for a in axes]
    if not axes and attrs.get("noop_with_empty_axes", 0):
        return x
    if sorted(a % 4 for a in axes) != [2, 3] or any(not -4 <= a < 4 for a in axes):
        raise ValueError(f"ReduceMean: the two spatial axes only ({axes})")
    return x.astype(np.float64).mean(axis=(2, 3), keepdims=bool(attrs.get("keepdims", 1))).astype(np.float32)


def _one_node(model, nd, env, const):
    """`nd` alone through onnx_ref.run: its constant inputs as initializers, the others as feeds."""
    m = object.__new__(R.Model)
    m.opset = model.opset
    m.nodes = [nd]
    names = [i for i in nd["inputs"] if i]
    m.inits = {i: env[i] for i in names if i in const}
    m.inputs, m.outputs = [], []
    want = [o for o in nd["outputs"] if o] if nd["op"] == "Split" else nd["outputs"][:1]
    return R.run(m, {i: env[i] for i in names if i not in const}, want=want)


def run(model, feeds, want=None):
    """{output name: array} of `model` (an onnx_ref.Model) on numpy feeds, or every value named in `want`."""
    env = dict(model.inits)
    env.update({k: np.asarray(v) for k, v in feeds.items()})
    const = set(model.inits) - set(feeds)
    for nd in model.nodes:
        op, a = nd["op"], nd["attrs"]
        ins = [env[i] if i else None for i in nd["inputs"]]
        if all(i in const for i in nd["inputs"] if i):
            const.update(nd["outputs"])
        if op not in OWN:
            env.update(_one_node(model, nd, env, const - set(nd["outputs"])))
            continue
        x = ins[0]
        if op == "ConvTranspose":
            if nd["inputs"][1] not in const:
                raise ValueError("ConvTranspose: weights must be constant")
            y = conv_transpose(x, ins[1], ins[2] if len(ins) > 2 else None, a)
        elif op == "HardSigmoid":
            y = hard_sigmoid(x, a)
        elif op == "HardSwish":
            y = hard_swish(x)
        else:
            if len(ins) > 1 and ins[1] is not None and nd["inputs"][1] not in const:
                raise ValueError("ReduceMean: constant axes only")
            y = reduce_mean(x, ins[1] if len(ins) > 1 and ins[1] is not None else a.get("axes"), a)
        env[nd["outputs"][0]] = y
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}
