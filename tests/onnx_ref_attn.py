"""The reference for LayerNormalization, Gelu, Erf, Sqrt, Pow and ReduceMean
over the last axis (test infrastructure): run() walks a model's nodes in
order, evaluates these itself in float64 from the ONNX operator definitions
(rounded to float32 once per node, as oracle/onnx_ref.py does) and hands every
other node to onnx_ref_ext.run as a one-node model, so the references cannot
drift apart.  The decomposed forms (a LayerNorm of ReduceMean / Sub / Pow /
Sqrt / Div nodes, the erf GELU, an attention of MatMul / Softmax nodes) are
evaluated node by node as written: what a session fuses is held to the
unfused definition.
"""
from __future__ import annotations

import math

import numpy as np

import onnx_ref as R
import onnx_ref_ext as X

OWN = ("LayerNormalization", "Gelu", "Erf", "Sqrt", "Pow")
_erf = np.frompyfunc(math.erf, 1, 1)


def erf(x):
    return _erf(np.asarray(x, np.float64)).astype(np.float64)


def layer_norm(x, scale, bias, attrs):
    """ONNX LayerNormalization (opset 17), output 0, in float64; float32 out."""
    axis = attrs.get("axis", -1)
    if not -x.ndim <= axis < x.ndim:
        raise ValueError(f"LayerNormalization: axis {axis} out of range")
    if attrs.get("stash_type", 1) != 1:
        raise ValueError("LayerNormalization: stash_type 1 only")
    axes = tuple(range(axis % x.ndim, x.ndim))
    x = x.astype(np.float64)
    mean = x.mean(axis=axes, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=axes, keepdims=True)
    y = d / np.sqrt(var + attrs.get("epsilon", 1e-5))
    y = y * scale.astype(np.float64)
    if bias is not None:
        y = y + bias.astype(np.float64)
    return y.astype(np.float32)


def gelu(x, attrs):
    x = x.astype(np.float64)
    ap = attrs.get("approximate", "none")
    if ap == "tanh":
        return (0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))).astype(np.float32)
    if ap != "none":
        raise ValueError(f"Gelu: approximate {ap}")
    return (0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))).astype(np.float32)


def reduce_mean_last(x, attrs):
    return x.astype(np.float64).mean(axis=-1, keepdims=bool(attrs.get("keepdims", 1))).astype(np.float32)


def _last_axis(axes, rank):
    return axes is not None and [int(a) % rank for a in axes] == [rank - 1]


def _one_node(model, nd, env, const):
    """`nd` alone through onnx_ref_ext.run: its constant inputs as initializers, the others as feeds."""
    m = object.__new__(R.Model)
    m.opset = model.opset
    m.nodes = [nd]
    names = [i for i in nd["inputs"] if i]
    m.inits = {i: env[i] for i in names if i in const}
    m.inputs, m.outputs = [], []
    want = [o for o in nd["outputs"] if o] if nd["op"] == "Split" else nd["outputs"][:1]
    return X.run(m, {i: env[i] for i in names if i not in const}, want=want)


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
        x = ins[0] if ins else None
        if op == "ReduceMean":
            axes = ins[1] if len(ins) > 1 and ins[1] is not None else a.get("axes")
            if not _last_axis(axes, x.ndim):
                env.update(_one_node(model, nd, env, const - set(nd["outputs"])))
                continue
            y = reduce_mean_last(x, a)
        elif op not in OWN:
            env.update(_one_node(model, nd, env, const - set(nd["outputs"])))
            continue
        elif op == "LayerNormalization":
            if any(o for o in nd["outputs"][1:]):
                raise ValueError("LayerNormalization: the Mean / InvStdDev outputs are not supported")
            if any(i not in const for i in nd["inputs"][1:] if i):
                raise ValueError("LayerNormalization: constant Scale and B only")
            y = layer_norm(x, ins[1], ins[2] if len(ins) > 2 else None, a)
        elif op == "Gelu":
            y = gelu(x, a)
        elif op == "Erf":
            y = erf(x).astype(np.float32)
        elif op == "Sqrt":
            y = np.sqrt(x.astype(np.float64)).astype(np.float32)
        else:
            y = np.power(x.astype(np.float64), ins[1].astype(np.float64)).astype(np.float32)
        env[nd["outputs"][0]] = y
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}
