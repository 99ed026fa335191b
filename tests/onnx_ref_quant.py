"""The reference for statically quantised (QDQ) graphs (test infrastructure):
QuantizeLinear and DequantizeLinear of runtime tensors, from the ONNX operator
text.  run_all() walks a model's nodes in order, evaluates these two itself in
float64 (quantised values stay uint8 / int8 arrays; a dequantised value is
rounded to float32 once) and hands every other node — the Conv, the Add, the
constant weights' DequantizeLinear among them — to onnx_ref_head.run as a
one-node model, so the references cannot drift apart.  A pattern a session
fuses (DequantizeLinear -> Conv -> Relu -> QuantizeLinear) is evaluated node by
node as written.
"""
from __future__ import annotations

import numpy as np

import onnx_ref as R
import onnx_ref_head as RH

OWN = ("QuantizeLinear", "DequantizeLinear")
RANGE = {np.dtype(np.uint8): (0, 255), np.dtype(np.int8): (-128, 127)}


def quantize_linear(x, scale, zp=None):
    """saturate(round_half_even(x / scale) + zero_point); the zero point's type, uint8 when it is absent."""
    dt = np.dtype(np.uint8) if zp is None else np.asarray(zp).dtype
    lo, hi = RANGE[dt]
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(np.asarray(x, np.float64) / np.float64(np.asarray(scale).reshape(()))) + \
            (0.0 if zp is None else np.float64(np.asarray(zp).reshape(())))
    return np.clip(v, lo, hi).astype(dt)


def dequantize_linear(x, scale, zp=None):
    """(x - zero_point) * scale in float64, rounded to float32 once."""
    z = 0.0 if zp is None else np.float64(np.asarray(zp).reshape(()))
    return ((np.asarray(x).astype(np.float64) - z) * np.float64(np.asarray(scale).reshape(()))).astype(np.float32)


def _one_node(model, nd, env, const):
    """`nd` alone through onnx_ref_head.run: its constant inputs as initializers, the others as feeds."""
    m = object.__new__(R.Model)
    m.opset = model.opset
    m.nodes = [nd]
    names = [i for i in nd["inputs"] if i]
    m.inits = {i: env[i] for i in names if i in const}
    m.inputs, m.outputs = [], []
    want = [o for o in nd["outputs"] if o] if nd["op"] == "Split" else nd["outputs"][:1]
    return RH.run(m, {i: env[i] for i in names if i not in const}, want=want)


def run_all(model, feeds):
    """Every value of `model` (an onnx_ref.Model) on numpy feeds, by name."""
    env = dict(model.inits)
    env.update({k: np.asarray(v) for k, v in feeds.items()})
    const = set(model.inits) - set(feeds)
    for nd in model.nodes:
        op = nd["op"]
        names = nd["inputs"]
        all_const = all(i in const for i in names if i)
        if all_const:
            const.update(nd["outputs"])
        if op not in OWN or all_const:
            env.update(_one_node(model, nd, env, const - set(nd["outputs"])))
            continue
        ins = [env[i] if i else None for i in names]
        for k in (1, 2):
            if len(ins) > k and ins[k] is not None:
                if names[k] not in const:
                    raise ValueError(f"{op}: a runtime scale or zero point")
                if np.asarray(ins[k]).size != 1:
                    raise ValueError(f"{op}: per-tensor quantisation of a runtime tensor only")
        zp = ins[2] if len(ins) > 2 else None
        if zp is not None and np.asarray(zp).dtype not in RANGE:
            raise ValueError(f"{op}: uint8 / int8 only")
        if op == "QuantizeLinear":
            y = quantize_linear(ins[0], ins[1], zp)
        else:
            if np.asarray(ins[0]).dtype not in RANGE:
                raise ValueError("DequantizeLinear: the runtime input is not a quantised tensor")
            y = dequantize_linear(ins[0], ins[1], zp)
        env[nd["outputs"][0]] = y
    return env


def run(model, feeds, want=None):
    """{output name: array} of `model` on numpy feeds, or every value named in `want`."""
    env = run_all(model, feeds)
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}


def unrounded(model, env, name):
    """For a graph value produced by QuantizeLinear: the reference's unrounded v = x / scale + zero_point in
    float64 (what the near-tie rule measures), else None."""
    for nd in model.nodes:
        if nd["outputs"][:1] == [name] and nd["op"] == "QuantizeLinear":
            ins = nd["inputs"]
            z = np.float64(np.asarray(env[ins[2]]).reshape(())) if len(ins) > 2 and ins[2] else 0.0
            with np.errstate(over="ignore", invalid="ignore"):
                return env[ins[0]].astype(np.float64) / np.float64(np.asarray(env[ins[1]]).reshape(())) + z
    return None
