"""The reference for the class-head operators (test infrastructure): Softmax
over any axis, LogSoftmax, ArgMax, ReduceMax, Equal, Gather and Cast to an
integer type.  run() walks a model's nodes in order, evaluates these itself in
float64 from the ONNX operator text (rounded to float32 once per node, as
oracle/onnx_ref.py does; indices and masks stay int64 / bool) and hands every
other node — the Resize in front of a head among them — to onnx_ref_ext.run as
a one-node model, so the references cannot drift apart.  A fused pattern
(Resize -> Softmax -> Gather, ArgMax -> Equal -> Cast) is evaluated node by
node as written: what a session fuses is held to the unfused definition.
"""
from __future__ import annotations

import numpy as np

import onnx_ref as R
import onnx_ref_ext as X

OWN = ("Softmax", "LogSoftmax", "ArgMax", "ReduceMax", "Equal", "Gather", "Cast")


def _axis(a, rank, default):
    ax = int(a.get("axis", default))
    if not -rank <= ax < rank:
        raise ValueError(f"axis {ax} out of range for rank {rank}")
    return ax % rank


def softmax(x, axis, log=False):
    """Softmax / LogSoftmax (opset 13 on) along `axis` in float64; float32 out."""
    xx = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = xx - xx.max(axis=axis, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=axis, keepdims=True)
    return (d - np.log(s) if log else e / s).astype(np.float32)


def argmax(x, axis, keepdims=1, select_last_index=0):
    """ArgMax: the first (or last) index of the maximum along `axis`, int64."""
    xx = x.astype(np.float64)
    if select_last_index:
        y = xx.shape[axis] - 1 - np.argmax(np.flip(xx, axis=axis), axis=axis)
    else:
        y = np.argmax(xx, axis=axis)
    y = y.astype(np.int64)
    return np.expand_dims(y, axis) if keepdims else y


def reduce_max(x, axes, keepdims=1):
    axes = tuple(int(a) % x.ndim for a in axes)
    return x.astype(np.float64).max(axis=axes, keepdims=bool(keepdims)).astype(np.float32)


def cast(x, to):
    return x.astype(R._NP[to])


def run_all(model, feeds):
    """Every value of `model` (an onnx_ref.Model) on numpy feeds, by name."""
    env = dict(model.inits)
    env.update({k: np.asarray(v) for k, v in feeds.items()})
    const = set(model.inits) - set(feeds)
    flat = 0 < model.opset < 13
    for nd in model.nodes:
        op, a = nd["op"], nd["attrs"]
        ins = [env[i] if i else None for i in nd["inputs"]]
        if all(i in const for i in nd["inputs"] if i):
            const.update(nd["outputs"])
        x = ins[0] if ins else None
        # below opset 13 Softmax is the flattened form, onnx_ref's; a Cast to a float type is onnx_ref's too
        if op not in OWN or (op in ("Softmax", "LogSoftmax") and flat) or \
                (op == "Cast" and a.get("to", 1) in (R.DT_FLOAT, R.DT_FLOAT16) and x.dtype == np.float32):
            env.update(X._one_node(model, nd, env, const - set(nd["outputs"])))
            continue
        if op in ("Softmax", "LogSoftmax"):
            y = softmax(x, _axis(a, x.ndim, -1), log=op == "LogSoftmax")
        elif op == "ArgMax":
            y = argmax(x, _axis(a, x.ndim, 0), a.get("keepdims", 1), a.get("select_last_index", 0))
        elif op == "ReduceMax":
            axes = ins[1] if len(ins) > 1 and ins[1] is not None else a.get("axes")
            if axes is None or len(axes) == 0:
                raise ValueError("ReduceMax: axes must be given")
            y = reduce_max(x, axes, a.get("keepdims", 1))
        elif op == "Equal":
            y = np.equal(x, ins[1])
        elif op == "Gather":
            idx = np.asarray(ins[1]).astype(np.int64)
            ax = _axis(a, x.ndim, 0)
            y = np.take(x, np.where(idx < 0, idx + x.shape[ax], idx), axis=ax)
        else:
            y = cast(x, a["to"])
        env[nd["outputs"][0]] = y
    return env


def run(model, feeds, want=None):
    """{output name: array} of `model` on numpy feeds, or every value named in `want`."""
    env = run_all(model, feeds)
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}


def label_source(model, name):
    """For a graph value that is a label plane or a label == k mask — ArgMax [-> Cast] or ArgMax -> Equal(k) ->
    Cast — (the logits' name, k or None, the ArgMax node's attributes); None for any other value."""
    prod = {o: nd for nd in model.nodes for o in nd["outputs"] if o}
    k, nd = None, prod.get(name)
    while nd is not None and nd["op"] in ("Cast", "Equal", "Identity", "Squeeze", "Unsqueeze", "Reshape"):
        if nd["op"] == "Equal":
            other = [i for i in nd["inputs"] if prod.get(i) is None or prod[i]["op"] != "ArgMax"]
            if len(other) != 1 or other[0] not in model.inits:
                return None
            k = float(np.asarray(model.inits[other[0]]).reshape(-1)[0])
            nd = prod.get([i for i in nd["inputs"] if i != other[0]][0])
        else:
            nd = prod.get(nd["inputs"][0])
    if nd is None or nd["op"] != "ArgMax":
        return None
    return nd["inputs"][0], k, nd["attrs"]
