"""The reference for dynamically quantised graphs (test infrastructure), the
form onnxruntime's quantize_dynamic writes: DynamicQuantizeLinear, ConvInteger
and MatMulInteger from the ONNX operator text.

DynamicQuantizeLinear is defined in float32, so it is stated in numpy float32,
one rounding per step — the oracle, and equality with it is exact:

    mn = min(0, min x), mx = max(0, max x), scale = (mx - mn) / 255,
    zp = saturate(rne((0 - mn) / scale)), y = saturate(rne(x / scale) + zp)

over the whole tensor, the batch included; mx == mn (all zero), which the text
leaves open, gives scale 1, zero point 0, y 0 as onnxruntime does.  ConvInteger
and MatMulInteger are int64 sums of (x - x_zero_point)(w - w_zero_point), stored
as int32.  run_all() walks a model's nodes in order, evaluates these three
itself and hands every other node — Cast, Mul, Add, Relu, the float layers
around them — to onnx_ref_attn.run / onnx_ref_head.run as a one-node model
(float64, rounded to float32 once per node), so the references cannot drift
apart.  A chain a session fuses (ConvInteger -> Cast -> Mul -> Add -> Relu) is
evaluated node by node as written.
"""
from __future__ import annotations

import numpy as np

import onnx_ref as R
import onnx_ref_attn as RA
import onnx_ref_head as RH
import onnx_ref_quant as RQ

OWN = ("DynamicQuantizeLinear", "ConvInteger", "MatMulInteger")
F32 = np.float32


def dynamic_quantize_linear(x):
    """(y uint8, y_scale float32 of rank 0, y_zero_point uint8 of rank 0) of a float32 tensor, in float32."""
    x = np.asarray(x, F32)
    mn = np.minimum(F32(0), x.min() if x.size else F32(0)).astype(F32)
    mx = np.maximum(F32(0), x.max() if x.size else F32(0)).astype(F32)
    if mx == mn:
        return np.zeros(x.shape, np.uint8), np.asarray(1, F32), np.asarray(0, np.uint8)
    scale = F32(F32(mx - mn) / F32(255))
    zp = np.clip(np.rint(F32(F32(F32(0) - mn) / scale)), F32(0), F32(255)).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.clip((np.rint((x / scale).astype(F32)) + zp).astype(F32), F32(0), F32(255))
    return y.astype(np.uint8), np.asarray(scale, F32), np.asarray(zp, F32).astype(np.uint8)


def _zero_point(zp, n, what):
    """A zero point as int64: 0 when absent, one value, or `n` values."""
    if zp is None:
        return np.zeros(1, np.int64)
    z = np.asarray(zp).astype(np.int64).reshape(-1)
    if z.size not in (1, n):
        raise ValueError(f"{what}: a zero point of {z.size} values for {n} channels")
    return z


def _pads(attrs, k, hw, strides, dil):
    """(top, left, bottom, right) of a convolution: pads, or auto_pad."""
    ap = attrs.get("auto_pad", "NOTSET")
    if ap in ("NOTSET", ""):
        return list(attrs.get("pads", [0, 0, 0, 0]))
    if ap == "VALID":
        return [0, 0, 0, 0]
    out = [0, 0, 0, 0]
    for d in range(2):
        o = -(-hw[d] // strides[d])
        total = max((o - 1) * strides[d] + dil[d] * (k[d] - 1) + 1 - hw[d], 0)
        lo = total // 2 if ap == "SAME_UPPER" else total - total // 2
        out[d], out[d + 2] = lo, total - lo
    return out


def conv_integer(x, w, x_zp=None, w_zp=None, attrs=None):
    """ConvInteger: sum (x - x_zp)(w - w_zp[m]) over the window in int64 (a tap outside the image adds 0), as int32."""
    a = attrs or {}
    x, w = np.asarray(x), np.asarray(w)
    n, c, h, wd = x.shape
    m, cg, kh, kw = w.shape
    g = int(a.get("group", 1))
    if c != cg * g or m % g:
        raise ValueError("ConvInteger: channel / group mismatch")
    st, dl = list(a.get("strides", [1, 1])), list(a.get("dilations", [1, 1]))
    pt, pl, pb, pr = _pads(a, (kh, kw), (h, wd), st, dl)
    zx = _zero_point(x_zp, 1, "ConvInteger x")
    if zx.size != 1:
        raise ValueError("ConvInteger: one x_zero_point only")
    xs = np.pad(x.astype(np.int64) - zx[0], ((0, 0), (0, 0), (pt, pb), (pl, pr)))  # x - zx is 0 outside the image
    ws = w.astype(np.int64) - _zero_point(w_zp, m, "ConvInteger w").reshape(-1, 1, 1, 1)
    ho = (h + pt + pb - dl[0] * (kh - 1) - 1) // st[0] + 1
    wo = (wd + pl + pr - dl[1] * (kw - 1) - 1) // st[1] + 1
    y = np.zeros((n, m, ho, wo), np.int64)
    mg = m // g
    for gi in range(g):
        xg, wg = xs[:, gi * cg:(gi + 1) * cg], ws[gi * mg:(gi + 1) * mg]
        for ky in range(kh):
            for kx in range(kw):
                win = xg[:, :, ky * dl[0]:ky * dl[0] + (ho - 1) * st[0] + 1:st[0], kx * dl[1]:kx * dl[1] + (wo - 1) * st[1] + 1:st[1]]
                y[:, gi * mg:(gi + 1) * mg] += np.einsum("nchw,mc->nmhw", win, wg[:, :, ky, kx])
    return y.astype(np.int32)  # (wraps as int32 arithmetic would)


def matmul_integer(a, b, a_zp=None, b_zp=None):
    """MatMulInteger with a 2-D B: (A - a_zp) @ (B - b_zp[column]) in int64, as int32."""
    a, b = np.asarray(a), np.asarray(b)
    if b.ndim != 2:
        raise ValueError("MatMulInteger: B of rank 2 only")
    za = _zero_point(a_zp, 1, "MatMulInteger A")
    return ((a.astype(np.int64) - za[0]) @ (b.astype(np.int64) - _zero_point(b_zp, b.shape[1], "MatMulInteger B"))).astype(np.int32)


def _one_node(model, nd, env, const):
    """`nd` alone through the float64 references: its constant inputs as initializers, the others as feeds."""
    m = object.__new__(R.Model)
    m.opset = model.opset
    m.nodes = [nd]
    names = [i for i in nd["inputs"] if i]
    m.inits = {i: env[i] for i in names if i in const}
    m.inputs, m.outputs = [], []
    want = [o for o in nd["outputs"] if o] if nd["op"] == "Split" else nd["outputs"][:1]
    run = RA.run if nd["op"] in RA.OWN else RH.run
    return run(m, {i: env[i] for i in names if i not in const}, want=want)


def run_all(model, feeds, override=None):
    """Every value of `model` (an onnx_ref.Model) on numpy feeds, by name.  override: {value name: f(its reference
    value) -> the value the nodes behind it read instead} (how far a float32 evaluation of a node moves the result)."""
    override = override or {}
    env = dict(model.inits)
    env.update({k: np.asarray(v) for k, v in feeds.items()})
    const = set(model.inits) - set(feeds)
    for nd in model.nodes:
        op, names = nd["op"], nd["inputs"]
        if all(i in const for i in names if i):
            const.update(nd["outputs"])
        ins = [env[i] if i else None for i in names] + [None] * 4
        if op == "DynamicQuantizeLinear":
            if np.asarray(ins[0]).dtype != np.float32:
                raise ValueError("DynamicQuantizeLinear: a float32 input only")
            for o, v in zip(nd["outputs"], dynamic_quantize_linear(ins[0])):
                if o:
                    env[o] = v
        elif op in ("ConvInteger", "MatMulInteger"):
            if names[1] not in const or (len(names) > 3 and names[3] and names[3] not in const):
                raise ValueError(f"{op}: constant weights and weight zero point only")
            if np.asarray(ins[0]).dtype not in RQ.RANGE:
                raise ValueError(f"{op}: input 0 is not a quantised tensor")
            env[nd["outputs"][0]] = conv_integer(ins[0], ins[1], ins[2], ins[3], nd["attrs"]) if op == "ConvInteger" \
                else matmul_integer(ins[0], ins[1], ins[2], ins[3])
        elif op in RQ.OWN and not all(i in const for i in names if i):
            zp = ins[2]
            env[nd["outputs"][0]] = RQ.quantize_linear(ins[0], ins[1], zp) if op == "QuantizeLinear" \
                else RQ.dequantize_linear(ins[0], ins[1], zp)
        else:
            env.update(_one_node(model, nd, env, const - set(nd["outputs"])))
        for o in nd["outputs"]:
            if o in override:
                env[o] = override[o](env[o])
    return env


def run(model, feeds, want=None):
    """{output name: array} of `model` on numpy feeds, or every value named in `want`."""
    env = run_all(model, feeds)
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}
