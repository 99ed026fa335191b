"""The ONNX oracle (oracle/onnx_ref.py) against an independent float64
evaluation of every value case of the operator matrix (tests/op_cases.py):
torch.nn.functional in double precision where torch has the operator, a
direct numpy statement of the ONNX definition where it has not (asymmetric
pads, the nearest modes, the coordinate transformations torch lacks).  Conv:
torch's conv2d in double on an input padded here, the pads worked out here.
Nothing here calls back into onnx_ref for the expected value.

Bars: data movement, MaxPool and nearest Resize compare equal; the rest agree
to 1e-6 * max(1, |want|) per element (float64 against float64, both rounded
to float32 once).  The refused cases must raise in the oracle too.

The inorm and ibn families (InstanceNormalization alone, MODNet's IBNorm
fusion) are pinned to 1e-12 and carry their own conditions: a float32
restatement of the kernels' arithmetic (tests/norm_ref.py) within half the
GPU bar, a Relu that leaves a quarter of the normalised values, and every
mutant of the restatement beyond the bar on the case made for it.

The ir family (inverted-residual blocks) is pinned to 1e-12 besides, and
carries the conditions its GPU bar rests on: a numpy restatement of the fused
kernels' arithmetic (tests/ir_ref.py) within half the bar, no saturated Clip,
and the restatement's mutants beyond the bar (at the end of this file).
"""
import numpy as np
import pytest

import onnx_ref as R
import op_cases as OC

TOL = 1e-6


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _f32(t):
    return (t.numpy() if hasattr(t, "numpy") else np.asarray(t)).astype(np.float32)


# ---- ONNX definitions torch has no operator for, stated directly ------------
def _same_pads(size, k, s, d, lower):
    """auto_pad SAME_*: the output is ceil(size / stride); the padding that needs, the odd one at the end (UPPER)."""
    out = -(-size // s)
    total = max((out - 1) * s + (k - 1) * d + 1 - size, 0)
    small, big = total // 2, total - total // 2
    return (big, small) if lower else (small, big)


def _pool_pads(at, shape):
    k, s, d = at["kernel_shape"], at.get("strides", [1, 1]), at.get("dilations", [1, 1])
    ap = at.get("auto_pad", "NOTSET")
    if ap in ("SAME_UPPER", "SAME_LOWER"):
        (t, b), (l, r) = (_same_pads(shape[2 + i], k[i], s[i], d[i], ap == "SAME_LOWER") for i in range(2))
        return [t, l, b, r]
    return [0, 0, 0, 0] if ap == "VALID" else list(at.get("pads", [0, 0, 0, 0]))


def _pool_numpy(xv, at, avg):
    """ONNX MaxPool / AveragePool, window by window.  The padded input spans
    [-pad_begin, size + pad_end); a ceil_mode window reaching past it is cut
    there.  count_include_pad=1 divides by what is left of the window,
    count_include_pad=0 by its taps on the input itself."""
    k, s, d = at["kernel_shape"], at.get("strides", [1, 1]), at.get("dilations", [1, 1])
    pt, pl, pb, pr = _pool_pads(at, xv.shape)
    h, w = xv.shape[2:]

    def out_size(size, p0, p1, kk, ss, dd):
        span = size + p0 + p1 - ((kk - 1) * dd + 1)
        o = (int(np.ceil(span / ss)) if at.get("ceil_mode", 0) else span // ss) + 1
        return o - 1 if (o - 1) * ss >= size + p0 else o  # the last window must start on the input or its left pad
    ho, wo = out_size(h, pt, pb, k[0], s[0], d[0]), out_size(w, pl, pr, k[1], s[1], d[1])
    xx = xv.astype(np.float64)
    out = np.empty(xv.shape[:2] + (ho, wo))
    for oy in range(ho):
        rows = [oy * s[0] - pt + i * d[0] for i in range(k[0])]
        rows = [r for r in rows if r < h + pb]
        for ox in range(wo):
            cols = [ox * s[1] - pl + j * d[1] for j in range(k[1])]
            cols = [q for q in cols if q < w + pr]
            inside = [(r, q) for r in rows for q in cols if 0 <= r < h and 0 <= q < w]
            vals = np.stack([xx[:, :, r, q] for r, q in inside], axis=-1)
            if avg:
                out[:, :, oy, ox] = vals.sum(-1) / (len(rows) * len(cols) if at.get("count_include_pad", 0) else len(inside))
            else:
                out[:, :, oy, ox] = vals.max(-1)
    return out.astype(np.float32)


def _pool_expected(cs, xv):
    import torch.nn.functional as F
    at = cs.attrs
    avg = cs.op == "AveragePool"
    pads = _pool_pads(at, xv.shape)
    k, s, d = tuple(at["kernel_shape"]), tuple(at.get("strides", [1, 1])), tuple(at.get("dilations", [1, 1]))
    if pads[0] != pads[2] or pads[1] != pads[3]:
        return _pool_numpy(xv, at, avg)  # torch pads both sides alike
    if avg:
        return _f32(F.avg_pool2d(_t(xv), k, s, (pads[0], pads[1]), ceil_mode=bool(at.get("ceil_mode", 0)),
                                 count_include_pad=bool(at.get("count_include_pad", 0))))
    return _f32(F.max_pool2d(_t(xv), k, s, (pads[0], pads[1]), dilation=d, ceil_mode=bool(at.get("ceil_mode", 0))))


def _resize_geometry(cs, ops):
    """(ctm, nearest_mode, mode, [(in, out, scale in float32, scale in float64)] for H and W) of a
    Resize / Upsample case: `sizes` mean the scale out / in, worked out in either precision."""
    at = cs.attrs
    xv = ops[0]
    if cs.op == "Upsample":
        ctm, nmode, scales, sizes = "asymmetric", "floor", ops[1], None
    else:
        ctm = at.get("coordinate_transformation_mode", "half_pixel")
        nmode = at.get("nearest_mode", "round_prefer_floor")
        scales = ops[2] if len(ops) > 2 and ops[2] is not None else None
        sizes = ops[3] if len(ops) > 3 else None
    dims = []
    for ax in (2, 3):
        n_in = xv.shape[ax]
        if sizes is not None:
            n_out = int(sizes[ax])
            dims.append((n_in, n_out, np.float32(n_out) / np.float32(n_in), n_out / n_in))
        else:
            dims.append((n_in, int(np.floor(n_in * float(scales[ax]))), np.float32(scales[ax]), float(scales[ax])))
    return ctm, nmode, at.get("mode", "nearest"), dims


def _src_coord(o, n_in, n_out, scale, ctm, ft):
    """x_original of output coordinate o (ONNX Resize), every operation in float type `ft`."""
    o, half = ft(o), ft(0.5)
    if ctm == "half_pixel":
        return (o + half) / ft(scale) - half
    if ctm == "pytorch_half_pixel":
        return (o + half) / ft(scale) - half if n_out > 1 else ft(0)
    if ctm == "align_corners":
        return o * ft(n_in - 1) / ft(n_out - 1) if n_out > 1 else ft(0)
    assert ctm == "asymmetric"
    return o / ft(scale)


def _nearest_index(v, nmode, n_in):
    if nmode == "round_prefer_floor":
        r = np.floor(v) if v - np.floor(v) <= 0.5 else np.ceil(v)   # halves go down
    elif nmode == "round_prefer_ceil":
        r = np.ceil(v) if v - np.floor(v) >= 0.5 else np.floor(v)   # halves go up
    elif nmode == "floor":
        r = np.floor(v)
    else:
        assert nmode == "ceil"
        r = np.ceil(v)
    return int(min(max(r, 0), n_in - 1))


def _linear_index(v, n_in):
    return int(np.floor(min(max(v, 0), n_in - 1)))


def _resize_expected(cs, ops):
    import torch.nn.functional as F
    ctm, nmode, mode, dims = _resize_geometry(cs, ops)
    xx = ops[0].astype(np.float64)
    (h, ho, _, sh), (w, wo, _, sw) = dims
    if mode == "linear" and ho > 1 and wo > 1 and ctm in ("half_pixel", "pytorch_half_pixel", "align_corners"):
        # torch's bilinear: (o + 0.5) / scale - 0.5 clamped at 0 from below, or the corner-aligned map
        kw = {"size": (ho, wo)} if cs.op == "Resize" and len(ops) > 3 else \
            {"scale_factor": (sh, sw), "recompute_scale_factor": False}
        return _f32(F.interpolate(_t(ops[0]), mode="bilinear", align_corners=ctm == "align_corners", **kw))
    if mode == "nearest":
        ys = [_nearest_index(_src_coord(o, h, ho, sh, ctm, np.float64), nmode, h) for o in range(ho)]
        xs = [_nearest_index(_src_coord(o, w, wo, sw, ctm, np.float64), nmode, w) for o in range(wo)]
        return xx[:, :, ys][:, :, :, xs].astype(np.float32)
    out = np.empty(xx.shape[:2] + (ho, wo))
    for oy in range(ho):
        cy = min(max(_src_coord(oy, h, ho, sh, ctm, np.float64), 0.0), h - 1.0)
        y0 = int(np.floor(cy))
        y1, fy = min(y0 + 1, h - 1), cy - y0
        for ox in range(wo):
            cx = min(max(_src_coord(ox, w, wo, sw, ctm, np.float64), 0.0), w - 1.0)
            x0 = int(np.floor(cx))
            x1, fx = min(x0 + 1, w - 1), cx - x0
            top = xx[:, :, y0, x0] * (1 - fx) + xx[:, :, y0, x1] * fx
            bot = xx[:, :, y1, x0] * (1 - fx) + xx[:, :, y1, x1] * fx
            out[:, :, oy, ox] = top * (1 - fy) + bot * fy
    return out.astype(np.float32)


def _onnx_slice_indices(length, start, end, step):
    """The indices ONNX Slice takes from an axis of `length`."""
    start = start + length if start < 0 else start
    end = end + length if end < 0 else end
    if step > 0:
        start, end = min(max(start, 0), length), min(max(end, 0), length)
    else:
        start, end = min(max(start, 0), length - 1), min(max(end, -1), length - 1)
    return list(range(start, end, step))


def _slice_expected(cs, ops):
    import torch
    xv = ops[0]
    if len(ops) == 1:
        starts, ends, axes, steps = cs.attrs["starts"], cs.attrs["ends"], cs.attrs.get("axes"), None
    else:
        starts, ends = ops[1], ops[2]
        axes = ops[3] if len(ops) > 3 else None
        steps = ops[4] if len(ops) > 4 else None
    axes = list(range(len(starts))) if axes is None else axes
    steps = [1] * len(starts) if steps is None else steps
    t = torch.from_numpy(xv)
    for b, e, ax, st in zip(starts, ends, axes, steps):
        ax = int(ax) % xv.ndim
        idx = _onnx_slice_indices(xv.shape[ax], int(b), int(e), int(st))
        t = t.index_select(ax, torch.tensor(idx, dtype=torch.long))
    return t.numpy()


def _pad_expected(cs, ops):
    import torch.nn.functional as F
    xv = ops[0]
    r = xv.ndim
    pads = [int(v) for v in (ops[1] if len(ops) > 1 else cs.attrs["pads"])]
    value = float(ops[2]) if len(ops) > 2 and ops[2] is not None else cs.attrs.get("value", 0.0)
    axes = [int(v) % r for v in ops[3]] if len(ops) > 3 else list(range(r))
    lo, hi = [0] * r, [0] * r
    for k, ax in enumerate(axes):
        lo[ax], hi[ax] = pads[k], pads[k + len(axes)]
    flat = []  # torch lists the last axis first; negative entries crop
    for ax in reversed(range(r)):
        flat += [lo[ax], hi[ax]]
    return F.pad(_t(xv), flat, value=value).float().numpy()


def _conv_f64(xt, w, b, at):
    """ONNX Conv of a float64 tensor, rounded to float32 once: torch's conv2d in
    double precision on an input padded here — explicit pads [top, left,
    bottom, right], or auto_pad worked out by _same_pads (auto_pad wins)."""
    import torch.nn.functional as F
    s, d, ap = at.get("strides", [1, 1]), at.get("dilations", [1, 1]), at.get("auto_pad", "NOTSET")
    if ap in ("SAME_UPPER", "SAME_LOWER"):
        (t, bt), (l, r) = (_same_pads(xt.shape[2 + i], w.shape[2 + i], s[i], d[i], ap == "SAME_LOWER") for i in range(2))
    else:
        t, l, bt, r = [0, 0, 0, 0] if ap == "VALID" else at.get("pads", [0, 0, 0, 0])
    y = F.conv2d(F.pad(xt, (l, r, t, bt)), _t(w), None if b is None else _t(b), stride=tuple(s), dilation=tuple(d),
                 groups=at.get("group", 1))
    return y.float().double()


NORM_FAMILIES = ("inorm", "ibn", "ibn9", "ibn16")


def _ev64(op, ins, at, opset):
    """One node of the norm families in double precision, its output rounded to float32 once: Conv by
    _conv_f64, the norms by their definition (two-pass sums), the rest by torch's own operators."""
    import torch
    import torch.nn.functional as F

    def T(v):
        return v if torch.is_tensor(v) else _t(v)
    x = T(ins[0])
    if op == "Conv":
        y = _conv_f64(x, ins[1], ins[2] if len(ins) > 2 else None, at)
    elif op == "InstanceNormalization":
        per_c = (1, -1) + (1,) * (x.ndim - 2)
        # a two-pass sum (torch.var_mean's running update errs by 4e-13 on a mean of 100: enough to cross
        # float32 ties on a few elements of a plane)
        plane = x.shape[:2] + (1,) * (x.ndim - 2)
        mean = (x.flatten(2).sum(dim=2) / x.flatten(2).shape[2]).reshape(plane)
        var = (((x - mean) ** 2).flatten(2).sum(dim=2) / x.flatten(2).shape[2]).reshape(plane)
        y = (x - mean) / torch.sqrt(var + float(np.float32(at.get("epsilon", 1e-5)))) * T(ins[1]).reshape(per_c) \
            + T(ins[2]).reshape(per_c)
    elif op == "BatchNormalization":
        sc, bb, mu, var = (T(v).reshape((1, -1) + (1,) * (x.ndim - 2)) for v in ins[1:5])
        y = (x - mu) / torch.sqrt(var + float(np.float32(at.get("epsilon", 1e-5)))) * sc + bb
    elif op == "Slice":
        if len(ins) > 1:
            starts, ends = ins[1], ins[2]
            axes = ins[3] if len(ins) > 3 else None
            steps = ins[4] if len(ins) > 4 else None
        else:
            starts, ends, axes, steps = at["starts"], at["ends"], at.get("axes"), None
        axes = list(range(len(starts))) if axes is None else axes
        steps = [1] * len(starts) if steps is None else steps
        y = x
        for b, e, ax, st in zip(starts, ends, axes, steps):
            ax = int(ax) % x.ndim
            idx = _onnx_slice_indices(y.shape[ax], int(b), int(e), int(st))
            y = y.index_select(ax, torch.tensor(idx, dtype=torch.long))
    elif op == "Split":
        return tuple(torch.split(x, [int(v) for v in ins[1]], dim=at["axis"]))
    elif op == "Concat":
        y = torch.cat([T(v) for v in ins], dim=at["axis"])
    else:
        assert op == "Relu", op
        y = F.relu(x)
    return y.float().double()


def _norm_expected(cs, ops, chain_ops):
    import norm_ref
    return [_f32(o) for o in norm_ref.walk(cs, ops, chain_ops, _ev64)]


def expected(cs, ops, chain_ops=()):
    """Outputs of the case (a list), evaluated independently of onnx_ref."""
    import torch
    import torch.nn.functional as F
    op, at = cs.op, cs.attrs
    xv = ops[0]
    if cs.family in NORM_FAMILIES:
        return _norm_expected(cs, ops, chain_ops)
    if op in ("MaxPool", "AveragePool"):
        return [_pool_expected(cs, xv)]
    if op in ("Resize", "Upsample"):
        return [_resize_expected(cs, ops)]
    if op == "Conv":  # then the nodes behind it
        y = _conv_f64(_t(xv), ops[1], ops[2] if len(ops) > 2 else None, at)
        follow = [(cs.post[0], [cs.post[1]], {}, {})] if cs.post else \
            [(nd[0], more, nd[2], nd[3] if len(nd) > 3 else {}) for nd, more in zip(cs.chain, chain_ops)]
        made, outs = [y], []  # every node's output (a chain operand may name one), the further graph outputs
        for op_, more, at_, opts in follow:
            # a reference ("prev" | "in", k | "node", j) to another value of the case, or the operand itself
            ins = [(made[-1] if v[0] == "prev" else _t(ops[v[1]]) if v[0] == "in" else made[v[1]])
                   if isinstance(v, tuple) else v for v in more]
            if not opts.get("whole"):
                ins = [made[-1]] + ins
            y = ins[0]
            if op_ == "Conv":
                y = _conv_f64(y, ins[1], ins[2] if len(ins) > 2 else None, at_)
            elif op_ == "Add":
                y = y + (ins[1] if torch.is_tensor(ins[1]) else _t(ins[1]))
            elif op_ == "Relu":
                y = F.relu(y)
            elif op_ == "Clip":  # bounds as inputs (either may be absent) or, before opset 11, attributes
                lo = at_.get("min") if len(ins) < 2 or ins[1] is None else float(ins[1])
                hi = at_.get("max") if len(ins) < 3 or ins[2] is None else float(ins[2])
                y = torch.clamp(y, lo, hi) if lo is not None or hi is not None else y
            elif op_ == "LeakyRelu":
                y = F.leaky_relu(y, float(np.float32(at_.get("alpha", 0.01))))
            elif op_ == "MaxPool":
                assert set(at_) == {"kernel_shape", "strides"}, at_
                y = F.max_pool2d(y, tuple(at_["kernel_shape"]), tuple(at_["strides"]))
            elif op_ == "Pad":  # zeros appended to the channels
                pads = [int(v) for v in ins[1]]
                assert len(pads) == 8 and not any(pads[:5] + pads[6:]), pads
                y = torch.cat([y, torch.zeros(y.shape[0], pads[5], *y.shape[2:], dtype=y.dtype)], dim=1)
            else:
                assert op_ == "PRelu", op_
                y = torch.where(y < 0, y * _t(ins[1]), y)
            y = y.float().double()  # every node's own float32 output
            made.append(y)
            if opts.get("out"):
                outs.append(y)
        return ([xv] if cs.echo else []) + [_f32(o) for o in outs + [y]]
    if op == "Relu":
        return [_f32(F.relu(_t(xv)))]
    if op == "LeakyRelu":
        return [_f32(F.leaky_relu(_t(xv), float(np.float32(at.get("alpha", 0.01)))))]
    if op == "Sigmoid":
        return [_f32(torch.sigmoid(_t(xv)))]
    if op == "Tanh":
        return [_f32(torch.tanh(_t(xv)))]
    if op == "Clip":
        lo = float(ops[1]) if len(ops) > 1 and ops[1] is not None else at.get("min")
        hi = float(ops[2]) if len(ops) > 2 and ops[2] is not None else at.get("max")
        return [_f32(torch.clamp(_t(xv), lo, hi)) if lo is not None or hi is not None else xv]
    if op == "PRelu":
        sl = ops[1]
        if sl.size == 1 or (sl.ndim >= 3 and sl.shape[-3] == sl.size == xv.shape[1]):  # one value, or per channel
            return [_f32(F.prelu(_t(xv), _t(sl).reshape(-1)))]
        return [_f32(torch.where(_t(xv) < 0, _t(xv) * _t(sl), _t(xv)))]  # numpy-style broadcast of the slope
    if op in ("Add", "Sub", "Mul", "Div"):
        fn = {"Add": torch.add, "Sub": torch.sub, "Mul": torch.mul, "Div": torch.div}[op]
        return [_f32(fn(_t(ops[0]), _t(ops[1])))]
    if op == "Slice":
        return [_slice_expected(cs, ops)]
    if op == "Concat":
        return [torch.cat([torch.from_numpy(o) for o in ops], dim=at["axis"]).numpy()]
    if op == "Split":
        ax = at.get("axis", 0)
        n = xv.shape[ax]
        if len(ops) > 1:
            sizes = [int(v) for v in ops[1]]
        elif "split" in at:
            sizes = list(at["split"])
        else:  # equal parts; opset 18: ceil-sized parts, the last one smaller
            part = -(-n // cs.n_out)
            sizes = [min(part, n - k * part) for k in range(cs.n_out)]
            assert cs.opset >= 18 or n % cs.n_out == 0
        return [t.numpy() for t in torch.split(torch.from_numpy(xv), sizes, dim=ax)]
    if op == "Transpose":
        return [torch.from_numpy(xv).permute(*at.get("perm", list(range(xv.ndim))[::-1])).contiguous().numpy()]
    if op == "Pad":
        return [_pad_expected(cs, ops)]
    if op == "Squeeze":
        axes = at.get("axes", ops[1] if len(ops) > 1 else None)
        t = torch.from_numpy(xv)
        for ax in sorted((int(a) % xv.ndim for a in axes), reverse=True) if axes is not None else ():
            t = t.squeeze(ax)
        return [(t if axes is not None else t.squeeze()).numpy()]
    if op == "Unsqueeze":
        axes = at.get("axes", ops[1] if len(ops) > 1 else None)
        t = torch.from_numpy(xv)
        for ax in sorted(int(a) % (xv.ndim + len(axes)) for a in axes):
            t = t.unsqueeze(ax)
        return [t.numpy()]
    if op == "Flatten":
        ax = at.get("axis", 1)
        ax = ax + xv.ndim if ax < 0 else ax
        return [torch.from_numpy(xv).reshape(int(np.prod(xv.shape[:ax], dtype=np.int64)), -1).numpy()]
    if op == "Reshape":
        shp = [xv.shape[k] if v == 0 else int(v) for k, v in enumerate(ops[1])]
        return [torch.from_numpy(xv).reshape(shp).numpy()]
    if op == "Gemm":
        a, b = _t(ops[0]), _t(ops[1])
        y = float(np.float32(at.get("alpha", 1.0))) * ((a.T if at.get("transA") else a) @ (b.T if at.get("transB") else b))
        if len(ops) > 2:
            y = y + float(np.float32(at.get("beta", 1.0))) * _t(ops[2])
        return [_f32(y)]
    if op == "MatMul":
        return [_f32(torch.matmul(_t(ops[0]), _t(ops[1])))]
    if op == "BatchNormalization":
        w, b, mean, var = (_t(o) for o in ops[1:5])
        return [_f32(F.batch_norm(_t(xv), mean, var, w, b, training=False, eps=float(np.float32(at.get("epsilon", 1e-5)))))]
    if op == "InstanceNormalization":
        eps = float(np.float32(at.get("epsilon", 1e-5)))
        if int(np.prod(xv.shape[2:])) == 1:  # torch refuses single-element planes: (x - x) / sqrt(0 + eps) * w + b
            return [np.broadcast_to(ops[2].reshape((1, -1) + (1,) * (xv.ndim - 2)), xv.shape).astype(np.float32)]
        return [_f32(F.instance_norm(_t(xv), weight=_t(ops[1]), bias=_t(ops[2]), eps=eps))]
    if op == "GlobalAveragePool":
        return [_f32(_t(xv).flatten(2).mean(dim=2).reshape(xv.shape[:2] + (1,) * (xv.ndim - 2)))]
    if op == "Softmax":
        if cs.opset < 13:  # the input as a matrix [prod(:axis), prod(axis:)], each row normalised
            ax = at.get("axis", 1) % xv.ndim
            m = _t(xv).reshape(int(np.prod(xv.shape[:ax], dtype=np.int64)), -1)
            return [_f32(F.softmax(m, dim=1).reshape(xv.shape))]
        return [_f32(F.softmax(_t(xv), dim=at.get("axis", -1)))]
    raise AssertionError(f"no independent evaluation for {op}")


# ---- the tests ---------------------------------------------------------------
_runs = {}


def _oracle_outputs(cs):
    """The oracle's outputs of the case, from one run of its whole family's model."""
    if cs.family not in _runs:
        fam = OC.groups()[cs.family]
        data, feeds, outs = OC.build(fam)
        try:
            _runs[cs.family] = (feeds, outs, R.run(R.load(data), feeds), None)
        except Exception as e:  # one broken case must not hide the others: run them one by one
            _runs[cs.family] = (feeds, outs, None, e)
    feeds, outs, got, err = _runs[cs.family]
    if got is None:
        data, feeds, outs = OC.build([cs])
        got = R.run(R.load(data), feeds)
    return feeds, [got[o] for o in outs[cs.name]]


@pytest.mark.parametrize("name", [k.name for k in OC.VALUE_CASES])
def test_oracle_matches_independent_f64(name):
    cs = OC.BY_NAME[name]
    feeds, got = _oracle_outputs(cs)
    want = expected(cs, OC.operands(cs, feeds), OC.chain_operands(cs, feeds))
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and w.dtype == np.float32, (name, k, g.dtype, w.dtype)
        assert g.shape == w.shape, (name, k, g.shape, w.shape)
        if cs.exact:
            assert np.array_equal(g, w), (name, k, float(np.abs(g - w).max()))
        else:
            excess = np.abs(g.astype(np.float64) - w) - TOL * np.maximum(1.0, np.abs(w))
            assert excess.max() <= 0, (name, k, float(np.abs(g.astype(np.float64) - w).max()))


@pytest.mark.parametrize("name", [k.name for k in OC.REFUSED_CASES])
def test_oracle_refuses(name):
    cs = OC.BY_NAME[name]
    data, feeds, _ = OC.build([cs])
    with pytest.raises((ValueError, NotImplementedError), match=cs.post[0] if cs.post else cs.op):
        R.run(R.load(data), feeds)


RESIZE_INDEX_CASES = [k.name for k in OC.VALUE_CASES if k.op in ("Resize", "Upsample")]


@pytest.mark.parametrize("name", RESIZE_INDEX_CASES)
def test_resize_indices_agree_in_f32_and_f64(name):
    """A condition on the inputs: k_resize works its source coordinates out in
    float32 (as onnxruntime does), the oracle in float64.  A case is only
    meaningful where both select the same source index for every output
    coordinate (nearest: the index taken; linear: the lower neighbour)."""
    cs = OC.BY_NAME[name]
    data, feeds, _ = OC.build([cs])
    ctm, nmode, mode, dims = _resize_geometry(cs, OC.operands(cs, feeds))
    for n_in, n_out, scale32, scale64 in dims:
        assert n_out >= 1
        for o in range(n_out):
            v32 = _src_coord(o, n_in, n_out, scale32, ctm, np.float32)
            v64 = _src_coord(o, n_in, n_out, scale64, ctm, np.float64)
            assert isinstance(v32, np.float32)
            if mode == "nearest":
                assert _nearest_index(v32, nmode, n_in) == _nearest_index(v64, nmode, n_in), (name, n_in, n_out, o, v32, v64)
            else:
                assert _linear_index(v32, n_in) == _linear_index(v64, n_in), (name, n_in, n_out, o, v32, v64)


def test_matrix_covers_the_kernel_forms():
    """Each kernel form the GPU file asserts has a case that names it."""
    named = {k for cs in OC.VALUE_CASES for k in cs.kernels}
    for form in ("k_resize<true>(", "k_resize<false>(", "k_gap_wave(", "k_gap(", "k_gemm<true>(", "k_gemm<false>(",
                 "k_binary_planes(", "k_binary(", "k_copy_rows<true>(", "k_copy_rows<false>(", "k_copy(", "k_affine(",
                 # the convolutions (k_conv_tile: tests/test_gpu_conv_tile_matrix.py)
                 *(OC.small(pw, ch, split) for pw in (False, True) for ch, split in ((8, False), (16, False),
                                                                                      (32, False), (16, True))),
                 "k_conv_gemm(", "k_conv_dw(", "k_conv_dw_plane<1>(", "k_conv_dw_plane<2>(", "k_conv_dwpw(",
                 *(f"k_conv_pw<{wm}, {dwk}>(" for wm in (1, 2, 4) for dwk in (0, 3, 5)),
                 *(f"k_conv_thin<{m}>(" for m in (1, 2, 3, 4))):
        assert form in named, form
    # the four-outputs-per-thread body inside k_conv_dw shares its launch name with the flat one
    quad = OC.BY_NAME["Conv_dw_quad_body"]
    n, c, h, w = quad.inputs[0][1]
    assert quad.kernels == ("k_conv_dw(",) and n * c > 65535 and n * c * h * w // 4 >= 1024 * 256 and w % 4 == 0


# ---- the ir family: inverted-residual blocks (csrc/vso_ir.hip) -------------------
# The GPU bar of the matrix (tests/test_gpu_op_matrix.py), per element.
BAR = 1e-4
IR = [k for k in OC.VALUE_CASES if k.family in ("ir", "ir6")]
IR_FUSED = [k for k in IR if any("k_ir" in n for n in k.kernels + k.kernels16)]
IR_MISSES = [k for k in IR if k not in IR_FUSED]
_ir_memo = {}


def _ir_restated(cs, form, mutant=None):
    """(the oracle's outputs, the restatement's, its Clips' inputs) of a fused case."""
    import ir_ref
    key = (cs.name, form, mutant)
    if key not in _ir_memo:
        feeds, want = _oracle_outputs(cs)
        got, clips = ir_ref.run(cs, OC.operands(cs, feeds), OC.chain_operands(cs, feeds), form, mutant)
        _ir_memo[key] = (want, got, clips)
    return _ir_memo[key]


def _err_over_bar(got, want):
    """The worst |got - want| / (BAR * max(1, |want|)) over the outputs' elements."""
    assert len(got) == len(want) and all(g.shape == w.shape for g, w in zip(got, want))
    return max(float((np.abs(g.astype(np.float64) - w) / (BAR * np.maximum(1.0, np.abs(w)))).max())
               for g, w in zip(got, want))


@pytest.mark.parametrize("name", [k.name for k in IR])
def test_ir_oracle_pinned_to_f64(name):
    """onnx_ref on every case of the family against the independent float64
    evaluation above (torch's conv2d in double on an input padded here), to
    1e-12 relative: both round every node's output to float32 once, so they
    differ only where a float64 sum of another order rounds across a float32
    tie — which these cases' values do not."""
    cs = OC.BY_NAME[name]
    feeds, got = _oracle_outputs(cs)
    want = expected(cs, OC.operands(cs, feeds), OC.chain_operands(cs, feeds))
    assert len(got) == len(want) == cs.n_out + cs.echo
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32
        assert (np.abs(g.astype(np.float64) - w) <= 1e-12 * np.maximum(1.0, np.abs(w))).all(), \
            (name, float(np.abs(g.astype(np.float64) - w).max()))


def test_ir_family_rounds_no_operand():
    """No convolution of the family is one a 16-bit session tiles (onnx_ref.tiled_conv):
    the oracle of a bf16 / f16 session is the f32 one."""
    for cs in IR:
        convs = [(cs.inputs[1][1], cs.attrs)] + [(nd[1][0][1], nd[2]) for nd in cs.chain if nd[0] == "Conv"]
        assert len(convs) % 3 == 0 and not any(R.tiled_conv(w, at_) for w, at_ in convs), cs.name


def test_ir_family_covers_the_forms():
    """Every instance of kIr and kIr16 (vso_ir.hip) and k_ir_reduce has a case
    that names it; the near misses and the cases without an f32 form name none."""
    f32 = {n for cs in IR for n in cs.kernels if n.startswith("k_ir")}
    b16 = {n for cs in IR for n in cs.kernels16 if n.startswith("k_ir")}
    entries = [(1, 2, 2), (2, 2, 1), (2, 2, 2), (2, 4, 2), (4, 4, 1), (4, 6, 1), (6, 6, 1), (6, 10, 2), (10, 10, 1),
               (10, 20, 1), (4, 4, 2), (6, 6, 2)]
    entries16 = [(1, 2, 2), (1, 2, 1), (1, 4, 2), (2, 4, 1), (2, 6, 1), (3, 6, 1), (3, 10, 2), (5, 10, 1), (5, 20, 1),
                 (2, 4, 2), (3, 6, 2)]
    assert f32 == {f"k_ir<{a}, {b}, {s}, 4>(" for a, b, s in entries} | {"k_ir_reduce("}
    assert b16 == {f"k_ir_b16<{a}, {b}, {s}, 4>(" for a, b, s in entries16} | {"k_ir_reduce("}
    for cs in IR_MISSES:
        assert cs.kernels == cs.kernels16 and cs.kernels and not any("k_ir" in n for n in cs.kernels), cs.name
    for name in ("IR_16_24_s1", "IR_48_64_s1"):
        cs = OC.BY_NAME[name]
        assert not any("k_ir" in n for n in cs.kernels) and "k_ir_b16<" in cs.kernels16[0]
    # one slice (no reduce launch) and several, in either precision
    for field in ("kernels", "kernels16"):
        assert {("k_ir_reduce(" in getattr(cs, field)) for cs in IR_FUSED} == {False, True}


@pytest.mark.parametrize("form", ["f32", "b16"])
@pytest.mark.parametrize("name", [k.name for k in IR_FUSED])
def test_ir_restatement_inside_half_the_bar(name, form):
    """Condition 1 on the inputs: each form's arithmetic, restated (tests/ir_ref.py),
    is within half the bar of the oracle on every element — a kernel that
    computes what it says has the other half for its own association."""
    cs = OC.BY_NAME[name]
    want, got, _ = _ir_restated(cs, form)
    ratio = _err_over_bar(got, want)
    print(f"{name} {form}: restatement err / bar {ratio:.4f}")
    assert ratio <= 0.5, (name, form, ratio)


@pytest.mark.parametrize("name", [k.name for k in IR_FUSED])
def test_ir_clips_not_saturated(name):
    """Condition 2 on the inputs: at least a quarter of the expand's outputs, and
    of the depthwise's, lie strictly inside their Clip's range (a saturated
    clip hides the errors of what feeds it).  A Clip without both bounds has
    no range to saturate."""
    cs = OC.BY_NAME[name]
    _, _, clips = _ir_restated(cs, "f32")
    assert len(clips) >= 2
    for k, (v, lo, hi) in enumerate(clips):
        if lo is None or hi is None:
            continue
        share = float(((v > lo) & (v < hi)).mean())
        print(f"{name} clip {k}: {share:.3f} inside ({lo}, {hi})")
        assert share >= 0.25, (name, k, share)


@pytest.mark.parametrize("mutant,name,form", [
    ("drop_wl_xh", "IR_96_96_res", "b16"),
    ("pad_clip", "IR_24_24_res_clip0.5_4", "f32"),
    ("pad_clip", "IR_24_24_res_clip0.5_4", "b16"),
    ("swap_taps", "IR_24_24_res", "f32"),
    ("swap_taps", "IR_16_24_s2", "b16"),
    ("no_res", "IR_24_24_res", "f32"),
    ("no_res", "IR_24_24_res_swapped", "b16"),
    ("drop_last_chunk", "IR_24_24_res_hid48", "b16"),
    ("drop_last_chunk", "IR_20_20_res", "f32"),
    ("cout_tail", "IR_28_49_s2", "f32"),
    ("cout_tail", "IR_84_81", "b16"),
    ("cout_tail", "IR_148_305", "b16"),
    ("cin_tail", "IR_20_20_res", "f32"),
    ("cin_tail", "IR_148_305", "f32"),
])
def test_ir_mutant_leaves_the_bar(mutant, name, form):
    """Each way the kernels could be wrong, applied to the restatement, is beyond
    the bar on the case made for it (and the restatement itself is not)."""
    cs = OC.BY_NAME[name]
    want, good, _ = _ir_restated(cs, form)
    _, bad, _ = _ir_restated(cs, form, mutant)
    ratio = _err_over_bar(bad, want)
    print(f"{name} {form} {mutant}: err / bar {ratio:.1f}")
    assert _err_over_bar(good, want) <= 0.5 and ratio > 1.0, (mutant, name, form, ratio)


# ---- the norm families: InstanceNormalization alone and the IBNorm fusion -----------
NORM = [k for k in OC.VALUE_CASES if k.family in NORM_FAMILIES]
IBN_FUSED = [k for k in NORM if k.name in OC.IBN and OC.IBN[k.name]["fused"]]
_norm_memo = {}


def _norm_restated(cs, mutant=None, plane=True, thin=True):
    """(the oracle's outputs, the restatement's (tests/norm_ref.py), what it kept) of a case."""
    import norm_ref as NR
    key = (cs.name, mutant, plane, thin)
    if key not in _norm_memo:
        feeds, want = _oracle_outputs(cs)
        ops, chain_ops, keep = OC.operands(cs, feeds), OC.chain_operands(cs, feeds), {}
        if cs in IBN_FUSED:
            got = NR.run_ibn(cs, OC.IBN[cs.name], ops, chain_ops, mutant, plane, thin, keep)
        elif cs.family == "inorm":
            y = NR.inorm(ops[0], ops[1], ops[2], float(np.float32(cs.attrs.get("epsilon", 1e-5))), mutant, plane)
            got = [np.maximum(y, np.float32(0)) if cs.chain else y]
        else:
            assert mutant is None
            got = NR.walk(cs, ops, chain_ops, NR.ev32(plane))
        _norm_memo[key] = (want, got, keep)
    return _norm_memo[key]


@pytest.mark.parametrize("name", [k.name for k in NORM])
def test_norm_oracle_pinned_to_f64(name):
    """onnx_ref on every case of the inorm and ibn families against the independent float64 evaluation
    above (_ev64: conv2d in double on an input padded here, a two-pass mean and variance), to 1e-12 relative."""
    cs = OC.BY_NAME[name]
    feeds, got = _oracle_outputs(cs)
    want = expected(cs, OC.operands(cs, feeds), OC.chain_operands(cs, feeds))
    assert len(got) == len(want) == cs.n_out
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32
        assert (np.abs(g.astype(np.float64) - w) <= 1e-12 * np.maximum(1.0, np.abs(w))).all(), \
            (name, float(np.abs(g.astype(np.float64) - w).max()))


@pytest.mark.parametrize("name", [k.name for k in NORM])
def test_norm_restatement_inside_half_the_bar(name):
    """Each form's arithmetic, restated in float32, is within half the bar of the oracle on every element
    (a `half` case: exactly B[c], as the oracle); where a Relu follows the norm, at least a quarter of the
    normalised outputs are positive (a Relu that clips nearly all of them hides the norm's errors)."""
    cs = OC.BY_NAME[name]
    want, got, keep = _norm_restated(cs)
    ratio = _err_over_bar(got, want)
    print(f"{name}: restatement err / bar {ratio:.4f}")
    assert ratio <= 0.5, (name, ratio)
    if cs.exact:
        b = cs.inputs[2][1].reshape((1, -1) + (1,) * (got[0].ndim - 2))
        assert np.array_equal(got[0], np.broadcast_to(b, got[0].shape)) and np.array_equal(want[0], got[0])
    relu = OC.IBN[name]["relu"] if name in OC.IBN else bool(cs.chain)
    if relu and (cs.family == "inorm" or cs in IBN_FUSED):
        v = keep["normalised"] if cs in IBN_FUSED else got[0]
        share = float((v > 0).mean())
        print(f"{name}: {share:.3f} of the normalised outputs positive")
        assert share >= 0.25, (name, share)


def test_norm_families_cover_the_forms():
    """Every launch the GPU file asserts has a case naming it: the plane instances in their float4 and scalar
    forms on both sides of each limit, the pair, and k_conv_thin<1..4> behind a deferred norm."""
    inn = [k for k in NORM if k.family == "inorm"]
    inner = lambda k: int(np.prod(k.inputs[0][1][2:]))
    for form, lo, hi in ((OC.PLANE16, 1, 4096), (OC.PLANE48, 4097, 12288), (OC.PLANE36, 12289, 36864)):
        sizes = {inner(k) for k in inn if k.kernels[0] == form}
        assert {lo, hi} <= sizes and all(lo <= v <= hi for v in sizes), (form, sizes)
        assert {v % 4 == 0 for v in sizes} == {False, True}
    pair = {inner(k) for k in inn if k.kernels[:2] == (OC.STATS, OC.APPLY)}
    assert {36865, 36868, 40960, 262656, 525625} <= pair and min(pair) == 36865
    deferred = [k for k in IBN_FUSED if OC.IBN[k.name]["defer"]]
    assert {k.kernels[-1] for k in deferred} >= {OC.THIN % m for m in (1, 2, 3, 4)}
    assert all(k.kernels[1] == OC.STATS and OC.APPLY not in k.kernels for k in deferred if k.name != "IBN_head_ibn_63")
    planes = {inner(k) for k in deferred}
    assert {63, 4096, 36865, 262656, 525625} <= planes  # 1 piece, 10 (the last of 1), 65, 129
    assert any(OC.IBN[k.name]["cat"] and OC.IBN[k.name]["cat"][0] == q for k in IBN_FUSED for q in (0, 1))
    convs = {k.kernels[0] for k in IBN_FUSED}
    assert {"k_conv_tile<", OC.small(False, 8, False), OC.pw_name(5), OC.pw_name(24), OC.pw_name(256)} <= convs
    m_nb = {(OC.IBN[k.name]["m"], OC.IBN[k.name]["nb"]) for k in IBN_FUSED}
    assert m_nb >= {(5, 1), (5, 4), (24, 12), (24, 7), (32, 16), (32, 5)}
    for k in NORM:
        assert k.kernels, k.name


NORM_MUTANTS = [
    ("cnt_m1", "IN_2"), ("cnt_m1", "IN_3"), ("cnt_m1", "IN_5"),
    ("last_full", "IN_36865"), ("last_full", "IBN_thin2_36865"),
    ("no_between", "IN_40960"), ("no_between", "IN_262656"), ("no_between", "IBN_thin2_36865"),
    ("no_between", "IBN_thin3_262656"),
    ("drop64", "IBN_thin3_262656"), ("drop64", "IBN_thin4_525625"),
    ("one_pass", "IN_4095_off100"), ("one_pass", "IN_12288_off100"), ("one_pass", "IN_36863_off100"),
    ("one_pass", "IN_36868_off100"),
    ("no_eps", "IN_4095_small_eps1e-5"), ("no_eps", "IN_12288_small_eps1e-3"), ("no_eps", "IN_36863_small_eps1e-5"),
    ("no_eps", "IN_36868_small_eps1e-3"), ("no_eps", "IN_default_eps"), ("no_eps", "IBN_thin2_63_small"),
    ("bn_no_eps", "IBN_pw_M5_nb2_var0.01"),
    ("c0_zero", "IBN_pw_M5_nb1_4"), ("c0_zero", "IBN_thin1_63"), ("c0_zero", "IBN_tile_M32_nb16_2304"),
    ("c0_zero", "IBN_cat_second_63"),
    ("ctot_M", "IBN_cat_first_63"), ("ctot_M", "IBN_cat_second_63"), ("ctot_M", "IBN_cat_second_36868"),
    ("stats_img0", "IN_63_relu"), ("stats_img0", "IN_36868"), ("stats_img0", "IBN_thin2_36865"),
    ("stats_img0", "IBN_cat_first_63"),
    ("relu_all", "IBN_pw_M5_nb4_63_neg"), ("relu_all", "IBN_thin4_4096"), ("relu_all", "IBN_cat_second_63"),
    ("no_relu_norm", "IBN_pw_M5_nb1_4"), ("no_relu_norm", "IBN_thin1_63"), ("no_relu_norm", "IBN_cat_first_63"),
    ("no_relu_norm", "IBN_tile_thin2_2304"),
]


@pytest.mark.parametrize("mutant,name", NORM_MUTANTS)
def test_norm_mutant_leaves_the_bar(mutant, name):
    """Each way the norm kernels or the fusion could be wrong, applied to the restatement, is beyond the bar
    on the case made for it, while the restatement itself stays within half of it."""
    cs = OC.BY_NAME[name]
    want, good, _ = _norm_restated(cs)
    _, bad, _ = _norm_restated(cs, mutant)
    ratio = _err_over_bar(bad, want)
    print(f"{name} {mutant}: err / bar {ratio:.1f} (the restatement: {_err_over_bar(good, want):.4f})")
    assert _err_over_bar(good, want) <= 0.5 and ratio > 1.0, (mutant, name, ratio)


def test_every_norm_mutant_has_a_case():
    import norm_ref as NR
    assert {m for m, _ in NORM_MUTANTS} == set(NR.MUTANTS)


@pytest.mark.parametrize("name", [k.name for k in NORM if k.family == "ibn16"])
def test_ibn16_fold_commutes_with_rounding(name):
    """A 16-bit session folds the BatchNorm into the conv's weights and then rounds them; the oracle
    (R.run(conv_operands=...)) rounds the weights and then applies the BatchNorm.  With the family's
    constants the fold factor is a power of two, so the two orders give the same weights bit for bit."""
    cs = OC.BY_NAME[name]
    meta = OC.IBN[name]
    w = cs.inputs[1][1]
    sc, _, _, var = (spec[1].astype(np.float64) for spec in cs.chain[meta["i_bn"] - 1][1][1:5])
    a = sc / np.sqrt(var + float(np.float32(cs.chain[meta["i_bn"] - 1][2]["epsilon"])))
    assert np.array_equal(a, 2.0 ** np.round(np.log2(a))) and len(set(a.tolist())) > 1, a
    assert R.tiled_conv(w, cs.attrs)
    a4 = a.reshape(-1, 1, 1, 1)
    for prec in ("bf16", "f16"):
        folded_then_rounded = R.round_operand((w[:meta["nb"]].astype(np.float64) * a4).astype(np.float32), prec)
        rounded_then_folded = (R.round_operand(w[:meta["nb"]], prec).astype(np.float64) * a4).astype(np.float32)
        assert np.array_equal(folded_then_rounded, rounded_then_folded), (name, prec)


def test_earlier_cases_build_as_before():
    """build()'s reference operands and further graph outputs leave the models
    and feeds of the cases without them as they were: a chain with fresh
    inputs, one with constants, a `post` pair and a multi-output case, each
    alone in its model (sha256 of the model's bytes, then of the feeds' names
    and bytes in name order, taken before the ir family was added)."""
    import hashlib
    for name, want in (("Conv_dwpw_3x3_s2_C32_M20", "bdf7b536833092ee"), ("Conv_small_K27_relu", "cbaf9f1e75aa4dcd"),
                       ("Conv_dwpw_7x7_C24_M20", "2aa72bb97bd375b2"), ("ConvPRelu_C11", "d9024db3b3f5c686"),
                       ("Split_sizes_input", "af60f2da80681bf2")):
        data, feeds, _ = OC.build([OC.BY_NAME[name]])
        h = hashlib.sha256(data)
        for k in sorted(feeds):
            h.update(k.encode())
            h.update(feeds[k].tobytes())
        assert h.hexdigest()[:16] == want, name
