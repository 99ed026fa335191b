"""The arithmetic of the fused inverted-residual kernels (csrc/vso_ir.hip),
restated in numpy for the cases of the operator matrix's `ir` family
(tests/op_cases.py): what k_ir and k_ir_b16 compute, operation by operation in
their number formats, without their tiling.

  f32 (k_ir):      every product and sum in float32.  The expand starts from
                   its bias and adds the input channels in order; the
                   depthwise starts from its bias and adds the taps in (ky,
                   kx) order over a hidden tensor that is 0 outside the image;
                   the project adds the hidden channels in order from 0, then
                   its bias, then the residual.
  b16 (k_ir_b16):  both operands of each 1x1 split hi = bf16(v), lo = bf16(v -
                   hi); per channel the three products wl xh + wh xl + wh xh
                   (exact in float32) are added to a float32 sum.  The
                   depthwise as in f32.

The kernels add in another association (MFMA steps of 4 / 32 channels, slices
summed by k_ir_reduce) and fuse the depthwise's multiply-adds: differences of
a few float32 roundings, far below the matrix's bar.  tests/
test_op_matrix_oracle.py holds this restatement to half the bar against the
f64 oracle on every fused case, and checks that each mutant below — a way the
kernels could be wrong — leaves the bar on a case made for it.

Mutants: "drop_wl_xh" (the project's wl xh product missing, b16),
"pad_clip" (the depthwise's padding taken as clip(0), not 0), "swap_taps"
(the depthwise's first two taps exchanged), "no_res" (the residual missing),
"drop_last_chunk" (the project without the last 16 hidden channels),
"cout_tail" (the last COUT % 16 output channels from the weight row before),
"cin_tail" (f32: the channels past CIN up to the next multiple of 16 not
zero-filled — channel CIN - 1 against the last four weights read again).
"""
import numpy as np

from seam_ref import bf16_round

F = np.float32


def split(v):
    """(hi, lo) bf16 parts of a float32 array, as float32."""
    v = np.asarray(v, F)
    hi = bf16_round(v).astype(F)
    return hi, bf16_round(v - hi).astype(F)


def pointwise(x, w, b, form, bias_first, mutant=None):
    """A 1x1 convolution [N, C, H, W] -> [N, M, H, W] in the form's arithmetic."""
    n, cin, h, wd = x.shape
    m = w.shape[0]
    w = np.asarray(w, F).reshape(m, cin)
    xs = x.reshape(n, 1, cin, h * wd)
    bias = np.zeros(m, F) if b is None else np.asarray(b, F)
    if mutant == "cout_tail" and m % 16:
        w = w.copy()
        w[m - m % 16:] = w[m - m % 16 - 1:m - 1]
    k_end = cin - 16 if mutant == "drop_last_chunk" else cin
    acc = np.zeros((n, m, h * wd), F)
    if bias_first:
        acc += bias[None, :, None]
    if form == "f32":
        for k in range(k_end):
            acc += w[None, :, k, None] * xs[:, :, k]
        if mutant == "cin_tail":
            for k in range(cin, -(-cin // 16) * 16):
                acc += w[None, :, cin - 4 + k % 4, None] * xs[:, :, cin - 1]
    else:
        (wh, wl), (xh, xl) = split(w), split(xs)
        for k in range(k_end):
            if mutant != "drop_wl_xh":
                acc += wl[None, :, k, None] * xh[:, :, k]
            acc += wh[None, :, k, None] * xl[:, :, k]
            acc += wh[None, :, k, None] * xh[:, :, k]
    if not bias_first:
        acc += bias[None, :, None]
    return acc.reshape(n, m, h, wd)


def depthwise3(x, w, b, stride, pad_value=0.0, mutant=None):
    """A 3x3 depthwise convolution, pads 1, in float32: the bias, then the taps in (ky, kx) order."""
    n, ch, h, wd = x.shape
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    w = np.asarray(w, F).reshape(ch, 9).copy()
    if mutant == "swap_taps":
        w[:, [0, 1]] = w[:, [1, 0]]
    xp = np.pad(np.asarray(x, F), ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=F(pad_value))
    acc = np.zeros((n, ch, ho, wo), F) + (np.zeros(ch, F) if b is None else np.asarray(b, F))[None, :, None, None]
    for ky in range(3):
        for kx in range(3):
            acc += w[None, :, 3 * ky + kx, None, None] * xp[:, :, ky:ky + stride * (ho - 1) + 1:stride,
                                                            kx:kx + stride * (wo - 1) + 1:stride]
    return acc


def run(cs, ops, chain_ops, form, mutant=None):
    """(the case's outputs in op_cases.build()'s order, [(a Clip's input, lo, hi)])
    of a fused case: its blocks in `form`'s arithmetic, every other node
    (the Adds) in float32.  `mutant` applies to the case's first block."""
    made, outs, clips = [], [], []
    x0 = np.asarray(ops[0], F)
    last_clip = (None, None)

    def ref(v):
        if isinstance(v, tuple):
            return made[-1] if v[0] == "prev" else x0 if v[0] == "in" else made[v[1]]
        return v

    nodes = [(cs.op, list(ops[1:]), cs.attrs, {"first": True})] + \
            [(nd[0], more, nd[2], nd[3] if len(nd) > 3 else {}) for nd, more in zip(cs.chain, chain_ops)]
    convs = 0
    for op_, more, at_, opts in nodes:
        ins = [ref(v) for v in more]
        if opts.get("first"):
            ins = [x0] + ins
        elif not opts.get("whole"):
            ins = [made[-1]] + ins
        mu = mutant if convs < 3 or (op_ == "Add" and convs == 3) else None
        if op_ == "Conv":
            w, b = ins[1], ins[2] if len(ins) > 2 else None
            if convs % 3 == 1:
                assert w.shape[1:] == (1, 3, 3) and at_.get("pads") == [1, 1, 1, 1], cs.name
                lo, hi = last_clip
                pad = float(np.clip(0.0, -np.inf if lo is None else lo, np.inf if hi is None else hi)) \
                    if mu == "pad_clip" else 0.0
                y = depthwise3(ins[0], w, b, at_.get("strides", [1, 1])[0], pad, mu)
            else:
                assert w.shape[2:] == (1, 1), cs.name
                expand = convs % 3 == 0
                skip = ("drop_last_chunk", "cout_tail", "drop_wl_xh") if expand else ("cin_tail",)
                y = pointwise(ins[0], w, b, form, expand, None if mu in skip else mu)
            convs += 1
        elif op_ == "Clip":
            lo = at_.get("min") if len(ins) < 2 or ins[1] is None else float(ins[1])
            hi = at_.get("max") if len(ins) < 3 or ins[2] is None else float(ins[2])
            clips.append((ins[0], lo, hi))
            last_clip = (lo, hi)
            y = ins[0] if lo is None and hi is None else np.clip(ins[0], lo, hi).astype(F)
        else:
            assert op_ == "Add", (cs.name, op_)
            res = (ins[0] is x0) != (ins[1] is x0)
            y = (ins[1] if ins[0] is x0 else ins[0]) if mu == "no_res" and res else ins[0] + ins[1]
        made.append(y)
        if opts.get("out"):
            outs.append(y)
    return ([x0] if cs.echo else []) + outs + [made[-1]], clips
