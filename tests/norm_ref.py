"""What the InstanceNorm kernels and the IBNorm fusion compute, restated in
numpy float32 (test infrastructure; vso_kernels.hip: k_norm_plane,
k_norm_stats, k_norm_apply, merge_stats, k_conv_thin; vso_plan.hip:
plan_norm, find_ibnorm, plan_conv's BatchNorm fold), for the inorm / ibn
families of the operator matrix (tests/op_cases.py):

  plane   two passes over the plane: mean = sum / n, M2 = sum (x - mean)^2
  pair    (mean, M2, n) per piece of 4096 elements, each by two passes; the
          pieces merged in order (k_norm_apply) or, before a thin head, by 64
          lanes folding pieces lane, lane + 64, ... and a butterfly over the
          lanes (merge_stats) — Chan et al.'s update, every operation float32
  apply   (x - mean) * (scale / sqrt(M2 / n + eps)) + B, then the Relu
  fold    a = scale / sqrt(var + eps) in double; w' = float32(w * a),
          b' = float32((b - mean) * a + B) on the first nb output channels,
          the Relu on those in the conv, on the others in the norm

Sums within a piece are numpy's float32 sums (the kernels' lane / wave order
is another association of the same additions); convolutions accumulate in
float64 and round once (the conv kernels have their own families).  Every
function takes `mutant`: one way the kernels could be wrong (MUTANTS), for
tests/test_op_matrix_oracle.py to show that the cases' inputs tell it from
the right arithmetic.
"""
import numpy as np

F = np.float32
CHUNK = 4096
PLANE_MAX = 36864
MUTANTS = ("cnt_m1", "last_full", "no_between", "drop64", "one_pass", "no_eps", "bn_no_eps", "c0_zero", "ctot_M",
           "stats_img0", "relu_all", "no_relu_norm")


# ---- statistics ---------------------------------------------------------------
def two_pass(v, mutant=None, n=None):
    """(mean, M2, count) of a float32 vector; n: the count the kernel believes."""
    n = F(v.size if n is None else n)
    mean = v.sum(dtype=F) / n
    if mutant == "one_pass":
        return mean, (v * v).sum(dtype=F) - n * mean * mean, n
    d = v - mean
    return mean, (d * d).sum(dtype=F), n


def pieces(v, mutant=None):
    out = []
    for b in range(0, v.size, CHUNK):
        part = v[b:b + CHUNK]
        out.append(two_pass(part, mutant, CHUNK if mutant == "last_full" else None))
    return out


def fold(a, b, mutant=None):
    """Chan et al.: piece b merged into a."""
    (mean, m2, cnt), (mb, m2b, nb) = a, b
    if nb == 0:
        return a
    nab, d = F(cnt + nb), F(mb - mean)
    mean = F(mean + d * F(nb / nab))
    between = F(0) if mutant == "no_between" else F(d * d * F(F(cnt * nb) / nab))
    return mean, F(m2 + F(m2b + between)), nab


def merge_seq(ps, mutant=None):
    acc = ps[0]
    for p in ps[1:]:
        acc = fold(acc, p, mutant)
    return acc


def merge_wave(ps, mutant=None):
    zero = (F(0), F(0), F(0))
    lanes = []
    for lane in range(64):
        acc = zero
        for k in range(lane, len(ps), 64):
            if mutant == "drop64" and k >= 64:
                break
            acc = fold(acc, ps[k], mutant)
        lanes.append(acc)
    o = 1
    while o < 64:  # (both partners: the lower lane's partial first)
        lanes = [fold(lanes[lane & ~o], lanes[lane | o], mutant) for lane in range(64)]
        o <<= 1
    assert all(t == lanes[0] for t in lanes)
    return lanes[0]


def form_of(inner, defer=False, plane=True):
    return "wave" if defer else "plane" if plane and inner <= PLANE_MAX else "seq"


def stats(v, form, mutant=None):
    if form == "plane":
        return two_pass(v, mutant)
    return (merge_wave if form == "wave" else merge_seq)(pieces(v, mutant), mutant)


def coeffs(st, scale, shift, eps, mutant=None):
    """(mean, sc, sf) of the apply step."""
    mean, m2, cnt = st
    with np.errstate(divide="ignore", invalid="ignore"):
        var = m2 / (F(cnt - 1) if mutant == "cnt_m1" else cnt)
        return mean, F(scale) / np.sqrt(F(var + (F(0) if mutant == "no_eps" else F(eps))), dtype=F), F(shift)


def apply(v, co, relu):
    mean, sc, sf = co
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v - mean) * sc + sf
    return np.maximum(y, F(0)) if relu else y


def norm_rows(buf, n_img, c_cnt, c0, ctot, inner, scale, shift, eps, form, relu, mutant=None, stats_only=False):
    """The norm kernels on a flat float32 buffer: planes (n, c0 + c) of an [n_img][ctot][inner] tensor, in
    place.  Returns the apply step's coefficients per (n, c) (stats_only: the buffer is left as it is)."""
    out = {}
    for n in range(n_img):
        for c in range(c_cnt):
            off = (n * ctot + c0 + c) * inner
            v = buf[off:off + inner]
            out[n, c] = coeffs(stats(v, form, mutant), scale[c], shift[c], eps, mutant)
    for n in range(n_img):
        for c in range(c_cnt):
            co = out[0 if mutant == "stats_img0" else n, c]
            out[n, c] = co
            if not stats_only:
                off = (n * ctot + c0 + c) * inner
                buf[off:off + inner] = apply(buf[off:off + inner], co, relu)
    return out


def inorm(x, scale, shift, eps, mutant=None, plane=True):
    """InstanceNormalization of [N, C, ...] alone."""
    n, c = x.shape[:2]
    inner = int(np.prod(x.shape[2:]))
    buf = np.ascontiguousarray(x, F).reshape(-1).copy()
    norm_rows(buf, n, c, 0, c, inner, scale, shift, eps, form_of(inner, plane=plane), False, mutant)
    return buf.reshape(x.shape)


# ---- convolutions (float64 accumulation, one rounding) --------------------------
def conv(x, w, b, attrs):
    import torch
    import torch.nn.functional as tf
    pads = attrs.get("pads", [0, 0, 0, 0])
    xt = tf.pad(torch.from_numpy(np.ascontiguousarray(x)).double(), (pads[1], pads[3], pads[0], pads[2]))
    y = tf.conv2d(xt, torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(),
                  stride=tuple(attrs.get("strides", [1, 1])), groups=attrs.get("group", 1))
    return y.numpy().astype(F)


# ---- the fused IBNorm -----------------------------------------------------------
def ibn_core(x, w, b, attrs, bn, eps_bn, inn, eps_in, nb, relu, form, mutant=None, cat=None, skip=None):
    """The conv with the BatchNorm folded in and the norm in place: (the tensor the conv and the norm wrote —
    the pattern's [N, M, H, W], or the later Concat's [N, ctot, H, W] —, the norm's coefficients, applied
    unless form is "wave": then the consumer applies them)."""
    sc, bb, mu, var = (t.astype(np.float64) for t in bn)
    m = w.shape[0]
    a = sc / np.sqrt(var + (0.0 if mutant == "bn_no_eps" else float(F(eps_bn))))
    wf, bias = w.copy(), (np.zeros(m, F) if b is None else b.copy())
    wf[:nb] = (w[:nb].astype(np.float64) * a.reshape(-1, 1, 1, 1)).astype(F)
    bias[:nb] = ((bias[:nb].astype(np.float64) - mu) * a + bb).astype(F)
    y = conv(x, wf, bias, attrs)
    relu_conv = relu or mutant == "relu_all"
    if relu_conv:
        y[:, :nb] = np.maximum(y[:, :nb], F(0))
    n_img, _, h, wd = y.shape
    inner = h * wd
    if cat is None:
        full, doff, ctot = y, 0, m
    else:  # the conv writes into the later Concat's output: the pattern first (cat[0] == 0) or second
        full = np.concatenate([y, skip] if cat[0] == 0 else [skip, y], axis=1)
        doff, ctot = (0 if cat[0] == 0 else skip.shape[1]), m + skip.shape[1]
    buf = np.ascontiguousarray(full, F).reshape(-1).copy()
    base = buf[doff * inner:]  # (the norm's x = y = the concatenation's base + the pattern's offset)
    relu_norm = relu_conv and mutant != "no_relu_norm"
    co = norm_rows(base, n_img, m - nb, 0 if mutant == "c0_zero" else nb, m if mutant == "ctot_M" else ctot, inner,
                   inn[0], inn[1], float(F(eps_in)), form, relu_norm, mutant, stats_only=form == "wave")
    return buf.reshape(full.shape), co, relu_norm


def thin_head(y, co, relu, c0, w, b, attrs, mutant=None):
    """k_conv_thin behind a deferred norm: channels c0 .. normalised in the loads, then the 1x1."""
    v = y.copy()
    for (n, c), k in co.items():
        ch = c if mutant == "c0_zero" else c0 + c
        v[n, ch] = apply(v[n, ch], k, relu)
    return conv(v, w, b, attrs)


def run_ibn(cs, meta, ops, chain_ops, mutant=None, plane=True, thin=True, keep=None):
    """The outputs of a fused ibn case (tests/op_cases.py, IBN: its figures), as the session computes them;
    plane / thin: False under VSO_NORM_PLANE=0 / VSO_THIN=0; keep: a dict that receives "normalised"."""
    x, w = ops[0], ops[1]
    b = ops[2] if len(ops) > 2 else None
    i_bn, pos, nb = meta["i_bn"], meta["pos"], meta["nb"]
    bn_nd, in_nd = cs.chain[i_bn - 1], cs.chain[i_bn]
    bn, inn = chain_ops[i_bn - 1][1:5], chain_ops[i_bn][1:3]
    inner = int(np.prod(x.shape[2:]))  # (every pattern's conv keeps the plane)
    cat, skip = meta["cat"], None
    if cat is not None:
        skip = [v for v in chain_ops[pos] if not isinstance(v, tuple)][0]
    tail = list(zip(cs.chain, chain_ops))[pos + (cat is not None):]
    # a head that is a second pattern's conv (IBN_head_ibn_63): found thin, declined — flush_norm launches
    # k_norm_apply on the statistics' pieces
    flush = len(tail) > 1
    defer = meta["defer"] and thin and not flush
    form = "seq" if meta["defer"] and thin and flush else form_of(inner, defer, plane)
    y, co, relu_norm = ibn_core(x, w, b, cs.attrs, bn, bn_nd[2].get("epsilon", 1e-5), inn, in_nd[2].get("epsilon", 1e-5),
                                nb, meta["relu"], form, mutant, cat, skip)
    if keep is not None:  # the normalised channels as the consumer sees them
        v = y[:, (0 if cat is None or cat[0] == 0 else skip.shape[1]):][:, nb:meta["m"]].copy()
        for (n, c), k in (co.items() if defer else ()):
            v[n, c] = apply(v[n, c], k, relu_norm)
        keep["normalised"] = v
    outs = [y] if meta["out"] else []
    if not tail:
        return outs + [y]
    (_, _, at_), more = tail[0][0][:3], tail[0][1]
    hw, hb = more[0], more[1] if len(more) > 1 else None
    if flush:  # Slice, Slice, BatchNormalization, InstanceNormalization, Concat behind the head's conv
        assert [t[0][0] for t in tail[1:]] == ["Slice", "Slice", "BatchNormalization", "InstanceNormalization", "Concat"]
        nb2 = int(tail[3][1][1].size)
        return outs + [ibn_core(y, hw, hb, at_, tail[3][1][1:5], tail[3][0][2].get("epsilon", 1e-5), tail[4][1][1:3],
                                tail[4][0][2].get("epsilon", 1e-5), nb2, False, form_of(inner, False, plane), mutant)[0]]
    return outs + [thin_head(y, co, relu_norm, nb, hw, hb, at_, mutant) if defer else conv(y, hw, hb, at_)]


# ---- the generic plan (the near misses) and a walker over a case's nodes -----------
def walk(cs, ops, chain_ops, ev):
    """The case's graph outputs, its nodes evaluated by ev(op, inputs, attrs, opset) -> array (tuple: several
    outputs), the references of tests/op_cases.py resolved here."""
    def first(v):
        return v[0] if isinstance(v, tuple) else v

    made = [ev(cs.op, list(ops), cs.attrs, cs.opset)]
    outs = [first(made[0])] if cs.op_out else []
    for k, (nd, more) in enumerate(zip(cs.chain, chain_ops)):
        opts = nd[3] if len(nd) > 3 else {}

        def ref(v):
            if not isinstance(v, tuple):
                return v
            if v[0] == "prev":
                return first(made[-1])
            if v[0] == "in":
                return ops[v[1]]
            return made[v[1]][v[2]] if len(v) > 2 else first(made[v[1]])
        ins = [ref(v) for v in more]
        made.append(ev(nd[0], ins if opts.get("whole") else [first(made[-1])] + ins, nd[2], cs.opset))
        if opts.get("out") and k + 1 < len(cs.chain):
            outs.append(first(made[-1]))
    return ([ops[0]] if cs.echo else []) + outs + [first(made[-1])]


def onnx_slice(x, ins, attrs):
    """ONNX Slice by its definition (inputs from opset 10 on, attributes before)."""
    if len(ins) > 1:
        starts, ends = ins[1], ins[2]
        axes = ins[3] if len(ins) > 3 and ins[3] is not None else None
        steps = ins[4] if len(ins) > 4 and ins[4] is not None else None
    else:
        starts, ends, axes, steps = attrs["starts"], attrs["ends"], attrs.get("axes"), None
    axes = list(range(len(starts))) if axes is None else axes
    steps = [1] * len(starts) if steps is None else steps
    for b, e, ax, st in zip(starts, ends, axes, steps):
        ax, b, e, st = int(ax) % x.ndim, int(b), int(e), int(st)
        assert st > 0
        n = x.shape[ax]
        b, e = min(max(b + n if b < 0 else b, 0), n), min(max(e + n if e < 0 else e, 0), n)
        x = np.take(x, np.arange(b, e, st), axis=ax)
    return x


def ev32(plane=True):
    """The generic plan's nodes in float32: a launch each."""
    def ev(op, ins, at, opset):
        x = ins[0]
        if op == "Conv":
            return conv(x, ins[1], ins[2] if len(ins) > 2 else None, at)
        if op == "InstanceNormalization":
            return inorm(x, ins[1], ins[2], float(F(at.get("epsilon", 1e-5))), plane=plane)
        if op == "BatchNormalization":  # k_affine: x * scale + shift, the two worked out in double
            a = ins[1].astype(np.float64) / np.sqrt(ins[4].astype(np.float64) + float(F(at.get("epsilon", 1e-5))))
            sh = (1, -1) + (1,) * (x.ndim - 2)
            return x * a.astype(F).reshape(sh) + (ins[2] - ins[3] * a).astype(F).reshape(sh)
        if op == "Slice":
            return onnx_slice(x, ins, at)
        if op == "Split":
            return tuple(np.split(x, np.cumsum([int(v) for v in ins[1]])[:-1], axis=at["axis"]))
        if op == "Concat":
            return np.concatenate(ins, axis=at["axis"])
        assert op == "Relu", op
        return np.maximum(x, F(0))
    return ev
