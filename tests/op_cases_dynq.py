"""The operator matrix of the dynamically quantised graphs (test
infrastructure), the form onnxruntime's quantize_dynamic writes:
DynamicQuantizeLinear (k_dyn_minmax + k_dyn_quantize), ConvInteger and
MatMulInteger (k_iconv_tile on the int8 MFMA, k_iconv_direct), the Cast of
their int32 output (k_cast_i32), and the chain a session fuses into the
integer launch's float epilogue,

    ConvInteger | MatMulInteger -> Cast -> Mul(., Mul(x_scale, w_scale)) [-> Add(bias)] [-> Relu | Clip].

Shared by tests/test_dynq_ref.py (the reference tests/onnx_ref_dynq.py against
PyTorch and the kernels' four-term identity, and this table's own conditions,
CPU) and tests/test_gpu_dynq_matrix.py (the GPU sessions against the
reference).  A case is a function adding its nodes to a family's model; build()
packs a family into one model, one graph output per case output.  `kernels`
names a case's launches in order, `unfused` those of the plan without the fused
epilogue (VSO_DYNQ=0).  Batch 2 unless a case says otherwise.

How an output is held (`outs`: graph output -> rule):
  "exact"  equal to the reference, every element and the dtype.  All of
           DynamicQuantizeLinear (the operator is float32 arithmetic, which the
           reference states step by step), every integer result (cast to float:
           the cases keep |acc| < 2^24) and every chain in the dyadic weighting:
           w_scale a power of two, the input's range planted at 255 * 2^-k so
           that x_scale = 2^-k, the bias a multiple of their product.
  a dict   a chain in the general weighting (seeded arbitrary scales): within
           4 * 2^-24 * (|acc| s + |bias|) of the float64 value act(acc * s + bias),
           s = x_scale * w_scale in float64 — one rounding each for the
           conversion (above 2^24 only), s, the product and the sum.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

import onnx_models as M
import onnx_ref as R

MINMAX, DYNQ, TILE, DIRECT, CAST = "k_dyn_minmax(", "k_dyn_quantize(", "k_iconv_tile(", "k_iconv_direct(", "k_cast_i32("
DQ, BINARY, UNARY = "k_dequantize(", "k_binary", "k_unary("
FORMS = (MINMAX, DYNQ, TILE, DIRECT, CAST)
U8, S8, F32 = np.uint8, np.int8, np.float32
ACC_MAX = 2 ** 24


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@dataclass
class Built:
    """What a case added to its family's model."""
    feeds: dict = field(default_factory=dict)     # graph input -> float32 array
    outs: dict = field(default_factory=dict)      # graph output -> "exact" | the general bound's ingredients
    kernels: tuple = ()
    unfused: tuple = ()
    fused: int = 0
    acc: tuple = ()                               # the int32 values of the case (reference names), for the CPU conditions
    expect_zp: dict = field(default_factory=dict)  # zero point output -> the value the case is built to give
    expect_scale: dict = field(default_factory=dict)


@dataclass
class Case:
    name: str
    family: str
    fn: object            # (Builder, Built) -> None
    expect: str = "value"  # or "refused"
    op: str = ""          # refused: the operator the message names


CASES: list[Case] = []


def case(name, family, fn, **kw):
    assert all(k.name != name for k in CASES), name
    CASES.append(Case(name, family, fn, **kw))


def build(cases):
    """(model bytes, feeds, {case: Built}) of one model holding `cases`."""
    b = M.Builder(0)
    built, feeds, outs = {}, {}, []
    for cs in cases:
        bt = Built()
        cs.fn(b, bt)
        built[cs.name] = bt
        feeds.update(bt.feeds)
        outs += [(o, []) for o in bt.outs]
    return b.model([(n, list(a.shape)) for n, a in feeds.items()], outs, opset=13), feeds, built


# ---- inputs --------------------------------------------------------------------------------
ZP_LO = {0: 0, 255: -255, "mid": -100}  # the range's lower end in steps, by the zero point it gives


def x_planted(name, shape, zp=0, dyadic=True, k=4, ties=False):
    """A float32 input whose range is planted: [lo, lo + 255] steps of 2^-k (dyadic: integer multiples of the step,
    or of half of it with `ties`, so x_scale is exactly 2^-k) or of 1.37 * 2^-k with arbitrary values between; both
    ends present, so the zero point is -lo."""
    r = _rng(name + "/x")
    lo = ZP_LO[zp]
    n = int(np.prod(shape))
    if dyadic:
        v = r.integers(lo, lo + 256, size=n).astype(np.float64)
        if ties:
            v = np.minimum(v + np.where(r.random(n) < 0.3, 0.5, 0.0), lo + 255)
        step = 2.0 ** -k
    else:
        v = r.uniform(lo, lo + 255, size=n)
        step = 1.37 * 2.0 ** -k
    if n >= 2:
        i, j = r.choice(n, size=2, replace=False)
        v[i], v[j] = lo, lo + 255
    return (v * step).astype(F32).reshape(shape)


def dynq(b, x):
    """DynamicQuantizeLinear(x): (y, y_scale, y_zero_point)."""
    return b.op("DynamicQuantizeLinear", [x], n_out=3)


def w_ints(name, shape, wt, zw, wmax, per=None):
    """Quantised weights of type `wt` with |Wq - zw| <= wmax.  zw: one value, or a list per channel along axis `per`."""
    r = _rng(name + "/w")
    lo, hi = (0, 255) if wt is U8 else (-128, 127)
    z = np.asarray(zw, np.int64)
    zb = z.reshape([-1 if d == per else 1 for d in range(len(shape))]) if z.ndim else z
    return np.clip(r.integers(-wmax, wmax + 1, size=shape) + zb, lo, hi).astype(wt), z.astype(wt)


def wmax_for(K):
    return int(max(1, min(255, (ACC_MAX - 1) // (255 * K))))


# ---- DynamicQuantizeLinear alone -----------------------------------------------------------
F_DQL = "dql"


def dql_case(name, shape, pattern):
    def fn(b, bt):
        r = _rng(name)
        n = int(np.prod(shape))
        if pattern == "zero":
            x = np.zeros(shape)
        elif pattern == "pos":
            x = r.uniform(0.3, 9.7, size=shape)
        elif pattern == "neg":
            x = -r.uniform(0.3, 9.7, size=shape)
        elif pattern == "mixed":
            x = r.standard_normal(shape) * 3.7
        elif pattern == "ties":
            x = x_planted(name, shape, "mid", True, k=5, ties=True)
        else:  # the extremes planted: at the first and the last element, or in the second image only
            x = r.uniform(-1.0, 1.0, size=shape)
            flat = x.reshape(-1)
            if pattern == "ends":
                flat[0], flat[-1] = 7.3, -4.9
            else:
                flat[n // 2 + 3], flat[n - 2] = -7.3, 4.9
        inp = f"{name}_x"
        bt.feeds[inp] = np.asarray(x, F32).reshape(shape)
        y, sc, zp = dynq(b, inp)
        bt.outs.update({y: "exact", sc: "exact", zp: "exact"})
        bt.kernels = bt.unfused = (MINMAX, DYNQ, DQ, DQ)
    case(name, F_DQL, fn)


for tag_, shape_ in (("n1", (1,)), ("n255", (255,)), ("n256", (256,)), ("2x5x70x100", (2, 5, 70, 100))):
    for pat_ in ("zero", "pos", "neg", "mixed", "ties", "ends", "second_image"):
        if (shape_ == (1,) and pat_ in ("ties", "ends", "second_image")) or (pat_ == "second_image" and len(shape_) == 1):
            continue
        dql_case(f"dql_{tag_}_{pat_}", shape_, pat_)


# ---- ConvInteger / MatMulInteger and what follows ---------------------------------------------
def integer_node(b, bt, name, kind, xs, wshape, wt=S8, zw=0, per_channel=False, zx="mid", attrs=None, dyadic=True,
                 xq=None, w_const=True):
    """DynamicQuantizeLinear(x) -> ConvInteger | MatMulInteger: (the int32 value, y_scale, y_zero_point, M, y)."""
    conv = kind == "conv"
    M_ = wshape[0] if conv else wshape[1]
    K = int(np.prod(wshape[1:])) if conv else wshape[0]
    if per_channel:
        zw = [(int(zw) + 37 * m) % 256 for m in range(M_)] if wt is U8 else [(int(zw) + 5 * m) % 64 - 32 for m in range(M_)]
    wq, zwc = w_ints(name, wshape, wt, zw, wmax_for(K), per=(0 if conv else 1))
    if xq is None:
        inp = f"{name}_x"
        bt.feeds[inp] = x_planted(name, xs, zx, dyadic)
        xq = dynq(b, inp)
        bt.expect_zp[xq[2]] = -ZP_LO[zx]
        if dyadic:
            bt.expect_scale[xq[1]] = 2.0 ** -4
    y, sc, zp = xq
    ins = [y, b.const(wq), zp] + ([] if (wt is S8 and not per_channel and zw == 0) else [b.const(zwc)])
    acc = b.op("ConvInteger" if conv else "MatMulInteger", ins, **(attrs or {}))
    bt.acc += (acc,)
    return acc, sc, zp, M_, y


def plain_case(name, family, kernel, kind, xs, wshape, **kw):
    """... -> Cast: the integers, exact."""
    def fn(b, bt):
        acc, _, _, _, _ = integer_node(b, bt, name, kind, xs, wshape, **kw)
        bt.outs[b.op("Cast", [acc], to=R.DT_FLOAT)] = "exact"
        bt.kernels = bt.unfused = (MINMAX, DYNQ, kernel, CAST)
    case(name, family, fn)


F_ICONV, F_IMM = "iconv", "imm"
P1 = {"pads": [1, 1, 1, 1]}


def iconv(name, cin, cout, k, hw, kernel=TILE, group=1, attrs=None, **kw):
    at = {"kernel_shape": list(k), "group": group}
    at.update(attrs or {})
    plain_case(f"ci_{name}", F_ICONV, kernel, "conv", (2, cin) + tuple(hw), (cout, cin // group) + tuple(k), attrs=at, **kw)


# k_iconv_tile: M on both sides of 64, K = C kh kw on both sides of 64 and its multiples, pixels no multiple of 64
iconv("3x3_3to5_K27", 3, 5, (3, 3), (9, 11), attrs=P1, zx="mid")
iconv("1x1_64to64_K64", 64, 64, (1, 1), (5, 7), zx=0)
iconv("7x7_3to70_K147", 3, 70, (7, 7), (12, 13), attrs={"pads": [3, 3, 3, 3]}, zx=255, wt=U8, zw=128)
iconv("5x5_8to5_K200", 8, 5, (5, 5), (9, 11), attrs={"pads": [2, 2, 2, 2]}, zx="mid", wt=U8, zw=37)
iconv("3x3_s2_16to64", 16, 64, (3, 3), (17, 33), attrs={"pads": [1, 1, 1, 1], "strides": [2, 2]}, zx="mid", wt=U8, zw=200)
iconv("3x3_d2_16to8", 16, 8, (3, 3), (12, 13), attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}, zx=255, wt=U8, zw=200)
iconv("3x3_8to70_per_channel", 8, 70, (3, 3), (9, 11), attrs=P1, zx="mid", wt=U8, zw=3, per_channel=True)
iconv("1x1_20to5_per_channel_s8", 20, 5, (1, 1), (5, 7), zx=0, wt=S8, zw=0, per_channel=True)
iconv("3x2_asym_pads_5to5", 5, 5, (3, 2), (9, 11), attrs={"pads": [0, 1, 2, 0]}, zx=255)
iconv("same_upper_s2_3to5", 3, 5, (3, 3), (12, 13), attrs={"auto_pad": "SAME_UPPER", "strides": [2, 2]}, zx="mid", wt=U8, zw=128)
# the threshold between the kernels: K = 2^15 - 1 on the MFMA, 2^15 on the VALU
iconv("1x1_K32767", 32767, 2, (1, 1), (2, 2), zx="mid", wt=U8, zw=128)
iconv("1x1_K32768_direct", 32768, 2, (1, 1), (2, 2), kernel=DIRECT, zx="mid", wt=U8, zw=128)
# k_iconv_direct: depthwise, grouped, a 9x1 window
iconv("dw3x3_C5", 5, 5, (3, 3), (12, 13), kernel=DIRECT, group=5, attrs=P1, zx="mid", wt=U8, zw=128)
iconv("dw3x3_s2_C32_per_channel", 32, 32, (3, 3), (17, 33), kernel=DIRECT, group=32,
      attrs={"pads": [1, 1, 1, 1], "strides": [2, 2]}, zx=255, wt=U8, zw=11, per_channel=True)
iconv("g2_3x3_8to6", 8, 6, (3, 3), (9, 11), kernel=DIRECT, group=2, attrs=P1, zx=0, wt=U8, zw=200)
iconv("dw9x1_C5", 5, 5, (9, 1), (12, 13), kernel=DIRECT, group=5, attrs={"pads": [4, 0, 4, 0]}, zx="mid")

# the lane map: a 1x1 convolution over 64 channels by an asymmetric integer matrix, every weight and every pixel
# distinct in what it selects — the input is one-hot per pixel in channel (p + 7 n) mod 64 at the top of the range
# (x_scale 1, zero point 0: xq = 255 there, 0 elsewhere), so the output at (m, p) is 255 W[m][that channel]
LANE_MAP = "ci_lane_map_1x1_64to40"


def _lane_w():
    m, k = np.meshgrid(np.arange(40), np.arange(64), indexing="ij")
    return ((3 * m + 5 * k) % 11 - 5).astype(S8).reshape(40, 64, 1, 1)


def _lane_case(b, bt):
    n, ch, h, w = 2, 64, 12, 13
    p = np.arange(h * w)
    a = np.zeros((n, ch, h * w), F32)
    for i in range(n):
        a[i, (p + 7 * i) % ch, p] = 255.0
    bt.feeds["lane_x"] = a.reshape(n, ch, h, w)
    y, sc, zp = dynq(b, "lane_x")
    bt.expect_zp[zp], bt.expect_scale[sc] = 0, 1.0
    acc = b.op("ConvInteger", [y, b.const(_lane_w()), zp], kernel_shape=[1, 1])
    bt.acc += (acc,)
    bt.outs[b.op("Cast", [acc], to=R.DT_FLOAT)] = "exact"
    bt.kernels = bt.unfused = (MINMAX, DYNQ, TILE, CAST)


case(LANE_MAP, F_ICONV, _lane_case)


def imm(name, ashape, n_out, **kw):
    plain_case(f"mm_{name}", F_IMM, TILE, "matmul", ashape, (ashape[-1], n_out), **kw)


for K_, N_ in ((20, 3), (64, 64), (200, 100), (20, 100), (200, 3)):
    imm(f"2x33x{K_}_N{N_}", (2, 33, K_), N_, zx="mid", wt=U8, zw=128 if K_ != 64 else 37)
    imm(f"65x{K_}_N{N_}", (65, K_), N_, zx=255 if K_ == 20 else 0, wt=S8 if K_ == 200 else U8, zw=0 if K_ == 200 else 200)
imm("2x33x64_N100_per_column", (2, 33, 64), 100, zx="mid", wt=U8, zw=9, per_channel=True)
imm("65x200_N3_per_column_s8", (65, 200), 3, zx="mid", wt=S8, zw=0, per_channel=True)


# ---- the fused chain ---------------------------------------------------------------------------
def chain_tail(b, bt, name, acc, sc, M_, kind, dyadic, bias=True, act=None, per_channel=False, swap=False,
               ws_shape=None, miss=None, K=1):
    """Cast -> Mul(., s) [-> Add] [-> Relu | Clip] behind the int32 value `acc`; s = Mul(x_scale, w_scale).
    Returns (the output, its rule).  miss: the near misses (see the cases)."""
    r = _rng(name + "/tail")
    conv = kind == "conv"
    chan = ((1, M_, 1, 1) if conv else (M_,))
    n_ws = int(np.prod(ws_shape)) if ws_shape else M_  # (the near miss: a w_scale that is not one per channel)
    if dyadic:
        ws = 2.0 ** -(5 + np.arange(n_ws) % 3) if per_channel else np.asarray(2.0 ** -5)
    else:
        ws = 0.0041 * (1.0 + np.arange(n_ws) / 7.0) if per_channel else np.asarray(0.0041)
    ws = np.asarray(ws, F32).reshape(ws_shape or (chan if per_channel else ()))
    f = b.op("Cast", [acc], to=R.DT_FLOAT)
    if miss == "cast_read_twice":
        bt.outs[f] = "exact"
    wsn = b.const(ws)
    s = b.op("Mul", [wsn, sc] if swap else [sc, wsn])
    if miss == "s_read_elsewhere":
        bt.outs[s] = "exact"
    y = b.op("Mul", [s, f] if swap else [f, s])
    bv = None
    if bias:
        # dyadic: a multiple of its channel's quantum x_scale * w_scale[m] (x_scale = 2^-4): the sum is that quantum
        # times acc + an integer below 2^24, exact
        wsm = np.broadcast_to(ws.reshape(-1), (M_,)) if ws.size == M_ else np.full(M_, ws.reshape(-1)[0])
        bv = (r.integers(-40, 41, size=M_) * 2.0 ** -4 * wsm if dyadic else r.standard_normal(M_) * 0.3).astype(F32)
        if miss == "runtime_bias":
            bn = f"{name}_bias"
            bt.feeds[bn] = bv.reshape(chan)
        else:
            bn = b.const(bv.reshape(chan if not (conv and not swap) else (M_, 1, 1)))
        y = b.op("Add", [bn, y] if swap else [y, bn])
    lo = hi = None
    if act == "relu":
        y = b.op("Relu", [y])
        lo = 0.0
    elif act == "clip":
        # (bounds about the sums' spread: 74 steps of the input's, wmax / 1.7 of the weights')
        sd = float(np.mean(ws)) * 2.0 ** -4 * (K ** 0.5) * 74.0 * wmax_for(K) / 1.7
        lo, hi = float(F32(-0.25 * sd)), float(F32(0.75 * sd))
        y = b.op("Clip", [y, b.const(F32(lo)), b.const(F32(hi))])
    rule = "exact" if dyadic else {"acc": acc, "scale": sc, "ws": np.broadcast_to(ws.reshape(-1), (M_,)) if ws.size > 1 else
                                   np.full(M_, float(ws.reshape(-1)[0]), F32), "bias": bv, "lo": lo, "hi": hi,
                                   "axis": 1 if conv else -1}
    bt.outs[y] = rule
    n_bin = 2 + (1 if bias else 0)
    return (CAST,) + (BINARY,) * n_bin + ((UNARY,) if act else ())


def chain_case(name, family, kernel, kind, xs, wshape, dyadic=True, attrs=None, expose=False, miss=None, tail=None, **kw):
    tail = dict(tail or {})

    def fn(b, bt):
        K = int(np.prod(wshape[1:])) if kind == "conv" else wshape[0]
        acc, sc, zp, M_, y = integer_node(b, bt, name, kind, xs, wshape, attrs=attrs, dyadic=dyadic, **kw)
        pub = ()
        if expose:  # the quantised input, its scale and zero point as graph outputs too
            bt.outs.update({y: "exact", sc: "exact", zp: "exact"})
            pub = (DQ, DQ)
        rest = chain_tail(b, bt, name, acc, sc, M_, kind, dyadic, miss=miss, K=K, **tail)
        bt.unfused = (MINMAX, DYNQ) + pub + (kernel,) + rest
        bt.kernels = bt.unfused if miss else (MINMAX, DYNQ) + pub + (kernel,)
        bt.fused = 0 if miss else 1
    case(name, family, fn)


F_CHAIN, F_MISS = "chain", "miss"
for dy_ in (True, False):
    t_ = "dy" if dy_ else "gen"

    def cconv(name, cin, cout, k, hw, kernel=TILE, group=1, attrs=None, tail=None, **kw):
        at = {"kernel_shape": list(k), "group": group}
        at.update(attrs or {})
        chain_case(f"ch_{name}_{t_}", F_CHAIN, kernel, "conv", (2, cin) + tuple(hw), (cout, cin // group) + tuple(k), dy_,
                   attrs=at, tail=tail, **kw)

    def cmm(name, ashape, n_out, tail=None, **kw):
        chain_case(f"ch_{name}_{t_}", F_CHAIN, TILE, "matmul", ashape, (ashape[-1], n_out), dy_, tail=tail, **kw)

    cconv("3x3_3to8_bias_relu", 3, 8, (3, 3), (9, 11), attrs=P1, wt=U8, zw=128, tail=dict(act="relu"), expose=True)
    cconv("1x1_64to70_clip_per_channel", 64, 70, (1, 1), (5, 7), wt=U8, zw=128, tail=dict(act="clip", per_channel=True))
    cconv("3x3_s2_16to5_nobias", 16, 5, (3, 3), (17, 33), attrs={"pads": [1, 1, 1, 1], "strides": [2, 2]}, wt=U8, zw=200,
          zx=255, tail=dict(bias=False))
    cconv("5x5_8to5_swapped_relu", 8, 5, (5, 5), (9, 11), attrs={"pads": [2, 2, 2, 2]}, wt=U8, zw=3, per_channel=True,
          tail=dict(act="relu", swap=True, per_channel=True))
    cconv("3x3_3to8_nobias_clip_swapped", 3, 8, (3, 3), (9, 11), attrs=P1, tail=dict(bias=False, act="clip", swap=True))
    cconv("1x1_20to5_wscale_C11", 20, 5, (1, 1), (5, 7), wt=U8, zw=128, tail=dict(per_channel=True, ws_shape=(5, 1, 1)))
    cconv("dw3x3_C5_bias_clip", 5, 5, (3, 3), (12, 13), kernel=DIRECT, group=5, attrs=P1, wt=U8, zw=128,
          tail=dict(act="clip", per_channel=True))
    cconv("dw3x3_s2_C32_relu", 32, 32, (3, 3), (17, 33), kernel=DIRECT, group=32, attrs={"pads": [1, 1, 1, 1], "strides": [2, 2]},
          wt=U8, zw=11, per_channel=True, zx=255, tail=dict(act="relu"))
    cmm("mm_2x33x64_N100_bias", (2, 33, 64), 100, wt=U8, zw=128, tail=dict(per_channel=True))
    cmm("mm_65x20_N3_bias_relu", (65, 20), 3, wt=U8, zw=200, zx=0, tail=dict(act="relu"))
    cmm("mm_2x33x200_N64_nobias_swapped", (2, 33, 200), 64, wt=S8, zw=0, per_channel=True, tail=dict(bias=False, swap=True))


# one DynamicQuantizeLinear feeding two chains (Q, K, V share one): both fuse, the quantise launches appear once
def _shared(b, bt):
    name = "ch_shared_two_convs"
    bt.feeds[f"{name}_x"] = x_planted(name, (2, 8, 9, 11), "mid", True)
    xq = dynq(b, f"{name}_x")
    rest = ()
    for q, (cout, k) in enumerate(((5, 3), (70, 1))):
        acc, sc, _, M_, _ = integer_node(b, bt, f"{name}/{q}", "conv", None, (cout, 8, k, k), wt=U8, zw=128, xq=xq,
                                         attrs={"kernel_shape": [k, k], "pads": [k // 2] * 4})
        rest += (TILE,) + chain_tail(b, bt, f"{name}/{q}", acc, sc, M_, "conv", True, act="relu", K=8 * k * k)
    bt.kernels, bt.unfused, bt.fused = (MINMAX, DYNQ, TILE, TILE), (MINMAX, DYNQ) + rest, 2


case("ch_shared_two_convs", F_CHAIN, _shared)


# ---- near misses: the launches as they are, the same values, vso_dynq_count 0 (dyadic) ---------------
def miss_case(name, miss, tail=None, **kw):
    chain_case(f"miss_{name}", F_MISS, TILE, "conv", (2, 8, 9, 11), (5, 8, 3, 3), True,
               attrs={"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, wt=U8, zw=128, miss=miss, tail=dict(tail or {}, act="relu"), **kw)


miss_case("cast_read_twice", "cast_read_twice")
miss_case("s_read_elsewhere", "s_read_elsewhere")
miss_case("runtime_bias", "runtime_bias")
# a w_scale of Wo = 11 values: it broadcasts along the last axis, not the channels
miss_case("w_scale_of_another_size", "w_scale_size", tail=dict(per_channel=True, ws_shape=(11,), bias=False))


# ---- refused at creation, naming the operator --------------------------------------------------
F_REF = "refused"


def refuse(name, op, fn):
    case(f"refuse_{name}", F_REF, fn, expect="refused", op=op)


def _refusal(kind, what):
    conv = kind == "conv"

    def fn(b, bt):
        xs = (2, 3, 5, 7) if conv else (2, 5, 7)
        bt.feeds["rx"] = x_planted("refuse", xs, "mid", True)
        y, sc, zp = dynq(b, "rx")
        wshape = (8, 3, 3, 3) if conv else (7, 8)
        wq, zw = w_ints("refuse", wshape, U8, 128, 3)
        ins = [y, b.const(wq), zp, b.const(zw)]
        if what == "runtime_weights":
            bt.feeds["rw"] = np.zeros(wshape, F32)
            ins[1] = "rw"
        elif what == "float_input":
            ins[0] = "rx"
        elif what == "runtime_weight_zero_point":
            bt.feeds["rz"] = np.zeros((), F32)
            ins[3] = "rz"
        elif what == "weight_zero_point_size":
            ins[3] = b.const(np.asarray([128, 127, 126], U8))
        elif what == "input_zero_point_size":
            ins[2] = b.const(np.asarray([0, 1], U8))
        elif what == "B_rank_3":
            ins[1] = b.const(np.zeros((2, 7, 8), U8))
        elif what == "int32_graph_output":
            pass
        acc = b.op("ConvInteger" if conv else "MatMulInteger", ins, **({"kernel_shape": [3, 3]} if conv else {}))
        if what == "int32_graph_output":
            bt.outs[acc] = "exact"
        elif what == "int32_read_by_relu":
            bt.outs[b.op("Relu", [acc])] = "exact"
        elif what == "zero_point_read_by_cast":
            bt.outs[b.op("Cast", [acc], to=R.DT_FLOAT)] = "exact"
            bt.outs[b.op("Cast", [zp], to=R.DT_FLOAT)] = "exact"
        elif what == "y_read_by_relu":
            bt.outs[b.op("Cast", [acc], to=R.DT_FLOAT)] = "exact"
            bt.outs[b.op("Relu", [y])] = "exact"
        else:
            bt.outs[b.op("Cast", [acc], to=R.DT_FLOAT)] = "exact"
    return fn


for kind_, op_ in (("conv", "ConvInteger"), ("matmul", "MatMulInteger")):
    for what_ in ("runtime_weights", "float_input", "runtime_weight_zero_point", "weight_zero_point_size",
                  "input_zero_point_size"):
        refuse(f"{op_}_{what_}", op_, _refusal(kind_, what_))
refuse("MatMulInteger_B_rank_3", "MatMulInteger", _refusal("matmul", "B_rank_3"))
refuse("int32_graph_output", "int32", _refusal("conv", "int32_graph_output"))
refuse("int32_read_by_Relu", "Relu", _refusal("conv", "int32_read_by_relu"))
refuse("zero_point_read_by_Cast", "Cast", _refusal("conv", "zero_point_read_by_cast"))
refuse("y_read_by_Relu", "Relu", _refusal("matmul", "y_read_by_relu"))

VALUE_CASES = [k for k in CASES if k.expect == "value"]
REFUSED_CASES = [k for k in CASES if k.expect == "refused"]
BY_NAME = {k.name: k for k in CASES}


def groups():
    """{family: its value cases}; one model and one session per family."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    return out


def general_bound(rule, env):
    """(the float64 value act(acc * s + bias), the bound 4 * 2^-24 * (|acc| s + |bias|)) of a general chain output."""
    acc = env[rule["acc"]].astype(np.float64)
    shape = [1] * acc.ndim
    shape[rule["axis"]] = -1
    s = np.float64(env[rule["scale"]]) * rule["ws"].astype(np.float64).reshape(shape)
    bias = np.zeros(1) if rule["bias"] is None else rule["bias"].astype(np.float64).reshape(shape)
    v = acc * s + bias
    if rule["lo"] is not None:
        v = np.maximum(v, rule["lo"])
    if rule["hi"] is not None:
        v = np.minimum(v, rule["hi"])
    return v, 4.0 * 2.0 ** -24 * (np.abs(acc) * s + np.abs(bias))
