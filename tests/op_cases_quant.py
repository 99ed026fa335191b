"""The operator matrix of the statically quantised (QDQ) graphs (test
infrastructure): QuantizeLinear / DequantizeLinear of runtime tensors and the
three patterns the sessions run on the integers — a dense Conv (k_qconv_tile),
a depthwise Conv (k_qconv_dw), the quantised residual Add (k_qadd).
op_cases.Case objects packed by build() (op_cases.build, then this module's
seeded inputs), kept in this module's own list.  Shared by
tests/test_quant_ref.py (the reference tests/onnx_ref_quant.py against numpy,
PyTorch and an integer restatement of the fused arithmetic, CPU) and
tests/test_gpu_quant_matrix.py (the GPU sessions against the reference).

A case is QuantizeLinear of a float graph input, then its pattern, ending in a
QuantizeLinear: the case's output is a quantised tensor (a graph output, which
the session writes as exact integers in float32: one more k_dequantize).
`kernels` names each case's launches, in order; META[name]["unfused"] those of
the plan without the fused forms (VSO_QDQ=0): k_dequantize, the float kernel,
k_quantize.  Batch 2 throughout.

Two weightings.  Dyadic: every scale a power of two and |Wq - zw| bounded so
that every accumulator stays below 2^24 — every dequantised value, product,
sum and quotient is exact in float32 and float64 alike, exact ties occur, and
a session must equal the reference exactly, at any depth (the chains).
General: seeded arbitrary scales, one fused layer; an element whose unrounded
reference value lies farther than 1e-5 max(1, |v|) from a half-integer must be
equal, one nearer may differ by a step, and at most 2 % of a case may be that
near (a condition on the inputs, which test_quant_ref.py checks).
"""
from __future__ import annotations

import zlib

import numpy as np

import op_cases as OC
from op_cases import PREV, Case, also_out, c, node, then

CASES: list[Case] = []
META: dict[str, dict] = {}
INPUTS: dict[str, list] = {}  # case -> [(chain index or None, operand position, generator(shape) -> float32 array)]

Q, DQ, QCONV, QDW, QADD = "k_quantize(", "k_dequantize(", "k_qconv_tile(", "k_qconv_dw(", "k_qadd("
FORMS = (Q, DQ, QCONV, QDW, QADD)
CONV, UNARY, BINARY = "k_conv", "k_unary(", "k_binary"
U8, S8 = np.uint8, np.int8
RANGE = {U8: (0, 255), S8: (-128, 127)}
TAU, NEAR_TIE_SHARE = 1e-5, 0.02


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def case(name, family, op, inputs, attrs=None, meta=None, gen=(), **kw):
    assert all(k.name != name for k in CASES), name
    # (a seed per case: no two cases share a graph input, so each input can be rewritten for its case)
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), seed=len(CASES) + 1, **kw))
    META[name] = dict(meta or {})
    INPUTS[name] = list(gen)


def build(cases):
    """op_cases.build, with the cases' float inputs drawn by their own generators."""
    cases = list(cases)
    data, feeds, outs = OC.build(cases)
    for cs in cases:
        for k, pos_, fn in INPUTS[cs.name]:
            n = OC._input_name(cs, pos_) if k is None else OC._chain_input_name(cs, k, pos_)
            feeds[n] = np.asarray(fn(feeds[n].shape), np.float32)
    return data, feeds, outs


def qc(scale, zp, dtype):
    """The (scale, zero point) constants of a Q / DQ node; zp None: absent."""
    return (c(scale, np.float32),) if zp is None else (c(scale, np.float32), c(zp, dtype))


def x_gen(name, scale, zp, dtype, dyadic):
    """A float input whose quantisation covers the type's range and both saturation ends; dyadic: multiples of
    scale / 2, so a tenth of the elements are exact ties."""
    lo, hi = RANGE[dtype]
    z = 0 if zp is None else zp

    def fn(shape):
        r = _rng(name + "/x")
        if dyadic:
            k = r.integers(lo - 4, hi + 5, size=shape).astype(np.float64)
            k += np.where(r.random(shape) < 0.1, 0.5, 0.0)
        else:
            k = r.uniform(lo - 4.0, hi + 4.0, size=shape)
        return ((k - z) * np.float64(np.float32(scale))).astype(np.float32)
    return fn


# ---- qdq: the plain launches ------------------------------------------------------------
F_QDQ = "qdq"


def qdq(name, shape, scale, zp, dtype, dyadic, values=None, dq=False, q_out=False):
    """QuantizeLinear alone (its quantised output the case's), or -> DequantizeLinear (a float output; q_out: the
    quantised tensor a graph output too)."""
    gen = (lambda shp: np.broadcast_to(np.asarray(values, np.float64) * np.float64(np.float32(scale)), shp)) \
        if values is not None else x_gen(name, scale, zp, dtype, dyadic)
    chain, kernels, kw = (), (Q, DQ), {}
    if dq:
        chain = (node("DequantizeLinear", [PREV, *qc(scale, zp, dtype)]),)
        kernels = (Q, DQ, DQ) if q_out else (Q, DQ)
        kw = {"op_out": True, "n_out": 2} if q_out else {}
    case(name, F_QDQ, "QuantizeLinear", [("x", tuple(shape)), *qc(scale, zp, dtype)], chain=chain, kernels=kernels,
         meta={"weighting": "dyadic" if dyadic else "general", "fused": 0, "unfused": kernels}, gen=[(None, 0, gen)], **kw)


TIES = [2.5, 3.5, -0.5, -1.5, 0.5, 1.5, -2.5, 1e6, -1e6, np.inf, -np.inf, 0.0, 255.5, 254.5, -128.5, -127.5]
for dt_, zps_ in ((U8, (0, 3, 128, None)), (S8, (-128, -5, 0))):
    for zp_ in zps_:
        tag = f"{'u8' if dt_ is U8 else 's8'}_z{'none' if zp_ is None else zp_}".replace("-", "m")
        qdq(f"Q_ties_{tag}", (2, len(TIES)), 0.25, zp_, dt_, True, values=TIES)
        qdq(f"Q_dy_{tag}", (2, 3, 5, 7), 0.125, zp_, dt_, True)
        qdq(f"Q_gen_{tag}", (2, 3, 5, 7), 0.0173, zp_, dt_, False)
        qdq(f"QDQ_dy_{tag}", (2, 3, 5, 7), 0.5, zp_, dt_, True, dq=True)
        qdq(f"QDQ_gen_{tag}", (2, 3, 12, 13), 0.0173, zp_, dt_, False, dq=True, q_out=zp_ in (3, -5))


# ---- the fused forms --------------------------------------------------------------------
def w_ints(name, shape, wtype, zw, wmax, per_channel):
    """Quantised weights with |Wq - zw| <= wmax: (Wq, zero point constant or None)."""
    r = _rng(name + "/w")
    lo, hi = RANGE[wtype]
    d = r.integers(-wmax, wmax + 1, size=shape)
    z = np.full(shape[0], zw) if per_channel else np.asarray(zw)
    wq = np.clip(d + (z.reshape(-1, 1, 1, 1) if per_channel else z), lo, hi).astype(wtype)
    return wq, z.astype(wtype)


def conv_case(name, family, kernel, cin, cout, k, hw, dyadic, xt=U8, zx=3, wt=S8, zw=0, per_channel=False, bias="f",
              act=None, yt=U8, zy=None, group=1, fused=True, miss=None, wmax=None, attrs=None, chain_after=0):
    """Q(x) -> DQ -> Conv(., DQ(Wq), [B]) [-> Relu | Clip] -> Q; chain_after further fused 1x1 layers (dyadic)."""
    kh, kw = k
    cg = cin // group
    K = cg * kh * kw
    r = _rng(name)
    if dyadic:
        sx = 2.0 ** -4
        sw = (2.0 ** -(5 + np.arange(cout) % 3)) if per_channel else np.asarray(2.0 ** -5)
        wm = min(wmax or 127, max(1, (2 ** 23) // (255 * K)))
    else:
        sx = 0.0173
        sw = 0.0041 * (1.0 + np.arange(cout) / 7.0) if per_channel else np.asarray(0.0041)
        wm = wmax or 127
    # the output scale: some 40 steps per standard deviation of the sums (a power of two in the dyadic weighting)
    sy = float(sx * np.mean(sw) * (K ** 0.5) * 74.0 * (wm / 1.7) / 40.0)
    if dyadic:
        sy = 2.0 ** round(np.log2(sy))
    if zy is None:
        zy = {U8: 120, S8: -7}[yt] if act is None else {U8: 0, S8: -128}[yt]
    wq, zwc = w_ints(name, (cout, cg, kh, kw), wt, zw, wm, per_channel)
    sw32 = np.asarray(sw, np.float32)
    chain = [node("DequantizeLinear", [PREV, *qc(sx, zx, xt)]),
             node("DequantizeLinear", [c(wq), c(sw32), c(zwc)], **({"axis": 0} if per_channel else {}))]
    conv_in = [("node", 1), ("node", 2)]
    if bias == "f":
        b = r.integers(-40, 41, size=cout) * (sx * np.min(sw)) if dyadic else r.standard_normal(cout) * sy * 20
        conv_in.append(c(b, np.float32))
    elif bias == "i32":
        # the usual int32 bias of scale sx * sw (per tensor here: one scale)
        sb = np.asarray(np.float32(sx) * sw32.reshape(-1)[0], np.float32)
        chain.append(node("DequantizeLinear", [c(r.integers(-3000, 3001, size=cout), np.int32), c(sb)]))
        conv_in.append(("node", 3))
    at = {"kernel_shape": [kh, kw], "group": group}
    at.update(attrs or {})
    conv = node("Conv", conv_in, **at)
    chain.append(also_out(conv) if miss == "conv_out" else conv)
    if miss == "dq_out":
        chain[0] = also_out(chain[0])
    tail = []
    if act == "relu":
        tail.append(then("Relu"))
    elif act == "clip6":
        tail.append(OC.clip(0.0, 6.0))
    elif act == "clip_lo":
        tail.append(OC.clip(-8.0 * sy, 24.0 * sy))
    elif act == "clip_attr":
        tail.append(OC.clip(0.0, 6.0, attr=True))
    elif act == "clip_late":  # the lower bound a Constant node placed behind the Conv: not a value yet at the Conv
        j = len(chain)        # (chain[j - 1] is the Conv: node j; the Constant node j + 1)
        tail += [node("Constant", [], value=np.asarray(0.0, np.float32)), node("Clip", [("node", j), ("node", j + 1)])]
    chain += tail
    chain.append(node("QuantizeLinear", [PREV, *qc(sy, zy, yt)]))
    n_fused = 1 if fused else 0
    kernels = [Q, kernel, DQ] if fused else None
    for q in range(chain_after):  # further 1x1 layers on the quantised output: each one more fused launch
        w2, z2 = w_ints(f"{name}/{q}", (cout, cout, 1, 1), S8, 0, max(1, min(127, (2 ** 23) // (255 * cout))), False)
        j = len(chain)
        chain += [node("DequantizeLinear", [PREV, *qc(sy, zy, yt)]),
                  node("DequantizeLinear", [c(w2), c(2.0 ** -6, np.float32), c(z2)]),
                  node("Conv", [("node", j + 1), ("node", j + 2)], kernel_shape=[1, 1]), then("Relu"),
                  node("QuantizeLinear", [PREV, *qc(sy, 0 if yt is U8 else -128, yt)])]
        zy = 0 if yt is U8 else -128
        kernels.insert(-1, QCONV)
        n_fused += 1
    float_conv = (Q, DQ, CONV, Q, DQ)
    if miss == "dq_out":
        kernels = list(float_conv)
    elif miss in ("conv_out", "late_bound"):
        kernels = [Q, DQ, CONV] + ([UNARY] if act else []) + [Q, DQ]
    elif not fused:
        kernels = list(float_conv)
    n_out = 2 if miss in ("dq_out", "conv_out") else 1
    case(name, family, "QuantizeLinear", [("x", (2, cin) + tuple(hw)), *qc(sx, zx, xt)], chain=tuple(chain),
         kernels=tuple(kernels), n_out=n_out,
         meta={"weighting": "dyadic" if dyadic else "general", "fused": n_fused,
               "unfused": (Q, DQ, CONV, Q) + (DQ, CONV, Q) * chain_after + (DQ,) if miss is None else tuple(kernels),
               "conv": dict(cin=cin, cout=cout, k=k, group=group, attrs=at, sx=sx, zx=zx, xt=xt, sw=sw32, zw=zwc, wq=wq,
                            sy=sy, zy=zy, yt=yt, act=act, K=K)},
         gen=[(None, 0, x_gen(name, sx, zx, xt, dyadic))])


F_QCONV, F_QDW, F_QADD, F_MISS = "qconv", "qdw", "qadd", "qmiss"
PADS = {1: [0, 0, 0, 0], 3: [1, 1, 1, 1], 5: [2, 2, 2, 2]}
for dy_ in (True, False):
    t_ = "dy" if dy_ else "gen"

    def qconv(name, *a, **kw):
        conv_case(f"{name}_{t_}", F_QCONV, QCONV, *a, dy_, **kw)

    # kernels x channels x planes: Cin kh kw on both sides of 64 and of its multiples
    qconv("c1x1_3to8_5x7", 3, 8, (1, 1), (5, 7), zx=0)
    qconv("c1x1_64to16_12x13", 64, 16, (1, 1), (12, 13), zx=128, act="relu")
    qconv("c1x1_20to1_17x33", 20, 1, (1, 1), (17, 33), zx=255, bias=None)
    qconv("c3x3_3to24_12x13", 3, 24, (3, 3), (12, 13), attrs={"pads": PADS[3]}, per_channel=True, act="clip6", wmax=4)
    qconv("c3x3_16to40_5x7", 16, 40, (3, 3), (5, 7), attrs={"pads": PADS[3]}, xt=S8, zx=-128, bias="i32")
    qconv("c3x3_20to16_17x33", 20, 16, (3, 3), (17, 33), attrs={"pads": PADS[3]}, xt=S8, zx=-5, act="relu", yt=S8)
    qconv("c3x3_64to8_5x7", 64, 8, (3, 3), (5, 7), attrs={"pads": PADS[3]}, xt=S8, zx=0, per_channel=True, bias="i32")
    qconv("c5x5_3to16_12x13", 3, 16, (5, 5), (12, 13), attrs={"pads": PADS[5]}, zx=128, wt=U8, zw=128)
    qconv("c5x5_16to24_5x7", 16, 24, (5, 5), (5, 7), attrs={"pads": PADS[5]}, zx=255, act="clip_lo", yt=S8)
    qconv("c3x2_20to8_12x13", 20, 8, (3, 2), (12, 13), attrs={"pads": [1, 0, 1, 1]}, zx=3, per_channel=True)
    qconv("c3x3_s2_16to16_17x33", 16, 16, (3, 3), (17, 33), attrs={"pads": PADS[3], "strides": [2, 2]}, zx=3, act="relu")
    qconv("c3x3_d2_16to8_12x13", 16, 8, (3, 3), (12, 13), attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}, zx=128)
    qconv("c3x3_asym_3to8_12x13", 3, 8, (3, 3), (12, 13), attrs={"pads": [0, 2, 1, 0]}, zx=255, bias=None)
    qconv("c3x3_same_upper_s2_16to8_12x13", 16, 8, (3, 3), (12, 13), attrs={"auto_pad": "SAME_UPPER", "strides": [2, 2]},
          xt=S8, zx=-5)
    qconv("c5x5_same_lower_3to8_5x7", 3, 8, (5, 5), (5, 7), attrs={"auto_pad": "SAME_LOWER"}, zx=3, act="clip_attr", wmax=4)
    qconv("c3x3_valid_20to24_5x7", 20, 24, (3, 3), (5, 7), attrs={"auto_pad": "VALID"}, zx=128, wt=U8, zw=128,
          per_channel=True)

    def qdw(name, ch, k, hw, **kw):
        conv_case(f"{name}_{t_}", F_QDW, QDW, ch, ch, (k, k), hw, dy_, group=ch, **kw)

    qdw("dw3x3_C5_12x13", 5, 3, (12, 13), attrs={"pads": PADS[3]}, zx=3, act="relu")
    qdw("dw3x3_s2_C32_17x33", 32, 3, (17, 33), attrs={"pads": PADS[3], "strides": [2, 2]}, zx=128, per_channel=True,
        act="clip6", wmax=6)
    qdw("dw5x5_C1_5x7", 1, 5, (5, 7), attrs={"pads": PADS[5]}, xt=S8, zx=-5, bias="i32")
    qdw("dw5x5_s2_C5_12x13", 5, 5, (12, 13), attrs={"pads": PADS[5], "strides": [2, 2]}, zx=255, yt=S8)
    qdw("dw7x7_C32_12x13", 32, 7, (12, 13), attrs={"pads": [3, 3, 3, 3]}, zx=3, wt=U8, zw=128, bias=None)
    qdw("dw7x7_s2_C1_17x33", 1, 7, (17, 33), attrs={"pads": [3, 3, 3, 3], "strides": [2, 2]}, xt=S8, zx=-128, act="relu")

# chains of fused layers: dyadic only (exact at any depth)
conv_case("chain2_3x3_16to16_12x13_dy", F_QCONV, QCONV, 16, 16, (3, 3), (12, 13), True, attrs={"pads": PADS[3]},
          act="relu", chain_after=1)
conv_case("chain3_1x1_20to24_5x7_dy", F_QCONV, QCONV, 20, 24, (1, 1), (5, 7), True, xt=S8, zx=-5, yt=S8, act="relu",
          chain_after=2)

# the lane map: a 1x1 convolution over 64 channels by an asymmetric integer matrix, the input one-hot per pixel in
# channel p mod 64 — the output at (m, p) is W[m][p mod 64] (x 2: sx / sy), naming the (row, k) element read
LANE_MAP = "lane_map_1x1_64to40_12x13_dy"


def _lane_w():
    m, k = np.meshgrid(np.arange(40), np.arange(64), indexing="ij")
    return ((3 * m + 5 * k) % 11 - 5).astype(S8).reshape(40, 64, 1, 1)


def _lane_x(shape):
    n, ch, h, w = shape
    p = np.arange(h * w)
    a = np.zeros((n, ch, h * w), np.float32)
    for i in range(n):
        a[i, (p + 7 * i) % ch, p] = 1.0  # sx = 1: the one-hot quantises to itself
    return a.reshape(shape)


case(LANE_MAP, F_QCONV, "QuantizeLinear", [("x", (2, 64, 12, 13)), *qc(1.0, 0, U8)],
     chain=(node("DequantizeLinear", [PREV, *qc(1.0, 0, U8)]),
            node("DequantizeLinear", [c(_lane_w()), c(1.0, np.float32), c(0, S8)]),
            node("Conv", [("node", 1), ("node", 2)], kernel_shape=[1, 1]),
            node("QuantizeLinear", [PREV, *qc(1.0, 0, S8)])),
     kernels=(Q, QCONV, DQ), meta={"weighting": "dyadic", "fused": 1, "unfused": (Q, DQ, CONV, Q, DQ)},
     gen=[(None, 0, _lane_x)])


def qadd(name, shape, dyadic, at=U8, za=3, bt=U8, zb=100, yt=U8, zy=0, relu=False, sat=False, fused=True):
    """Q(a) -> DQ, Q(b) -> DQ, Add [-> Relu] -> Q."""
    if dyadic:
        sa, sb, sy = 2.0 ** -4, 2.0 ** -3, (2.0 ** -4 if sat else 2.0 ** -2)
    else:
        sa, sb, sy = 0.0173, 0.0291, (0.012 if sat else 0.047)
    chain = [node("DequantizeLinear", [PREV, *qc(sa, za, at)]),
             node("QuantizeLinear", [("x", tuple(shape)), *qc(sb, zb, bt)]),
             node("DequantizeLinear", [PREV, *qc(sb, zb, bt)]),
             node("Add", [("node", 1), ("node", 3)])]
    if relu:
        chain.append(then("Relu"))
    chain.append(node("QuantizeLinear", [PREV, *qc(sy, zy, yt)]))
    unf = (Q, DQ, Q, DQ, BINARY) + ((UNARY,) if relu else ()) + (Q, DQ)
    case(name, F_QADD, "QuantizeLinear", [("x", tuple(shape)), *qc(sa, za, at)], chain=tuple(chain),
         kernels=(Q, Q, QADD, DQ) if fused else unf,
         meta={"weighting": "dyadic" if dyadic else "general", "fused": int(fused), "unfused": unf},
         gen=[(None, 0, x_gen(name + "/a", sa, za, at, dyadic)), (1, 0, x_gen(name + "/b", sb, zb, bt, dyadic))])


for dy_ in (True, False):
    t_ = "dy" if dy_ else "gen"
    qadd(f"add_u8_u8_{t_}", (2, 5, 12, 13), dy_, zy=90)
    qadd(f"add_s8_u8_relu_{t_}", (2, 3, 5, 7), dy_, at=S8, za=-5, relu=True)
    qadd(f"add_u8_s8_to_s8_{t_}", (2, 3, 17, 33), dy_, bt=S8, zb=-128, yt=S8, zy=-7)
    qadd(f"add_s8_s8_sat_{t_}", (2, 5, 5, 7), dy_, at=S8, za=0, bt=S8, zb=0, yt=S8, zy=0, sat=True)
    qadd(f"add_u8_u8_sat_relu_{t_}", (2, 5, 5, 7), dy_, zy=0, sat=True, relu=True)

# ---- near misses: separate launches, the same values (dyadic) ----------------------------
conv_case("miss_dq_read_twice", F_MISS, QCONV, 16, 8, (3, 3), (5, 7), True, attrs={"pads": PADS[3]}, act="relu",
          fused=False, miss="dq_out")
conv_case("miss_conv_read_twice", F_MISS, QCONV, 16, 8, (3, 3), (5, 7), True, attrs={"pads": PADS[3]}, fused=False,
          miss="conv_out")
# uint8 weights with zero point 0: Wq - zw reaches 255
conv_case("miss_weights_leave_int8", F_MISS, QCONV, 3, 8, (3, 3), (5, 7), True, attrs={"pads": PADS[3]}, wt=U8, zw=0,
          wmax=200, fused=False)

# a Clip whose bound is a Constant node behind the Conv (legal order): the pattern is found, the bound is no value
# when the Conv is planned, and the nodes keep their own launches — the Clip too, which the float Conv cannot take
conv_case("miss_clip_bound_behind_conv", F_MISS, QCONV, 16, 8, (3, 3), (5, 7), True, attrs={"pads": PADS[3]},
          act="clip_late", fused=False, miss="late_bound")

# ---- refused at creation, naming the node's operator -------------------------------------
F_REF = "qrefused"
NAMES: dict[str, str] = {}
X4 = ("x", (2, 3, 5, 7))


def refuse(name, op, inputs, names=None, chain=(), attrs=None, **kw):
    case(f"refuse_{name}", F_REF, op, inputs, attrs, expect="refused", chain=tuple(chain), **kw)
    NAMES[f"refuse_{name}"] = names or op


refuse("Q_runtime_scale", "QuantizeLinear", [X4, ("pos", ()), c(0, U8)])
refuse("Q_runtime_zero_point", "QuantizeLinear", [X4, c(0.5, np.float32), ("pos", ())])
refuse("Q_per_axis", "QuantizeLinear", [X4, c([0.5, 0.25, 0.125], np.float32), c([0, 1, 2], U8)], attrs={"axis": 1})
refuse("Q_zero_point_int32", "QuantizeLinear", [X4, c(0.5, np.float32), c(0, np.int32)])
# 16-bit, 4-bit and float8 outputs asked for by attribute (opset 21), no zero point
for nm_, dt_ in (("int16", 5), ("uint16", 4), ("int4", 22), ("uint4", 21), ("float8e4m3fn", 17), ("float8e5m2", 19)):
    refuse(f"Q_output_dtype_{nm_}", "QuantizeLinear", [X4, c(0.5, np.float32)], attrs={"output_dtype": dt_}, opset=21)
# a quantised tensor read by anything but DequantizeLinear — here by the Add a Conv takes into its epilogue
refuse("Add_of_quantised_in_conv_epilogue", "QuantizeLinear", [X4, c(0.5, np.float32), c(0, U8)], names="Add",
       chain=[node("Conv", [("x", (2, 3, 5, 7)), OC.cf((3, 3, 1, 1), 77)]), node("Add", [PREV, ("node", 0)])])
refuse("DQ_of_float", "DequantizeLinear", [X4, c(0.5, np.float32), c(0, U8)])
refuse("DQ_per_axis", "QuantizeLinear", [X4, c(0.5, np.float32), c(0, U8)], names="DequantizeLinear",
       chain=[node("DequantizeLinear", [PREV, c([0.5, 0.25, 0.125], np.float32), c([0, 1, 2], U8)], axis=1)])
refuse("DQ_runtime_scale", "QuantizeLinear", [X4, c(0.5, np.float32), c(0, U8)], names="DequantizeLinear",
       chain=[node("DequantizeLinear", [PREV, ("pos", ()), c(0, U8)])])
refuse("Relu_of_quantised", "QuantizeLinear", [X4, c(0.5, np.float32), c(0, S8)], names="Relu", chain=[then("Relu")])
for op_ in ("QLinearConv", "ConvInteger", "MatMulInteger", "QLinearMatMul", "QLinearAdd"):
    refuse(op_, op_, [X4, X4])
# (the per-axis activation scale in front of a Conv is refuse_DQ_per_axis)
for k_ in CASES:
    if k_.expect == "refused":
        META[k_.name].update(weighting=None, fused=0)

VALUE_CASES = [k for k in CASES if k.expect == "value"]
REFUSED_CASES = [k for k in CASES if k.expect == "refused"]
BY_NAME = {k.name: k for k in CASES}
DYADIC = [k for k in VALUE_CASES if META[k.name]["weighting"] == "dyadic"]
GENERAL = [k for k in VALUE_CASES if META[k.name]["weighting"] == "general"]


def quantised_failures(o, g, w, v, dyadic):
    """What is wrong with the quantised values `g` against the reference's `w` (v: the reference's unrounded
    values): equal everywhere in a dyadic case; else equal away from a tie, within one step at one."""
    d = np.asarray(g).astype(np.int64) - np.asarray(w).astype(np.int64)
    if dyadic:
        return [f"{o}: {int((d != 0).sum())} quantised values differ in a dyadic case, first at "
                f"{tuple(np.argwhere(d != 0)[0])}"] if d.any() else []
    out = []
    if (d != 0)[~near_tie(v)].any():
        out.append(f"{o}: {int((d != 0)[~near_tie(v)].sum())} values differ away from a tie")
    if (np.abs(d) > 1).any():
        out.append(f"{o}: {int((np.abs(d) > 1).sum())} values differ by more than one step")
    return out


def near_tie(v):
    """Where the unrounded value lies within TAU max(1, |v|) of a half-integer."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.abs(v - np.floor(v)) - 0.5) <= TAU * np.maximum(1.0, np.abs(v))


def groups():
    """{family: its value cases}; one model and one session per family."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    return out


# ---- refused zero points the array writer has no dtype for: 4-bit (onnx_ref.Packed4), 16-bit and float8 tensors
# written by hand.  {case: (model bytes, the operator its message names)}
def _raw_tensor(name, dims, dtype, raw):
    b = b"".join(OC.R._key(1, 0) + OC.R._enc_varint(int(d)) for d in dims)
    return b + OC.R._key(2, 0) + OC.R._enc_varint(dtype) + OC.R._str(8, name) + OC.R._len(9, raw)


def _zero_point_model(zp, dq):
    """QuantizeLinear(x, 0.5, zp) — or, dq: QuantizeLinear(x, 0.5, uint8 0) -> DequantizeLinear(., 0.5, zp) — with
    `zp` a Packed4 or (TensorProto type, raw bytes) scalar."""
    R_ = OC.R
    inits = [R_.make_tensor("s", np.asarray(0.5, np.float32)), R_.make_tensor("z8", np.asarray(0, U8)),
             R_.make_tensor("zp", zp) if isinstance(zp, R_.Packed4) else _raw_tensor("zp", (), *zp)]
    nodes = [R_.make_node("QuantizeLinear", ["x", "s", "z8" if dq else "zp"], ["q" if dq else "y"])]
    if dq:
        nodes.append(R_.make_node("DequantizeLinear", ["q", "s", "zp"], ["y"]))
    g = b"".join(R_._len(1, n) for n in nodes) + R_._str(2, "g") + b"".join(R_._len(5, t) for t in inits)
    g += R_._len(11, R_.make_value_info("x", [2, 3, 5, 7])) + R_._len(12, R_.make_value_info("y", []))
    return R_._key(1, 0) + R_._enc_varint(8) + R_._len(7, g) + R_._len(8, R_._str(1, "") + R_._key(2, 0) + R_._enc_varint(21))


RAW_REFUSED: dict[str, tuple] = {}
for nm_, zp_ in (("uint4", OC.R.Packed4([3], False)), ("int4", OC.R.Packed4([-2], True)), ("int16", (5, b"\x03\x00")),
                 ("uint16", (4, b"\x03\x00")), ("float8e4m3fn", (17, b"\x38")), ("float8e5m2", (19, b"\x3c"))):
    RAW_REFUSED[f"refuse_Q_zero_point_{nm_}"] = (_zero_point_model(zp_, False), "QuantizeLinear")
    RAW_REFUSED[f"refuse_DQ_zero_point_{nm_}"] = (_zero_point_model(zp_, True), "DequantizeLinear")
