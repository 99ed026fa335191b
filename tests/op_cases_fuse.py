"""The fusion matrix of the ONNX sessions' planner (test infrastructure): small
multi-node graphs, one per (deferred state of vso_plan.hip's Planner, consumer)
pair and per (kernel form, fused epilogue or in-place write) pair.  op_cases.Case
objects packed by op_cases.build, kept in this module's own list (op_cases.CASES
and the parametrisation of tests/test_gpu_op_matrix.py do not move).  Shared by
tests/test_fuse_ref.py (the oracle against PyTorch in float64, CPU) and
tests/test_gpu_fuse_matrix.py (the GPU sessions against the oracle).

Batch 2 everywhere: Epilogue::res_mode 1 / 2 address the residual's planes by
the image n, and a producer re-pointed into a Concat adds n * y_nx.  Planes 9x11
(99 pixels: a tail on every tile) and 7x9; 8x12 and 10x12 (rows of a multiple
of 4) for the float4 stores; a form with a size threshold takes the conv
family's smallest shape for it.  Weights are standard normal / sqrt(fan-in),
biases 0.1 standard normal.

Families (`kernels`: an f32 session's launches of the case alone, `kernels16`: a
bf16 / f16 session's where they differ; both asserted by name and order):

res     Add(Conv(x), Pad?(MaxPool2x2?(r))) [-> activation]: the Pad / MaxPool are
        find_residual_fusions' — no launch of their own, the convolution's
        epilogue reads r (Epilogue::res_mode 1: Pad only, 2: MaxPool), the only
        use of the n and pix every kernel passes to epilogue().  One case or more
        per kernel form; then the near misses, where Pad / MaxPool keep their
        launches.  (The Conv is the case's first node: where the Add's other
        operand is computed behind it, the Add is a launch of its own.)
res18   the near miss that needs opset 18 (Pad with axes).
cat     Concat(axis 1) of a produced tensor P and graph inputs, the Concat a
        graph output: P's producer writes into the Concat (y_nx), the graph
        inputs are copied.  CAT[name]: the Concat's inputs in order, ("P", channels)
        or ("in", position among the Concat node's inputs, channels).
catx    the same with a ConvTranspose producer (the oracle of tests/onnx_ref_ext.py).
pend    a deferred producer (up_pending / cat_up, cat_tail, pending_dw) in front
        of each kind of consumer: taken, or flushed by the consumer's plan.
hswish  Mul(x, HardSigmoid(x)) behind a Conv: one activation in its epilogue when
        the two are all that reads x.
"""
from __future__ import annotations

import numpy as np

import onnx_ref as R
import onnx_ref_ext as X
import op_cases as OC
from op_cases import IN0, PREV, Case, also_out, c, ci, node, small, then, x

CASES: list[Case] = []
CAT: dict[str, list] = {}
_seed = [0]

COPY, COPYR, POOL, BIN, UNARY = "k_copy(", "k_copy_rows<", "k_pool(", "k_binary", "k_unary("
DW, DWPW, GEMM, TILE, TILE_UP = "k_conv_dw(", "k_conv_dwpw(", "k_conv_gemm(", "k_conv_tile<", "k_conv_tile_up<"
RS_Q, RS_1 = "k_resize<true>(", "k_resize<false>("
P9, P7, P8 = (9, 11), (7, 9), (8, 12)


def case(name, family, op, inputs, attrs=None, **kw):
    assert all(k.name != name for k in CASES), name
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), **kw))


def w(shape, fan_in=None):
    """A seeded float32 constant: a weight (standard normal / sqrt(fan_in)) or, without fan_in, a bias."""
    _seed[0] += 1
    a = np.random.default_rng(9000 + _seed[0]).standard_normal(shape) * (0.1 if fan_in is None else fan_in ** -0.5)
    return ("c", a.astype(np.float32))


def cw(m, cg, kh=1, kw=None):
    """Conv weights [m][cg][kh][kw] and a bias."""
    kw = kh if kw is None else kw
    return [w((m, cg, kh, kw), cg * kh * kw), w((m,))]


def pw(name, m):
    return f"k_conv_pw<{1 if m <= 16 else 2 if m <= 32 else 4}, {name}>("


def tiled16(wspec, attrs, launches):
    """A case's launches in a bf16 / f16 session: a convolution onnx_ref.tiled_conv names runs on k_conv_tile."""
    if R.tiled_conv(wspec[1], attrs or {}):
        return tuple(TILE if k.startswith("k_conv_small<false") or k == GEMM else k for k in launches)
    return tuple(launches)


MAXPOOL = {"kernel_shape": [2, 2], "strides": [2, 2]}
RELU, LEAKY = then("Relu"), then("LeakyRelu", alpha=0.1)
CLIP6 = OC.CLIP6


def res_tail(k_conv, m, src, src_c, pool=True, pad=True, swap=False, act=None):
    """The nodes behind Conv node k_conv (m channels): [MaxPool 2x2 of `src`] -> [Pad to m channels] -> Add
    (swap: the residual first) [-> act]."""
    nodes, cur = [], src
    if pool:
        nodes.append(node("MaxPool", [cur], **MAXPOOL))
        cur = PREV
    if pad:
        nodes.append(node("Pad", [cur, ci(0, 0, 0, 0, 0, m - src_c, 0, 0)]))
        cur = PREV
    conv = ("node", k_conv)
    nodes.append(node("Add", [cur, conv] if swap else [conv, cur]))
    return nodes + ([act] if act else [])


def res(name, xs, ws, form, src, attrs=None, pre=(), m=None, family="res", k16=None, **tail):
    """Conv (weights `ws`; `pre`: the nodes behind it up to the convolution that carries the residual, which has m
    channels) with the strided residual of `src` (a graph input's shape, or IN0 with its shape in src_shape)."""
    src_shape = tail.pop("src_shape", None) or src
    src_spec = IN0 if src is IN0 else x(*src)
    m = m or ws[0]
    wb = cw(ws[0], ws[1], ws[2], ws[3])
    chain = list(pre) + res_tail(len(pre), m, src_spec, src_shape[1], **tail)
    launches = (form,) if isinstance(form, str) else tuple(form)
    case(f"Res_{name}", family, "Conv", [x(*xs)] + wb, attrs, kernels=launches, chain=tuple(chain),
         kernels16=k16 if k16 is not None else (launches if pre else tiled16(wb[0], attrs, launches)))


PADS1 = {"pads": [1, 1, 1, 1]}
S8, S16S, S32 = small(False, 8, False), small(False, 16, True), small(False, 32, False)
X9 = (2, 3, *P9)

# ---- res: k_conv_small<false, 8, false> (C 3 -> 5 / 20, 3x3 on 9x11) takes the whole list ----------------
# mode 1: Pad only, res_c 3 < M 5, the source plane the output plane
res("small8_pad_only", X9, (5, 3, 3, 3), S8, (2, 3, *P9), PADS1, pool=False)
# mode 2 without Pad: res_c == M, an even source plane
res("small8_pool", X9, (5, 3, 3, 3), S8, (2, 5, 18, 22), PADS1, pad=False)
# mode 2 with Pad: res_c 3 < M, the residual the Add's first operand
res("small8_pool_pad_swapped", X9, (5, 3, 3, 3), S8, (2, 3, 18, 22), PADS1, swap=True)
# mode 2 from an odd source plane, 19 x 23: its last row and column are not read; an activation behind the Add
res("small8_pool_pad_odd_relu", X9, (5, 3, 3, 3), S8, (2, 3, 19, 23), PADS1, act=RELU)
# res_c 17 of M 20: one past the 16-channel tile
res("small8_M20_resc17_odd_prelu", X9, (20, 3, 3, 3), S8, (2, 17, 19, 23), PADS1, act=then("PRelu", w((20, 1, 1), 4.0)))
res("small8_M20_pad_only_resc17_swapped_clip", X9, (20, 3, 3, 3), S8, (2, 17, *P9), PADS1, pool=False, swap=True, act=CLIP6)
# the other forms of k_conv_small<false, ...>: four waves over K (K 135), 32-wide chunks (K 72), stride 2
res("small16s_pool_pad_odd", (2, 15, *P9), (17, 15, 3, 3), S16S, (2, 5, 19, 23), PADS1, act=LEAKY)
res("small16s_pad_only_swapped", (2, 15, *P9), (17, 15, 3, 3), S16S, (2, 16, *P9), PADS1, pool=False, swap=True)
res("small32_pool_odd", (2, 8, *P9), (20, 8, 3, 3), S32, (2, 20, 19, 23), PADS1, pad=False)
res("small16_s2_pool_of_input", (2, 4, 19, 23), (17, 4, 3, 3), small(False, 16, False), IN0, {"strides": [2, 2], "pads": [0, 0, 1, 1]},
    src_shape=(2, 4, 19, 23), act=RELU)
# k_conv_small<true, ...>: a grouped 1x1
res("small_pw_G2_pool_pad_odd", (2, 8, *P9), (10, 4, 1, 1), small(True, 8, False), (2, 7, 19, 23), {"group": 2}, swap=True)
res("small_pw_G2_pad_only_relu", (2, 8, *P9), (10, 4, 1, 1), small(True, 8, False), (2, 9, *P9), {"group": 2}, pool=False, act=RELU)
# k_conv_pw<1 | 2 | 4, 0> on 7x9
res("pw1_pool_pad_odd", (2, 3, *P7), (5, 3, 1, 1), pw(0, 5), (2, 3, 15, 19))
res("pw1_pad_only_swapped_relu", (2, 3, *P7), (5, 3, 1, 1), pw(0, 5), (2, 4, *P7), pool=False, swap=True, act=RELU)
res("pw2_pool_pad_odd_resc17", (2, 33, *P7), (20, 33, 1, 1), pw(0, 20), (2, 17, 15, 19), act=CLIP6)
res("pw4_pool_pad_odd_resc33", (2, 33, *P7), (40, 33, 1, 1), pw(0, 40), (2, 33, 15, 19), swap=True, act=RELU)
res("pw4_pool_even", (2, 33, *P7), (40, 33, 1, 1), pw(0, 40), (2, 40, 14, 18), pad=False)
# k_conv_dw, one output per thread (the Add is the depthwise's consumer: nothing is deferred)
DW5 = {"group": 5, "pads": [1, 1, 1, 1]}
res("dw_pool_pad_odd", (2, 5, *P9), (5, 1, 3, 3), DW, (2, 3, 19, 23), DW5, act=RELU)
res("dw_pad_only_swapped", (2, 5, *P9), (5, 1, 3, 3), DW, (2, 4, *P9), DW5, pool=False, swap=True)
res("dw_s2_pool_of_input", (2, 5, 19, 23), (5, 1, 3, 3), DW, IN0, {"group": 5, "strides": [2, 2], "pads": [0, 0, 1, 1]},
    src_shape=(2, 5, 19, 23), pad=False)
# k_conv_dwpw: BlazeFace's block — depthwise 3x3 stride 2, 1x1, Add(Pad(MaxPool(block input))); the residual is the 1x1's
DW24S2 = {"group": 24, "strides": [2, 2], "pads": [0, 0, 1, 1]}
res("dwpw_s2_pool_pad_of_input_odd", (2, 24, 19, 23), (24, 1, 3, 3), DWPW, IN0, DW24S2, pre=[then("Conv", *cw(40, 24))],
    m=40, src_shape=(2, 24, 19, 23), act=RELU)
res("dwpw_s2_pool_of_input_even_swapped", (2, 24, 18, 22), (24, 1, 3, 3), DWPW, IN0, DW24S2, pre=[RELU, then("Conv", *cw(24, 24))],
    m=24, src_shape=(2, 24, 18, 22), pad=False, swap=True)
res("dwpw_pad_only", (2, 24, *P9), (24, 1, 3, 3), DWPW, (2, 17, *P9), {"group": 24, "pads": [1, 1, 1, 1]},
    pre=[then("Conv", *cw(20, 24))], m=20, pool=False, act=LEAKY)
# k_conv_thin<M>: 63 pixels (the scalar path, whose last four-pixel group reaches past the plane) and 80 (float4)
res("thin4_pool_pad_odd_leaky", (2, 5, *P7), (4, 5, 1, 1), "k_conv_thin<4>(", (2, 3, 15, 19), act=LEAKY)
res("thin3_pool_odd_swapped", (2, 5, *P7), (3, 5, 1, 1), "k_conv_thin<3>(", (2, 3, 15, 19), pad=False, swap=True)
res("thin2_pad_only_80", (2, 5, 8, 10), (2, 5, 1, 1), "k_conv_thin<2>(", (2, 1, 8, 10), pool=False)
res("thin1_pool_even_80", (2, 5, 8, 10), (1, 5, 1, 1), "k_conv_thin<1>(", (2, 1, 16, 20), pad=False, act=RELU)
# the forms with a size threshold: mode 2 with Pad from an odd source
# k_conv_gemm: 1024 64x64 tiles (the conv family's gemm_G8_Mg5)
res("gemm_G8_pool_pad_odd", (2, 24, 63, 65), (40, 3, 3, 3), GEMM, (2, 17, 127, 131), {"group": 8, "pads": [1, 1, 1, 1]},
    act=RELU, k16=(GEMM,))
# k_conv_pw<4, 3>: a depthwise 3x3 stride 2 -> 1x1 pair on 520 workgroups (the conv family's dwpw_pw4_3x3_s2)
res("dwpw_pw4_s2_pool_pad_of_input_odd", (2, 8, 181, 185), (8, 1, 3, 3), pw(3, 65), IN0,
    {"group": 8, "strides": [2, 2], "pads": [0, 0, 1, 1]}, pre=[then("Conv", *cw(65, 8))], m=65, src_shape=(2, 8, 181, 185))
# k_conv_dw_plane<2> (the conv family's dw_plane2_s2; under VSO_DW_PLANE=0 the quad body of k_conv_dw)
res("dw_plane2_s2_pool_pad_odd", (4, 64, 128, 128), (64, 1, 3, 3), "k_conv_dw_plane<2>(", (4, 40, 129, 129),
    {"group": 64, "strides": [2, 2], "pads": [0, 0, 1, 1]}, act=RELU)
# k_conv_tile in f32: the smallest square case above kTileMinMacs (2 x 32 x 32 x 9 x 21 x 21 = 8.1e6)
res("tile_f32_pool_pad_odd", (2, 32, 21, 21), (32, 32, 3, 3), TILE, (2, 20, 43, 43), PADS1, act=RELU, k16=(TILE,))
res("tile_f32_pad_only_swapped", (2, 32, 21, 21), (32, 32, 3, 3), TILE, (2, 31, 21, 21), PADS1, pool=False, swap=True, k16=(TILE,))

# ---- res: near misses — Pad / MaxPool keep their launches (the Conv, then the other nodes in order) --------
R3, R5 = (2, 3, 18, 22), (2, 5, 18, 22)


def res_miss(name, nodes, launches, family="res", opset=13, n_out=1, ahead=()):
    """`ahead`: the launches in front of the Conv's, `launches`: those behind it."""
    wb = cw(5, 3, 3, 3)
    case(f"Res_miss_{name}", family, "Conv", [x(*X9)] + wb, PADS1, kernels=tuple(ahead) + (S8,) + tuple(launches),
         chain=tuple(nodes), kernels16=tuple(ahead) + (TILE,) + tuple(launches), opset=opset, n_out=n_out)


CONV0 = ("node", 0)
ADD = node("Add", [CONV0, PREV])
res_miss("pad_value", [node("MaxPool", [x(*R3)], **MAXPOOL), node("Pad", [PREV, ci(0, 0, 0, 0, 0, 2, 0, 0), c(0.5, np.float32)]), ADD],
         (POOL, COPY, BIN))
res_miss("pad_before_channels", [node("MaxPool", [x(*R3)], **MAXPOOL), node("Pad", [PREV, ci(0, 1, 0, 0, 0, 1, 0, 0)]), ADD],
         (POOL, COPY, BIN))
res_miss("pad_H", [node("Pad", [x(2, 5, 8, 11), ci(0, 0, 1, 0, 0, 0, 0, 0)]), ADD], (COPY, BIN))
res_miss("pad_axes", [node("MaxPool", [x(*R3)], **MAXPOOL), node("Pad", [PREV, ci(0, 2), None, ci(1)]), ADD], (POOL, COPY, BIN),
         family="res18", opset=18)
res_miss("pool_3x3", [node("MaxPool", [x(2, 5, 19, 23)], kernel_shape=[3, 3], strides=[2, 2]), ADD], (POOL, BIN))
res_miss("pool_ceil", [node("MaxPool", [x(2, 5, 17, 21)], ceil_mode=1, **MAXPOOL), ADD], (POOL, BIN))
res_miss("pool_pads", [node("MaxPool", [x(2, 5, 17, 21)], pads=[1, 1, 0, 0], **MAXPOOL), ADD], (POOL, BIN))
res_miss("pool_dil2", [node("MaxPool", [x(2, 5, 19, 23)], dilations=[2, 2], **MAXPOOL), ADD], (POOL, BIN))
res_miss("avgpool", [node("AveragePool", [x(*R5)], **MAXPOOL), ADD], (POOL, BIN))
res_miss("pool_is_output", [also_out(node("MaxPool", [x(*R5)], **MAXPOOL)), ADD], (POOL, BIN), n_out=2)
res_miss("pool_read_twice", [node("MaxPool", [x(*R5)], **MAXPOOL), ADD, node("Add", [PREV, ("node", 1)])], (POOL, BIN, BIN))
res_miss("conv_read_twice", [node("MaxPool", [x(*R5)], **MAXPOOL), ADD, node("Add", [PREV, CONV0])], (POOL, BIN, BIN))
res_miss("add_self", [node("Add", [CONV0, CONV0])], (BIN,))
# the residual's source is computed behind the Conv in node order: nothing the Conv's launch could read yet
res_miss("source_behind_conv", [node("Relu", [x(*R5)]), node("MaxPool", [PREV], **MAXPOOL), ADD], (UNARY, POOL, BIN))
# the Add broadcasts the residual over the batch: not the per-image planes the epilogue addresses (found when the
# Conv is planned: the MaxPool's launch comes in front of the Conv's)
res_miss("batch_broadcast", [node("MaxPool", [x(1, 5, 18, 22)], **MAXPOOL), ADD], (BIN,), ahead=(POOL,))
# a ConvTranspose (here the stride-1 form, lowered to a Conv) is not find_residual_fusions': Pad / MaxPool keep their launches
case("Res_miss_deconv_s1", "resx", "ConvTranspose", [x(*X9), w((3, 5, 3, 3), 27), w((5,))], PADS1, opset=14,
     kernels=(S8, POOL, COPY, BIN), kernels16=(S8, POOL, COPY, BIN),
     chain=(node("MaxPool", [x(*R3)], **MAXPOOL), node("Pad", [PREV, ci(0, 0, 0, 0, 0, 2, 0, 0)]), ADD))
case("Res_miss_deconv_s2", "resx", "ConvTranspose", [x(2, 18, 5, 7), w((18, 20, 2, 2), 18), w((20,))], {"strides": [2, 2]},
     opset=14, kernels=("k_deconv_tile<1>(", POOL, COPY, BIN), kernels16=("k_deconv_tile<1>(", POOL, COPY, BIN),
     chain=(node("MaxPool", [x(2, 17, 20, 28)], **MAXPOOL), node("Pad", [PREV, ci(0, 0, 0, 0, 0, 3, 0, 0)]), ADD))

# ---- cat: producers writing into a Concat in place ------------------------------------------------------------


def cat(name, op, inputs, attrs, m, hw, launches, slot, pre=(), k16=None, family="cat", opset=13, nbr=(3, 2), n=2):
    """`op` (then `pre`) produces P, m channels of `hw`; Concat of P and two graph inputs of nbr channels, P in
    `slot`.  c0 = 0, 3 or 5 channels: an odd base offset on the odd planes."""
    a, b = x(n, nbr[0], *hw), x(n, nbr[1], *hw)
    p_ = ("node", len(pre))
    ins = [p_, a, b] if slot == 0 else [a, p_, b] if slot == 1 else [a, b, p_]
    nm = f"Cat_{name}_slot{slot}"
    CAT[nm] = [("P", m) if v is p_ else ("in", k, v[1][1]) for k, v in enumerate(ins)]
    launches = tuple(launches)
    case(nm, family, op, inputs, attrs, kernels=launches + (COPYR, COPYR), kernels16=tuple(k16 or launches) + (COPYR, COPYR),
         chain=tuple(pre) + (node("Concat", ins, axis=1),), opset=opset)


def cat_conv(name, xs, ws, attrs, launches, slots=(0, 1, 2), pre=(), m=None, k16=None, **kw):
    wb = cw(*ws)
    hw = kw.pop("hw", xs[2:])
    launches = (launches,) if isinstance(launches, str) else tuple(launches)
    for slot in slots:
        cat(name, "Conv", [x(*xs)] + wb, attrs, m or ws[0], hw, launches, slot, pre=pre,
            k16=k16 or (launches if pre else tiled16(wb[0], attrs, launches)), n=xs[0], **kw)


cat_conv("small8", X9, (5, 3, 3, 3), PADS1, S8)            # (16-bit: k_conv_tile at 9x11, one chunk of channels)
cat_conv("small16s", (2, 15, *P9), (17, 15, 3, 3), PADS1, S16S)
cat_conv("small16s_C200", (2, 200, *P9), (5, 200, 3, 3), PADS1, S16S, slots=(1,))  # (16-bit: k_conv_tile over 7 chunks)
cat_conv("small_pw_G2", (2, 8, *P9), (10, 4, 1, 1), {"group": 2}, small(True, 8, False))
cat_conv("pw1", (2, 3, *P7), (5, 3, 1, 1), {}, pw(0, 5))
cat_conv("pw2", (2, 33, *P7), (20, 33, 1, 1), {}, pw(0, 20))
cat_conv("pw4", (2, 33, *P7), (40, 33, 1, 1), {}, pw(0, 40))
cat_conv("dw", (2, 5, *P9), (5, 1, 3, 3), DW5, DW)
cat_conv("dwpw", (2, 24, *P9), (24, 1, 3, 3), {"group": 24, "pads": [1, 1, 1, 1]}, DWPW, pre=[RELU, then("Conv", *cw(70, 24))], m=70)
cat_conv("thin4", (2, 5, *P7), (4, 5, 1, 1), {}, "k_conv_thin<4>(")
cat_conv("thin3_8x12", (2, 5, *P8), (3, 5, 1, 1), {}, "k_conv_thin<3>(")  # (float4 stores at p.y + n (M P + y_nx) + m P)
# a Conv with an absorbed residual and activation: res is indexed without y_nx, y with it (res_mode 0, and 2)
cat_conv("small8_add_relu", X9, (5, 3, 3, 3), PADS1, S8, pre=[then("Add", x(2, 5, *P9)), RELU], k16=(TILE,))
cat_conv("small8_pool_pad_relu", X9, (5, 3, 3, 3), PADS1, S8, pre=res_tail(0, 5, x(2, 3, 19, 23), 3, act=RELU), k16=(TILE,))
# the forms with a size threshold, the middle slot: k_conv_gemm, k_conv_pw<4, 3>, and k_conv_dw_plane<1>'s float4 stores
cat_conv("gemm_G8", (2, 24, 63, 65), (40, 3, 3, 3), {"group": 8, "pads": [1, 1, 1, 1]}, GEMM, slots=(1,), k16=(GEMM,))
cat_conv("dwpw_pw4", (2, 8, 90, 92), (8, 1, 3, 3), {"group": 8, "pads": [1, 1, 1, 1]}, pw(3, 65), slots=(1,),
         pre=[then("Conv", *cw(65, 8))], m=65)
cat_conv("dw_plane1", (2, 33, 127, 128), (33, 1, 3, 3), {"group": 33, "pads": [1, 1, 1, 1]}, "k_conv_dw_plane<1>(", slots=(1,))
# Resize, not pending (the Concat is a graph output): nearest 2x onto 8x12 (float4), linear 1.5x onto 10x13
for slot_ in (0, 1, 2):
    cat("resize_quad", "Resize", [x(2, 3, 4, 6), None, c([1, 1, 2, 2], np.float32)], {"mode": "nearest"}, 3, P8, [RS_Q], slot_)
    cat("resize_one", "Resize", [x(2, 3, *P7), None, c([1, 1, 1.5, 1.5], np.float32)],
        {"mode": "linear", "coordinate_transformation_mode": "half_pixel"}, 3, (10, 13), [RS_1], slot_)
    # ConvTranspose: k_deconv_tile<1> and k_deconv_direct onto 10x14 (k_deconv_tile<2> needs 1024 workgroups: in a Concat
    # in tests/op_cases_deconv.py)
    cat("deconv_tile", "ConvTranspose", [x(2, 18, 5, 7), w((18, 20, 2, 2), 18), w((20,))], {"strides": [2, 2]}, 20, (10, 14),
        ["k_deconv_tile<1>("], slot_, family="catx", opset=14)
    cat("deconv_direct", "ConvTranspose", [x(2, 8, 5, 7), w((8, 3, 2, 2), 4), w((6,))], {"strides": [2, 2], "group": 2}, 6,
        (10, 14), ["k_deconv_direct("], slot_, family="catx", opset=14)

# k_deconv_tile<2> (both x phases per workgroup, float2 stores): 1024 workgroups, the middle slot
cat("deconv_tile2", "ConvTranspose", [x(2, 16, 64, 256), w((16, 16, 2, 2), 16), w((16,))], {"strides": [2, 2]}, 16, (128, 512),
    ["k_deconv_tile<2>("], 1, family="catx", opset=14)
# an inverted-residual block whose output goes into a Concat: match_ir leaves it to the generic plan (its last line),
# whose project (k_conv_dwpw, the residual Add in its epilogue) writes in place
_blk = [OC.clip(0.0, 6.0), then("Conv", *cw(144, 1, 3), group=144, pads=[1, 1, 1, 1]), OC.clip(0.0, 6.0),
        then("Conv", *cw(24, 144)), then("Add", IN0)]
cat("ir_block_generic", "Conv", [x(2, 24, 5, 18)] + cw(144, 24), {}, 24, (5, 18), [pw(0, 144), DWPW], 1, pre=_blk)

# two produced inputs in one Concat: both written in place, one copy
_wb = cw(5, 3, 3, 3)
CAT["Cat_two_produced"] = [("P", 5), ("in", 1, 3), ("P", 6)]
case("Cat_two_produced", "cat", "Conv", [x(*X9)] + _wb, PADS1, kernels=(S8, pw(0, 6), COPYR), kernels16=(TILE, pw(0, 6), COPYR),
     chain=(node("Conv", [IN0] + cw(6, 3)), node("Concat", [CONV0, x(2, 3, *P9), PREV], axis=1)))


def cat_miss(name, nodes, launches, parts, k16=None, **kw):
    CAT[f"Cat_miss_{name}"] = parts
    wb = cw(5, 3, 3, 3)
    case(f"Cat_miss_{name}", "cat", "Conv", [x(*X9)] + wb, PADS1, kernels=(S8,) + tuple(launches),
         kernels16=(TILE,) + tuple(k16 or launches), chain=tuple(nodes), **kw)


# near misses: P is copied like the graph inputs
cat_miss("axis2", [node("Concat", [x(2, 5, 2, 11), CONV0, x(2, 5, 1, 11)], axis=2)], (COPY,) * 3, None)
cat_miss("rank3", [then("Reshape", ci(2, 5, 99)), node("Concat", [x(2, 3, 99), PREV, x(2, 2, 99)], axis=1)], (COPYR,) * 3, None)
cat_miss("P_is_output", [node("Concat", [x(2, 3, *P9), CONV0, x(2, 2, *P9)], axis=1)], (COPYR,) * 3,
         [("in", 0, 3), ("P", 5), ("in", 2, 2)], op_out=True, n_out=2)
cat_miss("P_read_twice", [also_out(node("Relu", [CONV0])), node("Concat", [x(2, 3, *P9), CONV0, x(2, 2, *P9)], axis=1)],
         (UNARY,) + (COPYR,) * 3, [("in", 0, 3), ("P", 5), ("in", 2, 2)], n_out=2)
# a nested Concat: the inner one's inputs are written in place, its output is copied into the outer one
cat_miss("nested", [node("Concat", [x(2, 3, *P9), CONV0], axis=1), node("Concat", [PREV, x(2, 2, *P9)], axis=1)],
         (COPYR,) * 3, None)

# ---- pend: a deferred producer in front of each kind of consumer ----------------------------------------------
UP = {"mode": "linear", "coordinate_transformation_mode": "half_pixel"}
UP_PT = {"mode": "linear", "coordinate_transformation_mode": "pytorch_half_pixel"}
XU = (2, 32, 5, 6)      # -> 2 x 32 x 10 x 12
PU = (10, 12)
SCALE2 = c([1, 1, 2, 2], np.float32)
XQ = ("q8", XU)


def up(name, nodes, f32, b16, attrs=UP, family="pend", n_out=1, opset=13):
    """Resize 2x linear of a graph input [2, 32, 5, 6], then `nodes`.  f32 / b16: the launches of an f32 / a 16-bit
    session (f32: nothing is pending, the Resize is the first launch).  The input holds multiples of 1/8: the
    interpolation is exact, in the session's float32 and the oracle's float64 alike, so the convolution behind it
    rounds the same operands to 16 bits on both sides and the per-element bar tests the indexing (a standard normal
    input puts one operand in some thousand on the other side of a 16-bit rounding step: 3.7 to 8.8 bars in bf16)."""
    case(f"Up_{name}", family, "Resize", [XQ, None, SCALE2], attrs, kernels=tuple(f32), kernels16=tuple(b16),
         chain=tuple(nodes), n_out=n_out, opset=opset)


def conv3(m, cin=32, **attrs):
    return then("Conv", *cw(m, cin // attrs.get("group", 1), 3), **dict({"pads": [1, 1, 1, 1]}, **attrs))


# taken: a dense 3x3 / 5x5 at stride 1 onto one tile of at most 32 output channels interpolates while staging
up("conv3_M16_taken", [conv3(16)], (RS_Q, S16S), (TILE_UP,))
up("conv3_M32_relu_taken_pytorch", [conv3(32), RELU], (RS_Q, S16S), (TILE_UP,), attrs=UP_PT)
up("conv5_M16_taken", [then("Conv", *cw(16, 32, 5), pads=[2, 2, 2, 2])], (RS_Q, S16S), (TILE_UP,))
# consumers that cannot take it: the Resize keeps its launch
up("pw", [then("Conv", *cw(20, 32))], (RS_Q, pw(0, 20)), (RS_Q, pw(0, 20)))
up("thin", [then("Conv", *cw(2, 32))], (RS_Q, "k_conv_thin<2>("), (RS_Q, "k_conv_thin<2>("))
up("dw_pw", [then("Conv", *cw(32, 1, 3), group=32, pads=[1, 1, 1, 1]), RELU, then("Conv", *cw(20, 32))], (RS_Q, DWPW), (RS_Q, DWPW))
_ir = [then("Conv", *cw(192, 32)), OC.clip(0.0, 6.0), then("Conv", *cw(192, 1, 3), group=192, pads=[1, 1, 1, 1]),
       OC.clip(0.0, 6.0), then("Conv", *cw(24, 192))]
up("ir_start", _ir, (RS_Q, "k_ir<2, 2, 1", "k_ir_reduce("), (RS_Q, "k_ir_b16<1, 2, 1", "k_ir_reduce("))
up("conv3_s2", [conv3(16, strides=[2, 2])], (RS_Q, S16S), (RS_Q, TILE))
up("conv3_M40", [conv3(40)], (RS_Q, S16S), (RS_Q, TILE))
up("conv3_G2", [conv3(16, group=2)], (RS_Q, S16S), (RS_Q, S16S))
up("conv3_dil2", [conv3(16, dilations=[2, 2], pads=[2, 2, 2, 2])], (RS_Q, S16S), (RS_Q, S16S))
up("reshape_conv3", [then("Reshape", ci(2, 32, 10, 12)), conv3(16)], (RS_Q, S16S), (RS_Q, TILE))
up("deconv", [then("ConvTranspose", w((32, 16, 2, 2), 32), w((16,)), strides=[2, 2])], (RS_Q, "k_deconv_tile<1>("),
   (RS_Q, "k_deconv_tile<1>("), family="pendx", opset=14)
# through a Concat written in place
RES0 = ("node", 0)
# the Resize's range first and 32-aligned, two skips of 3 and 5 channels behind it: computed by the consumer
up("cat_first_taken", [node("Concat", [RES0, x(2, 3, *PU), x(2, 5, *PU)], axis=1), conv3(16, 40)],
   (RS_Q, COPYR, COPYR, S16S), (COPYR, COPYR, TILE_UP))
# ... and a last input that starts at channel 32: `up` and `cat_tail` together, no copy at all (f32: the tail is
# flushed, the convolution is below kTileMinMacs)
up("cat_first_and_tail_taken", [node("Concat", [RES0, x(2, 8, *PU)], axis=1), conv3(16, 40)], (RS_Q, COPYR, S16S), (TILE_UP,))
# the Resize's range behind a skip of 5 channels: not 32-aligned, flushed (into the Concat)
up("cat_second_flushed", [node("Concat", [x(2, 5, *PU), RES0], axis=1), conv3(16, 37)], (RS_Q, COPYR, S16S), (COPYR, RS_Q, TILE))
# two upsampled inputs in one Concat: both flushed
up("cat_two_flushed", [node("Resize", [XQ, None, SCALE2], **UP), node("Concat", [RES0, PREV], axis=1), conv3(16, 64)],
   (RS_Q, RS_Q, S16S), (RS_Q, RS_Q, TILE))
# the consumer of the Concat is a 1x1: flush_input's walk over cat_up
up("cat_first_pw", [node("Concat", [RES0, x(2, 3, *PU)], axis=1), then("Conv", *cw(20, 35))], (RS_Q, COPYR, pw(0, 20)),
   (COPYR, RS_Q, pw(0, 20)))
up("cat_first_thin", [node("Concat", [RES0, x(2, 3, *PU)], axis=1), then("Conv", *cw(2, 35))], (RS_Q, COPYR, "k_conv_thin<2>("),
   (COPYR, RS_Q, "k_conv_thin<2>("))
# the consumer takes the Resize and writes into a Concat itself
up("conv3_taken_into_cat", [conv3(16), node("Concat", [x(2, 3, *PU), PREV], axis=1)], (RS_Q, S16S, COPYR), (TILE_UP, COPYR))


# cat_tail: the Concat's last input starts at channel 32 and the Concat feeds one Conv
def tail(name, nodes, f32, b16, cin=(32, 8), **kw):
    """Concat of two graph inputs of 32 and 8 channels on 9x11, then `nodes`."""
    case(f"Tail_{name}", "pend", "Concat", [x(2, cin[0], *P9), x(2, cin[1], *P9)], {"axis": 1}, kernels=tuple(f32),
         kernels16=tuple(b16), chain=tuple(nodes), **kw)


CC = (COPYR, COPYR)
tail("conv3_tile_taken", [conv3(16, 40)], CC + (S16S,), (COPYR, TILE))
tail("conv3_s2_tile_taken", [conv3(16, 40, strides=[2, 2])], CC + (S16S,), (COPYR, TILE))
tail("pw", [then("Conv", *cw(20, 40))], CC + (pw(0, 20),), CC + (pw(0, 20),))
tail("dw", [then("Conv", *cw(40, 1, 3), group=40, pads=[1, 1, 1, 1])], CC + (DW,), CC + (DW,))
tail("thin", [then("Conv", *cw(3, 40)), then("Sigmoid")], CC + ("k_conv_thin<3>(",), CC + ("k_conv_thin<3>(",))
tail("conv3_G2", [conv3(16, 40, group=2)], CC + (S16S,), CC + (S16S,))
_ir64 = [then("Conv", *cw(384, 64)), OC.clip(0.0, 6.0), then("Conv", *cw(384, 1, 3), group=384, pads=[1, 1, 1, 1]),
         OC.clip(0.0, 6.0), then("Conv", *cw(64, 384))]
tail("ir_start", _ir64, CC + ("k_ir<4, 4, 1", "k_ir_reduce("), CC + ("k_ir_b16<2, 4, 1", "k_ir_reduce("), cin=(32, 32))
tail("cat_is_output", [conv3(16, 40)], CC + (S16S,), CC + (TILE,), n_out=2, op_out=True)
# the tile form in f32: above kTileMinMacs (2 x 32 x 64 x 9 x 21 x 21 = 1.6e7), the tail taken in every session
case("Tail_conv3_tile_f32_taken", "pend", "Concat", [x(2, 32, 21, 21), x(2, 32, 21, 21)], {"axis": 1}, kernels=(COPYR, TILE),
     kernels16=(COPYR, TILE), chain=(conv3(32, 64), RELU))

# pending_dw: a depthwise whose 1x1 consumer is also the first Conv of an inverted-residual candidate (match_ir leaves
# it to the generic plan: no launch writes the depthwise's output), and the block's own depthwise -> project pair
_dw_ir = [RELU, then("Conv", *cw(144, 24)), OC.clip(0.0, 6.0), then("Conv", *cw(144, 1, 3), group=144, pads=[1, 1, 1, 1]),
          OC.clip(0.0, 6.0), then("Conv", *cw(24, 144))]
case("Dw_into_ir_start", "pend", "Conv", [x(2, 24, 5, 18)] + cw(24, 1, 3), {"group": 24, "pads": [1, 1, 1, 1]},
     kernels=(DWPW, DWPW), kernels16=(DWPW, DWPW), chain=tuple(_dw_ir))

# ---- hswish: Mul(x, HardSigmoid(x)) behind a Conv ------------------------------------------------------------
_pw = [x(2, 6, *P9), w((5, 6, 1, 1), 6 / 9.0), w((5,))]  # (outputs of about +-3: both clamps bind)
HS = then("HardSigmoid", alpha=1 / 6, beta=0.5)
case("Hswish_fused", "hswish", "Conv", _pw, kernels=(pw(0, 5),), kernels16=(pw(0, 5),), opset=13,
     chain=(HS, node("Mul", [CONV0, PREV])))
case("Hswish_third_consumer", "hswish", "Conv", _pw, kernels=(pw(0, 5), UNARY, UNARY), kernels16=(pw(0, 5), UNARY, UNARY),
     n_out=2, chain=(HS, also_out(node("Mul", [CONV0, PREV])), node("Relu", [CONV0])))
case("Hswish_conv_is_output", "hswish", "Conv", _pw, kernels=(pw(0, 5), UNARY), kernels16=(pw(0, 5), UNARY), n_out=2,
     op_out=True, chain=(HS, node("Mul", [PREV, CONV0])))

VALUE_CASES = [k for k in CASES if k.expect == "value"]
BY_NAME = {k.name: k for k in CASES}
EXT = ("resx", "catx", "pendx", "hswish")  # families with a ConvTranspose or a HardSigmoid: tests/onnx_ref_ext.py's operators


def groups():
    """{family: its value cases}; a family has one opset, so one model holds it."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    for fam, ks in out.items():
        assert len({k.opset for k in ks}) == 1, fam
    return out


def oracle(model, feeds, prec="f32", want=None):
    """The float64 oracle's graph outputs (or the values named in `want`): oracle/onnx_ref.py's run() — for a
    bf16 / f16 session with conv_operands — and, node by node, tests/onnx_ref_ext.py for the operators that one holds."""
    conv_operands = None if prec == "f32" else prec
    if not any(nd["op"] in X.OWN for nd in model.nodes):
        return R.run(model, feeds, want=want, conv_operands=conv_operands)
    env = dict(model.inits)
    env.update({k: np.asarray(v) for k, v in feeds.items()})
    const = set(model.inits) - set(feeds)
    for nd in model.nodes:
        names = [i for i in nd["inputs"] if i]
        if all(i in const for i in names):
            const.update(nd["outputs"])
        m = object.__new__(R.Model)
        m.opset, m.nodes, m.inputs, m.outputs = model.opset, [nd], [], []
        m.inits = {i: env[i] for i in names if i in const - set(nd["outputs"])}
        run_feeds = {i: env[i] for i in names if i not in m.inits}
        if nd["op"] in X.OWN:
            env.update(X.run(m, run_feeds, want=nd["outputs"][:1]))
        else:
            env.update(R.run(m, run_feeds, want=[o for o in nd["outputs"] if o], conv_operands=conv_operands))
    return {k: env[k] for k in (want or [o[0] for o in model.outputs])}
