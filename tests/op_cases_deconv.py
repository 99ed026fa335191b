"""The operator matrix of ConvTranspose, HardSigmoid, HardSwish and ReduceMean
(test infrastructure): op_cases.Case objects in the style of tests/op_cases.py,
packed by op_cases.build, kept in this module's own list (op_cases.CASES and
the parametrisation of tests/test_gpu_op_matrix.py do not move).  Shared by
tests/test_deconv_ref.py (tests/onnx_ref_ext.py against PyTorch in float64,
CPU) and tests/test_gpu_deconv_matrix.py (the GPU sessions against
onnx_ref_ext).

Batch 2, planes 5x7 and 5x19: every phase grid is ragged (a phase's rows and
columns differ by one from its neighbour's), a 4-row pixel tile has a tail,
and at W = 19 a phase's columns cross one 16-column tile.  Weights are
standard normal / sqrt(fan-in), the fan-in being the channels per group times
the most taps of a phase, so outputs stay of order 1; biases 0.1 standard
normal.  `kernels` names the form each case is there to reach:
k_deconv_tile<1 | 2> (group 1, dilation 1, C >= 16 and M >= 16), k_deconv_direct
(the rest, and stride 1 with pads beyond the kernel's extent), or — stride 1 —
the convolution kernel of the Conv the node is rewritten to.
"""
from __future__ import annotations

import numpy as np

import op_cases as OC
from op_cases import Case, ci, then, x

CASES: list[Case] = []
TILE, DIRECT = "k_deconv_tile<1>(", "k_deconv_direct("
TILE2 = "k_deconv_tile<2>("  # stride 2 in x with at least 1024 workgroups: both x phases per workgroup
_seed = [0]


def case(name, family, op, inputs, attrs=None, **kw):
    assert all(k.name != name for k in CASES), name
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), **kw))


def _c(shape, scale):
    _seed[0] += 1
    return ("c", (np.random.default_rng(7000 + _seed[0]).standard_normal(shape) * scale).astype(np.float32))


def dw(c_, mg, k, s=(1, 1), group=1):
    """ConvTranspose weights [C][M / group][kh][kw]: fan-in = channels per group x the most taps of a phase."""
    taps = -(-k[0] // s[0]) * -(-k[1] // s[1])
    return _c((c_, mg, k[0], k[1]), ((c_ // group) * taps) ** -0.5)


def bias(m):
    return _c((m,), 0.1)


def deconv(name, family, xs, mg, k, kernels, s=(1, 1), group=1, with_bias=True, chain=(), **attrs):
    """One ConvTranspose of a graph input `xs` with constant weights (and a bias), then `chain`."""
    at = dict(attrs)
    if s != (1, 1):
        at["strides"] = list(s)
    if group != 1:
        at["group"] = group
    ins = [x(*xs), dw(xs[1], mg, k, s, group)] + ([bias(mg * group)] if with_bias else [])
    case(f"ConvTranspose_{name}", family, "ConvTranspose", ins, at, kernels=tuple(kernels), chain=tuple(chain), opset=14)


P57, P519 = (5, 7), (5, 19)
WHOLE = {"whole": True}

# ---- the tile form ------------------------------------------------------------------
T = "deconv_tile"
deconv("k2s2_18_20", T, (2, 18, *P57), 20, (2, 2), [TILE], s=(2, 2))
deconv("k2s2_18_20_nobias", T, (2, 18, *P57), 20, (2, 2), [TILE], s=(2, 2), with_bias=False)
deconv("k3s2_p1_op1_16_16", T, (2, 16, *P57), 16, (3, 3), [TILE], s=(2, 2), pads=[1, 1, 1, 1], output_padding=[1, 1])
deconv("k3s2_p1_op0_16_16", T, (2, 16, *P57), 16, (3, 3), [TILE], s=(2, 2), pads=[1, 1, 1, 1])
deconv("k4s2_p1_32_64_w19", T, (2, 32, *P519), 64, (4, 4), [TILE], s=(2, 2), pads=[1, 1, 1, 1])
deconv("k3s3_70_65", T, (2, 70, *P57), 65, (3, 3), [TILE], s=(3, 3))
deconv("k8s4_p2_18_20", T, (2, 18, *P57), 20, (8, 8), [TILE], s=(4, 4), pads=[2, 2, 2, 2])
deconv("k3x2_s2x1_18_20", T, (2, 18, *P57), 20, (3, 2), [TILE], s=(2, 1))
deconv("k4s2_pads0110_18_20_w19", T, (2, 18, *P519), 20, (4, 4), [TILE], s=(2, 2), pads=[0, 1, 1, 0])
# total padding 1 per axis (2 (H - 1) + 3 - 2 H): SAME_UPPER puts it at the end, SAME_LOWER at the beginning
deconv("k3s2_same_upper_16_16", T, (2, 16, *P57), 16, (3, 3), [TILE], s=(2, 2), auto_pad="SAME_UPPER")
deconv("k3s2_same_lower_16_16", T, (2, 16, *P57), 16, (3, 3), [TILE], s=(2, 2), auto_pad="SAME_LOWER")
# the unpadded output is 11 x 15: totals 1 and 2, split [1, 1, 0, 1]
deconv("k3s2_output_shape_16_16", T, (2, 16, *P57), 16, (3, 3), [TILE], s=(2, 2), output_shape=[10, 13])
deconv("k2s2_relu", T, (2, 18, *P57), 20, (2, 2), [TILE], s=(2, 2), chain=[then("Relu")])
deconv("k4s2_p1_hardswish", T, (2, 18, *P57), 20, (4, 4), [TILE], s=(2, 2), pads=[1, 1, 1, 1], chain=[then("HardSwish")])
deconv("k3s2_prelu", T, (2, 16, *P57), 20, (3, 3), [TILE], s=(2, 2), pads=[1, 1, 1, 1], output_padding=[1, 1],
       chain=[then("PRelu", _c((20, 1, 1), 0.25))])
deconv("k2s2_add", T, (2, 18, *P57), 20, (2, 2), [TILE], s=(2, 2), chain=[then("Add", x(2, 20, 10, 14))])
deconv("k4s2_p1_concat_skip", T, (2, 18, *P57), 20, (4, 4), [TILE, "k_copy_rows<"], s=(2, 2), pads=[1, 1, 1, 1],
       chain=[("Concat", (x(2, 6, 10, 14), ("prev",)), {"axis": 1}, WHOLE)])
# k_deconv_tile<2>: N x pixel tiles x y phases x channel blocks >= 1024.  64x256: outputs in aligned pairs
# (8-byte stores); 65x255 with pads 1: an odd plane (4-byte stores), ragged on every side; pads 1 on even
# planes: pairs that straddle the alignment and the row's ends
deconv("k2s2_16_16_64x256_pair", T, (2, 16, 64, 256), 16, (2, 2), [TILE2], s=(2, 2))
deconv("k3s2_p1_16_20_65x255_pair", T, (2, 16, 65, 255), 20, (3, 3), [TILE2], s=(2, 2), pads=[1, 1, 1, 1])
deconv("k4s2_p1_18_20_64x256_pair_relu", T, (2, 18, 64, 256), 20, (4, 4), [TILE2], s=(2, 2), pads=[1, 1, 1, 1],
       chain=[then("Relu")])

# ---- the direct form ----------------------------------------------------------------
D = "deconv_direct"
deconv("dw_k4s2_p1_12", D, (2, 12, *P57), 1, (4, 4), [DIRECT], s=(2, 2), group=12, pads=[1, 1, 1, 1])
deconv("g2_8_6_k3s2", D, (2, 8, *P57), 3, (3, 3), [DIRECT], s=(2, 2), group=2, pads=[1, 1, 1, 1], output_padding=[1, 1])
deconv("head_M1_k2s2_sigmoid", D, (2, 18, *P519), 1, (2, 2), [DIRECT], s=(2, 2), chain=[then("Sigmoid")])
deconv("head_C3_k4s2_p1", D, (2, 3, *P57), 20, (4, 4), [DIRECT], s=(2, 2), pads=[1, 1, 1, 1])
# (k d) mod s: dilation 2 at stride 2 leaves phase 1 without taps (those outputs are the bias);
# at stride 3 every phase has one tap, in the order 0, 2, 1
deconv("dil2_s2_18_20", D, (2, 18, *P57), 20, (3, 3), [DIRECT], s=(2, 2), dilations=[2, 2], pads=[1, 2, 2, 1])
deconv("dil2_s3_op21_6_5", D, (2, 6, *P57), 5, (3, 3), [DIRECT], s=(3, 3), dilations=[2, 2], output_padding=[2, 1])
deconv("dil2x1_s2x1_6_5", D, (2, 6, *P57), 5, (3, 2), [DIRECT], s=(2, 1), dilations=[2, 1])
deconv("below_C_15_16", D, (2, 15, *P57), 16, (2, 2), [DIRECT], s=(2, 2))
deconv("below_M_16_15", D, (2, 16, *P57), 15, (2, 2), [DIRECT], s=(2, 2), chain=[then("Relu")])
deconv("k9s2_taps5_16_16", D, (2, 16, *P57), 16, (9, 9), [DIRECT], s=(2, 2), pads=[4, 4, 4, 4])  # 5 taps: past the tile's 4
deconv("g2_concat_skip", D, (2, 8, *P57), 3, (2, 2), [DIRECT, "k_copy_rows<"], s=(2, 2), group=2,
       chain=[("Concat", (x(2, 5, 10, 14), ("prev",)), {"axis": 1}, WHOLE)])

# ---- stride 1: the Conv it equals (pads' = d (k - 1) - pads), or the direct form -------
S = "deconv_s1"
deconv("s1_k3_p1_6_5", S, (2, 6, *P57), 5, (3, 3), [OC.small(False, 16, False)], pads=[1, 1, 1, 1])
deconv("s1_k5_p2_3_4", S, (2, 3, *P57), 4, (5, 5), [OC.small(False, 32, False)], pads=[2, 2, 2, 2], chain=[then("Relu")])
deconv("s1_k3_p0_g4_8_12", S, (2, 8, *P57), 3, (3, 3), [OC.small(False, 8, False)], group=4)
deconv("s1_k3_dil2_pads1021", S, (2, 6, *P57), 5, (3, 3), [OC.small(False, 16, False)], dilations=[2, 2], pads=[1, 0, 2, 1])
deconv("s1_k3_p3_negative", S, (2, 6, 6, 9), 5, (3, 3), [DIRECT], pads=[3, 3, 3, 3])

# ---- HardSigmoid / HardSwish / ReduceMean -----------------------------------------------
A = "hard"
X = (2, 3, 10, 11)
PM80 = ("pm80", X)


def act(name, op, inputs, attrs=None, **kw):
    case(name, kw.pop("family", A), op, inputs, attrs, opset=kw.pop("opset", 14), **kw)


UNARY, CONV1 = ("k_unary(",), ("k_conv",)
act("HardSigmoid", "HardSigmoid", [x(*X)], kernels=UNARY)
act("HardSigmoid_pm80", "HardSigmoid", [PM80], kernels=UNARY)
act("HardSigmoid_alpha_beta", "HardSigmoid", [("x4", X)], {"alpha": 0.3, "beta": 0.4}, kernels=UNARY)
act("HardSwish", "HardSwish", [("x4", X)], kernels=UNARY)
act("HardSwish_pm80", "HardSwish", [PM80], kernels=UNARY)
_pw = [x(2, 6, 9, 11), _c((5, 6, 1, 1), 6 ** -0.5 * 3), bias(5)]  # (outputs of +-3: both clamps bind)
act("Conv_HardSigmoid", "Conv", _pw, kernels=CONV1, chain=[then("HardSigmoid", alpha=0.25, beta=0.45)])
act("Conv_HardSwish", "Conv", _pw, kernels=CONV1, chain=[then("HardSwish")])
act("Gemm_HardSwish", "Gemm", [x(5, 8), x(8, 7)], kernels=("k_gemm",), chain=[then("HardSwish")])
# the hard-swish of exports before opset 14: one activation behind its producer, or one k_unary launch
act("Conv_Mul_HardSigmoid", "Conv", _pw, kernels=CONV1,
    chain=[then("HardSigmoid", alpha=1 / 6, beta=0.5), ("Mul", (("node", 0), ("prev",)), {}, WHOLE)])
act("Conv_Mul_HardSigmoid_alpha_beta", "Conv", _pw, kernels=CONV1,
    chain=[then("HardSigmoid", alpha=0.3, beta=0.4), ("Mul", (("prev",), ("node", 0)), {}, WHOLE)])
act("Mul_HardSigmoid_of_input", "HardSigmoid", [("x4", X)], kernels=UNARY,
    chain=[("Mul", (("in", 0), ("prev",)), {}, WHOLE)])
# the HardSigmoid has a second consumer (it is a graph output): three launches, the same values
act("Conv_Mul_HardSigmoid_second_consumer", "Conv", _pw, n_out=2, kernels=CONV1 + UNARY + ("k_binary",),
    chain=[("HardSigmoid", (), {}, {"out": True}), ("Mul", (("node", 0), ("prev",)), {}, WHOLE)])
GAP = ("k_gap",)
act("ReduceMean_23_keep", "ReduceMean", [x(*X)], {"axes": [2, 3], "keepdims": 1}, kernels=GAP)
act("ReduceMean_23_drop", "ReduceMean", [x(*X)], {"axes": [2, 3], "keepdims": 0}, kernels=GAP)
act("ReduceMean_neg_default_keep", "ReduceMean", [x(*X)], {"axes": [-2, -1]}, kernels=GAP)
act("ReduceMean_neg_drop_pm80", "ReduceMean", [PM80], {"axes": [-1, -2], "keepdims": 0}, kernels=GAP)
act("ReduceMean_1025", "ReduceMean", [x(1, 5, 25, 41)], {"axes": [2, 3]}, kernels=GAP)
act("ReduceMean_input_23_drop", "ReduceMean", [x(*X), ci(2, 3)], {"keepdims": 0}, kernels=GAP, family="hard18", opset=18)
act("ReduceMean_input_neg_keep", "ReduceMean", [PM80, ci(-2, -1)], kernels=GAP, family="hard18", opset=18)
act("ReduceMean_noop_empty_axes", "ReduceMean", [x(*X)], {"noop_with_empty_axes": 1}, family="hard18", opset=18,
    exact=True)

# ---- refused at creation ----------------------------------------------------------------
R_ = "refused"
W22 = dw(6, 5, (2, 2), (2, 2))


def refuse(name, op, inputs, attrs=None, opset=14):
    case(f"refuse_{name}", R_, op, inputs, attrs, expect="refused", opset=opset)


refuse("ConvTranspose_runtime_weights", "ConvTranspose", [x(2, 6, *P57), x(6, 5, 2, 2)], {"strides": [2, 2]})
refuse("ConvTranspose_channels", "ConvTranspose", [x(2, 7, *P57), W22], {"strides": [2, 2]})
refuse("ConvTranspose_group", "ConvTranspose", [x(2, 6, *P57), W22], {"strides": [2, 2], "group": 4})
refuse("ConvTranspose_output_padding_eq_stride", "ConvTranspose", [x(2, 6, *P57), W22],
       {"strides": [2, 2], "output_padding": [2, 0]})
refuse("ConvTranspose_output_padding_eq_dilation", "ConvTranspose", [x(2, 6, *P57), W22],
       {"strides": [2, 2], "dilations": [3, 3], "output_padding": [0, 3]})
refuse("ConvTranspose_output_shape_beyond", "ConvTranspose", [x(2, 6, *P57), W22],
       {"strides": [2, 2], "output_shape": [11, 14]})
refuse("ConvTranspose_strides_1", "ConvTranspose", [x(2, 6, *P57), W22], {"strides": [2]})
refuse("ConvTranspose_dilations_3", "ConvTranspose", [x(2, 6, *P57), W22], {"dilations": [1, 1, 1]})
refuse("ConvTranspose_pads_2", "ConvTranspose", [x(2, 6, *P57), W22], {"strides": [2, 2], "pads": [1, 1]})
refuse("ConvTranspose_output_padding_1", "ConvTranspose", [x(2, 6, *P57), W22], {"strides": [2, 2], "output_padding": [1]})
refuse("ConvTranspose_output_shape_4", "ConvTranspose", [x(2, 6, *P57), W22],
       {"strides": [2, 2], "output_shape": [2, 5, 10, 14]})
refuse("ConvTranspose_empty_output", "ConvTranspose", [x(2, 6, *P57), W22], {"pads": [3, 3, 3, 3]})
refuse("ConvTranspose_rank3", "ConvTranspose", [x(2, 6, 7), _c((6, 5, 2), 0.3)], {"strides": [2]})
refuse("ReduceMean_axis1", "ReduceMean", [x(*X)], {"axes": [1]})
refuse("ReduceMean_axis3", "ReduceMean", [x(*X)], {"axes": [3]})
refuse("ReduceMean_axes123", "ReduceMean", [x(*X)], {"axes": [1, 2, 3]})
refuse("ReduceMean_all_axes", "ReduceMean", [x(*X)], {"keepdims": 0})
refuse("ReduceMean_rank3", "ReduceMean", [x(2, 3, 17)], {"axes": [1, 2]})
refuse("ReduceMean_input_axis0", "ReduceMean", [x(*X), ci(0, 2, 3)], opset=18)

# the explicit pads an auto_pad / output_shape case must equal (worked out by hand from the operator text)
EXPLICIT_PADS = {
    "ConvTranspose_k3s2_same_upper_16_16": [0, 0, 1, 1],
    "ConvTranspose_k3s2_same_lower_16_16": [1, 1, 0, 0],
    "ConvTranspose_k3s2_output_shape_16_16": [1, 1, 0, 1],
}

VALUE_CASES = [k for k in CASES if k.expect == "value"]
REFUSED_CASES = [k for k in CASES if k.expect == "refused"]
BY_NAME = {k.name: k for k in CASES}


def groups():
    """{family: its value cases}; a family has one opset, so one model holds it."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    for fam, ks in out.items():
        assert len({k.opset for k in ks}) == 1, fam
    return out
