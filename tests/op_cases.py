"""The operator conformance matrix of the ONNX sessions (test infrastructure):
one table of named single-operator cases, shared by
tests/test_op_matrix_oracle.py (the oracle against an independent float64
evaluation, CPU) and tests/test_gpu_op_matrix.py (the GPU session against the
oracle).

A case is one operator node (the conv family: with the nodes a session fuses
behind it, `chain`; the ir family: one inverted-residual block, a chain whose
nodes may name the case's input or each other; the inorm / ibn families: InstanceNormalization alone, or
MODNet's IBNorm pattern with its consumer): its attributes, its inputs in operator order
(graph inputs filled from a seeded generator, or constants where the operator
needs them constant), the model's opset, and whether the session must compute
it ("value") or refuse it at creation ("refused").  build() packs any number
of cases into one model with one graph output per case output, so one GPU
session serves a whole family; every operand that should reach a kernel is a
graph input (constant folding cannot eat a case).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

import onnx_models as M
import onnx_ref as R

I64 = np.int64
INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    op: str
    # per operator input: ("x", shape) standard normal | ("pos", shape) in [0.5, 1.5) |
    # ("pm80", shape) +-80 plus a standard normal | ("c", array) a constant | None (omitted)
    inputs: tuple
    attrs: dict = field(default_factory=dict)
    seed: int = 0
    opset: int = 13
    expect: str = "value"   # or "refused"
    exact: bool = False     # data movement / selection: bitwise
    n_out: int = 1
    post: tuple = ()        # ("PRelu", slope array): a second node on the output (the fused forms)
    kernels: tuple = ()     # what a session of this case alone launches (a part of each name, in order)
    # further nodes, each on the output of the one before: (op, its further inputs (as `inputs`), attributes);
    # the last one's output is the case's (the conv family's pairs and epilogues)
    chain: tuple = ()
    # a chain operand may also be ("in", k): the case's own input k, or ("node", j): the output of the case's
    # node j (0: its operator, j: chain[j - 1]).  A chain node may carry a fourth element, {"whole": its
    # inputs are all listed, ("prev",) standing for the node before; "out": its output is one more graph
    # output of the case, ahead of the last node's; "n": it has that many outputs, ("node", j, q) its q-th}.
    # Further input kinds (the norm families): "ramp", "off100", "small", "half"; "q8" (the fusion matrix) — see _generate.
    kernels16: tuple = ()   # `kernels` of a bf16 / f16 session (the ir family, whose fused forms differ by precision)
    echo: bool = False      # the case's input 0 is a graph output too (the first of the case's)
    op_out: bool = False    # the operator's own output (node 0 of a chain) is a graph output too (behind echo's)


CASES: list[Case] = []


def case(name, family, op, inputs, attrs=None, **kw):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), **kw))


def x(*shape):
    return ("x", tuple(shape))


def pos(*shape):
    return ("pos", tuple(shape))


def c(arr, dtype=None):
    return ("c", np.asarray(arr, dtype))


def ci(*v):
    return ("c", np.asarray(v, I64))


def cf(shape, seed, lo=None):
    """A seeded float32 constant: standard normal, or uniform in [lo, lo + 1)."""
    rng = np.random.default_rng(1000 + seed)
    a = rng.standard_normal(shape) if lo is None else rng.random(shape) + lo
    return ("c", a.astype(np.float32))


def wf(shape, seed, fan_in=None):
    """A seeded float32 constant of the ir family: a weight, standard normal / sqrt(fan_in), or a bias
    (no fan_in), 0.1 * standard normal."""
    a = np.random.default_rng(2000 + seed).standard_normal(shape) * (0.1 if fan_in is None else fan_in ** -0.5)
    return ("c", a.astype(np.float32))


def _tag(v):
    return "x".join(str(k) for k in v) if isinstance(v, (tuple, list)) else str(v)


X = (2, 3, 10, 11)

# ---------------------------------------------------------------------------
# MaxPool / AveragePool (k_pool)
for op_ in ("MaxPool", "AveragePool"):
    for k_ in (2, 3, (2, 3)):
        for s_ in (1, 2, (2, 1)):
            for p_ in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0)):
                for ceil_ in (0, 1):
                    for cip_ in ((0, 1) if op_ == "AveragePool" else (None,)):
                        kk = list(k_) if isinstance(k_, tuple) else [k_, k_]
                        ss = list(s_) if isinstance(s_, tuple) else [s_, s_]
                        at = {"kernel_shape": kk, "strides": ss, "pads": list(p_), "ceil_mode": ceil_}
                        nm = f"{op_}_k{_tag(k_)}_s{_tag(s_)}_p{''.join(map(str, p_))}_ceil{ceil_}"
                        if cip_ is not None:
                            at["count_include_pad"] = cip_
                            nm += f"_cip{cip_}"
                        case(nm, "pool", op_, [x(*X)], at, exact=op_ == "MaxPool")
for k_ in (2, 3):
    for s_ in (1, 2):
        for p_ in (0, 1):
            for ceil_ in (0, 1):
                case(f"MaxPool_dil2_k{k_}_s{s_}_p{p_}_ceil{ceil_}", "pool", "MaxPool", [x(*X)],
                     {"kernel_shape": [k_, k_], "strides": [s_, s_], "pads": [p_] * 4, "dilations": [2, 2],
                      "ceil_mode": ceil_}, exact=True)
for ap_ in ("SAME_UPPER", "SAME_LOWER", "VALID"):
    case(f"MaxPool_{ap_}", "pool", "MaxPool", [x(*X)], {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": ap_},
         exact=True)
    for cip_ in (0, 1):
        case(f"AveragePool_{ap_}_cip{cip_}", "pool", "AveragePool", [x(*X)],
             {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": ap_, "count_include_pad": cip_})
case("AveragePool_default_strides", "pool", "AveragePool", [x(*X)], {"kernel_shape": [2, 2]})

# ---------------------------------------------------------------------------
# Resize / Upsample (k_resize<true>: rows of a multiple of 4 outputs; <false>: the rest)
RX = (2, 3, 10, 12)
CTMS = ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric")


def _resize_inputs(scale=None, sizes=None):
    if sizes is not None:
        return [x(*RX), None, None, ci(RX[0], RX[1], *sizes)]
    return [x(*RX), None, c([1, 1, scale, scale], np.float32)]


for ctm_ in CTMS:
    for sc_ in (2.0, 0.5, 1.5):  # 20x24 (float4 rows), 5x6, 15x18
        case(f"Resize_linear_{ctm_}_x{sc_}", "resize", "Resize", _resize_inputs(scale=sc_),
             {"mode": "linear", "coordinate_transformation_mode": ctm_},
             kernels=("k_resize<true>(" if int(RX[3] * sc_) % 4 == 0 else "k_resize<false>(",))
    for sz_ in ((7, 13), (5, 16), (1, 8), (9, 1)):
        case(f"Resize_linear_{ctm_}_to{_tag(sz_)}", "resize", "Resize", _resize_inputs(sizes=sz_),
             {"mode": "linear", "coordinate_transformation_mode": ctm_})
for nm_ in ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil"):
    for ctm_ in ("asymmetric", "half_pixel"):
        for sc_ in (2.0, 0.5, 1.5):
            case(f"Resize_nearest_{nm_}_{ctm_}_x{sc_}", "resize", "Resize", _resize_inputs(scale=sc_),
                 {"mode": "nearest", "coordinate_transformation_mode": ctm_, "nearest_mode": nm_}, exact=True)
        for sz_ in ((7, 13), (25, 16)):
            case(f"Resize_nearest_{nm_}_{ctm_}_to{_tag(sz_)}", "resize", "Resize", _resize_inputs(sizes=sz_),
                 {"mode": "nearest", "coordinate_transformation_mode": ctm_, "nearest_mode": nm_}, exact=True)
case("Resize_nearest_defaults_x2", "resize", "Resize", _resize_inputs(scale=2.0), {}, exact=True)
case("Upsample_nearest_x2x3", "resize9", "Upsample", [x(*RX), c([1, 1, 2, 3], np.float32)], {"mode": "nearest"},
     opset=9, exact=True)
case("Upsample_nearest_x1.5", "resize9", "Upsample", [x(*RX), c([1, 1, 1.5, 1.5], np.float32)], {"mode": "nearest"},
     opset=9, exact=True)
case("Upsample_linear_x2", "resize9", "Upsample", [x(*RX), c([1, 1, 2, 2], np.float32)], {"mode": "linear"}, opset=9)
case("Upsample_linear_x1.5", "resize9", "Upsample", [x(*RX), c([1, 1, 1.5, 1.5], np.float32)], {"mode": "linear"},
     opset=9)

# ---------------------------------------------------------------------------
# standalone activations (k_unary; PRelu: k_binary)
case("Relu", "unary", "Relu", [x(*X)], exact=True)
case("LeakyRelu_default", "unary", "LeakyRelu", [x(*X)])
case("LeakyRelu_alpha0.2", "unary", "LeakyRelu", [x(*X)], {"alpha": 0.2})
case("Sigmoid", "unary", "Sigmoid", [("x4", X)])
case("Tanh", "unary", "Tanh", [("x4", X)])
case("Clip_min_max", "unary", "Clip", [x(*X), c(-0.5, np.float32), c(0.75, np.float32)], exact=True)
case("Clip_min_only", "unary", "Clip", [x(*X), c(-0.25, np.float32)], exact=True)
case("Clip_max_only", "unary", "Clip", [x(*X), None, c(0.5, np.float32)], exact=True)
case("Clip_none", "unary", "Clip", [x(*X)], exact=True)
case("Clip_attr_min_only", "unary6", "Clip", [x(*X)], {"min": -0.25}, opset=6, exact=True)
case("Clip_attr_max_only", "unary6", "Clip", [x(*X)], {"max": 0.5}, opset=6, exact=True)
case("PRelu_C11", "unary", "PRelu", [x(*X), cf((3, 1, 1), 1)])
case("PRelu_1C11", "unary", "PRelu", [x(*X), cf((1, 3, 1, 1), 2)])
case("PRelu_scalar", "unary", "PRelu", [x(*X), cf((1,), 3)])
case("PRelu_W_1d", "unary", "PRelu", [x(*X), cf((11,), 4)])
# a 1-D slope aligns with W, also where C == W (here both 4): not per channel
case("PRelu_1d_C_equals_W", "unary", "PRelu", [x(2, 4, 5, 4), cf((4,), 5)])
case("PRelu_runtime_slope", "unary", "PRelu", [x(*X), x(3, 1, 1)])
# behind a convolution: [C,1,1] in the epilogue, [C] (C == W) aligned with W by its own launch
case("ConvPRelu_C11", "fused", "Conv", [x(1, 3, 6, 4), cf((4, 3, 3, 3), 6), cf((4,), 7)],
     {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, post=("PRelu", cf((4, 1, 1), 8)[1]), kernels=("k_conv",))
case("ConvPRelu_1d_C_equals_W", "fused", "Conv", [x(1, 3, 6, 4), cf((4, 3, 3, 3), 6), cf((4,), 7)],
     {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, post=("PRelu", cf((4,), 9)[1]), kernels=("k_conv", "k_binary("))

# ---------------------------------------------------------------------------
# Add / Sub / Mul / Div (k_binary; a per-plane operand on contiguous planes: k_binary_planes)
for op_ in ("Add", "Sub", "Mul", "Div"):
    d_ = pos if op_ == "Div" else x
    case(f"{op_}_same_shape", "binary", op_, [x(*X), d_(*X)])
    case(f"{op_}_both_broadcast", "binary", op_, [x(2, 1, 10, 1), d_(1, 3, 1, 11)])
    case(f"{op_}_rank5", "binary", op_, [x(2, 1, 3, 1, 5), d_(1, 4, 1, 2, 5)])
    case(f"{op_}_rank6", "binary", op_, [x(2, 1, 2, 1, 3, 1), d_(1, 3, 1, 2, 1, 4)])
    case(f"{op_}_lower_rank", "binary", op_, [x(*X), d_(11)])
    case(f"{op_}_lower_rank_left", "binary", op_, [x(10, 1), d_(*X)])
    case(f"{op_}_planes", "binary", op_, [x(2, 3, 4, 6), d_(2, 3, 1, 1)], kernels=("k_binary_planes(",))
    case(f"{op_}_planes_odd", "binary", op_, [x(2, 3, 3, 5), d_(2, 3, 1, 1)], kernels=("k_binary(",))
    case(f"{op_}_const_right", "binary", op_, [x(*X), cf((3, 1, 1), 11, lo=0.5)])
    case(f"{op_}_const_left", "binary", op_, [cf((3, 1, 1), 12, lo=0.5), d_(*X)])
    case(f"{op_}_scalar_const_left", "binary", op_, [c(1.5, np.float32), d_(*X)])

# ---------------------------------------------------------------------------
# Slice (k_copy; whole trailing dims: k_copy_rows)
case("Slice_reverse_W", "slice", "Slice", [x(*X), ci(-1), ci(INT64_MIN), ci(3), ci(-1)], exact=True)
case("Slice_step-2", "slice", "Slice", [x(*X), ci(8), ci(1), ci(2), ci(-2)], exact=True)
case("Slice_step-3_past_both_ends", "slice", "Slice", [x(*X), ci(INT64_MAX), ci(INT64_MIN), ci(-1), ci(-3)], exact=True)
case("Slice_negative_indices", "slice", "Slice", [x(*X), ci(-7), ci(-2), ci(-2)], exact=True)
case("Slice_end_max", "slice", "Slice", [x(*X), ci(1, 4), ci(INT64_MAX, INT64_MAX), ci(1, 3)], exact=True)
case("Slice_steps_2_3", "slice", "Slice", [x(*X), ci(1, 0), ci(9, 11), ci(2, 3), ci(2, 3)], exact=True)
case("Slice_default_axes", "slice", "Slice", [x(*X), ci(0, 1), ci(2, 3)], exact=True)
case("Slice_steps_without_axes", "slice", "Slice", [x(*X), ci(1, 0), ci(2, 3), None, ci(1, 2)], exact=True)
case("Slice_channels", "slice", "Slice", [x(2, 4, 10, 12), ci(1), ci(3), ci(1)], exact=True,
     kernels=("k_copy_rows<true>(",))
case("Slice_batch_odd", "slice", "Slice", [x(*X), ci(1), ci(2), ci(0)], exact=True,
     kernels=("k_copy_rows<false>(",))
case("Slice_attr_form", "slice9", "Slice", [x(*X)], {"starts": [1, -6], "ends": [3, INT64_MAX], "axes": [1, 3]},
     opset=9, exact=True)

# ---------------------------------------------------------------------------
# Concat / Split (k_copy_rows<true>: 16-byte moves; <false>; k_copy)
case("Concat_axis0", "concat", "Concat", [x(1, 3, 10, 11), x(2, 3, 10, 11), x(1, 3, 10, 11)], {"axis": 0}, exact=True,
     kernels=("k_copy_rows<false>(",) * 3)
case("Concat_axis1_vec", "concat", "Concat", [x(2, 1, 10, 12), x(2, 2, 10, 12), x(2, 3, 10, 12)], {"axis": 1},
     exact=True, kernels=("k_copy_rows<true>(",) * 3)
case("Concat_axis1_odd", "concat", "Concat", [x(2, 1, 10, 11), x(2, 2, 10, 11), x(2, 3, 10, 11)], {"axis": 1},
     exact=True, kernels=("k_copy_rows<false>(",) * 3)
case("Concat_axis2", "concat", "Concat", [x(2, 3, 1, 11), x(2, 3, 4, 11), x(2, 3, 2, 11)], {"axis": 2}, exact=True,
     kernels=("k_copy(",) * 3)
case("Concat_axis-1", "concat", "Concat", [x(2, 3, 10, 1), x(2, 3, 10, 5), x(2, 3, 10, 3)], {"axis": -1}, exact=True,
     kernels=("k_copy(",) * 3)
case("Concat_rank2_axis-1", "concat", "Concat", [x(3, 5), x(3, 1), x(3, 2)], {"axis": -1}, exact=True)
case("Split_sizes_input", "split", "Split", [x(2, 7, 4, 5), ci(1, 4, 2)], {"axis": 1}, n_out=3, exact=True)
case("Split_sizes_W", "split", "Split", [x(*X), ci(5, 6)], {"axis": -1}, n_out=2, exact=True)
case("Split_default_even", "split", "Split", [x(2, 6, 4, 5)], {"axis": 1}, n_out=3, exact=True)
case("Split_default_axis", "split", "Split", [x(4, 3, 5)], {}, n_out=2, exact=True)
case("Split_sizes_attr", "split11", "Split", [x(2, 7, 4, 5)], {"axis": 1, "split": [3, 4]}, n_out=2, opset=11,
     exact=True)
case("Split_default_uneven", "split18", "Split", [x(2, 7, 4, 5)], {"axis": 1, "num_outputs": 3}, n_out=3, opset=18,
     exact=True)
case("Split_default_uneven_W", "split18", "Split", [x(2, 3, 4, 10)], {"axis": 3, "num_outputs": 4}, n_out=4, opset=18,
     exact=True)
case("Split_default_even_18", "split18", "Split", [x(2, 6, 4, 5)], {"axis": 1, "num_outputs": 2}, n_out=2, opset=18,
     exact=True)

# ---------------------------------------------------------------------------
# Transpose / Pad (k_copy)
case("Transpose_default_rank4", "move", "Transpose", [x(*X)], exact=True)
case("Transpose_default_rank3", "move", "Transpose", [x(3, 5, 7)], exact=True)
case("Transpose_default_rank2", "move", "Transpose", [x(5, 7)], exact=True)
case("Transpose_nhwc", "move", "Transpose", [x(*X)], {"perm": [0, 2, 3, 1]}, exact=True)
case("Transpose_rank5", "move", "Transpose", [x(2, 3, 4, 5, 6)], {"perm": [4, 0, 3, 1, 2]}, exact=True)
case("Pad_value", "move", "Pad", [x(*X), ci(0, 1, 2, 0, 0, 0, 1, 3), c(0.5, np.float32)], exact=True)
case("Pad_default_value", "move", "Pad", [x(*X), ci(0, 0, 1, 1, 0, 0, 1, 1)], exact=True)
case("Pad_negative", "move", "Pad", [x(*X), ci(0, 0, -2, -1, 0, -1, -3, 0)], exact=True)
case("Pad_mixed_sign", "move", "Pad", [x(*X), ci(0, 0, -2, 3, 0, 1, 2, -4), c(-1.0, np.float32)], exact=True)
case("Pad_axes", "move18", "Pad", [x(*X), ci(1, 2, 3, 0), c(2.0, np.float32), ci(3, 1)], opset=18, exact=True)
case("Pad_negative_axes", "move18", "Pad", [x(*X), ci(2, -3, -1, 1), None, ci(-1, -2)], opset=18, exact=True)
case("Pad_attr_form", "move9", "Pad", [x(*X)], {"pads": [0, 0, 1, 2, 0, 1, 0, 0], "value": 0.25}, opset=9, exact=True)

# ---------------------------------------------------------------------------
# the view ops (no launch: the output is the input's buffer)
case("Squeeze_axes_input", "view", "Squeeze", [x(2, 1, 5, 1), ci(1, -1)], exact=True)
case("Squeeze_all", "view", "Squeeze", [x(2, 1, 5, 1)], exact=True)
case("Unsqueeze_axes_input", "view", "Unsqueeze", [x(2, 5), ci(0, 3)], exact=True)
case("Unsqueeze_negative_axes", "view", "Unsqueeze", [x(2, 5), ci(-1, 1)], exact=True)
case("Squeeze_axes_attr", "view11", "Squeeze", [x(2, 1, 5, 1)], {"axes": [1, 3]}, opset=11, exact=True)
case("Unsqueeze_axes_attr", "view11", "Unsqueeze", [x(2, 5)], {"axes": [0, 3]}, opset=11, exact=True)
case("Flatten_axis0", "view", "Flatten", [x(*X)], {"axis": 0}, exact=True)
case("Flatten_axis2", "view", "Flatten", [x(*X)], {"axis": 2}, exact=True)
case("Flatten_axis-1", "view", "Flatten", [x(*X)], {"axis": -1}, exact=True)
case("Flatten_default", "view", "Flatten", [x(*X)], exact=True)
case("Reshape_0_-1", "view", "Reshape", [x(*X), ci(0, -1, 11)], exact=True)
case("Reshape_-1_first", "view", "Reshape", [x(*X), ci(-1, 0, 5, 2, 11)], exact=True)
case("Reshape_plain", "view", "Reshape", [x(*X), ci(6, 110)], exact=True)

# ---------------------------------------------------------------------------
# Gemm / MatMul (k_gemm<true>: both operands contiguous in k, K % 4 == 0; <false>: the rest)
case("Gemm_plain", "gemm", "Gemm", [x(5, 8), x(8, 7)], kernels=("k_gemm<false>(",))
case("Gemm_transB_vec", "gemm", "Gemm", [x(5, 8), x(7, 8), x(7)], {"transB": 1}, kernels=("k_gemm<true>(",))
case("Gemm_transB_K6", "gemm", "Gemm", [x(5, 6), x(7, 6), x(7)], {"transB": 1}, kernels=("k_gemm<false>(",))
case("Gemm_transA", "gemm", "Gemm", [x(8, 5), x(8, 7), x(5, 7)], {"transA": 1}, kernels=("k_gemm<false>(",))
case("Gemm_transA_transB", "gemm", "Gemm", [x(8, 5), x(7, 8), x(1, 7)], {"transA": 1, "transB": 1})
case("Gemm_alpha_beta", "gemm", "Gemm", [x(5, 8), x(8, 7), x(5, 7)], {"alpha": 0.5, "beta": -1.5})
case("Gemm_alpha_only", "gemm", "Gemm", [x(5, 8), x(8, 7)], {"alpha": 2.5})
case("Gemm_C_M1", "gemm", "Gemm", [x(5, 8), x(8, 7), x(5, 1)], {"beta": 0.75})
case("Gemm_C_1N", "gemm", "Gemm", [x(5, 8), x(8, 7), x(1, 7)])
case("Gemm_C_1", "gemm", "Gemm", [x(5, 8), x(8, 7), x(1)])
case("Gemm_C_11", "gemm", "Gemm", [x(5, 8), x(8, 7), x(1, 1)])
case("Gemm_C_const", "gemm", "Gemm", [x(5, 8), x(8, 7), cf((7,), 21)])
case("Gemm_tiles", "gemm", "Gemm", [x(18, 37), x(37, 33), x(18, 1)], {"alpha": 0.5})
case("Gemm_tiles_vec", "gemm", "Gemm", [x(18, 68), x(33, 68), x(33)], {"transB": 1},
     kernels=("k_gemm<true>(",))
case("MatMul_2d", "gemm", "MatMul", [x(5, 8), x(8, 7)])
case("MatMul_batch_broadcast_B2d", "gemm", "MatMul", [x(2, 3, 4, 5), x(5, 7)])
case("MatMul_batch_broadcast_B1", "gemm", "MatMul", [x(2, 4, 8), x(1, 8, 7)])
case("MatMul_batched_B", "gemm", "MatMul", [x(2, 3, 4, 8), x(2, 3, 8, 7)])
case("MatMul_const_B", "gemm", "MatMul", [x(2, 4, 8), cf((8, 7), 22)], kernels=("k_gemm<true>(",))
case("MatMul_const_B_K6", "gemm", "MatMul", [x(2, 4, 6), cf((6, 7), 23)], kernels=("k_gemm<false>(",))

# ---------------------------------------------------------------------------
# BatchNormalization alone (k_affine), InstanceNormalization, GlobalAveragePool, Softmax
for shp_ in ((4, 5), (2, 5, 7), (2, 5, 3, 4), (2, 5, 2, 3, 2)):
    case(f"BatchNormalization_rank{len(shp_)}", "norm", "BatchNormalization",
         [x(*shp_), cf((5,), 31, lo=0.5), cf((5,), 32), cf((5,), 33), cf((5,), 34, lo=0.5)], {"epsilon": 1e-3},
         kernels=("k_affine(",))
case("BatchNormalization_default_eps", "norm", "BatchNormalization",
     [x(2, 5, 3, 4), cf((5,), 31, lo=0.5), cf((5,), 32), cf((5,), 33), cf((5,), 34, lo=0.5)])
for shp_ in ((2, 3, 1, 1), (2, 3, 1, 3), (1, 2, 15, 17), (1, 2, 16, 16), (1, 2, 1, 257), (2, 3, 257), (2, 3, 33, 40)):
    case(f"InstanceNormalization_{_tag(shp_)}", "norm", "InstanceNormalization",
         [("x3", shp_), cf((shp_[1],), 35, lo=0.5), cf((shp_[1],), 36)], {"epsilon": 1e-5})
case("GlobalAveragePool_1024", "gap", "GlobalAveragePool", [x(1, 3, 32, 32)], kernels=("k_gap_wave(",))
case("GlobalAveragePool_1025", "gap", "GlobalAveragePool", [x(1, 5, 25, 41)], kernels=("k_gap(",))
case("GlobalAveragePool_rows6", "gap", "GlobalAveragePool", [x(*X)], kernels=("k_gap_wave(",))
case("GlobalAveragePool_1x1", "gap", "GlobalAveragePool", [x(3, 3, 1, 1)])
case("GlobalAveragePool_rank3", "gap", "GlobalAveragePool", [x(2, 3, 17)])
for n_ in (1, 255, 256, 257, 1000):
    case(f"Softmax_{n_}", "softmax", "Softmax", [x(3, n_)])
    case(f"Softmax_{n_}_pm80", "softmax", "Softmax", [("pm80", (3, n_))])
case("Softmax_rank3", "softmax", "Softmax", [x(2, 3, 5)], {"axis": -1})
case("Softmax_rank4_axis3", "softmax", "Softmax", [x(2, 3, 4, 5)], {"axis": 3})
# before opset 13: flattened to 2-D at `axis` (default 1), each row normalised
case("Softmax_opset11_default_axis_rank3", "softmax11", "Softmax", [x(2, 3, 5)], opset=11)
case("Softmax_opset11_axis1_rank4", "softmax11", "Softmax", [x(2, 3, 4, 5)], {"axis": 1}, opset=11)
case("Softmax_opset11_axis0", "softmax11", "Softmax", [x(3, 5)], {"axis": 0}, opset=11)
case("Softmax_opset11_axis-1", "softmax11", "Softmax", [x(2, 3, 5)], {"axis": -1}, opset=11)

# ---------------------------------------------------------------------------
# Conv: every kernel form launch_conv / conv_kernel_name (vso_kernels.hip) and
# plan_conv (vso_plan.hip) choose but k_conv_tile in f32 (tests/test_gpu_conv_tile_matrix.py),
# one Conv per case (or a depthwise -> 1x1 pair, or a Conv with its epilogue),
# the name of its launch asserted.  Batch 2, planes 9x11 (99 outputs: a pixel
# tile tail on every tile size) and channel counts off the 16 / 64 tiles unless
# a form's own threshold asks for more.  K = Cg * kh * kw.  In f32 a dense
# square 3x3 / 5x5 stride-1 or 3x3 stride-2 case stays below 8e6 MACs (above,
# it is k_conv_tile's); in a 16-bit session those cases run on k_conv_tile
# whatever their size (onnx_ref.tiled_conv), every other case as in f32.
_conv_seed = [100]


def _cw(*shape):
    _conv_seed[0] += 1
    return cf(shape, _conv_seed[0])


def small(pw, ch, split):
    return f"k_conv_small<{str(pw).lower()}, {ch}, {str(split).lower()}>("


def then(op_, *ins, **attrs):
    return (op_, tuple(ins), attrs)


def conv(name, xs, ws, attrs=None, kernels=(), bias=True, chain=()):
    """One Conv of a graph input `xs` with constant weights `ws` (and a bias), then `chain`."""
    case(f"Conv_{name}", "conv", "Conv", [x(*xs), _cw(*ws)] + ([_cw(ws[0])] if bias else []), attrs,
         kernels=tuple(kernels), chain=tuple(chain))


def pw_after(c_, m_, bias=True):
    """The 1x1 Conv of a depthwise -> 1x1 pair."""
    return then("Conv", _cw(m_, c_, 1, 1), *([_cw(m_)] if bias else []))


CLIP6 = then("Clip", c(0.0, np.float32), c(6.0, np.float32))
P9 = (9, 11)

# k_conv_small<false, 8 | 16 | 32, false> (K <= 32 | 64 | 128) and <false, 16, true> (K > 128: four
# waves, ceil(K / 16) * 4 of K each); A operands as float4 where K % 4 == 0, else one by one
conv("small_K27", (2, 3, *P9), (5, 3, 3, 3), {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, [small(False, 8, False)])
conv("small_K27_s2x1", (2, 3, *P9), (17, 3, 3, 3), {"strides": [2, 1], "pads": [1, 1, 1, 1]}, [small(False, 8, False)])
conv("small_K32_2x2", (2, 8, *P9), (17, 8, 2, 2), {"kernel_shape": [2, 2], "pads": [1, 0, 0, 1]},
     [small(False, 8, False)])
conv("small_K21_1x7", (2, 3, *P9), (16, 3, 1, 7), {"kernel_shape": [1, 7], "pads": [0, 3, 0, 2]},
     [small(False, 8, False)])
conv("small_K28_7x1_s2x1", (2, 4, *P9), (20, 4, 7, 1), {"strides": [2, 1], "pads": [3, 0, 3, 0]},
     [small(False, 8, False)])
conv("small_K36_s2", (2, 4, *P9), (17, 4, 3, 3), {"strides": [2, 2], "pads": [1, 1, 1, 1]}, [small(False, 16, False)])
conv("small_K63_dil2x1", (2, 7, *P9), (5, 7, 3, 3), {"dilations": [2, 1], "pads": [2, 1, 2, 1]},
     [small(False, 16, False)])
conv("small_K64_2x2_nobias", (2, 16, *P9), (20, 16, 2, 2), {"kernel_shape": [2, 2]}, [small(False, 16, False)],
     bias=False)
conv("small_K45_3x5_dil1x3", (2, 3, *P9), (16, 3, 3, 5), {"dilations": [1, 3], "pads": [1, 6, 1, 6]},
     [small(False, 16, False)])
# pads of the kernel's extent: the outputs of the outermost ring see no input, they equal the bias
conv("small_K72_pads3", (2, 8, *P9), (20, 8, 3, 3), {"pads": [3, 3, 3, 3]}, [small(False, 32, False)])
conv("small_K128_2x2_s2", (2, 32, *P9), (17, 32, 2, 2), {"strides": [2, 2]}, [small(False, 32, False)])
conv("small_K75_5x5", (2, 3, *P9), (5, 3, 5, 5), {"pads": [2, 2, 2, 2]}, [small(False, 32, False)])
conv("small_K98_7x7", (2, 2, *P9), (16, 2, 7, 7), {"pads": [3, 3, 3, 3]}, [small(False, 32, False)])
conv("small_K132_2x2", (2, 33, *P9), (20, 33, 2, 2), {"pads": [0, 1, 1, 0]}, [small(False, 16, True)])
conv("small_K135", (2, 15, *P9), (17, 15, 3, 3), {"pads": [1, 1, 1, 1]}, [small(False, 16, True)])  # last wave: 27 of 36
conv("small_K147_7x7_s2", (2, 3, *P9), (16, 3, 7, 7), {"strides": [2, 2], "pads": [3, 3, 3, 3]},
     [small(False, 16, True)])
conv("small_K1800", (2, 200, *P9), (5, 200, 3, 3), {"pads": [1, 1, 1, 1]}, [small(False, 16, True)])
conv("small_K27_relu", (2, 3, *P9), (5, 3, 3, 3), {"pads": [1, 1, 1, 1]}, [small(False, 8, False)],
     chain=[then("Add", x(2, 5, *P9)), then("Relu")])
conv("small_K135_prelu", (2, 15, *P9), (17, 15, 3, 3), {"pads": [1, 1, 1, 1]}, [small(False, 16, True)],
     chain=[then("PRelu", _cw(17, 1, 1))])
# groups: Mg 5 (a channel tile tail in every group), and a channel multiplier (Cg 1, Mg 2)
conv("small_G2_Mg5", (2, 6, *P9), (10, 3, 3, 3), {"group": 2, "pads": [1, 1, 1, 1]}, [small(False, 8, False)])
conv("small_G2_Mg5_K135", (2, 30, *P9), (10, 15, 3, 3), {"group": 2, "pads": [1, 1, 1, 1]}, [small(False, 16, True)])
conv("small_multiplier2", (2, 6, *P9), (12, 1, 3, 3), {"group": 6, "pads": [1, 1, 1, 1]}, [small(False, 8, False)])
# k_conv_small<true, ...>: a 1x1 that k_conv_pw does not take — grouped, or more than 192 channels on
# fewer than 256 of its workgroups
conv("small_pw_G2_Cg4", (2, 8, *P9), (10, 4, 1, 1), {"group": 2}, [small(True, 8, False)])
conv("small_pw_G2_Cg40", (2, 80, *P9), (34, 40, 1, 1), {"group": 2}, [small(True, 16, False)])
conv("small_pw_G2_Cg100", (2, 200, *P9), (40, 100, 1, 1), {"group": 2}, [small(True, 32, False)])
conv("small_pw_G3_Cg30", (2, 90, *P9), (15, 30, 1, 1), {"group": 3}, [small(True, 8, False)], bias=False)  # K % 4 != 0
conv("small_pw_C200", (2, 200, *P9), (20, 200, 1, 1), {}, [small(True, 16, True)])
conv("small_pw_C201", (2, 201, 7, 9), (5, 201, 1, 1), {}, [small(True, 16, True)],  # K % 4 != 0, last wave 45 of 52
     chain=[then("Add", x(2, 5, 7, 9)), CLIP6])

# k_conv_gemm: at least 1024 64x64 tiles.  Grouped: 64 pixel tiles x 16 (image, group) pairs, K 27 a
# K-step tail, 5 of a tile's 64 channels.  Dense: 256 pixel tiles (the last one pixel short) x 2
# channel tiles (the second holds one channel) x 2 images; non-square, so no precision tiles it
conv("gemm_G8_Mg5", (2, 24, 63, 65), (40, 3, 3, 3), {"group": 8, "pads": [1, 1, 1, 1]}, ["k_conv_gemm("])
conv("gemm_M65_2x3_dil2x1", (2, 3, 127, 129), (65, 3, 2, 3), {"dilations": [2, 1], "pads": [1, 1, 1, 1]},
     ["k_conv_gemm("], chain=[then("Relu")])

# k_conv_dw, one output per thread (a graph output: no 1x1 takes it over)
conv("dw_3x3", (2, 5, *P9), (5, 1, 3, 3), {"group": 5, "pads": [1, 1, 1, 1]}, ["k_conv_dw("])
conv("dw_5x5_s2", (2, 5, *P9), (5, 1, 5, 5), {"group": 5, "strides": [2, 2], "pads": [2, 2, 2, 2]}, ["k_conv_dw("],
     chain=[CLIP6])
conv("dw_3x5_s1x2", (2, 5, *P9), (5, 1, 3, 5), {"group": 5, "strides": [1, 2], "pads": [2, 1, 0, 1]}, ["k_conv_dw("])
conv("dw_7x1_dil2", (2, 5, *P9), (5, 1, 7, 1), {"group": 5, "dilations": [2, 2], "pads": [6, 0, 6, 0]},
     ["k_conv_dw("], bias=False)
conv("dw_3x3_dil2_pads0022", (2, 5, *P9), (5, 1, 3, 3), {"group": 5, "dilations": [2, 2], "pads": [0, 0, 2, 2]},
     ["k_conv_dw("])
# the four-outputs-per-thread body inside k_conv_dw: N * M = 65536 planes (one more than
# k_conv_dw_plane's grid takes) and exactly 1024 * 256 quads
conv("dw_quad_body", (2, 32768, 4, 4), (32768, 1, 3, 3), {"group": 32768, "pads": [1, 1, 1, 1]}, ["k_conv_dw("])
# k_conv_dw_plane<1 | 2>: 3x3, rows of a multiple of 4 outputs, at least 1024 * 256 quads.  (k_conv_dw's
# conv_dw_body<long> needs 2^30 outputs: it has no case.)
conv("dw_plane1", (2, 33, 127, 128), (33, 1, 3, 3), {"group": 33, "pads": [1, 1, 1, 1]}, ["k_conv_dw_plane<1>("])
conv("dw_plane2_s2", (4, 64, 128, 128), (64, 1, 3, 3), {"group": 64, "strides": [2, 2], "pads": [0, 0, 1, 1]},
     ["k_conv_dw_plane<2>("], chain=[then("Relu")])

# k_conv_dwpw: a depthwise -> 1x1 pair on fewer than 512 k_conv_pw workgroups (or a depthwise that is
# not 3x3 / 5x5).  Its 3x3 path and its generic one; C 24 (K % 16 != 0: A operands one by one) and 32;
# M 70 (the second channel block's last three waves have no channel); 99 / 90 / 30 pixels (a tile tail)
conv("dwpw_3x3_C24_M70", (2, 24, *P9), (24, 1, 3, 3), {"group": 24, "pads": [1, 1, 1, 1]}, ["k_conv_dwpw("],
     chain=[then("Relu"), pw_after(24, 70)])
conv("dwpw_3x3_s2_C32_M20", (2, 32, *P9), (32, 1, 3, 3), {"group": 32, "strides": [2, 2], "pads": [0, 0, 1, 1]},
     ["k_conv_dwpw("], chain=[CLIP6, pw_after(32, 20), then("Add", x(2, 20, 4, 5)), then("Relu")])
conv("dwpw_3x3_dil2_C24_M5", (2, 24, *P9), (24, 1, 3, 3), {"group": 24, "dilations": [2, 2], "pads": [2, 2, 2, 2]},
     ["k_conv_dwpw("], bias=False, chain=[pw_after(24, 5)])
conv("dwpw_3x3_pads0120_C32_M40", (2, 32, *P9), (32, 1, 3, 3), {"group": 32, "pads": [0, 1, 2, 0]},
     ["k_conv_dwpw("], chain=[then("PRelu", _cw(32, 1, 1)), pw_after(32, 40), then("PRelu", _cw(40, 1, 1))])
conv("dwpw_5x5_C24_M17", (2, 24, *P9), (24, 1, 5, 5), {"group": 24, "pads": [2, 2, 2, 2]}, ["k_conv_dwpw("],
     chain=[then("PRelu", _cw(24, 1, 1)), pw_after(24, 17, bias=False)])
conv("dwpw_3x5_dil2_C32_M70", (2, 32, *P9), (32, 1, 3, 5), {"group": 32, "dilations": [2, 2], "pads": [1, 4, 2, 3]},
     ["k_conv_dwpw("], chain=[then("Relu"), pw_after(32, 70), CLIP6])
conv("dwpw_5x5_s2_C32_M20", (2, 32, *P9), (32, 1, 5, 5), {"group": 32, "strides": [2, 2], "pads": [2, 1, 1, 2]},
     ["k_conv_dwpw("], bias=False, chain=[pw_after(32, 20)])
conv("dwpw_7x7_C24_M20", (2, 24, *P9), (24, 1, 7, 7), {"group": 24, "pads": [3, 3, 3, 3]}, ["k_conv_dwpw("],
     chain=[then("LeakyRelu", alpha=0.1), pw_after(24, 20), then("Add", x(2, 20, *P9))])

# k_conv_pw<1 | 2 | 4, 0> (M <= 16 | <= 32 | more): an ungrouped 1x1 of at most 192 channels (M 5 at
# least: up to 4 channels are k_conv_thin's), or of more on at least 256 workgroups; 63 pixels
for c_, m_ in ((3, 5), (32, 5), (33, 20), (68, 20), (32, 40), (68, 40)):
    conv(f"pw_C{c_}_M{m_}", (2, c_, 7, 9), (m_, c_, 1, 1), {}, [f"k_conv_pw<{1 if m_ <= 16 else 2 if m_ <= 32 else 4}, 0>("])
conv("pw_C33_M40_res_relu", (2, 33, 7, 9), (40, 33, 1, 1), {}, ["k_conv_pw<4, 0>("],
     chain=[then("Add", x(2, 40, 7, 9)), then("Relu")])
conv("pw_C3_M5_prelu_nobias", (2, 3, 7, 9), (5, 3, 1, 1), {}, ["k_conv_pw<1, 0>("], bias=False,
     chain=[then("PRelu", _cw(5, 1, 1))])
conv("pw_C200_M65", (2, 200, 90, 92), (65, 200, 1, 1), {}, ["k_conv_pw<4, 0>("])  # 130 x 2 x 2 = 520 workgroups
# (515 x 2 64x64 tiles: under VSO_PW=0 this one is k_conv_gemm's, the others k_conv_small<true, ...>'s)
conv("pw_C5_M10_181x182", (2, 5, 181, 182), (10, 5, 1, 1), {}, ["k_conv_pw<1, 0>("])

# k_conv_pw<WM, 3 | 5>: a 3x3 / 5x5 depthwise -> 1x1 pair on at least 512 workgroups (514 to 520)
conv("dwpw_pw1_3x3", (2, 5, 255, 258), (5, 1, 3, 3), {"group": 5, "pads": [1, 1, 1, 1]}, ["k_conv_pw<1, 3>("],
     chain=[then("Relu"), pw_after(5, 10)])
conv("dwpw_pw2_5x5", (2, 36, 181, 182), (36, 1, 5, 5), {"group": 36, "pads": [2, 2, 2, 2]}, ["k_conv_pw<2, 5>("],
     chain=[CLIP6, pw_after(36, 20), then("Add", x(2, 20, 181, 182))])
conv("dwpw_pw4_3x3", (2, 8, 90, 92), (8, 1, 3, 3), {"group": 8, "pads": [1, 1, 1, 1]}, ["k_conv_pw<4, 3>("],
     bias=False, chain=[pw_after(8, 65), then("Relu")])
conv("dwpw_pw4_3x3_s2", (2, 8, 180, 184), (8, 1, 3, 3), {"group": 8, "strides": [2, 2], "pads": [0, 0, 1, 1]},
     ["k_conv_pw<4, 3>("], chain=[then("PRelu", _cw(8, 1, 1)), pw_after(8, 65)])
conv("dwpw_pw2_3x3_pads0120", (2, 6, 183, 181), (6, 1, 3, 3), {"group": 6, "pads": [0, 1, 2, 0]}, ["k_conv_pw<2, 3>("],
     chain=[then("LeakyRelu", alpha=0.1), pw_after(6, 20)])
conv("dwpw_pw4_5x5_dil2", (2, 8, 90, 92), (8, 1, 5, 5), {"group": 8, "dilations": [2, 2], "pads": [4, 4, 4, 4]},
     ["k_conv_pw<4, 5>("], chain=[then("Relu"), pw_after(8, 65), then("Add", x(2, 65, 90, 92)), CLIP6])
conv("dwpw_pw1_5x5_s1x2", (2, 5, 255, 515), (5, 1, 5, 5), {"group": 5, "strides": [1, 2], "pads": [2, 2, 2, 2]},
     ["k_conv_pw<1, 5>("], chain=[pw_after(5, 10, bias=False)])

# k_conv_thin<1..4>: an ungrouped 1x1 onto at most 4 channels.  63 and 1089 pixels (odd), 80 and 1056
# (float4 loads); above 1024 a second workgroup per image
for m_, c_, hw_ in ((1, 5, (7, 9)), (2, 1, (8, 10)), (3, 256, (7, 9)), (4, 5, (33, 32)), (4, 256, (8, 10)),
                    (2, 5, (33, 33)), (1, 256, (33, 32)), (3, 1, (33, 33))):
    conv(f"thin_M{m_}_C{c_}_{_tag(hw_)}", (2, c_, *hw_), (m_, c_, 1, 1), {}, [f"k_conv_thin<{m_}>("])
conv("thin_M4_C5_res_leaky", (2, 5, 7, 9), (4, 5, 1, 1), {}, ["k_conv_thin<4>("],
     chain=[then("Add", x(2, 4, 7, 9)), then("LeakyRelu")])

# the attributes (k_conv_small<false, 8, false>): auto_pad on odd (9x11) and even (10x12) planes, the
# odd pad at the end (SAME_UPPER) or at the start (SAME_LOWER); auto_pad wins over pads; all omitted
for ap_ in ("SAME_UPPER", "SAME_LOWER"):
    for hw_ in (P9, (10, 12)):
        conv(f"attr_{ap_}_s2_{_tag(hw_)}", (2, 3, *hw_), (5, 3, 3, 3), {"auto_pad": ap_, "strides": [2, 2]},
             [small(False, 8, False)])
    conv(f"attr_{ap_}_dil2", (2, 3, *P9), (5, 3, 3, 3), {"auto_pad": ap_, "dilations": [2, 2]},
         [small(False, 8, False)])
    conv(f"attr_{ap_}_2x2", (2, 3, *P9), (5, 3, 2, 2), {"auto_pad": ap_}, [small(False, 8, False)])
    conv(f"attr_{ap_}_4x4_s3x2", (2, 2, 10, 12), (5, 2, 4, 4), {"auto_pad": ap_, "strides": [3, 2]},
         [small(False, 8, False)])
conv("attr_VALID", (2, 3, *P9), (5, 3, 3, 3), {"auto_pad": "VALID", "kernel_shape": [3, 3]}, [small(False, 8, False)])
conv("attr_VALID_with_pads", (2, 3, *P9), (5, 3, 3, 3), {"auto_pad": "VALID", "pads": [1, 1, 1, 1]},
     [small(False, 8, False)])
conv("attr_SAME_UPPER_with_pads", (2, 3, *P9), (5, 3, 3, 3), {"auto_pad": "SAME_UPPER", "pads": [0, 0, 0, 0]},
     [small(False, 8, False)])
conv("attr_none", (2, 3, *P9), (5, 3, 3, 3), {}, [small(False, 8, False)])

# ---------------------------------------------------------------------------
# The MobileNetV2 inverted residual, one block per case: Conv 1x1 -> Clip -> Conv 3x3 depthwise -> Clip ->
# Conv 1x1 [-> Add], fused by try_plan_ir (vso_plan.hip) into one launch of k_ir (f32 sessions) or k_ir_b16
# (bf16 / f16 sessions), plus k_ir_reduce where the hidden channels are split into slices (vso_ir.hip).
# ir_entry() picks the instance by (ceil(CIN / 16) in f32 | ceil(CIN / 32) in 16 bits, ceil(COUT / 16), stride).
#
# Planes: the 4 x 16 output tile's every tail on the smallest plane — 5 x 18 outputs (2 x 2 tiles, a 1-row
# and a 2-column tail) from 5 x 18 at stride 1, from 9 x 35 (odd) or 10 x 36 (even) at stride 2.
#
# Slices, written per case as (f32, b16), from try_plan_ir / ir_slab_plan under default knobs, wg0 = N * tiles
# workgroups per slice and nch = HID / 16 chunks:
#   f32: ks = min(nch, (512 + wg0 / 2) / wg0), cps = ceil(nch / ks), slices = ceil(nch / cps).  wg0 = 8 (batch
#        2 on 5 x 18) gives ks = min(nch, 64): one chunk per slice, nch slices.
#   b16: ks = ceil(nch / 6); below 256 workgroups ks = min(nch, ceil(256 / wg0)); cps = ceil(nch / ks), made even
#        unless it is all of nch; then cps drops by 2 while the slab and the hidden planes exceed 160 KiB of
#        LDS; slices = ceil(nch / cps).  wg0 = 8 gives chunk pairs: ceil(nch / 2) slices.
# Weights are 1 / sqrt(fan-in) normals (wf): standard-normal ones saturate the clips.
_ir_seed = [0]
PREV, IN0 = ("prev",), ("in", 0)
PW4, DWPW = "k_conv_pw<4, 0>(", "k_conv_dwpw("
ADD = ("k_binary(",)


def _iw(shape, fan_in=None):
    _ir_seed[0] += 1
    return wf(shape, _ir_seed[0], fan_in)


def node(op_, ins, **attrs):
    """A chain node with all its inputs listed (PREV: the node before it)."""
    return (op_, tuple(ins), attrs, {"whole": True})


def also_out(nd):
    """The chain node, its output one more graph output of the case."""
    return nd[:3] + (dict(nd[3] if len(nd) > 3 else {}, out=True),)


def clip(lo, hi, attr=False):
    """Clip to [lo, hi], either bound None for absent; attr: as attributes (before opset 11)."""
    if attr:
        return then("Clip", **{k: v for k, v in (("min", lo), ("max", hi)) if v is not None})
    ins = [None if lo is None else c(lo, np.float32), None if hi is None else c(hi, np.float32)]
    while ins and ins[-1] is None:
        ins.pop()
    return then("Clip", *ins)


def ir_launches(form, cin, cout, s, slices):
    """The launches of a fused block: its kernel instance, and k_ir_reduce above one slice."""
    nt = -(-cin // (16 if form == "k_ir" else 32))
    tail = ">(" if form == "k_ir_b16w" else ", 4>("
    return (f"{form}<{nt}, {-(-cout // 16)}, {s}{tail}",) + (("k_ir_reduce(",) if slices > 1 else ())


def ir(name, cin, cout, hw, f32, b16, s=1, hid=None, n=2, res=False, clips=((0.0, 6.0), (0.0, 6.0)),
       bias=(True, True, True), dw=None, k=3, ex=None, act1=None, tail=None, outs=(), after=(), after16=None,
       attr_clips=False, dw_gain=1.0, family="ir", **kw):
    """One block on a graph input [n, cin, *hw].  f32 / b16: the slices of the fused form in an f32 / a 16-bit
    session, or the launches of the generic plan where the block is not fused; `after`: further launches in
    both (after16: in a 16-bit session, where they differ).  `tail`: the nodes behind the project instead of
    the residual Add; `outs`: chain nodes whose outputs are graph outputs too; dw / ex: the depthwise's / the
    expand's attributes; act1: the first activation; dw_gain: the depthwise's weights times that (where
    1 / sqrt(9) leaves too few outputs inside the second Clip)."""
    hid = hid or 6 * cin
    dw_at = dw if dw is not None else {"group": hid, "strides": [s, s], "pads": [1, 1, 1, 1]}
    chain = [act1 or clip(*clips[0], attr=attr_clips),
             then("Conv", _iw((hid, 1, k, k), k * k / dw_gain ** 2), *([_iw((hid,))] if bias[1] else []), **dw_at),
             clip(*clips[1], attr=attr_clips),
             then("Conv", _iw((cout, hid, 1, 1), hid), *([_iw((cout,))] if bias[2] else []))]
    chain += list(tail) if tail is not None else [then("Add", IN0)] if res else []
    for j in outs:
        chain[j] = also_out(chain[j])
    launches = [ir_launches(form, cin, cout, s, v) if isinstance(v, int) else tuple(v)
                for form, v in (("k_ir", f32), ("k_ir_b16", b16))]
    case(f"IR_{name}", family, "Conv",
         [x(n, cin, *hw), _iw((hid, cin, 1, 1), cin)] + ([_iw((hid,))] if bias[0] else []), ex or {},
         kernels=launches[0] + tuple(after), kernels16=launches[1] + tuple(after if after16 is None else after16),
         chain=tuple(chain), n_out=1 + len(outs), **kw)


S1, ODD, EVEN = (5, 18), (9, 35), (10, 36)
# one case per entry of kIr / kIr16, expansion 6; the last four channel pairs on 3 x 5 outputs (one tile: two
# workgroups, up to 60 slices)
ir("16_24_s2", 16, 24, ODD, 6, 3, s=2)
ir("16_24_s2_even", 16, 24, EVEN, 6, 3, s=2)
ir("24_24_res", 24, 24, S1, 9, 5, res=True)
ir("24_32_s2", 24, 32, ODD, 9, 5, s=2)
ir("32_64_s2_even", 32, 64, EVEN, 12, 6, s=2)
ir("64_64_res", 64, 64, S1, 24, 12, res=True)
ir("64_96", 64, 96, S1, 24, 12)
ir("96_96_res", 96, 96, S1, 36, 18, res=True)
ir("96_160_s2", 96, 160, ODD, 36, 18, s=2)
ir("160_160_res_3x5", 160, 160, (3, 5), 60, 30, res=True)
ir("160_320_3x5", 160, 320, (3, 5), 60, 30)
# 26 images: 10 slices of 6 chunks reach 256 workgroups, and 6 chunks of 160 -> 320 weights exceed the LDS
# budget — ir_slab_plan steps down 6 -> 4 -> 2 chunks, 30 slices.  f32: (512 + 13) / 26 = 20 slices of 3.
ir("160_320_3x5_n26", 160, 320, (3, 5), 20, 30, n=26)
ir("64_64_s2_3x5", 64, 64, (5, 9), 24, 12, s=2)
ir("96_96_s2_3x5_even", 96, 96, (6, 10), 36, 18, s=2)
# channel tails: CIN off the 16 / 32 steps (the zero fill past CIN), COUT off 16 (the ch < COUT tails); HID a
# multiple of 16 near 6 CIN, an odd chunk count where it can be (7, 19, 31, 55 chunks)
ir("20_20_res", 20, 20, S1, 7, 4, hid=112, res=True)
ir("28_49_s2", 28, 49, ODD, 10, 5, hid=160, s=2)
ir("52_52_res", 52, 52, S1, 19, 10, hid=304, res=True)
ir("84_81", 84, 81, S1, 31, 16, hid=496)
ir("148_305", 148, 305, S1, 55, 28, hid=880)
ir("4_17_s2_hid16", 4, 17, EVEN, 1, 1, hid=16, s=2)
# forms that differ by precision: no f32 instance <1, 2, 1> / <3, 4, 1>, b16 instances <1, 2, 1> / <2, 4, 1>.
# f32: the expand on k_conv_pw, the depthwise inside the project's k_conv_dwpw (HID 96), or on its own ahead of
# a k_conv_small project (HID 288: above k_conv_dwpw's 256 channels, and a 1x1 of more than 192 channels on
# few workgroups)
ir("16_24_s1", 16, 24, S1, (PW4, DWPW), 3)
ir("48_64_s1", 48, 64, S1, (PW4, "k_conv_dw(", small(True, 16, True)), 9)
# hidden width: one chunk (the b16 forms project a half-empty pair), three (a pair and a tail), and nine on a
# plane of 9 x 19 tiles — f32: 342 workgroups, (512 + 171) / 342 = 1 slice of nine chunks; b16: ceil(9 / 6) = 2
# slices, of 6 and 3 chunks
ir("24_24_res_hid16", 24, 24, S1, 1, 1, hid=16, res=True)
ir("24_24_res_hid48", 24, 24, S1, 3, 2, hid=48, res=True)
ir("24_24_res_hid144_36x304", 24, 24, (36, 304), 1, 2, res=True)
# clips: a lower bound above 0 (the depthwise pads with 0, not with the clipped 0), two ranges that differ
# (lo1 / hi1 against lo2 / hi2), one bound, none, attributes
ir("24_24_res_clip0.5_4", 24, 24, S1, 9, 5, res=True, clips=((0.5, 4.0), (0.5, 4.0)), dw_gain=3.0)
ir("24_24_res_clips_differ", 24, 24, S1, 9, 5, res=True, clips=((-0.5, 2.0), (0.25, 5.0)))
ir("24_24_res_clip_min_only", 24, 24, S1, 9, 5, res=True, clips=((-1.0, None), (-1.0, None)))
ir("24_24_res_clip_none", 24, 24, S1, 9, 5, res=True, clips=((None, None), (None, None)))
ir("24_24_res_clip_attr", 24, 24, S1, 9, 5, res=True, attr_clips=True, family="ir6", opset=6)
# bias
ir("24_24_res_nobias", 24, 24, S1, 9, 5, res=True, bias=(False, False, False))
ir("24_32_s2_nobias_dw", 24, 32, EVEN, 9, 5, s=2, bias=(True, False, True))
# the residual and the outputs.  Fused with the residual: Add(x, project) too, and a block input that is a graph
# output.  Fused without (the Add its own k_binary launch): a project output that is a graph output, Add(project,
# project), Add(project, another input).  Two blocks in a row, both outputs read.
ir("24_24_res_swapped", 24, 24, S1, 9, 5, tail=[node("Add", [IN0, PREV])])
ir("24_24_res_input_out", 24, 24, S1, 9, 5, res=True, echo=True, seed=1)
ir("24_24_res_project_out", 24, 24, S1, 9, 5, res=True, outs=(3,), after=ADD)
ir("24_24_add_self", 24, 24, S1, 9, 5, tail=[node("Add", [PREV, PREV])], after=ADD)
ir("24_24_add_other", 24, 24, S1, 9, 5, tail=[then("Add", x(2, 24, *S1))], after=ADD)


def _second_block(cin, hid):
    """A second 24 -> 24 block behind the first one's Add (chain node 5), its residual from there."""
    return [then("Conv", _iw((hid, cin, 1, 1), cin), _iw((hid,))), clip(0.0, 6.0),
            then("Conv", _iw((hid, 1, 3, 3), 9), _iw((hid,)), group=hid, pads=[1, 1, 1, 1]), clip(0.0, 6.0),
            then("Conv", _iw((cin, hid, 1, 1), hid), _iw((cin,))), then("Add", ("node", 5))]


ir("24_24_res_twice", 24, 24, S1, 9, 5, tail=[then("Add", IN0)] + _second_block(24, 144), outs=(4,),
   after=ir_launches("k_ir", 24, 24, 1, 9), after16=ir_launches("k_ir_b16", 24, 24, 1, 5))
# planes and batch: one pixel, one row, one whole tile, one column; stride 2 from 1 x 1 and 2 x 2; batch 1, 3
# (wg0 = N * tiles stays far below 512 / 9: nch slices in f32, chunk pairs in b16)
for hw_ in ((1, 1), (1, 17), (4, 16), (5, 1)):
    ir(f"24_24_res_{_tag(hw_)}", 24, 24, hw_, 9, 5, res=True)
ir("16_24_s2_1x1", 16, 24, (1, 1), 6, 3, s=2)
ir("16_24_s2_2x2", 16, 24, (2, 2), 6, 3, s=2)
ir("24_24_res_n1", 24, 24, S1, 9, 5, n=1, res=True)
ir("24_24_res_n3", 24, 24, S1, 9, 5, n=3, res=True)
# near misses: graphs try_plan_ir must leave to the generic plan — the expand on k_conv_pw (a strided one on
# k_conv_small), the depthwise inside the project's k_conv_dwpw (the residual Add in its epilogue)
GEN = (PW4, DWPW)
ir("miss_dw_SAME_UPPER_s2", 24, 32, EVEN, GEN, GEN, s=2, dw={"group": 144, "strides": [2, 2], "auto_pad": "SAME_UPPER"})
ir("miss_dw_pads0110", 24, 32, S1, GEN, GEN, dw={"group": 144, "pads": [0, 1, 1, 0]})
ir("miss_dw_dil2", 24, 24, S1, GEN, GEN, dw={"group": 144, "dilations": [2, 2], "pads": [2, 2, 2, 2]}, res=True)
ir("miss_dw_5x5", 24, 24, S1, GEN, GEN, k=5, dw={"group": 144, "pads": [2, 2, 2, 2]}, res=True)
ir("miss_dw_s2x1", 24, 32, EVEN, GEN, GEN, dw={"group": 144, "strides": [2, 1], "pads": [1, 1, 1, 1]})
ir("miss_relu_first", 24, 24, S1, GEN, GEN, act1=then("Relu"), res=True)
ir("miss_clip1_out", 24, 24, S1, GEN, GEN, res=True, outs=(0,))
ir("miss_expand_s2", 24, 32, EVEN, (small(False, 8, False), DWPW), (small(False, 8, False), DWPW), ex={"strides": [2, 2]})
ir("miss_hid40", 24, 24, S1, GEN, GEN, hid=40, res=True)
ir("miss_cin18", 18, 24, S1, GEN, GEN, hid=96)
# 48 -> 48: <3, 3, 1> and <2, 3, 1> are in neither table (HID 288: as IR_48_64_s1 in f32)
ir("miss_48_48_res", 48, 48, S1, (PW4, "k_conv_dw(", small(True, 16, True)),
   (PW4, "k_conv_dw(", small(True, 16, True)), res=True)
# BlazeFace's strided residual around a stride-2 block: Add(project, [Pad(] MaxPool2x2(x) [)]).  The pool and the
# pad are find_residual_fusions' (read in the project's epilogue): the block is left to the generic plan
POOL = node("MaxPool", [IN0], kernel_shape=[2, 2], strides=[2, 2])
ir("miss_pool_residual", 64, 64, EVEN, GEN, GEN, s=2, hid=128, tail=[POOL, node("Add", [("node", 4), PREV])])
ir("miss_pool_pad_residual", 16, 24, EVEN, GEN, GEN, s=2,
   tail=[POOL, then("Pad", ci(0, 0, 0, 0, 0, 8, 0, 0)), node("Add", [("node", 4), PREV])])

# ---------------------------------------------------------------------------
# InstanceNormalization alone (family inorm).  plan_norm (vso_plan.hip) picks by the plane's element count:
# k_norm_plane<16, 256> up to 4096, <48, 256> up to 12288, <36, 1024> up to 36864 — one workgroup per plane, two
# passes over registers — and above that k_norm_stats ((mean, M2, count) per piece of 4096 elements) +
# k_norm_apply (the pieces merged in order, Chan et al.).  Each moves float4s where the plane is a multiple of
# 4 elements, single floats where not.  Planes on both sides of every limit, in either form; the pair at 10
# pieces with a last piece of 1 / of 4 elements / full, at 65 and at 129 pieces.  Inputs: a ramp of +-3 across
# the plane above 4096 elements (more than one piece, under VSO_NORM_PLANE=0 too), standard normal below.
PLANE16, PLANE48, PLANE36 = "k_norm_plane<16, 256>(", "k_norm_plane<48, 256>(", "k_norm_plane<36, 1024>("
STATS, APPLY = "k_norm_stats(", "k_norm_apply("


def norm_launches(inner, plane=True):
    """The launches of an InstanceNormalization of planes of `inner` elements (plane=False: VSO_NORM_PLANE=0)."""
    if plane and inner <= 36864:
        return (PLANE16 if inner <= 4096 else PLANE48 if inner <= 12288 else PLANE36,)
    return (STATS, APPLY)


def inorm(name, shape, kind=None, eps=1e-5, after=(), **kw):
    inner = int(np.prod(shape[2:]))
    case(f"IN_{name}", "inorm", "InstanceNormalization",
         [(kind or ("ramp" if inner > 4096 else "x"), tuple(shape)), cf((shape[1],), 35, lo=0.5), cf((shape[1],), 36)],
         {} if eps is None else {"epsilon": eps}, kernels=norm_launches(inner) + tuple(after), **kw)


for hw_ in ((1, 1), (1, 2), (3, 1), (1, 5), (2, 2), (63, 65), (64, 64), (17, 241), (41, 100), (96, 128), (11, 1117),
            (1, 12289), (28, 439), (192, 192), (191, 193)):
    inorm(str(hw_[0] * hw_[1]), (2, 3 if hw_[0] * hw_[1] <= 4100 else 2, *hw_))
inorm("36865", (2, 2, 73, 505))      # 10 pieces, the last of 1 element (scalar)
inorm("36868", (2, 2, 52, 709))      # the last of 4 (float4)
inorm("40960", (2, 2, 160, 256))     # 10 full pieces
inorm("262656", (1, 2, 512, 513))    # 65 pieces (float4)
inorm("525625", (1, 1, 725, 725))    # 129 pieces (scalar)
inorm("rank3_257", (2, 3, 257))
inorm("rank3_36865", (1, 2, 36865))
inorm("rank5_105", (2, 3, 3, 5, 7))
inorm("rank5_36865", (1, 2, 5, 73, 101))
for tag_, shp_ in (("4095", (2, 3, 63, 65)), ("12288", (2, 2, 96, 128)), ("36863", (2, 2, 191, 193)),
                   ("36868", (2, 2, 52, 709))):
    inorm(f"{tag_}_off100", shp_, "off100")
    inorm(f"{tag_}_small_eps1e-5", shp_, "small")
    inorm(f"{tag_}_small_eps1e-3", shp_, "small", eps=1e-3)
    inorm(f"{tag_}_half", shp_, "half", exact=True)
inorm("default_eps", (2, 3, 7, 9), "small", eps=None)
inorm("63_relu", (2, 3, 7, 9), after=("k_unary(",), chain=(then("Relu"),))
inorm("rows1", (1, 1, 3, 5))
inorm("rows257", (1, 257, 3, 5))

# ---------------------------------------------------------------------------
# MODNet's IBNorm (family ibn), one pattern per case, fused by find_ibnorm (vso_plan.hip):
#   c = Conv(x); Concat(BatchNorm(Slice(c, 0:nb)), InstanceNorm(Slice(c, nb:M)), axis 1) [-> Relu] [-> consumer]
# The conv writes the concatenation (the BatchNorm folded into its first nb channels, the Relu on them in its
# epilogue), the norm runs in place on channels nb .. M - 1 (c0 = nb, ctot = M).  Before a thin 1x1 head
# (k_conv_thin, up to 4 outputs from up to 256 channels) only k_norm_stats runs: the head merges the pieces
# (merge_stats) and normalises in its loads.  Before a Concat on axis 1 the conv writes into that Concat's
# output and the norm runs there (ctot > M).  Chain layout of every case: Slice, Slice, BatchNormalization,
# InstanceNormalization, Concat, [Relu], the consumer's nodes (IBN: the figures tests/norm_ref.py needs).
_ibn_seed = [0]
IBN = {}


def _bw(shape, fan_in=None, lo=None, gain=1.0):
    """A seeded float32 constant of the ibn family: a weight (normal / sqrt(fan_in)), gain * normal, or
    uniform in [lo, lo + 1)."""
    _ibn_seed[0] += 1
    rng = np.random.default_rng(3000 + _ibn_seed[0])
    if lo is not None:
        a = rng.random(shape) + lo
    else:
        a = rng.standard_normal(shape) * (gain if fan_in is None else fan_in ** -0.5)
    return ("c", a.astype(np.float32))


def _slice(src, b, e, form="axes"):
    """Slice(src, b:e) of the channels of M: form "axes" (starts, ends, axes), "steps" (and steps = [1]),
    "both" (axes omitted: axis 0 whole, then the channels); b / e as given (negative, INT64_MAX)."""
    if form == "both":
        return node("Slice", [src, ci(0, b), ci(INT64_MAX, e)])
    return node("Slice", [src, ci(b), ci(e), ci(1)] + ([ci(1)] if form == "steps" else []))


def pw_name(m):
    return f"k_conv_pw<{1 if m <= 16 else 2 if m <= 32 else 4}, 0>("


def ibn(name, xs, m, nb, conv, ks=1, relu=True, bias=True, eps_bn=None, eps_in=None, var=None, slices=None, tail=(),
        after=None, defer=False, cat=None, out=False, fused=True, order=(0, 1), c_in=None, axis=1, split=False,
        conv_out=False, family="ibn", bn=None, kind=None, **kw):
    """One pattern on a graph input `xs`: Conv (ks x ks, padded to keep the plane) onto m channels, nb of them
    to the BatchNorm.  conv: the conv's launch; after: the launches behind it (default: the norm's by plane
    size; defer: k_norm_stats alone); tail: the consumer's nodes; cat: (position of the pattern among a later
    Concat's two inputs, the skip's channels); out: the pattern's output is a graph output too; slices: the two
    Slice nodes where they are not 0:nb / nb:m; c_in: the InstanceNorm's channels where not m - nb; order: the
    Concat's inputs; split: a Split for the Slices; conv_out: the conv's output is a graph output too; bn: the
    BatchNorm's (scale, B, mean, var) where given; kind: the input's, where neither a ramp (planes above 4096
    elements) nor standard normal."""
    n, cch, h, w = xs
    inner = h * w
    c_in = m - nb if c_in is None else c_in
    conv0 = ("node", 0)
    if split:
        chain = [node("Split", [conv0, ci(nb, m - nb)], axis=1)[:3] + ({"whole": True, "n": 2},)]
        src_bn, src_in = ("node", 1), ("node", 1, 1)
    else:
        chain = list(slices or (_slice(conv0, 0, nb), _slice(conv0, nb, m)))
        src_bn, src_in = ("node", 1), ("node", 2)
    bn_c = bn or (_bw((nb,), lo=0.5), _bw((nb,), gain=0.5), _bw((nb,), gain=0.5),
                  ("c", np.full(nb, var, np.float32)) if var is not None else _bw((nb,), lo=0.5))
    i_bn = len(chain) + 1  # (node j is chain[j - 1])
    chain.append(node("BatchNormalization", [src_bn, *bn_c], **({} if eps_bn is None else {"epsilon": eps_bn})))
    chain.append(node("InstanceNormalization", [src_in, _bw((c_in,), lo=0.5), _bw((c_in,), gain=0.5)],
                      **({} if eps_in is None else {"epsilon": eps_in})))
    chain.append(node("Concat", [("node", i_bn + order[0]), ("node", i_bn + order[1])], axis=axis))
    if relu:
        chain.append(then("Relu"))
    if out:
        chain[-1] = also_out(chain[-1])
    pos_ = len(chain)  # the pattern's output: node pos_
    if cat is not None:
        skip = ("ramp" if inner > 4096 else "x", (n, cat[1], h, w))
        chain.append(node("Concat", [PREV, skip] if cat[0] == 0 else [skip, PREV], axis=1))
    chain += list(tail)
    if after is None:
        after = (STATS,) if defer else norm_launches(inner)
    n_out = 1 + bool(conv_out) + sum(1 for nd in chain[:-1] if len(nd) > 3 and nd[3].get("out"))
    pad = (ks - 1) // 2
    IBN[f"IBN_{name}"] = {"m": m, "nb": nb, "relu": relu, "defer": defer, "cat": cat, "fused": fused, "out": out,
                          "i_bn": i_bn, "pos": pos_}
    case(f"IBN_{name}", family, "Conv",
         [(kind or ("ramp" if inner > 4096 else "x"), tuple(xs)), _bw((m, cch, ks, ks), cch * ks * ks)]
         + ([_bw((m,), gain=0.5)] if bias else []),
         {"pads": [pad] * 4} if ks > 1 else {}, kernels=(conv,) + tuple(after), chain=tuple(chain), n_out=n_out,
         op_out=conv_out, **kw)


def head(m_out, c_, **attrs):
    """A 1x1 head onto m_out channels (with a bias)."""
    return then("Conv", _bw((m_out, c_, 1, 1), c_), _bw((m_out,), gain=0.5), **attrs)


THIN = "k_conv_thin<%d>("
# (a) a graph output: every conv form, nb 1 / M - 1 / M / 2 / odd of M 5 / 24 / 32, with and without the Relu and
# the bias, the epsilons default and explicit, planes on both sides of the norm's thresholds
ibn("pw_M5_nb1_4", (2, 3, 2, 2), 5, 1, pw_name(5))
ibn("pw_M5_nb4_63_neg", (2, 3, 7, 9), 5, 4, pw_name(5), relu=False, bias=False,
    slices=(_slice(("node", 0), -5, -1), _slice(("node", 0), -1, INT64_MAX)))
ibn("pw_M24_nb12_2304_eps", (2, 8, 36, 64), 24, 12, pw_name(24), eps_bn=1e-3, eps_in=1e-4,
    slices=(_slice(("node", 0), 0, 12, "steps"), _slice(("node", 0), 12, INT64_MAX, "steps")))
ibn("pw_M24_nb7_4100", (2, 8, 41, 100), 24, 7, pw_name(24))
ibn("pw_M5_nb2_36868", (2, 3, 52, 709), 5, 2, pw_name(5))
ibn("pw_M5_nb2_var0.01", (2, 3, 7, 9), 5, 2, pw_name(5), var=0.01, eps_bn=1e-3, relu=False)
ibn("small3x3_M5_nb2_99", (2, 3, 9, 11), 5, 2, small(False, 8, False), ks=3)
ibn("small3x3_M24_nb23_99", (2, 8, 9, 11), 24, 23, small(False, 32, False), ks=3, relu=False, bias=False)
ibn("tile_M32_nb16_2304", (2, 16, 36, 64), 32, 16, "k_conv_tile<", ks=3)
ibn("tile_M32_nb5_2304", (2, 16, 36, 64), 32, 5, "k_conv_tile<", ks=3, relu=False, bias=False, eps_in=1e-3)
# (b) a thin 1x1 head of 1 .. 4 outputs: the apply step inside k_conv_thin.  1 piece, 10 pieces with a last one
# of 1 element, 65, 129 (merge_stats' lane loop a second and a third time); its float4 and scalar pixel paths
ibn("thin1_63", (2, 3, 7, 9), 5, 2, pw_name(5), tail=[head(1, 5)], after=(STATS, THIN % 1), defer=True)
ibn("thin4_4096", (2, 4, 64, 64), 5, 3, pw_name(5), relu=False, tail=[head(4, 5)], after=(STATS, THIN % 4), defer=True)
ibn("thin2_36865", (2, 3, 73, 505), 5, 1, pw_name(5), tail=[head(2, 5)], after=(STATS, THIN % 2), defer=True)
ibn("thin3_262656", (1, 3, 512, 513), 2, 1, pw_name(2), tail=[head(3, 2)], after=(STATS, THIN % 3), defer=True)
ibn("thin4_525625", (1, 3, 725, 725), 2, 1, pw_name(2), bias=False, tail=[head(4, 2)], after=(STATS, THIN % 4), defer=True)
ibn("thin2_M256_nb1", (2, 3, 5, 7), 256, 1, pw_name(256), tail=[head(2, 256)], after=(STATS, THIN % 2), defer=True)
# (inputs of variance 1e-4: the epsilon inside k_conv_thin's scale counts)
ibn("thin2_63_small", (2, 3, 7, 9), 5, 2, pw_name(5), kind="small", tail=[head(2, 5)], after=(STATS, THIN % 2), defer=True)
# 257 channels: beyond k_conv_thin — the norm's own launch, the head on k_conv_small
ibn("head2_M257_nb1", (2, 3, 5, 7), 257, 1, pw_name(257), tail=[head(2, 257)], after=(PLANE16, small(True, 16, True)))
ibn("tile_thin2_2304", (2, 16, 36, 64), 32, 16, "k_conv_tile<", ks=3, tail=[head(2, 32)], after=(STATS, THIN % 2),
    defer=True)
# (c) heads k_conv_thin does not take: the norm applies itself.  A head that is an IBNorm's conv is found thin
# by feeds_thin and declined by plan_conv: its input's apply step is flush_norm's
ibn("head_s2_63", (2, 3, 7, 9), 5, 2, pw_name(5), tail=[head(2, 5, strides=[2, 2])], after=(PLANE16, small(False, 8, False)))
ibn("head5_63", (2, 3, 7, 9), 5, 2, pw_name(5), tail=[head(5, 5)], after=(PLANE16, pw_name(5)))
ibn("head_g5_63", (2, 3, 7, 9), 5, 2, pw_name(5), tail=[then("Conv", _bw((5, 1, 1, 1), 1), group=5)],
    after=(PLANE16, "k_conv_dw("))
# (the head's conv is node 7: its slices name it)
ibn("head_ibn_63", (2, 3, 7, 9), 5, 2, pw_name(5),
    tail=[head(4, 5), _slice(("node", 7), 0, 2), _slice(("node", 7), 2, 4),
          node("BatchNormalization", [("node", 8), _bw((2,), lo=0.5), _bw((2,), gain=0.5), _bw((2,), gain=0.5),
                                      _bw((2,), lo=0.5)]),
          node("InstanceNormalization", [("node", 9), _bw((2,), lo=0.5), _bw((2,), gain=0.5)]),
          node("Concat", [("node", 10), ("node", 11)], axis=1)],
    after=(STATS, APPLY, pw_name(4), PLANE16), defer=True)
# (d) the pattern's output a graph output besides: not deferred
ibn("thin2_and_out_63", (2, 3, 7, 9), 5, 2, pw_name(5), out=True, tail=[head(2, 5)], after=(PLANE16, THIN % 2))
# (e) into a later Concat on axis 1, as its first and as its second input: the conv and the norm write in place
# there (ctot 5 + 3), batch 2
ibn("cat_first_63", (2, 3, 7, 9), 5, 2, pw_name(5), cat=(0, 3), after=(PLANE16, "k_copy_rows<"))
ibn("cat_second_63", (2, 3, 7, 9), 5, 2, pw_name(5), cat=(1, 3), relu=False, after=(PLANE16, "k_copy_rows<"))
ibn("cat_second_36868", (2, 3, 52, 709), 5, 2, pw_name(5), cat=(1, 1), after=(STATS, APPLY, "k_copy_rows<"))
ibn("tile_cat_first_2304", (2, 16, 36, 64), 32, 16, "k_conv_tile<", ks=3, cat=(0, 2), after=(PLANE16, "k_copy_rows<"))
# Near misses: left to the generic plan — the conv, a copy per Slice (Split: per output), k_affine, the norm, a
# copy per Concat input, k_unary for the Relu
GENERIC = ("k_copy_rows<", "k_copy_rows<", "k_affine(", PLANE16, "k_copy_rows<", "k_copy_rows<")
RELU = ("k_unary(",)
ibn("miss_split", (2, 3, 7, 9), 5, 2, pw_name(5), split=True, fused=False, after=GENERIC + RELU)
ibn("miss_axes_omitted", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, after=GENERIC + RELU,
    slices=(_slice(("node", 0), 0, 2, "both"), _slice(("node", 0), 2, INT64_MAX, "both")))
ibn("miss_gap", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, c_in=2, after=GENERIC + RELU,
    slices=(_slice(("node", 0), 0, 2), _slice(("node", 0), 3, 5)))
ibn("miss_overlap", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, c_in=4, after=GENERIC + RELU,
    slices=(_slice(("node", 0), 0, 2), _slice(("node", 0), 1, 5)))
ibn("miss_in_then_bn", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, order=(1, 0), after=GENERIC + RELU)
ibn("miss_third_consumer", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, after=GENERIC + RELU + RELU, out=True,
    tail=[node("Relu", [("node", 0)])])
ibn("miss_axes-3", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, after=GENERIC + RELU,
    slices=(node("Slice", [("node", 0), ci(0), ci(2), ci(-3)]), node("Slice", [("node", 0), ci(2), ci(5), ci(-3)])))
ibn("miss_step2", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, c_in=2,
    after=("k_copy_rows<", "k_copy(", "k_affine(", PLANE16, "k_copy_rows<", "k_copy_rows<") + RELU,
    slices=(_slice(("node", 0), 0, 2), node("Slice", [("node", 0), ci(2), ci(5), ci(1), ci(2)])))
ibn("miss_concat_axis2", (2, 3, 7, 9), 6, 3, pw_name(6), fused=False, axis=2,
    after=("k_copy_rows<", "k_copy_rows<", "k_affine(", PLANE16, "k_copy(", "k_copy(") + RELU)
ibn("miss_slice_attr", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, family="ibn9", opset=9, after=GENERIC + RELU,
    slices=(node("Slice", [("node", 0)], starts=[0], ends=[2], axes=[1]),
            node("Slice", [("node", 0)], starts=[2], ends=[INT64_MAX], axes=[1])))
# the conv's output a graph output too
ibn("miss_conv_out", (2, 3, 7, 9), 5, 2, pw_name(5), fused=False, after=GENERIC + RELU, conv_out=True)

# 16-bit sessions fold the BatchNorm into the weights, then round them; the oracle rounds the weights, then
# applies the BatchNorm.  With epsilon 2^-10, var 1 - 2^-10 and power-of-two scales the fold factor is a power
# of two: the two commute, and the dense 3x3 patterns (k_conv_tile in a 16-bit session whatever their size) meet
# the oracle of R.run(conv_operands=...) at the matrix's bar (family ibn16)
def _bn16(nb):
    # (scales 1/2 .. 4; tests/test_op_matrix_oracle.py asserts the commutation on the weights drawn: a product in
    # float16's subnormal range would not commute)
    return (("c", (2.0 ** (np.arange(nb) % 4 - 1)).astype(np.float32)), _bw((nb,), gain=0.5), _bw((nb,), gain=0.5),
            ("c", np.full(nb, 1 - 2.0 ** -10, np.float32)))


ibn("b16_tile_M32_nb16_2304", (2, 16, 36, 64), 32, 16, "k_conv_tile<", ks=3, family="ibn16", bn=_bn16(16),
    eps_bn=2.0 ** -10)
ibn("b16_3x3_M5_nb2_99_thin2", (2, 3, 9, 11), 5, 2, small(False, 8, False), ks=3, family="ibn16", bn=_bn16(2),
    eps_bn=2.0 ** -10, tail=[head(2, 5)], after=(STATS, THIN % 2), defer=True)
ibn("b16_3x3_M24_nb7_cat_99", (2, 8, 9, 11), 24, 7, small(False, 32, False), ks=3, relu=False, family="ibn16",
    bn=_bn16(7), eps_bn=2.0 ** -10, cat=(1, 3), after=(PLANE16, "k_copy_rows<"))

# ---------------------------------------------------------------------------
# what the session refuses at creation (and the oracle refuses to evaluate)
case("refuse_Resize_antialias", "refused", "Resize", _resize_inputs(scale=0.5), {"mode": "linear", "antialias": 1},
     opset=18, expect="refused")
case("refuse_Resize_axes", "refused", "Resize", [x(*RX), None, c([2, 2], np.float32)], {"mode": "linear", "axes": [2, 3]},
     opset=18, expect="refused")
case("refuse_Resize_keep_aspect_ratio_policy", "refused", "Resize", _resize_inputs(sizes=(7, 13)),
     {"mode": "linear", "keep_aspect_ratio_policy": "not_larger"}, opset=18, expect="refused")
case("refuse_Resize_nearest_mode", "refused", "Resize", _resize_inputs(scale=2.0),
     {"mode": "nearest", "nearest_mode": "round_half_up"}, expect="refused")
case("refuse_Resize_cubic", "refused", "Resize", _resize_inputs(scale=2.0), {"mode": "cubic"}, expect="refused")
case("refuse_MaxPool_pads_length", "refused", "MaxPool", [x(*X)], {"kernel_shape": [3, 3], "pads": [1, 1]},
     expect="refused")
case("refuse_AveragePool_pads_length", "refused", "AveragePool", [x(*X)], {"kernel_shape": [3, 3], "pads": [1, 1]},
     expect="refused")
case("refuse_MaxPool_storage_order", "refused", "MaxPool", [x(*X)], {"kernel_shape": [2, 2], "storage_order": 1},
     expect="refused")
case("refuse_MaxPool_Indices", "refused", "MaxPool", [x(*X)], {"kernel_shape": [2, 2]}, n_out=2, expect="refused")
case("refuse_Pad_reflect", "refused", "Pad", [x(*X), ci(0, 0, 1, 1, 0, 0, 1, 1)], {"mode": "reflect"}, expect="refused")
case("refuse_Softmax_axis1_rank3", "refused", "Softmax", [x(2, 3, 5)], {"axis": 1}, expect="refused")
case("refuse_Softmax_axis0_rank2", "refused", "Softmax", [x(3, 5)], {"axis": 0}, expect="refused")
case("refuse_Split_uneven_opset13", "refused", "Split", [x(2, 7, 4, 5)], {"axis": 1}, n_out=3, expect="refused")
case("refuse_Split_uneven_opset11", "refused", "Split", [x(2, 7, 4, 5)], {"axis": 1}, n_out=2, opset=11,
     expect="refused")
# a 1-D slope aligns with W: [C] with C != W does not broadcast
case("refuse_PRelu_1d_channels", "refused", "PRelu", [x(*X), cf((3,), 41)], expect="refused")
case("refuse_ConvPRelu_1d_channels", "refused", "Conv", [x(1, 3, 6, 5), cf((4, 3, 3, 3), 6), cf((4,), 7)],
     {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, post=("PRelu", cf((4,), 9)[1]), expect="refused")
case("refuse_PRelu_wider_slope", "refused", "PRelu", [x(3, 1, 1), x(2, 3, 10, 11)], expect="refused")
case("refuse_Conv_runtime_weights", "refused", "Conv", [x(2, 3, *P9), x(5, 3, 3, 3)], expect="refused")
case("refuse_Conv_channels", "refused", "Conv", [x(2, 4, *P9), _cw(5, 3, 3, 3)], expect="refused")
case("refuse_Conv_group_channels", "refused", "Conv", [x(2, 6, *P9), _cw(5, 3, 3, 3)], {"group": 2}, expect="refused")
case("refuse_Conv_rank3", "refused", "Conv", [x(2, 3, 9), _cw(5, 3, 3)], expect="refused")
case("refuse_Conv_empty_output", "refused", "Conv", [x(2, 3, 2, 2), _cw(5, 3, 3, 3)], expect="refused")
case("refuse_Conv_pads_length", "refused", "Conv", [x(2, 3, *P9), _cw(5, 3, 3, 3)], {"pads": [1, 1]}, expect="refused")
case("refuse_Conv_strides_length", "refused", "Conv", [x(2, 3, *P9), _cw(5, 3, 3, 3)], {"strides": [2]},
     expect="refused")
case("refuse_Conv_dilations_length", "refused", "Conv", [x(2, 3, *P9), _cw(5, 3, 3, 3)], {"dilations": [2]},
     expect="refused")

case("refuse_InstanceNormalization_runtime_scale", "refused", "InstanceNormalization",
     [x(2, 3, 4, 5), x(3), cf((3,), 36)], expect="refused")
case("refuse_InstanceNormalization_rank2", "refused", "InstanceNormalization", [x(2, 3), cf((3,), 35, lo=0.5), cf((3,), 36)],
     expect="refused")
case("refuse_InstanceNormalization_scale_size", "refused", "InstanceNormalization",
     [x(2, 3, 4, 5), cf((2,), 35, lo=0.5), cf((3,), 36)], expect="refused")
case("refuse_InstanceNormalization_B_size", "refused", "InstanceNormalization",
     [x(2, 3, 4, 5), cf((3,), 35, lo=0.5), cf((4,), 36)], expect="refused")

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


def _input_name(cs: Case, pos_: int):
    kind, shape = cs.inputs[pos_]
    return f"{cs.family}_{kind}{pos_}_{_tag(shape)}_s{cs.seed}"


def _chain_input_name(cs: Case, k: int, pos_: int):
    kind, shape = cs.chain[k][1][pos_]
    return f"{cs.family}_{kind}{k}.{pos_}_{_tag(shape)}_s{cs.seed}"


def _generate(name, kind, shape):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if kind == "pos":
        a = rng.random(shape) + 0.5
    elif kind == "pm80":
        a = rng.choice([-80.0, 80.0], size=shape) + rng.standard_normal(shape)
    elif kind == "ramp":  # a ramp of +-3 across each plane: the pieces' means differ by more than a standard deviation
        inner = int(np.prod(shape[2:], dtype=np.int64))
        a = rng.standard_normal(shape) + np.linspace(-3.0, 3.0, inner).reshape((1, 1) + tuple(shape[2:]))
    elif kind == "off100":  # a mean far from 0: E[x^2] - E[x]^2 cancels
        a = rng.standard_normal(shape) + 100.0
    elif kind == "small":  # a variance of 1e-4: epsilon counts
        a = 0.01 * rng.standard_normal(shape)
    elif kind == "half":  # constant planes of a small multiple of 0.5 each: every float32 partial sum is exact
        k = np.arange(int(np.prod(shape[:2])), dtype=np.int64)
        a = np.broadcast_to((0.5 * (1 + k % 7) * (1 - 2 * (k % 2))).reshape(tuple(shape[:2]) + (1,) * (len(shape) - 2)),
                            shape)
    elif kind == "q8":  # multiples of 1/8: a 2x linear Resize of them is exact in float32 and float64 alike
        a = np.round(rng.standard_normal(shape) * 8.0) / 8.0
    else:  # "x", "x3", "x4": standard normal, times 3 / 4 (wider activations)
        a = rng.standard_normal(shape) * (float(kind[1:]) if len(kind) > 1 else 1.0)
    return a.astype(np.float32)


def output_names(cs: Case):
    return [cs.name] if cs.n_out == 1 else [f"{cs.name}.{k}" for k in range(cs.n_out)]


def build(cases):
    """(model bytes, feeds, {case name: its graph outputs}) of one model holding
    `cases`: cases of one family share the graph inputs they describe alike."""
    cases = list(cases)
    opset = cases[0].opset
    assert all(k.opset == opset for k in cases)
    b = M.Builder(0)
    feeds, graph_in, graph_out, outs = {}, [], [], {}

    def operand(spec, n):
        if spec is None:
            return ""
        if spec[0] == "c":
            return b.const(spec[1])
        if n not in feeds:
            feeds[n] = _generate(n, *spec)
            graph_in.append((n, list(spec[1])))
        return n

    for cs in cases:
        names = [operand(spec, spec and spec[0] != "c" and _input_name(cs, pos_)) for pos_, spec in enumerate(cs.inputs)]
        made = []  # the outputs of the case's nodes, in order

        def chain_operand(spec, k, pos_):
            if spec and spec[0] in ("prev", "in", "node"):
                if spec[0] == "node" and len(spec) > 2 and spec[2]:  # a further output of a node with several
                    return f"{made[spec[1]]}.{spec[2]}"
                return made[-1] if spec[0] == "prev" else names[spec[1]] if spec[0] == "in" else made[spec[1]]
            return operand(spec, spec and spec[0] != "c" and _chain_input_name(cs, k, pos_))

        while names and names[-1] == "":
            names.pop()
        finals = output_names(cs)
        if cs.chain:
            extra = iter(finals[:-1])
            made.append(next(extra) if cs.op_out else b.name("mid"))
            b.nodes.append(R.make_node(cs.op, names, [made[0]], **cs.attrs))
            for k, nd in enumerate(cs.chain):
                (op_, ins_, at_), opts = nd[:3], nd[3] if len(nd) > 3 else {}
                more = [chain_operand(spec, k, pos_) for pos_, spec in enumerate(ins_)]
                nxt = finals[-1] if k + 1 == len(cs.chain) else next(extra) if opts.get("out") else b.name("mid")
                nxts = [nxt] + [f"{nxt}.{q}" for q in range(1, opts.get("n", 1))]  # "n": a node of several outputs
                b.nodes.append(R.make_node(op_, more if opts.get("whole") else [made[-1]] + more, nxts, **at_))
                made.append(nxt)
        elif cs.post:
            mid = b.name("mid")
            b.nodes.append(R.make_node(cs.op, names, [mid], **cs.attrs))
            b.nodes.append(R.make_node(cs.post[0], [mid, b.const(cs.post[1])], finals))
        else:
            b.nodes.append(R.make_node(cs.op, names, finals, **cs.attrs))
        # MaxPool's Indices are asked for by naming them; only the values are graph outputs
        outs[cs.name] = finals[:1] if cs.op == "MaxPool" else ([names[0]] if cs.echo else []) + finals
        graph_out += [(o, []) for o in outs[cs.name]]
    return b.model(graph_in, graph_out, opset=opset), feeds, outs


def operands(cs: Case, feeds):
    """The case's operator inputs as arrays (None where omitted), in operator order."""
    out = []
    for pos_, spec in enumerate(cs.inputs):
        out.append(None if spec is None else spec[1] if spec[0] == "c" else feeds[_input_name(cs, pos_)])
    return out


def chain_operands(cs: Case, feeds):
    """Per node of the case's chain: its further inputs as arrays, in operator order."""
    def one(spec, k, pos_):
        if spec[0] in ("prev", "in", "node"):  # a reference to another value of the case: left as written
            return spec
        return spec[1] if spec[0] == "c" else feeds[_chain_input_name(cs, k, pos_)]
    return [[one(spec, k, pos_) for pos_, spec in enumerate(nd[1])] for k, nd in enumerate(cs.chain)]
