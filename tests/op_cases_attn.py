"""The operator matrix of the transformer-block operators (test
infrastructure): LayerNormalization and its decomposed form, Gelu / Erf and the
erf form of GELU, a Linear layer's bias, and the attention pattern.
op_cases.Case objects packed by op_cases.build, kept in this module's own list
(op_cases.CASES and the parametrisation of tests/test_gpu_op_matrix.py do not
move).  Shared by tests/test_attn_ref.py (tests/onnx_ref_attn.py against
PyTorch in float64, and float32 restatements of the kernels, CPU) and
tests/test_gpu_attn_matrix.py (the GPU sessions against onnx_ref_attn).

Batch 2 throughout.  `kernels` names each case's launches, in order.

lnorm   rows 2 x 15 and 2 x 3 x 7; D on both sides of every form of
        k_layer_norm — <4> (a wave per row, D <= 256), <16> (D <= 1024), <0>
        (a workgroup per row; the row in LDS up to 8192 elements, re-read
        beyond) — and off the 64-lane stride (3, 160, 1000, 4100).
gelu    inputs of 3 x standard normal (beyond +-6).
attn    [2, h, N, d] tensors; Nq across the 16-row wave tile and the 64-row
        workgroup tile, Nk across the 16-key half and the 32-key block, d
        across the 16-element fragment chunk and every instance <1> <2> <4>
        <8> of k_attn.
"""
from __future__ import annotations

import numpy as np

import op_cases as OC
from op_cases import IN0, PREV, Case, also_out, c, node, then, x

CASES: list[Case] = []
# per case, what tests/test_attn_ref.py needs to state it again in PyTorch and in float32 numpy: the constants,
# and where the operands sit in the case's chain ((chain node, input position) pairs)
META: dict[str, dict] = {}
_seed = [0]


def case(name, family, op, inputs, attrs=None, **kw):
    assert all(k.name != name for k in CASES), name
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), **kw))


def _c(shape, scale, shift=0.0):
    _seed[0] += 1
    return ("c", (np.random.default_rng(9000 + _seed[0]).standard_normal(shape) * scale + shift).astype(np.float32))


def f32(v):
    return c(v, np.float32)


LN = ("k_layer_norm<%d>(",)
LN4, LN16, LN0 = LN[0] % 4, LN[0] % 16, LN[0] % 0
UNARY, CONV1, GEMM, BIN = "k_unary(", "k_conv", "k_gemm", "k_binary"

# ---- LayerNormalization (opset 17) ----------------------------------------------------
L = "lnorm"


def lnorm(name, shape, kernel, axis=None, with_b=True, eps=None, kind="x", d=None, **kw):
    nshape = tuple(shape[axis:]) if axis is not None else tuple(shape[-1:])
    assert int(np.prod(nshape)) == (d or shape[-1])
    at = {}
    if axis is not None:
        at["axis"] = axis
    if eps is not None:
        at["epsilon"] = eps
    ins = [(kind, tuple(shape)), _c(nshape, 0.1, 1.0)] + ([_c(nshape, 0.1)] if with_b else [])
    case(f"LayerNorm_{name}", L, "LayerNormalization", ins, at, kernels=(kernel,), opset=17, **kw)
    META[f"LayerNorm_{name}"] = {"nshape": nshape, "gamma": ins[1][1], "beta": ins[2][1] if with_b else None,
                                 "eps": 1e-5 if eps is None else eps}


R15, R37 = (2, 15), (2, 3, 7)
lnorm("D3", R15 + (3,), LN4)
lnorm("D32", R37 + (32,), LN4)
lnorm("D64", R15 + (64,), LN4)
lnorm("D160", R37 + (160,), LN4)
lnorm("D256", R15 + (256,), LN4)
lnorm("D257", R15 + (257,), LN16)
lnorm("D1000", R37 + (1000,), LN16)
lnorm("D1024", R15 + (1024,), LN16)
lnorm("D1025", R15 + (1025,), LN0)
lnorm("D4100", R15 + (4100,), LN0)
lnorm("D8200_past_lds", (2, 3, 8200), LN0)
lnorm("axis_m2_D160", R15 + (8, 20), LN4, axis=-2, d=160)
lnorm("axis_2_D1200", (2, 3, 40, 30), LN0, axis=2, d=1200)
lnorm("D64_no_B", R37 + (64,), LN4, with_b=False)
lnorm("D160_eps1e-3_small", R15 + (160,), LN4, eps=1e-3, kind="small")
# rows of mean 100, std 1: E[x^2] - mean^2 in float32 loses the variance (test_attn_ref: the one-pass restatement fails)
lnorm("D256_off100", R15 + (256,), LN4, kind="off100")
lnorm("D1000_off100", R15 + (1000,), LN16, kind="off100")
lnorm("D4100_off100", R15 + (4100,), LN0, kind="off100")

# the decomposed form, as PyTorch exports it below opset 17: one k_layer_norm all the same
LD = "lnorm13"
AX = {"axes": [-1], "keepdims": 1}


def decomposed(square, gamma=None, beta=None, eps=1e-5, extra=()):
    sq = node("Pow", [("node", 1), f32(2.0)]) if square == "pow" else node("Mul", [("node", 1), ("node", 1)])
    chain = [node("Sub", [IN0, PREV]), sq, node("ReduceMean", [PREV], **AX), node("Add", [PREV, f32(eps)]),
             node("Sqrt", [PREV]), node("Div", [("node", 1), PREV])]
    if gamma is not None:
        chain.append(node("Mul", [PREV, gamma]))
    if beta is not None:
        chain.append(node("Add", [PREV, beta]))
    return tuple(chain) + tuple(extra)


def lnorm13(name, shape, kernel, chain, kind="x", gamma=None, beta=None, eps=1e-5, **kw):
    META[f"LayerNorm13_{name}"] = {"nshape": tuple(shape[-1:]), "gamma": gamma, "beta": beta, "eps": eps}
    case(f"LayerNorm13_{name}", kw.pop("family", LD), "ReduceMean", [(kind, tuple(shape))], dict(AX), chain=chain,
         kernels=(kernel,) if kernel else (), **kw)


def _ln13(name, shape, kernel, square, gamma=None, beta=None, eps=1e-5, **kw):
    lnorm13(name, shape, kernel, decomposed(square, gamma, beta, eps), gamma=gamma and gamma[1], beta=beta and beta[1],
            eps=eps, **kw)


_ln13("pow_gamma_beta_D64", R15 + (64,), LN4, "pow", _c((64,), 0.1, 1.0), _c((64,), 0.1))
_ln13("mul_gamma_beta_D160", R37 + (160,), LN4, "mul", _c((160,), 0.1, 1.0), _c((160,), 0.1), eps=1e-6)
_ln13("pow_plain_D1000", R15 + (1000,), LN16, "pow")
_ln13("mul_gamma_D4100", R15 + (4100,), LN0, "mul", _c((4100,), 0.1, 1.0))
_ln13("pow_scalar_gamma_off100_D256", R15 + (256,), LN4, "pow", f32(1.5), _c((256,), 0.1), kind="off100")

# ---- Gelu, Erf and the erf form (opset 20) --------------------------------------------
G = "gelu"
X3 = ("x3", (2, 3, 10, 11))
RT2 = float(np.sqrt(2.0))


def gelu(name, op, inputs, attrs=None, **kw):
    case(name, G, op, inputs, attrs, opset=20, **kw)


def erf_form(assoc, first=None):
    """The nodes behind x / sqrt 2 (node `first`, default the case's operator; x: that node's input 0)."""
    xs = IN0 if first is None else ("node", first)
    base = 0 if first is None else first + 1
    head = [then("Erf"), then("Add", f32(1.0))]
    one_erf = ("node", base + 2)
    if assoc == "x_erf_half":    # (x * (1 + erf)) * 0.5
        return head + [node("Mul", [xs, PREV]), then("Mul", f32(0.5))]
    if assoc == "erf_half_x":    # x * ((1 + erf) * 0.5)
        return head + [then("Mul", f32(0.5)), node("Mul", [xs, PREV])]
    return head + [node("Mul", [xs, f32(0.5)]), node("Mul", [PREV, one_erf])]  # (x * 0.5) * (1 + erf)


gelu("Gelu_none", "Gelu", [X3], kernels=(UNARY,))
gelu("Gelu_explicit_none", "Gelu", [X3], {"approximate": "none"}, kernels=(UNARY,))
gelu("Gelu_tanh", "Gelu", [X3], {"approximate": "tanh"}, kernels=(UNARY,))
gelu("Erf", "Erf", [X3], kernels=(UNARY,))
gelu("ErfGelu_div_x_erf_half", "Div", [X3, f32(RT2)], kernels=(UNARY,), chain=erf_form("x_erf_half"))
gelu("ErfGelu_div_half_x_erf", "Div", [X3, f32(RT2)], kernels=(UNARY,), chain=erf_form("half_x_erf"))
gelu("ErfGelu_mul_erf_half_x", "Mul", [X3, f32(1.0 / RT2)], kernels=(UNARY,), chain=erf_form("erf_half_x"))
gelu("ErfGelu_mul_x_erf_half", "Mul", [f32(1.0 / RT2), X3], kernels=(UNARY,),
     chain=[then("Erf"), then("Add", f32(1.0)), node("Mul", [PREV, ("in", 1)]), node("Mul", [f32(0.5), PREV])])
_pw = [x(2, 6, 9, 11), _c((5, 6, 1, 1), 6 ** -0.5 * 3), _c((5,), 0.1)]  # (outputs of +-3 and beyond)
gelu("Conv_Gelu", "Conv", _pw, kernels=(CONV1,), chain=[then("Gelu")])
gelu("Conv_Gelu_tanh", "Conv", _pw, kernels=(CONV1,), chain=[then("Gelu", approximate="tanh")])
gelu("Conv_ErfGelu", "Conv", _pw, kernels=(CONV1,), chain=[then("Div", f32(RT2))] + erf_form("x_erf_half", first=0))
gelu("Conv_ErfGelu_half_x", "Conv", _pw, kernels=(CONV1,),
     chain=[then("Mul", f32(1.0 / RT2))] + erf_form("half_x_erf", first=0))
gelu("Gemm_Gelu", "Gemm", [("x3", (5, 8)), x(8, 7)], kernels=(GEMM,), chain=[then("Gelu")])
gelu("MatMul_bias_Gelu", "MatMul", [("x3", (2, 5, 8)), _c((8, 7), 8 ** -0.5)], kernels=(GEMM,),
     chain=[then("Add", _c((7,), 0.1)), then("Gelu")])
gelu("MatMul_bias_ErfGelu", "MatMul", [("x3", (2, 5, 8)), _c((8, 7), 8 ** -0.5)], kernels=(GEMM,),
     chain=[then("Add", _c((7,), 0.1)), then("Div", f32(RT2))] + erf_form("x_erf_half", first=1))
# behind a Concat nothing absorbs it: the copies, then its own k_unary
gelu("Concat_Gelu", "Concat", [("x3", (2, 3, 10, 11)), ("x3", (2, 2, 10, 11))], {"axis": 1},
     kernels=("k_copy_rows<", "k_copy_rows<", UNARY), chain=[then("Gelu")])
gelu("Concat_ErfGelu", "Concat", [("x3", (2, 3, 10, 11)), ("x3", (2, 2, 10, 11))], {"axis": 1},
     kernels=("k_copy_rows<", "k_copy_rows<", UNARY), chain=[then("Div", f32(RT2))] + erf_form("half_x_erf", first=0))
# the near miss: 0.7 is not 1 / sqrt 2 — five nodes, five launches, Erf on k_unary
gelu("ErfGelu_near_miss_0p7", "Mul", [X3, f32(0.7)], kernels=(BIN, UNARY, BIN, BIN, BIN), chain=erf_form("x_erf_half"))

# ---- a Linear layer's bias (opset 13) -------------------------------------------------
LI = "linear"
_w87 = _c((8, 7), 8 ** -0.5)


def linear(name, chain, kernels, xs=(2, 5, 8)):
    case(f"Linear_{name}", LI, "MatMul", [x(*xs), _w87], kernels=tuple(kernels), chain=tuple(chain))


linear("bias", [then("Add", _c((7,), 0.3))], [GEMM])
linear("bias_first", [node("Add", [_c((7,), 0.3), PREV])], [GEMM])
linear("bias_111N", [then("Add", _c((1, 1, 7), 0.3))], [GEMM])
linear("bias_relu", [then("Add", _c((7,), 0.3)), then("Relu")], [GEMM])
linear("bias_hardswish_rank2", [then("Add", _c((7,), 0.3)), then("HardSwish")], [GEMM], xs=(19, 8))
# the product has a second reader: the Add stays a launch
linear("bias_second_consumer", [then("Add", _c((7,), 0.3)), node("Mul", [("node", 0), PREV])], [GEMM, BIN, BIN])
# a bias that is no [N]: a launch
linear("bias_per_row", [then("Add", _c((5, 1), 0.3))], [GEMM, BIN])

# ---- attention (opset 13) -------------------------------------------------------------
A = "attn"
ATTN = "k_attn<%d>("
COPY, SOFTMAX = "k_copy", "k_softmax("
UNFUSED = (COPY, GEMM, BIN, SOFTMAX, GEMM)  # Transpose, MatMul, the scale, Softmax, MatMul
SWAP = {"perm": [0, 1, 3, 2]}


def attn_chain(lead, nq, nk, d, dv, scale="mul", bias=None, c_=None, softmax_out=False):
    """The nodes behind the K Transpose (node 0).  scale: mul / div (behind the first MatMul), q / k (a Mul in
    front of it), None; bias: None, ("const", lead dims) or ("run", lead dims)."""
    c_ = float(d) ** -0.5 if c_ is None else c_
    q, v = x(*lead, nq, d), x(*lead, nk, dv)
    chain = []
    meta = {"q": (0, 0) if scale == "q" else (1, 0) if scale == "k" else (0, 0), "bias": None,
            "scale": 1.0 if scale is None else 1.0 / float(np.float32(1.0 / c_)) if scale == "div" else float(np.float32(c_))}
    if scale == "q":
        chain += [node("Mul", [q, f32(c_)]), node("MatMul", [PREV, ("node", 0)])]
    elif scale == "k":
        chain += [node("Mul", [f32(c_), PREV]), node("MatMul", [q, PREV])]
    else:
        chain += [node("MatMul", [q, PREV])]
    if scale == "mul":
        chain.append(then("Mul", f32(c_)))
    elif scale == "div":
        chain.append(then("Div", f32(1.0 / c_)))
    if bias is not None:
        shape = tuple(bias[1]) + (nq, nk)
        chain.append(then("Add", _c(shape, 1.0) if bias[0] == "const" else x(*shape)))
        meta["bias"] = (len(chain) - 1, 0)
    sm = then("Softmax", axis=-1)
    chain.append(also_out(sm) if softmax_out else sm)
    chain.append(node("MatMul", [PREV, v]))
    meta["v"] = (len(chain) - 1, 1)
    return tuple(chain), meta


def attn(name, lead, nq, nk, d, dv=None, kernels=None, perm=None, k_input=None, n_out=1, **kw):
    dv = dv or d
    u = -(-max(d, dv) // 16)
    u = 1 if u <= 1 else 2 if u <= 2 else 4 if u <= 4 else 8
    chain, META[f"Attn_{name}"] = attn_chain(lead, nq, nk, d, dv, **kw)
    case(f"Attn_{name}", A, "Transpose", [k_input or x(*lead, nk, d)], perm or SWAP, n_out=n_out,
         kernels=tuple(kernels) if kernels is not None else (ATTN % u,), chain=chain)


H2, H3 = (2, 2), (2, 3)
attn("q1_k1_d8", H2, 1, 1, 8)
attn("q15_k7_d20_div", H2, 15, 7, 20, scale="div")
attn("q17_k16_d32_on_q", H3, 17, 16, 32, scale="q")
attn("q17_k33_d32_dv20_on_k", H2, 17, 33, 32, dv=20, scale="k")
attn("q70_k33_d64_noscale", H2, 70, 33, 64, scale=None)
attn("q70_k145_d128", H3, 70, 145, 128)
attn("q15_k145_d32_const_bias", H2, 15, 145, 32, bias=("const", (2,)))
attn("q70_k7_d8_runtime_bias", H3, 70, 7, 8, bias=("run", (2, 1)))
attn("q17_k33_d64_bias_no_scale", H2, 17, 33, 64, scale=None, bias=("const", (1, 1)))
attn("q1_k16_d128_full_bias", H2, 1, 16, 128, scale="div", bias=("run", (2, 2)))
# logits of standard deviation 20 (x 3.5 on sqrt(32) ones), the largest beyond +-60: exp of them unsubtracted is inf
attn("q70_k145_d32_logits60", H2, 70, 145, 32, c_=3.5)
attn("q17_k1_d20_logits60_on_q", H2, 17, 1, 20, scale="q", c_=4.5)
# near misses: today's launches, by name
attn("miss_softmax_is_output", H2, 15, 7, 20, softmax_out=True, n_out=2, kernels=UNFUSED)
attn("miss_transpose_other_axes", H2, 15, 7, 20, perm={"perm": [1, 0, 3, 2]}, kernels=UNFUSED)
attn("miss_d6", H2, 15, 7, 6, kernels=UNFUSED)
attn("miss_d132", H2, 15, 7, 132, kernels=UNFUSED)
attn("miss_K_constant", H2, 15, 7, 20, k_input=_c((2, 2, 7, 20), 1.0), kernels=UNFUSED[1:])

# ---- refused at creation, naming the operator -------------------------------------------
R_ = "refused"


def refuse(name, op, inputs, attrs=None, opset=17, **kw):
    case(f"refuse_{name}", R_, op, inputs, attrs, expect="refused", opset=opset, **kw)


_g64, _b64 = _c((64,), 0.1, 1.0), _c((64,), 0.1)
refuse("LayerNorm_runtime_scale", "LayerNormalization", [x(2, 15, 64), x(64), _b64])
refuse("LayerNorm_runtime_bias", "LayerNormalization", [x(2, 15, 64), _g64, x(64)])
refuse("LayerNorm_mean_output_used", "LayerNormalization", [x(2, 15, 64), _g64, _b64], n_out=2)
refuse("LayerNorm_stash_type_0", "LayerNormalization", [x(2, 15, 64), _g64, _b64], {"stash_type": 0})
refuse("LayerNorm_scale_size", "LayerNormalization", [x(2, 15, 64), _c((32,), 0.1)])
refuse("Gelu_approximate_unknown", "Gelu", [X3], {"approximate": "fast"}, opset=20)
# decomposed LayerNorm near misses: the ReduceMean over the last axis is refused as before
refuse("LayerNorm13_d_third_consumer", "ReduceMean", [x(2, 15, 64)], dict(AX), opset=13,
       chain=decomposed("pow", extra=[node("Add", [PREV, ("node", 1)])]))
refuse("LayerNorm13_keepdims0", "ReduceMean", [x(2, 15, 64)], {"axes": [-1], "keepdims": 0}, opset=13,
       chain=decomposed("pow"))
refuse("LayerNorm13_axes_m2", "ReduceMean", [x(2, 15, 64)], {"axes": [-2], "keepdims": 1}, opset=13,
       chain=decomposed("pow"))
# outside the patterns Pow and Sqrt of runtime tensors stay refused
refuse("Pow_runtime", "Pow", [x(2, 15, 64), f32(2.0)], opset=13)
refuse("Sqrt_runtime", "Sqrt", [("pos", (2, 15, 64))], opset=13)

VALUE_CASES = [k for k in CASES if k.expect == "value"]
REFUSED_CASES = [k for k in CASES if k.expect == "refused"]
BY_NAME = {k.name: k for k in CASES}
# the cases one fused launch computes (the float32 restatements of tests/test_attn_ref.py cover them)
FUSED_ATTN = [k for k in VALUE_CASES if k.family == A and k.kernels[0].startswith("k_attn")]
LNORM_CASES = [k for k in VALUE_CASES if k.family in (L, LD)]


def groups():
    """{family: its value cases}; a family has one opset, so one model holds it."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    for fam, ks in out.items():
        assert len({k.opset for k in ks}) == 1, fam
    return out
