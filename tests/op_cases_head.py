"""The operator matrix of the class heads (test infrastructure): Softmax /
LogSoftmax / ArgMax / ReduceMax over the channel axis of [N, C, H, W] logits,
the linear Resize fused in front of them, the channel selections behind a
Softmax, ArgMax -> Equal -> Cast, Gather of a runtime tensor and the Cast of an
index tensor.  op_cases.Case objects packed by build() (op_cases.build, then
the seeded rewrites of the special inputs below), kept in this module's own
list.  Shared by tests/test_head_ref.py (tests/onnx_ref_head.py against PyTorch
in float64 and a float32 restatement of the kernel, CPU) and
tests/test_gpu_head_matrix.py (the GPU sessions against onnx_ref_head).

Batch 2 throughout.  `kernels` names each case's launches, in order.  A case's
META entry restates it for the CPU tests: the Resize in front (`up`), the
reduction (`red`), its attributes, the channels selected, the class compared.

Shapes: C in 1, 2, 3, 5, 19, 21, 150 — both sides of the class loops' unroll
by 2 and by 4; output widths 12 (four pixels per thread, one 16-byte store),
13 and 18 (one pixel per thread); upsampling 6x8 by 2 and by 4, 5x7 to 13x18,
every coordinate transformation, align_corners to one output row.
Values: 3 x standard normal; +-80 (pm80); one input with some — never all —
classes at -inf (seed 2); integer logits in [-8, 8] with repeated maxima (seed
1): behind a 2x or 4x half_pixel upsample the weights are multiples of 1/8, so
every interpolated logit is exact in float32 and float64 alike and the labels
must be exactly the reference's (`exact`).
"""
from __future__ import annotations

import numpy as np

import op_cases as OC
from op_cases import IN0, PREV, Case, also_out, c, ci, node, then, x

CASES: list[Case] = []
META: dict[str, dict] = {}
FUSED: set[str] = set()  # the cases whose k_class_head launch stands for more than its own node (head_nodes())


def HEAD(red, up, quad):
    return f"k_class_head<{red}, {str(bool(up)).lower()}, {str(bool(quad)).lower()}>("


FORMS = [HEAD(r, u, q) for r in (0, 1) for u in (0, 1) for q in (0, 1)]
RESIZE, COPY = "k_resize<", "k_copy"
TIES, NINF = 1, 2  # Case.seed of the rewritten inputs


def _fix_ties(a):
    return np.clip(np.round(a), -8.0, 8.0).astype(np.float32)


def _fix_ninf(a):
    rng = np.random.default_rng(77)
    m = rng.random(a.shape) < 0.35
    m[:, 0] = False  # class 0 stays finite everywhere: never all classes at -inf
    return np.where(m, -np.inf, a).astype(np.float32)


_FIX = {TIES: _fix_ties, NINF: _fix_ninf}


def build(cases):
    """op_cases.build, with input 0 of the cases of seed TIES / NINF rewritten (by name: once per shared input)."""
    cases = list(cases)
    data, feeds, outs = OC.build(cases)
    fixed = set()
    for cs in cases:
        if cs.seed in _FIX and cs.inputs[0][0] != "c":
            n = OC._input_name(cs, 0)
            if n not in fixed:
                feeds[n] = _FIX[cs.seed](feeds[n])
                fixed.add(n)
    return data, feeds, outs


def case(name, family, op, inputs, attrs=None, fused=False, meta=None, **kw):
    assert all(k.name != name for k in CASES), name
    CASES.append(Case(name, family, op, tuple(inputs), dict(attrs or {}), **kw))
    META[name] = dict(meta or {})
    if fused:
        FUSED.add(name)


def quad(w):
    return w % 4 == 0


def red_node(red, **at):
    """(chain node, META) of a reduction over the channel axis."""
    if red == "softmax":
        return then("Softmax", axis=at.get("axis", 1)), {"red": red}
    if red == "logsoftmax":
        return then("LogSoftmax", axis=at.get("axis", 1)), {"red": red}
    if red == "argmax":
        a = {"axis": at.get("axis", 1), "keepdims": at.get("keepdims", 1), "select_last_index": at.get("last", 0)}
        return then("ArgMax", **a), {"red": red, "keepdims": a["keepdims"], "last": a["select_last_index"]}
    a = {"axes": [at.get("axis", 1)], "keepdims": at.get("keepdims", 1)}
    return then("ReduceMax", **a), {"red": "max", "keepdims": a["keepdims"]}


RED_ID = {"softmax": 0, "logsoftmax": 0, "argmax": 1, "max": 1}

# ---- the plain form: each operator alone, one launch ------------------------------------
P = "plain"


def plain(name, red, shape, kind="x3", seed=0, exact=False, **at):
    nd, meta = red_node(red, **at)
    case(f"{name}", P, nd[0], [(kind, tuple(shape))], nd[2], kernels=(HEAD(RED_ID[red], 0, quad(shape[3])),), seed=seed,
         exact=exact, meta=dict(meta, up=None))


for k_, C_ in enumerate((1, 2, 3, 5, 19, 21, 150)):
    wa, wb = (12, 13) if k_ % 2 == 0 else (13, 12)
    plain(f"Softmax_C{C_}_w{wa}", "softmax", (2, C_, 5, wa))
    plain(f"ArgMax_C{C_}_w{wb}", "argmax", (2, C_, 5, wb))
plain("Softmax_C19_w18_axis_m3", "softmax", (2, 19, 3, 18), axis=-3)
plain("LogSoftmax_C5_w12", "logsoftmax", (2, 5, 5, 12))
plain("LogSoftmax_C19_w13_axis_m3", "logsoftmax", (2, 19, 5, 13), axis=-3)
plain("LogSoftmax_C150_w12", "logsoftmax", (2, 150, 3, 12))
plain("ArgMax_C19_w12_last", "argmax", (2, 19, 5, 12), last=1)
plain("ArgMax_C21_w18_keepdims0", "argmax", (2, 21, 3, 18), keepdims=0)
plain("ArgMax_C5_w12_keepdims0_last_axis_m3", "argmax", (2, 5, 5, 12), keepdims=0, last=1, axis=-3)
plain("ReduceMax_C19_w12", "max", (2, 19, 5, 12))
plain("ReduceMax_C5_w13_keepdims0", "max", (2, 5, 5, 13), keepdims=0)
plain("ReduceMax_C150_w18_axis_m3", "max", (2, 150, 3, 18), axis=-3)
# +-80: exp of them unsubtracted overflows
plain("Softmax_pm80_C19_w12", "softmax", (2, 19, 5, 12), kind="pm80")
plain("LogSoftmax_pm80_C21_w13", "logsoftmax", (2, 21, 5, 13), kind="pm80")
# (two classes: with nineteen, half of them near +80, the top two of a pixel are within twice the bar — 0.016 at
# 80 — at some 3 % of the pixels, beyond the cap the label rule allows; test_head_ref.py counts them)
plain("ArgMax_pm80_C2_w13", "argmax", (2, 2, 5, 13), kind="pm80")
plain("ReduceMax_pm80_C19_w12", "max", (2, 19, 5, 12), kind="pm80")
# some classes at -inf (never class 0)
plain("Softmax_ninf_C5_w12", "softmax", (2, 5, 5, 12), seed=NINF)
plain("ArgMax_ninf_C5_w12", "argmax", (2, 5, 5, 12), seed=NINF)
plain("ArgMax_ninf_C5_w12_last", "argmax", (2, 5, 5, 12), seed=NINF, last=1)
plain("ReduceMax_ninf_C5_w12", "max", (2, 5, 5, 12), seed=NINF)
# integer logits with repeated maxima: the labels are exactly the reference's
for C_, w_ in ((5, 12), (19, 13), (150, 12)):
    for last_ in (0, 1):
        plain(f"ArgMax_ties_C{C_}_w{w_}_last{last_}", "argmax", (2, C_, 5, w_), seed=TIES, exact=True, last=last_)

# ReduceMax with its axes as an input (opset 18)
P18 = "plain18"
case("ReduceMax18_C19_w12", P18, "ReduceMax", [("x3", (2, 19, 5, 12)), ci(1)], {"keepdims": 1}, opset=18,
     kernels=(HEAD(1, 0, 1),), meta={"red": "max", "keepdims": 1, "up": None})
case("ReduceMax18_C5_w13_m3_keepdims0", P18, "ReduceMax", [("x3", (2, 5, 5, 13)), ci(-3)], {"keepdims": 0}, opset=18,
     kernels=(HEAD(1, 0, 0),), meta={"red": "max", "keepdims": 0, "up": None})

# ---- fused: the Resize in front, the selections and Equal -> Cast behind ----------------
F = "fused"
CTMS = OC.CTMS


def resize_in(shape, scale=None, sizes=None, kind="x3"):
    if sizes is not None:
        return [(kind, tuple(shape)), None, None, ci(shape[0], shape[1], *sizes)]
    return [(kind, tuple(shape)), None, c([1, 1, scale, scale], np.float32)]


def out_hw(shape, scale=None, sizes=None):
    return tuple(sizes) if sizes is not None else (int(shape[2] * scale), int(shape[3] * scale))


def up(name, red, shape, scale=None, sizes=None, ctm="half_pixel", seed=0, exact=False, tail=(), tail_meta=None,
       family=F, kernels=None, mode="linear", fused=True, n_out=1, softmax_out=False, **at):
    """Resize (the case's operator) -> the reduction [-> tail]."""
    nd, meta = red_node(red, **at)
    if softmax_out:
        nd = also_out(nd)
    wo = out_hw(shape, scale, sizes)[1]
    at_ = {"mode": mode, "coordinate_transformation_mode": ctm}
    if mode == "nearest":
        at_["nearest_mode"] = "floor"
    case(name, family, "Resize", resize_in(shape, scale, sizes), at_, chain=(nd,) + tuple(tail), seed=seed, exact=exact,
         kernels=tuple(kernels) if kernels is not None else (HEAD(RED_ID[red], 1, quad(wo)),), fused=fused, n_out=n_out,
         meta=dict(meta, up={"scale": scale, "sizes": sizes, "ctm": ctm, "mode": mode}, **(tail_meta or {})))


S68, S57 = (2, 3, 6, 8), (2, 21, 5, 7)
for red_ in ("softmax", "logsoftmax", "argmax", "max"):
    up(f"Up2_{red_}_C3", red_, S68, scale=2.0)                       # 12 x 16: four pixels per thread
    up(f"Up13x18_{red_}_C21", red_, S57, sizes=(13, 18))             # a scale that is no power of two, one pixel per thread
up("Up4_softmax_C19", "softmax", (2, 19, 6, 8), scale=4.0)
up("Up4_argmax_C150", "argmax", (2, 150, 6, 8), scale=4.0)
up("Up4_argmax_C19_last", "argmax", (2, 19, 6, 8), scale=4.0, last=1)
up("Up2_max_C150_keepdims0", "max", (2, 150, 6, 8), scale=2.0, keepdims=0)
up("Up2_argmax_C2_w12", "argmax", (2, 2, 5, 6), scale=2.0)           # 10 x 12
up("Up2_softmax_C1_w12", "softmax", (2, 1, 5, 6), scale=2.0)
up("Up_softmax_C5_to13x13", "softmax", (2, 5, 5, 7), sizes=(13, 13))
for ctm_ in CTMS:
    up(f"Up13x18_argmax_C5_{ctm_}", "argmax", (2, 5, 5, 7), sizes=(13, 18), ctm=ctm_)
    up(f"Up2_softmax_C5_{ctm_}", "softmax", (2, 5, 6, 8), scale=2.0, ctm=ctm_)
up("Up_argmax_C5_align_corners_to1x12", "argmax", (2, 5, 5, 7), sizes=(1, 12), ctm="align_corners")
up("Up_softmax_C5_align_corners_to13x1", "softmax", (2, 5, 5, 7), sizes=(13, 1), ctm="align_corners")
up("Up_argmax_C5_pytorch_half_pixel_to1x18", "argmax", (2, 5, 5, 7), sizes=(1, 18), ctm="pytorch_half_pixel")
# ties behind an exact upsample
for sc_ in (2.0, 4.0):
    for last_ in (0, 1):
        up(f"Up{int(sc_)}_argmax_ties_C19_last{last_}", "argmax", (2, 19, 6, 8), scale=sc_, seed=TIES, exact=True, last=last_)
up("Up2_argmax_ties_C5_w18", "argmax", (2, 5, 5, 9), scale=2.0, seed=TIES, exact=True)


def sel_slice(b, e, step=1):
    return node("Slice", [PREV, ci(b), ci(e), ci(1), ci(step)])


def sel_gather(idx, scalar=True):
    return then("Gather", ("c", np.asarray(idx if scalar else [idx], np.int64)), axis=1)


def sel(name, shape, tail, c0, n, drop=False, scale=None, red="softmax"):
    """Softmax [behind a Resize] -> a channel selection: classes [c0, c0 + n), the axis dropped for a scalar Gather."""
    # (copies: the selection's launches when it is not fused — a Split copies every output)
    tm = {"sel": (c0, n, drop), "copies": tail[0][3].get("n", 1) if len(tail[0]) > 3 else 1}
    if scale is not None:
        up(name, red, shape, scale=scale, tail=tail, tail_meta=tm)
        return
    nd, meta = red_node(red)
    case(name, F, nd[0], [("x3", tuple(shape))], nd[2], chain=tuple(tail), kernels=(HEAD(0, 0, quad(shape[3])),),
         fused=True, meta=dict(meta, up=None, **tm))


sel("Softmax_Slice_1_3_C5_w12", (2, 5, 5, 12), [sel_slice(1, 3)], 1, 2)
sel("Softmax_Slice_m1_C19_w13", (2, 19, 5, 13), [sel_slice(-1, 2 ** 40)], 18, 1)
sel("Softmax_Gather_scalar_2_C5_w13", (2, 5, 5, 13), [sel_gather(2)], 2, 1, drop=True)
sel("Softmax_Gather_one_m1_C21_w12", (2, 21, 5, 12), [sel_gather(-1, scalar=False)], 20, 1)
# a Split whose first (last) output alone is used
sel("Softmax_Split_first_C5_w12", (2, 5, 5, 12), [(("Split"), (ci(2, 3),), {"axis": 1}, {"n": 2})], 0, 2)
sel("Softmax_Split_second_C5_w13", (2, 5, 5, 13),
    [("Split", (ci(2, 3),), {"axis": 1}, {"n": 2}), node("Identity", [("node", 1, 1)])], 2, 3)
sel("LogSoftmax_Slice_0_1_C5_w12", (2, 5, 5, 12), [sel_slice(0, 1)], 0, 1, red="logsoftmax")
sel("Up2_Softmax_Gather_15_C21", (2, 21, 6, 8), [sel_gather(15)], 15, 1, drop=True, scale=2.0)
sel("Up4_Softmax_Slice_1_3_C5", (2, 5, 6, 8), [sel_slice(1, 3)], 1, 2, scale=4.0)
sel("Up2_Softmax_Split_first_C3_w18", (2, 3, 5, 9), [("Split", (ci(1, 2),), {"axis": 1}, {"n": 2})], 0, 1, scale=2.0)


def eq_tail(k, dtype):
    return [then("Equal", ("c", np.asarray(k, dtype))), then("Cast", to=1)]


case("ArgMax_Equal_3_Cast_C5_w12", F, "ArgMax", [("x3", (2, 5, 5, 12))], {"axis": 1}, chain=eq_tail(3, np.int64),
     kernels=(HEAD(1, 0, 1),), fused=True, meta={"red": "argmax", "keepdims": 1, "last": 0, "up": None, "eq": 3})
case("ArgMax_Equal_float0_Cast_C19_w13_last", F, "ArgMax", [("x3", (2, 19, 5, 13))], {"axis": 1, "select_last_index": 1},
     chain=[node("Equal", [("c", np.asarray(0.0, np.float32)), PREV]), then("Cast", to=1)],
     kernels=(HEAD(1, 0, 0),), fused=True, meta={"red": "argmax", "keepdims": 1, "last": 1, "up": None, "eq": 0})
up("Up2_ArgMax_Equal_15_C21", "argmax", (2, 21, 6, 8), scale=2.0, tail=eq_tail(15, np.int64), tail_meta={"eq": 15})
up("Up13x18_ArgMax_Equal_1_C3_keepdims0", "argmax", (2, 3, 5, 7), sizes=(13, 18), keepdims=0, tail=eq_tail([1], np.int64),
   tail_meta={"eq": 1})
up("Up2_ArgMax_ties_Equal_0_C5", "argmax", (2, 5, 6, 8), scale=2.0, seed=TIES, exact=True, tail=eq_tail(0, np.int64),
   tail_meta={"eq": 0})

# ---- near misses: separate launches, the same values ------------------------------------
N_ = "miss"
# the Resize read by a second node: materialised by k_resize, each reader on the plain form
up("miss_Resize_read_twice", "softmax", (2, 5, 6, 8), scale=2.0, family=N_, fused=False, n_out=2, softmax_out=True,
   tail=[node("ArgMax", [("node", 0)], axis=1)], kernels=(RESIZE, HEAD(0, 0, 1), HEAD(1, 0, 1)),
   tail_meta={"tail": "argmax_of_resize"})
up("miss_Resize_nearest", "argmax", (2, 5, 6, 8), scale=2.0, family=N_, fused=False, mode="nearest", ctm="asymmetric",
   kernels=(RESIZE, HEAD(1, 0, 1)))
# the Softmax read twice: the Resize is still the head's, the Slice a copy
up("miss_Softmax_read_twice", "softmax", (2, 5, 6, 8), scale=2.0, family=N_, fused=True, n_out=2, softmax_out=True,
   tail=[sel_slice(1, 3)], kernels=(HEAD(0, 1, 1), COPY), tail_meta={"sel_after": (1, 3, 1)})
case("miss_Slice_step2", N_, "Softmax", [("x3", (2, 5, 5, 12))], {"axis": 1}, chain=[sel_slice(0, 5, 2)],
     kernels=(HEAD(0, 0, 1), COPY), meta={"red": "softmax", "up": None, "sel_after": (0, 5, 2)})
# Gather of a runtime tensor: a copy
for ax_, idx_, sc_ in ((0, 1, True), (1, -2, True), (3, 7, False), (1, 0, False)):
    case(f"Gather_axis{ax_}_{'scalar' if sc_ else 'one'}_{idx_}".replace("-", "m"), N_, "Gather",
         [("x3", (2, 5, 6, 12)), ("c", np.asarray(idx_ if sc_ else [idx_], np.int64))], {"axis": ax_}, kernels=(COPY,),
         exact=True, meta={"gather": (ax_, idx_, sc_)})
# Cast of an index tensor: an alias
for to_, nm_ in ((7, "INT64"), (6, "INT32"), (2, "UINT8"), (1, "FLOAT")):
    case(f"ArgMax_Cast_{nm_}", N_, "ArgMax", [("x3", (2, 19, 5, 12))], {"axis": 1, "keepdims": 0}, chain=[then("Cast", to=to_)],
         kernels=(HEAD(1, 0, 1),), meta={"red": "argmax", "keepdims": 0, "last": 0, "up": None})
case("ArgMax_Unsqueeze_Cast_INT64", N_, "ArgMax", [("x3", (2, 19, 5, 13))], {"axis": 1, "keepdims": 0},
     chain=[then("Unsqueeze", ci(1)), then("Cast", to=7)], kernels=(HEAD(1, 0, 0),),
     meta={"red": "argmax", "keepdims": 1, "last": 0, "up": None})

# ---- refused at creation, naming the operator -------------------------------------------
R_ = "refused"
NAMES: dict[str, str] = {}  # refused case -> the operator its message names


def refuse(name, op, inputs, attrs=None, names=None, **kw):
    case(f"refuse_{name}", R_, op, inputs, attrs, expect="refused", **kw)
    NAMES[f"refuse_{name}"] = names or op


X5 = ("x3", (2, 5, 6, 12))
refuse("ArgMax_axis2", "ArgMax", [X5], {"axis": 2})
refuse("ArgMax_rank3", "ArgMax", [("x3", (2, 5, 12))], {"axis": 1})
refuse("LogSoftmax_axis2", "LogSoftmax", [X5], {"axis": 2})
refuse("ReduceMax_axes_2_3", "ReduceMax", [X5], {"axes": [2, 3]})
refuse("Gather_two_indices", "Gather", [X5, ci(0, 2)], {"axis": 1})
refuse("Cast_conv_output_INT64", "Conv", [x(2, 3, 6, 12), OC.cf((4, 3, 1, 1), 901)], chain=[then("Cast", to=7)], names="Cast")
refuse("Equal_outside_pattern", "Equal", [X5, ("c", np.asarray(0.0, np.float32))])

VALUE_CASES = [k for k in CASES if k.expect == "value"]
REFUSED_CASES = [k for k in CASES if k.expect == "refused"]
BY_NAME = {k.name: k for k in CASES}
TIE_CASES = [k for k in VALUE_CASES if k.exact and META[k.name].get("red") == "argmax"]
# the ArgMax cases whose labels are held by the near-tie rule (every one that is no tie case)
LABEL_CASES = [k for k in VALUE_CASES if META[k.name].get("red") == "argmax" and not k.exact]


def groups():
    """{family: its value cases}; a family has one opset, so one model holds it."""
    out: dict[str, list[Case]] = {}
    for k in VALUE_CASES:
        out.setdefault(k.family, []).append(k)
    for fam, ks in out.items():
        assert len({k.opset for k in ks}) == 1, fam
    return out
