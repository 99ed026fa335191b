"""tests/onnx_ref_ext.py — the float64 reference of ConvTranspose, HardSigmoid,
HardSwish and ReduceMean that tests/test_gpu_deconv_matrix.py holds the GPU
sessions to — against PyTorch in float64 on every value case of
tests/op_cases_deconv.py (CPU).

PyTorch's conv_transpose2d gathers; the reference scatters.  It takes
symmetric pads only: a case with other pads is computed unpadded and cropped.
It has no auto_pad or output_shape: those cases must equal the explicit pads
written down for them by hand (op_cases_deconv.EXPLICIT_PADS), bit for bit.
Bar: the reference rounds each node's float64 result to float32 once, so a
case of k nodes may sit k roundings of 2^-24 (relative to values of order 1
or its own size) from the float64 chain: 4 * 2^-24 * max(1, |want|) covers
the three-node cases.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import onnx_ref as R
import onnx_ref_ext as X
import op_cases as OC
import op_cases_deconv as DC

BAR = 4 * 2.0 ** -24


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _torch_node(op, ins, attrs):
    x = ins[0]
    if op == "ConvTranspose":
        w, b = ins[1], ins[2] if len(ins) > 2 else None
        pt, pl, pb, pr = attrs.get("pads", [0, 0, 0, 0])
        kw = dict(stride=tuple(attrs.get("strides", [1, 1])), dilation=tuple(attrs.get("dilations", [1, 1])),
                  groups=attrs.get("group", 1), output_padding=tuple(attrs.get("output_padding", [0, 0])))
        if pt == pb and pl == pr:
            return F.conv_transpose2d(x, w, b, padding=(pt, pl), **kw)
        y = F.conv_transpose2d(x, w, b, **kw)
        return y[:, :, pt:y.shape[2] - pb, pl:y.shape[3] - pr]
    if op == "Conv":
        return F.conv2d(x, ins[1], ins[2] if len(ins) > 2 else None)
    if op == "Gemm":
        return x @ ins[1]
    if op == "HardSigmoid":
        al, be = attrs.get("alpha", 0.2), attrs.get("beta", 0.5)
        return F.hardsigmoid(x) if (al, be) == (1 / 6, 0.5) else torch.clamp(al * x + be, 0.0, 1.0)
    if op == "HardSwish":
        return F.hardswish(x)
    if op == "ReduceMean":
        axes = attrs.get("axes") if len(ins) < 2 else [int(a) for a in ins[1]]
        if not axes:
            return x
        return torch.mean(x, dim=tuple(axes), keepdim=bool(attrs.get("keepdims", 1)))
    if op == "Relu":
        return F.relu(x)
    if op == "Sigmoid":
        return torch.sigmoid(x)
    if op == "PRelu":
        return torch.where(x >= 0, x, x * ins[1])
    if op == "Add":
        return x + ins[1]
    if op == "Mul":
        return x * ins[1]
    if op == "Concat":
        return torch.cat(list(ins), dim=attrs["axis"])
    raise NotImplementedError(op)


def _torch_case(cs, feeds):
    """The outputs of the case's nodes, in order, in float64."""
    ins = [None if a is None else _t(a) for a in OC.operands(cs, feeds)]
    while ins and ins[-1] is None:
        ins.pop()
    made = [_torch_node(cs.op, ins, cs.attrs)]
    for nd, more in zip(cs.chain, OC.chain_operands(cs, feeds)):
        vals = []
        for v in more:
            if isinstance(v, tuple):  # ("prev",) | ("in", k) | ("node", j)
                vals.append(made[-1] if v[0] == "prev" else ins[v[1]] if v[0] == "in" else made[v[1]])
            else:
                vals.append(_t(v))
        whole = len(nd) > 3 and nd[3].get("whole")
        made.append(_torch_node(nd[0], vals if whole else [made[-1]] + vals, nd[2]))
    return made


_ref = {}


def _family(fam):
    """(feeds, {case: its graph outputs}, the reference's outputs) of a family's model, once."""
    if fam not in _ref:
        data, feeds, outs = OC.build(DC.groups()[fam])
        _ref[fam] = (feeds, outs, X.run(R.load(data), feeds))
    return _ref[fam]


def _expressible(cs):
    return not (cs.op == "ConvTranspose" and ("auto_pad" in cs.attrs or "output_shape" in cs.attrs))


@pytest.mark.parametrize("name", [k.name for k in DC.VALUE_CASES if _expressible(k)])
def test_reference_matches_torch(name):
    cs = DC.BY_NAME[name]
    feeds, outs, got = _family(cs.family)
    made = _torch_case(cs, feeds)
    # the case's graph outputs: the last node's, preceded by those a chain node marks "out"
    want = [made[k + 1] for k, nd in enumerate(cs.chain[:-1]) if len(nd) > 3 and nd[3].get("out")] + [made[-1]]
    assert len(want) == len(outs[cs.name])
    for o, w in zip(outs[cs.name], want):
        w = w.numpy()
        assert got[o].shape == w.shape, (o, got[o].shape, w.shape)
        assert got[o].dtype == np.float32
        err = np.abs(got[o].astype(np.float64) - w)
        print(f"{o}: max abs err {float(err.max()):.3e}")
        assert (err <= BAR * np.maximum(1.0, np.abs(w))).all(), (o, float(err.max()))


@pytest.mark.parametrize("name", sorted(DC.EXPLICIT_PADS))
def test_derived_pads_equal_explicit(name):
    cs = DC.BY_NAME[name]
    feeds, outs, got = _family(cs.family)
    xv, w, b = OC.operands(cs, feeds)
    explicit = {k: v for k, v in cs.attrs.items() if k not in ("auto_pad", "output_shape")}
    explicit["pads"] = DC.EXPLICIT_PADS[name]
    assert X.conv_transpose_geometry(xv.shape, w.shape, cs.attrs)[0] == DC.EXPLICIT_PADS[name]
    want = X.conv_transpose(xv, w, b, explicit)
    assert np.array_equal(got[outs[cs.name][0]], want)
    # ... and the explicit form is PyTorch's
    t = _torch_node("ConvTranspose", [_t(xv), _t(w), _t(b)], explicit).numpy()
    assert (np.abs(want - t) <= BAR * np.maximum(1.0, np.abs(t))).all()


def test_auto_pad_valid_and_output_shape_win_over_pads():
    """VALID means zero pads; output_shape makes the pads attribute irrelevant."""
    cs = DC.BY_NAME["ConvTranspose_k3s2_p1_op0_16_16"]
    feeds, _, _ = _family(cs.family)
    xv, w, b = OC.operands(cs, feeds)
    base = {"strides": [2, 2]}
    assert np.array_equal(X.conv_transpose(xv, w, b, {**base, "auto_pad": "VALID", "pads": [1, 1, 1, 1]}),
                          X.conv_transpose(xv, w, b, base))
    assert np.array_equal(X.conv_transpose(xv, w, b, {**base, "output_shape": [10, 13], "pads": [3, 3, 3, 3]}),
                          X.conv_transpose(xv, w, b, {**base, "pads": [1, 1, 0, 1]}))


@pytest.mark.parametrize("name", [k.name for k in DC.REFUSED_CASES])
def test_refused_cases_raise(name):
    data, feeds, _ = OC.build([DC.BY_NAME[name]])
    with pytest.raises(ValueError, match=DC.BY_NAME[name].op):
        X.run(R.load(data), feeds)


def test_other_nodes_go_to_onnx_ref():
    """A node that is none of the four is evaluated by oracle/onnx_ref.py: a model without them gives its outputs."""
    data, feeds, _ = OC.build(OC.groups()["unary"])
    model = R.load(data)
    want, got = R.run(model, feeds), X.run(model, feeds)
    assert want.keys() == got.keys() and all(np.array_equal(want[k], got[k], equal_nan=True) for k in want)
