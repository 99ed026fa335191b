"""The oracle of the fusion matrix (oracle/onnx_ref.py, with tests/onnx_ref_ext.py
for ConvTranspose and HardSigmoid: op_cases_fuse.oracle) against PyTorch in
float64 on every value case of tests/op_cases_fuse.py (CPU) — the reference
tests/test_gpu_fuse_matrix.py holds the GPU sessions to.

Each case's model is evaluated node by node with torch: conv2d,
conv_transpose2d, max_pool2d, avg_pool2d, pad, cat, interpolate and
elementwise arithmetic in float64, from the same feeds.  Bar, as in
tests/test_deconv_ref.py: the oracle rounds each node's float64 result to
float32 once, so a case of k nodes may sit k roundings of 2^-24 (relative to
values of order 1 or its own size) from the float64 chain — 4 * 2^-24 *
max(1, |want|) for up to four nodes, k * 2^-24 beyond (the inverted-residual
chains have six or seven).  MaxPool, Pad and Concat move or select float32
values: on the oracle's own inputs of the node, torch gives exactly the
oracle's output.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import onnx_ref as R
import op_cases as OC
import op_cases_fuse as FC

ULP = 2.0 ** -24


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _pool_args(x, a):
    """x padded as the node's pads say (-inf never wins a max; an AveragePool here has none), and the kwargs."""
    pt, pl, pb, pr = a.get("pads", [0, 0, 0, 0])
    if pt or pl or pb or pr:
        x = F.pad(x, (pl, pr, pt, pb), value=float("-inf"))
    return x, dict(kernel_size=tuple(a["kernel_shape"]), stride=tuple(a.get("strides", [1, 1])),
                   ceil_mode=bool(a.get("ceil_mode", 0)))


def torch_node(op, ins, a):
    x = ins[0]
    if op == "Conv":
        pt, pl, pb, pr = a.get("pads", [0, 0, 0, 0])
        return F.conv2d(F.pad(x, (pl, pr, pt, pb)), ins[1], ins[2] if len(ins) > 2 else None,
                        stride=tuple(a.get("strides", [1, 1])), dilation=tuple(a.get("dilations", [1, 1])),
                        groups=a.get("group", 1))
    if op == "ConvTranspose":
        pt, pl, pb, pr = a.get("pads", [0, 0, 0, 0])
        assert pt == pb and pl == pr
        return F.conv_transpose2d(x, ins[1], ins[2] if len(ins) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                                  padding=(pt, pl), groups=a.get("group", 1))
    if op == "MaxPool":
        xp, kw = _pool_args(x, a)
        return F.max_pool2d(xp, dilation=tuple(a.get("dilations", [1, 1])), **kw)
    if op == "AveragePool":
        assert not any(a.get("pads", [0]))
        return F.avg_pool2d(x, **_pool_args(x, a)[1])
    if op == "Pad":
        pads = [int(v) for v in ins[1]]
        value = float(ins[2]) if len(ins) > 2 and ins[2] is not None else 0.0
        axes = [int(v) for v in ins[3]] if len(ins) > 3 and ins[3] is not None else list(range(x.ndim))
        per = {ax: (pads[k], pads[k + len(axes)]) for k, ax in enumerate(axes)}
        flat = []
        for d in range(x.ndim - 1, -1, -1):  # F.pad lists the last dimension first
            flat += list(per.get(d, (0, 0)))
        return F.pad(x, flat, value=value)
    if op == "Concat":
        return torch.cat(list(ins), dim=a["axis"])
    if op == "Resize":
        scales = [float(v) for v in ins[2]]
        assert scales[:2] == [1.0, 1.0]
        if a.get("mode", "nearest") == "nearest":  # (2x, half_pixel, round_prefer_floor: floor(o / 2), torch's rule)
            assert scales[2:] == [2.0, 2.0]
            return F.interpolate(x, scale_factor=(2.0, 2.0), mode="nearest")
        assert a["coordinate_transformation_mode"] in ("half_pixel", "pytorch_half_pixel")
        return F.interpolate(x, scale_factor=tuple(scales[2:]), mode="bilinear", align_corners=False)
    if op == "Reshape":
        return x.reshape([int(v) for v in ins[1]])
    if op in ("Add", "Mul"):
        return x + ins[1] if op == "Add" else x * ins[1]
    if op == "Relu":
        return F.relu(x)
    if op == "LeakyRelu":
        return F.leaky_relu(x, a.get("alpha", 0.01))
    if op == "PRelu":
        return torch.where(x >= 0, x, x * ins[1])
    if op == "Clip":
        lo = float(ins[1]) if len(ins) > 1 and ins[1] is not None else float("-inf")
        hi = float(ins[2]) if len(ins) > 2 and ins[2] is not None else float("inf")
        return torch.clamp(x, lo, hi)
    if op == "Sigmoid":
        return torch.sigmoid(x)
    if op == "HardSigmoid":
        return torch.clamp(a.get("alpha", 0.2) * x + a.get("beta", 0.5), 0.0, 1.0)
    raise NotImplementedError(op)


def torch_run(model, feeds):
    """{value name: float64 tensor} of every node of `model`, in node order."""
    env = {k: _t(v) for k, v in model.inits.items()}
    env.update({k: _t(v) for k, v in feeds.items()})
    for nd in model.nodes:
        ins = [env[i] if i else None for i in nd["inputs"]]
        while ins and ins[-1] is None:
            ins.pop()
        env[nd["outputs"][0]] = torch_node(nd["op"], ins, nd["attrs"])
    return env


@pytest.mark.parametrize("name", [k.name for k in FC.VALUE_CASES])
def test_oracle_matches_torch(name):
    cs = FC.BY_NAME[name]
    data, feeds, outs = OC.build([cs])
    model = R.load(data)
    values = [nd["outputs"][0] for nd in model.nodes]
    got = FC.oracle(model, feeds, want=values)
    made = torch_run(model, feeds)
    bar = max(4, len(model.nodes)) * ULP
    for o in outs[cs.name]:
        if o in feeds:
            continue
        want = made[o].numpy()
        assert got[o].shape == want.shape, (o, got[o].shape, want.shape)
        assert got[o].dtype == np.float32
        err = np.abs(got[o].astype(np.float64) - want)
        print(f"{o}: max abs err {float(err.max()):.3e}, bar {bar:.3e} * max(1, |want|)")
        assert (err <= bar * np.maximum(1.0, np.abs(want))).all(), (o, float(err.max()))
    # the data movement: exact on the oracle's own inputs
    env = dict(model.inits)
    env.update(feeds)
    env.update(got)
    for nd in model.nodes:
        if nd["op"] not in ("MaxPool", "Pad", "Concat"):
            continue
        ins = [None if not i else _t(env[i]) if np.asarray(env[i]).dtype.kind == "f" else env[i] for i in nd["inputs"]]
        while ins and ins[-1] is None:
            ins.pop()
        want = torch_node(nd["op"], ins, nd["attrs"]).numpy()
        assert np.array_equal(got[nd["outputs"][0]].astype(np.float64), want), (name, nd["op"])


def test_table_covers_the_forms():
    """Every kernel form and deferred state the matrix is there for has a case naming it."""
    f32 = {k for cs in FC.VALUE_CASES for k in cs.kernels}
    b16 = {k for cs in FC.VALUE_CASES for k in cs.kernels16}
    res = {k for cs in FC.groups()["res"] if "miss" not in cs.name for k in cs.kernels}
    assert res >= {FC.S8, FC.S16S, FC.S32, OC.small(True, 8, False), FC.pw(0, 5), FC.pw(0, 20), FC.pw(0, 40), FC.pw(3, 65),
                   FC.DW, FC.DWPW, FC.GEMM, FC.TILE, "k_conv_dw_plane<2>("} | {f"k_conv_thin<{m}>(" for m in (1, 2, 3, 4)}
    assert f32 >= {FC.RS_Q, FC.RS_1, "k_deconv_tile<1>(", "k_deconv_direct(", "k_conv_dw_plane<1>("}
    assert {FC.TILE_UP, FC.TILE} <= b16
    assert sum("miss" in cs.name for cs in FC.groups()["res"]) >= 14
    for name, parts in FC.CAT.items():
        if parts is not None:
            assert any(p[0] == "P" for p in parts) and any(p[0] == "in" for p in parts), name
