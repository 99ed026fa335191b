"""tests/onnx_ref_head.py — the float64 reference the GPU class-head tests are
held to — checked on the CPU, on every value case of tests/op_cases_head.py:

 * against PyTorch in float64 (F.interpolate, softmax, log_softmax, argmax,
   amax), restated from each case's META.  PyTorch has no asymmetric linear
   interpolation and does not pin a one-pixel output to source 0 as
   pytorch_half_pixel does: those three cases are held by the second check only.
 * against a float32 numpy restatement of k_class_head's arithmetic — the
   source coordinate, the taps, resize_lerp's two fmas and three roundings,
   the three softmax passes, the strict (or >=) comparison of the arg forms —
   at the GPU tests' bar and label rule.
 * the near-tie condition, on the reference alone: in every ArgMax case that is
   no tie case, the pixels whose top two logits differ by at most
   2 x 1e-4 x max(1, |top|) number at most 1 % of the case.  So the GPU tests'
   cap on labels that may differ is one the draws leave room for.

Bars.  Reference against PyTorch: the reference rounds to float32 once per
node, PyTorch never; a case has at most two roundings between input and output
(the Resize's result, the head's), each at most 2^-24 of a magnitude up to
L = max(1, the largest finite |input|), and the first is doubled by the
subtraction of the maximum: |ref - torch| <= 4 x 2^-24 x L.  Labels may differ
from PyTorch's only where its top two logits are closer than that.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import onnx_ref as R
import onnx_ref_head as RH
import op_cases as OC
import op_cases_head as HC

TOL = 1e-4
NEAR_TIE_SHARE = 0.01
NO_TORCH = {"Up13x18_argmax_C5_asymmetric": "no asymmetric linear interpolation in PyTorch",
            "Up2_softmax_C5_asymmetric": "no asymmetric linear interpolation in PyTorch",
            "Up_argmax_C5_pytorch_half_pixel_to1x18": "PyTorch does not pin a one-pixel output to source 0"}
_fam = {}


def family(fam):
    """(feeds, {case: outputs}, model, every reference value) of a family, once."""
    if fam not in _fam:
        data, feeds, outs = HC.build(HC.groups()[fam])
        m = R.load(data)
        _fam[fam] = (feeds, outs, m, RH.run_all(m, feeds))
    return _fam[fam]


def case_input(cs, feeds):
    return feeds[OC._input_name(cs, 0)]


RED_CASES = [k for k in HC.VALUE_CASES if "red" in HC.META[k.name]]


# ---- PyTorch, float64 -------------------------------------------------------------------
def torch_outputs(cs, x):
    """The case's graph outputs, in order, from PyTorch in float64."""
    m = HC.META[cs.name]
    t = torch.from_numpy(x).double()
    if m["up"]:
        u = m["up"]
        kw = {"size": tuple(u["sizes"])} if u["sizes"] is not None else {"scale_factor": u["scale"]}
        if u["mode"] == "nearest":
            t = TF.interpolate(t, mode="nearest", **kw)
        else:
            t = TF.interpolate(t, mode="bilinear", align_corners=u["ctm"] == "align_corners", **kw)
    logits = t
    red = m["red"]
    if red == "softmax":
        y = torch.softmax(t, 1)
    elif red == "logsoftmax":
        y = torch.log_softmax(t, 1)
    elif red == "max":
        y = torch.amax(t, 1, keepdim=bool(m["keepdims"]))
    else:
        C = t.shape[1]
        y = C - 1 - torch.argmax(torch.flip(t, [1]), 1, keepdim=True) if m["last"] else torch.argmax(t, 1, keepdim=True)
        if "eq" in m:
            y = (y == m["eq"]).double()
        if not m["keepdims"]:
            y = y.squeeze(1)
    outs = [y]
    if "sel" in m:
        c0, n, drop = m["sel"]
        y = y[:, c0:c0 + n]
        outs = [y.squeeze(1) if drop else y]
    if "sel_after" in m:
        b, e, st = m["sel_after"]
        outs = ([y] if cs.n_out == 2 else []) + [y[:, b:e:st]]
    if m.get("tail") == "argmax_of_resize":
        outs = [y, torch.argmax(logits, 1, keepdim=True)]
    return [o.numpy() for o in outs], logits.numpy()


@pytest.mark.parametrize("name", [k.name for k in RED_CASES if k.name not in NO_TORCH])
def test_reference_matches_pytorch(name):
    cs = HC.BY_NAME[name]
    feeds, outs, model, env = family(cs.family)
    x = case_input(cs, feeds)
    want, logits = torch_outputs(cs, x)
    L = max(1.0, float(np.abs(x[np.isfinite(x)]).max()))
    bar = 4.0 * 2.0 ** -24 * L
    assert len(want) == len(outs[cs.name])
    for o, w in zip(outs[cs.name], want):
        r = env[o]
        assert r.shape == w.shape, (o, r.shape, w.shape)
        if RH.label_source(model, o) is not None:
            bad = r.astype(np.float64) != w.astype(np.float64)
            if cs.exact:
                assert not bad.any(), f"{o}: {int(bad.sum())} labels differ in a tie case"
                continue
            top2 = np.sort(logits, axis=1)[:, -2:] if logits.shape[1] > 1 else None
            gap = (top2[:, 1] - top2[:, 0]) if top2 is not None else np.full(logits[:, 0].shape, np.inf)
            assert not (bad.reshape(gap.shape) & (gap > bar)).any(), f"{o}: labels differ from PyTorch's where it has no near tie"
            continue
        same = r.astype(np.float64) == w
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(r.astype(np.float64) - w))
        print(f"{o}: max |ref - torch| {float(err.max()):.3e}, bar {bar:.3e}")
        assert (err <= bar).all(), (o, float(err.max()), bar)


def test_gather_and_cast_reference():
    """Gather is numpy's take (negative indices counted from the end, a scalar index dropping the axis); the Cast
    of a label plane keeps the integers."""
    feeds, outs, model, env = family(HC.N_)
    for cs in HC.groups()[HC.N_]:
        m = HC.META[cs.name]
        if "gather" in m:
            ax, idx, scalar = m["gather"]
            x = case_input(cs, feeds)
            w = np.take(x, idx % x.shape[ax] if scalar else [idx % x.shape[ax]], axis=ax)
            assert np.array_equal(env[outs[cs.name][0]], w), cs.name
    i64, i32, u8, f = (env[f"ArgMax_Cast_{n}"] for n in ("INT64", "INT32", "UINT8", "FLOAT"))
    assert i64.dtype == np.int64 and i32.dtype == np.int32 and u8.dtype == np.uint8 and f.dtype == np.float32
    assert np.array_equal(i64, i32) and np.array_equal(i64, u8) and np.array_equal(i64, f)


# ---- the kernel's arithmetic, float32 ---------------------------------------------------
F32 = np.float32


def fma32(a, b, c):
    """round32(a b + c): the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def resize_src32(o, scale, n_in, n_out, ctm):
    """resize_src_fast of vso_resize.h on an index vector, in float32."""
    o = o.astype(F32)
    scale = F32(scale)
    pow2 = np.frexp(scale)[0] == 0.5
    if ctm in ("half_pixel", "pytorch_half_pixel"):
        if ctm == "pytorch_half_pixel" and n_out <= 1:
            return np.zeros(o.shape, F32)
        if pow2:
            return fma32(o + F32(0.5), np.full(o.shape, F32(1.0) / scale, F32), np.full(o.shape, F32(-0.5)))
        return (o + F32(0.5)) / scale - F32(0.5)
    if ctm == "align_corners":
        return o * F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else np.zeros(o.shape, F32)
    return o / scale


def taps32(f, n_in):
    s = np.minimum(np.maximum(f, F32(0.0)), F32(n_in - 1))
    i0 = s.astype(np.int32)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0.astype(F32)


def logits32(cs, x):
    """The logits a head reads: x, or its linear Resize with resize_row / resize_col_taps / resize_lerp's arithmetic."""
    u = HC.META[cs.name]["up"]
    if not u or u["mode"] != "linear":
        return None if u else x
    N, C, H, W = x.shape
    if u["sizes"] is not None:
        Ho, Wo = u["sizes"]
        sy, sx = F32(Ho) / F32(H), F32(Wo) / F32(W)
    else:
        sy = sx = F32(u["scale"])
        Ho, Wo = int(np.floor(H * float(sy))), int(np.floor(W * float(sx)))
    y0, y1, ly = taps32(resize_src32(np.arange(Ho), sy, H, Ho, u["ctm"]), H)
    x0, x1, lx = taps32(resize_src32(np.arange(Wo), sx, W, Wo, u["ctm"]), W)
    ly, lx = ly[:, None], lx[None, :]
    v00, v01 = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    v10, v11 = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    lxb, lyb = np.broadcast_to(lx, v00.shape), np.broadcast_to(ly, v00.shape)
    top = fma32(lxb, v01, (F32(1.0) - lxb) * v00)
    bot = fma32(F32(1.0) - lxb, v10, lxb * v11)
    return ((F32(1.0) - lyb) * top + lyb * bot).astype(F32)


def head32(cs, v):
    """k_class_head's reduction of float32 logits v [N, C, H, W], class by class in float32."""
    m = HC.META[cs.name]
    C = v.shape[1]
    if m["red"] in ("softmax", "logsoftmax"):
        mx = np.full(v[:, 0].shape, -np.inf, F32)
        for k in range(C):
            mx = np.maximum(mx, v[:, k])
        s = np.zeros(mx.shape, F32)
        for k in range(C):
            s = (s + np.exp(v[:, k] - mx, dtype=F32)).astype(F32)
        c0, n, drop = m.get("sel", (0, C, False))
        if m["red"] == "logsoftmax":
            ls = np.log(s, dtype=F32)
            y = np.stack([v[:, c0 + k] - mx - ls for k in range(n)], 1)
        else:
            y = np.stack([np.exp(v[:, c0 + k] - mx, dtype=F32) / s for k in range(n)], 1)
        return y[:, 0] if drop else y
    best, idx = v[:, 0].copy(), np.zeros(v[:, 0].shape, np.int64)
    for k in range(1, C):
        take = v[:, k] >= best if m.get("last") else v[:, k] > best
        best = np.where(take, v[:, k], best)
        idx = np.where(take, k, idx)
    y = best if m["red"] == "max" else (idx == m["eq"]).astype(F32) if "eq" in m else idx.astype(F32)
    return y[:, None] if m["keepdims"] else y


# (a nearest Resize is k_resize's alone — the head reads its output — so that near miss is not restated)
@pytest.mark.parametrize("name", [k.name for k in RED_CASES if not (HC.META[k.name]["up"] or {}).get("mode") == "nearest"])
def test_float32_restatement_meets_the_gpu_bar(name):
    cs = HC.BY_NAME[name]
    feeds, outs, model, env = family(cs.family)
    v = logits32(cs, case_input(cs, feeds))
    with np.errstate(invalid="ignore", over="ignore"):
        g = head32(cs, v)
    m = HC.META[cs.name]
    o = outs[cs.name][0] if (cs.n_out == 2 and "sel_after" in m) or m.get("tail") else outs[cs.name][-1]
    if "sel_after" in m and cs.n_out == 1:
        b, e, st = m["sel_after"]
        g = g[:, b:e:st]
    w = env[o]
    assert g.shape == w.shape, (o, g.shape, w.shape)
    src = RH.label_source(model, o)
    if src is not None:
        bad = g.astype(np.float64) != w.astype(np.float64)
        if cs.exact:
            assert not bad.any(), f"{o}: {int(bad.sum())} labels differ in a tie case"
            return
        logits = env[src[0]].astype(np.float64)
        top = logits.max(axis=1)
        bar = TOL * np.maximum(1.0, np.abs(top))
        if src[1] is None:
            at = np.take_along_axis(logits, g.reshape(top.shape).astype(np.int64)[:, None], axis=1)[:, 0]
        else:
            at = logits[:, int(src[1])]
        assert not (bad.reshape(top.shape) & ~(top - at <= bar)).any() and bad.sum() <= NEAR_TIE_SHARE * bad.size, o
        return
    w = w.astype(np.float64)
    same = g == w
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(g.astype(np.float64) - w))
    bar = TOL * np.maximum(1.0, np.abs(np.where(np.isfinite(w), w, 0.0)))
    print(f"{o}: max |f32 - ref| {float(err.max()):.3e}, err / bar {float((err / bar).max()):.4f}")
    assert (err <= bar).all(), (o, float(err.max()))
    if cs.exact:
        assert np.array_equal(g, w.astype(F32)), o


# ---- near ties, on the reference alone --------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in HC.LABEL_CASES])
def test_near_ties_are_rare_in_the_reference(name):
    cs = HC.BY_NAME[name]
    _, outs, model, env = family(cs.family)
    o = [q for q in outs[cs.name] if RH.label_source(model, q) is not None][-1]
    logits = env[RH.label_source(model, o)[0]].astype(np.float64)
    if logits.shape[1] < 2:
        return
    top2 = np.sort(logits, axis=1)[:, -2:]
    near = (top2[:, 1] - top2[:, 0]) <= 2.0 * TOL * np.maximum(1.0, np.abs(top2[:, 1]))
    print(f"{name}: {int(near.sum())} of {near.size} pixels have their top two logits within twice the bar")
    assert near.sum() <= NEAR_TIE_SHARE * near.size, (int(near.sum()), near.size)
