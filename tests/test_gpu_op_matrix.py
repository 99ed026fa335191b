"""The GPU ONNX sessions (include/vso.h) against the ONNX oracle
(oracle/onnx_ref.py) on the operator matrix (tests/op_cases.py; the oracle
itself is pinned to an independent float64 evaluation of the same cases by
tests/test_op_matrix_oracle.py).  One f32 session per operator family, one
graph output per case.

Bars: data movement, MaxPool, nearest Resize, Relu and Clip (they select among
their inputs' values) compare equal; the rest meet the project's TOL = 1e-4
per element: |gpu - oracle| <= TOL * max(1, |oracle|).  Every session runs
twice: the graph replay is bitwise the same.  The refused cases fail at
session creation with a message naming the operator.

The conv family runs three more ways, each against the same bar.  In bf16 and
f16 sessions the oracle rounds the operands of the convolutions
onnx_ref.tiled_conv names (R.run(conv_operands=...)); the session must launch
k_conv_tile for exactly those cases, and for every other case the kernel of
the f32 session, with bitwise its output.  Under VSO_PW=0 the plain 1x1s move
from k_conv_pw to k_conv_small<true, ...> / k_conv_gemm, under VSO_DW_PLANE=0
the k_conv_dw_plane cases to the four-outputs-per-thread body of k_conv_dw,
whose outputs are bitwise the default's.  Both knobs are read once per
process: each setting is one child process (tests/conv_matrix_child.py), one
at a time, none started after an abnormal end.  One form has no case:
k_conv_dw's conv_dw_body<long> needs 2^30 outputs.  Measured errors per kernel
form and three deliberate breaks these tests catch: profiles/NOTES.md, "Conv
operator matrix".
"""
import math
import re

import numpy as np
import pytest

import conv_matrix_child as C
import onnx_ref as R
import op_cases as OC

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


@pytest.mark.parametrize("family", sorted(OC.groups()))
def test_family_matches_oracle(ort, family):
    cases = OC.groups()[family]
    data, feeds, outs = OC.build(cases)
    want = R.run(R.load(data), feeds)
    with ort.InferenceSession(data, precision="f32") as s:
        got = s.run(feeds)
        again = s.run(feeds)
        print(family, len(cases), "cases,", len(s.launches()), "launches")
    failures = []
    for cs in cases:
        for o in outs[cs.name]:
            g, w = got[o], want[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, oracle {w.shape}")
                continue
            if not np.array_equal(g, again[o], equal_nan=True):
                failures.append(f"{o}: the second run differs from the first")
            err = np.abs(g.astype(np.float64) - w)
            worst = float(err.max()) if err.size else 0.0
            print(f"{o}: max abs err {worst:.3e}{' (exact)' if cs.exact else ''}")
            if cs.exact:
                if not np.array_equal(g, w):
                    failures.append(f"{o}: not equal, max abs err {worst:.3e} in {int((g != w).sum())} elements")
            elif not (err <= TOL * np.maximum(1.0, np.abs(w))).all():
                bad = ~(err <= TOL * np.maximum(1.0, np.abs(w)))
                failures.append(f"{o}: {int(bad.sum())} elements beyond {TOL:g} * max(1, |want|), worst {worst:.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [k.name for k in OC.VALUE_CASES if k.kernels])
def test_kernel_form(ort, name):
    """A session holding the case alone launches the kernel form the case is there to reach."""
    cs = OC.BY_NAME[name]
    data, _, _ = OC.build([cs])
    with ort.InferenceSession(data, precision="f32") as s:
        names = s.launches()
    assert len(names) == len(cs.kernels) and all(k in n for k, n in zip(cs.kernels, names)), (cs.kernels, names)


@pytest.mark.parametrize("name", [k.name for k in OC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = OC.BY_NAME[name]
    data, _, _ = OC.build([cs])
    with pytest.raises(ort.VsoError, match=cs.post[0] if cs.post else cs.op):
        ort.InferenceSession(data, precision="f32").close()


# ---- the conv family: 16-bit sessions and the planner's knobs ------------------
CONV = OC.groups()["conv"]
_conv = {}


def _conv_model():
    if "model" not in _conv:
        _conv["model"] = OC.build(CONV)
    return _conv["model"]


def _conv_oracle(prec):
    """The oracle's outputs of the family, once per precision."""
    if prec not in _conv:
        data, feeds, _ = _conv_model()
        _conv[prec] = R.run(R.load(data), feeds, conv_operands=None if prec == "f32" else prec)
    return _conv[prec]


def _per_case(launches):
    """{case: its launches} of a session of the whole family: the launches come
    in node order, len(case.kernels) for each case."""
    assert len(launches) == sum(len(cs.kernels) for cs in CONV), launches
    out, k = {}, 0
    for cs in CONV:
        assert cs.kernels, cs.name
        out[cs.name] = launches[k:k + len(cs.kernels)]
        k += len(cs.kernels)
    return out


def _beyond_bar(got, want, label, names):
    """The family's outputs against the oracle's at the matrix's bar; the worst
    err / bar per kernel form (as launched: `names`, from _per_case) is printed."""
    failures, worst = [], {}
    for cs in CONV:
        g, w = got[cs.name], want[cs.name]
        if g.shape != w.shape:
            failures.append(f"{cs.name}: shape {g.shape}, oracle {w.shape}")
            continue
        err = np.abs(g.astype(np.float64) - w)
        ratio = float((err / (TOL * np.maximum(1.0, np.abs(w)))).max())
        print(f"{label} {cs.name}: max abs err {float(err.max()):.3e}, err / bar {ratio:.3f}")
        if not (err <= TOL * np.maximum(1.0, np.abs(w))).all():
            bad = ~(err <= TOL * np.maximum(1.0, np.abs(w)))
            failures.append(f"{cs.name}: {int(bad.sum())} elements beyond {TOL:g} * max(1, |want|), "
                            f"worst {float(err.max()):.3e}")
        form = " + ".join(re.search(r"k_\w+(<[^>]*>)?", n).group(0) for n in names[cs.name])
        worst[form] = max(worst.get(form, 0.0), ratio)
    for form, ratio in sorted(worst.items()):
        print(f"{label} worst err / bar, {form}: {ratio:.3f}")
    return failures


@pytest.fixture(scope="module")
def conv_f32(ort):
    """(outputs, {case: launches}) of the family's f32 session in this process, each case on the kernel it names."""
    data, feeds, _ = _conv_model()
    with ort.InferenceSession(data, precision="f32") as s:
        got = s.run(feeds)
        names = _per_case(s.launches())
    for cs in CONV:
        assert all(k in n for k, n in zip(cs.kernels, names[cs.name])), (cs.name, cs.kernels, names[cs.name])
    return got, names


def _tiled(cs):
    """onnx_ref.tiled_conv for the case's convolutions: the operands the oracle rounds in a 16-bit session."""
    convs = [(cs.inputs[1][1], cs.attrs)] + [(ins_[0][1], at_) for op_, ins_, at_ in cs.chain if op_ == "Conv"]
    return any(R.tiled_conv(w, at_) for w, at_ in convs)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_family_16bit(ort, conv_f32, prec):
    data, feeds, _ = _conv_model()
    want = _conv_oracle(prec)
    f32_out, f32_names = conv_f32
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        names = _per_case(s.launches())
    failures = _beyond_bar(got, want, prec, names)
    n_tiled = 0
    for cs in CONV:
        if not np.array_equal(got[cs.name], again[cs.name], equal_nan=True):
            failures.append(f"{cs.name}: the second run differs from the first")
        on_tile = ["k_conv_tile<" in n for n in names[cs.name]]
        if _tiled(cs):
            n_tiled += 1
            if on_tile != [True]:
                failures.append(f"{cs.name}: the oracle rounds its operands, the session launched {names[cs.name]}")
        else:
            if names[cs.name] != f32_names[cs.name]:
                failures.append(f"{cs.name}: launched {names[cs.name]}, in f32 {f32_names[cs.name]}")
            if not np.array_equal(got[cs.name], f32_out[cs.name]):
                failures.append(f"{cs.name}: differs from the f32 session's output")
    # (among them C 3, M 5 on 9x11, which the tile matrix does not run)
    assert n_tiled >= 10 and _tiled(OC.BY_NAME["Conv_small_K27"])
    assert not failures, "\n".join(failures)


def _pw_fallback(cs):
    """The kernel of a plain 1x1 case under VSO_PW=0 (vso_kernels.hip, conv_kind): k_conv_gemm from
    1024 64x64 tiles on, else k_conv_small<true, ...> by its K = C."""
    n, c_, h, w = cs.inputs[0][1]
    m = cs.inputs[1][1].shape[0]
    if math.ceil(h * w / 64) * math.ceil(m / 64) * n >= 1024:
        return "k_conv_gemm("
    return OC.small(True, *((8, False) if c_ <= 32 else (16, False) if c_ <= 64 else (32, False) if c_ <= 128
                            else (16, True)))


KNOBS = {"VSO_PW": re.compile(r"k_conv_pw<\d, 0>\("), "VSO_DW_PLANE": re.compile(r"k_conv_dw_plane<\d>\(")}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_conv_family_knob_off(ort, conv_f32, knob):
    """The family's f32 session in a child process with the knob at 0: the
    cases the knob moves launch the fallback kernel, every other case the
    same one and bitwise the same output; all meet the bar, and with
    VSO_DW_PLANE=0 all are bitwise the default's (the plane form and
    k_conv_dw's body do the same operations in the same order)."""
    f32_out, f32_names = conv_f32
    outs, info = C.run_child(f"{knob}=0", {knob: "0"}, "op_conv:f32")
    inf = info["op_conv/f32"]
    names = _per_case(inf["launches"])
    got = {cs.name: outs[f"op_conv/f32/{cs.name}"] for cs in CONV}
    failures = _beyond_bar(got, _conv_oracle("f32"), f"{knob}=0", names)
    assert inf["rerun_equal"]
    moved = [cs for cs in CONV if len(cs.kernels) == 1 and KNOBS[knob].fullmatch(cs.kernels[0])]
    assert len(moved) >= 2
    for cs in CONV:
        if cs in moved:
            expect = _pw_fallback(cs) if knob == "VSO_PW" else "k_conv_dw("
            if expect not in names[cs.name][0]:
                failures.append(f"{cs.name}: launched {names[cs.name]}, expected {expect}")
        elif names[cs.name] != f32_names[cs.name]:
            failures.append(f"{cs.name}: launched {names[cs.name]}, without the knob {f32_names[cs.name]}")
        if (cs not in moved or knob == "VSO_DW_PLANE") and not np.array_equal(got[cs.name], f32_out[cs.name]):
            failures.append(f"{cs.name}: differs from the default session's output, max "
                            f"{float(np.abs(got[cs.name] - f32_out[cs.name]).max()):.3e}")
    if knob == "VSO_PW":  # both fallbacks are reached
        assert {_pw_fallback(cs) for cs in moved} >= {"k_conv_gemm(", OC.small(True, 8, False), OC.small(True, 16, True)}
    assert not failures, "\n".join(failures)
