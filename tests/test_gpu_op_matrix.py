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

The ir family (one MobileNetV2 inverted residual per case, csrc/vso_ir.hip)
runs in f32 with the other families — k_ir and k_ir_reduce by `kernels`, the
near misses on the generic plan — and here in bf16 and f16 sessions
(`kernels16`: k_ir_b16; one oracle, no operand of the family is rounded) and
under each of try_plan_ir's knobs in a child process.  Figures and three
breaks of vso_ir.hip that only these tests catch: profiles/NOTES.md, "IR
block matrix".

The inorm and ibn families (InstanceNormalization alone; MODNet's IBNorm
pattern, fused by find_ibnorm, through each of its consumers) run in f32 with
the other families — every k_norm_plane instance in its float4 and scalar
form, k_norm_stats + k_norm_apply up to 129 pieces, k_conv_thin behind a
deferred norm — and here under VSO_NORM_PLANE=0 and VSO_THIN=0 in child
processes and in bf16 and f16 sessions (the ibn16 cases against the oracle
that rounds the conv's operands).  Figures and the value-only breaks of
vso_kernels.hip / vso_plan.hip that only these tests catch:
profiles/NOTES.md, "Norm operator matrix".
"""
import math
import re
import time

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


def _per_case(launches, cases=CONV, field="kernels"):
    """{case: its launches} of a session of the whole family: the launches come
    in node order, len(case.kernels) (or of another `field`) for each case."""
    assert len(launches) == sum(len(getattr(cs, field)) for cs in cases), launches
    out, k = {}, 0
    for cs in cases:
        assert getattr(cs, field), cs.name
        out[cs.name] = launches[k:k + len(getattr(cs, field))]
        k += len(getattr(cs, field))
    return out


def _beyond_bar(got, want, label, names, cases=CONV, outs=None):
    """The family's outputs (`outs`: {case: its graph outputs}, one of the case's name if None)
    against the oracle's at the matrix's bar; the worst err / bar per kernel
    form (as launched: `names`, from _per_case) is printed."""
    failures, worst = [], {}
    for cs in cases:
        ratio = 0.0
        for o in outs[cs.name] if outs else [cs.name]:
            g, w = got[o], want[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, oracle {w.shape}")
                continue
            err = np.abs(g.astype(np.float64) - w)
            ratio = max(ratio, float((err / (TOL * np.maximum(1.0, np.abs(w)))).max()))
            print(f"{label} {o}: max abs err {float(err.max()):.3e}, err / bar {ratio:.3f}")
            if not (err <= TOL * np.maximum(1.0, np.abs(w))).all():
                bad = ~(err <= TOL * np.maximum(1.0, np.abs(w)))
                failures.append(f"{o}: {int(bad.sum())} elements beyond {TOL:g} * max(1, |want|), "
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


# ---- the ir family: 16-bit sessions and the planner's knobs ---------------------
IR_FAMILIES = ("ir", "ir6")  # (one opset per model: the attribute-form Clips are a family of their own)
IR = [cs for fam in IR_FAMILIES for cs in OC.groups()[fam]]
IR_FUSED16 = [cs for cs in IR if "k_ir" in cs.kernels16[0]]
_ir = {}


def _ir_models():
    """{family: (model, feeds, {case: its graph outputs})}, and the f64 oracle's outputs of both
    (no convolution of the family is one onnx_ref.tiled_conv rounds: one oracle for every precision)."""
    if "models" not in _ir:
        _ir["models"] = {fam: OC.build(OC.groups()[fam]) for fam in IR_FAMILIES}
        _ir["outs"] = {k: v for m in _ir["models"].values() for k, v in m[2].items()}
        _ir["want"] = {k: v for data, feeds, _ in _ir["models"].values() for k, v in R.run(R.load(data), feeds).items()}
    return _ir["models"]


def _ir_sessions(ort, prec):
    """(outputs, launches in order, ir_blocks, whether a second run was bitwise the same) of both
    families' sessions in this process, once per precision."""
    if prec not in _ir:
        got, launches, blocks, same = {}, [], 0, True
        t0 = time.perf_counter()
        for fam, (data, feeds, _) in _ir_models().items():
            with ort.InferenceSession(data, precision=prec) as s:
                out = s.run(feeds)
                again = s.run(feeds)
                same = same and all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)
                got.update(out)
                launches += s.launches()
                blocks += s.ir_blocks()
        print(f"ir family, {prec} sessions: {time.perf_counter() - t0:.2f} s, {len(launches)} launches")
        _ir[prec] = (got, launches, blocks, same)
    return _ir[prec]


def _expect_launches(names, expect, failures):
    """Each case's launches against the parts of their names in `expect` ({case: tuple})."""
    for cs in IR:
        if len(names[cs.name]) != len(expect[cs.name]) or not all(k in n for k, n in zip(expect[cs.name], names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {expect[cs.name]}")


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_ir_family_16bit(ort, prec):
    """A bf16 / f16 session of the whole family: every case at the bar against
    the f64 oracle, on the launches it writes down (kernels16), a second run
    bitwise the same, ir_blocks() the number of fused cases' blocks — and the
    two precisions bitwise equal (k_ir_b16 splits into bf16 in both)."""
    _ir_models()
    got, launches, blocks, same = _ir_sessions(ort, prec)
    names = _per_case(launches, IR, "kernels16")
    failures = _beyond_bar(got, _ir["want"], prec, names, IR, _ir["outs"])
    _expect_launches(names, {cs.name: cs.kernels16 for cs in IR}, failures)
    assert same, "the second run differs from the first"
    assert blocks == sum(sum("k_ir_b16<" in k for k in cs.kernels16) for cs in IR), blocks
    other = _ir_sessions(ort, "f16" if prec == "bf16" else "bf16")[0]
    for o, g in got.items():
        if not np.array_equal(g, other[o], equal_nan=True):
            failures.append(f"{o}: the bf16 and f16 sessions differ")
    assert not failures, "\n".join(failures)


def _drop_reduce(cs, field, keep=()):
    return tuple(k for k in getattr(cs, field) if k != "k_ir_reduce(" or cs.name in keep)


# VSO_IR_KS1=1 (one slice from one workgroup on): a case keeps k_ir_reduce where all its chunks' weights do not
# fit the 160 KiB of LDS beside the hidden planes — ir_slab_plan steps the slice down two chunks at a time.  By
# its arithmetic (slab = 2 cps 16 (4 ceil(CIN / 32) + 2) 16 + 2 ceil(COUT / 16) 16 (4 ceil(cps / 2) + 2) 16 + 44
# cps 16 bytes, + 14336 at stride 1 | 39040 at stride 2): every case of HID >= 288 here; HID <= 192 fits whole.
KS1_KEEPS = {"IR_64_64_res", "IR_64_96", "IR_96_96_res", "IR_96_160_s2", "IR_160_160_res_3x5", "IR_160_320_3x5",
             "IR_160_320_3x5_n26", "IR_64_64_s2_3x5", "IR_96_96_s2_3x5_even", "IR_52_52_res", "IR_84_81", "IR_148_305",
             "IR_48_64_s1"}


def _wave(cs):
    """kernels16 under VSO_IR_WAVE=1: k_ir_b16w for the fused cases of at most 64 input channels
    (each of their forms is in kIr16w), the same slices."""
    if cs not in IR_FUSED16 or cs.inputs[0][1][1] > 64:
        return cs.kernels16
    return tuple(re.sub(r"k_ir_b16<(\d+, \d+, \d), 4>\(", r"k_ir_b16w<\1>(", k) for k in cs.kernels16)


IR_KNOBS = {
    # setting: (session precision, {case: launches})
    "VSO_IR=0": ("f32", None),
    "VSO_IR_WGS=1": ("f32", lambda cs: _drop_reduce(cs, "kernels")),
    "VSO_IR_B16=0": ("bf16", lambda cs: cs.kernels),
    "VSO_IR_WAVE=1": ("bf16", _wave),
    "VSO_IR_KS1=1": ("bf16", lambda cs: _drop_reduce(cs, "kernels16", KS1_KEEPS)),
    # the workgroup target alone ((512 + wg0 / 2) / wg0 slices, then whole pairs): the slices of the default
    # but on the 36 x 304 plane (342 workgroups: one slice)
    "VSO_IR_CPS=0": ("bf16", lambda cs: cs.kernels16[:1] if cs.name == "IR_24_24_res_hid144_36x304" else cs.kernels16),
}


@pytest.mark.parametrize("setting", sorted(IR_KNOBS))
def test_ir_family_knob(ort, setting):
    """The family under one setting of try_plan_ir's knobs (read once per
    process: a child process each, one at a time, none after an abnormal end):
    every case at the bar, on the launches the setting implies.  VSO_IR_B16=0
    in a bf16 session is the f32 session bitwise (the same kernels on the same
    operands); VSO_IR_WAVE=1 is the default bf16 session bitwise (k_ir_b16w:
    the same operands, products and sums as k_ir_b16)."""
    prec, expect = IR_KNOBS[setting]
    _ir_models()
    knob, value = setting.split("=")
    t0 = time.perf_counter()
    outs, info = C.run_child(setting, {knob: value}, ";".join(f"op_{fam}:{prec}" for fam in IR_FAMILIES))
    print(f"ir family, {setting} {prec} child: {time.perf_counter() - t0:.2f} s")
    got = {o: outs[f"op_{cs.family}/{prec}/{o}"] for cs in IR for o in _ir["outs"][cs.name]}
    launches = [n for fam in IR_FAMILIES for n in info[f"op_{fam}/{prec}"]["launches"]]
    blocks = sum(info[f"op_{fam}/{prec}"]["ir_blocks"] for fam in IR_FAMILIES)
    assert all(info[f"op_{fam}/{prec}"]["rerun_equal"] for fam in IR_FAMILIES)
    failures = []
    if expect is None:  # no fused block: the launches are the generic plan's, whatever their number
        assert blocks == 0 and launches and not any("k_ir" in n for n in launches), launches
        for cs in IR:
            for o in _ir["outs"][cs.name]:
                err = np.abs(got[o].astype(np.float64) - _ir["want"][o])
                if not (err <= TOL * np.maximum(1.0, np.abs(_ir["want"][o]))).all():
                    failures.append(f"{o}: beyond the bar, worst {float(err.max()):.3e}")
    else:
        want_names = {cs.name: expect(cs) for cs in IR}
        assert len(launches) == sum(len(v) for v in want_names.values()), launches
        names, k = {}, 0
        for cs in IR:
            names[cs.name] = launches[k:k + len(want_names[cs.name])]
            k += len(names[cs.name])
        failures = _beyond_bar(got, _ir["want"], setting, names, IR, _ir["outs"])
        _expect_launches(names, want_names, failures)
        assert blocks == sum(sum(k.startswith(("k_ir<", "k_ir_b16")) for k in v) for v in want_names.values()), blocks
    if setting in ("VSO_IR_B16=0", "VSO_IR_WAVE=1"):
        here, here_launches = _ir_sessions(ort, "f32" if setting == "VSO_IR_B16=0" else "bf16")[:2]
        if setting == "VSO_IR_B16=0" and launches != here_launches:
            failures.append(f"launched {launches}, this process's f32 session {here_launches}")
        for o, g in got.items():
            if not np.array_equal(g, here[o], equal_nan=True):
                failures.append(f"{o}: differs from this process's {'f32' if setting == 'VSO_IR_B16=0' else 'bf16'} "
                                f"session, max {float(np.abs(g - here[o]).max()):.3e}")
    if setting == "VSO_IR_WAVE=1":
        moved = [cs.name for cs in IR if _wave(cs) != cs.kernels16]
        assert len(moved) >= 20 and "IR_64_96" in moved and "IR_96_96_res" not in moved, moved
    if setting == "VSO_IR_KS1=1":
        assert KS1_KEEPS <= {cs.name for cs in IR_FUSED16}
    assert not failures, "\n".join(failures)


# ---- the norm families: 16-bit sessions and the planner's knobs -------------------
NORM_FAMILIES = ("inorm", "ibn", "ibn9", "ibn16")  # (ibn9: the attribute-form Slice's opset; ibn16: see op_cases)
NORM = [cs for fam in NORM_FAMILIES for cs in OC.groups()[fam]]
_norm = {}


def _norm_models():
    """{family: (model, feeds, {case: its graph outputs})} and the f64 oracle's outputs of all of them."""
    if "models" not in _norm:
        _norm["models"] = {fam: OC.build(OC.groups()[fam]) for fam in NORM_FAMILIES}
        _norm["outs"] = {k: v for m in _norm["models"].values() for k, v in m[2].items()}
        _norm["want"] = {k: v for data, feeds, _ in _norm["models"].values() for k, v in R.run(R.load(data), feeds).items()}
    return _norm["models"]


def _norm_sessions(ort, prec):
    """(outputs, launches in order, whether a second run was bitwise the same) of the families' sessions in
    this process, once per precision."""
    if prec not in _norm:
        got, launches, same = {}, [], True
        t0 = time.perf_counter()
        for fam, (data, feeds, _) in _norm_models().items():
            with ort.InferenceSession(data, precision=prec) as s:
                out = s.run(feeds)
                again = s.run(feeds)
                same = same and all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)
                got.update(out)
                launches += s.launches()
        print(f"norm families, {prec} sessions: {time.perf_counter() - t0:.2f} s, {len(launches)} launches")
        _norm[prec] = (got, launches, same)
    return _norm[prec]


def _split_launches(launches, expect):
    """{case: its launches} by the number each case expects ({case: tuple}), in case order."""
    assert len(launches) == sum(len(v) for v in expect.values()), (len(launches), launches)
    names, k = {}, 0
    for cs in NORM:
        names[cs.name] = launches[k:k + len(expect[cs.name])]
        k += len(expect[cs.name])
    return names


def _check_launches(names, expect, failures):
    for cs in NORM:
        if not all(k in n for k, n in zip(expect[cs.name], names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {expect[cs.name]}")


def _check_exact(got, failures):
    for cs in NORM:
        if cs.exact and not all(np.array_equal(got[o], _norm["want"][o]) for o in _norm["outs"][cs.name]):
            failures.append(f"{cs.name}: not equal to the oracle")


def _inner(cs):
    return int(np.prod(cs.inputs[0][1][2:]))


def _no_plane(cs):
    """`kernels` under VSO_NORM_PLANE=0: the pair for every plane launch, one piece included."""
    out = []
    for k in cs.kernels:
        out += [OC.STATS, OC.APPLY] if k.startswith("k_norm_plane<") else [k]
    return tuple(out)


def _no_thin(cs):
    """`kernels` under VSO_THIN=0: nothing is deferred — the norm's own launches by plane size — and a head
    of up to 4 outputs runs on k_conv_pw (up to 192 channels on these few workgroups) or k_conv_small."""
    out, ks = [], list(cs.kernels)
    deferred = cs.name in OC.IBN and OC.IBN[cs.name]["defer"]
    for j, k in enumerate(ks):
        if deferred and k == OC.STATS:
            out += list(OC.norm_launches(_inner(cs)))
        elif deferred and k == OC.APPLY and ks[j - 1] == OC.STATS:
            continue  # (flush_norm's, of the head no precision defers to: part of the pair above or not launched)
        elif k.startswith("k_conv_thin<"):
            c_in = [nd[1][0][1].shape[1] for nd in cs.chain if nd[0] == "Conv"][0]
            out.append(OC.pw_name(1) if c_in <= 192 else OC.small(True, 16, True))
        else:
            out.append(k)
    return tuple(out)


NORM_KNOBS = {"VSO_NORM_PLANE=0": _no_plane, "VSO_THIN=0": _no_thin}


@pytest.mark.parametrize("setting", sorted(NORM_KNOBS))
def test_norm_family_knob(ort, setting):
    """The inorm and ibn families' f32 sessions in a child process under one A/B knob (read once per
    process; one child at a time, none after an abnormal end): every case at the bar (the `half` cases
    exactly B[c]) on the launches the setting implies.  VSO_NORM_PLANE=0: every plane case on
    k_norm_stats + k_norm_apply, down to planes of one element in one piece.  VSO_THIN=0: every
    deferred case launches its apply step and the head runs on another conv kernel.  A case the knob does
    not move is bitwise this process's."""
    _norm_models()
    expect = {cs.name: NORM_KNOBS[setting](cs) for cs in NORM}
    moved = [cs for cs in NORM if expect[cs.name] != cs.kernels]
    knob, value = setting.split("=")
    t0 = time.perf_counter()
    outs, info = C.run_child(setting, {knob: value}, ";".join(f"op_{fam}:f32" for fam in NORM_FAMILIES))
    print(f"norm families, {setting} f32 child: {time.perf_counter() - t0:.2f} s")
    got = {o: outs[f"op_{cs.family}/f32/{o}"] for cs in NORM for o in _norm["outs"][cs.name]}
    launches = [n for fam in NORM_FAMILIES for n in info[f"op_{fam}/f32"]["launches"]]
    assert all(info[f"op_{fam}/f32"]["rerun_equal"] for fam in NORM_FAMILIES)
    names = _split_launches(launches, expect)
    failures = _beyond_bar(got, _norm["want"], setting, names, NORM, _norm["outs"])
    _check_launches(names, expect, failures)
    _check_exact(got, failures)
    here = _norm_sessions(ort, "f32")[0]
    for cs in NORM:
        if cs not in moved and not all(np.array_equal(got[o], here[o]) for o in _norm["outs"][cs.name]):
            failures.append(f"{cs.name}: differs from the default session's output")
    if knob == "VSO_NORM_PLANE":
        assert len(moved) >= 60 and {_inner(cs) for cs in moved} >= {1, 2, 3, 4, 5, 4096, 4097, 36864}
        assert not any("k_norm_plane" in n for n in launches)
    else:
        assert {cs.name for cs in moved} >= {k for k, v in OC.IBN.items() if v["defer"]} and len(moved) >= 9
        assert not any("k_conv_thin" in n for n in launches)
    assert not failures, "\n".join(failures)


def _norm_tiled(cs):
    """Whether a 16-bit session runs the case's pattern conv on k_conv_tile (onnx_ref.tiled_conv: the oracle
    rounds its operands); the 1x1 heads and the inorm family never are."""
    convs = ([(cs.inputs[1][1], cs.attrs)] if cs.op == "Conv" else []) + \
        [(nd[1][0][1], nd[2]) for nd in cs.chain if nd[0] == "Conv"]
    assert not any(R.tiled_conv(w, at_) for w, at_ in convs[1:]), cs.name
    return bool(convs) and R.tiled_conv(*convs[0])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_norm_families_16bit(ort, prec):
    """bf16 / f16 sessions of the inorm and ibn families.  A case whose conv the oracle does not round
    (onnx_ref.tiled_conv) launches the f32 session's kernels, its output bitwise the f32 session's.  The
    dense 3x3 patterns run on k_conv_tile, the other launches as in f32; their BatchNorm is folded into
    the weights before these are rounded, which the oracle (it rounds the weights first) matches only on
    the ibn16 cases' constants (the fold factor a power of two: tests/test_op_matrix_oracle.py) — those
    are held to the matrix's bar against R.run(conv_operands=prec), the ibn family's 3x3 cases to their
    launches and a bitwise second run."""
    models = _norm_models()
    if ("want", prec) not in _norm:
        data, feeds, _ = models["ibn16"]
        _norm["want", prec] = R.run(R.load(data), feeds, conv_operands=prec)
    f32_out, f32_launches, _ = _norm_sessions(ort, "f32")
    got, launches, same = _norm_sessions(ort, prec)
    assert same, "the second run differs from the first"
    tiled = [cs for cs in NORM if _norm_tiled(cs)]
    assert len(tiled) >= 9 and all(cs in tiled for cs in OC.groups()["ibn16"])
    expect = {cs.name: (("k_conv_tile<",) + cs.kernels[1:]) if cs in tiled else cs.kernels for cs in NORM}
    names = _split_launches(launches, expect)
    f32_names = _split_launches(f32_launches, {cs.name: cs.kernels for cs in NORM})
    b16 = OC.groups()["ibn16"]
    failures = _beyond_bar(got, _norm["want", prec], prec, names, b16, _norm["outs"])
    _check_launches(names, expect, failures)
    for cs in NORM:
        if cs in tiled:
            continue
        if names[cs.name] != f32_names[cs.name]:
            failures.append(f"{cs.name}: launched {names[cs.name]}, in f32 {f32_names[cs.name]}")
        if not all(np.array_equal(got[o], f32_out[o], equal_nan=True) for o in _norm["outs"][cs.name]):
            failures.append(f"{cs.name}: differs from the f32 session's output")
    assert not failures, "\n".join(failures)
