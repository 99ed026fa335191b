"""The GPU ONNX sessions (include/vso.h) on ConvTranspose, HardSigmoid,
HardSwish and ReduceMean: the case table of tests/op_cases_deconv.py against
the float64 reference tests/onnx_ref_ext.py (itself held to PyTorch's float64
by tests/test_deconv_ref.py).  One f32 session per family, one graph output
per case.

Bar: the operator matrix's, |gpu - ref| <= TOL * max(1, |ref|) with the
project's TOL = 1e-4 (the kernels' own f32 rounding measured at most 0.013 of
it on these cases: the bar tests the indexing, not f32).  A second run is
bitwise the first.  Every case launches the form it names — k_deconv_tile<1>,
<2> (both x phases per workgroup: the three cases of 1024 workgroups or more),
k_deconv_direct, or for stride 1 the kernel of the Conv it is rewritten to —
and the fused activations add no launch.  ConvTranspose and the 1x1 / Gemm
producers of the activation cases compute on f32 operands in every session:
the bf16 and f16 sessions of a family launch the same kernels and are bitwise
the f32 session's.  The tile family runs again under each setting of the
planning knobs VSO_DECONV_TILE and VSO_DECONV_PAIR, a child process each
(tests/deconv_matrix_child.py).  The refused cases fail at creation, on the
host, with a message naming the operator.  Worst err / bar per kernel form and the
value-only breaks of vso_deconv.hip these tests catch: profiles/NOTES.md,
"ConvTranspose".
"""
import re

import numpy as np
import pytest

import deconv_matrix_child as CH
import onnx_ref as R
import onnx_ref_ext as X
import op_cases as OC
import op_cases_deconv as DC

pytestmark = pytest.mark.gpu

TOL = 1e-4
FAMILIES = sorted(DC.groups())
_models, _f32 = {}, {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _model(fam):
    """(model, feeds, {case: its graph outputs}, the reference's outputs) of a family, once."""
    if fam not in _models:
        data, feeds, outs = OC.build(DC.groups()[fam])
        _models[fam] = (data, feeds, outs, X.run(R.load(data), feeds))
    return _models[fam]


def _session(ort, fam, prec):
    """(outputs, {case: its launches}, whether a second run was bitwise the first) of a family's session."""
    data, feeds, _, _ = _model(fam)
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        launches = s.launches()
    cases = DC.groups()[fam]
    assert len(launches) == sum(len(cs.kernels) for cs in cases), launches
    names, k = {}, 0
    for cs in cases:
        names[cs.name] = launches[k:k + len(cs.kernels)]
        k += len(cs.kernels)
    return got, names, all(np.array_equal(got[o], again[o], equal_nan=True) for o in got)


def _f32_session(ort, fam):
    if fam not in _f32:
        _f32[fam] = _session(ort, fam, "f32")
    return _f32[fam]


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_reference(ort, family):
    _, _, outs, want = _model(family)
    got, names, same = _f32_session(ort, family)
    assert same, "the second run differs from the first"
    failures, worst = [], {}
    for cs in DC.groups()[family]:
        if not all(k in n for k, n in zip(cs.kernels, names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {cs.kernels}")
        ratio = 0.0
        for o in outs[cs.name]:
            g, w = got[o], want[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, reference {w.shape}")
                continue
            err = np.abs(g.astype(np.float64) - w)
            bar = TOL * np.maximum(1.0, np.abs(w))
            ratio = max(ratio, float((err / bar).max()))
            print(f"{o}: max abs err {float(err.max()):.3e}, err / bar {ratio:.4f}")
            if cs.exact:
                if not np.array_equal(g, w):
                    failures.append(f"{o}: not equal, max abs err {float(err.max()):.3e}")
            elif not (err <= bar).all():
                failures.append(f"{o}: {int((~(err <= bar)).sum())} elements beyond {TOL:g} * max(1, |want|), "
                                f"worst {float(err.max()):.3e}")
        form = " + ".join(re.search(r"k_\w+(<[^>]*>)?", n).group(0) for n in names[cs.name]) or "(no launch)"
        worst[form] = max(worst.get(form, 0.0), ratio)
    for form, ratio in sorted(worst.items()):
        print(f"{family} worst err / bar, {form}: {ratio:.4f}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_16bit_is_f32(ort, family, prec):
    f32_out, f32_names, _ = _f32_session(ort, family)
    got, names, same = _session(ort, family, prec)
    assert same, "the second run differs from the first"
    failures = []
    for cs in DC.groups()[family]:
        if names[cs.name] != f32_names[cs.name]:
            failures.append(f"{cs.name}: launched {names[cs.name]}, in f32 {f32_names[cs.name]}")
    for o, g in got.items():
        if not np.array_equal(g, f32_out[o], equal_nan=True):
            failures.append(f"{o}: differs from the f32 session's output, max {float(np.abs(g - f32_out[o]).max()):.3e}")
    assert not failures, "\n".join(failures)


def _paired(cs):
    """The case's ConvTranspose has stride 2 in x: the layers VSO_DECONV_PAIR moves between k_deconv_tile<1> and <2>."""
    return cs.attrs.get("strides", [1, 1])[1] == 2


KNOBS = {
    # setting: the first launch of a case of the tile family under it
    "VSO_DECONV_TILE=0": lambda cs: DC.DIRECT,
    "VSO_DECONV_PAIR=0": lambda cs: DC.TILE,
    "VSO_DECONV_PAIR=1": lambda cs: DC.TILE2 if _paired(cs) else DC.TILE,
}


@pytest.mark.parametrize("setting", sorted(KNOBS))
def test_tile_family_knob(ort, setting):
    """The tile family's f32 session in a child process under one planning knob (read once per process; one
    child at a time, none after an abnormal end): every case at the bar on the form the setting implies.
    VSO_DECONV_TILE=0: all of them on k_deconv_direct.  VSO_DECONV_PAIR=1: every stride-2 case on
    k_deconv_tile<2>, down to the ragged 5x7 planes; =0: the three large ones on <1> — and both bitwise
    this process's session (a workgroup of either form adds a phase's taps and chunks in the same order)."""
    fam = "deconv_tile"
    cases = DC.groups()[fam]
    _, _, outs, want = _model(fam)
    here, _, _ = _f32_session(ort, fam)
    knob, value = setting.split("=")
    got, info = CH.run_child(setting, {knob: value}, f"dc_{fam}:f32")
    inf = info[f"dc_{fam}/f32"]
    assert inf["rerun_equal"]
    launches = inf["launches"]
    assert len(launches) == sum(len(cs.kernels) for cs in cases), launches
    failures, k, moved = [], 0, 0
    for cs in cases:
        first = launches[k]
        k += len(cs.kernels)
        expect = KNOBS[setting](cs)
        moved += expect != cs.kernels[0]
        if expect not in first:
            failures.append(f"{cs.name}: launched {first}, expected {expect}")
        for o in outs[cs.name]:
            g, w = got[f"dc_{fam}/f32/{o}"], want[o]
            err = np.abs(g.astype(np.float64) - w)
            if not (err <= TOL * np.maximum(1.0, np.abs(w))).all():
                failures.append(f"{o}: beyond the bar, worst {float(err.max()):.3e}")
            if knob == "VSO_DECONV_PAIR" and not np.array_equal(g, here[o]):
                failures.append(f"{o}: differs from the default session's output, max {float(np.abs(g - here[o]).max()):.3e}")
    assert moved >= 3, moved
    assert not failures, "\n".join(failures)


def test_forms_are_reached(ort):
    """The table names both kernels of vso_deconv.hip and, at stride 1, the existing convolution kernels."""
    forms = {k for cs in DC.VALUE_CASES if cs.op == "ConvTranspose" for k in cs.kernels}
    assert {DC.TILE, DC.TILE2, DC.DIRECT} <= forms and any(k.startswith("k_conv_small<") for k in forms)
    assert sum(cs.kernels[:1] == (DC.TILE,) for cs in DC.VALUE_CASES) >= 15
    assert sum(cs.kernels[:1] == (DC.DIRECT,) for cs in DC.VALUE_CASES) >= 10


@pytest.mark.parametrize("name", [k.name for k in DC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = DC.BY_NAME[name]
    data, _, _ = OC.build([cs])
    with pytest.raises(ort.VsoError, match=cs.op):
        ort.InferenceSession(data, precision="f32").close()
