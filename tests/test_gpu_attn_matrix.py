"""The GPU ONNX sessions (include/vso.h) on the transformer-block operators:
the case table of tests/op_cases_attn.py — LayerNormalization and its
decomposed form, Gelu / Erf and the erf form of GELU, a Linear layer's bias,
the attention pattern — against the float64 reference tests/onnx_ref_attn.py
(itself held to PyTorch's float64 by tests/test_attn_ref.py).  One f32 session
per family, one graph output per case output.

Bar: the operator matrix's, |gpu - ref| <= TOL * max(1, |ref|) with the
project's TOL = 1e-4.  Every case's launches are asserted by name and order:
one k_layer_norm per norm in either form, no launch for an absorbed Gelu or
bias Add, k_attn and nothing else for the five (or six) nodes of an attention,
and today's launches for every near miss.  A second run is bitwise the first.
k_layer_norm, k_unary, k_gemm and k_attn compute on f32 operands in every
session, and so do the 1x1 convolutions of the gelu family: the bf16 and f16
sessions of a family launch the same kernels and are bitwise the f32
session's.  The attention family runs again under VSO_ATTN=0, a child process
(tests/attn_matrix_child.py): the unfused launches, the same bar.  The refused
cases fail at creation, on the host, with a message naming the operator.
"""
import re

import numpy as np
import pytest

import attn_matrix_child as CH
import onnx_ref as R
import onnx_ref_attn as RA
import op_cases as OC
import op_cases_attn as AC

pytestmark = pytest.mark.gpu

TOL = 1e-4
FAMILIES = sorted(AC.groups())
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
        data, feeds, outs = OC.build(AC.groups()[fam])
        _models[fam] = (data, feeds, outs, RA.run(R.load(data), feeds))
    return _models[fam]


def _split(cases, launches):
    """{case: its launches} of a family's launch list, by each case's number of kernels."""
    assert len(launches) == sum(len(cs.kernels) for cs in cases), launches
    names, k = {}, 0
    for cs in cases:
        names[cs.name] = launches[k:k + len(cs.kernels)]
        k += len(cs.kernels)
    return names


def _session(ort, fam, prec):
    """(outputs, {case: its launches}, whether a second run was bitwise the first, attn_nodes()) of a family's session."""
    data, feeds, _, _ = _model(fam)
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        launches = s.launches()
        fused = s.attn_nodes()
    return got, _split(AC.groups()[fam], launches), all(np.array_equal(got[o], again[o], equal_nan=True) for o in got), fused


def _f32_session(ort, fam):
    if fam not in _f32:
        _f32[fam] = _session(ort, fam, "f32")
    return _f32[fam]


def _check(cases, outs, want, got, names, key=lambda o: o):
    """The failures of `cases` (launch names, shapes, the bar) and the worst err / bar per kernel form."""
    failures, worst = [], {}
    for cs in cases:
        if not all(k in n for k, n in zip(cs.kernels, names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {cs.kernels}")
        ratio = 0.0
        for o in outs[cs.name]:
            g, w = got[key(o)], want[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, reference {w.shape}")
                continue
            err = np.abs(g.astype(np.float64) - w)
            bar = TOL * np.maximum(1.0, np.abs(w))
            ratio = max(ratio, float((err / bar).max()))
            print(f"{o}: max abs err {float(err.max()):.3e}, err / bar {ratio:.4f}")
            if not (err <= bar).all():
                failures.append(f"{o}: {int((~(err <= bar)).sum())} elements beyond {TOL:g} * max(1, |want|), "
                                f"worst {float(err.max()):.3e}")
        form = " + ".join(re.search(r"k_\w+(<[^>]*>)?", n).group(0) for n in names[cs.name]) or "(no launch)"
        worst[form] = max(worst.get(form, 0.0), ratio)
    return failures, worst


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_reference(ort, family):
    _, _, outs, want = _model(family)
    got, names, same, fused = _f32_session(ort, family)
    assert same, "the second run differs from the first"
    cases = AC.groups()[family]
    failures, worst = _check(cases, outs, want, got, names)
    for form, ratio in sorted(worst.items()):
        print(f"{family} worst err / bar, {form}: {ratio:.4f}")
    assert not failures, "\n".join(failures)
    assert fused == sum(cs.kernels[0].startswith("k_attn") for cs in cases if cs.kernels)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_16bit_is_f32(ort, family, prec):
    f32_out, f32_names, _, _ = _f32_session(ort, family)
    got, names, same, _ = _session(ort, family, prec)
    assert same, "the second run differs from the first"
    failures = []
    for cs in AC.groups()[family]:
        if names[cs.name] != f32_names[cs.name]:
            failures.append(f"{cs.name}: launched {names[cs.name]}, in f32 {f32_names[cs.name]}")
    for o, g in got.items():
        if not np.array_equal(g, f32_out[o], equal_nan=True):
            failures.append(f"{o}: differs from the f32 session's output, max {float(np.abs(g - f32_out[o]).max()):.3e}")
    assert not failures, "\n".join(failures)


def test_attention_unfused_knob(ort):
    """The attention family's f32 session in a child process under VSO_ATTN=0 (read once per process): every
    case on today's launches — the K Transpose, MatMul, the scale and bias it has, Softmax, MatMul — at the same
    bar; within it, not bitwise the fused outputs (another order of the same sums)."""
    fam = AC.A
    cases = AC.groups()[fam]
    _, _, outs, want = _model(fam)
    got, info = CH.run_child("VSO_ATTN=0", {"VSO_ATTN": "0"}, f"at_{fam}:f32")
    inf = info[f"at_{fam}/f32"]
    assert inf["rerun_equal"]
    launches = inf["launches"]
    assert not any("k_attn" in n for n in launches), launches
    unfused, k = [], 0
    for cs in cases:  # a case's nodes, one launch each (a constant K: its Transpose is folded)
        n = len(cs.kernels) if not cs.kernels[0].startswith("k_attn") else 1 + len(cs.chain)
        unfused.append(launches[k:k + n])
        k += n
    assert k == len(launches), launches
    failures = []
    for cs, ls in zip(cases, unfused):
        if sum("k_softmax(" in n for n in ls) != 1 or sum("k_gemm" in n for n in ls) != 2:
            failures.append(f"{cs.name}: launched {ls}")
        for o in outs[cs.name]:
            g, w = got[f"at_{fam}/f32/{o}"], want[o]
            err = np.abs(g.astype(np.float64) - w)
            if not (err <= TOL * np.maximum(1.0, np.abs(w))).all():
                failures.append(f"{o}: beyond the bar, worst {float(err.max()):.3e}")
    assert not failures, "\n".join(failures)


def test_forms_are_reached():
    """The table names every instance of k_attn and every form of k_layer_norm."""
    forms = {k for cs in AC.VALUE_CASES for k in cs.kernels}
    assert {AC.ATTN % u for u in (1, 2, 4, 8)} <= forms and {AC.LN4, AC.LN16, AC.LN0} <= forms
    assert len(AC.FUSED_ATTN) >= 12 and len(AC.LNORM_CASES) >= 20


@pytest.mark.parametrize("name", [k.name for k in AC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = AC.BY_NAME[name]
    data, _, _ = OC.build([cs])
    with pytest.raises(ort.VsoError, match=cs.op):
        ort.InferenceSession(data, precision="f32").close()
