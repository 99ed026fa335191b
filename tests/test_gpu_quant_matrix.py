"""The GPU ONNX sessions (include/vso.h) on statically quantised (QDQ) graphs:
the case table of tests/op_cases_quant.py — QuantizeLinear / DequantizeLinear
of runtime tensors, and DequantizeLinear -> Conv | Add [-> Relu | Clip] ->
QuantizeLinear on the integers (k_qconv_tile on the int8 MFMA, k_qconv_dw,
k_qadd) — against the float64 reference tests/onnx_ref_quant.py (itself held
by tests/test_quant_ref.py).  One f32 session per family, one graph output per
case output.

Quantised outputs.  Dyadic cases (power-of-two scales, accumulators below
2^24: every intermediate exact in float32 and float64): equal to the
reference, every element.  General cases: with v the reference's unrounded
value, an element farther than TAU max(1, |v|) from a half-integer must be
equal, one nearer may differ by one step (both sides are a handful of float32
roundings, 6e-8 relative each, from the same rational number; TAU = 1e-5).
Float outputs: bitwise in the dyadic cases, the project's 1e-4 max(1, |ref|)
otherwise.  Every case's launches are asserted by name and order,
qconv_nodes() is the table's count, run() returns uint8 / int8, and a second
run is bitwise the first.  The fused forms compute in integers in every
session precision: the bf16 and f16 sessions are bitwise the f32 one (the near
misses are left out there: their float Conv rounds its 9-bit operands).  The
families run again under VSO_QDQ=0, a child process: k_dequantize, the float
kernel, k_quantize, and the dyadic cases still equal the reference.
"""
import numpy as np
import pytest

import onnx_ref as R
import onnx_ref_quant as RQ
import op_cases_quant as QC
import quant_matrix_child as CH

pytestmark = pytest.mark.gpu

TOL = 1e-4
FAMILIES = sorted(QC.groups())
_models, _f32 = {}, {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _model(fam):
    """(model bytes, feeds, {case: its graph outputs}, the parsed model, every value of the reference) of a family, once."""
    if fam not in _models:
        data, feeds, outs = QC.build(QC.groups()[fam])
        m = R.load(data)
        _models[fam] = (data, feeds, outs, m, RQ.run_all(m, feeds))
    return _models[fam]


def _split(cases, launches, key="kernels"):
    """{case: its launches} of a family's launch list, by each case's number of kernels."""
    want = {cs.name: (cs.kernels if key == "kernels" else QC.META[cs.name]["unfused"]) for cs in cases}
    assert len(launches) == sum(len(v) for v in want.values()), launches
    names, k = {}, 0
    for cs in cases:
        names[cs.name] = launches[k:k + len(want[cs.name])]
        k += len(want[cs.name])
    return names, want


def _session(ort, fam, prec):
    data, feeds, _, _, _ = _model(fam)
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        launches = s.launches()
        fused = s.qconv_nodes()
    same = all(np.array_equal(got[o], again[o], equal_nan=True) for o in got)
    return got, launches, same, fused


def _f32_session(ort, fam):
    if fam not in _f32:
        _f32[fam] = _session(ort, fam, "f32")
    return _f32[fam]


def value_failures(cs, o, g, model, env):
    """What is wrong with graph output `o` of case `cs`: the equality and near-tie rules above."""
    w = env[o]
    dyadic = QC.META[cs.name]["weighting"] == "dyadic"
    if g.shape != w.shape:
        return [f"{o}: shape {g.shape}, reference {w.shape}"]
    if w.dtype in (np.uint8, np.int8):
        if g.dtype != w.dtype:
            return [f"{o}: dtype {g.dtype}, reference {w.dtype}"]
        d = g.astype(np.int64) - w.astype(np.int64)
        print(f"{o}: {int((d != 0).sum())} of {d.size} quantised values differ, max |step| {int(np.abs(d).max())}")
        return QC.quantised_failures(o, g, w, RQ.unrounded(model, env, o), dyadic)
    if dyadic:
        return [] if np.array_equal(g, w) else [f"{o}: a float output of a dyadic case is not bitwise the reference's"]
    err = np.abs(g.astype(np.float64) - w.astype(np.float64))
    bar = TOL * np.maximum(1.0, np.abs(w.astype(np.float64)))
    print(f"{o}: max abs err {float(err.max()):.3e}, err / bar {float((err / bar).max()):.4f}")
    return [] if (err <= bar).all() else [f"{o}: {int((err > bar).sum())} elements beyond the bar, worst {float(err.max()):.3e}"]


def test_lane_map(ort):
    """First: k_qconv_tile's operand and result lane maps.  A 1x1 convolution over 64 channels by the asymmetric
    integer matrix W[m][c] = (3 m + 5 c) mod 11 - 5, the input one-hot per pixel in channel (p + 7 n) mod 64: the
    output at (m, p) is W[m][that channel], so a wrong row, column or k of any lane shows as a wrong integer."""
    cs = QC.BY_NAME[QC.LANE_MAP]
    data, feeds, outs = QC.build([cs])
    m = R.load(data)
    env = RQ.run_all(m, feeds)
    with ort.InferenceSession(data, precision="f32") as s:
        got = s.run(feeds)
        launches = s.launches()
        assert s.qconv_nodes() == 1
    assert len(launches) == 3 and all(k in n for k, n in zip(cs.kernels, launches)), launches
    o = outs[cs.name][0]
    w = env[o]
    wm = QC._lane_w().reshape(40, 64)
    p = np.arange(12 * 13)
    for n in range(2):  # the reference itself names the matrix element
        assert np.array_equal(w[n].reshape(40, -1), wm[:, (p + 7 * n) % 64])
    assert got[o].dtype == np.int8
    bad = np.argwhere(got[o] != w)
    assert not len(bad), f"{len(bad)} of {w.size} differ, first (n, m, y, x) = {tuple(bad[0])}: " \
                         f"{got[o][tuple(bad[0])]} for {w[tuple(bad[0])]}"


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_reference(ort, family):
    _, _, outs, model, env = _model(family)
    got, launches, same, fused = _f32_session(ort, family)
    assert same, "the second run differs from the first"
    cases = QC.groups()[family]
    names, want = _split(cases, launches)
    failures = []
    for cs in cases:
        if not all(k in n for k, n in zip(want[cs.name], names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {want[cs.name]}")
        for o in outs[cs.name]:
            failures += value_failures(cs, o, got[o], model, env)
    assert not failures, "\n".join(failures)
    assert fused == sum(QC.META[cs.name]["fused"] for cs in cases)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("family", [f for f in FAMILIES if f != QC.F_MISS])
def test_family_16bit_is_f32(ort, family, prec):
    f32_out, f32_launches, _, f32_fused = _f32_session(ort, family)
    got, launches, same, fused = _session(ort, family, prec)
    assert same, "the second run differs from the first"
    assert launches == f32_launches and fused == f32_fused
    bad = [o for o, g in got.items() if not np.array_equal(g, f32_out[o], equal_nan=True)]
    assert not bad, f"differ from the f32 session's: {bad}"


@pytest.mark.parametrize("family", FAMILIES)
def test_unfused_knob(ort, family):
    """The family's f32 session in a child process under VSO_QDQ=0 (read once per process): every pattern as
    k_dequantize / the float kernel / k_quantize, no fused launch, and the dyadic cases equal to the reference."""
    cases = QC.groups()[family]
    _, _, outs, model, env = _model(family)
    got, info = CH.run_child("VSO_QDQ=0", {"VSO_QDQ": "0"}, f"q_{family}:f32")
    inf = info[f"q_{family}/f32"]
    assert inf["rerun_equal"]
    assert not any(k in n for n in inf["launches"] for k in (QC.QCONV, QC.QDW, QC.QADD)), inf["launches"]
    names, want = _split(cases, inf["launches"], key="unfused")
    failures = []
    for cs in cases:
        if not all(k in n for k, n in zip(want[cs.name], names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {want[cs.name]}")
        if QC.META[cs.name]["weighting"] != "dyadic":
            continue
        for o in outs[cs.name]:
            g = got[f"q_{family}/f32/{o}"]
            failures += value_failures(cs, o, g, model, env)
    assert not failures, "\n".join(failures)


def test_forms_are_reached():
    """The table names each of the five kernels, in both weightings, and the chains."""
    forms = {k for cs in QC.VALUE_CASES for k in cs.kernels}
    assert set(QC.FORMS) <= forms, sorted(set(QC.FORMS) - forms)
    for form in (QC.QCONV, QC.QDW, QC.QADD):
        for cases in (QC.DYADIC, QC.GENERAL):
            assert any(form in cs.kernels for cs in cases), form
    assert any(cs.kernels.count(QC.QCONV) == 3 for cs in QC.DYADIC)


def test_qconv_count_symbol(pkg):
    assert hasattr(pkg.lib(), "vso_qconv_count")


@pytest.mark.parametrize("name", [k.name for k in QC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = QC.BY_NAME[name]
    data, _, _ = QC.build([cs])
    with pytest.raises(ort.VsoError, match=QC.NAMES[name]) as e:
        ort.InferenceSession(data, precision="f32").close()
    assert e.value.code == ort.VSO_E_UNSUPPORTED, str(e.value)


@pytest.mark.parametrize("name", sorted(QC.RAW_REFUSED))
def test_refused_zero_point_types(ort, name):
    """4-bit, 16-bit and float8 zero points of a runtime tensor: refused by the node's name, not by the reader."""
    data, op = QC.RAW_REFUSED[name]
    with pytest.raises(ort.VsoError, match=op) as e:
        ort.InferenceSession(data, precision="f32").close()
    assert e.value.code == ort.VSO_E_UNSUPPORTED, str(e.value)
