"""The GPU ONNX sessions (include/vso.h) on dynamically quantised graphs: the
case table of tests/op_cases_dynq.py — DynamicQuantizeLinear, ConvInteger and
MatMulInteger (k_iconv_tile on the int8 MFMA, k_iconv_direct), the Cast of
their int32 output, and the chain Cast -> Mul -> [Add] -> [Relu | Clip] fused
into the integer launch's float epilogue — against tests/onnx_ref_dynq.py
(itself held by tests/test_dynq_ref.py).  One session per family, one graph
output per case output.

"exact" outputs equal the reference's, every element: all of
DynamicQuantizeLinear (float32 arithmetic, stated step by step by the
reference), every integer result, every dyadic chain.  A general chain's float
output lies within 4 * 2^-24 * (|acc| s + |bias|) of the float64 value (one
rounding each for the conversion, s, the product, the sum).  Every case's
launches are asserted by name and order, dynq_nodes() is the table's count, a
second run is bitwise the first.  These nodes compute on integers: the bf16
session is bitwise the f32 one.  The families run again under VSO_DYNQ=0, a
child process, in both precisions: the unfused launch list, no fused launch,
and every output bitwise the fused session's.
"""
import numpy as np
import pytest

import onnx_ref as R
import onnx_ref_dynq as RD
import op_cases_dynq as DC
import dynq_matrix_child as CH

pytestmark = pytest.mark.gpu

FAMILIES = sorted(DC.groups())
_models, _sessions = {}, {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _model(fam):
    """(model bytes, feeds, {case: Built}, every value of the reference) of a family, once."""
    if fam not in _models:
        data, feeds, built = DC.build(DC.groups()[fam])
        _models[fam] = (data, feeds, built, RD.run_all(R.load(data), feeds))
    return _models[fam]


def _session(ort, fam, prec):
    if (fam, prec) not in _sessions:
        data, feeds, _, _ = _model(fam)
        with ort.InferenceSession(data, precision=prec) as s:
            got = s.run(feeds)
            again = s.run(feeds)
            launches = s.launches()
            fused = s.dynq_nodes()
        same = all(np.array_equal(got[o], again[o], equal_nan=True) for o in got)
        _sessions[(fam, prec)] = (got, launches, same, fused)
    return _sessions[(fam, prec)]


def _split(cases, built, launches, key):
    """{case: its launches} of a family's launch list, by each case's number of kernels."""
    want = {cs.name: getattr(built[cs.name], key) for cs in cases}
    assert len(launches) == sum(len(v) for v in want.values()), launches
    names, k = {}, 0
    for cs in cases:
        names[cs.name] = launches[k:k + len(want[cs.name])]
        k += len(want[cs.name])
    return names, want


def value_failures(o, rule, g, env):
    """What is wrong with graph output `o`: equality, or the general chain's bound."""
    w = env[o]
    if g.shape != w.shape:
        return [f"{o}: shape {g.shape}, reference {w.shape}"]
    if g.dtype != w.dtype:
        return [f"{o}: dtype {g.dtype}, reference {w.dtype}"]
    if isinstance(rule, str):
        bad = np.argwhere(g != w)
        print(f"{o}: {len(bad)} of {w.size} elements differ")
        return [f"{o}: {len(bad)} of {w.size} differ from the reference, first at {tuple(bad[0])}: "
                f"{g[tuple(bad[0])]!r} for {w[tuple(bad[0])]!r}"] if len(bad) else []
    v, bound = DC.general_bound(rule, env)
    err = np.abs(g.astype(np.float64) - v)
    print(f"{o}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}, max abs err {float(err.max()):.3e}")
    return [] if (err <= bound).all() else [f"{o}: {int((err > bound).sum())} elements beyond the bound, worst {float(err.max()):.3e}"]


def test_lane_map(ort):
    """First: k_iconv_tile's operand and result lane maps.  A 1x1 convolution over 64 channels by the asymmetric
    integer matrix W[m][c] = (3 m + 5 c) mod 11 - 5, the input 255 in channel (p + 7 n) mod 64 of pixel p and 0
    elsewhere (x_scale 1, zero point 0): the output at (m, p) is 255 W[m][that channel], so a wrong row, column
    or k of any lane shows as a wrong integer."""
    cs = DC.BY_NAME[DC.LANE_MAP]
    data, feeds, built = DC.build([cs])
    env = RD.run_all(R.load(data), feeds)
    with ort.InferenceSession(data, precision="f32") as s:
        got = s.run(feeds)
        launches = s.launches()
    bt = built[cs.name]
    assert len(launches) == len(bt.kernels) and all(k in n for k, n in zip(bt.kernels, launches)), launches
    (o,) = bt.outs
    w = env[o]
    wm = DC._lane_w().reshape(40, 64).astype(np.float32)
    p = np.arange(12 * 13)
    for n in range(2):  # the reference itself names the matrix element
        assert np.array_equal(w[n].reshape(40, -1), 255.0 * wm[:, (p + 7 * n) % 64])
    bad = np.argwhere(got[o] != w)
    assert not len(bad), f"{len(bad)} of {w.size} differ, first (n, m, y, x) = {tuple(bad[0])}: " \
                         f"{got[o][tuple(bad[0])]} for {w[tuple(bad[0])]}"


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_reference(ort, family):
    _, _, built, env = _model(family)
    got, launches, same, fused = _session(ort, family, "f32")
    assert same, "the second run differs from the first"
    cases = DC.groups()[family]
    names, want = _split(cases, built, launches, "kernels")
    failures = []
    for cs in cases:
        if not all(k in n for k, n in zip(want[cs.name], names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {want[cs.name]}")
        for o, rule in built[cs.name].outs.items():
            failures += value_failures(o, rule, got[o], env)
    assert not failures, "\n".join(failures)
    assert fused == sum(built[cs.name].fused for cs in cases)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_bf16_is_f32(ort, family):
    f32_out, f32_launches, _, f32_fused = _session(ort, family, "f32")
    got, launches, same, fused = _session(ort, family, "bf16")
    assert same, "the second run differs from the first"
    assert launches == f32_launches and fused == f32_fused
    bad = [o for o, g in got.items() if not np.array_equal(g, f32_out[o], equal_nan=True)]
    assert not bad, f"differ from the f32 session's: {bad}"


@pytest.mark.parametrize("family", FAMILIES)
def test_unfused_knob(ort, family):
    """The family's f32 and bf16 sessions in a child process under VSO_DYNQ=0 (read once per process): the unfused
    launch list, vso_dynq_count 0, and every output bitwise the fused session's (so held to the reference alike)."""
    cases = DC.groups()[family]
    _, _, built, _ = _model(family)
    fused_out = _session(ort, family, "f32")[0]
    got, info = CH.run_child("VSO_DYNQ=0", {"VSO_DYNQ": "0"}, f"d_{family}:f32,bf16")
    failures = []
    for prec in ("f32", "bf16"):
        inf = info[f"d_{family}/{prec}"]
        assert inf["rerun_equal"] and inf["dynq_nodes"] == 0
        names, want = _split(cases, built, inf["launches"], "unfused")
        for cs in cases:
            if not all(k in n for k, n in zip(want[cs.name], names[cs.name])):
                failures.append(f"{prec} {cs.name}: launched {names[cs.name]}, expected {want[cs.name]}")
            for o in built[cs.name].outs:
                g = got[f"d_{family}/{prec}/{o}"]
                if g.dtype != fused_out[o].dtype or not np.array_equal(g, fused_out[o], equal_nan=True):
                    failures.append(f"{prec} {cs.name}: {o} is not bitwise the fused session's "
                                    f"({int((g != fused_out[o]).sum())} of {g.size} differ)")
    assert not failures, "\n".join(failures)


def test_forms_are_reached():
    """The table names each of the five kernels, the fused epilogue on both integer kernels and in both weightings."""
    built = {}
    for fam, cases in DC.groups().items():
        built.update(DC.build(cases)[2])
    forms = {k for bt in built.values() for k in bt.kernels}
    assert set(DC.FORMS) <= forms, sorted(set(DC.FORMS) - forms)
    for form in (DC.TILE, DC.DIRECT):
        for dyadic in (True, False):
            assert any(bt.fused and form in bt.kernels and all(isinstance(r, str) for r in bt.outs.values()) == dyadic
                       for bt in built.values()), (form, dyadic)


def test_dynq_count_symbol(pkg):
    assert hasattr(pkg.lib(), "vso_dynq_count")


@pytest.mark.parametrize("name", [k.name for k in DC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = DC.BY_NAME[name]
    data, _, _ = DC.build([cs])
    with pytest.raises(ort.VsoError, match=cs.op) as e:
        ort.InferenceSession(data, precision="f32").close()
    assert e.value.code == ort.VSO_E_UNSUPPORTED, str(e.value)
