"""The GPU ONNX sessions (include/vso.h) on the class heads: the case table of
tests/op_cases_head.py — Softmax / LogSoftmax / ArgMax / ReduceMax over the
channel axis, the linear Resize fused in front, the channel selections and
ArgMax -> Equal -> Cast behind, Gather, the Cast of an index tensor — against
the float64 reference tests/onnx_ref_head.py (itself held to PyTorch's float64
by tests/test_head_ref.py).  One f32 session per family, one graph output per
case output.

Float outputs: the operator matrix's bar, |gpu - ref| <= TOL * max(1, |ref|)
with the project's TOL = 1e-4.  Labels: exactly the reference's in the tie
cases (integer logits, exact interpolation).  In every other case a pixel
whose label differs from the reference's passes only if the reference's logit
at the GPU's label is within the bar of the reference's maximum, and such
pixels number at most 1 % of the case (the cap tests/test_head_ref.py shows
the reference's own near ties to meet); the ArgMax == k masks follow the same
rule.  Every case's launches are asserted by name and order — k_class_head and
nothing else for a fused pattern — head_nodes() is the table's count, and a
second run is bitwise the first.  The head computes on f32 operands in every
session: the bf16 and f16 sessions launch the same kernels and are bitwise the
f32 session's.  The fused family runs again under VSO_HEAD=0, a child process
(tests/head_matrix_child.py): k_resize, the plain head, the selection's copy —
the same device functions in the same order, so the outputs are bitwise the
fused session's.  The refused cases fail at creation, on the host, with a
message naming the operator.
"""
import re

import numpy as np
import pytest

import head_matrix_child as CH
import onnx_ref as R
import onnx_ref_head as RH
import op_cases_head as HC

pytestmark = pytest.mark.gpu

TOL = 1e-4
NEAR_TIE_SHARE = 0.01
FAMILIES = sorted(HC.groups())
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
        data, feeds, outs = HC.build(HC.groups()[fam])
        m = R.load(data)
        _models[fam] = (data, feeds, outs, m, RH.run_all(m, feeds))
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
    """(outputs, {case: its launches}, whether a second run was bitwise the first, head_nodes()) of a family's session."""
    data, feeds, _, _, _ = _model(fam)
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        launches = s.launches()
        fused = s.head_nodes()
    return got, _split(HC.groups()[fam], launches), all(np.array_equal(got[o], again[o], equal_nan=True) for o in got), fused


def _f32_session(ort, fam):
    if fam not in _f32:
        _f32[fam] = _session(ort, fam, "f32")
    return _f32[fam]


def label_failures(o, g, model, env, exact):
    """What is wrong with the label plane or label == k mask `g` of graph output `o` (label_source: its ArgMax)."""
    logits_name, k, at = RH.label_source(model, o)
    w = env[o]
    g = np.asarray(g, np.float64).reshape(w.shape)
    bad = g != w.astype(np.float64)
    print(f"{o}: {int(bad.sum())} of {bad.size} labels differ from the reference's")
    if exact:
        return [f"{o}: {int(bad.sum())} labels differ in a tie case"] if bad.any() else []
    if not bad.any():
        return []
    logits = env[logits_name].astype(np.float64)  # [N, C, H, W]
    top = logits.max(axis=1)
    bar = TOL * np.maximum(1.0, np.abs(top))
    if k is None:
        lab = np.clip(g.reshape(top.shape), 0, logits.shape[1] - 1).astype(np.int64)
        at_gpu = np.take_along_axis(logits, lab[:, None], axis=1)[:, 0]
        ok = (g.reshape(top.shape) == lab) & (top - at_gpu <= bar)
    else:
        # a mask differs where one side says k and the other does not: class k must be within the bar of the
        # maximum there (either k is a near tie of the winner, or the winner a near tie of k)
        kk = int(k)
        ok = (top - logits[:, kk] <= bar) if 0 <= kk < logits.shape[1] else np.zeros(top.shape, bool)
    badp = bad.reshape(top.shape)
    out = []
    if (badp & ~ok).any():
        out.append(f"{o}: {int((badp & ~ok).sum())} labels differ where the reference's logits are no near tie")
    if badp.sum() > NEAR_TIE_SHARE * badp.size:
        out.append(f"{o}: {int(badp.sum())} labels differ, more than {NEAR_TIE_SHARE:.0%} of {badp.size}")
    return out


def _check(cases, outs, model, env, got, names, key=lambda o: o):
    """The failures of `cases` (launch names, shapes, the bar or the label rule) and the worst err / bar per kernel form."""
    failures, worst = [], {}
    for cs in cases:
        if not all(k in n for k, n in zip(cs.kernels, names[cs.name])):
            failures.append(f"{cs.name}: launched {names[cs.name]}, expected {cs.kernels}")
        ratio = 0.0
        for o in outs[cs.name]:
            g, w = got[key(o)], env[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, reference {w.shape}")
                continue
            if RH.label_source(model, o) is not None:
                failures += label_failures(o, g, model, env, cs.exact)
                continue
            if cs.exact:
                if not np.array_equal(g, w.astype(g.dtype)):
                    failures.append(f"{o}: not bitwise the reference's")
                continue
            w = w.astype(np.float64)
            same = (g == w)  # (-inf where the reference has -inf: LogSoftmax of a class at -inf)
            with np.errstate(invalid="ignore"):
                err = np.where(same, 0.0, np.abs(g.astype(np.float64) - w))
            bar = TOL * np.maximum(1.0, np.abs(np.where(np.isfinite(w), w, 0.0)))
            ratio = max(ratio, float((err / bar).max()))
            print(f"{o}: max abs err {float(err.max()):.3e}, err / bar {float((err / bar).max()):.4f}")
            if not (err <= bar).all():
                failures.append(f"{o}: {int((~(err <= bar)).sum())} elements beyond {TOL:g} * max(1, |want|), "
                                f"worst {float(err.max()):.3e}")
        form = " + ".join(re.search(r"k_\w+(<[^>]*>)?", n).group(0) for n in names[cs.name]) or "(no launch)"
        worst[form] = max(worst.get(form, 0.0), ratio)
    return failures, worst


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_reference(ort, family):
    _, _, outs, model, env = _model(family)
    got, names, same, fused = _f32_session(ort, family)
    assert same, "the second run differs from the first"
    cases = HC.groups()[family]
    failures, worst = _check(cases, outs, model, env, got, names)
    for form, ratio in sorted(worst.items()):
        print(f"{family} worst err / bar, {form}: {ratio:.4f}")
    assert not failures, "\n".join(failures)
    assert fused == sum(cs.name in HC.FUSED for cs in cases)
    for cs in cases:  # a fused pattern is k_class_head and nothing else
        if cs.name in HC.FUSED and cs.family == HC.F:
            assert len(names[cs.name]) == 1 and "k_class_head" in names[cs.name][0], (cs.name, names[cs.name])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_16bit_is_f32(ort, family, prec):
    f32_out, f32_names, _, _ = _f32_session(ort, family)
    got, names, same, _ = _session(ort, family, prec)
    assert same, "the second run differs from the first"
    failures = []
    for cs in HC.groups()[family]:
        if names[cs.name] != f32_names[cs.name]:
            failures.append(f"{cs.name}: launched {names[cs.name]}, in f32 {f32_names[cs.name]}")
    for o, g in got.items():
        if not np.array_equal(g, f32_out[o], equal_nan=True):
            failures.append(f"{o}: differs from the f32 session's output")
    assert not failures, "\n".join(failures)


def test_head_unfused_knob(ort):
    """The fused family's f32 session in a child process under VSO_HEAD=0 (read once per process): the Resize on
    k_resize, the head on its plain form, the selection a copy (ArgMax -> Equal -> Cast stays the head's: Equal
    has no kernel) — and every output bitwise the fused session's."""
    fam = HC.F
    cases = HC.groups()[fam]
    _, _, outs, _, _ = _model(fam)
    fused_out, _, _, _ = _f32_session(ort, fam)
    got, info = CH.run_child("VSO_HEAD=0", {"VSO_HEAD": "0"}, f"hd_{fam}:f32")
    inf = info[f"hd_{fam}/f32"]
    assert inf["rerun_equal"]
    launches, k, failures = inf["launches"], 0, []
    for cs in cases:
        m = HC.META[cs.name]
        want = (["k_resize<"] if m["up"] else []) + ["k_class_head<%d, false, " % HC.RED_ID[m["red"]]] + \
               ["k_copy"] * m.get("copies", 0)
        ls = launches[k:k + len(want)]
        k += len(want)
        if len(ls) != len(want) or not all(w in n for w, n in zip(want, ls)):
            failures.append(f"{cs.name}: launched {ls}, expected {want}")
        for o in outs[cs.name]:
            if not np.array_equal(got[f"hd_{fam}/f32/{o}"], fused_out[o], equal_nan=True):
                d = np.abs(got[f"hd_{fam}/f32/{o}"].astype(np.float64) - fused_out[o])
                failures.append(f"{o}: not bitwise the fused session's, {int((d > 0).sum())} elements, max {float(np.nanmax(d)):.3e}")
    assert k == len(launches), launches[k:]
    assert not failures, "\n".join(failures)


def test_forms_are_reached():
    """The table names every instantiation of k_class_head."""
    forms = {k for cs in HC.VALUE_CASES for k in cs.kernels}
    assert set(HC.FORMS) <= forms, sorted(set(HC.FORMS) - forms)
    assert len(HC.FORMS) == 8 and len(HC.TIE_CASES) >= 10 and len(HC.FUSED) >= 40


@pytest.mark.parametrize("name", [k.name for k in HC.REFUSED_CASES])
def test_refused_at_creation(ort, name):
    cs = HC.BY_NAME[name]
    data, _, _ = HC.build([cs])
    with pytest.raises(ort.VsoError, match=HC.NAMES[name]):
        ort.InferenceSession(data, precision="f32").close()
