"""The GPU ONNX sessions (include/vso.h) on what the planner does between
nodes: the case table of tests/op_cases_fuse.py — a strided residual read in
a convolution's epilogue (family res), producers writing into a Concat in
place (cat), deferred producers in front of consumers that take or flush them
(pend), the decomposed hard-swish (hswish) — against the float64 oracle
(op_cases_fuse.oracle: oracle/onnx_ref.py, for bf16 / f16 sessions with
conv_operands; itself held to PyTorch's float64 by tests/test_fuse_ref.py).
One session per family and precision, one graph output or more per case.

Every case's launches are asserted by name and order (`kernels` in f32,
`kernels16` in bf16 / f16): a fusion that silently does not happen, or
silently happens, fails.  Bars, none of them new: |gpu - oracle| <= TOL *
max(1, |oracle|) per element with the operator matrix's TOL = 1e-4; a case
with a k_conv_tile_up launch TOL_UP = 1e-3 of the output scale
(tests/test_gpu_conv_tile_matrix.py: an interpolated operand may land one
16-bit step from the oracle's); channels a Concat copies are bitwise its
inputs, so a tile or quad tail that spills into the next input's channels
shows; a second run is bitwise the first.

The knobs are read once per process: each setting is one child process
(tests/fuse_matrix_child.py), one at a time, none started after an abnormal
end.  VSO_LANES=2 against VSO_LANES=1: the packed sessions — many independent
small graphs — must be bitwise equal on two capture lanes and on one.  That
is deterministic for a wrong plan; a missing cross-lane edge is a race, which
this check catches only with some probability.

Worst err / bar per launch form, the near misses, the forms without a case
and the value-only breaks these tests catch: profiles/NOTES.md, "Fusion
matrix".
"""
import re

import numpy as np
import pytest

import fuse_matrix_child as CH
import onnx_ref as R
import op_cases as OC
import op_cases_fuse as FC

pytestmark = pytest.mark.gpu

TOL, TOL_UP = 1e-4, 1e-3
GROUPS = FC.groups()
FAMILIES = sorted(GROUPS)
PRECS = ("f32", "bf16", "f16")
_models, _oracles, _sessions, _children = {}, {}, {}, {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _model(fam):
    """(model bytes, feeds, {case: its graph outputs}) of a family, once."""
    if fam not in _models:
        _models[fam] = OC.build(GROUPS[fam])
    return _models[fam]


def _oracle(fam, prec):
    if (fam, prec) not in _oracles:
        data, feeds, _ = _model(fam)
        _oracles[fam, prec] = FC.oracle(R.load(data), feeds, prec)
    return _oracles[fam, prec]


def _session(ort, fam, prec):
    """(outputs, launches, whether a second run was bitwise the first) of a family's session, once."""
    if (fam, prec) not in _sessions:
        data, feeds, _ = _model(fam)
        with ort.InferenceSession(data, precision=prec) as s:
            got = s.run(feeds)
            again = s.run(feeds)
            launches = s.launches()
        _sessions[fam, prec] = (got, launches, all(np.array_equal(got[o], again[o], equal_nan=True) for o in got))
    return _sessions[fam, prec]


def _expected(cs, prec):
    return cs.kernels if prec == "f32" else cs.kernels16


def _form(names):
    return " + ".join(re.search(r"k_\w+(<[^>]*>)?", n).group(0) for n in names) or "(no launch)"


def _check(fam, prec, got, launches, expected=_expected, label=""):
    """The family's session against the oracle and the table: a list of failures (the worst err / bar per
    launch form is printed)."""
    cases = GROUPS[fam]
    _, feeds, outs = _model(fam)
    want = _oracle(fam, prec)
    total = sum(len(expected(cs, prec)) for cs in cases)
    assert len(launches) == total, (f"{len(launches)} launches, the table has {total}", launches)
    failures, worst, k = [], {}, 0
    for cs in cases:
        exp = expected(cs, prec)
        names = launches[k:k + len(exp)]
        k += len(exp)
        if not all(e in n for e, n in zip(exp, names)):
            failures.append(f"{cs.name}: launched {[_form([n]) for n in names]}, expected {exp}")
        up = any(FC.TILE_UP in n for n in names)
        ratio = 0.0
        for o in outs[cs.name]:
            g, w = got[o], want[o]
            if g.shape != w.shape:
                failures.append(f"{o}: shape {g.shape}, oracle {w.shape}")
                continue
            err = np.abs(g.astype(np.float64) - w)
            bar = TOL_UP * max(1.0, float(np.abs(w).max())) if up else TOL * np.maximum(1.0, np.abs(w))
            ratio = max(ratio, float((err / bar).max()))
            if not (err <= bar).all():
                failures.append(f"{o}: {int((~(err <= bar)).sum())} elements beyond the bar, worst {float(err.max()):.3e}")
        print(f"{label}{prec} {cs.name}: err / bar {ratio:.4f} on {_form(names)}")
        worst[_form(names)] = max(worst.get(_form(names), 0.0), ratio)
        parts = FC.CAT.get(cs.name)
        if parts:  # the Concat's copied channels are bitwise the graph inputs
            y, c0 = got[outs[cs.name][-1]], 0
            k_cat = len(cs.chain) - 1
            for p in parts:
                if p[0] == "in":
                    src = feeds[OC._chain_input_name(cs, k_cat, p[1])]
                    if not np.array_equal(y[:, c0:c0 + p[2]], src):
                        failures.append(f"{cs.name}: channels {c0}..{c0 + p[2] - 1} are not the Concat's input {p[1]}")
                elif cs.op_out and not np.array_equal(y[:, c0:c0 + p[1]], got[outs[cs.name][0]]):
                    failures.append(f"{cs.name}: channels {c0}..{c0 + p[1] - 1} are not the copied producer's output")
                c0 += p[-1]
            assert c0 == y.shape[1], cs.name
            if "miss" not in cs.name:  # one copy per input not written in place
                copies = sum("k_copy" in n for n in names)
                if copies != sum(p[0] == "in" for p in parts):
                    failures.append(f"{cs.name}: {copies} copies for {parts}")
    for form, ratio in sorted(worst.items()):
        print(f"{label}{fam} {prec} worst err / bar, {form}: {ratio:.4f}")
    return failures


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_oracle(ort, family, prec):
    got, launches, same = _session(ort, family, prec)
    failures = _check(family, prec, got, launches)
    assert same, "the second run differs from the first"
    assert not failures, "\n".join(failures)


def test_f32_operands_are_precision_independent(ort):
    """A case none of whose convolutions the oracle rounds (onnx_ref.tiled_conv) launches the same kernels in
    every precision, with bitwise the f32 session's output."""
    failures, n = [], 0
    for fam in FAMILIES:
        _, _, outs = _model(fam)
        f32 = _session(ort, fam, "f32")[0]
        for prec in ("bf16", "f16"):
            got = _session(ort, fam, prec)[0]
            for cs in GROUPS[fam]:
                if cs.kernels16 != cs.kernels or FC.TILE in cs.kernels16:
                    continue
                n += 1
                for o in outs[cs.name]:
                    if not np.array_equal(got[o], f32[o], equal_nan=True):
                        failures.append(f"{prec} {o}: differs from the f32 session's output")
    assert n >= 100
    assert not failures, "\n".join(failures)


# ---- the planner's knobs: one child process per setting ---------------------------------------------------
SETTINGS = {
    "lanes2": ({"VSO_LANES": "2"}, "fu_res:f32;fu_cat:f32;fu_pend:f32,bf16;fu_hswish:f32"),
    "lanes1": ({"VSO_LANES": "1"}, "fu_res:f32;fu_cat:f32;fu_pend:f32,bf16;fu_hswish:f32"),
    "up_fuse0": ({"VSO_UP_FUSE": "0"}, "fu_pend:bf16,f16"),
    "cat_tail0": ({"VSO_CAT_TAIL": "0"}, "fu_pend:f32,bf16"),
    "dw_plane0": ({"VSO_DW_PLANE": "0"}, "fu_res:f32;fu_cat:f32"),
    "want1": ({"VSO_CONV_WANT": "1"}, "fu_res:f32,bf16;fu_cat:bf16"),
}


def _child(setting):
    """(outputs, info) of the setting's child process, once."""
    if setting not in _children:
        env, spec = SETTINGS[setting]
        _children[setting] = CH.run_child(setting, env, spec, timeout=180)
    return _children[setting]


def _child_family(setting, fam, prec):
    outs, info = _child(setting)
    inf = info[f"fu_{fam}/{prec}"]
    assert inf["rerun_equal"], (setting, fam, prec)
    pre = f"fu_{fam}/{prec}/"
    return {k[len(pre):]: v for k, v in outs.items() if k.startswith(pre)}, inf


def _swap(launches, old, new):
    out = []
    for k in launches:
        out += list(new) if k == old else [k]
    return tuple(out)


def _expected_under(setting):
    def expected(cs, prec):
        exp = _expected(cs, prec)
        if setting == "up_fuse0":  # the Resize is flushed in front of the convolution that would have computed it
            return _swap(exp, FC.TILE_UP, (FC.RS_Q, FC.TILE))
        if setting == "cat_tail0" and cs.name.startswith("Tail_") and exp[:2] != FC.CC:  # the tail is copied
            return (FC.COPYR,) + exp
        if setting == "cat_tail0" and cs.name == "Up_cat_first_and_tail_taken" and prec != "f32":
            return (FC.COPYR,) + exp
        if setting == "dw_plane0":
            return tuple(FC.DW if k.startswith("k_conv_dw_plane<") else k for k in exp)
        return exp
    return expected


@pytest.mark.parametrize("setting", ["up_fuse0", "cat_tail0", "dw_plane0", "want1"])
def test_family_under_knob(ort, setting):
    """Each family of the setting's child at the bar, on the launches the knob implies.  VSO_UP_FUSE=0: every
    pending Resize is flushed (no k_conv_tile_up).  VSO_CAT_TAIL=0: every Concat input not written in place is
    copied.  VSO_DW_PLANE=0: the k_conv_dw_plane cases on the quad body of k_conv_dw, bitwise the default's
    (the same taps, FMA order and epilogue).  VSO_CONV_WANT=1: k_conv_tile without the K split (the default
    splits these small planes' chunks over workgroups)."""
    failures, moved = [], 0
    for model, precisions in CH.C.parse_spec(SETTINGS[setting][1]):
        fam = model[3:]
        for prec in precisions:
            got, inf = _child_family(setting, fam, prec)
            exp = _expected_under(setting)
            moved += sum(exp(cs, prec) != _expected(cs, prec) for cs in GROUPS[fam])
            failures += _check(fam, prec, got, inf["launches"], exp, label=f"{setting} ")
            if setting == "dw_plane0":
                here = _session(ort, fam, prec)[0]
                failures += [f"{o}: differs from the default session's output" for o in got if not np.array_equal(got[o], here[o])]
            if setting == "up_fuse0":
                assert not any(FC.TILE_UP in n for n in inf["launches"])
    assert moved >= {"up_fuse0": 12, "cat_tail0": 5, "dw_plane0": 2, "want1": 0}[setting], moved
    assert not failures, "\n".join(failures)


def test_two_lanes_equal_one(ort):
    """The packed sessions on two capture lanes (VSO_LANES=2) and on one: bitwise equal outputs, the same
    launches, each child's second run bitwise its first, and lanes() reports 2 and 1.  A wrong plan differs
    deterministically; a missing cross-lane edge is a race this catches only sometimes."""
    two, info2 = _child("lanes2")
    one, info1 = _child("lanes1")
    assert two.keys() == one.keys() and len(two) > 100
    bad = [k for k in two if not np.array_equal(two[k], one[k], equal_nan=True)]
    assert not bad, bad
    for key in info2:
        assert info2[key]["rerun_equal"] and info1[key]["rerun_equal"], key
        assert info2[key]["launches"] == info1[key]["launches"], key
        assert info1[key]["lanes"] == 1, (key, info1[key]["lanes"])
    assert any(inf["lanes"] == 2 for inf in info2.values()), {k: v["lanes"] for k, v in info2.items()}
    # ... and both are this process's sessions' values
    for key in info2:
        model, prec = key.split("/")
        here = _session(ort, model[3:], prec)[0]
        bad = [o for o in here if not np.array_equal(here[o], two[f"{key}/{o}"], equal_nan=True)]
        assert not bad, (key, bad)
