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
"""
import numpy as np
import pytest

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
