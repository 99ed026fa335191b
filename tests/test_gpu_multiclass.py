"""A multiclass segmentation net (tests/onnx_models_multiclass.py) in the GPU
ONNX sessions, against the float64 reference tests/onnx_ref_head.py: the
person probability (Softmax -> Gather), the int64 labels (ArgMax) and the
person mask (ArgMax -> Equal -> Cast) behind a Resize x4 of 21-class logits.

The exporter's form, one Resize read by the three heads, is a near miss: the
logits are materialised by one k_resize and the heads run on their plain
forms.  The export with a Resize per output plans three fused heads and no
k_resize.  Both meet the 1e-4 bar on the probability and the label rule of
tests/test_gpu_head_matrix.py on labels and mask; the labels are declared
int64 and run() returns them so; vso_run_device is bitwise vso_run (float32
buffers, the labels as exact integers).
"""
import numpy as np
import pytest

import onnx_models_multiclass as MC
import onnx_ref as R
import onnx_ref_head as RH
from test_gpu_head_matrix import TOL, label_failures

pytestmark = pytest.mark.gpu

_runs, _refs = {}, {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _ref(export):
    if export not in _refs:
        m = R.load(MC.multiclass(export)[0])
        _refs[export] = (m, RH.run_all(m, MC.feeds()))
    return _refs[export]


def _run(ort, export):
    """(outputs, launches, head_nodes(), output_types, run_device's outputs) of an export's f32 session, once."""
    if export not in _runs:
        import torch
        data, _, _ = MC.multiclass(export)
        feeds = MC.feeds()
        with ort.InferenceSession(data, precision="f32") as s:
            got = s.run(feeds)
            din = [torch.from_numpy(feeds[n]).cuda() for n in s.input_names]
            dout = [torch.empty(sh, dtype=torch.float32, device="cuda") for sh in s.output_shapes]
            st = torch.cuda.Stream()
            s.run_device([t.data_ptr() for t in din], [t.data_ptr() for t in dout], st.cuda_stream)
            st.synchronize()
            dev = {n: t.cpu().numpy() for n, t in zip(s.output_names, dout)}
            _runs[export] = (got, s.launches(), s.head_nodes(), list(s.output_types), dev)
    return _runs[export]


@pytest.mark.parametrize("export", ["shared", "per_head"])
def test_export_matches_reference(ort, export):
    model, env = _ref(export)
    got, launches, fused, types, dev = _run(ort, export)
    heads = [n for n in launches if "k_class_head" in n]
    if export == "shared":  # the near miss: the logits materialised once, three plain heads
        assert sum("k_resize<" in n for n in launches) == 1 and fused == 2, launches
        assert len(heads) == 3 and all("false, true>" in n for n in heads), launches
    else:
        assert not any("k_resize<" in n for n in launches) and fused == 3, launches
        assert len(heads) == 3 and all("true, true>" in n for n in heads), launches
    assert not any("k_copy" in n for n in launches), launches
    assert types == [np.float32, np.int64, np.float32]
    assert got["labels"].dtype == np.int64 and got["person"].dtype == np.float32 and got["mask"].dtype == np.float32
    w = env["person"].astype(np.float64)
    err = np.abs(got["person"].astype(np.float64) - w)
    print(f"person ({export}): max abs err {float(err.max()):.3e}, err / bar {float((err / (TOL * np.maximum(1.0, w))).max()):.4f}")
    assert got["person"].shape == w.shape and (err <= TOL * np.maximum(1.0, np.abs(w))).all()
    failures = []
    for o in ("labels", "mask"):
        assert got[o].shape == env[o].shape
        failures += label_failures(o, got[o], model, env, False)
    assert not failures, "\n".join(failures)
    for o in MC.OUTPUTS:
        assert dev[o].dtype == np.float32 and np.array_equal(dev[o], got[o].astype(np.float32)), \
            f"{o}: vso_run_device differs from vso_run"


def test_exports_agree(ort):
    """The materialised and the fused plan compute the same values, bit for bit."""
    a, b = _run(ort, "shared")[0], _run(ort, "per_head")[0]
    for o in MC.OUTPUTS:
        assert np.array_equal(a[o], b[o]), o
