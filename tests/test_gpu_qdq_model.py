"""A statically quantised (QDQ) MobileNet-style segmenter (tests/onnx_models_qdq.py)
through a GPU ONNX session, against the float64 reference
(tests/onnx_ref_quant.py): a strided stem and two inverted residuals with
quantised residual Adds on the fused integer kernels, a bilinear Resize between
DequantizeLinear and QuantizeLinear on the fallback launches in the middle, a
one-channel head, DequantizeLinear -> Sigmoid.  The scales are powers of two
and every accumulator stays below 2^24, so the two quantised outputs — the
head's uint8 tensor and an int8 interior one — must equal the reference's; the
float matte is held to the project's 1e-4 max(1, |ref|)."""
import numpy as np
import pytest

import onnx_models_qdq as MQ
import onnx_ref as R
import onnx_ref_quant as RQ

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


@pytest.fixture(scope="module")
def model():
    data, names, launches, fused = MQ.qdq_segmenter()
    feeds = MQ.feeds()
    return data, names, launches, fused, feeds, RQ.run(R.load(data), feeds)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_qdq_segmenter(ort, model, prec):
    data, names, launches, fused, feeds, want = model
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        ran = s.launches()
        n_fused = s.qconv_nodes()
    assert len(ran) == len(launches) and all(k in n for k, n in zip(launches, ran)), ran
    assert n_fused == fused == 10
    assert got[names["head_q"]].dtype == np.uint8 and got[names["feat_q"]].dtype == np.int8
    assert got[names["matte"]].dtype == np.float32
    for k in ("feat_q", "head_q"):
        g, w = got[names[k]], want[names[k]]
        assert g.shape == w.shape
        d = g.astype(np.int64) - w.astype(np.int64)
        print(f"{k}: {int((d != 0).sum())} of {d.size} quantised values differ")
        assert not d.any(), f"{k}: {int((d != 0).sum())} values differ, first at {tuple(np.argwhere(d != 0)[0])}"
    g, w = got[names["matte"]].astype(np.float64), want[names["matte"]].astype(np.float64)
    err = np.abs(g - w)
    print(f"matte: max abs err {float(err.max()):.3e}")
    assert (err <= TOL * np.maximum(1.0, np.abs(w))).all()
    assert all(np.array_equal(got[o], again[o]) for o in got), "the second run differs from the first"
