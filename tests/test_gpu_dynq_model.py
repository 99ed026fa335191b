"""Two dynamically quantised models (tests/onnx_models_dynq.py) through GPU
ONNX sessions, against the reference (tests/onnx_ref_dynq.py).

The MobileNet-style segmenter is built exact (tests/test_dynq_ref.py asserts
its conditions): every DynamicQuantizeLinear sees a power-of-two range, so
every tensor before the Sigmoid — the stem's output, the second block's, the
upsampled features, the head's — must equal the reference's; the matte is held
to the project's 1e-4 max(1, |ref|).  Every quantised layer is one fused launch
behind its DynamicQuantizeLinear pair; the launch list and dynq_nodes() are
asserted, in f32 and bf16 sessions (the integer layers do not depend on the
session precision, the float Resize between them is exact here).

The transformer block has general scales: LayerNormalization, three
MatMulInteger Linear layers off one DynamicQuantizeLinear, the float attention
core on k_attn (attn_nodes() is asserted), a MatMulInteger projection, the
residual.  Held to 1e-4 max(1, |ref|): a quantised value one step off would
show as x_scale |w| w_scale, some 1e-3 to 1e-2 here, and its input keeps every
element away from a rounding tie (asserted on the CPU)."""
import numpy as np
import pytest

import onnx_models_dynq as MD
import onnx_ref as R
import onnx_ref_dynq as RD

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
def segmenter():
    data, names, _, launches, fused = MD.dynq_segmenter()
    feeds = MD.segmenter_feeds()
    return data, names, launches, fused, feeds, RD.run(R.load(data), feeds)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_dynq_segmenter(ort, segmenter, prec):
    data, names, launches, fused, feeds, want = segmenter
    with ort.InferenceSession(data, precision=prec) as s:
        got = s.run(feeds)
        again = s.run(feeds)
        ran = s.launches()
        n_fused = s.dynq_nodes()
    assert len(ran) == len(launches) and all(k in n for k, n in zip(launches, ran)), ran
    assert n_fused == fused == 8
    for k in ("stem", "feat", "up", "head"):
        g, w = got[names[k]], want[names[k]]
        assert g.shape == w.shape and g.dtype == np.float32
        bad = np.argwhere(g != w)
        print(f"{k}: {len(bad)} of {w.size} values differ")
        assert not len(bad), f"{k}: {len(bad)} values differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"
    g, w = got[names["matte"]].astype(np.float64), want[names["matte"]].astype(np.float64)
    err = np.abs(g - w)
    print(f"matte: max abs err {float(err.max()):.3e}")
    assert (err <= TOL * np.maximum(1.0, np.abs(w))).all()
    assert all(np.array_equal(got[o], again[o]) for o in got), "the second run differs from the first"


def test_dynq_transformer(ort):
    data, out, _ = MD.dynq_transformer()
    feeds = MD.transformer_feeds()
    want = RD.run(R.load(data), feeds)[out].astype(np.float64)
    with ort.InferenceSession(data, precision="f32") as s:
        got = s.run(feeds)
        again = s.run(feeds)
        ran = s.launches()
        assert s.attn_nodes() == 1 and s.dynq_nodes() == 4
    assert sum(MD.TILE in n for n in ran) == 4 and sum(MD.DYNQ in n for n in ran) == 2 and sum("k_attn" in n for n in ran) == 1, ran
    assert not any("k_cast_i32" in n for n in ran), ran
    err = np.abs(got[out].astype(np.float64) - want)
    print(f"y: max abs err {float(err.max()):.3e}, max |ref| {float(np.abs(want).max()):.2f}")
    assert (err <= TOL * np.maximum(1.0, np.abs(want))).all(), f"{int((err > TOL * np.maximum(1.0, np.abs(want))).sum())} elements beyond the bar"
    assert np.array_equal(got[out], again[out]), "the second run differs from the first"
