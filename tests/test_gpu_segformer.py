"""The GPU ONNX sessions (include/vso.h) on a small mix-transformer
segmentation net (tests/onnx_models_segformer.py): two stages of patch
embedding, LayerNorm, efficient self-attention over spatially reduced keys,
Mix-FFN with a depthwise Conv and GELU, and an all-MLP decode head with a
sigmoid matte.  Its two exports — opset 17 with LayerNormalization nodes, opset
13 with everything decomposed — must plan the same launch list: one k_attn per
block, one k_layer_norm per norm, no k_softmax, no launch for a GELU or a
Linear's bias.  Every graph output meets the operator matrix's bar,
|gpu - ref| <= 1e-4 max(1, |ref|), against tests/onnx_ref_attn.py (the net's
float32 evaluation stays within half of it: tests/test_segformer_ref.py),
vso_attn_count is the number of blocks, and vso_run_device is bitwise vso_run.
"""
import numpy as np
import pytest

import onnx_models_segformer as S
import onnx_ref as R
import onnx_ref_attn as RA

pytestmark = pytest.mark.gpu

TOL = 1e-4
_runs = {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _run(ort, opset):
    """(outputs, launches, attn_nodes(), run_device's outputs) of an export's f32 session, once."""
    if opset not in _runs:
        import torch
        data, _, _ = S.segformer(opset)
        feeds = S.feeds()
        with ort.InferenceSession(data, precision="f32") as s:
            got = s.run(feeds)
            din = [torch.from_numpy(feeds[n]).cuda() for n in s.input_names]
            dout = [torch.empty(sh, dtype=torch.float32, device="cuda") for sh in s.output_shapes]
            st = torch.cuda.Stream()
            s.run_device([t.data_ptr() for t in din], [t.data_ptr() for t in dout], st.cuda_stream)
            st.synchronize()
            dev = {n: t.cpu().numpy() for n, t in zip(s.output_names, dout)}
            _runs[opset] = (got, s.launches(), s.attn_nodes(), dev)
    return _runs[opset]


@pytest.mark.parametrize("opset", [17, 13])
def test_export_matches_reference(ort, opset):
    data, _, names = S.segformer(opset)
    want = RA.run(R.load(data), S.feeds())
    got, launches, fused, dev = _run(ort, opset)
    assert sum("k_attn<" in n for n in launches) == S.BLOCKS == fused, launches
    assert sum("k_layer_norm<" in n for n in launches) == S.NORMS, launches
    assert not any("k_softmax" in n for n in launches), launches
    for o in names:
        err = np.abs(got[o].astype(np.float64) - want[o])
        bar = TOL * np.maximum(1.0, np.abs(want[o]))
        print(f"{o} (opset {opset}): max abs err {float(err.max()):.3e}, err / bar {float((err / bar).max()):.4f}")
        assert got[o].shape == want[o].shape and (err <= bar).all(), (o, float(err.max()))
        assert np.array_equal(dev[o], got[o]), f"{o}: vso_run_device differs from vso_run"


def test_exports_plan_the_same_launches(ort):
    _, l17, _, _ = _run(ort, 17)
    _, l13, _, _ = _run(ort, 13)
    assert l17 == l13, (l17, l13)
    # per block: the K Transpose of the attention launches nothing, the GELU and the Linear biases neither
    assert not any("k_unary" in n for n in l17[:-1]), l17  # (the matte's Sigmoid may be the last launch)
    assert sum("k_gemm" in n for n in l17) == S.BLOCKS * 6 + 2, l17  # q, k, v, proj, two of the FFN; the head's two
