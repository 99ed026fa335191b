"""A recurrent matting net in the reference's RVM calling convention
(tests/onnx_models_mnv3.py: hard-swish, squeeze-and-excite on HardSigmoid and
ReduceMean, a ConvGRU per scale, ConvTranspose up-blocks on both kernel forms)
through the GPU ONNX sessions, three frames from zero states, each side
feeding its own r*o back as r*i.

Every output of every step meets the operator matrix's bar against the
float64 reference (tests/onnx_ref_ext.py): |gpu - ref| <= 1e-4 * max(1, |ref|).
The device path (vso_run_device on torch tensors, two sets of state buffers
exchanged per frame as frameProcessorRVM.ts swaps r*o into r*i) is bitwise
the host path.  The opset-13 build (hard-swish as Mul(x, HardSigmoid(x)))
plans the launch list of the opset-14 build (the HardSwish operator), with
every hard-swish inside its producer's launch.
"""
import numpy as np
import pytest

import onnx_models_mnv3 as MN
import onnx_ref as R
import onnx_ref_ext as X

pytestmark = pytest.mark.gpu

TOL = 1e-4
STEPS = 3
STATES = (("r1i", "r1o"), ("r2i", "r2o"))
_ref = {}


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


def _reference(opset):
    """(model, shapes, frames, the reference's outputs per step) of a build, once."""
    if opset not in _ref:
        data, shapes, outs = MN.rvm_like(opset)
        model = R.load(data)
        src = MN.frames(STEPS, shapes["src"])
        state = {i: np.zeros(shapes[i], np.float32) for i, _ in STATES}
        steps = []
        for t in range(STEPS):
            y = X.run(model, {"src": src[t], **state})
            steps.append(y)
            state = {i: y[o] for i, o in STATES}
        _ref[opset] = (data, shapes, src, steps)
    return _ref[opset]


def _host_steps(s, shapes, src):
    state = {i: np.zeros(shapes[i], np.float32) for i, _ in STATES}
    steps = []
    for t in range(STEPS):
        y = s.run({"src": src[t], **state})
        steps.append(y)
        state = {i: y[o] for i, o in STATES}
    return steps


@pytest.mark.parametrize("opset", [14, 13])
def test_three_frames_match_reference(ort, opset):
    data, shapes, src, want = _reference(opset)
    with ort.InferenceSession(data, precision="f32") as s:
        assert s.input_names == ["src", "r1i", "r2i"] and s.output_names == ["pha", "r1o", "r2o"]
        assert s.output_shapes == [(1, 1) + shapes["src"][2:], shapes["r1i"], shapes["r2i"]]
        names = s.launches()
        got = _host_steps(s, shapes, src)
    assert sum("k_deconv_tile<" in n for n in names) == 1 and sum("k_deconv_direct(" in n for n in names) == 1, names
    failures = []
    for t in range(STEPS):
        for o, w in want[t].items():
            err = np.abs(got[t][o].astype(np.float64) - w)
            bar = TOL * np.maximum(1.0, np.abs(w))
            print(f"opset {opset} frame {t} {o}: max abs err {float(err.max()):.3e}, err / bar {float((err / bar).max()):.4f}")
            if not (err <= bar).all():
                failures.append(f"frame {t} {o}: worst {float(err.max()):.3e}")
    # (the states move: a frame's outputs are not the frame before's)
    assert not np.array_equal(got[1]["r2o"], got[2]["r2o"]) and float(np.abs(got[2]["r1o"]).max()) > 0.05
    assert not failures, "\n".join(failures)


def test_device_path_is_the_host_path(ort):
    import torch
    data, shapes, src, _ = _reference(14)
    with ort.InferenceSession(data, precision="f32") as s:
        host = _host_steps(s, shapes, src)
        dev = torch.device("cuda:0")
        # two sets of state buffers: a frame reads one and writes the other
        sets = [{k: torch.zeros(shapes[k], dtype=torch.float32, device=dev) for k, _ in STATES} for _ in range(2)]
        pha = torch.empty(s.output_shapes[0], dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream()
        for t in range(STEPS):
            x = torch.from_numpy(src[t]).to(dev)
            torch.cuda.synchronize()  # (the buffers' fills and the upload ran on torch's stream)
            rd, wr = sets[t % 2], sets[(t + 1) % 2]
            s.run_device([x.data_ptr(), rd["r1i"].data_ptr(), rd["r2i"].data_ptr()],
                         [pha.data_ptr(), wr["r1i"].data_ptr(), wr["r2i"].data_ptr()], stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(pha.cpu().numpy(), host[t]["pha"])
            for i, o in STATES:
                assert np.array_equal(wr[i].cpu().numpy(), host[t][o]), (t, o)


def test_opset13_build_plans_the_opset14_launches(ort):
    lists = {}
    for opset in (13, 14):
        with ort.InferenceSession(_reference(opset)[0], precision="f32") as s:
            lists[opset] = s.launches()
    assert lists[13] == lists[14]
    # 5 hard-swishes and no launch of their own: neither a k_unary nor a Mul beyond the gates' and the GRUs'
    assert not any("k_unary" in n for n in lists[14]), lists[14]
