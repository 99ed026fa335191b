"""The multiclass net of tests/onnx_models_multiclass.py through the TypeScript
host (ts/segment.ts over the Node-API addon): run() returns the int64 label
output as a Tensor of type 'int64' with BigInt64Array data, equal to the Python
host's int64 array; the float outputs are bitwise the Python host's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import onnx_models_multiclass as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = os.path.join(ROOT, "video-stream-segmenetation_amd", "ts")
NODE = shutil.which("node")


@pytest.fixture(scope="module")
def addon_built(pkg):
    if not NODE or not os.path.isdir("/usr/include/node"):
        pytest.skip("node / node headers not available")
    pkg.build()
    subprocess.run(["make", "-s", "-C", os.path.join(TS, "addon")], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("export", ["per_head", "shared"])
def test_node_multiclass_outputs_are_typed(addon_built, pkg, tmp_path, export):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    model, _, names = MC.multiclass(export)
    feeds = MC.feeds()
    mp, ip = tmp_path / "model.onnx", tmp_path / "inputs.bin"
    mp.write_bytes(model)
    np.concatenate([np.ascontiguousarray(v, np.float32).ravel() for v in feeds.values()]).tofile(ip)
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "run_head.js"), str(mp), str(ip), str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info["outputNames"] == names
    assert info["outputTypes"] == ["float32", "int64", "float32"] and info["onnxTypes"] == [1, 7, 1]
    assert info["arrays"] == ["Float32Array", "BigInt64Array", "Float32Array"]
    assert info["headNodes"] == (3 if export == "per_head" else 2) and info["indexFeedRejected"]
    from vss_amd import ort as pyort
    with pyort.InferenceSession(model) as s:
        py = s.run(feeds)
    assert py["labels"].dtype == np.int64
    for k, name in enumerate(names):
        got = np.fromfile(tmp_path / f"out_{k}.bin", py[name].dtype).reshape(py[name].shape)
        assert info["outputDims"][k] == list(py[name].shape)
        assert np.array_equal(got, py[name]), name
