"""The ONNX model reader and the constant folding (csrc/vso_onnx.cpp,
vso_fold.cpp) under AddressSanitizer + UBSan, on the host: they take a user's
file.  csrc/vso_onnx_check.cpp (make onnx-asan) parses each file it is given
and folds its constant nodes; here on the synthetic models, the two golden
MediaPipe models, truncations of two of them and an empty file.  Whole files
must read as oracle/onnx_ref.py reads them; a cut file must be reported ok or
with an error; any ASan / UBSan report fails the run."""
import glob
import os
import subprocess

import pytest

import onnx_models as M
import onnx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-stream-segmenetation_amd", "csrc")
EXE = os.path.join(ROOT, "video-stream-segmenetation_amd", "lib", "vso_onnx_check")


@pytest.fixture(scope="module")
def models():
    out = {n: getattr(M, n)() for n in ("ops_zoo", "conv_zoo", "modnet_like", "q4f16_like", "se_forms")}
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mediapipe_face_*.npz"))):
        out[os.path.splitext(os.path.basename(p))[0]] = M.load_golden(p)[0]
    assert len(out) == 7
    return out


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", CSRC, "onnx-asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")

    def run(paths):
        out = subprocess.run([EXE] + paths, capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(paths)
        return [ln.split("\t") for ln in lines]

    return run


def test_whole_models_read_as_the_oracle_reads_them(models, check, tmp_path):
    paths = []
    for n, data in models.items():
        paths.append(str(tmp_path / (n + ".onnx")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    for (n, data), rec in zip(models.items(), check(paths)):
        assert rec[0] == "ok", (n, rec)
        got = dict(kv.split("=", 1) for kv in rec[1:])
        want = R.load(data)
        assert int(got["opset"]) == want.opset, n
        assert int(got["nodes"]) == len(want.nodes), n
        assert int(got["inits"]) == len(want.inits), n
        assert got["inputs"].split(",") == [i[0] for i in want.inputs], n
        assert got["outputs"].split(",") == [o[0] for o in want.outputs], n


def test_truncated_and_empty_files_end_in_ok_or_an_error(models, check, tmp_path):
    paths = []
    for n in ("ops_zoo", "q4f16_like"):
        data = models[n]
        assert len(data) > 512 + 256
        cuts = list(range(512)) + [512 + (len(data) - 512) * k // 256 for k in range(256)]
        assert len(set(cuts)) == 768 and max(cuts) < len(data)
        for c in cuts:
            paths.append(str(tmp_path / f"{n}_{c}.onnx"))
            with open(paths[-1], "wb") as f:
                f.write(data[:c])
    assert os.path.getsize(paths[0]) == 0  # (the zero-length file: ops_zoo cut at 0)
    for p, rec in zip(paths, check(paths)):
        assert rec[0] == "ok" or (rec[0] == "error" and len(rec) == 2 and rec[1].strip()), (p, rec)
