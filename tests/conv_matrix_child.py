"""Sessions of the k_conv_tile matrix models (onnx_models.conv_tile_matrix /
conv_up_matrix) under one setting of the planner's knobs — which are read
once per process, so every setting but the default runs as a child process:

    python tests/conv_matrix_child.py <spec> > out.npz

spec: "plain:f32,bf16,f16;up:bf16,f16" — the models and the precisions to
run, one after another.  Writes an .npz to its standard output: every output
of every session's first run (key "<model>/<precision>/<case>") and "info",
the bytes of one JSON object {"<model>/<precision>": {"launches": [...],
"tile_convs": n, "ir_blocks": n, "rerun_equal": bool}}.  A model "op_<family>" is that family
of the operator matrix (tests/op_cases.py), its outputs keyed by graph output
name.  run_child() is the parent's side (tests/test_gpu_conv_tile_matrix.py,
tests/test_gpu_op_matrix.py): it starts no further child once one has ended
abnormally."""
import importlib.util
import io
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import onnx_models as M  # noqa: E402

MODELS = {"plain": (M.conv_tile_matrix, M.CONV_TILE_MATRIX_FEEDS, M.CONV_TILE_MATRIX_CASES, 41),
          "up": (M.conv_up_matrix, M.CONV_UP_MATRIX_FEEDS, M.CONV_UP_MATRIX_CASES, 42)}


def feeds(model):
    _, shapes, _, seed = MODELS[model]
    return M.matrix_feeds(shapes, seed)


def parse_spec(spec):
    return [(part.split(":")[0], part.split(":")[1].split(",")) for part in spec.split(";")]


def _model(model):
    """(bytes, feeds, one key per graph output, in order) of a model of a spec."""
    if model.startswith("op_"):
        import op_cases as OC
        cases = OC.groups()[model[3:]]
        data, f, outs = OC.build(cases)
        return data, f, [o for cs in cases for o in outs[cs.name]]
    return MODELS[model][0](), feeds(model), MODELS[model][2]


def run_sessions(ort, spec):
    """({"<model>/<precision>/<case>": output}, {"<model>/<precision>": info})
    of the sessions `spec` names, in this process."""
    outs, info = {}, {}
    for model, precisions in parse_spec(spec):
        data, f, cases = _model(model)
        for prec in precisions:
            with ort.InferenceSession(data, precision=prec) as s:
                got = s.run(f)
                again = s.run(f)
                assert len(s.output_names) == len(cases)
                for case, name in zip(cases, s.output_names):
                    outs[f"{model}/{prec}/{case}"] = got[name]
                info[f"{model}/{prec}"] = {"launches": s.launches(), "tile_convs": s.tile_convs(),
                                           "ir_blocks": s.ir_blocks(), "rerun_equal": all(np.array_equal(got[k], again[k]) for k in got)}
    return outs, info


# ---- the parent's side ----------------------------------------------------------
ABNORMAL = []  # the first child that ended abnormally: no child is started after it


def abnormal(returncode):
    """A fault, an abort or a segmentation fault (a timeout is handled by the caller)."""
    return returncode < 0 or returncode in (134, 139)


def run_child(tag, env, spec, timeout=120):
    """Run `spec` in a child process with `env` added; returns run_sessions()'s
    pair.  Raises AssertionError on any failure, and without starting the
    child when an earlier one ended abnormally."""
    if ABNORMAL:
        raise AssertionError(f"not started: an earlier child ended abnormally ({ABNORMAL[0]})")
    # (the outputs come back through the child's standard output: tens of MB per setting, no file)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), spec], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        ABNORMAL.append(f"{tag}: no exit within {timeout} s")
        raise AssertionError(ABNORMAL[0])
    err = r.stderr.decode(errors="replace")
    # (a GPU fault the runtime reports as an error code ends the child with a Python exception)
    if abnormal(r.returncode) or "illegal memory access" in err:
        ABNORMAL.append(f"{tag}: exit status {r.returncode}")
        raise AssertionError(ABNORMAL[0] + "\n" + err[-2000:])
    assert r.returncode == 0, (tag, r.returncode, err[-2000:])
    with np.load(io.BytesIO(r.stdout)) as z:
        outs = {k: z[k] for k in z.files if k != "info"}
        info = json.loads(bytes(z["info"]).decode())
    return outs, info


def main(spec):
    out_fd = os.dup(1)
    os.dup2(2, 1)  # whatever a library prints goes to the error stream, not into the archive
    pkg_dir = os.path.join(ROOT, "video-stream-segmenetation_amd")
    sp = importlib.util.spec_from_file_location("vss_amd", os.path.join(pkg_dir, "__init__.py"),
                                                submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(sp)
    sys.modules["vss_amd"] = mod
    sp.loader.exec_module(mod)
    import vss_amd.ort as ort
    outs, info = run_sessions(ort, spec)
    buf = io.BytesIO()
    np.savez(buf, info=np.frombuffer(json.dumps(info).encode(), np.uint8), **outs)
    with os.fdopen(out_fd, "wb") as f:
        f.write(buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[1])
