"""Families of tests/op_cases_fuse.py under one setting of the planner's knobs
(VSO_LANES, VSO_UP_FUSE, VSO_CAT_TAIL, VSO_DW_PLANE, VSO_CONV_WANT: read once
per process, so every setting but the default runs as a child process):

    python tests/fuse_matrix_child.py "fu_res:f32;fu_pend:bf16,f16" > out.npz

The archive is tests/conv_matrix_child.py's — every output of every session's
first run (key "<model>/<precision>/<graph output>") and "info", one JSON
object per session — with "fu_<family>" naming a family of op_cases_fuse and
each session's info holding its lanes() too.  run_child() is the parent's
side; it shares conv_matrix_child's record of a child that ended abnormally,
after which no further child is started."""
import io
import json
import os
import subprocess
import sys

import numpy as np

import conv_matrix_child as C


def _model(model):
    """(bytes, feeds, one key per graph output, in order) of "fu_<family>"."""
    import op_cases as OC
    import op_cases_fuse as FC
    assert model.startswith("fu_"), model
    cases = FC.groups()[model[3:]]
    data, f, outs = OC.build(cases)
    return data, f, [o for cs in cases for o in outs[cs.name]]


def run_sessions(ort, spec):
    """conv_matrix_child.run_sessions, with lanes() in each session's info."""
    outs, info = {}, {}
    for model, precisions in C.parse_spec(spec):
        data, f, keys = _model(model)
        for prec in precisions:
            with ort.InferenceSession(data, precision=prec) as s:
                got = s.run(f)
                again = s.run(f)
                assert list(s.output_names) == keys
                for k in keys:
                    outs[f"{model}/{prec}/{k}"] = got[k]
                info[f"{model}/{prec}"] = {"launches": s.launches(), "tile_convs": s.tile_convs(), "lanes": s.lanes(),
                                           "rerun_equal": all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)}
    return outs, info


def run_child(tag, env, spec, timeout=120):
    """conv_matrix_child.run_child for this script: run_sessions()'s pair of the sessions `spec` names,
    in a child process with `env` added."""
    if C.ABNORMAL:
        raise AssertionError(f"not started: an earlier child ended abnormally ({C.ABNORMAL[0]})")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), spec], cwd=C.ROOT, env=dict(os.environ, **env),
                           capture_output=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        C.ABNORMAL.append(f"{tag}: no exit within {timeout} s")
        raise AssertionError(C.ABNORMAL[0])
    err = r.stderr.decode(errors="replace")
    if C.abnormal(r.returncode) or "illegal memory access" in err:
        C.ABNORMAL.append(f"{tag}: exit status {r.returncode}")
        raise AssertionError(C.ABNORMAL[0] + "\n" + err[-2000:])
    assert r.returncode == 0, (tag, r.returncode, err[-2000:])
    with np.load(io.BytesIO(r.stdout)) as z:
        outs = {k: z[k] for k in z.files if k != "info"}
        info = json.loads(bytes(z["info"]).decode())
    return outs, info


if __name__ == "__main__":
    C.run_sessions = run_sessions
    C.main(sys.argv[1])
