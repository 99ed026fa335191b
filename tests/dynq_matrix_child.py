"""A family of tests/op_cases_dynq.py under one setting of the dynamic
quantisation knob (VSO_DYNQ: read once per process, so every setting but the
default runs as a child process):

    python tests/dynq_matrix_child.py d_chain:f32 > out.npz

The child and its archive are tests/conv_matrix_child.py's (the same keys and
"info"), with "d_<family>" naming a family of op_cases_dynq, and "dynq_nodes"
added to each session's info.  run_child() is the parent's side; it shares
conv_matrix_child's record of a child that ended abnormally, after which no
further child is started."""
import io
import json
import os
import subprocess
import sys

import numpy as np

import conv_matrix_child as C


def _model(model):
    """(bytes, feeds, one key per graph output, in order) of "d_<family>"."""
    import op_cases_dynq as DC
    assert model.startswith("d_"), model
    cases = DC.groups()[model[2:]]
    data, f, built = DC.build(cases)
    return data, f, [o for cs in cases for o in built[cs.name].outs]


def run_sessions(ort, spec):
    """conv_matrix_child.run_sessions, with vso_dynq_count in each session's info."""
    outs, info = {}, {}
    for model, precisions in C.parse_spec(spec):
        data, f, cases = _model(model)
        for prec in precisions:
            with ort.InferenceSession(data, precision=prec) as s:
                got = s.run(f)
                again = s.run(f)
                assert len(s.output_names) == len(cases)
                for case, name in zip(cases, s.output_names):
                    outs[f"{model}/{prec}/{case}"] = got[name]
                info[f"{model}/{prec}"] = {"launches": s.launches(), "dynq_nodes": s.dynq_nodes(),
                                           "rerun_equal": all(np.array_equal(got[k], again[k]) for k in got)}
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
