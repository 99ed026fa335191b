"""A family of tests/op_cases_quant.py under one setting of the quantised
planning knob (VSO_QDQ: read once per process, so every setting but the
default runs as a child process):

    python tests/quant_matrix_child.py q_qconv:f32 > out.npz

The child and its archive are tests/conv_matrix_child.py's (the same keys and
"info"), with "q_<family>" naming a family of op_cases_quant.  run_child() is
the parent's side; it shares conv_matrix_child's record of a child that ended
abnormally, after which no further child is started."""
import io
import json
import os
import subprocess
import sys

import numpy as np

import conv_matrix_child as C


def _model(model):
    """(bytes, feeds, one key per graph output, in order) of "q_<family>"."""
    import op_cases_quant as QC
    assert model.startswith("q_"), model
    cases = QC.groups()[model[2:]]
    data, f, outs = QC.build(cases)
    return data, f, [o for cs in cases for o in outs[cs.name]]


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
    C._model = _model
    C.main(sys.argv[1])
