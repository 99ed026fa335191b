"""Time dynamically quantised graphs on the GPU ONNX sessions (include/vso.h):

  segmenter  the dynamic MobileNet-style segmenter of tests/onnx_models_dynq.py
             scaled to 288x512;
  modnet     the MODNet topology (tests/onnx_models.py) at 288x512 with every
             convolution rewritten to the dynamic form (onnx_models_dynq.to_dynamic);

each at batch 1 and batch 8, three ways: `fused` (the session's own plan:
k_iconv_tile / k_iconv_direct with the float epilogue), `unfused` (VSO_DYNQ=0:
the integer launch, k_cast_i32, the Mul / Add / Clip launches) and `float` (the
f32 session of the float model: the yardstick).  The DynamicQuantizeLinear pair
(k_dyn_minmax + k_dyn_quantize) is timed on its own too, at the sizes the
segmenter's layers read: eight of them on one input, nothing else in the graph.

Inputs and outputs stay in HBM; one vso_run_device (hipGraph replay) per
iteration, HIP events on the run's stream, --windows windows of --iters runs
after --warmup runs, the median window reported.  VSO_DYNQ is read once per
process, so each form runs in a child process of its own (a fresh process each,
one at a time, none started after one ended abnormally).  One JSON line per
measurement.

    python tools/bench_dynq.py > profiles/dynq_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FORMS = ("fused", "unfused", "float")


def models(what, batch, form):
    """(model bytes, the session's input shape) of `what` in `form`."""
    import onnx_models as M
    import onnx_models_dynq as MD
    shape = (batch, 3, 288, 512)
    if what == "segmenter":
        return MD.dynq_segmenter(shape, float_model=form == "float")[0], shape
    data = M.modnet(288, 512)
    return (data if form == "float" else MD.to_dynamic(data)), shape


def quantise_only(shape, reps=8):
    """`reps` DynamicQuantizeLinear nodes of one input, their scales the graph outputs: 2 * reps launches, nothing else."""
    import onnx_models as M
    b = M.Builder(0)
    outs = [(b.op("DynamicQuantizeLinear", ["x"], n_out=3)[1], []) for _ in range(reps)]
    return b.model([("x", list(shape))], outs)


def child(args):
    import torch
    torch.cuda.init()
    import bench
    bench._load_pkg()
    import vss_amd.ort as ort
    from bench_qdq import time_session
    form = args.child
    for what in ("segmenter", "modnet"):
        for batch in (1, 8):
            data, shape = models(what, batch, form)
            ms, launches = time_session_shaped(ort, data, shape, args, time_session)
            quant = sum(n in ("k_dyn_minmax", "k_dyn_quantize") for n in launches)
            integer = sum(n in ("k_iconv_tile", "k_iconv_direct") for n in launches)
            # (a fused plan has no k_cast_i32 left: every integer launch ends in float32)
            assert ("k_cast_i32" not in launches) == (form != "unfused") and (quant > 0) == (form != "float"), (form, launches)
            print(json.dumps({"what": f"{what}_288x512_b{batch}", "form": form, "ms_per_run": round(ms, 4),
                              "launches": len(launches), "integer_launches": integer, "quantise_launches": quant}), flush=True)
    if form != "fused":
        return
    # the DynamicQuantizeLinear pair alone, at the sizes the segmenter's layers read
    for batch in (1, 8):
        for shp in ((batch, 3, 288, 512), (batch, 16, 144, 256), (batch, 32, 144, 256), (batch, 16, 288, 512)):
            ms, launches = time_session_shaped(ort, quantise_only(shp), shp, args, time_session)
            assert launches == ["k_dyn_minmax", "k_dyn_quantize"] * 8, launches
            print(json.dumps({"what": "dynamic_quantize_pair", "shape": list(shp), "us_per_pair": round(1e3 * ms / 8, 2)}), flush=True)


def time_session_shaped(ort, data, shape, args, time_session):
    """bench_qdq.time_session on a session created at `shape` (the batch is the caller's)."""
    class _Shaped:
        @staticmethod
        def InferenceSession(model, precision="f32"):
            return ort.InferenceSession(model, input_shape=shape, precision=precision)
    return time_session(_Shaped, data, "f32", args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", choices=FORMS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    for form in FORMS:
        env = dict(os.environ)
        env.pop("VSO_DYNQ", None)
        if form == "unfused":
            env["VSO_DYNQ"] = "0"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--iters", str(args.iters),
               "--windows", str(args.windows), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
        sys.stdout.write("".join(line + "\n" for line in p.stdout.splitlines() if line.startswith("{")))
        sys.stdout.flush()
        if p.returncode != 0:  # (nothing more is started on the GPU after an abnormal end)
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"bench_dynq: the {form} child ended with {p.returncode}")


if __name__ == "__main__":
    main()
