"""Time statically quantised (QDQ) graphs on the GPU ONNX sessions (include/vso.h):

  segmenter  the QDQ MobileNet-style segmenter of tests/onnx_models_qdq.py at
             288x512, batch 8, two ways: `fused` (the session's own plan:
             k_qconv_tile / k_qconv_dw / k_qadd on the integers) and `unfused`
             (VSO_QDQ=0: k_dequantize, the float kernel, k_quantize);
  layer      one 3x3 64 -> 64 convolution with Relu at 144x256, batch 8, as the
             difference between a stack of five and a stack of one, divided by
             four: k_qconv_tile in a QDQ stack against k_conv_tile in a bf16
             session of the float stack.

Inputs and outputs stay in HBM; one vso_run_device (hipGraph replay) per
iteration, HIP events on the run's stream, --windows windows of --iters runs
after --warmup runs, the median window reported.  VSO_QDQ is read once per
process, so each form runs in a child process of its own (a fresh process each,
one at a time, none started after one ended abnormally).  One JSON line per
measurement.

    python tools/bench_qdq.py > profiles/qdq_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FORMS = ("fused", "unfused")


def conv_stack(layers, quantised, shape=(8, 64, 144, 256)):
    """`layers` 3x3 convolutions over shape[1] channels with Relu, as a QDQ graph (one k_qconv_tile each, between a
    QuantizeLinear and a quantised output) or as its float counterpart (one k_conv_tile each in a bf16 session)."""
    import numpy as np
    import onnx_models_qdq as MQ
    b = MQ._B(13)
    ch = shape[1]
    if quantised:
        t = b.q("image", 2.0 ** -4, np.uint8(128))
        for _ in range(layers):
            t = b.qconv(t, ch, ch, 3, 2.0 ** -4, np.uint8(0), wmax=1)
        return b.model([("image", list(shape))], [(t[0], list(shape), MQ.R.DT_UINT8)])
    t = "image"
    for _ in range(layers):
        t = b.op("Relu", [b.conv(t, ch, ch, 3)])
    return b.model([("image", list(shape))], [(t, list(shape))])


def time_session(ort, model, precision, args):
    """(ms per run: the median window, the launch names) of a session of `model`."""
    import torch
    with ort.InferenceSession(model, precision=precision) as s:
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.rand(s.input_shapes[0], generator=g, dtype=torch.float32).cuda()
        ys = [torch.empty(shp, dtype=torch.float32, device="cuda") for shp in s.output_shapes]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        ip, op = [x.data_ptr()], [y.data_ptr() for y in ys]
        for _ in range(args.warmup):
            s.run_device(ip, op, st.cuda_stream)
        st.synchronize()
        windows = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.iters):
                s.run_device(ip, op, st.cuda_stream)
            e1.record(st)
            st.synchronize()
            windows.append(e0.elapsed_time(e1) / args.iters)
        return statistics.median(windows), [n.split("(")[0].split("::")[-1] for n in s.launches()]


def child(args):
    import bench
    bench._load_pkg()
    import vss_amd.ort as ort
    import onnx_models_qdq as MQ
    form = args.child
    model, _, _, fused = MQ.qdq_segmenter((8, 3, 288, 512))
    ms, launches = time_session(ort, model, "f32", args)
    assert any("k_qconv_tile" in n for n in launches) == (form == "fused"), launches
    print(json.dumps({"what": "segmenter_288x512_b8", "form": form, "ms_per_run": round(ms, 4), "launches": launches}), flush=True)
    if form != "fused":
        return
    for kind, quantised, prec, kernel in (("k_qconv_tile", True, "f32", "k_qconv_tile"), ("k_conv_tile_bf16", False, "bf16", "k_conv_tile")):
        t = {}
        for layers in (1, 5):
            t[layers], launches = time_session(ort, conv_stack(layers, quantised), prec, args)
            assert sum(kernel in n for n in launches) == layers, launches
        print(json.dumps({"what": "conv3x3_64to64_144x256_b8", "kernel": kind, "us_per_layer": round(1e3 * (t[5] - t[1]) / 4, 2),
                          "ms_1_layer": round(t[1], 4), "ms_5_layers": round(t[5], 4)}), flush=True)


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
        env.pop("VSO_QDQ", None)
        if form == "unfused":
            env["VSO_QDQ"] = "0"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--iters", str(args.iters),
               "--windows", str(args.windows), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        sys.stdout.write("".join(line + "\n" for line in p.stdout.splitlines() if line.startswith("{")))
        sys.stdout.flush()
        if p.returncode != 0:  # (nothing more is started on the GPU after an abnormal end)
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"bench_qdq: the {form} child ended with {p.returncode}")


if __name__ == "__main__":
    main()
