"""Time the class heads of the GPU ONNX sessions (include/vso.h) fused and
unfused: one-head models Resize(linear, x4) -> a reduction over the classes,
at batch 8, logits (C, h, w) = (19, 128, 128) and (150, 128, 128) -> 512x512
and (21, 72, 128) -> 288x512, two reductions each:

  argmax   ArgMax over the classes: the [8, 1, H, W] label plane
  softmax  Softmax -> Gather(class 1): one [8, H, W] probability plane

each two ways:

  fused    the session's own plan: one k_class_head launch (vso_head.hip)
           that interpolates every logit on the fly
  unfused  the same model under VSO_HEAD=0: k_resize writes the [8, C, H, W]
           logits, the plain k_class_head reads them back (and k_copy_rows
           selects the channel)

The low-resolution logits and the output stay in HBM; one vso_run_device
(hipGraph replay) per iteration, HIP events on the run's stream, --windows
windows of --iters runs after --warmup runs, the median window reported.
VSO_HEAD is read once per process, so each form runs in a child process of its
own (a fresh process each, one at a time, none started after one ended
abnormally), --rounds rounds of the two forms alternating; the parent prints
one JSON line per shape, reduction and form with the median over rounds and
the spread, and the fused form's speed-up over the unfused one.

    python tools/bench_head.py [--rounds 3] [--iters 100] [--windows 5] > profiles/head_bench.jsonl
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

# name: (C, h, w): the logits, upsampled x4
SHAPES = {"c19_128x128": (19, 128, 128), "c150_128x128": (150, 128, 128), "c21_72x128": (21, 72, 128)}
BATCH, SCALE = 8, 4
REDUCTIONS = ("argmax", "softmax")
FORMS = ("fused", "unfused")


def head_model(name, red):
    """(model bytes, the input shape) of one class head behind its Resize."""
    import numpy as np
    import onnx_models as M
    c, h, w = SHAPES[name]
    b = M.Builder(5)
    up = b.op("Resize", ["x", "", b.const(np.array([1, 1, SCALE, SCALE], np.float32))], mode="linear",
              coordinate_transformation_mode="half_pixel")
    if red == "argmax":
        b.nodes.append(M.R.make_node("ArgMax", [up], ["y"], axis=1, keepdims=1))
        out = [BATCH, 1, SCALE * h, SCALE * w]
    else:
        b.nodes.append(M.R.make_node("Gather", [b.op("Softmax", [up], axis=1), b.const(np.asarray(1, np.int64))], ["y"], axis=1))
        out = [BATCH, SCALE * h, SCALE * w]
    return b.model([("x", [BATCH, c, h, w])], [("y", out)]), [BATCH, c, h, w]


def child(args):
    """One form, every shape and reduction: a JSON line each (ms per run: the median window)."""
    import numpy as np
    import torch
    import bench
    bench._load_pkg()
    import vss_amd.ort as ort
    form = args.child
    for name in SHAPES:
        for red in REDUCTIONS:
            model, shape = head_model(name, red)
            with ort.InferenceSession(model, precision="f32") as s:
                launches = s.launches()
                want = 1 if form == "fused" else 2 if red == "argmax" else 3
                assert len(launches) == want and ("k_resize" in launches[0]) == (form == "unfused"), (form, launches)
                g = torch.Generator(device="cpu").manual_seed(1)
                x = (3.0 * torch.randn(shape, generator=g, dtype=torch.float32)).cuda()
                y = torch.empty(s.output_shapes[0], dtype=torch.float32, device="cuda")
                st = torch.cuda.Stream()
                torch.cuda.synchronize()
                ip, op = [x.data_ptr()], [y.data_ptr()]
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
                out = y.cpu().numpy()
                print(json.dumps({"shape": name, "reduction": red, "form": form, "ms": statistics.median(windows),
                                  "launches": [n.split("(")[0].split("::")[-1] for n in launches],
                                  "checksum": float(np.abs(out.astype(np.float64)).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--child", choices=FORMS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {}
    for rnd in range(args.rounds):
        for form in FORMS:
            env = dict(os.environ)
            env.pop("VSO_HEAD", None)
            if form == "unfused":
                env["VSO_HEAD"] = "0"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--iters", str(args.iters),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:  # (nothing more is started on the GPU after an abnormal end)
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_head: the {form} child ended with {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    res.setdefault((r["shape"], r["reduction"], r["form"]), []).append(r)
            print(f"bench_head: round {rnd + 1}, {form} done", file=sys.stderr, flush=True)
    for (shape, red, form), rs in sorted(res.items()):
        ms = [r["ms"] for r in rs]
        med = statistics.median(ms)
        other = statistics.median(r["ms"] for r in res[(shape, red, "unfused")])
        sums = {f: res[(shape, red, f)][0]["checksum"] for f in FORMS}
        print(json.dumps({"shape": shape, "batch": BATCH, "reduction": red, "form": form, "us_per_run": round(1e3 * med, 2),
                          "us_min": round(1e3 * min(ms), 2), "us_max": round(1e3 * max(ms), 2), "rounds": len(ms),
                          "launches": rs[0]["launches"], "speedup_over_unfused": round(other / med, 3),
                          "sum_abs_rel_to_fused": round(rs[0]["checksum"] / sums["fused"], 7)}), flush=True)


if __name__ == "__main__":
    main()
