"""Time the attention core of the GPU ONNX sessions (include/vso.h) fused and
unfused: one-block models Transpose(K) -> MatMul -> Mul(1 / sqrt d) -> Softmax
-> MatMul at SegFormer-B0's four stage shapes for a 288x512 input, (Nq, Nk,
heads, d) = (9216, 144, 1, 32), (2304, 144, 2, 32), (576, 144, 5, 32),
(144, 144, 8, 32), at batch 1 and 8, each two ways:

  fused    the session's own plan: one k_attn launch (vso_attn.hip)
  unfused  the same model under VSO_ATTN=0: k_copy, k_gemm, k_binary,
           k_softmax, k_gemm — the [B, h, Nq, Nk] scores through HBM

Q, K, V and the output stay in HBM; one vso_run_device (hipGraph replay) per
iteration, HIP events on the run's stream, --windows windows of --iters runs
after --warmup runs, the median window reported.  VSO_ATTN is read once per
process, so each form runs in a child process of its own (a fresh process
each, one at a time, none started after one ended abnormally), --rounds rounds
of the two forms alternating; the parent prints one JSON line per shape, batch
and form with the median over rounds and the spread, and the fused form's
speed-up over the unfused one.

    python tools/bench_attn.py [--rounds 3] [--iters 200] [--windows 5]
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

# name: (Nq, Nk, heads, d)
SHAPES = {"stage1_9216x144_h1": (9216, 144, 1, 32), "stage2_2304x144_h2": (2304, 144, 2, 32),
          "stage3_576x144_h5": (576, 144, 5, 32), "stage4_144x144_h8": (144, 144, 8, 32)}
BATCHES = (1, 8)
FORMS = ("fused", "unfused")


def block_model(name, batch):
    """(model bytes, the three input shapes) of one attention core."""
    import numpy as np
    import onnx_models as M
    nq, nk, h, d = SHAPES[name]
    b = M.Builder(5)
    kt = b.op("Transpose", ["k"], perm=[0, 1, 3, 2])
    s = b.op("Mul", [b.op("MatMul", ["q", kt]), b.const(np.float32(d ** -0.5))])
    b.nodes.append(M.R.make_node("MatMul", [b.op("Softmax", [s], axis=-1), "v"], ["y"]))
    shapes = [[batch, h, nq, d], [batch, h, nk, d], [batch, h, nk, d]]
    return b.model(list(zip(("q", "k", "v"), shapes)), [("y", [batch, h, nq, d])]), shapes


def child(args):
    """One form, every shape and batch: a JSON line each (ms per run: the median window)."""
    import numpy as np
    import torch
    import bench
    bench._load_pkg()
    import vss_amd.ort as ort
    form = args.child
    for name in SHAPES:
        for batch in BATCHES:
            model, shapes = block_model(name, batch)
            with ort.InferenceSession(model, precision="f32") as s:
                launches = s.launches()
                assert (len(launches) == 1 and "k_attn" in launches[0]) if form == "fused" else len(launches) == 5, \
                    (form, launches)
                g = torch.Generator(device="cpu").manual_seed(1)
                ins = [torch.randn(sh, generator=g, dtype=torch.float32).cuda() for sh in shapes]
                y = torch.empty(s.output_shapes[0], dtype=torch.float32, device="cuda")
                st = torch.cuda.Stream()
                torch.cuda.synchronize()
                ip, op = [t.data_ptr() for t in ins], [y.data_ptr()]
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
                print(json.dumps({"shape": name, "batch": batch, "form": form, "ms": statistics.median(windows),
                                  "launches": [n.split("(")[0].split("::")[-1] for n in launches],
                                  "checksum": float(np.abs(out.astype(np.float64)).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
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
            env.pop("VSO_ATTN", None)
            if form == "unfused":
                env["VSO_ATTN"] = "0"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--iters", str(args.iters),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:  # (nothing more is started on the GPU after an abnormal end)
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_attn: the {form} child ended with {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    res.setdefault((r["shape"], r["batch"], r["form"]), []).append(r)
            print(f"bench_attn: round {rnd + 1}, {form} done", file=sys.stderr, flush=True)
    for (shape, batch, form), rs in sorted(res.items()):
        ms = [r["ms"] for r in rs]
        med = statistics.median(ms)
        other = statistics.median(r["ms"] for r in res[(shape, batch, "unfused")])
        sums = {f: res[(shape, batch, f)][0]["checksum"] for f in FORMS}
        print(json.dumps({"shape": shape, "batch": batch, "form": form, "us_per_run": round(1e3 * med, 2),
                          "us_min": round(1e3 * min(ms), 2), "us_max": round(1e3 * max(ms), 2), "rounds": len(ms),
                          "launches": rs[0]["launches"], "speedup_over_unfused": round(other / med, 3),
                          "sum_abs_rel_to_fused": round(rs[0]["checksum"] / sums["fused"], 7)}), flush=True)


if __name__ == "__main__":
    main()
