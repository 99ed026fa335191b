"""Time one-layer ConvTranspose models on the GPU ONNX sessions (include/vso.h):
MODNet-sized decoder steps, 64 -> 32 k4 s2 p1 at 72x128 and 32 -> 16 k2 s2 at
144x256, at batch 1 and 8, each these ways:

  tile    the session's own plan: k_deconv_tile<1 | 2>
  tile_x1 the same model under VSO_DECONV_PAIR=0: k_deconv_tile<1> (one phase
          per workgroup, a row's stores 2 floats apart)
  tile_x2 under VSO_DECONV_PAIR=1: k_deconv_tile<2> (both x phases per
          workgroup, rows stored contiguous)
  direct  the same model under VSO_DECONV_TILE=0: k_deconv_direct
  stuffed the same layer written with operators the sessions ran before they
          had ConvTranspose: nearest Resize x s (asymmetric, floor) -> Mul by a
          constant 0/1 lattice -> Conv with the flipped kernel, pads k - 1 - p
          at the beginning and k - p - s at the end (zero-stuffed form: s^2
          times the multiply-adds, three launches)

Inputs and outputs stay in HBM; one vso_run_device (hipGraph replay) per
iteration, HIP events on the run's stream, --windows windows of --iters runs
after --warmup runs, the median window reported.  The VSO_DECONV_* knobs are
read once per process, so every form runs in a child process of its own (a
fresh process each, one at a time, none started after one ended abnormally),
--rounds rounds of the five forms alternating; the parent prints one JSON
line per layer and form with the median over rounds, the spread, and the
achieved fraction of HBM bandwidth: the layer's algorithmic bytes (input +
weights + output, float32) over the time, over 8.0 TB/s.

    python tools/bench_deconv.py [--rounds 3] [--iters 200] [--windows 5]
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

HBM_BYTES_PER_S = 8.0e12
# name: (C, M, k, s, p, H, W)
LAYERS = {"64to32_k4s2p1_72x128": (64, 32, 4, 2, 1, 72, 128), "32to16_k2s2_144x256": (32, 16, 2, 2, 0, 144, 256)}
BATCHES = (1, 8)
FORMS = ("tile", "tile_x1", "tile_x2", "direct", "stuffed")
KNOBS = {"tile_x1": ("VSO_DECONV_PAIR", "0"), "tile_x2": ("VSO_DECONV_PAIR", "1"), "direct": ("VSO_DECONV_TILE", "0")}


def layer_model(name, batch, stuffed):
    """(model bytes, input shape, algorithmic bytes) of a layer as one ConvTranspose, or in the zero-stuffed form."""
    import numpy as np
    import onnx_models as M
    c, m, k, s, p, h, w = LAYERS[name]
    b = M.Builder(5)
    taps = (-(-k // s)) ** 2
    wt = (b.rng.standard_normal((c, m, k, k)) * (c * taps) ** -0.5).astype(np.float32)
    bias = (b.rng.standard_normal(m) * 0.1).astype(np.float32)
    ho, wo = s * (h - 1) + k - 2 * p, s * (w - 1) + k - 2 * p
    if stuffed:
        up = b.op("Resize", ["x", "", b.const(np.array([1, 1, s, s], np.float32))], mode="nearest",
                  coordinate_transformation_mode="asymmetric", nearest_mode="floor")
        lattice = np.zeros((1, 1, s * h, s * w), np.float32)
        lattice[:, :, ::s, ::s] = 1.0
        z = b.op("Mul", [up, b.const(lattice)])
        wc = np.ascontiguousarray(wt[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        b.nodes.append(M.R.make_node("Conv", [z, b.const(wc), b.const(bias)], ["y"], kernel_shape=[k, k],
                                     pads=[k - 1 - p, k - 1 - p, k - p - s, k - p - s]))
    else:
        b.nodes.append(M.R.make_node("ConvTranspose", ["x", b.const(wt), b.const(bias)], ["y"], kernel_shape=[k, k],
                                     strides=[s, s], pads=[p] * 4))
    nbytes = 4 * (batch * c * h * w + c * m * k * k + m + batch * m * ho * wo)
    return b.model([("x", [batch, c, h, w])], [("y", [batch, m, ho, wo])]), (batch, c, h, w), nbytes


def child(args):
    """One form, every layer and batch: a JSON line each (ms per run: the median window)."""
    import numpy as np
    import torch
    import bench
    bench._load_pkg()
    import vss_amd.ort as ort
    form = args.child
    for name in LAYERS:
        for batch in BATCHES:
            model, shape, nbytes = layer_model(name, batch, form == "stuffed")
            with ort.InferenceSession(model, precision="f32") as s:
                launches = s.launches()
                want = {"tile": "k_deconv_tile<", "tile_x1": "k_deconv_tile<1>(", "tile_x2": "k_deconv_tile<2>(",
                        "direct": "k_deconv_direct(", "stuffed": "k_conv"}[form]
                assert any(want in n for n in launches), (form, launches)
                g = torch.Generator(device="cpu").manual_seed(1)
                x = torch.randn(shape, generator=g, dtype=torch.float32).cuda()
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
                print(json.dumps({"layer": name, "batch": batch, "form": form, "ms": statistics.median(windows),
                                  "launches": [n.split("(")[0].split("::")[-1] for n in launches], "bytes": nbytes,
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
    for _ in range(args.rounds):
        for form in FORMS:
            env = dict(os.environ)
            for knob, _ in KNOBS.values():
                env.pop(knob, None)
            if form in KNOBS:
                env[KNOBS[form][0]] = KNOBS[form][1]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--iters", str(args.iters),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:  # (nothing more is started on the GPU after an abnormal end)
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_deconv: the {form} child ended with {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    res.setdefault((r["layer"], r["batch"], r["form"]), []).append(r)
    for (layer, batch, form), rs in sorted(res.items()):
        ms = [r["ms"] for r in rs]
        med = statistics.median(ms)
        sums = {f: res[(layer, batch, f)][0]["checksum"] for f in FORMS if (layer, batch, f) in res}
        print(json.dumps({"layer": layer, "batch": batch, "form": form, "us_per_run": round(1e3 * med, 2),
                          "us_min": round(1e3 * min(ms), 2), "us_max": round(1e3 * max(ms), 2), "rounds": len(ms),
                          "launches": rs[0]["launches"], "algorithmic_MB": round(rs[0]["bytes"] / 1e6, 3),
                          "hbm_fraction": round(rs[0]["bytes"] / (med * 1e-3) / HBM_BYTES_PER_S, 4),
                          "sum_abs_rel_to_tile": round(rs[0]["checksum"] / sums["tile"], 7) if "tile" in sums else None}),
              flush=True)


if __name__ == "__main__":
    main()
