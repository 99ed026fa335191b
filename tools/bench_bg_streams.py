#!/usr/bin/env python3
"""Time the backgrounds over many streams against the per-stream composite.

8 streams x 1 frame, 640x480 RGBA frames and 144x256 alpha bytes resident in
HBM.  Five arms, their calls interleaved call by call in every round so that
drift hits all alike; per arm the HIP-event median over rounds * calls calls,
the per-round medians and their spread, and the same for the host time the
enqueue itself took:

  pooled_mixed    (a) one vss_background_composite_streams_device call, 8 streams:
                  2 colour, 2 sharing one image object with layers, 2 blur with
                  different radii, 2 with refinement
  single_8x1      (b) the same 8 frames as 8 vss_background_composite_device calls of
                  n = 1 on the same objects: the only way to do the same job
                  without the pooled call, and the yardstick
  pooled_colour   (c) one pooled call over 8 colour backgrounds
  single_colour   (d) one vss_background_composite_device call of n = 8 in colour
                  mode: against (c), the price of the pooled form
  pooled_shared   (e) one pooled call whose 8 frames name ONE colour object: the
                  launches of (c) with one event record, which splits (c) - (d)
                  into the descriptor form and the per-object bookkeeping

The claim (a) < (b) holds for a quantity when the gain 1 - a/b exceeds the larger
of the two arms' round-median spreads.  Prints one JSON line.

    python tools/bench_bg_streams.py [--rounds 5 --calls 8 --warmup 5]

Needs a GPU: there is no fall-back.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "video-stream-segmenetation_amd")


def load_pkg():
    spec = importlib.util.spec_from_file_location("vss_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vss_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8, help="timed calls per arm and round")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds * a.calls < 20:
        ap.error("at least 20 timed calls per arm (rounds * calls)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bg_streams: no GPU")
    pkg = load_pkg()
    import vss_amd.synthetic as syn
    n, fh, fw, fc, H, W = 8, 480, 640, 4, 144, 256
    frames = np.stack([syn.make_frame(500 + i, fh, fw, fc) for i in range(n)])
    rng = np.random.default_rng(7)
    with pkg.Session(model_h=H, model_w=W, dtype="bf16x2", max_batch=n, autotune=False) as s:
        with pkg.PostPool(s, n) as pool:
            alpha = pool.segment(list(range(n)), frames)[1].reshape(n, H, W)
        # a stream of its own: handle 0 (the null stream) would send the calls to the session's stream,
        # away from the events
        st = torch.cuda.Stream()
        stream = st.cuda_stream
        df = torch.from_numpy(frames).cuda()
        da = torch.from_numpy(alpha).cuda()
        do = torch.empty((n, fh, fw, 4), dtype=torch.uint8, device="cuda")
        rs, fs, P = fw * fc, fh * fw * fc, H * W

        def bg(mode, refine=None, layers=False, **kw):
            b = pkg.Background(s)
            if mode == "colour":
                b.set_color(*kw["color"])
            elif mode == "image":
                b.set_image(rng.integers(0, 256, (360, 480, 3), dtype=np.uint8))
            else:
                b.set_blur(*kw["blur"])
            if layers:
                b.set_layers([pkg.Layer("rect", 1, 100, 800, 700, 200, radius=40, color=(20, 40, 200, 200),
                                        shadow={"color": (0, 0, 0, 160), "blur": 24, "dx": 6, "dy": 8}),
                              pkg.Layer("image", 1, 1500, 60, 300, 160,
                                        pixels=rng.integers(0, 256, (64, 120, 4), dtype=np.uint8))])
            if refine:
                b.set_refine(*refine)
            return b

        plate = bg("image", layers=True)  # the company plate two participants share
        mixed = [bg("colour", color=(10, 200, 90)), bg("colour", color=(200, 10, 90)), plate, plate,
                 bg("blur", blur=(8, 4.0)), bg("blur", blur=(24, 10.0)),
                 bg("colour", color=(30, 30, 30), refine=(2, 16.0)), bg("image", refine=(4, 16.0))]
        colours = [bg("colour", color=(20 * i, 255 - 20 * i, 7 * i)) for i in range(n)]
        objects = list(dict.fromkeys(mixed + colours))

        def call(arm):
            if arm == "pooled_mixed":
                pkg.composite_streams_device(s, mixed, df.data_ptr(), n, fh, fw, fc, rs, fs, da.data_ptr(), do.data_ptr(),
                                             stream=stream)
            elif arm == "single_8x1":
                for t in range(n):
                    pkg.background_composite_device(s, mixed[t], df.data_ptr() + t * fs, 1, fh, fw, fc, rs, fs,
                                                    da.data_ptr() + t * P, do.data_ptr() + t * fh * fw * 4,
                                                    stream=stream)
            elif arm == "pooled_colour":
                pkg.composite_streams_device(s, colours, df.data_ptr(), n, fh, fw, fc, rs, fs, da.data_ptr(),
                                             do.data_ptr(), stream=stream)
            elif arm == "pooled_shared":
                pkg.composite_streams_device(s, colours[:1] * n, df.data_ptr(), n, fh, fw, fc, rs, fs, da.data_ptr(),
                                             do.data_ptr(), stream=stream)
            else:
                pkg.background_composite_device(s, colours[0], df.data_ptr(), n, fh, fw, fc, rs, fs, da.data_ptr(),
                                                do.data_ptr(), stream=stream)

        arms = ("pooled_mixed", "single_8x1", "pooled_colour", "single_colour", "pooled_shared")
        for m in arms:
            for _ in range(a.warmup):
                call(m)
        torch.cuda.synchronize()
        times = {m: [[] for _ in range(a.rounds)] for m in arms}
        host = {m: [[] for _ in range(a.rounds)] for m in arms}
        for r in range(a.rounds):
            pairs = []
            for _ in range(a.calls):
                for m in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    t0 = time.perf_counter()
                    call(m)
                    host[m][r].append((time.perf_counter() - t0) * 1e6)
                    e1.record(st)
                    pairs.append((m, e0, e1))
            torch.cuda.synchronize()
            for m, e0, e1 in pairs:
                times[m][r].append(e0.elapsed_time(e1) * 1e3)  # us
        # the two mixed arms write the same bytes
        outs = []
        for m in ("pooled_mixed", "single_8x1"):
            do.zero_()
            call(m)
            torch.cuda.synchronize()
            outs.append(do.clone())
        if not torch.equal(outs[0], outs[1]):
            raise SystemExit("bench_bg_streams: the pooled call and the 8 single calls wrote different bytes")
        result = {"bench": "bg_streams", "streams": n, "width": fw, "height": fh, "channels": fc, "mask_w": W,
                  "mask_h": H, "timed_calls_per_arm": a.rounds * a.calls}

        def summary(per_round):
            flat = [t for rr in per_round for t in rr]
            rounds = [statistics.median(rr) for rr in per_round]
            return {"median_us": round(statistics.median(flat), 2), "round_medians_us": [round(v, 2) for v in rounds],
                    "spread": round(max(rounds) / min(rounds) - 1, 4)}

        for m in arms:
            result[m] = {"device": summary(times[m]), "host_enqueue": summary(host[m])}
        for q in ("device", "host_enqueue"):
            pa, pb = result["pooled_mixed"][q], result["single_8x1"][q]
            gain, bar = 1 - pa["median_us"] / pb["median_us"], max(pa["spread"], pb["spread"])
            result[f"mixed_{q}_gain"] = round(gain, 4)
            result[f"mixed_{q}_gain_exceeds_spread"] = bool(gain > bar)
        result["pooled_colour_vs_single_colour_device"] = round(
            result["pooled_colour"]["device"]["median_us"] / result["single_colour"]["device"]["median_us"], 3)
        result["pooled_shared_vs_single_colour_device"] = round(
            result["pooled_shared"]["device"]["median_us"] / result["single_colour"]["device"]["median_us"], 3)
        for o in objects:
            o.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
