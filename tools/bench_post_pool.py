#!/usr/bin/env python3
"""Time the post chain over many streams against the per-stream chain.

8 streams x 1 frame, 640x480 RGB frames and 144x256 masks resident in HBM.
Three arms, their calls interleaved call by call in every round so that drift
hits all alike; per arm the HIP-event median over rounds * calls calls, the
per-round medians and their spread, and the host time the enqueue itself took:

  pooled      one vss_post_pool_process_device call, 8 stream ids
  chain_8x1   8 vss_postprocess_device calls of n = 1 on one vss_post_state: the
              only way to do the same job without a pool, and the yardstick
  chain_1x8   one vss_postprocess_device call of n = 8: the same pixels as a
              temporal batch of one stream, for scale

Prints one JSON line.

    python tools/bench_post_pool.py [--rounds 5 --calls 8 --warmup 5]

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
        raise SystemExit("bench_post_pool: no GPU")
    pkg = load_pkg()
    import vss_amd.synthetic as syn
    n, fh, fw, fc, H, W = 8, 480, 640, 3, 144, 256
    frames = np.stack([syn.make_frame(500 + i, fh, fw, fc) for i in range(n)])
    with pkg.Session(model_h=H, model_w=W, dtype="bf16x2", max_batch=n, autotune=False) as s:
        masks = s.segment_frames(frames)[0].reshape(n, H, W)
        # a stream of its own: handle 0 (the null stream) would send the calls to the session's stream,
        # away from the events
        st = torch.cuda.Stream()
        stream = st.cuda_stream
        df = torch.from_numpy(frames).cuda()
        dm = torch.from_numpy(masks).cuda()
        da = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        du = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        pool = pkg.PostPool(s, n)
        chain1, chain8 = pkg.PostChain(s), pkg.PostChain(s)
        ids = list(range(n))
        rs, fs, P = fw * fc, fh * fw * fc, H * W

        def call(arm):
            if arm == "pooled":
                pool.process_device(ids, df.data_ptr(), n, fh, fw, fc, rs, fs, dm.data_ptr(), da.data_ptr(),
                                    du.data_ptr(), stream)
            elif arm == "chain_8x1":
                for t in range(n):
                    chain1.process_device(df.data_ptr() + t * fs, 1, fh, fw, fc, rs, fs, dm.data_ptr() + t * P * 4,
                                          da.data_ptr() + t * P * 4, du.data_ptr() + t * P, stream)
            else:
                chain8.process_device(df.data_ptr(), n, fh, fw, fc, rs, fs, dm.data_ptr(), da.data_ptr(),
                                      du.data_ptr(), stream)

        arms = ("pooled", "chain_8x1", "chain_1x8")
        for m in arms:
            for _ in range(a.warmup):
                call(m)
        torch.cuda.synchronize()
        times = {m: [[] for _ in range(a.rounds)] for m in arms}
        host = {m: [] for m in arms}
        for r in range(a.rounds):
            pairs = []
            for _ in range(a.calls):
                for m in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    t0 = time.perf_counter()
                    call(m)
                    host[m].append((time.perf_counter() - t0) * 1e6)
                    e1.record(st)
                    pairs.append((m, e0, e1))
            torch.cuda.synchronize()
            for m, e0, e1 in pairs:
                times[m][r].append(e0.elapsed_time(e1) * 1e3)  # us
        # the same call on the same state gives the same bytes
        outs = []
        for _ in range(2):
            pool.reset()
            call("pooled")
            torch.cuda.synchronize()
            outs.append((da.clone(), du.clone()))
        if not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
            raise SystemExit("bench_post_pool: the output changed between two runs of the same call")
        result = {"bench": "post_pool", "streams": n, "width": fw, "height": fh, "mask_w": W, "mask_h": H,
                  "timed_calls_per_arm": a.rounds * a.calls}
        for m in arms:
            flat = [t for rr in times[m] for t in rr]
            rounds = [statistics.median(rr) for rr in times[m]]
            result[m] = {"median_us": round(statistics.median(flat), 2),
                         "round_medians_us": [round(v, 2) for v in rounds],
                         "spread": round(max(rounds) / min(rounds) - 1, 4),
                         "host_enqueue_median_us": round(statistics.median(host[m]), 2)}
        result["pooled_vs_chain_8x1"] = round(result["pooled"]["median_us"] / result["chain_8x1"]["median_us"], 3)
        result["pooled_vs_chain_1x8"] = round(result["pooled"]["median_us"] / result["chain_1x8"]["median_us"], 3)
        for o in (pool, chain1, chain8):
            o.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
