#!/usr/bin/env python3
"""Time the virtual-background kernels against the parent's k_composite.

For 8 x 640x480 and 8 x 1080p RGB frames resident in HBM: the HIP-event median
per call of vss_composite_device (the yardstick) and of
vss_background_composite_device in colour, image and blur mode, the calls of
the four interleaved round by round so that drift hits all alike; the spread
of the yardstick's per-round medians; each mode's algorithmic bytes and the
share of 8 TB/s they imply at the measured time.  Prints one JSON line.

    python tools/bench_background.py [--radius 7 --sigma 2.5 --rounds 5 --calls 8] [--refine R,EPS]

--refine R,EPS (opt-in; without it the output is what it always was) adds, in
the same interleaved rounds: the three modes with the edge-aware matte on
(colour_refined, image_refined, blur_refined; each with its ratio to its own
unrefined mode), and the frame-size alpha plane alone with refinement off and
on (alpha_plain, alpha_refined).  The mask-resolution stage has no entry point
of its own: matte_stage_us is alpha_refined - alpha_plain, an upper estimate
(the refined alpha kernel also reads the frame, which the plain one does not).

--nv12 (opt-in) adds a leg for the NV12 video I/O, 8 x 1080p resident in HBM, in
interleaved rounds of its own: the two conversion kernels alone (nv12_unpack,
nv12_pack: median, algorithmic bytes, achieved GB/s), k_bg_composite<COLOR> over
the same RGBA frames (colour_rgba: the yardstick of a streaming kernel in this
run), vss_video_process_device in colour mode (video_process), and the same
frames, already RGBA, through vss_segment_device + vss_postprocess_device +
vss_background_composite_device as before NV12 existed (rgba_path).
nv12_overhead_us is video_process - rgba_path: both conversions and the RGBA
round trip through the scratch.

--layers (opt-in) adds, in the same interleaved rounds, the three modes under
the branding layers of the reference's `corporate__rect` template
(tests/golden/branding_templates.json) at privacy level 3, every text line and
image a stub sprite (colour_layers, image_layers, blur_layers): colour and image
run k_bg_composite<IMAGE> over the baked plate, so they are compared with
`image`; blur reads the overlay plate, 4 more bytes per pixel, and is compared
with `blur`.  plate_build_us is the one-off cost, for information: the median
of vss_background_overlay_device right after a privacy change (the whole plate
rebuilt, plus one device copy of it).

Needs a GPU: there is no fall-back.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "video-stream-segmenetation_amd")
HBM_BYTES_PER_S = 8e12


def load_pkg():
    spec = importlib.util.spec_from_file_location("vss_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vss_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def algorithmic_bytes(mode, n, fh, fw, fc, H, W):
    """Bytes each mode must move per call: every input read once, every output written once."""
    px = n * fh * fw
    alpha = n * H * W
    base = px * (fc + 4) + alpha           # frame in, RGBA out, mask alpha
    if mode in ("composite", "colour"):
        return base
    if mode == "image":
        return base + px * 3               # the cached scaled image, RGB
    return base + px * (fc + 4) + px * 4   # blur: the horizontal pass (frame in, RGBX out), RGBX back in


def refined_extra_bytes(n, fh, fw, fc, H, W):
    """What refinement adds: the guide pass reads the frame once more; per mask pixel L out and in,
    p in, (a_q, b_q) out and in, (abar, bbar) out and in, in place of nothing (the alpha bytes stay)."""
    return n * fh * fw * fc + n * H * W * (1 + 1 + 1 + 8 + 8 + 8 + 8)


def template_stub_layers(pkg):
    """The corporate__rect template with stub sprites: a translucent block per text line, opaque icons."""
    with open(os.path.join(ROOT, "tests", "golden", "branding_templates.json"), encoding="utf-8") as f:
        template = json.load(f)["templates"]["corporate__rect"]
    fields = {"full_name": "Name Surname", "position": "Senior engineer", "department": "Department",
              "company": "Company", "office_location": "City, street 1", "email": "name@example.com",
              "telegram": "@name", "slogan": "A slogan of some length"}
    rng = np.random.default_rng(7)

    def rasterize(text, font, color):
        size = int(font.replace("bold ", "").split("px")[0])
        px = np.zeros((size, max(1, size * len(text) // 2), 4), np.uint8)
        px[..., :3] = color[:3]
        px[..., 3] = rng.integers(0, 256, px.shape[:2], dtype=np.uint8)
        return px, int(size * 0.8)

    images = {k: rng.integers(0, 256, (128, 128, 4), dtype=np.uint8)
              for k in ("email_icon", "telegram_icon", "qr_code", "company_logo")}
    return pkg.template_layers(template, fields, images, rasterize)


def nv12_leg(pkg, torch, s, a, n, H, W):
    """The --nv12 leg (see the module docstring) -> its result dict."""
    fh, fw = 1080, 1920
    rng = np.random.default_rng(1)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    dy = torch.from_numpy(rng.integers(0, 256, (n, fh, fw), dtype=np.uint8)).cuda()
    duv = torch.from_numpy(rng.integers(0, 256, (n, fh // 2, fw), dtype=np.uint8)).cuda()
    oy, ouv = torch.empty_like(dy), torch.empty_like(duv)
    drgba = torch.empty((n, fh, fw, 4), dtype=torch.uint8, device="cuda")
    dout = torch.empty_like(drgba)
    masks = torch.empty((n, H * W), dtype=torch.float32, device="cuda")
    alpha = torch.empty((n, H * W), dtype=torch.uint8, device="cuda")
    bg, bg2 = pkg.Background(s), pkg.Background(s)   # colour mode, one per path
    chain, chain2 = pkg.PostChain(s), pkg.PostChain(s)
    video = pkg.Video(s, "bt709")
    ygeo = (dy.data_ptr(), fw, fw * fh, duv.data_ptr(), fw, fw * fh // 2)
    ogeo = (oy.data_ptr(), fw, fw * fh, ouv.data_ptr(), fw, fw * fh // 2)
    rgeo = (n, fh, fw, 4, fw * 4, fh * fw * 4)

    def call(mode):
        if mode == "nv12_unpack":
            pkg.nv12_to_rgba_device(s, "bt709", *ygeo, n, fh, fw, drgba.data_ptr(), stream=stream)
        elif mode == "nv12_pack":
            pkg.rgba_to_nv12_device(s, "bt709", drgba.data_ptr(), 0, 0, n, fh, fw, *ogeo, stream=stream)
        elif mode == "colour_rgba":
            pkg.background_composite_device(s, bg2, drgba.data_ptr(), *rgeo, alpha.data_ptr(), dout.data_ptr(),
                                            stream=stream)
        elif mode == "video_process":
            video.process_device(chain, bg, *ygeo, n, fh, fw, *ogeo, stream=stream)
        else:  # rgba_path
            s.segment_device(drgba.data_ptr(), *rgeo, masks.data_ptr(), stream)
            chain2.process_device(drgba.data_ptr(), *rgeo, masks.data_ptr(), 0, alpha.data_ptr(), stream)
            pkg.background_composite_device(s, bg2, drgba.data_ptr(), *rgeo, alpha.data_ptr(), dout.data_ptr(),
                                            stream=stream)

    # each entry reads what an earlier one wrote
    modes = ("nv12_unpack", "rgba_path", "colour_rgba", "nv12_pack", "video_process")
    for m in modes:
        for _ in range(a.warmup):
            call(m)
    torch.cuda.synchronize()
    times = {m: [[] for _ in range(a.rounds)] for m in modes}
    for r in range(a.rounds):
        pairs = []
        for _ in range(a.calls):
            for m in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call(m)
                e1.record(st)
                pairs.append((m, e0, e1))
        torch.cuda.synchronize()
        for m, e0, e1 in pairs:
            times[m][r].append(e0.elapsed_time(e1) * 1e3)  # us
    px = n * fh * fw
    conv_bytes = px + px // 2 + px * 4
    out = {"width": fw, "height": fh, "n": n}
    for m in modes:
        flat = [t for rr in times[m] for t in rr]
        med = statistics.median(flat)
        rounds = [statistics.median(rr) for rr in times[m]]
        out[m] = {"median_us": round(med, 2), "round_medians_us": [round(v, 2) for v in rounds],
                  "spread": round(max(rounds) / min(rounds) - 1, 4)}
        by = {"nv12_unpack": conv_bytes, "nv12_pack": conv_bytes,
              "colour_rgba": algorithmic_bytes("colour", n, fh, fw, 4, H, W)}.get(m)
        if by:
            out[m].update({"bytes": by, "gb_per_s": round(by / (med * 1e-6) / 1e9, 1),
                           "hbm_fraction": round(by / (med * 1e-6) / HBM_BYTES_PER_S, 4)})
    out["nv12_overhead_us"] = round(out["video_process"]["median_us"] - out["rgba_path"]["median_us"], 2)
    # the conversions are deterministic: pack(unpack(in)) twice gives the same planes
    call("nv12_unpack")
    call("nv12_pack")
    torch.cuda.synchronize()
    ref_planes = (oy.clone(), ouv.clone())
    call("nv12_unpack")
    call("nv12_pack")
    torch.cuda.synchronize()
    if not (torch.equal(ref_planes[0], oy) and torch.equal(ref_planes[1], ouv)):
        raise SystemExit("bench_background: the NV12 output changed between two runs of the same call")
    for o in (video, chain, chain2, bg, bg2):
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--sigma", type=float, default=2.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8, help="timed calls per mode and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--refine", default=None, metavar="R,EPS", help="also time the edge-aware matte (opt-in)")
    ap.add_argument("--layers", action="store_true", help="also time the modes under branding layers (opt-in)")
    ap.add_argument("--nv12", action="store_true", help="also time the NV12 video I/O at 8 x 1080p (opt-in)")
    a = ap.parse_args()
    if a.rounds * a.calls < 20:
        ap.error("at least 20 timed calls per mode (rounds * calls)")
    refine = None
    if a.refine:
        try:
            refine = (int(a.refine.split(",")[0]), float(a.refine.split(",")[1]))
        except (ValueError, IndexError):
            ap.error("--refine takes R,EPS, e.g. 4,16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_background: no GPU")
    pkg = load_pkg()
    n, fc, H, W = 8, 3, 144, 256
    rng = np.random.default_rng(0)
    result = {"bench": "background", "n": n, "radius": a.radius, "sigma": a.sigma,
              "timed_calls_per_mode": a.rounds * a.calls, "sizes": {}}
    if refine:
        result["refine"] = {"radius": refine[0], "eps": refine[1]}
    with pkg.Session(model_h=H, model_w=W, dtype="bf16x2", max_batch=n, autotune=False) as s:
        # a stream of its own: handle 0 (the null stream) would send the calls to the session's stream,
        # away from the events
        st = torch.cuda.Stream()
        stream = st.cuda_stream
        for fh, fw in ((480, 640), (1080, 1920)):
            df = torch.from_numpy(rng.integers(0, 256, (n, fh, fw, fc), dtype=np.uint8)).cuda()
            da = torch.from_numpy(rng.integers(0, 256, (n, H, W), dtype=np.uint8)).cuda()
            do = torch.empty((n, fh, fw, 4), dtype=torch.uint8, device="cuda")
            bgs = {m: pkg.Background(s) for m in ("colour", "image", "blur")}
            bgs["image"].set_image(rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8))
            bgs["blur"].set_blur(a.radius, a.sigma)
            geo = (n, fh, fw, fc, fw * fc, fh * fw * fc)
            if refine:
                for m in ("colour", "image", "blur"):
                    bgs[m + "_refined"] = pkg.Background(s)
                bgs["image_refined"].set_image(rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8))
                bgs["blur_refined"].set_blur(a.radius, a.sigma)
                bgs["alpha_plain"], bgs["alpha_refined"] = pkg.Background(s), pkg.Background(s)
                for m in ("colour_refined", "image_refined", "blur_refined", "alpha_refined"):
                    bgs[m].set_refine(*refine)
                dal = torch.empty((n, fh, fw), dtype=torch.uint8, device="cuda")
            if a.layers:
                for m in ("colour", "image", "blur"):
                    bgs[m + "_layers"] = pkg.Background(s)
                bgs["image_layers"].set_image(rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8))
                bgs["blur_layers"].set_blur(a.radius, a.sigma)
                stub = template_stub_layers(pkg)
                for m in ("colour_layers", "image_layers", "blur_layers"):
                    bgs[m].set_layers(stub)
                    bgs[m].set_privacy("high")

            def call(mode):
                if mode == "composite":
                    pkg.composite_device(s, df.data_ptr(), *geo, da.data_ptr(), do.data_ptr(), stream=stream)
                elif mode.startswith("alpha_"):
                    pkg.background_alpha_device(s, bgs[mode], df.data_ptr(), *geo, da.data_ptr(), dal.data_ptr(),
                                                stream=stream)
                else:
                    pkg.background_composite_device(s, bgs[mode], df.data_ptr(), *geo, da.data_ptr(), do.data_ptr(),
                                                    stream=stream)

            modes = ("composite", "colour", "image", "blur")
            if refine:  # the default modes stay first and warm up last-but-these, so `check` below is still blur's
                modes = ("colour_refined", "image_refined", "blur_refined", "alpha_plain", "alpha_refined") + modes
            if a.layers:
                modes = ("colour_layers", "image_layers", "blur_layers") + modes
            for m in modes:
                for _ in range(a.warmup):
                    call(m)
            torch.cuda.synchronize()
            check = do.clone()  # blur ran last in the warm-up
            times = {m: [[] for _ in range(a.rounds)] for m in modes}
            for r in range(a.rounds):
                pairs = []
                for _ in range(a.calls):
                    for m in modes:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        call(m)
                        e1.record(st)
                        pairs.append((m, e0, e1))
                torch.cuda.synchronize()
                for m, e0, e1 in pairs:
                    times[m][r].append(e0.elapsed_time(e1) * 1e3)  # us
            call("blur")
            torch.cuda.synchronize()
            if not torch.equal(check, do):
                raise SystemExit("bench_background: the output changed between two runs of the same call")
            out = {}
            for m in modes:
                flat = [t for rr in times[m] for t in rr]
                med = statistics.median(flat)
                if m.startswith("alpha_"):
                    by = n * fh * fw + n * H * W + (n * fh * fw * fc if m == "alpha_refined" else 0)
                else:
                    by = algorithmic_bytes({"colour_layers": "image"}.get(m, m.replace("_refined", "").replace(
                        "_layers", "")), n, fh, fw, fc, H, W)
                if m == "blur_layers":
                    by += n * fh * fw * 4  # the overlay plate, read per frame (L2 may serve the batch's repeats)
                if m.endswith("_refined"):
                    by += refined_extra_bytes(n, fh, fw, fc, H, W)
                rounds = [statistics.median(rr) for rr in times[m]]
                out[m] = {"median_us": round(med, 2), "round_medians_us": [round(v, 2) for v in rounds],
                          "bytes": by, "bytes_per_px": round(by / (n * fh * fw), 3),
                          "hbm_fraction": round(by / (med * 1e-6) / HBM_BYTES_PER_S, 4)}
            base = out["composite"]
            base["spread"] = round(max(base["round_medians_us"]) / min(base["round_medians_us"]) - 1, 4)
            for m in ("colour", "image", "blur"):
                out[m]["ratio_to_composite"] = round(out[m]["median_us"] / base["median_us"], 3)
                if refine:
                    rm = out[m + "_refined"]
                    rm["ratio_to_unrefined"] = round(rm["median_us"] / out[m]["median_us"], 3)
                    rm["bytes_ratio_to_unrefined"] = round(rm["bytes"] / out[m]["bytes"], 3)
                    rm["spread"] = round(max(rm["round_medians_us"]) / min(rm["round_medians_us"]) - 1, 4)
            if a.layers:
                for m, ref_mode in (("colour_layers", "image"), ("image_layers", "image"), ("blur_layers", "blur")):
                    lm = out[m]
                    lm["ratio_to_" + ref_mode] = round(lm["median_us"] / out[ref_mode]["median_us"], 3)
                    lm["bytes_ratio_to_" + ref_mode] = round(lm["bytes"] / out[ref_mode]["bytes"], 3)
                    lm["spread"] = round(max(lm["round_medians_us"]) / min(lm["round_medians_us"]) - 1, 4)
                for m in ("image", "blur"):
                    out[m]["spread"] = round(max(out[m]["round_medians_us"]) / min(out[m]["round_medians_us"]) - 1, 4)
                plate = torch.empty((fh, fw, 4), dtype=torch.uint8, device="cuda")
                builds = []
                for k in range(7):
                    bgs["blur_layers"].set_privacy(1 + k % 2)
                    bgs["blur_layers"].set_privacy(3)  # the level changed: the next call rebuilds the plate
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    pkg._check(pkg.lib().vss_background_overlay_device(s._h, bgs["blur_layers"]._bg, fh, fw,
                                                                       plate.data_ptr(), fw * 4, stream), s._h)
                    e1.record(st)
                    torch.cuda.synchronize()
                    builds.append(e0.elapsed_time(e1) * 1e3)
                out["plate_build_us"] = round(statistics.median(builds[2:]), 2)
                out["layers"] = len(stub)
            if refine:
                out["matte_stage_us"] = round(out["alpha_refined"]["median_us"] - out["alpha_plain"]["median_us"], 2)
            result["sizes"][f"{fw}x{fh}"] = out
            for b in bgs.values():
                b.close()
        if a.nv12:
            result["nv12"] = nv12_leg(pkg, torch, s, a, n, H, W)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
