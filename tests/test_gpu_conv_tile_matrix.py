"""Every k_conv_tile / k_conv_tile_up form the planner can reach
(vso_conv.hip: conv_tile_shape), each against the float64 oracle with the
same operand rounding (oracle/onnx_ref.py, run(conv_operands=...)).

The models (onnx_models.conv_tile_matrix / conv_up_matrix) are small — odd
planes, batch 2 — and the planner's A/B knobs steer them onto the tiles that
production sizes use.  The knobs are read once per process, so each setting
but the default runs in one child process (tests/conv_matrix_child.py), all
its precisions one after another; the children run one at a time, and none is
started after one has ended abnormally.

Setting                                    forms (asserted by name: th, tw, bm)
default (this process)                     2x32 / 4x16 with the K split; the deep 5x5 on 4x32 (16-bit)
VSO_CONV_WANT=1                            f32 8x32 / 16x16; 16-bit 2x32 / 4x16; upsample 8x32 / 16x16
VSO_CONV_WANT=1 VSO_CONV_MAX_TH=0          16-bit 8x32 / 16x16
VSO_CONV_WANT=1 VSO_CONV_MAX_TH=4          4x32 in every precision, plain and upsample
  VSO_UP_MAX_TH=4
VSO_CONV_DEEP_TILE=2                       the deep 5x5 on 8x32 with the K split (16-bit)
VSO_CONV_WANT=1 VSO_UP_BM64=1              the 48-channel upsample cases on the 64-channel upsample tiles:
  [VSO_CONV_MAX_TH=0 | 4]                  2x32 / 4x16 [8x32 / 16x16 | 4x32]
VSO_CONV_GRID=8 (f32; default want, and    the persistent body, 8 workgroups: 6-85 items each, across
  VSO_CONV_WANT=1)                         split, tile, channel-tile and batch boundaries

With VSO_CONV_WANT=1 every launch has ksplit 1 (conv_tile_shape splits only
below want / 2 workgroups), each workgroup running all its chunks: 3 on the
72-channel cases, 17 on the deep one.  The launch names carry no ksplit; that
follows from the planner's rule.

Bars, those of tests/test_gpu_onnx.py: plain forms 1e-4 of the output scale
(max(1, max |oracle|)) in every precision, and per element 1e-4 * max(1,
|oracle|) — the op matrix's form; upsample forms 1e-3 of the output scale
(test_conv_upsample_fusion: an interpolated operand may land one 16-bit step
from the oracle's).  A second run of every session is bitwise the first.
Within a precision, ksplit-1 outputs are bitwise equal across tile shapes
(the same chunk and tap order per output pixel), and the outputs under
VSO_CONV_GRID=8 bitwise those without the cap.

Together the settings launch 148 of the 168 compiled instances; the other 20
(16-bit 5x5 on 64-channel tiles) no knob reaches.  Measured errors and two
deliberate breaks these tests catch and the earlier ones do not:
profiles/NOTES.md, "k_conv_tile form matrix".
"""
import re

import numpy as np
import pytest

import conv_matrix_child as C
import onnx_ref as R

pytestmark = pytest.mark.gpu

TOL, TOL_UP = 1e-4, 1e-3
PRECS = ("f32", "bf16", "f16")
PREC_ID = {"f32": 0, "bf16": 1, "f16": 2}

# case -> its convolutions (plane class, kernel, stride, output channels), in launch order
PLAIN = {"w3_16": [("wide", 3, 1, 16)], "w3_24": [("wide", 3, 1, 24)], "w3_70": [("wide", 3, 1, 70)],
         "w5_16": [("wide", 5, 1, 16)], "w5_32": [("wide", 5, 1, 32)], "w5_70": [("wide", 5, 1, 70)],
         "ws2_24": [("s2w", 3, 2, 24)], "wcat_24": [("wide", 3, 1, 24)], "n3_16": [("narrow", 3, 1, 16)],
         "n3_70": [("narrow", 3, 1, 70)], "n5_24": [("narrow", 5, 1, 24)], "ns2_48": [("s2n", 3, 2, 48)],
         "d5_48": [("deep", 5, 1, 48)], "k_48": [("narrow", 5, 1, 48), ("narrow", 3, 1, 48)],
         "n3_24": [("narrow", 3, 1, 24)], "n5_16": [("narrow", 5, 1, 16)], "ws2_16": [("s2w", 3, 2, 16)],
         "ws2_70": [("s2w", 3, 2, 70)], "xs2_16": [("s2n", 3, 2, 16)], "xs2_24": [("s2n", 3, 2, 24)]}
UP = {"ua_24": ("wide", 3, 24), "uc_16": ("narrow", 5, 16), "uw5_32": ("wide", 5, 32), "un3_16": ("narrow", 3, 16),
      "u48": ("wide", 3, 48), "uw3_16": ("wide", 3, 16), "un3_24": ("narrow", 3, 24), "un3_48": ("narrow", 3, 48),
      "uw5_16": ("wide", 5, 16), "un5_24": ("narrow", 5, 24)}
N_PLAIN_CONVS, N_UP_CONVS = sum(len(v) for v in PLAIN.values()), len(UP)
S2 = {"s2w": (2, 32), "s2n": (4, 16)}  # the stride-2 tiles: one candidate each

# setting -> (environment, sessions, tiles).  tiles: (th, tw) per plane class
# for f32 sessions, 16-bit sessions and the upsample forms.
SETTINGS = {
    "default": ({}, "plain:f32,bf16,f16;up:bf16,f16",
                {"f32": {"wide": (2, 32), "narrow": (4, 16), "deep": (2, 32)},
                 "b16": {"wide": (2, 32), "narrow": (4, 16), "deep": (4, 32)},
                 "up": {"wide": (2, 32), "narrow": (4, 16)}}),
    "want1": ({"VSO_CONV_WANT": "1"}, "plain:f32,bf16,f16;up:bf16,f16",
              {"f32": {"wide": (8, 32), "narrow": (16, 16), "deep": (8, 32)},
               "b16": {"wide": (2, 32), "narrow": (4, 16), "deep": (2, 32)},
               "up": {"wide": (8, 32), "narrow": (16, 16)}}),
    "want1_th0": ({"VSO_CONV_WANT": "1", "VSO_CONV_MAX_TH": "0"}, "plain:bf16,f16;up:bf16,f16",
                  {"b16": {"wide": (8, 32), "narrow": (16, 16), "deep": (8, 32)},
                   "up": {"wide": (8, 32), "narrow": (16, 16)}}),
    "want1_th4": ({"VSO_CONV_WANT": "1", "VSO_CONV_MAX_TH": "4", "VSO_UP_MAX_TH": "4"},
                  "plain:f32,bf16,f16;up:bf16,f16",
                  {"f32": {"wide": (4, 32), "narrow": (4, 16), "deep": (4, 32)},
                   "b16": {"wide": (4, 32), "narrow": (4, 16), "deep": (4, 32)},
                   "up": {"wide": (4, 32), "narrow": (4, 16)}}),
    "deep2": ({"VSO_CONV_DEEP_TILE": "2"}, "plain:bf16,f16",
              {"b16": {"wide": (2, 32), "narrow": (4, 16), "deep": (8, 32)}}),
    "want1_bm64": ({"VSO_CONV_WANT": "1", "VSO_UP_BM64": "1"}, "up:bf16,f16",
                   {"up": {"wide": (8, 32), "narrow": (16, 16), "wide64": (2, 32), "narrow64": (4, 16)}}),
    "want1_bm64_th0": ({"VSO_CONV_WANT": "1", "VSO_UP_BM64": "1", "VSO_CONV_MAX_TH": "0"}, "up:bf16,f16",
                       {"up": {"wide": (8, 32), "narrow": (16, 16), "wide64": (8, 32), "narrow64": (16, 16)}}),
    "want1_bm64_th4": ({"VSO_CONV_WANT": "1", "VSO_UP_BM64": "1", "VSO_CONV_MAX_TH": "4"}, "up:bf16,f16",
                       {"up": {"wide": (8, 32), "narrow": (16, 16), "wide64": (4, 32), "narrow64": (4, 16)}}),
    "grid8": ({"VSO_CONV_GRID": "8"}, "plain:f32",
              {"f32": {"wide": (2, 32), "narrow": (4, 16), "deep": (2, 32)}}),
    "want1_grid8": ({"VSO_CONV_WANT": "1", "VSO_CONV_GRID": "8"}, "plain:f32",
                    {"f32": {"wide": (8, 32), "narrow": (16, 16), "deep": (8, 32)}}),
}
SESSIONS = [(st, model, prec) for st, (_, spec, _) in SETTINGS.items() for model, precs in C.parse_spec(spec)
            for prec in precs]


def _bm(m, ks, prec):
    """The output-channel tile (conv_tile_shape): 16 up to 16 channels, 32 up
    to 32 and for every 16-bit 5x5, else 64."""
    return 16 if m <= 16 else 32 if m <= 32 or (ks == 5 and prec != "f32") else 64


def expected_launches(setting, model, prec):
    """The k_conv_tile / k_conv_tile_up launches of one session, in order."""
    tiles = SETTINGS[setting][2]
    plain = tiles.get("f32" if prec == "f32" else "b16")
    p = PREC_ID[prec]
    names = []
    if model == "plain":
        for convs in PLAIN.values():
            for cls, ks, s, m in convs:
                th, tw = S2[cls] if cls in S2 else plain[cls]
                names.append(f"k_conv_tile<{p}, {ks}, {s}, {th}, {tw}, {_bm(m, ks, prec)}>")
    else:
        for case, (cls, ks, m) in UP.items():
            bm = _bm(m, ks, prec)
            if bm <= 32:
                th, tw = tiles["up"][cls]
                names.append(f"k_conv_tile_up<{p}, {ks}, 1, {th}, {tw}, {bm}>")
            elif "wide64" in tiles["up"]:  # VSO_UP_BM64=1: the 64-channel upsample tile, capped like the plain 16-bit ones
                th, tw = tiles["up"][cls + "64"]
                names.append(f"k_conv_tile_up<{p}, {ks}, 1, {th}, {tw}, {bm}>")
            else:                          # not fused: its Resize keeps a launch
                th, tw = plain[cls]
                names.append(f"k_conv_tile<{p}, {ks}, 1, {th}, {tw}, {bm}>")
    return names


@pytest.fixture(scope="module")
def ort(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vss_amd.ort as o
    return o


@pytest.fixture(scope="module")
def oracle():
    """{"<model>/<precision>/<case>": the oracle's output}, computed once."""
    want = {}
    for model, (build, _, cases, _) in C.MODELS.items():
        m = R.load(build())
        f = C.feeds(model)
        for prec in PRECS if model == "plain" else PRECS[1:]:
            got = R.run(m, f, conv_operands=None if prec == "f32" else prec)
            for case, (name, _, _) in zip(cases, m.outputs):
                want[f"{model}/{prec}/{case}"] = got[name]
    return want


_RESULTS = {}  # setting -> (outputs, info) or the AssertionError its run ended with


def _setting(ort, setting):
    if setting not in _RESULTS:
        env, spec, _ = SETTINGS[setting]
        try:
            _RESULTS[setting] = C.run_sessions(ort, spec) if setting == "default" else C.run_child(setting, env, spec)
        except AssertionError as e:
            _RESULTS[setting] = e
    if isinstance(_RESULTS[setting], AssertionError):
        raise _RESULTS[setting]
    return _RESULTS[setting]


@pytest.mark.parametrize("setting,model,prec", SESSIONS, ids=["-".join(s) for s in SESSIONS])
def test_forms_against_oracle(ort, oracle, setting, model, prec):
    """One session: the forms it launched (by name, in order), every
    convolution tiled, the Concat's last input read in place, a second run
    bitwise the first, and every output within the bar of the oracle."""
    outs, info = _setting(ort, setting)
    inf = info[f"{model}/{prec}"]
    names = inf["launches"]
    tiled = [re.search(r"k_conv_tile(_up)?<[^>]*>", n).group(0) for n in names if "k_conv_tile" in n]
    print(setting, model, prec, [n.split("(")[0] for n in names])
    assert tiled == expected_launches(setting, model, prec), names
    if model == "plain":
        assert inf["tile_convs"] == N_PLAIN_CONVS
        # Concat(a, b): a's copy only — b (13 channels at offset 32) is read by the convolution itself
        assert sum("k_copy" in n for n in names) == 1, names
    else:
        assert inf["tile_convs"] == N_UP_CONVS
        fused = sum("k_conv_tile_up<" in n for n in tiled)
        assert sum("k_resize" in n for n in names) == N_UP_CONVS - fused, names
    assert inf["rerun_equal"]
    tol = TOL if model == "plain" else TOL_UP
    worst = []
    for case in (PLAIN if model == "plain" else UP):
        key = f"{model}/{prec}/{case}"
        g, w = outs[key].astype(np.float64), oracle[key].astype(np.float64)
        assert g.shape == w.shape, (key, g.shape, w.shape)
        d = np.abs(g - w)
        scale = max(1.0, float(np.abs(w).max()))
        rel = float((d / np.maximum(1.0, np.abs(w))).max())
        print(f"{setting} {key}: max abs err {float(d.max()):.3e} (scale {scale:.2f}), per element {rel:.3e}")
        if not (d.max() <= tol * scale and (model != "plain" or rel <= tol)):
            worst.append((case, float(d.max()), scale, rel))
    assert not worst, (setting, model, prec, worst)


def _same(a, b, keys):
    bad = [(k, float(np.abs(a[k] - b[k]).max())) for k in keys if not np.array_equal(a[k], b[k])]
    assert not bad, bad


@pytest.mark.parametrize("prec", PRECS)
def test_ksplit1_bitwise_across_tile_shapes(ort, prec):
    """With VSO_CONV_WANT=1 no launch splits K, and an output pixel's sum runs
    over the chunks and taps in the same order on every tile: the plain forms
    on 8x32 / 16x16 (f32; 16-bit with no height cap), 4x32 / 4x16 (a cap of 4)
    and 2x32 / 4x16 (16-bit, the default cap), and the upsample forms on 8x32
    / 16x16 and 4x32 / 4x16, are bitwise equal within a precision."""
    base, _ = _setting(ort, "want1")
    others = ["want1_th4"] + ([] if prec == "f32" else ["want1_th0"])
    models = ("plain",) if prec == "f32" else ("plain", "up")
    keys = [k for k in base if k.split("/")[0] in models and k.split("/")[1] == prec]
    assert keys
    for other in others:
        o, _ = _setting(ort, other)
        _same(base, o, keys)
    if prec != "f32":  # the 64-channel upsample tiles: 2x32 / 4x16, 8x32 / 16x16, 4x32
        base, _ = _setting(ort, "want1_bm64")
        keys = [k for k in base if k.split("/")[1] == prec]
        assert keys
        for other in ("want1_bm64_th0", "want1_bm64_th4"):
            o, _ = _setting(ort, other)
            _same(base, o, keys)


@pytest.mark.parametrize("capped,plain", [("grid8", "default"), ("want1_grid8", "want1")])
def test_persistent_items_per_workgroup_bitwise(ort, capped, plain):
    """The persistent f32 body on 8 workgroups (VSO_CONV_GRID=8): each runs
    items blockIdx.x, + 8, ... — 43 to 85 of the wide cases' 342 / 684 at the
    default want (K split on: consecutive items of a workgroup differ in
    split, tile, channel tile and batch), 4 to 8 three-chunk items on 8x32
    tiles at VSO_CONV_WANT=1 — against one or two items per workgroup without
    the cap: the same arithmetic per item, so bitwise equal outputs (the
    Concat-tail case among them)."""
    a, ia = _setting(ort, capped)
    b, _ = _setting(ort, plain)
    assert ia["plain/f32"]["rerun_equal"]
    keys = [k for k in a if k.startswith("plain/f32/")]
    assert len(keys) == len(PLAIN) and "plain/f32/wcat_24" in keys
    _same(a, b, keys)
