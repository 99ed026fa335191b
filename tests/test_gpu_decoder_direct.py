"""The decoders' even tiles upsample their low-res src from registers — every
2 x 2 output quad's four source taps loaded straight from global memory —
instead of from a region staged in LDS: the same operations in the same order,
so d1..d3 and the masks are bitwise what the commit before that change
produced, recorded on the GPU from a build of it (tests/golden/
decoder_parent.npz and decoder_parent_xor.npz, made by
tests/golden/make_decoder_golden.py).

Model 80 x 112, 3 frames of 100 x 140 RGB, autotune off: d1 is 10 x 14 pixels,
d2 20 x 28 and d3 40 x 56, so the batch is odd and the pinned tiles below are
partial at the bottom and at the right (4 x 8 in d1, 6 rows in d2, 6 x 16 in
d3): the taps' clamps to the source's last row / column and the zeroing past
the image's edge both run.  Odd-sided tiles keep the path through LDS; they
are held to the same fixture, i.e. bitwise to the even ones.  (d3's shape
compiles no odd-sided tile — its pixel blocks split over two wave groups — so
the odd cases pin d1 and d2.)
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_decoder_golden as gold  # noqa: E402  (the fixture's config and its decoding)

pytestmark = pytest.mark.gpu

# name -> (VSS_TILE spec, {layer: (TH, TW)} it pins)
TILES = {
    "planner": ("", {}),
    "bench_tiles": ("8:4x8,9:4x8,10:6x16", {8: (4, 8), 9: (4, 8), 10: (6, 16)}),
    "d2_6x8": ("9:6x8", {9: (6, 8)}),
    "d3_4x16_d1_2x8": ("8:2x8,10:4x16", {8: (2, 8), 10: (4, 16)}),
    "d3_8x8_d2_6x16": ("9:6x16,10:8x8", {9: (6, 16), 10: (8, 8)}),
    "odd_d1_3x16_d2_3x16": ("8:3x16,9:3x16", {8: (3, 16), 9: (3, 16)}),
    "odd_d1_1x16_d2_1x16": ("8:1x16,9:1x16", {8: (1, 16), 9: (1, 16)}),
}
CASES = [(name, dt, ks) for name in TILES for dt, ks in gold.CONFIGS
         if name in ("planner", "bench_tiles", "odd_d1_3x16_d2_3x16") or (dt, ks) == ("bf16x2", False)]


@pytest.fixture(scope="module")
def golden():
    g = gold.load(os.path.join(HERE, "golden", "decoder_parent.npz"))  # and decoder_parent_xor.npz
    assert len(str(g["commit"])) == 40  # the recorded commit's hash
    assert tuple(g["model_hw"]) == gold.MODEL_HW and tuple(g["frame_hw"]) == gold.FRAME_HW
    assert tuple(g["seeds"]) == gold.SEEDS
    return g


@pytest.fixture(scope="module")
def want(golden):
    """Every recorded array's bits, decoded once."""
    return {gold.prefix(dt, ks) + "_" + k: gold.decode(golden, gold.prefix(dt, ks) + "_" + k).view(np.uint32)
            for dt, ks in gold.CONFIGS for k in [f"L{li}" for li in gold.LAYERS] + ["masks"]}


@pytest.mark.parametrize("name,dtype,ksplit", CASES, ids=[f"{n}-{gold.prefix(d, k)}" for n, d, k in CASES])
def test_decoders_bitwise_parent(pkg, synthetic, want, name, dtype, ksplit):
    spec, pinned = TILES[name]

    def check(s):
        # the pinned tiles are the ones that run: the layer's LDS is block_lds() of that tile
        for li, (th, tw) in pinned.items():
            cin, cskip, cout = gold.SHAPES[li]
            assert s.layer_occupancy(li)[1] == pkg.block_lds_bytes(2, 1, th, tw, cin, cskip, cin + cskip, cout), li

    got = gold.record(pkg, gold.frames(synthetic), dtype, ksplit, spec, check)
    assert len(got) == len(gold.LAYERS) + 1
    bad = [k for k, v in got.items() if v.shape != want[k].shape
           or not np.array_equal(np.ascontiguousarray(v).view(np.uint32), want[k])]
    assert not bad, bad
