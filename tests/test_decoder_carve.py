"""The decoders' LDS carve (block_lds() in csrc/vss_kernels.h, through the
library's vss_block_lds_bytes; no GPU needed).  Even-sided tiles upsample their
src from registers and have no low-res region: their work region is the 1024-
float statistics scratch.  Odd-sided tiles keep the region and the tap records,
i.e. the totals they had before.  tools/lds_sites.py restates the carve.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_sites  # noqa: E402

SHAPES = {"d1": (64, 48, 48), "d2": (48, 32, 32), "d3": (32, 16, 16)}  # (cin, cskip, cout), model/spec.json
# (layer, TH, TW) -> bytes.  Even tiles: the region's r4(SR * SC * cin) floats
# gone from max(1024, region) — d3 6 x 16: 44,736 - 4 (2112 - 1024) = 40,384,
# d2 4 x 8: 37,568 - 4 (1680 - 1024) = 34,944, d1 4 x 8: 55,360 - 4 (2240 - 1024)
# = 50,496 (the bench's tiles), and further compiled even tiles alike.
EVEN = {("d3", 6, 16): 40384, ("d2", 4, 8): 34944, ("d1", 4, 8): 50496,
        ("d2", 6, 8): 44288 - 4 * (6 * 7 * 48 - 1024), ("d3", 4, 16): 36160 - 4 * (5 * 11 * 32 - 1024),
        ("d1", 2, 8): 46144 - 4 * (4 * 7 * 64 - 1024), ("d3", 2, 8): 18112}  # (d3 2 x 8: the region was < 1024 floats)
# Odd tiles: what block_lds() gave before the even tiles lost their region.
ODD = {("d1", 3, 16): 78400, ("d1", 1, 16): 59712, ("d2", 3, 16): 55232, ("d2", 1, 16): 41344,
       ("d3", 3, 16): 34112, ("d3", 1, 16): 25024}


def _args(layer, th, tw):
    cin, cskip, cout = SHAPES[layer]
    return 2, 1, th, tw, cin, cskip, cin + cskip, cout


@pytest.mark.parametrize("key", list(EVEN), ids=lambda k: "%s_%dx%d" % k)
def test_even_tiles_have_no_src_region(pkg, key):
    assert pkg.block_lds_bytes(*_args(*key)) == EVEN[key]


@pytest.mark.parametrize("key", list(ODD), ids=lambda k: "%s_%dx%d" % k)
def test_odd_tiles_keep_their_carve(pkg, key):
    assert pkg.block_lds_bytes(*_args(*key)) == ODD[key]


@pytest.mark.parametrize("key", list(EVEN) + list(ODD), ids=lambda k: "%s_%dx%d" % k)
def test_lds_sites_restates_the_carve(pkg, key):
    assert lds_sites.Lds(*_args(*key), swz=True).total * 4 == pkg.block_lds_bytes(*_args(*key))


def test_residency_steps(pkg):
    """What the carve buys: LDS goes to workgroups in 2 KiB granules, 80 per CU."""
    def per_cu(key):
        return 80 // -(-pkg.block_lds_bytes(*_args(*key)) // 2048)
    assert per_cu(("d3", 6, 16)) == 4 and per_cu(("d1", 4, 8)) == 3 and per_cu(("d2", 4, 8)) == 4
