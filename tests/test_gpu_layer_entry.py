"""The layer kernels' entry code — workgroup -> (tile, frame, slice) from the
tile map the host passes with the kernel's parameters — and the graph path's
parameter patching leave every float as it was: each layer's output and the
masks are bitwise what the commit before that change produced, recorded on the
GPU from a build of it (tests/golden/entry_parent.npz, made by
tests/golden/make_entry_golden.py, which documents the shapes).

Model 32 x 48 with 1 frame (the deep layers' grids have fewer than 8
workgroups) and model 80 x 112 with 3 frames (ragged tiles, grids whose sizes
are no multiple of 8); bf16x2, f32 and bf16x2 with VSS_KSPLIT=1; eager launches
and graph replay; six calls on one slot with rotating buffers, so that the last
graph calls patch their executable's kernel arguments.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_entry_golden as gold  # noqa: E402  (the fixture's config and its recipe)

pytestmark = pytest.mark.gpu

CASES = [(shape, dt, ks, mode) for shape in gold.SHAPES for dt, ks in gold.CONFIGS for mode in gold.MODES]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "entry_parent.npz"), allow_pickle=False)
    assert len(str(g["commit"])) == 40 and int(g["calls"]) == gold.CALLS  # the recorded commit's hash
    return g


@pytest.mark.parametrize("shape,dtype,ksplit,mode", CASES,
                         ids=[gold.prefix(s[0], d, k, m) for s, d, k, m in CASES])
def test_layers_bitwise_parent(pkg, synthetic, golden, shape, dtype, ksplit, mode):
    import torch
    got = gold.record(pkg, torch, synthetic, shape, dtype, ksplit, mode)
    pre = gold.prefix(shape[0], dtype, ksplit, mode)
    want = {k: golden[k] for k in golden.files if k.startswith(pre + "_")}
    assert len(want) == 11 + 3 and sorted(got) == sorted(want)  # 11 layer outputs, 2 masks, the patch count
    # the graph calls past the slot's executables patched one; eager calls never do
    assert int(got[pre + "_patches"]) == int(want[pre + "_patches"]) == (gold.CALLS - 4 if mode == "graph" else 0)
    bad = [k for k in sorted(want) if not np.array_equal(got[k], want[k])]
    assert not bad, bad
