"""The expand blocks take their chunks' weights from per-wave fragment records
in global memory instead of an LDS weight image: same operations in the same
order, so every expand layer's output and the masks are bitwise what the commit
before that change produced — recorded on the GPU from a build of it
(tests/golden/expand_parent.npz, made by tests/golden/make_expand_golden.py).

Model 48 x 80, 3 frames of 60 x 100 RGB, autotune off: b7 is 3 x 5 pixels and
b2 12 x 20, so every expand layer has ragged tiles in both directions, the edge
vmask paths run, and the batch is odd.  Both precisions; once more with the
hidden split (VSS_KSPLIT=1), whose slices use the same records with chunk
indices local to the slice.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_expand_golden as gold  # noqa: E402  (the fixture's config and its decoding)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "expand_parent.npz"), allow_pickle=False)
    assert len(str(g["commit"])) == 40  # the recorded commit's hash
    assert tuple(g["model_hw"]) == gold.MODEL_HW and tuple(g["frame_hw"]) == gold.FRAME_HW
    assert tuple(g["seeds"]) == gold.SEEDS
    return g


@pytest.mark.parametrize("ksplit", [False, True], ids=["unsplit", "ksplit"])
@pytest.mark.parametrize("dtype", gold.DTYPES)
def test_expand_layers_bitwise_parent(pkg, synthetic, golden, dtype, ksplit):
    got = gold.record(pkg, gold.frames(synthetic), dtype, ksplit)
    assert len(got) == len(gold.LAYERS) + 1
    bad = [k for k, v in got.items()
           if not np.array_equal(np.ascontiguousarray(v).view(np.uint32), gold.decode(golden, k).view(np.uint32))]
    assert not bad, bad
