"""Golden activations of the expand layers (b2..b7) and the masks, recorded on
the GPU from a build of the commit BEFORE the expand blocks took their weights
from per-wave fragment records (tests/test_gpu_expand_frag.py holds every later
build bitwise equal to them).

Run from the repo root, on a machine with an MI355X, with the library of the
commit to record (its hash is stored in the file):
    VSS_LIBRARY=<that build's libvss.so> python tests/golden/make_expand_golden.py <commit hash> [out.npz]

Config: model 48 x 80, 3 frames of 60 x 100 RGB (seeds 700..702), autotune off.
b7 is 3 x 5 pixels and b2 12 x 20 there: every expand layer has ragged tiles in
both directions, the edge vmask paths run, and the batch is odd.  Recorded for
bf16x2 and f32, each without and with the hidden split (VSS_KSPLIT=1; a split
layer's value is its parts summed in part order, as vss_read_layer reports it).
Keys: <dtype>[_ks]_L<layer> for layers 2..7 and <dtype>[_ks]_masks.

To keep the file small only bf16x2's arrays are stored as floats.  Every other
array is stored as the XOR of its bits (uint32) with those of its base array —
f32's with bf16x2's, a _ks array's with the same dtype's unsplit one: they
agree in all but the low mantissa bits, so the differences compress well and
the floats come back exactly (decode()).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODEL_HW = (48, 80)
FRAME_HW = (60, 100)
SEEDS = (700, 701, 702)
LAYERS = (2, 3, 4, 5, 6, 7)
DTYPES = ("bf16x2", "f32")


def frames(syn) -> np.ndarray:
    return np.stack([syn.make_frame(s, FRAME_HW[0], FRAME_HW[1], 3) for s in SEEDS])


def record(pkg, f: np.ndarray, dtype: str, ksplit: bool) -> dict:
    """{key: array} of one configuration (a new session: VSS_KSPLIT is read at creation)."""
    if ksplit:
        os.environ["VSS_KSPLIT"] = "1"
    else:
        os.environ.pop("VSS_KSPLIT", None)
    try:
        with pkg.Session(model_h=MODEL_HW[0], model_w=MODEL_HW[1], dtype=dtype, max_batch=len(f),
                         max_frame_h=FRAME_HW[0], max_frame_w=FRAME_HW[1], autotune=False) as s:
            masks, _, _ = s.segment_frames(f)
            pre = dtype + ("_ks" if ksplit else "")
            out = {f"{pre}_L{li}": s.read_layer(li, len(f)) for li in LAYERS}
            out[f"{pre}_masks"] = masks
    finally:
        os.environ.pop("VSS_KSPLIT", None)
    return out


def base_key(key: str):
    """The key an array is stored relative to (None: stored as is)."""
    dt, rest = key.split("_", 1)
    if rest.startswith("ks_"):
        return f"{dt}_{rest[3:]}"
    return None if dt == "bf16x2" else f"bf16x2_{rest}"


def encode(data: dict) -> dict:
    out = {}
    for k, v in data.items():
        b = base_key(k)
        out[k] = v if b is None else v.view(np.uint32) ^ data[b].view(np.uint32)
    return out


def decode(g, key: str) -> np.ndarray:
    """Array `key` of the loaded fixture g, as recorded."""
    b = base_key(key)
    return g[key] if b is None else (g[key] ^ decode(g, b).view(np.uint32)).view(np.float32)


def main():
    from conftest import load_pkg
    pkg = load_pkg()
    import vss_amd.synthetic as syn

    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "expand_parent.npz")
    f = frames(syn)
    data = {}
    for dt in DTYPES:
        for ks in (False, True):
            data.update(record(pkg, f, dt, ks))
    np.savez_compressed(path, commit=np.array(commit), seeds=np.array(SEEDS), model_hw=np.array(MODEL_HW),
                        frame_hw=np.array(FRAME_HW), **encode(data))
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items() if k.startswith("bf16x2_")})


if __name__ == "__main__":
    main()
