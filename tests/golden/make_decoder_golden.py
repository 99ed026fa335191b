"""Golden activations of the decoder layers (d1..d3) and the masks, recorded on
the GPU from a build of the commit BEFORE the decoders' even tiles took their
upsample taps from registers instead of a low-res region in LDS
(tests/test_gpu_decoder_direct.py holds every later build bitwise equal to them).

Run from the repo root, on a machine with an MI355X, with the library of the
commit to record (its hash is stored in the file):
    VSS_LIBRARY=<that build's libvss.so> python tests/golden/make_decoder_golden.py <commit hash> [out.npz]

Config: model 80 x 112, 3 frames of 100 x 140 RGB (seeds 710..712), autotune
off.  d1 is 10 x 14 pixels, d2 20 x 28 and d3 40 x 56 there: the batch is odd,
and 4 x 8 tiles in d1, 6 x 16 tiles in d3 and 6-row tiles in d2 are partial at
the bottom and at the right.  Recorded for bf16x2 and f32, and bf16x2 once more
with the hidden split (VSS_KSPLIT=1: d1's src then arrives in parts, summed in
part order as the prologue loads them).
Keys: <dtype>[_ks]_L<layer> for layers 8..10 and <dtype>[_ks]_masks.

To keep the file small only bf16x2's arrays are stored as floats.  Every other
array is stored as the XOR of its bits (uint32) with those of bf16x2's array —
they agree in all but the low mantissa bits — and every array is stored as its
four byte planes (all the low bytes, then the next ones, ...): the planes of
equal bytes compress where the interleaved words do not.  The floats come back
exactly (decode()).  Float mantissas do not compress: bf16x2's arrays alone are
0.68 MB, so they are one file (decoder_parent.npz) and the XORs another
(decoder_parent_xor.npz, 0.6 MB), each under the 1 MB a committed file may have.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODEL_HW = (80, 112)
FRAME_HW = (100, 140)
SEEDS = (710, 711, 712)
LAYERS = (8, 9, 10)  # d1, d2, d3
# (cin, cskip, cout) of the layers (model/spec.json): their k_block shape is
# mode 2, stride 1, chid = cin + cskip
SHAPES = {8: (64, 48, 48), 9: (48, 32, 32), 10: (32, 16, 16)}
CONFIGS = (("bf16x2", False), ("f32", False), ("bf16x2", True))  # (dtype, VSS_KSPLIT=1)


def frames(syn) -> np.ndarray:
    return np.stack([syn.make_frame(s, FRAME_HW[0], FRAME_HW[1], 3) for s in SEEDS])


def prefix(dtype: str, ksplit: bool) -> str:
    return dtype + ("_ks" if ksplit else "")


def record(pkg, f: np.ndarray, dtype: str, ksplit: bool, tiles: str = "", check=None) -> dict:
    """{key: array} of one configuration (a new session: VSS_KSPLIT and VSS_TILE
    are read at creation).  tiles = a VSS_TILE spec or ""; check(session) runs
    before the forward."""
    env = {"VSS_KSPLIT": "1" if ksplit else None, "VSS_TILE": tiles or None}
    for k, v in env.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        with pkg.Session(model_h=MODEL_HW[0], model_w=MODEL_HW[1], dtype=dtype, max_batch=len(f),
                         max_frame_h=FRAME_HW[0], max_frame_w=FRAME_HW[1], autotune=False) as s:
            if check is not None:
                check(s)
            masks, _, _ = s.segment_frames(f)
            pre = prefix(dtype, ksplit)
            out = {f"{pre}_L{li}": s.read_layer(li, len(f)) for li in LAYERS}
            out[f"{pre}_masks"] = masks
    finally:
        for k in env:
            os.environ.pop(k, None)
    return out


def base_key(key: str):
    """The key an array is stored relative to (None: stored as is)."""
    pre, rest = key.rsplit("_", 1)
    return None if pre == "bf16x2" else f"bf16x2_{rest}"


def _planes(u32: np.ndarray) -> np.ndarray:
    """[4][...] uint8: byte b of every word (little-endian order made explicit)."""
    return np.stack([((u32 >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8) for b in range(4)])


def encode(data: dict) -> dict:
    out = {}
    for k, v in data.items():
        b = base_key(k)
        bits = np.ascontiguousarray(v).view(np.uint32)
        out[k] = _planes(bits if b is None else bits ^ np.ascontiguousarray(data[b]).view(np.uint32))
    return out


def _bits(g, key: str) -> np.ndarray:
    p = g[key].astype(np.uint32)
    w = p[0] | (p[1] << np.uint32(8)) | (p[2] << np.uint32(16)) | (p[3] << np.uint32(24))
    b = base_key(key)
    return w if b is None else w ^ _bits(g, b)


def decode(g, key: str) -> np.ndarray:
    """Array `key` of the loaded fixture g, as recorded (float32)."""
    return _bits(g, key).view(np.float32)


def xor_path(path: str) -> str:
    return path[:-4] + "_xor.npz"


def save(data: dict, commit: str, path: str) -> int:
    """Writes `path` (bf16x2's arrays) and xor_path(path) (every other array's XOR with them)."""
    enc = encode(data)
    meta = dict(commit=np.array(commit), seeds=np.array(SEEDS), model_hw=np.array(MODEL_HW), frame_hw=np.array(FRAME_HW))
    np.savez_compressed(path, **meta, **{k: v for k, v in enc.items() if base_key(k) is None})
    np.savez_compressed(xor_path(path), **meta, **{k: v for k, v in enc.items() if base_key(k) is not None})
    return max(os.path.getsize(path), os.path.getsize(xor_path(path)))


def load(path: str) -> dict:
    """The two files' arrays in one dict (for decode()); their metadata must agree."""
    a, b = (np.load(q, allow_pickle=False) for q in (path, xor_path(path)))
    for k in ("commit", "seeds", "model_hw", "frame_hw"):
        assert np.array_equal(a[k], b[k]), k
    return {**{k: b[k] for k in b.files}, **{k: a[k] for k in a.files}}


def main():
    from conftest import load_pkg
    pkg = load_pkg()
    import vss_amd.synthetic as syn

    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "decoder_parent.npz")
    f = frames(syn)
    data = {}
    for dt, ks in CONFIGS:
        data.update(record(pkg, f, dt, ks))
    size = save(data, commit, path)
    print(path, "largest file", size, "bytes;", {k: v.shape for k, v in data.items() if k.startswith("bf16x2_L")})


if __name__ == "__main__":
    main()
