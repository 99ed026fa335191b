"""Digests of every layer's output and of the masks, recorded on the GPU from
a build of the commit BEFORE the layer kernels' entry code changed (the tile
remap by host-computed reciprocals instead of run-time divisions)
(tests/test_gpu_layer_entry.py holds every later build bitwise equal to them).

Run from the repo root, on a machine with an MI355X, with the library of the
commit to record (its hash is stored in the file):
    VSS_LIBRARY=<that build's libvss.so> python tests/golden/make_entry_golden.py <commit hash> [out.npz]

Shapes, chosen for the entry code (workgroup -> tile, frame and slice):
  * model 32 x 48, 1 frame of 40 x 60 RGB: the deep layers' grids have fewer
    than 8 workgroups, so no workgroup is remapped (`per` = 0);
  * model 80 x 112, 3 frames of 100 x 140 RGB: ragged tiles, grids whose sizes
    are no multiple of 8 (a remapped part and a remainder that keeps its index).
Each for bf16x2, f32 and bf16x2 with VSS_KSPLIT=1 (grid z = frame x slice),
autotune off, eager launches and graph replay.  One session of one slot runs
CALLS device calls, each with its own mask buffer and alternating between two
sets of frames: with more buffer pairs than a slot keeps executables, the
last calls patch a graph's kernel arguments.  Recorded: the first call's
masks, and the last call's masks and layer outputs (the stem's too:
VSS_OPT_KEEP_STEM), as SHA-256 digests of the arrays' bytes - equal digests
are equal bits, and the file stays a few KiB.
Keys: m<H>x<W>_<dtype>[_ks]_<eager|graph>_<first_masks|masks|L<layer>>.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (model H, W), (frame H, W), seeds of frame set A, of frame set B
SHAPES = (((32, 48), (40, 60), (720,), (730,)),
          ((80, 112), (100, 140), (710, 711, 712), (713, 714, 715)))
CONFIGS = (("bf16x2", False), ("f32", False), ("bf16x2", True))  # (dtype, VSS_KSPLIT=1)
MODES = ("eager", "graph")
CALLS = 6  # > the executables a slot keeps per shape (4): calls 5 and 6 patch


def prefix(model_hw, dtype: str, ksplit: bool, mode: str) -> str:
    return f"m{model_hw[0]}x{model_hw[1]}_{dtype}{'_ks' if ksplit else ''}_{mode}"


def digest(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def record(pkg, torch, syn, shape, dtype: str, ksplit: bool, mode: str) -> dict:
    """{key: digest} of one configuration (a new session: VSS_KSPLIT is read at creation)."""
    model_hw, frame_hw, seeds_a, seeds_b = shape
    fh, fw = frame_hw
    n = len(seeds_a)
    sets = [torch.from_numpy(np.stack([syn.make_frame(s, fh, fw, 3) for s in seeds])).cuda()
            for seeds in (seeds_a, seeds_b)]
    os.environ.pop("VSS_KSPLIT", None)
    if ksplit:
        os.environ["VSS_KSPLIT"] = "1"
    try:
        with pkg.Session(model_h=model_hw[0], model_w=model_hw[1], dtype=dtype, max_batch=n, max_frame_h=fh,
                         max_frame_w=fw, autotune=False, queue_depth=1) as s:
            s.set_option(pkg.VSS_OPT_USE_GRAPH, 1 if mode == "graph" else 0)
            s.set_option(pkg.VSS_OPT_KEEP_STEM, 1)
            outs = [torch.full((n, s.mask_h * s.mask_w), float("nan"), device="cuda") for _ in range(CALLS)]
            torch.cuda.synchronize()
            for k in range(CALLS):
                s.segment_device(sets[k % 2].data_ptr(), n, fh, fw, 3, fw * 3, fh * fw * 3, outs[k].data_ptr())
            s.synchronize()
            torch.cuda.synchronize()
            patches = s.graph_patches
            pre = prefix(model_hw, dtype, ksplit, mode)
            out = {f"{pre}_L{li}": digest(s.read_layer(li, n)) for li in range(s.n_layers - 1)}
            out[f"{pre}_first_masks"] = digest(outs[0].cpu().numpy())
            out[f"{pre}_masks"] = digest(outs[CALLS - 1].cpu().numpy())
            out[f"{pre}_patches"] = np.array(patches)
    finally:
        os.environ.pop("VSS_KSPLIT", None)
    return out


def record_all(pkg, torch, syn) -> dict:
    data = {}
    for shape in SHAPES:
        for dt, ks in CONFIGS:
            for mode in MODES:
                data.update(record(pkg, torch, syn, shape, dt, ks, mode))
    return data


def main():
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    import vss_amd.synthetic as syn

    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "entry_parent.npz")
    data = record_all(pkg, torch, syn)
    np.savez_compressed(path, commit=np.array(commit), calls=np.array(CALLS), **data)
    print(path, os.path.getsize(path), "bytes;", len(data), "arrays; patches",
          {k: int(v) for k, v in data.items() if k.endswith("_patches")})


if __name__ == "__main__":
    main()
