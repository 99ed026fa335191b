"""The seam's kernels LAYER BY LAYER against the f64 reference of tests/seam_ref.py,
on more than the seed-7 weights, in both pointwise modes.

Every layer li of a forward is read back (vss_read_layer; the stem under
VSS_OPT_KEEP_STEM), the reference computes layer li from the GPU's OWN outputs
of li's src and skip layers (the stem: from oracle.preprocess, pinned bit-exact
elsewhere), and |gpu - ref| <= bound must hold element by element, the bound
being the one derived in seam_ref's docstring for the mode.  The mask is
checked as the head's output.  Earlier layers' errors do not add up, small
elements are held as tightly as large ones, and an error all tiles share shows.

Blob families (seam_ref.family): two more draws of the generator, and four
scalings of the seed-7 blob that reach branches no O(1) activation reaches:
the upper clamp of relu6, var < eps, the int64 re-summation of the statistics
epilogue (q >= 2^51), and a mean far above the spread.

Model 48 x 80 and 80 x 112: the /16 levels are 3x5 and 5x7, every level is
odd-sized against every tile.  3 frames of 100 x 140: all 0, all 255, synthetic.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(48, 80), (80, 112)]
FH, FW = 100, 140


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    """{family: (path, Net)}: the blobs written once into a temporary directory."""
    d = tmp_path_factory.mktemp("seam_blobs")
    out = {}
    for name in sr.FAMILIES:
        b = sr.family_blob(name)
        p = d / f"{name}.bin"
        p.write_bytes(b)
        out[name] = (str(p), sr.Net(b))
    return out


@pytest.fixture(scope="module")
def frames(synthetic):
    """8 frames of 100 x 140: all 0, all 255, then synthetic ones (the first 3 are the standard set)."""
    f = [np.zeros((FH, FW, 3), np.uint8), np.full((FH, FW, 3), 255, np.uint8)]
    f += [synthetic.make_frame(60 + i, FH, FW, 3) for i in range(6)]
    return np.stack(f)


def _forward(pkg, path, mode, hm, wm, f, max_batch=None):
    """One forward of a new session -> (the per-layer outputs [N, C, H, W], the last being the
    masks; each layer's kernel; each layer's compiled candidates, by name)."""
    n = len(f)
    with pkg.Session(model_h=hm, model_w=wm, dtype=mode, max_batch=max_batch or n, max_frame_h=FH, max_frame_w=FW,
                     weights_path=path, autotune=False) as s:
        s.set_option(pkg.VSS_OPT_KEEP_STEM, 1)
        masks, mw, mh = s.segment_frames(f)
        assert (mh, mw) == (hm, wm)
        outs = [s.read_layer(li, n) for li in range(s.n_layers - 1)]
        kernels = [s.layer_kernel(li) for li in range(s.n_layers)]
        tiles = {li: [s.layer_tile_kernel(li, k) for k in range(len(s.layer_tiles(li)))] for li in range(s.n_layers)}
    return outs + [masks.reshape(n, 1, hm, wm).copy()], kernels, tiles


def _check(tag, net, mode, outs, x0, layers=None):
    """Every layer (or `layers`) of outs against the reference on the GPU's own inputs."""
    bad, row = [], []
    for li in (range(net.n_layers) if layers is None else layers):
        ref = sr.layer(net, li, sr.inputs_of(net, li, outs, x0))
        assert outs[li].shape == ref.y.shape, (tag, li, outs[li].shape, ref.y.shape)
        assert np.isfinite(outs[li]).all(), (tag, li)
        ratio, at, err, bound = sr.worst(outs[li], ref, mode)
        print(f"{tag} {mode} layer {li}: worst err/bound {ratio:.3f} at {at} (err {err:.3e}, bound {bound:.3e}, "
              f"ref {ref.y[at]:.6g}, its channel's std {ref.y[at[0], at[1]].std():.3g}); "
              f"largest err {np.abs(outs[li] - ref.y).max():.3e}")
        row.append(f"{ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((li, ratio, at, err, bound))
    print(f"TABLE {tag} {mode} | " + " | ".join(row))
    assert not bad, f"{tag} {mode}: layers outside the bound (layer, err/bound, index, err, bound): {bad}"


@pytest.mark.parametrize("hm,wm", SIZES)
@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("name", sr.FAMILIES)
def test_layers_inside_the_bound(pkg, torch_cuda, oracle, blobs, frames, name, mode, hm, wm):
    path, net = blobs[name]
    f = frames[:3]
    outs, _, _ = _forward(pkg, path, mode, hm, wm, f)
    if name == "huge_dec":  # what the family is for, on these frames: the int64 branch runs, the totals fit
        for li in range(net.n_layers):
            if net.kind(li) == sr.K_DEC:
                q = outs[li].astype(np.float64) ** 2 * 2.0 ** 24
                assert q.max() >= 2.0 ** 51 and q.sum(axis=(2, 3)).max() < 2.0 ** 62, (li, q.max())
    _check(f"{name} {hm}x{wm}", net, mode, outs, oracle.preprocess(f, hm, wm))


@pytest.mark.parametrize("mode", sr.MODES)
def test_headline_planner_choices(pkg, torch_cuda, oracle, blobs, frames, mode):
    """144 x 256, max_batch 8, 8 frames: the kernels the headline runs."""
    path, net = blobs["seed11"]
    outs, _, _ = _forward(pkg, path, mode, 144, 256, frames)
    _check("seed11 144x256 b8", net, mode, outs, oracle.preprocess(frames, 144, 256))


@pytest.mark.parametrize("hm,wm", [(48, 80), (144, 256)])
@pytest.mark.parametrize("mode", sr.MODES)
def test_batch_one(pkg, torch_cuda, oracle, blobs, frames, mode, hm, wm, monkeypatch):
    """max_batch = 1: the batch-1 tiles, and the wide stem + b1 kernel (k_stem_b1, which only
    the autotuner picks: pinned here, every compiled tile of it)."""
    path, net = blobs["seed11"]
    f = frames[2:3]
    x0 = oracle.preprocess(f, hm, wm)
    outs, _, tiles = _forward(pkg, path, mode, hm, wm, f, max_batch=1)
    _check(f"seed11 {hm}x{wm} b1", net, mode, outs, x0)
    wide = [k for k, name in enumerate(tiles[1]) if "k_stem_b1<" in name]
    assert wide, tiles[1]
    for k in wide:
        monkeypatch.setenv("VSS_TILE", f"1:#{k}")
        got, pinned, _ = _forward(pkg, path, mode, hm, wm, f, max_batch=1)
        assert pinned[1] == tiles[1][k]
        _check(f"seed11 {hm}x{wm} b1 {tiles[1][k].split('(')[0].split('::')[1]}", net, mode, got, x0, layers=[0, 1])


@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("name", ["seed11", "huge_dec"])
def test_hidden_split(pkg, torch_cuda, oracle, blobs, frames, name, mode, monkeypatch):
    """VSS_KSPLIT=1 at 80 x 112: the deep expand layers in parts, their consumers summing them."""
    monkeypatch.setenv("VSS_KSPLIT", "1")
    path, net = blobs[name]
    f = frames[:3]
    outs, kernels, _ = _forward(pkg, path, mode, 80, 112, f)
    flags = [int(k.split("<")[1].split(",")[8]) for k in kernels if "k_block<" in k]
    assert any((fl >> 6) & 3 for fl in flags), kernels  # some layer split (KS > 1)
    _check(f"{name} 80x112 ksplit", net, mode, outs, oracle.preprocess(f, 80, 112))


@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("name", ["huge_dec", "offset_dec"])
def test_decoder_tiles_agree_bitwise(pkg, torch_cuda, oracle, blobs, frames, name, mode, monkeypatch):
    """Every compiled tile of d1, d2, d3 (VSS_TILE="li:#k") at 48 x 80: the decoders
    and the masks bitwise equal to the unpinned run (the statistics epilogue's
    totals do not depend on the tiling, the int64 fallback included), and inside
    the bound."""
    path, net = blobs[name]
    f = frames[:3]
    x0 = oracle.preprocess(f, 48, 80)
    ref, _, tiles = _forward(pkg, path, mode, 48, 80, f)
    dec = [li for li in range(net.n_layers) if net.kind(li) == sr.K_DEC]
    assert dec == [8, 9, 10] and all(len(tiles[li]) > 1 for li in dec), tiles
    bad = []
    for li in dec:
        for k in range(len(tiles[li])):
            monkeypatch.setenv("VSS_TILE", f"{li}:#{k}")
            got, kernels, _ = _forward(pkg, path, mode, 48, 80, f)
            diff = [q for q in dec + [net.n_layers - 1] if not np.array_equal(got[q], ref[q])]
            if diff:
                bad.append((li, k, kernels[li], diff))
            _check(f"{name} 48x80 tile {li}:#{k}", net, mode, got, x0, layers=dec + [net.n_layers - 1])
    assert not bad, bad
