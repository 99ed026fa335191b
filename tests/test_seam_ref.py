"""CPU tests of tests/seam_ref.py, the f64 one-layer-at-a-time reference of the
seam and its error bound (derived in that module's docstring):

  * it agrees, layer by layer and within its f32 bound, with the project's two
    other CPU implementations (oracle/vss_oracle.c for every blob family,
    oracle/torch_ref.py for the seed-7 blob);
  * each blob family reaches the branch it was built for;
  * six deliberately wrong layers each leave the bound, in both modes' bounds
    (a bound that let them pass would be too loose to be worth asserting);
  * the device's norm formula, restated with its roundings, stays inside the
    statistics' error model the bound starts from.

Model 48 x 80 (levels 24x40 .. 3x5), 2 frames: one synthetic, one all 255."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_ref as sr  # noqa: E402

HM, WM = 48, 80
ALL = ("seed7",) + sr.FAMILIES


@pytest.fixture(scope="module")
def frames(synthetic):
    return np.stack([synthetic.make_frame(3, 100, 140, 3), np.full((100, 140, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def blobs():
    return {name: sr.family_blob(name) for name in ALL}


@pytest.fixture(scope="module")
def runs(oracle, blobs, frames):
    """Per family: (net, x0, the oracle's f32 taps [layer] -> [N, C, H, W], the
    reference's Out per layer on the oracle's inputs); computed once."""
    out = {}
    x0 = oracle.preprocess(frames, HM, WM)
    for name, b in blobs.items():
        net = sr.Net(b)
        masks, taps = oracle.forward(b, frames, HM, WM, mode=0, want_taps=True)
        outs = [np.stack([taps[i][li] for i in range(len(frames))]) for li in range(net.n_layers)]
        outs[-1] = masks[:, None]
        refs = [sr.layer(net, li, sr.inputs_of(net, li, outs, x0)) for li in range(net.n_layers)]
        out[name] = (net, x0, outs, refs)
    return out


def test_seed7_family_is_the_committed_blob(blob, blobs):
    assert blobs["seed7"] == blob


@pytest.mark.parametrize("name", ALL)
def test_reference_matches_the_c_oracle(runs, name):
    net, _, outs, refs = runs[name]
    for li in range(net.n_layers):
        assert outs[li].shape == refs[li].y.shape, li
        ratio, at, err, bound = sr.worst(outs[li], refs[li], "f32")
        print(f"{name} layer {li}: worst err/bound {ratio:.3f} at {at} (err {err:.3e}, bound {bound:.3e})")
        assert ratio <= 1.0, f"{name} layer {li}: err {err:.3e} > bound {bound:.3e} at {at}"


def test_reference_matches_torch_ref(blob, frames):
    import torch_ref
    net = sr.Net(blob)
    taps = []
    torch_ref.forward(blob, frames, HM, WM, mode=0, taps=taps)
    outs = [t.numpy() for t in taps]
    x0 = torch_ref.preprocess(frames, HM, WM).numpy()
    for li in range(net.n_layers):
        ref = sr.layer(net, li, sr.inputs_of(net, li, outs, x0))
        ratio, at, err, bound = sr.worst(outs[li], ref, "f32")
        print(f"torch_ref layer {li}: worst err/bound {ratio:.3f} at {at}")
        assert ratio <= 1.0, f"layer {li}: err {err:.3e} > bound {bound:.3e} at {at}"


def _dec_layers(net):
    return [li for li in range(net.n_layers) if net.kind(li) == sr.K_DEC]


def test_saturate_reaches_the_upper_clamp(runs):
    net, _, _, refs = runs["saturate"]
    stem = refs[0].y
    hidden = refs[2].aux["hidden"]  # b2's expand output
    assert net.kind(2) == sr.K_IR and hidden.shape[1] == 64
    print(f"saturate: stem at 6: {np.mean(stem == 6.0):.3f}, b2 hidden at 6: {np.mean(hidden == 6.0):.3f}")
    assert np.mean(stem == 6.0) >= 0.30
    assert np.mean(hidden == 6.0) >= 0.30


def test_tiny_reaches_variance_below_eps(runs):
    net, _, outs, _ = runs["tiny"]
    small = 0
    for li in _dec_layers(net):
        _, var = sr.stats(outs[li].astype(np.float64))
        small += int((var < net.eps).sum())
        q_zero = np.mean(np.rint(outs[li].astype(np.float64) ** 2 * 2.0 ** 24) == 0)
        print(f"tiny layer {li}: min var {var.min():.3e}, channels below eps {int((var < net.eps).sum())}, "
              f"q terms that round to 0: {q_zero:.3f}")
    assert small > 0


def test_huge_dec_reaches_the_int64_resummation(runs, oracle, blobs, frames):
    net, _, _, refs = runs["huge_dec"]
    # the GPU tests' other size as well (the totals grow with the pixel count)
    _, taps = oracle.forward(blobs["huge_dec"], frames, 80, 112, mode=0, want_taps=True)
    for li in _dec_layers(net):
        big = np.stack([taps[i][li] for i in range(len(frames))]).astype(np.float64)
        assert ((big * big).sum(axis=(2, 3)) * 2.0 ** 24).max() < 2.0 ** 63
        assert np.abs(big.sum(axis=(2, 3)) * 2.0 ** 32).max() < 2.0 ** 63
        v = refs[li].y
        q = (v * v).sum(axis=(2, 3)) * 2.0 ** 24
        print(f"huge_dec layer {li}: max|v| {np.abs(v).max():.1f}, max q total 2^{np.log2(q.max()):.1f}")
        assert np.abs(v).max() >= 2.0 ** 12
        assert q.max() < 2.0 ** 63
        # a single q term of 2^51 takes its lane into the int64 branch whatever the tiling
        assert (v * v * 2.0 ** 24).max() >= 2.0 ** 51


def test_offset_dec_reaches_mean_far_above_spread(runs):
    net, _, _, refs = runs["offset_dec"]
    for li in _dec_layers(net):
        mean, var = sr.stats(refs[li].y)
        r = np.abs(mean) / np.sqrt(var)
        print(f"offset_dec layer {li}: max |mean|/std {r.max():.1f}")
        assert r.max() >= 100.0


def _applies(net, li, mutant):
    kind, flags = net.kind(li), net.recs[li][5]
    reads_dec = kind in (sr.K_DEC, sr.K_HEAD) and net.kind(net.src(li)) == sr.K_DEC
    return {"bf16_act": kind in (sr.K_IR, sr.K_DEC), "dw_swap": kind in (sr.K_IR, sr.K_DEC),
            "up_clamp": kind in (sr.K_DEC, sr.K_HEAD), "no_residual": kind == sr.K_IR and bool(flags & sr.F_RESIDUAL),
            "var_nm1": reads_dec, "no_beta": reads_dec}[mutant]


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_bound_catches_a_wrong_layer(runs, mutant):
    """The mutant layer, on the same inputs, leaves the right layer's bound on
    at least one element, in every layer it applies to and in both modes."""
    net, x0, outs, refs = runs["seed7"]
    hit = 0
    for li in range(net.n_layers):
        if not _applies(net, li, mutant):
            continue
        bad = sr.layer(net, li, sr.inputs_of(net, li, outs, x0), mutate=mutant)
        for mode in sr.MODES:
            ratio, at, err, bound = sr.worst(bad.y, refs[li], mode)
            print(f"{mutant} layer {li} {mode}: worst err/bound {ratio:.1f} at {at}")
            assert ratio > 1.0, f"{mutant} stays inside the {mode} bound of layer {li} (worst {ratio:.3f})"
        hit += 1
    assert hit > 0


def _device_norm(v, gamma, beta, eps):
    """norm_affine and the consumer's relu(v * scale + shift) of csrc/vss_kernels.h
    restated in numpy with the device's roundings (f32 products, the fixed-point
    terms, int64 totals, f64 statistics, f32 scale and shift; no FMA)."""
    f32 = np.float32
    v = v.astype(f32)
    n = v.shape[2] * v.shape[3]
    s = np.rint(v.astype(np.float64) * 2.0 ** 32).astype(np.int64).sum(axis=(2, 3), keepdims=True)
    q = np.rint((v * v).astype(np.float64) * 2.0 ** 24).astype(np.int64).sum(axis=(2, 3), keepdims=True)
    mean = s.astype(np.float64) * (2.0 ** -32 * (1.0 / n))
    ex2 = q.astype(np.float64) * (2.0 ** -24 * (1.0 / n))
    var = np.maximum(ex2 - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(f32(eps)))).astype(f32)
    sc = rstd * gamma.astype(f32)[None, :, None, None]
    sh = beta.astype(f32)[None, :, None, None] - mean.astype(f32) * sc
    return np.maximum(v * sc + sh, f32(0)).astype(np.float64)


@pytest.mark.parametrize("name", ALL)
def test_statistics_error_model_covers_the_device_formula(runs, name):
    """The device's norm arithmetic, restated, stays inside e_a, the error model
    the bound starts from; the figures for DESIGN.md's note on what that model
    allows (offset_dec, tiny) are printed."""
    net, _, outs, _ = runs[name]
    for li in _dec_layers(net):
        w = net.weights(li)
        v = outs[li].astype(np.float64)
        a, e_a, mean, var = sr.norm_relu(v, w["gamma"], w["beta"], net.eps)
        err = np.abs(_device_norm(outs[li], w["gamma"], w["beta"], net.eps) - a)
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        r = (np.abs(mean) / np.sqrt(var + net.eps))[at[0], at[1], 0, 0]
        print(f"{name} layer {li}: worst normalised-output error {err.max():.3e} (model allows {e_a[at]:.3e}) "
              f"at |mean|/std {r:.1f}, var {var[at[0], at[1], 0, 0]:.3e}; worst err/e_a {np.max(err / e_a):.3f}")
        assert np.all(err <= sr.SECOND * e_a)
