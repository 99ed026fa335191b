"""The reference for quantised (QDQ) graphs, tests/onnx_ref_quant.py, and the
case table tests/op_cases_quant.py, checked on the CPU:

* QuantizeLinear / DequantizeLinear against a direct numpy statement of the
  operator text and against torch.quantize_per_tensor; the dequantised Conv
  against torch.nn.functional.conv2d in float64;
* the table's own conditions: in every dyadic case no accumulator reaches
  2^24 (so float32 and float64 agree exactly), each family has exact ties and
  saturated elements, and in every general case at most 2 % of the elements lie
  within TAU of a tie (computed from the reference alone);
* an integer restatement of the fused arithmetic (uint8 activations with the
  top bit flipped, sum x w - zx sum w, spatial padding with zx, K padded to
  64 with zero weights, the float32 epilogue) meets the rules the GPU sessions
  are held to — and seven mutants of it, each a classic silent error, do not.
"""
import numpy as np
import pytest
import torch

import onnx_ref as R
import onnx_ref_quant as RQ
import op_cases_quant as QC

_models = {}


def _model(fam):
    if fam not in _models:
        cases = QC.groups()[fam]
        data, feeds, outs = QC.build(cases)
        m = R.load(data)
        _models[fam] = (cases, feeds, outs, m, RQ.run_all(m, feeds))
    return _models[fam]


# ---- the two operators -------------------------------------------------------------------
def _round_half_even(v):
    f = np.floor(v)
    d = v - f
    return np.where(d > 0.5, f + 1, np.where(d < 0.5, f, np.where(f % 2 == 0, f, f + 1)))


@pytest.mark.parametrize("dtype,zp", [(np.uint8, 0), (np.uint8, 3), (np.uint8, 255), (np.uint8, None), (np.int8, -128),
                                      (np.int8, -5), (np.int8, 127)])
def test_quantize_is_the_operator_text(dtype, zp):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-80, 80, 4000), np.arange(-600, 600) * 0.125, [np.inf, -np.inf, 1e30, -1e30]])
    x = x.astype(np.float32)
    for scale in (0.25, 0.0173):
        lo, hi = QC.RANGE[dtype]
        with np.errstate(invalid="ignore"):
            v = _round_half_even(np.where(np.isfinite(x), x.astype(np.float64) / np.float64(np.float32(scale)), 0.0))
        v = np.where(np.isposinf(x), np.inf, np.where(np.isneginf(x), -np.inf, v)) + (zp or 0)
        want = np.clip(v, lo, hi).astype(dtype)
        got = RQ.quantize_linear(x, np.float32(scale), None if zp is None else np.asarray(zp, dtype))
        assert got.dtype == dtype and np.array_equal(got, want)
        back = RQ.dequantize_linear(got, np.float32(scale), None if zp is None else np.asarray(zp, dtype))
        assert back.dtype == np.float32
        assert np.array_equal(back, ((got.astype(np.float64) - (zp or 0)) * np.float64(np.float32(scale))).astype(np.float32))


def test_ties_round_to_even_and_both_ends_saturate():
    s = np.float32(0.25)
    x = np.asarray([2.5, 3.5, -0.5, -1.5, 0.5, 1.5, 300.0, -300.0], np.float32) * s
    assert RQ.quantize_linear(x, s, np.asarray(0, np.int8)).tolist() == [2, 4, 0, -2, 0, 2, 127, -128]
    assert RQ.quantize_linear(x, s, np.asarray(3, np.uint8)).tolist() == [5, 7, 3, 1, 3, 5, 255, 0]
    assert RQ.quantize_linear(x, s).dtype == np.uint8


@pytest.mark.parametrize("dtype,tq,zp", [(np.uint8, torch.quint8, 3), (np.int8, torch.qint8, -5)])
def test_quantize_is_torch(dtype, tq, zp):
    x = QC.x_gen("torch", 0.125, zp, dtype, True)((2, 3, 12, 13))  # multiples of scale / 2: exact in float32
    q = torch.quantize_per_tensor(torch.from_numpy(x), 0.125, zp, tq)
    got = RQ.quantize_linear(x, np.float32(0.125), np.asarray(zp, dtype))
    assert np.array_equal(got, q.int_repr().numpy())
    assert np.array_equal(RQ.dequantize_linear(got, np.float32(0.125), np.asarray(zp, dtype)), q.dequantize().numpy())


def _pattern(model, out):
    """The nodes of a fused conv case, from its output back: (Q, act or None, Conv, DQ of x)."""
    prod = {o: nd for nd in model.nodes for o in nd["outputs"] if o}
    q = prod[out]
    nd = prod[q["inputs"][0]]
    act = None
    if nd["op"] in ("Relu", "Clip"):
        act, nd = nd, prod[nd["inputs"][0]]
    assert q["op"] == "QuantizeLinear" and nd["op"] == "Conv"
    return q, act, nd, prod[nd["inputs"][0]], prod


SINGLE = [k for k in QC.VALUE_CASES if k.family in (QC.F_QCONV, QC.F_QDW) and QC.META[k.name]["fused"] == 1]


@pytest.mark.parametrize("name", [k.name for k in SINGLE if QC.META[k.name]["weighting"] == "dyadic"][::3])
def test_conv_is_torch_float64(name):
    cs = QC.BY_NAME[name]
    _, _, outs, model, env = _model(cs.family)
    _, _, conv, _, _ = _pattern(model, outs[name][0])
    a, ins = conv["attrs"], conv["inputs"]
    x, w = (torch.from_numpy(env[i].astype(np.float64)) for i in ins[:2])
    b = torch.from_numpy(env[ins[2]].astype(np.float64)) if len(ins) > 2 else None
    pt, pl, pb, pr = R._pads2(a, w.shape[2:], x.shape[2:], a.get("strides", [1, 1]), a.get("dilations", [1, 1]))
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (pl, pr, pt, pb)), w, b, stride=a.get("strides", [1, 1]),
                                   dilation=a.get("dilations", [1, 1]), groups=a.get("group", 1))
    assert np.array_equal(y.numpy().astype(np.float32), env[conv["outputs"][0]])  # dyadic: exact on both sides


# ---- the table's own conditions ----------------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in QC.DYADIC if k.family in (QC.F_QCONV, QC.F_QDW, QC.F_MISS)])
def test_dyadic_accumulators_stay_below_2_24(name):
    cs = QC.BY_NAME[name]
    _, _, _, model, env = _model(cs.family)
    prod = {o: nd for nd in model.nodes for o in nd["outputs"] if o}
    n_conv = 0
    for nd in model.nodes:
        if nd["op"] != "Conv" or not nd["outputs"][0].startswith(name) and not any(
                o.startswith(name) for o in _downstream(model, nd["outputs"][0])):
            continue
        n_conv += 1
        dx, dw = prod[nd["inputs"][0]], prod[nd["inputs"][1]]
        sx, sw = float(env[dx["inputs"][1]]), env[dw["inputs"][1]].astype(np.float64).reshape(-1)
        assert all(np.log2(v) == np.round(np.log2(v)) for v in [sx, *sw]), "a dyadic case with a scale that is no power of two"
        wq = env[dw["inputs"][0]].astype(np.int64)
        zw = env[dw["inputs"][2]].astype(np.int64).reshape(-1, 1, 1, 1) if len(dw["inputs"]) > 2 else 0
        wi = np.abs(wq - zw).reshape(wq.shape[0], -1).sum(axis=1)  # every partial sum of |x - zx| |w| is below 255 sum |w|
        bias = np.abs(env[nd["inputs"][2]].astype(np.float64)) / (sx * sw.min()) if len(nd["inputs"]) > 2 else 0.0
        assert float((255 * wi + bias).max()) < 2 ** 24
    assert n_conv >= 1


def _downstream(model, name, depth=4):
    out, frontier = [], [name]
    for _ in range(depth):
        nxt = [o for nd in model.nodes if any(i in frontier for i in nd["inputs"]) for o in nd["outputs"]]
        out += nxt
        frontier = nxt
    return out


@pytest.mark.parametrize("family", sorted(QC.groups()))
def test_dyadic_families_have_ties_and_saturation(family):
    cases, _, outs, model, env = _model(family)
    ties = sat = 0
    for cs in cases:
        if QC.META[cs.name]["weighting"] != "dyadic":
            continue
        for o in outs[cs.name]:
            v = RQ.unrounded(model, env, o)
            if v is None:
                continue
            lo, hi = QC.RANGE[env[o].dtype.type]
            fin = np.isfinite(v)
            ties += int((np.abs(v[fin] - np.floor(v[fin])) == 0.5).sum())
            sat += int(((v[fin] > hi + 0.5) | (v[fin] < lo - 0.5)).sum())
    print(f"{family}: {ties} exact ties, {sat} saturated elements in the dyadic cases")
    assert ties >= 1 and sat >= 1


@pytest.mark.parametrize("name", [k.name for k in QC.GENERAL])
def test_general_near_tie_share(name):
    cs = QC.BY_NAME[name]
    _, _, outs, model, env = _model(cs.family)
    for o in outs[name]:
        v = RQ.unrounded(model, env, o)
        if v is None:
            continue
        share = float(QC.near_tie(v).mean())
        print(f"{o}: {share:.4%} of {v.size} within TAU of a tie")
        assert share <= QC.NEAR_TIE_SHARE


# ---- the fused arithmetic, restated in integers ------------------------------------------
MUTANTS = ("pad_zero", "kpad_zx", "no_sum_w", "half_away", "wrong_range", "scale_axis", "relu_after")


def restate(model, env, out, mutant=None):
    """The case's quantised output as k_qconv_tile / k_qconv_dw compute it, in numpy integers and float32."""
    q, act, conv, dqx, prod = _pattern(model, out)
    dqw = prod[conv["inputs"][1]]
    a = conv["attrs"]
    xq = env[dqx["inputs"][0]]
    sx = np.float32(env[dqx["inputs"][1]])
    zx = int(env[dqx["inputs"][2]]) if len(dqx["inputs"]) > 2 else 0
    wq = env[dqw["inputs"][0]].astype(np.int64)
    M = wq.shape[0]
    sw = np.broadcast_to(env[dqw["inputs"][1]].astype(np.float32).reshape(-1), (M,)) if env[dqw["inputs"][1]].size in (1, M) else None
    zw = np.broadcast_to(env[dqw["inputs"][2]].astype(np.int64).reshape(-1), (M,)) if len(dqw["inputs"]) > 2 else np.zeros(M, np.int64)
    wi = wq - zw.reshape(-1, 1, 1, 1)
    assert wi.min() >= -128 and wi.max() <= 127
    bias = env[conv["inputs"][2]].astype(np.float32) if len(conv["inputs"]) > 2 else None
    # signed operands: a uint8 activation with its top bit flipped is xq - 128, its zero point zx - 128
    if xq.dtype == np.uint8:
        xs, zxs = (xq ^ 0x80).view(np.int8).astype(np.int64), zx - 128
    else:
        xs, zxs = xq.astype(np.int64), zx
    n, c, h, w_ = xs.shape
    _, cg, kh, kw = wi.shape
    g = a.get("group", 1)
    st, dl = a.get("strides", [1, 1]), a.get("dilations", [1, 1])
    pt, pl, pb, pr = R._pads2(a, (kh, kw), (h, w_), st, dl)
    ho = (h + pt + pb - dl[0] * (kh - 1) - 1) // st[0] + 1
    wo = (w_ + pl + pr - dl[1] * (kw - 1) - 1) // st[1] + 1
    xp = np.pad(xs, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=0 if mutant == "pad_zero" else zxs)
    K, mg = cg * kh * kw, M // g
    Kp = -(-K // 64) * 64
    acc = np.zeros((n, M, ho * wo), np.int64)
    for gi in range(g):
        cols = np.stack([xp[:, gi * cg + ci, ky * dl[0]:ky * dl[0] + st[0] * (ho - 1) + 1:st[0],
                            kx * dl[1]:kx * dl[1] + st[1] * (wo - 1) + 1:st[1]].reshape(n, -1)
                         for ci in range(cg) for ky in range(kh) for kx in range(kw)], axis=1)  # [n, K, P], k = (c, ky, kx)
        wg = wi[gi * mg:(gi + 1) * mg].reshape(mg, K)
        wpad = np.zeros((mg, Kp), np.int64)
        wpad[:, :K] = wg
        xpad = np.zeros((n, Kp, ho * wo), np.int64)
        xpad[:, :K] = cols
        if mutant == "kpad_zx":  # the padded k read past the row's end, against zx
            flat = np.concatenate([wg.reshape(-1), np.zeros(Kp, np.int64)])
            wpad = np.stack([flat[m * K:m * K + Kp] for m in range(mg)])
            xpad[:, K:] = zxs
        corr = 0 if mutant == "no_sum_w" else zxs * wg.sum(axis=1)
        acc[:, gi * mg:(gi + 1) * mg] = np.einsum("mk,nkp->nmp", wpad, xpad) - np.reshape(corr, (1, -1, 1))
    mult = (sx * sw).astype(np.float32)
    if mutant == "scale_axis":  # the per-channel scale by the pixel's column instead of the channel
        v = acc.astype(np.float32) * mult[np.arange(ho * wo) % M][None, None, :]
    else:
        v = acc.astype(np.float32) * mult[None, :, None]
    if bias is not None:
        v = v + bias[None, :, None]
    sy = np.float32(env[q["inputs"][1]])
    zy = int(env[q["inputs"][2]]) if len(q["inputs"]) > 2 else 0
    yt = env[q["inputs"][2]].dtype.type if len(q["inputs"]) > 2 else np.uint8
    relu_after = mutant == "relu_after" and act is not None and act["op"] == "Relu"
    if act is not None and not relu_after:
        if act["op"] == "Relu":
            v = np.maximum(v, np.float32(0))
        else:
            lo = env[act["inputs"][1]] if len(act["inputs"]) > 1 and act["inputs"][1] else act["attrs"].get("min", -np.inf)
            hi = env[act["inputs"][2]] if len(act["inputs"]) > 2 and act["inputs"][2] else act["attrs"].get("max", np.inf)
            v = np.clip(v, np.float32(lo), np.float32(hi))
    t = (v / sy).astype(np.float32)
    r = (np.sign(t) * np.floor(np.abs(t) + np.float32(0.5))) if mutant == "half_away" else np.rint(t)
    r = r + np.float32(zy)
    if relu_after:
        r = np.maximum(r, 0)
    lo, hi = QC.RANGE[np.int8 if (yt is np.uint8) == (mutant == "wrong_range") else np.uint8]
    return np.clip(r, lo, hi).astype(np.int64).reshape(n, M, ho, wo)


def _restated_failures(cs, mutant=None):
    _, _, outs, model, env = _model(cs.family)
    o = outs[cs.name][0]
    y = restate(model, env, o, mutant)
    return QC.quantised_failures(o, y, env[o], RQ.unrounded(model, env, o), QC.META[cs.name]["weighting"] == "dyadic")


@pytest.mark.parametrize("name", [k.name for k in SINGLE])
def test_integer_restatement_meets_the_rules(name):
    assert not _restated_failures(QC.BY_NAME[name])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_leave_the_rules(mutant):
    """Each classic error breaks the rules in at least one case of each weighting (the rounding mode shows at
    exact ties alone, which only the dyadic weighting has)."""
    for group in (QC.DYADIC,) if mutant == "half_away" else (QC.DYADIC, QC.GENERAL):
        caught = [k.name for k in SINGLE if k in group and _restated_failures(k, mutant)]
        print(f"{mutant}: caught by {len(caught)} cases, e.g. {caught[:3]}")
        assert caught, mutant
