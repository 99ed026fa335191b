"""The reference of the transformer-block operators and float32 restatements
of their kernels, on the CPU.

* tests/onnx_ref_attn.py (float64 per node, rounded to float32 once per node)
  is held to PyTorch in float64 — torch.nn.functional.layer_norm, gelu,
  torch.erf, and the plain statement softmax(scale Q K^T + bias) V — on every
  value case of tests/op_cases_attn.py, within REF_SHARE of the GPU bar: what
  the reference's own per-node float32 rounding may cost (a LayerNorm13 case
  rounds its mean of 100 to float32, 4e-6 of a unit standard deviation; the
  +-60 logits are rounded at an ulp of 4e-6 to 8e-6 before the exponential).
* a float32 numpy restatement of k_attn's blocked recurrence (32-key blocks,
  running maximum and sum, tail keys at -inf, the bias plane by broadcast
  strides) and of k_layer_norm (mean, then the variance about it) stays within
  HALF the bar of the reference on every fused case;
* mutants of the restatements — what a wrong kernel would compute — leave the
  bar on the cases the table holds for them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import onnx_ref as R
import onnx_ref_attn as RA
import op_cases as OC
import op_cases_attn as AC

TOL = 1e-4
REF_SHARE = 0.25
_refs = {}


def _ref(fam):
    """(feeds, {case: outputs}, the reference's outputs) of a family, once."""
    if fam not in _refs:
        data, feeds, outs = OC.build(AC.groups()[fam])
        _refs[fam] = (feeds, outs, RA.run(R.load(data), feeds))
    return _refs[fam]


def _ratio(got, want):
    """max |got - want| / (TOL max(1, |want|)); inf when anything is not finite."""
    got = np.asarray(got, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / (TOL * np.maximum(1.0, np.abs(want)))).max())


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---- PyTorch in float64 ---------------------------------------------------------------
def _attn_operands(cs, feeds):
    """(q, k as fed, v, bias or None, scale, the Transpose's perm) of an attention case."""
    m = AC.META[cs.name]
    ch = OC.chain_operands(cs, feeds)
    pick = lambda kp: ch[kp[0]][kp[1]]
    return (pick(m["q"]), OC.operands(cs, feeds)[0], pick(m["v"]), pick(m["bias"]) if m["bias"] else None, m["scale"],
            cs.attrs["perm"])


def _torch_gelu_family(cs, feeds):
    ops, ch = OC.operands(cs, feeds), OC.chain_operands(cs, feeds)
    n = cs.name
    if cs.op == "Conv":
        pre = F.conv2d(t64(ops[0]), t64(ops[1]), t64(ops[2]))
    elif cs.op == "Gemm":
        pre = t64(ops[0]) @ t64(ops[1])
    elif cs.op == "MatMul":
        pre = t64(ops[0]) @ t64(ops[1]) + t64(ch[0][0])
    elif cs.op == "Concat":
        pre = torch.cat([t64(ops[0]), t64(ops[1])], dim=1)
    else:
        pre = t64(next(o for o in ops if o.ndim == 4))
    if n == "Erf":
        return torch.erf(pre)
    if "near_miss" in n:
        return pre * 0.5 * (1.0 + torch.erf(pre * float(np.float32(0.7))))
    return F.gelu(pre, approximate="tanh" if "tanh" in n else "none")


def _torch_linear(cs, feeds):
    ops, ch = OC.operands(cs, feeds), OC.chain_operands(cs, feeds)
    mm = t64(ops[0]) @ t64(ops[1])
    bias = t64(next(o for o in ch[0] if isinstance(o, np.ndarray)))
    y = mm + bias
    if "relu" in cs.name:
        y = torch.relu(y)
    if "hardswish" in cs.name:
        y = F.hardswish(y)
    if "second_consumer" in cs.name:
        y = mm * y
    return y


def torch_expected(cs, feeds):
    """The case's outputs by PyTorch in float64 (a list, in graph-output order)."""
    if cs.family in (AC.L, AC.LD):
        m = AC.META[cs.name]
        x = t64(OC.operands(cs, feeds)[0])
        ns = m["nshape"]
        g = None if m["gamma"] is None else t64(np.broadcast_to(m["gamma"], ns).copy())
        b = None if m["beta"] is None else t64(np.broadcast_to(m["beta"], ns).copy())
        return [F.layer_norm(x, ns, g, b, m["eps"])]
    if cs.family == AC.G:
        return [_torch_gelu_family(cs, feeds)]
    if cs.family == AC.LI:
        return [_torch_linear(cs, feeds)]
    q, k, v, bias, scale, perm = _attn_operands(cs, feeds)
    s = (t64(q) @ t64(k).permute(*perm)) * scale
    if bias is not None:
        s = s + t64(bias)
    p = torch.softmax(s, dim=-1)
    return ([p] if cs.n_out == 2 else []) + [p @ t64(v)]


@pytest.mark.parametrize("name", [k.name for k in AC.VALUE_CASES])
def test_reference_matches_torch_float64(name):
    cs = AC.BY_NAME[name]
    feeds, outs, ref = _ref(cs.family)
    want = torch_expected(cs, feeds)
    assert len(want) == len(outs[name])
    for o, w in zip(outs[name], want):
        r = _ratio(ref[o], w.numpy())
        print(f"{o}: reference against PyTorch float64, err / bar {r:.4f}")
        assert r <= REF_SHARE, (o, r)


# ---- float32 restatements -------------------------------------------------------------
def layer_norm_f32(x, nshape, gamma, beta, eps, mutant=None):
    """k_layer_norm in float32: the mean, then the variance about it over the same row."""
    f = np.float32
    d = int(np.prod(nshape))
    rows = x.astype(f).reshape(-1, d)
    inv_d = f(1.0) / f(d)
    mean = rows.sum(axis=1, keepdims=True, dtype=f) * inv_d
    c = rows - mean
    if mutant == "one_pass":
        var = (rows * rows).sum(axis=1, keepdims=True, dtype=f) * inv_d - mean * mean
    else:
        var = (c * c).sum(axis=1, keepdims=True, dtype=f) * inv_d
    if mutant == "eps_outside":
        rstd = f(1.0) / (np.sqrt(var) + f(eps))
    else:
        rstd = f(1.0) / np.sqrt(var + f(eps))
    y = c * rstd
    if gamma is not None:
        y = y * np.broadcast_to(gamma, nshape).reshape(1, d).astype(f)
    if beta is not None:
        y = y + np.broadcast_to(beta, nshape).reshape(1, d).astype(f)
    return y.reshape(x.shape)


def attn_f32(q, k, v, bias, scale, mutant=None, block=32):
    """k_attn in float32: per slice of the leading dims, the keys in blocks of `block`, the running maximum m
    and sum l, the output accumulators scaled by exp(m_old - m_new), one division by l at the end."""
    f = np.float32
    lead = q.shape[:-2]
    bh, nq, nk, dv = int(np.prod(lead)), q.shape[-2], k.shape[-2], v.shape[-1]
    q2, k2, v2 = (a.astype(f).reshape((bh,) + a.shape[-2:]) for a in (q, k, v))
    out = np.zeros((bh, nq, dv), f)
    if bias is not None:
        planes = bias.astype(f).reshape((-1, nq, nk))
        blead = (1,) * (len(lead) - (bias.ndim - 2)) + bias.shape[:-2]
    for b in range(bh):
        bp = None
        if bias is not None:
            if mutant == "bias_no_broadcast":
                bp = planes[min(b, len(planes) - 1)]
            else:  # the plane by broadcast strides over the unravelled slice index
                idx = np.unravel_index(b, lead)
                bp = planes[int(np.ravel_multi_index([i if n > 1 else 0 for i, n in zip(idx, blead)], blead))]
        m = np.full((nq, 1), -np.inf, f)
        l = np.zeros((nq, 1), f)
        o = np.zeros((nq, dv), f)
        for j0 in range(0, nk, block):
            kb = np.zeros((block, k2.shape[-1]), f)
            vb = np.zeros((block, dv), f)
            n = min(block, nk - j0)
            kb[:n], vb[:n] = k2[b, j0:j0 + n], v2[b, j0:j0 + n]
            s = q2[b] @ kb.T
            if mutant != "no_scale":
                s = s * f(scale)
            if bp is not None:
                s = s + bp[:, np.minimum(np.arange(j0, j0 + block), nk - 1)]
            if mutant != "tail_unmasked":
                s[:, n:] = -np.inf
            with np.errstate(over="ignore", invalid="ignore"):
                m_new = np.zeros_like(m) if mutant == "no_max" else np.maximum(m, s.max(axis=1, keepdims=True))
                alpha = np.exp(m - m_new)
                p = np.exp(s - m_new)
                if mutant == "no_rescale":
                    l = l + p.sum(axis=1, keepdims=True, dtype=f)
                else:
                    l = l * alpha + p.sum(axis=1, keepdims=True, dtype=f)
                o = o * alpha + p @ vb
            m = m_new
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = o / l
    return out.reshape(lead + (nq, dv))


def _ln_f32(cs, feeds, mutant=None):
    m = AC.META[cs.name]
    return layer_norm_f32(OC.operands(cs, feeds)[0], m["nshape"], m["gamma"], m["beta"], m["eps"], mutant)


def _attn_f32(cs, feeds, mutant=None):
    q, k, v, bias, scale, _ = _attn_operands(cs, feeds)
    return attn_f32(q, k, v, bias, scale, mutant)


@pytest.mark.parametrize("name", [k.name for k in AC.LNORM_CASES])
def test_layer_norm_restatement_within_half_the_bar(name):
    cs = AC.BY_NAME[name]
    feeds, outs, ref = _ref(cs.family)
    r = _ratio(_ln_f32(cs, feeds), ref[outs[name][0]])
    print(f"{name}: float32 restatement, err / bar {r:.4f}")
    assert r <= 0.5, r


@pytest.mark.parametrize("name", [k.name for k in AC.FUSED_ATTN])
def test_attention_restatement_within_half_the_bar(name):
    cs = AC.BY_NAME[name]
    feeds, outs, ref = _ref(cs.family)
    r = _ratio(_attn_f32(cs, feeds), ref[outs[name][-1]])
    print(f"{name}: float32 restatement, err / bar {r:.4f}")
    assert r <= 0.5, r


def test_off100_rows_need_the_two_step_variance():
    """Rows of mean 100 and standard deviation 1: the float64 reference meets the bar against PyTorch, the
    two-step float32 restatement meets half of it, and a one-pass E[x^2] - mean^2 in float32 does not meet it."""
    cases = [k for k in AC.LNORM_CASES if "off100" in k.name]
    assert len(cases) >= 3
    for cs in cases:
        feeds, outs, ref = _ref(cs.family)
        want = ref[outs[cs.name][0]]
        assert _ratio(want, torch_expected(cs, feeds)[0].numpy()) <= 1.0
        assert _ratio(_ln_f32(cs, feeds), want) <= 0.5
        r = _ratio(_ln_f32(cs, feeds, "one_pass"), want)
        print(f"{cs.name}: one-pass variance, err / bar {r:.1f}")
        assert r > 1.0, (cs.name, r)


# mutant: the cases (at least) on which it must leave the bar
LN_MUTANTS = {"one_pass": ["LayerNorm_D256_off100", "LayerNorm_D1000_off100", "LayerNorm_D4100_off100",
                           "LayerNorm13_pow_scalar_gamma_off100_D256"],
              "eps_outside": ["LayerNorm_D160_eps1e-3_small"]}
ATTN_MUTANTS = {"no_max": ["Attn_q70_k145_d32_logits60"],
                "tail_unmasked": ["Attn_q15_k7_d20_div", "Attn_q17_k33_d32_dv20_on_k", "Attn_q70_k145_d128",
                                  "Attn_q17_k1_d20_logits60_on_q"],
                "no_rescale": ["Attn_q70_k145_d128", "Attn_q70_k145_d32_logits60"],
                "no_scale": ["Attn_q15_k7_d20_div", "Attn_q17_k16_d32_on_q", "Attn_q17_k33_d32_dv20_on_k",
                             "Attn_q70_k145_d128"],
                "bias_no_broadcast": ["Attn_q15_k145_d32_const_bias", "Attn_q70_k7_d8_runtime_bias"]}


@pytest.mark.parametrize("mutant", sorted(LN_MUTANTS) + sorted(ATTN_MUTANTS))
def test_mutant_leaves_the_bar(mutant):
    table, fn = (LN_MUTANTS, _ln_f32) if mutant in LN_MUTANTS else (ATTN_MUTANTS, _attn_f32)
    for name in table[mutant]:
        cs = AC.BY_NAME[name]
        feeds, outs, ref = _ref(cs.family)
        r = _ratio(fn(cs, feeds, mutant), ref[outs[name][-1]])
        print(f"{mutant} on {name}: err / bar {r:.1f}")
        assert r > 1.0, (mutant, name, r)
