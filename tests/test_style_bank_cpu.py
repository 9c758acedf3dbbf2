"""tests/support/style_ref.py without a GPU: the float64 restatement of the style bank agrees with a plain torch.float64 autograd of the same
expressions, an fp32-rounded model of the kernels passes its bounds, and each of six wrong kernels misses them by at least 5 x on every case it
can show in -- so the bounds tests/test_gpu_style_bank.py holds the kernels to are not vacuous."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import style_ref as R      # noqa: E402


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_reference_agrees_with_float64_autograd(case):
    """F1 .. F5 of the header from one autograd graph: styles and d forward; with upstream gradients dout (of the styles) and dd (of d), the gradient
    of the latent is F4 (whose dout_extra is F3) and those of the affine weights and biases are F5."""
    ws = _t(case['ws'], True)
    loss, params, outs = 0.0, [], []
    for ly in case['layers']:
        W, b = _t(ly['W'], True), _t(ly['b'], True)
        wg, bg, po = (float(np.float32(ly[k])) for k in ('wgain', 'bgain', 'post'))
        s = (ws[:, ly['wrow'], :] @ (W * wg).t() + b * bg) * po
        d = None
        if ly['wsq'] is not None:
            d = torch.rsqrt(s.square() @ _t(ly['wsq']).t() + float(np.float32(1e-8)))
        if ly['dout'] is not None:
            loss = loss + (s * _t(ly['dout'])).sum()
        if ly['dd'] is not None:
            loss = loss + (d * _t(ly['dd'])).sum() + (s * _t(ly['e0'])).sum()          # (a starting value of dout_extra is one more gradient of the styles)
        params.append((W, b))
        outs.append((s, d))
    loss.backward()
    es = []
    for ly, (s, d) in zip(case['layers'], outs):
        ref, _ = R.affine_fwd_ref(case['ws'], ly['W'], ly['b'], ly['wrow'], ly['wgain'], ly['bgain'], ly['post'])
        np.testing.assert_allclose(ref, s.detach().numpy(), rtol=1e-12, atol=1e-12)
        e = None
        if ly['wsq'] is not None:
            ref, _ = R.demod_fwd_ref(s.detach().numpy(), ly['wsq'])
            np.testing.assert_allclose(ref, d.detach().numpy(), rtol=1e-12, atol=1e-12)
        if ly['dd'] is not None:
            e, _ = R.demod_bwd_ref(s.detach().numpy(), d.detach().numpy(), ly['dd'], ly['wsq'], ly['e0'])
        es.append(e)
    ref, _ = R.affine_bwd_ref(case, es, np.zeros_like(case['dws0']))
    np.testing.assert_allclose(ref, ws.grad.numpy(), rtol=1e-10, atol=1e-10)
    for ly, e, (W, b) in zip(case['layers'], es, params):
        if ly['dout'] is None and e is None:
            continue
        rW, _, rb, _ = R.wgrad_ref(case, ly, e)
        np.testing.assert_allclose(rW, W.grad.numpy(), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(rb, b.grad.numpy(), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_bounds_accept_the_model_and_reject_every_mutant(case):
    worst = R.check(case, R.model(case))
    assert max(worst.values()) <= 1.0, worst
    for m in R.MUTANTS:
        if not R.applies(case, m):
            continue
        w = max(R.check(case, R.model(case, m)).values())
        assert w >= 5.0, (case['name'], m, w)


def test_every_mutant_and_every_required_size_is_exercised():
    cs = R.cases()
    for m in R.MUTANTS:
        assert sum(R.applies(c, m) for c in cs) >= 10, m
    assert {c['D'] for c in cs} >= {4, 260, 512, 516} and {c['N'] for c in cs} == {1, 2, 3} and {c['L'] for c in cs} >= {1, 14}
    Cs = {ly['C'] for c in cs for ly in c['layers']}
    Cos = {ly['Co'] for c in cs for ly in c['layers'] if ly['Co'] is not None}
    assert set(R.FWD_TILE_C + R.BWD_TILE_C + R.ALWAYS_C + R.DEMOD_C + R.DEMOD_K) <= Cs and set(R.OSPLIT_CO + R.TILE_CO) <= Cos
    assert {len(c['layers']) for c in cs} >= {1, 3, 26, R.STYLE_BANK_MAX}
    assert all(len(c['layers']) <= R.STYLE_BANK_MAX for c in cs)
