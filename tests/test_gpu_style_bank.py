"""The style bank of csrc/style_affine.hip on its own -- eg3d_style_affine_fwd / _bwd through hipops.style_affine, nothing else -- against the float64
restatement and the derived elementwise bounds of tests/support/style_ref.py (checked without a GPU in tests/test_style_bank_cpu.py).

Every case of style_ref.cases(): D 4 / 260 / 512 (and 516), N 1 / 2 / 3, L 1 / 14; C and Co at every tile edge of the kernels and at the osplit boundaries;
demodulated C 63 / 64 / 65 and around the k chunks; banks of 1, 3, 26 and STYLE_BANK_MAX layers that mix conv layers and toRGB-like ones; layers that
share a latent row; dout only, dout_extra only and both; dws and dout_extra that start from non-zero values; and dws = None with dweights / dbiases
(the Phase B path).  The same file once more in a fresh interpreter under the deterministic build, where it also asserts run-to-run bit identity and
det_misses() == 0.  Every case prints its worst err / tol.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import style_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _det():
    from inv3d_amd import _lib as L
    return L.DETERMINISTIC


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _run(case):
    """One forward, one backward into non-zero dws / dout_extra, one Phase B backward (dws = None): the `got` dict of style_ref.check."""
    from inv3d_amd import hipops
    N = case['N']
    lys = case['layers']
    ws = _dev(case['ws'])
    layers = [(_dev(ly['W']), _dev(ly['b']), ly['wrow'], ly['wgain'], ly['bgain'], ly['post']) for ly in lys]
    wsq = [_dev(ly['wsq']) for ly in lys]
    outs = [torch.full((N, ly['C']), float('nan'), device=DEV) for ly in lys]
    d = [torch.full((N, ly['Co']), float('nan'), device=DEV) if ly['wsq'] is not None else None for ly in lys]
    hipops.style_affine(ws, layers, outs=outs, demod=[(q, a, None, None) if q is not None else None for q, a in zip(wsq, d)])
    douts, dd = [_dev(ly['dout']) for ly in lys], [_dev(ly['dd']) for ly in lys]

    def demod(e):
        return [(q, a, g, x) if q is not None else None for q, a, g, x in zip(wsq, d, dd, e)]
    e = [_dev(ly['e0']) for ly in lys]
    dws = _dev(case['dws0'])
    hipops.style_affine(ws, layers, outs=outs, douts=douts, dws=dws, demod=demod(e), backward=True)
    eB = [_dev(ly['e0']) for ly in lys]
    has = [ly['dout'] is not None or ly['dd'] is not None for ly in lys]
    dW = [torch.full_like(l[0], float('nan')) if h else None for l, h in zip(layers, has)]
    db = [torch.full_like(l[1], float('nan')) if h else None for l, h in zip(layers, has)]
    hipops.style_affine(ws, layers, outs=outs, douts=douts, dws=None, demod=demod(eB), backward=True, dweights=dW, dbiases=db)
    torch.cuda.synchronize()
    assert torch.equal(ws, _dev(case['ws'])), 'the latent was modified'
    conv = lambda xs: [_np(x) for x in xs]          # noqa: E731
    return dict(s=conv(outs), d=conv(d), e=conv(e), eB=conv(eB), dW=conv(dW), db=conv(db), dws=_np(dws))


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_style_bank_forward_backward_and_phase_b(case):
    from inv3d_amd import _lib as L
    got = _run(case)
    worst = R.check(case, got, det=_det())
    print(f'style bank {case["name"]}: worst err/tol ' + ' '.join(f'{k} {v:.4f}' for k, v in worst.items()) + (' (deterministic build)' if _det() else ''))
    assert max(worst.values()) <= 1.0, (case['name'], worst)
    if _det():
        again = _run(case)
        for k in ('e', 'eB', 'dws', 's', 'd', 'dW', 'db'):
            a, b = got[k], again[k]
            same = np.array_equal(a, b) if k == 'dws' else all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))
            assert same, f'two runs differ in {k} under the deterministic build'
        assert L.det_misses() == 0


def test_deterministic_build_has_no_misses():
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_style_bank.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
