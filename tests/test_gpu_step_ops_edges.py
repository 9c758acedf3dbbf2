"""eg3d_adam_step around the boundaries of its 16-byte form (csrc/noise_ops.hip: a thread owns four consecutive elements and moves them as one
16-byte access where every base of the leaf is 16-byte aligned and the four lie inside it, as 4-byte accesses otherwise), against the float64
restatement and bounds of tests/support/step_ref.py:

  * leaves of 1, 3, 4, 5, 4095, 4096 and 4097 elements (the quad that straddles the end of a leaf, the 4096-element chunk);
  * the same leaves as views whose base is 4 bytes off a 16-byte boundary -- the parameter, the gradients and the moments each on their own, and all;
  * a renormalised 512^2 map together with a 4^2 one, aligned and not.
Under the deterministic build (EG3D_DETERMINISTIC=1) the renormalised maps are also bit-identical from run to run.  Every case prints its worst err / tol.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import step_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
SIZES = (1, 3, 4, 5, 4095, 4096, 4097)
KINDS = ('g', 'g2', 'both')
OFF = {'aligned': (), 'parameter': ('p',), 'gradients': ('g', 'g2'), 'moments': ('m', 'v'), 'all': ('p', 'g', 'g2', 'm', 'v')}


def _place(a, shape, off):
    """fp32 array -> device tensor of `shape` whose first element lies 4 bytes past a 16-byte boundary when `off`."""
    store = torch.zeros(a.size + 4, device=DEV)
    assert store.data_ptr() % 16 == 0
    t = store[1:1 + a.size] if off else store[:a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    t = t.view(shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if off else 0)
    return t


def _step(leaves, t0, lr, off, seed):
    """leaves: [(shape, kind, slices)].  One HipAdam step from arbitrary fp32 state; returns the worst err / tol per quantity and the new parameters."""
    from inv3d_amd import hipops
    params, extra, norm, host = [], {}, {}, []
    for i, (shape, kind, slices) in enumerate(leaves):
        n = int(np.prod(shape))
        p, g, g2, m, v = R.adam_state(n, 1000 * seed + i, **(dict(gmag=(1e-3, 1.0), mean=1.0) if slices else {}))
        host.append((p, g, g2, m, v))
        q = _place(p, shape, 'p' in off).requires_grad_(True)
        if kind in ('g', 'both'):
            q.grad = _place(g, shape, 'g' in off)
        if kind in ('g2', 'both'):
            extra[q] = _place(g2, shape, 'g2' in off)
        if slices:
            norm[q] = slices
        params.append(q)
    opt = hipops.HipAdam(params, lr=float(lr))
    opt.step_t.fill_(float(t0))
    for q, (shape, _, _), h in zip(params, leaves, host):
        opt.state[q]['exp_avg'] = _place(h[3], shape, 'm' in off)
        opt.state[q]['exp_avg_sq'] = _place(h[4], shape, 'v' in off)
    opt.step(extra_grads=extra, normalize=norm)
    torch.cuda.synchronize()
    assert float(opt.step_t) == t0 + 1.0
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
    for q, (shape, kind, slices), (p, g, g2, m, v) in zip(params, leaves, host):
        rp, rm, rv, tp, tm, tv = R.adam_ref(p, g if kind in ('g', 'both') else None, g2 if kind in ('g2', 'both') else None, m, v, t0, lr, tol=True)
        got = lambda t: t.detach().cpu().numpy().reshape(-1)          # noqa: E731
        worst['m'] = max(worst['m'], R.compare(got(opt.state[q]['exp_avg']), rm, tm)[1])
        worst['v'] = max(worst['v'], R.compare(got(opt.state[q]['exp_avg_sq']), rv, tv)[1])
        if not slices:
            worst['p'] = max(worst['p'], R.compare(got(q), rp, tp)[1])
        else:
            per = rp.size // slices
            for s in range(slices):
                ref, tol = R.adam_norm_ref(rp[s * per:(s + 1) * per], tp[s * per:(s + 1) * per])
                worst['norm'] = max(worst['norm'], R.compare(got(q)[s * per:(s + 1) * per], ref, tol)[1])
    return worst, [q.detach().clone() for q in params]


def _report(name, worst):
    from inv3d_amd import _lib as L
    print(f'Adam edges {name}: worst err/tol p {worst["p"]:.4f} m {worst["m"]:.4f} v {worst["v"]:.4f} renormalised {worst["norm"]:.4f}'
          + (' (deterministic build)' if L.DETERMINISTIC else ''))
    assert max(worst.values()) <= 1.0, (name, worst)
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


@pytest.mark.parametrize('t0', [0, 999])
@pytest.mark.parametrize('where', list(OFF))
def test_adam_leaves_around_the_quad_and_the_chunk(where, t0):
    leaves = [((n,), k, 0) for n in SIZES for k in KINDS]          # 21 items: one launch
    worst, _ = _step(leaves, t0, 0.1, OFF[where], seed=t0 % 5 + len(where))
    _report(f'{where}, t {t0}', worst)


@pytest.mark.parametrize('where', ['aligned', 'parameter', 'all'])
def test_adam_renormalised_512_map_with_a_4_map(where):
    from inv3d_amd import _lib as L
    leaves = [((1, 1, 512, 512), 'both', 1), ((1, 1, 4, 4), 'both', 1), ((2, 1, 4, 4), 'g2', 2)]
    worst, new = _step(leaves, 7, 3e-4, OFF[where], seed=11)
    _report(f'512^2 with 4^2, {where}', worst)
    if L.DETERMINISTIC:
        _, again = _step(leaves, 7, 3e-4, OFF[where], seed=11)
        assert all(torch.equal(a, b) for a, b in zip(new, again)), 'two runs differ under the deterministic build'


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_step_ops_edges.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
