"""The four kernels of csrc/torgb_small.hip on their own -- torgb_small_kernel<4 | 8>, the twelve instances of torgb_mid_kernel, torgb_small_bwd_kernel and
torgb_mid_bwd_kernel, called through hipops.torgb_small / torgb_small_bwd -- against the float64 restatement and the derived bounds of
tests/support/torgb_ref.py (checked without a GPU in tests/test_torgb_cpu.py).  The layer tests pass whether the kernel or the implicit GEMM ran and compare
at 2e-5 / 1e-4 of the largest entry; here every listed case must be launched (the wrappers' return values and the library's own family predicates are
asserted against the restated launch arithmetic), every output is compared element by element, the outputs start as NaN with a NaN guard band of one tile
behind them, and the inputs must come back bit-unchanged.

  * forward, small: one pixel .. 135 blocks, NW = 4 and 8, one to three batches per wave, full and half-resolution addend (N = 3, ragged tile), w_row > C;
  * forward with `pre`: the producing layer's epilogue inside the launch -- x, max|x| (onto a start of zero, below and above) and out, and out bit-identical
    to PendingEpilogue.run() followed by the plain launch;
  * forward, mid: all twelve <KS, ADD, FILL> instances, tiles that straddle a row, two images, two iterations with a partly valid last one for both KS;
  * backward, small and mid: plain, add_scale, add_scale + add_ds, act_on; empty wave shares, 127 tiles, exactly 4096 pixels, two iterations per wave;
  * refusals through the wrappers; the same file once more in a fresh interpreter under the deterministic build.
Every case prints its worst err / tol."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import torgb_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
NAN = float('nan')


def _det():
    from inv3d_amd import _lib as L
    return L.DETERMINISTIC


def _no_misses():
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _cl(a, H, W):
    """[N, HW, C] or [N, H, W, C] numpy -> [N, C, H, W] channels_last on the device."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.reshape(a.shape[0], H, W, a.shape[-1])).to(DEV).permute(0, 3, 1, 2)


def _nhwc(t):
    n, c, h, w = t.shape
    return _np(t.permute(0, 2, 3, 1)).reshape(n, h * w, c)


def _guarded(N, C, H, W):
    """A NaN-filled channels_last [N, C, H, W] with a NaN guard band of one tile (32 pixels) behind it: (buffer, tensor, elements of the tensor)."""
    n = N * H * W * C
    buf = torch.full((n + R.TS_PIX * C,), NAN, device=DEV)
    return buf, buf[:n].view(N, H, W, C).permute(0, 3, 1, 2), n


def _guard_intact(g):
    return bool(torch.isnan(g[0][g[2]:]).all())


def _untouched(g):
    return bool(torch.isnan(g[0]).all())


def _same(t, a, H, W):
    return np.array_equal(_nhwc(t), np.asarray(a).reshape(a.shape[0], H * W, a.shape[-1]))


def _report(name, pairs):
    res = [(k, *R.compare(got, ref, tol)) for k, got, ref, tol in pairs]
    print(f'{name}: worst err/tol ' + ', '.join(f'{k} {r:.4f}' for k, _, r in res) + (' (deterministic build)' if _det() else ''))
    bad = [(k, r) for k, ok, r in res if not ok]
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------------ forward
def _pending(case, x, z, xout, amax):
    from inv3d_amd import hipops as H
    p, (act, _, _, noise, _, _) = x['pre'], case.pre
    shared = noise == 'shared'
    nz = None if p['noise'] is None else _dev(p['noise'].reshape(-1) if shared else p['noise'])
    return H.PendingEpilogue(z, xout, _dev(p['d']), amax, noise=nz, noise_nstride=0 if shared or nz is None else case.HW,
                             noise_strength=None if nz is None else torch.tensor(R.STRENGTH, dtype=torch.float32, device=DEV), bias=_dev(p['bias']), act=act,
                             alpha=R.ALPHA if act == 'lrelu' else 0.0, gain=p['gain'], clamp=p['clamp'])


def _fwd_operands(case, x):
    N, C, Hh, Ww, Cp = case.geom
    wbuf = _dev(x['wbuf'])
    add = _cl(x['addend'], Hh, Ww) if case.add == 'full' else (_cl(x['addend'], Hh // 2, Ww // 2) if case.add == 'half' else None)
    return dict(wbuf=wbuf, wf=wbuf[:, :C], s=_dev(x['s']), bias=_dev(x['bias']), add=add, taps=R.TAPS if case.add == 'half' else None)


def _mid_fwd_supported(xin, o, out):
    from inv3d_amd import _lib as L
    import ctypes as C
    n, c, h, w = xin.shape
    p = L.TorgbSmallParams(x=xin.data_ptr(), w=o['wf'].data_ptr(), s=o['s'].data_ptr(), bias=L.ptr(o['bias']), addend=L.ptr(o['add']), out=out.data_ptr(), N=n, H=h, W=w, C=c,
                           Cp=out.shape[1], ldx=c, ldo=out.shape[1], w_row=o['wf'].stride(0), addend_up2=1 if o['taps'] is not None else 0, clamp=-1.0)
    return bool(L.lib().eg3d_torgb_mid_supported(C.byref(p)))


@pytest.mark.parametrize('case', R.FWD_CASES, ids=lambda c: c.id)
def test_forward(case):
    from inv3d_amd import hipops as H
    x, ref = R.fwd_case_ref(case)
    Lc = ref['launch']
    N, C, Hh, Ww, Cp = case.geom
    o = _fwd_operands(case, x)
    og = _guarded(N, Cp, Hh, Ww)
    src = _cl(x['x'], Hh, Ww)
    xg, pre, amax = None, None, None
    if case.pre is not None:
        xg = _guarded(N, C, Hh, Ww)
        amax = torch.full((1,), ref['amax_start'], dtype=torch.float32, device=DEV)
        pre = _pending(case, x, src, xg[1], amax)
    xin = src if pre is None else xg[1]
    took = H.torgb_small(xin, o['wf'], o['s'], og[1], bias=o['bias'], clamp=x['clamp'], addend=o['add'], addend_up2_taps=o['taps'], pre=pre)
    torch.cuda.synchronize()
    assert took is True, 'the launch was refused'
    assert _mid_fwd_supported(src, o, og[1]) == (Lc['family'] == 'mid' and pre is None), 'the library and the restated launch arithmetic disagree on the family'
    assert _guard_intact(og) and (xg is None or _guard_intact(xg)), 'the guard band behind an output was written'
    assert _same(src, x['x'], Hh, Ww), 'the input was modified'
    if o['add'] is not None:
        assert np.array_equal(_np(o['add'].permute(0, 2, 3, 1)).reshape(x['addend'].shape), x['addend']), 'the addend was modified'
    assert np.array_equal(_np(o['wbuf']), x['wbuf'], equal_nan=True)
    pairs = [('out', _nhwc(og[1]), ref['out'], ref['tol_out'])]
    if pre is not None:
        got_x = _nhwc(xg[1])
        pairs += [('x', got_x, ref['x'], ref['tol_x']), ('x_amax', float(amax), ref['x_amax'], ref['tol_x_amax'])]
    what = f'NW {Lc["NW"]}, batches {max(Lc["batches"])}' if Lc['family'] == 'small' else f'<{Lc["KS"]}, {Lc["ADD"]}, {Lc["FILL"]}>, {Lc["blocks"]} blocks, {Lc["iters"]} iters'
    _report(f'torgb forward {Lc["family"]} {case.id} ({what})', pairs)
    if pre is not None:
        own = np.float32(np.abs(got_x).max())
        assert np.float32(float(amax)) == max(np.float32(ref['amax_start']), own), 'x_amax is not max(start, max|x|) of the x the kernel wrote'
        if case.pre[5] == 'above':
            assert float(amax) == ref['amax_start'], 'a start above the maximum did not survive'
        if case.pre[4]:
            assert (np.abs(got_x) == np.float32(R.CLAMP)).any(), 'the clamp case has no clamped x'
        # the same x from the separate epilogue launch, then the plain launch: the contraction is the same instruction sequence on the same x
        x2, og2, amax2 = _guarded(N, C, Hh, Ww), _guarded(N, Cp, Hh, Ww), torch.zeros(1, device=DEV)
        _pending(case, x, src, x2[1], amax2).run()
        assert H.torgb_small(x2[1], o['wf'], o['s'], og2[1], bias=o['bias'], clamp=x['clamp'], addend=o['add'], addend_up2_taps=o['taps']) is True
        torch.cuda.synchronize()
        assert torch.equal(og[1], og2[1]), 'the merged launch differs from PendingEpilogue.run() + the plain launch'
    if x['clamp'] >= 0 and case.add == 'none':
        assert (np.abs(ref['out']) == R.CLAMP).any(), 'the clamp case has no clamped output'


def test_forward_refusals_leave_the_output_untouched():
    from inv3d_amd import hipops as H
    for (N, C, Hh, Ww, Cp), half in (((1, 32, 5, 4, 96), True), ((1, 24, 4, 4, 96), False), ((1, 32, 4, 4, 48), False)):
        assert R.launch_fwd(N, C, Hh, Ww, Cp, add='half' if half else 'none') is None
        og = _guarded(N, Cp, Hh, Ww)
        xin, wf, s = torch.randn(N, Hh, Ww, C, device=DEV).permute(0, 3, 1, 2), torch.randn(Cp, C, device=DEV), torch.ones(N, C, device=DEV)
        add = torch.randn(N, max(Hh // 2, 1), Ww // 2, Cp, device=DEV).permute(0, 3, 1, 2) if half else None
        assert H.torgb_small(xin, wf, s, og[1], addend=add, addend_up2_taps=R.TAPS if half else None) is False
        torch.cuda.synchronize()
        assert _untouched(og)


# ------------------------------------------------------------------------------------------------------------------ backward
def _bwd_call(case, form, x, start, ref):
    from inv3d_amd import hipops as H, _lib as L
    import ctypes as C
    fm = R.bwd_form(case, form)
    N, Cc, Hh, Ww, Cp = case.geom
    HW = Hh * Ww
    shared = case.noise == 'shared'

    def target(k, shape, want=True):
        if k not in ref or not want:
            return None
        return _dev(np.asarray(start[k], dtype=np.float32).reshape(shape)) if k in start else torch.zeros(shape, device=DEV)

    T = dict(ds=target('ds', (N, Cc), fm['ds']), add_ds=target('add_ds', (N, Cc)), dbias=target('dbias', (Cc,)), dd=target('dd', (N, Cc)),
             dnoise=target('dnoise', (HW,) if shared else (N, HW)), dstrength=target('dstrength', ()))
    wbuf = _dev(x['wbuf'])
    t = dict(dy=_cl(x['dy'], Hh, Ww), wbuf=wbuf, wa=wbuf[:, :Cp], s=_dev(x['s']), xin=_cl(x['xin'], Hh, Ww), add=_cl(x['addend'], Hh, Ww), asc=_dev(x['add_scale']))
    spec = None
    if fm['act']:
        p = x['act']
        nz = None if p['noise'] is None else _dev(p['noise'].reshape(-1) if shared else p['noise'])
        nstride = 0 if shared or nz is None else HW
        spec = H.ActBwdSpec(d=_dev(p['d']), bias=_dev(p['bias']), noise=nz, noise_nstride=nstride, noise_strength=None if nz is None else torch.tensor(R.STRENGTH, dtype=torch.float32, device=DEV),
                            act=case.act, alpha=R.ALPHA if case.act == 'lrelu' else 0.0, gain=p['gain'], clamp=p['clamp'], dbias=T['dbias'], dd=T['dd'], dnoise=T['dnoise'],
                            dnoise_nstride=nstride, dstrength=T['dstrength'])
    dg = _guarded(N, Cc, Hh, Ww)
    amax = torch.zeros(1, device=DEV)
    r = H.torgb_small_bwd(t['dy'], t['wa'], t['s'], t['xin'], dg[1], ds=T['ds'], addend=t['add'], act_bwd=spec, out_amax=amax, addend_scale=t['asc'], addend_ds=T['add_ds'])
    torch.cuda.synchronize()
    assert r is not None, 'the launch was refused'
    assert r is fm['act'], 'the activation backward was not fused' if fm['act'] else r
    q = L.TorgbSmallBwdParams(dy=t['dy'].data_ptr(), wa=t['wa'].data_ptr(), s=t['s'].data_ptr(), xin=t['xin'].data_ptr(), dx=dg[1].data_ptr(), N=N, H=Hh, W=Ww, C=Cc, Cp=Cp,
                              ldg=Cp, ldx=Cc, wa_row=t['wa'].stride(0), act_on=0, no_mid=0)
    assert bool(L.lib().eg3d_torgb_mid_bwd_supported(C.byref(q))) == (ref['launch']['family'] == 'mid'), 'the library and the restated launch arithmetic disagree on the family'
    assert _guard_intact(dg), 'the guard band behind dx was written'
    assert _same(t['dy'], x['dy'], Hh, Ww) and _same(t['xin'], x['xin'], Hh, Ww) and (t['add'] is None or _same(t['add'], x['addend'], Hh, Ww)), 'an input was modified'
    return dg[1], amax, T


@pytest.mark.parametrize('form', R.BWD_FORMS)
@pytest.mark.parametrize('case', R.BWD_CASES, ids=lambda c: c.id)
def test_backward(case, form):
    x, start, ref = R.bwd_case_ref(case, form)
    fm, Lc = R.bwd_form(case, form), ref['launch']
    dx, amax, T = _bwd_call(case, form, x, start, ref)
    pairs = [('dz' if fm['act'] else 'dx', _nhwc(dx), ref['dx'], ref['tol_dx']), ('out_amax', float(amax), ref['amax'], ref['tol_amax'])]
    pairs += [(k, _np(T[k]), ref[k], ref['tol_' + k]) for k in R.BWD_SUMS if T[k] is not None]
    assert (T['ds'] is not None) == fm['ds'] and (T['add_ds'] is not None) == fm['add_ds'] and (T['dbias'] is not None) == fm['act']
    assert (T['dd'] is not None) == (fm['act'] and case.d) and (T['dnoise'] is not None) == (T['dstrength'] is not None) == (fm['act'] and case.noise != 'none')
    what = f'{Lc["tiles"]} tiles, shares {[b - a for a, b in Lc["shares"]]}' if Lc['family'] == 'small' else f'grid {Lc["grid_mid"]}, {Lc["iters"]} iters'
    _report(f'torgb backward {Lc["family"]} {case.id} {form} ({what})', pairs)
    assert float(amax) == float(dx.abs().max()), 'out_amax is not the maximum of the dx the kernel wrote'
    if _det():
        dx2, amax2, T2 = _bwd_call(case, form, x, start, ref)
        assert torch.equal(dx, dx2) and torch.equal(amax, amax2)
        assert all(torch.equal(T[k], T2[k]) for k in T if T[k] is not None), 'two calls differ under the deterministic build'
    _no_misses()


def test_backward_refusals_leave_the_output_untouched():
    from inv3d_amd import hipops as H
    rnd = lambda n, c, h, w: torch.randn(n, h, w, c, device=DEV).permute(0, 3, 1, 2)      # noqa: E731
    # more than 4096 pixels that are no whole number of tiles: neither form takes it
    N, Cc, Hh, Ww, Cp = 1, 32, 129, 33, 96
    assert R.launch_bwd(N, Cc, Hh, Ww, Cp)['wrapper_takes'] is False
    dg, ds = _guarded(N, Cc, Hh, Ww), torch.full((N, Cc), 3.0, device=DEV)
    assert H.torgb_small_bwd(rnd(N, Cp, Hh, Ww), torch.randn(Cc, Cp, device=DEV), torch.ones(N, Cc, device=DEV), rnd(N, Cc, Hh, Ww), dg[1], ds=ds) is None
    torch.cuda.synchronize()
    assert _untouched(dg) and bool((ds == 3.0).all())
    # add_ds without add_scale: the addend would be finished without its scale
    N, Cc, Hh, Ww, Cp = 2, 32, 9, 7, 96
    for spec in (None, H.ActBwdSpec(act='linear', alpha=0.0, gain=1.0, clamp=-1.0, dbias=torch.zeros(Cc, device=DEV))):
        dg, ds, ads = _guarded(N, Cc, Hh, Ww), torch.full((N, Cc), 3.0, device=DEV), torch.full((N, Cc), 5.0, device=DEV)
        r = H.torgb_small_bwd(rnd(N, Cp, Hh, Ww), torch.randn(Cc, Cp, device=DEV), torch.ones(N, Cc, device=DEV), rnd(N, Cc, Hh, Ww), dg[1], ds=ds, addend=rnd(N, Cc, Hh, Ww),
                              act_bwd=spec, addend_ds=ads)
        torch.cuda.synchronize()
        assert r is None and _untouched(dg) and bool((ds == 3.0).all()) and bool((ads == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ deterministic build
def test_deterministic_build_has_no_misses():
    _no_misses()


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_torgb.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
