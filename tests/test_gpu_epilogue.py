"""The kernels of csrc/epilogue.hip on their own -- the layer epilogue forward (all four code paths and the strip form), the activation backward in its
three incoming-gradient forms (eg3d_modconv_epilogue_bwd, eg3d_dgrad_finish_act, eg3d_torgb_dgrad_act), eg3d_dgrad_finish, eg3d_weight_sqsum,
eg3d_demod_fwd / _bwd, eg3d_weight_grad_finish (slabs, batched) and eg3d_unpack_weight_grad -- against the float64 restatement and the derived bounds of
tests/support/epilogue_ref.py (checked without a GPU in tests/test_epilogue_cpu.py).  The layer and loop tests compare at 1e-4 of the largest entry and
up, on white-noise cotangents; a lane, a tail pixel or one block's share dropped from a reduction stays below that.

  * activation backward: every launch-shape class (C = 4 ... 1024, idle threads, a pixel wider than a wave, one pixel, one full trip, two trips with a
    ragged last one), lrelu / linear / relu, clamp with outputs exactly at the clamp, noise none / shared / per image, null d and bias, accumulation
    onto non-zero targets, max|dz|;
  * the demodulation and weight-gradient kernels at sizes off every tile, slabs with NaN between them, Ip > I with NaN padding;
  * the same file once more in a fresh interpreter under the deterministic build, where every atomically accumulated output is also bit-identical over
    two calls and det_misses() == 0.
Every case prints its worst err / tol."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import epilogue_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
EG3D_ERR_UNSUPPORTED = -2


def _det():
    from inv3d_amd import _lib as L
    return L.DETERMINISTIC


def _tag():
    return ' (deterministic build)' if _det() else ''


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


def _nhwc(t, flat=True):
    n, c, h, w = t.shape
    a = _np(t.permute(0, 2, 3, 1))
    return a.reshape(n, h * w, c) if flat else a


def _report(name, pairs):
    """pairs: [(output, got, ref, tol)].  Prints the worst err / tol of each and asserts all of them."""
    res = [(k, *R.compare(got, ref, tol)) for k, got, ref, tol in pairs]
    print(f'{name}: worst err/tol ' + ', '.join(f'{k} {r:.4f}' for k, _, r in res) + _tag())
    bad = [(k, r) for k, ok, r in res if not ok]
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------------ activation backward
def _act_call(case, form, x, start, ref):
    from inv3d_amd import hipops as H
    N, HW, Cc, Hh, Ww = case.N, case.HW, case.C, case.H, case.W
    kw = R.act_settings(case, form)
    act = case.act_of(form)
    shared = case.noise == 'shared'

    def target(k, shape):
        if k not in ref:
            return None
        return _dev(np.asarray(start[k], dtype=np.float32).reshape(shape)) if k in start else torch.zeros(shape, device=DEV)

    T = dict(dbias=target('dbias', (Cc,)), dd=target('dd', (N, Cc)), dnoise=target('dnoise', (HW,) if shared else (N, HW)), dstrength=target('dstrength', ()),
             ds=target('ds', (N, Cc)))
    out_d, d_d, b_d = _cl(x['out'], Hh, Ww), _dev(x['d']), _dev(x['bias'])
    nz_d = None if x['noise'] is None else _dev(x['noise'].reshape(-1) if shared else x['noise'])
    st_d = None if x['noise'] is None else torch.tensor(R.STRENGTH, dtype=torch.float32, device=DEV)
    nstride = 0 if shared or x['noise'] is None else HW
    dz = H.empty_cl(N, Cc, Hh, Ww, DEV).fill_(float('nan'))
    amax = torch.zeros(1, device=DEV)
    common = dict(d=d_d, noise=nz_d, noise_nstride=nstride, noise_strength=st_d, bias=b_d, act=act, alpha=R.ALPHA if act == 'lrelu' else 0.0, gain=kw['gain'],
                  clamp=kw['clamp'], dbias=T['dbias'], dd=T['dd'], dnoise=T['dnoise'], dnoise_nstride=nstride, dstrength=T['dstrength'])
    if form == 'plain':
        H.epilogue_bwd(_cl(x['dout'], Hh, Ww), out_d, dz, dz_amax=amax, **common)
    else:
        spec = H.ActBwdSpec(**common)
        s_d, add_d = _dev(x['s']), _cl(x['addend'], Hh, Ww)
        if form == 'finish':
            H.dgrad_finish_act(_cl(x['z'], Hh, Ww), out_d, s_d, dz, spec, ds=T['ds'], addend=add_d, dz_amax=amax)
        else:
            H.torgb_dgrad_act(_cl(x['dy4'], Hh, Ww), _dev(x['wa4']), out_d, s_d, dz, spec, ds=T['ds'], addend=add_d, dz_amax=amax)
    torch.cuda.synchronize()
    assert np.array_equal(_nhwc(out_d), x['out']), 'the saved output was modified'
    return dz, amax, T


@pytest.mark.parametrize('form', R.ACT_FORMS)
@pytest.mark.parametrize('case', R.ACT_CASES, ids=lambda c: c.id)
def test_activation_backward(case, form):
    x, start, ref = R.act_case_ref(case, form)
    dz, amax, T = _act_call(case, form, x, start, ref)
    pairs = [('dz', _nhwc(dz), ref['dz'], ref['tol_dz']), ('max|dz|', float(amax), ref['dz_amax'], ref['tol_dz_amax'])]
    pairs += [(k, _np(T[k]), ref[k], ref['tol_' + k]) for k in ('dbias', 'dd', 'dnoise', 'dstrength', 'ds') if k in ref]
    L = ref['launch']
    _report(f'activation backward {form} {case.id} {case.act_of(form)} (ppb {L["ppb"]}, {L["bx"]} blocks, {L["trips"]} trips)', pairs)
    assert (T['dd'] is None) == ('dd' not in ref) and (T['ds'] is None) == (form == 'plain')
    if _det():
        dz2, amax2, T2 = _act_call(case, form, x, start, ref)
        assert torch.equal(dz, dz2) and torch.equal(amax, amax2)
        assert all(torch.equal(T[k], T2[k]) for k in T if T[k] is not None), 'two calls differ under the deterministic build'
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ dgrad_finish
@pytest.mark.parametrize('case', R.FINISH_CASES, ids=str)
def test_dgrad_finish(case):
    from inv3d_amd import hipops as H
    Cc, N, Hh, Ww, with_ds, with_s, with_add = case
    x = R.finish_inputs(case)
    ref = R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], x['start'])

    def call():
        dx, ds = H.empty_cl(N, Cc, Hh, Ww, DEV).fill_(float('nan')), _dev(x['start'])
        H.dgrad_finish(_cl(x['z'], Hh, Ww), _cl(x['x'], Hh, Ww), _dev(x['s']), dx, ds=ds, addend=_cl(x['addend'], Hh, Ww))
        torch.cuda.synchronize()
        return dx, ds
    dx, ds = call()
    pairs = [('dx', _nhwc(dx), ref['dx'], ref['tol_dx'])] + ([('ds', _np(ds), ref['ds'], ref['tol_ds'])] if with_ds else [])
    _report(f'dgrad_finish {case}', pairs)
    if _det() and with_ds:
        assert torch.equal(ds, call()[1]), 'two calls differ under the deterministic build'
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ demodulation
@pytest.mark.parametrize('case', R.DEMOD_CASES, ids=str)
def test_demodulation_forward_and_backward(case):
    from inv3d_amd import hipops as H
    x = R.small_inputs('demod', case)
    d_ref, tol_d = R.demod_fwd_ref(x['s'], x['wsq'])
    s_d, wsq_d, dd_d = _dev(x['s']), _dev(x['wsq']), _dev(x['dd'])
    d = H.demod_fwd(s_d, wsq_d)
    d32 = d_ref.astype(np.float32)                      # the backward's own input: the rounded reference, so that its bound carries no forward error
    ds_ref, tol_ds, dwsq_ref, tol_dwsq = R.demod_bwd_ref(x['s'], x['wsq'], d32, x['dd'], x['start_ds'], x['start_dwsq'])

    def call():
        ds, dwsq = _dev(x['start_ds']), _dev(x['start_dwsq'])
        H.demod_bwd(s_d, wsq_d, _dev(d32), dd_d, ds=ds, dwsq=dwsq)
        torch.cuda.synchronize()
        return ds, dwsq
    ds, dwsq = call()
    _report(f'demodulation Co {case[0]} Ck {case[1]} N {case[2]}', [('d', _np(d), d_ref, tol_d), ('ds', _np(ds), ds_ref, tol_ds), ('dwsq', _np(dwsq), dwsq_ref, tol_dwsq)])
    only = _dev(x['start_ds'])
    H.demod_bwd(s_d, wsq_d, _dev(d32), dd_d, ds=only)                    # dwsq null: ds alone
    assert R.compare(_np(only), ds_ref, tol_ds)[0]
    if _det():
        again = call()
        assert torch.equal(ds, again[0]) and torch.equal(dwsq, again[1]), 'two calls differ under the deterministic build'
    _no_misses()


@pytest.mark.parametrize('case', R.SQSUM_CASES, ids=str)
def test_weight_sqsum(case):
    from inv3d_amd import hipops as H
    Co, Ck, T = case
    wp = R.small_inputs('sqsum', case)['wp']
    ref, tol = R.weight_sqsum_ref(wp)
    _report(f'weight_sqsum {case}', [('wsq', _np(H.weight_sqsum(_dev(wp), Co, T, Ck)), ref, tol)])


# ------------------------------------------------------------------------------------------------------------------ weight_grad_finish
def _wgf_single(x, case):
    """One launch through the C ABI (slabs with their own stride)."""
    from inv3d_amd import _lib as L
    O, I, T, N, with_dd, nslab, gap = case
    t = dict(buf=_dev(x['buf']), w=_dev(x['w']), s=_dev(x['s']), d=_dev(x['d']), dd=_dev(x['dd']), dw=torch.full((O, I, T), float('nan'), device=DEV))
    L.check(L.lib().eg3d_weight_grad_finish_slabs(L.ptr(t['buf']), nslab, x['stride'], L.ptr(t['w']), L.ptr(t['s']), L.ptr(t['d']), L.ptr(t['dd']), L.ptr(t['dw']), N, O, I, T,
                                                  L.stream_ptr()), 'weight_grad_finish_slabs')
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize('case', R.WGF_CASES, ids=str)
def test_weight_grad_finish(case):
    from inv3d_amd import hipops as H
    O, I, T, N, with_dd, nslab, gap = case
    x = R.small_inputs('wgf', case)
    ref, tol = R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'])
    t = _wgf_single(x, case)
    pairs = [('dw', _np(t['dw']), ref, tol)]
    if nslab == 1 and T in (1, 4, 9):                   # the wrapper, with the parameter's own [O, I, kh, kw] shape
        k = {1: 1, 4: 2, 9: 3}[T]
        dw = H.weight_grad_finish(_dev(x['slabs'][0]), t['w'].reshape(O, I, k, k), t['s'], t['d'], t['dd'])
        if dw is not None:
            pairs.append(('dw through hipops', _np(dw).reshape(O, I, T), ref, tol))
    _report(f'weight_grad_finish {case}', pairs)


def test_weight_grad_finish_batched_equals_the_single_launches():
    from inv3d_amd import _lib as L
    cases = [R.WGF_CASES[i] for i in R.WGF_BATCH]
    xs = [R.small_inputs('wgf', c) for c in cases]
    singles = [_wgf_single(x, c) for x, c in zip(xs, cases)]
    arr = (L.WgfItem * len(cases))()
    outs = []
    for it, x, c, t in zip(arr, xs, cases, singles):
        O, I, T, N, with_dd, nslab, gap = c
        dw = torch.full((O, I, T), float('nan'), device=DEV)
        outs.append(dw)
        it.g, it.w, it.s, it.d, it.dd, it.dw = t['buf'].data_ptr(), t['w'].data_ptr(), t['s'].data_ptr(), t['d'].data_ptr(), t['dd'].data_ptr() if with_dd else None, dw.data_ptr()
        it.slab_stride, it.N, it.O, it.I, it.T, it.nslab = x['stride'], N, O, I, T, nslab
    L.check(L.lib().eg3d_weight_grad_finish_batched(arr, len(cases), L.stream_ptr()), 'weight_grad_finish_batched')
    torch.cuda.synchronize()
    pairs = []
    for x, c, t, dw in zip(xs, cases, singles, outs):
        ref, tol = R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'])
        pairs.append((f'item {c[:4]}', _np(dw), ref, tol))
        assert torch.equal(dw, t['dw']), f'the batched launch differs from the single launch of {c}'
    _report('weight_grad_finish batched', pairs)


def test_weight_grad_finish_refuses_a_row_beyond_the_lds_limit():
    """I = 2048 with nine taps needs (T (I + 1) + I) floats = 80 KB of LDS: a host check, nothing is launched."""
    from inv3d_amd import _lib as L
    O, I, T, N = R.WGF_TOO_LARGE
    g, w, dw = (torch.zeros(O * T * I, device=DEV) for _ in range(3))
    rc = L.lib().eg3d_weight_grad_finish(L.ptr(g), L.ptr(w), None, None, None, L.ptr(dw), N, O, I, T, L.stream_ptr())
    assert rc == EG3D_ERR_UNSUPPORTED, rc
    item = (L.WgfItem * 1)()
    item[0].g, item[0].w, item[0].dw, item[0].N, item[0].O, item[0].I, item[0].T, item[0].nslab = g.data_ptr(), w.data_ptr(), dw.data_ptr(), N, O, I, T, 1
    assert L.lib().eg3d_weight_grad_finish_batched(item, 1, L.stream_ptr()) == EG3D_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ unpack_weight_grad
@pytest.mark.parametrize('case', R.UNPACK_CASES, ids=str)
def test_unpack_weight_grad(case):
    from inv3d_amd import _lib as L
    O, I, Ip, T, with_a, with_da = case
    x = R.small_inputs('unpack', case)
    dw_ref, tol_dw, da_ref, tol_da = R.unpack_weight_grad_ref(x['g'], x['w'], x['a'], Ip)
    g, w, a = _dev(x['g']), _dev(x['w']), _dev(x['a'])
    dw, da = torch.full((O, I, T), float('nan'), device=DEV), torch.full((O,), 7.0, device=DEV) if with_da else None
    L.check(L.lib().eg3d_unpack_weight_grad(L.ptr(g), L.ptr(w), L.ptr(a), L.ptr(dw), L.ptr(da), O, I, Ip, T, L.stream_ptr()), 'unpack_weight_grad')
    torch.cuda.synchronize()
    _report(f'unpack_weight_grad {case}', [('dw', _np(dw), dw_ref, tol_dw)] + ([('da', _np(da), da_ref, tol_da)] if with_da else []))


# ------------------------------------------------------------------------------------------------------------------ forward
def _forward(case, strip=False):
    from inv3d_amd import hipops as H
    name, N, Cc, Hh, Ww, kind, pad0, noise, clamp, act = case
    x, kw = R.fwd_inputs(case)
    ref, tol, amax_ref, tol_amax = R.fwd_ref(x['z'], fir=x['fir'], d=x['d'], noise=x['noise'], bias=x['bias'], **kw)
    hz, wz = x['z'].shape[1:3]
    z = _cl(x['z'], hz, wz)
    out, amax = H.empty_cl(N, Cc, Hh, Ww, DEV).fill_(float('nan')), torch.zeros(1, device=DEV)
    shared = noise == 'shared'
    args = dict(pad0=pad0, fir_gain=kw['fir_gain'], d=_dev(x['d']), noise=None if x['noise'] is None else _dev(x['noise'][0] if shared else x['noise']),
                noise_nstride=0 if shared or x['noise'] is None else Hh * Ww, noise_strength=None if x['noise'] is None else torch.tensor(R.STRENGTH, dtype=torch.float32, device=DEV),
                bias=_dev(x['bias']), act=act, alpha=R.ALPHA if act == 'lrelu' else 0.0, gain=kw['gain'], clamp=kw['clamp'], out_amax=amax)
    if strip:
        assert H.upconv_epilogue_fwd(z, out, **args) is None
    else:
        H.epilogue_fwd(z, out, fir=_dev(x['fir']), **args)
    torch.cuda.synchronize()
    _report(f'forward {"strip " if strip else ""}{name} {N}x{Cc}x{Hh}x{Ww}', [('out', _nhwc(out, flat=False), ref, tol), ('max|out|', float(amax), amax_ref, tol_amax)])
    if kw['clamp'] >= 0:
        assert float(amax) <= R.CLAMP and (np.abs(ref) == R.CLAMP).any(), 'the clamp case has no clamped output'


@pytest.mark.parametrize('case', R.FWD_CASES, ids=lambda c: c[0])
def test_epilogue_forward(case):
    _forward(case)


def test_upconv_epilogue_forward_strip_against_float64():
    _forward(R.UPCONV_CASE, strip=True)
    _forward(R.UPCONV_CASE)                 # the same case on the 2 x 2-block kernel


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
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_epilogue.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
