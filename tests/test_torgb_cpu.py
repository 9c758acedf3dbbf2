"""The yardstick of tests/test_gpu_torgb.py, checked without a GPU: tests/support/torgb_ref.py equals torch autograd in float64 on the reference expressions
(networks_stylegan2.py:338-359, 433-436; upfirdn2d.upsample2d) to 1e-12; its case lists reach every launch class of csrc/torgb_small.hip by the restated
launch arithmetic; its comparisons reject fourteen kinds of wrong result, each in at least half of the outputs it touches by five tolerances or more, in every
listed case where the mutant applies; and the bounds accept the same operations evaluated in fp32 numpy in the kernels' own order (shares, trees, column sums)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import torgb_ref as R      # noqa: E402

MARGIN = 5.0
T64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))      # noqa: E731
f32 = np.float32


def _eq(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    scale = float(np.abs(b).max())
    assert scale > 0, what
    assert float(np.abs(a - b).max()) <= 1e-12 * scale, (what, float(np.abs(a - b).max()) / scale)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def _up2_torch(low):
    """upfirdn2d(low [N, C, h, w], f = outer([1, 3, 3, 1]) / 64, up=2, padding=[2, 1, 2, 1], gain=4): zeros inserted, padded, a true convolution."""
    N, C, h, w = low.shape
    up = torch.zeros(N, C, 2 * h, 2 * w, dtype=low.dtype)
    up[:, :, ::2, ::2] = low
    f1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=low.dtype) / 8
    k = torch.flip(torch.outer(f1, f1) * 4, (0, 1))
    return F.conv2d(F.pad(up, (2, 1, 2, 1)), k[None, None].repeat(C, 1, 1, 1), groups=C)


@pytest.mark.parametrize('hw', [(2, 2), (4, 6), (6, 10), (2, 8)])
def test_upsampled_addend_equals_upfirdn2d(hw):
    rng = np.random.default_rng(2)
    H, W = hw
    low = rng.standard_normal((3, H // 2, W // 2, 5))
    val, mag = R.up2_ref(low, H, W)
    want = _up2_torch(T64(low).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(3, H * W, 5)
    _eq(val, want.numpy(), 'up-sampled addend')
    assert (mag >= np.abs(val) - 1e-15).all()
    assert sum(R.TAPS[1::2]) == 1.0 and sum(R.TAPS[0::2]) == 1.0


def _pre_torch(z, d, noise, strength, bias, slope, gain, clamp):
    v = z
    if d is not None:
        v = v * d[:, None, :]
    if noise is not None:
        v = v + (noise * strength)[:, :, None]
    if bias is not None:
        v = v + bias[None, None, :]
    v = torch.where(v > 0, v, v * slope) * gain
    return v.clamp(-clamp, clamp) if clamp >= 0 else v


@pytest.mark.parametrize('geom,add', [((2, 32, 3, 5, 32), 'none'), ((3, 40, 4, 6, 64), 'half'), ((1, 72, 6, 6, 32), 'full')])
@pytest.mark.parametrize('pre', [None, ('lrelu', 'image', 1.2), ('linear', 'shared', -1.0), ('relu', 'none', 1.2)])
def test_forward_and_pre_equal_torch(geom, add, pre):
    rng = np.random.default_rng(5)
    N, C, H, W, Cp = geom
    HW = H * W
    L = R.launch_fwd(*geom, add=add, pre=pre is not None)
    x, s, w, bias = rng.standard_normal((N, HW, C)), 0.75 + 0.5 * rng.random((N, C)), rng.standard_normal((Cp, C)) / np.sqrt(C), 0.3 * rng.standard_normal(Cp)
    addend = None if add == 'none' else rng.standard_normal((N, HW, Cp) if add == 'full' else (N, H // 2, W // 2, Cp))
    tx = T64(x)
    if pre is not None:
        act, noise, clamp = pre
        d, pb = 0.5 + rng.random((N, C)), 0.1 * rng.standard_normal(C)
        nz = None if noise == 'none' else rng.standard_normal((1 if noise == 'shared' else N, HW))
        xr, _, amax, _ = R.pre_ref(x, L, d=d, noise=nz, strength=0.37, bias=pb, slope=R.SLOPES[act], gain=R.GAIN, clamp=clamp)
        tx = _pre_torch(T64(x), T64(d), None if nz is None else T64(nz), float(f32(0.37)), T64(pb), R.SLOPES[act], R.GAIN, clamp)
        _eq(xr, tx.numpy(), 'x')
        assert amax == float(tx.abs().max())
        assert R.pre_ref(x, L, d=d, noise=nz, strength=0.37, bias=pb, slope=R.SLOPES[act], gain=R.GAIN, clamp=clamp, start=amax + 1)[2] == amax + 1
        x = xr
    out = R.fwd_ref(x, s, w, L, H, W, bias=bias, clamp=1.2, addend=addend, add=add)['out']
    y = ((tx * T64(s)[:, None, :]) @ T64(w).T + T64(bias)).clamp(-1.2, 1.2)
    if add == 'full':
        y = y + T64(addend)
    elif add == 'half':
        y = y + _up2_torch(T64(addend).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(N, HW, Cp)
    _eq(out, y.numpy(), 'out')
    assert add != 'none' or (np.abs(out) == 1.2).any()


@pytest.mark.parametrize('form', ['plain', 'scale', 'scale_ds', 'act_lrelu_clamp_shared', 'act_linear_image', 'act_lrelu_none'])
@pytest.mark.parametrize('geom', [(2, 32, 3, 5, 8), (3, 64, 4, 6, 96)])
def test_backward_equals_autograd(geom, form):
    """dx and ds are the gradients of sum(out dy) of the forward with respect to x and s; add_scale / add_ds those of the pass-through term; with act the
    cotangent g meets the producing layer's forward (as tests/test_epilogue_cpu.py does for the activation backward's own forms)."""
    rng = np.random.default_rng(6)
    N, C, H, W, Cp = geom
    HW = H * W
    L = R.launch_bwd(*geom)
    dy, w, s = rng.standard_normal((N, HW, Cp)), rng.standard_normal((Cp, C)), 0.75 + 0.5 * rng.random((N, C))
    addend, asc = rng.standard_normal((N, HW, C)), (0.75 + 0.5 * rng.random((N, C)) if form != 'plain' else None)
    ts = T64(s).requires_grad_(True)
    tas = T64(asc if asc is not None else np.ones((N, C))).requires_grad_(True)
    g_t = (T64(dy) @ T64(w)) * ts[:, None, :] + T64(addend) * tas[:, None, :]
    if not form.startswith('act'):
        xin = rng.standard_normal((N, HW, C))
        r = R.bwd_ref(dy, w.T.copy(), s, xin, L, addend=addend, add_scale=asc, add_ds=form == 'scale_ds')
        tx = T64(xin).requires_grad_(True)
        y = (tx * ts[:, None, :]) @ T64(w).T                       # the forward of the same layer: its adjoint is the data gradient
        gx, gs = torch.autograd.grad((y * T64(dy)).sum(), [tx, ts])
        _eq(r['dx'], (gx + T64(addend) * tas[:, None, :]).detach().numpy(), 'dx')
        _eq(r['ds'], gs.numpy(), 'ds')
        gs2, gas = torch.autograd.grad((g_t * T64(xin)).sum(), [ts, tas])
        _eq(r['ds'], gs2.numpy(), 'ds as the gradient of the finishing pass')
        if form == 'scale_ds':
            _eq(r['add_ds'], gas.numpy(), 'add_ds')
        assert r['amax'] == float(np.abs(r['dx']).max())
        return
    _, act, *rest = form.split('_')
    clamp, noise = (1.2, rest[1]) if rest[0] == 'clamp' else (-1.0, rest[0])
    z, d, bias = rng.standard_normal((N, HW, C)), 0.5 + rng.random((N, C)), 0.1 * rng.standard_normal(C)
    nz = None if noise == 'none' else rng.standard_normal((1 if noise == 'shared' else N, HW))
    kw = dict(d=d, noise=nz, strength=0.37, bias=bias, slope=R.SLOPES[act], gain=R.GAIN, clamp=clamp)
    out = R.pre_ref(z, None, **kw)[0]
    leaves = [T64(a).requires_grad_(True) for a in (z, d, bias)]
    tn = None if nz is None else T64(nz).requires_grad_(True)
    tst = torch.tensor(float(f32(0.37)), dtype=torch.float64, requires_grad=True)
    to = _pre_torch(leaves[0], leaves[1], tn, tst, leaves[2], R.SLOPES[act], R.GAIN, clamp)
    r = R.bwd_ref(dy, w.T.copy(), s, out, L, addend=addend, add_scale=asc, add_ds=True, act=kw)
    want = leaves + ([tn, tst] if tn is not None else [])
    grads = torch.autograd.grad((to * g_t.detach()).sum(), want)
    _eq(r['dx'], grads[0].numpy(), 'dz')
    _eq(r['dd'], grads[1].numpy(), 'dd')
    _eq(r['dbias'], grads[2].numpy(), 'dbias')
    if tn is not None:
        _eq(r['dnoise'], grads[3].numpy(), 'dnoise')
        _eq(r['dstrength'], grads[4].numpy(), 'dstrength')
    gs, gas = torch.autograd.grad((g_t * T64(out)).sum(), [ts, tas])
    _eq(r['ds'], gs.numpy(), 'ds')
    _eq(r['add_ds'], gas.numpy(), 'add_ds')


# ------------------------------------------------------------------------------------------------------------------ case classes
def test_the_listed_cases_reach_every_launch_class():
    reached = {}
    for c in R.FWD_CASES:
        for k in R.classes('fwd', *c.geom, add=c.add, pre=c.pre is not None):
            reached.setdefault(k, []).append(c.id)
    missing = set(R.FWD_CLASSES) - set(reached)
    assert not missing, missing
    for c in R.BWD_CASES:
        for k in R.classes('bwd', *c.geom):
            reached.setdefault(k, []).append(c.id)
    missing = set(R.BWD_CLASSES) - set(reached)
    assert not missing, missing
    print('\n'.join(f'{k}: {len(v)} case(s)' for k, v in sorted(reached.items())))
    # the cases the issue names, with the launch values it states
    L = lambda *g, **kw: R.launch_fwd(*g, **kw)      # noqa: E731
    assert L(1, 32, 1, 1, 32)['shares'] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert [b - a for a, b in L(2, 40, 9, 7, 96)['shares']] == [1, 1, 1, 2]
    g = L(1, 264, 4, 4, 96)
    assert g['NW'] == 8 and sorted({b - a for a, b in g['shares']}) == [4, 5]
    g = L(1, 520, 4, 4, 96)
    assert g['NW'] == 8 and g['batches'] == [1] * 7 + [2] and g['shares'][-1] == (56, 65)
    g = L(1, 520, 40, 36, 96, add='half')
    assert g['NW'] == 4 and g['grid'] == (45, 3) and [b - a for a, b in g['shares']] == [16, 16, 16, 17] and max(g['batches']) == 3
    g = L(1, 256, 128, 132, 96)
    assert (g['KS'], g['T'], g['blocks'], g['iters'], g['valid_last'], g['FILL']) == (2, 528, 256, 2, 16, 24)
    g = L(2, 160, 130, 128, 96)
    assert (g['KS'], g['T'], g['blocks'], g['iters'], g['valid_last'], g['nb']) == (1, 1040, 256, 2, 16, 15)
    for geom in R.TWO_ITERS:
        assert sum(c.geom[:4] == geom for c in R.FWD_MID) == 3
    assert L(1, 160, 64, 128, 96)['nb'] == 15 and L(1, 32, 64, 128, 96)['per_cu'] >= 2 and L(1, 32, 64, 128, 96)['blocks'] == 64
    # thresholds, from both sides
    assert L(1, 32, 64, 127, 96) is not None and not L(1, 32, 64, 127, 96)['mid'] and L(1, 32, 64, 128, 96)['mid']
    assert L(1, 256, 128, 256, 96)['KS'] == 1 and L(1, 256, 128, 252, 96)['KS'] == 2                  # T = 1024 | 1008
    assert L(1, 128, 64, 128, 96)['FILL'] == 12 and L(1, 160, 64, 128, 96)['FILL'] == 24
    assert L(1, 24, 4, 4, 96) is None and L(1, 32, 4, 4, 48) is None and L(1, 32, 3, 4, 96, add='half') is None and L(1, 32, 3, 4, 96, add='full') is not None
    assert L(1, 264, 24, 56, 96)['NW'] == 8 and L(1, 264, 24, 58, 96)['NW'] == 4                       # 126 | 132 blocks
    assert L(1, 256, 4, 4, 96)['NW'] == 4                                                            # 32 groups: one batch per wave of four
    B = R.launch_bwd
    assert B(2, 32, 9, 7, 8)['shares'] == [(0, 0), (0, 0), (0, 0), (0, 1)] and B(2, 32, 9, 7, 8)['wave_iters'] == [0, 0, 0, 1]
    assert B(1, 32, 58, 70, 96)['tiles'] == 127 and not B(1, 32, 58, 70, 96)['mid']
    g = B(1, 64, 64, 64, 96)
    assert g['mid'] and g['grid_mid'] == (32, 2, 1) and g['iters'] == 1 and not B(1, 64, 63, 64, 96)['mid']
    g = B(1, 32, 43, 96, 96)
    assert g['tpi'] == 129 and g['grid_mid'] == (33, 1, 1) and g['wave_iters'][-4:] == [1, 0, 0, 0]
    g = B(3, 256, 43, 96, 96)
    assert g['grid_mid'] == (21, 8, 3) and g['tstep'] == 84 and g['wave_iters'].count(2) == 45 and g['wave_iters'].count(1) == 39
    assert B(1, 32, 129, 33, 96)['wrapper_takes'] is False and B(1, 24, 4, 4, 96) is None
    # the settings
    assert {c.pre[0] for c in R.FWD_PRE} == {'lrelu', 'linear', 'relu'} and {c.pre[3] for c in R.FWD_PRE} == {'none', 'shared', 'image'}
    assert {c.pre[5] for c in R.FWD_PRE} == {'zero', 'below', 'above'} and {(c.pre[1], c.pre[2], c.pre[4]) for c in R.FWD_PRE} >= {(True, True, True), (False, False, False)}
    assert {c.geom for c in R.FWD_PRE} >= {(2, 40, 9, 7, 96), (3, 136, 6, 10, 96), (1, 264, 4, 4, 96)} and any(c.Cp == 32 for c in R.FWD_PRE)
    assert any(c.wpad and c.launch['family'] == 'small' for c in R.FWD_CASES) and any(c.wpad and c.launch['family'] == 'mid' for c in R.FWD_CASES)
    assert all(c.launch['wrapper_takes'] for c in R.FWD_CASES) and all(c.launch['wrapper_takes'] for c in R.BWD_CASES)
    assert {(c.act, c.clamp) for c in R.BWD_CASES} == {('lrelu', True), ('linear', False)} and {c.noise for c in R.BWD_CASES} == {'none', 'shared', 'image'}
    for fam in ('small', 'mid'):
        cs = [c for c in R.BWD_CASES if c.launch['family'] == fam]
        assert {c.noise for c in cs} == {'none', 'shared', 'image'} and {c.act for c in cs} == {'lrelu', 'linear'}
        assert any(not R.bwd_form(c, 'plain')['ds'] for c in cs) and any(R.bwd_form(c, 'act')['add_ds'] for c in cs)
    assert any(not c.start for c in R.BWD_CASES) and any(c.wpad for c in R.BWD_CASES)


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_every_mutant_applies_to_some_listed_case():
    assert {m for c in R.FWD_CASES for m, _ in R.fwd_mutants(c)} == set(R.FWD_MUTANTS)
    assert {m for c in R.FWD_CASES for m, must in R.fwd_mutants(c) if must} == set(R.FWD_MUTANTS), 'a mutant that is never required to touch an output'
    assert {m for c in R.BWD_CASES for f in R.BWD_FORMS for m in R.bwd_mutants(c, f)} == set(R.BWD_MUTANTS)
    assert len(set(R.FWD_MUTANTS) | set(R.BWD_MUTANTS)) == 14


def _ratios(mut, ref, tol):
    mut, ref, tol = (np.asarray(a, dtype=np.float64) for a in (mut, ref, tol))
    diff = np.abs(np.nan_to_num(mut, nan=np.inf) - ref)
    hit = diff > 0
    return (diff[hit] / np.broadcast_to(tol, diff.shape)[hit]).ravel()


def _fails(name, outs, mut, ref, seen, must_touch=True):
    """The mutant fails the comparison, and by >= MARGIN tolerances in at least half of the outputs it touches (the outputs of one mutant pooled)."""
    r = np.concatenate([_ratios(mut[k], ref[k], ref['tol_' + k]) for k in outs])
    if r.size == 0:
        assert not must_touch, f'{name}: {outs} not touched'
        return
    m = float(np.median(r))
    assert r.max() > 1.0 and not all(R.compare(mut[k], ref[k], ref['tol_' + k])[0] for k in outs), (name, outs)
    assert m >= MARGIN, f'{name}: {outs} fails by a median of only {m:.2f} tolerances'
    seen[name] = m


@pytest.mark.parametrize('case', R.FWD_CASES, ids=lambda c: c.id)
def test_forward_mutants_fail_with_margin(case):
    x, ref = R.fwd_case_ref(case)
    assert np.isfinite(ref['out']).all() and (case.wpad == 0 or np.isnan(x['wbuf'][:, case.C:]).all())
    seen = {}
    for mutant, must in R.fwd_mutants(case):
        mut = R.fwd_eval(case, x, mutant=mutant)
        outs = ['x_amax'] if mutant == 'amax_missing_wave' else (['out', 'x', 'x_amax'] if mutant == 'noise_without_strength' else ['out'])
        _fails(mutant, outs, mut, ref, seen, must)
    assert 'last_group_dropped' in seen
    print(f'{case.id}: ' + ', '.join(f'{k} {v:.0f}' for k, v in seen.items()))


@pytest.mark.parametrize('form', R.BWD_FORMS)
@pytest.mark.parametrize('case', R.BWD_CASES, ids=lambda c: c.id)
def test_backward_mutants_fail_with_margin(case, form):
    x, start, ref = R.bwd_case_ref(case, form)
    sums = [k for k in R.BWD_SUMS if k in ref]
    seen = {}
    for mutant in R.bwd_mutants(case, form):
        mut = R.bwd_eval(case, form, x, start, mutant=mutant)
        if mutant in ('last_row_dropped', 'second_iteration_dropped'):
            _fails(mutant, [k for k in sums if k != 'dnoise'], mut, ref, seen)
            for k in ('ds', 'add_ds', 'dd'):
                if k in ref:
                    _fails(mutant + ' ' + k, [k], mut, ref, seen)
        elif mutant == 'add_ds_scaled':
            _fails(mutant, ['add_ds'], mut, ref, seen)
        else:
            _fails(mutant, ['dx'], mut, ref, seen)
            _fails(mutant + ' sums', [k for k in sums if k != 'add_ds'] + ['amax'], mut, ref, seen)
    if start:
        mut = R.bwd_eval(case, form, x, None)
        for k in sums:
            _fails('overwrite ' + k, [k], mut, ref, seen)
    print(f'{case.id} {form}: ' + ', '.join(f'{k} {v:.0f}' for k, v in seen.items()))


# ------------------------------------------------------------------------------------------------------------------ honesty of the bounds
def _seq(a, axis):
    return np.take(np.cumsum(a, axis=axis, dtype=f32), -1, axis=axis)


def _chain(a, w, shares):
    """a [P, K], w [O, K] fp32 -> each share's partial tile [P, O]: the 8-channel groups one after the other, fp32 throughout."""
    parts = []
    for g0, g1 in shares:
        acc = np.zeros((a.shape[0], w.shape[0]), dtype=f32)
        for g in range(g0, g1):
            acc = acc + a[:, 8 * g:8 * g + 8] @ w[:, 8 * g:8 * g + 8].T
        parts.append(acc)
    return parts


def _tree4(p):
    return (p[0] + p[1]) + (p[2] + p[3])


def _up2_f32(low, H, W):
    t = [f32(v) for v in R.TAPS]
    lp = np.pad(low, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y, x = np.arange(H), np.arange(W)
    r, c = (y >> 1) + (y & 1), (x >> 1) + (x & 1)
    wy0, wy1 = np.where(y & 1, t[2], t[3])[None, :, None, None], np.where(y & 1, t[0], t[1])[None, :, None, None]
    wx0, wx1 = np.where(x & 1, t[2], t[3])[None, None, :, None], np.where(x & 1, t[0], t[1])[None, None, :, None]
    A, B, Cc, D = lp[:, r][:, :, c], lp[:, r][:, :, c + 1], lp[:, r + 1][:, :, c], lp[:, r + 1][:, :, c + 1]
    v = wy0 * (wx0 * A + wx1 * B) + wy1 * (wx0 * Cc + wx1 * D)
    assert v.dtype == f32
    return v.reshape(low.shape[0], H * W, -1)


@pytest.mark.parametrize('case', R.FWD_CASES, ids=lambda c: c.id)
def test_fp32_numpy_forward_stays_under_the_bounds(case):
    x, ref = R.fwd_case_ref(case)
    L = ref['launch']
    N, C, H, W, Cp = case.geom
    xin, res = x['x'], []
    if case.pre is not None:
        p = x['pre']
        v = xin * p['d'][:, None, :] if p['d'] is not None else xin
        if p['noise'] is not None:
            v = v + (p['noise'] * f32(p['strength']))[:, :, None]
        if p['bias'] is not None:
            v = v + p['bias']
        v = np.where(v > 0, v, v * f32(p['slope'])) * f32(p['gain'])
        xin = np.clip(v, -f32(p['clamp']), f32(p['clamp'])) if p['clamp'] >= 0 else v
        assert xin.dtype == f32
        res += [('x', R.compare(xin, ref['x'], ref['tol_x'])), ('x_amax', R.compare(max(f32(ref['amax_start']), np.abs(xin).max()), ref['x_amax'], ref['tol_x_amax']))]
    a = (xin * x['s'][:, None, :]).reshape(-1, C)
    parts = _chain(a, np.ascontiguousarray(x['w']), L['shares'])
    if L['family'] == 'small':
        v = _tree4(parts[:4]) if L['NW'] == 4 else _tree4(parts[:4]) + _tree4(parts[4:])
    else:
        v = parts[0] + parts[1] if L['KS'] == 2 else parts[0]
    v = v.reshape(N, H * W, Cp)
    if x['bias'] is not None:
        v = v + x['bias']
    if x['clamp'] >= 0:
        v = np.clip(v, -f32(x['clamp']), f32(x['clamp']))
    if case.add == 'full':
        v = v + x['addend']
    elif case.add == 'half':
        v = v + _up2_f32(x['addend'], H, W)
    assert v.dtype == f32
    res.append(('out', R.compare(v, ref['out'], ref['tol_out'])))
    print(f'fp32 numpy {case.id}: worst err/tol ' + ', '.join(f'{k} {r:.3f}' for k, (_, r) in res))
    assert all(ok for _, (ok, _) in res), res


def _colsum(terms, L):
    """terms [N, HW, K] fp32 -> the blocks' partial column sums [N, blocks per plane, K] in the kernels' shape (header B of torgb_ref)."""
    N, HW, K = terms.shape
    if L['family'] == 'small':
        pad = np.zeros((N, L['tiles'] * 32, K), dtype=f32)
        pad[:, :HW] = terms
        return _seq(pad.reshape(N, L['tiles'], 32, K), 2)
    ts, it = L['tstep'], L['iters']
    pad = np.zeros((N, it * ts * 32, K), dtype=f32)
    pad[:, :HW] = terms
    v = pad.reshape(N, it, ts, 4, 8, K).transpose(0, 2, 1, 3, 4, 5).reshape(N, ts, it * 4, 8, K)           # pixel row = er0 + 8 k
    v = _seq(v, 2)
    v = ((v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])) + ((v[:, :, 4] + v[:, :, 5]) + (v[:, :, 6] + v[:, :, 7]))
    v = v.reshape(N, ts // 4, 4, K)
    return (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])


def _onto(start, parts, axis=1):
    """The partial sums added one after the other onto the start value."""
    st = np.broadcast_to(np.asarray(start, dtype=f32), np.delete(parts.shape, axis))
    return _seq(np.concatenate([np.expand_dims(st, axis), parts], axis), axis)


@pytest.mark.parametrize('form', R.BWD_FORMS)
@pytest.mark.parametrize('case', R.BWD_CASES, ids=lambda c: c.id)
def test_fp32_numpy_backward_stays_under_the_bounds(case, form):
    x, start, ref = R.bwd_case_ref(case, form)
    fm, L = R.bwd_form(case, form), ref['launch']
    N, C, H, W, Cp = case.geom
    HW = H * W
    st = lambda k: start[k] if k in start else f32(0)          # noqa: E731
    parts = _chain(x['dy'].reshape(-1, Cp), np.ascontiguousarray(x['wa']), L['shares'])
    zz = (_tree4(parts) if L['family'] == 'small' else parts[0]).reshape(N, HW, C)
    xin = x['xin']
    got = dict(ds=_onto(st('ds'), _colsum(zz * xin, L)))
    a = x['addend'] if x['addend'] is not None else np.zeros((1, 1, 1), dtype=f32)
    if fm['add_ds']:
        got['add_ds'] = _onto(st('add_ds'), _colsum(a * xin, L))
    a_s = a * x['add_scale'][:, None, :] if x['add_scale'] is not None else a
    g = zz * x['s'][:, None, :] + a_s
    if x['act'] is None:
        got['dx'] = g
    else:
        p = x['act']
        gain, slope, strength = f32(p['gain']), f32(p['slope']), f32(p['strength'])
        yy = xin * (f32(1) / gain)
        pos = yy > 0
        dyv = g * gain * np.where(pos, f32(1), slope)
        if p['clamp'] >= 0:
            dyv = np.where(np.abs(xin) >= f32(p['clamp']), f32(0), dyv)
        pre = np.where(pos, yy, yy * (f32(1) / slope))
        dv = p['d'] if p['d'] is not None else np.ones((1, C), dtype=f32)
        b = p['bias'] if p['bias'] is not None else np.zeros(C, dtype=f32)
        nraw = p['noise'] if p['noise'] is not None else np.zeros((1, HW), dtype=f32)
        td = dyv * (pre - b - (nraw * strength)[:, :, None])
        got['dx'] = dyv * dv[:, None, :]
        got['dbias'] = _onto(st('dbias'), _colsum(dyv, L).reshape(-1, C), 0)
        got['dd'] = _onto(st('dd'), _colsum(td, L) / dv[:, None, :])
        if p['noise'] is not None:
            q = dyv.reshape(N, HW, C // 32, 8, 4)
            q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
            cs = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + ((q[..., 4] + q[..., 5]) + (q[..., 6] + q[..., 7]))          # [N, HW, C / 32]
            if case.noise == 'shared':
                got['dnoise'] = _onto(st('dnoise'), (cs * strength).transpose(0, 2, 1).reshape(1, -1, HW))
            else:
                got['dnoise'] = _onto(st('dnoise'), (cs * strength).transpose(0, 2, 1))
            got['dstrength'] = _onto(st('dstrength'), _colsum(cs * nraw[:, :, None], L).reshape(-1), 0)
    assert all(v.dtype == f32 for v in got.values())
    got['amax'] = float(np.abs(got['dx']).max())
    res = [(k, R.compare(got[k], ref[k], ref['tol_' + k])) for k in ('dx', 'amax') + R.BWD_SUMS if k in ref and k in got]
    print(f'fp32 numpy {case.id} {form}: worst err/tol ' + ', '.join(f'{k} {r:.3f}' for k, (_, r) in res))
    assert all(ok for _, (ok, _) in res), res
    assert ('add_ds' in ref) == fm['add_ds'] and ('dd' in ref) == (fm['act'] and case.d) and ('dnoise' in ref) == (fm['act'] and case.noise != 'none')
