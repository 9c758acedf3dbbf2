"""The yardstick of tests/test_gpu_epilogue.py, checked without a GPU: tests/support/epilogue_ref.py equals torch autograd in float64 on the reference
expressions (networks_stylegan2.py:60-66, 89-90, 327-329) to 1e-12; its comparisons reject fifteen kinds of wrong result, each in at least half of the
outputs it touches by five tolerances or more, in every listed case where the mutant applies; the bounds accept the same operations evaluated in fp32
numpy, summed once in the kernel's own shape (lanes, tree, block partials) and once with np.sum; and the listed cases reach every launch-shape class."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import epilogue_ref as R      # noqa: E402

MARGIN = 5.0
T64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))      # noqa: E731


def _eq(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    scale = float(np.abs(b).max())
    assert scale > 0, what
    assert float(np.abs(a - b).max()) <= 1e-12 * scale, (what, float(np.abs(a - b).max()) / scale)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def _fwd_torch(z, fir, pad0, fir_gain, d, noise, strength, bias, slope, gain, clamp):
    """z [N, Hz, Wz, C] -> out [N, H, W, C]: upfirdn2d (flip_filter=False: a true convolution), the demodulation, add_ noise, bias_act."""
    v = z.permute(0, 3, 1, 2)
    C = v.shape[1]
    if fir is not None:
        k = torch.flip(fir, (0, 1)) * fir_gain
        v = F.conv2d(F.pad(v, (pad0, pad0, pad0, pad0)), k[None, None].repeat(C, 1, 1, 1), groups=C)
    if d is not None:
        v = v * d[:, :, None, None]
    if noise is not None:
        v = v + (noise * strength)[:, None]
    if bias is not None:
        v = v + bias[None, :, None, None]
    v = torch.where(v > 0, v, v * slope) * gain
    if clamp >= 0:
        v = v.clamp(-clamp, clamp)
    return v.permute(0, 2, 3, 1)


@pytest.mark.parametrize('form', R.ACT_FORMS)
@pytest.mark.parametrize('act,clamp,noise', [('lrelu', -1.0, 'image'), ('lrelu', 1.2, 'shared'), ('linear', 1.2, 'image'), ('relu', -1.0, 'shared'), ('lrelu', -1.0, 'none')])
def test_forward_and_activation_backward_equal_autograd(act, clamp, noise, form):
    """out = the forward restatement of a float64 z (no filter, so that dz is the gradient of z); the cotangent is the form's incoming gradient, so that
    autograd of sum(out cotangent) with respect to z, d, bias, noise, strength and the consumer's s gives every output of the backward restatement."""
    rng = np.random.default_rng(5)
    N, H, W, C = 3, 5, 4, 8
    slope, gain = R.SLOPES[act], R.GAIN
    z, d, bias = rng.standard_normal((N, H, W, C)), 0.5 + rng.random((N, C)), 0.1 * rng.standard_normal(C)
    nz = None if noise == 'none' else rng.standard_normal((1 if noise == 'shared' else N, H, W))
    strength = 0.37
    out, _, amax, _ = R.fwd_ref(z, d=d, noise=nz, strength=strength, bias=bias, slope=slope, gain=gain, clamp=clamp)
    leaves = [T64(a).requires_grad_(True) for a in (z, d, bias)]
    tn = None if nz is None else T64(nz).requires_grad_(True)
    ts = torch.tensor(float(np.float32(strength)), dtype=torch.float64, requires_grad=True)
    to = _fwd_torch(leaves[0], None, 0, 1.0, leaves[1], tn, ts, leaves[2], slope, gain, clamp)
    _eq(out, to.detach().numpy(), 'forward')
    assert amax == float(to.detach().abs().max())
    s, add = 0.75 + 0.5 * rng.random((N, C)), 0.1 * rng.standard_normal((N, H * W, C))
    tsty = T64(s).requires_grad_(True)
    if form == 'plain':
        G = R.grad_plain(1.0 + 0.5 * rng.standard_normal((N, H * W, C)))
        cot = T64(G['g'])
    elif form == 'finish':
        zc = 1.0 + 0.5 * rng.standard_normal((N, H * W, C))
        G = R.grad_finish(zc, s, add)
        cot = T64(zc) * tsty[:, None, :] + T64(add)
    else:
        dy4, wa4 = rng.standard_normal((N, H * W, 4)), rng.standard_normal((C, 4))
        G = R.grad_torgb(dy4, wa4, s, add)
        cot = (T64(dy4) @ T64(wa4).T) * tsty[:, None, :] + T64(add)
    ref = R.act_bwd_ref(G, out.reshape(N, H * W, C), d=d, bias=bias, noise=None if nz is None else nz.reshape(-1, H * W), strength=strength, slope=slope,
                        gain=gain, clamp=clamp, relu=act == 'relu')
    want = leaves + ([tn, ts] if tn is not None else []) + ([tsty] if form != 'plain' else [])
    grads = list(torch.autograd.grad((to.reshape(N, H * W, C) * cot).sum(), want))
    _eq(ref['dz'], grads[0].numpy(), 'dz')
    _eq(ref['dbias'], grads[2].numpy(), 'dbias')
    assert ('dd' in ref) == (act != 'relu')
    if act != 'relu':
        _eq(ref['dd'], grads[1].numpy(), 'dd')
    if tn is not None:
        _eq(ref['dnoise'], grads[3].numpy(), 'dnoise')
        _eq(ref['dstrength'], grads[4].numpy(), 'dstrength')
    if form != 'plain':
        # (the cotangent depends on s, out does not: d/ds of sum(out cot) is sum_p out z)
        _eq(ref['ds'], grads[-1].numpy(), 'ds')
    assert ref['dz_amax'] == float(np.abs(ref['dz']).max())


@pytest.mark.parametrize('kind,pad0', [('fir44n', 0), ('fir44n', 1), ('fir44n', 2), ('fir32', 0), ('fir32', 1), ('fir32', 2)])
def test_filtered_forward_equals_upfirdn2d_expression(kind, pad0):
    rng = np.random.default_rng(9)
    fir = R.FILTERS[kind].astype(np.float64)
    N, C, hz, wz = 2, 4, 6, 7
    z, d, bias = rng.standard_normal((N, hz, wz, C)), 0.5 + rng.random((N, C)), rng.standard_normal(C)
    out = R.fwd_ref(z, fir=fir, pad0=pad0, fir_gain=4.0, d=d, bias=bias, slope=0.2, gain=R.GAIN)[0]
    to = _fwd_torch(T64(z), T64(fir), pad0, 4.0, T64(d), None, 0.0, T64(bias), 0.2, R.GAIN, -1.0)
    _eq(out, to.numpy(), 'filtered forward')
    assert out.shape == (N, hz + 2 * pad0 - fir.shape[0] + 1, wz + 2 * pad0 - fir.shape[1] + 1, C)


def test_demodulation_and_weight_gradients_equal_autograd():
    """d = rsqrt(sum_i (w s)^2 + 1e-8) through wsq = sum_t w^2;  L = sum(d cot) + sum(G w):  dL/ds, dL/dwsq, dL/dw."""
    rng = np.random.default_rng(3)
    N, O, I, T, nslab = 3, 5, 7, 4, 3
    s, w, cot = 1 + 0.5 * rng.standard_normal((N, I)), rng.standard_normal((O, I, T)) / math.sqrt(I * T), rng.standard_normal((N, O))
    slabs = rng.standard_normal((nslab, O, T * I))
    wp = w.transpose(0, 2, 1)                                            # [O, T, I]
    wsq, _ = R.weight_sqsum_ref(wp)
    d, _ = R.demod_fwd_ref(s, wsq)
    ts, tw = T64(s).requires_grad_(True), T64(w).requires_grad_(True)
    twsq = (tw * tw).sum(2)
    twsq.retain_grad()
    td = ((ts[:, None, :] ** 2 * twsq[None]).sum(2) + R.EPS32).rsqrt()
    td2 = ((tw[None] * ts[:, None, :, None]) ** 2).sum((2, 3)).add(R.EPS32).rsqrt()            # the reference's own order: (w s)^2 summed over i and taps
    _eq(wsq, twsq.detach().numpy(), 'wsq')
    _eq(d, td.detach().numpy(), 'd')
    _eq(d, td2.detach().numpy(), 'd, reference order')
    Gt = T64(slabs.sum(0).reshape(O, T, I).transpose(0, 2, 1).copy())
    ((td * T64(cot)).sum() + (Gt * tw).sum()).backward()
    ds, _, dwsq, _ = R.demod_bwd_ref(s, wsq, d, cot)
    _eq(ds, ts.grad.numpy(), 'ds')
    _eq(dwsq, twsq.grad.numpy(), 'dwsq')
    dw, _ = R.weight_grad_finish_ref(slabs, w, s, d, cot)
    _eq(dw, tw.grad.numpy(), 'dw')
    dw0, _ = R.weight_grad_finish_ref(slabs, w, None, None, None)
    _eq(dw0, Gt.numpy(), 'dw without demodulation')


def test_unpack_weight_grad_and_dgrad_finish_equal_autograd():
    rng = np.random.default_rng(4)
    O, I, Ip, T = 3, 5, 8, 4
    g = np.full((O, T, Ip), np.nan)
    g[:, :, :I] = rng.standard_normal((O, T, I))
    w, a = rng.standard_normal((O, I, T)), 0.5 + rng.random(O)
    tw, ta = T64(w).requires_grad_(True), T64(a).requires_grad_(True)
    (T64(g[:, :, :I].transpose(0, 2, 1).copy()) * (tw * ta[:, None, None])).sum().backward()
    dw, _, da, _ = R.unpack_weight_grad_ref(g.reshape(O, T * Ip), w, a, Ip)
    _eq(dw, tw.grad.numpy(), 'unpack dw')
    _eq(da, ta.grad.numpy(), 'unpack da')
    N, HW, C = 2, 6, 8
    z, x, s, add = (rng.standard_normal(sh) for sh in ((N, HW, C), (N, HW, C), (N, C), (N, HW, C)))
    tsv = T64(s).requires_grad_(True)
    dx_t = T64(z) * tsv[:, None, :] + T64(add)
    (dx_t * T64(x)).sum().backward()
    r = R.dgrad_finish_ref(z, x, s, add)
    _eq(r['dx'], dx_t.detach().numpy(), 'dx')
    _eq(r['ds'], tsv.grad.numpy(), 'ds')


# ------------------------------------------------------------------------------------------------------------------ case classes
def test_the_listed_cases_reach_every_launch_class():
    reached = set()
    for c in R.ACT_CASES:
        reached |= R.classes(c.C, c.N, c.HW)
    assert reached >= set(R.ACT_CLASSES), set(R.ACT_CLASSES) - reached
    for c in R.ACT_MULTI:
        assert 'two trips, ragged last' in R.classes(c.C, c.N, c.HW), c.id
    idle = {c.C for c in R.ACT_CASES if R.launch(c.C, c.N, c.HW)['idle']}
    assert len(idle) >= 2 and idle != {160}
    full = [c for c in R.ACT_CASES if c.HW == R.launch(c.C, c.N, c.HW)['span']]
    assert full, 'no case with HW = 4 ppb bx'
    assert {c.act for c in R.ACT_CASES} == {'linear', 'relu', 'lrelu'} and {c.noise for c in R.ACT_CASES} == {'none', 'shared', 'image'}
    assert {c.clamp for c in R.ACT_CASES} == {False, True} and {c.start for c in R.ACT_CASES} == {False, True} and not all(c.d and c.bias for c in R.ACT_CASES)
    for C, N, H, W, *_ in R.FINISH_CASES[:-1]:
        L = R.launch(C, N, H * W, finish=True)
        assert L['trips'] == 2 and (H * W) % L['span'], (C, N, H, W)
    assert {c[0] for c in R.FINISH_CASES} == {1024, 512, 160, 64, 12, 4}
    assert {c[0] for c in R.DEMOD_CASES} == {1, 15, 16, 33, 257, 512} and {c[1] for c in R.DEMOD_CASES} == {1, 63, 64, 65, 200, 512} and {c[2] for c in R.DEMOD_CASES} == {1, 3}
    assert {c[1] for c in R.WGF_CASES} >= {1, 3, 255, 256, 257, 512, 1024} and {c[2] for c in R.WGF_CASES} == {1, 4, 9} and {c[3] for c in R.WGF_CASES} == {1, 3}
    assert any(c[5] == 3 and c[6] > 0 for c in R.WGF_CASES) and any(not c[4] for c in R.WGF_CASES) and R.WGF_CASES[R.WGF_BATCH[0]][0] == 1
    O, I, T, _ = R.WGF_TOO_LARGE
    assert (T * (I + 1) + I) * 4 > 64 * 1024
    assert {c[0] for c in R.UNPACK_CASES} == {1, 5} and {c[1] for c in R.UNPACK_CASES} == {3, 64, 300} and {c[3] for c in R.UNPACK_CASES} == {1, 9}
    assert any(c[2] > c[1] for c in R.UNPACK_CASES) and any(c[2] == c[1] for c in R.UNPACK_CASES)
    big = [c for c in R.FWD_CASES if c[1] * c[3] * c[4] * c[2] // 4 > 4096 * 256 and c[5] == 'none']
    assert big, 'no forward case reaches the second lap of the grid-stride loop'
    assert any(c[5].startswith('fir44') and c[3] % 2 == 0 and c[4] % 2 == 0 for c in R.FWD_CASES) and any(c[5].startswith('fir44') and (c[3] % 2 or c[4] % 2) for c in R.FWD_CASES)
    assert {c[6] for c in R.FWD_CASES if c[5] != 'none'} == {0, 1, 2} and {c[2] for c in R.FWD_CASES} >= {4, 12, 64} and {c[1] for c in R.FWD_CASES} == {1, 3}
    assert not np.array_equal(R.FIR32, R.FIR32[::-1, ::-1]) and not np.array_equal(R.FIR44N, R.FIR44N[::-1, ::-1])


# ------------------------------------------------------------------------------------------------------------------ mutants
def _ratios(mut, ref, tol):
    mut, ref, tol = (np.asarray(a, dtype=np.float64) for a in (mut, ref, tol))
    diff = np.abs(np.nan_to_num(mut, nan=np.inf) - ref)
    hit = diff > 0
    return (diff[hit] / np.broadcast_to(tol, diff.shape)[hit]).ravel()


def _fails(name, what, mut, ref, tol, seen, must_touch=True):
    """The mutant fails the comparison, and by >= MARGIN tolerances in at least half of the outputs it touches.  `what`: one output name, or a list of
    them with mut / ref dicts (the outputs of one mutant are pooled: a scalar over four million terms cannot resolve one pixel, in any arithmetic)."""
    if isinstance(what, str):
        r = _ratios(mut, ref, tol)
    else:
        r = np.concatenate([_ratios(mut[k], ref[k], ref['tol_' + k]) for k in what])
    if r.size == 0:
        assert not must_touch, f'{name}: {what} is not touched'
        return
    m = float(np.median(r))
    assert r.max() > 1.0, (name, what)
    assert m >= MARGIN, f'{name}: {what} fails by a median of only {m:.2f} tolerances'
    seen.setdefault(name, []).append(m)


@pytest.mark.parametrize('form', R.ACT_FORMS)
@pytest.mark.parametrize('case', R.ACT_CASES, ids=lambda c: c.id)
def test_activation_backward_mutants_fail_with_margin(case, form):
    """Pixels dropped from the reductions (the last of every image, one block's share, one pixel lane, the last trip), overwrite instead of accumulate,
    shared noise summed without one image, the neighbouring image's noise, d where 1 / d belongs."""
    x, start, ref = R.act_case_ref(case, form)
    t = R.act_case_terms(case, form)
    N, HW, C = case.N, case.HW, case.C
    L = ref['launch']
    blk, lane, trip = R.pixel_owner(C, N, HW)
    sums = [k for k in ('dbias', 'dd', 'dstrength', 'ds') if k in ref]
    seen = {}

    def masked(name, mask):
        mut = R.act_reduce(t, start, mask=mask)
        _fails(name, sums, mut, ref, None, seen)
        for k in sums:
            if np.ndim(ref[k]):
                _fails(name, k, mut[k], ref[k], ref['tol_' + k], seen)

    ones = np.ones((N, HW))
    m = ones.copy()
    m[:, HW - 1] = 0
    masked('last pixel of every image dropped', m)
    if L['bx'] > 1:
        m = ones.copy()
        m[0, blk == L['bx'] - 1] = 0
        mut = R.act_reduce(t, start, mask=m)
        img0 = lambda r: {k: (v if k.endswith('dbias') or np.ndim(v) == 0 else v[0]) for k, v in r.items() if k in sums or k[4:] in sums}          # noqa: E731
        _fails('one block dropped', sums, img0(mut), img0(ref), None, seen)
        for k in sums:
            if np.ndim(ref[k]):
                _fails('one block dropped', k, img0(mut)[k], img0(ref)[k], img0(ref)['tol_' + k], seen)
    if L['ppb'] > 1 and HW >= L['ppb']:
        m = ones.copy()
        m[:, lane == L['ppb'] - 1] = 0
        masked('one pixel lane dropped', m)
    if L['trips'] > 1:
        m = ones.copy()
        m[:, trip == L['trips'] - 1] = 0
        masked('last trip dropped', m)
    if start:
        mut = R.act_reduce(t, None)
        for k in sums + (['dnoise'] if 'dnoise' in ref else []):
            _fails('overwrite instead of accumulate', k, mut[k], ref[k], ref['tol_' + k], seen)
    if case.noise == 'shared' and N > 1:
        m = ones.copy()
        m[N - 1] = 0
        mut = R.act_reduce(t, start, mask=m)
        _fails('shared noise without one image', 'dnoise', mut['dnoise'], ref['dnoise'], ref['tol_dnoise'], seen)
    if case.noise == 'image' and N > 1:
        G = R.act_grad(x, form)
        mut = R.act_bwd_ref(G, x['out'], d=x['d'], bias=x['bias'], noise=np.roll(x['noise'], 1, 0), start=start, **R.act_settings(case, form))
        # (dstrength = sum noise sum_c dy changes only through the fluctuation of sum_c dy around its mean: rolling the images leaves sum_n noise alone)
        _fails('noise of the neighbouring image', [k for k in ('dd', 'dstrength') if k in ref], mut, ref, None, seen)
    if 'dd' in ref:
        mut = R.act_reduce(t, start, mutant='dd_times_d')
        _fails('d for 1 / d', 'dd', mut['dd'], ref['dd'], ref['tol_dd'], seen)
    assert 'last pixel of every image dropped' in seen
    print(f'{case.id} {form}: ' + ', '.join(f'{k} {min(v):.1f}' for k, v in seen.items()))


@pytest.mark.parametrize('case', R.FINISH_CASES, ids=str)
def test_dgrad_finish_mutants_fail(case):
    """A dropped last pixel, a dropped last trip and overwrite instead of accumulate fail in ds.  (The margin condition is the activation backward's: this
    kernel adds its ppb lanes in sequence, which makes the derived bound of the narrow channel counts wide; a pixel may weigh less than five of them.)"""
    C, N, H, W, with_ds, with_s, with_add = case
    if not with_ds:
        return
    x = R.finish_inputs(case)
    ref = R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], x['start'])
    HW = H * W
    trip = R.pixel_owner(C, N, HW, finish=True)[2]
    m = np.ones((N, HW))
    m[:, trip == ref['launch']['trips'] - 1] = 0
    muts = {'overwrite': R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], None)}
    if ref['launch']['trips'] > 1:
        muts['last trip dropped'] = R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], x['start'], mask=m)
    for name, mut in muts.items():
        assert not R.compare(mut['ds'], ref['ds'], ref['tol_ds'])[0], name
        assert R.margin(mut['ds'], ref['ds'], ref['tol_ds']) >= MARGIN, name
    m = np.ones((N, HW))
    m[:, HW - 1] = 0
    assert not R.compare(R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], x['start'], mask=m)['ds'], ref['ds'], ref['tol_ds'])[0]


@pytest.mark.parametrize('case', R.DEMOD_CASES, ids=str)
def test_demodulation_mutants_fail_with_margin(case):
    x = R.small_inputs('demod', case)
    d, tol_d = R.demod_fwd_ref(x['s'], x['wsq'])
    d32 = d.astype(np.float32)
    ref = R.demod_bwd_ref(x['s'], x['wsq'], d32, x['dd'], x['start_ds'], x['start_dwsq'])
    seen = {}
    _fails('s for s^2', 'd', R.demod_fwd_ref(x['s'], x['wsq'], mutant='s_for_s2')[0], d, tol_d, seen)
    for name, mutant, outs in (('d^2 for d^3', 'd2', (0, 2)), ('-1/2 missing', 'no_half', (2,)), ('s for s^2', 's_for_s2', (2,))):
        mut = R.demod_bwd_ref(x['s'], x['wsq'], d32, x['dd'], x['start_ds'], x['start_dwsq'], mutant=mutant)
        for o in outs:
            _fails(name, ('ds', '', 'dwsq')[o], mut[o], ref[o], ref[o + 1], seen)
    mut = R.demod_bwd_ref(x['s'], x['wsq'], d32, x['dd'])
    for o in (0, 2):
        _fails('overwrite instead of accumulate', ('ds', '', 'dwsq')[o], mut[o], ref[o], ref[o + 1], seen)


@pytest.mark.parametrize('case', R.WGF_CASES, ids=str)
def test_weight_grad_finish_mutants_fail_with_margin(case):
    x = R.small_inputs('wgf', case)
    ref, tol = R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'])
    assert np.isfinite(ref).all()
    seen = {}
    if x['dd'] is not None:
        for name, mutant in (('d^2 for d^3', 'd2'), ('factor 2 missing', 'no_two'), ('-1/2 missing', 'no_half'), ('s for s^2', 's_for_s2')):
            _fails(name, 'dw', R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'], mutant=mutant)[0], ref, tol, seen)
    if case[5] > 1:
        _fails('a slab missing', 'dw', R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'], mutant='slab_missing')[0], ref, tol, seen)
        strided = np.stack([x['buf'][k, :ref.size] for k in range(case[5])])
        assert np.array_equal(strided.reshape(x['slabs'].shape), x['slabs']) and (case[6] == 0 or np.isnan(x['buf'][:, ref.size:]).all())


@pytest.mark.parametrize('case', R.UNPACK_CASES, ids=str)
def test_unpack_weight_grad_mutant_fails_with_margin(case):
    O, I, Ip, T, with_a, with_da = case
    x = R.small_inputs('unpack', case)
    dw, tol_dw, da, tol_da = R.unpack_weight_grad_ref(x['g'], x['w'], x['a'], Ip)
    assert np.isfinite(dw).all() and np.isfinite(da).all()
    if Ip > I and T > 1:
        mw, _, ma, _ = R.unpack_weight_grad_ref(x['g'], x['w'], x['a'], Ip, mutant='ip_as_i')
        assert not R.compare(mw, dw, tol_dw)[0] and not R.compare(ma, da, tol_da)[0]
        bad = ~(np.abs(np.nan_to_num(mw, nan=np.inf) - dw) <= tol_dw * MARGIN)
        assert bad.mean() >= 0.5 * (T - 1) / T, 'Ip read as I touches every row but the first'


@pytest.mark.parametrize('case', [c for c in R.FWD_CASES if c[5] != 'none' and c[1] * c[2] * c[3] * c[4] < 1 << 20] + [R.UPCONV_CASE], ids=lambda c: c[0])
def test_forward_mutants_fail_with_margin(case):
    """The filter not flipped (the non-symmetric filters) and the window off by one (every filter)."""
    x, kw = R.fwd_inputs(case)
    ref, tol, _, _ = R.fwd_ref(x['z'], fir=x['fir'], d=x['d'], noise=x['noise'], bias=x['bias'], **kw)
    seen = {}
    if not np.array_equal(x['fir'], x['fir'][::-1, ::-1]):
        _fails('filter not flipped', 'out', R.fwd_ref(x['z'], fir=x['fir'], d=x['d'], noise=x['noise'], bias=x['bias'], flip=False, **kw)[0], ref, tol, seen)
    for shift in (1, -1):
        _fails('pad0 off by one', 'out', R.fwd_ref(x['z'], fir=x['fir'], d=x['d'], noise=x['noise'], bias=x['bias'], shift=shift, **kw)[0], ref, tol, seen)


# ------------------------------------------------------------------------------------------------------------------ honesty of the bounds
f32 = np.float32


def _seq(a, axis):
    """fp32 sum along an axis, one term after the other."""
    return np.take(np.cumsum(a, axis=axis, dtype=f32), -1, axis=axis)


def _kernel_sum(terms, L):
    """terms [N, HW, K] fp32 -> the blocks' partial sums [N, bx, K] in the kernel's shape: a lane adds its 4 trips pixels in order, the lanes meet in the tree."""
    N, HW, K = terms.shape
    span, ppb, bx = L['span'], L['ppb'], L['bx']
    pad = np.zeros((N, L['trips'] * span, K), dtype=f32)
    pad[:, :HW] = terms
    v = pad.reshape(N, L['trips'], PER_LANE, bx, ppb, K).reshape(N, L['trips'] * PER_LANE, bx, ppb, K)
    acc = _seq(v, 1)                                                  # [N, bx, ppb, K]  (adding the zeros of absent pixels changes nothing)
    st = 1
    while st < ppb:
        idx = np.arange(0, ppb - st, 2 * st)
        acc[:, :, idx] = acc[:, :, idx] + acc[:, :, idx + st]
        st <<= 1
    return acc[:, :, 0]


PER_LANE = R.PER_LANE


def _act_fp32(case, form, order):
    """The activation backward in fp32 numpy.  order 'kernel': lanes, tree, block partials added one after the other; 'npsum': np.sum."""
    x, start, ref = R.act_case_ref(case, form)
    kw = R.act_settings(case, form)
    L = ref['launch']
    N, HW, C = case.N, case.HW, case.C
    gain, slope, clamp, strength = f32(kw['gain']), f32(kw['slope']), kw['clamp'], f32(kw['strength'])
    out = x['out']
    zz = None
    if form == 'plain':
        g = x['dout']
    else:
        if form == 'finish':
            zz = x['z']
        else:
            zz = np.zeros((N, HW, C), dtype=f32)
            for o in range(4):
                zz = zz + x['dy4'][:, :, o:o + 1] * x['wa4'][None, None, :, o].reshape(1, 1, C)
        g = zz * x['s'][:, None, :] + x['addend']
    inv_gain, inv_slope = f32(1.0) / gain, (f32(1.0) / slope if slope != 0 else f32(0))
    pos = out > 0
    dy = g * gain * np.where(pos, f32(1), slope)
    if clamp >= 0:
        dy = np.where(np.abs(out) >= f32(clamp), f32(0), dy)
    dv = x['d'] if x['d'] is not None else np.ones((1, C), dtype=f32)
    got = dict(dz=dy * dv[:, None, :])
    got['dz_amax'] = float(np.abs(got['dz']).max())
    st = lambda k: start[k] if k in start else f32(0)          # noqa: E731

    def total(terms, per_image):
        """[N, HW, K] -> [N, K] (per image) or [K]."""
        if order == 'npsum':
            # (the summed axis made contiguous: numpy's pairwise summation only runs along the innermost axis; over an outer axis np.sum IS the fully
            #  sequential order that the depth bound does not describe)
            tt = np.ascontiguousarray(terms.transpose(0, 2, 1))
            return tt.sum(2, dtype=f32) if per_image else np.ascontiguousarray(tt.transpose(1, 0, 2)).reshape(terms.shape[2], -1).sum(1, dtype=f32)
        part = _kernel_sum(terms, L)
        return part if per_image else _seq(part.reshape(N * L['bx'], -1), 0)

    got['dbias'] = total(dy, False) + st('dbias')
    nraw = x['noise'] if x['noise'] is not None else np.zeros((1, HW), dtype=f32)
    nz = nraw * strength
    if 'dd' in ref:
        yy = out * inv_gain
        pre = np.where(pos | (slope == 0), yy, yy * inv_slope)
        b = x['bias'] if x['bias'] is not None else np.zeros(C, dtype=f32)
        td = dy * (pre - b[None, None, :] - nz[:, :, None])
        if order == 'npsum':
            got['dd'] = total(td, True) / dv + st('dd')
        else:
            got['dd'] = _seq(np.concatenate([np.broadcast_to(st('dd'), (N, C))[:, None].astype(f32), _kernel_sum(td, L) / dv[:, None, :]], 1), 1)
    if 'dnoise' in ref:
        cs = dy.sum(2, dtype=f32)
        dn = cs * strength
        shared = case.noise == 'shared'
        got['dnoise'] = (_seq(np.concatenate([np.broadcast_to(st('dnoise'), (1, HW)).astype(f32), dn], 0), 0)[None] if shared else dn + st('dnoise'))
        got['dstrength'] = float(_seq(np.concatenate([np.reshape(st('dstrength'), 1).astype(f32), total((cs * nraw)[:, :, None], False).reshape(-1)]), 0))
    if 'ds' in ref:
        tz = zz * out
        got['ds'] = total(tz, True) + st('ds') if order == 'npsum' else _seq(np.concatenate([np.broadcast_to(st('ds'), (N, C))[:, None].astype(f32), _kernel_sum(tz, L)], 1), 1)
    return got, ref


@pytest.mark.parametrize('form', R.ACT_FORMS)
@pytest.mark.parametrize('case', R.ACT_CASES, ids=lambda c: c.id)
def test_fp32_numpy_activation_backward_stays_under_the_bounds(case, form):
    worst = {}
    for order in ('kernel', 'npsum'):
        got, ref = _act_fp32(case, form, order)
        for k in R.ACT_OUTPUTS + ('dz_amax',):
            if k in ref:
                ok, r = R.compare(got[k], ref[k], ref['tol_' + k])
                worst[(k, order)] = r
                assert ok, (case.id, form, k, order, r)
    print(f'fp32 numpy {case.id} {form}: worst err/tol ' + ', '.join(f'{k} {worst[(k, "kernel")]:.3f}/{worst[(k, "npsum")]:.3f}' for k in R.ACT_OUTPUTS if (k, 'kernel') in worst))
    if case.C == 12 and case.N == 64 and form == 'plain':            # a fully sequential sum is NOT what the bound describes: shown, not asserted
        x, start, ref = R.act_case_ref(case, form)
        dy = (x['dout'] * f32(R.GAIN) * np.where(x['out'] > 0, f32(1), f32(R.ALPHA))).reshape(-1, case.C)
        seq = _seq(np.concatenate([start['dbias'][None], dy], 0), 0)
        print(f'   dbias summed in one sequence of {dy.shape[0]} terms: err/tol {R.compare(seq, ref["dbias"], ref["tol_dbias"])[1]:.2f}')


def test_fp32_numpy_other_kernels_stay_under_the_bounds():
    worst = {}

    def note(fam, got, ref, tol):
        ok, r = R.compare(got, ref, tol)
        worst[fam] = max(worst.get(fam, 0.0), r)
        assert ok, (fam, r)

    for case in R.FINISH_CASES:
        x = R.finish_inputs(case)
        ref = R.dgrad_finish_ref(x['z'], x['x'], x['s'], x['addend'], x['start'])
        zs = x['z'] * x['s'][:, None, :] if x['s'] is not None else x['z']
        note('dgrad_finish dx', zs + x['addend'] if x['addend'] is not None else zs, ref['dx'], ref['tol_dx'])
        if x['x'] is not None:
            t = x['z'] * x['x']
            note('dgrad_finish ds', t.sum(1, dtype=f32) + x['start'], ref['ds'], ref['tol_ds'])
            note('dgrad_finish ds', _seq(np.concatenate([x['start'][:, None], t], 1), 1), ref['ds'], ref['tol_ds'])
    for case in R.SQSUM_CASES:
        wp = R.small_inputs('sqsum', case)['wp']
        ref, tol = R.weight_sqsum_ref(wp)
        note('weight_sqsum', _seq(wp * wp, 1), ref, tol)
    for case in R.DEMOD_CASES:
        x = R.small_inputs('demod', case)
        d, tol = R.demod_fwd_ref(x['s'], x['wsq'])
        s2w = (x['s'] * x['s'])[:, None, :] * x['wsq'][None]
        for acc in (_seq(s2w, 2), s2w.sum(2, dtype=f32)):
            note('demod_fwd', f32(1) / np.sqrt(acc + f32(1e-8)), d, tol)
        d32 = d.astype(f32)
        ds, tds, dwsq, tdw = R.demod_bwd_ref(x['s'], x['wsq'], d32, x['dd'], x['start_ds'], x['start_dwsq'])
        c = x['dd'] * d32 * d32 * d32
        t = c[:, :, None] * x['wsq'][None]                        # [N, Co, Ck]
        for acc in (_seq(t, 1), t.sum(1, dtype=f32)):
            note('demod_bwd ds', x['start_ds'] + -x['s'] * acc, ds, tds)
        t = (c * f32(-0.5))[:, :, None] * (x['s'] * x['s'])[:, None, :]
        note('demod_bwd dwsq', x['start_dwsq'] + _seq(t, 0), dwsq, tdw)
    for case in R.WGF_CASES:
        x = R.small_inputs('wgf', case)
        O, I, T = x['w'].shape
        ref, tol = R.weight_grad_finish_ref(x['slabs'], x['w'], x['s'], x['d'], x['dd'])
        G = _seq(x['slabs'], 0).reshape(O, T, I).transpose(0, 2, 1)
        q = np.zeros((O, I), dtype=f32)
        if x['dd'] is not None:
            c = x['dd'] * f32(-0.5) * x['d'] * x['d'] * x['d']
            q = f32(2) * _seq(c[:, :, None] * (x['s'] * x['s'])[:, None, :], 0)
        note('weight_grad_finish', x['w'] * q[:, :, None] + G, ref, tol)
    for case in R.UNPACK_CASES:
        O, I, Ip, T, _, _ = case
        x = R.small_inputs('unpack', case)
        dw, tdw, da, tda = R.unpack_weight_grad_ref(x['g'], x['w'], x['a'], Ip)
        gg = x['g'].reshape(O, T, Ip)[:, :, :I].transpose(0, 2, 1)
        note('unpack dw', gg * (x['a'][:, None, None] if x['a'] is not None else f32(1)), dw, tdw)
        for acc in (_seq((gg * x['w']).reshape(O, -1), 1), (gg * x['w']).sum((1, 2), dtype=f32)):
            note('unpack da', acc, da, tda)
    for case in [c for c in R.FWD_CASES if c[1] * c[2] * c[3] * c[4] < 1 << 20] + [R.UPCONV_CASE]:
        x, kw = R.fwd_inputs(case)
        ref, tol, amax, tol_amax = R.fwd_ref(x['z'], fir=x['fir'], d=x['d'], noise=x['noise'], bias=x['bias'], **kw)
        v = x['z']
        if x['fir'] is not None:
            fh, fw = x['fir'].shape
            H, W, p = case[3], case[4], kw['pad0']
            zp = np.pad(x['z'], ((0, 0), (p, p), (p, p), (0, 0)))
            ff = x['fir'][::-1, ::-1] * f32(kw['fir_gain'])
            v = np.zeros((case[1], H, W, case[2]), dtype=f32)
            for ky in range(fh):
                for kx in range(fw):
                    v = v + ff[ky, kx] * zp[:, ky:ky + H, kx:kx + W]
        v = v * x['d'][:, None, None, :]
        if x['noise'] is not None:
            v = v + (x['noise'] * f32(kw['strength']))[:, :, :, None]
        v = v + x['bias']
        v = np.where(v > 0, v, v * f32(kw['slope'])) * f32(kw['gain'])
        if kw['clamp'] >= 0:
            v = np.clip(v, -f32(kw['clamp']), f32(kw['clamp']))
        assert v.dtype == f32
        note('forward', v, ref, tol)
        assert abs(float(np.abs(v).max()) - amax) <= tol_amax
    print('fp32 numpy, worst err/tol: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
