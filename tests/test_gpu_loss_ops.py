"""The kernels of csrc/loss_ops.hip on their own -- max pooling, the channel normalisation (single-level ABI and the levels launch, eps outside and
inside the root), image_prepare, sqdist, sqdist_sum / tv_norm, slice_rgb4, the warp projection, the channels-last grid sample, the direct 3 x 3
convolution in its four forms and eg3d_pool2_act_bwd -- against the float64 restatement and the derived bounds of tests/support/loss_ref.py (checked
without a GPU in tests/test_loss_ops_cpu.py).  The network- and loop-level tests compare fp32 against fp32 at 1e-5 ... 1e-3 of the largest entry on
square power-of-two shapes; a dropped lane, a dropped block's share or exchanged H / W stays below that.

  * every launch-shape class of every launcher at the smallest shapes that reach it (non-square images, ragged last blocks, G = 1 / 2 / 4 at every Ci,
    KS = 1 / 4 with unevenly dealt quads, second trips with one lane, more blocks than the caps of the reductions);
  * NaN canaries in every byte a kernel must not read or write (pad channels of ldx > C, the feature vector outside the slices, the fourth image
    channel), asserted afterwards: a NaN of the reference must be a NaN of the result and nothing else may be one;
  * exact classes (pooling, slice_rgb4, grid sample at dyadic coordinates) compared bit for bit; XF bit-equal to pool2_act_bwd + the plain launch;
  * the same file once more in a fresh interpreter under the deterministic build, where every atomically accumulated output is also bit-identical
    over two calls and det_misses() == 0.
Every case prints its worst err / tol; no comparison leaves an element out."""
import math
import os
import subprocess
import sys
from ctypes import byref

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import loss_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
EG3D_ERR_INVALID, EG3D_ERR_UNSUPPORTED = -1, -2
F32 = np.float32
NAN = float('nan')


def _L():
    from inv3d_amd import _lib as L
    return L


def _det():
    return _L().DETERMINISTIC


def _tag():
    return ' (deterministic build)' if _det() else ''


def _no_misses():
    L = _L()
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _cl(a):
    """[N, H, W, C] numpy -> [N, C, H, W] channels_last on the device."""
    return None if a is None else _dev(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return _np(t.permute(0, 2, 3, 1))


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(a, ld):
    """[..., C] -> [..., ld] with NaN in the pad channels."""
    a = np.asarray(a)
    out = np.full(a.shape[:-1] + (ld,), np.nan, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _report(name, pairs):
    """pairs: [(output, got, ref, tol)].  Prints the worst err / tol of each and asserts all of them."""
    res = [(k, *R.compare(got, ref, tol)) for k, got, ref, tol in pairs]
    print(f'{name}: worst err/tol ' + ', '.join(f'{k} {r:.4f}' for k, _, r in res) + _tag())
    bad = [(k, r) for k, ok, r in res if not ok]
    assert not bad, (name, bad)


def _check(rc, what):
    _L().check(rc, what)


# ------------------------------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize('case', R.POOL_CASES, ids=str)
def test_max_pool(case):
    from inv3d_amd import loss_nets as LN
    L = _L()
    k, s, H, W, C = case
    N = R.POOL_N
    x = R.pool_input(case)
    y_ref, idx_ref = R.maxpool_ref(x, k, s)
    Ho, Wo = R.pool_out(H, W, k, s)
    rng = np.random.default_rng(1)
    dy_d, dy_r = R.dyadic(rng, y_ref.shape), rng.standard_normal(y_ref.shape).astype(F32)
    (dx_d, _), (dx_r, tol_r) = R.maxpool_bwd_ref(dy_d, idx_ref, H, W, k, s), R.maxpool_bwd_ref(dy_r, idx_ref, H, W, k, s)
    # the wrapper (ldx = C)
    xg = _cl(x).requires_grad_(True)
    y = LN.max_pool(xg, k, s)
    assert R.exact(_nhwc(y), y_ref), 'max pool values'
    gd, = torch.autograd.grad(y, xg, _cl(dy_d), retain_graph=True)
    gr, = torch.autograd.grad(y, xg, _cl(dy_r))
    assert R.exact(_nhwc(gd), dx_d.astype(F32)), 'max pool gradient of a dyadic dy'
    # the ABI with ldx = C + 4: NaN in the pad channels of x (not read) and of dx (not written)
    ld = C + 4
    xp, yo, io = _dev(_padded(x, ld)), _nan(N, Ho, Wo, C), torch.full((N, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
    _check(L.lib().eg3d_maxpool2d_fwd(L.ptr(xp), L.ptr(yo), L.ptr(io), N, H, W, C, ld, k, s, L.stream_ptr()), 'maxpool2d_fwd')
    assert R.exact(_np(yo), y_ref) and np.array_equal(_np(io), idx_ref), 'max pool through the ABI: values / arg-max bytes'
    pairs = [('dx', _nhwc(gr), dx_r, tol_r)]
    for dy, ref, tol, exact in ((dy_d, dx_d, 0.0, True), (dy_r, dx_r, tol_r, False)):
        dxp, dyd = _nan(N, H, W, ld), _dev(dy)
        _check(L.lib().eg3d_maxpool2d_bwd(L.ptr(dyd), L.ptr(io), L.ptr(dxp), N, H, W, C, ld, k, s, L.stream_ptr()), 'maxpool2d_bwd')
        got = _np(dxp)
        assert np.isnan(got[..., C:]).all(), 'the backward wrote the pad channels'
        if exact:
            assert R.exact(got[..., :C], ref.astype(F32))
        else:
            pairs.append(('dx (ldx = C + 4)', got[..., :C], ref, tol))
    assert (dx_r[:, ~R.pool_covered(H, W, k, s)] == 0).all() and (_nhwc(gr)[:, ~R.pool_covered(H, W, k, s)] == 0).all(), 'uncovered pixels'
    _report(f'max pool k {k} s {s} {H}x{W} C {C}', pairs)


# ------------------------------------------------------------------------------------------------------------------ unit normalise
def _unit_single(x, scale, g, N, HW, C, mul, inside, gap=R.LEVELS_GAP):
    """Forward and backward through the single-level ABI with ldx = C + 8, NaN in the pad channels and in the gap after every image's slice."""
    L = _L()
    ld, stride = C + R.UNIT_LDX_PAD, HW * C + gap
    xp, sc = _dev(_padded(x.reshape(N * HW, C), ld)), _dev(scale)
    feat = _nan(N, stride)
    _check(L.lib().eg3d_unit_normalize_fwd(L.ptr(xp), L.ptr(sc), L.ptr(feat), N, HW, C, ld, mul, R.EPS, stride, inside, L.stream_ptr()), 'unit_normalize_fwd')
    dfeat = _dev(_padded(g.reshape(N, HW * C), stride))
    dx = _nan(N * HW, ld)
    _check(L.lib().eg3d_unit_normalize_bwd(L.ptr(xp), L.ptr(sc), L.ptr(dfeat), L.ptr(dx), N, HW, C, ld, mul, R.EPS, stride, inside, L.stream_ptr()), 'unit_normalize_bwd')
    return feat, dx


@pytest.mark.parametrize('C', R.UNIT_CHANNELS)
def test_unit_normalise_single_level(C):
    for (N, HW) in R.UNIT_PIXELS:
        x, scale, g, kinds = R.unit_input(N, HW, C)
        mul = R.r32(1.0 / math.sqrt(HW))
        for inside in (0, 1):
            for sc in (scale, None):
                f, tf = R.unit_fwd_ref(x, sc, mul, R.EPS, inside)
                dx, td = R.unit_bwd_ref(x, sc, g, mul, R.EPS, inside)
                feat, dxg = _unit_single(x, sc, g, N, HW, C, mul, inside)
                stride = HW * C + R.LEVELS_GAP
                ref_f, tol_f = R.assemble_features([f], stride, [0]), np.nan_to_num(R.assemble_features([tf], stride, [0]))
                ld = C + R.UNIT_LDX_PAD
                L_ = R.unit_launch(N * HW, C)
                _report(f'unit normalise C {C} N {N} HW {HW} eps {"inside" if inside else "outside"} scale {sc is not None} (G {L_["G"]}, {L_["trips"]} trips, {L_["blocks"]} blocks)',
                        [('f', _np(feat), ref_f, tol_f), ('dx', _np(dxg), _padded(dx.reshape(N * HW, C), ld), np.nan_to_num(_padded(td.reshape(N * HW, C), ld)))])
                if not inside and 'zero' in kinds:
                    assert (_np(dxg)[0, :C] == 0).all() and (_np(feat)[0, :C] == 0).all(), 'the all-zero pixel'


def _levels_data():
    offs, sizes, stride = R.levels_layout(R.LEVELS, R.LEVELS_GAP)
    data = []
    for l, (hw, c) in enumerate(R.LEVELS):
        x, scale, g, _ = R.unit_input(R.LEVELS_N, hw, c, seed=l)
        data.append(dict(x=x, scale=scale, g=g, HW=hw, C=c, mul=R.r32(1.0 / math.sqrt(hw))))
    return offs, sizes, stride, data


@pytest.mark.parametrize('inside', (0, 1))
def test_unit_normalise_levels_launch(inside):
    """Five levels of 1 ... 400 pixels in one launch through the ABI (ldx = C + 8, NaN between the images' slices), the backward without the middle level:
    inside the bounds and bit-equal to the single-level launches of the same data."""
    L = _L()
    N = R.LEVELS_N
    offs, sizes, stride, data = _levels_data()
    with_scale = not inside
    refs = [R.unit_fwd_ref(d['x'], d['scale'] if with_scale else None, d['mul'], R.EPS, inside) for d in data]
    feat, single = _nan(N, stride), _nan(N, stride)
    dfeat = _dev(_padded(np.concatenate([d['g'].reshape(N, -1) for d in data], 1), stride))
    batch = L.UnitLevels(n=len(data), N=N, eps_inside=inside, eps=R.EPS, feat_nstride=stride)
    keep = []
    for l, d in enumerate(data):
        ld = d['C'] + R.UNIT_LDX_PAD
        d['xp'], d['sc'] = _dev(_padded(d['x'].reshape(N * d['HW'], d['C']), ld)), (_dev(d['scale']) if with_scale else None)
        batch.levels[l] = L.UnitLevel(x=d['xp'].data_ptr(), scale=d['sc'].data_ptr() if with_scale else None, feat=feat.data_ptr() + 4 * offs[l], dx=None, HW=d['HW'],
                                      C=d['C'], ldx=ld, mul=d['mul'])
        _check(L.lib().eg3d_unit_normalize_fwd(L.ptr(d['xp']), L.ptr(d['sc']), single.data_ptr() + 4 * offs[l], N, d['HW'], d['C'], ld, d['mul'], R.EPS, stride, inside,
                                               L.stream_ptr()), 'unit_normalize_fwd')
    _check(L.lib().eg3d_unit_normalize_levels(byref(batch), 0, L.stream_ptr()), 'unit_normalize_levels')
    ref = R.assemble_features([r[0] for r in refs], stride, offs)
    tol = np.nan_to_num(R.assemble_features([r[1] for r in refs], stride, offs))
    assert _same_bits(feat, single), 'the levels launch differs from the single-level launches'
    # backward: level LEVELS_NO_GRAD is left out, the others move up (the compaction of loss_nets._LpipsHeadFn.backward)
    bb = L.UnitLevels(N=N, eps_inside=inside, eps=R.EPS, feat_nstride=stride)
    pairs, k = [('f', _np(feat), ref, tol)], 0
    for l, d in enumerate(data):
        if l == R.LEVELS_NO_GRAD:
            continue
        ld = d['C'] + R.UNIT_LDX_PAD
        d['dx'], d['dx1'] = _nan(N * d['HW'], ld), _nan(N * d['HW'], ld)
        bb.levels[k] = L.UnitLevel(x=d['xp'].data_ptr(), scale=d['sc'].data_ptr() if with_scale else None, feat=dfeat.data_ptr() + 4 * offs[l], dx=d['dx'].data_ptr(),
                                   HW=d['HW'], C=d['C'], ldx=ld, mul=d['mul'])
        k += 1
        _check(L.lib().eg3d_unit_normalize_bwd(L.ptr(d['xp']), L.ptr(d['sc']), dfeat.data_ptr() + 4 * offs[l], L.ptr(d['dx1']), N, d['HW'], d['C'], ld, d['mul'], R.EPS,
                                               stride, inside, L.stream_ptr()), 'unit_normalize_bwd')
    bb.n = k
    _check(L.lib().eg3d_unit_normalize_levels(byref(bb), 1, L.stream_ptr()), 'unit_normalize_levels')
    torch.cuda.synchronize()
    for l, d in enumerate(data):
        if l == R.LEVELS_NO_GRAD:
            continue
        ld = d['C'] + R.UNIT_LDX_PAD
        dx, td = R.unit_bwd_ref(d['x'], d['scale'] if with_scale else None, d['g'], d['mul'], R.EPS, inside)
        pairs.append((f'dx{l}', _np(d['dx']), _padded(dx.reshape(-1, d['C']), ld), np.nan_to_num(_padded(td.reshape(-1, d['C']), ld))))
        assert _same_bits(d['dx'], d['dx1']), f'level {l}: the levels launch differs from the single-level launch'
    _report(f'unit normalise levels eps {"inside" if inside else "outside"}', pairs)


def test_feature_heads_through_the_wrappers():
    """loss_nets.lpips_features (eps outside, the `lin` roots as scale) and loss_nets.unit_features (eps inside, no scale) on the five levels; the middle level
    does not require a gradient."""
    from inv3d_amd import loss_nets as LN
    N = R.LEVELS_N
    offs, sizes, stride, data = _levels_data()
    offs0, _, F_ = R.levels_layout(R.LEVELS, 0)
    gflat = np.concatenate([d['g'].reshape(N, -1) for d in data], 1)
    for inside in (0, 1):
        xs = []
        for l, d in enumerate(data):
            side = math.isqrt(d['HW'])
            assert side * side == d['HW']
            t = _cl(d['x'].reshape(N, side, side, d['C']))
            xs.append(t.requires_grad_(l != R.LEVELS_NO_GRAD))
        feat = LN.unit_features(xs) if inside else LN.lpips_features(xs, [_dev(d['scale']) for d in data])
        assert feat.shape == (N, F_)
        feat.backward(_dev(gflat))
        refs = [R.unit_fwd_ref(d['x'], None if inside else d['scale'], d['mul'], R.EPS, inside) for d in data]
        pairs = [('f', _np(feat), R.assemble_features([r[0] for r in refs], F_, offs0), R.assemble_features([r[1] for r in refs], F_, offs0))]
        assert xs[R.LEVELS_NO_GRAD].grad is None
        for l, d in enumerate(data):
            if l != R.LEVELS_NO_GRAD:
                dx, td = R.unit_bwd_ref(d['x'], None if inside else d['scale'], d['g'], d['mul'], R.EPS, inside)
                pairs.append((f'dx{l}', _nhwc(xs[l].grad).reshape(dx.shape), dx, td))
        _report(f'feature head through the wrapper, eps {"inside" if inside else "outside"}', pairs)


# ------------------------------------------------------------------------------------------------------------------ image_prepare
@pytest.mark.parametrize('case', R.PREP_CASES, ids=str)
def test_image_prepare(case):
    from inv3d_amd import loss_nets as LN
    N, H, W, f = case
    img, g = R.prep_input(case)                      # NaN in the fourth channel of both inputs: not read
    for mul, add in R.PREP_AFFINE:
        out, tol = R.image_prepare_fwd_ref(img, f, mul, add)
        d, td = R.image_prepare_bwd_ref(g, f, mul)
        x = _cl(img).requires_grad_(True)
        y = LN.image_prepare(x, f, mul, add)
        gx, = torch.autograd.grad(y, x, _cl(g))
        assert y.shape == (N, 4, H // f, W // f)
        _report(f'image_prepare {case} mul {mul} add {add}', [('out', _nhwc(y), out, tol), ('dimg', _nhwc(gx), d, td)])
        assert (_nhwc(y)[..., 3] == 0).all() and (_nhwc(gx)[..., 3] == 0).all(), 'channel 3 is exactly 0 in both directions'


# ------------------------------------------------------------------------------------------------------------------ sqdist
@pytest.mark.parametrize('kind', R.SQ_KINDS)
@pytest.mark.parametrize('F_', R.SQ_SIZES)
def test_sqdist(F_, kind):
    from inv3d_amd import loss_nets as LN
    a, b, g = R.sq_input(F_, kind)
    S, tol = R.sqdist_ref(a, b)
    (da, tda), (db, tdb) = R.sqdist_bwd_ref(a, b, g, 'a'), R.sqdist_bwd_ref(a, b, g, 'b')
    ad, bd, gd = _dev(a), _dev(b), _dev(g)
    pairs = []
    for need in ('a', 'b', 'ab'):
        ta, tb = ad.clone().requires_grad_('a' in need), bd.clone().requires_grad_('b' in need)
        dist = LN.sqdist(ta, tb)
        (dist * gd).sum().backward()
        pairs.append((f'S[{need}]', _np(dist), S, tol))
        assert (ta.grad is None) == ('a' not in need) and (tb.grad is None) == ('b' not in need)
        if 'a' in need:
            pairs.append((f'da[{need}]', _np(ta.grad), da, tda))
        if 'b' in need:
            pairs.append((f'db[{need}]', _np(tb.grad), db, tdb))
    L_ = R.sq_launch(F_, R.SQ_CAP)
    _report(f'sqdist F {F_} {kind} ({L_["blocks"]} blocks, {L_["trips"]} trips)', pairs)
    if _det():
        assert torch.equal(LN.sqdist(ad, bd), LN.sqdist(ad, bd)), 'two calls differ under the deterministic build'
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ sqdist_sum, tv_norm
def _targets(which):
    """(term, total) device scalars at their non-zero starting values, or None."""
    t = torch.tensor([R.OBJ_START[0]], device=DEV) if which in ('term', 'both') else None
    T = torch.tensor([R.OBJ_START[1]], device=DEV) if which in ('total', 'both') else None
    return t, T


@pytest.mark.parametrize('n', R.SQSUM_SIZES)
def test_sqdist_sum_through_the_abi(n):
    L = _L()
    a, b, _ = R.sq_input(n, 'random', seed=1, N=1)
    S, D, blocks = R.sqsum_term(a, b)
    scale, gw = R.r32(1.0 / n), R.r32(0.7 / n)
    ad, bd = _dev(a), _dev(b)
    pairs = []
    for which in ('term', 'total', 'both'):
        def call():
            t, T = _targets(which)
            _check(L.lib().eg3d_sqdist_sum_fwd(L.ptr(ad), L.ptr(bd), n, L.ptr(t), scale, L.ptr(T), gw, L.stream_ptr()), 'sqdist_sum_fwd')
            return t, T
        t, T = call()
        if t is not None:
            pairs.append((f'term[{which}]', _np(t)[0], R.OBJ_START[0] + scale * S, R.accumulate_bound(R.OBJ_START[0], [(scale, S, D, blocks)])))
        if T is not None:
            pairs.append((f'total[{which}]', _np(T)[0], R.OBJ_START[1] + gw * S, R.accumulate_bound(R.OBJ_START[1], [(gw, S, D, blocks)])))
        if _det():
            t2, T2 = call()
            assert (t is None or torch.equal(t, t2)) and (T is None or torch.equal(T, T2)), 'two calls differ under the deterministic build'
    g = torch.tensor([1.5], device=DEV)
    da = _nan(1, n)
    _check(L.lib().eg3d_sqdist_sum_bwd(L.ptr(ad), L.ptr(bd), L.ptr(g), gw, L.ptr(da), n, L.stream_ptr()), 'sqdist_sum_bwd')
    ref, tol = R.sqsum_bwd_ref(a, b, gw * 1.5)
    pairs.append(('da', _np(da), ref, tol))
    _report(f'sqdist_sum n {n} ({blocks} blocks{", beyond the cap" if R.sq_launch(n, R.SQSUM_CAP)["beyond_cap"] else ""})', pairs)
    assert L.lib().eg3d_sqdist_sum_fwd(L.ptr(ad), L.ptr(bd), n, None, scale, None, gw, L.stream_ptr()) == EG3D_ERR_INVALID         # neither target: refused, nothing launched
    _no_misses()


@pytest.mark.parametrize('shape', R.TV_SHAPES, ids=str)
def test_tv_norm_through_the_abi(shape):
    L = _L()
    B, H, W = shape
    v = R.tv_input(shape)
    S, D, blocks = R.tv_ref(v)
    scale, gw = R.r32(1.0 / ((H - 1) * (W - 1))), R.r32(1.3 / ((H - 1) * (W - 1)))
    vd = _dev(v)
    pairs = []
    for which in ('term', 'total', 'both'):
        def call():
            t, T = _targets(which)
            _check(L.lib().eg3d_tv_norm_fwd(L.ptr(vd), B, H, W, L.ptr(t), scale, L.ptr(T), gw, L.stream_ptr()), 'tv_norm_fwd')
            return t, T
        t, T = call()
        if t is not None:
            pairs.append((f'term[{which}]', _np(t)[0], R.OBJ_START[0] + scale * S, R.accumulate_bound(R.OBJ_START[0], [(scale, S, D, blocks)])))
        if T is not None:
            pairs.append((f'total[{which}]', _np(T)[0], R.OBJ_START[1] + gw * S, R.accumulate_bound(R.OBJ_START[1], [(gw, S, D, blocks)])))
        if _det():
            t2, T2 = call()
            assert (t is None or torch.equal(t, t2)) and (T is None or torch.equal(T, T2)), 'two calls differ under the deterministic build'
    g = torch.tensor([0.75], device=DEV)
    dv = _nan(B, H, W)
    _check(L.lib().eg3d_tv_norm_bwd(L.ptr(vd), L.ptr(g), gw, L.ptr(dv), B, H, W, L.stream_ptr()), 'tv_norm_bwd')
    ref, tol = R.tv_bwd_ref(v, gw * 0.75)
    pairs.append(('dv', _np(dv), ref, tol))
    _report(f'tv_norm {shape} ({blocks} blocks)', pairs)
    _no_misses()


def test_weighted_objective_two_terms_in_one_group():
    """loss_nets.weighted_objective: two squared distances in group 0 and a total variation in group 1; value, parts and every gradient."""
    from inv3d_amd import loss_nets as LN
    a1, b1, _ = R.sq_input(1020, 'random', seed=1, N=1)
    a2, b2, _ = R.sq_input(4100, 'close', seed=2, N=1)
    v = R.tv_input((3, 33, 47))
    lam = (0.7, 1.3)
    s1, s2, s3 = R.r32(1.0 / 1020), R.r32(2.0 / 4100), R.r32(1.0 / (32 * 46))
    t = [_dev(x).requires_grad_(True) for x in (a1, b1, a2, v)]
    total, parts = LN.weighted_objective([('sq', 0, s1, t[0], t[1]), ('sq', 0, s2, t[2], _dev(b2)), ('tv', 1, s3, t[3])], lam)
    total.backward()
    (S1, D1, B1), (S2, D2, B2), (S3, D3, B3) = R.sqsum_term(a1, b1), R.sqsum_term(a2, b2), R.tv_ref(v)
    gw = [R.r32(lam[0] * s1), R.r32(lam[0] * s2), R.r32(lam[1] * s3)]              # (the wrapper forms weight * scale in double and hands it over as a float)
    pairs = [('total', float(total.detach()), gw[0] * S1 + gw[1] * S2 + gw[2] * S3, R.accumulate_bound(0.0, [(gw[0], S1, D1, B1), (gw[1], S2, D2, B2), (gw[2], S3, D3, B3)])),
             ('part 0', _np(parts)[0], s1 * S1 + s2 * S2, R.accumulate_bound(0.0, [(s1, S1, D1, B1), (s2, S2, D2, B2)])),
             ('part 1', _np(parts)[1], s3 * S3, R.accumulate_bound(0.0, [(s3, S3, D3, B3)]))]
    da1, tda1 = R.sqsum_bwd_ref(a1, b1, gw[0])
    da2, tda2 = R.sqsum_bwd_ref(a2, b2, gw[1])
    dv, tdv = R.tv_bwd_ref(v, gw[2])
    pairs += [('da1', _np(t[0].grad), da1, tda1), ('db1', _np(t[1].grad), -da1, tda1), ('da2', _np(t[2].grad), da2, tda2), ('dv', _np(t[3].grad), dv, tdv)]
    _report('weighted_objective, two terms in one group', pairs)
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ slice_rgb4
@pytest.mark.parametrize('case', R.SLICE_CASES, ids=str)
def test_slice_rgb4(case):
    L = _L()
    P, C, add = case
    rng = np.random.default_rng(P + C)
    x, dy = rng.standard_normal((P, C)).astype(F32), rng.standard_normal((P, 4)).astype(F32)
    dy[:, 3] = np.nan                                       # the fourth channel of the incoming image gradient: not used
    addend = rng.standard_normal((P, C)).astype(F32) if add else None
    y, xd, dyd, addd = _nan(P, 4), _dev(x), _dev(dy), _dev(addend)
    _check(L.lib().eg3d_slice_rgb4_fwd(L.ptr(xd), L.ptr(y), P, C, L.stream_ptr()), 'slice_rgb4_fwd')
    assert R.exact(_np(y), R.slice_rgb4_ref(x))
    dx = _nan(P, C)
    if add:
        _check(L.lib().eg3d_slice_rgb4_bwd_add(L.ptr(dyd), L.ptr(addd), L.ptr(dx), P, C, L.stream_ptr()), 'slice_rgb4_bwd_add')
    else:
        _check(L.lib().eg3d_slice_rgb4_bwd(L.ptr(dyd), L.ptr(dx), P, C, L.stream_ptr()), 'slice_rgb4_bwd')
    assert R.exact(_np(dx), R.slice_rgb4_bwd_ref(dy, C, addend))
    print(f'slice_rgb4 {case}: exact' + _tag())


def test_slice_rgb4_through_the_wrapper():
    from inv3d_amd import fused
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((2, 9, 32)).astype(F32)
    t = _dev(feat).requires_grad_(True)
    y = fused.slice_rgb4(t, 3)
    gy = rng.standard_normal((2, 3, 3, 4)).astype(F32)
    y.backward(_cl(gy))
    assert R.exact(_nhwc(y).reshape(2, 9, 4), R.slice_rgb4_ref(feat)) and R.exact(_np(t.grad), R.slice_rgb4_bwd_ref(gy.reshape(2, 9, 4), 32))


# ------------------------------------------------------------------------------------------------------------------ warp projection
@pytest.mark.parametrize('view', R.WARP_VIEWS)
@pytest.mark.parametrize('P', R.WARP_P)
def test_warp_projection(P, view):
    from inv3d_amd import inversion as INV
    ext, K, o, d, depth, duv = R.warp_input(P, view)
    init_ext, intrinsic = _dev(ext.reshape(1, 4, 4)), _dev(K.reshape(9))
    consts = _np(INV._warp_consts_packed(init_ext, intrinsic))
    c64 = R.warp_consts(ext, K)
    # the constants come from torch.linalg.inv in fp32, not from a kernel of this file: a loose sanity bound; the kernel's reference takes the very
    # 24 floats the kernel reads
    assert consts.shape == (24,) and float(np.abs(consts - c64).max()) <= 1e-5 * float(np.abs(c64).max())
    uv, tol = R.warp_fwd_ref(consts, o, d, depth)
    (go, gd, gt), (to_, td_, tt_) = R.warp_bwd_ref(consts, o, d, depth, duv)
    t = [_dev(x).requires_grad_(True) for x in (o, d, depth)]
    got = INV.warp_project(t[0], t[1], t[2], init_ext, intrinsic)
    g = torch.autograd.grad(got, t, _dev(duv))
    _report(f'warp projection P {P} {view}', [('uv', _np(got), uv, tol), ('d origins', _np(g[0]), go, to_), ('d dirs', _np(g[1]), gd, td_), ('d depth', _np(g[2]), gt, tt_)])


# ------------------------------------------------------------------------------------------------------------------ grid sample
def _gs_bwd_abi(inp, grid, dout, start, case):
    L = _L()
    N, C, H, W, Ho, Wo = case
    dgrid = _nan(N, Ho, Wo, 2)
    dinp = None if start is None else _dev(start)
    _check(L.lib().eg3d_grid_sample_nhwc_bwd(L.ptr(inp), L.ptr(grid), L.ptr(dout), L.ptr(dgrid), L.ptr(dinp), N, H, W, C, Ho, Wo, L.stream_ptr()), 'grid_sample_nhwc_bwd')
    return dgrid, dinp


@pytest.mark.parametrize('case', R.GS_CASES, ids=str)
def test_grid_sample(case):
    from inv3d_amd import inversion as INV
    N, C, H, W, Ho, Wo = case
    classes = [('random', R.gs_random_grid(case)), ('contention', R.gs_contention_grid(case))]
    if H & (H - 1) == 0 and W & (W - 1) == 0:
        classes.append(('exact', R.gs_exact_grid(case)))
    for name, grid in classes:
        inp, dout, start = R.gs_data(case, name == 'exact')
        if name != 'exact':
            assert R.gs_border_distance(grid, H, W) >= R.GS_BORDER_DISTANCE, 'dgrid is discontinuous on a cell border'
        out, tol = R.grid_sample_ref(inp, grid)
        dgrid, tgrid, dinp0, tinp0 = R.grid_sample_bwd_ref(inp, grid, dout, None)
        _, _, dinp, tinp = R.grid_sample_bwd_ref(inp, grid, dout, start)
        # the wrapper: forward, and the backward onto a zero dinput
        ti, tg = _cl(inp).requires_grad_(True), _dev(grid).requires_grad_(True)
        to = INV.grid_sample_bilinear(ti, tg)
        gi, gg = torch.autograd.grad(to, [ti, tg], _cl(dout))
        # the ABI: accumulation onto a non-zero dinput, and dinput null
        ind, gd, dd = _dev(inp), _dev(grid), _dev(dout)
        dgrid_a, dinp_a = _gs_bwd_abi(ind, gd, dd, start, case)
        dgrid_n, _ = _gs_bwd_abi(ind, gd, dd, None, case)
        assert _same_bits(dgrid_a, dgrid_n) and _same_bits(dgrid_a, gg), 'dgrid depends on whether dinput is asked for'
        if name == 'exact':
            assert R.exact(_nhwc(to), out.astype(F32)) and R.exact(_np(gg), dgrid.astype(F32)) and R.exact(_nhwc(gi), dinp0.astype(F32)) and \
                R.exact(_np(dinp_a), dinp.astype(F32)), 'the dyadic class is exact'
            assert len(R.gs_validity_classes(grid, H, W)) == 16
        _report(f'grid sample {case} {name}', [('out', _nhwc(to), out, tol), ('dgrid', _np(gg), dgrid, tgrid), ('dinput', _nhwc(gi), dinp0, tinp0),
                                               ('dinput onto a start', _np(dinp_a), dinp, tinp)])
        if _det():
            again = _gs_bwd_abi(ind, gd, dd, start, case)
            assert torch.equal(dinp_a, again[1]) and _same_bits(dgrid_a, again[0]), 'two calls differ under the deterministic build'
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ conv3x3_direct
def _conv(x, wp, Co, G, N, H, W, *, y=False, pooled=False, act=False, ga=None, gb=None):
    """One launch through loss_nets._conv3x3_direct on NaN-filled outputs; returns (y, pooled) as [N, H, W, Co] / [N, H/2, W/2, Co] device tensors."""
    from inv3d_amd import loss_nets as LN
    yo = _nan(N, H, W, Co) if y else None
    po = _nan(N, H // 2, W // 2, Co) if pooled else None
    LN._conv3x3_direct(x.permute(0, 3, 1, 2), wp, Co, G, y=yo, pooled=po, act=act, alpha=R.ALPHA, gain=R.GAIN, ga=ga, gb=gb)
    return yo, po


@pytest.mark.parametrize('case', R.CONV_CASES, ids=str)
def test_conv3x3_direct(case):
    from inv3d_amd import loss_nets as LN
    L = _L()
    shape, Ci = case
    N, H, W = shape
    worst = {}

    def note(name, pairs):
        for k, got, ref, tol in pairs:
            ok, r = R.compare(got, ref, tol)
            assert ok, (name, k, r)
            worst[k] = max(worst.get(k, 0.0), r)

    for Co in R.CONV_CO:
        x, w, ga, gb = R.conv_input(shape, Ci, Co)
        ysave, wa = R.saved_output(shape, Ci), R.conv_input(shape, Ci, Co, seed=2)[1]
        act_ref, plain_ref = R.conv_fwd_ref(x, w, True), R.conv_fwd_ref(x, w, False)
        xd, ysd, gad, gbd = _dev(x), _dev(ysave), _dev(ga), _dev(gb)
        xf_refs = [R.conv_fwd_ref(R.pool2_act_bwd_ref(an, bn, ysave)[0], wa, False, extra_roundings=3) for an, bn in ((ga, None), (None, gb), (ga, gb))]
        for G in R.CONV_G:
            wp, wap = _dev(R.pack_direct(w, G)), _dev(R.pack_direct(wa, G))
            assert torch.equal(LN._pack_direct(_dev(w), G), wp), 'loss_nets._pack_direct differs from the documented layout'
            name = f'conv {shape} Ci {Ci} Co {Co} G {G}'
            y, p = _conv(xd, wp, Co, G, N, H, W, y=True, pooled=True, act=True)
            note(name, [('y', _np(y), act_ref['y'], act_ref['tol_y']), ('pooled', _np(p), act_ref['pooled'], act_ref['tol_pooled'])])
            assert (_np(y)[..., 1] == 0).all() and (_np(p)[..., 1] == 0).all(), 'the zero-weight channel'
            _, p1 = _conv(xd, wp, Co, G, N, H, W, pooled=True, act=True)
            assert _same_bits(p, p1), 'pooled-only output differs'
            y0, _ = _conv(xd, wp, Co, G, N, H, W, y=True)
            note(name, [('plain', _np(y0), plain_ref['y'], plain_ref['tol_y'])])
            for (a, b), xf_ref in zip(((gad, None), (None, gbd), (gad, gbd)), xf_refs):
                xf, _ = _conv(ysd, wap, Co, G, N, H, W, y=True, ga=a, gb=b)
                dz = _nan(N, H, W, Ci)
                _check(L.lib().eg3d_pool2_act_bwd(L.ptr(a), L.ptr(b), L.ptr(ysd), L.ptr(dz), N, H, W, Ci, R.ALPHA, R.GAIN, L.stream_ptr()), 'pool2_act_bwd')
                two, _ = _conv(dz, wap, Co, G, N, H, W, y=True)
                assert torch.equal(xf, two), f'{name}: XF differs from pool2_act_bwd followed by the plain launch (ga {a is not None}, gb {b is not None})'
                note(name, [('xf', _np(xf), xf_ref['y'], xf_ref['tol_y'])])
    L_ = R.conv_launch(N, H, W, Ci, 4, 1)
    print(f'conv3x3_direct {shape} Ci {Ci} ({L_["quads"]} quads, {L_["blocks"]} blocks, KS {L_["KS"]}, quads per wave {L_["per_wave"]}): worst err/tol '
          + ', '.join(f'{k} {r:.4f}' for k, r in worst.items()) + _tag())


@pytest.mark.parametrize('shape', R.CONV_SHAPES, ids=str)
def test_pool2_act_backward(shape):
    L = _L()
    N, H, W = shape
    pairs = []
    for C in (4, 12):
        y = R.saved_output(shape, C)
        _, _, ga, gb = R.conv_input(shape, C, 4)
        yd = _dev(y)
        for a, b, tag in ((ga, gb, 'both'), (ga, None, 'ga'), (None, gb, 'gb')):
            ref, tol = R.pool2_act_bwd_ref(a, b, y)
            dz, ad, bd = _nan(N, H, W, C), _dev(a), _dev(b)
            _check(L.lib().eg3d_pool2_act_bwd(L.ptr(ad), L.ptr(bd), L.ptr(yd), L.ptr(dz), N, H, W, C, R.ALPHA, R.GAIN, L.stream_ptr()), 'pool2_act_bwd')
            pairs.append((f'C {C} {tag}', _np(dz), ref, tol))
    _report(f'pool2_act_bwd {shape}', pairs)


def test_conv3x3_direct_refusals():
    """Odd H, XF together with act or pooled, Co % G: refused by the launcher's argument checks, before any launch; the outputs keep their canaries."""
    L = _L()
    x, wgt = torch.zeros(1, 6, 6, 4, device=DEV), torch.zeros(4 * 4 * 9, device=DEV)
    y, p, g = _nan(1, 6, 6, 4), _nan(1, 3, 3, 4), torch.zeros(1, 3, 3, 4, device=DEV)

    def rc(**kw):
        a = dict(x=x.data_ptr(), w=wgt.data_ptr(), y=y.data_ptr(), pooled=None, N=1, H=6, W=6, Ci=4, Co=4, G=4, act=0, alpha=R.ALPHA, gain=R.GAIN, ga=None, gb=None)
        a.update(kw)
        return L.lib().eg3d_conv3x3_direct(byref(L.Conv3x3DirectParams(**a)), L.stream_ptr())
    assert rc(H=5) == EG3D_ERR_UNSUPPORTED and rc(W=5) == EG3D_ERR_UNSUPPORTED
    assert rc(Co=6, G=4) == EG3D_ERR_UNSUPPORTED
    assert rc(ga=g.data_ptr(), act=1) == EG3D_ERR_INVALID
    assert rc(gb=g.data_ptr(), pooled=p.data_ptr()) == EG3D_ERR_INVALID
    assert rc(y=None) == EG3D_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(p).all()


# ------------------------------------------------------------------------------------------------------------------ deterministic build
def test_deterministic_build_has_no_misses():
    _no_misses()


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again."""
    L = _L()
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_loss_ops.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
