"""The yardstick of tests/test_gpu_loss_ops.py, checked without a GPU: tests/support/loss_ref.py equals torch float64 (autograd of the reference
expressions, F.max_pool2d, F.grid_sample, F.interpolate(mode='area'), avg_pool2d(lrelu(conv2d))) to 1e-12; its bounds accept the same operations
evaluated in fp32 numpy, once in the kernel's own order (lanes, xor tree, block partials, the fma chain along Ci) and once with np.sum; its
comparisons reject nineteen kinds of wrong result by five tolerances or more in every listed case where the mutant applies; and the listed cases
reach every launch-shape class."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import loss_ref as R      # noqa: E402

MARGIN = 5.0
F32 = np.float32
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))      # noqa: E731


def _eq(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    scale = float(np.abs(b).max())
    assert scale > 0, what
    assert float(np.abs(a - b).max()) <= 1e-12 * scale, (what, float(np.abs(a - b).max()) / scale)


def _inside(name, pairs):
    """pairs: [(what, got, ref, tol)]: prints the worst err / tol and asserts every element inside its bound."""
    res = [(k, *R.compare(g, r, t)) for k, g, r, t in pairs]
    print(f'{name}: worst err/tol ' + ', '.join(f'{k} {r:.4f}' for k, _, r in res))
    assert all(ok for _, ok, _ in res), (name, [(k, r) for k, ok, r in res if not ok])


def _rejected(what, wrong, ref, tol):
    ok, ratio = R.compare(wrong, ref, tol)
    assert not ok and ratio >= MARGIN, (what, ratio)


# ------------------------------------------------------------------------------------------------------------------ fp32 in the kernels' order
def _tree(v):
    """xor-shuffle tree over the last axis (a power of two), fp32."""
    G = v.shape[-1]
    lane = np.arange(G)
    m = G >> 1
    while m >= 1:
        v = (v + v[..., lane ^ m]).astype(F32)
        m >>= 1
    return v[..., 0]


def _block_reduce(terms, blocks, scale=None):
    """terms [n] fp32, element i owned by thread (i % 256) of block (i // 256) % blocks: the running sum per thread, the wave tree, the four waves, one
    value per block (times scale)."""
    n = terms.size
    trips = -(-n // (blocks * R.NT))
    t = np.zeros(trips * blocks * R.NT, dtype=F32)
    t[:n] = terms
    t = t.reshape(trips, blocks, 4, 64)
    s = np.zeros((blocks, 4, 64), dtype=F32)
    for j in range(trips):
        s = (s + t[j]).astype(F32)
    w = _tree(s)
    v = ((w[:, 0] + w[:, 1]).astype(F32) + (w[:, 2] + w[:, 3]).astype(F32)).astype(F32)
    return v if scale is None else (v * F32(scale)).astype(F32)


def _atomics(start, parts):
    s = F32(start)
    for p in parts:
        s = F32(s + p)
    return s


def _fma(x, w, acc):
    return (np.asarray(x, dtype=np.float64) * np.asarray(w, dtype=np.float64) + acc).astype(F32)


def _sq4(d):
    """((dx dx + dy dy) + dz dz) + dw dw of [..., 4] fp32."""
    q = (d * d).astype(F32)
    return (((q[..., 0] + q[..., 1]).astype(F32) + q[..., 2]).astype(F32) + q[..., 3]).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize('case', R.POOL_CASES, ids=str)
def test_max_pool(case):
    k, s, H, W, C = case
    x = R.pool_input(case)
    y, idx = R.maxpool_ref(x, k, s)
    tx = T64(x).permute(0, 3, 1, 2).requires_grad_(True)
    ty, ti = F.max_pool2d(tx, k, s, return_indices=True)
    assert R.exact(y, ty.detach().permute(0, 2, 3, 1).numpy())
    Ho, Wo = R.pool_out(H, W, k, s)
    ti = ti.permute(0, 2, 3, 1).numpy()
    oy, ox = np.arange(Ho)[None, :, None, None], np.arange(Wo)[None, None, :, None]
    assert np.array_equal((ti // W - oy * s) * k + (ti % W - ox * s), idx), 'arg-max routing differs from F.max_pool2d'
    assert np.isnan(y[1, 0, 0, 1]) and idx[1, 0, 0, 1] == k * k - 1 and np.isneginf(y[1, -1, -1, 2]) and idx[1, -1, -1, 2] == 0
    rng = np.random.default_rng(1)
    for kind in ('dyadic', 'random'):
        dy = R.dyadic(rng, y.shape) if kind == 'dyadic' else rng.standard_normal(y.shape).astype(F32)
        dx, tol = R.maxpool_bwd_ref(dy, idx, H, W, k, s)
        g, = torch.autograd.grad(ty, tx, T64(dy).permute(0, 3, 1, 2), retain_graph=True)
        _eq(dx, g.permute(0, 2, 3, 1).numpy(), 'max pool backward')
        assert (dx[:, ~R.pool_covered(H, W, k, s)] == 0).all() and (tol[:, ~R.pool_covered(H, W, k, s)] == 0).all()
        # fp32, the windows of a pixel added in scan order
        d32 = np.zeros((R.POOL_N, H, W, C), dtype=F32)
        for oy_ in range(Ho):
            for ox_ in range(Wo):
                for ky in range(k):
                    for kx in range(k):
                        hit = idx[:, oy_, ox_] == ky * k + kx
                        d32[:, oy_ * s + ky, ox_ * s + kx] += np.where(hit, dy[:, oy_, ox_], F32(0))
        if kind == 'dyadic':
            assert R.exact(d32, dx.astype(F32)) and (dx.astype(F32) == dx).all()
        _inside(f'max pool backward {case} {kind}', [('dx', d32, dx, tol)])
        # mutants 8, 9, 3
        for mutant in ('last_max', 'nan_dropped', 'hw_swapped'):
            if (mutant == 'last_max' and k == 1) or (mutant == 'hw_swapped' and H == W):
                continue
            ym, im = R.maxpool_ref(x, k, s, mutant)
            assert not R.exact(ym, y) or not np.array_equal(im, idx), mutant
            if mutant == 'last_max':
                assert R.exact(ym, y)                       # the values agree: only the routing tells
            _rejected(f'{mutant} {case}', R.maxpool_bwd_ref(dy, im, H, W, k, s)[0] if mutant == 'last_max' else ym, dx if mutant == 'last_max' else y,
                      tol if mutant == 'last_max' else 0.0)


# ------------------------------------------------------------------------------------------------------------------ unit normalise
def _unit32(x, scale, g, mul, eps, inside, order):
    """fp32 forward and backward; order 'kernel': lanes of a group, trips, xor tree; 'sum': np.sum."""
    x = np.asarray(x, dtype=F32)
    C = x.shape[-1]
    L = R.unit_launch(1, C)
    G, trips = L['G'], L['trips']
    s = np.ones(C, dtype=F32) if scale is None else scale
    xg = (x * g).astype(F32) * s
    if order == 'sum':
        ss, dot = np.sum((x * x).astype(F32), -1, dtype=F32), np.sum(xg.astype(F32), -1, dtype=F32)
    else:
        def lanes(a):
            p = np.zeros(a.shape[:-1] + (trips * G * 4,), dtype=F32)
            p[..., :C] = a
            return p.reshape(a.shape[:-1] + (trips, G, 4))
        xx, gg = lanes((x * x).astype(F32)), lanes(xg.astype(F32))
        ss, dot = np.zeros(x.shape[:-1] + (G,), dtype=F32), np.zeros(x.shape[:-1] + (G,), dtype=F32)
        for t in range(trips):
            for acc, a in ((ss, xx), (dot, gg)):
                q = (((a[..., t, :, 0] + a[..., t, :, 1]).astype(F32) + a[..., t, :, 2]).astype(F32) + a[..., t, :, 3]).astype(F32)
                acc += q
        ss, dot = _tree(ss), _tree(dot)
    ss, dot = ss[..., None], dot[..., None]
    mul, eps = F32(mul), F32(eps)
    r = np.sqrt(ss)
    with np.errstate(divide='ignore', invalid='ignore'):
        if inside:
            q = (F32(1) / np.sqrt(ss + eps)).astype(F32)
            inv, back = mul * q, dot * mul * q * q * q
        else:
            inv = mul / (r + eps)
            back = np.where(r > 0, dot * mul / (r * (r + eps) * (r + eps)), F32(0))
            inv_b = np.where(r > 0, inv, F32(0))
    f = (x * s).astype(F32) * inv
    dx = (g * s).astype(F32) * (inv if inside else inv_b) - x * back
    return f.astype(F32), dx.astype(F32)


@pytest.mark.parametrize('C', R.UNIT_CHANNELS)
def test_unit_normalise(C):
    for (N, HW) in R.UNIT_PIXELS:
        x, scale, g, kinds = R.unit_input(N, HW, C)
        mul = R.r32(1.0 / math.sqrt(HW))
        for inside in (0, 1):
            for sc in (scale, None):
                f, tf = R.unit_fwd_ref(x, sc, mul, R.EPS, inside)
                dx, td = R.unit_bwd_ref(x, sc, g, mul, R.EPS, inside)
                # torch float64 autograd of the reference expression (the zero pixel of the eps-outside form: 0 by definition, NaN in autograd)
                tx = T64(x).requires_grad_(True)
                ts = torch.ones(C, dtype=torch.float64) if sc is None else T64(sc)
                nrm2 = (tx * tx).sum(-1, keepdim=True)
                tf_ = tx * ts * mul * (torch.rsqrt(nrm2 + R.EPS) if inside else 1.0 / (nrm2.sqrt() + R.EPS))
                _eq(f, tf_.detach().numpy(), 'unit forward')
                tg, = torch.autograd.grad(tf_, tx, T64(g))
                tg = tg.numpy()
                if not inside and 'zero' in kinds:
                    assert np.isnan(tg.reshape(-1, C)[0]).all() and (dx.reshape(-1, C)[0] == 0).all() and (td.reshape(-1, C)[0] == 0).all()
                    tg.reshape(-1, C)[0] = 0
                _eq(dx, tg, 'unit backward')
                name = f'unit normalise C {C} N {N} HW {HW} eps {"inside" if inside else "outside"} scale {sc is not None}'
                for order in ('kernel', 'sum'):
                    f32, d32 = _unit32(x, sc, g, mul, R.EPS, inside, order)
                    _inside(f'{name} fp32 {order}', [('f', f32, f, tf), ('dx', d32, dx, td)])
                # mutants 1 (last channel quad), 6 (eps on the other side of the root), 7 (the zero pixel's gradient)
                if C >= 8 and 'big' in kinds:               # (a pixel far below eps does not feel its norm: the dropped lane shows in the others)
                    _rejected('last quad fwd', R.unit_fwd_ref(x, sc, mul, R.EPS, inside, 'last_quad')[0], f, tf)
                    _rejected('last quad bwd', R.unit_bwd_ref(x, sc, g, mul, R.EPS, inside, 'last_quad')[0], dx, td)
                assert 'tiny' in kinds
                _rejected('eps fwd', R.unit_fwd_ref(x, sc, mul, R.EPS, inside, 'eps_swapped')[0], f, tf)
                _rejected('eps bwd', R.unit_bwd_ref(x, sc, g, mul, R.EPS, inside, 'eps_swapped')[0], dx, td)
                if not inside and 'zero' in kinds:
                    for m in ('zero_nan', 'zero_limit'):
                        _rejected(m, R.unit_bwd_ref(x, sc, g, mul, R.EPS, inside, m)[0], dx, td)


def test_feature_vector_layout_mutants():
    """Mutants 4 and 5: the slices of the flat feature vector."""
    offs, sizes, stride = R.levels_layout(R.LEVELS, R.LEVELS_GAP)
    assert sizes.index(max(sizes)) != 0 and max(hw for hw, _ in R.LEVELS) == 400 and min(hw for hw, _ in R.LEVELS) == 1
    outs, tols = [], []
    for l, (hw, c) in enumerate(R.LEVELS):
        x, scale, g, _ = R.unit_input(R.LEVELS_N, hw, c, seed=l)
        f, t = R.unit_fwd_ref(x, scale, R.r32(1 / math.sqrt(hw)))
        outs.append(f)
        tols.append(t)
    ref, tol = R.assemble_features(outs, stride, offs), np.nan_to_num(R.assemble_features(tols, stride, offs))
    assert np.isnan(ref[:, stride - R.LEVELS_GAP:]).all() and not np.isnan(ref[:, :stride - R.LEVELS_GAP]).any()
    assert R.compare(ref, ref, tol) == (True, 0.0)
    for m in ('batch_stride', 'level_offset'):
        _rejected(m, R.assemble_features(outs, stride, offs, m), ref, tol)
    one = R.assemble_features(outs[:1], sizes[0], [0])
    assert not np.isnan(one).any() and R.exact(R.assemble_features(outs[:1], sizes[0], [0], 'batch_stride'), one)       # (a single level: stride == slice)


# ------------------------------------------------------------------------------------------------------------------ image_prepare
@pytest.mark.parametrize('case', R.PREP_CASES, ids=str)
def test_image_prepare(case):
    N, H, W, f = case
    img, g = R.prep_input(case, nan_channel3=False)
    for mul, add in R.PREP_AFFINE:
        out, tol = R.image_prepare_fwd_ref(img, f, mul, add)
        d, td = R.image_prepare_bwd_ref(g, f, mul)
        ti = T64(img[..., :3]).permute(0, 3, 1, 2).requires_grad_(True)
        to = F.interpolate(ti * R.r32(mul) + R.r32(add), size=(H // f, W // f), mode='area')
        _eq(out[..., :3], to.detach().permute(0, 2, 3, 1).numpy(), 'image_prepare')
        tg, = torch.autograd.grad(to, ti, T64(g[..., :3]).permute(0, 3, 1, 2))
        _eq(d[..., :3], tg.permute(0, 2, 3, 1).numpy(), 'image_prepare backward')
        assert (out[..., 3] == 0).all() and (d[..., 3] == 0).all() and (tol[..., 3] == 0).all() and (td[..., 3] == 0).all()
        v = img[..., :3].reshape(N, H // f, f, W // f, f, 3)
        m = F32(F32(mul) / F32(f * f))
        seq = np.zeros((N, H // f, W // f, 3), dtype=F32)
        for ky in range(f):
            for kx in range(f):
                seq = (seq + v[:, :, ky, :, kx]).astype(F32)
        pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (1,), dtype=F32)], -1)      # noqa: E731
        _inside(f'image_prepare {case} mul {mul}', [('kernel order', pad(_fma(seq, m, F32(add))), out, tol),
                                                    ('np.sum', pad((np.sum(v, (2, 4), dtype=F32) * m + F32(add)).astype(F32)), out, tol),
                                                    ('backward', (np.repeat(np.repeat(g, f, 1), f, 2) * np.array([m, m, m, 0], dtype=F32)).astype(F32), d, td)])
        assert H != W
        if f > 1:                                           # (f = 1 is the identity on the flat buffer: there is no index split to get wrong)
            _rejected('hw fwd', R.image_prepare_fwd_ref(img, f, mul, add, 'hw_swapped')[0], out, tol)
            _rejected('hw bwd', R.image_prepare_bwd_ref(g, f, mul, 'hw_swapped')[0], d, td)
            _rejected('mean over f', R.image_prepare_fwd_ref(img, f, mul, add, 'mean_over_f')[0], out, tol)
            _rejected('mean over f bwd', R.image_prepare_bwd_ref(g, f, mul, 'mean_over_f')[0], d, td)


# ------------------------------------------------------------------------------------------------------------------ sqdist, sqdist_sum, tv
@pytest.mark.parametrize('kind', R.SQ_KINDS)
@pytest.mark.parametrize('F_', R.SQ_SIZES)
def test_sqdist(F_, kind):
    a, b, g = R.sq_input(F_, kind)
    S, tol = R.sqdist_ref(a, b)
    ta, tb = T64(a).requires_grad_(True), T64(b).requires_grad_(True)
    ts = (ta - tb).square().sum(1)
    _eq(S, ts.detach().numpy(), 'sqdist')
    ga, gb = torch.autograd.grad((ts * T64(g)).sum(), [ta, tb])
    (da, tda), (db, tdb) = R.sqdist_bwd_ref(a, b, g, 'a'), R.sqdist_bwd_ref(a, b, g, 'b')
    _eq(da, ga.numpy(), 'd sqdist / da')
    _eq(db, gb.numpy(), 'd sqdist / db')
    L = R.sq_launch(F_, R.SQ_CAP)
    d32 = (a - b).astype(F32)
    kern = np.array([_atomics(0, _block_reduce(_sq4(d32[n].reshape(-1, 4)), L['blocks'])) for n in range(R.SQ_N)])
    k32 = (F32(2) * g)[:, None] * d32
    _inside(f'sqdist F {F_} {kind} ({L["blocks"]} blocks, {L["trips"]} trips)',
            [('kernel order', kern, S, tol), ('np.sum', np.sum((d32 * d32).astype(F32), 1, dtype=F32), S, tol), ('da', k32, da, tda), ('db', -k32, db, tdb)])
    if kind == 'close':
        assert float(tol.max()) < 1e-4 * float(S.max()) and float(S.max()) < 1e-10 * float((a.astype(np.float64) ** 2).sum(1).min())       # the bound follows a ~ b
    if L['blocks'] > 1:
        _rejected('block dropped', R.sqdist_ref(a, b, mutant='block_dropped')[0], S, tol)
    _rejected('b sign', R.sqdist_bwd_ref(a, b, g, 'b', 'b_sign')[0], db, tdb)
    for w in 'ab':
        _rejected('factor 2', R.sqdist_bwd_ref(a, b, g, w, 'no_factor_2')[0], *R.sqdist_bwd_ref(a, b, g, w))


@pytest.mark.parametrize('n', R.SQSUM_SIZES)
def test_sqdist_sum_accumulates(n):
    a, b, _ = R.sq_input(n, 'random', seed=1, N=1)
    S, D, blocks = R.sqsum_term(a, b)
    scale, gw = 1.0 / n, 0.7 / n
    start_t, start_T = R.OBJ_START
    ref_t, ref_T = start_t + scale * S, start_T + gw * S
    tol_t, tol_T = R.accumulate_bound(start_t, [(scale, S, D, blocks)]), R.accumulate_bound(start_T, [(gw, S, D, blocks)])
    d32 = (a - b).astype(F32).reshape(-1, 4)
    got_t = _atomics(start_t, _block_reduce(_sq4(d32), blocks, scale))
    got_T = _atomics(start_T, _block_reduce(_sq4(d32), blocks, gw))
    sm = np.sum((d32 * d32).astype(F32), dtype=F32)
    _inside(f'sqdist_sum n {n} ({blocks} blocks)', [('term', got_t, ref_t, tol_t), ('total', got_T, ref_T, tol_T),
                                                   ('np.sum', F32(F32(start_t) + sm * F32(scale)), ref_t, tol_t)])
    _rejected('start ignored', scale * S, ref_t, tol_t)
    if blocks > 1:
        i4 = np.arange(n // 4)
        dropped = float((d32.astype(np.float64) ** 2).sum(1)[(i4 // R.NT) % blocks != 1].sum())
        _rejected('block dropped', start_t + scale * dropped, ref_t, tol_t)
    # two terms in one group
    tol2 = R.accumulate_bound(start_t, [(scale, S, D, blocks), (2 * scale, S, D, blocks)])
    got2 = _atomics(got_t, _block_reduce(_sq4(d32), blocks, 2 * scale))
    _inside('two terms in one group', [('term', got2, start_t + 3 * scale * S, tol2)])
    _rejected('second term dropped', ref_t, start_t + 3 * scale * S, tol2)


@pytest.mark.parametrize('shape', R.TV_SHAPES, ids=str)
def test_tv_norm(shape):
    B, H, W = shape
    v = R.tv_input(shape)
    S, D, blocks = R.tv_ref(v)
    tv = T64(v).requires_grad_(True)
    v00, v01, v10 = tv[:, :-1, :-1], tv[:, :-1, 1:], tv[:, 1:, :-1]
    loss = ((v00 - v01) ** 2) + ((v00 - v10) ** 2)
    _eq(S / loss.numel(), torch.mean(torch.mean(loss)).item(), 'compute_tv_norm')
    k = 0.37
    tg, = torch.autograd.grad(loss.sum() * k, tv)
    dv, tdv = R.tv_bwd_ref(v, k)
    _eq(dv, tg.numpy(), 'tv backward')
    scale = 1.0 / ((H - 1) * (W - 1))
    start = R.OBJ_START[0]
    ref, tol = start + scale * S, R.accumulate_bound(start, [(scale, S, D, blocks)])
    t32 = np.zeros((B, H, W), dtype=F32)
    c = v[:, :-1, :-1]
    r, d = (c - v[:, :-1, 1:]).astype(F32), (c - v[:, 1:, :-1]).astype(F32)
    t32[:, :-1, :-1] = ((r * r).astype(F32) + (d * d).astype(F32)).astype(F32)
    a32 = np.zeros((B, H, W), dtype=F32)
    a32[:, :-1, :-1] = (r + d).astype(F32)
    a32[:, :-1, 1:] -= r
    a32[:, 1:, :-1] -= d
    _inside(f'tv {shape} ({blocks} blocks)', [('kernel order', _atomics(start, _block_reduce(t32.reshape(-1), blocks, scale)), ref, tol),
                                              ('np.sum', F32(F32(start) + np.sum(t32, dtype=F32) * F32(scale)), ref, tol),
                                              ('dv', (F32(2) * F32(k) * a32).astype(F32), dv, tdv)])
    _rejected('last row / column', start + scale * R.tv_ref(v, 'last_row_col')[0], ref, tol)
    _rejected('last row / column bwd', R.tv_bwd_ref(v, k, 'last_row_col')[0], dv, tdv)
    if H != W:
        _rejected('hw', start + scale * R.tv_ref(v, 'hw_swapped')[0], ref, tol)
        _rejected('hw bwd', R.tv_bwd_ref(v, k, 'hw_swapped')[0], dv, tdv)
    if blocks > 1:
        _rejected('block dropped', start + scale * R.tv_ref(v, 'block_dropped')[0], ref, tol)


def test_slice_rgb4_restatement():
    rng = np.random.default_rng(0)
    for P, C, add in R.SLICE_CASES:
        x, dy = rng.standard_normal((P, C)).astype(F32), rng.standard_normal((P, 4)).astype(F32)
        y = R.slice_rgb4_ref(x)
        assert np.array_equal(y[:, :3], x[:, :3]) and (y[:, 3] == 0).all()
        addend = R.dyadic(rng, (P, C)) if add else None
        dx = R.slice_rgb4_bwd_ref(dy, C, addend)
        want = np.zeros((P, C), dtype=F32) if addend is None else addend.copy()
        want[:, :3] = want[:, :3] + dy[:, :3]
        assert np.array_equal(dx, want) and dx.dtype == F32


# ------------------------------------------------------------------------------------------------------------------ warp projection
def _warp_chain(ext, K, o, d, depth):
    """warping_loss.py:18-54 and LinePlaneCollision (:58-72) in torch float64."""
    P = depth.shape[0]
    xyz = o + d * depth[:, None]
    cam_o = ext[:3, 3].expand(P, 3)
    vectors, normal = xyz - cam_o, -cam_o
    plane_pt = (ext @ torch.tensor([0., 0., 1., 1.], dtype=torch.float64))[:3].expand(P, 3)
    ndotu = (normal * vectors).sum(-1, keepdim=True)
    w_vec = cam_o - plane_pt
    si = -(normal * w_vec).sum(-1, keepdim=True) / ndotu
    hit = w_vec + si * vectors + plane_pt
    hit1 = torch.cat([hit, torch.ones(P, 1, dtype=torch.float64)], -1).t()
    uv = (torch.linalg.inv(ext) @ hit1)[:3].t()
    uv = uv / uv[:, 2:]
    uv = (K @ uv.t())[:2].t()
    return (uv - 0.5) * 2


@pytest.mark.parametrize('view', R.WARP_VIEWS)
@pytest.mark.parametrize('P', R.WARP_P)
def test_warp_projection(P, view):
    ext, K, o, d, depth, duv = R.warp_input(P, view)
    assert depth.min() >= 2.2 and depth.max() <= 3.2
    c64 = R.warp_consts(ext, K)
    uv64, _ = R.warp_fwd_ref(c64, o, d, depth)
    to, td, tt = (T64(a).requires_grad_(True) for a in (o, d, depth))
    tu = _warp_chain(T64(ext), T64(K), to, td, tt)
    _eq(uv64, tu.detach().numpy(), 'warp projection')
    grads = torch.autograd.grad((tu * T64(duv)).sum(), [to, td, tt])
    adj = R.warp_adjoint(c64, o, d, depth, duv)
    bwd, _ = R.warp_bwd_ref(c64, o, d, depth, duv)
    for a, b, g, name in zip(adj, bwd, grads, ('d origins', 'd dirs', 'd depth')):
        _eq(a, g.numpy(), name)
        _eq(b, g.numpy(), name + ' (backward program)')
    # the kernel's inputs are the 24 constants in fp32: the reference of the fp32 evaluations takes those
    c32 = c64.astype(F32)
    uv, tol = R.warp_fwd_ref(c32, o, d, depth)
    (go, gd, gt), (to_, td_, tt_) = R.warp_bwd_ref(c32, o, d, depth, duv)
    k32 = [F32(v) for v in c32]
    o32, d32 = [o[:, i] for i in range(3)], [d[:, i] for i in range(3)]
    u32 = np.stack(R.warp_fwd_eval(k32, o32, d32, depth), -1)
    b32 = R.warp_bwd_eval(k32, o32, d32, depth, duv[:, 0], duv[:, 1])
    assert u32.dtype == F32 and all(b.dtype == F32 for b in b32)
    _inside(f'warp projection P {P} {view} fp32', [('uv', u32, uv, tol), ('d origins', np.stack(b32[0:3], -1), go, to_), ('d dirs', np.stack(b32[3:6], -1), gd, td_),
                                                   ('d depth', b32[6], gt, tt_)])
    assert float(tol.max()) < 1e-4 and float(np.abs(uv).max()) > 0.1
    # the intersection scale cancels in q_xy / q_z: a wrong plane point is not observable in uv (loss_ref.py, W) ...
    assert R.compare(R.warp_fwd_ref(R.warp_consts(ext, K, 'plane_point_transposed').astype(F32), o, d, depth)[0], uv, tol)[0]
    # ... mutant 19 is a transposed intrinsics row (a constant shift where K_01 = K_10 = 0: the gradient cannot tell) and the transposed rotation
    for m in ('intrinsics_transposed', 'rotation_transposed'):
        cm = R.warp_consts(ext, K, m).astype(F32)
        _rejected(m, R.warp_fwd_ref(cm, o, d, depth)[0], uv, tol)
        if m == 'rotation_transposed':
            wrong = R.warp_bwd_ref(cm, o, d, depth, duv)[0]
            for a, b, t in zip(wrong, (go, gd, gt), (to_, td_, tt_)):
                _rejected(m + ' bwd', a, b, t)


def test_warp_cameras_are_the_synthetic_cameras_construction():
    """loss_ref.camera is the look-at construction of the oracle's synth_cameras (same radius, focal length, yaw / pitch inside its ranges); the third
    view is the canonical one turned by 60 degrees."""
    from oracle import eg3d_oracle as O
    c = O.synth_cameras(1, seed=5)
    assert np.array_equal(c[0, 16:].numpy().reshape(3, 3), R.WARP_K)
    for yaw, pitch in ((math.pi / 2 + 0.1, math.pi / 2 - 0.05), (math.pi / 2 - 0.3, math.pi / 2 + 0.2), (math.pi / 2 + 0.1 + math.pi / 3, math.pi / 2 - 0.05)):
        origin = torch.tensor([2.7 * math.sin(pitch) * math.cos(math.pi - yaw), 2.7 * math.cos(pitch), 2.7 * math.sin(pitch) * math.sin(math.pi - yaw)], dtype=torch.float32)
        want = O.lookat_cam2world(origin, torch.zeros(3)).numpy()
        assert float(np.abs(R.camera(yaw, pitch) - want).max()) <= 4 * 2.0 ** -24 * 2.7
    ext, _, o, _, _, _ = R.warp_input(257, 'rotated60')
    c0, c1 = ext[:3, 3].astype(np.float64), o.mean(0).astype(np.float64)
    cosang = float(c0[[0, 2]] @ c1[[0, 2]] / (np.linalg.norm(c0[[0, 2]]) * np.linalg.norm(c1[[0, 2]])))
    assert abs(math.degrees(math.acos(cosang)) - 60.0) < 0.5


# ------------------------------------------------------------------------------------------------------------------ grid sample
def _gs32(inp, grid, dout, start):
    """fp32 in the kernel's order: a wave per output pixel, lane = channel quad, trips over 256 channels, xor tree for dgrid; dinput in pixel order."""
    N, H, W, C = inp.shape
    Ho, Wo = grid.shape[1:3]
    gx, gy = grid[..., 0], grid[..., 1]
    ix = (((gx + F32(1)) * F32(W)).astype(F32) - F32(1)) * F32(0.5)
    iy = (((gy + F32(1)) * F32(H)).astype(F32) - F32(1)) * F32(0.5)
    fx, fy = np.floor(ix), np.floor(iy)
    tx, ty = (ix - fx).astype(F32), (iy - fy).astype(F32)
    x0, y0 = fx.astype(int), fy.astype(int)
    ux, uy = (F32(1) - tx).astype(F32), (F32(1) - ty).astype(F32)
    cs = [(0, 0, ux * uy, -uy, -ux), (0, 1, tx * uy, uy, -tx), (1, 0, ux * ty, -ty, ux), (1, 1, tx * ty, ty, tx)]
    n = np.broadcast_to(np.arange(N)[:, None, None], x0.shape)
    trips = -(-C // 256)
    out = np.zeros((N, Ho, Wo, C), dtype=F32)
    ggx, ggy = np.zeros((N, Ho, Wo, trips * 64), dtype=F32), np.zeros((N, Ho, Wo, trips * 64), dtype=F32)
    dinp = start.copy()
    for dy, dx, w, sx, sy in cs:
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        t = inp[n, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None]
        out = _fma(w[..., None], t, out)
        p = np.zeros((N, Ho, Wo, trips * 256), dtype=F32)
        p[..., :C] = (dout * t).astype(F32)
        p = p.reshape(N, Ho, Wo, trips * 64, 4)
        dot = (((p[..., 0] + p[..., 1]).astype(F32) + p[..., 2]).astype(F32) + p[..., 3]).astype(F32)
        ggx, ggy = _fma(sx[..., None], dot, ggx), _fma(sy[..., None], dot, ggy)
        np.add.at(dinp, (n, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)), ((w * ok)[..., None] * dout).astype(F32))
    def lanes(a):
        a = a.reshape(N, Ho, Wo, trips, 64)
        s = np.zeros((N, Ho, Wo, 64), dtype=F32)
        for t_ in range(trips):
            s = (s + a[..., t_, :]).astype(F32)
        return _tree(s)
    # (a lane's trips interleave with its corners in the kernel; the sum per lane is over the same eight terms)
    dgrid = np.stack([(lanes(ggx) * F32(W)).astype(F32) * F32(0.5), (lanes(ggy) * F32(H)).astype(F32) * F32(0.5)], -1)
    return out, dgrid.astype(F32), dinp


@pytest.mark.parametrize('case', R.GS_CASES, ids=str)
def test_grid_sample(case):
    N, C, H, W, Ho, Wo = case
    classes = [('random', R.gs_random_grid(case)), ('contention', R.gs_contention_grid(case))]
    if H & (H - 1) == 0 and W & (W - 1) == 0:
        classes.append(('exact', R.gs_exact_grid(case)))
        assert len(R.gs_validity_classes(classes[-1][1], H, W)) == 16
    for name, grid in classes:
        inp, dout, start = R.gs_data(case, name == 'exact')
        out, tol = R.grid_sample_ref(inp, grid)
        dgrid, tgrid, dinp, tinp = R.grid_sample_bwd_ref(inp, grid, dout, start)
        ti, tg = T64(inp).permute(0, 3, 1, 2).requires_grad_(True), T64(grid).requires_grad_(True)
        to = F.grid_sample(ti, tg, mode='bilinear', padding_mode='zeros', align_corners=False)
        if name != 'exact':
            assert R.gs_border_distance(grid, H, W) >= R.GS_BORDER_DISTANCE
        _eq(out, to.detach().permute(0, 2, 3, 1).numpy(), 'grid sample')
        gi, gg = torch.autograd.grad(to, [ti, tg], T64(dout).permute(0, 3, 1, 2))
        _eq(dinp, gi.permute(0, 2, 3, 1).numpy() + start, 'd input')
        if name != 'exact':                             # (on a cell border dgrid is one-sided: torch and the kernel both take the cell of floor())
            _eq(dgrid, gg.numpy(), 'd grid')
        o32, g32, i32 = _gs32(inp, grid, dout, start)
        if name == 'exact':
            assert R.exact(o32, out.astype(F32)) and R.exact(g32, dgrid.astype(F32)) and R.exact(i32, dinp.astype(F32))
            assert (out.astype(F32) == out).all() and (dgrid.astype(F32) == dgrid).all() and (dinp.astype(F32) == dinp).all()
        _inside(f'grid sample {case} {name} fp32', [('out', o32, out, tol), ('dgrid', g32, dgrid, tgrid), ('dinput', i32, dinp, tinp)])
        if name == 'contention':
            assert float(tinp.max()) > 0 and int((np.abs(dinp - start) > 0).any(-1).sum()) == 4 * N        # Ho * Wo terms in each of four pixels per image
        if name == 'random':
            for m in ('align_corners', 'border', 'w01_w10', 'last_quad'):
                _rejected(m, R.grid_sample_ref(inp, grid, m)[0], out, tol)
            for m in ('align_corners', 'border', 'w01_w10', 'no_half_size', 'last_quad'):
                wrong = R.grid_sample_bwd_ref(inp, grid, dout, start, m)
                _rejected(m + ' dgrid', wrong[0], dgrid, tgrid)
                if m not in ('no_half_size', 'last_quad'):
                    _rejected(m + ' dinput', wrong[2], dinp, tinp)


# ------------------------------------------------------------------------------------------------------------------ conv3x3_direct
def _conv32(x, w, KS, order):
    """fp32 accumulators [N, H, W, Co]; 'kernel': fma chain over the wave's channel quads (tap, channel of the quad), KS - 1 LDS adds; 'sum': fp32 einsum."""
    N, H, W, Ci = x.shape
    Co = w.shape[0]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if order == 'sum':
        cols = np.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], -1)      # [N, H, W, Ci, 9]
        return np.einsum('nhwct,oct->nhwo', cols, w.reshape(Co, Ci, 9).astype(F32)).astype(F32)
    part = []
    for ks in range(KS):
        acc = np.zeros((N, H, W, Co), dtype=F32)
        for cq in range(ks, Ci // 4, KS):
            for ky in range(3):
                for kx in range(3):
                    for j in range(4):
                        c = 4 * cq + j
                        acc = _fma(xp[:, ky:ky + H, kx:kx + W, c][..., None], w[:, c, ky, kx], acc)
        part.append(acc)
    acc = part[0]
    for p in part[1:]:
        acc = (acc + p).astype(F32)
    return acc


def _epilogue32(z, act, alpha, gain):
    alpha, gain = F32(alpha), F32(gain)
    y = (z * np.where(z > 0, gain, gain * alpha)).astype(F32) if act else z
    N, H, W, C = y.shape
    q = y.reshape(N, H // 2, 2, W // 2, 2, C)
    pool = (((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]).astype(F32) + q[:, :, 1, :, 0]).astype(F32) + q[:, :, 1, :, 1]).astype(F32) * F32(0.25)
    return y, pool


@pytest.mark.parametrize('case', R.CONV_CASES, ids=str)
def test_conv3x3_direct(case):
    shape, Ci = case
    N, H, W = shape
    KS = 4 if Ci >= 16 else 1
    for Co in R.CONV_CO:
        x, w, ga, gb = R.conv_input(shape, Ci, Co)
        ref = R.conv_fwd_ref(x, w, True)
        tx = T64(x).permute(0, 3, 1, 2).requires_grad_(True)
        tz = F.conv2d(tx, T64(w), padding=1)
        ty = F.leaky_relu(tz, R.r32(R.ALPHA)) * R.r32(R.GAIN)
        _eq(ref['y'], ty.detach().permute(0, 2, 3, 1).numpy(), 'lrelu(conv) gain')
        _eq(ref['pooled'], F.avg_pool2d(ty, 2).detach().permute(0, 2, 3, 1).numpy(), 'avg_pool2d')
        assert (ref['y'][..., 1] == 0).all() and (ref['tol_y'][..., 1] == 0).all(), 'the zero-weight channel is exactly 0'
        # the plain form on the adjoint weights is the data gradient
        dz = R.saved_output(shape, Co, seed=5)
        plain = R.conv_fwd_ref(dz, R.adjoint_weights(w), False)
        tg, = torch.autograd.grad(tz, tx, T64(dz).permute(0, 3, 1, 2), retain_graph=True)
        _eq(plain['y'], tg.permute(0, 2, 3, 1).numpy(), 'data gradient')
        for order in ('kernel', 'sum'):
            y32, p32 = _epilogue32(_conv32(x, w, KS, order), True, R.ALPHA, R.GAIN)
            _inside(f'conv {case} Co {Co} fp32 {order}', [('y', y32, ref['y'], ref['tol_y']), ('pooled', p32, ref['pooled'], ref['tol_pooled']),
                                                          ('plain', _conv32(dz, R.adjoint_weights(w), 4 if Co >= 16 else 1, order), plain['y'], plain['tol_y'])])
        # XF: the pooling / activation backward formed on the fly equals pool2_act_bwd followed by the plain conv
        ysave = R.saved_output(shape, Ci)
        wa = R.conv_input(shape, Ci, Co, seed=2)[1]
        for a, b in ((ga, None), (None, gb), (ga, gb)):
            dzr, tdz = R.pool2_act_bwd_ref(a, b, ysave)
            xf = R.conv_fwd_ref(dzr, wa, False, extra_roundings=3)
            gsum = (np.zeros_like(ga) if a is None else a) + (np.zeros_like(gb) if b is None else b)
            alpha, gain = F32(R.ALPHA), F32(R.GAIN)
            dz32 = (np.repeat(np.repeat(gsum.astype(F32), 2, 1), 2, 2) * np.where(ysave > 0, F32(0.25) * gain, F32(0.25) * gain * alpha)).astype(F32)
            _inside(f'XF {case} Co {Co} ga {a is not None} gb {b is not None}', [('dz', dz32, dzr, tdz), ('conv', _conv32(dz32, wa, KS, 'kernel'), xf['y'], xf['tol_y'])])
        # mutants 1, 3, 11
        for m in ('last_quad', 'hw_swapped', 'no_quarter'):
            if m == 'hw_swapped' and H == W:
                continue
            wrong = R.conv_fwd_ref(x, w, True, mutant=m)
            if m != 'no_quarter':
                _rejected(f'{m} y', wrong['y'], ref['y'], ref['tol_y'])
            _rejected(f'{m} pooled', wrong['pooled'], ref['pooled'], ref['tol_pooled'])


@pytest.mark.parametrize('shape', R.CONV_SHAPES, ids=str)
def test_pool2_act_backward(shape):
    N, H, W = shape
    for C in (4, 12):
        y = R.saved_output(shape, C)
        _, _, ga, gb = R.conv_input(shape, C, 4)
        assert (y == 0).any() and (y[..., 1] == 0).all()
        tz = T64(np.where(y == 0, -1.0, y)).permute(0, 3, 1, 2).requires_grad_(True)      # a pre-activation with the sign of the saved output (0 counts as not positive)
        tp = F.avg_pool2d(F.leaky_relu(tz, R.r32(R.ALPHA)) * R.r32(R.GAIN), 2)
        tg, = torch.autograd.grad(tp, tz, (T64(ga) + T64(gb)).permute(0, 3, 1, 2))
        dz, tol = R.pool2_act_bwd_ref(ga, gb, y)
        _eq(dz, tg.permute(0, 2, 3, 1).numpy(), 'pool2_act_bwd')
        for a, b in ((ga, None), (None, gb)):
            one, _ = R.pool2_act_bwd_ref(a, b, y)
            assert np.array_equal(one, R.pool2_act_bwd_ref(a if a is not None else b, np.zeros_like(ga), y)[0])
        for m in ('ge_sign', 'no_quarter', 'hw_swapped'):
            if m == 'hw_swapped' and H == W:
                continue
            _rejected(m, R.pool2_act_bwd_ref(ga, gb, y, mutant=m)[0], dz, tol)


# ------------------------------------------------------------------------------------------------------------------ launch-shape coverage
def test_the_listed_cases_reach_every_launch_shape_class():
    got = R.launch_classes()
    assert R.REQUIRED_CLASSES <= got, sorted(R.REQUIRED_CLASSES - got)
    # the conv classes of the issue, by name
    assert R.conv_launch(2, 6, 10, 4, 4, 1)['quads'] == 15 and R.conv_launch(1, 18, 16, 4, 4, 1)['quads'] == 72 and R.conv_launch(1, 2, 2, 4, 4, 1)['quads'] == 1
    assert R.conv_launch(1, 18, 16, 20, 4, 1)['per_wave'] == [2, 1, 1, 1] and R.conv_launch(1, 18, 16, 12, 4, 1)['KS'] == 1
    assert R.sq_launch(R.SQ_SIZES[-1], R.SQ_CAP) == dict(blocks=256, trips=5, beyond_cap=True) and R.sq_launch(R.SQSUM_SIZES[-1], R.SQSUM_CAP)['beyond_cap']
    assert R.unit_launch(1, 260) == dict(G=64, trips=2, idle_lanes=63, blocks=1, pixel_trips=1) and R.unit_launch(1, 12)['idle_lanes'] == 1
    assert R.gs_launch(2, 4, 3, 5)['straddles'] and R.gs_launch(2, 260, 2, 3)['trips'] == 2
    assert R.group_width(1) == 1 and R.group_width(3) == 4 and R.group_width(65) == 64


def test_compare_counts_every_element():
    ref, tol = np.array([1.0, np.nan, np.inf, 0.0]), np.array([1e-6, 0.0, 0.0, 0.0])
    assert R.compare(ref, ref, tol) == (True, 0.0)
    for i, v in enumerate((1.1, 0.0, 1e30, 1e-30)):
        got = ref.copy()
        got[i] = v
        assert R.compare(got, ref, tol)[0] is False
    assert R.compare(np.array([np.nan]), np.array([1.0]), 1.0)[0] is False
