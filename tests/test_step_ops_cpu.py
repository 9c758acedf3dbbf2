"""The yardstick of tests/test_gpu_step_ops.py, checked without a GPU: tests/support/step_ref.py equals torch autograd on the reference's
regulariser expression (w_projector.py:221-237) and torch.optim.Adam in float64; every structured case gives every pyramid level a share of the
value and of |g|max at least 100 times the derived tolerance; the comparisons of the GPU file reject nine kinds of wrong result; and the bounds
accept the same operations evaluated in fp32 numpy in two summation orders."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import step_ref as R      # noqa: E402

SENS_RES = (64, 128, 512)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def _reg_torch(x, scale):
    noise = x[None, None]
    reg = 0.0
    while True:
        reg = reg + (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
        reg = reg + (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
        if noise.shape[2] <= 8:
            break
        noise = F.avg_pool2d(noise, kernel_size=2)
    return reg * scale


@pytest.mark.parametrize('res', [1, 2, 4, 8, 16, 64, 512])
def test_reg_ref_equals_autograd_of_the_reference_expression(res):
    for maker, scale in ((R.structured_case, 1.0), (R.randn_case, 1e5)):
        x = maker(res, 3)
        ref = R.reg_ref(x, scale)
        t = torch.from_numpy(x).double().requires_grad_(True)
        val = _reg_torch(t, scale)
        g, = torch.autograd.grad(val, t)
        assert abs(ref['total'] - float(val)) <= 1e-12 * abs(float(val))
        assert float(np.abs(ref['grad'] - g.numpy()).max()) <= 1e-12 * float(g.abs().max())
        assert len(ref['values']) == R.levels(res) and float(g.abs().max()) > 0


def test_adam_ref_equals_torch_adam_in_float64_over_five_steps():
    """torch gets the fp32-rounded lr, betas and eps the kernel gets (the only difference between adam_ref and Adam(0.9, 0.999, 1e-8) in float64),
    both gradients summed, and a learning rate that changes between the steps."""
    f = lambda v: float(np.float32(v))
    p0, g, g2, m0, v0 = R.adam_state(5000, 5, gmag=(1e-6, 1e2))
    p = torch.from_numpy(p0).double().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=f(0.1), betas=(f(0.9), f(0.999)), eps=f(1e-8))
    rp, rm, rv = p0.astype(np.float64), np.zeros(5000), np.zeros(5000)
    rng = np.random.default_rng(0)
    for t in range(5):
        lr = 0.1 if t < 2 else 3e-4
        ga, gb = rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 2, 5000), rng.standard_normal(5000)
        opt.param_groups[0]['lr'] = f(lr)
        p.grad = torch.from_numpy(ga + gb)
        opt.step()
        rp, rm, rv = R.adam_ref(rp, ga, gb, rm, rv, t, lr)
        st = opt.state[p]
        for a, b in ((rp, p.detach().numpy()), (rm, st['exp_avg'].numpy()), (rv, st['exp_avg_sq'].numpy())):
            assert float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max()), t
    assert float(np.abs(rp - p0).max()) > 0.1


def test_normalize_ref_is_the_two_pass_form():
    x = R.norm_case(64, 8.0)
    y = R.normalize_ref(x)
    assert abs(float(y.mean())) < 1e-12 and abs(float((y * y).mean()) - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ the share condition
@pytest.mark.parametrize('res,seed', R.all_structured_cases(), ids=lambda v: str(v))
def test_every_level_of_every_structured_case_carries_a_hundred_tolerances(res, seed):
    for scale in R.SCALES:
        _, ref = R.struct_ref(res, seed, scale)
        sv, sg, tv, tg = R.shares(ref)
        print(f'shares {res}^2 seed {seed} scale {scale:g}: value {" ".join(f"{s:.3f}" for s in sv)} | gmax {" ".join(f"{s:.3f}" for s in sg)} | '
              f'tol / value {tv:.2e}, tol / gmax {tg:.2e}')
        assert min(sv) >= 100 * tv, (res, seed, scale, sv, tv)
        assert min(sg) >= 100 * tg, (res, seed, scale, sg, tg)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _refs(scale=1.0):
    return [R.struct_ref(r, 100, scale)[1] for r in SENS_RES]


@pytest.mark.parametrize('k', range(len(SENS_RES)), ids=[str(r) for r in SENS_RES])
def test_wrong_regulariser_gradients_are_rejected(k):
    refs = _refs()
    ref = refs[k]
    x = R.struct_ref(SENS_RES[k], 100, 1.0)[0].astype(np.float64)
    total = sum(r['total'] for r in refs)
    good = [r['grad'] for r in refs]
    assert R.compare_reg(total, good, refs)[0]

    def rejected(g):
        gs = list(good)
        gs[k] = g
        return not R.compare_reg(total, gs, refs)[0]
    nl = len(ref['grads'])
    for l in range(nl):
        assert rejected(ref['grad'] - ref['grads'][l]), f'level {l} dropped'
        assert rejected(ref['grad'] - 2 * ref['grads'][l]), f'level {l} with the wrong sign'
    assert rejected(sum(g * 2.0 ** l for l, g in enumerate(ref['grads']))), '2^-l for 4^-l'
    # the left neighbour of column 0 taken from the row above (flat index i - 1) at level 0
    n = x.size
    left = np.roll(x.ravel(), 1).reshape(x.shape)
    mx = ref['m'][0][0]
    wrong = ref['grad'] + 2.0 / n * mx * (left - np.roll(x, 1, 1))
    assert rejected(wrong), 'wrap to the wrong row'
    # a level that reads the wrong ancestor (x >> l of the neighbouring column pair) -- coarsest level shifted by one level-0 column
    assert rejected(ref['grad'] - ref['grads'][nl - 1] + np.roll(ref['grads'][nl - 1], 1, 1)), 'wrong ancestor'


def test_a_total_that_omits_one_buffer_is_rejected():
    for scale in R.SCALES:
        refs = _refs(scale)
        total = sum(r['total'] for r in refs)
        for k in range(len(refs)):
            assert not R.compare_reg(total - refs[k]['total'], None, refs)[0], (scale, SENS_RES[k])
    refs = [R.struct_ref(r, s, 1.0)[1] for r, s in R.BANK17]
    total = sum(r['total'] for r in refs)
    for k in range(len(refs)):
        assert not R.compare_reg(total - refs[k]['total'], None, refs)[0], R.BANK17[k]


def _adam_ok(got, ref):
    return all(R.compare(got[i], ref[i], ref[3 + i])[0] for i in range(3))


def test_wrong_adam_updates_are_rejected():
    for lr in (0.1, 3e-4):
        for t in (1, 999):
            p, g, g2, m, v = R.adam_state(12800, 7)
            ref = R.adam_ref(p, g, g2, m, v, t, lr, tol=True)
            assert _adam_ok(ref[:3], ref)
            tail = [a.copy() for a in ref[:3]]
            for a, old in zip(tail, (p, m, v)):
                a[3 * R.ADAM_CHUNK:] = old[3 * R.ADAM_CHUNK:]
            assert not R.compare(tail[0], ref[0], ref[3])[0], 'last partial chunk dropped (p)'
            assert not R.compare(tail[1], ref[1], ref[4])[0] and not R.compare(tail[2], ref[2], ref[5])[0], 'last partial chunk dropped (m, v)'
            assert not R.compare(R.adam_ref(p, g, g2, m, v, t - 1, lr)[0], ref[0], ref[3])[0], 't where t + 1 belongs'
            assert not R.compare(R.adam_ref(p, g, None, m, v, t, lr)[0], ref[0], ref[3])[0], 'second gradient ignored'
            # bc2s without the square root
            b2 = float(np.float32(0.999))
            bc2 = 1.0 - b2 ** (t + 1.0)
            p1, m1, v1 = ref[:3]
            b1 = float(np.float32(0.9))
            wrong = p.astype(np.float64) - float(np.float32(lr)) / (1 - b1 ** (t + 1.0)) * m1 / (np.sqrt(v1) / bc2 + float(np.float32(1e-8)))
            assert not R.compare(wrong, p1, ref[3])[0], 'bc2 without the square root'


def test_wrong_normalisations_are_rejected():
    for form in ('block', 'multi', 'adam'):
        for res in (64, 128, 512):
            x = R.norm_case(res, 1.0).astype(np.float64)
            ref, tol = R.normalize_ref(x), R.normalize_tol(x, form)
            assert R.compare(ref, ref, tol)[0]
            about0 = (x - x.mean()) / math.sqrt(float((x * x).mean()))
            assert not R.compare(about0, ref, tol)[0], 'variance about 0'
            assert not R.compare(x / x.std(), ref, tol)[0], 'mean not subtracted'
    # a renormalised Adam leaf whose moments miss the variance's  - mean^2
    p, g, g2, m, v = R.adam_state(128 * 128, 9, gmag=(1e-3, 1.0), mean=1.0)
    p1, _, _, tp, _, _ = R.adam_ref(p, g, g2, m, v, 3, 0.1, tol=True)
    ref, tol = R.adam_norm_ref(p1, tp)
    assert not R.compare((p1 - p1.mean()) / math.sqrt(float((p1 * p1).mean())), ref, tol)[0]


# ------------------------------------------------------------------------------------------------------------------ the bounds admit fp32
def _sum32(a, order, chunk):
    """fp32 sum of a flat fp32 array in the kernels' partition: chunks of `chunk` elements, each summed by `order`, the chunk sums added one after
    the other (the atomics)."""
    t = np.float32(0.0)
    for lo in range(0, a.size, chunk):
        c = a[lo:lo + chunk]
        t = np.float32(t + (np.cumsum(c, dtype=np.float32)[-1] if order == 'cumsum' else np.sum(c, dtype=np.float32)))
    return t


def _reg_fp32(x, scale, order):
    f = np.float32
    v = x.astype(f)
    res = v.shape[0]
    nl = R.levels(res)
    g = np.zeros_like(v)
    total = f(0.0)
    for l in range(nl):
        n = f(v.size)
        mx = f(_sum32((v * np.roll(v, 1, 1)).ravel(), order, R.CHUNK) / n)
        my = f(_sum32((v * np.roll(v, 1, 0)).ravel(), order, R.CHUNK) / n)
        w = f(f(f(2.0) / n * f(scale)) / f(1 << (2 * l)))
        lr_, ud = R._nb(v)
        g = (g + R._up((f(mx * w) * lr_ + f(my * w) * ud).astype(f), 1 << l)).astype(f)
        total = f(total + f(mx * mx + my * my))
        if l + 1 < nl:
            v = R._pool(v).astype(f)
    return f(total * f(scale)), g


@pytest.mark.parametrize('res', [8, 64, 128, 512, 1024])
def test_the_regulariser_bound_accepts_fp32_numpy_in_two_orders(res):
    for maker in (R.structured_case, R.randn_case):
        for scale in R.SCALES:
            x = maker(res, 100)
            ref = R.struct_ref(res, 100, scale)[1] if maker is R.structured_case else R.reg_ref(x, scale)
            for order in ('cumsum', 'sum'):
                total, g = _reg_fp32(x, scale, order)
                ok, worst, what = R.compare_reg(total, [g], [ref])
                print(f'fp32 numpy regulariser {maker.__name__} {res}^2 scale {scale:g} {order}: worst err/tol {worst:.3f} ({what})')
                assert ok, (res, scale, order, worst, what)


@pytest.mark.parametrize('res', [2, 4, 64, 512])
def test_the_normalise_bound_accepts_fp32_numpy_in_two_orders(res):
    f = np.float32
    for ratio in R.NORM_MEANS:
        x = R.norm_case(res, ratio)
        ref = R.normalize_ref(x)
        n = f(x.size)
        for order in ('cumsum', 'sum'):
            for form, chunk in (('block', x.size), ('multi', R.NORM_CHUNK), ('adam', R.ADAM_CHUNK)):
                if form == 'block':            # two passes; a thread's strided terms one after the other, then the block's tree
                    cols = x.ravel().reshape(-1, min(R.NT, x.size))
                    s32 = lambda a: (np.cumsum(a, axis=0, dtype=f)[-1] if order == 'cumsum' else a.sum(0, dtype=f)).sum(dtype=f)
                    mean = f(s32(cols) / n)
                    d = (cols - mean).astype(f)
                    got = (d * f(f(1.0) / np.sqrt(f(s32(d * d) / n)))).astype(f).reshape(x.shape)
                else:                          # one pass: sum and sum of squares
                    mean = f(_sum32(x.ravel(), order, chunk) / n)
                    var = f(f(_sum32((x * x).ravel(), order, chunk) / n) - f(mean * mean))
                    got = ((x - mean).astype(f) * f(f(1.0) / np.sqrt(var))).astype(f)
                ok, worst = R.compare(got, ref, R.normalize_tol(x, form))
                print(f'fp32 numpy normalise {res}^2 mean/std {ratio:g} {form} {order}: worst err/tol {worst:.3f}')
                assert ok, (res, ratio, form, order, worst)


@pytest.mark.parametrize('t', [0, 1, 999, 9999])
def test_the_adam_bound_accepts_fp32_numpy(t):
    f = np.float32
    for lr in (0.1, 3e-4):
        p, g, g2, m, v = R.adam_state(12800, 11 + t)
        ref = R.adam_ref(p, g, g2, m, v, t, lr, tol=True)
        b1, b2, eps, t1 = f(0.9), f(0.999), f(1e-8), f(t + 1)
        gg = g + g2
        m1 = m + (gg - m) * (f(1) - b1)
        v1 = v * b2 + (f(1) - b2) * gg * gg
        bc1, bc2s = f(1) - np.power(b1, t1), np.sqrt(f(1) - np.power(b2, t1))
        p1 = p - f(f(lr) / bc1) * m1 / (np.sqrt(v1) / bc2s + eps)
        assert p1.dtype == f and m1.dtype == f and v1.dtype == f
        worst = [R.compare(a, ref[i], ref[3 + i]) for i, a in enumerate((p1, m1, v1))]
        print(f'fp32 numpy Adam t {t} lr {lr:g}: worst err/tol p {worst[0][1]:.3f} m {worst[1][1]:.3f} v {worst[2][1]:.3f}')
        assert all(w[0] for w in worst), (t, lr, worst)
