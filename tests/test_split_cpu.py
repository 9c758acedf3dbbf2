"""tests/support/split_ref.py -- the bit-exact restatement of the operand-split passes (csrc/conv_v2.hip) that tests/test_gpu_split.py holds the
kernels to -- checked on its own, without a GPU: the two roundings, the range scalar, the decode bound and the two image layouts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import split_ref as R      # noqa: E402


def _all_finite_f16():
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    return h[np.isfinite(h) & (h != 0)]


def test_rtz16_truncates_every_fp16_interval():
    """For every finite fp16 v != 0: v is a fixed point, the next fp32 away from zero still rounds back to v (nearest-even would agree there;
    the LAST fp32 in front of the next fp16 value must too, where nearest-even would not), and the next fp32 toward zero gives the previous fp16."""
    v = _all_finite_f16()
    v32 = v.astype(np.float32)
    assert np.array_equal(R.rtz16(v32).view(np.uint16), v.view(np.uint16))
    away = np.nextafter(v32, np.where(v32 > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    assert np.array_equal(R.rtz16(away).view(np.uint16), v.view(np.uint16))
    with np.errstate(over='ignore'):                                        # (+-65504 steps to +-inf: left out below)
        nxt = np.nextafter(v, np.where(v > 0, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float32)
    inner = np.isfinite(nxt)
    last = np.nextafter(nxt[inner], np.float32(0))                          # one fp32 step in front of the next fp16 value
    assert np.array_equal(R.rtz16(last).view(np.uint16), v[inner].view(np.uint16))
    toward = np.nextafter(v32, np.float32(0))                               # one fp32 step inside the previous interval
    prev = np.nextafter(v, np.float16(0))
    assert np.array_equal(R.rtz16(toward).view(np.uint16), prev.view(np.uint16))


def test_rtz16_overflow_subnormals_and_specials():
    got = R.rtz16(np.array([70000.0, -70000.0, 65504.0, 65519.99, 65520.0, 65535.99, 3e38, -3e38], dtype=np.float32))
    assert got.tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0]
    tiny = np.float32(2.0 ** -24)
    got = R.rtz16(np.array([tiny, 1.75 * tiny, 0.99 * tiny, -1.75 * tiny, 0.0], dtype=np.float32))
    assert got.view(np.uint16).tolist() == [1, 1, 0, 0x8001, 0]              # subnormals kept, truncated; below the smallest one: 0
    got = R.rtz16(np.array([np.inf, -np.inf, np.nan], dtype=np.float32))
    assert np.isposinf(got[0]) and np.isneginf(got[1]) and np.isnan(got[2])


def test_range_mul_brings_amax_into_2_13_2_14():
    amax = [np.float32(2.0) ** k for k in range(-80, 81)]                    # exact powers of two ...
    amax += [np.nextafter(a, np.float32(0)) for a in amax]                   # ... and one ulp below them
    amax += [np.float32(1e-30), np.float32(1e30), np.float32(1.0), np.float32(3.0), np.float32(4.0), np.float32(16383.99), np.float32(16384.0)]
    for a in amax:
        m = R.range_mul(a)
        assert m.dtype == np.float32 and np.frexp(m)[0] == 0.5, (a, m)       # a power of two
        top = np.float64(a) * np.float64(m)
        assert 2.0 ** 13 <= top < 2.0 ** 14, (a, m, top)
    assert R.range_mul(np.float32(2.0)) == np.float32(2.0 ** 12) and R.range_mul(np.nextafter(np.float32(2.0), np.float32(0))) == np.float32(2.0 ** 13)
    for a in (0.0, -1.0, np.inf, -np.inf, np.nan, 3.1e38):
        assert R.range_mul(np.float32(a)) == np.float32(1.0), a
    assert R.range_mul(np.float32(2.0 ** -120)) == np.float32(2.0 ** 114)    # the exponent clamp (+-100)
    assert R.range_mul(np.float32(2.0 ** 120)) == np.float32(2.0 ** -86)


def _distribution(kind, n, rng):
    if kind == 'randn':
        return rng.standard_normal(n).astype(np.float32)
    if kind == 'heavy':
        return R.heavy_tailed(rng, n)
    return (rng.standard_normal(n) * 1e-20).astype(np.float32)


@pytest.mark.parametrize('lo_mul', [R.ACT_LO_MUL, R.W_LO_MUL])
@pytest.mark.parametrize('kind', ['randn', 'heavy', 'tiny'])
def test_decode_stays_within_decode_bound(kind, lo_mul):
    """2^20 elements per distribution, with a style factor (the second fp32 multiply): hi + lo / lo_mul against the float64 product, elementwise within
    decode_bound, no violation allowed."""
    rng = np.random.default_rng(len(kind) * 7 + int(lo_mul))
    n = 1 << 20
    x = _distribution(kind, n, rng)
    s = (1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    v = (x * s).astype(np.float32)
    mul = R.range_mul(np.abs(v).max())
    hi, lo = R.split(v, mul, lo_mul)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    a64 = x.astype(np.float64) * s.astype(np.float64) * np.float64(mul)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) / lo_mul - a64)
    bound = R.decode_bound(a64, lo_mul)
    ratio = float((err / bound).max())
    print(f'split decode {kind} lo_mul {lo_mul}: worst error / bound {ratio:.4f}')
    assert int((err > bound).sum()) == 0, ratio
    assert ratio > 0.05, 'the bound is far from what the split achieves: it would not notice a lost low piece'
    # a lost low piece IS noticed
    err_hi = np.abs(hi.astype(np.float64) - a64)
    assert int((err_hi > bound).sum()) > n // 4


@pytest.mark.parametrize('shape', [(1, 1, 1, 8, 8), (2, 3, 5, 24, 16), (3, 9, 7, 64, 64), (2, 4, 4, 136, 136)])
def test_activation_layout_round_trip(shape):
    """Every element of x[n, pixel, c] holds its own index: the image decodes back to it exactly, pitch ldx > C included."""
    N, H, W, ldx, C = shape
    x = R.index_operand((N, H, W, ldx))
    amax = x[..., :C].max()
    img, scale = R.split_activation_ref(x, C, None, amax)
    assert img.shape == (N, 2, C // 8, H * W, 8) and img.dtype == np.uint16
    dec = R.decode_activation(img, scale, N, C, H * W)
    assert np.array_equal(dec, x[..., :C].reshape(N, H * W, C).astype(np.float64))
    # one element, by hand: its high piece sits at [n][0][c / 8][pixel][c % 8]
    n, p, c = N - 1, H * W - 1, C - 3
    h = img.view(np.float16)[n, 0, c // 8, p, c % 8].astype(np.float64) + img.view(np.float16)[n, 1, c // 8, p, c % 8].astype(np.float64) / 2048.0
    assert h / float(scale) == float(x.reshape(N, H * W, ldx)[n, p, c])
    # power-of-two styles keep it exact; the style row is the image's own
    s = np.stack([np.float32(2.0) ** ((np.arange(C) + n) % 3 - 1) * (-1.0) ** (np.arange(C) + n) for n in range(N)]).astype(np.float32)
    img, scale = R.split_activation_ref(x, C, s, amax)
    dec = R.decode_activation(img, scale, N, C, H * W)
    assert np.array_equal(dec, x[..., :C].reshape(N, H * W, C).astype(np.float64) * s[:, None, :].astype(np.float64))
    assert scale == R.range_mul(np.float32(amax) * np.float32(2.0))


@pytest.mark.parametrize('shape', [(3, 16, 1, 0), (40, 32, 9, 0), (128, 48, 4, 24)])
def test_weight_layout_round_trip(shape):
    """Every element of w[o, tap * I + i] holds its own index: the image decodes back to it exactly, row pitch > T * I included."""
    O, I, T, extra = shape
    w = R.index_operand((O, T * I + extra))
    amax = w[:, :T * I].max()
    img, scale = R.split_weight_ref(w, O, I, T, amax)
    assert img.shape == (T, I // 16, 2, 2, O, 8) and img.dtype == np.uint16
    assert np.array_equal(R.decode_weight(img, scale, O, I, T), w[:, :T * I].astype(np.float64))
    o, tap, i = O - 1, T - 1, I - 11
    f = img.view(np.float16).astype(np.float64)
    chunk, koct, q = i // 16, (i // 8) % 2, i % 8
    assert (f[tap, chunk, 0, koct, o, q] + f[tap, chunk, 1, koct, o, q]) / float(scale) == float(w[o, tap * I + i])
