"""Bit-exact restatement (numpy, no GPU) of the operand-split passes of csrc/conv_v2.hip -- split_act_kernel, split_act_lds_kernel<64 | 128>,
split_w_kernel, split_w_batched_kernel -- written from their contract, not from their code:

  range scalar   mul = range_mul(amax): the power of two that brings amax into [2^13, 2^14); 1 when amax is not in (0, 3e38)
  one element    a = fl32(v * mul);  hi = rtz16(a);  lo = rne16(clamp((a - hi) * lo_mul, +-65504))       (a - hi is exact in fp32)
                 lo_mul = 2048 for activations, 1 for weights;  the element decodes as (hi + lo / lo_mul) / mul
  activations    v = fl32(x * s[n, c]) (one fp32 multiply in front of the range multiply), mul = range_mul(fl32(x_amax * smax));
                 image [N][2 piece][C/8][H*W][8] fp16
  weights        image [T][I/16][2 piece][2 koct][O][8] fp16, element w[o, tap * I + (2 chunk + koct) * 8 + q]

The split is elementwise, order-free and deterministic, so the images a kernel writes are compared with these BYTE FOR BYTE (tests/test_gpu_split.py);
tests/test_split_cpu.py checks this file on its own.  All arithmetic below is numpy float32 / float16 (IEEE, round to nearest even, subnormals kept)
except where a rounding is restated by hand (rtz16).
"""
import numpy as np

F16_MAX = np.float32(65504.0)
ACT_LO_MUL, W_LO_MUL = 2048.0, 1.0


def rtz16(a):
    """fp32 -> fp16 rounded toward zero: finite overflow gives +-65504 (never inf), fp16 subnormals are kept, +-inf and NaN pass through."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(over='ignore'):
        h = a.astype(np.float16)                                        # nearest-even: at most one fp16 step away from the truncation
    away = np.abs(h.astype(np.float32)) > np.abs(a)                     # (inf for |a| >= 65520: also "away")
    away &= np.isfinite(a)
    h = np.where(away, np.nextafter(h, np.float16(0)), h)               # nextafter(+-inf, 0) = +-65504
    return h.astype(np.float16)


def rne16(a):
    """fp32 -> fp16, round to nearest even (what a plain conversion does)."""
    with np.errstate(over='ignore'):
        return np.asarray(a, dtype=np.float32).astype(np.float16)


def range_mul(amax):
    """The power of two 2^(14 - e), frexp(amax) = (m, e), e clamped to +-100; 1.0 when amax is not in (0, 3e38)."""
    amax = np.float32(amax)
    if not (amax > np.float32(0)) or not (amax < np.float32(3.0e38)):
        return np.float32(1.0)
    _, e = np.frexp(amax)
    e = int(min(100, max(-100, int(e))))
    return np.float32(np.ldexp(np.float32(1.0), 14 - e))


def split(v, mul, lo_mul):
    """(hi, lo) fp16 arrays of the fp32 array v."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        a = (v * np.float32(mul)).astype(np.float32)
        hi = rtz16(a)
        r = (a - hi.astype(np.float32)).astype(np.float32)
        lo = rne16(np.clip((r * np.float32(lo_mul)).astype(np.float32), -F16_MAX, F16_MAX))
    return hi, lo


def _u16(h):
    return np.ascontiguousarray(h).view(np.uint16)


def split_activation_ref(x_nhwc, C, s, x_amax, s_amax=None):
    """x_nhwc [N, H, W, ldx] fp32 (channels 0 .. C-1 are read), s [N, C] | None, x_amax, s_amax | None (None with s given: max|s| over all of s)
    -> (uint16 image [N, 2, C/8, H*W, 8], float32 scale)."""
    x = np.asarray(x_nhwc, dtype=np.float32)
    N, H, W, ldx = x.shape
    assert C % 8 == 0 and C <= ldx
    v = x[..., :C].reshape(N, H * W, C)
    smax = np.float32(1.0)
    if s is not None:
        s = np.asarray(s, dtype=np.float32).reshape(N, C)
        v = (v * s[:, None, :]).astype(np.float32)
        smax = np.float32(np.abs(s).max())
    if s_amax is not None:
        smax = np.float32(s_amax)
    with np.errstate(over='ignore'):
        mul = range_mul(np.float32(x_amax) * smax)
    hi, lo = split(v, mul, ACT_LO_MUL)
    img = np.stack([hi, lo], axis=1)                                    # [N, 2, HW, C]
    img = img.reshape(N, 2, H * W, C // 8, 8).transpose(0, 1, 3, 2, 4)  # [N, 2, C/8, HW, 8]
    return _u16(img), mul


def split_weight_ref(w, O, I, T, amax):
    """w [O, w_row >= T*I] fp32 packed (tap major, input channel minor) -> (uint16 image [T, I/16, 2 piece, 2 koct, O, 8], float32 scale)."""
    w = np.asarray(w, dtype=np.float32)
    assert w.shape[0] == O and w.shape[1] >= T * I and I % 16 == 0
    mul = range_mul(amax)
    hi, lo = split(w[:, :T * I], mul, W_LO_MUL)
    img = np.stack([hi, lo], axis=0).reshape(2, O, T, I // 16, 2, 8)    # [piece, o, tap, chunk, koct, q]
    img = img.transpose(2, 3, 0, 4, 1, 5)                               # [tap, chunk, piece, koct, o, q]
    return _u16(img), mul


def _f16(img):
    return np.ascontiguousarray(np.asarray(img)).view(np.float16).astype(np.float64)


def decode_activation(img, scale, N, C, HW, lo_mul=ACT_LO_MUL):
    """Image [N][2][C/8][HW][8] (uint16 / int16 bit patterns or float16) -> float64 [N, HW, C] = (hi + lo / lo_mul) / scale."""
    v = _f16(img).reshape(N, 2, C // 8, HW, 8)
    x = (v[:, 0] + v[:, 1] / lo_mul) / float(scale)
    return x.transpose(0, 2, 1, 3).reshape(N, HW, C)


def decode_weight(img, scale, O, I, T, lo_mul=W_LO_MUL):
    """Image [T][I/16][2][2][O][8] -> float64 [O, T*I]."""
    v = _f16(img).reshape(T, I // 16, 2, 2, O, 8)
    x = (v[:, :, 0] + v[:, :, 1] / lo_mul) / float(scale)               # [tap, chunk, koct, o, q]
    return x.transpose(3, 0, 1, 2, 4).reshape(O, T * I)


def ulp16(a):
    """Spacing of fp16 at |a|: 2^(max(floor(log2|a|), -14) - 10)."""
    _, e = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))            # |a| = m 2^e, m in [0.5, 1): floor(log2|a|) = e - 1  (a = 0: e = 0, below the floor anyway)
    e = np.where(np.asarray(a) == 0, -1000, e - 1)
    return np.ldexp(1.0, np.maximum(e, -14) - 10)


def decode_bound(a64, lo_mul):
    """Elementwise bound on |hi + lo / lo_mul - a64|, a64 = the exact scaled element (float64): 2^-11 ulp16(a) (nearest-even rounding of the low
    piece, whose magnitude is below ulp16(a) * lo_mul) + 2^-25 / lo_mul (half a step of the fp16 subnormal grid, where the low piece lands there)
    + 2^-23 |a| (the two fp32 multiplies, 2^-24 relative each)."""
    a64 = np.asarray(a64, dtype=np.float64)
    return 2.0 ** -11 * ulp16(a64) + 2.0 ** -25 / lo_mul + 2.0 ** -23 * np.abs(a64)


# ---- operands of the tests ------------------------------------------------------------------------------------------------------------
def heavy_tailed(rng, shape):
    """randn * 10^U(-8, 0): eight decades, so that the low pieces of small elements matter."""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-8.0, 0.0, shape)).astype(np.float32)


def index_operand(shape):
    """Every element holds its own linear index + 1 (< 2^22: exact in the two pieces, 11 bits each)."""
    n = int(np.prod(shape))
    assert n < (1 << 22)
    return (np.arange(n, dtype=np.float64) + 1.0).reshape(shape).astype(np.float32)
