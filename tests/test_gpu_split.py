"""The operand-split passes of csrc/conv_v2.hip on their own -- split_act_kernel, split_act_lds_kernel<64 | 128>, split_w_kernel, split_w_batched_kernel (ranges
from absmax_batched_kernel) through hipops.split_activation / split_weight / split_weights_batched -- against the bit-exact restatement of
tests/support/split_ref.py (checked in tests/test_split_cpu.py).  The split is elementwise, order-free and deterministic:

  A - C   image bytes (torch.equal on the int16 view) and the scale (==), no tolerance anywhere;
  D       the fused producers (upconv_epilogue_fwd(split_in_scale=), torgb_dgrad_act_split) against the same restatement of the fp32 tensor they wrote;
  E       the exact-integer class through the stride-1 consumers (conv_v2 and its split-K / KH = 2 forms, conv_v3, conv_ws, conv_wgrad_v2): operands whose high
          pieces are exact and low pieces zero, so every product and partial sum is a multiple of 0.5 below 2^22 and ANY summation order must return the
          float64 result bit for bit -- a failure there is a lost, doubled or misplaced term, not a rounding.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import split_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CL = torch.channels_last


def _dev_image(ref_u16):
    return torch.from_numpy(np.ascontiguousarray(ref_u16).view(np.int16).reshape(-1)).to(DEV)


def _assert_image(simg, ref_u16, ref_scale, names, what):
    """Image bytes equal (int16 view) and scale ==; on a mismatch: the count and the first differing index in the image's own layout."""
    torch.cuda.synchronize()
    got_scale = float(simg.scale)
    assert got_scale == float(ref_scale), f'{what}: scale {got_scale!r}, expected {float(ref_scale)!r}'
    got = simg.data.view(torch.int16)
    want = _dev_image(ref_u16)
    assert got.numel() == want.numel(), (what, got.numel(), want.numel())
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).flatten()
        i = np.unravel_index(int(bad[0]), ref_u16.shape)
        g, w = int(got[bad[0]]) & 0xffff, int(want[bad[0]]) & 0xffff
        raise AssertionError(f'{what}: {bad.numel()} of {got.numel()} halves differ; first at [{names}] = {tuple(int(k) for k in i)}: '
                             f'got 0x{g:04x} ({float(np.uint16(g).view(np.float16))!r}), expected 0x{w:04x} ({float(np.uint16(w).view(np.float16))!r})')


ACT_NAMES = 'n, piece, octet, pixel, lane'
W_NAMES = 'tap, chunk, piece, koct, o, lane'


# ====================================================================================================================== A. split_activation
# (N, H, W, cx = pitch, C)
ACT_SHAPES = [
    (1, 8, 8, 128, 128), (3, 9, 7, 256, 256), (2, 5, 13, 136, 128),        # lds<128>: 63 pixels per image (a 64-pixel tile straddles two images, ragged last tile), two channel chunks, ldx > C
    (3, 9, 7, 64, 64), (1, 1, 1, 72, 64), (5, 3, 5, 64, 64),               # lds<64>; (5, 3, 5): a tile holds pixels of five images and N * C = 320 > 256
    (2, 9, 33, 8, 8), (1, 16, 16, 72, 72), (1, 4, 4, 136, 136),            # thread per pixel: 594 pixels; 9 octets over 2 groups (5 + 4); 17 octets over 4 groups (5, 5, 5, 2)
    (3, 17, 16, 192, 192), (1, 1, 1, 40, 40),                              # 816 pixels x 24 octets over 4 groups; one pixel
]
SCALE_MODES = ['plain', 'styles_amax', 'styles_own_max']
OPERANDS = ['randn', 'heavy', 'index', 'zeros', 'amax_pow2', 'amax_loose']


def _styles(rng, N, C):
    """Negative and positive styles, a different row per image; the largest magnitude sits in the last row, behind index 256 where N * C allows."""
    s = (1.0 + 0.6 * rng.standard_normal((N, C))).astype(np.float32)
    s[rng.random((N, C)) < 0.3] *= -1.0
    s[N - 1, C - 3] = -3.75
    return s


def _act_operand(kind, rng, shape):
    """(x [N, H, W, cx] fp32, factor on max|x| for the x_amax handed to the kernel)."""
    N, H, W, cx, C = shape
    if kind == 'heavy':
        x = R.heavy_tailed(rng, (N, H, W, cx))
    elif kind == 'index':
        x = R.index_operand((N, H, W, cx))
    elif kind == 'zeros':
        x = np.zeros((N, H, W, cx), np.float32)
        x[..., C:] = 7.0                                                    # (pitch columns are not part of the operand)
    else:
        x = rng.standard_normal((N, H, W, cx)).astype(np.float32)
    if kind == 'amax_pow2':
        x[..., :C] = np.clip(x[..., :C], -2.0, 2.0)
        x[N - 1, H - 1, W - 1, C - 1] = -2.0                                # max|x| = 2 exactly: the lower edge of a binade
    return x, (256.0 if kind == 'amax_loose' else 1.0)


def _run_split_activation(x, C, s, x_amax, s_amax):
    from inv3d_amd import hipops as H
    N, Hh, W, cx = x.shape
    xd = torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2)                    # [N, cx, H, W] channels_last view of the NHWC array
    sd = torch.from_numpy(s).to(DEV) if s is not None else None
    xa = torch.tensor([x_amax], dtype=torch.float32, device=DEV)
    sa = torch.tensor([s_amax], dtype=torch.float32, device=DEV) if s_amax is not None else None
    return H.split_activation(xd, xa, in_scale=sd, s_amax=sa, C=C)


@pytest.mark.parametrize('mode', SCALE_MODES)
@pytest.mark.parametrize('shape', ACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_split_activation_bit_equal(shape, mode):
    """Every dispatch path x every scale mode, each with all six operands: randn, heavy-tailed, index-carrying, all zeros (scale 1 without styles), max|x| an
    exact power of two, x_amax 2^8 too large (the carried-bound case of torgb_dgrad_act_split)."""
    N, Hh, W, cx, C = shape
    rng = np.random.default_rng(N * 1000 + Hh * 100 + W * 10 + C)
    s = _styles(rng, N, C) if mode != 'plain' else None
    for kind in OPERANDS:
        x, loose = _act_operand(kind, rng, shape)
        x_amax = float(np.abs(x[..., :C]).max()) * loose
        s_amax = float(np.abs(s).max()) if mode == 'styles_amax' else None
        ref, scale = R.split_activation_ref(x, C, s, x_amax, s_amax)
        simg = _run_split_activation(x, C, s, x_amax, s_amax)
        _assert_image(simg, ref, scale, ACT_NAMES, f'split_activation {shape} {mode} {kind}')
        if kind == 'zeros':
            assert bool((simg.data == 0).all()) and float(simg.scale) == 1.0      # (0 x a negative style is -0: still zero)


@pytest.mark.parametrize('shape', [(3, 9, 7, 256, 256), (3, 9, 7, 64, 64), (3, 17, 16, 192, 192)], ids=lambda s: 'x'.join(map(str, s)))
def test_split_activation_stale_range_saturates(shape):
    """x_amax 2^4 too small (a stale range), one shape per kernel: elements that do not saturate stay bit-equal to the restatement; saturating ones have
    hi = +-65504 with the element's sign; nothing in the image is inf or NaN.
    Found on the MI355X (2, 135 and 14 saturating elements at the three shapes): the hardware agrees with the restatement on the saturating elements too -- the
    packed round-toward-zero conversion returns the largest finite fp16 on finite overflow, as round-toward-zero does (IEEE 754-2008, 7.4), and the low piece is
    the clamp's +-65504 -- so the whole image is asserted equal as well."""
    N, Hh, W, cx, C = shape
    rng = np.random.default_rng(C + 5)
    x = rng.standard_normal((N, Hh, W, cx)).astype(np.float32)
    s = _styles(rng, N, C)
    x_amax = float(np.abs(x[..., :C]).max()) / 16.0
    s_amax = float(np.abs(s).max())
    ref, scale = R.split_activation_ref(x, C, s, x_amax, s_amax)
    simg = _run_split_activation(x, C, s, x_amax, s_amax)
    torch.cuda.synchronize()
    assert float(simg.scale) == float(scale)
    got = simg.data.view(torch.int16).cpu().numpy().view(np.uint16).reshape(ref.shape)
    gf = got.view(np.float16)
    assert np.isfinite(gf).all(), f'{int((~np.isfinite(gf)).sum())} non-finite halves in the image'
    a = (x[..., :C].reshape(N, Hh * W, C) * s[:, None, :]).astype(np.float32).astype(np.float64) * float(scale)       # scaled elements
    a = a.reshape(N, Hh * W, C // 8, 8).transpose(0, 2, 1, 3)                                                       # [n, octet, pixel, lane]
    sat = np.abs(a) >= 65504.0
    assert 0 < int(sat.sum()) < sat.size // 2
    for piece in (0, 1):
        assert np.array_equal(got[:, piece][~sat], ref[:, piece][~sat]), f'piece {piece}: elements that do not saturate differ from the restatement'
    assert np.array_equal(gf[:, 0][sat].astype(np.float64), np.where(a[sat] > 0, 65504.0, -65504.0)), 'saturating elements: hi is not +-65504 with the right sign'
    print(f'stale range {shape}: {int(sat.sum())} saturating elements; whole image equal to the restatement: {np.array_equal(got, ref)}')
    assert np.array_equal(got, ref)


# ====================================================================================================================== B. split_weight
W_SHAPES = [(128, 16, 9), (64, 48, 1), (3, 16, 1), (128, 512, 9), (192, 80, 4), (40, 32, 9)]          # (O, I, T)
W_OPERANDS = ['randn', 'heavy', 'index', 'zeros']


def _w_operand(kind, rng, O, I, T, extra=0):
    if kind == 'heavy':
        w = R.heavy_tailed(rng, (O, T * I + extra))
    elif kind == 'index':
        w = R.index_operand((O, T * I + extra))
    elif kind == 'zeros':
        w = np.zeros((O, T * I + extra), np.float32)
    else:
        w = (rng.standard_normal((O, T * I + extra)) / math.sqrt(I * T)).astype(np.float32)
    return w


@pytest.mark.parametrize('kind', W_OPERANDS)
@pytest.mark.parametrize('shape', W_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_split_weight_bit_equal(shape, kind):
    from inv3d_amd import hipops as H
    O, I, T = shape
    rng = np.random.default_rng(O + 7 * I + T)
    w = _w_operand(kind, rng, O, I, T)
    ref, scale = R.split_weight_ref(w, O, I, T, np.abs(w).max())
    _assert_image(H.split_weight(torch.from_numpy(w).to(DEV), O, I, T), ref, scale, W_NAMES, f'split_weight {shape} {kind}')


@pytest.mark.parametrize('kind', ['randn', 'index'])
@pytest.mark.parametrize('shape', [(40, 32, 9), (128, 16, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_split_weight_row_view_of_a_wider_matrix(shape, kind):
    """w_row > T * I: the rows are a strided view of a wider matrix whose other columns hold LARGER values -- they are neither weights nor part of the range."""
    from inv3d_amd import hipops as H
    O, I, T = shape
    rng = np.random.default_rng(O + I)
    wide = _w_operand(kind, rng, O, I, T, extra=24)
    wide[:, T * I:] = 1.0e6
    wide[O - 1, T * I - 1] *= 3.0                                          # the largest weight sits in the last row
    view = torch.from_numpy(wide).to(DEV)[:, :T * I]
    assert view.stride(0) == T * I + 24 and not view.is_contiguous()
    ref, scale = R.split_weight_ref(wide, O, I, T, np.abs(wide[:, :T * I]).max())
    _assert_image(H.split_weight(view, O, I, T), ref, scale, W_NAMES, f'split_weight {shape} {kind}, row pitch {T * I + 24}')


@pytest.mark.parametrize('shape', [(128, 16, 3), (192, 80, 1), (32, 32, 3), (64, 48, 3)], ids=lambda s: 'x'.join(map(str, s)))     # (both O and I: multiples of 16)
def test_split_weight_of_packed_forward_and_adjoint_matrices(shape):
    """[O, I, k, k] weights through pack_weight_fwd and pack_weight_adj (roles of O and I swapped): each image is the restatement of the same packed matrix,
    and decodes to the weight it was packed from at [o, i, tap]."""
    from inv3d_amd import hipops as H
    O, I, k = shape
    rng = np.random.default_rng(O * 3 + I)
    wt = torch.from_numpy((rng.standard_normal((O, I, k, k)) / math.sqrt(I * k * k)).astype(np.float32)).to(DEV)
    for pack, rows, cols in ((H.pack_weight_fwd, O, I), (H.pack_weight_adj, I, O)):
        wp = pack(wt)
        wn = wp.cpu().numpy()
        ref, scale = R.split_weight_ref(wn, rows, cols, k * k, np.abs(wn).max())
        simg = H.split_weight(wp, rows, cols, k * k)
        _assert_image(simg, ref, scale, W_NAMES, f'split_weight of {pack.__name__} {shape}')
        dec = R.decode_weight(simg.data.view(torch.int16).cpu().numpy(), float(simg.scale), rows, cols, k * k).reshape(rows, k, k, cols)
        want = wt.double().cpu().numpy()
        want = want.transpose(0, 2, 3, 1) if pack is H.pack_weight_fwd else want.transpose(1, 2, 3, 0)
        a64 = want * float(simg.scale)
        assert int((np.abs(dec * float(simg.scale) - a64) > R.decode_bound(a64, R.W_LO_MUL)).sum()) == 0


# ====================================================================================================================== C. split_weights_batched
def _batch_list(rng, second=False):
    """[(name, matrix fp32 numpy, O, I, T)]: the six shapes + two all-zero matrices."""
    mats = []
    for k, (O, I, T) in enumerate(W_SHAPES):
        kind = ('randn', 'heavy', 'index')[k % 3]
        w = _w_operand(kind, rng, O, I, T)
        if second:
            w = (w * np.float32(0.013)).astype(np.float32) if kind != 'index' else w[::-1].copy()
        mats.append((w, O, I, T))
    for O, I, T in ((16, 16, 1), (128, 32, 9)):
        mats.append((np.zeros((O, T * I), np.float32), O, I, T))
    return mats


def _assert_batch(H, dev_mats, np_mats, what):
    imgs = H.split_weights_batched(dev_mats)
    assert len(imgs) == len(np_mats)
    for k, ((w, O, I, T), simg) in enumerate(zip(np_mats, imgs)):
        ref, scale = R.split_weight_ref(w, O, I, T, np.abs(w).max())
        _assert_image(simg, ref, scale, W_NAMES, f'{what}: matrix {k} {(O, I, T)}')
        one = H.split_weight(dev_mats[k][0], O, I, T)
        assert float(one.scale) == float(simg.scale) and torch.equal(one.data.view(torch.int16), simg.data.view(torch.int16)), f'{what}: matrix {k} differs from split_weight'
        if not w.any():
            assert float(simg.scale) == 1.0 and bool((simg.data == 0).all())


@pytest.mark.parametrize('reps', [1, 4], ids=['one_group', 'past_batch_max'])
def test_split_weights_batched_bit_equal(reps):
    """The six shapes + two all-zero matrices in one call; the same list four times (32 matrices > SPLIT_W_BATCH_MAX: the grouping loop runs twice).  Then new
    weights (smaller ranges) in the SAME tensors: the second result follows the second weights -- the range accumulator is an atomicMax into a buffer the
    wrapper zeroes."""
    from inv3d_amd import hipops as H, _lib as L
    rng = np.random.default_rng(99)
    first = _batch_list(rng) * reps
    assert (len(first) > L.SPLIT_W_BATCH_MAX) == (reps > 1)
    tensors = [torch.from_numpy(w).to(DEV) for w, _, _, _ in first]
    dev_mats = [(t, O, I, T) for t, (_, O, I, T) in zip(tensors, first)]
    _assert_batch(H, dev_mats, first, f'batched x{reps}')
    second = _batch_list(rng, second=True) * reps
    for t, (w, _, _, _) in zip(tensors, second):
        t.copy_(torch.from_numpy(w))
    _assert_batch(H, dev_mats, second, f'batched x{reps}, second weights in the same tensors')


# ====================================================================================================================== D. the fused producers
@pytest.mark.parametrize('shape', [(1, 128, 8, 16), (2, 128, 27, 37)], ids=lambda s: 'x'.join(map(str, s)))
def test_upconv_epilogue_split_image_bit_equal(shape):
    """upconv_epilogue_fwd(split_in_scale=s, clamp=4): the image is split_activation_ref(out, s, x_amax = 4, s_amax = max|s|) of the fp32 `out` the same
    launch wrote -- the range is the clamp times the kernel's own max|s|, the element out * s * mul in that order (csrc/epilogue.hip, phase 3)."""
    from inv3d_amd import hipops as H
    n, c, h, w = shape
    g = torch.Generator().manual_seed(61 + h)
    z = H.to_cl((torch.randn(n, c, h + 1, w + 1, generator=g) * 3).to(DEV))
    d = (0.5 + torch.rand(n, c, generator=g)).to(DEV)
    noise, strength = torch.randn(h, w, generator=g).to(DEV), torch.tensor(0.3, device=DEV)
    bias = (0.1 * torch.randn(c, generator=g)).to(DEV)
    s = torch.from_numpy(_styles(np.random.default_rng(h), n, c)).to(DEV)
    out = H.empty_cl(n, c, h, w, DEV)
    simg = H.upconv_epilogue_fwd(z, out, pad0=1, fir_gain=4.0, clamp=4.0, split_in_scale=s, d=d, noise=noise, noise_nstride=0, noise_strength=strength,
                                 bias=bias, act='lrelu', alpha=0.2, gain=math.sqrt(2.0))
    torch.cuda.synchronize()
    o = out.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    assert float(np.abs(o).max()) == 4.0                                    # the clamp is reached: the range is the bound itself
    sn = s.cpu().numpy()
    ref, scale = R.split_activation_ref(o, c, sn, 4.0, float(np.abs(sn).max()))
    _assert_image(simg, ref, scale, ACT_NAMES, f'upconv_epilogue_fwd split image {shape}')


@pytest.mark.parametrize('with_addend', [False, True])
def test_torgb_dgrad_act_split_image_bit_equal(with_addend):
    """torgb_dgrad_act_split at (2, 128, 9, 7): the image is the restatement of the fp32 dz of torgb_dgrad_act at the scale the kernel reports (a bound on
    max|dz|, not max|dz|: the scale is taken from the kernel, the bytes from the restatement)."""
    from inv3d_amd import hipops as H
    n, c, h, w = 2, 128, 9, 7
    g = torch.Generator().manual_seed(78)
    dy4 = (torch.randn(n, 4, h, w, generator=g) * 1e-3).to(DEV).contiguous(memory_format=CL)
    wa = (torch.randn(c, 4, generator=g) / 2).to(DEV).contiguous()
    s = (1 + 0.5 * torch.randn(n, c, generator=g)).to(DEV)
    x = (torch.randn(n, c, h, w, generator=g) * 1.5).to(DEV).contiguous(memory_format=CL)
    add = (torch.randn(n, c, h, w, generator=g) * 2e-3).to(DEV).contiguous(memory_format=CL) if with_addend else None
    d = (0.5 + torch.rand(n, c, generator=g)).to(DEV)
    bias = (torch.randn(c, generator=g) * 0.1).to(DEV)
    noise = torch.randn(n, 1, h, w, generator=g).to(DEV)
    st = torch.tensor(0.37, device=DEV)

    def spec():
        return H.ActBwdSpec(d=d, bias=bias, noise=noise, noise_nstride=h * w, noise_strength=st, act='lrelu', alpha=0.2, gain=math.sqrt(2), clamp=256.0,
                            dnoise_nstride=h * w, dbias=torch.zeros(c, device=DEV), dd=torch.zeros(n, c, device=DEV), dnoise=torch.zeros_like(noise),
                            dstrength=torch.zeros((), device=DEV))
    dz = H.torgb_dgrad_act(dy4, wa, x, s, H.empty_cl(n, c, h, w, DEV), spec(), ds=torch.zeros(n, c, device=DEV), addend=add)
    simg = H.torgb_dgrad_act_split(dy4, wa, x, s, spec(), H.absmax(dy4), ds=torch.zeros(n, c, device=DEV), addend=add,
                                   addend_amax=H.absmax(add) if add is not None else None)
    torch.cuda.synchronize()
    scale = float(simg.scale)
    dzn = dz.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    top = float(np.abs(dzn).max()) * scale
    assert scale > 0 and math.frexp(scale)[0] == 0.5 and 2.0 ** 5 <= top < 2.0 ** 14, (scale, top)
    hi, lo = R.split(dzn.reshape(n, h * w, c), np.float32(scale), R.ACT_LO_MUL)
    ref = np.stack([hi, lo], axis=1).reshape(n, 2, h * w, c // 8, 8).transpose(0, 1, 3, 2, 4)
    _assert_image(simg, np.ascontiguousarray(ref).view(np.uint16), scale, ACT_NAMES, f'torgb_dgrad_act_split image, addend {with_addend}')


# ====================================================================================================================== E. exact-integer class
def _ints(g, shape, lo=-4, hi=4):
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    t.view(-1)[0] = float(hi)                                               # max|.| = 4: the range scalar is the same for every seed
    return t


def _int_styles(g, n, c):
    vals = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
    s = vals[torch.randint(0, 6, (n, c), generator=g)]
    s[n - 1, c - 1] = -2.0
    return s


@functools.lru_cache(maxsize=None)
def _exact_case(n, ci, h, w, co):
    """(x, styles, weights, float64 3x3 correlation of x * styles cast to fp32, on the device, channels_last) -- computed once per shape."""
    g = torch.Generator().manual_seed(n * 7 + ci + 3 * h + w + co)
    x, s, wt = _ints(g, (n, ci, h, w)), _int_styles(g, n, ci), _ints(g, (co, ci, 3, 3))
    ref = F.conv2d(x.double() * s.double()[:, :, None, None], wt.double(), padding=1)
    assert float(ref.abs().max()) < 2.0 ** 22 and torch.equal(ref * 2, (ref * 2).round())
    return x, s, wt, ref.float().to(DEV).contiguous(memory_format=CL)


def _exact_operands(case):
    from inv3d_amd import hipops as H
    x, s, wt, _ = case
    co, ci = wt.shape[:2]
    xc = x.to(DEV).contiguous(memory_format=CL)
    sd = s.to(DEV).contiguous()
    aimg = H.split_activation(xc, H.absmax(xc), in_scale=sd, s_amax=H.absmax(sd))
    wimg = H.split_weight(H.pack_weight_fwd(wt.to(DEV)), co, ci, 9)
    assert not aimg.data.view(torch.int16).view(x.shape[0], 2, -1)[:, 1].any(), 'exact class: a low piece of the activation image is not zero'
    assert not wimg.data.view(torch.int16).view(9, ci // 16, 2, -1)[:, :, 1].any(), 'exact class: a low piece of the weight image is not zero'
    return xc, sd, aimg, wimg


def _assert_exact(got, want, what):
    torch.cuda.synchronize()
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        i = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {bad.shape[0]} of {got.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first at {i}: '
                             f'got {float(got[i])!r}, expected {float(want[i])!r}')


@pytest.mark.parametrize('products', [3, 1])
@pytest.mark.parametrize('rows', [8, 4, 2])
@pytest.mark.parametrize('shape', [(2, 64, 9, 33, 128), (1, 48, 9, 33, 128)], ids=lambda s: 'x'.join(map(str, s)))
def test_exact_conv_v2(shape, rows, products, monkeypatch):
    """conv_v2, nine taps, plain store, patch rows 8 / 4 / 2 (the four-wave forms: V2_KHALVES off), ragged 9 x 33 grid; Ck / 16 = 4 and 3 (an odd chunk count)."""
    from inv3d_amd import hipops as H, _lib as L
    case = _exact_case(*shape)
    n, ci, h, w, co = shape
    _, _, aimg, wimg = _exact_operands(case)
    monkeypatch.setattr(H, 'V2_KHALVES', False)
    out = H.empty_cl(n, co, h, w, DEV)
    H.conv_v2(aimg, wimg, out, H.classes_corr(h, w, 3, 3, 1), epi=L.EPI_STORE, products=products, patch_rows=rows)
    _assert_exact(out, case[3], f'conv_v2 {shape} rows {rows} products {products}')


@pytest.mark.parametrize('products', [3, 1])
def test_exact_conv_v2_split_k(products):
    """Split-K with ks = 3 over 3 chunks at (1, 48, 8, 32, 128): fp32 atomics into a zeroed buffer, any order."""
    from inv3d_amd import hipops as H, _lib as L
    shape = (1, 48, 8, 32, 128)
    case = _exact_case(*shape)
    n, ci, h, w, co = shape
    _, _, aimg, wimg = _exact_operands(case)
    z = torch.zeros((n, co, h, w), device=DEV).contiguous(memory_format=CL)
    H.conv_v2(aimg, wimg, z, H.classes_corr(h, w, 3, 3, 1), epi=L.EPI_ATOMIC, ksplit=3, products=products)
    _assert_exact(z, case[3], f'conv_v2 split-K x3 products {products}')


@pytest.mark.parametrize('products', [3, 1])
@pytest.mark.parametrize('shape', [(2, 64, 9, 33, 128), (1, 96, 20, 64, 128)], ids=lambda s: 'x'.join(map(str, s)))
def test_exact_conv_v2_k_halves(shape, products, monkeypatch):
    """The KH = 2 form (eight waves, the contraction split over the two halves of the workgroup), selected as
    test_conv_v2_k_halves_equal_the_four_wave_form selects it: V2_KHALVES on, patch_rows = 4; chunk counts 4 and 6."""
    from inv3d_amd import hipops as H, _lib as L
    case = _exact_case(*shape)
    n, ci, h, w, co = shape
    _, _, aimg, wimg = _exact_operands(case)
    cls = H.classes_corr(h, w, 3, 3, 1)
    monkeypatch.setattr(H, 'V2_KHALVES', True)
    assert (ci // 16) % 2 == 0 and ci >= 64 and H.tiles(cls, n, 4, co, 128) <= H.V2_KHALVES_MAX_TILES          # what conv_v2 asks of a KH = 2 launch
    out = H.empty_cl(n, co, h, w, DEV)
    H.conv_v2(aimg, wimg, out, cls, epi=L.EPI_STORE, products=products, patch_rows=4)
    _assert_exact(out, case[3], f'conv_v2 KH = 2 {shape} products {products}')


@pytest.mark.parametrize('products', [3, 1])
@pytest.mark.parametrize('plan', [(4, 4), (2, 4), (2, 8)], ids=lambda p: f'rows{p[0]}_waves{p[1]}')      # V3_PLANS of tests/test_gpu_ops.py
def test_exact_conv_v3(plan, products):
    """conv_v3 at (1, 80, 9, 33, 64): five chunks over four / eight waves (some waves own one chunk, some none), every plan."""
    from inv3d_amd import hipops as H, _lib as L
    shape = (1, 80, 9, 33, 64)
    case = _exact_case(*shape)
    n, ci, h, w, co = shape
    _, _, aimg, wimg = _exact_operands(case)
    out = H.empty_cl(n, co, h, w, DEV)
    H.conv_v3(aimg, wimg, out, H.classes_corr(h, w, 3, 3, 1), plan=plan, epi=L.EPI_STORE, products=products)
    _assert_exact(out, case[3], f'conv_v3 plan {plan} products {products}')


@pytest.mark.parametrize('products', [3, 1])
@pytest.mark.parametrize('adjoint', [False, True])
@pytest.mark.parametrize('shape', [(1, 96, 5, 7, 64), (3, 32, 2, 32, 192)], ids=lambda s: 'x'.join(map(str, s)))
def test_exact_conv_ws(shape, adjoint, products):
    """conv_ws (fp32 activation in, split in the loader, split-K atomics into a buffer that holds integers): forward taps with styles, and the data gradient
    (adjoint weight image, flipped taps) against conv_transpose2d in float64."""
    from inv3d_amd import hipops as H
    n, ci, h, w, co = shape
    g = torch.Generator().manual_seed(ci + co + h)
    wt = _ints(g, (co, ci, 3, 3))
    if adjoint:
        x, s = _ints(g, (n, co, h, w)), None
        ref = F.conv_transpose2d(x.double(), wt.double(), padding=1)
        wimg = H.split_weight(H.pack_weight_adj(wt.to(DEV)), ci, co, 9)
        cls, cout = H.classes_corr_adjoint(h, w, 3, 3, 1), ci
    else:
        x, s = _ints(g, (n, ci, h, w)), _int_styles(g, n, ci)
        ref = F.conv2d(x.double() * s.double()[:, :, None, None], wt.double(), padding=1)
        wimg = H.split_weight(H.pack_weight_fwd(wt.to(DEV)), co, ci, 9)
        cls, cout = H.classes_corr(h, w, 3, 3, 1), co
    assert H.conv_ws_ok(x.shape[1], cout, cls, n, h, w)
    xc = x.to(DEV).contiguous(memory_format=CL)
    base = _ints(g, (n, cout, h, w), -64, 64).to(DEV).contiguous(memory_format=CL)
    out = base.clone(memory_format=CL)
    H.conv_ws(xc, wimg, out, cls, in_scale=s.to(DEV).contiguous() if s is not None else None, x_amax=H.absmax(xc), products=products)
    want = (base.double().cpu() + ref).float().to(DEV).contiguous(memory_format=CL)
    _assert_exact(out, want, f'conv_ws {shape} adjoint {adjoint} products {products}')


@pytest.mark.parametrize('products', [3, 1])
def test_exact_conv_wgrad_v2(products):
    """conv_wgrad_v2 at (1, 64, 128, 9, 33, 3) (a shape tuple of test_conv_wgrad_v2_vs_torch: ragged strip, three row groups): the float64 weight gradient of
    the style-modulated 3x3 correlation, accumulated with atomics and through the slab form."""
    from inv3d_amd import hipops as H
    n, ci, co, h, w, rg = 1, 64, 128, 9, 33, 3
    g = torch.Generator().manual_seed(17)
    x, s, dy = _ints(g, (n, ci, h, w)), _int_styles(g, n, ci), _ints(g, (n, co, h, w))
    wt = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double() * s.double()[:, :, None, None], wt, padding=1).backward(dy.double())
    ref = wt.grad
    assert float(ref.abs().max()) < 2.0 ** 22
    ref = ref.float().to(DEV)
    xq, gq = x.to(DEV).contiguous(memory_format=CL), dy.to(DEV).contiguous(memory_format=CL)
    ximg = H.split_activation(xq, H.absmax(xq), in_scale=s.to(DEV).contiguous())
    gimg = H.split_activation(gq, H.absmax(gq))
    cls = H.classes_corr(h, w, 3, 3, 1)
    assert H.conv_wgrad_v2_ok(gimg, ximg, cls)
    dwp = torch.zeros(co, 9 * ci, device=DEV)
    H.conv_wgrad_v2(gimg, ximg, dwp, cls, products=products, row_groups=rg)
    _assert_exact(dwp.view(co, 3, 3, ci).permute(0, 3, 1, 2).contiguous(), ref, f'conv_wgrad_v2 products {products}')
    slabs = H.conv_wgrad_v2_slabs(gimg, ximg, cls, products=products, row_groups=rg)
    got = H.weight_grad_finish(slabs, torch.zeros(co, ci, 3, 3, device=DEV), None, None, None)
    _assert_exact(got.contiguous(), ref, f'conv_wgrad_v2 slabs products {products}')
