"""The two separable [1,3,3,1] FIR tile passes of the up layers on their own, at the smallest shapes where their band-walking schedule can go
wrong: eg3d_upconv_epilogue_fwd (rolling row window down a column strip, fused operand split) and eg3d_fir44_adjoint_split (the parity images of
the FIR adjoint).  The workload's sizes are covered by the generator / loop suites; here every shape takes another path through the schedule.

How many bands a block walks is the launcher's choice: it cuts a strip (16 columns x 64 channels of an image) into as many row segments as fill
the GPU in one round, so a small tensor gets one band per block whatever its height.  The carried rows, the prefetch under the stores and the
barrier between bands only run when there are several hundred strips; the last shape of each list is the smallest such tensor (512 / 272 strips:
segments of at least three full bands and a ragged one).  All comparisons are made on the device."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def rel_close(a, b, tol, what=''):
    """max |a - b| <= tol x max |b|."""
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape and bool(torch.isfinite(a).all()), what
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= tol * scale, f'{what}: err {err:.3e} > {tol} * {scale:.3e}'


def decode_split(img, scale, n, c, planes, h, w):
    """Two-piece fp16 image [N][2][C/8][planes][h][w][8] -> float64 [N, C, planes, h, w] = (hi + lo / 2048) / scale."""
    v = img.data.view(n, 2, c // 8, planes, h, w, 8).double()
    x = (v[:, 0] + v[:, 1] / 2048.0) / float(scale)
    return x.permute(0, 1, 5, 2, 3, 4).reshape(n, c, planes, h, w)


# output shapes (N, C, H, W): one band / one strip; >= 3 bands + a ragged last one (the carried rows); ragged columns, two channel blocks, image index;
# shorter than one band of the 8-row form with many strips; the small-grid choice of the launcher; 512 strips: the plain form walks segments of 16 and 13
# rows (4 bands; 3 bands + 1 ragged row), the pad0 = 2 form 16 and 14, the split form one segment of 29 (7 bands + 1 row), with a ragged last column tile
UPCONV_SHAPES = [(1, 64, 8, 16), (1, 64, 29, 16), (2, 128, 27, 37), (1, 192, 5, 70), (2, 64, 64, 64), (4, 512, 29, 250)]


def _upconv_inputs(shape, seed=61):
    n, c, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    return g, dict(d=0.5 + torch.rand(n, c, generator=g, device=DEV), bias=0.1 * torch.randn(c, generator=g, device=DEV),
                   noise_strength=torch.tensor(0.3, device=DEV), act='lrelu', alpha=0.2, gain=math.sqrt(2.0))


@pytest.mark.parametrize('shape', UPCONV_SHAPES)
def test_upconv_epilogue_strip_vs_25_load_kernel(shape):
    """pad0 = 1 with demodulation, bias, lrelu, gain sqrt 2, clamp in {-1, 4} and noise shared by the batch or per image; and the bare pad0 = 2,
    gain 4 form the FIR adjoint uses (z H x W -> out (H + 1) x (W + 1)) -- against the 25-load kernel, 2e-6 of max|ref|, max|out| likewise."""
    from inv3d_amd import hipops as H
    from inv3d_amd.fused import fir44
    n, c, h, w = shape
    g, kw = _upconv_inputs(shape)
    z = H.to_cl(torch.randn(n, c, h + 1, w + 1, generator=g, device=DEV) * 3)
    for nstride, noise in ((0, torch.randn(h, w, generator=g, device=DEV)), (h * w, torch.randn(n, h, w, generator=g, device=DEV))):
        for clamp in (-1.0, 4.0):
            ref, out = H.empty_cl(n, c, h, w, DEV), H.empty_cl(n, c, h, w, DEV)
            a0, a1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
            H.epilogue_fwd(z, ref, fir=fir44(DEV), pad0=1, fir_gain=4.0, clamp=clamp, out_amax=a0, noise=noise, noise_nstride=nstride, **kw)
            assert H.upconv_epilogue_fwd(z, out, pad0=1, fir_gain=4.0, clamp=clamp, out_amax=a1, noise=noise, noise_nstride=nstride, **kw) is None
            rel_close(out, ref, 2e-6, f'upconv epilogue {shape} clamp {clamp} noise stride {nstride}')
            assert abs(float(a0) - float(a1)) <= 2e-6 * float(a0)
    zz = H.to_cl(torch.randn(n, c, h, w, generator=g, device=DEV))
    ref, out = H.empty_cl(n, c, h + 1, w + 1, DEV), H.empty_cl(n, c, h + 1, w + 1, DEV)
    H.epilogue_fwd(zz, ref, fir=fir44(DEV), pad0=2, fir_gain=4.0)
    H.upconv_epilogue_fwd(zz, out, pad0=2, fir_gain=4.0)
    rel_close(out, ref, 2e-6, f'bare FIR adjoint form {shape}')


@pytest.mark.parametrize('shape', [s for s in UPCONV_SHAPES if s[1] % 128 == 0] + [(1, 128, 29, 40)])
def test_upconv_epilogue_strip_fused_split(shape):
    """The operand image written beside `out` (split_in_scale = s, clamp 4) decodes to out * s within 2^-21 of its range bound clamp * max|s|, and
    drives the pre-split convolution to the result of the stand-alone split pass."""
    from inv3d_amd import hipops as H, _lib as L
    n, c, h, w = shape
    g, kw = _upconv_inputs(shape, seed=62)
    z = H.to_cl(torch.randn(n, c, h + 1, w + 1, generator=g, device=DEV) * 3)
    noise = torch.randn(h, w, generator=g, device=DEV)
    s = 1 + 0.5 * torch.randn(n, c, generator=g, device=DEV)
    out = H.empty_cl(n, c, h, w, DEV)
    simg = H.upconv_epilogue_fwd(z, out, pad0=1, fir_gain=4.0, clamp=4.0, split_in_scale=s, noise=noise, noise_nstride=0, **kw)
    bound = 4.0 * float(s.abs().max())
    assert float(simg.scale) == 2.0 ** (14 - math.frexp(bound)[1])
    dec = decode_split(simg, simg.scale, n, c, 1, h, w)[:, :, 0]
    want = out.double() * s.double()[:, :, None, None]
    err = float((dec - want).abs().max())
    assert err <= 2.0 ** -21 * bound, (shape, err, bound)
    wt = torch.randn(128, c, 3, 3, generator=g, device=DEV) / math.sqrt(c * 9)
    wimg = H.split_weight(H.pack_weight_fwd(wt), 128, c, 9)
    y1, y2 = H.empty_cl(n, 128, h, w, DEV), H.empty_cl(n, 128, h, w, DEV)
    H.conv_v2(simg, wimg, y1, H.classes_corr(h, w, 3, 3, 1), epi=L.EPI_STORE)
    H.conv_v2(H.split_activation(out, H.absmax(out), in_scale=s), wimg, y2, H.classes_corr(h, w, 3, 3, 1), epi=L.EPI_STORE)
    a, b = y1.double(), y2.double()
    assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), shape


# (N, C, Hi, Wi): dz is 2 Hi x 2 Wi.  One cell row pair; >= 3 bands, ragged, across one cell-column tile; batch + two channel blocks + three tiles; square;
# 272 strips: one segment of 11 cell rows per strip (5 bands + 1 ragged cell row), 17 column tiles of which the last holds 5 cells
ADJ_SHAPES = [(1, 64, 2, 32), (1, 64, 9, 33), (2, 128, 7, 70), (1, 192, 32, 32), (2, 512, 10, 260)]


def _adjoint_inputs(shape, kind):
    n, c, hi, wi = shape
    g = torch.Generator(device=DEV).manual_seed(63)
    if kind == 'random':
        return torch.randn(n, c, 2 * hi, 2 * wi, generator=g, device=DEV)
    dz = 0.01 * torch.randn(n, c, 2 * hi, 2 * wi, generator=g, device=DEV)          # one large element at each corner: halo and bounds
    for k, (y, x) in enumerate(((0, 0), (0, -1), (-1, 0), (-1, -1))):
        dz[n - 1, (k * 17) % c, y, x] = 100.0 * (-1) ** k
    return dz


@pytest.mark.parametrize('kind', ['random', 'corners'])
@pytest.mark.parametrize('shape', ADJ_SHAPES)
def test_fir44_adjoint_split_alone(shape, kind):
    """The four parity images decode to g = upfirdn2d(dz, outer(f, f), pad 2, flipped, gain 4) re-sampled by parity, within 2e-6 max|g| (fp32
    arithmetic) + 2^-21 max|g| (two-piece representation); cells an odd parity does not have are exactly zero; the scale is the power of two the
    range formula gives for gain * max|dz|."""
    from inv3d_amd import hipops as H
    from inv3d_amd.fused import fir44
    n, c, hi, wi = shape
    dzc = H.to_cl(_adjoint_inputs(shape, kind))
    amax = H.absmax(dzc)
    gimg = H.fir44_adjoint_split(dzc, amax, gain=4.0)
    gref = H.upfirdn2d_nhwc(dzc, fir44(DEV), pad=(2, 2, 2, 2), flip=True, gain=4.0).double()
    assert gref.shape == (n, c, 2 * hi + 1, 2 * wi + 1)
    bound = float(torch.tensor(float(amax), dtype=torch.float32) * 4.0)
    assert float(gimg.scale) == 2.0 ** (14 - math.frexp(bound)[1])
    dec = decode_split(gimg, gimg.scale, n, c, 4, hi + 1, wi + 1)
    raw = gimg.data.view(n, 2, c // 8, 4, hi + 1, wi + 1, 8)
    tol = (2e-6 + 2.0 ** -21) * float(gref.abs().max())
    for py in range(2):
        for px in range(2):
            want = gref[:, :, py::2, px::2]
            got = dec[:, :, py * 2 + px]
            err = float((got[:, :, :want.shape[2], :want.shape[3]] - want).abs().max())
            assert err <= tol, (shape, kind, py, px, err, tol)
            if py:
                assert not bool(raw[:, :, :, py * 2 + px, hi].any())
            if px:
                assert not bool(raw[:, :, :, py * 2 + px, :, wi].any())


def test_fir_pass_launchers_refuse_as_before():
    """C not a multiple of 64 and misaligned pointers: EG3D_ERR_UNSUPPORTED (-2); an empty batch: EG3D_ERR_INVALID (-1); an image beyond the 32-bit
    offsets of the strip kernels' stores (2 GiB): EG3D_ERR_UNSUPPORTED.  Nothing is launched."""
    from inv3d_amd import hipops as H, _lib as L
    lib, k4 = L.lib(), (C.c_float * 4)(0.125, 0.375, 0.375, 0.125)
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()

    def up(z, out, n, c, h=8):
        return lib.eg3d_upconv_epilogue_fwd(C.c_void_p(z), C.c_void_p(out), n, h, h, c, h + 1, h + 1, k4, 1, 4.0, None, None, 0, None, None, L.ACT_IDS['linear'], 0.0, 1.0, -1.0,
                                            None, None, None, None, L.stream_ptr())

    def adj(dz, img, n, c, hi=4):
        return lib.eg3d_fir44_adjoint_split(C.c_void_p(dz), C.c_void_p(p), C.c_void_p(img), C.c_void_p(p + 16), n, hi, hi, c, c, 4.0, L.stream_ptr())

    q = p + (1 << 17)
    assert up(p + 64, q, 1, 32) == -2 and up(p + 68, q, 1, 64) == -2 and up(p + 64, q + 4, 1, 64) == -2 and up(p + 64, q, 0, 64) == -1
    assert adj(p + 64, q, 1, 32) == -2 and adj(p + 68, q, 1, 64) == -2 and adj(p + 64, q + 4, 1, 64) == -2 and adj(p + 64, q, 0, 64) == -1
    assert up(p + 64, q, 1, 64, h=4096) == -2 and adj(p + 64, q, 1, 64, hi=4096) == -2
    torch.cuda.synchronize()
