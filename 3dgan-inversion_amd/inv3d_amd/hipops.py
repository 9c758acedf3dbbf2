"""Thin, allocation-aware wrappers over the C-ABI kernels (one Python function per entry point).

Tensors handed to the fused path are fp32 "NHWC": logical shape [N,C,H,W] with channels_last strides (so the
reference-facing API keeps NCHW shapes while memory is channel-contiguous, which is what the MFMA implicit GEMM,
the float4 epilogues and the 128-byte tri-plane gathers want).
"""
import contextlib
import gc
import math
import os
import weakref
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

CL = torch.channels_last


class LaunchProfiler:
    """Optional per-launch timing (bench.py roofline): HIP events recorded on the launch stream around every implicit-GEMM conv launch,
    with the launch's algorithmic FLOPs and kernel id (tile configuration 0..4 of eg3d_conv2d_igemm_f32, V2_CONFIG for the pre-split
    kernel), and around named spans (the renderer's forward / backward)."""

    def __init__(self, only_config=None, keep_meta=False):
        self.records = []          # ((config_id, precision_id), algo_flops, start_event, end_event): one key per kernel family
        self.spans = []            # (name, start_event, end_event)
        self.only_config = only_config      # time only launches of this kernel id (keeps the event overhead small)
        self.meta = [] if keep_meta else None      # per record: launch geometry (tools/conv_launch_table.py)

    def summary(self):
        out = {}
        for cfg, fl, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            d = out.setdefault(cfg, dict(launches=0, flops=0.0, ms=0.0))
            d['launches'] += 1
            d['flops'] += fl
            d['ms'] += ms
        return out

    def span_summary(self):
        out = {}
        for name, e0, e1 in self.spans:
            d = out.setdefault(name, dict(count=0, ms=0.0))
            d['count'] += 1
            d['ms'] += e0.elapsed_time(e1)
        return out


class _Span:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prof = PROFILER
        if self.prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.prof is not None:
            self.e1.record()
            self.prof.spans.append((self.name, self.e0, self.e1))


def span_between_grads(name, t_start, t_end):
    """Profiler span over a stretch of the BACKWARD pass: opened when the gradient of `t_start` arrives, closed when that of `t_end` does
    (bench.py: the backbone's backward = from d planes to d ws).  No-op without an active profiler."""
    prof = PROFILER
    if prof is None or not (torch.is_tensor(t_start) and torch.is_tensor(t_end) and t_start.requires_grad and t_end.requires_grad):
        return
    st = {}

    def opened(g):
        st['e0'] = torch.cuda.Event(enable_timing=True)
        st['e0'].record()

    def closed(g):
        if 'e0' in st:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            prof.spans.append((name, st.pop('e0'), e1))
    t_start.register_hook(opened)
    t_end.register_hook(closed)


TILE_NAMES = {0: '128,128,2,2', 1: '64,128,2,2', 2: '32,128,1,4', 3: '128,32,4,1', 4: '256,64,4,1'}


PROFILER = None


def is_cl(t: torch.Tensor) -> bool:
    return t.dim() == 4 and t.is_cuda and t.dtype == torch.float32 and (t.stride(1) == 1 or t.shape[1] == 1) and \
        t.is_contiguous(memory_format=CL)


@contextlib.contextmanager
def capture_guard():
    """Wrap a HIP-graph capture: the cyclic garbage collector must not run inside it.  Collecting the remains of an EARLIER capture (a
    CUDAGraph, tensors of its pool) frees device memory, which the runtime refuses while a stream is capturing -- the process aborts
    ("Fatal Python error: Aborted ... Garbage-collecting", seen once in four runs of the GPU suite).  Collect before, hold during."""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def to_cl(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous(memory_format=CL)


def empty_cl(n, c, h, w, device) -> torch.Tensor:
    return torch.empty((n, c, h, w), dtype=torch.float32, device=device, memory_format=CL)


class ZeroArena:
    """One zero-fill launch per optimisation step instead of ~60.

    Split-K partial-sum buffers and the small atomically accumulated outputs (style / noise / bias gradients ...) all have to start
    at zero, and inside a replayed graph every fill is a ~5 us kernel.  The arena hands out slices of ONE buffer that is cleared once
    at the start of the step; the demand of the previous step sizes it (shapes are static from step to step; anything that does not
    fit falls back to torch.zeros and enlarges the arena for the next step).  Slices are only valid until the next begin(): use it
    for temporaries and for gradients that are consumed within the step (inversion.LatentProjector does)."""

    def __init__(self, device):
        self.device, self.buf, self.off, self.limit, self.demand, self.prev_demand = device, None, 0, 0, 0, 0

    def begin(self):
        need = self.prev_demand
        if need and (self.buf is None or self.buf.numel() < need):
            self.buf = torch.empty(need, dtype=torch.float32, device=self.device)
        self.limit = need if self.buf is not None else 0
        if self.limit:
            self.buf[:self.limit].fill_(0.0)         # a fill kernel, not a memset node: memset / memcpy nodes split a captured graph into
                                                     # separately submitted segments (~50 us of idle GPU each on ROCm 7)
        self.off = self.demand = 0

    def take(self, numel: int):
        n = -(-numel // 64) * 64                        # 256-byte granules
        self.demand += n
        if self.off + n > self.limit:
            return None
        v = self.buf[self.off:self.off + numel]
        self.off += n
        return v

    def end(self):
        self.prev_demand = max(self.prev_demand, self.demand)


ARENA: Optional[ZeroArena] = None


class zero_arena:
    """Context manager: route hipops.zeros / zeros_cl through `arena` for the duration of one step."""

    def __init__(self, arena: Optional[ZeroArena]):
        self.arena = arena

    def __enter__(self):
        global ARENA
        self.prev, ARENA = ARENA, self.arena
        if self.arena is not None:
            self.arena.begin()
        return self.arena

    def __exit__(self, *exc):
        global ARENA
        if self.arena is not None:
            self.arena.end()
        ARENA = self.prev
        return False


def zeros(shape, device) -> torch.Tensor:
    """fp32 zeros; from the step's ZeroArena when one is active."""
    shape = tuple(shape)
    numel = 1
    for d in shape:
        numel *= int(d)
    a = ARENA.take(numel) if (ARENA is not None and torch.device(device) == ARENA.device and numel > 0) else None
    return a.view(shape) if a is not None else torch.zeros(shape, dtype=torch.float32, device=device)


def zeros_cl(n, c, h, w, device) -> torch.Tensor:
    a = ARENA.take(n * c * h * w) if (ARENA is not None and torch.device(device) == ARENA.device) else None
    if a is not None:
        return a.view(n, h, w, c).permute(0, 3, 1, 2)           # NHWC memory, NCHW shape = channels_last
    return torch.empty((n, c, h, w), dtype=torch.float32, device=device, memory_format=CL).zero_()


def _dtype_code(t):
    try:
        return {torch.float32: L.F32, torch.float16: L.F16, torch.float64: L.F64}[t.dtype]
    except KeyError:
        raise L.Eg3dHipError(f'unsupported dtype {t.dtype}')


# ------------------------------------------------------------------------------------------------- bias_act
def bias_act_raw(x, b, xref, yref, dy, grad, dim, act_id, alpha, gain, clamp):
    """y = eg3d_bias_act(...); x dense (any layout); output has x's layout."""
    L.require_cuda(x, b, xref, yref, dy)
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    size_b = b.numel() if b is not None else 0
    step_b = x.stride(dim) if b is not None else 1
    L.check(L.lib().eg3d_bias_act(L.ptr(x), L.ptr(b), L.ptr(xref), L.ptr(yref), L.ptr(dy), L.ptr(y), _dtype_code(x), x.numel(),
                                  size_b, step_b, grad, act_id, float(alpha), float(gain), float(clamp), L.stream_ptr()), 'bias_act')
    return y


# ------------------------------------------------------------------------------------------------- upfirdn2d
def upfirdn2d_raw(x, f2d, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain):
    L.require_cuda(x, f2d)
    n, c, h, w = x.shape
    fh, fw = f2d.shape
    ow = (w * upx + padx0 + padx1 - fw + downx) // downx
    oh = (h * upy + pady0 + pady1 - fh + downy) // downy
    if ow < 1 or oh < 1:
        raise L.Eg3dHipError('upfirdn2d: output must be at least 1x1')
    mf = CL if (x.stride(1) == 1 and c > 1) else torch.contiguous_format
    y = torch.empty((n, c, oh, ow), dtype=x.dtype, device=x.device, memory_format=mf)
    xs = (C.c_int64 * 4)(*x.stride())
    ys = (C.c_int64 * 4)(*y.stride())
    f2d = f2d.contiguous().float()
    L.check(L.lib().eg3d_upfirdn2d(L.ptr(x), L.ptr(f2d), L.ptr(y), _dtype_code(x), n, c, h, w, xs, fh, fw, upx, upy, downx, downy,
                                   padx0, padx1, pady0, pady1, int(bool(flip)), float(gain), oh, ow, ys, L.stream_ptr()), 'upfirdn2d')
    return y


def upfirdn2d_nhwc(x, f2d, up=1, down=1, pad=(0, 0, 0, 0), flip=False, gain=1.0, out=None, accumulate=False, addend=None):
    """addend (fp32 channels_last, the output's shape): returns result + addend in the same pass (eg3d_upfirdn2d_nhwc_add)."""
    assert is_cl(x), 'upfirdn2d_nhwc expects an fp32 channels_last CUDA tensor'
    n, c, h, w = x.shape
    fh, fw = f2d.shape
    px0, px1, py0, py1 = pad
    ow = (w * up + px0 + px1 - fw + down) // down
    oh = (h * up + py0 + py1 - fh + down) // down
    if out is None:
        out = empty_cl(n, c, oh, ow, x.device)
        accumulate = False
    if addend is not None:
        assert not accumulate and is_cl(addend) and tuple(addend.shape) == (n, c, oh, ow) and addend.dtype == torch.float32
        L.check(L.lib().eg3d_upfirdn2d_nhwc_add(L.ptr(x), L.ptr(f2d), L.ptr(addend), L.ptr(out), n, c, h, w, fh, fw, up, down, px0, px1, py0, py1,
                                                int(bool(flip)), float(gain), oh, ow, L.stream_ptr()), 'upfirdn2d_nhwc_add')
        return out
    L.check(L.lib().eg3d_upfirdn2d_nhwc(L.ptr(x), L.ptr(f2d), L.ptr(out), n, c, h, w, fh, fw, up, down, px0, px1, py0, py1,
                                        int(bool(flip)), float(gain), oh, ow, int(bool(accumulate)), L.stream_ptr()), 'upfirdn2d_nhwc')
    return out


# ------------------------------------------------------------------------------------------------- conv tap lists
def _mk_class(Ha, Wa, py, px, taps):
    c = L.ConvClass()
    c.Ha, c.Wa, c.out_py, c.out_px, c.ntaps = Ha, Wa, py, px, len(taps)
    assert 1 <= len(taps) <= 9
    for i, (dy, dx, wt) in enumerate(taps):
        c.dy[i], c.dx[i], c.wtap[i] = dy, dx, wt
    return c


def classes_corr(Ho, Wo, kh, kw, pad, flip_taps=False, dil=1):
    """stride-1 correlation: out[y,x] = sum_k w[ky,kx] * in[y+dil*ky-pad, x+dil*kx-pad]  (flip_taps: true convolution; dil: dilation)."""
    taps = []
    for ky in range(kh):
        for kx in range(kw):
            wt = ((kh - 1 - ky) * kw + (kw - 1 - kx)) if flip_taps else (ky * kw + kx)
            taps.append((dil * ky - pad, dil * kx - pad, wt))
    return [_mk_class(Ho, Wo, 0, 0, taps)]


def classes_corr_adjoint(Hi, Wi, kh, kw, pad, flip_taps=False, dil=1):
    """data-gradient of classes_corr: dx[y,x] = sum_k w[ky,kx] * g[y-dil*ky+pad, x-dil*kx+pad]."""
    taps = []
    for ky in range(kh):
        for kx in range(kw):
            wt = ((kh - 1 - ky) * kw + (kw - 1 - kx)) if flip_taps else (ky * kw + kx)
            taps.append((pad - dil * ky, pad - dil * kx, wt))
    return [_mk_class(Hi, Wi, 0, 0, taps)]


def classes_convT(Hi, Wi, kh, kw, up, flip_taps=False):
    """stride-`up` transposed conv, no padding: out[up*a+ky, up*b+kx] += in[a,b]*w[ky,kx]; out = (Hi-1)*up + kh.
    One class per output phase (py,px); taps ky == py (mod up) read in[a - (ky-py)/up]."""
    Ho, Wo = (Hi - 1) * up + kh, (Wi - 1) * up + kw
    cls = []
    for py in range(up):
        for px in range(up):
            taps = []
            for ky in range(py, kh, up):
                for kx in range(px, kw, up):
                    wt = ((kh - 1 - ky) * kw + (kw - 1 - kx)) if flip_taps else (ky * kw + kx)
                    taps.append((-(ky - py) // up, -(kx - px) // up, wt))
            Ha = (Ho - py + up - 1) // up
            Wa = (Wo - px + up - 1) // up
            if taps and Ha > 0 and Wa > 0:
                cls.append(_mk_class(Ha, Wa, py, px, taps))
    return cls, Ho, Wo


def classes_convT_adjoint(Hi, Wi, kh, kw, up, flip_taps=False):
    """data-gradient of classes_convT: dx[a,b] = sum_k g[up*a+ky, up*b+kx] * w[ky,kx]  (in_stride = up)."""
    taps = []
    for ky in range(kh):
        for kx in range(kw):
            wt = ((kh - 1 - ky) * kw + (kw - 1 - kx)) if flip_taps else (ky * kw + kx)
            taps.append((ky, kx, wt))
    return [_mk_class(Hi, Wi, 0, 0, taps)]


_MEMO = {}
WEIGHTS_EPOCH = 0


def weights_changed():
    """Invalidate every derived weight image (memo(), fused.WeightCache).  The caches key on a tensor's in-place version counter, which
    ordinary in-place updates bump -- but fused multi-tensor optimisers (torch.optim.Adam(fused=True)) write parameters without
    touching it.  Call this after such an update (inversion.PivotalTuner registers it as an optimizer step hook)."""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1



CAPTURE_REFS = None           # a list while graphed.capture runs: every derived tensor handed out (memo / WeightCache) is appended, so that the
                              # captured graph's owner can keep alive what its kernels hold raw pointers to


def keep_for_capture(*objs):
    if CAPTURE_REFS is not None:
        CAPTURE_REFS.extend(o for o in objs if o is not None)


def memo(tag, tensors, fn):
    """Derived images of parameters (packed / padded / pre-scaled weights), recomputed only when a source tensor changes (storage
    pointer or in-place version).  One entry per (tag, storage): frozen weights cost nothing per step, trained ones are rebuilt."""
    # the optimiser epoch only concerns tensors an optimiser can write: frozen sources (the loss / pose / encoder networks during
    # pivotal tuning) keep their images across the tuned generator's steps
    epoch = WEIGHTS_EPOCH if any(t.requires_grad for t in tensors) else -1
    key = (epoch,) + tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)
    slot = (tag, tensors[0].data_ptr())
    hit = _MEMO.get(slot)
    # the entry is only valid for the very same tensor objects (a freed temporary's address can be reused by another tensor)
    if hit is None or hit[0] != key or any(r() is not t for r, t in zip(hit[2], tensors)):
        if len(_MEMO) > 512:
            _MEMO.clear()
        with torch.no_grad():
            hit = (key, fn(), tuple(weakref.ref(t) for t in tensors))
        _MEMO[slot] = hit
    keep_for_capture(hit[1])
    return hit[1]


def pack_weight_fwd(w):
    """[O,I,kh,kw] -> [O, kh*kw*I]  (row o: taps major, input channel minor)."""
    o, i, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(o, kh * kw * i).contiguous()


def pack_weight_adj(w):
    """[O,I,kh,kw] -> [I, kh*kw*O]  (for data gradients: roles of I and O swapped)."""
    o, i, kh, kw = w.shape
    return w.permute(1, 2, 3, 0).reshape(i, kh * kw * o).contiguous()


# Matrix-core arithmetic of the implicit GEMMs (include/eg3d_hip.h EG3D_PREC_*).  Operands, accumulators and results are fp32 in
# every mode; the modes differ in how an fp32 product is formed on the matrix cores:
#   'f16x3'   two fp16 pieces per operand, three products; error vs fp64 as small as the fp32 MFMA path for operands of ordinary
#             magnitude (|x| ~ 2^-4 .. 2^16), 1.45x the rate of bf16x6.  Needs the operand range: used where it is known.
#   'bf16x6'  three bf16 pieces, six products; fp32-equivalent for any operand range.
#   'f32'     v_mfma_f32_32x32x2_f32.       'bf16x3'  three bf16 products (~2^-15), opt-in only.
# Mode 'auto' (default): the style-modulated convolutions run 'f16x3' -- their forward operands are demodulated O(1) activations and
# unit-variance weights, and the data gradient is range-normalised with the max|dz| its producer (epilogue_bwd) reports -- everything
# else (toRGB, the generic conv2d of conv2d_gradfix) runs 'bf16x6'.  Any other value forces that mode everywhere.
# Set with set_conv_precision() or the EG3D_CONV_PRECISION environment variable.
PRECISIONS = {'f32': 0, 'bf16x6': 1, 'bf16x3': 2, 'f16x3': 3, 'f16x1': 4}      # 'f16x1': single product of the high fp16 pieces (include/eg3d_hip.h)
CONV_MODE = os.environ.get('EG3D_CONV_PRECISION', 'auto')
CONV_PRECISION = PRECISIONS['bf16x6' if CONV_MODE == 'auto' else CONV_MODE]


def set_conv_precision(name):
    global CONV_MODE, CONV_PRECISION
    assert name == 'auto' or name in PRECISIONS
    CONV_MODE = name
    CONV_PRECISION = PRECISIONS['bf16x6' if name == 'auto' else name]


MODCONV_OVERRIDE = None      # 'f16x1' inside modconv_override(): every modulated conv on the pre-split kernels runs ONE product of fp16-rounded operands


def modconv_precision() -> str:
    """Arithmetic of the style-modulated convolutions (the dominant kernels) under the current mode."""
    if MODCONV_OVERRIDE is not None and CONV_MODE == 'auto':
        return MODCONV_OVERRIDE
    return 'f16x3' if CONV_MODE == 'auto' else CONV_MODE


@contextlib.contextmanager
def modconv_override(name):
    """Arithmetic class of the reference's own GPU path for the modulated convs of BOTH networks (backbone + super-resolution head): `f16x1` =
    one v_mfma_f32_32x32x16_f16 product of range-normalised fp16-rounded operands, fp32 accumulation, fp32 results -- an 11-bit significand
    per operand, what a TF32 convolution keeps (the reference never disables TF32 on its inversion path: only training/training_loop.py:135-136
    and calc_metrics.py:52-53 do).  Layers still on the loader-split kernel (it has no single-product form) keep three products."""
    global MODCONV_OVERRIDE
    assert name in (None, 'f16x1', 'f16x3')
    prev, MODCONV_OVERRIDE = MODCONV_OVERRIDE, name
    try:
        yield
    finally:
        MODCONV_OVERRIDE = prev


class ActBwdSpec:
    """What EPI_BWD_ACT needs about the layer that produced a data gradient's `xin`: that layer's epilogue constants (saved at its forward)
    and the pre-zeroed reduction targets of its backward (filled by the fused launch)."""
    __slots__ = ('d', 'bias', 'noise', 'noise_nstride', 'noise_strength', 'act', 'alpha', 'gain', 'clamp', 'dbias', 'dd', 'dnoise',
                 'dnoise_nstride', 'dstrength')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def fill(self, ab):
        tp = lambda t: t.data_ptr() if t is not None else None
        ab.d, ab.bias, ab.noise, ab.noise_strength = tp(self.d), tp(self.bias), tp(self.noise), tp(self.noise_strength)
        ab.noise_nstride, ab.dnoise_nstride = int(self.noise_nstride or 0), int(self.dnoise_nstride or 0)
        ab.act, ab.alpha, ab.gain, ab.clamp = L.ACT_IDS[self.act], float(self.alpha), float(self.gain), float(self.clamp)
        ab.dbias, ab.dd, ab.dnoise, ab.dstrength = tp(self.dbias), tp(self.dd), tp(self.dnoise), tp(self.dstrength)


def _try_act_bwd(p, act_bwd, supported, aligned16=True):
    """Turn a prepared EPI_BWD launch into EPI_BWD_ACT when the library takes it (`supported`: its check for this kernel) and, for the kernels
    that load them as 16-byte vectors, the producer's d / bias are so aligned; else leave a plain EPI_BWD.  Returns whether the fused epilogue runs."""
    p.epi = L.EPI_BWD_ACT
    act_bwd.fill(p.act_bwd)
    ok = bool(supported(C.byref(p))) and (not aligned16 or all(t is None or t.data_ptr() % 16 == 0 for t in (act_bwd.d, act_bwd.bias)))
    if not ok:
        p.epi = L.EPI_BWD
        p.act_bwd = L.ActBwd()
    return ok


def _recorded(launch, cfg_id, prec_id, algo_flops, default_flops, meta):
    """Run the launch thunk; under an active LaunchProfiler that times this kernel id, between two events, and leave its record
    ((kernel id, precision id), algorithmic FLOPs -- `default_flops()` when the caller gave none --, events) and, when kept, `meta()`."""
    prof = PROFILER
    if prof is None or (prof.only_config is not None and prof.only_config != cfg_id):
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    prof.records.append(((cfg_id, prec_id), float(default_flops() if algo_flops is None else algo_flops), e0, e1))
    if prof.meta is not None:
        prof.meta.append(meta())


def _patches(N, H, W, rows):
    """rows x 32-cell patches that cover an H x W grid of N images."""
    return N * -(-H // rows) * -(-W // 32)


def tiles(classes, N, rows, Nc, ctile):
    """Workgroups of a launch that covers every tap class of N images with rows x 32-cell patches and ctile-channel tiles."""
    return sum(_patches(N, c.Ha, c.Wa, rows) for c in classes) * (Nc // ctile)


def _taps_in_3x3(c):
    """All taps of a class within a 3 x 3 window (the halo the pre-split kernels stage)."""
    dys, dxs = [c.dy[t] for t in range(c.ntaps)], [c.dx[t] for t in range(c.ntaps)]
    return max(dys) - min(dys) <= 2 and max(dxs) - min(dxs) <= 2


def conv_igemm(x, wp, Ck, Nc, out, classes, in_stride=1, out_stride=1, in_scale=None, epi=L.EPI_STORE, ksplit=1,
               out_scale=None, bias=None, noise=None, noise_nstride=0, noise_strength=None, act='linear', alpha=0.0, gain=1.0,
               clamp=-1.0, addend=None, xin=None, ds=None, algo_flops=None, precision=None, a_amax=None, a_amax_mul=1.0, out_amax=None,
               act_bwd=None, w_pieces=None, addend_up2_taps=None):
    """Launch eg3d_conv2d_igemm_f32.  x/out/addend/xin: channels_last fp32 [N,C,H,W]; wp: packed weights [Nc, taps*Ck].
    act_bwd (an ActBwdSpec, with epi=EPI_BWD): try EPI_BWD_ACT; returns True when the fused epilogue ran (out then holds the producing
    layer's dz), False when the launch was a plain EPI_BWD."""
    assert is_cl(x) and is_cl(out), 'conv_igemm expects fp32 channels_last CUDA tensors'
    if len(classes) > 4:        # (a stride-3 transposed conv has nine output phases) the classes of a store / atomic launch are independent: four per launch
        assert epi in (L.EPI_STORE, L.EPI_ATOMIC) and ds is None and out_amax is None and act_bwd is None, 'more than four tap classes: plain store launches only'
        for i in range(0, len(classes), 4):
            conv_igemm(x, wp, Ck, Nc, out, classes[i:i + 4], in_stride=in_stride, out_stride=out_stride, in_scale=in_scale, epi=epi, ksplit=ksplit,
                       out_scale=out_scale, algo_flops=None if algo_flops is None else algo_flops * min(4, len(classes) - i) / len(classes),
                       precision=precision, a_amax=a_amax, a_amax_mul=a_amax_mul, w_pieces=w_pieces)
        return False
    p = L.ConvParams()
    n, cx, hi, wi = x.shape
    _, co, ho, wo = out.shape
    p.x, p.w, p.out = x.data_ptr(), wp.data_ptr(), out.data_ptr()
    p.N, p.Hi, p.Wi, p.Ck, p.ldx = n, hi, wi, Ck, cx
    p.Nc, p.w_row = Nc, wp.stride(0)
    p.Ho, p.Wo, p.ldo = ho, wo, co
    p.in_stride, p.out_stride = in_stride, out_stride
    p.ncls = len(classes)
    for i, c in enumerate(classes):
        p.cls[i] = c
    p.in_scale = in_scale.data_ptr() if in_scale is not None else None
    p.epi, p.ksplit = epi, ksplit
    p.out_scale = out_scale.data_ptr() if out_scale is not None else None
    p.bias = bias.data_ptr() if bias is not None else None
    p.noise = noise.data_ptr() if noise is not None else None
    p.noise_nstride = noise_nstride
    p.noise_strength = noise_strength.data_ptr() if noise_strength is not None else None
    p.act, p.alpha, p.gain, p.clamp = L.ACT_IDS[act], float(alpha), float(gain), float(clamp)
    p.addend = addend.data_ptr() if addend is not None else None
    if addend_up2_taps is not None:             # addend is the half-resolution skip image, up-sampled inside the epilogue
        p.addend_up2 = 1
        p.addend_taps[:] = [float(t) for t in addend_up2_taps]
    p.xin = xin.data_ptr() if xin is not None else None
    p.ds = ds.data_ptr() if ds is not None else None
    p.precision = CONV_PRECISION if precision is None else PRECISIONS[precision]
    p.a_amax = a_amax.data_ptr() if a_amax is not None else None
    p.a_amax_mul = float(a_amax_mul)
    p.ds_replicas = ds.shape[0] if (ds is not None and ds.dim() == 3) else 1
    p.out_amax = out_amax.data_ptr() if out_amax is not None else None
    if w_pieces is not None and p.precision == PRECISIONS['f16x3']:      # the packed weights' pre-split image (split_weight_pieces): same indexing
        assert w_pieces.shape == wp.shape and w_pieces.stride() == wp.stride()
        p.w, p.w_presplit = w_pieces.data_ptr(), 1
    fused_act = act_bwd is not None and epi == L.EPI_BWD and _try_act_bwd(p, act_bwd, L.lib().eg3d_conv2d_igemm_act_bwd_ok, aligned16=False)
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_igemm_f32(C.byref(p), L.stream_ptr()), 'conv2d_igemm_f32'),
              L.lib().eg3d_conv2d_igemm_config(C.byref(p)) if PROFILER is not None else None, int(p.precision), algo_flops,
              lambda: 2.0 * Ck * Nc * sum(n * c.Ha * c.Wa * c.ntaps for c in classes),
              lambda: dict(N=n, Hi=hi, Wi=wi, Ck=Ck, Nc=Nc, Ho=ho, Wo=wo, taps=[c.ntaps for c in classes], epi=epi, ksplit=ksplit,
                           in_stride=in_stride, out_stride=out_stride, prec=p.precision))
    return fused_act if act_bwd is not None else out


# ------------------------------------------------------------------------------------------------- pre-split convolution (csrc/conv_v2.hip)
def absmax(x, out=None):
    """Device scalar max|x| (eg3d_absmax); `out`: a pre-zeroed 1-element tensor to accumulate into."""
    if out is None:
        out = zeros((1,), x.device)
    L.check(L.lib().eg3d_absmax(L.ptr(x), x.numel(), L.ptr(out), L.stream_ptr()), 'absmax')
    return out


def tag_amax(t, amax):
    """Attach the device scalar max|t| its producer kernel reported to a tensor (read back by amax_of)."""
    t._eg3d_amax = amax
    return t


def amax_of(t):
    """Device scalar max|t|: the producer's report when the tensor carries one, else one reduction pass (eg3d_absmax)."""
    a = getattr(t, '_eg3d_amax', None)
    return a if a is not None else absmax(t)


class SplitImage:
    """Two-piece fp16 image of an operand + the power-of-two scale it was written with (device scalar).

    An element v leaves as a = fl32(v * scale), hi = fp16(a) rounded toward zero, lo = fp16((a - hi) * lo_mul) rounded to nearest, and reads back as
    (hi + lo / lo_mul) / scale; scale brings the operand's range to [2^13, 2^14).
      activations   [N][2 piece][C/8][H*W][8],              lo_mul = 2048  (shape = (N, C, H, W); v = x * in_scale[n, c])
      weights       [T][I/16][2 piece][2 koct][O][8],       lo_mul = 1     (shape = (O, I, T); element w[o, tap * I + (2 chunk + koct) * 8 + lane])
    tests/support/split_ref.py restates both bit for bit (and decodes them); tests/test_gpu_split.py holds the kernels to it."""
    __slots__ = ('data', 'scale', 'shape')

    def __init__(self, data, scale, shape):
        self.data, self.scale, self.shape = data, scale, shape


def split_activation(x, x_amax, in_scale=None, s_amax=None, C=None):
    """fp32 channels_last [N,C,H,W] (times in_scale[n,c]) -> SplitImage [N][2][C/8][H][W][8] fp16, range-normalised with the device scalars
    x_amax = max|x| and s_amax = max|in_scale|."""
    assert is_cl(x)
    n, cx, h, w = x.shape
    C_ = cx if C is None else C
    img = torch.empty((n * h * w * C_ * 2,), dtype=torch.float16, device=x.device)
    scale = torch.empty((1,), dtype=torch.float32, device=x.device)
    L.check(L.lib().eg3d_split_activation(L.ptr(x), L.ptr(in_scale), L.ptr(x_amax), L.ptr(s_amax), L.ptr(img), L.ptr(scale), n, h, w, C_, cx,
                                          L.stream_ptr()), 'split_activation')
    return SplitImage(img, scale, (n, C_, h, w))


def split_weight(wp, O, I, T):
    """Packed fp32 weights [O, T*I] (forward or adjoint image; rows may be a view of a wider matrix: the kernel takes the row pitch) -> SplitImage
    [T][I/16][2][2][O][8] fp16 (unscaled low piece)."""
    assert wp.dtype == torch.float32 and tuple(wp.shape) == (O, T * I) and wp.stride(1) == 1 and wp.stride(0) >= T * I
    # eg3d_absmax reads a dense array: of a row view it would reduce the first O*T*I floats of the wider matrix (columns that are not weights, rows missing)
    amax = absmax(wp if wp.is_contiguous() else wp.contiguous())
    img = torch.empty((O * T * I * 2,), dtype=torch.float16, device=wp.device)
    scale = torch.empty((1,), dtype=torch.float32, device=wp.device)
    L.check(L.lib().eg3d_split_weight(L.ptr(wp), L.ptr(amax), L.ptr(img), L.ptr(scale), O, I, T, wp.stride(0), L.stream_ptr()), 'split_weight')
    return SplitImage(img, scale, (O, I, T))


def split_weights_batched(mats):
    """[(packed fp32 matrix [O, T*I], O, I, T), ...] -> [SplitImage, ...] from two launches per batch of SPLIT_W_BATCH_MAX (eg3d_split_weights_batched)."""
    outs = []
    for b0 in range(0, len(mats), L.SPLIT_W_BATCH_MAX):
        grp = mats[b0:b0 + L.SPLIT_W_BATCH_MAX]
        dev = grp[0][0].device
        amax = zeros((len(grp),), dev)
        scales = torch.empty((len(grp),), dtype=torch.float32, device=dev)
        b = L.SplitWBatch()
        b.n = len(grp)
        for k, (wp, O, I, T) in enumerate(grp):
            assert wp.is_contiguous() and wp.shape == (O, T * I)
            img = torch.empty((O * T * I * 2,), dtype=torch.float16, device=dev)
            it = b.items[k]
            it.w, it.image, it.scale_out, it.amax = wp.data_ptr(), img.data_ptr(), scales[k:k + 1].data_ptr(), amax[k:k + 1].data_ptr()
            it.O, it.I, it.T, it.w_row = O, I, T, T * I
            outs.append(SplitImage(img, scales[k:k + 1], (O, I, T)))
        L.check(L.lib().eg3d_split_weights_batched(C.byref(b), L.stream_ptr()), 'split_weights_batched')
    return outs


def _conv_v2_params(a, w, out, classes, out_stride, epi, out_scale, bias, noise, noise_nstride, noise_strength, act, alpha, gain, clamp,
                    addend, xin, ds, out_amax):
    p = L.ConvV2Params()
    n, ck, hi, wi = a.shape
    nc, _, wtaps = w.shape
    _, co, ho, wo = out.shape
    p.a, p.w, p.a_scale, p.w_scale, p.out = a.data.data_ptr(), w.data.data_ptr(), a.scale.data_ptr(), w.scale.data_ptr(), out.data_ptr()
    p.N, p.Hi, p.Wi, p.Ck, p.Nc, p.wtaps = n, hi, wi, ck, nc, wtaps
    p.Ho, p.Wo, p.ldo, p.in_stride, p.out_stride = ho, wo, co, 1, out_stride
    p.ncls = len(classes)
    for i, c in enumerate(classes):
        p.cls[i] = c
    p.epi = epi
    p.out_scale = out_scale.data_ptr() if out_scale is not None else None
    p.bias = bias.data_ptr() if bias is not None else None
    p.noise = noise.data_ptr() if noise is not None else None
    p.noise_nstride = noise_nstride
    p.noise_strength = noise_strength.data_ptr() if noise_strength is not None else None
    p.act, p.alpha, p.gain, p.clamp = L.ACT_IDS[act], float(alpha), float(gain), float(clamp)
    p.addend = addend.data_ptr() if addend is not None else None
    p.xin = xin.data_ptr() if xin is not None else None
    p.ds = ds.data_ptr() if ds is not None else None
    p.out_amax = out_amax.data_ptr() if out_amax is not None else None
    return p


def conv_v2_tiles(Nc, classes, N=1):
    """256-cell x 128-channel tiles of a launch of the pre-split kernel."""
    return tiles(classes, N, 8, Nc, 128)


def conv_v2_geometry_ok(Ck, Nc, classes):
    if Ck % 16 or Nc % 128 or CONV_MODE != 'auto':
        return False
    return all(c.ntaps in (9, 4, 2, 1) and _taps_in_3x3(c) for c in classes)


def conv_v2_rows(Ck, Nc, classes, N=1):
    """Patch rows (8 | 4) the pre-split kernel should run this launch with, 0 = not a launch for it.  8 x 32-cell patches when they fill the
    chip (>= V2_MIN_TILES workgroups); nine-tap classes whose 8-row grid does not but whose 4-row grid does (128^2 x 256: 128 -> 256
    workgroups) take the half-height patch -- fused epilogues intact, no split-K."""
    if not conv_v2_geometry_ok(Ck, Nc, classes):
        return 0
    tiles8 = conv_v2_tiles(Nc, classes, N)
    half_ok = V2_HALF and all(c.ntaps == 9 for c in classes)
    if half_ok and tiles8 < V2_HALF_BELOW and tiles(classes, N, 4, Nc, 128) >= V2_MIN_TILES:
        return 4
    return 8 if tiles8 >= V2_MIN_TILES else 0


def conv_v2_supported(Ck, Nc, classes, N=1):
    """Geometry the pre-split kernel takes (see eg3d_conv2d_v2_supported) AND enough tiles to fill the chip (conv_v2_rows)."""
    return conv_v2_rows(Ck, Nc, classes, N) != 0


V2_MIN_TILES = 256
USE_V2 = os.environ.get('EG3D_CONV_V2', '1') != '0'
# 4 x 32-cell patches for under-filled 3x3 grids (conv_v2_rows): 128^2 x 256: 107 -> 91 us, 256^2 x 128: 84 -> 67 us per launch.  (Off in the
# first half of round 3: with the fused epilogues a few hundred of 8 M output elements per launch came out wrong on full-size layers --
# a miscompile of the scalar epilogue arithmetic by the SLP vectoriser, see the Makefile; tests/test_gpu_ops.py::test_conv_v2_half_patch_full_size.)
# 4-row launches that give every CU at most one workgroup (128^2 x 256, 256^2 x 128 at N = 1) as eight-wave workgroups whose two halves split the contraction
# (csrc/conv_v2.hip KH = 2): two waves per SIMD instead of one
V2_KHALVES = os.environ.get('EG3D_V2_KHALVES', '1') != '0'
V2_KHALVES_MAX_TILES = 256
V2_HALF = os.environ.get('EG3D_V2_HALF', '1') != '0'             # half-height (4 x 32) patches for nine-tap launches ...
V2_HALF_BELOW = 512      # ... when the 8-row grid has fewer workgroups than this (256^2 x 128: 84 -> 67 us, 128^2 x 256: 107 -> 91 us)


def conv_v2(a: SplitImage, w: SplitImage, out, classes, out_stride=1, epi=L.EPI_STORE, out_scale=None, bias=None, noise=None, noise_nstride=0,
            noise_strength=None, act='linear', alpha=0.0, gain=1.0, clamp=-1.0, addend=None, xin=None, ds=None, out_amax=None, algo_flops=None,
            act_bwd=None, products=3, ksplit=1, patch_rows=None, rgb_head=None, rgb_head_ran=None):
    """Launch eg3d_conv2d_v2 (operands prepared by split_activation / split_weight).  act_bwd (ActBwdSpec, with epi=EPI_BWD): EPI_BWD_ACT when
    the kernel takes it -- returns True if the fused epilogue ran, False for a plain EPI_BWD.
    rgb_head (EPI_FWD, 128 output channels): (w4 [4, >= Nc] packed weight rows, styles [N, Nc], bias4 [4] | None, y4 [N,4,H,W] channels_last, clamp[, 3 = the
    fourth row is padding]) --
    the 1x1 layer that reads `out` next, evaluated in this launch's epilogue (eg3d_conv_v2_params::rgb_out); rgb_head_ran (a list): receives True / False =
    the library took / refused the head (refused: the launch runs without it)."""
    assert is_cl(out)
    p = _conv_v2_params(a, w, out, classes, out_stride, epi, out_scale, bias, noise, noise_nstride, noise_strength, act, alpha, gain, clamp,
                        addend, xin, ds, out_amax)
    p.products = int(products)
    p.ksplit = int(ksplit)
    assert ksplit <= 1 or epi == L.EPI_ATOMIC
    if patch_rows is None:          # the caller did not plan: 4-row patches where they fill the chip and 8-row ones do not
        patch_rows = conv_v2_rows(p.Ck, p.Nc, classes, p.N) if epi != L.EPI_ATOMIC else 8
    p.patch_rows = patch_rows if patch_rows in (4, 2) else 8
    if (V2_KHALVES and p.patch_rows == 4 and epi != L.EPI_ATOMIC and ksplit <= 1 and rgb_head is None and (p.Ck // 16) % 2 == 0 and p.Ck >= 64
            and tiles(classes, p.N, 4, p.Nc, 128) <= V2_KHALVES_MAX_TILES):
        # one workgroup per CU: eight waves, the contraction split over the two four-wave halves inside the workgroup (KH = 2 of conv_v2_kernel)
        p.ksplit = 2
    if rgb_head is not None:
        w4, s4, b4, y4, rclamp = rgb_head[:5]
        p.rgb_nout = int(rgb_head[5]) if len(rgb_head) > 5 else 4
        assert epi == L.EPI_FWD and is_cl(y4) and y4.shape[1] == 4 and w4.shape[0] == 4 and w4.stride(1) == 1 and s4.is_contiguous()
        p.rgb_w, p.rgb_s, p.rgb_bias, p.rgb_out = w4.data_ptr(), s4.data_ptr(), (b4.data_ptr() if b4 is not None else None), y4.data_ptr()
        p.rgb_clamp, p.rgb_ldw = float(rclamp), w4.stride(0)
        if not L.lib().eg3d_conv2d_v2_supported(C.byref(p)):        # (alignment of the head's operands, patch height ...): this launch without the head, the caller launches the 1x1 layer itself
            p.rgb_w = p.rgb_s = p.rgb_bias = p.rgb_out = None
            p.rgb_nout = 0
            rgb_head = None
        if rgb_head_ran is not None:
            rgb_head_ran.append(rgb_head is not None)
    fused_act = act_bwd is not None and epi == L.EPI_BWD and xin is not None and _try_act_bwd(p, act_bwd, L.lib().eg3d_conv2d_v2_supported)
    cfg_id = {8: V2_CONFIG, 4: V2H_CONFIG, 2: V2Q_CONFIG}[int(p.patch_rows)]   # the patch heights are different instantiations: separate profiler records
    if rgb_head is not None:
        cfg_id = V2RGB_CONFIG       # ... and so is the one with the 1x1 head (conv_v2_kernel<9,*,false,4,true>)
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_v2(C.byref(p), L.stream_ptr()), 'conv2d_v2'), cfg_id, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * p.Ck * p.Nc * sum(p.N * c.Ha * c.Wa * c.ntaps for c in classes),
              lambda: dict(N=p.N, Hi=p.Hi, Wi=p.Wi, Ck=p.Ck, Nc=p.Nc, Ho=p.Ho, Wo=p.Wo, taps=[c.ntaps for c in classes], epi=epi, ksplit=int(ksplit),
                           in_stride=1, out_stride=out_stride, prec=3, v2=True, patch_rows=int(p.patch_rows)))
    return fused_act if act_bwd is not None else out


# ------------------------------------------------------------------------------------------------- wave-split pre-split convolution (csrc/conv_v3.hip)
V3_CONFIG = 11       # profiler id of conv_v3_kernel
USE_V3 = os.environ.get('EG3D_CONV_V3', '1') != '0'
V3_MAX_TILES8 = 128       # 256-cell x 128-channel tiles below which a 3x3 launch goes to the wave-split kernel
V3_MIN_CELLS = 1024        # class grids (all images) from this many cells (32^2) -- below, launches are latency-bound


def conv_v3_plan(Ck, Nc, classes, N=1):
    """(patch_rows, waves) for eg3d_conv2d_v3, or None when the launch is not one for it: nine-tap stride-1 classes whose 256 x 128 tiling
    leaves the chip under-filled.  128-cell tiles with the contraction over four waves when they give >= 192 workgroups, else 64-cell tiles
    over eight waves (twice the workgroups, half the steps per wave)."""
    if not USE_V3 or CONV_MODE != 'auto' or Ck % 16 or Nc % 64 or not (1 <= len(classes) <= 4):
        return None
    if any(c.ntaps != 9 or not _taps_in_3x3(c) for c in classes):
        return None
    cells = sum(N * c.Ha * c.Wa for c in classes)
    tiles8 = sum(_patches(N, c.Ha, c.Wa, 8) for c in classes) * -(-Nc // 128)      # (a 64-channel remainder counts as a tile)
    if cells < V3_MIN_CELLS or tiles8 >= V3_MAX_TILES8:
        return None
    return conv_v3_tiling(classes, N, Nc)


def conv_v3_tiling(classes, N, Nc):
    """(patch_rows, waves) of a launch the wave-split kernel takes: see conv_v3_plan."""
    return (4, 4) if tiles(classes, N, 4, Nc, 64) >= 192 else (2, 8)


def conv_v3(a: SplitImage, w: SplitImage, out, classes, plan=None, out_stride=1, epi=L.EPI_STORE, out_scale=None, bias=None, noise=None, noise_nstride=0,
            noise_strength=None, act='linear', alpha=0.0, gain=1.0, clamp=-1.0, addend=None, xin=None, ds=None, out_amax=None, algo_flops=None,
            act_bwd=None, products=3):
    """Launch eg3d_conv2d_v3 (operands as for conv_v2).  plan = (patch_rows, waves).  act_bwd (ActBwdSpec, with epi=EPI_BWD): EPI_BWD_ACT when the
    kernel takes it -- returns True if the fused epilogue ran, False for a plain EPI_BWD."""
    assert is_cl(out)
    p = _conv_v2_params(a, w, out, classes, out_stride, epi, out_scale, bias, noise, noise_nstride, noise_strength, act, alpha, gain, clamp,
                        addend, xin, ds, out_amax)
    rows, waves = plan if plan is not None else (4, 4)
    p.products, p.patch_rows, p.ksplit = int(products), int(rows), int(waves)
    fused_act = act_bwd is not None and epi == L.EPI_BWD and xin is not None and _try_act_bwd(p, act_bwd, L.lib().eg3d_conv2d_v3_supported)
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_v3(C.byref(p), L.stream_ptr()), 'conv2d_v3'), V3_CONFIG, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * p.Ck * p.Nc * sum(p.N * c.Ha * c.Wa * c.ntaps for c in classes),
              lambda: dict(N=p.N, Hi=p.Hi, Wi=p.Wi, Ck=p.Ck, Nc=p.Nc, Ho=p.Ho, Wo=p.Wo, taps=[c.ntaps for c in classes], epi=epi, ksplit=int(waves),
                           in_stride=1, out_stride=out_stride, prec=3, v3=True, patch_rows=int(rows)))
    return fused_act if act_bwd is not None else out


RGB_HEAD = os.environ.get('EG3D_RGB_HEAD', '1') != '0'       # the SR head's last toRGB evaluated in conv1's forward epilogue (eg3d_conv_v2_params::rgb_out)
CONV_WS = os.environ.get('EG3D_CONV_WS', '1') != '0'
CONV_WS_MAX_CELLS = 256
CONV_WS_S2 = os.environ.get('EG3D_CONV_WS_S2', '1') != '0'      # ... and its stride-2 adjoint form for the data gradients of the 8^2 .. 32^2 up layers
WS_CONFIG = 12


def _conv_ws_params(x, w: SplitImage, out, cls, in_scale, x_amax, x_amax_mul, products, in_stride=1):
    p = L.ConvWsParams()
    n, cx, hx, wx = x.shape
    _, co, ho, wo = out.shape
    assert cls.ntaps == 9 and (cls.Ha, cls.Wa, cls.out_py, cls.out_px) == (ho, wo, 0, 0) and (in_stride == 2 or (hx, wx) == (ho, wo))
    p.x, p.in_scale, p.x_amax, p.x_amax_mul = x.data_ptr(), (in_scale.data_ptr() if in_scale is not None else None), x_amax.data_ptr(), float(x_amax_mul)
    p.w, p.w_scale, p.out = w.data.data_ptr(), w.scale.data_ptr(), out.data_ptr()
    O, I, T = w.shape
    p.N, p.H, p.W, p.Ck, p.ldx = n, ho, wo, I, cx
    p.Nc, p.ldo, p.wtaps = O, co, T
    for t in range(9):
        p.dy[t], p.dx[t], p.wtap[t] = cls.dy[t], cls.dx[t], cls.wtap[t]
    p.products = int(products)
    p.in_stride, p.Hx, p.Wx = int(in_stride), hx, wx
    return p


def conv_ws_ok(Ck, Nc, classes, N, H, W, in_stride=1):
    """A split (atomic) 3x3 launch on the weight-streaming kernel (csrc/conv_ws.hip): the stride-1 layers of the 4^2 .. 16^2 blocks at one image per GPU;
    in_stride 2: the stride-2 adjoint (data gradient of an up layer) with H x W <= 256 output cells."""
    if not (USE_V2 and CONV_WS) or CONV_MODE != 'auto' or len(classes) != 1 or classes[0].ntaps != 9 or Ck % 16 or Nc % 32 or W > 32:
        return False
    c = classes[0]
    if (c.Ha, c.Wa, c.out_py, c.out_px) != (H, W, 0, 0):
        return False
    if in_stride == 2:
        if not CONV_WS_S2 or any(not (0 <= c.dy[t] <= 2 and 0 <= c.dx[t] <= 2) for t in range(9)) or H * W > 256 or N != 1:
            return False
        return _conv_ws_geometry_ok(Ck, Nc, N, H, W, c, 2, 2 * H + 1, 2 * W + 1, 1)
    if any(abs(c.dy[t]) > 1 or abs(c.dx[t]) > 1 for t in range(9)):
        return False
    # the routing threshold, then the library's own geometry check (e.g. a 64 x 4 grid passes the cell count but not the kernel's halo-slot limit): a launch the
    # kernel refuses must fall back to the split-K implicit GEMM here, not raise from L.check later
    return N * H * W <= CONV_WS_MAX_CELLS and _conv_ws_geometry_ok(Ck, Nc, N, H, W, c, 1, H, W, 1)


def _conv_ws_geometry_ok(Ck, Nc, N, H, W, c, in_stride, Hx, Wx, out_stride):
    """eg3d_conv2d_ws_supported on the geometry alone (it reads no pointer)."""
    p = L.ConvWsParams()
    p.N, p.H, p.W, p.Ck, p.ldx, p.Nc, p.ldo, p.wtaps = N, H, W, Ck, Ck, Nc, Nc, 9
    for t in range(9):
        p.dy[t], p.dx[t], p.wtap[t] = (c.dy[t], c.dx[t], c.wtap[t]) if c is not None else (0, 0, t)
    p.products, p.in_stride, p.Hx, p.Wx, p.out_stride = 3, in_stride, Hx, Wx, out_stride
    return bool(L.lib().eg3d_conv2d_ws_supported(C.byref(p)))


def conv_ws(x, w: SplitImage, out, classes, in_scale=None, x_amax=None, x_amax_mul=1.0, products=3, algo_flops=None, in_stride=1):
    """Launch eg3d_conv2d_ws: out (pre-zeroed, channels_last fp32) += conv(x * in_scale, W) over the nine taps of classes[0]; w: split_weight image.
    in_stride 2: the stride-2 adjoint form (x: the FIR-adjointed gradient of an up layer, out: its data gradient before the style scale)."""
    assert is_cl(x) and is_cl(out) and x.dtype == torch.float32
    p = _conv_ws_params(x, w, out, classes[0], in_scale, x_amax if x_amax is not None else absmax(x), x_amax_mul, products, in_stride)
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_ws(C.byref(p), L.stream_ptr()), 'conv2d_ws'), WS_CONFIG, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * p.Ck * p.Nc * p.N * p.H * p.W * 9,
              lambda: dict(N=p.N, Hi=p.Hx, Wi=p.Wx, Ck=p.Ck, Nc=p.Nc, Ho=p.H, Wo=p.W, taps=[9], epi=L.EPI_ATOMIC, ksplit=p.Ck // 16,
                           in_stride=int(in_stride), out_stride=1, prec=3, ws=True))
    return out


CONV_WS_UP = os.environ.get('EG3D_CONV_WS_UP', '1') != '0'      # ... and its transposed form for the forward of the 8^2 block's up layer
CONV_WS_UP_MAX_CELLS = 32      # cells per output parity routed there: 4^2 -> 9^2 (25 cells) 18.9 -> 12.4 us; 8^2 -> 17^2 (81 cells: three row tiles x four parity sets per wave, 1.2 M output atomics) 18.0 -> 23.1, stays on the split-K implicit GEMM


def conv_ws_up_ok(Ck, Nc, N, H, W, max_cells=None):
    """Forward of an up layer (stride-2 transposed 3x3 conv, split-K accumulation into a zeroed buffer) on the weight-streaming kernel: 4^2 / 8^2
    input cells at one image per GPU.  max_cells: cells per output parity the caller accepts (default: the routing threshold; the kernel takes 96)."""
    return bool(USE_V2 and CONV_WS and CONV_WS_UP and CONV_MODE == 'auto' and Ck % 16 == 0 and Nc % 32 == 0 and N == 1 and (H + 1) * (W + 1) <= min(96, max_cells or CONV_WS_UP_MAX_CELLS)
                and W <= 30 and _conv_ws_geometry_ok(Ck, Nc, N, H, W, None, 1, H, W, 2))


def conv_ws_up(x, w: SplitImage, out, in_scale=None, x_amax=None, x_amax_mul=1.0, products=3, algo_flops=None):
    """Launch eg3d_conv2d_ws with out_stride 2: out [N,Co,2H+1,2W+1] (pre-zeroed, channels_last) += conv_transpose2d(x * in_scale, W, stride 2);
    w: the FORWARD split weight image (tap index 3 ky + kx)."""
    assert is_cl(x) and is_cl(out) and x.dtype == torch.float32
    p = L.ConvWsParams()
    n, cx, hx, wx = x.shape
    _, co, ho, wo = out.shape
    assert (ho, wo) == (2 * hx + 1, 2 * wx + 1)
    xa = x_amax if x_amax is not None else absmax(x)
    p.x, p.in_scale, p.x_amax, p.x_amax_mul = x.data_ptr(), (in_scale.data_ptr() if in_scale is not None else None), xa.data_ptr(), float(x_amax_mul)
    p.w, p.w_scale, p.out = w.data.data_ptr(), w.scale.data_ptr(), out.data_ptr()
    O, I, T = w.shape
    p.N, p.H, p.W, p.Ck, p.ldx = n, hx, wx, I, cx
    p.Nc, p.ldo, p.wtaps = O, co, T
    for t in range(9):
        p.dy[t], p.dx[t], p.wtap[t] = 0, 0, t
    p.products, p.in_stride, p.out_stride = int(products), 1, 2
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_ws(C.byref(p), L.stream_ptr()), 'conv2d_ws (transposed)'), WS_CONFIG, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * p.Ck * p.Nc * p.N * p.H * p.W * 9,
              lambda: dict(N=p.N, Hi=p.H, Wi=p.W, Ck=p.Ck, Nc=p.Nc, Ho=ho, Wo=wo, taps=[4, 2, 2, 1], epi=L.EPI_ATOMIC, ksplit=p.Ck // 16,
                           in_stride=1, out_stride=2, prec=3, ws=True))
    return out


def fir44_adjoint_split(dz, dz_amax, gain=4.0):
    """FIR adjoint of an up layer + operand split in one pass (eg3d_fir44_adjoint_split): dz [N,C,2Hi,2Wi] channels_last ->
    SplitImage of the four parity images of G = upfirdn2d(dz, [1,3,3,1]^2 / 64, pad 2, gain), shape (N, C, Hi + 1, Wi + 1) per parity."""
    assert is_cl(dz)
    n, c, ho, wo = dz.shape
    assert ho % 2 == 0 and wo % 2 == 0 and c % 8 == 0
    hi, wi = ho // 2, wo // 2
    img = torch.empty((int(L.lib().eg3d_fir44_adjoint_split_bytes(n, hi, wi, c)) // 2,), dtype=torch.float16, device=dz.device)
    scale = torch.empty((1,), dtype=torch.float32, device=dz.device)
    L.check(L.lib().eg3d_fir44_adjoint_split(L.ptr(dz), L.ptr(dz_amax), L.ptr(img), L.ptr(scale), n, hi, wi, c, c, float(gain), L.stream_ptr()), 'fir44_adjoint_split')
    return SplitImage(img, scale, (n, c, hi + 1, wi + 1))


V2_S2ADJ = os.environ.get('EG3D_V2_S2ADJ', '1') != '0'
S2ADJ_MIN_TILES = 256     # 128 tiles (257^2 x 128 -> 128^2 x 256): 79 us vs 65-70 on the loader-split kernel
S2ADJ_CONFIG = 7


def conv_s2adj_ok(Ck, Nc, Hi, Wi, N=1):
    """The up layers' data gradient on the parity-split kernel (csrc/conv_v2_s2adj.hip): geometry + enough 256 x 128 tiles."""
    if not (USE_V2 and V2_S2ADJ) or CONV_MODE != 'auto' or Ck % 64 or Nc % 128:
        return False
    return _patches(N, Hi, Wi, 8) * (Nc // 128) >= S2ADJ_MIN_TILES


V3_S2ADJ = os.environ.get('EG3D_V3_S2ADJ', '1') != '0'
V3_S2ADJ_MIN_CELLS = 4096


def conv_v3_s2adj_ok(Ck, Nc, Hi, Wi, N=1):
    """The up layers' data gradient on the wave-split form of the parity-split kernel (conv_v3_s2adj_kernel): the grids conv_s2adj_ok turns down
    for want of 256 x 128 tiles, from 32^2 cells."""
    if not (USE_V3 and V3_S2ADJ) or CONV_MODE != 'auto' or Ck % 16 or Nc % 64 or conv_s2adj_ok(Ck, Nc, Hi, Wi, N):
        return False
    return N * Hi * Wi >= V3_S2ADJ_MIN_CELLS


def conv_v2_s2adj(a: SplitImage, w: SplitImage, out, classes, epi=L.EPI_STORE, out_scale=None, addend=None, xin=None, ds=None, out_amax=None, algo_flops=None,
                  act_bwd=None, products=3, ksplit=1, v3=False):
    """Launch eg3d_conv2d_v2_s2adj (v3: eg3d_conv2d_v3_s2adj, the wave-split form): `a` = parity-split image of G (fir44_adjoint_split),
    `classes` = classes_convT_adjoint(...).  Returns like conv_v2."""
    assert is_cl(out) and len(classes) == 1
    fn_ok, fn, nm, cfg_id = ((L.lib().eg3d_conv2d_v3_s2adj_supported, L.lib().eg3d_conv2d_v3_s2adj, 'conv2d_v3_s2adj', V3_CONFIG) if v3 else
                             (L.lib().eg3d_conv2d_v2_s2adj_supported, L.lib().eg3d_conv2d_v2_s2adj, 'conv2d_v2_s2adj', S2ADJ_CONFIG))
    p = _conv_v2_params(a, w, out, classes, 1, epi, out_scale, None, None, 0, None, 'linear', 0.0, 1.0, -1.0, addend, xin, ds, out_amax)
    p.in_stride = 2
    p.products, p.ksplit = int(products), int(ksplit)
    fused_act = act_bwd is not None and epi == L.EPI_BWD and xin is not None and _try_act_bwd(p, act_bwd, fn_ok)
    _recorded(lambda: L.check(fn(C.byref(p), L.stream_ptr()), nm), cfg_id, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * p.Ck * p.Nc * p.N * classes[0].Ha * classes[0].Wa * 9,
              lambda: dict(N=p.N, Hi=2 * p.Hi - 1, Wi=2 * p.Wi - 1, Ck=p.Ck, Nc=p.Nc, Ho=p.Ho, Wo=p.Wo, taps=[9], epi=epi, ksplit=int(ksplit), in_stride=2,
                           out_stride=1, prec=3, v2=True))
    return fused_act if act_bwd is not None else out


V2_CONFIG = 5        # "tile configuration" id of the pre-split kernel in profiler records (eg3d_conv2d_igemm_config returns 0..4)
UP2_CONFIG = 6       # ... of the fused-parity transposed-conv kernel (csrc/conv_v2_up.hip)
V2H_CONFIG = 8       # ... of the pre-split kernel's half-height (4 x 32) patch instantiation
V2Q_CONFIG = 9       # ... of its quarter-height (2 x 32) patch instantiation
V2RGB_CONFIG = 13    # ... of the 8-row instantiation that carries the 1x1 head of the forward epilogue (eg3d_conv_v2_params::rgb_out)
V2_UP2 = os.environ.get('EG3D_V2_UP2', '1') != '0'
UP2_MIN_TILES = 256      # workgroups (512 threads, 115 KB of LDS: one per CU) below which the layer stays on the loader-split kernel
UP2_MIN_CK = 32      # 32: SR block 0 conv0 (32 -> 256 channels, 128^2 -> 256^2) too: +0.2 % on the step (A/B twice)


def conv_up2_plan(Ck, Nc, Hi, Wi, N=1):
    """(ksplit, ragged) for the fused-parity transposed-conv kernel on an Hi x Wi -> (2 Hi + 1) x (2 Wi + 1) layer, or None when the layer
    stays on the loader-split kernel.  Measured on MI355X (N = 1): 256^2 x 256 -> 513^2 x 128 172 -> 115 us, 128^2 x 256 -> 257^2 x 128
    64 -> 50 us; the 64^2 / 32^2 layers (64 / 32 workgroups) gain nothing, with or without split-K (fp32 atomics on an output four
    times the size of the input cost what they save), and would pay for the operand split pass on top.
    ragged: the launch covers the full (Hi + 1) x (Wi + 1) cell grid -- chosen when that still fits one round of workgroups (one per
    CU); otherwise the main Hi x Wi grid (perfectly tiled) + the last output row / column as border classes of the loader-split kernel."""
    if not (USE_V2 and V2_UP2) or CONV_MODE != 'auto' or Ck % 16 or Nc % 64 or Ck < UP2_MIN_CK or Hi < 8 or Wi < 32:
        return None
    # 8 x 32-cell patches (eight waves, one workgroup per CU) when they fill the chip; else 4 x 32-cell patches (conv_v2_up2r_kernel: four waves, tap-row weight
    # ring, two workgroups per CU) when THOSE do -- the backbone's 128^2 -> 256^2 layer at one image (128 -> 256 workgroups)
    if _patches(N, Hi, Wi, 8) * (Nc // 64) >= UP2_MIN_TILES:
        rows = 8
    elif UP2_ROWS4 and _patches(N, Hi, Wi, 4) * (Nc // 64) >= UP2_MIN_TILES:
        rows = 4
    else:
        return None
    # ragged: the full (Hi + 1) x (Wi + 1) cell grid in one launch when it still fits one round of workgroups (8 rows: one per CU; 4 rows: two per CU)
    ragged = _patches(N, Hi + 1, Wi + 1, rows) * (Nc // 64) <= (512 if rows == 4 else 256)
    return 1, ragged, rows


# Round 6, A/B in one session (EG3D_UP2_ROWS4=0 | 1 for ALL up2 launches): the SR layers do not care (256^2 x 256 -> 128: 116.9 vs 117.0 us -- 0.99 PFLOP/s executed
# either way, the kernel is at the matrix pipe's sustained rate, not waiting for its epilogue; 128^2 x 32 -> 256: 23.3 vs 27.4 us), the backbone's b256 conv0 leaves the
# loader-split kernel: 64.7 -> 7.9 (operand split) + 50.3 us.  Hence: 4-row patches only where the 8-row grid does not fill the chip.
UP2_ROWS4 = True


def up2_border_classes(Hi, Wi, kh=3, kw=3):
    """The last output row (y = 2 Hi) and column (x = 2 Wi) of the stride-2 transposed 3x3 conv as four tap classes of
    eg3d_conv2d_igemm_f32 (out_stride 2, in_stride 1): cells a = Hi resp. b = Wi, which the 8 x 32-patch grid of conv_up2 leaves out."""
    assert kh == 3 and kw == 3
    wt = lambda ky, kx: ky * 3 + kx                                       # noqa: E731
    return [_mk_class(1, Wi + 1, 2 * Hi, 0, [(Hi - 1, 0, wt(2, 0)), (Hi - 1, -1, wt(2, 2))]),
            _mk_class(1, Wi, 2 * Hi, 1, [(Hi - 1, 0, wt(2, 1))]),
            _mk_class(Hi, 1, 0, 2 * Wi, [(0, Wi - 1, wt(0, 2)), (-1, Wi - 1, wt(2, 2))]),
            _mk_class(Hi, 1, 1, 2 * Wi, [(0, Wi - 1, wt(1, 2))])]


def conv_up2(a: SplitImage, w: SplitImage, out, Hc=None, Wc=None, epi=L.EPI_STORE, ksplit=1, products=3, algo_flops=None, patch_rows=8):
    """Launch eg3d_conv2d_up2: out [N,Co,2Hi+1,2Wi+1] channels_last (+)= transposed 3x3 stride-2 conv of the split image `a` with the
    forward weight image `w`, for the cells a < Hc, b < Wc (default: the full (Hi + 1) x (Wi + 1) grid)."""
    assert is_cl(out)
    p = L.ConvUp2Params()
    n, ck, hi, wi = a.shape
    nc, _, wtaps = w.shape
    assert wtaps == 9
    _, co, ho, wo = out.shape
    p.a, p.w, p.a_scale, p.w_scale, p.out = a.data.data_ptr(), w.data.data_ptr(), a.scale.data_ptr(), w.scale.data_ptr(), out.data_ptr()
    p.N, p.Hi, p.Wi, p.Ck, p.Nc = n, hi, wi, ck, nc
    p.Hc, p.Wc = (hi + 1 if Hc is None else Hc), (wi + 1 if Wc is None else Wc)
    p.Ho, p.Wo, p.ldo = ho, wo, co
    for t in range(9):
        p.wtap[t] = t
    p.epi, p.products, p.ksplit, p.patch_rows = epi, int(products), int(ksplit), int(patch_rows)
    _recorded(lambda: L.check(L.lib().eg3d_conv2d_up2(C.byref(p), L.stream_ptr()), 'conv2d_up2'), UP2_CONFIG, PRECISIONS['f16x3'], algo_flops,
              lambda: 2.0 * ck * nc * n * hi * wi * 9,
              lambda: dict(N=n, Hi=hi, Wi=wi, Ck=ck, Nc=nc, Ho=ho, Wo=wo, taps=[4, 2, 2, 1], epi=epi, ksplit=int(ksplit), in_stride=1, out_stride=2,
                           prec=3, v2=True, up2=True))
    return out


def conv_wgrad(x, g, Ck, Nc, dwp, classes, in_stride=1, out_stride=1, in_scale=None, psplit=0, precision='f32', g_amax=None, g_amax_mul=1.0):
    """dwp[Nc, taps*Ck] += grad of the packed weights (dwp pre-zeroed).  precision 'f32' | 'f16x3' (g_amax: device scalar max|g|
    for the range normalisation of the gradient operand, see include/eg3d_hip.h)."""
    assert is_cl(x) and is_cl(g)
    if len(classes) > 4:        # the launch accumulates into dwp: four classes at a time
        for i in range(0, len(classes), 4):
            conv_wgrad(x, g, Ck, Nc, dwp, classes[i:i + 4], in_stride, out_stride, in_scale, psplit, precision, g_amax, g_amax_mul)
        return dwp
    p = L.WgradParams()
    n, cx, hi, wi = x.shape
    _, cg, ho, wo = g.shape
    p.x, p.g, p.dw = x.data_ptr(), g.data_ptr(), dwp.data_ptr()
    p.N, p.Hi, p.Wi, p.Ck, p.ldx = n, hi, wi, Ck, cx
    p.Nc, p.w_row = Nc, dwp.stride(0)
    p.Ho, p.Wo, p.ldg = ho, wo, cg
    p.in_stride, p.out_stride = in_stride, out_stride
    p.ncls = len(classes)
    for i, c in enumerate(classes):
        p.cls[i] = c
    p.in_scale = in_scale.data_ptr() if in_scale is not None else None
    p.psplit = psplit
    p.precision = PRECISIONS[precision]
    p.g_amax = g_amax.data_ptr() if g_amax is not None else None
    p.g_amax_mul = float(g_amax_mul)
    if DEFERRED_CONV_WGRADS is not None and precision in ('f16x3', 'f16x1'):
        # queued (deferred_weight_grads): launched together with the other layers' by flush_weight_grads; the operands stay referenced until then
        DEFERRED_CONV_WGRADS.append((p, (x, g, dwp, in_scale, g_amax)))
        return dwp
    L.check(L.lib().eg3d_conv2d_wgrad_f32(C.byref(p), L.stream_ptr()), 'conv2d_wgrad_f32')
    return dwp


WGRAD_V2 = os.environ.get('EG3D_WGRAD_V2', '1') != '0'       # weight gradients of split-image layers on csrc/conv_wgrad_v2.hip


def conv_wgrad_v2_shapes_ok(gshape, xshape, classes):
    """Operand images of equal geometry, channel counts multiples of 64, one stride-1 class of 9 (3x3) or 1 taps."""
    if not (WGRAD_V2 and USE_V2) or len(classes) != 1 or classes[0].ntaps not in (9, 1):
        return False
    n, co, h, w = gshape
    n2, ci, h2, w2 = xshape
    c = classes[0]
    return (n, h, w) == (n2, h2, w2) and co % 64 == 0 and ci % 64 == 0 and (c.Ha, c.Wa) == (h, w) and c.out_py == 0 and c.out_px == 0


def conv_wgrad_v2_ok(gimg, ximg, classes):
    """Both operands at hand as SplitImages that conv_wgrad_v2_shapes_ok accepts."""
    return gimg is not None and ximg is not None and conv_wgrad_v2_shapes_ok(gimg.shape, ximg.shape, classes)


WGRAD_SLABS = os.environ.get('EG3D_WGRAD_SLABS', '0') != '0'   # partial weight-gradient tiles stored to slabs and summed in order (no atomics)


def _wgrad_v2_params(gimg, ximg, classes, products, row_groups):
    p = L.WgradV2Params()
    n, co, h, w = gimg.shape
    _, ci, _, _ = ximg.shape
    c = classes[0]
    p.g, p.x, p.g_scale, p.x_scale = gimg.data.data_ptr(), ximg.data.data_ptr(), gimg.scale.data_ptr(), ximg.scale.data_ptr()
    p.N, p.H, p.W, p.Co, p.Ci, p.w_row = n, h, w, co, ci, c.ntaps * ci
    p.ntaps = c.ntaps
    for t in range(c.ntaps):
        p.dy[t], p.dx[t], p.wtap[t] = c.dy[t], c.dx[t], c.wtap[t]
    p.products, p.row_groups = int(products), int(row_groups)
    return p


def conv_wgrad_v2(gimg: SplitImage, ximg: SplitImage, dwp, classes, products=3, row_groups=0):
    """dwp[Co, taps*Ci] += weight gradient from the split images of dz (gimg) and of the modulated input (ximg) (eg3d_conv2d_wgrad_v2)."""
    p = _wgrad_v2_params(gimg, ximg, classes, products, row_groups)
    p.dw, p.w_row, p.slabs = dwp.data_ptr(), dwp.stride(0), 0
    L.check(L.lib().eg3d_conv2d_wgrad_v2(C.byref(p), L.stream_ptr()), 'conv2d_wgrad_v2')
    return dwp


WGRAD_V2_UP = os.environ.get('EG3D_WGRAD_V2_UP', '1') != '0'
WGRAD_V2_UP_MIN_CELLS = 1024      # input cells (32^2) from which an up layer's weight gradient takes the parity-split kernel


def conv_wgrad_v2_up_ok(Ci, Co, Hi, Wi, N=1):
    """An up-sampling layer's weight gradient on conv_wgrad_v2_up_kernel (parity-split G image x split X image)."""
    return bool(WGRAD_V2 and WGRAD_V2_UP and USE_V2 and CONV_MODE == 'auto' and Ci % 64 == 0 and Co % 64 == 0 and N * Hi * Wi >= WGRAD_V2_UP_MIN_CELLS)


def conv_wgrad_v2_up(gimg: SplitImage, ximg: SplitImage, dwp, wtaps, products=3, row_groups=0):
    """dwp[Co, 9*Ci] += weight gradient of a stride-2 3x3 transposed conv from the parity-split image of its gradient operand (fir44_adjoint_split) and
    the split image of its modulated input; wtaps[3 ky + kx] = weight tap (eg3d_conv2d_wgrad_v2_up)."""
    p = L.WgradV2Params()
    n, ci, h, w = ximg.shape
    co = gimg.shape[1]
    p.g, p.x, p.g_scale, p.x_scale = gimg.data.data_ptr(), ximg.data.data_ptr(), gimg.scale.data_ptr(), ximg.scale.data_ptr()
    p.N, p.H, p.W, p.Co, p.Ci = n, h, w, co, ci
    p.ntaps = 9
    for t in range(9):
        p.dy[t], p.dx[t], p.wtap[t] = 0, 0, int(wtaps[t])
    p.products, p.row_groups, p.slabs = int(products), int(row_groups), 0
    p.dw, p.w_row = dwp.data_ptr(), dwp.stride(0)
    L.check(L.lib().eg3d_conv2d_wgrad_v2_up(C.byref(p), L.stream_ptr()), 'conv2d_wgrad_v2_up')
    return dwp


def conv_wgrad_v2_slabs(gimg: SplitImage, ximg: SplitImage, classes, products=3, row_groups=0):
    """The same without atomics: returns slabs [nslab, Co, taps*Ci] of partial gradients whose sum IN SLAB ORDER is the gradient
    (weight_grad_finish(slabs, ...) sums them; torch.sum(0) for tests)."""
    p = _wgrad_v2_params(gimg, ximg, classes, products, row_groups)
    ns = int(L.lib().eg3d_conv2d_wgrad_v2_slabs(C.byref(p)))
    if ns < 1:
        raise L.Eg3dHipError(f'conv2d_wgrad_v2_slabs: {ns}')
    slabs = torch.empty((ns, p.Co, p.w_row), dtype=torch.float32, device=gimg.data.device)
    p.dw, p.slabs = slabs.data_ptr(), 1
    L.check(L.lib().eg3d_conv2d_wgrad_v2(C.byref(p), L.stream_ptr()), 'conv2d_wgrad_v2')
    return slabs


# ------------------------------------------------------------------------------------------------- epilogues
def epilogue_fwd(z, out, fir=None, pad0=0, fir_gain=1.0, d=None, noise=None, noise_nstride=0, noise_strength=None, bias=None,
                 act='linear', alpha=0.0, gain=1.0, clamp=-1.0, out_amax=None):
    assert is_cl(z) and is_cl(out)
    n, c, h, w = out.shape
    _, _, hz, wz = z.shape
    fh, fw = (fir.shape if fir is not None else (0, 0))
    L.check(L.lib().eg3d_modconv_epilogue_fwd(L.ptr(z), L.ptr(out), n, h, w, c, hz, wz, L.ptr(fir), fh, fw, pad0, float(fir_gain),
                                              L.ptr(d), L.ptr(noise), noise_nstride, L.ptr(noise_strength), L.ptr(bias),
                                              L.ACT_IDS[act], float(alpha), float(gain), float(clamp), L.ptr(out_amax), L.stream_ptr()),
            'modconv_epilogue_fwd')
    return out


UPCONV_EPI = os.environ.get('EG3D_UPCONV_EPI', '1') != '0'       # LDS-staged separable FIR epilogue for the up layers (eg3d_upconv_epilogue_fwd)
UPCONV_EPI_SPLIT = os.environ.get('EG3D_UPCONV_EPI_SPLIT', '1') != '0'   # ... that also writes the consumer's split operand image (clamp-bounded layers)
_K4 = (C.c_float * 4)(0.125, 0.375, 0.375, 0.125)


def upconv_epilogue_fwd(z, out, pad0=1, fir_gain=4.0, d=None, noise=None, noise_nstride=0, noise_strength=None, bias=None, act='linear', alpha=0.0, gain=1.0,
                        clamp=-1.0, out_amax=None, split_in_scale=None):
    """eg3d_upconv_epilogue_fwd with the [1,3,3,1] / 8 taps.  split_in_scale (the consumer layer's styles [N,C]; needs clamp >= 0): also returns
    that layer's SplitImage of `out`."""
    assert is_cl(z) and is_cl(out)
    n, c, h, w = out.shape
    _, _, hz, wz = z.shape
    img = scale = None
    if split_in_scale is not None:
        img = torch.empty((n * h * w * c * 2,), dtype=torch.float16, device=out.device)
        scale = torch.empty((1,), dtype=torch.float32, device=out.device)
    L.check(L.lib().eg3d_upconv_epilogue_fwd(L.ptr(z), L.ptr(out), n, h, w, c, hz, wz, _K4, pad0, float(fir_gain), L.ptr(d), L.ptr(noise), noise_nstride,
                                             L.ptr(noise_strength), L.ptr(bias), L.ACT_IDS[act], float(alpha), float(gain), float(clamp), L.ptr(out_amax),
                                             L.ptr(split_in_scale), L.ptr(img), L.ptr(scale), L.stream_ptr()), 'upconv_epilogue_fwd')
    return SplitImage(img, scale, (n, c, h, w)) if img is not None else None


def epilogue_bwd(dout, out, dz, d=None, noise=None, noise_nstride=0, noise_strength=None, bias=None, act='linear', alpha=0.0, gain=1.0,
                 clamp=-1.0, dbias=None, dd=None, dnoise=None, dnoise_nstride=0, dstrength=None, dz_amax=None):
    assert is_cl(dout) and is_cl(out) and is_cl(dz)
    n, c, h, w = out.shape
    L.check(L.lib().eg3d_modconv_epilogue_bwd(L.ptr(dout), L.ptr(out), L.ptr(dz), n, h, w, c, L.ptr(d), L.ptr(noise), noise_nstride,
                                              L.ptr(noise_strength), L.ptr(bias), L.ACT_IDS[act], float(alpha), float(gain),
                                              float(clamp), L.ptr(dbias), L.ptr(dd), L.ptr(dnoise), dnoise_nstride, L.ptr(dstrength),
                                              L.ptr(dz_amax), L.stream_ptr()), 'modconv_epilogue_bwd')
    return dz


def dgrad_finish(z, x, s, dx, ds=None, addend=None):
    n, c, h, w = z.shape
    L.check(L.lib().eg3d_dgrad_finish(L.ptr(z), L.ptr(x), L.ptr(s), L.ptr(addend), L.ptr(dx), L.ptr(ds), n, h, w, c, L.stream_ptr()), 'dgrad_finish')
    return dx


def dgrad_finish_act(z, x, s, dz, act_bwd, ds=None, addend=None, dz_amax=None):
    """eg3d_dgrad_finish_act: split-K finish + the activation backward of the layer that produced x; dz receives THAT layer's dz."""
    n, c, h, w = z.shape
    ab = L.ActBwd()
    act_bwd.fill(ab)
    L.check(L.lib().eg3d_dgrad_finish_act(L.ptr(z), L.ptr(x), L.ptr(s), L.ptr(addend), L.ptr(dz), L.ptr(ds), n, h, w, c, C.byref(ab), L.ptr(dz_amax),
                                          L.stream_ptr()), 'dgrad_finish_act')
    return dz


def torgb_dgrad_act(dy4, wa4, x, s, dz, act_bwd, ds=None, addend=None, dz_amax=None):
    """eg3d_torgb_dgrad_act: data gradient of a 1x1 layer with four (padded) outputs + the activation backward of the layer that produced x,
    one element-wise pass.  dy4 [N,4,H,W] channels_last, wa4 [C,4] contiguous; dz receives the producing layer's dz."""
    n, c, h, w = x.shape
    assert is_cl(dy4) and dy4.shape[1] == 4 and tuple(wa4.shape) == (c, 4) and wa4.is_contiguous()
    ab = L.ActBwd()
    act_bwd.fill(ab)
    L.check(L.lib().eg3d_torgb_dgrad_act(L.ptr(dy4), L.ptr(wa4), L.ptr(x), L.ptr(s), L.ptr(addend), L.ptr(dz), L.ptr(ds), n, h, w, c, C.byref(ab), L.ptr(dz_amax),
                                         L.stream_ptr()), 'torgb_dgrad_act')
    return dz


def torgb_dgrad_act_split(dy4, wa4, x, s, act_bwd, dy_amax, ds=None, addend=None, addend_amax=None, dz=None):
    """eg3d_torgb_dgrad_act_split: torgb_dgrad_act whose dz leaves as the SplitImage the consuming data gradient reads (no split pass, and no
    fp32 dz unless `dz` is given).  dy_amax / addend_amax: device scalars max|dy4| / max|addend|."""
    n, c, h, w = x.shape
    assert is_cl(dy4) and dy4.shape[1] == 4 and tuple(wa4.shape) == (c, 4) and wa4.is_contiguous() and c % 8 == 0
    ab = L.ActBwd()
    act_bwd.fill(ab)
    img = torch.empty((n * h * w * c * 2,), dtype=torch.float16, device=x.device)
    scale = torch.empty((1,), dtype=torch.float32, device=x.device)
    L.check(L.lib().eg3d_torgb_dgrad_act_split(L.ptr(dy4), L.ptr(wa4), L.ptr(x), L.ptr(s), L.ptr(addend), L.ptr(dz), L.ptr(ds), n, h, w, c, C.byref(ab),
                                               L.ptr(dy_amax), L.ptr(addend_amax), L.ptr(img), L.ptr(scale), L.stream_ptr()), 'torgb_dgrad_act_split')
    return SplitImage(img, scale, (n, c, h, w))


def rows_gram(a, b, out_scale=1.0, colsum_scale=1.0):
    """(out_scale * a^T b [Ka,Kb], colsum_scale * column sums of a [Ka]) for row matrices a [S,Ka], b [S,Kb] with Ka, Kb <= 64 (eg3d_rows_gram_scaled)."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.is_contiguous() and b.is_contiguous()
    z = zeros((a.shape[1] * b.shape[1] + a.shape[1],), a.device)
    out, cs = z[:a.shape[1] * b.shape[1]].view(a.shape[1], b.shape[1]), z[a.shape[1] * b.shape[1]:]
    L.check(L.lib().eg3d_rows_gram_scaled(L.ptr(a), L.ptr(b), a.shape[0], a.shape[1], b.shape[1], L.ptr(out), L.ptr(cs), float(out_scale), float(colsum_scale),
                                          L.stream_ptr()), 'rows_gram')
    return out, cs


def style_affine(ws, layers, outs=None, douts=None, dws=None, demod=None, backward=False, dweights=None, dbiases=None):
    """eg3d_style_affine_fwd / _bwd.  ws: [N,L,D] contiguous fp32; layers: sequence of (weight [C,D], bias [C] | None, wrow, wgain,
    bgain, post); outs: per-layer [N,C] styles (written by fwd, read by bwd); demod: per layer None or (wsq [Co,C], d [N,Co],
    dd [N,Co] | None, dout_extra [N,C] | None) -- the demodulation coefficients of the layer's conv and their backward;
    dweights / dbiases: per layer None or the tensor that receives the gradient of that layer's affine weight / bias (backward)."""
    assert ws.is_contiguous() and ws.dtype == torch.float32 and len(layers) <= L.STYLE_BANK_MAX
    b = L.StyleBank()
    b.ws, b.N, b.L, b.D, b.nlayers = ws.data_ptr(), ws.shape[0], ws.shape[1], ws.shape[2], len(layers)
    b.dws = dws.data_ptr() if dws is not None else None
    for i, (w, bias, wrow, wgain, bgain, post) in enumerate(layers):
        ly = b.layers[i]
        assert w.is_contiguous() and w.dtype == torch.float32 and w.shape[1] == b.D
        ly.weight, ly.bias = w.data_ptr(), (bias.data_ptr() if bias is not None else None)
        ly.C, ly.wrow, ly.wgain, ly.bgain, ly.post = w.shape[0], int(wrow), float(wgain), float(bgain), float(post)
        ly.out = outs[i].data_ptr() if outs is not None else None
        ly.dout = douts[i].data_ptr() if (douts is not None and douts[i] is not None) else None
        if dweights is not None and dweights[i] is not None:
            assert dweights[i].is_contiguous() and dweights[i].shape == w.shape
            ly.dweight = dweights[i].data_ptr()
        if dbiases is not None and dbiases[i] is not None:
            ly.dbias = dbiases[i].data_ptr()
        dm = demod[i] if demod is not None else None
        if dm is not None:
            wsq, d, dd, extra = dm
            assert wsq.is_contiguous() and wsq.shape[1] == w.shape[0]
            ly.Co, ly.wsq, ly.d = wsq.shape[0], wsq.data_ptr(), d.data_ptr()
            ly.dd = dd.data_ptr() if dd is not None else None
            ly.dout_extra = extra.data_ptr() if extra is not None else None
    fn = L.lib().eg3d_style_affine_bwd if backward else L.lib().eg3d_style_affine_fwd
    L.check(fn(C.byref(b), L.stream_ptr()), 'style_affine')


def pack_conv_weight(w):
    """[O,I,kh,kw] fp32 contiguous -> (wf [O, taps*I], wa [I, taps*O], wsq [O,I]) in one launch (eg3d_pack_conv_weight)."""
    L.require_cuda(w)
    w = w.detach().contiguous().float()
    o, i, kh, kw = w.shape
    wf = torch.empty((o, kh * kw * i), device=w.device)
    wa = torch.empty((i, kh * kw * o), device=w.device)
    wsq = torch.empty((o, i), device=w.device)
    L.check(L.lib().eg3d_pack_conv_weight(w.data_ptr(), wf.data_ptr(), wa.data_ptr(), wsq.data_ptr(), o, i, kh * kw, L.stream_ptr()), 'pack_conv_weight')
    return wf, wa, wsq


def pack_conv_weight_padded(w, wf_p, wa_p, o_pad):
    """eg3d_pack_conv_weight_padded into caller-owned, zero-initialised buffers wf_p [o_pad, taps*I], wa_p [I, taps*o_pad]."""
    L.require_cuda(w, wf_p, wa_p)
    w = w.detach().contiguous().float()
    o, i, kh, kw = w.shape
    assert tuple(wf_p.shape) == (o_pad, kh * kw * i) and tuple(wa_p.shape) == (i, kh * kw * o_pad) and wf_p.is_contiguous() and wa_p.is_contiguous()
    L.check(L.lib().eg3d_pack_conv_weight_padded(w.data_ptr(), wf_p.data_ptr(), wa_p.data_ptr(), None, o, i, kh * kw, o_pad, L.stream_ptr()),
            'pack_conv_weight_padded')


def split_weight_pieces(wp):
    """The two-piece fp16 image of a packed weight matrix for conv_igemm(..., w_pieces=): element group [4j..4j+3] -> 4 high + 4 low fp16
    pieces in the same 16 bytes (eg3d_split_weight_pieces).  Returned as a float32-typed tensor of wp's shape (it holds fp16 bit patterns)."""
    L.require_cuda(wp)
    assert wp.is_contiguous() and wp.dtype == torch.float32 and wp.numel() % 4 == 0
    img = torch.empty_like(wp)
    L.check(L.lib().eg3d_split_weight_pieces(wp.data_ptr(), img.data_ptr(), wp.numel(), L.stream_ptr()), 'split_weight_pieces')
    return img


def pack_conv_weights_batched(items):
    """items: list of (w [O,I,kh,kw], wf, wa | None, wsq | None, o_pad[, oscale [O] | None]) with caller-allocated outputs (eg3d_pack_conv_weights_batched);
    one launch per L.PACK_BATCH_MAX layers."""
    for a in range(0, len(items), L.PACK_BATCH_MAX):
        chunk = items[a:a + L.PACK_BATCH_MAX]
        arr = (L.PackItem * len(chunk))()
        for q, item in zip(arr, chunk):
            w, wf, wa, wsq, o_pad = item[:5]
            oscale = item[5] if len(item) > 5 else None          # [O]: folded into both images (eg3d_pack_item::oscale)
            L.require_cuda(w, wf)
            assert w.is_contiguous() and w.dtype == torch.float32
            o, i, kh, kw = w.shape
            q.w, q.wf, q.wa, q.wsq = w.data_ptr(), wf.data_ptr(), L.ptr(wa), L.ptr(wsq)
            q.O, q.I, q.T, q.O_pad = o, i, kh * kw, int(o_pad)
            q.oscale = L.ptr(oscale)
        L.check(L.lib().eg3d_pack_conv_weights_batched(arr, len(chunk), L.stream_ptr()), 'pack_conv_weights_batched')


DEFERRED_WGRADS = None         # a list while `deferred_weight_grads()` is active: weight_grad_finish() queues its arguments there and returns None
DEFERRED_CONV_WGRADS = None    # ... and conv_wgrad() its launch parameters (eg3d_conv2d_wgrad_batched: the small layers fill the chip only together)
BATCH_CONV_WGRADS = os.environ.get('EG3D_BATCH_CONV_WGRADS', '1') != '0'


@contextlib.contextmanager
def deferred_weight_grads():
    """Pivotal tuning: the conv layers' backward passes queue their packed weight-gradient images instead of launching one
    eg3d_weight_grad_finish each (17 launches of 5 - 13 us); `flush_weight_grads(queue)` turns all of them into the parameters' `.grad` with one
    launch (eg3d_weight_grad_finish_batched).  Inside the context the layers return NO gradient for their weights through autograd --
    only a caller that flushes before its optimiser step may use it (inversion.PivotalTuner does)."""
    global DEFERRED_WGRADS, DEFERRED_CONV_WGRADS
    prev, DEFERRED_WGRADS = DEFERRED_WGRADS, []
    prev_c, DEFERRED_CONV_WGRADS = DEFERRED_CONV_WGRADS, ([] if BATCH_CONV_WGRADS else None)
    DEFERRED_WGRADS.append(DEFERRED_CONV_WGRADS)          # (slot 0 of the queue: the conv launches, which the finishing pass depends on)
    try:
        yield DEFERRED_WGRADS
    finally:
        DEFERRED_WGRADS, DEFERRED_CONV_WGRADS = prev, prev_c


_WGRAD_BUFS = {}               # id(weight) -> (weakref(weight), persistent gradient buffer): the same storage every step (graph replay)


def flush_weight_grads(queue):
    """One launch for everything `deferred_weight_grads()` queued; sets / accumulates `weight.grad`."""
    if not queue:
        return
    convs, queue = queue[0], queue[1:]
    if convs:              # first the queued weight-gradient GEMMs themselves, five layers per launch
        arr = (L.WgradParams * len(convs))(*[p for p, _ in convs])
        L.check(L.lib().eg3d_conv2d_wgrad_batched(arr, len(convs), L.stream_ptr()), 'conv2d_wgrad_batched')
        keep_for_capture(*[t for _, ts in convs for t in ts if t is not None])
    for a in range(0, len(queue), L.WGF_BATCH_MAX):
        chunk = queue[a:a + L.WGF_BATCH_MAX]
        arr = (L.WgfItem * len(chunk))()
        outs = []
        for q, (dwp, weight, styles, d, dd) in zip(arr, chunk):
            w = weight.detach()
            assert w.is_contiguous() and w.dtype == torch.float32
            o, i, kh, kw = w.shape
            ent = _WGRAD_BUFS.get(id(weight))
            if ent is None or ent[0]() is not weight or ent[1].shape != w.shape:
                if len(_WGRAD_BUFS) > 512:
                    _WGRAD_BUFS.clear()
                ent = (weakref.ref(weight), torch.empty_like(w))
                _WGRAD_BUFS[id(weight)] = ent
            dw = ent[1]
            q.g, q.w, q.s, q.d, q.dd, q.dw = dwp.data_ptr(), w.data_ptr(), L.ptr(styles), L.ptr(d), L.ptr(dd), dw.data_ptr()
            q.N, q.O, q.I, q.T = (styles.shape[0] if styles is not None else 1), o, i, kh * kw
            if dwp.dim() == 3:
                assert dwp.is_contiguous() and dwp.shape[1:] == (o, kh * kw * i)
                q.nslab, q.slab_stride = dwp.shape[0], dwp.stride(0)
            else:
                q.nslab, q.slab_stride = 1, 0
            outs.append((weight, dw))
        L.check(L.lib().eg3d_weight_grad_finish_batched(arr, len(chunk), L.stream_ptr()), 'weight_grad_finish_batched')
        keep_for_capture(*[t for item in chunk for t in item if torch.is_tensor(t)])
        for weight, dw in outs:
            if weight.grad is None:
                weight.grad = dw
            elif weight.grad.data_ptr() != dw.data_ptr():
                weight.grad.add_(dw)
            # (else: the optimiser kept last step's buffer as .grad -- it now holds this step's gradient)


def weight_grad_finish(dwp, weight, styles, d, dd):
    """[O,I,kh,kw] gradient of a demodulated modulated conv weight from the packed weight-gradient image dwp [O, taps*I] and the
    demodulation path (eg3d_weight_grad_finish); dd None: no demodulation term."""
    L.require_cuda(dwp, weight)
    if DEFERRED_WGRADS is not None and weight.is_contiguous() and weight.dtype == torch.float32:
        DEFERRED_WGRADS.append((dwp, weight, styles, d, dd))
        return None
    w = weight.detach().contiguous().float()
    o, i, kh, kw = w.shape
    dw = torch.empty_like(w)
    n = styles.shape[0] if styles is not None else 1
    if dwp.dim() == 3:          # slabs [nslab, O, taps*I] (conv_wgrad_v2_slabs): summed in slab order by the same pass
        assert dwp.is_contiguous() and dwp.shape[1:] == (o, kh * kw * i)
        L.check(L.lib().eg3d_weight_grad_finish_slabs(dwp.data_ptr(), dwp.shape[0], dwp.stride(0), w.data_ptr(), L.ptr(styles), L.ptr(d), L.ptr(dd),
                                                      dw.data_ptr(), n, o, i, kh * kw, L.stream_ptr()), 'weight_grad_finish_slabs')
        return dw
    L.check(L.lib().eg3d_weight_grad_finish(dwp.data_ptr(), w.data_ptr(), L.ptr(styles), L.ptr(d), L.ptr(dd), dw.data_ptr(), n, o, i, kh * kw,
                                            L.stream_ptr()), 'weight_grad_finish')
    return dw


def weight_sqsum(wp, Co, ntaps, Ck):
    wsq = torch.empty((Co, Ck), dtype=torch.float32, device=wp.device)
    L.check(L.lib().eg3d_weight_sqsum(L.ptr(wp), L.ptr(wsq), Co, ntaps, Ck, L.stream_ptr()), 'weight_sqsum')
    return wsq


def demod_fwd(s, wsq):
    n, ck = s.shape
    co = wsq.shape[0]
    d = torch.empty((n, co), dtype=torch.float32, device=s.device)
    L.check(L.lib().eg3d_demod_fwd(L.ptr(s), L.ptr(wsq), L.ptr(d), n, co, ck, L.stream_ptr()), 'demod_fwd')
    return d


def demod_bwd(s, wsq, d, dd, ds=None, dwsq=None):
    n, ck = s.shape
    co = wsq.shape[0]
    L.check(L.lib().eg3d_demod_bwd(L.ptr(s), L.ptr(wsq), L.ptr(d), L.ptr(dd), L.ptr(ds), L.ptr(dwsq), n, co, ck, L.stream_ptr()),
            'demod_bwd')


# ------------------------------------------------------------------------------------------------- renderer
def ray_gen_fwd(c2w, K, res):
    n = c2w.shape[0]
    o = torch.empty((n, res * res, 3), dtype=torch.float32, device=c2w.device)
    d = torch.empty_like(o)
    L.check(L.lib().eg3d_ray_gen_fwd(L.ptr(c2w), L.ptr(K), L.ptr(o), L.ptr(d), n, res, L.stream_ptr()), 'ray_gen_fwd')
    return o, d


def ray_gen_bwd(c2w, K, g_o, g_d, res, want_K=True):
    n = c2w.shape[0]
    d_c2w = torch.empty((n, 4, 4), dtype=torch.float32, device=c2w.device)
    d_K = torch.empty((n, 3, 3), dtype=torch.float32, device=c2w.device) if want_K else None
    L.check(L.lib().eg3d_ray_gen_bwd(L.ptr(c2w), L.ptr(K), L.ptr(g_o), L.ptr(g_d), L.ptr(d_c2w), L.ptr(d_K), n, res, L.stream_ptr()),
            'ray_gen_bwd')
    return d_c2w, d_K


SCATTER_F16 = True      # tri-plane gradient accumulation with three fp16 products per fp32 product (scatter_accum16h): 128 -> 112 us, C2 +0.4 % (round 6, three alternating pairs); False = exact fp32 products (scatter_accum16p)


def make_render_params(planes, origins, dirs, u1, u2, opts, w0, b0, w1t, b1, rgb, depth, wsum, minmax, fine, ray_limits=None, save=None, ray_tile_width=None, pos_rows=None,
                       feat_rows=None, dbg=None):
    """planes: channels_last [N, 3*C, Hp, Wp]; decoder weights with gains folded (w1t transposed [H, 1+Cout])."""
    assert is_cl(planes)
    p = L.RenderParams()
    n, c3, hp, wp = planes.shape
    p.planes, p.N, p.Hp, p.Wp, p.ldp, p.C = planes.data_ptr(), n, hp, wp, c3, c3 // 3
    p.origins, p.dirs, p.R = origins.data_ptr(), dirs.data_ptr(), origins.shape[1]
    p.u1 = u1.data_ptr()
    p.u2 = u2.data_ptr() if u2 is not None else None
    p.Dc, p.Df = int(opts['depth_resolution']), int(opts['depth_resolution_importance'])
    if ray_limits is not None:
        p.ray_limits = ray_limits.data_ptr()
        p.ray_start = p.ray_end = 0.0
    else:
        p.ray_limits = None
        p.ray_start, p.ray_end = float(opts['ray_start']), float(opts['ray_end'])
    p.disparity = int(bool(opts.get('disparity_space_sampling', False)))
    p.box_warp = float(opts['box_warp'])
    p.white_back = int(bool(opts.get('white_back', False)))
    p.w0, p.b0, p.w1, p.b1 = w0.data_ptr(), b0.data_ptr(), w1t.data_ptr(), b1.data_ptr()
    p.Hdim, p.Cout = w0.shape[0], w1t.shape[1] - 1
    p.rgb = rgb.data_ptr() if rgb is not None else None
    p.depth = depth.data_ptr() if depth is not None else None
    p.wsum = wsum.data_ptr() if wsum is not None else None
    p.depth_minmax = minmax.data_ptr() if minmax is not None else None
    p.fine_depths = fine.data_ptr() if fine is not None else None
    if save is not None:
        p.save_sigma, p.save_rgb = save[0].data_ptr(), save[1].data_ptr()
    if ray_tile_width is None:          # RaySampler emits the pixels of a square image in row-major order (ray_sampler.py:43-48)
        side = int(round(p.R ** 0.5))
        ray_tile_width = side if side * side == p.R and side % 32 == 0 else 0
    p.ray_tile_width = int(ray_tile_width)
    p.pos_rows = pos_rows.data_ptr() if pos_rows is not None else None       # workspace [2, N*R, D, 4]: selects the pipelined forward
    p.feat_rows = feat_rows.data_ptr() if feat_rows is not None else None    # [S, 32]: gather as its own pass, rows re-read by the decoder kernels
    if dbg is not None:                  # (int32 [N*R, Df, 3], int32 [N*R, Dc + Df]): the sampler's integer side (include/eg3d_hip.h)
        p.dbg_inds, p.dbg_ranks = dbg[0].data_ptr(), dbg[1].data_ptr()
        p.dbg_cdf = dbg[2].data_ptr() if len(dbg) > 2 and dbg[2] is not None else None
    return p


def render_sizes(p):
    """Element counts of every caller-owned renderer buffer (eg3d_render_query_sizes): the host allocates from the library's own answer."""
    z = L.RenderSizes()
    L.check(L.lib().eg3d_render_query_sizes(C.byref(p), C.byref(z)), 'render_query_sizes')
    return z


def render_fwd(p):
    L.check(L.lib().eg3d_render_fwd(C.byref(p), L.stream_ptr()), 'render_fwd')


def render_finalize(depth, minmax):
    L.check(L.lib().eg3d_render_finalize(L.ptr(depth), L.ptr(minmax), depth.numel(), L.stream_ptr()), 'render_finalize')


def render_bwd(p, d_rgb, d_depth, d_wsum, d_planes, d_origins, d_dirs, dumps=None, gram=None):
    """d_planes (pre-zeroed, channels_last [N,3C,Hp,Wp]) is filled by the tile-binned scatter of the dumped rows."""
    bp = L.RenderBwdParams()
    bp.fwd = p
    bp.depth_out = None
    bp.d_rgb = d_rgb.data_ptr()
    bp.d_depth = d_depth.data_ptr() if d_depth is not None else None
    bp.d_wsum = d_wsum.data_ptr() if d_wsum is not None else None
    rows = pos = None
    D = max(p.Dc, p.Df)
    z = render_sizes(p)
    S = z.S
    dev = d_rgb.device
    ag = torch.empty(z.ag_rows, dtype=torch.float32, device=dev)
    bp.ag_rows = ag.data_ptr()
    if d_origins is not None or d_dirs is not None:
        gc = torch.empty(z.gc_rows, dtype=torch.float32, device=dev)
        bp.gc_rows = gc.data_ptr()
    pos = torch.empty(z.df_pos, dtype=torch.float32, device=dev)        # (x, y, z, depth) per sample row, NaN = absent
    bp.df_pos = pos.data_ptr()
    if d_planes is not None:
        rows = torch.empty(z.df_rows, dtype=torch.float32, device=dev)
        bp.df_rows = rows.data_ptr()
    bp.d_origins = d_origins.data_ptr() if d_origins is not None else None
    bp.d_dirs = d_dirs.data_ptr() if d_dirs is not None else None
    if dumps is not None:
        bp.dump_dpre, bp.dump_h, bp.dump_dout, bp.dump_feat = [t.data_ptr() for t in dumps]
    if gram is not None:        # (w0 [64,32], b0 [64], w1 [33,64], b1 [33] pre-zeroed, scale0, scale1, bias_scale): contracted inside the sample-level kernel
        bp.gram_w0, bp.gram_b0, bp.gram_w1, bp.gram_b1 = [t.data_ptr() for t in gram[:4]]
        bp.gram_scale0, bp.gram_scale1, bp.gram_bias_scale = float(gram[4]), float(gram[5]), float(gram[6])
        if p.feat_rows and bp.dump_feat == p.feat_rows:         # the caller uses the saved feature rows as that operand: nothing to dump
            bp.dump_feat = None
    amax = None
    if d_planes is not None and SCATTER_F16:        # plane-gradient accumulation on the 16-bit matrix cores: needs max|df_rows| (written by the call)
        amax = torch.empty(1, dtype=torch.float32, device=dev)
        bp.df_amax = amax.data_ptr()
    L.check(L.lib().eg3d_render_bwd(C.byref(bp), L.stream_ptr()), 'render_bwd')
    if d_planes is not None:
        rw = math.isqrt(p.R)            # rays are generated row by row over a square image (ray_sampler.py:41-50): a hint for the binning order only
        triplane_scatter(rows, pos, d_planes, p.box_warp, ray_w=rw if rw * rw == p.R else 0, rows_per_ray=2 * D, amax=amax)


def triplane_scatter(rows, pos, d_planes, box_warp, ray_w=0, rows_per_ray=0, amax=None):
    """d_planes (channels_last [N,3C,Hp,Wp], i.e. [N,Hp,Wp,ldp] in memory) += the bilinear-adjoint scatter of the gradient rows [S,32] at the positions
    pos [S,4] (x, y, z, -; x = NaN marks an absent row, whose gradient row is never read); image n owns rows n S/N .. (n+1) S/N - 1.
    ray_w, rows_per_ray: the optional brick-walk hint of the binning passes.  amax: [1] tensor holding max|rows| selects the accumulation
    on the 16-bit matrix cores, None the exact fp32 products (eg3d_triplane_scatter, include/eg3d_hip.h)."""
    assert is_cl(d_planes) and d_planes.dtype == torch.float32
    n, ldp, hp, wp = d_planes.shape
    S = pos.numel() // 4
    assert rows.numel() == S * 32 and S % n == 0
    nints = L.lib().eg3d_triplane_scatter_workspace_ints(S, n, hp, wp)
    ws = torch.empty(nints, dtype=torch.int32, device=d_planes.device)
    L.check(L.lib().eg3d_triplane_scatter(L.ptr(rows), L.ptr(pos), S, S // n, L.ptr(d_planes), n, hp, wp, ldp, float(box_warp), L.ptr(ws),
                                          int(ray_w), int(rows_per_ray), L.ptr(amax) if amax is not None else None, L.stream_ptr()),
            'triplane_scatter')


def sample_decode(p, coords, M):
    n = p.N
    rgb = torch.empty((n, M, p.Cout), dtype=torch.float32, device=coords.device)
    sigma = torch.empty((n, M, 1), dtype=torch.float32, device=coords.device)
    L.check(L.lib().eg3d_sample_decode(C.byref(p), L.ptr(coords), M, L.ptr(rgb), L.ptr(sigma), L.stream_ptr()), 'sample_decode')
    return rgb, sigma


# ------------------------------------------------------------------------------------------------- noise buffers
def _buf_arrays(bufs):
    n = len(bufs)
    xs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
    res = (C.c_int32 * n)(*[int(b.shape[-1]) for b in bufs])
    return n, xs, res


NOISE_BANK_MAX = 32          # buffers per launch of the noise kernels (include/eg3d_hip.h)


def noise_regularizer(bufs, scale=1.0, want_grad=True, grads=None):
    """Returns (reg [0-d tensor] = scale * regulariser summed over all buffers, grads list or None) for square fp32 noise buffers;
    one launch per 32 buffers (a batch of images brings 17 per image).  `grads`: optional pre-allocated gradient tensors (views allowed)."""
    for b in bufs:
        L.require_cuda(b)
        assert b.dim() == 2 and b.shape[0] == b.shape[1] and b.is_contiguous() and b.dtype == torch.float32
    dev = bufs[0].device
    if want_grad and grads is None:
        grads = [torch.empty_like(b) for b in bufs]
    total = None
    for lo in range(0, len(bufs), NOISE_BANK_MAX):
        part = bufs[lo:lo + NOISE_BANK_MAX]
        n, xs, res = _buf_arrays(part)
        gs = (C.c_void_p * n)(*[g.data_ptr() for g in grads[lo:lo + NOISE_BANK_MAX]]) if want_grad else (C.c_void_p * n)()
        ws = torch.empty(int(L.lib().eg3d_noise_reg_workspace_floats(res, n)), dtype=torch.float32, device=dev)
        reg = torch.empty((), dtype=torch.float32, device=dev)
        L.check(L.lib().eg3d_noise_regularizer(xs, gs, res, n, L.ptr(ws), L.ptr(reg), float(scale), L.stream_ptr()), 'noise_regularizer')
        total = reg if total is None else total + reg
    return total, (grads if want_grad else None)



class PendingEpilogue:
    """A 3 x 3 layer's finishing epilogue that has not run yet: the layer's output tensor is allocated but still unwritten, `z` holds the split-K
    sums.  The toRGB launch that consumes the output next runs it (torgb_small(pre=...)); anything else calls run() first."""
    __slots__ = ('z', 'out', 'd', 'noise', 'noise_nstride', 'noise_strength', 'bias', 'act', 'alpha', 'gain', 'clamp', 'out_amax')

    def __init__(self, z, out, d, out_amax, noise=None, noise_nstride=0, noise_strength=None, bias=None, act='linear', alpha=0.0, gain=1.0, clamp=-1.0):
        self.z, self.out, self.d, self.out_amax = z, out, d, out_amax
        self.noise, self.noise_nstride, self.noise_strength, self.bias = noise, noise_nstride, noise_strength, bias
        self.act, self.alpha, self.gain, self.clamp = act, alpha, gain, clamp

    def run(self):
        epilogue_fwd(self.z, self.out, d=self.d, out_amax=self.out_amax, noise=self.noise, noise_nstride=self.noise_nstride, noise_strength=self.noise_strength,
                     bias=self.bias, act=self.act, alpha=self.alpha, gain=self.gain, clamp=self.clamp)


# conv1's finishing pass inside the toRGB launch of the 4^2 .. 64^2 blocks (eg3d_torgb_small_params::pre_z): five launches fewer per step.  The first
# version was NOT faster (merged launch 17.9 - 18.9 us against 10.0 - 10.9 + 5.5 - 9.1 for the two): its d / bias loads sat under (uniform) null-pointer
# branches inside the unrolled batch, and a load under a branch is a memory round trip of its own -- sixteen in sequence per batch.  Issued with the
# operand loads (dummy address when absent) the merged launch is 14.2 - 15.3 us and the step +0.5 % (220.1 vs 219.0 steps/s, A/B).  EG3D_DEFER_EPILOGUE=0: separate pass.
DEFER_EPILOGUE = os.environ.get('EG3D_DEFER_EPILOGUE', '1') != '0'
# the mirror image in the backward pass: conv0's split-K data gradient goes to the previous block's toRGB node unfinished (fused.PENDING_DGRAD) and that
# node's launch applies the styles and accumulates the style gradient (eg3d_torgb_small_bwd_params::add_scale): the dgrad_finish launch of the 8^2 .. 64^2 blocks is gone
DEFER_DGRAD_FINISH = os.environ.get('EG3D_DEFER_DGRAD_FINISH', '1') != '0'

TORGB_SMALL = os.environ.get('EG3D_TORGB_SMALL', '1') != '0'            # low-latency toRGB launch for small pixel counts (csrc/torgb_small.hip)
TORGB_SMALL_MAX_PIX = 4096
# (the data gradient at 64^2 takes 31 us in the trace against 27 for the implicit GEMM it replaced -- yet the step is 0.2 % faster with it: A/B 209.1 vs 208.8)
TORGB_SMALL_BWD_MAX_PIX = 4096
# the streaming form of the same entry points for the 128^2 / 256^2 blocks (torgb_mid_kernel / torgb_mid_bwd_kernel, csrc/torgb_small.hip): beyond
# TORGB_SMALL_*_MAX_PIX the launch is taken only when the library says it runs in that form (eg3d_torgb_mid_supported); EG3D_TORGB_MID=0: implicit GEMM as before
TORGB_MID = os.environ.get('EG3D_TORGB_MID', '1') != '0'
TORGB_MID_BWD = os.environ.get('EG3D_TORGB_MID_BWD', '1') != '0'


def torgb_small(x, wf, styles, out, bias=None, clamp=-1.0, addend=None, addend_up2_taps=None, pre=None):
    """eg3d_torgb_small_fwd: out = clamp(conv1x1(x * styles, wf) + bias) + addend.  x / out / addend channels_last fp32; wf [Cp, C] packed rows.
    `pre` (a PendingEpilogue): x does not exist yet -- the launch runs the producing layer's finishing epilogue on its split-K sums and WRITES x.
    Returns False (nothing launched) when the geometry is not the kernel's."""
    assert is_cl(x) and is_cl(out)
    n, c, h, w = x.shape
    p = L.TorgbSmallParams(x=x.data_ptr(), w=wf.data_ptr(), s=styles.data_ptr(), bias=bias.data_ptr() if bias is not None else None,
                           addend=addend.data_ptr() if addend is not None else None, out=out.data_ptr(), N=n, H=h, W=w, C=c, Cp=out.shape[1],
                           ldx=c, ldo=out.shape[1], w_row=wf.stride(0), addend_up2=1 if addend_up2_taps is not None else 0, clamp=float(clamp))
    if addend_up2_taps is not None:
        p.addend_taps[:] = [float(t) for t in addend_up2_taps]
    if pre is not None:
        if pre.act not in ('linear', 'lrelu', 'relu') or tuple(pre.z.shape) != tuple(x.shape) or not is_cl(pre.z):
            return False
        p.pre_z, p.pre_d, p.pre_bias = pre.z.data_ptr(), L.ptr(pre.d), L.ptr(pre.bias)
        p.pre_noise, p.pre_strength, p.pre_noise_nstride = L.ptr(pre.noise), L.ptr(pre.noise_strength), int(pre.noise_nstride or 0)
        p.x_amax = L.ptr(pre.out_amax)
        p.pre_slope = {'linear': 1.0, 'lrelu': float(pre.alpha), 'relu': 0.0}[pre.act]
        p.pre_gain, p.pre_clamp = float(pre.gain), float(pre.clamp)
    if not L.lib().eg3d_torgb_small_supported(C.byref(p)):
        return False
    if n * h * w > TORGB_SMALL_MAX_PIX and not (TORGB_MID and L.lib().eg3d_torgb_mid_supported(C.byref(p))):
        return False
    L.check(L.lib().eg3d_torgb_small_fwd(C.byref(p), L.stream_ptr()), 'torgb_small_fwd')
    return True


def torgb_small_bwd(dy, wa, styles, x, dx, ds=None, addend=None, act_bwd=None, out_amax=None, addend_scale=None, addend_ds=None):
    """eg3d_torgb_small_bwd: the toRGB data gradient for small pixel counts (+ the producing layer's activation backward when act_bwd is an
    ActBwdSpec the kernel takes).  Returns None when nothing was launched (geometry not the kernel's), else True / False = the activation
    backward was / was not fused (as conv_igemm)."""
    assert is_cl(dy) and is_cl(x) and is_cl(dx)
    n, c, h, w = x.shape
    p = L.TorgbSmallBwdParams(dy=dy.data_ptr(), wa=wa.data_ptr(), s=styles.data_ptr(), xin=x.data_ptr(), addend=addend.data_ptr() if addend is not None else None,
                              dx=dx.data_ptr(), ds=ds.data_ptr() if ds is not None else None, out_amax=out_amax.data_ptr() if out_amax is not None else None,
                              N=n, H=h, W=w, C=c, Cp=dy.shape[1], ldg=dy.shape[1], ldx=c, wa_row=wa.stride(0), act_on=0,
                              no_mid=0 if TORGB_MID_BWD else 1)          # (the library picks the streaming form itself from 4096 pixels: the switch must reach it)
    if addend_scale is not None:          # the addend is an unfinished split-K data gradient: finish it in this launch (PendingDgrad)
        p.add_scale = addend_scale.data_ptr()
    if addend_ds is not None:             # (without addend_scale the library refuses the launch: an addend_ds dropped here would silently stay unaccumulated)
        p.add_ds = addend_ds.data_ptr()
    fused = False
    if act_bwd is not None:
        p.act_on = 1
        act_bwd.fill(p.act_bwd)
        fused = bool(L.lib().eg3d_torgb_small_bwd_supported(C.byref(p)))
        if not fused:
            p.act_on = 0
            p.act_bwd = L.ActBwd()
            p.out_amax = None
    if not fused and not L.lib().eg3d_torgb_small_bwd_supported(C.byref(p)):
        return None
    if n * h * w > TORGB_SMALL_BWD_MAX_PIX and not (TORGB_MID_BWD and L.lib().eg3d_torgb_mid_bwd_supported(C.byref(p))):
        return None
    L.check(L.lib().eg3d_torgb_small_bwd(C.byref(p), L.stream_ptr()), 'torgb_small_bwd')
    return fused


def conv_atomic(x, wp, Ck, Nc, out, classes, in_stride=1, out_stride=1, in_scale=None, ksplit=1, **igemm_kw):
    """A split (EPI_ATOMIC) launch of the implicit GEMM with `ksplit` slices into the pre-zeroed `out`."""
    conv_igemm(x, wp, Ck, Nc, out, classes, in_stride=in_stride, out_stride=out_stride, in_scale=in_scale, epi=L.EPI_ATOMIC, ksplit=ksplit, **igemm_kw)


class HipAdam:
    """torch.optim.Adam(params, lr, betas, eps) for fp32 leaves in one launch per 32 leaves (`eg3d_adam_step`), with two extras the latent
    projector's step wants folded in: a second gradient per leaf (the noise regulariser's, which does not go through autograd) and the
    renormalisation of the noise maps after the update (w_projector.py:264-270).  The learning rate and the step count are device scalars, so
    a captured step can be replayed for every step index.  Same surface as the torch optimiser where the projector touches it
    (`param_groups[0]['lr']` -- a float or a device scalar --, `zero_grad`, `step`, `state`)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        dev = self.params[0].device
        self._lr_t = lr if torch.is_tensor(lr) else torch.tensor(float(lr), device=dev)
        self._lr_host = None if torch.is_tensor(lr) else float(lr)
        self.param_groups = [dict(params=self.params, lr=lr, betas=betas, eps=eps)]
        self.step_t = torch.zeros((), device=dev)
        self.state = {p: dict(exp_avg=torch.zeros_like(p, memory_format=torch.contiguous_format),
                              exp_avg_sq=torch.zeros_like(p, memory_format=torch.contiguous_format), step=self.step_t) for p in self.params}
        for p in self.params:
            assert p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def step(self, extra_grads=None, normalize=None, skip=None):
        """extra_grads: {param: tensor} added to the gradient; normalize: {param: number of equal slices renormalised separately} (a noise
        map [N,1,r,r] of N independent images: N); skip: device scalar, != 0 -> this step changes nothing (eg3d_adam_list::skip)."""
        g = self.param_groups[0]
        lr = g['lr']
        if torch.is_tensor(lr):
            self._lr_t = lr
        elif getattr(self, '_lr_host', None) != float(lr):          # (a fill launch per step only when the host value changed)
            self._lr_t.fill_(float(lr))
            self._lr_host = float(lr)
        items = []
        for p in self.params:
            e = extra_grads.get(p) if extra_grads else None
            if p.grad is None and e is None:
                continue
            gr = p.grad
            assert gr is None or (gr.dtype == torch.float32 and gr.is_contiguous()), 'HipAdam: fp32 contiguous gradients'
            assert e is None or (e.dtype == torch.float32 and e.is_contiguous() and e.shape == p.shape)
            st = self.state[p]
            k = int(normalize.get(p, 0)) if normalize else 0
            parts = max(k, 1)
            n = p.numel() // parts
            assert n * parts == p.numel()
            for i in range(parts):
                o = 4 * n * i
                items.append((p.data_ptr() + o, gr.data_ptr() + o if gr is not None else None, e.data_ptr() + o if e is not None else None,
                              st['exp_avg'].data_ptr() + o, st['exp_avg_sq'].data_ptr() + o, n, 1 if k else 0))
        dev = self.params[0].device
        # the kernel writes through raw pointers: tell autograd / memo() that the leaves changed (no launch involved)
        touched = [p for p in self.params if p.grad is not None or (extra_grads and extra_grads.get(p) is not None)]
        bump = getattr(torch._C._autograd, '_unsafe_set_version_counter', None)
        if bump is not None and touched:
            bump(touched, [p._version + 1 for p in touched])
        else:
            weights_changed()
        for lo in range(0, len(items), L.ADAM_ITEMS_MAX):
            bank = items[lo:lo + L.ADAM_ITEMS_MAX]
            a = L.AdamList(n=len(bank), bump_step=int(lo + L.ADAM_ITEMS_MAX >= len(items)), beta1=g['betas'][0], beta2=g['betas'][1], eps=g['eps'],
                           lr=self._lr_t.data_ptr(), step=self.step_t.data_ptr(), skip=skip.data_ptr() if skip is not None else None)
            for j, it in enumerate(bank):
                a.items[j] = L.AdamItem(*it)
            ws = zeros((2 * len(bank) + 1,), dev)
            L.check(L.lib().eg3d_adam_step(C.byref(a), L.ptr(ws), L.stream_ptr()), 'adam_step')


def early_stop_flag(value, threshold, done):
    """done <- 1 where value <= threshold (sticky device flag; eg3d_early_stop_flag)."""
    L.check(L.lib().eg3d_early_stop_flag(L.ptr(value), float(threshold), L.ptr(done), L.stream_ptr()), 'early_stop_flag')
    return done


def noise_normalize_(bufs):
    for lo in range(0, len(bufs), NOISE_BANK_MAX):
        n, xs, res = _buf_arrays(bufs[lo:lo + NOISE_BANK_MAX])
        ws = zeros((2 * n,), bufs[0].device)          # per-buffer (sum, sum of squares): multi-block path
        L.check(L.lib().eg3d_noise_normalize(xs, res, n, L.ptr(ws), L.stream_ptr()), 'noise_normalize')


_INT32_MAX = 2 ** 31 - 1


def _grid3(vol: torch.Tensor, what: str) -> torch.Tensor:
    """vol checked as a 3-D fp32 grid on the GPU: the contiguous grid."""
    L.require_cuda(vol)
    if vol.dim() != 3 or vol.dtype != torch.float32:
        raise L.Eg3dHipError(f'{what}: a 3-D fp32 grid, got {tuple(vol.shape)} {vol.dtype}')
    return vol.contiguous()


def _cams25(cams: torch.Tensor, what: str, dev) -> torch.Tensor:
    """cams checked as camera vectors [F >= 1, 25] on a GPU: contiguous fp32 on dev."""
    L.require_cuda(cams)
    if cams.dim() != 2 or cams.shape[1] != 25 or cams.shape[0] < 1:
        raise L.Eg3dHipError(f'{what}: cameras [F >= 1, 25], got {tuple(cams.shape)}')
    return cams.to(device=dev, dtype=torch.float32).contiguous()


def _fill_frame(p, origin, spacing, axes):
    """The world-to-grid frame of a params struct that has one (IsoParams, MeshNormalsParams)."""
    p.axes[:] = [int(v) for v in axes]
    p.origin[:] = [float(v) for v in origin]
    p.spacing[:] = [float(v) for v in spacing]


def marching_cubes(vol: torch.Tensor, level: float, origin=None, spacing=None):
    """(verts fp32 [V,3], faces int32 [F,3]) of the level-`level` surface of the fp32 grid vol [D0,D1,D2] (eg3d_mc_*; include/eg3d_hip.h):
    the frame of skimage's marching_cubes(vol.transpose(2,1,0), level) (grid point (i0,i1,i2) -> (i2,i1,i0)), then * spacing + origin per
    output axis.  Inside = v > level; the faces' right-hand normals point toward lower values.  Finite values assumed.  Workspace from
    the caching allocator; one host synchronise (the totals)."""
    vol = _grid3(vol, 'marching_cubes')
    dev = vol.device
    p = L.McParams(vol=vol.data_ptr(), D0=vol.shape[0], D1=vol.shape[1], D2=vol.shape[2], level=float(level))
    p.origin[:] = [float(v) for v in (origin if origin is not None else (0.0, 0.0, 0.0))]
    p.spacing[:] = [float(v) for v in (spacing if spacing is not None else (1.0, 1.0, 1.0))]
    lib = L.lib()
    count_bytes, per_active = C.c_int64(0), C.c_int64(0)
    L.check(lib.eg3d_mc_query_workspace(C.byref(p), C.byref(count_bytes), C.byref(per_active)), 'mc_query_workspace')
    ws = torch.empty(count_bytes.value, dtype=torch.uint8, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    p.workspace, p.workspace_bytes, p.totals = ws.data_ptr(), count_bytes.value, totals.data_ptr()
    L.check(lib.eg3d_mc_count(C.byref(p), L.stream_ptr()), 'mc_count')
    A, V, F, _ = totals.tolist()
    if max(A, V, F) > _INT32_MAX:
        L.check(-3, f'marching_cubes ({A} active points, {V} vertices, {F} faces)')
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    if A == 0:
        return verts, faces
    emit = torch.empty(A * per_active.value, dtype=torch.uint8, device=dev)
    p.emit_workspace, p.emit_workspace_bytes = emit.data_ptr(), emit.numel()
    p.verts, p.vert_capacity, p.faces, p.face_capacity = verts.data_ptr(), V, faces.data_ptr(), F
    L.check(lib.eg3d_mc_emit(C.byref(p), L.stream_ptr()), 'mc_emit')
    return verts, faces


def _iso_grid_params(vol: torch.Tensor, what: str):
    vol = _grid3(vol, what)
    return vol, L.IsoParams(vol=vol.data_ptr(), D0=vol.shape[0], D1=vol.shape[1], D2=vol.shape[2])


def iso_bricks_shape(shape):
    """Bricks per axis of a grid of `shape`: ceil((D - 1) / 8)."""
    return tuple((int(d) + L.ISO_BRICK - 2) // L.ISO_BRICK for d in shape)


def iso_bricks(vol: torch.Tensor) -> torch.Tensor:
    """fp32 [B0,B1,B2], B = ceil((D - 1) / 8): per 8x8x8-cell brick of the fp32 grid vol [D0,D1,D2] the maximum over the brick's corner range
    dilated by one voxel on every side (NaN ignored) -- what iso_render's empty-space skipping reads.  It does not depend on the level: one
    pass per grid serves every level and every frame (eg3d_iso_bricks; include/eg3d_hip.h "Shape views").  One launch."""
    vol, p = _iso_grid_params(vol, 'iso_bricks')
    out = torch.empty(iso_bricks_shape(vol.shape), dtype=torch.float32, device=vol.device)
    p.bricks = out.data_ptr()
    L.check(L.lib().eg3d_iso_bricks(C.byref(p), L.stream_ptr()), 'iso_bricks')
    return out


ISO_SHADE_MODES = dict(lambert=L.ISO_LAMBERT, normal=L.ISO_NORMAL)


def iso_render(vol: torch.Tensor, cams: torch.Tensor, res: int, level: float, origin, spacing, axes=(0, 1, 2), step: float = 0.5, refine: int = 4,
               bricks: Optional[torch.Tensor] = None, skip: bool = True, shade: str = 'lambert', ambient: float = 0.15, background: float = 1.0,
               want_hit_k: bool = False) -> dict:
    """First-hit views of the surface {vol = level} of the fp32 grid vol [D0,D1,D2] from the cameras cams [F,25] (cam2world 16 + intrinsics 9,
    the generator's conditioning vectors) at res x res pixels; the rays are RaySampler's, so the frames register with G.synthesis's images
    (eg3d_iso_render; the algorithm is specified operation by operation in include/eg3d_hip.h "Shape views").  Grid index i of grid axis a sits
    at world coordinate origin[a] + i * spacing[a] of world axis axes[a]; spacing may be negative.  Inside = v > level; NaN never hits.
    Samples every step * min|spacing| along the ray, trilinear field, `refine` bisections and one secant step at the first crossing.
    Returns a dict:
      depth  fp32 [F,res,res]     distance along the unit ray in world units (what image_depth measures), 0 on a miss
      normal fp32 [F,res,res,3]   world-space unit normal toward lower values, 0 on a miss or where the gradient vanishes
      mask   uint8 [F,res,res]
      shade  fp32 [F,3,res,res]   in [-1,1], ready for jpeg_encode / image_grid_u8 (which show x * 127.5 + 128):
                                  'lambert': grey v * 2 - 1 with v = ambient + (1 - ambient) * max(0, n . -d) in [0,1] (a headlight);
                                  'normal':  colour * 2 - 1 with colour = camera-space normal * 0.5 + 0.5 in [0,1];
                                  a miss takes `background`, which is already in [-1,1] (1.0 = white)
      hit_k  int32 [F,res,res]    with want_hit_k: index of the hit sample, -1 on a miss
      bricks                      the brick maxima used (pass them back in for the next call on the same grid)
    skip=True jumps over bricks whose maximum is <= level; the outputs are bit-identical either way.  One launch (two when it has to build the
    bricks), no host synchronise."""
    vol, p = _iso_grid_params(vol, 'iso_render')
    cams = _cams25(cams, 'iso_render', vol.device)
    if shade not in ISO_SHADE_MODES:
        raise L.Eg3dHipError(f'iso_render: shade {sorted(ISO_SHADE_MODES)}, got {shade!r}')
    dev, F, res = vol.device, cams.shape[0], int(res)
    if skip:
        if bricks is None:
            bricks = iso_bricks(vol)
        L.require_cuda(bricks)
        if tuple(bricks.shape) != iso_bricks_shape(vol.shape) or bricks.dtype != torch.float32 or not bricks.is_contiguous():
            raise L.Eg3dHipError(f'iso_render: bricks must be contiguous fp32 {iso_bricks_shape(vol.shape)}, got {tuple(bricks.shape)} {bricks.dtype}')
    if res < 1:
        raise L.Eg3dHipError(f'iso_render: res >= 1, got {res}')
    out = dict(depth=torch.empty((F, res, res), dtype=torch.float32, device=dev), normal=torch.empty((F, res, res, 3), dtype=torch.float32, device=dev),
               mask=torch.empty((F, res, res), dtype=torch.uint8, device=dev), shade=torch.empty((F, 3, res, res), dtype=torch.float32, device=dev))
    if want_hit_k:
        out['hit_k'] = torch.empty((F, res, res), dtype=torch.int32, device=dev)
        p.hit_k = out['hit_k'].data_ptr()
    p.cams, p.bricks = cams.data_ptr(), (bricks.data_ptr() if skip else None)
    p.depth, p.normal, p.mask, p.shade = out['depth'].data_ptr(), out['normal'].data_ptr(), out['mask'].data_ptr(), out['shade'].data_ptr()
    p.F, p.res = F, res
    _fill_frame(p, origin, spacing, axes)
    p.level, p.step, p.refine, p.skip = float(level), float(step), int(refine), int(bool(skip))
    p.shade_mode, p.ambient, p.background = ISO_SHADE_MODES[shade], float(ambient), float(background)
    L.check(L.lib().eg3d_iso_render(C.byref(p), L.stream_ptr()), 'iso_render')
    out['bricks'] = bricks
    return out


def _mesh_rows(t: torch.Tensor, what: str, dev=None, rows=None) -> torch.Tensor:
    L.require_cuda(t)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or not t.is_contiguous() or (rows is not None and t.shape[0] != rows):
        raise L.Eg3dHipError(f'{what} must be contiguous fp32 [{"V" if rows is None else rows}, 3], got {tuple(t.shape)} {t.dtype}')
    if dev is not None and t.device != dev:
        raise L.Eg3dHipError(f'{what} is on {t.device}, expected {dev}')
    return t


def mesh_normals(vol: torch.Tensor, points: torch.Tensor, origin, spacing, axes=(0, 1, 2)) -> torch.Tensor:
    """fp32 [V,3]: the unit normal of the trilinear field of the fp32 grid vol [D0,D1,D2] at the world points [V,3], toward lower values (out of
    the dense region): clamped +-1 voxel differences of iso_render's field, its 'normal at the hit' at arbitrary points (eg3d_mesh_normals;
    include/eg3d_hip.h "Mesh attributes").  The frame (origin, spacing, axes) is iso_render's.  0 where the gradient vanishes or is not finite
    and for a NaN point.  One launch, no host synchronise."""
    vol = _grid3(vol, 'mesh_normals')
    points = _mesh_rows(points, 'mesh_normals: points', vol.device)
    out = torch.empty_like(points)
    p = L.MeshNormalsParams(vol=vol.data_ptr(), points=points.data_ptr(), normals=out.data_ptr(), V=points.shape[0], D0=vol.shape[0], D1=vol.shape[1],
                            D2=vol.shape[2])
    _fill_frame(p, origin, spacing, axes)
    L.check(L.lib().eg3d_mesh_normals(C.byref(p), L.stream_ptr()), 'mesh_normals')
    return out


def _bake_views(what: str, images, depth, mask, cams, dev):
    """The views of mesh_bake / mesh_texture checked: (F, cams as contiguous fp32)."""
    L.require_cuda(images, depth, mask)
    cams = _cams25(cams, what, dev)
    F = cams.shape[0]
    if images.dim() != 4 or images.shape[0] != F or images.shape[1] != 3 or images.shape[2] != images.shape[3] or images.shape[2] < 1 \
            or images.dtype != torch.float32 or not images.is_contiguous():
        raise L.Eg3dHipError(f'{what}: images must be contiguous fp32 [{F}, 3, H, H], got {tuple(images.shape)} {images.dtype}')
    if depth.dim() != 3 or depth.shape[0] != F or depth.shape[1] != depth.shape[2] or depth.shape[1] < 1 or depth.dtype != torch.float32 \
            or not depth.is_contiguous():
        raise L.Eg3dHipError(f'{what}: depth must be contiguous fp32 [{F}, R, R], got {tuple(depth.shape)} {depth.dtype}')
    if tuple(mask.shape) != tuple(depth.shape) or mask.dtype != torch.uint8 or not mask.is_contiguous():
        raise L.Eg3dHipError(f'{what}: mask must be contiguous uint8 {tuple(depth.shape)}, got {tuple(mask.shape)} {mask.dtype}')
    for name, t in (('images', images), ('depth', depth), ('mask', mask)):
        if t.device != dev:
            raise L.Eg3dHipError(f'{what}: {name} is on {t.device}, expected {dev}')
    return F, cams


def mesh_bake(points: torch.Tensor, normals: torch.Tensor, images: torch.Tensor, depth: torch.Tensor, mask: torch.Tensor, cams: torch.Tensor,
              fallback: Optional[torch.Tensor] = None, depth_tol: float = 0.0, cos_min: float = 0.1, power: int = 2) -> dict:
    """Vertex colours from rendered views (eg3d_mesh_bake; specified operation by operation in include/eg3d_hip.h "Mesh attributes").
    points, normals fp32 [V,3] in world coordinates; images fp32 [F,3,H,H] in [-1,1], the renders of cams [F,25]; depth fp32 [F,R,R] and mask
    uint8 [F,R,R] as iso_render gives them for the same cameras.  A vertex takes colour from a view when it projects inside the frame, lies no
    further than depth + depth_tol (world units) behind the first hit of one of the four depth pixels around it, and faces the camera with
    cosine c > cos_min; the views' bilinear samples are blended with weights c ** power (power 1..8).  A vertex no view sees takes
    `fallback` [V,3] (0 without one).  Returns a dict:
      color  fp32 [V,3]   in [-1,1]
      rgb    uint8 [V,3]  color * 127.5 + 128, clamped and truncated as image_grid_u8 does
      weight fp32 [V]     the sum of the weights
      views  uint8 [V]    how many views contributed
    One launch, no host synchronise."""
    points = _mesh_rows(points, 'mesh_bake: points')
    dev, V = points.device, points.shape[0]
    normals = _mesh_rows(normals, 'mesh_bake: normals', dev, V)
    F, cams = _bake_views('mesh_bake', images, depth, mask, cams, dev)
    if fallback is not None:
        fallback = _mesh_rows(fallback, 'mesh_bake: fallback', dev, V)
    out = dict(color=torch.empty((V, 3), dtype=torch.float32, device=dev), rgb=torch.empty((V, 3), dtype=torch.uint8, device=dev),
               weight=torch.empty((V,), dtype=torch.float32, device=dev), views=torch.empty((V,), dtype=torch.uint8, device=dev))
    p = L.MeshBakeParams(points=points.data_ptr(), normals=normals.data_ptr(), cams=cams.data_ptr(), images=images.data_ptr(), depth=depth.data_ptr(),
                         mask=mask.data_ptr(), fallback=None if fallback is None else fallback.data_ptr(), color=out['color'].data_ptr(),
                         rgb=out['rgb'].data_ptr(), weight=out['weight'].data_ptr(), views=out['views'].data_ptr(), V=V, F=F, H=images.shape[2],
                         R=depth.shape[1], depth_tol=float(depth_tol), cos_min=float(cos_min), power=int(power))
    L.check(L.lib().eg3d_mesh_bake(C.byref(p), L.stream_ptr()), 'mesh_bake')
    return out


def mesh_texture(points: torch.Tensor, normals: torch.Tensor, faces: torch.Tensor, images: torch.Tensor, depth: torch.Tensor, mask: torch.Tensor,
                 cams: torch.Tensor, fallback: Optional[torch.Tensor] = None, tile: int = 8, fill: int = 128, depth_tol: float = 0.0,
                 cos_min: float = 0.1, power: int = 2) -> dict:
    """A texture atlas for the mesh (points, normals fp32 [V,3] in world coordinates, faces int32 [F,3]) baked from the rendered views
    (eg3d_mesh_texture; specified operation by operation in include/eg3d_hip.h "Mesh texture").  Two faces share a tile x tile block of the
    atlas, one per triangle of its diagonal, the corner opposite a face's longest edge at the right angle; every texel interpolates its
    face's vertices and goes through mesh_bake's view loop (images, depth, mask, cams, depth_tol, cos_min, power as there; `fallback` [V,3]
    is interpolated too).  A bilinear lookup inside a face's uv triangle reads only that face's texels.  Returns a dict:
      texture uint8 [Ht,Wt,3]  (Ht, Wt) = mesh_texture_size(F, tile); texels no face owns hold `fill`
      views   uint8 [Ht,Wt]    how many views coloured the texel (0: fallback or fill)
      uv      fp32 [F,3,2]     per face corner, in the faces' own corner order: (u, v) in [0,1] with the origin at the top-left texel
      corner  uint8 [F]        the face corner that took the right angle
    The bytes are a function of the inputs alone.  A face index outside [0, V) raises (no such vertex is read).  One launch besides the
    counter's; one host synchronise (the counter)."""
    points = _mesh_rows(points, 'mesh_texture: points')
    dev, V = points.device, points.shape[0]
    normals = _mesh_rows(normals, 'mesh_texture: normals', dev, V)
    faces = _mesh_faces(faces, 'mesh_texture: faces', dev)
    N, cams = _bake_views('mesh_texture', images, depth, mask, cams, dev)
    if fallback is not None:
        fallback = _mesh_rows(fallback, 'mesh_texture: fallback', dev, V)
    if not 4 <= int(tile) <= 64 or not 0 <= int(fill) <= 255:
        raise L.Eg3dHipError(f'mesh_texture: tile in [4, 64] and fill in [0, 255], got tile = {tile!r}, fill = {fill!r}')
    F = faces.shape[0]
    Ht, Wt = mesh_texture_size(F, tile)
    out = dict(texture=torch.empty((Ht, Wt, 3), dtype=torch.uint8, device=dev), views=torch.empty((Ht, Wt), dtype=torch.uint8, device=dev),
               uv=torch.empty((F, 3, 2), dtype=torch.float32, device=dev), corner=torch.empty((F,), dtype=torch.uint8, device=dev))
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    p = L.MeshTextureParams(points=points.data_ptr(), normals=normals.data_ptr(), faces=faces.data_ptr(), cams=cams.data_ptr(),
                            images=images.data_ptr(), depth=depth.data_ptr(), mask=mask.data_ptr(),
                            fallback=None if fallback is None else fallback.data_ptr(), texture=out['texture'].data_ptr(),
                            views=out['views'].data_ptr(), uv=out['uv'].data_ptr(), corner=out['corner'].data_ptr(), bad_faces=bad.data_ptr(),
                            V=V, F=F, N=N, H=images.shape[2], R=depth.shape[1], tile=int(tile), fill=int(fill), depth_tol=float(depth_tol),
                            cos_min=float(cos_min), power=int(power))
    L.check(L.lib().eg3d_mesh_texture(C.byref(p), L.stream_ptr()), 'mesh_texture')
    n_bad = int(bad.item())
    if n_bad:
        raise L.Eg3dHipError(f'mesh_texture: {n_bad} face(s) with an index outside [0, {V})')
    return out


RASTER_MODES = dict(texture=L.RASTER_TEXTURE, vertex=L.RASTER_VERTEX, lambert=L.RASTER_LAMBERT)
RASTER_CULL = dict(none=0, back=1)


def mesh_raster(points: torch.Tensor, faces: torch.Tensor, cams: torch.Tensor, res: int, mode: str = 'texture', uv: Optional[torch.Tensor] = None,
                texture: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                cull: str = 'back', near: float = 0.1, background: float = 1.0, ambient: float = 0.2) -> dict:
    """Views of the mesh (points fp32 [V,3] in world coordinates, faces int32 [F,3]) from the cameras cams [N,25] at res x res pixels, through
    a z-buffer (eg3d_mesh_raster; specified operation by operation in include/eg3d_hip.h "Mesh previews").  The pixels are iso_render's and
    G.synthesis's: pixel (y, x) looks along the same ray.  Perspective-correct interpolation; nothing is clipped: a face with a vertex no further
    than `near` in front of the camera plane is dropped.  cull='back' drops faces whose right-hand normal points away from the camera.
      mode='texture'  uv fp32 [F,3,2] and texture uint8 [Ht,Wt,3] as mesh_texture returns them: a bilinear fetch at the interpolated uv
      mode='vertex'   colors fp32 [V,3] in [-1,1] (mesh_bake's 'color'), interpolated
      mode='lambert'  normals fp32 [V,3] (mesh_normals), interpolated and normalised: grey v * 2 - 1, v = ambient + (1 - ambient) * max(0, n . -d)
    Returns a dict:
      image fp32 [N,3,res,res]  in [-1,1]; a miss takes `background`
      face  int32 [N,res,res]   the face seen, -1 on a miss
      z     fp32 [N,res,res]    camera-space depth, 0 on a miss
      depth fp32 [N,res,res]    distance along the unit ray (iso_render's depth), 0 on a miss
      mask  uint8 [N,res,res]
      bary  fp32 [N,res,res,3]  perspective-correct barycentrics of the face's corners
      small_faces, large_faces  ints: (view, face) pairs drawn one per lane, and by a whole workgroup (more than 8 pixels wide or high)
    The bytes are a function of the inputs alone.  A face index outside [0, V) raises (no such vertex is read).  Five launches; one host
    synchronise (the counters)."""
    points = _mesh_rows(points, 'mesh_raster: points')
    dev, V = points.device, points.shape[0]
    faces = _mesh_faces(faces, 'mesh_raster: faces', dev)
    F, res = faces.shape[0], int(res)
    cams = _cams25(cams, 'mesh_raster', dev)
    N = cams.shape[0]
    if mode not in RASTER_MODES or cull not in RASTER_CULL:
        raise L.Eg3dHipError(f'mesh_raster: mode {sorted(RASTER_MODES)} and cull {sorted(RASTER_CULL)}, got {mode!r}, {cull!r}')
    if res < 1 or not float(near) > 0.0 or not 0.0 <= float(ambient) <= 1.0:
        raise L.Eg3dHipError(f'mesh_raster: res >= 1, near > 0 and ambient in [0, 1], got {res}, {near!r}, {ambient!r}')
    p = L.MeshRasterParams(points=points.data_ptr(), faces=faces.data_ptr(), cams=cams.data_ptr(), V=V, F=F, N=N, res=res, mode=RASTER_MODES[mode],
                           cull=RASTER_CULL[cull], near=float(near), background=float(background), ambient=float(ambient))
    if mode == 'texture':
        if uv is None or texture is None:
            raise L.Eg3dHipError("mesh_raster: mode='texture' needs uv and texture")
        L.require_cuda(uv, texture)
        if tuple(uv.shape) != (F, 3, 2) or uv.dtype != torch.float32 or not uv.is_contiguous() or uv.device != dev:
            raise L.Eg3dHipError(f'mesh_raster: uv must be contiguous fp32 [{F}, 3, 2] on {dev}, got {tuple(uv.shape)} {uv.dtype} on {uv.device}')
        if texture.dim() != 3 or texture.shape[2] != 3 or min(texture.shape[:2]) < 2 or texture.dtype != torch.uint8 or not texture.is_contiguous() \
                or texture.device != dev:
            raise L.Eg3dHipError(f'mesh_raster: texture must be contiguous uint8 [Ht >= 2, Wt >= 2, 3] on {dev}, got {tuple(texture.shape)} '
                                 f'{texture.dtype} on {texture.device}')
        p.uv, p.texture, p.Ht, p.Wt = uv.data_ptr(), texture.data_ptr(), texture.shape[0], texture.shape[1]
    elif mode == 'vertex':
        if colors is None:
            raise L.Eg3dHipError("mesh_raster: mode='vertex' needs colors")
        p.colors = _mesh_rows(colors, 'mesh_raster: colors', dev, V).data_ptr()
    else:
        if normals is None:
            raise L.Eg3dHipError("mesh_raster: mode='lambert' needs normals")
        p.normals = _mesh_rows(normals, 'mesh_raster: normals', dev, V).data_ptr()
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_mesh_raster_query_workspace(C.byref(p), C.byref(nbytes)), 'mesh_raster_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = dict(image=torch.empty((N, 3, res, res), dtype=torch.float32, device=dev), face=torch.empty((N, res, res), dtype=torch.int32, device=dev),
               z=torch.empty((N, res, res), dtype=torch.float32, device=dev), depth=torch.empty((N, res, res), dtype=torch.float32, device=dev),
               mask=torch.empty((N, res, res), dtype=torch.uint8, device=dev), bary=torch.empty((N, res, res, 3), dtype=torch.float32, device=dev))
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
    p.bad_faces, p.stats = counts.data_ptr(), counts.data_ptr() + 4
    for k, t in out.items():
        setattr(p, k, t.data_ptr())
    L.check(lib.eg3d_mesh_raster(C.byref(p), L.stream_ptr()), 'mesh_raster')
    n_bad, n_small, n_large = counts.tolist()
    if n_bad:
        raise L.Eg3dHipError(f'mesh_raster: {n_bad} face(s) with an index outside [0, {V})')
    out['small_faces'], out['large_faces'] = n_small, n_large
    return out


def grid_components(vol: torch.Tensor, level: float, connectivity: int = 6) -> dict:
    """Connected components of {vol > level} of the fp32 grid vol [D0,D1,D2] (eg3d_cc_*; include/eg3d_hip.h "Grid components").  Inside =
    v > level as in marching_cubes and iso_render (NaN and v == level are outside); connectivity 6 joins face neighbours, 26 also edge and
    corner neighbours.  Returns a dict:
      labels int32 [D0,D1,D2]   0 outside, 1..K inside, components numbered in ascending order of their smallest linear index
      sizes  int32 [K]          voxels per component;   roots int32 [K]  each component's smallest linear index
      count  K;   inside        voxels above the level (Python ints)
    The result is a function of the input alone (bit-identical between runs and builds).  Workspace (4 bytes per voxel) from the caching
    allocator; one host synchronise (the totals)."""
    vol = _grid3(vol, 'grid_components')
    if connectivity not in (6, 26):
        raise L.Eg3dHipError(f'grid_components: connectivity 6 or 26, got {connectivity!r}')
    dev = vol.device
    labels = torch.empty(vol.shape, dtype=torch.int32, device=dev)
    p = L.CcParams(vol=vol.data_ptr(), labels=labels.data_ptr(), D0=vol.shape[0], D1=vol.shape[1], D2=vol.shape[2], level=float(level),
                   connectivity=int(connectivity))
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_cc_query_workspace(C.byref(p), C.byref(nbytes)), 'cc_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    p.workspace, p.workspace_bytes, p.totals = ws.data_ptr(), nbytes.value, totals.data_ptr()
    L.check(lib.eg3d_cc_label(C.byref(p), L.stream_ptr()), 'cc_label')
    K, inside = totals.tolist()
    sizes = torch.empty(K, dtype=torch.int32, device=dev)
    roots = torch.empty(K, dtype=torch.int32, device=dev)
    p.count, p.sizes, p.roots = K, (sizes.data_ptr() if K else None), (roots.data_ptr() if K else None)
    L.check(lib.eg3d_cc_finish(C.byref(p), L.stream_ptr()), 'cc_finish')
    return dict(labels=labels, sizes=sizes, roots=roots, count=K, inside=inside)


def grid_keep(vol: torch.Tensor, labels: torch.Tensor, keep_mask: torch.Tensor, fill: float = -1000.0) -> torch.Tensor:
    """A copy of the fp32 grid vol in which every voxel of a component the mask drops holds `fill`: out = keep[labels] ? vol : fill with
    keep = (True, *keep_mask) -- keep_mask [K] is indexed by label - 1 (select_components' result), and label 0, the outside, stays as it
    was (NaN included).  labels as grid_components returns them.  One streaming launch (eg3d_cc_keep), no host synchronise."""
    vol = _grid3(vol, 'grid_keep')
    L.require_cuda(labels)
    if labels.shape != vol.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != vol.device:
        raise L.Eg3dHipError(f'grid_keep: labels must be contiguous int32 {tuple(vol.shape)} on {vol.device}, got {tuple(labels.shape)} {labels.dtype}')
    if keep_mask.dim() != 1:
        raise L.Eg3dHipError(f'grid_keep: keep_mask [K], got {tuple(keep_mask.shape)}')
    K = keep_mask.shape[0]
    table = torch.ones(K + 1, dtype=torch.uint8, device=vol.device)
    table[1:] = keep_mask.to(device=vol.device, dtype=torch.bool)
    out = torch.empty_like(vol)
    p = L.CcParams(vol=vol.data_ptr(), labels=labels.data_ptr(), D0=vol.shape[0], D1=vol.shape[1], D2=vol.shape[2], count=K, keep=table.data_ptr(),
                   out=out.data_ptr(), fill=float(fill))
    L.check(L.lib().eg3d_cc_keep(C.byref(p), L.stream_ptr()), 'cc_keep')
    return out


def _mesh_faces(t: torch.Tensor, what: str, dev) -> torch.Tensor:
    L.require_cuda(t)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.int32 or not t.is_contiguous():
        raise L.Eg3dHipError(f'{what} must be contiguous int32 [F, 3], got {tuple(t.shape)} {t.dtype}')
    if t.device != dev:
        raise L.Eg3dHipError(f'{what} is on {t.device}, expected {dev}')
    return t


def mesh_simplify(verts: torch.Tensor, faces: torch.Tensor, cell: float, origin=(0.0, 0.0, 0.0)) -> dict:
    """Vertex clustering (eg3d_simplify_*; specified step by step in include/eg3d_hip.h "Mesh simplification and smoothing"): the vertices
    verts fp32 [V,3] that fall in one cell of the grid of side `cell` anchored at `origin` become one vertex at their mean; faces int32 [F,3]
    that collapse, or repeat an earlier face with the same winding, are dropped, and so are clusters no face is left on.  Returns a dict:
      verts      fp32 [V',3]   in ascending (cell z, y, x) order, the order marching_cubes emits
      faces      int32 [F',3]  the survivors in their original order, each rotated so that its smallest index comes first (winding kept)
      vertex_map int32 [V]     the output vertex every input vertex went to, -1 where its cluster was removed
      clusters   int           occupied cells, before the unreferenced ones are removed
    A vertex that is not finite or lies outside cells [0, 2^21) of an axis, and a face index outside [0, V), raise.  The result is a function
    of the input alone (no atomics, fixed summation order).  The sorts and prefix sums between the kernels are torch's; one host synchronise
    (the flags and the counts)."""
    cell = float(cell)
    origin = [float(v) for v in origin]
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f'mesh_simplify: cell must be positive and finite, got {cell}')
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f'mesh_simplify: origin must be three finite numbers, got {origin}')
    verts = _mesh_rows(verts, 'mesh_simplify: verts')
    dev = verts.device
    faces = _mesh_faces(faces, 'mesh_simplify: faces', dev)
    V, F = verts.shape[0], faces.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    lib, st = L.lib(), L.stream_ptr()
    flags, keys, heads = torch.empty(2, **i32), torch.empty(V, dtype=torch.int64, device=dev), torch.empty(V, **i32)
    tri, alive, used = torch.empty((3, F), **i32), torch.empty(F, **i32), torch.empty(V, **i32)
    vertex_map = torch.empty(V, **i32)
    p = L.SimplifyParams(verts=verts.data_ptr(), faces=faces.data_ptr(), V=V, F=F, cell=cell, flags=flags.data_ptr(), keys=keys.data_ptr(),
                         heads=heads.data_ptr(), tri=tri.data_ptr(), alive=alive.data_ptr(), used=used.data_ptr(), vertex_map=vertex_map.data_ptr())
    p.origin[:] = origin
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_simplify_query_workspace(C.byref(p), C.byref(nbytes)), 'simplify_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
    L.check(lib.eg3d_simplify_keys(C.byref(p), st), 'simplify_keys')
    skeys, order = torch.sort(keys, stable=True)
    p.sorted_keys, p.order = skeys.data_ptr(), order.data_ptr()
    L.check(lib.eg3d_simplify_heads(C.byref(p), st), 'simplify_heads')
    head_scan = torch.cumsum(heads, 0, dtype=torch.int32)
    p.head_scan = head_scan.data_ptr()
    L.check(lib.eg3d_simplify_clusters(C.byref(p), st), 'simplify_clusters')
    face_order = None
    for k in (2, 1, 0):                                   # three stable column sorts: lexicographic in (column 0, 1, 2, index), any K
        idx = torch.sort(tri[k] if face_order is None else tri[k][face_order], stable=True)[1]
        face_order = idx if face_order is None else face_order[idx]
    p.face_order = face_order.data_ptr()
    L.check(lib.eg3d_simplify_mark(C.byref(p), st), 'simplify_mark')
    alive_scan, used_scan = torch.cumsum(alive, 0, dtype=torch.int32), torch.cumsum(used, 0, dtype=torch.int32)
    p.alive_scan, p.used_scan = alive_scan.data_ptr(), used_scan.data_ptr()
    zero = torch.zeros(1, **i32)
    last = lambda t: t[-1:] if t.numel() else zero      # noqa: E731
    bad_vertex, bad_face, K, F2, V2 = torch.cat([flags, last(head_scan), last(alive_scan), last(used_scan)]).tolist()
    if bad_vertex:
        raise L.Eg3dHipError(f'mesh_simplify: a vertex is not finite or lies outside cells [0, 2^21) of the grid (cell {cell}, origin {origin})')
    if bad_face:
        raise L.Eg3dHipError(f'mesh_simplify: a face index lies outside [0, {V})')
    out_verts, out_faces = torch.empty((V2, 3), dtype=torch.float32, device=dev), torch.empty((F2, 3), **i32)
    p.out_verts, p.out_vert_capacity = (out_verts.data_ptr() if V2 else None), V2
    p.out_faces, p.out_face_capacity = (out_faces.data_ptr() if F2 else None), F2
    L.check(lib.eg3d_simplify_emit(C.byref(p), st), 'simplify_emit')
    return dict(verts=out_verts, faces=out_faces, vertex_map=vertex_map, clusters=K)


def mesh_adjacency(faces: torch.Tensor, V: int):
    """(rowptr int32 [V+1], cols int32 [nnz], boundary uint8 [V]) of the faces [F,3] (any integer dtype) with indices in [0, V): row i of the CSR holds the
    distinct j != i that share a face edge with i, ascending; boundary marks the endpoints of undirected edges that occur exactly once among
    the faces' edges.  Plain torch on integers (sort, unique, searchsorted): the result is unique.  What eg3d_smooth reads."""
    dev = faces.device
    f = faces.to(torch.int64)
    a, b = torch.cat([f[:, 0], f[:, 1], f[:, 2]]), torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b                                         # a face with a repeated index adds no self-edge
    lo, hi = torch.minimum(a, b)[keep], torch.maximum(a, b)[keep]
    ukey, count = torch.unique(lo * V + hi, return_counts=True)
    lo, hi = torch.div(ukey, V, rounding_mode='floor'), torch.remainder(ukey, V)
    boundary = torch.zeros(V, dtype=torch.uint8, device=dev)
    once = count == 1
    boundary[lo[once]] = 1
    boundary[hi[once]] = 1
    dkey = torch.sort(torch.cat([lo * V + hi, hi * V + lo]))[0]       # distinct: (row, column) ascending
    rows, cols = torch.div(dkey, V, rounding_mode='floor'), torch.remainder(dkey, V).to(torch.int32)
    if rows.numel() > _INT32_MAX:
        L.check(-3, f'mesh_adjacency ({rows.numel()} directed edges)')
    rowptr = torch.searchsorted(rows, torch.arange(V + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    return rowptr, cols.contiguous(), boundary


def mesh_smooth(verts: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                pin_boundary: bool = True) -> torch.Tensor:
    """fp32 [V,3]: Taubin lambda|mu smoothing of verts fp32 [V,3] over the edges of faces int32 [F,3] with uniform (umbrella) weights
    (eg3d_smooth; include/eg3d_hip.h "Mesh simplification and smoothing").  One iteration moves every vertex by lam times its offset from the
    mean of its neighbours, then by mu times (mu < -lam: the second pass undoes the shrinkage of the first).  pin_boundary keeps the endpoints
    of edges that belong to one face only where they are.  A vertex without neighbours stays.  iterations=0 returns a copy.  A face index
    outside [0, V) raises.  The adjacency is built once per call with torch's integer sort / unique (mesh_adjacency: host synchronises there);
    then 2 * iterations launches with no host synchronise between them.  Jacobi passes with a fixed order of every sum: the result is a
    function of the input alone."""
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if iterations < 0:
        raise ValueError(f'mesh_smooth: iterations >= 0, got {iterations}')
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f'mesh_smooth: lam and mu must be finite, got {lam}, {mu}')
    verts = _mesh_rows(verts, 'mesh_smooth: verts')
    dev = verts.device
    faces = _mesh_faces(faces, 'mesh_smooth: faces', dev)
    V = verts.shape[0]
    if faces.numel() and bool(((faces < 0) | (faces >= V)).any()):
        raise L.Eg3dHipError(f'mesh_smooth: a face index lies outside [0, {V})')
    out = torch.empty_like(verts)
    p = L.SmoothParams(verts=verts.data_ptr(), out=out.data_ptr(), V=V, iterations=iterations, lam=lam, mu=mu)
    if iterations > 0 and V > 0:
        rowptr, cols, boundary = mesh_adjacency(faces, V)
        p.rowptr, p.cols, p.nnz = rowptr.data_ptr(), (cols.data_ptr() if cols.numel() else None), cols.numel()
        p.pinned = boundary.data_ptr() if pin_boundary else None
    nbytes = C.c_int64(0)
    L.check(L.lib().eg3d_smooth_query_workspace(C.byref(p), C.byref(nbytes)), 'smooth_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = (ws.data_ptr() if nbytes.value else None), nbytes.value
    L.check(L.lib().eg3d_smooth(C.byref(p), L.stream_ptr()), 'smooth')
    return out


def _ssim_params(x, y, mode, weights, nonnegative, size_average, win_size, win_sigma, C1, C2):
    N, Ch, Hh, Ww = x.shape
    p = L.SsimParams(x=x.data_ptr(), y=y.data_ptr(), N=N, C=Ch, H=Hh, W=Ww, mode=mode, levels=len(weights), nonnegative=int(bool(nonnegative)),
                     size_average=int(bool(size_average)), win_size=int(win_size), win_sigma=float(win_sigma), C1=float(C1), C2=float(C2))
    p.weights[:len(weights)] = [float(w) for w in weights]
    pyr, st, fwd, bwd = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    L.check(L.lib().eg3d_ssim_query_workspace(C.byref(p), C.byref(pyr), C.byref(st), C.byref(fwd), C.byref(bwd)), 'ssim_query_workspace')
    return p, pyr.value, st.value, fwd.value, bwd.value


def ssim_forward(x, y, mode, weights, nonnegative=False, size_average=True, win_size=11, win_sigma=1.5, C1=1e-4, C2=9e-4):
    """SSIM (mode 0, one level) / MS-SSIM (mode 1, len(weights) levels) of fp32 [N,C,H,W] images (eg3d_ssim_*; include/eg3d_hip.h):
    (out [N] or [] with size_average, pooled pyramid, per-channel stats) -- the last two are what ssim_backward reads.  levels + 1 launches,
    workspace from the caching allocator, no host synchronise."""
    L.require_cuda(x, y)
    x, y = x.contiguous(), y.contiguous()
    p, npyr, nst, fwd, _ = _ssim_params(x, y, mode, weights, nonnegative, size_average, win_size, win_sigma, C1, C2)
    dev = x.device
    pyr = torch.empty(max(npyr, 1), dtype=torch.float32, device=dev)
    stats = torch.empty(nst, dtype=torch.float64, device=dev)
    out = torch.empty(1 if size_average else x.shape[0], dtype=torch.float32, device=dev)
    ws = torch.empty(fwd, dtype=torch.uint8, device=dev)
    p.pyramid, p.stats, p.out, p.workspace, p.workspace_bytes = pyr.data_ptr(), stats.data_ptr(), out.data_ptr(), ws.data_ptr(), fwd
    L.check(L.lib().eg3d_ssim_forward(C.byref(p), L.stream_ptr()), 'ssim_forward')
    return (out.view(()) if size_average else out), pyr, stats


def ssim_backward(x, y, pyr, stats, grad_out, need_x, need_y, mode, weights, nonnegative=False, size_average=True, win_size=11, win_sigma=1.5,
                  C1=1e-4, C2=9e-4):
    """(grad_x, grad_y) of ssim_forward's output weighted by grad_out (either None when not needed): 2 launches per level, coarsest first."""
    x, y = x.contiguous(), y.contiguous()
    p, _, _, _, bwd = _ssim_params(x, y, mode, weights, nonnegative, size_average, win_size, win_sigma, C1, C2)
    g = grad_out.detach().float().contiguous().reshape(-1)
    gx = torch.empty_like(x) if need_x else None
    gy = torch.empty_like(y) if need_y else None
    ws = torch.empty(bwd, dtype=torch.uint8, device=x.device)
    p.pyramid, p.stats, p.workspace, p.workspace_bytes = pyr.data_ptr(), stats.data_ptr(), ws.data_ptr(), bwd
    p.grad_out, p.grad_x, p.grad_y = g.data_ptr(), (gx.data_ptr() if need_x else None), (gy.data_ptr() if need_y else None)
    L.check(L.lib().eg3d_ssim_backward(C.byref(p), L.stream_ptr()), 'ssim_backward')
    return gx, gy


def face_pool(x: torch.Tensor, r0: int, r1: int, c0: int, c1: int, size: int) -> torch.Tensor:
    """AdaptiveAvgPool2d(size)(x[:, :, r0:r1, c0:c1]) (bounds within the image) of fp32 [N,3,H,W], written as the channels-last [N,4,size,size]
    image with a zero fourth channel that the IR-SE trunk takes (eg3d_face_pool): one launch."""
    L.require_cuda(x)
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise L.Eg3dHipError(f'face_pool: fp32 [N,3,H,W], got {tuple(x.shape)} {x.dtype}')
    x = x.contiguous()
    N, _, Hh, Ww = x.shape
    out = empty_cl(N, 4, size, size, x.device)
    L.check(L.lib().eg3d_face_pool(x.data_ptr(), N, Hh, Ww, r0, r1, c0, c1, size, out.data_ptr(), L.stream_ptr()), 'face_pool')
    return out


# ------------------------------------------------------------------------------------------------- BatchNorm on batch statistics
def _bn_params(x, gamma, act):
    N, Cc, Hh, Ww = x.shape
    M = N * Hh * Ww
    nbytes = C.c_int64(0)
    L.check(L.lib().eg3d_batchnorm_query_workspace(M, Cc, C.byref(nbytes)), 'batchnorm_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    p = L.BatchNormParams(x=x.data_ptr(), gamma=gamma.data_ptr(), M=M, C=Cc, act=L.ACT_IDS[act], workspace=ws.data_ptr(), workspace_bytes=nbytes.value)
    return p, ws


class _BatchNormTrainFn(torch.autograd.Function):
    """eg3d_batchnorm_forward / eg3d_batchnorm_backward (csrc/batchnorm.hip): three launches each, running statistics updated on the device."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, num_batches_tracked, momentum, eps, act):
        L.require_cuda(x, gamma, beta, residual, running_mean, running_var, num_batches_tracked)
        if not is_cl(x) or (residual is not None and not (is_cl(residual) and residual.shape == x.shape)):
            raise L.Eg3dHipError(f'batch_norm_train: fp32 channels-last [N,C,H,W] operands, got {tuple(x.shape)} {x.dtype} strides {x.stride()}')
        for t in (running_mean, running_var):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous()):
                raise L.Eg3dHipError('batch_norm_train: running statistics must be contiguous fp32')
        if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
            raise L.Eg3dHipError('batch_norm_train: num_batches_tracked must be int64')
        g, b = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
        N, Cc, Hh, Ww = x.shape
        y = empty_cl(N, Cc, Hh, Ww, x.device)
        stats = torch.empty(2 * Cc, dtype=torch.float64, device=x.device)
        save = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
        p, ws = _bn_params(x, g, act)
        p.beta, p.residual, p.y = b.data_ptr(), L.ptr(residual), y.data_ptr()
        p.eps, p.momentum = float(eps), float(momentum)
        p.running_mean, p.running_var, p.num_batches_tracked = L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked)
        p.save_mean, p.save_invstd, p.stats = save[0].data_ptr(), save[1].data_ptr(), stats.data_ptr()
        L.check(L.lib().eg3d_batchnorm_forward(C.byref(p), L.stream_ptr()), 'batchnorm_forward')
        ctx.save_for_backward(x, g, y if act == 'relu' else None, stats)
        ctx.act, ctx.has_res = act, residual is not None
        ctx.mark_non_differentiable(save)
        return y, save

    @staticmethod
    def backward(ctx, dy, _dsave):
        x, g, y, stats = ctx.saved_tensors
        need_x, need_g, need_b, need_r = ctx.needs_input_grad[:4]
        dy = to_cl(dy.float())
        N, Cc, Hh, Ww = x.shape
        dx = empty_cl(N, Cc, Hh, Ww, x.device) if need_x else None
        dres = None
        if need_r and ctx.has_res:
            dres = empty_cl(N, Cc, Hh, Ww, x.device) if ctx.act == 'relu' else dy          # linear: dy' is dy itself
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
        p, ws = _bn_params(x, g, ctx.act)
        p.y, p.stats, p.dy = L.ptr(y), stats.data_ptr(), dy.data_ptr()
        p.dx, p.dresidual = L.ptr(dx), (dres.data_ptr() if (dres is not None and dres is not dy) else None)
        p.dgamma, p.dbeta = dgb[0].data_ptr(), dgb[1].data_ptr()
        L.check(L.lib().eg3d_batchnorm_backward(C.byref(p), L.stream_ptr()), 'batchnorm_backward')
        return dx, (dgb[0] if need_g else None), (dgb[1] if need_b else None), dres, None, None, None, None, None, None


def batch_norm_train(x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1, eps=1e-5, residual=None, act='linear',
                     return_stats=False):
    """act(batch_norm(x; batch statistics) * gamma + beta [+ residual]) -- torch.nn.BatchNorm2d in training mode, with the residual add and the
    ReLU of a ResNet block folded into the same pass.  The running buffers (and the batch counter) are updated in place as PyTorch does
    (through raw pointers: their tensor version counters do not move, so a cache keyed on them must be dropped by the caller):
    momentum-weighted, the unbiased variance into running_var.  Gradients flow into x, gamma, beta and residual.  GPU: fp32 channels-last
    tensors on the HIP kernels (csrc/batchnorm.hip; capturable, no host read); a missing kernel is an error.  CPU tensors: the same function
    composed from torch.nn.functional.batch_norm(training=True) + add + relu, so that callers can be exercised without a GPU.
    return_stats: also return the saved [2,C] fp32 (batch mean, 1 / sqrt(var + eps)) (GPU only)."""
    if act not in ('linear', 'relu'):
        raise ValueError(f"batch_norm_train: act must be 'linear' or 'relu', got {act!r}")
    if momentum is None:
        raise ValueError('batch_norm_train: a cumulative moving average (momentum=None) is not supported')
    if not x.is_cuda:
        y = torch.nn.functional.batch_norm(x, running_mean, running_var, gamma, beta, True, float(momentum), float(eps))
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        if residual is not None:
            y = y + residual
        y = torch.relu(y) if act == 'relu' else y
        assert not return_stats, 'the saved statistics are those of the HIP kernel'
        return y
    y, save = _BatchNormTrainFn.apply(x, gamma, beta, residual, running_mean, running_var, num_batches_tracked, float(momentum), float(eps), act)
    return (y, save) if return_stats else y


# ------------------------------------------------------------------------------------------------- GANSpace: PCA of W, edit grids (csrc/pca.hip)
PCA_SLAB_ROWS = 256              # EG3D_PCA_SLAB_ROWS: the rows one fp32 sum of pca_moments runs over
PCA_MAX_DIM = 512


class PcaMoments:
    """Running second moments of row data about `shift`: fp64 device accumulators gram [D,D], sum [D], and the rows seen so far."""

    def __init__(self, shift):
        D = shift.numel()
        self.shift = shift
        self.gram = torch.zeros((D, D), dtype=torch.float64, device=shift.device)
        self.sum = torch.zeros(D, dtype=torch.float64, device=shift.device)
        self.n = 0


def pca_moments_slabs(S: int, D: int) -> int:
    """Slabs eg3d_pca_moments splits S rows of D columns into: each slab's sums run in fp32 over at most PCA_SLAB_ROWS rows."""
    r = L.lib().eg3d_pca_moments_slabs(int(S), int(D))
    L.check(min(r, 0), 'pca_moments_slabs')
    return r


def pca_moments(x: torch.Tensor, shift: Optional[torch.Tensor], state: Optional[PcaMoments] = None) -> PcaMoments:
    """Adds the rows of x [S,D] (fp32, D <= 512, unit column stride) to `state` (a new one about `shift` [D] when None; a later chunk's
    `shift` is ignored: the state keeps its own).  Per-slab exact fp32 products, slabs added in order into fp64: no atomics."""
    L.require_cuda(x, shift)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or not 1 <= x.shape[1] <= PCA_MAX_DIM:
        raise L.Eg3dHipError(f'pca_moments: fp32 rows [S >= 1, 1 <= D <= {PCA_MAX_DIM}], got {tuple(x.shape)} {x.dtype}')
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    S, D = x.shape
    if state is None:
        if shift is None or shift.numel() != D:
            raise L.Eg3dHipError(f'pca_moments: the first chunk needs a shift of {D} values')
        state = PcaMoments(shift.detach().to(torch.float32).reshape(D).contiguous().clone())
    elif state.shift.numel() != D or state.shift.device != x.device:
        raise L.Eg3dHipError(f'pca_moments: the state holds {state.shift.numel()} columns on {state.shift.device}, the chunk {D} on {x.device}')
    slabs = pca_moments_slabs(S, D)
    part = torch.empty(slabs * (D * D + D), dtype=torch.float32, device=x.device)
    gp, sp = part[:slabs * D * D], part[slabs * D * D:]
    lib = L.lib()
    L.check(lib.eg3d_pca_moments(L.ptr(x), S, D, x.stride(0), L.ptr(state.shift), L.ptr(gp), L.ptr(sp), L.stream_ptr()), 'pca_moments')
    L.check(lib.eg3d_pca_moments_accumulate(L.ptr(gp), L.ptr(sp), slabs, D, L.ptr(state.gram), L.ptr(state.sum), L.stream_ptr()), 'pca_moments_accumulate')
    state.n += S
    return state


def pca_covariance(state: PcaMoments):
    """(cov fp32 [D,D] with ddof 0, bit-symmetric; mean fp32 [D]; rows seen) of everything added to `state`."""
    if state.n < 1:
        raise L.Eg3dHipError('pca_covariance: no rows were added')
    D = state.shift.numel()
    cov = torch.empty((D, D), dtype=torch.float32, device=state.shift.device)
    mean = torch.empty(D, dtype=torch.float32, device=state.shift.device)
    L.check(L.lib().eg3d_pca_covariance(L.ptr(state.gram), L.ptr(state.sum), state.n, D, L.ptr(state.shift), L.ptr(cov), L.ptr(mean), L.stream_ptr()),
            'pca_covariance')
    return cov, mean, state.n


def sym_eig(a: torch.Tensor, max_sweeps: int = 60, tol: Optional[float] = None):
    """(evals [n] descending, evecs [n,n] with eigenvector i as row i and its largest-magnitude entry positive, sweeps, converged) of the
    symmetric fp32 matrix a [n,n], n <= 512 (eg3d_sym_eig: parallel-ordered Jacobi, one launch per round).  Synchronises once per sweep: not
    capturable.  Reaching max_sweeps is reported (converged False, outputs still written), not raised.  tol None: 8 * 2^-23."""
    L.require_cuda(a)
    if a.dim() != 2 or a.shape[0] != a.shape[1] or a.dtype != torch.float32 or not 1 <= a.shape[0] <= PCA_MAX_DIM:
        raise L.Eg3dHipError(f'sym_eig: a square fp32 matrix of side 1..{PCA_MAX_DIM}, got {tuple(a.shape)} {a.dtype}')
    if torch.cuda.is_current_stream_capturing():
        raise L.Eg3dHipError('sym_eig reads its convergence flag back every sweep: it cannot be captured into a graph')
    a = a.contiguous()
    n = a.shape[0]
    nbytes = C.c_int64(0)
    lib = L.lib()
    L.check(lib.eg3d_sym_eig_workspace(n, C.byref(nbytes)), 'sym_eig_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device)
    evals = torch.empty(n, dtype=torch.float32, device=a.device)
    evecs = torch.empty((n, n), dtype=torch.float32, device=a.device)
    info = (C.c_int32 * 2)(0, 0)
    L.check(lib.eg3d_sym_eig(L.ptr(a), n, L.ptr(evals), L.ptr(evecs), int(max_sweeps), float(tol or 0.0), L.ptr(ws), info, L.stream_ptr()), 'sym_eig')
    return evals, evecs, int(info[0]), bool(info[1])


def image_grid_size(N: int, H: int, W: int, nrow: int, padding: int = 2):
    """(Ht, Wt) of torchvision.utils.make_grid for N images of H x W."""
    xmaps = min(int(nrow), N)
    ymaps = -(-N // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


MESH_TEXTURE_MAX_SIDE = 16384


def mesh_texture_size(F: int, tile: int = 8):
    """(Ht, Wt) of mesh_texture's atlas for F faces: two faces per tile x tile block, ceil(sqrt(blocks)) blocks per row (integer arithmetic;
    eg3d_mesh_texture_size computes the same).  F = 0 gives one block.  A side above 16384 raises."""
    F, tile = int(F), int(tile)
    if F < 0 or not 4 <= tile <= 64:
        raise ValueError(f'mesh_texture_size: F >= 0 and tile in [4, 64], got F = {F}, tile = {tile}')
    nb = max(-(-F // 2), 1)
    per_row = math.isqrt(nb - 1) + 1                      # ceil(sqrt(nb)) for nb >= 1
    Ht, Wt = tile * -(-nb // per_row), tile * per_row
    if max(Ht, Wt) > MESH_TEXTURE_MAX_SIDE:
        raise L.Eg3dHipError(f'mesh_texture: {F} faces at tile {tile} need a {Ht} x {Wt} atlas, above {MESH_TEXTURE_MAX_SIDE} a side: '
                             'simplify the mesh first (simplify_mesh) or lower `tile`')
    return Ht, Wt


def image_grid_u8(img: torch.Tensor, nrow: int, padding: int = 2, pad_value: int = 0) -> torch.Tensor:
    """uint8 [Ht,Wt,3]: the fp32 [N,3,H,W] batch as uint8(clamp(x * 127.5 + 128, 0, 255)), tiled HWC the way torchvision.utils.make_grid(nrow,
    padding, pad_value) tiles (eg3d_image_grid_u8); padding=0 is a plain tiling, nrow=1 with padding=0 a column of images.  One launch."""
    L.require_cuda(img)
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32 or img.shape[0] < 1:
        raise L.Eg3dHipError(f'image_grid_u8: fp32 [N >= 1,3,H,W], got {tuple(img.shape)} {img.dtype}')
    img = img.contiguous()
    N, _, Hh, Ww = img.shape
    Ht, Wt = image_grid_size(N, Hh, Ww, nrow, padding)
    out = torch.empty((Ht, Wt, 3), dtype=torch.uint8, device=img.device)
    L.check(L.lib().eg3d_image_grid_u8(L.ptr(img), N, Hh, Ww, int(nrow), int(padding), int(pad_value), L.ptr(out), L.stream_ptr()), 'image_grid_u8')
    return out


_jpeg_headers = {}


def jpeg_encode(img: torch.Tensor, quality: int = 90, subsampling: str = '420', restart_interval: Optional[int] = None):
    """(bytes uint8 [total], offsets int64 [N+1] on the host): N baseline JFIF files back to back, frame n = bytes[offsets[n]:offsets[n+1]]
    (eg3d_jpeg_*; include/eg3d_hip.h).  img [N,C,H,W], C = 3 (RGB) or 1 (grey): fp32 in [-1,1], quantised as image_grid_u8, or uint8 as is.
    subsampling '420' | '444' (grey ignores it); restart_interval in MCUs, None = MCUs per row capped at 32 -- every interval is coded by its
    own wave.  The header (video.jpeg_header) is built and uploaded once per configuration.  Four launches, workspace from the caching
    allocator, one host synchronise (the total)."""
    from . import video as V
    L.require_cuda(img)
    if img.dim() != 4 or img.shape[1] not in (1, 3) or img.dtype not in (torch.float32, torch.uint8) or min(img.shape) < 1:
        raise L.Eg3dHipError(f'jpeg_encode: fp32 or uint8 [N >= 1, 1 | 3, H, W], got {tuple(img.shape)} {img.dtype}')
    if subsampling not in ('420', '444'):
        raise L.Eg3dHipError(f"jpeg_encode: subsampling '420' | '444', got {subsampling!r}")
    img = img.contiguous()
    N, Ch, Hh, Ww = img.shape
    dev = img.device
    R = V.default_restart_interval(Hh, Ww, subsampling, Ch) if restart_interval is None else int(restart_interval)
    if not (1 <= R <= V.MAX_RESTART_INTERVAL and 1 <= int(quality) <= 100):
        raise L.Eg3dHipError(f'jpeg_encode: restart interval 1..{V.MAX_RESTART_INTERVAL} and quality 1..100, got {R}, {quality}')
    key = (Hh, Ww, Ch, subsampling, int(quality), R, dev)
    hdr = _jpeg_headers.get(key)
    if hdr is None:
        if len(_jpeg_headers) >= 64:
            _jpeg_headers.clear()
        raw = V.jpeg_header(Hh, Ww, quality=int(quality), subsampling=subsampling, restart_interval=R, channels=Ch)
        hdr = _jpeg_headers[key] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    p = L.JpegParams(img=img.data_ptr(), header=hdr.data_ptr(), header_bytes=hdr.numel(), dtype=L.JPEG_F32 if img.dtype == torch.float32 else L.JPEG_U8,
                     N=N, C=Ch, H=Hh, W=Ww, subsampling=L.JPEG_420 if subsampling == '420' else L.JPEG_444, quality=int(quality), restart_interval=R)
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_jpeg_query_workspace(C.byref(p), C.byref(nbytes)), 'jpeg_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    p.workspace, p.workspace_bytes, p.offsets = ws.data_ptr(), nbytes.value, offsets.data_ptr()
    L.check(lib.eg3d_jpeg_encode(C.byref(p), L.stream_ptr()), 'jpeg_encode')
    offsets = offsets.cpu()
    total = int(offsets[N])
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    p.out, p.out_capacity = out.data_ptr(), total
    L.check(lib.eg3d_jpeg_pack(C.byref(p), L.stream_ptr()), 'jpeg_pack')
    return out, offsets


class JpegDecodeRefused(L.Eg3dHipError):
    """hipops.jpeg_decode: the device ended in a non-zero status (a damaged or unusual entropy-coded stream); .status holds the bits."""

    def __init__(self, status: int):
        why = '; '.join(text for bit, text in L.JPEGDEC_ERRORS.items() if status & bit)
        super().__init__(f'jpeg_decode: the device refused the entropy-coded data: status {status} ({why})')
        self.status = status


def jpeg_decode_tables(plan) -> bytes:
    """eg3d_jpegdec_params.tables for a video.JpegScanPlan: the quantisation tables 0..3 (natural order, zeros where the file has none), then
    the Huffman tables DC 0, DC 1, AC 0, AC 1 as BITS[16] HUFFVAL[256] (zeros where the file has none)."""
    blob = bytearray()
    for q in plan.quant:
        blob += bytes(q) if q is not None else bytes(64)
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        bits, vals = plan.huffman.get(key, ((0,) * 16, ()))
        blob += bytes(bits) + bytes(vals) + bytes(256 - len(vals))
    assert len(blob) == L.JPEGDEC_TABLE_BYTES
    return bytes(blob)


def _jpegdec_begin(raw: bytes, subseq_bytes: int, device=None):
    """Parse, upload and allocate for one eg3d_jpegdec_decode: (params, tensors the params point into, out, result)."""
    from . import video as V
    B = int(subseq_bytes)
    if not (16 <= B <= 1024 and B & (B - 1) == 0):
        raise L.Eg3dHipError(f'jpeg_decode: subseq_bytes a power of two in 16..1024, got {subseq_bytes}')
    plan = V.jpeg_scan_plan(raw)
    if not torch.cuda.is_available():
        raise L.Eg3dHipError('jpeg_decode: no GPU (there is no fallback path)')
    dev = torch.device('cuda' if device is None else device)
    n = plan.scan_end - plan.scan_start
    head = (L.JPEGDEC_TABLE_BYTES + 15) // 16 * 16
    host = torch.zeros(head + (n + 15) // 16 * 16, dtype=torch.uint8)             # tables, then the entropy-coded segment, both 16-byte aligned
    view = host.numpy()
    view[:L.JPEGDEC_TABLE_BYTES] = np.frombuffer(jpeg_decode_tables(plan), dtype=np.uint8)
    view[head:head + n] = np.frombuffer(raw, dtype=np.uint8, count=n, offset=plan.scan_start)
    blob = host.to(dev)
    comps = plan.components
    p = L.JpegDecParams(data=blob.data_ptr() + head, data_bytes=n, tables=blob.data_ptr(), H=plan.height, W=plan.width, ncomp=len(comps),
                        hsamp=comps[0].h, vsamp=comps[0].v, restart_interval=plan.restart_interval, subseq_bytes=B)
    for c, comp in enumerate(comps):
        p.tq[c], p.td[c], p.ta[c] = comp.tq, comp.td, comp.ta
    nbytes = C.c_int64(0)
    L.check(L.lib().eg3d_jpegdec_query_workspace(C.byref(p), C.byref(nbytes)), 'jpegdec_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.empty((plan.height, plan.width, 3), dtype=torch.uint8, device=dev)
    result = torch.empty(L.JPEGDEC_RESULT_WORDS, dtype=torch.int32, device=dev)
    p.workspace, p.workspace_bytes, p.out, p.result = ws.data_ptr(), nbytes.value, out.data_ptr(), result.data_ptr()
    return p, (blob, ws), out, result


def jpeg_decode(data, subseq_bytes: int = 128, device=None, stats: Optional[dict] = None) -> torch.Tensor:
    """uint8 [H,W,3] on the device: the pixels PIL.Image.open(file).convert('RGB') gives for a baseline JPEG file, byte for byte (eg3d_jpegdec_*;
    include/eg3d_hip.h "Baseline JPEG decoder").  data: the file as bytes or as a host uint8 tensor.  The markers are parsed on the host
    (video.jpeg_scan_plan: video.JpegUnsupported for what the decoder does not take -- progressive, CMYK, other sampling factors, ...); the
    tables and the entropy-coded bytes go up in one copy; the device does the rest.  subseq_bytes (a power of two, 16..1024): the stretch of
    the stream one lane of the self-synchronising Huffman decode owns.  A stream the device refuses (a stray marker, restart markers that do
    not fit the geometry, a truncated or surplus segment, bits that are no code) raises JpegDecodeRefused (an Eg3dHipError) with the status: there is no fallback
    here.  One host synchronise (the status).  stats, if given, receives status, rounds (of the synchronisation: inside the workgroups +
    across them), lanes, unstuffed_bytes and restart_markers."""
    if isinstance(data, torch.Tensor) and (data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1):
        raise L.Eg3dHipError(f'jpeg_decode: the file as bytes or a host uint8 [n] tensor, got {data.dtype} {tuple(data.shape)} on {data.device}')
    raw = data.contiguous().numpy().tobytes() if isinstance(data, torch.Tensor) else bytes(data)
    p, keep, out, result = _jpegdec_begin(raw, subseq_bytes, device)
    with torch.cuda.device(out.device):
        L.check(L.lib().eg3d_jpegdec_decode(C.byref(p), L.stream_ptr()), 'jpegdec_decode')
        res = result.tolist()                                                      # the one synchronise
    del keep
    if stats is not None:
        stats.update(status=res[0], rounds=res[1] + res[2], rounds_workgroup=res[1], rounds_across=res[2], lanes=res[3], unstuffed_bytes=res[4],
                     restart_markers=res[5])
    if res[0] != 0:
        raise JpegDecodeRefused(res[0])
    return out


def _jpeg_file_bytes(data, who: str) -> bytes:
    if isinstance(data, torch.Tensor):
        if data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1:
            raise L.Eg3dHipError(f'{who}: the file as bytes or a host uint8 [n] tensor, got {data.dtype} {tuple(data.shape)} on {data.device}')
        return data.contiguous().numpy().tobytes()
    return bytes(data)


def _jpegdec_batch_begin(raws, plans, subseq_bytes: int, device=None):
    """Upload and allocate for one eg3d_jpegdec_batch_decode of already parsed files: (params, tensors the params point into, outs, result).
    One host buffer -- the plan records, then per file the tables and the entropy-coded bytes -- goes up in one copy; outs are views of one
    output buffer."""
    B = int(subseq_bytes)
    if not (16 <= B <= 1024 and B & (B - 1) == 0):
        raise L.Eg3dHipError(f'jpeg_decode_batch: subseq_bytes a power of two in 16..1024, got {subseq_bytes}')
    if not torch.cuda.is_available():
        raise L.Eg3dHipError('jpeg_decode_batch: no GPU (there is no fallback path)')
    dev = torch.device('cuda' if device is None else device)
    n = len(raws)
    images = (L.JpegDecImage * n)()
    p = L.JpegDecBatchParams(images=images, n=n, subseq_bytes=B)
    for im, plan in zip(images, plans):
        comps = plan.components
        im.H, im.W, im.ncomp, im.hsamp, im.vsamp = plan.height, plan.width, len(comps), comps[0].h, comps[0].v
        im.restart_interval, im.data_bytes = plan.restart_interval, plan.scan_end - plan.scan_start
        for c, comp in enumerate(comps):
            im.tq[c], im.td[c], im.ta[c] = comp.tq, comp.td, comp.ta
    ws_bytes, plan_bytes = C.c_int64(0), C.c_int64(0)
    lib = L.lib()
    L.check(lib.eg3d_jpegdec_batch_query_workspace(C.byref(p), C.byref(ws_bytes), C.byref(plan_bytes)), 'jpegdec_batch_query_workspace')
    head = (L.JPEGDEC_TABLE_BYTES + 15) // 16 * 16
    at, px = plan_bytes.value, 0
    for im in images:                                                              # tables, then the entropy-coded segment, both 16-byte aligned
        im.tables_offset, im.data_offset = at, at + head
        at += head + (im.data_bytes + 15) // 16 * 16
        px += im.H * im.W * 3
    host = torch.zeros(at, dtype=torch.uint8)
    view = host.numpy()
    for im, raw, plan in zip(images, raws, plans):
        view[im.tables_offset:im.tables_offset + L.JPEGDEC_TABLE_BYTES] = np.frombuffer(jpeg_decode_tables(plan), dtype=np.uint8)
        view[im.data_offset:im.data_offset + im.data_bytes] = np.frombuffer(raw, dtype=np.uint8, count=im.data_bytes, offset=plan.scan_start)
    blob = torch.empty(at, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev)
    out = torch.empty(px, dtype=torch.uint8, device=dev)
    result = torch.empty((n, L.JPEGDEC_RESULT_WORDS), dtype=torch.int32, device=dev)
    outs, px = [], 0
    for im in images:
        im.out = out.data_ptr() + px
        outs.append(out[px:px + im.H * im.W * 3].view(im.H, im.W, 3))
        px += im.H * im.W * 3
    p.plan, p.upload, p.upload_bytes, p.workspace, p.workspace_bytes, p.result = host.data_ptr(), blob.data_ptr(), at, ws.data_ptr(), ws_bytes.value, result.data_ptr()
    L.check(lib.eg3d_jpegdec_batch_plan(C.byref(p)), 'jpegdec_batch_plan')                # (host only: the records, with the device addresses in them)
    blob.copy_(host)                                                                     # the one upload
    p.plan = None
    return p, (images, blob, ws, out), outs, result


def _jpegdec_stats(res) -> dict:
    return dict(status=res[0], rounds=res[1] + res[2], rounds_workgroup=res[1], rounds_across=res[2], lanes=res[3], unstuffed_bytes=res[4],
                restart_markers=res[5])


def jpeg_decode_batch(files, subseq_bytes: int = 128, device=None, stats: Optional[list] = None, return_errors: bool = False,
                      default_huffman: bool = False) -> list:
    """[uint8 [H,W,3] on the device per file]: jpeg_decode's pixels for every file of `files` (bytes or host uint8 tensors; any mix of sizes,
    samplings, restart intervals and tables) in ONE device call (eg3d_jpegdec_batch_*; include/eg3d_hip.h "Baseline JPEG decoder, N images per
    call"): one host buffer, one upload, one workspace, one output buffer of which the returned contiguous tensors are views, the launches of
    a single decode, one host synchronise (the statuses).  Every file is parsed by video.jpeg_scan_plan (default_huffman: Annex K's tables
    for those a file does not define, as Motion-JPEG frames leave them out).  A file the parser does not take raises video.JpegUnsupported
    before anything runs; else the first file the device refuses raises JpegDecodeRefused.  return_errors=True: nothing raises; the list
    holds the exception instance in place of that file's tensor, files that fail the parse never enter the device batch and every other file
    is decoded.  stats, if given, is a list that receives one dict per file as jpeg_decode fills it (None for a file that failed the
    parse).  An empty `files` gives []."""
    from . import video as V
    raws = [_jpeg_file_bytes(f, 'jpeg_decode_batch') for f in files]
    got: list = [None] * len(raws)
    plans, taken = [], []
    for i, raw in enumerate(raws):
        try:
            plans.append(V.jpeg_scan_plan(raw, default_huffman=default_huffman))
            taken.append(i)
        except V.JpegUnsupported as e:
            if not return_errors:
                raise
            got[i] = e
    per: list = [None] * len(raws)
    if taken:
        p, keep, outs, result = _jpegdec_batch_begin([raws[i] for i in taken], plans, subseq_bytes, device)
        with torch.cuda.device(result.device):
            L.check(L.lib().eg3d_jpegdec_batch_decode(C.byref(p), L.stream_ptr()), 'jpegdec_batch_decode')
            res = result.tolist()                                                  # the one synchronise
        del keep
        for i, out, r in zip(taken, outs, res):
            per[i] = _jpegdec_stats(r)
            got[i] = out if r[0] == 0 else JpegDecodeRefused(r[0])
    if stats is not None:
        stats[:] = per
    if not return_errors:
        for g in got:
            if isinstance(g, Exception):
                raise g
    return got


PNG_FILTERS = dict(adaptive=-1, none=0, sub=1, up=2, average=3, paeth=4)


def _png_begin(img: torch.Tensor, filter='adaptive', block_bytes: int = 32768, stages: int = 0):
    """The first two calls of the eg3d_png_* protocol: (params, workspace, offsets on the device).  The workspace must outlive the pack."""
    L.require_cuda(img)
    if img.dtype != torch.uint8 or img.dim() not in (2, 3, 4):
        raise L.Eg3dHipError(f'png_encode: uint8 [N,H,W,C], [H,W,C] or [H,W], got {tuple(img.shape)} {img.dtype}')
    if img.dim() == 2:
        img = img[None, :, :, None]
    elif img.dim() == 3:
        img = img[None]
    if img.shape[3] not in (1, 3) or min(img.shape) < 1:
        raise L.Eg3dHipError(f'png_encode: C = 1 or 3 and N, H, W >= 1, got {tuple(img.shape)}')
    f = PNG_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if isinstance(f, bool) or not isinstance(f, int) or not -1 <= f <= 4:
        raise L.Eg3dHipError(f'png_encode: filter one of {sorted(PNG_FILTERS)} or -1..4, got {filter!r}')
    img = img.contiguous()
    N, Hh, Ww, Ch = img.shape
    p = L.PngParams(img=img.data_ptr(), N=N, C=Ch, H=Hh, W=Ww, filter=f, block_bytes=int(block_bytes), stages=int(stages))
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_png_query_workspace(C.byref(p), C.byref(nbytes)), 'png_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=img.device)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=img.device)
    p.workspace, p.workspace_bytes, p.offsets = ws.data_ptr(), nbytes.value, offsets.data_ptr()
    L.check(lib.eg3d_png_encode(C.byref(p), L.stream_ptr()), 'png_encode')
    return p, (ws, img), offsets


def _png_pack(p, out: torch.Tensor, capacity: int, total: int) -> None:
    """The third call: the streams into out[:capacity]; capacity < total is refused before any launch."""
    p.out, p.out_capacity, p.total_bytes = out.data_ptr(), int(capacity), int(total)
    L.check(L.lib().eg3d_png_pack(C.byref(p), L.stream_ptr()), 'png_pack')


def png_encode(img: torch.Tensor, filter='adaptive', block_bytes: int = 32768):
    """(bytes uint8 [total] on the device, offsets int64 [N+1] on the host): N zlib streams back to back, image n's IDAT payload =
    bytes[offsets[n]:offsets[n+1]] (eg3d_png_*; include/eg3d_hip.h "PNG encoder"; video.png_container makes the file).  img uint8 [N,H,W,C],
    C = 1 (grey) or 3 (RGB); [H,W], [H,W,1] and [H,W,3] are one image.  filter 'adaptive' (per row the smallest sum of absolute values) or
    'none' | 'sub' | 'up' | 'average' | 'paeth' (or -1..4); block_bytes 64..65536 of filtered stream per deflate block, every block coded by
    its own workgroup with its own Huffman codes.  Five launches, workspace from the caching allocator, one host synchronise (the total)."""
    p, keep, offsets = _png_begin(img, filter, block_bytes)
    offsets = offsets.cpu()
    total = int(offsets[-1])
    out = torch.empty(total, dtype=torch.uint8, device=img.device)
    _png_pack(p, out, total, total)
    del keep
    return out, offsets


# ---- image ingestion (csrc/imgprep.hip; include/eg3d_hip.h "Image ingestion"): Pillow's resize and QUAD warp, align_face's pad, ToTensor ------
PIL_FILTER_SUPPORT = dict(bilinear=1.0, lanczos=3.0)
RESAMPLE_TILE = 64                       # EG3D_RESAMPLE_TILE: output pixels of a row one workgroup of the horizontal pass produces


def _pil_filter(name: str, t: float) -> float:
    if name == 'bilinear':
        t = -t if t < 0.0 else t
        return 1.0 - t if t < 1.0 else 0.0
    if -3.0 <= t < 3.0:                  # lanczos: sinc(t) sinc(t / 3), truncated
        sinc = lambda v: 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
        return sinc(t) * sinc(t / 3)
    return 0.0


def pil_resize_coeffs(in_size: int, out_size: int, filter: str):
    """(bounds int32 [out,2] = (xmin, count), coef int32 [out,ksize]) of Pillow's 8-bit resize along one axis (Resample.c precompute_coeffs +
    normalize_coeffs_8bpc): float64 weights of the `filter` ('bilinear' | 'lanczos') scaled to the reduction, normalised by their left-to-right
    sum, quantised to 22 fractional bits with the rounding offset following the weight's sign.  Plain numpy / host code."""
    if filter not in PIL_FILTER_SUPPORT:
        raise ValueError(f"pil_resize_coeffs: filter 'bilinear' | 'lanczos', got {filter!r}")
    if in_size < 1 or out_size < 1:
        raise ValueError(f'pil_resize_coeffs: sizes >= 1, got {in_size} -> {out_size}')
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = PIL_FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        count = min(int(c + support + 0.5), in_size) - xmin
        w = [_pil_filter(filter, (x + xmin - c + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, count)
        coef[xx, :count] = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
    return bounds, coef


def pil_quad_coeffs(size, quad) -> np.ndarray:
    """The eight float64 coefficients Pillow's Image.transform derives from QUAD data (NW, SW, SE, NE corners as x, y pairs) for an output of
    size = (w, h): xin = a0 + a1 xi + a2 yi + a3 xi yi, yin = a4 + ... with xi = x + 0.5, yi = y + 0.5."""
    w, h = int(size[0]), int(size[1])
    q = [float(v) for v in np.asarray(quad, dtype=np.float64).reshape(8)]
    nw, sw, se, ne = q[0:2], q[2:4], q[4:6], q[6:8]
    x0, y0 = nw
    As, At = 1.0 / w, 1.0 / h
    return np.array([x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                     y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At], np.float64)


def gauss_weights(sigma: float) -> np.ndarray:
    """g[0..radius] float64: one half of scipy.ndimage's normalised Gaussian kernel (radius int(4 sigma + 0.5))."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2) if radius > 0 else np.ones(1)
    phi = phi / phi.sum()
    return phi[radius:].copy()


def _u8_images(img: torch.Tensor, what: str):
    L.require_cuda(img)
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] not in (1, 3) or min(img.shape) < 1:
        raise L.Eg3dHipError(f'{what}: uint8 [N,H,W,C] or [H,W,C] with C = 1 | 3, got {tuple(img.shape)} {img.dtype}')
    x = img.contiguous()
    return (x[None] if img.dim() == 3 else x), img.dim() == 3


_resample_tables = {}


def _resample_axis(in_size: int, out_size: int, filter: str, dev, horizontal: bool):
    """Device tables of one pass (cached per configuration): bounds [out,2], coef ([ksize,out] tap-major for the horizontal pass, [out,ksize]
    for the vertical), ksize, and the longest input span a tile of RESAMPLE_TILE outputs reads."""
    key = (in_size, out_size, filter, str(dev), horizontal)
    hit = _resample_tables.get(key)
    if hit is None:
        if len(_resample_tables) >= 64:
            _resample_tables.clear()
        bounds, coef = pil_resize_coeffs(in_size, out_size, filter)
        seg = 0
        for t0 in range(0, out_size, RESAMPLE_TILE):
            t1 = min(t0 + RESAMPLE_TILE, out_size)
            seg = max(seg, int((bounds[t0:t1, 0] + bounds[t0:t1, 1]).max() - bounds[t0:t1, 0].min()))
        c = np.ascontiguousarray(coef.T) if horizontal else coef
        hit = _resample_tables[key] = (torch.from_numpy(bounds).to(dev), torch.from_numpy(c).to(dev), coef.shape[1], seg)
    return hit


def pil_resize(img: torch.Tensor, size, filter: str = 'bilinear') -> torch.Tensor:
    """PIL.Image.resize(size, filter) of uint8 images [N,H,W,C] (or [H,W,C]), C = 1 | 3, on the device, byte for byte (eg3d_resample8): size =
    (width, height) as Pillow takes it, filter 'bilinear' | 'lanczos' (ANTIALIAS).  The integer coefficient tables are built on the host
    (pil_resize_coeffs) and cached per configuration; one launch per axis that changes."""
    x, squeeze = _u8_images(img, 'pil_resize')
    if filter not in PIL_FILTER_SUPPORT:
        raise L.Eg3dHipError(f"pil_resize: filter 'bilinear' | 'lanczos', got {filter!r}")
    Wo, Ho = int(size[0]), int(size[1])
    N, Hi, Wi, Ch = x.shape
    if Wo < 1 or Ho < 1:
        raise L.Eg3dHipError(f'pil_resize: size >= 1, got {size}')
    dev = x.device
    out = torch.empty((N, Ho, Wo, Ch), dtype=torch.uint8, device=dev)
    p = L.Resample8Params(src=x.data_ptr(), dst=out.data_ptr(), N=N, Hi=Hi, Wi=Wi, C=Ch, Ho=Ho, Wo=Wo)
    keep = []
    if Wo != Wi:
        hb, hc, p.hksize, p.hseg = _resample_axis(Wi, Wo, filter, dev, True)
        p.hbounds, p.hcoef = hb.data_ptr(), hc.data_ptr()
        keep += [hb, hc]
    if Ho != Hi:
        vb, vc, p.vksize, _ = _resample_axis(Hi, Ho, filter, dev, False)
        p.vbounds, p.vcoef = vb.data_ptr(), vc.data_ptr()
        keep += [vb, vc]
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_resample8_query_workspace(C.byref(p), C.byref(nbytes)), 'resample8_query_workspace')
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
    L.check(lib.eg3d_resample8(C.byref(p), L.stream_ptr()), 'resample8')
    return out[0] if squeeze else out


def pil_quad_warp(img: torch.Tensor, size, quad) -> torch.Tensor:
    """PIL.Image.transform(size, QUAD, quad, BILINEAR) of uint8 images [N,H,W,C] (or [H,W,C]) on the device, byte for byte, pixels whose source
    falls outside the image 0 (eg3d_quad_warp8): size = (width, height), quad = the NW, SW, SE, NE corners as eight numbers (x, y pairs)."""
    x, squeeze = _u8_images(img, 'pil_quad_warp')
    Wo, Ho = int(size[0]), int(size[1])
    if Wo < 1 or Ho < 1:
        raise L.Eg3dHipError(f'pil_quad_warp: size >= 1, got {size}')
    N, Hi, Wi, Ch = x.shape
    out = torch.empty((N, Ho, Wo, Ch), dtype=torch.uint8, device=x.device)
    p = L.QuadWarp8Params(src=x.data_ptr(), dst=out.data_ptr(), N=N, Hi=Hi, Wi=Wi, C=Ch, Ho=Ho, Wo=Wo)
    p.a[:] = [float(v) for v in pil_quad_coeffs((Wo, Ho), quad)]
    L.check(L.lib().eg3d_quad_warp8(C.byref(p), L.stream_ptr()), 'quad_warp8')
    return out[0] if squeeze else out


_gauss_tables = {}


def feather_pad(img: torch.Tensor, pads, qsize: float) -> torch.Tensor:
    """The pad branch of the reference's align_face (utils/alignment.py:95-105) on the device (eg3d_feather_pad): uint8 [N,H,W,C] (or [H,W,C])
    reflect-padded by pads = (left, top, right, bottom) >= 1, blended towards its Gaussian blur (sigma 0.02 qsize) and then towards the
    per-channel median of the blended image by the reference's border mask, rounded to uint8.  fp32 with a pixel-fixed summation order."""
    x, squeeze = _u8_images(img, 'feather_pad')
    left, top, right, bottom = (int(v) for v in pads)
    if min(left, top, right, bottom) < 1:
        raise L.Eg3dHipError(f'feather_pad: pads >= 1 (the mask divides by them), got {tuple(pads)}')
    N, Hi, Wi, Ch = x.shape
    dev = x.device
    key = (float(qsize), str(dev))
    gd = _gauss_tables.get(key)
    if gd is None:
        if len(_gauss_tables) >= 64:
            _gauss_tables.clear()
        gd = _gauss_tables[key] = torch.from_numpy(gauss_weights(float(qsize) * 0.02).astype(np.float32)).to(dev)
    out = torch.empty((N, Hi + top + bottom, Wi + left + right, Ch), dtype=torch.uint8, device=dev)
    p = L.FeatherPadParams(src=x.data_ptr(), dst=out.data_ptr(), gauss=gd.data_ptr(), N=N, H=Hi, W=Wi, C=Ch, left=left, top=top, right=right,
                           bottom=bottom, radius=gd.numel() - 1)
    lib = L.lib()
    nbytes = C.c_int64(0)
    L.check(lib.eg3d_feather_pad_query_workspace(C.byref(p), C.byref(nbytes)), 'feather_pad_query_workspace')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
    L.check(lib.eg3d_feather_pad(C.byref(p), L.stream_ptr()), 'feather_pad')
    return out[0] if squeeze else out


def u8_to_target(img: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize([0.5] * 3, [0.5] * 3) of uint8 [N,H,W,3] (or [H,W,3]): fp32 [N,3,H,W] = (v / 255 - 0.5) / 0.5, every step a
    correctly rounded fp32 operation as torchvision's host pipeline computes it (eg3d_u8_to_target)."""
    x, _ = _u8_images(img, 'u8_to_target')
    if x.shape[-1] != 3:
        raise L.Eg3dHipError(f'u8_to_target: C = 3, got {tuple(img.shape)}')
    N, Hi, Wi, _ = x.shape
    out = torch.empty((N, 3, Hi, Wi), dtype=torch.float32, device=x.device)
    L.check(L.lib().eg3d_u8_to_target(L.ptr(x), N, Hi, Wi, L.ptr(out), L.stream_ptr()), 'u8_to_target')
    return out


def _paste_inputs(what: str, photo, edits, matrix, region, feather_px, mask, layout):
    """The checks paste_back and paste_blend share: (photo [1,Hp,Wp,C], edits [N,S,S,C], squeeze, m, (x0, y0, x1, y1), feather_px, mask)."""
    ph, _ = _u8_images(photo, what + ' (photo)')
    x, squeeze = _u8_images(edits, what + ' (edits)')
    if photo.dim() != 3 or x.shape[-1] != ph.shape[-1] or x.shape[1] != x.shape[2] or x.device != ph.device:
        raise L.Eg3dHipError(f'{what}: one photo [Hp,Wp,C] and square edits [N,S,S,C] of the same C and device, got {tuple(photo.shape)} and '
                             f'{tuple(edits.shape)}')
    if layout not in ('hwc', 'chw'):
        raise L.Eg3dHipError(f"{what}: layout 'hwc' | 'chw', got {layout!r}")
    N, S, _, Ch = x.shape
    _, Hp, Wp, _ = ph.shape
    m = [float(v) for v in np.asarray(matrix, dtype=np.float64).reshape(-1)]
    x0, y0, x1, y1 = (int(v) for v in region)
    if len(m) != 6 or not (0 <= x0 <= x1 <= Wp and 0 <= y0 <= y1 <= Hp):
        raise L.Eg3dHipError(f'{what}: six matrix numbers and a region inside the {Wp} x {Hp} photo, got {len(m)} and {tuple(region)}')
    feather_px = float(feather_px)
    if not feather_px >= 0.0:
        raise L.Eg3dHipError(f'{what}: feather_px >= 0, got {feather_px}')
    mk = None
    if mask is not None:
        L.require_cuda(mask)
        if mask.dtype != torch.uint8 or tuple(mask.shape) not in ((S, S), (N, S, S)) or mask.device != ph.device:
            raise L.Eg3dHipError(f'{what}: mask uint8 [{S},{S}] or [{N},{S},{S}], got {tuple(mask.shape)} {mask.dtype}')
        mk = mask.contiguous()
    return ph, x, squeeze, m, (x0, y0, x1, y1), feather_px, mk


def paste_back(photo: torch.Tensor, edits: torch.Tensor, matrix, region, feather_px: float = 0.0, mask: Optional[torch.Tensor] = None,
               whole: bool = True, layout: str = 'hwc') -> torch.Tensor:
    """Edited aligned frames blended into their photograph on the device (eg3d_paste_back8; include/eg3d_hip.h states the arithmetic): photo
    uint8 [Hp,Wp,C], edits uint8 [N,S,S,C] (or [S,S,C]: the frame axis is dropped from the result too), C = 1 | 3; matrix = the six float64
    numbers m0..m5 of the affine map photo -> aligned frame (images.paste_plan); region = (x0, y0, x1, y1) inside the photo, the only pixels
    that are computed; feather_px = the width in aligned pixels over which the blend weight rises from the frame's edge (0: a hard edge);
    mask = uint8 [S,S] or [N,S,S] in the aligned frame, 255 = all of the edit.  whole=True gives the whole photograph per frame, [N,Hp,Wp,C]
    (two launches: the photo into every frame, then the region); whole=False the region alone, [N, y1 - y0, x1 - x0, C] (one launch).
    layout='chw' gives [N,C,H,W] instead, what jpeg_encode takes."""
    ph, x, squeeze, m, (x0, y0, x1, y1), feather_px, mk = _paste_inputs('paste_back', photo, edits, matrix, region, feather_px, mask, layout)
    N, S, _, Ch = x.shape
    _, Hp, Wp, _ = ph.shape
    Ho, Wo = (Hp, Wp) if whole else (y1 - y0, x1 - x0)
    out = torch.empty((N, Ch, Ho, Wo) if layout == 'chw' else (N, Ho, Wo, Ch), dtype=torch.uint8, device=ph.device)
    if out.numel() > 0:
        p = L.PasteBack8Params(photo=ph.data_ptr(), edits=x.data_ptr(), mask=mk.data_ptr() if mk is not None else None, dst=out.data_ptr(),
                               inv_feather=1.0 / feather_px if feather_px > 0.0 else 0.0, N=N, Hp=Hp, Wp=Wp, C=Ch, S=S, x0=x0, y0=y0, x1=x1, y1=y1,
                               mask_frames=N if (mk is not None and mk.dim() == 3) else 1, whole=int(bool(whole)),
                               layout=L.PASTE_CHW if layout == 'chw' else L.PASTE_HWC)
        p.m[:] = m
        L.check(L.lib().eg3d_paste_back8(C.byref(p), L.stream_ptr()), 'paste_back8')
    return out[0] if squeeze else out


def paste_blend_window(region, bands: int, Hp: int, Wp: int):
    """(wx0, wy0, wx1, wy1): the window eg3d_paste_blend8 works on -- the box grown by 2^(bands + 2) pixels and clamped to the photo."""
    x0, y0, x1, y1 = (int(v) for v in region)
    M = 1 << (int(bands) + 2)
    return max(x0 - M, 0), max(y0 - M, 0), min(x1 + M, Wp), min(y1 + M, Hp)


def paste_blend(photo: torch.Tensor, edits: torch.Tensor, matrix, region, bands: int, feather_px: float = 0.0,
                mask: Optional[torch.Tensor] = None, whole: bool = True, layout: str = 'hwc', return_levels: bool = False):
    """paste_back with a multi-band blend (eg3d_paste_blend8, csrc/blend.hip; include/eg3d_hip.h states the arithmetic): the difference
    edit - photo goes through a Laplacian pyramid of `bands` = 1..6 levels and every level is weighted by the blend weight reduced to it,
    over the window paste_blend_window gives.  The arguments and the result are paste_back's: whole=True writes the whole window into each
    photo copy; whole=False gives the region (the bounding box) alone and drops what the blend changes in the margin around it.
    An empty region gives what paste_back gives.  return_levels=True also returns the pyramid the kernels left in the workspace, a dict of
    fp32 tensors 'D' / 'alpha' (levels 1..bands: [N,C,h,w] / [N,h,w]) and 'R' (levels 1..bands - 1), each a list indexed by level - 1.
    The workspace is a torch allocation; no host synchronise."""
    ph, x, squeeze, m, (x0, y0, x1, y1), feather_px, mk = _paste_inputs('paste_blend', photo, edits, matrix, region, feather_px, mask, layout)
    if isinstance(bands, bool) or not isinstance(bands, (int, np.integer)) or not 1 <= int(bands) <= L.BLEND_MAX_BANDS:
        raise L.Eg3dHipError(f'paste_blend: bands an int in 1..{L.BLEND_MAX_BANDS}, got {bands!r}')
    bands = int(bands)
    N, S, _, Ch = x.shape
    _, Hp, Wp, _ = ph.shape
    Ho, Wo = (Hp, Wp) if whole else (y1 - y0, x1 - x0)
    out = torch.empty((N, Ch, Ho, Wo) if layout == 'chw' else (N, Ho, Wo, Ch), dtype=torch.uint8, device=ph.device)
    levels = dict(D=[], alpha=[], R=[])
    if out.numel() > 0:
        with torch.cuda.device(ph.device):
            p = L.PasteBlend8Params(photo=ph.data_ptr(), edits=x.data_ptr(), mask=mk.data_ptr() if mk is not None else None, dst=out.data_ptr(),
                                    inv_feather=1.0 / feather_px if feather_px > 0.0 else 0.0, N=N, Hp=Hp, Wp=Wp, C=Ch, S=S, x0=x0, y0=y0, x1=x1,
                                    y1=y1, mask_frames=N if (mk is not None and mk.dim() == 3) else 1, whole=int(bool(whole)),
                                    layout=L.PASTE_CHW if layout == 'chw' else L.PASTE_HWC, bands=bands)
            p.m[:] = m
            lib = L.lib()
            nbytes = C.c_int64(0)
            L.check(lib.eg3d_paste_blend8_query_workspace(C.byref(p), C.byref(nbytes)), 'paste_blend8_query_workspace')
            ws = torch.empty(max(nbytes.value // 4, 4), dtype=torch.float32, device=ph.device)
            p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
            L.check(lib.eg3d_paste_blend8(C.byref(p), L.stream_ptr()), 'paste_blend8')
        if return_levels and nbytes.value > 0:
            wx0, wy0, wx1, wy1 = paste_blend_window((x0, y0, x1, y1), bands, Hp, Wp)
            sizes, h, w = [], wy1 - wy0, wx1 - wx0
            for _ in range(bands):
                h, w = (h + 1) // 2, (w + 1) // 2
                sizes.append((h, w))
            at = 0
            for h, w in sizes:
                da = ws[at:at + N * (Ch + 1) * h * w].view(N, Ch + 1, h, w)
                levels['D'].append(da[:, :Ch])
                levels['alpha'].append(da[:, Ch])
                at += N * (Ch + 1) * h * w
            for h, w in sizes[:-1]:
                levels['R'].append(ws[at:at + N * Ch * h * w].view(N, Ch, h, w))
                at += N * Ch * h * w
    out = out[0] if squeeze else out
    return (out, levels) if return_levels else out


def edt2(mask_u8: torch.Tensor, thresholds=(), impl: str = 'auto') -> torch.Tensor:
    """Exact signed squared Euclidean distance transform on the device (eg3d_edt2; include/eg3d_hip.h "Head mattes" states it): mask_u8 uint8
    [N,H,W] (or [H,W]: the frame axis is dropped from the result too), foreground = nonzero -> int32 of the same shape, + the squared distance
    to the nearest background pixel of the frame at a foreground pixel, - the squared distance to the nearest foreground pixel at a background
    pixel, magnitude 2^28 where the frame has no pixel of the other class.  thresholds = up to 4 ints, the morphology stages: for each in
    order the binary image becomes sd2 > t and the transform runs again (erode by r: floor(r^2); dilate by r: -floor(r^2) - 1).
    impl = 'tiled' (any size up to 4096 a side, two launches per transform) | 'resident' (H W <= 16384: every stage in one launch) | 'auto'
    (the faster one as measured: 'tiled' at every size); all give the same integers.
    No host synchronise."""
    L.require_cuda(mask_u8)
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() not in (2, 3) or mask_u8.numel() == 0:
        raise L.Eg3dHipError(f'edt2: a non-empty uint8 mask [N,H,W] or [H,W], got {tuple(mask_u8.shape)} {mask_u8.dtype}')
    if impl not in L.EDT_IMPLS:
        raise L.Eg3dHipError(f"edt2: impl 'auto' | 'resident' | 'tiled', got {impl!r}")
    t = [int(v) for v in thresholds]
    if len(t) > L.EDT_MAX_STAGES or any(abs(v) >= 1 << 31 for v in t):
        raise L.Eg3dHipError(f'edt2: at most {L.EDT_MAX_STAGES} int32 thresholds, got {t}')
    squeeze = mask_u8.dim() == 2
    x = (mask_u8[None] if squeeze else mask_u8).contiguous()
    N, H, W = x.shape
    out = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        p = L.Edt2Params(src=x.data_ptr(), sd2=out.data_ptr(), N=N, H=H, W=W, n_stages=len(t), impl=L.EDT_IMPLS[impl])
        p.t[:len(t)] = t
        lib = L.lib()
        nbytes = C.c_int64(0)
        L.check(lib.eg3d_edt2_query_workspace(C.byref(p), C.byref(nbytes)), 'edt2_query_workspace')
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=x.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes.value
        L.check(lib.eg3d_edt2(C.byref(p), L.stream_ptr()), 'edt2')
    return out[0] if squeeze else out


def matte8(sd2: torch.Tensor, size, shrink_px: float = 0.0, feather_px: float = 0.0) -> torch.Tensor:
    """edt2's signed squared distances int32 [N,Hs,Ws] (or [Hs,Ws]) -> the soft matte uint8 [N,Ho,Wo] at size = (Ho, Wo) or one int for both
    (eg3d_matte8; the header states the eight fp64 steps): bilinear taps of the signed distance, whose zero lies half-way between a foreground
    and a background centre, so the edge is placed at sub-pixel precision; shrink_px moves it inwards (negative: outwards) and feather_px is
    the width of the smoothstep ramp that starts at it, both in output pixels (0: a hard edge).  The scale is one for both axes
    (Ho Ws == Wo Hs).  No host synchronise."""
    L.require_cuda(sd2)
    if sd2.dtype != torch.int32 or sd2.dim() not in (2, 3) or sd2.numel() == 0:
        raise L.Eg3dHipError(f'matte8: non-empty int32 distances [N,Hs,Ws] or [Hs,Ws], got {tuple(sd2.shape)} {sd2.dtype}')
    Ho, Wo = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    shrink_px, feather_px = float(shrink_px), float(feather_px)
    if not feather_px >= 0.0 or shrink_px != shrink_px:
        raise L.Eg3dHipError(f'matte8: feather_px >= 0 and a finite shrink_px, got {feather_px} and {shrink_px}')
    squeeze = sd2.dim() == 2
    x = (sd2[None] if squeeze else sd2).contiguous()
    N, Hs, Ws = x.shape
    if Ho < 1 or Wo < 1 or Ho * Ws != Wo * Hs:
        raise L.Eg3dHipError(f'matte8: a size >= 1 with the source\'s aspect ({Hs} x {Ws}), got {(Ho, Wo)}')
    if max(Ho, Wo) > L.MATTE_MAX_SIDE or N * Ho * Wo >= 1 << 31:                  # the library's limits, before the output is allocated
        raise L.Eg3dHipError(f'matte8: sides up to {L.MATTE_MAX_SIDE} and fewer than 2^31 output pixels, got {N} x {Ho} x {Wo}')
    out = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        p = L.Matte8Params(sd2=x.data_ptr(), dst=out.data_ptr(), step=float(Ws) / float(Wo), inv_step=float(Wo) / float(Ws), shrink_px=shrink_px,
                           inv_feather=1.0 / feather_px if feather_px > 0.0 else 0.0, N=N, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo)
        L.check(L.lib().eg3d_matte8(C.byref(p), L.stream_ptr()), 'matte8')
    return out[0] if squeeze else out
