"""numpy restatement of the multi-band paste-back (csrc/blend.hip; include/eg3d_hip.h eg3d_paste_blend8), the checker of
tests/test_blend_cpu.py and tests/test_gpu_blend.py:

  reduce2 / expand2   one pyramid step on float32 arrays [..., h, w]: zero extension, rows first, then columns, the header's 1-D formulas
  collapse            D [..., h, w] and alpha (broadcast against it) -> R_0 and the levels
  window              the box grown by 2^(bands + 2) and clamped to the photo
  level0              D and alpha of a window: paste_ref's float64 steps (the same taps and order), then one rounding to float32
  blend8              the whole entry: uint8 frames as hipops.paste_blend gives them

Every float32 operation is its own numpy statement on float32 arrays, so it is rounded on its own, in the header's order; numpy keeps
float32 subnormals, and so do the kernels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paste_ref import _bilinear, _taps  # noqa: E402

F = np.float32


def reduce1(x):
    """Along the last axis: r[i] = (((x[2i-2] + x[2i+2]) + 4 (x[2i-1] + x[2i+1])) + 6 x[2i]) / 16, zeros outside, ceil(n / 2) outputs."""
    n = x.shape[-1]
    m = (n + 1) // 2
    p = np.zeros(x.shape[:-1] + (2 * m + 4,), F)
    p[..., 2:2 + n] = x

    def t(k):
        return p[..., 2 + k:2 + k + 2 * m:2]
    return (((t(-2) + t(2)) + F(4) * (t(-1) + t(1))) + F(6) * t(0)) * F(1 / 16)


def reduce2(x):
    return np.swapaxes(reduce1(np.swapaxes(reduce1(x), -1, -2)), -1, -2)


def expand1(x, n):
    """Along the last axis to n outputs: even 2j: ((x[j-1] + x[j+1]) + 6 x[j]) / 8, odd 2j + 1: (x[j] + x[j+1]) / 2, zeros outside."""
    m = x.shape[-1]
    assert (n + 1) // 2 == m
    p = np.zeros(x.shape[:-1] + (m + 2,), F)
    p[..., 1:1 + m] = x
    out = np.zeros(x.shape[:-1] + (2 * m,), F)
    out[..., 0::2] = ((p[..., 0:m] + p[..., 2:m + 2]) + F(6) * p[..., 1:m + 1]) * F(1 / 8)
    out[..., 1::2] = (p[..., 1:m + 1] + p[..., 2:m + 2]) * F(0.5)
    return out[..., :n]


def expand2(x, h, w):
    return np.swapaxes(expand1(np.swapaxes(expand1(x, w), -1, -2), h), -1, -2)


def collapse(D, alpha, bands, return_levels=False):
    """R_0 of the header for float32 D [..., h, w] and alpha broadcastable against it."""
    D, alpha = np.asarray(D, F), np.asarray(alpha, F)
    Ds, As = [D], [alpha]
    for _ in range(bands):
        Ds.append(reduce2(Ds[-1]))
        As.append(reduce2(As[-1]))
    Rs = [None] * bands + [Ds[bands] * As[bands]]
    for k in range(bands - 1, -1, -1):
        h, w = Ds[k].shape[-2:]
        Rs[k] = (Ds[k] - expand2(Ds[k + 1], h, w)) * As[k] + expand2(Rs[k + 1], h, w)
    return (Rs[0], dict(D=Ds, alpha=As, R=Rs)) if return_levels else Rs[0]


def window(region, bands, Hp, Wp):
    x0, y0, x1, y1 = region
    M = 1 << (bands + 2)
    return max(x0 - M, 0), max(y0 - M, 0), min(x1 + M, Wp), min(y1 + M, Hp)


def level0(photo, edits, matrix, win, feather_px=0.0, mask=None):
    """(D float32 [N,C,wh,ww], alpha float32 [N,1,wh,ww]) of the window: paste_ref.paste8's float64 steps up to val and a."""
    N, S, _, C = edits.shape
    m = [np.float64(v) for v in np.asarray(matrix, dtype=np.float64).reshape(6)]
    x0, y0, x1, y1 = win
    inv_feather = np.float64(1.0 / feather_px) if feather_px > 0 else np.float64(0.0)
    inv255 = np.float64(1.0) / np.float64(255.0)
    Xc = (np.arange(x0, x1, dtype=np.float64) + 0.5)[None, :]
    Yc = (np.arange(y0, y1, dtype=np.float64) + 0.5)[:, None]
    u = m[0] + m[1] * Xc + m[2] * Yc
    v = m[3] + m[4] * Xc + m[5] * Yc
    Sd = np.float64(S)
    with np.errstate(invalid='ignore'):
        inside = (u >= 0.0) & (u < Sd) & (v >= 0.0) & (v < Sd)
    u, v = np.where(inside, u, 0.5), np.where(inside, v, 0.5)
    taps = _taps(u, v, S)
    d = np.minimum(np.minimum(u, Sd - u), np.minimum(v, Sd - v))
    f = np.minimum(d * inv_feather, 1.0) if inv_feather > 0 else np.ones_like(d)
    a0 = (f * f) * (3.0 - 2.0 * f)
    ph = photo[y0:y1, x0:x1].astype(np.float64)
    D = np.zeros((N, C, y1 - y0, x1 - x0), F)
    A = np.zeros((N, 1, y1 - y0, x1 - x0), F)
    for n in range(N):
        a = a0
        if mask is not None:
            mk = np.asarray(mask)
            mk = (mk if mk.ndim == 2 else mk[n]).astype(np.float64)[..., None]
            a = a * (_bilinear(mk, taps)[..., 0] * inv255)
        val = _bilinear(edits[n].astype(np.float64), taps)
        D[n] = np.where(inside[..., None], (val - ph).astype(F), F(0)).transpose(2, 0, 1)
        A[n, 0] = np.where(inside, a.astype(F), F(0))
    return D, A


def blend8(photo, edits, matrix, region, bands, feather_px=0.0, mask=None, whole=True, return_levels=False):
    """The header's arithmetic.  Returns [N,...] (or one frame for [S,S,C] edits) as paste_ref.paste8 does: the photo per frame with the
    window written (whole) or the box alone; with return_levels also the dict of levels (lists indexed by level, 0 included)."""
    photo, edits = np.asarray(photo), np.asarray(edits)
    squeeze = edits.ndim == 3
    if squeeze:
        edits = edits[None]
    N, _, _, C = edits.shape
    Hp, Wp = photo.shape[:2]
    x0, y0, x1, y1 = region
    out = np.repeat(photo[None], N, 0) if whole else np.empty((N, y1 - y0, x1 - x0, C), np.uint8)
    levels = None
    if x1 > x0 and y1 > y0:
        win = window(region, bands, Hp, Wp)
        wx0, wy0, wx1, wy1 = win
        D, A = level0(photo, edits, matrix, win, feather_px, mask)
        R0, levels = collapse(D, A, bands, return_levels=True)
        ph = photo[wy0:wy1, wx0:wx1].astype(F).transpose(2, 0, 1)[None]
        r = np.clip(np.rint(ph + R0), F(0), F(255)).astype(np.uint8).transpose(0, 2, 3, 1)
        if whole:
            out[:, wy0:wy1, wx0:wx1] = r
        else:
            out[:] = r[:, y0 - wy0:y1 - wy0, x0 - wx0:x1 - wx0]
    out = out[0] if squeeze else out
    return (out, levels) if return_levels else out
