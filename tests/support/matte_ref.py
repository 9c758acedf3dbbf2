"""numpy restatement of the head-matte kernels (csrc/matte.hip; include/eg3d_hip.h "Head mattes"), the checker of tests/test_matte_cpu.py (which
pins it against scipy) and tests/test_gpu_matte.py (integer and byte equality with the device).

  edt2(mask, thresholds)                     column sweeps, then a brute-force row minimum over every x' (no early stop), with the stages
  matte8(sd2, size, shrink_px, feather_px)   the header's eight numbered steps in float64, one rounded numpy operation each
  stage_thresholds / matte_from_mask         images.matte_from_mask's radius -> threshold conversion and chain, restated"""
import math

import numpy as np

SENT = 1 << 14


def _column_distance(present):
    """[H,W] bool -> int64 [H,W]: per column, the distance |y - y'| to the nearest True of that column, SENT where it has none."""
    H, W = present.shape
    g = np.full((H, W), SENT, dtype=np.int64)
    d = np.full(W, SENT, dtype=np.int64)
    for y in range(H):                                     # down sweep
        d = np.where(present[y], 0, np.minimum(d + 1, SENT))
        g[y] = d
    d = np.full(W, SENT, dtype=np.int64)
    for y in range(H - 1, -1, -1):                         # up sweep
        d = np.where(present[y], 0, np.minimum(d + 1, SENT))
        g[y] = np.minimum(g[y], d)
    return g


def _edt2_frame(fg):
    H, W = fg.shape
    g_fg, g_bg = _column_distance(fg), _column_distance(~fg)
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                                       # [x, x']
    out = np.empty((H, W), dtype=np.int64)
    rows = max(1, (1 << 22) // (W * W))                                        # a few rows at a time: the [rows, x, x'] table stays small
    for y in range(0, H, rows):
        to_bg = (dx2[None] + (g_bg[y:y + rows] ** 2)[:, None, :]).min(axis=2)  # [rows, x]
        to_fg = (dx2[None] + (g_fg[y:y + rows] ** 2)[:, None, :]).min(axis=2)
        out[y:y + rows] = np.where(fg[y:y + rows], to_bg, -to_fg)
    return out


def edt2(mask, thresholds=()):
    """mask [N,H,W] or [H,W] (foreground = nonzero) -> int32 signed squared distances; for each threshold in order the binary image becomes
    sd2 > t and the transform runs again."""
    m = np.asarray(mask)
    frames = m[None] if m.ndim == 2 else m
    out = np.empty(frames.shape, dtype=np.int32)
    for n in range(frames.shape[0]):
        sd2 = _edt2_frame(frames[n] != 0)
        for t in thresholds:
            sd2 = _edt2_frame(sd2 > int(t))
        out[n] = sd2
    return out[0] if m.ndim == 2 else out


def matte8(sd2, size, shrink_px=0.0, feather_px=0.0):
    """sd2 int32 [N,Hs,Ws] or [Hs,Ws] -> uint8 at size = (Ho, Wo) (or one int for both), the header's steps 1..8 in float64."""
    s = np.asarray(sd2)
    frames = s[None] if s.ndim == 2 else s
    N, Hs, Ws = frames.shape
    Ho, Wo = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    assert Ho * Ws == Wo * Hs
    step, inv_step = np.float64(Ws) / np.float64(Wo), np.float64(Wo) / np.float64(Ws)
    shrink_px = np.float64(shrink_px)
    inv_feather = np.float64(1.0) / np.float64(feather_px) if feather_px > 0 else np.float64(0.0)

    def axis(n_out, n_src):
        u = (np.arange(n_out, dtype=np.float64) + 0.5) * step - 0.5            # 1
        f = np.floor(u)                                                        # 2
        i = f.astype(np.int64)
        return u - f, np.clip(i, 0, n_src - 1), np.clip(i + 1, 0, n_src - 1)
    dx, xa, xb = axis(Wo, Ws)
    dy, ya, yb = axis(Ho, Hs)
    f64 = frames.astype(np.float64)
    d = np.where(frames > 0, np.sqrt(np.abs(f64)) - 0.5, -(np.sqrt(np.abs(f64)) - 0.5))      # 3
    p00, p01 = d[:, ya][:, :, xa], d[:, ya][:, :, xb]
    p10, p11 = d[:, yb][:, :, xa], d[:, yb][:, :, xb]
    dxb, dyb = dx[None, None, :], dy[None, :, None]
    r0 = p00 + (p01 - p00) * dxb                                               # 4
    r1 = p10 + (p11 - p10) * dxb
    val = r0 + (r1 - r0) * dyb
    e = val * inv_step - shrink_px                                             # 5
    if inv_feather > 0:                                                        # 6
        t = np.minimum(np.maximum(e * inv_feather, 0.0), 1.0)
    else:
        t = np.where(e > 0, 1.0, 0.0)
    a = (t * t) * (3.0 - 2.0 * t)                                              # 7
    out = np.rint(255.0 * a).astype(np.uint8)                                  # 8
    return out[0] if s.ndim == 2 else out


def stage_thresholds(side, open=0.02, close=0.04):
    """images.matte_from_mask's thresholds for a source of `side` rows: open = erode, dilate; close = dilate, erode; a zero radius drops
    its two stages.  r = frac * side in float64; erode t = floor(r^2), dilate t = -floor(r^2) - 1."""
    t = []
    for frac, first_erodes in ((open, True), (close, False)):
        r = float(frac) * side
        if r > 0.0:
            q = int(math.floor(r * r))
            t += [q, -q - 1] if first_erodes else [-q - 1, q]
    return tuple(t)


def matte_from_mask(mask, size, open=0.02, close=0.04, shrink=0.0, feather=0.03):
    m = np.asarray(mask)
    Hs = m.shape[-2]
    return matte8(edt2(m, stage_thresholds(Hs, open, close)), size, shrink_px=float(shrink) * size, feather_px=float(feather) * size)
