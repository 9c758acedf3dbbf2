"""numpy restatement of paste-back (csrc/imgprep.hip paste_back_kernel; include/eg3d_hip.h eg3d_paste_back8), the checker of
tests/test_paste_cpu.py and tests/test_gpu_paste.py:

  paste_matrix        the affine map photo -> aligned frame, built from images.align_plan on its own (np.linalg.solve on homogeneous 3 x 3
                      matrices, not images.paste_plan's closed form)
  paste8              the kernel's arithmetic: float64, every operation its own numpy statement in the header's order
  upright_landmarks   68 x 2 landmarks with given eye centre, eye-to-eye and eye-to-mouth vectors
  ramp_photo          the linear-ramp photograph of the round-trip check

Images are uint8 numpy arrays: photo [Hp,Wp,C], edits [N,S,S,C] or [S,S,C], mask [S,S] or [N,S,S]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))


def upright_landmarks(eye_avg, eye_to_eye, eye_to_mouth):
    """lm[36:42] = the left eye, lm[42:48] = the right eye, lm[48] = lm[54] = the mouth centre: all align_plan reads."""
    eye_avg, e2e, e2m = (np.asarray(v, dtype=np.float64) for v in (eye_avg, eye_to_eye, eye_to_mouth))
    lm = np.zeros((68, 2), np.float64)
    lm[36:42] = eye_avg - e2e * 0.5
    lm[42:48] = eye_avg + e2e * 0.5
    lm[48] = lm[54] = eye_avg + e2m
    return lm


EXACT_LANDMARKS = [upright_landmarks((50.5, 40.5), (16, 0), (0, 10)),          # identity + translation (photo 100 x 100, S = 64)
                   upright_landmarks((50.5, 50.5), (0, 16), (-10, 0)),         # a quarter turn
                   upright_landmarks((50.5, 60.5), (-16, 0), (0, -10))]        # a half turn


def paste_matrix(height, width, landmarks, output_size):
    """(m0..m5, region): photo -> aligned frame as the product of the forward steps' homogeneous matrices, inverted by a linear solve."""
    from inv3d_amd.hipops import pil_quad_coeffs
    from inv3d_amd.images import align_plan
    S = int(output_size)
    plan = align_plan(height, width, landmarks, S)
    a = pil_quad_coeffs((S, S), plan.quad)
    fwd = np.eye(3)                                                        # photo -> the image the QUAD warp reads
    if plan.shrink_size is not None:
        fwd = np.diag([plan.shrink_size[0] / width, plan.shrink_size[1] / height, 1.0]) @ fwd
    if plan.crop is not None:
        fwd = np.array([[1.0, 0, -plan.crop[0]], [0, 1.0, -plan.crop[1]], [0, 0, 1.0]]) @ fwd
    if plan.pad is not None:
        fwd = np.array([[1.0, 0, plan.pad[0]], [0, 1.0, plan.pad[1]], [0, 0, 1.0]]) @ fwd
    quad = np.array([[a[1], a[2], a[0]], [a[5], a[6], a[4]], [0, 0, 1.0]])  # aligned frame -> that image
    M = np.linalg.solve(quad, fwd)
    inv = np.linalg.inv(M)                                                 # aligned frame -> photo
    corners = inv @ np.array([[0, 0, S, S], [0, S, S, 0], [1.0, 1, 1, 1]])
    region = (int(np.clip(np.floor(corners[0].min()), 0, width)), int(np.clip(np.floor(corners[1].min()), 0, height)),
              int(np.clip(np.ceil(corners[0].max()), 0, width)), int(np.clip(np.ceil(corners[1].max()), 0, height)))
    return np.array([M[0, 2], M[0, 0], M[0, 1], M[1, 2], M[1, 0], M[1, 1]]), region


def _taps(u, v, S):
    xin, yin = u - 0.5, v - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = xin - fx, yin - fy
    xa, xb = np.clip(fx, 0, S - 1).astype(np.int64), np.clip(fx + 1, 0, S - 1).astype(np.int64)
    ya, yb = np.clip(fy, 0, S - 1).astype(np.int64), np.clip(fy + 1, 0, S - 1).astype(np.int64)
    return xa, xb, ya, yb, dx, dy


def _bilinear(img, taps):
    """img float64 [S,S,C]; quad_warp8's r0 / r1 / v order, not truncated."""
    xa, xb, ya, yb, dx, dy = taps
    dx, dy = dx[..., None], dy[..., None]
    r0 = img[ya, xa] + (img[ya, xb] - img[ya, xa]) * dx
    r1 = img[yb, xa] + (img[yb, xb] - img[yb, xa]) * dx
    return r0 + (r1 - r0) * dy


def paste8(photo, edits, matrix, region, feather_px=0.0, mask=None, whole=True, return_alpha=False):
    """The header's arithmetic.  Returns [N,...] (or one frame for [S,S,C] edits); with return_alpha also the blend weight a [N,rh,rw] of the
    region (0 outside the aligned frame)."""
    photo, edits = np.asarray(photo), np.asarray(edits)
    squeeze = edits.ndim == 3
    if squeeze:
        edits = edits[None]
    N, S, _, C = edits.shape
    m = [np.float64(v) for v in np.asarray(matrix, dtype=np.float64).reshape(6)]
    x0, y0, x1, y1 = region
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
    out = np.repeat(photo[None], N, 0) if whole else np.empty((N, y1 - y0, x1 - x0, C), np.uint8)
    alphas = np.zeros((N, y1 - y0, x1 - x0))
    for n in range(N):
        a = a0
        if mask is not None:
            mk = np.asarray(mask)
            mk = (mk if mk.ndim == 2 else mk[n]).astype(np.float64)[..., None]
            a = a * (_bilinear(mk, taps)[..., 0] * inv255)
        val = _bilinear(edits[n].astype(np.float64), taps)
        r = np.rint(ph + (val - ph) * a[..., None])                        # np.rint: half to even
        r = np.where(inside[..., None], np.clip(r, 0.0, 255.0), ph).astype(np.uint8)
        if whole:
            out[n, y0:y1, x0:x1] = r
        else:
            out[n] = r
        alphas[n] = np.where(inside, a, 0.0)
    out = out[0] if squeeze else out
    return (out, alphas) if return_alpha else out


def ramp_photo(height, width):
    """channels 10 + 235 x / W, 10 + 235 y / H, 10 + 117 (x / W + y / H), rounded to uint8."""
    y, x = np.mgrid[:height, :width].astype(np.float64)
    img = np.stack([10 + 235 * x / width, 10 + 235 * y / height, 10 + 117 * (x / width + y / height)], -1)
    return np.rint(img).astype(np.uint8)
