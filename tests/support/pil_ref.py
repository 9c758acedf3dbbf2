"""numpy restatements of the image-ingestion kernels (csrc/imgprep.hip; include/eg3d_hip.h "Image ingestion"), the checkers of
tests/test_align_cpu.py and tests/test_gpu_align.py:

  resize8        Pillow's 8-bit separable resize on the integer tables of hipops.pil_resize_coeffs (horizontal, then vertical, uint8 between)
  quad_warp8     Image.transform(size, QUAD, data, BILINEAR), fill 0: fp64 in Pillow's operation order, truncating store
  feather_pad    the pad branch of the reference's align_face (utils/alignment.py:95-105) in fp32, in the kernels' summation order
  scipy_pad      the same branch as the reference states it (scipy.ndimage.gaussian_filter, np.median): what feather_pad is bounded against
  align_face     inv3d_amd.images.align_face's host geometry driven through the three restatements

Images are uint8 [H,W,C] numpy arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))


def _pass8(img, bounds, coef, axis):
    """One pass along `axis` (0 = vertical, 1 = horizontal): acc = 2^21 + sum pixel * k in int32, clip(acc >> 22, 0, 255)."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for o, (lo, cnt) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(coef[o, :cnt].astype(np.int64), src[lo:lo + cnt], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize8(img, size, filter):
    from inv3d_amd.hipops import pil_resize_coeffs
    wo, ho = size
    h, w = img.shape[:2]
    if wo != w:
        img = _pass8(img, *pil_resize_coeffs(w, wo, filter), axis=1)
    if ho != h:
        img = _pass8(img, *pil_resize_coeffs(h, ho, filter), axis=0)
    return np.ascontiguousarray(img)


def quad_warp8(img, size, quad):
    from inv3d_amd.hipops import pil_quad_coeffs
    wo, ho = size
    h, w = img.shape[:2]
    a = pil_quad_coeffs(size, quad)
    xi = (np.arange(wo, dtype=np.float64) + 0.5)[None, :]
    yi = (np.arange(ho, dtype=np.float64) + 0.5)[:, None]
    xin = a[0] + a[1] * xi + a[2] * yi + a[3] * xi * yi
    yin = a[4] + a[5] * xi + a[6] * yi + a[7] * xi * yi
    inside = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    x0, x1 = np.clip(fx, 0, w - 1).astype(np.int64), np.clip(fx + 1, 0, w - 1).astype(np.int64)
    y0, y1 = np.clip(fy, 0, h - 1).astype(np.int64), np.clip(fy + 1, 0, h - 1).astype(np.int64)
    p = img.astype(np.float64)
    r0 = p[y0, x0] + (p[y0, x1] - p[y0, x0]) * dx
    r1 = p[y1, x0] + (p[y1, x1] - p[y1, x0]) * dx
    v = r0 + (r1 - r0) * dy
    return np.where(inside[..., None], v, 0.0).astype(np.uint8)              # astype truncates; v is within [0, 255]


def pad_mask(h, w, pads):
    """The reference's mask (alignment.py:99-101) for a padded image of h x w, in float64."""
    left, top, right, bottom = pads
    y, x, _ = np.ogrid[:h, :w, :1]
    return np.maximum(1.0 - np.minimum(np.float32(x) / np.int64(left), np.float32(w - 1 - x) / np.int64(right)),
                      1.0 - np.minimum(np.float32(y) / np.int64(top), np.float32(h - 1 - y) / np.int64(bottom)))


def scipy_pad(img, pads, qsize):
    """alignment.py:97-105 as the reference states it; pads = (left, top, right, bottom)."""
    import scipy.ndimage
    left, top, right, bottom = pads
    img = np.pad(np.float32(img), ((top, bottom), (left, right), (0, 0)), 'reflect')
    h, w, _ = img.shape
    mask = pad_mask(h, w, pads)
    blur = qsize * 0.02
    img += (scipy.ndimage.gaussian_filter(img, [blur, blur, 0]) - img) * np.clip(mask * 3.0 + 1.0, 0.0, 1.0)
    img += (np.median(img, axis=(0, 1)) - img) * np.clip(mask, 0.0, 1.0)
    return np.uint8(np.clip(np.rint(img), 0, 255))


def _blur32(p, g, axis):
    """Symmetric-boundary correlation along `axis` in fp32, the kernels' order: g[0] p, then += g[k] (p[-k] + p[+k]) for k = 1 .. radius."""
    n, r = p.shape[axis], len(g) - 1
    idx = np.arange(-r, n + r)
    idx = np.mod(idx, 2 * n)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)                             # numpy 'symmetric' = scipy 'reflect'
    e = np.take(p, idx, axis=axis)
    sl = lambda k: np.take(e, np.arange(r + k, r + k + n), axis=axis)
    acc = g[0] * sl(0)
    for k in range(1, r + 1):
        acc = acc + g[k] * (sl(-k) + sl(k))
    assert acc.dtype == np.float32
    return acc


def feather_pad(img, pads, qsize):
    from inv3d_amd.hipops import gauss_weights
    left, top, right, bottom = pads
    g = gauss_weights(qsize * 0.02).astype(np.float32)
    p = np.pad(np.float32(img), ((top, bottom), (left, right), (0, 0)), 'reflect')
    h, w, _ = p.shape
    y, x, _ = np.ogrid[:h, :w, :1]
    one = np.float32(1.0)
    mask = np.maximum(one - np.minimum(np.float32(x) / np.float32(left), np.float32(w - 1 - x) / np.float32(right)),
                      one - np.minimum(np.float32(y) / np.float32(top), np.float32(h - 1 - y) / np.float32(bottom)))
    assert mask.dtype == np.float32
    blur = _blur32(_blur32(p, g, 0), g, 1)
    v = p + (blur - p) * np.clip(mask * np.float32(3.0) + one, 0, 1)
    med = np.median(v, axis=(0, 1)).astype(np.float32)
    v = v + (med - v) * np.clip(mask, 0, 1)
    assert v.dtype == np.float32
    return np.uint8(np.clip(np.rint(v), 0, 255))


def align_face(img, landmarks, output_size):
    """images.align_face's geometry (align_plan) with every pixel step done by the restatements above."""
    from inv3d_amd.images import align_plan
    plan = align_plan(img.shape[0], img.shape[1], landmarks, output_size)
    if plan.shrink_size is not None:
        img = resize8(img, plan.shrink_size, 'lanczos')
    if plan.crop is not None:
        x0, y0, x1, y1 = plan.crop
        img = img[y0:y1, x0:x1]
    if plan.pad is not None:
        img = feather_pad(img, plan.pad, plan.qsize)
    return quad_warp8(img, (output_size, output_size), plan.quad)
