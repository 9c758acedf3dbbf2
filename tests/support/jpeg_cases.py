"""The JPEG case list shared by tests/test_video_cpu.py (every restatement stream opens in PIL) and tests/test_gpu_video.py (the GPU bytes equal
the restatement's): name -> (uint8 image [C,H,W], quality, subsampling, restart interval | None).  Sizes are chosen for the paths of
csrc/jpeg.hip: one block, one 4:2:0 MCU, 1 x 1, both replicate paddings, an RSTm index that wraps, an interval that does not divide the MCU row,
grey, one full 512 x 512 frame; contents for EOB-only blocks, the longest codes with byte stuffing, and the largest amplitudes.  The restatement's
bytes are computed once per case and cached."""
import functools

import numpy as np

import jpeg_ref as J


def smooth(h=200, w=160, seed=0):
    """Band-limited noise: uniform noise through a separable Gaussian (sigma 4), stretched to 0..255."""
    rng = np.random.RandomState(seed)
    a = rng.rand(3, h + 24, w + 24)
    k = np.exp(-np.arange(-12, 13) ** 2 / 32.0)
    k /= k.sum()
    a = np.apply_along_axis(lambda r: np.convolve(r, k, 'valid'), 2, a)
    a = np.apply_along_axis(lambda r: np.convolve(r, k, 'valid'), 1, a)
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def noise(c, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (c, h, w)).astype(np.uint8)


def textured(h, w, seed):
    """smooth + uniform +-20 noise: a moderate number of non-zero coefficients per block."""
    s = smooth(h, w, seed).astype(np.int64)
    return np.clip(s + np.random.RandomState(seed + 1).randint(-20, 21, s.shape), 0, 255).astype(np.uint8)


def checkerboard(h, w):
    """Max-contrast one-pixel checkerboard, the three channels in phase: every block is one coefficient of the largest amplitude."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[None], 3, 0)


def binary_noise(h, w, seed):
    """Every sample 0 or 255 at random: large amplitudes in all 63 AC coefficients at quality 100 (the slots' worst case in practice)."""
    return (np.random.RandomState(seed).randint(0, 2, (3, h, w)) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # sizes (width x height as the issue writes them)
    c['one_block_444'] = (noise(3, 8, 8, 1), 90, '444', None)
    c['one_mcu_420'] = (noise(3, 16, 16, 2), 90, '420', None)
    c['1x1_420'] = (noise(3, 1, 1, 3), 90, '420', None)
    c['1x1_444'] = (noise(3, 1, 1, 3), 90, '444', None)
    for ss in ('420', '444'):
        c[f'17x23_{ss}'] = (textured(23, 17, 4), 90, ss, None)
        c[f'37x53_{ss}'] = (textured(53, 37, 5), 90, ss, None)
    c['24x160_r1'] = (textured(160, 24, 6), 90, '420', 1)                 # 2 x 10 MCUs, 20 intervals: RST0..7 wraps twice
    c['64x48_r3_420'] = (textured(48, 64, 7), 90, '420', 3)               # 4 MCUs per row
    c['64x48_r3_444'] = (textured(48, 64, 7), 90, '444', 3)               # 8 MCUs per row
    c['grey_20x12'] = (noise(1, 12, 20, 8), 90, '420', None)
    c['grey_37x53_r5'] = (textured(53, 37, 9)[:1], 75, '444', 5)
    c['frame_512'] = (textured(512, 512, 10), 90, '420', None)           # 32 x 32 MCUs, 32 intervals of 192 blocks
    # contents
    c['constant'] = (np.full((3, 40, 56), 77, np.uint8), 90, '420', None)
    c['noise_q100_444'] = (noise(3, 64, 96, 11), 100, '444', None)
    c['checkerboard_q100_444'] = (checkerboard(48, 64), 100, '444', None)
    c['checkerboard_q100_420'] = (checkerboard(48, 64), 100, '420', None)
    c['binary_noise_q100_444_r32'] = (binary_noise(32, 512, 12), 100, '444', 32)     # 64 MCUs per row, two intervals of 96 blocks each
    c['binary_noise_q100_420'] = (binary_noise(32, 512, 13), 100, '420', None)       # 32 MCUs per row: 192 blocks per interval
    for q in (50, 90, 100):
        for ss in ('420', '444'):
            c[f'textured_q{q}_{ss}'] = (textured(40, 72, 14), q, ss, None)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's file for a case (bytes)."""
    img, q, ss, r = cases()[name]
    return J.encode(img, quality=q, subsampling=ss, restart_interval=r)
