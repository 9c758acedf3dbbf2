"""The decoder's case list, shared by tests/test_jpeg_decode_cpu.py (the restatement equals PIL) and tests/test_gpu_jpeg_decode.py (the device
equals both): name -> the bytes of a JPEG file.  Every file is made by an encoder -- PIL's writer (quality, subsampling 0 / 1 / 2 = 4:4:4 /
4:2:2 / 4:2:0, optimize, restart_marker_blocks / restart_marker_rows) or this project's own restatement jpeg_ref.encode (always restart-coded)
-- never from hand-made coefficients, so that libjpeg-turbo's SIMD and C paths agree on them.  Sizes are width x height.

  geometry   1x1, one block, one 4:2:0 MCU, odd sizes, several MCUs, in the three samplings; grey; down-sampled widths 1, 2 (replication) and
             3 (the first fancy-upsampled width), down-sampled heights 1 and 2
  content    constant (EOB-only blocks: many blocks per subsequence), uniform and binary noise at quality 100 (longest codes, largest amplitudes,
             many stuffed FF 00), textured at quality 50 / 90, optimize=True (tables that are not Annex K's, codes far beyond the 9-bit lookup; Annex K's own 16-bit
             codes are what the noise cases use), quality 1 - 5 (ZRL)
  restarts   interval 1 over twelve segments (RSTm wraps), an interval that does not divide the MCU row, one MCU row, the project's encoder
  sync       one 256 x 192 quality-100 noise file without restarts: ~1000 subsequences of 128 bytes, several workgroups

The PIL decode and the restatement's decode of a case are computed once and cached; treat them as read-only."""
import functools
import io

import numpy as np

import jpeg_cases as JC
import jpeg_ref
import jpegdec_ref

SUBSEQ = (16, 128)                       # every case is decoded at both subsequence sizes
BIG = 'noise_q100_256x192'


def pil_file(img_chw, quality, subsampling=None, **kw):
    from PIL import Image
    a = np.ascontiguousarray(np.transpose(img_chw, (1, 2, 0)))
    im = Image.fromarray(a[:, :, 0], 'L') if a.shape[2] == 1 else Image.fromarray(a, 'RGB')
    buf = io.BytesIO()
    if subsampling is not None:
        kw['subsampling'] = subsampling
    im.save(buf, 'JPEG', quality=quality, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for i, (w, h) in enumerate(((1, 1), (8, 8), (16, 16), (9, 17), (17, 23), (37, 53), (40, 72))):
        for ss, name in ((0, '444'), (1, '422'), (2, '420')):
            c[f'{w}x{h}_{name}'] = pil_file(JC.textured(h, w, 20 + i) if min(w, h) > 1 else JC.noise(3, h, w, 20 + i), 90, ss)
    c['grey_20x12'] = pil_file(JC.noise(1, 12, 20, 30), 90)
    for w, h in ((2, 5), (5, 2), (3, 3), (4, 9), (5, 9), (6, 4)):
        c[f'{w}x{h}_420'] = pil_file(JC.noise(3, h, w, 31 + w + h), 95, 2)
    c['4x9_422'] = pil_file(JC.noise(3, 9, 4, 40), 95, 1)
    c['5x3_422'] = pil_file(JC.noise(3, 3, 5, 41), 95, 1)
    c['constant_420'] = pil_file(np.full((3, 40, 56), 77, np.uint8), 90, 2)
    c['constant_444_200x64'] = pil_file(np.full((3, 64, 200), 200, np.uint8), 75, 0)
    c['noise_q100_444'] = pil_file(JC.noise(3, 48, 64, 42), 100, 0)
    c['noise_q100_422'] = pil_file(JC.noise(3, 48, 64, 43), 100, 1)
    c['binary_noise_q100_420'] = pil_file(JC.binary_noise(48, 64, 44), 100, 2)
    c['binary_noise_q100_444'] = pil_file(JC.binary_noise(40, 56, 45), 100, 0)
    for q in (50, 90):
        for ss, name in ((0, '444'), (2, '420')):
            c[f'textured_q{q}_{name}'] = pil_file(JC.textured(40, 72, 46), q, ss)
    c['optimize_37x53_420'] = pil_file(JC.textured(53, 37, 47), 90, 2, optimize=True)
    c['optimize_noise_q100_444'] = pil_file(JC.noise(3, 40, 56, 48), 100, 0, optimize=True)
    c['optimize_128x128_q98_444'] = pil_file(JC.textured(128, 128, 70), 98, 0, optimize=True)            # its own tables reach 15-bit codes
    c['optimize_grey'] = pil_file(JC.textured(53, 37, 49)[:1], 80, optimize=True)
    for q in (1, 3, 5):
        c[f'textured_q{q}_420'] = pil_file(JC.textured(72, 40, 50 + q), q, 2)
    c['restart1_64x48_420'] = pil_file(JC.textured(48, 64, 60), 90, 2, restart_marker_blocks=1)          # 12 MCUs, 12 segments: RST0..7, RST0..2
    c['restart3_64x48_444'] = pil_file(JC.textured(48, 64, 61), 90, 0, restart_marker_blocks=3)          # 8 MCUs per row
    c['restart5_70x50_422'] = pil_file(JC.textured(50, 70, 62), 85, 1, restart_marker_blocks=5)          # 5 MCUs per row, 7 rows
    c['restart_row_72x40_420'] = pil_file(JC.textured(40, 72, 63), 90, 2, restart_marker_rows=1)
    c['restart1_grey_noise_q100'] = pil_file(JC.noise(1, 24, 40, 64), 100, restart_marker_blocks=1)
    c['own_37x53_420'] = jpeg_ref.encode(JC.textured(53, 37, 65), quality=90, subsampling='420')
    c['own_64x48_r3_444'] = jpeg_ref.encode(JC.textured(48, 64, 66), quality=90, subsampling='444', restart_interval=3)
    c['own_grey_20x12'] = jpeg_ref.encode(JC.noise(1, 12, 20, 67), quality=90)
    c['own_binary_noise_q100_420'] = jpeg_ref.encode(JC.binary_noise(32, 96, 68), quality=100, subsampling='420')
    c[BIG] = pil_file(JC.noise(3, 192, 256, 69), 100, 0)
    return c


@functools.lru_cache(maxsize=None)
def pil_decode(name):
    """uint8 [H,W,3]: PIL.Image.open(file).convert('RGB')"""
    from PIL import Image
    with Image.open(io.BytesIO(cases()[name])) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def ref_decode(name):
    """uint8 [H,W,3]: the restatement"""
    return jpegdec_ref.decode(cases()[name])
