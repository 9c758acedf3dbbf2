"""Fresh-interpreter helper of tests/test_gpu_png.py: SHA-256 of the bytes and offsets hipops.png_encode gives for a few cases of
tests/support/png_cases.py and for one batch, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way
tests/support/jpeg_digest.py does.  csrc/png.hip holds no floating point and no global atomic: the two builds must agree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402
import png_cases as PC  # noqa: E402
import png_ref as P  # noqa: E402

NAMES = ('rgb_37x53_bb1024', 'winners_adaptive', 'fibonacci_limiter', 'sevens_300x300_bb1000', 'noise_rgb_64x64')


def _sha(data, offsets):
    return hashlib.sha256(data.cpu().numpy().tobytes() + offsets.numpy().tobytes()).hexdigest()


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    for name in NAMES:
        img, filt, bb = PC.cases()[name]
        out[name] = _sha(*H.png_encode(torch.from_numpy(img).cuda(), filter=filt, block_bytes=bb))
    batch = np.stack([P.image(45, 70, s, 2 * s) for s in range(3)])
    out['batch'] = _sha(*H.png_encode(torch.from_numpy(batch).cuda(), block_bytes=2048))
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
