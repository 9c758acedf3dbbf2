"""Fresh-interpreter helper of tests/test_gpu_video.py: SHA-256 of the bytes and offsets hipops.jpeg_encode gives for a few cases of
tests/support/jpeg_cases.py and for one fp32 batch, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic build,
the way tests/support/pca_digest.py does.  csrc/jpeg.hip holds no floating-point sum and no global atomic: the two builds must agree."""
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
import jpeg_cases as JC  # noqa: E402

NAMES = ('37x53_420', '64x48_r3_444', 'grey_20x12', 'noise_q100_444', 'binary_noise_q100_420')


def _sha(data, offsets):
    return hashlib.sha256(data.cpu().numpy().tobytes() + offsets.numpy().tobytes()).hexdigest()


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    for name in NAMES:
        img, q, ss, r = JC.cases()[name]
        out[name] = _sha(*H.jpeg_encode(torch.from_numpy(img)[None].cuda(), quality=q, subsampling=ss, restart_interval=r))
    x = torch.from_numpy(np.random.RandomState(5).uniform(-1.2, 1.2, (3, 3, 45, 70)).astype(np.float32)).cuda()
    out['fp32_batch'] = _sha(*H.jpeg_encode(x, quality=75))
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
