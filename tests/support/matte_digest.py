"""Fresh-interpreter helper of tests/test_gpu_matte.py: SHA-256 of what the head-matte kernels (csrc/matte.hip: hipops.edt2, hipops.matte8,
images.matte_from_mask) give for a few fixed inputs, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic build,
the way tests/support/paste_digest.py does.  The kernels have no atomics and no sum across threads: the two builds must agree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H, images  # noqa: E402


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    rs = np.random.RandomState(23)
    for name, (n, h, w, density) in dict(small=(2, 33, 130, 0.1), resident=(3, 128, 128, 0.6), tiled=(1, 128, 129, 0.5)).items():
        m = torch.from_numpy((rs.random_sample((n, h, w)) < density).astype(np.uint8)).cuda()
        for impl in ('auto', 'tiled') + (('resident',) if h * w <= 16384 else ()):
            out[f'edt2_{name}_{impl}'] = _sha(H.edt2(m, (2, -3, -10, 9), impl=impl))
    m = torch.from_numpy((rs.random_sample((2, 64, 64)) < 0.7).astype(np.uint8)).cuda()
    sd2 = H.edt2(m)
    out['matte8'] = _sha(H.matte8(sd2, 150, shrink_px=0.75, feather_px=4.5))
    out['matte8_hard'] = _sha(H.matte8(sd2, (96, 96)))
    out['chain'] = _sha(images.matte_from_mask(m, 256))
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
