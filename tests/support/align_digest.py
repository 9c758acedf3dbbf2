"""Fresh-interpreter helper of tests/test_gpu_align.py: SHA-256 of what the image-ingestion entries (csrc/imgprep.hip) give for a few fixed
inputs, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/support/jpeg_digest.py does.
The file holds integer atomics only and no floating-point sum across threads: the two builds must agree."""
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
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.randint(0, 256, (2, 37, 53, 3), dtype=np.uint8)).cuda()
    out['resize_lanczos'] = _sha(H.pil_resize(x, (16, 11), 'lanczos'))
    out['resize_bilinear_up'] = _sha(H.pil_resize(x, (130, 61), 'bilinear'))
    out['quad'] = _sha(H.pil_quad_warp(x, (24, 20), (3.7, 2.2, -4.5, 35.1, 50.3, 44.9, 60.2, -3.5)))
    out['feather_pad'] = _sha(H.feather_pad(x, (12, 20, 7, 31), 80))
    out['u8_to_target'] = _sha(H.u8_to_target(x))
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'align.npz'), allow_pickle=False)
    for name in ('pad_corner_rotated', 'shrink_pad'):
        out['align_' + name] = _sha(images.align_face(torch.from_numpy(z[name + '.image']).cuda(), z[name + '.landmarks'], int(z[name + '.output_size'])))
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
