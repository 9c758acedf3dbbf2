"""Fresh-interpreter helper of tests/test_gpu_blend.py: SHA-256 of what the multi-band paste-back (csrc/blend.hip eg3d_paste_blend8,
images.paste_back(bands=...)) gives for a few fixed inputs, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic
build, the way tests/support/paste_digest.py does.  The kernels have no atomics and no sum across threads: the two builds must agree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inv3d_amd import _lib as L, hipops as H, images  # noqa: E402
import paste_ref as P  # noqa: E402


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    rs = np.random.RandomState(19)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'align.npz'), allow_pickle=False)
    for name in ('pad_corner_rotated', 'shrink'):
        photo, lm, S = z[name + '.image'], z[name + '.landmarks'], int(z[name + '.output_size'])
        edits = torch.from_numpy(rs.randint(0, 256, (2, S, S, 3), dtype=np.uint8)).cuda()
        mask = torch.from_numpy(rs.randint(0, 256, (2, S, S), dtype=np.uint8)).cuda()
        plan = images.paste_plan(photo.shape[0], photo.shape[1], lm, S)
        ph = torch.from_numpy(photo).cuda()
        whole, levels = H.paste_blend(ph, edits, plan.matrix, plan.region, 3, 0.08 * S, mask, return_levels=True)
        out['hwc_' + name] = _sha(whole)
        out['levels_' + name] = [_sha(t) for key in ('D', 'alpha', 'R') for t in levels[key]]
        out['chw_region_' + name] = _sha(H.paste_blend(ph, edits, plan.matrix, plan.region, 1, 0.0, None, whole=False, layout='chw'))
        out['images_' + name] = _sha(images.paste_back(ph, edits, lm, mask=mask[0], region='bbox', bands='auto'))
    photo = torch.from_numpy(rs.randint(0, 256, (100, 100, 3), dtype=np.uint8)).cuda()
    edits = torch.from_numpy(rs.randint(0, 256, (1, 128, 128, 3), dtype=np.uint8)).cuda()
    out['minified'] = _sha(images.paste_back(photo, edits, P.EXACT_LANDMARKS[1], bands=2))
    out['grey'] = _sha(H.paste_blend(photo[..., :1], edits[..., :1], (3.25, 0.7, -0.2, -8.5, 0.2, 0.7), (5, 7, 93, 99), 4, 11.0))
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
