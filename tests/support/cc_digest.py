"""Fresh-interpreter helper of tests/test_gpu_grid_components.py: grid_components and grid_keep on the grids of an .npz, printed as one JSON
line of SHA-256 digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/support/mesh_digest.py does."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H, inference as INF  # noqa: E402

z = np.load(sys.argv[1])
sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()      # noqa: E731
out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
for name in sorted(k for k in z.files if k.startswith('vol_')):
    vol = torch.from_numpy(np.ascontiguousarray(z[name])).cuda()
    for conn in (6, 26):
        cc = H.grid_components(vol, float(z['level']), conn)
        kept = H.grid_keep(vol, cc['labels'], INF.select_components(cc['sizes'], keep=1))
        out[f'{name}/{conn}'] = [sha(cc['labels']), sha(cc['sizes']), sha(cc['roots']), cc['count'], cc['inside'], sha(kept)]
print(json.dumps(out))
