"""Fresh-interpreter helper of tests/test_gpu_mesh_raster.py: mesh_raster on the inputs of an .npz in its three modes, printed as one JSON line
of SHA-256 digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/support/texture_digest.py does for the atlas."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402

OUTPUTS = ('image', 'face', 'z', 'depth', 'mask', 'bary')
z = np.load(sys.argv[1])
dev = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).cuda()      # noqa: E731
out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
for mode in ('texture', 'vertex', 'lambert'):
    t = H.mesh_raster(dev('points'), dev('faces'), dev('cams'), int(z['res']), mode=mode, uv=dev('uv'), texture=dev('texture'), colors=dev('colors'),
                      normals=dev('normals'), cull=str(z['cull']))
    h = hashlib.sha256()
    for k in OUTPUTS:
        h.update(np.ascontiguousarray(t[k].cpu().numpy()).tobytes())
    out[mode] = h.hexdigest()
print(json.dumps(out))
