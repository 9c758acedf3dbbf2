"""Fresh-interpreter helper of tests/test_gpu_mesh_color.py: mesh_normals and mesh_bake on the inputs of an .npz, printed as one JSON line of
SHA-256 digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/support/mc_digest.py does for marching cubes."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402

z = np.load(sys.argv[1])
dev = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).cuda()      # noqa: E731
sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()      # noqa: E731
out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
out['normals'] = sha(H.mesh_normals(dev('vol'), dev('pts'), z['origin'].tolist(), z['spacing'].tolist(), [int(a) for a in z['axes']]))
b = H.mesh_bake(dev('points'), dev('normals'), dev('images'), dev('depth'), dev('mask'), dev('cams'), fallback=dev('fallback'),
                depth_tol=float(z['depth_tol']), cos_min=float(z['cos_min']), power=int(z['power']))
out.update({k: sha(b[k]) for k in ('color', 'rgb', 'weight', 'views')})
print(json.dumps(out))
