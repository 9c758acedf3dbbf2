"""Fresh-interpreter helper of tests/test_gpu_mesh_texture.py: mesh_texture on the inputs of an .npz, printed as one JSON line of SHA-256
digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/support/mesh_digest.py does for the vertex bake."""
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
t = H.mesh_texture(dev('points'), dev('normals'), dev('faces'), dev('images'), dev('depth'), dev('mask'), dev('cams'), fallback=dev('fallback'),
                   tile=int(z['tile']), fill=int(z['fill']), depth_tol=float(z['depth_tol']), cos_min=float(z['cos_min']), power=int(z['power']))
out.update({k: sha(t[k]) for k in ('texture', 'views', 'uv', 'corner')})
print(json.dumps(out))
