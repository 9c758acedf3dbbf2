"""Fresh-interpreter helper of tests/test_gpu_mesh.py: marching cubes of a grid saved with np.save, printed as one JSON line (counts and
SHA-256 of the vertex / face bytes) -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/test_gpu_det.py does."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402

grid = torch.from_numpy(np.load(sys.argv[1])).cuda()
out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
for level in sys.argv[2:]:
    v, f = H.marching_cubes(grid, float(level))
    out[level] = [v.shape[0], f.shape[0], hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(f.cpu().numpy().tobytes()).hexdigest()]
print(json.dumps(out))
