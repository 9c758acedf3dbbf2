"""Fresh-interpreter helper of tests/test_gpu_ganspace.py: SHA-256 digests of the covariance, mean, eigenvalues, eigenvectors and one image
grid that csrc/pca.hip computes for fixed seeded inputs, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the deterministic
build, the way tests/support/mc_digest.py does.  Nothing in that translation unit accumulates with atomics: the two builds must agree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digests():
    rng = np.random.RandomState(21)
    x = torch.from_numpy((rng.randn(1500, 70) * 0.9 ** np.arange(70) * (1 + 50)).astype(np.float32)).cuda()
    x = x + 50 * 0.9 ** torch.arange(70, device='cuda', dtype=torch.float32)
    st = None
    for lo, hi in ((0, 300), (300, 1001), (1001, 1500)):
        st = H.pca_moments(x[lo:hi], x[:256].mean(0), st)
    cov, mean, n = H.pca_covariance(st)
    evals, evecs, sweeps, converged = H.sym_eig(cov)
    img = torch.from_numpy(rng.randn(5, 3, 9, 6).astype(np.float32)).cuda()
    grid = H.image_grid_u8(img, nrow=3)
    torch.cuda.synchronize()
    return dict(deterministic_build=bool(L.lib().eg3d_det_enabled()), n=n, sweeps=sweeps, converged=converged, cov=_sha(cov), mean=_sha(mean),
                evals=_sha(evals), evecs=_sha(evecs), grid=_sha(grid))


if __name__ == '__main__':
    print(json.dumps(digests()))
