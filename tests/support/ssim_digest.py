"""Fresh-interpreter helper of tests/test_gpu_metrics.py: MS-SSIM and its gradients on seeded inputs, printed as one JSON line of SHA-256
digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/test_gpu_det.py does."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def inputs(dev):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 257, 300, generator=g)
    y = (x + 0.2 * torch.randn(2, 3, 257, 300, generator=g))
    return x.to(dev), y.to(dev)


def run(x, y):
    from inv3d_amd.metrics import ms_ssim, ssim
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    v = ms_ssim(xs, ys, data_range=1, size_average=False)
    s = ssim(xs, ys, data_range=1)
    (v.sum() + s).backward()
    torch.cuda.synchronize()
    return {k: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest() for k, t in (('v', v), ('s', s), ('gx', xs.grad), ('gy', ys.grad))}


if __name__ == '__main__':
    from inv3d_amd import _lib as L
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    out.update(run(*inputs('cuda')))
    print(json.dumps(out))
