"""Fresh-interpreter helper of tests/test_gpu_pose_train.py: hipops.batch_norm_train forward and backward on seeded inputs, printed as one JSON
line of SHA-256 digests -- run with EG3D_DETERMINISTIC=1 to use the deterministic build, the way tests/test_gpu_det.py does."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CL = torch.channels_last


def inputs(dev, shape=(3, 128, 29, 31), seed=13):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = (torch.randn(shape, generator=g) * 1.7 + 0.4).to(dev).contiguous(memory_format=CL)
    res = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=CL)
    dy = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=CL)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    return x, res, dy, gamma, beta


def run(x, res, dy, gamma, beta):
    from inv3d_amd import hipops as H
    c = x.shape[1]
    out = {}
    for act, r in (('relu', res), ('linear', None)):
        xs, gs, bs = x.clone(memory_format=CL).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rs = r.clone(memory_format=CL).requires_grad_(True) if r is not None else None
        rm, rv, nbt = torch.zeros(c, device=x.device), torch.ones(c, device=x.device), torch.zeros((), dtype=torch.int64, device=x.device)
        y, save = H.batch_norm_train(xs, gs, bs, rm, rv, nbt, 0.1, 1e-5, residual=rs, act=act, return_stats=True)
        y.backward(dy)
        torch.cuda.synchronize()
        ts = dict(y=y, save=save, rm=rm, rv=rv, nbt=nbt, dx=xs.grad, dg=gs.grad, db=bs.grad)
        if rs is not None:
            ts['dres'] = rs.grad
        for k, t in ts.items():
            out[f'{act}.{k}'] = hashlib.sha256(t.detach().contiguous(memory_format=CL if t.dim() == 4 else torch.contiguous_format).cpu().numpy().tobytes()).hexdigest()
    return out


if __name__ == '__main__':
    from inv3d_amd import _lib as L
    res = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    res.update(run(*inputs('cuda')))
    print(json.dumps(res))
