#!/usr/bin/env python3
"""Pose-estimator-training fixture generator (tests/golden/pose_train.npz).  Runs on the CPU of a development machine with a checkout of the
reference (cvlab-kaist/3DGAN-Inversion):

    python tests/golden/make_golden_pose_train.py REFERENCE_ROOT

Records, from the reference's own code:
  * utils.camera_utils.LookAt3DPoseSampler.sample for a handful of (yaw, pitch, roll, use_roll) tuples (the pseudo-dataset poses of
    scripts/gen_pseudo_dataset.py:169-177);
  * compute_geodesic_loss and the trainer's whole loss expression (scripts/train_pose_estimator.py:117-141), lifted from the script by AST
    (the script itself imports tensorboard and opens a URL), for recorded pred / ext_gt batches of the three camera types ('2' at batch 1:
    the reference's own branch does not run at any other);
  * the reference resnet34(output_dims=4) in .train() mode with the weights of oracle/pose_net_oracle.synth_state (never stored) on a seeded
    [4,3,64,64] batch: output, loss, running statistics of three BatchNorm layers after the step, parameter gradients (strided where large).
The same computation is repeated in float64; the fp32-vs-fp64 error of every quantity is printed, and the share of parameter tensors whose
fp32 gradient misses the fp64 one by more than the GPU test's tolerance (2e-3 of the tensor's largest entry) has to be 0.
The reference's helpers call .cuda(); that is made the identity for this process, as make_golden.py does."""
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED, DIMS, TOL, GRAD_TOL = 3, 4, 2e-6, 2e-3
POSES = ((0.0, 0.0, 0.0, False), (0.21, -0.07, 0.0, False), (-0.3, 0.15, 0.1, False), (0.12, 0.05, 0.25, True), (-0.28, -0.11, -0.3, True),
         (0.0, 0.0, 0.31, True))
STAT_LAYERS = ('bn1', 'layer2.0.downsample.1', 'layer4.2.bn2')
GRAD_KEYS = ('conv1.weight', 'bn1.weight', 'bn1.bias', 'layer1.0.conv2.weight', 'layer1.2.bn2.weight', 'layer2.0.downsample.0.weight',
             'layer2.0.downsample.1.weight', 'layer3.2.bn1.bias', 'layer4.2.conv1.weight', 'layer4.2.bn2.bias', 'fc.weight', 'fc3.weight', 'fc3.bias')

torch.Tensor.cuda = lambda self, *a, **k: self


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(1e-30, float(b.double().abs().max())))


class _fp64:
    """Run the reference's helpers in float64: they build their constants with torch.eye / torch.ones / torch.FloatTensor."""

    def __enter__(self):
        self.ft = torch.FloatTensor
        torch.set_default_dtype(torch.float64)
        torch.FloatTensor = lambda v: torch.tensor(v, dtype=torch.float64)

    def __exit__(self, *exc):
        torch.FloatTensor = self.ft
        torch.set_default_dtype(torch.float32)


def _randn(tag, shape, dtype=torch.float32):
    g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(tag)) * 7919 + SEED)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)


def lift_loss(ref_root):
    """(compute_geodesic_loss, loss_fn(pred, ext_batch, camera_type, bs) -> dict of the loop's loss terms) from the trainer script."""
    tree = ast.parse(open(os.path.join(ref_root, 'scripts', 'train_pose_estimator.py')).read())
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('compute_geodesic')]
    main = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'main'][0]
    loop = [n for n in ast.walk(main) if isinstance(n, ast.For) and 'dataset_loader' in ast.unparse(n.iter)][0]
    first = [i for i, n in enumerate(loop.body) if isinstance(n, ast.If) and 'camera_type' in ast.unparse(n.test)][0]
    last = [i for i, n in enumerate(loop.body) if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == 'loss'][0]
    fn = ast.parse('def loss_fn(pred, ext_batch, camera_type, bs, radius):\n    pass\n    return dict(loss=loss, rot_loss=rot_loss, trans_loss=trans_loss, '
                   'reg_loss=reg_loss, pred_ext=pred_ext)').body[0]
    fn.body = loop.body[first:last + 1] + fn.body[1:]
    mod = ast.Module(body=funcs + [fn], type_ignores=[])
    ast.fix_missing_locations(mod)
    from utils.camera_utils import compute_rotation_matrix_from_quaternion, euler2rot, rot6d_to_rotmat
    ns = dict(torch=torch, math=math, nn=torch.nn, F=torch.nn.functional, euler2rot=euler2rot, rot6d_to_rotmat=rot6d_to_rotmat,
              compute_rotation_matrix_from_quaternion=compute_rotation_matrix_from_quaternion)
    exec(compile(mod, 'train_pose_estimator_lifted', 'exec'), ns)
    return ns['compute_geodesic_loss'], ns['loss_fn']


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, 'scripts'))
    sys.path.insert(0, ref_root)
    sys.path.insert(0, ROOT)
    from utils.camera_utils import LookAt3DPoseSampler
    from resnet import resnet as ref_resnet
    from oracle import pose_net_oracle as PO
    geo_loss, loss_fn = lift_loss(ref_root)
    out = dict(seed=np.int64(SEED), tol=np.float32(TOL))

    # ---- the sampler
    pivot = torch.zeros(3)
    ext = []
    for yaw, pitch, roll, use_roll in POSES:
        e = LookAt3DPoseSampler.sample(np.pi / 2 + yaw, np.pi / 2 + pitch, torch.tensor([roll]), pivot, radius=2.7, device='cpu', use_roll=use_roll)
        ext.append(e.reshape(4, 4))
    ext = torch.stack(ext)
    out['pose_angles'] = np.asarray([p[:3] for p in POSES], np.float64)
    out['pose_use_roll'] = np.asarray([p[3] for p in POSES], np.bool_)
    out['pose_ext'] = ext.numpy()
    print('sampler: |R^T R - 1| max', float((ext[:, :3, :3].transpose(1, 2) @ ext[:, :3, :3] - torch.eye(3)).abs().max()))

    # ---- the loss, three camera types
    for ct, bs in (('4', 4), ('6', 4), ('2', 1)):
        pred = torch.tanh(_randn(f'pred{ct}', (bs, int(ct))) * (0.2 if ct == '2' else 0.8))
        if ct == '4':
            pred = pred + torch.tensor([0., 1., 0., 0.])          # about the canonical quaternion
        if ct == '6':
            pred = pred * 0.3 + torch.tensor([1., 0., 0., 0., -1., 0.])
        gt = ext[[1, 2, 3, 4]][:bs]
        r32 = loss_fn(pred, gt, ct, bs, 2.7)
        r64 = None          # ('2': euler2rot's helper builds an explicitly fp32 up vector -- no float64 run)
        if ct != '2':
            with _fp64():
                r64 = loss_fn(pred.double(), gt.double(), ct, bs, 2.7)
        g = geo_loss(r32['pred_ext'][:, :3, :3], gt[:, :3, :3])
        assert float((g - r32['rot_loss']).abs()) == 0
        out.update({f'loss{ct}_pred': pred.numpy(), f'loss{ct}_ext': gt.numpy(), f'loss{ct}_rot': r32['rot_loss'].numpy(), f'loss{ct}_trans': r32['trans_loss'].numpy(),
                    f'loss{ct}_reg': r32['reg_loss'].numpy(), f'loss{ct}_total': r32['loss'].numpy()})
        print(f'loss type {ct}: total {float(r32["loss"]):.6f} rot {float(r32["rot_loss"]):.6f} trans {float(r32["trans_loss"]):.3e} reg {float(r32["reg_loss"]):.3e}',
              '' if r64 is None else f'fp32-vs-fp64 {abs(float(r32["loss"]) - float(r64["loss"])):.2e}')

    # ---- the network in training mode, fp32 and fp64: the first of a fixed list of seeded inputs on which the reference's fp32 gradients all
    # agree with its own fp64 ones (no ReLU / max-pool routing flip between the two precisions)
    gt = ext[[1, 2, 3, 4]]
    for cand in range(16):
        img = ((torch.tanh(_randn(f'img{cand}', (4, 3, 64, 64))) * 0.5 + 0.5) * 255).float()
        res = {}
        for dt in (torch.float32, torch.float64):
            net = ref_resnet.resnet34(output_dims=DIMS)
            net.load_state_dict(PO.synth_state(seed=SEED, output_dims=DIMS), strict=True)
            net = net.to(dt).train()
            y = net(img.to(dt))
            if dt == torch.float64:
                with _fp64():
                    r = loss_fn(y, gt.to(dt), '4', 4, 2.7)
            else:
                r = loss_fn(y, gt.to(dt), '4', 4, 2.7)
            r['loss'].backward()
            sd = net.state_dict()
            res[dt] = dict(y=y.detach(), loss=r['loss'].detach(), grads={k: p.grad.detach() for k, p in net.named_parameters()},
                           stats={f'{l}.{s}': sd[f'{l}.{s}'].clone() for l in STAT_LAYERS for s in ('running_mean', 'running_var')},
                           nbt=int(sd['bn1.num_batches_tracked']))
        a, b = res[torch.float32], res[torch.float64]
        errs = {k: _rel(a['grads'][k], b['grads'][k]) for k in a['grads']}
        share = sum(e > GRAD_TOL for e in errs.values()) / len(errs)
        print(f'input candidate {cand}: worst gradient fp32-vs-fp64 {max(errs.values()):.2e}; share above {GRAD_TOL}: {share:.3f}')
        if share == 0:
            break
    print('train-mode output fp32-vs-fp64', _rel(a['y'], b['y']), 'loss', abs(float(a['loss']) - float(b['loss'])))
    for k in a['stats']:
        print(f'  {k}: fp32-vs-fp64 {_rel(a["stats"][k], b["stats"][k]):.2e}')
    for k in GRAD_KEYS:
        print(f'  grad {k}: fp32-vs-fp64 {errs[k]:.2e}')
    assert share == 0, 'choose another input'
    assert a['nbt'] == 1
    out.update(net_candidate=np.int64(cand), net_img=img.numpy(), net_ext=gt.numpy(), net_y=a['y'].numpy(), net_loss=a['loss'].numpy())
    for k, v in a['stats'].items():
        out[f'net_stat.{k}'] = v.numpy()
    for k in GRAD_KEYS:
        g = a['grads'][k]
        if g.numel() <= 40000:
            out[f'net_g.{k}'] = g.numpy()
        else:
            out[f'net_gs.{k}'] = g.flatten()[::97].clone().numpy()
    path = os.path.join(HERE, 'pose_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
