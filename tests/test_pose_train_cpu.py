"""CPU checks of the pose-estimator training path (inv3d_amd/pose_train.py) against tests/golden/pose_train.npz, which
tests/golden/make_golden_pose_train.py records from the reference's own sampler, loss and ResNet class in .train() mode."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import pose_net_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_SYMBOLS = ('eg3d_batchnorm_query_workspace', 'eg3d_batchnorm_forward', 'eg3d_batchnorm_backward')


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert torch.isfinite(a).all()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def test_pose_sampler_matches_reference(golden):
    from inv3d_amd.pose_train import poses_from_angles, sample_pseudo_poses
    d = golden('pose_train')
    ang, use_roll, want, tol = d['pose_angles'], d['pose_use_roll'], torch.from_numpy(d['pose_ext']), float(d['tol'])
    for i in range(len(ang)):
        yaw, pitch, roll = (float(v) for v in ang[i])
        got = poses_from_angles(torch.tensor([math.pi / 2 + yaw]), torch.tensor([math.pi / 2 + pitch]), torch.tensor([roll]), bool(use_roll[i]), radius=2.7)[0]
        assert float((got - want[i]).abs().max()) <= tol, (i, float((got - want[i]).abs().max()))
    # the batched sampler: the same function of its own angles, proper rotations, angles inside the requested ranges
    for ur in (False, True):
        g = torch.Generator().manual_seed(5)
        ext, a = sample_pseudo_poses(64, 0.2, 0.1, 0.2, ur, 2.7, g, return_angles=True)
        assert ext.shape == (64, 4, 4)
        again = poses_from_angles(math.pi / 2 + a[:, 0], math.pi / 2 + a[:, 1], a[:, 2], ur, 2.7)
        assert torch.equal(ext, again)
        R = ext[:, :3, :3]
        assert float((R.transpose(1, 2) @ R - torch.eye(3)).abs().max()) < 1e-5
        assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-5
        assert float(a[:, 0].abs().max()) <= math.pi * 0.1 and float(a[:, 1].abs().max()) <= math.pi * 0.05 and float(a[:, 2].abs().max()) <= math.pi * 0.1
        assert float(a[:, 0].std()) > 0.1 and float(a[:, 1].std()) > 0.05
        assert float((ext[:, :3, 3].norm(dim=1) - 2.7).abs().max()) < 1e-5          # on the sphere (re-derived from R with roll)
        assert float((ext[:, :3, 3] + 2.7 * R[:, :, 2]).abs().max()) < 1e-5         # looking at the origin
        assert torch.equal(ext[:, 3], torch.tensor([0., 0., 0., 1.]).expand(64, 4))
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert torch.equal(sample_pseudo_poses(8, generator=g1), sample_pseudo_poses(8, generator=g2))


@pytest.mark.parametrize('ct', ['4', '6', '2'])
def test_pose_training_loss_matches_reference(ct, golden):
    from inv3d_amd.pose_train import pose_training_loss
    d = golden('pose_train')
    pred, ext = torch.from_numpy(d[f'loss{ct}_pred']), torch.from_numpy(d[f'loss{ct}_ext'])
    loss, parts = pose_training_loss(pred, ext, ct, 2.7)
    for k in ('rot', 'trans', 'reg'):
        want = float(d[f'loss{ct}_{k}'])
        assert abs(float(parts[k]) - want) <= 1e-5 * max(abs(want), 1e-3), (k, float(parts[k]), want)
    assert abs(float(loss) - float(d[f'loss{ct}_total'])) <= 1e-5 * abs(float(d[f'loss{ct}_total']))
    with pytest.raises(ValueError):
        pose_training_loss(pred, ext, '3')


def test_trainable_net_train_mode_matches_reference_on_cpu(golden):
    """The CPU composite of hipops.batch_norm_train under TrainablePoseNet: output, loss, running statistics and gradients of the
    reference's resnet34(4).train() step."""
    from inv3d_amd.pose_train import pose_training_loss, resnet34_pose_trainable
    d = golden('pose_train')
    net = resnet34_pose_trainable(4)
    net.load_state_dict(PO.synth_state(seed=int(d['seed']), output_dims=4), strict=True)
    net.requires_grad_(True)
    net.train()
    assert net.training and net.bn1.training
    y = net(torch.from_numpy(d['net_img']))
    assert _rel(y, d['net_y']) < 1e-5
    loss, _ = pose_training_loss(y, torch.from_numpy(d['net_ext']), '4', 2.7)
    assert abs(float(loss) - float(d['net_loss'])) <= 1e-5 * abs(float(d['net_loss']))
    loss.backward()
    sd = net.state_dict()
    stat_keys = [k[len('net_stat.'):] for k in d.files if k.startswith('net_stat.')]
    assert len(stat_keys) == 6
    for k in stat_keys:
        assert _rel(sd[k], d[f'net_stat.{k}']) < 1e-5, k
    assert int(sd['bn1.num_batches_tracked']) == 1 and int(sd['layer4.2.bn2.num_batches_tracked']) == 1
    params = dict(net.named_parameters())
    n = 0
    for k in d.files:
        if k.startswith('net_g.'):
            assert _rel(params[k[6:]].grad, d[k]) < 2e-3, k
            n += 1
        elif k.startswith('net_gs.'):
            assert _rel(params[k[7:]].grad.flatten()[::97], d[k]) < 2e-3, k
            n += 1
    assert n >= 10


def test_state_dict_moves_between_the_classes_and_eval_matches_oracle():
    from inv3d_amd.pose_net import ResNetPose, resnet34_pose
    from inv3d_amd.pose_train import TrainablePoseNet, resnet34_pose_trainable
    sd = PO.synth_state(seed=3, output_dims=6)
    t = resnet34_pose_trainable(6)
    assert isinstance(t, TrainablePoseNet) and isinstance(t, ResNetPose) and not t.training
    assert list(t.state_dict().keys()) == list(resnet34_pose(6).state_dict().keys())
    assert set(t.state_dict()) == set(sd)
    t.load_state_dict(sd, strict=True)
    plain = resnet34_pose(6)
    plain.load_state_dict(t.state_dict(), strict=True)
    back = resnet34_pose_trainable(6)
    back.load_state_dict(plain.state_dict(), strict=True)
    for k, v in sd.items():
        assert torch.equal(back.state_dict()[k], v), k
    with pytest.raises(NotImplementedError):
        plain.train()
    t.train()
    assert t.training
    t.eval()
    assert not t.training
    img = torch.tanh(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))) * 100 + 128
    with torch.no_grad():
        assert _rel(t(img), PO.forward(sd, img)) < 1e-5


def test_batch_norm_train_cpu_composite():
    from inv3d_amd import hipops as H
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 8, 5, 5, generator=g) * 2 + 1
    res = torch.randn(3, 8, 5, 5, generator=g)
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    rm, rv, nbt = torch.zeros(8), torch.ones(8), torch.tensor(0)
    y = H.batch_norm_train(x, gamma, beta, rm, rv, nbt, 0.1, 1e-5, residual=res, act='relu')
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    want = torch.relu((x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + 1e-5) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1) + res)
    assert float((y - want).abs().max()) < 1e-5
    assert float((rm - 0.1 * mean).abs().max()) < 1e-6
    assert float((rv - (0.9 + 0.1 * x.var((0, 2, 3), unbiased=True))).abs().max()) < 1e-6
    assert int(nbt) == 1
    with pytest.raises(ValueError):
        H.batch_norm_train(x, gamma, beta, act='tanh')


def test_batchnorm_symbols_declared_and_exported_in_both_libraries():
    from inv3d_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'eg3d_hip.h')).read()
    declared = set(re.findall(r'\b(eg3d_[a-z0-9_]+)\s*\(', hdr))
    for name in BN_SYMBOLS:
        assert name in declared and name in L.EXPORTED_SYMBOLS, name
    assert 'eg3d_batchnorm_params' in hdr
    for so in ('libeg3d_hip.so', 'libeg3d_hip_det.so'):
        h = C.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), so))
        for name in BN_SYMBOLS:
            assert hasattr(h, name), (so, name)
    # host-side validation needs no device: the query refuses what the kernels cannot take
    q = L.lib().eg3d_batchnorm_query_workspace
    n = C.c_int64(0)
    assert q(1024, 64, C.byref(n)) == 0 and n.value >= 2 * 64 * 8
    assert q(1024, 66, C.byref(n)) == -1 and q(1, 64, C.byref(n)) == -1 and q(1024, 64, None) == -1


def test_batchnorm_struct_matches_the_header():
    import shutil
    import subprocess
    import tempfile
    from inv3d_amd import _lib as L
    cc = next((c for c in ('gcc', 'cc', 'clang', '/opt/rocm/llvm/bin/clang') if shutil.which(c)), None)
    if cc is None:
        pytest.skip('no C compiler')
    cls = L.BatchNormParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', ' printf("%zu\\n", sizeof(eg3d_batchnorm_params));']
    want = [C.sizeof(cls)]
    for f in cls._fields_:
        src.append(f' printf("%zu\\n", offsetof(eg3d_batchnorm_params, {f[0]}));')
        want.append(getattr(cls, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
