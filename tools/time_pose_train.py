#!/usr/bin/env python3
"""Device-event timings of the pose-estimator training path (inv3d_amd/pose_train.py, csrc/batchnorm.hip).

    python tools/time_pose_train.py [--batch 32] [--windows 5] [--iters 20] [--out FILE.json]
    python tools/time_pose_train.py --profile DIR        # kernel counts of one trainer step from a rocprofv3 --kernel-trace --stats run

(a) hipops.batch_norm_train forward and forward+backward at the estimator's layer shapes, against torch.nn.functional.batch_norm(training=True)
    (+ add + relu where the HIP op fuses them) on the same channels-last tensors;
(b) one whole PoseEstimatorTrainer step at 256^2 against the same step in plain torch ops on the same GPU (torch convs, torch BatchNorm,
    torch.optim.Adam), both fed the same pre-rendered batch;
(c) the PseudoPoseStream rate in images/s (full-size synthetic generator unless --small).
Every figure is the median over `--windows` windows of `--iters` back-to-back iterations between two device events, after a warm-up window."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CL = torch.channels_last
# (name, C, H = W at 256^2 input, residual, act)
LAYERS = (('stem bn1', 64, 128, False, 'relu'), ('layer1 bn1', 64, 64, False, 'relu'), ('layer1 bn2+add+relu', 64, 64, True, 'relu'),
          ('layer2 bn1', 128, 32, False, 'relu'), ('layer2 bn2+add+relu', 128, 32, True, 'relu'), ('layer2 downsample', 128, 32, False, 'linear'),
          ('layer3 bn1', 256, 16, False, 'relu'), ('layer3 bn2+add+relu', 256, 16, True, 'relu'),
          ('layer4 bn1', 512, 8, False, 'relu'), ('layer4 bn2+add+relu', 512, 8, True, 'relu'))


def timed(fn, windows, iters):
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), min(ms), max(ms)


def bench_bn(batch, windows, iters):
    from inv3d_amd import hipops as H
    rows = []
    for name, c, hw, with_res, act in LAYERS:
        g = torch.Generator().manual_seed(c + hw)
        x = torch.randn(batch, c, hw, hw, generator=g).cuda().contiguous(memory_format=CL).requires_grad_(True)
        res = torch.randn(batch, c, hw, hw, generator=g).cuda().contiguous(memory_format=CL).requires_grad_(True) if with_res else None
        dy = torch.randn(batch, c, hw, hw, generator=g).cuda().contiguous(memory_format=CL)
        gamma, beta = torch.ones(c, device='cuda', requires_grad=True), torch.zeros(c, device='cuda', requires_grad=True)
        rm, rv, nbt = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda'), torch.zeros((), dtype=torch.int64, device='cuda')
        ins = [t for t in (x, gamma, beta, res) if t is not None]

        def hip_f():
            return H.batch_norm_train(x, gamma, beta, rm, rv, nbt, 0.1, 1e-5, residual=res, act=act)

        def torch_f():
            y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
            if res is not None:
                y = y + res
            return torch.relu(y) if act == 'relu' else y

        def fb(f):
            return lambda: torch.autograd.grad(f(), ins, dy)
        with torch.no_grad():
            hf, tf = timed(hip_f, windows, iters), timed(torch_f, windows, iters)
        hb, tb = timed(fb(hip_f), windows, iters), timed(fb(torch_f), windows, iters)
        mb = batch * c * hw * hw * 4 / 1e6
        rows.append(dict(layer=name, C=c, M=batch * hw * hw, MB=round(mb, 2), hip_fwd_us=round(hf[0] * 1e3, 1), torch_fwd_us=round(tf[0] * 1e3, 1),
                         hip_fwdbwd_us=round(hb[0] * 1e3, 1), torch_fwdbwd_us=round(tb[0] * 1e3, 1),
                         fwd_speedup=round(tf[0] / hf[0], 2), fwdbwd_speedup=round(tb[0] / hb[0], 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def torch_resnet34(dims):
    """The same network from torch modules (torch convs, torch BatchNorm): the plain-torch step of comparison (b)."""
    from inv3d_amd.pose_train import resnet34_pose_trainable

    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = resnet34_pose_trainable(dims)

        def forward(self, img):
            n = self.net
            x = F.relu(n.bn1(n.conv1(img)))
            x = F.max_pool2d(x, 3, 2, 1)
            for layer in (n.layer1, n.layer2, n.layer3, n.layer4):
                for blk in layer:
                    out = F.relu(blk.bn1(blk.conv1(x)))
                    idn = x if blk.downsample is None else blk.downsample(x)
                    x = F.relu(blk.bn2(blk.conv2(out)) + idn)
            return n._head(x)
    return Plain()


def bench_step(batch, windows, iters, small):
    from inv3d_amd.pose_train import PoseEstimatorTrainer, PseudoPoseStream, pose_training_loss, resnet34_pose_trainable
    G = make_generator(small)
    stream = PseudoPoseStream(G, batch, seed=0)
    img, ext = stream.next()
    torch.manual_seed(0)
    net = resnet34_pose_trainable(4).cuda()
    tr = PoseEstimatorTrainer(G, net, batch_size=batch, camera_type='4')
    hip = timed(lambda: tr.step((img, ext)), windows, iters)
    plain = torch_resnet34(4).cuda().to(memory_format=CL).train()
    torch.nn.Module.train(plain.net, True)
    opt = torch.optim.Adam(plain.parameters(), lr=1e-4, fused=True)
    img_cl = img.contiguous(memory_format=CL)

    def torch_step():
        loss, _ = pose_training_loss(plain(img_cl), ext, '4', 2.7)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    tt = timed(torch_step, windows, iters)
    rate = timed(stream.next, windows, max(2, iters // 4))
    return dict(batch=batch, hip_step_ms=round(hip[0], 3), hip_step_ms_range=[round(hip[1], 3), round(hip[2], 3)], torch_step_ms=round(tt[0], 3),
                torch_step_ms_range=[round(tt[1], 3), round(tt[2], 3)], step_speedup=round(tt[0] / hip[0], 3),
                stream_images_per_s=round(batch / rate[0] * 1e3, 1), stream_generator='small synthetic' if small else 'full-size synthetic (512^2 output)')


def make_generator(small):
    from inv3d_amd import synthetic as S
    if small:
        from oracle import eg3d_oracle as O
        G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                             rendering_kwargs=O.small_config().rendering, device='cuda')
    else:
        G = S.make_generator(device='cuda')
    S.load_synthetic_weights(G, 0)
    return G


def profile(out_dir, batch):
    """One rocprofv3 --kernel-trace --stats run of a fresh child process that does a few trainer steps; returns calls per kernel name per step."""
    os.makedirs(out_dir, exist_ok=True)
    steps = 4
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out_dir, '-o', 'pose_train', '--output-format', 'csv', '--', sys.executable, os.path.abspath(__file__),
           '--child-steps', str(steps), '--batch', str(batch), '--small']
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=900)
    import csv
    import glob
    counts = {}
    for f in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        for row in csv.DictReader(open(f)):
            counts[row['Name']] = dict(calls=int(row['Calls']), total_us=round(float(row['TotalDurationNs']) / 1e3, 1))
    return dict(steps=steps, kernels=counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--small', action='store_true', help='small synthetic generator for the stream (the estimator and its 256^2 input stay full size)')
    ap.add_argument('--out')
    ap.add_argument('--profile', metavar='DIR')
    ap.add_argument('--child-steps', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_steps:
        from inv3d_amd.pose_train import PoseEstimatorTrainer, PseudoPoseStream, resnet34_pose_trainable
        G = make_generator(a.small)
        tr = PoseEstimatorTrainer(G, resnet34_pose_trainable(4).cuda(), batch_size=a.batch, camera_type='4')
        batch = PseudoPoseStream(G, a.batch, seed=0).next()
        for _ in range(a.child_steps):
            tr.step(batch)
        torch.cuda.synchronize()
        return
    res = {}
    if a.profile:
        res['profile'] = profile(a.profile, a.batch)
    else:
        res['batch_norm'] = bench_bn(a.batch, a.windows, a.iters)
        res['step'] = bench_step(a.batch, a.windows, max(3, a.iters // 4), a.small)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
