#!/usr/bin/env python3
"""Train the pose estimator of a generator on its own renderings (inv3d_amd/pose_train.py): the reference's gen_pseudo_dataset.py +
train_pose_estimator.py as one GPU loop, no files in between.

    python tools/train_pose_estimator.py --network G.pt --camera-type 4 --steps 20000 --batch 32 --out-dir runs/pose_ffhq
    python tools/train_pose_estimator.py --synthetic small --steps 100 --out-dir runs/pose_smoke

--network: a generator archive as inv3d_amd.weights.load_generator reads it; --synthetic full|small: a seeded synthetic generator.
Writes OUT/model_best.pt (best validation score), OUT/model_last.pt and OUT/log.json; both checkpoints load with
`inv3d_amd.pose_net.resnet34_pose(int(camera_type)).load_state_dict`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--network')
    src.add_argument('--synthetic', choices=['full', 'small'])
    ap.add_argument('--camera-type', choices=['2', '4', '6'], default='4')
    ap.add_argument('--steps', type=int, default=20000)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--validate-every', type=int, default=1000)
    ap.add_argument('--val-batches', type=int, default=4)
    ap.add_argument('--trunc', type=float, default=1.0)
    ap.add_argument('--trunc-cutoff', type=int, default=14)
    ap.add_argument('--use-roll', action='store_true')
    ap.add_argument('--max-yaw', type=float, default=0.2)
    ap.add_argument('--max-pitch', type=float, default=0.1)
    ap.add_argument('--max-roll', type=float, default=0.2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--init', help='state dict to start from (He initialisation otherwise)')
    ap.add_argument('--out-dir', required=True)
    a = ap.parse_args()
    import torch
    from inv3d_amd import synthetic as S
    from inv3d_amd.pose_net import resnet34_pose
    from inv3d_amd.pose_train import PoseEstimatorTrainer, resnet34_pose_trainable
    if a.network:
        from inv3d_amd import weights as W
        G = W.load_generator(a.network, device='cuda')
    else:
        if a.synthetic == 'small':
            from oracle import eg3d_oracle as O
            G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                                 rendering_kwargs=O.small_config().rendering, device='cuda')
        else:
            G = S.make_generator(device='cuda')
        S.load_synthetic_weights(G, a.seed)
    torch.manual_seed(a.seed)
    net = resnet34_pose_trainable(int(a.camera_type))
    if a.init:
        net.load_state_dict(torch.load(a.init, map_location='cpu'))
    tr = PoseEstimatorTrainer(G, net.cuda(), batch_size=a.batch, lr=a.lr, camera_type=a.camera_type, seed=a.seed, val_seed=a.seed + 1, val_batches=a.val_batches,
                              stream_kwargs=dict(truncation_psi=a.trunc, truncation_cutoff=a.trunc_cutoff, use_roll=a.use_roll, max_yaw=a.max_yaw,
                                                 max_pitch=a.max_pitch, max_roll=a.max_roll))
    log = tr.fit(a.steps, a.validate_every, a.out_dir)
    for r in log:
        print(json.dumps(r))
    json.dump(log, open(os.path.join(a.out_dir, 'log.json'), 'w'), indent=1)
    resnet34_pose(int(a.camera_type)).load_state_dict(torch.load(os.path.join(a.out_dir, 'model_best.pt'), map_location='cpu'), strict=True)
    print('wrote', os.path.join(a.out_dir, 'model_best.pt'))


if __name__ == '__main__':
    main()
