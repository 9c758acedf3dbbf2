"""Training the pose estimator on the generator's own renderings (scripts/gen_pseudo_dataset.py + scripts/train_pose_estimator.py of the
reference, which its README asks users of any other generator to run first).

The reference renders a pseudo dataset to PNG files at known random poses and then trains its ResNet-34 on them.  Here both halves are
one loop on the GPU: `PseudoPoseStream` renders batches on the fly (no files), `TrainablePoseNet` is `pose_net.ResNetPose` with a working
training mode -- every conv on the implicit-GEMM kernels with a linear epilogue, followed by BatchNorm on batch statistics
(hipops.batch_norm_train, csrc/batchnorm.hip; the block's residual add and ReLU ride in the same pass) -- and `PoseEstimatorTrainer` runs
the reference's objective with Adam.  In eval mode the network IS the folded path of pose_net.py, so a checkpoint written here is what
`LatentProjector(pose_net=...)` and `InversionCoach` consume.  On CPU tensors the network runs on plain torch ops (tests)."""
import math
import os
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import hipops as H
from .inversion import pose_to_rotmat
from .loss_nets import conv_act, conv_scale_act_ok, max_pool, _ConvScaleActFn
from .pose_net import ResNetPose

CAMERA_MODES = {'4': 'quat', '6': '6d', '2': 'euler'}          # --camera_type of the reference's trainer -> inversion.pose_to_rotmat mode
ROLL_RADIUS = 2.7          # create_cam2world_matrix_roll re-derives the origin with this literal, whatever radius the caller passed


# ---------------------------------------------------------------------------------------------------------------- the network
class TrainablePoseNet(ResNetPose):
    """ResNetPose (same module tree, same state-dict keys) whose `train()` works.

    train mode, GPU: conv (linear epilogue, no folded scale, no bias) -> batch_norm_train; both packed images of every conv weight come
    from one batched launch per step, as ResNetPose._pack_all builds the folded ones.  eval mode, GPU: ResNetPose.forward unchanged.
    CPU tensors (either mode): torch.nn.functional ops, with hipops.batch_norm_train's CPU composite in train mode."""

    def __init__(self, layers=(3, 4, 6, 3), output_dims=4):
        super().__init__(layers, output_dims)
        self._consts = {}

    def train(self, mode=True):
        self._stat_key = None          # the running statistics move while training: eval must re-read them
        return torch.nn.Module.train(self, mode)

    def _pairs(self):
        pairs = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                pairs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
                if blk.downsample is not None:
                    pairs.append((blk.downsample[0], blk.downsample[1]))
        return pairs

    def _const(self, kind, n, dev):
        key = (kind, n, str(dev))
        if key not in self._consts:
            self._consts[key] = (torch.ones if kind == 'one' else torch.zeros)(n, device=dev)
        return self._consts[key]

    def _pack_plain(self):
        items, convs = [], []
        for conv, _ in self._pairs():
            w = conv.weight
            Co, Ci, kh, kw = w.shape
            if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and conv_scale_act_ok(Ci, w, 'linear')):
                continue
            wf = torch.empty((Co, kh * kw * Ci), device=w.device)
            wa = torch.empty((Ci, kh * kw * Co), device=w.device)
            items.append((w.detach(), wf, wa, None, 0))
            conv._eg3d_packed = (wf, wa)
            convs.append(conv)
        if items:
            H.pack_conv_weights_batched(items)
        return convs

    def _conv(self, x, conv):
        w = conv.weight
        Co = w.shape[0]
        if conv_scale_act_ok(x.shape[1], w, 'linear'):
            return _ConvScaleActFn.apply(x, w, self._const('one', Co, x.device), self._const('zero', Co, x.device), conv.stride[0], conv.padding[0],
                                         'linear', getattr(conv, '_eg3d_packed', None))
        assert conv is self.conv1, 'only the 7x7 / 3-channel stem may leave the packed path'
        return conv_act(x, w, self._const('zero', Co, x.device), conv.stride[0], conv.padding[0], 'linear')       # the 7x7 stem

    @staticmethod
    def _bn(x, bn, act, residual=None):
        return H.batch_norm_train(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                                  residual=residual, act=act)

    def _head(self, x):
        x = x.mean((2, 3))
        x = F.relu(self.fc(x))
        x = F.relu(self.fc2(x))
        return torch.tanh(self.fc3(x))

    def _forward_torch(self, img):
        def bn(x, m, act, residual=None):
            if self.training:
                return self._bn(x, m, act, residual)
            y = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
            y = y if residual is None else y + residual
            return F.relu(y) if act == 'relu' else y

        def cv(x, c):
            return F.conv2d(x, c.weight, None, c.stride, c.padding)
        x = bn(cv(img.to(self.conv1.weight.dtype), self.conv1), self.bn1, 'relu')
        x = F.max_pool2d(x, 3, 2, 1)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                out = bn(cv(x, blk.conv1), blk.bn1, 'relu')
                idn = x if blk.downsample is None else bn(cv(x, blk.downsample[0]), blk.downsample[1], 'linear')
                x = bn(cv(out, blk.conv2), blk.bn2, 'relu', idn)
        return self._head(x)

    def forward(self, img):
        if not img.is_cuda:
            return self._forward_torch(img)
        if not self.training:
            return super().forward(img)
        n, c, h, w = img.shape
        x = torch.cat([img.float(), img.new_zeros(n, 1, h, w, dtype=torch.float32)], 1).contiguous(memory_format=torch.channels_last)
        convs = self._pack_plain()
        try:
            x = self._bn(self._conv(x, self.conv1), self.bn1, 'relu')
            x = max_pool(H.to_cl(F.pad(x, (1, 1, 1, 1), value=float('-inf'))), 3, 2)
            for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
                for blk in layer:
                    out = self._bn(self._conv(x, blk.conv1), blk.bn1, 'relu')
                    idn = x if blk.downsample is None else self._bn(self._conv(x, blk.downsample[0]), blk.downsample[1], 'linear')
                    x = self._bn(self._conv(out, blk.conv2), blk.bn2, 'relu', idn)
        finally:
            for cv in convs:
                cv._eg3d_packed = None
        return self._head(x)


def resnet34_pose_trainable(output_dims=4):
    return TrainablePoseNet((3, 4, 6, 3), output_dims)


# ---------------------------------------------------------------------------------------------------------------- poses
def poses_from_angles(theta: torch.Tensor, phi: torch.Tensor, roll: Optional[torch.Tensor] = None, use_roll: bool = False, radius: float = 2.7,
                      pivot: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n,4,4] cam2world of cameras at azimuth theta / polar angle phi on the sphere of `radius`, looking at `pivot` (origin), y up -- the
    reference's LookAt3DPoseSampler.sample (utils/camera_utils.py:58-74).  With use_roll the rotation is roll about the view axis times
    that rotation, and the camera origin is re-derived as -2.7 * R[:, :, 2] whatever `radius` and `pivot` are (:158-187): the reference's
    own data has that quirk, so the estimator is trained on it."""
    theta, phi = theta.reshape(-1, 1).float(), phi.reshape(-1, 1).float()
    dev = theta.device
    sp = torch.sin(phi)
    origin = torch.cat([radius * sp * torch.cos(math.pi - theta), radius * torch.cos(phi), radius * sp * torch.sin(math.pi - theta)], 1)
    look = torch.zeros(3, device=dev) if pivot is None else pivot.to(dev).float().reshape(1, 3)
    fwd = look - origin
    fwd = fwd / torch.norm(fwd, dim=-1, keepdim=True)
    fwd = fwd / torch.norm(fwd, dim=-1, keepdim=True)          # normalised twice, as there
    up0 = torch.tensor([0., 1., 0.], device=dev).expand_as(fwd)
    right = torch.linalg.cross(up0, fwd, dim=-1)
    right = -(right / torch.norm(right, dim=-1, keepdim=True))
    up = torch.linalg.cross(fwd, right, dim=-1)
    up = up / torch.norm(up, dim=-1, keepdim=True)
    rot = torch.stack((right, up, fwd), dim=-1)
    if use_roll:
        r = roll.reshape(-1, 1).float().to(dev)
        c, s, z, o = torch.cos(r), torch.sin(r), torch.zeros_like(r), torch.ones_like(r)
        rot = torch.bmm(torch.stack([torch.cat([c, -s, z], 1), torch.cat([s, c, z], 1), torch.cat([z, z, o], 1)], 1), rot)
        origin = -rot[:, :, 2] * ROLL_RADIUS
    n = rot.shape[0]
    bottom = torch.tensor([0., 0., 0., 1.], device=dev).expand(n, 1, 4)
    return torch.cat([torch.cat([rot, origin.unsqueeze(-1)], 2), bottom], 1)


def sample_pseudo_poses(n: int, max_yaw: float = 0.2, max_pitch: float = 0.1, max_roll: float = 0.2, use_roll: bool = False, radius: float = 2.7,
                        generator: Optional[torch.Generator] = None, device=None, return_angles: bool = False):
    """[n,4,4] cam2world matrices of the reference's pseudo-dataset distribution (scripts/gen_pseudo_dataset.py:169-177): yaw uniform in
    +-pi/2 * max_yaw and pitch uniform in +-pi/2 * max_pitch about pi/2, roll uniform in +-pi/2 * max_roll (drawn always, used with
    use_roll).  Batched; runs on `device` (the generator's device by default)."""
    dev = torch.device(device if device is not None else (generator.device if generator is not None else 'cpu'))
    u = torch.rand((n, 3), generator=generator, device=generator.device if generator is not None else dev).to(dev)
    yaw = (u[:, 0] - 0.5) * (math.pi * max_yaw)
    pitch = (u[:, 1] - 0.5) * (math.pi * max_pitch)
    roll = (u[:, 2] - 0.5) * (math.pi * max_roll)
    ext = poses_from_angles(math.pi / 2 + yaw, math.pi / 2 + pitch, roll, use_roll, radius)
    return (ext, torch.stack([yaw, pitch, roll], 1)) if return_angles else ext


def fov_to_intrinsics(fov_deg: float = 18.837, device='cpu') -> torch.Tensor:
    """Normalised 3x3 intrinsics of the reference's FOV_to_intrinsics (it spells pi as 3.14159 and sqrt 2 as 1.414; so does this)."""
    f = float(1 / (math.tan(fov_deg * 3.14159 / 360) * 1.414))
    return torch.tensor([[f, 0, 0.5], [0, f, 0.5], [0, 0, 1]], device=device)


# ---------------------------------------------------------------------------------------------------------------- the data
class PseudoPoseStream:
    """Endless seeded source of (image [B,3,S,S] in [0,255], extrinsic [B,4,4]) batches rendered on the fly: z ~ N(0,1) -> G.mapping(z,
    frontal camera, truncation_psi, truncation_cutoff) -> G.synthesis(ws, camera at a `sample_pseudo_poses` pose)['image'] -> * 127.5 + 128,
    clamp to [0,255] -> (quantize, the default) truncate to the 256 levels the reference's PNG files hold -> area resize to S = 256 -- the
    tensor train_pose_estimator.py:110-112 hands the estimator after undoing its loader's normalisation.  Nothing is written to disk; the
    stratified-sampling uniforms and the per-layer noise come from the stream's seed too, so two streams with one seed yield the same batches.  A fixed
    validation set is `PseudoPoseStream(..., seed=other).take(k)`."""

    def __init__(self, G, batch_size: int = 32, seed: int = 0, *, truncation_psi: float = 1.0, truncation_cutoff: Optional[int] = 14,
                 max_yaw: float = 0.2, max_pitch: float = 0.1, max_roll: float = 0.2, use_roll: bool = False, radius: Optional[float] = None,
                 fov_deg: float = 18.837, quantize: bool = True, size: int = 256, device=None, synth_kwargs: Optional[dict] = None, render_chunk: int = 8):
        self.G = G          # left as found: rendering runs under no_grad and switches to eval mode only for the duration of a batch
        self.dev = torch.device(device if device is not None else next(G.parameters()).device)
        self.B, self.size, self.quantize = int(batch_size), int(size), bool(quantize)
        self.chunk = max(1, int(render_chunk))
        self.psi, self.cutoff = truncation_psi, truncation_cutoff
        self.pose_kw = dict(max_yaw=max_yaw, max_pitch=max_pitch, max_roll=max_roll, use_roll=use_roll,
                            radius=float(G.rendering_kwargs.get('avg_camera_radius', 2.7) if radius is None else radius))
        self.gen = torch.Generator(device=self.dev).manual_seed(int(seed))
        self._host_gen = torch.Generator().manual_seed(int(seed))          # seeds of the generator's own random draws (per-layer noise), no device read
        self.K = fov_to_intrinsics(fov_deg, self.dev).reshape(1, 9)
        front = poses_from_angles(torch.tensor([math.pi / 2], device=self.dev), torch.tensor([math.pi / 2], device=self.dev), radius=self.pose_kw['radius'])
        self.cond = torch.cat([front.reshape(1, 16), self.K], 1)
        self.synth_kwargs = dict(synth_kwargs or {})

    @torch.no_grad()
    def next(self) -> Tuple[torch.Tensor, torch.Tensor]:
        G, B = self.G, self.B
        z = torch.randn((B, G.z_dim), generator=self.gen, device=self.dev)
        ext = sample_pseudo_poses(B, generator=self.gen, device=self.dev, **self.pose_kw)
        cam = torch.cat([ext.reshape(B, 16), self.K.expand(B, 9)], 1)
        cutoff = None if self.cutoff is None else min(int(self.cutoff), G.backbone.num_ws)
        ws = G.mapping(z, self.cond.expand(B, 25), truncation_psi=self.psi, truncation_cutoff=cutoff)
        rk = G.rendering_kwargs
        m = int(G.neural_rendering_resolution) ** 2
        u1 = torch.rand((B, m, int(rk['depth_resolution']), 1), generator=self.gen, device=self.dev)
        df = int(rk['depth_resolution_importance'])
        u2 = torch.rand((B * m, df), generator=self.gen, device=self.dev) if df > 0 else None
        # the synthesis draws its per-layer noise (noise_mode 'random', as the reference renders its dataset) from the global generator: seeded
        # from the stream for the duration of the call, the caller's generator state untouched
        was_training = G.training
        G.eval()
        with torch.random.fork_rng(devices=[self.dev] if self.dev.type == 'cuda' else []):
            torch.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=self._host_gen)))
            parts = []
            for a in range(0, B, self.chunk):          # the generator's kernels are built for the inversion loops' batches (<= 8 images)
                b = min(B, a + self.chunk)
                uu = (u1[a:b], u2[a * m:b * m] if u2 is not None else None)
                parts.append(G.synthesis(ws[a:b], cam[a:b], render_uniforms=uu, **self.synth_kwargs)['image'].float())
            img = parts[0] if len(parts) == 1 else torch.cat(parts)
        G.train(was_training)
        img = (img * 127.5 + 128).clamp(0, 255)
        if self.quantize:
            img = img.floor()
        return _resize_area(img, self.size).contiguous(), ext

    def take(self, batches: int) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        return [self.next() for _ in range(batches)]

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        while True:
            yield self.next()


def _resize_area(img: torch.Tensor, size: int) -> torch.Tensor:
    h, w = img.shape[-2:]
    if h == size and w == size:
        return img
    if h % size == 0 and w % size == 0 and h // size == w // size:
        return F.avg_pool2d(img, h // size)
    return F.interpolate(img, size=(size, size), mode='area')


# ---------------------------------------------------------------------------------------------------------------- the objective
def geodesic_distance(r1: torch.Tensor, r2: torch.Tensor) -> torch.Tensor:
    """[B] rotation angle between [B,3,3] rotations: acos of the clamped (trace(r1 r2^T) - 1) / 2 (train_pose_estimator.py:246-255)."""
    m = torch.bmm(r1, r2.transpose(1, 2))
    cos = (m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2
    return torch.acos(torch.clamp(cos, -1.0, 1.0))


def pose_training_loss(pred: torch.Tensor, ext_gt: torch.Tensor, mode: str = '4', radius: float = 2.7):
    """(loss, parts) of the reference's trainer (train_pose_estimator.py:117-141): mean geodesic rotation distance + MSE of the translation
    -radius * R[:, :, 2] against the ground truth's, / batch * 10 + 1e-10 * mean of 1 / (|R00| - 1)^2 (keeps R off the exact identity
    diagonal).  mode: '4' quaternion | '6' 6-D | '2' two angles about pi/2 (the reference's own '2' branch only runs at batch 1)."""
    if mode not in CAMERA_MODES:
        raise ValueError(f"camera type must be one of {sorted(CAMERA_MODES)}, got {mode!r}")
    rot = pose_to_rotmat(pred, CAMERA_MODES[mode])
    bs = pred.shape[0]
    rot_loss = geodesic_distance(rot, ext_gt[:, :3, :3]).mean()
    trans_loss = F.mse_loss(-radius * rot[:, :3, 2], ext_gt[:, :3, 3]) / bs * 10
    reg_loss = (1 / (rot[:, 0, 0].abs() - 1).pow(2)).sum() / bs * 1e-10
    return rot_loss + trans_loss + reg_loss, dict(rot=rot_loss.detach(), trans=trans_loss.detach(), reg=reg_loss.detach())


# ---------------------------------------------------------------------------------------------------------------- the trainer
class PoseEstimatorTrainer:
    """scripts/train_pose_estimator.py on the GPU: `step()` = stream batch -> train-mode forward -> pose_training_loss -> backward -> Adam.

    Adam is torch.optim.Adam (fused multi-tensor on the GPU), as LatentProjector uses for this network: the library's own hipops.HipAdam
    takes 32 leaves per launch and the estimator has over a hundred parameter tensors, so torch's single launch is the better fit.
    `validate()` runs the folded eval path on a fixed validation set (the same stream class, another seed) and returns the mean geodesic
    error and the mean L1 translation error; `fit()` keeps model_best.pt by their sum, as the reference keeps it by its validation score.
    The reference's loop also evaluates a VGG16 on every batch and discards the result (train_pose_estimator.py:114,177); that call has no
    effect on the training and is not reproduced."""

    def __init__(self, G, net: TrainablePoseNet, *, batch_size: int = 32, lr: float = 1e-4, camera_type: str = '4', seed: int = 0, val_seed: int = 1,
                 val_batches: int = 2, radius: float = 2.7, stream_kwargs: Optional[dict] = None, stream=None, validation=None):
        if camera_type not in CAMERA_MODES:
            raise ValueError(f"camera type must be one of {sorted(CAMERA_MODES)}, got {camera_type!r}")
        self.net, self.mode, self.radius = net, camera_type, radius
        kw = dict(stream_kwargs or {})
        # stream: any object whose next() returns (image, extrinsic); validation: a list of such batches (both default to rendered ones)
        self.stream = stream if stream is not None else (PseudoPoseStream(G, batch_size, seed, **kw) if G is not None else None)
        self._val_src = (G, batch_size, val_seed, kw, val_batches)
        self._val = list(validation) if validation is not None else None
        params = list(net.parameters())
        for p in params:
            p.requires_grad_(True)
        self.optimizer = torch.optim.Adam(params, lr=lr, **(dict(fused=True) if params[0].is_cuda else {}))
        self.steps = 0

    def step(self, batch: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        img, ext = self.stream.next() if batch is None else batch
        self.net.train()
        pred = self.net(img)
        loss, parts = pose_training_loss(pred, ext, self.mode, self.radius)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        self.steps += 1
        return dict(loss=loss.detach(), **parts)

    def validation_set(self):
        if self._val is None:
            G, bs, seed, kw, k = self._val_src
            self._val = PseudoPoseStream(G, bs, seed, **kw).take(k)
        return self._val

    @torch.no_grad()
    def validate(self, batches=None) -> Dict[str, float]:
        """Mean geodesic error (radians) and mean L1 translation error over the validation set, through the eval (folded) path."""
        was = self.net.training
        self.net.eval()
        geo, l1, n = 0.0, 0.0, 0
        for img, ext in (self.validation_set() if batches is None else batches):
            rot = pose_to_rotmat(self.net(img), CAMERA_MODES[self.mode])
            geo += float(geodesic_distance(rot, ext[:, :3, :3]).sum())
            l1 += float((-self.radius * rot[:, :3, 2] - ext[:, :3, 3]).abs().mean(1).sum())
            n += img.shape[0]
        self.net.train(was)
        return dict(geodesic=geo / n, translation_l1=l1 / n)

    def fit(self, steps: int, validate_every: int = 1000, out_dir: Optional[str] = None) -> List[Dict[str, float]]:
        """`steps` training steps; validation before the first, every `validate_every` and after the last.  Returns the log (one dict of
        scalars per validation); writes out_dir/model_best.pt whenever geodesic + translation_l1 improves, and out_dir/model_last.pt."""
        log, best = [], float('inf')
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)

        def _validate(last_loss):
            nonlocal best
            v = self.validate()
            rec = dict(step=self.steps, loss=last_loss, **v)
            score = v['geodesic'] + v['translation_l1']
            rec['best'] = score < best
            if score < best:
                best = score
                if out_dir is not None:
                    torch.save(self.net.state_dict(), os.path.join(out_dir, 'model_best.pt'))
            log.append(rec)
        _validate(float('nan'))
        for i in range(steps):
            out = self.step()
            if (i + 1) % validate_every == 0 or i + 1 == steps:
                _validate(float(out['loss']))
        if out_dir is not None:
            torch.save(self.net.state_dict(), os.path.join(out_dir, 'model_last.pt'))
        return log
