"""Reconstruction metrics of the reference's evaluation block (training/coaches/single_id_coach.py:87-117) on the gfx950 kernels.

    ms_ssim / ssim           pytorch_msssim 1.0's functions (win=None), drop-in: autograd functions over csrc/ssim.hip (levels + 1 launches
                             forward, 2 per level backward, no floating-point atomics, no host synchronise)
    IDLoss                   criteria/id_loss.py: ArcFace Backbone(112, 50, 'ir_se') (models/encoders/model_irse.py) on the implicit-GEMM
                             kernels of e4e.py; the face crop + AdaptiveAvgPool2d(112) + layout is one kernel (hipops.face_pool), the output
                             layer (BatchNorm2d, Linear 25088 -> 512, BatchNorm1d folded into one weight) a 7x7 valid convolution
    reconstruction_metrics   the four numbers the reference writes to {name}metrics.txt, computed as it computes them
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import _lib as L
from . import hipops as H
from .e4e import _bn_affine, ir_se50_layers, run_input_layer
from .loss_nets import conv_act

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, Y, cfg):
        out, pyr, stats = H.ssim_forward(X.detach(), Y.detach(), *cfg)
        ctx.save_for_backward(X, Y, pyr, stats)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, g):
        X, Y, pyr, stats = ctx.saved_tensors
        gx, gy = H.ssim_backward(X.detach(), Y.detach(), pyr, stats, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1], *ctx.cfg)
        return gx, gy, None


def _check(X, Y, win_size, win, levels):
    if win is not None:
        raise NotImplementedError('only win=None (the Gaussian window from win_size / win_sigma) is supported')
    if X.shape != Y.shape:
        raise ValueError(f'Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}.')
    if X.dim() != 4:
        raise ValueError(f'Input images should be 4-d tensors [N,C,H,W], but got {tuple(X.shape)}')
    if X.dtype != torch.float32 or Y.dtype != torch.float32:
        raise ValueError(f'Input images should be float32, got {X.dtype} and {Y.dtype}')
    if win_size % 2 != 1 or not 1 <= win_size <= 15:
        raise ValueError('Window size should be odd (and at most 15).')
    L.require_cuda(X, Y)
    h, w = X.shape[-2:]
    for lvl in range(levels):
        # pytorch_msssim skips the smoothing along a side shorter than the window; here that is an error (a documented deviation)
        if min(h, w) < win_size:
            raise ValueError(f'level {lvl} is {h}x{w}, smaller than the {win_size}-tap window')
        h, w = h // 2 + h % 2, w // 2 + w % 2


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: the mean SSIM per image [N] (or over everything with size_average) of fp32 [N,C,H,W] images."""
    _check(X, Y, win_size, win, 1)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    return _SsimFn.apply(X, Y, (0, (1.0,), bool(nonnegative_ssim), bool(size_average), int(win_size), float(win_sigma), C1, C2))


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: prod_l relu(m_l)^w_l per (image, channel) with m_l the mean contrast-structure term of levels 0..L-2 and the mean
    SSIM of the last, averaged over channels [N] (or over everything with size_average).  A term at or below 0 passes no gradient (the relu),
    so a clamped level gives a zero gradient, not NaN."""
    weights = MS_SSIM_WEIGHTS if weights is None else tuple(float(w) for w in (weights.tolist() if torch.is_tensor(weights) else weights))
    if not 1 <= len(weights) <= L.SSIM_MAX_LEVELS:
        raise ValueError(f'1 to {L.SSIM_MAX_LEVELS} weights, got {len(weights)}')
    smaller_side = min(X.shape[-2:])
    if not smaller_side > (win_size - 1) * (2 ** 4):
        raise ValueError('Image size should be larger than %d due to the 4 downsamplings in ms-ssim' % ((win_size - 1) * (2 ** 4)))
    _check(X, Y, win_size, win, len(weights))
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    return _SsimFn.apply(X, Y, (1, weights, False, bool(size_average), int(win_size), float(win_sigma), C1, C2))


class Backbone(torch.nn.Module):
    """models/encoders/model_irse.py Backbone(112, 50, 'ir_se'): the same module tree and state-dict keys (input_layer.*, body.N.*,
    output_layer.{0,3,4}), so the reference's model_ir_se50.pth loads with load_state_dict.  Inference only (eval-mode BatchNorm, Dropout off)."""

    def __init__(self, input_size=112, num_layers=50, mode='ir_se', drop_ratio=0.6, affine=True):
        super().__init__()
        if (input_size, num_layers, mode, affine) != (112, 50, 'ir_se', True):
            raise NotImplementedError("the identity metric uses Backbone(112, 50, 'ir_se') (criteria/id_loss.py)")
        self.input_layer, body = ir_se50_layers()
        self.output_layer = torch.nn.Sequential(torch.nn.BatchNorm2d(512), torch.nn.Dropout(drop_ratio), torch.nn.Flatten(),
                                                torch.nn.Linear(512 * 7 * 7, 512), torch.nn.BatchNorm1d(512, affine=affine))
        self.body = body
        self.eval()

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('the ArcFace network runs with frozen BatchNorm statistics (id_loss.py facenet.eval())')
        return super().train(False)

    def _folded_output(self):
        """BatchNorm2d, Linear and BatchNorm1d as one 7x7 convolution: w[j,c,h,w] = a1[j] W[j, c*49 + h*7 + w] a2[c] (Flatten's (c, h, w) order
        is the conv weight's), b = a1 (W b2 + bias) + b1."""
        bn2, lin, bn1 = self.output_layer[0], self.output_layer[3], self.output_layer[4]
        a2, b2 = _bn_affine(bn2)
        a1, b1 = _bn_affine(bn1)
        wt = lin.weight.view(512, 512, 7, 7)
        w = (wt * a2.view(1, -1, 1, 1) * a1.view(-1, 1, 1, 1)).contiguous()
        b = a1 * (lin.bias + (wt * b2.view(1, -1, 1, 1)).sum((1, 2, 3))) + b1
        return w, b

    @torch.no_grad()
    def forward(self, x):
        """[N,3,112,112] (or the channels-last [N,4,112,112] image with a zero fourth channel) -> l2-normalised features [N,512]."""
        if x.shape[1] == 3:
            n, _, h, w = x.shape
            x = torch.cat([x.float(), x.new_zeros(n, 1, h, w, dtype=torch.float32)], 1).contiguous(memory_format=torch.channels_last)
        x = run_input_layer(self.input_layer, x)
        for unit in self.body:
            x = unit(x)
        bn2, lin, bn1 = self.output_layer[0], self.output_layer[3], self.output_layer[4]
        srcs = [lin.weight, lin.bias] + [getattr(bn, k) for bn in (bn2, bn1) for k in ('weight', 'bias', 'running_mean', 'running_var')]
        w, b = H.memo('arcface_output', srcs, self._folded_output)
        z = conv_act(x, w, b, 1, 0, 'linear').reshape(x.shape[0], 512)
        return z / torch.norm(z, 2, 1, True)                       # l2_norm (helpers.py)


def _seed_(module: torch.nn.Module, seed: int):
    """Stand-in weights (no ArcFace checkpoint ships with the package): He-scaled convolutions with damped residual branches and gates,
    BatchNorm / PReLU parameters near their usual values, a 1 / sqrt(fan_in) linear layer."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * math.sqrt(2.0 / (p.shape[1] * p.shape[2] * p.shape[3])))
                if '.res_layer.3.' in name or name.endswith('fc2.weight'):
                    p.mul_(0.25)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]))
            elif name.endswith('.bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif '.res_layer.2.' in name or name == 'input_layer.2.weight':
                p.copy_(0.25 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))


class IDLoss(torch.nn.Module):
    """criteria/id_loss.py IDLoss: facenet = Backbone(112, 50, 'ir_se'); seeded stand-in weights unless `seed` is None -- load the real ones with
    IDLoss().facenet.load_state_dict(torch.load('model_ir_se50.pth'))."""
    CROP = (slice(35, 223), slice(32, 220))

    def __init__(self, seed: Optional[int] = 17):
        super().__init__()
        self.facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
        if seed is not None:
            _seed_(self.facenet, seed)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('IDLoss is an inference-only metric')
        return super().train(False)

    @torch.no_grad()
    def extract_feats(self, x):
        """x[:, :, 35:223, 32:220] (Python slice bounds: clamped to the image, as the reference applies it to 512^2 images) -> AdaptiveAvgPool2d(112)
        -> facenet: [N,512]."""
        r0, r1, _ = self.CROP[0].indices(x.shape[2])
        c0, c1, _ = self.CROP[1].indices(x.shape[3])
        if r1 <= r0 or c1 <= c0:
            raise ValueError(f'the face crop [35:223, 32:220] of a {x.shape[2]}x{x.shape[3]} image is empty')
        return self.facenet(H.face_pool(x.float(), r0, r1, c0, c1, 112))

    def identity_distance(self, y_hat, y):
        """1 - <f(y_hat), f(y)> per image, [N]."""
        f = self.extract_feats(torch.cat([y_hat, y]))
        return 1 - (f[:y_hat.shape[0]] * f[y_hat.shape[0]:]).sum(1)

    def forward(self, y_hat, y):
        """The reference's loss: 1 - <f(y_hat)[0], f(y)[0]> (the first image of the batch only)."""
        return self.identity_distance(y_hat[:1], y[:1])[0]


@torch.no_grad()
def reconstruction_metrics(img, target, lpips_net, id_net) -> Dict[str, float]:
    """single_id_coach.py:90-99 as written: img / target in [-1,1] mapped to [0,1] by (v + 1) / 2 without a clamp; mse (l2_loss.l2_loss), lpips
    (the [-1,1] network fed the [0,1] images, as the reference does), ms_ssim(data_range=1), identity on the images mapped back to [-1,1].
    A batch gives batch means (the reference's .item() takes one image)."""
    synimg = (img + 1) / 2
    image = (target + 1) / 2
    m_mse = F.mse_loss(synimg, image).item()
    m_lpips = lpips_net.distance(synimg, image).mean().item()
    m_msssim = ms_ssim(synimg, image, data_range=1, size_average=False).mean().item()
    m_identity = id_net(synimg * 2 - 1, image * 2 - 1).item()
    return dict(mse=m_mse, lpips=m_lpips, msssim=m_msssim, identity=m_identity)


def format_metrics_txt(m: Dict[str, float]) -> str:
    """The text of {name}metrics.txt (single_id_coach.py:102-106)."""
    return ''.join('{}: {}\n'.format(k, float(m[k])) for k in ('mse', 'lpips', 'msssim', 'identity'))
