"""CPU restatement of the identity metric (criteria/id_loss.py IDLoss with models/encoders/model_irse.py Backbone(112, 50, 'ir_se')) as a
function of a state dict with the reference's keys, built on oracle.e4e_oracle.trunk (the same IR-SE-50 units).  Pinned against the
reference's own Backbone by tests/golden/make_golden_identity.py (fixture tests/golden/identity.npz)."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import e4e_oracle as EO  # noqa: E402
from oracle.pose_net_oracle import _key_seed  # noqa: E402

SIZES = (256, 512, 192)          # crop in bounds; the reference's crop applied to 512^2 unchanged; a crop clamped to the image


def synth_state(seed=0):
    """The input_layer / body keys of e4e_oracle.synth_state(seed) plus seeded output_layer weights (BatchNorm statistics away from identity).
    The input convolution is scaled back up by 128: the e4e weights expect [0,255] pixels, the identity metric feeds [-1,1] images."""
    sd = {k: v for k, v in EO.synth_state(seed, heads=()).items() if k.startswith(('input_layer.', 'body.'))}
    sd['input_layer.0.weight'] = sd['input_layer.0.weight'] * 128.0

    def rnd(k, shape):
        return torch.randn(shape, generator=torch.Generator().manual_seed(_key_seed(k, seed)))
    for p in ('output_layer.0', 'output_layer.4'):
        sd[f'{p}.weight'] = 1 + 0.1 * rnd(f'{p}.weight', (512,))
        sd[f'{p}.bias'] = 0.1 * rnd(f'{p}.bias', (512,))
        sd[f'{p}.running_mean'] = 0.1 * rnd(f'{p}.running_mean', (512,))
        sd[f'{p}.running_var'] = 0.5 + torch.rand(512, generator=torch.Generator().manual_seed(_key_seed(f'{p}.running_var', seed)))
        sd[f'{p}.num_batches_tracked'] = torch.tensor(0)
    sd['output_layer.3.weight'] = rnd('output_layer.3.weight', (512, 512 * 49)) / math.sqrt(512 * 49)
    sd['output_layer.3.bias'] = 0.1 * rnd('output_layer.3.bias', (512,))
    return sd


def _bn(x, sd, p):
    return F.batch_norm(x, sd[f'{p}.running_mean'], sd[f'{p}.running_var'], sd[f'{p}.weight'], sd[f'{p}.bias'], False, 0.0, 1e-5)


def facenet(sd, x):
    """Backbone.forward: [N,3,112,112] -> l2-normalised [N,512]."""
    f = EO.trunk(sd, x)[2]
    z = F.linear(_bn(f, sd, 'output_layer.0').flatten(1), sd['output_layer.3.weight'], sd['output_layer.3.bias'])
    z = _bn(z, sd, 'output_layer.4')
    return z / torch.norm(z, 2, 1, True)


def face_crop_pool(x):
    return F.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], 112)


def extract_feats(sd, x):
    return facenet(sd, face_crop_pool(x))


def images(size, seed):
    """The fixture's seeded (y_hat, y) pair, [2,3,size,size] each in [-1,1]: y a smooth random image, y_hat y plus noise."""
    g = torch.Generator().manual_seed(seed * 1000 + size)
    y = F.interpolate(torch.rand(2, 3, size // 16, size // 16, generator=g), size=(size, size), mode='bilinear', align_corners=False) * 2 - 1
    y_hat = (y + 0.3 * torch.randn(2, 3, size, size, generator=g)).clamp(-1, 1)
    return y_hat, y
