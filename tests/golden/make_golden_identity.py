#!/usr/bin/env python3
"""Identity-metric fixture generator (tests/golden/identity.npz).  Runs on a development machine with a checkout of the reference
(cvlab-kaist/3DGAN-Inversion):

    python tests/golden/make_golden_identity.py REFERENCE_ROOT

Loads tests/support/id_ref.synth_state into the reference's own models.encoders.model_irse.Backbone(112, 50, 'ir_se') (strict), checks that
the CPU restatement id_ref agrees with it, and stores its features and IDLoss values (criteria/id_loss.py: crop [35:223, 32:220],
AdaptiveAvgPool2d(112), 1 - <f(y_hat)[0], f(y)[0]>) for the seeded image pairs of id_ref.images at 256^2, 512^2 and 192^2.  Images and
weights come from seeds: only the probes are stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED = 3


def main(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
    import id_ref as IR
    from models.encoders.model_irse import Backbone
    net = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se').eval()
    sd = IR.synth_state(SEED)
    net.load_state_dict(sd, strict=True)
    out = dict(seed=np.int64(SEED))
    with torch.no_grad():
        for size in IR.SIZES:
            y_hat, y = IR.images(size, SEED)
            x = torch.cat([y_hat, y])
            f = net(torch.nn.functional.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], 112))
            fo = IR.extract_feats(sd, x)
            err = float((f - fo).abs().max())
            assert err < 2e-5, (size, err)
            d = 1 - (f[:2] * f[2:]).sum(1)
            assert float(d.min()) > 1e-3, d                           # distinguishable images
            out[f'feats_{size}'] = f.numpy().astype(np.float32)
            out[f'dist_{size}'] = d.numpy().astype(np.float32)
            out[f'loss_{size}'] = np.float32(1 - f[0].dot(f[2]))
            print(size, 'restatement err', err, 'distances', d.tolist())
    np.savez_compressed(os.path.join(HERE, 'identity.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
