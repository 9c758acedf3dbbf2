"""Reconstruction metrics without a GPU: the float64 MS-SSIM restatement's own properties (tests/support/msssim_ref.py, the oracle of the GPU
kernels), the ArcFace Backbone's reference keys and the CPU identity restatement against the reference's Backbone (tests/golden/identity.npz),
the metrics.txt text and the coach's argument validation."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import id_ref as IR  # noqa: E402
import msssim_ref as M  # noqa: E402


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_restatement_identity_and_symmetry():
    x, y = _rand((2, 3, 177, 203), 1), _rand((2, 3, 177, 203), 2)
    assert torch.allclose(M.ms_ssim(x, x, data_range=1, size_average=False), torch.ones(2, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(M.ssim(x, x, data_range=1), torch.tensor(1.0, dtype=torch.float64), atol=1e-12)
    y = 0.7 * x + 0.3 * y
    assert torch.allclose(M.ms_ssim(x, y, data_range=1), M.ms_ssim(y, x, data_range=1), atol=1e-14, rtol=0)
    assert torch.allclose(M.ssim(x, y, data_range=255), M.ssim(y, x, data_range=255), atol=1e-14, rtol=0)


def test_restatement_constant_images_closed_form():
    """Constant images a, b: variances 0, so cs = 1 and ssim = (2ab + C1) / (a^2 + b^2 + C1) at every level (pooling keeps them constant
    away from the zero-padded border of odd sides -- 192 = 2^6 * 3 keeps every level even)."""
    a, b, dr = 0.3, 0.8, 1.0
    x = torch.full((1, 3, 192, 192), a, dtype=torch.float64)
    y = torch.full((1, 3, 192, 192), b, dtype=torch.float64)
    C1 = (0.01 * dr) ** 2
    l = (2 * a * b + C1) / (a * a + b * b + C1)
    assert abs(float(M.ssim(x, y, data_range=dr)) - l) < 1e-12
    assert abs(float(M.ms_ssim(x, y, data_range=dr)) - l ** M.WEIGHTS[-1]) < 1e-12


def test_window_is_normalised_and_symmetric():
    for size, sigma in ((11, 1.5), (7, 1.0), (15, 3.0)):
        g = M.gauss_1d(size, sigma)
        assert abs(float(g.sum()) - 1) < 1e-15 and torch.equal(g, g.flip(0)) and int(g.argmax()) == size // 2
        assert abs(float(g[0] / g[size // 2]) - math.exp(-(size // 2) ** 2 / (2 * sigma ** 2))) < 1e-14


def test_level_sizes_and_pool_divisor():
    assert M.level_sizes(177, 203) == [(177, 203), (89, 102), (45, 51), (23, 26), (12, 13)]
    assert M.level_sizes(512, 512) == [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32)]
    x = torch.ones(1, 1, 5, 4, dtype=torch.float64)
    p = M.pool(x)
    assert p.shape == (1, 1, 3, 2)
    # an odd side pads one zero at both ends and still divides by 4: the first window holds the pad and one row (the far pad is never
    # reached: 5 rows + 2 pads make 3 windows, the last of rows 3-4)
    assert torch.equal(p[0, 0], torch.tensor([[0.5, 0.5], [1.0, 1.0], [1.0, 1.0]], dtype=torch.float64))
    assert M.pool(torch.ones(1, 1, 7, 7, dtype=torch.float64))[0, 0, 0, 0] == 0.25


def test_restatement_rejects_small_images():
    x = _rand((1, 3, 160, 400), 3)
    with pytest.raises(AssertionError):
        M.ms_ssim(x, x)
    with pytest.raises(ValueError):
        M.ssim(x[..., :10, :], x[..., :10, :])


def test_idloss_has_the_reference_keys():
    from inv3d_amd.metrics import IDLoss
    net = IDLoss()
    sd = IR.synth_state(0)
    net.facenet.load_state_dict(sd, strict=True)
    assert set(net.facenet.state_dict()) == set(sd)
    assert net.facenet.output_layer[3].weight.shape == (512, 25088)


def test_identity_restatement_vs_reference_fixture():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'identity.npz'))
    seed = int(z['seed'])
    sd = IR.synth_state(seed)
    with torch.no_grad():
        for size in IR.SIZES:
            y_hat, y = IR.images(size, seed)
            f = IR.extract_feats(sd, torch.cat([y_hat, y]))
            assert float((f - torch.from_numpy(z[f'feats_{size}'])).abs().max()) <= 2e-5, size
            d = 1 - (f[:2] * f[2:]).sum(1)
            assert float((d - torch.from_numpy(z[f'dist_{size}'])).abs().max()) <= 2e-5, size


def test_format_metrics_txt():
    from inv3d_amd.metrics import format_metrics_txt
    m = dict(identity=np.float32(0.25), mse=0.1, lpips=torch.tensor(0.5).item(), msssim=1)
    assert format_metrics_txt(m) == 'mse: 0.1\nlpips: 0.5\nmsssim: 1.0\nidentity: 0.25\n'


def test_coach_argument_validation():
    from inv3d_amd.coach import InversionCoach, InversionResult
    G = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match='eval_dir'):
        InversionCoach(G, do_evaluation=True, w_avg_samples=0)
    with pytest.raises(ValueError, match='pivot_dir'):
        InversionCoach(G, save_pivot=True, w_avg_samples=0)
    assert list(InversionResult.__dataclass_fields__)[-1] == 'metrics'
