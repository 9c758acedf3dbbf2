"""GANSpace latent editing, the parts that need no GPU (inv3d_amd/ganspace.py; tests/support/pca_ref.py, grid_ref.py): the float64 PCA
restatement against the recorded output of the reference's estimator (tests/golden/ganspace.npz, tests/golden/make_golden_ganspace.py), the edit
directions against a literal restatement of run_ganspace.py:31-36, the component files, the table of named directions and the grid layout."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
from pca_ref import pca_ref  # noqa: E402
from grid_ref import grid_ref, grid_size  # noqa: E402


def test_pca_ref_reproduces_the_estimator():
    """Agreement measured when the fixture was made: 1.5e-6 components, 3e-7 stdev, 2e-7 var_ratio, 7e-8 total_var (sklearn works in float32)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ganspace.npz'))
    assert g['X'].shape == (400, 24) and g['X'].dtype == np.float32 and g['components'].shape == (24, 24)
    r = pca_ref(g['X'], 24)
    assert np.abs(r['components'] - g['components']).max() <= 4e-6
    assert np.abs(r['stdev'] - g['stdev']).max() <= 1e-6
    assert np.abs(r['var_ratio'] - g['var_ratio']).max() <= 1e-6
    assert abs(r['total_var'] - float(g['total_var'])) <= 1e-6
    assert np.all(np.diff(g['stdev']) < 0)


def _directions_literal(pca_comp, idx_comp, start_layer, layer_num, edit_power, num_imgs, num_ws=14):
    """run_ganspace.py:27-36, with the device moves and the rendering left out."""
    V = torch.tensor(pca_comp).transpose(0, 1)
    K = V.shape[1]
    direction_list = []
    for i in range(1, num_imgs + 1):
        control_params = torch.zeros(K)
        control_params[idx_comp] = -edit_power + ((2 * edit_power) / (num_imgs - 1)) * (i - 1)
        direction = torch.matmul(V, control_params).reshape(1, -1).unsqueeze(0).expand(-1, layer_num, -1)
        direction_matrix = torch.zeros(1, num_ws, V.shape[0])
        direction_matrix[0, start_layer:start_layer + layer_num, :] = direction
        direction_list.append(direction_matrix)
    return torch.cat(direction_list, 0)


@pytest.mark.parametrize('idx,start,num,power,imgs', [(0, 0, 14, 1, 2), (12, 0, 5, 2, 5), (2, 7, 7, 4, 6)])
def test_edit_directions_match_the_reference_loop(idx, start, num, power, imgs):
    from inv3d_amd import ganspace as GS
    comp = np.random.RandomState(5).randn(16, 40).astype(np.float32)
    d = GS.edit_directions(comp, idx, start, num, power, imgs)
    want = _directions_literal(comp, idx, start, num, power, imgs)
    assert d.shape == (imgs, 14, 40) and d.dtype == torch.float32
    assert torch.equal(d, want)
    outside = torch.ones(14, dtype=torch.bool)
    outside[start:start + num] = False
    assert not d[:, outside].any()
    assert d[:, start:start + num].abs().sum() > 0
    if imgs % 2:
        assert not d[imgs // 2].any()
    assert torch.equal(d[0, start], torch.from_numpy(comp[idx]) * -power) and torch.equal(d[-1, start], torch.from_numpy(comp[idx]) * power)


def test_edit_directions_refuse_what_the_reference_mishandles():
    from inv3d_amd import ganspace as GS
    comp = np.ones((3, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        GS.edit_directions(comp, 0, start_layer=8, layer_num=7)
    with pytest.raises(ValueError):
        GS.edit_directions(comp, 0, num_imgs=1)
    assert GS.edit_directions(comp, 0, start_layer=7, layer_num=7).shape == (5, 14, 8)
    assert GS.edit_directions(comp, 0, start_layer=2, layer_num=2, num_ws=4).shape == (5, 4, 8)


def test_components_round_trip(tmp_path):
    from inv3d_amd import ganspace as GS
    comp = np.random.RandomState(6).randn(5, 12).astype(np.float32)
    p = str(tmp_path / 'comp.npy')
    GS.save_components(p, comp)
    assert np.array_equal(GS.load_components(p), comp) and np.array_equal(np.load(p), comp)
    res = GS.PCAResult(torch.from_numpy(comp), torch.ones(5), torch.ones(5) / 5, torch.zeros(12), 5.0, 10, 3, True)
    GS.save_components(p, res)
    assert np.array_equal(GS.load_components(p), comp)
    # a file as the reference's ganspace/pca_comp/*.npy: [512, 512] float32, written by plain np.save
    full = np.random.RandomState(7).randn(512, 512).astype(np.float32)
    p2 = str(tmp_path / 'pca_10_5_frontcam.npy')
    np.save(p2, full)
    got = GS.load_components(p2)
    assert got.dtype == np.float32 and np.array_equal(got, full)


def test_named_directions_and_front_camera():
    from inv3d_amd import ganspace as GS
    assert GS.GANSPACE_DIRECTIONS == {'bright hair': (2, 7, 7, 4), 'smile': (12, 0, 5, 2), 'age': (5, 0, 5, 3.5), 'short hair': (2, 0, 5, 4),
                                      'glass': (4, 0, 5, 4), 'gender': (0, 0, 5, 4)}
    assert list(GS.FRONT_CAM) == [0.9966070652008057, 0.003541737562045455, -0.08222994953393936, 0.20670529656089412, -0.009605886414647102,
                                  -0.9872410893440247, -0.15894262492656708, 0.4137044218920643, -0.08174371719360352, 0.1591932326555252,
                                  -0.9838574528694153, 2.660098037982929, 0, 0, 0, 1, 4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1]


def test_package_needs_no_sklearn_torchvision_or_imageio():
    src = open(os.path.join(ROOT, '3dgan-inversion_amd', 'inv3d_amd', 'ganspace.py')).read()
    for name in ('sklearn', 'torchvision', 'imageio'):
        assert f'import {name}' not in src and f'from {name}' not in src


LAYOUTS = [(1, 8, 4, 4, 2), (5, 8, 8, 8, 2), (7, 3, 17, 5, 2), (6, 3, 4, 4, 0)]


@pytest.mark.parametrize('N,nrow,H,W,padding', LAYOUTS)
def test_grid_ref_layout(N, nrow, H, W, padding):
    from inv3d_amd import hipops
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    want = (ymaps * (H + padding) + padding, xmaps * (W + padding) + padding)
    assert grid_size(N, H, W, nrow, padding) == want == hipops.image_grid_size(N, H, W, nrow, padding)
    # image k is the constant (k + 1) / 128: byte k + 129 at its cell, pad_value everywhere else
    img = np.stack([np.full((3, H, W), (k + 1) / 127.5, dtype=np.float32) for k in range(N)])
    g = grid_ref(img, nrow, padding, pad_value=7)
    assert g.shape == want + (3,) and g.dtype == np.uint8
    covered = np.zeros(want, dtype=bool)
    for k in range(N):
        y0, x0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        assert np.all(g[y0:y0 + H, x0:x0 + W] == k + 129)
        covered[y0:y0 + H, x0:x0 + W] = True
    assert np.all(g[~covered] == 7) and int(covered.sum()) == N * H * W


def test_grid_ref_conversion():
    from grid_ref import to_u8
    x = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 3.0, (200 - 128) / 127.5, 0.999], dtype=np.float32)
    want = (torch.from_numpy(x) * 127.5 + 128).clamp(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(to_u8(x), want) and list(want[:6]) == [0, 0, 128, 128, 255, 255]


def test_wrappers_refuse_cpu_tensors():
    from inv3d_amd import hipops, ganspace as GS
    from inv3d_amd._lib import Eg3dHipError
    with pytest.raises(Eg3dHipError):
        hipops.pca_moments(torch.zeros(4, 3), torch.zeros(3))
    with pytest.raises(Eg3dHipError):
        hipops.sym_eig(torch.eye(3))
    with pytest.raises(Eg3dHipError):
        hipops.image_grid_u8(torch.zeros(1, 3, 4, 4), 8)
    with pytest.raises(Eg3dHipError):
        GS.fit_pca(torch.zeros(8, 3))
