"""Shape export on the GPU (csrc/marching_cubes.hip, hipops.marching_cubes, inference.extract_mesh / write_ply / write_mrc, the coach's
gen_mesh): bit-exact against the numpy restatement tests/support/mc_ref.py, closed oriented meshes of the full-size generator's 512^3 grid,
run-to-run and normal-vs-deterministic-build identity, and the per-image export of create_geometry (single_id_coach.py:109-110,120-163)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import mc_ref as M  # noqa: E402
from test_mesh_cpu import sphere, torus  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _gpu(g, level, **kw):
    from inv3d_amd import hipops as H
    v, f = H.marching_cubes(torch.from_numpy(np.ascontiguousarray(g)).to(DEV), level, **kw)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy(), f.cpu().numpy()


def _same(g, level, **kw):
    rv, rf = M.marching_cubes(g, level, **kw)
    v, f = _gpu(g, level, **kw)
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(f, rf)
    # the same fp32 operations in the same order (IEEE division, no contraction): no ulp allowance is needed
    assert np.array_equal(v.view(np.int32), rv.view(np.int32))
    return v, f


@pytest.mark.parametrize('dims', [(2, 2, 2), (3, 5, 7), (37, 53, 61), (64, 64, 64)])
def test_random_fields_match_the_restatement(dims):
    g = np.random.RandomState(sum(dims)).randn(*dims).astype(np.float32)
    for level in (0.0, 0.7, -1.3):
        _same(g, level)
    _same(g, 0.25, origin=(-0.5, 1.0, 2.0), spacing=(0.125, 0.5, 3.0))


def test_analytic_fields_match_the_restatement():
    v, f = _same(sphere(), 0.0)
    assert M.edge_pairing(f) == (True, True) and M.euler(v, f) == 2 and M.signed_volume(v, f) > 0
    v, f = _same(torus(), 0.0)
    assert M.edge_pairing(f) == (True, True) and M.euler(v, f) == 0
    g = np.round(sphere(24, 8.0, 11.5))                     # many corners exactly at the level
    v, f = _same(g, 0.0)
    assert M.edge_pairing(f) == (True, True)
    v, f = _same(np.zeros((9, 10, 11), np.float32), 0.0)     # empty
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.fixture(scope='module')
def full_generator():
    from inv3d_amd import synthetic as S
    G = S.make_generator(device=DEV)
    S.load_synthetic_weights(G, seed=0)
    ws = S.synth_ws(14, 512, 1, seed=3).to(DEV)
    return G, ws


def test_density_grid_128_matches_the_restatement(full_generator):
    from inv3d_amd import inference as INF
    G, ws = full_generator
    g = INF.density_grid(G, ws, res=128).cpu().numpy()
    inner = g[g > -999]
    for level in (10.0, float(np.quantile(inner, 0.5))):
        v, f = _same(g, level)
        print('128^3 level', level, 'V', len(v), 'F', len(f))
    assert len(f) > 0


def _pairing_on_device(f: torch.Tensor, nv: int):
    """(closed, oriented) with a device sort: every undirected edge in exactly two faces, each directed edge in exactly one."""
    f = f.long()
    d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = torch.minimum(d[:, 0], d[:, 1]) * nv + torch.maximum(d[:, 0], d[:, 1])
    _, cu = torch.unique(und, return_counts=True)
    _, cd = torch.unique(d[:, 0] * nv + d[:, 1], return_counts=True)
    return bool((cu == 2).all()), bool((cd == 1).all())


def test_full_size_grid_meshes(full_generator, tmp_path):
    from inv3d_amd import hipops as H, inference as INF
    G, ws = full_generator
    grid = INF.density_grid(G, ws, res=512)
    inner = grid[60:-60:4, 60:-60:4, 60:-60:4].reshape(-1)
    q = float(torch.quantile(inner[:1 << 24], 0.7))
    levels = [10.0, q]
    digests = {}
    for level in levels:
        v, f = H.marching_cubes(grid, level)
        v2, f2 = H.marching_cubes(grid, level)
        torch.cuda.synchronize()
        assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(f, f2)          # run to run
        print(f'512^3 level {level:.4f}: V {v.shape[0]} F {f.shape[0]}')
        if f.shape[0]:
            assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
            assert _pairing_on_device(f, v.shape[0]) == (True, True)
            # every vertex lies inside the grid, on a grid line (two of its three coordinates are integers)
            frac = (v - v.floor() != 0).sum(1)
            assert int(frac.max()) <= 1 and float(v.min()) >= 0 and float(v.max()) <= 511
        digests[repr(level)] = [v.shape[0], f.shape[0], hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest(),
                                hashlib.sha256(f.cpu().numpy().tobytes()).hexdigest()]
    assert digests[repr(q)][1] > 1_000_000, digests              # a large mesh
    # the deterministic build, in a fresh interpreter (tests/test_gpu_det.py): the same bytes
    path = str(tmp_path / 'grid.npy')
    np.save(path, grid.cpu().numpy())
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'mc_digest.py'), path] + [repr(l) for l in levels], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == digests


def _small_generator():
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    with torch.no_grad():
        target = G.synthesis(O.synth_ws(cfg, 1, seed=7).to(DEV), cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    return G, cam, target


def _read_ply(path):
    data = open(path, 'rb').read()
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode().splitlines()
    nv = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    nf = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    v = np.frombuffer(body[:nv * 12], '<f4').reshape(nv, 3)
    rec = np.frombuffer(body[nv * 12:], np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    assert len(rec) == nf and np.all(rec['n'] == 3)
    return v, rec['i']


def test_coach_gen_mesh(tmp_path):
    from inv3d_amd import inference as INF
    from inv3d_amd.coach import InversionCoach
    G, cam, target = _small_generator()
    res = 48
    kw = dict(first_inv_steps=3, max_pti_steps=3, lpips_threshold=0.0, seed=3, w_avg_samples=0, keep_tuned_state=True)
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    # default: no file, no mesh path
    before = set(os.listdir(os.getcwd()))
    r0 = InversionCoach(G, **kw).invert('a', target, cam)
    assert r0.mesh_path is None and set(os.listdir(os.getcwd())) == before and os.listdir(tmp_path) == []
    G.load_state_dict(pristine)
    # '.mrc': the tuned generator's density grid at the pivot latent
    d1 = str(tmp_path / 'mrc')
    coach = InversionCoach(G, gen_mesh=True, mesh_dir=d1, mesh_res=res, **kw)
    r1 = coach.invert('a', target, cam)
    assert r1.mesh_path == os.path.join(d1, 'a_pti.mrc') and os.listdir(d1) == ['a_pti.mrc']
    data = open(r1.mesh_path, 'rb').read()
    got = np.frombuffer(data[1024:], '<f4').reshape(res, res, res)
    G.load_state_dict(r1.tuned_state)
    want = INF.density_grid(G, r1.w_pivot, res=res).cpu().numpy()
    assert np.array_equal(got, want)
    assert not all(torch.equal(pristine[k], v) for k, v in r1.tuned_state.items())          # it is the tuned generator's shape
    # '.ply' at a level that gives a non-empty mesh
    inner = want[want > -999]
    level = float(np.quantile(inner, 0.6))
    G.load_state_dict(pristine)
    d2 = str(tmp_path / 'ply')
    r2 = InversionCoach(G, gen_mesh=True, mesh_dir=d2, mesh_res=res, mesh_level=level, mesh_format='.ply', **kw).invert('a', target, cam)
    assert r2.mesh_path == os.path.join(d2, 'a_pti.ply') and os.listdir(d2) == ['a_pti.ply']
    v, f = _read_ply(r2.mesh_path)
    G.load_state_dict(r2.tuned_state)
    ev, ef = INF.extract_mesh(G, r2.w_pivot, res=res, level=level)
    assert len(f) > 0
    assert np.array_equal(v, ev.cpu().numpy()) and np.array_equal(f, ef.cpu().numpy())
