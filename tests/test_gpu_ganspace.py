"""GANSpace latent editing on the GPU (csrc/pca.hip, hipops.pca_moments / pca_covariance / sym_eig / image_grid_u8, inv3d_amd/ganspace.py): the
shifted second moments against float64 with torch's own fp32 product as the yardstick, the Jacobi eigen-solver against float64 eigh, the fit against
the recorded output of the reference's estimator (tests/golden/ganspace.npz) and against tests/support/pca_ref.py on mapped latents, the uint8
grid against tests/support/grid_ref.py, the edits against separate synthesis calls, and normal-vs-deterministic-build identity."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
from pca_ref import pca_ref, sym_eig_ref  # noqa: E402
from grid_ref import grid_ref, tile_u8  # noqa: E402
from test_ganspace_cpu import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -23


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------------ moments
def _moment_data(S, D):
    rng = np.random.RandomState(1000 * D + S % 997)
    scale = 0.9 ** np.arange(D)
    return ((rng.randn(S, D) + 50.0) * scale).astype(np.float32)          # column mean = 50 x the column's spread


FLT_MIN = 2.0 ** -126


def _measure(C, C64, R):
    """max_ij |dC_ij| / sqrt(C_ii C_jj) over the entries fp32 can hold to relative precision.  With column scales 0.9^j and D = 512 the last
    columns' products lie below fp32's range (0.9^(i+j) < 2^-126 from i + j = 830; C_ii of column 511 is 1e-47, not an fp32 number), so a
    relative measure is 1 there for ANY fp32 result -- measured on MI355X: 1.0 for these kernels and for torch's product alike.  The error model
    with underflow is |fl(ab) - ab| <= eps |ab| + FLT_MIN: entries with sqrt(C_ii C_jj) < FLT_MIN / eps (where the second term dominates)
    are held to the absolute form |dC_ij| <= R eps sqrt(C_ii C_jj) + FLT_MIN instead, all others to the relative measure.  A zero denominator
    (a constant column) has to be exact."""
    den = np.sqrt(np.outer(np.diag(C64), np.diag(C64)))
    d = np.abs(np.asarray(C, dtype=np.float64) - C64)
    assert np.all(d[den == 0] == 0)
    tiny = (den > 0) & (den < FLT_MIN / EPS)
    assert np.all(d[tiny] <= R * EPS * den[tiny] + FLT_MIN)
    rel = den >= FLT_MIN / EPS
    return float((d[rel] / den[rel]).max()) if np.any(rel) else 0.0


@pytest.mark.parametrize('S,D', [(1, 1), (7, 5), (64, 64), (1000, 33), (4099, 96), (3000, 512)])
def test_moments(S, D):
    """Measured on MI355X, in units of eps32 (one chunk / three chunks / torch's fp32 product): 0 / 0 / 0, 0.29 / 0.53 / 0.79, 3.31 / 1.44 / 3.31,
    2.35 / 2.42 / 7.78, 1.66 / 1.49 / 21.93, 1.69 / 2.10 / 21.29 (table in DESIGN.md 3.4)."""
    from inv3d_amd import hipops as H
    X = _moment_data(S, D)
    x = _dev(X)
    shift = x[:256].mean(0)
    X64 = X.astype(np.float64)
    R = min(S, H.PCA_SLAB_ROWS)                                            # the rows one fp32 sum runs over
    mean64 = X64.mean(0)
    C64 = (X64 - mean64).T @ (X64 - mean64) / S
    # the yardstick: torch's own fp32 product about the same shift, against the float64 second moment about that shift
    xs = x - shift
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    try:
        M32 = (xs.T @ xs / S).cpu().numpy()
    finally:
        torch.set_float32_matmul_precision(old)
    xs64 = xs.cpu().numpy().astype(np.float64)
    yard = _measure(M32, xs64.T @ xs64 / S, S)
    slabs = H.pca_moments_slabs(S, D)
    assert slabs == -(-S // H.PCA_SLAB_ROWS)
    cuts = sorted({0, S // 5, S // 5 + (S - S // 5) // 3, S})              # three unequal chunks where S allows
    results = []
    for bounds in ([0, S], cuts):
        st = None
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            st = H.pca_moments(x[lo:hi], shift, st)
        cov, mean, n = H.pca_covariance(st)
        assert n == S and cov.shape == (D, D) and mean.shape == (D,) and cov.dtype == mean.dtype == torch.float32
        assert torch.equal(cov, cov.T)                                     # bit-symmetric
        err = _measure(cov.cpu().numpy(), C64, R)
        print(f'moments S {S} D {D} chunks {len(bounds) - 1}: err {err / EPS:.3f} eps, torch fp32 product {yard / EPS:.3f} eps, R {R}')
        results.append((err, cov, mean))
    for err, cov, mean in results:
        assert err <= 2 * yard, (err, yard)
        assert err <= R * EPS
        assert np.abs(mean.cpu().numpy().astype(np.float64) - mean64).max() <= 4 * EPS * np.abs(mean64).max()
    st = H.pca_moments(x, shift)
    cov2, mean2, _ = H.pca_covariance(st)
    assert torch.equal(cov2, results[0][1]) and torch.equal(mean2, results[0][2])         # run to run


def test_moments_strided_rows_and_errors():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    X = _moment_data(300, 40)
    x = _dev(X)
    shift = x[:, :33].mean(0)
    a = H.pca_covariance(H.pca_moments(x[:, :33], shift))                  # leading dimension 40
    b = H.pca_covariance(H.pca_moments(x[:, :33].contiguous(), shift))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(Eg3dHipError):
        H.pca_moments(torch.zeros(4, 513, device=DEV), torch.zeros(513, device=DEV))
    with pytest.raises(Eg3dHipError):
        H.pca_moments(x, shift[:5])
    with pytest.raises(Eg3dHipError):
        H.pca_moments(x[:, :20], None, H.pca_moments(x[:, :33], shift))


# ------------------------------------------------------------------------------------------------------------------------------------ eigen-solver
def _geometric(n, decay, seed=0):
    rng = np.random.RandomState(seed + n)
    q, _ = np.linalg.qr(rng.randn(n, n))
    a = (q * decay ** np.arange(n)) @ q.T
    return ((a + a.T) / 2).astype(np.float32)


def _check_eig(a, geometric=False, max_sweeps=60):
    """Solves a on the GPU and checks it against float64 eigh of the same fp32 matrix; returns what it measured in units of u = n eps32."""
    from inv3d_amd import hipops as H
    n = a.shape[0]
    ad = _dev(a)
    evals, evecs, sweeps, converged = H.sym_eig(ad, max_sweeps=max_sweeps)
    evals2, evecs2, sweeps2, _ = H.sym_eig(ad, max_sweeps=max_sweeps)
    assert torch.equal(evals, evals2) and torch.equal(evecs, evecs2) and sweeps == sweeps2          # run to run
    lam, vec = evals.cpu().numpy(), evecs.cpu().numpy()
    assert lam.shape == (n,) and vec.shape == (n, n) and lam.dtype == vec.dtype == np.float32
    assert converged and sweeps <= 60
    rl, rv = sym_eig_ref(a)
    u, lmax = n * EPS, float(np.abs(rl).max())
    l64, v64, a64 = lam.astype(np.float64), vec.astype(np.float64), a.astype(np.float64)
    e_val = float(np.abs(l64 - rl).max())
    e_res = float(np.abs(a64 @ v64.T - v64.T * l64).max())
    e_orth = float(np.abs(v64 @ v64.T - np.eye(n)).max())
    scale = u * lmax if lmax > 0 else 1.0
    print(f'sym_eig n {n}: sweeps {sweeps}, eigenvalues {e_val / scale:.2f} u lmax, residual {e_res / scale:.2f} u lmax, orthogonality {e_orth / u:.2f} u')
    assert e_val <= 4 * u * lmax and e_res <= 4 * u * lmax and e_orth <= 12 * u
    assert np.all(np.diff(lam) <= 0)                                       # descending
    piv = np.argmax(np.abs(vec), axis=1)                                   # the first of equals
    assert np.all(vec[np.arange(n), piv] > 0)                              # the sign rule
    if geometric:
        k = min(16, n)
        for i in range(k):
            gap = min((abs(rl[i] - rl[j]) for j in range(n) if j != i), default=np.inf)
            cos = abs(float(v64[i] @ rv[i])) / (np.linalg.norm(v64[i]) * np.linalg.norm(rv[i]))
            assert 1 - cos <= (4 * u * lmax / gap) ** 2 / 2 + 4 * 2.0 ** -52, (i, 1 - cos, gap)          # (+ the float64 rounding of the cosine itself)
    return lam, vec, sweeps


@pytest.mark.parametrize('n,decay', [(1, 0.7), (2, 0.7), (3, 0.7), (8, 0.7), (33, 0.8), (64, 0.8), (65, 0.8), (96, 0.9), (512, 0.97)])
def test_sym_eig_geometric(n, decay):
    """Measured on MI355X over all cases of this file: eigenvalues at most 0.84 u lmax (n = 512), residual 0.37 u lmax, orthogonality 0.55 u
    (both n = 2); 22 sweeps at n = 512 (table in DESIGN.md 3.4).  The cosine is normalised in float64: fp32 unit rows alone leave 1e-7 in
    1 - cos, four orders above the bound at n = 2."""
    _check_eig(_geometric(n, decay), geometric=True)


def test_sym_eig_identity_and_sorted_output():
    lam, vec, sweeps = _check_eig(np.eye(33, dtype=np.float32))
    assert sweeps <= 1 and np.array_equal(vec, np.eye(33, dtype=np.float32)) and np.all(lam == 1)          # no rotation is applied
    d = np.arange(1, 21, dtype=np.float32)
    lam, vec, sweeps = _check_eig(np.diag(d))                              # ascending diagonal: the final sort
    assert np.array_equal(lam, d[::-1]) and np.array_equal(vec, np.eye(20, dtype=np.float32)[::-1])


def test_sym_eig_rank_deficient():
    rng = np.random.RandomState(3)
    z = rng.randn(10, 10)
    z = z @ z.T
    z[3] = 0
    z[:, 3] = 0
    lam, _, _ = _check_eig(z.astype(np.float32))                           # a zero row and column
    assert lam[-1] == 0 or abs(lam[-1]) <= 4 * 10 * EPS * lam[0]
    x = rng.randn(40, 64) * 0.85 ** np.arange(64) + 3
    c = np.cov(x.T, bias=True)
    _check_eig(((c + c.T) / 2).astype(np.float32))                         # rank 39 in 64 dimensions


def test_sym_eig_sweep_limit_is_a_status():
    from inv3d_amd import hipops as H
    a = _geometric(96, 0.9)
    evals, evecs, sweeps, converged = H.sym_eig(_dev(a), max_sweeps=1)
    assert sweeps == 1 and converged is False
    assert bool(torch.isfinite(evals).all()) and bool(torch.isfinite(evecs).all())
    assert np.all(np.diff(evals.cpu().numpy()) <= 0)


# ------------------------------------------------------------------------------------------------------------------------------------ fit
def _check_fit(res, want_comp, want_stdev, D, min_rel_gap=None):
    u = D * EPS
    lam = np.asarray(want_stdev, dtype=np.float64) ** 2
    comp, stdev = res.components.cpu().numpy().astype(np.float64), res.stdev.cpu().numpy().astype(np.float64)
    assert np.abs(stdev - want_stdev).max() <= 4 * u * want_stdev[0] + 1e-6
    assert abs(float(res.var_ratio.double().sum()) - 1) <= 1e-5 or res.components.shape[0] < D
    checked = 0
    for i in range(comp.shape[0]):
        gap = min(abs(lam[i] - lam[j]) for j in range(len(lam)) if j != i)
        if min_rel_gap is not None and not gap / lam[i] > min_rel_gap:
            continue
        err = np.abs(comp[i] - want_comp[i]).max()
        assert err <= 4 * u * lam[0] / gap + 4e-6, (i, err, gap)
        checked += 1
    return checked


def test_fit_pca_matches_the_reference_estimator():
    from inv3d_amd import ganspace as GS
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ganspace.npz'))
    x = _dev(g['X'])
    for chunks in (x, [x[i:i + 128] for i in range(0, 400, 128)]):
        res = GS.fit_pca(chunks)
        assert res.converged and res.n_samples == 400 and res.components.shape == (24, 24)
        assert _check_fit(res, g['components'].astype(np.float64), g['stdev'].astype(np.float64), 24) == 24
        assert abs(res.total_var - float(g['total_var'])) <= 1e-5 * float(g['total_var'])
        # var_ratio = stdev^2 / total_var: twice the relative bound on stdev, times a ratio that is at most 1
        assert np.abs(res.var_ratio.cpu().numpy() - g['var_ratio']).max() <= 8 * 24 * EPS + 1e-6
        mean64 = g['X'].astype(np.float64).mean(0)
        assert np.abs(res.mean.cpu().numpy() - mean64).max() <= 4 * EPS * np.abs(mean64).max()
    top, full = GS.fit_pca(x, n_components=5), GS.fit_pca(x)
    assert top.components.shape == (5, 24) and torch.equal(top.components, full.components[:5]) and top.stdev.shape == (5,)


_SMALL = {}


def _small():
    """The small synthetic generator of tests/test_gpu_mesh.py, with pinned sampling uniforms so that separate synthesis calls can be compared."""
    if not _SMALL:
        from inv3d_amd import synthetic as S
        from oracle import eg3d_oracle as O
        cfg = O.small_config()
        G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                             rendering_kwargs=cfg.rendering, device=DEV)
        S.load_synthetic_weights(G, 0)
        for p in G.parameters():
            p.requires_grad_(False)
        u1, u2 = O.make_uniforms(cfg, 1, seed=4)
        _SMALL.update(G=G, cam=O.synth_cameras(1, seed=2).float().to(DEV), w=O.synth_ws(cfg, 1, seed=7).float().to(DEV),
                      kw=dict(noise_mode='const', force_fp32=True, render_uniforms=(u1.to(DEV), u2.to(DEV))))
    return _SMALL


FIT_SEED = 0


def test_fit_w_pca_on_mapped_latents():
    from inv3d_amd import ganspace as GS
    G = _small()['G']
    chunks = list(GS.sample_w(G, 4000, seed=FIT_SEED, chunk=1024))
    assert [tuple(c.shape) for c in chunks] == [(1024, 32)] * 3 + [(928, 32)]
    again = list(GS.sample_w(G, 4000, seed=FIT_SEED, chunk=1024))
    assert all(torch.equal(a, b) for a, b in zip(chunks, again))           # reproducible for a seed
    assert not torch.equal(chunks[0], next(GS.sample_w(G, 1024, seed=FIT_SEED + 1, chunk=1024)))
    ref = pca_ref(torch.cat(chunks).cpu().numpy())
    lam = ref['evals']
    rel_gap = [min(abs(lam[i] - lam[j]) for j in range(32) if j != i) / lam[i] for i in range(32)]
    print('relative eigenvalue gaps of the reference:', ' '.join(f'{g:.3f}' for g in rel_gap))
    assert all(g > 0.05 for g in rel_gap[:4])                              # a property of the data, not of the code under test
    res = GS.fit_w_pca(G, n_samples=4000, n_components=32, seed=FIT_SEED, chunk=1024)
    assert res.n_samples == 4000 and res.converged
    assert _check_fit(res, ref['components'], ref['stdev'], 32, min_rel_gap=0.05) >= 4
    assert np.abs(res.mean.cpu().numpy() - ref['mean']).max() <= 4 * EPS * np.abs(ref['mean']).max()


# ------------------------------------------------------------------------------------------------------------------------------------ grid
def _grid_input(N, H, W, seed):
    rng = np.random.RandomState(seed)
    img = (rng.randn(N, 3, H, W) * 1.5).astype(np.float32)                 # a fair share outside [-1, 1]
    flat = img.reshape(-1)
    special = np.array([-0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 1e9, -1e9, np.float32(-128 / 127.5), np.float32(127 / 127.5)]
                       + [(k - 128) / 127.5 for k in (0, 1, 64, 128, 200, 255)] + [k / 127.5 + 2.0 ** -20 for k in (-3, 5)], dtype=np.float32)
    pos = rng.permutation(flat.size)[:special.size]                        # (several of these land exactly on integers after * 127.5 + 128)
    flat[pos] = special[:pos.size]
    return img


@pytest.mark.parametrize('N,nrow,H,W,padding', LAYOUTS)
def test_image_grid_u8(N, nrow, H, W, padding):
    from inv3d_amd import hipops as H_
    img = _grid_input(N, H, W, seed=N * 31 + H)
    for pad_value in (0, 200):
        got = H_.image_grid_u8(_dev(img), nrow, padding=padding, pad_value=pad_value)
        assert got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), grid_ref(img, nrow, padding, pad_value))
    cl = _dev(img).contiguous(memory_format=torch.channels_last)           # what the generator returns
    assert np.array_equal(H_.image_grid_u8(cl, nrow, padding=padding).cpu().numpy(), grid_ref(img, nrow, padding))


# ------------------------------------------------------------------------------------------------------------------------------------ edits
def _u8_diff(a, b):
    return int((a.to(torch.int16) - b.to(torch.int16)).abs().max())


def test_edit_ganspace_and_orbit():
    from inv3d_amd import ganspace as GS, hipops as H, inference as INF
    s = _small()
    G, cam, w, kw = s['G'], s['cam'], s['w'], s['kw']
    num_ws = w.shape[1]
    comp = np.linalg.qr(np.random.RandomState(9).randn(32, 32))[0][:6].astype(np.float32)
    args = dict(idx_comp=2, start_layer=1, layer_num=min(5, num_ws - 1), edit_power=3.0, num_imgs=3)
    out = GS.edit_ganspace(G, comp, w, cam, synth_kwargs=kw, **args)
    want_d = GS.edit_directions(comp, num_ws=num_ws, **args).to(DEV)
    assert torch.equal(out['directions'], want_d) and torch.equal(out['ws'], w + want_d)
    assert out['images'].dtype == torch.uint8 and out['images'].shape[0] == 3 and out['images'].shape[-1] == 3

    def direct(i, c):
        with torch.no_grad():
            return H.image_grid_u8(G.synthesis(out['ws'][i:i + 1], c, **kw)['image'].float(), nrow=1, padding=0)

    # the allowance: what two identical separate calls differ by (0 = bit identity is required)
    allow = max(_u8_diff(direct(i, cam), direct(i, cam)) for i in range(3))
    print('uint8 difference between two identical synthesis calls:', allow)
    for i in range(3):
        assert out['images'][i].shape == direct(i, cam).shape
        assert _u8_diff(out['images'][i], direct(i, cam)) <= allow
    assert _u8_diff(out['images'][0], out['images'][2]) > allow            # the edit does something
    assert np.array_equal(out['grid'].cpu().numpy(), tile_u8(out['images'].cpu().numpy(), nrow=8, padding=2))
    cams = INF.orbit_cameras(3, device=DEV)
    orbit = GS.edit_orbit(G, comp, w, num_frames=3, cameras=cams, synth_kwargs=kw, **args)
    assert orbit.dtype == torch.uint8 and tuple(orbit.shape) == (3, 3) + tuple(out['images'].shape[1:])
    for i in range(3):
        assert _u8_diff(orbit[i, 0], direct(i, cams[:1])) <= allow


def test_run_ganspace_tool_writes_the_grid(tmp_path):
    """tools/run_ganspace.py fit, then edit, on the small generator: the PNG decodes to the grid the edit computed."""
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location('run_ganspace_tool', os.path.join(ROOT, 'tools', 'run_ganspace.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    s = _small()
    comp_path, out_dir = str(tmp_path / 'comp.npy'), str(tmp_path / 'edits')
    res = tool.main(['fit', '--synthetic', 'small', '--samples', '2000', '--chunk', '512', '--out', comp_path])
    assert np.load(comp_path).shape == (32, 32) and res.converged
    np.save(str(tmp_path / 'a_ws.npy'), s['w'].cpu().numpy())
    np.save(str(tmp_path / 'a_cam.npy'), s['cam'].cpu().numpy())
    out = tool.main(['edit', '--synthetic', 'small', '--components', comp_path, '--ws', str(tmp_path / 'a_ws.npy'), '--cam', str(tmp_path / 'a_cam.npy'),
                     '--params', '1', '0', '3', '2.5', '--num-imgs', '3', '--out-dir', out_dir, '--name', 'a', '--save-images'])
    assert sorted(os.listdir(out_dir)) == ['a_grid.png', 'a_inter_1.png', 'a_inter_2.png', 'a_inter_3.png']
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, 'a_grid.png'))), out['grid'].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, 'a_inter_2.png'))), out['images'][1].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------------ build identity
def test_both_builds_give_the_same_bits():
    """csrc/pca.hip accumulates nothing with atomics: the deterministic build, in a fresh interpreter, prints the digests this process computes."""
    import pca_digest
    here = pca_digest.digests()
    assert here['converged']
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'pca_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here
