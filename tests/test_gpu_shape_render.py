"""Shape views on the GPU (csrc/iso_render.hip, hipops.iso_bricks / iso_render, inference.render_shape, the shape option of the media
writers): every output EQUALS the numpy restatement tests/support/iso_ref.py bit for bit, with empty-space skipping on and off; the frames
register with the package's own rays; the generator-level path, the side-by-side orbit video and the two-row pivot grid."""
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import iso_ref as R  # noqa: E402
from test_video_cpu import check_avi  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K9 = [4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.]


def _cam(m, focal=4.2647):
    k = list(K9)
    k[0] = k[4] = focal
    return torch.cat([torch.as_tensor(m, dtype=torch.float32).reshape(16), torch.tensor(k)]).reshape(1, 25)


def cameras():
    """canonical (exact entries: with an odd res the centre ray is exactly (0,0,-1), two direction components exactly 0), two lookat_pose
    views, one camera inside the box, one whose rays all miss it."""
    from inv3d_amd.inference import lookat_pose
    canonical = _cam([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2.7], [0, 0, 0, 1]])
    return dict(canonical=canonical,
                look_a=_cam(lookat_pose(math.pi / 2 + 0.35, math.pi / 2 - 0.25, (0., 0., 0.), 2.7)),
                look_b=_cam(lookat_pose(math.pi / 2 - 0.8, math.pi / 2 + 0.4, (0.05, -0.02, 0.), 1.9), focal=2.0),
                inside=_cam(lookat_pose(0.3, 1.1, (0., 0., 0.), 0.3), focal=1.0),
                miss=_cam(lookat_pose(math.pi / 2, math.pi / 2, (0., 10., 0.), 2.7)))


VIEWS = [(37, ('canonical', 'look_a', 'inside')), (8, ('miss',)), (8, ('look_b', 'canonical', 'miss')), (37, ('canonical',))]      # res 8 | 37, F 1 | 3


def _sphere(noise=0.0):
    i = np.arange(64, dtype=np.float64) - 31.5
    f = 20.0 - np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    if noise:
        f = f + np.random.RandomState(0).normal(0.0, noise, f.shape)
    return f.astype(np.float32)


def _frame(shape, flip0=False, axes=(0, 1, 2)):
    """the grid spans [-0.5, 0.5] along each of its world axes (anisotropic spacing unless it is a cube)"""
    sp = [1.0 / (d - 1) for d in shape]
    org = [-0.5] * 3
    if flip0:
        sp[0], org[0] = -sp[0], 0.5
    return dict(origin=tuple(org), spacing=tuple(sp), axes=axes)


def grids():
    rng = np.random.RandomState(3)
    padded = _sphere(0.3)
    for s in (np.s_[:3], np.s_[-3:]):
        padded[s] = padded[:, s] = padded[:, :, s] = -1000.0
    padded[rng.randint(0, 64, 300), rng.randint(0, 64, 300), rng.randint(0, 64, 300)] = np.nan
    padded[20:24, 30:40, 8:30] = np.nan
    g = {
        '2x2x2': (rng.normal(size=(2, 2, 2)).astype(np.float32), _frame((2, 2, 2))),
        '17x17x17': (rng.normal(size=(17, 17, 17)).astype(np.float32), _frame((17, 17, 17))),           # the cells end exactly on a brick boundary
        '37x53x61': (rng.normal(size=(37, 53, 61)).astype(np.float32), _frame((37, 53, 61))),
        'sphere': (_sphere(), _frame((64, 64, 64))),
        'noisy_sphere': (_sphere(0.3), _frame((64, 64, 64))),
        'negative_spacing': (_sphere(0.3), _frame((64, 64, 64), flip0=True)),
        'permuted_axes': (rng.normal(size=(37, 53, 61)).astype(np.float32), _frame((37, 53, 61), flip0=True, axes=(2, 0, 1))),
        'nan_and_padding': (padded, _frame((64, 64, 64))),
    }
    return g


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _gpu(vol, cams, res, level, frame, **kw):
    from inv3d_amd import hipops as H
    out = H.iso_render(vol, cams.to(DEV), res, level, want_hit_k=True, **frame, **kw)
    torch.cuda.synchronize()
    o = {k: out[k].cpu().numpy() for k in ('depth', 'normal', 'mask', 'hit_k', 'shade')}
    o['shade'] = np.ascontiguousarray(o['shade'].transpose(0, 2, 3, 1))       # channel last, as the restatement
    return o


def _assert_equal(got, want, what):
    for k in ('mask', 'hit_k', 'depth', 'normal', 'shade'):
        a, b = _bits(got[k]).reshape(-1), _bits(np.asarray(want[k])).reshape(-1)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), got[k].reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])


@pytest.mark.parametrize('name', sorted(grids()))
def test_outputs_equal_the_restatement(name):
    """mask, hit_k, depth, normal, shade: GPU with skipping == GPU without == the fp32 restatement, bit for bit; levels 0, 0.7 and one above
    the grid's maximum (every ray misses); res 8 and 37, 1 and 3 cameras, both shade modes."""
    from inv3d_amd import hipops as H
    vol, frame = grids()[name]
    vd = torch.from_numpy(vol).to(DEV)
    bricks = H.iso_bricks(vd)
    assert np.array_equal(_bits(bricks.cpu().numpy()), _bits(R.bricks(vol)))
    cams = cameras()
    hits = 0
    for level in (0.0, 0.7, float(np.nanmax(vol)) + 1.0):
        for i, (res, names) in enumerate(VIEWS):
            c = torch.cat([cams[n] for n in names])
            kw = dict(shade='normal', background=-0.25, ambient=0.3, refine=3) if i == 2 else {}
            on = _gpu(vd, c, res, level, frame, skip=True, bricks=bricks, **kw)
            off = _gpu(vd, c, res, level, frame, skip=False, **kw)
            _assert_equal(on, off, (name, level, res, names, 'skip on vs off'))
            want = R.march(vol, c.numpy(), res, level, skip=True, **frame, **kw)
            _assert_equal(on, want, (name, level, res, names, 'gpu vs restatement'))
            if level > 0.7:
                assert on['mask'].sum() == 0 and (on['hit_k'] == -1).all() and (on['depth'] == 0).all()
            if 'miss' in names:
                assert on['mask'].reshape(len(names), -1)[names.index('miss')].sum() == 0
            hits += int(on['mask'].sum())
    assert hits > 0


def test_registration_with_the_ray_sampler():
    """A planar field level + (z0 - z_world) on a 33^3 grid: the points o + depth * d, with o and d from the package's own RaySampler for the
    same c, lie on the plane z = z0 within 1e-5 world units (1/200 of a voxel at 512^3; the fp32 spacing at magnitude 3 is 2.4e-7, through
    about a dozen operations) -- the rays are RaySampler's, the depth is a distance along its unit direction."""
    from inv3d_amd import hipops as H
    from inv3d_amd.training.volumetric_rendering.ray_sampler import RaySampler
    z0, level, res = 0.1, 3.0, 32
    cams = cameras()
    c = torch.cat([cams['canonical'], cams['look_a'], _cam(cams['look_a'][0, :16], focal=3.0)]).to(DEV)
    for frame in (_frame((33, 33, 33), flip0=True), _frame((33, 33, 33), axes=(1, 2, 0))):
        a = frame['axes'].index(2)                                             # the grid axis that runs along world z
        zw = frame['origin'][a] + np.arange(33, dtype=np.float64) * frame['spacing'][a]
        shape = [1, 1, 1]
        shape[a] = 33
        vol = np.broadcast_to((level + (z0 - zw)).reshape(shape), (33, 33, 33)).astype(np.float32)
        out = H.iso_render(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), c, res, level, **frame)
        o, d = RaySampler()(c[:, :16].view(-1, 4, 4), c[:, 16:25].view(-1, 3, 3), res)
        assert bool(out['mask'].all())
        pts = o.double() + d.double() * out['depth'].reshape(3, res * res, 1).double()
        err = float((pts[..., 2] - z0).abs().max())
        print(f'registration: worst |z - z0| = {err:.2e}')
        assert err < 1e-5
        # the normal of the plane's dense side points to +z
        assert float((out['normal'][..., 2] - 1).abs().max()) < 1e-5


def test_the_kernel_tests_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs the restatement and registration tests of this file
    again: csrc/iso_render.hip accumulates nothing, so the other build must give the same bits."""
    import subprocess
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', '-k', 'restatement or registration',
                        os.path.join('tests', 'test_gpu_shape_render.py')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '9 passed' in r.stdout, r.stdout[-1000:]


@pytest.fixture(scope='module')
def full_generator():
    from inv3d_amd import synthetic as S
    G = S.make_generator(device=DEV)
    S.load_synthetic_weights(G, 0)
    for p in G.parameters():
        p.requires_grad_(False)
    return G, S.synth_ws(G.backbone.num_ws, G.w_dim, 1).to(DEV)


def test_generator_level(full_generator):
    """The synthetic full-size generator, density_grid(res=128), the level at the grid's 0.7 quantile (seeded weights do not reach 10), 128^2
    pixels, 4 orbit cameras: some rays hit and some miss, skipping on == off, 4096 seeded pixels == the restatement, two runs identical.

    The orbit's default focal length (4.2647) frames +-0.32 world units at the centre plane, inside the un-padded part of the grid (+-0.38):
    every ray crosses the seeded generator's noise-like density and meets a value above its 0.7 quantile -- measured, 65536 of 65536 pixels
    hit.  Those four cameras are rendered and compared like the rest; the hit / miss mixture is asserted on four orbit cameras of focal
    length 2 (orbit_cameras(4, focal=2.0)), whose frames reach beyond the box, so their outer rays miss it."""
    from inv3d_amd import inference as INF
    G, ws = full_generator
    grid = INF.density_grid(G, ws, res=128)
    level = float(torch.quantile(grid.reshape(-1), 0.7))
    cams = torch.cat([INF.orbit_cameras(4, device=DEV), INF.orbit_cameras(4, focal=2.0, device=DEV)])
    F = cams.shape[0]
    a = INF.render_shape(G, ws, cams, res=128, level=level, grid=grid, want_hit_k=True)
    b = INF.render_shape(G, ws, cams, res=128, level=level, grid=grid, want_hit_k=True, skip=False)
    c = INF.render_shape(G, ws, cams, res=128, level=level, grid=grid, want_hit_k=True, bricks=a['bricks'])
    n_default, n = int(a['mask'][:4].sum()), int(a['mask'][4:].sum())
    print(f'generator level: {n_default} of {a["mask"][:4].numel()} pixels hit at the default focal length, {n} of {a["mask"][4:].numel()} at focal 2')
    assert n_default > 0 and 0 < n < a['mask'][4:].numel(), (n_default, n)
    tb = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for k in ('depth', 'normal', 'mask', 'hit_k', 'shade'):
        assert torch.equal(tb(a[k]), tb(b[k])), k
        assert torch.equal(tb(a[k]), tb(c[k])), k
    assert a['shade'].shape == (F, 3, 128, 128) and float(a['shade'].abs().max()) <= 1.0 + 1e-6
    pix = np.sort(np.random.RandomState(5).choice(F * 128 * 128, 4096, replace=False))
    origin, spacing, axes = INF.grid_frame(G, 128)
    want = R.march(grid.cpu().numpy(), cams.cpu().numpy(), 128, level, origin, spacing, axes, pix=pix)
    got = dict(depth=a['depth'].reshape(-1)[pix], normal=a['normal'].reshape(-1, 3)[pix], mask=a['mask'].reshape(-1)[pix], hit_k=a['hit_k'].reshape(-1)[pix],
               shade=a['shade'].permute(0, 2, 3, 1).reshape(-1, 3)[pix])
    _assert_equal({k: v.cpu().numpy() for k, v in got.items()}, want, 'generator level')
    # default res = the generator's image resolution
    d = INF.render_shape(G, ws, cams[:1], level=level, grid=grid, bricks=a['bricks'])
    assert d['shade'].shape == (1, 3, G.img_resolution, G.img_resolution)
    frames = list(INF.render_shape_orbit(G, ws, cameras=cams, res=128, level=level, grid=grid))
    assert len(frames) == F and all(torch.equal(f, a['shade'][i]) for i, f in enumerate(frames))


def _small_generator():
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    for p in G.parameters():
        p.requires_grad_(False)
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    ws = O.synth_ws(cfg, 1, seed=7).to(DEV)
    uni = tuple(u.to(DEV) for u in O.make_uniforms(cfg, 1, seed=4))        # pinned stratified-sampling draws: two renders give the same frame
    return G, ws, cam, uni


@pytest.fixture(scope='module')
def small():
    from inv3d_amd import inference as INF
    G, ws, cam, uni = _small_generator()
    grid = INF.density_grid(G, ws, res=64)
    return G, ws, cam, uni, grid, float(torch.quantile(grid.reshape(-1), 0.7))


def _decode(b):
    from PIL import Image
    im = Image.open(io.BytesIO(b))
    im.load()
    return np.asarray(im).astype(np.int32)


def test_orbit_video_with_shape(tmp_path, small):
    """shape=True: 4 frames of twice the width, image | shape.  The frame width is a multiple of the 4:2:0 MCU (16), so the left half's blocks
    carry exactly the coefficients of the plain frame's: decoded, the two differ only where the decoder's chroma upsampling looks across the
    seam (the last two columns).  shape=False writes the bytes of the old call signature."""
    from inv3d_amd import hipops as H, inference as INF, video as V
    G, ws, _, uni, grid, level = small
    kw = dict(num_frames=4, fps=30, quality=85, batch=3, force_fp32=True, render_uniforms=uni)
    plain, old, both = str(tmp_path / 'plain.avi'), str(tmp_path / 'old.avi'), str(tmp_path / 'both.avi')
    assert V.write_orbit_video(G, ws, plain, shape=False, **kw) == 4
    assert V.write_orbit_video(G, ws, old, **kw) == 4
    assert open(plain, 'rb').read() == open(old, 'rb').read()
    assert V.write_orbit_video(G, ws, both, shape=True, shape_kwargs=dict(grid=grid, level=level), **kw) == 4
    hh = ww = G.img_resolution
    assert ww % 16 == 0
    a = check_avi(open(both, 'rb').read(), 4, 30, 2 * ww, hh)
    p = check_avi(open(plain, 'rb').read(), 4, 30, ww, hh)
    shapes = list(INF.render_shape_orbit(G, ws, num_frames=4, res=ww, level=level, grid=grid))
    for i in range(4):
        wide, single = _decode(a['frames'][i]), _decode(p['frames'][i])
        assert wide.shape == (hh, 2 * ww, 3) and single.shape == (hh, ww, 3)
        assert np.array_equal(wide[:, :ww - 2], single[:, :ww - 2])
        # the right half is the shape frame: against a separate encode of it, away from the seam
        data, _ = H.jpeg_encode(shapes[i][None], quality=85)
        right = _decode(data.cpu().numpy().tobytes())
        assert np.array_equal(wide[:, ww + 2:], right[:, 2:])
    assert 0 < sum(int((s < 0.99).sum()) for s in shapes)                   # not all background
    # the grid built inside (one per video) gives the same file as the grid passed in
    inner = str(tmp_path / 'inner.avi')
    assert V.write_orbit_video(G, ws, inner, shape=True, shape_kwargs=dict(grid_res=64, level=level), **kw) == 4
    assert open(inner, 'rb').read() == open(both, 'rb').read()


def test_pivot_grid_with_shape(small):
    from inv3d_amd import hipops as H, video as V
    G, ws, cam, uni, grid, level = small
    with torch.no_grad():
        target = G.synthesis(ws, cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    one = V.pivot_grid(G, ws, cam, target, render_uniforms=uni, force_fp32=True)
    same = V.pivot_grid(G, ws, cam, target, shape=False, render_uniforms=uni, force_fp32=True)
    two = V.pivot_grid(G, ws, cam, target, shape=True, shape_kwargs=dict(grid=grid, level=level, background=0.5), render_uniforms=uni, force_fp32=True)
    hh, ww = target.shape[-2:]
    assert torch.equal(one, same) and tuple(one.shape) == (*H.image_grid_size(5, hh, ww, 5), 3)
    assert tuple(two.shape) == (*H.image_grid_size(10, hh, ww, 5), 3) and two.shape[0] == 2 * (hh + 2) + 2
    assert torch.equal(two[:one.shape[0]], one)
    cell = two[hh + 4:2 * hh + 4, 2:2 + ww]                                  # under the target: background 0.5 -> uint8(0.5 * 127.5 + 128) = 191
    assert bool((cell == 191).all())
    views = two[hh + 4:2 * hh + 4, ww + 4:]
    assert bool((views != 191).any())


def test_coach_shape_views(tmp_path, small):
    """InversionCoach(shape_views=True) hands the option to both writers: two-row grids, double-width videos (defaults: 512^3 grid, level 10)."""
    from PIL import Image
    from inv3d_amd import hipops as H
    from inv3d_amd.coach import InversionCoach
    G, ws, cam, uni, _, _ = small
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        target = G.synthesis(ws, cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    d = str(tmp_path / 'media')
    try:
        r = InversionCoach(G, first_inv_steps=2, max_pti_steps=2, lpips_threshold=0.0, seed=3, w_avg_samples=0, synth_kwargs=dict(render_uniforms=uni),
                           save_grid=True, gen_video=True, media_dir=d, shape_views=True).invert('a', target, cam)
    finally:
        G.load_state_dict(pristine)
    hh, ww = target.shape[-2:]
    for p in r.grid_paths:
        assert np.asarray(Image.open(p)).shape == (*H.image_grid_size(10, hh, ww, 5), 3)
    for p in r.video_paths:
        check_avi(open(p, 'rb').read(), 240, 60, 2 * ww, hh)
