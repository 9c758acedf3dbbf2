"""GPU tests of the grid components (csrc/grid_components.hip; include/eg3d_hip.h "Grid components"): hipops.grid_components must equal the
numpy restatement tests/support/cc_ref.py exactly -- labels, sizes, roots and counts, connectivity 6 and 26 -- and hipops.grid_keep must equal
np.where byte for byte.  Then the layers above: clean_grid's subset property under marching cubes, and the keep option through extract_mesh,
render_shape, render_shape_orbit, color_mesh and the coach."""
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
import cc_cases as CS  # noqa: E402
import cc_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _tile():
    from inv3d_amd import _lib as L
    return tuple(L.CC_TILE)


def _shapes():
    t = _tile()
    return [(1, 1, 1), (2, 3, 5), (33, 17, 9), (9, 17, 33), (40, 40, 40), tuple(2 * e + 1 for e in t)]


CONTENTS = ['all_inside', 'all_outside', 'one_voxel', 'random_0.1', 'random_0.3', 'random_0.5', 'checkerboard', 'specials']
_REF = {}


def _ref(key, vol, level, conn):
    """the restatement, computed once per case and shared"""
    if (key, conn) not in _REF:
        r = CR.label(vol, level, conn)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[(key, conn)] = r
    return _REF[(key, conn)]


def _gpu(vol, level, conn):
    from inv3d_amd import hipops as H
    return H.grid_components(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, conn)


def _assert_equal(got, want, what):
    assert got['count'] == want['count'] and got['inside'] == want['inside'], (what, got['count'], want['count'], got['inside'], want['inside'])
    lab = got['labels'].cpu().numpy()
    assert lab.dtype == np.int32 and lab.shape == want['labels'].shape
    bad = np.flatnonzero(lab.reshape(-1) != want['labels'].reshape(-1))
    assert bad.size == 0, f'{what}: {bad.size} labels differ, first at {bad[:5]}'
    for k in ('sizes', 'roots'):
        a = got[k].cpu().numpy()
        assert a.dtype == np.int32 and np.array_equal(a, want[k]), (what, k)


@pytest.mark.parametrize('conn', [6, 26])
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('si', range(6))
def test_labels_equal_the_restatement(si, content, conn):
    shape = _shapes()[si]
    vol, level = CS.make(content, shape, seed=si)
    want = _ref((si, content), vol, level, conn)
    _assert_equal(_gpu(vol, level, conn), want, f'{shape} {content} {conn}')
    n = int(np.prod(shape))
    if content == 'all_inside':
        assert want['count'] == 1 and want['sizes'][0] == n
    if content == 'all_outside':
        assert want['count'] == 0
    if content == 'checkerboard':
        assert want['count'] == ((n + 1) // 2 if conn == 6 else 1)


def test_serpentines():
    """Two long chains through every tile of a 40^3 grid: two components under 6; a spur that touches across an edge makes them one under 26."""
    g = CS.serpentines((40, 40, 40))
    vol = np.where(g, np.float32(3.0), np.float32(-1.0)).astype(np.float32)
    for conn, k in ((6, 2), (26, 1)):
        want = _ref('serpentines', vol, 0.0, conn)
        assert want['count'] == k and want['inside'] == int(g.sum()) and want['sizes'].min() > 10000 // k
        _assert_equal(_gpu(vol, 0.0, conn), want, f'serpentines {conn}')


def test_pairs_across_tile_faces_edges_and_corners():
    g, pairs = CS.planted_pairs(_tile())
    vol = np.where(g, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    for conn in (6, 26):
        want = _ref('pairs', vol, CS.LEVEL, conn)
        assert want['count'] == (len(pairs) if conn == 26 else 2 * len(pairs) - 3)          # three of the pairs are face neighbours
        _assert_equal(_gpu(vol, CS.LEVEL, conn), want, f'pairs {conn}')


def test_non_contiguous_and_misaligned_inputs():
    """A strided view is made contiguous; a grid whose storage is not 16-byte aligned takes the scalar path."""
    from inv3d_amd import hipops as H
    vol, level = CS.make('random_0.3', (12, 9, 72), seed=5)                     # D2 % 4 == 0: the vector path when aligned
    want = _ref('misaligned', vol, level, 26)
    flat = torch.zeros(vol.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = torch.from_numpy(vol).reshape(-1).to(DEV)
    view = flat[1:].view(vol.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _assert_equal(H.grid_components(view, level, 26), want, 'misaligned')
    _assert_equal(_gpu(vol, level, 26), want, 'aligned')
    wide = torch.zeros((12, 9, 144), dtype=torch.float32, device=DEV)
    wide[:, :, ::2] = torch.from_numpy(vol).to(DEV)
    _assert_equal(H.grid_components(wide[:, :, ::2], level, 26), want, 'strided')
    kept = H.grid_keep(view, H.grid_components(view, level, 26)['labels'], torch.from_numpy(CR.select(want['sizes'], 1)))
    assert np.array_equal(kept.cpu().numpy().view(np.int32), CR.keep_grid(vol, want['labels'], CR.select(want['sizes'], 1)).view(np.int32))


@pytest.mark.parametrize('shape,content', [((33, 17, 9), 'specials'), ((40, 40, 40), 'random_0.3'), ((2, 3, 5), 'random_0.5'), ((1, 1, 1), 'all_outside')])
def test_keep_equals_where(shape, content):
    from inv3d_amd import hipops as H, inference as INF
    vol, level = CS.make(content, shape, seed=3)
    want = _ref(('keep', shape, content), vol, level, 6)
    t = torch.from_numpy(vol).to(DEV)
    cc = H.grid_components(t, level, 6)
    _assert_equal(cc, want, 'keep labels')
    rng = np.random.RandomState(1)
    masks = [CR.select(want['sizes'], 1), CR.select(want['sizes'], None, 3), rng.rand(want['count']) < 0.5, np.zeros(want['count'], bool)]
    for m, fill in zip(masks, (-1000.0, 0.25, -np.float32(7.5).item(), -1000.0)):
        got = H.grid_keep(t, cc['labels'], torch.from_numpy(m), fill).cpu().numpy()
        exp = CR.keep_grid(vol, want['labels'], m, fill)
        assert np.array_equal(got.view(np.int32), exp.view(np.int32))            # byte for byte: NaN voxels pass through
    assert torch.equal(INF.select_components(cc['sizes'], keep=1).cpu(), torch.from_numpy(masks[0]))
    assert torch.equal(INF.select_components(cc['sizes'], keep=None, min_voxels=3).cpu(), torch.from_numpy(masks[1]))
    if content == 'specials':
        assert np.isnan(vol).any() and np.array_equal(np.isnan(got), np.isnan(vol))


def test_ties_keep_the_lower_label():
    from inv3d_amd import inference as INF
    g = np.zeros((20, 12, 70), np.float32)
    g[2:5, 2:5, 2:5] = 1
    g[12:15, 6:9, 60:63] = 1
    g[8, 8, 30] = 1
    t = torch.from_numpy(g).to(DEV)
    out, info = INF.clean_grid(t, 0.5, keep=1)
    assert info['count'] == 3 and info['sizes'].tolist() == [27, 1, 27] and info['kept'].tolist() == [1] and info['removed_voxels'] == 28
    exp = np.where(g > 0.5, np.float32(-1000.0), g)
    exp[2:5, 2:5, 2:5] = 1
    assert np.array_equal(out.cpu().numpy(), exp) and torch.equal(t.cpu(), torch.from_numpy(g))
    same, info = INF.clean_grid(t, 0.5, keep=None, min_voxels=0)
    assert same is t and info['removed_voxels'] == 0 and info['kept'].tolist() == [1, 2, 3]


def _blobs(shape, centres):
    idx = np.indices(shape).astype(np.float32)
    vol = np.full(shape, -1.0, np.float32)
    for c, r in centres:
        d = np.sqrt(sum((idx[a] - np.float32(c[a])) ** 2 for a in range(3)))
        vol = np.maximum(vol, (1.0 - d / np.float32(r)).astype(np.float32))
    return vol


def _rows(a):
    return {r.tobytes() for r in np.ascontiguousarray(a)}


def test_cleaned_mesh_is_a_subset_of_the_raw_mesh():
    """Components at least two cells apart: marching cubes of the cleaned grid gives exactly the raw mesh's vertices (bit-identical rows, in
    order) and faces (indices remapped) inside the kept component's bounding region.  On any grid every cleaned vertex is a raw vertex."""
    from inv3d_amd import hipops as H, inference as INF
    shape = (24, 20, 80)
    vol = _blobs(shape, [((11.3, 9.6, 30.2), 8.5), ((4.2, 4.1, 70.4), 3.2), ((19.5, 15.2, 68.7), 2.6)])
    t = torch.from_numpy(vol).to(DEV)
    level = 0.1
    want = _ref('blobs', vol, level, 6)
    assert want['count'] == 3
    clean, info = INF.clean_grid(t, level, keep=1)
    assert info['kept'].tolist() == [int(np.argmax(want['sizes'])) + 1]
    rv, rf = (a.cpu().numpy() for a in H.marching_cubes(t, level))
    cv, cf = (a.cpu().numpy() for a in H.marching_cubes(clean, level))
    where = np.argwhere(want['labels'] == info['kept'][0].item())
    lo, hi = where.min(0) - 1, where.max(0) + 1                                   # grid indices; a vertex is (i2, i1, i0)
    others = np.argwhere((want['labels'] > 0) & (want['labels'] != info['kept'][0].item()))
    assert not np.any(np.all((others >= lo - 2) & (others <= hi + 2), axis=1))    # the region holds the kept component alone
    inbox = np.all((rv[:, ::-1] >= lo) & (rv[:, ::-1] <= hi), axis=1)
    assert 0 < inbox.sum() < len(rv)
    assert np.array_equal(rv[inbox].view(np.int32), cv.view(np.int32))
    remap = np.cumsum(inbox) - 1
    fin = inbox[rf].all(1)
    assert not np.any(inbox[rf].any(1) & ~fin)
    assert np.array_equal(remap[rf[fin]].astype(np.int32), cf) and len(cf) > 0
    # any grid
    vol2, level2 = CS.make('random_0.3', (33, 17, 9), seed=11)
    t2 = torch.from_numpy(vol2).to(DEV)
    clean2, info2 = INF.clean_grid(t2, level2, keep=1, connectivity=6)
    assert info2['removed_voxels'] > 0
    raw_rows, clean_rows = _rows(H.marching_cubes(t2, level2)[0].cpu().numpy()), _rows(H.marching_cubes(clean2, level2)[0].cpu().numpy())
    assert clean_rows and clean_rows < raw_rows


def _digests(vols, level):
    """what tests/support/cc_digest.py prints, from this process"""
    from inv3d_amd import hipops as H, inference as INF
    sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()      # noqa: E731
    out = {}
    for name in sorted(vols):
        vol = torch.from_numpy(vols[name]).to(DEV)
        for conn in (6, 26):
            cc = H.grid_components(vol, level, conn)
            kept = H.grid_keep(vol, cc['labels'], INF.select_components(cc['sizes'], keep=1))
            out[f'{name}/{conn}'] = [sha(cc['labels']), sha(cc['sizes']), sha(cc['roots']), cc['count'], cc['inside'], sha(kept)]
    return out


def test_runs_and_builds_are_identical(tmp_path):
    """Two runs give the same bytes, and so does the deterministic build in a fresh interpreter: the merge is lock-free, but the result does
    not depend on its schedule."""
    from inv3d_amd import _lib as L
    vols = dict(vol_random=CS.make('random_0.3', (40, 40, 40), seed=2)[0], vol_tiles=CS.make('random_0.5', tuple(2 * e + 1 for e in _tile()), seed=4)[0])
    level = 0.6
    first, second = _digests(vols, level), _digests(vols, level)
    assert first == second
    if L.DETERMINISTIC:
        return
    path = str(tmp_path / 'inputs.npz')
    np.savez(path, level=level, **vols)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'cc_digest.py'), path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == first


# ---- generator level ---------------------------------------------------------------------------------------------------------------------

RES = 48
BOX = (slice(7, 10),) * 3                                # the planted block; the unpadded region starts at int(30 * 48 / 256) = 5
ZONE = (slice(5, 12),) * 3                               # emptied around it, so that the block is a component of its own whatever the weights give


@pytest.fixture(scope='module')
def small():
    """the small synthetic generator of tests/test_gpu_mesh_color.py and its 48^3 grid, once as it is apart from an emptied corner ('base') and
    once with a 3^3 block above the level planted in that corner ('planted')"""
    from inv3d_amd import inference as INF, synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    for p in G.parameters():
        p.requires_grad_(False)
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    ws = O.synth_ws(cfg, 1, seed=7).to(DEV)
    uni = tuple(u.to(DEV) for u in O.make_uniforms(cfg, 1, seed=4))
    grid = INF.density_grid(G, ws, res=RES)
    level = float(torch.quantile(grid[grid > -999], 0.6))
    density_grid = INF.density_grid

    def plant(g, block=True):
        g = g.clone()
        g[ZONE] = -1000.0
        if block:
            g[BOX] = level + 1.0
        return g

    return dict(G=G, ws=ws, cam=cam, uni=uni, level=level, base=plant(grid, False), planted=plant(grid), plant=plant, density_grid=density_grid)


def _in_box(verts):
    """vertices (i2, i1, i0 order, the same box on every axis) within the planted block's surface range"""
    v = verts.cpu().numpy()
    return np.all((v >= BOX[0].start - 1) & (v <= BOX[0].stop), axis=1)


def _tb(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_keep_through_the_inference_entry_points(small, monkeypatch):
    from inv3d_amd import hipops as H, inference as INF
    G, ws, level, cam = (small[k] for k in ('G', 'ws', 'level', 'cam'))
    calls = []
    real = H.grid_components
    monkeypatch.setattr(H, 'grid_components', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(INF, 'density_grid', lambda *a, **k: small['planted'].clone())
    cc = real(small['planted'], level)
    assert cc['count'] >= 2 and int(cc['sizes'].max()) > 27
    block_label = int(cc['labels'][BOX[0].start, BOX[1].start, BOX[2].start])
    assert int(cc['sizes'][block_label - 1]) == 27                              # the block is a component of its own
    # extract_mesh
    rv, rf = INF.extract_mesh(G, ws, res=RES, level=level)
    assert _in_box(rv).sum() > 0 and not calls
    nv, nf = INF.extract_mesh(G, ws, res=RES, level=level, keep=None, min_voxels=0)
    assert torch.equal(_tb(nv), _tb(rv)) and torch.equal(nf, rf) and not calls     # the default path: nothing labelled
    cv, cf = INF.extract_mesh(G, ws, res=RES, level=level, keep=1)
    assert len(calls) == 1 and 0 < cv.shape[0] < rv.shape[0] and _in_box(cv).sum() == 0
    bv, bf = H.marching_cubes(INF.clean_grid(small['base'], level, keep=1)[0], level)
    assert torch.equal(_tb(cv), _tb(bv)) and torch.equal(cf, bf)                 # the mesh of the unplanted grid, cleaned the same way
    mv, _ = INF.extract_mesh(G, ws, res=RES, level=level, min_voxels=28)
    assert _in_box(mv).sum() == 0 and mv.shape[0] >= cv.shape[0]
    # render_shape
    base_clean = INF.clean_grid(small['base'], level, keep=1)[0]
    want = INF.render_shape(G, ws, cam, res=64, level=level, grid=base_clean)
    raw = INF.render_shape(G, ws, cam, res=64, level=level)
    assert torch.equal(raw['grid'], small['planted'])
    del calls[:]
    got = INF.render_shape(G, ws, cam, res=64, level=level, keep=1)
    assert len(calls) == 1 and torch.equal(got['grid'], base_clean)
    for k in ('mask', 'depth', 'shade'):
        assert torch.equal(_tb(got[k]), _tb(want[k])), k
    same = INF.render_shape(G, ws, cam, res=64, level=level, keep=None)
    assert all(torch.equal(_tb(same[k]), _tb(raw[k])) for k in ('mask', 'depth', 'shade')) and len(calls) == 1
    # render_shape_orbit: one labelling for three frames
    cams = INF.orbit_cameras(3, device=DEV)
    del calls[:]
    frames = list(INF.render_shape_orbit(G, ws, cameras=cams, res=64, level=level, keep=1))
    assert len(frames) == 3 and len(calls) == 1
    for f, w in zip(frames, INF.render_shape_orbit(G, ws, cameras=cams, res=64, level=level, grid=base_clean)):
        assert torch.equal(_tb(f), _tb(w))
    assert len(calls) == 1
    # color_mesh builds and cleans its own grid: the attributes are those of the cleaned grid passed in
    del calls[:]
    kw = dict(render_uniforms=small['uni'], force_fp32=True)
    views = torch.cat([cam, INF.bake_cameras(2, 1, device=DEV)])
    a = INF.color_mesh(G, ws, cv, RES, level=level, cameras=views, keep=1, **kw)
    b = INF.color_mesh(G, ws, cv, RES, level=level, cameras=views, grid=base_clean, **kw)
    assert len(calls) == 1
    for k in ('normals', 'color', 'colors', 'views'):
        assert torch.equal(_tb(a[k]), _tb(b[k])), k


def test_coach_mesh_keep(tmp_path, small, monkeypatch):
    """mesh_keep=1: the PLY and the MRC hold the cleaned grid's shape; the default coach writes what extract_mesh / density_grid give."""
    from inv3d_amd import coach as CO, inference as INF
    G, ws, cam, uni, level = (small[k] for k in ('G', 'ws', 'cam', 'uni', 'level'))
    planted_grid = lambda *a, **k: small['plant'](small['density_grid'](*a, **k))      # noqa: E731
    monkeypatch.setattr(INF, 'density_grid', planted_grid)
    monkeypatch.setattr(CO, 'density_grid', planted_grid)
    kw = dict(first_inv_steps=1, max_pti_steps=1, w_avg_samples=0, gen_mesh=True, mesh_res=RES, mesh_level=level, synth_kwargs=dict(render_uniforms=uni))
    with pytest.raises(ValueError):
        CO.InversionCoach(G, mesh_dir=str(tmp_path), mesh_keep=-1, **kw)
    w, paths = ws, {}
    for name, extra in (('raw', {}), ('clean', dict(mesh_keep=1)), ('sized', dict(mesh_min_voxels=28))):
        for fmt in ('.ply', '.mrc'):
            c = CO.InversionCoach(G, mesh_dir=str(tmp_path / name), mesh_format=fmt, **extra, **kw)
            paths[name, fmt] = c.write_mesh('a', w, cam)
    rv, rf = INF.extract_mesh(G, w, res=RES, level=level)
    cv, cf = INF.extract_mesh(G, w, res=RES, level=level, keep=1)
    assert _in_box(rv).sum() > 0 and _in_box(cv).sum() == 0
    for name, (v, f), grid in (('raw', (rv, rf), planted_grid(G, w, res=RES)), ('clean', (cv, cf), INF.clean_grid(planted_grid(G, w, res=RES), level, keep=1)[0])):
        INF.write_ply(str(tmp_path / f'{name}.ply'), v, f)
        INF.write_mrc(str(tmp_path / f'{name}.mrc'), grid)
        for fmt in ('.ply', '.mrc'):
            assert open(paths[name, fmt], 'rb').read() == open(str(tmp_path / f'{name}{fmt}'), 'rb').read(), (name, fmt)
    assert open(paths['raw', '.ply'], 'rb').read() != open(paths['clean', '.ply'], 'rb').read()
    sized = open(paths['sized', '.ply'], 'rb').read()
    assert sized != open(paths['raw', '.ply'], 'rb').read() and len(sized) >= len(open(paths['clean', '.ply'], 'rb').read())
