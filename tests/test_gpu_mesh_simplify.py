"""GPU tests of the mesh simplification and smoothing (csrc/mesh_simplify.hip; include/eg3d_hip.h "Mesh simplification and smoothing"):
hipops.mesh_simplify must equal the numpy restatement tests/support/simplify_ref.py bit for bit in verts, faces, vertex_map and clusters, and
hipops.mesh_smooth in verts.  Then the layers above: extract_mesh's simplify / smooth options, the attributes of the final vertices, and the
coach's PLYs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import simplify_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_REF = {}


def _ref(key, fn):
    """a restatement result, computed once per case, shared and read-only"""
    if key not in _REF:
        r = fn()
        for a in (r.values() if isinstance(r, dict) else [r]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _dev(v, f):
    return torch.from_numpy(np.array(v, np.float32)).to(DEV), torch.from_numpy(np.array(f, np.int32).reshape(-1, 3)).to(DEV)      # copies: the cases are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _simplify_equal(v, f, cell, origin, want, what):
    from inv3d_amd import hipops as H
    got = H.mesh_simplify(*_dev(v, f), cell, origin)
    gv, gf, gm = got['verts'].cpu().numpy(), got['faces'].cpu().numpy(), got['vertex_map'].cpu().numpy()
    assert got['clusters'] == want['clusters'], (what, got['clusters'], want['clusters'])
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gm.dtype == np.int32
    assert gv.shape == want['verts'].shape and gf.shape == want['faces'].shape and gm.shape == want['vertex_map'].shape, (what, gv.shape, gf.shape)
    assert np.array_equal(gm, want['vertex_map']), what
    assert np.array_equal(gf, want['faces']), what
    bad = np.flatnonzero(np.any(_bits(gv) != _bits(want['verts']), axis=1))
    assert bad.size == 0, f'{what}: {bad.size} vertices differ, first at {bad[:5]}'
    return got


def _smooth_equal(v, f, what, **kw):
    from inv3d_amd import hipops as H
    want = _ref(('smooth', what, tuple(sorted(kw.items()))), lambda: SR.smooth(v, f, **kw))
    got = H.mesh_smooth(*_dev(v, f), **kw).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(np.any(_bits(got) != _bits(want), axis=1))
    assert bad.size == 0, f'{what} {kw}: {bad.size} vertices differ, first at {bad[:5]}'
    return got


MESHES = dict(sphere=lambda: SR.ball(24, 8.7, (11.6, 12.2, 11.9)), torus=SR.torus)


@pytest.mark.parametrize('cell', [1.0, 2.0, 8.0])
@pytest.mark.parametrize('name', sorted(MESHES))
def test_simplify_equals_the_restatement_on_marching_cubes_meshes(name, cell):
    v, f = MESHES[name]()
    want = _ref(('simplify', name, cell), lambda: SR.simplify(v, f, cell))
    assert 0 < len(want['faces']) < len(f) and 0 < len(want['verts']) < len(v)
    if cell == 8.0:
        c, _ = SR.cells(v, cell)
        members = np.unique((c * np.array([1, 2 ** 21, 2 ** 42])).sum(1), return_counts=True)[1]
        assert members.max() > 64                          # a segment longer than a wave: walked by one thread, in order
    _simplify_equal(v, f, cell, (0.0, 0.0, 0.0), want, f'{name}/{cell}')


@pytest.mark.parametrize('n', [63, 64, 65, 257, 4097])
def test_simplify_and_smooth_across_wave_and_workgroup_edges(n):
    v, f = SR.soup(n, seed=n)
    for cell, origin in ((0.75, (0.0, 0.0, 0.0)), (4.0, (-1.0, -0.5, -2.0))):
        want = _ref(('simplify', 'soup', n, cell), lambda: SR.simplify(v, f, cell, origin))
        assert 0 < len(want['faces']) < len(f)
        _simplify_equal(v, f, cell, origin, want, f'soup {n}/{cell}')
    s = SR.simplify(v, f, 0.75)                           # a mesh without repeated indices, with the same vertex count classes
    _smooth_equal(s['verts'], s['faces'], f'soup {n}', iterations=2, pin_boundary=False)
    _smooth_equal(v, f, f'raw soup {n}', iterations=1, pin_boundary=True)      # faces with repeated indices: no self-edges


def test_simplify_empty_and_single_inputs():
    from inv3d_amd import hipops as H
    e3f, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    r = _simplify_equal(e3f, e3i, 1.0, (0, 0, 0), SR.simplify(e3f, e3i, 1.0), 'V = 0')
    assert r['verts'].shape == (0, 3) and r['faces'].shape == (0, 3) and r['clusters'] == 0
    v, f = SR.soup(65, seed=1)
    r = _simplify_equal(v, e3i, 4.0, (0, 0, 0), SR.simplify(v, e3i, 4.0), 'F = 0')
    assert r['verts'].shape == (0, 3) and r['clusters'] > 1 and bool((r['vertex_map'] == -1).all())
    tri_v, tri_f = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5]], np.float32), np.array([[2, 0, 1]], np.int32)
    r = _simplify_equal(tri_v, tri_f, 1.0, (0, 0, 0), SR.simplify(tri_v, tri_f, 1.0), 'one triangle')
    assert r['faces'].tolist() == [[0, 1, 2]] and r['clusters'] == 3
    r = _simplify_equal(tri_v, tri_f, 8.0, (0, 0, 0), SR.simplify(tri_v, tri_f, 8.0), 'one triangle, one cell')
    assert r['faces'].shape == (0, 3) and r['verts'].shape == (0, 3) and r['clusters'] == 1
    assert torch.equal(H.mesh_smooth(*_dev(e3f, e3i)), torch.zeros((0, 3), device=DEV))
    _smooth_equal(tri_v, tri_f, 'one triangle', iterations=3, pin_boundary=False)
    _smooth_equal(tri_v, e3i, 'no faces', iterations=3)


def test_simplify_planted_cases():
    """a cluster of one vertex, a face that collapses to an edge, one to a point, duplicates after rotation, opposite windings that both stay, an
    unreferenced cluster, vertices exactly on cell borders, a non-zero origin (tests/support/simplify_ref.py planted)"""
    v, f, want_faces, want_map, clusters = SR.planted()
    origin = (-3.0, 0.5, 2.0)
    want = SR.simplify(v, f, 2.0, origin)
    assert want['clusters'] == clusters and np.array_equal(want['faces'], want_faces) and np.array_equal(want['vertex_map'], want_map)
    got = _simplify_equal(v, f, 2.0, origin, want, 'planted')
    assert got['verts'].shape == (5, 3)
    assert np.array_equal(_bits(got['verts'][1:4].cpu().numpy()), _bits(v[2:5]))      # clusters of one vertex: the vertex itself


def test_smooth_equals_the_restatement():
    lv, lf = SR.lattice(9, 8)                             # an open mesh
    rng = np.random.RandomState(5)
    lv = lv + (rng.rand(*lv.shape) * 0.4).astype(np.float32)
    for pin in (True, False):
        for it in (0, 1, 7):
            got = _smooth_equal(lv, lf, 'lattice', iterations=it, pin_boundary=pin)
            if it == 0:
                assert np.array_equal(_bits(got), _bits(lv))
    _, _, boundary = SR.adjacency(lf, len(lv))
    pinned = _smooth_equal(lv, lf, 'lattice', iterations=7, pin_boundary=True)
    assert np.array_equal(_bits(pinned[boundary]), _bits(lv[boundary])) and np.any(pinned[~boundary] != lv[~boundary])
    fv, ff = SR.fan(70)                                   # degree 70 > 64, and a vertex with no faces
    rows, _, _ = SR.adjacency(ff, len(fv))
    assert np.bincount(rows, minlength=len(fv)).max() == 70 and np.bincount(rows, minlength=len(fv))[-1] == 0
    for it in (1, 7):
        got = _smooth_equal(fv, ff, 'fan', iterations=it, pin_boundary=False)
        assert np.array_equal(_bits(got[-1]), _bits(fv[-1]))
    _smooth_equal(fv, ff, 'fan', iterations=7, lam=0.33, mu=-0.34, pin_boundary=True)
    sv, sf = MESHES['torus']()
    _smooth_equal(sv, sf, 'torus', iterations=7)


def test_invalid_input_raises_and_the_process_goes_on():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    v, f = SR.soup(257, seed=3)
    want = _ref(('simplify', 'soup-ok', 257), lambda: SR.simplify(v, f, 2.0))
    for bad in (np.nan, np.inf, -0.25, 2.0 * 2 ** 21, -np.inf):
        w = v.copy()
        w[130, 1] = bad
        with pytest.raises(Eg3dHipError):
            H.mesh_simplify(*_dev(w, f), 2.0)
        _simplify_equal(v, f, 2.0, (0, 0, 0), want, 'after a bad vertex')
    for bad in (-1, 257, 2 ** 31 - 1, -2 ** 31):
        g = f.copy()
        g[200, 2] = bad
        with pytest.raises(Eg3dHipError):
            H.mesh_simplify(*_dev(v, g), 2.0)
        with pytest.raises(Eg3dHipError):
            H.mesh_smooth(*_dev(v, g), iterations=1)
        _simplify_equal(v, f, 2.0, (0, 0, 0), want, 'after a bad face index')
    with pytest.raises(Eg3dHipError):
        H.mesh_simplify(torch.zeros((0, 3), device=DEV), _dev(v, f)[1], 1.0)      # V = 0: every index is out of range
    _smooth_equal(v, f, 'after the errors', iterations=1)


def test_two_calls_are_identical():
    from inv3d_amd import hipops as H
    v, f = _dev(*MESHES['sphere']())
    a, b = H.mesh_simplify(v, f, 2.0), H.mesh_simplify(v, f, 2.0)
    assert a['clusters'] == b['clusters']
    for k in ('verts', 'faces', 'vertex_map'):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(H.mesh_smooth(a['verts'], a['faces'], 5), H.mesh_smooth(b['verts'], b['faces'], 5))
    assert torch.equal(v, _dev(*MESHES['sphere']())[0])   # the input is not modified


# ---- generator level ---------------------------------------------------------------------------------------------------------------------

RES = 48


@pytest.fixture(scope='module')
def small():
    """the small synthetic generator of tests/test_gpu_mesh_color.py, a level its 48^3 grid reaches, and the plain mesh"""
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
    verts, faces = INF.extract_mesh(G, ws, res=RES, level=level)
    return dict(G=G, ws=ws, cam=cam, uni=uni, level=level, verts=verts, faces=faces)


def _tb(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_extract_mesh_options(small, monkeypatch):
    from inv3d_amd import hipops as H, inference as INF
    G, ws, level, verts, faces = (small[k] for k in ('G', 'ws', 'level', 'verts', 'faces'))
    assert verts.shape[0] > 1000
    calls = []
    for name in ('mesh_simplify', 'mesh_smooth'):
        real = getattr(H, name)
        monkeypatch.setattr(H, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    dv, df = INF.extract_mesh(G, ws, res=RES, level=level, simplify=None, smooth=0)
    assert torch.equal(_tb(dv), _tb(verts)) and torch.equal(df, faces) and not calls      # the defaults: the plain output, no new code runs
    s = SR.simplify(verts.cpu().numpy(), faces.cpu().numpy(), 2.0)
    want_v = SR.smooth(s['verts'], s['faces'], iterations=3)
    gv, gf = INF.extract_mesh(G, ws, res=RES, level=level, simplify=2, smooth=3)
    assert calls == ['mesh_simplify', 'mesh_smooth']
    assert 0 < gf.shape[0] < faces.shape[0] and np.array_equal(gf.cpu().numpy(), s['faces'])
    assert np.array_equal(_bits(gv.cpu().numpy()), _bits(want_v))
    ov, of = INF.extract_mesh(G, ws, res=RES, level=level, simplify=2)
    assert np.array_equal(_bits(ov.cpu().numpy()), _bits(s['verts'])) and torch.equal(of, gf)
    kv, kf = INF.extract_mesh(G, ws, res=RES, level=level, smooth=2, smooth_kwargs=dict(lam=0.4, mu=-0.42, pin_boundary=False))
    assert torch.equal(kf, faces)
    assert np.array_equal(_bits(kv.cpu().numpy()), _bits(SR.smooth(verts.cpu().numpy(), faces.cpu().numpy(), 2, 0.4, -0.42, False)))
    sv, sf, info = INF.simplify_mesh(verts, faces, 2.0)
    assert torch.equal(_tb(sv), _tb(ov)) and torch.equal(sf, of) and info['clusters'] == s['clusters']
    assert np.array_equal(info['vertex_map'].cpu().numpy(), s['vertex_map'])
    assert torch.equal(_tb(INF.smooth_mesh(sv, sf, 3)), _tb(gv))
    # attributes: those of the final vertices (the sampling draws pinned, so that two bakes are comparable)
    views = torch.cat([small['cam'], INF.bake_cameras(2, 1, device=DEV)])
    pinned = dict(cameras=views, render_uniforms=small['uni'], force_fp32=True)
    real_color = INF.color_mesh
    seen = []
    monkeypatch.setattr(INF, 'color_mesh', lambda G_, ws_, v_, res_, **k: (seen.append(v_), real_color(G_, ws_, v_, res_, **dict(k, **pinned)))[1])
    av, af, an, ac = INF.extract_mesh(G, ws, res=RES, level=level, simplify=2, smooth=3, attributes=True)
    assert torch.equal(_tb(av), _tb(gv)) and torch.equal(af, gf) and len(seen) == 1 and torch.equal(_tb(seen[0]), _tb(gv))
    att = real_color(G, ws, gv, RES, level=level, **pinned)
    assert an.shape == gv.shape and torch.equal(_tb(an), _tb(att['normals'])) and torch.equal(ac, att['colors'])
    assert float(an.norm(dim=1).max()) <= 1.0 + 1e-5 and int((att['views'] > 0).sum()) > 0


def _ply_counts(path):
    head = open(path, 'rb').read().split(b'end_header\n', 1)[0].decode('ascii')
    n = {line.split()[1]: int(line.split()[2]) for line in head.splitlines() if line.startswith('element ')}
    return n['vertex'], n['face'], 'property uchar red' in head


def test_coach_writes_the_simplified_mesh(tmp_path, small):
    from inv3d_amd import coach as CO, inference as INF
    G, ws, cam, uni, level = (small[k] for k in ('G', 'ws', 'cam', 'uni', 'level'))
    kw = dict(first_inv_steps=1, max_pti_steps=1, w_avg_samples=0, gen_mesh=True, mesh_res=RES, mesh_level=level, mesh_format='.ply',
              synth_kwargs=dict(render_uniforms=uni))
    with pytest.raises(ValueError):
        CO.InversionCoach(G, mesh_dir=str(tmp_path), mesh_simplify=-2.0, **kw)
    gv, gf = INF.extract_mesh(G, ws, res=RES, level=level, simplify=2, smooth=3)
    assert 0 < gf.shape[0] < small['faces'].shape[0]
    plain = CO.InversionCoach(G, mesh_dir=str(tmp_path / 'plain'), mesh_simplify=2, mesh_smooth=3, **kw).write_mesh('a', ws, cam)
    assert _ply_counts(plain) == (gv.shape[0], gf.shape[0], False)
    want = str(tmp_path / 'want.ply')
    INF.write_ply(want, gv, gf)
    assert open(plain, 'rb').read() == open(want, 'rb').read()
    colour = CO.InversionCoach(G, mesh_dir=str(tmp_path / 'colour'), mesh_simplify=2, mesh_smooth=3, mesh_colors=True, **kw).write_mesh('a', ws, cam)
    assert _ply_counts(colour) == (gv.shape[0], gf.shape[0], True)
    raw = CO.InversionCoach(G, mesh_dir=str(tmp_path / 'raw'), **kw).write_mesh('a', ws, cam)
    assert _ply_counts(raw) == (small['verts'].shape[0], small['faces'].shape[0], False)
