"""Textured meshes on the GPU (csrc/mesh_bake.hip mesh_texture_kernel, hipops.mesh_texture, inference.texture_mesh / write_obj, the coach's
mesh_format='.obj'): the atlas, its view counts, the uv and the corner rotation EQUAL the numpy restatement tests/support/texture_ref.py bit
for bit; corner texels equal hipops.mesh_bake's vertices; null outputs, error codes and a bad face index; run-to-run and
normal-vs-deterministic-build identity; and the generator-level pipeline against its composition by hand."""
import ctypes as C
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
import texture_ref as TR  # noqa: E402
from test_gpu_mesh_color import RES, TWO_VOXELS, _assert_bits, _bits, _tb, bake_inputs, small  # noqa: E402,F401
from test_mesh_texture_cpu import _parse_obj, texture_faces  # noqa: E402
from test_mesh_texture_cpu import test_entry_rejects_bad_arguments_before_any_launch as _error_codes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
COUNTS = (1, 2, 3, 9, 19, 200)                          # half a block, a block, a second one, 5 and 10 blocks (one more than a square), 100 blocks
TILES = (4, 5, 8, 16)                                   # 16, 25, 64, 256 texels a block: a quarter of a wave, no divisor of one, one wave, four
OUTPUTS = ('texture', 'views', 'uv', 'corner')
KW = dict(depth_tol=TWO_VOXELS, cos_min=0.1, power=2)


def _device(inp, faces):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in inp.items()}
    t['faces'] = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV)
    return t


def _gpu_texture(t, F, with_fallback=True, **kw):
    from inv3d_amd import hipops as H
    out = H.mesh_texture(t['points'], t['normals'], t['faces'][:F].contiguous(), t['images'], t['depth'], t['mask'], t['cams'],
                         fallback=t['fallback'] if with_fallback else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref_texture(inp, faces, F, with_fallback=True, **kw):
    return TR.texture(inp['points'], inp['normals'], faces[:F], inp['images'], inp['depth'], inp['mask'], inp['cams'],
                      fallback=inp['fallback'] if with_fallback else None, **kw)


@pytest.mark.parametrize('HR', [(8, 8), (37, 16), (1, 1)])
@pytest.mark.parametrize('N', [1, 3])
def test_texture_equals_the_restatement(N, HR):
    """texture, views, uv and corner equal the restatement bit for bit for every face count in COUNTS (prefixes of the 200 seeded faces of
    tests/test_mesh_texture_cpu.py over bake_inputs' 1000 vertices: a repeated index, NaN vertices, vertices behind the camera, at its origin
    and on the frame's edge among them) at every tile in TILES; power 1 and 8, cos_min 0 and 0.1, with and without a fallback take turns
    over those 24 cases, and all eight combinations run at 200 faces and tile 8.  At 200 faces a case is not vacuous: at least a tenth of
    the owned texels are coloured from views and at least a tenth are not."""
    from inv3d_amd import hipops as H
    Hh, R = HR
    inp = bake_inputs(N, Hh, R)
    faces = texture_faces(inp)
    assert faces[1][0] == faces[1][1] and np.isnan(inp['points'][faces[2]]).any()
    t = _device(inp, faces)
    combos = [dict(power=p, cos_min=c, with_fallback=fb) for p in (1, 8) for c in (0.0, 0.1) for fb in (True, False)]
    cases = [(F, T, combos[i % 8]) for i, (F, T) in enumerate((F, T) for F in COUNTS for T in TILES)]
    cases += [(200, 8, c) for c in combos]
    seen_combo = set()
    for F, T, c in cases:
        kw = dict(c, tile=T, depth_tol=TWO_VOXELS)
        got, want = _gpu_texture(t, F, **kw), _ref_texture(inp, faces, F, **kw)
        assert got['texture'].shape == (*H.mesh_texture_size(F, T), 3) and got['uv'].shape == (F, 3, 2) and got['corner'].shape == (F,)
        for k in OUTPUTS:
            _assert_bits(got[k], want[k], (N, Hh, R, F, T, tuple(c.values()), k))
        own = TR.owners(F, T)
        assert (got['texture'][own < 0] == 128).all() and not got['views'][own < 0].any()
        assert int(got['views'].max()) <= N
        if F == 200:
            seen = (got['views'] > 0)[own >= 0].mean()
            assert seen >= 0.1 and 1 - seen >= 0.1, (N, Hh, R, T, seen)
            seen_combo.add(tuple(c.values()))
            assert len(set(got['corner'].tolist())) == 3                       # every rotation occurs
            if not c['with_fallback']:
                assert (got['texture'][(got['views'] == 0)] == 128).all()      # colour 0 is grey 128, as the fill
    assert len(seen_combo) == 8
    # another fill value reaches exactly the texels nobody owns
    got = _gpu_texture(t, 19, tile=5, fill=7, **KW)
    base = _ref_texture(inp, faces, 19, tile=5, **KW)
    own = TR.owners(19, 5)
    assert (got['texture'][own < 0] == 7).all() and np.array_equal(got['texture'][own >= 0], base['texture'][own >= 0]) and (own < 0).sum() > 12


def test_corner_texels_equal_the_vertex_bake():
    """What ties the new kernel to the old one: at the three triangle corners of every face whose vertices are finite the barycentrics are a
    unit vector, so the texel's colour and view count are hipops.mesh_bake's rgb and views of that vertex, bit for bit."""
    from inv3d_amd import hipops as H
    inp = bake_inputs(3, 37, 16)
    faces = texture_faces(inp)
    t = _device(inp, faces)
    vert = H.mesh_bake(t['points'], t['normals'], t['images'], t['depth'], t['mask'], t['cams'], fallback=t['fallback'], **KW)
    rgb, views = vert['rgb'].cpu().numpy(), vert['views'].cpu().numpy()
    finite = np.isfinite(inp['points']).all(1) & np.isfinite(inp['normals']).all(1)
    for T in TILES:
        got = _gpu_texture(t, 200, tile=T, **KW)
        Ht, Wt = got['views'].shape
        checked = 0
        for f in range(200):
            if not finite[faces[f]].all():
                continue
            for k in range(3):
                x = int(round(float(got['uv'][f, k, 0]) * Wt - 0.5))
                y = int(round(float(got['uv'][f, k, 1]) * Ht - 0.5))
                assert np.array_equal(got['texture'][y, x], rgb[faces[f, k]]) and got['views'][y, x] == views[faces[f, k]], (T, f, k)
                checked += 1
        assert checked >= 3 * 190
        assert (views[faces[finite[faces].all(1)]] > 0).mean() > 0.1 and (views[faces[finite[faces].all(1)]] == 0).mean() > 0.1


def _raw_texture(t, F, outputs, tile=8, fill=128, count=True, **kw):
    """eg3d_mesh_texture through ctypes with only `outputs` bound: (the four buffers, pre-filled with 7, and the bad-face count)"""
    from inv3d_amd import _lib as L
    Ht, Wt, _ = TR.size(F, tile)
    out = dict(texture=torch.full((Ht, Wt, 3), 7, dtype=torch.uint8, device=DEV), views=torch.full((Ht, Wt), 7, dtype=torch.uint8, device=DEV),
               uv=torch.full((F, 3, 2), 7.0, device=DEV), corner=torch.full((F,), 7, dtype=torch.uint8, device=DEV))
    bad = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    p = L.MeshTextureParams(points=t['points'].data_ptr(), normals=t['normals'].data_ptr(), faces=t['faces'].data_ptr(), cams=t['cams'].data_ptr(),
                            images=t['images'].data_ptr(), depth=t['depth'].data_ptr(), mask=t['mask'].data_ptr(), fallback=t['fallback'].data_ptr(),
                            V=t['points'].shape[0], F=F, N=t['cams'].shape[0], H=t['images'].shape[2], R=t['depth'].shape[1], tile=tile, fill=fill,
                            bad_faces=bad.data_ptr() if count else None, **kw)
    for k in outputs:
        setattr(p, k, out[k].data_ptr())
    L.check(L.lib().eg3d_mesh_texture(C.byref(p), L.stream_ptr()), 'mesh_texture')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, int(bad.item())


def test_null_outputs_and_error_codes():
    """Each output alone gives the bytes of the full call and leaves the unbound buffers alone; no output at all is legal; every error code
    (tests/test_mesh_texture_cpu.py's list, here where a launch would succeed); F = 0 through the wrapper is one block of fill."""
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    inp = bake_inputs(3, 37, 16)
    faces = texture_faces(inp)
    t = _device(inp, faces)
    full, bad = _raw_texture(t, 19, OUTPUTS, tile=5, **KW)
    want = _ref_texture(inp, faces, 19, tile=5, **KW)
    assert bad == 0
    for k in OUTPUTS:
        _assert_bits(full[k], want[k], k)
    for k in OUTPUTS:
        alone, bad = _raw_texture(t, 19, (k,), tile=5, count=(k == 'uv'), **KW)
        _assert_bits(alone[k], full[k], k)
        assert bad == (0 if k == 'uv' else 7)
        for other in OUTPUTS:
            if other != k:
                assert (alone[other] == 7).all(), (k, other)
    none, bad = _raw_texture(t, 19, (), tile=5, count=False, **KW)
    assert all((v == 7).all() for v in none.values()) and bad == 7
    _error_codes()
    e = H.mesh_texture(t['points'], t['normals'], t['faces'][:0].contiguous(), t['images'], t['depth'], t['mask'], t['cams'], tile=16, fill=9)
    assert e['texture'].shape == (16, 16, 3) and bool((e['texture'] == 9).all()) and not bool(e['views'].any()) and e['uv'].shape == (0, 3, 2)
    for bad_kw in (dict(power=9), dict(tile=3), dict(tile=65), dict(fill=256), dict(cos_min=1.0)):
        with pytest.raises(Eg3dHipError):
            H.mesh_texture(t['points'], t['normals'], t['faces'], t['images'], t['depth'], t['mask'], t['cams'], **bad_kw)
    with pytest.raises(Eg3dHipError):
        H.mesh_texture(t['points'], t['normals'], t['faces'].long(), t['images'], t['depth'], t['mask'], t['cams'])
    with pytest.raises(Eg3dHipError):
        H.mesh_texture(t['points'], t['normals'][:5], t['faces'], t['images'], t['depth'], t['mask'], t['cams'])
    with pytest.raises(Eg3dHipError):
        H.mesh_texture(t['points'], t['normals'], t['faces'], t['images'][:2], t['depth'], t['mask'], t['cams'])


def test_a_bad_face_index_raises_and_the_rest_is_as_specified():
    """Indices 1000 (= V), 2^31 - 1 and -1 in three of 19 faces: no vertex of those faces is read, their texels hold the fill and 0 views, their
    rotation is 0, the counter says 3, every other texel is what the restatement says -- and the wrapper raises."""
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    inp = bake_inputs(3, 37, 16)
    faces = texture_faces(inp)[:19].copy()
    faces[4, 1], faces[11, 2], faces[18, 0] = 1000, 2 ** 31 - 1, -1
    t = _device(inp, faces)
    for T in (5, 8):
        got, bad = _raw_texture(t, 19, OUTPUTS, tile=T, **KW)
        want = _ref_texture(inp, faces, 19, tile=T, **KW)
        assert bad == 3 and want['bad_faces'] == 3
        for k in OUTPUTS:
            _assert_bits(got[k], want[k], (T, k))
        own = TR.owners(19, T)
        for f in (4, 11, 18):
            assert (got['texture'][own == f] == 128).all() and not got['views'][own == f].any() and got['corner'][f] == 0
        assert (got['views'][(own >= 0) & ~np.isin(own, (4, 11, 18))] > 0).mean() > 0.1
    with pytest.raises(Eg3dHipError, match='3 face'):
        H.mesh_texture(t['points'], t['normals'], t['faces'], t['images'], t['depth'], t['mask'], t['cams'], fallback=t['fallback'], **KW)
    # no vertices at all: every face is bad, nothing is read
    with pytest.raises(Eg3dHipError, match='19 face'):
        H.mesh_texture(t['points'][:0], t['normals'][:0], t['faces'], t['images'], t['depth'], t['mask'], t['cams'], **KW)


def _digests(t, kw):
    """what tests/support/texture_digest.py prints, from this process"""
    got = _gpu_texture(t, 200, **kw)
    return {k: hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest() for k in OUTPUTS}


def test_runs_and_builds_are_identical(tmp_path):
    """Two runs in one process give the same bytes, and so does the deterministic build in a fresh interpreter (the library is chosen at
    import; tests/support/texture_digest.py): no texel depends on another thread."""
    from inv3d_amd import _lib as L
    inp = bake_inputs(3, 37, 16)
    faces = texture_faces(inp)
    t = _device(inp, faces)
    kw = dict(KW, tile=8, fill=128)
    first, second = _digests(t, kw), _digests(t, kw)
    assert first == second
    if L.DETERMINISTIC:
        return
    path = str(tmp_path / 'inputs.npz')
    np.savez(path, faces=faces, **kw, **inp)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'texture_digest.py'), path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == first


# ---- generator level ---------------------------------------------------------------------------------------------------------------------

def test_texture_mesh_is_its_composition(small, monkeypatch):  # noqa: F811
    """texture_mesh on the simplified (cell 2) mesh of the 48^3 generator == mesh_to_world, mesh_normals, the radiance fallback, G.synthesis
    per camera, iso_render, mesh_bake and mesh_texture composed here by hand, bit for bit (pinned sampling draws); its per-vertex entries
    are color_mesh's, and color_mesh itself is what the same composition gives.  In a frame that mirrors, the bake runs on the re-wound
    faces and uv comes back in the order of the faces passed in."""
    from inv3d_amd import hipops as H, inference as INF
    G, ws, grid, level, uni = (small[k] for k in ('G', 'ws', 'grid', 'level', 'uni'))
    verts, faces, _ = INF.simplify_mesh(small['verts'], small['faces'], 2.0)
    V, F = verts.shape[0], faces.shape[0]
    assert 100 < F < small['faces'].shape[0] // 2
    cams = torch.cat([small['cam'], INF.bake_cameras(3, 2, device=DEV)])
    kw = dict(render_uniforms=uni, force_fp32=True)
    got = INF.texture_mesh(G, ws, verts, faces, RES, level=level, grid=grid, cameras=cams, tile=5, **kw)
    col = INF.color_mesh(G, ws, verts, RES, level=level, grid=grid, cameras=cams, **kw)
    origin, spacing, axes = INF.grid_frame(G, RES)
    world, wfaces = INF.mesh_to_world(G, verts, faces, RES)
    assert wfaces is faces
    normals = H.mesh_normals(grid, world, origin, spacing, axes)
    planes = G.backbone.synthesis(ws[:1], noise_mode='const')
    planes = planes.view(1, 3, -1, planes.shape[-2], planes.shape[-1])
    fallback = (G.renderer.run_model(planes, G.decoder, world.unsqueeze(0), None, G.rendering_kwargs)['rgb'].reshape(V, -1)[:, :3].float() * 2 - 1).contiguous()
    images = torch.cat([G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image']
                        for i in range(cams.shape[0])]).float().contiguous()
    iso = H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes)
    bkw = dict(fallback=fallback, depth_tol=2 * abs(spacing[0]), cos_min=0.1, power=2)
    baked = H.mesh_bake(world, normals, images, iso['depth'], iso['mask'], cams, **bkw)
    tex = H.mesh_texture(world, normals, faces, images, iso['depth'], iso['mask'], cams, tile=5, **bkw)
    for k, want in (('world', world), ('world_normals', normals), ('normals', INF.normals_to_mesh(G, normals, RES)), ('color', baked['color']),
                    ('colors', baked['rgb']), ('views', baked['views']), ('texture', tex['texture']), ('uv', tex['uv']), ('texture_views', tex['views'])):
        assert got[k].shape == want.shape and torch.equal(_tb(got[k]), _tb(want)), k
    assert set(got) == set(col) | {'texture', 'uv', 'texture_views'}
    for k in col:                                                              # color_mesh is unchanged, and texture_mesh's share of it is color_mesh's
        assert torch.equal(_tb(col[k]), _tb(got[k])), k
    assert tuple(got['texture'].shape) == (*H.mesh_texture_size(F, 5), 3)
    own = torch.from_numpy(TR.owners(F, 5) >= 0).to(DEV)
    seen = float((got['texture_views'] > 0)[own].float().mean())
    print(f'texture_mesh: {F} faces, atlas {tuple(got["texture"].shape[:2])}, {seen:.3f} of the owned texels coloured from views')
    assert seen > 0.05
    # the restatement on the same device inputs
    want = TR.texture(world.cpu().numpy(), normals.cpu().numpy(), faces.cpu().numpy(), images.cpu().numpy(), iso['depth'].cpu().numpy(),
                      iso['mask'].cpu().numpy(), cams.cpu().numpy(), fallback=fallback.cpu().numpy(), tile=5, depth_tol=2 * abs(spacing[0]), cos_min=0.1, power=2)
    for k, r in (('texture', 'texture'), ('texture_views', 'views'), ('uv', 'uv')):
        _assert_bits(got[k].cpu().numpy(), want[r], k + ' vs restatement')
    # a frame without the flip of grid axis 0 mirrors: the bake sees faces[:, [0, 2, 1]], uv returns to the order of `faces`
    monkeypatch.setattr(INF, 'grid_frame', lambda G, res: ((-0.5, -0.5, -0.5), (1.0 / (res - 1),) * 3, (0, 1, 2)))
    mir = INF.texture_mesh(G, ws, verts, faces, RES, level=level, grid=grid, cameras=cams[:2], tile=4, **kw)
    world2, wfaces2 = INF.mesh_to_world(G, verts, faces, RES)
    assert torch.equal(wfaces2, faces[:, [0, 2, 1]])
    o2, s2, a2 = INF.grid_frame(G, RES)
    img2 = images[:2].contiguous()
    iso2 = H.iso_render(grid, cams[:2], img2.shape[-1], level, o2, s2, axes=a2)
    tex2 = H.mesh_texture(world2, mir['world_normals'], wfaces2, img2, iso2['depth'], iso2['mask'], cams[:2].contiguous(), fallback=None, tile=4,
                          depth_tol=2 * abs(s2[0]), cos_min=0.1, power=2)
    assert torch.equal(_tb(mir['uv']), _tb(tex2['uv'][:, [0, 2, 1]].contiguous())) and torch.equal(mir['texture_views'], tex2['views'])


def test_coach_writes_an_obj(tmp_path, small):  # noqa: F811
    """mesh_format='.obj' with mesh_simplify: three files; the OBJ parses with the vertices, faces and normals of extract_mesh / texture_mesh on
    the tuned generator, indices in range, and the PNG is texture_mesh's atlas for the pivot camera in front of bake_cameras()."""
    from PIL import Image
    from inv3d_amd import inference as INF
    from inv3d_amd.coach import InversionCoach
    G, ws, cam, uni, level = (small[k] for k in ('G', 'ws', 'cam', 'uni', 'level'))
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        target = G.synthesis(ws, cam, noise_mode='const', force_fp32=True, render_uniforms=uni)['image'].clamp(-1, 1)
    kw = dict(first_inv_steps=2, max_pti_steps=2, lpips_threshold=0.0, seed=3, w_avg_samples=0, keep_tuned_state=True, synth_kwargs=dict(render_uniforms=uni),
              gen_mesh=True, mesh_res=RES, mesh_level=level, mesh_format='.obj', mesh_simplify=2.0, mesh_texture_tile=5)
    try:
        r1 = InversionCoach(G, mesh_dir=str(tmp_path / 'obj'), **kw).invert('a', target, cam)
        assert r1.mesh_path == os.path.join(str(tmp_path / 'obj'), 'a_pti.obj')
        assert sorted(os.listdir(tmp_path / 'obj')) == ['a_pti.mtl', 'a_pti.obj', 'a_pti.png']
        G.load_state_dict(r1.tuned_state)
        for p in G.parameters():
            p.requires_grad_(False)
        verts, faces = INF.extract_mesh(G, r1.w_pivot, res=RES, level=level, simplify=2.0)
        att = INF.texture_mesh(G, r1.w_pivot, verts, faces, RES, level=level, cameras=InversionCoach.mesh_cameras(r1.cam), tile=5, render_uniforms=uni)
        o = _parse_obj(r1.mesh_path)
        V, F = verts.shape[0], faces.shape[0]
        assert F > 100 and len(o['v']) == V and len(o['vn']) == V and len(o['vt']) == 3 * F and len(o['f']) == F
        assert o['mtllib'] == ['a_pti.mtl'] and open(os.path.join(str(tmp_path / 'obj'), 'a_pti.mtl')).read().split('\n')[2] == 'map_Kd a_pti.png'
        assert np.array_equal(_bits(np.asarray(o['v'], np.float32)), _bits(verts.cpu().numpy()))
        assert np.array_equal(_bits(np.asarray(o['vn'], np.float32)), _bits(att['normals'].cpu().numpy()))
        fi = np.asarray(o['f'])
        assert np.array_equal(fi[:, :, 0] - 1, faces.cpu().numpy()) and np.array_equal(fi[:, :, 1] - 1, np.arange(3 * F).reshape(F, 3))
        vt = np.asarray(o['vt'], np.float64)
        assert vt.min() >= 0 and vt.max() <= 1 and np.array_equal(vt[:, 0].astype(np.float32), att['uv'].cpu().numpy().reshape(-1, 2)[:, 0])
        png = np.asarray(Image.open(os.path.join(str(tmp_path / 'obj'), 'a_pti.png')).convert('RGB'))
        assert np.array_equal(png, att['texture'].cpu().numpy())
        assert int((att['texture_views'] > 0).sum()) > 0
        # the JPEG variant of the writer: three files, an image of the atlas's size close to it (4:4:4, quality 90)
        paths = INF.write_obj(str(tmp_path / 'j.obj'), verts, faces, att['uv'], att['texture'], texture_format='jpg')
        assert paths[2].endswith('j.jpg') and open(paths[1]).read().split('\n')[2] == 'map_Kd j.jpg'
        jpg = np.asarray(Image.open(paths[2]).convert('RGB')).astype(np.int32)
        diff = float(np.abs(jpg - png.astype(np.int32)).mean())
        print(f'jpg atlas: mean absolute difference from the png {diff:.2f} of 255')
        assert jpg.shape == png.shape and diff < 16                           # an unrelated image would differ by some 60; quality 90 quantises by less than 16
    finally:
        G.load_state_dict(pristine)
        for p in G.parameters():
            p.requires_grad_(False)
