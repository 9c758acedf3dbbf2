"""Mesh previews on the GPU (csrc/mesh_raster.hip, hipops.mesh_raster, inference.render_mesh / mesh_fidelity, video.write_mesh_video): every
output EQUALS the numpy restatement tests/support/raster_ref.py bit for bit over resolutions, view counts, face counts, modes and cull
settings, on faces that exercise every path of the kernels; the marching-cubes sphere against the iso-surface marcher on the device; null
outputs, error codes and a bad face index; run-to-run and normal-vs-deterministic-build identity; and the generator-level pipeline from the
bake through the atlas and the uv to pixels."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import raster_ref as RR  # noqa: E402
import texture_ref as TR  # noqa: E402
from test_gpu_mesh_color import RES, _assert_bits, _tb, _unproject0, bake_cameras, small  # noqa: E402,F401
from test_mesh_raster_cpu import GRID, depth_against_the_marcher, raster_inputs, ref_raster, sphere  # noqa: E402,F401
from test_mesh_raster_cpu import RES as SPHERE_RES  # noqa: E402
from test_mesh_raster_cpu import test_entry_rejects_bad_arguments_before_any_launch as _error_codes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUTPUTS = ('image', 'face', 'z', 'depth', 'mask', 'bary')
COUNTS = (0, 1, 2, 63, 64, 65, 200)                      # nothing, one lane, a wave minus / exactly / plus one, a partial workgroup
F32 = np.float32


def _device(inp):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in inp.items()}


def _gpu_raster(t, res, mode, cull, F=None, **kw):
    from inv3d_amd import hipops as H
    F = t['faces'].shape[0] if F is None else F
    out = H.mesh_raster(t['points'], t['faces'][:F].contiguous(), t['cams'], res, mode=mode, uv=t['uv'][:F].contiguous(), texture=t['texture'],
                        colors=t['colors'], normals=t['normals'], cull=cull, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _prefix(inp, F):
    return dict(inp, faces=inp['faces'][:F], uv=inp['uv'][:F])


def _compare(got, want, what):
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        _assert_bits(got[k], want[k], (what, k))
    assert (got['small_faces'], got['large_faces']) == (want['small_faces'], want['large_faces']), what


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('res', [1, 7, 64, 65])
def test_raster_equals_the_restatement(res, N):
    """image, face, z, depth, mask, bary and the two path counts equal the restatement for every face count in COUNTS (prefixes of the 200
    seeded faces of tests/test_mesh_texture_cpu.py over bake_inputs' 1000 vertices), the three modes and the two cull settings.  At 200 faces
    and more than one pixel a case is not vacuous: between a tenth and nine tenths of the pixels are covered, and where a frame can hold a
    large face (more than 8 pixels a side) both draw paths are taken."""
    inp = raster_inputs(N)
    t = _device(inp)
    for F in COUNTS:
        for cull in ('back', 'none'):
            for i, mode in enumerate(RR.MODES):
                kw = dict(background=(1.0, -0.5, 0.25)[i], ambient=(0.2, 0.0, 1.0)[i], near=(0.1, 0.1, 2.2)[i] if F == 65 else 0.1)
                got, want = _gpu_raster(t, res, mode, cull, F=F, **kw), ref_raster(_prefix(inp, F), res, mode, cull, **kw)
                _compare(got, want, (res, N, F, mode, cull))
                assert got['image'].shape == (N, 3, res, res) and got['bary'].shape == (N, res, res, 3)
                assert ((got['face'] >= 0) == (got['mask'] > 0)).all() and got['face'].max(initial=-1) < max(F, 1)
                if F == 0:
                    assert not got['mask'].any() and (got['image'] == F32(kw['background'])).all() and not got['depth'].any()
                if F == 200 and res > 1:
                    covered = float(got['mask'].mean())
                    assert 0.1 <= covered <= 0.9, (res, N, cull, covered)
                    assert got['small_faces'] > 0 and (got['large_faces'] > 0) == (res > RR.SMALL)


def special_inputs(res=64):
    """Faces that each take one path, in cam0's frame at `res` pixels (vertices at height 0.5, where cam0's projection of short binary
    fractions is exact at res 64): pixel ranges of 9, 8 and 7 pixels -- one more than the widest range a lane draws, exactly that, one less --
    in x and in y; a face around the whole frame; faces inside one pixel with and without its centre; a zero-area face and a repeated
    index; two coincident faces; a face behind the others; a face with a vertex behind the camera."""
    def at(px, py, z=0.5):
        return _unproject0(np.array([(px + 0.5) / res]), np.array([(py + 0.5) / res]), z)[0]
    verts, faces = [], []

    def tri(a, b, c, z=0.5):
        k = len(verts)
        verts.extend([at(*a, z), at(*b, z), at(*c, z)])
        faces.append((k, k + 2, k + 1))                                        # image y runs against world y: this order faces the camera

    for i, w in enumerate((8.0, 7.0, 6.5)):                                    # ranges of 9, 8 and 7 pixels along x, 4 along y
        tri((10.0, 3.0 + 10 * i), (10.0 + w, 3.0 + 10 * i), (10.0, 6.0 + 10 * i))
    for i, h in enumerate((8.0, 7.0, 6.5)):                                    # and along y
        tri((30.0 + 6 * i, 10.0), (33.0 + 6 * i, 10.0), (30.0 + 6 * i, 10.0 + h))
    tri((-3.0 * res, -3.0 * res), (6.0 * res, -3.0 * res), (-3.0 * res, 6.0 * res), z=-0.3)      # around the whole frame, behind everything else
    tri((20.2, 20.3), (20.6, 20.3), (20.2, 20.7))                              # inside a pixel, no centre
    tri((21.8, 21.8), (22.3, 21.8), (21.8, 22.3))                              # inside a pixel square around the centre (22, 22)
    tri((40.0, 40.0), (44.0, 44.0), (48.0, 48.0))                              # zero area
    k = len(verts)
    verts.extend([at(50.0, 50.0), at(55.0, 50.0)])
    faces.append((k, k, k + 1))                                                # a repeated index
    tri((12.0, 40.0), (24.0, 40.0), (12.0, 52.0), z=0.25)
    faces.append(faces[-1])                                                    # coincident with the face before it
    k = len(verts)
    verts.extend([at(5.0, 5.0), at(9.0, 5.0), np.array([0.0, 0.0, 2.6])])      # the third vertex lies behind cam0 (at height 2.5)
    faces.append((k, k + 2, k + 1))
    rng = np.random.RandomState(5)
    V, F = len(verts), len(faces)
    Ht, Wt, _ = TR.size(F, 8)
    return dict(points=np.asarray(verts, F32), faces=np.asarray(faces, np.int32), cams=bake_cameras()[:1], uv=TR.uv(F, 8, rng.randint(0, 3, F).astype(np.uint8)),
                texture=rng.randint(0, 256, (Ht, Wt, 3)).astype(np.uint8), colors=rng.uniform(-1, 1, (V, 3)).astype(F32), normals=rng.normal(size=(V, 3)).astype(F32))


def _raw_raster(t, res, outputs, mode='vertex', cull=1, count=True, stats=True):
    """eg3d_mesh_raster through ctypes with only `outputs` bound: (the six buffers, pre-filled with 7, the bad-face count, the two path counts)"""
    from inv3d_amd import _lib as L
    N, V, F = t['cams'].shape[0], t['points'].shape[0], t['faces'].shape[0]
    out = dict(image=torch.full((N, 3, res, res), 7.0, device=DEV), face=torch.full((N, res, res), 7, dtype=torch.int32, device=DEV),
               z=torch.full((N, res, res), 7.0, device=DEV), depth=torch.full((N, res, res), 7.0, device=DEV),
               mask=torch.full((N, res, res), 7, dtype=torch.uint8, device=DEV), bary=torch.full((N, res, res, 3), 7.0, device=DEV))
    counts = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    p = L.MeshRasterParams(points=t['points'].data_ptr(), faces=t['faces'].data_ptr(), cams=t['cams'].data_ptr(), uv=t['uv'].data_ptr(),
                           texture=t['texture'].data_ptr(), colors=t['colors'].data_ptr(), normals=t['normals'].data_ptr(), V=V, F=F, N=N, res=res,
                           Ht=t['texture'].shape[0], Wt=t['texture'].shape[1], mode=dict(texture=0, vertex=1, lambert=2)[mode], cull=cull, near=0.1,
                           background=1.0, ambient=0.2, bad_faces=counts.data_ptr() if count else None, stats=counts.data_ptr() + 4 if stats else None)
    n = C.c_int64(0)
    L.check(L.lib().eg3d_mesh_raster_query_workspace(C.byref(p), C.byref(n)), 'query')
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), n.value
    for k in outputs:
        setattr(p, k, out[k].data_ptr())
    L.check(L.lib().eg3d_mesh_raster(C.byref(p), L.stream_ptr()), 'mesh_raster')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, counts.tolist()


def test_faces_that_take_one_path_each():
    """special_inputs at 64^2 and 65^2: ranges of 9, 8 and 7 pixels fall on the two sides of the bound as counted by hand; the face around
    the frame fills every pixel nothing else covers; a face inside a pixel draws that pixel only when it holds the centre; zero-area faces
    draw nothing; of two coincident faces the lower index is seen; and everything equals the restatement."""
    for res in (64, 65):
        inp = special_inputs(res)
        t = _device(inp)
        for cull in ('back', 'none'):
            for mode in RR.MODES:
                got, want = _gpu_raster(t, res, mode, cull), ref_raster(inp, res, mode, cull)
                _compare(got, want, (res, mode, cull))
            face = got['face'][0]
            assert got['mask'].all() and (face == 6).mean() > 0.8              # the face around the frame: everywhere but under the others
            if res == 64:
                # large: 9 wide, 9 high, the frame-filling face, the two coincident faces (13 x 13); small: 8 and 7 wide and high, the pixel face
                assert (got['large_faces'], got['small_faces']) == (5, 5)
                assert face[22, 22] == 8 and face[20, 20] == 6 and face[21, 21] == 6
                assert set(np.unique(face)) == {0, 1, 2, 3, 4, 5, 6, 8, 11}     # 7: no centre; 9, 10: no area; 12: behind 11; 13: a vertex behind the camera
                assert (face[3, 10:19] == 0).all() and face[3, 19] == 6 and (face[13, 10:18] == 1).all() and face[13, 18] == 6
                assert (face[10:19, 30] == 3).all() and face[19, 30] == 6 and (face[10:18, 36] == 4).all() and face[18, 36] == 6
    # an index outside [0, V): the face is dropped and counted, the rest is what the restatement says
    inp = special_inputs(64)
    inp['faces'] = inp['faces'].copy()
    inp['faces'][4, 1] = len(inp['points'])
    t = _device(inp)
    want = ref_raster(inp, 64, 'vertex', 'back')
    got, counts = _raw_raster(t, 64, OUTPUTS)
    assert want['bad_faces'] == 1 and counts == [1, want['small_faces'], want['large_faces']] and not (got['face'] == 4).any()
    for k in OUTPUTS:
        _assert_bits(got[k], want[k], ('bad index', k))
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    with pytest.raises(Eg3dHipError, match='1 face'):
        H.mesh_raster(t['points'], t['faces'], t['cams'], 64, mode='vertex', colors=t['colors'])
    with pytest.raises(Eg3dHipError, match=f'{len(inp["faces"])} face'):       # no vertices at all: every face is bad, nothing is read
        H.mesh_raster(t['points'][:0], t['faces'], t['cams'], 64, mode='vertex', colors=t['colors'][:0])


def test_null_outputs_and_error_codes():
    """Each output alone gives the bytes of the full call and leaves the unbound buffers alone; no output at all is legal and launches
    nothing; every error code (tests/test_mesh_raster_cpu.py's list, here where a launch would succeed); the wrapper's refusals."""
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    inp = raster_inputs(3)
    t = _device(inp)
    for mode in RR.MODES:
        full, counts = _raw_raster(t, 33, OUTPUTS, mode=mode)
        want = ref_raster(inp, 33, mode, 'back')
        assert counts == [0, want['small_faces'], want['large_faces']]
        for k in OUTPUTS:
            _assert_bits(full[k], want[k], (mode, k))
        for k in OUTPUTS:
            alone, counts = _raw_raster(t, 33, (k,), mode=mode, count=(k == 'z'), stats=(k == 'mask'))
            _assert_bits(alone[k], full[k], (mode, k))
            assert counts == [0 if k == 'z' else 7, want['small_faces'] if k == 'mask' else 7, want['large_faces'] if k == 'mask' else 7]
            for other in OUTPUTS:
                if other != k:
                    assert (alone[other] == 7).all(), (k, other)
    none, counts = _raw_raster(t, 33, (), count=False, stats=False)
    assert all((v == 7).all() for v in none.values()) and counts == [7, 7, 7]
    _error_codes()
    for bad in (dict(mode='phong'), dict(cull='front'), dict(near=0.0), dict(ambient=1.5), dict(mode='texture', uv=None), dict(mode='lambert', normals=None),
                dict(mode='vertex', colors=t['colors'][:5]), dict(mode='texture', texture=t['texture'][:1]), dict(mode='texture', uv=t['uv'][:5])):
        kw = dict(dict(mode='vertex', uv=t['uv'], texture=t['texture'], colors=t['colors'], normals=t['normals']), **bad)
        with pytest.raises(Eg3dHipError):
            H.mesh_raster(t['points'], t['faces'], t['cams'], 33, **kw)
    with pytest.raises(Eg3dHipError):
        H.mesh_raster(t['points'], t['faces'].long(), t['cams'], 33, mode='vertex', colors=t['colors'])
    with pytest.raises(Eg3dHipError):
        H.mesh_raster(t['points'], t['faces'], t['cams'][:, :24], 33, mode='vertex', colors=t['colors'])
    with pytest.raises(Eg3dHipError):
        H.mesh_raster(t['points'], t['faces'], t['cams'], 0, mode='vertex', colors=t['colors'])


def test_sphere_equals_the_restatement_and_agrees_with_the_marcher(sphere):  # noqa: F811
    """The marching-cubes sphere of tests/test_mesh_raster_cpu.py from bake_cameras() at 64^2: bit equality with the restatement, and its
    depth against hipops.iso_render on the same grid, level and cameras within sqrt(3) |spacing| / 0.5 (the comparison of the CPU test)."""
    from inv3d_amd import hipops as H
    world, faces, cams = (torch.from_numpy(np.ascontiguousarray(sphere[k])).to(DEV) for k in ('world', 'faces', 'cams'))
    normals = torch.from_numpy(sphere['normals']).to(DEV)
    got = H.mesh_raster(world, faces, cams, SPHERE_RES, mode='lambert', normals=normals, cull='back')
    torch.cuda.synchronize()
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    _compare(host, sphere['back'], 'sphere')
    assert host['small_faces'] > 1000 and GRID == 24
    fr = sphere['frame']
    iso = H.iso_render(torch.from_numpy(sphere['vol']).to(DEV), cams, SPHERE_RES, 0.0, fr['origin'], fr['spacing'], axes=fr['axes'])
    worst, bound, used, both, covered = depth_against_the_marcher(host['depth'], host['mask'], iso['depth'].cpu().numpy(), iso['mask'].cpu().numpy(),
                                                                  iso['normal'].cpu().numpy(), sphere['cams'], SPHERE_RES, fr['spacing'][1])
    print(f'sphere on the device: {used} of {both} doubly masked pixels compared, covered {covered:.3f}, largest depth difference {worst:.5f}, bound {bound:.5f}')
    assert 0.25 <= covered <= 0.75 and used >= both / 2 and worst <= bound


def _digests(t, res, cull):
    """what tests/support/raster_digest.py prints, from this process"""
    out = {}
    for mode in RR.MODES:
        got = _gpu_raster(t, res, mode, cull)
        h = hashlib.sha256()
        for k in OUTPUTS:
            h.update(np.ascontiguousarray(got[k]).tobytes())
        out[mode] = h.hexdigest()
    return out


def test_runs_and_builds_are_identical(tmp_path):
    """Five launches in one process give one digest although the queue of large faces and the order of the atomic minima differ from run to
    run, and so does the deterministic build in a fresh interpreter (the library is chosen at import; tests/support/raster_digest.py)."""
    from inv3d_amd import _lib as L
    inp = raster_inputs(3)
    t = _device(inp)
    runs = [_digests(t, 65, 'none') for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    if L.DETERMINISTIC:
        return
    path = str(tmp_path / 'inputs.npz')
    np.savez(path, res=65, cull='none', **inp)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'raster_digest.py'), path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == runs[0]


# ---- generator level ---------------------------------------------------------------------------------------------------------------------

def _avi_frames(data):
    """(frames the headers announce, the index's (offset, size) entries) of a Motion-JPEG AVI, each entry checked against its chunk"""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI ' and struct.unpack('<I', data[4:8])[0] == len(data) - 8
    total = struct.unpack('<I', data[32 + 16:32 + 20])[0]
    movi = data.index(b'movi')
    at = data.rindex(b'idx1')
    n = struct.unpack('<I', data[at + 4:at + 8])[0] // 16
    entries = []
    for i in range(n):
        tag, _, off, size = struct.unpack('<4sIII', data[at + 8 + 16 * i:at + 24 + 16 * i])
        chunk = movi + off
        assert tag == b'00dc' and data[chunk:chunk + 4] == b'00dc' and struct.unpack('<I', data[chunk + 4:chunk + 8])[0] == size
        assert data[chunk + 8:chunk + 10] == b'\xff\xd8' and data[chunk + 8 + size - 2:chunk + 8 + size] == b'\xff\xd9'
        entries.append((off, size))
    return total, entries


def test_the_pipeline_from_bake_to_pixels(small, monkeypatch, tmp_path):  # noqa: F811
    """extract (cell-2 simplification), texture_mesh, render_mesh at the bake cameras on the 48^3 generator: render_mesh is mesh_to_world and
    hipops.mesh_raster composed by hand, and the restatement on the same inputs; supersampling is avg_pool2d of the finer render;
    mesh_fidelity is finite with a silhouette that overlaps the marcher's (a sanity floor, not a measurement); in a frame that mirrors the
    faces are re-wound and the uv rows follow; write_mesh_video writes the frames its index names, and write_orbit_video's bytes are what its
    parts compose to."""
    from inv3d_amd import hipops as H, inference as INF, video as VID
    G, ws, grid, level, uni = (small[k] for k in ('G', 'ws', 'grid', 'level', 'uni'))
    verts, faces, _ = INF.simplify_mesh(small['verts'], small['faces'], 2.0)
    F = faces.shape[0]
    cams = INF.bake_cameras(3, 2, device=DEV)
    kw = dict(render_uniforms=uni, force_fp32=True)
    att = INF.texture_mesh(G, ws, verts, faces, RES, level=level, grid=grid, cameras=cams, tile=5, **kw)
    res = int(G.img_resolution)
    got = INF.render_mesh(G, verts, faces, cams, mode='texture', uv=att['uv'], texture=att['texture'], grid_res=RES)
    world, wfaces = INF.mesh_to_world(G, verts, faces, RES)
    assert wfaces is faces
    hand = H.mesh_raster(world, faces, cams, res, mode='texture', uv=att['uv'], texture=att['texture'])
    assert got['image'].shape == (6, 3, res, res)
    for k in OUTPUTS:
        assert torch.equal(_tb(got[k]), _tb(hand[k])), k
    want = RR.raster(world.cpu().numpy(), faces.cpu().numpy(), cams.cpu().numpy(), res, mode='texture', uv=att['uv'].cpu().numpy(),
                     texture=att['texture'].cpu().numpy())
    for k in OUTPUTS:
        _assert_bits(got[k].cpu().numpy(), want[k], k + ' vs restatement')
    covered = float(got['mask'].float().mean())
    print(f'render_mesh: {F} faces at {res}^2 from 6 cameras, covered {covered:.3f}, {got["small_faces"]} small and {got["large_faces"]} large faces')
    assert 0.05 < covered < 0.95
    # the other two modes through the exporters' own attributes
    vert = INF.render_mesh(G, verts, faces, cams[:2], mode='vertex', colors=att['color'], grid_res=RES)
    hand = H.mesh_raster(world, faces, cams[:2].contiguous(), res, mode='vertex', colors=att['color'])
    assert torch.equal(_tb(vert['image']), _tb(hand['image'])) and torch.equal(vert['face'], got['face'][:2])
    lam = INF.render_mesh(G, verts, faces, cams[:2], mode='lambert', normals=att['normals'], grid_res=RES, ambient=0.1)
    hand = H.mesh_raster(world, faces, cams[:2].contiguous(), res, mode='lambert', normals=att['world_normals'], ambient=0.1)
    assert torch.equal(_tb(lam['image']), _tb(hand['image']))
    # supersampling
    ss = INF.render_mesh(G, verts, faces, cams[:1], mode='texture', uv=att['uv'], texture=att['texture'], grid_res=RES, supersample=2)
    fine = H.mesh_raster(world, faces, cams[:1].contiguous(), 2 * res, mode='texture', uv=att['uv'], texture=att['texture'])
    assert set(ss) == {'image', 'coverage'} and ss['image'].shape == (1, 3, res, res) and ss['coverage'].shape == (1, res, res)
    assert torch.equal(ss['image'], torch.nn.functional.avg_pool2d(fine['image'], 2))
    assert torch.equal(ss['coverage'], torch.nn.functional.avg_pool2d(fine['mask'].float().unsqueeze(1), 2)[:, 0])
    # the orbit generator is render_mesh per camera
    orbit = list(INF.render_mesh_orbit(G, verts, faces, cameras=cams[:2], mode='texture', uv=att['uv'], texture=att['texture'], grid_res=RES))
    assert len(orbit) == 2 and torch.equal(_tb(torch.stack(orbit)), _tb(got['image'][:2]))
    # fidelity
    fid = INF.mesh_fidelity(G, ws, verts, faces, att['uv'], att['texture'], grid=grid, level=level, **kw)
    print('mesh_fidelity on the 48^3 generator:', json.dumps({k: v for k, v in fid.items() if k.startswith('mean_')}))
    assert fid['views'] == 18 and all(len(fid[k]) == 18 for k in ('psnr', 'psnr_covered', 'silhouette_iou'))
    assert all(np.isfinite(fid[k]) for k in ('mean_psnr', 'mean_psnr_covered', 'mean_silhouette_iou')) and np.isfinite(fid['psnr']).all()
    assert fid['mean_silhouette_iou'] > 0.5
    # the videos
    mesh = dict(verts=verts, faces=faces, grid_res=RES, uv=att['uv'], texture=att['texture'])
    for beside, width in ((None, res), ('image', 2 * res), ('shape', 2 * res)):
        path = str(tmp_path / f'mesh_{beside}.avi')
        n = VID.write_mesh_video(G, mesh, path, num_frames=5, beside=beside, ws=ws, batch=2, res=res, synthesis_kwargs=kw,
                                 shape_kwargs=dict(grid=grid, level=level))
        data = open(path, 'rb').read()
        total, entries = _avi_frames(data)
        assert n == 5 and total == 5 and len(entries) == 5
        assert struct.unpack('<II', data[32 + 32:32 + 40]) == (width, res)
    orbit_path = str(tmp_path / 'orbit.avi')
    assert VID.write_orbit_video(G, ws, orbit_path, num_frames=3, batch=2, **kw) == 3
    frames = torch.stack([f.float().clone() for f in INF.render_orbit(G, ws, num_frames=3, **kw)])
    by_hand = str(tmp_path / 'by_hand.avi')
    with VID.MjpegAviWriter(by_hand, res, res, fps=60) as w:
        for lo in (0, 2):
            data, offsets = H.jpeg_encode(frames[lo:lo + 2], quality=90)
            host, off = data.cpu().numpy(), offsets.tolist()
            for i in range(len(off) - 1):
                w.write(host[off[i]:off[i + 1]].tobytes())
    assert open(orbit_path, 'rb').read() == open(by_hand, 'rb').read()
    # a frame without the flip of grid axis 0 mirrors: the rasteriser sees faces[:, [0, 2, 1]] and the uv rows in that order
    monkeypatch.setattr(INF, 'grid_frame', lambda G, res: ((-0.5, -0.5, -0.5), (1.0 / (res - 1),) * 3, (0, 1, 2)))
    world2, wfaces2 = INF.mesh_to_world(G, verts, faces, RES)
    assert torch.equal(wfaces2, faces[:, [0, 2, 1]])
    mir = INF.render_mesh(G, verts, faces, cams[:2], mode='texture', uv=att['uv'], texture=att['texture'], grid_res=RES, cull='none')
    hand = H.mesh_raster(world2, wfaces2, cams[:2].contiguous(), res, mode='texture', uv=att['uv'][:, [0, 2, 1]].contiguous(), texture=att['texture'], cull='none')
    for k in OUTPUTS:
        assert torch.equal(_tb(mir[k]), _tb(hand[k])), k
    assert bool(mir['mask'].any())
