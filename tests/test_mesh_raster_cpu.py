"""Mesh previews without a GPU: the rasteriser of include/eg3d_hip.h "Mesh previews" as tests/support/raster_ref.py restates it (what
tests/test_gpu_mesh_raster.py requires the GPU outputs to equal bit for bit) checked for the properties the specification promises --
watertight coverage, independence of the face order, depth, texture fetches, the front-face sign on a closed mesh, agreement with the
iso-surface marcher -- and the host side: the parameter structure against the header, every error code, the wrappers' and the tool's
argument checks."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import iso_ref as IR  # noqa: E402
import mc_ref as MC  # noqa: E402
import raster_ref as RR  # noqa: E402
import texture_ref as TR  # noqa: E402
from test_mesh_color_cpu import CANONICAL, _fake_g, camera  # noqa: E402
from inv3d_amd import inference as I  # noqa: E402

F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def quad(half, z):
    """two faces sharing the diagonal v0 - v2 of the square |x|, |y| <= half at height z, wound to face a camera on the +z axis"""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], F32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# ---- properties of the restatement -------------------------------------------------------------------------------------------------------

def test_two_faces_cover_a_frame_exactly():
    """A quad of half-width 0.5 in the plane z = 0 overfills the 16^2 frame of the canonical camera (half-width 0.317 there): every pixel is
    covered, by face 0 below the shared diagonal and face 1 above it; on the diagonal itself (x + y = 15, where both faces cover the pixel
    centre up to rounding) either may win, and the barycentrics sum to 1."""
    v, f = quad(0.5, 0.0)
    cam = camera(CANONICAL)[None]
    for cull in ('back', 'none'):
        out = RR.raster(v, f, cam, 16, mode='vertex', colors=np.zeros((4, 3), F32), cull=cull)
        assert out['mask'].all() and out['mask'].sum() == 256
        y, x = np.mgrid[0:16, 0:16]
        face = out['face'][0]
        assert (face[x + y > 15] == 0).all() and (face[x + y < 15] == 1).all() and np.isin(face[x + y == 15], (0, 1)).all()
        assert np.abs(out['bary'].sum(-1) - 1).max() < 1e-6 and out['bary'].min() >= 0
        assert out['large_faces'] == 2 and out['small_faces'] == 0
    # seen from behind there is nothing with culling, and the same coverage without
    back = camera([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, -2.7], [0, 0, 0, 1]])[None]
    assert not RR.raster(v, f, back, 16, mode='vertex', colors=np.zeros((4, 3), F32), cull='back')['mask'].any()
    assert RR.raster(v, f, back, 16, mode='vertex', colors=np.zeros((4, 3), F32), cull='none')['mask'].all()


def _soup(seed, F=60, V=40):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-0.35, 0.35, (V, 3)).astype(F32)
    f = rng.randint(0, V, (F, 3)).astype(np.int32)
    r = rng.randint(0, 3, F).astype(np.uint8)
    Ht, Wt, _ = TR.size(F, 8)
    return dict(v=v, f=f, uv=TR.uv(F, 8, r), tex=rng.randint(0, 256, (Ht, Wt, 3)).astype(np.uint8), col=rng.uniform(-1, 1, (V, 3)).astype(F32),
                nrm=rng.normal(size=(V, 3)).astype(F32))


def test_the_face_order_does_not_matter():
    """60 random faces that cross one another: shuffling them (uv permuted alike) leaves z, depth, mask and image bit-identical in the three
    modes; two copies of one face resolve to the lower index wherever that face is seen."""
    s = _soup(1)
    cams = np.stack([camera(CANONICAL), camera(yaw=math.pi / 2 + 0.4, pitch=math.pi / 2 - 0.2)])
    perm = np.random.RandomState(2).permutation(60)
    for mode in RR.MODES:
        kw = dict(mode=mode, texture=s['tex'], colors=s['col'], normals=s['nrm'], cull='none')
        a = RR.raster(s['v'], s['f'], cams, 33, uv=s['uv'], **kw)
        b = RR.raster(s['v'], s['f'][perm], cams, 33, uv=s['uv'][perm], **kw)
        assert 0.3 < a['mask'].mean() < 1.0
        for k in ('z', 'depth', 'mask', 'image'):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (mode, k)
        assert np.array_equal(perm[b['face'][b['mask'] > 0]], a['face'][a['mask'] > 0])
    a = RR.raster(s['v'], s['f'], cams, 33, mode='vertex', colors=s['col'], cull='none')
    k = int(np.bincount(a['face'][a['mask'] > 0]).argmax())                      # the face seen most
    seen = int((a['face'] == k).sum())
    assert seen > 10
    after = RR.raster(s['v'], np.concatenate([s['f'], s['f'][k:k + 1]]), cams, 33, mode='vertex', colors=s['col'], cull='none')      # again as face 60
    assert np.array_equal(after['face'], a['face']) and not (after['face'] == 60).any()
    before = RR.raster(s['v'], np.concatenate([s['f'][k:k + 1], s['f']]), cams, 33, mode='vertex', colors=s['col'], cull='none')     # again as face 0
    assert (before['face'] == 0).sum() == seen and not (before['face'] == k + 1).any()
    for c in (after, before):
        assert np.array_equal(_bits(a['image']), _bits(c['image'])) and np.array_equal(_bits(a['z']), _bits(c['z']))


def test_depth_of_a_fronto_parallel_quad():
    """A quad at height 0.2 under the canonical camera (at height 2.7): camera depth z0 = 2.5 at every vertex.  z = 1 / W with W the sum of
    three l_k / z0 whose l_k sum to 1 up to rounding: three divisions, two sums and the reciprocal, 4 ulp.  depth is z times the length of the
    pixel's lifted ray, formed in the operations the header names."""
    v, f = quad(0.5, 0.2)
    cam = camera(CANONICAL)
    out = RR.raster(v, f, cam[None], 16, mode='vertex', colors=np.zeros((4, 3), F32))
    assert out['mask'].all()
    z0 = F32(2.5)
    assert np.abs(out['z'].astype(np.float64) - 2.5).max() <= 4 * float(np.spacing(z0))
    y, x = np.mgrid[0:16, 0:16]
    xl, yl = RR.lift(cam, 16, x, y)
    want = out['z'][0] * np.sqrt((xl * xl + yl * yl) + F32(1))
    assert want.dtype == np.float32 and np.array_equal(_bits(out['depth'][0]), _bits(want))
    assert out['depth'].min() >= out['z'].min() and float(out['depth'][0, 0, 0]) > float(out['depth'][0, 8, 8])


def test_a_constant_atlas_gives_a_constant_image():
    s = _soup(3)
    tex = np.empty_like(s['tex'])
    tex[...] = (200, 17, 128)
    out = RR.raster(s['v'], s['f'], camera(CANONICAL)[None], 33, mode='texture', uv=s['uv'], texture=tex, cull='none', background=-0.25)
    hit = out['mask'][0] > 0
    assert 0.3 < hit.mean() < 1.0
    for j, c in enumerate((200, 17, 128)):
        assert (out['image'][0, j][hit] == (F32(c) - F32(127.5)) / F32(127.5)).all() and (out['image'][0, j][~hit] == F32(-0.25)).all()


# ---- a closed mesh: the front-face sign, and the marcher -------------------------------------------------------------------------------------

GRID, RADIUS, BOX, RES = 24, 8.0, 0.75, 64


@pytest.fixture(scope='module')
def sphere():
    """The marching-cubes sphere of radius 8 voxels in a 24^3 grid (level 0 of RADIUS - |i - centre|), in world coordinates through
    mesh_to_world on a box of side 0.75 (grid_frame's layout: axis 0 flipped) -- radius 0.26 where bake_cameras' frames are 0.63 wide, so that
    the disc fills about half of a frame -- and its culled views from bake_cameras() at 64^2 by the restatement."""
    G = _fake_g(BOX)
    idx = np.stack(np.meshgrid(*[np.arange(GRID, dtype=np.float64)] * 3, indexing='ij'), -1)
    vol = (RADIUS - np.linalg.norm(idx - (GRID - 1) / 2, axis=-1)).astype(F32)
    v, f = MC.marching_cubes(vol, 0.0)
    world, wf = I.mesh_to_world(G, torch.from_numpy(v), torch.from_numpy(f), GRID)
    world, wf = world.numpy(), np.ascontiguousarray(wf.numpy())
    origin, spacing, axes = I.grid_frame(G, GRID)
    cams = I.bake_cameras().numpy()
    normals = world / np.linalg.norm(world, axis=1, keepdims=True)
    kw = dict(mode='lambert', normals=normals.astype(F32))
    return dict(vol=vol, world=world, faces=wf, cams=cams, frame=dict(origin=origin, spacing=spacing, axes=axes), normals=normals.astype(F32),
                back=RR.raster(world, wf, cams, RES, cull='back', **kw))


def test_culling_on_a_closed_mesh(sphere):
    """On a closed surface every back face lies behind a front face, so culling changes no pixel: the face maps are identical.  That pins the
    sign (front faces have area2 < 0): with the other sign the culled frames would show the far hemisphere.  With the winding reversed they do:
    every face that was drawn is culled, and what is left lies beyond the tangent points (a closed mesh never gives an empty frame; the faces
    that were drawn, taken alone, do)."""
    world, faces, cams = sphere['world'], sphere['faces'], sphere['cams']
    back, none = sphere['back'], RR.raster(world, faces, cams, RES, mode='lambert', normals=sphere['normals'], cull='none')
    assert len(faces) > 1000 and MC.edge_pairing(faces) == (True, True) and MC.signed_volume(world, faces) > 0
    assert np.array_equal(back['face'], none['face']) and np.array_equal(_bits(back['depth']), _bits(none['depth']))
    assert 0.25 <= back['mask'].mean() <= 0.75
    drawn = back['small_faces'] + back['large_faces']
    assert 0.3 * 15 * len(faces) < drawn < 0.6 * 15 * len(faces)                                # about half of the faces face each camera
    assert none['small_faces'] + none['large_faces'] > 1.8 * drawn
    vs = BOX / (GRID - 1)
    tangent = math.sqrt(2.7 ** 2 - (RADIUS * vs) ** 2)                                          # the ray length to the silhouette of the sphere
    assert back['depth'][back['mask'] > 0].max() < tangent + vs
    kw = dict(mode='lambert', normals=sphere['normals'])
    rev = RR.raster(world, faces[:, [0, 2, 1]], cams[6:9], RES, cull='back', **kw)
    assert rev['mask'].mean() > 0.25 and rev['depth'][rev['mask'] > 0].min() > tangent - vs
    for i in range(3):
        assert not np.isin(rev['face'][i][rev['mask'][i] > 0], back['face'][6 + i][back['mask'][6 + i] > 0]).any()
    inner = RR.raster(world, faces[:, [0, 2, 1]], cams[6:9], RES, cull='none', **kw)
    # without culling the winding does not matter, up to the rounding of a sum whose terms swap places
    assert np.array_equal(inner['face'], none['face'][6:9]) and np.abs(inner['depth'] - none['depth'][6:9]).max() < 1e-5
    # the open cap that faces the frontal camera (float64, with a margin): reversed and culled, nothing of it is drawn
    tri = world.astype(np.float64)[faces]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    to_cam = cams[7][[3, 7, 11]].astype(np.float64) - tri.mean(1)
    cos = (fn * to_cam).sum(1) / (np.linalg.norm(fn, axis=1) * np.linalg.norm(to_cam, axis=1))
    cap = np.ascontiguousarray(faces[cos > 0.05])
    assert 0.3 * len(faces) < len(cap) < 0.5 * len(faces)
    assert RR.raster(world, cap, cams[7:8], RES, cull='back', **kw)['mask'].mean() > 0.25
    assert not RR.raster(world, cap[:, [0, 2, 1]], cams[7:8], RES, cull='back', **kw)['mask'].any()


def _erode(m):
    e = m.copy()
    e[:, 1:] &= m[:, :-1]
    e[:, :-1] &= m[:, 1:]
    e[:, :, 1:] &= m[:, :, :-1]
    e[:, :, :-1] &= m[:, :, 1:]
    e[:, 0] = e[:, -1] = False
    e[:, :, 0] = e[:, :, -1] = False
    return e


def depth_against_the_marcher(mesh_depth, mesh_mask, iso_depth, iso_mask, iso_normal, cams, res, spacing):
    """(largest difference, the bound, pixels compared, pixels doubly masked, covered share): the comparison the CPU and the GPU test share.
    Pixels where both masks, eroded by one pixel, are set and the marcher's surface faces the ray with -n.d >= 0.5.  Both surfaces pass
    through the same grid cells, so along a ray they are at most a cell diagonal over the facing cosine apart: sqrt(3) |spacing| / 0.5."""
    N = cams.shape[0]
    _, d = IR.rays(cams, res, np.arange(N * res * res))
    facing = -(iso_normal.reshape(-1, 3).astype(np.float64) * d.astype(np.float64)).sum(1).reshape(N, res, res)
    both = (mesh_mask > 0) & (iso_mask > 0)
    use = _erode(mesh_mask > 0) & _erode(iso_mask > 0) & (facing >= 0.5)
    diff = np.abs(mesh_depth.astype(np.float64) - iso_depth.astype(np.float64))[use]
    return float(diff.max()), math.sqrt(3.0) * abs(spacing) / 0.5, int(use.sum()), int(both.sum()), float((mesh_mask > 0).mean())


def test_depth_agrees_with_the_marcher(sphere):
    m = sphere['back']
    iso = IR.march(sphere['vol'], sphere['cams'], RES, 0.0, **sphere['frame'])
    N = len(sphere['cams'])
    worst, bound, used, both, covered = depth_against_the_marcher(m['depth'], m['mask'], iso['depth'].reshape(N, RES, RES), iso['mask'].reshape(N, RES, RES),
                                                                  iso['normal'].reshape(N, RES, RES, 3), sphere['cams'], RES, sphere['frame']['spacing'][1])
    print(f'sphere: {used} of {both} doubly masked pixels compared, covered {covered:.3f}, largest depth difference {worst:.5f}, bound {bound:.5f}')
    assert 0.25 <= covered <= 0.75
    assert used >= both / 2
    assert worst <= bound
    iou = ((m['mask'] > 0) & (iso['mask'].reshape(N, RES, RES) > 0)).sum() / ((m['mask'] > 0) | (iso['mask'].reshape(N, RES, RES) > 0)).sum()
    assert iou > 0.95


# ---- host side ---------------------------------------------------------------------------------------------------------------------------

def test_structure_matches_the_header():
    """eg3d_mesh_raster_params of inv3d_amd/_lib.py against its C definition (gcc), as tests/test_mesh_texture_cpu.py does for its own."""
    import shutil
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    cname, cls = 'eg3d_mesh_raster_params', L.MeshRasterParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', f' printf("%zu\\n", sizeof({cname}));']
    want = [C.sizeof(cls)]
    for f in cls._fields_:
        src.append(f' printf("%zu\\n", offsetof({cname}, {f[0]}));')
        want.append(getattr(cls, f[0]).offset)
    src += [' printf("%d %d %d %d\\n", EG3D_RASTER_TEXTURE, EG3D_RASTER_VERTEX, EG3D_RASTER_LAMBERT, EG3D_RASTER_SMALL);', ' return 0;', '}']
    want += [L.RASTER_TEXTURE, L.RASTER_VERTEX, L.RASTER_LAMBERT, L.RASTER_SMALL]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want and RR.SMALL == L.RASTER_SMALL


def test_entry_rejects_bad_arguments_before_any_launch():
    """Every error code of eg3d_mesh_raster and of its workspace query, answered from the arguments alone (no GPU here: a launch would be an
    error of its own); with no output bound the call is a normal result with no launch.  tests/test_gpu_mesh_raster.py runs this again where
    a launch would succeed."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    OK, INVALID, UNSUPPORTED, TOO_LARGE = 0, -1, -2, -3
    a = 0x1000                                                                  # a non-null, 16-byte aligned pointer that is never dereferenced
    nan, inf = float('nan'), float('inf')
    base = dict(points=a, faces=a, cams=a, uv=a, texture=a, colors=a, normals=a, workspace=a, workspace_bytes=1 << 40, V=10, F=7, N=3, res=8, Ht=8,
                Wt=16, mode=L.RASTER_TEXTURE, cull=1, near=0.1, background=1.0, ambient=0.2)

    def ras(**kw):
        p = L.MeshRasterParams(**dict(base, **kw))
        return lib.eg3d_mesh_raster(C.byref(p), None)

    def query(**kw):
        p = L.MeshRasterParams(**dict(base, **kw))
        n = C.c_int64(-1)
        return lib.eg3d_mesh_raster_query_workspace(C.byref(p), C.byref(n)), n.value
    assert lib.eg3d_mesh_raster(None, None) == INVALID and lib.eg3d_mesh_raster_query_workspace(None, None) == INVALID
    assert ras() == OK and ras(F=0, faces=None, uv=None) == OK and ras(V=0, points=None) == OK and ras(cull=0) == OK and ras(ambient=0.0) == OK
    assert ras(ambient=1.0) == OK and ras(Ht=2, Wt=2) == OK and ras(res=16384) == OK and ras(N=65535) == OK and ras(background=nan) == OK
    for mode, gone in ((L.RASTER_TEXTURE, ('colors', 'normals')), (L.RASTER_VERTEX, ('uv', 'texture', 'normals')), (L.RASTER_LAMBERT, ('uv', 'texture', 'colors'))):
        assert ras(mode=mode, Ht=0, Wt=0, **{k: None for k in gone}) == (INVALID if mode == L.RASTER_TEXTURE else OK)
        assert ras(mode=mode, **{k: None for k in gone}) == OK
    for bad in (dict(cams=None), dict(points=None), dict(faces=None), dict(uv=None), dict(texture=None), dict(mode=L.RASTER_VERTEX, colors=None),
                dict(mode=L.RASTER_LAMBERT, normals=None), dict(V=-1), dict(F=-1), dict(N=0), dict(res=0), dict(near=0.0), dict(near=-1.0), dict(near=nan),
                dict(near=inf), dict(mode=3), dict(mode=-1), dict(cull=2), dict(cull=-1), dict(ambient=-0.1), dict(ambient=1.1), dict(ambient=nan),
                dict(Ht=1), dict(Wt=1), dict(workspace=None), dict(workspace=a + 4), dict(workspace_bytes=0)):
        assert ras(**bad) == INVALID, bad
    for bad in (dict(res=16385), dict(N=65536), dict(Ht=16385), dict(Wt=16385)):
        assert ras(**bad) == UNSUPPORTED, bad
    assert ras(V=2 ** 31) == TOO_LARGE and ras(F=2 ** 31) == TOO_LARGE and ras(F=2 ** 30, N=2) == TOO_LARGE and ras(F=2 ** 31 - 1, N=1) == OK
    # the workspace: 8 bytes a pixel, 16 per view and vertex, 8 per view and face, the counters; what the query says is enough, a byte less is not
    rc, n = query()
    assert rc == OK and n == 3 * 8 * 8 * 8 + 3 * 10 * 16 + 16 * ((3 * 7 * 8 + 15) // 16) + 16
    assert ras(workspace_bytes=n) == OK and ras(workspace_bytes=n - 1) == INVALID
    assert query(near=0.0)[0] == INVALID and query(res=16385)[0] == UNSUPPORTED and query(V=2 ** 31)[0] == TOO_LARGE


def test_wrappers_and_options_refuse_bad_arguments(tmp_path):
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.coach import InversionCoach
    z = torch.zeros
    with pytest.raises(Eg3dHipError):                                          # host tensors
        H.mesh_raster(z(5, 3), z(2, 3, dtype=torch.int32), z(1, 25), 8, mode='vertex', colors=z(5, 3))
    base = dict(gen_mesh=True, mesh_dir='m', w_avg_samples=0)
    with pytest.raises(ValueError):                                            # a preview shows colours: a bare '.ply' or an '.mrc' has none
        InversionCoach(None, mesh_preview=True, mesh_format='.ply', **base)
    with pytest.raises(ValueError):
        InversionCoach(None, mesh_preview=True, mesh_format='.mrc', **base)
    with pytest.raises(ValueError):
        InversionCoach(None, mesh_preview=True, mesh_format='.obj', gen_mesh=False, w_avg_samples=0)
    G = torch.nn.Linear(1, 1)
    assert InversionCoach(G, mesh_format='.obj', **base).mesh_preview is False
    assert InversionCoach(G, mesh_format='.obj', mesh_preview=True, **base).mesh_preview is True
    with pytest.raises(ValueError):                                            # vertex colours are not what the preview shows
        InversionCoach(None, mesh_preview=True, mesh_format='.ply', mesh_colors=True, **base)
    for bad in (dict(mode='phong'), dict(supersample=0), dict(mode='texture'), dict(mode='vertex'), dict(mode='lambert')):
        with pytest.raises(ValueError):
            I.render_mesh(_fake_g(), z(4, 3), z(2, 3, dtype=torch.int32), z(1, 25), res=8, grid_res=16, **bad)
    with pytest.raises(ValueError):
        I.render_mesh(_fake_g(), z(4, 3), z(2, 3, dtype=torch.int32), z(1, 25), res=8, mode='lambert', normals=z(4, 3))      # no grid_res
    from inv3d_amd import video as VID
    with pytest.raises(ValueError):
        VID.write_mesh_video(None, dict(), str(tmp_path / 'a.avi'), beside='depth')
    with pytest.raises(ValueError):
        VID.write_mesh_video(None, dict(), str(tmp_path / 'a.avi'), num_frames=0)
    assert not os.listdir(tmp_path)
    # the tool refuses --preview without something to show, before it touches a GPU or a file
    tool = os.path.join(ROOT, 'tools', 'extract_mesh.py')
    r = subprocess.run([sys.executable, tool, '--ws', str(tmp_path / 'none.npy'), '--out', str(tmp_path / 'a.ply'), '--preview', str(tmp_path / 'p.png')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--preview' in r.stderr and not os.listdir(tmp_path)
    r = subprocess.run([sys.executable, tool, '--ws', str(tmp_path / 'none.npy'), '--out', str(tmp_path / 'a.obj'), '--obj', '--preview', str(tmp_path / 'p.gif')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--preview' in r.stderr and not os.listdir(tmp_path)


# ---- the GPU test's cases, checked here to make them not vacuous ---------------------------------------------------------------------------

def raster_inputs(N, F=200):
    """What tests/test_gpu_mesh_raster.py draws: the seeded faces of tests/test_mesh_texture_cpu.py over bake_inputs' 1000 vertices (NaN
    vertices, vertices behind the camera, at its origin and on the frame's edge, a repeated index, a third of zero area), the uv of an atlas
    with seeded corner rotations, a seeded atlas, the vertices' fallback colours and normals."""
    from test_gpu_mesh_color import bake_inputs
    from test_mesh_texture_cpu import texture_faces
    inp = bake_inputs(N, 8, 8)
    faces = texture_faces(inp)[:F]
    rng = np.random.RandomState(11)
    Ht, Wt, _ = TR.size(200, 8)
    uv = TR.uv(200, 8, rng.randint(0, 3, 200).astype(np.uint8))[:F]
    return dict(points=inp['points'], faces=np.ascontiguousarray(faces), cams=inp['cams'], uv=np.ascontiguousarray(uv),
                texture=rng.randint(0, 256, (Ht, Wt, 3)).astype(np.uint8), colors=np.ascontiguousarray(inp['fallback'], dtype=F32),
                normals=np.ascontiguousarray(inp['normals'], dtype=F32))


def ref_raster(inp, res, mode, cull, **kw):
    return RR.raster(inp['points'], inp['faces'], inp['cams'], res, mode=mode, uv=inp['uv'], texture=inp['texture'], colors=inp['colors'],
                     normals=inp['normals'], cull=cull, **kw)


def test_the_gpu_case_is_not_vacuous():
    """The 200-face case through the restatement alone, at the resolutions of more than one pixel that the GPU test draws: between a tenth
    and nine tenths of the pixels are covered, and both draw paths are taken.  (A 1 x 1 frame has no such share: its one pixel is covered or
    it is not.)"""
    for N in (1, 3):
        inp = raster_inputs(N)
        assert inp['faces'].shape == (200, 3) and inp['cams'].shape == (N, 25)
        for res in (7, 64, 65):
            for cull in ('back', 'none'):
                out = ref_raster(inp, res, 'vertex', cull)
                covered = float(out['mask'].mean())
                print(f'views {N}, res {res}, cull {cull}: covered {covered:.3f}, {out["small_faces"]} small and {out["large_faces"]} large faces')
                assert out['bad_faces'] == 0 and 0.1 <= covered <= 0.9, (N, res, cull, covered)
                # a frame of at most 8 x 8 pixels holds no large face; the others take both paths
                assert out['small_faces'] > 0 and (out['large_faces'] > 0) == (res > RR.SMALL)
