"""Coloured meshes without a GPU: the numpy restatement of the mesh-attribute kernels (tests/support/mesh_ref.py, what
tests/test_gpu_mesh_color.py requires the GPU outputs to equal bit for bit) checked against things that are not ours -- the radial direction
and an analytic texture of a sphere, ray-sphere intersection for the views, the silhouette of an occluder -- and the host side: the PLY
writer's optional properties, mesh_to_world's winding, the parameter structures against the header, argument errors of the two entries."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import iso_ref as IR  # noqa: E402
import mc_ref as MC  # noqa: E402
import mesh_ref as MR  # noqa: E402
from inv3d_amd import inference as I  # noqa: E402

N = 33
VS = 1.0 / (N - 1)                                       # the grid spans [-0.5, 0.5] along each of its world axes
FRAMES = dict(plain=dict(origin=(-0.5, -0.5, -0.5), spacing=(VS, VS, VS), axes=(0, 1, 2)),
              flipped=dict(origin=(0.5, -0.5, -0.5), spacing=(-VS, VS, VS), axes=(0, 1, 2)),
              permuted=dict(origin=(0.5, -0.5, -0.5), spacing=(-VS, VS, VS), axes=(2, 0, 1)))


def grid_world(frame):
    """[N,N,N,3] world coordinate of every grid point of a frame"""
    idx = np.stack(np.meshgrid(*[np.arange(N, dtype=np.float64)] * 3, indexing='ij'), -1)
    w = np.zeros_like(idx)
    for a in range(3):
        w[..., frame['axes'][a]] = frame['origin'][a] + idx[..., a] * frame['spacing'][a]
    return w


def verts_world(verts, frame):
    """marching-cubes vertices (column k = grid axis 2 - k, voxel units) in world coordinates, fp32 product then sum like mesh_to_world"""
    w = np.zeros_like(verts)
    for k in range(3):
        a = 2 - k
        w[:, frame['axes'][a]] = verts[:, k] * np.float32(frame['spacing'][a]) + np.float32(frame['origin'][a])
    return w


def spheres(frame, balls):
    """max over balls (centre, radius) of radius - |x - centre| on the grid"""
    w = grid_world(frame)
    return np.max([r - np.linalg.norm(w - np.asarray(c), axis=-1) for c, r in balls], axis=0).astype(np.float32)


def camera(m=None, yaw=math.pi / 2, pitch=math.pi / 2, radius=2.7, focal=4.2647, sk=0.0, cx=0.5, cy=0.5):
    m = I.lookat_pose(yaw, pitch, (0., 0., 0.), radius) if m is None else torch.as_tensor(m, dtype=torch.float32)
    return torch.cat([m.reshape(16), torch.tensor([focal, sk, cx, 0, focal, cy, 0, 0, 1.])]).numpy().astype(np.float32)


CANONICAL = [[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2.7], [0, 0, 0, 1]]      # on the +z axis, looking at the origin


def ray_spheres(cams, res, balls):
    """Float64 ray-sphere intersection per pixel of cams [F,25]: (depth [F,res,res] fp32, 0 on a miss; mask uint8; hit points [F,res,res,3])."""
    F = cams.shape[0]
    o, d = IR.rays(cams, res, np.arange(F * res * res), np.float64)
    best = np.full(F * res * res, np.inf)
    for c, r in balls:
        oc = o - np.asarray(c, dtype=np.float64)
        b = (oc * d).sum(1)
        disc = b * b - ((oc * oc).sum(1) - r * r)
        t = -b - np.sqrt(np.maximum(disc, 0.0))
        best = np.where((disc > 0) & (t > 0) & (t < best), t, best)
    hit = np.isfinite(best)
    depth = np.where(hit, best, 0.0)
    pts = o + depth[:, None] * d
    return depth.astype(np.float32).reshape(F, res, res), hit.astype(np.uint8).reshape(F, res, res), pts.reshape(F, res, res, 3)


def texture(p):
    """a smooth colour in [-1, 1] of a world point [..., 3] -> [..., 3]"""
    return np.stack([0.8 * np.sin(3.0 * p[..., 0] + 0.5), 0.8 * np.cos(2.0 * p[..., 1] - 0.3), 0.6 * np.sin(2.5 * p[..., 2]) + 0.2 * p[..., 0]], -1)


# ---- the PLY writer ----------------------------------------------------------------------------------------------------------------------

def _parse_ply(data):
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode('ascii').splitlines()
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0']
    elems, cur = [], None
    for l in lines[2:]:
        w = l.split()
        if w[0] == 'element':
            cur = (w[1], int(w[2]), [])
            elems.append(cur)
        elif w[0] == 'property':
            cur[2].append(w[1:])
    return elems, body


def test_ply_with_attributes_round_trips(tmp_path):
    rng = np.random.RandomState(0)
    v, n = rng.normal(size=(7, 3)).astype(np.float32), rng.normal(size=(7, 3)).astype(np.float32)
    c = rng.randint(0, 256, (7, 3)).astype(np.uint8)
    f = rng.randint(0, 7, (5, 3)).astype(np.int32)
    kinds = dict(x='<f4', y='<f4', z='<f4', nx='<f4', ny='<f4', nz='<f4', red='u1', green='u1', blue='u1')
    for normals, colors, names in ((n, c, ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue']), (n, None, ['x', 'y', 'z', 'nx', 'ny', 'nz']),
                                   (None, c, ['x', 'y', 'z', 'red', 'green', 'blue'])):
        path = str(tmp_path / 'a.ply')
        I.write_ply(path, torch.from_numpy(v), f, normals=normals, colors=None if colors is None else torch.from_numpy(colors))
        elems, body = _parse_ply(open(path, 'rb').read())
        assert [(e[0], e[1]) for e in elems] == [('vertex', 7), ('face', 5)]
        assert [p[-1] for p in elems[0][2]] == names
        assert [p[0] for p in elems[0][2]] == ['float' if kinds[k] == '<f4' else 'uchar' for k in names]
        assert elems[1][2] == [['list', 'uchar', 'int', 'vertex_indices']]
        dt = np.dtype([(k, kinds[k]) for k in names])
        rec = np.frombuffer(body[:7 * dt.itemsize], dt)
        assert np.array_equal(np.stack([rec['x'], rec['y'], rec['z']], 1).view(np.uint32), v.view(np.uint32))
        if normals is not None:
            assert np.array_equal(np.stack([rec['nx'], rec['ny'], rec['nz']], 1).view(np.uint32), n.view(np.uint32))
        if colors is not None:
            assert np.array_equal(np.stack([rec['red'], rec['green'], rec['blue']], 1), c)
        fr = np.frombuffer(body[7 * dt.itemsize:], np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
        assert len(fr) == 5 and np.all(fr['n'] == 3) and np.array_equal(fr['i'], f)
    with pytest.raises(ValueError):
        I.write_ply(str(tmp_path / 'b.ply'), v, f, normals=n[:3])


def test_ply_without_vertices_or_attributes(tmp_path):
    """V = 0 with attributes; and without attributes the bytes of the reference's file, assembled here by hand."""
    path = str(tmp_path / 'e.ply')
    I.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8))
    elems, body = _parse_ply(open(path, 'rb').read())
    assert [(e[0], e[1]) for e in elems] == [('vertex', 0), ('face', 0)] and len(elems[0][2]) == 9 and body == b''
    v = np.array([[0.5, -1.25, 3.0], [1.0, 2.0, 4.5]], np.float32)
    f = np.array([[0, 1, 1]], np.int32)
    I.write_ply(path, v, f)
    want = (b'ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n'
            b'element face 1\nproperty list uchar int vertex_indices\nend_header\n'
            + b''.join(np.float32(x).tobytes() for x in (0.5, -1.25, 3.0, 1.0, 2.0, 4.5)) + b'\x03' + b''.join(np.int32(i).tobytes() for i in (0, 1, 1)))
    assert open(path, 'rb').read() == want
    I.write_ply(path, v, f, normals=None, colors=None)
    assert open(path, 'rb').read() == want


# ---- normals -----------------------------------------------------------------------------------------------------------------------------

R0 = 0.3


@pytest.fixture(scope='module')
def sphere_mesh():
    """per frame: (vol, verts, faces, world vertices, restated normals) of the sphere r0 - |x| at level 0"""
    out = {}
    for name, frame in FRAMES.items():
        vol = spheres(frame, [((0., 0., 0.), R0)])
        v, f = MC.marching_cubes(vol, 0.0)
        w = verts_world(v, frame)
        out[name] = (vol, v, f, w, MR.normals(vol, w, **frame))
    return out


ANGLE_MEASURED = 0.1211                                  # degrees


@pytest.mark.parametrize('name', sorted(FRAMES))
def test_sphere_normals_are_radial(sphere_mesh, name):
    """f = r0 - |x|, r0 = 0.3, on the 33^3 grid over [-0.5, 0.5]^3: the restated normal at the 1758 marching-cubes vertices against x / |x|.
    The difference is the discretisation error of central differences of a trilinear field.  Measured on the CPU (fp32 restatement): the
    largest angle is 0.1211 degrees in all three frames (the sphere is symmetric under the flips and permutations); bound = 2 x that."""
    vol, v, f, w, n = sphere_mesh[name]
    assert len(v) > 1000 and n.dtype == np.float32
    w64 = w.astype(np.float64)
    radial = w64 / np.linalg.norm(w64, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    ang = np.degrees(np.arccos(np.clip((n * radial).sum(1), -1, 1)))
    print(f'{name}: {len(v)} vertices, largest angle {ang.max():.4f} degrees')
    assert ang.max() <= 2 * ANGLE_MEASURED


def test_normals_that_are_exactly_zero():
    """A constant grid has no gradient; a NaN anywhere in the 24 cells of the difference stencil, or in the point, gives exactly 0."""
    frame = FRAMES['flipped']
    pts = np.array([[0.01, 0.02, 0.03], [0.4, -0.4, 0.1], [5.0, 0.0, 0.0]], np.float32)
    assert not MR.normals(np.full((N, N, N), 2.5, np.float32), pts, **frame).any()
    vol = spheres(frame, [((0., 0., 0.), R0)])
    vol[14:19, 14:19, 14:19] = np.nan
    got = MR.normals(vol, np.array([[0.01, 0.02, 0.03], [0.3, 0.0, 0.0], [np.nan, 0.0, 0.3], [0.0, 0.3, np.nan]], np.float32), **frame)
    assert not got[[0, 2, 3]].any() and abs(np.linalg.norm(got[1]) - 1) < 1e-6
    assert np.array_equal(np.signbit(got[[0, 2, 3]]), np.zeros((3, 3), bool))


# ---- the bake ----------------------------------------------------------------------------------------------------------------------------

BAKE_MEASURED = 0.00264                                  # colour units ([-1, 1])


def test_textured_sphere(sphere_mesh):
    """The sphere's marching-cubes vertices and restated normals, three cameras on the frontal side (focal 3.4: the sphere fills most of the
    frame), 32^2 images and 16^2 depth maps from float64 ray-sphere intersection, colour = texture(hit point); depth_tol two voxels, power 2,
    cos_min 0.5 (the bilinear footprint of a contributing view then stays inside the silhouette: cos 0.5 lies 1.6 image pixels from it).
    The baked colour of every seen vertex against texture(r0 x / |x|): the difference is the bilinear sampling error of the 32^2 images (plus
    the vertex's distance to the true sphere, under 0.02 voxel).  Measured on the CPU (fp32 restatement): worst error 0.00264 over the 670
    seen vertices (38.1 % seen, 61.9 % not); bound = 2 x that."""
    vol, v, f, w, n = sphere_mesh['flipped']
    cams = np.stack([camera(yaw=math.pi / 2 + dy, pitch=math.pi / 2 + dp, focal=3.4) for dy, dp in ((0.0, 0.0), (0.7, 0.1), (-0.6, -0.2))])
    ball = [((0., 0., 0.), R0)]
    _, _, pts = ray_spheres(cams, 32, ball)
    images = np.ascontiguousarray(texture(pts).transpose(0, 3, 1, 2)).astype(np.float32)
    depth, mask, _ = ray_spheres(cams, 16, ball)
    assert 0 < mask.sum() < mask.size
    fallback = np.random.RandomState(1).uniform(-1, 1, w.shape).astype(np.float32)
    cos_min = 0.5
    out = MR.bake(w, n, images, depth, mask, cams, fallback=fallback, depth_tol=2 * VS, cos_min=cos_min, power=2)
    w64 = w.astype(np.float64)
    radial = w64 / np.linalg.norm(w64, axis=1, keepdims=True)
    o = cams[:, [3, 7, 11]].astype(np.float64)
    toward = o[None] - w64[:, None]
    cosv = (radial[:, None] * toward).sum(-1) / np.linalg.norm(toward, axis=-1)               # [V,F] analytic cosine to every camera
    seen = out['views'] > 0
    print(f'textured sphere: seen {seen.mean():.3f}, unseen {1 - seen.mean():.3f}, views histogram {np.bincount(out["views"])}')
    assert seen.mean() >= 1 / 3 and (~seen).mean() >= 1 / 10
    err = np.abs(out['color'][seen].astype(np.float64) - texture(R0 * radial[seen])).max()
    print(f'textured sphere: worst colour error {err:.5f}')
    # vertices that face no camera (the analytic cosine is below cos_min by more than the normals' error) take the fallback exactly
    away = (cosv < cos_min - 0.01).all(1)
    assert away.mean() >= 1 / 10
    assert not out['views'][away].any() and not out['weight'][away].any()
    assert np.array_equal(out['color'][away].view(np.uint32), fallback[away].view(np.uint32))
    assert np.array_equal(out['color'][~seen].view(np.uint32), fallback[~seen].view(np.uint32))
    # vertices that squarely face a camera are seen by it
    assert seen[(cosv > cos_min + 0.1).any(1)].all()
    assert err <= 2 * BAKE_MEASURED


def test_occlusion():
    """A small sphere (radius 0.1 at z = 0.3) between the camera on the +z axis and a large one (radius 0.25 at z = -0.1), one 32^2 depth map of
    both from float64 ray-sphere intersection; the vertices are the large sphere's.  Both spheres sit on the optical axis, so the near one's
    silhouette is the circle of radius rho = focal * tan(asin(r / d)) around the image centre (5.7 depth pixels).  The visibility test reads the
    four depth pixels around the projection, whose centres lie within one pixel per axis (1.41 pixels) of it: a vertex more than 1.5 pixels
    inside the silhouette meets only the near sphere's depth (0.27 world units in front of it, against a tolerance of 0.0625) and takes no
    colour; a vertex more than 1.5 pixels outside that squarely faces the camera (cosine above 0.5) meets only its own sphere and does."""
    frame = FRAMES['plain']
    near, far = ((0., 0., 0.3), 0.1), ((0., 0., -0.1), 0.25)
    cam = camera(CANONICAL)[None]
    Rr = 32
    depth, mask, _ = ray_spheres(cam, Rr, [near, far])
    images = np.full((1, 3, 8, 8), 0.25, np.float32)
    vol = spheres(frame, [far])
    v, _ = MC.marching_cubes(vol, 0.0)
    w = verts_world(v, frame)
    n = MR.normals(vol, w, **frame)
    out = MR.bake(w, n, images, depth, mask, cam, depth_tol=2 * VS, cos_min=0.1, power=2)
    _, t, c2, xc, yc = MR.project(cam[0], w.astype(np.float64), np.float64)
    rad = np.hypot(xc - 0.5, yc - 0.5)
    d_near = 2.7 - near[0][2]
    rho = 4.2647 * math.tan(math.asin(near[1] / d_near))
    w64 = w.astype(np.float64) - np.asarray(far[0])
    toward = np.array([0, 0, 2.7]) - w.astype(np.float64)
    cosv = (w64 * toward).sum(1) / (np.linalg.norm(w64, axis=1) * np.linalg.norm(toward, axis=1))
    inside = (rad < rho - 1.5 / Rr) & (cosv > 0)
    outside = (rad > rho + 1.5 / Rr) & (cosv > 0.5)
    print(f'occlusion: rho {rho * Rr:.2f} depth pixels, {inside.sum()} vertices inside the silhouette, {outside.sum()} outside and facing')
    assert inside.sum() >= 20 and outside.sum() >= 100
    assert not out['views'][inside].any() and not out['color'][inside].any()
    assert (out['views'][outside] == 1).all() and (out['color'][outside] == 0.25).all()


# ---- host side ---------------------------------------------------------------------------------------------------------------------------

def _fake_g(box=1.0):
    return types.SimpleNamespace(rendering_kwargs=dict(box_warp=box))


def _face_dots(verts, faces, normals):
    tri = verts.astype(np.float64)[faces]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return (fn * normals.astype(np.float64)[faces].mean(1)).sum(1)


@pytest.mark.parametrize('mirrored', [False, True])
def test_mesh_to_world_keeps_the_winding(monkeypatch, mirrored):
    """The sphere in density_grid's frame (grid_frame: axis 0 flipped; the voxel -> world map is then a proper rotation) and in a frame without
    the flip (the map mirrors, so the faces must come back re-wound): in the voxel frame and in the world frame every face's right-hand normal
    has a positive dot product with the mean of its vertices' normals."""
    G = _fake_g()
    if mirrored:
        monkeypatch.setattr(I, 'grid_frame', lambda G, res: ((-0.5, -0.5, -0.5), (1.0 / (res - 1),) * 3, (0, 1, 2)))
    origin, spacing, axes = I.grid_frame(G, N)
    frame = dict(origin=origin, spacing=spacing, axes=axes)
    vol = spheres(frame, [((0., 0., 0.), R0)])
    v, f = MC.marching_cubes(vol, 0.0)
    world, wf = I.mesh_to_world(G, torch.from_numpy(v), torch.from_numpy(f), N)
    world, wf = world.numpy(), wf.numpy()
    assert np.array_equal(world.view(np.uint32), verts_world(v, frame).view(np.uint32))
    assert np.array_equal(wf, f[:, [0, 2, 1]] if mirrored else f)
    assert I.mesh_to_world(G, torch.from_numpy(v), None, N)[1] is None
    n_world = MR.normals(vol, world, **frame)
    n_mesh = I.normals_to_mesh(G, torch.from_numpy(n_world), N).numpy()
    assert _face_dots(world, wf, n_world).min() > 0
    assert _face_dots(v, f, n_mesh).min() > 0
    # the mesh-frame normals are the radial direction of the voxel-frame sphere
    centred = v.astype(np.float64) - (N - 1) / 2
    assert ((n_mesh * centred).sum(1) / np.linalg.norm(centred, axis=1)).min() > 0.999


def test_bake_cameras():
    cams = I.bake_cameras()
    assert tuple(cams.shape) == (15, 25) and cams.dtype == torch.float32
    front = torch.cat([I.lookat_pose(math.pi / 2, math.pi / 2, (0., 0., 0.), 2.7).reshape(16), torch.tensor([4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.])])
    assert torch.equal(cams[7], front)                                       # the middle of 3 x 5 is the frontal camera
    assert torch.equal(I.bake_cameras(1, 1)[0], front)
    pos = cams[:, [3, 7, 11]]
    assert float((pos.norm(dim=1) - 2.7).abs().max()) < 1e-5 and len({tuple(p.tolist()) for p in pos}) == 15
    assert tuple(I.bake_cameras(2, 4, focal=2.0).shape) == (8, 25) and float(I.bake_cameras(2, 4, focal=2.0)[0, 16]) == 2.0


def test_structures_match_the_header():
    """eg3d_mesh_normals_params / eg3d_mesh_bake_params of inv3d_amd/_lib.py against their C definitions (gcc), as test_host.py does."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {']
    want = []
    for cname, cls in (('eg3d_mesh_normals_params', L.MeshNormalsParams), ('eg3d_mesh_bake_params', L.MeshBakeParams)):
        src.append(f' printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            src.append(f' printf("%zu\\n", offsetof({cname}, {f[0]}));')
            want.append(getattr(cls, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_wrappers_and_options_refuse_bad_arguments():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.coach import InversionCoach
    z = torch.zeros
    with pytest.raises(Eg3dHipError):
        H.mesh_normals(z(4, 4, 4), z(5, 3), (0, 0, 0), (1, 1, 1))
    with pytest.raises(Eg3dHipError):
        H.mesh_bake(z(5, 3), z(5, 3), z(1, 3, 8, 8), z(1, 8, 8), z(1, 8, 8, dtype=torch.uint8), z(1, 25))
    with pytest.raises(ValueError):
        InversionCoach(None, gen_mesh=True, mesh_dir='m', mesh_format='.mrc', mesh_colors=True, w_avg_samples=0)
    with pytest.raises(ValueError):
        I.color_mesh(None, None, z(0, 3), 8, source='texture')


def test_entries_reject_bad_arguments_before_any_launch():
    """Every error code of the two entries, answered from the arguments alone (no GPU here: a launch would be an error of its own); V = 0 is a
    normal result with no launch.  tests/test_gpu_mesh_color.py runs this again where a launch would succeed."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    OK, INVALID, UNSUPPORTED, TOO_LARGE = 0, -1, -2, -3
    a = 0x1000                                                                  # a non-null pointer that is never dereferenced
    nan, inf = float('nan'), float('inf')

    def normals(**kw):
        axes, origin, spacing = kw.pop('axes', (0, 1, 2)), kw.pop('origin', (0., 0., 0.)), kw.pop('spacing', (1., -1., 1.))
        p = L.MeshNormalsParams(**dict(dict(vol=a, points=a, normals=a, V=0, D0=16, D1=16, D2=16), **kw))
        p.axes[:], p.origin[:], p.spacing[:] = axes, origin, spacing
        return lib.eg3d_mesh_normals(C.byref(p), None)

    def bake(**kw):
        p = L.MeshBakeParams(**dict(dict(points=a, normals=a, cams=a, images=a, depth=a, mask=a, fallback=a, color=a, rgb=a, weight=a, views=a, V=0, F=3,
                                         H=8, R=8, depth_tol=0.01, cos_min=0.1, power=2), **kw))
        return lib.eg3d_mesh_bake(C.byref(p), None)
    assert lib.eg3d_mesh_normals(None, None) == INVALID and lib.eg3d_mesh_bake(None, None) == INVALID
    assert normals() == OK and normals(points=None, normals=None) == OK         # V = 0
    for bad in (dict(vol=None), dict(V=5, points=None), dict(V=5, normals=None), dict(V=-1), dict(D0=1), dict(D2=0), dict(axes=(0, 1, 1)), dict(axes=(0, 1, 3)),
                dict(spacing=(1., 0., 1.)), dict(spacing=(1., nan, 1.)), dict(spacing=(inf, 1., 1.)), dict(origin=(0., inf, 0.)), dict(origin=(nan, 0., 0.))):
        assert normals(**bad) == INVALID, bad
    assert normals(D0=2048, D1=2048, D2=512) == TOO_LARGE and normals(V=2 ** 31) == TOO_LARGE
    assert bake() == OK and bake(points=None, normals=None, fallback=None, color=None, rgb=None, weight=None, views=None) == OK
    for bad in (dict(cams=None), dict(images=None), dict(depth=None), dict(mask=None), dict(V=5, points=None), dict(V=5, normals=None), dict(V=-1), dict(F=0),
                dict(H=0), dict(R=0), dict(depth_tol=-0.5), dict(depth_tol=nan), dict(depth_tol=inf), dict(cos_min=-0.1), dict(cos_min=1.0), dict(cos_min=nan),
                dict(power=0), dict(power=9)):
        assert bake(**bad) == INVALID, bad
    for bad in (dict(F=256), dict(H=16385), dict(R=16385)):
        assert bake(**bad) == UNSUPPORTED, bad
    assert bake(V=2 ** 31) == TOO_LARGE
