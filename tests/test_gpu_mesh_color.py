"""Coloured meshes on the GPU (csrc/mesh_bake.hip, hipops.mesh_normals / mesh_bake, inference.color_mesh, extract_mesh(attributes=True), the
coach's mesh_colors): both kernels EQUAL the numpy restatement tests/support/mesh_ref.py bit for bit, null outputs and error codes, run-to-run
and normal-vs-deterministic-build identity, and the generator-level pipeline against its composition by hand."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import mesh_ref as MR  # noqa: E402
from test_mesh_color_cpu import test_entries_reject_bad_arguments_before_any_launch as _error_codes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = (1, 63, 64, 65, 1000)                            # one lane, a wave minus / exactly / plus one, four blocks (the last one partial)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_bits(got, want, what):
    a, b = _bits(got).reshape(-1), _bits(np.asarray(want)).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), np.asarray(got).reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])


# ---- normals -----------------------------------------------------------------------------------------------------------------------------

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
    """the grids of tests/test_gpu_shape_render.py that the normals are checked on, built the same way"""
    rng = np.random.RandomState(3)
    padded = _sphere(0.3)
    for s in (np.s_[:3], np.s_[-3:]):
        padded[s] = padded[:, s] = padded[:, :, s] = -1000.0
    padded[rng.randint(0, 64, 300), rng.randint(0, 64, 300), rng.randint(0, 64, 300)] = np.nan
    padded[20:24, 30:40, 8:30] = np.nan
    return {
        '2x2x2': (rng.normal(size=(2, 2, 2)).astype(np.float32), _frame((2, 2, 2))),
        '17x17x17': (rng.normal(size=(17, 17, 17)).astype(np.float32), _frame((17, 17, 17))),
        '37x53x61': (rng.normal(size=(37, 53, 61)).astype(np.float32), _frame((37, 53, 61))),
        'negative_spacing': (_sphere(0.3), _frame((64, 64, 64), flip0=True)),
        'permuted_axes': (rng.normal(size=(37, 53, 61)).astype(np.float32), _frame((37, 53, 61), flip0=True, axes=(2, 0, 1))),
        'nan_and_padding': (padded, _frame((64, 64, 64))),
    }


def normal_points(shape, frame, n=1000, seed=0):
    """n world points for a grid: index coordinates strictly inside, exactly on grid planes (every coordinate an integer, the faces 0 and D - 1
    among them; the spacings of the 2^3 and 17^3 grids are powers of two, so those land exactly), outside the grid on either side, one NaN
    point; shuffled, so every prefix is a mixture."""
    rng = np.random.RandomState(seed)
    D = np.asarray(shape, dtype=np.float64)
    inside = rng.uniform(0, 1, (n // 2, 3)) * (D - 1)
    planes = np.floor(rng.uniform(0, 1, (n // 4, 3)) * D)
    planes[::3, rng.randint(0, 3)] = 0
    planes[1::3, 1] = D[1] - 1
    half = np.floor(rng.uniform(0, 1, (n // 8, 3)) * (D - 1)) + 0.5
    outside = rng.uniform(-3, 3, (n - n // 2 - n // 4 - n // 8, 3))
    outside = np.where(outside > 0, outside + D - 1, outside)
    outside[::2, 1] = rng.uniform(0, 1, len(outside[::2])) * (D[1] - 1)          # outside along some axes only
    idx = np.concatenate([inside, planes, half, outside])[rng.permutation(n)]
    world = np.zeros_like(idx)
    for a in range(3):
        world[:, frame['axes'][a]] = frame['origin'][a] + idx[:, a] * frame['spacing'][a]
    world = world.astype(np.float32)
    world[min(5, n - 1), 1] = np.nan
    return world


@pytest.mark.parametrize('name', sorted(grids()))
def test_normals_equal_the_restatement(name):
    from inv3d_amd import hipops as H
    vol, frame = grids()[name]
    pts = normal_points(vol.shape, frame)
    pts[0] = pts[7]                                                            # V = 1 is an ordinary point
    vd, pd = torch.from_numpy(vol).to(DEV), torch.from_numpy(pts).to(DEV)
    want = MR.normals(vol, pts, **frame)
    for V in SIZES:
        got = H.mesh_normals(vd, pd[:V].contiguous(), **frame)
        torch.cuda.synchronize()
        assert got.shape == (V, 3) and got.dtype == torch.float32
        _assert_bits(got.cpu().numpy(), want[:V], (name, V))
    lens = np.linalg.norm(want.astype(np.float64), axis=1)
    assert not want[5].any() and ((np.abs(lens - 1) < 1e-6) | (lens == 0)).all() and (lens > 0).sum() > 500
    if name == 'nan_and_padding':
        assert (lens == 0).sum() > 1                                           # NaN neighbourhoods, beside the NaN point
    assert H.mesh_normals(vd, pd[:0].contiguous(), **frame).shape == (0, 3)


# ---- the bake ----------------------------------------------------------------------------------------------------------------------------

TWO_VOXELS = 2.0 / 32


def bake_cameras():
    """cam0: on the +z axis at 2.5 looking at the origin, focal 4, principal point 0.5 -- every entry a short binary fraction, so pixel centres
    and frame edges can be hit exactly; cam1: a lookat_pose view with skew and an off-centre principal point; cam2: a plain lookat_pose view."""
    from inv3d_amd.inference import lookat_pose

    def cam(m, fx, fy, sk=0.0, cx=0.5, cy=0.5):
        return np.concatenate([np.asarray(m, dtype=np.float32).reshape(16), np.array([fx, sk, cx, 0, fy, cy, 0, 0, 1], np.float32)])
    return np.stack([cam([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2.5], [0, 0, 0, 1]], 4.0, 4.0),
                     cam(lookat_pose(math.pi / 2 + 0.5, math.pi / 2 - 0.2, (0., 0., 0.), 2.7).numpy(), 3.0, 3.2, sk=0.05, cx=0.52, cy=0.47),
                     cam(lookat_pose(math.pi / 2 - 0.6, math.pi / 2 + 0.3, (0.02, -0.01, 0.), 2.2).numpy(), 4.2647, 4.2647)])


def _unproject0(xc, yc, z):
    """the world point at height z that cam0 projects to the normalised image point (xc, yc): exact in fp32 for short binary fractions"""
    c2 = 2.5 - z
    return np.stack([(xc - 0.5) / 4.0 * c2, -((yc - 0.5) / 4.0 * c2), np.broadcast_to(z, np.shape(xc)) + 0 * xc], -1)


def bake_inputs(F, H, R, seed=0):
    """1000 vertices, shuffled, for the cameras bake_cameras()[:F] at image resolution H and depth resolution R:
      300 on cam0's optical axis (they project to xc = yc = 0.5 exactly: the only vertices a 1 x 1 frame can see), normals toward it
      400 anywhere in the box with random normals
      the 64 pixel centres of an 8^2 frame of cam0, and for r in {1, 8, 16, 37} its frame edges px = 0 and px = r - 1 exactly (where the edge is
        a binary fraction) with neighbours a few fp32 steps to either side
      40 inside the part of cam0's frame whose depth pixels are masked out (xc, yc < 0.3)
      behind cam0, at cam0's origin, zero normals, back-facing normals, NaN coordinates
      the rest in front of cam1 / cam2 with normals toward them
    depth: per pixel the camera's distance from the origin + U(-0.35, 0.25) (somewhat less than half of the box is in front of it), mask 85 % ones; cam0's
    centre pixels lie at 3.2 (behind the whole box) and are unmasked, its corner xc, yc < 0.3 is masked out (not for R = 1)."""
    rng = np.random.RandomState(seed + 17 * H + R)
    cams = bake_cameras()
    P, Nn = [], []
    z = rng.uniform(-0.4, 0.4, 300)
    P.append(np.stack([0 * z, 0 * z, z], 1))
    Nn.append(np.stack([rng.normal(0, 0.3, 300), rng.normal(0, 0.3, 300), np.ones(300)], 1))
    P.append(rng.uniform(-0.35, 0.35, (400, 3)))
    n = rng.normal(size=(400, 3))
    Nn.append(n / np.linalg.norm(n, axis=1, keepdims=True))
    i = (np.arange(8) + 0.5) / 8
    xc, yc = np.meshgrid(i, i)
    P.append(_unproject0(xc.reshape(-1), yc.reshape(-1), 0.5))
    Nn.append(np.tile([0.1, -0.2, 1.0], (64, 1)))
    edges = []
    for r in (1, 8, 16, 37):
        for e in (0.5 / r, (r - 0.5) / r):
            c = np.float32((e - 0.5) / 4.0 * 2.0)                              # cam0's camera-space x (or -y) of the edge at c2 = 2; 0 for r = 1
            d = np.float32(2.0 ** -23 if e >= 0.5 else -2.0 ** -23)              # a few fp32 steps of the image coordinate, outward
            for v in (np.float32(c + d), c, np.float32(c - d)):                # just outside the frame, the edge, just inside
                edges += [(v, 0.0), (0.0, v), (v, v)]
    edges = np.asarray(edges, dtype=np.float64)
    P.append(np.stack([edges[:, 0], -edges[:, 1], np.full(len(edges), 0.5)], 1))
    Nn.append(np.tile([0.0, 0.0, 1.0], (len(edges), 1)))
    xm, ym = rng.uniform(0.08, 0.2, 40), rng.uniform(0.08, 0.2, 40)
    P.append(_unproject0(xm, ym, rng.uniform(-0.3, 0.3, 40)))
    Nn.append(np.tile([0.0, 0.0, 1.0], (40, 1)))
    special_p = [[0.1, 0.1, 3.0], [0.0, 0.0, 2.75], [0.0, 0.0, 2.5], [0.0, 0.0, 0.1], [0.05, 0.0, 0.2], [0.0, 0.0, -0.1], [0.02, 0.03, 0.0],
                 [np.nan, 0.0, 0.0], [0.0, np.nan, 0.1], [0.0, 0.0, np.nan], [0.0, 0.0, 0.3]]
    special_n = [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, -1], [0.1, 0, -1],
                 [0, 0, 1], [0, 0, 1], [0, 0, 1], [np.nan, 0, 1]]
    P.append(np.asarray(special_p, dtype=np.float64))
    Nn.append(np.asarray(special_n, dtype=np.float64))
    rest = 1000 - sum(len(p) for p in P)
    pr = rng.uniform(-0.3, 0.3, (rest, 3))
    o = cams[1 + (np.arange(rest) % 2)][:, [3, 7, 11]].astype(np.float64)
    nr = o - pr
    P.append(pr)
    Nn.append(nr / np.linalg.norm(nr, axis=1, keepdims=True) + rng.normal(0, 0.2, (rest, 3)))
    perm = rng.permutation(1000)
    points, normals = np.concatenate(P)[perm].astype(np.float32), np.concatenate(Nn)[perm].astype(np.float32)
    images = rng.uniform(-1, 1, (3, 3, H, H)).astype(np.float32)
    dist = np.linalg.norm(cams[:, [3, 7, 11]], axis=1)
    depth = (dist[:, None, None] + rng.uniform(-0.35, 0.25, (3, R, R))).astype(np.float32)
    mask = (rng.uniform(0, 1, (3, R, R)) < 0.85).astype(np.uint8)
    c = (R - 1) / 2
    lo, hi = max(int(math.floor(c)) - 1, 0), min(int(math.ceil(c)) + 1, R - 1)
    depth[0, lo:hi + 1, lo:hi + 1] = 3.2
    mask[0, lo:hi + 1, lo:hi + 1] = 1
    if R > 1:
        k = int(math.ceil(0.3 * R))
        mask[0, :k, :k] = 0
    fallback = rng.uniform(-1, 1, (1000, 3)).astype(np.float32)
    return dict(points=points, normals=normals, images=np.ascontiguousarray(images[:F]), depth=np.ascontiguousarray(depth[:F]),
                mask=np.ascontiguousarray(mask[:F]), cams=np.ascontiguousarray(cams[:F]), fallback=fallback)


def _gpu_bake(inp, V, with_fallback=True, **kw):
    from inv3d_amd import hipops as H
    t = {k: torch.from_numpy(np.ascontiguousarray(v[:V] if k in ('points', 'normals', 'fallback') else v)).to(DEV) for k, v in inp.items()}
    out = H.mesh_bake(t['points'], t['normals'], t['images'], t['depth'], t['mask'], t['cams'], fallback=t['fallback'] if with_fallback else None, **kw)
    torch.cuda.synchronize()
    assert out['color'].shape == (V, 3) and out['rgb'].dtype == torch.uint8 and out['views'].shape == (V,)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref_bake(inp, V, with_fallback=True, **kw):
    return MR.bake(inp['points'][:V], inp['normals'][:V], inp['images'], inp['depth'], inp['mask'], inp['cams'],
                   fallback=inp['fallback'][:V] if with_fallback else None, **kw)


@pytest.mark.parametrize('HR', [(8, 8), (37, 16), (1, 1)])
@pytest.mark.parametrize('F', [1, 3])
def test_bake_equals_the_restatement(F, HR):
    """color, rgb, weight and views equal the restatement bit for bit for power 1, 2, 8, cos_min 0 and 0.1, depth_tol 0 and two voxels, at
    1000 vertices with and without a fallback and at the prefixes 1, 63, 64, 65 of the same (shuffled) vertices.  A case is one combination of
    the parameters at its 1000 vertices: at least a fifth of them are seen and at least a fifth are not (a prefix of one vertex cannot be
    both).  The special vertices are checked to be what they are meant to be with the restatement's own projection."""
    H, R = HR
    inp = bake_inputs(F, H, R)
    # the inputs contain what they should: exact pixel centres and frame edges of cam0 (r = 8 and 16: binary fractions), vertices just outside
    with np.errstate(all='ignore'):
        q, t, c2, xc, yc = MR.project(inp['cams'][0], inp['points'])
    assert (t == 0).sum() >= 1 and (c2 < 0).sum() >= 2 and np.isnan(inp['points']).any(1).sum() == 3
    assert (~inp['normals'].any(1)).sum() == 2 and np.isnan(inp['normals']).any()
    for r in sorted({H, R}):
        with np.errstate(all='ignore'):
            px, py = xc * np.float32(r) - np.float32(0.5), yc * np.float32(r) - np.float32(0.5)
            assert ((px == np.floor(px)) & (py == np.floor(py)) & (px >= 0) & (px <= r - 1) & (py >= 0) & (py <= r - 1)).sum() >= (64 if r == 8 else 1)
            if r != 37:                                                        # 0.5 / 37 is no binary fraction: its edge vertices are near the edge, not on it
                assert (px == 0).any() and (px == r - 1).any() and (py == 0).any() and (py == r - 1).any()
                assert ((px < 0) & (px > -1e-4)).any() and ((px > r - 1) & (px < r - 1 + 1e-4)).any()
    if F == 3:
        assert inp['cams'][1, 17] != 0 and inp['cams'][1, 18] != 0.5 and inp['cams'][1, 21] != 0.5
    cases = 0
    for power in (1, 2, 8):
        for cos_min in (0.0, 0.1):
            for tol in (0.0, TWO_VOXELS):
                kw = dict(depth_tol=tol, cos_min=cos_min, power=power)
                what = (F, H, R, power, cos_min, tol)
                for V in SIZES:
                    got, want = _gpu_bake(inp, V, **kw), _ref_bake(inp, V, **kw)
                    for k in ('views', 'weight', 'color', 'rgb'):
                        _assert_bits(got[k], want[k], what + (V, k))
                seen = got['views'] > 0
                assert seen.mean() >= 0.2 and (~seen).mean() >= 0.2, (what, seen.mean())
                assert int(got['views'].max()) <= F and (F == 1 or H == 1 or int(got['views'].max()) >= 2)      # a 1 x 1 frame: only cam0's axis is inside
                assert np.array_equal(_bits(got['color'][~seen]), _bits(inp['fallback'][~seen]))
                cases += 1
    assert cases == 12
    # without a fallback the unseen vertices are 0 (and grey 128); everything else as before
    kw = dict(depth_tol=TWO_VOXELS, cos_min=0.1, power=2)
    got, want, full = _gpu_bake(inp, 1000, with_fallback=False, **kw), _ref_bake(inp, 1000, with_fallback=False, **kw), _ref_bake(inp, 1000, **kw)
    for k in ('views', 'weight', 'color', 'rgb'):
        _assert_bits(got[k], want[k], (F, H, R, 'no fallback', k))
    seen = got['views'] > 0
    assert not got['color'][~seen].any() and (got['rgb'][~seen] == 128).all()
    assert np.array_equal(_bits(got['color'][seen]), _bits(full['color'][seen])) and np.array_equal(got['weight'], full['weight'])
    # a vertex seen only through masked-out depth pixels of cam0: visible to the same call with every pixel unmasked
    if F == 1 and R > 1:
        opened = dict(inp, mask=np.ones_like(inp['mask']), depth=np.full_like(inp['depth'], 10.0))
        more = _ref_bake(opened, 1000, **kw)['views'] > 0
        with np.errstate(all='ignore'):
            corner = (xc > 0.07) & (xc < 0.21) & (yc > 0.07) & (yc < 0.21)
        assert (corner & more & ~seen).sum() >= 30 and not (corner & seen).any()


def _raw_bake(t, V, outputs, **kw):
    """eg3d_mesh_bake through ctypes with only `outputs` bound"""
    from inv3d_amd import _lib as L
    out = dict(color=torch.full((V, 3), 7.0, device=DEV), rgb=torch.full((V, 3), 7, dtype=torch.uint8, device=DEV),
               weight=torch.full((V,), 7.0, device=DEV), views=torch.full((V,), 7, dtype=torch.uint8, device=DEV))
    p = L.MeshBakeParams(points=t['points'].data_ptr(), normals=t['normals'].data_ptr(), cams=t['cams'].data_ptr(), images=t['images'].data_ptr(),
                         depth=t['depth'].data_ptr(), mask=t['mask'].data_ptr(), fallback=t['fallback'].data_ptr(), V=V, F=t['cams'].shape[0],
                         H=t['images'].shape[2], R=t['depth'].shape[1], **kw)
    for k in outputs:
        setattr(p, k, out[k].data_ptr())
    L.check(L.lib().eg3d_mesh_bake(C.byref(p), L.stream_ptr()), 'mesh_bake')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_null_outputs_and_error_codes():
    """Each output alone gives the bytes of the full call and leaves the unbound buffers alone; no output at all is legal; every error code
    (tests/test_mesh_color_cpu.py's list, here where a launch would succeed); V = 0 through the wrappers."""
    from inv3d_amd import hipops as H
    inp = bake_inputs(3, 37, 16)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    kw = dict(depth_tol=TWO_VOXELS, cos_min=0.1, power=2)
    full = _raw_bake(t, 1000, ('color', 'rgb', 'weight', 'views'), **kw)
    want = _ref_bake(inp, 1000, **kw)
    for k in full:
        _assert_bits(full[k], want[k], k)
    for k in full:
        alone = _raw_bake(t, 1000, (k,), **kw)
        _assert_bits(alone[k], full[k], k)
        for other in full:
            if other != k:
                assert (alone[other] == 7).all(), (k, other)
    none = _raw_bake(t, 1000, (), **kw)
    assert all((v == 7).all() for v in none.values())
    _error_codes()
    e = H.mesh_bake(t['points'][:0], t['normals'][:0], t['images'], t['depth'], t['mask'], t['cams'], fallback=t['fallback'][:0], **kw)
    assert e['color'].shape == (0, 3) and e['rgb'].shape == (0, 3) and e['weight'].shape == (0,) and e['views'].shape == (0,)
    with pytest.raises(L_error()):
        H.mesh_bake(t['points'], t['normals'], t['images'], t['depth'], t['mask'], t['cams'], power=9)
    with pytest.raises(L_error()):
        H.mesh_bake(t['points'], t['normals'][:5], t['images'], t['depth'], t['mask'], t['cams'])
    with pytest.raises(L_error()):
        H.mesh_bake(t['points'], t['normals'], t['images'][:2], t['depth'], t['mask'], t['cams'])
    with pytest.raises(L_error()):
        H.mesh_bake(t['points'], t['normals'], t['images'], t['depth'], t['mask'].float(), t['cams'])


def L_error():
    from inv3d_amd._lib import Eg3dHipError
    return Eg3dHipError


def _digests(vol, frame, pts, inp, kw):
    """what tests/support/mesh_digest.py prints, from this process"""
    from inv3d_amd import hipops as H
    n = H.mesh_normals(torch.from_numpy(vol).to(DEV), torch.from_numpy(pts).to(DEV), **frame)
    b = _gpu_bake(inp, 1000, **kw)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()      # noqa: E731
    return dict(normals=sha(n.cpu().numpy()), **{k: sha(b[k]) for k in ('color', 'rgb', 'weight', 'views')})


def test_runs_and_builds_are_identical(tmp_path):
    """Two runs in one process give the same bytes, and so does the deterministic build in a fresh interpreter (the library is chosen at
    import; tests/support/mesh_digest.py): neither kernel accumulates across threads."""
    from inv3d_amd import _lib as L
    vol, frame = grids()['nan_and_padding']
    pts = normal_points(vol.shape, frame)
    inp = bake_inputs(3, 37, 16)
    kw = dict(depth_tol=TWO_VOXELS, cos_min=0.1, power=2)
    first, second = _digests(vol, frame, pts, inp, kw), _digests(vol, frame, pts, inp, kw)
    assert first == second
    if L.DETERMINISTIC:
        return
    path = str(tmp_path / 'inputs.npz')
    np.savez(path, vol=vol, pts=pts, origin=np.asarray(frame['origin']), spacing=np.asarray(frame['spacing']), axes=np.asarray(frame['axes']),
             depth_tol=kw['depth_tol'], cos_min=kw['cos_min'], power=kw['power'], **inp)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'mesh_digest.py'), path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == first


# ---- generator level ---------------------------------------------------------------------------------------------------------------------

RES = 48


@pytest.fixture(scope='module')
def small():
    """the small synthetic generator of tests/test_gpu_mesh.py, its 48^3 grid and the level at the 0.6 quantile of the unpadded densities"""
    from inv3d_amd import hipops as H, inference as INF, synthetic as S
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
    grid = INF.density_grid(G, ws, res=RES)
    level = float(torch.quantile(grid[grid > -999], 0.6))
    verts, faces = H.marching_cubes(grid, level)
    return dict(G=G, ws=ws, cam=cam, uni=uni, grid=grid, level=level, verts=verts, faces=faces)


def _tb(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_color_mesh_is_its_composition(small):
    """color_mesh == density_grid, marching_cubes, mesh_to_world, mesh_normals, G.synthesis per camera, iso_render and mesh_bake composed here
    by hand, bit for bit (pinned sampling draws); source='radiance' returns the fallback; extract_mesh(attributes=True)."""
    from inv3d_amd import hipops as H, inference as INF
    G, ws, grid, level, verts, faces, uni = (small[k] for k in ('G', 'ws', 'grid', 'level', 'verts', 'faces', 'uni'))
    V = verts.shape[0]
    assert V > 1000 and faces.shape[0] > 0
    cams = torch.cat([small['cam'], INF.bake_cameras(3, 2, device=DEV)])
    kw = dict(render_uniforms=uni, force_fp32=True)
    got = INF.color_mesh(G, ws, verts, RES, level=level, grid=grid, cameras=cams, **kw)
    # by hand
    origin, spacing, axes = INF.grid_frame(G, RES)
    world, wfaces = INF.mesh_to_world(G, verts, faces, RES)
    assert torch.equal(wfaces, faces)                                          # density_grid's frame does not mirror
    normals = H.mesh_normals(grid, world, origin, spacing, axes)
    planes = G.backbone.synthesis(ws[:1], noise_mode='const')
    planes = planes.view(1, 3, -1, planes.shape[-2], planes.shape[-1])
    fallback = (G.renderer.run_model(planes, G.decoder, world.unsqueeze(0), None, G.rendering_kwargs)['rgb'].reshape(V, -1)[:, :3].float() * 2 - 1).contiguous()
    images = torch.cat([G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image']
                        for i in range(cams.shape[0])]).float().contiguous()      # one backbone pass, as render_orbit
    iso = H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes)
    baked = H.mesh_bake(world, normals, images, iso['depth'], iso['mask'], cams, fallback=fallback, depth_tol=2 * abs(spacing[0]), cos_min=0.1, power=2)
    for k, want in (('world', world), ('world_normals', normals), ('normals', INF.normals_to_mesh(G, normals, RES)), ('color', baked['color']),
                    ('colors', baked['rgb']), ('views', baked['views'])):
        assert got[k].shape == want.shape and torch.equal(_tb(got[k]), _tb(want)), k
    seen = int((got['views'] > 0).sum())
    print(f'color_mesh: {V} vertices, {seen} coloured from views, {V - seen} from the fallback; views up to {int(got["views"].max())}')
    assert seen > 0
    lens = got['normals'].norm(dim=1)
    assert bool((((lens - 1).abs() < 1e-5) | (lens == 0)).all()) and int((lens > 0).sum()) > V // 2
    # the restatement on the same device inputs
    want = MR.bake(world.cpu().numpy(), normals.cpu().numpy(), images.cpu().numpy(), iso['depth'].cpu().numpy(), iso['mask'].cpu().numpy(),
                   cams.cpu().numpy(), fallback=fallback.cpu().numpy(), depth_tol=2 * abs(spacing[0]), cos_min=0.1, power=2)
    _assert_bits(got['color'].cpu().numpy(), want['color'], 'color vs restatement')
    _assert_bits(got['views'].cpu().numpy(), want['views'], 'views vs restatement')
    _assert_bits(got['world_normals'].cpu().numpy(), MR.normals(grid.cpu().numpy(), world.cpu().numpy(), origin, spacing, axes), 'normals vs restatement')
    # radiance
    rad = INF.color_mesh(G, ws, verts, RES, level=level, grid=grid, source='radiance', **kw)
    assert torch.equal(_tb(rad['color']), _tb(fallback)) and not bool(rad['views'].any())
    assert torch.equal(rad['colors'], (fallback * 127.5 + 128).clamp(0, 255).to(torch.uint8))
    assert torch.equal(_tb(rad['normals']), _tb(got['normals']))
    unseen = got['views'] == 0
    assert torch.equal(_tb(got['color'][unseen]), _tb(fallback[unseen]))
    # the grid built inside gives the same normals
    inner = INF.color_mesh(G, ws, verts, RES, level=level, source='radiance')
    assert torch.equal(_tb(inner['normals']), _tb(got['normals'])) and torch.equal(_tb(inner['color']), _tb(fallback))
    # extract_mesh
    pv, pf = INF.extract_mesh(G, ws, res=RES, level=level)
    av, af, an, ac = INF.extract_mesh(G, ws, res=RES, level=level, attributes=True)
    assert torch.equal(_tb(pv), _tb(verts)) and torch.equal(pf, faces) and torch.equal(_tb(av), _tb(pv)) and torch.equal(af, pf)
    assert an.shape == (V, 3) and an.dtype == torch.float32 and ac.shape == (V, 3) and ac.dtype == torch.uint8
    assert torch.equal(_tb(an), _tb(got['normals']))


def _read_ply(path, attributes):
    data = open(path, 'rb').read()
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode().splitlines()
    nv = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    nf = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith('property') and 'list' not in l]
    assert props == (['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue'] if attributes else ['x', 'y', 'z'])
    dt = np.dtype([('p', '<f4', (3,)), ('n', '<f4', (3,)), ('c', 'u1', (3,))] if attributes else [('p', '<f4', (3,))])
    v = np.frombuffer(body[:nv * dt.itemsize], dt)
    rec = np.frombuffer(body[nv * dt.itemsize:], np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    assert len(rec) == nf and np.all(rec['n'] == 3)
    return v, rec['i']


def test_coach_mesh_colors(tmp_path, small):
    """mesh_colors=True: the PLY has the x y z and faces of the uncoloured file, and normals and colours equal to color_mesh's on the tuned
    generator with the pivot camera in front of bake_cameras(); '.mrc' refuses the option.  The uncoloured file is written by a coach without
    the option from the SAME tuned generator and pivot: two optimisation runs of the default build differ in the last bits (its backward passes
    sum with float atomics), which would make a comparison between two runs a test of that, not of the writer."""
    from inv3d_amd import inference as INF
    from inv3d_amd.coach import InversionCoach
    G, ws, cam, uni, level = (small[k] for k in ('G', 'ws', 'cam', 'uni', 'level'))
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        target = G.synthesis(ws, cam, noise_mode='const', force_fp32=True, render_uniforms=uni)['image'].clamp(-1, 1)
    kw = dict(first_inv_steps=2, max_pti_steps=2, lpips_threshold=0.0, seed=3, w_avg_samples=0, keep_tuned_state=True, synth_kwargs=dict(render_uniforms=uni),
              gen_mesh=True, mesh_res=RES, mesh_level=level, mesh_format='.ply')
    try:
        with pytest.raises(ValueError):
            InversionCoach(G, **dict(kw, mesh_format='.mrc', mesh_dir=str(tmp_path / 'x'), mesh_colors=True))
        r1 = InversionCoach(G, mesh_dir=str(tmp_path / 'colour'), mesh_colors=True, **kw).invert('a', target, cam)
        assert r1.mesh_path == os.path.join(str(tmp_path / 'colour'), 'a_pti.ply')
        G.load_state_dict(r1.tuned_state)
        for p in G.parameters():
            p.requires_grad_(False)
        assert not all(torch.equal(pristine[k], v) for k, v in r1.tuned_state.items())          # it is the tuned generator's mesh
        plain = InversionCoach(G, mesh_dir=str(tmp_path / 'plain'), **kw).write_mesh('a', r1.w_pivot, r1.cam)
        v0, f0 = _read_ply(plain, False)
        v1, f1 = _read_ply(r1.mesh_path, True)
        assert len(f0) > 0 and np.array_equal(_bits(v0['p']), _bits(v1['p'])) and np.array_equal(f0, f1)
        verts, faces = INF.extract_mesh(G, r1.w_pivot, res=RES, level=level)
        assert np.array_equal(_bits(verts.cpu().numpy()), _bits(v1['p'])) and np.array_equal(faces.cpu().numpy(), f1)
        views = InversionCoach.mesh_cameras(r1.cam)
        assert views.shape == (16, 25) and torch.equal(views[0], r1.cam[0].float().cpu())
        att = INF.color_mesh(G, r1.w_pivot, verts, RES, level=level, cameras=views, render_uniforms=uni)
        assert att['views'].shape[0] == len(v1)
        assert np.array_equal(v1['c'], att['colors'].cpu().numpy())
        assert np.array_equal(_bits(v1['n']), _bits(att['normals'].cpu().numpy()))
    finally:
        G.load_state_dict(pristine)
        for p in G.parameters():
            p.requires_grad_(False)
