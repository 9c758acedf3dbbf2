"""Textured meshes without a GPU: the atlas layout of include/eg3d_hip.h "Mesh texture" as tests/support/texture_ref.py restates it (what
tests/test_gpu_mesh_texture.py requires the GPU outputs to equal bit for bit) checked for the properties the layout promises -- sizes, one
owner per texel, bilinear lookups that never leave a face's texels, the corner rotation on planted faces -- a planted sphere on which the
texture beats vertex colours, and the host side: the parameter structure against the header, every error code, write_obj, the coach's
argument checks."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import mesh_ref as MR  # noqa: E402
import texture_ref as TR  # noqa: E402
from test_mesh_color_cpu import camera, ray_spheres  # noqa: E402
from inv3d_amd import inference as I  # noqa: E402

TILES = (4, 5, 8, 16)
COUNTS = (0, 1, 2, 3, 8, 9, 18, 19)                      # 8, 9, 18, 19 faces: 4, 5, 9, 10 blocks -- a full square of blocks and one more


# ---- the layout --------------------------------------------------------------------------------------------------------------------------

def test_texture_size():
    """hipops.mesh_texture_size, eg3d_mesh_texture_size and the restatement agree, on values worked out by hand for tile 8."""
    from inv3d_amd import _lib as L, hipops as H
    lib = L.lib()
    by_hand = {0: (8, 8), 1: (8, 8), 2: (8, 8), 3: (8, 16), 8: (16, 16), 9: (16, 24), 18: (24, 24), 19: (24, 32)}      # (Ht, Wt) at T = 8
    for F in COUNTS:
        for T in TILES:
            want = TR.size(F, T)[:2]
            assert H.mesh_texture_size(F, T) == want
            ht, wt = C.c_int32(-1), C.c_int32(-1)
            assert lib.eg3d_mesh_texture_size(F, T, C.byref(ht), C.byref(wt)) == 0 and (ht.value, wt.value) == want
            assert want[0] % T == 0 and want[1] % T == 0 and (want[0] // T) * (want[1] // T) >= max((F + 1) // 2, 1)
            assert (want[0] // T - 1) * (want[1] // T) < max((F + 1) // 2, 1)                    # no empty row of blocks
        assert H.mesh_texture_size(F, 8) == by_hand[F]
    assert H.mesh_texture_size(7) == H.mesh_texture_size(7, 8)
    # the largest atlas and the first that is too large: 2048^2 blocks of 8 texels, two faces each
    assert H.mesh_texture_size(2 * 2048 * 2048, 8) == (16384, 16384)
    with pytest.raises(L.Eg3dHipError, match='simplify'):
        H.mesh_texture_size(2 * 2048 * 2048 + 1, 8)
    for bad in ((-1, 8), (4, 3), (4, 65)):
        with pytest.raises(ValueError):
            H.mesh_texture_size(*bad)


@pytest.mark.parametrize('T', TILES)
def test_every_texel_has_one_owner_or_is_fill(T):
    """Painted face by face from the ownership rule (block-local loops, not the restatement's vectorised form): no texel is painted twice,
    the even face of a block has T (T + 1) / 2 texels, the odd one T (T - 1) / 2, and what is left is what the restatement calls fill."""
    for F in COUNTS:
        Ht, Wt, per_row = TR.size(F, T)
        count, who = np.zeros((Ht, Wt), np.int64), np.full((Ht, Wt), -1, np.int64)
        for f in range(F):
            b, n = f // 2, 0
            for j in range(T):
                for i in range(T):
                    if (i + j >= T) if f % 2 else (i + j <= T - 1):
                        y, x = (b // per_row) * T + j, (b % per_row) * T + i
                        count[y, x] += 1
                        who[y, x] = f
                        n += 1
            assert n == (T * (T - 1) // 2 if f % 2 else T * (T + 1) // 2)
        assert count.max(initial=0) <= 1
        own = TR.owners(F, T)
        assert own.shape == (Ht, Wt) and np.array_equal(own, who)
        assert (own < 0).sum() == Ht * Wt - sum(T * (T - 1) // 2 if f % 2 else T * (T + 1) // 2 for f in range(F))
        if F == 0:
            assert (Ht, Wt) == (T, T) and (own < 0).all()


def _triangle_points(c, rng, n):
    """float64 points of the triangle with the integer corners c (right angle first, legs along the axes): n strictly inside or on it by
    rejection, then the three corners, and points at multiples of 1 / 64 of every edge -- all exactly representable, so 'on the edge' is exact."""
    (ax, ay), (bx, by), (cx, cy) = c
    leg = abs(bx - ax)
    sx, sy = np.sign(bx - ax), np.sign(cy - ay)
    s, t = rng.uniform(0, leg, 4 * n), rng.uniform(0, leg, 4 * n)
    keep = s + t <= leg
    px, py = [ax + sx * s[keep][:n]], [ay + sy * t[keep][:n]]
    e = np.arange(65) / 64.0 * leg
    px += [ax + sx * e, ax + 0 * e, ax + sx * e]           # the leg along x, the leg along y, the hypotenuse
    py += [ay + 0 * e, ay + sy * e, ay + sy * (leg - e)]
    return np.concatenate(px), np.concatenate(py)


@pytest.mark.parametrize('T', TILES)
def test_bilinear_lookups_stay_inside_the_face(T):
    """For every face of a 19-face atlas (10 blocks: a last block with one face, neighbours on every side of some block): bilinear lookups
    at random points of the face's texel triangle, at its corners and along its edges give non-zero weight only to texels inside the atlas
    that the face owns -- nothing bleeds across the diagonal or into a neighbouring block, so no gutter is needed at this mip level.  The
    lookups run in exact texel-centre coordinates; the fp32 uv of the corners are within 1e-3 texel of them."""
    F = 19
    Ht, Wt, per_row = TR.size(F, T)
    own = TR.owners(F, T)
    rng = np.random.RandomState(T)
    r = rng.randint(0, 3, F).astype(np.uint8)
    uv = TR.uv(F, T, r)
    marker = np.zeros((Ht, Wt, 1))
    touched = 0
    for f in range(F):
        b = f // 2
        x0, y0 = (b % per_row) * T, (b // per_row) * T
        c = [(x0 + lx, y0 + ly) for lx, ly in TR.corners(T, f % 2 == 1)]
        for k in range(3):                                                   # corner k of the face sits at triangle corner (k - r) % 3
            ex, ey = c[(k - int(r[f])) % 3]
            assert abs(float(uv[f, k, 0]) * Wt - 0.5 - ex) < 1e-3 and abs(float(uv[f, k, 1]) * Ht - 0.5 - ey) < 1e-3
            assert 0.0 < uv[f, k, 0] < 1.0 and 0.0 < uv[f, k, 1] < 1.0
        px, py = _triangle_points(c, rng, 300)
        assert len(px) >= 300 + 3 * 65
        _, taps = TR.lookup_px(marker, px, py)
        total = 0.0
        for yy, xx, w in taps:
            hit = w > 0
            assert (yy[hit] >= 0).all() and (yy[hit] < Ht).all() and (xx[hit] >= 0).all() and (xx[hit] < Wt).all(), (T, f)
            assert (own[yy[hit], xx[hit]] == f).all(), (T, f)
            touched += int(hit.sum())
            total = total + w
        assert np.abs(total - 1).max() < 1e-12
        # the face's texels that a lookup can reach cover its triangle: the three corner texels are among them
        for ex, ey in c:
            assert own[ey, ex] == f
    assert touched > F * 300


def test_corner_rotation_on_planted_faces():
    """The corner opposite the longest edge takes the right angle; ties keep the lower corner; a NaN length never wins; a zero-area face and
    a repeated index are ordinary faces; a face with an index outside [0, V) gets 0 and is reported."""
    nan = np.nan
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 1], [nan, 0, 0], [2, 0, 0], [4, 0, 0]], np.float32)
    cases = [((0, 1, 2), 0),       # e_0 = |v_2 - v_1|^2 = 5, e_1 = |v_0 - v_2|^2 = 4, e_2 = |v_1 - v_0|^2 = 1
             ((1, 2, 0), 2),       # the same triangle rotated: the vertex at the origin is now corner 2
             ((2, 0, 1), 1),
             ((1, 0, 3), 1),       # e = 9, 10, 1
             ((0, 1, 4), 1),       # e = 2, 3, 1
             ((0, 4, 1), 2),       # the other winding of the same vertices: e = 2, 1, 3
             ((4, 4, 4), 0),       # a point: every length 0, the first of the ties
             ((0, 0, 1), 0),       # a repeated index: e = 1, 1, 0 -- the first of the tie
             ((1, 0, 0), 1),       # e = 0, 1, 1 -- the first of that tie
             ((0, 1, 6), 1),       # collinear (zero area): e = 1, 4, 1
             ((0, 6, 7), 1),       # collinear: e = 4, 16, 4
             ((5, 0, 1), 0),       # a NaN vertex at corner 0: e_0 = 1 is the only comparable length
             ((0, 5, 1), 0),       # a NaN e_0 is never replaced: every comparison with it is false
             ((0, 1, 5), 0)]
    faces = np.array([c[0] for c in cases], np.int64)
    r, ok = TR.rotation(P, faces)
    assert ok.all() and r.dtype == np.uint8
    assert r.tolist() == [c[1] for c in cases]
    # rotating a face's indices rotates the answer with it (distinct lengths): the same vertex takes the right angle
    for f, want in (((0, 1, 2), 0), ((1, 0, 3), 1)):
        vert = f[want]
        for s in range(3):
            g = tuple(f[(k + s) % 3] for k in range(3))
            assert g[int(TR.rotation(P, np.array([g]))[0][0])] == vert
    bad = np.array([[0, 1, 2], [0, 8, 1], [-1, 0, 1], [0, 1, 7]], np.int64)
    r, ok = TR.rotation(P, bad)
    assert ok.tolist() == [True, False, False, True] and r[1] == 0 and r[2] == 0
    # the uv triangle keeps the winding whatever the rotation: the signed area of (uv0, uv1, uv2) has one sign for every face and every r
    for T in TILES:
        for rr in range(3):
            uv = TR.uv(6, T, np.full(6, rr, np.uint8)).astype(np.float64)
            a, b = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
            assert (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] > 0).all()


def test_corner_texels_are_their_vertices_and_the_rest_is_fill():
    """The restated per-texel inputs: at the three triangle corners of a face with finite vertices the barycentrics are a unit vector and
    the interpolated point is the vertex bit for bit; the owned texels beyond the hypotenuse extrapolate (b_0 < 0); texels nobody owns and the
    texels of a face with a bad index do not appear."""
    rng = np.random.RandomState(5)
    P = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    Nn = rng.normal(size=(40, 3)).astype(np.float32)
    faces = rng.randint(0, 40, (9, 3))
    faces[3] = (1, 40, 2)                                                     # out of range: its texels stay fill
    for T in TILES:
        t = TR.texels(P, Nn, faces, T)
        Ht, Wt, per_row = TR.size(9, T)
        assert not (t['face'] == 3).any() and not t['ok'][3] and t['ok'].sum() == 8
        n_owned = sum(T * (T - 1) // 2 if f % 2 else T * (T + 1) // 2 for f in range(9) if f != 3)
        assert len(t['y']) == n_owned
        assert (t['b'][:, 0] < -0.01).sum() == sum((T - 1) if f % 2 else T for f in range(9) if f != 3)      # one diagonal of texels per face
        for f in range(9):
            if f == 3:
                continue
            b = f // 2
            x0, y0 = (b % per_row) * T, (b // per_row) * T
            for s, (lx, ly) in enumerate(TR.corners(T, f % 2 == 1)):
                at = np.nonzero((t['y'] == y0 + ly) & (t['x'] == x0 + lx))[0]
                assert len(at) == 1 and t['face'][at[0]] == f
                want = np.zeros(3, np.float32)
                want[s] = 1
                assert np.array_equal(t['b'][at[0]], want)
                v = faces[f, (int(t['r'][f]) + s) % 3]
                assert np.array_equal(t['point'][at[0]].view(np.uint32), (P[v] + np.float32(0)).view(np.uint32))
                assert np.array_equal(t['normal'][at[0]].view(np.uint32), (Nn[v] + np.float32(0)).view(np.uint32))


# ---- the point of the feature -----------------------------------------------------------------------------------------------------------

R0 = 0.3


def _octasphere(levels):
    """an octahedron subdivided `levels` times and pushed onto the sphere of radius R0: (verts fp32 [V,3], faces [F,3] wound outward)"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.asarray(p, dtype=np.float64) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return (R0 * np.asarray(v)).astype(np.float32), np.asarray(f, dtype=np.int64)


def pattern(p):
    """a smooth colour in [-1, 1] of a world point with a wavelength (0.16) close to a face's edge (0.12): several image pixels per period"""
    return np.stack([0.8 * np.sin(40.0 * p[..., 0] + 0.5), 0.8 * np.cos(36.0 * p[..., 1] - 0.3), 0.8 * np.sin(38.0 * p[..., 2] + 1.0)], -1)


def test_texture_keeps_detail_that_vertex_colours_lose():
    """A 128-face sphere (edges of 0.12 world units, 19 pixels of a 128^2 view) under a pattern of wavelength 0.16, three views from float64
    ray-sphere intersection.  At 4000 random points of the mesh surface the colour of a direct bake of the point (the restatement's) is
    compared with (a) a bilinear lookup in the restated 16-texel atlas at the point's uv and (b) barycentric interpolation of the baked
    vertex colours, over the points where all three are coloured from views.  The texture's error is the smaller one; the ratio is reported
    (DESIGN.md 3.4 records it), no threshold is fixed for it."""
    verts, faces = _octasphere(2)
    assert faces.shape == (128, 3)
    normals = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(np.float32)
    tri = verts.astype(np.float64)[faces]
    assert (np.einsum('ij,ij->i', np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), tri.mean(1)) > 0).all()      # wound outward
    cams = np.stack([camera(yaw=math.pi / 2 + dy, pitch=math.pi / 2 + dp, focal=3.4) for dy, dp in ((0.0, 0.0), (0.7, 0.1), (-0.6, -0.2))])
    ball = [((0., 0., 0.), R0)]
    _, _, pts = ray_spheres(cams, 128, ball)
    images = np.ascontiguousarray(pattern(pts).transpose(0, 3, 1, 2)).astype(np.float32)
    depth, mask, _ = ray_spheres(cams, 64, ball)
    kw = dict(depth_tol=0.03, cos_min=0.3, power=2)                          # the chords lie up to 0.006 inside the sphere the depth maps show
    T = 16
    tex = TR.texture(verts, normals, faces, images, depth, mask, cams, tile=T, **kw)
    vert = MR.bake(verts, normals, images, depth, mask, cams, **kw)
    rng = np.random.RandomState(0)
    n = 4000
    face = rng.randint(0, len(faces), n)
    b = rng.dirichlet((1, 1, 1), n)
    mixd = lambda a: np.einsum('nk,nkc->nc', b, a.astype(np.float64)[faces[face]])      # noqa: E731
    direct = MR.bake(mixd(verts).astype(np.float32), mixd(normals).astype(np.float32), images, depth, mask, cams, **kw)
    uv = np.einsum('nk,nkc->nc', b, tex['uv'].astype(np.float64)[face])
    colour = (tex['texture'].astype(np.float64) + 0.5 - 128) / 127.5       # the centre of the truncation interval
    got_tex, taps = TR.lookup(colour, uv[:, 0], uv[:, 1])
    seen_tex = np.ones(n, bool)
    for yy, xx, w in taps:
        seen_tex &= (w == 0) | (tex['views'][np.clip(yy, 0, colour.shape[0] - 1), np.clip(xx, 0, colour.shape[1] - 1)] > 0)
    got_vert = mixd(vert['color'])
    use = (direct['views'] > 0) & seen_tex & (vert['views'][faces[face]] > 0).all(1)
    assert use.sum() >= n // 4, use.sum()
    want = direct['color'].astype(np.float64)[use]
    rms = lambda d: float(np.sqrt((d * d).mean()))      # noqa: E731
    e_tex, e_vert = rms(got_tex[use] - want), rms(got_vert[use] - want)
    print(f'planted sphere: {use.sum()} points; rms error texture {e_tex:.4f}, vertex colours {e_vert:.4f}, ratio {e_vert / e_tex:.1f}')
    assert e_tex < e_vert


# ---- host side ---------------------------------------------------------------------------------------------------------------------------

def test_structure_matches_the_header():
    """eg3d_mesh_texture_params of inv3d_amd/_lib.py against its C definition (gcc), as test_host.py does."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    cname, cls = 'eg3d_mesh_texture_params', L.MeshTextureParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', f' printf("%zu\\n", sizeof({cname}));']
    want = [C.sizeof(cls)]
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


def test_entry_rejects_bad_arguments_before_any_launch():
    """Every error code of eg3d_mesh_texture and eg3d_mesh_texture_size, answered from the arguments alone (no GPU here: a launch would be an
    error of its own); with no output bound the call is a normal result with no launch.  tests/test_gpu_mesh_texture.py runs this again
    where a launch would succeed."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    OK, INVALID, UNSUPPORTED, TOO_LARGE = 0, -1, -2, -3
    a = 0x1000                                                                  # a non-null pointer that is never dereferenced
    nan, inf = float('nan'), float('inf')

    def tex(**kw):
        p = L.MeshTextureParams(**dict(dict(points=a, normals=a, faces=a, cams=a, images=a, depth=a, mask=a, fallback=a, V=10, F=7, N=3, H=8, R=8, tile=8,
                                            fill=128, depth_tol=0.01, cos_min=0.1, power=2), **kw))
        return lib.eg3d_mesh_texture(C.byref(p), None)
    assert lib.eg3d_mesh_texture(None, None) == INVALID
    assert tex() == OK and tex(fallback=None) == OK and tex(V=0, points=None, normals=None) == OK and tex(F=0, faces=None) == OK
    assert tex(tile=4) == OK and tex(tile=64) == OK and tex(fill=0) == OK and tex(fill=255) == OK
    for bad in (dict(cams=None), dict(images=None), dict(depth=None), dict(mask=None), dict(points=None), dict(normals=None), dict(faces=None), dict(V=-1),
                dict(F=-1), dict(N=0), dict(H=0), dict(R=0), dict(depth_tol=-0.5), dict(depth_tol=nan), dict(depth_tol=inf), dict(cos_min=-0.1),
                dict(cos_min=1.0), dict(cos_min=nan), dict(power=0), dict(power=9), dict(tile=3), dict(tile=65), dict(tile=0), dict(fill=-1), dict(fill=256)):
        assert tex(**bad) == INVALID, bad
    for bad in (dict(N=256), dict(H=16385), dict(R=16385), dict(F=2 * 2048 * 2048 + 1), dict(F=2 * 256 * 256 + 1, tile=64), dict(F=2 ** 31 - 1, tile=4)):
        assert tex(**bad) == UNSUPPORTED, bad
    assert tex(F=2 * 2048 * 2048) == OK and tex(F=2 * 256 * 256, tile=64) == OK
    assert tex(V=2 ** 31) == TOO_LARGE and tex(F=2 ** 31) == TOO_LARGE
    ht, wt = C.c_int32(0), C.c_int32(0)
    size = lambda F, T, h=C.byref(ht), w=C.byref(wt): lib.eg3d_mesh_texture_size(F, T, h, w)      # noqa: E731
    assert size(0, 8) == OK and (ht.value, wt.value) == (8, 8)
    assert size(-1, 8) == INVALID and size(4, 3) == INVALID and size(4, 65) == INVALID and size(4, 8, None) == INVALID and size(4, 8, C.byref(ht), None) == INVALID
    assert size(2 ** 31, 8) == TOO_LARGE and size(2 * 2048 * 2048 + 1, 8) == UNSUPPORTED and size(2 * 2048 * 2048, 8) == OK


def _parse_obj(path):
    out = dict(v=[], vn=[], vt=[], f=[], mtllib=[], usemtl=[])
    for line in open(path).read().splitlines():
        w = line.split()
        if not w or w[0].startswith('#'):
            continue
        assert w[0] in out, line
        if w[0] in ('v', 'vn', 'vt'):
            out[w[0]].append([float(x) for x in w[1:]])
        elif w[0] == 'f':
            out['f'].append([[int(x) for x in c.split('/')] for c in w[1:]])
        else:
            out[w[0]].append(w[1])
    return out


@pytest.mark.parametrize('with_normals', [True, False])
def test_write_obj_round_trips(tmp_path, with_normals):
    """Through a small OBJ parser: counts, indices in range, the vertices and normals bit for bit, vt = (u, 1 - v) inside [0, 1], the MTL names
    the image, and the PNG decodes with Pillow to the atlas bytes."""
    from PIL import Image
    rng = np.random.RandomState(2)
    V, F, T = 11, 7, 5
    verts, normals = rng.normal(size=(V, 3)).astype(np.float32), rng.normal(size=(V, 3)).astype(np.float32)
    faces = rng.randint(0, V, (F, 3)).astype(np.int32)
    Ht, Wt, _ = TR.size(F, T)
    uv = TR.uv(F, T, rng.randint(0, 3, F).astype(np.uint8))
    atlas = rng.randint(0, 256, (Ht, Wt, 3)).astype(np.uint8)
    path = str(tmp_path / 'head_pti.obj')
    got = I.write_obj(path, torch.from_numpy(verts), faces, torch.from_numpy(uv), torch.from_numpy(atlas), normals=normals if with_normals else None)
    assert got == (path, str(tmp_path / 'head_pti.mtl'), str(tmp_path / 'head_pti.png'))
    assert sorted(os.listdir(tmp_path)) == ['head_pti.mtl', 'head_pti.obj', 'head_pti.png']
    o = _parse_obj(path)
    assert o['mtllib'] == ['head_pti.mtl'] and o['usemtl'] == ['head_pti']
    assert len(o['v']) == V and len(o['vt']) == 3 * F and len(o['f']) == F and len(o['vn']) == (V if with_normals else 0)
    assert np.array_equal(np.asarray(o['v'], np.float32).view(np.uint32), verts.view(np.uint32))
    if with_normals:
        assert np.array_equal(np.asarray(o['vn'], np.float32).view(np.uint32), normals.view(np.uint32))
    vt = np.asarray(o['vt'], np.float64)
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    assert np.array_equal(vt[:, 0].astype(np.float32), uv.reshape(-1, 2)[:, 0]) and np.abs(vt[:, 1] - (1.0 - uv.reshape(-1, 2)[:, 1].astype(np.float64))).max() < 1e-8
    fi = np.asarray(o['f'])
    assert fi.shape == (F, 3, 3 if with_normals else 2)
    assert np.array_equal(fi[:, :, 0] - 1, faces) and np.array_equal(fi[:, :, 1] - 1, np.arange(3 * F).reshape(F, 3))
    if with_normals:
        assert np.array_equal(fi[:, :, 2], fi[:, :, 0])
    assert fi.min() >= 1 and fi[:, :, 0].max() <= V and fi[:, :, 1].max() <= 3 * F
    mtl = open(got[1]).read().split('\n')
    assert mtl[:3] == ['newmtl head_pti', 'Kd 1 1 1', 'map_Kd head_pti.png']
    assert np.array_equal(np.asarray(Image.open(got[2]).convert('RGB')), atlas)
    # the lookup a viewer does (v from the bottom) lands on the texel the uv names
    k = 3
    x, y = vt[k, 0] * Wt - 0.5, (1.0 - vt[k, 1]) * Ht - 0.5
    assert abs(x - round(x)) < 1e-3 and abs(y - round(y)) < 1e-3
    with pytest.raises(ValueError):
        I.write_obj(path, verts, faces, uv[:3], atlas)
    with pytest.raises(ValueError):
        I.write_obj(path, verts, faces, uv, atlas, normals=normals[:2])
    with pytest.raises(ValueError):
        I.write_obj(path, verts, faces + V, uv, atlas)
    with pytest.raises(ValueError):
        I.write_obj(path, verts, faces, uv, atlas, texture_format='bmp')
    with pytest.raises(ValueError):
        I.write_obj(path, verts, faces, uv, atlas.astype(np.float32))


def test_wrappers_and_options_refuse_bad_arguments():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.coach import InversionCoach
    z = torch.zeros
    with pytest.raises(Eg3dHipError):                                          # host tensors
        H.mesh_texture(z(5, 3), z(5, 3), z(2, 3, dtype=torch.int32), z(1, 3, 8, 8), z(1, 8, 8), z(1, 8, 8, dtype=torch.uint8), z(1, 25))
    base = dict(gen_mesh=True, mesh_dir='m', w_avg_samples=0)
    for bad in (dict(mesh_format='.stl'), dict(mesh_format='.obj', mesh_texture_tile=3), dict(mesh_format='.obj', mesh_texture_tile=65),
                dict(mesh_format='.ply', mesh_texture_tile=16), dict(mesh_format='.mrc', mesh_texture_tile=4), dict(mesh_format='.mrc', mesh_colors=True),
                dict(mesh_format='.mrc', mesh_simplify=2.0), dict(mesh_format='.obj', mesh_simplify=-1.0), dict(mesh_format='.obj', mesh_smooth=-1),
                dict(mesh_format='.obj', mesh_keep=-1), dict(mesh_format='.obj', mesh_dir=None)):
        with pytest.raises(ValueError):
            InversionCoach(None, **dict(base, **bad))
    G = torch.nn.Linear(1, 1)                                                  # a constructor that gets past the checks copies the state dict
    for mesh_colors in (False, True):                                          # '.obj' implies the colours and composes with the mesh options
        c = InversionCoach(G, mesh_format='.obj', mesh_colors=mesh_colors, mesh_texture_tile=16, mesh_keep=1, mesh_min_voxels=10, mesh_simplify=2.0,
                           mesh_smooth=3, **base)
        assert c.mesh_colors is True and c.mesh_texture_tile == 16 and c.mesh_format == '.obj' and c.mesh_simplify == 2.0 and c.mesh_smooth == 3
    assert InversionCoach(G, mesh_format='.ply', **base).mesh_colors is False
    with pytest.raises(ValueError):
        I.texture_mesh(None, None, z(0, 3), z(0, 3, dtype=torch.int32), 8, grid=z(4, 4, 4))


# ---- the GPU test's faces, checked here to make a case that is not vacuous -----------------------------------------------------------------

FACE_SEED = 0


def texture_faces(inp, seed=FACE_SEED, F=200):
    """F seeded faces over the 1000 vertices of test_gpu_mesh_color.bake_inputs.  A third join arbitrary vertices (faces across the whole
    box); a third join a vertex with two of its five nearest neighbours, so that they are small; a third join three of the vertices on cam0's
    optical axis (zero area; every texel of such a face lies on the axis exactly, the only points a 1 x 1 frame can see).  Planted near the
    front, so that every prefix of 9 or more has them all: face 1 repeats an index, face 2 has a NaN vertex; faces 4 - 8 use a vertex behind
    cam0, the vertex at its origin, and vertices exactly on / just outside the edge of its frame."""
    rng = np.random.RandomState(seed)
    pts = inp['points']
    faces = rng.randint(0, 1000, (F, 3))
    finite = np.nonzero(np.isfinite(pts).all(1))[0]
    axis = np.nonzero((pts[:, 0] == 0) & (pts[:, 1] == 0) & (np.abs(pts[:, 2]) <= 0.4) & (inp['normals'][:, 2] == 1))[0]
    assert len(axis) >= 300
    for f in range(F):
        if f % 3 == 1:
            a = finite[rng.randint(len(finite))]
            near = finite[np.argsort(((pts[finite] - pts[a]) ** 2).sum(1))[1:6]]
            faces[f] = (a, *rng.choice(near, 2, replace=False))
        elif f % 3 == 2:
            faces[f] = rng.choice(axis, 3, replace=False)
    with np.errstate(all='ignore'):
        q, t, c2, xc, yc = MR.project(inp['cams'][0], pts)
        px = xc * np.float32(8) - np.float32(0.5)
    nanv = np.nonzero(np.isnan(pts).any(1))[0]
    behind = np.nonzero(c2 < 0)[0]
    origin = np.nonzero(t == 0)[0]
    edge = np.nonzero((px == 0) | (px == 7))[0]
    outside = np.nonzero(((px < 0) & (px > -1e-4)) | ((px > 7) & (px < 7 + 1e-4)))[0]
    assert len(nanv) == 3 and len(behind) >= 2 and len(origin) >= 1 and len(edge) >= 2 and len(outside) >= 2
    faces[1] = (faces[1][0], faces[1][0], faces[1][2])
    planted = [(2, (faces[2][0], nanv[0], faces[2][2])), (4, (behind[0], faces[4][1], faces[4][2])), (5, (faces[5][0], origin[0], edge[0])),
               (6, (edge[0], edge[1], outside[0])), (7, (outside[1], faces[7][1], edge[1])), (8, (nanv[1], nanv[2], behind[1]))]
    for f, tri in planted:
        if f < F:
            faces[f] = tri
    return faces.astype(np.int32)


def test_the_gpu_case_is_not_vacuous():
    """The faces tests/test_gpu_mesh_texture.py bakes (FACE_SEED) on its inputs, through the restatement alone: at 200 faces at least a tenth
    of the owned texels are coloured from views and at least a tenth are not, at every tile size and input set it uses."""
    from test_gpu_mesh_color import TWO_VOXELS, bake_inputs
    for nviews, H, R in ((3, 8, 8), (3, 37, 16), (1, 8, 8), (1, 37, 16), (3, 1, 1), (1, 1, 1)):
        inp = bake_inputs(nviews, H, R)
        faces = texture_faces(inp)
        assert faces.shape == (200, 3) and faces[1][0] == faces[1][1] and np.isnan(inp['points'][faces[2]]).any()
        for T in (4, 8):
            out = TR.texture(inp['points'], inp['normals'], faces, inp['images'], inp['depth'], inp['mask'], inp['cams'], fallback=inp['fallback'],
                             tile=T, depth_tol=TWO_VOXELS, cos_min=0.1, power=2)
            owned = TR.owners(200, T) >= 0
            seen = (out['views'] > 0)[owned].mean()
            print(f'views {nviews}, H {H}, R {R}, tile {T}: {seen:.3f} of the owned texels coloured from views')
            assert out['bad_faces'] == 0 and seen >= 0.1 and 1 - seen >= 0.1, (nviews, H, R, T, seen)
