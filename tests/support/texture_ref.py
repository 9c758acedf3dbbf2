"""numpy restatement of the mesh-texture kernel (csrc/mesh_bake.hip mesh_texture_kernel; the specification is the comment of
include/eg3d_hip.h "Mesh texture"): the atlas layout, the corner rotation, the per-texel interpolation, the uv and the fill, operation for
operation in the order the header states.  The interpolated points go to mesh_ref.bake for the view loop, so the loop is restated once.  In
float32 (the default) tests/test_gpu_mesh_texture.py requires the GPU outputs to equal these bit for bit."""
import math

import numpy as np

import mesh_ref as MR


def size(F, T):
    """(Ht, Wt, per_row): two faces per T x T block, ceil(sqrt(blocks)) blocks per row, in integers"""
    nb = max((F + 1) // 2, 1)
    per_row = math.isqrt(nb)
    if per_row * per_row < nb:
        per_row += 1
    return T * ((nb + per_row - 1) // per_row), T * per_row, per_row


def owners(F, T):
    """int64 [Ht,Wt]: the face that owns every texel, -1 where none does (the fill)"""
    Ht, Wt, per_row = size(F, T)
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing='ij')
    blk = (y // T) * per_row + x // T
    f = 2 * blk + ((x % T + y % T) >= T)
    return np.where(f < F, f, -1)


def rotation(points, faces):
    """uint8 [F]: the corner opposite the longest edge (the first among equals; a NaN length never wins); 0 for a face with a bad index"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(p))).all(1)
    v = p[np.where(ok[:, None], f, 0)] if len(p) else np.zeros((len(f), 3, 3), np.float32)
    with np.errstate(all='ignore'):
        e = []
        for a, b in ((2, 1), (0, 2), (1, 0)):              # e_k: the edge opposite corner k
            d = v[:, a] - v[:, b]
            e.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        r = np.zeros(len(f), np.int64)
        er = e[0].copy()
        for k in (1, 2):
            win = e[k] > er
            r = np.where(win, k, r)
            er = np.where(win, e[k], er)
    return np.where(ok, r, 0).astype(np.uint8), ok


def corners(T, upper):
    """block-local texel centres of A_0, A_1, A_2"""
    return ((T - 1, T - 1), (2, T - 1), (T - 1, 2)) if upper else ((0, 0), (T - 2, 0), (0, T - 2))


def uv(F, T, r):
    """fp32 [F,3,2] in the faces' original corner order, origin top-left"""
    Ht, Wt, per_row = size(F, T)
    out = np.zeros((F, 3, 2), np.float32)
    for f in range(F):
        blk = f // 2
        x0, y0 = (blk % per_row) * T, (blk // per_row) * T
        c = corners(T, f % 2 == 1)
        for k in range(3):
            lx, ly = c[(k - int(r[f])) % 3]
            out[f, k, 0] = (np.float32(x0 + lx) + np.float32(0.5)) / np.float32(Wt)
            out[f, k, 1] = (np.float32(y0 + ly) + np.float32(0.5)) / np.float32(Ht)
    return out


def _mix(b0, b1, b2, a0, a1, a2):
    return (b0[:, None] * a0 + b1[:, None] * a1) + b2[:, None] * a2


def texels(points, normals_, faces, T, fallback=None):
    """Per owned texel of a face with good indices: dict(y, x, face, point [n,3], normal [n,3], fallback [n,3] | None, b [n,3]) in fp32"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = np.asarray(normals_, dtype=np.float32).reshape(-1, 3)
    fb = None if fallback is None else np.asarray(fallback, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(f)
    r, ok = rotation(p, f)
    own = owners(F, T)
    live = (own >= 0) & ok[np.maximum(own, 0)]
    y, x = np.nonzero(live)
    face = own[y, x]
    i, j = x % T, y % T
    upper = face % 2 == 1
    ii, jj, leg = np.where(upper, T - 1 - i, i), np.where(upper, T - 1 - j, j), np.where(upper, T - 3, T - 2)
    one = np.float32(1)
    with np.errstate(all='ignore'):
        b1 = ii.astype(np.float32) / leg.astype(np.float32)
        b2 = jj.astype(np.float32) / leg.astype(np.float32)
        b0 = (one - b1) - b2
        rr = r[face].astype(np.int64)
        idx = [f[face, (rr + s) % 3] for s in range(3)]    # A_0, A_1, A_2: cyclic from corner r
        mix = lambda a: _mix(b0, b1, b2, a[idx[0]], a[idx[1]], a[idx[2]])      # noqa: E731
        return dict(y=y, x=x, face=face, point=mix(p), normal=mix(n), fallback=None if fb is None else mix(fb), b=np.stack([b0, b1, b2], 1),
                    r=r, ok=ok)


def texture(points, normals_, faces, images, depth, mask, cams, fallback=None, tile=8, fill=128, depth_tol=0.0, cos_min=0.1, power=2):
    """dict(texture uint8 [Ht,Wt,3], views uint8 [Ht,Wt], uv fp32 [F,3,2], corner uint8 [F], bad_faces int) exactly as the kernel writes them"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F, T = len(f), int(tile)
    Ht, Wt, _ = size(F, T)
    t = texels(points, normals_, f, T, fallback)
    tex = np.full((Ht, Wt, 3), fill, np.uint8)
    views = np.zeros((Ht, Wt), np.uint8)
    if len(t['y']):
        baked = MR.bake(t['point'], t['normal'], images, depth, mask, cams, fallback=t['fallback'], depth_tol=depth_tol, cos_min=cos_min, power=power)
        tex[t['y'], t['x']] = baked['rgb']
        views[t['y'], t['x']] = baked['views']
    return dict(texture=tex, views=views, uv=uv(F, T, t['r']), corner=t['r'], bad_faces=int((~t['ok']).sum()))


def lookup(tex, u, v):
    """lookup_px at the uv coordinates (origin top-left, texel centres at ((x + 0.5) / Wt, (y + 0.5) / Ht))"""
    Ht, Wt = tex.shape[:2]
    return lookup_px(tex, np.asarray(u, np.float64) * Wt - 0.5, np.asarray(v, np.float64) * Ht - 0.5)


def lookup_px(tex, px, py):
    """Bilinear lookup of a [Ht,Wt,C] array at texel-centre coordinates (px, py) in float64, with the four taps: (value [n,C], list of
    (y, x, weight) arrays -- a tap outside the atlas is reported where it lies and read clamped)."""
    Ht, Wt = tex.shape[:2]
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    tx, ty = px - x0, py - y0
    val, taps = 0.0, []
    for dy, wy in ((0, 1 - ty), (1, ty)):
        for dx, wx in ((0, 1 - tx), (1, tx)):
            w = wy * wx
            yy, xx = np.clip(y0 + dy, 0, Ht - 1), np.clip(x0 + dx, 0, Wt - 1)
            val = val + w[:, None] * tex[yy, xx].astype(np.float64)
            taps.append((y0 + dy, x0 + dx, w))
    return val, taps
