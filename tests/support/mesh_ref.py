"""numpy restatement of the mesh-attribute kernels (csrc/mesh_bake.hip; the specification is the comment of include/eg3d_hip.h "Mesh
attributes"): the normal of the density field at points and the view bake of vertex colours, operation for operation in the order the header
states, vectorised over vertices with a loop over the views.  In float32 (the default) tests/test_gpu_mesh_color.py requires the GPU outputs
to equal these bit for bit; with dtype=np.float64 the same algorithm runs in double precision.

Every scalar is wrapped in the working dtype before it meets an array, so nothing is promoted on the way.  The field (clamp, clamped lerp,
trilinear cell) is tests/support/iso_ref.py's: the header defines it once, under "Shape views"."""
import numpy as np

from iso_ref import _Grid, _clamp


def normals(vol, points, origin, spacing, axes=(0, 1, 2), dtype=np.float32):
    """[V,3]: unit normal toward lower values at the world points [V,3]; 0 where its length is 0 or not finite, and for a NaN point."""
    T = dtype
    g = _Grid(vol, T)
    x = np.asarray(points, dtype=np.float32).astype(T).reshape(-1, 3)
    org = [T(np.float32(v)) for v in origin]              # inputs arrive through the C structure as fp32 whatever the working precision
    sp = [T(np.float32(v)) for v in spacing]
    V = x.shape[0]
    n = np.zeros((V, 3), T)
    if V == 0:
        return n
    with np.errstate(all='ignore'):
        r = [(x[:, axes[a]] - org[a]) / sp[a] for a in range(3)]
        valid = (r[0] == r[0]) & (r[1] == r[1]) & (r[2] == r[2])
        p = [_clamp(r[a], g.h[a], T) for a in range(3)]
        for a in range(3):
            u, l = _clamp(p[a] + T(1), g.h[a], T), _clamp(p[a] - T(1), g.h[a], T)
            pu, pl = list(p), list(p)
            pu[a], pl[a] = u, l
            n[:, axes[a]] = -((g.field(pu) - g.field(pl)) / ((u - l) * sp[a]))
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = valid & (ln > T(0)) & (ln < T(np.inf))
        n = np.where(ok[:, None], n / ln[:, None], T(0))
    return n.astype(T)


def _lerp(a, b, f):
    return a + f * (b - a)


def project(cam, points, dtype=np.float32):
    """(t, c2, xc, yc) of one camera [25] for the points [V,3]: steps 1 and 2 of the bake up to the normalised image coordinates."""
    T = dtype
    m = np.asarray(cam, dtype=np.float32).astype(T)
    q = [points[:, i] - m[4 * i + 3] for i in range(3)]
    t = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    c = [(m[j] * q[0] + m[4 + j] * q[1]) + m[8 + j] * q[2] for j in range(3)]
    fx, sk, cx, fy, cy = m[16], m[17], m[18], m[20], m[21]
    xl, yl = c[0] / c[2], c[1] / c[2]
    yc = yl * fy + cy
    xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy
    return q, t, c[2], xc, yc


def bake(points, normals_, images, depth, mask, cams, fallback=None, depth_tol=0.0, cos_min=0.1, power=2, dtype=np.float32):
    """dict(color [V,3], rgb uint8 [V,3], weight [V], views uint8 [V]) exactly as the kernel writes them."""
    T = dtype
    p = np.asarray(points, dtype=np.float32).astype(T).reshape(-1, 3)
    n = np.asarray(normals_, dtype=np.float32).astype(T).reshape(-1, 3)
    img = np.asarray(images, dtype=np.float32).astype(T)
    dep = np.asarray(depth, dtype=np.float32).astype(T)
    msk = np.asarray(mask)
    cams = np.asarray(cams, dtype=np.float32)
    F, H, R, V = cams.shape[0], img.shape[2], dep.shape[1], p.shape[0]
    assert img.shape == (F, 3, H, H) and dep.shape == (F, R, R) and msk.shape == (F, R, R) and 1 <= power <= 8
    tol, cmin = T(np.float32(depth_tol)), T(np.float32(cos_min))
    acc, wsum, views = np.zeros((V, 3), T), np.zeros(V, T), np.zeros(V, np.int64)
    with np.errstate(all='ignore'):
        for f in range(F):
            q, t, c2, xc, yc = project(cams[f], p, T)
            live = (t > T(0)) & (c2 > T(0))
            pxH, pyH = xc * T(H) - T(0.5), yc * T(H) - T(0.5)
            pxR, pyR = xc * T(R) - T(0.5), yc * T(R) - T(0.5)
            for v, hi in ((pxH, T(H - 1)), (pyH, T(H - 1)), (pxR, T(R - 1)), (pyR, T(R - 1))):
                live &= (v >= T(0)) & (v <= hi)
            idx = np.nonzero(live)[0]
            if idx.size == 0:
                continue
            x0, y0 = np.floor(pxR[idx]).astype(np.int64), np.floor(pyR[idx]).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, R - 1), np.minimum(y0 + 1, R - 1)
            vis = np.zeros(idx.size, bool)
            for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
                vis |= (msk[f, yy, xx] != 0) & (t[idx] <= dep[f, yy, xx] + tol)
            idx = idx[vis]
            c = -((n[idx, 0] * q[0][idx] + n[idx, 1] * q[1][idx]) + n[idx, 2] * q[2][idx]) / t[idx]
            keep = c > cmin
            idx, c = idx[keep], c[keep]
            if idx.size == 0:
                continue
            w = c
            for _ in range(power - 1):
                w = w * c
            if H >= 2:
                bx, by = np.minimum(np.floor(pxH[idx]).astype(np.int64), H - 2), np.minimum(np.floor(pyH[idx]).astype(np.int64), H - 2)
                tx, ty = pxH[idx] - bx.astype(T), pyH[idx] - by.astype(T)
                col = [_lerp(_lerp(img[f, j, by, bx], img[f, j, by, bx + 1], tx), _lerp(img[f, j, by + 1, bx], img[f, j, by + 1, bx + 1], tx), ty)
                       for j in range(3)]
            else:
                col = [np.full(idx.size, img[f, j, 0, 0], T) for j in range(3)]
            for j in range(3):
                acc[idx, j] = acc[idx, j] + w * col[j]
            wsum[idx] = wsum[idx] + w
            views[idx] = np.minimum(views[idx] + 1, 255)
        fb = np.zeros((V, 3), T) if fallback is None else np.asarray(fallback, dtype=np.float32).astype(T).reshape(-1, 3)
        seen = wsum > T(0)
        color = np.where(seen[:, None], acc / np.where(seen, wsum, T(1))[:, None], fb).astype(T)
        rgb = np.fmin(np.fmax(color * T(127.5) + T(128), T(0)), T(255)).astype(np.int32).astype(np.uint8)
    return dict(color=color, rgb=rgb, weight=wsum, views=views.astype(np.uint8))
