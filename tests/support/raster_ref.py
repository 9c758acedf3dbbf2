"""numpy restatement of the mesh rasteriser (csrc/mesh_raster.hip; the specification is the comment of include/eg3d_hip.h "Mesh previews"):
the vertex stage vectorised over vertices, the face stage as a loop over the faces in index order that keeps the minimum key of every pixel
(int64 edge functions, fp32 wherever the header says fp32), the resolve stage vectorised over the covered pixels.
tests/test_gpu_mesh_raster.py requires the GPU outputs to equal these bit for bit.

Every scalar is wrapped in float32 before it meets an array, so nothing is promoted on the way."""
import numpy as np

T = np.float32
SMALL = 8                                                 # EG3D_RASTER_SMALL
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = ('texture', 'vertex', 'lambert')


def project(cams, points, res, near):
    """(X int64 [N,V], Y, z fp32 [N,V], valid bool [N,V]): the vertex stage."""
    cams = np.asarray(cams, dtype=T).reshape(-1, 25)
    p = np.asarray(points, dtype=T).reshape(-1, 3)
    N, V = cams.shape[0], p.shape[0]
    X, Y = np.zeros((N, V), np.int64), np.zeros((N, V), np.int64)
    z, valid = np.zeros((N, V), T), np.zeros((N, V), bool)
    lim = T(32768)
    with np.errstate(all='ignore'):
        for n in range(N):
            m = cams[n]
            q = [p[:, i] - m[4 * i + 3] for i in range(3)]
            c = [(m[j] * q[0] + m[4 + j] * q[1]) + m[8 + j] * q[2] for j in range(3)]
            fx, sk, cx, fy, cy = m[16], m[17], m[18], m[20], m[21]
            xl, yl = c[0] / c[2], c[1] / c[2]
            yc = yl * fy + cy
            xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy
            px, py = xc * T(res) - T(0.5), yc * T(res) - T(0.5)
            ok = (c[2] > T(near)) & (px >= -lim) & (px <= lim) & (py >= -lim) & (py <= lim)
            X[n] = np.where(ok, np.floor(np.where(ok, px, T(0)) * T(256) + T(0.5)), T(0)).astype(np.int64)
            Y[n] = np.where(ok, np.floor(np.where(ok, py, T(0)) * T(256) + T(0.5)), T(0)).astype(np.int64)
            z[n], valid[n] = c[2], ok
    return X, Y, z, valid


def _orient(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def weights(S, zs, area2, x, y):
    """(covered and kept, w [3], W): S = (X0, Y0, X1, Y1, X2, Y2) int64, zs = (z0, z1, z2) fp32, pixel coordinates x, y (int64); everything
    broadcasts, so the face loop passes scalars for the face and the resolve stage arrays."""
    X0, Y0, X1, Y1, X2, Y2 = S
    PX, PY = 256 * x, 256 * y
    E = [_orient(X1, Y1, X2, Y2, PX, PY), _orient(X2, Y2, X0, Y0, PX, PY), _orient(X0, Y0, X1, Y1, PX, PY)]
    neg = area2 < 0
    E = [np.where(neg, -e, e) for e in E]
    A = np.where(neg, -area2, area2)
    inside = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
    with np.errstate(all='ignore'):
        fa = np.asarray(A, np.int64).astype(T)
        w = [(np.asarray(E[k], np.int64).astype(T) / fa) / zs[k] for k in range(3)]
        W = (w[0] + w[1]) + w[2]
        kept = inside & (W > T(0)) & (W < T(np.inf))
    return kept, w, W


def lift(cam, res, x, y):
    """(xl, yl) of the pixels (y, x): the ray lift as the marcher forms it"""
    c = np.asarray(cam, dtype=T)
    fx, sk, cx, fy, cy = c[16], c[17], c[18], c[20], c[21]
    xc, yc = (x.astype(T) + T(0.5)) / T(res), (y.astype(T) + T(0.5)) / T(res)
    xl = (((xc - cx) + (cy * sk) / fy) - (sk * yc) / fy) / fx
    yl = (yc - cy) / fy
    return xl, yl


def _mix(b, a0, a1, a2):
    return (b[0] * a0 + b[1] * a1) + b[2] * a2


def _clamp(p, h):
    p = np.where(p > T(0), p, T(0))
    return np.where(p < h, p, h)


def _lerp(a, b, f):
    return a + f * (b - a)


def raster(points, faces, cams, res, mode='texture', uv=None, texture=None, colors=None, normals=None, cull='back', near=0.1, background=1.0,
           ambient=0.2):
    """dict(image [N,3,res,res], face int32, z, depth, mask uint8 [N,res,res], bary [N,res,res,3], bad_faces, small_faces, large_faces)
    exactly as the kernel writes them."""
    assert mode in MODES and cull in ('back', 'none')
    cams = np.asarray(cams, dtype=T).reshape(-1, 25)
    p = np.asarray(points, dtype=T).reshape(-1, 3)
    fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N, V, F = cams.shape[0], p.shape[0], fc.shape[0]
    near, background, ambient = T(near), T(background), T(ambient)
    X, Y, z, valid = project(cams, p, res, near)
    inrange = ((fc >= 0) & (fc < V)).all(1)
    safe = np.where(inrange[:, None], fc, 0)
    out = dict(image=np.full((N, 3, res, res), background, T), face=np.full((N, res, res), -1, np.int32), z=np.zeros((N, res, res), T),
               depth=np.zeros((N, res, res), T), mask=np.zeros((N, res, res), np.uint8), bary=np.zeros((N, res, res, 3), T),
               bad_faces=int((~inrange).sum()), small_faces=0, large_faces=0)
    for n in range(N):
        zb = np.full((res, res), EMPTY, np.uint64)
        if F and V:
            SX, SY, SZ = X[n][safe], Y[n][safe], z[n][safe]                                # [F,3]
            area2 = _orient(SX[:, 0], SY[:, 0], SX[:, 1], SY[:, 1], SX[:, 2], SY[:, 2])
            live = inrange & valid[n][safe].all(1) & (area2 != 0)
            if cull == 'back':
                live &= ~(area2 > 0)
            x0, y0 = np.maximum((SX.min(1) + 255) >> 8, 0), np.maximum((SY.min(1) + 255) >> 8, 0)
            x1, y1 = np.minimum(SX.max(1) >> 8, res - 1), np.minimum(SY.max(1) >> 8, res - 1)
            live &= (x1 >= x0) & (y1 >= y0)
            small = live & (x1 - x0 + 1 <= SMALL) & (y1 - y0 + 1 <= SMALL)
            out['small_faces'] += int(small.sum())
            out['large_faces'] += int((live & ~small).sum())
            for f in np.nonzero(live)[0]:
                yy, xx = np.meshgrid(np.arange(y0[f], y1[f] + 1), np.arange(x0[f], x1[f] + 1), indexing='ij')
                S = (SX[f, 0], SY[f, 0], SX[f, 1], SY[f, 1], SX[f, 2], SY[f, 2])
                kept, _, W = weights(S, (SZ[f, 0], SZ[f, 1], SZ[f, 2]), area2[f], xx, yy)
                if not kept.any():
                    continue
                with np.errstate(all='ignore'):
                    zp = (T(1) / W).astype(T)
                key = (zp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
                win = zb[y0[f]:y1[f] + 1, x0[f]:x1[f] + 1]
                win[...] = np.where(kept & (key < win), key, win)
        hit = zb != EMPTY
        yy, xx = np.nonzero(hit)
        if yy.size == 0:
            continue
        f = (zb[yy, xx] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        k = fc[f]                                                                          # [P,3]
        S = (X[n][k[:, 0]], Y[n][k[:, 0]], X[n][k[:, 1]], Y[n][k[:, 1]], X[n][k[:, 2]], Y[n][k[:, 2]])
        zs = (z[n][k[:, 0]], z[n][k[:, 1]], z[n][k[:, 2]])
        area2 = _orient(*S)
        kept, w, W = weights(S, zs, area2, xx.astype(np.int64), yy.astype(np.int64))
        assert kept.all()
        with np.errstate(all='ignore'):
            zp = T(1) / W
            b = [w[j] / W for j in range(3)]
            xl, yl = lift(cams[n], res, xx, yy)
            out['face'][n, yy, xx] = f.astype(np.int32)
            out['z'][n, yy, xx] = zp
            out['depth'][n, yy, xx] = zp * np.sqrt((xl * xl + yl * yl) + T(1))
            out['mask'][n, yy, xx] = 1
            out['bary'][n, yy, xx] = np.stack(b, 1)
            if mode == 'texture':
                tex = np.asarray(texture)
                assert tex.dtype == np.uint8 and tex.ndim == 3 and tex.shape[2] == 3
                Ht, Wt = tex.shape[:2]
                A = np.asarray(uv, dtype=T).reshape(-1, 3, 2)[f]                           # [P,3,2]
                u, v = _mix(b, A[:, 0, 0], A[:, 1, 0], A[:, 2, 0]), _mix(b, A[:, 0, 1], A[:, 1, 1], A[:, 2, 1])
                tx, ty = _clamp(u * T(Wt) - T(0.5), T(Wt - 1)), _clamp(v * T(Ht) - T(0.5), T(Ht - 1))
                ix, iy = np.minimum(np.floor(tx).astype(np.int64), Wt - 2), np.minimum(np.floor(ty).astype(np.int64), Ht - 2)
                gx, gy = tx - ix.astype(T), ty - iy.astype(T)
                t = tex.astype(T)
                for j in range(3):
                    col = _lerp(_lerp(t[iy, ix, j], t[iy, ix + 1, j], gx), _lerp(t[iy + 1, ix, j], t[iy + 1, ix + 1, j], gx), gy)
                    out['image'][n, j, yy, xx] = (col - T(127.5)) / T(127.5)
            elif mode == 'vertex':
                col = np.asarray(colors, dtype=T).reshape(-1, 3)
                for j in range(3):
                    out['image'][n, j, yy, xx] = _mix(b, col[k[:, 0], j], col[k[:, 1], j], col[k[:, 2], j])
            else:
                nr = np.asarray(normals, dtype=T).reshape(-1, 3)
                nn = [_mix(b, nr[k[:, 0], j], nr[k[:, 1], j], nr[k[:, 2], j]) for j in range(3)]
                ln = np.sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2])
                ok = (ln > T(0)) & (ln < T(np.inf))
                nn = [np.where(ok, nn[j] / np.where(ok, ln, T(1)), T(0)) for j in range(3)]
                c = cams[n]
                e = [(((c[4 * i] * xl + c[4 * i + 1] * yl) + c[4 * i + 2]) + c[4 * i + 3]) - c[4 * i + 3] for i in range(3)]
                dn = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                d = [e[i] / dn for i in range(3)]
                s = -((nn[0] * d[0] + nn[1] * d[1]) + nn[2] * d[2])
                s = np.where(s > T(0), s, T(0))
                val = (ambient + (T(1) - ambient) * s) * T(2) - T(1)
                for j in range(3):
                    out['image'][n, j, yy, xx] = val
    return out
