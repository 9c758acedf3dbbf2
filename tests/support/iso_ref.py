"""numpy restatement of the shape-view kernels (csrc/iso_render.hip; the specification is the comment of include/eg3d_hip.h "Shape views"):
the brick maxima and the first-hit ray marcher, operation for operation in the order the header states, vectorised over pixels with a loop
over the march steps.  In float32 (the default) tests/test_gpu_shape_render.py requires the GPU outputs to equal these bit for bit; with
dtype=np.float64 the same algorithm runs in double precision (the analytic checks of tests/test_shape_render_cpu.py).

Every scalar is wrapped in the working dtype before it meets an array, so nothing is promoted on the way."""
import numpy as np

BRICK = 8
KMAX = 1 << 24
LAMBERT, NORMAL = 'lambert', 'normal'


def bricks_shape(shape):
    return tuple((int(d) + BRICK - 2) // BRICK for d in shape)


def bricks(vol):
    """[B0,B1,B2]: max of vol over [8b - 1, 8b + 9] per axis, clamped to the grid, NaN ignored (-inf if nothing else), + 0 (no -0)."""
    v = np.asarray(vol)
    T = v.dtype.type
    m = np.where(np.isnan(v), T(-np.inf), v)
    for ax in range(3):
        D = m.shape[ax]
        parts = []
        for b in range(bricks_shape(v.shape)[ax]):
            lo, hi = max(BRICK * b - 1, 0), min(BRICK * b + BRICK + 1, D - 1)
            parts.append(np.max(np.take(m, np.arange(lo, hi + 1), axis=ax), axis=ax, keepdims=True))
        m = np.concatenate(parts, axis=ax)              # a maximum is exact: separable passes give the same values as one pass over 11^3
    return (m + T(0)).astype(v.dtype)


def _clamp(p, h, T):
    p = np.where(p > T(0), p, T(0))
    return np.where(p < h, p, h)


def _lerp(a, b, f):
    r = a + f * (b - a)
    lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
    r = np.where(r < lo, lo, r)
    return np.where(r > hi, hi, r)


class _Grid:
    def __init__(self, vol, T):
        self.v = np.ascontiguousarray(vol, dtype=T)
        self.T = T
        self.D = self.v.shape
        self.h = [T(d - 1) for d in self.D]
        self.evals = 0

    def cell(self, p):
        """p: three clamped coordinate arrays -> (i, f) per axis"""
        i = [np.minimum(np.floor(p[a]).astype(np.int64), self.D[a] - 2) for a in range(3)]
        f = [p[a] - i[a].astype(self.T) for a in range(3)]
        return i, f

    def trilinear(self, i, f):
        v = self.v
        self.evals += int(i[0].size)
        i0, i1, i2 = i
        c00 = _lerp(v[i0, i1, i2], v[i0, i1, i2 + 1], f[2])
        c01 = _lerp(v[i0, i1 + 1, i2], v[i0, i1 + 1, i2 + 1], f[2])
        c10 = _lerp(v[i0 + 1, i1, i2], v[i0 + 1, i1, i2 + 1], f[2])
        c11 = _lerp(v[i0 + 1, i1 + 1, i2], v[i0 + 1, i1 + 1, i2 + 1], f[2])
        return _lerp(_lerp(c00, c01, f[1]), _lerp(c10, c11, f[1]), f[0])

    def field(self, p):
        """p: three unclamped coordinate arrays"""
        return self.trilinear(*self.cell([_clamp(p[a], self.h[a], self.T) for a in range(3)]))


def rays(cams, res, pix, dtype=np.float32):
    """(o [P,3], d [P,3]) of the flat pixel indices pix (into [F,res,res]) exactly as the kernel forms them (RaySampler's rays)."""
    T = dtype
    c = np.asarray(cams, dtype=T)[pix // (res * res)]
    x, y = (pix % res).astype(T), ((pix // res) % res).astype(T)
    fx, sk, cx, fy, cy = c[:, 16], c[:, 17], c[:, 18], c[:, 20], c[:, 21]
    xc, yc = (x + T(0.5)) / T(res), (y + T(0.5)) / T(res)
    xl = (((xc - cx) + (cy * sk) / fy) - (sk * yc) / fy) / fx
    yl = (yc - cy) / fy
    o = np.stack([c[:, 4 * i + 3] for i in range(3)], 1)
    w = np.stack([((c[:, 4 * i] * xl + c[:, 4 * i + 1] * yl) + c[:, 4 * i + 2]) + c[:, 4 * i + 3] for i in range(3)], 1)
    e = w - o
    n = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return o, e / n[:, None]


def march(vol, cams, res, level, origin, spacing, axes=(0, 1, 2), step=0.5, refine=4, skip=True, bricks_=None, shade=LAMBERT, ambient=0.15,
          background=1.0, pix=None, dtype=np.float32):
    """The marcher for the flat pixel indices `pix` (default: all F * res * res).  Returns a dict of arrays over those pixels: depth [P],
    normal [P,3], mask uint8 [P], hit_k int32 [P], shade [P,3] (channel last), and 'evals': the number of field evaluations of the march
    loop (what skipping saves)."""
    T = dtype
    cams = np.asarray(cams)
    F = cams.shape[0]
    pix = np.arange(F * res * res, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64)
    P = pix.size
    g = _Grid(vol, T)
    # inputs arrive through the C structure as fp32 whatever the working precision
    org = [T(np.float32(v)) for v in origin]
    sp = [T(np.float32(v)) for v in spacing]
    level = T(np.float32(level))
    dt = T(np.float32(step) * min(abs(np.float32(s)) for s in spacing))         # formed on the host in fp32
    ambient, background = T(np.float32(ambient)), T(np.float32(background))
    with np.errstate(all='ignore'):
        o, d = rays(cams, res, pix, T)
        oi = [(o[:, axes[a]] - org[a]) / sp[a] for a in range(3)]
        di = [d[:, axes[a]] / sp[a] for a in range(3)]
        tn, tf, live = np.zeros(P, T), np.full(P, np.inf, T), np.ones(P, bool)
        for a in range(3):
            z = di[a] == T(0)
            live &= np.where(z, (oi[a] >= T(0)) & (oi[a] <= g.h[a]), True)
            t0, t1 = (T(0) - oi[a]) / di[a], (g.h[a] - oi[a]) / di[a]
            lo, hi = np.where(t0 < t1, t0, t1), np.where(t0 < t1, t1, t0)
            tn = np.where(~z & (lo > tn), lo, tn)
            tf = np.where(~z & (hi < tf), hi, tf)
        live &= tf >= tn
        q = np.floor((tf - tn) / dt)
        ok = live & (q >= T(0))
        small = ok & (q < T(KMAX))
        K = np.where(ok, np.where(small, np.where(small, q, T(0)).astype(np.int64), KMAX), -1)
        if skip and bricks_ is None:
            bricks_ = bricks(g.v)
        k = np.zeros(P, np.int64)
        hit = np.full(P, -1, np.int64)
        fb = np.zeros(P, T)
        while True:
            idx = np.nonzero((hit < 0) & (k <= K))[0]
            if idx.size == 0:
                break
            t = tn[idx] + k[idx].astype(T) * dt
            ci, cf = g.cell([_clamp(oi[a][idx] + t * di[a][idx], g.h[a], T) for a in range(3)])
            ev = np.ones(idx.size, bool)
            if skip:
                b = [ci[a] >> 3 for a in range(3)]
                ev = ~(bricks_[b[0], b[1], b[2]] <= level)
                s = np.nonzero(~ev)[0]
                if s.size:
                    si = idx[s]
                    te = np.full(s.size, np.inf, T)
                    for a in range(3):
                        da, ba = di[a][si], b[a][s]
                        plane = np.where(da > T(0), (BRICK * ba + BRICK).astype(T), (BRICK * ba).astype(T))
                        ta = (plane - oi[a][si]) / da
                        te = np.where((da != T(0)) & (ta < te), ta, te)
                    q = np.floor((te - tn[si]) / dt)
                    kn = k[si] + 1
                    far = q > kn.astype(T)
                    inside = far & (q < (K[si] + 1).astype(T))
                    k[si] = np.where(far, np.where(inside, np.where(inside, q, T(0)).astype(np.int64), K[si] + 1), kn)
            e = np.nonzero(ev)[0]
            if e.size:
                ei = idx[e]
                v = g.trilinear([c[e] for c in ci], [c[e] for c in cf])
                h = v > level
                hit[ei[h]] = k[ei[h]]
                fb[ei[h]] = v[h]
                k[ei[~h]] += 1
        evals = g.evals

        th = np.zeros(P, T)
        th[hit == 0] = tn[hit == 0]
        r = np.nonzero(hit > 0)[0]
        if r.size:
            point = lambda tt: [oi[a][r] + tt * di[a][r] for a in range(3)]     # noqa: E731
            ta, tb = tn[r] + (hit[r] - 1).astype(T) * dt, tn[r] + hit[r].astype(T) * dt
            fa, fbr = g.field(point(ta)), fb[r]
            for _ in range(refine):
                tm = ta + (tb - ta) * T(0.5)
                fm = g.field(point(tm))
                up = fm > level
                tb, fbr = np.where(up, tm, tb), np.where(up, fm, fbr)
                ta, fa = np.where(up, ta, tm), np.where(up, fa, fm)
            ts = ta + (tb - ta) * ((level - fa) / (fbr - fa))
            th[r] = np.where((ts >= ta) & (ts <= tb), ts, tb)

        n = np.zeros((P, 3), T)
        hh = np.nonzero(hit >= 0)[0]
        if hh.size:
            p = [_clamp(oi[a][hh] + th[hh] * di[a][hh], g.h[a], T) for a in range(3)]
            for a in range(3):
                u, l = _clamp(p[a] + T(1), g.h[a], T), _clamp(p[a] - T(1), g.h[a], T)
                pu, pl = list(p), list(p)
                pu[a], pl[a] = u, l
                n[hh, axes[a]] = -((g.field(pu) - g.field(pl)) / ((u - l) * sp[a]))
            nh = n[hh]
            ln = np.sqrt((nh[:, 0] * nh[:, 0] + nh[:, 1] * nh[:, 1]) + nh[:, 2] * nh[:, 2])
            okn = ln > T(0)
            n[hh] = np.where(okn[:, None], nh / ln[:, None], T(0))

        sh = np.full((P, 3), background, T)
        if hh.size:
            nh, dh = n[hh], d[hh]
            if shade == LAMBERT:
                lam = -((nh[:, 0] * dh[:, 0] + nh[:, 1] * dh[:, 1]) + nh[:, 2] * dh[:, 2])
                lam = np.where(lam > T(0), lam, T(0))
                v = ambient + (T(1) - ambient) * lam
                sh[hh] = (v * T(2) - T(1))[:, None]
            elif shade == NORMAL:
                c = np.asarray(cams, dtype=T)[pix[hh] // (res * res)]
                for j in range(3):
                    nc = (c[:, j] * nh[:, 0] + c[:, 4 + j] * nh[:, 1]) + c[:, 8 + j] * nh[:, 2]
                    sh[hh, j] = (nc * T(0.5) + T(0.5)) * T(2) - T(1)
            else:
                raise ValueError(shade)
    return dict(depth=th, normal=n, mask=(hit >= 0).astype(np.uint8), hit_k=hit.astype(np.int32), shade=sh, evals=evals)
