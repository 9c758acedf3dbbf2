"""Independent float64 restatement of the kernels of csrc/epilogue.hip -- the layer epilogue forward, the activation backward in its three
incoming-gradient forms, eg3d_dgrad_finish, eg3d_weight_sqsum, eg3d_demod_fwd / _bwd, eg3d_weight_grad_finish (slabs) and eg3d_unpack_weight_grad --
their derived error bounds, the launch arithmetic of the activation backward and the case lists of tests/test_epilogue_cpu.py and
tests/test_gpu_epilogue.py.  Plain numpy, float64, no autograd; nothing here calls the library.  Only the piecewise-linear activations (linear,
relu, lrelu) are on the path and restated; the other activations of the epilogue templates are out of scope.

Layout: activations are [N, HW, C] (the kernels' NHWC with the pixels flattened), noise [1, HW] (shared by the batch) or [N, HW].

The operations (networks_stylegan2.py:60-66, 89-90, 327-329; bias_act semantics)
  forward      out = clamp(gain pwl(FIR(z) d[n,c] + noise strength + bias[c])),  pwl(v) = v (v > 0), slope v (else); slope 1 / alpha / 0;
               FIR = true convolution (flipped filter) of z zero-padded by pad0 on every side, times fir_gain.
  act backward keyed on the fp32 `out` the kernel reads (its sign and its clamp comparison are then exact on both sides):
               dy = g gain (out > 0 ? 1 : slope), 0 where |out| >= clamp;   dz = dy d;   dbias[c] = sum_{n,p} dy;
               pre = out / gain (out > 0), out / gain / slope (else; relu: not invertible, no dd);   dd[n,c] = sum_p dy (pre - bias - noise strength) / d;
               dnoise[n,p] = strength sum_c dy (shared noise: also summed over n);   dstrength = sum_{n,p} noise sum_c dy.
               g = dout | z s[n,c] + addend with ds[n,c] += sum_p z out | (dy4 wa4^T) s + addend the same way.
  dgrad_finish dx = z s + addend,  ds[n,c] += sum_p z x.
  demodulation wsq[o,k] = sum_t w^2;  d[n,o] = (sum_k s^2 wsq + 1e-8)^-1/2;  ds[n,k] += -s sum_o dd d^3 wsq;  dwsq[o,k] += sum_n dd (-1/2) d^3 s^2;
               dw[o,i,t] = sum_slabs g[o][t I + i] + 2 w[o,i,t] dwsq[o,i]   (weight_grad_finish);
               dw[o,i,t] = g[o][t Ip + i] a[o],  da[o] = sum_{i,t} g w      (unpack_weight_grad; Ip >= I pads a row of g).

The bounds.  u = 2^-24.  A product or a sum rounds once (relative u); an fma dot of m terms has an error of at most (m + 1) u sum|terms|; a sum whose
terms pass through at most D additions has at most D u sum|terms| (first order; Higham, Accuracy and Stability, 4.2).  A target that starts from a
non-zero value takes part in the atomic additions, so its |start| joins sum|terms|.  No constant comes from what a kernel returns; the depths are read
off the kernels' loops and the host code's launch arithmetic.

  F  forward.  The filter is multiplied by fir_gain once (u), then an m = fh fw term dot:  eF = (m + 2) u sum|f z| (the separable strip form -- two
     4-term passes of depth 3 and one product -- is inside it).  With A = |FIR d| + |noise strength| + |bias|: the product with d, the product
     noise strength and two additions of partial sums:  e_pre = eF |d| + 4 u A.  The activation multiplies by slope and gain (2 u) and is 1-Lipschitz
     times gain across the kink; the clamp is non-expansive:  tol_out = gain sl e_pre + 2 u |out|,  sl = slope where pre < -e_pre, else 1.
     max|out| is compared within the largest tol_out.
  G  incoming gradient.  plain: exact.  z s + addend: 2 u (|z s| + |addend|) (mul + add or one fma).  dy4 wa4^T: a 4-term fma dot, 5 u sum|dy4 wa4| = e_zz,
     then |s| e_zz + 2 u (|zz s| + |addend|).
  E  elementwise.  dy = g gain slope: 2 u |dy| + gain sl e_g = e_dy;  dz = dy d: e_dz = 3 u |dz| + gain sl |d| e_g.  max|dz| within the largest e_dz.
  L  launch (host code):  ppb = max(1024 // (C/4), 1) pixel lanes per block;  bx = max(1, min(ceil(HW / (4 ppb)), max(1, 256 // N))) blocks per image
     (8 ppb in eg3d_dgrad_finish);  trips = ceil(HW / (4 bx ppb)), four pixels per lane and trip.  A lane adds its 4 trips terms in sequence, the lanes
     meet in a tree of ceil(log2 ppb) levels (dgrad_finish: one thread adds the ppb lanes in sequence), every block commits one atomic:
         D_img = 4 trips + ceil(log2 ppb) + bx        (dd, ds: one image),     D_ch = 4 trips + ceil(log2 ppb) + bx N      (dbias: all images).
  R  reductions of the activation backward, T = the float64 terms:
     dbias:  (D_ch + 2) u (sum|dy| + |start|) + sum gain sl e_g        (2: the roundings of dy itself)
     dd:     the term dy (pre - bias - nz): pre = (out inv_gain) inv_slope with both reciprocals rounded (4 u), nz one product, two subtractions and the
             product -- at most 9 u T_d, T_d = |dy| (|pre| + |bias| + |nz|); the sum D_img; the division by d one more:
             ((D_img + 10) u sum T_d + sum gain sl e_g (|pre| + |bias| + |nz|)) / |d| + D_img u |start|.
     ds:     terms z out (u each; dy4 form: e_zz |out| too):  (D_img + 1) u (sum|z out| + |start|) + sum e_zz |out|.
     dnoise: a lane's four channels in two levels, C/4 lanes of a pixel by a shuffle tree inside a wave (C/4 a power of two: log2 min(C/4, 64) levels, then
             one atomic per wave of the pixel; else one atomic per lane), the product with strength, images into a shared map one after the other:
             D_n = 2 + log2 grp + (C/4 / grp) imgs + 3   or   2 + (C/4) imgs + 3;   D_n u (|strength| sum_c |dy| + |start|) + |strength| sum_c e_dy.
     dstrength: the pixel's channel sum as above times noise (u), a lane's 4 trips terms in sequence, then the block's LDS accumulation -- one atomic add
             into one LDS word per contributing thread, up to 1024 in sequence -- and one atomic per block:
             D_s = 2 + log2 grp + 1 + 4 trips + leaders + bx N,  leaders = ppb C/4 / grp;   D_s u (sum |noise| sum_c|dy| + |start|) + sum |noise| sum_c e_dy.
             (The deterministic build adds every lane's partial exactly; it is inside the same bound.)
  D  dgrad_finish.  dx: 2 u (|z s| + |addend|).  ds: (4 trips + ppb + bx + 1) u (sum|z x| + |start|), the launch arithmetic with 8 ppb.
  Q  weight_sqsum: T squares added in sequence: (T + 1) u wsq.
  M  demod_fwd.  A lane adds ceil(Ck / 64) terms s s wsq (2 roundings each), six shuffle levels; the terms are non-negative, so the sum is relatively
     accurate to Dk u, Dk = ceil(Ck / 64) + 8; + 1e-8f (u); sqrt and the reciprocal are allowed 1 ulp = 2 u each:   tol_d = |d| ((Dk + 1) / 2 + 4) u.
     ds: a thread adds ceil(per / 4) fma terms (dd d d d: 3 roundings) of its slice of `per` = ceil(Co / osplit) outputs, osplit = max(1, min(Co // 16, 16)),
     four partial sums meet (3), the product with -s (1), one atomic per slice:  (ceil(per / 4) + 8 + osplit) u (|s| sum_o |dd d^3 wsq| + |start|).
     dwsq: N terms of five roundings added in sequence, and the final `+=`:  (N + 6) u (sum_n |term| + |start|).
  W  weight_grad_finish.  The slabs are added in order: (nslab - 1) u sum|g|;  q[i] = 2 sum_n fma(dd (-1/2) d^3, s s): four roundings per term and the
     dot:  e_q = (N + 5) u 2 sum_n |term|;  the final fma:   tol = (nslab - 1) u sum_slabs |g| + |w| e_q + u (|w q| + |sum g|).
  P  unpack_weight_grad.  dw = g a: u |dw|.  da: a thread's fma dot of ceil(I T / 256) terms, six shuffle levels, two more over the four waves:
     (ceil(I T / 256) + 9) u sum|g w|.
"""
import math
import zlib

import numpy as np

U = 2.0 ** -24
THREADS, CAP, PER_LANE = 1024, 256, 4
EPS32 = float(np.float32(1e-8))
F32 = lambda v: float(np.float32(v))      # noqa: E731
GAIN, ALPHA, STRENGTH, CLAMP = F32(math.sqrt(2.0)), F32(0.2), F32(0.37), F32(1.2)          # as the kernels receive them


def _seed(*a):
    return zlib.crc32(repr(a).encode())


def cdiv(a, b):
    return -(-a // b)


def clog2(n):
    return int(math.ceil(math.log2(n))) if n > 1 else 0


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def launch(C, N, HW, finish=False):
    """The activation backward's (finish: eg3d_dgrad_finish's) grid for [N, HW, C], from the host code's formulas (header, L)."""
    assert C % 4 == 0 and 4 <= C <= 1024
    C4 = C // 4
    ppb = max(THREADS // C4, 1)
    bx = max(1, min(cdiv(HW, ppb * (8 if finish else 4)), max(1, CAP // N)))
    trips = cdiv(HW, PER_LANE * bx * ppb)
    pow2 = C4 & (C4 - 1) == 0
    grp = min(C4, 64) if pow2 else 1
    tree = ppb if finish else clog2(ppb)
    return dict(C4=C4, ppb=ppb, bx=bx, trips=trips, pow2=pow2, grp=grp, idle=THREADS - ppb * C4, span=PER_LANE * bx * ppb,
                D_img=PER_LANE * trips + tree + bx, D_ch=PER_LANE * trips + tree + bx * N,
                leaders=ppb * C4 // grp)


def classes(C, N, HW):
    """The launch-shape classes a case belongs to."""
    g = launch(C, N, HW)
    out = set()
    if g['idle']:
        out.add('idle threads')
    if g['C4'] > 64:
        out.add('pixel wider than a wave')
    if HW == 1:
        out.add('one pixel')
    if g['trips'] == 1 and HW % g['span']:
        out.add('single partial trip')
    if g['trips'] == 1 and HW == g['span']:
        out.add('single full trip')
    if g['trips'] == 2 and HW % g['span']:
        out.add('two trips, ragged last')
    if g['ppb'] == THREADS:
        out.add('1024 pixel lanes')
    if C == 1024:
        out.add('channel limit')
    return out


def pixel_owner(C, N, HW, finish=False):
    """(block, lane, trip) of every pixel of an image."""
    g = launch(C, N, HW, finish)
    p = np.arange(HW)
    return (p // g['ppb']) % g['bx'], p % g['ppb'], p // g['span']


# ---------------------------------------------------------------------------------------------------------------- forward
def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def fir_ref(z, f, pad0, fir_gain, flip=True, shift=0):
    """z [N, Hz, Wz, C], f [fh, fw] -> (FIR [N, H, W, C], sum |f z| the same shape).  flip=False / shift=1 are the mutants."""
    z, f = _f64(z), _f64(f)
    fh, fw = f.shape
    n, hz, wz, c = z.shape
    h, w = hz + 2 * pad0 - fh + 1, wz + 2 * pad0 - fw + 1
    q = pad0 + 1
    zp = np.pad(z, ((0, 0), (q, q), (q, q), (0, 0)))
    ff = (f[::-1, ::-1] if flip else f) * fir_gain
    val, mag = np.zeros((n, h, w, c)), np.zeros((n, h, w, c))
    for ky in range(fh):
        for kx in range(fw):
            win = zp[:, 1 + shift + ky:1 + shift + ky + h, 1 + shift + kx:1 + shift + kx + w]
            val += ff[ky, kx] * win
            mag += abs(ff[ky, kx]) * np.abs(win)
    return val, mag


def fwd_ref(z, fir=None, pad0=0, fir_gain=1.0, d=None, noise=None, strength=0.0, bias=None, slope=1.0, gain=1.0, clamp=-1.0, flip=True, shift=0):
    """z [N, Hz, Wz, C]; d [N, C]; noise [1 or N, H, W]; bias [C].  Returns (out [N, H, W, C], tol, max|out|, tol of the maximum)."""
    z = _f64(z)
    if fir is not None:
        v, mag = fir_ref(z, fir, pad0, fir_gain, flip, shift)
        eF = (fir.shape[0] * fir.shape[1] + 2) * U * mag
    else:
        v, eF = z, np.zeros_like(z)
    dv = np.ones((1, 1, 1, 1)) if d is None else _f64(d)[:, None, None, :]
    nz = 0.0 if noise is None else (_f64(noise) * F32(strength))[:, :, :, None]
    b = 0.0 if bias is None else _f64(bias)[None, None, None, :]
    pre = v * dv + nz + b
    e_pre = eF * np.abs(dv) + 4 * U * (np.abs(v * dv) + np.abs(nz) + np.abs(b))
    sl_ref = np.where(pre > 0, 1.0, slope)
    out = pre * sl_ref * gain
    sl = np.where(pre < -e_pre, slope, 1.0)
    tol = gain * sl * e_pre + 2 * U * np.abs(out)
    if clamp >= 0:
        out = np.clip(out, -clamp, clamp)
    return out, tol, float(np.abs(out).max()), float(tol.max())


# ---------------------------------------------------------------------------------------------------------------- incoming gradient
def grad_plain(dout):
    return dict(g=_f64(dout), e_g=None)


def grad_finish(z, s, addend):
    """g = z s[n,c] + addend; also the terms of ds (z)."""
    z = _f64(z)
    zs = z * (1.0 if s is None else _f64(s)[:, None, :])
    a = 0.0 if addend is None else _f64(addend)
    return dict(g=zs + a, e_g=2 * U * (np.abs(zs) + np.abs(a)), zz=z, e_zz=None)


def grad_torgb(dy4, wa4, s, addend):
    """dy4 [N, HW, 4], wa4 [C, 4]:  zz = dy4 wa4^T."""
    dy4, wa4 = _f64(dy4), _f64(wa4)
    sh = dy4.shape[:2] + (wa4.shape[0],)
    zz = (dy4.reshape(-1, 4) @ wa4.T).reshape(sh)                        # (2-D: one dgemm)
    e_zz = (5 * U) * (np.abs(dy4).reshape(-1, 4) @ np.abs(wa4).T).reshape(sh)
    sv = np.ones((1, 1, 1)) if s is None else _f64(s)[:, None, :]
    a = 0.0 if addend is None else _f64(addend)
    return dict(g=zz * sv + a, e_g=np.abs(sv) * e_zz + 2 * U * (np.abs(zz * sv) + np.abs(a)), zz=zz, e_zz=e_zz)


# ---------------------------------------------------------------------------------------------------------------- activation backward
def act_terms(G, out, d=None, bias=None, noise=None, strength=0.0, slope=ALPHA, gain=GAIN, clamp=-1.0, relu=False):
    """The per-element float64 quantities of one activation backward (everything act_reduce sums): see act_bwd_ref."""
    g, e_g = G['g'], G['e_g']
    out = _f64(out)
    N, HW, C = out.shape
    pos = out > 0
    sl = np.where(pos, 1.0, slope)
    sl *= gain
    dy = g * sl
    p_dy = sl * e_g if e_g is not None else None                         # propagated from the incoming gradient (None: it is exact)
    if clamp >= 0:
        live = np.abs(out) < clamp
        dy *= live
        if p_dy is not None:
            p_dy *= live
    t = dict(N=N, HW=HW, C=C, L=launch(C, N, HW), dy=dy, p_dy=p_dy, dv=np.ones((1, C)) if d is None else _f64(d), has_d=d is not None, relu=relu,
             shared=noise is not None and np.shape(noise)[0] == 1, has_noise=noise is not None, s32=F32(strength))
    t['nraw'] = np.zeros((1, HW)) if noise is None else _f64(noise)
    nz = t['nraw'] * t['s32']
    b = np.zeros(C) if bias is None else _f64(bias)
    if d is not None and not relu:
        yy = out / gain
        pre = np.where(pos, yy, yy / slope)
        t['rest'] = pre - b[None, None, :] - nz[:, :, None]
        t['mag'] = np.abs(pre) + np.abs(b)[None, None, :] + np.abs(nz)[:, :, None]
    if 'zz' in G:
        t['tz'], t['e_tz'] = G['zz'] * out, G['e_zz'] * np.abs(out) if G['e_zz'] is not None else None
    return t


def _act_fixed(t):
    """What act_reduce needs that depends neither on the mask nor on the start: computed once per act_terms."""
    if 'fixed' in t:
        return t['fixed']
    N, HW, C, L, dy, p_dy, dv = t['N'], t['HW'], t['C'], t['L'], t['dy'], t['p_dy'], t['dv']
    ady = np.abs(dy)
    zero = np.zeros(())
    f = dict(ady=ady, dz=dy * dv[:, None, :])
    f['tol_dz'] = 3 * U * np.abs(f['dz'])
    if p_dy is not None:
        f['tol_dz'] += np.abs(dv)[:, None, :] * p_dy
    f['dz_amax'], f['tol_dz_amax'] = float(np.abs(f['dz']).max()), float(f['tol_dz'].max())
    f['s_ady'], f['s_pdy'] = ady.sum((0, 1)), p_dy.sum((0, 1)) if p_dy is not None else zero
    if 'rest' in t:
        f['td'] = dy * t['rest']
        f['s_mag'], f['s_pmag'] = (ady * t['mag']).sum(1), (p_dy * t['mag']).sum(1) if p_dy is not None else zero
    if t['has_noise']:
        f['cs'], f['acs'] = dy.sum(2), ady.sum(2)
        f['ecs'] = 2 * U * f['acs'] + (p_dy.sum(2) if p_dy is not None else 0.0)
    if 'tz' in t:
        f['s_atz'], f['s_etz'] = np.abs(t['tz']).sum(1), t['e_tz'].sum(1) if t['e_tz'] is not None else zero
    t['fixed'] = f
    return f


def _msum(a, mask, axes):
    """Sum of a [N, HW, C] over `axes`, the pixels weighted by mask [N, HW] (None: all ones)."""
    return a.sum(axes) if mask is None else (a * _f64(mask)[:, :, None]).sum(axes)


def act_reduce(t, start=None, mask=None, mutant=None):
    """The outputs and bounds from act_terms.  mask [N, HW]: weights of the pixels in every reduction (the CPU file's mutants drop pixels with it);
    mutant: 'dd_times_d'."""
    N, HW, C, L, dy, dv = t['N'], t['HW'], t['C'], t['L'], t['dy'], t['dv']
    f = _act_fixed(t)
    start = start or {}
    st = lambda k: _f64(start[k]) if start.get(k) is not None else 0.0          # noqa: E731
    r = dict(dz=f['dz'], tol_dz=f['tol_dz'], dz_amax=f['dz_amax'], tol_dz_amax=f['tol_dz_amax'], launch=L)
    r['dbias'] = _msum(dy, mask, (0, 1)) + st('dbias')
    r['tol_dbias'] = (L['D_ch'] + 2) * U * (f['s_ady'] + np.abs(st('dbias'))) + f['s_pdy']
    if 'rest' in t:
        dd = _msum(f['td'], mask, 1)
        dd = dd * dv if mutant == 'dd_times_d' else dd / dv
        r['dd'] = dd + st('dd')
        r['tol_dd'] = ((L['D_img'] + 10) * U * f['s_mag'] + f['s_pmag']) / np.abs(dv) + L['D_img'] * U * np.abs(st('dd'))
    if t['has_noise']:
        shared, nraw, s32 = t['shared'], t['nraw'], t['s32']
        cs, acs, ecs = f['cs'] if mask is None else f['cs'] * _f64(mask), f['acs'], f['ecs']                      # [N, HW]
        imgs = N if shared else 1
        Dn = (2 + clog2(L['grp']) + L['C4'] // L['grp'] * imgs + 3) if L['pow2'] else (2 + L['C4'] * imgs + 3)
        dn = cs.sum(0, keepdims=True) if shared else cs
        adn, edn = (acs.sum(0, keepdims=True), ecs.sum(0, keepdims=True)) if shared else (acs, ecs)
        r['dnoise'] = s32 * dn + st('dnoise')
        r['tol_dnoise'] = Dn * U * (abs(s32) * adn + np.abs(st('dnoise'))) + abs(s32) * edn
        Ds = 2 + clog2(L['grp']) + 1 + PER_LANE * L['trips'] + L['leaders'] + L['bx'] * N
        r['dstrength'] = float((cs * nraw).sum()) + st('dstrength')
        r['tol_dstrength'] = Ds * U * (float((acs * np.abs(nraw)).sum()) + np.abs(st('dstrength'))) + float((ecs * np.abs(nraw)).sum())
    if 'tz' in t:
        r['ds'] = _msum(t['tz'], mask, 1) + st('ds')
        r['tol_ds'] = (L['D_img'] + 1) * U * (f['s_atz'] + np.abs(st('ds'))) + f['s_etz']
    return r


def act_bwd_ref(G, out, d=None, bias=None, noise=None, strength=0.0, slope=ALPHA, gain=GAIN, clamp=-1.0, relu=False, start=None, mask=None, mutant=None):
    """G: grad_plain / grad_finish / grad_torgb;  out [N, HW, C] (the fp32 values the kernel reads);  d [N, C];  bias [C];  noise [1 or N, HW];
    start: dict of the targets' starting values (dbias [C], dd [N, C], dnoise like noise, dstrength scalar, ds [N, C]).
    Returns value and tol_<name> of dz, dbias, dd (not relu, d given), dnoise, dstrength (noise given), ds (finish forms), dz_amax."""
    return act_reduce(act_terms(G, out, d, bias, noise, strength, slope, gain, clamp, relu), start, mask, mutant)


ACT_OUTPUTS = ('dz', 'dbias', 'dd', 'dnoise', 'dstrength', 'ds')


# ---------------------------------------------------------------------------------------------------------------- the remaining kernels
def dgrad_finish_ref(z, x, s, addend, start_ds=None, mask=None):
    """z, x, addend [N, HW, C]; s [N, C].  Returns dx, tol_dx and (x given) ds, tol_ds."""
    z = _f64(z)
    N, HW, C = z.shape
    L = launch(C, N, HW, finish=True)
    zs = z * (1.0 if s is None else _f64(s)[:, None, :])
    a = 0.0 if addend is None else _f64(addend)
    r = dict(dx=zs + a, tol_dx=2 * U * (np.abs(zs) + np.abs(a)), launch=L)
    if x is not None:
        t = z * _f64(x)
        s0 = 0.0 if start_ds is None else _f64(start_ds)
        m3 = 1.0 if mask is None else _f64(mask)[:, :, None]
        r['ds'] = (t * m3).sum(1) + s0
        r['tol_ds'] = (L['D_img'] + 1) * U * (np.abs(t).sum(1) + np.abs(s0))
    return r


def weight_sqsum_ref(wp):
    """wp [Co, T, Ck] (the packed forward operand) -> wsq [Co, Ck], tol."""
    wp = _f64(wp)
    wsq = (wp * wp).sum(1)
    return wsq, (wp.shape[1] + 1) * U * wsq


def demod_fwd_ref(s, wsq, mutant=None):
    s, wsq = _f64(s), _f64(wsq)
    acc = (s if mutant == 's_for_s2' else s * s) @ wsq.T + EPS32
    d = 1.0 / np.sqrt(acc)
    Dk = cdiv(s.shape[1], 64) + 8
    return d, np.abs(d) * ((Dk + 1) / 2 + 4) * U


def demod_bwd_ref(s, wsq, d, dd, start_ds=None, start_dwsq=None, mutant=None):
    """s [N, Ck], wsq [Co, Ck], d and dd [N, Co] -> ds [N, Ck], tol_ds, dwsq [Co, Ck], tol_dwsq.  mutants: 'd2', 'no_half', 's_for_s2'."""
    s, wsq, d, dd = _f64(s), _f64(wsq), _f64(d), _f64(dd)
    N, Ck = s.shape
    Co = wsq.shape[0]
    d3 = d * d if mutant == 'd2' else d * d * d
    c = dd * d3                                                    # [N, Co]
    s0 = 0.0 if start_ds is None else _f64(start_ds)
    w0 = 0.0 if start_dwsq is None else _f64(start_dwsq)
    osplit = max(1, min(Co // 16, 16))
    per = cdiv(Co, osplit)
    ds = -s * (c @ wsq) + s0
    tol_ds = (cdiv(per, 4) + 8 + osplit) * U * (np.abs(s) * (np.abs(c) @ np.abs(wsq)) + np.abs(s0))
    s2 = s if mutant == 's_for_s2' else s * s
    half = 1.0 if mutant == 'no_half' else 0.5
    dwsq = -half * (c.T @ s2) + w0
    tol_dwsq = (N + 6) * U * (0.5 * (np.abs(c).T @ (s * s)) + np.abs(w0))
    return ds, tol_ds, dwsq, tol_dwsq


def weight_grad_finish_ref(slabs, w, s, d, dd, mutant=None):
    """slabs [nslab, O, T I] (packed rows g[o][t I + i]), w [O, I, T], s [N, I], d and dd [N, O] (dd None: no demodulation term) -> dw [O, I, T], tol.
    mutants: 'd2', 'no_two', 'no_half', 's_for_s2', 'slab_missing'."""
    slabs, w = _f64(slabs), _f64(w)
    O, I, T = w.shape
    use = slabs[:-1] if mutant == 'slab_missing' else slabs
    G = use.sum(0).reshape(O, T, I).transpose(0, 2, 1)
    aG = np.abs(slabs).sum(0).reshape(O, T, I).transpose(0, 2, 1)
    q, e_q = np.zeros((O, I)), np.zeros((O, I))
    if dd is not None:
        s, d, dd = _f64(s), _f64(d), _f64(dd)
        N = s.shape[0]
        c = dd * (d * d if mutant == 'd2' else d * d * d)
        s2 = s if mutant == 's_for_s2' else s * s
        q = (1.0 if mutant == 'no_two' else 2.0) * -(1.0 if mutant == 'no_half' else 0.5) * (c.T @ s2)
        e_q = (N + 5) * U * 2.0 * 0.5 * (np.abs(c).T @ (s * s))
    wq = w * q[:, :, None]
    tol = (slabs.shape[0] - 1) * U * aG + np.abs(w) * e_q[:, :, None] + U * (np.abs(wq) + np.abs(G))
    return G + wq, tol


def unpack_weight_grad_ref(g, w, a, Ip, mutant=None):
    """g [O, T Ip] (rows g[o][t Ip + i], the padding may hold anything), w [O, I, T], a [O] or None -> dw [O, I, T], tol, da [O], tol.
    mutant 'ip_as_i': the row read with stride I."""
    w = _f64(w)
    O, I, T = w.shape
    g = np.asarray(g, dtype=np.float64)
    if mutant == 'ip_as_i':
        gg = g[:, :T * I].reshape(O, T, I)
    else:
        gg = g.reshape(O, T, Ip)[:, :, :I]
    gg = gg.transpose(0, 2, 1)
    av = np.ones(O) if a is None else _f64(a)
    dw = gg * av[:, None, None]
    da = (gg * w).sum((1, 2))
    return dw, U * np.abs(dw), da, (cdiv(I * T, 256) + 9) * U * np.abs(gg * w).sum((1, 2))


def compare(got, ref, tol):
    """(every element within its bound, largest err / tol); NaN and a non-zero error under a zero bound count as infinite."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    err = np.abs(got.reshape(ref.shape) - ref)
    if not err.size:
        return True, 0.0
    tol = np.broadcast_to(tol, err.shape)
    zero = tol <= 0
    if zero.any():
        if (err[zero] != 0).any():            # (NaN != 0 too)
            return False, float('inf')
        tol = np.where(zero, 1.0, tol)
    err /= tol
    m = float(err.max())            # (NaN propagates through max)
    return (m <= 1.0, m) if m == m else (False, float('inf'))


def margin(mut, ref, tol):
    """Median of |mutant - reference| / tol over the outputs the mutant touches (None: it touches nothing)."""
    mut, ref, tol = (np.asarray(a, dtype=np.float64) for a in (mut, ref, tol))
    diff = np.abs(mut - ref)
    hit = diff > 0
    if not hit.any():
        return None
    return float(np.median(diff[hit] / np.broadcast_to(tol, diff.shape)[hit]))


# ---------------------------------------------------------------------------------------------------------------- cases: activation backward
class ActCase:
    """One launch shape and epilogue setting of the activation backward; `form` is chosen by the test."""

    def __init__(self, C, N, H, W, act='lrelu', clamp=False, noise='image', d=True, bias=True, start=True):
        self.C, self.N, self.H, self.W, self.HW = C, N, H, W, H * W
        self.act, self.clamp, self.noise, self.d, self.bias, self.start = act, clamp, noise, d, bias, start

    @property
    def id(self):
        return f'{self.C}x{self.N}x{self.H}x{self.W}'

    def act_of(self, form):
        """relu has no fused form (eg3d_dgrad_finish_act / eg3d_torgb_dgrad_act take linear and lrelu): those forms run the case as lrelu."""
        return 'lrelu' if self.act == 'relu' and form != 'plain' else self.act


ACT_MULTI = (ActCase(1024, 3, 37, 37, noise='image'),
             ActCase(512, 4, 45, 47, clamp=True, noise='shared', start=False),
             ActCase(160, 8, 57, 57, act='linear', noise='image'),
             ActCase(64, 16, 65, 65, clamp=True, noise='shared', d=False, bias=False),
             ActCase(12, 64, 74, 74, noise='shared'),
             ActCase(4, 128, 91, 91, act='relu', noise='image', start=False))
ACT_SMALL = (ActCase(64, 2, 9, 11, clamp=True, noise='image'),
             ActCase(12, 3, 9, 11, act='linear', clamp=True, noise='shared'),
             ActCase(4, 1, 3, 5, act='relu', noise='none'),
             ActCase(256, 2, 1, 1, noise='image'),
             ActCase(64, 2, 16, 16, noise='shared', start=False))                 # HW = 4 ppb bx exactly
ACT_CASES = ACT_MULTI + ACT_SMALL
ACT_FORMS = ('plain', 'finish', 'torgb')
ACT_CLASSES = ('idle threads', 'pixel wider than a wave', 'one pixel', 'single partial trip', 'single full trip', 'two trips, ragged last',
               '1024 pixel lanes', 'channel limit')
SLOPES = dict(linear=1.0, lrelu=ALPHA, relu=0.0)


def act_inputs(case, form):
    """fp32 inputs of one (case, form) by the recipe of the margin condition: a cotangent whose mean is away from zero (1 + 0.5 randn, or the finish
    forms' equivalents), out = 1.5 randn (clipped to +-clamp when the clamp is on, as a forward would leave it: many outputs exactly at the clamp),
    d = 0.5 + rand, bias = 0.1 randn, strength 0.37, gain sqrt 2, alpha 0.2."""
    c = case
    rng = np.random.default_rng(_seed('act', c.C, c.N, c.H, c.W, form))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)          # noqa: E731
    randn = lambda sh: rng.standard_normal(sh, dtype=np.float32)          # noqa: E731
    N, HW, C = c.N, c.HW, c.C
    out = np.float32(1.5) * randn((N, HW, C))
    if c.clamp:
        out = np.clip(out, -np.float32(CLAMP), np.float32(CLAMP))
    x = dict(out=f(out), d=f(0.5 + rng.random((N, C))) if c.d else None, bias=f(0.1 * rng.standard_normal(C)) if c.bias else None, noise=None)
    if c.noise != 'none':
        x['noise'] = f(rng.standard_normal((1 if c.noise == 'shared' else N, HW)))
    if form == 'plain':
        x['dout'] = np.float32(1.0) + np.float32(0.5) * randn((N, HW, C))
    else:
        x['s'] = f(0.75 + 0.5 * rng.random((N, C)))
        x['addend'] = np.float32(0.1) * randn((N, HW, C))
        if form == 'finish':
            x['z'] = np.float32(1.0) + np.float32(0.5) * randn((N, HW, C))
        else:
            x['dy4'] = f(1.0 + 0.5 * rng.standard_normal((N, HW, 4)))
            x['wa4'] = f((0.5 + rng.random((C, 4))) / 4.0)
    return x


def act_grad(x, form):
    if form == 'plain':
        return grad_plain(x['dout'])
    if form == 'finish':
        return grad_finish(x['z'], x['s'], x['addend'])
    return grad_torgb(x['dy4'], x['wa4'], x['s'], x['addend'])


def act_settings(case, form):
    act = case.act_of(form)
    return dict(strength=STRENGTH if case.noise != 'none' else 0.0, slope=SLOPES[act], gain=GAIN, clamp=CLAMP if case.clamp else -1.0, relu=act == 'relu')


def act_start(case, form, ref0, seed=7):
    """Starting values of the accumulated targets, either sign: a tenth of the typical size of the float64 result, and at least twenty of its derived
    tolerances (dstrength is a cancelling sum: a tenth of its value can be below one), so that an overwriting kernel shows; zero when the case says so.
    ref0 is the reference from zero; nothing here comes from a kernel."""
    if not case.start:
        return {}
    rng = np.random.default_rng(seed)
    st = {}
    for k in ('dbias', 'dd', 'dnoise', 'dstrength', 'ds'):
        if k in ref0:
            v = np.asarray(ref0[k], dtype=np.float64)
            scale = max(0.1 * float(np.median(np.abs(v))), 20.0 * float(np.median(ref0['tol_' + k]))) + 1e-3
            st[k] = (rng.choice([-1.0, 1.0], v.shape) * rng.uniform(0.5, 1.5, v.shape) * scale).astype(np.float32)
    return st


_ACT = {}


def act_case_ref(case, form):
    """(inputs, start, reference) of a listed case, computed once for the tests that follow each other on it and left unchanged."""
    assert case in ACT_CASES and form in ACT_FORMS
    k = (case.id, form)
    if k not in _ACT:
        while len(_ACT) >= len(ACT_FORMS):            # the forms of one case at a time: a multi-trip case holds a few hundred MB of float64 terms
            _ACT.pop(next(iter(_ACT)))
        x = act_inputs(case, form)
        G = act_grad(x, form)
        t = act_terms(G, x['out'], d=x['d'], bias=x['bias'], noise=x['noise'], **act_settings(case, form))
        start = act_start(case, form, act_reduce(t))
        _ACT[k] = (x, start, act_reduce(t, start), t)
    return _ACT[k][:3]


def act_case_terms(case, form):
    """act_terms of a listed case (for the mutants of the CPU file)."""
    act_case_ref(case, form)
    return _ACT[(case.id, form)][3]


# ---------------------------------------------------------------------------------------------------------------- cases: the other kernels
# dgrad_finish: (C, N, H, W, with ds, with s, with addend); every channel class, two trips with a ragged last one by the 8 ppb arithmetic
FINISH_CASES = ((1024, 2, 9, 9, True, True, True), (512, 3, 11, 13, True, False, True), (160, 2, 17, 19, True, True, False), (64, 3, 33, 35, False, True, True),
                (64, 3, 33, 35, True, True, True), (12, 2, 37, 41, True, True, True), (4, 3, 70, 70, True, False, False), (4, 1, 1, 1, True, True, True))
# demodulation: (Co, Ck, N); weight_sqsum: (Co, Ck, T)
DEMOD_CASES = ((1, 1, 1), (15, 63, 3), (16, 64, 1), (33, 65, 3), (257, 200, 1), (512, 512, 3))
SQSUM_CASES = ((15, 63, 9), (33, 65, 1), (257, 200, 9))
# weight_grad_finish: (O, I, T, N, with dd, nslab, extra slab stride)
WGF_CASES = ((5, 1, 9, 1, True, 1, 0), (7, 3, 4, 3, True, 1, 0), (4, 255, 1, 3, True, 1, 0), (3, 256, 9, 1, True, 1, 0), (6, 257, 4, 3, True, 1, 0),
             (2, 512, 9, 3, False, 1, 0), (2, 1024, 9, 1, True, 1, 0), (5, 257, 4, 3, True, 3, 37), (1, 3, 1, 3, True, 3, 5))
WGF_BATCH = (8, 0, 3, 1, 5)                         # indices into WGF_CASES of the batched launch's five items (the first has O = 1)
WGF_TOO_LARGE = (2, 2048, 9, 1)                     # (O, I, T, N): T (I + 1) + I floats of LDS exceed 64 KB
# unpack_weight_grad: (O, I, Ip, T, with scale, with da)
UNPACK_CASES = ((1, 3, 3, 1, False, False), (5, 3, 8, 9, True, True), (5, 64, 64, 9, True, True), (1, 64, 69, 1, True, False), (5, 300, 305, 9, False, True),
                (1, 300, 300, 1, True, True), (5, 300, 305, 1, True, True))
# forward: (name, N, C, H, W (output), filter kind, pad0, noise, clamp, act)
FIR44 = np.outer([1, 3, 3, 1], [1, 3, 3, 1]).astype(np.float32) / 64.0
FIR44N = (np.outer([1, 3, 3, 1], [1, 3, 3, 1]) + np.arange(16).reshape(4, 4) / 4.0).astype(np.float32) / 64.0          # not symmetric: the flip shows
FIR32 = np.array([[0.5, -0.25], [0.125, 1.0], [0.75, 0.0625]], dtype=np.float32)
FILTERS = dict(none=None, fir44=FIR44, fir44n=FIR44N, fir32=FIR32)
FWD_CASES = (('no filter', 3, 12, 5, 7, 'none', 0, 'shared', True, 'lrelu'),
             ('no filter, relu', 1, 64, 3, 3, 'none', 0, 'image', False, 'relu'),
             ('4x4 even', 1, 64, 8, 6, 'fir44n', 1, 'image', True, 'lrelu'),
             ('4x4 even pad 2', 3, 4, 4, 6, 'fir44n', 2, 'shared', False, 'linear'),
             ('4x4 even pad 0', 3, 12, 2, 4, 'fir44', 0, 'image', False, 'lrelu'),
             ('4x4 odd H', 3, 12, 7, 6, 'fir44n', 1, 'image', True, 'lrelu'),
             ('4x4 odd W pad 0', 1, 4, 4, 5, 'fir44n', 0, 'shared', False, 'lrelu'),
             ('4x4 odd pad 2', 3, 64, 5, 5, 'fir44', 2, 'none', False, 'lrelu'),
             ('3x2 pad 1', 3, 4, 6, 5, 'fir32', 1, 'image', False, 'lrelu'),
             ('3x2 pad 0', 1, 12, 4, 7, 'fir32', 0, 'shared', True, 'linear'),
             ('3x2 pad 2', 3, 64, 5, 4, 'fir32', 2, 'image', False, 'lrelu'),
             ('second lap', 1, 128, 192, 192, 'none', 0, 'shared', True, 'lrelu'))
UPCONV_CASE = ('strip, ragged', 2, 64, 13, 21, 'fir44', 1, 'image', True, 'lrelu')


def fwd_inputs(case):
    name, N, C, H, W, kind, pad0, noise, clamp, act = case
    rng = np.random.default_rng(_seed('fwd', N, C, H, W, kind, pad0))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)          # noqa: E731
    fir = FILTERS[kind]
    fh, fw = fir.shape if fir is not None else (1, 1)
    hz, wz = H - 2 * pad0 + fh - 1, W - 2 * pad0 + fw - 1
    x = dict(z=f(rng.standard_normal((N, hz, wz, C))), d=f(0.5 + rng.random((N, C))), bias=f(0.1 * rng.standard_normal(C)), fir=fir, noise=None)
    if noise != 'none':
        x['noise'] = f(rng.standard_normal((1 if noise == 'shared' else N, H, W)))
    kw = dict(pad0=pad0, fir_gain=4.0 if fir is not None else 1.0, strength=STRENGTH if noise != 'none' else 0.0, slope=SLOPES[act], gain=GAIN,
              clamp=CLAMP if clamp else -1.0)
    return x, kw


def finish_inputs(case):
    """fp32 inputs of one dgrad_finish case (the recipe of act_inputs; a non-zero start of ds)."""
    Cc, N, Hh, Ww, with_ds, with_s, with_add = case
    rng = np.random.default_rng(_seed('finish', case))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)          # noqa: E731
    sh = (N, Hh * Ww, Cc)
    return dict(z=f(1.0 + 0.5 * rng.standard_normal(sh)), x=f(1.0 + 0.5 * rng.standard_normal(sh)) if with_ds else None, s=f(0.75 + 0.5 * rng.random((N, Cc))) if with_s else None,
                addend=f(0.1 * rng.standard_normal(sh)) if with_add else None, start=f(3.0 + rng.standard_normal((N, Cc))) if with_ds else None)


def small_inputs(kind, case, seed=0):
    """fp32 inputs of the demodulation / weight-gradient families."""
    rng = np.random.default_rng(_seed(kind, tuple(case), seed))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)          # noqa: E731
    if kind == 'demod':
        Co, Ck, N = case
        w = rng.standard_normal((Co, 9, Ck)) / math.sqrt(9 * Ck)
        return dict(s=f(1.0 + 0.5 * rng.standard_normal((N, Ck))), wsq=f((w * w).sum(1)), dd=f(1.0 + 0.5 * rng.standard_normal((N, Co))),
                    start_ds=f(0.3 * rng.standard_normal((N, Ck))), start_dwsq=f(0.3 * rng.standard_normal((Co, Ck))))
    if kind == 'sqsum':
        Co, Ck, T = case
        return dict(wp=f(rng.standard_normal((Co, T, Ck))))
    if kind == 'wgf':
        O, I, T, N, with_dd, nslab, gap = case
        stride = O * T * I + gap
        buf = np.full((nslab, stride), np.nan, dtype=np.float32)
        buf[:, :O * T * I] = rng.standard_normal((nslab, O * T * I))
        return dict(buf=buf, slabs=buf[:, :O * T * I].reshape(nslab, O, T * I).copy(), stride=stride, w=f(rng.standard_normal((O, I, T)) / math.sqrt(I * T)),
                    s=f(1.0 + 0.5 * rng.standard_normal((N, I))), d=f(0.5 + rng.random((N, O))), dd=f(1.0 + 0.5 * rng.standard_normal((N, O))) if with_dd else None)
    if kind == 'unpack':
        O, I, Ip, T, with_a, with_da = case
        g = np.full((O, T, Ip), np.nan, dtype=np.float32)
        g[:, :, :I] = 1.0 + 0.5 * rng.standard_normal((O, T, I))
        return dict(g=g.reshape(O, T * Ip), w=f(1.0 + 0.5 * rng.standard_normal((O, I, T))), a=f(0.5 + rng.random(O)) if with_a else None)
    raise KeyError(kind)
