"""Independent float64 restatement of the four kernels of csrc/torgb_small.hip -- torgb_small_kernel<4 | 8>, torgb_mid_kernel<KS, ADD, FILL> (twelve
instances), torgb_small_bwd_kernel and torgb_mid_bwd_kernel -- the launch arithmetic of their host code, derived error bounds, mutants and the case
lists of tests/test_torgb_cpu.py and tests/test_gpu_torgb.py.  Plain numpy, float64; nothing here calls the library.  The activation arithmetic, the
comparison and u come from epilogue_ref.

Layout: activations [N, HW, C] (NHWC, pixels flattened), the half-resolution addend [N, H/2, W/2, Cp], w [Cp, C], wa [C, Cp] = w^T, styles [N, C].

The operations (networks_stylegan2.py:338-359, 433-436)
  forward   out = clamp(sum_c x s[n,c] w[o,c] + bias[o]) + addend;  addend absent | [N, HW, Cp] | the half-resolution image through up2_at's expression
            wy0 (wx0 A + wx1 B) + wy1 (wx0 C + wx1 D):  taps t = (0.25, 0.75, 0.75, 0.25), (w0, w1) = (t3, t1) at an even coordinate, (t2, t0) at an odd
            one, A .. D the 2 x 2 neighbours from row (y >> 1) - 1 + (y & 1) on, zero outside the image.  The clamp comes before the addend.
  pre       x = clamp(gain pwl(z d + noise strength + bias)) in epilogue_fwd_kernel's order (epilogue_ref.fwd_ref without a filter); x is written,
            max|x| committed (atomic max onto the start value) and the forward runs on x.
  backward  zz = sum_o dy wa;  g = zz s + addend add_scale (ones when absent);  ds[n,c] += sum_p zz xin;  add_ds[n,c] += sum_p addend xin (UNscaled);
            dx = g, or with act_on g goes through epilogue_ref.act_bwd_ref (dz, dbias, dd, dnoise, dstrength, max|dz|; xin is that layer's output).

The bounds.  u = 2^-24; no constant comes from a kernel's output.  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain (one rounding per product-and-add,
no wider accumulation), so a wave's share of m channels is an m-term fma chain over a = fl(x s): (m + 1) u sum|a w| for the chain (epilogue_ref's rule
for an fma dot) and u sum|x s w| for the rounding of a.
  F  forward.  S = sum_c |x s w|.  m = the longest share (small: 8 max(g1 - g0); mid: C / KS);  the partial-sum tree has `levels` = 2 (NW = 4), 3 (NW = 8),
     1 (KS = 2), 0 (KS = 1) additions;  the bias add is one more:      e_v = (m + 3 + levels) u (S + |bias|).
     The clamp is non-expansive.  The up-sampled addend: inner products, inner sum, outer product, outer sum -- three levels of products and sums, a term
     passes through at most four roundings:  e_a = 4 u sum|wy wx A|  (the full-resolution addend is an input: 0).  The final add: u |out|.
         tol_out = e_v + e_a + u |out|     (+ sum_c e_x |s w| with `pre`, e_x = bound F of epilogue_ref on x;  max|x| within the largest e_x).
  B  backward.  Szz = sum_o |dy wa|;  m = 8 max share of the Cp / 8 groups over four waves and 2 tree levels (small), m = Cp and no tree (mid):
         e_zz = (m + 1 + levels) u Szz;      g: two products and the add:   e_g = |s| e_zz + 2 u (|zz s| + |addend add_scale|).
     Column sums (ds, add_ds, dbias, dd), depths read off the loops:
       small: the 32 rows of a tile in sequence, then one atomic per tile of the image:             D_img = 32 + tiles,       D_ch = 32 + N tiles;
       mid:   a lane adds 4 rows per tile over the wave's iterations, three shuffle levels, two levels over the waves, one atomic per block of the plane:
                                                                                                  D_img = 4 iters + 5 + gx,  D_ch = 4 iters + 5 + gx N.
       ds: (D_img + 1) u (sum|zz xin| + |start|) + sum e_zz |xin|;     add_ds: (D_img + 1) u (sum|addend xin| + |start|).
     With act_on the formulas E and R of epilogue_ref hold with these depths: the pixel's channel sum is 2 levels in the unit and 3 over the 8 lanes of a
     row (grp = 8), then one atomic per 32-channel tile (C / 32 per image);  dstrength: small -- the 32 rows of a block meet in one LDS word in sequence
     (leaders = 32), one atomic per block (N tiles C / 32);  mid -- 4 iters terms per lane, six shuffle and two wave levels (leaders = 8), gx N C / 32 atomics.
     max|dx| / max|dz| within the largest element tolerance.
"""
import numpy as np

import epilogue_ref as E
from epilogue_ref import U, cdiv, compare, margin, _f64, _seed      # noqa: F401

TS_PIX, TS_OUT, TS_BATCH = 32, 32, 8
TAPS = (0.25, 0.75, 0.75, 0.25)
SMALL_MAX_PIX = 4096                        # hipops.TORGB_SMALL_MAX_PIX / _BWD_MAX_PIX: beyond it the wrappers launch only the streaming form
ADD_IDS = dict(none=0, full=1, half=2)
GAIN, ALPHA, STRENGTH, CLAMP = E.GAIN, E.ALPHA, E.STRENGTH, E.CLAMP
FWD_MUTANTS = ('wave_dropped', 'last_group_dropped', 'last_row_dropped', 'second_iteration_dropped', 'ks_partner_dropped', 'bias_after_clamp',
               'addend_before_clamp', 'parity_swapped', 'border_clamped', 'image0_low', 'noise_without_strength', 'amax_missing_wave')
BWD_MUTANTS = ('wave_dropped', 'last_group_dropped', 'last_row_dropped', 'second_iteration_dropped', 'add_scale_ignored', 'add_ds_scaled')


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def launch_fwd(N, C, H, W, Cp, add='none', pre=False):
    """eg3d_torgb_small_supported, eg3d_torgb_mid_supported, launch_torgb_mid and eg3d_torgb_small_fwd restated.  None: refused."""
    HW = H * W
    if N < 1 or H < 1 or W < 1 or C < 32 or C % 8 or Cp < TS_OUT or Cp % TS_OUT:
        return None
    if add == 'half' and (H % 2 or W % 2):
        return None
    mid = not pre and Cp == 96 and C % 32 == 0 and C <= 256 and W >= TS_PIX and HW % TS_PIX == 0 and N * HW >= 8192
    groups = C // 8
    if not mid:
        tiles = cdiv(HW, TS_PIX)
        grid = (N * tiles, Cp // TS_OUT)
        NW = 8 if groups > 4 * TS_BATCH and grid[0] * grid[1] <= 128 else 4
        shares = [(groups * w // NW, groups * (w + 1) // NW) for w in range(NW)]
        return dict(family='small', mid=False, NW=NW, shares=shares, batches=[cdiv(b - a, TS_BATCH) for a, b in shares], tiles=tiles, grid=grid, ADD=ADD_IDS[add],
                    m=8 * max(b - a for a, b in shares), levels=2 if NW == 4 else 3, wrapper_takes=N * HW <= SMALL_MAX_PIX)
    T = N * HW // TS_PIX
    ks2 = T < 1024 and C % 64 == 0
    smem = 96 * (C + 4) * 4 + 2 * 48 * 64 * 4 + 4096
    per_cu = max(1, (160 * 1024) // (smem + 1024))
    tpb = 2 if ks2 else 4
    blocks = min(cdiv(T, tpb), 256 * min(per_cu, 2))
    stride = blocks * tpb
    iters = cdiv(T, stride)
    KS = 2 if ks2 else 1
    ng = groups // KS
    return dict(family='mid', mid=True, KS=KS, ADD=ADD_IDS[add], FILL=24 if C > 128 else 12, nb=96 * (C // 4) // 256, smem=smem, per_cu=per_cu, blocks=blocks,
                T=T, tpi=HW // TS_PIX, stride=stride, iters=iters, valid_last=T - (iters - 1) * stride, shares=[(k * ng, (k + 1) * ng) for k in range(KS)],
                m=C // KS, levels=KS - 1, straddle=W % TS_PIX != 0, wrapper_takes=True)


def launch_bwd(N, C, H, W, Cp):
    """eg3d_torgb_small_bwd_supported, eg3d_torgb_mid_bwd_supported and eg3d_torgb_small_bwd restated, with the reduction depths of header B."""
    HW = H * W
    if N < 1 or H < 1 or W < 1 or Cp < 8 or Cp % 8 or C < TS_OUT or C % TS_OUT:
        return None
    mid = Cp == 96 and HW % TS_PIX == 0 and N <= 65535 and N * HW >= 4096
    groups = Cp // 8
    ct = C // TS_OUT
    if not mid:
        tiles = cdiv(HW, TS_PIX)
        shares = [(groups * w // 4, groups * (w + 1) // 4) for w in range(4)]
        return dict(family='small', mid=False, shares=shares, wave_iters=[cdiv(b - a, TS_BATCH) for a, b in shares], tiles=tiles, grid=(N * tiles, ct),
                    m=8 * max(b - a for a, b in shares), levels=2, wrapper_takes=N * HW <= SMALL_MAX_PIX,
                    D_img=32 + tiles, D_ch=32 + N * tiles, C4=C // 4, grp=8, pow2=True, trips=0, leaders=32, bx=tiles * ct)
    tpi = HW // TS_PIX
    gx = max(1, min(cdiv(tpi, 4), 512 // max(1, ct * N)))
    tstep = gx * 4
    wave_iters = [cdiv(tpi - w, tstep) if w < tpi else 0 for w in range(tstep)]
    iters = max(wave_iters)
    return dict(family='mid', mid=True, shares=[(0, groups)], tpi=tpi, grid_mid=(gx, ct, N), tstep=tstep, wave_iters=wave_iters, iters=iters, m=Cp, levels=0,
                wrapper_takes=True, D_img=4 * iters + 5 + gx, D_ch=4 * iters + 5 + gx * N, C4=C // 4, grp=8, pow2=True, trips=iters, leaders=8, bx=gx * ct)


def classes(kind, N, C, H, W, Cp, add='none', pre=False):
    """The launch classes of one case; kind 'fwd' | 'bwd'."""
    HW, out = H * W, set()
    if kind == 'fwd':
        L = launch_fwd(N, C, H, W, Cp, add, pre)
        if L['family'] == 'small':
            out |= {f'NW = {L["NW"]}', f'{max(L["batches"])} batch(es)', 'small forward'}
            if any((b - a) % TS_BATCH for a, b in L['shares']):
                out.add('partly filled batch')
            if HW == 1:
                out.add('one pixel')
            if HW == TS_PIX:
                out.add('one full tile')
            if HW % TS_PIX and HW > TS_PIX:
                out.add('ragged last tile')
            if N > 1:
                out.add('N > 1, small forward')
            if add == 'half' and N > 1 and HW % TS_PIX:
                out.add('half-resolution addend, N > 1, ragged')
            if pre:
                out.add('pre')
        else:
            out |= {f'mid <{L["KS"]}, {L["ADD"]}, {L["FILL"]}>', 'mid forward'}
            if L['iters'] == 2 and 0 < L['valid_last'] < L['stride']:
                out.add(f'two iterations, partly valid last, KS = {L["KS"]}')
            if L['straddle']:
                out.add('tile straddles a row')
            if N > 1:
                out.add(f'N > 1, mid forward, KS = {L["KS"]}')
            if L['FILL'] == 24 and L['nb'] % 12 and L['nb'] < 24:
                out.add('partly filled second fill batch')
    else:
        L = launch_bwd(N, C, H, W, Cp)
        out.add(f'{L["family"]} backward')
        if N > 1:
            out.add(f'N > 1, {L["family"]} backward')
        if L['family'] == 'small':
            if any(a == b for a, b in L['shares']):
                out.add('empty wave shares')
            if L['tiles'] == 127:
                out.add('127 tiles per image')
            if HW % TS_PIX:
                out.add('ragged last tile, backward')
        else:
            if N * HW == 4096:
                out.add('exactly 4096 pixels')
            if len(set(L['wave_iters'])) > 1 and L['iters'] == 2:
                out.add('ragged wave assignment')
            if L['tpi'] % 4 == 1:
                out.add('last block with one busy wave')
            if N >= 3:
                out.add('three grid planes in z')
    return out


FWD_CLASSES = ('NW = 4', 'NW = 8', '1 batch(es)', '2 batch(es)', '3 batch(es)', 'partly filled batch', 'one pixel', 'one full tile', 'ragged last tile',
               'N > 1, small forward', 'half-resolution addend, N > 1, ragged', 'pre') + tuple(f'mid <{k}, {a}, {f}>' for k in (1, 2) for a in (0, 1, 2) for f in (12, 24)) + \
              ('two iterations, partly valid last, KS = 1', 'two iterations, partly valid last, KS = 2', 'tile straddles a row', 'N > 1, mid forward, KS = 1',
               'N > 1, mid forward, KS = 2', 'partly filled second fill batch')
BWD_CLASSES = ('small backward', 'mid backward', 'N > 1, small backward', 'N > 1, mid backward', 'empty wave shares', '127 tiles per image', 'ragged last tile, backward',
               'exactly 4096 pixels', 'ragged wave assignment', 'last block with one busy wave', 'three grid planes in z')


# ---------------------------------------------------------------------------------------------------------------- masks of the mutants
def _chan_mask(L, K, mutant):
    """Weights of the K contraction channels under a mutant of the contraction."""
    cm = np.ones(K)
    busy = [(a, b) for a, b in L['shares'] if b > a]
    if mutant == 'wave_dropped':
        a, b = busy[-1]
        cm[8 * a:8 * b] = 0
    elif mutant == 'last_group_dropped':
        for a, b in busy:
            cm[8 * (b - 1):8 * b] = 0
    elif mutant == 'ks_partner_dropped':
        cm[K // 2:] = 0
    return cm


def _pixel_mask(L, N, HW, mutant, step):
    """Weights [N, HW] of the pixels: the last row of every tile, or the tiles of the second iteration (step = first tile index of that iteration)."""
    pm = np.ones((N, HW))
    p = np.arange(HW)
    if mutant == 'last_row_dropped':
        pm[:, p % TS_PIX == TS_PIX - 1] = 0
    elif mutant == 'second_iteration_dropped':
        pm[(np.arange(N)[:, None] * step[1] + p[None, :] // TS_PIX) >= step[0]] = 0
    return pm


# ---------------------------------------------------------------------------------------------------------------- forward
def up2_ref(low, H, W, taps=TAPS, mutant=None):
    """low [N, H/2, W/2, Cp] -> (the up-sampled image [N, HW, Cp], sum |wy wx A| the same shape): up2_at's expression."""
    low = _f64(low)
    if mutant == 'image0_low':
        low = np.broadcast_to(low[:1], low.shape)
    n, hl, wl, cp = low.shape
    t = [float(v) for v in taps]
    lp = np.pad(low, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge' if mutant == 'border_clamped' else 'constant')

    def axis(size):
        i = np.arange(size)
        odd = (i & 1).astype(bool)
        if mutant == 'parity_swapped':
            odd = ~odd
        return (i >> 1) + (i & 1), np.where(odd, t[2], t[3]), np.where(odd, t[0], t[1])          # index of the first neighbour in the padded image, w0, w1

    r, wy0, wy1 = axis(H)
    c, wx0, wx1 = axis(W)
    A, B = lp[:, r][:, :, c], lp[:, r][:, :, c + 1]
    Cc, D = lp[:, r + 1][:, :, c], lp[:, r + 1][:, :, c + 1]
    wy0, wy1, wx0, wx1 = wy0[None, :, None, None], wy1[None, :, None, None], wx0[None, None, :, None], wx1[None, None, :, None]
    val = wy0 * (wx0 * A + wx1 * B) + wy1 * (wx0 * Cc + wx1 * D)
    mag = np.abs(wy0) * (np.abs(wx0 * A) + np.abs(wx1 * B)) + np.abs(wy1) * (np.abs(wx0 * Cc) + np.abs(wx1 * D))
    return val.reshape(n, H * W, cp), mag.reshape(n, H * W, cp)


def pre_ref(z, L, d=None, noise=None, strength=0.0, bias=None, slope=1.0, gain=1.0, clamp=-1.0, start=0.0, mutant=None):
    """z [N, HW, C], noise [1 or N, HW] -> (x, tol_x, max(start, max|x|), its tolerance): epilogue_fwd_kernel's arithmetic without a filter."""
    z = _f64(z)
    N, HW, C = z.shape
    nz = None if noise is None else _f64(noise).reshape(-1, HW, 1)
    x, tol, amax, tol_amax = E.fwd_ref(z.reshape(N, HW, 1, C), d=d, noise=nz, strength=1.0 if mutant == 'noise_without_strength' else strength, bias=bias,
                                       slope=slope, gain=gain, clamp=clamp)
    x, tol = x.reshape(N, HW, C), tol.reshape(N, HW, C)
    if mutant == 'amax_missing_wave':          # the share that holds the maximum does not commit
        c = int(np.argmax(np.abs(x).max((0, 1))))
        a, b = next((a, b) for a, b in L['shares'] if 8 * a <= c < 8 * b)
        keep = np.ones(C, dtype=bool)
        keep[8 * a:8 * b] = False
        amax = float(np.abs(x[:, :, keep]).max())
    return x, tol, max(float(start), amax), tol_amax


def fwd_ref(x, s, w, L, H, W, bias=None, clamp=-1.0, addend=None, add='none', e_x=None, mutant=None):
    """x [N, HW, C], s [N, C], w [Cp, >= C], addend [N, HW, Cp] (full) or [N, H/2, W/2, Cp] (half) -> dict(out, tol_out)."""
    x, s = _f64(x), _f64(s)
    N, HW, C = x.shape
    w = _f64(w)[:, :C]
    Cp = w.shape[0]
    a = x * s[:, None, :]
    cm = _chan_mask(L, C, mutant)
    acc = ((a * cm).reshape(-1, C) @ w.T).reshape(N, HW, Cp)
    if mutant in ('last_row_dropped', 'second_iteration_dropped'):
        acc = acc * _pixel_mask(L, N, HW, mutant, (L.get('stride', 0), L.get('tpi', 0)))[:, :, None]
    S = (np.abs(a).reshape(-1, C) @ np.abs(w).T).reshape(N, HW, Cp)
    b = np.zeros(Cp) if bias is None else _f64(bias)
    e_v = (L['m'] + 3 + L['levels']) * U * (S + np.abs(b))
    if e_x is not None:
        e_v = e_v + ((e_x * np.abs(s)[:, None, :]).reshape(-1, C) @ np.abs(w).T).reshape(N, HW, Cp)
    ad, e_a = 0.0, 0.0
    if add == 'full':
        ad = _f64(addend)
    elif add == 'half':
        ad, mag = up2_ref(addend, H, W, mutant=mutant)
        e_a = 4 * U * mag
    clip = (lambda v: np.clip(v, -clamp, clamp)) if clamp >= 0 else (lambda v: v)
    if mutant == 'bias_after_clamp':
        out = clip(acc) + b + ad
    elif mutant == 'addend_before_clamp':
        out = clip(acc + b + ad)
    else:
        out = clip(acc + b) + ad
    return dict(out=out, tol_out=e_v + e_a + U * np.abs(out), launch=L)


# ---------------------------------------------------------------------------------------------------------------- backward
def bwd_ref(dy, wa, s, xin, L, addend=None, add_scale=None, add_ds=False, act=None, start=None, mutant=None):
    """dy [N, HW, Cp], wa [C, >= Cp], s [N, C], xin / addend [N, HW, C], add_scale [N, C];  act: None or the keyword arguments of epilogue_ref.act_terms
    (d, bias, noise [1 or N, HW], strength, slope, gain, clamp);  start: dict of the accumulated targets' starting values.
    Returns dx | dz, amax, ds, add_ds (asked for), and with act dbias, dd, dnoise, dstrength -- each with tol_<name>."""
    dy, s, xin = _f64(dy), _f64(s), _f64(xin)
    N, HW, Cp = dy.shape
    wa = _f64(wa)[:, :Cp]
    C = wa.shape[0]
    start = start or {}
    cm = _chan_mask(L, Cp, mutant)
    zz = ((dy * cm).reshape(-1, Cp) @ wa.T).reshape(N, HW, C)
    e_zz = (L['m'] + 1 + L['levels']) * U * (np.abs(dy).reshape(-1, Cp) @ np.abs(wa).T).reshape(N, HW, C)
    a = np.zeros((1, 1, 1)) if addend is None else _f64(addend)
    asv = np.ones((1, 1, 1)) if add_scale is None or mutant == 'add_scale_ignored' else _f64(add_scale)[:, None, :]
    a_s = a * asv
    zs = zz * s[:, None, :]
    G = dict(g=zs + a_s, e_g=np.abs(s)[:, None, :] * e_zz + 2 * U * (np.abs(zs) + np.abs(a_s)), zz=zz, e_zz=e_zz)
    mask = None
    if mutant in ('last_row_dropped', 'second_iteration_dropped'):
        mask = _pixel_mask(L, N, HW, mutant, (L.get('tstep', 0), 0))
    st = lambda k: _f64(start[k]) if start.get(k) is not None else 0.0          # noqa: E731
    if act is None:
        r = dict(dx=G['g'], tol_dx=G['e_g'], amax=float(np.abs(G['g']).max()), tol_amax=float(G['e_g'].max()))
        tz = zz * xin
        r['ds'] = E._msum(tz, mask, 1) + st('ds')
        r['tol_ds'] = (L['D_img'] + 1) * U * (np.abs(tz).sum(1) + np.abs(st('ds'))) + (e_zz * np.abs(xin)).sum(1)
    else:
        t = E.act_terms(G, xin, **act)
        t['L'] = L                                   # the depths of header B in place of the activation-backward kernel's own
        q = E.act_reduce(t, start, mask)
        r = {k: v for k, v in q.items() if k != 'launch'}
        r['dx'], r['tol_dx'], r['amax'], r['tol_amax'] = r.pop('dz'), r.pop('tol_dz'), r.pop('dz_amax'), r.pop('tol_dz_amax')
    if add_ds:
        ta = (a_s if mutant == 'add_ds_scaled' else a) * xin
        r['add_ds'] = E._msum(ta, mask, 1) + st('add_ds')
        r['tol_add_ds'] = (L['D_img'] + 1) * U * (np.abs(a * xin).sum(1) + np.abs(st('add_ds')))
    r['launch'] = L
    return r


BWD_SUMS = ('ds', 'add_ds', 'dbias', 'dd', 'dnoise', 'dstrength')


# ---------------------------------------------------------------------------------------------------------------- cases: forward
class FwdCase:
    """One forward launch.  pre: None or (act, d, bias, noise, clamp, start) with noise 'none' | 'shared' | 'image' and start 'zero' | 'below' | 'above'."""

    def __init__(self, N, C, H, W, Cp, add='none', bias=True, clamp=True, wpad=0, pre=None):
        self.N, self.C, self.H, self.W, self.Cp, self.HW = N, C, H, W, Cp, H * W
        self.add, self.bias, self.clamp, self.wpad, self.pre = add, bias, clamp, wpad, pre

    @property
    def geom(self):
        return self.N, self.C, self.H, self.W, self.Cp

    @property
    def id(self):
        p = '' if self.pre is None else '-pre-' + '-'.join(str(v) for v in self.pre)
        return f'{self.N}x{self.C}x{self.H}x{self.W}x{self.Cp}-{self.add}{"-wpad" if self.wpad else ""}{p}'

    @property
    def launch(self):
        return launch_fwd(*self.geom, add=self.add, pre=self.pre is not None)


FWD_SMALL = (FwdCase(1, 32, 1, 1, 32, bias=False, clamp=False),                 # one pixel, one group per wave
             FwdCase(1, 64, 4, 8, 96, add='full', clamp=False),                # exactly one full tile
             FwdCase(2, 40, 9, 7, 96, add='full'),                             # shares 1, 1, 1, 2; ragged 63-pixel images
             FwdCase(3, 136, 6, 10, 96, add='half'),                           # half-resolution addend, N = 3, ragged tile, every border
             FwdCase(1, 264, 4, 4, 96, add='half', bias=False),                # NW = 8, shares 4 and 5
             FwdCase(1, 520, 4, 4, 96),                                        # NW = 8, the last wave has two batches, the second holding one group
             FwdCase(1, 520, 40, 36, 96, add='half'),                          # 135 blocks: NW = 4, shares 16, 16, 16, 17, three batches
             FwdCase(2, 40, 9, 7, 96, add='full', wpad=8))                     # w_row > C, NaN in the row padding
PRE_GEOMS = ((2, 40, 9, 7, 96, 'full'), (3, 136, 6, 10, 96, 'half'), (1, 264, 4, 4, 96, 'half'), (2, 64, 5, 5, 32, 'none'))
PRE_SETTINGS = (('lrelu', True, True, 'image', True, 'zero'), ('linear', False, True, 'shared', False, 'below'), ('relu', True, False, 'none', True, 'above'),
                ('lrelu', False, False, 'shared', False, 'zero'))
FWD_PRE = tuple(FwdCase(*g[:5], add=g[5], bias=i % 2 == 0, clamp=i % 2 == 1, pre=ps) for g in PRE_GEOMS for i, ps in enumerate(PRE_SETTINGS))
MID_GEOMS = ((1, 32, 64, 128), (1, 96, 208, 40), (2, 64, 104, 40), (1, 128, 64, 128), (1, 160, 64, 128), (1, 192, 64, 128), (1, 256, 128, 132), (2, 160, 130, 128))
FWD_MID = tuple(FwdCase(*g, 96, add=add, bias=(i + j) % 3 != 0, clamp=(i + j) % 2 == 0, wpad=4 if (i, j) == (4, 1) else 0)
                for i, g in enumerate(MID_GEOMS) for j, add in enumerate(('none', 'full', 'half')))
FWD_CASES = FWD_SMALL + FWD_PRE + FWD_MID
TWO_ITERS = ((1, 256, 128, 132), (2, 160, 130, 128))
SLOPES = E.SLOPES


def fwd_inputs(case):
    """fp32 inputs: x (or z with `pre`) = randn, s = 0.75 + 0.5 rand, w = randn / sqrt(C) inside a NaN-padded row buffer, bias = 0.3 randn, clamp 1.2 (about a
    fifth of the outputs at the clamp), addend randn.  pre: d = 0.5 + rand, bias 0.1 randn, noise randn, strength 0.37, gain sqrt 2, clamp 1.2."""
    c = case
    rng = np.random.default_rng(_seed('torgb fwd', c.id))
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)          # noqa: E731
    N, C, H, W, Cp = c.geom
    wbuf = np.full((Cp, C + c.wpad), np.nan, dtype=np.float32)
    wbuf[:, :C] = rng.standard_normal((Cp, C)) / np.sqrt(C)
    x = dict(x=f(rng.standard_normal((N, H * W, C))), s=f(0.75 + 0.5 * rng.random((N, C))), wbuf=wbuf, w=wbuf[:, :C], bias=f(0.3 * rng.standard_normal(Cp)) if c.bias else None,
             clamp=CLAMP if c.clamp else -1.0, addend=None)
    if c.add == 'full':
        x['addend'] = f(rng.standard_normal((N, H * W, Cp)))
    elif c.add == 'half':
        x['addend'] = f(rng.standard_normal((N, H // 2, W // 2, Cp)))
    if c.pre is not None:
        act, d, bias, noise, clamp, start = c.pre
        x['pre'] = dict(d=f(0.5 + rng.random((N, C))) if d else None, bias=f(0.1 * rng.standard_normal(C)) if bias else None,
                        noise=None if noise == 'none' else f(rng.standard_normal((1 if noise == 'shared' else N, H * W))),
                        strength=STRENGTH if noise != 'none' else 0.0, slope=SLOPES[act], gain=GAIN, clamp=CLAMP if clamp else -1.0)
    return x


def fwd_eval(case, x, mutant=None):
    """The float64 reference (or one of its mutants) of a case on the inputs x."""
    c, L = case, case.launch
    r = {}
    xin, e_x = x['x'], None
    if c.pre is not None:
        true_amax = pre_ref(x['x'], L, **x['pre'])[2]
        start = dict(zero=0.0, below=float(np.float32(0.5 * true_amax)), above=float(np.float32(2.0 * true_amax + 1.0)))[c.pre[5]]
        xin, e_x, r['x_amax'], r['tol_x_amax'] = pre_ref(x['x'], L, start=start, mutant=mutant, **x['pre'])
        r.update(x=xin, tol_x=e_x, amax_start=start)
    r.update(fwd_ref(xin, x['s'], x['w'], L, c.H, c.W, bias=x['bias'], clamp=x['clamp'], addend=x['addend'], add=c.add, e_x=e_x, mutant=mutant))
    return r


def fwd_mutants(case):
    """(mutant, must touch an output) for every mutant that applies to a case."""
    c, L = case, case.launch
    out = [('last_group_dropped', True)]
    if L['family'] == 'small':
        out.append(('wave_dropped', True))
    if c.HW >= TS_PIX:
        out.append(('last_row_dropped', True))
    if L['family'] == 'mid' and L['iters'] == 2:
        out.append(('second_iteration_dropped', True))
    if L['family'] == 'mid' and L['KS'] == 2:
        out.append(('ks_partner_dropped', True))
    if c.bias and c.clamp:
        out.append(('bias_after_clamp', c.HW * c.N >= 32))
    if c.add != 'none' and c.clamp:
        out.append(('addend_before_clamp', c.HW * c.N >= 32))
    if c.add == 'half':
        out += [('parity_swapped', True), ('border_clamped', True)]
        if c.N > 1:
            out.append(('image0_low', True))
    if c.pre is not None:
        if c.pre[3] != 'none':
            out.append(('noise_without_strength', True))
        out.append(('amax_missing_wave', not c.pre[4] and c.pre[5] != 'above'))
    return out


_CACHE = {}


def _cached(key, make, keep=3):
    if key not in _CACHE:
        while len(_CACHE) >= keep:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make()
    return _CACHE[key]


def fwd_case_ref(case):
    """(inputs, reference) of a listed case, computed once for the tests that follow each other on it and left unchanged."""
    def make():
        x = fwd_inputs(case)
        return x, fwd_eval(case, x)
    return _cached(('fwd', case.id), make)


# ---------------------------------------------------------------------------------------------------------------- cases: backward
class BwdCase:
    """One backward geometry with the settings of its act form: (act, clamp, noise, d, bias)."""

    def __init__(self, N, C, H, W, Cp, act, clamp, noise, d=True, bias=True, start=True, plain_ds=True, wpad=0):
        self.N, self.C, self.H, self.W, self.Cp, self.HW = N, C, H, W, Cp, H * W
        self.act, self.clamp, self.noise, self.d, self.bias, self.start, self.plain_ds, self.wpad = act, clamp, noise, d, bias, start, plain_ds, wpad

    @property
    def geom(self):
        return self.N, self.C, self.H, self.W, self.Cp

    @property
    def id(self):
        return 'x'.join(str(v) for v in self.geom)

    @property
    def launch(self):
        return launch_bwd(*self.geom)


BWD_FORMS = ('plain', 'scale', 'scale_ds', 'act')
BWD_CASES = (BwdCase(2, 32, 9, 7, 8, 'lrelu', True, 'shared', plain_ds=False),            # three waves with an empty share
             BwdCase(2, 160, 9, 7, 96, 'linear', False, 'image', wpad=4),
             BwdCase(1, 32, 58, 70, 96, 'lrelu', True, 'none', d=False, bias=False),      # 127 tiles per image, just under the mid threshold
             BwdCase(1, 64, 64, 64, 96, 'linear', False, 'none', start=False)  ,         # exactly 4096 pixels
             BwdCase(1, 32, 43, 96, 96, 'lrelu', True, 'image', plain_ds=False),          # 129 tiles: the last block has one busy wave
             BwdCase(3, 256, 43, 96, 96, 'lrelu', True, 'shared'))                        # two iterations per wave, ragged, three grid planes in z


def bwd_form(case, form):
    """What a form of a case passes: (addend, add_scale, add_ds, ds, act).  The act form carries add_scale and add_ds on every other case."""
    i = BWD_CASES.index(case)
    if form == 'plain':
        return dict(addend=i % 2 == 0, add_scale=False, add_ds=False, ds=case.plain_ds, act=False)
    if form == 'scale':
        return dict(addend=True, add_scale=True, add_ds=False, ds=True, act=False)
    if form == 'scale_ds':
        return dict(addend=True, add_scale=True, add_ds=True, ds=True, act=False)
    return dict(addend=True, add_scale=i % 2 == 1, add_ds=i % 2 == 1, ds=True, act=True)


def bwd_inputs(case, form):
    """fp32 inputs by the recipe of epilogue_ref.act_inputs: dy = 1 + 0.5 randn, wa = (0.5 + rand) / Cp inside a NaN-padded row buffer, xin = 1.5 randn (clipped
    to the clamp in the act form, as a forward leaves it), addend = 1 + 0.5 randn (an unfinished gradient), add_scale = 0.75 + 0.5 rand."""
    c, fm = case, bwd_form(case, form)
    rng = np.random.default_rng(_seed('torgb bwd', c.id, form))
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)          # noqa: E731
    N, C, H, W, Cp = c.geom
    HW = H * W
    wbuf = np.full((C, Cp + c.wpad), np.nan, dtype=np.float32)
    wbuf[:, :Cp] = (0.5 + rng.random((C, Cp))) / Cp
    xin = np.float32(1.5) * rng.standard_normal((N, HW, C), dtype=np.float32)
    act = None
    if fm['act']:
        if c.clamp:
            xin = np.clip(xin, -np.float32(CLAMP), np.float32(CLAMP))
        act = dict(d=f(0.5 + rng.random((N, C))) if c.d else None, bias=f(0.1 * rng.standard_normal(C)) if c.bias else None,
                   noise=None if c.noise == 'none' else f(rng.standard_normal((1 if c.noise == 'shared' else N, HW))),
                   strength=STRENGTH if c.noise != 'none' else 0.0, slope=SLOPES[c.act], gain=GAIN, clamp=CLAMP if c.clamp else -1.0)
    return dict(dy=f(1.0 + 0.5 * rng.standard_normal((N, HW, Cp))), wbuf=wbuf, wa=wbuf[:, :Cp], s=f(0.75 + 0.5 * rng.random((N, C))), xin=f(xin),
                addend=f(1.0 + 0.5 * rng.standard_normal((N, HW, C))) if fm['addend'] else None, add_scale=f(0.75 + 0.5 * rng.random((N, C))) if fm['add_scale'] else None, act=act)


def bwd_eval(case, form, x, start=None, mutant=None):
    fm = bwd_form(case, form)
    return bwd_ref(x['dy'], x['wa'], x['s'], x['xin'], case.launch, addend=x['addend'], add_scale=x['add_scale'], add_ds=fm['add_ds'], act=x['act'], start=start, mutant=mutant)


def bwd_start(case, ref0, seed=11):
    """Starting values of the accumulated targets by the rule of epilogue_ref.act_start (from the float64 reference from zero, never from a kernel)."""
    if not case.start:
        return {}
    rng = np.random.default_rng(seed)
    st = {}
    for k in BWD_SUMS:
        if k in ref0:
            v = np.asarray(ref0[k], dtype=np.float64)
            scale = max(0.1 * float(np.median(np.abs(v))), 20.0 * float(np.median(ref0['tol_' + k]))) + 1e-3
            st[k] = (rng.choice([-1.0, 1.0], v.shape) * rng.uniform(0.5, 1.5, v.shape) * scale).astype(np.float32)
    return st


def bwd_mutants(case, form):
    fm, L = bwd_form(case, form), case.launch
    out = ['last_group_dropped']
    if L['family'] == 'small':
        out.append('wave_dropped')
    if case.HW >= TS_PIX:
        out.append('last_row_dropped')
    if L['family'] == 'mid' and L['iters'] == 2:
        out.append('second_iteration_dropped')
    if fm['add_scale']:
        out.append('add_scale_ignored')
    if fm['add_ds']:
        out.append('add_ds_scaled')
    return out


def bwd_case_ref(case, form):
    """(inputs, start, reference) of a listed (case, form), computed once and left unchanged."""
    def make():
        x = bwd_inputs(case, form)
        start = bwd_start(case, bwd_eval(case, form, x))
        return x, start, bwd_eval(case, form, x, start)
    return _cached(('bwd', case.id, form), make)
