"""Independent float64 restatement of the style bank of csrc/style_affine.hip (eg3d_style_affine_fwd / _bwd), its derived elementwise bounds and the
case builders of tests/test_style_bank_cpu.py and tests/test_gpu_style_bank.py.  Plain numpy, float64, no autograd; nothing here calls the library.

The operations (header of csrc/style_affine.hip), per layer l with C rows, latent row wrow and, for a conv layer, wsq [Co, C]:
  F1 styles   s[n, j]   = (sum_k ws[n, wrow, k] W[j, k] wgain + b[j] bgain) post                                  contraction over D
  F2 demod    d[n, o]   = rsqrt(sum_k s[n, k]^2 wsq[o, k] + 1e-8)                                                  contraction over C
  F3 demod'   e[n, k]  += -s[n, k] sum_o dd[n, o] d[n, o]^3 wsq[o, k]          (e = dout_extra)                    contraction over Co
  F4 affine'  dws[n, wrow, k] += sum_j (dout[n, j] + e[n, j]) post W[j, k] wgain                                   contraction over C (of every layer
                                                                                                                   that shares the row)
  F5 weights  dW[j, k] = sum_n c[n, j] wgain ws[n, wrow, k],   db[j] = sum_n c[n, j] bgain,   c = (dout + e) post     contraction over N

The bound.  u = 2^-24.  A sum of K terms has, in ANY order of summation (sequential, tree, atomics in arrival order), an error of at most
(K - 1) u sum|terms| to first order (Higham, Accuracy and Stability, 4.2); every term carries a few roundings of its own (the product, the gain, post,
the bias, the coefficient's sum): 4 more.  So every output element is held to
      tol = (K + 4) u sum|terms|,
with K the number of terms that meet in the element (D, C, Co or N above; for F4 the sum of C over the layers that share the row, plus the starting
value; for F3 the starting value counts as one more term).  For F2 the same bound of the sum, relative to the sum, is halved by the square root, and
rsqrt and its rounding add 2 ulp:  tol_d = |d| ((K + 4) u sum|terms| / |sum| / 2 + 2 * 2^-23).
Nothing in the bound comes from what a kernel returns.  Each stage is referred to the inputs its kernel actually read: F2 and F3 to the fp32 styles
(and d) the forward left, F4 and F5 to the fp32 e the demodulation backward left -- so no bound has to carry another stage's error.
The deterministic build adds values as fixed-point numbers with bit 0 = 2^-90 and truncates below it: K 2^-90 more.
"""
import numpy as np

U = 2.0 ** -24
ULP = 2.0 ** -23
DET_QUANTUM = 2.0 ** -90
STYLE_BANK_MAX = 32


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def affine_fwd_ref(ws, W, b, wrow, wgain, bgain, post):
    """F1 -> (s [N, C], tol)."""
    x, W = _f64(ws)[:, wrow, :], _f64(W)
    D = W.shape[1]
    wg, bg, po = (float(np.float32(v)) for v in (wgain, bgain, post))
    acc = x @ (W * wg).T
    mag = np.abs(x) @ np.abs(W * wg).T
    if b is not None:
        acc = acc + _f64(b)[None] * bg
        mag = mag + np.abs(_f64(b))[None] * abs(bg)
    return acc * po, (D + 4) * U * mag * abs(po)


def demod_fwd_ref(s, wsq):
    """F2 from the fp32 styles s [N, C] -> (d [N, Co], tol)."""
    s2, wsq = _f64(s) ** 2, _f64(wsq)
    C = wsq.shape[1]
    acc = s2 @ wsq.T + float(np.float32(1e-8))
    mag = s2 @ np.abs(wsq).T + 1e-8
    d = 1.0 / np.sqrt(acc)
    return d, np.abs(d) * ((C + 4) * U * mag / np.abs(acc) / 2 + 2 * ULP)


def demod_bwd_ref(s, d, dd, wsq, e0, det=False):
    """F3 from the fp32 s, d -> (e [N, C] after the call, tol)."""
    s, d, dd, wsq, e0 = (_f64(a) for a in (s, d, dd, wsq, e0))
    Co = wsq.shape[0]
    c = dd * d * d * d
    add = -s * (c @ wsq)
    mag = np.abs(s) * (np.abs(c) @ np.abs(wsq)) + np.abs(e0)
    return e0 + add, (Co + 1 + 4) * U * mag + (Co * DET_QUANTUM if det else 0.0)


def coef_ref(dout, e, post, shape):
    """c = (dout + e) post of F4 / F5 (either may be None) and |dout| + |e| scaled the same way."""
    c, m = np.zeros(shape), np.zeros(shape)
    for a in (dout, e):
        if a is not None:
            c, m = c + _f64(a), m + np.abs(_f64(a))
    po = float(np.float32(post))
    return c * po, m * abs(po)


def affine_bwd_ref(case, es, dws0, det=False):
    """F4 over the whole bank, from the fp32 e the demodulation backward left (es: per layer array or None) -> (dws [N, L, D], tol)."""
    dws0 = _f64(dws0)
    out, mag, K = dws0.copy(), np.abs(dws0), np.ones(case['L'])
    for ly, e in zip(case['layers'], es):
        if ly['dout'] is None and e is None:
            continue
        c, m = coef_ref(ly['dout'], e, ly['post'], (case['N'], ly['C']))
        Wg = _f64(ly['W']) * float(np.float32(ly['wgain']))
        out[:, ly['wrow'], :] += c @ Wg
        mag[:, ly['wrow'], :] += m @ np.abs(Wg)
        K[ly['wrow']] += ly['C']
    return out, (K[None, :, None] + 4) * U * mag + (K[None, :, None] * DET_QUANTUM if det else 0.0)


def wgrad_ref(case, ly, e):
    """F5 of one layer -> (dW [C, D], tol, db [C], tol)."""
    N = case['N']
    c, m = coef_ref(ly['dout'], e, ly['post'], (N, ly['C']))
    x = _f64(case['ws'])[:, ly['wrow'], :]
    wg, bg = float(np.float32(ly['wgain'])), float(np.float32(ly['bgain']))
    return (c.T @ x) * wg, (N + 4) * U * (m.T @ np.abs(x)) * abs(wg), c.sum(0) * bg, (N + 4) * U * m.sum(0) * abs(bg)


def ratio(got, ref, tol):
    """Largest err / tol; NaN and a non-zero error under a zero bound count as infinite."""
    got, ref, tol = (_f64(a) for a in (got, ref, tol))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    r = np.nan_to_num(r, nan=np.inf, posinf=np.inf)
    return float(r.max()) if r.size else 0.0


def check(case, got, det=False):
    """got: what one forward, one backward and (optionally) one Phase B backward of the case left, all fp32 arrays:
         s[l], d[l] (None without demodulation), e[l] (dout_extra after the backward, None where the layer has none), dws,
         and optionally eB[l], dW[l], db[l] of a backward with dws = None.
    Returns {output group: worst err / tol}."""
    worst = dict(s=0.0, d=0.0, e=0.0, dws=0.0, dW=0.0, db=0.0)
    for i, ly in enumerate(case['layers']):
        ref, tol = affine_fwd_ref(case['ws'], ly['W'], ly['b'], ly['wrow'], ly['wgain'], ly['bgain'], ly['post'])
        worst['s'] = max(worst['s'], ratio(got['s'][i], ref, tol))
        if ly['wsq'] is not None:
            ref, tol = demod_fwd_ref(got['s'][i], ly['wsq'])
            worst['d'] = max(worst['d'], ratio(got['d'][i], ref, tol))
        for key in ('e', 'eB'):
            if ly['dd'] is not None and key in got:
                ref, tol = demod_bwd_ref(got['s'][i], got['d'][i], ly['dd'], ly['wsq'], ly['e0'], det)
                worst['e'] = max(worst['e'], ratio(got[key][i], ref, tol))
        if 'dW' in got:
            rW, tW, rb, tb = wgrad_ref(case, ly, got['eB'][i])
            if got['dW'][i] is not None:
                worst['dW'] = max(worst['dW'], ratio(got['dW'][i], rW, tW))
            if got['db'][i] is not None:
                worst['db'] = max(worst['db'], ratio(got['db'][i], rb, tb))
    ref, tol = affine_bwd_ref(case, got['e'], case['dws0'], det)
    worst['dws'] = ratio(got['dws'], ref, tol)
    return worst


# ---------------------------------------------------------------------------------------------------------------- a model of the kernels, and its mutants
MUTANTS = ('drop_last_row', 'drop_last_k_quad', 'drop_last_o', 'swap_post_wgain', 'ignore_dout_extra', 'neighbour_wrow')


def _r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def model(case, mutant=None):
    """The bank computed in float64 and rounded to fp32 where a kernel stores -- far inside every bound -- with one of MUTANTS applied: what `check`
    must reject.  Returns the `got` dict of check(), Phase B included."""
    N, L, D = case['N'], case['L'], case['D']
    got = dict(s=[], d=[], e=[], eB=[], dW=[], db=[])
    dws = _f64(case['dws0']).copy()
    kD = D - 4 if mutant == 'drop_last_k_quad' else D
    for ly in case['layers']:
        C, W = ly['C'], _f64(ly['W'])
        wg, bg, po = (float(np.float32(ly[k])) for k in ('wgain', 'bgain', 'post'))
        if mutant == 'swap_post_wgain':
            wg, po = po, wg
        x = _f64(case['ws'])[:, ly['wrow'], :]
        s = (x[:, :kD] @ W[:, :kD].T) * wg
        if ly['b'] is not None:
            s = s + _f64(ly['b'])[None] * bg
        s = s * po
        if mutant == 'drop_last_row':
            s[:, C - 1] = 0.0
        s = _r32(s)
        got['s'].append(s)
        d = None
        if ly['wsq'] is not None:
            wsq = _f64(ly['wsq'])
            d = 1.0 / np.sqrt(_f64(s) ** 2 @ wsq.T + 1e-8)
            if mutant == 'drop_last_o':
                d[:, -1] = 0.0
            d = _r32(d)
        got['d'].append(d)
        e = None
        if ly['dd'] is not None:
            c = _f64(ly['dd']) * _f64(d) ** 3
            if mutant == 'drop_last_o':
                c[:, -1] = 0.0
            e = _r32(_f64(ly['e0']) - _f64(s) * (c @ wsq))
        got['e'].append(e)
        got['eB'].append(e)
        if ly['dout'] is None and e is None:
            got['dW'].append(None)
            got['db'].append(None)
            continue
        c, _ = coef_ref(ly['dout'], None if mutant == 'ignore_dout_extra' else e, 1.0, (N, C))
        c = c * po
        cr = c.copy()
        if mutant == 'drop_last_row':
            cr[:, C - 1] = 0.0
        add = (cr @ W) * wg
        if mutant == 'drop_last_k_quad':
            add[:, D - 4:] = 0.0
        dws[:, (ly['wrow'] + 1) % L if mutant == 'neighbour_wrow' else ly['wrow'], :] += add
        got['dW'].append(_r32((c.T @ x) * wg))
        got['db'].append(_r32(c.sum(0) * bg))
    got['dws'] = _r32(dws)
    return got


def applies(case, mutant):
    """Whether the mutant changes anything the case can see."""
    lys = case['layers']
    if mutant == 'drop_last_o':
        return any(ly['wsq'] is not None for ly in lys)
    if mutant == 'ignore_dout_extra':
        return any(ly['dd'] is not None for ly in lys)
    if mutant == 'neighbour_wrow':
        return case['L'] > 1
    return True            # (every layer of every case has a bias, so exchanged gains show in F1 and in db)


# ---------------------------------------------------------------------------------------------------------------- case builders
def make_case(name, N, L, D, layers, seed=0):
    """layers: list of (C, Co | None, wrow, mode) with mode 'dout', 'extra' (dd but no dout: conv layers only) or 'both'.  Every tensor fp32; dws and
    every dout_extra start from non-zero values; gains differ from one another."""
    rng = np.random.default_rng(seed)

    def rn(*shape, scale=1.0):
        return (scale * rng.standard_normal(shape)).astype(np.float32)
    case = dict(name=name, N=N, L=L, D=D, ws=rn(N, L, D), dws0=rn(N, L, D), layers=[])
    for i, (C, Co, wrow, mode) in enumerate(layers):
        assert 0 <= wrow < L and (Co is not None or mode == 'dout')
        ly = dict(C=C, Co=Co, wrow=wrow, W=rn(C, D), b=(1.0 + 0.25 * rng.standard_normal(C)).astype(np.float32),
                  wgain=1.0 / np.sqrt(D), bgain=0.75 + 0.5 * (i % 2), post=(1.0, 1.0 / np.sqrt(C + 1.0), 1.5)[i % 3],
                  wsq=None, dd=None, e0=None, dout=rn(N, C) if mode in ('dout', 'both') else None)
        if Co is not None:
            ly['wsq'] = (rng.standard_normal((Co, C)) ** 2 * 9.0 / 4.0).astype(np.float32)
            if mode in ('extra', 'both'):
                ly['dd'], ly['e0'] = rn(N, Co), rn(N, C)
        case['layers'].append(ly)
    return case


FWD_TILE_C = (3, 4, 5, 15, 16, 17)                 # forward: 4 rows a wave, 16 a block
BWD_TILE_C = (15, 16, 17, 63, 64, 65)              # affine backward: 16 rows a row group, 64 a block
ALWAYS_C = (1, 3, 5, 33, 512)
OSPLIT_CO = (1, 15, 16, 17, 255, 256, 257, 272)
TILE_CO = (3, 4, 5, 7, 8, 9, 31, 32, 33)           # demodulation: forward 4 rows a wave / 16 a block, backward 8 a row group / 32 a block
DEMOD_C = (63, 64, 65)
DEMOD_K = (127, 128, 129, 508, 511, 512, 513, 516)  # the k chunk of a demodulation block: 512 floats in 16-byte loads, 128 in 4-byte ones
MODES = ('both', 'dout', 'extra')


def _mixed(n, L, rng_seed):
    """n layers mixing conv layers (every mode) and toRGB-like ones over L latent rows."""
    rng = np.random.default_rng(rng_seed)
    out = []
    for i in range(n):
        C = int(rng.choice((5, 16, 33, 64, 65)))
        if i % 3 == 2:
            out.append((C, None, i % L, 'dout'))
        else:
            out.append((C, int(rng.choice((1, 15, 17, 32))), i % L, MODES[i % 4 % 3]))
    return out


def cases():
    """Every case of the two test files, built once and left unchanged."""
    if _CASES:
        return _CASES
    out = []
    small = [(5, 17, 0, 'both'), (33, None, 0, 'dout'), (64, 15, 0, 'extra')]
    for D in (4, 260, 512):
        for N in (1, 2, 3):
            for L in (1, 14):
                lys = [(C, Co, (3 * i + 1) % L, m) for i, (C, Co, _, m) in enumerate(small)]
                out.append(make_case(f'D {D} N {N} L {L}', N, L, D, lys, seed=len(out)))
    cs = sorted(set(FWD_TILE_C + BWD_TILE_C + ALWAYS_C))
    out.append(make_case('C at the tile edges', 2, 14, 512, [(C, None, i % 14, 'dout') for i, C in enumerate(cs)], seed=101))
    cos = sorted(set(OSPLIT_CO + TILE_CO))
    for C in DEMOD_C:
        out.append(make_case(f'Co at the tile and osplit edges, C {C}', 2, 14, 260, [(C, Co, i % 14, MODES[i % 3]) for i, Co in enumerate(cos)], seed=110 + C))
    out.append(make_case('demodulated C at the k-chunk edges', 2, 1, 512, [(C, 33, 0, MODES[i % 3]) for i, C in enumerate(DEMOD_K)], seed=120))
    for n in (1, 3, 26, STYLE_BANK_MAX):
        for L in (1, 14):
            out.append(make_case(f'bank of {n}, L {L}', 2, L, 260, _mixed(n, L, n), seed=130 + n + L))
    out.append(make_case('two layers share a row', 3, 14, 512, [(33, 17, 5, 'both'), (65, None, 5, 'dout'), (16, 16, 6, 'extra')], seed=140))
    # one quad past the 512 columns a forward wave holds in registers and a backward block takes per chunk
    out.append(make_case('D 516, past the column chunk', 2, 3, 516, [(17, 9, 0, 'both'), (65, None, 1, 'dout'), (4, 33, 2, 'extra')], seed=150))
    _CASES.extend(out)
    return _CASES


_CASES = []
