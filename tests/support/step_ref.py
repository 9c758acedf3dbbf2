"""Independent float64 restatement of the per-step kernels of csrc/noise_ops.hip (eg3d_noise_regularizer, eg3d_noise_normalize, eg3d_adam_step),
their derived elementwise error bounds and the case builders of tests/test_step_ops_cpu.py and tests/test_gpu_step_ops.py.  Plain numpy, float64,
no autograd; nothing here calls the library.

The operations
  regulariser (w_projector.py:221-237): per buffer x [res, res], levels v_0 = x, v_{l+1} = avg_pool2d(v_l, 2) while res_l > 8,
      m_l = (mean(v_l roll(v_l, 1, W)), mean(v_l roll(v_l, 1, H))),   value = scale sum_l |m_l|^2,
      d value / d x[i] = scale sum_l 4^-l 2 / n_l (mx_l (left + right) + my_l (up + down))   taken at the level-l ancestor of i.
  normalise (w_projector.py:264-270): x <- (x - mean(x)) rsqrt(mean((x - mean)^2)).
  Adam: one step of torch.optim.Adam without weight decay and amsgrad.

The bounds.  u = 2^-24 is the unit roundoff of fp32; a sum of k terms added with depth D (the largest number of additions any term passes
through) has an error of at most D u sum|terms| (first order; Higham, Accuracy and Stability, 4.2).  No constant below comes from what a kernel
returns; the depths are read off the kernels' loops.

  R1 pooled levels.  A pooled value is ((a + b) + (c + d)) / 4: three roundings, each of a sum of non-negative-weighted children, so with
     a_l = the same pyramid of |x| :  |d v_l| <= pe_l a_l,  pe_l = (1 + u)^(3 l) - 1.
  R2 level moment.  The moments pass gives a thread 4 products (4 additions), a block 10 tree steps (6 shuffles in a wave, 4 over the 16 waves) and
     one atomic per 4096-element chunk into the level's slot: depth 4 + 10 + ceil(n_l / 4096); + 1 for the product's own rounding and + 1 for the
     division by n_l in the gradient pass:  D_l = 16 + ceil(n_l / 4096)  (80 for level 0 of a 512^2 map, 272 for 1024^2).  With
     S_l = sum |v roll v| and P_l = sum a_l roll(a_l):   |d m_l| <= (D_l u (S_l + q_l P_l) + q_l P_l) / n_l,   q_l = 2 pe_l + pe_l^2   (R1 in both
     factors of a product).
  R3 value of a buffer.  m^2 terms: 2 |m| |d m| + |d m|^2 each; then mx mx + my my (2 roundings), four shuffle steps over the levels, the product
     with scale and nothing else (the atomic adds into a zero): 8 u of the value.  Several buffers in one call add through one atomic each: B u of
     the sum of the buffers' values; two launches (more than 32 buffers) one more addition.
  R4 gradient element.  Per level the coefficient c_l = scale 4^-l 2 / n_l m_l carries |d m_l| and two roundings (scale, product), the neighbour sum
     one, the product one, the sum of the two directions one and the running sum over levels at most nl:
         tol_g[i] = sum_l scale 4^-l 2 / n_l ( |d m_l| (|L| + |R|) + |m_l| pe_l (aL + aR) + (nl + 6) u |m_l| (|L| + |R|) )   + the same in y,
     with L, R the level's float64 neighbours and aL, aR those of a_l, all at the ancestor of i.
  N  normalise.  kappa = mean^2 / var.  sum x and sum x^2 with depth D:  |d mean| <= D u mean|x| <= D u sqrt(E2),  E2 = mean(x^2) = var (1 + kappa);
     the one-pass variance E2 - mean^2 has |d var| <= (D + 1) u E2 + 2 |mean| |d mean| + 3 u E2 <= (3 D + 4) u E2, i.e. relative (3 D + 4) u (1 + kappa);
     rsqrt halves it and adds two roundings (sqrt, divide), (x - mean) inv two more:
         tol[i] = |x'[i]| ((3 D + 4) u (1 + kappa) / 2 + 4 u) + D u sqrt(1 + kappa).
     The two-pass forms (variance about the computed mean) are inside the same bound.  D: one block per buffer: ceil(n / 1024) + 10 + 2; multi-block:
     8 + 10 + ceil(n / 8192) + 2; Adam's fused moments: 4 + 10 + ceil(n / 4096) + 2.
  A  Adam.  g = g1 + g2 (u |g|).  m' = m + (g - m)(1 - b1): three roundings of numbers below |m| + |g|, and (1 - b1) u |g|:  tol_m = 4 u (|m| + |g|).
     v' = v b2 + (1 - b2) g g: non-negative terms, four roundings and 2 u from g:  tol_v = 6 u v'.  The denominator sqrt(v') / bc2s + eps is a sum of
     non-negative terms: relative 3 u + u (sqrt) + u (divide) + e2 + u (add) = 6 u + e2.  The bias corrections 1 - b^t come from powf, documented at
     1 ulp (2 u relative); POW_ULP = 2 ulp are allowed.  The subtraction from 1 magnifies that by b^t / (1 - b^t):
         e1 = u (1 + 2 POW_ULP b1^t / (1 - b1^t)),    e2 = u (1 + 2 POW_ULP b2^t / (1 - b2^t)) / 2 + u     (sqrt halves, and rounds once).
     upd = (lr / bc1) m' / denom:  relative e1 + u + 2 u + 6 u + e2 plus the share of tol_m;  p' = p - upd rounds once:
         tol_p = u (|p| + |upd|) + |upd| (9 u + e1 + e2) + (lr / bc1) tol_m / denom.
     This bound has no slack on purpose: its leading term u |p'| IS the final rounding and is attained (err / tol 0.99, on the GPU and in fp32 numpy
     alike) whenever p' lies just above a power of two, so a ratio near 1 is what a correct kernel gives.  The only headroom is POW_ULP = 2 against a
     powf documented at 1 ulp: a device powf that got worse than 2 ulp would fail this test at once (first at small t, where b2^t / (1 - b2^t) is
     largest), and that is intended -- it would change every update by more than its last bit.
     A renormalised leaf: the bound N of the float64 result, plus what tol_p of the update moves:  inv (tol_p[i] + max tol_p) + |x'[i]| max tol_p / std.
"""
import math

import numpy as np

U = 2.0 ** -24
NT, CHUNK, NORM_CHUNK, ADAM_CHUNK = 1024, 4096, 8192, 4096
POW_ULP = 2.0
TINY = 2.0 ** -148            # two steps of fp32's subnormal spacing
MODEL_RES = (4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512)         # 13 backbone + 4 SR maps, the generator's own order
STRUCT_RES = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)


def levels(res):
    nl, r = 1, res
    while r > 8:
        nl, r = nl + 1, r >> 1
    return nl


def _pool(v):
    return 0.25 * ((v[0::2, 0::2] + v[0::2, 1::2]) + (v[1::2, 0::2] + v[1::2, 1::2]))


def _up(a, f):
    return a if f == 1 else np.repeat(np.repeat(a, f, 0), f, 1)


def _nb(v):
    """(left + right, up + down) of every element, periodic."""
    return np.roll(v, 1, 1) + np.roll(v, -1, 1), np.roll(v, 1, 0) + np.roll(v, -1, 0)


def moment_depth(n):
    return 16 + -(-n // CHUNK)


def reg_ref(x, scale=1.0, tol=True):
    """x: [res, res] (fp32 values).  Returns a dict: total (float), values [nl], grads [nl] (each [res, res]; their sum is the gradient), grad,
    m [nl, 2], absmom [nl, 2] (sum |v roll v| / n per direction), and with tol: dm [nl, 2], tol_total, tol_grad [res, res]."""
    v = np.asarray(x, dtype=np.float64)
    res = v.shape[0]
    assert v.shape == (res, res)
    nl = levels(res)
    a = np.abs(v)
    out = dict(values=[], grads=[], m=[], absmom=[], dm=[])
    tg = np.zeros_like(v)
    tv = 0.0
    for l in range(nl):
        n = v.size
        rx, ry = np.roll(v, 1, 1), np.roll(v, 1, 0)
        mx, my = float((v * rx).sum() / n), float((v * ry).sum() / n)
        lr_, ud = _nb(v)
        c = scale * 0.25 ** l * 2.0 / n
        out['values'].append(scale * (mx * mx + my * my))
        out['grads'].append(_up(c * (mx * lr_ + my * ud), 1 << l))
        out['m'].append((mx, my))
        Sx, Sy = float(np.abs(v * rx).sum()), float(np.abs(v * ry).sum())
        out['absmom'].append((Sx / n, Sy / n))
        if tol:
            pe = (1.0 + U) ** (3 * l) - 1.0
            q = 2 * pe + pe * pe
            Px, Py = float((a * np.roll(a, 1, 1)).sum()), float((a * np.roll(a, 1, 0)).sum())
            D = moment_depth(n)
            dmx, dmy = (D * U * (Sx + q * Px) + q * Px) / n, (D * U * (Sy + q * Py) + q * Py) / n
            out['dm'].append((dmx, dmy))
            tv += scale * (2 * abs(mx) * dmx + dmx * dmx + 2 * abs(my) * dmy + dmy * dmy)
            alr, aud = _nb(np.abs(v))
            plr, pud = _nb(a)
            tg += _up(c * (dmx * alr + abs(mx) * pe * plr + (nl + 6) * U * abs(mx) * alr
                           + dmy * aud + abs(my) * pe * pud + (nl + 6) * U * abs(my) * aud), 1 << l)
        if l + 1 < nl:
            v, a = _pool(v), _pool(a)
    out['total'] = float(sum(out['values']))
    out['grad'] = sum(out['grads'])
    if tol:
        out['tol_total'] = tv + 8 * U * out['total']
        out['tol_grad'] = tg
    return out


def reg_total_tol(refs, launches=1):
    """Bound of the value of one call over several buffers (R3)."""
    s = sum(r['total'] for r in refs)
    return sum(r['tol_total'] for r in refs) + (len(refs) + launches - 1) * U * s


def normalize_ref(x):
    x = np.asarray(x, dtype=np.float64)
    d = x - x.mean()
    return d / math.sqrt(float((d * d).mean()))


def norm_depth(n, form):
    return {'block': -(-n // NT) + 12, 'multi': 20 + -(-n // NORM_CHUNK), 'adam': 16 + -(-n // ADAM_CHUNK)}[form]


def normalize_tol(x, form):
    """Bound N for the float64 input x (any shape: one buffer)."""
    x = np.asarray(x, dtype=np.float64)
    mean = float(x.mean())
    var = float(((x - mean) ** 2).mean())
    k1 = 1.0 + mean * mean / var
    D = norm_depth(x.size, form)
    return np.abs(normalize_ref(x)) * ((3 * D + 4) * U * k1 / 2 + 4 * U) + D * U * math.sqrt(k1)


def _f32(v):
    return float(np.float32(v))


def adam_ref(p, g, g2, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, tol=False):
    """One step; t = the number of steps already made.  g or g2 may be None.  Returns (p, m, v) in float64, with tol: also (tol_p, tol_m, tol_v)."""
    b1, b2, eps, lr = _f32(beta1), _f32(beta2), _f32(eps), _f32(lr)
    p, m, v = (np.asarray(a, dtype=np.float64) for a in (p, m, v))
    gs = [np.asarray(a, dtype=np.float64) for a in (g, g2) if a is not None]
    gg = gs[0] + gs[1] if len(gs) == 2 else gs[0]
    t1 = float(t) + 1.0
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** t1, 1.0 - b2 ** t1
    denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / denom
    p1 = p - upd
    if not tol:
        return p1, m1, v1
    tm = 4 * U * (np.abs(m) + np.abs(gg)) + TINY            # TINY: a result below fp32's normal range (two gradients that cancel) rounds to a subnormal
    tv = 6 * U * v1 + TINY
    e1 = U * (1 + 2 * POW_ULP * b1 ** t1 / bc1)
    e2 = U * (1 + 2 * POW_ULP * b2 ** t1 / bc2) / 2 + U
    tp = U * (np.abs(p) + np.abs(upd)) + np.abs(upd) * (9 * U + e1 + e2) + (lr / bc1) * tm / denom
    return p1, m1, v1, tp, tm, tv


def adam_norm_ref(p1, tp):
    """A renormalised leaf slice: (float64 result, bound) from the float64 update p1 and its bound tp (header, A)."""
    x = normalize_ref(p1)
    std = math.sqrt(float(((p1 - p1.mean()) ** 2).mean()))
    tmax = float(tp.max())
    return x, normalize_tol(p1, 'adam') + (tp + tmax) / std + np.abs(x) * tmax / std


def compare(got, ref, tol):
    """(every element within its bound, largest err / tol); NaN and a non-zero error under a zero bound count as infinite."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    ratio = np.nan_to_num(ratio, nan=np.inf, posinf=np.inf)
    return bool((ratio <= 1.0).all()), float(ratio.max()) if ratio.size else 0.0


def compare_reg(got_total, got_grads, refs, launches=1):
    """The GPU file's comparison of one regulariser call: refs = reg_ref(...) of every buffer, got_grads = list (None entries are not compared) or
    None.  Returns (ok, worst err / tol, what was worst)."""
    ok, worst, what = True, 0.0, 'value'
    o, r = compare(got_total, sum(q['total'] for q in refs), reg_total_tol(refs, launches))
    ok, worst = ok and o, r
    for i, q in enumerate(refs):
        if got_grads is None or got_grads[i] is None:
            continue
        o, r = compare(got_grads[i], q['grad'], q['tol_grad'])
        ok = ok and o
        if r > worst:
            worst, what = r, f'grad of buffer {i} ({q["grad"].shape[0]}^2)'
    return ok, worst, what


# ---------------------------------------------------------------------------------------------------------------- case builders
def structured_case(res, seed=0):
    """A map whose every pyramid level carries lag-1 correlation: a correlated c x c pattern (c = the coarsest level's side) blown up to res, plus
    white noise; standardised (res > 1) and rounded to fp32.  With randn alone the correlation of level l is ~ 1 / sqrt(n_l) and the coarse levels of a
    large map vanish next to the fine ones."""
    rng = np.random.default_rng(1000 * res + seed)
    c = res >> (levels(res) - 1)
    z = rng.standard_normal((c, c))
    p = z + 0.7 * np.roll(z, 1, 0) + 0.5 * np.roll(z, 1, 1)
    x = _up(p, res // c) + 0.5 * rng.standard_normal((res, res))
    if res > 1:
        x = (x - x.mean()) / x.std()
    return x.astype(np.float32)


def randn_case(res, seed=0):
    return np.random.default_rng(77 * res + seed).standard_normal((res, res)).astype(np.float32)


def shares(ref):
    """Per level: (share of the buffer's value, share of |g|max) and the tolerance relative to the same two quantities."""
    gmax = float(np.abs(ref['grad']).max())
    sv = [v / ref['total'] for v in ref['values']]
    sg = [float(np.abs(g).max()) / gmax for g in ref['grads']]
    return sv, sg, ref['tol_total'] / ref['total'], float(ref['tol_grad'].max()) / gmax


def adam_state(n, seed, gmag=(1e-12, 1e4), zeros=0.1, mean=0.0):
    """Arbitrary fp32 state of a leaf of n elements: p ~ mean + randn, m of either sign, v >= 0, gradients g, g2 log-uniform in gmag with `zeros` of
    them exactly 0.  Every square and every product of the update stays inside fp32's normal range (|g| <= 1e4, v in [1e-24, 1e6] or 0)."""
    rng = np.random.default_rng(seed)

    def grad():
        e = rng.uniform(math.log10(gmag[0]), math.log10(gmag[1]), n)
        g = rng.choice([-1.0, 1.0], n) * 10.0 ** e
        g[rng.random(n) < zeros] = 0.0
        return g.astype(np.float32)
    g, g2 = grad(), grad()
    p = (mean + rng.standard_normal(n)).astype(np.float32)
    m = (g.astype(np.float64) * rng.uniform(-2, 2, n)).astype(np.float32)
    m[np.abs(m) < 1e-20] = 0.0
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.1, 3, n)).astype(np.float32)
    v[v < 1e-24] = 0.0
    return p, g, g2, m, v


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU file
SCALES = (1.0, 1e5)
BANK17 = tuple((r, i) for i, r in enumerate(MODEL_RES))                 # (res, seed) of the model's 17 maps
SINGLES = tuple((r, 100) for r in STRUCT_RES)                           # one structured map of every size; 1024^2 is called alone
VIEW_N = 2                                                              # images per [N, 1, r, r] tensor of the gradient-view test
VIEW_CASES = tuple((r, 10 * i + n) for i, r in enumerate((8, 16, 64, 256)) for n in range(VIEW_N))
NORM_RES = (2, 4, 64, 512)
NORM_MEANS = (0.0, 1.0, 8.0)                                            # mean / std of the normalise inputs
ADAM_SIZES = (1, 3, 4095, 4096, 4097, 8191, 12800, 3 * 4096 + 1)
ADAM_MAPS = ((2, 1, 16, 16), (3, 1, 64, 64), (2, 1, 128, 128))
_REFS = {}
_LISTED = frozenset(BANK17) | frozenset(SINGLES) | frozenset(VIEW_CASES)


def struct_ref(res, seed, scale):
    """(fp32 map, reg_ref of it), computed once and left unchanged.  Only the listed cases: those are the ones whose share condition
    tests/test_step_ops_cpu.py asserts, so a test cannot use a structured map that the assertion does not cover."""
    assert (res, seed) in _LISTED and scale in SCALES, f'structured case {(res, seed, scale)} is not in all_structured_cases()'
    k = (res, seed, scale)
    if k not in _REFS:
        x = structured_case(res, seed)
        _REFS[k] = (x, reg_ref(x, scale))
    return _REFS[k]


def all_structured_cases():
    """Every (res, seed) a structured map is built for, in either test file."""
    return sorted(_LISTED)


def norm_case(res, ratio, seed=0):
    """randn map with mean / std = ratio (fp32)."""
    x = np.random.default_rng(31 * res + seed).standard_normal((res, res))
    x = (x - x.mean()) / x.std() + ratio
    return (x * 1.7).astype(np.float32)
