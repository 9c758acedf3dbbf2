"""Independent float64 restatement of the kernels of csrc/loss_ops.hip -- max pooling, the channel normalisation of the LPIPS head (eps outside the
root) and of the stand-in feature net (eps inside), image_prepare, the squared distances, the total variation, slice_rgb4, the warp projection, the
channels-last grid sample, the direct 3 x 3 convolution with its pooling / activation backward -- each with its adjoint, the derived elementwise error
bounds, the launch arithmetic of every launcher, and the case lists that tests/test_loss_ops_cpu.py and tests/test_gpu_loss_ops.py share.  Plain numpy,
float64; nothing here calls the library or imports the package.

The operations (reference expressions)
  max pool        F.max_pool2d(x, k, s) without padding: first maximum in scan order, a NaN wins over everything (the last NaN of a window is kept).
  unit normalise  eps outside: f = x s mul / (|x| + eps)       (lpips normalize_tensor, the `lin` weight's root and 1 / sqrt(HW) folded into s, mul);
                  eps inside:  f = x s mul rsqrt(|x|^2 + eps)  (the stand-in feature net).  Backward dx = g s inv - x back with
                  back = (x . g s) mul / (r (r + eps)^2)  resp.  (x . g s) mul q^3.  An all-zero pixel of the eps-outside form has gradient 0 by definition
                  (autograd gives NaN there, the limit is g / eps).
  image_prepare   (img + 1) 255 / 2 area-resized by an integer factor f (w_projector.py:198-200): mul mean_{f x f}(img) + add, channel 3 = 0.
  sqdist          sum_i (a - b)^2 per image (w_projector.py:216-219); sqdist_sum / tv_norm: the terms of base_coach.py:104-126 and compute_tv_norm
                  (:294-305) added, scaled, onto `term` and `total`.
  warp project    warping_loss.py:18-54 with LinePlaneCollision (:58-72) per pixel.
  grid sample     F.grid_sample(bilinear, zeros, align_corners=False) on a channels-last map.
  conv3x3_direct  avg_pool2d(lrelu(conv2d(x, w, padding=1)) gain, 2); the plain form is its data gradient on flipped, transposed weights; XF forms the
                  pooling / activation backward 0.25 (ga + gb) gain (y > 0 ? 1 : alpha) of the saved output y on the fly.

The bounds.  u = 2^-24.  The library is compiled without contraction, so every product and every sum rounds once; division and square root are
documented at 1 ulp = 2 u by the HIP math API (DIV = SQRT = 2, in units of u).  A sum whose terms pass through at most D roundings has an error of at
most D u sum|terms| (first order; Higham 4.2); the sums of absolute values are float64 sums of the exact terms.  A block partial that meets others in
an atomic counts one more add per block, and an add onto a running target rounds u (|start| + sum|terms|).  No constant comes from what a kernel returns.

  P  max pool backward: at most ceil(k / s)^2 windows meet in a pixel, added in scan order: (terms - 1) u sum|terms|; 0 for uncovered pixels.
  N  normalise.  A lane adds per trip four squares (product, three adds) and one add into its sum: 5 roundings; trips = ceil(C4 / G) and log2 G
     xor steps: D_ss = 5 trips + log2 G, all terms >= 0: |d ss| <= D_ss u ss.  r = sqrt(ss): e_r = (D_ss / 2 + SQRT) u.
     eps outside: inv = mul / (r + eps): e_inv = e_r + (1 + DIV) u;  eps inside: q = 1 / sqrt(ss + eps): e_q = ((D_ss + 1) / 2 + SQRT + DIV) u,
     e_inv = e_q + u.  f = (x s) inv: two more roundings:  tol_f = |f| (e_inv + 2 u).
     Backward: dot = sum x g s with two products per term: D_dot = 6 trips + log2 G, |d dot| <= D_dot u A, A = sum |x g s|.
     back = dot mul / (r (r + eps) (r + eps)):  |d back| <= (D_dot u A + |dot| (3 e_r + (5 + DIV) u)) mul / (r (r + eps)^2);
     inside: back = dot mul q q q: |d back| <= (D_dot u A + |dot| (3 e_q + 4 u)) mul q^3.
     dx = g s inv - x back, a cancelling difference:  tol = |g s inv| (e_inv + 3 u) + |x| |d back| + 2 u |x back|  -- over the absolute values of both
     parts, so it follows the conditioning of the pixel (A / |dot|), not the largest entry.
  I  image_prepare: f^2 sequential adds, m = mul / f^2 rounds once, one fma:  u ((f^2 - 1) |m| sum|v| + 2 |S m| + |add|); backward 2 u |g m|.
  S  sqdist: d = a - b rounds once (exactly, when a ~ b), d d once, a thread adds four squares and one running add per trip, 6 xor steps, 2 adds
     over the waves:  D = 3 + 4 trips + 8 and one add per block in the atomic:  (D + blocks) u sum d^2.  Relative to sum d^2, not to |a|^2: the bound
     follows a ~ b.  Gradient 2 g (a - b): 2 u |da|.  sqdist_sum / tv add `scale` (one rounding) and accumulate onto a start value:
     |scale| S (D + 1) u + blocks u (|start| + |scale| S); tv per element: two differences, two squares, one add, one running add: D = 3 + 2 trips + 8.
     tv backward k a with a = up to four differences added: |k| 4 u sum|differences| + 2 u |k a|.
  W  warp projection: running error.  Every fp32 intermediate v contributes u |v| |d out / d v|; the partials are those of the float64
     restatement (a small reverse sweep over its own tape).  Factor 4 (WARP_MARGIN) for second-order terms and for the products of two errors near the
     division by n . u: a margin over the reference, not a measurement of the kernel.  The backward's bound is the running error of its own restatement.
     (The camera centre maps to the origin of the camera frame, so q = s A u and s = kk / n.u cancels in q_xy / q_z: the plane point P0 has no influence
     on uv beyond rounding.  A transposed plane point is therefore no observable mutant -- the CPU file asserts that it stays inside the bound -- and
     mutant 19 is the transposed intrinsics row and the transposed rotation.)
  G  grid sample.  ix = ((gx + 1) W - 1) / 2: |d ix| <= (2 |(gx + 1) W| + |(gx + 1) W - 1|) u / 2; tx = ix - floor(ix) is exact, 1 - tx rounds once.
     A weight w = a b: |d w| <= |d ix| |dw / dix| + |d iy| |dw / diy| + 3 u w.  out (four fmas): sum |t| |d w| + 4 u sum |w t|.
     dgrid: per corner a 4-term dot (4 roundings) and one fma per corner and trip, 6 xor steps, two products at the end:
     D = 4 + 4 trips + 6 + 2:  (D u sum |s| |d . t| + sum |d . t| |d s|) W / 2,  |d s| = |d i| + u.
     dinput: n terms w d meet in an element: sum (|d w| + u w) |d| + n u (|start| + sum |w d|), in any order.
     Dyadic coordinates on power-of-two maps with dyadic data are exact in every step: compared with array_equal.
  C  conv: 9 Ci fmas, KS - 1 LDS adds:  tol_z = (9 Ci + KS - 1) u A,  A = sum |x| |w|.  The activation is Lipschitz with constant gain, so a sign
     decided differently within tol_z stays inside  tol_y = gain tol_z + 2 u |y|  (gain alpha and the product round).  The average: three adds,
     tol_p = 0.25 sum tol_y + 0.75 u sum |y|.  pool2_act_bwd: the sum, gain alpha and the product: 3 u |dz|.  XF: the same conv on a dz that carries
     those 3 u: D + 3.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -148
DIV = SQRT = 2.0
NT = 256
ALPHA, GAIN = 0.2, math.sqrt(2.0)
WARP_MARGIN = 4.0
EPS = float(np.float32(1e-10))
F32 = np.float32


def f64(a):
    return np.asarray(a, dtype=np.float64)


def r32(v):
    """A Python float as the library receives it (c_float)."""
    return float(np.float32(v))


def compare(got, ref, tol):
    """(every element within its bound, largest err / tol).  A NaN of the reference must be a NaN of the result (canaries, propagated NaN), equal
    infinities agree; any other NaN and a non-zero error under a zero bound count as infinite.  No element is left out."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = np.broadcast_to(f64(tol), ref.shape)
    nr, ng = np.isnan(ref), np.isnan(got)
    with np.errstate(all='ignore'):
        err = np.where(got == ref, 0.0, np.abs(got - ref))
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(nr | ng, np.where(nr & ng, 0.0, np.inf), ratio)
    ratio = np.nan_to_num(ratio, nan=np.inf, posinf=np.inf)
    return bool((ratio <= 1.0).all()), float(ratio.max()) if ratio.size else 0.0


def exact(got, ref):
    """Exact classes: the same values everywhere (NaN in the same places)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return got.shape == ref.shape and bool(np.array_equal(f64(got), f64(ref), equal_nan=True))


def dyadic(rng, shape, denom=4, span=8):
    """Multiples of 1 / denom in [-span / denom, span / denom]: sums and products of a few hundred of them are exact in fp32."""
    return (rng.integers(-span, span + 1, shape) / float(denom)).astype(F32)


def grid_blocks(threads):
    return int(min(8192, -(-threads // NT)))


# ====================================================================================================================== max pool
POOL_GEOMS = ((2, 2, 4, 6), (2, 2, 9, 7), (3, 2, 8, 11), (3, 1, 5, 4), (2, 3, 8, 7), (1, 1, 3, 3))        # (k, s, H, W)
POOL_CHANNELS = (4, 8, 12)
POOL_N = 2
POOL_CASES = tuple((k, s, H, W, C) for (k, s, H, W) in POOL_GEOMS for C in POOL_CHANNELS)


def pool_out(H, W, k, s):
    return (H - k) // s + 1, (W - k) // s + 1


def pool_input(case):
    """x [N, H, W, C] fp32 with a fully tied window (image 0, window (0, 0)), two NaN in one window (image 1, window (0, 0), channel 1: its first and
    its last element) and a window of -inf (image 1, the last window, channel 2)."""
    k, s, H, W, C = case
    rng = np.random.default_rng(1000 * k + 100 * s + 10 * H + W + C)
    x = rng.standard_normal((POOL_N, H, W, C)).astype(F32)
    Ho, Wo = pool_out(H, W, k, s)
    x[0, 0:k, 0:k, :] = 3.0
    x[1, 0, 0, 1] = np.nan
    x[1, k - 1, k - 1, 1] = np.nan
    x[1, (Ho - 1) * s:(Ho - 1) * s + k, (Wo - 1) * s:(Wo - 1) * s + k, 2] = -np.inf
    return x


def maxpool_ref(x, k, s, mutant=None):
    """(y, argmax byte) of x [N, H, W, C]; y keeps x's dtype (the maximum is one of the inputs)."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, W, k, s)
    if mutant == 'hw_swapped':
        y, idx = maxpool_ref(x.reshape(N, W, H, C), k, s)
        return y.reshape(N, Ho, Wo, C), idx.reshape(N, Ho, Wo, C)
    y = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    idx = np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    for ky in range(k):
        for kx in range(k):
            v = x[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :]
            nan = np.isnan(v)
            with np.errstate(invalid='ignore'):
                take = (v >= y) if mutant == 'last_max' else (v > y)
            if mutant != 'nan_dropped':
                take = take | nan
            y = np.where(take, v, y)
            idx = np.where(take, np.uint8(ky * k + kx), idx)
    return y, idx


def maxpool_bwd_ref(dy, idx, H, W, k, s):
    """(dx float64 [N, H, W, C], bound P)."""
    dy = f64(dy)
    N, Ho, Wo, C = dy.shape
    dx, ab, cnt = (np.zeros((N, H, W, C)) for _ in range(3))
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + (Ho - 1) * s + 1, s), slice(kx, kx + (Wo - 1) * s + 1, s), slice(None))
            hit = idx == ky * k + kx
            dx[sl] += np.where(hit, dy, 0.0)
            ab[sl] += np.where(hit, np.abs(dy), 0.0)
            cnt[sl] += hit
    return dx, np.maximum(cnt - 1, 0) * U * ab


def pool_covered(H, W, k, s):
    """[H, W] bool: pixels inside at least one window."""
    Ho, Wo = pool_out(H, W, k, s)
    c = np.zeros((H, W), dtype=bool)
    for oy in range(Ho):
        for ox in range(Wo):
            c[oy * s:oy * s + k, ox * s:ox * s + k] = True
    return c


# ====================================================================================================================== unit normalise
UNIT_CHANNELS = (4, 8, 12, 64, 192, 256, 260, 512)
# the issue lists N * HW in {1, 3, 64, 65} with N = 2; 1, 3 and 65 pixels are odd counts, so those run with one image, and two images (the batch stride of
# the feature vector) run with HW = 1, 3, 32 and 65: N * HW = 2, 6, 64 (one full block at G = 4) and 130
UNIT_PIXELS = ((1, 1), (1, 3), (1, 65), (2, 1), (2, 3), (2, 32), (2, 65))           # (N, HW)
UNIT_LDX_PAD = 8
UNIT_CASES = tuple((N, HW, C) for C in UNIT_CHANNELS for (N, HW) in UNIT_PIXELS)
# five levels, pixel counts 1 ... 400; level 2 needs no gradient (the backward's compaction); the level with the most pixels is not the first
LEVELS = ((9, 12), (400, 8), (1, 260), (64, 64), (25, 192))                          # (HW, C)
LEVELS_N = 2
LEVELS_NO_GRAD = 2
LEVELS_GAP = 8                                                                      # floats of NaN after the slices of an image (ABI launches)


def group_width(C4):
    g = 1
    while g < C4 and g < 64:
        g <<= 1
    return g


def unit_launch(npix, C):
    C4 = C // 4
    G = group_width(C4)
    blocks = grid_blocks(npix * G)
    return dict(G=G, trips=-(-C4 // G), idle_lanes=G * -(-C4 // G) - C4, blocks=blocks, pixel_trips=-(-npix // (blocks * NT // G)))


def unit_input(N, HW, C, seed=0):
    """(x [N, HW, C], scale [C], g [N, HW, C], which special pixels exist).  Flat pixel 0 is all zero, 1 has norm 1e-12 (next to eps = 1e-10), 2 has norm
    1e3; a single pixel is the tiny one."""
    rng = np.random.default_rng(7919 * C + 31 * HW + N + seed)
    x = rng.standard_normal((N * HW, C))
    kinds = ('tiny',) if N * HW == 1 else ('zero', 'tiny', 'big')[:N * HW]
    for i, kind in enumerate(kinds):
        nrm = math.sqrt(float((x[i] ** 2).sum()))
        x[i] = dict(zero=0.0, tiny=1e-12 / nrm, big=1e3 / nrm)[kind] * x[i]
    scale = (0.5 + rng.random(C)).astype(F32)
    g = rng.standard_normal((N, HW, C)).astype(F32)
    return x.reshape(N, HW, C).astype(F32), scale, g, kinds


def _unit_common(x, scale, mul, eps, eps_inside, mutant):
    x = f64(x)
    C = x.shape[-1]
    L = unit_launch(1, C)
    s = np.ones(C) if scale is None else f64(scale)
    xs = x if mutant != 'last_quad' else np.concatenate([x[..., :-4], np.zeros_like(x[..., -4:])], -1)
    ss = (xs * xs).sum(-1, keepdims=True)
    Dss = 5 * L['trips'] + math.log2(L['G'])
    inside = bool(eps_inside) != (mutant == 'eps_swapped')
    r = np.sqrt(ss)
    e_r = (Dss / 2 + SQRT) * U
    e_q = ((Dss + 1) / 2 + SQRT + DIV) * U
    if inside:
        q = 1.0 / np.sqrt(ss + eps)
        inv, e_inv = mul * q, e_q + U
    else:
        q = None
        inv, e_inv = mul / (r + eps), e_r + (1 + DIV) * U
    return x, s, L, ss, r, q, inv, e_inv, e_r, e_q, inside


def unit_fwd_ref(x, scale, mul, eps=EPS, eps_inside=0, mutant=None):
    """x [..., C] -> (f float64, bound N)."""
    x, s, L, ss, r, q, inv, e_inv, e_r, e_q, inside = _unit_common(x, scale, mul, eps, eps_inside, mutant)
    f = x * s * inv
    return f, np.abs(f) * (e_inv + 2 * U) + TINY * (f != 0)


def unit_bwd_ref(x, scale, g, mul, eps=EPS, eps_inside=0, mutant=None):
    """(dx float64, bound N) for the cotangent g of the features."""
    x, s, L, ss, r, q, inv, e_inv, e_r, e_q, inside = _unit_common(x, scale, mul, eps, eps_inside, None if mutant in ('zero_nan', 'zero_limit') else mutant)
    g = f64(g)
    xd = x if mutant != 'last_quad' else np.concatenate([x[..., :-4], np.zeros_like(x[..., -4:])], -1)
    dot = (xd * g * s).sum(-1, keepdims=True)
    A = np.abs(x * g * s).sum(-1, keepdims=True)
    Ddot = 6 * L['trips'] + math.log2(L['G'])
    with np.errstate(divide='ignore', invalid='ignore'):
        if inside:
            k = mul * q ** 3
            back = dot * k
            dback = (Ddot * U * A + np.abs(dot) * (3 * e_q + 4 * U)) * k
        else:
            k = np.where(r > 0, mul / (r * (r + eps) ** 2), 0.0)
            back = dot * k
            dback = (Ddot * U * A + np.abs(dot) * (3 * e_r + (5 + DIV) * U)) * k
            inv = np.where(r > 0, inv, 0.0)                 # the zero pixel: gradient 0 by definition
    p1, p2 = g * s * inv, x * back
    dx = p1 - p2
    if not inside and mutant == 'zero_nan':
        dx = np.where(r > 0, dx, np.nan)
    if not inside and mutant == 'zero_limit':
        dx = np.where(r > 0, dx, g * s * mul / eps)
    return dx, np.abs(p1) * (e_inv + 3 * U) + np.abs(x) * dback + 2 * U * np.abs(p2) + TINY * ((p1 != 0) | (p2 != 0))


def levels_layout(levels=LEVELS, gap=0):
    """(offsets, slice sizes, batch stride) of the flat feature vector."""
    sizes = [hw * c for hw, c in levels]
    offs = [int(v) for v in np.cumsum([0] + sizes[:-1])]
    return offs, sizes, sum(sizes) + gap


def assemble_features(outs, stride, offs, mutant=None):
    """outs[l] [N, HW_l, C_l] -> [N, stride], NaN wherever no slice lies.  Mutants: the batch stride equal to the slice size ('batch_stride'), a level's
    offset taken one level late ('level_offset')."""
    N = outs[0].shape[0]
    flat = np.full(N * stride + max(o.shape[1] * o.shape[2] for o in outs) * (N + 1), np.nan)
    for l, o in enumerate(outs):
        size = o.shape[1] * o.shape[2]
        off = offs[l] if mutant != 'level_offset' else offs[l] + size
        nstride = size if mutant == 'batch_stride' else stride
        for n in range(N):
            flat[n * nstride + off:n * nstride + off + size] = f64(o[n]).reshape(-1)
    return flat[:N * stride].reshape(N, stride)


# ====================================================================================================================== image_prepare
PREP_CASES = ((2, 6, 10, 2), (1, 9, 6, 3), (2, 5, 7, 1), (1, 8, 12, 4))              # (N, H, W, f)
PREP_AFFINE = ((127.5, 128.0), (1.0, 0.0))


def prep_input(case, nan_channel3=True):
    N, H, W, f = case
    rng = np.random.default_rng(100 * H + W + f)
    img = (rng.random((N, H, W, 4)) * 2 - 1).astype(F32)
    img[..., 3] = np.nan if nan_channel3 else 0.0                # the kernel must not read the pad channel
    g = rng.standard_normal((N, H // f, W // f, 4)).astype(F32)
    g[..., 3] = np.nan if nan_channel3 else 0.0
    return img, g


def image_prepare_fwd_ref(img, f, mul, add, mutant=None):
    img = f64(img)
    N, H, W, _ = img.shape
    if mutant == 'hw_swapped':                                  # the index split with W and H exchanged, on the same memory
        o, t = image_prepare_fwd_ref(img.reshape(N, W, H, 4), f, mul, add)
        return o.reshape(N, H // f, W // f, 4), t.reshape(N, H // f, W // f, 4)
    Ho, Wo = H // f, W // f
    v = img[..., :3].reshape(N, Ho, f, Wo, f, 3)
    S, Sa = v.sum((2, 4)), np.abs(v).sum((2, 4))
    m = r32(mul) / (f if mutant == 'mean_over_f' else f * f)
    out, tol = np.zeros((N, Ho, Wo, 4)), np.zeros((N, Ho, Wo, 4))
    out[..., :3] = S * m + r32(add)
    tol[..., :3] = U * ((f * f - 1) * abs(m) * Sa + 2 * np.abs(S * m) + abs(r32(add)))
    return out, tol


def image_prepare_bwd_ref(g, f, mul, mutant=None):
    g = f64(g)
    N, Ho, Wo, _ = g.shape
    if mutant == 'hw_swapped':
        o, t = image_prepare_bwd_ref(g.reshape(N, Wo, Ho, 4), f, mul)
        return o.reshape(N, Ho * f, Wo * f, 4), t.reshape(N, Ho * f, Wo * f, 4)
    m = r32(mul) / (f if mutant == 'mean_over_f' else f * f)
    d = np.zeros((N, Ho * f, Wo * f, 4))
    d[..., :3] = np.repeat(np.repeat(g[..., :3], f, 1), f, 2) * m
    return d, 2 * U * np.abs(d)


# ====================================================================================================================== sqdist, sqdist_sum, tv
SQ_N = 3
SQ_SIZES = (4, 20, 1020, 4100, 4 * (256 * 1024 + 1))               # the last: more float4 than 256 blocks x 1024 take in one trip each
SQ_KINDS = ('random', 'close')                                     # b random; b = a (1 + 1e-6)
SQSUM_CAP, SQ_CAP = 512, 256
SQSUM_SIZES = (4, 1020, 4100, 4 * (512 * 1024 + 1))                # the last is beyond the 512-block cap
TV_SHAPES = ((1, 2, 2), (2, 2, 9), (2, 9, 2), (3, 33, 47))
OBJ_START = (0.75, -1.25)                                          # (term, total) before the calls: the kernels add


def sq_launch(F, cap):
    F4 = F // 4
    bx = max(1, min(cap, -(-F4 // (NT * 4))))
    return dict(blocks=bx, trips=-(-F4 // (bx * NT)), beyond_cap=-(-F4 // (NT * 4)) > cap)


def sq_input(F, kind, seed=0, N=SQ_N):
    rng = np.random.default_rng(F % 100003 + seed)
    a = rng.standard_normal((N, F)).astype(F32)
    b = rng.standard_normal((N, F)).astype(F32) if kind == 'random' else (f64(a) * (1 + 1e-6)).astype(F32)
    g = (0.5 + rng.random(N)).astype(F32)
    return a, b, g


def sqdist_ref(a, b, cap=SQ_CAP, mutant=None):
    """a, b [N, F] -> (sum of squares [N], bound S without scale and start)."""
    d = f64(a) - f64(b)
    F = d.shape[-1]
    L = sq_launch(F, cap)
    sq = d * d
    S = sq.sum(-1)
    if mutant == 'block_dropped':                       # block 1's share: float4 index i with (i // NT) % blocks == 1
        i4 = np.arange(F // 4)
        keep = np.repeat((i4 // NT) % L['blocks'] != 1, 4)
        return (sq * keep).sum(-1), None
    return S, (3 + 4 * L['trips'] + 8 + L['blocks']) * U * S


def sqdist_bwd_ref(a, b, g, which='a', mutant=None):
    """d / da (which = 'a') or d / db of sum_n g[n] sqdist[n]."""
    k = (1.0 if mutant == 'no_factor_2' else 2.0) * f64(g)[:, None]
    da = k * (f64(a) - f64(b))
    if which == 'b' and mutant != 'b_sign':
        da = -da
    return da, 2 * U * np.abs(da) + TINY * (da != 0)


def accumulate_bound(start, contributions):
    """Bound of a target that starts at `start` and takes, in turn, the terms (scale, S, D, blocks): S >= 0 the exact sum, D the roundings inside a block."""
    tol, run = 0.0, abs(float(start))
    for scale, S, D, blocks in contributions:
        run += abs(scale) * S
        tol += abs(scale) * S * (D + 1) * U + blocks * U * run
    return tol


def sqsum_term(a, b):
    """(S, D, blocks) of one sqdist_sum term over two tensors of n floats."""
    d = f64(a).reshape(-1) - f64(b).reshape(-1)
    L = sq_launch(d.size, SQSUM_CAP)
    return float((d * d).sum()), 3 + 4 * L['trips'] + 8, L['blocks']


def sqsum_bwd_ref(a, b, k):
    """d / da of k sum (a - b)^2 with k = gscale g formed in fp32 (one rounding), the difference and the product: 3 u."""
    da = 2.0 * k * (f64(a) - f64(b))
    return da, 3 * U * np.abs(da) + TINY * (da != 0)


def tv_launch(B, H, W):
    n = B * H * W
    blocks = grid_blocks(n)
    return dict(blocks=blocks, trips=-(-n // (blocks * NT)))


def tv_input(shape, seed=0):
    B, H, W = shape
    rng = np.random.default_rng(97 * H + W + seed)
    return (2.0 + rng.random((B, H, W))).astype(F32)


def tv_ref(v, mutant=None):
    """(S, D, blocks): S = sum over y < H - 1, x < W - 1 of (v - right)^2 + (v - below)^2."""
    v = f64(v)
    B, H, W = v.shape
    if mutant == 'hw_swapped':
        return tv_ref(v.reshape(B, W, H))
    L = tv_launch(B, H, W)
    if mutant == 'last_row_col':                         # every horizontal and every vertical difference, the last row and column included
        S = float(((v[:, :, :-1] - v[:, :, 1:]) ** 2).sum() + ((v[:, :-1, :] - v[:, 1:, :]) ** 2).sum())
    else:
        c = v[:, :-1, :-1]
        S = float(((c - v[:, :-1, 1:]) ** 2 + (c - v[:, 1:, :-1]) ** 2).sum())
    if mutant == 'block_dropped':
        i = np.arange(v.size).reshape(v.shape)
        c = v[:, :-1, :-1]
        t = (c - v[:, :-1, 1:]) ** 2 + (c - v[:, 1:, :-1]) ** 2
        S = float((t * ((i[:, :-1, :-1] // NT) % L['blocks'] != 1)).sum())
    return S, 3 + 2 * L['trips'] + 8, L['blocks']


def tv_bwd_ref(v, k, mutant=None):
    """(dv = k dS / dv, bound)."""
    v = f64(v)
    B, H, W = v.shape
    if mutant == 'hw_swapped':
        d, t = tv_bwd_ref(v.reshape(B, W, H), k)
        return d.reshape(B, H, W), t.reshape(B, H, W)
    a, ab = np.zeros_like(v), np.zeros_like(v)
    if mutant == 'last_row_col':
        r, d = v[:, :, :-1] - v[:, :, 1:], v[:, :-1, :] - v[:, 1:, :]
        a[:, :, :-1] += r; a[:, :, 1:] -= r; a[:, :-1, :] += d; a[:, 1:, :] -= d
    else:
        c = v[:, :-1, :-1]
        r, d = c - v[:, :-1, 1:], c - v[:, 1:, :-1]
        a[:, :-1, :-1] += r + d; a[:, :-1, 1:] -= r; a[:, 1:, :-1] -= d
        ab[:, :-1, :-1] += np.abs(r) + np.abs(d); ab[:, :-1, 1:] += np.abs(r); ab[:, 1:, :-1] += np.abs(d)
    dv = 2.0 * k * a
    return dv, 2 * abs(k) * 4 * U * ab + 2 * U * np.abs(dv) + TINY * (ab != 0)


# ====================================================================================================================== slice_rgb4
SLICE_CASES = tuple((P, C, add) for P in (1, 255, 257) for C in (4, 32) for add in (False, True))


def slice_rgb4_ref(x):
    y = np.array(np.asarray(x)[..., :4], dtype=F32)
    y[..., 3] = 0
    return y


def slice_rgb4_bwd_ref(dy, C, addend=None):
    dy = np.asarray(dy, dtype=F32)
    dx = np.zeros(dy.shape[:-1] + (C,), dtype=F32) if addend is None else np.array(addend, dtype=F32)
    dx[..., :3] += dy[..., :3]                              # one fp32 add per element: exact by construction (dyadic inputs) or the very same rounding
    return dx


# ====================================================================================================================== warp projection
class Tape:
    """A minimal reverse-mode tape over numpy float64 arrays: enough for the adjoint and the running-error bound of the projection."""

    def __init__(self):
        self.nodes = []

    def leaf(self, v):
        return Node(self, f64(v), (), False)


class Node:
    def __init__(self, tape, v, parents, rounds=True):
        self.tape, self.v, self.parents, self.rounds = tape, v, parents, rounds
        tape.nodes.append(self)

    def _c(self, o):
        return o if isinstance(o, Node) else Node(self.tape, f64(o), (), False)

    def __add__(self, o):
        o = self._c(o)
        return Node(self.tape, self.v + o.v, ((self, 1.0), (o, 1.0)))

    def __sub__(self, o):
        o = self._c(o)
        return Node(self.tape, self.v - o.v, ((self, 1.0), (o, -1.0)))

    def __mul__(self, o):
        o = self._c(o)
        return Node(self.tape, self.v * o.v, ((self, o.v), (o, self.v)))

    def __truediv__(self, o):
        o = self._c(o)
        return Node(self.tape, self.v / o.v, ((self, 1.0 / o.v), (o, -self.v / (o.v * o.v))))

    def __neg__(self):
        return Node(self.tape, -self.v, ((self, -1.0),), False)

    def __rtruediv__(self, o):
        return self._c(o) / self

    __radd__ = __add__
    __rmul__ = __mul__


def adjoints(out):
    """{id(node): d out / d node} for every node `out` depends on."""
    adj = {id(out): np.ones_like(out.v)}
    for n in reversed(out.tape.nodes):
        a = adj.get(id(n))
        if a is None:
            continue
        for p, d in n.parents:
            adj[id(p)] = adj.get(id(p), 0.0) + a * d
    return adj


def running_error(out, adj=None):
    adj = adjoints(out) if adj is None else adj
    e = 0.0
    for n in out.tape.nodes:
        a = adj.get(id(n))
        if a is not None and n.rounds:
            e = e + np.abs(n.v) * np.abs(a)
    return WARP_MARGIN * U * e + TINY


def _lookat(origin):
    fwd = -origin / np.linalg.norm(origin)
    right = -np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    up /= np.linalg.norm(up)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, fwd, origin
    return m


def camera(yaw, pitch, radius=2.7):
    """cam2world looking at the origin (the construction of the synthetic cameras), rounded to fp32."""
    o = np.array([radius * math.sin(pitch) * math.cos(math.pi - yaw), radius * math.cos(pitch), radius * math.sin(pitch) * math.sin(math.pi - yaw)])
    return _lookat(o).astype(F32)


WARP_K = np.array([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]], dtype=F32)
WARP_P = (1, 257)
WARP_VIEWS = ('synth', 'rotated60')


def warp_consts(ext, K, mutant=None):
    """The 24 constants from the canonical cam2world `ext` and the intrinsics K, in float64: camera centre, plane point ext (0, 0, 1, 1)^T, rows 0..2 of
    ext^-1 (A, then b), rows 0..1 of K."""
    ext, K = f64(ext).reshape(4, 4), f64(K).reshape(3, 3)
    w2c = np.linalg.inv(ext)
    pt = (ext.T if mutant == 'plane_point_transposed' else ext) @ np.array([0.0, 0.0, 1.0, 1.0])
    Kr = K.T if mutant == 'intrinsics_transposed' else K
    A = w2c[:3, :3].T if mutant == 'rotation_transposed' else w2c[:3, :3]
    return np.concatenate([ext[:3, 3], pt[:3], A.reshape(-1), w2c[:3, 3], Kr[:2].reshape(-1)])


def warp_input(P, view, seed=0):
    """(canonical ext, K, origins [P, 3], dirs [P, 3], depth [P] in [2.2, 3.2], duv [P, 2]) in fp32; `view`: a second synthetic camera or one rotated 60 degrees."""
    rng = np.random.default_rng(13 * P + seed + len(view))
    ext = camera(math.pi / 2 + 0.1, math.pi / 2 - 0.05)
    cam = camera(math.pi / 2 - 0.3, math.pi / 2 + 0.2) if view == 'synth' else camera(math.pi / 2 + 0.1 + math.pi / 3, math.pi / 2 - 0.05)
    c = f64(cam[:3, 3])
    o = (c + 0.01 * rng.standard_normal((P, 3))).astype(F32)
    d = -c + 0.25 * rng.standard_normal((P, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    depth = (2.2 + rng.random(P)).astype(F32)
    duv = rng.standard_normal((P, 2)).astype(F32)
    return ext, WARP_K, o, d, depth, duv


def _warp_pixel(k, o, d, t):
    u = [o[i] + d[i] * t - k[i] for i in range(3)]
    n = [-k[i] for i in range(3)]
    ndotu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2]
    kk = -(n[0] * (k[0] - k[3]) + n[1] * (k[1] - k[4]) + n[2] * (k[2] - k[5]))
    si = kk / ndotu
    h = [k[i] + si * u[i] for i in range(3)]
    q = [k[6 + 3 * r] * h[0] + k[7 + 3 * r] * h[1] + k[8 + 3 * r] * h[2] + k[15 + r] for r in range(3)]
    return u, ndotu, si, q


def warp_fwd_eval(k, o, d, t):
    """[uv_x, uv_y] from 24 constants, three origin and three direction components and the depth: written once for tape nodes (float64, with partials)
    and for plain arrays of any precision (the fp32 evaluations of the CPU file)."""
    u, ndotu, si, q = _warp_pixel(k, o, d, t)
    rx, ry = q[0] / q[2], q[1] / q[2]
    return [(k[18 + 3 * r] * rx + k[19 + 3 * r] * ry + k[20 + 3 * r] - 0.5) * 2.0 for r in range(2)]


def warp_bwd_eval(k, o, d, t, gx, gy):
    """The backward as its own straight-line program (chain rule through the division by q_z, the world->camera rows and the intersection scale
    s = kk / n.u): [d_o x3, d_d x3, d_depth]."""
    u, ndotu, si, q = _warp_pixel(k, o, d, t)
    drx, dry = (k[18] * gx + k[21] * gy) * 2.0, (k[19] * gx + k[22] * gy) * 2.0
    iz = 1.0 / q[2]
    dq = [drx * iz, dry * iz, -((drx * q[0] + dry * q[1]) * iz * iz)]
    dh = [k[6 + i] * dq[0] + k[9 + i] * dq[1] + k[12 + i] * dq[2] for i in range(3)]
    dsi = dh[0] * u[0] + dh[1] * u[1] + dh[2] * u[2]
    dn = -(si / ndotu) * dsi
    g = [si * dh[i] - k[i] * dn for i in range(3)]
    return g + [g[i] * t for i in range(3)] + [g[0] * d[0] + g[1] * d[1] + g[2] * d[2]]


def _warp_leaves(consts, o, d, depth):
    T = Tape()
    o, d = f64(o), f64(d)
    return T, [T.leaf(c) for c in f64(consts)], [T.leaf(o[:, i]) for i in range(3)], [T.leaf(d[:, i]) for i in range(3)], T.leaf(f64(depth))


def warp_fwd_ref(consts, o, d, depth):
    """(uv [P, 2] float64, running-error bound W)."""
    T, k, on, dn, tn = _warp_leaves(consts, o, d, depth)
    uv = warp_fwd_eval(k, on, dn, tn)
    return np.stack([uv[0].v, uv[1].v], -1), np.stack([running_error(uv[0]), running_error(uv[1])], -1)


def warp_adjoint(consts, o, d, depth, duv):
    """(d_o [P, 3], d_d [P, 3], d_depth [P]) = J^T duv from the forward tape alone."""
    T, k, on, dn, tn = _warp_leaves(consts, o, d, depth)
    uv = warp_fwd_eval(k, on, dn, tn)
    duv = f64(duv)
    a0, a1 = adjoints(uv[0]), adjoints(uv[1])
    g = lambda n: duv[:, 0] * a0[id(n)] + duv[:, 1] * a1[id(n)]      # noqa: E731
    return np.stack([g(n) for n in on], -1), np.stack([g(n) for n in dn], -1), g(tn)


def warp_bwd_ref(consts, o, d, depth, duv):
    """((d_o, d_d, d_depth), (their bounds)): the values of warp_bwd_eval in float64 (equal to warp_adjoint) and the running error of that program."""
    T, k, on, dn, tn = _warp_leaves(consts, o, d, depth)
    duv = f64(duv)
    outs = warp_bwd_eval(k, on, dn, tn, T.leaf(duv[:, 0]), T.leaf(duv[:, 1]))
    val = [n.v for n in outs]
    tol = [running_error(n) for n in outs]
    return (np.stack(val[0:3], -1), np.stack(val[3:6], -1), val[6]), (np.stack(tol[0:3], -1), np.stack(tol[3:6], -1), tol[6])


# ====================================================================================================================== grid sample
GS_CASES = ((2, 4, 4, 8, 3, 5), (2, 260, 3, 5, 2, 3), (1, 256, 8, 8, 4, 4))          # (N, C, H, W, Ho, Wo)
GS_BORDER_DISTANCE = 1e-3


def gs_launch(N, C, Ho, Wo):
    P = N * Ho * Wo
    return dict(blocks=-(-P // 4), trips=-(-C // 256), straddles=(Ho * Wo) % 4 != 0 and N > 1, ragged_last_block=P % 4 != 0)


def gs_unnormalize(g, size, mutant=None):
    if mutant == 'align_corners':
        return (g + 1.0) / 2.0 * (size - 1)
    return ((g + 1.0) * size - 1.0) / 2.0


def gs_exact_grid(case):
    """Dyadic grid points on a power-of-two map covering all sixteen combinations of corner validity; ix takes -1.5, -1, -0.5, W - 1, W - 0.5, W + 0.5 and
    two interior values exactly (iy alike)."""
    N, C, H, W, Ho, Wo = case
    assert H & (H - 1) == 0 and W & (W - 1) == 0
    xa, xb = (-1.5, -1.0, 2.25, W - 1.0), (W + 0.5, -0.5, 1.5, W - 0.5)
    ya, yb = (-1.5, -1.0, 1.25, H - 1.0), (H + 0.5, -0.5, 0.5, H - 0.5)
    pts = []
    for j in range(N * Ho * Wo):
        xc, yc, alt = j % 4, (j // 4) % 4, (j // 16) % 2
        ix = (xa if (yc + alt) % 2 == 0 else xb)[xc]
        iy = (ya if (xc + alt) % 2 == 0 else yb)[yc]
        pts.append(((2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1))
    return np.array(pts, dtype=F32).reshape(N, Ho, Wo, 2)


def gs_validity_classes(grid, H, W):
    """The set of (x0 valid, x0 + 1 valid, y0 valid, y0 + 1 valid) over the grid points."""
    g = f64(grid).reshape(-1, 2)
    x0, y0 = np.floor(gs_unnormalize(g[:, 0], W)), np.floor(gs_unnormalize(g[:, 1], H))
    ok = lambda v, n: (v >= 0) & (v < n)         # noqa: E731
    return set(zip(ok(x0, W).tolist(), ok(x0 + 1, W).tolist(), ok(y0, H).tolist(), ok(y0 + 1, H).tolist()))


def gs_random_grid(case, seed=0):
    """Points from outside the map to outside on the other side, each at least 0.01 from a cell border before the rounding of the grid value to fp32."""
    N, C, H, W, Ho, Wo = case
    rng = np.random.default_rng(17 * C + W + seed)
    ix = rng.integers(-2, W + 1, (N, Ho, Wo)) + rng.uniform(0.01, 0.99, (N, Ho, Wo))
    iy = rng.integers(-2, H + 1, (N, Ho, Wo)) + rng.uniform(0.01, 0.99, (N, Ho, Wo))
    return np.stack([(2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1], -1).astype(F32)


def gs_border_distance(grid, H, W):
    g = f64(grid)
    ix, iy = gs_unnormalize(g[..., 0], W), gs_unnormalize(g[..., 1], H)
    fr = lambda v: np.minimum(v - np.floor(v), np.ceil(v) - v)      # noqa: E731
    return float(min(fr(ix).min(), fr(iy).min()))


def gs_contention_grid(case, seed=0):
    """All grid points of an image equal (an interior point, 0.3 / 0.6 into its cell)."""
    N, C, H, W, Ho, Wo = case
    g = np.zeros((N, Ho, Wo, 2))
    for n in range(N):
        ix, iy = (W - 1) / 2.0 - 0.2 + 0.5 * n, (H - 1) / 2.0 + 0.1 - 0.5 * n
        g[n, ..., 0], g[n, ..., 1] = (2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1
    return g.astype(F32)


def gs_data(case, exact_class, seed=0):
    N, C, H, W, Ho, Wo = case
    rng = np.random.default_rng(5 * C + H + seed)
    if exact_class:
        return dyadic(rng, (N, H, W, C)), dyadic(rng, (N, Ho, Wo, C)), dyadic(rng, (N, H, W, C))
    return (rng.standard_normal((N, H, W, C)).astype(F32), rng.standard_normal((N, Ho, Wo, C)).astype(F32), rng.standard_normal((N, H, W, C)).astype(F32))


def _gs_corners(grid, H, W, mutant):
    g = f64(grid)
    ix, iy = gs_unnormalize(g[..., 0], W, mutant), gs_unnormalize(g[..., 1], H, mutant)
    bx, by = (g[..., 0] + 1.0) * W, (g[..., 1] + 1.0) * H
    dix, diy = U * (2 * np.abs(bx) + np.abs(bx - 1)) / 2, U * (2 * np.abs(by) + np.abs(by - 1)) / 2
    inside = np.ones_like(ix)
    if mutant == 'border':
        inside = ((ix >= 0) & (ix <= W - 1)).astype(float), ((iy >= 0) & (iy <= H - 1)).astype(float)       # d clip / d i
        ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = ix - x0, iy - y0
    # (dy, dx, weight, d weight / d ix, d weight / d iy)
    cs = [(0, 0, (1 - tx) * (1 - ty), -(1 - ty), -(1 - tx)), (0, 1, tx * (1 - ty), (1 - ty), -tx), (1, 0, (1 - tx) * ty, -ty, (1 - tx)), (1, 1, tx * ty, ty, tx)]
    if mutant == 'w01_w10':
        cs = [cs[0], (0, 1) + cs[2][2:], (1, 0) + cs[1][2:], cs[3]]
    return x0.astype(int), y0.astype(int), cs, dix, diy, inside


def grid_sample_ref(inp, grid, mutant=None):
    """inp [N, H, W, C], grid [N, Ho, Wo, 2] -> (out [N, Ho, Wo, C], bound G)."""
    inp = f64(inp)
    N, H, W, C = inp.shape
    x0, y0, cs, dix, diy, _ = _gs_corners(grid, H, W, mutant)
    n = np.arange(N)[:, None, None]
    out, tol = np.zeros(x0.shape + (C,)), np.zeros(x0.shape + (C,))
    for dy, dx, w, sx, sy in cs:
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        t = inp[n, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None]
        if mutant == 'last_quad':
            t = t.copy()
            t[..., -4:] = 0
        out += w[..., None] * t
        dw = dix * np.abs(sx) + diy * np.abs(sy) + 3 * U * np.abs(w)
        tol += np.abs(t) * dw[..., None] + 4 * U * np.abs(w[..., None] * t)
    return out, tol


def grid_sample_bwd_ref(inp, grid, dout, start=None, mutant=None):
    """(dgrid [N, Ho, Wo, 2], its bound, dinput [N, H, W, C] added onto `start`, its bound)."""
    inp, dout = f64(inp), f64(dout)
    N, H, W, C = inp.shape
    x0, y0, cs, dix, diy, inside = _gs_corners(grid, H, W, mutant)
    n = np.broadcast_to(np.arange(N)[:, None, None], x0.shape)
    trips = -(-C // 256)
    D = 4 + 4 * trips + 6 + 2
    gx, gy, tgx, tgy = (np.zeros(x0.shape) for _ in range(4))
    dinp, term, dterm, cnt = (np.zeros_like(inp) for _ in range(4))
    for dy, dx, w, sx, sy in cs:
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
        t = inp[n, yc, xc] * ok[..., None]
        dd = dout.copy()
        if mutant == 'last_quad':
            dd[..., -4:] = 0
        dot, adot = (dd * t).sum(-1), np.abs(dout * t).sum(-1)
        gx += sx * dot
        gy += sy * dot
        tgx += D * U * np.abs(sx) * adot + adot * (diy + U)
        tgy += D * U * np.abs(sy) * adot + adot * (dix + U)
        dw = dix * np.abs(sx) + diy * np.abs(sy) + 3 * U * np.abs(w)
        wd = (w * ok)[..., None] * dout
        np.add.at(dinp, (n, yc, xc), wd)
        np.add.at(term, (n, yc, xc), np.abs(wd))
        np.add.at(dterm, (n, yc, xc), ((dw + U * np.abs(w)) * ok)[..., None] * np.abs(dout))
        np.add.at(cnt, (n, yc, xc), np.broadcast_to(ok[..., None], dout.shape).astype(float))
    if mutant == 'border':
        gx, gy = gx * inside[0], gy * inside[1]
    mx, my = (1.0, 1.0) if mutant == 'no_half_size' else ((W - 1) / 2.0, (H - 1) / 2.0) if mutant == 'align_corners' else (W / 2.0, H / 2.0)
    start = np.zeros_like(inp) if start is None else f64(start)
    dgrid, tgrid = np.stack([gx * mx, gy * my], -1), np.stack([tgx * W / 2.0, tgy * H / 2.0], -1) + TINY
    return dgrid, tgrid, start + dinp, dterm + cnt * U * (np.abs(start) + term)


# ====================================================================================================================== conv3x3_direct
CONV_SHAPES = ((2, 6, 10), (1, 18, 16), (1, 2, 2))                 # 15 quads: one ragged block; 72: two blocks, the second ragged; one quad
CONV_CI = (4, 12, 16, 20)
CONV_CO = (4, 8)
CONV_G = (1, 2, 4)
CONV_FORMS = ('act_pool', 'plain', 'pooled_only', 'xf_ga', 'xf_gb', 'xf_both')
CONV_CASES = tuple((shape, ci) for shape in CONV_SHAPES for ci in CONV_CI)


def conv_launch(N, H, W, Ci, Co, G):
    quads = (H // 2) * (W // 2)
    KS = 4 if Ci >= 16 else 1
    per_wave = [len(range(k, Ci // 4, KS)) for k in range(KS)]
    return dict(quads=quads, blocks=-(-quads // 64), ragged=quads % 64 != 0, KS=KS, per_wave=per_wave, uneven=len(set(per_wave)) > 1, grid=(-(-quads // 64), Co // G, N))


def conv_input(shape, Ci, Co, seed=0):
    """x [N, H, W, Ci]; w [Co, Ci, 3, 3] whose output channel 1 is all zero (outputs exactly 0 before the activation); ga, gb [N, H/2, W/2, Ci]."""
    N, H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * Ci + Co + seed)
    x = rng.standard_normal((N, H, W, Ci)).astype(F32)
    w = (rng.standard_normal((Co, Ci, 3, 3)) / math.sqrt(9 * Ci)).astype(F32)
    w[1] = 0
    ga, gb = (rng.standard_normal((N, H // 2, W // 2, Ci)).astype(F32) for _ in range(2))
    return x, w, ga, gb


def conv_ref(x, w, mutant=None):
    """(z [N, H, W, Co], A = sum |x| |w|)."""
    x, w = f64(x), f64(w)
    N, H, W, Ci = x.shape
    if mutant == 'hw_swapped':
        z, A = conv_ref(x.reshape(N, W, H, Ci), w)
        return z.reshape(N, H, W, -1), A.reshape(N, H, W, -1)
    if mutant == 'last_quad':
        x = x.copy()
        x[..., -4:] = 0
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    z, A = np.zeros((N, H, W, w.shape[0])), np.zeros((N, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            p = xp[:, ky:ky + H, kx:kx + W]
            z += np.einsum('nhwc,oc->nhwo', p, w[:, :, ky, kx])
            A += np.einsum('nhwc,oc->nhwo', np.abs(p), np.abs(w[:, :, ky, kx]))
    return z, A


def _pool4(a):
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).sum((2, 4))


def conv_fwd_ref(x, w, act, alpha=ALPHA, gain=GAIN, extra_roundings=0, mutant=None):
    """dict(y, tol_y, pooled, tol_pooled) of the kernel's epilogue on z = conv(x, w); alpha, gain as the library receives them."""
    z, A = conv_ref(x, w, mutant if mutant in ('hw_swapped', 'last_quad') else None)
    Ci = np.shape(x)[-1]
    KS = 4 if Ci >= 16 else 1
    tol_z = (9 * Ci + KS - 1 + extra_roundings) * U * A
    alpha, gain = r32(alpha), r32(gain)
    if act:
        y = z * np.where(z > 0, gain, gain * alpha)
        tol_y = gain * tol_z + 2 * U * np.abs(y)
    else:
        y, tol_y = z, tol_z
    quarter = 1.0 if mutant == 'no_quarter' else 0.25
    return dict(y=y, tol_y=tol_y + TINY * (A != 0), pooled=quarter * _pool4(y), tol_pooled=0.25 * _pool4(tol_y) + 0.75 * U * _pool4(np.abs(y)) + TINY)


def pool2_act_bwd_ref(ga, gb, yref, alpha=ALPHA, gain=GAIN, mutant=None):
    """(dz [N, H, W, C], bound): 0.25 (ga + gb)[cell] gain (y > 0 ? 1 : alpha) on the saved output y."""
    yref = f64(yref)
    N, H, W, C = yref.shape
    if mutant == 'hw_swapped':
        sw = lambda a: None if a is None else f64(a).reshape(N, W // 2, H // 2, C)      # noqa: E731
        d, t = pool2_act_bwd_ref(sw(ga), sw(gb), yref.reshape(N, W, H, C), alpha, gain)
        return d.reshape(N, H, W, C), t.reshape(N, H, W, C)
    g = sum(f64(a) for a in (ga, gb) if a is not None)
    g = np.repeat(np.repeat(g, 2, 1), 2, 2)
    alpha, gain = r32(alpha), r32(gain)
    pos = (yref >= 0) if mutant == 'ge_sign' else (yref > 0)
    dz = (1.0 if mutant == 'no_quarter' else 0.25) * g * gain * np.where(pos, 1.0, alpha)
    return dz, 3 * U * np.abs(dz) + TINY * (dz != 0)


def saved_output(shape, C, seed=0):
    """A saved activation output with exact zeros (one channel, and scattered elements)."""
    N, H, W = shape
    rng = np.random.default_rng(3 * H + C + seed)
    y = rng.standard_normal((N, H, W, C)).astype(F32)
    y[..., 1] = 0
    y[rng.random(y.shape) < 0.1] = 0
    return y


def pack_direct(w, G):
    """[Co, Ci, 3, 3] -> [Co / G][Ci / 4][9][4][G], the layout the kernel reads (include/eg3d_hip.h)."""
    w = np.asarray(w, dtype=F32)
    Co, Ci = w.shape[:2]
    return np.ascontiguousarray(w.reshape(Co // G, G, Ci // 4, 4, 9).transpose(0, 2, 4, 3, 1))


def adjoint_weights(w):
    """The data gradient's weights: flipped taps, channels exchanged."""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


# ====================================================================================================================== launch-shape classes
def launch_classes():
    """The launch-shape classes the listed cases reach, from the launch arithmetic above (asserted in tests/test_loss_ops_cpu.py)."""
    c = set()
    for (k, s, H, W, C) in POOL_CASES:
        Ho, Wo = pool_out(H, W, k, s)
        c.add(('pool', 'overlap' if s < k else 'gaps' if s > k else 'tiled'))
        if not pool_covered(H, W, k, s).all():
            c.add(('pool', 'uncovered pixels'))
        if H != W:
            c.add(('pool', 'non-square'))
    for (N, HW, C) in UNIT_CASES:
        L = unit_launch(N * HW, C)
        c.add(('unit', 'G', L['G']))
        c.add(('unit', 'trips', L['trips']))
        if L['idle_lanes'] and L['trips'] == 1:
            c.add(('unit', 'idle lane in a group'))
        if L['trips'] == 2 and C // 4 - L['G'] == 1:
            c.add(('unit', 'second trip with one lane'))
        c.add(('unit', 'blocks', min(L['blocks'], 2)))
        if (N * HW * L['G']) % NT:
            c.add(('unit', 'ragged block'))
    for F in SQ_SIZES:
        L = sq_launch(F, SQ_CAP)
        c.add(('sqdist', 'blocks', min(L['blocks'], 2)))
        c.add(('sqdist', 'beyond cap', L['beyond_cap']))
        if (F // 4) % NT:
            c.add(('sqdist', 'ragged'))
    for F in SQSUM_SIZES:
        c.add(('sqsum', 'beyond cap', sq_launch(F, SQSUM_CAP)['beyond_cap']))
    for (B, H, W) in TV_SHAPES:
        c.add(('tv', 'blocks', min(tv_launch(B, H, W)['blocks'], 2)))
        if H == 2:
            c.add(('tv', 'H = 2'))
        if W == 2:
            c.add(('tv', 'W = 2'))
    for case in GS_CASES:
        N, C, H, W, Ho, Wo = case
        L = gs_launch(N, C, Ho, Wo)
        c.add(('gs', 'trips', L['trips']))
        if L['straddles']:
            c.add(('gs', 'block straddles two images'))
        if L['ragged_last_block']:
            c.add(('gs', 'ragged last block'))
    for (shape, Ci) in CONV_CASES:
        for Co in CONV_CO:
            for G in CONV_G:
                L = conv_launch(*shape, Ci, Co, G)
                c.add(('conv', 'G', G, 'KS', L['KS']))
                c.add(('conv', 'blocks', L['blocks'], 'ragged', L['ragged']))
                if L['uneven']:
                    c.add(('conv', 'quads dealt unevenly'))
                if L['KS'] == 1 and Ci // 4 == 3:
                    c.add(('conv', 'KS 1, three quads'))
    return c


REQUIRED_CLASSES = frozenset({
    ('pool', 'overlap'), ('pool', 'gaps'), ('pool', 'tiled'), ('pool', 'uncovered pixels'), ('pool', 'non-square'),
    ('unit', 'G', 1), ('unit', 'G', 2), ('unit', 'G', 4), ('unit', 'G', 16), ('unit', 'G', 64), ('unit', 'trips', 1), ('unit', 'trips', 2),
    ('unit', 'idle lane in a group'), ('unit', 'second trip with one lane'), ('unit', 'blocks', 1), ('unit', 'blocks', 2), ('unit', 'ragged block'),
    ('sqdist', 'blocks', 1), ('sqdist', 'blocks', 2), ('sqdist', 'beyond cap', True), ('sqdist', 'beyond cap', False), ('sqdist', 'ragged'),
    ('sqsum', 'beyond cap', True), ('sqsum', 'beyond cap', False),
    ('tv', 'blocks', 1), ('tv', 'blocks', 2), ('tv', 'H = 2'), ('tv', 'W = 2'),
    ('gs', 'trips', 1), ('gs', 'trips', 2), ('gs', 'block straddles two images'), ('gs', 'ragged last block'),
    ('conv', 'G', 1, 'KS', 1), ('conv', 'G', 2, 'KS', 1), ('conv', 'G', 4, 'KS', 1), ('conv', 'G', 1, 'KS', 4), ('conv', 'G', 2, 'KS', 4), ('conv', 'G', 4, 'KS', 4),
    ('conv', 'blocks', 1, 'ragged', True), ('conv', 'blocks', 2, 'ragged', True), ('conv', 'quads dealt unevenly'), ('conv', 'KS 1, three quads'),
})
