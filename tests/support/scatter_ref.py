"""Independent reference of the tri-plane gradient scatter (eg3d_triplane_scatter, csrc/renderer.hip), its derived error bound and the case
builders of tests/test_gpu_scatter.py and tests/test_scatter_cpu.py.  Plain torch, float64, usable on either device; nothing here calls the library.

The operation (grid_sample's backward w.r.t. the planes: bilinear, zeros padding, align_corners=False -- checked against autograd in
tests/test_scatter_cpu.py):  for every present row s of image n and every plane pl, with (u, v) = (x, y), (x, z), (z, x) of pos * (2 / box_warp),
    ix = ((u + 1) Wp - 1) / 2,  iy = ((v + 1) Hp - 1) / 2,  x0 = floor(ix),  y0 = floor(iy),  wx = ix - x0,  wy = iy - y0,
    d_planes[n, y0 + j, x0 + i, 32 pl + c] += (i ? wx : 1 - wx) (j ? wy : 1 - wy) rows[s, c]      for the corners (i, j) inside the plane.
A row with pos.x = NaN is absent: its gradient row is not part of the data (it may hold anything, NaN included).
"""
import math

import torch

FC = 32          # channels per plane
TS = 15          # interior texels per tile side of the kernel's binning (a tile's accumulator is 16 wide: its column 15 is the next tile's column 0)


# ---------------------------------------------------------------------------------------------------------------- the reference
def corner_pairs(pos, N, Hp, Wp, box_warp):
    """Every (present row, plane, corner inside the plane) as flat tensors: image n, plane pl, texel y / x, float64 bilinear weight w, global row
    index row, the cell's x0 / y0 and the corner's side i / j.  The product pos * (2 / box_warp) is done in fp32, as the kernel does (so that both
    start from the same coordinate); everything after it is float64.  Cells without a corner in range (+-Inf and 1e30 coordinates among them) and
    absent rows (pos.x = NaN) contribute nothing."""
    pos = pos.reshape(-1, 4)
    S = pos.shape[0]
    Si = S // N
    dev = pos.device
    cs = torch.tensor(2.0, dtype=torch.float32, device=dev) / torch.tensor(float(box_warp), dtype=torch.float32, device=dev)
    p = (pos[:, :3].float() * cs).double()
    present = ~torch.isnan(pos[:, 0])
    rows_all = torch.arange(S, device=dev)
    out = {k: [] for k in ('n', 'pl', 'y', 'x', 'w', 'row', 'x0', 'y0', 'i', 'j')}
    for pl, (a, b) in enumerate(((0, 1), (0, 2), (2, 0))):
        u, v = p[:, a], p[:, b]
        ix, iy = ((u + 1) * Wp - 1) / 2, ((v + 1) * Hp - 1) / 2
        fx, fy = torch.floor(ix), torch.floor(iy)
        ok = present & torch.isfinite(ix) & torch.isfinite(iy) & (fx >= -1) & (fx <= Wp - 1) & (fy >= -1) & (fy <= Hp - 1)
        r = rows_all[ok]
        ix, iy, x0, y0 = ix[ok], iy[ok], fx[ok].long(), fy[ok].long()
        wx, wy = ix - x0, iy - y0
        for j in (0, 1):
            for i in (0, 1):
                x, y = x0 + i, y0 + j
                inr = (x >= 0) & (x < Wp) & (y >= 0) & (y < Hp)
                w = (wx if i else 1 - wx) * (wy if j else 1 - wy)
                out['n'].append((r // Si)[inr]); out['pl'].append(torch.full_like(r[inr], pl)); out['y'].append(y[inr]); out['x'].append(x[inr])
                out['w'].append(w[inr]); out['row'].append(r[inr]); out['x0'].append(x0[inr]); out['y0'].append(y0[inr])
                out['i'].append(torch.full_like(r[inr], i)); out['j'].append(torch.full_like(r[inr], j))
    return {k: torch.cat(v) for k, v in out.items()}


def accumulate(pairs, rows, N, Hp, Wp, ldp, mode='bilinear', dtype=torch.float64, order=None):
    """index_add_ of the corner contributions into [N, Hp, Wp, ldp].  mode: 'bilinear' = w g (the reference), 'abs' = w |g|, 'count' = 1 per pair and
    corner.  order: a permutation of the contributions (the exactness check sums in float32 in several orders)."""
    rows = rows.reshape(-1, FC)
    sel = slice(None) if order is None else order
    n, pl, y, x, w, r = (pairs[k][sel] for k in ('n', 'pl', 'y', 'x', 'w', 'row'))
    g = rows[r].to(dtype)
    if mode == 'abs':
        g = g.abs()
    val = torch.ones_like(g) if mode == 'count' else w.to(dtype)[:, None] * g
    out = torch.zeros(N * Hp * Wp, ldp, dtype=dtype, device=rows.device)
    flat = (n * Hp + y) * Wp + x
    for q in range(3):
        m = pl == q
        blk = torch.zeros(N * Hp * Wp, FC, dtype=dtype, device=rows.device)
        blk.index_add_(0, flat[m], val[m])
        out[:, FC * q:FC * (q + 1)] = blk
    return out.reshape(N, Hp, Wp, ldp)


def scatter_ref(rows, pos, N, Hp, Wp, ldp, box_warp):
    """float64 [N, Hp, Wp, ldp]: what eg3d_triplane_scatter adds to d_planes (channels 96 .. ldp - 1 stay zero)."""
    return accumulate(corner_pairs(pos, N, Hp, Wp, box_warp), rows, N, Hp, Wp, ldp)


def unit_weight_plane(rows, pos, N, Hp, Wp, ldp, box_warp):
    """A1: |g| with weight 1 on every texel a pair's weight can move to or from when ix, iy carry an error of up to d = 2^-22 (Wp or Hp): the four
    corners of the reference's cell, and the next column / row on the side where ix +- d (iy +- d) crosses an integer -- there the kernel's fp32
    floor() may pick the neighbouring cell."""
    pos = pos.reshape(-1, 4)
    rows = rows.reshape(-1, FC)
    S = pos.shape[0]
    Si = S // N
    dev = pos.device
    cs = torch.tensor(2.0, dtype=torch.float32, device=dev) / torch.tensor(float(box_warp), dtype=torch.float32, device=dev)
    p = (pos[:, :3].float() * cs).double()
    present = ~torch.isnan(pos[:, 0])
    out = torch.zeros(N * Hp * Wp, ldp, dtype=torch.float64, device=dev)
    rid = torch.arange(S, device=dev)
    dx, dy = 2.0 ** -22 * Wp, 2.0 ** -22 * Hp
    for pl, (a, b) in enumerate(((0, 1), (0, 2), (2, 0))):
        ix, iy = ((p[:, a] + 1) * Wp - 1) / 2, ((p[:, b] + 1) * Hp - 1) / 2
        ok = present & torch.isfinite(ix) & torch.isfinite(iy) & (ix >= -1 - dx) & (ix < Wp + dx) & (iy >= -1 - dy) & (iy < Hp + dy)
        r, ix, iy = rid[ok], ix[ok], iy[ok]
        xl, xh, yl, yh = torch.floor(ix - dx).long(), torch.floor(ix + dx).long() + 1, torch.floor(iy - dy).long(), torch.floor(iy + dy).long() + 1
        g = rows[r].double().abs()
        blk = torch.zeros(N * Hp * Wp, FC, dtype=torch.float64, device=dev)
        for oy in range(3):
            for ox in range(3):
                x, y = xl + ox, yl + oy
                m = (x <= xh) & (y <= yh) & (x >= 0) & (x < Wp) & (y >= 0) & (y < Hp)
                blk.index_add_(0, (((r // Si) * Hp + y) * Wp + x)[m], g[m])
        out[:, FC * pl:FC * (pl + 1)] = blk
    return out.reshape(N, Hp, Wp, ldp)


def tolerance_planes(rows, pos, N, Hp, Wp, ldp, box_warp):
    """(A1, Aw, cnt) of within_tol, float64 [N, Hp, Wp, ldp] each."""
    pairs = corner_pairs(pos, N, Hp, Wp, box_warp)
    return (unit_weight_plane(rows, pos, N, Hp, Wp, ldp, box_warp), accumulate(pairs, rows, N, Hp, Wp, ldp, mode='abs'),
            accumulate(pairs, rows, N, Hp, Wp, ldp, mode='count'))


def within_tol(got, ref, A1, Aw, cnt, Hp, Wp, f16, amax=0.0):
    """Elementwise bound per (texel, channel); returns (every element within its bound, the largest err / tol).

        tol = 2^-22 (Hp + Wp) A1 + 2^-23 (cnt + 2) Aw    [+ 2^-19 Aw + 2^-40 amax cnt    for the fp16 arithmetic]

    Derivation (u = 2^-24, the unit roundoff of fp32; the reference and the kernel start from the same fp32 coordinate p = pos * (2 / box_warp)).
    1. Position.  The kernel forms ix = ((p + 1) Wp - 1) / 2 in fp32: three roundings of values of magnitude <= 2, 2 Wp, 2 Wp for a cell that
       touches the plane, i.e. |d ix| <= (2 u Wp + 2 u Wp + 2 u Wp) / 2 = 3 u Wp < 2^-22 Wp, and |d iy| < 2^-22 Hp.  A corner's weight is a product
       of a factor in x and a factor in y, both in [0, 1]: it changes by at most |d ix| + |d iy|, whichever corner, and that amount MOVES between
       neighbouring texels -- so the bound carries |g| with weight ONE on every texel the pair can reach (A1, unit_weight_plane), not the bilinear
       weight.  This also covers the cases where the rounding crosses an integer (the kernel's cell is the neighbour; the weight on the far texels
       is below |d ix|) and where it crosses the plane's border (a dropped or kept corner of weight below |d ix|).  The kernel's 1 - wx, 1 - wy and
       their product add three more roundings of numbers <= 1: 3 u per corner, and the fp16 subnormal tails of tiny weights 2^-35; the slack
       (2^-22 - 3 u)(Hp + Wp) = u (Hp + Wp) covers them for Hp + Wp >= 4 (asserted).
    2. Sum.  A texel's value is the sum of cnt products w g -- each rounded once, or exact and rounded on accumulation -- added in some order on
       the matrix cores (fp32 accumulator), and then at most two atomic additions (a texel row receives the lower half of one list and the upper
       half of the next; tiles share a column).  The standard bound for cnt + 2 roundings of partial sums that never exceed Aw = sum w |g| is
       (cnt + 2) u Aw; 2^-23 = 2 u allows an accumulator that truncates instead of rounding to nearest.
    3. fp16 arithmetic: 1024 w = hw + lw and g S = h + l 2^-11 with hw, h rounded toward zero to 11 bits (remainder < 2^-10 relative) and lw, l the
       remainders rounded to 11 bits (2^-21 relative to the operand each); the product lw (l 2^-11) <= 2^-10 2^-10 is dropped.  Together
       (2^-21 + 2^-21 + 2^-20)(1 + ...) < 2^-19 relative to w |g|: 2^-19 Aw.  The three products of a pair are exact in the fp32 accumulator's
       input (11 x 11 bits), and 3 cnt / 16 matrix instructions round fewer times than the cnt + 2 of point 2.
    4. fp16 subnormals: g S is at most 2^14 for max|g| = amax, and a value below 2^-14 has h and l rounded to multiples of 2^-24 (l: of g S 2^11):
       an absolute error of at most 2^-36 in g S, i.e. 2^-36 2^-13 amax = 2^-49 amax in g, per pair and corner of weight <= 1.  2^-40 amax cnt is
       the bound of the issue that asked for this test; it is kept (512 times the derived one, and still 2^-40 of the largest gradient).
    No constant comes from what the kernel returns."""
    assert Hp + Wp >= 4
    ref = ref.double()
    err = (got.double() - ref).abs()
    tol = 2.0 ** -22 * (Hp + Wp) * A1 + 2.0 ** -23 * (cnt + 2) * Aw
    if f16:
        tol = tol + 2.0 ** -19 * Aw + 2.0 ** -40 * float(amax) * cnt
    bad = ~(err <= tol)                              # (also catches NaN)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    return (not bool(bad.any())), float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------- exact class
# Why a float64 result can be demanded bit for bit of both arithmetics, both builds and any summation order:
#   * box_warp = 2: the scale 2 / box_warp is 1, p = pos.
#   * Hp, Wp are powers of two with ratio <= 2, and a coordinate is (m + 4) / (4 side) - 1 for an integer m and side = the plane side of the axis it
#     is built for: few-bit dyadic numbers, so (p + 1) W - 1 and its half are exact in fp32 and ix = (m + 4) W / (8 side) - 1/2: m / 8 on a plane
#     side equal to `side`, m / 4 + 1/2 on twice and m / 16 - 1/4 on half that side.  x is used with Wp (planes 0, 1) and Hp (plane 2), z with Hp
#     (plane 1) and Wp (plane 2), y with Hp.  Weights wx, 1 - wx, wy, 1 - wy are therefore multiples of 1/16 at worst and their products multiples
#     of 1/256, exact in fp32.
#   * fp16 arithmetic: 1024 w is a multiple of 4 up to 1024, at most 9 significant bits (odd multiples of 4 up to 1024 need 8; 9 is a safe count):
#     hw = 1024 w exactly, lw = 0, hw 2^-11 >= 2^-9 is a normal fp16.  Gradients are integers in [-8, 8] with 8 attained, so amax = 8 exactly, the
#     operand scale is S = 2^10, g S <= 2^13 has 4 significant bits: h = g S exactly, l = 0.  The only non-zero product hw h is a multiple of 2^12.
#   * every partial sum, in any order and grouping, is then an integer multiple of 1/256 (2^12 in the scaled fp16 units) of magnitude at most
#     8 cnt + |start|: exact in fp32 while that stays below 2^24 / 256 = 65536 -- cnt <= 8191 pairs per texel with |start| <= 8 (checked by
#     tests/test_scatter_cpu.py).  The deterministic build's fixed-point accumulator is exact for any fp32 inputs.
EXACT_GMAX = 8
EXACT_MAX_PAIRS = 8191


def _coord(m, side):
    return (m.double() + 4) / (4 * side) - 1


def _exact_rows(S, present, gen, dev):
    rows = torch.randint(-EXACT_GMAX, EXACT_GMAX + 1, (S, FC), generator=gen).float()
    first = int(torch.nonzero(present)[0])
    rows[first, 0] = EXACT_GMAX                   # max|g| attained on a present row: amax = 8 exactly
    return rows.to(dev)


def _finish(pos, rows, N, Hp, Wp, ray_w, rpr, dev, **extra):
    d = dict(rows=rows.to(dev).contiguous(), pos=pos.float().to(dev).contiguous(), N=N, Hp=Hp, Wp=Wp, box_warp=2.0, amax=float(EXACT_GMAX), ray_w=ray_w,
             rows_per_ray=rpr)
    d.update(extra)
    return d


def exact_case_c1(Hp, Wp, rays, rpr, ray_w, seed, dev='cpu', N=2):
    """C1: random dyadic positions with ix, iy over [-1, side) on the axis' own plane side, so cells with x0 = -1 and x0 = side - 1 occur on every
    edge and corner; a quarter of the coordinates exactly on texel centres (weights 0 and 1), an eighth of the rows with x0 in {14, 15} at a tile
    seam (each axis independently), one row in five absent (its gradient row holds other integers: reading it shows), a few rows at 1e30 and +-Inf."""
    gen = torch.Generator().manual_seed(seed)
    Si = rays * rpr
    S = N * Si
    sides = (Wp, Hp, Hp)                         # x: u of planes 0 and 1; y: v of plane 0; z: v of plane 1
    pos = torch.zeros(S, 4, dtype=torch.float64)
    for a, side in enumerate(sides):
        m = torch.randint(-8, 8 * side, (S,), generator=gen)
        centre = torch.rand(S, generator=gen) < 0.25
        m = torch.where(centre, (m // 8) * 8, m)
        if side > TS:
            seam = torch.rand(S, generator=gen) < 0.125
            k = torch.randint(1, side // TS + 1, (S,), generator=gen)
            m = torch.where(seam, 8 * (TS * k - 1) + torch.randint(0, 16, (S,), generator=gen), m)
        pos[:, a] = _coord(m, side)
    pos[:, 3] = 1.0
    far = torch.randperm(S, generator=gen)[:24]
    for q, r in enumerate(far.tolist()):
        pos[r, q % 3] = (1e30, -1e30, math.inf, -math.inf)[q % 4]
    absent = torch.rand(S, generator=gen) < 0.2
    absent[0] = False
    pos[absent, 0] = math.nan
    rows = _exact_rows(S, ~absent, gen, 'cpu')
    return _finish(pos, rows, N, Hp, Wp, ray_w, rpr, dev)


C2_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 4096, 4097, 5000)


def exact_case_lists(plane, lengths=C2_LENGTHS, seed=0, dev='cpu', N=2, Hp=256, Wp=256, Si=24576, poison=False):
    """C2: for each L of `lengths`, L rows of every image share one (tile, upper texel row) list of plane `plane`: list j sits in tile (tx, ty) =
    (j, (j + 3) % 17) with upper texel row y0 = 15 ty + j -- except list 0 of image 1, which has y0 = -1 (the list of the cells half above the
    plane).  Its rows have x0 anywhere in the tile's 15 columns (x0 = -1 included for tx = 0) and 8 sub-texel offsets on each axis.
    The third coordinate is 1e30, so plane 0's lists leave planes 1 and 2 empty; a list of plane 1 (x, z) or 2 (z, x) also lands, transposed, on the
    other of the two.  Row ids are a random subset of the image's rows, the others are absent.  One call holds all lists.
    poison (C6): row 0 of image 1 is absent and its gradient row is NaN; one more absent row per image holds Inf."""
    assert Hp == 256 and Wp == 256 and sum(lengths) < Si
    gen = torch.Generator().manual_seed(1000 + seed + 10 * plane)
    S = N * Si
    pos = torch.full((S, 4), math.nan, dtype=torch.float64)
    pos[:, 3] = 1.0
    ua, va = ((0, 1), (0, 2), (2, 0))[plane]
    oa = 3 - ua - va
    present = torch.zeros(S, dtype=torch.bool)
    for n in range(N):
        ids = torch.randperm(Si - 1, generator=gen)[:sum(lengths)] + 1          # row 0 of every image stays absent
        at = 0
        for j, L in enumerate(lengths):
            r = ids[at:at + L] + n * Si
            at += L
            tx, ty = j, (j + 3) % 17
            y0 = ty * TS + j
            if j == 0 and n == 1:
                y0 = -1
            lo = -8 if tx == 0 else 8 * TS * tx
            mx = torch.randint(lo, 8 * TS * (tx + 1), (L,), generator=gen)
            my = 8 * y0 + torch.randint(0, 8, (L,), generator=gen)
            pos[r, ua], pos[r, va], pos[r, oa] = _coord(mx, Wp), _coord(my, Hp), 1e30
            present[r] = True
    pos[~present, 0] = math.nan
    if not poison:                              # row 0 of image 0 present (a legitimate row 0), anywhere on the plane
        pos[0, :3] = _coord(torch.tensor([100, 200, 300]), 256)
        present[0] = True
    rows = _exact_rows(S, present, gen, 'cpu')
    if poison:
        rows[Si] = math.nan                     # image 1's row 0: absent, never to be read
        rows[0] = math.nan                      # image 0's likewise
        other = torch.nonzero(~present)
        for n in range(N):
            o = int(other[(other >= n * Si) & (other < (n + 1) * Si)][7])
            rows[o] = math.inf
            rows[o, 1::2] = -math.inf
    return _finish(pos, rows, N, Hp, Wp, 32, 48, dev)


def exact_start(N, Hp, Wp, ldp, seed, dev='cpu'):
    """Start value of d_planes (the contract is +=): small integers; channels 96 .. ldp - 1 hold a sentinel that must come back unchanged."""
    gen = torch.Generator().manual_seed(77 + seed)
    st = torch.randint(-8, 9, (N, Hp, Wp, ldp), generator=gen).float()
    st[..., 3 * FC:] = 12345.0
    return st.to(dev)


# ---------------------------------------------------------------------------------------------------------------- general class
GENERAL_PLANES = ((15, 15), (30, 45), (31, 17), (2, 3), (1, 16), (270, 270), (61, 61))


def general_case(Hp, Wp, box_warp, seed, dev='cpu', N=2, rays=256, rpr=48, ray_w=16, dense=False):
    """Random fp32 positions in the box, a tenth of them up to 1.3 x outside it, randn gradients, about 10 % absent rows.
    dense: every sample inside a ball of 4 texels around the plane centre (a disc on each plane): thousands of pairs per texel."""
    gen = torch.Generator().manual_seed(seed)
    S = N * rays * rpr
    if dense:
        d = torch.randn(S, 3, generator=gen, dtype=torch.float64)
        d = d / d.norm(dim=1, keepdim=True) * torch.rand(S, 1, generator=gen, dtype=torch.float64) ** (1 / 3) * 4.0      # texels
        pc = d * 2 / torch.tensor([Wp, Hp, min(Hp, Wp)], dtype=torch.float64)           # in [-1, 1] units around the centre
    else:
        pc = torch.rand(S, 3, generator=gen, dtype=torch.float64) * 2 - 1
        out = torch.rand(S, generator=gen) < 0.1
        pc[out] = pc[out] * 1.3
    pos = torch.cat([pc * (box_warp / 2), torch.ones(S, 1, dtype=torch.float64)], 1).float()
    absent = torch.rand(S, generator=gen) < 0.1
    pos[absent, 0] = math.nan
    rows = torch.randn(S, FC, generator=gen)
    return dict(rows=rows.to(dev).contiguous(), pos=pos.to(dev).contiguous(), N=N, Hp=Hp, Wp=Wp, box_warp=float(box_warp), amax=float(rows.abs().max()),
                ray_w=ray_w, rows_per_ray=rpr)
