"""The yardstick of tests/test_gpu_scatter.py, checked without a GPU: tests/support/scatter_ref.py equals the float64 autograd gradient of
F.grid_sample w.r.t. the planes (what the reference's renderer differentiates, training/volumetric_rendering/renderer.py:64); the exact-class
builders really are exact in fp32 under any summation order; the two comparisons reject six deliberately wrong scatters; and
eg3d_triplane_scatter refuses planes beyond 270 x 270 from its arguments alone."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import scatter_ref as R      # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('Hp,Wp,box_warp', [(31, 17, 2.5), (16, 16, 1.0)])
def test_reference_equals_the_autograd_gradient_of_grid_sample(Hp, Wp, box_warp):
    N, Si = 2, 600
    gen = torch.Generator().manual_seed(Hp)
    pos = ((torch.rand(N * Si, 4, generator=gen) * 2 - 1) * (box_warp / 2) * 1.4).float()           # out-of-range points included
    pos[:40, 1] = 3.0 * box_warp                                                                 # far outside on one axis only
    absent = torch.rand(N * Si, generator=gen) < 0.15
    pos[absent, 0] = float('nan')
    rows = torch.randn(N * Si, R.FC, generator=gen)
    ref = R.scatter_ref(rows, pos, N, Hp, Wp, 96, box_warp)
    cs = torch.tensor(2.0) / torch.tensor(box_warp)
    p = (torch.nan_to_num(pos[:, :3], nan=0.0) * cs).double().reshape(N, Si, 3)
    g = torch.where(absent[:, None], torch.zeros_like(rows), rows).double().reshape(N, Si, R.FC)
    for pl, (a, b) in enumerate(((0, 1), (0, 2), (2, 0))):
        planes = torch.zeros(N, R.FC, Hp, Wp, dtype=torch.float64, requires_grad=True)
        out = F.grid_sample(planes, torch.stack([p[..., a], p[..., b]], -1)[:, None], mode='bilinear', padding_mode='zeros', align_corners=False)
        (out[:, :, 0].permute(0, 2, 1) * g).sum().backward()
        want = planes.grad.permute(0, 2, 3, 1)
        got = ref[..., R.FC * pl:R.FC * (pl + 1)]
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), pl
        assert float(want.abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------------------------ exactness of the exact class
def _exact_cases():
    yield 'C1 16x16', R.exact_case_c1(16, 16, 256, 32, 16, seed=16016 + 32)
    yield 'C1 32x64', R.exact_case_c1(32, 64, 512, 48, 32, seed=32064 + 48)
    yield 'C1 64x32', R.exact_case_c1(64, 32, 512, 48, 32, seed=64032 + 48)
    yield 'C2 plane 0', R.exact_case_lists(0)
    yield 'C2 plane 2', R.exact_case_lists(2)
    yield 'C6', R.exact_case_lists(0, lengths=(5, 33, 100), poison=True)


@pytest.mark.parametrize('name,case', list(_exact_cases()), ids=[n for n, _ in _exact_cases()])
def test_exact_class_is_exact_in_fp32_under_any_order(name, case):
    N, Hp, Wp = case['N'], case['Hp'], case['Wp']
    pairs = R.corner_pairs(case['pos'], N, Hp, Wp, 2.0)
    ref = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96)
    assert torch.isfinite(ref).all()
    cnt = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96, mode='count')
    assert int(cnt.max()) <= R.EXACT_MAX_PAIRS, int(cnt.max())
    present = ~torch.isnan(case['pos'][:, 0])
    assert float(case['rows'][present].abs().max()) == R.EXACT_GMAX == case['amax']
    # coordinates and weights are what the derivation says: the kernel's fp32 evaluation of ix / iy is exact, weights are multiples of 1/16
    p32 = case['pos'][present][:, :3]
    p32 = p32[(p32.abs() < 4).all(1)]
    for side in (Hp, Wp):
        assert torch.equal((((p32 + 1) * side - 1) * 0.5).double(), ((p32.double() + 1) * side - 1) / 2)
    assert torch.equal((pairs['w'] * 256).round(), pairs['w'] * 256)
    assert torch.equal(ref.float().double(), ref)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        order = torch.randperm(pairs['w'].numel(), generator=gen)
        got = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96, dtype=torch.float32, order=order)
        assert torch.equal(got, ref.float()), name
    if name.startswith('C2'):       # image 1's lists of the plane have exactly the lengths asked for (image 0 has one more present row, its row 0)
        pl = int(name[-1])
        m = (pairs['pl'] == pl) & (pairs['n'] == 1)
        x0 = torch.full((case['pos'].shape[0],), -99, dtype=torch.long)
        y0 = x0.clone()
        x0[pairs['row'][m]], y0[pairs['row'][m]] = pairs['x0'][m], pairs['y0'][m]
        key = (x0.clamp_min(0) // R.TS) * 1000 + y0 + 1
        assert sorted(torch.unique(key[x0 > -99], return_counts=True)[1].tolist()) == sorted(R.C2_LENGTHS)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _mutants(pairs, N, Hp, Wp, long_list):
    """name -> corner contributions of a deliberately wrong scatter.  long_list: a mask selecting the corners of one long list."""
    def clone(**kw):
        d = dict(pairs)
        d.update(kw)
        return d
    idx = torch.nonzero(long_list & (pairs['w'] > 0.2))[0]
    one = (pairs['row'] == pairs['row'][idx]) & (pairs['pl'] == pairs['pl'][idx])                 # the corners of one (row, plane) pair
    yield 'one pair dropped', {k: v[~one] for k, v in pairs.items()}
    yield 'one pair doubled', {k: torch.cat([v, v[one]]) for k, v in pairs.items()}
    # plane 2 read as (x, z) instead of (z, x): its texel coordinates transposed (square planes only)
    if Hp == Wp:
        p2 = pairs['pl'] == 2
        yield 'plane 2 read as (x, z)', clone(x=torch.where(p2, pairs['y'], pairs['x']), y=torch.where(p2, pairs['x'], pairs['y']))
    # a tile's accumulator column 15 (texel 15 t + 15 = column 0 of tile t + 1) written as if that tile began one texel later: at texel 15 t + 16
    seam = (pairs['x'] % R.TS == 0) & (pairs['x'] > 0) & (pairs['i'] == 1) & (pairs['x'] + 1 < Wp)
    assert seam.any()
    yield 'column 15 of a tile written one texel further', clone(x=torch.where(seam, pairs['x'] + 1, pairs['x']))
    # wx and 1 - wx swapped: the two columns of a cell exchange their weights (cells with both columns inside the plane)
    x_in = (pairs['x0'] >= 0) & (pairs['x0'] < Wp - 1)
    yield 'wx and 1 - wx swapped', clone(x=torch.where(x_in, pairs['x0'] + 1 - pairs['i'], pairs['x']))
    yield 'image 1 written to image 0', clone(n=torch.zeros_like(pairs['n']))


def test_exact_comparison_rejects_wrong_scatters():
    case = R.exact_case_lists(2)
    N, Hp, Wp = 2, 256, 256
    pairs = R.corner_pairs(case['pos'], N, Hp, Wp, 2.0)
    ref = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96).float()
    long_list = (pairs['pl'] == 2) & (pairs['n'] == 1) & (pairs['x0'] // R.TS == 13) & (pairs['x0'] >= 0)       # the 5000-pair list
    assert int((long_list & (pairs['i'] == 0) & (pairs['j'] == 0)).sum()) == 5000
    names = []
    for name, bad in _mutants(pairs, N, Hp, Wp, long_list):
        wrong = R.accumulate(bad, case['rows'], N, Hp, Wp, 96).float()
        assert not torch.equal(wrong, ref), name
        names.append(name)
    assert len(names) == 6


def test_derived_bound_accepts_fp32_noise_and_rejects_wrong_scatters():
    """General class, dense lists (61 x 61, all samples within 4 texels of the centre: thousands of pairs per texel) and sparse ones (31 x 17).
    The float32 evaluation of the same sum passes the bound; each wrong scatter -- one pair of thousands dropped or doubled included -- fails it."""
    for Hp, Wp, dense in ((61, 61, True), (31, 17, False)):
        case = R.general_case(Hp, Wp, 2.5, seed=9, dense=dense)
        N = 2
        pairs = R.corner_pairs(case['pos'], N, Hp, Wp, 2.5)
        ref = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96)
        A1, Aw, cnt = R.tolerance_planes(case['rows'], case['pos'], N, Hp, Wp, 96, 2.5)
        f32 = R.accumulate(pairs, case['rows'], N, Hp, Wp, 96, dtype=torch.float32)
        for f16 in (False, True):
            ok, ratio = R.within_tol(f32, ref, A1, Aw, cnt, Hp, Wp, f16, case['amax'])
            assert ok and ratio < 1.0, (Hp, Wp, f16, ratio)
        if dense:
            assert int(cnt.max()) >= 1000
            centre = (pairs['x0'] == 30) & (pairs['y0'] == 30)
        else:
            centre = (pairs['x0'] == R.TS - 1)
        n = 0
        for name, bad in _mutants(pairs, N, Hp, Wp, centre & (pairs['pl'] == 0) & (pairs['n'] == 1)):
            wrong = R.accumulate(bad, case['rows'], N, Hp, Wp, 96)
            ok, ratio = R.within_tol(wrong.float(), ref, A1, Aw, cnt, Hp, Wp, True, case['amax'])           # the wider (fp16) bound
            assert not ok and ratio > 1.0, (Hp, Wp, name, ratio)
            n += 1
        assert n == (6 if Hp == Wp else 5)
    nan = ref.clone().float()
    nan[0, 0, 0, 0] = float('nan')
    assert not R.within_tol(nan, ref, A1, Aw, cnt, Hp, Wp, True, case['amax'])[0]


# ------------------------------------------------------------------------------------------------------------------ refusals at the limit
def test_triplane_scatter_refuses_planes_beyond_270_from_the_arguments_alone():
    """3 * ceil(Hp / 15) * ceil(Wp / 15) * 16 <= 16384 lists: 270 x 270 is the last supported plane (3 * 18 * 18 * 16 = 15552); 270 x 271 and
    271 x 271 are refused by both libraries before any HIP call (fake addresses: never dereferenced)."""
    from inv3d_amd import _lib as L
    INVALID, UNSUPPORTED = -1, -2
    libs = [L.lib()]
    if not L.DETERMINISTIC:
        det = C.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), 'libeg3d_hip_det.so'))
        for fn in ('eg3d_triplane_scatter', 'eg3d_triplane_scatter_workspace_ints'):
            getattr(det, fn).restype, getattr(det, fn).argtypes = getattr(L.lib(), fn).restype, getattr(L.lib(), fn).argtypes
        libs.append(det)
    a = 0x10000
    for lib in libs:
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 270, 271, 96, 1.0, a, 0, 0, None, None) == UNSUPPORTED
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 271, 270, 96, 1.0, a, 0, 0, None, None) == UNSUPPORTED
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 271, 271, 96, 1.0, a, 0, 0, None, None) == UNSUPPORTED
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 270, 270, 96, 1.0, None, 0, 0, None, None) == INVALID     # 270 x 270 itself gets as far as the null check
        S = 2 * 12288
        assert lib.eg3d_triplane_scatter_workspace_ints(S, 2, 270, 270) == 3 * (3 * 18 * 18 * 16) + 1 + 3 + 12 * S
