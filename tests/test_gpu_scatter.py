"""eg3d_triplane_scatter (csrc/renderer.hip) on its own, through hipops.triplane_scatter, against the float64 adjoint of tests/support/scatter_ref.py
(the reference's counterpart: autograd of F.grid_sample w.r.t. the planes, training/volumetric_rendering/renderer.py:64; checked in
tests/test_scatter_cpu.py).

  * exact class (C1 .. C6): inputs for which every product and partial sum is exactly representable, so both arithmetics (fp32 products,
    amax=None; three fp16 products, amax = max|rows|), both builds and any summation order must return the float64 result BIT FOR BIT --
    the comparison that notices one lost, doubled or misplaced pair in a list of thousands;
  * general class: random fp32 positions and randn gradients under the derived elementwise bound scatter_ref.within_tol;
  * the same file once more in a fresh interpreter under the deterministic build, where it also asserts run-to-run and walk-to-walk bit identity
    and det_misses() == 0.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import scatter_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
ARITH = ['fp32', 'fp16']


def _scatter(case, start, f16, hint=True, amax=None):
    """One library call on a copy of `start` ([N, Hp, Wp, ldp]); returns the result in the same layout."""
    from inv3d_amd import hipops
    buf = start.clone()
    d_planes = buf.permute(0, 3, 1, 2)
    am = None
    if f16:
        am = torch.tensor([case['amax'] if amax is None else amax], dtype=torch.float32, device=DEV)
    rw, rpr = hint if isinstance(hint, tuple) else ((case['ray_w'], case['rows_per_ray']) if hint else (0, 0))
    hipops.triplane_scatter(case['rows'], case['pos'], d_planes, case['box_warp'], ray_w=rw, rows_per_ray=rpr, amax=am)
    torch.cuda.synchronize()
    return buf


@functools.lru_cache(maxsize=2)
def _exact(kind, *args):
    """(case, {ldp: (start, expected fp32)}) of an exact-class case; the reference is computed once per case."""
    if kind == 'c1':
        Hp, Wp, rays, rpr, ray_w = args
        case = R.exact_case_c1(Hp, Wp, rays, rpr, ray_w, seed=Hp * 1000 + Wp + rpr, dev=DEV)
    else:
        plane, poison = args
        case = R.exact_case_lists(plane, lengths=(5, 33, 100) if poison else R.C2_LENGTHS, dev=DEV, poison=poison)
    return case, {}


def _expected(case, cache, ldp):
    if ldp not in cache:
        start = R.exact_start(case['N'], case['Hp'], case['Wp'], ldp, seed=ldp, dev=DEV)
        ref = R.scatter_ref(case['rows'], case['pos'], case['N'], case['Hp'], case['Wp'], ldp, case['box_warp'])
        assert torch.isfinite(ref).all()
        cache[ldp] = (start, (start.double() + ref).float())
    return cache[ldp]


def _assert_equal(got, want, what):
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        nan = int(torch.isnan(got).sum())
        i = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {bad.shape[0]} of {got.numel()} elements differ ({nan} NaN); first at [n, y, x, c] = {i}: '
                             f'got {float(got[i])!r}, expected {float(want[i])!r}')
    assert torch.equal(got[..., 96:], want[..., 96:])


C1_SHAPES = [(16, 16, 256, 32, 16), (32, 64, 512, 48, 32), (64, 32, 512, 48, 32), (256, 256, 512, 48, 32)]


@pytest.mark.parametrize('arith', ARITH)
@pytest.mark.parametrize('shape', C1_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_exact_c1_random_dyadic_positions(shape, arith):
    """C1: cells on every edge, corner and tile seam, texel centres, absent rows, 1e30 and +-Inf coordinates; ldp = 128 with a sentinel in channels
    96 .. 127 and integer start values (the contract is +=)."""
    case, cache = _exact('c1', *shape)
    start, want = _expected(case, cache, 128)
    _assert_equal(_scatter(case, start, arith == 'fp16'), want, f'C1 {shape[:2]} {arith}')


@pytest.mark.parametrize('arith', ARITH)
@pytest.mark.parametrize('plane', [0, 1, 2])
def test_exact_c2_list_lengths(plane, arith):
    """C2: lists of exactly 1, 15 .. 17, 63 .. 65, 127 .. 129, 200, 4096, 4097 and 5000 pairs in one call (ends of a 16-pair group and of a 64-pair
    super-step; 4097 and 5000 take the deterministic build's in-global sort), on each plane."""
    case, cache = _exact('lists', plane, False)
    start, want = _expected(case, cache, 128)
    _assert_equal(_scatter(case, start, arith == 'fp16'), want, f'C2 plane {plane} {arith}')


@pytest.mark.parametrize('arith', ARITH)
def test_exact_c3_walks_of_the_binning_pass(arith):
    """C3: the brick walk with 24-row bricks (32, 48), a hint that falls back (32, 40) and no hint on a 512 x 48 layout; 16-row bricks (32, 32) and
    no hint on a 512 x 32 layout: all the float64 result, hence equal to each other."""
    f16 = arith == 'fp16'
    case, cache = _exact('c1', 32, 64, 512, 48, 32)
    start, want = _expected(case, cache, 128)
    for hint in ((32, 48), (32, 40), (0, 0)):
        _assert_equal(_scatter(case, start, f16, hint=hint), want, f'C3 512 x 48, hint {hint}, {arith}')
    case, cache = _exact('c1', 32, 64, 512, 32, 32)
    start, want = _expected(case, cache, 128)
    for hint in ((32, 32), (0, 0)):
        _assert_equal(_scatter(case, start, f16, hint=hint), want, f'C3 512 x 32, hint {hint}, {arith}')


@pytest.mark.parametrize('arith', ARITH)
@pytest.mark.parametrize('ldp', [96, 128])
def test_exact_c4_plane_pitch(ldp, arith):
    case, cache = _exact('c1', 16, 16, 256, 32, 16)
    start, want = _expected(case, cache, ldp)
    _assert_equal(_scatter(case, start, arith == 'fp16'), want, f'C4 ldp {ldp} {arith}')


def test_exact_c5_zero_gradients_with_zero_amax():
    """C5: all-zero gradients and amax = 0 on the fp16 arithmetic: exactly the start values, no NaN from the operand scale."""
    case, cache = _exact('c1', 16, 16, 256, 32, 16)
    start, _ = _expected(case, cache, 128)
    zero = dict(case, rows=torch.zeros_like(case['rows']))
    got = _scatter(zero, start, True, amax=0.0)
    assert not torch.isnan(got).any()
    _assert_equal(got, start, 'C5')


@pytest.mark.parametrize('arith', ARITH)
def test_exact_c6_rows_of_absent_samples_are_never_read(arith):
    """C6: row 0 of both images is absent and its gradient row is NaN, one more absent row per image holds +-Inf, and the lists (5, 33 and 100
    pairs) end inside a 16-pair group, so that the accumulate kernels pad them.  The padding must not read row 0: before the padding record
    carried the row id of the list's first record, 0 x NaN from the padded lanes turned both texel rows of every padded list into NaN."""
    case, cache = _exact('lists', 0, True)
    assert torch.isnan(case['rows'][0]).all() and torch.isnan(case['pos'][0, 0])
    start, want = _expected(case, cache, 128)
    got = _scatter(case, start, arith == 'fp16')
    assert torch.isfinite(got).all(), f'C6 {arith}: {int((~torch.isfinite(got)).sum())} non-finite elements'
    _assert_equal(got, want, f'C6 {arith}')


# ------------------------------------------------------------------------------------------------------------------ general class
@functools.lru_cache(maxsize=1)
def _general(i):
    Hp, Wp = R.GENERAL_PLANES[i]
    case = R.general_case(Hp, Wp, (1.0, 2.5)[i % 2], seed=500 + i, dev=DEV, dense=(Hp, Wp) == (61, 61))
    ref = R.scatter_ref(case['rows'], case['pos'], 2, Hp, Wp, 96, case['box_warp'])
    return case, ref, R.tolerance_planes(case['rows'], case['pos'], 2, Hp, Wp, 96, case['box_warp'])


@pytest.mark.parametrize('i', range(len(R.GENERAL_PLANES)), ids=[f'{h}x{w}' for h, w in R.GENERAL_PLANES])
def test_general_class_within_the_derived_bound(i):
    """Random positions (a tenth outside the box), randn gradients, ~10 % absent rows: both arithmetics, with and without the walk hint, each
    element within scatter_ref.within_tol.  Deterministic build: two calls, and the four walks of the binning pass (24-row bricks, 16-row bricks, a
    hint that falls back, no hint), are bit-identical."""
    from inv3d_amd import _lib as L
    case, ref, (A1, Aw, cnt) = _general(i)
    Hp, Wp = case['Hp'], case['Wp']
    start = torch.zeros(2, Hp, Wp, 96, device=DEV)
    for f16 in (False, True):
        outs = []
        for hint in (True, False):
            got = _scatter(case, start, f16, hint=hint)
            ok, ratio = R.within_tol(got, ref, A1, Aw, cnt, Hp, Wp, f16, case['amax'])
            print(f'scatter general {Hp}x{Wp} box_warp {case["box_warp"]} {"fp16" if f16 else "fp32"} hint {int(hint)}: max pairs per texel {int(cnt.max())}, '
                  f'max err/tol {ratio:.4f}{" (deterministic build)" if L.DETERMINISTIC else ""}')
            assert ok, (Hp, Wp, f16, hint, ratio)
            outs.append(got)
        if L.DETERMINISTIC:
            assert torch.equal(outs[0], outs[1]), 'the walks differ under the deterministic build'
            for hint in ((16, 16), (16, 40)):       # the same rows read as 768 rays x 16 rows: 16-row bricks; a hint that falls back to consecutive rows
                assert torch.equal(outs[0], _scatter(case, start, f16, hint=hint)), f'walk {hint} differs under the deterministic build'
            assert torch.equal(outs[0], _scatter(case, start, f16, hint=True)), 'two calls differ under the deterministic build'
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def test_deterministic_build_has_no_misses():
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again: C2's 4097 and 5000 lists reach
    scatter_sort16_kernel's in-global sort there."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_scatter.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
