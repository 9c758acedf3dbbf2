"""Shape views without a GPU: the numpy restatement of the iso-surface marcher (tests/support/iso_ref.py, what tests/test_gpu_shape_render.py
requires the GPU outputs to equal bit for bit) checked against things that are not ours -- its own result without empty-space skipping, the
analytic ray-sphere intersection -- and the host side: inference.grid_frame against density_grid's layout, eg3d_iso_params against the header,
argument validation of the two entries."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import iso_ref as R  # noqa: E402
from inv3d_amd import inference as I  # noqa: E402

N, R0 = 64, 20.0
SPACING = 1.0 / (N - 1)                                 # the grid spans [-0.5, 0.5]^3; one voxel = SPACING world units
FRAME = dict(origin=(-0.5, -0.5, -0.5), spacing=(SPACING,) * 3, axes=(0, 1, 2))
CENTRE = (N - 1) / 2


def sphere_field(noise=0.0, seed=0):
    """r0 - |p - centre| in voxel units on the 64^3 grid (+ N(0, noise))."""
    i = np.arange(N, dtype=np.float64) - CENTRE
    f = R0 - np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    if noise:
        f = f + np.random.RandomState(seed).normal(0.0, noise, f.shape)
    return f.astype(np.float32)


def camera(yaw=math.pi / 2, pitch=math.pi / 2, radius=2.7, focal=3.0):
    """[1,25]: a lookat_pose camera on the sphere of `radius` (outside the grid); focal 3 sees the whole sphere and misses around it."""
    m = I.lookat_pose(yaw, pitch, (0., 0., 0.), radius).reshape(16)
    return torch.cat([m, torch.tensor([focal, 0, 0.5, 0, focal, 0.5, 0, 0, 1.])]).reshape(1, 25).numpy().astype(np.float32)


@pytest.mark.parametrize('noise', [0.0, 0.3])
def test_skipping_is_bit_identical(noise):
    """The contract of the empty-space skipping: hit index and depth bits (and everything derived from them) equal with skip on and off, on
    the 64^3 sphere and on the sphere + N(0, 0.3) noise, 64^2 rays, two views."""
    vol = sphere_field(noise)
    for cam in (camera(), camera(math.pi / 2 + 0.4, math.pi / 2 - 0.3)):
        a = R.march(vol, cam, 64, 0.0, skip=True, **FRAME)
        b = R.march(vol, cam, 64, 0.0, skip=False, **FRAME)
        assert 0 < a['mask'].sum() < a['mask'].size
        assert np.array_equal(a['hit_k'], b['hit_k'])
        for k in ('depth', 'normal', 'shade'):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert a['evals'] * 2 < b['evals'], (a['evals'], b['evals'])          # skipping saves at least half of the field evaluations here
        print(f'noise {noise}: field evaluations {b["evals"]} -> {a["evals"]} ({b["evals"] / a["evals"]:.2f}x)')


def test_bricks_are_the_dilated_maxima():
    """bricks() (separable passes) against the definition evaluated directly, on a grid whose sides end on, before and after a brick boundary,
    with NaN and -0 in it."""
    rng = np.random.RandomState(1)
    vol = rng.normal(size=(17, 18, 10)).astype(np.float32)
    vol[3, 4, 5] = np.nan
    vol[8:, :, :] = np.minimum(vol[8:, :, :], 0) * 0 - 0.0                    # a block of -0
    got = R.bricks(vol)
    assert got.shape == (2, 3, 2) == R.bricks_shape(vol.shape)
    for b in np.ndindex(*got.shape):
        sl = tuple(slice(max(8 * b[a] - 1, 0), min(8 * b[a] + 9, vol.shape[a] - 1) + 1) for a in range(3))
        want = np.nanmax(vol[sl])
        assert got[b] == want and not np.signbit(got[b]), b
    allnan = np.full((2, 2, 2), np.nan, np.float32)
    assert R.bricks(allnan)[0, 0, 0] == -np.inf


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_analytic_sphere(dtype):
    """Field r0 - |p|, r0 = 20 voxels, sampled on the 64^3 grid, cameras outside it, step 0.5 voxel, refine 4.

    Hit / miss: a ray whose closest approach b to the centre differs from r0 by more than one step (0.5 voxel) must agree with the analytic
    ray-sphere test: with b < r0 - 0.5 the chord inside the sphere is 2 sqrt(r0^2 - b^2) > 8 voxels, many samples; with b > r0 + 0.5 the field
    along the ray stays below -0.5 + the interpolation error.

    Depth bound, derived (not tuned): trilinear interpolation of a C^2 field on unit cells errs by at most sum over the three axes of
    h^2 / 8 * max |d^2 f / dx_a^2|, h = 1; for f = r0 - |p| every second derivative is at most 1 / |p| = 1 / r0 at the surface:
    3 / (8 r0) = 0.01875.  |grad f| = 1, so the interpolated surface lies within 0.01875 voxel of the sphere along the normal, and within
    0.01875 / cos along a ray of incidence cosine cos; for cos >= 0.5: 0.0375 voxel.  (After 4 halvings the bracket is 1/32 voxel and the secant
    step's residual on it is of order curvature * bracket^2 < 1e-4; fp32 rounding of a depth near 2.7 is 2.4e-7 world = 1.5e-5 voxel.)
    Observed worst error: 0.024 voxel in both precisions."""
    vol = sphere_field()
    bound = (3.0 / (8.0 * R0)) / 0.5
    assert abs(bound - 0.0375) < 1e-12
    res = 64
    checked = 0
    for cam in (camera(), camera(math.pi / 2 + 0.4, math.pi / 2 - 0.3), camera(math.pi / 2 - 0.9, math.pi / 2 + 0.5, radius=2.0, focal=2.2)):
        out = R.march(vol, cam, res, 0.0, dtype=dtype, **FRAME)
        o, d = R.rays(cam, res, np.arange(res * res), np.float64)
        oc = (o - FRAME['origin'][0]) / SPACING - CENTRE                       # origin relative to the sphere centre, in voxels
        tca = -(oc * d).sum(1)
        b = np.sqrt(np.maximum((oc * oc).sum(1) - tca * tca, 0.0))
        hit = out['mask'].astype(bool)
        sure_in, sure_out = b < R0 - 0.5, b > R0 + 0.5
        assert sure_in.any() and sure_out.any()
        assert hit[sure_in].all() and not hit[sure_out].any()
        t_exact = tca - np.sqrt(np.maximum(R0 * R0 - b * b, 0.0))              # voxels along the ray (d is a unit vector, isotropic spacing)
        nrm = (oc + t_exact[:, None] * d) / R0
        cos = -(nrm * d).sum(1)
        sel = hit & (b < R0) & (cos >= 0.5)
        err = np.abs(out['depth'][sel].astype(np.float64) / SPACING - t_exact[sel])
        print(f'{np.dtype(dtype).name}: {sel.sum()} rays, worst depth error {err.max():.4f} voxel (bound {bound})')
        assert err.max() <= bound
        # the normals of those rays are the sphere's: each central difference over +-1 voxel errs by at most 2 * 0.01875 / 2 (interpolation) +
        # 1 / (6 r0^2) (truncation) = 0.0192 per component, the length by sqrt(3) times that, so a normalised component by < 0.0192 + 0.0333
        assert (np.abs(out['normal'][sel].astype(np.float64) - nrm[sel]).max()) < 0.0525
        checked += int(sel.sum())
    assert checked > 2500


def test_pixel_subset_and_shade_modes():
    """A pixel subset gives the rows of the full result; 'normal' shading is the camera-space normal (a frontal camera sees z toward itself)."""
    vol = sphere_field()
    cams = np.concatenate([camera(), camera(math.pi / 2 + 0.4, math.pi / 2 - 0.3)])
    full = R.march(vol, cams, 16, 0.0, **FRAME)
    pix = np.random.RandomState(0).choice(2 * 16 * 16, 50, replace=False)
    part = R.march(vol, cams, 16, 0.0, pix=pix, **FRAME)
    for k in ('depth', 'normal', 'shade', 'hit_k', 'mask'):
        assert np.array_equal(full[k][pix], part[k], equal_nan=True), k
    nm = R.march(vol, cams, 16, 0.0, shade='normal', **FRAME)
    hit = nm['mask'].astype(bool)
    assert (nm['shade'][hit][:, 2] < 0).all()                                   # surface normals face the camera: camera-space z < 0
    assert (nm['shade'][~hit] == 1.0).all() and (np.abs(nm['shade']) <= 1.0 + 1e-6).all()
    assert (full['shade'][hit] >= 2 * 0.15 - 1 - 1e-6).all()


class _FakeG:
    """What density_grid touches of a generator, with sigma = a known affine function of the world point."""
    COEF = torch.tensor([1.0, 10.0, 100.0])

    def __init__(self, box):
        self.rendering_kwargs = dict(box_warp=box)
        self.decoder = None
        self.backbone = types.SimpleNamespace(synthesis=lambda ws, **kw: torch.zeros(1, 96, 4, 4))
        self.renderer = types.SimpleNamespace(run_model=lambda planes, dec, pts, dirs, kw: dict(sigma=(pts * _FakeG.COEF).sum(-1, keepdim=True)))


def test_grid_frame_is_density_grids_layout():
    """density_grid of a generator whose sigma is c . p, against c . (origin + i * spacing) of grid_frame: the difference is the reference's
    float-division skew, which moves a point by less than one voxel toward + along world x and y and not at all along z."""
    box, res = 1.0, 21
    G = _FakeG(box)
    grid = I.density_grid(G, torch.zeros(1, 14, 8), res=res, pad=0, max_batch=4000).double().numpy()
    origin, spacing, axes = I.grid_frame(G, res)
    assert axes == (0, 1, 2) and spacing[0] < 0 < spacing[1] == spacing[2] and origin == (box / 2, -box / 2, -box / 2)
    vs = box / (res - 1)
    idx = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).astype(np.float64)
    world = np.zeros_like(idx)
    for a in range(3):
        world[..., axes[a]] = origin[a] + idx[..., a] * spacing[a]
    c = _FakeG.COEF.double().numpy()
    diff = grid - (world * c).sum(-1)
    assert diff.min() > -1e-3 and diff.max() < (c[0] + c[1]) * vs + 1e-3         # 0 <= skew < one voxel on x and on y
    # and it is exactly that skew: x carries i1 / res + i2 / res^2 of a voxel, y carries i2 / res, z nothing
    skew = c[0] * vs * (idx[..., 1] / res + idx[..., 2] / res ** 2) + c[1] * vs * (idx[..., 2] / res)
    assert np.abs(diff - skew).max() < 1e-3
    # the padding of density_grid does not move the frame
    assert float(I.density_grid(G, torch.zeros(1, 14, 8), res=res, pad=2)[0, 5, 5]) == -1000.0


def test_iso_params_structure_matches_the_header():
    """eg3d_iso_params of inv3d_amd/_lib.py against its C definition (gcc), as test_host.py does for the other structures."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', ' printf("%zu\\n", sizeof(eg3d_iso_params));']
    want = [C.sizeof(L.IsoParams)]
    for f in L.IsoParams._fields_:
        src.append(f' printf("%zu\\n", offsetof(eg3d_iso_params, {f[0]}));')
        want.append(getattr(L.IsoParams, f[0]).offset)
    src += [' printf("%d %d\\n", EG3D_ISO_LAMBERT, EG3D_ISO_NORMAL);', ' return 0;', '}']
    want += [L.ISO_LAMBERT, L.ISO_NORMAL]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_entries_reject_bad_arguments_before_any_launch():
    """Both entries answer argument errors with a negative status and launch nothing (no GPU here: a launch would be an error of its own)."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    INVALID, UNSUPPORTED, TOO_LARGE = -1, -2, -3
    a = 0x1000                                                                  # a non-null pointer that is never dereferenced

    def params(**kw):
        base = dict(vol=a, bricks=a, cams=a, depth=a, D0=16, D1=16, D2=16, F=1, res=8, level=0.0, step=0.5, refine=4, skip=1, shade_mode=0,
                    ambient=0.15, background=1.0)
        axes, origin, spacing = kw.pop('axes', (0, 1, 2)), kw.pop('origin', (0., 0., 0.)), kw.pop('spacing', (1., -1., 1.))
        base.update(kw)
        p = L.IsoParams(**base)
        p.axes[:], p.origin[:], p.spacing[:] = axes, origin, spacing
        return C.byref(p)
    assert lib.eg3d_iso_bricks(None, None) == INVALID and lib.eg3d_iso_render(None, None) == INVALID
    for bad in (dict(vol=None), dict(bricks=None), dict(D1=1), dict(D0=0)):
        assert lib.eg3d_iso_bricks(params(**bad), None) == INVALID, bad
    assert lib.eg3d_iso_bricks(params(D0=2048, D1=2048, D2=512), None) == TOO_LARGE
    for bad in (dict(vol=None), dict(cams=None), dict(bricks=None), dict(D2=1), dict(F=0), dict(res=0), dict(axes=(0, 1, 1)), dict(axes=(0, 1, 3)),
                dict(spacing=(1., 0., 1.)), dict(spacing=(1., float('nan'), 1.)), dict(spacing=(float('inf'), 1., 1.)), dict(origin=(0., float('inf'), 0.)),
                dict(level=float('nan')), dict(step=0.0), dict(step=-1.0), dict(step=100.0), dict(step=float('nan')), dict(refine=-1), dict(refine=33),
                dict(shade_mode=2), dict(ambient=1.5), dict(ambient=float('nan')), dict(background=float('inf'))):
        assert lib.eg3d_iso_render(params(**bad), None) == INVALID, bad
    assert lib.eg3d_iso_render(params(D0=2048, D1=2048, D2=512), None) == TOO_LARGE
    assert lib.eg3d_iso_render(params(res=16385), None) == UNSUPPORTED
    assert lib.eg3d_iso_render(params(F=65536), None) == UNSUPPORTED


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    with pytest.raises(Eg3dHipError):
        H.iso_bricks(torch.zeros(4, 4, 4))
    with pytest.raises(Eg3dHipError):
        H.iso_render(torch.zeros(4, 4, 4), torch.zeros(1, 25), 8, 0.0, (0, 0, 0), (1, 1, 1))
    assert H.iso_bricks_shape((2, 9, 10)) == (1, 1, 2) and H.iso_bricks_shape((512, 512, 512)) == (64, 64, 64)
    assert H.iso_bricks_shape((17, 37, 61)) == R.bricks_shape((17, 37, 61)) == (2, 5, 8)
