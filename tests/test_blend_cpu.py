"""Multi-band paste-back, host side (no GPU): the properties of the numpy restatement tests/support/blend_ref.py that the kernels of
csrc/blend.hip are held to byte for byte (tests/test_gpu_blend.py), images.paste_bands, the parameter structure against the header and the
entry's refusals before any launch.

  reach          with D and alpha supported in a rectangle, R_0 is exactly 0 further than 4 2^L - 4 pixels outside it, at every offset of the
                 rectangle against the pyramid's grid: the window's margin 2^(L + 2) truncates nothing
  zero alpha     alpha == 0 gives R == 0 exactly; so does D == 0
  unit alpha     alpha == 1 returns D in the interior (zero extension makes alpha_k < 1 near the border: not asserted there)
  seam gradient  a constant offset of 40 levels under a smoothstep ramp: the steepest step of R through the seam falls from one band to
                 two to four -- what the feature is for"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_ref as B  # noqa: E402
import paste_ref as P  # noqa: E402

F = np.float32


@pytest.mark.parametrize('L', [1, 2, 3, 4])
def test_reach_is_inside_the_margin(L):
    worst, pad = 0, 4 * 2 ** L + 8
    for off in range(0, 2 ** L + 1):
        for size in (37, 64):
            s, n = pad + off, 2 * pad + 2 ** L + size
            D, a = np.zeros((n, n), F), np.zeros((n, n), F)
            D[s:s + size, s:s + size] = 255
            a[s:s + size, s:s + size] = 1
            R = B.collapse(D, a, L)
            assert R[s + size // 2, s + size // 2] != 0
            for nz in (np.where((R != 0).any(1))[0], np.where((R != 0).any(0))[0]):
                worst = max(worst, s - nz.min(), nz.max() - (s + size - 1))
    print(f'bands {L}: R_0 is nonzero up to {worst} pixels outside the rectangle (bound {4 * 2 ** L - 4}, margin {2 ** (L + 2)})')
    assert worst <= 4 * 2 ** L - 4 < 2 ** (L + 2)


def test_zero_alpha_and_zero_difference_give_the_photo_exactly():
    rs = np.random.RandomState(3)
    D = rs.uniform(-255, 255, (3, 77, 165)).astype(F)
    a = rs.uniform(0, 1, (1, 77, 165)).astype(F)
    for L in (1, 3, 5):
        assert not B.collapse(D, np.zeros_like(a), L).any()
        assert not B.collapse(np.zeros_like(D), a, L).any()
    photo = rs.randint(0, 256, (60, 70, 3)).astype(np.uint8)
    edits = rs.randint(0, 256, (2, 32, 32, 3)).astype(np.uint8)
    matrix, region = (-4.0, 0.8, 0.1, -3.0, -0.1, 0.8), (4, 3, 50, 45)
    zero = np.zeros((32, 32), np.uint8)
    assert np.array_equal(B.blend8(photo, edits, matrix, region, 2, 3.0, zero), np.repeat(photo[None], 2, 0))
    assert (B.blend8(photo, edits, matrix, region, 2, 3.0) != photo).any()


def test_unit_alpha_returns_the_difference_in_the_interior():
    rs = np.random.RandomState(4)
    D = rs.uniform(-255, 255, (3, 150, 170)).astype(F)
    for L in (1, 2, 3):
        R = B.collapse(D, np.ones((1, 150, 170), F), L)
        m = 4 * 2 ** L
        err = np.abs(R - D)[:, m:-m, m:-m].max()
        print(f'bands {L}: |R - D| <= {err:.3g} in the interior')
        assert err <= 1e-3


def test_seam_gradient_falls_with_the_bands():
    n = 301
    D = np.zeros((n, n), F)
    D[60:241, 60:241] = 40
    yy, xx = np.mgrid[:n, :n]
    f = np.minimum(np.minimum(np.minimum(xx - 60, 240 - xx), np.minimum(yy - 60, 240 - yy)).clip(0, None) / 14.0, 1)
    a = (f * f * (3 - 2 * f)).astype(F)
    a[D == 0] = 0
    grad = {L: float(np.abs(np.diff((D * a if L == 0 else B.collapse(D, a, L))[150])).max()) for L in (0, 2, 4)}
    print('steepest step of R through the seam:', grad)
    assert grad[0] > grad[2] > grad[4] > 0


def test_restatement_is_the_paste_at_level_zero_and_keeps_shapes():
    """D and alpha ARE paste8's val - photo and a; the outputs have paste8's shapes; an empty box gives the photo."""
    rs = np.random.RandomState(5)
    photo = rs.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    edits = rs.randint(0, 256, (2, 16, 16, 3)).astype(np.uint8)
    matrix, region = (-3.0, 0.5, 0.05, -2.0, -0.05, 0.5), (8, 6, 38, 36)
    mask = rs.randint(0, 256, (2, 16, 16)).astype(np.uint8)
    win = B.window(region, 1, 40, 50)
    assert win == (0, 0, 46, 40)
    D, A = B.level0(photo, edits, matrix, win, 2.0, mask)
    _, alpha = P.paste8(photo, edits, matrix, win, 2.0, mask, return_alpha=True)
    assert D.dtype == F and A.dtype == F and np.array_equal(A[:, 0], alpha.astype(F)) and (A > 0).any()
    whole, lv = B.blend8(photo, edits, matrix, region, 3, 2.0, mask, return_levels=True)
    assert whole.shape == (2, 40, 50, 3) and [d.shape[-2:] for d in lv['D']] == [(40, 50), (20, 25), (10, 13), (5, 7)]
    box = B.blend8(photo, edits, matrix, region, 3, 2.0, mask, whole=False)
    assert box.shape == (2, 30, 30, 3) and np.array_equal(box, whole[:, 6:36, 8:38])
    assert np.array_equal(B.blend8(photo, edits[0], matrix, region, 3, 2.0, mask[0]), whole[0])
    assert np.array_equal(B.blend8(photo, edits, matrix, (8, 6, 8, 36), 3), np.repeat(photo[None], 2, 0))
    assert B.blend8(photo, edits, matrix, (8, 6, 8, 36), 3, whole=False).shape == (2, 30, 0, 3)


def test_paste_bands():
    from inv3d_amd.images import PastePlan, paste_bands
    plan = lambda scale: PastePlan((0.0,) * 6, (0, 0, 1, 1), None, scale)
    # feather S / scale photo pixels: < 8 -> 1 (the floor), [8, 16) -> 2, [16, 32) -> 3, [32, 64) -> 4, >= 64 -> 5 (the ceiling)
    for feather, S, scale, want in ((0.08, 512, 0.309, 5), (0.08, 512, 1.0, 4), (0.08, 512, 2.0, 3), (0.08, 128, 1.0, 2), (0.08, 64, 1.0, 1),
                                    (0.0, 512, 1.0, 1), (0.08, 99.9, 1.0, 1), (0.125, 64, 1.0, 2), (0.5, 512, 0.25, 5), (0.125, 128, 1.0, 3), (0.125, 127, 1.0, 2)):
        assert paste_bands(plan(scale), S, feather) == want, (feather, S, scale)


def test_cpu_tensors_raise():
    import torch
    from inv3d_amd import hipops as H, images
    from inv3d_amd._lib import Eg3dHipError
    photo = torch.zeros((100, 100, 3), dtype=torch.uint8)
    edit = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(Eg3dHipError):
        H.paste_blend(photo, edit, (0, 1, 0, 0, 0, 1), (0, 0, 10, 10), 2)
    with pytest.raises(Eg3dHipError):
        images.paste_back(photo, edit, P.EXACT_LANDMARKS[0], bands=2)
    with pytest.raises(Eg3dHipError):
        images.paste_back(photo, edit, P.EXACT_LANDMARKS[0], bands='auto')
    for bad in (-1, 7, 2.0, 'many', True, None):
        with pytest.raises(ValueError):
            images.paste_back(photo, edit, P.EXACT_LANDMARKS[0], bands=bad)
    assert images.bands_arg('auto') == 'auto' and images.bands_arg('0') == 0 and images.bands_arg('6') == 6
    for bad in ('7', '-1', 'some'):
        with pytest.raises(ValueError):
            images.bands_arg(bad)


def test_structure_matches_the_header_and_the_entry_validates_on_the_host():
    import ctypes as C
    import shutil
    import subprocess
    import tempfile
    from inv3d_amd import _lib as L
    lib = L.lib()
    a = 0x10000                                                        # non-null fake address: validation fails before any launch

    def params(**kw):
        base = dict(photo=a, edits=a, mask=None, dst=a, inv_feather=0.0, N=2, Hp=20, Wp=30, C=3, S=8, x0=4, y0=5, x1=4, y1=9, mask_frames=1,
                    whole=0, layout=L.PASTE_HWC, bands=2, workspace=None, workspace_bytes=0)
        base.update(kw)
        p = L.PasteBlend8Params(**base)
        p.m[:] = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        return p
    n = C.c_int64(-1)
    assert lib.eg3d_paste_blend8(C.byref(params()), None) == 0                           # an empty box: valid, nothing launched, no workspace
    assert lib.eg3d_paste_blend8_query_workspace(C.byref(params()), C.byref(n)) == 0 and n.value == 0
    # box 4..14 x 5..9, bands 2: margin 16, window 30 x 20 (clamped) -> levels 15 x 10 and 8 x 5; D + alpha on both, R on level 1
    box = dict(x1=14)
    assert lib.eg3d_paste_blend8_query_workspace(C.byref(params(**box)), C.byref(n)) == 0
    assert n.value == 4 * 2 * (4 * (150 + 40) + 3 * 150)
    assert lib.eg3d_paste_blend8_query_workspace(C.byref(params(C=1, **box)), C.byref(n)) == 0 and n.value == 4 * 2 * (2 * (150 + 40) + 150)
    # bands 1: margin 8, window 22 x 17 -> level 1 of 11 x 9, no R level
    assert lib.eg3d_paste_blend8_query_workspace(C.byref(params(bands=1, **box)), C.byref(n)) == 0 and n.value == 4 * 2 * 4 * 11 * 9
    need = 4 * 2 * (4 * (150 + 40) + 3 * 150)
    assert lib.eg3d_paste_blend8(None, None) == -1 and lib.eg3d_paste_blend8_query_workspace(None, C.byref(n)) == -1
    assert lib.eg3d_paste_blend8_query_workspace(C.byref(params()), None) == -1
    for bad in (dict(workspace=None, workspace_bytes=need), dict(workspace=a, workspace_bytes=need - 4), dict(workspace=a + 2, workspace_bytes=need),
                dict(workspace=a, workspace_bytes=need, bands=0), dict(workspace=a, workspace_bytes=need, bands=7),
                dict(workspace=a, workspace_bytes=need, bands=-1)):
        assert lib.eg3d_paste_blend8(C.byref(params(**dict(box, **bad))), None) == -1, bad
    for bad in (dict(photo=None), dict(edits=None), dict(dst=None), dict(C=2), dict(C=4), dict(S=0), dict(S=65536), dict(Wp=65536), dict(N=0),
                dict(x0=-1), dict(x1=31), dict(y1=21), dict(x0=5, x1=4), dict(y0=10, y1=9), dict(layout=2), dict(mask=a, mask_frames=3),
                dict(inv_feather=-1.0), dict(inv_feather=float('nan')), dict(bands=0), dict(bands=7)):
        assert lib.eg3d_paste_blend8(C.byref(params(**bad)), None) == -1, bad
        assert lib.eg3d_paste_blend8_query_workspace(C.byref(params(**bad)), C.byref(n)) == -1, bad
    assert L.PasteBlend8Params._fields_[:len(L.PasteBack8Params._fields_)] == L.PasteBack8Params._fields_
    if shutil.which('gcc') is None:
        return
    cname, cls = 'eg3d_paste_blend8_params', L.PasteBlend8Params
    src, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {'], []
    src.append(f' printf("%zu\\n", sizeof({cname}));')
    want.append(C.sizeof(cls))
    for fld in cls._fields_:
        src.append(f' printf("%zu\\n", offsetof({cname}, {fld[0]}));')
        want.append(getattr(cls, fld[0]).offset)
    for name, value in (('EG3D_BLEND_MAX_BANDS', L.BLEND_MAX_BANDS), ('EG3D_BLEND_L1_TILE_W', L.BLEND_L1_TILE[0]),
                        ('EG3D_BLEND_L1_TILE_H', L.BLEND_L1_TILE[1]), ('EG3D_BLEND_COMPOSE_TILE_W', L.BLEND_COMPOSE_TILE[0]),
                        ('EG3D_BLEND_COMPOSE_TILE_H', L.BLEND_COMPOSE_TILE[1])):
        src.append(f' printf("%d\\n", {name});')
        want.append(value)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
