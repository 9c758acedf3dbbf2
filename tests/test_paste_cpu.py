"""Paste-back, host side (no GPU): images.paste_plan's geometry and the numpy restatement tests/support/paste_ref.py that the GPU kernel is
held to byte for byte (tests/test_gpu_paste.py).

  corner mapping    on the golden cases without a shrink the matrix maps the reference's quad onto the corners of [0, S]^2: float64 round-off
  exact round trips three landmark sets where align and paste are integer isometries: paste(align(photo)) IS the photo
  ramp round trip   every golden case, a linear-ramp photo: the LANCZOS shrink, the bilinear warp and the bilinear paste all reproduce a linear
                    function exactly, which leaves the three uint8 stages -- rint (the ramp), truncation (the warp), rint (the paste): the
                    difference lies in [-2, 1] on the interior.  Derived, not measured; a half-aligned-pixel error of the geometry reads 5 or 6
                    on the shrink cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paste_ref as P  # noqa: E402
import pil_ref as R  # noqa: E402
import test_align_cpu as TC  # noqa: E402

CASES = TC.align_cases()
NO_SHRINK = [n for n in sorted(CASES) if not CASES[n]['branches'][0]]
EXACT_PHOTO = TC.noise_image(100, 100, 3, 21)
EXACT_S = 64


def paste_full_ref(photo, edit, landmarks, feather=0.08, mask=None, region='photo'):
    """images.paste_back's steps on the restatements: paste_plan, Pillow-LANCZOS presize where scale > 1, paste8."""
    from inv3d_amd.images import paste_plan
    S = edit.shape[-2]
    plan = paste_plan(photo.shape[0], photo.shape[1], landmarks, S)
    matrix, fpx = np.asarray(plan.matrix), feather * S
    if plan.presize is not None and plan.presize != S:
        ps = plan.presize
        edit = R.resize8(edit, (ps, ps), 'lanczos') if edit.ndim == 3 else np.stack([R.resize8(e, (ps, ps), 'lanczos') for e in edit])
        if mask is not None:
            mask = R.resize8(mask[..., None], (ps, ps), 'lanczos')[..., 0] if mask.ndim == 2 else \
                np.stack([R.resize8(k[..., None], (ps, ps), 'lanczos')[..., 0] for k in mask])
        matrix, fpx = matrix * (ps / S), fpx * (ps / S)
    return P.paste8(photo, edit, matrix, plan.region, fpx, mask, whole=region == 'photo')


def reference_quad(landmarks):
    """The oriented square of the reference's align_face in photo pixels, before any shrink (alignment.py:49-56), + 0.5."""
    lm = np.asarray(landmarks, dtype=np.float64)
    eye_left, eye_right = lm[36:42].mean(0), lm[42:48].mean(0)
    eye_avg, eye_to_eye = (eye_left + eye_right) * 0.5, eye_right - eye_left
    eye_to_mouth = (lm[48] + lm[54]) * 0.5 - eye_avg
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y]) + 0.5


def _apply(matrix, pts):
    m = np.asarray(matrix)
    return np.stack([m[0] + m[1] * pts[:, 0] + m[2] * pts[:, 1], m[3] + m[4] * pts[:, 0] + m[5] * pts[:, 1]], 1)


@pytest.mark.parametrize('name', NO_SHRINK)
def test_matrix_maps_the_reference_quad_onto_the_square(name):
    from inv3d_amd.images import paste_plan
    case = CASES[name]
    S = case['output_size']
    plan = paste_plan(case['image'].shape[0], case['image'].shape[1], case['landmarks'], S)
    got = _apply(plan.matrix, reference_quad(case['landmarks']))
    err = np.abs(got - np.array([[0, 0], [0, S], [S, S], [S, 0]], np.float64)).max()
    print(f'{name}: corner error {err:.3g}')
    assert err <= 1e-9


def test_there_are_four_cases_without_a_shrink_and_two_with():
    assert len(NO_SHRINK) == 4 and len(CASES) == 6


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_matrix_agrees_with_paste_plan(name):
    """Two derivations of the same map (closed-form 2 x 2 inverse; homogeneous matrices and a linear solve)."""
    from inv3d_amd.images import paste_plan
    case = CASES[name]
    h, w = case['image'].shape[:2]
    plan = paste_plan(h, w, case['landmarks'], case['output_size'])
    m, region = P.paste_matrix(h, w, case['landmarks'], case['output_size'])
    corners = np.array([[0.0, 0.0], [0.0, h], [w, h], [w, 0.0]])
    assert np.abs(_apply(plan.matrix, corners) - _apply(m, corners)).max() <= 1e-9 * case['output_size']
    assert region == plan.region
    assert plan.scale == pytest.approx(np.sqrt(abs(m[1] * m[5] - m[2] * m[4])), rel=1e-12)


@pytest.mark.parametrize('k', range(3))
def test_exact_round_trips(k):
    from inv3d_amd.images import paste_plan
    lm, S, photo = P.EXACT_LANDMARKS[k], EXACT_S, EXACT_PHOTO
    plan = paste_plan(100, 100, lm, S)
    m = np.asarray(plan.matrix)
    assert np.array_equal(m, np.rint(m)) and abs(m[1] * m[5] - m[2] * m[4]) == 1.0 and plan.scale == 1.0 and plan.presize is None
    assert np.array_equal(np.abs(m[[1, 2, 4, 5]]), [[1, 0, 0, 1], [0, 1, 1, 0], [1, 0, 0, 1]][k])
    aligned = R.align_face(photo, lm, S)
    assert np.array_equal(P.paste8(photo, aligned, m, plan.region, 0.0), photo)
    black, alpha = P.paste8(photo, np.zeros_like(aligned), m, plan.region, 0.0, return_alpha=True)
    assert photo.any(-1).all()                                                          # no black pixel in the photo: every pasted one changes
    assert int((black != photo).any(-1).sum()) == 4096 and int((alpha == 1.0).sum()) == 4096
    _, alpha = P.paste8(photo, aligned, m, plan.region, 8.0, return_alpha=True)
    assert int((alpha == 1.0).sum()) == 2304 and int(((alpha > 0.0) & (alpha < 1.0)).sum()) == 1792
    assert np.array_equal(P.paste8(photo, aligned, m, plan.region, 8.0), photo)        # blending a pixel with itself, whatever the weight


@pytest.mark.parametrize('name', sorted(CASES))
def test_ramp_round_trip(name):
    from inv3d_amd.images import paste_plan
    case = CASES[name]
    h, w = case['image'].shape[:2]
    S, lm = case['output_size'], case['landmarks']
    photo = P.ramp_photo(h, w)
    got = paste_full_ref(photo, R.align_face(photo, lm, S), lm, feather=0.0)
    plan = paste_plan(h, w, lm, S)
    yy, xx = np.mgrid[:h, :w]
    uv = _apply(plan.matrix, np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], 1)).reshape(h, w, 2)
    margin = 4 * max(1, int(round(1.0 / plan.scale)))
    interior = ((uv >= 1.0) & (uv <= S - 1.0)).all(-1) & (xx >= margin) & (xx < w - margin) & (yy >= margin) & (yy < h - margin)
    d = got.astype(np.int32) - photo.astype(np.int32)
    print(f'{name}: scale {plan.scale:.4f}, interior {int(interior.sum())} pixels, difference in [{d[interior].min()}, {d[interior].max()}]')
    assert interior.sum() > 0
    assert d[interior].min() >= -2 and d[interior].max() <= 1


def test_presize_at_scale_two():
    from inv3d_amd.images import paste_plan
    plan = paste_plan(100, 100, P.EXACT_LANDMARKS[0], 128)
    assert plan.scale == 2.0 and plan.presize == 64
    assert paste_plan(100, 100, P.EXACT_LANDMARKS[0], 64).presize is None


@pytest.mark.parametrize('name', ['pad_edge', 'pad_corner_rotated'])
def test_region_is_clamped_by_the_photo_border(name):
    from inv3d_amd.images import paste_plan
    case = CASES[name]
    h, w = case['image'].shape[:2]
    plan = paste_plan(h, w, case['landmarks'], case['output_size'])
    x0, y0, x1, y1 = plan.region
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
    assert x0 == 0 or y0 == 0 or x1 == w or y1 == h                                     # the square leaves the photo: that is why the case pads
    quad = reference_quad(case['landmarks'])
    assert quad[:, 0].min() < 0 or quad[:, 1].min() < 0 or quad[:, 0].max() > w or quad[:, 1].max() > h
    far = P.upright_landmarks((-500.5, 40.5), (16, 0), (0, 10))                         # a face wholly outside: an empty region
    r = paste_plan(100, 100, far, 64).region
    assert r[2] - r[0] == 0


def test_bad_quads_and_landmarks_raise(monkeypatch):
    from inv3d_amd import images
    with pytest.raises(ValueError):
        images.paste_plan(100, 100, np.zeros((5, 2)), 64)
    with pytest.raises(ValueError):
        images.paste_plan(100, 100, np.zeros((68, 3)), 64)
    good = images.align_plan(100, 100, P.EXACT_LANDMARKS[0], 64)
    trapezoid = list(good.quad)
    trapezoid[4] += 9.0                                                                 # the SE corner alone: no parallelogram
    monkeypatch.setattr(images, 'align_plan', lambda *a: good._replace(quad=tuple(trapezoid)))
    with pytest.raises(ValueError):
        images.paste_plan(100, 100, P.EXACT_LANDMARKS[0], 64)


def test_cpu_tensors_raise():
    import torch
    from inv3d_amd import hipops as H, images
    from inv3d_amd._lib import Eg3dHipError
    photo = torch.zeros((100, 100, 3), dtype=torch.uint8)
    edit = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(Eg3dHipError):
        H.paste_back(photo, edit, (0, 1, 0, 0, 0, 1), (0, 0, 10, 10))
    with pytest.raises(Eg3dHipError):
        images.paste_back(photo, edit, P.EXACT_LANDMARKS[0])
    with pytest.raises(ValueError):
        images.paste_back(photo, edit, P.EXACT_LANDMARKS[0], region='face')
    with pytest.raises(ValueError):
        images.paste_back(photo, edit.float(), P.EXACT_LANDMARKS[0])


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
                    whole=0, layout=L.PASTE_HWC)
        base.update(kw)
        p = L.PasteBack8Params(**base)
        p.m[:] = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        return p
    assert lib.eg3d_paste_back8(C.byref(params()), None) == 0                            # an empty region: valid, nothing launched
    assert lib.eg3d_paste_back8(None, None) == -1
    for bad in (dict(photo=None), dict(edits=None), dict(dst=None), dict(C=2), dict(C=4), dict(S=0), dict(S=65536), dict(Wp=65536), dict(N=0),
                dict(x0=-1), dict(x1=31), dict(y1=21), dict(x0=5, x1=4), dict(y0=10, y1=9), dict(layout=2), dict(mask=a, mask_frames=3),
                dict(inv_feather=-1.0), dict(inv_feather=float('nan'))):
        assert lib.eg3d_paste_back8(C.byref(params(**bad)), None) == -1, bad
    if shutil.which('gcc') is None:
        return
    cname, cls = 'eg3d_paste_back8_params', L.PasteBack8Params
    src, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {'], []
    src.append(f' printf("%zu\\n", sizeof({cname}));')
    want.append(C.sizeof(cls))
    for fld in cls._fields_:
        src.append(f' printf("%zu\\n", offsetof({cname}, {fld[0]}));')
        want.append(getattr(cls, fld[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
