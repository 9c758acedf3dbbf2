"""Target-image ingestion, host side (no GPU): the integer coefficient builder and the numpy restatements of tests/support/pil_ref.py against
Pillow itself (byte-equal), inv3d_amd.images.align_face's host geometry against the reference's align_face (tests/golden/align.npz, made by
tests/golden/make_golden_align.py), and the new structures against the header.

The pad bound (stage (c) is floating point in the reference -- float32 arrays, float64 sums inside scipy -- so byte equality is not asked):
at most 1 level anywhere, exact wherever both blend weights are exactly 0, and at most 1e-3 of the pixels different at all.  Measured here
for the restatement: no pixel differs, on the five pad shapes below and on the three golden cases that pad."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import pil_ref as R  # noqa: E402

PAD_SHARE_CAP = 1e-3

# (H, W) -> (W', H'), channels
RESIZE_CASES = [((37, 53), (16, 11), 3), ((8, 8), (19, 23), 3), ((1, 1), (4, 4), 3), ((7, 301), (5, 7), 3), ((3, 257), (2, 3), 3),
                ((64, 64), (64, 64), 3), ((40, 40), (13, 40), 3), ((29, 31), (12, 45), 1)]
QUAD_IMAGE = (41, 57)
QUAD_SIZE = (24, 20)
QUADS = dict(partly_outside=(3.7, 2.2, -4.5, 35.1, 50.3, 44.9, 60.2, -3.5), integer_axis_aligned=(2, 3, 2, 23, 26, 23, 26, 3))
# (H, W), pads (left, top, right, bottom), qsize
PAD_CASES = [((120, 100), (30, 30, 30, 30), 100), ((90, 140), (42, 42, 42, 42), 140), ((60, 50), (10, 10, 10, 10), 33),
             ((70, 64), (12, 20, 7, 31), 80),
             ((5, 6), (13, 9, 8, 14), 500)]         # pads and a tap radius (40) beyond the image: indices fold more than once; no zero-weight pixel


def noise_image(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c), dtype=np.uint8)


def smooth_image(h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.stack([128 + 80 * np.sin(xx / 17 + yy / 23), 100 + 60 * np.cos(xx / 11), 90 + yy], -1) + rs.normal(0, 12, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def pil_resize(img, size, filter):
    from PIL import Image
    f = dict(bilinear=Image.BILINEAR, lanczos=Image.LANCZOS)[filter]
    src = Image.fromarray(img if img.shape[2] == 3 else img[..., 0])
    return np.asarray(src.resize(size, f)).reshape(size[1], size[0], img.shape[2])


def pil_quad(img, size, quad):
    from PIL import Image
    return np.asarray(Image.fromarray(img).transform(size, Image.QUAD, quad, Image.BILINEAR))


def pad_bound(got, want, pads, what=''):
    """The pad bound of the module docstring on a padded image; returns the share of differing pixels."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d.max(-1) > 0).mean())
    print(f'{what}: max |d| {d.max()}, share of differing pixels {share:.3g}')
    assert d.max() <= 1, (what, int(d.max()))
    zero = (R.pad_mask(got.shape[0], got.shape[1], pads) <= -1.0 / 3.0)[..., 0]          # clip(3 mask + 1) = clip(mask) = 0
    assert zero.any() or got.shape[0] < 40, what
    assert not zero.any() or d[zero].max() == 0, what
    assert share <= PAD_SHARE_CAP, (what, share)
    return share


def align_cases():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'align.npz'), allow_pickle=False)
    names = sorted({k.split('.')[0] for k in z.files})
    return {n: dict(image=z[n + '.image'], landmarks=z[n + '.landmarks'], output_size=int(z[n + '.output_size']), aligned=z[n + '.aligned'],
                    branches=tuple(bool(b) for b in z[n + '.branches'])) for n in names}


def align_bound(got, case, what=''):
    """Byte-equal without the pad branch; with it at most 1 level (a bilinear warp of an image that is off by at most one moves by at most
    one again) and at most 1e-3 of the pixels."""
    want = case['aligned']
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d.max(-1) > 0).mean())
    print(f'{what}: pad {case["branches"][2]}, max |d| {d.max()}, share of differing pixels {share:.3g}')
    if not case['branches'][2]:
        assert d.max() == 0, what
    else:
        assert d.max() <= 1 and share <= PAD_SHARE_CAP, (what, int(d.max()), share)
    return share


@pytest.mark.parametrize('filter', ['bilinear', 'lanczos'])
@pytest.mark.parametrize('hw,size,ch', RESIZE_CASES)
def test_resize_restatement_is_byte_equal_to_pillow(hw, size, ch, filter):
    img = noise_image(hw[0], hw[1], ch, hw[0] * 1000 + hw[1])
    assert np.array_equal(R.resize8(img, size, filter), pil_resize(img, size, filter))


def test_coefficient_tables():
    from inv3d_amd.hipops import pil_resize_coeffs
    b, c = pil_resize_coeffs(8, 8, 'bilinear')                      # identity: one full-weight tap per output (and zero-weight neighbours)
    assert c.shape == (8, 3) and all(int(c[i].sum()) == 1 << 22 for i in range(8))
    b, c = pil_resize_coeffs(257, 2, 'lanczos')                     # ksize grows with the reduction: hundreds of taps
    assert c.shape[1] == 2 * int(np.ceil(3 * 257 / 2)) + 1 and c.shape[1] > 700
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 257).all() and (b[:, 1] <= c.shape[1]).all()
    assert 255 * int(np.abs(c.astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31          # the int32 accumulator cannot overflow
    with pytest.raises(ValueError):
        pil_resize_coeffs(8, 8, 'bicubic')


@pytest.mark.parametrize('name', sorted(QUADS))
def test_quad_restatement_is_byte_equal_to_pillow(name):
    img = noise_image(QUAD_IMAGE[0], QUAD_IMAGE[1], 3, 7)
    want = pil_quad(img, QUAD_SIZE, QUADS[name])
    assert np.array_equal(R.quad_warp8(img, QUAD_SIZE, QUADS[name]), want)
    if name == 'partly_outside':
        assert int((want.max(-1) == 0).sum()) == 32               # the part of the quad outside the image stays 0


@pytest.mark.parametrize('hw,pads,qsize', PAD_CASES)
def test_pad_restatement_against_the_scipy_statements(hw, pads, qsize):
    img = smooth_image(hw[0], hw[1], hw[0])
    pad_bound(R.feather_pad(img, pads, qsize), R.scipy_pad(img, pads, qsize), pads, f'restatement {hw} {pads}')


@pytest.mark.parametrize('name', sorted(align_cases()))
def test_align_geometry_through_the_restatement_reproduces_the_reference(name):
    case = align_cases()[name]
    got = R.align_face(case['image'], case['landmarks'], case['output_size'])
    align_bound(got, case, f'restatement {name}')


def test_golden_covers_every_branch_combination():
    from inv3d_amd.images import align_plan
    seen = set()
    for name, case in align_cases().items():
        plan = align_plan(case['image'].shape[0], case['image'].shape[1], case['landmarks'], case['output_size'])
        got = (plan.shrink_size is not None, plan.crop is not None, plan.pad is not None)
        assert got == case['branches'], name                         # the plan takes the branches the reference took
        seen.add(got)
    assert {(False, False, False), (False, True, False), (False, True, True), (True, True, False), (True, True, True)} <= seen


def test_cpu_tensors_raise_and_arguments_are_checked():
    import torch
    from inv3d_amd import hipops as H, images
    from inv3d_amd._lib import Eg3dHipError
    x = torch.zeros((4, 4, 3), dtype=torch.uint8)
    for call in (lambda: H.pil_resize(x, (2, 2)), lambda: H.pil_quad_warp(x, (2, 2), (0, 0, 0, 4, 4, 4, 4, 0)), lambda: H.feather_pad(x, (1, 1, 1, 1), 10),
                 lambda: H.u8_to_target(x), lambda: images.align_face(x, np.zeros((68, 2)) + np.arange(68)[:, None], 4)):
        with pytest.raises(Eg3dHipError):
            call()
    with pytest.raises(ValueError):
        images.align_plan(10, 10, np.zeros((5, 2)), 4)


def test_new_structures_match_the_header_and_entries_validate_on_the_host():
    import ctypes as C
    import shutil
    import subprocess
    import tempfile
    from inv3d_amd import _lib as L
    lib = L.lib()
    a = 0x10000                                                        # non-null fake address: validation fails before any launch
    nb = C.c_int64(-1)
    p = L.Resample8Params(src=a, dst=a, N=1, Hi=8, Wi=8, C=3, Ho=4, Wo=4, hbounds=a, hcoef=a, vbounds=a, vcoef=a, hksize=5, vksize=5, hseg=8)
    assert lib.eg3d_resample8_query_workspace(C.byref(p), C.byref(nb)) == 0 and nb.value == 8 * 4 * 3
    p.C = 2
    assert lib.eg3d_resample8_query_workspace(C.byref(p), C.byref(nb)) == -1
    p.C, p.hbounds = 3, None                                           # a pass that changes the width needs its tables
    assert lib.eg3d_resample8(C.byref(p), None) == -1
    p.hbounds, p.hseg, p.Wi = a, 40000, 50000                          # a row segment beyond the LDS budget
    assert lib.eg3d_resample8(C.byref(p), None) == -2
    f = L.FeatherPadParams(src=a, dst=a, gauss=a, N=2, H=10, W=12, C=3, left=3, top=4, right=5, bottom=6, radius=2)
    assert lib.eg3d_feather_pad_query_workspace(C.byref(f), C.byref(nb)) == 0 and nb.value >= 2 * (2 * 20 * 20 * 3 * 4)
    assert lib.eg3d_feather_pad(C.byref(f), None) == -1                # no workspace
    f.left = 0
    assert lib.eg3d_feather_pad_query_workspace(C.byref(f), C.byref(nb)) == -1
    q = L.QuadWarp8Params(src=None, dst=a, N=1, Hi=4, Wi=4, C=3, Ho=4, Wo=4)
    assert lib.eg3d_quad_warp8(C.byref(q), None) == -1
    assert lib.eg3d_u8_to_target(None, 1, 4, 4, a, None) == -1
    if shutil.which('gcc') is None:
        return
    pairs = [('eg3d_resample8_params', L.Resample8Params), ('eg3d_quad_warp8_params', L.QuadWarp8Params), ('eg3d_feather_pad_params', L.FeatherPadParams)]
    src, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {'], []
    for cname, cls in pairs:
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
