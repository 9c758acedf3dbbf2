"""The numpy restatement of the head-matte kernels (tests/support/matte_ref.py) pinned against scipy, and the host side of
images.matte_from_mask: what tests/test_gpu_matte.py then demands integer and byte equality with."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
import matte_ref as M  # noqa: E402
from scipy import ndimage as ndi  # noqa: E402


def random_mask(h, w, density, seed, n=None):
    rs = np.random.RandomState(seed)
    m = (rs.random_sample((h, w) if n is None else (n, h, w)) < density).astype(np.uint8) * 255
    return m


def blob_mask(h, w, seed, holes=6, specks=6):
    """A disc-like head with a few holes inside and a few specks outside: what open and close are for."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    m = ((yy - 0.52 * h) ** 2 / (0.36 * h) ** 2 + (xx - 0.47 * w) ** 2 / (0.30 * w) ** 2) < 1.0
    for _ in range(holes):
        y, x = int(rs.randint(h // 3, 2 * h // 3)), int(rs.randint(w // 3, 2 * w // 3))
        m[y:y + 1 + h // 64, x:x + 1 + w // 64] = False
    for _ in range(specks):
        y, x = int(rs.randint(0, h // 10 + 1)), int(rs.randint(0, w))
        m[y, x] = True
    return m.astype(np.uint8) * 255


def scipy_sq_distance(to):
    """int64 squared distance from every pixel to the nearest True of `to` (the integer offsets of scipy's feature transform)."""
    _, idx = ndi.distance_transform_edt(~to, return_indices=True)
    yy, xx = np.mgrid[:to.shape[0], :to.shape[1]]
    return (idx[0] - yy).astype(np.int64) ** 2 + (idx[1] - xx).astype(np.int64) ** 2


def disc(r):
    k = int(math.floor(r))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return (yy * yy + xx * xx) <= r * r


SHAPES = [(1, 1), (1, 7), (9, 1), (5, 5), (17, 33), (40, 23), (97, 130)]


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('density', [0.03, 0.5, 0.97])
def test_squared_distances_equal_scipy(h, w, density):
    m = random_mask(h, w, density, 7 * h + w)
    fg = m != 0
    sd2 = M.edt2(m)
    if fg.all() or not fg.any():                                        # one class only (the 1 x 1 frame always): the sentinel
        assert (sd2 == (1 << 28 if fg.all() else -(1 << 28))).all()
        return
    assert sd2.dtype == np.int32 and (sd2 != 0).all()
    assert np.array_equal(sd2 > 0, fg)
    assert np.array_equal(np.abs(sd2)[fg], scipy_sq_distance(~fg)[fg])
    assert np.array_equal(np.abs(sd2)[~fg], scipy_sq_distance(fg)[~fg])


@pytest.mark.parametrize('r', [1, 1.5, 2, 3.3])
@pytest.mark.parametrize('h,w', [(1, 9), (13, 1), (31, 37), (64, 50)])
def test_stages_equal_disc_morphology(r, h, w):
    m = random_mask(h, w, 0.8, int(10 * r) + h) if h * w > 20 else random_mask(h, w, 0.6, 3)
    fg = m != 0
    q = int(math.floor(r * r))
    eroded = ndi.binary_erosion(fg, structure=disc(r), border_value=1)
    assert np.array_equal(M.edt2(m) > q, eroded)
    sparse = random_mask(h, w, 0.05, int(10 * r) + w) != 0
    dilated = ndi.binary_dilation(sparse, structure=disc(r))
    assert np.array_equal(M.edt2(sparse.astype(np.uint8)) > -q - 1, dilated)
    # and chained: the staged transform is the transform of the morphology's result
    if eroded.any() and not eroded.all():
        assert np.array_equal(M.edt2(m, (q,)), M.edt2(eroded.astype(np.uint8)))
        opened = ndi.binary_dilation(eroded, structure=disc(r))
        assert np.array_equal(M.edt2(m, (q, -q - 1)) > 0, opened)


def test_sentinels_and_frames_do_not_leak():
    m = np.stack([np.zeros((6, 9), np.uint8), np.full((6, 9), 255, np.uint8), random_mask(6, 9, 0.4, 1)])
    sd2 = M.edt2(m)
    assert (sd2[0] == -(1 << 28)).all() and (sd2[1] == 1 << 28).all()
    assert np.array_equal(sd2[2], M.edt2(m[2])) and np.abs(sd2[2]).max() < 1 << 25
    # a stage that empties the frame: the sentinel again
    assert (M.edt2(m[2], (10 ** 6,)) == -(1 << 28)).all() and (M.edt2(m[2], (-10 ** 6,)) == 1 << 28).all()
    assert (M.matte8(sd2[:2], (12, 18), feather_px=3.0)[0] == 0).all() and (M.matte8(sd2[:2], (12, 18), feather_px=3.0)[1] == 255).all()
    assert (M.matte8(sd2[:2], (12, 18))[0] == 0).all() and (M.matte8(sd2[:2], (12, 18), shrink_px=50.0)[1] == 255).all()


def test_matte8_properties():
    m = blob_mask(32, 32, 3)
    sd2 = M.edt2(m)
    a = M.matte8(sd2, 96, feather_px=6.0)
    assert a.shape == (96, 96) and a.dtype == np.uint8
    up = np.repeat(np.repeat(sd2, 3, 0), 3, 1)
    # deep inside (the 6-pixel ramp is 2 source pixels; distances are 1-Lipschitz across the taps), outside beyond the contour's own cell
    assert (a[up >= 4 * 4 + 1] == 255).all() and (a[up <= -4] == 0).all() and 0 < ((a > 0) & (a < 255)).sum()
    # monotone in sd2: a mask that contains another gives a matte that is nowhere lower
    grown = M.edt2(m, (-5,))
    assert (grown >= sd2).all() and (M.matte8(grown, 96, feather_px=6.0) >= a).all()
    assert (M.matte8(sd2, 96, shrink_px=-2.0, feather_px=6.0) >= a).all() and (M.matte8(sd2, 96, shrink_px=2.0, feather_px=6.0) <= a).all()
    # flips commute (the taps and weights mirror exactly: u(Wo - 1 - X) = Ws - 1 - u(X) in these power-of-two ratios)
    b = M.matte8(M.edt2(m[::-1, ::-1]), 128, feather_px=5.0)
    assert np.array_equal(b[::-1, ::-1], M.matte8(sd2, 128, feather_px=5.0))
    # a hard edge is e > 0: at the source resolution the matte is the mask itself
    assert np.array_equal(M.matte8(sd2, 32), m)
    hard = M.matte8(sd2, 64, shrink_px=1.5)
    assert set(np.unique(hard)) <= {0, 255} and (hard <= M.matte8(sd2, 64)).all() and hard.sum() < M.matte8(sd2, 64).sum()
    # the edge is sub-pixel: at 4x the contour of a straight vertical edge lies on the half-way line between the two centres
    half = np.zeros((8, 8), np.uint8)
    half[:, 4:] = 255
    assert np.array_equal(M.matte8(M.edt2(half), 32)[5], np.r_[np.zeros(16, np.uint8), np.full(16, 255, np.uint8)])


def test_radius_to_threshold_conversion():
    from inv3d_amd import images
    for side in (16, 128, 512, 77):
        for op, cl in ((0.02, 0.04), (0.0, 0.04), (0.02, 0.0), (0.0, 0.0), (0.013, 0.2)):
            t = images.matte_thresholds(side, op, cl)
            assert t == M.stage_thresholds(side, op, cl)
            want = []
            if op > 0:
                q = int(math.floor((op * side) ** 2))
                want += [q, -q - 1]
            if cl > 0:
                q = int(math.floor((cl * side) ** 2))
                want += [-q - 1, q]
            assert list(t) == want
    assert images.matte_thresholds(128) == (6, -7, -27, 26)            # r = 2.56 and 5.12 pixels
    with pytest.raises(ValueError):
        images.matte_thresholds(128, open=-0.1)


def test_structures_match_the_header_and_the_entries_validate_on_the_host():
    import ctypes as C
    import shutil
    import subprocess
    import tempfile
    from inv3d_amd import _lib as L
    lib = L.lib()
    a = 0x10000                                                        # non-null fake address: validation fails before any launch

    def edt(**kw):
        base = dict(src=a, sd2=a, workspace=a, workspace_bytes=1 << 40, N=2, H=128, W=128, n_stages=2, impl=L.EDT_IMPLS['auto'])
        base.update(kw)
        return L.Edt2Params(**base)
    nbytes = C.c_int64(-1)
    assert lib.eg3d_edt2_query_workspace(C.byref(edt(impl=L.EDT_IMPLS['tiled'])), C.byref(nbytes)) == 0 and nbytes.value == 2 * 128 * 128 * 2
    assert lib.eg3d_edt2_query_workspace(C.byref(edt(impl=L.EDT_IMPLS['resident'])), C.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.eg3d_edt2_query_workspace(C.byref(edt()), None) == -1 and lib.eg3d_edt2(None, None) == -1
    for bad, status in ((dict(src=None), -1), (dict(sd2=None), -1), (dict(N=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(n_stages=5), -1),
                        (dict(n_stages=-1), -1), (dict(impl=3), -1), (dict(impl=L.EDT_IMPLS['tiled'], workspace=None), -1),
                        (dict(impl=L.EDT_IMPLS['tiled'], workspace_bytes=2 * 128 * 128 * 2 - 1), -1), (dict(H=4097), -2), (dict(W=4097), -2),
                        (dict(N=32768, H=256, W=256), -2), (dict(impl=L.EDT_IMPLS['resident'], W=129), -2)):
        assert lib.eg3d_edt2(C.byref(edt(**bad)), None) == status, bad

    def matte(**kw):
        base = dict(sd2=a, dst=a, step=0.25, inv_step=4.0, shrink_px=0.0, inv_feather=0.0, N=1, Hs=16, Ws=16, Ho=64, Wo=64)
        base.update(kw)
        return L.Matte8Params(**base)
    assert lib.eg3d_matte8(None, None) == -1
    for bad, status in ((dict(sd2=None), -1), (dict(dst=None), -1), (dict(N=0), -1), (dict(Hs=0), -1), (dict(Wo=0), -1), (dict(Ho=65), -1),
                        (dict(Ws=15), -1), (dict(step=0.0), -1), (dict(inv_step=-4.0), -1), (dict(inv_feather=-1.0), -1),
                        (dict(inv_feather=float('nan')), -1), (dict(shrink_px=float('nan')), -1), (dict(Hs=4097, Ws=4097, Ho=4097, Wo=4097), -2),
                        (dict(Ho=16385, Wo=16385), -2), (dict(N=1 << 20, Ho=64, Wo=64), -2)):
        assert lib.eg3d_matte8(C.byref(matte(**bad)), None) == status, bad
    if shutil.which('gcc') is None:
        return
    src, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {'], []
    for cname, cls in (('eg3d_edt2_params', L.Edt2Params), ('eg3d_matte8_params', L.Matte8Params)):
        src.append(f' printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for fld in cls._fields_:
            src.append(f' printf("%zu\\n", offsetof({cname}, {fld[0]}));')
            want.append(getattr(cls, fld[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert L.EDT_MAX_STAGES == 4 and L.EDT_IMPLS == dict(auto=0, resident=1, tiled=2)


def test_chain_cleans_a_ragged_mask():
    m = blob_mask(128, 128, 5)
    fg = m != 0
    sd2 = M.edt2(m, M.stage_thresholds(128))
    clean = sd2 > 0
    assert not clean[:14].any() and fg[:14].any()                       # the specks are gone
    assert ndi.label(clean)[1] == 1 and ndi.label(~clean)[1] == 1 and ndi.label(~fg)[1] > 1     # one head, no holes
    assert abs(int(clean.sum()) - int(fg.sum())) < 0.02 * fg.sum()
    a = M.matte_from_mask(m, 512)
    assert a.shape == (512, 512) and a[256, 240] == 255 and a[5, 5] == 0
