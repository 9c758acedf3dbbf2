"""CPU tests of the grid components: the numpy restatement (tests/support/cc_ref.py) against scipy.ndimage.label, select_components, the
parameter structure against the header, the entries' argument errors (answered before any launch) and clean_grid's argument errors, and the
subset property of a cleaned grid on the restatement alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import cc_cases as CS  # noqa: E402
import cc_ref as CR  # noqa: E402
import mc_ref as MC  # noqa: E402
from inv3d_amd import inference as I  # noqa: E402


@pytest.mark.parametrize('conn', [6, 26])
@pytest.mark.parametrize('p', [0.2, 0.3, 0.5])
@pytest.mark.parametrize('shape', [(33, 17, 9), (40, 40, 40)])
def test_restatement_equals_scipy(shape, p, conn):
    """scipy numbers components in raster order of first appearance too: the labels are equal one for one."""
    ndi = pytest.importorskip('scipy.ndimage')
    vol, level = CS.make(f'random_{p}', shape, seed=int(p * 10))
    got = CR.label(vol, level, conn)
    structure = ndi.generate_binary_structure(3, 1 if conn == 6 else 3)
    want, k = ndi.label(vol > level, structure=structure)
    assert got['count'] == k and np.array_equal(got['labels'], want.astype(np.int32))
    assert np.array_equal(got['sizes'], np.bincount(want.reshape(-1), minlength=k + 1)[1:])
    first = np.full(k, vol.size, np.int64)
    np.minimum.at(first, want.reshape(-1)[want.reshape(-1) > 0] - 1, np.flatnonzero(want.reshape(-1) > 0))
    assert np.array_equal(got['roots'], first) and got['inside'] == int((vol > level).sum())


def test_restatement_on_special_values_and_constructions():
    v = np.array([[[0.5, np.nan, np.inf, -np.inf, 0.50000006, 1.0]]], np.float32)
    r = CR.label(v, 0.5, 6)
    assert r['labels'].tolist() == [[[0, 0, 1, 0, 2, 2]]] and r['sizes'].tolist() == [1, 2] and r['roots'].tolist() == [2, 4]
    g = CS.serpentines((40, 40, 40))
    vol = np.where(g, np.float32(1), np.float32(0))
    assert CR.label(vol, 0.5, 6)['count'] == 2 and CR.label(vol, 0.5, 26)['count'] == 1
    from inv3d_amd import _lib as L
    g, pairs = CS.planted_pairs(L.CC_TILE)
    vol = np.where(g, np.float32(1), np.float32(0))
    assert g.sum() == 2 * len(pairs) and g.shape == tuple(2 * e + 1 for e in L.CC_TILE)
    assert CR.label(vol, 0.5, 6)['count'] == 2 * len(pairs) - 3 and CR.label(vol, 0.5, 26)['count'] == len(pairs)
    n = 5 * 4 * 3
    assert CR.label(CS.make('checkerboard', (5, 4, 3))[0], 0.5, 6)['count'] == n // 2 and CR.label(CS.make('checkerboard', (5, 4, 3))[0], 0.5, 26)['count'] == 1


def test_select_components():
    sel = lambda s, **kw: I.select_components(torch.tensor(s, dtype=torch.int32), **kw).tolist()      # noqa: E731
    s = [5, 9, 9, 1, 7, 9]
    assert sel(s) == [False, True, False, False, False, False]                  # ties go to the smaller label
    assert sel(s, keep=2) == [False, True, True, False, False, False]
    assert sel(s, keep=4) == [False, True, True, False, True, True]
    assert sel(s, keep=0) == [False] * 6 and sel(s, keep=100) == [True] * 6
    assert sel(s, keep=None) == [True] * 6 and sel(s, keep=None, min_voxels=6) == [False, True, True, False, True, True]
    assert sel(s, keep=3, min_voxels=9) == [False, True, True, False, False, True] and sel(s, keep=2, min_voxels=10) == [False] * 6
    assert sel([], keep=1) == [] and I.select_components(torch.zeros(0, dtype=torch.int32)).dtype == torch.bool
    big = [2 ** 31 - 1, 1, 2 ** 31 - 1]
    assert sel(big, keep=1) == [True, False, False]
    rng = np.random.RandomState(0)
    for _ in range(20):
        s = rng.randint(1, 6, size=rng.randint(1, 40))
        for keep, mv in ((1, 0), (3, 2), (None, 3), (5, 0)):
            assert sel(s.tolist(), keep=keep, min_voxels=mv) == CR.select(s, keep, mv).tolist()
    with pytest.raises(ValueError):
        I.select_components(torch.zeros(2, 2))
    with pytest.raises(ValueError):
        I.select_components(torch.zeros(2), keep=-1)


def test_structure_matches_the_header():
    """eg3d_cc_params of inv3d_amd/_lib.py against its C definition (gcc), and the exported tile extents against the header's."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {',
           ' printf("%d %d %d\\n", EG3D_CC_TILE0, EG3D_CC_TILE1, EG3D_CC_TILE2);', ' printf("%zu\\n", sizeof(eg3d_cc_params));']
    want = [*L.CC_TILE, C.sizeof(L.CcParams)]
    for f in L.CcParams._fields_:
        src.append(f' printf("%zu\\n", offsetof(eg3d_cc_params, {f[0]}));')
        want.append(getattr(L.CcParams, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_entries_reject_bad_arguments_before_any_launch():
    """Every error code of the four entries, answered from the arguments alone (no GPU here: a launch would be an error of its own)."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    OK, INVALID, TOO_LARGE = 0, -1, -3
    a = 0x1000                                                                  # a non-null pointer that is never dereferenced
    nbytes = C.c_int64(0)

    def params(**kw):
        return L.CcParams(**dict(dict(vol=a, labels=a, D0=16, D1=16, D2=16, level=0.5, connectivity=6, count=3, workspace=a, workspace_bytes=1 << 30, totals=a,
                                      sizes=a, roots=a, keep=a, out=a, fill=-1000.0), **kw))
    query = lambda **kw: lib.eg3d_cc_query_workspace(C.byref(params(**kw)), C.byref(nbytes))      # noqa: E731
    label = lambda **kw: lib.eg3d_cc_label(C.byref(params(**kw)), None)      # noqa: E731
    finish = lambda **kw: lib.eg3d_cc_finish(C.byref(params(**kw)), None)      # noqa: E731
    keep = lambda **kw: lib.eg3d_cc_keep(C.byref(params(**kw)), None)      # noqa: E731
    assert query() == OK and nbytes.value >= 16 ** 3 * 4
    need = nbytes.value
    assert query(D0=1, D1=1, D2=1) == OK and 0 < nbytes.value < need
    assert query(D0=1290, D1=1290, D2=1290) == OK and nbytes.value >= 4 * 1290 ** 3      # just below 2^31 voxels
    assert lib.eg3d_cc_query_workspace(None, C.byref(nbytes)) == INVALID and lib.eg3d_cc_query_workspace(C.byref(params()), None) == INVALID
    for fn in (lib.eg3d_cc_label, lib.eg3d_cc_finish, lib.eg3d_cc_keep):
        assert fn(None, None) == INVALID
    for fn in (query, label, finish, keep):
        for bad in (dict(D0=0), dict(D1=-1), dict(D2=0)):
            assert fn(**bad) == INVALID, bad
        for bad in (dict(D0=2048, D1=2048, D2=512), dict(D0=1 << 30, D1=1 << 30, D2=1 << 30), dict(D0=65536, D1=65536, D2=1)):
            assert fn(**bad) == TOO_LARGE, bad
    for bad in (dict(vol=None), dict(workspace=None), dict(totals=None), dict(connectivity=0), dict(connectivity=18), dict(connectivity=8),
                dict(workspace_bytes=need - 1), dict(workspace_bytes=0)):
        assert label(**bad) == INVALID, bad
    for bad in (dict(labels=None), dict(workspace=None), dict(count=-1), dict(sizes=None), dict(roots=None), dict(workspace_bytes=need - 1)):
        assert finish(**bad) == INVALID, bad
    for bad in (dict(vol=None), dict(labels=None), dict(out=None), dict(count=-1), dict(keep=None)):
        assert keep(**bad) == INVALID, bad


def test_wrappers_and_options_refuse_bad_arguments():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.coach import InversionCoach
    z = torch.zeros
    with pytest.raises(Eg3dHipError):
        H.grid_components(z(4, 4, 4), 0.0)                                      # a CPU tensor: there is no fallback
    with pytest.raises(Eg3dHipError):
        H.grid_keep(z(4, 4, 4), z(4, 4, 4, dtype=torch.int32), z(1, dtype=torch.bool))
    for bad in (dict(fill=float('nan')), dict(fill=float('inf')), dict(fill=-float('inf')), dict(fill=0.75), dict(connectivity=18)):
        with pytest.raises(ValueError):
            I.clean_grid(z(4, 4, 4), 0.5, **bad)
    with pytest.raises(ValueError):
        InversionCoach(None, gen_mesh=True, mesh_dir='m', mesh_keep=-1, w_avg_samples=0)


def test_cleaned_grid_keeps_the_kept_surface():
    """The subset property on the restatement alone: the removed components are separated from the kept one by voxels at or below the level,
    so every edge crossing of the cleaned grid is an edge crossing of the raw grid with the same two values -- the marching-cubes vertices of
    the cleaned grid (tests/support/mc_ref.py) occur bit for bit among the raw grid's."""
    vol, level = CS.make('random_0.3', (12, 11, 10), seed=4)
    for conn in (6, 26):
        r = CR.label(vol, level, conn)
        mask = CR.select(r['sizes'], 1)
        clean = CR.keep_grid(vol, r['labels'], mask)
        assert r['count'] > 2 and (clean != vol).sum() == r['sizes'][~mask].sum()
        again = CR.label(clean, level, conn)
        assert again['count'] == 1 and np.array_equal(again['labels'] > 0, r['labels'] == int(np.argmax(r['sizes'])) + 1)
        inside = clean > level
        for ax in range(3):                                                     # every crossing edge of the cleaned grid is unchanged
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[ax], b[ax] = slice(0, -1), slice(1, None)
            cross = inside[tuple(a)] != inside[tuple(b)]
            assert np.array_equal(clean[tuple(a)][cross], vol[tuple(a)][cross]) and np.array_equal(clean[tuple(b)][cross], vol[tuple(b)][cross])
        rows = lambda v: {x.tobytes() for x in np.ascontiguousarray(v)}      # noqa: E731
        raw_v, clean_v = MC.marching_cubes(vol, level)[0], MC.marching_cubes(clean, level)[0]
        assert rows(clean_v) < rows(raw_v)
