"""CPU tests of the mesh simplification and smoothing: the numpy restatement (tests/support/simplify_ref.py) on its own -- the invariants of a
simplified sphere, the identity cases, the exact smoothing cases, one comparison with a float64 operator under a bound computed from the
test's own quantities -- and the host side: the parameter structures against the header, every error code of every entry (answered before any
launch), and the argument errors of the wrappers and the coach."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import simplify_ref as SR  # noqa: E402

sphere = SR.ball                                          # mc_ref.marching_cubes of a ball on a 20^3 grid (16^3 for the dense operator)


def _rotated(f):
    s = np.argmin(f, axis=1)
    return np.take_along_axis(f, (s[:, None] + np.arange(3)[None, :]) % 3, axis=1)


@pytest.mark.parametrize('cell', [2.0, 8.0])
def test_simplified_sphere_invariants(cell):
    v, f = sphere()
    r = SR.simplify(v, f, cell)
    sv, sf, vmap = r['verts'], r['faces'], r['vertex_map']
    assert sv.dtype == np.float32 and sf.dtype == np.int32 and vmap.dtype == np.int32 and vmap.shape == (len(v),)
    assert 0 < len(sv) < len(v) and 0 < len(sf) < len(f) and len(sv) <= r['clusters']
    assert np.all(sf[:, 0] != sf[:, 1]) and np.all(sf[:, 1] != sf[:, 2]) and np.all(sf[:, 0] != sf[:, 2])
    assert np.all(sf[:, 0] < sf[:, 1]) and np.all(sf[:, 0] < sf[:, 2])            # the smallest index first
    assert len({tuple(t) for t in sf.tolist()}) == len(sf)                       # no rotated triple repeats
    assert np.array_equal(np.unique(sf), np.arange(len(sv)))                     # every vertex is referenced
    c, ok = SR.cells(v, cell)
    assert ok.all()
    for k in range(len(sv)):
        members = np.flatnonzero(vmap == k)
        assert len(members) > 0
        m = v[members]
        assert np.all(sv[k] >= m.min(0)) and np.all(sv[k] <= m.max(0))           # in the bounding box of its members
        assert np.all(SR.cells(sv[k:k + 1], cell)[0][0] == c[members[0]]) and np.all(c[members] == c[members[0]])      # ... and in their cell
    # vertex_map is consistent with the faces: a face whose three vertices map to distinct outputs survives as that triple
    g = vmap[f]
    live = (g.min(1) >= 0) & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    first = {}
    for t in _rotated(g[live]).tolist():
        first.setdefault(tuple(t), len(first))
    assert [tuple(t) for t in sf.tolist()] == list(first)                        # the survivors, in their original order
    keys = (SR.cells(sv, cell)[0] * np.array([1, 2 ** 21, 2 ** 42])).sum(1)
    assert np.all(np.diff(keys) > 0)                                             # ascending key order


def test_tiny_cell_changes_nothing_but_the_order():
    """cell 2^-10: every vertex has a cell of its own (marching-cubes vertices sit on grid edges: two integer coordinates, distinct points)."""
    v, f = sphere()
    r = SR.simplify(v, f, 2.0 ** -10)
    c, _ = SR.cells(v, 2.0 ** -10)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    assert r['clusters'] == len(v) and len(r['verts']) == len(v) and len(r['faces']) == len(f)
    assert np.array_equal(r['verts'].view(np.int32), v[order].view(np.int32))    # bit for bit, in key order
    assert np.array_equal(r['vertex_map'][order], np.arange(len(v)))
    assert np.array_equal(r['faces'], _rotated(r['vertex_map'][f]))


def test_planted_simplify_cases():
    v = np.array([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [2.5, 2.5, 0.5], [9.5, 9.5, 9.5]], np.float32)
    f = np.array([[0, 2, 3], [1, 3, 2], [3, 0, 2], [0, 1, 2], [0, 1, 1], [2, 4, 3]], np.int32)
    r = SR.simplify(v, f, 1.0)
    # clusters in key order: {0,1}, {2}, {3}, {4}, {5}; face 1 is the opposite winding of face 0 and stays, face 2 repeats face 0, face 3
    # collapses to an edge, face 4 to a point; cluster {5} is unreferenced
    assert r['clusters'] == 5 and r['faces'].tolist() == [[0, 1, 2], [0, 2, 1], [1, 3, 2]] and r['vertex_map'].tolist() == [0, 0, 1, 2, 3, -1]
    assert np.array_equal(r['verts'][0], ((v[0].astype(np.float64) + v[1].astype(np.float64)) / 2).astype(np.float32))
    pv, pf, want_faces, want_map, clusters = SR.planted()
    r = SR.simplify(pv, pf, 2.0, origin=(-3.0, 0.5, 2.0))
    assert r['clusters'] == clusters and np.array_equal(r['faces'], want_faces) and np.array_equal(r['vertex_map'], want_map)
    for bad in ([np.nan, 0, 0], [-0.5, 0, 0], [0, float(2 ** 21), 0], [np.inf, 0, 0]):
        with pytest.raises(SR.InvalidMesh):
            SR.simplify(np.array([bad], np.float32), np.zeros((0, 3), np.int32), 1.0)
    with pytest.raises(SR.InvalidMesh):
        SR.simplify(v, np.array([[0, 1, 6]], np.int32), 1.0)
    e = SR.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert e['verts'].shape == (0, 3) and e['faces'].shape == (0, 3) and e['vertex_map'].shape == (0,) and e['clusters'] == 0
    e = SR.simplify(v, np.zeros((0, 3), np.int32), 1.0)
    assert e['verts'].shape == (0, 3) and e['clusters'] == 5 and e['vertex_map'].tolist() == [-1] * 6


def test_smoothing_exact_cases():
    v, f = SR.lattice(7, 6)
    assert np.array_equal(SR.smooth(v, f, iterations=0), v)
    rows, cols, boundary = SR.adjacency(f, len(v))
    interior = ~boundary
    assert interior.sum() == 5 * 4 and np.all(np.bincount(rows, minlength=len(v))[interior] == 6)
    assert np.all(np.diff(rows * len(v) + cols) > 0)                             # neighbours distinct, ascending
    pinned = SR.smooth(v, f, iterations=4, pin_boundary=True)
    assert np.array_equal(pinned.view(np.int32), v.view(np.int32))               # all sums exact: the whole mesh is unchanged
    one = SR.smooth_pass(v, rows, cols, np.zeros(len(v), bool), 0.5)
    assert np.array_equal(one[interior].view(np.int32), v[interior].view(np.int32))
    centre = v.mean(0)
    moved = boundary & np.any(one != v, axis=1)
    assert moved.sum() == boundary.sum()                                         # without pinning the boundary moves, and moves inward
    assert np.all(np.linalg.norm(one[moved, :2] - centre[:2], axis=1) < np.linalg.norm(v[moved, :2] - centre[:2], axis=1))
    # a face with a repeated index adds no self-edge; a vertex without faces stays
    fv, ff = SR.fan(70)
    r2, c2, _ = SR.adjacency(np.concatenate([ff, [[0, 0, 1]]]), len(fv))
    assert np.all(r2 != c2) and np.bincount(r2, minlength=len(fv))[0] == 70 and np.bincount(r2, minlength=len(fv))[-1] == 0
    assert np.array_equal(SR.smooth(fv, ff, iterations=2, pin_boundary=False)[-1], fv[-1])


def test_smoothing_against_a_float64_operator():
    """The fp32 restatement against the same iteration as a dense float64 operator, 5 iterations on a sphere.  Bound, per pass: the neighbour
    sum of n <= d_max terms carries at most (n - 1) roundings, the division, the subtraction, the product and the final sum one each, and the
    float64 run starts from the same fp32 input: (d_max + 4) roundings of relative size 2^-24 on quantities of magnitude at most 2 P (a
    difference of two coordinates).  An error made in one pass is carried through every later pass, whose operator I + f (D^-1 A - I) has
    infinity norm at most |1 - f| + |f|: 1 for a lam pass (0 < lam <= 1), 1 + 2 |mu| for a mu pass (mu < 0)."""
    v, f = sphere(16, 5.2, (7.4, 7.9, 7.6))
    iters, lam, mu = 5, 0.5, -0.53
    got = SR.smooth(v, f, iterations=iters, lam=lam, mu=mu, pin_boundary=True)
    want, d_max, P = SR.smooth_f64(v, f, iters, lam, mu, pin_boundary=True)
    norms = [1.0, 1.0 + 2.0 * abs(mu)] * iters
    bound = sum((d_max + 4) * 2.0 ** -24 * 2.0 * P * float(np.prod(norms[k + 1:])) for k in range(2 * iters))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f'V {len(v)} d_max {d_max} P {P:.3f} err {err:.3e} bound {bound:.3e}')
    assert d_max >= 6 and np.abs(want - v).max() > 1e-3                          # the smoothing did move the staircase
    assert err <= bound


def _against_header(struct, cname):
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', f' printf("%zu\\n", sizeof({cname}));']
    want = [C.sizeof(struct)]
    for f in struct._fields_:
        src.append(f' printf("%zu\\n", offsetof({cname}, {f[0]}));')
        want.append(getattr(struct, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(x) for x in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_structures_match_the_header():
    from inv3d_amd import _lib as L
    _against_header(L.SimplifyParams, 'eg3d_simplify_params')
    _against_header(L.SmoothParams, 'eg3d_smooth_params')


def test_entries_reject_bad_arguments_before_any_launch():
    """Every error code of every entry, answered from the arguments alone (no GPU here: a launch would be an error of its own)."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    OK, INVALID, TOO_LARGE = 0, -1, -3
    a, b = 0x1000, 0x2000                                                        # non-null pointers that are never dereferenced
    nbytes = C.c_int64(0)
    BIG = 2 ** 31

    def sp(**kw):
        d = dict(verts=a, faces=a, V=100, F=200, cell=2.0, flags=a, keys=a, sorted_keys=a, order=a, heads=a, head_scan=a, tri=a, alive=a, face_order=a,
                 used=a, alive_scan=a, used_scan=a, workspace=a, workspace_bytes=1 << 30, out_verts=a, out_vert_capacity=10, out_faces=a,
                 out_face_capacity=10, vertex_map=a)
        origin = kw.pop('origin', (0.0, 0.0, 0.0))
        d.update(kw)
        p = L.SimplifyParams(**d)
        p.origin[:] = origin
        return p
    squery = lambda **kw: lib.eg3d_simplify_query_workspace(C.byref(sp(**kw)), C.byref(nbytes))      # noqa: E731
    entries = {n: (lambda fn: lambda **kw: fn(C.byref(sp(**kw)), None))(getattr(lib, 'eg3d_simplify_' + n)) for n in ('keys', 'heads', 'clusters', 'mark', 'emit')}
    assert squery() == OK and nbytes.value >= 100 * 4 + 101 * 4 + 100 * 12
    need = nbytes.value
    assert squery(V=0, F=0) == OK and 0 <= nbytes.value < need
    assert squery(V=BIG - 1, F=BIG - 1) == OK and nbytes.value >= 20 * (BIG - 1)
    assert lib.eg3d_simplify_query_workspace(None, C.byref(nbytes)) == INVALID and lib.eg3d_simplify_query_workspace(C.byref(sp()), None) == INVALID
    for name, fn in dict(entries, query=squery).items():
        for bad in (dict(V=-1), dict(F=-1)):
            assert fn(**bad) == INVALID, (name, bad)
        for bad in (dict(V=BIG), dict(F=BIG), dict(V=1 << 40, F=1 << 40)):
            assert fn(**bad) == TOO_LARGE, (name, bad)
    for name in entries:
        assert getattr(lib, 'eg3d_simplify_' + name)(None, None) == INVALID, name
    nan, inf = float('nan'), float('inf')
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(origin=(nan, 0, 0)), dict(origin=(0, inf, 0)), dict(origin=(0, 0, -inf)),
                dict(flags=None), dict(verts=None), dict(keys=None)):
        assert entries['keys'](**bad) == INVALID, bad
    for bad in (dict(sorted_keys=None), dict(heads=None)):
        assert entries['heads'](**bad) == INVALID, bad
    for bad in (dict(flags=None), dict(verts=None), dict(order=None), dict(heads=None), dict(head_scan=None), dict(used=None), dict(workspace=None),
                dict(workspace_bytes=need - 1), dict(faces=None), dict(tri=None), dict(alive=None)):
        assert entries['clusters'](**bad) == INVALID, bad
    for bad in (dict(tri=None), dict(alive=None), dict(face_order=None), dict(used=None)):
        assert entries['mark'](**bad) == INVALID, bad
    for bad in (dict(used=None), dict(used_scan=None), dict(vertex_map=None), dict(workspace=None), dict(workspace_bytes=need - 1), dict(out_verts=None),
                dict(out_faces=None), dict(tri=None), dict(alive=None), dict(alive_scan=None), dict(out_vert_capacity=-1), dict(out_face_capacity=-1)):
        assert entries['emit'](**bad) == INVALID, bad
    for bad in (dict(out_vert_capacity=BIG), dict(out_face_capacity=BIG)):
        assert entries['emit'](**bad) == TOO_LARGE, bad
    # nothing to do is success without a launch: no vertices and no faces
    empty = dict(V=0, F=0, verts=None, faces=None, keys=None, sorted_keys=None, order=None, heads=None, head_scan=None, tri=None, alive=None, face_order=None,
                 used=None, alive_scan=None, used_scan=None, out_verts=None, out_faces=None, vertex_map=None, out_vert_capacity=0, out_face_capacity=0)
    for name in ('heads', 'mark', 'emit'):
        assert entries[name](**empty) == OK, name

    def mp(**kw):
        return L.SmoothParams(**dict(dict(verts=a, out=b, rowptr=a, cols=a, pinned=a, V=100, nnz=600, iterations=3, lam=0.5, mu=-0.53, workspace=a,
                                          workspace_bytes=1 << 30), **kw))
    mquery = lambda **kw: lib.eg3d_smooth_query_workspace(C.byref(mp(**kw)), C.byref(nbytes))      # noqa: E731
    smooth = lambda **kw: lib.eg3d_smooth(C.byref(mp(**kw)), None)      # noqa: E731
    assert mquery() == OK and nbytes.value >= 100 * 12
    mneed = nbytes.value
    assert mquery(iterations=0) == OK and nbytes.value == 0
    assert lib.eg3d_smooth_query_workspace(None, C.byref(nbytes)) == INVALID and lib.eg3d_smooth_query_workspace(C.byref(mp()), None) == INVALID
    assert lib.eg3d_smooth(None, None) == INVALID
    for fn in (mquery, smooth):
        for bad in (dict(V=-1), dict(nnz=-1), dict(iterations=-1)):
            assert fn(**bad) == INVALID, bad
        for bad in (dict(V=BIG), dict(nnz=BIG)):
            assert fn(**bad) == TOO_LARGE, bad
    for bad in (dict(lam=nan), dict(mu=inf), dict(verts=None), dict(out=None), dict(out=a), dict(rowptr=None), dict(cols=None), dict(workspace=None),
                dict(workspace_bytes=mneed - 1)):
        assert smooth(**bad) == INVALID, bad
    assert smooth(V=0, nnz=0, verts=None, out=None, rowptr=None, cols=None, workspace=None, workspace_bytes=0) == OK


def test_wrappers_and_options_refuse_bad_arguments():
    from inv3d_amd import hipops as H, inference as I
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.coach import InversionCoach
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for call in (lambda: H.mesh_simplify(v, f, 1.0), lambda: H.mesh_smooth(v, f), lambda: I.simplify_mesh(v, f, 2.0), lambda: I.smooth_mesh(v, f, 3)):
        with pytest.raises(Eg3dHipError):
            call()                                                               # CPU tensors: there is no fallback
    for cell in (0.0, -2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            H.mesh_simplify(v, f, cell)
    for origin in ((0.0, 0.0), (float('nan'), 0.0, 0.0), (0.0, float('inf'), 0.0)):
        with pytest.raises(ValueError):
            H.mesh_simplify(v, f, 1.0, origin=origin)
    for bad in (dict(iterations=-1), dict(lam=float('nan')), dict(mu=float('inf'))):
        with pytest.raises(ValueError):
            H.mesh_smooth(v, f, **bad)
    for bad in (dict(simplify=0.0), dict(simplify=-1.0), dict(simplify=float('nan')), dict(smooth=-1)):
        with pytest.raises(ValueError):
            I.extract_mesh(None, None, **bad)                                    # refused before the generator is touched
    kw = dict(gen_mesh=True, mesh_dir='m', w_avg_samples=0)
    for bad in (dict(mesh_simplify=0.0, mesh_format='.ply'), dict(mesh_simplify=float('inf'), mesh_format='.ply'), dict(mesh_smooth=-1, mesh_format='.ply'),
                dict(mesh_simplify=2.0, mesh_format='.mrc'), dict(mesh_smooth=3)):
        with pytest.raises(ValueError):
            InversionCoach(None, **bad, **kw)
