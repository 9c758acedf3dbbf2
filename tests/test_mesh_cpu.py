"""Shape export, host side (no GPU): the marching-cubes case table (csrc/mc_tables.h, tools/gen_mc_tables.py) checked exhaustively, the
numpy restatement of the kernel (tests/support/mc_ref.py) on analytic fields, the PLY / MRC writers byte for byte, and the C-ABI of the
eg3d_mc_* group (structure layout, host-only workspace query).  Reference: create_geometry, training/coaches/single_id_coach.py:120-163;
convert_sdf_samples_to_ply / convert_mrc, shape_utils.py:40-100."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import mc_ref as M  # noqa: E402

T = M.TABLES
CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def _edge_corners(e):
    lo, ax = int(T['edge_lo'][e]), int(T['edge_axis'][e])
    return lo, lo | (1 << ax)


def _face_ring(axis, side):
    u, v = [a for a in range(3) if a != axis]
    b = side << axis
    return [b, b | (1 << u), b | (1 << u) | (1 << v), b | (1 << v)]


def _edge_id(c1, c2):
    for e in range(12):
        if set(_edge_corners(e)) == {c1, c2}:
            return e
    raise KeyError((c1, c2))


def _tris(case):
    n = int(T['tri_count'][case])
    return [tuple(int(x) for x in T['tri_edges'][case][3 * t:3 * t + 3]) for t in range(n)]


def _boundary(case):
    """Directed edges of the case's triangles that no other triangle of the case uses in reverse: the surface's trace on the cube faces."""
    d = [(t[i], t[(i + 1) % 3]) for t in _tris(case) for i in range(3)]
    return {e for e in d if (e[1], e[0]) not in d}


def _on_face(e, axis, side):
    return set(_edge_corners(e)) <= set(_face_ring(axis, side))


def _rule_segments(case, axis, side):
    """The face rule restated: undirected segments between the face's crossing edges; diagonal inside corners are cut off one by one."""
    ring = _face_ring(axis, side)
    ins = [(case >> c) & 1 for c in ring]
    edges = [_edge_id(ring[i], ring[(i + 1) % 4]) for i in range(4)]        # edges[i] joins ring[i] and ring[i+1]
    cross = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    if not cross:
        return set()
    if len(cross) == 2:
        return {frozenset((edges[cross[0]], edges[cross[1]]))}
    segs = set()
    for i in range(4):                   # four crossings = diagonal: a segment around each INSIDE corner (edges i-1 and i meet at ring[i])
        if ins[i]:
            segs.add(frozenset((edges[(i - 1) % 4], edges[i])))
    return segs


def test_generator_reproduces_the_committed_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_mc_tables.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_table_uses_exactly_the_crossing_edges():
    assert int(T['tri_count'].max()) <= 5 and T['tri_edges'].shape == (256, 15)
    for case in range(256):
        crossing = {e for e in range(12) if ((case >> _edge_corners(e)[0]) & 1) != ((case >> _edge_corners(e)[1]) & 1)}
        used = {e for t in _tris(case) for e in t}
        assert used == crossing, case
        assert all(len(set(t)) == 3 for t in _tris(case)), case
        assert all(int(x) == -1 for x in T['tri_edges'][case][3 * len(_tris(case)):]), case


def test_table_boundary_is_the_face_rule():
    for case in range(256):
        bnd = _boundary(case)
        got = {}
        for a, b in bnd:
            faces = [(ax, s) for ax in range(3) for s in range(2) if _on_face(a, ax, s) and _on_face(b, ax, s)]
            assert len(faces) == 1, (case, a, b)
            got.setdefault(faces[0], set()).add(frozenset((a, b)))
        assert len(bnd) == sum(len(v) for v in got.values()), case
        for ax in range(3):
            for s in range(2):
                assert got.get((ax, s), set()) == _rule_segments(case, ax, s), (case, ax, s)


def test_adjacent_cubes_agree_on_the_shared_face():
    """Cube c1 and its +axis neighbour c2 with the same signs on the shared face cut it with the same segments, in opposite directions."""
    pairs = 0
    for axis in range(3):
        bit = 1 << axis
        for c1 in range(256):
            for c2 in range(256):
                if any(((c1 >> c) & 1) != ((c2 >> (c ^ bit)) & 1) for c in range(8) if c & bit):
                    continue
                pairs += 1
                s1 = {(a, b) for a, b in _boundary(c1) if _on_face(a, axis, 1) and _on_face(b, axis, 1)}
                s2 = {(a, b) for a, b in _boundary(c2) if _on_face(a, axis, 0) and _on_face(b, axis, 0)}

                def shift(e):                  # the same grid edge, seen from the neighbour cube
                    lo, hi = _edge_corners(e)
                    return _edge_id(lo ^ bit, hi ^ bit)
                assert {(shift(b), shift(a)) for a, b in s1} == s2, (axis, c1, c2)
    assert pairs == 3 * 256 * 16


def _field(shape, f):
    i0, i1, i2 = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    return f(i2, i1, i0).astype(np.float32)


def sphere(n=32, r=10.0, c=15.3):
    return _field((n, n, n), lambda x, y, z: r - np.sqrt((x - c) ** 2 + (y - c - 0.2) ** 2 + (z - c + 0.1) ** 2))


def torus(n=40):
    return _field((n, n, n), lambda x, y, z: 4 - np.sqrt((np.sqrt((x - 19.5) ** 2 + (y - 19.7) ** 2) - 10) ** 2 + (z - 19.3) ** 2))


def _closed_oriented(v, f):
    closed, oriented = M.edge_pairing(f)
    assert closed and oriented
    assert f.min() >= 0 and f.max() < len(v)


def test_restatement_sphere():
    v, f = M.marching_cubes(sphere(), 0.0)
    _closed_oriented(v, f)
    assert M.euler(v, f) == 2
    vol = M.signed_volume(v, f)
    assert abs(vol - 4 / 3 * np.pi * 1000) < 0.02 * 4 / 3 * np.pi * 1000, vol
    # the frame is the reference's marching_cubes(vol.transpose(2,1,0)): vertex x runs along the grid's last axis
    g = sphere()
    v2, f2 = M.marching_cubes(np.ascontiguousarray(g[:, :, ::-1]), 0.0)
    assert abs(float(v2[:, 0].mean()) - (31 - float(v[:, 0].mean()))) < 1e-3


def test_restatement_torus_and_two_spheres():
    v, f = M.marching_cubes(torus(), 0.0)
    _closed_oriented(v, f)
    assert M.euler(v, f) == 0 and M.signed_volume(v, f) > 0
    two = _field((40, 40, 40), lambda x, y, z: np.maximum(6 - np.sqrt((x - 10) ** 2 + (y - 12) ** 2 + (z - 11) ** 2),
                                                           7 - np.sqrt((x - 28) ** 2 + (y - 27) ** 2 + (z - 26) ** 2)))
    v, f = M.marching_cubes(two, 0.0)
    _closed_oriented(v, f)
    assert M.euler(v, f) == 4 and M.signed_volume(v, f) > 0


def test_restatement_corners_at_the_level_and_empty():
    g = np.round(_field((24, 24, 24), lambda x, y, z: 8 - np.sqrt((x - 11.5) ** 2 + (y - 11.5) ** 2 + (z - 11.5) ** 2)))
    assert (g == 0).sum() > 100
    v, f = M.marching_cubes(g, 0.0)
    _closed_oriented(v, f)                   # degenerate (zero-area) triangles allowed, the topology stays closed
    assert M.euler(v, f) == 2
    for g in (np.zeros((5, 6, 7), np.float32), np.full((2, 2, 2), 3.0, np.float32)):
        v, f = M.marching_cubes(g, 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_restatement_origin_spacing():
    g = sphere(16, 5.0, 7.4)
    v, f = M.marching_cubes(g, 0.5)
    v2, f2 = M.marching_cubes(g, 0.5, origin=(-1.0, 2.0, 0.5), spacing=(0.25, 2.0, 1.0))
    assert np.array_equal(f, f2)
    assert np.array_equal(v2, v * np.float32([0.25, 2.0, 1.0]) + np.float32([-1.0, 2.0, 0.5]))


def test_write_ply_header_and_payload(tmp_path):
    from inv3d_amd.inference import write_ply
    v = np.random.RandomState(0).randn(5, 3).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 1, 0]], np.int32)
    p = str(tmp_path / 'm.ply')
    write_ply(p, v, f)
    data = open(p, 'rb').read()
    head = (b'ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n'
            b'element face 3\nproperty list uchar int vertex_indices\nend_header\n')
    assert data[:len(head)] == head
    body = data[len(head):]
    assert len(body) == 5 * 12 + 3 * 13
    assert np.array_equal(np.frombuffer(body[:60], '<f4').reshape(5, 3), v)
    rec = np.frombuffer(body[60:], np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    assert np.all(rec['n'] == 3) and np.array_equal(rec['i'], f)
    write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert b'element vertex 0\n' in open(p, 'rb').read() and open(p, 'rb').read().endswith(b'end_header\n')


def test_write_mrc_header_and_payload(tmp_path):
    import torch
    from inv3d_amd.inference import write_mrc
    g = np.random.RandomState(1).randn(3, 4, 5).astype(np.float32)
    for src in (g, torch.from_numpy(g)):
        p = str(tmp_path / 'g.mrc')
        write_mrc(p, src)
        data = open(p, 'rb').read()
        assert len(data) == 1024 + g.size * 4
        h = data[:1024]
        assert struct.unpack_from('<4i', h, 0) == (5, 4, 3, 2)                      # nx = shape[2], ny = shape[1], nz = shape[0], mode 2
        assert struct.unpack_from('<3i', h, 28) == (5, 4, 3)                        # mx, my, mz
        assert struct.unpack_from('<3i', h, 64) == (1, 2, 3)                        # mapc, mapr, maps
        dmin, dmax, dmean = struct.unpack_from('<3f', h, 76)
        assert dmin == g.min() and dmax == g.max()
        assert dmean == np.float32(g.mean(dtype=np.float64))
        assert struct.unpack_from('<f', h, 216)[0] == np.float32(g.std(dtype=np.float64))
        assert struct.unpack_from('<i', h, 108)[0] == 20140
        assert h[208:212] == b'MAP ' and h[212:216] == bytes([0x44, 0x44, 0, 0])
        assert np.array_equal(np.frombuffer(data[1024:], '<f4').reshape(3, 4, 5), g)


def test_mc_params_match_the_header():
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    cls = L.McParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', ' printf("%zu\\n", sizeof(eg3d_mc_params));']
    want = [C.sizeof(cls)]
    for f in cls._fields_:
        src.append(f' printf("%zu\\n", offsetof(eg3d_mc_params, {f[0]}));')
        want.append(getattr(cls, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_mc_workspace_query_is_host_only():
    from inv3d_amd import _lib as L
    lib = L.lib()
    cb, per = C.c_int64(-1), C.c_int64(-1)

    def q(D0, D1, D2, out=True):
        p = L.McParams(D0=D0, D1=D1, D2=D2, level=10.0)
        return lib.eg3d_mc_query_workspace(C.byref(p), C.byref(cb) if out else None, C.byref(per))
    assert q(512, 512, 512) == 0
    assert per.value == 16 and cb.value >= 512 ** 3 // 4096 * 48
    assert q(2, 2, 2) == 0 and cb.value > 0
    assert q(1, 5, 5) == -1 and q(5, 0, 5) == -1 and q(5, 5, -3) == -1
    assert q(4, 4, 4, out=False) == -1
    assert lib.eg3d_mc_query_workspace(None, C.byref(cb), C.byref(per)) == -1
    assert q(2048, 1024, 1024) == -3                                              # 2^31 points
    # the device entries refuse missing buffers before launching anything
    p = L.McParams(D0=4, D1=4, D2=4, level=0.0)
    assert lib.eg3d_mc_count(C.byref(p), None) == -1
    assert lib.eg3d_mc_emit(C.byref(p), None) == -1
