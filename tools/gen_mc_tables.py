"""Generate 3dgan-inversion_amd/csrc/mc_tables.h: the 256-case triangle table of the marching-cubes kernel (csrc/marching_cubes.hip).

Conventions (all in the OUTPUT frame x, y, z of the mesh; grid point (i0, i1, i2) is the vertex coordinate (i2, i1, i0)):
  corner c = bx + 2*by + 4*bz   at offset (bx, by, bz); a higher corner number is a higher linear grid index
  edge   e = 4*axis + k         from corner lo to lo + (1 << axis), lo = the k-th corner (ascending) whose bit `axis` is 0
  case     = sum of (1 << c) over the corners that are inside (v > level)

Construction, per case:
  1. on each of the 6 cube faces, segments between the face's crossing edges;
  2. face rule: a face whose two inside corners are diagonal gets two segments, each cutting off one INSIDE corner (the rule reads only
     the face's four signs, so the two cubes sharing a face cut it identically: the mesh has no cracks);
  3. every segment is directed so that the surface's right-hand normal points from the inside corners to the outside ones (toward lower
     values); the directed segments chain into closed loops;
  4. each loop is fan-triangulated from its first vertex: the loop starts at its lowest edge, rotated forward to the first vertex whose fan
     diagonals join no two vertices on a common cube face (a diagonal on a face could otherwise be produced by both cubes sharing it);
  5. at most MAX_TRIS triangles per case: the kernel's per-cube output stride relies on it.

Run:  python tools/gen_mc_tables.py [--check]   (--check: exit 1 if the committed header differs)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), '3dgan-inversion_amd', 'csrc', 'mc_tables.h')
MAX_TRIS = 5

CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def _edges():
    edges = []
    for axis in range(3):
        for lo in range(8):
            if not (lo >> axis) & 1:
                edges.append((lo, lo | (1 << axis), axis))
    return edges


EDGES = _edges()                                     # (lo corner, hi corner, axis)
EDGE_OF = {frozenset((a, b)): e for e, (a, b, _) in enumerate(EDGES)}
# faces: (axis, side); corners in cyclic order around the face
FACES = []
for axis in range(3):
    u, v = [a for a in range(3) if a != axis]
    for side in range(2):
        base = side << axis
        FACES.append((axis, side, [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]))


def _mid(e):
    a, b, _ = EDGES[e]
    return [(CORNERS[a][k] + CORNERS[b][k]) / 2 for k in range(3)]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(a[k] * b[k] for k in range(3))


def _centroid(cs):
    return [sum(CORNERS[c][k] for c in cs) / len(cs) for k in range(3)]


def face_segments(case, face):
    """Directed segments (edge_from, edge_to) the face rule prescribes on `face` for `case`."""
    axis, side, ring = face
    inside = [(case >> c) & 1 for c in ring]
    n_in = sum(inside)
    if n_in in (0, 4):
        return []
    cuts = []                   # (corners on the inside side of the segment, the two crossing edges)
    if n_in == 2 and inside[0] == inside[2]:            # diagonal: cut off each inside corner
        for i in range(4):
            if inside[i]:
                cuts.append(([ring[i]], i))
    elif n_in in (1, 3):                                 # the corner of the minority sign is cut off
        for i in range(4):
            if inside[i] == (1 if n_in == 1 else 0):
                cuts.append(([ring[i]] if n_in == 1 else [ring[j] for j in range(4) if j != i], i))
    else:                                                # two adjacent inside corners: one segment across the face
        for i in range(4):
            if inside[i] and inside[(i + 1) % 4]:
                cuts.append(([ring[i], ring[(i + 1) % 4]], i))
    normal = [0, 0, 0]
    normal[axis] = 1 if side else -1                     # outward normal of the cube face
    segs = []
    for ins, i in cuts:
        if len(ins) == 2:                                # the edges leaving the inside pair
            e1 = EDGE_OF[frozenset((ring[(i - 1) % 4], ring[i]))]
            e2 = EDGE_OF[frozenset((ring[(i + 1) % 4], ring[(i + 2) % 4]))]
        else:                                            # the two edges at the cut-off corner
            e1 = EDGE_OF[frozenset((ring[(i - 1) % 4], ring[i]))]
            e2 = EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))]
        outs = [c for c in ring if c not in ins]
        u = _sub(_centroid(outs), _centroid(ins))        # in the face, from the inside side of the segment to the outside side
        d = _sub(_mid(e2), _mid(e1))
        s = _dot(d, _cross(u, normal))                   # CCW seen from the surface normal (toward the outside corners)
        assert s != 0
        segs.append((e1, e2) if s > 0 else (e2, e1))
    return segs


def case_segments(case):
    return [s for f in FACES for s in face_segments(case, f)]


def _face_of_edges(e1, e2):
    """True if edges e1, e2 lie on a common cube face."""
    c1 = set(EDGES[e1][:2])
    c2 = set(EDGES[e2][:2])
    return any(c1 <= set(f[2]) and c2 <= set(f[2]) for f in FACES)


def case_triangles(case):
    segs = case_segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (case, 'edge starts two segments')
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), (case, 'open loop')
    tris = []
    seen = set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        n = len(loop)
        for r in range(n):
            cand = loop[r:] + loop[:r]
            if all(not _face_of_edges(cand[0], cand[k]) for k in range(2, n - 1)):
                loop = cand
                break
        else:
            raise AssertionError((case, 'no fan apex without a face diagonal', loop))
        for k in range(1, n - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))
    assert len(tris) <= MAX_TRIS, (case, len(tris))
    return tris


def render():
    tables = [case_triangles(c) for c in range(256)]
    lines = ['/* mc_tables.h -- GENERATED by tools/gen_mc_tables.py; do not edit.  Marching-cubes case table (256 cases).',
             ' *   corner c = bx + 2*by + 4*bz at offset (bx, by, bz) of the OUTPUT frame (x = grid i2, y = i1, z = i0)',
             ' *   edge   e = 4*axis + k, from corner mc_edge_lo[e] along `axis` (mc_edge_axis[e]) to mc_edge_lo[e] + (1 << axis)',
             ' *   case     = OR of (1 << c) over the inside corners (v > level)',
             ' *   mc_tri_count[case] triangles, mc_tri_edges[case][3*t + j] their edges; the right-hand normal points toward lower values.',
             ' *   Face rule: a face with diagonal inside corners is cut around each inside corner (crack-free: it reads the face only). */',
             '#ifndef EG3D_MC_TABLES_H', '#define EG3D_MC_TABLES_H', '',
             '#ifndef MC_TABLE', '#define MC_TABLE static const', '#endif', '',
             f'#define MC_MAX_TRIS {MAX_TRIS}', '',
             'MC_TABLE unsigned char mc_edge_lo[12] = {' + ', '.join(str(e[0]) for e in EDGES) + '};',
             'MC_TABLE unsigned char mc_edge_axis[12] = {' + ', '.join(str(e[2]) for e in EDGES) + '};', '']
    lines.append('MC_TABLE unsigned char mc_tri_count[256] = {')
    for r in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(len(t)) for t in tables[r:r + 32]) + ',')
    lines.append('};')
    lines.append('')
    lines.append(f'MC_TABLE signed char mc_tri_edges[256][{3 * MAX_TRIS}] = {{')
    for c, t in enumerate(tables):
        flat = [e for tri in t for e in tri] + [-1] * (3 * MAX_TRIS - 3 * len(t))
        lines.append('    {' + ', '.join(str(e) for e in flat) + f'}},  /* {c:3d} */')
    lines.append('};')
    lines += ['', '#endif /* EG3D_MC_TABLES_H */', '']
    return '\n'.join(lines)


def main():
    text = render()
    if '--check' in sys.argv[1:]:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print('mc_tables.h up to date' if same else 'mc_tables.h differs from the generator')
        sys.exit(0 if same else 1)
    with open(OUT, 'w') as f:
        f.write(text)
    print('wrote', OUT)


if __name__ == '__main__':
    main()
