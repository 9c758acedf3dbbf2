"""numpy restatement of the mesh simplification and smoothing (csrc/mesh_simplify.hip; include/eg3d_hip.h "Mesh simplification and smoothing"),
step for step: np.float32 arithmetic for the cells and the smoothing, np.add.at (sequential in index order) on float64 for the cluster sums
and on float32 for the neighbour sums.  The GPU outputs are compared with these bit for bit."""
import numpy as np

CELLS = 2 ** 21


class InvalidMesh(ValueError):
    pass


def _check_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise InvalidMesh(f'a face index lies outside [0, {V})')
    return f


def cells(verts, cell, origin=(0.0, 0.0, 0.0)):
    """int64 [V,3] cell per column and bool [V] validity: floor((v - origin) / cell), each operation rounded to fp32."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        c = np.floor((v - np.asarray(origin, np.float32)[None, :]) / np.float32(cell))
        assert c.dtype == np.float32
        ok = np.all((c >= 0) & (c < CELLS), axis=1)          # NaN and the infinities compare false
    return np.where(ok[:, None], c, 0).astype(np.int64), ok


def simplify(verts, faces, cell, origin=(0.0, 0.0, 0.0)):
    """-> dict(verts float32 [V',3], faces int32 [F',3], vertex_map int32 [V], clusters int)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    V = len(v)
    c, ok = cells(v, cell, origin)
    if not ok.all():
        raise InvalidMesh('a vertex is not finite or lies outside the cells [0, 2^21)')
    f = _check_faces(faces, V)
    key = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
    ukeys, vid = np.unique(key, return_inverse=True)         # ascending keys; id(v) = the rank of its key
    vid = vid.reshape(-1)
    K = len(ukeys)
    sums = np.zeros((K, 3), np.float64)
    np.add.at(sums, vid, v.astype(np.float64))               # sequential: members in ascending original index
    n = np.bincount(vid, minlength=K).astype(np.float64)
    cpos = (sums / n[:, None]).astype(np.float32)            # one fp64 division, one rounding to fp32
    g = vid[f] if len(f) else np.zeros((0, 3), np.int64)
    alive = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    shift = np.argmin(g, axis=1) if len(g) else np.zeros(0, np.int64)          # distinct ids on every live face: the smallest is unique
    rot = np.take_along_axis(g, (shift[:, None] + np.arange(3)[None, :]) % 3, axis=1)
    seen = set()
    for i in np.flatnonzero(alive):                          # a face dies if a face of lower index survived with the same rotated triple
        t = (int(rot[i, 0]), int(rot[i, 1]), int(rot[i, 2]))
        if t in seen:
            alive[i] = False
        else:
            seen.add(t)
    rot = rot[alive]
    used = np.zeros(K, bool)
    used[rot.reshape(-1)] = True
    new = np.cumsum(used) - 1                                # ascending key order kept
    vertex_map = np.where(used[vid], new[vid], -1).astype(np.int32) if V else np.zeros(0, np.int32)
    return dict(verts=np.ascontiguousarray(cpos[used]), faces=new[rot].astype(np.int32).reshape(-1, 3), vertex_map=vertex_map, clusters=int(K))


def adjacency(faces, V):
    """(rows, cols) of the directed edges sorted by (row, col): the distinct j != i that share a face edge with i; and bool [V] boundary: the
    endpoints of undirected edges that occur exactly once among the three edges of all faces."""
    f = _check_faces(faces, V)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    und, count = np.unique(np.stack([lo, hi], 1), axis=0, return_counts=True) if len(lo) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    boundary = np.zeros(V, bool)
    boundary[und[count == 1].reshape(-1)] = True
    d = np.concatenate([und, und[:, ::-1]])
    d = d[np.lexsort((d[:, 1], d[:, 0]))]
    return d[:, 0], d[:, 1], boundary


def smooth_pass(p, rows, cols, pinned, factor):
    """One Jacobi pass in fp32: q_i = p_i + f * (sum_j p_j / n - p_i), the sum sequential in ascending j from 0."""
    p = np.ascontiguousarray(p, np.float32)
    s = np.zeros_like(p)
    np.add.at(s, rows, p[cols])                              # unbuffered: one fp32 addition per edge, in the order of the sorted edges
    n = np.bincount(rows, minlength=len(p))
    move = (n > 0) & ~pinned
    q = p.copy()
    m = s[move] / n[move].astype(np.float32)[:, None]
    d = m - p[move]
    q[move] = p[move] + np.float32(factor) * d
    assert q.dtype == np.float32 and m.dtype == np.float32
    return q


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True):
    """-> float32 [V,3]"""
    p = np.ascontiguousarray(verts, np.float32).reshape(-1, 3).copy()
    rows, cols, boundary = adjacency(faces, len(p))
    pinned = boundary if pin_boundary else np.zeros(len(p), bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for _ in range(int(iterations)):
            p = smooth_pass(p, rows, cols, pinned, lam)
            p = smooth_pass(p, rows, cols, pinned, mu)
    return p


def smooth_f64(verts, faces, iterations, lam, mu, pin_boundary=True):
    """The same iteration as a dense float64 operator, p <- p + f (D^-1 A - I) p with pinned and isolated rows zeroed.  Returns (p, largest
    degree, the largest coordinate magnitude any buffer of the run held)."""
    p = np.asarray(verts, np.float64).reshape(-1, 3).copy()
    V = len(p)
    rows, cols, boundary = adjacency(faces, V)
    A = np.zeros((V, V))
    A[rows, cols] = 1.0
    deg = A.sum(1)
    stay = (deg == 0) | (boundary if pin_boundary else False)
    L = A / np.maximum(deg, 1)[:, None] - np.eye(V)
    L[stay] = 0.0
    peak = float(np.abs(p).max())
    for _ in range(int(iterations)):
        for f in (lam, mu):
            p = p + float(np.float32(f)) * (L @ p)
            peak = max(peak, float(np.abs(p).max()))
    return p, int(deg.max()), peak


# ---- test meshes -------------------------------------------------------------------------------------------------------------------------
_MESH = {}


def _march(key, field):
    """marching cubes (tests/support/mc_ref.py) of a field at level 0, computed once and read-only"""
    import mc_ref as MC
    if key not in _MESH:
        v, f = MC.marching_cubes(field().astype(np.float32), 0.0)
        v.setflags(write=False)
        f.setflags(write=False)
        _MESH[key] = (v, f)
    return _MESH[key]


def ball(n=20, radius=7.3, centre=(9.6, 10.2, 9.9)):
    i = np.arange(n, dtype=np.float64)
    return _march(('ball', n, radius, centre), lambda: radius - np.sqrt((i[:, None, None] - centre[0]) ** 2 + (i[None, :, None] - centre[1]) ** 2
                                                                        + (i[None, None, :] - centre[2]) ** 2))


def torus(n=24, major=7.2, minor=3.1, centre=(11.4, 11.7, 11.2)):
    i = np.arange(n, dtype=np.float64)
    x, y, z = i[:, None, None] - centre[0], i[None, :, None] - centre[1], i[None, None, :] - centre[2]
    return _march(('torus', n, major, minor, centre), lambda: minor - np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z))


def soup(n, seed=0, extent=16.0):
    """n random vertices (a quarter of them on integer coordinates: cell borders) and 3 n random faces, repeated indices and repeated faces
    among them"""
    rng = np.random.RandomState(seed)
    v = (rng.rand(n, 3) * extent).astype(np.float32)
    v[::4] = np.floor(v[::4])
    f = rng.randint(0, n, size=(3 * n, 3)).astype(np.int32)
    f[1::7] = f[0::7][:len(f[1::7])][:, [1, 2, 0]]           # the same face, rotated: a duplicate
    f[2::7] = f[0::7][:len(f[2::7])][:, [0, 2, 1]]           # the opposite winding: another face
    return v, f


def planted(origin=(-3.0, 0.5, 2.0), cell=2.0):
    """(verts, faces, expected faces, expected vertex_map, clusters): a hand-built soup in cells relative to a non-zero origin.  Cells (x, y, z):
    A (0,0,0) two vertices, one exactly on the cell's lower corner; B (1,0,0) one vertex exactly on its lower border; C (0,1,0); D (1,1,0);
    E (0,0,1) one vertex; U (5,5,5) one vertex no face uses.  Key order: A, B, C, D, E, U."""
    o = np.asarray(origin, np.float64)
    at = lambda cx, cy, cz, fx=0.5, fy=0.5, fz=0.5: o + cell * np.array([cx + fx, cy + fy, cz + fz])      # noqa: E731
    v = np.array([at(0, 0, 0, 0.0, 0.0, 0.0), at(0, 0, 0, 0.75, 0.25, 0.5), at(1, 0, 0, 0.0, 0.5, 0.5), at(0, 1, 0), at(1, 1, 0, 0.25, 0.0, 0.25),
                  at(0, 0, 1), at(5, 5, 5)], np.float32)
    f = np.array([[2, 3, 0],        # B C A -> (A, B, C)
                  [1, 1, 3],        # a repeated index: dies
                  [0, 1, 2],        # A A B: collapses to an edge
                  [0, 1, 0],        # A A A: collapses to a point
                  [1, 2, 3],        # A B C: a duplicate of face 0 after rotation
                  [3, 2, 1],        # C B A -> (A, C, B): the opposite winding stays
                  [4, 3, 2],        # D C B -> (B, D, C)
                  [5, 0, 4]],       # E A D -> (A, D, E)
                 np.int32)
    want_faces = np.array([[0, 1, 2], [0, 2, 1], [1, 3, 2], [0, 3, 4]], np.int32)
    want_map = np.array([0, 0, 1, 2, 3, 4, -1], np.int32)
    return v, f, want_faces, want_map, 6


def lattice(nx, ny, z=3.0):
    """A flat regular triangulated lattice with small integer coordinates in which every interior vertex's six neighbours are symmetric about
    it: (verts float32 [nx * ny, 3], faces int32)."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    v = np.stack([ix.reshape(-1), iy.reshape(-1), np.full(nx * ny, z)], 1).astype(np.float32)
    idx = lambda i, j: i * ny + j      # noqa: E731
    f = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, np.int32)


def fan(n, seed=0):
    """A closed fan: vertex 0 in the middle of a ring of n vertices (degree n), random heights; plus one vertex no face uses."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([5 + 4 * np.cos(t), 5 + 4 * np.sin(t), rng.rand(n)], 1)
    v = np.concatenate([[[5.0, 5.0, 2.0]], ring, [[1.0, 2.0, 3.0]]]).astype(np.float32)
    f = np.array([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], np.int32)
    return v, f
