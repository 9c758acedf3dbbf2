"""numpy restatement of the marching-cubes kernel (3dgan-inversion_amd/csrc/marching_cubes.hip): the same case table (parsed from
csrc/mc_tables.h), the same fp32 interpolation and the same deterministic vertex / face order, so the GPU output can be compared with it
bit for bit.

  vol [D0, D1, D2] float32, grid point (i0, i1, i2) -> vertex coordinate (i2, i1, i0) (= marching_cubes(vol.transpose(2,1,0)));
  inside iff v > level; one vertex per crossing grid edge, owned by its lower end, ordered by (owner's linear index, axis x, y, z);
  faces ordered by (cube's min-corner linear index, table order)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, '3dgan-inversion_amd', 'csrc', 'mc_tables.h')


def _array(text, name):
    m = re.search(name + r'(?:\[\d+\])+\s*=\s*\{(.*?)\};', text, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    return np.array([int(v) for v in re.findall(r'-?\d+', body)])


def load_tables():
    text = open(HEADER).read()
    return dict(edge_lo=_array(text, 'mc_edge_lo'), edge_axis=_array(text, 'mc_edge_axis'),
                tri_count=_array(text, 'mc_tri_count'), tri_edges=_array(text, 'mc_tri_edges').reshape(256, -1))


TABLES = load_tables()


def marching_cubes(vol, level, origin=None, spacing=None):
    """-> (verts float32 [V,3], faces int32 [F,3]) exactly as the kernel writes them."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    D0, D1, D2 = vol.shape
    level = np.float32(level)
    inside = vol > level
    N = vol.size
    flat = vol.reshape(-1)
    strides = (1, D2, D1 * D2)                                   # output axes x, y, z = grid i2, i1, i0
    i0, i1, i2 = np.meshgrid(np.arange(D0), np.arange(D1), np.arange(D2), indexing='ij')
    pos = [i2.reshape(-1), i1.reshape(-1), i0.reshape(-1)]     # output-frame coordinate of every point
    lim = (D2, D1, D0)
    idx = np.arange(N, dtype=np.int64)
    ins = inside.reshape(-1)
    mask = np.zeros(N, np.int64)
    for a in range(3):
        ok = pos[a] < lim[a] - 1
        cross = np.zeros(N, bool)
        cross[ok] = ins[idx[ok]] != ins[idx[ok] + strides[a]]
        mask |= cross.astype(np.int64) << a
    nv = ((mask >> 0) & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1)
    vbase = np.cumsum(nv) - nv
    V = int(nv.sum())
    verts = np.empty((V, 3), np.float32)
    org = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32)
    spc = np.ones(3, np.float32) if spacing is None else np.asarray(spacing, np.float32)
    for a in range(3):
        sel = ((mask >> a) & 1).astype(bool)
        p = idx[sel]
        lower = mask[sel] & ((1 << a) - 1)
        slot = vbase[sel] + (lower & 1) + ((lower >> 1) & 1)
        va, vb = flat[p], flat[p + strides[a]]
        t = (level - va) / (vb - va)
        for k in range(3):
            c = pos[k][p].astype(np.float32)
            if k == a:
                c = c + t
            verts[slot, k] = c * spc[k] + org[k]
    # cubes
    cube = (pos[0] < D2 - 1) & (pos[1] < D1 - 1) & (pos[2] < D0 - 1)
    cidx = idx[cube]
    case = np.zeros(cidx.shape, np.int64)
    for c in range(8):
        off = (c & 1) * strides[0] + ((c >> 1) & 1) * strides[1] + ((c >> 2) & 1) * strides[2]
        case |= ins[cidx + off].astype(np.int64) << c
    T = TABLES
    ntri = T['tri_count'][case]
    keep = ntri > 0
    cidx, case, ntri = cidx[keep], case[keep], ntri[keep]
    F = int(ntri.sum())
    faces = np.empty((F, 3), np.int32)
    if F:
        rep_cube = np.repeat(np.arange(len(cidx)), ntri)
        tri_in_case = np.arange(F) - np.repeat(np.cumsum(ntri) - ntri, ntri)
        for j in range(3):
            e = T['tri_edges'][case[rep_cube], 3 * tri_in_case + j]
            lo, ax = T['edge_lo'][e], T['edge_axis'][e]
            owner = cidx[rep_cube] + (lo & 1) * strides[0] + ((lo >> 1) & 1) * strides[1] + ((lo >> 2) & 1) * strides[2]
            lower = mask[owner] & ((1 << ax) - 1)
            assert np.all((mask[owner] >> ax) & 1), 'triangle edge without a vertex'
            faces[:, j] = vbase[owner] + (lower & 1) + ((lower >> 1) & 1)
    return verts, faces


# ---- mesh checks -------------------------------------------------------------------------------------------------------------------------

def edge_pairing(faces):
    """(closed, oriented): every undirected edge in exactly two faces, and used in opposite directions by them."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return True, True
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    key = d[:, 0] * n + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])
    _, cnt = np.unique(und, return_counts=True)
    closed = bool(np.all(cnt == 2))
    _, dcnt = np.unique(key, return_counts=True)
    oriented = closed and bool(np.all(dcnt == 1))
    return closed, oriented


def euler(verts, faces):
    f = np.asarray(faces, np.int64)
    used = np.unique(f) if len(f) else np.zeros(0, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]) if len(f) else np.zeros((0, 2), np.int64)
    und = np.unique(np.sort(d, 1), axis=0)
    return len(used) - len(und) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
