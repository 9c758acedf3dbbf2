"""Grids for the grid-components tests (tests/test_gpu_grid_components.py, tests/test_grid_components_cpu.py, tests/support/cc_digest.py):
(vol fp32, level) by name, built around the tile extents the library exports so that components cross tile faces, edges and corners."""
import numpy as np

LEVEL = 0.5


def _occ(mask):
    return np.where(mask, np.float32(1.0), np.float32(0.0)).astype(np.float32)


def serpentines(shape):
    """Two one-voxel-wide chains winding through the whole grid, never face neighbours of each other.  Chain A runs along full i2 lines at
    even i1 in the slabs i0 = 0, 4, 8, ... over i2 in [0, last - 2], bridged at alternating ends and carried to the next slab by a column at
    i2 = 0; chain B does the same in the slabs i0 = 2, 6, 10, ... over i2 in [2, last] with its columns at i2 = last.  A two-voxel spur of B in
    slab 1 touches a line of A across an edge: two components under connectivity 6, one under 26."""
    D0, D1, D2 = shape
    g = np.zeros(shape, dtype=bool)
    last = D2 - 1
    n1 = (D1 + 1) // 2
    n1 -= n1 % 2                                        # an even number of lines: every slab's path ends where it began along i2
    top = 2 * (n1 - 1)
    for s0, lo, hi, col in ((0, 0, last - 2, 0), (2, 2, last, last)):
        far = hi if col == lo else lo
        for j, a0 in enumerate(range(s0, D0, 4)):
            for m in range(n1):
                g[a0, 2 * m, lo:hi + 1] = True
                if m + 1 < n1:
                    g[a0, 2 * m + 1, far if m % 2 == 0 else col] = True
            if a0 + 4 < D0:
                g[a0 + 1:a0 + 4, top if j % 2 == 0 else 0, col] = True
    g[2, 1, D2 // 2] = True
    g[1, 1, D2 // 2] = True
    return g


def planted_pairs(tile):
    """Shape 2 * tile + 1 with isolated voxel pairs adjacent across a tile face, tile edges and tile corners (forward and backward diagonals)."""
    t0, t1, t2 = tile
    shape = (2 * t0 + 1, 2 * t1 + 1, 2 * t2 + 1)
    g = np.zeros(shape, dtype=bool)
    pairs = [((t0 - 1, 3, 10), (t0, 3, 10)), ((3, t1 - 1, 20), (3, t1, 20)), ((5, 3, t2 - 1), (5, 3, t2)),                 # faces
             ((1, t1 - 1, t2 - 1), (1, t1, t2)), ((1, t1 + 3, t2 - 1), (1, t1 + 2, t2)), ((t0 - 1, t1 - 1, 30), (t0, t1, 30)),      # edges
             ((t0 - 1, t1 + 4, 30), (t0, t1 + 3, 30)), ((t0 - 1, 1, t2 + 3), (t0, 1, t2 + 2)),
             ((t0 - 1, t1 - 1, t2 - 1), (t0, t1, t2)), ((t0 - 1, 2 * t1 - 1, t2), (t0, 2 * t1 - 2, t2 - 1)),                      # corners
             ((t0 - 1, t1 - 5, t2), (t0, t1 - 4, t2 - 1)), ((2 * t0 - 1, t1, 2 * t2 - 1), (2 * t0, t1 - 1, 2 * t2))]
    for a, b in pairs:
        g[a] = True
        g[b] = True
    return g, pairs


def specials(shape, seed):
    """Values exactly at the level, NaN, +-inf, and values on both sides."""
    rng = np.random.RandomState(seed)
    vals = np.array([LEVEL, np.nan, np.inf, -np.inf, 0.0, 1.0, np.nextafter(np.float32(LEVEL), np.float32(1.0)),
                     np.nextafter(np.float32(LEVEL), np.float32(0.0))], dtype=np.float32)
    return vals[rng.randint(0, len(vals), size=shape)]


def make(content, shape, seed=0):
    """(vol fp32 [shape], level)."""
    n = int(np.prod(shape))
    if content == 'all_inside':
        return _occ(np.ones(shape, bool)), LEVEL
    if content == 'all_outside':
        return _occ(np.zeros(shape, bool)), LEVEL
    if content == 'one_voxel':
        g = np.zeros(shape, bool)
        g[tuple(d // 2 for d in shape)] = True
        return _occ(g), LEVEL
    if content.startswith('random_'):
        p = float(content.split('_')[1])
        return np.random.RandomState(seed).rand(*shape).astype(np.float32), np.float32(1.0 - p).item()
    if content == 'checkerboard':
        return _occ(np.indices(shape).sum(0) % 2 == 0), LEVEL
    if content == 'specials':
        return specials(shape, seed), LEVEL
    raise ValueError(content + f' ({n} voxels)')
