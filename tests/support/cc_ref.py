"""numpy restatement of the grid-components result (include/eg3d_hip.h "Grid components"): what hipops.grid_components must return exactly.

A sequential union-find over every pair (voxel, forward neighbour) of inside voxels -- 3 offsets for connectivity 6, 13 for 26 -- that hooks
the larger root under the smaller, so a set's root is its smallest linear index; the labels are then numbered in ascending order of that
index.  The pairs are gathered with numpy, the unions run in plain Python: a 40^3 grid takes well under a second."""
import itertools

import numpy as np


def forward_offsets(connectivity):
    """The neighbour offsets (d0, d1, d2) with a positive linear offset: half of the 6 or 26 neighbours."""
    if connectivity not in (6, 26):
        raise ValueError(f'connectivity 6 or 26, got {connectivity!r}')
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]
    if connectivity == 6:
        offs = [o for o in offs if sum(abs(c) for c in o) == 1]
    return offs


def inside_mask(vol, level):
    """v > level in fp32: NaN and v == level are outside, +inf is inside."""
    with np.errstate(invalid='ignore'):
        return np.asarray(vol, dtype=np.float32) > np.float32(level)


def _pairs(inside, connectivity):
    idx = np.arange(inside.size, dtype=np.int64).reshape(inside.shape)
    out = []
    for off in forward_offsets(connectivity):
        a = tuple(slice(max(0, -d), inside.shape[k] - max(0, d)) for k, d in enumerate(off))
        b = tuple(slice(max(0, d), inside.shape[k] - max(0, -d)) for k, d in enumerate(off))
        both = inside[a] & inside[b]
        out.append(np.stack([idx[a][both], idx[b][both]], 1))
    return np.concatenate(out, 0)


def label(vol, level, connectivity=6):
    """dict(labels int32 like vol, sizes int32 [K], roots int32 [K], count, inside) of {vol > level}."""
    inside = inside_mask(vol, level)
    parent = list(range(inside.size))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in _pairs(inside, connectivity).tolist():
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    flat = inside.reshape(-1)
    where = np.flatnonzero(flat)
    root_of = np.array([find(int(v)) for v in where], dtype=np.int64)
    roots = np.unique(root_of)                                  # ascending: the numbering
    labels = np.zeros(inside.size, dtype=np.int32)
    labels[where] = (np.searchsorted(roots, root_of) + 1).astype(np.int32)
    sizes = np.bincount(labels[where] - 1, minlength=len(roots)).astype(np.int32)
    return dict(labels=labels.reshape(inside.shape), sizes=sizes, roots=roots.astype(np.int32), count=int(len(roots)), inside=int(len(where)))


def select(sizes, keep=1, min_voxels=0):
    """bool [K]: the `keep` largest components of at least `min_voxels` voxels (keep=None: all of those); ties go to the smaller label."""
    sizes = np.asarray(sizes, dtype=np.int64)
    order = sorted(range(len(sizes)), key=lambda i: (-int(sizes[i]), i))
    order = [i for i in order if sizes[i] >= min_voxels]
    if keep is not None:
        order = order[:max(int(keep), 0)]
    mask = np.zeros(len(sizes), dtype=bool)
    mask[order] = True
    return mask


def keep_grid(vol, labels, keep_mask, fill=-1000.0):
    """np.where(keep[labels], vol, fill) with label 0 always kept."""
    table = np.concatenate([[True], np.asarray(keep_mask, dtype=bool)])
    return np.where(table[labels], np.asarray(vol, dtype=np.float32), np.float32(fill)).astype(np.float32)
