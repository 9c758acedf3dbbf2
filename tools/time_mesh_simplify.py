"""Mesh simplification and smoothing at full size (DESIGN.md 3.4 "Mesh simplification and smoothing"): the full-size synthetic generator's 512^3
density grid, the level at the grid's 0.7 quantile (seeded weights do not reach the reference's 10), its marching-cubes mesh.  Reports the
vertex and face counts before and after hipops.mesh_simplify with cells of 2 and 4 voxels, and milliseconds for each simplify, for
hipops.mesh_smooth(iterations=10) on the raw mesh and on the cell-2 mesh, and for marching cubes from the same run, for scale.  A simplify call
synchronises with the host once (its counts), so every call is timed by the host clock around the call and a device synchronise; median and
range of REPEATS calls after a warm-up call.

  python tools/time_mesh_simplify.py [--grid 512] [--quantile 0.7] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import hipops as H, inference as INF, synthetic as S  # noqa: E402

REPEATS = 7


def host_ms(fn):
    """median, min and max over REPEATS calls of the host time of fn() up to a device synchronise (one warm-up call first)"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), repeats=REPEATS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    res = dict(grid=a.grid)
    with torch.no_grad():
        grid = INF.density_grid(G, ws, res=a.grid)
        # the quantile of a strided subsample (torch.quantile takes at most 2^24 elements); the padding's -1000 is part of the grid
        sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]
        level = float(torch.quantile(sample, a.quantile))
        res['level'] = level
        res['marching_cubes'] = host_ms(lambda: H.marching_cubes(grid, level))
        verts, faces = H.marching_cubes(grid, level)
        res['vertices'], res['faces'] = verts.shape[0], faces.shape[0]
        meshes = {}
        for cell in (2.0, 4.0):
            r = H.mesh_simplify(verts, faces, cell)
            meshes[cell] = r
            res[f'simplify_cell_{cell:g}'] = dict(host_ms(lambda: H.mesh_simplify(verts, faces, cell)), vertices=r['verts'].shape[0], faces=r['faces'].shape[0],
                                                  clusters=r['clusters'])
        res['smooth_10_raw'] = host_ms(lambda: H.mesh_smooth(verts, faces, iterations=10))
        res['smooth_10_cell_2'] = host_ms(lambda: H.mesh_smooth(meshes[2.0]['verts'], meshes[2.0]['faces'], iterations=10))
        # the passes alone (the adjacency is built once per call by torch's integer sorts: the difference is its cost)
        rowptr, cols, boundary = H.mesh_adjacency(faces, verts.shape[0])
        res['adjacency_raw'] = host_ms(lambda: H.mesh_adjacency(faces, verts.shape[0]))
        res['directed_edges_raw'] = cols.numel()
        torch.cuda.synchronize()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
