"""Floater removal at full size (DESIGN.md 3.4 "Grid components"): hipops.grid_components and hipops.grid_keep on the full-size synthetic
generator's 512^3 density grid at the level of the grid's 0.7 quantile (seeded weights do not reach the reference's 10).  Device events,
median and range of 5 windows after a warm-up, the same grid replayed: the wrapper end to end (allocations and its one host synchronise
included), the two library entries alone (eg3d_cc_label: local labelling, border merge, root count, scan; eg3d_cc_finish: ranks, relabel and
sizes) and the keep pass.  Beside them the grid + marching-cubes time tools/extract_mesh.py prints, scipy.ndimage.label on the host for the
same grid when scipy is importable, and the ratio to a byte-count floor (grid read once, one int32 volume written and read for the parents,
labels written; keep reads grid and labels and writes a grid: 7 x 4 bytes per voxel at 4 TB/s).

  python tools/time_grid_components.py [--grid 512] [--quantile 0.7] [--connectivity 6] [--no-scipy] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import _lib as L, hipops as H, inference as INF, synthetic as S  # noqa: E402

WINDOWS = 5
FLOOR_BYTES_PER_VOXEL = 28
FLOOR_BYTES_PER_SECOND = 4e12


def event_ms(fn, reps=1):
    """(median, min, max) over WINDOWS windows of the device time of one fn() (one warm-up call first); a window is `reps` calls back to back."""
    fn()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), calls_per_window=reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    ap.add_argument('--connectivity', type=int, default=6, choices=(6, 26))
    ap.add_argument('--no-scipy', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    res = dict(grid=a.grid, connectivity=a.connectivity)
    with torch.no_grad():
        grid = INF.density_grid(G, ws, res=a.grid)
        sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]        # torch.quantile takes at most 2^24 elements
        level = float(torch.quantile(sample, a.quantile))
        res['level'] = level

        def grid_and_march():
            return H.marching_cubes(INF.density_grid(G, ws, res=a.grid), level)
        res['grid_and_march'] = event_ms(grid_and_march)
        res['marching_cubes'] = event_ms(lambda: H.marching_cubes(grid, level), reps=10)
        cc = H.grid_components(grid, level, a.connectivity)
        K = cc['count']
        res.update(components=K, inside_voxels=cc['inside'], largest=int(cc['sizes'].max()) if K else 0)
        res['grid_components'] = event_ms(lambda: H.grid_components(grid, level, a.connectivity), reps=10)
        # the two entries alone, on buffers allocated once
        lib = L.lib()
        labels = torch.empty(grid.shape, dtype=torch.int32, device=dev)
        p = L.CcParams(vol=grid.data_ptr(), labels=labels.data_ptr(), D0=a.grid, D1=a.grid, D2=a.grid, level=level, connectivity=a.connectivity)
        nbytes = C.c_int64(0)
        L.check(lib.eg3d_cc_query_workspace(C.byref(p), C.byref(nbytes)), 'cc_query_workspace')
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        sizes, roots = torch.empty(max(K, 1), dtype=torch.int32, device=dev), torch.empty(max(K, 1), dtype=torch.int32, device=dev)
        p.workspace, p.workspace_bytes, p.totals = work.data_ptr(), nbytes.value, totals.data_ptr()
        p.count, p.sizes, p.roots = K, sizes.data_ptr(), roots.data_ptr()
        res['workspace_bytes'] = nbytes.value
        label = lambda: L.check(lib.eg3d_cc_label(C.byref(p), L.stream_ptr()), 'cc_label')      # noqa: E731
        res['label_entry'] = event_ms(label, reps=10)

        def both():                                                             # finish consumes the parents: it is timed with label, minus label
            label()
            L.check(lib.eg3d_cc_finish(C.byref(p), L.stream_ptr()), 'cc_finish')
        res['label_and_finish_entries'] = event_ms(both, reps=10)
        assert torch.equal(labels, cc['labels']) and torch.equal(sizes[:K], cc['sizes']) and totals.tolist() == [K, cc['inside']]
        mask = INF.select_components(cc['sizes'], keep=1)
        res['keep'] = event_ms(lambda: H.grid_keep(grid, cc['labels'], mask), reps=10)
        res['select_components'] = event_ms(lambda: INF.select_components(cc['sizes'], keep=1), reps=10)
        res['clean_grid'] = event_ms(lambda: INF.clean_grid(grid, level, keep=1, connectivity=a.connectivity), reps=5)
        cleaned, info = INF.clean_grid(grid, level, keep=1, connectivity=a.connectivity)
        res['removed_voxels'] = info['removed_voxels']
        torch.cuda.synchronize()
    floor_ms = FLOOR_BYTES_PER_VOXEL * grid.numel() / FLOOR_BYTES_PER_SECOND * 1e3
    res['floor_ms'] = floor_ms
    res['label_finish_keep_ms'] = res['label_and_finish_entries']['median_ms'] + res['keep']['median_ms']
    res['over_floor'] = res['label_finish_keep_ms'] / floor_ms
    res['scipy'] = None
    if not a.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            res['scipy'] = 'not importable'
        else:
            host = grid.cpu().numpy()
            t0 = time.perf_counter()
            lab, k = ndimage.label(host > level, structure=ndimage.generate_binary_structure(3, 1 if a.connectivity == 6 else 3))
            res['scipy'] = dict(label_s=time.perf_counter() - t0, components=int(k), labels_equal=bool((lab == cc['labels'].cpu().numpy()).all()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
