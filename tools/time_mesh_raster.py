"""Mesh previews at full size (DESIGN.md 3.4 "Mesh previews"): hipops.mesh_raster in texture mode on the full-size synthetic generator's 512^3
mesh -- cleaned (the largest component) -- and on its cell-2 simplification, one 512^2 frame from one camera, beside one G.synthesis frame
and one iso_render frame of the same grid from the same camera.  The entry itself is timed (the wrapper's counter read would put a
synchronise in the window); device events, the candidates alternating, median and range of 7 windows after a warm-up.  The share of the
large-face path: the same frame drawn from the faces whose pixel range exceeds 8 pixels alone (classified here in torch from the same
projection, so a few faces on the bound may fall on the other side), against the whole frame.

  python tools/time_mesh_raster.py [--grid 512] [--quantile 0.7] [--res 512] [--tile 8] [--out result.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import _lib as L, hipops as H, inference as INF, synthetic as S  # noqa: E402

WINDOWS = 7


def alternate_ms(fns, reps):
    """{name: median / min / max} over WINDOWS windows per function, the functions taking turns window by window (one warm-up call each first)."""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls_per_window=reps) for k, v in out.items()}


def raster_entry(world, faces, cam, res, uv, texture):
    """(a function that runs eg3d_mesh_raster once, the tensors it writes and lends): every output bound, as the wrapper binds them"""
    dev, N, V, F = world.device, cam.shape[0], world.shape[0], faces.shape[0]
    out = dict(image=torch.empty((N, 3, res, res), device=dev), face=torch.empty((N, res, res), dtype=torch.int32, device=dev),
               z=torch.empty((N, res, res), device=dev), depth=torch.empty((N, res, res), device=dev),
               mask=torch.empty((N, res, res), dtype=torch.uint8, device=dev), bary=torch.empty((N, res, res, 3), device=dev))
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    p = L.MeshRasterParams(points=world.data_ptr(), faces=faces.data_ptr(), cams=cam.data_ptr(), uv=uv.data_ptr(), texture=texture.data_ptr(), V=V, F=F, N=N,
                           res=res, Ht=texture.shape[0], Wt=texture.shape[1], mode=L.RASTER_TEXTURE, cull=1, near=0.1, background=1.0, ambient=0.2,
                           bad_faces=counts.data_ptr(), stats=counts.data_ptr() + 4)
    n = C.c_int64(0)
    L.check(L.lib().eg3d_mesh_raster_query_workspace(C.byref(p), C.byref(n)), 'mesh_raster_query_workspace')
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), n.value
    for k, t in out.items():
        setattr(p, k, t.data_ptr())
    lib = L.lib()

    def run():
        L.check(lib.eg3d_mesh_raster(C.byref(p), L.stream_ptr()), 'mesh_raster')
    return run, out, counts, (ws, p)


def large_faces(world, faces, cam, res):
    """bool [F]: the faces whose pixel range in this view is wider or higher than 8 pixels (projection in torch, fp32)"""
    m = cam[0, :16].view(4, 4)
    q = world - m[:3, 3]
    c = q @ m[:3, :3]
    px = (c[:, 0] / c[:, 2] * cam[0, 16] + cam[0, 18]) * res - 0.5
    py = (c[:, 1] / c[:, 2] * cam[0, 20] + cam[0, 21]) * res - 0.5
    f = faces.long()
    span = lambda p: torch.floor(p[f].max(1).values).clamp(max=res - 1) - torch.ceil(p[f].min(1).values).clamp(min=0) + 1      # noqa: E731
    return (span(px) > 8) | (span(py) > 8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--tile', type=int, default=8)
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    cam = torch.cat([INF.lookat_pose(math.pi / 2 + 0.1, math.pi / 2 - 0.05, (0., 0., 0.), 2.7).reshape(1, 16),
                     torch.tensor([[4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.]])], 1).to(dev).contiguous()
    res = dict(grid=a.grid, res=a.res, tile=a.tile, windows=WINDOWS, meshes=[])
    with torch.no_grad():
        grid = INF.density_grid(G, ws, res=a.grid)
        sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]      # torch.quantile takes at most 2^24 elements
        level = float(torch.quantile(sample, a.quantile))
        grid = INF.clean_grid(grid, level, keep=1)[0]
        verts0, faces0 = H.marching_cubes(grid, level)
        origin, spacing, axes = INF.grid_frame(G, a.grid)
        bricks = H.iso_bricks(grid)
        G.synthesis(ws, cam, noise_mode='const', cache_backbone=True)
        others = alternate_ms(dict(synthesis=lambda: G.synthesis(ws, cam, noise_mode='const', use_cached_backbone=True),
                                   iso_render=lambda: H.iso_render(grid, cam, a.res, level, origin, spacing, axes=axes, bricks=bricks)), reps=5)
        res.update(level=level, synthesis=others['synthesis'], iso_render=others['iso_render'])
        for cell in (None, 2.0):
            verts, faces = (verts0, faces0) if cell is None else INF.simplify_mesh(verts0, faces0, cell)[:2]
            world, wfaces = INF.mesh_to_world(G, verts, faces, a.grid)
            world, wfaces = world.contiguous(), wfaces.contiguous()
            F = wfaces.shape[0]
            try:
                Ht, Wt = H.mesh_texture_size(F, a.tile)
            except L.Eg3dHipError:                                             # the full mesh needs a smaller tile for a 16384-texel side
                Ht, Wt = H.mesh_texture_size(F, 4)
            texture = torch.randint(0, 256, (Ht, Wt, 3), dtype=torch.uint8, device=dev)      # the fetch costs the same whatever the texels hold
            uv = torch.rand((F, 3, 2), device=dev)
            big = large_faces(world, wfaces, cam, a.res)
            lf, luv = wfaces[big].contiguous(), uv[big].contiguous()
            whole, out, counts, keep1 = raster_entry(world, wfaces, cam, a.res, uv, texture)
            fns = dict(whole=whole)
            if lf.shape[0]:
                fns['large_only'], _, _, keep2 = raster_entry(world, lf, cam, a.res, luv, texture)
            t = alternate_ms(fns, reps=10)
            torch.cuda.synchronize()
            bad, small, large = counts.tolist()
            m = dict(cell=cell, vertices=world.shape[0], faces=F, atlas=[Ht, Wt], covered=float(out['mask'].float().mean()), bad_faces=bad,
                     small_pairs=small, large_pairs=large, large_classified_here=int(big.sum()), whole=t['whole'], large_only=t.get('large_only'))
            if 'large_only' in t:
                m['large_share_of_time'] = t['large_only']['median_ms'] / t['whole']['median_ms']
            res['meshes'].append(m)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
