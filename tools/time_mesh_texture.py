"""Textured meshes at full size (DESIGN.md 3.4 "Mesh texture"): hipops.mesh_texture on the full-size synthetic generator's 512^3 mesh -- cleaned
(the largest component), simplified at cell 2 and at cell 4 -- with tile 8 and 16 views (a frontal camera in front of the default 15) at the
generator's image resolution.  Beside the fused kernel, the same atlas composed from operations that existed before it: torch interpolation of
the three vertices to per-texel points, normals and fallbacks, eg3d_mesh_bake on that point list, and a scatter of its rgb / views into the
atlas (the texel -> face tables of the layout are built once outside the timed window, which favours the composition).  Device events, the
two alternating, median and range of 7 windows after a warm-up.  Reports milliseconds, the atlas size, the bytes each has to move and the
fused kernel's achieved bytes per second against the 6.29 TB/s a float4 copy reaches on this GPU, and whether the two atlases are the same bytes.

  python tools/time_mesh_texture.py [--grid 512] [--quantile 0.7] [--tile 8] [--cells 2 4] [--out result.json]"""
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
COPY_TBPS = 6.29                                          # measured float4 copy, MI355X


def alternate_ms(fns, reps):
    """{name: (median, min, max)} over WINDOWS windows per function, the functions taking turns window by window (one warm-up call each
    first); a window is `reps` calls back to back."""
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


def layout_tables(F, T, dev):
    """The layout as index tables, per owned texel: (flat atlas offset, face, ii, jj, leg) -- include/eg3d_hip.h "Mesh texture" in tensor ops."""
    Ht, Wt = H.mesh_texture_size(F, T)
    y, x = torch.meshgrid(torch.arange(Ht, device=dev), torch.arange(Wt, device=dev), indexing='ij')
    i, j = x % T, y % T
    upper = (i + j) >= T
    face = 2 * ((y // T) * (Wt // T) + x // T) + upper.long()
    own = face < F
    i, j, upper, face = i[own], j[own], upper[own], face[own]
    ii, jj = torch.where(upper, T - 1 - i, i).float(), torch.where(upper, T - 1 - j, j).float()
    leg = torch.where(upper, T - 3, T - 2).float()
    return (y * Wt + x)[own], face, ii, jj, leg


def composed(world, normals, fallback, faces, tables, views, kw, T, fill=128):
    """The atlas from pre-existing operations: rotation and interpolation in torch, eg3d_mesh_bake on the texel list, a scatter."""
    off, face, ii, jj, leg = tables
    f = faces.long()
    v = world[f]                                                              # [F,3,3]
    e = torch.stack([(v[:, 2] - v[:, 1]).square(), (v[:, 0] - v[:, 2]).square(), (v[:, 1] - v[:, 0]).square()], 1)      # [F,3,3]
    e = (e[..., 0] + e[..., 1]) + e[..., 2]
    r = torch.zeros(f.shape[0], dtype=torch.long, device=f.device)
    er = e[:, 0].clone()
    for k in (1, 2):
        win = e[:, k] > er
        r = torch.where(win, torch.full_like(r, k), r)
        er = torch.where(win, e[:, k], er)
    rot = torch.stack([torch.gather(f, 1, ((r + s) % 3)[:, None])[:, 0] for s in range(3)], 1)[face]      # [n,3]: A_0, A_1, A_2 per texel
    b1, b2 = (ii / leg)[:, None], (jj / leg)[:, None]
    b0 = (1.0 - b1) - b2
    mix = lambda a: ((b0 * a[rot[:, 0]] + b1 * a[rot[:, 1]]) + b2 * a[rot[:, 2]]).contiguous()      # noqa: E731
    baked = H.mesh_bake(mix(world), mix(normals), views['images'], views['depth'], views['mask'], views['cams'], fallback=mix(fallback), **kw)
    Ht, Wt = H.mesh_texture_size(f.shape[0], T)
    tex = torch.full((Ht * Wt, 3), fill, dtype=torch.uint8, device=f.device)
    cnt = torch.zeros(Ht * Wt, dtype=torch.uint8, device=f.device)
    tex[off] = baked['rgb']
    cnt[off] = baked['views']
    return tex.view(Ht, Wt, 3), cnt.view(Ht, Wt)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    ap.add_argument('--tile', type=int, default=8)
    ap.add_argument('--cells', type=float, nargs='+', default=(2.0, 4.0))
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    front = torch.cat([INF.lookat_pose(math.pi / 2 + 0.1, math.pi / 2 - 0.05, (0., 0., 0.), 2.7).reshape(1, 16),
                       torch.tensor([[4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.]])], 1).to(dev)
    cams = torch.cat([front, INF.bake_cameras(device=dev)]).contiguous()
    N, T = cams.shape[0], a.tile
    res = dict(grid=a.grid, views=N, tile=T, windows=WINDOWS, settings=[])
    with torch.no_grad():
        grid = INF.density_grid(G, ws, res=a.grid)
        sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]      # torch.quantile takes at most 2^24 elements
        level = float(torch.quantile(sample, a.quantile))
        grid = INF.clean_grid(grid, level, keep=1)[0]
        verts0, faces0 = H.marching_cubes(grid, level)
        res.update(level=level, vertices=verts0.shape[0], faces=faces0.shape[0])
        origin, spacing, axes = INF.grid_frame(G, a.grid)
        images = torch.cat([G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0))['image']
                            for i in range(N)]).float().contiguous()
        res['image_res'] = images.shape[-1]
        iso = H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes, bricks=H.iso_bricks(grid))
        views = dict(images=images, depth=iso['depth'], mask=iso['mask'], cams=cams)
        kw = dict(depth_tol=2.0 * abs(spacing[0]), cos_min=0.1, power=2)
        for cell in a.cells:
            verts, faces, _ = INF.simplify_mesh(verts0, faces0, cell)
            world, wfaces = INF.mesh_to_world(G, verts, faces, a.grid)
            normals = H.mesh_normals(grid, world, origin, spacing, axes)
            fallback = torch.zeros_like(world)
            V, F = world.shape[0], wfaces.shape[0]
            Ht, Wt = H.mesh_texture_size(F, T)
            full = H.mesh_texture(world, normals, wfaces, images, iso['depth'], iso['mask'], cams, fallback=fallback, tile=T, **kw)
            tex, cnt = torch.empty_like(full['texture']), torch.empty_like(full['views'])
            p = L.MeshTextureParams(points=world.data_ptr(), normals=normals.data_ptr(), faces=wfaces.data_ptr(), cams=cams.data_ptr(),
                                    images=images.data_ptr(), depth=iso['depth'].data_ptr(), mask=iso['mask'].data_ptr(), fallback=fallback.data_ptr(),
                                    texture=tex.data_ptr(), views=cnt.data_ptr(), uv=full['uv'].data_ptr(), corner=full['corner'].data_ptr(), V=V, F=F,
                                    N=N, H=images.shape[-1], R=iso['depth'].shape[-1], tile=T, fill=128, **kw)
            lib = L.lib()

            def fused():                                                      # the entry itself: the wrapper's counter read would put a synchronise in the window
                L.check(lib.eg3d_mesh_texture(C.byref(p), L.stream_ptr()), 'mesh_texture')
            tables = layout_tables(F, T, dev)
            owned = int(tables[0].numel())
            t = alternate_ms(dict(fused=fused, composed=lambda: composed(world, normals, fallback, wfaces, tables, views, kw, T)), reps=20)
            ctex, ccnt = composed(world, normals, fallback, wfaces, tables, views, kw, T)
            torch.cuda.synchronize()
            contributing = int(full['views'].sum(dtype=torch.int64))
            # what the fused kernel has to move: every vertex's point, normal and fallback once (36 B), the face indices (12 B), uv and corner
            # (25 B per face), 4 B per texel out, twelve image taps per contributing (texel, view) pair.  Depth and mask taps of the pairs that
            # fall in a frame are not counted (their number is not an output).  The composition adds, per owned texel: the three index and
            # three weight reads of the interpolation (36 B), the interpolated point, normal and fallback written and read back (72 B), and the
            # rgb / views written by the bake, read by the scatter and written again with an 8-byte offset (16 B).
            fused_bytes = 36 * V + 37 * F + 4 * Ht * Wt + 48 * contributing
            composed_bytes = fused_bytes + (36 + 72 + 16) * owned
            s = dict(cell=cell, vertices=V, faces=F, atlas=[Ht, Wt], texels=Ht * Wt, owned_texels=owned, contributing_pairs=contributing,
                     texels_from_views=int((full['views'] > 0).sum()), fused=t['fused'], composed=t['composed'], fused_bytes=fused_bytes,
                     composed_bytes=composed_bytes, composed_over_fused=t['composed']['median_ms'] / t['fused']['median_ms'],
                     fused_effective_GBps=fused_bytes / (t['fused']['median_ms'] * 1e-3) / 1e9)
            s['fused_share_of_copy_bandwidth'] = s['fused_effective_GBps'] / (COPY_TBPS * 1e3)
            s['timed_equals_wrapper'] = bool(torch.equal(tex, full['texture']) and torch.equal(cnt, full['views']))
            s['composed_differing_texels'] = int(((ctex != full['texture']).any(-1) | (ccnt != full['views'])).sum())
            res['settings'].append(s)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
