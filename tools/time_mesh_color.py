"""Coloured meshes at full size (DESIGN.md 3.4 "Mesh attributes"): the stages of inference.color_mesh on the full-size synthetic generator --
the 512^3 density grid, the level at the grid's 0.7 quantile (seeded weights do not reach the reference's 10), the pivot-like frontal camera
in front of the default 15 bake views, 512^2 images and depth maps.  Device events, median and range of 5 windows after a warm-up.  Reports
milliseconds per stage (grid, marching cubes, view renders, iso depth, normals, bake), the bake's effective bytes per second, and beside it a
plain-torch composite of the same bake (projection in tensor ops, gathered depth taps, F.grid_sample) at the same V and F with its measured
difference from the kernel.

  python tools/time_mesh_color.py [--grid 512] [--quantile 0.7] [--out result.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import hipops as H, inference as INF, synthetic as S  # noqa: E402

WINDOWS = 5


def event_ms(fn, reps=1):
    """(median, min, max) over WINDOWS windows of the device time of one fn() (one warm-up call first); a window is `reps` calls back to
    back, so that a sub-millisecond stage is timed over tens of milliseconds."""
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


def torch_bake(points, normals, images, depth, mask, cams, fallback, depth_tol, cos_min, power):
    """The bake as tensor ops: [F,V] temporaries, gathered depth taps, F.grid_sample for the colours.  Returns (color, views, in-frame pairs,
    contributing pairs)."""
    F, V = cams.shape[0], points.shape[0]
    Hh, R = images.shape[-1], depth.shape[-1]
    m = cams[:, :16].view(F, 4, 4)
    q = points[None] - m[:, None, :3, 3]
    t = q.norm(dim=-1)
    c = torch.einsum('fvi,fij->fvj', q, m[:, :3, :3])
    fx, sk, cx, fy, cy = (cams[:, i, None] for i in (16, 17, 18, 20, 21))
    xl, yl = c[..., 0] / c[..., 2], c[..., 1] / c[..., 2]
    yc = yl * fy + cy
    xc = xl * fx + cx - cy * sk / fy + sk * yc / fy
    live = (t > 0) & (c[..., 2] > 0)
    for r in (Hh, R):
        px, py = xc * r - 0.5, yc * r - 0.5
        live &= (px >= 0) & (px <= r - 1) & (py >= 0) & (py <= r - 1)
    px, py = (xc * R - 0.5).nan_to_num(0).clamp(0, R - 1), (yc * R - 0.5).nan_to_num(0).clamp(0, R - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    x1, y1 = (x0 + 1).clamp(max=R - 1), (y0 + 1).clamp(max=R - 1)
    dflat, mflat = depth.view(F, -1), mask.view(F, -1)
    vis = torch.zeros_like(live)
    for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        idx = yy * R + xx
        vis |= (mflat.gather(1, idx) != 0) & (t <= dflat.gather(1, idx) + depth_tol)
    cos = -(normals[None] * q).sum(-1) / t
    use = live & vis & (cos > cos_min)
    w = torch.where(use, cos ** power, torch.zeros_like(cos))
    grid = torch.stack([xc * 2 - 1, yc * 2 - 1], -1).nan_to_num(0).view(F, 1, V, 2)
    col = torch.nn.functional.grid_sample(images, grid, mode='bilinear', padding_mode='border', align_corners=False)[:, :, 0]      # [F,3,V]
    acc = (col * w[:, None]).sum(0).t()
    wsum = w.sum(0)
    color = torch.where(wsum[:, None] > 0, acc / wsum[:, None].clamp_min(1e-30), fallback)
    return color, use.sum(0), int(live.sum()), int(use.sum())


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
    front = torch.cat([INF.lookat_pose(math.pi / 2 + 0.1, math.pi / 2 - 0.05, (0., 0., 0.), 2.7).reshape(1, 16),
                       torch.tensor([[4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.]])], 1).to(dev)
    cams = torch.cat([front, INF.bake_cameras(device=dev)]).contiguous()
    F = cams.shape[0]
    res = dict(grid=a.grid, views=F)
    with torch.no_grad():
        res['density_grid'] = event_ms(lambda: INF.density_grid(G, ws, res=a.grid))
        grid = INF.density_grid(G, ws, res=a.grid)
        # the quantile of a strided subsample (torch.quantile takes at most 2^24 elements); the padding's -1000 is part of the grid
        sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]
        level = float(torch.quantile(sample, a.quantile))
        res['level'] = level
        res['marching_cubes'] = event_ms(lambda: H.marching_cubes(grid, level), reps=10)
        verts, faces = H.marching_cubes(grid, level)
        V = verts.shape[0]
        res['vertices'], res['faces'] = V, faces.shape[0]
        origin, spacing, axes = INF.grid_frame(G, a.grid)
        world, _ = INF.mesh_to_world(G, verts, None, a.grid)

        def renders():
            return torch.cat([G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0))['image']
                              for i in range(F)]).float().contiguous()
        res['view_renders'] = event_ms(renders)
        images = renders()
        res['image_res'] = images.shape[-1]
        bricks = H.iso_bricks(grid)
        res['iso_depth'] = event_ms(lambda: H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes, bricks=bricks), reps=20)
        iso = H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes, bricks=bricks)
        res['normals'] = event_ms(lambda: H.mesh_normals(grid, world, origin, spacing, axes), reps=200)
        normals = H.mesh_normals(grid, world, origin, spacing, axes)
        fallback = torch.zeros_like(world)
        tol = 2.0 * abs(spacing[0])
        kw = dict(fallback=fallback, depth_tol=tol, cos_min=0.1, power=2)
        res['bake'] = event_ms(lambda: H.mesh_bake(world, normals, images, iso['depth'], iso['mask'], cams, **kw), reps=100)
        baked = H.mesh_bake(world, normals, images, iso['depth'], iso['mask'], cams, **kw)
        targs = (world, normals, images, iso['depth'], iso['mask'], cams, fallback, tol, 0.1, 2)
        res['torch_composite'] = event_ms(lambda: torch_bake(*targs), reps=4)
        tcol, tviews, inframe, contributing = torch_bake(*targs)
        torch.cuda.synchronize()
    # what the algorithm has to move: per vertex 36 B in (point, normal, fallback) and 20 B out (color, rgb, weight, views); per in-frame
    # (vertex, view) pair four depth taps and four mask bytes; per contributing pair twelve image taps
    nbytes = 56 * V + 20 * inframe + 48 * contributing
    res['bake_bytes'] = nbytes
    res['bake_effective_GBps'] = nbytes / (res['bake']['median_ms'] * 1e-3) / 1e9
    res['in_frame_pairs'], res['contributing_pairs'] = inframe, contributing
    res['seen_vertices'] = int((baked['views'] > 0).sum())
    # a vertex whose depth test or cosine sits on the threshold can fall on either side in the composite's differently rounded arithmetic and
    # then takes the fallback in one of the two: counted; the colours are compared where both used the same views
    same = tviews == baked['views'].long()
    res['torch_vs_kernel'] = dict(views_differ=int((~same).sum()),
                                  max_abs_color_diff_where_views_agree=float((tcol - baked['color'])[same].abs().max()) if V else 0.0)
    res['torch_over_kernel'] = res['torch_composite']['median_ms'] / res['bake']['median_ms']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
