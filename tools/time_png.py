"""Where the time of a PNG goes (DESIGN.md 3.4 "PNG encoder"): the GPU path of video.write_png / write_pngs split into its stages, against the
host path (filter 0 + zlib level 6, what write_png(encoder='host') runs) and PIL.Image.save on the same arrays, with the three file sizes.

Cases: the texture atlas of tools/time_mesh_texture.py's setting at simplification cell 2, a pivot grid (video.pivot_grid of the synthetic
generator), and eight 512 x 512 frames as one batch (the generator's views, as aligned targets arrive).  Per case the median and range of 7
windows: the row-filter kernel, the deflate + offsets + Adler kernels, the pack kernel (device events), the device-to-host copy, the host CRC-32
with the container, the file write; then the whole calls.

  python tools/time_png.py [--grid 512] [--windows 7] [--skip-atlas] [--out result.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from inv3d_amd import _lib as L, hipops as H, inference as INF, synthetic as S, video as V  # noqa: E402


def stat(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def device_ms(fn, windows):
    out = []
    for _ in range(windows + 1):                                              # the first window warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stat(out[1:])


def host_ms(fn, windows):
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return stat(out)


def time_case(name, batch, windows, tmp):
    """batch: uint8 [N,H,W,3] on the device."""
    from PIL import Image
    N, hh, ww, ch = batch.shape
    lib = L.lib()
    res = dict(case=name, shape=[N, hh, ww, ch], raw_bytes=batch.numel())
    p, keep, offsets = H._png_begin(batch)                                     # everything, once: the workspace stays filled
    off = offsets.cpu()
    total = int(off[-1])
    out = torch.empty(total, dtype=torch.uint8, device=batch.device)

    def stage(k):
        def run():
            p.stages = k
            L.check(lib.eg3d_png_encode(C.byref(p), L.stream_ptr()), 'png_encode')
        return run
    res['filter_kernel_ms'] = device_ms(stage(1), windows)
    res['deflate_kernels_ms'] = device_ms(stage(2), windows)
    res['pack_kernel_ms'] = device_ms(lambda: H._png_pack(p, out, total, total), windows)
    res['download_ms'] = host_ms(lambda: out.cpu(), windows)
    host, offs = out.cpu().numpy(), off.tolist()
    streams = [host[offs[i]:offs[i + 1]].tobytes() for i in range(N)]
    res['host_crc_container_ms'] = host_ms(lambda: [V.png_container(s, hh, ww, ch) for s in streams], windows)
    files = [V.png_container(s, hh, ww, ch) for s in streams]
    paths = [os.path.join(tmp, f'{name}_{i}.png') for i in range(N)]

    def write_files():
        for path, data in zip(paths, files):
            with open(path, 'wb') as f:
                f.write(data)
    res['file_write_ms'] = host_ms(write_files, windows)
    res['gpu_path_total_ms'] = host_ms(lambda: V.write_pngs(paths, batch), windows)
    res['gpu_bytes'] = sum(os.path.getsize(q) for q in paths)
    arrays = batch.cpu().numpy()
    assert all(np.array_equal(np.asarray(Image.open(q)), arrays[i]) for i, q in enumerate(paths))

    def host_path():
        for i, path in enumerate(paths):
            V.write_png(path, arrays[i], encoder='host')
    res['host_path_from_device_ms'] = host_ms(lambda: [V.write_png(q, batch[i], encoder='host') for i, q in enumerate(paths)], windows)
    res['host_path_ms'] = host_ms(host_path, windows)
    res['host_bytes'] = sum(os.path.getsize(q) for q in paths)

    def pil_path():
        for i, path in enumerate(paths):
            Image.fromarray(arrays[i]).save(path)
    res['pil_save_ms'] = host_ms(pil_path, windows)
    res['pil_bytes'] = sum(os.path.getsize(q) for q in paths)
    for q in paths:
        os.remove(q)
    del keep
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    ap.add_argument('--tile', type=int, default=8)
    ap.add_argument('--cell', type=float, default=2.0)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--skip-atlas', action='store_true')
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
    results = []
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        images = torch.cat([G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0))['image']
                            for i in range(cams.shape[0])]).float().contiguous()
        frames = torch.stack([H.image_grid_u8(images[i:i + 1], nrow=1, padding=0) for i in range(8)]).contiguous()
        results.append(time_case('frames_8x512', frames, a.windows, tmp))
        print(json.dumps(results[-1]), flush=True)
        grid_img = V.pivot_grid(G, ws, cams[:1], images[1:2])
        results.append(time_case('pivot_grid', grid_img[None].contiguous(), a.windows, tmp))
        print(json.dumps(results[-1]), flush=True)
        if not a.skip_atlas:
            grid = INF.density_grid(G, ws, res=a.grid)
            sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]
            level = float(torch.quantile(sample, a.quantile))
            grid = INF.clean_grid(grid, level, keep=1)[0]
            verts0, faces0 = H.marching_cubes(grid, level)
            origin, spacing, axes = INF.grid_frame(G, a.grid)
            iso = H.iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes, bricks=H.iso_bricks(grid))
            verts, faces, _ = INF.simplify_mesh(verts0, faces0, a.cell)
            world, wfaces = INF.mesh_to_world(G, verts, faces, a.grid)
            normals = H.mesh_normals(grid, world, origin, spacing, axes)
            tex = H.mesh_texture(world, normals, wfaces, images, iso['depth'], iso['mask'], cams, fallback=torch.zeros_like(world), tile=a.tile,
                                 depth_tol=2.0 * abs(spacing[0]), cos_min=0.1, power=2)['texture']
            del grid, iso
            results.append(time_case(f'atlas_cell{a.cell:g}', tex[None].contiguous(), a.windows, tmp))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(windows=a.windows, results=results), f, indent=1)


if __name__ == '__main__':
    main()
