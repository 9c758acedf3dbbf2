"""Shape export from the command line: a latent in, a mesh out (create_geometry's '.ply' branch, training/coaches/single_id_coach.py:120-163;
convert_sdf_samples_to_ply, shape_utils.py:40-100), on the GPU kernels of this package.

  python tools/extract_mesh.py --ws pivot_ws.npy --out face.ply [--weights G.safetensors] [--res 512] [--level 10] [--mrc face.mrc]
                               [--colors [--views N_YAW N_PITCH] [--radiance]] [--keep N] [--min-voxels M] [--connectivity {6,26}]
                               [--simplify CELL] [--smooth N] [--obj [--tile T] [--texture-format {png,jpg}]] [--preview PATH]

--weights: a generator archive (inv3d_amd.weights, tools/convert_eg3d_pickle.py); without it, the full-size synthetic generator
(inv3d_amd.synthetic, seed --seed).  --ws: a [1, num_ws, w_dim] (or [num_ws, w_dim]) .npy latent, e.g. the reference's {image}_ws.npy.
--mrc additionally writes the density grid as create_geometry's '.mrc' branch does.
--colors adds per-vertex normals (nx ny nz) and colours (red green blue) to the PLY (inference.color_mesh; no reference counterpart): colours
blended from N_YAW x N_PITCH rendered views around the frontal camera (default 5 x 3), or with --radiance the generator's own radiance at the vertices, without rendering.
--keep N / --min-voxels M remove floaters first (inference.clean_grid; no reference counterpart): only the N largest connected components of
{sigma > level} that have at least M voxels stay (--connectivity 6: face neighbours, 26: edges and corners too), in the mesh, its colours and the
--mrc grid alike; the components found and kept and the voxels removed are printed.  Without either option nothing is labelled.
--simplify CELL merges the vertices of every CELL-voxel cell into their mean and drops the faces that collapse (inference.simplify_mesh; no
reference counterpart): CELL 2 leaves about a fifth of the faces.  --smooth N runs N Taubin iterations over the result
(inference.smooth_mesh).  With --colors the normals and colours are those of the final vertices.  The counts before and after are printed.
--obj writes a textured mesh instead of a PLY (inference.texture_mesh / write_obj; no reference counterpart): --out names the .obj, and its
.mtl and .png (or .jpg) land beside it.  Two faces share a block of T x T texels (--tile, default 8) baked from the same views as --colors;
a mesh that is too large for a 16384-texel atlas side wants --simplify first.  The atlas size and the share of its texels coloured from
views are printed.
--preview PATH (with --obj or --colors; no reference counterpart) looks at the mesh just written through the rasteriser (inference.render_mesh):
a .png is a grid of the bake cameras, the generator's images above and the mesh below; an .avi is an orbit, generator | mesh.  With --obj the
mesh is drawn with its texture and inference.mesh_fidelity's dict is printed as one JSON line (PSNR against the generator's views, silhouette
agreement with the density surface); with --colors it is drawn with its vertex colours."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--ws', required=True, help='latent .npy, [1, num_ws, w_dim] or [num_ws, w_dim]')
    ap.add_argument('--out', required=True, help='output .ply')
    ap.add_argument('--weights', default=None, help='generator archive; default: the synthetic full-size generator')
    ap.add_argument('--seed', type=int, default=0, help='synthetic generator weights seed')
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--level', type=float, default=10.0)
    ap.add_argument('--mrc', default=None, help='also write the density grid to this .mrc')
    ap.add_argument('--colors', action='store_true', help='write per-vertex normals and colours too')
    ap.add_argument('--views', type=int, nargs=2, default=(5, 3), metavar=('N_YAW', 'N_PITCH'), help='bake views around the frontal camera')
    ap.add_argument('--radiance', action='store_true', help="colour from the generator's radiance at the vertices instead of rendered views")
    ap.add_argument('--keep', type=int, default=None, help='keep only the N largest connected components above the level')
    ap.add_argument('--min-voxels', type=int, default=0, help='drop connected components of fewer voxels')
    ap.add_argument('--connectivity', type=int, default=6, choices=(6, 26))
    ap.add_argument('--simplify', type=float, default=None, metavar='CELL', help='vertex clustering with cells of CELL voxels')
    ap.add_argument('--smooth', type=int, default=0, metavar='N', help='Taubin smoothing iterations')
    ap.add_argument('--obj', action='store_true', help='write --out as an OBJ with an MTL and a texture atlas beside it')
    ap.add_argument('--tile', type=int, default=8, metavar='T', help='texels per side of the block two faces share (4..64)')
    ap.add_argument('--texture-format', default='png', choices=('png', 'jpg'))
    ap.add_argument('--png-gpu', action='store_true', help='encode the PNGs on the GPU (hipops.png_encode: adaptive filters, run-length deflate)')
    ap.add_argument('--preview', default=None, metavar='PATH', help='a .png grid or an .avi orbit of the written mesh, generator beside mesh (with --obj or --colors)')
    a = ap.parse_args()
    if a.preview is not None and (not (a.obj or a.colors) or os.path.splitext(a.preview)[1].lower() not in ('.png', '.avi')):
        ap.error('--preview takes a .png or .avi path and goes with --obj or --colors: a bare mesh has nothing to show')
    if (a.simplify is not None and not a.simplify > 0) or a.smooth < 0:
        ap.error('--simplify takes a positive cell size, --smooth a count >= 0')
    if not 4 <= a.tile <= 64 or (a.obj and a.radiance):
        ap.error('--tile takes 4..64; --obj bakes from views, not with --radiance')
    from inv3d_amd import inference as INF
    dev = torch.device('cuda')
    if a.weights:
        from inv3d_amd.weights import load_generator
        G = load_generator(a.weights, device=dev)
    else:
        from inv3d_amd import synthetic as S
        G = S.make_generator(device=dev)
        S.load_synthetic_weights(G, seed=a.seed)
    ws = torch.from_numpy(np.load(a.ws)).float().to(dev)
    if ws.dim() == 2:
        ws = ws.unsqueeze(0)
    t0 = time.perf_counter()
    grid = INF.density_grid(G, ws, res=a.res)
    from inv3d_amd.hipops import marching_cubes
    cleaned = ''
    if a.keep is not None or a.min_voxels > 0:
        t1 = time.perf_counter()
        grid, info = INF.clean_grid(grid, a.level, keep=a.keep, min_voxels=a.min_voxels, connectivity=a.connectivity)
        torch.cuda.synchronize()
        cleaned = (f'; {info["count"]} components found, {info["kept"].numel()} kept, {info["removed_voxels"]} voxels removed '
                   f'({(time.perf_counter() - t1) * 1e3:.1f} ms)')
    verts, faces = marching_cubes(grid, a.level)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    note = cleaned
    if a.simplify is not None or a.smooth > 0:
        t1 = time.perf_counter()
        v0, f0 = verts.shape[0], faces.shape[0]
        if a.simplify is not None:
            verts, faces, _ = INF.simplify_mesh(verts, faces, a.simplify)
        if a.smooth > 0:
            verts = INF.smooth_mesh(verts, faces, iterations=a.smooth)
        torch.cuda.synchronize()
        note += (f'; from {v0} vertices, {f0} faces' + (f', cells of {a.simplify:g} voxels' if a.simplify is not None else '')
                 + (f', {a.smooth} smoothing iterations' if a.smooth > 0 else '') + f' ({(time.perf_counter() - t1) * 1e3:.1f} ms)')
    if a.obj:
        t1 = time.perf_counter()
        cams = INF.bake_cameras(a.views[0], a.views[1], device=dev)
        att = INF.texture_mesh(G, ws, verts, faces, a.res, level=a.level, grid=grid, cameras=cams, tile=a.tile)
        torch.cuda.synchronize()
        paths = INF.write_obj(a.out, verts, faces, att['uv'], att['texture'], normals=att['normals'], texture_format=a.texture_format,
                              png_encoder='gpu' if a.png_gpu else 'host')
        Ht, Wt = att['texture'].shape[:2]
        nf = faces.shape[0]
        seen, owned = int((att['texture_views'] > 0).sum()), (nf // 2) * a.tile * a.tile + (nf % 2) * a.tile * (a.tile + 1) // 2
        note += (f'; normals + texture {(time.perf_counter() - t1) * 1e3:.1f} ms, atlas {Ht} x {Wt} ({os.path.basename(paths[2])}), '
                 f'{seen} of {owned} owned texels ({100.0 * seen / max(owned, 1):.1f} %) coloured from {cams.shape[0]} views')
    elif a.colors:
        t1 = time.perf_counter()
        cams = INF.bake_cameras(a.views[0], a.views[1], device=dev)
        att = INF.color_mesh(G, ws, verts, a.res, level=a.level, grid=grid, cameras=cams, source='radiance' if a.radiance else 'views')
        torch.cuda.synchronize()
        INF.write_ply(a.out, verts, faces, normals=att['normals'], colors=att['colors'])
        seen = int((att['views'] > 0).sum())
        note += (f'; normals + colours {(time.perf_counter() - t1) * 1e3:.1f} ms, '
                + ('radiance' if a.radiance else f'{seen} of {verts.shape[0]} vertices coloured from {cams.shape[0]} views'))
    else:
        INF.write_ply(a.out, verts, faces)
    if a.mrc:
        INF.write_mrc(a.mrc, grid)
    if a.preview is not None:
        import json
        from inv3d_amd import video as VID
        how = dict(mode='texture', uv=att['uv'], texture=att['texture']) if a.obj else dict(mode='vertex', colors=att['color'])
        if a.preview.lower().endswith('.png'):
            if a.obj:
                tiles = INF.mesh_preview_grid(G, ws, verts, faces, att['uv'], att['texture'], a.res, cameras=cams, nrow=a.views[0])
            else:
                from inv3d_amd.hipops import image_grid_u8
                gen = torch.cat([G.synthesis(ws[:1], cams[i:i + 1], noise_mode='const')['image'].float() for i in range(cams.shape[0])])
                mesh = INF.render_mesh(G, verts, faces, cams, res=gen.shape[-1], grid_res=a.res, **how)['image']
                tiles = image_grid_u8(torch.cat([gen, mesh]).contiguous(), nrow=cams.shape[0], padding=2, pad_value=128)
            VID.write_png(a.preview, tiles, encoder='gpu' if a.png_gpu else 'host')
        else:
            VID.write_mesh_video(G, dict(verts=verts, faces=faces, grid_res=a.res, **{k: v for k, v in how.items() if k != 'mode'}), a.preview,
                                 beside='image', ws=ws, mode=how['mode'])
        if a.obj:
            print(json.dumps(INF.mesh_fidelity(G, ws, verts, faces, att['uv'], att['texture'], grid=grid, level=a.level)))
    print(f'{a.out}: {verts.shape[0]} vertices, {faces.shape[0]} faces ({a.res}^3 grid, level {a.level}; grid + march {dt * 1e3:.1f} ms{note})')


if __name__ == '__main__':
    main()
