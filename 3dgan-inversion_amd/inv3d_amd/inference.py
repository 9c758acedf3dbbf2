"""Inference consumers of the hot path: everything here is a no-grad caller of G.synthesis /
G.mapping / ImportanceRenderer.run_model on the gfx950 kernels.

  lookat_pose, orbit_cameras   <- utils/camera_utils.py:87-105,137-156 and the per-frame cameras of gen_videos.py:105-117
  render_orbit                 <- gen_interp_video, gen_videos.py:63-146 (one latent, 240-frame orbit; frames are returned as tensors:
                                  video.write_orbit_video encodes them on the GPU and writes the file)
  estimate_w_stats             <- mean latent / spread of the projector, training/projectors/w_projector.py:88-97
  density_grid                 <- create_geometry + create_samples, training/coaches/single_id_coach.py:120-186 (sigma on a res^3 grid)
  extract_mesh, write_ply      <- create_geometry's '.ply' branch (single_id_coach.py:155-157) and convert_sdf_samples_to_ply /
                                  convert_mrc, shape_utils.py:40-100: marching cubes on the device (hipops.marching_cubes), no skimage / plyfile
  write_mrc                    <- create_geometry's '.mrc' branch (single_id_coach.py:158-160, mrcfile.new_mmap mode 2), no mrcfile
  grid_frame, render_shape,    no reference counterpart: shaded first-hit views of the density surface from the generator's own cameras
  render_shape_orbit              (hipops.iso_render over density_grid's grid), to look at the recovered shape without an external viewer
  select_components,           no reference counterpart (it exports every blob above the level): floater removal on the density grid --
  clean_grid                      hipops.grid_components labels {sigma > level}, the components to drop are filled with a low value, and one
                                  cleaned grid serves marching cubes, the shaded views, the mesh attributes and the .mrc writer
  mesh_to_world, bake_cameras, no reference counterpart (its meshes are bare x y z): per-vertex normals of the density field and vertex colours
  color_mesh, normals_to_mesh     blended from rendered views that see the vertex (hipops.mesh_normals / mesh_bake), for write_ply's optional
                                  nx ny nz / red green blue properties
  simplify_mesh, smooth_mesh   no reference counterpart (its PLYs carry every marching-cubes triangle): vertex clustering and Taubin
                                  smoothing of the extracted mesh (hipops.mesh_simplify / mesh_smooth), between marching cubes and the attributes
  texture_mesh, write_obj      no reference counterpart: a per-face texture atlas baked from color_mesh's views (hipops.mesh_texture), so that
                                  colour resolution no longer follows the vertex count, and the OBJ + MTL + image that carry it
  render_mesh, render_mesh_orbit, no reference counterpart: views of the exported mesh itself from the generator's cameras (hipops.mesh_raster,
  mesh_fidelity, mesh_preview_grid  a z-buffer rasteriser), registered pixel for pixel with G.synthesis and render_shape; the PSNR of the
                                  textured mesh against the generator's views and its silhouette agreement with the iso-surface marcher

Differences from the reference that do not change results: the tri-planes of a fixed latent are synthesised once per orbit / per grid
instead of once per frame / per chunk (the reference re-runs the backbone every time), and grid coordinates are generated per chunk on
the device instead of materialising res^3 x 3 floats on the host."""
import math
import os
import struct
from typing import Iterator, Optional, Tuple

import numpy as np
import torch


def lookat_pose(h: float, v: float, lookat=(0., 0., 0.), radius: float = 2.7, device='cpu') -> torch.Tensor:
    """cam2world [4,4] of a camera on the sphere of `radius` at yaw h, pitch v looking at `lookat` (y up, no roll)."""
    v = min(max(float(v), 1e-5), math.pi - 1e-5)
    theta = torch.tensor(float(h))
    phi = torch.arccos(torch.tensor(1 - 2 * (v / math.pi)))
    origin = torch.stack([radius * torch.sin(phi) * torch.cos(math.pi - theta), radius * torch.cos(phi),
                          radius * torch.sin(phi) * torch.sin(math.pi - theta)]).float()
    fwd = torch.nn.functional.normalize(torch.as_tensor(lookat, dtype=torch.float32) - origin, dim=0)
    up0 = torch.tensor([0., 1., 0.])
    right = -torch.nn.functional.normalize(torch.linalg.cross(up0, fwd), dim=0)
    up = torch.nn.functional.normalize(torch.linalg.cross(fwd, right), dim=0)
    m = torch.eye(4)
    m[:3, :3] = torch.stack((right, up, fwd), -1)
    m[:3, 3] = origin
    return m.to(device)


def orbit_cameras(num_frames: int = 240, yaw_range: float = 0.35, pitch_range: float = 0.25, radius: float = 2.7, focal: float = 4.2647,
                  lookat=(0., 0., 0.), device='cpu') -> torch.Tensor:
    """[F,25] conditioning vectors (cam2world 16 + intrinsics 9) of the reference's orbit; it spells pi as 3.14 and so does this."""
    K = torch.tensor([focal, 0, 0.5, 0, focal, 0.5, 0, 0, 1.])
    cams = []
    for i in range(num_frames):
        m = lookat_pose(3.14 / 2 + yaw_range * np.sin(2 * 3.14 * i / num_frames), 3.14 / 2 - 0.05 + pitch_range * np.cos(2 * 3.14 * i / num_frames),
                        lookat, radius)
        cams.append(torch.cat([m.reshape(16), K]))
    return torch.stack(cams).to(device)


@torch.no_grad()
def render_orbit(G, ws: torch.Tensor, num_frames: int = 240, image_mode: str = 'image', cameras: Optional[torch.Tensor] = None,
                 with_depth: bool = False, **synthesis_kwargs) -> Iterator[torch.Tensor]:
    """Yields one [3,H,W] (or [1,h,w] for image_depth, normalised to [-1,1] as gen_videos.py:143-145) frame per camera for the single
    latent ws [1,num_ws,w_dim].  The backbone runs once; every frame is rendering + super-resolution.  with_depth=True yields
    (frame, the same render's raw image_depth [1,h,w]) instead -- what images.head_matte(depth=...) takes, without a second render."""
    dev = ws.device
    cams = orbit_cameras(num_frames, device=dev) if cameras is None else cameras.to(dev)
    kw = dict(noise_mode='const', **synthesis_kwargs)
    for i in range(cams.shape[0]):
        out = G.synthesis(ws[:1], cams[i:i + 1], cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)
        img = out[image_mode][0]
        if image_mode == 'image_depth':
            img = -img
            img = (img - img.min()) / (img.max() - img.min()) * 2 - 1
        yield (img, out['image_depth'][0]) if with_depth else img


@torch.no_grad()
def estimate_w_stats(G, num_samples: int = 10000, seed: int = 123, truncation_psi: float = 0.7, truncation_cutoff: int = 14,
                     batch: int = 2048) -> Tuple[torch.Tensor, float]:
    """(w_avg [1,1,w_dim], w_std): statistics of the first latent row over `num_samples` mapped z ~ N(0,1) (numpy RandomState(seed), as
    the reference) conditioned on the canonical frontal camera."""
    dev = next(G.parameters()).device
    cam = torch.cat([lookat_pose(math.pi / 2, math.pi / 2, (0., 0., 0.), 2.7).reshape(1, 16),
                     torch.tensor([[4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.]])], 1).to(dev)
    z = torch.from_numpy(np.random.RandomState(seed).randn(num_samples, G.z_dim)).float()
    rows = []
    for i in range(0, num_samples, batch):
        zb = z[i:i + batch].to(dev)
        rows.append(G.mapping(zb, cam.expand(zb.shape[0], -1), truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff)[:, :1, :].float())
    w = torch.cat(rows, 0)
    w_avg = w.mean(0, keepdim=True)
    w_std = float(((w - w_avg).double().square().sum() / num_samples).sqrt())
    return w_avg, w_std


def _grid_points(res: int, cube_length: float, start: int, stop: int, device) -> torch.Tensor:
    """Points start..stop of create_samples(res, [0,0,0], cube_length): index i -> (i // res^2, (i // res) % res, i % res) scaled to
    [-L/2, L/2].  The reference derives the two slow indices with float32 divisions and `% N`, which leaves fractional parts in the
    coordinates ((i / N) % N is not an integer); reproduced exactly."""
    vs = cube_length / (res - 1)
    idx = torch.arange(start, stop, dtype=torch.long, device=device)
    f = idx.float()
    x = ((f / res) / res) % res
    y = (f / res) % res
    z = (idx % res).float()
    return torch.stack([x, y, z], -1) * vs - cube_length / 2


@torch.no_grad()
def density_grid(G, ws: torch.Tensor, res: int = 512, max_batch: int = 1 << 22, pad: Optional[int] = None, pad_value: float = -1000.0,
                 **synthesis_kwargs) -> torch.Tensor:
    """sigma on the res^3 grid spanning the rendering box, laid out as create_geometry hands it to marching cubes: [res,res,res]
    flipped along axis 0, with a border of int(30*res/256) voxels set to -1000."""
    dev = ws.device
    box = float(G.rendering_kwargs['box_warp'])
    planes = G.backbone.synthesis(ws[:1], noise_mode='const', **synthesis_kwargs)
    planes = planes.view(1, 3, -1, planes.shape[-2], planes.shape[-1])
    total = res ** 3
    sig = torch.empty(total, device=dev)
    for head in range(0, total, max_batch):
        stop = min(total, head + max_batch)
        pts = _grid_points(res, box, head, stop, dev).unsqueeze(0)
        sig[head:stop] = G.renderer.run_model(planes, G.decoder, pts, None, G.rendering_kwargs)['sigma'].reshape(-1)
    g = torch.flip(sig.view(res, res, res), [0]).contiguous()
    pad = int(30 * res / 256) if pad is None else pad
    if pad > 0:
        g[:pad] = pad_value
        g[-pad:] = pad_value
        g[:, :pad] = pad_value
        g[:, -pad:] = pad_value
        g[:, :, :pad] = pad_value
        g[:, :, -pad:] = pad_value
    return g


def select_components(sizes: torch.Tensor, keep: Optional[int] = 1, min_voxels: int = 0) -> torch.Tensor:
    """bool [K] over the components of hipops.grid_components (entry i is label i + 1): the `keep` largest that have at least `min_voxels`
    voxels; keep=None puts no cap on the count.  Ties go to the smaller label.  Plain torch on the device of `sizes` (CPU tensors work): the
    order is that of one int64 key per component, (size << 32) | (2^31 - 1 - index), descending -- not topk's treatment of equal values."""
    sizes = torch.as_tensor(sizes)
    if sizes.dim() != 1:
        raise ValueError(f'select_components: sizes [K], got {tuple(sizes.shape)}')
    if keep is not None and int(keep) < 0:
        raise ValueError(f'select_components: keep >= 0 or None, got {keep!r}')
    K = sizes.shape[0]
    idx = torch.arange(K, dtype=torch.int64, device=sizes.device)
    key = (sizes.to(torch.int64) << 32) | ((1 << 31) - 1 - idx)
    order = torch.argsort(key, descending=True)                 # the keys are distinct: any sort gives this order
    order = order[sizes[order] >= int(min_voxels)]              # a prefix: the keys descend with the sizes
    if keep is not None:
        order = order[:int(keep)]
    mask = torch.zeros(K, dtype=torch.bool, device=sizes.device)
    mask[order] = True
    return mask


def _wants_cleaning(keep, min_voxels) -> bool:
    return keep is not None or int(min_voxels) > 0


@torch.no_grad()
def clean_grid(grid: torch.Tensor, level: float, keep: Optional[int] = 1, min_voxels: int = 0, connectivity: int = 6, fill: float = -1000.0):
    """(cleaned grid, info): `grid` with every connected component of {grid > level} that select_components(keep, min_voxels) drops filled with
    `fill` (hipops.grid_components, then hipops.grid_keep; the input is not modified).  Components are separated by voxels at or below the
    level, so on the kept ones marching cubes and the ray marcher see the samples they saw before.  fill must be finite and not above the
    level (density_grid's padding value by default).  info: count (components found), kept (int64 labels, ascending), sizes (int32 [count]),
    removed_voxels."""
    from .hipops import grid_components, grid_keep
    fill = float(fill)
    if not math.isfinite(fill):
        raise ValueError(f'clean_grid: fill must be finite, got {fill}')
    if fill > float(level):
        raise ValueError(f'clean_grid: fill {fill} is above the level {level}: the removed components would stay inside')
    if connectivity not in (6, 26):
        raise ValueError(f'clean_grid: connectivity 6 or 26, got {connectivity!r}')
    cc = grid_components(grid, level, connectivity)
    mask = select_components(cc['sizes'], keep=keep, min_voxels=min_voxels)
    removed = int(cc['sizes'][~mask].to(torch.int64).sum()) if cc['count'] else 0
    info = dict(count=cc['count'], kept=torch.nonzero(mask).reshape(-1) + 1, sizes=cc['sizes'], removed_voxels=removed)
    if removed == 0:
        return grid, info
    return grid_keep(grid, cc['labels'], mask, fill), info


def _check_mesh_options(simplify, smooth, what: str) -> None:
    if simplify is not None and not (float(simplify) > 0.0 and math.isfinite(float(simplify))):
        raise ValueError(f'{what}: simplify must be a positive finite cell size or None, got {simplify!r}')
    if int(smooth) < 0:
        raise ValueError(f'{what}: smooth must be >= 0 iterations, got {smooth!r}')


@torch.no_grad()
def simplify_mesh(verts: torch.Tensor, faces: torch.Tensor, cell: float, origin=(0.0, 0.0, 0.0)):
    """(verts, faces, info): the mesh with the vertices of every cell of side `cell` (in the vertices' own units: voxels for extract_mesh's
    output) merged into their mean, collapsed and repeated faces dropped (hipops.mesh_simplify; the inputs are not modified).  Cell 2 leaves
    about a fifth of a marching-cubes mesh's faces, cell 4 about a seventeenth.  Placement is the members' mean, not a quadric minimiser: the
    result is reproducible to the bit, and on a marching-cubes mesh, whose vertices already lie on the surface at sub-voxel spacing, the mean
    stays within the cell's extent of it.  info: clusters (occupied cells), vertex_map (int32 per input vertex, -1 where its cluster went)."""
    from .hipops import mesh_simplify
    r = mesh_simplify(verts, faces, cell, origin)
    return r['verts'], r['faces'], dict(clusters=r['clusters'], vertex_map=r['vertex_map'])


@torch.no_grad()
def smooth_mesh(verts: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                pin_boundary: bool = True) -> torch.Tensor:
    """The vertices after `iterations` Taubin lambda|mu iterations over the faces' edges (hipops.mesh_smooth; the input is not modified): the
    voxel staircase of a marching-cubes mesh goes, the volume stays (the mu pass undoes the lam pass's shrinkage).  Faces are unchanged.
    pin_boundary keeps the rim of an open mesh where it is."""
    from .hipops import mesh_smooth
    return mesh_smooth(verts, faces, iterations=iterations, lam=lam, mu=mu, pin_boundary=pin_boundary)


@torch.no_grad()
def extract_mesh(G, ws: torch.Tensor, res: int = 512, level: float = 10.0, max_batch: int = 1 << 22, attributes: bool = False,
                 keep: Optional[int] = None, min_voxels: int = 0, connectivity: int = 6, simplify: Optional[float] = None, smooth: int = 0,
                 smooth_kwargs: Optional[dict] = None, **synthesis_kwargs):
    """(verts fp32 [V,3], faces int32 [F,3]) on the device: density_grid, then marching cubes at `level` in the coordinates of the reference's
    PLY (marching_cubes(np.transpose(grid, (2,1,0)), level, spacing=[1]*3), origin [0,0,0]: voxel units).  Faces are wound so that their
    right-hand normals point out of the dense region.  Triangles may differ from skimage's Lewiner method in ambiguous cubes; vertices do not.
    attributes=True: (verts, faces, normals fp32 [V,3], colors uint8 [V,3]) with color_mesh's defaults on the same grid; verts and faces are
    those of the plain call.  keep / min_voxels / connectivity: clean_grid first (floater removal); with keep=None and min_voxels=0, the
    default, nothing is labelled and the call is what it was.  simplify (a cell size in voxels) / smooth (Taubin iterations; smooth_kwargs:
    lam, mu, pin_boundary): simplify_mesh with origin 0, then smooth_mesh, after marching cubes; the attributes are then those of the final
    vertices (normals and colours are functions of a vertex's position alone).  With simplify=None and smooth=0, the default, neither runs."""
    from .hipops import marching_cubes
    _check_mesh_options(simplify, smooth, 'extract_mesh')
    grid = density_grid(G, ws, res=res, max_batch=max_batch, **synthesis_kwargs)
    if _wants_cleaning(keep, min_voxels):
        grid = clean_grid(grid, level, keep=keep, min_voxels=min_voxels, connectivity=connectivity)[0]
    verts, faces = marching_cubes(grid, level)
    if simplify is not None:
        verts, faces, _ = simplify_mesh(verts, faces, float(simplify))
    if int(smooth) > 0:
        verts = smooth_mesh(verts, faces, iterations=int(smooth), **(smooth_kwargs or {}))
    if not attributes:
        return verts, faces
    att = color_mesh(G, ws, verts, res, level=level, grid=grid, **synthesis_kwargs)
    return verts, faces, att['normals'], att['colors']


def grid_frame(G, res: int):
    """(origin, spacing, axes) of density_grid(G, ws, res)'s layout for hipops.iso_render: grid index i of grid axis a sits at world coordinate
    origin[a] + i * spacing[a] of world axis axes[a].  Grid axes 0, 1, 2 run along world x, y, z over [-L/2, L/2] (L = box_warp) with
    res points each, and axis 0 is flipped (create_geometry's flip): its index 0 is x = +L/2 and its spacing is negative.
    The reference's float-division skew (_grid_points: the two slow coordinates carry the faster indices' fractions, less than one voxel) is
    ignored: the frame is the regular grid those points were meant to be."""
    box = float(G.rendering_kwargs['box_warp'])
    vs = box / (int(res) - 1)
    return (box / 2, -box / 2, -box / 2), (-vs, vs, vs), (0, 1, 2)


@torch.no_grad()
def render_shape(G, ws: torch.Tensor, cameras: torch.Tensor, res: Optional[int] = None, grid_res: int = 512, level: float = 10.0,
                 grid: Optional[torch.Tensor] = None, keep: Optional[int] = None, min_voxels: int = 0, connectivity: int = 6, **kw) -> dict:
    """Shaded first-hit views of the sigma = level surface of one latent from `cameras` [F,25]: hipops.iso_render's dict (depth, normal, mask,
    shade [F,3,res,res] in [-1,1], bricks) plus 'grid'.  res defaults to the generator's image resolution, so a frame registers pixel for pixel
    with G.synthesis(ws, camera)['image'].  The density grid (density_grid at grid_res, laid out as grid_frame says) is built here unless one is
    passed; pass the returned 'grid' and 'bricks' back in (grid=..., bricks=...) to render more views of the same latent.  Further keywords go to
    hipops.iso_render (step, refine, skip, shade, ambient, background, bricks).  keep / min_voxels / connectivity: the grid (built here or
    passed) goes through clean_grid first, and 'grid' is the cleaned one -- a caller that passes it back in for more views leaves the options
    out, as render_shape_orbit does; bricks passed in must belong to the cleaned grid."""
    from .hipops import iso_render
    if grid is None:
        grid = density_grid(G, ws, res=grid_res)
    if _wants_cleaning(keep, min_voxels):
        grid = clean_grid(grid, level, keep=keep, min_voxels=min_voxels, connectivity=connectivity)[0]
    if grid.dim() != 3 or len(set(grid.shape)) != 1:
        raise ValueError(f'render_shape: a cubic density grid, got {tuple(grid.shape)}')
    origin, spacing, axes = grid_frame(G, grid.shape[0])
    out = iso_render(grid, cameras.to(grid.device), int(G.img_resolution if res is None else res), level, origin, spacing, axes=axes, **kw)
    out['grid'] = grid
    return out


@torch.no_grad()
def render_shape_orbit(G, ws: torch.Tensor, num_frames: int = 240, cameras: Optional[torch.Tensor] = None, res: Optional[int] = None,
                       grid_res: int = 512, level: float = 10.0, grid: Optional[torch.Tensor] = None, keep: Optional[int] = None,
                       min_voxels: int = 0, connectivity: int = 6, **kw) -> Iterator[torch.Tensor]:
    """Yields one shaded [3,res,res] frame per camera of orbit_cameras (or `cameras`), the companion of render_orbit: one density grid and one
    brick pass for the whole orbit, one launch per frame.  keep / min_voxels / connectivity (clean_grid) apply once, with the first frame."""
    dev = ws.device
    cams = orbit_cameras(num_frames, device=dev) if cameras is None else cameras.to(dev)
    state = dict(grid=grid, bricks=kw.pop('bricks', None))
    clean = dict(keep=keep, min_voxels=min_voxels, connectivity=connectivity)
    for i in range(cams.shape[0]):
        out = render_shape(G, ws, cams[i:i + 1], res=res, grid_res=grid_res, level=level, grid=state['grid'], bricks=state['bricks'],
                           **(clean if i == 0 else {}), **kw)
        state = dict(grid=out['grid'], bricks=out['bricks'])
        yield out['shade'][0]


def _mesh_axes(G, res: int):
    """Per vertex column k of marching_cubes' frame (grid point (i0, i1, i2) -> vertex (i2, i1, i0)): (world axis, origin, spacing), and the
    determinant's sign of the voxel -> world map (a signed permutation: -1 means it mirrors)."""
    origin, spacing, axes = grid_frame(G, res)
    cols = [(axes[2 - k], origin[2 - k], spacing[2 - k]) for k in range(3)]
    perm = [c[0] for c in cols]
    sign = 1 if perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1]) else -1
    for c in cols:
        sign = -sign if c[2] < 0 else sign
    return cols, sign


def mesh_to_world(G, verts: torch.Tensor, faces: Optional[torch.Tensor], res: int):
    """(world fp32 [V,3], faces): the vertices marching_cubes / extract_mesh return (voxel units, the (i2, i1, i0) frame of the reference's PLY)
    in world coordinates through grid_frame(G, res): column k is grid axis 2 - k, so world[axes[2-k]] = verts[k] * spacing[2-k] + origin[2-k]
    (a product, then a sum, in fp32).  That is a reversal of the axes plus the flipped grid axis 0; where the map mirrors, the faces come back
    re-wound (columns 1 and 2 swapped) so that right-hand face normals still point out of the dense region.  faces may be None."""
    cols, sign = _mesh_axes(G, res)
    world = torch.empty_like(verts, dtype=torch.float32)
    for k, (w, o, s) in enumerate(cols):
        world[:, w] = verts[:, k].float() * s + o
    if faces is not None and sign < 0:
        faces = faces[:, [0, 2, 1]].contiguous()
    return world, faces


def normals_to_mesh(G, normals: torch.Tensor, res: int) -> torch.Tensor:
    """World-space normals [V,3] in the frame of the mesh vertices (what a PLY carries beside x y z): the inverse of mesh_to_world applied to
    directions.  The grid is cubic with one |spacing|, so it is a permutation with sign changes, exact in fp32."""
    cols, _ = _mesh_axes(G, res)
    return torch.stack([-normals[:, w] if s < 0 else normals[:, w] for (w, _, s) in cols], 1).contiguous()


def bake_cameras(n_yaw: int = 5, n_pitch: int = 3, yaw_range: float = 0.6, pitch_range: float = 0.25, radius: float = 2.7, focal: float = 4.2647,
                 device='cpu') -> torch.Tensor:
    """[n_yaw * n_pitch, 25] lookat_pose views around the frontal camera (yaw pi/2, pitch pi/2) for color_mesh: yaw offsets evenly over
    [-yaw_range, yaw_range], pitch offsets over [-pitch_range, pitch_range] (a single value is offset 0), pitch-major.  Callers may prepend the
    inversion's own camera, the view the photograph constrains best."""
    K = torch.tensor([focal, 0, 0.5, 0, focal, 0.5, 0, 0, 1.])
    span = lambda n, r: [0.0] if n <= 1 else [-r + 2 * r * i / (n - 1) for i in range(n)]     # noqa: E731
    cams = [torch.cat([lookat_pose(math.pi / 2 + dy, math.pi / 2 + dp, (0., 0., 0.), radius).reshape(16), K])
            for dp in span(int(n_pitch), pitch_range) for dy in span(int(n_yaw), yaw_range)]
    return torch.stack(cams).to(device)


def _to_u8(color: torch.Tensor) -> torch.Tensor:
    """x * 127.5 + 128 clamped to [0, 255] and truncated: image_grid_u8's conversion."""
    return (color * 127.5 + 128).clamp(0, 255).to(torch.uint8)


@torch.no_grad()
def _mesh_views(G, ws, verts, res, level, grid, cameras, source, depth_tol, keep, min_voxels, connectivity, what, synthesis_kwargs):
    """What color_mesh and texture_mesh share: (dict(world, world_normals, normals), the radiance fallback [V,3], the rendered views --
    dict(cams, images, depth, mask, depth_tol) -- or None for source='radiance' and for a mesh without vertices)."""
    from .hipops import iso_bricks, iso_render, mesh_normals
    if source not in ('views', 'radiance'):
        raise ValueError(f"{what}: source 'views' or 'radiance', got {source!r}")
    res = int(res)
    if grid is None:
        grid = density_grid(G, ws, res=res)
        if _wants_cleaning(keep, min_voxels):
            grid = clean_grid(grid, level, keep=keep, min_voxels=min_voxels, connectivity=connectivity)[0]
    if tuple(grid.shape) != (res, res, res):
        raise ValueError(f'{what}: a {res}^3 density grid, got {tuple(grid.shape)}')
    dev = grid.device
    verts = verts.to(dev)
    origin, spacing, axes = grid_frame(G, res)
    world, _ = mesh_to_world(G, verts, None, res)
    V = world.shape[0]
    world_normals = mesh_normals(grid, world, origin, spacing, axes)
    out = dict(world=world, world_normals=world_normals, normals=normals_to_mesh(G, world_normals, res))
    fallback = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if V:
        bkw = {k: v for k, v in synthesis_kwargs.items() if k not in ('force_fp32', 'render_uniforms', 'sr_fp16', 'neural_rendering_resolution')}
        planes = G.backbone.synthesis(ws[:1], noise_mode='const', **bkw)
        planes = planes.view(1, 3, -1, planes.shape[-2], planes.shape[-1])
        for head in range(0, V, 1 << 22):
            rgb = G.renderer.run_model(planes, G.decoder, world[head:head + (1 << 22)].unsqueeze(0), None, G.rendering_kwargs)['rgb']
            fallback[head:head + (1 << 22)] = rgb.reshape(-1, rgb.shape[-1])[:, :3].float() * 2 - 1
    if source == 'radiance' or V == 0:
        return out, fallback, None
    cams = (bake_cameras(device=dev) if cameras is None else cameras.to(dev)).float().contiguous()
    kw = dict(noise_mode='const', **synthesis_kwargs)
    images = None
    for i in range(cams.shape[0]):
        img = G.synthesis(ws[:1], cams[i:i + 1], cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image']
        if images is None:
            images = torch.empty((cams.shape[0], *img.shape[1:]), dtype=torch.float32, device=dev)
        images[i] = img[0]
    iso = iso_render(grid, cams, images.shape[-1], level, origin, spacing, axes=axes, bricks=iso_bricks(grid))
    tol = 2.0 * abs(spacing[0]) if depth_tol is None else float(depth_tol)
    return out, fallback, dict(cams=cams, images=images, depth=iso['depth'], mask=iso['mask'], depth_tol=tol)


@torch.no_grad()
def color_mesh(G, ws: torch.Tensor, verts: torch.Tensor, res: int, level: float = 10.0, grid: Optional[torch.Tensor] = None,
               cameras: Optional[torch.Tensor] = None, source: str = 'views', depth_tol: Optional[float] = None, cos_min: float = 0.1,
               power: int = 2, keep: Optional[int] = None, min_voxels: int = 0, connectivity: int = 6, **synthesis_kwargs) -> dict:
    """Normals and colours for the vertices `verts` [V,3] of marching_cubes / extract_mesh at grid resolution `res` and `level`.  Returns a dict:
      world   fp32 [V,3]   the vertices in world coordinates (mesh_to_world)
      normals fp32 [V,3]   unit normals of the density field (hipops.mesh_normals on density_grid's grid, built here unless `grid` is passed)
                           in the frame of `verts` (normals_to_mesh: what a PLY carries); 'world_normals' has them in world coordinates
      color   fp32 [V,3]   in [-1,1];  colors uint8 [V,3] = color * 127.5 + 128 clamped and truncated
      views   uint8 [V]    how many views coloured the vertex (0: it carries the fallback)
    source='views': every camera of `cameras` [F,25] (default bake_cameras()) renders one G.synthesis image (noise_mode='const', one backbone
    pass) and one first-hit depth map of the same surface from the same rays (hipops.iso_render at the image resolution, one brick pass);
    hipops.mesh_bake blends the views' samples where the vertex is visible and faces the camera (cos_min, power).  A vertex no view sees takes the
    fallback: the generator's own radiance at the vertex, the first three colour channels of G.renderer.run_model on the planes of ws, * 2 - 1
    as the renderer forms image_raw.  source='radiance': the fallback is the colour and nothing is rendered.
    depth_tol=None means two voxels of the grid in world units: a default chosen from geometry (at 512 pixels over the frame a depth pixel is
    about as wide as a voxel of a 512^3 grid, and the mesh vertex and the marcher's hit differ by interpolation, less than a voxel), not
    tuned on real heads.  keep / min_voxels / connectivity: a grid built here goes through clean_grid first, so that removed floaters neither
    shape the normals nor occlude the views (a grid that is passed in is taken as it is).  Further keywords go to G.synthesis."""
    from .hipops import mesh_bake
    out, fallback, views = _mesh_views(G, ws, verts, res, level, grid, cameras, source, depth_tol, keep, min_voxels, connectivity, 'color_mesh',
                                       synthesis_kwargs)
    if views is None:
        out.update(color=fallback, colors=_to_u8(fallback), views=torch.zeros(fallback.shape[0], dtype=torch.uint8, device=fallback.device))
        return out
    baked = mesh_bake(out['world'], out['world_normals'], views['images'], views['depth'], views['mask'], views['cams'], fallback=fallback,
                      depth_tol=views['depth_tol'], cos_min=cos_min, power=power)
    out.update(color=baked['color'], colors=baked['rgb'], views=baked['views'])
    return out


@torch.no_grad()
def texture_mesh(G, ws: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, res: int, level: float = 10.0, grid: Optional[torch.Tensor] = None,
                 cameras: Optional[torch.Tensor] = None, tile: int = 8, fill: int = 128, depth_tol: Optional[float] = None, cos_min: float = 0.1,
                 power: int = 2, keep: Optional[int] = None, min_voxels: int = 0, connectivity: int = 6, **synthesis_kwargs) -> dict:
    """color_mesh's dict for the mesh (verts [V,3], faces int32 [F,3]) plus a texture atlas baked from the same views:
      texture       uint8 [Ht,Wt,3]  hipops.mesh_texture's atlas, (Ht, Wt) = hipops.mesh_texture_size(F, tile)
      uv            fp32 [F,3,2]     per corner of `faces`, in their order; origin at the top-left texel (write_obj flips v)
      texture_views uint8 [Ht,Wt]    how many views coloured the texel (0: the interpolated radiance fallback, or `fill` where no face lies)
    The views, depth maps, normals and the per-vertex radiance fallback are color_mesh's, rendered once for both bakes, so the per-vertex
    results are color_mesh's bit for bit.  A texture keeps the views' detail whatever the vertex count: it is what simplify_mesh's output
    wants.  Where the voxel -> world map mirrors, the bake runs on mesh_to_world's re-wound faces and uv comes back in the order of `faces`.
    An atlas side above 16384 raises: simplify first or lower `tile`."""
    from .hipops import mesh_bake, mesh_texture, mesh_texture_size
    out, fallback, views = _mesh_views(G, ws, verts, res, level, grid, cameras, 'views', depth_tol, keep, min_voxels, connectivity, 'texture_mesh',
                                       synthesis_kwargs)
    dev = fallback.device
    faces = faces.to(device=dev, dtype=torch.int32).contiguous()
    F = faces.shape[0]
    if views is None:                                     # no vertices: nothing was rendered
        if F:
            raise ValueError(f'texture_mesh: {F} faces without vertices')
        Ht, Wt = mesh_texture_size(0, tile)
        out.update(color=fallback, colors=_to_u8(fallback), views=torch.zeros(0, dtype=torch.uint8, device=dev),
                   texture=torch.full((Ht, Wt, 3), int(fill), dtype=torch.uint8, device=dev), uv=torch.zeros((0, 3, 2), device=dev),
                   texture_views=torch.zeros((Ht, Wt), dtype=torch.uint8, device=dev))
        return out
    kw = dict(fallback=fallback, depth_tol=views['depth_tol'], cos_min=cos_min, power=power)
    baked = mesh_bake(out['world'], out['world_normals'], views['images'], views['depth'], views['mask'], views['cams'], **kw)
    wfaces = mesh_to_world(G, verts, faces, int(res))[1]
    tex = mesh_texture(out['world'], out['world_normals'], wfaces, views['images'], views['depth'], views['mask'], views['cams'], tile=tile, fill=fill,
                       **kw)
    uv = tex['uv'] if wfaces is faces else tex['uv'][:, [0, 2, 1]].contiguous()
    out.update(color=baked['color'], colors=baked['rgb'], views=baked['views'], texture=tex['texture'], uv=uv, texture_views=tex['views'])
    return out


def normals_to_world(G, normals: torch.Tensor, res: int) -> torch.Tensor:
    """The inverse of normals_to_mesh: normals [V,3] in the frame of the mesh vertices (what a PLY or an OBJ carries) in world coordinates."""
    cols, _ = _mesh_axes(G, res)
    world = torch.empty_like(normals, dtype=torch.float32)
    for k, (w, _, s) in enumerate(cols):
        world[:, w] = -normals[:, k].float() if s < 0 else normals[:, k].float()
    return world


RENDER_MESH_MODES = dict(texture=('uv', 'texture'), vertex=('colors',), lambert=('normals',))


@torch.no_grad()
def render_mesh(G, verts: torch.Tensor, faces: torch.Tensor, cameras: torch.Tensor, res: Optional[int] = None, mode: str = 'texture',
                uv: Optional[torch.Tensor] = None, texture: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None,
                normals: Optional[torch.Tensor] = None, grid_res: Optional[int] = None, supersample: int = 1, **kw) -> dict:
    """Views of an extracted mesh from `cameras` [N,25] through the rasteriser (hipops.mesh_raster; no reference counterpart): the mesh as the
    exporters hold it -- verts [V,3] and faces int32 [F,3] in the frame of extract_mesh / write_ply at grid resolution `grid_res` (required: it
    fixes the map to world coordinates), and per mode
      'texture'  uv [F,3,2] and texture uint8 [Ht,Wt,3] of texture_mesh (what write_obj writes)
      'vertex'   colors [V,3]: color_mesh's fp32 'color' in [-1,1], or its uint8 'colors' (shown at the centre of their truncation interval)
      'lambert'  normals [V,3] in the frame of the vertices (color_mesh's 'normals', what a PLY carries): a grey headlight view
    The vertices go through mesh_to_world; where that map mirrors, the faces are re-wound and the uv rows re-ordered with them, as texture_mesh
    does.  res defaults to the generator's image resolution, so a frame registers pixel for pixel with G.synthesis(ws, c)['image'] and with
    render_shape.  Returns hipops.mesh_raster's dict (image, face, z, depth, mask, bary, small_faces, large_faces; face indexes `faces` as
    passed, bary follows the re-wound corner order).  supersample = s > 1 renders at s * res and returns only 'image' [N,3,res,res], averaged
    over s x s blocks (torch's avg_pool2d), and 'coverage' [N,res,res], the blocks' mean of mask.  Further keywords go to hipops.mesh_raster
    (cull, near, background, ambient)."""
    from .hipops import mesh_raster
    if mode not in RENDER_MESH_MODES:
        raise ValueError(f'render_mesh: mode {sorted(RENDER_MESH_MODES)}, got {mode!r}')
    given = dict(uv=uv, texture=texture, colors=colors, normals=normals)
    missing = [k for k in RENDER_MESH_MODES[mode] if given[k] is None]
    if missing:
        raise ValueError(f'render_mesh: mode {mode!r} needs {" and ".join(missing)}')
    if grid_res is None or int(grid_res) < 2:
        raise ValueError('render_mesh: grid_res, the resolution of the grid the mesh was extracted from, is required')
    s = int(supersample)
    if s < 1 or s != supersample:
        raise ValueError(f'render_mesh: supersample is an integer >= 1, got {supersample!r}')
    res = int(G.img_resolution if res is None else res)
    dev = verts.device
    faces = faces.to(device=dev, dtype=torch.int32).contiguous()
    world, wfaces = mesh_to_world(G, verts, faces, int(grid_res))
    rewound = wfaces is not faces
    args = {}
    if mode == 'texture':
        uv = uv.to(device=dev, dtype=torch.float32)
        args = dict(uv=(uv[:, [0, 2, 1]] if rewound else uv).contiguous(), texture=texture.to(dev).contiguous())
    elif mode == 'vertex':
        colors = colors.to(dev)
        args = dict(colors=((colors.float() + (0.5 - 128.0)) / 127.5 if colors.dtype == torch.uint8 else colors.float()).contiguous())
    else:
        args = dict(normals=normals_to_world(G, normals.to(dev), int(grid_res)).contiguous())
    out = mesh_raster(world.contiguous(), wfaces, cameras.to(dev).float().contiguous(), res * s, mode=mode, **args, **kw)
    if s == 1:
        return out
    pool = torch.nn.functional.avg_pool2d
    return dict(image=pool(out['image'], s), coverage=pool(out['mask'].float().unsqueeze(1), s)[:, 0])


@torch.no_grad()
def render_mesh_orbit(G, verts: torch.Tensor, faces: torch.Tensor, num_frames: int = 240, cameras: Optional[torch.Tensor] = None,
                      **kw) -> Iterator[torch.Tensor]:
    """Yields one [3,res,res] frame of the mesh per camera of orbit_cameras (or `cameras`), the companion of render_shape_orbit: one
    render_mesh call per frame, so the workspace is that of one view whatever the orbit's length.  Keywords as render_mesh."""
    dev = verts.device
    cams = orbit_cameras(num_frames, device=dev) if cameras is None else cameras.to(dev)
    for i in range(cams.shape[0]):
        yield render_mesh(G, verts, faces, cams[i:i + 1], **kw)['image'][0]


def fidelity_cameras(device='cpu') -> torch.Tensor:
    """mesh_fidelity's default views: bake_cameras() and three views of the orbit, which no default bake has seen."""
    return torch.cat([bake_cameras(device=device), orbit_cameras(3, device=device)])


@torch.no_grad()
def mesh_fidelity(G, ws: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, uv: torch.Tensor, texture: torch.Tensor,
                  cameras: Optional[torch.Tensor] = None, res: Optional[int] = None, grid_res: Optional[int] = None, level: float = 10.0,
                  grid: Optional[torch.Tensor] = None, raster_kwargs: Optional[dict] = None, **synthesis_kwargs) -> dict:
    """How faithful the textured mesh is to the generator it came from (no reference counterpart), per view of `cameras` (default
    fidelity_cameras()) and as means:
      psnr            the textured frame (render_mesh, mode 'texture', white background) against G.synthesis's image, both mapped to [0,1]
                      (inversion.psnr_01); the generator's background counts against the mesh
      psnr_covered    the same over the pixels the mesh covers
      silhouette_iou  the rasteriser's mask against render_shape's mask of the density surface at `level`
    Returns dict(psnr=[...], psnr_covered=[...], silhouette_iou=[...], mean_psnr, mean_psnr_covered, mean_silhouette_iou, views) of floats.
    grid_res: the grid the mesh was extracted from (default: grid's side); `grid` is built at grid_res unless passed.  A view the mesh does
    not cover at all has psnr_covered nan and is left out of that mean.  Further keywords go to G.synthesis."""
    from .inversion import psnr_01
    dev = ws.device
    if grid is None:
        if grid_res is None:
            raise ValueError('mesh_fidelity: grid or grid_res')
        grid = density_grid(G, ws, res=int(grid_res))
    grid_res = int(grid.shape[0] if grid_res is None else grid_res)
    cams = (fidelity_cameras(dev) if cameras is None else cameras.to(dev)).float().contiguous()
    kw = dict(noise_mode='const', **synthesis_kwargs)
    out = dict(psnr=[], psnr_covered=[], silhouette_iou=[])
    bricks = None
    for i in range(cams.shape[0]):
        c = cams[i:i + 1]
        img = G.synthesis(ws[:1], c, cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image'].float()
        r = int(img.shape[-1] if res is None else res)
        if r != img.shape[-1]:
            raise ValueError(f'mesh_fidelity: res {r} is not the resolution of the generator\'s images, {img.shape[-1]}')
        m = render_mesh(G, verts, faces, c, res=r, mode='texture', uv=uv, texture=texture, grid_res=grid_res, **(raster_kwargs or {}))
        shape = render_shape(G, ws, c, res=r, level=level, grid=grid, bricks=bricks)
        bricks = shape['bricks']
        mm, sm = m['mask'][0] > 0, shape['mask'][0] > 0
        out['psnr'].append(float(psnr_01(m['image'], img)))
        sel = mm.unsqueeze(0).expand(3, -1, -1)
        out['psnr_covered'].append(float(psnr_01(m['image'][0][sel], img[0][sel])) if bool(mm.any()) else float('nan'))
        union = int((mm | sm).sum())
        out['silhouette_iou'].append(int((mm & sm).sum()) / union if union else 1.0)
    for k in ('psnr', 'psnr_covered', 'silhouette_iou'):
        vals = [v for v in out[k] if v == v]
        out['mean_' + k] = sum(vals) / len(vals) if vals else float('nan')
    out['views'] = int(cams.shape[0])
    return out


@torch.no_grad()
def mesh_preview_grid(G, ws: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, uv: torch.Tensor, texture: torch.Tensor, grid_res: int,
                      cameras: Optional[torch.Tensor] = None, nrow: int = 5, raster_kwargs: Optional[dict] = None, **synthesis_kwargs) -> torch.Tensor:
    """uint8 [H',W',3] on the device for video.write_png: the generator's image from every camera of `cameras` (default bake_cameras()) in rows
    of `nrow`, and under them the textured mesh from the same cameras (hipops.image_grid_u8, padding 2)."""
    from .hipops import image_grid_u8
    dev = ws.device
    cams = (bake_cameras(device=dev) if cameras is None else cameras.to(dev)).float().contiguous()
    kw = dict(noise_mode='const', **synthesis_kwargs)
    gen = torch.cat([G.synthesis(ws[:1], cams[i:i + 1], cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image'].float()
                     for i in range(cams.shape[0])])
    mesh = torch.cat([render_mesh(G, verts, faces, cams[i:i + 1], res=gen.shape[-1], mode='texture', uv=uv, texture=texture, grid_res=grid_res,
                                  **(raster_kwargs or {}))['image'] for i in range(cams.shape[0])])
    pad = (-cams.shape[0]) % int(nrow)                  # fill the generator's last row, so that the mesh rows start on a row of their own
    blank = torch.ones((pad, *gen.shape[1:]), device=dev)
    return image_grid_u8(torch.cat([gen, blank, mesh]).contiguous(), nrow=int(nrow), padding=2, pad_value=128)


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path: str, verts, faces, normals=None, colors=None) -> None:
    """Binary little-endian PLY with the header plyfile writes for the reference's dtypes (shape_utils.py:84-97: vertex x, y, z 'f4'; face
    vertex_indices 'i4' x 3 as a list with a uchar count).  normals fp32 [V,3] add 'property float nx / ny / nz', colors uint8 [V,3] add
    'property uchar red / green / blue', in that order after z (the names MeshLab and Blender read); with neither, the file is the reference's."""
    v = _host(verts, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    props, fields = ['property float x', 'property float y', 'property float z'], [('p', '<f4', (3,))]
    if normals is not None:
        props += ['property float nx', 'property float ny', 'property float nz']
        fields.append(('n', '<f4', (3,)))
    if colors is not None:
        props += ['property uchar red', 'property uchar green', 'property uchar blue']
        fields.append(('c', 'u1', (3,)))
    vrec = np.empty(len(v), dtype=np.dtype(fields))
    vrec['p'] = v
    for key, arr, dt in (('n', normals, np.float32), ('c', colors, np.uint8)):
        if arr is not None:
            a = _host(arr, dt).reshape(-1, 3)
            if len(a) != len(v):
                raise ValueError(f'write_ply: {len(a)} attribute rows for {len(v)} vertices')
            vrec[key] = a
    header = '\n'.join(['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', *props,
                        f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']) + '\n'
    rec = np.empty(len(f), dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    rec['n'] = 3
    rec['i'] = f
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(rec.tobytes())


def _obj_rows(tag: str, a: np.ndarray) -> str:
    fmt = tag + ' %.9g' * a.shape[1]                      # 9 significant digits: an fp32 value reads back as itself
    return ''.join(fmt % tuple(r) + '\n' for r in a.tolist())


def write_obj(path: str, verts, faces, uv, texture, normals=None, texture_format: str = 'png', png_encoder: str = 'host') -> tuple:
    """Wavefront OBJ + MTL + image for a textured mesh (texture_mesh's verts, faces, 'uv' and 'texture').  Three files: `path` (the OBJ),
    and beside it stem.mtl and stem.png / stem.jpg with path's stem.  Returns the three paths.
      OBJ  'mtllib stem.mtl', 'usemtl stem', V lines 'v x y z' (the vertices as given: the frame of write_ply, so the two files overlay),
           V lines 'vn' when normals [V,3] are given, 3 F lines 'vt u v' (three per face, v = 1 - uv's: OBJ's origin is bottom-left), and
           F lines 'f a/ta/na b/tb/nb c/tc/nc' ('f a/ta ...' without normals), indices from 1.
      MTL  'newmtl stem', 'Kd 1 1 1', 'map_Kd' with the image's base name.
      image  texture uint8 [Ht,Wt,3]: 'png' through video.write_png (lossless: the atlas bytes; png_encoder 'host' | 'gpu' is its encoder),
           'jpg' through hipops.jpeg_encode on the GPU at 4:4:4 (chroma subsampling would smear neighbouring faces' texels into each other)."""
    if texture_format not in ('png', 'jpg'):
        raise ValueError(f"write_obj: texture_format 'png' or 'jpg', got {texture_format!r}")
    v = _host(verts, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    t = _host(uv, np.float32).reshape(-1, 3, 2)
    if len(t) != len(f):
        raise ValueError(f'write_obj: {len(t)} uv rows for {len(f)} faces')
    n = None if normals is None else _host(normals, np.float32).reshape(-1, 3)
    if n is not None and len(n) != len(v):
        raise ValueError(f'write_obj: {len(n)} normals for {len(v)} vertices')
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f'write_obj: a face index outside [0, {len(v)})')
    tex = texture if isinstance(texture, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(texture))
    if tex.dim() != 3 or tex.shape[2] != 3 or tex.dtype != torch.uint8:
        raise ValueError(f'write_obj: texture uint8 [Ht,Wt,3], got {tuple(tex.shape)} {tex.dtype}')
    base = os.path.splitext(path)[0]
    stem = os.path.basename(base)
    mtl_path, img_path = base + '.mtl', f'{base}.{texture_format}'
    if texture_format == 'png':
        from .video import write_png
        write_png(img_path, tex, encoder=png_encoder)
    else:
        from .hipops import jpeg_encode
        data, offsets = jpeg_encode((tex if tex.is_cuda else tex.cuda()).permute(2, 0, 1).unsqueeze(0).contiguous(), subsampling='444')
        with open(img_path, 'wb') as fh:
            fh.write(data[int(offsets[0]):int(offsets[1])].cpu().numpy().tobytes())
    with open(mtl_path, 'w') as fh:
        fh.write(f'newmtl {stem}\nKd 1 1 1\nmap_Kd {os.path.basename(img_path)}\n')
    vt = t.reshape(-1, 2).astype(np.float64)
    vt[:, 1] = 1.0 - vt[:, 1]
    a = f.astype(np.int64) + 1
    ti = np.arange(1, 3 * len(f) + 1, dtype=np.int64).reshape(-1, 3)
    if n is None:
        rows = np.stack([a[:, 0], ti[:, 0], a[:, 1], ti[:, 1], a[:, 2], ti[:, 2]], 1)
        ffmt = 'f %d/%d %d/%d %d/%d\n'
    else:
        rows = np.stack([a[:, 0], ti[:, 0], a[:, 0], a[:, 1], ti[:, 1], a[:, 1], a[:, 2], ti[:, 2], a[:, 2]], 1)
        ffmt = 'f %d/%d/%d %d/%d/%d %d/%d/%d\n'
    with open(path, 'w') as fh:
        fh.write(f'mtllib {os.path.basename(mtl_path)}\nusemtl {stem}\n')
        fh.write(_obj_rows('v', v))
        if n is not None:
            fh.write(_obj_rows('vn', n))
        fh.write(_obj_rows('vt', vt))
        fh.write(''.join(ffmt % tuple(r) for r in rows.tolist()))
    return path, mtl_path, img_path


def write_mrc(path: str, grid) -> None:
    """MRC2014 mode 2 (fp32) file of the [nz, ny, nx] grid as the reference writes it un-transposed (mrcfile.new_mmap(shape=grid.shape,
    mrc_mode=2)): 1024-byte header (nx = shape[2], ny = shape[1], nz = shape[0]; mx/my/mz = the same; cell 0, angles 90; mapc/r/s = 1,2,3;
    dmin/dmax/dmean/rms of the data; ispg 1; nversion 20140; 'MAP '; little-endian stamp 44 44 00 00), then the data, x fastest."""
    if isinstance(grid, torch.Tensor):
        g = grid.detach()
        if g.dim() != 3:
            raise ValueError(f'write_mrc: a 3-D grid, got {tuple(g.shape)}')
        g64 = g.double()
        stats = (float(g.min()), float(g.max()), float(g64.mean()), float(g64.std(unbiased=False)))
        data = _host(g, np.float32)
    else:
        data = _host(grid, np.float32)
        if data.ndim != 3:
            raise ValueError(f'write_mrc: a 3-D grid, got {data.shape}')
        stats = (float(data.min()), float(data.max()), float(data.mean(dtype=np.float64)), float(data.std(dtype=np.float64)))
    nz, ny, nx = data.shape
    h = bytearray(1024)
    struct.pack_into('<10i', h, 0, nx, ny, nz, 2, 0, 0, 0, nx, ny, nz)
    struct.pack_into('<6f', h, 40, 0.0, 0.0, 0.0, 90.0, 90.0, 90.0)
    struct.pack_into('<3i', h, 64, 1, 2, 3)
    struct.pack_into('<3f', h, 76, stats[0], stats[1], stats[2])
    struct.pack_into('<2i', h, 88, 1, 0)
    struct.pack_into('<i', h, 108, 20140)
    h[208:212] = b'MAP '
    h[212:216] = bytes([0x44, 0x44, 0x00, 0x00])
    struct.pack_into('<f', h, 216, stats[3])
    with open(path, 'wb') as fh:
        fh.write(bytes(h))
        fh.write(np.ascontiguousarray(data, dtype='<f4').data)
