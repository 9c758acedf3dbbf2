"""Per-image inversion driver: the caller of the hot path.

Counterpart of the reference's image loop (training/coaches/single_id_coach.py:27-84 on top of base_coach.py:52-99 and
training/projectors/w_projector.py:55-283), reduced to what touches the generator:

    for every image of this rank's shard:
        restore the pristine generator                        (restart_training: a fresh G per image, base_coach.py:52-61)
        Phase A  first_inv_steps of LatentProjector.step()    -> pivot latent (+ optimised camera)
        restore the generator's noise buffers                 (the reference projects on a deep copy of G, w_projector.py:68)
        Phase B  <= max_pti_steps of PivotalTuner.step(), early stop on the perceptual threshold (single_id_coach.py:69)
        metrics: MSE / PSNR of the pivot and of the tuned reconstruction
    one packed-stat all-reduce over the ranks at the end     (inv3d_amd.dist)

Images are independent optimisations, so N GPUs = N shards with no data-path communication (weak scaling).  Shape export is here:
with `gen_mesh` every image's tuned generator writes {mesh_dir}/{name}_pti.mrc (or .ply) at the pivot latent after Phase B, as
global_config.gen_mesh -> create_geometry does (single_id_coach.py:109-110,120-163; inference.density_grid / extract_mesh / write_mrc /
write_ply).  Evaluation is here too: with `do_evaluation` the tuned reconstruction's mse / lpips / msssim / identity (metrics.py: GPU
MS-SSIM, the ArcFace IR-SE-50 identity distance) go to {eval_dir}/{name}metrics.txt, and `save_pivot` writes {name}_ws.npy /
{name}_cam.npy (single_id_coach.py:87-117).  Media export is here as well: with `save_grid` / `gen_video` the pivot grid PNG and the orbit video
are written before Phase B to {media_dir}/pivot/ and again after it to {media_dir}/ (single_id_coach.py:57-62,80-85; video.py: the GPU JPEG
encoder in a Motion-JPEG AVI, since there is no H.264 encoder to call).  Image loading and face alignment are images.py (load_targets gives
the tuples `run` takes); wandb logging of the reference loop is outside this package; the e4e encoder, the pose head and ArcFace are in
e4e.py, pose_net.py and metrics.py.
"""
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import math
import os

import numpy as np
import torch

from . import dist as D
from .inference import (bake_cameras, clean_grid, color_mesh, density_grid, estimate_w_stats, extract_mesh, simplify_mesh, smooth_mesh, texture_mesh,
                        write_mrc, write_obj, write_ply)
from .inversion import LatentProjector, PivotalTuner, psnr_01
from .metrics import IDLoss, format_metrics_txt, reconstruction_metrics
from .video import pivot_grid, write_orbit_video, write_png


@dataclass
class InversionResult:
    name: str
    w_pivot: torch.Tensor                 # [1, num_ws, w_dim]
    cam: torch.Tensor                     # [1, 25]
    psnr_pivot: float
    psnr_tuned: float
    mse_tuned: float
    steps_a: int
    steps_b: int
    tuned_state: Optional[Dict[str, torch.Tensor]] = field(default=None, repr=False)    # generator weights after Phase B (opt-in)
    mesh_path: Optional[str] = None                                                       # the shape written with gen_mesh
    metrics: Optional[Dict[str, float]] = None                                            # mse / lpips / msssim / identity with do_evaluation
    # media export: plain attributes that the coach sets after construction, not constructor arguments (the field list ends with `metrics`)
    grid_paths = None                                                                     # (pivot, tuned) grid PNGs with save_grid
    video_paths = None                                                                    # (pivot, tuned) orbit videos with gen_video


class InversionCoach:
    def __init__(self, G, *, first_inv_steps: int = 400, max_pti_steps: int = 400, lpips_threshold: float = 0.06, first_inv_lr: float = 8e-3,
                 pti_lr: float = 3e-4, optimize_pose: bool = False, use_warping_loss: bool = False, wplus: bool = False,
                 feature_net: Optional[Callable] = None, early_stop_interval: int = 1, use_graph: bool = False, keep_tuned_state: bool = False,
                 synth_kwargs: Optional[dict] = None, seed: int = 0, pose_net_factory: Optional[Callable] = None, pose_mode: str = 'quat',
                 w_avg_samples: int = 10000, w_stats: Optional[Tuple[torch.Tensor, float]] = None,
                 start_w_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, sr_fp16: bool = True, gen_mesh: bool = False,
                 mesh_dir: Optional[str] = None, mesh_res: int = 512, mesh_level: float = 10.0, mesh_format: str = '.mrc', mesh_colors: bool = False,
                 mesh_keep: Optional[int] = None, mesh_min_voxels: int = 0, mesh_simplify: Optional[float] = None, mesh_smooth: int = 0,
                 mesh_texture_tile: int = 8, mesh_preview: bool = False, png_encoder: str = 'host',
                 do_evaluation: bool = False, eval_dir: Optional[str] = None, lpips_eval_net: Optional[Callable] = None,
                 id_net: Optional[Callable] = None, save_pivot: bool = False, pivot_dir: Optional[str] = None, shape_views: bool = False,
                 on_tuned: Optional[Callable[[str, torch.Tensor], None]] = None, on_tuned_depth: bool = False,
                 save_grid: bool = False, gen_video: bool = False, media_dir: Optional[str] = None, video_quality: int = 90):
        """Hyper-parameter names and defaults follow configs/hyperparameters.py.  `early_stop_interval` = how often Phase B reads the
        early-stop state back to the host (1 = every step like the reference).  With the library's Adam the TEST itself runs on the device
        in every step whatever the interval (PivotalTuner.device_stop): the interval then only bounds how many masked no-op steps are
        issued after the stop, not when tuning stops.  Phase A starts where the reference starts (w_projector.py:88-97,100,118): at the mean latent
        of `w_avg_samples` mapped z (plus `start_w_fn(target_255_256)`, the e4e encoder's offset, when given) with the latent-noise scale
        tied to their standard deviation; `w_stats=(w_avg, w_std)` overrides the estimate, `w_avg_samples=0` starts at w = 0, std 1.
        `gen_mesh` (global_config.gen_mesh): after Phase B write the tuned generator's shape at the pivot latent to
        {mesh_dir}/{name}_pti{mesh_format} like create_geometry(shape_res=mesh_res, shape_format=mesh_format): '.mrc' = the raw density grid,
        '.ply' = its marching-cubes mesh at `mesh_level` (the reference's level 10).  `mesh_colors` (no reference counterpart; '.ply', and implied by '.obj'):
        the PLY also carries per-vertex normals and colours (inference.color_mesh with the pivot camera first among the bake views: the view
        the photograph constrains); x y z and the faces are those of the plain file.  `mesh_keep` / `mesh_min_voxels` (no reference
        counterpart): floater removal, inference.clean_grid(keep=, min_voxels=) on the density grid before it is meshed, coloured or written
        ('.mrc' then holds the cleaned grid), and on the grid behind `shape_views`; the defaults leave every file as it was.
        `mesh_simplify` (a cell size in voxels) / `mesh_smooth` (Taubin iterations; no reference counterpart; '.ply' and '.obj'): the mesh goes
        through inference.simplify_mesh, then inference.smooth_mesh, before it is written; with `mesh_colors` the normals and colours are
        those of the final vertices.  None and 0, the defaults, run neither.
        mesh_format='.obj' (no reference counterpart): {name}_pti.obj, {name}_pti.mtl and {name}_pti.png -- the mesh with normals and a
        texture atlas baked from the same views (inference.texture_mesh with `mesh_texture_tile` texels per block side, then
        inference.write_obj); mesh_colors is implied, and mesh_keep / mesh_min_voxels / mesh_simplify / mesh_smooth compose as for '.ply'.
        `mesh_preview` (no reference counterpart; '.obj' only: it shows the texture): beside the mesh, {name}_pti_preview.png -- the generator's
        images from the bake views above the textured mesh from the same cameras (inference.mesh_preview_grid) -- and {name}_pti_fidelity.json,
        inference.mesh_fidelity's dict.  Off by default: a run then writes what it wrote before.
        `do_evaluation` (global_config.do_evaluation): after Phase B render G.synthesis(w_pivot[:, :14], cam[:, :25]) with the tuned generator and
        write metrics.reconstruction_metrics to {eval_dir}/{name}metrics.txt; `lpips_eval_net` (LPIPSAlex) and `id_net` (IDLoss) are built
        once per coach when None.  `save_pivot` writes {pivot_dir}/{name}_ws.npy and {name}_cam.npy; in the reference it only takes effect
        under do_evaluation, here it is independent of it (like gen_mesh).
        `save_grid`: video.pivot_grid (target, the render at the pivot camera, three look_at views; noise_mode='const') as
        {media_dir}/pivot/{name}.png before Phase B and {media_dir}/{name}.png after it.  `gen_video` (global_config.gen_video):
        video.write_orbit_video (240 frames, 60 fps, JPEG quality `video_quality`) as {media_dir}/pivot/{name}_pivot.avi and {media_dir}/{name}.avi.
        `shape_views` (no reference counterpart): both get shaded views of the density surface beside the renders (shape=True of
        video.pivot_grid: a second row; of video.write_orbit_video: image | shape, twice the width).
        `on_tuned` (no reference counterpart): called as on_tuned(name, image) after Phase B with the tuned reconstruction, fp32 [1,3,H,W] --
        what tools/run_inversion.py --paste-back blends into the photograph (images.paste_back).  `on_tuned_depth`: the call is
        on_tuned(name, image, image_depth) with the same render's raw depth [1,1,h,w] -- what images.head_matte(depth=...) takes.
        `png_encoder` 'host' | 'gpu': video.write_png's encoder for every PNG the coach writes (the grids, the mesh preview, the OBJ's atlas);
        'gpu' filters and deflates on the device (hipops.png_encode).  The default writes the files it wrote before."""
        self.on_tuned, self.on_tuned_depth = on_tuned, bool(on_tuned_depth)
        if png_encoder not in ('host', 'gpu'):
            raise ValueError(f"png_encoder 'host' or 'gpu', got {png_encoder!r}")
        self.png_encoder = png_encoder
        if (save_grid or gen_video) and not media_dir:
            raise ValueError('save_grid / gen_video need a media_dir')
        self.save_grid, self.gen_video, self.media_dir, self.video_quality = save_grid, gen_video, media_dir, int(video_quality)
        self.shape_views = bool(shape_views)
        if do_evaluation and not eval_dir:
            raise ValueError('do_evaluation needs an eval_dir')
        if save_pivot and not pivot_dir:
            raise ValueError('save_pivot needs a pivot_dir')
        if mesh_format not in ('.mrc', '.ply', '.obj'):
            raise ValueError(f"mesh_format must be '.mrc', '.ply' or '.obj', got {mesh_format!r}")
        if gen_mesh and not mesh_dir:
            raise ValueError('gen_mesh needs a mesh_dir')
        if mesh_colors and mesh_format == '.mrc':
            raise ValueError("mesh_colors needs mesh_format='.ply' or '.obj': an '.mrc' file is the density grid")
        self.mesh_colors = bool(mesh_colors) or mesh_format == '.obj'
        if not 4 <= int(mesh_texture_tile) <= 64:
            raise ValueError(f'mesh_texture_tile must lie in [4, 64], got {mesh_texture_tile!r}')
        if int(mesh_texture_tile) != 8 and mesh_format != '.obj':
            raise ValueError("mesh_texture_tile needs mesh_format='.obj': only an '.obj' file carries a texture")
        self.mesh_texture_tile = int(mesh_texture_tile)
        if mesh_preview and not (gen_mesh and mesh_format == '.obj'):
            raise ValueError("mesh_preview needs gen_mesh and mesh_format='.obj': the preview shows the textured mesh")
        self.mesh_preview = bool(mesh_preview)
        if mesh_keep is not None and int(mesh_keep) < 0:
            raise ValueError(f'mesh_keep must be >= 0 or None, got {mesh_keep!r}')
        self.mesh_keep, self.mesh_min_voxels = (None if mesh_keep is None else int(mesh_keep)), int(mesh_min_voxels)
        if mesh_simplify is not None and not (float(mesh_simplify) > 0.0 and math.isfinite(float(mesh_simplify))):
            raise ValueError(f'mesh_simplify must be a positive finite cell size or None, got {mesh_simplify!r}')
        if int(mesh_smooth) < 0:
            raise ValueError(f'mesh_smooth must be >= 0 iterations, got {mesh_smooth!r}')
        if (mesh_simplify is not None or int(mesh_smooth) > 0) and mesh_format == '.mrc':
            raise ValueError("mesh_simplify / mesh_smooth need mesh_format='.ply' or '.obj': an '.mrc' file is the density grid")
        self.mesh_simplify, self.mesh_smooth = (None if mesh_simplify is None else float(mesh_simplify)), int(mesh_smooth)
        self.gen_mesh, self.mesh_dir, self.mesh_res, self.mesh_level, self.mesh_format = gen_mesh, mesh_dir, int(mesh_res), float(mesh_level), mesh_format
        self.do_evaluation, self.eval_dir, self.save_pivot, self.pivot_dir = do_evaluation, eval_dir, save_pivot, pivot_dir
        self.lpips_eval_net, self.id_net = lpips_eval_net, id_net
        if do_evaluation:
            dev = next(G.parameters()).device
            if self.lpips_eval_net is None:
                from .loss_nets import LPIPSAlex
                self.lpips_eval_net = LPIPSAlex('pm1').to(dev)           # lpips.LPIPS(net='alex') (base_coach.py:48)
            if self.id_net is None:
                self.id_net = IDLoss().to(dev)
        self.G = G
        self.first_inv_steps, self.max_pti_steps, self.thr = first_inv_steps, max_pti_steps, lpips_threshold
        self.first_inv_lr, self.pti_lr = first_inv_lr, pti_lr
        self.optimize_pose, self.use_warp, self.wplus = optimize_pose, use_warping_loss, wplus
        self.feature_net, self.interval, self.use_graph, self.keep = feature_net, max(1, early_stop_interval), use_graph, keep_tuned_state
        self.synth_kwargs, self.seed = dict(synth_kwargs or {}), seed
        self.pose_net_factory = pose_net_factory      # () -> a fresh pose estimator per image (the reference deep-copies its encoder, w_projector.py:62)
        self.pose_mode, self.start_w_fn = pose_mode, start_w_fn
        self.sr_fp16 = sr_fp16                        # Phase B runs the SR head like the reference does (PivotalTuner); Phase A is always fp32-equivalent
        if w_stats is not None:
            self.w_avg, self.w_std = w_stats[0], float(w_stats[1])
        elif w_avg_samples > 0:
            self.w_avg, self.w_std = estimate_w_stats(G, num_samples=w_avg_samples)     # once per generator: the weights are restored per image
        else:
            self.w_avg, self.w_std = None, 1.0
        # pristine copy of every parameter and buffer: what "re-loading the generator" means without a pickle on disk
        self._pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}

    def restore_generator(self, only_buffers: bool = False):
        with torch.no_grad():
            bufs = {k for k, _ in self.G.named_buffers()}
            for k, v in self.G.state_dict().items():
                if only_buffers and k not in bufs:
                    continue
                v.copy_(self._pristine[k])
        for b in self.G.buffers():
            b.requires_grad = False
            b.grad = None

    def invert(self, name: str, target: torch.Tensor, cam: Optional[torch.Tensor] = None) -> InversionResult:
        G = self.G
        self.restore_generator()
        # ---- Phase A: latent (+ pose) with frozen weights ----------------------------------------------------------------------
        G.requires_grad_(False)
        start_w = None
        if self.start_w_fn is not None:
            with torch.no_grad():
                t255 = (target + 1) * (255 / 2)
                if t255.shape[2] > 256:
                    t255 = torch.nn.functional.interpolate(t255, size=(256, 256), mode='area')
                start_w = self.start_w_fn(t255)                       # e4e_enc(target_e4e).unsqueeze(1)  (w_projector.py:71-74,100)
        proj = LatentProjector(G, target, num_steps=self.first_inv_steps, cam=cam, optimize_pose=self.optimize_pose,
                               use_warping_loss=self.use_warp, first_inv_lr=self.first_inv_lr, wplus=self.wplus,
                               feature_net=self.feature_net, synth_kwargs=self.synth_kwargs, seed=self.seed,
                               use_graph=self.use_graph, w_avg=self.w_avg, w_std=self.w_std, start_w=start_w, pose_mode=self.pose_mode,
                               pose_net=self.pose_net_factory() if (self.pose_net_factory is not None and self.optimize_pose) else None)
        out = {}
        for _ in range(self.first_inv_steps):
            out = proj.step()
        w = proj.w_opt.detach()
        w_pivot = (w.repeat(1, G.backbone.num_ws, 1) if w.shape[1] == 1 else w).clone()
        cam_pivot = out['cam'].detach().clone() if out else proj.cam.detach().clone()
        self.restore_generator(only_buffers=True)
        with torch.no_grad():
            img = G.synthesis(w_pivot, cam_pivot, noise_mode='const', force_fp32=True, **self.synth_kwargs)['image']
            psnr_pivot = float(psnr_01(img, target))
        grid_pivot, video_pivot = self.write_media(name, w_pivot, cam_pivot, target, pivot=True)
        # ---- Phase B: generator weights around the pivot ------------------------------------------------------------------------
        tuner = PivotalTuner(G, target, w_pivot, cam_pivot, lr=self.pti_lr, lpips_threshold=self.thr, feature_net=self.feature_net,
                             synth_kwargs=self.synth_kwargs, sr_fp16=self.sr_fp16, use_graph=self.use_graph)
        steps_b = 0
        if tuner.hip_adam and tuner.device_stop:
            # the criterion is evaluated ON THE DEVICE in every step (a sticky flag that masks the update from the step at which it is met:
            # the reference's every-step `break` before the update, single_id_coach.py:68-71) -- every step can be a graph replay, and the
            # host only polls the flag (every `early_stop_interval` steps) to stop issuing work.  The number of updates made is the
            # optimiser's own device-side step count.
            for i in range(self.max_pti_steps):
                tuner.step()
                if (i % self.interval) == self.interval - 1 and tuner.stopped():
                    break
            steps_b = int(round(float(tuner.optimizer.step_t.item())))
        else:
            for i in range(self.max_pti_steps):
                check = (i % self.interval) == self.interval - 1
                res = tuner.step(early_stop=check)
                if check and res.get('done'):         # the reference leaves before the update (single_id_coach.py:68-71)
                    break
                steps_b += 1
        # how the two phases were actually issued (a refused capture falls back to eager launches with a warning: callers that quote timings check this)
        self.last_launch_modes = dict(phase_a='graph' if getattr(proj, '_graph', None) is not None else 'eager',
                                      phase_b='graph' if getattr(tuner, '_graph', None) is not None else 'eager')
        with torch.no_grad():
            tuned = G.synthesis(w_pivot, cam_pivot, noise_mode='const', force_fp32=True, **self.synth_kwargs)
            img = tuned['image']
            psnr_tuned = float(psnr_01(img, target))
            mse = float(((img.clamp(-1, 1) - target) ** 2).mean() / 4.0)
            if self.on_tuned is not None:
                self.on_tuned(name, img, tuned['image_depth']) if self.on_tuned_depth else self.on_tuned(name, img)
        state = {k: v.detach().clone() for k, v in G.state_dict().items()} if self.keep else None
        G.requires_grad_(False)
        mesh_path = self.write_mesh(name, w_pivot, cam_pivot) if self.gen_mesh else None
        metrics = self.evaluate(name, w_pivot, cam_pivot, target) if self.do_evaluation else None
        grid_tuned, video_tuned = self.write_media(name, w_pivot, cam_pivot, target, pivot=False)
        if self.save_pivot:
            os.makedirs(self.pivot_dir, exist_ok=True)
            np.save(os.path.join(self.pivot_dir, f'{name}_cam.npy'), cam_pivot.detach().cpu().numpy())
            np.save(os.path.join(self.pivot_dir, f'{name}_ws.npy'), w_pivot.detach().cpu().numpy())
        res = InversionResult(name, w_pivot, cam_pivot, psnr_pivot, psnr_tuned, mse, self.first_inv_steps, steps_b, state, mesh_path, metrics)
        res.grid_paths = (grid_pivot, grid_tuned) if self.save_grid else None
        res.video_paths = (video_pivot, video_tuned) if self.gen_video else None
        return res

    def evaluate(self, name: str, w_pivot: torch.Tensor, cam: torch.Tensor, target: torch.Tensor) -> Dict[str, float]:
        """single_id_coach.py:87-106 with the generator as it is now (the tuned one): the metrics, written to {eval_dir}/{name}metrics.txt."""
        with torch.no_grad():
            img = self.G.synthesis(w_pivot[:, :14], cam[:, :25], noise_mode='const', force_fp32=True, **self.synth_kwargs)['image']
        m = reconstruction_metrics(img, target, self.lpips_eval_net, self.id_net)
        os.makedirs(self.eval_dir, exist_ok=True)
        with open(os.path.join(self.eval_dir, f'{name}metrics.txt'), 'w') as f:
            f.write(format_metrics_txt(m))
        return m

    def write_media(self, name: str, w_pivot: torch.Tensor, cam: torch.Tensor, target: torch.Tensor, pivot: bool):
        """(grid path | None, video path | None) of the generator as it is now: single_id_coach.py:57-62 (pivot=True: before Phase B, into
        {media_dir}/pivot/, the video named {name}_pivot) and :80-85 (after Phase B, into {media_dir}/)."""
        if not (self.save_grid or self.gen_video):
            return None, None
        d = os.path.join(self.media_dir, 'pivot') if pivot else self.media_dir
        os.makedirs(d, exist_ok=True)
        grid_path = video_path = None
        if self.save_grid:
            grid_path = os.path.join(d, f'{name}.png')
            write_png(grid_path, pivot_grid(self.G, w_pivot, cam, target, shape=self.shape_views, shape_kwargs=self._clean_kwargs() or None,
                                            **self.synth_kwargs), encoder=self.png_encoder)
        if self.gen_video:
            video_path = os.path.join(d, f'{name}_pivot.avi' if pivot else f'{name}.avi')
            write_orbit_video(self.G, w_pivot, video_path, quality=self.video_quality, shape=self.shape_views,
                              shape_kwargs=self._clean_kwargs() or None, **self.synth_kwargs)
        return grid_path, video_path

    def _clean_kwargs(self) -> dict:
        """keep / min_voxels for inference.clean_grid and its callers; empty with the defaults, so that nothing is labelled."""
        if self.mesh_keep is None and self.mesh_min_voxels <= 0:
            return {}
        return dict(keep=self.mesh_keep, min_voxels=self.mesh_min_voxels)

    def write_mesh(self, name: str, w_pivot: torch.Tensor, cam: Optional[torch.Tensor] = None) -> str:
        """create_geometry(G, w_pivot, outdir=mesh_dir, fname=name + '_pti') with the generator as it is now (the tuned one); with
        mesh_colors the PLY carries normals and colours baked from `cam` (the pivot camera) and inference.bake_cameras(); '.obj' writes the
        OBJ (the path returned), its MTL and its PNG atlas baked from the same views."""
        os.makedirs(self.mesh_dir, exist_ok=True)
        path = os.path.join(self.mesh_dir, f'{name}_pti{self.mesh_format}')
        clean = self._clean_kwargs()
        if self.mesh_format in ('.ply', '.obj'):
            if self.mesh_colors:
                from .hipops import marching_cubes
                grid = density_grid(self.G, w_pivot, res=self.mesh_res)                  # extract_mesh's two steps, keeping the grid for the bake
                if clean:
                    grid = clean_grid(grid, self.mesh_level, **clean)[0]
                verts, faces = marching_cubes(grid, self.mesh_level)
                if self.mesh_simplify is not None:
                    verts, faces, _ = simplify_mesh(verts, faces, self.mesh_simplify)
                if self.mesh_smooth > 0:
                    verts = smooth_mesh(verts, faces, iterations=self.mesh_smooth)
                if self.mesh_format == '.obj':
                    att = texture_mesh(self.G, w_pivot, verts, faces, self.mesh_res, level=self.mesh_level, grid=grid, cameras=self.mesh_cameras(cam),
                                       tile=self.mesh_texture_tile, **self.synth_kwargs)
                    write_obj(path, verts, faces, att['uv'], att['texture'], normals=att['normals'], png_encoder=self.png_encoder)
                    if self.mesh_preview:
                        self.write_mesh_preview(path, w_pivot, verts, faces, att, grid)
                    return path
                att = color_mesh(self.G, w_pivot, verts, self.mesh_res, level=self.mesh_level, grid=grid, cameras=self.mesh_cameras(cam),
                                 **self.synth_kwargs)
                write_ply(path, verts, faces, normals=att['normals'], colors=att['colors'])
            else:
                verts, faces = extract_mesh(self.G, w_pivot, res=self.mesh_res, level=self.mesh_level, simplify=self.mesh_simplify,
                                            smooth=self.mesh_smooth, **clean)
                write_ply(path, verts, faces)
        else:
            grid = density_grid(self.G, w_pivot, res=self.mesh_res)
            write_mrc(path, clean_grid(grid, self.mesh_level, **clean)[0] if clean else grid)
        return path

    def write_mesh_preview(self, path: str, w_pivot: torch.Tensor, verts, faces, att: dict, grid: torch.Tensor) -> Tuple[str, str]:
        """The preview grid and the fidelity numbers of the textured mesh just written to `path`: ({stem}_preview.png, {stem}_fidelity.json)."""
        import json
        from .inference import mesh_fidelity, mesh_preview_grid
        stem = os.path.splitext(path)[0]
        png, js = stem + '_preview.png', stem + '_fidelity.json'
        write_png(png, mesh_preview_grid(self.G, w_pivot, verts, faces, att['uv'], att['texture'], self.mesh_res, **self.synth_kwargs),
                  encoder=self.png_encoder)
        fid = mesh_fidelity(self.G, w_pivot, verts, faces, att['uv'], att['texture'], grid=grid, level=self.mesh_level, **self.synth_kwargs)
        with open(js, 'w') as f:
            f.write(json.dumps(fid) + '\n')
        return png, js

    @staticmethod
    def mesh_cameras(cam: Optional[torch.Tensor]) -> torch.Tensor:
        """The bake views of a coloured mesh: the pivot camera (when there is one) in front of inference.bake_cameras()."""
        views = bake_cameras()
        return views if cam is None else torch.cat([cam.detach()[:1, :25].float().cpu(), views])

    def run(self, images: Sequence[Tuple[str, torch.Tensor, Optional[torch.Tensor]]]) -> Tuple[List[InversionResult], Dict[str, float]]:
        """Invert this rank's shard of `images` = [(name, target [1,3,H,W] in [-1,1], cam [1,25] | None), ...] (every rank passes the
        same full list).  Returns (results of this rank, stats summed / maxed over all ranks)."""
        rank, world, local = D.init_from_env()
        if world > 1 and len(images):
            D.pin_to_numa(local, int(os.environ.get('LOCAL_WORLD_SIZE', world)))
            D.warm_up(images[0][1].device)          # the communicator exists before any step is captured
        results = []
        for i in D.shard_images(len(images), rank, world):
            name, target, cam = images[i]
            results.append(self.invert(name, target, cam))
        dev = images[0][1].device if len(images) else torch.device('cpu')
        stats = D.allreduce_stats(dict(psnr=sum(r.psnr_tuned for r in results), mse=sum(r.mse_tuned for r in results),
                                       n_done=float(len(results)), steps=float(sum(r.steps_a + r.steps_b for r in results))), dev)
        if stats['n_done'] > 0:
            stats['mean_psnr'] = stats['psnr'] / stats['n_done']
        if self.do_evaluation:
            keys = ('mse', 'lpips', 'msssim', 'identity')
            sums = torch.tensor([sum(r.metrics[k] for r in results) for k in keys], dtype=torch.float64, device=dev)
            for k, v in zip(keys, D.allreduce_stats_device(sums).tolist()):
                stats[f'eval_{k}'] = v
                if stats['n_done'] > 0:
                    stats[f'mean_eval_{k}'] = v / stats['n_done']
        self.restore_generator()
        return results, stats
