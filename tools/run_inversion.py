"""Invert a directory of photographs (the reference's scripts/run_pti.py: ImagesDataset + SingleIDCoach.train): decode, align on the GPU where
landmarks are given (inv3d_amd/images.py), then InversionCoach.run -- Phase A, Phase B and the per-image outputs that were asked for.

  python tools/run_inversion.py --in-dir photos --out-dir out [--landmarks landmarks.json] [--weights G.safetensors | --synthetic small|full]
                                [--steps-a 400] [--steps-b 400] [--optimize-pose] [--graph] [--save-grid] [--gen-video] [--gen-mesh]
                                [--mesh-format .mrc|.ply] [--mesh-res 512] [--do-evaluation] [--save-pivot] [--paste-back]
                                [--paste-bands N|auto]

Images with an entry in --landmarks (a .json {name: 68 x 2} or an .npz) are aligned to the generator's resolution; the others must have it
already.  --weights: a generator archive (inv3d_amd.weights, tools/convert_eg3d_pickle.py); otherwise a synthetic generator.  Outputs go to
{out-dir}/media (grids, videos), /mesh, /eval, /pivot; a summary line per image and the totals are printed.  --paste-back also writes
{out-dir}/pasted/{name}.png for every image that had landmarks: the tuned reconstruction blended back into the photograph it was aligned
from (images.paste_back); with --paste-matte [--matte-feather F] [--matte-shrink F] through the head's own matte (images.head_matte, from the
depth of the same render), so the photograph's background stays around the head; with --paste-bands N|auto blended through a Laplacian
pyramid of N levels (images.paste_back(bands=...)) instead of the one alpha.  --video PATH [--frames A:B:S] in place of --in-dir: the targets are
the frames of a Motion-JPEG AVI (images.video_targets; names {stem}_{index:06d}), decoded on the GPU --decode-batch frames per call;
--decode-batch N with --in-dir --jpeg-gpu decodes N files per call."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def _generator(a, dev):
    if a.weights:
        from inv3d_amd.weights import load_generator
        return load_generator(a.weights, device=dev)
    from inv3d_amd import synthetic as S
    if a.synthetic == 'small':
        from oracle import eg3d_oracle as O
        G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                             rendering_kwargs=O.small_config().rendering, device=dev)
    else:
        G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=a.seed)
    for p in G.parameters():
        p.requires_grad_(False)
    return G


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--in-dir', default=None, help='a directory of target images (or --video)')
    ap.add_argument('--video', default=None, metavar='PATH', help='a Motion-JPEG AVI whose frames are the targets (images.video_targets)')
    ap.add_argument('--frames', default=None, metavar='A:B:S', help='--video: the frames start:stop:step (default: all)')
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--landmarks', default=None)
    ap.add_argument('--weights', default=None, help='generator archive; default: a synthetic generator')
    ap.add_argument('--synthetic', choices=('full', 'small'), default='full')
    ap.add_argument('--seed', type=int, default=0, help='synthetic generator weights seed')
    ap.add_argument('--output-size', type=int, default=None, help="default: the generator's img_resolution")
    ap.add_argument('--steps-a', type=int, default=400)
    ap.add_argument('--steps-b', type=int, default=400)
    ap.add_argument('--lpips-threshold', type=float, default=0.06)
    ap.add_argument('--w-avg-samples', type=int, default=None, help='default: 10000 with --weights, 0 with a synthetic generator')
    ap.add_argument('--optimize-pose', action='store_true')
    ap.add_argument('--graph', action='store_true', help='capture the steps into HIP graphs')
    ap.add_argument('--save-grid', action='store_true')
    ap.add_argument('--gen-video', action='store_true')
    ap.add_argument('--png-gpu', action='store_true', help='encode the PNGs on the GPU (hipops.png_encode: adaptive filters, run-length deflate)')
    ap.add_argument('--jpeg-gpu', action='store_true', help='decode baseline JPEG inputs on the GPU (hipops.jpeg_decode: the same pixels as PIL; other files take the PIL path)')
    ap.add_argument('--decode-batch', type=int, default=1, metavar='N', help='--jpeg-gpu: decode N files, or --video: N frames, per device call (hipops.jpeg_decode_batch: the same pixels)')
    ap.add_argument('--gen-mesh', action='store_true')
    ap.add_argument('--mesh-format', choices=('.mrc', '.ply'), default='.mrc')
    ap.add_argument('--mesh-res', type=int, default=512)
    ap.add_argument('--do-evaluation', action='store_true')
    ap.add_argument('--save-pivot', action='store_true')
    ap.add_argument('--paste-back', action='store_true', help='write the tuned reconstruction blended into its photograph (needs --landmarks)')
    ap.add_argument('--paste-feather', type=float, default=0.08, help='--paste-back: blend ramp as a fraction of the aligned side')
    ap.add_argument('--paste-matte', action='store_true', help="--paste-back: paste through the head's matte (images.head_matte), not the whole square")
    ap.add_argument('--matte-feather', type=float, default=0.03, help="--paste-matte: the matte edge's ramp as a fraction of the aligned side")
    ap.add_argument('--matte-shrink', type=float, default=0.0, help='--paste-matte: move the matte edge inwards by this fraction of the aligned side')
    ap.add_argument('--paste-bands', default='0', metavar='N|auto', help='--paste-back: multi-band blend of 1..6 levels, or auto (images.paste_bands); 0: one alpha')
    a = ap.parse_args(argv)
    if (a.in_dir is None) == (a.video is None):
        raise SystemExit('one of --in-dir and --video')
    if a.frames is not None and a.video is None:
        raise SystemExit('--frames belongs to --video')
    if a.video is not None and a.paste_back:
        raise SystemExit('--paste-back takes photographs (--in-dir), not --video')
    if a.decode_batch < 1:
        raise SystemExit('--decode-batch >= 1')
    try:
        frames = slice(*[int(t) if t else None for t in a.frames.split(':')]) if a.frames else slice(None)
    except (ValueError, TypeError):
        raise SystemExit(f'--frames: A:B:S, got {a.frames!r}')
    if a.paste_matte and not a.paste_back:
        raise SystemExit('--paste-matte belongs to --paste-back')
    from inv3d_amd import images
    try:
        bands = images.bands_arg(a.paste_bands)
    except ValueError as e:
        raise SystemExit(f'--paste-bands: {e}')
    if bands != 0 and not a.paste_back:
        raise SystemExit('--paste-bands belongs to --paste-back')
    from inv3d_amd.coach import InversionCoach
    dev = torch.device('cuda')
    G = _generator(a, dev)
    size = a.output_size or int(G.img_resolution)
    decoder = 'gpu' if a.jpeg_gpu else 'pil'
    if a.video is not None:                                                # the device decoder unless told otherwise: frames come 16 at a time
        targets = images.video_targets(a.video, a.landmarks, frames, output_size=size, device=dev, batch=a.decode_batch if a.decode_batch > 1 else 16)
    else:
        targets = images.load_targets(a.in_dir, a.landmarks, output_size=size, device=dev, decoder=decoder, decode_batch=a.decode_batch)
    if not targets:
        raise SystemExit(f'no image files in {a.in_dir}' if a.video is None else f'no frames {a.frames} in {a.video}')
    sub = lambda d: os.path.join(a.out_dir, d)
    on_tuned = None
    if a.paste_back:
        if not a.landmarks:
            raise SystemExit('--paste-back needs --landmarks: only an aligned photograph has a place to paste into')
        from inv3d_amd.video import write_png
        lms, paths = images.load_landmarks(a.landmarks), dict(images.image_files(a.in_dir))

        def on_tuned(name, img, depth=None):
            if name not in lms:
                return
            os.makedirs(sub('pasted'), exist_ok=True)
            kw = dict(bands=bands) if bands != 0 else {}
            if a.paste_matte:                                                  # the head's own matte, from the depth of the same render
                kw['mask'] = images.head_matte(G, None, None, size=img.shape[-1], depth=depth, feather=a.matte_feather, shrink=a.matte_shrink)
            pasted = images.paste_back(images.decode_rgb(paths[name], dev, decoder), img.float(), lms[name], feather=a.paste_feather, **kw)
            write_png(os.path.join(sub('pasted'), f'{name}.png'), pasted[0], encoder='gpu' if a.png_gpu else 'host')
    samples = a.w_avg_samples if a.w_avg_samples is not None else (10000 if a.weights else 0)
    coach = InversionCoach(G, first_inv_steps=a.steps_a, max_pti_steps=a.steps_b, lpips_threshold=a.lpips_threshold, optimize_pose=a.optimize_pose,
                           use_graph=a.graph, w_avg_samples=samples, save_grid=a.save_grid, gen_video=a.gen_video,
                           media_dir=sub('media') if (a.save_grid or a.gen_video) else None, gen_mesh=a.gen_mesh,
                           mesh_dir=sub('mesh') if a.gen_mesh else None, mesh_format=a.mesh_format, mesh_res=a.mesh_res,
                           do_evaluation=a.do_evaluation, eval_dir=sub('eval') if a.do_evaluation else None, save_pivot=a.save_pivot,
                           pivot_dir=sub('pivot') if a.save_pivot else None, on_tuned=on_tuned, on_tuned_depth=a.paste_matte,
                           png_encoder='gpu' if a.png_gpu else 'host')
    results, stats = coach.run(targets)
    for r in results:
        print(f'{r.name}: {r.steps_a} + {r.steps_b} steps, PSNR {r.psnr_pivot:.2f} dB at the pivot, {r.psnr_tuned:.2f} dB tuned')
    print(' '.join(f'{k}={v:.6g}' for k, v in sorted(stats.items())))
    return results, stats


if __name__ == '__main__':
    main()
