"""Orbit video from the command line: a pivot latent in, a Motion-JPEG AVI out (gen_interp_video, gen_videos.py:74-146, as
single_id_coach.py:61-62,84-85 calls it), frames encoded by the GPU JPEG encoder of this package (inv3d_amd/video.py, csrc/jpeg.hip).

  python tools/render_video.py --ws pivot_ws.npy --out orbit.avi [--weights G.safetensors] [--depth] [--frames 240] [--fps 60] [--quality 90]

--weights: a generator archive (inv3d_amd.weights, tools/convert_eg3d_pickle.py); without it, the full-size synthetic generator
(inv3d_amd.synthetic, seed --seed).  --ws: a [1, num_ws, w_dim] (or [num_ws, w_dim]) .npy latent, e.g. the coach's {image}_ws.npy.
--depth renders image_depth (grey frames) instead of the colour image.  --shape puts the shaded first-hit view of the density surface
(--shape-level, --shape-grid, --shape-shade lambert | normal) beside every frame: twice the width, one density grid per video.
With --shape, --keep N / --min-voxels M / --connectivity {6,26} remove floaters from that grid first (inference.clean_grid, once per video).
--paste-photo P --landmarks L blends every frame back into the photograph P the latent was inverted from (images.paste_back): the video
shows the face's bounding box in the photo, with --paste-whole the whole photograph.  --paste-matte [--matte-feather F] [--matte-shrink F]
pastes every frame through its own head matte (images.head_matte, from the depth of the frame's render): the photograph's background stays
around the head.  --paste-bands N|auto: the multi-band blend of images.paste_back(bands=...) instead of the one alpha (with the matte too).
--synthetic small: the 32-wide synthetic generator of the tests instead of the full-size one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--ws', required=True, help='latent .npy, [1, num_ws, w_dim] or [num_ws, w_dim]')
    ap.add_argument('--out', required=True, help='output .avi')
    ap.add_argument('--weights', default=None, help='generator archive; default: the synthetic full-size generator')
    ap.add_argument('--seed', type=int, default=0, help='synthetic generator weights seed')
    ap.add_argument('--depth', action='store_true', help="render image_depth instead of image")
    ap.add_argument('--frames', type=int, default=240)
    ap.add_argument('--fps', type=int, default=60)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--batch', type=int, default=16, help='frames per encoder call')
    ap.add_argument('--shape', action='store_true', help='image | shaded density surface side by side (twice the width)')
    ap.add_argument('--shape-level', type=float, default=10.0, help='density level of the surface')
    ap.add_argument('--shape-grid', type=int, default=512, help='side of the density grid')
    ap.add_argument('--shape-shade', default='lambert', choices=['lambert', 'normal'])
    ap.add_argument('--keep', type=int, default=None, help='--shape: keep only the N largest connected components above the level')
    ap.add_argument('--min-voxels', type=int, default=0, help='--shape: drop connected components of fewer voxels')
    ap.add_argument('--connectivity', type=int, default=6, choices=(6, 26))
    ap.add_argument('--paste-photo', default=None, help='the photograph the latent was inverted from: every frame is blended back into it')
    ap.add_argument('--landmarks', default=None, help='--paste-photo: a .json / .npz of 68 x 2 landmarks with an entry for the photo')
    ap.add_argument('--paste-whole', action='store_true', help="--paste-photo: the whole photograph per frame, not the face's bounding box")
    ap.add_argument('--paste-matte', action='store_true', help="--paste-photo: paste every frame through its head's matte (images.head_matte)")
    ap.add_argument('--matte-feather', type=float, default=0.03, help="--paste-matte: the matte edge's ramp as a fraction of the side")
    ap.add_argument('--matte-shrink', type=float, default=0.0, help='--paste-matte: move the matte edge inwards by this fraction of the side')
    ap.add_argument('--paste-bands', default='0', metavar='N|auto', help='--paste-photo: multi-band blend of 1..6 levels, or auto (images.paste_bands); 0: one alpha')
    ap.add_argument('--synthetic', choices=('full', 'small'), default='full', help='without --weights: which synthetic generator')
    a = ap.parse_args(argv)
    if a.paste_matte and a.paste_photo is None:
        raise SystemExit('--paste-matte belongs to --paste-photo')
    if a.paste_bands != '0' and a.paste_photo is None:
        raise SystemExit('--paste-bands belongs to --paste-photo')
    from inv3d_amd import video as V
    dev = torch.device('cuda')
    if a.weights:
        from inv3d_amd.weights import load_generator
        G = load_generator(a.weights, device=dev)
    else:
        from inv3d_amd import synthetic as S
        if a.synthetic == 'small':
            from oracle import eg3d_oracle as O
            G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                                 rendering_kwargs=O.small_config().rendering, device=dev)
        else:
            G = S.make_generator(device=dev)
        S.load_synthetic_weights(G, seed=a.seed)
    ws = torch.from_numpy(np.load(a.ws)).float().to(dev)
    if ws.dim() == 2:
        ws = ws.unsqueeze(0)
    clean = dict(keep=a.keep, min_voxels=a.min_voxels, connectivity=a.connectivity) if (a.keep is not None or a.min_voxels > 0) else {}
    paste = None
    if a.paste_photo is not None:
        from inv3d_amd import images
        if not a.landmarks:
            raise SystemExit('--paste-photo needs --landmarks')
        lms, key = images.load_landmarks(a.landmarks), os.path.basename(a.paste_photo).split('.')[0]
        if key not in lms:
            raise SystemExit(f'{a.landmarks} has no entry for {key}')
        paste = (images.decode_rgb(a.paste_photo, dev), lms[key])
    pkw = dict(region='photo') if a.paste_whole else {}
    if a.paste_matte:
        pkw['matte'] = dict(feather=a.matte_feather, shrink=a.matte_shrink)
    if a.paste_bands != '0':
        try:
            pkw['bands'] = images.bands_arg(a.paste_bands)
        except ValueError as e:
            raise SystemExit(f'--paste-bands: {e}')
    t0 = time.perf_counter()
    n = V.write_orbit_video(G, ws, a.out, num_frames=a.frames, image_mode='image_depth' if a.depth else 'image', fps=a.fps, quality=a.quality,
                            batch=a.batch, shape=a.shape, shape_kwargs=dict(level=a.shape_level, grid_res=a.shape_grid, shade=a.shape_shade, **clean),
                            paste=paste, paste_kwargs=pkw or None)
    dt = time.perf_counter() - t0
    print(f'{a.out}: {n} frames, {os.path.getsize(a.out)} bytes ({dt * 1e3:.1f} ms, {n / dt:.1f} frames/s)')
    return n


if __name__ == '__main__':
    main()
