"""GANSpace latent editing from the command line (the reference's ganspace/pca_anlaysis.py and run_ganspace.py) on the GPU kernels of this
package (inv3d_amd/ganspace.py, csrc/pca.hip).

  python tools/run_ganspace.py fit  --out comp.npy [--weights G.safetensors | --synthetic small|full] [--samples 100000] [--components 512]
  python tools/run_ganspace.py edit --components comp.npy --ws a_ws.npy --cam a_cam.npy (--direction smile | --params IDX START NUM POWER)
                                    --out-dir edits --name a [--num-imgs 5] [--save-images] [--weights ... | --synthetic ...]

fit   writes the [K, w_dim] float32 components of a PCA of W at the frontal camera; the reference's ganspace/pca_comp/*.npy load the same way.
edit  takes a pivot as the coach's save_pivot writes it ({name}_ws.npy [1, num_ws, w_dim], {name}_cam.npy [1, 25]) and a named direction of
      ganspace.GANSPACE_DIRECTIONS or its four numbers (component, first layer, layers, power); writes {name}_grid.png and, with --save-images,
      {name}_inter_{i}.png (i from 1) as the reference names them.  With --paste-photo P --landmarks L (no reference counterpart) also
      {name}_pasted.png: every edit blended back into the photograph P (images.paste_back), the face's bounding box of each side by side;
      with --paste-matte [--matte-feather F] [--matte-shrink F] each through its own head matte (images.head_matte, from the edit's depth);
      with --paste-bands N|auto through the multi-band blend (images.paste_back(bands=...)) instead of the one alpha.
--weights: a generator archive (inv3d_amd.weights, tools/convert_eg3d_pickle.py); otherwise a synthetic generator (inv3d_amd.synthetic, weights
seed --seed): 'full' is the full-size one, 'small' the 32-wide one of the tests."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
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


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument('--weights', default=None, help='generator archive; default: a synthetic generator')
    common.add_argument('--synthetic', choices=('full', 'small'), default='full')
    common.add_argument('--seed', type=int, default=0, help='synthetic generator weights seed')
    fit = sub.add_parser('fit', parents=[common])
    fit.add_argument('--out', required=True, help='components .npy')
    fit.add_argument('--samples', type=int, default=100_000)
    fit.add_argument('--components', type=int, default=512)
    fit.add_argument('--chunk', type=int, default=8192)
    fit.add_argument('--z-seed', type=int, default=0)
    ed = sub.add_parser('edit', parents=[common])
    ed.add_argument('--components', required=True)
    ed.add_argument('--ws', required=True)
    ed.add_argument('--cam', required=True)
    which = ed.add_mutually_exclusive_group(required=True)
    which.add_argument('--direction', help='a name of ganspace.GANSPACE_DIRECTIONS')
    which.add_argument('--params', nargs=4, type=float, metavar=('IDX', 'START', 'NUM', 'POWER'))
    ed.add_argument('--num-imgs', type=int, default=5)
    ed.add_argument('--out-dir', required=True)
    ed.add_argument('--name', required=True)
    ed.add_argument('--save-images', action='store_true')
    ed.add_argument('--paste-photo', default=None, help='the photograph the pivot was inverted from: also write {name}_pasted.png')
    ed.add_argument('--landmarks', default=None, help='--paste-photo: a .json / .npz of 68 x 2 landmarks with an entry for the photo (or --name)')
    ed.add_argument('--paste-feather', type=float, default=0.08)
    ed.add_argument('--paste-matte', action='store_true', help="--paste-photo: paste every edit through its head's matte (images.head_matte)")
    ed.add_argument('--paste-bands', default='0', metavar='N|auto', help='--paste-photo: multi-band blend of 1..6 levels, or auto (images.paste_bands); 0: one alpha')
    ed.add_argument('--matte-feather', type=float, default=0.03, help="--paste-matte: the matte edge's ramp as a fraction of the side")
    ed.add_argument('--matte-shrink', type=float, default=0.0, help='--paste-matte: move the matte edge inwards by this fraction of the side')
    return ap


def main(argv=None):
    a = _parser().parse_args(argv)
    from inv3d_amd import ganspace as GS
    dev = torch.device('cuda')
    G = _generator(a, dev)
    if a.cmd == 'fit':
        res = GS.fit_w_pca(G, n_samples=a.samples, n_components=a.components, seed=a.z_seed, chunk=a.chunk)
        GS.save_components(a.out, res)
        print(f'{a.out}: {tuple(res.components.shape)} components of {res.n_samples} latents, {res.sweeps} sweeps, '
              f'leading variance ratios {" ".join(f"{v:.4f}" for v in res.var_ratio[:5].tolist())}')
        return res
    from PIL import Image
    if a.direction is not None:
        if a.direction not in GS.GANSPACE_DIRECTIONS:
            raise SystemExit(f'unknown direction {a.direction!r}; known: {", ".join(GS.GANSPACE_DIRECTIONS)}')
        idx, start, num, power = GS.GANSPACE_DIRECTIONS[a.direction]
    else:
        idx, start, num, power = int(a.params[0]), int(a.params[1]), int(a.params[2]), a.params[3]
    comp = GS.load_components(a.components)
    w = torch.from_numpy(np.load(a.ws)).float().to(dev)
    cam = torch.from_numpy(np.load(a.cam)).float().to(dev)
    if a.paste_matte and a.paste_photo is None:
        raise SystemExit('--paste-matte belongs to --paste-photo')
    out = GS.edit_ganspace(G, comp, w, cam, idx, start_layer=start, layer_num=num, edit_power=power, num_imgs=a.num_imgs,
                           **(dict(with_depth=True) if a.paste_matte else {}))
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, f'{a.name}_grid.png')
    Image.fromarray(out['grid'].cpu().numpy(), 'RGB').save(path)
    if a.save_images:
        for i in range(a.num_imgs):
            Image.fromarray(out['images'][i].cpu().numpy(), 'RGB').save(os.path.join(a.out_dir, f'{a.name}_inter_{i + 1}.png'))
    print(f'{path}: component {idx}, layers {start}..{start + num - 1}, power {power}, {a.num_imgs} images')
    if a.paste_photo is not None:
        from inv3d_amd import images
        from inv3d_amd.video import write_png
        if not a.landmarks:
            raise SystemExit('--paste-photo needs --landmarks')
        lms = images.load_landmarks(a.landmarks)
        key = os.path.basename(a.paste_photo).split('.')[0]
        key = key if key in lms else a.name
        if key not in lms:
            raise SystemExit(f'{a.landmarks} has no entry for {os.path.basename(a.paste_photo)} or {a.name}')
        try:
            bands = images.bands_arg(a.paste_bands)
        except ValueError as e:
            raise SystemExit(f'--paste-bands: {e}')
        kw = dict(bands=bands) if bands != 0 else {}
        if a.paste_matte:                                                      # one matte per edit, from the depth of the edit's own render
            kw['mask'] = images.head_matte(G, None, None, size=out['images'].shape[1], depth=out['depth'], feather=a.matte_feather,
                                           shrink=a.matte_shrink)
        pasted = images.paste_back(images.decode_rgb(a.paste_photo, dev), out['images'], lms[key], feather=a.paste_feather, region='bbox', **kw)
        out['pasted'] = pasted                                                 # [num_imgs, h, w, 3]: the face's bounding box in the photo, per edit
        ppath = os.path.join(a.out_dir, f'{a.name}_pasted.png')
        write_png(ppath, torch.cat(list(pasted), dim=1))
        print(f'{ppath}: {a.num_imgs} edits in the photo, {pasted.shape[2]} x {pasted.shape[1]} each')
    return out


if __name__ == '__main__':
    main()
