"""Paste-back from the command line: edited aligned images blended back into the photograph they were aligned from, on the GPU kernels of
this package (inv3d_amd/images.py paste_back, csrc/imgprep.hip).  No reference counterpart: the reference's alignment goes one way only.

  python tools/paste_back.py --photo photo.jpg --landmarks landmarks.json --edit a_inter_1.png a_inter_2.png --out-dir pasted
                             [--feather 0.08] [--mask mask.png [--mask-binary [--matte-feather 0.03] [--matte-shrink 0]]] [--bbox]
                             [--paste-bands N|auto]

--landmarks: a .json {name: 68 x 2} or an .npz with an entry for the photo (its file name up to the first dot) -- the points align_face took.
--edit: square RGB images in the aligned frame (any side); each is written as {out-dir}/{edit name}.png, the whole photograph with the edit in
it, or with --bbox only the face's bounding box in the photo.  --feather: the blend ramp from the frame's edge as a fraction of the side.
--mask: a grey image of the edits' side in the aligned frame, 255 = all of the edit.  --mask-binary: the file is a raw binary mask instead
(nonzero = head, e.g. a segmentation): it goes through images.matte_from_mask first (specks removed, holes closed, the edge feathered).
--paste-bands: 1..6 or auto -- the multi-band blend (images.paste_back(bands=...), csrc/blend.hip) instead of the one alpha; 0, the default,
writes what the tool wrote before the option existed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--photo', required=True)
    ap.add_argument('--landmarks', required=True, help='.json {name: 68 x 2} or .npz')
    ap.add_argument('--edit', required=True, nargs='+', metavar='FILE')
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--feather', type=float, default=0.08)
    ap.add_argument('--png-gpu', action='store_true', help='encode the PNGs on the GPU (hipops.png_encode: adaptive filters, run-length deflate)')
    ap.add_argument('--jpeg-gpu', action='store_true', help='decode baseline JPEG inputs on the GPU (hipops.jpeg_decode: the same pixels as PIL; other files take the PIL path)')
    ap.add_argument('--decode-batch', type=int, default=1, metavar='N', help='--jpeg-gpu: decode N files per device call (hipops.jpeg_decode_batch: the same pixels)')
    ap.add_argument('--mask', default=None)
    ap.add_argument('--mask-binary', action='store_true', help='--mask is a raw binary mask (nonzero = head): clean and feather it first')
    ap.add_argument('--matte-feather', type=float, default=0.03, help="--mask-binary: the matte edge's ramp as a fraction of the side")
    ap.add_argument('--matte-shrink', type=float, default=0.0, help='--mask-binary: move the matte edge inwards by this fraction of the side')
    ap.add_argument('--bbox', action='store_true')
    ap.add_argument('--paste-bands', default='0', metavar='N|auto', help='multi-band blend of 1..6 levels, or auto (images.paste_bands); 0: one alpha')
    a = ap.parse_args(argv)
    if a.decode_batch < 1:
        raise SystemExit('--decode-batch >= 1')
    from inv3d_amd import images, video
    try:
        bands = images.bands_arg(a.paste_bands)
    except ValueError as e:
        raise SystemExit(f'--paste-bands: {e}')
    bkw = dict(bands=bands) if bands != 0 else {}
    dev = torch.device('cuda')
    lms, key = images.load_landmarks(a.landmarks), os.path.basename(a.photo).split('.')[0]
    if key not in lms:
        raise SystemExit(f'{a.landmarks} has no entry for {key}')
    decoder = 'gpu' if a.jpeg_gpu else 'pil'
    photo = images.decode_rgb(a.photo, dev, decoder)
    mask = None
    if a.mask is not None:
        from PIL import Image
        with Image.open(a.mask) as im:
            mask = torch.from_numpy(np.array(im.convert('L'), dtype=np.uint8)).to(dev)
        if a.mask_binary:
            if mask.shape[0] != mask.shape[1]:
                raise SystemExit(f'--mask-binary: a square mask, got {mask.shape[1]} x {mask.shape[0]}')
            mask = images.matte_from_mask(mask, mask.shape[0], feather=a.matte_feather, shrink=a.matte_shrink)
    elif a.mask_binary:
        raise SystemExit('--mask-binary belongs to --mask')
    os.makedirs(a.out_dir, exist_ok=True)
    written = []
    edits = []
    for k in range(0, len(a.edit), a.decode_batch):
        block = a.edit[k:k + a.decode_batch]
        edits += images.decode_rgb_batch(block, dev, decoder) if a.decode_batch > 1 else [images.decode_rgb(p, dev, decoder) for p in block]
    for path, edit in zip(a.edit, edits):
        out = os.path.join(a.out_dir, os.path.basename(path).split('.')[0] + '.png')
        video.write_png(out, images.paste_back(photo, edit, lms[key], feather=a.feather, mask=mask, region='bbox' if a.bbox else 'photo', **bkw),
                        encoder='gpu' if a.png_gpu else 'host')
        written.append(out)
        print(out)
    return written


if __name__ == '__main__':
    main()
