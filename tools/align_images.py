"""Face alignment from the command line (the reference's utils/align_data.py over utils/alignment.py::align_face) on the GPU kernels of this
package (inv3d_amd/images.py, csrc/imgprep.hip).

  python tools/align_images.py --in-dir photos --landmarks landmarks.json --out-dir aligned [--output-size 512]

Every image file of --in-dir whose name (up to its first dot) is in the landmarks file -- a .json {name: 68 x 2} or an .npz with one array per
name; there is no landmark detector here, the points come from a file as in EG3D's own preprocessing -- is decoded on the host, aligned on the
GPU and written as {out-dir}/{name}.png.  Files without landmarks are reported and skipped."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--in-dir', required=True)
    ap.add_argument('--landmarks', required=True, help='.json {name: 68 x 2} or .npz')
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--output-size', type=int, default=512)
    a = ap.parse_args(argv)
    from inv3d_amd import images, video
    dev = torch.device('cuda')
    lms = images.load_landmarks(a.landmarks)
    os.makedirs(a.out_dir, exist_ok=True)
    written = []
    for name, path in images.image_files(a.in_dir):
        if name not in lms:
            print(f'{path}: no landmarks, skipped')
            continue
        out = os.path.join(a.out_dir, name + '.png')
        video.write_png(out, images.align_face(images.decode_rgb(path, dev), lms[name], a.output_size))
        written.append(out)
        print(out)
    print(f'{len(written)} aligned images of {a.output_size} x {a.output_size} in {a.out_dir}')
    return written


if __name__ == '__main__':
    main()
