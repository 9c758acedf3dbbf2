"""Face alignment from the command line (the reference's utils/align_data.py over utils/alignment.py::align_face) on the GPU kernels of this
package (inv3d_amd/images.py, csrc/imgprep.hip).

  python tools/align_images.py --in-dir photos --landmarks landmarks.json --out-dir aligned [--output-size 512]

Every image file of --in-dir whose name (up to its first dot) is in the landmarks file -- a .json {name: 68 x 2} or an .npz with one array per
name; there is no landmark detector here, the points come from a file as in EG3D's own preprocessing -- is decoded on the host, aligned on the
GPU and written as {out-dir}/{name}.png (--png-gpu: encoded on the GPU as well, eight frames per batch; --jpeg-gpu: baseline JPEG inputs
are decoded on the GPU too, to the same pixels).  Files without landmarks are
reported and skipped."""
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
    ap.add_argument('--png-gpu', action='store_true', help='filter and deflate the PNGs on the GPU, eight frames per encode')
    ap.add_argument('--jpeg-gpu', action='store_true', help='decode baseline JPEG inputs on the GPU (hipops.jpeg_decode: the same pixels as PIL; other files take the PIL path)')
    ap.add_argument('--decode-batch', type=int, default=1, metavar='N', help='--jpeg-gpu: decode N files per device call (hipops.jpeg_decode_batch: the same pixels)')
    a = ap.parse_args(argv)
    if a.decode_batch < 1:
        raise SystemExit('--decode-batch >= 1')
    from inv3d_amd import images
    written = images.write_aligned(a.in_dir, a.landmarks, a.out_dir, a.output_size, device=torch.device('cuda'),
                                   png_encoder='gpu' if a.png_gpu else 'host', report=lambda path: print(f'{path}: no landmarks, skipped'),
                                   decoder='gpu' if a.jpeg_gpu else 'pil', decode_report=lambda path, why: print(f'{path}: decoded by PIL ({why})'), decode_batch=a.decode_batch)
    for out in written:
        print(out)
    print(f'{len(written)} aligned images of {a.output_size} x {a.output_size} in {a.out_dir}')
    return written


if __name__ == '__main__':
    main()
