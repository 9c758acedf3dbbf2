"""Image ingestion on the GPU: one 1024^2 photograph -> the 512^2 fp32 target (images.align_face + hipops.u8_to_target: crop, the feathered
reflect pad when the face touches the frame, the QUAD warp, uint8 -> [-1, 1]) against the same chain on the host (Pillow crop / transform,
scipy.ndimage.gaussian_filter + np.median for the pad, numpy for the conversion).  The photograph is already decoded and, for the GPU, already
on the device: decoding is host work either way.  Device events around each timed window, after warm-up; median of 5 windows.

    python tools/time_align.py
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pil_ref as R  # noqa: E402
from make_golden_align import landmarks, photo  # noqa: E402
from inv3d_amd import hipops as H, images  # noqa: E402

dev = torch.device('cuda')
SIZE = 512


def host_chain(img, lm):
    from PIL import Image
    plan = images.align_plan(img.shape[0], img.shape[1], lm, SIZE)
    im = Image.fromarray(img)
    if plan.shrink_size is not None:
        im = im.resize(plan.shrink_size, Image.LANCZOS)
    if plan.crop is not None:
        im = im.crop(plan.crop)
    if plan.pad is not None:
        im = Image.fromarray(R.scipy_pad(np.asarray(im), plan.pad, plan.qsize), 'RGB')
    im = im.transform((SIZE, SIZE), Image.QUAD, plan.quad, Image.BILINEAR)
    return (np.asarray(im).transpose(2, 0, 1)[None].astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5), plan


def gpu_chain(img_d, lm):
    return H.u8_to_target(images.align_face(img_d, lm, SIZE))


def timed_gpu_ms(f, reps=10, windows=5):
    for _ in range(3):
        f()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            f()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def timed_host_ms(f, reps=3, windows=5):
    f()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


# eye centres and mouth centre in a 1024^2 frame: a face well inside it, and one at the left edge (the pad branch)
for name, el, er, mo in (('face inside the frame', (430, 470), (600, 476), (512, 650)), ('face at the frame edge', (60, 470), (230, 480), (140, 655))):
    img = photo(1024, 1024, 1)
    lm = landmarks(el, er, mo, 2)
    img_d = torch.from_numpy(img).to(dev)
    want, plan = host_chain(img, lm)
    got = gpu_chain(img_d, lm).cpu().numpy()
    diff = np.abs(np.rint(got * 127.5).astype(np.int64) - np.rint(want * 127.5).astype(np.int64))
    steps = ' + '.join(s for s, on in (('shrink', plan.shrink_size), ('crop', plan.crop), (f'pad {plan.pad}', plan.pad), ('warp', True), ('to target', True)) if on)
    print(f'{name}: {steps}; GPU vs host target: max {int(diff.max())} levels, {float((diff.max(1) > 0).mean()):.3g} of the pixels differ', flush=True)
    g = timed_gpu_ms(lambda: gpu_chain(img_d, lm))
    h = timed_host_ms(lambda: host_chain(img, lm))
    print(f'  GPU (HIP kernels, device events) {g[0]:8.3f} ms  (min {g[1]:.3f}, max {g[2]:.3f})', flush=True)
    print(f'  host (Pillow / scipy / numpy)    {h[0]:8.3f} ms  (min {h[1]:.3f}, max {h[2]:.3f})   ratio {h[0] / g[0]:.1f}x', flush=True)
