"""Paste-back on the GPU: 16 edited 512^2 frames blended into one 3000 x 4000 photograph whose face square is about 1500 px
(hipops.paste_back, csrc/imgprep.hip) -- the face's bounding box alone (whole=False, one launch) and the whole photograph per frame
(whole=True: the photo into every frame, then the region) -- against a torch composite of the same result: F.affine_grid / F.grid_sample
(bilinear, border padding) of the frames over the bounding box, the smoothstep feather, the blend, rounding, and for the whole form the copy
into 16 photographs.  torch works in fp32, the kernel in fp64: the two may differ by a level where a value lands next to a half.  Device
events around each timed window, after warm-up; median of 5 windows.

    python tools/time_paste_back.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from inv3d_amd import hipops as H, images  # noqa: E402

dev = torch.device('cuda')
HP, WP, S, N, FEATHER = 3000, 4000, 512, 16, 0.08


def landmarks():
    """Eyes 375 px apart, slightly tilted: a face square of about 1500 px in the middle of the photograph."""
    lm = np.zeros((68, 2))
    eye_avg, e2e, e2m = np.array([2000.5, 1350.5]), np.array([373.0, 40.0]), np.array([-45.0, 400.0])
    lm[36:42], lm[42:48] = eye_avg - e2e / 2, eye_avg + e2e / 2
    lm[48] = lm[54] = eye_avg + e2m
    return lm


def torch_composite(photo_f, frames_f, plan, whole, photo_u8):
    """photo_f fp32 [1,3,Hp,Wp], frames_f fp32 [N,3,S,S] (the uint8 values): the same composite with torch operators."""
    x0, y0, x1, y1 = plan.region
    m = plan.matrix
    ys, xs = torch.meshgrid(torch.arange(y0, y1, device=dev, dtype=torch.float32) + 0.5, torch.arange(x0, x1, device=dev, dtype=torch.float32) + 0.5,
                            indexing='ij')
    u, v = m[0] + m[1] * xs + m[2] * ys, m[3] + m[4] * xs + m[5] * ys
    grid = torch.stack([u * (2.0 / S) - 1.0, v * (2.0 / S) - 1.0], -1)[None].expand(N, -1, -1, -1)
    val = F.grid_sample(frames_f, grid, mode='bilinear', padding_mode='border', align_corners=False)
    inside = (u >= 0) & (u < S) & (v >= 0) & (v < S)
    f = (torch.minimum(torch.minimum(u, S - u), torch.minimum(v, S - v)) * (1.0 / (FEATHER * S))).clamp(0.0, 1.0)
    a = torch.where(inside, f * f * (3.0 - 2.0 * f), torch.zeros_like(f))
    ph = photo_f[:, :, y0:y1, x0:x1]
    out = torch.round(ph + (val - ph) * a).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    if not whole:
        return out.contiguous()
    full = photo_u8[None].repeat(N, 1, 1, 1)
    full[:, y0:y1, x0:x1] = out
    return full


def timed_gpu_ms(f, reps=5, windows=5):
    for _ in range(2):
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


rs = np.random.RandomState(0)
yy, xx = np.mgrid[:HP, :WP]
photo = torch.from_numpy(np.clip(np.stack([128 + 80 * np.sin(xx / 170 + yy / 230), 100 + 60 * np.cos(xx / 110), 40 + yy / 16], -1) +
                                 rs.normal(0, 10, (HP, WP, 3)), 0, 255).astype(np.uint8)).to(dev)
frames = torch.from_numpy(rs.randint(0, 256, (N, S, S, 3), dtype=np.uint8)).to(dev)
plan = images.paste_plan(HP, WP, landmarks(), S)
x0, y0, x1, y1 = plan.region
print(f'photo {WP} x {HP}, {N} frames of {S}^2, scale {plan.scale:.4f} aligned px per photo px, region {x1 - x0} x {y1 - y0}', flush=True)
photo_f, frames_f = photo.permute(2, 0, 1)[None].float(), frames.permute(0, 3, 1, 2).float().contiguous()
for whole in (False, True):
    hip = lambda: H.paste_back(photo, frames, plan.matrix, plan.region, FEATHER * S, whole=whole)
    ref = lambda: torch_composite(photo_f, frames_f, plan, whole, photo)
    d = (hip().to(torch.int16) - ref().to(torch.int16)).abs()
    print(f"{'whole photograph per frame' if whole else 'bounding box alone'}: HIP vs torch max {int(d.max())} levels, "
          f'{float((d > 0).float().mean()):.3g} of the bytes differ', flush=True)
    del d
    g = timed_gpu_ms(hip)
    t = timed_gpu_ms(ref)
    print(f'  HIP kernel(s)            {g[0]:8.3f} ms  (min {g[1]:.3f}, max {g[2]:.3f})', flush=True)
    print(f'  torch grid_sample blend  {t[0]:8.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})   ratio {t[0] / g[0]:.2f}x', flush=True)
