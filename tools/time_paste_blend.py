"""Multi-band paste-back on the GPU (hipops.paste_blend, csrc/blend.hip) on tools/time_paste_back.py's case: 16 edited 512^2 frames blended
into one 3000 x 4000 photograph whose face square is about 1500 px, feather 0.08 -- bands 1..5, the bounding box alone (whole=False) and the
whole photograph per frame (whole=True) -- against
  (a) the one-alpha paste (hipops.paste_back) on the same inputs: what the feature costs;
  (b) a torch composite of the same pyramid in fp32: the level-0 planes from F.grid_sample over the window, F.conv2d stride 2 with the 5 x 5
      kernel for the reduce, F.conv_transpose2d for the expand; how many bytes differ from the kernels is reported (torch's level 0 is fp32
      and its convolutions sum in their own order).
The time is also given as bytes per window pixel and frame at the bandwidth a plain device copy reaches in the same run, next to the bytes
model of the fused design (level 0 never stored: about 18 B).  Device events around each timed window, after warm-up; median of 5 windows.

    python tools/time_paste_blend.py [--bands 1 2 3 4 5] [--no-torch]
"""
import argparse
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
    """Eyes 375 px apart, slightly tilted: a face square of about 1500 px in the middle of the photograph (time_paste_back.py's)."""
    lm = np.zeros((68, 2))
    eye_avg, e2e, e2m = np.array([2000.5, 1350.5]), np.array([373.0, 40.0]), np.array([-45.0, 400.0])
    lm[36:42], lm[42:48] = eye_avg - e2e / 2, eye_avg + e2e / 2
    lm[48] = lm[54] = eye_avg + e2m
    return lm


K1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0])


def torch_blend(photo_f, frames_f, plan, bands, whole, photo_u8):
    """photo_f fp32 [1,3,Hp,Wp], frames_f fp32 [N,3,S,S] (the uint8 values): the same pyramid with torch operators."""
    wx0, wy0, wx1, wy1 = H.paste_blend_window(plan.region, bands, HP, WP)
    m = plan.matrix
    ys, xs = torch.meshgrid(torch.arange(wy0, wy1, device=dev, dtype=torch.float32) + 0.5,
                            torch.arange(wx0, wx1, device=dev, dtype=torch.float32) + 0.5, indexing='ij')
    u, v = m[0] + m[1] * xs + m[2] * ys, m[3] + m[4] * xs + m[5] * ys
    grid = torch.stack([u * (2.0 / S) - 1.0, v * (2.0 / S) - 1.0], -1)[None].expand(N, -1, -1, -1)
    val = F.grid_sample(frames_f, grid, mode='bilinear', padding_mode='border', align_corners=False)
    inside = (u >= 0) & (u < S) & (v >= 0) & (v < S)
    f = (torch.minimum(torch.minimum(u, S - u), torch.minimum(v, S - v)) * (1.0 / (FEATHER * S))).clamp(0.0, 1.0)
    a = torch.where(inside, f * f * (3.0 - 2.0 * f), torch.zeros_like(f))
    ph = photo_f[:, :, wy0:wy1, wx0:wx1]
    da = torch.cat([(val - ph) * inside, a[None, None].expand(N, -1, -1, -1)], 1)            # [N,4,h,w]: D and alpha
    k2 = (K1[:, None] * K1[None, :]).to(dev)
    kr, ke = (k2 / 256.0)[None, None].repeat(4, 1, 1, 1), (k2 / 64.0)[None, None].repeat(3, 1, 1, 1)
    lv = [da]
    for _ in range(bands):
        lv.append(F.conv2d(lv[-1], kr, stride=2, padding=2, groups=4))

    def expand(x, like):
        h, w = like.shape[-2:]
        return F.conv_transpose2d(x, ke, stride=2, padding=2, output_padding=(h - 2 * x.shape[-2] + 1, w - 2 * x.shape[-1] + 1), groups=3)
    r = lv[bands][:, :3] * lv[bands][:, 3:]
    for k in range(bands - 1, -1, -1):
        r = (lv[k][:, :3] - expand(lv[k + 1][:, :3], lv[k])) * lv[k][:, 3:] + expand(r, lv[k])
    out = torch.round(ph + r).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    if not whole:
        x0, y0, x1, y1 = plan.region
        return out[:, y0 - wy0:y1 - wy0, x0 - wx0:x1 - wx0].contiguous()
    full = photo_u8[None].repeat(N, 1, 1, 1)
    full[:, wy0:wy1, wx0:wx1] = out
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--bands', type=int, nargs='+', default=[1, 2, 3, 4, 5])
    ap.add_argument('--no-torch', action='store_true', help='skip the torch composite (b)')
    a = ap.parse_args(argv)
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[:HP, :WP]
    photo = torch.from_numpy(np.clip(np.stack([128 + 80 * np.sin(xx / 170 + yy / 230), 100 + 60 * np.cos(xx / 110), 40 + yy / 16], -1) +
                                     rs.normal(0, 10, (HP, WP, 3)), 0, 255).astype(np.uint8)).to(dev)
    frames = torch.from_numpy(rs.randint(0, 256, (N, S, S, 3), dtype=np.uint8)).to(dev)
    plan = images.paste_plan(HP, WP, landmarks(), S)
    x0, y0, x1, y1 = plan.region
    print(f'photo {WP} x {HP}, {N} frames of {S}^2, scale {plan.scale:.4f} aligned px per photo px, box {x1 - x0} x {y1 - y0}, '
          f"'auto' = {images.paste_bands(plan, S, FEATHER)} bands", flush=True)
    big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(big)
    c = timed_gpu_ms(lambda: dst.copy_(big))
    bw = 2 * big.numel() / (c[0] * 1e-3)                                         # bytes read + written per second
    print(f'device copy of 1 GiB: {c[0]:.3f} ms, {bw / 1e12:.2f} TB/s read + written', flush=True)
    del big, dst
    photo_f, frames_f = photo.permute(2, 0, 1)[None].float(), frames.permute(0, 3, 1, 2).float().contiguous()
    rows = []
    for whole in (False, True):
        form = 'whole photograph per frame' if whole else 'bounding box alone'
        one = timed_gpu_ms(lambda: H.paste_back(photo, frames, plan.matrix, plan.region, FEATHER * S, whole=whole))
        print(f'{form}: (a) one-alpha paste_back {one[0]:8.3f} ms  (min {one[1]:.3f}, max {one[2]:.3f})', flush=True)
        for bands in a.bands:
            wx0, wy0, wx1, wy1 = H.paste_blend_window(plan.region, bands, HP, WP)
            px = N * (wx1 - wx0) * (wy1 - wy0)
            hip = lambda: H.paste_blend(photo, frames, plan.matrix, plan.region, bands, FEATHER * S, whole=whole)
            g = timed_gpu_ms(hip)
            line = (f'  bands {bands}: window {wx1 - wx0} x {wy1 - wy0}  HIP {g[0]:8.3f} ms  (min {g[1]:.3f}, max {g[2]:.3f})  '
                    f'{g[0] / one[0]:.2f}x of (a), +{g[0] - one[0]:.3f} ms')
            if not whole:                                                         # (the whole form also copies N photographs)
                line += f'  implied {g[0] * 1e-3 * bw / px:.1f} B/px (model: 18 fused, 60 level by level)'
            t = None
            if not a.no_torch:
                ref = lambda: torch_blend(photo_f, frames_f, plan, bands, whole, photo)
                d = (hip().to(torch.int16) - ref().to(torch.int16)).abs()
                diff, worst = float((d > 0).float().mean()), int(d.max())
                del d
                t = timed_gpu_ms(ref, reps=2)
                line += f'\n           (b) torch pyramid {t[0]:8.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})  {t[0] / g[0]:.2f}x of HIP; ' \
                        f'{diff:.3g} of the bytes differ, by at most {worst} levels'
                torch.cuda.empty_cache()
            print(line, flush=True)
            rows.append((whole, bands, g[0], one[0], None if t is None else t[0]))
    return rows


if __name__ == '__main__':
    main()
