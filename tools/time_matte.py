"""Head mattes on the GPU (hipops.edt2, hipops.matte8, images.matte_from_mask; csrc/matte.hip): what the chain costs and which path AUTO
should take.  Device events around each timed window, after warm-up; median of 5 windows (min, max beside it).

  1. the default chain (open 0.02, close 0.04: five transforms, then the matte) on a 128^2 head mask -> 512^2, N = 1 and 16, RESIDENT (one
     launch for the five transforms) against TILED (ten), and the two halves (edt2, matte8) on their own
  2. TILED at 512^2 -> 512^2 (head_matte(source='shape'))
  3. the worst case of the row scan: one foreground pixel in a corner (every background lane scans to it), plain transform and full chain
  4. the same chain on the host with scipy (binary_erosion / binary_dilation with discs, two distance_transform_edt), for scale
  5. the matte's share of a pasted orbit batch: 16 frames rendered (render_orbit), matted, pasted into a 1024^2 photograph, JPEG-encoded

    python tools/time_matte.py [--small]          (--small: the 32-wide synthetic generator for part 5, a rehearsal)
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, '3dgan-inversion_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from inv3d_amd import hipops as H, images  # noqa: E402

dev = torch.device('cuda')


def head_mask(n, s, seed=0):
    """n ragged head-like masks of side s: an ellipse, a few holes inside, a few specks outside."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:s, :s]
    out = []
    for _ in range(n):
        cy, cx = 0.52 + 0.03 * rs.randn(), 0.5 + 0.03 * rs.randn()
        m = ((yy - cy * s) ** 2 / (0.36 * s) ** 2 + (xx - cx * s) ** 2 / (0.30 * s) ** 2) < 1.0
        for _ in range(8):
            y, x = rs.randint(s // 3, 2 * s // 3, 2)
            m[y:y + 1 + s // 64, x:x + 1 + s // 64] = False
        m[rs.randint(0, s // 10 + 1, 8), rs.randint(0, s, 8)] = True
        out.append(m)
    return torch.from_numpy(np.stack(out).astype(np.uint8) * 255).to(dev)


def timed_gpu_ms(f, reps=20, windows=5):
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


def line(what, t):
    print(f'  {what:<58s} {t[0] * 1e3:9.1f} us  (min {t[1] * 1e3:.1f}, max {t[2] * 1e3:.1f})', flush=True)


def scipy_chain(mask, size, open=0.02, close=0.04):
    from scipy import ndimage as ndi

    def disc(r):
        k = int(math.floor(r))
        yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
        return (yy * yy + xx * xx) <= r * r
    s = mask.shape[0]
    fg = mask != 0
    fg = ndi.binary_dilation(ndi.binary_erosion(fg, disc(open * s), border_value=1), disc(open * s))
    fg = ndi.binary_erosion(ndi.binary_dilation(fg, disc(close * s)), disc(close * s), border_value=1)
    d = ndi.distance_transform_edt(fg) - ndi.distance_transform_edt(~fg)
    return ndi.zoom(d, size / s, order=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--small', action='store_true')
    a = ap.parse_args(argv)
    print('1. default chain, 128^2 -> 512^2', flush=True)
    for n in (1, 16):
        m = head_mask(n, 128)
        t = images.matte_thresholds(128)
        same = torch.equal(H.edt2(m, t, impl='resident'), H.edt2(m, t, impl='tiled'))
        print(f' N = {n}: thresholds {t}, RESIDENT == TILED: {same}', flush=True)
        for impl in ('resident', 'tiled'):
            line(f'matte_from_mask impl={impl}', timed_gpu_ms(lambda: images.matte_from_mask(m, 512, impl=impl)))
            line(f'  edt2 alone, 4 stages, impl={impl}', timed_gpu_ms(lambda: H.edt2(m, t, impl=impl)))
            line(f'  edt2 alone, no stage, impl={impl}', timed_gpu_ms(lambda: H.edt2(m, (), impl=impl)))
        sd2 = H.edt2(m, t)
        line('  matte8 alone', timed_gpu_ms(lambda: H.matte8(sd2, 512, feather_px=0.03 * 512)))
    print('2. TILED, 512^2 -> 512^2', flush=True)
    for n in (1, 16):
        m = head_mask(n, 512)
        line(f'matte_from_mask N = {n}', timed_gpu_ms(lambda: images.matte_from_mask(m, 512), reps=5))
        line(f'  edt2 alone, no stage, N = {n}', timed_gpu_ms(lambda: H.edt2(m), reps=5))
    print('3. one foreground pixel in a corner', flush=True)
    for s, impls in ((128, ('resident', 'tiled')), (512, ('tiled',))):
        m = torch.zeros((1, s, s), dtype=torch.uint8, device=dev)
        m[0, s - 1, 0] = 255
        for impl in impls:
            line(f'edt2 {s}^2, no stage, impl={impl}', timed_gpu_ms(lambda: H.edt2(m, (), impl=impl), reps=5))
            line(f'matte_from_mask {s}^2 -> 512^2, impl={impl}', timed_gpu_ms(lambda: images.matte_from_mask(m, 512, impl=impl), reps=5))
    print('4. the chain on the host (scipy), 128^2 -> 512^2, one frame', flush=True)
    host = head_mask(1, 128)[0].cpu().numpy()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        scipy_chain(host, 512)
        ts.append((time.perf_counter() - t0) * 1e3)
    line('scipy morphology + 2 EDT + bilinear zoom (no copies counted)', (statistics.median(ts), min(ts), max(ts)))
    print('5. a pasted orbit batch of 16 frames', flush=True)
    from inv3d_amd import synthetic as S
    from inv3d_amd.inference import render_orbit
    if a.small:
        from oracle import eg3d_oracle as O
        G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                             rendering_kwargs=O.small_config().rendering, device=dev)
    else:
        G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(0)).to(dev)
    side = int(G.img_resolution)
    lm = np.zeros((68, 2))
    eye_avg, e2e, e2m = np.array([512.5, 460.5]), np.array([128.0, 6.0]), np.array([-4.0, 140.0])
    lm[36:42], lm[42:48] = eye_avg - e2e / 2, eye_avg + e2e / 2
    lm[48] = lm[54] = eye_avg + e2m
    photo = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (1024, 1024, 3), dtype=np.uint8)).to(dev)
    state = {}

    def render():
        pairs = [(f.float().clone(), d.float().clone()) for f, d in render_orbit(G, ws, num_frames=16, with_depth=True)]
        state['frames'], state['depth'] = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    def matte():
        state['matte'] = images.head_matte(G, ws, None, size=side, depth=state['depth'])

    def paste(with_matte):
        state['pasted'] = images.paste_back(photo, state['frames'], lm, region='bbox', layout='chw', mask=state['matte'] if with_matte else None)

    def encode():
        H.jpeg_encode(state['pasted'], quality=90)[0].cpu()
    with torch.no_grad():
        render()
        print(f' frames {tuple(state["frames"].shape)}, depth {tuple(state["depth"].shape)}', flush=True)
        r = timed_gpu_ms(render, reps=1, windows=3)
        line('render 16 frames (render_orbit, backbone cached)', r)
        mt = timed_gpu_ms(matte, reps=5)
        line('head_matte(depth=...) of the 16 frames', mt)
        line('paste_back, feathered square', timed_gpu_ms(lambda: paste(False), reps=5))
        p = timed_gpu_ms(lambda: paste(True), reps=5)
        line('paste_back through the matte', p)
        e = timed_gpu_ms(encode, reps=3)
        line('jpeg_encode + copy to the host', e)
        print(f'  the matte is {100.0 * mt[0] / (r[0] + mt[0] + p[0] + e[0]):.2f} % of render + matte + paste + JPEG', flush=True)


if __name__ == '__main__':
    main()
