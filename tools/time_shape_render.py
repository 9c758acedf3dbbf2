"""Shape views at full size (DESIGN.md 3.4 "Shape views"): the iso-surface ray marcher against the render it sits beside, on the full-size
synthetic generator -- the 512^3 density grid, the level at the grid's 0.7 quantile (seeded weights do not reach the reference's 10), 512^2
pixels, the cameras of the 240-frame orbit.  Device events, median of 5 windows after a warm-up.  Reports the brick pass, iso_render per frame
with empty-space skipping on and off, and G.synthesis per frame with cached planes (the method of tools/time_video.py).

  python tools/time_shape_render.py [--frames 240] [--grid 512] [--res 512] [--quantile 0.7]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import hipops as H, inference as INF, synthetic as S  # noqa: E402

WINDOWS = 5


def event_ms(fn):
    """Median over WINDOWS windows of the device time of fn() (one warm-up call first)."""
    fn()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--frames', type=int, default=240, help='cameras taken evenly from the 240-frame orbit')
    ap.add_argument('--grid', type=int, default=512)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--quantile', type=float, default=0.7)
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    cams = INF.orbit_cameras(240, device=dev)[::max(1, 240 // a.frames)][:a.frames]
    n = cams.shape[0]
    res = dict(frames=n, grid=a.grid, res=a.res)
    ms, _ = event_ms(lambda: INF.density_grid(G, ws, res=a.grid))
    res['density_grid_ms'] = ms
    grid = INF.density_grid(G, ws, res=a.grid)
    # the quantile of a strided subsample (torch.quantile takes at most 2^24 elements); the padding's -1000 is part of the grid
    sample = grid.reshape(-1)[::max(1, grid.numel() // (1 << 22))]
    level = float(torch.quantile(sample, a.quantile))
    res['level'] = level
    origin, spacing, axes = INF.grid_frame(G, a.grid)
    ms, _ = event_ms(lambda: H.iso_bricks(grid))
    res['bricks_ms'] = ms
    bricks = H.iso_bricks(grid)
    res['bricks_below_level'] = float((bricks <= level).float().mean())
    for skip in (True, False):
        kw = dict(bricks=bricks) if skip else {}
        ms, _ = event_ms(lambda: [H.iso_render(grid, cams[i:i + 1], a.res, level, origin, spacing, axes, skip=skip, **kw) for i in range(n)])
        res[f'iso_render_ms_per_frame_skip_{"on" if skip else "off"}'] = ms / n
    out = H.iso_render(grid, cams, a.res, level, origin, spacing, axes, bricks=bricks)
    res['hit_fraction'] = float(out['mask'].float().mean())
    ms, _ = event_ms(lambda: [G.synthesis(ws, cams[i:i + 1], noise_mode='const', cache_backbone=(i == 0), use_cached_backbone=(i > 0)) for i in range(n)])
    res['synthesis_ms_per_frame'] = ms / n
    res['launches'] = dict(bricks=1, iso_render=1)
    for k, v in res.items():
        print(f'{k}: {v:.4f}' if isinstance(v, float) else f'{k}: {v}', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
