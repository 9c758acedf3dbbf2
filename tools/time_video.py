"""Media export at full size (DESIGN.md 3.4 "Media export"): the GPU JPEG encoder against the render that feeds it, on the full-size synthetic
generator, 240 frames at 512^2.  Device events, median of 5 windows after warm-up.  Reports per-frame encode time at batch 1 and 16 (4:2:0,
quality 90), PIL's save(..., 'JPEG') of the same frames on the host, render_orbit alone, and write_orbit_video end to end with the file size.

  python tools/time_video.py [--frames 240] [--out DIR]"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import torch  # noqa: E402
from inv3d_amd import hipops as H, inference as INF, synthetic as S, video as V  # noqa: E402

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
    ap.add_argument('--frames', type=int, default=240)
    ap.add_argument('--out', default=None, help='directory for the video (default: a temporary one)')
    a = ap.parse_args()
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    ws = S.synth_ws(14, 512, 1, seed=3).to(dev)
    n = a.frames
    res = {}
    ms, _ = event_ms(lambda: [f for f in INF.render_orbit(G, ws, num_frames=n)])
    res['render_orbit_ms_per_frame'] = ms / n
    frames = torch.stack([f.float().clone() for f in INF.render_orbit(G, ws, num_frames=n)])
    for batch in (1, 16):
        ms, _ = event_ms(lambda: [H.jpeg_encode(frames[i:i + batch]) for i in range(0, n, batch)])
        res[f'encode_ms_per_frame_batch{batch}'] = ms / n
    sizes = []
    for i in range(0, n, 16):
        _, off = H.jpeg_encode(frames[i:i + 16])
        sizes += (off[1:] - off[:-1]).tolist()
    res['mean_frame_bytes'] = sum(sizes) / len(sizes)
    # the host alternative: the same frames, already uint8 HWC in host memory, through PIL (libjpeg); wall clock
    from PIL import Image
    u8 = torch.stack([H.image_grid_u8(frames[i:i + 1], nrow=1, padding=0) for i in range(n)]).cpu().numpy()
    t = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for i in range(n):
            Image.fromarray(u8[i]).save(io.BytesIO(), 'JPEG', quality=90, subsampling=2)
        t.append((time.perf_counter() - t0) * 1e3)
    res['pil_ms_per_frame'] = statistics.median(t) / n
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(a.out or tmp, 'orbit.avi')
        t = []
        for _ in range(1 + WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            V.write_orbit_video(G, ws, path, num_frames=n)
            t.append((time.perf_counter() - t0) * 1e3)
        res['write_orbit_video_ms_per_frame'] = statistics.median(t[1:]) / n
        res['video_bytes'] = os.path.getsize(path)
    res['frames'] = n
    res['launches_per_batch'] = 4
    for k, v in res.items():
        print(f'{k}: {v:.4f}' if isinstance(v, float) else f'{k}: {v}', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
