"""Inference consumers at full size: orbit frames/s, 512^3 density grid, mean-latent statistics."""
import sys
import time
sys.path.insert(0, '/root/repo/3dgan-inversion_amd')
import torch
from inv3d_amd import inference as INF, synthetic as S

dev = torch.device('cuda')
G = S.make_generator(device=dev)
S.load_synthetic_weights(G, seed=0)
ws = S.synth_ws(14, 512, 1, seed=3).to(dev)


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


list(INF.render_orbit(G, ws, num_frames=4))
dt, frames = timed(lambda: [f for f in INF.render_orbit(G, ws, num_frames=60)])
print(f'orbit: {60 / dt:.1f} frames/s (512^2, backbone cached; {dt / 60 * 1e3:.2f} ms/frame)', flush=True)
INF.density_grid(G, ws, res=64)
for res in (256, 512):
    dt, g = timed(lambda: INF.density_grid(G, ws, res=res))
    print(f'density grid {res}^3: {dt * 1e3:.1f} ms = {res ** 3 / dt / 1e9:.2f} G points/s', flush=True)
dt, (w_avg, w_std) = timed(lambda: INF.estimate_w_stats(G, num_samples=10000))
print(f'w_avg over 10000 mapped latents: {dt * 1e3:.1f} ms (w_std {w_std:.4f})', flush=True)
# marching cubes alone on the full-size grid (g: the 512^3 grid of the loop above): count + scan + emit + faces, one host synchronise inside
from inv3d_amd import hipops as H
for level in (10.0, float(torch.quantile(g[60:-60:4, 60:-60:4, 60:-60:4].reshape(-1), 0.7))):
    H.marching_cubes(g, level)
    dt, (v, f) = timed(lambda: H.marching_cubes(g, level), reps=10)
    floor = 2 * g.numel() * 4            # two passes read the grid: >= 1 GB at 512^3 (~0.13 ms at 8 TB/s)
    print(f'marching cubes 512^3 level {level:.3f}: {dt * 1e3:.2f} ms, V {v.shape[0]} F {f.shape[0]}, '
          f'{floor / dt / 1e12:.2f} TB/s against the {floor / 1e9:.2f} GB byte floor', flush=True)
