"""Every implicit-GEMM conv launch of one eager C2 step, in order: geometry, epilogue, time, algorithmic TFLOP/s (in-situ, HIP events).

    python tools/conv_launch_table.py                  # needs a GPU
    python tools/conv_launch_table.py --plan [N]       # no GPU: what inv3d_amd/conv_plan.py routes every modulated 3x3 layer of the full-size generator to
    python tools/conv_launch_table.py --plan --json    # ... as tests/golden/conv_routes.json (N in 1, 2, 8; frozen / trainable weights; f16x3 / f16x1)
"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
import torch
from inv3d_amd import synthetic as S, hipops as H, conv_plan as P


def modconv_layers():
    """(name, Ci, Co, Hi, Wi, up) of every SynthesisLayer of the full-size generator (built on the CPU)."""
    from inv3d_amd.training.networks_stylegan2 import SynthesisLayer
    G = S.make_generator(device='cpu')
    return [(n, m.in_channels, m.out_channels, m.resolution // m.up, m.resolution // m.up, m.up) for n, m in G.named_modules() if isinstance(m, SynthesisLayer)]


def plan_json():
    lines = []
    for name, ci, co, hi, wi, up in modconv_layers():
        rows = [f'   "N{n} {"frozen" if frozen else "trainable"} {prec}": {json.dumps(P.describe(n, ci, co, hi, wi, 3, up, prec, frozen), sort_keys=True)}'
                for n in (1, 2, 8) for frozen in (True, False) for prec in ('f16x3', 'f16x1')]
        lines.append(f' "{name}": {{\n  "geometry": {json.dumps(dict(Ci=ci, Co=co, Hi=hi, Wi=wi, up=up))},\n  "routes": {{\n' + ',\n'.join(rows) + '\n  }\n }')
    return '{\n' + ',\n'.join(lines) + '\n}'


def plan_table(n):
    def short(p):
        if p is None:
            return '-'
        extra = [f'rows {p.rows}' if getattr(p, 'rows', 0) else '', f'rows,waves {p.v3}' if getattr(p, 'v3', None) else '',
                 f'ks {p.ksplit}' if getattr(p, 'ksplit', 1) > 1 else '', 'ragged' if getattr(p, 'ragged', False) else '', '+rgb' if getattr(p, 'rgb_head', False) else '']
        return ' '.join([str(p.form)] + [e for e in extra if e])
    print(f'N = {n}, f16x3.  forward / data gradient with frozen weights; [..] where trainable weights differ; weight gradient')
    print(f'{"layer":30s} {"in":>14} up  {"forward":26s} {"dgrad":26s} wgrad')
    for name, ci, co, hi, wi, up in modconv_layers():
        g = (n, ci, co, hi, wi, 3, up, 'f16x3')
        f, d, ft, dt = P.plan_forward(*g, True), P.plan_dgrad(*g, True), P.plan_forward(*g, False), P.plan_dgrad(*g, False, need_w=True)
        fs = short(f) + (f' [{short(ft)}]' if ft != f else '')
        ds = short(d) + (f' [{short(dt)}]' if dt.form != d.form else '')
        print(f'{name.replace("synthesis.", ""):30s} {hi:4d}x{wi:<4d}x{ci:<4d} {up:2d}  {fs:26s} {ds:26s} {P.plan_wgrad(*g).form}')


if '--plan' in sys.argv:
    if '--json' in sys.argv:
        print(plan_json())
    else:
        plan_table(int(sys.argv[-1]) if sys.argv[-1].isdigit() else 1)
    sys.exit(0)

from inv3d_amd.inversion import LatentProjector
dev = torch.device('cuda')
G = S.make_generator(device=dev); S.load_synthetic_weights(G, seed=0)
cam = S.synth_cameras(1, seed=2).to(dev)
with torch.no_grad():
    target = G.synthesis(S.synth_ws(14, 512, 1, seed=3).to(dev), cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
proj = LatentProjector(G, target, num_steps=400, cam=cam, seed=100); proj.preheat = 0
for _ in range(3): proj.step()
reps = 5
profs = []
for _ in range(reps):
    prof = H.LaunchProfiler(keep_meta=True); H.PROFILER = prof
    proj.step(); torch.cuda.synchronize(); H.PROFILER = None
    profs.append(prof)
EPI = {0: 'store', 1: 'atomic', 2: 'fwd', 3: 'bwd'}
PREC = {0: 'f32', 1: 'bf16x6', 2: 'bf16x3', 3: 'f16x3'}
tot = 0.0
print(f'{"#":>3} cfg {"in":>14} {"out":>14} taps           epi    ks prec   {"GF":>7} {"us":>7} {"TF/s":>6}')
for i, (rec, m) in enumerate(zip(profs[0].records, profs[0].meta)):
    us = sorted(p.records[i][2].elapsed_time(p.records[i][3]) for p in profs)[reps // 2] * 1e3
    tot += us
    print(f'{i:3d} {rec[0][0]:3d} {m["Hi"]:4d}x{m["Wi"]:<4d}x{m["Ck"]:<4d} {m["Ho"]:4d}x{m["Wo"]:<4d}x{m["Nc"]:<4d} {str(m["taps"]):14s} {EPI[m["epi"]]:6s} {m["ksplit"]:2d} {PREC[m["prec"]]:6s} '
          f'{rec[1] / 1e9:7.2f} {us:7.1f} {rec[1] / us / 1e6:6.1f}')
print(f'total {tot / 1e3:.3f} ms over {len(profs[0].records)} launches')
