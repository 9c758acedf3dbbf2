"""The passes of a C2 step that touch only the optimised parameters -- the style bank (forward, backward), the noise regulariser and Adam -- each
timed alone with HIP events, at exactly the arguments one eager step of bench.py's projector hands them (recorded from that step, then replayed
back to back from a HIP graph, so the operands are in the caches: the step's own figures come from the kernel trace).  us per call (a call is
1 .. 3 kernels) and TB/s over the bytes the call must move.     usage: [EG3D_LIBNAME=libeg3d_hip_prev.so] python tools/time_param_passes.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import hipops as H, synthetic as S       # noqa: E402
from inv3d_amd.inversion import LatentProjector          # noqa: E402

DEV = torch.device('cuda', 0)


def timeit(f, reps=20, iters=10):
    """us per call of f, replayed `reps` times back to back from one HIP graph (the host side of a call costs more than its kernels run)."""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            f()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (iters * reps) * 1e3


def main():
    torch.cuda.set_device(0)
    G = S.make_generator(device=DEV)
    S.load_synthetic_weights(G, seed=0)
    cam = S.synth_cameras(1, seed=2).to(DEV)
    with torch.no_grad():
        target = G.synthesis(S.synth_ws(14, 512, 1, seed=3).to(DEV), cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    proj = LatentProjector(G, target, num_steps=400, cam=cam, seed=100, use_graph=False)
    proj.preheat = 0
    proj.step()
    calls = []           # (name, bytes, closure)
    orig_style, orig_reg, orig_adam = H.style_affine, H.noise_regularizer, H.HipAdam.step

    def style(ws, layers, **kw):
        nbytes = sum(l[0].numel() * 4 for l in layers) + sum(d[0].numel() * 4 for d in (kw.get('demod') or []) if d is not None)
        calls.append(('style bank ' + ('backward' if kw.get('backward') else 'forward') + f' ({len(layers)} layers)', nbytes, lambda: orig_style(ws, layers, **kw)))
        return orig_style(ws, layers, **kw)

    def reg(bufs, **kw):
        nbytes = sum(b.numel() * 4 for b in bufs) * 2 * (2 if kw.get('want_grad', True) else 1)
        calls.append((f'noise regulariser ({len(bufs)} maps)', nbytes, lambda: orig_reg(bufs, **kw)))
        return orig_reg(bufs, **kw)

    def adam(self, *a, **kw):
        n = sum(p.numel() for g in self.param_groups for p in g['params']) if hasattr(self, 'param_groups') else 0
        grads = [p.grad for p in self.params]          # (the projector drops them after the step)

        def again():
            for p, g in zip(self.params, grads):
                p.grad = g
            orig_adam(self, *a, **kw)          # + the fill of its 2 n + 1 word workspace, which the step's zero arena spares it
        calls.append((f'Adam ({n} elements)', n * 4 * 9, again))
        return orig_adam(self, *a, **kw)
    H.style_affine, H.noise_regularizer, H.HipAdam.step = style, reg, adam
    try:
        proj.step()
    finally:
        H.style_affine, H.noise_regularizer, H.HipAdam.step = orig_style, orig_reg, orig_adam
    torch.cuda.synchronize()
    print(f'library {os.environ.get("EG3D_LIBNAME", "libeg3d_hip.so")}')
    for name, nbytes, f in calls:
        t = timeit(f)
        print(f'{name:40s} {nbytes / 1e6:6.1f} MB   {t:6.1f} us  {nbytes / t / 1e6:5.2f} TB/s', flush=True)


if __name__ == '__main__':
    main()
