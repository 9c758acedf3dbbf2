"""Reconstruction metrics on the GPU: ms_ssim (csrc/ssim.hip) forward and forward + backward at N = 1 and 8, 512^2 x 3, against the same
computed by the fp32 torch restatement (tests/support/msssim_ref.py: grouped conv2d + avg_pool2d, what pytorch_msssim runs), and the whole
per-image evaluation block (metrics.reconstruction_metrics: mse, LPIPS-Alex, MS-SSIM, ArcFace identity) at 512^2.  Device events around
each timed window, after warm-up; median of 5 windows.

    python tools/time_metrics.py              # timings
    python tools/time_metrics.py --profile    # one forward + backward at N = 1 only (for rocprofv3 --kernel-trace --stats)
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import torch  # noqa: E402
import msssim_ref as M  # noqa: E402
from inv3d_amd import metrics as MT  # noqa: E402

dev = torch.device('cuda')


def pair(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, 512, 512, generator=g)
    return x.to(dev), (x + 0.1 * torch.randn(n, 3, 512, 512, generator=g)).to(dev)


def fwd(fn, x, y):
    return lambda: fn(x, y, data_range=1, size_average=False)


def fwd_bwd(fn, x, y):
    xs = x.clone().requires_grad_(True)
    return lambda: torch.autograd.grad(fn(xs, y, data_range=1, size_average=False).sum(), xs)


def timed_ms(f, reps=20, windows=5):
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


if '--profile' in sys.argv:
    x, y = pair(1)
    xs = x.clone().requires_grad_(True)
    v = MT.ms_ssim(xs, y, data_range=1, size_average=False)
    torch.autograd.grad(v.sum(), xs)
    torch.cuda.synchronize()
    print('profiled one ms_ssim forward + backward, N=1, 512^2 x 3', flush=True)
    sys.exit(0)

for n in (1, 8):
    x, y = pair(n)
    for what, mk in (('forward', fwd), ('forward+backward', fwd_bwd)):
        for name, fn in (('HIP kernels', MT.ms_ssim), ('fp32 torch restatement', M.ms_ssim)):
            med, lo, hi = timed_ms(mk(fn, x, y))
            print(f'ms_ssim {what:17s} N={n} 512^2x3  {name:23s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})', flush=True)

from inv3d_amd.loss_nets import LPIPSAlex  # noqa: E402
lp, idn = LPIPSAlex('pm1').to(dev), MT.IDLoss().to(dev)
g = torch.Generator().manual_seed(1)
img = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev)
tgt = (img.cpu() + 0.1 * torch.randn(1, 3, 512, 512, generator=g)).clamp(-1, 1).to(dev)
med, lo, hi = timed_ms(lambda: MT.reconstruction_metrics(img, tgt, lp, idn), reps=5)
print(f'evaluation block (reconstruction_metrics: mse, lpips, msssim, identity; four host reads) 512^2: {med:.3f} ms  (min {lo:.3f}, max {hi:.3f})',
      flush=True)
print(MT.format_metrics_txt(MT.reconstruction_metrics(img, tgt, lp, idn)), end='')
