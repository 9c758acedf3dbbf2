"""A full-size GANSpace fit on the GPU, timed: 10^5 latents of the full-size synthetic generator mapped at the frontal camera, D = 512
(ganspace/pca_anlaysis.py), split into mapping, second moments (csrc/pca.hip: per-slab fp32 MFMA products, fp64 across slabs) and the Jacobi
eigen-solver.  For comparison, the same covariance through torch.linalg.eigh on the device and numpy eigh on the host, and how far the Jacobi
eigenvalues are from the host's float64 ones.  Wall-clock around synchronised sections: every part is tens of milliseconds or more.  An offline
fit: there is no speed bar.

    python tools/time_ganspace.py [--samples 100000] [--chunk 8192]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--samples', type=int, default=100_000)
    ap.add_argument('--chunk', type=int, default=8192)
    a = ap.parse_args()
    from inv3d_amd import ganspace as GS, hipops as H, synthetic as S
    dev = torch.device('cuda')
    G = S.make_generator(device=dev)
    S.load_synthetic_weights(G, seed=0)
    for p in G.parameters():
        p.requires_grad_(False)
    list(GS.sample_w(G, a.chunk, chunk=a.chunk))                           # warm-up of the mapping network
    H.sym_eig(torch.eye(8, device=dev))
    chunks, t_map = timed(lambda: list(GS.sample_w(G, a.samples, chunk=a.chunk)))

    def moments():
        st = None
        for x in chunks:
            st = H.pca_moments(x, x.mean(0) if st is None else None, st)
        return H.pca_covariance(st)

    moments()
    (cov, mean, n), t_mom = timed(moments)
    (evals, evecs, sweeps, converged), t_eig = timed(lambda: H.sym_eig(cov))
    torch.linalg.eigh(cov)
    (tl, tv), t_torch = timed(lambda: torch.linalg.eigh(cov))
    c64 = cov.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    nl, nv = np.linalg.eigh(c64)
    t_np = (time.perf_counter() - t0) * 1e3
    lmax = float(nl.max())
    e_j = float(np.abs(evals.cpu().numpy().astype(np.float64) - nl[::-1]).max()) / (512 * 2.0 ** -23 * lmax)
    e_t = float(np.abs(tl.cpu().numpy().astype(np.float64) - nl).max()) / (512 * 2.0 ** -23 * lmax)
    _, t_fit = timed(lambda: GS.fit_pca(chunks, 512))
    print(f'{n} latents, D = {cov.shape[0]}, chunks of {a.chunk}')
    print(f'  mapping                {t_map:9.1f} ms')
    print(f'  moments + covariance   {t_mom:9.1f} ms')
    print(f'  sym_eig (Jacobi)       {t_eig:9.1f} ms   {sweeps} sweeps, converged {converged}, eigenvalues within {e_j:.2f} n eps lmax of float64')
    print(f'  torch.linalg.eigh      {t_torch:9.1f} ms   eigenvalues within {e_t:.2f} n eps lmax of float64')
    print(f'  numpy eigh (host, f64) {t_np:9.1f} ms')
    print(f'  fit_pca on the chunks  {t_fit:9.1f} ms')


if __name__ == '__main__':
    main()
