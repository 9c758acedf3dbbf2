// GANSpace latent editing (ganspace/pca_anlaysis.py, estimator.py, run_ganspace.py of the reference): the device side of a PCA of W and of the edit grids.
//
//   moments      (x - shift)^T (x - shift) and column sums of (x - shift) for row data [S, D <= 512], per slab of EG3D_PCA_SLAB_ROWS rows: every wave owns a
//                32 x 32 tile of one slab and streams row pairs into v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain).  Slabs are then added in slab order into
//                fp64 accumulators and turned into the ddof-0 covariance.  No atomics anywhere: both builds of the library give the same bits (no det.h).
//   sym_eig      one-sided (Hestenes) Jacobi with a round-robin ordering.  The working matrix W = A V and V are kept TRANSPOSED (a column is a contiguous row;
//                A symmetric: W0^T = A, V0^T = I).  A round's n/2 disjoint rotations are one launch, one wave per pair; the round boundary is the launch
//                boundary (no grid barrier, no persistent kernel, nothing waits on another workgroup).  The sweep loop is on the host, bounded by max_sweeps.
//   image grid   [N,3,H,W] fp32 -> uint8 HWC in torchvision.utils.make_grid's layout.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------ moments
constexpr int SLAB_ROWS = EG3D_PCA_SLAB_ROWS;
constexpr int MOM_UNROLL = 8;            // row pairs in flight per wave and trip
static_assert(SLAB_ROWS % (2 * MOM_UNROLL) == 0, "a slab is a whole number of trips");

// grid (slabs, tiles): tile t -> the 64 x 64 block (ti <= tj) of the upper triangle; wave w -> its 32 x 32 quarter.  Elements below the diagonal of
// gram_part are not written (and never read).  Diagonal tiles also write the slab's column sums of their 64 columns.
__global__ void __launch_bounds__(256) pca_moments_kernel(const float* __restrict__ x, int64_t S, int D, int64_t ldx, const float* __restrict__ shift,
                                                          float* __restrict__ gram_part, float* __restrict__ sum_part, int ntile) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 31, h = lane >> 5;
    int ti = 0, t = blockIdx.y;
    while (t >= ntile - ti) { t -= ntile - ti; ++ti; }               // row ti of the triangle holds ntile - ti tiles
    const int tj = ti + t;
    const int i0 = ti * 64 + (wave >> 1) * 32, j0 = tj * 64 + (wave & 1) * 32;
    if (i0 >= D || j0 >= D || j0 + 31 < i0) return;                  // outside the matrix, or wholly below the diagonal
    const int64_t slab = blockIdx.x, r_begin = slab * SLAB_ROWS, r_end = r_begin + SLAB_ROWS < S ? r_begin + SLAB_ROWS : S;
    const bool ia = i0 + l < D, jb = j0 + l < D;
    const float sa = ia ? shift[i0 + l] : 0.f, sb = jb ? shift[j0 + l] : 0.f;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float cs = 0.f;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += 2 * MOM_UNROLL) {
        float av[MOM_UNROLL], bv[MOM_UNROLL];
#pragma unroll
        for (int u = 0; u < MOM_UNROLL; ++u) {
            const int64_t row = r0 + 2 * u + h;
            const bool ok = row < r_end;
            const float* xr = x + row * ldx;
            av[u] = (ok && ia) ? xr[i0 + l] - sa : 0.f;
            bv[u] = (ok && jb) ? xr[j0 + l] - sb : 0.f;
        }
#pragma unroll
        for (int u = 0; u < MOM_UNROLL; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            cs += av[u];
        }
    }
    float* gp = gram_part + slab * (int64_t)D * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * h, j = j0 + l;
        if (i < D && j < D && i <= j) gp[(int64_t)i * D + j] = acc[r];
    }
    if (i0 == j0) {                                                  // waves 0 and 3 of a diagonal tile: columns i0 .. i0 + 31
        cs += __shfl_xor(cs, 32);                                    // even rows + odd rows
        if (h == 0 && ia) sum_part[slab * D + i0 + l] = cs;
    }
}

__global__ void __launch_bounds__(256) pca_accumulate_kernel(const float* __restrict__ gram_part, const float* __restrict__ sum_part, int slabs, int D,
                                                             double* __restrict__ gram, double* __restrict__ sum) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, DD = (int64_t)D * D;
    if (idx < DD) {
        const int i = (int)(idx / D), j = (int)(idx % D);
        const float* p = gram_part + (i <= j ? (int64_t)i * D + j : (int64_t)j * D + i);
        double g = gram[idx];
        for (int s = 0; s < slabs; ++s) g += (double)p[s * DD];
        gram[idx] = g;
    } else if (idx < DD + D) {
        const int j = (int)(idx - DD);
        double g = sum[j];
        for (int s = 0; s < slabs; ++s) g += (double)sum_part[(int64_t)s * D + j];
        sum[j] = g;
    }
}

__global__ void __launch_bounds__(256) pca_covariance_kernel(const double* __restrict__ gram, const double* __restrict__ sum, double inv_s, int D,
                                                             const float* __restrict__ shift, float* __restrict__ cov, float* __restrict__ mean) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, DD = (int64_t)D * D;
    if (idx < DD) {
        const int i = (int)(idx / D), j = (int)(idx % D), a = i <= j ? i : j, b = i <= j ? j : i;     // the upper triangle, mirrored: exactly symmetric
        const double ma = sum[a] * inv_s, mb = sum[b] * inv_s;
        cov[idx] = (float)(gram[(int64_t)a * D + b] * inv_s - ma * mb);
    } else if (idx < DD + D) {
        const int j = (int)(idx - DD);
        mean[j] = (float)((double)shift[j] + sum[j] * inv_s);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ eigen-solver
constexpr int EIG_MAX_N = 512;
constexpr int EIG_PER_LANE = EIG_MAX_N / 64;

struct eig_workspace {
    float *wt, *vt, *lam, *crit, *scalars;     // scalars: [0] skip threshold (squared norm), [1] largest criterion of the sweep
    int32_t* rank;
};
int64_t eig_align(int64_t floats) { return (floats + 63) / 64 * 64; }
int64_t eig_workspace_floats(int n) { return 2 * eig_align((int64_t)n * n) + 3 * eig_align(n) + eig_align(2); }
eig_workspace eig_carve(void* workspace, int n) {
    eig_workspace w;
    float* p = reinterpret_cast<float*>(workspace);
    w.wt = p; p += eig_align((int64_t)n * n);
    w.vt = p; p += eig_align((int64_t)n * n);
    w.lam = p; p += eig_align(n);
    w.crit = p; p += eig_align(n);
    w.rank = reinterpret_cast<int32_t*>(p); p += eig_align(n);
    w.scalars = p;
    return w;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ void __launch_bounds__(256) eig_init_kernel(const float* __restrict__ a, int n, float* __restrict__ wt, float* __restrict__ vt) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    wt[idx] = a[(int64_t)j * n + i];             // column i of A (= its row i when A is symmetric, which the caller promises)
    vt[idx] = i == j ? 1.f : 0.f;
}

// One block: the largest squared column norm of W -> the skip threshold of this sweep, and the sweep's criteria cleared.
__global__ void __launch_bounds__(1024) eig_sweep_begin_kernel(const float* __restrict__ wt, int n, float skip_rel2, float* __restrict__ crit, int ncrit,
                                                               float* __restrict__ scalars) {
    __shared__ float s_max[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = 0.f;
    for (int row = wave; row < n; row += 16) {
        float q = 0.f;
        for (int k = lane; k < n; k += 64) { const float v = wt[(int64_t)row * n + k]; q = fmaf(v, v, q); }
        m = fmaxf(m, wave_sum(q));
    }
    if (lane == 0) s_max[wave] = m;
    for (int k = threadIdx.x; k < ncrit; k += 1024) crit[k] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, s_max[w]);
        scalars[0] = skip_rel2 * m;
        scalars[1] = 0.f;
    }
}

__global__ void __launch_bounds__(64) eig_sweep_end_kernel(const float* __restrict__ crit, int ncrit, float* __restrict__ scalars) {
    float m = 0.f;
    bool bad = false;
    for (int k = threadIdx.x; k < ncrit; k += 64) { const float c = crit[k]; bad |= !(c == c); m = fmaxf(m, c); }
    m = wave_max(m);
    bad = __any(bad);
    if (threadIdx.x == 0) scalars[1] = bad ? __builtin_nanf("") : m;          // a NaN never counts as converged
}

// Round `round` of the circle method on m = n + (n & 1) players: block b = 0 pairs (m - 1, round), block b > 0 pairs ((round + b) mod (m - 1),
// (round - b) mod (m - 1)).  Player n of an odd n does not exist: its partner has a bye.  One wave rotates columns p, q of W and of V (rows of wt / vt).
__global__ void __launch_bounds__(64) eig_round_kernel(float* __restrict__ wt, float* __restrict__ vt, int n, int m, int round, float tol,
                                                       float* __restrict__ crit, const float* __restrict__ scalars) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int p, q;
    if (b == 0) { p = m - 1; q = round; }
    else { p = (round + b) % (m - 1); q = (round - b + (m - 1)) % (m - 1); }
    if (p > q) { const int t = p; p = q; q = t; }
    if (q >= n) return;                                                       // the bye
    float* wp = wt + (int64_t)p * n;
    float* wq = wt + (int64_t)q * n;
    float a[EIG_PER_LANE], c[EIG_PER_LANE];
    float alpha = 0.f, beta = 0.f, gamma = 0.f;
#pragma unroll
    for (int k = 0; k < EIG_PER_LANE; ++k) {
        const int e = lane + 64 * k;
        a[k] = e < n ? wp[e] : 0.f;
        c[k] = e < n ? wq[e] : 0.f;
        alpha = fmaf(a[k], a[k], alpha);
        beta = fmaf(c[k], c[k], beta);
        gamma = fmaf(a[k], c[k], gamma);
    }
    alpha = wave_sum(alpha); beta = wave_sum(beta); gamma = wave_sum(gamma);
    // columns of the numerical null space are rounding noise, never relatively orthogonal to anything: pairs with one are left alone
    if (!(fminf(alpha, beta) > scalars[0]) && alpha == alpha && beta == beta) return;
    const float criterion = fabsf(gamma) / sqrtf(alpha * beta);               // NaN input: NaN, recorded, never "converged"
    if (lane == 0) crit[b] = (criterion == criterion) ? fmaxf(crit[b], criterion) : criterion;
    if (!(criterion > tol)) return;
    const float zeta = (beta - alpha) / (2.f * gamma);
    const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
    const float cs = 1.f / sqrtf(1.f + t * t), sn = cs * t;
#pragma unroll
    for (int k = 0; k < EIG_PER_LANE; ++k) {
        const int e = lane + 64 * k;
        if (e < n) {
            wp[e] = cs * a[k] - sn * c[k];
            wq[e] = sn * a[k] + cs * c[k];
        }
    }
    float* vp = vt + (int64_t)p * n;
    float* vq = vt + (int64_t)q * n;
#pragma unroll
    for (int k = 0; k < EIG_PER_LANE; ++k) {
        const int e = lane + 64 * k;
        if (e < n) {
            const float x = vp[e], y = vq[e];
            vp[e] = cs * x - sn * y;
            vq[e] = sn * x + cs * y;
        }
    }
}

// lam[i] = v_i . w_i / v_i . v_i (the Rayleigh quotient of column i: signed, second order in the vector's error)
__global__ void __launch_bounds__(64) eig_rayleigh_kernel(const float* __restrict__ wt, const float* __restrict__ vt, int n, float* __restrict__ lam) {
    const int i = blockIdx.x, lane = threadIdx.x;
    float vw = 0.f, vv = 0.f;
    for (int e = lane; e < n; e += 64) {
        const float v = vt[(int64_t)i * n + e];
        vw = fmaf(v, wt[(int64_t)i * n + e], vw);
        vv = fmaf(v, v, vv);
    }
    vw = wave_sum(vw); vv = wave_sum(vv);
    if (lane == 0) lam[i] = vw / vv;
}

// rank[i] = position of lam[i] in descending order (ties: the lower index first; a NaN after everything that is not)
__global__ void __launch_bounds__(256) eig_rank_kernel(const float* __restrict__ lam, int n, int32_t* __restrict__ rank) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float li = lam[i];
    const bool ni = !(li == li);
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const float lj = lam[j];
        const bool nj = !(lj == lj);
        const bool before = ni ? (!nj || j < i) : (!nj && (lj > li || (lj == li && j < i)));
        r += before ? 1 : 0;
    }
    rank[i] = r;
}

// row rank[i] of the output = +-v_i / |v_i|, signed so that its largest-magnitude entry (the first of equals) is positive
__global__ void __launch_bounds__(64) eig_emit_kernel(const float* __restrict__ vt, const float* __restrict__ lam, const int32_t* __restrict__ rank, int n,
                                                      float* __restrict__ evals, float* __restrict__ evecs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const float* v = vt + (int64_t)i * n;
    float vv = 0.f, best = -1.f;
    int best_e = 0x7fffffff;
    for (int e = lane; e < n; e += 64) {                                      // ascending e per lane: a strict > keeps the first of equals
        const float x = v[e], ax = fabsf(x);
        vv = fmaf(x, x, vv);
        if (ax > best) { best = ax; best_e = e; }
    }
    vv = wave_sum(vv);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oe = __shfl_xor(best_e, o);
        if (ob > best || (ob == best && oe < best_e)) { best = ob; best_e = oe; }
    }
    const float pivot = best_e < n ? v[best_e] : 1.f;
    const float scale = (pivot < 0.f ? -1.f : 1.f) / sqrtf(vv);
    const int r = rank[i];
    for (int e = lane; e < n; e += 64) evecs[(int64_t)r * n + e] = v[e] * scale;
    if (lane == 0) evals[r] = lam[i];
}

// ------------------------------------------------------------------------------------------------------------------------------------ image grid
__global__ void __launch_bounds__(256) image_grid_u8_kernel(const float* __restrict__ img, int N, int H, int W, int xmaps, int padding, int pad_value, int Ht,
                                                            int Wt, uint8_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Ht * Wt) return;
    const int y = (int)(idx / Wt) - padding, x = (int)(idx % Wt) - padding, ch = H + padding, cw = W + padding;
    uint8_t* o = out + idx * 3;
    int k = -1, iy = 0, ix = 0;
    if (y >= 0 && x >= 0) {
        const int row = y / ch, col = x / cw;
        iy = y % ch; ix = x % cw;
        if (iy < H && ix < W && col < xmaps && row * xmaps + col < N) k = row * xmaps + col;
    }
    if (k < 0) { o[0] = o[1] = o[2] = (uint8_t)pad_value; return; }
    const float* p = img + ((int64_t)k * 3 * H + iy) * W + ix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = p[(int64_t)c * H * W] * 127.5f + 128.f;              // (-ffp-contract=off: a product, then a sum, as the reference)
        o[c] = (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f);                     // truncation toward zero
    }
}

}  // namespace

extern "C" int eg3d_pca_moments_slabs(int64_t S, int D) {
    if (S < 1 || D < 1) return EG3D_ERR_INVALID;
    if (D > 512) return EG3D_ERR_UNSUPPORTED;
    const int64_t slabs = (S + SLAB_ROWS - 1) / SLAB_ROWS;
    return slabs > 0x7fffffffLL / 2 ? EG3D_ERR_TOO_LARGE : (int)slabs;
}

extern "C" int eg3d_pca_moments(const float* x, int64_t S, int D, int64_t ldx, const float* shift, float* gram_part, float* sum_part, void* stream) {
    if (!x || !shift || !gram_part || !sum_part || ldx < D) return EG3D_ERR_INVALID;
    const int slabs = eg3d_pca_moments_slabs(S, D);
    if (slabs < 0) return slabs;
    const int ntile = (D + 63) / 64;
    hipLaunchKernelGGL(pca_moments_kernel, dim3(slabs, ntile * (ntile + 1) / 2), dim3(256), 0, (hipStream_t)stream, x, S, D, ldx, shift, gram_part, sum_part, ntile);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_pca_moments_accumulate(const float* gram_part, const float* sum_part, int slabs, int D, double* gram, double* sum, void* stream) {
    if (!gram_part || !sum_part || !gram || !sum || slabs < 1 || D < 1) return EG3D_ERR_INVALID;
    if (D > 512) return EG3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pca_accumulate_kernel, dim3(eg3d_cdiv((int64_t)D * D + D, 256)), dim3(256), 0, (hipStream_t)stream, gram_part, sum_part, slabs, D, gram, sum);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_pca_covariance(const double* gram, const double* sum, int64_t S_total, int D, const float* shift, float* cov, float* mean, void* stream) {
    if (!gram || !sum || !shift || !cov || !mean || S_total < 1 || D < 1) return EG3D_ERR_INVALID;
    if (D > 512) return EG3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pca_covariance_kernel, dim3(eg3d_cdiv((int64_t)D * D + D, 256)), dim3(256), 0, (hipStream_t)stream, gram, sum, 1.0 / (double)S_total, D, shift,
                       cov, mean);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_sym_eig_workspace(int n, int64_t* bytes) {
    if (!bytes || n < 1) return EG3D_ERR_INVALID;
    if (n > EIG_MAX_N) return EG3D_ERR_UNSUPPORTED;
    *bytes = eig_workspace_floats(n) * (int64_t)sizeof(float);
    return EG3D_OK;
}

extern "C" int eg3d_sym_eig(const float* a, int n, float* evals, float* evecs, int max_sweeps, float tol, void* workspace, int32_t* info, void* stream) {
    if (!a || !evals || !evecs || !workspace || !info || n < 1 || max_sweeps < 1 || ((uintptr_t)workspace & 15)) return EG3D_ERR_INVALID;
    if (n > EIG_MAX_N) return EG3D_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    const eig_workspace w = eig_carve(workspace, n);
    const float eps = 1.1920928955078125e-7f;
    if (!(tol > 0.f)) tol = 8.f * eps;
    const int m = n + (n & 1), npairs = m / 2;
    // an fp32 numpy model of this solver on spectra that fall to 1e-7 of their top: without the skip n = 512 never converges; with n eps / 2 it takes
    // 21 sweeps and the skipped columns' Rayleigh quotients are within 0.8 n eps of the top eigenvalue (1.8 with n eps, 0.4 with n eps / 4)
    const float skip_rel2 = (0.5f * (float)n * eps) * (0.5f * (float)n * eps);
    hipLaunchKernelGGL(eig_init_kernel, dim3(eg3d_cdiv((int64_t)n * n, 256)), dim3(256), 0, st, a, n, w.wt, w.vt);
    EG3D_LAUNCH_CHECK();
    int sweeps = 0, converged = 0;
    while (sweeps < max_sweeps && !converged) {
        hipLaunchKernelGGL(eig_sweep_begin_kernel, dim3(1), dim3(1024), 0, st, w.wt, n, skip_rel2, w.crit, npairs, w.scalars);
        for (int round = 0; round < m - 1; ++round)
            hipLaunchKernelGGL(eig_round_kernel, dim3(npairs), dim3(64), 0, st, w.wt, w.vt, n, m, round, tol, w.crit, w.scalars);
        hipLaunchKernelGGL(eig_sweep_end_kernel, dim3(1), dim3(64), 0, st, w.crit, npairs, w.scalars);
        EG3D_LAUNCH_CHECK();
        float worst = 0.f;                                                     // the one read-back per sweep: this function synchronises
        hipError_t e = hipMemcpyAsync(&worst, w.scalars + 1, sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        ++sweeps;
        converged = worst <= tol ? 1 : 0;
    }
    hipLaunchKernelGGL(eig_rayleigh_kernel, dim3(n), dim3(64), 0, st, w.wt, w.vt, n, w.lam);
    hipLaunchKernelGGL(eig_rank_kernel, dim3(eg3d_cdiv(n, 256)), dim3(256), 0, st, w.lam, n, w.rank);
    hipLaunchKernelGGL(eig_emit_kernel, dim3(n), dim3(64), 0, st, w.vt, w.lam, w.rank, n, evals, evecs);
    EG3D_LAUNCH_CHECK();
    info[0] = sweeps;
    info[1] = converged;
    return EG3D_OK;
}

extern "C" int eg3d_image_grid_u8(const float* img, int N, int H, int W, int nrow, int padding, int pad_value, uint8_t* out, void* stream) {
    if (!img || !out || N < 1 || H < 1 || W < 1 || nrow < 1 || padding < 0 || pad_value < 0 || pad_value > 255) return EG3D_ERR_INVALID;
    const int xmaps = nrow < N ? nrow : N, ymaps = (N + xmaps - 1) / xmaps;
    const int64_t Ht = (int64_t)ymaps * (H + padding) + padding, Wt = (int64_t)xmaps * (W + padding) + padding;
    if (Ht * Wt * 3 > 0x7fffffffLL || (int64_t)N * 3 * H * W > 0x7fffffffLL) return EG3D_ERR_TOO_LARGE;
    hipLaunchKernelGGL(image_grid_u8_kernel, dim3(eg3d_cdiv(Ht * Wt, 256)), dim3(256), 0, (hipStream_t)stream, img, N, H, W, xmaps, padding, pad_value, (int)Ht, (int)Wt, out);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
