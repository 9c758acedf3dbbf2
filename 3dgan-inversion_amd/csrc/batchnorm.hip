// Training-mode BatchNorm2d on channels-last fp32 [M = N*H*W, C], forward and backward (include/eg3d_hip.h "BatchNorm on batch statistics";
// the pose estimator's training path, inv3d_amd/pose_train.py).
//
// Every pass uses one geometry: a thread owns one channel quad (float4) and walks rows; QB = min(pow2 >= C/4, 64) quads side by side, so a wave
// reads whole contiguous row segments; 256 / QB rows per block iteration; grid = (row chunks, quad groups).
//   forward   bn_stats_kernel      per row chunk: sum (x - s), sum (x - s)^2 per channel about the shift s = x[0, c], accumulated in double
//             bn_finish_fwd_kernel one wave per channel: the chunk partials in a fixed order -> mean, 1/sqrt(var + eps) (double and fp32),
//                                  the running statistics and the batch counter
//             bn_apply_fwd_kernel  y = act(gamma * xhat + beta [+ residual])
//   backward  bn_reduce_bwd_kernel per row chunk: sum dy', sum dy' * xhat (dy' = dy masked by the saved output under ReLU), in double
//             bn_finish_bwd_kernel one wave per channel -> dbeta, dgamma, and the two per-channel coefficients of the apply pass
//             bn_apply_bwd_kernel  dx = gamma * invstd * (dy' - dbeta / M - xhat * dgamma / M) [, dresidual = dy']
// The second moment is never formed as E[x^2] - E[x]^2 in fp32: the sums are double-precision sums of differences from a per-channel shift
// (the cancellation left is that of (x[0,c] - mean)^2 against the variance, a few units, in double).  x - mean is formed in double from the
// double mean and rounded once.  No atomics: partials per workgroup, combined in a fixed order (bit-identical between runs and builds).
#include "common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_PARTS = 1024;
constexpr int BN_UNROLL = 4;

struct BnGeom {
    int64_t M;
    int64_t rows_per_part;
    int32_t C, Q;          // channels, channel quads
    int32_t qb_log2;       // log2 of the quads per block
    int32_t gy;            // quad groups (grid.y)
    int32_t nparts;        // row chunks (grid.x)
};

__host__ BnGeom bn_geom(int64_t M, int C) {
    BnGeom g;
    g.M = M;
    g.C = C;
    g.Q = C / 4;
    int lg = 0;
    while ((1 << lg) < g.Q && lg < 6) ++lg;
    g.qb_log2 = lg;
    const int QB = 1 << lg, rpi = BN_THREADS / QB;
    g.gy = (g.Q + QB - 1) / QB;
    // eight rows or more per thread; at most ~2048 workgroups in all and BN_MAX_PARTS chunks
    int64_t parts = (M + (int64_t)rpi * 8 - 1) / ((int64_t)rpi * 8);
    int64_t cap = 2048 / g.gy;
    if (cap > BN_MAX_PARTS) cap = BN_MAX_PARTS;
    if (cap < 1) cap = 1;
    if (parts > cap) parts = cap;
    if (parts < 1) parts = 1;
    g.rows_per_part = (M + parts - 1) / parts;
    g.nparts = (int)((M + g.rows_per_part - 1) / g.rows_per_part);
    return g;
}

struct BnThread {
    int tx, ty, rpi, cq;
    bool ok;
    int64_t r0, r1;
};

__device__ __forceinline__ BnThread bn_thread(const BnGeom& g) {
    BnThread t;
    const int QB = 1 << g.qb_log2;
    t.tx = threadIdx.x & (QB - 1);
    t.ty = threadIdx.x >> g.qb_log2;
    t.rpi = BN_THREADS >> g.qb_log2;
    t.cq = blockIdx.y * QB + t.tx;
    t.ok = t.cq < g.Q;
    t.r0 = (int64_t)blockIdx.x * g.rows_per_part;
    t.r1 = t.r0 + g.rows_per_part < g.M ? t.r0 + g.rows_per_part : g.M;
    return t;
}

__device__ __forceinline__ void bn_unpack(const float4 v, float* a) {
    a[0] = v.x;
    a[1] = v.y;
    a[2] = v.z;
    a[3] = v.w;
}

// the threads' pairs of sums per channel -> one partial per (row chunk, channel): rows of the block summed in a fixed order
__device__ __forceinline__ void bn_block_partials(const BnGeom& g, const BnThread& t, const double* a, const double* b, double2* sh, double2* __restrict__ part) {
    const int QB = 1 << g.qb_log2;
    for (int k = 0; k < 4; ++k) sh[(t.ty * QB + t.tx) * 4 + k] = make_double2(a[k], b[k]);
    __syncthreads();
    if ((int)threadIdx.x < QB * 4) {
        const int c = blockIdx.y * QB * 4 + threadIdx.x;
        if (c < g.C) {
            double2 s = sh[threadIdx.x];
            for (int j = 1; j < t.rpi; ++j) {
                const double2 v = sh[j * QB * 4 + threadIdx.x];
                s.x += v.x;
                s.y += v.y;
            }
            part[(int64_t)blockIdx.x * g.C + c] = s;
        }
    }
}

// one wave per channel: the chunk partials, lane-strided and then across the lanes, always in the same order
__device__ __forceinline__ double2 bn_wave_total(const double2* __restrict__ part, int nparts, int C, int c) {
    const int lane = threadIdx.x & 63;
    double a = 0.0, b = 0.0;
    for (int p = lane; p < nparts; p += 64) {
        const double2 v = part[(int64_t)p * C + c];
        a += v.x;
        b += v.y;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    return make_double2(a, b);
}

__global__ void __launch_bounds__(BN_THREADS) bn_stats_kernel(const float4* __restrict__ x, BnGeom g, double2* __restrict__ part) {
    __shared__ double2 sh[BN_THREADS * 4];
    const BnThread t = bn_thread(g);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.ok) {
        float sf[4];
        bn_unpack(x[t.cq], sf);
        const double shift[4] = {(double)sf[0], (double)sf[1], (double)sf[2], (double)sf[3]};
        const float4* px = x + t.cq;
        int64_t r = t.r0 + t.ty;
        const int64_t step = t.rpi;
        for (; r + (BN_UNROLL - 1) * step < t.r1; r += BN_UNROLL * step) {
            float4 v[BN_UNROLL];
#pragma unroll
            for (int u = 0; u < BN_UNROLL; ++u) v[u] = px[(r + u * step) * g.Q];
#pragma unroll
            for (int u = 0; u < BN_UNROLL; ++u) {
                float e[4];
                bn_unpack(v[u], e);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double d = (double)e[k] - shift[k];
                    s1[k] += d;
                    s2[k] += d * d;
                }
            }
        }
        for (; r < t.r1; r += step) {
            float e[4];
            bn_unpack(px[r * g.Q], e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)e[k] - shift[k];
                s1[k] += d;
                s2[k] += d * d;
            }
        }
    }
    bn_block_partials(g, t, s1, s2, sh, part);
}

__global__ void __launch_bounds__(BN_THREADS) bn_finish_fwd_kernel(const float* __restrict__ x, const double2* __restrict__ part, BnGeom g, float eps, float momentum,
                                                                   double* __restrict__ stats, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                   float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                   int64_t* __restrict__ num_batches_tracked) {
    const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= g.C) return;                                     // wave-uniform
    const double2 s = bn_wave_total(part, g.nparts, g.C, c);
    if ((threadIdx.x & 63) != 0) return;
    const double M = (double)g.M;
    const double m = s.x / M;
    const double mean = (double)x[c] + m;
    double var = s.y / M - m * m;
    if (!(var > 0.0)) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)eps);
    stats[c] = mean;
    stats[g.C + c] = invstd;
    if (save_mean != nullptr) save_mean[c] = (float)mean;
    if (save_invstd != nullptr) save_invstd[c] = (float)invstd;
    const double mom = (double)momentum;
    if (running_mean != nullptr) running_mean[c] = (float)((1.0 - mom) * (double)running_mean[c] + mom * mean);
    if (running_var != nullptr) running_var[c] = (float)((1.0 - mom) * (double)running_var[c] + mom * (var * M / (M - 1.0)));
    if (num_batches_tracked != nullptr && c == 0) num_batches_tracked[0] += 1;
}

template <bool RELU, bool RES>
__global__ void __launch_bounds__(BN_THREADS) bn_apply_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ res, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const double* __restrict__ stats, BnGeom g,
                                                                  float4* __restrict__ y) {
    const BnThread t = bn_thread(g);
    if (!t.ok) return;
    double mean[4];
    float a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = t.cq * 4 + k;
        mean[k] = stats[c];
        a[k] = (float)((double)gamma[c] * stats[g.C + c]);
        b[k] = beta[c];
    }
    const int64_t step = t.rpi;
    auto one = [&](const float4 xv, const float4 rv) {
        float e[4], q[4], o[4];
        bn_unpack(xv, e);
        bn_unpack(rv, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v = (float)((double)e[k] - mean[k]) * a[k] + b[k];
            if (RES) v += q[k];
            o[k] = RELU ? (v > 0.f ? v : 0.f) : v;
        }
        return make_float4(o[0], o[1], o[2], o[3]);
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t r = t.r0 + t.ty;
    for (; r + (BN_UNROLL - 1) * step < t.r1; r += BN_UNROLL * step) {
        float4 v[BN_UNROLL], q[BN_UNROLL];
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) {
            const int64_t i = (r + u * step) * g.Q + t.cq;
            v[u] = x[i];
            q[u] = RES ? res[i] : zero;
        }
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) y[(r + u * step) * g.Q + t.cq] = one(v[u], q[u]);
    }
    for (; r < t.r1; r += step) {
        const int64_t i = r * g.Q + t.cq;
        y[i] = one(x[i], RES ? res[i] : zero);
    }
}

template <bool RELU>
__global__ void __launch_bounds__(BN_THREADS) bn_reduce_bwd_kernel(const float4* __restrict__ x, const float4* __restrict__ dy, const float4* __restrict__ y,
                                                                   const double* __restrict__ stats, BnGeom g, double2* __restrict__ part) {
    __shared__ double2 sh[BN_THREADS * 4];
    const BnThread t = bn_thread(g);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.ok) {
        double mean[4], invstd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mean[k] = stats[t.cq * 4 + k];
            invstd[k] = stats[g.C + t.cq * 4 + k];
        }
        const int64_t step = t.rpi;
        auto one = [&](const float4 xv, const float4 gv, const float4 yv) {
            float e[4], d[4], o[4];
            bn_unpack(xv, e);
            bn_unpack(gv, d);
            bn_unpack(yv, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double dv = (RELU && !(o[k] > 0.f)) ? 0.0 : (double)d[k];
                s1[k] += dv;
                s2[k] += dv * (((double)e[k] - mean[k]) * invstd[k]);
            }
        };
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t r = t.r0 + t.ty;
        for (; r + (BN_UNROLL - 1) * step < t.r1; r += BN_UNROLL * step) {
            float4 v[BN_UNROLL], d[BN_UNROLL], o[BN_UNROLL];
#pragma unroll
            for (int u = 0; u < BN_UNROLL; ++u) {
                const int64_t i = (r + u * step) * g.Q + t.cq;
                v[u] = x[i];
                d[u] = dy[i];
                o[u] = RELU ? y[i] : zero;
            }
#pragma unroll
            for (int u = 0; u < BN_UNROLL; ++u) one(v[u], d[u], o[u]);
        }
        for (; r < t.r1; r += step) {
            const int64_t i = r * g.Q + t.cq;
            one(x[i], dy[i], RELU ? y[i] : zero);
        }
    }
    bn_block_partials(g, t, s1, s2, sh, part);
}

// coef[c] = dbeta / M, coef[C + c] = dgamma / M
__global__ void __launch_bounds__(BN_THREADS) bn_finish_bwd_kernel(const double2* __restrict__ part, BnGeom g, double* __restrict__ coef, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
    const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= g.C) return;
    const double2 s = bn_wave_total(part, g.nparts, g.C, c);
    if ((threadIdx.x & 63) != 0) return;
    coef[c] = s.x / (double)g.M;
    coef[g.C + c] = s.y / (double)g.M;
    if (dbeta != nullptr) dbeta[c] = (float)s.x;
    if (dgamma != nullptr) dgamma[c] = (float)s.y;
}

template <bool RELU>
__global__ void __launch_bounds__(BN_THREADS) bn_apply_bwd_kernel(const float4* __restrict__ x, const float4* __restrict__ dy, const float4* __restrict__ y,
                                                                  const float* __restrict__ gamma, const double* __restrict__ stats, const double* __restrict__ coef,
                                                                  BnGeom g, float4* __restrict__ dx, float4* __restrict__ dres) {
    const BnThread t = bn_thread(g);
    if (!t.ok) return;
    double mean[4];
    float invstd[4], a[4], c1[4], c2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = t.cq * 4 + k;
        mean[k] = stats[c];
        invstd[k] = (float)stats[g.C + c];
        a[k] = (float)((double)gamma[c] * stats[g.C + c]);
        c1[k] = (float)coef[c];
        c2[k] = (float)coef[g.C + c];
    }
    const int64_t step = t.rpi;
    auto one = [&](const int64_t i, const float4 xv, const float4 gv, const float4 yv) {
        float e[4], d[4], o[4], w[4];
        bn_unpack(xv, e);
        bn_unpack(gv, d);
        bn_unpack(yv, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (RELU && !(o[k] > 0.f)) d[k] = 0.f;
            const float xh = (float)((double)e[k] - mean[k]) * invstd[k];
            w[k] = a[k] * ((d[k] - c1[k]) - xh * c2[k]);
        }
        if (dx != nullptr) dx[i] = make_float4(w[0], w[1], w[2], w[3]);
        if (dres != nullptr) dres[i] = make_float4(d[0], d[1], d[2], d[3]);
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t r = t.r0 + t.ty;
    for (; r + (BN_UNROLL - 1) * step < t.r1; r += BN_UNROLL * step) {
        float4 v[BN_UNROLL], d[BN_UNROLL], o[BN_UNROLL];
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) {
            const int64_t i = (r + u * step) * g.Q + t.cq;
            v[u] = x[i];
            d[u] = dy[i];
            o[u] = RELU ? y[i] : zero;
        }
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) one((r + u * step) * g.Q + t.cq, v[u], d[u], o[u]);
    }
    for (; r < t.r1; r += step) {
        const int64_t i = r * g.Q + t.cq;
        one(i, x[i], dy[i], RELU ? y[i] : zero);
    }
}

bool bn_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int64_t bn_parts_bytes(const BnGeom& g) { return (int64_t)g.nparts * g.C * (int64_t)sizeof(double2); }
int64_t bn_workspace_bytes(const BnGeom& g) { return bn_parts_bytes(g) + 2 * (int64_t)g.C * (int64_t)sizeof(double); }

// the checks every entry shares: sizes, the activation, the tensors both directions read
int bn_check(const eg3d_batchnorm_params* p, BnGeom& g) {
    if (p == nullptr || p->C < 4 || p->C % 4 != 0 || p->M < 2) return EG3D_ERR_INVALID;
    if (p->act != EG3D_ACT_LINEAR && p->act != EG3D_ACT_RELU) return EG3D_ERR_UNSUPPORTED;
    if (p->C > (1 << 20) || p->M > ((int64_t)1 << 40)) return EG3D_ERR_TOO_LARGE;
    g = bn_geom(p->M, p->C);
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_batchnorm_query_workspace(int64_t M, int32_t C, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr || C < 4 || C % 4 != 0 || M < 2) return EG3D_ERR_INVALID;
    if (C > (1 << 20) || M > ((int64_t)1 << 40)) return EG3D_ERR_TOO_LARGE;
    *workspace_bytes = bn_workspace_bytes(bn_geom(M, C));
    return EG3D_OK;
}

extern "C" int eg3d_batchnorm_forward(const eg3d_batchnorm_params* p, void* stream) {
    BnGeom g;
    const int s = bn_check(p, g);
    if (s != EG3D_OK) return s;
    if (p->x == nullptr || p->gamma == nullptr || p->beta == nullptr || p->y == nullptr || p->stats == nullptr || p->workspace == nullptr) return EG3D_ERR_INVALID;
    if (bn_misaligned(p->x, 16) || bn_misaligned(p->y, 16) || bn_misaligned(p->residual, 16) || bn_misaligned(p->workspace, 16) || bn_misaligned(p->stats, 8) ||
        bn_misaligned(p->num_batches_tracked, 8))
        return EG3D_ERR_INVALID;
    if (p->workspace_bytes < bn_parts_bytes(g) || !(p->eps >= 0.f) || !(p->momentum >= 0.f && p->momentum <= 1.f)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    double2* part = reinterpret_cast<double2*>(p->workspace);
    const float4* x = reinterpret_cast<const float4*>(p->x);
    const float4* res = reinterpret_cast<const float4*>(p->residual);
    float4* y = reinterpret_cast<float4*>(p->y);
    const dim3 grid(g.nparts, g.gy), block(BN_THREADS);
    hipLaunchKernelGGL(bn_stats_kernel, grid, block, 0, st, x, g, part);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_finish_fwd_kernel, dim3((g.C + 3) / 4), block, 0, st, p->x, part, g, p->eps, p->momentum, p->stats, p->save_mean, p->save_invstd,
                       p->running_mean, p->running_var, p->num_batches_tracked);
    EG3D_LAUNCH_CHECK();
    const bool relu = p->act == EG3D_ACT_RELU;
    if (res != nullptr) {
        if (relu) hipLaunchKernelGGL((bn_apply_fwd_kernel<true, true>), grid, block, 0, st, x, res, p->gamma, p->beta, p->stats, g, y);
        else hipLaunchKernelGGL((bn_apply_fwd_kernel<false, true>), grid, block, 0, st, x, res, p->gamma, p->beta, p->stats, g, y);
    } else {
        if (relu) hipLaunchKernelGGL((bn_apply_fwd_kernel<true, false>), grid, block, 0, st, x, res, p->gamma, p->beta, p->stats, g, y);
        else hipLaunchKernelGGL((bn_apply_fwd_kernel<false, false>), grid, block, 0, st, x, res, p->gamma, p->beta, p->stats, g, y);
    }
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_batchnorm_backward(const eg3d_batchnorm_params* p, void* stream) {
    BnGeom g;
    const int s = bn_check(p, g);
    if (s != EG3D_OK) return s;
    const bool relu = p->act == EG3D_ACT_RELU;
    if (p->x == nullptr || p->gamma == nullptr || p->dy == nullptr || p->stats == nullptr || p->workspace == nullptr || (relu && p->y == nullptr)) return EG3D_ERR_INVALID;
    if (bn_misaligned(p->x, 16) || bn_misaligned(p->y, 16) || bn_misaligned(p->dy, 16) || bn_misaligned(p->dx, 16) || bn_misaligned(p->dresidual, 16) ||
        bn_misaligned(p->workspace, 16) || bn_misaligned(p->stats, 8))
        return EG3D_ERR_INVALID;
    if (p->workspace_bytes < bn_workspace_bytes(g)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    double2* part = reinterpret_cast<double2*>(p->workspace);
    double* coef = reinterpret_cast<double*>(reinterpret_cast<char*>(p->workspace) + bn_parts_bytes(g));
    const float4* x = reinterpret_cast<const float4*>(p->x);
    const float4* dy = reinterpret_cast<const float4*>(p->dy);
    const float4* y = reinterpret_cast<const float4*>(p->y);
    float4* dx = reinterpret_cast<float4*>(p->dx);
    float4* dres = reinterpret_cast<float4*>(p->dresidual);
    const dim3 grid(g.nparts, g.gy), block(BN_THREADS);
    if (relu) hipLaunchKernelGGL(bn_reduce_bwd_kernel<true>, grid, block, 0, st, x, dy, y, p->stats, g, part);
    else hipLaunchKernelGGL(bn_reduce_bwd_kernel<false>, grid, block, 0, st, x, dy, y, p->stats, g, part);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_finish_bwd_kernel, dim3((g.C + 3) / 4), block, 0, st, part, g, coef, p->dgamma, p->dbeta);
    EG3D_LAUNCH_CHECK();
    if (dx == nullptr && dres == nullptr) return EG3D_OK;
    if (relu) hipLaunchKernelGGL(bn_apply_bwd_kernel<true>, grid, block, 0, st, x, dy, y, p->gamma, p->stats, coef, g, dx, dres);
    else hipLaunchKernelGGL(bn_apply_bwd_kernel<false>, grid, block, 0, st, x, dy, y, p->gamma, p->stats, coef, g, dx, dres);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
