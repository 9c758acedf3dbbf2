// SSIM / MS-SSIM forward and backward, and the face crop + pool of the identity metric (reconstruction metrics of the reference's evaluation,
// include/eg3d_hip.h "SSIM / MS-SSIM").
//
// Every pass works on 32 x 32 output tiles of one (image, channel) plane with the separable window applied through LDS: the tile's input
// (32 + win - 1)^2 is staged, blurred along W into LDS, then along H in registers (thread = 1 column x 4 rows).
//   forward, per level   ssim_fwd_kernel     the five moments, the ssim / cs maps summed per workgroup (double) -> partials; the same
//                                            workgroup writes a 16 x 16 tile of the next level's pooled x and y
//   forward, once        ssim_finish_kernel  one workgroup: the partials summed per plane and level in a fixed order -> stats, out
//   backward, per level  ssim_maps_kernel    the moments again; d(out)/d(mu_x, mu_y, E[x^2] = E[y^2] coefficient, E[xy]) per output pixel
//                        ssim_grad_kernel    the transposed (full) window on those four maps, the element-wise products with x and y, plus
//                                            the next coarser level's gradient through the pool adjoint
// The second moments are formed about a per-plane constant shift (the plane's centre pixel of that level): s_xx = G*((x-c)^2) - (G*(x-c))^2
// is exact in real arithmetic for any constant c and keeps the cancellation to the local contrast.  The backward uses the same shift, which
// it must: its products with (x - c) pair with the forward's means about the same c.
// No atomics: the output is a function of the input (bit-identical between runs and between the two builds).
#include "common.h"

namespace {

constexpr int SS_T = 32;                                   // output tile side
constexpr int SS_THREADS = 256;
constexpr int SS_ROWS = 4;                                 // output rows per thread in the vertical pass (8 row groups x 32 columns)
constexpr int SS_IN = SS_T + EG3D_SSIM_MAX_WIN - 1;        // staged tile side (row pitch of the LDS arrays)
constexpr int SS_PT = SS_T / 2;                            // pooled tile side written by one forward workgroup

struct SsWin {
    float g[EG3D_SSIM_MAX_WIN];
    int n;
};

struct SsLevel {
    int32_t H, W, Ho, Wo;          // image, valid output
    int32_t Hn, Wn, ph, pw;        // pooled next level (0 at the last level), pool padding
    int32_t ty, tx;                // forward tile grid
    int64_t part_off;              // offset of this level's partials (double2 units), plane-major
    int64_t pyr_off;               // offset of this level's x in the pyramid (levels >= 1); y follows after N*C*H*W floats
};

struct SsGeom {
    int NC, L;
    SsLevel lv[EG3D_SSIM_MAX_LEVELS];
    int64_t parts, pyr_floats, maps_floats;
};

__device__ __forceinline__ double2 ss_block_sum(double a, double b, double2* sh) {
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = make_double2(a, b);
    __syncthreads();
    double2 r = sh[0];
    for (int i = 1; i < SS_THREADS / 64; ++i) {
        r.x += sh[i].x;
        r.y += sh[i].y;
    }
    return r;
}

// Stage Q planes of a tile whose origin is (r0, c0) (may be negative) from `src[q]` (H x W, or float4-interleaved when Q == 4 and `f4`),
// zero outside [0,H) x [0,W), minus shift[q]; then the W-direction blur into hb.  in: [Q][SS_IN * SS_IN], hb: [QH][SS_IN * SS_T].
// Returns after a barrier; hb holds rows 0 .. T+win-2 of the tile blurred along W.
template <int Q>
__device__ __forceinline__ void ss_stage(const float* const* src, const float4* src4, int H, int W, int r0, int c0, const float* shift, const SsWin& win,
                                         float (*in)[SS_IN * SS_IN]) {
    const int n = SS_T + win.n - 1;
    for (int i = threadIdx.x; i < n * n; i += SS_THREADS) {
        const int rr = i / n, cc = i - rr * n;
        const int gr = r0 + rr, gc = c0 + cc;
        const bool ok = gr >= 0 && gr < H && gc >= 0 && gc < W;
        if (src4 != nullptr) {
            const float4 v = ok ? src4[(int64_t)gr * W + gc] : make_float4(0.f, 0.f, 0.f, 0.f);
            in[0][rr * SS_IN + cc] = v.x;
            in[1][rr * SS_IN + cc] = v.y;
            in[2][rr * SS_IN + cc] = v.z;
            in[3][rr * SS_IN + cc] = v.w;
        } else {
            for (int q = 0; q < Q; ++q) in[q][rr * SS_IN + cc] = ok ? src[q][(int64_t)gr * W + gc] - shift[q] : 0.f;
        }
    }
    __syncthreads();
}

// the five W-blurred moments of the shifted x (in[0]) and y (in[1]): x, y, x^2, y^2, xy
__device__ __forceinline__ void ss_hblur_moments(const float (*in)[SS_IN * SS_IN], float (*hb)[SS_IN * SS_T], const SsWin& win) {
    const int n = SS_T + win.n - 1;
    for (int i = threadIdx.x; i < n * SS_T; i += SS_THREADS) {
        const int rr = i / SS_T, cc = i - rr * SS_T;
        float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < win.n; ++k) {
            const float a = in[0][rr * SS_IN + cc + k], b = in[1][rr * SS_IN + cc + k], g = win.g[k];
            s[0] += g * a;
            s[1] += g * b;
            s[2] += g * (a * a);
            s[3] += g * (b * b);
            s[4] += g * (a * b);
        }
        for (int q = 0; q < 5; ++q) hb[q][rr * SS_T + cc] = s[q];
    }
    __syncthreads();
}

// H-direction blur of QH planes of hb for this thread's column and SS_ROWS rows: v[j][q]
template <int QH>
__device__ __forceinline__ void ss_vblur(const float (*hb)[SS_IN * SS_T], const SsWin& win, int row0, int col, float (*v)[QH]) {
    for (int j = 0; j < SS_ROWS; ++j)
        for (int q = 0; q < QH; ++q) v[j][q] = 0.f;
    for (int k = 0; k < win.n; ++k) {
        const float g = win.g[k];
        for (int j = 0; j < SS_ROWS; ++j)
            for (int q = 0; q < QH; ++q) v[j][q] += g * hb[q][(row0 + j + k) * SS_T + col];
    }
}

struct SsPix {
    float mx, my, A, B, D1, D2, l, cs;
};

__device__ __forceinline__ SsPix ss_pixel(const float* m, float cx, float cy, float C1, float C2) {
    SsPix p;
    p.mx = m[0];
    p.my = m[1];
    const float sxx = m[2] - p.mx * p.mx, syy = m[3] - p.my * p.my, sxy = m[4] - p.mx * p.my;
    p.A = cx + p.mx;
    p.B = cy + p.my;
    p.D2 = sxx + syy + C2;
    p.cs = (2.f * sxy + C2) / p.D2;
    p.D1 = p.A * p.A + p.B * p.B + C1;
    p.l = (2.f * p.A * p.B + C1) / p.D1;
    return p;
}

__device__ __forceinline__ float ss_centre(const float* plane, int H, int W) { return plane[(int64_t)(H / 2) * W + W / 2]; }

__global__ void __launch_bounds__(SS_THREADS) ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, SsLevel lv, SsWin win, float C1,
                                                              float C2, double2* __restrict__ part, float* __restrict__ xn, float* __restrict__ yn) {
    __shared__ float in[2][SS_IN * SS_IN];
    __shared__ float hb[5][SS_IN * SS_T];
    __shared__ double2 red[SS_THREADS / 64];
    const int plane = blockIdx.z;
    const int64_t HW = (int64_t)lv.H * lv.W;
    const float* xp = x + plane * HW;
    const float* yp = y + plane * HW;
    const int r0 = blockIdx.y * SS_T, c0 = blockIdx.x * SS_T;
    double as = 0.0, ac = 0.0;
    if (r0 < lv.Ho && c0 < lv.Wo) {                          // workgroup-uniform
        const float shift[2] = {ss_centre(xp, lv.H, lv.W), ss_centre(yp, lv.H, lv.W)};
        const float* src[2] = {xp, yp};
        ss_stage<2>(src, nullptr, lv.H, lv.W, r0, c0, shift, win, in);
        ss_hblur_moments(in, hb, win);
        const int col = threadIdx.x & (SS_T - 1), row0 = (threadIdx.x / SS_T) * SS_ROWS;
        float v[SS_ROWS][5];
        ss_vblur<5>(hb, win, row0, col, v);
        for (int j = 0; j < SS_ROWS; ++j) {
            if (r0 + row0 + j < lv.Ho && c0 + col < lv.Wo) {
                const SsPix p = ss_pixel(v[j], shift[0], shift[1], C1, C2);
                as += (double)(p.l * p.cs);
                ac += (double)p.cs;
            }
        }
    }
    const double2 s = ss_block_sum(as, ac, red);
    if (threadIdx.x == 0) part[(int64_t)plane * lv.ty * lv.tx + blockIdx.y * lv.tx + blockIdx.x] = s;
    if (xn != nullptr) {                                     // avg_pool2d(2, 2, padding (ph, pw), count_include_pad): divisor 4
        const int pi = blockIdx.y * SS_PT + (int)(threadIdx.x / SS_PT), pj = blockIdx.x * SS_PT + (int)(threadIdx.x % SS_PT);
        if (pi < lv.Hn && pj < lv.Wn) {
            const int ra = 2 * pi - lv.ph, ca = 2 * pj - lv.pw;
            float sx = 0.f, sy = 0.f;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int r = ra + a, c = ca + b;
                    if (r >= 0 && r < lv.H && c >= 0 && c < lv.W) {
                        sx += xp[(int64_t)r * lv.W + c];
                        sy += yp[(int64_t)r * lv.W + c];
                    }
                }
            const int64_t o = (int64_t)plane * lv.Hn * lv.Wn + (int64_t)pi * lv.Wn + pj;
            xn[o] = sx * 0.25f;
            yn[o] = sy * 0.25f;
        }
    }
}

struct SsReduce {
    int N, C, mode, nonnegative, size_average;
    float w[EG3D_SSIM_MAX_LEVELS];
};

__global__ void __launch_bounds__(SS_THREADS) ssim_finish_kernel(const double2* __restrict__ part, SsGeom g, SsReduce rd, double* __restrict__ stats,
                                                                 float* __restrict__ out) {
    const int L = g.L;
    for (int plane = threadIdx.x; plane < g.NC; plane += SS_THREADS) {
        double V = 1.0, m = 0.0;
        for (int l = 0; l < L; ++l) {
            const SsLevel& lv = g.lv[l];
            const int nt = lv.ty * lv.tx;
            const double2* pp = part + lv.part_off + (int64_t)plane * nt;
            double ss = 0.0, cs = 0.0;
            for (int t = 0; t < nt; ++t) {
                ss += pp[t].x;
                cs += pp[t].y;
            }
            const double P = (double)lv.Ho * (double)lv.Wo;
            m = (l < L - 1 ? cs : ss) / P;
            stats[(int64_t)plane * (L + 1) + l] = m;
            if (rd.mode == 1) V *= pow(fmax(m, 0.0), (double)rd.w[l]);
        }
        if (rd.mode == 0) V = rd.nonnegative ? fmax(m, 0.0) : m;
        stats[(int64_t)plane * (L + 1) + L] = V;
    }
    __syncthreads();
    if (rd.size_average) {
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int plane = 0; plane < g.NC; ++plane) s += stats[(int64_t)plane * (L + 1) + L];
            out[0] = (float)(s / (double)g.NC);
        }
    } else {
        for (int n = threadIdx.x; n < rd.N; n += SS_THREADS) {
            double s = 0.0;
            for (int c = 0; c < rd.C; ++c) s += stats[((int64_t)n * rd.C + c) * (L + 1) + L];
            out[n] = (float)(s / (double)rd.C);
        }
    }
}

// d out / d m_l for this plane, divided by the level's pixel count: the per-pixel weight of the level's mean map
__device__ __forceinline__ double ss_level_weight(const double* st, int l, int L, const SsReduce& rd, double gv, double P) {
    const double m = st[l];
    if (!(m > 0.0) && (rd.mode == 1 || rd.nonnegative)) return 0.0;    // relu: a clamped term (or a zero one) passes no gradient
    double d = 1.0;
    if (rd.mode == 1) {
        d = (double)rd.w[l] * pow(m, (double)rd.w[l] - 1.0);
        for (int k = 0; k < L; ++k)
            if (k != l) d *= pow(fmax(st[k], 0.0), (double)rd.w[k]);
    }
    return gv * d / P;
}

__global__ void __launch_bounds__(SS_THREADS) ssim_maps_kernel(const float* __restrict__ x, const float* __restrict__ y, SsLevel lv, int l, int L, SsWin win,
                                                               float C1, float C2, SsReduce rd, const double* __restrict__ stats,
                                                               const float* __restrict__ gout, float4* __restrict__ maps) {
    __shared__ float in[2][SS_IN * SS_IN];
    __shared__ float hb[5][SS_IN * SS_T];
    const int plane = blockIdx.z;
    const int64_t HW = (int64_t)lv.H * lv.W;
    const float* xp = x + plane * HW;
    const float* yp = y + plane * HW;
    const int r0 = blockIdx.y * SS_T, c0 = blockIdx.x * SS_T;
    const double gv = rd.size_average ? (double)gout[0] / ((double)rd.N * rd.C) : (double)gout[plane / rd.C] / (double)rd.C;
    const float s = (float)ss_level_weight(stats + (int64_t)plane * (L + 1), l, L, rd, gv, (double)lv.Ho * (double)lv.Wo);
    const bool last = l == L - 1;
    const float shift[2] = {ss_centre(xp, lv.H, lv.W), ss_centre(yp, lv.H, lv.W)};
    const float* src[2] = {xp, yp};
    ss_stage<2>(src, nullptr, lv.H, lv.W, r0, c0, shift, win, in);
    ss_hblur_moments(in, hb, win);
    const int col = threadIdx.x & (SS_T - 1), row0 = (threadIdx.x / SS_T) * SS_ROWS;
    float v[SS_ROWS][5];
    ss_vblur<5>(hb, win, row0, col, v);
    float4* mp = maps + (int64_t)plane * lv.Ho * lv.Wo;
    for (int j = 0; j < SS_ROWS; ++j) {
        const int r = r0 + row0 + j, c = c0 + col;
        if (r < lv.Ho && c < lv.Wo) {
            const SsPix p = ss_pixel(v[j], shift[0], shift[1], C1, C2);
            // cs = (2 s_xy + C2) / D2 with s_xx = E'xx - mx^2, s_xy = E'xy - mx my (shifted moments): d cs / d mx = (2 mx cs - 2 my) / D2,
            // d cs / d E'xx = d cs / d E'yy = -cs / D2, d cs / d E'xy = 2 / D2; the luminance term l = (2AB + C1) / D1: d l / d A = 2 (B - l A) / D1
            const float dA = (2.f * p.mx * p.cs - 2.f * p.my) / p.D2, dB = (2.f * p.my * p.cs - 2.f * p.mx) / p.D2;
            float4 o;
            if (last) {
                o.x = s * (p.l * dA + p.cs * (2.f * (p.B - p.l * p.A) / p.D1));
                o.y = s * (p.l * dB + p.cs * (2.f * (p.A - p.l * p.B) / p.D1));
                o.z = -s * p.l * p.cs / p.D2;
                o.w = 2.f * s * p.l / p.D2;
            } else {
                o.x = s * dA;
                o.y = s * dB;
                o.z = -s * p.cs / p.D2;
                o.w = 2.f * s / p.D2;
            }
            mp[(int64_t)r * lv.Wo + c] = o;
        }
    }
}

// gx[r,c] = G^T mA + 2 (x - cx) G^T mXX + (y - cy) G^T mXY (+ the coarser level's gradient / 4 through the pool); gy likewise
__global__ void __launch_bounds__(SS_THREADS) ssim_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, SsLevel lv, SsWin win,
                                                               const float4* __restrict__ maps, const float* __restrict__ gxn, const float* __restrict__ gyn,
                                                               float* __restrict__ gx, float* __restrict__ gy) {
    __shared__ float in[4][SS_IN * SS_IN];
    __shared__ float hb[4][SS_IN * SS_T];
    const int plane = blockIdx.z;
    const int64_t HW = (int64_t)lv.H * lv.W;
    const float* xp = x + plane * HW;
    const float* yp = y + plane * HW;
    const int r0 = blockIdx.y * SS_T, c0 = blockIdx.x * SS_T;
    const int h = win.n - 1;
    ss_stage<4>(nullptr, maps + (int64_t)plane * lv.Ho * lv.Wo, lv.Ho, lv.Wo, r0 - h, c0 - h, nullptr, win, in);
    const int n = SS_T + h;
    for (int i = threadIdx.x; i < n * SS_T; i += SS_THREADS) {
        const int rr = i / SS_T, cc = i - rr * SS_T;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < win.n; ++k) {
            const float g = win.g[k];
            for (int q = 0; q < 4; ++q) s[q] += g * in[q][rr * SS_IN + cc + k];
        }
        for (int q = 0; q < 4; ++q) hb[q][rr * SS_T + cc] = s[q];
    }
    __syncthreads();
    const int col = threadIdx.x & (SS_T - 1), row0 = (threadIdx.x / SS_T) * SS_ROWS;
    float v[SS_ROWS][4];
    ss_vblur<4>(hb, win, row0, col, v);
    const float cx = ss_centre(xp, lv.H, lv.W), cy = ss_centre(yp, lv.H, lv.W);
    for (int j = 0; j < SS_ROWS; ++j) {
        const int r = r0 + row0 + j, c = c0 + col;
        if (r >= lv.H || c >= lv.W) continue;
        const int64_t o = (int64_t)r * lv.W + c;
        const float xv = xp[o] - cx, yv = yp[o] - cy;
        const int64_t on = gxn != nullptr || gyn != nullptr ? (int64_t)plane * lv.Hn * lv.Wn + (int64_t)((r + lv.ph) >> 1) * lv.Wn + ((c + lv.pw) >> 1) : 0;
        if (gx != nullptr) {
            float d = v[j][0] + 2.f * xv * v[j][2] + yv * v[j][3];
            if (gxn != nullptr) d += 0.25f * gxn[on];
            gx[plane * HW + o] = d;
        }
        if (gy != nullptr) {
            float d = v[j][1] + 2.f * yv * v[j][2] + xv * v[j][3];
            if (gyn != nullptr) d += 0.25f * gyn[on];
            gy[plane * HW + o] = d;
        }
    }
}

__global__ void __launch_bounds__(256) face_pool_kernel(const float* __restrict__ x, int N, int H, int W, int r0, int c0, int Hc, int Wc, int S,
                                                        float4* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)N * S * S) return;
    const int j = (int)(t % S), i = (int)((t / S) % S), n = (int)(t / ((int64_t)S * S));
    const int ra = r0 + (i * Hc) / S, rb = r0 + ((i + 1) * Hc + S - 1) / S;
    const int ca = c0 + (j * Wc) / S, cb = c0 + ((j + 1) * Wc + S - 1) / S;
    float s[3] = {0.f, 0.f, 0.f};
    for (int ch = 0; ch < 3; ++ch) {
        const float* p = x + ((int64_t)n * 3 + ch) * H * W;
        for (int r = ra; r < rb; ++r)
            for (int c = ca; c < cb; ++c) s[ch] += p[(int64_t)r * W + c];
    }
    const float k = (float)((rb - ra) * (cb - ca));
    out[t] = make_float4(s[0] / k, s[1] / k, s[2] / k, 0.f);
}

// validates the request; fills the level geometry and the window
int ss_geom(const eg3d_ssim_params* p, SsGeom& g, SsWin& win) {
    if (p == nullptr || p->N < 1 || p->C < 1 || p->H < 1 || p->W < 1) return EG3D_ERR_INVALID;
    if (p->mode != 0 && p->mode != 1) return EG3D_ERR_INVALID;
    if (p->levels < 1 || p->levels > EG3D_SSIM_MAX_LEVELS || (p->mode == 0 && p->levels != 1)) return EG3D_ERR_INVALID;
    if (p->win_size < 1 || p->win_size > EG3D_SSIM_MAX_WIN || p->win_size % 2 == 0 || !(p->win_sigma > 0.f)) return EG3D_ERR_INVALID;
    if ((int64_t)p->N * p->C > 65535) return EG3D_ERR_TOO_LARGE;                        // planes ride on grid.z
    if ((int64_t)p->N * p->C * p->H * p->W > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.NC = p->N * p->C;
    g.L = p->levels;
    int H = p->H, W = p->W;
    int64_t parts = 0, pyr = 0;
    g.maps_floats = 0;
    for (int l = 0; l < g.L; ++l) {
        SsLevel& lv = g.lv[l];
        lv.H = H;
        lv.W = W;
        lv.Ho = H - p->win_size + 1;
        lv.Wo = W - p->win_size + 1;
        if (lv.Ho < 1 || lv.Wo < 1) return EG3D_ERR_INVALID;
        const bool pool = l < g.L - 1;
        lv.ph = pool ? H % 2 : 0;
        lv.pw = pool ? W % 2 : 0;
        lv.Hn = pool ? (H + 2 * lv.ph - 2) / 2 + 1 : 0;
        lv.Wn = pool ? (W + 2 * lv.pw - 2) / 2 + 1 : 0;
        lv.ty = (lv.Ho + SS_T - 1) / SS_T;
        lv.tx = (lv.Wo + SS_T - 1) / SS_T;
        if (pool) {
            lv.ty = lv.ty > (lv.Hn + SS_PT - 1) / SS_PT ? lv.ty : (lv.Hn + SS_PT - 1) / SS_PT;
            lv.tx = lv.tx > (lv.Wn + SS_PT - 1) / SS_PT ? lv.tx : (lv.Wn + SS_PT - 1) / SS_PT;
        }
        lv.part_off = parts;
        parts += (int64_t)g.NC * lv.ty * lv.tx;
        lv.pyr_off = pyr;
        if (l > 0) pyr += 2 * (int64_t)g.NC * H * W;
        const int64_t mf = 4 * (int64_t)g.NC * lv.Ho * lv.Wo;
        if (mf > g.maps_floats) g.maps_floats = mf;
        H = lv.Hn;
        W = lv.Wn;
    }
    g.parts = parts;
    g.pyr_floats = pyr;
    // the window exactly as pytorch_msssim's _fspecial_gauss_1d forms it in fp32 (arange - size // 2, exp, normalise)
    win.n = p->win_size;
    float sum = 0.f;
    for (int k = 0; k < win.n; ++k) {
        const float d = (float)(k - win.n / 2);
        win.g[k] = expf(-(d * d) / (2.f * p->win_sigma * p->win_sigma));
        sum += win.g[k];
    }
    for (int k = 0; k < win.n; ++k) win.g[k] /= sum;
    for (int k = win.n; k < EG3D_SSIM_MAX_WIN; ++k) win.g[k] = 0.f;
    return EG3D_OK;
}

constexpr int64_t SS_ALIGN = 256;
int64_t ss_align(int64_t b) { return (b + SS_ALIGN - 1) / SS_ALIGN * SS_ALIGN; }
int64_t ss_bwd_bytes(const SsGeom& g) { return ss_align(g.maps_floats * 4) + ss_align(g.pyr_floats * 4); }

SsReduce ss_reduce(const eg3d_ssim_params* p) {
    SsReduce rd;
    rd.N = p->N;
    rd.C = p->C;
    rd.mode = p->mode;
    rd.nonnegative = p->nonnegative;
    rd.size_average = p->size_average;
    for (int l = 0; l < EG3D_SSIM_MAX_LEVELS; ++l) rd.w[l] = p->weights[l];
    return rd;
}

const float* ss_level_x(const eg3d_ssim_params* p, const SsGeom& g, int l) { return l == 0 ? p->x : p->pyramid + g.lv[l].pyr_off; }
const float* ss_level_y(const eg3d_ssim_params* p, const SsGeom& g, int l) {
    return l == 0 ? p->y : p->pyramid + g.lv[l].pyr_off + (int64_t)g.NC * g.lv[l].H * g.lv[l].W;
}

}  // namespace

extern "C" int eg3d_ssim_query_workspace(const eg3d_ssim_params* p, int64_t* pyramid_floats, int64_t* stats_doubles, int64_t* forward_bytes,
                                         int64_t* backward_bytes) {
    if (pyramid_floats == nullptr || stats_doubles == nullptr || forward_bytes == nullptr || backward_bytes == nullptr) return EG3D_ERR_INVALID;
    SsGeom g;
    SsWin win;
    const int s = ss_geom(p, g, win);
    if (s != EG3D_OK) return s;
    *pyramid_floats = g.pyr_floats;
    *stats_doubles = (int64_t)g.NC * (g.L + 1);
    *forward_bytes = ss_align(g.parts * (int64_t)sizeof(double2));
    *backward_bytes = ss_bwd_bytes(g);
    return EG3D_OK;
}

extern "C" int eg3d_ssim_forward(const eg3d_ssim_params* p, void* stream) {
    SsGeom g;
    SsWin win;
    const int s = ss_geom(p, g, win);
    if (s != EG3D_OK) return s;
    if (p->x == nullptr || p->y == nullptr || p->stats == nullptr || p->out == nullptr || p->workspace == nullptr) return EG3D_ERR_INVALID;
    if ((g.pyr_floats > 0 && p->pyramid == nullptr) || p->workspace_bytes < g.parts * (int64_t)sizeof(double2)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    double2* part = reinterpret_cast<double2*>(p->workspace);
    for (int l = 0; l < g.L; ++l) {
        const SsLevel& lv = g.lv[l];
        const bool pool = l < g.L - 1;
        float* xn = pool ? p->pyramid + g.lv[l + 1].pyr_off : nullptr;
        float* yn = pool ? xn + (int64_t)g.NC * lv.Hn * lv.Wn : nullptr;
        hipLaunchKernelGGL(ssim_fwd_kernel, dim3(lv.tx, lv.ty, g.NC), dim3(SS_THREADS), 0, st, ss_level_x(p, g, l), ss_level_y(p, g, l), lv, win, p->C1,
                           p->C2, part + lv.part_off, xn, yn);
        EG3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(SS_THREADS), 0, st, part, g, ss_reduce(p), p->stats, p->out);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_ssim_backward(const eg3d_ssim_params* p, void* stream) {
    SsGeom g;
    SsWin win;
    const int s = ss_geom(p, g, win);
    if (s != EG3D_OK) return s;
    if (p->x == nullptr || p->y == nullptr || p->stats == nullptr || p->grad_out == nullptr || p->workspace == nullptr) return EG3D_ERR_INVALID;
    if ((g.pyr_floats > 0 && p->pyramid == nullptr) || p->workspace_bytes < ss_bwd_bytes(g)) return EG3D_ERR_INVALID;
    if (p->grad_x == nullptr && p->grad_y == nullptr) return EG3D_OK;
    hipStream_t st = (hipStream_t)stream;
    float4* maps = reinterpret_cast<float4*>(p->workspace);
    float* gpyr = reinterpret_cast<float*>(reinterpret_cast<char*>(p->workspace) + ss_align(g.maps_floats * 4));   // level gradients, pyramid layout
    const SsReduce rd = ss_reduce(p);
    for (int l = g.L - 1; l >= 0; --l) {
        const SsLevel& lv = g.lv[l];
        const float* xl = ss_level_x(p, g, l);
        const float* yl = ss_level_y(p, g, l);
        hipLaunchKernelGGL(ssim_maps_kernel, dim3((lv.Wo + SS_T - 1) / SS_T, (lv.Ho + SS_T - 1) / SS_T, g.NC), dim3(SS_THREADS), 0, st, xl, yl, lv, l, g.L,
                           win, p->C1, p->C2, rd, p->stats, p->grad_out, maps);
        EG3D_LAUNCH_CHECK();
        const int64_t planes = (int64_t)g.NC * lv.H * lv.W;
        float* gx = p->grad_x == nullptr ? nullptr : (l == 0 ? p->grad_x : gpyr + lv.pyr_off);
        float* gy = p->grad_y == nullptr ? nullptr : (l == 0 ? p->grad_y : gpyr + lv.pyr_off + planes);
        const float* gxn = nullptr;
        const float* gyn = nullptr;
        if (l < g.L - 1) {
            const int64_t nplanes = (int64_t)g.NC * lv.Hn * lv.Wn;
            if (gx != nullptr) gxn = gpyr + g.lv[l + 1].pyr_off;
            if (gy != nullptr) gyn = gpyr + g.lv[l + 1].pyr_off + nplanes;
        }
        hipLaunchKernelGGL(ssim_grad_kernel, dim3((lv.W + SS_T - 1) / SS_T, (lv.H + SS_T - 1) / SS_T, g.NC), dim3(SS_THREADS), 0, st, xl, yl, lv, win, maps,
                           gxn, gyn, gx, gy);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_face_pool(const float* x, int N, int H, int W, int r0, int r1, int c0, int c1, int S, float* out, void* stream) {
    if (x == nullptr || out == nullptr || N < 1 || S < 1 || r0 < 0 || c0 < 0 || r1 > H || c1 > W || r1 <= r0 || c1 <= c0) return EG3D_ERR_INVALID;
    if ((int64_t)N * 3 * H * W > INT32_MAX || (int64_t)N * S * S > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    const int64_t n = (int64_t)N * S * S;
    hipLaunchKernelGGL(face_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, r0, c0, r1 - r0, c1 - c0, S,
                       reinterpret_cast<float4*>(out));
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
