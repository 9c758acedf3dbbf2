// Multi-band paste-back (include/eg3d_hip.h eg3d_paste_blend8): the edit's difference to the photograph blended through a Laplacian pyramid
// (Burt-Adelson) instead of one alpha -- the coarse bands of the difference get a wide transition, the detail a narrow one.  No reference
// counterpart: the reference's alignment goes one way only.
//
//   blend_sample          level 0 of one window pixel: eg3d_paste_back8's fp64 steps (csrc/imgprep.hip paste_back_kernel: the same taps and
//                         order) up to val and a, then D_c = (float)(val_c - photo_c), alpha = (float)a.  ONE function for the two kernels
//                         that need level 0, so both see the same bits
//   blend_level1_kernel   level 0 fused with the first reduce: a workgroup samples the (2 * 32 + 3) x (2 * 16 + 3) level-0 pixels under its
//                         32 x 16 level-1 outputs into LDS (C planes of D and one of alpha; zeros outside the window) and writes level 1
//                         only -- level 0 never reaches memory
//   blend_reduce_kernel   level k -> k + 1 for k >= 1 (a quarter of the pixels and less): one thread per output pixel, its planes in a loop
//   blend_collapse_kernel R_k = (D_k - E(D_k+1)) alpha_k + E(R_k+1) for k >= 1; at k = L - 1 the taps of R_L are D_L alpha_L on the fly; a thread
//                         owns 2 x 2 pixels as in blend_compose_kernel
//   blend_compose_kernel  level 0 again: a thread owns a 2 x 2 block of window pixels, which share one 3 x 3 level-1 neighbourhood (so the
//                         parity of the expand is fixed per pixel: no divergence, a quarter of the loads), samples D_0 / alpha_0 once more,
//                         adds R_0 to the photo, rounds and writes uint8 -- HWC or planar, into the photo copy or the bounding box alone
//
// fp32 from D and alpha on, every operation rounded on its own in the header's order (the translation unit is compiled -ffp-contract=off); the
// kernels run with fp32 subnormals kept (the code object's float_denorm_mode_32 = 3, the compiler's default for gfx9), which the tails of
// alpha need.  No atomics, no sum across threads: both builds and every batch size give the same bytes.
#include "common.h"

namespace {

constexpr int BL_MAX_SIDE = 65535;
constexpr int BL_T1X = EG3D_BLEND_L1_TILE_W / 2, BL_T1Y = EG3D_BLEND_L1_TILE_H / 2;   // level-1 outputs of a blend_level1 workgroup
constexpr int BL_T0X = 2 * BL_T1X + 3, BL_T0Y = 2 * BL_T1Y + 3;                      // the level-0 pixels under them (2-pixel halo)
constexpr int BL_T0P = BL_T0X + 1;                                                  // LDS row pitch
constexpr int BL_CX = EG3D_BLEND_COMPOSE_TILE_W, BL_CY = EG3D_BLEND_COMPOSE_TILE_H;  // window pixels of a blend_compose workgroup
static_assert(BL_CX == 64 && BL_CY == 16, "blend_compose_kernel: 32 x 8 threads of 2 x 2 pixels");

struct BlendGeom {
    double m[6];
    double inv_feather, inv255;          // host doubles: no division on the device
    int64_t mask_stride;                 // bytes between the masks of two frames; 0: one mask for all
    int32_t Wp, S;
    int32_t wx0, wy0, ww, wh;            // the window in the photo
    int32_t h1, w1;                      // level 1
    int32_t cx0, cy0, cx1, cy1;          // the window pixels that are written (window coordinates)
    int32_t Ho, Wo, ox, oy;              // a frame of dst; window pixel (x, y) lands at (x + ox, y + oy)
    int32_t chw;
};

// Level 0 at photo pixel (X, Y) of frame n.  eg3d_paste_back8's steps in fp64, then one rounding to fp32 each.
template <int CH>
__device__ __forceinline__ void blend_sample(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits, const uint8_t* __restrict__ mask,
                                             const BlendGeom& g, int n, int X, int Y, float (&D)[CH], float& alpha) {
    const int S = g.S;
    const double Xc = X + 0.5, Yc = Y + 0.5, Sd = (double)S;
    const double u = g.m[0] + g.m[1] * Xc + g.m[2] * Yc;                          // left to right, every operation rounded on its own
    const double v = g.m[3] + g.m[4] * Xc + g.m[5] * Yc;
#pragma unroll
    for (int c = 0; c < CH; ++c) D[c] = 0.f;
    alpha = 0.f;
    if (!(u >= 0.0 && u < Sd && v >= 0.0 && v < Sd)) return;                      // outside the aligned frame (or NaN)
    const uint8_t* ph = photo + ((int64_t)Y * g.Wp + X) * CH;
    const double xin = u - 0.5, yin = v - 0.5;
    const double fxd = floor(xin), fyd = floor(yin);
    const double dx = xin - fxd, dy = yin - fyd;
    const int fx = (int)fxd, fy = (int)fyd;                                     // within [-1, S - 1]
    const int xa = min(max(fx, 0), S - 1), xb = min(max(fx + 1, 0), S - 1);
    const int ya = min(max(fy, 0), S - 1), yb = min(max(fy + 1, 0), S - 1);
    const double d = fmin(fmin(u, Sd - u), fmin(v, Sd - v));
    const double f = g.inv_feather > 0.0 ? fmin(d * g.inv_feather, 1.0) : 1.0;
    double a = (f * f) * (3.0 - 2.0 * f);
    if (mask != nullptr) {
        const uint8_t* mk = mask + (int64_t)n * g.mask_stride;
        const double p00 = mk[(int64_t)ya * S + xa], p01 = mk[(int64_t)ya * S + xb], p10 = mk[(int64_t)yb * S + xa], p11 = mk[(int64_t)yb * S + xb];
        const double r0 = p00 + (p01 - p00) * dx;
        const double r1 = p10 + (p11 - p10) * dx;
        a = a * ((r0 + (r1 - r0) * dy) * g.inv255);
    }
    const uint8_t* ra = edits + (((int64_t)n * S + ya) * S) * CH;
    const uint8_t* rb = edits + (((int64_t)n * S + yb) * S) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double p00 = ra[xa * CH + c], p01 = ra[xb * CH + c], p10 = rb[xa * CH + c], p11 = rb[xb * CH + c];
        const double r0 = p00 + (p01 - p00) * dx;
        const double r1 = p10 + (p11 - p10) * dx;
        const double val = r0 + (r1 - r0) * dy;
        D[c] = (float)(val - (double)ph[c]);
    }
    alpha = (float)a;
}

// the 1-D reduce of the header on taps x[2i - 2] .. x[2i + 2]
__device__ __forceinline__ float reduce5(float a, float b, float c, float d, float e) { return (((a + e) + 4.f * (b + d)) + 6.f * c) * 0.0625f; }

// the 1-D expand of the header at an even (taps j - 1, j, j + 1) or odd (taps j, j + 1) index; t0, t1, t2 = x[j - 1], x[j], x[j + 1]
__device__ __forceinline__ float expand3(bool odd, float t0, float t1, float t2) {
    const float ev = ((t0 + t2) + 6.f * t1) * 0.125f, od = (t1 + t2) * 0.5f;
    return odd ? od : ev;
}

// rows first, then columns, on the 3 x 3 neighbourhood t[r][c] = x[jy - 1 + r][jx - 1 + c] (zeros outside the array)
__device__ __forceinline__ float expand9(bool xodd, bool yodd, const float (&t)[9]) {
    const float r0 = expand3(xodd, t[0], t[1], t[2]), r1 = expand3(xodd, t[3], t[4], t[5]), r2 = expand3(xodd, t[6], t[7], t[8]);
    return expand3(yodd, r0, r1, r2);
}

// the 3 x 3 neighbourhood of (jy, jx) in a plane of h x w floats, zeros outside
__device__ __forceinline__ void load9(const float* __restrict__ pl, int h, int w, int jy, int jx, float (&t)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int y = jy - 1 + r;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int x = jx - 1 + c;
            t[r * 3 + c] = (y >= 0 && y < h && x >= 0 && x < w) ? pl[(int64_t)y * w + x] : 0.f;
        }
    }
}

// grid (ceil(w1 / BL_T1X), ceil(h1 / BL_T1Y), N), block 256.  lvl1: [N][CH + 1][h1][w1], the planes of D and then alpha
template <int CH>
__global__ void __launch_bounds__(256) blend_level1_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                           const uint8_t* __restrict__ mask, float* __restrict__ lvl1, BlendGeom g) {
    __shared__ float s[CH + 1][BL_T0Y][BL_T0P];
    const int i0 = blockIdx.x * BL_T1X, j0 = blockIdx.y * BL_T1Y, n = blockIdx.z;
    const int bx = 2 * i0 - 2, by = 2 * j0 - 2;                                   // the tile's first level-0 pixel (window coordinates)
    for (int t = threadIdx.x; t < BL_T0X * BL_T0Y; t += 256) {
        const int ty = t / BL_T0X, tx = t - ty * BL_T0X;
        const int x = bx + tx, y = by + ty;
        float D[CH], a = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) D[c] = 0.f;
        if (x >= 0 && x < g.ww && y >= 0 && y < g.wh) blend_sample<CH>(photo, edits, mask, g, n, g.wx0 + x, g.wy0 + y, D, a);
#pragma unroll
        for (int c = 0; c < CH; ++c) s[c][ty][tx] = D[c];
        s[CH][ty][tx] = a;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < (CH + 1) * BL_T1X * BL_T1Y; t += 256) {
        const int p = t / (BL_T1X * BL_T1Y), r = t - p * (BL_T1X * BL_T1Y);
        const int oy = r / BL_T1X, ox = r - oy * BL_T1X;
        const int i = i0 + ox, j = j0 + oy;
        if (i >= g.w1 || j >= g.h1) continue;
        float row[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float* q = &s[p][2 * oy + k][2 * ox];
            row[k] = reduce5(q[0], q[1], q[2], q[3], q[4]);
        }
        lvl1[(((int64_t)n * (CH + 1) + p) * g.h1 + j) * g.w1 + i] = reduce5(row[0], row[1], row[2], row[3], row[4]);
    }
}

// grid (ceil(wd / 64), ceil(hd / 4), N), block 256; src [N][planes][hs][ws] -> dst [N][planes][hd][wd]
__global__ void __launch_bounds__(256) blend_reduce_kernel(const float* __restrict__ src, float* __restrict__ dst, int planes, int hs, int ws, int hd,
                                                           int wd) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (i >= wd || j >= hd) return;
    for (int p = 0; p < planes; ++p) {
        const float* pl = src + ((int64_t)n * planes + p) * hs * ws;
        float row[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int y = 2 * j - 2 + k;
            float q[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                const int x = 2 * i - 2 + e;
                q[e] = (y >= 0 && y < hs && x >= 0 && x < ws) ? pl[(int64_t)y * ws + x] : 0.f;
            }
            row[k] = reduce5(q[0], q[1], q[2], q[3], q[4]);
        }
        dst[(((int64_t)n * planes + p) * hd + j) * wd + i] = reduce5(row[0], row[1], row[2], row[3], row[4]);
    }
}

// grid (ceil(wk1 / 64), ceil(hk1 / 4), N), block 256: a thread owns the 2 x 2 pixels of level k under pixel (jy, jx) of level k + 1, which
// share its 3 x 3 neighbourhood.  da_k [N][CH + 1][hk][wk], da_k1 [N][CH + 1][hk1][wk1], r_k1 [N][CH][hk1][wk1] or nullptr (level k + 1 is
// the coarsest: R = D alpha), r_k [N][CH][hk][wk]
template <int CH>
__global__ void __launch_bounds__(256) blend_collapse_kernel(const float* __restrict__ da_k, const float* __restrict__ da_k1,
                                                             const float* __restrict__ r_k1, float* __restrict__ r_k, int hk, int wk, int hk1, int wk1) {
    const int jx = blockIdx.x * 64 + (threadIdx.x & 63), jy = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (jx >= wk1 || jy >= hk1) return;
    const int64_t pk = (int64_t)hk * wk, pk1 = (int64_t)hk1 * wk1;
    const float* ak = da_k + ((int64_t)n * (CH + 1) + CH) * pk;
    float ta[9];
    if (r_k1 == nullptr) load9(da_k1 + ((int64_t)n * (CH + 1) + CH) * pk1, hk1, wk1, jy, jx, ta);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        float td[9], tr[9];
        load9(da_k1 + ((int64_t)n * (CH + 1) + c) * pk1, hk1, wk1, jy, jx, td);
        if (r_k1 == nullptr) {
#pragma unroll
            for (int e = 0; e < 9; ++e) tr[e] = td[e] * ta[e];
        } else {
            load9(r_k1 + ((int64_t)n * CH + c) * pk1, hk1, wk1, jy, jx, tr);
        }
        const float* dk = da_k + ((int64_t)n * (CH + 1) + c) * pk;
        float* rk = r_k + ((int64_t)n * CH + c) * pk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = 2 * jx + (q & 1), y = 2 * jy + (q >> 1);
            if (x >= wk || y >= hk) continue;
            const int64_t at = (int64_t)y * wk + x;
            rk[at] = (dk[at] - expand9(q & 1, q >> 1, td)) * ak[at] + expand9(q & 1, q >> 1, tr);
        }
    }
}

// grid (ceil(ww / BL_CX), ceil(wh / BL_CY), N), block 256 = 32 x 8: a thread owns the 2 x 2 window pixels under level-1 pixel
// (blockIdx.y * 8 + threadIdx.x / 32, blockIdx.x * 32 + threadIdx.x % 32).  da_1 [N][CH + 1][h1][w1]; r_1 [N][CH][h1][w1] or nullptr (bands = 1: R_1 = D_1 alpha_1)
template <int CH>
__global__ void __launch_bounds__(256) blend_compose_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                            const uint8_t* __restrict__ mask, const float* __restrict__ da_1,
                                                            const float* __restrict__ r_1, uint8_t* __restrict__ dst, BlendGeom g) {
    const int jx = blockIdx.x * (BL_CX / 2) + (threadIdx.x & 31), jy = blockIdx.y * (BL_CY / 2) + (threadIdx.x >> 5), n = blockIdx.z;
    const int x0 = 2 * jx, y0 = 2 * jy;
    if (x0 >= g.cx1 || y0 >= g.cy1 || x0 + 2 <= g.cx0 || y0 + 2 <= g.cy0) return;  // none of the four pixels is written
    const int64_t p1 = (int64_t)g.h1 * g.w1;
    float td[CH][9], tr[CH][9];
    if (r_1 == nullptr) {
        float ta[9];
        load9(da_1 + ((int64_t)n * (CH + 1) + CH) * p1, g.h1, g.w1, jy, jx, ta);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            load9(da_1 + ((int64_t)n * (CH + 1) + c) * p1, g.h1, g.w1, jy, jx, td[c]);
#pragma unroll
            for (int e = 0; e < 9; ++e) tr[c][e] = td[c][e] * ta[e];
        }
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            load9(da_1 + ((int64_t)n * (CH + 1) + c) * p1, g.h1, g.w1, jy, jx, td[c]);
            load9(r_1 + ((int64_t)n * CH + c) * p1, g.h1, g.w1, jy, jx, tr[c]);
        }
    }
    const int64_t plane = (int64_t)g.Ho * g.Wo, cs = g.chw ? plane : 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = x0 + (q & 1), y = y0 + (q >> 1);
        if (x < g.cx0 || x >= g.cx1 || y < g.cy0 || y >= g.cy1) continue;       // the written pixels lie inside the window
        const int X = g.wx0 + x, Y = g.wy0 + y;
        float D[CH], a;
        blend_sample<CH>(photo, edits, mask, g, n, X, Y, D, a);
        const uint8_t* ph = photo + ((int64_t)Y * g.Wp + X) * CH;
        const int64_t pix = (int64_t)(g.oy + y) * g.Wo + (g.ox + x);
        uint8_t* o = dst + (int64_t)n * plane * CH + (g.chw ? pix : pix * CH);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float r0 = (D[c] - expand9(q & 1, q >> 1, td[c])) * a + expand9(q & 1, q >> 1, tr[c]);
            const float r = rintf((float)ph[c] + r0);                            // round half to even
            o[c * cs] = (uint8_t)(int)fminf(fmaxf(r, 0.f), 255.f);
        }
    }
}

struct BlendLevels {
    int L;
    int h[EG3D_BLEND_MAX_BANDS + 1], w[EG3D_BLEND_MAX_BANDS + 1];
    int wx0, wy0;
    int64_t da[EG3D_BLEND_MAX_BANDS + 1], r[EG3D_BLEND_MAX_BANDS + 1];          // offsets in floats into the workspace (levels 1..L, 1..L-1)
    int64_t floats;
};

// everything eg3d_paste_back8 refuses, and the bands
bool blend_params_ok(const eg3d_paste_blend8_params* p) {
    auto dims_ok = [](int N, int H, int W, int C) {
        return N >= 1 && N <= BL_MAX_SIDE && (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= BL_MAX_SIDE && W <= BL_MAX_SIDE;
    };
    if (p == nullptr || p->photo == nullptr || p->edits == nullptr || p->dst == nullptr) return false;
    if (!dims_ok(p->N, p->Hp, p->Wp, p->C) || !dims_ok(p->N, p->S, p->S, p->C)) return false;
    if (p->x0 < 0 || p->y0 < 0 || p->x1 < p->x0 || p->y1 < p->y0 || p->x1 > p->Wp || p->y1 > p->Hp) return false;
    if (p->layout != EG3D_PASTE_HWC && p->layout != EG3D_PASTE_CHW) return false;
    if (p->mask != nullptr && p->mask_frames != 1 && p->mask_frames != p->N) return false;
    if (!(p->inv_feather >= 0.0)) return false;
    return p->bands >= 1 && p->bands <= EG3D_BLEND_MAX_BANDS;
}

// the window, the level sizes and the workspace layout; an empty box has no levels (floats = 0)
BlendLevels blend_levels(const eg3d_paste_blend8_params* p) {
    BlendLevels v = {};
    v.L = p->bands;
    if (p->x1 == p->x0 || p->y1 == p->y0) return v;
    const int M = 1 << (p->bands + 2);
    v.wx0 = p->x0 - M > 0 ? p->x0 - M : 0;
    v.wy0 = p->y0 - M > 0 ? p->y0 - M : 0;
    v.w[0] = (p->x1 + M < p->Wp ? p->x1 + M : p->Wp) - v.wx0;
    v.h[0] = (p->y1 + M < p->Hp ? p->y1 + M : p->Hp) - v.wy0;
    int64_t at = 0;
    for (int k = 1; k <= v.L; ++k) {
        v.h[k] = (v.h[k - 1] + 1) / 2;
        v.w[k] = (v.w[k - 1] + 1) / 2;
        v.da[k] = at;
        at += (int64_t)p->N * (p->C + 1) * v.h[k] * v.w[k];
    }
    for (int k = 1; k < v.L; ++k) {
        v.r[k] = at;
        at += (int64_t)p->N * p->C * v.h[k] * v.w[k];
    }
    v.floats = at;
    return v;
}

}  // namespace

extern "C" int eg3d_paste_blend8_query_workspace(const eg3d_paste_blend8_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr || !blend_params_ok(p)) return EG3D_ERR_INVALID;
    *workspace_bytes = blend_levels(p).floats * (int64_t)sizeof(float);
    return EG3D_OK;
}

extern "C" int eg3d_paste_blend8(const eg3d_paste_blend8_params* p, void* stream) {
    if (!blend_params_ok(p)) return EG3D_ERR_INVALID;
    const BlendLevels v = blend_levels(p);
    if (v.floats > 0 && (p->workspace == nullptr || p->workspace_bytes < v.floats * (int64_t)sizeof(float) ||
                         (reinterpret_cast<uintptr_t>(p->workspace) & 3) != 0))
        return EG3D_ERR_INVALID;
    // whole = 1: eg3d_paste_back8's own copy of the photo into every frame, by a call of it with an empty region (nothing else is launched)
    eg3d_paste_back8_params cp = {};
    cp.photo = p->photo; cp.edits = p->edits; cp.mask = p->mask; cp.dst = p->dst;
    for (int i = 0; i < 6; ++i) cp.m[i] = p->m[i];
    cp.inv_feather = p->inv_feather;
    cp.N = p->N; cp.Hp = p->Hp; cp.Wp = p->Wp; cp.C = p->C; cp.S = p->S;
    cp.x0 = cp.x1 = p->x0; cp.y0 = cp.y1 = p->y0;
    cp.mask_frames = p->mask_frames; cp.whole = p->whole; cp.layout = p->layout;
    const int rc = eg3d_paste_back8(&cp, stream);
    if (rc != EG3D_OK || v.floats == 0) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int CH = p->C, N = p->N, L = v.L;
    float* ws = static_cast<float*>(p->workspace);
    BlendGeom g;
    for (int i = 0; i < 6; ++i) g.m[i] = p->m[i];
    g.inv_feather = p->inv_feather;
    g.inv255 = 1.0 / 255.0;
    g.mask_stride = p->mask != nullptr && p->mask_frames > 1 ? (int64_t)p->S * p->S : 0;
    g.Wp = p->Wp; g.S = p->S;
    g.wx0 = v.wx0; g.wy0 = v.wy0; g.ww = v.w[0]; g.wh = v.h[0];
    g.h1 = v.h[1]; g.w1 = v.w[1];
    if (p->whole) {
        g.cx0 = 0; g.cy0 = 0; g.cx1 = g.ww; g.cy1 = g.wh;
        g.Ho = p->Hp; g.Wo = p->Wp; g.ox = g.wx0; g.oy = g.wy0;
    } else {                                                                     // the bounding box alone: the margin's changes are dropped
        g.cx0 = p->x0 - g.wx0; g.cy0 = p->y0 - g.wy0; g.cx1 = p->x1 - g.wx0; g.cy1 = p->y1 - g.wy0;
        g.Ho = p->y1 - p->y0; g.Wo = p->x1 - p->x0; g.ox = -g.cx0; g.oy = -g.cy0;
    }
    g.chw = p->layout == EG3D_PASTE_CHW;

    const dim3 g1((unsigned)((g.w1 + BL_T1X - 1) / BL_T1X), (unsigned)((g.h1 + BL_T1Y - 1) / BL_T1Y), (unsigned)N);
    if (CH == 3)
        hipLaunchKernelGGL(blend_level1_kernel<3>, g1, dim3(256), 0, st, p->photo, p->edits, p->mask, ws + v.da[1], g);
    else
        hipLaunchKernelGGL(blend_level1_kernel<1>, g1, dim3(256), 0, st, p->photo, p->edits, p->mask, ws + v.da[1], g);
    EG3D_LAUNCH_CHECK();
    auto grid_of = [N](int h, int w) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)N); };
    for (int k = 1; k < L; ++k) {
        hipLaunchKernelGGL(blend_reduce_kernel, grid_of(v.h[k + 1], v.w[k + 1]), dim3(256), 0, st, ws + v.da[k], ws + v.da[k + 1], CH + 1, v.h[k],
                           v.w[k], v.h[k + 1], v.w[k + 1]);
        EG3D_LAUNCH_CHECK();
    }
    for (int k = L - 1; k >= 1; --k) {
        const float* rk1 = k + 1 == L ? nullptr : ws + v.r[k + 1];
        if (CH == 3)
            hipLaunchKernelGGL(blend_collapse_kernel<3>, grid_of(v.h[k + 1], v.w[k + 1]), dim3(256), 0, st, ws + v.da[k], ws + v.da[k + 1], rk1, ws + v.r[k],
                               v.h[k], v.w[k], v.h[k + 1], v.w[k + 1]);
        else
            hipLaunchKernelGGL(blend_collapse_kernel<1>, grid_of(v.h[k + 1], v.w[k + 1]), dim3(256), 0, st, ws + v.da[k], ws + v.da[k + 1], rk1, ws + v.r[k],
                               v.h[k], v.w[k], v.h[k + 1], v.w[k + 1]);
        EG3D_LAUNCH_CHECK();
    }
    const float* r1 = L == 1 ? nullptr : ws + v.r[1];
    const dim3 gc((unsigned)((g.ww + BL_CX - 1) / BL_CX), (unsigned)((g.wh + BL_CY - 1) / BL_CY), (unsigned)N);
    if (CH == 3)
        hipLaunchKernelGGL(blend_compose_kernel<3>, gc, dim3(256), 0, st, p->photo, p->edits, p->mask, ws + v.da[1], r1, p->dst, g);
    else
        hipLaunchKernelGGL(blend_compose_kernel<1>, gc, dim3(256), 0, st, p->photo, p->edits, p->mask, ws + v.da[1], r1, p->dst, g);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
