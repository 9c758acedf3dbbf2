// Shape views: first-hit iso-surface ray marcher over a regular fp32 grid (include/eg3d_hip.h "Shape views").
//
// Two kernels:
//   iso_bricks_kernel  one workgroup per 8x8x8-cell brick: the maximum of the grid over the brick's corner range dilated by one voxel (at most 11^3
//                      values; 16 lanes along i2, 16 rows per pass).  A maximum is exact in any order, so the reduction order does not matter.
//   iso_render_kernel  one wave per 8x8 pixel tile of one camera (neighbouring rays walk neighbouring cells: their loads share cache lines), one
//                      lane per ray.  The grid is read with plain global loads (512^3 is larger than every cache; the brick array, 1 MB, is not),
//                      nothing is shared between lanes and nothing is accumulated: every output is a function of its own ray.
// The field, the frame, the normal and the camera maps are csrc/shape_common.h's; its rule holds here too: the arithmetic is the header's
// specification operation for operation (tests/support/iso_ref.py restates it, the outputs are compared bit for bit).
#include "shape_common.h"

namespace {

constexpr int ISO_BRICK = 8;
constexpr int ISO_BRICK_THREADS = 256;
constexpr int ISO_TILE = 8;
constexpr int ISO_KMAX = 1 << 24;                     // float(k) is exact up to here

using shape::Cell;
using shape::Grid;

__global__ void __launch_bounds__(ISO_BRICK_THREADS) iso_bricks_kernel(const float* __restrict__ vol, int32_t D0, int32_t D1, int32_t D2, int32_t B1,
                                                                      int32_t B2, float* __restrict__ bricks) {
    __shared__ float wmax[ISO_BRICK_THREADS / 64];
    const int32_t b = (int32_t)blockIdx.x;
    const int32_t b2 = b % B2, b1 = (b / B2) % B1, b0 = b / (B2 * B1);
    const int32_t lo0 = max(b0 * ISO_BRICK - 1, 0), hi0 = min(b0 * ISO_BRICK + ISO_BRICK + 1, D0 - 1);
    const int32_t lo1 = max(b1 * ISO_BRICK - 1, 0), hi1 = min(b1 * ISO_BRICK + ISO_BRICK + 1, D1 - 1);
    const int32_t lo2 = max(b2 * ISO_BRICK - 1, 0), hi2 = min(b2 * ISO_BRICK + ISO_BRICK + 1, D2 - 1);
    const int32_t n1 = hi1 - lo1 + 1, rows = (hi0 - lo0 + 1) * n1;
    const int32_t i2 = lo2 + (int32_t)(threadIdx.x & 15);
    float m = -INFINITY;
    if (i2 <= hi2) {
        for (int32_t r = (int32_t)(threadIdx.x >> 4); r < rows; r += ISO_BRICK_THREADS / 16) {
            const int32_t i0 = lo0 + r / n1, i1 = lo1 + r % n1;
            const float v = vol[((int64_t)i0 * D1 + i1) * D2 + i2];
            m = v > m ? v : m;                        // a NaN never replaces m
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float y = __shfl_xor(m, o);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ISO_BRICK_THREADS / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
        bricks[b] = m + 0.0f;                         // -0 -> +0: the stored bits do not depend on the order the zeros were met in
    }
}

// one slab; returns false when the ray cannot meet it
__device__ __forceinline__ bool iso_slab(float o, float d, float h, float& tn, float& tf) {
    if (d == 0.0f) return o >= 0.0f && o <= h;
    const float t0 = (0.0f - o) / d, t1 = (h - o) / d;
    const float lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
    tn = lo > tn ? lo : tn;
    tf = hi < tf ? hi : tf;
    return true;
}

// the brick's exit distance along one axis folded into te
__device__ __forceinline__ void iso_exit(float o, float d, int32_t b, float& te) {
    if (d == 0.0f) return;
    const float plane = d > 0.0f ? (float)(ISO_BRICK * b + ISO_BRICK) : (float)(ISO_BRICK * b);
    const float t = (plane - o) / d;
    te = t < te ? t : te;
}

struct IsoArgs {
    Grid g;
    const float* bricks;
    int32_t B1, B2;                                   // bricks per axis 1 and 2
    const float* cams;
    float* depth;
    float* normal;
    uint8_t* mask;
    int32_t* hit_k;
    float* shade;
    int32_t res;
    shape::Frame fr;
    float level, dt;
    int32_t refine, skip, shade_mode;
    float ambient, background;
};

__global__ void __launch_bounds__(ISO_TILE* ISO_TILE) iso_render_kernel(IsoArgs a) {
    const int32_t x = (int32_t)blockIdx.x * ISO_TILE + (int32_t)(threadIdx.x & (ISO_TILE - 1));
    const int32_t y = (int32_t)blockIdx.y * ISO_TILE + (int32_t)(threadIdx.x / ISO_TILE);
    const int32_t f = (int32_t)blockIdx.z;
    if (x >= a.res || y >= a.res) return;
    const Grid& g = a.g;
    const float* __restrict__ c = a.cams + (int64_t)f * 25;
    float xl, yl, o[3], d[3];
    shape::pixel_to_local(c, x, y, a.res, xl, yl);
    shape::local_to_world_dir(c, xl, yl, o, d);
    float oi0, oi1, oi2;
    shape::world_to_index(a.fr, o[0], o[1], o[2], oi0, oi1, oi2);
    const float di0 = shape::sel(d[0], d[1], d[2], a.fr.ax0) / a.fr.sp0;
    const float di1 = shape::sel(d[0], d[1], d[2], a.fr.ax1) / a.fr.sp1;
    const float di2 = shape::sel(d[0], d[1], d[2], a.fr.ax2) / a.fr.sp2;

    float tn = 0.0f, tf = INFINITY;
    bool live = iso_slab(oi0, di0, g.h0, tn, tf);
    live = iso_slab(oi1, di1, g.h1, tn, tf) && live;
    live = iso_slab(oi2, di2, g.h2, tn, tf) && live;
    live = live && tf >= tn;
    int32_t K = -1;                                   // the loop bound: fixed before the loop, k grows by at least one per iteration
    if (live) {
        const float q = floorf((tf - tn) / a.dt);
        if (q >= 0.0f) K = q < (float)ISO_KMAX ? (int32_t)q : ISO_KMAX;
    }
    int32_t hit = -1;
    float fb = 0.0f;
    int32_t k = 0;
    while (k <= K) {
        const float t = tn + (float)k * a.dt;
        const Cell cell = shape::cell(g, shape::clamp(oi0 + t * di0, g.h0), shape::clamp(oi1 + t * di1, g.h1), shape::clamp(oi2 + t * di2, g.h2));
        if (a.skip) {
            const int32_t b0 = cell.i0 >> 3, b1 = cell.i1 >> 3, b2 = cell.i2 >> 3;
            if (a.bricks[((int64_t)b0 * a.B1 + b1) * a.B2 + b2] <= a.level) {
                float te = INFINITY;
                iso_exit(oi0, di0, b0, te);
                iso_exit(oi1, di1, b1, te);
                iso_exit(oi2, di2, b2, te);
                const float q = floorf((te - tn) / a.dt);
                int32_t kn = k + 1;
                if (q > (float)kn) kn = q < (float)(K + 1) ? (int32_t)q : K + 1;
                k = kn;
                continue;
            }
        }
        const float v = shape::trilinear(g, cell);
        if (v > a.level) {
            hit = k;
            fb = v;
            break;
        }
        ++k;
    }

    float th = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    if (hit >= 0) {
        th = tn;
        if (hit > 0) {
            float ta = tn + (float)(hit - 1) * a.dt, tb = tn + (float)hit * a.dt;
            float fa = shape::field(g, oi0 + ta * di0, oi1 + ta * di1, oi2 + ta * di2);
            for (int32_t r = 0; r < a.refine; ++r) {
                const float tm = ta + (tb - ta) * 0.5f;
                const float fm = shape::field(g, oi0 + tm * di0, oi1 + tm * di1, oi2 + tm * di2);
                if (fm > a.level) {
                    tb = tm;
                    fb = fm;
                } else {
                    ta = tm;
                    fa = fm;
                }
            }
            th = ta + (tb - ta) * ((a.level - fa) / (fb - fa));
            if (!(th >= ta && th <= tb)) th = tb;
        }
        const float p0 = shape::clamp(oi0 + th * di0, g.h0), p1 = shape::clamp(oi1 + th * di1, g.h1), p2 = shape::clamp(oi2 + th * di2, g.h2);
        shape::gradient_normal(g, a.fr, p0, p1, p2, n);
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const bool ok = len > 0.0f;                   // false for a NaN gradient too
        for (int w = 0; w < 3; ++w) n[w] = ok ? n[w] / len : 0.0f;
    }

    const int64_t pix = ((int64_t)f * a.res + y) * a.res + x;
    if (a.depth) a.depth[pix] = th;
    if (a.mask) a.mask[pix] = hit >= 0 ? 1 : 0;
    if (a.hit_k) a.hit_k[pix] = hit;
    if (a.normal) {
        a.normal[pix * 3] = n[0];
        a.normal[pix * 3 + 1] = n[1];
        a.normal[pix * 3 + 2] = n[2];
    }
    if (a.shade) {
        float s[3] = {a.background, a.background, a.background};
        if (hit >= 0) {
            if (a.shade_mode == EG3D_ISO_LAMBERT) {
                const float v = shape::headlight(a.ambient, n, d);
                s[0] = s[1] = s[2] = v * 2.0f - 1.0f;
            } else {
                for (int j = 0; j < 3; ++j) {
                    const float nc = (c[j] * n[0] + c[4 + j] * n[1]) + c[8 + j] * n[2];
                    s[j] = (nc * 0.5f + 0.5f) * 2.0f - 1.0f;
                }
            }
        }
        const int64_t plane = (int64_t)a.res * a.res;
        float* __restrict__ sp = a.shade + (int64_t)f * 3 * plane + (int64_t)y * a.res + x;
        sp[0] = s[0];
        sp[plane] = s[1];
        sp[2 * plane] = s[2];
    }
}

// validates what both entries share; fills g and the bricks per axis
int iso_grid(const eg3d_iso_params* p, Grid& g, int32_t B[3]) {
    if (p == nullptr || p->vol == nullptr) return EG3D_ERR_INVALID;
    const int s = shape::grid_fill(p->vol, p->D0, p->D1, p->D2, g);
    if (s != EG3D_OK) return s;
    B[0] = (p->D0 + 6) / ISO_BRICK;
    B[1] = (p->D1 + 6) / ISO_BRICK;
    B[2] = (p->D2 + 6) / ISO_BRICK;
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_iso_bricks(const eg3d_iso_params* p, void* stream) {
    Grid g;
    int32_t B[3];
    const int s = iso_grid(p, g, B);
    if (s != EG3D_OK) return s;
    if (p->bricks == nullptr) return EG3D_ERR_INVALID;
    hipLaunchKernelGGL(iso_bricks_kernel, dim3((unsigned)(B[0] * B[1] * B[2])), dim3(ISO_BRICK_THREADS), 0, (hipStream_t)stream, g.vol, g.D0, g.D1, g.D2,
                       B[1], B[2], p->bricks);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_iso_render(const eg3d_iso_params* p, void* stream) {
    IsoArgs a;
    int32_t B[3];
    const int s = iso_grid(p, a.g, B);
    if (s != EG3D_OK) return s;
    if (p->cams == nullptr || p->F < 1 || p->res < 1) return EG3D_ERR_INVALID;
    if (p->skip != 0 && p->bricks == nullptr) return EG3D_ERR_INVALID;
    if (!shape::frame_fill(p->axes, p->origin, p->spacing, a.fr)) return EG3D_ERR_INVALID;
    if (!shape::finite(p->level) || !(p->step >= 1.0f / 64 && p->step <= 64.0f) || p->refine < 0 || p->refine > 32) return EG3D_ERR_INVALID;
    if (!(p->ambient >= 0.0f && p->ambient <= 1.0f) || !shape::finite(p->background)) return EG3D_ERR_INVALID;
    if (p->shade_mode != EG3D_ISO_LAMBERT && p->shade_mode != EG3D_ISO_NORMAL) return EG3D_ERR_INVALID;
    if (p->res > 16384 || p->F > 65535) return EG3D_ERR_UNSUPPORTED;
    float ms = fabsf(p->spacing[0]);
    for (int i = 1; i < 3; ++i) ms = fabsf(p->spacing[i]) < ms ? fabsf(p->spacing[i]) : ms;
    a.bricks = p->bricks;
    a.B1 = B[1];
    a.B2 = B[2];
    a.cams = p->cams;
    a.depth = p->depth;
    a.normal = p->normal;
    a.mask = p->mask;
    a.hit_k = p->hit_k;
    a.shade = p->shade;
    a.res = p->res;
    a.level = p->level;
    a.dt = p->step * ms;
    a.refine = p->refine;
    a.skip = p->skip;
    a.shade_mode = p->shade_mode;
    a.ambient = p->ambient;
    a.background = p->background;
    if (!(a.dt > 0.0f) || !shape::finite(a.dt)) return EG3D_ERR_INVALID;
    const unsigned tiles = (unsigned)((p->res + ISO_TILE - 1) / ISO_TILE);
    hipLaunchKernelGGL(iso_render_kernel, dim3(tiles, tiles, (unsigned)p->F), dim3(ISO_TILE * ISO_TILE), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
