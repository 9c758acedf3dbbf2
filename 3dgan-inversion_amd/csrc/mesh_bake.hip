// Mesh attributes: per-vertex normals of the density field and view-baked vertex colours (include/eg3d_hip.h "Mesh attributes").
//
// Two kernels, one thread per vertex, nothing shared between threads and no atomics: every output is a function of its own vertex.
//   mesh_normals_kernel  the gradient of the trilinear field at the vertex (24 field evaluations of 8 loads each; neighbouring vertices
//                        read neighbouring cells).  The field functions restate csrc/iso_render.hip's: that file stays as it is.
//   mesh_bake_kernel     walks the views in index order: projection, four depth taps, four image taps per channel.  Vertices arrive ordered
//                        by owning grid point (mc_emit), so a wave projects to neighbouring pixels and its gathers share cache lines.  The view
//                        index is uniform over the launch, so the 25 camera floats of a view are uniform loads, not one load per lane.
//   mesh_texture_kernel  one thread per texel of the per-face atlas ("Mesh texture"): decodes its face and barycentrics, interpolates the
//                        face's three vertices and runs the same view loop (mesh_blend_views, the one copy).
// The arithmetic is the header's specification operation for operation: tests/support/mesh_ref.py restates it and the outputs are compared
// bit for bit, so nothing here may be reassociated, contracted or replaced by a reciprocal.
#include "common.h"

namespace {

constexpr int MESH_THREADS = 256;

struct MeshGrid {
    const float* vol;
    int32_t D0, D1, D2, S;                            // S = D1 * D2
    float h0, h1, h2;                                 // D - 1
};

__device__ __forceinline__ float mesh_clamp(float p, float h) {
    p = p > 0.0f ? p : 0.0f;                          // NaN -> 0
    return p < h ? p : h;
}

__device__ __forceinline__ float mesh_lerp_clamped(float a, float b, float f) {
    float r = a + f * (b - a);
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    r = r < lo ? lo : r;
    r = r > hi ? hi : r;
    return r;
}

__device__ __forceinline__ float mesh_field(const MeshGrid& g, float p0, float p1, float p2) {
    p0 = mesh_clamp(p0, g.h0);
    p1 = mesh_clamp(p1, g.h1);
    p2 = mesh_clamp(p2, g.h2);
    const int32_t i0 = min((int32_t)floorf(p0), g.D0 - 2), i1 = min((int32_t)floorf(p1), g.D1 - 2), i2 = min((int32_t)floorf(p2), g.D2 - 2);
    const float f0 = p0 - (float)i0, f1 = p1 - (float)i1, f2 = p2 - (float)i2;
    const float* __restrict__ q = g.vol + ((int64_t)i0 * g.S + (int64_t)i1 * g.D2 + i2);
    const float v000 = q[0], v001 = q[1], v010 = q[g.D2], v011 = q[g.D2 + 1];
    const float v100 = q[g.S], v101 = q[g.S + 1], v110 = q[g.S + g.D2], v111 = q[g.S + g.D2 + 1];
    const float c00 = mesh_lerp_clamped(v000, v001, f2), c01 = mesh_lerp_clamped(v010, v011, f2);
    const float c10 = mesh_lerp_clamped(v100, v101, f2), c11 = mesh_lerp_clamped(v110, v111, f2);
    return mesh_lerp_clamped(mesh_lerp_clamped(c00, c01, f1), mesh_lerp_clamped(c10, c11, f1), f0);
}

__device__ __forceinline__ float mesh_sel(float v0, float v1, float v2, int32_t w) { return w == 0 ? v0 : (w == 1 ? v1 : v2); }

struct NormalArgs {
    MeshGrid g;
    const float* points;
    float* normals;
    int64_t V;
    int32_t ax0, ax1, ax2;
    float org0, org1, org2, sp0, sp1, sp2;
};

__global__ void __launch_bounds__(MESH_THREADS) mesh_normals_kernel(NormalArgs a) {
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const MeshGrid& g = a.g;
    const float x0 = a.points[v * 3], x1 = a.points[v * 3 + 1], x2 = a.points[v * 3 + 2];
    const float r0 = (mesh_sel(x0, x1, x2, a.ax0) - a.org0) / a.sp0;
    const float r1 = (mesh_sel(x0, x1, x2, a.ax1) - a.org1) / a.sp1;
    const float r2 = (mesh_sel(x0, x1, x2, a.ax2) - a.org2) / a.sp2;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (r0 == r0 && r1 == r1 && r2 == r2) {           // a NaN index coordinate: no normal (the clamp would send it to index 0)
        const float p0 = mesh_clamp(r0, g.h0), p1 = mesh_clamp(r1, g.h1), p2 = mesh_clamp(r2, g.h2);
        const float u0 = mesh_clamp(p0 + 1.0f, g.h0), l0 = mesh_clamp(p0 - 1.0f, g.h0);
        const float u1 = mesh_clamp(p1 + 1.0f, g.h1), l1 = mesh_clamp(p1 - 1.0f, g.h1);
        const float u2 = mesh_clamp(p2 + 1.0f, g.h2), l2 = mesh_clamp(p2 - 1.0f, g.h2);
        const float g0 = (mesh_field(g, u0, p1, p2) - mesh_field(g, l0, p1, p2)) / ((u0 - l0) * a.sp0);
        const float g1 = (mesh_field(g, p0, u1, p2) - mesh_field(g, p0, l1, p2)) / ((u1 - l1) * a.sp1);
        const float g2 = (mesh_field(g, p0, p1, u2) - mesh_field(g, p0, p1, l2)) / ((u2 - l2) * a.sp2);
        for (int w = 0; w < 3; ++w) n[w] = -(a.ax0 == w ? g0 : (a.ax1 == w ? g1 : g2));
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const bool ok = len > 0.0f && len < INFINITY;  // false for a NaN or infinite component too
        for (int w = 0; w < 3; ++w) n[w] = ok ? n[w] / len : 0.0f;
    }
    a.normals[v * 3] = n[0];
    a.normals[v * 3 + 1] = n[1];
    a.normals[v * 3 + 2] = n[2];
}

// what the view loop reads beside its point and normal: shared by the vertex bake and the texel bake
struct MeshViews {
    const float* cams;
    const float* images;
    const float* depth;
    const uint8_t* mask;
    int32_t F, H, R;
    float depth_tol, cos_min;
    int32_t power;
};

struct MeshBlend {
    float acc0, acc1, acc2, wsum;
    int32_t seen;
};

struct BakeArgs {
    MeshViews s;
    const float* points;
    const float* normals;
    const float* fallback;
    float* color;
    uint8_t* rgb;
    float* weight;
    uint8_t* views;
    int64_t V;
};

__device__ __forceinline__ float mesh_lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ bool mesh_inside(float p, float hi) { return p >= 0.0f && p <= hi; }      // false for NaN

// Steps 1-5 of the header's "Mesh attributes" bake for one point p with normal n: the one copy of the view loop (mesh_bake_kernel and
// mesh_texture_kernel both call it, so a vertex and a texel that sits on it blend the same bits).
__device__ __forceinline__ MeshBlend mesh_blend_views(const MeshViews& a, float p0, float p1, float p2, float n0, float n1, float n2) {
    const float fH = (float)a.H, fR = (float)a.R, hiH = (float)(a.H - 1), hiR = (float)(a.R - 1);
    const int64_t planeH = (int64_t)a.H * a.H, planeR = (int64_t)a.R * a.R;
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, wsum = 0.0f;
    int32_t seen = 0;
    for (int32_t f = 0; f < a.F; ++f) {
        const float* __restrict__ m = a.cams + (int64_t)f * 25;
        const float q0 = p0 - m[3], q1 = p1 - m[7], q2 = p2 - m[11];
        const float t = sqrtf((q0 * q0 + q1 * q1) + q2 * q2);
        const float c0 = (m[0] * q0 + m[4] * q1) + m[8] * q2;
        const float c1 = (m[1] * q0 + m[5] * q1) + m[9] * q2;
        const float c2 = (m[2] * q0 + m[6] * q1) + m[10] * q2;
        if (!(t > 0.0f && c2 > 0.0f)) continue;
        const float fx = m[16], sk = m[17], cx = m[18], fy = m[20], cy = m[21];
        const float xl = c0 / c2, yl = c1 / c2;
        const float yc = yl * fy + cy;
        const float xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy;
        const float pxH = xc * fH - 0.5f, pyH = yc * fH - 0.5f;
        const float pxR = xc * fR - 0.5f, pyR = yc * fR - 0.5f;
        if (!(mesh_inside(pxH, hiH) && mesh_inside(pyH, hiH) && mesh_inside(pxR, hiR) && mesh_inside(pyR, hiR))) continue;
        // visibility: the four depth pixels around (pxR, pyR); the coordinates are within [0, R - 1], so the indices are too
        const int32_t dx0 = (int32_t)floorf(pxR), dy0 = (int32_t)floorf(pyR);
        const int32_t dx1 = min(dx0 + 1, a.R - 1), dy1 = min(dy0 + 1, a.R - 1);
        const float* __restrict__ dp = a.depth + (int64_t)f * planeR;
        const uint8_t* __restrict__ mp = a.mask + (int64_t)f * planeR;
        const int64_t o00 = (int64_t)dy0 * a.R + dx0, o01 = (int64_t)dy0 * a.R + dx1, o10 = (int64_t)dy1 * a.R + dx0, o11 = (int64_t)dy1 * a.R + dx1;
        const bool vis = (mp[o00] != 0 && t <= dp[o00] + a.depth_tol) || (mp[o01] != 0 && t <= dp[o01] + a.depth_tol) ||
                         (mp[o10] != 0 && t <= dp[o10] + a.depth_tol) || (mp[o11] != 0 && t <= dp[o11] + a.depth_tol);
        if (!vis) continue;
        const float c = -((n0 * q0 + n1 * q1) + n2 * q2) / t;
        if (!(c > a.cos_min)) continue;
        float w = c;
        for (int32_t k = 1; k < a.power; ++k) w = w * c;
        const float* __restrict__ ip = a.images + (int64_t)f * 3 * planeH;
        float col0, col1, col2;
        if (a.H >= 2) {
            const int32_t bx = min((int32_t)floorf(pxH), a.H - 2), by = min((int32_t)floorf(pyH), a.H - 2);
            const float tx = pxH - (float)bx, ty = pyH - (float)by;
            const float* __restrict__ s = ip + (int64_t)by * a.H + bx;
            col0 = mesh_lerp(mesh_lerp(s[0], s[1], tx), mesh_lerp(s[a.H], s[a.H + 1], tx), ty);
            s += planeH;
            col1 = mesh_lerp(mesh_lerp(s[0], s[1], tx), mesh_lerp(s[a.H], s[a.H + 1], tx), ty);
            s += planeH;
            col2 = mesh_lerp(mesh_lerp(s[0], s[1], tx), mesh_lerp(s[a.H], s[a.H + 1], tx), ty);
        } else {
            col0 = ip[0];
            col1 = ip[1];
            col2 = ip[2];
        }
        acc0 = acc0 + w * col0;
        acc1 = acc1 + w * col1;
        acc2 = acc2 + w * col2;
        wsum = wsum + w;
        seen = min(seen + 1, 255);
    }
    return MeshBlend{acc0, acc1, acc2, wsum, seen};
}

__device__ __forceinline__ uint8_t mesh_u8(float x) { return (uint8_t)(int)fminf(fmaxf(x * 127.5f + 128.f, 0.f), 255.f); }      // truncation, as eg3d_image_grid_u8

__global__ void __launch_bounds__(MESH_THREADS) mesh_bake_kernel(BakeArgs a) {
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const MeshBlend b = mesh_blend_views(a.s, a.points[v * 3], a.points[v * 3 + 1], a.points[v * 3 + 2], a.normals[v * 3], a.normals[v * 3 + 1],
                                         a.normals[v * 3 + 2]);
    float out0 = 0.0f, out1 = 0.0f, out2 = 0.0f;
    if (b.wsum > 0.0f) {
        out0 = b.acc0 / b.wsum;
        out1 = b.acc1 / b.wsum;
        out2 = b.acc2 / b.wsum;
    } else if (a.fallback) {
        out0 = a.fallback[v * 3];
        out1 = a.fallback[v * 3 + 1];
        out2 = a.fallback[v * 3 + 2];
    }
    if (a.color) {
        a.color[v * 3] = out0;
        a.color[v * 3 + 1] = out1;
        a.color[v * 3 + 2] = out2;
    }
    if (a.rgb) {
        a.rgb[v * 3] = mesh_u8(out0);
        a.rgb[v * 3 + 1] = mesh_u8(out1);
        a.rgb[v * 3 + 2] = mesh_u8(out2);
    }
    if (a.weight) a.weight[v] = b.wsum;
    if (a.views) a.views[v] = (uint8_t)b.seen;
}

// ---- mesh texture (include/eg3d_hip.h "Mesh texture") ----
// One thread per texel of the atlas, block-major: thread g is texel g % T^2 of block g / T^2, so at T = 8 a wave is one block -- two faces --
// and its lanes project to neighbouring pixels of every view (a row-major map over the atlas would give a wave 64 / T blocks, 16 faces at
// T = 8, and as many scattered gathers).  The three vertices of a face are read by every texel of its half block: uniform over half a wave,
// one cache line each.  Nothing per texel is written but the 3 + 1 output bytes.
struct TextureArgs {
    MeshViews s;
    const float* points;
    const float* normals;
    const int32_t* faces;
    const float* fallback;
    uint8_t* texture;
    uint8_t* views;
    float* uv;
    uint8_t* corner;
    int32_t* bad_faces;
    int64_t V, F, texels;
    int32_t T, per_row, Ht, Wt, fill;
};

__device__ __forceinline__ int32_t mesh_seli(int32_t v0, int32_t v1, int32_t v2, int32_t w) { return w == 0 ? v0 : (w == 1 ? v1 : v2); }

__device__ __forceinline__ float mesh_mix(float b0, float b1, float b2, float a0, float a1, float a2) { return (b0 * a0 + b1 * a1) + b2 * a2; }

__global__ void mesh_texture_clear_kernel(int32_t* bad_faces) { *bad_faces = 0; }

__global__ void __launch_bounds__(MESH_THREADS) mesh_texture_kernel(TextureArgs a) {
    const int64_t g = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (g >= a.texels) return;
    const int32_t T = a.T;
#ifdef EG3D_TEXTURE_ROWMAJOR                              // measurement switch: thread g is texel g of the atlas in raster order
    const int32_t ay = (int32_t)(g / a.Wt), ax = (int32_t)(g - (int64_t)ay * a.Wt);
    const int32_t brow = ay / T, j = ay - brow * T, bcol = ax / T, i = ax - bcol * T;
    const int32_t blk = brow * a.per_row + bcol;
#else
    const int32_t TT = T * T;
    const int32_t blk = (int32_t)(g / TT), loc = (int32_t)(g - (int64_t)blk * TT);
    const int32_t j = loc / T, i = loc - j * T;
    const int32_t brow = blk / a.per_row, bcol = blk - brow * a.per_row;
#endif
    const int32_t x0 = bcol * T, y0 = brow * T;
    const int64_t o = (int64_t)(y0 + j) * a.Wt + (x0 + i);
    const bool upper = i + j >= T;
    const int64_t f = 2 * (int64_t)blk + (upper ? 1 : 0);
    uint8_t t0 = (uint8_t)a.fill, t1 = (uint8_t)a.fill, t2 = (uint8_t)a.fill, seen = 0;
    if (f < a.F) {
        const int32_t k0 = a.faces[f * 3], k1 = a.faces[f * 3 + 1], k2 = a.faces[f * 3 + 2];
        const bool ok = k0 >= 0 && k0 < a.V && k1 >= 0 && k1 < a.V && k2 >= 0 && k2 < a.V;      // a bad index is never dereferenced
        const bool lead = upper ? (i == T - 1 && j == T - 1) : (i == 0 && j == 0);                 // the right-angle texel speaks for the face
        int32_t r = 0;
        if (ok) {
            const float* __restrict__ P0 = a.points + (int64_t)k0 * 3;
            const float* __restrict__ P1 = a.points + (int64_t)k1 * 3;
            const float* __restrict__ P2 = a.points + (int64_t)k2 * 3;
            const float u0 = P0[0], u1 = P0[1], u2 = P0[2], v0 = P1[0], v1 = P1[1], v2 = P1[2], w0 = P2[0], w1 = P2[1], w2 = P2[2];
            // e_k: the squared length of the edge opposite corner k
            float dx = w0 - v0, dy = w1 - v1, dz = w2 - v2;
            const float e0 = (dx * dx + dy * dy) + dz * dz;
            dx = u0 - w0, dy = u1 - w1, dz = u2 - w2;
            const float e1 = (dx * dx + dy * dy) + dz * dz;
            dx = v0 - u0, dy = v1 - u1, dz = v2 - u2;
            const float e2 = (dx * dx + dy * dy) + dz * dz;
            float er = e0;
            if (e1 > er) { r = 1; er = e1; }
            if (e2 > er) { r = 2; er = e2; }
            if (a.texture || a.views) {
                const int32_t ii = upper ? T - 1 - i : i, jj = upper ? T - 1 - j : j, leg = upper ? T - 3 : T - 2;
                const float b1 = (float)ii / (float)leg, b2 = (float)jj / (float)leg;
                const float b0 = (1.0f - b1) - b2;
                // corner r at the right angle, then the next two in the face's cyclic order
                const int32_t c0 = mesh_seli(k0, k1, k2, r), c1 = mesh_seli(k1, k2, k0, r), c2 = mesh_seli(k2, k0, k1, r);
                const float* __restrict__ A0 = a.points + (int64_t)c0 * 3;
                const float* __restrict__ A1 = a.points + (int64_t)c1 * 3;
                const float* __restrict__ A2 = a.points + (int64_t)c2 * 3;
                const float* __restrict__ N0 = a.normals + (int64_t)c0 * 3;
                const float* __restrict__ N1 = a.normals + (int64_t)c1 * 3;
                const float* __restrict__ N2 = a.normals + (int64_t)c2 * 3;
                const MeshBlend b = mesh_blend_views(a.s, mesh_mix(b0, b1, b2, A0[0], A1[0], A2[0]), mesh_mix(b0, b1, b2, A0[1], A1[1], A2[1]),
                                                     mesh_mix(b0, b1, b2, A0[2], A1[2], A2[2]), mesh_mix(b0, b1, b2, N0[0], N1[0], N2[0]),
                                                     mesh_mix(b0, b1, b2, N0[1], N1[1], N2[1]), mesh_mix(b0, b1, b2, N0[2], N1[2], N2[2]));
                float out0 = 0.0f, out1 = 0.0f, out2 = 0.0f;
                if (b.wsum > 0.0f) {
                    out0 = b.acc0 / b.wsum;
                    out1 = b.acc1 / b.wsum;
                    out2 = b.acc2 / b.wsum;
                } else if (a.fallback) {
                    const float* __restrict__ F0 = a.fallback + (int64_t)c0 * 3;
                    const float* __restrict__ F1 = a.fallback + (int64_t)c1 * 3;
                    const float* __restrict__ F2 = a.fallback + (int64_t)c2 * 3;
                    out0 = mesh_mix(b0, b1, b2, F0[0], F1[0], F2[0]);
                    out1 = mesh_mix(b0, b1, b2, F0[1], F1[1], F2[1]);
                    out2 = mesh_mix(b0, b1, b2, F0[2], F1[2], F2[2]);
                }
                t0 = mesh_u8(out0);
                t1 = mesh_u8(out1);
                t2 = mesh_u8(out2);
                seen = (uint8_t)b.seen;
            }
        } else if (lead && a.bad_faces) {
            atomicAdd(a.bad_faces, 1);                                         // an integer count on the error path: no output depends on it
        }
        if (lead) {
            if (a.corner) a.corner[f] = (uint8_t)r;
            if (a.uv) {
                const float fW = (float)a.Wt, fH = (float)a.Ht;
                for (int32_t k = 0; k < 3; ++k) {
                    const int32_t slot = k >= r ? k - r : k - r + 3;             // where corner k went: 0 = the right angle
                    const int32_t lx = upper ? (slot == 1 ? 2 : T - 1) : (slot == 1 ? T - 2 : 0);
                    const int32_t ly = upper ? (slot == 2 ? 2 : T - 1) : (slot == 2 ? T - 2 : 0);
                    a.uv[f * 6 + k * 2] = ((float)(x0 + lx) + 0.5f) / fW;
                    a.uv[f * 6 + k * 2 + 1] = ((float)(y0 + ly) + 0.5f) / fH;
                }
            }
        }
    }
    if (a.texture) {
        a.texture[o * 3] = t0;
        a.texture[o * 3 + 1] = t1;
        a.texture[o * 3 + 2] = t2;
    }
    if (a.views) a.views[o] = seen;
}

bool mesh_finite(float v) { return v == v && v - v == 0.0f; }

// per_row = ceil(sqrt(nb)) in integers
int64_t mesh_ceil_sqrt(int64_t nb) {
    int64_t r = (int64_t)sqrt((double)nb);
    while (r * r < nb) ++r;
    while (r > 0 && (r - 1) * (r - 1) >= nb) --r;
    return r;
}

}  // namespace

extern "C" int eg3d_mesh_texture_size(int64_t F, int32_t tile, int32_t* Ht, int32_t* Wt) {
    if (F < 0 || tile < 4 || tile > 64 || Ht == nullptr || Wt == nullptr) return EG3D_ERR_INVALID;
    if (F > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    const int64_t nb = F == 0 ? 1 : (F + 1) / 2;
    const int64_t per_row = mesh_ceil_sqrt(nb), rows = (nb + per_row - 1) / per_row;
    if (per_row * tile > 16384 || rows * tile > 16384) return EG3D_ERR_UNSUPPORTED;
    *Wt = (int32_t)(per_row * tile);
    *Ht = (int32_t)(rows * tile);
    return EG3D_OK;
}

extern "C" int eg3d_mesh_texture(const eg3d_mesh_texture_params* p, void* stream) {
    if (p == nullptr || p->V < 0 || p->F < 0 || p->N < 1 || p->H < 1 || p->R < 1) return EG3D_ERR_INVALID;
    if (p->cams == nullptr || p->images == nullptr || p->depth == nullptr || p->mask == nullptr) return EG3D_ERR_INVALID;
    if (!(p->depth_tol >= 0.0f) || !mesh_finite(p->depth_tol) || !(p->cos_min >= 0.0f && p->cos_min < 1.0f)) return EG3D_ERR_INVALID;
    if (p->power < 1 || p->power > 8) return EG3D_ERR_INVALID;
    if (p->tile < 4 || p->tile > 64 || p->fill < 0 || p->fill > 255) return EG3D_ERR_INVALID;
    if (p->F > 0 && p->faces == nullptr) return EG3D_ERR_INVALID;
    if (p->V > 0 && (p->points == nullptr || p->normals == nullptr)) return EG3D_ERR_INVALID;
    if (p->N > 255 || p->H > 16384 || p->R > 16384) return EG3D_ERR_UNSUPPORTED;
    if (p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    int32_t Ht = 0, Wt = 0;
    const int rc = eg3d_mesh_texture_size(p->F, p->tile, &Ht, &Wt);
    if (rc != EG3D_OK) return rc;
    if (p->texture == nullptr && p->views == nullptr && p->uv == nullptr && p->corner == nullptr && p->bad_faces == nullptr) return EG3D_OK;
    TextureArgs a;
    a.s = MeshViews{p->cams, p->images, p->depth, p->mask, p->N, p->H, p->R, p->depth_tol, p->cos_min, p->power};
    a.points = p->points;
    a.normals = p->normals;
    a.faces = p->faces;
    a.fallback = p->fallback;
    a.texture = p->texture;
    a.views = p->views;
    a.uv = p->uv;
    a.corner = p->corner;
    a.bad_faces = p->bad_faces;
    a.V = p->V;
    a.F = p->F;
    a.texels = (int64_t)Ht * Wt;
    a.T = p->tile;
    a.per_row = Wt / p->tile;
    a.Ht = Ht;
    a.Wt = Wt;
    a.fill = p->fill;
    if (p->bad_faces) {
        hipLaunchKernelGGL(mesh_texture_clear_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->bad_faces);
        EG3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mesh_texture_kernel, dim3((unsigned)((a.texels + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_mesh_normals(const eg3d_mesh_normals_params* p, void* stream) {
    if (p == nullptr || p->vol == nullptr || p->V < 0) return EG3D_ERR_INVALID;
    if (p->D0 < 2 || p->D1 < 2 || p->D2 < 2) return EG3D_ERR_INVALID;
    int seen = 0;
    for (int i = 0; i < 3; ++i) {
        if (p->axes[i] < 0 || p->axes[i] > 2) return EG3D_ERR_INVALID;
        seen |= 1 << p->axes[i];
        if (!mesh_finite(p->spacing[i]) || p->spacing[i] == 0.0f || !mesh_finite(p->origin[i])) return EG3D_ERR_INVALID;
    }
    if (seen != 7) return EG3D_ERR_INVALID;
    if ((int64_t)p->D0 * p->D1 * p->D2 > INT32_MAX || p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if (p->V == 0) return EG3D_OK;
    if (p->points == nullptr || p->normals == nullptr) return EG3D_ERR_INVALID;
    NormalArgs a;
    a.g.vol = p->vol;
    a.g.D0 = p->D0;
    a.g.D1 = p->D1;
    a.g.D2 = p->D2;
    a.g.S = p->D1 * p->D2;
    a.g.h0 = (float)(p->D0 - 1);
    a.g.h1 = (float)(p->D1 - 1);
    a.g.h2 = (float)(p->D2 - 1);
    a.points = p->points;
    a.normals = p->normals;
    a.V = p->V;
    a.ax0 = p->axes[0];
    a.ax1 = p->axes[1];
    a.ax2 = p->axes[2];
    a.org0 = p->origin[0];
    a.org1 = p->origin[1];
    a.org2 = p->origin[2];
    a.sp0 = p->spacing[0];
    a.sp1 = p->spacing[1];
    a.sp2 = p->spacing[2];
    hipLaunchKernelGGL(mesh_normals_kernel, dim3((unsigned)((p->V + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_mesh_bake(const eg3d_mesh_bake_params* p, void* stream) {
    if (p == nullptr || p->V < 0 || p->F < 1 || p->H < 1 || p->R < 1) return EG3D_ERR_INVALID;
    if (p->cams == nullptr || p->images == nullptr || p->depth == nullptr || p->mask == nullptr) return EG3D_ERR_INVALID;
    if (!(p->depth_tol >= 0.0f) || !mesh_finite(p->depth_tol) || !(p->cos_min >= 0.0f && p->cos_min < 1.0f)) return EG3D_ERR_INVALID;
    if (p->power < 1 || p->power > 8) return EG3D_ERR_INVALID;
    if (p->F > 255 || p->H > 16384 || p->R > 16384) return EG3D_ERR_UNSUPPORTED;
    if (p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if (p->V == 0) return EG3D_OK;
    if (p->points == nullptr || p->normals == nullptr) return EG3D_ERR_INVALID;
    BakeArgs a;
    a.s = MeshViews{p->cams, p->images, p->depth, p->mask, p->F, p->H, p->R, p->depth_tol, p->cos_min, p->power};
    a.points = p->points;
    a.normals = p->normals;
    a.fallback = p->fallback;
    a.color = p->color;
    a.rgb = p->rgb;
    a.weight = p->weight;
    a.views = p->views;
    a.V = p->V;
    hipLaunchKernelGGL(mesh_bake_kernel, dim3((unsigned)((p->V + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
