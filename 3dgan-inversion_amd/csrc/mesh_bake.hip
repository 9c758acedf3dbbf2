// Mesh attributes: per-vertex normals of the density field and view-baked vertex colours (include/eg3d_hip.h "Mesh attributes").
//
// Two kernels, one thread per vertex, nothing shared between threads and no atomics: every output is a function of its own vertex.
//   mesh_normals_kernel  the gradient of the trilinear field at the vertex (24 field evaluations of 8 loads each; neighbouring vertices
//                        read neighbouring cells).  The field functions restate csrc/iso_render.hip's: that file stays as it is.
//   mesh_bake_kernel     walks the views in index order: projection, four depth taps, four image taps per channel.  Vertices arrive ordered
//                        by owning grid point (mc_emit), so a wave projects to neighbouring pixels and its gathers share cache lines.  The view
//                        index is uniform over the launch, so the 25 camera floats of a view are uniform loads, not one load per lane.
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

struct BakeArgs {
    const float* points;
    const float* normals;
    const float* cams;
    const float* images;
    const float* depth;
    const uint8_t* mask;
    const float* fallback;
    float* color;
    uint8_t* rgb;
    float* weight;
    uint8_t* views;
    int64_t V;
    int32_t F, H, R;
    float depth_tol, cos_min;
    int32_t power;
};

__device__ __forceinline__ float mesh_lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ bool mesh_inside(float p, float hi) { return p >= 0.0f && p <= hi; }      // false for NaN

__global__ void __launch_bounds__(MESH_THREADS) mesh_bake_kernel(BakeArgs a) {
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const float p0 = a.points[v * 3], p1 = a.points[v * 3 + 1], p2 = a.points[v * 3 + 2];
    const float n0 = a.normals[v * 3], n1 = a.normals[v * 3 + 1], n2 = a.normals[v * 3 + 2];
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
    float out0 = 0.0f, out1 = 0.0f, out2 = 0.0f;
    if (wsum > 0.0f) {
        out0 = acc0 / wsum;
        out1 = acc1 / wsum;
        out2 = acc2 / wsum;
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
        a.rgb[v * 3] = (uint8_t)(int)fminf(fmaxf(out0 * 127.5f + 128.f, 0.f), 255.f);          // truncation, as eg3d_image_grid_u8
        a.rgb[v * 3 + 1] = (uint8_t)(int)fminf(fmaxf(out1 * 127.5f + 128.f, 0.f), 255.f);
        a.rgb[v * 3 + 2] = (uint8_t)(int)fminf(fmaxf(out2 * 127.5f + 128.f, 0.f), 255.f);
    }
    if (a.weight) a.weight[v] = wsum;
    if (a.views) a.views[v] = (uint8_t)seen;
}

bool mesh_finite(float v) { return v == v && v - v == 0.0f; }

}  // namespace

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
    a.points = p->points;
    a.normals = p->normals;
    a.cams = p->cams;
    a.images = p->images;
    a.depth = p->depth;
    a.mask = p->mask;
    a.fallback = p->fallback;
    a.color = p->color;
    a.rgb = p->rgb;
    a.weight = p->weight;
    a.views = p->views;
    a.V = p->V;
    a.F = p->F;
    a.H = p->H;
    a.R = p->R;
    a.depth_tol = p->depth_tol;
    a.cos_min = p->cos_min;
    a.power = p->power;
    hipLaunchKernelGGL(mesh_bake_kernel, dim3((unsigned)((p->V + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
