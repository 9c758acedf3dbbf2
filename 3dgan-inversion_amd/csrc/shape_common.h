// The one copy of what the shape and mesh family shares (include/eg3d_hip.h "Shape views", "Mesh attributes", "Mesh texture", "Mesh previews"):
// the clamped trilinear field of a regular fp32 grid, the world-to-grid frame, the field-gradient normal and the maps of the 25-float camera
// vector.  csrc/iso_render.hip, csrc/mesh_bake.hip and csrc/mesh_raster.hip call these and keep only what is specific to them.
// The arithmetic is the header's specification operation for operation: tests/support/{iso,mesh,raster}_ref.py restate it and the outputs are
// compared bit for bit, so nothing here may be reassociated, contracted or replaced by a reciprocal, and a ternary stays a ternary.
#pragma once
#include "common.h"

namespace shape {

// ---- small arithmetic ----
__device__ __forceinline__ float clamp(float p, float h) {
    p = p > 0.0f ? p : 0.0f;                          // NaN -> 0
    return p < h ? p : h;
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ float lerp_clamped(float a, float b, float f) {
    float r = a + f * (b - a);
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    r = r < lo ? lo : r;
    r = r > hi ? hi : r;
    return r;
}

__device__ __forceinline__ float mix(float b0, float b1, float b2, float a0, float a1, float a2) { return (b0 * a0 + b1 * a1) + b2 * a2; }

__device__ __forceinline__ float sel(float v0, float v1, float v2, int32_t w) { return w == 0 ? v0 : (w == 1 ? v1 : v2); }
__device__ __forceinline__ int32_t sel(int32_t v0, int32_t v1, int32_t v2, int32_t w) { return w == 0 ? v0 : (w == 1 ? v1 : v2); }

__device__ __forceinline__ uint8_t u8(float x) { return (uint8_t)(int)fminf(fmaxf(x * 127.5f + 128.f, 0.f), 255.f); }      // truncation, as eg3d_image_grid_u8

inline bool finite(float v) { return v == v && v - v == 0.0f; }

// ---- the grid and its clamped trilinear field ----
struct Grid {
    const float* vol;
    int32_t D0, D1, D2, S;                            // S = D1 * D2
    float h0, h1, h2;                                 // D - 1
};

struct Cell {
    int32_t i0, i1, i2;
    float f0, f1, f2;
};

// p already clamped to [0, h]
__device__ __forceinline__ Cell cell(const Grid& g, float p0, float p1, float p2) {
    Cell c;
    c.i0 = min((int32_t)floorf(p0), g.D0 - 2);
    c.i1 = min((int32_t)floorf(p1), g.D1 - 2);
    c.i2 = min((int32_t)floorf(p2), g.D2 - 2);
    c.f0 = p0 - (float)c.i0;
    c.f1 = p1 - (float)c.i1;
    c.f2 = p2 - (float)c.i2;
    return c;
}

__device__ __forceinline__ float trilinear(const Grid& g, const Cell& c) {
    const float* __restrict__ q = g.vol + ((int64_t)c.i0 * g.S + (int64_t)c.i1 * g.D2 + c.i2);
    const float v000 = q[0], v001 = q[1], v010 = q[g.D2], v011 = q[g.D2 + 1];
    const float v100 = q[g.S], v101 = q[g.S + 1], v110 = q[g.S + g.D2], v111 = q[g.S + g.D2 + 1];
    const float c00 = lerp_clamped(v000, v001, c.f2), c01 = lerp_clamped(v010, v011, c.f2);
    const float c10 = lerp_clamped(v100, v101, c.f2), c11 = lerp_clamped(v110, v111, c.f2);
    const float c0 = lerp_clamped(c00, c01, c.f1), c1 = lerp_clamped(c10, c11, c.f1);
    return lerp_clamped(c0, c1, c.f0);
}

__device__ __forceinline__ float field(const Grid& g, float p0, float p1, float p2) {
    return trilinear(g, cell(g, clamp(p0, g.h0), clamp(p1, g.h1), clamp(p2, g.h2)));
}

// every D >= 2 (EG3D_ERR_INVALID otherwise), fewer than 2^31 points (EG3D_ERR_TOO_LARGE otherwise), in that order; fills g
inline int grid_fill(const float* vol, int32_t D0, int32_t D1, int32_t D2, Grid& g) {
    if (D0 < 2 || D1 < 2 || D2 < 2) return EG3D_ERR_INVALID;
    if ((int64_t)D0 * D1 * D2 > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.vol = vol;
    g.D0 = D0;
    g.D1 = D1;
    g.D2 = D2;
    g.S = D1 * D2;
    g.h0 = (float)(D0 - 1);
    g.h1 = (float)(D1 - 1);
    g.h2 = (float)(D2 - 1);
    return EG3D_OK;
}

// ---- the frame: grid index i of grid axis a sits at world coordinate org[a] + i * sp[a] of world axis ax[a] ----
struct Frame {
    int32_t ax0, ax1, ax2;
    float org0, org1, org2, sp0, sp1, sp2;
};

// world point -> index coordinates (not clamped)
__device__ __forceinline__ void world_to_index(const Frame& fr, float x0, float x1, float x2, float& r0, float& r1, float& r2) {
    r0 = (sel(x0, x1, x2, fr.ax0) - fr.org0) / fr.sp0;
    r1 = (sel(x0, x1, x2, fr.ax1) - fr.org1) / fr.sp1;
    r2 = (sel(x0, x1, x2, fr.ax2) - fr.org2) / fr.sp2;
}

// axes a permutation of 0..2, spacing finite and not 0, origin finite: false otherwise; fills fr
inline bool frame_fill(const int32_t* axes, const float* origin, const float* spacing, Frame& fr) {
    int seen = 0;
    for (int i = 0; i < 3; ++i) {
        if (axes[i] < 0 || axes[i] > 2) return false;
        seen |= 1 << axes[i];
        if (!finite(spacing[i]) || spacing[i] == 0.0f || !finite(origin[i])) return false;
    }
    if (seen != 7) return false;
    fr.ax0 = axes[0];
    fr.ax1 = axes[1];
    fr.ax2 = axes[2];
    fr.org0 = origin[0];
    fr.org1 = origin[1];
    fr.org2 = origin[2];
    fr.sp0 = spacing[0];
    fr.sp1 = spacing[1];
    fr.sp2 = spacing[2];
    return true;
}

// The field's gradient at the clamped index coordinates p from clamped +-1-voxel differences, negated (toward lower values) and scattered to
// the world axes; not normalised: the callers differ in which lengths they accept.
__device__ __forceinline__ void gradient_normal(const Grid& g, const Frame& fr, float p0, float p1, float p2, float n[3]) {
    const float u0 = clamp(p0 + 1.0f, g.h0), l0 = clamp(p0 - 1.0f, g.h0);
    const float u1 = clamp(p1 + 1.0f, g.h1), l1 = clamp(p1 - 1.0f, g.h1);
    const float u2 = clamp(p2 + 1.0f, g.h2), l2 = clamp(p2 - 1.0f, g.h2);
    const float g0 = (field(g, u0, p1, p2) - field(g, l0, p1, p2)) / ((u0 - l0) * fr.sp0);
    const float g1 = (field(g, p0, u1, p2) - field(g, p0, l1, p2)) / ((u1 - l1) * fr.sp1);
    const float g2 = (field(g, p0, p1, u2) - field(g, p0, p1, l2)) / ((u2 - l2) * fr.sp2);
    for (int w = 0; w < 3; ++w) n[w] = -(fr.ax0 == w ? g0 : (fr.ax1 == w ? g1 : g2));
}

// ---- the camera: c = cam2world [16] + intrinsics [9], the generator's conditioning vector ----
// centre of pixel (y, x) of a res x res frame -> the camera-space ray (xl, yl, 1)
__device__ __forceinline__ void pixel_to_local(const float* __restrict__ c, int32_t x, int32_t y, int32_t res, float& xl, float& yl) {
    const float fx = c[16], sk = c[17], cx = c[18], fy = c[20], cy = c[21];
    const float xc = ((float)x + 0.5f) / (float)res, yc = ((float)y + 0.5f) / (float)res;
    xl = (((xc - cx) + (cy * sk) / fy) - (sk * yc) / fy) / fx;
    yl = (yc - cy) / fy;
}

// the camera-space ray (xl, yl, 1) -> world origin o and unit direction d
__device__ __forceinline__ void local_to_world_dir(const float* __restrict__ c, float xl, float yl, float o[3], float d[3]) {
    for (int i = 0; i < 3; ++i) {
        const float w = ((c[4 * i] * xl + c[4 * i + 1] * yl) + c[4 * i + 2]) + c[4 * i + 3];
        o[i] = c[4 * i + 3];
        d[i] = w - o[i];
    }
    const float dn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int i = 0; i < 3; ++i) d[i] = d[i] / dn;
}

// world point p -> q = p - camera position and its camera-space coordinates
__device__ __forceinline__ void world_to_camera(const float* __restrict__ m, float p0, float p1, float p2, float& q0, float& q1, float& q2, float& c0,
                                                float& c1, float& c2) {
    q0 = p0 - m[3], q1 = p1 - m[7], q2 = p2 - m[11];
    c0 = (m[0] * q0 + m[4] * q1) + m[8] * q2;
    c1 = (m[1] * q0 + m[5] * q1) + m[9] * q2;
    c2 = (m[2] * q0 + m[6] * q1) + m[10] * q2;
}

// camera-space point -> normalised image coordinates (pixel centre (y, x) of a res x res frame sits at ((x + 0.5) / res, (y + 0.5) / res))
__device__ __forceinline__ void camera_to_image(const float* __restrict__ m, float c0, float c1, float c2, float& xc, float& yc) {
    const float fx = m[16], sk = m[17], cx = m[18], fy = m[20], cy = m[21];
    const float xl = c0 / c2, yl = c1 / c2;
    yc = yl * fy + cy;
    xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy;
}

// ambient + (1 - ambient) * max(0, n . -d) in [0, 1]
__device__ __forceinline__ float headlight(float ambient, const float n[3], const float d[3]) {
    float l = -((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]);
    l = l > 0.0f ? l : 0.0f;
    return ambient + (1.0f - ambient) * l;
}

}  // namespace shape
