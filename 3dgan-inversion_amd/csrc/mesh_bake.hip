// Mesh attributes: per-vertex normals of the density field and view-baked vertex colours (include/eg3d_hip.h "Mesh attributes").
//
// Two kernels, one thread per vertex, nothing shared between threads and no atomics: every output is a function of its own vertex.
//   mesh_normals_kernel  the gradient of the trilinear field at the vertex (24 field evaluations of 8 loads each; neighbouring vertices
//                        read neighbouring cells).
//   mesh_bake_kernel     walks the views in index order: projection, four depth taps, four image taps per channel.  Vertices arrive ordered
//                        by owning grid point (mc_emit), so a wave projects to neighbouring pixels and its gathers share cache lines.  The view
//                        index is uniform over the launch, so the 25 camera floats of a view are uniform loads, not one load per lane.
//   mesh_texture_kernel  one thread per texel of the per-face atlas ("Mesh texture"): decodes its face and barycentrics, interpolates the
//                        face's three vertices and runs the same view loop (mesh_blend_views, the one copy).
// The field, the frame, the normal and the camera maps are csrc/shape_common.h's; its rule holds here too: the arithmetic is the header's
// specification operation for operation (tests/support/mesh_ref.py restates it, the outputs are compared bit for bit).
#include "shape_common.h"

namespace {

constexpr int MESH_THREADS = 256;

struct NormalArgs {
    shape::Grid g;
    const float* points;
    float* normals;
    int64_t V;
    shape::Frame fr;
};

__global__ void __launch_bounds__(MESH_THREADS) mesh_normals_kernel(NormalArgs a) {
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const shape::Grid& g = a.g;
    float r0, r1, r2;
    shape::world_to_index(a.fr, a.points[v * 3], a.points[v * 3 + 1], a.points[v * 3 + 2], r0, r1, r2);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (r0 == r0 && r1 == r1 && r2 == r2) {           // a NaN index coordinate: no normal (the clamp would send it to index 0)
        shape::gradient_normal(g, a.fr, shape::clamp(r0, g.h0), shape::clamp(r1, g.h1), shape::clamp(r2, g.h2), n);
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
        float q0, q1, q2, c0, c1, c2, xc, yc;
        shape::world_to_camera(m, p0, p1, p2, q0, q1, q2, c0, c1, c2);
        const float t = sqrtf((q0 * q0 + q1 * q1) + q2 * q2);
        if (!(t > 0.0f && c2 > 0.0f)) continue;
        shape::camera_to_image(m, c0, c1, c2, xc, yc);
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
            col0 = shape::lerp(shape::lerp(s[0], s[1], tx), shape::lerp(s[a.H], s[a.H + 1], tx), ty);
            s += planeH;
            col1 = shape::lerp(shape::lerp(s[0], s[1], tx), shape::lerp(s[a.H], s[a.H + 1], tx), ty);
            s += planeH;
            col2 = shape::lerp(shape::lerp(s[0], s[1], tx), shape::lerp(s[a.H], s[a.H + 1], tx), ty);
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
        a.rgb[v * 3] = shape::u8(out0);
        a.rgb[v * 3 + 1] = shape::u8(out1);
        a.rgb[v * 3 + 2] = shape::u8(out2);
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
                const int32_t c0 = shape::sel(k0, k1, k2, r), c1 = shape::sel(k1, k2, k0, r), c2 = shape::sel(k2, k0, k1, r);
                const float* __restrict__ A0 = a.points + (int64_t)c0 * 3;
                const float* __restrict__ A1 = a.points + (int64_t)c1 * 3;
                const float* __restrict__ A2 = a.points + (int64_t)c2 * 3;
                const float* __restrict__ N0 = a.normals + (int64_t)c0 * 3;
                const float* __restrict__ N1 = a.normals + (int64_t)c1 * 3;
                const float* __restrict__ N2 = a.normals + (int64_t)c2 * 3;
                const MeshBlend b = mesh_blend_views(a.s, shape::mix(b0, b1, b2, A0[0], A1[0], A2[0]), shape::mix(b0, b1, b2, A0[1], A1[1], A2[1]),
                                                     shape::mix(b0, b1, b2, A0[2], A1[2], A2[2]), shape::mix(b0, b1, b2, N0[0], N1[0], N2[0]),
                                                     shape::mix(b0, b1, b2, N0[1], N1[1], N2[1]), shape::mix(b0, b1, b2, N0[2], N1[2], N2[2]));
                float out0 = 0.0f, out1 = 0.0f, out2 = 0.0f;
                if (b.wsum > 0.0f) {
                    out0 = b.acc0 / b.wsum;
                    out1 = b.acc1 / b.wsum;
                    out2 = b.acc2 / b.wsum;
                } else if (a.fallback) {
                    const float* __restrict__ F0 = a.fallback + (int64_t)c0 * 3;
                    const float* __restrict__ F1 = a.fallback + (int64_t)c1 * 3;
                    const float* __restrict__ F2 = a.fallback + (int64_t)c2 * 3;
                    out0 = shape::mix(b0, b1, b2, F0[0], F1[0], F2[0]);
                    out1 = shape::mix(b0, b1, b2, F0[1], F1[1], F2[1]);
                    out2 = shape::mix(b0, b1, b2, F0[2], F1[2], F2[2]);
                }
                t0 = shape::u8(out0);
                t1 = shape::u8(out1);
                t2 = shape::u8(out2);
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

// what eg3d_mesh_bake (P::F views) and eg3d_mesh_texture (P::N views) ask of their views: `count` is that number; fills s
template <class P>
int mesh_views(const P* p, int32_t count, MeshViews& s) {
    if (count < 1 || p->H < 1 || p->R < 1) return EG3D_ERR_INVALID;
    if (p->cams == nullptr || p->images == nullptr || p->depth == nullptr || p->mask == nullptr) return EG3D_ERR_INVALID;
    if (!(p->depth_tol >= 0.0f) || !shape::finite(p->depth_tol) || !(p->cos_min >= 0.0f && p->cos_min < 1.0f)) return EG3D_ERR_INVALID;
    if (p->power < 1 || p->power > 8) return EG3D_ERR_INVALID;
    if (count > 255 || p->H > 16384 || p->R > 16384) return EG3D_ERR_UNSUPPORTED;
    s = MeshViews{p->cams, p->images, p->depth, p->mask, count, p->H, p->R, p->depth_tol, p->cos_min, p->power};
    return EG3D_OK;
}

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
    if (p == nullptr || p->V < 0 || p->F < 0) return EG3D_ERR_INVALID;
    if (p->tile < 4 || p->tile > 64 || p->fill < 0 || p->fill > 255) return EG3D_ERR_INVALID;
    if (p->F > 0 && p->faces == nullptr) return EG3D_ERR_INVALID;
    if (p->V > 0 && (p->points == nullptr || p->normals == nullptr)) return EG3D_ERR_INVALID;
    TextureArgs a;
    int rc = mesh_views(p, p->N, a.s);                // after the entry's own invalid arguments: every EG3D_ERR_INVALID precedes EG3D_ERR_UNSUPPORTED
    if (rc != EG3D_OK) return rc;
    if (p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    int32_t Ht = 0, Wt = 0;
    rc = eg3d_mesh_texture_size(p->F, p->tile, &Ht, &Wt);
    if (rc != EG3D_OK) return rc;
    if (p->texture == nullptr && p->views == nullptr && p->uv == nullptr && p->corner == nullptr && p->bad_faces == nullptr) return EG3D_OK;
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
    NormalArgs a;
    const int gs = shape::grid_fill(p->vol, p->D0, p->D1, p->D2, a.g);
    if (gs == EG3D_ERR_INVALID) return gs;
    if (!shape::frame_fill(p->axes, p->origin, p->spacing, a.fr)) return EG3D_ERR_INVALID;      // a bad frame is reported before a grid that is too large
    if (gs != EG3D_OK || p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if (p->V == 0) return EG3D_OK;
    if (p->points == nullptr || p->normals == nullptr) return EG3D_ERR_INVALID;
    a.points = p->points;
    a.normals = p->normals;
    a.V = p->V;
    hipLaunchKernelGGL(mesh_normals_kernel, dim3((unsigned)((p->V + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_mesh_bake(const eg3d_mesh_bake_params* p, void* stream) {
    if (p == nullptr || p->V < 0) return EG3D_ERR_INVALID;
    BakeArgs a;
    const int rc = mesh_views(p, p->F, a.s);
    if (rc != EG3D_OK) return rc;
    if (p->V > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if (p->V == 0) return EG3D_OK;
    if (p->points == nullptr || p->normals == nullptr) return EG3D_ERR_INVALID;
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
