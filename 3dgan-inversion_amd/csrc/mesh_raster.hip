// Mesh previews: a z-buffer rasteriser for the exported meshes (include/eg3d_hip.h "Mesh previews").
//
// Five launches on one stream, no host synchronise, no floating-point atomics:
//   raster_clear_kernel    the z-buffer to all ones, the counters to 0
//   raster_vertex_kernel   one thread per (view, vertex): projection and snap, once -- 16 bytes per projected vertex, which the face stage and
//                          the resolve stage read with one 16-byte load each
//   raster_face_kernel     one thread per (view, face): setup, cull, clamped bounding box.  A box of at most RASTER_SMALL x RASTER_SMALL pixels
//                          is walked by the lane itself (the millions of sub-pixel faces of a marching-cubes mesh: one or no pixel each).  A
//                          larger one is appended to a queue -- an integer atomic add; the queue's order depends on the schedule, the z-buffer
//                          does not, because an integer minimum is the same in every order
//   raster_large_kernel    a fixed grid of workgroups walks the queue; a workgroup takes a face, each of its four waves every fourth 8 x 8 tile
//                          of the box, one lane per pixel: no lane ever walks a large box alone and no wave waits for one that does
//   raster_resolve_kernel  one thread per pixel: the winner's weights again (the same device function, so the same bits) and the outputs
// The depth test is a 64-bit unsigned atomicMin on (bits(zp) << 32) | face: global_atomic_umin_x2 on gfx950, not a compare-and-swap loop.
// The camera maps, the headlight and the small arithmetic are csrc/shape_common.h's; its rule holds here too: the arithmetic is the header's
// specification operation for operation (tests/support/raster_ref.py restates it, the outputs are compared bit for bit).
#include "shape_common.h"

namespace {

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_SMALL = EG3D_RASTER_SMALL;
constexpr int RASTER_QUEUE_BLOCKS = 1024;              // 256 CUs x 4: enough workgroups in flight for any queue; an idle one reads one counter and ends
constexpr uint64_t RASTER_EMPTY = ~0ull;

// What one launch hands to the next through the workspace besides the projected vertices -- the z-buffer words, the queue and the counters --
// is written and read at agent scope (write-through stores, loads that bypass the CU's L1), like the atomics that work on it in between.
// Launch boundaries already order these accesses; the scope costs nothing measurable on words touched once.
#define RLOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define RSTORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct RasterVertex {                                  // 16 bytes: one load
    int32_t X, Y;
    float z;
    int32_t valid;
};

struct RasterArgs {
    const float* points;
    const int32_t* faces;
    const float* cams;
    const float* uv;
    const uint8_t* texture;
    const float* colors;
    const float* normals;
    int32_t* face;
    float* z;
    float* depth;
    uint8_t* mask;
    float* bary;
    float* image;
    int32_t* bad_faces;
    int32_t* stats;
    uint64_t* zbuf;                                    // [N][res][res]
    RasterVertex* sv;                                  // [N][V]
    int64_t* queue;                                    // [N * F]: (view << 32) | face
    int32_t* counters;                                 // [0] queue length, [1] faces drawn by the small path, [2] bad faces
    int64_t V, F, pixels;                              // pixels = res * res
    int32_t N, res, Ht, Wt, mode, cull;
    float near, background, ambient;
};

struct RasterFace {
    int32_t X0, Y0, X1, Y1, X2, Y2;
    float z0, z1, z2;
    float fa;                                          // float(|area2|)
    int64_t area2;
};

__global__ void __launch_bounds__(RASTER_THREADS) raster_clear_kernel(uint64_t* zbuf, int64_t n, int32_t* counters) {
    const int64_t stride = (int64_t)gridDim.x * RASTER_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x; i < n; i += stride) RSTORE(&zbuf[i], RASTER_EMPTY);
    if (blockIdx.x == 0 && threadIdx.x < 4) RSTORE(&counters[threadIdx.x], 0);
}

__global__ void __launch_bounds__(RASTER_THREADS) raster_vertex_kernel(RasterArgs a) {
    const int64_t v = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const int32_t n = (int32_t)blockIdx.y;
    const float* __restrict__ m = a.cams + (int64_t)n * 25;
    float q0, q1, q2, c0, c1, c2, xc, yc;
    shape::world_to_camera(m, a.points[v * 3], a.points[v * 3 + 1], a.points[v * 3 + 2], q0, q1, q2, c0, c1, c2);
    shape::camera_to_image(m, c0, c1, c2, xc, yc);
    const float fr = (float)a.res;
    const float px = xc * fr - 0.5f, py = yc * fr - 0.5f;
    RasterVertex o;
    o.valid = (c2 > a.near && px >= -32768.0f && px <= 32768.0f && py >= -32768.0f && py <= 32768.0f) ? 1 : 0;      // false for NaN
    o.X = o.valid ? (int32_t)floorf(px * 256.0f + 0.5f) : 0;
    o.Y = o.valid ? (int32_t)floorf(py * 256.0f + 0.5f) : 0;
    o.z = c2;
    a.sv[(int64_t)n * a.V + v] = o;
}

// int32 x int32 -> int64 from the two 32-bit halves (v_mul_hi_i32, v_mul_lo_u32), not (int64_t)a * b.  With the latter (v_mad_i64_i32 in the
// pixel loop, its carry-out naming a scalar register pair that a scalar move reuses two instructions later) the depth keys of whole runs of
// lanes came out wrong on gfx950 in about half of the launches, by factors that grow like powers of two from lane to lane; the resolve
// stage, which has no such loop, recomputed the right depth for the same face and pixel.  With this form 30 of 30 repeated launches and
// every case of tests/test_gpu_mesh_raster.py are exact.  The register reuse is what the two listings differ in; that it is the cause is
// a supposition (DESIGN.md 3.4 "Mesh previews").
__device__ __forceinline__ int64_t raster_mul(int32_t a, int32_t b) {
    return (int64_t)(((uint64_t)(uint32_t)__mulhi(a, b) << 32) | (uint64_t)((uint32_t)a * (uint32_t)b));
}

__device__ __forceinline__ int64_t raster_orient(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
    return raster_mul(bx - ax, py - ay) - raster_mul(by - ay, px - ax);
}

// the three vertices of face f in view n; false when an index lies outside [0, V) (never dereferenced) or a vertex is invalid in this view
__device__ __forceinline__ bool raster_load(const RasterArgs& a, int32_t n, int64_t f, RasterFace& t, bool& bad) {
    const int32_t k0 = a.faces[f * 3], k1 = a.faces[f * 3 + 1], k2 = a.faces[f * 3 + 2];
    bad = !(k0 >= 0 && k0 < a.V && k1 >= 0 && k1 < a.V && k2 >= 0 && k2 < a.V);
    if (bad) return false;
    const RasterVertex* __restrict__ sv = a.sv + (int64_t)n * a.V;
    const RasterVertex s0 = sv[k0], s1 = sv[k1], s2 = sv[k2];
    if (!(s0.valid && s1.valid && s2.valid)) return false;
    t.X0 = s0.X, t.Y0 = s0.Y, t.X1 = s1.X, t.Y1 = s1.Y, t.X2 = s2.X, t.Y2 = s2.Y;
    t.z0 = s0.z, t.z1 = s1.z, t.z2 = s2.z;
    t.area2 = raster_orient(t.X0, t.Y0, t.X1, t.Y1, t.X2, t.Y2);
    t.fa = (float)(t.area2 < 0 ? -t.area2 : t.area2);
    return true;
}

// coverage and perspective weights of pixel (y, x): the one copy, called by both draw paths and by the resolve stage
__device__ __forceinline__ bool raster_weights(const RasterFace& t, int32_t x, int32_t y, float& w0, float& w1, float& w2, float& W) {
    const int32_t PX = 256 * x, PY = 256 * y;
    int64_t E0 = raster_orient(t.X1, t.Y1, t.X2, t.Y2, PX, PY);
    int64_t E1 = raster_orient(t.X2, t.Y2, t.X0, t.Y0, PX, PY);
    int64_t E2 = raster_orient(t.X0, t.Y0, t.X1, t.Y1, PX, PY);
    if (t.area2 < 0) { E0 = -E0; E1 = -E1; E2 = -E2; }
    if (E0 < 0 || E1 < 0 || E2 < 0) return false;
    const float fa = t.fa;
    const float l0 = (float)E0 / fa, l1 = (float)E1 / fa, l2 = (float)E2 / fa;
    w0 = l0 / t.z0;
    w1 = l1 / t.z1;
    w2 = l2 / t.z2;
    W = (w0 + w1) + w2;
    return W > 0.0f && W < INFINITY;
}

__device__ __forceinline__ void raster_draw(const RasterFace& t, int32_t x, int32_t y, uint64_t* zrow, int32_t res, int64_t f) {
    float w0, w1, w2, W;
    if (!raster_weights(t, x, y, w0, w1, w2, W)) return;
    const float zp = 1.0f / W;
    const uint64_t key = ((uint64_t)__float_as_uint(zp) << 32) | (uint64_t)(uint32_t)f;
    atomicMin(reinterpret_cast<unsigned long long*>(zrow + (int64_t)y * res + x), (unsigned long long)key);
}

// the pixels whose centres (256 x, 256 y) can lie in the face: ceil(min / 256) .. floor(max / 256), clamped to the frame
__device__ __forceinline__ void raster_box(const RasterFace& t, int32_t res, int32_t& x0, int32_t& y0, int32_t& x1, int32_t& y1) {
    const int32_t lox = min(t.X0, min(t.X1, t.X2)), hix = max(t.X0, max(t.X1, t.X2));
    const int32_t loy = min(t.Y0, min(t.Y1, t.Y2)), hiy = max(t.Y0, max(t.Y1, t.Y2));
    x0 = max((lox + 255) >> 8, 0);
    y0 = max((loy + 255) >> 8, 0);
    x1 = min(hix >> 8, res - 1);
    y1 = min(hiy >> 8, res - 1);
}

__global__ void __launch_bounds__(RASTER_THREADS) raster_face_kernel(RasterArgs a) {
    const int64_t f = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    const int32_t n = (int32_t)blockIdx.y;
    RasterFace t;
    int32_t x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    bool live = false;
    if (f < a.F) {
        bool bad;
        live = raster_load(a, n, f, t, bad);
        if (bad && n == 0) atomicAdd(&a.counters[2], 1);                       // the error path: once per face, no output depends on it
        live = live && t.area2 != 0 && !(a.cull == 1 && t.area2 > 0);         // front faces have area2 < 0
        if (live) raster_box(t, a.res, x0, y0, x1, y1);
        live = live && x1 >= x0 && y1 >= y0;
    }
    const int32_t w = x1 - x0 + 1, h = y1 - y0 + 1;
    const bool small = live && w <= RASTER_SMALL && h <= RASTER_SMALL;
    if (live && !small) RSTORE(&a.queue[atomicAdd(&a.counters[0], 1)], ((int64_t)n << 32) | f);      // at most N * F entries: the queue's size
    const unsigned long long ballot = __ballot(small);
    if (ballot != 0 && (threadIdx.x & 63) == (unsigned)__ffsll((long long)ballot) - 1) atomicAdd(&a.counters[1], __popcll(ballot));
    if (!small) return;
    uint64_t* zb = a.zbuf + (int64_t)n * a.pixels;
    for (int32_t y = y0; y <= y1; ++y)
        for (int32_t x = x0; x <= x1; ++x) raster_draw(t, x, y, zb, a.res, f);
}

__global__ void __launch_bounds__(RASTER_THREADS) raster_large_kernel(RasterArgs a) {
    const int32_t count = RLOAD(&a.counters[0]);
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t lx = lane & 7, ly = lane >> 3;
    for (int32_t i = (int32_t)blockIdx.x; i < count; i += (int32_t)gridDim.x) {
        const int64_t e = RLOAD(&a.queue[i]);
        const int32_t n = (int32_t)(e >> 32);
        const int64_t f = e & 0x7fffffff;
        RasterFace t;
        bool bad;
        if (!raster_load(a, n, f, t, bad)) continue;                           // cannot happen for a queued face; uniform over the workgroup
        int32_t x0, y0, x1, y1;
        raster_box(t, a.res, x0, y0, x1, y1);
        const int32_t tw = (x1 - x0 + 8) >> 3, th = (y1 - y0 + 8) >> 3;
        uint64_t* zb = a.zbuf + (int64_t)n * a.pixels;
        for (int32_t tile = wave; tile < tw * th; tile += RASTER_THREADS / 64) {
            const int32_t ty = tile / tw, tx = tile - ty * tw;
            const int32_t x = x0 + tx * 8 + lx, y = y0 + ty * 8 + ly;
            if (x <= x1 && y <= y1) raster_draw(t, x, y, zb, a.res, f);
        }
    }
}

__global__ void __launch_bounds__(RASTER_THREADS) raster_resolve_kernel(RasterArgs a) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (a.bad_faces) *a.bad_faces = RLOAD(&a.counters[2]);
        if (a.stats) {
            a.stats[0] = RLOAD(&a.counters[1]);
            a.stats[1] = RLOAD(&a.counters[0]);
        }
    }
    const int64_t p = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (p >= a.pixels) return;
    const int32_t n = (int32_t)blockIdx.y;
    const int32_t y = (int32_t)(p / a.res), x = (int32_t)(p - (int64_t)y * a.res);
    const int64_t pix = (int64_t)n * a.pixels + p;
    const uint64_t key = RLOAD(&a.zbuf[pix]);
    const bool hit = key != RASTER_EMPTY;
    int64_t f = -1;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, W = 1.0f;
    if (hit) {
        f = (int64_t)(uint32_t)key;
        RasterFace t;
        bool bad;
        raster_load(a, n, f, t, bad);                                          // a face that won a pixel passed every test of the face stage
        raster_weights(t, x, y, w0, w1, w2, W);
    }
    const float zp = hit ? 1.0f / W : 0.0f;
    const float b0 = hit ? w0 / W : 0.0f, b1 = hit ? w1 / W : 0.0f, b2 = hit ? w2 / W : 0.0f;
    if (a.face) a.face[pix] = (int32_t)f;
    if (a.z) a.z[pix] = zp;
    if (a.mask) a.mask[pix] = hit ? 1 : 0;
    if (a.bary) {
        a.bary[pix * 3] = b0;
        a.bary[pix * 3 + 1] = b1;
        a.bary[pix * 3 + 2] = b2;
    }
    const bool need_ray = a.depth != nullptr || (a.image != nullptr && a.mode == EG3D_RASTER_LAMBERT);
    float xl = 0.0f, yl = 0.0f;
    const float* __restrict__ c = a.cams + (int64_t)n * 25;
    if (need_ray) shape::pixel_to_local(c, x, y, a.res, xl, yl);
    if (a.depth) a.depth[pix] = hit ? zp * sqrtf((xl * xl + yl * yl) + 1.0f) : 0.0f;
    if (!a.image) return;
    float s0 = a.background, s1 = a.background, s2 = a.background;
    if (hit) {
        const int32_t k0 = a.faces[f * 3], k1 = a.faces[f * 3 + 1], k2 = a.faces[f * 3 + 2];
        if (a.mode == EG3D_RASTER_TEXTURE) {
            const float* __restrict__ A = a.uv + f * 6;
            const float u = shape::mix(b0, b1, b2, A[0], A[2], A[4]), v = shape::mix(b0, b1, b2, A[1], A[3], A[5]);
            const float tx = shape::clamp(u * (float)a.Wt - 0.5f, (float)(a.Wt - 1)), ty = shape::clamp(v * (float)a.Ht - 0.5f, (float)(a.Ht - 1));
            const int32_t ix = min((int32_t)floorf(tx), a.Wt - 2), iy = min((int32_t)floorf(ty), a.Ht - 2);
            const float gx = tx - (float)ix, gy = ty - (float)iy;
            const uint8_t* __restrict__ r0 = a.texture + ((int64_t)iy * a.Wt + ix) * 3;
            const uint8_t* __restrict__ r1 = r0 + (int64_t)a.Wt * 3;
            float col[3];
            for (int j = 0; j < 3; ++j) {
                col[j] = shape::lerp(shape::lerp((float)r0[j], (float)r0[3 + j], gx), shape::lerp((float)r1[j], (float)r1[3 + j], gx), gy);
                col[j] = (col[j] - 127.5f) / 127.5f;
            }
            s0 = col[0], s1 = col[1], s2 = col[2];
        } else if (a.mode == EG3D_RASTER_VERTEX) {
            const float* __restrict__ C0 = a.colors + (int64_t)k0 * 3;
            const float* __restrict__ C1 = a.colors + (int64_t)k1 * 3;
            const float* __restrict__ C2 = a.colors + (int64_t)k2 * 3;
            s0 = shape::mix(b0, b1, b2, C0[0], C1[0], C2[0]);
            s1 = shape::mix(b0, b1, b2, C0[1], C1[1], C2[1]);
            s2 = shape::mix(b0, b1, b2, C0[2], C1[2], C2[2]);
        } else {
            const float* __restrict__ N0 = a.normals + (int64_t)k0 * 3;
            const float* __restrict__ N1 = a.normals + (int64_t)k1 * 3;
            const float* __restrict__ N2 = a.normals + (int64_t)k2 * 3;
            float nn[3];
            for (int j = 0; j < 3; ++j) nn[j] = shape::mix(b0, b1, b2, N0[j], N1[j], N2[j]);
            const float len = sqrtf((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
            const bool ok = len > 0.0f && len < INFINITY;
            for (int j = 0; j < 3; ++j) nn[j] = ok ? nn[j] / len : 0.0f;
            float o[3], d[3];
            shape::local_to_world_dir(c, xl, yl, o, d);
            const float v = shape::headlight(a.ambient, nn, d);
            s0 = s1 = s2 = v * 2.0f - 1.0f;
        }
    }
    float* __restrict__ ip = a.image + (int64_t)n * 3 * a.pixels + p;
    ip[0] = s0;
    ip[a.pixels] = s1;
    ip[2 * a.pixels] = s2;
}

int64_t raster_align(int64_t b) { return (b + 15) & ~(int64_t)15; }

struct RasterLayout {
    int64_t zbuf, sv, queue, counters, total;
};

// validates everything but the workspace; fills the workspace layout
int raster_check(const eg3d_mesh_raster_params* p, RasterLayout& l) {
    if (p == nullptr || p->V < 0 || p->F < 0 || p->N < 1 || p->res < 1) return EG3D_ERR_INVALID;
    if (!(p->near > 0.0f) || !shape::finite(p->near) || !(p->ambient >= 0.0f && p->ambient <= 1.0f)) return EG3D_ERR_INVALID;
    if (p->cull != 0 && p->cull != 1) return EG3D_ERR_INVALID;
    if (p->mode != EG3D_RASTER_TEXTURE && p->mode != EG3D_RASTER_VERTEX && p->mode != EG3D_RASTER_LAMBERT) return EG3D_ERR_INVALID;
    if (p->cams == nullptr || (p->V > 0 && p->points == nullptr) || (p->F > 0 && p->faces == nullptr)) return EG3D_ERR_INVALID;
    if (p->mode == EG3D_RASTER_TEXTURE && (p->texture == nullptr || p->Ht < 2 || p->Wt < 2 || (p->F > 0 && p->uv == nullptr))) return EG3D_ERR_INVALID;
    if (p->mode == EG3D_RASTER_VERTEX && p->V > 0 && p->colors == nullptr) return EG3D_ERR_INVALID;
    if (p->mode == EG3D_RASTER_LAMBERT && p->V > 0 && p->normals == nullptr) return EG3D_ERR_INVALID;
    if (p->res > 16384 || p->N > 65535) return EG3D_ERR_UNSUPPORTED;
    if (p->mode == EG3D_RASTER_TEXTURE && (p->Ht > 16384 || p->Wt > 16384)) return EG3D_ERR_UNSUPPORTED;
    if (p->V > INT32_MAX || p->F > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if ((int64_t)p->N * p->F > INT32_MAX) return EG3D_ERR_TOO_LARGE;           // the queue's length is an int32 counter
    l.zbuf = 0;
    l.sv = l.zbuf + raster_align((int64_t)p->N * p->res * p->res * 8);
    l.queue = l.sv + raster_align((int64_t)p->N * p->V * 16);
    l.counters = l.queue + raster_align((int64_t)p->N * p->F * 8);
    l.total = l.counters + 16;
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_mesh_raster_query_workspace(const eg3d_mesh_raster_params* p, int64_t* workspace_bytes) {
    RasterLayout l;
    const int rc = raster_check(p, l);
    if (rc != EG3D_OK) return rc;
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    *workspace_bytes = l.total;
    return EG3D_OK;
}

extern "C" int eg3d_mesh_raster(const eg3d_mesh_raster_params* p, void* stream) {
    RasterLayout l;
    const int rc = raster_check(p, l);
    if (rc != EG3D_OK) return rc;
    if (p->workspace == nullptr || ((uintptr_t)p->workspace & 15) != 0 || p->workspace_bytes < l.total) return EG3D_ERR_INVALID;
    if (p->face == nullptr && p->z == nullptr && p->depth == nullptr && p->mask == nullptr && p->bary == nullptr && p->image == nullptr &&
        p->bad_faces == nullptr && p->stats == nullptr)
        return EG3D_OK;
    char* ws = (char*)p->workspace;
    RasterArgs a;
    a.points = p->points;
    a.faces = p->faces;
    a.cams = p->cams;
    a.uv = p->uv;
    a.texture = p->texture;
    a.colors = p->colors;
    a.normals = p->normals;
    a.face = p->face;
    a.z = p->z;
    a.depth = p->depth;
    a.mask = p->mask;
    a.bary = p->bary;
    a.image = p->image;
    a.bad_faces = p->bad_faces;
    a.stats = p->stats;
    a.zbuf = (uint64_t*)(ws + l.zbuf);
    a.sv = (RasterVertex*)(ws + l.sv);
    a.queue = (int64_t*)(ws + l.queue);
    a.counters = (int32_t*)(ws + l.counters);
    a.V = p->V;
    a.F = p->F;
    a.pixels = (int64_t)p->res * p->res;
    a.N = p->N;
    a.res = p->res;
    a.Ht = p->Ht;
    a.Wt = p->Wt;
    a.mode = p->mode;
    a.cull = p->cull;
    a.near = p->near;
    a.background = p->background;
    a.ambient = p->ambient;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = (int64_t)p->N * a.pixels;
    const int64_t clear_blocks = (cells + RASTER_THREADS - 1) / RASTER_THREADS;
    hipLaunchKernelGGL(raster_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(RASTER_THREADS), 0, s, a.zbuf, cells, a.counters);
    EG3D_LAUNCH_CHECK();
    if (p->F > 0) {
        if (p->V > 0) {
            hipLaunchKernelGGL(raster_vertex_kernel, dim3((unsigned)((p->V + RASTER_THREADS - 1) / RASTER_THREADS), (unsigned)p->N), dim3(RASTER_THREADS), 0, s, a);
            EG3D_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(raster_face_kernel, dim3((unsigned)((p->F + RASTER_THREADS - 1) / RASTER_THREADS), (unsigned)p->N), dim3(RASTER_THREADS), 0, s, a);
        EG3D_LAUNCH_CHECK();
        const int64_t most = (int64_t)p->N * p->F;
        hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)(most < RASTER_QUEUE_BLOCKS ? most : RASTER_QUEUE_BLOCKS)), dim3(RASTER_THREADS), 0, s, a);
        EG3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((a.pixels + RASTER_THREADS - 1) / RASTER_THREADS), (unsigned)p->N), dim3(RASTER_THREADS), 0, s, a);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
