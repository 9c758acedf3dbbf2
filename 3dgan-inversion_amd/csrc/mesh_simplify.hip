// Mesh simplification (vertex clustering) and Taubin smoothing (include/eg3d_hip.h "Mesh simplification and smoothing").
//
// Simplify: five entries with the caller's sorts and prefix sums between them (torch.sort(stable=True) and cumsum are plumbing; every value
// they order or add is an integer, so their results are unique).  One thread per vertex, per cluster or per face; a thread writes words no
// other thread writes, except the flag and `used` words, where every writer stores the same 1.  No atomics, no LDS, no det.h.
//   ms_keys      vertex -> cell -> int64 key, invalid vertices flagged            (sort by key, stable: members of a cluster ascend)
//   ms_heads     heads[i] = sorted key i opens a cluster                          (inclusive scan: rank + 1 of every sorted position)
//   ms_ids       id[order[i]] = rank, seg[rank] = first sorted position;  ms_mean  one thread per cluster walks its segment in fp64
//   ms_faces     faces -> cluster ids, range check, degenerate faces die, rotation (three stable column sorts: equal triples adjacent)
//   ms_dups      a face equal to its predecessor in that order dies;  ms_used  clusters of surviving faces   (two inclusive scans)
//   ms_emit_*    compaction and renumbering of faces, cluster positions and the vertex map
// Smooth: one kernel, one thread per vertex over a CSR row, launched 2 * iterations times between two buffers.
// The arithmetic is the header's specification operation for operation (tests/support/simplify_ref.py restates it, compared bit for bit):
// nothing here may be reassociated, contracted or replaced by a reciprocal.
#include "common.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int64_t MS_ALIGN = 256;
constexpr float MS_CELLS = 2097152.0f;                  // 2^21 cells per axis
constexpr int64_t MS_BAD_KEY = INT64_MAX;               // an invalid vertex: sorts last, the call fails on the flag

inline unsigned ms_blocks(int64_t n) { return (unsigned)((n + MS_THREADS - 1) / MS_THREADS); }
inline int64_t ms_align(int64_t b) { return (b + MS_ALIGN - 1) / MS_ALIGN * MS_ALIGN; }
inline bool ms_finite(float v) { return v - v == 0.0f; }

__device__ __forceinline__ int64_t ms_tid() { return (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; }

// ---- simplify -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) ms_keys_kernel(const float* __restrict__ verts, int32_t V, float cell, float o0, float o1, float o2,
                                                             int64_t* __restrict__ keys, int32_t* __restrict__ flags) {
    const int64_t v = ms_tid();
    if (v >= V) return;
    const float org[3] = {o0, o1, o2};
    int64_t c[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = floorf(__fdiv_rn(__fsub_rn(verts[v * 3 + k], org[k]), cell));
        ok = ok && f >= 0.0f && f < MS_CELLS;           // NaN and the infinities compare false
        c[k] = ok ? (int64_t)f : 0;
    }
    keys[v] = ok ? ((c[2] << 42) | (c[1] << 21) | c[0]) : MS_BAD_KEY;
    if (!ok) flags[0] = 1;
}

__global__ void __launch_bounds__(MS_THREADS) ms_heads_kernel(const int64_t* __restrict__ skeys, int32_t V, int32_t* __restrict__ heads) {
    const int64_t i = ms_tid();
    if (i >= V) return;
    heads[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}

// id of every vertex and the first sorted position of every cluster; seg[K] = V
__global__ void __launch_bounds__(MS_THREADS) ms_ids_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ heads,
                                                            const int32_t* __restrict__ scan, int32_t V, int32_t* __restrict__ id, int32_t* __restrict__ seg) {
    const int64_t i = ms_tid();
    if (i >= V) return;
    const int32_t rank = scan[i] - 1;
    const int64_t v = order[i];
    if ((uint64_t)v < (uint64_t)V) id[v] = rank;
    if ((uint32_t)rank >= (uint32_t)V) return;          // never with an inclusive scan of heads
    if (heads[i]) seg[rank] = (int32_t)i;
    if (i == V - 1) seg[rank + 1] = V;
}

// One thread per cluster: the members in ascending original index (the sort was stable), summed sequentially in fp64, one division, one
// rounding to fp32.  A wave-level tree would change the order of the sum.
__global__ void __launch_bounds__(MS_THREADS) ms_mean_kernel(const float* __restrict__ verts, const int64_t* __restrict__ order,
                                                             const int32_t* __restrict__ scan, const int32_t* __restrict__ seg, int32_t V,
                                                             float* __restrict__ cpos) {
    const int64_t c = ms_tid();
    if (c >= V || c >= scan[V - 1]) return;
    const int32_t lo = seg[c], hi = seg[c + 1];
    if (lo < 0 || hi > V || lo >= hi) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int32_t i = lo; i < hi; ++i) {
        const int64_t v = order[i];
        if ((uint64_t)v >= (uint64_t)V) continue;
        s0 = __dadd_rn(s0, (double)verts[v * 3 + 0]);
        s1 = __dadd_rn(s1, (double)verts[v * 3 + 1]);
        s2 = __dadd_rn(s2, (double)verts[v * 3 + 2]);
    }
    const double n = (double)(hi - lo);
    cpos[c * 3 + 0] = (float)__ddiv_rn(s0, n);
    cpos[c * 3 + 1] = (float)__ddiv_rn(s1, n);
    cpos[c * 3 + 2] = (float)__ddiv_rn(s2, n);
}

// tri is planar [3][F] (the column sorts read contiguous columns).  An index outside [0, V) is flagged and never dereferenced.
__global__ void __launch_bounds__(MS_THREADS) ms_faces_kernel(const int32_t* __restrict__ faces, int32_t F, int32_t V, const int32_t* __restrict__ id,
                                                              int32_t* __restrict__ tri, int32_t* __restrict__ alive, int32_t* __restrict__ flags) {
    const int64_t f = ms_tid();
    if (f >= F) return;
    const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    int32_t g0 = -1, g1 = -1, g2 = -1, live = 0;
    if ((uint32_t)a < (uint32_t)V && (uint32_t)b < (uint32_t)V && (uint32_t)c < (uint32_t)V) {
        const int32_t x = id[a], y = id[b], z = id[c];
        live = (x != y && y != z && x != z) ? 1 : 0;
        if (y < x && y <= z) g0 = y, g1 = z, g2 = x;    // the smallest id first, winding kept (ids of a live face are distinct)
        else if (z < x && z < y) g0 = z, g1 = x, g2 = y;
        else g0 = x, g1 = y, g2 = z;
    } else {
        flags[1] = 1;
    }
    tri[f] = g0;
    tri[(int64_t)F + f] = g1;
    tri[2 * (int64_t)F + f] = g2;
    alive[f] = live;
}

// forder sorts the faces by (tri, original index).  A live face has three distinct ids, so it never equals a degenerate one: within a run of
// equal live triples the first has the lowest index and survives, every other one dies.
__global__ void __launch_bounds__(MS_THREADS) ms_dups_kernel(const int64_t* __restrict__ forder, const int32_t* __restrict__ tri, int32_t F,
                                                             int32_t* __restrict__ alive) {
    const int64_t j = ms_tid();
    if (j < 1 || j >= F) return;
    const int64_t a = forder[j], b = forder[j - 1];
    if ((uint64_t)a >= (uint64_t)F || (uint64_t)b >= (uint64_t)F) return;
    if (tri[a] == tri[b] && tri[(int64_t)F + a] == tri[(int64_t)F + b] && tri[2 * (int64_t)F + a] == tri[2 * (int64_t)F + b]) alive[a] = 0;
}

__global__ void __launch_bounds__(MS_THREADS) ms_used_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ alive, int32_t F, int32_t V,
                                                             int32_t* __restrict__ used) {
    const int64_t f = ms_tid();
    if (f >= F || !alive[f]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t g = tri[k * (int64_t)F + f];
        if ((uint32_t)g < (uint32_t)V) used[g] = 1;
    }
}

__global__ void __launch_bounds__(MS_THREADS) ms_emit_faces_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ alive,
                                                                   const int32_t* __restrict__ ascan, const int32_t* __restrict__ uscan, int32_t F, int32_t V,
                                                                   int32_t* __restrict__ out, int64_t cap) {
    const int64_t f = ms_tid();
    if (f >= F || !alive[f]) return;
    const int64_t row = (int64_t)ascan[f] - 1;
    if (row < 0 || row >= cap) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t g = tri[k * (int64_t)F + f];
        out[row * 3 + k] = (uint32_t)g < (uint32_t)V ? uscan[g] - 1 : -1;
    }
}

__global__ void __launch_bounds__(MS_THREADS) ms_emit_verts_kernel(const float* __restrict__ cpos, const int32_t* __restrict__ id,
                                                                   const int32_t* __restrict__ used, const int32_t* __restrict__ uscan, int32_t V,
                                                                   float* __restrict__ out, int64_t cap, int32_t* __restrict__ vmap) {
    const int64_t t = ms_tid();
    if (t >= V) return;
    if (used[t]) {                                      // t as a cluster: used is zero from K on
        const int64_t row = (int64_t)uscan[t] - 1;
        if (row >= 0 && row < cap) {
            out[row * 3 + 0] = cpos[t * 3 + 0];
            out[row * 3 + 1] = cpos[t * 3 + 1];
            out[row * 3 + 2] = cpos[t * 3 + 2];
        }
    }
    const int32_t g = id[t];                            // t as a vertex
    vmap[t] = ((uint32_t)g < (uint32_t)V && used[g]) ? uscan[g] - 1 : -1;
}

// ---- smooth -------------------------------------------------------------------------------------------------------------------------
// q_i = p_i + f * (mean of the neighbours - p_i), the neighbours of a CSR row added in the row's order (ascending j).
__global__ void __launch_bounds__(MS_THREADS) ms_smooth_kernel(const float* __restrict__ p, float* __restrict__ q, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ cols, const uint8_t* __restrict__ pinned, int32_t V, int32_t nnz,
                                                               float f) {
    const int64_t i = ms_tid();
    if (i >= V) return;
    const float p0 = p[i * 3 + 0], p1 = p[i * 3 + 1], p2 = p[i * 3 + 2];
    float q0 = p0, q1 = p1, q2 = p2;
    const int32_t lo = max(rowptr[i], 0), hi = min(rowptr[i + 1], nnz);
    if (hi > lo && !(pinned != nullptr && pinned[i])) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int32_t e = lo; e < hi; ++e) {
            const int32_t j = cols[e];
            if ((uint32_t)j >= (uint32_t)V) continue;   // never in a row built from checked faces
            s0 = __fadd_rn(s0, p[(int64_t)j * 3 + 0]);
            s1 = __fadd_rn(s1, p[(int64_t)j * 3 + 1]);
            s2 = __fadd_rn(s2, p[(int64_t)j * 3 + 2]);
        }
        const float n = (float)(hi - lo);
        q0 = __fadd_rn(p0, __fmul_rn(f, __fsub_rn(__fdiv_rn(s0, n), p0)));
        q1 = __fadd_rn(p1, __fmul_rn(f, __fsub_rn(__fdiv_rn(s1, n), p1)));
        q2 = __fadd_rn(p2, __fmul_rn(f, __fsub_rn(__fdiv_rn(s2, n), p2)));
    }
    q[i * 3 + 0] = q0;
    q[i * 3 + 1] = q1;
    q[i * 3 + 2] = q2;
}

__global__ void __launch_bounds__(MS_THREADS) ms_copy_kernel(const float* __restrict__ p, float* __restrict__ q, int64_t n) {
    const int64_t i = ms_tid();
    if (i < n) q[i] = p[i];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int ms_sizes(const eg3d_simplify_params* p) {
    if (p == nullptr || p->V < 0 || p->F < 0) return EG3D_ERR_INVALID;
    if (p->V > INT32_MAX || p->F > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    return EG3D_OK;
}

struct MsWorkspace {
    int32_t* id;                                        // [V] cluster of every vertex
    int32_t* seg;                                       // [V + 1] first sorted position of every cluster, then V
    float* cpos;                                        // [V][3] cluster positions (K rows used)
    int64_t bytes;
};

MsWorkspace ms_workspace(void* base, int64_t V) {
    MsWorkspace w;
    char* b = reinterpret_cast<char*>(base);
    const int64_t o1 = ms_align(V * 4), o2 = o1 + ms_align((V + 1) * 4);
    w.id = reinterpret_cast<int32_t*>(b);
    w.seg = reinterpret_cast<int32_t*>(b + o1);
    w.cpos = reinterpret_cast<float*>(b + o2);
    w.bytes = o2 + ms_align(V * 12);
    return w;
}

bool ms_has_workspace(const eg3d_simplify_params* p) { return p->workspace != nullptr && p->workspace_bytes >= ms_workspace(nullptr, p->V).bytes; }

int sm_sizes(const eg3d_smooth_params* p) {
    if (p == nullptr || p->V < 0 || p->nnz < 0 || p->iterations < 0) return EG3D_ERR_INVALID;
    if (p->V > INT32_MAX || p->nnz > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_simplify_query_workspace(const eg3d_simplify_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    *workspace_bytes = ms_workspace(nullptr, p->V).bytes;
    return EG3D_OK;
}

extern "C" int eg3d_simplify_keys(const eg3d_simplify_params* p, void* stream) {
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    if (!(p->cell > 0.0f) || !ms_finite(p->cell) || !ms_finite(p->origin[0]) || !ms_finite(p->origin[1]) || !ms_finite(p->origin[2])) return EG3D_ERR_INVALID;
    if (p->flags == nullptr || (p->V > 0 && (p->verts == nullptr || p->keys == nullptr))) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    eg3d_zero_words(p->flags, 2, st);
    EG3D_LAUNCH_CHECK();
    if (p->V == 0) return EG3D_OK;
    hipLaunchKernelGGL(ms_keys_kernel, dim3(ms_blocks(p->V)), dim3(MS_THREADS), 0, st, p->verts, (int32_t)p->V, p->cell, p->origin[0], p->origin[1],
                       p->origin[2], p->keys, p->flags);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_simplify_heads(const eg3d_simplify_params* p, void* stream) {
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    if (p->V == 0) return EG3D_OK;
    if (p->sorted_keys == nullptr || p->heads == nullptr) return EG3D_ERR_INVALID;
    hipLaunchKernelGGL(ms_heads_kernel, dim3(ms_blocks(p->V)), dim3(MS_THREADS), 0, (hipStream_t)stream, p->sorted_keys, (int32_t)p->V, p->heads);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_simplify_clusters(const eg3d_simplify_params* p, void* stream) {
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    if (p->flags == nullptr) return EG3D_ERR_INVALID;
    if (p->V > 0 && (p->verts == nullptr || p->order == nullptr || p->heads == nullptr || p->head_scan == nullptr || p->used == nullptr || !ms_has_workspace(p)))
        return EG3D_ERR_INVALID;
    if (p->F > 0 && (p->faces == nullptr || p->tri == nullptr || p->alive == nullptr)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const MsWorkspace w = ms_workspace(p->workspace, p->V);
    const int32_t V = (int32_t)p->V, F = (int32_t)p->F;
    if (V > 0) {
        hipLaunchKernelGGL(ms_ids_kernel, dim3(ms_blocks(V)), dim3(MS_THREADS), 0, st, p->order, p->heads, p->head_scan, V, w.id, w.seg);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_mean_kernel, dim3(ms_blocks(V)), dim3(MS_THREADS), 0, st, p->verts, p->order, p->head_scan, w.seg, V, w.cpos);
        EG3D_LAUNCH_CHECK();
        eg3d_zero_words(p->used, V, st);
        EG3D_LAUNCH_CHECK();
    }
    if (F > 0) {                                        // with V = 0 every index is out of range: id is not read
        hipLaunchKernelGGL(ms_faces_kernel, dim3(ms_blocks(F)), dim3(MS_THREADS), 0, st, p->faces, F, V, w.id, p->tri, p->alive, p->flags);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_simplify_mark(const eg3d_simplify_params* p, void* stream) {
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    if (p->F == 0) return EG3D_OK;
    if (p->tri == nullptr || p->alive == nullptr || p->face_order == nullptr || (p->V > 0 && p->used == nullptr)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int32_t V = (int32_t)p->V, F = (int32_t)p->F;
    hipLaunchKernelGGL(ms_dups_kernel, dim3(ms_blocks(F)), dim3(MS_THREADS), 0, st, p->face_order, p->tri, F, p->alive);
    EG3D_LAUNCH_CHECK();
    if (V > 0) {
        hipLaunchKernelGGL(ms_used_kernel, dim3(ms_blocks(F)), dim3(MS_THREADS), 0, st, p->tri, p->alive, F, V, p->used);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_simplify_emit(const eg3d_simplify_params* p, void* stream) {
    const int s = ms_sizes(p);
    if (s != EG3D_OK) return s;
    if (p->out_vert_capacity < 0 || p->out_face_capacity < 0) return EG3D_ERR_INVALID;
    if (p->out_vert_capacity > INT32_MAX || p->out_face_capacity > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    if (p->V > 0 && (p->used == nullptr || p->used_scan == nullptr || p->vertex_map == nullptr || !ms_has_workspace(p))) return EG3D_ERR_INVALID;
    if (p->V > 0 && p->out_vert_capacity > 0 && p->out_verts == nullptr) return EG3D_ERR_INVALID;
    if (p->F > 0 && (p->tri == nullptr || p->alive == nullptr || p->alive_scan == nullptr)) return EG3D_ERR_INVALID;
    if (p->F > 0 && p->out_face_capacity > 0 && (p->out_faces == nullptr || p->used_scan == nullptr)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const MsWorkspace w = ms_workspace(p->workspace, p->V);
    const int32_t V = (int32_t)p->V, F = (int32_t)p->F;
    if (F > 0 && p->out_face_capacity > 0) {
        hipLaunchKernelGGL(ms_emit_faces_kernel, dim3(ms_blocks(F)), dim3(MS_THREADS), 0, st, p->tri, p->alive, p->alive_scan, p->used_scan, F, V, p->out_faces,
                           p->out_face_capacity);
        EG3D_LAUNCH_CHECK();
    }
    if (V > 0) {
        hipLaunchKernelGGL(ms_emit_verts_kernel, dim3(ms_blocks(V)), dim3(MS_THREADS), 0, st, w.cpos, w.id, p->used, p->used_scan, V, p->out_verts,
                           p->out_vert_capacity, p->vertex_map);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_smooth_query_workspace(const eg3d_smooth_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    const int s = sm_sizes(p);
    if (s != EG3D_OK) return s;
    *workspace_bytes = p->iterations > 0 ? ms_align(p->V * 12) : 0;
    return EG3D_OK;
}

extern "C" int eg3d_smooth(const eg3d_smooth_params* p, void* stream) {
    const int s = sm_sizes(p);
    if (s != EG3D_OK) return s;
    if (!ms_finite(p->lam) || !ms_finite(p->mu)) return EG3D_ERR_INVALID;
    if (p->V == 0) return EG3D_OK;
    if (p->verts == nullptr || p->out == nullptr || p->out == p->verts) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int32_t V = (int32_t)p->V;
    if (p->iterations == 0) {
        hipLaunchKernelGGL(ms_copy_kernel, dim3(ms_blocks(p->V * 3)), dim3(MS_THREADS), 0, st, p->verts, p->out, p->V * 3);
        EG3D_LAUNCH_CHECK();
        return EG3D_OK;
    }
    if (p->rowptr == nullptr || (p->nnz > 0 && p->cols == nullptr)) return EG3D_ERR_INVALID;
    if (p->workspace == nullptr || p->workspace_bytes < ms_align(p->V * 12)) return EG3D_ERR_INVALID;
    float* tmp = reinterpret_cast<float*>(p->workspace);
    const float* src = p->verts;                        // verts -> tmp -> out -> tmp -> out ...: the input is never written, the last pass writes out
    for (int it = 0; it < p->iterations; ++it) {
        hipLaunchKernelGGL(ms_smooth_kernel, dim3(ms_blocks(V)), dim3(MS_THREADS), 0, st, src, tmp, p->rowptr, p->cols, p->pinned, V, (int32_t)p->nnz, p->lam);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_smooth_kernel, dim3(ms_blocks(V)), dim3(MS_THREADS), 0, st, tmp, p->out, p->rowptr, p->cols, p->pinned, V, (int32_t)p->nnz, p->mu);
        EG3D_LAUNCH_CHECK();
        src = p->out;
    }
    return EG3D_OK;
}
