// Marching cubes on a fp32 density grid (shape export: create_geometry / convert_mrc of the reference, include/eg3d_hip.h "Marching cubes").
//
// Four launches, all streaming the grid in 4096-point tiles (256 threads x 16 points, i2 fastest: every load is coalesced):
//   mc_count  per tile: active points (a crossing edge owned, or a cube with triangles), vertices, triangles     -> counts[tile]
//   mc_scan   one workgroup: exclusive scan of the tile triples                                                  -> offsets[tile], totals
//   (the host reads the totals and allocates)
//   mc_emit   per tile, recomputes every point; a workgroup exclusive scan (wave shuffles + LDS) places its vertices and one record
//             (point index, vertex base, face base, edge mask | case << 8) per active point.  The record list is sorted by construction.
//   mc_faces  per active record: its cube's triangles; each triangle corner's vertex is found by a binary search for the owning point in
//             the record list, then base + popcount(mask & lower axes).
// Integer counts only and no atomics: the output is a function of the input (bit-identical between runs and between the two builds).
#include "common.h"

#define MC_TABLE static __constant__ const
#include "mc_tables.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_ITERS = 16;
constexpr int MC_TILE = MC_THREADS * MC_ITERS;
constexpr int MC_SCAN_THREADS = 1024;
constexpr int MC_FIELD = 21;                          // bits per count when (active, vertices, triangles) travel as one 64-bit word
constexpr unsigned long long MC_FMASK = (1ull << MC_FIELD) - 1;

struct McDims {
    int32_t N, D0, D1, D2, S;                         // S = D1 * D2
};

struct McPoint {
    uint32_t mask;                                    // bit a: this point owns a vertex on its edge along output axis a (x = i2, y = i1, z = i0)
    uint32_t cube;                                    // case index of the cube whose min corner this is (0 if none)
    float v0, vn[3];                                  // value here and at the +x, +y, +z neighbours
    int32_t i0, i1, i2;
};

__device__ __forceinline__ McPoint mc_eval(const float* __restrict__ vol, int32_t p, const McDims& d, float level) {
    McPoint r;
    const uint32_t q = (uint32_t)p / (uint32_t)d.D2;
    r.i2 = p - (int32_t)q * d.D2;
    r.i0 = (int32_t)(q / (uint32_t)d.D1);
    r.i1 = (int32_t)q - r.i0 * d.D1;
    const bool hx = r.i2 < d.D2 - 1, hy = r.i1 < d.D1 - 1, hz = r.i0 < d.D0 - 1;
    r.v0 = vol[p];
    r.vn[0] = hx ? vol[p + 1] : r.v0;
    r.vn[1] = hy ? vol[p + d.D2] : r.v0;
    r.vn[2] = hz ? vol[p + d.S] : r.v0;
    const bool in0 = r.v0 > level, inx = r.vn[0] > level, iny = r.vn[1] > level, inz = r.vn[2] > level;
    r.mask = (uint32_t)(hx && inx != in0) | ((uint32_t)(hy && iny != in0) << 1) | ((uint32_t)(hz && inz != in0) << 2);
    r.cube = 0;
    if (hx && hy && hz) {
        const bool ixy = vol[p + 1 + d.D2] > level, ixz = vol[p + 1 + d.S] > level, iyz = vol[p + d.D2 + d.S] > level,
                   ixyz = vol[p + 1 + d.D2 + d.S] > level;
        r.cube = (uint32_t)in0 | ((uint32_t)inx << 1) | ((uint32_t)iny << 2) | ((uint32_t)ixy << 3) | ((uint32_t)inz << 4) | ((uint32_t)ixz << 5) |
                 ((uint32_t)iyz << 6) | ((uint32_t)ixyz << 7);
    }
    return r;
}

// (active, vertices, triangles) of one point packed into 21-bit fields: a tile holds at most 4096 / 12288 / 20480 of them
__device__ __forceinline__ unsigned long long mc_pack(const McPoint& r) {
    const unsigned long long ntri = mc_tri_count[r.cube];
    const unsigned long long act = (r.mask != 0u || ntri != 0ull) ? 1ull : 0ull;
    return act | ((unsigned long long)__popc(r.mask) << MC_FIELD) | (ntri << (2 * MC_FIELD));
}

__global__ void __launch_bounds__(MC_THREADS) mc_count_kernel(const float* __restrict__ vol, McDims d, float level, int4* __restrict__ counts) {
    __shared__ unsigned long long wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
    unsigned long long acc = 0;
    for (int k = 0; k < MC_ITERS; ++k) {
        const int64_t p = base + k * MC_THREADS + threadIdx.x;
        if (p < d.N) acc += mc_pack(mc_eval(vol, (int32_t)p, d, level));
    }
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < MC_THREADS / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = make_int4((int)(t & MC_FMASK), (int)((t >> MC_FIELD) & MC_FMASK), (int)(t >> (2 * MC_FIELD)), 0);
    }
}

// one workgroup: offsets[i] = sum of counts[0..i) per field (int64), totals = the sums over all tiles
__global__ void __launch_bounds__(MC_SCAN_THREADS) mc_scan_kernel(const int4* __restrict__ counts, int nb, longlong4* __restrict__ offsets,
                                                                 int64_t* __restrict__ totals) {
    __shared__ long long sh[2][3][MC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (nb + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    long long s[3] = {0, 0, 0};
    for (int i = lo; i < hi; ++i) {
        const int4 c = counts[i];
        s[0] += c.x;
        s[1] += c.y;
        s[2] += c.z;
    }
    int cur = 0;
    for (int f = 0; f < 3; ++f) sh[cur][f][t] = s[f];
    __syncthreads();
    for (int o = 1; o < MC_SCAN_THREADS; o <<= 1) {          // inclusive Hillis-Steele scan of the per-thread sums
        for (int f = 0; f < 3; ++f) sh[cur ^ 1][f][t] = sh[cur][f][t] + (t >= o ? sh[cur][f][t - o] : 0ll);
        __syncthreads();
        cur ^= 1;
    }
    long long run[3];
    for (int f = 0; f < 3; ++f) run[f] = sh[cur][f][t] - s[f];
    for (int i = lo; i < hi; ++i) {
        const int4 c = counts[i];
        offsets[i] = make_longlong4(run[0], run[1], run[2], 0);
        run[0] += c.x;
        run[1] += c.y;
        run[2] += c.z;
    }
    if (t == MC_SCAN_THREADS - 1) {
        totals[0] = sh[cur][0][t];
        totals[1] = sh[cur][1][t];
        totals[2] = sh[cur][2][t];
        totals[3] = 0;
    }
}

__global__ void __launch_bounds__(MC_THREADS) mc_emit_kernel(const float* __restrict__ vol, McDims d, float level, float3 origin, float3 spacing,
                                                             const longlong4* __restrict__ offsets, float* __restrict__ verts, int64_t vcap,
                                                             int4* __restrict__ recs, int64_t rcap) {
    __shared__ unsigned long long wsum[2][MC_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const longlong4 off = offsets[blockIdx.x];
    long long run_a = off.x, run_v = off.y, run_f = off.z;
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
    const float org[3] = {origin.x, origin.y, origin.z}, spc[3] = {spacing.x, spacing.y, spacing.z};
    for (int k = 0; k < MC_ITERS; ++k) {
        const int64_t p = base + k * MC_THREADS + threadIdx.x;
        McPoint r{};
        unsigned long long own = 0;
        if (p < d.N) {
            r = mc_eval(vol, (int32_t)p, d, level);
            own = mc_pack(r);
        }
        unsigned long long incl = own;                        // wave-inclusive scan of the packed counts
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[k & 1][wave] = incl;
        __syncthreads();                                      // wsum[k & 1] complete; wsum[(k + 1) & 1] no longer read by iteration k - 1
        unsigned long long excl = incl - own, total = 0;
        for (int w = 0; w < MC_THREADS / 64; ++w) {
            const unsigned long long s = wsum[k & 1][w];
            if (w < wave) excl += s;
            total += s;
        }
        if (own & MC_FMASK) {
            const long long ra = run_a + (long long)(excl & MC_FMASK);
            const long long rv = run_v + (long long)((excl >> MC_FIELD) & MC_FMASK);
            const long long rf = run_f + (long long)(excl >> (2 * MC_FIELD));
            if (ra < rcap) recs[ra] = make_int4((int)p, (int)rv, (int)rf, (int)(r.mask | (r.cube << 8)));
            const float pos[3] = {(float)r.i2, (float)r.i1, (float)r.i0};
            long long slot = rv;
            for (int a = 0; a < 3; ++a) {
                if (!((r.mask >> a) & 1u)) continue;
                const float t = (level - r.v0) / (r.vn[a] - r.v0);
                if (slot < vcap) {
                    float* o = verts + slot * 3;
                    for (int c = 0; c < 3; ++c) {
                        const float x = c == a ? pos[c] + t : pos[c];
                        o[c] = x * spc[c] + org[c];
                    }
                }
                ++slot;
            }
        }
        run_a += (long long)(total & MC_FMASK);
        run_v += (long long)((total >> MC_FIELD) & MC_FMASK);
        run_f += (long long)(total >> (2 * MC_FIELD));
    }
}

__global__ void __launch_bounds__(MC_THREADS) mc_faces_kernel(const int4* __restrict__ recs, const int64_t* __restrict__ totals, int64_t rcap,
                                                              int32_t D2, int32_t S, int32_t* __restrict__ faces, int64_t fcap) {
    const int64_t A = min((int64_t)totals[0], rcap);
    const int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (r >= A) return;
    const int4 rec = recs[r];
    const uint32_t cs = (uint32_t)rec.w >> 8;
    const int nt = mc_tri_count[cs];
    for (int t = 0; t < nt; ++t) {
        const int64_t f = (int64_t)rec.z + t;
        for (int j = 0; j < 3; ++j) {
            const int e = mc_tri_edges[cs][3 * t + j];
            const int lo = mc_edge_lo[e], ax = mc_edge_axis[e];
            const int32_t owner = rec.x + (lo & 1) + ((lo >> 1) & 1) * D2 + ((lo >> 2) & 1) * S;
            // records have distinct increasing point indices: the owner's record lies in [r, r + (owner - rec.x)]
            int64_t a = r, b = min(A, r + (int64_t)(owner - rec.x) + 1);
            while (a < b) {                                   // first record with point index >= owner
                const int64_t m = (a + b) >> 1;
                if (recs[m].x < owner) a = m + 1;
                else b = m;
            }
            int32_t vid = -1;                                 // only with capacities below the totals (a truncated record list)
            if (a < A && recs[a].x == owner) {
                const int4 q = recs[a];
                vid = q.y + __popc((uint32_t)q.w & 0xffu & ((1u << ax) - 1u));
            }
            if (f < fcap) faces[f * 3 + j] = vid;
        }
    }
}

constexpr int64_t MC_ALIGN = 256;
int64_t mc_align(int64_t b) { return (b + MC_ALIGN - 1) / MC_ALIGN * MC_ALIGN; }

// validates the dimensions; fills d and the number of tiles
int mc_dims(const eg3d_mc_params* p, McDims& d, int64_t& nb) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (p->D0 < 2 || p->D1 < 2 || p->D2 < 2) return EG3D_ERR_INVALID;
    const int64_t n = (int64_t)p->D0 * p->D1 * p->D2;
    if (n > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    d.N = (int32_t)n;
    d.D0 = p->D0;
    d.D1 = p->D1;
    d.D2 = p->D2;
    d.S = p->D1 * p->D2;
    nb = (n + MC_TILE - 1) / MC_TILE;
    return EG3D_OK;
}

int64_t mc_count_bytes(int64_t nb) { return mc_align(nb * (int64_t)sizeof(int4)) + mc_align(nb * (int64_t)sizeof(longlong4)); }

}  // namespace

extern "C" int eg3d_mc_query_workspace(const eg3d_mc_params* p, int64_t* count_bytes, int64_t* emit_bytes_per_active) {
    if (count_bytes == nullptr || emit_bytes_per_active == nullptr) return EG3D_ERR_INVALID;
    McDims d;
    int64_t nb;
    const int s = mc_dims(p, d, nb);
    if (s != EG3D_OK) return s;
    *count_bytes = mc_count_bytes(nb);
    *emit_bytes_per_active = (int64_t)sizeof(int4);
    return EG3D_OK;
}

extern "C" int eg3d_mc_count(const eg3d_mc_params* p, void* stream) {
    McDims d;
    int64_t nb;
    const int s = mc_dims(p, d, nb);
    if (s != EG3D_OK) return s;
    if (p->vol == nullptr || p->workspace == nullptr || p->totals == nullptr || p->workspace_bytes < mc_count_bytes(nb)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int4* counts = reinterpret_cast<int4*>(p->workspace);
    longlong4* offsets = reinterpret_cast<longlong4*>(reinterpret_cast<char*>(p->workspace) + mc_align(nb * (int64_t)sizeof(int4)));
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)nb), dim3(MC_THREADS), 0, st, p->vol, d, p->level, counts);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, st, counts, (int)nb, offsets, p->totals);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_mc_emit(const eg3d_mc_params* p, void* stream) {
    McDims d;
    int64_t nb;
    const int s = mc_dims(p, d, nb);
    if (s != EG3D_OK) return s;
    if (p->vol == nullptr || p->workspace == nullptr || p->totals == nullptr || p->workspace_bytes < mc_count_bytes(nb)) return EG3D_ERR_INVALID;
    if (p->vert_capacity < 0 || p->face_capacity < 0 || p->emit_workspace_bytes < 0) return EG3D_ERR_INVALID;
    if ((p->vert_capacity > 0 && p->verts == nullptr) || (p->face_capacity > 0 && p->faces == nullptr) ||
        (p->emit_workspace_bytes > 0 && p->emit_workspace == nullptr))
        return EG3D_ERR_INVALID;
    const int64_t rcap = p->emit_workspace_bytes / (int64_t)sizeof(int4);
    if (p->vert_capacity > INT32_MAX || p->face_capacity > INT32_MAX || rcap > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    const longlong4* offsets = reinterpret_cast<const longlong4*>(reinterpret_cast<const char*>(p->workspace) + mc_align(nb * (int64_t)sizeof(int4)));
    int4* recs = reinterpret_cast<int4*>(p->emit_workspace);
    hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)nb), dim3(MC_THREADS), 0, st, p->vol, d, p->level,
                       make_float3(p->origin[0], p->origin[1], p->origin[2]), make_float3(p->spacing[0], p->spacing[1], p->spacing[2]), offsets,
                       p->verts, p->vert_capacity, recs, rcap);
    EG3D_LAUNCH_CHECK();
    if (rcap > 0) {
        hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)((rcap + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, recs, p->totals, rcap, d.D2,
                           d.S, p->faces, p->face_capacity);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}
