// Connected components of {vol > level} on a fp32 grid, and removal of components (include/eg3d_hip.h "Grid components").
//
// One int32 parent per voxel in the lent workspace: -1 outside, otherwise the linear index of a voxel of the same component that is not
// larger than the voxel's own (a root points to itself).  Six launches, passes (a)-(f) of the header:
//   cc_local   per 8 x 8 x 64 tile: union-find over the tile's own adjacencies in LDS                    -> parent = the tile-local root
//   cc_merge   per tile: voxels with a forward neighbour in another tile unite the two sets in global memory (lock-free)
//   cc_count   per 4096-voxel chunk: roots and inside voxels  -> counts[chunk];   cc_scan: one workgroup -> offsets[chunk], totals
//   (the host reads the totals and allocates)
//   cc_rank    per chunk: parent[root] = -2 - rank, roots[rank] = root (ranks ascend with the linear index: no sort)
//   cc_relabel per tile: labels = rank of the voxel's root + 1; sizes
//
// Rules (per-XCD L2s are not coherent with each other; a CU's L1 is never refreshed by another CU's stores):
//   * cc_merge is the only kernel in which workgroups touch the same words.  There every access to a parent word is an agent-scope atomic
//     (cc_ld = __hip_atomic_load relaxed, atomicMin, atomicCAS), never a plain load or store.  Correctness does not even need the loads to be
//     fresh: every value a parent word has ever held is an ancestor-or-self of that voxel in the final forest, roots are changed by
//     compare-and-swap alone (it executes at the memory side and fails on a stale view), and non-roots only by atomicMin with an ancestor.
//   * cc_merge writes parent words of tile-local roots only: a voxel that is not a local root keeps pointing at its local root, which
//     cc_relabel uses to sum the sizes per tile.
//   * every other kernel reads what an earlier launch wrote, or words only the reading thread writes.
//   * no workgroup waits for another: no flags, no spin loops, no grid barriers.  Every parent walk ends because a parent is strictly smaller
//     than its child; every retry of a union continues from strictly smaller indices (said again at each loop).
//   * integers only; the partition, each component's smallest index and the sums do not depend on the schedule: bit-identical results.
#include "common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_T0 = EG3D_CC_TILE0, CC_T1 = EG3D_CC_TILE1, CC_T2 = EG3D_CC_TILE2;
constexpr int CC_TILE = CC_T0 * CC_T1 * CC_T2;          // 4096 voxels: 256 threads x 4 rounds x 4 consecutive voxels along i2
constexpr int CC_ROUNDS = CC_TILE / (CC_THREADS * 4);
constexpr int CC_CHUNK = 4096;                          // consecutive voxels per workgroup of the linear passes
constexpr int CC_ITERS = CC_CHUNK / CC_THREADS;
constexpr int CC_SCAN_THREADS = 1024;
static_assert(CC_T0 == 8 && CC_T1 == 8 && CC_T2 == 64 && CC_ROUNDS == 4, "the thread -> voxel map below is written for 8 x 8 x 64 tiles");

struct CcDims {
    int32_t N, D0, D1, D2, S;                           // S = D1 * D2
    int32_t nt0, nt1, nt2;                              // tiles per axis
};

// forward neighbours (higher linear index): faces first, so connectivity 6 takes the first three
__constant__ const int8_t cc_off[13][3] = {{0, 0, 1}, {0, 1, 0},  {1, 0, 0},  {0, 1, -1}, {0, 1, 1},  {1, -1, -1}, {1, -1, 0},
                                           {1, -1, 1}, {1, 0, -1}, {1, 0, 1}, {1, 1, -1}, {1, 1, 0},  {1, 1, 1}};

struct CcTile {
    int32_t b0, b1, b2, o0, o1, o2;                     // tile coordinates and the grid index of its first voxel
};

__device__ __forceinline__ CcTile cc_tile(const CcDims& d) {
    CcTile t;
    const uint32_t bid = blockIdx.x;
    const uint32_t q = bid / (uint32_t)d.nt2;
    t.b2 = (int32_t)(bid - q * (uint32_t)d.nt2);
    t.b0 = (int32_t)(q / (uint32_t)d.nt1);
    t.b1 = (int32_t)q - t.b0 * d.nt1;
    t.o0 = t.b0 * CC_T0;
    t.o1 = t.b1 * CC_T1;
    t.o2 = t.b2 * CC_T2;
    return t;
}

// round r of thread t covers local voxels (l0, l1, l2 .. l2 + 3); their local index is r * 1024 + t * 4 + k
__device__ __forceinline__ void cc_local_coords(int r, int& l0, int& l1, int& l2) {
    l0 = r * 2 + ((int)threadIdx.x >> 7);
    l1 = ((int)threadIdx.x >> 4) & 7;
    l2 = ((int)threadIdx.x & 15) * 4;
}

// ---- union-find in LDS (one workgroup) ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_ld_lds(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int cc_find_lds(int* lab, int x) {
    int p = cc_ld_lds(&lab[x]);
    while (p != x) {                                    // ends: p < x, the index strictly decreases
        const int g = cc_ld_lds(&lab[p]);
        if (g != p) atomicMin(&lab[x], g);              // path halving: x is no root, g is an ancestor of x
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void cc_unite_lds(int* lab, int a, int b) {
    int ra = cc_find_lds(lab, a), rb = cc_find_lds(lab, b);
    while (ra != rb) {                                  // ends: max(ra, rb) strictly decreases on every retry
        if (ra < rb) {
            const int t = ra;
            ra = rb;
            rb = t;
        }
        const int old = atomicCAS(&lab[ra], ra, rb);    // hook the larger root under the smaller index
        if (old == ra) break;
        ra = cc_find_lds(lab, old);                     // ra was no root any more: old < ra
        rb = cc_find_lds(lab, rb);
    }
}

// ---- union-find in global memory (all workgroups of cc_merge) -----------------------------------------------------------------------
__device__ __forceinline__ int cc_ld(const int32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(int32_t* par, int x) {
    int p = cc_ld(&par[x]);
    while (p != x) {                                    // ends: p < x, the index strictly decreases
        const int g = cc_ld(&par[p]);
        if (g != p) atomicMin(&par[x], g);              // path halving with an ancestor; x is a non-root local root
        x = p;
        p = g;
    }
    return x;
}

// a and b are local roots (cc_merge passes parents of voxels): only local roots are ever written
__device__ __forceinline__ void cc_unite(int32_t* par, int a, int b) {
    int ra = cc_find(par, a), rb = cc_find(par, b);
    while (ra != rb) {                                  // ends: max(ra, rb) strictly decreases on every retry, and it is >= 0
        if (ra < rb) {
            const int t = ra;
            ra = rb;
            rb = t;
        }
        const int old = atomicCAS(&par[ra], ra, rb);    // succeeds only while ra is still a root
        if (old == ra) break;
        ra = cc_find(par, old);                         // old < ra
        rb = cc_find(par, rb);
    }
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(CC_THREADS) cc_local_kernel(const float* __restrict__ vol, CcDims d, float level, int noff, int32_t* __restrict__ par) {
    __shared__ int lab[CC_TILE];
    const CcTile t = cc_tile(d);
    uint32_t inside = 0;                                // bit r * 4 + k
    for (int r = 0; r < CC_ROUNDS; ++r) {
        int l0, l1, l2;
        cc_local_coords(r, l0, l1, l2);
        const int i0 = t.o0 + l0, i1 = t.o1 + l1, i2 = t.o2 + l2;
        const bool row = i0 < d.D0 && i1 < d.D1;
        const int32_t g = row ? (i0 * d.D1 + i1) * d.D2 + i2 : 0;
        float v[4];
        bool ok[4];
        if (VEC) {                                      // D2 % 4 == 0: the four voxels are in the grid together
            const bool in = row && i2 < d.D2;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in) q = *reinterpret_cast<const float4*>(vol + g);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            for (int k = 0; k < 4; ++k) ok[k] = in;
        } else {
            for (int k = 0; k < 4; ++k) {
                ok[k] = row && i2 + k < d.D2;
                v[k] = ok[k] ? vol[g + k] : 0.f;
            }
        }
        const int l = r * (CC_THREADS * 4) + (int)threadIdx.x * 4;
        for (int k = 0; k < 4; ++k) {
            const bool in = ok[k] && v[k] > level;      // NaN compares false: outside
            inside |= (uint32_t)in << (r * 4 + k);
            lab[l + k] = in ? l + k : -1;
        }
    }
    __syncthreads();
    for (int r = 0; r < CC_ROUNDS; ++r) {
        int l0, l1, l2;
        cc_local_coords(r, l0, l1, l2);
        for (int k = 0; k < 4; ++k) {
            if (!((inside >> (r * 4 + k)) & 1u)) continue;
            const int l = r * (CC_THREADS * 4) + (int)threadIdx.x * 4 + k;
            for (int o = 0; o < noff; ++o) {
                const int n0 = l0 + cc_off[o][0], n1 = l1 + cc_off[o][1], n2 = l2 + k + cc_off[o][2];
                if ((unsigned)n0 >= (unsigned)CC_T0 || (unsigned)n1 >= (unsigned)CC_T1 || (unsigned)n2 >= (unsigned)CC_T2) continue;
                const int nl = (n0 * CC_T1 + n1) * CC_T2 + n2;
                if (cc_ld_lds(&lab[nl]) >= 0) cc_unite_lds(lab, l, nl);      // an inside voxel's entry stays >= 0
            }
        }
    }
    __syncthreads();
    for (int r = 0; r < CC_ROUNDS; ++r) {
        int l0, l1, l2;
        cc_local_coords(r, l0, l1, l2);
        const int i0 = t.o0 + l0, i1 = t.o1 + l1, i2 = t.o2 + l2;
        if (i0 >= d.D0 || i1 >= d.D1) continue;
        const int32_t g = (i0 * d.D1 + i1) * d.D2 + i2;
        int32_t out[4];
        for (int k = 0; k < 4; ++k) {
            out[k] = -1;
            if ((inside >> (r * 4 + k)) & 1u) {
                const int rt = cc_find_lds(lab, r * (CC_THREADS * 4) + (int)threadIdx.x * 4 + k);
                out[k] = ((t.o0 + (rt >> 9)) * d.D1 + t.o1 + ((rt >> 6) & 7)) * d.D2 + t.o2 + (rt & 63);
            }
        }
        if (VEC) {
            if (i2 < d.D2) *reinterpret_cast<int4*>(par + g) = make_int4(out[0], out[1], out[2], out[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (i2 + k < d.D2) par[g + k] = out[k];
        }
    }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(CcDims d, int noff, int32_t* par) {
    const CcTile t = cc_tile(d);
    for (int r = 0; r < CC_ROUNDS; ++r) {
        int l0, l1, l2b;
        cc_local_coords(r, l0, l1, l2b);
        const int i0 = t.o0 + l0, i1 = t.o1 + l1;
        if (i0 >= d.D0 || i1 >= d.D1) continue;
        const int32_t v = (i0 * d.D1 + i1) * d.D2 + t.o2 + l2b;
        int pv[4] = {0, 0, 0, 0};                       // par[v + k], read once (any value it ever held is an ancestor-or-self of the voxel)
        uint32_t have = 0;
        for (int o = 0; o < noff; ++o) {
            const int e0 = cc_off[o][0], e1 = cc_off[o][1], e2 = cc_off[o][2];
            const int n0 = l0 + e0, n1 = l1 + e1, g0 = i0 + e0, g1 = i1 + e1;
            if ((unsigned)g0 >= (unsigned)d.D0 || (unsigned)g1 >= (unsigned)d.D1) continue;
            const bool other_row = (unsigned)n0 >= (unsigned)CC_T0 || (unsigned)n1 >= (unsigned)CC_T1;
            const int32_t nb = (g0 * d.D1 + g1) * d.D2 + t.o2 + l2b + e2;
            int last_v = -1, last_n = -1;               // consecutive voxels along i2 mostly join the same two local roots: unite them once
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l2 = l2b + k, g2 = t.o2 + l2 + e2;
                if (t.o2 + l2 >= d.D2 || (unsigned)g2 >= (unsigned)d.D2) continue;
                if (!other_row && (unsigned)(l2 + e2) < (unsigned)CC_T2) continue;      // a neighbour in this tile: cc_local's
                if (!((have >> k) & 1u)) {
                    pv[k] = cc_ld(&par[v + k]);
                    have |= 1u << k;
                }
                if (pv[k] < 0) continue;                // v is outside
                const int pn = cc_ld(&par[nb + k]);
                if (pn < 0 || (pv[k] == last_v && pn == last_n)) continue;
                last_v = pv[k];
                last_n = pn;
                cc_unite(par, pv[k], pn);               // from the parents on: v and its neighbour themselves are never written
            }
        }
    }
}

// ---- (c), (d) -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_count_kernel(const int32_t* __restrict__ par, int32_t N, int2* __restrict__ counts) {
    __shared__ unsigned long long wsum[CC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
    unsigned long long acc = 0;                         // roots | inside << 32
    for (int k = 0; k < CC_ITERS; ++k) {
        const int64_t p = base + k * CC_THREADS + threadIdx.x;
        if (p < N) {
            const int32_t x = par[p];
            acc += (x == (int32_t)p ? 1ull : 0ull) | (x >= 0 ? 1ull << 32 : 0ull);
        }
    }
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) s += wsum[w];
        counts[blockIdx.x] = make_int2((int)(s & 0xffffffffull), (int)(s >> 32));
    }
}

// one workgroup: offsets[i] = roots in chunks [0, i); totals = (roots, inside voxels) of the grid
__global__ void __launch_bounds__(CC_SCAN_THREADS) cc_scan_kernel(const int2* __restrict__ counts, int nb, int32_t* __restrict__ offsets,
                                                                 int64_t* __restrict__ totals) {
    __shared__ long long sh[2][2][CC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (nb + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    long long s[2] = {0, 0};
    for (int i = lo; i < hi; ++i) {
        const int2 c = counts[i];
        s[0] += c.x;
        s[1] += c.y;
    }
    int cur = 0;
    for (int f = 0; f < 2; ++f) sh[cur][f][t] = s[f];
    __syncthreads();
    for (int o = 1; o < CC_SCAN_THREADS; o <<= 1) {     // inclusive Hillis-Steele scan of the per-thread sums
        for (int f = 0; f < 2; ++f) sh[cur ^ 1][f][t] = sh[cur][f][t] + (t >= o ? sh[cur][f][t - o] : 0ll);
        __syncthreads();
        cur ^= 1;
    }
    long long run = sh[cur][0][t] - s[0];
    for (int i = lo; i < hi; ++i) {
        offsets[i] = (int32_t)run;
        run += counts[i].x;
    }
    if (t == CC_SCAN_THREADS - 1) {
        totals[0] = sh[cur][0][t];
        totals[1] = sh[cur][1][t];
    }
}

// ---- (e) ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_rank_kernel(int32_t* __restrict__ par, int32_t N, const int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ roots, int32_t count) {
    __shared__ int wsum[2][CC_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
    int run = offsets[blockIdx.x];
    for (int k = 0; k < CC_ITERS; ++k) {
        const int64_t p = base + k * CC_THREADS + threadIdx.x;
        const bool root = p < N && par[p] == (int32_t)p;                      // a word only this thread writes
        const unsigned long long b = __ballot(root);
        if (lane == 0) wsum[k & 1][wave] = __popcll(b);
        __syncthreads();                                // wsum[k & 1] complete; wsum[(k + 1) & 1] no longer read by iteration k - 1
        int before = 0, total = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) {
            const int s = wsum[k & 1][w];
            if (w < wave) before += s;
            total += s;
        }
        if (root) {
            const int rank = run + before + __popcll(b & ((1ull << lane) - 1ull));
            par[p] = -2 - rank;
            if (rank < count) roots[rank] = (int32_t)p;
        }
        run += total;
    }
}

// ---- (f) ----------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(CC_THREADS) cc_relabel_kernel(const int32_t* __restrict__ par, CcDims d, int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ sizes, int32_t count) {
    __shared__ int cnt[CC_TILE];
    const CcTile t = cc_tile(d);
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) cnt[i] = 0;
    __syncthreads();
    int32_t lbl[CC_ROUNDS * 4];
    int ckey = -1, crun = 0;                            // this thread's current run of equal keys
    for (int r = 0; r < CC_ROUNDS; ++r) {
        int l0, l1, l2;
        cc_local_coords(r, l0, l1, l2);
        const int i0 = t.o0 + l0, i1 = t.o1 + l1, i2 = t.o2 + l2;
        for (int k = 0; k < 4; ++k) lbl[r * 4 + k] = 0;
        if (i0 >= d.D0 || i1 >= d.D1) continue;
        const int32_t g = (i0 * d.D1 + i1) * d.D2 + i2;
        int32_t pv[4];
        if (VEC) {
            int4 q = make_int4(-1, -1, -1, -1);
            if (i2 < d.D2) q = *reinterpret_cast<const int4*>(par + g);
            pv[0] = q.x, pv[1] = q.y, pv[2] = q.z, pv[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k) pv[k] = i2 + k < d.D2 ? par[g + k] : -1;
        }
        for (int k = 0; k < 4; ++k) {
            if (pv[k] == -1) continue;                  // outside (or beyond the grid): label 0
            int x = pv[k];
            while (x >= 0) x = par[x];                  // ends: a parent is strictly smaller than its child; a root holds -2 - rank
            lbl[r * 4 + k] = -1 - x;                    // rank + 1
            // The slot the voxel is counted in: its parent's when that is another voxel of this tile (its local root, or for a local root
            // hooked to another local root of the tile, a voxel of the same component), else its own.  The voxel at a slot always has the
            // label of every voxel counted there.
            int key = r * (CC_THREADS * 4) + (int)threadIdx.x * 4 + k;
            if (pv[k] >= 0 && pv[k] != g + k) {
                const uint32_t q = (uint32_t)pv[k] / (uint32_t)d.D2;
                const int j2 = pv[k] - (int32_t)q * d.D2;
                const int j0 = (int)(q / (uint32_t)d.D1);
                const int j1 = (int)q - j0 * d.D1;
                if ((j0 >> 3) == t.b0 && (j1 >> 3) == t.b1 && (j2 >> 6) == t.b2) key = ((j0 & 7) * CC_T1 + (j1 & 7)) * CC_T2 + (j2 & 63);
            }
            if (key != ckey) {
                if (crun) atomicAdd(&cnt[ckey], crun);
                ckey = key;
                crun = 0;
            }
            ++crun;
        }
        if (VEC) {
            if (i2 < d.D2) *reinterpret_cast<int4*>(labels + g) = make_int4(lbl[r * 4], lbl[r * 4 + 1], lbl[r * 4 + 2], lbl[r * 4 + 3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (i2 + k < d.D2) labels[g + k] = lbl[r * 4 + k];
        }
    }
    if (crun) atomicAdd(&cnt[ckey], crun);
    __syncthreads();
    for (int r = 0; r < CC_ROUNDS; ++r)
        for (int k = 0; k < 4; ++k) {
            const int c = cnt[r * (CC_THREADS * 4) + (int)threadIdx.x * 4 + k];
            const int32_t lb = lbl[r * 4 + k];
            if (c > 0 && lb >= 1 && lb <= count) atomicAdd(&sizes[lb - 1], c);
        }
}

// ---- keep ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cc_keep_one(float v, int32_t l, const uint8_t* __restrict__ keep, int32_t count, float fill) {
    return (l < 1 || l > count || keep[l]) ? v : fill;
}

template <bool VEC>
__global__ void __launch_bounds__(CC_THREADS) cc_keep_kernel(const float* vol, const int32_t* __restrict__ labels, const uint8_t* __restrict__ keep,
                                                             int32_t count, float fill, float* out, int32_t N) {
    const int64_t i = ((int64_t)blockIdx.x * CC_THREADS + threadIdx.x) * 4;
    if (i >= N) return;
    if (VEC && i + 3 < N) {
        const float4 v = *reinterpret_cast<const float4*>(vol + i);
        const int4 l = *reinterpret_cast<const int4*>(labels + i);
        *reinterpret_cast<float4*>(out + i) = make_float4(cc_keep_one(v.x, l.x, keep, count, fill), cc_keep_one(v.y, l.y, keep, count, fill),
                                                          cc_keep_one(v.z, l.z, keep, count, fill), cc_keep_one(v.w, l.w, keep, count, fill));
    } else {
        for (int k = 0; k < 4 && i + k < N; ++k) out[i + k] = cc_keep_one(vol[i + k], labels[i + k], keep, count, fill);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
constexpr int64_t CC_ALIGN = 256;
int64_t cc_align(int64_t b) { return (b + CC_ALIGN - 1) / CC_ALIGN * CC_ALIGN; }

// validates the dimensions; fills d, the number of tiles and the number of chunks
int cc_dims(const eg3d_cc_params* p, CcDims& d, int64_t& ntiles, int64_t& nchunks) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (p->D0 < 1 || p->D1 < 1 || p->D2 < 1) return EG3D_ERR_INVALID;
    const int64_t rows = (int64_t)p->D0 * p->D1;            // checked before the third factor: no overflow of int64
    if (rows > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    const int64_t n = rows * p->D2;
    if (n > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    d.N = (int32_t)n;
    d.D0 = p->D0;
    d.D1 = p->D1;
    d.D2 = p->D2;
    d.S = p->D1 * p->D2;
    d.nt0 = (p->D0 + CC_T0 - 1) / CC_T0;
    d.nt1 = (p->D1 + CC_T1 - 1) / CC_T1;
    d.nt2 = (p->D2 + CC_T2 - 1) / CC_T2;
    ntiles = (int64_t)d.nt0 * d.nt1 * d.nt2;                // <= N
    nchunks = (n + CC_CHUNK - 1) / CC_CHUNK;
    return EG3D_OK;
}

struct CcWorkspace {
    int32_t* par;
    int2* counts;
    int32_t* offsets;
    int64_t bytes;
};

CcWorkspace cc_workspace(void* base, const CcDims& d, int64_t nchunks) {
    CcWorkspace w;
    char* b = reinterpret_cast<char*>(base);
    const int64_t o1 = cc_align((int64_t)d.N * 4), o2 = o1 + cc_align(nchunks * (int64_t)sizeof(int2));
    w.par = reinterpret_cast<int32_t*>(b);
    w.counts = reinterpret_cast<int2*>(b + o1);
    w.offsets = reinterpret_cast<int32_t*>(b + o2);
    w.bytes = o2 + cc_align(nchunks * 4);
    return w;
}

bool cc_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15u) == 0; }

int cc_noff(int connectivity) { return connectivity == 6 ? 3 : connectivity == 26 ? 13 : 0; }

}  // namespace

extern "C" int eg3d_cc_query_workspace(const eg3d_cc_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    CcDims d;
    int64_t ntiles, nchunks;
    const int s = cc_dims(p, d, ntiles, nchunks);
    if (s != EG3D_OK) return s;
    *workspace_bytes = cc_workspace(nullptr, d, nchunks).bytes;
    return EG3D_OK;
}

extern "C" int eg3d_cc_label(const eg3d_cc_params* p, void* stream) {
    CcDims d;
    int64_t ntiles, nchunks;
    const int s = cc_dims(p, d, ntiles, nchunks);
    if (s != EG3D_OK) return s;
    const int noff = cc_noff(p->connectivity);
    if (noff == 0 || p->vol == nullptr || p->workspace == nullptr || p->totals == nullptr) return EG3D_ERR_INVALID;
    const CcWorkspace w = cc_workspace(p->workspace, d, nchunks);
    if (p->workspace_bytes < w.bytes) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = d.D2 % 4 == 0 && cc_aligned16(p->vol) && cc_aligned16(w.par);
    if (vec) hipLaunchKernelGGL(cc_local_kernel<true>, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, p->vol, d, p->level, noff, w.par);
    else hipLaunchKernelGGL(cc_local_kernel<false>, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, p->vol, d, p->level, noff, w.par);
    EG3D_LAUNCH_CHECK();
    if (ntiles > 1) {
        hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, d, noff, w.par);
        EG3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nchunks), dim3(CC_THREADS), 0, st, w.par, d.N, w.counts);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, w.counts, (int)nchunks, w.offsets, p->totals);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_cc_finish(const eg3d_cc_params* p, void* stream) {
    CcDims d;
    int64_t ntiles, nchunks;
    const int s = cc_dims(p, d, ntiles, nchunks);
    if (s != EG3D_OK) return s;
    if (p->labels == nullptr || p->workspace == nullptr || p->count < 0) return EG3D_ERR_INVALID;
    if (p->count > 0 && (p->sizes == nullptr || p->roots == nullptr)) return EG3D_ERR_INVALID;
    const CcWorkspace w = cc_workspace(p->workspace, d, nchunks);
    if (p->workspace_bytes < w.bytes) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (p->count == 0) {                                // every voxel is outside
        eg3d_zero_words(p->labels, d.N, st);
        EG3D_LAUNCH_CHECK();
        return EG3D_OK;
    }
    eg3d_zero_words(p->sizes, p->count, st);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)nchunks), dim3(CC_THREADS), 0, st, w.par, d.N, w.offsets, p->roots, p->count);
    EG3D_LAUNCH_CHECK();
    const bool vec = d.D2 % 4 == 0 && cc_aligned16(p->labels) && cc_aligned16(w.par);
    if (vec) hipLaunchKernelGGL(cc_relabel_kernel<true>, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, w.par, d, p->labels, p->sizes, p->count);
    else hipLaunchKernelGGL(cc_relabel_kernel<false>, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, w.par, d, p->labels, p->sizes, p->count);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_cc_keep(const eg3d_cc_params* p, void* stream) {
    CcDims d;
    int64_t ntiles, nchunks;
    const int s = cc_dims(p, d, ntiles, nchunks);
    if (s != EG3D_OK) return s;
    if (p->vol == nullptr || p->labels == nullptr || p->out == nullptr || p->count < 0 || (p->count > 0 && p->keep == nullptr)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)(((int64_t)d.N + CC_THREADS * 4 - 1) / (CC_THREADS * 4));
    const bool vec = cc_aligned16(p->vol) && cc_aligned16(p->labels) && cc_aligned16(p->out);
    if (vec) hipLaunchKernelGGL(cc_keep_kernel<true>, dim3(nb), dim3(CC_THREADS), 0, st, p->vol, p->labels, p->keep, p->count, p->fill, p->out, d.N);
    else hipLaunchKernelGGL(cc_keep_kernel<false>, dim3(nb), dim3(CC_THREADS), 0, st, p->vol, p->labels, p->keep, p->count, p->fill, p->out, d.N);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
