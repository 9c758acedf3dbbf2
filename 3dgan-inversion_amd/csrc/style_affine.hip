// All style affines of a synthesis network in one launch.
//
// Every modulated layer owns a FullyConnectedLayer(w_dim -> in_channels, bias_init=1) that maps the layer's latent row to its
// styles (training/networks_stylegan2.py:98-108 conv layers, :129-137 toRGB with its extra weight_gain).  Per layer that is a
// [N,512]x[512,C] GEMM plus two scalings -- ~5 launches forward+backward for 26 layers, each far below a microsecond of work.
// Here the bank of layers is one memory-bound pass over the ~20 MB of affine weights (and one over the ~10 MB of wsq):
//   fwd:  styles_l[n, j] = ( sum_k ws[n, wrow_l, k] * (W_l[j,k] * wgain_l) + b_l[j] * bgain_l ) * post_l
//   bwd:  dws[n, wrow_l, k] += sum_j dstyles_l[n, j] * post_l * (W_l[j,k] * wgain_l)
//         dW_l[j,k] = sum_n dstyles_l[n,j] * post_l * wgain_l * ws[n,wrow_l,k],  db_l[j] = sum_n dstyles_l[n,j] * post_l * bgain_l
//         (trainable affines: the pivotal-tuning phase)
#include "common.h"
#include "det.h"

namespace {

// Each kernel is one stream over its matrix: a thread issues all the loads of its share before the first instruction that depends on one.
//   forward (styles, d): a wave owns GEMV_ROWS rows and holds the first 512 columns of each in registers (8 x 16 bytes in flight per lane at D = 512),
//       then walks the batch over them -- a row is read once for all N;
//   backward (dws, dout_extra): a block owns a tile of rows; thread = (column quad, row group) holds its TILE / 4 rows of the quad in registers, the
//       row groups meet in LDS and one atomic per (block, column) leaves the block.
constexpr int GEMV_ROWS = 4, GEMV_WAVES = 4, GEMV_TILE = GEMV_ROWS * GEMV_WAVES;       // forward: rows per wave, waves per block, rows per block
constexpr int COLS_THREADS = 512, COLS_KQ = 128, COLS_RG = COLS_THREADS / COLS_KQ;     // backward: column groups x row groups of a block
#ifndef EG3D_STYLE_AFFINE_BWD_TILE
#define EG3D_STYLE_AFFINE_BWD_TILE 64
#endif
#ifndef EG3D_STYLE_DEMOD_BWD_TILE
#define EG3D_STYLE_DEMOD_BWD_TILE 32
#endif
constexpr int AFFINE_BWD_TILE = EG3D_STYLE_AFFINE_BWD_TILE;       // 9 760 rows of the C2 bank: ~160 blocks, each address of a dws row sees one atomic per block
constexpr int DEMOD_BWD_TILE = EG3D_STYLE_DEMOD_BWD_TILE;         // wsq is half the bytes: half the tile keeps as many blocks in the air
constexpr int WGRAD_ROWS = 32;

// block -> (layer, tile of the layer), tiles(layer) = the number of blocks the layer takes.  Lane l reads layer l's counts and the lanes scan them: one
// round trip to the kernel arguments.  (Walking the layers in a loop is one DEPENDENT scalar load per layer, each a miss of its own -- ~10 us in
// front of the first matrix load of every block, which was the floor all four kernels of the C2 bank shared.)  Returns b.nlayers for a block past the end.
static_assert(EG3D_STYLE_BANK_MAX <= 64, "one lane per layer");
template <class Tiles>
__device__ __forceinline__ int find_tile(const eg3d_style_bank& b, int blk, Tiles tiles, int& tile) {
    const int lane = threadIdx.x & 63;
    const int nt = lane < b.nlayers ? tiles(b.layers[lane]) : 0;
    int inc = nt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    const unsigned long long m = __ballot(lane < b.nlayers && blk < inc);
    if (m == 0) { tile = 0; return b.nlayers; }
    const int l = __ffsll(m) - 1;
    tile = __builtin_amdgcn_readfirstlane(blk - __shfl(inc - nt, l));
    return l;
}

__device__ __forceinline__ int find_layer(const eg3d_style_bank& b, int blk, const int rows_per_block, int& row0) {
    const int l = find_tile(b, blk, [&](const eg3d_style_layer& q) { return (q.C + rows_per_block - 1) / rows_per_block; }, row0);
    row0 *= rows_per_block;
    return l;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// dot(n, r) = sum_k f(x[n, k]) * (M[row0 + r, k] * mscale), f = square or identity, for the wave's GEMV_ROWS rows and every n; lane r < GEMV_ROWS runs
// emit(n, row0 + r, dot, rowc[row0 + r]) (rowc: a per-row constant read with the first loads, or null).  K % 4 == 0, M and x 16-byte aligned.
// Rows past `rows` are read at the last row and not emitted; columns past K read column 0 against a zero of x.
template <bool SQUARE, class Emit>
__device__ __forceinline__ void wave_rows_dot(const float* __restrict__ M, int rows, int K, int row0, float mscale, const float* __restrict__ x, int64_t xstride,
                                              int N, const float* __restrict__ rowc, int lane, Emit emit) {
    const bool mine = lane < GEMV_ROWS && row0 + lane < rows;
    const float rc = (rowc != nullptr && mine) ? rowc[row0 + lane] : 0.f;
    const int k0 = lane * 4, k1 = 256 + lane * 4;
    const bool in0 = k0 < K, in1 = k1 < K;
    float4 w[GEMV_ROWS][2];
#pragma unroll
    for (int r = 0; r < GEMV_ROWS; ++r) {
        const float* p = M + (int64_t)min(row0 + r, rows - 1) * K;
        w[r][0] = ld4(p + (in0 ? k0 : 0));
        w[r][1] = ld4(p + (in1 ? k1 : 0));
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v0 = in0 ? ld4(x + k0) : zero, v1 = in1 ? ld4(x + k1) : zero;
#pragma unroll
    for (int r = 0; r < GEMV_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) { w[r][c].x *= mscale; w[r][c].y *= mscale; w[r][c].z *= mscale; w[r][c].w *= mscale; }
    for (int n = 0; n < N; ++n) {
        const float* xn = x + (int64_t)n * xstride;
        if (n > 0) { v0 = in0 ? ld4(xn + k0) : zero; v1 = in1 ? ld4(xn + k1) : zero; }
        if (SQUARE) { v0.x *= v0.x; v0.y *= v0.y; v0.z *= v0.z; v0.w *= v0.w; v1.x *= v1.x; v1.y *= v1.y; v1.z *= v1.z; v1.w *= v1.w; }
        float acc[GEMV_ROWS];
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r) {
            float a = v0.x * w[r][0].x;
            a += v0.y * w[r][0].y; a += v0.z * w[r][0].z; a += v0.w * w[r][0].w;
            a += v1.x * w[r][1].x; a += v1.y * w[r][1].y; a += v1.z * w[r][1].z; a += v1.w * w[r][1].w;
            acc[r] = a;
        }
        for (int k = 512 + lane * 4; k < K; k += 256) {          // rows longer than the registers hold (not the generator's: D = 512, C <= 512)
            float4 v = ld4(xn + k);
            if (SQUARE) { v.x *= v.x; v.y *= v.y; v.z *= v.z; v.w *= v.w; }
#pragma unroll
            for (int r = 0; r < GEMV_ROWS; ++r) {
                const float4 q = ld4(M + (int64_t)min(row0 + r, rows - 1) * K + k);
                acc[r] += v.x * (q.x * mscale); acc[r] += v.y * (q.y * mscale); acc[r] += v.z * (q.z * mscale); acc[r] += v.w * (q.w * mscale);
            }
        }
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r)
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
        float mine_v = acc[0];          // (after the butterfly every lane holds every row's sum)
#pragma unroll
        for (int r = 1; r < GEMV_ROWS; ++r) mine_v = lane == r ? acc[r] : mine_v;
        if (mine) emit(n, row0 + lane, mine_v, rc);
    }
}

__global__ void __launch_bounds__(GEMV_WAVES * 64) style_affine_fwd_kernel(const eg3d_style_bank b) {
    int row0;
    const int l = find_layer(b, blockIdx.x, GEMV_TILE, row0);
    if (l >= b.nlayers) return;
    const eg3d_style_layer& ly = b.layers[l];
    const int lane = threadIdx.x & 63;
    row0 += (threadIdx.x >> 6) * GEMV_ROWS;
    if (row0 >= ly.C) return;
    wave_rows_dot<false>(ly.weight, ly.C, b.D, row0, ly.wgain, b.ws + (int64_t)ly.wrow * b.D, (int64_t)b.L * b.D, b.N, ly.bias, lane, [&](int n, int j, float dot, float bias) {
        ly.out[(int64_t)n * ly.C + j] = (dot + bias * ly.bgain) * ly.post;          // (no bias: 0 * bgain)
    });
}

// demodulation coefficients of every conv layer of the bank: d[n, o] = rsqrt(sum_k s[n, k]^2 wsq[o, k] + 1e-8), the same GEMV over wsq
__global__ void __launch_bounds__(GEMV_WAVES * 64) style_demod_fwd_kernel(const eg3d_style_bank b) {
    int blk;
    const int l = find_tile(b, blockIdx.x, [](const eg3d_style_layer& q) { return q.wsq != nullptr ? (q.Co + GEMV_TILE - 1) / GEMV_TILE : 0; }, blk);
    if (l >= b.nlayers) return;
    const eg3d_style_layer& ly = b.layers[l];
    const int lane = threadIdx.x & 63, o0 = blk * GEMV_TILE + (threadIdx.x >> 6) * GEMV_ROWS;
    if (o0 >= ly.Co) return;
    if ((ly.C & 3) == 0 && ((reinterpret_cast<uintptr_t>(ly.wsq) | reinterpret_cast<uintptr_t>(ly.out)) & 15) == 0) {
        wave_rows_dot<true>(ly.wsq, ly.Co, ly.C, o0, 1.0f, ly.out, ly.C, b.N, nullptr, lane, [&](int n, int o, float dot, float) {
            ly.d[(int64_t)n * ly.Co + o] = 1.0f / sqrtf(dot + 1e-8f);
        });
        return;
    }
    for (int n = 0; n < b.N; ++n) {              // rows that 16-byte loads cannot walk (C % 4 != 0)
        const float* s = ly.out + (int64_t)n * ly.C;
        for (int o = o0; o < min(o0 + GEMV_ROWS, ly.Co); ++o) {
            const float* wq = ly.wsq + (int64_t)o * ly.C;
            float acc = 0.f;
            for (int k = lane; k < ly.C; k += 64) { const float sv = s[k]; acc += sv * sv * wq[k]; }
            for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
            if (lane == 0) ly.d[(int64_t)n * ly.Co + o] = 1.0f / sqrtf(acc + 1e-8f);
        }
    }
}

// emit(n, k, sum_r coef_of(n, row0 + r) * M[row0 + r, k], pre(n, k)) over the block's TILE rows, for every column k < K and every n: thread = (group of V
// columns, row group); the rows of a thread are loaded in one trip and stay in registers while the batch walks over them.  What the first round needs
// beside them -- its coefficient, and pre(), an operand of emit -- is in flight together with the rows, the next round's during the current one.
// K % V == 0, V == 4: M 16-byte aligned.  coef [TILE] and part [COLS_RG * COLS_KQ * V] are LDS.  Rows past `rows` are read at the tile's last row with a
// zero coefficient.
template <int TILE, int V, class Coef, class Pre, class Emit>
__device__ __forceinline__ void block_cols_sum(const float* __restrict__ M, int rows, int K, int row0, int N, float* coef, float* part,
                                               Coef coef_of, Pre pre, Emit emit) {
    constexpr int U = TILE / COLS_RG, CW = COLS_KQ * V;
    static_assert(TILE % COLS_RG == 0 && TILE <= COLS_THREADS && CW <= COLS_THREADS, "one thread per coefficient and per column of the chunk");
    const int tid = threadIdx.x, kq = tid & (COLS_KQ - 1), rg = tid / COLS_KQ;
    const int nrows = min(TILE, rows - row0);
    const bool has_coef = tid < nrows;
    for (int kc = 0; kc < K; kc += CW) {
        const int k = kc + kq * V;
        const bool kin = k < K, has_col = tid < CW && kc + tid < K;
        float w[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* p = M + (int64_t)(row0 + min(rg * U + u, nrows - 1)) * K + (kin ? k : 0);
            if constexpr (V == 4) { const float4 q = ld4(p); w[u][0] = q.x; w[u][1] = q.y; w[u][2] = q.z; w[u][3] = q.w; }
            else w[u][0] = *p;
        }
        // (after the rows in program order: the compiler waits for a coefficient where it is formed, and ahead of the rows that wait was a round trip of its own)
        // Clamped addresses, not branches: a load under a divergent branch is waited for inside it.
        const int crow = row0 + min(tid, nrows - 1), ecol = min(kc + tid, K - 1);
        float c_next = coef_of(0, crow), e_next = pre(0, ecol);
        for (int n = 0; n < N; ++n) {
            const float c_now = c_next, e_now = e_next;
            __syncthreads();                   // coef and part of the round before were read
            if (tid < TILE) coef[tid] = has_coef ? c_now : 0.f;
            __syncthreads();
            if (n + 1 < N) {
                c_next = coef_of(n + 1, crow);
                e_next = pre(n + 1, ecol);
            }
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float c = coef[rg * U + u];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += c * w[u][v];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) part[rg * CW + kq * V + v] = acc[v];
            __syncthreads();
            if (has_col) {
                float sum = part[tid];
#pragma unroll
                for (int g = 1; g < COLS_RG; ++g) sum += part[g * CW + tid];
                emit(n, kc + tid, sum, e_now);
            }
        }
    }
}

// dout_extra[n, k] += -s[n, k] * sum_o dd[n, o] d[n, o]^3 wsq[o, k]: one block per DEMOD_BWD_TILE rows o of a layer's wsq; dd d^3 is formed once per (n, o)
__global__ void __launch_bounds__(COLS_THREADS) style_demod_bwd_kernel(const eg3d_style_bank b) {
    __shared__ float coef[DEMOD_BWD_TILE];
    __shared__ __attribute__((aligned(16))) float part[COLS_RG * COLS_KQ * 4];
    int blk;
    const int l = find_tile(b, blockIdx.x, [](const eg3d_style_layer& q) {
        return (q.dd != nullptr && q.wsq != nullptr) ? (q.Co + DEMOD_BWD_TILE - 1) / DEMOD_BWD_TILE : 0; }, blk);
    if (l >= b.nlayers) return;
    const eg3d_style_layer& ly = b.layers[l];
    auto coef_of = [&](int n, int o) { const float dv = ly.d[(int64_t)n * ly.Co + o]; return ly.dd[(int64_t)n * ly.Co + o] * dv * dv * dv; };
    auto pre = [&](int n, int k) { return ly.out[(int64_t)n * ly.C + k]; };
    auto emit = [&](int n, int k, float t, float sv) { eg3d_acc(ly.dout_extra + (int64_t)n * ly.C + k, -sv * t); };
    if ((ly.C & 3) == 0 && (reinterpret_cast<uintptr_t>(ly.wsq) & 15) == 0)
        block_cols_sum<DEMOD_BWD_TILE, 4>(ly.wsq, ly.Co, ly.C, blk * DEMOD_BWD_TILE, b.N, coef, part, coef_of, pre, emit);
    else
        block_cols_sum<DEMOD_BWD_TILE, 1>(ly.wsq, ly.Co, ly.C, blk * DEMOD_BWD_TILE, b.N, coef, part, coef_of, pre, emit);
}

// dws[n, wrow, k] += sum_j ((dout[n, j] + dout_extra[n, j]) post wgain) W[j, k]: one block per AFFINE_BWD_TILE rows of a layer's affine weight
__global__ void __launch_bounds__(COLS_THREADS) style_affine_bwd_kernel(const eg3d_style_bank b) {
    __shared__ float coef[AFFINE_BWD_TILE];
    __shared__ __attribute__((aligned(16))) float part[COLS_RG * COLS_KQ * 4];
    int row0;
    const int l = find_layer(b, blockIdx.x, AFFINE_BWD_TILE, row0);
    if (l >= b.nlayers) return;
    const eg3d_style_layer& ly = b.layers[l];
    if (ly.dout == nullptr && ly.dout_extra == nullptr) return;
    block_cols_sum<AFFINE_BWD_TILE, 4>(ly.weight, ly.C, b.D, row0, b.N, coef, part,
        [&](int n, int j) {
            const int64_t i = (int64_t)n * ly.C + j;
            return ((ly.dout ? ly.dout[i] : 0.f) + (ly.dout_extra ? ly.dout_extra[i] : 0.f)) * ly.post * ly.wgain;
        },
        [](int, int) { return 0.f; },
        [&](int n, int k, float t, float) { eg3d_acc(b.dws + ((int64_t)n * b.L + ly.wrow) * b.D + k, t); });
}

// Gradients of trainable affines: the block owns rows [row0, row0+32) of its layer, so plain stores.
__global__ void __launch_bounds__(128) style_affine_wgrad_kernel(const eg3d_style_bank b) {
    int row0;
    const int l = find_layer(b, blockIdx.x, WGRAD_ROWS, row0);
    if (l >= b.nlayers) return;
    const eg3d_style_layer& ly = b.layers[l];
    if ((ly.dweight == nullptr && ly.dbias == nullptr) || (ly.dout == nullptr && ly.dout_extra == nullptr)) return;
    const int rows = min(WGRAD_ROWS, ly.C - row0);
    auto coef = [&](int n, int r) {
        const int64_t j = (int64_t)n * ly.C + row0 + r;
        return ((ly.dout ? ly.dout[j] : 0.f) + (ly.dout_extra ? ly.dout_extra[j] : 0.f)) * ly.post;
    };
    if (ly.dbias != nullptr && threadIdx.x < rows) {
        float s = 0.f;
        for (int n = 0; n < b.N; ++n) s += coef(n, threadIdx.x);
        ly.dbias[row0 + threadIdx.x] = s * ly.bgain;
    }
    if (ly.dweight == nullptr) return;
    for (int k = threadIdx.x * 4; k < b.D; k += 512) {
        for (int r = 0; r < rows; ++r) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int n = 0; n < b.N; ++n) {
                const float4 x = *reinterpret_cast<const float4*>(b.ws + ((int64_t)n * b.L + ly.wrow) * b.D + k);
                const float c = coef(n, r) * ly.wgain;
                acc.x += c * x.x; acc.y += c * x.y; acc.z += c * x.z; acc.w += c * x.w;
            }
            *reinterpret_cast<float4*>(ly.dweight + (int64_t)(row0 + r) * b.D + k) = acc;
        }
    }
}

int check_bank(const eg3d_style_bank* pb, bool bwd) {
    if (!pb) return EG3D_ERR_INVALID;
    const eg3d_style_bank& b = *pb;
    if (b.nlayers < 1 || b.nlayers > EG3D_STYLE_BANK_MAX || b.N < 1 || b.L < 1 || b.D < 4 || (b.D & 3)) return EG3D_ERR_INVALID;
    bool wants_wgrad = false;
    for (int l = 0; l < b.nlayers && l < EG3D_STYLE_BANK_MAX; ++l) wants_wgrad |= b.layers[l].dweight != nullptr || b.layers[l].dbias != nullptr;
    if (!b.ws || (bwd && !b.dws && !wants_wgrad)) return EG3D_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(b.ws) & 15) || (bwd && (reinterpret_cast<uintptr_t>(b.dws) & 15))) return EG3D_ERR_UNSUPPORTED;
    for (int l = 0; l < b.nlayers; ++l) {
        const eg3d_style_layer& ly = b.layers[l];
        if (!ly.weight || ly.C < 1 || ly.wrow < 0 || ly.wrow >= b.L) return EG3D_ERR_INVALID;
        if (!bwd && !ly.out) return EG3D_ERR_INVALID;
        if ((reinterpret_cast<uintptr_t>(ly.weight) & 15) || (reinterpret_cast<uintptr_t>(ly.dweight) & 15)) return EG3D_ERR_UNSUPPORTED;
    }
    return EG3D_OK;
}

int total_tiles(const eg3d_style_bank& b, int rows_per_block) {
    int t = 0;
    for (int l = 0; l < b.nlayers; ++l) t += eg3d_cdiv(b.layers[l].C, rows_per_block);
    return t;
}

}  // namespace

extern "C" int eg3d_style_affine_fwd(const eg3d_style_bank* pb, void* stream) {
    if (int rc = check_bank(pb, false)) return rc;
    hipLaunchKernelGGL(style_affine_fwd_kernel, dim3(total_tiles(*pb, GEMV_TILE)), dim3(GEMV_WAVES * 64), 0, (hipStream_t)stream, *pb);
    int dblocks = 0;
    for (int l = 0; l < pb->nlayers; ++l) {
        const eg3d_style_layer& ly = pb->layers[l];
        if (ly.wsq != nullptr) {
            if (ly.Co < 1 || ly.d == nullptr) return EG3D_ERR_INVALID;
            dblocks += eg3d_cdiv(ly.Co, GEMV_TILE);
        }
    }
    if (dblocks > 0) hipLaunchKernelGGL(style_demod_fwd_kernel, dim3(dblocks), dim3(GEMV_WAVES * 64), 0, (hipStream_t)stream, *pb);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_style_affine_bwd(const eg3d_style_bank* pb, void* stream) {
    if (int rc = check_bank(pb, true)) return rc;
    int dblocks = 0;
    for (int l = 0; l < pb->nlayers; ++l) {
        const eg3d_style_layer& ly = pb->layers[l];
        if (ly.dd != nullptr && ly.wsq != nullptr) {
            if (ly.Co < 1 || ly.d == nullptr || ly.dout_extra == nullptr || ly.out == nullptr) return EG3D_ERR_INVALID;
            dblocks += eg3d_cdiv(ly.Co, DEMOD_BWD_TILE);
        }
    }
    EG3D_DET_SCOPE(det, stream);
    for (int l = 0; l < pb->nlayers; ++l) {
        const eg3d_style_layer& ly = pb->layers[l];
        if (ly.dd != nullptr && ly.wsq != nullptr) { EG3D_DET_BIND(det, ly.dout_extra, (int64_t)pb->N * ly.C); }
    }
    EG3D_DET_BIND(det, pb->dws, (int64_t)pb->N * pb->L * pb->D);
    EG3D_DET_COMMIT(det);
    if (dblocks > 0) hipLaunchKernelGGL(style_demod_bwd_kernel, dim3(dblocks), dim3(COLS_THREADS), 0, (hipStream_t)stream, *pb);
    EG3D_DET_FLUSH(det);          // (the affine backward reads the demodulation part it just accumulated)
    if (pb->dws != nullptr) hipLaunchKernelGGL(style_affine_bwd_kernel, dim3(total_tiles(*pb, AFFINE_BWD_TILE)), dim3(COLS_THREADS), 0, (hipStream_t)stream, *pb);
    EG3D_DET_END(det);
    bool wants_wgrad = false;
    for (int l = 0; l < pb->nlayers; ++l) wants_wgrad |= pb->layers[l].dweight != nullptr || pb->layers[l].dbias != nullptr;
    if (wants_wgrad) hipLaunchKernelGGL(style_affine_wgrad_kernel, dim3(total_tiles(*pb, WGRAD_ROWS)), dim3(128), 0, (hipStream_t)stream, *pb);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
