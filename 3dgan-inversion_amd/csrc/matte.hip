// Head mattes (include/eg3d_hip.h "Head mattes"): from a ragged binary mask in the aligned frame to the soft matte paste_back_kernel
// (csrc/imgprep.hip) takes.  No reference counterpart: the reference thresholds its depth (training/warping_loss.py:12-16) and stops there.
//
//   edt_column_kernel    TILED column pass: one thread per column, a wave along 64 adjacent columns (coalesced rows), a down and an up sweep
//                        that leave the signed column distance g of every pixel (int16; see below) in the workspace, in place
//   edt_row_kernel       TILED row pass: a row's g in LDS (several rows per workgroup while they fit the block), every lane scans outwards
//                        from its own x (x -/+ k) from best = g(x)^2 and stops at k^2 >= best; consecutive lanes read consecutive LDS
//                        addresses; a row wider than the block is a loop.  Writes the final sd2, or the next stage's binary image over g
//   edt_resident_kernel  RESIDENT: one workgroup per frame of H W <= 16384 pixels, g in 32 KB of LDS, every stage and the final transform in
//                        one launch with barriers between the passes (measured slower than TILED's launches: AUTO does not pick it)
//   matte8_kernel        sd2 -> uint8 at the output resolution: one thread per output pixel, a wave along 64 pixels of a row (the shape of
//                        paste_back_kernel), fp64 in the header's operation order
//
// One signed distance per pixel carries both column distances: at a foreground pixel the distance to the column's nearest foreground pixel is 0
// and g = +(distance to its nearest background pixel); at a background pixel g = -(distance to its nearest foreground pixel).  The row
// minimum of a foreground pixel runs over g_bg(x') = max(g(x'), 0), that of a background pixel over g_fg(x') = max(-g(x'), 0).  |g| is
// 1..4095 or the sentinel 2^14, so it fits int16, and the sign of g is the binary image.
// Integers and per-thread fp64 only, no atomics, no sum across threads: both builds and every batch size give the same bytes.
#include "common.h"

namespace {

constexpr int EDT_SENT = 1 << 14;                                               // a column without the class: the distance saturates here
constexpr int EDT_MAX_SIDE = 4096;
constexpr int EDT_RES_PIX = 16384;                                              // RESIDENT: pixels per frame (int16 each: 32 KB of LDS)
constexpr int EDT_RES_THREADS = 1024;
constexpr int EDT_RES_PER = EDT_RES_PIX / EDT_RES_THREADS;
constexpr int MATTE_MAX_SIDE = 16384;

// one step of a column sweep: dF / dB = the distance to the nearest foreground / background pixel met so far, this pixel included
__device__ __forceinline__ int edt_step(bool fg, int& dF, int& dB) {
    if (fg) {
        dF = 0;
        dB = min(dB + 1, EDT_SENT);
        return dB;
    }
    dB = 0;
    dF = min(dF + 1, EDT_SENT);
    return -dF;
}

// the two sweeps of one column; g points at the column's first pixel, rows are `stride` apart; is_fg(y) is read before g[y] is written
template <typename G, typename F>
__device__ __forceinline__ void edt_column(G* g, int H, int stride, F is_fg) {
    int dF = EDT_SENT, dB = EDT_SENT;
#pragma unroll 8
    for (int y = 0; y < H; ++y) g[y * stride] = (int16_t)edt_step(is_fg(y), dF, dB);
    dF = dB = EDT_SENT;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {
        const int v = g[y * stride];
        const bool fg = v > 0;
        const int w = edt_step(fg, dF, dB);
        g[y * stride] = (int16_t)(fg ? min(v, w) : max(v, w));                 // the nearer of above and below, sign kept
    }
}

// the signed squared distance of pixel x of a row whose g is s[0..W): exact, whatever the stopping rule cuts
__device__ __forceinline__ int edt_row_scan(const int16_t* s, int x, int W) {
    const int v = s[x];
    const int sg = v > 0 ? 1 : -1;
    int best = v * v;                                                           // 2^28 at the sentinel
    for (int k = 1; k * k < best; ++k) {
        const int xl = x - k, xr = x + k, kk = k * k;
        if (xl < 0 && xr >= W) break;
        if (xl >= 0) {
            const int m = max(sg * (int)s[xl], 0);
            best = min(best, kk + m * m);
        }
        if (xr < W) {
            const int m = max(sg * (int)s[xr], 0);
            best = min(best, kk + m * m);
        }
    }
    return sg * best;
}

// grid N * ceil(W / 64), block 64: thread = one column of one frame.  FROM_SRC: the binary image is src != 0, else the sign of g
template <bool FROM_SRC>
__global__ void __launch_bounds__(64) edt_column_kernel(const uint8_t* __restrict__ src, int16_t* __restrict__ g, int H, int W, int cblocks) {
    const int n = blockIdx.x / cblocks, x = (blockIdx.x - n * cblocks) * 64 + threadIdx.x;
    if (x >= W) return;
    const int64_t base = (int64_t)n * H * W + x;
    int16_t* col = g + base;
    if (FROM_SRC) {
        const uint8_t* sc = src + base;
        edt_column(col, H, W, [&](int y) { return sc[y * W] != 0; });
    } else {
        edt_column(col, H, W, [&](int y) { return col[y * W] > 0; });
    }
}

// grid ceil(rows / R), block 256, LDS R * wpad int16: rows = N H (a row knows nothing of its frame); T threads along a row, R rows per block
__global__ void __launch_bounds__(256) edt_row_kernel(int16_t* __restrict__ g, int32_t* __restrict__ sd2, int64_t rows, int W, int R, int T,
                                                      int wpad, int final_pass, int thr) {
    extern __shared__ int16_t s_rows[];
    const int r = threadIdx.x / T, x0 = threadIdx.x - r * T;
    const int64_t row = (int64_t)blockIdx.x * R + r;
    const bool active = r < R && row < rows;
    int16_t* s = s_rows + r * wpad;
    int16_t* grow = g + row * W;
    if (active)
        for (int x = x0; x < W; x += T) s[x] = grow[x];
    __syncthreads();
    if (!active) return;
    for (int x = x0; x < W; x += T) {
        const int d = edt_row_scan(s, x, W);
        if (final_pass)
            sd2[row * W + x] = d;
        else
            grow[x] = d > thr ? 1 : -1;                                         // the next stage's binary image; the row is in LDS already
    }
}

struct EdtStages {
    int32_t n;
    int32_t t[4];
};

// grid N, block 1024: one frame per workgroup, H W <= EDT_RES_PIX
__global__ void __launch_bounds__(EDT_RES_THREADS) edt_resident_kernel(const uint8_t* __restrict__ src, int32_t* __restrict__ sd2, int H, int W,
                                                                       EdtStages st) {
    __shared__ int16_t s[EDT_RES_PIX];
    const int tid = threadIdx.x, hw = H * W;
    src += (int64_t)blockIdx.x * hw;
    sd2 += (int64_t)blockIdx.x * hw;
    for (int p = tid; p < hw; p += EDT_RES_THREADS) s[p] = src[p] != 0 ? 1 : -1;
    __syncthreads();
    for (int stage = 0;; ++stage) {
        for (int x = tid; x < W; x += EDT_RES_THREADS) {
            int16_t* col = s + x;
            edt_column(col, H, W, [&](int y) { return col[y * W] > 0; });
        }
        __syncthreads();
        if (stage == st.n) break;
        const int thr = st.t[stage];
        uint32_t keep = 0;                                                     // this thread's pixels of the next binary image
#pragma unroll
        for (int i = 0; i < EDT_RES_PER; ++i) {
            const int p = tid + i * EDT_RES_THREADS;
            if (p < hw) {
                const int y = p / W;
                if (edt_row_scan(s + y * W, p - y * W, W) > thr) keep |= 1u << i;
            }
        }
        __syncthreads();                                                        // every scan has read g
#pragma unroll
        for (int i = 0; i < EDT_RES_PER; ++i) {
            const int p = tid + i * EDT_RES_THREADS;
            if (p < hw) s[p] = (keep >> i) & 1u ? 1 : -1;
        }
        __syncthreads();
    }
    for (int p = tid; p < hw; p += EDT_RES_THREADS) {
        const int y = p / W;
        sd2[p] = edt_row_scan(s + y * W, p - y * W, W);
    }
}

// ---------------------------------------------------------------------------------------------------------------- matte
struct MatteGeom {
    double step, inv_step, shrink_px, inv_feather;
    int64_t rows;                        // N Ho
    int32_t Hs, Ws, Ho, Wo;
};

__device__ __forceinline__ double matte_tap(int s) {                             // the contour lies half-way between centres
    return s > 0 ? sqrt((double)s) - 0.5 : -(sqrt(-(double)s) - 0.5);
}

// grid (ceil(N Ho / 4), ceil(Wo / 64)), block 256: a wave along 64 output pixels of a row
__global__ void __launch_bounds__(256) matte8_kernel(const int32_t* __restrict__ sd2, uint8_t* __restrict__ out, MatteGeom g) {
    const int X = blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (X >= g.Wo || row >= g.rows) return;
    const int64_t n = row / g.Ho;
    const int Y = (int)(row - n * g.Ho);
    const double u = (X + 0.5) * g.step - 0.5, v = (Y + 0.5) * g.step - 0.5;       // every operation rounded on its own
    const double fxd = floor(u), fyd = floor(v);
    const double dx = u - fxd, dy = v - fyd;
    const int fx = (int)fxd, fy = (int)fyd;
    const int xa = min(max(fx, 0), g.Ws - 1), xb = min(max(fx + 1, 0), g.Ws - 1);
    const int ya = min(max(fy, 0), g.Hs - 1), yb = min(max(fy + 1, 0), g.Hs - 1);
    const int32_t* f = sd2 + n * g.Hs * g.Ws;
    const double p00 = matte_tap(f[ya * g.Ws + xa]), p01 = matte_tap(f[ya * g.Ws + xb]);
    const double p10 = matte_tap(f[yb * g.Ws + xa]), p11 = matte_tap(f[yb * g.Ws + xb]);
    const double r0 = p00 + (p01 - p00) * dx;
    const double r1 = p10 + (p11 - p10) * dx;
    const double val = r0 + (r1 - r0) * dy;
    const double e = val * g.inv_step - g.shrink_px;
    const double t = g.inv_feather > 0.0 ? fmin(fmax(e * g.inv_feather, 0.0), 1.0) : (e > 0.0 ? 1.0 : 0.0);
    const double a = (t * t) * (3.0 - 2.0 * t);
    out[row * g.Wo + X] = (uint8_t)(int)rint(255.0 * a);                          // round half to even; a is within [0, 1]
}

// the checks of both entries; *impl = the path that runs
int edt2_resolve(const eg3d_edt2_params* p, int* impl) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (p->N < 1 || p->H < 1 || p->W < 1 || p->n_stages < 0 || p->n_stages > EG3D_EDT_MAX_STAGES) return EG3D_ERR_INVALID;
    if (p->impl != EG3D_EDT_AUTO && p->impl != EG3D_EDT_RESIDENT && p->impl != EG3D_EDT_TILED) return EG3D_ERR_INVALID;
    if (p->H > EDT_MAX_SIDE || p->W > EDT_MAX_SIDE || (int64_t)p->N * p->H * p->W >= ((int64_t)1 << 31)) return EG3D_ERR_UNSUPPORTED;
    const bool fits = (int64_t)p->H * p->W <= EDT_RES_PIX;
    if (p->impl == EG3D_EDT_RESIDENT && !fits) return EG3D_ERR_UNSUPPORTED;
    // AUTO is TILED at every size: measured (DESIGN.md 3.4 "Head mattes"), the default chain on 128^2 frames takes 300 us in its ten launches
    // and 633 us in RESIDENT's one -- a frame's row scans are latency-bound on the one CU that holds it, and spread over 64 workgroups otherwise
    *impl = p->impl == EG3D_EDT_AUTO ? EG3D_EDT_TILED : p->impl;
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_edt2_query_workspace(const eg3d_edt2_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    int impl;
    const int rc = edt2_resolve(p, &impl);
    if (rc != EG3D_OK) return rc;
    *workspace_bytes = impl == EG3D_EDT_TILED ? (int64_t)p->N * p->H * p->W * (int64_t)sizeof(int16_t) : 0;
    return EG3D_OK;
}

extern "C" int eg3d_edt2(const eg3d_edt2_params* p, void* stream) {
    int impl;
    int64_t need;
    const int rc = edt2_resolve(p, &impl);
    if (rc != EG3D_OK) return rc;
    if (p->src == nullptr || p->sd2 == nullptr) return EG3D_ERR_INVALID;
    eg3d_edt2_query_workspace(p, &need);
    if (need > 0 && (p->workspace == nullptr || p->workspace_bytes < need || (reinterpret_cast<uintptr_t>(p->workspace) & 1) != 0))
        return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (impl == EG3D_EDT_RESIDENT) {
        EdtStages stg;
        stg.n = p->n_stages;
        for (int i = 0; i < EG3D_EDT_MAX_STAGES; ++i) stg.t[i] = p->t[i];
        hipLaunchKernelGGL(edt_resident_kernel, dim3((unsigned)p->N), dim3(EDT_RES_THREADS), 0, st, p->src, p->sd2, p->H, p->W, stg);
        EG3D_LAUNCH_CHECK();
        return EG3D_OK;
    }
    int16_t* g = static_cast<int16_t*>(p->workspace);
    const int W = p->W, cblocks = (W + 63) / 64, w64 = cblocks * 64;
    const int T = w64 >= 256 ? 256 : w64, R = w64 >= 256 ? 1 : 256 / w64;       // threads along a row, rows per workgroup
    const int64_t rows = (int64_t)p->N * p->H;
    const dim3 cgrid((unsigned)((int64_t)p->N * cblocks)), rgrid((unsigned)((rows + R - 1) / R));
    const size_t lds = (size_t)R * w64 * sizeof(int16_t);
    for (int stage = 0; stage <= p->n_stages; ++stage) {
        if (stage == 0)
            hipLaunchKernelGGL(edt_column_kernel<true>, cgrid, dim3(64), 0, st, p->src, g, p->H, W, cblocks);
        else
            hipLaunchKernelGGL(edt_column_kernel<false>, cgrid, dim3(64), 0, st, p->src, g, p->H, W, cblocks);
        EG3D_LAUNCH_CHECK();
        const int last = stage == p->n_stages;
        hipLaunchKernelGGL(edt_row_kernel, rgrid, dim3(256), lds, st, g, p->sd2, rows, W, R, T, w64, last, last ? 0 : p->t[stage]);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_matte8(const eg3d_matte8_params* p, void* stream) {
    if (p == nullptr || p->sd2 == nullptr || p->dst == nullptr) return EG3D_ERR_INVALID;
    if (p->N < 1 || p->Hs < 1 || p->Ws < 1 || p->Ho < 1 || p->Wo < 1) return EG3D_ERR_INVALID;
    if ((int64_t)p->Ho * p->Ws != (int64_t)p->Wo * p->Hs) return EG3D_ERR_INVALID;                // one scale for both axes
    if (!(p->step > 0.0) || !(p->inv_step > 0.0) || !(p->inv_feather >= 0.0) || !(p->shrink_px == p->shrink_px)) return EG3D_ERR_INVALID;
    if (p->Hs > EDT_MAX_SIDE || p->Ws > EDT_MAX_SIDE || p->Ho > MATTE_MAX_SIDE || p->Wo > MATTE_MAX_SIDE ||
        (int64_t)p->N * p->Hs * p->Ws >= ((int64_t)1 << 31) || (int64_t)p->N * p->Ho * p->Wo >= ((int64_t)1 << 31))
        return EG3D_ERR_UNSUPPORTED;
    MatteGeom g;
    g.step = p->step; g.inv_step = p->inv_step; g.shrink_px = p->shrink_px; g.inv_feather = p->inv_feather;
    g.rows = (int64_t)p->N * p->Ho;
    g.Hs = p->Hs; g.Ws = p->Ws; g.Ho = p->Ho; g.Wo = p->Wo;
    const dim3 grid((unsigned)((g.rows + 3) / 4), (unsigned)((p->Wo + 63) / 64));
    hipLaunchKernelGGL(matte8_kernel, grid, dim3(256), 0, (hipStream_t)stream, p->sd2, p->dst, g);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
