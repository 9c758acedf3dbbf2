// Image ingestion (include/eg3d_hip.h "Image ingestion"): the pixel work of the reference's align_face (utils/alignment.py:72-111) and of
// ToTensor / Normalize on uint8 [N,H,W,C] images.
//
//   resample_h_kernel / resample_v_kernel   Pillow's 8-bit separable resize on host-built integer tables: the horizontal pass stages the row
//                                           segment each of its waves needs in LDS (the interleaved channel bytes of a row are otherwise read
//                                           with a stride), the vertical pass has its lanes along the bytes of a row and walks the rows
//   quad_warp_kernel                        Pillow's QUAD bilinear transform in fp64, Pillow's operation order, truncating store
//   fpad_blur_y / fpad_blur_x_blend         reflect pad on the fly, separable Gaussian (fp32, a pixel-fixed summation order), first blend
//   fpad_hist / fpad_select / fpad_above    exact per-channel median: radix select over the ordered float bits, 4 passes of 8 bits
//                                           (integer histograms: LDS, then one integer add per bin and workgroup)
//   fpad_final                              second blend towards the median, round half to even, uint8
//   u8_to_target_kernel                     (v / 255 - 0.5) / 0.5, NHWC -> NCHW
// and the way back (eg3d_paste_back8; no reference counterpart, the reference's alignment goes one way only):
//   paste_back_kernel                       N edited aligned frames blended into the one photograph they share: one thread per (frame, photo
//                                           pixel of the region), a wave along 64 pixels of a photo row; the affine map photo -> aligned frame,
//                                           quad_warp_kernel's bilinear taps (not truncated), a smoothstep feather from the frame's edge, an
//                                           optional mask through the same taps, round half to even -- fp64, the header's operation order,
//                                           no division; HWC or planar output (the JPEG encoder's input), the region alone or inside the photo
//   photo_frames_kernel / photo_frames16    the photo into every frame before the region is written (whole = 1): bytes (also HWC -> planes),
//                                           or 16 bytes per thread where the buffers allow
// Integer atomics only (order-independent) and no floating-point sum across threads: both builds and every batch size give the same bytes.
// The translation unit is compiled with -ffp-contract=off (Makefile): every product and sum below is its own rounded operation.
#include "common.h"

namespace {

constexpr int RS_LDS_BYTES = 48 * 1024;                                         // horizontal pass: all rows of a workgroup
constexpr int RS_MAX_ROWS = 4;                                                 // waves (rows) per workgroup
constexpr int IMG_MAX_SIDE = 65535;

// ---------------------------------------------------------------------------------------------------------------- resize
__device__ __forceinline__ uint8_t rs_clip8(int acc) { return (uint8_t)min(max(acc >> 22, 0), 255); }

// grid (ceil(Wo / 64), ceil(Hi / rows), N), block (64, rows): wave r of a workgroup owns input row blockIdx.y * rows + r
template <int CH>
__global__ void __launch_bounds__(64 * RS_MAX_ROWS) resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                      const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                                      int Hi, int Wi, int Wo, int seg, int ksize) {
    extern __shared__ uint8_t s_seg[];                                          // [rows][seg * CH]
    const int lane = threadIdx.x, r = threadIdx.y;
    const int y = blockIdx.y * blockDim.y + r, n = blockIdx.z;
    const int x0 = blockIdx.x * EG3D_RESAMPLE_TILE, x1 = min(x0 + EG3D_RESAMPLE_TILE, Wo);
    const int x = x0 + lane;
    int xmin = 0, count = 0;
    if (x < x1) {
        xmin = bounds[2 * x];
        count = bounds[2 * x + 1];
    }
    // the tile's span: xmin is non-decreasing in x for Pillow's tables, but take the wave's minimum and maximum rather than rely on it
    int lo = x < x1 ? xmin : INT32_MAX, hi = x < x1 ? xmin + count : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    lo = max(lo, 0);
    hi = min(hi, Wi);
    const int span = min(max(hi - lo, 0), seg);                               // never more than the LDS holds
    uint8_t* row = s_seg + (size_t)r * seg * CH;
    if (y < Hi) {
        const uint8_t* g = src + (((int64_t)n * Hi + y) * Wi + lo) * CH;
        for (int i = lane; i < span * CH; i += 64) row[i] = g[i];
    }
    __syncthreads();
    if (y >= Hi || x >= x1) return;
    uint8_t* o = dst + (((int64_t)n * Hi + y) * Wo + x) * CH;
    const int off = xmin - lo;
    if (count < 0 || count > ksize || off < 0 || off + count > span) {                           // tables that disagree with hseg: defined output, no stray read
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = 0;
        return;
    }
    int acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 1 << 21;
    const uint8_t* p = row + off * CH;
    for (int i = 0; i < count; ++i) {
        const int k = coef[(int64_t)i * Wo + x];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] += (int)p[i * CH + c] * k;
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) o[c] = rs_clip8(acc[c]);
}

// grid (ceil(rowbytes / 256), Ho, N): rowbytes = W * C, thread j owns byte column j
__global__ void __launch_bounds__(256) resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int32_t* __restrict__ bounds,
                                                         const int32_t* __restrict__ coef, int Hi, int Ho, int rowbytes, int ksize) {
    const int j = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y, n = blockIdx.z;
    if (j >= rowbytes) return;
    int ymin = bounds[2 * yo], count = bounds[2 * yo + 1];
    ymin = min(max(ymin, 0), Hi);
    count = min(min(max(count, 0), Hi - ymin), ksize);                          // stay inside the image and the table whatever the caller passed
    const uint8_t* p = src + ((int64_t)n * Hi + ymin) * rowbytes + j;
    const int32_t* k = coef + (int64_t)yo * ksize;
    int acc = 1 << 21;
    for (int i = 0; i < count; ++i) acc += (int)p[(int64_t)i * rowbytes] * k[i];
    dst[((int64_t)n * Ho + yo) * rowbytes + j] = rs_clip8(acc);
}

__global__ void __launch_bounds__(256) copy_bytes_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

bool img_dims_ok(int N, int H, int W, int C) {
    return N >= 1 && N <= IMG_MAX_SIDE && (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= IMG_MAX_SIDE && W <= IMG_MAX_SIDE;
}

int resample_geom(const eg3d_resample8_params* p, bool& horiz, bool& vert, int64_t& ws) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (!img_dims_ok(p->N, p->Hi, p->Wi, p->C) || !img_dims_ok(p->N, p->Ho, p->Wo, p->C)) return EG3D_ERR_INVALID;
    horiz = p->Wo != p->Wi;
    vert = p->Ho != p->Hi;
    if (horiz != (p->hbounds != nullptr) || horiz != (p->hcoef != nullptr) || vert != (p->vbounds != nullptr) || vert != (p->vcoef != nullptr))
        return EG3D_ERR_INVALID;
    if (horiz && (p->hksize < 1 || p->hseg < 1 || p->hseg > p->Wi)) return EG3D_ERR_INVALID;
    if (vert && p->vksize < 1) return EG3D_ERR_INVALID;
    if (horiz && (int64_t)p->hseg * p->C > RS_LDS_BYTES) return EG3D_ERR_UNSUPPORTED;
    ws = horiz && vert ? (int64_t)p->N * p->Hi * p->Wo * p->C : 0;
    return EG3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- QUAD warp
struct QuadCoef {
    double a[8];
};

template <int CH>
__global__ void __launch_bounds__(256) quad_warp_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, QuadCoef q, int Hi, int Wi, int Ho,
                                                        int Wo) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (x >= Wo || y >= Ho) return;
    uint8_t* o = dst + (((int64_t)n * Ho + y) * Wo + x) * CH;
    const double xi = x + 0.5, yi = y + 0.5;
    double xin = q.a[0] + q.a[1] * xi + q.a[2] * yi + q.a[3] * xi * yi;         // left to right, every operation rounded on its own
    double yin = q.a[4] + q.a[5] * xi + q.a[6] * yi + q.a[7] * xi * yi;
    if (!(xin >= 0.0 && xin < (double)Wi && yin >= 0.0 && yin < (double)Hi)) {   // also refuses NaN (a degenerate quad)
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = 0;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const double fxd = floor(xin), fyd = floor(yin);
    const double dx = xin - fxd, dy = yin - fyd;
    const int fx = (int)fxd, fy = (int)fyd;                                     // within [-1, side - 1]
    const int xa = min(max(fx, 0), Wi - 1), xb = min(max(fx + 1, 0), Wi - 1);
    const int ya = min(max(fy, 0), Hi - 1), yb = min(max(fy + 1, 0), Hi - 1);
    const uint8_t* ra = src + ((int64_t)n * Hi + ya) * Wi * CH;
    const uint8_t* rb = src + ((int64_t)n * Hi + yb) * Wi * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double p00 = ra[xa * CH + c], p01 = ra[xb * CH + c], p10 = rb[xa * CH + c], p11 = rb[xb * CH + c];
        const double r0 = p00 + (p01 - p00) * dx;
        const double r1 = p10 + (p11 - p10) * dx;
        const double v = r0 + (r1 - r0) * dy;
        o[c] = (uint8_t)(int)v;                                                 // truncation; v lies within [0, 255]
    }
}

// ---------------------------------------------------------------------------------------------------------------- feathered pad
struct FpadGeom {
    int32_t N, H, W, C, left, top, right, bottom, radius;
    int32_t Hp, Wp;
};

struct FpadState {                       // per (n, c)
    uint32_t prefix;                     // ordered key of the lower middle value, built 8 bits per pass
    uint32_t rank;                       // rank still to find among the keys that share the prefix
    uint32_t equal;                      // after the last pass: how many values equal the lower middle value
    uint32_t above;                      // smallest key greater than the lower middle value
};

// numpy 'reflect': no edge repeat, any distance.  One fold covers every index within n - 1 of the image (the common case: a tap radius or a
// pad below the side); the remainder arithmetic only runs beyond that
__device__ __forceinline__ int refl_index(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int f = i < 0 ? -i : 2 * (n - 1) - i;
    if ((unsigned)f < (unsigned)n) return f;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// numpy 'symmetric' (scipy 'reflect'): the edge repeats
__device__ __forceinline__ int symm_index(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int f = i < 0 ? -1 - i : 2 * n - 1 - i;
    if ((unsigned)f < (unsigned)n) return f;
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

__device__ __forceinline__ uint32_t fkey(float v) {                             // order-preserving map of the float bits
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float fpad_mask(const FpadGeom& g, int y, int x) {
    const float mx = fminf((float)x / (float)g.left, (float)(g.Wp - 1 - x) / (float)g.right);
    const float my = fminf((float)y / (float)g.top, (float)(g.Hp - 1 - y) / (float)g.bottom);
    return fmaxf(1.f - mx, 1.f - my);
}

// grid (ceil(Wp * C / 256), Hp, N): t[n][y][x][c] = sum over padded rows.  The padded image is never stored: P[y][x] = src[refl(y - top)][refl(x - left)]
__global__ void __launch_bounds__(256) fpad_blur_y_kernel(const uint8_t* __restrict__ src, const float* __restrict__ gw, FpadGeom g, float* __restrict__ t) {
    const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (j >= g.Wp * g.C) return;
    const int x = j / g.C, c = j - x * g.C;
    const uint8_t* col = src + (int64_t)n * g.H * g.W * g.C + (int64_t)refl_index(x - g.left, g.W) * g.C + c;
    const int64_t rs = (int64_t)g.W * g.C;
    float acc = gw[0] * (float)col[refl_index(y - g.top, g.H) * rs];
    for (int k = 1; k <= g.radius; ++k) {
        const float a = (float)col[refl_index(symm_index(y - k, g.Hp) - g.top, g.H) * rs];
        const float b = (float)col[refl_index(symm_index(y + k, g.Hp) - g.top, g.H) * rs];
        acc += gw[k] * (a + b);
    }
    t[((int64_t)n * g.Hp + y) * g.Wp * g.C + j] = acc;
}

// same grid: blur along x of t, then V = P + (B - P) clip(3 mask + 1, 0, 1)
__global__ void __launch_bounds__(256) fpad_blur_x_blend_kernel(const uint8_t* __restrict__ src, const float* __restrict__ gw, FpadGeom g,
                                                                const float* __restrict__ t, float* __restrict__ v) {
    const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (j >= g.Wp * g.C) return;
    const int x = j / g.C, c = j - x * g.C;
    const float* row = t + ((int64_t)n * g.Hp + y) * g.Wp * g.C + c;
    float acc = gw[0] * row[x * g.C];
    for (int k = 1; k <= g.radius; ++k) acc += gw[k] * (row[symm_index(x - k, g.Wp) * g.C] + row[symm_index(x + k, g.Wp) * g.C]);
    const float p = (float)src[(((int64_t)n * g.H + refl_index(y - g.top, g.H)) * g.W + refl_index(x - g.left, g.W)) * g.C + c];
    const float w = fminf(fmaxf(fpad_mask(g, y, x) * 3.f + 1.f, 0.f), 1.f);
    v[((int64_t)n * g.Hp + y) * g.Wp * g.C + j] = p + (acc - p) * w;
}

// grid (blocks, N): histogram of byte `shift / 8` of the keys that match the prefix found so far, per channel
__global__ void __launch_bounds__(256) fpad_hist_kernel(const float* __restrict__ v, FpadGeom g, const FpadState* __restrict__ state, int shift,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[3 * 256];
    __shared__ uint32_t s_prefix[3];
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) s_h[i] = 0u;
    if (threadIdx.x < g.C) s_prefix[threadIdx.x] = state[n * g.C + threadIdx.x].prefix;
    __syncthreads();
    const uint32_t himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    const int64_t total = (int64_t)g.Hp * g.Wp * g.C;                           // <= INT32_MAX (fpad_geom)
    const float* base = v + (int64_t)n * total;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((uint32_t)i % (uint32_t)g.C);
        const uint32_t k = fkey(base[i]);
        if ((k & himask) == (s_prefix[c] & himask)) atomicAdd(&s_h[c * 256 + ((k >> shift) & 255u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < g.C * 256; i += 256)
        if (s_h[i]) atomicAdd(&hist[(int64_t)n * g.C * 256 + i], s_h[i]);      // integer: the order of the additions does not matter
}

// grid (N * C), block 256: the bin that holds the rank; clears the histogram for the next pass
__global__ void __launch_bounds__(256) fpad_select_kernel(FpadState* __restrict__ state, uint32_t* __restrict__ hist, int shift) {
    __shared__ uint32_t s_h[256];
    uint32_t* h = hist + (int64_t)blockIdx.x * 256;
    s_h[threadIdx.x] = h[threadIdx.x];
    h[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        FpadState s = state[blockIdx.x];
        uint32_t cum = 0;
        int b = 0;
        for (; b < 255; ++b) {
            if (s.rank < cum + s_h[b]) break;
            cum += s_h[b];
        }
        s.prefix |= (uint32_t)b << shift;
        s.rank -= cum;
        s.equal = s_h[b];
        state[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) fpad_state_init_kernel(FpadState* __restrict__ state, int count, uint32_t rank) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) state[i] = FpadState{0u, rank, 0u, 0xffffffffu};
}

// grid (blocks, N): smallest key above the lower middle value (an even count averages the two middle values)
__global__ void __launch_bounds__(256) fpad_above_kernel(const float* __restrict__ v, FpadGeom g, FpadState* __restrict__ state) {
    __shared__ uint32_t s_min[3];
    __shared__ uint32_t s_prefix[3];
    const int n = blockIdx.y;
    if (threadIdx.x < 3) s_min[threadIdx.x] = 0xffffffffu;
    if (threadIdx.x < g.C) s_prefix[threadIdx.x] = state[n * g.C + threadIdx.x].prefix;
    __syncthreads();
    const int64_t total = (int64_t)g.Hp * g.Wp * g.C;
    const float* base = v + (int64_t)n * total;
    uint32_t best[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % g.C);
        const uint32_t k = fkey(base[i]);
        if (k > s_prefix[c]) {
            if (c == 0) best[0] = min(best[0], k);
            else if (c == 1) best[1] = min(best[1], k);
            else best[2] = min(best[2], k);
        }
    }
    for (int c = 0; c < g.C; ++c)
        if (best[c] != 0xffffffffu) atomicMin(&s_min[c], best[c]);
    __syncthreads();
    if (threadIdx.x < g.C && s_min[threadIdx.x] != 0xffffffffu) atomicMin(&state[n * g.C + threadIdx.x].above, s_min[threadIdx.x]);
}

// grid (ceil(Wp * C / 256), Hp, N)
__global__ void __launch_bounds__(256) fpad_final_kernel(const float* __restrict__ v, FpadGeom g, const FpadState* __restrict__ state, int even,
                                                         uint8_t* __restrict__ dst) {
    const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (j >= g.Wp * g.C) return;
    const int x = j / g.C, c = j - x * g.C;
    const FpadState s = state[n * g.C + c];
    const float lo = fkey_inv(s.prefix);
    float med = lo;
    if (even) {
        const float hi = s.rank + 1u < s.equal ? lo : fkey_inv(s.above);       // the upper middle value equals the lower one, or is the next larger
        med = (lo + hi) * 0.5f;
    }
    const int64_t i = ((int64_t)n * g.Hp + y) * g.Wp * g.C + j;
    const float a = v[i];
    const float w = fminf(fmaxf(fpad_mask(g, y, x), 0.f), 1.f);
    const float r = rintf(a + (med - a) * w);                                     // round half to even
    dst[i] = (uint8_t)(int)fminf(fmaxf(r, 0.f), 255.f);
}

int64_t fpad_align(int64_t b) { return (b + 15) / 16 * 16; }

struct FpadLayout {
    int64_t t, v, hist, state, total;
};

int fpad_geom(const eg3d_feather_pad_params* p, FpadGeom& g, FpadLayout& l) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (!img_dims_ok(p->N, p->H, p->W, p->C)) return EG3D_ERR_INVALID;
    if (p->left < 1 || p->top < 1 || p->right < 1 || p->bottom < 1 || p->radius < 0) return EG3D_ERR_INVALID;
    const int64_t Hp = (int64_t)p->H + p->top + p->bottom, Wp = (int64_t)p->W + p->left + p->right;
    if (Hp > IMG_MAX_SIDE || Wp > IMG_MAX_SIDE || p->radius > IMG_MAX_SIDE) return EG3D_ERR_TOO_LARGE;
    if (Hp * Wp * p->C > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.N = p->N; g.H = p->H; g.W = p->W; g.C = p->C;
    g.left = p->left; g.top = p->top; g.right = p->right; g.bottom = p->bottom; g.radius = p->radius;
    g.Hp = (int32_t)Hp; g.Wp = (int32_t)Wp;
    const int64_t img = fpad_align((int64_t)p->N * Hp * Wp * p->C * (int64_t)sizeof(float));
    l.t = 0;
    l.v = img;
    l.hist = 2 * img;
    l.state = l.hist + fpad_align((int64_t)p->N * p->C * 256 * (int64_t)sizeof(uint32_t));
    l.total = l.state + fpad_align((int64_t)p->N * p->C * (int64_t)sizeof(FpadState));
    return EG3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ToTensor + Normalize
__global__ void __launch_bounds__(256) u8_to_target_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int64_t hw, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                   // output index [n][c][pixel]
    if (i >= total) return;
    const int64_t nc = i / hw, px = i - nc * hw, n = nc / 3, c = nc - n * 3;
    const float v = (float)img[(n * hw + px) * 3 + c];
    out[i] = (v / 255.f - 0.5f) / 0.5f;                                          // IEEE division (HIP's default): not v * (1 / 255)
}

// ---------------------------------------------------------------------------------------------------------------- paste-back
struct PasteGeom {
    double m[6];
    double inv_feather, inv255;          // host doubles: no division on the device
    int64_t mask_stride;                 // bytes between the masks of two frames; 0: one mask for all
    int32_t Wp, S;
    int32_t x0, y0, rw, rh;              // the region in the photo
    int32_t Ho, Wo, ox, oy;              // a frame of dst and where the region starts in it
    int32_t chw;
};

// grid (ceil(total / 256), N): frame n of dst = the photo, its [total] bytes as they are (ch = 1) or its ch planes one after the other
__global__ void __launch_bounds__(256) photo_frames_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t hw, int ch) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = hw * ch;  // output index [c][pixel]
    if (i >= total) return;
    int64_t j = i;
    if (ch > 1) {
        const int64_t c = i / hw;
        j = (i - c * hw) * ch + c;
    }
    dst[(int64_t)blockIdx.y * total + i] = src[j];
}

// the same copy, 16 bytes per thread: grid (ceil(n16 / 256), N); both buffers 16-byte aligned and the photo a multiple of 16 bytes
__global__ void __launch_bounds__(256) photo_frames16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[(int64_t)blockIdx.y * n16 + i] = src[i];
}

// grid (ceil(rw / 64), ceil(rh / 4), N), block 256: a wave along 64 photo pixels of a row, one thread per (frame, region pixel)
template <int CH>
__global__ void __launch_bounds__(256) paste_back_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                         const uint8_t* __restrict__ mask, uint8_t* __restrict__ dst, PasteGeom g) {
    const int rx = blockIdx.x * 64 + (threadIdx.x & 63), ry = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (rx >= g.rw || ry >= g.rh) return;
    const int X = g.x0 + rx, Y = g.y0 + ry, S = g.S;
    const uint8_t* ph = photo + ((int64_t)Y * g.Wp + X) * CH;
    const int64_t plane = (int64_t)g.Ho * g.Wo, pix = (int64_t)(g.oy + ry) * g.Wo + (g.ox + rx);
    uint8_t* o = dst + (int64_t)n * plane * CH + (g.chw ? pix : pix * CH);
    const int64_t cs = g.chw ? plane : 1;
    const double Xc = X + 0.5, Yc = Y + 0.5, Sd = (double)S;
    const double u = g.m[0] + g.m[1] * Xc + g.m[2] * Yc;                          // left to right, every operation rounded on its own
    const double v = g.m[3] + g.m[4] * Xc + g.m[5] * Yc;
    if (!(u >= 0.0 && u < Sd && v >= 0.0 && v < Sd)) {                           // outside the aligned frame (or NaN): the photo's pixel
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c * cs] = ph[c];
        return;
    }
    const double xin = u - 0.5, yin = v - 0.5;
    const double fxd = floor(xin), fyd = floor(yin);
    const double dx = xin - fxd, dy = yin - fyd;
    const int fx = (int)fxd, fy = (int)fyd;                                     // within [-1, S - 1]
    const int xa = min(max(fx, 0), S - 1), xb = min(max(fx + 1, 0), S - 1);
    const int ya = min(max(fy, 0), S - 1), yb = min(max(fy + 1, 0), S - 1);
    const double d = fmin(fmin(u, Sd - u), fmin(v, Sd - v));
    const double f = g.inv_feather > 0.0 ? fmin(d * g.inv_feather, 1.0) : 1.0;
    double a = (f * f) * (3.0 - 2.0 * f);
    if (mask != nullptr) {
        const uint8_t* mk = mask + (int64_t)n * g.mask_stride;
        const double p00 = mk[(int64_t)ya * S + xa], p01 = mk[(int64_t)ya * S + xb], p10 = mk[(int64_t)yb * S + xa], p11 = mk[(int64_t)yb * S + xb];
        const double r0 = p00 + (p01 - p00) * dx;
        const double r1 = p10 + (p11 - p10) * dx;
        a = a * ((r0 + (r1 - r0) * dy) * g.inv255);
    }
    const uint8_t* ra = edits + (((int64_t)n * S + ya) * S) * CH;
    const uint8_t* rb = edits + (((int64_t)n * S + yb) * S) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double p00 = ra[xa * CH + c], p01 = ra[xb * CH + c], p10 = rb[xa * CH + c], p11 = rb[xb * CH + c];
        const double r0 = p00 + (p01 - p00) * dx;
        const double r1 = p10 + (p11 - p10) * dx;
        const double val = r0 + (r1 - r0) * dy;
        const double pv = ph[c];
        const double r = rint(pv + (val - pv) * a);                               // round half to even
        o[c * cs] = (uint8_t)(int)fmin(fmax(r, 0.0), 255.0);                      // a can pass 1 by a rounding: stay inside the byte
    }
}

}  // namespace

extern "C" int eg3d_paste_back8(const eg3d_paste_back8_params* p, void* stream) {
    if (p == nullptr || p->photo == nullptr || p->edits == nullptr || p->dst == nullptr) return EG3D_ERR_INVALID;
    if (!img_dims_ok(p->N, p->Hp, p->Wp, p->C) || !img_dims_ok(p->N, p->S, p->S, p->C)) return EG3D_ERR_INVALID;
    if (p->x0 < 0 || p->y0 < 0 || p->x1 < p->x0 || p->y1 < p->y0 || p->x1 > p->Wp || p->y1 > p->Hp) return EG3D_ERR_INVALID;
    if (p->layout != EG3D_PASTE_HWC && p->layout != EG3D_PASTE_CHW) return EG3D_ERR_INVALID;
    if (p->mask != nullptr && p->mask_frames != 1 && p->mask_frames != p->N) return EG3D_ERR_INVALID;
    if (!(p->inv_feather >= 0.0)) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int chw = p->layout == EG3D_PASTE_CHW;
    if (p->whole) {
        const int64_t hw = (int64_t)p->Hp * p->Wp, total = hw * p->C;
        const bool planes = chw && p->C > 1;                                     // one launch for the N frames (copy_bytes_kernel fills one buffer)
        const bool wide = !planes && total % 16 == 0 && ((reinterpret_cast<uintptr_t>(p->photo) | reinterpret_cast<uintptr_t>(p->dst)) & 15) == 0;
        if (wide)
            hipLaunchKernelGGL(photo_frames16_kernel, dim3((unsigned)((total / 16 + 255) / 256), (unsigned)p->N), dim3(256), 0, st,
                               reinterpret_cast<const uint4*>(p->photo), reinterpret_cast<uint4*>(p->dst), total / 16);
        else
            hipLaunchKernelGGL(photo_frames_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)p->N), dim3(256), 0, st, p->photo, p->dst,
                               planes ? hw : total, planes ? p->C : 1);
        EG3D_LAUNCH_CHECK();
    }
    PasteGeom g;
    for (int i = 0; i < 6; ++i) g.m[i] = p->m[i];
    g.inv_feather = p->inv_feather;
    g.inv255 = 1.0 / 255.0;
    g.mask_stride = p->mask != nullptr && p->mask_frames > 1 ? (int64_t)p->S * p->S : 0;
    g.Wp = p->Wp; g.S = p->S;
    g.x0 = p->x0; g.y0 = p->y0; g.rw = p->x1 - p->x0; g.rh = p->y1 - p->y0;
    g.Ho = p->whole ? p->Hp : g.rh; g.Wo = p->whole ? p->Wp : g.rw;
    g.ox = p->whole ? p->x0 : 0; g.oy = p->whole ? p->y0 : 0;
    g.chw = chw;
    if (g.rw == 0 || g.rh == 0) return EG3D_OK;
    const dim3 grid((unsigned)((g.rw + 63) / 64), (unsigned)((g.rh + 3) / 4), (unsigned)p->N);
    if (p->C == 3)
        hipLaunchKernelGGL(paste_back_kernel<3>, grid, dim3(256), 0, st, p->photo, p->edits, p->mask, p->dst, g);
    else
        hipLaunchKernelGGL(paste_back_kernel<1>, grid, dim3(256), 0, st, p->photo, p->edits, p->mask, p->dst, g);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_resample8_query_workspace(const eg3d_resample8_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    bool horiz, vert;
    int64_t ws;
    const int s = resample_geom(p, horiz, vert, ws);
    if (s != EG3D_OK) return s;
    *workspace_bytes = ws;
    return EG3D_OK;
}

extern "C" int eg3d_resample8(const eg3d_resample8_params* p, void* stream) {
    bool horiz, vert;
    int64_t ws;
    const int s = resample_geom(p, horiz, vert, ws);
    if (s != EG3D_OK) return s;
    if (p->src == nullptr || p->dst == nullptr || (ws > 0 && (p->workspace == nullptr || p->workspace_bytes < ws))) return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (!horiz && !vert) {
        const int64_t n = (int64_t)p->N * p->Hi * p->Wi * p->C;
        hipLaunchKernelGGL(copy_bytes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->src, p->dst, n);
        EG3D_LAUNCH_CHECK();
        return EG3D_OK;
    }
    const uint8_t* cur = p->src;
    if (horiz) {
        uint8_t* hdst = vert ? reinterpret_cast<uint8_t*>(p->workspace) : p->dst;
        const int rowlds = p->hseg * p->C;
        int rows = RS_LDS_BYTES / rowlds;
        rows = rows > RS_MAX_ROWS ? RS_MAX_ROWS : rows;                          // >= 1: resample_geom refused hseg * C > RS_LDS_BYTES
        const dim3 grid((unsigned)((p->Wo + EG3D_RESAMPLE_TILE - 1) / EG3D_RESAMPLE_TILE), (unsigned)((p->Hi + rows - 1) / rows), (unsigned)p->N);
        const size_t lds = (size_t)rows * rowlds;
        if (p->C == 3)
            hipLaunchKernelGGL(resample_h_kernel<3>, grid, dim3(64, rows), lds, st, cur, hdst, p->hbounds, p->hcoef, p->Hi, p->Wi, p->Wo, p->hseg, p->hksize);
        else
            hipLaunchKernelGGL(resample_h_kernel<1>, grid, dim3(64, rows), lds, st, cur, hdst, p->hbounds, p->hcoef, p->Hi, p->Wi, p->Wo, p->hseg, p->hksize);
        EG3D_LAUNCH_CHECK();
        cur = hdst;
    }
    if (vert) {
        const int rowbytes = p->Wo * p->C;
        hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)((rowbytes + 255) / 256), (unsigned)p->Ho, (unsigned)p->N), dim3(256), 0, st, cur, p->dst,
                           p->vbounds, p->vcoef, p->Hi, p->Ho, rowbytes, p->vksize);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_quad_warp8(const eg3d_quad_warp8_params* p, void* stream) {
    if (p == nullptr || p->src == nullptr || p->dst == nullptr) return EG3D_ERR_INVALID;
    if (!img_dims_ok(p->N, p->Hi, p->Wi, p->C) || !img_dims_ok(p->N, p->Ho, p->Wo, p->C)) return EG3D_ERR_INVALID;
    QuadCoef q;
    for (int i = 0; i < 8; ++i) q.a[i] = p->a[i];
    const dim3 grid((unsigned)((p->Wo + 63) / 64), (unsigned)((p->Ho + 3) / 4), (unsigned)p->N);
    hipStream_t st = (hipStream_t)stream;
    if (p->C == 3)
        hipLaunchKernelGGL(quad_warp_kernel<3>, grid, dim3(256), 0, st, p->src, p->dst, q, p->Hi, p->Wi, p->Ho, p->Wo);
    else
        hipLaunchKernelGGL(quad_warp_kernel<1>, grid, dim3(256), 0, st, p->src, p->dst, q, p->Hi, p->Wi, p->Ho, p->Wo);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_feather_pad_query_workspace(const eg3d_feather_pad_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    FpadGeom g;
    FpadLayout l;
    const int s = fpad_geom(p, g, l);
    if (s != EG3D_OK) return s;
    *workspace_bytes = l.total;
    return EG3D_OK;
}

extern "C" int eg3d_feather_pad(const eg3d_feather_pad_params* p, void* stream) {
    FpadGeom g;
    FpadLayout l;
    const int s = fpad_geom(p, g, l);
    if (s != EG3D_OK) return s;
    if (p->src == nullptr || p->dst == nullptr || p->gauss == nullptr || p->workspace == nullptr || p->workspace_bytes < l.total ||
        (reinterpret_cast<uintptr_t>(p->workspace) & 15))
        return EG3D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(p->workspace);
    float* t = reinterpret_cast<float*>(ws + l.t);
    float* v = reinterpret_cast<float*>(ws + l.v);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + l.hist);
    FpadState* state = reinterpret_cast<FpadState*>(ws + l.state);
    const int rowelems = g.Wp * g.C, nc = g.N * g.C;
    const dim3 pix((unsigned)((rowelems + 255) / 256), (unsigned)g.Hp, (unsigned)g.N);
    hipLaunchKernelGGL(fpad_blur_y_kernel, pix, dim3(256), 0, st, p->src, p->gauss, g, t);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(fpad_blur_x_blend_kernel, pix, dim3(256), 0, st, p->src, p->gauss, g, (const float*)t, v);
    EG3D_LAUNCH_CHECK();
    const int64_t count = (int64_t)g.Hp * g.Wp;                                  // values per (n, c)
    const int even = count % 2 == 0;
    eg3d_zero_words(hist, (int64_t)nc * 256, st);
    hipLaunchKernelGGL(fpad_state_init_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, state, nc, (uint32_t)((count - 1) / 2));
    EG3D_LAUNCH_CHECK();
    int64_t blocks = (count * g.C + 256 * 16 - 1) / (256 * 16);                  // 16 values per thread
    blocks = blocks > 1024 ? 1024 : blocks;
    const dim3 scan((unsigned)blocks, (unsigned)g.N);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(fpad_hist_kernel, scan, dim3(256), 0, st, (const float*)v, g, (const FpadState*)state, shift, hist);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(fpad_select_kernel, dim3((unsigned)nc), dim3(256), 0, st, state, hist, shift);
        EG3D_LAUNCH_CHECK();
    }
    if (even) {
        hipLaunchKernelGGL(fpad_above_kernel, scan, dim3(256), 0, st, (const float*)v, g, state);
        EG3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fpad_final_kernel, pix, dim3(256), 0, st, (const float*)v, g, (const FpadState*)state, even, p->dst);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_u8_to_target(const uint8_t* img, int N, int H, int W, float* out, void* stream) {
    if (img == nullptr || out == nullptr || N < 1 || H < 1 || W < 1) return EG3D_ERR_INVALID;
    const int64_t hw = (int64_t)H * W, total = hw * 3 * N;
    if ((total + 255) / 256 > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    hipLaunchKernelGGL(u8_to_target_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, out, hw, total);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
