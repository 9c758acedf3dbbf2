// Batched baseline JPEG encoder (media export: the frames of the orbit videos; include/eg3d_hip.h "Baseline JPEG encoder").
//
// Four launches per batch of N frames, integer arithmetic only:
//   jpeg_dct_kernel      one wave per 8 x 8 block in scan order (4 per workgroup): colour conversion, replicate padding, 4:2:0 averaging, the
//                        two passes of the integer DCT through LDS, quantisation                              -> int16 coefficients, zigzag order
//   jpeg_entropy_kernel  one wave per restart interval: per block every lane codes its own coefficient (run length from a ballot of the
//                        non-zero lanes, ZRLs and the Huffman code packed into one 64-bit pattern), a wave scan of the bit counts places the
//                        patterns, integer LDS OR assembles them (order-independent); then the bytes are stuffed (ballot + popcount) into the
//                        interval's slot of the workspace, followed by RSTm / EOI                             -> slot bytes, slot length
//   jpeg_offsets_kernel  one workgroup: exclusive scan of header and slot lengths                            -> offsets[N + 1], slot destinations
//   (the host reads offsets[N] and allocates)
//   jpeg_pack_kernel     one workgroup per interval: header (first interval of a frame) and slot into the output
// No atomics on global memory, no floating-point sums: the output is a function of the input (bit-identical between runs and builds).
#include "common.h"

#define JPEG_TABLE static __constant__ const
#include "jpeg_tables.h"

namespace {

constexpr int JPEG_BLOCK_BITS = 22 + 63 * 26;                                  // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits, 63 times
constexpr int JPEG_MAX_BLOCKS = EG3D_JPEG_MAX_RESTART * 6;                     // per interval (4:2:0: 6 blocks per MCU)
constexpr int JPEG_LDS_WORDS = (JPEG_MAX_BLOCKS * JPEG_BLOCK_BITS + 31) / 32 + 4;   // + the words a 64-bit pattern may touch past the last bit
constexpr int JPEG_SCAN_THREADS = 1024;
constexpr int64_t JPEG_ALIGN = 16;

struct JpegGeom {
    int32_t N, C, H, W, dtype;
    int32_t s420;                        // 1: 4:2:0 (C = 3 only)
    int32_t mx, mcus;                    // MCUs per row, per frame
    int32_t bpm, nblk;                   // blocks per MCU, per frame
    int32_t R, I;                        // MCUs per interval, intervals per frame
    int32_t qscale;                      // jpeg_quality_scaling(quality)
    int32_t hdr;                         // header bytes
    int64_t stride;                      // slot bytes per interval
};

__device__ __forceinline__ int jpeg_px(const void* __restrict__ img, int dtype, int64_t idx) {
    if (dtype == EG3D_JPEG_U8) return (int)reinterpret_cast<const uint8_t*>(img)[idx];
    const float v = reinterpret_cast<const float*>(img)[idx] * 127.5f + 128.f;                 // (-ffp-contract=off: a product, then a sum)
    return (int)fminf(fmaxf(v, 0.f), 255.f);                                                  // truncation, as eg3d_image_grid_u8
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of the full-resolution pixel (y, x), coordinates clamped to the image (replicate padding)
__device__ __forceinline__ int jpeg_sample(const void* __restrict__ img, const JpegGeom& g, int n, int comp, int y, int x) {
    y = min(y, g.H - 1);
    x = min(x, g.W - 1);
    const int64_t hw = (int64_t)g.H * g.W, base = (int64_t)n * g.C * hw + (int64_t)y * g.W + x;
    if (g.C == 1) return jpeg_px(img, g.dtype, base);
    const int r = jpeg_px(img, g.dtype, base), gr = jpeg_px(img, g.dtype, base + hw), b = jpeg_px(img, g.dtype, base + 2 * hw);
    if (comp == 0) return (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * gr + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * gr - 5329 * b + 8388608 + 32767) >> 16;
}

__global__ void __launch_bounds__(256) jpeg_dct_kernel(const void* __restrict__ img, JpegGeom g, int16_t* __restrict__ coef) {
    __shared__ int s_ci[64];
    __shared__ int s_s[4][64], s_t[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 64) s_ci[threadIdx.x] = jpeg_ci[threadIdx.x];
    const int64_t blk = (int64_t)blockIdx.x * 4 + wave;
    const bool active = blk < (int64_t)g.N * g.nblk;
    int comp = 0;
    if (active) {
        const int n = (int)(blk / g.nblk), b = (int)(blk % g.nblk);
        const int mcu = b / g.bpm, k = b % g.bpm, my = mcu / g.mx, mxi = mcu % g.mx;
        const int y = lane >> 3, x = lane & 7;
        int p;
        if (g.s420) {
            if (k < 4) {
                p = jpeg_sample(img, g, n, 0, my * 16 + (k >> 1) * 8 + y, mxi * 16 + (k & 1) * 8 + x);
            } else {
                comp = k - 3;
                const int cy = 2 * (my * 8 + y), cx = 2 * (mxi * 8 + x);
                p = (jpeg_sample(img, g, n, comp, cy, cx) + jpeg_sample(img, g, n, comp, cy, cx + 1) + jpeg_sample(img, g, n, comp, cy + 1, cx) +
                     jpeg_sample(img, g, n, comp, cy + 1, cx + 1) + 2) >> 2;
            }
        } else {
            comp = k;                                                              // 4:4:4: Y Cb Cr; grey: k = 0
            p = jpeg_sample(img, g, n, comp, my * 8 + y, mxi * 8 + x);
        }
        s_s[wave][lane] = p - 128;
    }
    __syncthreads();
    const int u = lane >> 3, v = lane & 7;
    if (active) {
        int acc = 0;                                                               // T[u][x] = sum_y CI[u][y] S[y][x], x = v
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += s_ci[u * 8 + y] * s_s[wave][y * 8 + v];
        s_t[wave][lane] = (acc + 1024) >> 11;
    }
    __syncthreads();
    if (active) {
        int acc = 0;                                                               // D[u][v] = sum_x T[u][x] CI[v][x]
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += s_t[wave][u * 8 + x] * s_ci[v * 8 + x];
        const int d = (acc + 16384) >> 15;
        const int q = min(max(((int)jpeg_quant_base[comp ? 1 : 0][lane] * g.qscale + 50) / 100, 1), 255);
        const int m = (abs(d) + (q >> 1)) / q;
        coef[blk * 64 + jpeg_zz_of_nat[lane]] = (int16_t)(d < 0 ? -m : m);
    }
}

__device__ __forceinline__ int jpeg_bitlen(int v) { return v ? 32 - __clz(v) : 0; }

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const int16_t* __restrict__ coef, JpegGeom g, uint8_t* __restrict__ slots,
                                                          int32_t* __restrict__ lens) {
    __shared__ uint32_t s_bits[JPEG_LDS_WORDS];
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int n = (int)(j / g.I), iv = (int)(j % g.I);
    const int mcu0 = iv * g.R, nm = min(g.R, g.mcus - mcu0), nb = nm * g.bpm;    // nb <= JPEG_MAX_BLOCKS: R <= EG3D_JPEG_MAX_RESTART, bpm <= 6
    const int16_t* c0 = coef + ((int64_t)n * g.nblk + (int64_t)mcu0 * g.bpm) * 64;
    const int nwords = (nb * JPEG_BLOCK_BITS + 31) / 32 + 4;                      // <= JPEG_LDS_WORDS
    for (int w = lane; w < nwords; w += 64) s_bits[w] = 0u;
    if (lane < 32) s_dc[lane >> 4][lane & 15] = jpeg_dc_code[lane >> 4][lane & 15];
    for (int w = lane; w < 512; w += 64) s_ac[w >> 8][w & 255] = jpeg_ac_code[w >> 8][w & 255];
    __syncthreads();
    uint32_t bitpos = 0;
    int cnext = nb > 0 ? (int)c0[lane] : 0;
    for (int blk = 0; blk < nb; ++blk) {
        const int c = cnext;
        if (blk + 1 < nb) cnext = (int)c0[(int64_t)(blk + 1) * 64 + lane];
        const int k = blk % g.bpm;
        int t, back;                                                               // Huffman table; distance to the previous block of this component
        if (g.bpm == 6) { t = k >= 4; back = k == 0 ? 3 : (k < 4 ? 1 : 6); }
        else { t = k != 0; back = g.bpm; }
        const int pred = blk >= back ? (int)c0[(int64_t)(blk - back) * 64] : 0;   // DC prediction restarts with the interval
        const unsigned long long nzmask = __ballot(lane > 0 && c != 0);
        unsigned long long pat = 0;
        int len = 0;
        if (lane == 0) {
            const int diff = c - pred, s = jpeg_bitlen(abs(diff));
            const uint32_t code = s_dc[t][s];
            pat = ((unsigned long long)(code & 0xffffu) << s) | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << s) - 1));
            len = (int)(code >> 16) + s;
        } else if (c != 0) {
            const unsigned long long below = nzmask & ((1ull << lane) - 1ull);
            const int prev = below ? 63 - __clzll((long long)below) : 0;
            const int run = lane - 1 - prev, s = jpeg_bitlen(abs(c));
            const uint32_t zrl = s_ac[t][0xF0], code = s_ac[t][((run & 15) << 4) | s];
            for (int z = 0; z < (run >> 4); ++z) {                               // at most 3: 33 + 16 + 10 bits fit the pattern
                pat = (pat << (zrl >> 16)) | (zrl & 0xffffu);
                len += (int)(zrl >> 16);
            }
            pat = (pat << (code >> 16)) | (code & 0xffffu);
            pat = (pat << s) | (uint32_t)((c < 0 ? c - 1 : c) & ((1 << s) - 1));
            len += (int)(code >> 16) + s;
        } else if (lane == 63) {                                                   // the last coefficient is zero: end of block
            const uint32_t eob = s_ac[t][0];
            pat = eob & 0xffffu;
            len = (int)(eob >> 16);
        }
        int incl = len;                                                            // wave-inclusive scan of the bit counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const int total = __shfl(incl, 63);
        if (len > 0) {
            const uint32_t pos = bitpos + (uint32_t)(incl - len), sh = pos & 31u, w = pos >> 5;
            const unsigned long long left = pat << (64 - len);                    // MSB-first: the pattern left-aligned, then moved right by sh
            const unsigned long long hi = left >> sh;
            const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi, w2 = sh ? (uint32_t)((left << (64 - sh)) >> 32) : 0u;
            if (w0) atomicOr(&s_bits[w], w0);
            if (w1) atomicOr(&s_bits[w + 1], w1);
            if (w2) atomicOr(&s_bits[w + 2], w2);
        }
        bitpos += (uint32_t)total;
    }
    __syncthreads();
    const uint32_t nbytes = (bitpos + 7u) >> 3, fill = nbytes * 8u - bitpos;
    if (lane == 0 && fill) s_bits[bitpos >> 5] |= ((1u << fill) - 1u) << (32u - (bitpos & 31u) - fill);     // 1-bits up to the byte boundary
    __syncthreads();
    uint8_t* slot = slots + j * g.stride;                                          // stride >= 2 * ceil(nb * JPEG_BLOCK_BITS / 8) + 2
    uint32_t nff = 0;
    for (uint32_t base = 0; base < nbytes; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < nbytes;
        const uint32_t byte = valid ? (s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 0xffu : 0u;
        const bool ff = valid && byte == 0xffu;
        const unsigned long long m = __ballot(ff);
        const uint32_t o = i + nff + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid) {
            slot[o] = (uint8_t)byte;
            if (ff) slot[o + 1] = 0;
        }
        nff += (uint32_t)__popcll(m);
    }
    if (lane == 0) {
        const uint32_t end = nbytes + nff;
        slot[end] = 0xff;
        slot[end + 1] = iv == g.I - 1 ? (uint8_t)0xD9 : (uint8_t)(0xD0 + (iv & 7));            // EOI after the last interval, RSTm between intervals
        lens[j] = (int32_t)(end + 2);
    }
}

// one workgroup: item j = slot j, preceded by the header when it opens a frame.  dst[j] = where slot j goes; offsets[n] = where frame n starts
__global__ void __launch_bounds__(JPEG_SCAN_THREADS) jpeg_offsets_kernel(const int32_t* __restrict__ lens, JpegGeom g, int64_t* __restrict__ dst,
                                                                         int64_t* __restrict__ offsets) {
    __shared__ long long sh[2][JPEG_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t M = (int64_t)g.N * g.I;
    const int64_t per = (M + JPEG_SCAN_THREADS - 1) / JPEG_SCAN_THREADS;
    const int64_t lo = min(M, t * per), hi = min(M, lo + per);
    long long s = 0;
    for (int64_t j = lo; j < hi; ++j) s += lens[j] + (j % g.I == 0 ? g.hdr : 0);
    int cur = 0;
    sh[cur][t] = s;
    __syncthreads();
    for (int o = 1; o < JPEG_SCAN_THREADS; o <<= 1) {
        sh[cur ^ 1][t] = sh[cur][t] + (t >= o ? sh[cur][t - o] : 0ll);
        __syncthreads();
        cur ^= 1;
    }
    long long run = sh[cur][t] - s;
    for (int64_t j = lo; j < hi; ++j) {
        if (j % g.I == 0) {
            offsets[j / g.I] = run;
            run += g.hdr;
        }
        dst[j] = run;
        run += lens[j];
    }
    if (t == JPEG_SCAN_THREADS - 1) offsets[g.N] = sh[cur][t];
}

__global__ void __launch_bounds__(256) jpeg_pack_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens, const int64_t* __restrict__ dst,
                                                        const uint8_t* __restrict__ header, JpegGeom g, uint8_t* __restrict__ out, int64_t cap) {
    const int64_t j = blockIdx.x;
    const int64_t d = dst[j];
    const int32_t len = lens[j];
    const uint8_t* slot = slots + j * g.stride;
    if (j % g.I == 0)
        for (int i = threadIdx.x; i < g.hdr; i += 256)
            if (d - g.hdr + i < cap) out[d - g.hdr + i] = header[i];
    for (int i = threadIdx.x; i < len; i += 256)
        if (d + i < cap) out[d + i] = slot[i];
}

int64_t jpeg_align(int64_t b) { return (b + JPEG_ALIGN - 1) / JPEG_ALIGN * JPEG_ALIGN; }

struct JpegLayout {
    int64_t coef, slots, lens, dst, total;                                        // byte offsets into the workspace
};

int jpeg_geom(const eg3d_jpeg_params* p, JpegGeom& g, JpegLayout& l) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (p->N < 1 || (p->C != 1 && p->C != 3) || p->H < 1 || p->W < 1 || p->H > 65535 || p->W > 65535) return EG3D_ERR_INVALID;
    if (p->dtype != EG3D_JPEG_F32 && p->dtype != EG3D_JPEG_U8) return EG3D_ERR_INVALID;
    if (p->subsampling != EG3D_JPEG_444 && p->subsampling != EG3D_JPEG_420) return EG3D_ERR_INVALID;
    if (p->quality < 1 || p->quality > 100 || p->restart_interval < 0 || p->restart_interval > EG3D_JPEG_MAX_RESTART) return EG3D_ERR_INVALID;
    g.N = p->N; g.C = p->C; g.H = p->H; g.W = p->W; g.dtype = p->dtype;
    g.s420 = (p->C == 3 && p->subsampling == EG3D_JPEG_420) ? 1 : 0;
    const int mcu = g.s420 ? 16 : 8;
    g.mx = (p->W + mcu - 1) / mcu;
    const int64_t mcus = (int64_t)g.mx * ((p->H + mcu - 1) / mcu);
    g.bpm = p->C == 1 ? 1 : (g.s420 ? 6 : 3);
    g.R = p->restart_interval > 0 ? p->restart_interval : (g.mx < EG3D_JPEG_MAX_RESTART ? g.mx : EG3D_JPEG_MAX_RESTART);
    const int64_t I = (mcus + g.R - 1) / g.R;
    if (mcus * g.bpm * (int64_t)p->N * 64 > INT32_MAX || I * p->N > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.mcus = (int32_t)mcus;
    g.nblk = (int32_t)(mcus * g.bpm);
    g.I = (int32_t)I;
    g.qscale = p->quality < 50 ? 5000 / p->quality : 200 - 2 * p->quality;
    g.hdr = p->header_bytes;
    g.stride = jpeg_align(2 * (((int64_t)g.R * g.bpm * JPEG_BLOCK_BITS + 7) / 8) + 2);   // worst-case bits, every byte stuffed, the marker
    const int64_t M = I * p->N;
    l.coef = 0;
    l.slots = jpeg_align((int64_t)p->N * g.nblk * 64 * (int64_t)sizeof(int16_t));
    l.lens = l.slots + jpeg_align(M * g.stride);
    l.dst = l.lens + jpeg_align(M * (int64_t)sizeof(int32_t));
    l.total = l.dst + jpeg_align(M * (int64_t)sizeof(int64_t));
    return EG3D_OK;
}

int jpeg_check(const eg3d_jpeg_params* p, JpegGeom& g, JpegLayout& l) {
    const int s = jpeg_geom(p, g, l);
    if (s != EG3D_OK) return s;
    if (p->img == nullptr || p->header == nullptr || p->header_bytes < 1 || p->workspace == nullptr || p->offsets == nullptr ||
        p->workspace_bytes < l.total || (reinterpret_cast<uintptr_t>(p->workspace) & (JPEG_ALIGN - 1)))
        return EG3D_ERR_INVALID;
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_jpeg_query_workspace(const eg3d_jpeg_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    JpegGeom g;
    JpegLayout l;
    const int s = jpeg_geom(p, g, l);
    if (s != EG3D_OK) return s;
    *workspace_bytes = l.total;
    return EG3D_OK;
}

extern "C" int eg3d_jpeg_encode(const eg3d_jpeg_params* p, void* stream) {
    JpegGeom g;
    JpegLayout l;
    const int s = jpeg_check(p, g, l);
    if (s != EG3D_OK) return s;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(p->workspace);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
    uint8_t* slots = reinterpret_cast<uint8_t*>(ws + l.slots);
    int32_t* lens = reinterpret_cast<int32_t*>(ws + l.lens);
    int64_t* dst = reinterpret_cast<int64_t*>(ws + l.dst);
    const int64_t nblocks = (int64_t)g.N * g.nblk, M = (int64_t)g.N * g.I;
    hipLaunchKernelGGL(jpeg_dct_kernel, dim3((unsigned)((nblocks + 3) / 4)), dim3(256), 0, st, p->img, g, coef);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)M), dim3(64), 0, st, coef, g, slots, lens);
    EG3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(JPEG_SCAN_THREADS), 0, st, lens, g, dst, p->offsets);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}

extern "C" int eg3d_jpeg_pack(const eg3d_jpeg_params* p, void* stream) {
    JpegGeom g;
    JpegLayout l;
    const int s = jpeg_check(p, g, l);
    if (s != EG3D_OK) return s;
    if (p->out_capacity < 0 || (p->out_capacity > 0 && p->out == nullptr)) return EG3D_ERR_INVALID;
    if (p->out_capacity == 0) return EG3D_OK;
    hipStream_t st = (hipStream_t)stream;
    const char* ws = reinterpret_cast<const char*>(p->workspace);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)((int64_t)g.N * g.I)), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(ws + l.slots),
                       reinterpret_cast<const int32_t*>(ws + l.lens), reinterpret_cast<const int64_t*>(ws + l.dst), p->header, g, p->out, p->out_capacity);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
