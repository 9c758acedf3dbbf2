// Batched PNG encoder: adaptive row filters and a run-length deflate (include/eg3d_hip.h "PNG encoder"; the lossless half of media export).
//
// Five launches per batch of N images, integer arithmetic only:
//   png_filter_kernel   one workgroup per row: raw rows y and y - 1 into LDS (dword loads), the five filters' sums of |int8|, a workgroup
//                       reduction picks the type, the filtered row goes into the image's stream in dwords           -> [type][W * C bytes] rows
//   png_deflate_kernel  one workgroup per block of block_bytes: the block into LDS, run starts by neighbour compare, every thread walks its
//                       chunk (the run reaching in from the left / out to the right comes from two workgroup scans), histogram by integer LDS
//                       atomics, both Huffman codes (rank sort, two-queue merge by one thread, depths per leaf, miniz's Kraft fix-up,
//                       canonical codes), bit offsets by scan, tokens ORed into an LDS window that is flushed to the block's slot in dwords;
//                       the block's Adler-32 partial sums                                                           -> slot bytes, slot length, (a, b)
//   png_offsets_kernel  one workgroup: exclusive scan of the slot lengths (+ 2 header, + 4 trailer bytes per image)   -> offsets[N + 1], slot destinations
//   png_adler_kernel    one workgroup per image: the blocks' partials combined by the concatenation rule              -> Adler-32 per image
//   (the host reads offsets[N] and allocates)
//   png_pack_kernel     one workgroup per block: 78 01 (first block), the slot, the Adler-32 (last block) into the output, interior in dwords
// No atomics on global memory, no floating point: the output is a function of the input (bit-identical between runs and builds).
#include "common.h"

namespace {

constexpr int PNG_FILTER_THREADS = 256;
constexpr int PNG_THREADS = 1024;                                              // deflate workgroup
constexpr int PNG_WINDOW_WORDS = 4096;                                         // LDS bit window: 16 KiB of output per pass over the tokens
constexpr uint32_t PNG_WINDOW_BITS = PNG_WINDOW_WORDS * 32u;
constexpr int PNG_LIT = 286, PNG_LITPAD = 288, PNG_CL = 19, PNG_CLPAD = 32;
constexpr int PNG_HEADER_BITS = 17 + 19 * 3 + 287 * 7;                         // BFINAL BTYPE HLIT HDIST HCLEN; 19 lengths; 286 + 1 lengths of at most 7 bits
constexpr uint32_t PNG_ADLER = 65521u;
constexpr int64_t PNG_ALIGN = 16;
constexpr int PNG_SCAN_THREADS = 1024;
constexpr int PNG_ADLER_THREADS = 256;

struct PngGeom {
    int32_t N, C, H, W, filter, bb;
    int32_t rowb;                        // W * C
    int32_t L;                           // H * (1 + rowb): bytes of an image's filtered stream
    int32_t I;                           // blocks per image
    int64_t fstride;                     // bytes between the streams of two images (16-aligned, >= L + 16: the block loads read whole dwords)
    int64_t sstride;                     // slot bytes per block
};

__host__ __device__ inline int64_t png_align(int64_t b) { return (b + PNG_ALIGN - 1) / PNG_ALIGN * PNG_ALIGN; }

// ---- row filters ----------------------------------------------------------------------------------------------------------------------------
// bytes [g0, g0 + n) of `src` into lds so that byte i lands at lds[(addr & 3) + i]: aligned dwords where the dword lies inside [0, total)
__device__ __forceinline__ void png_load_bytes(const uint8_t* __restrict__ src, int64_t g0, int n, int64_t total, uint8_t* lds, int threads) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) + (uintptr_t)g0;
    const int mis = (int)(a & 3);
    const int words = (mis + n + 3) >> 2;
    const int64_t w0 = g0 - mis;                                               // offset of the first dword from src
    uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
    for (int k = threadIdx.x; k < words; k += threads) {
        const int64_t o = w0 + 4 * (int64_t)k;
        uint32_t v;
        if (o >= 0 && o + 4 <= total) {
            v = *reinterpret_cast<const uint32_t*>(src + o);
        } else {
            v = 0u;
            for (int b = 0; b < 4; ++b)
                if (o + b >= 0 && o + b < total) v |= (uint32_t)src[o + b] << (8 * b);
        }
        l32[k] = v;
    }
}

__device__ __forceinline__ int png_abs8(int v) { return v < 128 ? v : 256 - v; }

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_filtered(int t, int x, int a, int b, int c) {
    int q = 0;
    if (t == 1) q = a;
    else if (t == 2) q = b;
    else if (t == 3) q = (a + b) >> 1;
    else if (t == 4) q = png_paeth(a, b, c);
    return (x - q) & 255;
}

__global__ void __launch_bounds__(PNG_FILTER_THREADS) png_filter_kernel(const uint8_t* __restrict__ img, PngGeom g, uint8_t* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    __shared__ int s_sum[5][PNG_FILTER_THREADS / 64];
    __shared__ int s_type;
    const int rowb = g.rowb, bpp = g.C;
    const int half = (int)png_align(rowb + 8);
    uint8_t* s_cur = png_lds;
    uint8_t* s_up = png_lds + half;
    const int64_t row = blockIdx.x;
    const int n = (int)(row / g.H), y = (int)(row % g.H);
    const int64_t total = (int64_t)g.N * g.H * rowb;
    const int64_t g0 = ((int64_t)n * g.H + y) * rowb;
    png_load_bytes(img, g0, rowb, total, s_cur, PNG_FILTER_THREADS);
    if (y > 0) png_load_bytes(img, g0 - rowb, rowb, total, s_up, PNG_FILTER_THREADS);
    const int cb = (int)((reinterpret_cast<uintptr_t>(img) + (uintptr_t)g0) & 3);
    const int ub = (int)((reinterpret_cast<uintptr_t>(img) + (uintptr_t)(g0 - rowb)) & 3);
    __syncthreads();
    const bool has_up = y > 0;
    int type = g.filter;
    if (type < 0) {
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
        for (int i = threadIdx.x; i < rowb; i += PNG_FILTER_THREADS) {
            const int x = s_cur[cb + i];
            const int a = i >= bpp ? (int)s_cur[cb + i - bpp] : 0;
            const int b = has_up ? (int)s_up[ub + i] : 0;
            const int c = (has_up && i >= bpp) ? (int)s_up[ub + i - bpp] : 0;
            s0 += png_abs8(x);
            s1 += png_abs8((x - a) & 255);
            s2 += png_abs8((x - b) & 255);
            s3 += png_abs8((x - ((a + b) >> 1)) & 255);
            s4 += png_abs8((x - png_paeth(a, b, c)) & 255);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_down(s0, o);
            s1 += __shfl_down(s1, o);
            s2 += __shfl_down(s2, o);
            s3 += __shfl_down(s3, o);
            s4 += __shfl_down(s4, o);
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
            s_sum[0][wave] = s0; s_sum[1][wave] = s1; s_sum[2][wave] = s2; s_sum[3][wave] = s3; s_sum[4][wave] = s4;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int best = 0, bestv = 0;
            for (int t = 0; t < 5; ++t) {
                int v = 0;
                for (int w = 0; w < PNG_FILTER_THREADS / 64; ++w) v += s_sum[t][w];
                if (t == 0 || v < bestv) { best = t; bestv = v; }                 // strict: a tie keeps the lower type
            }
            s_type = best;
        }
        __syncthreads();
        type = s_type;
    }
    // the row's record [type][rowb bytes] occupies bytes [o, o + 1 + rowb) of the image's stream; the stream base is 16-byte aligned
    const int64_t o = (int64_t)y * (1 + rowb);
    uint8_t* dst = filt + (int64_t)n * g.fstride;
    const int64_t wlo = o >> 2, whi = (o + 1 + rowb + 3) >> 2;
    for (int64_t k = wlo + threadIdx.x; k < whi; k += PNG_FILTER_THREADS) {
        uint32_t v = 0u;
        int inside = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t j = 4 * k + b - o;                                    // byte of the record
            if (j < 0 || j > rowb) continue;
            int val = type;
            if (j > 0) {
                const int i = (int)j - 1;
                const int x = s_cur[cb + i];
                const int a = i >= bpp ? (int)s_cur[cb + i - bpp] : 0;
                const int bb = has_up ? (int)s_up[ub + i] : 0;
                const int c = (has_up && i >= bpp) ? (int)s_up[ub + i - bpp] : 0;
                val = png_filtered(type, x, a, bb, c);
            }
            v |= (uint32_t)val << (8 * b);
            inside |= 1 << b;
        }
        if (inside == 15) {
            *reinterpret_cast<uint32_t*>(dst + 4 * k) = v;
        } else {                                                               // the dword is shared with the neighbouring row's record
            for (int b = 0; b < 4; ++b)
                if (inside & (1 << b)) dst[4 * k + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

// ---- deflate --------------------------------------------------------------------------------------------------------------------------------
struct PngMax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct PngMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct PngAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };

// inclusive scan over the workgroup in the order of idx (a permutation of 0 .. PNG_THREADS - 1); buf: 2 * PNG_THREADS words
template <typename Op>
__device__ uint32_t png_scan(uint32_t v, int idx, uint32_t* buf, Op op) {
    int cur = 0;
    buf[idx] = v;
    __syncthreads();
    for (int o = 1; o < PNG_THREADS; o <<= 1) {
        uint32_t x = buf[cur * PNG_THREADS + idx];
        if (idx >= o) x = op(buf[cur * PNG_THREADS + idx - o], x);
        buf[(cur ^ 1) * PNG_THREADS + idx] = x;
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t r = buf[cur * PNG_THREADS + idx];
    __syncthreads();
    return r;
}

// symbol of a match length 3..258 -> (symbol, extra bits, extra value)
__device__ __forceinline__ void png_length_symbol(int length, int& sym, int& ebits, int& eval) {
    if (length == 258) { sym = 285; ebits = 0; eval = 0; return; }
    const int l = length - 3;
    if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
    const int e = 29 - __clz(l);                                               // floor(log2 l) - 2
    sym = 261 + 4 * e + ((l >> e) & 3);
    ebits = e;
    eval = l & ((1 << e) - 1);
}

// The tokens of positions [lo, hi) of the block s[0 .. len): f(symbol, length) with length = 0 for a literal.  prev = the last run start
// before lo (used when lo is inside a run), next = the first run start at or after hi (len when there is none).
template <typename F>
__device__ __forceinline__ void png_walk(const uint8_t* s, int lo, int hi, int prev, int next, F&& f) {
    if (lo >= hi) return;
    int i = lo;
    int p = (i == 0 || s[i] != s[i - 1]) ? i : prev;
    while (i < hi) {
        const int v = s[i];
        int e = i + 1;
        while (e < hi && s[e] == v) ++e;
        const int end = e == hi ? next : e;                                   // where the run really ends
        const int m = end - p - 1, full = (m / 258) * 258, q = m - full;
        for (int pos = i; pos < e; ++pos) {
            const int k = pos - p;
            if (k == 0) {
                f(v, 0);
            } else {
                const int j = k - 1;
                if (j < full) {
                    if (j % 258 == 0) f(285, 258);
                } else if (q >= 3) {
                    if (j == full) f(-1, q);
                } else {
                    f(v, 0);
                }
            }
        }
        i = e;
        p = e;
    }
}

// Length-limited canonical Huffman code over counts[0 .. nsym) (at least two used symbols), by the whole workgroup:
//   sorted by (count, symbol) with a rank sort; two-queue merge by thread 0, a tie goes to the leaf; depth per leaf; number of codes per depth
//   folded into `limit`, miniz's Kraft fix-up; lengths handed out from the far end of the order; canonical codes (RFC 1951 3.2.2).
// out[s] = (length << 16) | the code's bits reversed (ready for an LSB-first stream); 0 for an unused symbol.
__device__ void png_build_code(const uint32_t* counts, int nsym, int limit, uint32_t* out, uint32_t* s_sorted, uint32_t* s_w, uint32_t* s_parent,
                               uint32_t* s_num, uint32_t* s_next) {
    const int t = threadIdx.x;
    const uint32_t c = t < nsym ? counts[t] : 0u;
    const int n = __syncthreads_count(c > 0u);
    if (t < 64) s_num[t] = 0u;
    if (t < nsym) out[t] = 0u;
    if (c > 0u) {
        int rank = 0;
        for (int s = 0; s < nsym; ++s) {
            const uint32_t cs = counts[s];
            rank += (cs > 0u && (cs < c || (cs == c && s < t))) ? 1 : 0;
        }
        s_sorted[rank] = (uint32_t)t;
        s_w[rank] = c;
    }
    __syncthreads();
    if (t == 0) {
        int leaf = 0, inode = n;
        for (int nxt = n; nxt < 2 * n - 1; ++nxt) {
            uint32_t w = 0u;
            for (int k = 0; k < 2; ++k) {
                int pick;
                if (leaf < n && (inode >= nxt || s_w[leaf] <= s_w[inode])) pick = leaf++;
                else pick = inode++;
                w += s_w[pick];
                s_parent[pick] = (uint32_t)nxt;
            }
            s_w[nxt] = w;
        }
    }
    __syncthreads();
    if (t < n) {
        int j = t, d = 0;
        while (j != 2 * n - 2 && d < 2 * PNG_LITPAD) { j = (int)s_parent[j]; ++d; }   // (every parent has a higher index: at most 2n - 2 steps)
        atomicAdd(&s_num[min(d, limit)], 1u);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0u;
        for (int i = limit; i > 0; --i) total += s_num[i] << (limit - i);
        if (n < 2) { s_num[1] = (uint32_t)n; total = 1u << limit; }           // (not reached by the encoder: both alphabets use two symbols or more)
        while (total > (1u << limit)) {                                        // (a Huffman tree's Kraft sum is 1 and folding only raises it)
            s_num[limit]--;
            for (int i = limit - 1; i > 0; --i)
                if (s_num[i]) { s_num[i]--; s_num[i + 1] += 2u; break; }
            total--;
        }
        uint32_t code = 0u, cum = 0u;
        s_num[0] = 0u;
        for (int bits = 1; bits <= limit; ++bits) {
            code = (code + s_num[bits - 1]) << 1;
            s_next[bits] = code;
        }
        for (int bits = 1; bits <= limit; ++bits) {                             // s_num[32 + bits] = codes of length <= bits
            cum += s_num[bits];
            s_num[32 + bits] = cum;
        }
    }
    __syncthreads();
    if (t < n) {
        const uint32_t k = (uint32_t)(n - 1 - t);                               // position from the most frequent symbol
        int len = 1;
        while (s_num[32 + len] <= k) ++len;
        out[s_sorted[t]] = (uint32_t)len << 16;
    }
    __syncthreads();
    if (t < nsym) {
        const uint32_t len = out[t] >> 16;
        if (len) {
            uint32_t before = 0u;
            for (int s = 0; s < t; ++s) before += (out[s] >> 16) == len ? 1u : 0u;
            const uint32_t code = s_next[len] + before;
            out[t] = (len << 16) | (__brev(code) >> (32u - len));
        }
    }
    __syncthreads();
}

// OR `len` (<= 32) bits of pat at bit `pos` of the block's output into the window that starts at bit w0
__device__ __forceinline__ void png_put(uint32_t* win, uint32_t w0, uint32_t pos, uint32_t pat, uint32_t len) {
    if (pos + len <= w0 || pos >= w0 + PNG_WINDOW_BITS) return;
    unsigned long long v = pat;
    uint32_t rel;
    if (pos < w0) { v >>= (w0 - pos); rel = 0u; }
    else rel = pos - w0;
    v <<= (rel & 31u);
    const uint32_t w = rel >> 5, lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo) atomicOr(&win[w], lo);
    if (hi && w + 1 < (uint32_t)PNG_WINDOW_WORDS) atomicOr(&win[w + 1], hi);
}

struct PngLds {                                                                // offsets into the dynamic LDS, every one a multiple of 16
    int in, win, cnt, lcode, clcnt, clcode, sorted, w, parent, num, next, scan, misc, total;
};

__host__ __device__ inline PngLds png_lds_layout(int bb) {
    PngLds l;
    int o = 0;
    l.in = o;      o += (int)png_align(bb + 8);
    l.win = o;     o += PNG_WINDOW_WORDS * 4;
    l.cnt = o;     o += PNG_LITPAD * 4;
    l.lcode = o;   o += PNG_LITPAD * 4;
    l.clcnt = o;   o += PNG_CLPAD * 4;
    l.clcode = o;  o += PNG_CLPAD * 4;
    l.sorted = o;  o += PNG_LITPAD * 4;
    l.w = o;       o += 2 * PNG_LITPAD * 4;
    l.parent = o;  o += 2 * PNG_LITPAD * 4;
    l.num = o;     o += 64 * 4;
    l.next = o;    o += 16 * 4;
    l.scan = o;    o += 2 * PNG_THREADS * 4;
    l.misc = o;    o += 16 * 4;
    l.total = o;
    return l;
}

enum { PNG_M_MATCH = 0, PNG_M_SA = 1, PNG_M_SB = 2, PNG_M_NLIT = 3, PNG_M_HDR = 4 };

__global__ void __launch_bounds__(PNG_THREADS) png_deflate_kernel(const uint8_t* __restrict__ filt, PngGeom g, uint8_t* __restrict__ slots,
                                                                  int32_t* __restrict__ lens, uint32_t* __restrict__ adl) {
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    const PngLds l = png_lds_layout(g.bb);
    uint8_t* s_in = png_lds + l.in;
    uint32_t* s_win = reinterpret_cast<uint32_t*>(png_lds + l.win);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(png_lds + l.cnt);
    uint32_t* s_lcode = reinterpret_cast<uint32_t*>(png_lds + l.lcode);
    uint32_t* s_clcnt = reinterpret_cast<uint32_t*>(png_lds + l.clcnt);
    uint32_t* s_clcode = reinterpret_cast<uint32_t*>(png_lds + l.clcode);
    uint32_t* s_sorted = reinterpret_cast<uint32_t*>(png_lds + l.sorted);
    uint32_t* s_w = reinterpret_cast<uint32_t*>(png_lds + l.w);
    uint32_t* s_parent = reinterpret_cast<uint32_t*>(png_lds + l.parent);
    uint32_t* s_num = reinterpret_cast<uint32_t*>(png_lds + l.num);
    uint32_t* s_next = reinterpret_cast<uint32_t*>(png_lds + l.next);
    uint32_t* s_scan = reinterpret_cast<uint32_t*>(png_lds + l.scan);
    uint32_t* s_misc = reinterpret_cast<uint32_t*>(png_lds + l.misc);
    const int t = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int n = (int)(j / g.I), b = (int)(j % g.I);
    const int start = b * g.bb;                                                  // < L <= INT32_MAX
    const int len = min(g.bb, g.L - start);
    const bool final = b == g.I - 1;

    // the block into LDS: the stream's base is 16-byte aligned and fstride >= L + 16, so whole dwords are inside the workspace
    const int mis = start & 3;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(filt + (int64_t)n * g.fstride + (start - mis));
        uint32_t* d32 = reinterpret_cast<uint32_t*>(s_in);
        const int words = (mis + len + 3) >> 2;
        for (int k = t; k < words; k += PNG_THREADS) d32[k] = src[k];
    }
    for (int k = t; k < PNG_LITPAD; k += PNG_THREADS) s_cnt[k] = 0u;
    if (t < PNG_CLPAD) s_clcnt[t] = 0u;
    if (t < 16) s_misc[t] = 0u;
    __syncthreads();
    const uint8_t* s = s_in + mis;

    // run starts: the last one before my chunk, the first one at or after its end
    const int chunk = (len + PNG_THREADS - 1) / PNG_THREADS;
    const int lo = min(len, t * chunk), hi = min(len, lo + chunk);
    uint32_t last = 0u, first = 0xffffffffu;                                    // last: position + 1 (0 = none)
    uint32_t sa = 0u, sb = 0u;
    for (int i = lo; i < hi; ++i) {
        const uint32_t d = s[i];
        if (i == 0 || s[i - 1] != d) {
            last = (uint32_t)i + 1u;
            if (first == 0xffffffffu) first = (uint32_t)i;
        }
        sa += d;
        sb += (uint32_t)(len - i) * d;                                          // <= 64 * 65536 * 255
    }
    const uint32_t incl_last = png_scan(last, t, s_scan, PngMax());
    // exclusive forms through LDS: prev[t] = inclusive max of threads < t; next[t] = inclusive min of threads > t
    s_scan[t] = incl_last;
    __syncthreads();
    const int prev = t > 0 ? (int)s_scan[t - 1] - 1 : -1;
    __syncthreads();
    const uint32_t incl_first = png_scan(first, PNG_THREADS - 1 - t, s_scan, PngMin());
    s_scan[t] = incl_first;
    __syncthreads();
    const uint32_t nf = t + 1 < PNG_THREADS ? s_scan[t + 1] : 0xffffffffu;
    const int next = nf == 0xffffffffu ? len : (int)nf;
    __syncthreads();

    // histogram: equal symbols in a row are counted in a register first
    {
        int csym = -1;
        uint32_t ccnt = 0u;
        bool match = false;
        png_walk(s, lo, hi, prev, next, [&](int sym, int length) {
            if (length) {
                match = true;
                if (sym < 0) { int eb, ev; png_length_symbol(length, sym, eb, ev); }
            }
            if (sym != csym) {
                if (ccnt) atomicAdd(&s_cnt[csym], ccnt);
                csym = sym;
                ccnt = 0u;
            }
            ++ccnt;
        });
        if (ccnt) atomicAdd(&s_cnt[csym], ccnt);
        if (match) s_misc[PNG_M_MATCH] = 1u;
        if (t == 0) s_cnt[256] = 1u;
        atomicAdd(&s_misc[PNG_M_SA], sa % PNG_ADLER);
        atomicAdd(&s_misc[PNG_M_SB], sb % PNG_ADLER);
    }
    __syncthreads();
    png_build_code(s_cnt, PNG_LIT, 15, s_lcode, s_sorted, s_w, s_parent, s_num, s_next);

    // the code-length alphabet over the nlit literal/length lengths and the one distance length
    {
        const uint32_t used = (t < PNG_LIT && s_cnt[t] > 0u) ? (uint32_t)t + 1u : 0u;
        if (used) atomicMax(&s_misc[PNG_M_NLIT], used);
    }
    __syncthreads();
    const int nlit = (int)s_misc[PNG_M_NLIT];                                    // >= 257
    const uint32_t dist_len = s_misc[PNG_M_MATCH];
    if (t < nlit) atomicAdd(&s_clcnt[s_lcode[t] >> 16], 1u);
    if (t == 0) atomicAdd(&s_clcnt[dist_len], 1u);
    __syncthreads();
    png_build_code(s_clcnt, PNG_CL, 7, s_clcode, s_sorted, s_w, s_parent, s_num, s_next);

    // bits: the header (thread 0 counts it), my tokens, end-of-block and the flush (the last thread)
    uint32_t mybits = 0u;
    png_walk(s, lo, hi, prev, next, [&](int sym, int length) {
        if (length) {
            int eb = 0, ev = 0;
            if (sym < 0) png_length_symbol(length, sym, eb, ev);
            mybits += (s_lcode[sym] >> 16) + (uint32_t)eb + 1u;
        } else {
            mybits += s_lcode[sym] >> 16;
        }
    });
    if (t <= nlit) atomicAdd(&s_misc[PNG_M_HDR], s_clcode[t < nlit ? (s_lcode[t] >> 16) : dist_len] >> 16);
    const uint32_t incl = png_scan(mybits, t, s_scan, PngAdd());
    s_scan[t] = incl;
    __syncthreads();
    const uint32_t tok_bits = s_scan[PNG_THREADS - 1];
    const uint32_t hdr_bits = 17u + 57u + s_misc[PNG_M_HDR];
    const uint32_t mystart = hdr_bits + incl - mybits;
    const uint32_t eob_pos = hdr_bits + tok_bits;
    const uint32_t eob_end = eob_pos + (s_lcode[256] >> 16);
    const uint32_t nbytes = final ? (eob_end + 7u) >> 3 : ((eob_end + 3u + 7u) >> 3) + 4u;
    __syncthreads();

    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + j * g.sstride);        // sstride: 16-aligned, >= nbytes rounded up to dwords
    const uint32_t nwords = (nbytes + 3u) >> 2;
    for (uint32_t w0 = 0u, word0 = 0u; word0 < nwords; w0 += PNG_WINDOW_BITS, word0 += PNG_WINDOW_WORDS) {
        for (int k = t; k < PNG_WINDOW_WORDS; k += PNG_THREADS) s_win[k] = 0u;
        __syncthreads();
        if (t == 0 && w0 == 0u) {                                               // the header lies in the first window: PNG_HEADER_BITS < PNG_WINDOW_BITS
            uint32_t pos = 0u;
            png_put(s_win, 0u, pos, (final ? 1u : 0u) | (2u << 1), 3u); pos += 3u;
            png_put(s_win, 0u, pos, (uint32_t)(nlit - 257), 5u); pos += 5u;
            png_put(s_win, 0u, pos, 0u, 5u); pos += 5u;
            png_put(s_win, 0u, pos, 15u, 4u); pos += 4u;
            const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int k = 0; k < 19; ++k) { png_put(s_win, 0u, pos, s_clcode[order[k]] >> 16, 3u); pos += 3u; }
            for (int k = 0; k <= nlit; ++k) {
                const uint32_t c = s_clcode[k < nlit ? (s_lcode[k] >> 16) : dist_len];
                png_put(s_win, 0u, pos, c & 0xffffu, c >> 16);
                pos += c >> 16;
            }
        }
        if (mybits && mystart < w0 + PNG_WINDOW_BITS && mystart + mybits > w0) {
            uint32_t pos = mystart;
            png_walk(s, lo, hi, prev, next, [&](int sym, int length) {
                uint32_t pat, nb;
                if (length) {
                    int eb = 0, ev = 0;
                    if (sym < 0) png_length_symbol(length, sym, eb, ev);
                    const uint32_t c = s_lcode[sym];
                    pat = (c & 0xffffu) | ((uint32_t)ev << (c >> 16));             // code, extra bits, then the 1-bit distance code 0
                    nb = (c >> 16) + (uint32_t)eb + 1u;
                } else {
                    const uint32_t c = s_lcode[sym];
                    pat = c & 0xffffu;
                    nb = c >> 16;
                }
                png_put(s_win, w0, pos, pat, nb);
                pos += nb;
            });
        }
        if (t == PNG_THREADS - 1) {
            png_put(s_win, w0, eob_pos, s_lcode[256] & 0xffffu, s_lcode[256] >> 16);
            if (!final) png_put(s_win, w0, (nbytes - 2u) * 8u, 0xffffu, 16u);   // 00 00 FF FF of the empty stored block
        }
        __syncthreads();
        const uint32_t cnt = min((uint32_t)PNG_WINDOW_WORDS, nwords - word0);
        for (uint32_t k = t; k < cnt; k += PNG_THREADS) slot[word0 + k] = s_win[k];
        __syncthreads();
    }
    if (t == 0) {
        lens[j] = (int32_t)nbytes;
        adl[2 * j] = s_misc[PNG_M_SA] % PNG_ADLER;
        adl[2 * j + 1] = s_misc[PNG_M_SB] % PNG_ADLER;
    }
}

// one workgroup: item j = block j's slot, preceded by 78 01 when it opens an image and followed by the Adler-32 when it closes one
__global__ void __launch_bounds__(PNG_SCAN_THREADS) png_offsets_kernel(const int32_t* __restrict__ lens, PngGeom g, int64_t* __restrict__ dst,
                                                                       int64_t* __restrict__ offsets) {
    __shared__ long long sh[2][PNG_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t M = (int64_t)g.N * g.I;
    const int64_t per = (M + PNG_SCAN_THREADS - 1) / PNG_SCAN_THREADS;
    const int64_t lo = min(M, t * per), hi = min(M, lo + per);
    long long s = 0;
    for (int64_t j = lo; j < hi; ++j) s += lens[j] + (j % g.I == 0 ? 2 : 0) + (j % g.I == g.I - 1 ? 4 : 0);
    int cur = 0;
    sh[cur][t] = s;
    __syncthreads();
    for (int o = 1; o < PNG_SCAN_THREADS; o <<= 1) {
        sh[cur ^ 1][t] = sh[cur][t] + (t >= o ? sh[cur][t - o] : 0ll);
        __syncthreads();
        cur ^= 1;
    }
    long long run = sh[cur][t] - s;
    for (int64_t j = lo; j < hi; ++j) {
        if (j % g.I == 0) {
            offsets[j / g.I] = run;
            run += 2;
        }
        dst[j] = run;
        run += lens[j] + (j % g.I == g.I - 1 ? 4 : 0);
    }
    if (t == PNG_SCAN_THREADS - 1) offsets[g.N] = sh[cur][t];
}

// (n, a, b) of two byte strings in a row: n = n1 + n2, a = a1 + a2, b = b1 + n2 a1 + b2 (mod 65521; a, b as if Adler's a started from 0)
struct PngAdler { uint32_t n, a, b; };
__device__ __forceinline__ PngAdler png_adler_cat(PngAdler x, PngAdler y) {
    PngAdler r;
    r.n = (uint32_t)(((unsigned long long)x.n + y.n) % PNG_ADLER);
    r.a = (x.a + y.a) % PNG_ADLER;
    r.b = (uint32_t)((x.b + (unsigned long long)y.n * x.a + y.b) % PNG_ADLER);
    return r;
}

__global__ void __launch_bounds__(PNG_ADLER_THREADS) png_adler_kernel(const uint32_t* __restrict__ adl, PngGeom g, uint32_t* __restrict__ adler) {
    __shared__ PngAdler sh[PNG_ADLER_THREADS];
    const int t = threadIdx.x, n = blockIdx.x;
    const int per = (g.I + PNG_ADLER_THREADS - 1) / PNG_ADLER_THREADS;
    const int lo = min(g.I, t * per), hi = min(g.I, lo + per);
    PngAdler acc = {0u, 0u, 0u};
    for (int b = lo; b < hi; ++b) {
        const int64_t j = (int64_t)n * g.I + b;
        const int len = min(g.bb, g.L - b * g.bb);
        const PngAdler x = {(uint32_t)len % PNG_ADLER, adl[2 * j], adl[2 * j + 1]};
        acc = png_adler_cat(acc, x);
    }
    sh[t] = acc;
    __syncthreads();
    if (t == 0) {
        PngAdler all = {0u, 0u, 0u};
        for (int k = 0; k < PNG_ADLER_THREADS; ++k) all = png_adler_cat(all, sh[k]);
        adler[n] = (((all.n + all.b) % PNG_ADLER) << 16) | ((1u + all.a) % PNG_ADLER);   // a starts from 1: + 1 on a, + n on b
    }
}

__global__ void __launch_bounds__(256) png_pack_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens, const int64_t* __restrict__ dst,
                                                       const uint32_t* __restrict__ adler, PngGeom g, uint8_t* __restrict__ out, int64_t cap) {
    const int64_t j = blockIdx.x;
    const int64_t d = dst[j];
    const int len = lens[j];
    const int t = threadIdx.x;
    const uint32_t* slot = reinterpret_cast<const uint32_t*>(slots + j * g.sstride);
    if (j % g.I == 0 && t < 2 && d - 2 + t < cap) out[d - 2 + t] = t == 0 ? (uint8_t)0x78 : (uint8_t)0x01;
    if (j % g.I == g.I - 1 && t < 4 && d + len + t < cap) out[d + len + t] = (uint8_t)(adler[j / g.I] >> (24 - 8 * t));
    // head bytes up to the output's dword boundary, whole dwords (source dwords funnel-shifted), tail bytes
    const int head = min(len, (int)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(out) + (uintptr_t)d) & 3u)) & 3u));
    const int nw = (len - head) >> 2, tail0 = head + 4 * nw;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(slot);
    if (t < head && d + t < cap) out[d + t] = sb[t];
    if (t < len - tail0 && d + tail0 + t < cap) out[d + tail0 + t] = sb[tail0 + t];
    const uint32_t sh = 8u * (uint32_t)head;
    for (int k = t; k < nw; k += 256) {
        const int64_t o = d + head + 4 * (int64_t)k;
        if (o + 4 > cap) {
            for (int b = 0; b < 4; ++b)
                if (o + b < cap) out[o + b] = sb[head + 4 * k + b];
            continue;
        }
        const uint32_t v = sh ? (slot[k] >> sh) | (slot[k + 1] << (32u - sh)) : slot[k];     // slot[k + 1]: inside the slot, sstride has 8 spare bytes
        *reinterpret_cast<uint32_t*>(out + o) = v;
    }
}

struct PngLayout {
    int64_t filt, slots, lens, dst, adl, adler, total;                          // byte offsets into the workspace
};

int png_geom(const eg3d_png_params* p, PngGeom& g, PngLayout& l) {
    if (p == nullptr) return EG3D_ERR_INVALID;
    if (p->N < 1 || (p->C != 1 && p->C != 3) || p->H < 1 || p->W < 1) return EG3D_ERR_INVALID;
    if (p->filter < -1 || p->filter > 4 || p->block_bytes < 64 || p->block_bytes > 65536) return EG3D_ERR_INVALID;
    if (p->stages < 0 || p->stages > 3) return EG3D_ERR_INVALID;
    if (p->H > 16384 || p->W > 16384) return EG3D_ERR_UNSUPPORTED;
    g.N = p->N; g.C = p->C; g.H = p->H; g.W = p->W; g.filter = p->filter; g.bb = p->block_bytes;
    g.rowb = p->W * p->C;
    const int64_t L = (int64_t)p->H * (1 + g.rowb);                              // <= 16384 * 49153 < 2^31
    const int64_t I = (L + g.bb - 1) / g.bb;
    if ((int64_t)p->N * p->H > INT32_MAX || I * p->N > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.L = (int32_t)L;
    g.I = (int32_t)I;
    g.fstride = png_align(L) + PNG_ALIGN;
    // a block of n bytes: header <= PNG_HEADER_BITS; a literal <= 15 bits for 1 byte, a match <= 15 + 5 + 1 bits for >= 3 bytes: <= 15 n bits;
    // end-of-block <= 15 bits; 3 bits of the stored block and up to 7 of padding, its 4 bytes; 8 spare bytes (whole dwords, the packer's funnel)
    g.sstride = png_align((PNG_HEADER_BITS + 15 * (int64_t)g.bb + 15 + 3 + 7) / 8 + 4 + 8);
    const int64_t M = I * p->N;
    l.filt = 0;
    l.slots = l.filt + (int64_t)p->N * g.fstride;
    l.lens = l.slots + M * g.sstride;
    l.dst = l.lens + png_align(M * (int64_t)sizeof(int32_t));
    l.adl = l.dst + png_align(M * (int64_t)sizeof(int64_t));
    l.adler = l.adl + png_align(2 * M * (int64_t)sizeof(uint32_t));
    l.total = l.adler + png_align((int64_t)p->N * (int64_t)sizeof(uint32_t));
    return EG3D_OK;
}

int png_check(const eg3d_png_params* p, PngGeom& g, PngLayout& l) {
    const int s = png_geom(p, g, l);
    if (s != EG3D_OK) return s;
    if (p->img == nullptr || p->workspace == nullptr || p->offsets == nullptr || p->workspace_bytes < l.total ||
        (reinterpret_cast<uintptr_t>(p->workspace) & (PNG_ALIGN - 1)))
        return EG3D_ERR_INVALID;
    return EG3D_OK;
}

std::atomic<uint64_t> png_filter_lds_done{0}, png_deflate_lds_done{0};

}  // namespace

extern "C" int eg3d_png_query_workspace(const eg3d_png_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    PngGeom g;
    PngLayout l;
    const int s = png_geom(p, g, l);
    if (s != EG3D_OK) return s;
    *workspace_bytes = l.total;
    return EG3D_OK;
}

extern "C" int eg3d_png_encode(const eg3d_png_params* p, void* stream) {
    PngGeom g;
    PngLayout l;
    const int s = png_check(p, g, l);
    if (s != EG3D_OK) return s;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(p->workspace);
    uint8_t* filt = reinterpret_cast<uint8_t*>(ws + l.filt);
    uint8_t* slots = reinterpret_cast<uint8_t*>(ws + l.slots);
    int32_t* lens = reinterpret_cast<int32_t*>(ws + l.lens);
    int64_t* dst = reinterpret_cast<int64_t*>(ws + l.dst);
    uint32_t* adl = reinterpret_cast<uint32_t*>(ws + l.adl);
    uint32_t* adler = reinterpret_cast<uint32_t*>(ws + l.adler);
    const int64_t M = (int64_t)g.N * g.I;
    const int stages = p->stages == 0 ? 3 : p->stages;
    if (stages & 1) {
        const int lds = 2 * (int)png_align(g.rowb + 8);
        if (lds > 65536) {
            const int e = eg3d_ensure_dynamic_lds(reinterpret_cast<const void*>(png_filter_kernel), 2 * (int)png_align(3 * 16384 + 8), png_filter_lds_done);
            if (e) return e;
        }
        hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((int64_t)g.N * g.H)), dim3(PNG_FILTER_THREADS), lds, st, p->img, g, filt);
        EG3D_LAUNCH_CHECK();
    }
    if (stages & 2) {
        const int lds = png_lds_layout(g.bb).total;
        if (lds > 65536) {
            const int e = eg3d_ensure_dynamic_lds(reinterpret_cast<const void*>(png_deflate_kernel), png_lds_layout(65536).total, png_deflate_lds_done);
            if (e) return e;
        }
        hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)M), dim3(PNG_THREADS), lds, st, filt, g, slots, lens, adl);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(PNG_SCAN_THREADS), 0, st, lens, g, dst, p->offsets);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned)g.N), dim3(PNG_ADLER_THREADS), 0, st, adl, g, adler);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

extern "C" int eg3d_png_pack(const eg3d_png_params* p, void* stream) {
    PngGeom g;
    PngLayout l;
    const int s = png_check(p, g, l);
    if (s != EG3D_OK) return s;
    if (p->out_capacity < 0 || p->total_bytes < 0 || (p->out_capacity > 0 && p->out == nullptr)) return EG3D_ERR_INVALID;
    if (p->out_capacity < p->total_bytes) return EG3D_ERR_INVALID;              // total_bytes = offsets[N] as the caller read it: nothing is written
    if (p->out_capacity == 0) return EG3D_OK;
    hipStream_t st = (hipStream_t)stream;
    const char* ws = reinterpret_cast<const char*>(p->workspace);
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)((int64_t)g.N * g.I)), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(ws + l.slots),
                       reinterpret_cast<const int32_t*>(ws + l.lens), reinterpret_cast<const int64_t*>(ws + l.dst),
                       reinterpret_cast<const uint32_t*>(ws + l.adler), g, p->out, p->out_capacity);
    EG3D_LAUNCH_CHECK();
    return EG3D_OK;
}
