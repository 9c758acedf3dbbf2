// Baseline JPEG decoder (target-image ingestion: the photographs arrive as JPEGs; include/eg3d_hip.h "Baseline JPEG decoder").  One image per
// call, or N images of any geometry per call (eg3d_jpegdec_batch_*: the same kernels, each launched once, the image in blockIdx.y -- .z for
// the colour pass -- and its record read from device memory); integers only, the output bytes are those of libjpeg(-turbo)'s default decode
// (ISLOW IDCT, fancy upsampling).
//
//   jd_marker_count / _scan / _apply   the raw entropy-coded segment: every FF xx classified (FF 00 stuffing, FF D0..D7 restart, else status), a
//                                      scan of the kept bytes and of the restart markers, the compaction -> the unstuffed stream and the start
//                                      of every restart segment in it
//   jd_segments_kernel                 one workgroup: every segment cut into subsequences of B bytes, one lane each -> lane_base[segment]
//   jd_sync_kernel                     the self-synchronising Huffman decode inside a workgroup of 256 lanes: a lane decodes its subsequence
//                                      from a guessed state (first lane of a segment: the known one) and records the state it leaves in; then
//                                      in rounds every lane re-decodes from its left neighbour's recorded exit state (LDS) until a round changes
//                                      nothing.  Per lane: exit state, entry state used, blocks started, DC differences summed per component
//   jd_stitch_kernel                   one workgroup: the same rounds across the workgroup borders (the first lane of a workgroup against the
//                                      last of the one before; a changed entry is walked lane by lane until it meets a recorded exit state or
//                                      the workgroup ends) to the fixed point; exclusive scan of the per-lane counts and DC sums; every
//                                      segment's block total and final state checked against the geometry
//   jd_write_kernel                    every lane decodes once more from its now true entry state and writes the coefficients (natural order,
//                                      DC already predicted: the prefix of the DC sums) into the zeroed int16 [blocks][64]
//   jd_idct_kernel                     dequantisation and jidctint's ISLOW inverse DCT, 32 blocks per workgroup -> one uint8 plane per component
//   jd_colour_kernel                   one thread per pixel: fancy upsampling of the chroma, YCbCr -> RGB -> uint8 [H][W][3]
// The per-item arithmetic is csrc/jpeg_decode_core.h.  Every store of the entropy passes is guarded by the geometry and every read beyond a
// segment's end yields zero bits: a malformed stream ends in a status, not in an access out of range.  The only atomics are integer ORs into
// the status word (order-independent).
#include <algorithm>

#include "common.h"
#include "jpeg_decode_core.h"

#define JPEG_TABLE static __constant__ const
#include "jpeg_tables.h"

namespace {

constexpr int JD_LANES = 256;                       // lanes (threads) per workgroup of the decode passes
constexpr int JD_CHUNK = 4096;                      // raw bytes per workgroup of the marker pass: 256 threads x 16
constexpr int JD_ONE = 1024;                        // threads of the single-workgroup kernels
constexpr int64_t JD_ALIGN = 16;
constexpr int JD_QUANT_BYTES = 256, JD_HUFF_BYTES = 16 + 256;     // the tables blob: quant[4][64], then DC0, DC1, AC0, AC1 as BITS[16] HUFFVAL[256]
// result words
constexpr int JD_STATUS = 0, JD_ROUNDS_IN = 1, JD_ROUNDS_X = 2, JD_L = 3, JD_TOTAL = 4, JD_NRST = 5;

// the workspace ranges of one image, in the order they lie in (each a multiple of JD_ALIGN bytes)
enum { F_SUMS, F_OFFS, F_STREAM, F_SEG_START, F_LANE_BASE, F_EXIT, F_ENTRY, F_ACC, F_PRE, F_ROUNDS, F_COEF, F_PLANE0, F_PLANE1, F_PLANE2, JD_FIELDS };

struct JdImage {                                    // everything the kernels know about one image: the geometry and where its data lies
    JdGeom g;
    const uint8_t* raw;                             // the entropy-coded segment as in the file
    const uint8_t* blob;                            // the tables
    uint8_t* out;
    int32_t* result;
    int2 *sums, *offs;
    uint8_t* stream;
    int32_t *seg_start, *lane_base;
    unsigned long long *exit_state, *entry_state;
    int4 *acc, *pre;
    int32_t* rounds;
    int16_t* coef;
    uint8_t* plane[3];
    int32_t pw[3], reserved;                        // padded plane widths
};

// where a workgroup finds its image: the one-image call passes the record as a kernel argument, the batch call an array in device memory
// (uniform per workgroup: scalar loads)
struct JdOne {
    JdImage im;
    __device__ __forceinline__ const JdImage& at(unsigned) const { return im; }
};
struct JdMany {
    const JdImage* ims;
    __device__ __forceinline__ const JdImage& at(unsigned i) const { return ims[i]; }
};

struct JdLane {
    int32_t seg, j;                                 // segment, subsequence within it
    uint32_t start, limit, segend;                  // bits
    int32_t blk_begin, blk_end;                     // the segment's blocks
};

__device__ __forceinline__ bool jd_is_rst(int b) { return b >= 0xD0 && b <= 0xD7; }

// the 16 raw bytes of thread t of chunk c with their neighbours: kept bytes, restart markers, status
struct JdBytes {
    uint32_t w[4];
    int prev, next;
    int64_t base;
};

__device__ __forceinline__ JdBytes jd_load16(const uint8_t* __restrict__ raw, int64_t n, int64_t base) {
    JdBytes r;
    r.base = base;
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
    r.prev = 0;
    r.next = 1;                                     // beyond the end: a byte that makes a trailing FF an error
    if (base < n) {
        const uint4 v = *reinterpret_cast<const uint4*>(raw + base);               // (the buffer is readable up to the next multiple of 16)
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
        if (base > 0) r.prev = raw[base - 1];
        if (base + 16 < n) r.next = raw[base + 16];
    }
    return r;
}

__device__ __forceinline__ int jd_byte(const JdBytes& r, int q) { return (int)((r.w[q >> 2] >> (8 * (q & 3))) & 0xffu); }

// flags of byte q: 1 kept, 2 a restart marker's FF, 4 error
__device__ __forceinline__ int jd_classify(const JdBytes& r, int64_t n, int q) {
    if (r.base + q >= n) return 0;
    const int cur = jd_byte(r, q);
    const int prev = q > 0 ? jd_byte(r, q - 1) : r.prev;
    const int next = r.base + q + 1 >= n ? 1 : (q < 15 ? jd_byte(r, q + 1) : r.next);
    if (prev == 0xFF && (cur == 0 || jd_is_rst(cur))) return 0;                    // the second byte of FF 00 / RSTm
    if (cur != 0xFF) return 1;
    if (next == 0) return 1;
    if (jd_is_rst(next)) return 2;
    return 4;
}

template <class Src>
__global__ void __launch_bounds__(256) jd_marker_count_kernel(Src src) {
    __shared__ int s_k[256], s_r[256];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    if ((int)blockIdx.x >= g.nchunks) return;                                      // (the whole workgroup: a batch's grid is its largest image's)
    const uint8_t* __restrict__ raw = im.raw;
    int2* __restrict__ sums = im.sums;
    int32_t* __restrict__ result = im.result;
    const int t = threadIdx.x;
    const JdBytes r = jd_load16(raw, g.n, (int64_t)blockIdx.x * JD_CHUNK + t * 16);
    int keep = 0, rst = 0, err = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int f = jd_classify(r, g.n, q);
        keep += f & 1; rst += (f >> 1) & 1; err |= f & 4;
    }
    s_k[t] = keep; s_r[t] = rst;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { s_k[t] += s_k[t + o]; s_r[t] += s_r[t + o]; }
        __syncthreads();
    }
    if (t == 0) sums[blockIdx.x] = make_int2(s_k[0], s_r[0]);
    if (err) atomicOr(&result[JD_STATUS], JD_ERR_MARKER);
}

// exclusive scan of M items by one workgroup of JD_ONE threads: thread t owns a run of consecutive items.  ld(j) -> int4, st(j, prefix).
// Returns the total.  sh: int4 [2][JD_ONE].
template <class Load, class Store>
__device__ __forceinline__ int4 jd_scan_one(int64_t M, Load ld, Store st, int4 (*sh)[JD_ONE]) {
    const int t = threadIdx.x;
    const int64_t per = (M + JD_ONE - 1) / JD_ONE, lo = min(M, t * per), hi = min(M, lo + per);
    int4 s = make_int4(0, 0, 0, 0);
    for (int64_t j = lo; j < hi; ++j) {
        const int4 v = ld(j);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    int cur = 0;
    sh[0][t] = s;
    __syncthreads();
    for (int o = 1; o < JD_ONE; o <<= 1) {
        int4 v = sh[cur][t];
        if (t >= o) {
            const int4 u = sh[cur][t - o];
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        sh[cur ^ 1][t] = v;
        __syncthreads();
        cur ^= 1;
    }
    int4 run = sh[cur][t];
    run.x -= s.x; run.y -= s.y; run.z -= s.z; run.w -= s.w;
    for (int64_t j = lo; j < hi; ++j) {
        const int4 v = ld(j);
        st(j, run);
        run.x += v.x; run.y += v.y; run.z += v.z; run.w += v.w;
    }
    const int4 total = sh[cur][JD_ONE - 1];
    __syncthreads();
    return total;
}

template <class Src>
__global__ void __launch_bounds__(JD_ONE) jd_marker_scan_kernel(Src src) {
    __shared__ int4 sh[2][JD_ONE];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const int2* __restrict__ sums = im.sums;
    int2* __restrict__ offs = im.offs;
    int32_t* __restrict__ seg_start = im.seg_start;
    int32_t* __restrict__ result = im.result;
    const int4 total = jd_scan_one(
        g.nchunks, [&](int64_t j) { const int2 v = sums[j]; return make_int4(v.x, v.y, 0, 0); },
        [&](int64_t j, int4 p) { offs[j] = make_int2(p.x, p.y); }, sh);
    if (threadIdx.x == 0) {
        result[JD_TOTAL] = total.x;
        result[JD_NRST] = total.y;
        seg_start[0] = 0;
        seg_start[g.nseg] = total.x;
    }
}

template <class Src>
__global__ void __launch_bounds__(256) jd_marker_apply_kernel(Src src) {
    __shared__ int s_k[2][256], s_r[2][256];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    if ((int)blockIdx.x >= g.nchunks) return;                                      // (the whole workgroup)
    const uint8_t* __restrict__ raw = im.raw;
    const int2* __restrict__ offs = im.offs;
    uint8_t* __restrict__ stream = im.stream;
    int32_t* __restrict__ seg_start = im.seg_start;
    int32_t* __restrict__ result = im.result;
    const int t = threadIdx.x;
    const JdBytes r = jd_load16(raw, g.n, (int64_t)blockIdx.x * JD_CHUNK + t * 16);
    int flags[16], keep = 0, rst = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        flags[q] = jd_classify(r, g.n, q);
        keep += flags[q] & 1; rst += (flags[q] >> 1) & 1;
    }
    int cur = 0;
    s_k[0][t] = keep; s_r[0][t] = rst;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        s_k[cur ^ 1][t] = s_k[cur][t] + (t >= o ? s_k[cur][t - o] : 0);
        s_r[cur ^ 1][t] = s_r[cur][t] + (t >= o ? s_r[cur][t - o] : 0);
        __syncthreads();
        cur ^= 1;
    }
    const int2 off = offs[blockIdx.x];
    int64_t pos = (int64_t)off.x + s_k[cur][t] - keep;        // < g.n: at most one kept byte per raw byte
    int seg = off.y + s_r[cur][t] - rst;                      // restart markers before this thread
    int err = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (flags[q] & 1) stream[pos++] = (uint8_t)jd_byte(r, q);
        if (flags[q] & 2) {
            const int m = (q < 15 ? jd_byte(r, q + 1) : r.next) - 0xD0;
            if (m != (seg & 7)) err = 1;                       // RSTm out of sequence
            ++seg;                                             // the segment that starts here
            if (seg < g.nseg) seg_start[seg] = (int32_t)pos;
        }
    }
    if (err) atomicOr(&result[JD_STATUS], JD_ERR_SEGMENTS);
}

template <class Src>
__global__ void __launch_bounds__(JD_ONE) jd_segments_kernel(Src src) {
    __shared__ int4 sh[2][JD_ONE];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const int32_t* __restrict__ seg_start = im.seg_start;
    int32_t* __restrict__ lane_base = im.lane_base;
    int32_t* __restrict__ result = im.result;
    const bool ok = result[JD_STATUS] == 0 && result[JD_NRST] + 1 == g.nseg;       // (written by earlier launches)
    __syncthreads();
    if (!ok) {
        if (threadIdx.x == 0) {
            if (result[JD_NRST] + 1 != g.nseg) atomicOr(&result[JD_STATUS], JD_ERR_SEGMENTS);
            result[JD_L] = 0;                                                      // nothing for the decode passes to do
        }
        return;
    }
    // with the expected number of restart markers every seg_start[1 .. nseg - 1] was written once, in increasing order, all <= the total
    const int4 total = jd_scan_one(
        g.nseg, [&](int64_t s) { const int len = seg_start[s + 1] - seg_start[s]; return make_int4(max(1, (len + g.B - 1) / g.B), 0, 0, 0); },
        [&](int64_t s, int4 p) { lane_base[s] = p.x; }, sh);
    if (threadIdx.x == 0) {
        lane_base[g.nseg] = total.x;
        result[JD_L] = min(total.x, g.Lmax);                                       // (total <= Lmax by the bound the workspace was sized with)
        if (total.x > g.Lmax) atomicOr(&result[JD_STATUS], JD_ERR_SEGMENTS);
    }
}

// has any thread of the workgroup raised its flag?  (Plain LDS stores of one value between barriers; every thread must call it.)
__device__ __forceinline__ bool jd_any(bool mine, int* s_flag) {
    if (threadIdx.x == 0) *s_flag = 0;
    __syncthreads();
    if (mine) {
        *s_flag = 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                          // retired inside the branch: the store is not in flight at whatever barrier the layout puts next
    }
    __syncthreads();
    const bool any = *s_flag != 0;
    __syncthreads();                                                               // read before the next call's reset
    return any;
}

// the four tables into LDS: limits by four threads, then the 9-bit lookup by everyone.  blob: the tables argument of the C-ABI
__device__ __forceinline__ void jd_load_tables(const uint8_t* __restrict__ blob, JdHuff* tabs, int nthreads) {
    const int t = threadIdx.x;
    for (int i = t; i < 4 * 256; i += nthreads) tabs[i >> 8].vals[i & 255] = blob[JD_QUANT_BYTES + (i >> 8) * JD_HUFF_BYTES + 16 + (i & 255)];
    if (t < 4) jd_build_limits(blob + JD_QUANT_BYTES + t * JD_HUFF_BYTES, tabs[t]);
    __syncthreads();
    for (int i = t; i < 4 * 512; i += nthreads) tabs[i >> 9].lut[i & 511] = jd_lut_entry(tabs[i >> 9], i & 511);
    __syncthreads();
}

__device__ __forceinline__ JdLane jd_lane(int i, const JdGeom& g, const int32_t* __restrict__ lane_base, const int32_t* __restrict__ seg_start) {
    int lo = 0, hi = g.nseg - 1;                                                   // the last segment s with lane_base[s] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lane_base[mid] <= i) lo = mid; else hi = mid - 1;
    }
    JdLane l;
    l.seg = lo;
    l.j = i - lane_base[lo];
    const uint32_t b0 = (uint32_t)seg_start[lo], b1 = (uint32_t)seg_start[lo + 1];
    l.segend = b1 * 8u;
    l.start = min(b0 * 8u + (uint32_t)l.j * (uint32_t)g.B * 8u, l.segend);
    l.limit = min(l.start + (uint32_t)g.B * 8u, l.segend);
    if (i + 1 == lane_base[lo + 1]) l.limit = l.segend;
    l.blk_begin = lo * g.R * g.bpm;
    l.blk_end = min(g.mcus, (lo + 1) * g.R) * g.bpm;
    return l;
}

template <class Src>
__global__ void __launch_bounds__(JD_LANES) jd_sync_kernel(Src src) {
    __shared__ JdHuff tabs[4];
    __shared__ unsigned long long s_exit[JD_LANES];
    __shared__ int s_flag;
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const uint8_t* __restrict__ blob = im.blob;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(im.stream);
    const int32_t* __restrict__ lane_base = im.lane_base;
    const int32_t* __restrict__ seg_start = im.seg_start;
    unsigned long long* __restrict__ exit_state = im.exit_state;
    unsigned long long* __restrict__ entry_state = im.entry_state;
    int4* __restrict__ acc_out = im.acc;
    int32_t* __restrict__ rounds_wg = im.rounds;
    const int32_t* __restrict__ result = im.result;
    const int t = threadIdx.x, L = result[JD_L];
    const int i = blockIdx.x * JD_LANES + t;
    if (blockIdx.x * JD_LANES >= L) return;                                        // (the whole workgroup)
    jd_load_tables(blob, tabs, JD_LANES);
    const bool active = i < L;
    JdLane l;
    l.j = 0; l.start = l.limit = l.segend = 0u;
    if (active) l = jd_lane(i, g, lane_base, seg_start);
    // round 0: from the subsequence's first bit, block 0, coefficient 0 -- the truth for the first lane of a segment, a guess for the others
    unsigned long long ent = jd_pack(l.start, 0, 0), ex;
    int32_t acc[4];
    auto run = [&](unsigned long long from) {
        uint32_t p; int b, k;
        jd_unpack(from, p, b, k);
        acc[0] = acc[1] = acc[2] = acc[3] = 0;
        jd_decode<false>(tabs, words, g, l.segend, l.limit, p, b, k, acc, nullptr, 0, 0, nullptr);
        return (unsigned long long)jd_pack(p, b, k);
    };
    ex = run(ent);
    s_exit[t] = ex;
    const bool follows = active && l.j > 0 && t > 0;                               // takes its entry from the lane to its left in this workgroup
    int rounds = 0;
    while (true) {
        __syncthreads();
        const unsigned long long e = follows ? s_exit[t - 1] : ent;
        const bool redo = e != ent;
        if (redo) {
            ent = e;
            ex = run(e);
        }
        __syncthreads();                                                           // every read of this round is done
        bool changed = false;
        if (redo && ex != s_exit[t]) {
            s_exit[t] = ex;
            changed = true;
        }
        if (!jd_any(changed, &s_flag)) break;                                      // the fixed point: a round that changed nothing
        ++rounds;                                                                  // (at most JD_LANES - 1 rounds change something)
    }
    if (active) {
        exit_state[i] = ex;
        entry_state[i] = ent;
        acc_out[i] = make_int4(acc[0], acc[1], acc[2], acc[3]);
    }
    if (t == 0) rounds_wg[blockIdx.x] = rounds;
}

template <class Src>
__global__ void __launch_bounds__(JD_ONE) jd_stitch_kernel(Src src) {
    __shared__ JdHuff tabs[4];
    __shared__ int4 sh[2][JD_ONE];
    __shared__ int s_max[JD_ONE];
    __shared__ int s_flag;
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const uint8_t* __restrict__ blob = im.blob;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(im.stream);
    const int32_t* __restrict__ lane_base = im.lane_base;
    const int32_t* __restrict__ seg_start = im.seg_start;
    unsigned long long* __restrict__ exit_state = im.exit_state;
    unsigned long long* __restrict__ entry_state = im.entry_state;
    int4* __restrict__ acc_io = im.acc;
    int4* __restrict__ pre = im.pre;
    const int32_t* __restrict__ rounds_wg = im.rounds;
    int32_t* __restrict__ result = im.result;
    const int t = threadIdx.x, L = result[JD_L];
    if (L <= 0) return;
    jd_load_tables(blob, tabs, JD_ONE);
    const int nwg = (L + JD_LANES - 1) / JD_LANES;
    // the rounds across the workgroup borders.  A pass handles JD_ONE borders: first everyone reads the state left of its border, then the
    // changed ones are walked -- a walk writes only lanes of its own workgroup, so no lane has two writers and no read races a write
    int rounds = 0;
    while (true) {
        bool any = false;
        for (int w0 = 1; w0 < nwg; w0 += JD_ONE) {
            const int w = w0 + t, i0 = w * JD_LANES;
            unsigned long long e = 0;
            bool walk = false;
            JdLane l;
            if (w < nwg) {
                l = jd_lane(i0, g, lane_base, seg_start);
                if (l.j > 0) {
                    e = exit_state[i0 - 1];
                    walk = e != entry_state[i0];
                }
            }
            __syncthreads();
            if (walk) {
                any = true;
                const int iend = min(i0 + JD_LANES, L);
                for (int i = i0; i < iend; ++i) {
                    if (i > i0) {
                        l = jd_lane(i, g, lane_base, seg_start);
                        if (l.j == 0) break;                                       // a new segment: its state is known
                    }
                    uint32_t p; int b, k;
                    int32_t acc[4] = {0, 0, 0, 0};
                    jd_unpack(e, p, b, k);
                    jd_decode<false>(tabs, words, g, l.segend, l.limit, p, b, k, acc, nullptr, 0, 0, nullptr);
                    const unsigned long long ex = jd_pack(p, b, k);
                    entry_state[i] = e;
                    acc_io[i] = make_int4(acc[0], acc[1], acc[2], acc[3]);
                    if (ex == exit_state[i]) break;                                // synchronised: the lanes to the right stand
                    exit_state[i] = ex;
                    e = ex;
                }
            }
            __threadfence();
            __syncthreads();
        }
        if (!jd_any(any, &s_flag)) break;
        ++rounds;                                                                  // (at most nwg - 1 rounds change something)
    }
    __threadfence();
    __syncthreads();
    int m = 0;
    for (int w = t; w < nwg; w += JD_ONE) m = max(m, rounds_wg[w]);
    s_max[t] = m;
    __syncthreads();
    for (int o = JD_ONE / 2; o > 0; o >>= 1) {
        if (t < o) s_max[t] = max(s_max[t], s_max[t + o]);
        __syncthreads();
    }
    if (t == 0) {
        result[JD_ROUNDS_IN] = s_max[0];
        result[JD_ROUNDS_X] = rounds;
    }
    // where every lane's first block and DC predictions are: the prefix of the counts and sums (taken relative to the segment's first lane)
    jd_scan_one(L, [&](int64_t j) { return acc_io[j]; }, [&](int64_t j, int4 p) { pre[j] = p; }, sh);
    __threadfence();
    __syncthreads();
    int err = 0;
    for (int s = t; s < g.nseg; s += JD_ONE) {
        const int first = lane_base[s], last = lane_base[s + 1] - 1;
        if (last >= L || last < first) { err = 1; continue; }
        const int blocks = pre[last].x + acc_io[last].x - pre[first].x;
        uint32_t p; int b, k;
        jd_unpack(exit_state[last], p, b, k);
        if (blocks != (min(g.mcus, (s + 1) * g.R) - s * g.R) * g.bpm || b != 0 || k != 0) err = 1;
    }
    if (err) atomicOr(&result[JD_STATUS], JD_ERR_BLOCKS);
}

template <class Src>
__global__ void __launch_bounds__(JD_LANES) jd_write_kernel(Src src) {
    __shared__ JdHuff tabs[4];
    __shared__ uint8_t s_nat[64];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const uint8_t* __restrict__ blob = im.blob;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(im.stream);
    const int32_t* __restrict__ lane_base = im.lane_base;
    const int32_t* __restrict__ seg_start = im.seg_start;
    const unsigned long long* __restrict__ exit_state = im.exit_state;
    const int4* __restrict__ pre = im.pre;
    int16_t* __restrict__ coef = im.coef;
    int32_t* __restrict__ result = im.result;
    const int t = threadIdx.x, L = result[JD_L];
    if (blockIdx.x * JD_LANES >= L || result[JD_STATUS] != 0) return;             // (the whole workgroup: both were written by earlier launches)
    if (t < 64) s_nat[jpeg_zz_of_nat[t]] = (uint8_t)t;
    jd_load_tables(blob, tabs, JD_LANES);
    const int i = blockIdx.x * JD_LANES + t;
    if (i >= L) return;
    const JdLane l = jd_lane(i, g, lane_base, seg_start);
    uint32_t p = l.start; int b = 0, k = 0;
    if (l.j > 0) jd_unpack(exit_state[i - 1], p, b, k);
    const int4 mine = pre[i], first = pre[i - l.j];
    int32_t acc[4] = {mine.x - first.x, mine.y - first.y, mine.z - first.z, mine.w - first.w};
    const uint32_t err = jd_decode<true>(tabs, words, g, l.segend, l.limit, p, b, k, acc, coef, l.blk_begin, l.blk_end, s_nat);
    if (err) atomicOr(&result[JD_STATUS], (int)err);
}

// 32 blocks per workgroup; thread = (block, column) in the column pass, (block, row) in the row pass.  LDS rows are 9 words apart: no bank conflicts
template <class Src>
__global__ void __launch_bounds__(256) jd_idct_kernel(Src src) {
    __shared__ int32_t s_v[32 * 72];
    __shared__ int32_t s_q[3 * 64];
    const JdImage& im = src.at(blockIdx.y);
    const JdGeom g = im.g;
    const int64_t blk0 = (int64_t)blockIdx.x * 32;
    if (blk0 >= g.nblk) return;                                                    // (the whole workgroup)
    const int16_t* __restrict__ coef = im.coef;
    const uint8_t* __restrict__ blob = im.blob;
    const int t = threadIdx.x;
    if (t < g.ncomp * 64) s_q[t] = blob[(t < 64 ? g.tq[0] : (t < 128 ? g.tq[1] : g.tq[2])) * 64 + (t & 63)];   // (constant indices: the record stays in registers)
    __syncthreads();
    for (int e = t; e < 32 * 64; e += 256) {                                       // coalesced: 2048 consecutive coefficients
        const int64_t blk = blk0 + (e >> 6);
        int v = 0;
        if (blk < g.nblk) v = (int)coef[blk * 64 + (e & 63)] * s_q[jd_comp_of(g, (int)(blk % g.bpm)) * 64 + (e & 63)];
        s_v[(e >> 6) * 72 + ((e & 63) >> 3) * 9 + (e & 7)] = v;
    }
    __syncthreads();
    const int lb = t >> 3, idx = t & 7;
    int32_t x[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = s_v[lb * 72 + r * 9 + idx];
    jd_idct8(x, 11);                                                               // CONST_BITS - PASS1_BITS
#pragma unroll
    for (int r = 0; r < 8; ++r) s_v[lb * 72 + r * 9 + idx] = x[r];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = s_v[lb * 72 + idx * 9 + c];
    jd_idct8(x, 18);                                                               // CONST_BITS + PASS1_BITS + 3
    const int64_t blk = blk0 + lb;
    if (blk >= g.nblk) return;
    const int mcu = (int)(blk / g.bpm), b = (int)(blk % g.bpm), comp = jd_comp_of(g, b);
    const int hc = comp == 0 ? g.hs : 1, vc = comp == 0 ? g.vs : 1, bi = comp == 0 ? b : 0;
    const int x0 = ((mcu % g.mx) * hc + bi % hc) * 8, y0 = ((mcu / g.mx) * vc + bi / hc) * 8 + idx;      // < pw, ph: whole MCUs
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        lo |= (uint32_t)jd_range_limit(x[c]) << (8 * c);
        hi |= (uint32_t)jd_range_limit(x[c + 4]) << (8 * c);
    }
    uint8_t* plane = comp == 0 ? im.plane[0] : (comp == 1 ? im.plane[1] : im.plane[2]);
    const int pw = comp == 0 ? im.pw[0] : (comp == 1 ? im.pw[1] : im.pw[2]);
    *reinterpret_cast<uint2*>(plane + (int64_t)y0 * pw + x0) = make_uint2(lo, hi);   // 8-byte aligned: the plane, pw and x0 are multiples of 8
}

template <class Src>
__global__ void __launch_bounds__(256) jd_colour_kernel(Src src) {
    const JdImage& im = src.at(blockIdx.z);
    const JdGeom g = im.g;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    uint8_t* __restrict__ out = im.out;
    const int yy = im.plane[0][(int64_t)y * im.pw[0] + x];
    uint8_t rgb[3];
    if (g.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)yy;
    } else {
        const int dw = (g.W + g.hs - 1) / g.hs, dh = (g.H + g.vs - 1) / g.vs;      // the chroma's real size
        const int cb = jd_chroma(im.plane[1], im.pw[1], dw, dh, g.hs, g.vs, y, x);
        const int cr = jd_chroma(im.plane[2], im.pw[2], dw, dh, g.hs, g.vs, y, x);
        jd_ycc_to_rgb(yy, cb, cr, rgb);
    }
    uint8_t* o = out + ((int64_t)y * g.W + x) * 3;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

int64_t jd_align(int64_t b) { return (b + JD_ALIGN - 1) / JD_ALIGN * JD_ALIGN; }

// one image as either entry describes it
struct JdDesc {
    int32_t H, W, ncomp, hsamp, vsamp, restart_interval;
    const int32_t *tq, *td, *ta;
    int64_t data_bytes;
};

int jd_call_args(int B, int stages) { return (B < 16 || B > 1024 || (B & (B - 1)) || stages < 0 || stages > 31) ? EG3D_ERR_INVALID : EG3D_OK; }

// the geometry of one image, the bytes of each of its workspace ranges and its padded plane widths
int jd_geom(const JdDesc& p, int B, JdGeom& g, int64_t* size, int32_t* pw) {
    if (p.H < 1 || p.W < 1 || p.H > 65535 || p.W > 65535 || (p.ncomp != 1 && p.ncomp != 3) || p.data_bytes < 0 || p.restart_interval < 0 ||
        p.restart_interval > 65535)
        return EG3D_ERR_INVALID;
    g.ncomp = p.ncomp;
    g.hs = p.ncomp == 3 ? p.hsamp : 1;
    g.vs = p.ncomp == 3 ? p.vsamp : 1;
    if (!((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2))) return EG3D_ERR_UNSUPPORTED;
    g.dc_sel = g.ac_sel = 0;
    for (int c = 0; c < 3; ++c) {
        g.tq[c] = 0;
        if (c >= p.ncomp) continue;
        if (p.tq[c] < 0 || p.tq[c] > 3 || p.td[c] < 0 || p.td[c] > 1 || p.ta[c] < 0 || p.ta[c] > 1) return EG3D_ERR_INVALID;
        g.tq[c] = p.tq[c];
        g.dc_sel |= p.td[c] << c;
        g.ac_sel |= p.ta[c] << c;
    }
    if (p.data_bytes >= (1ll << 28)) return EG3D_ERR_TOO_LARGE;                     // bit positions are 32-bit
    g.H = p.H; g.W = p.W; g.B = B; g.n = p.data_bytes;
    g.mx = (p.W + 8 * g.hs - 1) / (8 * g.hs);
    g.my = (p.H + 8 * g.vs - 1) / (8 * g.vs);
    const int64_t mcus = (int64_t)g.mx * g.my;
    g.bpm = p.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    if (mcus * g.bpm * 64 > INT32_MAX) return EG3D_ERR_TOO_LARGE;
    g.mcus = (int32_t)mcus;
    g.nblk = (int32_t)(mcus * g.bpm);
    g.R = p.restart_interval > 0 ? (int32_t)(p.restart_interval < mcus ? p.restart_interval : mcus) : (int32_t)mcus;
    g.nseg = (int32_t)((mcus + g.R - 1) / g.R);
    g.Lmax = (int32_t)(g.n / B) + g.nseg + 1;                                      // sum over the segments of max(1, ceil(len / B)) <= n / B + nseg
    g.nchunks = (int32_t)((g.n + JD_CHUNK - 1) / JD_CHUNK);
    const int nwg = (g.Lmax + JD_LANES - 1) / JD_LANES;
    if (nwg > 65536) return EG3D_ERR_TOO_LARGE;
    size[F_SUMS] = jd_align((int64_t)(g.nchunks + 1) * 8);
    size[F_OFFS] = jd_align((int64_t)(g.nchunks + 1) * 8);
    size[F_STREAM] = jd_align(g.n + 16);                                           // the decode reads whole dwords, one beyond the last bit's
    size[F_SEG_START] = jd_align((int64_t)(g.nseg + 1) * 4);
    size[F_LANE_BASE] = jd_align((int64_t)(g.nseg + 1) * 4);
    size[F_EXIT] = jd_align((int64_t)g.Lmax * 8);
    size[F_ENTRY] = jd_align((int64_t)g.Lmax * 8);
    size[F_ACC] = jd_align((int64_t)g.Lmax * 16);
    size[F_PRE] = jd_align((int64_t)g.Lmax * 16);
    size[F_ROUNDS] = jd_align((int64_t)nwg * 4);
    size[F_COEF] = jd_align((int64_t)g.nblk * 64 * 2);
    for (int c = 0; c < 3; ++c) {
        pw[c] = g.mx * 8 * (c == 0 ? g.hs : 1);
        size[F_PLANE0 + c] = c < g.ncomp ? jd_align((int64_t)pw[c] * (g.my * 8 * (c == 0 ? g.vs : 1))) : 0;
    }
    return EG3D_OK;
}

void jd_bind(JdImage& im, char* ws, const int64_t* off, const int32_t* pw) {
    im.sums = reinterpret_cast<int2*>(ws + off[F_SUMS]);
    im.offs = reinterpret_cast<int2*>(ws + off[F_OFFS]);
    im.stream = reinterpret_cast<uint8_t*>(ws + off[F_STREAM]);
    im.seg_start = reinterpret_cast<int32_t*>(ws + off[F_SEG_START]);
    im.lane_base = reinterpret_cast<int32_t*>(ws + off[F_LANE_BASE]);
    im.exit_state = reinterpret_cast<unsigned long long*>(ws + off[F_EXIT]);
    im.entry_state = reinterpret_cast<unsigned long long*>(ws + off[F_ENTRY]);
    im.acc = reinterpret_cast<int4*>(ws + off[F_ACC]);
    im.pre = reinterpret_cast<int4*>(ws + off[F_PRE]);
    im.rounds = reinterpret_cast<int32_t*>(ws + off[F_ROUNDS]);
    im.coef = reinterpret_cast<int16_t*>(ws + off[F_COEF]);
    for (int c = 0; c < 3; ++c) {
        im.plane[c] = reinterpret_cast<uint8_t*>(ws + off[F_PLANE0 + c]);
        im.pw[c] = pw[c];
    }
    im.reserved = 0;
}

// what a call launches, over all of its images
struct JdGrid {
    int n;                                           // images
    int nchunks, nwg, nblk, tx, ty;                  // the largest image's workgroups per pass
    char* ws;
    int64_t zero_segs, zero_segs_words, zero_coef, zero_coef_words;      // the ranges a call zeroes: segment starts + lane bases, coefficients
    int32_t* result;
};

void jd_grid_add(JdGrid& k, const JdGeom& g) {
    k.nchunks = std::max(k.nchunks, g.nchunks);
    k.nwg = std::max(k.nwg, (g.Lmax + JD_LANES - 1) / JD_LANES);
    k.nblk = std::max(k.nblk, (g.nblk + 31) / 32);
    k.tx = std::max(k.tx, (g.W + 63) / 64);
    k.ty = std::max(k.ty, (g.H + 3) / 4);
}

// the launches of both entries: every pass once, whatever the number of images
template <class Src>
int jd_run(const Src& src, const JdGrid& k, int stages, hipStream_t st) {
    const unsigned n = (unsigned)k.n;
    if (stages == 0) stages = 31;
    if (stages & EG3D_JPEGDEC_STAGE_MARKERS) {
        eg3d_zero_words(k.result, (int64_t)k.n * EG3D_JPEGDEC_RESULT_WORDS, st);
        eg3d_zero_words(k.ws + k.zero_segs, k.zero_segs_words, st);
        EG3D_LAUNCH_CHECK();
        if (k.nchunks > 0) {
            hipLaunchKernelGGL(jd_marker_count_kernel<Src>, dim3((unsigned)k.nchunks, n), dim3(256), 0, st, src);
            EG3D_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(jd_marker_scan_kernel<Src>, dim3(1, n), dim3(JD_ONE), 0, st, src);
        EG3D_LAUNCH_CHECK();
        if (k.nchunks > 0) {
            hipLaunchKernelGGL(jd_marker_apply_kernel<Src>, dim3((unsigned)k.nchunks, n), dim3(256), 0, st, src);
            EG3D_LAUNCH_CHECK();
        }
    }
    if (stages & EG3D_JPEGDEC_STAGE_SYNC) {
        hipLaunchKernelGGL(jd_segments_kernel<Src>, dim3(1, n), dim3(JD_ONE), 0, st, src);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(jd_sync_kernel<Src>, dim3((unsigned)k.nwg, n), dim3(JD_LANES), 0, st, src);
        EG3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(jd_stitch_kernel<Src>, dim3(1, n), dim3(JD_ONE), 0, st, src);
        EG3D_LAUNCH_CHECK();
    }
    if (stages & EG3D_JPEGDEC_STAGE_WRITE) {
        eg3d_zero_words(k.ws + k.zero_coef, k.zero_coef_words, st);
        hipLaunchKernelGGL(jd_write_kernel<Src>, dim3((unsigned)k.nwg, n), dim3(JD_LANES), 0, st, src);
        EG3D_LAUNCH_CHECK();
    }
    if (stages & EG3D_JPEGDEC_STAGE_IDCT) {
        hipLaunchKernelGGL(jd_idct_kernel<Src>, dim3((unsigned)k.nblk, n), dim3(256), 0, st, src);
        EG3D_LAUNCH_CHECK();
    }
    if (stages & EG3D_JPEGDEC_STAGE_COLOUR) {
        hipLaunchKernelGGL(jd_colour_kernel<Src>, dim3((unsigned)k.tx, (unsigned)k.ty, n), dim3(256), 0, st, src);
        EG3D_LAUNCH_CHECK();
    }
    return EG3D_OK;
}

// ---- one image -------------------------------------------------------------------------------------------------------------------------------------------
int jd_one(const eg3d_jpegdec_params* p, JdImage& im, int64_t* off) {                // off: JD_FIELDS + 1 offsets, the last one the total
    if (p == nullptr) return EG3D_ERR_INVALID;
    const JdDesc d = {p->H, p->W, p->ncomp, p->hsamp, p->vsamp, p->restart_interval, p->tq, p->td, p->ta, p->data_bytes};
    int64_t size[JD_FIELDS];
    int s = jd_call_args(p->subseq_bytes, p->stages);
    if (s == EG3D_OK) s = jd_geom(d, p->subseq_bytes, im.g, size, im.pw);
    if (s != EG3D_OK) return s;
    off[0] = 0;
    for (int f = 0; f < JD_FIELDS; ++f) off[f + 1] = off[f] + size[f];
    return EG3D_OK;
}

// ---- a batch ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int JD_MAX_BATCH = 65535;                  // the image is a grid dimension

int64_t jd_plan_bytes(int n) { return jd_align((int64_t)n * (int64_t)sizeof(JdImage)); }

bool jd_batch_pointers(const eg3d_jpegdec_batch_params* p, int64_t total) {
    return p->upload != nullptr && p->workspace != nullptr && p->result != nullptr && p->workspace_bytes >= total &&
           !(reinterpret_cast<uintptr_t>(p->workspace) & (JD_ALIGN - 1)) && !(reinterpret_cast<uintptr_t>(p->upload) & (JD_ALIGN - 1));
}

// Every image's geometry and place.  The workspace holds range after range, each range image after image, so that what a call zeroes is
// two stretches whatever the number of images.  plan (may be null): the records; k (may be null): the grid.
int jd_batch(const eg3d_jpegdec_batch_params* p, JdImage* plan, JdGrid* k, int64_t* total) {
    if (p == nullptr || p->images == nullptr || p->n < 1) return EG3D_ERR_INVALID;
    if (p->n > JD_MAX_BATCH) return EG3D_ERR_TOO_LARGE;
    int s = jd_call_args(p->subseq_bytes, p->stages);
    if (s != EG3D_OK) return s;
    int64_t range[JD_FIELDS + 1] = {0};              // bytes of every range over the batch, then their starts
    JdGeom g;
    int64_t size[JD_FIELDS];
    int32_t pw[3];
    for (int i = 0; i < p->n; ++i) {
        const eg3d_jpegdec_image& q = p->images[i];
        const JdDesc d = {q.H, q.W, q.ncomp, q.hsamp, q.vsamp, q.restart_interval, q.tq, q.td, q.ta, q.data_bytes};
        s = jd_geom(d, p->subseq_bytes, g, size, pw);
        if (s != EG3D_OK) return s;
        if (k != nullptr) jd_grid_add(*k, g);
        for (int f = 0; f < JD_FIELDS; ++f) range[f] += size[f];
    }
    int64_t at = 0;
    for (int f = 0; f <= JD_FIELDS; ++f) {
        const int64_t bytes = range[f];
        range[f] = at;
        at += bytes;
    }
    *total = range[JD_FIELDS];
    if ((plan != nullptr || k != nullptr) && !jd_batch_pointers(p, *total)) return EG3D_ERR_INVALID;
    if (k != nullptr) {
        k->n = p->n;
        k->ws = reinterpret_cast<char*>(p->workspace);
        k->result = p->result;
        k->zero_segs = range[F_SEG_START];
        k->zero_segs_words = (range[F_EXIT] - range[F_SEG_START]) / 4;
        k->zero_coef = range[F_COEF];
        k->zero_coef_words = (range[F_PLANE0] - range[F_COEF]) / 4;
    }
    if (plan == nullptr) return EG3D_OK;
    const int64_t head = jd_plan_bytes(p->n);
    int64_t off[JD_FIELDS];
    for (int f = 0; f < JD_FIELDS; ++f) off[f] = range[f];
    for (int i = 0; i < p->n; ++i) {
        const eg3d_jpegdec_image& q = p->images[i];
        const JdDesc d = {q.H, q.W, q.ncomp, q.hsamp, q.vsamp, q.restart_interval, q.tq, q.td, q.ta, q.data_bytes};
        JdImage& im = plan[i];
        jd_geom(d, p->subseq_bytes, im.g, size, pw);
        if (q.out == nullptr || q.data_offset < head || q.tables_offset < head || (q.data_offset & (JD_ALIGN - 1)) ||
            q.data_offset + jd_align(q.data_bytes) > p->upload_bytes || q.tables_offset + EG3D_JPEGDEC_TABLE_BYTES > p->upload_bytes)
            return EG3D_ERR_INVALID;
        jd_bind(im, reinterpret_cast<char*>(p->workspace), off, pw);
        im.raw = p->upload + q.data_offset;
        im.blob = p->upload + q.tables_offset;
        im.out = q.out;
        im.result = p->result + (int64_t)i * EG3D_JPEGDEC_RESULT_WORDS;
        for (int f = 0; f < JD_FIELDS; ++f) off[f] += size[f];
    }
    return EG3D_OK;
}

}  // namespace

extern "C" int eg3d_jpegdec_query_workspace(const eg3d_jpegdec_params* p, int64_t* workspace_bytes) {
    if (workspace_bytes == nullptr) return EG3D_ERR_INVALID;
    JdImage im;
    int64_t off[JD_FIELDS + 1];
    const int s = jd_one(p, im, off);
    if (s != EG3D_OK) return s;
    *workspace_bytes = off[JD_FIELDS];
    return EG3D_OK;
}

extern "C" int eg3d_jpegdec_decode(const eg3d_jpegdec_params* p, void* stream) {
    JdOne src;
    int64_t off[JD_FIELDS + 1];
    const int s = jd_one(p, src.im, off);
    if (s != EG3D_OK) return s;
    if (p->data == nullptr || p->tables == nullptr || p->workspace == nullptr || p->out == nullptr || p->result == nullptr ||
        p->workspace_bytes < off[JD_FIELDS] || (reinterpret_cast<uintptr_t>(p->workspace) & (JD_ALIGN - 1)) ||
        (reinterpret_cast<uintptr_t>(p->data) & (JD_ALIGN - 1)))
        return EG3D_ERR_INVALID;
    int32_t pw[3] = {src.im.pw[0], src.im.pw[1], src.im.pw[2]};
    jd_bind(src.im, reinterpret_cast<char*>(p->workspace), off, pw);
    src.im.raw = p->data;
    src.im.blob = p->tables;
    src.im.out = p->out;
    src.im.result = p->result;
    JdGrid k = {};
    jd_grid_add(k, src.im.g);
    k.n = 1;
    k.ws = reinterpret_cast<char*>(p->workspace);
    k.result = p->result;
    k.zero_segs = off[F_SEG_START];
    k.zero_segs_words = (off[F_EXIT] - off[F_SEG_START]) / 4;
    k.zero_coef = off[F_COEF];
    k.zero_coef_words = (off[F_PLANE0] - off[F_COEF]) / 4;
    return jd_run(src, k, p->stages, (hipStream_t)stream);
}

extern "C" int eg3d_jpegdec_batch_query_workspace(const eg3d_jpegdec_batch_params* p, int64_t* workspace_bytes, int64_t* plan_bytes) {
    if (workspace_bytes == nullptr || plan_bytes == nullptr) return EG3D_ERR_INVALID;
    int64_t total = 0;
    const int s = jd_batch(p, nullptr, nullptr, &total);
    if (s != EG3D_OK) return s;
    *workspace_bytes = total;
    *plan_bytes = jd_plan_bytes(p->n);
    return EG3D_OK;
}

extern "C" int eg3d_jpegdec_batch_plan(const eg3d_jpegdec_batch_params* p) {
    int64_t total = 0;
    if (p == nullptr || p->plan == nullptr || (reinterpret_cast<uintptr_t>(p->plan) & 7)) return EG3D_ERR_INVALID;
    return jd_batch(p, reinterpret_cast<JdImage*>(p->plan), nullptr, &total);
}

extern "C" int eg3d_jpegdec_batch_decode(const eg3d_jpegdec_batch_params* p, void* stream) {
    JdGrid k = {};
    int64_t total = 0;
    const int s = jd_batch(p, nullptr, &k, &total);
    if (s != EG3D_OK) return s;
    for (int i = 0; i < p->n; ++i)
        if (p->images[i].out == nullptr) return EG3D_ERR_INVALID;
    const JdMany src = {reinterpret_cast<const JdImage*>(p->upload)};
    return jd_run(src, k, p->stages, (hipStream_t)stream);
}
