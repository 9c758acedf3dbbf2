// The per-item arithmetic of the baseline JPEG decoder (csrc/jpeg_decode.hip; include/eg3d_hip.h "Baseline JPEG decoder"): what one lane does with
// one subsequence of the entropy-coded stream, one thread with one column or row of a block, one thread with one output pixel.  Integers only.
// Host and device: the same functions can be driven by a plain loop on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

// status bits (EG3D_JPEGDEC_ERR_*)
#define JD_ERR_MARKER 1
#define JD_ERR_SEGMENTS 2
#define JD_ERR_BLOCKS 4
#define JD_ERR_CODE 8

struct JdHuff {                          // one Huffman table as the decode passes keep it in LDS
    uint16_t lut[512];                   // the next 9 bits -> (code length << 8) | symbol; 0: the code is longer than 9 bits
    int32_t maxcode[18];                 // [1..16]: the largest code of that length, -1 where there is none (jdhuff.c)
    int32_t valoff[18];                  // [1..16]: symbol index = code + valoff
    uint8_t vals[256];                   // HUFFVAL, zero-filled
};

struct JdGeom {
    int32_t H, W, ncomp, hs, vs;         // hs x vs: the luma sampling factors (chroma 1 x 1)
    int32_t mx, my, mcus, bpm, nblk;     // MCUs per row / column / image, blocks per MCU / image
    int32_t R, nseg;                     // MCUs per restart segment (mcus without restarts), segments
    int32_t B, Lmax;                     // subsequence bytes, capacity of the lane arrays
    int32_t nchunks;                     // workgroups of the marker pass
    int32_t dc_sel, ac_sel;              // bit c: the DC / AC table of component c
    int32_t tq[3];
    int64_t n;                           // bytes of the raw entropy-coded segment
};

// component of block b of an MCU: hs * vs luma blocks, then Cb, Cr
JD_HD int jd_comp_of(const JdGeom& g, int b) {
    const int nl = g.hs * g.vs;
    return b < nl ? 0 : b - nl + 1;
}

// ---- Huffman tables -----------------------------------------------------------------------------------------------------------------------------------
JD_HD void jd_build_limits(const uint8_t* bits, JdHuff& h) {
    int code = 0, p = 0;
    h.maxcode[0] = -1; h.valoff[0] = 0; h.maxcode[17] = -1; h.valoff[17] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int nb = bits[l - 1];
        if (nb) {
            h.valoff[l] = p - code;
            p += nb;
            code += nb;
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
            h.valoff[l] = 0;
        }
        code <<= 1;
    }
}

JD_HD uint16_t jd_lut_entry(const JdHuff& h, int idx) {
    for (int l = 1; l <= 9; ++l) {
        const int c = idx >> (9 - l);
        if (c <= h.maxcode[l]) return (uint16_t)((l << 8) | h.vals[(c + h.valoff[l]) & 255]);
    }
    return 0;
}

// (flag << 16) | (code length << 8) | symbol of the code that opens `bits` (MSB first); flag: no code of the table matches (length 16, symbol 0)
JD_HD uint32_t jd_symbol(const JdHuff& h, uint32_t bits) {
    const uint32_t e = h.lut[bits >> 23];
    if (e) return e;
    for (int l = 10; l <= 16; ++l) {
        const int c = (int)(bits >> (32 - l));
        if (c <= h.maxcode[l]) return (uint32_t)((l << 8) | h.vals[(c + h.valoff[l]) & 255]);
    }
    return 0x10000u | (16u << 8);
}

// ---- the bit stream -------------------------------------------------------------------------------------------------------------------------------------
JD_HD uint32_t jd_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// 32 bits at bit position p of the unstuffed stream (dwords, bytes in file order), MSB first; every bit at or beyond `end` reads as zero and
// nothing beyond the dword after the one holding bit end - 1 is touched
JD_HD uint32_t jd_peek(const uint32_t* w, uint32_t p, uint32_t end) {
    if (p >= end) return 0u;
    const uint32_t i = p >> 5, sh = p & 31u;
    const uint32_t a = jd_bswap(w[i]), b = jd_bswap(w[i + 1]);
    const uint32_t v = sh ? (a << sh) | (b >> (32u - sh)) : a;
    const uint32_t rem = end - p;
    return rem < 32u ? v & ~(0xffffffffu >> rem) : v;
}

// ---- one lane's decode ------------------------------------------------------------------------------------------------------------------------------------
JD_HD uint64_t jd_pack(uint32_t p, int b, int k) { return (uint64_t)p | ((uint64_t)(uint32_t)b << 32) | ((uint64_t)(uint32_t)k << 40); }
JD_HD void jd_unpack(uint64_t s, uint32_t& p, int& b, int& k) { p = (uint32_t)s; b = (int)((s >> 32) & 0xff); k = (int)((s >> 40) & 0xff); }

// Decode symbols from state (p, b, k) -- bit position, block of the MCU, zigzag index -- until p >= limit or the next symbol does not fit
// the segment [.., segend).  acc[0] counts the blocks started (DC symbols), acc[1 + c] sums component c's DC differences; both continue from
// what the caller put there.  WRITE: acc came in as the lane's prefix within its segment, so block blk_begin + acc[0] - 1 is the current one
// and acc[1 + c] the running DC prediction; values go to coef[block][natural index], only for blocks in [blk_begin, blk_end) and k < 64.
// Returns status bits (meaningful for WRITE: a lane started from a wrong state may see anything).
template <bool WRITE>
JD_HD uint32_t jd_decode(const JdHuff* tabs, const uint32_t* words, const JdGeom& g, uint32_t segend, uint32_t limit, uint32_t& p, int& b, int& k,
                         int32_t* acc, int16_t* coef, int32_t blk_begin, int32_t blk_end, const uint8_t* nat) {
    uint32_t err = 0;
    while (p < limit) {
        const uint32_t bits = jd_peek(words, p, segend);
        const int comp = jd_comp_of(g, b);
        if (k == 0) {
            const uint32_t e = jd_symbol(tabs[(g.dc_sel >> comp) & 1], bits);
            const int len = (int)((e >> 8) & 0xff), s = (int)(e & 15u);
            if (p + (uint32_t)(len + s) > segend) break;
            if (e >> 16) err |= JD_ERR_CODE;
            int v = 0;
            if (s) {
                v = (int)((bits << len) >> (32 - s));
                if (v < (1 << (s - 1))) v -= (1 << s) - 1;
            }
            acc[0] += 1;
            acc[1 + comp] = (int32_t)((uint32_t)acc[1 + comp] + (uint32_t)v);
            if (WRITE) {
                const int32_t cur = blk_begin + acc[0] - 1;
                if (cur >= blk_begin && cur < blk_end) coef[(int64_t)cur * 64] = (int16_t)acc[1 + comp];
                else err |= JD_ERR_BLOCKS;
            }
            p += (uint32_t)(len + s);
            k = 1;
        } else {
            const uint32_t e = jd_symbol(tabs[2 + ((g.ac_sel >> comp) & 1)], bits);
            const int len = (int)((e >> 8) & 0xff), s = (int)(e & 15u), r = (int)((e >> 4) & 15u);
            if (p + (uint32_t)(len + s) > segend) break;
            if (e >> 16) err |= JD_ERR_CODE;
            if (s == 0) {
                k = r == 15 ? k + 16 : 64;                     // ZRL, or the end of the block (any other run with size 0 ends it, as in libjpeg)
            } else {
                k += r;
                if (WRITE) {
                    int v = (int)((bits << len) >> (32 - s));
                    if (v < (1 << (s - 1))) v -= (1 << s) - 1;
                    const int32_t cur = blk_begin + acc[0] - 1;
                    if (k < 64 && cur >= blk_begin && cur < blk_end) coef[(int64_t)cur * 64 + nat[k]] = (int16_t)v;
                    else err |= k < 64 ? JD_ERR_BLOCKS : JD_ERR_CODE;
                }
                k += 1;
            }
            p += (uint32_t)(len + s);
        }
        if (k >= 64) {
            k = 0;
            b = b + 1 == g.bpm ? 0 : b + 1;
        }
    }
    return err;
}

// ---- inverse DCT: jidctint.c jpeg_idct_islow, CONST_BITS 13 ----------------------------------------------------------------------------------------------
// one pass over x[0..7] in place, descaled by `shift` with rounding (11 for the column pass, 18 for the row pass); 32-bit wrap-around arithmetic
JD_HD void jd_idct8(int32_t* x, int shift) {
    typedef uint32_t U;
    const U in0 = (U)x[0], in1 = (U)x[1], in2 = (U)x[2], in3 = (U)x[3], in4 = (U)x[4], in5 = (U)x[5], in6 = (U)x[6], in7 = (U)x[7];
    U z1 = (in2 + in6) * 4433u;
    U tmp2 = z1 + in6 * (U)(-15137);
    U tmp3 = z1 + in2 * 6270u;
    U tmp0 = (in0 + in4) << 13;
    U tmp1 = (in0 - in4) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in7; tmp1 = in5; tmp2 = in3; tmp3 = in1;
    z1 = tmp0 + tmp3;
    U z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (U)(-7373); z2 *= (U)(-20995);
    z3 = z3 * (U)(-16069) + z5;
    z4 = z4 * (U)(-3196) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const U half = 1u << (shift - 1);
    x[0] = (int32_t)(tmp10 + tmp3 + half) >> shift;
    x[7] = (int32_t)(tmp10 - tmp3 + half) >> shift;
    x[1] = (int32_t)(tmp11 + tmp2 + half) >> shift;
    x[6] = (int32_t)(tmp11 - tmp2 + half) >> shift;
    x[2] = (int32_t)(tmp12 + tmp1 + half) >> shift;
    x[5] = (int32_t)(tmp12 - tmp1 + half) >> shift;
    x[3] = (int32_t)(tmp13 + tmp0 + half) >> shift;
    x[4] = (int32_t)(tmp13 - tmp0 + half) >> shift;
}

// libjpeg's range-limit table behind the IDCT: the low 10 bits as a signed value, + 128, clamped to 0..255
JD_HD int jd_range_limit(int32_t v) {
    int s = v & 1023;
    if (s >= 512) s -= 1024;
    s += 128;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// ---- upsampling and colour (jdsample.c, jdcolor.c) --------------------------------------------------------------------------------------------------------
// the chroma sample at full-resolution (y, x) of a 1 x 1 component beside hs x vs luma; dw x dh = its real down-sampled size
JD_HD int jd_chroma(const uint8_t* p, int stride, int dw, int dh, int hs, int vs, int y, int x) {
    if (hs == 1) return p[(int64_t)y * stride + x];                              // (vs = 1: 4:4:4)
    const int c = x >> 1, r = vs == 2 ? y >> 1 : y;
    if (dw <= 2) return p[(int64_t)r * stride + c];                              // libjpeg leaves fancy upsampling to more than two columns
    int side = (x & 1) ? c + 1 : c - 1;
    side = side < 0 ? 0 : (side > dw - 1 ? dw - 1 : side);
    const uint8_t* near = p + (int64_t)r * stride;
    if (vs == 1) return (3 * near[c] + near[side] + ((x & 1) ? 2 : 1)) >> 2;     // h2v1: biases 1, 2
    int fr = (y & 1) ? r + 1 : r - 1;
    fr = fr < 0 ? 0 : (fr > dh - 1 ? dh - 1 : fr);
    const uint8_t* far = p + (int64_t)fr * stride;
    const int s0 = 3 * near[c] + far[c], s1 = 3 * near[side] + far[side];
    return (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;                               // h2v2: biases 8, 7
}

JD_HD int jd_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

JD_HD void jd_ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128; cr -= 128;
    rgb[0] = (uint8_t)jd_clamp8(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = (uint8_t)jd_clamp8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    rgb[2] = (uint8_t)jd_clamp8(y + ((116130 * cb + 32768) >> 16));
}
