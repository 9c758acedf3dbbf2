"""numpy restatement of the baseline JPEG decoder (csrc/jpeg_decode.hip; include/eg3d_hip.h "Baseline JPEG decoder"): a video.jpeg_scan_plan and
the file's bytes -> uint8 [H,W,3], integer arithmetic only, written for clarity.  The stages are the device's -- marker pass, Huffman decode, DC
prediction, dequantisation and libjpeg's jidctint ISLOW inverse DCT, libjpeg-turbo's fancy h2v1 / h2v2 upsampling, libjpeg's YCbCr -> RGB -- but
the entropy decode here is the plain sequential one: the device's self-synchronising decode must give the same coefficients.

DecodeError carries the device's status bits for streams the device refuses."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
from inv3d_amd import video as V  # noqa: E402

ERR_MARKER, ERR_SEGMENTS, ERR_BLOCKS, ERR_CODE = 1, 2, 4, 8          # EG3D_JPEGDEC_ERR_*


class DecodeError(ValueError):
    def __init__(self, status, what):
        super().__init__(f'status {status}: {what}')
        self.status = status


# ---- marker pass ------------------------------------------------------------------------------------------------------------------------------------
def unstuff(raw):
    """(unstuffed bytes, [segment start, ..., total] in unstuffed bytes): FF 00 -> FF, FF D0..D7 removed and a new restart segment begun; any
    other FF xx, a trailing FF, or RSTm out of sequence is an error."""
    out, starts, i, n = bytearray(), [0], 0, len(raw)
    while i < n:
        b = raw[i]
        if b != 0xFF:
            out.append(b)
            i += 1
            continue
        nxt = raw[i + 1] if i + 1 < n else -1
        if nxt == 0:
            out.append(0xFF)
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != (len(starts) - 1) & 7:
                raise DecodeError(ERR_SEGMENTS, f'RST{nxt - 0xD0} where RST{(len(starts) - 1) & 7} was due')
            starts.append(len(out))
        else:
            raise DecodeError(ERR_MARKER, f'FF {nxt:02x} inside the entropy-coded segment')
        i += 2
    return bytes(out), starts + [len(out)]


# ---- Huffman decode ---------------------------------------------------------------------------------------------------------------------------------
def decode_tables(bits, vals):
    """(maxcode[1..16] (-1: no code of that length), valoff[1..16]) as libjpeg's jdhuff builds them: a code of length l is the smallest l whose
    l-bit prefix is <= maxcode[l]; its symbol is vals[prefix + valoff[l]]."""
    maxcode, valoff, code, p = [-1] * 17, [0] * 17, 0, 0
    for length in range(1, 17):
        if bits[length - 1]:
            valoff[length] = p - code
            p += bits[length - 1]
            code += bits[length - 1]
            maxcode[length] = code - 1
        code <<= 1
    return maxcode, valoff


class BitReader:
    """MSB-first bits of one restart segment; bits beyond its end read as zero, and a symbol that does not fit the segment ends the decode."""

    def __init__(self, data, begin, end):
        self.d = data[begin:end]
        self.n = (end - begin) * 8
        self.p = 0

    def peek(self, count):
        """`count` <= 32 bits at the position, zero-extended beyond the end"""
        i = self.p >> 3
        chunk = int.from_bytes(self.d[i:i + 5].ljust(5, b'\0'), 'big')
        return (chunk >> (40 - (self.p & 7) - count)) & ((1 << count) - 1)


def _symbol(reader, table):
    """(symbol, code length) at the reader's position, (None, 16) where no code of the table matches"""
    maxcode, valoff, vals = table
    window = reader.peek(16)
    for length in range(1, 17):
        code = window >> (16 - length)
        if code <= maxcode[length]:
            return vals[(code + valoff[length]) & 255], length
    return None, 16


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def decode_coefficients(plan, data):
    """int32 [blocks, 64] in natural order, scan (MCU-interleaved) order, the DC terms already predicted (summed per component within every
    restart segment)."""
    comps = plan.components
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    mx, my = -(-plan.width // (8 * hmax)), -(-plan.height // (8 * vmax))
    comp_of = [ci for ci, c in enumerate(comps) for _ in range(c.h * c.v)]
    bpm, mcus = len(comp_of), mx * my
    R = plan.restart_interval or mcus
    nseg = -(-mcus // R)
    stream, starts = unstuff(data[plan.scan_start:plan.scan_end])
    if len(starts) - 1 != nseg:
        raise DecodeError(ERR_SEGMENTS, f'{len(starts) - 1} restart segments where the geometry has {nseg}')
    tables = {key: decode_tables(*bv) + (tuple(bv[1]) + (0,) * (256 - len(bv[1])),) for key, bv in plan.huffman.items()}
    coef = np.zeros((mcus * bpm, 64), np.int32)
    for s in range(nseg):
        rd = BitReader(stream, starts[s], starts[s + 1])
        pred = [0] * len(comps)
        first, count = s * R * bpm, min(R, mcus - s * R) * bpm
        for blk in range(first, first + count):
            c = comps[comp_of[(blk - first) % bpm]]
            k = 0
            while k < 64:
                sym, length = _symbol(rd, tables[(0 if k == 0 else 1, c.td if k == 0 else c.ta)])
                size = (sym or 0) & 15
                if rd.p + length + size > rd.n:
                    raise DecodeError(ERR_BLOCKS, f'restart segment {s} ends inside block {blk - first} of {count}')
                if sym is None:
                    raise DecodeError(ERR_CODE, f'no Huffman code matches in restart segment {s}')
                value = _extend(rd.peek(length + size) & ((1 << size) - 1), size) if size else 0
                rd.p += length + size
                if k == 0:
                    pred[comp_of[(blk - first) % bpm]] += value
                    coef[blk, 0] = pred[comp_of[(blk - first) % bpm]]
                    k = 1
                elif size == 0:
                    k = k + 16 if sym >> 4 == 15 else 64            # ZRL, or end of block (as libjpeg: any other run with size 0 ends the block)
                else:
                    k += sym >> 4
                    if k > 63:
                        raise DecodeError(ERR_CODE, f'a run past coefficient 63 in restart segment {s}')
                    coef[blk, V.ZIGZAG[k]] = value
                    k += 1
        # what is left must be the filler alone: no further symbol fits the segment
        sym, length = _symbol(rd, tables[(0, comps[0].td)])
        if sym is not None and rd.p + length + (sym & 15) <= rd.n:
            raise DecodeError(ERR_BLOCKS, f'restart segment {s} holds more than its {count} blocks')
    return coef, (mx, my, comp_of)


# ---- inverse DCT ------------------------------------------------------------------------------------------------------------------------------------
def _idct_1d(x, shift):
    """jidctint.c jpeg_idct_islow's one-dimensional pass over the leading axis of int32 x [8, ...]: CONST_BITS = 13; the result descaled by
    `shift` with rounding.  32-bit wrap-around arithmetic, as the device's (no difference for coefficients any encoder writes)."""
    i32 = np.int32
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * i32(4433)
    tmp2 = z1 + z3 * i32(-15137)
    tmp3 = z1 + z2 * i32(6270)
    tmp0 = (x[0] + x[4]) << i32(13)
    tmp1 = (x[0] - x[4]) << i32(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * i32(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * i32(2446), tmp1 * i32(16819), tmp2 * i32(25172), tmp3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = i32(1 << (shift - 1))
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + half) >> i32(shift) for o in out])


def idct_blocks(coef, quant):
    """uint8 [n, 8, 8]: coef int32 [n, 64] (natural order) times quant [64], columns (descale 11) then rows (descale 18), & 1023, libjpeg's
    range-limit table centred on 128 (the 10-bit value taken as signed, + 128, clamped to 0..255)."""
    with np.errstate(over='ignore'):
        d = (coef.astype(np.int32) * np.asarray(quant, np.int32)[None]).reshape(-1, 8, 8)
        ws = _idct_1d(d.transpose(1, 0, 2), 11)                    # [row, n, col] -> over rows = the column pass; result [row', n, col]
        out = _idct_1d(ws.transpose(2, 1, 0), 18)                  # [col, n, row'] -> over columns = the row pass; result [col', n, row']
    v = out.transpose(1, 2, 0) & 1023
    v = np.where(v >= 512, v - 1024, v) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def component_planes(plan, coef, layout):
    """One uint8 plane per component, padded to whole MCUs."""
    mx, my, comp_of = layout
    comps, bpm = plan.components, len(comp_of)
    planes = []
    for ci, c in enumerate(comps):
        px = idct_blocks(coef.reshape(my, mx, bpm, 64)[:, :, [b for b in range(bpm) if comp_of[b] == ci]].reshape(-1, 64), plan.quant[c.tq])
        px = px.reshape(my, mx, c.v, c.h, 8, 8).transpose(0, 2, 4, 1, 3, 5)          # my, v, row, mx, h, col
        planes.append(px.reshape(my * c.v * 8, mx * c.h * 8))
    return planes


# ---- upsampling and colour ----------------------------------------------------------------------------------------------------------------------------
def upsample(plane, h, v, height, width):
    """jdsample.c for a 1 x 1 component beside h x v luma: [height, width] int32 from the padded plane.  The real down-sampled size is
    ceil(width / h) x ceil(height / v); neighbours are clamped to it.  h = 2 with more than two real columns: fancy (triangle) upsampling --
    h2v1: (3 a + left + 1) >> 2 for even columns, (3 a + right + 2) >> 2 for odd ones; h2v2: with s = 3 near row + far row (the far row is
    the one above for even output rows, below for odd ones), (3 s + s_left + 8) >> 4 and (3 s + s_right + 7) >> 4.  Otherwise replication."""
    dw, dh = -(-width // h), -(-height // v)
    p = plane[:dh, :dw].astype(np.int32)
    y, x = np.arange(height), np.arange(width)
    if h == 1 and v == 1:
        return p
    if dw <= 2:
        return p[(y // v)[:, None], (x // h)[None]]
    c = x // 2
    side = np.clip(np.where(x & 1, c + 1, c - 1), 0, dw - 1)
    if v == 1:
        return (3 * p[:, c] + p[:, side] + np.where(x & 1, 2, 1)[None]) >> 2
    r = y // 2
    far = np.clip(np.where(y & 1, r + 1, r - 1), 0, dh - 1)
    s = 3 * p[r] + p[far]                                                            # [height, dw]
    return (3 * s[:, c] + s[:, side] + np.where(x & 1, 7, 8)[None]) >> 4


def ycc_to_rgb(yy, cb, cr):
    """jdcolor.c: 16-bit fixed-point constants, the red and blue terms rounded on their own, the two green terms rounded together; clamped."""
    cb, cr = cb - 128, cr - 128
    r = yy + ((91881 * cr + 32768) >> 16)
    g = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = yy + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, plan=None):
    """uint8 [H,W,3]: what PIL.Image.open(file).convert('RGB') gives for a file jpeg_scan_plan takes."""
    data = bytes(data)
    plan = V.jpeg_scan_plan(data) if plan is None else plan
    coef, layout = decode_coefficients(plan, data)
    planes = component_planes(plan, coef, layout)
    hh, ww = plan.height, plan.width
    yy = planes[0][:hh, :ww].astype(np.int32)
    if len(planes) == 1:
        return np.repeat(yy.astype(np.uint8)[:, :, None], 3, 2)
    h, v = plan.components[0].h, plan.components[0].v
    return ycc_to_rgb(yy, upsample(planes[1], h, v, hh, ww), upsample(planes[2], h, v, hh, ww))
