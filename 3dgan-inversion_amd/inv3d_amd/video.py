"""Media export: the files the reference writes per image next to the numbers.

  jpeg_tables, jpeg_header     <- the constant part of a baseline JFIF file: what hipops.jpeg_encode (csrc/jpeg.hip) puts in front of every
                                  frame's entropy-coded scan; quantisation tables scaled as libjpeg's jpeg_quality_scaling, Annex K Huffman tables
  jpeg_scan_plan               the decoder's side of the format (no reference counterpart): a file's markers parsed into what hipops.jpeg_decode
                                  (csrc/jpeg_decode.hip) needs -- geometry, tables, restart interval, the entropy-coded byte range -- or
                                  JpegUnsupported with the reason
  MjpegAviWriter               <- imageio.get_writer(mp4, mode='I', fps=60, codec='libx264') of gen_interp_video, gen_videos.py:74-146: there
                                  is no video encoder to call, so the container is a Motion-JPEG AVI (RIFF 'AVI ', one 'MJPG' video stream,
                                  'idx1' index) written here, the frames are the GPU encoder's JFIF files
  MjpegAviReader,              no reference counterpart: such files read back -- this project's own, a camera's, ffmpeg's -- `batch` frames per
  read_mjpeg_frames               hipops.jpeg_decode_batch, to PIL's pixels
  write_png                    <- PIL.Image.fromarray(...).save(png), single_id_coach.py:60,83 (zlib only; encoder='gpu': hipops.png_encode)
  png_container, write_pngs    the file around the GPU encoder's zlib streams; N same-size images in one encode
  write_orbit_video            <- gen_interp_video(G, w_pivot, path), single_id_coach.py:61-62,84-85
  write_mesh_video             no reference counterpart: the same orbit of the exported mesh itself (inference.render_mesh), alone or beside the
                                  generator's frame or the density surface
  look_at_small, pivot_grid    <-BaseCoach.forward(ws, needs_img_grid='small', grid_num=5, need_gt_ingrid=(target, cam)) with look_at /
                                  gen_eyes(num='small'), base_coach.py:128-159,216-291

Everything but the rendering and hipops.jpeg_encode / png_encode / image_grid_u8 is host code on the standard library."""
import math
import struct
import zlib
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

# ---- ITU-T T.81 Annex K ------------------------------------------------------------------------------------------------------------------
# K.1 / K.2: quantisation tables in natural (row-major) order
QUANT_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
QUANT_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zigzag position k -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# K.3 - K.6: Huffman tables as (BITS[1..16], HUFFVAL)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
           (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
             (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)
MAX_RESTART_INTERVAL = 32               # EG3D_JPEG_MAX_RESTART: one wave codes an interval out of an LDS bit buffer sized for this many MCUs


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table: canonical codes in order of increasing length (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def jpeg_tables(quality: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(luma, chroma) quantisation tables in natural order for a libjpeg quality 1..100: jpeg_quality_scaling, then
    (base * scale + 50) / 100 clamped to 1..255 (jpeg_add_quant_table with force_baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in (QUANT_LUMA, QUANT_CHROMA))


def default_restart_interval(height: int, width: int, subsampling: str = '420', channels: int = 3) -> int:
    """MCUs per row, capped at MAX_RESTART_INTERVAL."""
    mcu = 16 if (channels == 3 and subsampling == '420') else 8
    return min(-(-int(width) // mcu), MAX_RESTART_INTERVAL)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(height: int, width: int, quality: int = 90, subsampling: str = '420', restart_interval: Optional[int] = None, channels: int = 3) -> bytes:
    """Everything of a baseline JFIF file in front of the entropy-coded data: SOI, APP0 'JFIF' 1.01, two DQT (luma id 0, chroma id 1, zigzag
    order), SOF0, four DHT (DC/AC luma, DC/AC chroma), DRI, SOS.  channels = 1 (grey): one component, the same tables."""
    if subsampling not in ('420', '444') or channels not in (1, 3):
        raise ValueError(f"jpeg_header: subsampling '420' | '444', channels 1 | 3, got {subsampling!r}, {channels}")
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f'jpeg_header: sides 1..65535, got {height} x {width}')
    R = default_restart_interval(height, width, subsampling, channels) if restart_interval is None else int(restart_interval)
    if not 1 <= R <= MAX_RESTART_INTERVAL:
        raise ValueError(f'jpeg_header: restart interval 1..{MAX_RESTART_INTERVAL}, got {R}')
    ql, qc = jpeg_tables(quality)
    h = b'\xff\xd8' + _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for tid, tab in ((0, ql), (1, qc)):
        h += _segment(0xDB, bytes([tid]) + bytes(tab[ZIGZAG[k]] for k in range(64)))
    ysamp = 0x22 if (channels == 3 and subsampling == '420') else 0x11
    comps = [(1, ysamp, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [])
    h += _segment(0xC0, struct.pack('>BHHB', 8, height, width, len(comps)) + b''.join(bytes(c) for c in comps))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN):
        h += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    h += _segment(0xDD, struct.pack('>H', R))
    h += _segment(0xDA, bytes([len(comps)]) + b''.join(bytes([cid, 0x00 if cid == 1 else 0x11]) for cid, _, _ in comps) + b'\x00\x3f\x00')
    return h


# ---- the decoder's side of the format: what hipops.jpeg_decode (csrc/jpeg_decode.hip) needs to know about a file ---------------------------------
class JpegUnsupported(ValueError):
    """A JPEG file outside what the GPU decoder takes (jpeg_scan_plan); the message is the reason."""


class JpegComponent(NamedTuple):
    id: int
    h: int                               # sampling factors
    v: int
    tq: int                              # quantisation table
    td: int                              # DC Huffman table
    ta: int                              # AC Huffman table


class JpegScanPlan(NamedTuple):
    height: int
    width: int
    components: Tuple[JpegComponent, ...]
    quant: Tuple[Optional[Tuple[int, ...]], ...]          # the four tables Tq = 0..3 in natural order, None where the file defines none
    huffman: dict                                         # {(tc, th): (BITS[1..16], HUFFVAL)}, tc 0 = DC, 1 = AC
    restart_interval: int                                 # MCUs, 0 = none
    scan_start: int                                       # data[scan_start:scan_end]: the entropy-coded segment (stuffing and RSTm included),
    scan_end: int                                         # scan_end = the position of EOI's FF

    @property
    def subsampling(self) -> str:
        return {(1, 1): '444', (2, 1): '422', (2, 2): '420'}[(self.components[0].h, self.components[0].v)] if len(self.components) == 3 else 'grey'


JPEG_SAMPLINGS = ((1, 1), (2, 1), (2, 2))               # luma h x v beside 1 x 1 chroma: 4:4:4, 4:2:2, 4:2:0
_SOF_NAMES = {0xC1: 'extended sequential', 0xC2: 'progressive', 0xC3: 'lossless', 0xC5: 'differential sequential', 0xC6: 'differential progressive',
              0xC7: 'differential lossless', 0xC9: 'arithmetic-coded sequential', 0xCA: 'arithmetic-coded progressive', 0xCB: 'arithmetic-coded lossless',
              0xCD: 'arithmetic-coded differential sequential', 0xCE: 'arithmetic-coded differential progressive', 0xCF: 'arithmetic-coded differential lossless'}


def jpeg_scan_plan(data, default_huffman: bool = False) -> JpegScanPlan:
    """Parse a JPEG file's markers (SOI, APPn / COM skipped, DQT, SOF0, DHT, DRI, SOS, EOI) into what the GPU decoder needs.  Taken: 8-bit
    baseline (SOF0), Huffman-coded, one interleaved scan of three components sampled 1x1 / 2x1 / 2x2 beside 1x1 chroma, or one component;
    any legal Huffman tables, any restart interval.  Everything else raises JpegUnsupported with the reason: progressive, extended, 12-bit,
    arithmetic coding, several scans, four components, other sampling factors, 16-bit quantisation tables, an Adobe APP14 segment with
    transform 0 (RGB-coded), a truncated header, a missing EOI.  EXIF orientation is ignored, as PIL's open().convert() ignores it.
    default_huffman=True: a Huffman table a component uses and the file does not define is Annex K's (table 0 the luma one, table 1 the
    chroma one) -- Motion-JPEG frames are commonly written without DHT, and libjpeg-turbo, so PIL, decodes them with these tables."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        raise JpegUnsupported('no SOI marker: not a JPEG file')
    quant, huff = [None] * 4, {}
    frame, restart, adobe_transform, pos = None, 0, None, 2

    def truncated(what):
        return JpegUnsupported(f'truncated header: the file ends inside {what}')
    while True:
        if pos + 2 > n:
            raise truncated('the marker segments (no SOS)')
        if data[pos] != 0xFF:
            raise JpegUnsupported(f'byte {pos}: a marker was expected, found 0x{data[pos]:02x}')
        marker = data[pos + 1]
        if marker == 0xFF:                               # fill byte
            pos += 1
            continue
        if marker == 0xD9:
            raise JpegUnsupported('EOI before any scan')
        if marker == 0x01 or 0xD0 <= marker <= 0xD7:     # stand-alone markers
            pos += 2
            continue
        if pos + 4 > n:
            raise truncated(f'marker 0x{marker:02x}')
        length = struct.unpack_from('>H', data, pos + 2)[0]
        if length < 2 or pos + 2 + length > n:
            raise truncated(f'the segment of marker 0x{marker:02x}')
        seg = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0:
                    raise JpegUnsupported('16-bit quantisation table')
                if tq > 3 or i + 65 > len(seg):
                    raise JpegUnsupported('malformed DQT segment')
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = seg[i + 1 + k]
                quant[tq] = tuple(nat)
                i += 65
        elif marker == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise JpegUnsupported('malformed DHT segment')
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = tuple(seg[i + 1:i + 17])
                count = sum(bits)
                if tc > 1 or th > 3 or count > 256 or i + 17 + count > len(seg):
                    raise JpegUnsupported('malformed DHT segment')
                vals = tuple(seg[i + 17:i + 17 + count])
                code = 0
                for length_ in range(1, 17):             # the codes of every length must fit it, all-ones excluded (libjpeg: bogus Huffman table)
                    code = (code + bits[length_ - 1]) << 1
                    if bits[length_ - 1] and (code >> 1) > (1 << length_) - 1:
                        raise JpegUnsupported('malformed DHT segment: over-subscribed code lengths')
                if tc == 0 and any(v > 15 for v in vals):
                    raise JpegUnsupported('malformed DHT segment: a DC category above 15')
                huff[(tc, th)] = (bits, vals)
                i += 17 + count
        elif marker == 0xC0:
            if frame is not None:
                raise JpegUnsupported('more than one frame header')
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                raise JpegUnsupported('malformed SOF0 segment')
            prec, hh, ww, nc = struct.unpack_from('>BHHB', seg, 0)
            if prec != 8:
                raise JpegUnsupported(f'{prec}-bit samples')
            if hh == 0 or ww == 0:
                raise JpegUnsupported('a frame of height or width 0 (DNL)')
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
            frame = (hh, ww, comps)
        elif marker in _SOF_NAMES:
            raise JpegUnsupported(f'{_SOF_NAMES[marker]} JPEG (SOF{marker - 0xC0}): baseline only')
        elif marker == 0xCC:
            raise JpegUnsupported('arithmetic coding (DAC)')
        elif marker == 0xDD:
            if len(seg) != 2:
                raise JpegUnsupported('malformed DRI segment')
            restart = struct.unpack('>H', seg)[0]
        elif marker == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                adobe_transform = seg[11]
        elif marker == 0xDA:
            break
        # APPn, COM and anything else with a length: skipped
    if frame is None:
        raise JpegUnsupported('SOS before SOF0')
    hh, ww, comps = frame
    if len(comps) not in (1, 3):
        raise JpegUnsupported(f'{len(comps)} components: grey or YCbCr only')
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise JpegUnsupported('malformed SOS segment')
    if seg[0] != len(comps):
        raise JpegUnsupported('several scans (a non-interleaved file)')
    if tuple(seg[1 + 2 * seg[0]:]) != (0, 63, 0):
        raise JpegUnsupported('a scan that is not the full baseline spectrum')
    out = []
    for c, (cid, h, v, tq) in enumerate(comps):
        if seg[1 + 2 * c] != cid:
            raise JpegUnsupported('the scan lists the components in another order than the frame')
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if tq > 3 or quant[tq] is None:
            raise JpegUnsupported(f'component {cid} uses quantisation table {tq}, which the file does not define')
        if td > 1 or ta > 1:
            raise JpegUnsupported(f'component {cid} uses Huffman table {max(td, ta)}: baseline has tables 0 and 1')
        for key in ((0, td), (1, ta)):
            if key not in huff:
                if not default_huffman:
                    raise JpegUnsupported(f'component {cid} uses a Huffman table the file does not define')
                huff[key] = HUFFMAN[2 * key[1] + key[0]]
        out.append(JpegComponent(cid, h, v, tq, td, ta))
    if len(out) == 3:
        if adobe_transform == 0:
            raise JpegUnsupported('Adobe APP14 transform 0: the components are RGB, not YCbCr')
        if adobe_transform is None and tuple(c.id for c in out) == (0x52, 0x47, 0x42):
            raise JpegUnsupported("component ids 'R', 'G', 'B': the components are RGB, not YCbCr")
        if (out[0].h, out[0].v) not in JPEG_SAMPLINGS or (out[1].h, out[1].v, out[2].h, out[2].v) != (1, 1, 1, 1):
            raise JpegUnsupported('sampling factors ' + ' / '.join(f'{c.h}x{c.v}' for c in out) + ': 4:4:4, 4:2:2 and 4:2:0 only')
    else:
        out[0] = out[0]._replace(h=1, v=1)               # one component: the factors mean nothing (T.81 A.2.2), the MCU is one block
    # the entropy-coded segment ends at the first marker that is neither stuffing (FF 00), a restart (FF D0..D7) nor fill (FF FF)
    a = np.frombuffer(data, dtype=np.uint8, offset=pos)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    if ends.size == 0:
        raise JpegUnsupported('missing EOI: the entropy-coded data runs to the end of the file')
    end = pos + int(ends[0])
    if data[end + 1] != 0xD9:
        raise JpegUnsupported(f'marker 0x{data[end + 1]:02x} after the first scan: several scans or tables between them')
    return JpegScanPlan(hh, ww, tuple(out), tuple(quant), huff, restart, pos, end)


# ---- containers ------------------------------------------------------------------------------------------------------------------------------
class MjpegAviWriter:
    """Motion-JPEG AVI 1.0: RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' vids/MJPG, 'strf' BITMAPINFOHEADER } }, LIST 'movi' { '00dc'
    chunks, each padded to an even length }, 'idx1' }.  write() appends one complete JFIF file per frame; close() writes the index and patches
    the RIFF / movi sizes and the frame counts.  One RIFF chunk: files up to 4 GiB."""
    _AVIH, _STRH_LEN, _MOVI = 32, 108 + 32, 212        # offsets of avih's payload, strh's dwLength and the 'movi' LIST header (fixed layout below)

    def __init__(self, path: str, width: int, height: int, fps: int = 60):
        self.path, self.width, self.height, self.fps = path, int(width), int(height), int(fps)
        if self.fps < 1 or self.width < 1 or self.height < 1:
            raise ValueError('MjpegAviWriter: width, height, fps >= 1')
        self._index: List[Tuple[int, int]] = []       # (offset from the 'movi' fourcc, size) per frame
        self._max = 0
        self._f = open(path, 'wb')
        avih = struct.pack('<14I', 1000000 // self.fps, 0, 0, 0x10, 0, 0, 1, 0, self.width, self.height, 0, 0, 0, 0)       # AVIF_HASINDEX
        strh = struct.pack('<4s4sIHHIIIIIIIIhhhh', b'vids', b'MJPG', 0, 0, 0, 0, 1, self.fps, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, b'MJPG', self.width * self.height * 3, 0, 0, 0, 0)
        strl = b'strl' + self._chunk(b'strh', strh) + self._chunk(b'strf', strf)
        hdrl = b'hdrl' + self._chunk(b'avih', avih) + self._chunk(b'LIST', strl)
        head = b'RIFF' + struct.pack('<I', 0) + b'AVI ' + self._chunk(b'LIST', hdrl) + b'LIST' + struct.pack('<I', 0) + b'movi'
        assert len(head) == self._MOVI + 12 and head[self._AVIH - 8:self._AVIH - 4] == b'avih', len(head)
        self._f.write(head)
        self._pos = 4                                  # bytes of the movi LIST payload so far (its fourcc)

    @staticmethod
    def _chunk(fourcc: bytes, payload: bytes) -> bytes:
        return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')

    def write(self, frame_bytes) -> None:
        data = bytes(frame_bytes)
        self._index.append((self._pos, len(data)))
        self._max = max(self._max, len(data))
        self._f.write(self._chunk(b'00dc', data))
        self._pos += 8 + len(data) + (len(data) & 1)

    def close(self) -> None:
        if self._f is None:
            return
        f, n = self._f, len(self._index)
        f.write(b'idx1' + struct.pack('<I', 16 * n) + b''.join(struct.pack('<4sIII', b'00dc', 0x10, off, size) for off, size in self._index))     # AVIIF_KEYFRAME
        end = f.tell()
        f.seek(4)
        f.write(struct.pack('<I', end - 8))
        f.seek(self._AVIH + 4)                         # avih dwMaxBytesPerSec, then dwTotalFrames and dwSuggestedBufferSize
        f.write(struct.pack('<I', self._max * self.fps))
        f.seek(self._AVIH + 16)
        f.write(struct.pack('<I', n))
        f.seek(self._AVIH + 28)
        f.write(struct.pack('<I', self._max))
        f.seek(self._STRH_LEN)
        f.write(struct.pack('<II', n, self._max))      # strh dwLength, dwSuggestedBufferSize
        f.seek(self._MOVI + 4)
        f.write(struct.pack('<I', self._pos))
        f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MjpegAviReader:
    """The reading side of MjpegAviWriter, and of the Motion-JPEG AVI 1.0 files cameras and ffmpeg write: num_frames, fps, width, height,
    frame_bytes(i) (one complete JPEG file), iteration over the frames' bytes, a context manager.  The first video stream is read; chunks of
    other streams (audio) are skipped.  Frames are located by the 'idx1' index where there is one -- its offsets counted from the 'movi'
    fourcc, as MjpegAviWriter and most writers count them, or from the start of the file: whichever lands on the frame's '##dc' / '##db'
    chunk header -- and by walking the 'movi' list ('rec ' lists included, chunks padded to an even length) otherwise.  Refused with a
    ValueError that names the reason: a file that is no RIFF 'AVI ', no video stream, a video stream that is not 'MJPG', OpenDML 'AVIX'
    extensions (files beyond the first RIFF chunk), a zero-length frame chunk (a dropped frame), a chunk or index entry beyond the file."""

    def __init__(self, path: str):
        self.path = path
        self._f = open(path, 'rb')
        try:
            self._parse()
        except Exception:
            self._f.close()
            self._f = None
            raise

    def _read(self, pos: int, n: int) -> bytes:
        self._f.seek(pos)
        return self._f.read(n)

    def _chunks(self, pos: int, end: int):
        """(fourcc, payload position, payload size) of the chunks in [pos, end)"""
        while pos + 8 <= end:
            cc, size = struct.unpack('<4sI', self._read(pos, 8))
            yield cc, pos + 8, size
            pos += 8 + size + (size & 1)

    def _parse(self) -> None:
        size = self._f.seek(0, 2)
        head = self._read(0, 12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'AVI ':
            raise ValueError(f"MjpegAviReader: {self.path} is no RIFF 'AVI ' file")
        riff = struct.unpack('<I', head[4:8])[0]
        riff_end = min(size, 8 + riff + (riff & 1)) if riff else size            # (a size never patched: the file was not closed)
        self._stream, self._rate, self._micro, self._total, self._avih_size, self._strf = None, None, 0, 0, (0, 0), None
        movi, idx1 = None, None
        for cc, at, n in self._chunks(12, riff_end):
            if cc == b'LIST':
                kind = self._read(at, 4)
                if kind == b'hdrl':
                    self._headers(at + 4, min(at + n, size))
                elif kind == b'movi' and movi is None:
                    movi = (at, min(at + n, size))                                 # from the 'movi' fourcc
            elif cc == b'idx1' and idx1 is None:
                idx1 = (at, min(n, size - at))
        for cc, at, n in self._chunks(riff_end, size):
            if cc == b'RIFF' and self._read(at, 4) == b'AVIX':
                raise ValueError(f"MjpegAviReader: {self.path} has OpenDML 'AVIX' extensions, which are not read")
        if self._stream is None:
            raise ValueError(f'MjpegAviReader: {self.path} has no video stream')
        handler, comp, bw, bh = self._strf
        if comp.upper() != b'MJPG' or (handler.upper() != b'MJPG' and handler != bytes(4)):
            raise ValueError(f"MjpegAviReader: the video stream of {self.path} is {comp!r} (handler {handler!r}), not 'MJPG'")
        if movi is None:
            raise ValueError(f"MjpegAviReader: {self.path} has no 'movi' list")
        self.width, self.height = (bw, abs(bh)) if bw > 0 and bh != 0 else self._avih_size
        scale, rate = self._rate
        self.fps = rate / scale if scale > 0 and rate > 0 else (1e6 / self._micro if self._micro > 0 else 0.0)
        ids = (b'%02ddc' % self._stream, b'%02ddb' % self._stream)
        frames = self._from_index(idx1, movi, ids, size) if idx1 is not None else None
        if frames is None:
            frames = []
            self._walk(movi[0] + 4, movi[1], ids, frames)
        for i, (at, n) in enumerate(frames):
            if n == 0:
                raise ValueError(f'MjpegAviReader: frame {i} of {self.path} is a zero-length chunk (a dropped frame)')
            if at + n > size:
                raise ValueError(f'MjpegAviReader: frame {i} of {self.path} lies beyond the end of the file')
        self._frames = frames
        self.num_frames = len(frames)

    def _headers(self, pos: int, end: int) -> None:
        number = 0
        for cc, at, n in self._chunks(pos, end):
            if cc == b'avih' and n >= 40:
                a = struct.unpack('<10I', self._read(at, 40))
                self._micro, self._total, self._avih_size = a[0], a[4], (a[8], a[9])
            elif cc == b'LIST' and self._read(at, 4) == b'strl':
                strh = strf = None
                for c2, at2, n2 in self._chunks(at + 4, at + n):
                    if c2 == b'strh' and n2 >= 36:
                        strh = self._read(at2, 36)
                    elif c2 == b'strf' and n2 >= 20:
                        strf = self._read(at2, 20)
                if self._stream is None and strh is not None and strh[:4] == b'vids' and strf is not None:
                    self._stream = number
                    self._rate = struct.unpack('<II', strh[20:28])
                    bw, bh = struct.unpack('<ii', strf[4:12])
                    self._strf = (strh[4:8], strf[16:20], bw, bh)
                number += 1

    def _from_index(self, idx1, movi, ids, size):
        """[(payload position, size)] from 'idx1', or None where its offsets fit neither convention"""
        raw = self._read(idx1[0], idx1[1] // 16 * 16)
        entries = [e for e in struct.iter_unpack('<4sIII', raw) if e[0] in ids]
        if not entries:
            return None
        cc, _, off, n = entries[0]
        for base in (movi[0], 0):
            if base + off + 8 <= size and self._read(base + off, 8) == cc + struct.pack('<I', n):
                return [(base + o + 8, m) for _, _, o, m in entries]
        return None

    def _walk(self, pos: int, end: int, ids, frames) -> None:
        for cc, at, n in self._chunks(pos, end):
            if cc == b'LIST':
                if self._read(at, 4) == b'rec ':
                    self._walk(at + 4, at + n, ids, frames)
            elif cc in ids:
                frames.append((at, n))

    def frame_bytes(self, i: int) -> bytes:
        if not 0 <= i < self.num_frames:
            raise IndexError(f'MjpegAviReader: frame {i} of {self.num_frames}')
        at, n = self._frames[i]
        return self._read(at, n)

    def __len__(self) -> int:
        return self.num_frames

    def __iter__(self):
        return (self.frame_bytes(i) for i in range(self.num_frames))

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_mjpeg_frames(path: str, start: int = 0, stop: Optional[int] = None, step: int = 1, batch: int = 16, device='cuda', decoder: str = 'gpu',
                      report=None):
    """A generator of (first_index, uint8 [n,H,W,3] on the device) over frames start:stop:step of a Motion-JPEG AVI (MjpegAviReader), n <=
    `batch` frames at a time; frame j of a block is frame first_index + j * step of the file.  decoder='gpu': a block is one
    hipops.jpeg_decode_batch with Annex K's Huffman tables for frames that carry none; a frame the device decoder does not take or refuses
    goes through PIL and report(index, reason), if given, is told -- the rule of images.decode_rgb.  decoder='pil': every frame is decoded
    on the host.  The pixels are PIL.Image.open(frame).convert('RGB') either way.  The frames of one file have one geometry: ValueError
    otherwise."""
    import io
    if decoder not in ('pil', 'gpu') or batch < 1:
        raise ValueError(f"read_mjpeg_frames: decoder 'pil' | 'gpu' and batch >= 1, got {decoder!r}, {batch}")

    def pil(data):
        from PIL import Image
        with Image.open(io.BytesIO(data)) as im:
            return torch.from_numpy(np.array(im.convert('RGB'), dtype=np.uint8)).to(device)
    with MjpegAviReader(path) as reader:
        shape = None
        index = range(reader.num_frames)[slice(start, stop, step)]
        for k in range(0, len(index), batch):
            block = index[k:k + batch]
            files = [reader.frame_bytes(i) for i in block]
            if decoder == 'gpu':
                from .hipops import jpeg_decode_batch
                frames = jpeg_decode_batch(files, device=device, return_errors=True, default_huffman=True)
                for j, f in enumerate(frames):
                    if isinstance(f, Exception):
                        if report is not None:
                            report(block[j], str(f))
                        frames[j] = pil(files[j])
            else:
                frames = [pil(f) for f in files]
            if any(f.shape != frames[0].shape for f in frames) or (shape is not None and frames[0].shape != shape):
                raise ValueError(f'read_mjpeg_frames: the frames of {path} differ in size')
            shape = frames[0].shape
            yield block[0], torch.stack(frames)


def _png_chunk(tag: bytes, payload: bytes) -> bytes:
    return struct.pack('>I', len(payload)) + tag + payload + struct.pack('>I', zlib.crc32(tag + payload) & 0xFFFFFFFF)


def png_container(stream, height: int, width: int, channels: int) -> bytes:
    """The PNG file around one zlib stream of filtered rows: signature, IHDR (8 bits, colour type 0 grey or 2 RGB, no interlace), one IDAT,
    IEND; the chunk CRCs are zlib.crc32 on the host."""
    if channels not in (1, 3) or not (1 <= height < 2 ** 31 and 1 <= width < 2 ** 31):
        raise ValueError(f'png_container: channels 1 | 3 and sides >= 1, got {height} x {width} x {channels}')
    return (b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)) +
            _png_chunk(b'IDAT', bytes(stream)) + _png_chunk(b'IEND', b''))


PNG_ENCODERS = ('host', 'gpu')


def write_png(path: str, u8_hwc, encoder: str = 'host') -> None:
    """8-bit PNG of a uint8 [H,W,3] (RGB) or [H,W] / [H,W,1] (grey) array.  encoder='host': IHDR, one IDAT (filter 0 rows, zlib level 6), IEND.
    encoder='gpu': the rows are filtered and deflated on the device (hipops.png_encode: adaptive filters, run-length deflate; a CPU tensor or an
    array is uploaded), the host adds the container."""
    if encoder not in PNG_ENCODERS:
        raise ValueError(f'write_png: encoder one of {PNG_ENCODERS}, got {encoder!r}')
    if encoder == 'gpu':
        a = u8_hwc if isinstance(u8_hwc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(u8_hwc))
        if a.dtype != torch.uint8 or a.dim() not in (2, 3) or (a.dim() == 3 and a.shape[2] not in (1, 3)) or min(a.shape) < 1:
            raise ValueError(f'write_png: uint8 [H,W,3] or [H,W], got {a.dtype} {tuple(a.shape)}')
        write_pngs([path], a[None])
        return
    a = u8_hwc.detach().cpu().numpy() if isinstance(u8_hwc, torch.Tensor) else np.asarray(u8_hwc)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'write_png: uint8 [H,W,3] or [H,W], got {a.dtype} {a.shape}')
    hh, ww, ch = a.shape
    rows = np.zeros((hh, 1 + ww * ch), np.uint8)
    rows[:, 1:] = a.reshape(hh, ww * ch)

    def chunk(tag, payload):
        return struct.pack('>I', len(payload)) + tag + payload + struct.pack('>I', zlib.crc32(tag + payload) & 0xFFFFFFFF)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', ww, hh, 8, 2 if ch == 3 else 0, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def write_pngs(paths, batch, filter='adaptive', block_bytes: int = 32768) -> None:
    """len(paths) PNG files of a uint8 batch [N,H,W,3], [N,H,W,1] or [N,H,W] (a tensor on any device or an array) through one
    hipops.png_encode: one encode, one device-to-host copy, then container and file per image."""
    from .hipops import png_encode
    a = batch if isinstance(batch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch))
    if a.dim() == 3:
        a = a[..., None]
    if a.dtype != torch.uint8 or a.dim() != 4 or a.shape[3] not in (1, 3) or min(a.shape) < 1 or a.shape[0] != len(paths):
        raise ValueError(f'write_pngs: uint8 [N,H,W,3] or [N,H,W] with N = {len(paths)} paths, got {a.dtype} {tuple(a.shape)}')
    if not a.is_cuda:
        a = a.cuda()
    data, offsets = png_encode(a.detach(), filter=filter, block_bytes=block_bytes)
    host, off = data.cpu().numpy(), offsets.tolist()
    for i, path in enumerate(paths):
        with open(path, 'wb') as f:
            f.write(png_container(host[off[i]:off[i + 1]].tobytes(), a.shape[1], a.shape[2], a.shape[3]))


# ---- the per-image outputs -----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def write_orbit_video(G, ws: torch.Tensor, path: str, num_frames: int = 240, image_mode: str = 'image', fps: int = 60, quality: int = 90,
                      batch: int = 16, shape: bool = False, shape_kwargs: Optional[dict] = None, paste=None, paste_kwargs: Optional[dict] = None,
                      **synthesis_kwargs) -> int:
    """gen_interp_video for one latent: inference.render_orbit's frames, `batch` at a time through hipops.jpeg_encode (4:2:0; grey for
    image_depth), one device-to-host copy per batch, into a Motion-JPEG AVI at `path`.  Returns the number of frames written.
    shape=True (no reference counterpart): every frame is image | shape side by side, twice the width -- the shaded first-hit view of the
    density surface from the same camera at the frame's resolution (inference.render_shape; shape_kwargs: grid_res, level, shade, keep,
    min_voxels, connectivity, ...).  The density grid and its brick maxima are built once per video, and so is inference.clean_grid's pass.  With shape=False the file is what it was before the option existed.
    paste=(photo uint8 [H,W,3] on the device, landmarks 68 x 2) (no reference counterpart): every frame is blended back into the photograph
    the latent was inverted from (images.paste_back, `batch` frames per call, planar output straight into the encoder) and the video shows
    the photo, by default the face's bounding box in it (paste_kwargs: region='photo' for the whole photograph, feather, mask, bands=1..6 |
    'auto' for the multi-band blend -- with the matte too).  Colour frames
    only, and not together with shape.  With paste=None the file is what it was before the option existed.
    paste_kwargs=dict(matte=True | {images.matte_from_mask's keywords}): every frame is pasted through its own head matte, made from the
    depth of the frame's own render (images.head_matte(depth=...): no second render, no host synchronise), so the photograph's background
    stays around the head.  Without `matte` the file is what it was before that option existed."""
    from .hipops import jpeg_encode
    from .inference import clean_grid, density_grid, orbit_cameras, render_orbit, render_shape
    if batch < 1:
        raise ValueError('write_orbit_video: batch >= 1')
    if paste is not None and (shape or image_mode != 'image'):
        raise ValueError("write_orbit_video: paste takes the colour frames alone (image_mode='image', shape=False)")
    writer, pending, depths, n = None, [], [], 0
    pkw = dict(paste_kwargs or {})
    matte = pkw.pop('matte', False) if paste is not None else False       # True | matte_kwargs: one matte per frame from that frame's own depth
    if matte and 'mask' in pkw:
        raise ValueError('write_orbit_video: paste_kwargs takes matte or mask, not both')
    if shape:
        skw = dict(shape_kwargs or {})
        cams = synthesis_kwargs.get('cameras')
        cams = orbit_cameras(num_frames, device=ws.device) if cams is None else cams.to(ws.device)
        # before the first frame: the grid runs the backbone, and render_orbit keeps the planes of its first frame for the later ones
        grid = skw.pop('grid', None)
        state = dict(grid=density_grid(G, ws, res=skw.get('grid_res', 512)) if grid is None else grid, bricks=skw.pop('bricks', None))
        clean = {k: skw.pop(k) for k in ('keep', 'min_voxels', 'connectivity') if k in skw}      # floater removal: once per video, not per frame
        if clean.get('keep') is not None or int(clean.get('min_voxels', 0)) > 0:
            state['grid'] = clean_grid(state['grid'], skw.get('level', 10.0), **clean)[0]

    def beside(i, frame):
        out = render_shape(G, ws, cams[i:i + 1], res=frame.shape[-1], grid=state['grid'], bricks=state['bricks'], **skw)
        state['bricks'] = out['bricks']
        return torch.cat([frame, out['shade'][0, :frame.shape[0]]], dim=-1)

    def flush():
        nonlocal writer, n
        frames = torch.stack(pending)
        if paste is not None:
            from .images import head_matte, paste_back
            kw = dict(dict(region='bbox'), **pkw)
            if matte:
                kw['mask'] = head_matte(G, ws, None, size=frames.shape[-1], depth=torch.stack(depths), **(matte if isinstance(matte, dict) else {}))
                depths.clear()
            frames = paste_back(paste[0], frames, paste[1], layout='chw', **kw)
        data, offsets = jpeg_encode(frames, quality=quality)
        host, off = data.cpu().numpy(), offsets.tolist()                 # (offsets are already on the host: one copy, the bytes)
        if writer is None:
            writer = MjpegAviWriter(path, frames.shape[-1], frames.shape[-2], fps=fps)
        for i in range(len(pending)):
            writer.write(host[off[i]:off[i + 1]].tobytes())
        n += len(pending)
        pending.clear()
    try:
        for i, frame in enumerate(render_orbit(G, ws, num_frames=num_frames, image_mode=image_mode, with_depth=bool(matte), **synthesis_kwargs)):
            if matte:
                frame, depth = frame
                depths.append(depth.float().clone())
            pending.append(beside(i, frame.float()) if shape else frame.float().clone())      # (the frame may be a view of a buffer the next render reuses)
            if len(pending) == batch:
                flush()
        if pending:
            flush()
    finally:
        if writer is not None:
            writer.close()
    return n


@torch.no_grad()
def write_mesh_video(G, mesh: dict, path: str, num_frames: int = 240, beside: Optional[str] = None, ws: Optional[torch.Tensor] = None, fps: int = 60,
                     quality: int = 90, batch: int = 16, cameras: Optional[torch.Tensor] = None, shape_kwargs: Optional[dict] = None,
                     synthesis_kwargs: Optional[dict] = None, **render_kwargs) -> int:
    """An orbit of the exported mesh as a Motion-JPEG AVI at `path` (no reference counterpart): inference.render_mesh_orbit's frames through
    the batching, encoder and container of write_orbit_video.  `mesh` holds what render_mesh takes: verts, faces, grid_res, and uv + texture
    (mode 'texture', the default when both are there), colors or normals; render_kwargs (mode, res, supersample, cull, background, ...) go to
    render_mesh.  beside='image': every frame is generator | mesh, twice the width (G.synthesis of `ws` from the same camera; the mesh is drawn
    at the image's resolution);  beside='shape': density surface | mesh (inference.render_shape of `ws`; shape_kwargs: grid, grid_res, level,
    ...; the grid is built once).  Returns the number of frames written."""
    from .hipops import jpeg_encode
    from .inference import density_grid, orbit_cameras, render_mesh, render_shape
    if beside not in (None, 'image', 'shape'):
        raise ValueError(f"write_mesh_video: beside None, 'image' or 'shape', got {beside!r}")
    if int(num_frames) < 1 or batch < 1:
        raise ValueError('write_mesh_video: num_frames >= 1 and batch >= 1')
    if beside is not None and ws is None:
        raise ValueError(f'write_mesh_video: beside={beside!r} needs the latent ws')
    verts, faces = mesh['verts'], mesh['faces']
    dev = verts.device
    kw = dict(render_kwargs)
    kw.setdefault('mode', 'texture' if mesh.get('uv') is not None and mesh.get('texture') is not None else ('vertex' if mesh.get('colors') is not None else 'lambert'))
    for k in ('uv', 'texture', 'colors', 'normals', 'grid_res'):
        if mesh.get(k) is not None:
            kw.setdefault(k, mesh[k])
    cams = orbit_cameras(int(num_frames), device=dev) if cameras is None else cameras.to(dev)
    skw, state = dict(shape_kwargs or {}), {}
    if beside == 'shape':
        grid = skw.pop('grid', None)
        state = dict(grid=density_grid(G, ws, res=skw.pop('grid_res', 512)) if grid is None else grid, bricks=skw.pop('bricks', None))
    gkw = dict(noise_mode='const', **(synthesis_kwargs or {}))
    writer, pending, n = None, [], 0

    def flush():
        nonlocal writer, n
        frames = torch.stack(pending)
        data, offsets = jpeg_encode(frames, quality=quality)
        host, off = data.cpu().numpy(), offsets.tolist()
        if writer is None:
            writer = MjpegAviWriter(path, frames.shape[-1], frames.shape[-2], fps=fps)
        for i in range(len(pending)):
            writer.write(host[off[i]:off[i + 1]].tobytes())
        n += len(pending)
        pending.clear()
    try:
        for i in range(cams.shape[0]):
            c = cams[i:i + 1]
            left = None
            if beside == 'image':
                left = G.synthesis(ws[:1], c, cache_backbone=(i == 0), use_cached_backbone=(i > 0), **gkw)['image'][0].float()
                kw['res'] = left.shape[-1]
            frame = render_mesh(G, verts, faces, c, **kw)['image'][0]
            if beside == 'shape':
                out = render_shape(G, ws, c, res=frame.shape[-1], grid=state['grid'], bricks=state['bricks'], **skw)
                state['bricks'] = out['bricks']
                left = out['shade'][0]
            pending.append(frame if left is None else torch.cat([left, frame], dim=-1))
            if len(pending) == batch:
                flush()
        if pending:
            flush()
    finally:
        if writer is not None:
            writer.close()
    return n


def small_eyes(coeff: int = 8) -> List[Tuple[float, float, float]]:
    """gen_eyes(num='small'), base_coach.py:252-271: right, centre, left on the unit circle of the x-y plane, pi / coeff off the y axis."""
    x, y = math.sin(math.pi / coeff), math.cos(math.pi / coeff)
    return [(x, y, 0.0), (0.0, 1.0, 0.0), (-x, y, 0.0)]


def look_at_small(radius: float = 2.7) -> torch.Tensor:
    """look_at(num='small'), base_coach.py:216-249: fp32 [3,16] cam2world matrices (row-major 4 x 4) of the right / centre / left views.
    Per eye: z = eye, x = up x z normalised (up = (0,0,1)), y = z x x normalised, M = [x y z] as columns; the EG3D convention is the rows
    (-M0, -M2, -M1), and the camera sits at -radius times that matrix's third column."""
    up = torch.tensor([0., 0., 1.])
    mats = []
    for eye in small_eyes():
        z_axis = torch.tensor(eye, dtype=torch.float32)
        x_axis = torch.linalg.cross(up, z_axis)
        x_axis = x_axis / torch.norm(x_axis)
        y_axis = torch.linalg.cross(z_axis, x_axis)
        y_axis = y_axis / torch.norm(y_axis)
        mat = torch.stack([x_axis, y_axis, z_axis], dim=-1)
        rot = torch.stack([-mat[0], -mat[2], -mat[1]], dim=0)
        loc = -rot[:, 2] * radius
        mats.append(torch.cat([torch.cat([rot, loc.unsqueeze(1)], dim=1).reshape(12), torch.tensor([0., 0., 0., 1.])]))
    return torch.stack(mats)


@torch.no_grad()
def pivot_grid(G, ws: torch.Tensor, cam: torch.Tensor, target: torch.Tensor, shape: bool = False, shape_kwargs: Optional[dict] = None,
               **synthesis_kwargs) -> torch.Tensor:
    """uint8 [H',W',3] on the device: the reference's forward(ws, needs_img_grid='small', grid_num=5, need_gt_ingrid=(target, cam)) after its
    (grid * 127.5 + 128).clamp(0, 255).to(uint8): target, the render at `cam`, and the right / centre / left look_at views, one row of five
    tiled as make_grid(nrow=5, padding=2) (hipops.image_grid_u8; make_grid's float padding 0 is the grey 128 here).
    Rendered with noise_mode='const': the reference calls G.synthesis with its default 'random', which would make the file differ from run
    to run; everything else (full ws, intrinsics 4.2647 / 0.5) is the reference's.  The renderer's stratified-sampling draws are still random
    unless render_uniforms=(u1, u2) is among the synthesis kwargs.
    shape=True (no reference counterpart) adds a second row: under each of the four renders the shaded first-hit view of the density surface
    from the same camera (inference.render_shape at the render's resolution; shape_kwargs: grid_res, level, shade, background, ...), under the
    target a cell of the background value.  The first row is the shape=False grid."""
    from .hipops import image_grid_u8
    from .inference import render_shape
    dev = ws.device
    K = torch.tensor([4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1.])
    cams = [cam[:1].to(dev).float()] + [torch.cat([m, K]).unsqueeze(0).to(dev) for m in look_at_small()]
    kw = dict(noise_mode='const', **synthesis_kwargs)
    images = [target[:1].to(dev).float()]
    for i, c in enumerate(cams):
        images.append(G.synthesis(ws[:1], c, cache_backbone=(i == 0), use_cached_backbone=(i > 0), **kw)['image'].float())
    if shape:
        skw = dict(shape_kwargs or {})
        views = render_shape(G, ws, torch.cat(cams, 0), res=images[1].shape[-1], **skw)['shade']
        images += [torch.full_like(views[:1], float(skw.get('background', 1.0))), views]
    return image_grid_u8(torch.cat(images, 0), nrow=5, padding=2, pad_value=128)
