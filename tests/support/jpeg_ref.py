"""numpy restatement of the whole JPEG encoder of csrc/jpeg.hip (include/eg3d_hip.h "Baseline JPEG encoder"): colour conversion, padding,
subsampling, the integer DCT, quantisation, Huffman coding, restart intervals, byte stuffing and the file header.  Independent of the
product: its tables are its own copy of ITU-T T.81 Annex K (tests/test_video_cpu.py checks both against the segments PIL writes), nothing
is imported from inv3d_amd.  The arithmetic is integer only, so the GPU bytes must EQUAL these."""
import struct

import numpy as np

# Annex K.1 / K.2, natural order
K1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
               [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
               [72, 92, 95, 98, 112, 100, 103, 99]], np.int64)
K2 = np.full((8, 8), 99, np.int64)
K2[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# Annex K.3 - K.6 as hex strings: BITS (16 counts), then HUFFVAL
_K3 = ('00010501010101010100000000000000', '000102030405060708090a0b')
_K4 = ('00030101010101010101010000000000', '000102030405060708090a0b')
_K5 = ('0002010303020403050504040000017d',
       '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
       '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
       'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_K6 = ('00020102040403040705040400010277',
       '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a'
       '535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6'
       'c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
DHT = [(cls_id, bytes.fromhex(b), bytes.fromhex(v)) for cls_id, (b, v) in zip((0x00, 0x10, 0x01, 0x11), (_K3, _K5, _K4, _K6))]   # file order


def _zigzag():
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, (n // 8) if (n // 8 + n % 8) % 2 else (n % 8)))
    return np.array(order)


ZZ = _zigzag()                     # zigzag position -> natural index
CI = np.array([[round(8192 * ((1 / 8) ** 0.5 if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)) for x in range(8)] for u in range(8)], np.int64)


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for n in range(16):
        for _ in range(bits[n]):
            out[vals[k]] = (code, n + 1)
            code, k = code + 1, k + 1
        code *= 2
    return out


DC_CODES = [_codes(DHT[0][1], DHT[0][2]), _codes(DHT[2][1], DHT[2][2])]       # [luma, chroma]
AC_CODES = [_codes(DHT[1][1], DHT[1][2]), _codes(DHT[3][1], DHT[3][2])]


def quant_tables(quality):
    """libjpeg: jpeg_quality_scaling, then (base * scale + 50) / 100 clamped to 1..255."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((b * scale + 50) // 100, 1, 255) for b in (K1, K2)]


def quantise_input(x):
    """fp32 in [-1,1] -> uint8 as eg3d_image_grid_u8: float32 product, float32 sum, clamp, truncation."""
    x = np.asarray(x, np.float32)
    return np.clip(x * np.float32(127.5) + np.float32(128.0), np.float32(0), np.float32(255)).astype(np.uint8)


def planes(img_u8, subsampling):
    """uint8 [C,H,W] -> list of (padded plane int64 [h,w], table index), and the MCU size in pixels."""
    c, hh, ww = img_u8.shape
    p = img_u8.astype(np.int64)
    if c == 1:
        comps, mcu = [p[0]], 8
    else:
        r, g, b = p
        comps = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                 (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                 (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16]
        mcu = 16 if subsampling == '420' else 8
    ph, pw = -(-hh // mcu) * mcu, -(-ww // mcu) * mcu
    comps = [np.pad(a, ((0, ph - hh), (0, pw - ww)), mode='edge') for a in comps]
    if c == 3 and subsampling == '420':
        for i in (1, 2):
            a = comps[i]
            comps[i] = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    return [(a, 0 if i == 0 else 1) for i, a in enumerate(comps)], mcu


def dct_unquantised(plane):
    """int64 [h/8, w/8, 8, 8]: D of every 8 x 8 block of a padded plane."""
    h, w = plane.shape
    s = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    t = (np.einsum('uy,abyx->abux', CI, s) + 1024) >> 11
    return (np.einsum('abux,vx->abuv', t, CI) + 16384) >> 15


def quantise(d, q):
    return np.sign(d) * ((np.abs(d) + (q >> 1)) // q)


def coefficients(img_u8, quality, subsampling):
    """Per component: quantised coefficients int64 [bh, bw, 64] in zigzag order."""
    qt = quant_tables(quality)
    comps, mcu = planes(img_u8, subsampling)
    return [quantise(dct_unquantised(a), qt[t]).reshape(a.shape[0] // 8, a.shape[1] // 8, 64)[:, :, ZZ] for a, t in comps], mcu


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self):
        fill = -self.n % 8
        self.put((1 << fill) - 1, fill)
        raw = self.acc.to_bytes(self.n // 8, 'big') if self.n else b''
        return raw.replace(b'\xff', b'\xff\x00')


def _amplitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v - 1) & ((1 << s) - 1)


def _encode_block(bw, zz, pred, t):
    dc = int(zz[0])
    s, amp = _amplitude(dc - pred)
    bw.put(*DC_CODES[t][s])
    bw.put(amp, s)
    last = 0
    for k in np.nonzero(zz[1:])[0] + 1:
        run = int(k) - last - 1
        while run >= 16:
            bw.put(*AC_CODES[t][0xF0])
            run -= 16
        s, amp = _amplitude(int(zz[k]))
        bw.put(*AC_CODES[t][run << 4 | s])
        bw.put(amp, s)
        last = int(k)
    if last < 63:
        bw.put(*AC_CODES[t][0x00])
    return dc


def default_restart(width, subsampling, channels):
    mcu = 16 if (channels == 3 and subsampling == '420') else 8
    return min(-(-width // mcu), 32)


def header(hh, ww, channels, quality, subsampling, restart):
    def seg(marker, payload):
        return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00' + struct.pack('>BBBHHBB', 1, 1, 0, 1, 1, 0, 0))
    for i, q in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in q.reshape(64)[ZZ]))
    comps = [(1, 0x22 if (channels == 3 and subsampling == '420') else 0x11, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [])
    out += seg(0xC0, struct.pack('>BHHB', 8, hh, ww, len(comps)) + b''.join(bytes(c) for c in comps))
    for cls_id, bits, vals in DHT:
        out += seg(0xC4, bytes([cls_id]) + bits + vals)
    out += seg(0xDD, struct.pack('>H', restart))
    out += seg(0xDA, bytes([len(comps)]) + b''.join(bytes([c[0], 0x00 if c[2] == 0 else 0x11]) for c in comps) + bytes([0, 63, 0]))
    return out


def encode(img, quality=90, subsampling='420', restart_interval=None):
    """One JFIF file (bytes) of img [C,H,W], C = 3 | 1, uint8 or fp32 in [-1,1]."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        img = quantise_input(img)
    c, hh, ww = img.shape
    coefs, mcu = coefficients(img, quality, subsampling)
    my, mx = -(-hh // mcu), -(-ww // mcu)
    R = default_restart(ww, subsampling, c) if restart_interval is None else int(restart_interval)
    if c == 1:
        layout = [(0, 0, 0)]                                    # (component, dy, dx) of the blocks of one MCU
    elif mcu == 16:
        layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]
    else:
        layout = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    ysub = 2 if mcu == 16 else 1
    out = [header(hh, ww, c, quality, subsampling, R)]
    nmcu = my * mx
    for iv, start in enumerate(range(0, nmcu, R)):
        bw, pred = _Bits(), [0, 0, 0]
        for m in range(start, min(start + R, nmcu)):
            r, col = divmod(m, mx)
            for comp, dy, dx in layout:
                f = ysub if comp == 0 else 1
                pred[comp] = _encode_block(bw, coefs[comp][r * f + dy, col * f + dx], pred[comp], 0 if comp == 0 else 1)
        out.append(bw.flush())
        out.append(b'\xff' + bytes([0xD0 + iv % 8]) if start + R < nmcu else b'\xff\xd9')
    return b''.join(out)


def encode_batch(imgs, **kw):
    """(bytes, offsets) of N frames back to back, the layout of hipops.jpeg_encode."""
    files = [encode(im, **kw) for im in imgs]
    return b''.join(files), np.cumsum([0] + [len(f) for f in files])
