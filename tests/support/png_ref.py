"""numpy restatement of the PNG encoder (csrc/png.hip; include/eg3d_hip.h "PNG encoder"): integers only, so the device bytes must EQUAL these.

  filtered_stream   PNG 1.2 section 6 row filters (None, Sub, Up, Average, Paeth), adaptive = the smallest sum of |int8(byte)|, ties to the lower type
  tokens            per block of block_bytes: maximal runs of equal bytes -> literal, matches of 258 at distance 1, a rest of >= 3 as one match
  code_lengths      two-queue Huffman merge over the used symbols sorted by (count, symbol), ties to the leaf queue, then miniz's Kraft fix-up
                    for the length limit and lengths handed out by sorted position (the most frequent symbol gets the shortest code)
  encode            one zlib stream: 78 01, dynamic-Huffman blocks (all 19 code-length code lengths sent, no repeat codes 16 / 17 / 18, one
                    distance code), an empty stored block after every block but the last, Adler-32 from per-block partials
"""
import struct

import numpy as np

MAX_BITS, MAX_CL_BITS = 15, 7
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
ADLER = 65521


def image(h, w, seed, sigma):
    """The synthetic photograph-like test image: smooth colour gradients plus Gaussian noise of standard deviation sigma."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(x / 17 + y / 23), 100 + 60 * np.cos(x / 11), 90 + y * 160 / h], -1)
    return np.clip(base + np.random.RandomState(seed).normal(0, sigma, base.shape) if sigma > 0 else base, 0, 255).astype(np.uint8)


def half_flat():
    a = image(128, 128, 3, 2)
    a[:, 64:] = 255
    return a


def as_hwc(img):
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] in (1, 3) and a.shape[0] >= 1 and a.shape[1] >= 1, (a.dtype, a.shape)
    return a


def filtered_stream(img, filt=-1):
    """(stream bytes of H rows [type][W * C bytes], the H types)."""
    a = as_hwc(img)
    hh, ww, bpp = a.shape
    raw = a.reshape(hh, ww * bpp).astype(np.int32)
    prev = np.zeros(ww * bpp, np.int32)
    out, types = np.zeros((hh, 1 + ww * bpp), np.uint8), []
    for y in range(hh):
        x = raw[y]
        left = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        p = left + prev - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        cands = [(x - q) & 255 for q in (0, left, prev, (left + prev) >> 1, paeth)]
        if filt == -1:
            t = int(np.argmin([int(np.where(v < 128, v, 256 - v).sum()) for v in cands]))        # the first minimum: ties to the lower type
        else:
            t = int(filt)
        types.append(t)
        out[y, 0], out[y, 1:] = t, cands[t]
        prev = x
    return out.tobytes(), types


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258."""
    i = max(k for k in range(29) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def tokens(block):
    """[(symbol, extra bits, extra value)] of one block, end-of-block included; a symbol >= 257 is a match at distance 1."""
    b = np.frombuffer(block, np.uint8)
    starts = np.concatenate([[0], np.nonzero(b[1:] != b[:-1])[0] + 1, [len(b)]])
    out = []
    for s, e in zip(starts[:-1], starts[1:]):
        v, m = int(b[s]), int(e - s) - 1
        out.append((v, 0, 0))
        out += [(285, 0, 0)] * (m // 258)
        q = m % 258
        out += [length_symbol(q)] if q >= 3 else [(v, 0, 0)] * q
    out.append((256, 0, 0))
    return out


def huffman_depths(counts):
    """{symbol: depth} of the unrestricted two-queue Huffman tree over the used symbols (at least two)."""
    syms = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    n = len(syms)
    assert n >= 2
    w, parent = [counts[s] for s in syms] + [0] * (n - 1), [0] * (2 * n - 1)
    state = dict(leaf=0, inode=n)
    for nxt in range(n, 2 * n - 1):
        def pick():
            if state['leaf'] < n and (state['inode'] >= nxt or w[state['leaf']] <= w[state['inode']]):       # a tie goes to the leaf
                state['leaf'] += 1
                return state['leaf'] - 1
            state['inode'] += 1
            return state['inode'] - 1
        a = pick()
        b = pick()
        w[nxt], parent[a], parent[b] = w[a] + w[b], nxt, nxt
    depth = [0] * (2 * n - 1)
    for j in range(2 * n - 3, -1, -1):
        depth[j] = depth[parent[j]] + 1
    return {syms[i]: depth[i] for i in range(n)}, syms


def code_lengths(counts, limit):
    """Code length per symbol (0 = unused): huffman_depths, the number of codes per depth, miniz's tdefl_huffman_enforce_max_code_size, and
    the lengths handed out along the (count, symbol) order from its far end."""
    depths, syms = huffman_depths(counts)
    num = [0] * 64
    for d in depths.values():
        num[d] += 1
    for d in range(limit + 1, 64):
        num[limit] += num[d]
        num[d] = 0
    total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
    while total != 1 << limit:
        num[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    lens, j = [0] * len(counts), len(syms)
    for i in range(1, limit + 1):
        for _ in range(num[i]):
            j -= 1
            lens[syms[j]] = i
    assert j == 0
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2: code per symbol, most significant bit first."""
    mx = max(lens)
    bl = [0] * (mx + 2)
    for v in lens:
        if v:
            bl[v] += 1
    nxt, code = [0] * (mx + 2), 0
    for bits in range(1, mx + 1):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = nxt[v]
            nxt[v] += 1
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):                                        # least significant bit first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):                                        # a Huffman code: most significant bit first
        self.bits(int(format(code, f'0{length}b')[::-1], 2) if length else 0, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def block_plan(block):
    """Everything the coder decides for one block: tokens, the two count tables, lengths, codes."""
    toks = tokens(block)
    lit = [0] * 286
    for s, _, _ in toks:
        lit[s] += 1
    nlit = max(s for s in range(286) if lit[s]) + 1                      # >= 257: end-of-block is always used
    lit_len = code_lengths(lit, MAX_BITS)
    dist_len = 1 if any(s > 256 for s, _, _ in toks) else 0
    seq = lit_len[:nlit] + [dist_len]
    cl = [0] * 19
    for v in seq:
        cl[v] += 1
    cl_len = code_lengths(cl, MAX_CL_BITS)
    return dict(tokens=toks, lit=lit, nlit=nlit, lit_len=lit_len, dist_len=dist_len, seq=seq, cl=cl, cl_len=cl_len)


def encode_block(block, final):
    p = block_plan(block)
    lit_code, cl_code = canonical_codes(p['lit_len']), canonical_codes(p['cl_len'])
    w = BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(p['nlit'] - 257, 5)
    w.bits(0, 5)
    w.bits(15, 4)
    for s in CL_ORDER:
        w.bits(p['cl_len'][s], 3)
    for v in p['seq']:
        w.code(cl_code[v], p['cl_len'][v])
    for s, eb, ev in p['tokens']:
        w.code(lit_code[s], p['lit_len'][s])
        if s > 256:
            w.bits(ev, eb)
            w.bits(0, 1)                                                 # the one distance code, length 1: distance 1, no extra bits
    if final:
        w.align()
    else:
        w.bits(0, 3)                                                     # an empty stored block: the next block starts on a byte
        w.align()
        w.out += b'\x00\x00\xff\xff'
    return bytes(w.out)


def adler_partial(block):
    """(sum of the bytes, sum of (n - i) * byte i), both mod 65521: the block's share of (a, b) when a starts from 0."""
    d = np.frombuffer(block, np.uint8).astype(np.int64)
    n = len(d)
    return int(d.sum() % ADLER), int((d * (n - np.arange(n))).sum() % ADLER)


def adler_combine(parts):
    """parts: (n, sa, sb) per block, in order."""
    n, sa, sb = 0, 0, 0
    for n2, sa2, sb2 in parts:
        sb = (sb + n2 * sa + sb2) % ADLER
        sa = (sa + sa2) % ADLER
        n += n2
    return (((n + sb) % ADLER) << 16) | ((1 + sa) % ADLER)


def blocks_of(stream, block_bytes):
    return [stream[i:i + block_bytes] for i in range(0, len(stream), block_bytes)]


def encode(img, filt=-1, block_bytes=32768):
    """The zlib stream of one image."""
    assert 64 <= block_bytes <= 65536 and -1 <= filt <= 4
    stream, _ = filtered_stream(img, filt)
    blocks = blocks_of(stream, block_bytes)
    body = b''.join(encode_block(b, i == len(blocks) - 1) for i, b in enumerate(blocks))
    adler = adler_combine([(len(b),) + adler_partial(b) for b in blocks])
    return b'\x78\x01' + body + struct.pack('>I', adler)


def encode_batch(imgs, filt=-1, block_bytes=32768):
    """(bytes, offsets [N+1]) of N same-size images."""
    parts = [encode(a, filt, block_bytes) for a in imgs]
    return b''.join(parts), [0] + list(np.cumsum([len(p) for p in parts]))


def workspace_slot_bytes(block_len):
    """The bound of the header on one block's coded bytes: 17 + 19 * 3 + 287 * 7 header bits, 15 bits per byte, end-of-block 15, the 3 bits
    of the stored block, then the byte padding and its 4 bytes."""
    return (17 + 57 + 287 * 7 + 15 * block_len + 15 + 3 + 7) // 8 + 4
