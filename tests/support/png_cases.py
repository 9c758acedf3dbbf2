"""The cases of tests/test_png_cpu.py and tests/test_gpu_png.py: name -> (uint8 image [H,W] or [H,W,C], filter -1..4, block_bytes), the smallest
shapes at which each stage of the PNG encoder can go wrong, and reference(name) = the restatement's zlib stream, computed once per process."""
import functools

import numpy as np

import png_ref as P


def noise(h, w, c, seed):
    a = np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


def five_winners():
    """Grey 10 x 64: between rows of noise, a row made for each filter type -- +5 / -5 alternating (None), a ramp (Sub), a copy of the row
    above (Up), x = (left + up) >> 1 (Average), and a row whose left half copies the row above while its right half
    is flat under a flat row (Paeth follows both)."""
    w, rng = 64, np.random.RandomState(11)
    rows = []
    for kind in range(5):
        up = rng.randint(0, 256, w)
        rows.append(up)
        if kind == 0:
            x = np.where(np.arange(w) % 2 == 0, 5, 251)
        elif kind == 1:
            x = (40 + 3 * np.arange(w)) % 256
        elif kind == 2:
            x = up.copy()
        elif kind == 3:
            x = np.zeros(w, np.int64)
            for i in range(w):
                x[i] = ((int(x[i - 1]) if i else 0) + int(up[i])) >> 1
        else:                                                                   # left half: the row above predicts; right half: the left byte does
            up[w // 2:] = 90
            x = np.where(np.arange(w) < w // 2, up, 97)
        rows.append(x)
    return np.stack(rows).astype(np.uint8)


def _interleave(values):
    """values sorted so that equal ones are together -> an order in which no two equal values are adjacent (the most frequent fills at most
    every other place)."""
    n = len(values)
    out = np.zeros(n, np.uint8)
    half = (n + 1) // 2
    out[0::2], out[1::2] = values[:half], values[half:]
    return out


def fibonacci_limiter():
    """Grey 55 x 520, filter 0: the counts of the block's 21 symbols are the Fibonacci numbers F1 .. F21 -- end-of-block is F1 = 1, the 55
    filter bytes are the value 0 (F10), the pixels hold 19 more values with the other counts F2 .. F21: 28 655 stream bytes in one block, no two
    equal bytes adjacent.  Every leaf is heavier than all the lighter ones together, so the Huffman tree is a chain of depth 20.  (A twenty-first
    byte value of count 1 would be a third 1 beside end-of-block: the tie lets the merge pair leaves and the depth drops to 11.)"""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    assert fib[9] == 55 and sum(fib[1:]) == 28655 == 55 * 521
    counts = [f for i, f in enumerate(fib) if i not in (0, 9)]
    values = np.concatenate([np.full(c, v + 1, np.uint8) for v, c in sorted(enumerate(counts), key=lambda t: -t[1])])
    return _interleave(values).reshape(55, 520)


CL_LIMITER_CODES = (0, 0, 0, 1, 2, 9, 11, 10, 31, 31, 28, 17, 4, 3, 0, 4)      # codes per length 0..15: Kraft sum 1, 151 symbols (one is end-of-block)


def cl_limiter():
    """Grey 31 x 1056, filter 0: symbol frequencies 2^(15 - length) for the lengths of CL_LIMITER_CODES, so the literal/length code IS that
    set of lengths (32 767 bytes + end-of-block in one block), and the counts of the code-length alphabet (107 zeros, 1 2 9 11 10 31 31 28 17
    4 3 4) give an unrestricted tree of depth 8 > 7.  Value 0 has the shortest code: its 4096 occurrences include the 31 filter bytes."""
    lengths = [l for l, k in enumerate(CL_LIMITER_CODES) for _ in range(k)]
    assert sum(2 ** (15 - l) for l in lengths) == 1 << 15 and lengths[-1] == 15
    freq = [2 ** (15 - l) for l in lengths[:-1]]                                # the last length-15 code is end-of-block
    freq[0] -= 31
    values = np.concatenate([np.full(f, v, np.uint8) for v, f in enumerate(freq)])
    return _interleave(values).reshape(31, 1056)


@functools.lru_cache(maxsize=None)
def cases():
    c = {
        'grey_1x1_two_symbols': (np.zeros((1, 1), np.uint8), 0, 32768),
        'grey_1x2': (np.array([[3, 200]], np.uint8), -1, 32768),
        'rgb_3x5_no_match': (noise(3, 5, 3, 1), -1, 32768),
        'rgb_37x53': (P.image(37, 53, 3, 2), -1, 32768),
        'rgb_37x53_bb1024': (P.image(37, 53, 3, 2), -1, 1024),
        'grey_64x48': (P.image(64, 48, 3, 2)[:, :, 1], -1, 32768),
        'rgb_96x128': (P.image(96, 128, 3, 2), -1, 32768),
        'rgb_96x128_bb1024': (P.image(96, 128, 3, 2), -1, 1024),
        'half_flat': (P.half_flat(), -1, 32768),
        'half_flat_bb1024': (P.half_flat(), -1, 1024),
        'winners_adaptive': (five_winners(), -1, 32768),
        'exact_multiple': (noise(64, 63, 1, 2) // 64, 0, 1024),                  # L = 64 * 64 = 4 * 1024
        'one_byte_over': (noise(64, 63, 1, 2) // 64, 0, 4095),                   # L = 4095 + 1
        'fibonacci_limiter': (fibonacci_limiter(), 0, 32768),
        'cl_limiter': (cl_limiter(), 0, 32768),
        'noise_rgb_64x64': (noise(64, 64, 3, 3), -1, 32768),
        'rgb_40x30_bb65536': (P.image(40, 30, 5, 12), -1, 65536),
    }
    for t in range(5):
        c[f'winners_filter{t}'] = (five_winners(), t, 32768)
    for bb in (64, 1000, 65536):
        c[f'zeros_300x300_bb{bb}'] = (np.zeros((300, 300), np.uint8), 0, bb)     # one run per block, cut by the block ends
        c[f'sevens_300x300_bb{bb}'] = (np.full((300, 300), 7, np.uint8), 0, bb)  # runs of 300 between the filter bytes
    for w in (259, 260, 261, 262, 517):                                         # rests q = (w - 1) % 258 = 0, 1, 2, 3, 0 (two full matches)
        c[f'sevens_5x{w}'] = (np.full((5, w), 7, np.uint8), 0, 65536)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    img, filt, bb = cases()[name]
    return P.encode(img, filt, bb)
