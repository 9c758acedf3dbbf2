"""The PNG encoder without a GPU: the numpy restatement tests/support/png_ref.py (what tests/test_gpu_png.py requires the GPU bytes to equal)
and the host code of inv3d_amd/video.py, validated against things that are not ours -- zlib's inflate and Adler-32, PIL's PNG reader, a heapq
Huffman code -- and the size condition against the host path."""
import heapq
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import png_cases as PC  # noqa: E402
import png_ref as P  # noqa: E402
from inv3d_amd import video as V  # noqa: E402

NAMES = sorted(PC.cases())


def _hwc(img):
    return img if img.ndim == 3 else img[:, :, None]


def _host_png(img):
    """The file the parent's write_png writes, from zlib and struct alone."""
    a = _hwc(img)
    hh, ww, ch = a.shape
    rows = np.zeros((hh, 1 + ww * ch), np.uint8)
    rows[:, 1:] = a.reshape(hh, ww * ch)

    def chunk(tag, payload):
        return struct.pack('>I', len(payload)) + tag + payload + struct.pack('>I', zlib.crc32(tag + payload) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', ww, hh, 8, 2 if ch == 3 else 0, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def _pixels(png_bytes):
    return np.asarray(Image.open(io.BytesIO(png_bytes)))


@pytest.mark.parametrize('name', NAMES)
def test_stream_inflates_to_the_filtered_rows_and_opens_in_pil(name):
    img, filt, bb = PC.cases()[name]
    z = PC.reference(name)
    stream, types = P.filtered_stream(img, filt)
    assert zlib.decompress(z) == stream
    assert z[:2] == b'\x78\x01' and struct.unpack('>I', z[-4:])[0] == zlib.adler32(stream)
    a = _hwc(img)
    got = _pixels(V.png_container(z, a.shape[0], a.shape[1], a.shape[2]))
    assert np.array_equal(got.reshape(a.shape), a)
    assert len(z) <= 2 + 4 + sum(P.workspace_slot_bytes(len(b)) for b in P.blocks_of(stream, bb))
    if filt >= 0:
        assert set(types) == {filt}


def test_the_filters_are_pngs():
    """Un-filtering by PIL (above) checks every type that occurs; here each forced type and the adaptive choice on the five-winners image."""
    img = PC.five_winners()
    _, types = P.filtered_stream(img, -1)
    assert set(types) == {0, 1, 2, 3, 4}, types
    assert types[1::2] == [0, 1, 2, 3, 4]                                   # the row made for each type is won by it
    rgb = P.image(37, 53, 3, 12)
    for t in range(5):
        for a in (img, rgb):
            z = P.encode(a, t, 32768)
            assert np.array_equal(_pixels(V.png_container(z, a.shape[0], a.shape[1], _hwc(a).shape[2])).reshape(a.shape), a)


def _heapq_cost(counts):
    """(total bits, depth) of an unrestricted Huffman code built with heapq."""
    heap = [(c, s, 0) for s, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    cost, tick = 0, len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


@pytest.mark.parametrize('name', NAMES)
def test_codes_are_complete_limited_and_optimal(name):
    img, filt, bb = PC.cases()[name]
    stream, _ = P.filtered_stream(img, filt)
    for block in P.blocks_of(stream, bb):
        p = P.block_plan(block)
        for counts, lens, limit in ((p['lit'], p['lit_len'], 15), (p['cl'], p['cl_len'], 7)):
            assert all((l > 0) == (c > 0) for l, c in zip(lens, counts))
            assert max(lens) <= limit
            assert sum(2 ** (limit - l) for l in lens if l) == 2 ** limit      # Kraft sum 1: the code is complete
            cost, depth = _heapq_cost(counts)
            if depth <= limit:
                assert sum(l * c for l, c in zip(lens, counts)) == cost
            codes = P.canonical_codes(lens)
            words = sorted(format(codes[s], f'0{lens[s]}b') for s in range(len(lens)) if lens[s])
            assert all(not b.startswith(a) for a, b in zip(words, words[1:]))  # prefix-free
        assert p['lit'][256] == 1 and p['nlit'] >= 257
        assert p['dist_len'] == (1 if any(s > 256 for s, _, _ in p['tokens']) else 0)


def test_the_special_cases_are_what_they_claim():
    plan = lambda name: P.block_plan(P.filtered_stream(*PC.cases()[name][:2])[0])      # noqa: E731  (single-block cases)
    p = plan('fibonacci_limiter')
    assert len(P.filtered_stream(*PC.cases()['fibonacci_limiter'][:2])[0]) == 28655
    assert p['dist_len'] == 0 and sorted(c for c in p['lit'] if c)[:5] == [1, 1, 2, 3, 5] and sum(1 for c in p['lit'] if c) == 21
    assert max(P.huffman_depths(p['lit'])[0].values()) == 20 > 15 and max(p['lit_len']) == 15
    p = plan('cl_limiter')
    assert max(P.huffman_depths(p['cl'])[0].values()) > 7 and max(p['cl_len']) == 7
    assert max(P.huffman_depths(p['lit'])[0].values()) == 15
    assert [sum(1 for l in p['lit_len'] if l == k) for k in range(1, 16)] == list(PC.CL_LIMITER_CODES[1:])
    p = plan('grey_1x1_two_symbols')
    assert [s for s in range(286) if p['lit'][s]] == [0, 256] and p['dist_len'] == 0
    assert plan('rgb_3x5_no_match')['dist_len'] == 0 and plan('noise_rgb_64x64')['dist_len'] == 0
    rests = set()
    for w in (259, 260, 261, 262, 517):
        toks = plan(f'sevens_5x{w}')['tokens']
        assert sum(1 for s, _, _ in toks if s == 285) == 5 * ((w - 1) // 258)
        rests.add((w - 1) % 258)
        assert sum(1 for s, _, _ in toks if 257 <= s < 285) == (5 if (w - 1) % 258 >= 3 else 0)
    assert rests == {0, 1, 2, 3}
    stream = P.filtered_stream(*PC.cases()['zeros_300x300_bb1000'][:2])[0]
    toks = P.tokens(P.blocks_of(stream, 1000)[0])                            # one run of 1000: a literal, 3 x 258, a rest of 225
    assert [s for s, _, _ in toks] == [0, 285, 285, 285, P.length_symbol(225)[0], 256]
    assert len(P.filtered_stream(*PC.cases()['exact_multiple'][:2])[0]) == 4 * 1024
    assert len(P.filtered_stream(*PC.cases()['one_byte_over'][:2])[0]) == 4095 + 1
    for length in range(3, 259):                                             # the length table against zlib's own decoder is the round trip; here its shape
        s, eb, ev = P.length_symbol(length)
        assert P.LEN_BASE[s - 257] + ev == length and ev < (1 << eb) or (eb == 0 and ev == 0)
    assert P.length_symbol(258) == (285, 0, 0) and P.length_symbol(257) == (284, 5, 30)


def test_container_and_host_encoder(tmp_path):
    for a in (P.image(37, 53, 3, 2), P.image(20, 28, 4, 2)[:, :, 0]):
        a3 = _hwc(a)
        rows = np.zeros((a3.shape[0], 1 + a3.shape[1] * a3.shape[2]), np.uint8)
        rows[:, 1:] = a3.reshape(a3.shape[0], -1)
        png = V.png_container(zlib.compress(rows.tobytes(), 9), a3.shape[0], a3.shape[1], a3.shape[2])
        im = Image.open(io.BytesIO(png))
        assert im.mode == ('RGB' if a3.shape[2] == 3 else 'L') and np.array_equal(np.asarray(im), a)
        path = str(tmp_path / 'host.png')
        V.write_png(path, a, encoder='host')
        assert open(path, 'rb').read() == _host_png(a)
        V.write_png(path, a)                                                 # the default is the host path
        assert open(path, 'rb').read() == _host_png(a)
        import torch
        V.write_png(path, torch.from_numpy(a), encoder='host')
        assert open(path, 'rb').read() == _host_png(a)
    with pytest.raises(ValueError):
        V.write_png(str(tmp_path / 'x.png'), a, encoder='fast')
    with pytest.raises(ValueError):
        V.png_container(b'', 4, 4, 2)


@pytest.mark.parametrize('bb', [32768, 1024])
@pytest.mark.parametrize('which', ['96x128', '37x53', 'half_flat'])
def test_smaller_than_the_host_path(which, bb):
    img = dict([('96x128', P.image(96, 128, 3, 2)), ('37x53', P.image(37, 53, 3, 2)), ('half_flat', P.half_flat())])[which]
    ours = V.png_container(P.encode(img, -1, bb), img.shape[0], img.shape[1], 3)
    assert len(ours) < len(_host_png(img)), (len(ours), len(_host_png(img)))


def test_size_against_zlib_rle():
    """Nothing is asserted on the ratio (DESIGN.md 3.4 records it): zlib's Z_RLE at level 6 over the same filtered stream and the same block
    cuts, every block a stream of its own, against the restatement's bytes."""
    for name in NAMES:
        img, filt, bb = PC.cases()[name]
        stream, _ = P.filtered_stream(img, filt)
        rle = 0
        for block in P.blocks_of(stream, bb):
            c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
            rle += len(c.compress(block) + c.flush())
        ours = len(PC.reference(name)) - 6
        print(f'{name}: raw {_hwc(img).size} ours {ours} zlib-rle {rle} ratio {ours / rle:.3f}')
