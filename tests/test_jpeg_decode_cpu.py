"""The JPEG decoder's host side and its numpy restatement (no GPU): tests/support/jpegdec_ref.py equals PIL byte for byte on every case of
tests/support/jpegdec_cases.py; video.jpeg_scan_plan reads the fields of files from both encoders and names what it refuses; the ctypes
structure matches the header; images.decode_rgb(decoder='gpu') routes and falls back as documented (hipops.jpeg_decode replaced)."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))

PIL = pytest.importorskip('PIL')
from PIL import Image, features  # noqa: E402

if not features.check('jpg'):
    pytest.skip('PIL without JPEG support', allow_module_level=True)

import jpeg_cases as JC  # noqa: E402
import jpegdec_cases as DC  # noqa: E402
import jpegdec_ref as R  # noqa: E402
from inv3d_amd import video as V  # noqa: E402


@pytest.mark.parametrize('name', list(DC.cases()))
def test_restatement_equals_pil(name):
    got, want = DC.ref_decode(name), DC.pil_decode(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f'{int((got != want).sum())} bytes differ'


def test_case_list_covers_what_it_claims():
    c = DC.cases()
    plans = {n: V.jpeg_scan_plan(b) for n, b in c.items()}
    assert {p.subsampling for p in plans.values()} == {'444', '422', '420', 'grey'}
    assert plans['restart1_64x48_420'].restart_interval == 1 and c['restart1_64x48_420'].count(b'\xff\xd0') >= 2       # RST0 twice: the index wraps
    assert plans['restart3_64x48_444'].restart_interval == 3 and plans['restart5_70x50_422'].restart_interval == 5
    assert plans['own_37x53_420'].restart_interval > 0 and plans['own_grey_20x12'].subsampling == 'grey'
    assert plans['optimize_37x53_420'].huffman[(1, 0)] != V.AC_LUMA and plans['37x53_420'].huffman[(1, 0)] == (V.AC_LUMA[0], V.AC_LUMA[1])
    longest = lambda name: max(i + 1 for i, n in enumerate(plans[name].huffman[(1, 0)][0]) if n)
    assert longest('optimize_128x128_q98_444') >= 14 and longest('noise_q100_444') == 16                              # beyond the 9-bit lookup
    assert plans[DC.BIG].restart_interval == 0 and plans[DC.BIG].scan_end - plans[DC.BIG].scan_start > 4 * 256 * 128  # more than four workgroups
    assert c['noise_q100_444'].count(b'\xff\x00') > 10                                                                # stuffed bytes


def test_scan_plan_fields():
    img = JC.textured(53, 37, 5)
    own = V.jpeg_header(53, 37, quality=75, subsampling='420', restart_interval=2) + b'\x00' * 5 + b'\xff\xd9'
    p = V.jpeg_scan_plan(own)
    ql, qc = V.jpeg_tables(75)
    assert (p.height, p.width, p.restart_interval, p.subsampling) == (53, 37, 2, '420')
    assert p.components == (V.JpegComponent(1, 2, 2, 0, 0, 0), V.JpegComponent(2, 1, 1, 1, 1, 1), V.JpegComponent(3, 1, 1, 1, 1, 1))
    assert p.quant == (ql, qc, None, None)
    assert p.huffman == {(0, 0): V.DC_LUMA, (1, 0): V.AC_LUMA, (0, 1): V.DC_CHROMA, (1, 1): V.AC_CHROMA}
    assert own[p.scan_start:p.scan_end] == b'\x00' * 5 and own[p.scan_end:] == b'\xff\xd9'
    pil = DC.pil_file(img, 85, 1, optimize=True, comment=b'a comment')             # COM is skipped
    p = V.jpeg_scan_plan(pil)
    with Image.open(io.BytesIO(pil)) as im:
        assert (p.width, p.height) == im.size
        for tq, tab in im.quantization.items():
            assert sorted(p.quant[tq]) == sorted(tab)                                      # (whichever order this PIL lists them in)
    assert p.subsampling == '422' and p.restart_interval == 0 and [c.tq for c in p.components] == [0, 1, 1]
    assert pil[p.scan_end:p.scan_end + 2] == b'\xff\xd9' and pil[p.scan_start - 3:p.scan_start] == b'\x00\x3f\x00'
    for (tc, th), (bits, vals) in p.huffman.items():
        assert len(bits) == 16 and sum(bits) == len(vals) and tc in (0, 1) and th in (0, 1)
    grey = V.jpeg_scan_plan(DC.cases()['grey_20x12'])
    assert len(grey.components) == 1 and (grey.components[0].h, grey.components[0].v) == (1, 1) and grey.subsampling == 'grey'


def _unsupported(data, *words):
    with pytest.raises(V.JpegUnsupported) as e:
        V.jpeg_scan_plan(data)
    assert all(w in str(e.value) for w in words), str(e.value)


def test_unsupported_kinds_raise_with_their_reason():
    img = JC.textured(40, 40, 3)
    good = DC.pil_file(img, 90, 2)
    _unsupported(DC.pil_file(img, 90, 2, progressive=True), 'progressive')
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.transpose(np.concatenate([img, img[:1]]), (1, 2, 0))), 'CMYK').save(buf, 'JPEG', quality=90)
    _unsupported(buf.getvalue(), '4 components')
    try:
        f440 = DC.pil_file(img, 90, '4:4:0')
    except (ValueError, TypeError, KeyError, OSError):
        f440 = None
    if f440 is None:                                                               # this PIL does not write 4:4:0: patch the sampling byte of a 4:2:2 file
        f = bytearray(DC.pil_file(img, 90, 1))
        i = f.index(b'\xff\xc0')
        assert f[i + 11] == 0x21
        f[i + 11] = 0x12
        f440 = bytes(f)
    _unsupported(f440, 'sampling factors', '1x2')
    _unsupported(good[:V.jpeg_scan_plan(good).scan_start - 30], 'truncated header')
    _unsupported(good[:200], 'truncated header')
    _unsupported(good[:-2], 'missing EOI')
    _unsupported(b'\x89PNG\r\n\x1a\n' + bytes(32), 'not a JPEG')
    i = good.index(b'\xff\xdb')
    sixteen = good[:i] + b'\xff\xdb' + struct.pack('>H', 2 + 1 + 128) + b'\x10' + bytes(range(1, 129)) + good[i:]
    _unsupported(sixteen, '16-bit quantisation')
    soi_app14 = good[:2] + b'\xff\xee' + struct.pack('>H', 14) + b'Adobe\x00\x64\x00\x00\x00\x00\x00' + good[2:]
    _unsupported(soi_app14, 'Adobe', 'RGB')
    j = good.index(b'\xff\xc0')
    _unsupported(good[:j + 4] + b'\x0c' + good[j + 5:], '12-bit')
    _unsupported(good[:j + 1] + b'\xc9' + good[j + 2:], 'arithmetic')
    p = V.jpeg_scan_plan(good)
    two_scans = good[:p.scan_end] + good[p.scan_start - 14:p.scan_end] + b'\xff\xd9'
    _unsupported(two_scans, 'several scans')
    assert issubclass(V.JpegUnsupported, ValueError)


def test_restatement_names_the_status_of_damaged_streams():
    name = 'textured_q90_420'
    data, p = DC.cases()[name], V.jpeg_scan_plan(DC.cases()[name])
    half = data[:p.scan_start + (p.scan_end - p.scan_start) // 2] + b'\xff\xd9'
    with pytest.raises(R.DecodeError) as e:
        R.decode(half)
    assert e.value.status == R.ERR_BLOCKS
    stray = bytearray(data)
    stray[p.scan_start + 40:p.scan_start + 42] = b'\xff\xd3'                        # a restart marker in a file without restarts
    with pytest.raises(R.DecodeError) as e:
        R.decode(bytes(stray), p)
    assert e.value.status in (R.ERR_SEGMENTS, R.ERR_MARKER)


def test_ctypes_structure_matches_the_header(tmp_path):
    """JpegDecParams against eg3d_jpegdec_params compiled with gcc (tests/test_host.py checks the older structures the same way)."""
    import ctypes as C
    import shutil
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    fields = [f[0] for f in L.JpegDecParams._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', ' printf("%zu\\n", sizeof(eg3d_jpegdec_params));']
    src += [f' printf("%zu\\n", offsetof(eg3d_jpegdec_params, {f}));' for f in fields]
    src += [' printf("%d %d\\n", EG3D_JPEGDEC_TABLE_BYTES, EG3D_JPEGDEC_RESULT_WORDS);', ' return 0;', '}']
    (tmp_path / 't.c').write_text('\n'.join(src) + '\n')
    r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 't'), str(tmp_path / 't.c')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-600:]
    got = [int(v) for v in subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(L.JpegDecParams)] + [getattr(L.JpegDecParams, f).offset for f in fields] + [L.JPEGDEC_TABLE_BYTES, L.JPEGDEC_RESULT_WORDS]
    assert got == want
    lib = L.lib()
    p, n = L.JpegDecParams(H=53, W=37, ncomp=3, hsamp=2, vsamp=2, subseq_bytes=128, data_bytes=1000), C.c_int64(0)
    assert lib.eg3d_jpegdec_query_workspace(C.byref(p), C.byref(n)) == 0 and n.value > 3 * 4 * 6 * 64 * 2            # host only: answerable here
    for bad in (dict(subseq_bytes=100), dict(subseq_bytes=8), dict(ncomp=4), dict(H=0), dict(data_bytes=-1)):
        q = L.JpegDecParams(**dict(dict(H=53, W=37, ncomp=3, hsamp=2, vsamp=2, subseq_bytes=128, data_bytes=1000), **bad))
        assert lib.eg3d_jpegdec_query_workspace(C.byref(q), C.byref(n)) == -1, bad
    q = L.JpegDecParams(H=53, W=37, ncomp=3, hsamp=1, vsamp=2, subseq_bytes=128, data_bytes=1000)
    assert lib.eg3d_jpegdec_query_workspace(C.byref(q), C.byref(n)) == -2
    assert lib.eg3d_jpegdec_decode(C.byref(p), None) == -1                                                           # null pointers: no launch


def test_decode_rgb_routing_and_fallback(tmp_path, monkeypatch):
    from inv3d_amd import hipops, images
    img = JC.textured(24, 32, 8)
    files = {}
    for fname, data in (('a.jpg', DC.pil_file(img, 90, 2)), ('b.JPEG', DC.pil_file(img, 80, 0)), ('prog.jpg', DC.pil_file(img, 90, 2, progressive=True))):
        files[fname] = str(tmp_path / fname)
        open(files[fname], 'wb').write(data)
    files['c.png'] = str(tmp_path / 'c.png')
    Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0)))).save(files['c.png'])
    calls, marker = [], torch.full((24, 32, 3), 7, dtype=torch.uint8)

    def fake(data, subseq_bytes=128, device=None, stats=None):
        V.jpeg_scan_plan(data)                                                     # the real parser: JpegUnsupported for the progressive file
        calls.append(len(data))
        if calls and fake.refuse:
            raise hipops.JpegDecodeRefused(4)
        return marker
    fake.refuse = False
    monkeypatch.setattr(hipops, 'jpeg_decode', fake)
    pil = lambda f: np.asarray(Image.open(files[f]).convert('RGB'))
    assert np.array_equal(images.decode_rgb(files['a.jpg'], 'cpu').numpy(), pil('a.jpg')) and calls == []            # the default is PIL
    assert np.array_equal(images.decode_rgb(files['a.jpg'], 'cpu', decoder='pil').numpy(), pil('a.jpg')) and calls == []
    assert images.decode_rgb(files['a.jpg'], 'cpu', decoder='gpu') is marker and len(calls) == 1
    assert images.decode_rgb(files['b.JPEG'], 'cpu', decoder='gpu') is marker and len(calls) == 2                    # any case of the extension
    assert np.array_equal(images.decode_rgb(files['c.png'], 'cpu', decoder='gpu').numpy(), pil('c.png')) and len(calls) == 2
    told = []
    out = images.decode_rgb(files['prog.jpg'], 'cpu', decoder='gpu', report=lambda p, why: told.append((p, why)))
    assert np.array_equal(out.numpy(), pil('prog.jpg')) and len(calls) == 2 and told[0][0] == files['prog.jpg'] and 'progressive' in told[0][1]
    fake.refuse = True                                                             # a device status: PIL's pixels, and the caller hears of it
    out = images.decode_rgb(files['a.jpg'], 'cpu', decoder='gpu', report=lambda p, why: told.append((p, why)))
    assert np.array_equal(out.numpy(), pil('a.jpg')) and len(told) == 2 and 'status 4' in told[1][1]
    assert np.array_equal(images.decode_rgb(files['a.jpg'], 'cpu', decoder='gpu').numpy(), pil('a.jpg'))              # without a callback too
    bad = str(tmp_path / 'bad.jpg')
    open(bad, 'wb').write(b'not a jpeg at all')
    with pytest.raises(Exception) as e1:
        images.decode_rgb(bad, 'cpu')
    with pytest.raises(type(e1.value)):
        images.decode_rgb(bad, 'cpu', decoder='gpu')                               # a bad file raises what PIL raises
    with pytest.raises(ValueError):
        images.decode_rgb(files['a.jpg'], 'cpu', decoder='cuda')
    with pytest.raises(ValueError):
        images.load_targets(str(tmp_path), decoder='host')
    with pytest.raises(ValueError):
        images.write_aligned(str(tmp_path), {}, str(tmp_path / 'o'), decoder='host')


def test_jpeg_decode_refuses_without_falling_back():
    """hipops.jpeg_decode itself never takes another path: an unsupported file is JpegUnsupported, bad arguments and a missing GPU are errors."""
    from inv3d_amd import hipops
    from inv3d_amd._lib import Eg3dHipError
    good = DC.cases()['17x23_420']
    with pytest.raises(V.JpegUnsupported):
        hipops.jpeg_decode(DC.pil_file(JC.textured(24, 32, 8), 90, 2, progressive=True))
    with pytest.raises(Eg3dHipError):
        hipops.jpeg_decode(good, subseq_bytes=100)
    with pytest.raises(Eg3dHipError):
        hipops.jpeg_decode(torch.zeros(4, dtype=torch.float32))
    if not torch.cuda.is_available():
        with pytest.raises(Eg3dHipError):
            hipops.jpeg_decode(good)
    blob = hipops.jpeg_decode_tables(V.jpeg_scan_plan(good))
    assert len(blob) == 256 + 4 * 272 and blob[:64] == bytes(V.jpeg_scan_plan(good).quant[0]) and blob[256:272] == bytes(V.DC_LUMA[0])
