"""The host side of the batched JPEG decode and of the Motion-JPEG reader (no GPU): video.MjpegAviReader reads back what MjpegAviWriter writes
-- with its index, without it, with file-relative index offsets -- and names what it refuses; video.jpeg_scan_plan(default_huffman=True)
gives a file without DHT the tables of the file with them, and the restatement then equals PIL; the ctypes structures of
eg3d_jpegdec_batch_* match the header and the host-only calls answer, and reject, without a device."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))

PIL = pytest.importorskip('PIL')
from PIL import features  # noqa: E402

if not features.check('jpg'):
    pytest.skip('PIL without JPEG support', allow_module_level=True)

import jpeg_cases as JC  # noqa: E402
import jpeg_ref  # noqa: E402
import jpegbatch_cases as BC  # noqa: E402
import jpegdec_cases as DC  # noqa: E402
import jpegdec_ref as R  # noqa: E402
from inv3d_amd import video as V  # noqa: E402

W, H, FPS = 40, 24, 25


def _frames():
    """six frames of W x H from both encoders; odd and even lengths are both among them"""
    frames = [jpeg_ref.encode(JC.textured(H, W, 100 + i), quality=90, subsampling='420') for i in range(2)]
    i = 0
    while len(frames) < 6 or len({len(f) & 1 for f in frames}) < 2:
        frames.append(DC.pil_file(JC.textured(H, W, 110 + i), 80 + i % 15, (0, 1, 2)[i % 3]))
        i += 1
    return frames


@pytest.fixture(scope='module')
def avi(tmp_path_factory):
    frames = _frames()
    path = str(tmp_path_factory.mktemp('avi') / 'clip.avi')
    BC.write_avi(path, frames, W, H, FPS)
    return path, frames


def _check(path, frames):
    with V.MjpegAviReader(path) as r:
        assert (r.num_frames, r.fps, r.width, r.height) == (len(frames), FPS, W, H) and len(r) == len(frames)
        assert [r.frame_bytes(i) for i in range(r.num_frames)] == frames
        assert list(r) == frames
        with pytest.raises(IndexError):
            r.frame_bytes(len(frames))


def test_avi_round_trip(avi):
    path, frames = avi
    assert {len(f) & 1 for f in frames} == {0, 1}
    _check(path, frames)


def test_avi_without_index_and_with_file_offsets(avi, tmp_path):
    path, frames = avi
    data = open(path, 'rb').read()
    for name, variant in (('noindex.avi', BC.avi_without_index(data)), ('fileoffsets.avi', BC.avi_with_file_offsets(data))):
        assert variant != data
        p = str(tmp_path / name)
        open(p, 'wb').write(variant)
        _check(p, frames)
    # an index that fits neither convention: the 'movi' list is walked
    at = data.rindex(b'idx1')
    broken = bytearray(data)
    for i in range(len(frames)):
        broken[at + 16 + 16 * i:at + 20 + 16 * i] = struct.pack('<I', 3)
    p = str(tmp_path / 'badindex.avi')
    open(p, 'wb').write(bytes(broken))
    _check(p, frames)


def test_avi_refusals_name_their_reason(avi, tmp_path):
    path, frames = avi
    data = open(path, 'rb').read()
    p = str(tmp_path / 'bad.avi')
    open(p, 'wb').write(data.replace(b'MJPG', b'H264'))
    with pytest.raises(ValueError, match='MJPG'):
        V.MjpegAviReader(p)
    open(p, 'wb').write(data + b'RIFF' + struct.pack('<I', 16) + b'AVIX' + b'LIST' + struct.pack('<I', 4) + b'movi')
    with pytest.raises(ValueError, match='AVIX'):
        V.MjpegAviReader(p)
    BC.write_avi(p, frames[:2] + [b''] + frames[2:], W, H, FPS)
    with pytest.raises(ValueError, match='zero-length'):
        V.MjpegAviReader(p)
    open(p, 'wb').write(b'RIFF' + struct.pack('<I', 4) + b'WAVE')
    with pytest.raises(ValueError, match='AVI'):
        V.MjpegAviReader(p)


@pytest.mark.parametrize('kind', ['444', '420', 'grey'])
def test_default_huffman_tables(kind):
    img = JC.textured(40, 56, 120)
    data = DC.pil_file(img[:1], 85) if kind == 'grey' else DC.pil_file(img, 85, 0 if kind == '444' else 2)
    stripped = BC.strip_dht(data)
    assert b'\xff\xc4' not in stripped[:V.jpeg_scan_plan(data).scan_start] and len(stripped) < len(data)
    with pytest.raises(V.JpegUnsupported, match='uses a Huffman table the file does not define'):
        V.jpeg_scan_plan(stripped)
    full, plan = V.jpeg_scan_plan(data), V.jpeg_scan_plan(stripped, default_huffman=True)
    assert plan.huffman == full.huffman and len(plan.huffman) == (2 if kind == 'grey' else 4)
    assert plan.components == full.components and plan.quant == full.quant
    assert V.jpeg_scan_plan(data, default_huffman=True) == full                     # tables the file defines are the file's
    want = BC.pil_rgb(stripped)
    assert np.array_equal(want, BC.pil_rgb(data))
    assert np.array_equal(R.decode(stripped, plan), want)


def test_batch_structures_match_the_header(tmp_path):
    """JpegDecImage / JpegDecBatchParams against the header compiled with gcc; the host-only calls answer here and reject bad arguments
    before any launch."""
    import ctypes as C
    import shutil
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    pairs = (('eg3d_jpegdec_image', L.JpegDecImage), ('eg3d_jpegdec_batch_params', L.JpegDecBatchParams))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {']
    want = []
    for cname, cls in pairs:
        src.append(f' printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            src.append(f' printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(cls, f).offset)
    src += [' return 0;', '}']
    (tmp_path / 't.c').write_text('\n'.join(src) + '\n')
    r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 't'), str(tmp_path / 't.c')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-600:]
    got = [int(v) for v in subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    lib = L.lib()

    def params(n=2, **kw):
        images = (L.JpegDecImage * max(n, 1))()
        for im in images:
            im.H, im.W, im.ncomp, im.hsamp, im.vsamp, im.data_bytes = 53, 37, 3, 2, 2, 1000
        images[-1].H, images[-1].W, images[-1].ncomp = 8, 300, 1
        return L.JpegDecBatchParams(images=images, n=n, subseq_bytes=128, **kw), images
    ws, plan, one = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    p, images = params()
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(p), C.byref(ws), C.byref(plan)) == 0                      # host only: answerable here
    singles = 0
    for im in images:
        q = L.JpegDecParams(H=im.H, W=im.W, ncomp=im.ncomp, hsamp=2, vsamp=2, subseq_bytes=128, data_bytes=1000)
        assert lib.eg3d_jpegdec_query_workspace(C.byref(q), C.byref(one)) == 0
        singles += one.value
    assert ws.value == singles and plan.value >= 2 * 200 and plan.value % 16 == 0
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(params(n=0)[0]), C.byref(ws), C.byref(plan)) == -1          # N = 0
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(params(n=-3)[0]), C.byref(ws), C.byref(plan)) == -1
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(p), None, C.byref(plan)) == -1
    assert lib.eg3d_jpegdec_batch_query_workspace(None, C.byref(ws), C.byref(plan)) == -1
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(L.JpegDecBatchParams(n=2, subseq_bytes=128)), C.byref(ws), C.byref(plan)) == -1
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(params(n=L.JPEGDEC_MAX_BATCH + 1)[0]), C.byref(ws), C.byref(plan)) == -3
    q, images = params()
    q.subseq_bytes = 100
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(q), C.byref(ws), C.byref(plan)) == -1
    q, images = params()
    images[1].hsamp, images[1].ncomp = 4, 3
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(q), C.byref(ws), C.byref(plan)) == -2
    q, images = params()
    images[0].data_bytes = 1 << 28                                                                                  # an over-large image
    assert lib.eg3d_jpegdec_batch_query_workspace(C.byref(q), C.byref(ws), C.byref(plan)) == -3
    assert lib.eg3d_jpegdec_batch_decode(C.byref(q), None) == -3 and lib.eg3d_jpegdec_batch_plan(C.byref(q)) == -1
    assert lib.eg3d_jpegdec_batch_decode(C.byref(p), None) == -1 and lib.eg3d_jpegdec_batch_plan(C.byref(p)) == -1    # null pointers: no launch
    assert lib.eg3d_jpegdec_batch_decode(None, None) == -1 and lib.eg3d_jpegdec_batch_plan(None) == -1


def test_batch_wrapper_without_a_device(monkeypatch):
    """An empty list is [] without touching a device; parse failures raise, or come back in place with return_errors=True and keep the other
    files out of no batch (the device call is replaced: it sees exactly the files that parsed)."""
    import torch
    from inv3d_amd import hipops as H
    assert H.jpeg_decode_batch([]) == []
    good, bad = DC.cases()['8x8_444'], BC.progressive_file()
    with pytest.raises(V.JpegUnsupported, match='progressive'):
        H.jpeg_decode_batch([good, bad])
    seen = []

    def begin(raws, plans, subseq_bytes, device=None):
        seen.append((list(raws), subseq_bytes))
        raise RuntimeError('stop here')
    monkeypatch.setattr(H, '_jpegdec_batch_begin', begin)
    with pytest.raises(RuntimeError, match='stop here'):
        H.jpeg_decode_batch([good, bad, torch.frombuffer(bytearray(good), dtype=torch.uint8)], subseq_bytes=64, return_errors=True)
    assert seen == [([good, good], 64)]
    stats = ['old']
    out = H.jpeg_decode_batch([bad], return_errors=True, stats=stats)
    assert len(out) == 1 and isinstance(out[0], V.JpegUnsupported) and stats == [None] and len(seen) == 1
