"""Media export without a GPU: the numpy restatement of the JPEG encoder (tests/support/jpeg_ref.py, what tests/test_gpu_video.py requires the
GPU bytes to equal) and the host code of inv3d_amd/video.py, validated against things that are not ours -- the tables PIL (libjpeg) writes,
PIL's decoder and encoder, a float64 DCT, a RIFF walker, and the cameras recorded from the reference's own look_at / gen_eyes."""
import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import jpeg_cases as JC  # noqa: E402
import jpeg_ref as J  # noqa: E402
from inv3d_amd import video as V  # noqa: E402


def _segments(data):
    """[(marker, payload)] of a JPEG file up to SOS."""
    assert data[:2] == b'\xff\xd8'
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        marker, length = data[i + 1], struct.unpack('>H', data[i + 2:i + 4])[0]
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            return out


def _split_tables(payloads, size_of):
    """A DQT / DHT segment may hold several tables: {first byte: table bytes}."""
    out = {}
    for p in payloads:
        i = 0
        while i < len(p):
            n = size_of(p, i)
            out[p[i]] = p[i + 1:i + n]
            i += n
    return out


@pytest.mark.parametrize('q', [1, 50, 75, 90, 100])
def test_tables_equal_what_pil_writes(q):
    bio = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(bio, 'JPEG', quality=q, subsampling=2)
    segs = _segments(bio.getvalue())
    want_q = _split_tables([p for m, p in segs if m == 0xDB], lambda p, i: 65)
    want_h = _split_tables([p for m, p in segs if m == 0xC4], lambda p, i: 17 + sum(p[i + 1:i + 17]))
    assert sorted(want_q) == [0, 1] and sorted(want_h) == [0x00, 0x01, 0x10, 0x11]
    for name, hdr in (('product', V.jpeg_header(16, 16, quality=q)), ('restatement', J.header(16, 16, 3, q, '420', 1))):
        segs = _segments(hdr)
        got_q = _split_tables([p for m, p in segs if m == 0xDB], lambda p, i: 65)
        got_h = _split_tables([p for m, p in segs if m == 0xC4], lambda p, i: 17 + sum(p[i + 1:i + 17]))
        assert got_q == want_q, name
        assert got_h == want_h, name
    # the natural-order tables themselves
    zz = np.array(V.ZIGZAG)
    for tid, (mine, ref) in enumerate(zip(V.jpeg_tables(q), J.quant_tables(q))):
        assert bytes(np.array(mine)[zz].tolist()) == want_q[tid]
        assert bytes(ref.reshape(64)[J.ZZ].tolist()) == want_q[tid]


def test_product_header_equals_the_restatement_header():
    for name, (img, q, ss, r) in JC.cases().items():
        c, h, w = img.shape
        rr = J.default_restart(w, ss, c) if r is None else r
        assert V.jpeg_header(h, w, quality=q, subsampling=ss, restart_interval=r, channels=c) == J.header(h, w, c, q, ss, rr), name
        assert V.default_restart_interval(h, w, ss, c) == J.default_restart(w, ss, c)
    with pytest.raises(ValueError):
        V.jpeg_header(8, 8, restart_interval=33)
    with pytest.raises(ValueError):
        V.jpeg_header(8, 8, subsampling='422')


def test_generated_kernel_tables_are_current():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_jpeg_tables.py'), '--check'])
    assert r.returncode == 0, 'csrc/jpeg_tables.h differs from what tools/gen_jpeg_tables.py generates'


def test_jpeg_params_structure_matches_the_header():
    """eg3d_jpeg_params of inv3d_amd/_lib.py against its C definition (gcc), as test_ctypes_structures_match_the_header does for the others."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {', ' printf("%zu\\n", sizeof(eg3d_jpeg_params));']
    want = [C.sizeof(L.JpegParams)]
    for f in L.JpegParams._fields_:
        src.append(f' printf("%zu\\n", offsetof(eg3d_jpeg_params, {f[0]}));')
        want.append(getattr(L.JpegParams, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_workspace_query_is_host_only_and_rejects_bad_arguments():
    """eg3d_jpeg_query_workspace answers without a GPU; the slot stride is the derived worst case: (22 + 63 * 26) bits per block, every byte
    stuffed, two marker bytes, rounded up to 16."""
    from inv3d_amd import _lib as L
    lib = L.lib()
    n = C.c_int64(0)

    def query(**kw):
        base = dict(N=1, C=3, H=512, W=512, dtype=L.JPEG_U8, subsampling=L.JPEG_420, quality=90, restart_interval=0)
        base.update(kw)
        return lib.eg3d_jpeg_query_workspace(C.byref(L.JpegParams(**base)), C.byref(n))
    assert query() == 0
    stride = -(-(2 * -(-(32 * 6 * (22 + 63 * 26)) // 8) + 2) // 16) * 16
    assert n.value == 6144 * 64 * 2 + 32 * stride + 32 * 4 + 32 * 8
    assert query(N=16) == 0 and n.value == 16 * (6144 * 64 * 2 + 32 * stride + 32 * 4 + 32 * 8)
    assert query(C=1, H=12, W=20) == 0                                   # 3 x 2 blocks, R = 3, 2 intervals
    s1 = -(-(2 * -(-(3 * (22 + 63 * 26)) // 8) + 2) // 16) * 16
    assert n.value == 6 * 64 * 2 + 2 * s1 + 16 + 16
    for bad in (dict(C=2), dict(H=0), dict(W=70000), dict(quality=0), dict(quality=101), dict(restart_interval=33), dict(restart_interval=-1),
                dict(dtype=2), dict(subsampling=2), dict(N=0)):
        assert query(**bad) == -1, bad                                   # EG3D_ERR_INVALID
    # encode / pack refuse null pointers before any launch
    p = L.JpegParams(N=1, C=3, H=8, W=8, dtype=L.JPEG_U8, subsampling=L.JPEG_444, quality=90)
    assert lib.eg3d_jpeg_encode(C.byref(p), None) == -1 and lib.eg3d_jpeg_pack(C.byref(p), None) == -1


def test_jpeg_encode_refuses_cpu_tensors():
    import torch
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    with pytest.raises(Eg3dHipError):
        H.jpeg_encode(torch.zeros(1, 3, 8, 8))


def _decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize('name', sorted(JC.cases()))
def test_every_restatement_stream_opens_in_pil(name):
    img, q, ss, r = JC.cases()[name]
    im = _decode(JC.reference(name))
    assert im.size == (img.shape[2], img.shape[1])
    assert im.mode == ('L' if img.shape[0] == 1 else 'RGB')
    got = np.asarray(im)
    if name == 'constant':
        assert np.all(got == 77)                                          # DC only, and 77 survives the colour round trip exactly
    if name == 'noise_q100_444':
        assert JC.reference(name).count(b'\xff\x00') > 100                # byte stuffing is exercised


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def _quality_inputs():
    s = JC.smooth(200, 160, 0)
    rng = np.random.RandomState(1)
    return dict(smooth=s, smooth_noise=np.clip(s.astype(np.int64) + rng.randint(-20, 21, s.shape), 0, 255).astype(np.uint8),
                noise=rng.randint(0, 256, s.shape).astype(np.uint8), crop=np.ascontiguousarray(s[:, 40:93, 60:97]))


_FLOAT_DCT = np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


@pytest.mark.parametrize('q', [50, 90, 100])
@pytest.mark.parametrize('ss', ['420', '444'])
def test_dct_rounding_and_psnr_against_pil(q, ss):
    """The integer DCT + quantiser never differs by more than 1 from round(float64 DCT / Q), on at most 8 % of the coefficients (measured: at
    most 6.1 %, at quality 100); decoded by PIL, the restatement's files are within 0.3 dB of PIL's own encoder with the same tables and
    subsampling (measured: between 0.35 dB better and 0.20 dB worse on these inputs; DESIGN.md 3.4 lists the values)."""
    qt = J.quant_tables(q)
    for name, img in _quality_inputs().items():
        comps, _ = J.planes(img, ss)
        differ = total = 0
        for a, t in comps:
            d = J.quantise(J.dct_unquantised(a), qt[t])
            s = (a - 128).reshape(a.shape[0] // 8, 8, a.shape[1] // 8, 8).transpose(0, 2, 1, 3).astype(np.float64)
            f = np.round(np.einsum('uy,abyx,vx->abuv', _FLOAT_DCT, s, _FLOAT_DCT) / qt[t])
            diff = np.abs(d - f)
            assert diff.max() <= 1, (name, diff.max())
            differ += int((diff != 0).sum())
            total += diff.size
        share = differ / total
        mine = np.asarray(_decode(J.encode(img, q, ss)).convert('RGB')).transpose(2, 0, 1)
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).save(bio, 'JPEG', qtables=[[int(v) for v in t.reshape(64)] for t in qt],
                                                                          subsampling=2 if ss == '420' else 0)
        pil = np.asarray(_decode(bio.getvalue())).transpose(2, 0, 1)
        p_mine, p_pil = _psnr(mine, img), _psnr(pil, img)
        print(f'q{q} {ss} {name}: share {share:.4f}  psnr {p_mine:.3f} dB  pil {p_pil:.3f} dB  shortfall {p_pil - p_mine:+.3f}')
        assert share <= 0.08, (name, share)
        assert p_mine >= p_pil - 0.3, (name, p_mine, p_pil)


# ---- AVI ------------------------------------------------------------------------------------------------------------------------------------
def walk_avi(data):
    """Parse a RIFF AVI: dict(avih=..., strh=..., strf=..., frames=[bytes], idx=[(ckid, flags, offset, size)], movi_start=offset of the 'movi'
    fourcc).  Asserts the structural invariants on the way: sizes add up, chunks are even-aligned."""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    out = dict(frames=[], idx=[], chunk_pos=[])

    def walk(lo, hi):
        i = lo
        while i < hi:
            assert i % 2 == 0, i
            cc, size = data[i:i + 4], struct.unpack('<I', data[i + 4:i + 8])[0]
            body = i + 8
            assert body + size <= hi, (cc, size)
            if cc == b'LIST':
                kind = data[body:body + 4]
                if kind == b'movi':
                    out['movi_start'], out['movi_size'] = body, size
                walk(body + 4, body + size)
            elif cc == b'00dc':
                out['frames'].append(data[body:body + size])
                out['chunk_pos'].append(i)
            elif cc == b'idx1':
                assert size % 16 == 0
                out['idx'] = [struct.unpack('<4sIII', data[body + 16 * k:body + 16 * k + 16]) for k in range(size // 16)]
            else:
                out[cc.decode().strip()] = data[body:body + size]
            i = body + size + (size & 1)
        assert i == hi or i == hi + 1, (i, hi)
    walk(12, len(data))
    return out


def check_avi(data, nframes, fps, width, height):
    a = walk_avi(data)
    avih = struct.unpack('<14I', a['avih'])
    assert avih[0] == 1000000 // fps and avih[4] == nframes and avih[6] == 1 and (avih[8], avih[9]) == (width, height) and avih[3] & 0x10
    strh = struct.unpack('<4s4sIHHIIIIIIIIhhhh', a['strh'])
    assert strh[0] == b'vids' and strh[1] == b'MJPG' and strh[7] / strh[6] == fps and strh[9] == nframes
    strf = struct.unpack('<IiiHH4sIiiII', a['strf'])
    assert strf[:6] == (40, width, height, 1, 24, b'MJPG')
    assert len(a['frames']) == nframes and len(a['idx']) == nframes
    assert avih[7] == strh[10] == max(len(f) for f in a['frames'])
    for k, (ckid, flags, off, size) in enumerate(a['idx']):
        pos = a['movi_start'] + off
        assert ckid == b'00dc' and flags & 0x10 and pos == a['chunk_pos'][k]
        assert data[pos:pos + 4] == b'00dc' and struct.unpack('<I', data[pos + 4:pos + 8])[0] == size == len(a['frames'][k])
    end = a['chunk_pos'][-1] + 8 + len(a['frames'][-1]) + (len(a['frames'][-1]) & 1)
    assert a['movi_size'] == end - a['movi_start']
    return a


def test_avi_round_trip(tmp_path):
    frames = [J.encode(JC.textured(24, 40, 20 + k), 90 - 20 * (k % 2), '420') for k in range(5)]
    if not any(len(f) & 1 for f in frames):
        frames[2] = J.encode(JC.textured(24, 40, 99), 77, '420')
    k = 100
    while not any(len(f) & 1 for f in frames):                            # an odd-length frame is part of the check: its chunk is padded
        frames[2] = J.encode(JC.noise(3, 24, 40, k), 90, '420')
        k += 1
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)
    path = str(tmp_path / 'a.avi')
    with V.MjpegAviWriter(path, 40, 24, fps=30) as w:
        for f in frames:
            w.write(f)
    data = open(path, 'rb').read()
    a = check_avi(data, 5, 30, 40, 24)
    assert a['frames'] == frames
    for f in a['frames']:
        im = _decode(f)
        assert im.size == (40, 24) and im.mode == 'RGB'


@pytest.mark.parametrize('width', [1, 7])
def test_png_round_trip(tmp_path, width):
    rng = np.random.RandomState(width)
    for shape in ((5, width, 3), (3, width)):
        a = rng.randint(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / f'{len(shape)}.png')
        V.write_png(path, a)
        im = Image.open(path)
        assert im.mode == ('RGB' if len(shape) == 3 else 'L') and im.size == (width, shape[0])
        assert np.array_equal(np.asarray(im), a)
    with pytest.raises(ValueError):
        V.write_png(str(tmp_path / 'x.png'), np.zeros((2, 2, 3), np.float32))


def test_pivot_grid_cameras_equal_the_reference():
    """look_at_small() against tests/golden/pivot_cameras.npz, recorded from the reference's own look_at / gen_eyes
    (tests/golden/make_golden_pivot_cameras.py): the same fp32 operations in the same order, so the values are equal, not close."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'pivot_cameras.npz'))
    assert g['cams'].shape == (3, 16) and g['cams'].dtype == np.float32
    assert np.array_equal(V.look_at_small().numpy(), g['cams'])
    assert np.array_equal(np.array(V.small_eyes(), np.float32), g['eyes'])


def test_coach_media_switches_default_off_and_need_a_directory():
    import inspect
    from inv3d_amd.coach import InversionCoach, InversionResult
    sig = inspect.signature(InversionCoach.__init__).parameters
    assert [sig[k].default for k in ('save_grid', 'gen_video', 'media_dir', 'video_quality')] == [False, False, None, 90]
    assert list(sig)[-4:] == ['save_grid', 'gen_video', 'media_dir', 'video_quality']
    # the media paths are attributes with a None default that the coach fills in; the constructor's field list is unchanged
    assert 'grid_paths' not in InversionResult.__dataclass_fields__ and 'video_paths' not in InversionResult.__dataclass_fields__
    r = InversionResult('a', None, None, 0.0, 0.0, 0.0, 0, 0)
    assert r.grid_paths is None and r.video_paths is None
    with pytest.raises(ValueError):
        InversionCoach(None, save_grid=True)
    with pytest.raises(ValueError):
        InversionCoach(None, gen_video=True)
