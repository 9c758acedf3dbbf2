"""The PNG encoder on the GPU (csrc/png.hip, hipops.png_encode, video.write_png(encoder='gpu') / write_pngs, write_obj(png_encoder='gpu')): the
device bytes and offsets EQUAL those of the numpy restatement tests/support/png_ref.py for every case of tests/support/png_cases.py (the
arithmetic is integer only) and, independently of it, inflate with zlib and open in PIL to the pixels; batches, run-to-run and
normal-vs-deterministic-build identity, the packer's capacity guard, every refused argument, and the files end to end.

The Fibonacci limiter case has 21 symbols with counts F1 .. F21, end-of-block being the first 1 (28 655 bytes): with a twenty-first byte value
of count 1 beside end-of-block the merge's tie rule (leaf first) pairs the light leaves and the unrestricted depth is 11, not above 15."""
import io
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import png_cases as PC  # noqa: E402
import png_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _hwc(img):
    return img if img.ndim == 3 else img[:, :, None]


def _encode(imgs, **kw):
    from inv3d_amd import hipops as H
    x = imgs if isinstance(imgs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs))
    data, offsets = H.png_encode(x.to(DEV), **kw)
    torch.cuda.synchronize()
    n = x.shape[0] if x.dim() == 4 else 1
    assert data.dtype == torch.uint8 and data.is_cuda and offsets.dtype == torch.int64 and not offsets.is_cuda and offsets.shape == (n + 1,)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == data.numel()
    return data.cpu().numpy().tobytes(), offsets.tolist()


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if len(d) else n)


def _open(stream, img):
    from PIL import Image
    from inv3d_amd import video as V
    a = _hwc(img)
    return np.asarray(Image.open(io.BytesIO(V.png_container(stream, a.shape[0], a.shape[1], a.shape[2])))).reshape(a.shape)


@pytest.mark.parametrize('name', sorted(PC.cases()))
def test_bytes_equal_the_restatement(name):
    img, filt, bb = PC.cases()[name]
    got, off = _encode(img, filter=filt, block_bytes=bb)
    # independently of the restatement: zlib inflates it to rows that PIL un-filters to the pixels, and the Adler-32 is zlib's
    rows = zlib.decompress(got)
    assert len(rows) == img.shape[0] * (1 + _hwc(img).shape[1] * _hwc(img).shape[2])
    assert struct.unpack('>I', got[-4:])[0] == zlib.adler32(rows)
    assert np.array_equal(_open(got, img), _hwc(img))
    want = PC.reference(name)
    assert off == [0, len(want)], (off, len(want))
    assert got == want, _first_difference(got, want)


def test_the_cases_reach_what_they_are_for():
    """From the restatement: all five filter types win a row, the limiters are exercised, a block has no match, a block has two symbols."""
    plan = lambda name: P.block_plan(P.filtered_stream(*PC.cases()[name][:2])[0])      # noqa: E731
    assert set(P.filtered_stream(PC.five_winners(), -1)[1]) == {0, 1, 2, 3, 4}
    assert max(P.huffman_depths(plan('fibonacci_limiter')['lit'])[0].values()) > 15
    assert max(P.huffman_depths(plan('cl_limiter')['cl'])[0].values()) > 7
    assert plan('rgb_3x5_no_match')['dist_len'] == 0
    assert sum(1 for c in plan('grey_1x1_two_symbols')['lit'] if c) == 2
    assert {(w - 1) % 258 for w in (259, 260, 261, 262)} == {0, 1, 2, 3}


def test_batch_of_different_images():
    imgs = np.stack([P.image(45, 70, 30, 2), PC.noise(45, 70, 3, 31), np.full((45, 70, 3), 200, np.uint8)])
    for kw in (dict(), dict(filter='paeth', block_bytes=2048), dict(filter=-1, block_bytes=64)):
        got, off = _encode(imgs, **kw)
        assert all(b > a for a, b in zip(off, off[1:]))
        assert len(set(b - a for a, b in zip(off, off[1:]))) == 3             # streams of different lengths: the offsets are not a stride
        for i in range(3):
            one = got[off[i]:off[i + 1]]
            assert np.array_equal(_open(one, imgs[i]), imgs[i])               # each stream decodes on its own
            assert one == _encode(imgs[i], **kw)[0]
        want, woff = P.encode_batch(imgs, P_FILTER.get(kw.get('filter', -1), kw.get('filter', -1)), kw.get('block_bytes', 32768))
        assert got == want and off == list(woff)


P_FILTER = dict(adaptive=-1, none=0, sub=1, up=2, average=3, paeth=4)


def test_grey_input_shapes():
    g = P.image(20, 28, 4, 2)[:, :, 0]
    a = _encode(torch.from_numpy(g))
    assert a == _encode(torch.from_numpy(g[:, :, None])) == _encode(torch.from_numpy(g[None, :, :, None]))
    assert a[0] == P.encode(g) and np.array_equal(_open(a[0], g)[:, :, 0], g)
    rgb = P.image(20, 28, 4, 2)
    assert _encode(torch.from_numpy(rgb)) == _encode(torch.from_numpy(rgb[None]))


def test_two_runs_give_identical_bytes():
    imgs = np.stack([P.image(64, 80, s, 3) for s in range(4)])
    assert _encode(imgs, block_bytes=4096) == _encode(imgs, block_bytes=4096)


def test_both_builds_give_the_same_bytes():
    """csrc/png.hip holds no floating point: the deterministic build, in a fresh interpreter, prints the digests this process computes."""
    import png_digest
    here = png_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'png_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def test_pack_refuses_a_short_output_and_writes_nothing_past_the_end():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    imgs = torch.from_numpy(np.stack([P.image(37, 53, s, 2) for s in range(2)])).to(DEV)
    p, keep, offsets = H._png_begin(imgs, block_bytes=1024)
    total = int(offsets.cpu()[-1])
    want = P.encode_batch(imgs.cpu().numpy(), -1, 1024)[0]
    assert total == len(want)
    guard = 64
    out = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(Eg3dHipError):
        H._png_pack(p, out, total - 1, total)                                 # one short: an error before any launch
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # a caller that understates the total as well: the kernel itself stops at the capacity
    H._png_pack(p, out, total - 1, total - 1)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[:total - 1].tobytes() == want[:total - 1] and np.all(host[total - 1:] == 0xA5)
    H._png_pack(p, out, total, total)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[:total].tobytes() == want and np.all(host[total:] == 0xA5)
    del keep


def test_invalid_arguments_are_refused():
    import ctypes as C
    from inv3d_amd import hipops as H, _lib as L
    from inv3d_amd._lib import Eg3dHipError
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    for kw in (dict(filter=5), dict(filter=-2), dict(filter='best'), dict(block_bytes=63), dict(block_bytes=65537)):
        with pytest.raises(Eg3dHipError):
            H.png_encode(x, **kw)
    for bad in (torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=DEV), torch.zeros(1, 8, 8, 3, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV),
                torch.zeros(1, 0, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 1, 16385, 1, dtype=torch.uint8, device=DEV),
                torch.zeros(1, 16385, 1, 1, dtype=torch.uint8, device=DEV)):
        with pytest.raises(Eg3dHipError):
            H.png_encode(bad)
    # the C entry points themselves: codes, before any launch (the pointers below are never dereferenced)
    lib, n = L.lib(), C.c_int64(0)
    ok = dict(N=1, C=3, H=8, W=8, filter=-1, block_bytes=32768)
    INVALID, UNSUPPORTED, TOO_LARGE = -1, -2, -3                              # EG3D_ERR_* of include/eg3d_hip.h
    codes = {}
    for name, kw in (('C', dict(C=2)), ('N', dict(N=0)), ('H', dict(H=0)), ('W', dict(W=0)), ('filter', dict(filter=5)), ('bb_lo', dict(block_bytes=63)),
                     ('bb_hi', dict(block_bytes=65537)), ('H_big', dict(H=16385)), ('W_big', dict(W=16385)),
                     ('blocks', dict(N=2 ** 31 - 1, H=16384, W=16384, block_bytes=64)), ('rows', dict(N=2 ** 31 - 1, H=16384))):
        codes[name] = lib.eg3d_png_query_workspace(C.byref(L.PngParams(**dict(ok, **kw))), C.byref(n))
    assert lib.eg3d_png_query_workspace(C.byref(L.PngParams(**ok)), C.byref(n)) == 0 and n.value > 0
    assert lib.eg3d_png_query_workspace(C.byref(L.PngParams(**ok)), None) != 0 and lib.eg3d_png_query_workspace(None, C.byref(n)) != 0
    assert all(codes[k] == INVALID for k in ('C', 'N', 'H', 'W', 'filter', 'bb_lo', 'bb_hi')), codes
    assert codes['H_big'] == codes['W_big'] == UNSUPPORTED and codes['blocks'] == codes['rows'] == TOO_LARGE, codes
    ws = torch.zeros(n.value + 16, dtype=torch.uint8, device=DEV)
    off = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    good = dict(ok, img=x.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=n.value, offsets=off.data_ptr())
    for kw in (dict(img=None), dict(workspace=None), dict(offsets=None), dict(workspace_bytes=n.value - 1), dict(workspace=ws.data_ptr() + 4)):
        assert lib.eg3d_png_encode(C.byref(L.PngParams(**dict(good, **kw))), L.stream_ptr()) == INVALID
        assert lib.eg3d_png_pack(C.byref(L.PngParams(**dict(good, **kw))), L.stream_ptr()) == INVALID
    assert lib.eg3d_png_pack(C.byref(L.PngParams(out=None, out_capacity=5, total_bytes=5, **good)), L.stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert off.tolist() == [-7, -7]                                           # nothing ran


def test_files_end_to_end(tmp_path):
    from PIL import Image
    from inv3d_amd import inference as INF, video as V
    img = P.image(96, 128, 3, 2)
    gpu, host = str(tmp_path / 'gpu.png'), str(tmp_path / 'host.png')
    V.write_png(gpu, torch.from_numpy(img).to(DEV), encoder='gpu')
    V.write_png(host, img, encoder='host')
    assert np.array_equal(np.asarray(Image.open(gpu)), img) and Image.open(gpu).mode == 'RGB'
    assert os.path.getsize(gpu) < os.path.getsize(host)
    assert open(gpu, 'rb').read() == V.png_container(P.encode(img), 96, 128, 3)
    grey = str(tmp_path / 'grey.png')
    V.write_png(grey, img[:, :, 1], encoder='gpu')                            # a numpy array is uploaded
    assert np.array_equal(np.asarray(Image.open(grey)), img[:, :, 1]) and Image.open(grey).mode == 'L'
    batch = np.stack([P.image(40, 56, s, 3) for s in range(3)])
    paths = [str(tmp_path / f'b{i}.png') for i in range(3)]
    V.write_pngs(paths, torch.from_numpy(batch).to(DEV))
    for i, path in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(path)), batch[i])
    with pytest.raises(ValueError):
        V.write_pngs(paths[:2], batch)
    # a tiny textured mesh: one quad, a 2 x 2-cell atlas
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.array([[[0.1, 0.1], [0.4, 0.1], [0.4, 0.4]], [[0.6, 0.6], [0.9, 0.9], [0.6, 0.9]]], np.float32)
    atlas = P.image(32, 48, 9, 4)
    obj, mtl, tex = INF.write_obj(str(tmp_path / 'm.obj'), verts, faces, uv, torch.from_numpy(atlas).to(DEV), png_encoder='gpu')
    assert tex.endswith('m.png') and np.array_equal(np.asarray(Image.open(tex)), atlas)
    assert 'map_Kd m.png' in open(mtl).read() and 'mtllib m.mtl' in open(obj).read()
    obj2, _, tex2 = INF.write_obj(str(tmp_path / 'h.obj'), verts, faces, uv, atlas)
    assert np.array_equal(np.asarray(Image.open(tex2)), atlas) and open(obj2).read().replace('h.mtl', 'm.mtl').replace('usemtl h', 'usemtl m') == open(obj).read()


def test_align_images_tool_with_gpu_pngs(tmp_path):
    """tools/align_images.py --png-gpu: the aligned frames of a directory go through one batched encode (three frames, batches of at most
    eight) and the files hold align_face's bytes, as the host-encoded ones do; they are the smaller files."""
    from PIL import Image
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import align_images
    import test_align_cpu as TC
    cases = TC.align_cases()
    names = ['pad_edge', 'shrink', 'inside']
    d = tmp_path / 'photos'
    d.mkdir()
    for n in names:
        V.write_png(str(d / (n + '.png')), cases[n]['image'])
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, **{n: cases[n]['landmarks'] for n in names})
    out_gpu, out_host = str(tmp_path / 'gpu'), str(tmp_path / 'host')
    written = align_images.main(['--in-dir', str(d), '--landmarks', lm_path, '--out-dir', out_gpu, '--output-size', '32', '--png-gpu'])
    align_images.main(['--in-dir', str(d), '--landmarks', lm_path, '--out-dir', out_host, '--output-size', '32'])
    assert sorted(os.listdir(out_gpu)) == sorted(n + '.png' for n in names) and len(written) == 3
    for n in names:
        want = images.align_face(torch.from_numpy(cases[n]['image']).to(DEV), cases[n]['landmarks'], 32).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(os.path.join(out_gpu, n + '.png'))), want)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out_host, n + '.png'))), want)
        assert open(os.path.join(out_gpu, n + '.png'), 'rb').read() == V.png_container(P.encode(want), 32, 32, 3)
