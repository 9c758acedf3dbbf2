"""The batched JPEG decode on the GPU (eg3d_jpegdec_batch_*, hipops.jpeg_decode_batch) and what stands on it (video.read_mjpeg_frames,
images.decode_rgb_batch / load_targets / write_aligned with decode_batch, images.video_targets): every case of tests/support/jpegdec_cases.py
in ONE call EQUALS the numpy restatement and PIL, with the per-image result words of the one-image call; the order of a batch, a
multi-workgroup file beside one-block files, N = 1, 2 and 1025 change no byte; a damaged or unsupported file in the middle of a batch ends
in its own status and leaves its neighbours alone; run-to-run and normal-vs-deterministic-build identity; Motion-JPEG files read back to
PIL's pixels, with and without DHT; the consumers give what the PIL path gives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import jpeg_cases as JC  # noqa: E402
import jpegbatch_cases as BC  # noqa: E402
import jpegdec_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = list(DC.cases())


def _batch(files, **kw):
    from inv3d_amd import hipops as H
    outs = H.jpeg_decode_batch(files, **kw)
    assert len(outs) == len(files)
    for o in outs:
        if isinstance(o, torch.Tensor):
            assert o.is_cuda and o.dtype == torch.uint8 and o.dim() == 3 and o.shape[2] == 3 and o.is_contiguous()
    return outs


def _check_names(names, outs):
    for name, o in zip(names, outs):
        got, pil = o.cpu().numpy(), DC.pil_decode(name)
        assert got.shape == pil.shape and np.array_equal(got, pil), f'{name}: differs from PIL'


@pytest.mark.parametrize('B', DC.SUBSEQ)
def test_all_cases_in_one_batch(B):
    from inv3d_amd import hipops as H
    assert len(NAMES) == 57
    stats = []
    outs = _batch([DC.cases()[n] for n in NAMES], subseq_bytes=B, stats=stats)
    assert len(stats) == len(NAMES)
    for name, o, s in zip(NAMES, outs, stats):
        got, want, pil = o.cpu().numpy(), DC.ref_decode(name), DC.pil_decode(name)
        assert got.shape == want.shape == pil.shape, name
        assert np.array_equal(got, want), f'{name}: {int((got != want).sum())} bytes differ from the restatement'
        assert np.array_equal(got, pil), f'{name}: {int((got != pil).sum())} bytes differ from PIL'
        single = {}
        one = H.jpeg_decode(DC.cases()[name], subseq_bytes=B, stats=single)
        assert s == single and s['status'] == 0 and s['lanes'] >= 1, (name, s, single)
        assert torch.equal(one, o), name
    assert max(s['rounds_workgroup'] for s in stats) >= 2 and stats[NAMES.index(DC.BIG)]['lanes'] > 4 * 256      # the serial rounds really ran


def test_order_and_n_edges():
    files = [DC.cases()[n] for n in NAMES]
    _check_names(NAMES[::-1], _batch(files[::-1]))
    rest = [n for n in NAMES if n != DC.BIG][:9]
    for names in ([DC.BIG] + rest, rest + [DC.BIG]):                              # the multi-workgroup file sets the grid; the others leave early
        for B in DC.SUBSEQ:
            _check_names(names, _batch([DC.cases()[n] for n in names], subseq_bytes=B))
    _check_names(['37x53_420'], _batch([DC.cases()['37x53_420']]))
    _check_names(['1x1_420', DC.BIG], _batch([DC.cases()['1x1_420'], DC.cases()[DC.BIG]]))
    assert _batch([]) == []


def test_more_images_than_one_workgroup_has_threads():
    files, want = BC.tiny_files(1025)
    assert len(set(files)) > 1000 and max(len(f) for f in files) < 1000
    stats = []
    outs = _batch(list(files), stats=stats)
    flat = torch.cat([o.reshape(-1) for o in outs]).cpu().numpy()                   # one copy
    assert np.array_equal(flat, np.concatenate([w.reshape(-1) for w in want]))
    assert [o.shape for o in outs] == [w.shape for w in want]
    assert all(s['status'] == 0 and s['lanes'] == 1 for s in stats)


def test_damaged_and_unsupported_files_in_a_batch():
    """A stray restart marker, a truncated segment and a progressive file between good files: each damaged file's status is the one-image
    call's, it comes back as JpegDecodeRefused (return_errors=True) or raises, and its neighbours equal PIL."""
    from inv3d_amd import hipops as H, video as V
    good = ['40x72_420', 'noise_q100_444', DC.BIG, 'grey_20x12']
    damaged = {'stray': BC.stray_marker(DC.cases()['textured_q90_420']), 'half': BC.truncated(DC.cases()['restart3_64x48_444']),
               'half_big': BC.truncated(DC.cases()[DC.BIG])}
    for B in DC.SUBSEQ:
        single = {}
        for k, f in damaged.items():
            single[k] = {}
            with pytest.raises(H.JpegDecodeRefused):
                H.jpeg_decode(f, subseq_bytes=B, stats=single[k])
            assert single[k]['status'] != 0
        files = [DC.cases()[good[0]], damaged['stray'], DC.cases()[good[1]], BC.progressive_file(), damaged['half'], DC.cases()[good[2]],
                 damaged['half_big'], DC.cases()[good[3]]]
        stats = []
        outs = _batch(files, subseq_bytes=B, stats=stats, return_errors=True)
        _check_names(good, [outs[0], outs[2], outs[5], outs[7]])
        for i, k in ((1, 'stray'), (4, 'half'), (6, 'half_big')):
            assert isinstance(outs[i], H.JpegDecodeRefused) and outs[i].status == single[k]['status'] == stats[i]['status']
            assert stats[i] == single[k], (k, stats[i], single[k])
        assert isinstance(outs[3], V.JpegUnsupported) and 'progressive' in str(outs[3]) and stats[3] is None
        assert all(stats[i]['status'] == 0 for i in (0, 2, 5, 7))
    with pytest.raises(H.JpegDecodeRefused):
        _batch([DC.cases()[good[0]], damaged['stray'], DC.cases()[good[1]]])
    with pytest.raises(V.JpegUnsupported):
        _batch([DC.cases()[good[0]], BC.progressive_file()])
    torch.cuda.synchronize()
    _check_names(good, _batch([DC.cases()[n] for n in good]))                       # and the next batch is fine


def test_two_runs_and_the_deterministic_build_give_the_same_digests():
    """csrc/jpeg_decode.hip holds no floating point: two runs here agree, and the deterministic build, in a fresh interpreter, prints the
    digests this process computes, for all cases in one batch."""
    import jpegbatch_digest
    here = jpegbatch_digest.digests()
    assert jpegbatch_digest.digests() == here and len(here) == 1 + 2 * len(NAMES)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'jpegbatch_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def test_mjpeg_frames_read_back(tmp_path):
    """5 frames of 64 x 48 from the GPU encoder through MjpegAviWriter: read_mjpeg_frames(batch=2) equals PIL's decode of every frame, with
    the frames' DHT segments stripped too, and start / stop / step select the right frames."""
    from inv3d_amd import hipops as H, video as V
    imgs = np.stack([JC.textured(48, 64, 130 + i) for i in range(5)])
    data, offsets = H.jpeg_encode(torch.from_numpy(imgs).to(DEV), quality=90)
    host, off = data.cpu().numpy().tobytes(), offsets.tolist()
    frames = [host[off[i]:off[i + 1]] for i in range(5)]
    for label, fs in (('full', frames), ('nodht', [BC.strip_dht(f) for f in frames])):
        path = str(tmp_path / f'{label}.avi')
        BC.write_avi(path, fs, 64, 48, 30)
        want = [BC.pil_rgb(f) for f in fs]
        assert all(np.array_equal(a, b) for a, b in zip(want, [BC.pil_rgb(f) for f in frames]))
        told = []
        blocks = list(V.read_mjpeg_frames(path, batch=2, device=DEV, report=lambda i, why: told.append((i, why))))
        assert [(first, tuple(b.shape)) for first, b in blocks] == [(0, (2, 48, 64, 3)), (2, (2, 48, 64, 3)), (4, (1, 48, 64, 3))] and told == []
        got = torch.cat([b for _, b in blocks]).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, np.stack(want))
        sel = list(V.read_mjpeg_frames(path, start=1, stop=5, step=2, batch=4, device=DEV))
        assert len(sel) == 1 and sel[0][0] == 1 and np.array_equal(sel[0][1].cpu().numpy(), np.stack([want[1], want[3]]))
        pil = list(V.read_mjpeg_frames(path, batch=3, device=DEV, decoder='pil'))
        assert np.array_equal(torch.cat([b for _, b in pil]).cpu().numpy(), got)
    # a frame the device refuses goes through PIL's rule: PIL raises on it here or gives pixels; either way the report names the frame
    path = str(tmp_path / 'mixed.avi')
    prog = DC.pil_file(imgs[1], 85, 2, progressive=True)
    BC.write_avi(path, [frames[0], prog, frames[2]], 64, 48, 30)
    told = []
    (first, block), = list(V.read_mjpeg_frames(path, batch=8, device=DEV, report=lambda i, why: told.append((i, why))))
    assert first == 0 and len(told) == 1 and told[0][0] == 1 and 'progressive' in told[0][1]
    assert np.array_equal(block.cpu().numpy(), np.stack([BC.pil_rgb(frames[0]), BC.pil_rgb(prog), BC.pil_rgb(frames[2])]))


def _mixed_dir(tmp_path):
    """JPEGs of different sizes and samplings (two with landmarks), a PNG and a progressive JPEG"""
    from PIL import Image
    import test_align_cpu as TC
    cases = TC.align_cases()
    d = tmp_path / 'photos'
    d.mkdir()
    lms = {}
    for n, ss in (('shrink', 2), ('inside', 0), ('crop_only', 1)):
        open(str(d / (n + '.jpg')), 'wb').write(DC.pil_file(np.transpose(cases[n]['image'], (2, 0, 1)), 92, ss))
        lms[n] = cases[n]['landmarks']
    Image.fromarray(cases['pad_edge']['image']).save(str(d / 'pad_edge.png'))
    lms['pad_edge'] = cases['pad_edge']['landmarks']
    open(str(d / 'shrink_pad.jpeg'), 'wb').write(DC.pil_file(np.transpose(cases['shrink_pad']['image'], (2, 0, 1)), 90, 2, progressive=True))
    lms['shrink_pad'] = cases['shrink_pad']['landmarks']
    return str(d), lms


def test_consumers_with_the_batched_decode(tmp_path):
    from inv3d_amd import images
    d, lms = _mixed_dir(tmp_path)
    paths = [p for _, p in images.image_files(d)]
    assert len(paths) == 5
    told = []
    a = images.decode_rgb_batch(paths, DEV)
    b = images.decode_rgb_batch(paths, DEV, decoder='gpu', report=lambda p, why: told.append((os.path.basename(p), why)))
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert len(told) == 1 and told[0][0] == 'shrink_pad.jpeg' and 'progressive' in told[0][1]
    told.clear()
    ta = images.load_targets(d, lms, output_size=32, device=DEV)
    tb = images.load_targets(d, lms, output_size=32, device=DEV, decoder='gpu', decode_report=lambda p, why: told.append(p), decode_batch=4)
    assert [n for n, _, _ in ta] == [n for n, _, _ in tb] == sorted(lms) and len(told) == 1
    assert all(torch.equal(x, y) for (_, x, _), (_, y, _) in zip(ta, tb))
    told.clear()
    del lms['crop_only']                                                            # a file without landmarks: reported and skipped, as before
    skipped = []
    w1 = images.write_aligned(d, lms, str(tmp_path / 'pil'), output_size=32, device=DEV, png_encoder='gpu')
    w2 = images.write_aligned(d, lms, str(tmp_path / 'gpu'), output_size=32, device=DEV, png_encoder='gpu', decoder='gpu', decode_batch=3,
                              report=skipped.append, decode_report=lambda p, why: told.append(p))
    assert [os.path.basename(p) for p in w1] == [os.path.basename(p) for p in w2] and len(w1) == 4 and len(told) == 1 and len(skipped) == 1
    for p1, p2 in zip(w1, w2):
        assert open(p1, 'rb').read() == open(p2, 'rb').read()


def test_video_targets(tmp_path):
    """Frames of a 100 x 100 clip as targets: the frame with landmarks is aligned, the others are taken as they are; names carry the index."""
    import test_align_cpu as TC
    from inv3d_amd import hipops as H, images
    case = TC.align_cases()['inside']
    img = case['image']
    assert img.shape == (100, 100, 3)
    frames = [DC.pil_file(np.transpose(np.roll(img, i, axis=1), (2, 0, 1)), 92, 2) for i in range(4)]
    path = str(tmp_path / 'head.clip.avi')
    BC.write_avi(path, frames, 100, 100, 24)
    out = images.video_targets(path, {'head_000001': case['landmarks']}, output_size=100, device=DEV, batch=3)
    assert [n for n, _, _ in out] == [f'head_{i:06d}' for i in range(4)] and all(c is None for _, _, c in out)
    for i, (_, t, _) in enumerate(out):
        px = torch.from_numpy(BC.pil_rgb(frames[i])).to(DEV)
        if i == 1:
            px = images.align_face(px, case['landmarks'], 100)
        assert t.shape == (1, 3, 100, 100) and torch.equal(t, H.u8_to_target(px))
    sub = images.video_targets(path, None, frames=slice(1, None, 2), output_size=100, device=DEV)
    assert [n for n, _, _ in sub] == ['head_000001', 'head_000003'] and torch.equal(sub[1][1], out[3][1])
    with pytest.raises(ValueError, match='no landmarks'):
        images.video_targets(path, None, output_size=64, device=DEV)
