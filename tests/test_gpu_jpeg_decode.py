"""The JPEG decoder on the GPU (csrc/jpeg_decode.hip, hipops.jpeg_decode, images.decode_rgb(decoder='gpu')): the device pixels EQUAL those of
the numpy restatement tests/support/jpegdec_ref.py and, independently, PIL's, for every case of tests/support/jpegdec_cases.py at both
subsequence sizes -- hipops.jpeg_decode is called directly, so no fallback can hide a failure; the synchronisation rounds really run; the
round trip through the project's own encoder; a damaged stream ends in a status; run-to-run and normal-vs-deterministic-build identity;
load_targets / write_aligned / the align tool give what the PIL path gives."""
import io
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
import jpegdec_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_rounds = {}


def _decode(data, B, stats=None):
    from inv3d_amd import hipops as H
    out = H.jpeg_decode(data, subseq_bytes=B, stats=stats)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 3 and out.shape[2] == 3 and out.is_contiguous()
    return out.cpu().numpy()


@pytest.mark.parametrize('B', DC.SUBSEQ)
@pytest.mark.parametrize('name', list(DC.cases()))
def test_device_equals_restatement_and_pil(name, B):
    stats = {}
    got = _decode(DC.cases()[name], B, stats)
    print(name, B, stats)
    _rounds[(name, B)] = stats
    want, pil = DC.ref_decode(name), DC.pil_decode(name)
    assert got.shape == want.shape == pil.shape
    assert np.array_equal(got, want), f'{int((got != want).sum())} bytes differ from the restatement'
    assert np.array_equal(got, pil), f'{int((got != pil).sum())} bytes differ from PIL'
    assert stats['status'] == 0 and stats['lanes'] >= 1


def test_synchronisation_rounds_run():
    """The fixed-point loop is alive: some case needs two rounds or more inside a workgroup, the big file spans several workgroups at the
    default subsequence size and its lanes do not all start synchronised; lanes and restart markers are what the files' geometry says."""
    from inv3d_amd import video as V
    for name in ('37x53_420', DC.BIG, 'restart1_64x48_420'):
        for B in DC.SUBSEQ:
            if (name, B) not in _rounds:
                _rounds[(name, B)] = {}
                _decode(DC.cases()[name], B, _rounds[(name, B)])
    print({k: (v['rounds_workgroup'], v['rounds_across'], v['lanes']) for k, v in _rounds.items()})
    assert max(v['rounds_workgroup'] for v in _rounds.values()) >= 2
    assert _rounds[('37x53_420', 16)]['rounds'] >= 2 and _rounds[('37x53_420', 16)]['lanes'] > 64
    big = _rounds[(DC.BIG, 128)]
    p = V.jpeg_scan_plan(DC.cases()[DC.BIG])
    assert big['lanes'] == -(-big['unstuffed_bytes'] // 128) > 4 * 256 and big['rounds'] >= 2
    assert big['unstuffed_bytes'] == (p.scan_end - p.scan_start) - DC.cases()[DC.BIG][p.scan_start:p.scan_end].count(b'\xff\x00')
    r1 = _rounds[('restart1_64x48_420', 128)]
    assert r1['restart_markers'] == 11 and r1['lanes'] >= 12


@pytest.mark.parametrize('kw', [dict(subsampling='420'), dict(subsampling='444'), dict(subsampling='420', grey=True), dict(subsampling='420', quality=35, batch=True)])
def test_round_trip_through_the_gpu_encoder(kw):
    from PIL import Image
    from inv3d_amd import hipops as H
    kw = dict(kw)
    grey, batch = kw.pop('grey', False), kw.pop('batch', False)
    imgs = np.stack([JC.textured(70, 90, 80 + i)[:1 if grey else 3] for i in range(2 if batch else 1)])
    data, offsets = H.jpeg_encode(torch.from_numpy(imgs).to(DEV), **kw)
    host, off = data.cpu().numpy().tobytes(), offsets.tolist()
    for i in range(len(imgs)):
        f = host[off[i]:off[i + 1]]
        want = np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
        for B in DC.SUBSEQ:
            assert np.array_equal(_decode(f, B), want)
    assert np.array_equal(_decode(torch.frombuffer(bytearray(host[off[0]:off[1]]), dtype=torch.uint8), 128), np.asarray(Image.open(io.BytesIO(host[off[0]:off[1]])).convert('RGB')))


def test_damaged_stream_ends_in_a_status(tmp_path):
    """Half the entropy-coded segment with EOI re-appended: a non-zero status as Eg3dHipError (the guarded stores and zero-padded reads make
    it so), and decode_rgb(decoder='gpu') then gives what PIL gives or raises what PIL raises."""
    from PIL import Image
    from inv3d_amd import hipops as H, images, video as V
    from inv3d_amd._lib import Eg3dHipError
    for name in ('textured_q90_420', 'restart3_64x48_444', DC.BIG):
        data = DC.cases()[name]
        p = V.jpeg_scan_plan(data)
        half = data[:p.scan_start + (p.scan_end - p.scan_start) // 2] + b'\xff\xd9'
        for B in DC.SUBSEQ:
            stats = {}
            with pytest.raises(Eg3dHipError):
                H.jpeg_decode(half, subseq_bytes=B, stats=stats)
            assert stats['status'] != 0
        path = str(tmp_path / (name + '.jpg'))
        open(path, 'wb').write(half)
        told = []
        try:
            with Image.open(path) as im:
                want = np.asarray(im.convert('RGB'))
        except Exception as e:
            with pytest.raises(type(e)):
                images.decode_rgb(path, DEV, decoder='gpu')
        else:
            got = images.decode_rgb(path, DEV, decoder='gpu', report=lambda f, why: told.append(why))
            assert np.array_equal(got.cpu().numpy(), want) and len(told) == 1 and 'status' in told[0]
    stray = bytearray(DC.cases()['textured_q90_420'])
    p = V.jpeg_scan_plan(bytes(stray))
    stray[p.scan_start + 40:p.scan_start + 42] = b'\xff\xd3'                        # a restart marker the geometry does not have
    with pytest.raises(Eg3dHipError):
        H.jpeg_decode(bytes(stray))
    torch.cuda.synchronize()
    assert np.array_equal(_decode(DC.cases()['textured_q90_420'], 128), DC.pil_decode('textured_q90_420'))             # and the next decode is fine


def test_two_runs_are_bit_identical():
    for name in ('40x72_420', 'noise_q100_444', DC.BIG):
        for B in DC.SUBSEQ:
            s1, s2 = {}, {}
            a, b = _decode(DC.cases()[name], B, s1), _decode(DC.cases()[name], B, s2)
            assert np.array_equal(a, b) and s1 == s2


def test_deterministic_build_gives_the_same_digests():
    """csrc/jpeg_decode.hip holds no floating point: the deterministic build, in a fresh interpreter, prints the digests this process computes."""
    import jpegdec_digest
    here = jpegdec_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'jpegdec_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def _photo_dir(tmp_path):
    """two JPEG photographs of the alignment cases (4:2:0 and 4:4:4) with their landmarks"""
    import test_align_cpu as TC
    cases = TC.align_cases()
    names = ['shrink', 'inside']
    d = tmp_path / 'photos'
    d.mkdir()
    for n, ss in zip(names, (2, 0)):
        open(str(d / (n + '.jpg')), 'wb').write(DC.pil_file(np.transpose(cases[n]['image'], (2, 0, 1)), 92, ss))
    return str(d), {n: cases[n]['landmarks'] for n in names}, names


def test_load_targets_and_write_aligned_with_the_gpu_decoder(tmp_path):
    from inv3d_amd import images
    d, lms, names = _photo_dir(tmp_path)
    told = []
    a = images.load_targets(d, lms, output_size=32, device=DEV)
    b = images.load_targets(d, lms, output_size=32, device=DEV, decoder='gpu', decode_report=lambda p, why: told.append(p))
    assert [n for n, _, _ in a] == [n for n, _, _ in b] == sorted(names) and told == []
    for (_, x, _), (_, y, _) in zip(a, b):
        assert torch.equal(x, y)
    for enc in ('host', 'gpu'):
        w1 = images.write_aligned(d, lms, str(tmp_path / f'pil_{enc}'), output_size=32, device=DEV, png_encoder=enc)
        w2 = images.write_aligned(d, lms, str(tmp_path / f'gpu_{enc}'), output_size=32, device=DEV, png_encoder=enc, decoder='gpu',
                                  decode_report=lambda p, why: told.append(p))
        assert [os.path.basename(p) for p in w1] == [os.path.basename(p) for p in w2] and len(w1) == 2 and told == []
        for p1, p2 in zip(w1, w2):
            assert open(p1, 'rb').read() == open(p2, 'rb').read()


def test_tools_take_jpeg_gpu(tmp_path):
    """--jpeg-gpu on tools/align_images.py and tools/paste_back.py: the same files as without it."""
    d, lms, names = _photo_dir(tmp_path)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import align_images
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, **lms)
    out = {}
    for flag in ((), ('--jpeg-gpu',)):
        out[flag] = str(tmp_path / ('aligned' + '_'.join(flag)))
        written = align_images.main(['--in-dir', d, '--landmarks', lm_path, '--out-dir', out[flag], '--output-size', '32', *flag])
        assert len(written) == 2
    for n in names:
        assert open(os.path.join(out[()], n + '.png'), 'rb').read() == open(os.path.join(out[('--jpeg-gpu',)], n + '.png'), 'rb').read()
    import paste_back
    from PIL import Image
    edit = str(tmp_path / 'edit.jpg')
    Image.open(os.path.join(out[()], names[0] + '.png')).save(edit, 'JPEG', quality=95, subsampling=1)               # a 4:2:2 edit
    res = {}
    for flag in ((), ('--jpeg-gpu',)):
        res[flag] = str(tmp_path / ('pasted' + '_'.join(flag)))
        written = paste_back.main(['--photo', os.path.join(d, names[0] + '.jpg'), '--landmarks', lm_path, '--edit', edit, '--out-dir', res[flag], *flag])
        assert [os.path.basename(w) for w in written] == ['edit.png']
    assert open(os.path.join(res[()], 'edit.png'), 'rb').read() == open(os.path.join(res[('--jpeg-gpu',)], 'edit.png'), 'rb').read()


def test_run_inversion_tool_takes_jpeg_gpu(tmp_path, monkeypatch):
    """tools/run_inversion.py --jpeg-gpu (in process, the small synthetic generator, one step per phase): the photograph goes through
    hipops.jpeg_decode, and the target the coach gets is the PIL path's (load_targets above)."""
    from inv3d_amd import hipops as H
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_inversion
    d, lms, names = _photo_dir(tmp_path)
    os.remove(os.path.join(d, names[0] + '.jpg'))
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, **lms)
    calls, real = [], H.jpeg_decode
    monkeypatch.setattr(H, 'jpeg_decode', lambda data, **kw: (calls.append(len(data)), real(data, **kw))[1])
    results, stats = run_inversion.main(['--in-dir', d, '--landmarks', lm_path, '--out-dir', str(tmp_path / 'out'), '--synthetic', 'small', '--steps-a', '1',
                                         '--steps-b', '1', '--jpeg-gpu'])
    assert [r.name for r in results] == [names[1]] and stats['n_done'] == 1 and len(calls) == 1
