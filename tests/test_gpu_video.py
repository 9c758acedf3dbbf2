"""Media export on the GPU (csrc/jpeg.hip, hipops.jpeg_encode, inv3d_amd/video.py, the coach's save_grid / gen_video): the encoder's bytes EQUAL
those of the numpy restatement tests/support/jpeg_ref.py for every case of tests/support/jpeg_cases.py (the arithmetic is integer only), batches,
fp32 input, run-to-run and normal-vs-deterministic-build identity, the orbit video and the four files of a coach run."""
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
import jpeg_ref as J  # noqa: E402
from test_video_cpu import check_avi  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _encode(imgs, **kw):
    from inv3d_amd import hipops as H
    x = imgs if isinstance(imgs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs))
    data, offsets = H.jpeg_encode(x.to(DEV), **kw)
    torch.cuda.synchronize()
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.shape == (x.shape[0] + 1,)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == data.numel()
    return data.cpu().numpy().tobytes(), offsets.tolist()


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if len(d) else n)


@pytest.mark.parametrize('name', sorted(JC.cases()))
def test_bytes_equal_the_restatement(name):
    img, q, ss, r = JC.cases()[name]
    want = JC.reference(name)
    got, off = _encode(img[None], quality=q, subsampling=ss, restart_interval=r)
    assert off == [0, len(want)], (off, len(want))
    assert got == want, _first_difference(got, want)
    if name == 'noise_q100_444':
        assert got.count(b'\xff\x00') > 100                                # several hundred stuffed bytes went through the kernel
    if name == '24x160_r1':
        assert b'\xff\xd7' in got and got.count(b'\xff\xd0') >= 3          # the RSTm index wrapped
    if name == 'constant':
        from PIL import Image
        assert np.all(np.asarray(Image.open(io.BytesIO(got))) == 77)


def test_batch_equals_single_calls():
    imgs = np.stack([JC.textured(45, 70, 30), JC.noise(3, 45, 70, 31), np.full((3, 45, 70), 200, np.uint8)])
    for kw in (dict(quality=90, subsampling='420'), dict(quality=50, subsampling='444', restart_interval=2)):
        got, off = _encode(imgs, **kw)
        singles = [_encode(imgs[i:i + 1], **kw)[0] for i in range(3)]
        assert off == [0] + list(np.cumsum([len(s) for s in singles]))
        assert got == b''.join(singles)
        want, woff = J.encode_batch(imgs, **kw)
        assert got == want and off == list(woff)
        assert len(set(len(s) for s in singles)) == 3                       # frames of different lengths: the offsets are not a stride


def test_fp32_input_is_quantised_as_image_grid_u8():
    from inv3d_amd import hipops as H
    rng = np.random.RandomState(7)
    x = torch.from_numpy(rng.uniform(-1.3, 1.3, (2, 3, 37, 53)).astype(np.float32))
    x[0, :, :4, :4] = torch.tensor([-1.0, 1.0, 0.0, 0.999])               # the ends of the range and the truncation
    xd = x.to(DEV)
    u8 = torch.stack([H.image_grid_u8(xd[i:i + 1], nrow=1, padding=0).permute(2, 0, 1) for i in range(2)])
    assert np.array_equal(u8.cpu().numpy(), J.quantise_input(x.numpy()))
    got, off = _encode(xd, quality=90)
    assert (got, off) == _encode(u8, quality=90)
    want, woff = J.encode_batch(x.numpy(), quality=90)
    assert got == want and off == list(woff)
    g = torch.from_numpy(rng.uniform(-1, 1, (1, 1, 20, 28)).astype(np.float32))      # grey, as image_depth frames arrive
    assert _encode(g, quality=90)[0] == J.encode(g.numpy()[0], 90)


def test_two_runs_give_identical_bytes():
    img, q, ss, r = JC.cases()['binary_noise_q100_420']
    a = _encode(img[None], quality=q, subsampling=ss, restart_interval=r)
    b = _encode(img[None], quality=q, subsampling=ss, restart_interval=r)
    assert a == b


def test_both_builds_give_the_same_bytes():
    """csrc/jpeg.hip accumulates nothing in floating point: the deterministic build, in a fresh interpreter, prints the digests this process computes."""
    import jpeg_digest
    here = jpeg_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'jpeg_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def test_invalid_arguments_are_refused():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    for kw in (dict(restart_interval=33), dict(restart_interval=0), dict(quality=0), dict(subsampling='422')):
        with pytest.raises(Eg3dHipError):
            H.jpeg_encode(x, **kw)
    for bad in (torch.zeros(1, 2, 8, 8, device=DEV), torch.zeros(3, 8, 8, device=DEV), torch.zeros(1, 3, 8, 8, device=DEV, dtype=torch.float16)):
        with pytest.raises(Eg3dHipError):
            H.jpeg_encode(bad)


def _small_generator():
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    for p in G.parameters():
        p.requires_grad_(False)
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    ws = O.synth_ws(cfg, 1, seed=7).to(DEV)
    with torch.no_grad():
        target = G.synthesis(ws, cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    uni = tuple(u.to(DEV) for u in O.make_uniforms(cfg, 1, seed=4))        # pinned stratified-sampling draws: two renders give the same frame
    return G, ws, cam, target, uni


@pytest.mark.parametrize('image_mode', ['image', 'image_depth'])
def test_orbit_video(tmp_path, image_mode):
    from inv3d_amd import hipops as H, inference as INF, video as V
    G, ws, _, _, uni = _small_generator()
    path = str(tmp_path / 'orbit.avi')
    n = V.write_orbit_video(G, ws, path, num_frames=5, image_mode=image_mode, fps=60, quality=85, batch=2, force_fp32=True, render_uniforms=uni)
    assert n == 5
    frames = list(INF.render_orbit(G, ws, num_frames=5, image_mode=image_mode, force_fp32=True, render_uniforms=uni))
    hh, ww = frames[0].shape[-2:]
    a = check_avi(open(path, 'rb').read(), 5, 60, ww, hh)
    from PIL import Image
    for f, got in zip(frames, a['frames']):
        data, off = H.jpeg_encode(f[None].float(), quality=85)
        assert got == data.cpu().numpy().tobytes()
        im = Image.open(io.BytesIO(got))
        im.load()
        assert im.size == (ww, hh) and im.mode == ('RGB' if image_mode == 'image' else 'L')


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_coach_media(tmp_path):
    from inv3d_amd import video as V
    from inv3d_amd.coach import InversionCoach
    G, _, cam, target, uni = _small_generator()
    kw = dict(first_inv_steps=3, max_pti_steps=3, lpips_threshold=0.0, seed=3, w_avg_samples=0, keep_tuned_state=True, synth_kwargs=dict(render_uniforms=uni))
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    # default: no file, no paths
    r0 = InversionCoach(G, **kw).invert('a', target, cam)
    assert r0.grid_paths is None and r0.video_paths is None and os.listdir(tmp_path) == []
    G.load_state_dict(pristine)
    d = str(tmp_path / 'media')
    r1 = InversionCoach(G, save_grid=True, gen_video=True, media_dir=d, video_quality=80, **kw).invert('a', target, cam)
    assert r1.grid_paths == (os.path.join(d, 'pivot', 'a.png'), os.path.join(d, 'a.png'))
    assert r1.video_paths == (os.path.join(d, 'pivot', 'a_pivot.avi'), os.path.join(d, 'a.avi'))
    assert sorted(os.listdir(d)) == ['a.avi', 'a.png', 'pivot'] and sorted(os.listdir(os.path.join(d, 'pivot'))) == ['a.png', 'a_pivot.avi']
    hh, ww = target.shape[-2:]
    # the PNGs are pivot_grid's bytes: of the pristine generator before Phase B, of the tuned one after it
    G.load_state_dict(pristine)
    want_pivot = V.pivot_grid(G, r1.w_pivot, r1.cam, target, render_uniforms=uni).cpu().numpy()
    G.load_state_dict(r1.tuned_state)
    want_tuned = V.pivot_grid(G, r1.w_pivot, r1.cam, target, render_uniforms=uni).cpu().numpy()
    assert want_pivot.shape == (hh + 4, 5 * (ww + 2) + 2, 3) and want_pivot.dtype == np.uint8
    assert np.array_equal(_read_png(r1.grid_paths[0]), want_pivot)
    assert np.array_equal(_read_png(r1.grid_paths[1]), want_tuned)
    assert not np.array_equal(want_pivot, want_tuned)                       # Phase B changed the generator
    # the first tile is the target as the reference quantises it; the border is make_grid's 0.0 -> 128
    assert np.array_equal(want_pivot[2:2 + hh, 2:2 + ww], J.quantise_input(target[0].cpu().numpy()).transpose(1, 2, 0))
    assert np.all(want_pivot[:2] == 128) and np.all(want_pivot[:, :2] == 128)
    for p in r1.video_paths:
        check_avi(open(p, 'rb').read(), 240, 60, ww, hh)
    # the two videos differ (the tuned generator) and the default path left no file outside media_dir
    assert open(r1.video_paths[0], 'rb').read() != open(r1.video_paths[1], 'rb').read()
