"""Head mattes on the GPU (csrc/matte.hip: hipops.edt2, hipops.matte8; images.foreground_mask, matte_from_mask, head_matte and their
consumers).  Every operation of the kernels is an integer one or an IEEE fp64 add, multiply, sqrt, min, floor or rint in a fixed order, so the
bar is INTEGER and BYTE EQUALITY with the numpy restatement tests/support/matte_ref.py (pinned against scipy by tests/test_matte_cpu.py): on
the shapes the indexing can get wrong, on both paths of the transform (RESIDENT == TILED == AUTO), in both builds, and through head_matte, the
video writer and the four tools on the small synthetic generator.

The small generator's frame for the consumer tests is test_gpu_video._small_generator's own (ws seed 7, camera seed 2, pinned uniforms): the
test asserts that its depth mask has between 5 % and 95 % foreground."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_ref as M  # noqa: E402
import test_matte_cpu as MC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _corner(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h - 1, 0] = 9                                                     # foreground is != 0, not 255
    return m


def _mixed_frames():
    return np.stack([np.zeros((20, 45), np.uint8), MC.random_mask(20, 45, 0.5, 11), np.full((20, 45), 255, np.uint8)])


# name -> (mask, thresholds): the shapes of the issue, with 0..4 stages of mixed erosions and dilations spread over them
EDT_CASES = {
    '1x1_fg': (np.full((1, 1), 255, np.uint8), (0, -1)),
    '1x1_bg': (np.zeros((1, 1), np.uint8), ()),
    '1x70': (MC.random_mask(1, 70, 0.5, 1), (1,)),
    '65x1': (MC.random_mask(65, 1, 0.5, 2), (-2,)),
    '33x130_sparse': (MC.random_mask(33, 130, 0.02, 3), ()),
    '33x130_sparse_staged': (MC.random_mask(33, 130, 0.02, 3), (-10, 4, 2, -3)),
    '97x65_dense': (MC.random_mask(97, 65, 0.5, 4), (1, -2, -3)),
    '64x64_98': (MC.random_mask(64, 64, 0.98, 5), (2, -3)),
    '64x64_98_plain': (MC.random_mask(64, 64, 0.98, 5), ()),
    '40x300_corner': (_corner(40, 300), ()),
    '40x300_corner_grown': (_corner(40, 300), (-900, 100)),
    'n3_sentinels': (_mixed_frames(), ()),
    'n3_sentinels_staged': (_mixed_frames(), (1, -2, -5, 4)),
    '128x128': (MC.blob_mask(128, 128, 6)[None].repeat(2, 0), M.stage_thresholds(128)),
    '128x129': (MC.random_mask(128, 129, 0.6, 7), (1, -2)),
    '200x192_three_waves': (MC.random_mask(200, 192, 0.3, 8), (-2, 1)),
}


@functools.lru_cache(maxsize=None)
def _edt_want(name):
    mask, t = EDT_CASES[name]
    want = M.edt2(mask, t)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize('name', sorted(EDT_CASES))
def test_edt2_equals_the_restatement(name):
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    mask, t = EDT_CASES[name]
    want = _edt_want(name)
    got = {impl: H.edt2(_gpu(mask), t, impl=impl) for impl in ('auto', 'tiled')}
    if mask.shape[-1] * mask.shape[-2] <= 16384:
        got['resident'] = H.edt2(_gpu(mask), t, impl='resident')
    else:
        with pytest.raises(Eg3dHipError):                               # just over the limit: refused there, TILED under AUTO
            H.edt2(_gpu(mask), t, impl='resident')
    for impl, g in got.items():
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == mask.shape and (g != 0).all(), impl
        assert np.array_equal(g, want), (name, impl, int((g != want).sum()))
    if name.startswith('n3'):
        assert (want[0] == -(1 << 28)).all() and (want[2] == 1 << 28).all() and np.abs(want[1]).max() < 1 << 25


def test_edt2_large_path():
    from inv3d_amd import hipops as H
    mask = MC.blob_mask(512, 512, 9)
    t = M.stage_thresholds(512, 0.004, 0.008)                          # radii 2.05 and 4.1 pixels: the specks go, the holes close
    want = M.edt2(mask, t)
    assert np.array_equal(H.edt2(_gpu(mask), t).cpu().numpy(), want)
    assert np.array_equal(H.edt2(_gpu(mask), t, impl='tiled').cpu().numpy(), want)
    assert want.max() > 64 ** 2 and want.min() < -64 ** 2               # scans that run further than a wave is wide, on both sides


MATTE_CASES = {
    # name -> (source shape, output size, shrink_px, feather_px)
    '16to64': ((1, 16, 16), 64, 0.0, 3.0),
    '16to64_hard': ((1, 16, 16), 64, 0.0, 0.0),
    '24to60': ((1, 24, 24), 60, 0.0, 2.5),
    '24to60_shrunk_hard': ((1, 24, 24), 60, 1.25, 0.0),
    '32to32': ((1, 32, 32), 32, -0.5, 1.5),
    '20x30to40x60': ((1, 20, 30), (40, 60), 0.75, 4.0),
    '20x30to40x60_grown': ((1, 20, 30), (40, 60), -2.0, 4.0),
    'n2_16to130': ((2, 16, 16), 130, 0.4, 7.0),
    '48to20_minified': ((2, 48, 48), 20, 0.0, 1.0),
}


@pytest.mark.parametrize('name', sorted(MATTE_CASES))
def test_matte8_equals_the_restatement(name):
    from inv3d_amd import hipops as H
    (n, h, w), size, shrink, feather = MATTE_CASES[name]
    sd2 = M.edt2(np.stack([MC.blob_mask(h, w, h + w + i) for i in range(n)]))      # an inside, an outside, holes and specks: every part of the ramp
    want = M.matte8(sd2, size, shrink, feather)
    got = H.matte8(_gpu(sd2), size, shrink_px=shrink, feather_px=feather).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert (want == 255).any() and (want == 0).any()
    if feather > 0:
        assert ((want > 0) & (want < 255)).any()
    one = H.matte8(_gpu(sd2[0]), size, shrink_px=shrink, feather_px=feather)                # a [Hs,Ws] input drops the frame axis
    assert one.dim() == 2 and np.array_equal(one.cpu().numpy(), want[0])


def test_matte8_sentinels():
    from inv3d_amd import hipops as H
    sd2 = H.edt2(_gpu(np.stack([np.zeros((8, 8), np.uint8), np.full((8, 8), 1, np.uint8)])))
    for kw in (dict(), dict(feather_px=5.0), dict(shrink_px=40.0, feather_px=2.0), dict(shrink_px=-40.0)):
        a = H.matte8(sd2, 24, **kw).cpu().numpy()
        assert (a[0] == 0).all() and (a[1] == 255).all(), kw


@pytest.mark.parametrize('kw', [dict(), dict(open=0.0), dict(close=0.0), dict(open=0.0, close=0.0, feather=0.0), dict(shrink=0.01, feather=0.05),
                                dict(open=0.05, close=0.02, shrink=-0.01, impl='tiled')], ids=str)
def test_matte_from_mask_equals_the_composed_restatement(kw):
    from inv3d_amd import images
    mask = np.stack([MC.blob_mask(64, 64, 12), MC.random_mask(64, 64, 0.5, 13)])
    ref_kw = {k: v for k, v in kw.items() if k != 'impl'}
    want = M.matte_from_mask(mask, 160, **ref_kw)
    got = images.matte_from_mask(_gpu(mask), 160, **kw).cpu().numpy()
    assert got.shape == (2, 160, 160) and np.array_equal(got, want)
    assert np.array_equal(images.matte_from_mask(_gpu(mask[0]), 160, **kw).cpu().numpy(), want[0])


def test_foreground_mask_is_per_frame():
    from inv3d_amd import images
    rs = np.random.RandomState(4)
    d = rs.random_sample((3, 1, 16, 16)).astype(np.float32)
    d[1] += 10.0                                                        # a frame far away: a batch mean would make it all background
    got = images.foreground_mask(_gpu(d)).cpu().numpy()
    # the device's fp32 mean of 256 values below 11 is within 256 * 2^-21 < 2e-4 of the float64 mean whatever its summation order: no pixel
    # of this input sits that close to its frame's mean, so the comparison cannot depend on the order
    means = d.astype(np.float64).mean(axis=(1, 2, 3))
    assert all(np.abs(f.astype(np.float64) - m).min() > 2e-4 for f, m in zip(d, means))
    want = np.stack([f[0].astype(np.float64) < m for f, m in zip(d, means)]).astype(np.uint8) * 255
    assert got.dtype == np.uint8 and got.shape == (3, 16, 16) and np.array_equal(got, want) and 0 < got[1].sum() < 255 * 256


def test_invalid_arguments_are_refused():
    from inv3d_amd import hipops as H, images
    from inv3d_amd._lib import Eg3dHipError
    m = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    sd2 = torch.ones((2, 8, 8), dtype=torch.int32, device=DEV)
    for call in (lambda: H.edt2(m.float()), lambda: H.edt2(m[None]), lambda: H.edt2(m[0, 0]), lambda: H.edt2(m.cpu()),
                 lambda: H.edt2(m, (1, 2, 3, 4, 5)), lambda: H.edt2(m, impl='fast'),
                 lambda: H.edt2(torch.zeros((1, 4097, 2), dtype=torch.uint8, device=DEV)),
                 lambda: H.edt2(torch.zeros((1, 2, 4097), dtype=torch.uint8, device=DEV)),
                 lambda: H.edt2(torch.zeros((1, 128, 129), dtype=torch.uint8, device=DEV), impl='resident'),
                 lambda: H.matte8(sd2, (16, 17)), lambda: H.matte8(sd2.float(), 16), lambda: H.matte8(sd2[None], 16),
                 lambda: H.matte8(sd2.cpu(), 16), lambda: H.matte8(sd2, 16, feather_px=-1.0), lambda: H.matte8(sd2, 0),
                 lambda: H.matte8(sd2, 16385), lambda: H.matte8(sd2, 16, shrink_px=float('nan'))):
        with pytest.raises(Eg3dHipError):
            call()
    for call in (lambda: images.matte_from_mask(m[:, :, :7], 16), lambda: images.matte_from_mask(m, 16, open=-1.0),
                 lambda: images.foreground_mask(sd2), lambda: images.head_matte(None, None, None, size=8, source='hair')):
        with pytest.raises(ValueError):
            call()


def test_both_builds_give_the_same_bytes():
    import matte_digest
    here = matte_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'matte_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here
    for k in [k for k in here if k.endswith('_auto')]:
        assert here[k] == here[k[:-5] + '_tiled'] == here.get(k[:-5] + '_resident', here[k])


# ------------------------------------------------------------------------------------------------------------------------------------ consumers
@functools.lru_cache(maxsize=None)
def _frame():
    """The small generator, its latent, camera and uniforms, and ONE render of them: image uint8 [1,S,S,3], raw depth [1,1,h,w]."""
    from inv3d_amd import hipops as H
    from test_gpu_video import _small_generator
    G, ws, cam, _, uni = _small_generator()
    with torch.no_grad():
        out = G.synthesis(ws, cam, noise_mode='const', force_fp32=True, render_uniforms=uni)
    img = H.image_grid_u8(out['image'].float(), nrow=1, padding=0)[None]
    return G, ws, cam, uni, img, out['image_depth'].float().clone()


def _photo():
    import test_gpu_paste as TP
    return TP._rotated_photo()


def test_head_matte_from_depth():
    from inv3d_amd import images
    G, ws, cam, uni, img, depth = _frame()
    S = img.shape[1]
    mask = images.foreground_mask(depth).cpu().numpy()
    frac = float((mask != 0).mean())
    print(f'foreground fraction of the small generator\'s depth mask: {frac:.3f} ({mask.shape[-1]} x {mask.shape[-2]})')
    assert 0.05 < frac < 0.95
    want = M.matte_from_mask(mask, S)
    got = images.head_matte(G, ws, cam, depth=depth).cpu().numpy()
    assert got.shape == (1, S, S) and np.array_equal(got, want)
    assert want.min() == 0 and want.max() == 255 and 0 < int((want == 255).sum()) < want.size
    kw = dict(open=0.0, close=0.1, shrink=0.02, feather=0.1)
    assert np.array_equal(images.head_matte(G, ws, cam, size=96, depth=depth, **kw).cpu().numpy(), M.matte_from_mask(mask, 96, **kw))
    # without a depth the function renders the frame itself (its own stratified draws: no bytes to compare)
    own = images.head_matte(G, ws, cam)
    assert own.shape == (1, S, S) and own.dtype == torch.uint8 and 0 < int(own.sum())


def test_head_matte_from_shape():
    from inv3d_amd import images, inference as INF
    G, ws, _, _, _, _ = _frame()
    grid = INF.density_grid(G, ws, res=32)
    # seeded weights do not reach the default level: the grid's 0.7 quantile, and two wide cameras whose outer rays miss the box
    kw = dict(grid=grid, level=float(torch.quantile(grid.reshape(-1), 0.7)))
    cams = INF.orbit_cameras(2, focal=2.0, device=DEV)
    mask = INF.render_shape(G, ws, cams, res=144, **kw)['mask'].cpu().numpy()
    print(f'first-hit mask: {float((mask != 0).mean()):.3f} foreground')
    got = images.head_matte(G, ws, cams, size=144, source='shape', shape_kwargs=kw, feather=0.05).cpu().numpy()      # 144^2 > 16384: TILED
    assert got.shape == (2, 144, 144) and np.array_equal(got, M.matte_from_mask(mask, 144, feather=0.05))


def test_outside_the_matte_the_photograph_is_untouched():
    import paste_ref as P
    from inv3d_amd import hipops as H, images
    G, ws, cam, _, img, depth = _frame()
    photo, lm = _photo()
    S = img.shape[1]
    matte = images.head_matte(G, ws, cam, depth=depth)
    plan = images.paste_plan(photo.shape[0], photo.shape[1], lm, S)
    x0, y0, x1, y1 = plan.region
    got = H.paste_back(_gpu(photo), img, plan.matrix, plan.region, 0.08 * S, mask=matte).cpu().numpy()[0]
    plain = H.paste_back(_gpu(photo), img, plan.matrix, plan.region, 0.08 * S).cpu().numpy()[0]
    # the blend weights of the region, with and without the matte, from the paste's own restatement
    blank = np.zeros((S, S, 3), np.uint8)
    _, a_matte = P.paste8(photo, blank, np.asarray(plan.matrix), plan.region, 0.08 * S, mask=matte.cpu().numpy()[0], return_alpha=True)
    _, a_plain = P.paste8(photo, blank, np.asarray(plan.matrix), plan.region, 0.08 * S, return_alpha=True)
    spared = (a_matte[0] == 0) & (a_plain[0] > 0)                       # inside the feathered square, outside the head
    assert spared.sum() >= 16 and (a_matte[0] > 0).sum() >= 16
    box, pbox, gbox = photo[y0:y1, x0:x1], plain[y0:y1, x0:x1], got[y0:y1, x0:x1]
    assert np.array_equal(gbox[a_matte[0] == 0], box[a_matte[0] == 0]) and (pbox[spared] != box[spared]).any()
    assert (gbox[a_matte[0] > 0] != box[a_matte[0] > 0]).any()
    keep = np.ones(photo.shape[:2], bool)
    keep[y0:y1, x0:x1] = False
    assert np.array_equal(got[keep], photo[keep])


def test_orbit_video_matte(tmp_path):
    from inv3d_amd import hipops as H, images, inference as INF, video as V
    from test_video_cpu import check_avi
    G, ws, _, uni, _, _ = _frame()
    photo, lm = _photo()
    kw = dict(num_frames=3, fps=30, quality=85, batch=2, force_fp32=True, render_uniforms=uni)
    mk = dict(feather=0.06, shrink=0.01)
    files = {}
    for name, pk in dict(none=None, plain={}, matte=dict(matte=True), matte_kw=dict(matte=mk), off=dict(matte=False)).items():
        files[name] = str(tmp_path / f'{name}.avi')
        extra = {} if pk is None else dict(paste_kwargs=pk)
        assert V.write_orbit_video(G, ws, files[name], paste=(_gpu(photo), lm), **extra, **kw) == 3
    data = {k: open(v, 'rb').read() for k, v in files.items()}
    assert data['none'] == data['plain'] == data['off']                 # without `matte`: the file of before
    assert data['matte'] != data['none'] and data['matte_kw'] != data['matte']
    # the same frames pasted by hand through head_matte(depth=...) and encoded
    pairs = [(f.float().clone(), d.float().clone()) for f, d in INF.render_orbit(G, ws, num_frames=3, with_depth=True, force_fp32=True,
                                                                                  render_uniforms=uni)]
    plan = images.paste_plan(160, 160, lm, pairs[0][0].shape[-1])
    x0, y0, x1, y1 = plan.region
    for name, m_kw in (('matte', {}), ('matte_kw', mk)):
        a = check_avi(data[name], 3, 30, x1 - x0, y1 - y0)
        for i, (frame, depth) in enumerate(pairs):
            assert depth.shape[0] == 1 and depth.dim() == 3
            matte = images.head_matte(G, ws, None, size=frame.shape[-1], depth=depth[None], **m_kw)
            pasted = images.paste_back(_gpu(photo), frame[None], lm, mask=matte, region='bbox', layout='chw')
            jpg, off = H.jpeg_encode(pasted, quality=85)
            assert a['frames'][i] == jpg.cpu().numpy()[int(off[0]):int(off[1])].tobytes(), (name, i)
    with pytest.raises(ValueError):
        V.write_orbit_video(G, ws, files['off'], paste=(_gpu(photo), lm), paste_kwargs=dict(matte=True, mask=torch.zeros(1)), **kw)


class _Spy:
    """Stands in for images.head_matte / images.paste_back while a tool runs: the real call, its arguments and result kept."""

    def __init__(self, module, name):
        self.module, self.name, self.real, self.calls = module, name, getattr(module, name), []

    def __enter__(self):
        def spy(*args, **kw):
            out = self.real(*args, **kw)
            self.calls.append((args, kw, out))
            return out
        setattr(self.module, self.name, spy)
        return self

    def __exit__(self, *exc):
        setattr(self.module, self.name, self.real)


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_paste_back_tool_mask_binary(tmp_path):
    from inv3d_amd import images, video as V
    import test_matte_cpu as MC
    import test_align_cpu as TC
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import paste_back as tool
    photo, lm = _photo()
    edit, mask = TC.smooth_image(48, 48, 50), MC.blob_mask(48, 48, 2)
    V.write_png(str(tmp_path / 'me.png'), photo)
    V.write_png(str(tmp_path / 'mask.png'), mask)
    V.write_png(str(tmp_path / 'edit.png'), edit)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    base = ['--photo', str(tmp_path / 'me.png'), '--landmarks', str(tmp_path / 'lm.npz'), '--edit', str(tmp_path / 'edit.png'), '--mask',
            str(tmp_path / 'mask.png')]
    raw = tool.main(base + ['--out-dir', str(tmp_path / 'raw')])
    out = tool.main(base + ['--out-dir', str(tmp_path / 'bin'), '--mask-binary', '--matte-feather', '0.1', '--matte-shrink', '0.02'])
    assert np.array_equal(_read_png(raw[0]), images.paste_back(_gpu(photo), _gpu(edit), lm, mask=_gpu(mask)).cpu().numpy())     # as before
    matte = _gpu(M.matte_from_mask(mask, 48, feather=0.1, shrink=0.02))
    want = images.paste_back(_gpu(photo), _gpu(edit), lm, mask=matte).cpu().numpy()
    assert np.array_equal(_read_png(out[0]), want) and (want != _read_png(raw[0])).any()
    with pytest.raises(SystemExit):
        tool.main(base[:-2] + ['--out-dir', str(tmp_path / 'x'), '--mask-binary'])


def test_run_ganspace_tool_paste_matte(tmp_path):
    import importlib.util
    from inv3d_amd import images, video as V
    spec = importlib.util.spec_from_file_location('run_ganspace_tool', os.path.join(ROOT, 'tools', 'run_ganspace.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, ws, cam, _, _, _ = _frame()
    photo, lm = _photo()
    V.write_png(str(tmp_path / 'me.png'), photo)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    np.save(str(tmp_path / 'comp.npy'), np.linalg.qr(np.random.RandomState(1).normal(size=(32, 32)))[0].astype(np.float32))
    np.save(str(tmp_path / 'a_ws.npy'), ws.cpu().numpy())
    np.save(str(tmp_path / 'a_cam.npy'), cam.cpu().numpy())
    args = ['edit', '--synthetic', 'small', '--components', str(tmp_path / 'comp.npy'), '--ws', str(tmp_path / 'a_ws.npy'), '--cam',
            str(tmp_path / 'a_cam.npy'), '--params', '1', '0', '3', '2.5', '--num-imgs', '3', '--name', 'a', '--out-dir', str(tmp_path / 'edits'),
            '--paste-photo', str(tmp_path / 'me.png'), '--landmarks', str(tmp_path / 'lm.npz')]
    with _Spy(images, 'head_matte') as spy:
        out = tool.main(args + ['--paste-matte', '--matte-feather', '0.07'])
    (_, kw, matte), = spy.calls
    assert kw['feather'] == 0.07 and kw['shrink'] == 0.0 and torch.equal(kw['depth'], out['depth']) and out['depth'].shape[:2] == (3, 1)
    S = out['images'].shape[1]
    assert np.array_equal(matte.cpu().numpy(), M.matte_from_mask(images.foreground_mask(out['depth']).cpu().numpy(), S, feather=0.07))
    want = images.paste_back(_gpu(photo), out['images'], lm, region='bbox', mask=matte)
    assert torch.equal(out['pasted'], want) and not torch.equal(want, images.paste_back(_gpu(photo), out['images'], lm, region='bbox'))
    assert np.array_equal(_read_png(str(tmp_path / 'edits' / 'a_pasted.png')), np.concatenate(list(want.cpu().numpy()), 1))
    with pytest.raises(SystemExit):
        tool.main(args[:-4] + ['--paste-matte'])


def test_run_inversion_tool_paste_matte(tmp_path):
    from inv3d_amd import images, video as V
    import test_paste_cpu as PC
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_inversion
    case = PC.CASES['inside']
    d = tmp_path / 'photos'
    d.mkdir()
    V.write_png(str(d / 'inside.png'), case['image'])
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, inside=case['landmarks'])
    with _Spy(images, 'head_matte') as hm, _Spy(images, 'paste_back') as pb:
        run_inversion.main(['--in-dir', str(d), '--landmarks', lm_path, '--out-dir', str(tmp_path / 'out'), '--synthetic', 'small', '--steps-a', '1',
                            '--steps-b', '1', '--paste-back', '--paste-matte', '--matte-shrink', '0.01'])
    (_, mkw, matte), = hm.calls
    (pargs, pkw, pasted), = pb.calls
    edit = pargs[1]
    assert mkw['shrink'] == 0.01 and mkw['feather'] == 0.03 and mkw['depth'].shape[:2] == (1, 1) and pkw['mask'] is matte
    S = int(edit.shape[-1])
    assert np.array_equal(matte.cpu().numpy(), M.matte_from_mask(images.foreground_mask(mkw['depth']).cpu().numpy(), S, shrink=0.01))
    png = _read_png(str(tmp_path / 'out' / 'pasted' / 'inside.png'))
    want = images.paste_back(_gpu(case['image']), edit, case['landmarks'], mask=matte)[0].cpu().numpy()
    assert np.array_equal(png, want) and np.array_equal(png, pasted[0].cpu().numpy())
    with pytest.raises(SystemExit):
        run_inversion.main(['--in-dir', str(d), '--out-dir', str(tmp_path / 'o2'), '--synthetic', 'small', '--paste-matte'])


def test_render_video_tool_paste_matte(tmp_path):
    from inv3d_amd import hipops as H, images, video as V
    from test_video_cpu import check_avi
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import render_video
    _, ws, _, _, img, _ = _frame()
    photo, lm = _photo()
    V.write_png(str(tmp_path / 'me.png'), photo)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    np.save(str(tmp_path / 'ws.npy'), ws.cpu().numpy())
    args = ['--ws', str(tmp_path / 'ws.npy'), '--synthetic', 'small', '--frames', '3', '--batch', '2', '--paste-photo', str(tmp_path / 'me.png'),
            '--landmarks', str(tmp_path / 'lm.npz')]
    with _Spy(images, 'head_matte') as hm, _Spy(images, 'paste_back') as pb:
        assert render_video.main(args + ['--out', str(tmp_path / 'matte.avi'), '--paste-matte', '--matte-feather', '0.05']) == 3
    assert [c[1]['depth'].shape[0] for c in hm.calls] == [2, 1] and all(c[1]['feather'] == 0.05 and c[1]['shrink'] == 0.0 for c in hm.calls)
    assert [c[1]['mask'] is h[2] for c, h in zip(pb.calls, hm.calls)] == [True, True]
    S = img.shape[1]
    for _, kw, matte in hm.calls:
        assert np.array_equal(matte.cpu().numpy(), M.matte_from_mask(images.foreground_mask(kw['depth']).cpu().numpy(), S, feather=0.05))
    x0, y0, x1, y1 = images.paste_plan(160, 160, lm, S).region
    a = check_avi(open(str(tmp_path / 'matte.avi'), 'rb').read(), 3, 60, x1 - x0, y1 - y0)
    # the file's frames are the tool's own renders pasted by hand through the restated matte and encoded
    i = 0
    for (pargs, _, _), (_, kw, _) in zip(pb.calls, hm.calls):
        matte = _gpu(M.matte_from_mask(images.foreground_mask(kw['depth']).cpu().numpy(), S, feather=0.05))
        for k in range(pargs[1].shape[0]):
            pasted = images.paste_back(_gpu(photo), pargs[1][k:k + 1], lm, mask=matte[k:k + 1], region='bbox', layout='chw')
            jpg, off = H.jpeg_encode(pasted, quality=90)
            assert a['frames'][i] == jpg.cpu().numpy()[int(off[0]):int(off[1])].tobytes(), i
            i += 1
    assert i == 3
    with _Spy(images, 'head_matte') as hm:
        assert render_video.main(args + ['--out', str(tmp_path / 'plain.avi')]) == 3
    assert hm.calls == []
