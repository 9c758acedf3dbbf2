"""Paste-back on the GPU (csrc/imgprep.hip paste_back_kernel, hipops.paste_back, images.paste_back and its consumers): the kernel EQUALS the
numpy restatement tests/support/paste_ref.py byte for byte -- every operation is an IEEE fp64 add, multiply, min, floor or rint in a fixed
order, so equality is the bar -- on the six golden alignment plans and the three exact ones (where the round trip is the photo itself), on
the shapes the indexing can get wrong, through the minifying and the fp32 paths of images.paste_back, in both builds, and through the video
writer and the three tools on the small synthetic generator."""
import functools
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paste_ref as P  # noqa: E402
import pil_ref as R  # noqa: E402
import test_align_cpu as TC  # noqa: E402
import test_paste_cpu as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PLANS = sorted(PC.CASES) + ['exact0', 'exact1', 'exact2']


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _paste(photo, edits, matrix, region, feather_px=0.0, mask=None, **kw):
    from inv3d_amd import hipops as H
    return H.paste_back(_gpu(photo), _gpu(edits), matrix, region, feather_px, None if mask is None else _gpu(mask), **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _plan_case(name):
    """(photo, landmarks, S, plan, edits [2,S,S,3]: the aligned photo and a noise frame, masks)."""
    from inv3d_amd.images import paste_plan
    if name.startswith('exact'):
        photo, lm, S = PC.EXACT_PHOTO, P.EXACT_LANDMARKS[int(name[-1])], PC.EXACT_S
    else:
        photo, lm, S = PC.CASES[name]['image'], PC.CASES[name]['landmarks'], PC.CASES[name]['output_size']
    plan = paste_plan(photo.shape[0], photo.shape[1], lm, S)
    edits = np.stack([R.align_face(photo, lm, S), TC.noise_image(S, S, 3, 40 + S)])
    yy, xx = np.mgrid[:S, :S]
    ramp = np.rint(255.0 * (xx + yy) / (2 * S - 2)).astype(np.uint8)
    per_frame = np.stack([ramp, TC.noise_image(S, S, 1, 5)[..., 0]])
    return photo, lm, S, plan, edits, dict(ramp=ramp, per_frame=per_frame, full=np.full((S, S), 255, np.uint8))


@pytest.mark.parametrize('name', PLANS)
def test_kernel_equals_the_restatement(name):
    photo, lm, S, plan, edits, masks = _plan_case(name)
    assert max(photo.shape[:2]) <= 250 and S <= 128
    for fpx in (0.0, 0.08 * S):
        plain = P.paste8(photo, edits, plan.matrix, plan.region, fpx)
        for which in (None, 'ramp', 'per_frame', 'full'):
            mask = None if which is None else masks[which]
            want = plain if which in (None, 'full') else P.paste8(photo, edits, plan.matrix, plan.region, fpx, mask)   # all 255 IS no mask
            got = _paste(photo, edits, plan.matrix, plan.region, fpx, mask)
            assert got.shape == want.shape == (2,) + photo.shape
            assert np.array_equal(got, want), (name, fpx, which, int((got != want).any(-1).sum()))
        assert (plain[1] != photo).any()
        if name.startswith('exact'):
            assert np.array_equal(plain[0], photo)                      # paste(align(photo)) is the photo: integer isometries


def test_wide_region_one_row_and_frames():
    """A region of 165 columns (two full tiles of 64 and a remainder) and 77 rows (no multiple of 4); one row of it; three frames at once."""
    photo, S = TC.smooth_image(90, 200, 3), 48
    edits = np.stack([TC.noise_image(S, S, 3, 60 + k) for k in range(3)])
    matrix, region = (-2.75, 0.3, 0.05, 1.5, -0.05, 0.3), (10, 3, 175, 80)
    want = P.paste8(photo, edits, matrix, region, 5.0)
    got = _paste(photo, edits, matrix, region, 5.0)
    assert np.array_equal(got, want) and (got[0] != got[1]).any() and (got[1] != got[2]).any()
    for k in range(3):
        assert np.array_equal(_paste(photo, edits[k], matrix, region, 5.0), want[k]), k        # [S,S,C] in, one frame out
    row = (10, 40, 175, 41)
    assert np.array_equal(_paste(photo, edits, matrix, row, 5.0), P.paste8(photo, edits, matrix, row, 5.0))
    part = _paste(photo, edits, matrix, region, 5.0, whole=False)
    assert part.shape == (3, 77, 165, 3) and np.array_equal(part, want[:, 3:80, 10:175])
    for whole in (True, False):
        chw = _paste(photo, edits, matrix, region, 5.0, whole=whole, layout='chw')
        assert np.array_equal(chw, (want if whole else part).transpose(0, 3, 1, 2))
    assert np.array_equal(_paste(photo, edits, matrix, (30, 20, 30, 60), 5.0), np.repeat(photo[None], 3, 0))      # an empty region: the photo
    assert _paste(photo, edits, matrix, (30, 20, 30, 60), 5.0, whole=False).shape == (3, 40, 0, 3)


@pytest.mark.parametrize('side,eye_avg', [('left', (10.5, 40.5)), ('right', (90.5, 40.5)), ('top', (50.5, 5.5)), ('bottom', (50.5, 80.5))])
def test_region_clamped_on_each_side(side, eye_avg):
    from inv3d_amd.images import paste_plan
    photo, S = PC.EXACT_PHOTO, 64
    lm = P.upright_landmarks(eye_avg, (16, 0), (0, 10))
    plan = paste_plan(100, 100, lm, S)
    x0, y0, x1, y1 = plan.region
    assert dict(left=x0 == 0, right=x1 == 100, top=y0 == 0, bottom=y1 == 100)[side] and (x1 - x0) * (y1 - y0) < 4096
    edit = TC.noise_image(S, S, 3, 77)
    for whole in (True, False):
        assert np.array_equal(_paste(photo, edit, plan.matrix, plan.region, 6.0, whole=whole),
                              P.paste8(photo, edit, plan.matrix, plan.region, 6.0, whole=whole)), whole


def test_grey_equals_a_channel_of_colour():
    photo = np.repeat(TC.noise_image(70, 90, 1, 8), 3, -1)
    edits = np.repeat(TC.noise_image(40, 40, 1, 9), 3, -1)[None]
    mask = TC.noise_image(40, 40, 1, 10)[..., 0]
    matrix, region = (-4.0, 0.55, 0.1, -3.0, -0.1, 0.55), (2, 1, 88, 70)
    colour = _paste(photo, edits, matrix, region, 4.0, mask)
    grey = _paste(photo[..., :1], edits[..., :1], matrix, region, 4.0, mask)
    assert grey.shape == (1, 70, 90, 1) and np.array_equal(grey[..., 0], colour[..., 0]) and (colour[0] != photo).any()
    assert np.array_equal(_paste(photo[..., :1], edits[..., :1], matrix, region, 4.0, mask, layout='chw'), grey.transpose(0, 3, 1, 2))


def test_minification_presizes_with_lanczos():
    """Scale 2: the face is 64 px in the photo, the edit 128.  images.paste_back equals the restatement on the Pillow-LANCZOS-resized edit."""
    from inv3d_amd import images
    photo, lm = PC.EXACT_PHOTO, P.EXACT_LANDMARKS[0]
    edits = np.stack([TC.smooth_image(128, 128, 4), TC.noise_image(128, 128, 3, 6)])
    mask = TC.smooth_image(128, 128, 12)[..., 0]
    assert images.paste_plan(100, 100, lm, 128).presize == 64
    for region in ('photo', 'bbox'):
        for m in (None, mask):
            got = images.paste_back(_gpu(photo), _gpu(edits), lm, mask=None if m is None else _gpu(m), region=region).cpu().numpy()
            assert np.array_equal(got, PC.paste_full_ref(photo, edits, lm, mask=m, region=region)), (region, m is None)
    one = images.paste_back(_gpu(photo), _gpu(edits[0]), lm).cpu().numpy()
    assert one.shape == photo.shape and np.array_equal(one, PC.paste_full_ref(photo, edits[0], lm))
    with pytest.raises(ValueError):
        images.paste_back(_gpu(photo), _gpu(edits), P.upright_landmarks((-500.5, 40.5), (16, 0), (0, 10)), region='bbox')
    outside = images.paste_back(_gpu(photo), _gpu(edits), P.upright_landmarks((-500.5, 40.5), (16, 0), (0, 10))).cpu().numpy()
    assert np.array_equal(outside, np.repeat(photo[None], 2, 0))


def test_fp32_frames_are_quantised_as_image_grid_u8():
    from inv3d_amd import hipops as H, images
    photo, lm = PC.CASES['crop_only']['image'], PC.CASES['crop_only']['landmarks']
    x = torch.from_numpy(np.random.RandomState(2).uniform(-1.2, 1.2, (3, 3, 32, 32)).astype(np.float32)).to(DEV)
    u8 = H.image_grid_u8(x, nrow=1, padding=0).reshape(3, 32, 32, 3)
    got = images.paste_back(_gpu(photo), x, lm)
    assert got.shape == (3,) + photo.shape and torch.equal(got, images.paste_back(_gpu(photo), u8, lm))
    assert np.array_equal(got.cpu().numpy(), PC.paste_full_ref(photo, u8.cpu().numpy(), lm))


def test_both_builds_give_the_same_bytes():
    import paste_digest
    here = paste_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'paste_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def test_invalid_arguments_are_refused():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    photo = torch.zeros((20, 30, 3), dtype=torch.uint8, device=DEV)
    edits = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    m, r = (0, 1, 0, 0, 0, 1), (0, 0, 8, 8)
    for call in (lambda: H.paste_back(photo, edits, m, (0, 0, 31, 8)), lambda: H.paste_back(photo, edits, m, (5, 0, 4, 8)),
                 lambda: H.paste_back(photo, edits, m[:5], r), lambda: H.paste_back(photo, edits[..., :1], m, r),
                 lambda: H.paste_back(photo, edits[:, :, :7], m, r), lambda: H.paste_back(photo[None], edits, m, r),
                 lambda: H.paste_back(photo, edits, m, r, layout='nchw'), lambda: H.paste_back(photo, edits, m, r, feather_px=-1.0),
                 lambda: H.paste_back(photo, edits, m, r, mask=torch.zeros((3, 8, 8), dtype=torch.uint8, device=DEV)),
                 lambda: H.paste_back(photo, edits.float(), m, r)):
        with pytest.raises(Eg3dHipError):
            call()


# ------------------------------------------------------------------------------------------------------------------------------------ consumers
def _rotated_photo():
    """A 160 x 160 photograph whose face square is turned by 45 degrees: its bounding box has four corners the square does not cover."""
    return TC.smooth_image(160, 160, 31), P.upright_landmarks((80.5, 78.5), (12, 12), (-8, 8))


def test_orbit_video_paste(tmp_path):
    from PIL import Image
    from inv3d_amd import hipops as H, images, video as V
    from test_gpu_video import _small_generator
    from test_video_cpu import check_avi
    G, ws, _, target, uni = _small_generator()
    S = int(target.shape[-1])
    photo, lm = _rotated_photo()
    plan = images.paste_plan(160, 160, lm, S)
    x0, y0, x1, y1 = plan.region
    kw = dict(num_frames=3, fps=30, quality=85, batch=2, force_fp32=True, render_uniforms=uni)
    path, plain = str(tmp_path / 'pasted.avi'), str(tmp_path / 'plain.avi')
    assert V.write_orbit_video(G, ws, path, paste=(_gpu(photo), lm), **kw) == 3
    a = check_avi(open(path, 'rb').read(), 3, 30, x1 - x0, y1 - y0)                    # frames of the bounding box's size
    # where the blend weight is 0 the frame IS the photo: luma blocks of 8 x 8 wholly outside the square decode as those of the bare region
    bare, _ = H.jpeg_encode(_gpu(photo[y0:y1, x0:x1].transpose(2, 0, 1)[None]), quality=85)

    def luma(data):
        im = Image.open(io.BytesIO(data))
        im.draft('YCbCr', im.size)
        assert im.mode == 'YCbCr'
        return np.asarray(im)[..., 0]
    got, want = luma(a['frames'][0]), luma(bare.cpu().numpy().tobytes())
    _, alpha = P.paste8(photo, np.zeros((S, S, 3), np.uint8), np.asarray(plan.matrix), plan.region, 0.08 * S, return_alpha=True)
    hb, wb = (y1 - y0) // 8, (x1 - x0) // 8
    free = (alpha[0][:hb * 8, :wb * 8].reshape(hb, 8, wb, 8) == 0).all((1, 3))
    assert free.sum() >= 16 and not free.all()
    px = np.repeat(np.repeat(free, 8, 0), 8, 1)
    assert np.array_equal(got[:hb * 8, :wb * 8][px], want[:hb * 8, :wb * 8][px]) and (got != want).any()
    V.write_orbit_video(G, ws, plain, paste=None, **kw)
    today = str(tmp_path / 'today.avi')
    V.write_orbit_video(G, ws, today, **kw)
    assert open(plain, 'rb').read() == open(today, 'rb').read()
    whole = str(tmp_path / 'whole.avi')
    V.write_orbit_video(G, ws, whole, paste=(_gpu(photo), lm), paste_kwargs=dict(region='photo'), **kw)
    check_avi(open(whole, 'rb').read(), 3, 30, 160, 160)
    with pytest.raises(ValueError):
        V.write_orbit_video(G, ws, whole, paste=(_gpu(photo), lm), image_mode='image_depth', **kw)


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_paste_back_tool(tmp_path):
    """tools/paste_back.py (in process): the PNGs are images.paste_back's bytes."""
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import paste_back as tool
    photo, lm = _rotated_photo()
    edits = [TC.smooth_image(48, 48, 50), TC.noise_image(48, 48, 3, 51)]
    mask = TC.smooth_image(48, 48, 52)[..., 0]
    V.write_png(str(tmp_path / 'me.png'), photo)
    V.write_png(str(tmp_path / 'mask.png'), mask)
    for k, e in enumerate(edits):
        V.write_png(str(tmp_path / f'edit{k}.png'), e)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    base = ['--photo', str(tmp_path / 'me.png'), '--landmarks', str(tmp_path / 'lm.npz'), '--edit', str(tmp_path / 'edit0.png'), str(tmp_path / 'edit1.png')]
    out = tool.main(base + ['--out-dir', str(tmp_path / 'whole')])
    assert [os.path.basename(p) for p in out] == ['edit0.png', 'edit1.png']
    box = tool.main(base + ['--out-dir', str(tmp_path / 'box'), '--bbox', '--feather', '0.2', '--mask', str(tmp_path / 'mask.png')])
    for k, e in enumerate(edits):
        assert np.array_equal(_read_png(out[k]), images.paste_back(_gpu(photo), _gpu(e), lm).cpu().numpy())
        want = images.paste_back(_gpu(photo), _gpu(e), lm, feather=0.2, mask=_gpu(mask), region='bbox').cpu().numpy()
        assert np.array_equal(_read_png(box[k]), want) and want.shape[0] < 160


def test_run_ganspace_tool_pastes_the_edit_row(tmp_path):
    import importlib.util
    from inv3d_amd import images, video as V
    from test_gpu_video import _small_generator
    spec = importlib.util.spec_from_file_location('run_ganspace_tool', os.path.join(ROOT, 'tools', 'run_ganspace.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, ws, cam, _, _ = _small_generator()
    photo, lm = _rotated_photo()
    V.write_png(str(tmp_path / 'me.png'), photo)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    np.save(str(tmp_path / 'comp.npy'), np.linalg.qr(np.random.RandomState(1).normal(size=(32, 32)))[0].astype(np.float32))
    np.save(str(tmp_path / 'a_ws.npy'), ws.cpu().numpy())
    np.save(str(tmp_path / 'a_cam.npy'), cam.cpu().numpy())
    args = ['edit', '--synthetic', 'small', '--components', str(tmp_path / 'comp.npy'), '--ws', str(tmp_path / 'a_ws.npy'), '--cam',
            str(tmp_path / 'a_cam.npy'), '--params', '1', '0', '3', '2.5', '--num-imgs', '3', '--name', 'a']
    plain = tool.main(args + ['--out-dir', str(tmp_path / 'plain')])
    out = tool.main(args + ['--out-dir', str(tmp_path / 'edits'), '--paste-photo', str(tmp_path / 'me.png'), '--landmarks', str(tmp_path / 'lm.npz')])
    assert sorted(os.listdir(str(tmp_path / 'plain'))) == ['a_grid.png'] and 'pasted' not in plain
    assert sorted(os.listdir(str(tmp_path / 'edits'))) == ['a_grid.png', 'a_pasted.png']
    assert np.array_equal(_read_png(str(tmp_path / 'edits' / 'a_grid.png')), out['grid'].cpu().numpy())       # the grid is written as before
    want = images.paste_back(_gpu(photo), out['images'], lm, region='bbox')
    assert want.shape[0] == 3 and torch.equal(out['pasted'], want)
    assert np.array_equal(_read_png(str(tmp_path / 'edits' / 'a_pasted.png')), np.concatenate(list(want.cpu().numpy()), 1))


def test_run_inversion_tool_pastes_the_reconstruction(tmp_path):
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_inversion
    cases = PC.CASES
    d = tmp_path / 'photos'
    d.mkdir()
    V.write_png(str(d / 'inside.png'), cases['inside']['image'])
    V.write_png(str(d / 'square.png'), TC.smooth_image(64, 64, 9))                              # no landmarks: inverted, not pasted
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, inside=cases['inside']['landmarks'])
    seen = {}
    real = images.paste_back

    def spy(photo, edit, landmarks, **kw):
        out = real(photo, edit, landmarks, **kw)
        seen['out'], seen['edit'] = out, edit
        return out
    images.paste_back = spy
    try:
        results, stats = run_inversion.main(['--in-dir', str(d), '--landmarks', lm_path, '--out-dir', str(tmp_path / 'out'), '--synthetic', 'small',
                                             '--steps-a', '1', '--steps-b', '1', '--paste-back'])
    finally:
        images.paste_back = real
    assert stats['n_done'] == 2 and sorted(os.listdir(str(tmp_path / 'out'))) == ['pasted']
    assert os.listdir(str(tmp_path / 'out' / 'pasted')) == ['inside.png']
    png = _read_png(str(tmp_path / 'out' / 'pasted' / 'inside.png'))
    photo = cases['inside']['image']
    assert seen['edit'].shape[0] == 1 and seen['edit'].dtype == torch.float32
    assert np.array_equal(png, seen['out'][0].cpu().numpy()) and png.shape == photo.shape
    assert np.array_equal(png, real(_gpu(photo), seen['edit'], cases['inside']['landmarks'])[0].cpu().numpy())
    x0, y0, x1, y1 = images.paste_plan(photo.shape[0], photo.shape[1], cases['inside']['landmarks'], int(seen['edit'].shape[-1])).region
    keep = np.ones(photo.shape[:2], bool)
    keep[y0:y1, x0:x1] = False
    assert keep.any() and np.array_equal(png[keep], photo[keep]) and (png != photo).any()
