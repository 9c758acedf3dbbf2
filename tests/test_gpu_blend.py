"""Multi-band paste-back on the GPU (csrc/blend.hip, hipops.paste_blend, images.paste_back(bands=...) and its consumers): the kernels EQUAL
the numpy restatement tests/support/blend_ref.py byte for byte -- level 0 is eg3d_paste_back8's fp64 arithmetic, everything after it one
IEEE fp32 add, subtract or multiply at a time in a fixed order, so equality is the bar and no tolerance is needed -- on the six golden
alignment plans and the three exact ones, on odd sizes at every level, at the edges of both level-0 kernels' tiles, on coarsest levels of one
or two pixels, with the window clamped on each side of the photo, through the minifying path of images.paste_back, in both builds, and
through the video writer and the tools on the small synthetic generator.  Photos <= 250 px, S <= 128: every test takes seconds."""
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
import blend_ref as B  # noqa: E402
import paste_ref as P  # noqa: E402
import pil_ref as R  # noqa: E402
import test_align_cpu as TC  # noqa: E402
import test_gpu_paste as GP  # noqa: E402
import test_paste_cpu as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_gpu = GP._gpu


def _blend(photo, edits, matrix, region, bands, feather_px=0.0, mask=None, **kw):
    from inv3d_amd import hipops as H
    return H.paste_blend(_gpu(photo), _gpu(edits), matrix, region, bands, feather_px, None if mask is None else _gpu(mask), **kw).cpu().numpy()


def _same_levels(got, want, bands):
    """The pyramid the kernels left in the workspace against the restatement's, bit for bit (levels 1..L of D and alpha, 1..L-1 of R)."""
    for k in range(1, bands + 1):
        assert np.array_equal(got['D'][k - 1].cpu().numpy().view(np.uint32), want['D'][k].view(np.uint32)), ('D', k)
        assert np.array_equal(got['alpha'][k - 1].cpu().numpy().view(np.uint32), want['alpha'][k][:, 0].view(np.uint32)), ('alpha', k)
    for k in range(1, bands):
        assert np.array_equal(got['R'][k - 1].cpu().numpy().view(np.uint32), want['R'][k].view(np.uint32)), ('R', k)


def blend_full_ref(photo, edit, landmarks, bands, feather=0.08, mask=None, region='photo'):
    """images.paste_back(bands=...)'s steps on the restatements: paste_plan, Pillow-LANCZOS presize where scale > 1, blend8."""
    from inv3d_amd.images import paste_plan
    S = edit.shape[-2]
    plan = paste_plan(photo.shape[0], photo.shape[1], landmarks, S)
    matrix, fpx = np.asarray(plan.matrix), feather * S
    if plan.presize is not None and plan.presize != S:
        ps = plan.presize
        edit = R.resize8(edit, (ps, ps), 'lanczos') if edit.ndim == 3 else np.stack([R.resize8(e, (ps, ps), 'lanczos') for e in edit])
        if mask is not None:
            mask = R.resize8(mask[..., None], (ps, ps), 'lanczos')[..., 0] if mask.ndim == 2 else \
                np.stack([R.resize8(k[..., None], (ps, ps), 'lanczos')[..., 0] for k in mask])
        matrix, fpx = matrix * (ps / S), fpx * (ps / S)
    return B.blend8(photo, edit, matrix, plan.region, bands, fpx, mask, whole=region == 'photo')


@pytest.mark.parametrize('name', GP.PLANS)
def test_kernels_equal_the_restatement(name):
    photo, lm, S, plan, edits, masks = GP._plan_case(name)
    assert max(photo.shape[:2]) <= 250 and S <= 128
    for bands in (1, 2, 3) + ((4,) if name == 'pad_corner_rotated' else ()):
        for fpx in (0.0, 0.08 * S):
            for which in (None, 'ramp', 'per_frame'):
                mask = None if which is None else masks[which]
                want = B.blend8(photo, edits, plan.matrix, plan.region, bands, fpx, mask)
                got = _blend(photo, edits, plan.matrix, plan.region, bands, fpx, mask)
                assert got.shape == want.shape == (2,) + photo.shape
                assert np.array_equal(got, want), (name, bands, fpx, which, int((got != want).any(-1).sum()))
                assert (want[1] != photo).any()
                if name.startswith('exact'):
                    assert np.array_equal(got[0], photo)                # paste(align(photo)): D == 0 exactly, so R == 0 and the photo stays


def test_odd_sizes_at_every_level():
    """A 165 x 77 box in a 200 x 90 photo: 83 x 39, 42 x 20 and 21 x 10 before the margins; three frames; one frame as [S,S,C]; a one-row
    box; the box alone; planar output; an empty box."""
    from inv3d_amd import hipops as H
    photo, S = TC.smooth_image(90, 200, 3), 48
    edits = np.stack([TC.noise_image(S, S, 3, 60 + k) for k in range(3)])
    matrix, region = (-2.75, 0.3, 0.05, 1.5, -0.05, 0.3), (10, 3, 175, 80)
    want, lv = B.blend8(photo, edits, matrix, region, 3, 5.0, return_levels=True)
    got, glv = H.paste_blend(_gpu(photo), _gpu(edits), matrix, region, 3, 5.0, return_levels=True)
    _same_levels(glv, lv, 3)
    got = got.cpu().numpy()
    assert np.array_equal(got, want) and (got[0] != got[1]).any() and (got[1] != got[2]).any()
    for k in range(3):
        assert np.array_equal(_blend(photo, edits[k], matrix, region, 3, 5.0), want[k]), k         # [S,S,C] in, one frame out
    row = (10, 40, 175, 41)
    assert np.array_equal(_blend(photo, edits, matrix, row, 3, 5.0), B.blend8(photo, edits, matrix, row, 3, 5.0))
    part = _blend(photo, edits, matrix, region, 3, 5.0, whole=False)
    assert part.shape == (3, 77, 165, 3) and np.array_equal(part, want[:, 3:80, 10:175])
    assert np.array_equal(part, B.blend8(photo, edits, matrix, region, 3, 5.0, whole=False))
    for whole in (True, False):
        chw = _blend(photo, edits, matrix, region, 3, 5.0, whole=whole, layout='chw')
        assert np.array_equal(chw, (want if whole else part).transpose(0, 3, 1, 2))
    assert np.array_equal(_blend(photo, edits, matrix, (30, 20, 30, 60), 3, 5.0), np.repeat(photo[None], 3, 0))    # an empty box: the photo
    assert _blend(photo, edits, matrix, (30, 20, 30, 60), 3, 5.0, whole=False).shape == (3, 40, 0, 3)


def _tile_sides():
    from inv3d_amd import _lib as L
    widths = sorted({v for t in (L.BLEND_L1_TILE, L.BLEND_COMPOSE_TILE) for v in (t[0], t[0] + 1, 2 * t[0] + 37)})
    heights = sorted({v for t in (L.BLEND_L1_TILE, L.BLEND_COMPOSE_TILE) for v in (t[1], t[1] + 1, 2 * t[1] + 5)})
    return widths, heights


def test_tile_edges():
    """Windows of exactly one tile, one tile + 1 and two tiles + a remainder of the level-1 kernel and of the compose kernel, per axis: the
    box is the whole photo, so the window is the photo."""
    widths, heights = _tile_sides()
    assert max(widths) <= 250 and max(heights) <= 250
    S = 32
    edits = np.stack([TC.noise_image(S, S, 3, 70), TC.smooth_image(S, S, 71)])
    mask = TC.noise_image(S, S, 1, 72)[..., 0]
    for w in widths:
        for h in heights:
            photo = TC.noise_image(h, w, 3, 100 + w + h)
            matrix = (-1.0, (S + 2.0) / w, 0.0, -1.0, 0.0, (S + 2.0) / h)          # the square ends a little inside the photo
            for bands in (1, 2):
                want = B.blend8(photo, edits, matrix, (0, 0, w, h), bands, 3.0, mask)
                got = _blend(photo, edits, matrix, (0, 0, w, h), bands, 3.0, mask)
                assert np.array_equal(got, want), (w, h, bands, int((got != want).any(-1).sum()))
            assert (want != photo).any()


@pytest.mark.parametrize('hw', [(7, 9), (7, 8)])
def test_tiny_coarsest_levels(hw):
    """A 5 x 3 box, bands 3: the coarsest level is 2 x 1 (photo 9 x 7) or 1 x 1 (photo 8 x 7)."""
    from inv3d_amd import hipops as H
    h, w = hw
    photo = TC.noise_image(h, w, 3, 80)
    edits = np.stack([TC.noise_image(8, 8, 3, 81), TC.noise_image(8, 8, 3, 82)])
    matrix, region = (-3.0, 1.5, 0.0, -3.0, 0.0, 1.5), (2, 2, 7, 5)
    want, lv = B.blend8(photo, edits, matrix, region, 3, 2.0, return_levels=True)
    assert lv['D'][3].shape[-2:] == ((1, 2) if w == 9 else (1, 1))
    got, glv = H.paste_blend(_gpu(photo), _gpu(edits), matrix, region, 3, 2.0, return_levels=True)
    _same_levels(glv, lv, 3)
    assert np.array_equal(got.cpu().numpy(), want) and (want != photo).any()
    assert np.array_equal(_blend(photo, edits, matrix, region, 3, 2.0, whole=False), want[:, 2:5, 2:7])


@pytest.mark.parametrize('side,eye_avg', [('left', (10.5, 40.5)), ('right', (90.5, 40.5)), ('top', (50.5, 5.5)), ('bottom', (50.5, 80.5))])
def test_window_clamped_on_each_side(side, eye_avg):
    from inv3d_amd.images import paste_plan
    photo, S = PC.EXACT_PHOTO, 64
    lm = P.upright_landmarks(eye_avg, (16, 0), (0, 10))
    plan = paste_plan(100, 100, lm, S)
    x0, y0, x1, y1 = plan.region
    assert dict(left=x0 == 0, right=x1 == 100, top=y0 == 0, bottom=y1 == 100)[side]
    wx0, wy0, wx1, wy1 = B.window(plan.region, 2, 100, 100)
    assert dict(left=wx0 == 0, right=wx1 == 100, top=wy0 == 0, bottom=wy1 == 100)[side] and (wx1 - wx0) * (wy1 - wy0) < 10000
    edit = TC.noise_image(S, S, 3, 77)
    for whole in (True, False):
        assert np.array_equal(_blend(photo, edit, plan.matrix, plan.region, 2, 6.0, whole=whole),
                              B.blend8(photo, edit, plan.matrix, plan.region, 2, 6.0, whole=whole)), whole


def test_grey_equals_a_channel_of_colour():
    photo = np.repeat(TC.noise_image(70, 90, 1, 8), 3, -1)
    edits = np.repeat(TC.noise_image(40, 40, 1, 9), 3, -1)[None]
    mask = TC.noise_image(40, 40, 1, 10)[..., 0]
    matrix, region = (-4.0, 0.55, 0.1, -3.0, -0.1, 0.55), (12, 9, 80, 66)
    for bands in (1, 3):
        colour = _blend(photo, edits, matrix, region, bands, 4.0, mask)
        grey = _blend(photo[..., :1], edits[..., :1], matrix, region, bands, 4.0, mask)
        assert grey.shape == (1, 70, 90, 1) and np.array_equal(grey[..., 0], colour[..., 0]) and (colour[0] != photo).any()
        assert np.array_equal(grey, B.blend8(photo[..., :1], edits[..., :1], matrix, region, bands, 4.0, mask))
        assert np.array_equal(_blend(photo[..., :1], edits[..., :1], matrix, region, bands, 4.0, mask, layout='chw'), grey.transpose(0, 3, 1, 2))


def test_subnormal_alpha_tails_are_kept():
    """The hazard of the header: feather values of about 1e-37 times a mask of 16 / 255 put alpha_0 on both sides of the smallest normal
    fp32 (the fp64 -> fp32 conversion lands on subnormals), and every reduce keeps some of it there.  numpy keeps subnormals; the kernels
    must too -- compared bit for bit in the workspace, since a weight that small cannot move a byte of the output."""
    from inv3d_amd import hipops as H
    photo = TC.noise_image(40, 40, 3, 90)
    edits = TC.noise_image(8, 8, 3, 91)[None]
    mask = np.full((8, 8), 16, np.uint8)
    matrix, region = (2.0 ** -63, 2.0 ** -65, 0.0, 4.0, 0.0, 0.0), (0, 0, 40, 40)       # u = 2^-63 + 2^-65 (X + 0.5): d = u, f = u, a ~ 3 u^2
    want, lv = B.blend8(photo, edits, matrix, region, 3, 1.0, mask, return_levels=True)
    tiny = np.finfo(np.float32).tiny
    for k in (0, 1, 2, 3):
        a = lv['alpha'][k]
        assert (a > 0).all() and (a < tiny).any() and a.max() < 1e-35, k
    assert (lv['alpha'][0] >= tiny).any()
    got, glv = H.paste_blend(_gpu(photo), _gpu(edits), matrix, region, 3, 1.0, _gpu(mask), return_levels=True)
    _same_levels(glv, lv, 3)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want[0], photo)


def test_bands_zero_is_todays_call_and_bands_two_changes_only_the_window():
    from inv3d_amd import images
    photo, lm = GP._rotated_photo()
    edit = TC.noise_image(48, 48, 3, 51)
    today = images.paste_back(_gpu(photo), _gpu(edit), lm)
    assert torch.equal(images.paste_back(_gpu(photo), _gpu(edit), lm, bands=0), today)
    for region in ('photo', 'bbox'):
        assert torch.equal(images.paste_back(_gpu(photo), _gpu(edit), lm, bands=0, region=region), images.paste_back(_gpu(photo), _gpu(edit), lm, region=region))
    two = images.paste_back(_gpu(photo), _gpu(edit), lm, bands=2).cpu().numpy()
    assert np.array_equal(two, blend_full_ref(photo, edit, lm, 2))
    plan = images.paste_plan(160, 160, lm, 48)
    wx0, wy0, wx1, wy1 = B.window(plan.region, 2, 160, 160)
    changed = (two != today.cpu().numpy()).any(-1)
    assert changed.any()
    changed[wy0:wy1, wx0:wx1] = False
    assert not changed.any() and (wx1 - wx0) * (wy1 - wy0) < 160 * 160
    outside = np.ones((160, 160), bool)
    outside[wy0:wy1, wx0:wx1] = False
    assert np.array_equal(two[outside], photo[outside])


def test_minification_presizes_with_lanczos():
    """Scale 2: the face is 64 px in the photo, the edit 128: the blend comes after the same Pillow-LANCZOS presize as the one-alpha paste."""
    from inv3d_amd import images
    photo, lm = PC.EXACT_PHOTO, P.EXACT_LANDMARKS[0]
    edits = np.stack([TC.smooth_image(128, 128, 4), TC.noise_image(128, 128, 3, 6)])
    mask = TC.smooth_image(128, 128, 12)[..., 0]
    assert images.paste_plan(100, 100, lm, 128).presize == 64
    for region in ('photo', 'bbox'):
        for m in (None, mask):
            got = images.paste_back(_gpu(photo), _gpu(edits), lm, mask=None if m is None else _gpu(m), region=region, bands=2).cpu().numpy()
            assert np.array_equal(got, blend_full_ref(photo, edits, lm, 2, mask=m, region=region)), (region, m is None)
    one = images.paste_back(_gpu(photo), _gpu(edits[0]), lm, bands=3).cpu().numpy()
    assert one.shape == photo.shape and np.array_equal(one, blend_full_ref(photo, edits[0], lm, 3))
    with pytest.raises(ValueError):
        images.paste_back(_gpu(photo), _gpu(edits), P.upright_landmarks((-500.5, 40.5), (16, 0), (0, 10)), region='bbox', bands=2)
    outside = images.paste_back(_gpu(photo), _gpu(edits), P.upright_landmarks((-500.5, 40.5), (16, 0), (0, 10)), bands=2).cpu().numpy()
    assert np.array_equal(outside, np.repeat(photo[None], 2, 0))


def test_zero_mask_gives_the_photo():
    photo, lm, S, plan, edits, _ = GP._plan_case('inside')
    zero = np.zeros((S, S), np.uint8)
    for bands in (1, 3):
        assert np.array_equal(_blend(photo, edits, plan.matrix, plan.region, bands, 0.08 * S, zero), np.repeat(photo[None], 2, 0))


def test_auto_resolves_to_paste_bands():
    from inv3d_amd import images
    for name, feather in (('inside', 0.08), ('crop_only', 0.3), ('exact0', 0.5)):
        photo, lm, S, plan, edits, _ = GP._plan_case(name)
        n = images.paste_bands(plan, S, feather)
        assert 1 <= n <= 5
        auto = images.paste_back(_gpu(photo), _gpu(edits), lm, feather=feather, bands='auto')
        assert torch.equal(auto, images.paste_back(_gpu(photo), _gpu(edits), lm, feather=feather, bands=n))
        assert not torch.equal(auto, images.paste_back(_gpu(photo), _gpu(edits), lm, feather=feather, bands=n + 1))
    assert {images.paste_bands(GP._plan_case(nm)[3], GP._plan_case(nm)[2], f) for nm, f in (('inside', 0.08), ('crop_only', 0.3), ('exact0', 0.5))} != {1}


def test_both_builds_give_the_same_bytes():
    import blend_digest
    here = blend_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'blend_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
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
    assert H.paste_blend(photo, edits, m, r, 2).shape == (2, 20, 30, 3)
    for call in (lambda: H.paste_blend(photo, edits, m, (0, 0, 31, 8), 2), lambda: H.paste_blend(photo, edits, m, (5, 0, 4, 8), 2),
                 lambda: H.paste_blend(photo, edits, m[:5], r, 2), lambda: H.paste_blend(photo, edits[..., :1], m, r, 2),
                 lambda: H.paste_blend(photo, edits[:, :, :7], m, r, 2), lambda: H.paste_blend(photo[None], edits, m, r, 2),
                 lambda: H.paste_blend(photo, edits, m, r, 2, layout='nchw'), lambda: H.paste_blend(photo, edits, m, r, 2, feather_px=-1.0),
                 lambda: H.paste_blend(photo, edits, m, r, 2, mask=torch.zeros((3, 8, 8), dtype=torch.uint8, device=DEV)),
                 lambda: H.paste_blend(photo, edits.float(), m, r, 2), lambda: H.paste_blend(photo, edits, m, r, 0),
                 lambda: H.paste_blend(photo, edits, m, r, 7), lambda: H.paste_blend(photo, edits, m, r, 2.5),
                 lambda: H.paste_blend(photo, edits, m, r, 'auto')):
        with pytest.raises(Eg3dHipError):
            call()


# ------------------------------------------------------------------------------------------------------------------------------------ consumers
def test_orbit_video_paste_bands(tmp_path):
    from PIL import Image
    import io
    from inv3d_amd import images, video as V
    from test_gpu_video import _small_generator
    from test_video_cpu import check_avi
    G, ws, _, target, uni = _small_generator()
    S = int(target.shape[-1])
    photo, lm = GP._rotated_photo()
    x0, y0, x1, y1 = images.paste_plan(160, 160, lm, S).region
    kw = dict(num_frames=3, fps=30, quality=85, batch=2, force_fp32=True, render_uniforms=uni)
    files = {}
    for tag, pkw in (('plain', None), ('zero', dict(bands=0)), ('two', dict(bands=2)), ('matte', dict(bands=2, matte=True))):
        path = str(tmp_path / f'{tag}.avi')
        assert V.write_orbit_video(G, ws, path, paste=(_gpu(photo), lm), paste_kwargs=pkw, **kw) == 3
        files[tag] = open(path, 'rb').read()
        a = check_avi(files[tag], 3, 30, x1 - x0, y1 - y0)                               # frames of the bounding box's size
        for f in a['frames']:
            assert Image.open(io.BytesIO(f)).size == (x1 - x0, y1 - y0)
    assert files['zero'] == files['plain'] and files['two'] != files['plain'] and files['matte'] != files['two']


def test_paste_back_tool_bands(tmp_path):
    """tools/paste_back.py (in process): --paste-bands 2 writes images.paste_back(bands=2)'s bytes; without the flag, today's."""
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import paste_back as tool
    photo, lm = GP._rotated_photo()
    edit = TC.noise_image(48, 48, 3, 51)
    V.write_png(str(tmp_path / 'me.png'), photo)
    V.write_png(str(tmp_path / 'edit0.png'), edit)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    base = ['--photo', str(tmp_path / 'me.png'), '--landmarks', str(tmp_path / 'lm.npz'), '--edit', str(tmp_path / 'edit0.png')]
    plain = tool.main(base + ['--out-dir', str(tmp_path / 'plain')])
    two = tool.main(base + ['--out-dir', str(tmp_path / 'two'), '--paste-bands', '2'])
    auto = tool.main(base + ['--out-dir', str(tmp_path / 'auto'), '--paste-bands', 'auto', '--bbox'])
    assert np.array_equal(GP._read_png(plain[0]), images.paste_back(_gpu(photo), _gpu(edit), lm).cpu().numpy())
    want = images.paste_back(_gpu(photo), _gpu(edit), lm, bands=2).cpu().numpy()
    assert np.array_equal(GP._read_png(two[0]), want) and (want != GP._read_png(plain[0])).any()
    assert np.array_equal(GP._read_png(auto[0]), images.paste_back(_gpu(photo), _gpu(edit), lm, bands='auto', region='bbox').cpu().numpy())
    with pytest.raises(SystemExit):
        tool.main(base + ['--out-dir', str(tmp_path / 'bad'), '--paste-bands', '9'])


def test_run_ganspace_tool_bands(tmp_path):
    import importlib.util
    from inv3d_amd import images, video as V
    from test_gpu_video import _small_generator
    spec = importlib.util.spec_from_file_location('run_ganspace_tool', os.path.join(ROOT, 'tools', 'run_ganspace.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, ws, cam, _, _ = _small_generator()
    photo, lm = GP._rotated_photo()
    V.write_png(str(tmp_path / 'me.png'), photo)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    np.save(str(tmp_path / 'comp.npy'), np.linalg.qr(np.random.RandomState(1).normal(size=(32, 32)))[0].astype(np.float32))
    np.save(str(tmp_path / 'a_ws.npy'), ws.cpu().numpy())
    np.save(str(tmp_path / 'a_cam.npy'), cam.cpu().numpy())
    args = ['edit', '--synthetic', 'small', '--components', str(tmp_path / 'comp.npy'), '--ws', str(tmp_path / 'a_ws.npy'), '--cam',
            str(tmp_path / 'a_cam.npy'), '--params', '1', '0', '3', '2.5', '--num-imgs', '3', '--name', 'a', '--paste-photo', str(tmp_path / 'me.png'),
            '--landmarks', str(tmp_path / 'lm.npz')]
    plain = tool.main(args + ['--out-dir', str(tmp_path / 'plain')])
    two = tool.main(args + ['--out-dir', str(tmp_path / 'two'), '--paste-bands', '2'])
    assert torch.equal(plain['pasted'], images.paste_back(_gpu(photo), plain['images'], lm, region='bbox'))
    want = images.paste_back(_gpu(photo), two['images'], lm, region='bbox', bands=2)
    assert torch.equal(two['pasted'], want) and two['pasted'].shape == plain['pasted'].shape and not torch.equal(two['pasted'], plain['pasted'])
    assert np.array_equal(GP._read_png(str(tmp_path / 'two' / 'a_pasted.png')), np.concatenate(list(want.cpu().numpy()), 1))


class _Spy:
    """Records (args, kwargs, result) of every call of module.name while active."""

    def __init__(self, module, name):
        self.module, self.name, self.calls = module, name, []

    def __enter__(self):
        self.real = getattr(self.module, self.name)

        def wrapper(*a, **kw):
            out = self.real(*a, **kw)
            self.calls.append((a, kw, out))
            return out
        setattr(self.module, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.module, self.name, self.real)


def test_render_video_tool_bands(tmp_path):
    from inv3d_amd import images, video as V
    from test_gpu_video import _small_generator
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import render_video
    _, ws, _, _, _ = _small_generator()
    photo, lm = GP._rotated_photo()
    V.write_png(str(tmp_path / 'me.png'), photo)
    np.savez(str(tmp_path / 'lm.npz'), me=lm)
    np.save(str(tmp_path / 'ws.npy'), ws.cpu().numpy())
    args = ['--ws', str(tmp_path / 'ws.npy'), '--synthetic', 'small', '--frames', '3', '--batch', '2', '--paste-photo', str(tmp_path / 'me.png'),
            '--landmarks', str(tmp_path / 'lm.npz')]
    with _Spy(images, 'paste_back') as pb:
        assert render_video.main(args + ['--out', str(tmp_path / 'two.avi'), '--paste-bands', '2']) == 3
    assert [c[1]['bands'] for c in pb.calls] == [2, 2]
    with _Spy(images, 'paste_back') as pb:
        assert render_video.main(args + ['--out', str(tmp_path / 'plain.avi')]) == 3
    assert len(pb.calls) == 2 and all('bands' not in c[1] for c in pb.calls)         # without the flag: the call it made before
    with pytest.raises(SystemExit):
        render_video.main(['--ws', str(tmp_path / 'ws.npy'), '--synthetic', 'small', '--out', str(tmp_path / 'bad.avi'), '--paste-bands', '2'])


def test_run_inversion_tool_bands(tmp_path):
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_inversion
    case = PC.CASES['inside']
    d = tmp_path / 'photos'
    d.mkdir()
    V.write_png(str(d / 'inside.png'), case['image'])
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, inside=case['landmarks'])
    base = ['--in-dir', str(d), '--landmarks', lm_path, '--synthetic', 'small', '--steps-a', '1', '--steps-b', '1', '--paste-back']
    with _Spy(images, 'paste_back') as pb:
        run_inversion.main(base + ['--out-dir', str(tmp_path / 'out'), '--paste-bands', 'auto'])
    (pargs, pkw, pasted), = pb.calls
    assert pkw['bands'] == 'auto'
    png = GP._read_png(str(tmp_path / 'out' / 'pasted' / 'inside.png'))
    S = int(pargs[1].shape[-1])
    n = images.paste_bands(images.paste_plan(case['image'].shape[0], case['image'].shape[1], case['landmarks'], S), S, 0.08)
    want = images.paste_back(_gpu(case['image']), pargs[1], case['landmarks'], bands=n)[0].cpu().numpy()
    assert np.array_equal(png, want) and np.array_equal(png, pasted[0].cpu().numpy())
    assert not np.array_equal(png, images.paste_back(_gpu(case['image']), pargs[1], case['landmarks'])[0].cpu().numpy())
    with _Spy(images, 'paste_back') as pb:
        run_inversion.main(base + ['--out-dir', str(tmp_path / 'plain')])
    assert 'bands' not in pb.calls[0][1]                                                 # without the flag: the call it made before
    with pytest.raises(SystemExit):
        run_inversion.main(['--in-dir', str(d), '--out-dir', str(tmp_path / 'o2'), '--synthetic', 'small', '--paste-bands', '2'])
