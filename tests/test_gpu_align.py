"""Target-image ingestion on the GPU (csrc/imgprep.hip, hipops.pil_resize / pil_quad_warp / feather_pad / u8_to_target, inv3d_amd/images.py):
the resize and the QUAD warp EQUAL Pillow and the numpy restatement byte for byte, the feathered pad and the whole align_face keep the pad
bound of tests/test_align_cpu.py against the reference's scipy / numpy statements and against tests/golden/align.npz, the uint8 -> [-1, 1]
conversion equals torch's bits, both builds give the same bytes, and a directory of PNGs goes through load_targets into InversionCoach.run.

Measured on an MI355X: no byte differs from the scipy statements on any pad shape and from the reference on any golden case."""
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
import pil_ref as R  # noqa: E402
import test_align_cpu as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# the CPU cases plus: more than one tile of 64 output columns with a remainder, and the exact ratio 4 of the shrink step
RESIZE_CASES = TC.RESIZE_CASES + [((50, 200), (130, 40), 3), ((300, 260), (65, 75), 3)]
QUADS = dict(TC.QUADS, outside=(-100, -100, -100, -50, -50, -50, -50, -100))


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _resize_case(i, filter):
    hw, size, ch = RESIZE_CASES[i]
    img = TC.noise_image(hw[0], hw[1], ch, 31 + i)
    return img, size, TC.pil_resize(img, size, filter), R.resize8(img, size, filter)


@pytest.mark.parametrize('filter', ['bilinear', 'lanczos'])
@pytest.mark.parametrize('i', range(len(RESIZE_CASES)))
def test_resize_is_byte_equal_to_pillow_and_the_restatement(i, filter):
    from inv3d_amd import hipops as H
    img, size, pil, rest = _resize_case(i, filter)
    got = H.pil_resize(_gpu(img), size, filter).cpu().numpy()
    assert got.shape == pil.shape and np.array_equal(got, pil) and np.array_equal(got, rest)


@pytest.mark.parametrize('filter', ['bilinear', 'lanczos'])
def test_resize_batch_of_three(filter):
    from inv3d_amd import hipops as H
    imgs = np.stack([TC.noise_image(37, 53, 3, 70 + k) for k in range(3)])
    got = H.pil_resize(_gpu(imgs), (16, 11), filter).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], TC.pil_resize(imgs[k], (16, 11), filter)), k


@pytest.mark.parametrize('name', sorted(QUADS))
def test_quad_warp_is_byte_equal_to_pillow(name):
    from inv3d_amd import hipops as H
    img = TC.noise_image(TC.QUAD_IMAGE[0], TC.QUAD_IMAGE[1], 3, 7)
    got = H.pil_quad_warp(_gpu(img), TC.QUAD_SIZE, QUADS[name]).cpu().numpy()
    assert np.array_equal(got, TC.pil_quad(img, TC.QUAD_SIZE, QUADS[name]))
    if name == 'outside':
        assert not got.any()
    grey = H.pil_quad_warp(_gpu(img[..., :1]), TC.QUAD_SIZE, QUADS[name]).cpu().numpy()          # C = 1 is its own instantiation
    assert np.array_equal(grey, got[..., :1])


@pytest.mark.parametrize('hw,pads,qsize', TC.PAD_CASES)
def test_feather_pad_against_the_scipy_statements(hw, pads, qsize):
    from inv3d_amd import hipops as H
    img = TC.smooth_image(hw[0], hw[1], hw[0])
    got = H.feather_pad(_gpu(img), pads, qsize).cpu().numpy()
    TC.pad_bound(got, R.scipy_pad(img, pads, qsize), pads, f'GPU {hw} {pads}')
    rest = R.feather_pad(img, pads, qsize)
    print(f'GPU vs fp32 restatement: {int((got != rest).any(-1).sum())} pixels differ')


def test_feather_pad_batch_equals_single_calls():
    """The summation order is a function of the pixel alone and the median is per image: a batch gives the bytes of its images one at a time.
    The two images have different medians; 111 x 83 values per channel and image is an odd count, the first of PAD_CASES an even one."""
    from inv3d_amd import hipops as H
    imgs = np.stack([TC.smooth_image(60, 64, 5), 255 - TC.smooth_image(60, 64, 6)])
    pads, qsize = (12, 20, 7, 31), 80
    both = H.feather_pad(_gpu(imgs), pads, qsize).cpu().numpy()
    for k in range(2):
        one = H.feather_pad(_gpu(imgs[k]), pads, qsize).cpu().numpy()
        assert np.array_equal(both[k], one), k
        TC.pad_bound(one, R.scipy_pad(imgs[k], pads, qsize), pads, f'GPU batch image {k}')


def test_u8_to_target_is_bit_equal_to_torch():
    """Every byte value, on the device and against the host pipeline.  The divisor is a device tensor: with a host scalar torch's GPU kernel
    multiplies by the rounded reciprocal of 255, which differs from the division ToTensor performs on the host in 126 of the 256 values."""
    from inv3d_amd import hipops as H
    x = torch.from_numpy(np.random.RandomState(3).permutation(np.arange(2 * 16 * 24 * 3) % 256).astype(np.uint8).reshape(2, 16, 24, 3)).to(DEV)
    got = H.u8_to_target(x)
    want = (x.permute(0, 3, 1, 2).float() / torch.tensor(255.0, device=DEV) - 0.5) / 0.5
    assert got.shape == (2, 3, 16, 24) and got.dtype == torch.float32 and torch.equal(got, want)
    host = x.cpu().permute(0, 3, 1, 2).float().div(255).sub_(0.5).div_(0.5)                     # ToTensor + Normalize(0.5, 0.5)
    assert torch.equal(got.cpu(), host)


def test_e4e_image_transform_equals_the_pil_pipeline():
    from PIL import Image
    from inv3d_amd import images
    t = torch.from_numpy(np.random.RandomState(4).uniform(0, 1, (2, 3, 40, 52)).astype(np.float32))
    got = images.e4e_image_transform(t.to(DEV)).cpu()
    for k in range(2):
        u8 = t[k].mul(255).byte().permute(1, 2, 0).numpy()                                      # ToPILImage
        r = np.asarray(Image.fromarray(u8).resize((256, 256), Image.BILINEAR))                  # Resize((256, 256)): bilinear, antialiased
        want = torch.from_numpy(r.copy()).permute(2, 0, 1).float().div(255).sub_(0.5).div_(0.5)
        assert torch.equal(got[k], want), k


@pytest.mark.parametrize('name', sorted(TC.align_cases()))
def test_align_face_reproduces_the_reference(name):
    from inv3d_amd import images
    case = TC.align_cases()[name]
    got = images.align_face(_gpu(case['image']), case['landmarks'], case['output_size']).cpu().numpy()
    assert got.shape == case['aligned'].shape
    TC.align_bound(got, case, f'GPU {name}')


def test_both_builds_give_the_same_bytes():
    import align_digest
    here = align_digest.digests()
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'align_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    det = json.loads(r.stdout.strip().splitlines()[-1])
    assert det.pop('deterministic_build') is True
    here.pop('deterministic_build')
    assert det == here


def test_invalid_arguments_are_refused():
    from inv3d_amd import hipops as H
    from inv3d_amd._lib import Eg3dHipError
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for call in (lambda: H.pil_resize(x, (4, 4), 'bicubic'), lambda: H.pil_resize(x, (0, 4)), lambda: H.pil_resize(x.float(), (4, 4)),
                 lambda: H.pil_resize(x[..., :2], (4, 4)), lambda: H.feather_pad(x, (0, 1, 1, 1), 10), lambda: H.u8_to_target(x[..., :1]),
                 lambda: H.pil_quad_warp(x, (0, 3), (0, 0, 0, 8, 8, 8, 8, 0))):
        with pytest.raises(Eg3dHipError):
            call()


def test_load_targets_into_a_coach_run(tmp_path):
    """A directory of PNGs -> load_targets -> InversionCoach.run: the tuples are accepted and a result per image comes back."""
    from inv3d_amd import images, video as V
    from inv3d_amd.coach import InversionCoach
    from test_gpu_video import _small_generator
    G, _, _, target, uni = _small_generator()
    S = int(target.shape[-1])
    cases = TC.align_cases()
    d = tmp_path / 'photos'
    d.mkdir()
    V.write_png(str(d / 'b_inside.png'), torch.from_numpy(cases['inside']['image']))
    square = TC.smooth_image(S, S, 9)
    V.write_png(str(d / 'a_square.png'), torch.from_numpy(square))
    (d / 'notes.txt').write_text('not an image')
    lm_path = str(tmp_path / 'landmarks.json')
    json.dump({'b_inside': cases['inside']['landmarks'].tolist()}, open(lm_path, 'w'))
    targets = images.load_targets(str(d), lm_path, output_size=S, device=DEV)
    assert [t[0] for t in targets] == ['a_square', 'b_inside'] and all(t[2] is None for t in targets)
    for _, t, _ in targets:
        assert t.shape == (1, 3, S, S) and t.dtype == torch.float32 and t.is_cuda and float(t.abs().max()) <= 1.0
    assert torch.equal(targets[0][1], (torch.from_numpy(square).to(DEV).permute(2, 0, 1)[None].float() / torch.tensor(255.0, device=DEV) - 0.5) / 0.5)
    want = images.align_face(_gpu(cases['inside']['image']), cases['inside']['landmarks'], S)
    from inv3d_amd import hipops as H
    assert torch.equal(targets[1][1], H.u8_to_target(want))
    with pytest.raises(ValueError):
        images.load_targets(str(d), None, output_size=S, device=DEV)                            # b_inside is 100 x 100 and has no landmarks
    coach = InversionCoach(G, first_inv_steps=2, max_pti_steps=2, lpips_threshold=0.0, seed=3, w_avg_samples=0, synth_kwargs=dict(render_uniforms=uni))
    results, stats = coach.run(targets)
    assert [r.name for r in results] == ['a_square', 'b_inside'] and stats['n_done'] == 2
    for r in results:
        assert r.steps_a == 2 and np.isfinite(r.psnr_tuned) and r.w_pivot.shape[0] == 1


def _photo_dir(tmp_path, names):
    from inv3d_amd import video as V
    cases = TC.align_cases()
    d = tmp_path / 'photos'
    d.mkdir()
    for n in names:
        V.write_png(str(d / (n + '.png')), cases[n]['image'])
    lm_path = str(tmp_path / 'landmarks.npz')
    np.savez(lm_path, **{n: cases[n]['landmarks'] for n in names})
    return str(d), lm_path, cases


def test_align_images_tool(tmp_path):
    """tools/align_images.py (in process): a directory of photographs plus a landmarks file -> the aligned PNGs, align_face's bytes."""
    from PIL import Image
    from inv3d_amd import images, video as V
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import align_images
    d, lm_path, cases = _photo_dir(tmp_path, ['pad_edge', 'shrink'])
    V.write_png(os.path.join(d, 'stranger.png'), TC.smooth_image(20, 20, 1))                    # no landmarks: reported and skipped
    out = str(tmp_path / 'aligned')
    written = align_images.main(['--in-dir', d, '--landmarks', lm_path, '--out-dir', out, '--output-size', '32'])
    assert sorted(os.listdir(out)) == ['pad_edge.png', 'shrink.png'] and len(written) == 2
    for n in ('pad_edge', 'shrink'):
        want = images.align_face(_gpu(cases[n]['image']), cases[n]['landmarks'], 32).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, n + '.png'))), want)


def test_run_inversion_tool(tmp_path):
    """tools/run_inversion.py (in process): the same directory through coach.run on the small synthetic generator, options switched through."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_inversion
    d, lm_path, _ = _photo_dir(tmp_path, ['inside'])
    out = str(tmp_path / 'out')
    results, stats = run_inversion.main(['--in-dir', d, '--landmarks', lm_path, '--out-dir', out, '--synthetic', 'small', '--steps-a', '1',
                                         '--steps-b', '1', '--save-grid', '--save-pivot'])
    assert [r.name for r in results] == ['inside'] and stats['n_done'] == 1
    assert sorted(os.listdir(out)) == ['media', 'pivot'] and sorted(os.listdir(os.path.join(out, 'pivot'))) == ['inside_cam.npy', 'inside_ws.npy']
    assert os.path.exists(os.path.join(out, 'media', 'inside.png')) and os.path.exists(os.path.join(out, 'media', 'pivot', 'inside.png'))
