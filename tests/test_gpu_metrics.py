"""Reconstruction metrics on the GPU (csrc/ssim.hip, inv3d_amd.metrics, the coach's do_evaluation / save_pivot): MS-SSIM / SSIM values and
gradients against the float64 restatement tests/support/msssim_ref.py -- at least as accurate as the fp32 composite they replace --,
bit-identical results run to run, from the deterministic build and from a replayed graph, the face crop + pool, the ArcFace identity
distance against the reference's own Backbone (tests/golden/identity.npz) and the per-image evaluation of single_id_coach.py:87-117."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
import id_ref as IR  # noqa: E402
import msssim_ref as M  # noqa: E402
from ssim_digest import inputs as digest_inputs, run as digest_run  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _pair(shape, seed, scale=1.0, offset=0.0, noise=0.2, sign=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    y = sign * x + (1 - sign) / 2 + noise * torch.randn(shape, generator=g, dtype=torch.float64)     # sign -1: 1 - x, anti-correlated
    return x * scale + offset, y * scale + offset


def _errs(fn, ref_fn, x, y, **kw):
    """(|kernel - f64|, |fp32 composite - f64|) elementwise maxima of the metric."""
    want = ref_fn(x, y, **kw)
    got = fn(x.float().to(DEV), y.float().to(DEV), **kw).double().cpu()
    f32 = ref_fn(x.float().to(DEV), y.float().to(DEV), **kw).double().cpu()
    assert got.shape == want.shape
    return float((got - want).abs().max()), float((f32 - want).abs().max()), want


VALUE_CASES = [
    ('512x512_N2', (2, 3, 512, 512), dict(), dict(data_range=1)),
    ('odd_177x203', (2, 3, 177, 203), dict(), dict(data_range=1)),
    ('outside_01', (1, 3, 200, 224), dict(scale=2.5, offset=-1.2), dict(data_range=1)),
    ('range_255', (2, 3, 192, 192), dict(scale=255.0), dict(data_range=255)),
]


@pytest.mark.parametrize('name,shape,pk,kw', VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
@pytest.mark.parametrize('size_average', [False, True])
def test_ms_ssim_value(name, shape, pk, kw, size_average):
    from inv3d_amd.metrics import ms_ssim
    x, y = _pair(shape, 3, **pk)
    e, e32, want = _errs(ms_ssim, M.ms_ssim, x, y, size_average=size_average, **kw)
    assert float(want.min()) > 0.05                                # a non-trivial value
    assert e <= max(1e-6, e32), (e, e32)


@pytest.mark.parametrize('nonneg', [False, True])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_ssim_value(nonneg, sign):
    from inv3d_amd.metrics import ssim
    x, y = _pair((2, 3, 96, 131), 5, sign=sign)
    e, e32, want = _errs(ssim, M.ssim, x, y, size_average=False, data_range=1, nonnegative_ssim=nonneg)
    if sign < 0:
        assert float(want.max()) == 0.0 if nonneg else float(want.max()) < 0
    assert e <= max(1e-6, e32), (e, e32)


def _grads(fn, x, y):
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = fn(xs, ys)
    (out * torch.arange(1, out.numel() + 1, dtype=out.dtype, device=out.device).view(out.shape)).sum().backward()
    return xs.grad.double().cpu(), ys.grad.double().cpu()


@pytest.mark.parametrize('which', ['ms_ssim', 'ssim'])
def test_gradients(which):
    from inv3d_amd import metrics as MT
    x, y = _pair((2, 3, 177, 190), 7)
    ours = getattr(MT, which)
    ref = getattr(M, which)
    kw = dict(data_range=1, size_average=False)
    want = _grads(lambda a, b: ref(a, b, **kw), x, y)
    got = _grads(lambda a, b: ours(a, b, **kw), x.float().to(DEV), y.float().to(DEV))
    f32 = _grads(lambda a, b: ref(a, b, **kw), x.float().to(DEV), y.float().to(DEV))
    for g, w, h in zip(got, want, f32):
        e, e32 = float((g - w).abs().max()), float((h - w).abs().max())
        assert e <= max(1e-5 * float(w.abs().max()), 2 * e32), (which, e, e32, float(w.abs().max()))


def test_only_the_requested_gradient():
    from inv3d_amd.metrics import ms_ssim
    x, y = _pair((1, 3, 170, 170), 8)
    xs = x.float().to(DEV).requires_grad_(True)
    ms_ssim(xs, y.float().to(DEV), data_range=1).backward()
    want = _grads(lambda a, b: M.ms_ssim(a, b, data_range=1), x, y)[0]
    assert float((xs.grad.double().cpu() - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_clamped_level_gives_zero_gradient():
    """Anti-correlated images: every level's mean cs is negative, relu clamps it, the value is 0 -- the gradient is 0, not NaN."""
    from inv3d_amd.metrics import ms_ssim
    x, y = _pair((1, 3, 176, 176), 9, sign=-1.0, noise=0.05)
    _, cs = M.ssim_cs(x, y, data_range=1)
    assert float(cs.max()) < 0
    xs, ys = x.float().to(DEV).requires_grad_(True), y.float().to(DEV).requires_grad_(True)
    v = ms_ssim(xs, ys, data_range=1)
    v.backward()
    assert float(v.detach()) == 0.0
    for g in (xs.grad, ys.grad):
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0


def test_bit_identical_runs_builds_and_graph_replay():
    x, y = digest_inputs(DEV)
    first = digest_run(x, y)
    assert digest_run(x, y) == first
    # the deterministic build, in a fresh interpreter (tests/test_gpu_det.py)
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'ssim_digest.py')], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == first
    # captured forward + backward, replayed on new inputs copied into the static ones
    from inv3d_amd.metrics import ms_ssim
    xs, ys = torch.zeros_like(x).requires_grad_(True), torch.zeros_like(y)
    with torch.no_grad():
        xs.copy_(x * 0.5)
        ys.copy_(y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            v = ms_ssim(xs, ys, data_range=1, size_average=False)
            torch.autograd.grad(v.sum(), xs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = ms_ssim(xs, ys, data_range=1, size_average=False)
        gx, = torch.autograd.grad(v.sum(), xs)
    with torch.no_grad():
        xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    eager_v = ms_ssim(x, y, data_range=1, size_average=False)
    xe = x.clone().requires_grad_(True)
    eager_g, = torch.autograd.grad(ms_ssim(xe, y, data_range=1, size_average=False).sum(), xe)
    assert torch.equal(v, eager_v) and torch.equal(gx, eager_g)


@pytest.mark.parametrize('size', [512, 256, 192])
def test_face_pool(size):
    from inv3d_amd import hipops as H
    g = torch.Generator().manual_seed(size)
    x = torch.randn(2, 3, size, size, generator=g)
    r0, r1, _ = slice(35, 223).indices(size)
    c0, c1, _ = slice(32, 220).indices(size)
    got = H.face_pool(x.to(DEV), r0, r1, c0, c1, 112)
    assert got.shape == (2, 4, 112, 112) and got.is_contiguous(memory_format=torch.channels_last)
    want = IR.face_crop_pool(x.double())
    got = got.double().cpu()
    assert float((got[:, :3] - want).abs().max()) <= 1e-6 and float(got[:, 3].abs().max()) == 0.0


@pytest.fixture(scope='module')
def id_golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'identity.npz'))


def test_id_loss_vs_reference(id_golden):
    from inv3d_amd.metrics import IDLoss
    net = IDLoss().to(DEV)
    net.facenet.load_state_dict(IR.synth_state(int(id_golden['seed'])), strict=True)
    for size in IR.SIZES:
        y_hat, y = IR.images(size, int(id_golden['seed']))
        f = net.extract_feats(torch.cat([y_hat, y]).to(DEV)).cpu()
        assert float((f - torch.from_numpy(id_golden[f'feats_{size}'])).abs().max()) <= 2e-5, size
        d = net.identity_distance(y_hat.to(DEV), y.to(DEV)).cpu()
        assert float((d - torch.from_numpy(id_golden[f'dist_{size}'])).abs().max()) <= 2e-5, size
        loss = net(y_hat.to(DEV), y.to(DEV))
        assert loss.dim() == 0 and abs(float(loss) - float(id_golden[f'loss_{size}'])) <= 2e-5, size


def test_id_loss_empty_crop():
    from inv3d_amd.metrics import IDLoss
    net = IDLoss().to(DEV)
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError):
        net(x, x)


def _eval_generator():
    """sr_in_res = nrr = 64: the SR head makes 256^2 images (MS-SSIM needs a side > 160, the face crop 223 rows)."""
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=64, sr_in_res=64, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    with torch.no_grad():
        target = G.synthesis(O.synth_ws(cfg, 1, seed=7).to(DEV), cam, noise_mode='const', force_fp32=True)['image'].clamp(-1, 1)
    return G, cam, target


def test_coach_evaluation_and_pivots(tmp_path):
    from inv3d_amd.coach import InversionCoach
    from inv3d_amd.loss_nets import LPIPSAlex
    from inv3d_amd.metrics import IDLoss, format_metrics_txt, reconstruction_metrics
    G, cam, target = _eval_generator()
    assert target.shape[-1] == 256
    kw = dict(first_inv_steps=2, max_pti_steps=2, lpips_threshold=0.0, seed=3, w_avg_samples=0)
    pristine = {k: v.detach().clone() for k, v in G.state_dict().items()}
    cwd_before = set(os.listdir(os.getcwd()))
    r0 = InversionCoach(G, **kw).invert('a', target, cam)
    assert r0.metrics is None and set(os.listdir(os.getcwd())) == cwd_before
    G.load_state_dict(pristine)
    lp, idn = LPIPSAlex('pm1').to(DEV), IDLoss().to(DEV)
    ev, pv = str(tmp_path / 'eval'), str(tmp_path / 'pivots')
    coach = InversionCoach(G, do_evaluation=True, eval_dir=ev, lpips_eval_net=lp, id_net=idn, save_pivot=True, pivot_dir=pv, **kw)
    # the renderer draws its depth jitter from torch's generator: the evaluation render and the direct one below start from the same seed
    evaluate = coach.evaluate

    def seeded(*a, **k):
        torch.manual_seed(123)
        return evaluate(*a, **k)
    coach.evaluate = seeded
    r1 = coach.invert('a', target, cam)
    assert os.listdir(ev) == ['ametrics.txt'] and sorted(os.listdir(pv)) == ['a_cam.npy', 'a_ws.npy']
    # the generator is still the tuned one: the same metrics computed directly
    torch.manual_seed(123)
    with torch.no_grad():
        img = G.synthesis(r1.w_pivot[:, :14], r1.cam[:, :25], noise_mode='const', force_fp32=True)['image']
    m = reconstruction_metrics(img, target, lp, idn)
    text = open(os.path.join(ev, 'ametrics.txt')).read()
    assert text == format_metrics_txt(r1.metrics)
    # MSE and the MS-SSIM kernels are deterministic: the same bits.  The LPIPS and ArcFace convolutions may accumulate split-K partial sums
    # with atomics in the normal build (the deterministic build exists for bit-exact runs): the same value to fp32 summation-order noise.
    assert text.splitlines()[0] == format_metrics_txt(m).splitlines()[0] and text.splitlines()[2] == format_metrics_txt(m).splitlines()[2]
    for k in ('lpips', 'identity'):
        assert abs(r1.metrics[k] - m[k]) <= 1e-5 * max(1.0, abs(m[k])), (k, r1.metrics[k], m[k])
    assert 0 < m['msssim'] <= 1 and m['mse'] > 0 and np.isfinite(m['identity'])
    assert np.array_equal(np.load(os.path.join(pv, 'a_ws.npy')), r1.w_pivot.cpu().numpy())
    assert np.array_equal(np.load(os.path.join(pv, 'a_cam.npy')), r1.cam.cpu().numpy())
    # run(): the metrics enter the reduced stats only with evaluation on
    G.load_state_dict(pristine)
    _, stats = coach.run([('b', target, cam)])
    assert abs(stats['eval_msssim'] - stats['mean_eval_msssim']) < 1e-12 and 0 < stats['eval_msssim'] <= 1
    G.load_state_dict(pristine)
    _, stats0 = InversionCoach(G, **kw).run([('b', target, cam)])
    assert not any(k.startswith(('eval_', 'mean_eval_')) for k in stats0)
