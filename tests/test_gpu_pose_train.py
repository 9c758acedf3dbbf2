"""GPU checks of the pose-estimator training path: hipops.batch_norm_train (csrc/batchnorm.hip) against a float64 restatement with torch's
own fp32 composite as the yardstick, TrainablePoseNet against the reference fixture (tests/golden/pose_train.npz), the trainer against the
same loop in plain torch ops, and the rendered stream."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import pose_net_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
from bn_digest import inputs as digest_inputs, run as digest_run  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CL = torch.channels_last
EPS, MOM = 1e-5, 0.1


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert torch.isfinite(a).all()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def _bn_case(shape, seed, offset=0.4, scale=1.7):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * scale + offset).float()
    res, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return [t.to(DEV).contiguous(memory_format=CL) if t.dim() == 4 else t.to(DEV) for t in (x, res, dy, gamma, beta, rm, rv)]


def _restated(x, res, dy, gamma, beta, rm, rv, act, dt):
    """The op from elementary torch ops in dtype dt (float64: the reference result; float32 is not used -- the fp32 yardstick is F.batch_norm)."""
    x, dy, gamma, beta = (t.detach().to(dt).requires_grad_(t is not dy) for t in (x, dy, gamma, beta))
    res = res.detach().to(dt).requires_grad_(True) if res is not None else None
    m = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean((0, 2, 3))
    var = (x - mean.view(1, -1, 1, 1)).square().mean((0, 2, 3))
    invstd = 1 / torch.sqrt(var + EPS)
    pre = (x - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    if res is not None:
        pre = pre + res
    y = torch.relu(pre) if act == 'relu' else pre
    y.backward(dy)
    out = dict(y=y, mean=mean, invstd=invstd, rm=(1 - MOM) * rm.to(dt) + MOM * mean, rv=(1 - MOM) * rv.to(dt) + MOM * var * m / (m - 1), dx=x.grad, dg=gamma.grad, db=beta.grad)
    if res is not None:
        out['dres'] = res.grad
    return {k: v.detach() for k, v in out.items()}, pre.detach()


def _composite32(x, res, dy, gamma, beta, rm, rv, act):
    """torch's own fp32 training-mode batch norm (+ add + relu) on the same channels-last tensors."""
    x, gamma, beta = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (x, gamma, beta))
    res = res.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) if res is not None else None
    rm, rv = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS)
    if res is not None:
        y = y + res
    y = torch.relu(y) if act == 'relu' else y
    y.backward(dy)
    with torch.no_grad():
        mean = x.mean((0, 2, 3))
        invstd = torch.rsqrt(x.var((0, 2, 3), unbiased=False) + EPS)
    out = dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, dx=x.grad, dg=gamma.grad, db=beta.grad)
    if res is not None:
        out['dres'] = res.grad
    return {k: v.detach() for k, v in out.items()}


def _hip(x, res, dy, gamma, beta, rm, rv, act):
    from inv3d_amd import hipops as H
    x, gamma, beta = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (x, gamma, beta))
    res = res.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) if res is not None else None
    rm, rv, nbt = rm.clone(), rv.clone(), torch.full((), 6, dtype=torch.int64, device=DEV)
    y, save = H.batch_norm_train(x, gamma, beta, rm, rv, nbt, MOM, EPS, residual=res, act=act, return_stats=True)
    y.backward(dy)
    assert int(nbt) == 7
    assert H.is_cl(y) and H.is_cl(x.grad)
    out = dict(y=y, mean=save[0], invstd=save[1], rm=rm, rv=rv, dx=x.grad, dg=gamma.grad, db=beta.grad)
    if res is not None:
        out['dres'] = res.grad
    return {k: v.detach() for k, v in out.items()}


# the estimator's layer shapes at batch 4 and 256^2 input, two shapes whose row count is no multiple of any tile, and the cancellation case
BN_CASES = [
    ('stem', (4, 64, 128, 128), 'relu', False, {}),
    ('layer1', (4, 64, 64, 64), 'relu', True, {}),
    ('layer1-lin', (4, 64, 64, 64), 'linear', False, {}),
    ('layer2', (4, 128, 32, 32), 'relu', True, {}),
    ('layer2-down', (4, 128, 32, 32), 'linear', False, {}),
    ('layer3', (4, 256, 16, 16), 'relu', True, {}),
    ('layer3-lin-res', (4, 256, 16, 16), 'linear', True, {}),
    ('layer4', (4, 512, 8, 8), 'relu', True, {}),
    ('layer4-relu', (4, 512, 8, 8), 'relu', False, {}),
    ('odd-64', (3, 64, 7, 9), 'relu', True, {}),
    ('odd-512', (2, 512, 5, 3), 'linear', False, {}),
    ('odd-12', (5, 12, 3, 7), 'relu', False, {}),
    ('cancellation', (4, 64, 32, 32), 'relu', True, dict(offset=1000.0, scale=1.0)),
    ('cancellation-lin', (4, 128, 16, 16), 'linear', False, dict(offset=-1000.0, scale=1.0)),
]


@pytest.mark.parametrize('name,shape,act,with_res,kw', BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batch_norm_train_parity(name, shape, act, with_res, kw):
    """Every output of forward and backward against float64; the bound is 2 x the error of torch's fp32 F.batch_norm(training=True)
    composite on the same device and inputs against the same float64 result (both are summation-order rounding noise).  Under ReLU the
    elements whose float64 pre-activation lies within the composite's own output error of zero are left out (their mask may flip), and
    their share must stay below 0.1 %; that band is capped at 64 fp32 ulps of the largest pre-activation (the rounding error an fp32
    evaluation of gamma * xhat + beta + residual can have), which only narrows the exclusion where the composite itself is far off."""
    x, res, dy, gamma, beta, rm, rv = _bn_case(shape, seed=len(name) * 131 + shape[1], **kw)
    res = res if with_res else None
    ref, pre = _restated(x, res, dy, gamma, beta, rm, rv, act, torch.float64)
    comp = _composite32(x, res, dy, gamma, beta, rm, rv, act)
    hip = _hip(x, res, dy, gamma, beta, rm, rv, act)
    keep = None
    if act == 'relu':
        band = min(float((comp['y'].double() - ref['y']).abs().max()), 64 * 2.0 ** -24 * float(pre.abs().max()))
        keep = pre.abs() > band
        excluded = 1.0 - float(keep.double().mean())
        print(f'{name}: relu band {band:.3e}, excluded share {excluded:.3e}')
        assert excluded < 1e-3
    centred = None
    if kw:          # cancellation: the composite itself is off by 0.3 there, so 2 x its error guards nothing.  y, the gradients, 1/sigma and the
        # variance do not change when x is shifted, so they must also meet the bound of the SAME case with the offset taken out
        x0 = (x.double() - kw['offset']).float().contiguous(memory_format=CL)
        ref0, _ = _restated(x0, res, dy, gamma, beta, rm, rv, act, torch.float64)
        comp0 = _composite32(x0, res, dy, gamma, beta, rm, rv, act)
        centred = {k: float((comp0[k].double() - ref0[k]).abs().max()) for k in ('y', 'dx', 'dres', 'dg', 'db', 'invstd') if k in ref0}
    for k in ref:
        eh, ec = (hip[k].double() - ref[k]).abs(), (comp[k].double() - ref[k]).abs()
        if keep is not None and k in ('y', 'dx', 'dres'):
            eh, ec = eh[keep], ec[keep]
        eh, ec = float(eh.max()), float(ec.max())
        print(f'{name}: {k}: hip {eh:.3e} composite {ec:.3e} ratio {eh / max(ec, 1e-300):.3f}' + (f' centred composite {centred[k]:.3e}' if centred and k in centred else ''))
        assert eh <= 2 * ec, (name, k, eh, ec)
        if centred and k in centred:
            assert eh <= 2 * centred[k], (name, k, eh, centred[k])


def test_batch_norm_train_bit_identical_runs_builds_and_graph_replay():
    from inv3d_amd import hipops as H
    args = digest_inputs(DEV)
    first = digest_run(*args)
    assert digest_run(*args) == first
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'bn_digest.py')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out.pop('deterministic_build') is True
    assert out == first
    # captured forward + backward, replayed on new inputs copied into the static ones
    x, res, dy, gamma, beta = args
    c = x.shape[1]
    xs = torch.zeros_like(x).requires_grad_(True)
    rs = res.clone(memory_format=CL).requires_grad_(True)
    gs, bs = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv, nbt = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    with torch.no_grad():
        xs.copy_(x * 0.5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            y = H.batch_norm_train(xs, gs, bs, rm, rv, nbt, MOM, EPS, residual=rs, act='relu')
            torch.autograd.grad(y, (xs, gs, bs, rs), dy)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with H.capture_guard(), torch.cuda.graph(graph):
        y = H.batch_norm_train(xs, gs, bs, rm, rv, nbt, MOM, EPS, residual=rs, act='relu')
        grads = torch.autograd.grad(y, (xs, gs, bs, rs), dy)
    with torch.no_grad():
        xs.copy_(x)
        rm.zero_()
        rv.fill_(1.0)
        nbt.zero_()
    graph.replay()
    torch.cuda.synchronize()
    xe, re_ = x.clone(memory_format=CL).requires_grad_(True), res.clone(memory_format=CL).requires_grad_(True)
    ge, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rme, rve, nbte = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    ye = H.batch_norm_train(xe, ge, be, rme, rve, nbte, MOM, EPS, residual=re_, act='relu')
    eager = torch.autograd.grad(ye, (xe, ge, be, re_), dy)
    assert torch.equal(y, ye) and all(torch.equal(a, b) for a, b in zip(grads, eager))
    assert torch.equal(rm, rme) and torch.equal(rv, rve) and int(nbt) == int(nbte) == 1


def test_batch_norm_argument_validation():
    """The entries refuse bad arguments on the host with an error code, before anything is launched."""
    from inv3d_amd import _lib as L
    from inv3d_amd import hipops as H
    lib = L.lib()
    Cn, M = 64, 96
    x = torch.randn(M * Cn + 4, device=DEV)
    y = torch.empty_like(x)
    g, b = torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    stats = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
    n = C.c_int64(0)
    assert lib.eg3d_batchnorm_query_workspace(M, Cn, C.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)

    def params(**kw):
        p = L.BatchNormParams(x=x.data_ptr(), gamma=g.data_ptr(), beta=b.data_ptr(), y=y.data_ptr(), M=M, C=Cn, act=L.ACT_IDS['relu'], eps=EPS, momentum=MOM,
                              stats=stats.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=n.value, dy=x.data_ptr(), dx=y.data_ptr())
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    torch.cuda.synchronize()
    y.fill_(-7.0)
    torch.cuda.synchronize()
    bad = [dict(x=None), dict(gamma=None), dict(y=None), dict(stats=None), dict(workspace=None), dict(x=x.data_ptr() + 4), dict(y=y.data_ptr() + 8),
           dict(C=66), dict(C=0), dict(M=1), dict(workspace_bytes=16), dict(momentum=1.5), dict(residual=x.data_ptr() + 4)]
    for kw in bad:
        assert lib.eg3d_batchnorm_forward(C.byref(params(**kw)), L.stream_ptr()) == -1, kw
    assert lib.eg3d_batchnorm_forward(C.byref(params(act=L.ACT_IDS['tanh'])), L.stream_ptr()) == -2
    assert lib.eg3d_batchnorm_forward(None, L.stream_ptr()) == -1
    for kw in [dict(x=None), dict(dy=None), dict(y=None), dict(stats=None), dict(dy=x.data_ptr() + 4), dict(dx=y.data_ptr() + 4), dict(C=6), dict(M=0),
               dict(workspace_bytes=n.value - 8)]:
        assert lib.eg3d_batchnorm_backward(C.byref(params(**kw)), L.stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    assert float((y + 7.0).abs().max()) == 0.0          # nothing was launched
    assert lib.eg3d_batchnorm_forward(C.byref(params()), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(y[:M * Cn].min()) >= 0.0
    xc = torch.randn(2, 64, 4, 4, device=DEV)          # the host op refuses a tensor that is not channels-last rather than copying it silently
    with pytest.raises(L.Eg3dHipError):
        H.batch_norm_train(xc, g, b)


# ---------------------------------------------------------------------------------------------------------------- the whole network
def test_trainable_net_train_mode_matches_reference(golden):
    """TrainablePoseNet.train() on the GPU against the reference's resnet34(4).train() step (fixture).  Tolerances of test_gpu_posenet.py:
    output 1e-4 relative; parameter gradients 2e-3 relative for >= 95 % of the tensors, none off by more than 0.2 (the allowance is for
    ReLU / max-pool routing flips; the fixture's maker shows the reference's own fp32 needs none against its fp64 on this input); running
    statistics 1e-5 relative."""
    from inv3d_amd.pose_net import resnet34_pose
    from inv3d_amd.pose_train import pose_training_loss, resnet34_pose_trainable
    d = golden('pose_train')
    sd = PO.synth_state(seed=int(d['seed']), output_dims=4)
    with pytest.raises(NotImplementedError):
        resnet34_pose(4).train()
    net = resnet34_pose_trainable(4)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).requires_grad_(True)
    assert net.train() is net and net.training
    img = torch.from_numpy(d['net_img']).to(DEV)
    y = net(img)
    print('output rel err', _rel(y, d['net_y']))
    assert _rel(y, d['net_y']) < 1e-4
    loss, _ = pose_training_loss(y, torch.from_numpy(d['net_ext']).to(DEV), '4', 2.7)
    assert abs(float(loss) - float(d['net_loss'])) <= 1e-4 * abs(float(d['net_loss']))
    loss.backward()
    new = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for k in d.files:
        if k.startswith('net_stat.'):
            print(k, _rel(new[k[9:]], d[k]))
            assert _rel(new[k[9:]], d[k]) < 1e-5, k
    assert all(int(v) == 1 for k, v in new.items() if k.endswith('num_batches_tracked'))
    params = dict(net.named_parameters())
    worst = {}
    for k in d.files:
        if k.startswith('net_g.'):
            worst[k[6:]] = _rel(params[k[6:]].grad, d[k])
        elif k.startswith('net_gs.'):
            worst[k[7:]] = _rel(params[k[7:]].grad.flatten()[::97], d[k])
    print('gradient rel errs', {k: f'{v:.2e}' for k, v in worst.items()})
    assert len(worst) >= 10
    bad = [k for k, e in worst.items() if e > 2e-3]
    assert len(bad) <= 0.05 * len(worst), (bad[:5], [worst[k] for k in bad[:5]])
    assert max(worst.values()) < 0.2, max(worst.items(), key=lambda kv: kv[1])
    # after the train-mode step, eval on the GPU (the folded path, on the updated statistics) equals the CPU oracle on the updated state dict
    net.eval()
    assert not net.training
    with torch.no_grad():
        ye = net(img)
        assert _rel(ye, PO.forward(new, img.cpu())) < 1e-4
        plain = resnet34_pose(4)
        plain.load_state_dict(new, strict=True)
        assert _rel(plain.to(DEV)(img), ye) < 1e-5          # eval mode IS the existing path (whose split convs sum with float atomics: not bit for bit)


# ---------------------------------------------------------------------------------------------------------------- trainer
def _small_generator():
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    return G


def _plain_torch_steps(sd, batches, dt, lr=1e-4):
    """The trainer's step in plain torch ops on the CPU (TrainablePoseNet's torch path: F.conv2d, F.batch_norm(training=True), torch.optim.Adam)."""
    from inv3d_amd.pose_train import PoseEstimatorTrainer, resnet34_pose_trainable
    net = resnet34_pose_trainable(4)
    net.load_state_dict(sd, strict=True)
    net = net.to(dt)
    tr = PoseEstimatorTrainer(None, net, lr=lr, camera_type='4')
    losses = [float(tr.step((img.cpu().to(dt), ext.cpu().to(dt)))['loss']) for img, ext in batches]
    return losses, {k: v.detach().double() for k, v in net.state_dict().items()}


def test_trainer_trajectory_against_plain_torch():
    """Five PoseEstimatorTrainer.step() calls on the small synthetic generator against five steps of the same loop in plain torch ops, from
    the same initial state (He initialisation, seed 0) and the same recorded batches (batch 8, 64^2).  Compared against the plain loop in
    fp64: every step's loss (largest difference over the steps) and the five-step change of fc3.weight, fc3.bias, bn1.weight, bn1.bias
    (L2 norm of the difference, relative to the fp64 change).

    Neither side is one number.  Adam's first update is lr * sign(g), so a rounding-level difference in a gradient near zero becomes a
    full 1e-4 step: the fp32 loop agrees with fp64 to 3e-6 in the loss at step 1 and to 2e-3 at step 2, and from there every evaluation
    order is another draw.  The HIP training path is not reproducible from run to run in the normal build (its split convolutions sum with
    float atomics; six runs of these five steps gave six different states) and is bit for bit reproducible in the deterministic build.
    Measured, yardstick side: the plain fp32 loop on 1 / 3 / 8 CPU threads drifts 2.1e-2 / 4.2e-3 / 4.2e-3 in the loss, 1.8e-3 / 7.2e-4 /
    7.2e-4 in fc3.bias, 0.092 / 0.059 / 0.059 in bn1.weight.  HIP side, six runs: loss 2.0e-2 .. 3.8e-2, fc3.weight 2.5e-2 .. 4.9e-2
    (yardstick 2.2e-2), fc3.bias 1.9e-3 .. 3.7e-3, bn1.weight 0.150 .. 0.183, bn1.bias 0.160 .. 0.194 (yardstick 0.114); deterministic
    build: 1.4e-2, 4.2e-2, 6.8e-4, 0.076, 0.114.
    So the yardstick is the largest drift of the plain fp32 loop over two evaluation orders (1 thread, default threads), the HIP figure
    is the median over five runs from the same state (all five printed), and the allowance is the issue's 3 x: the HIP convs form
    products from split 16-bit operands and sum in another order -- a different draw of the same noise."""
    from inv3d_amd.pose_train import PoseEstimatorTrainer, PseudoPoseStream, resnet34_pose_trainable
    import statistics
    G = _small_generator()
    batches = PseudoPoseStream(G, 8, seed=21, size=64).take(5)
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in resnet34_pose_trainable(4).state_dict().items()}
    keys = ('fc3.weight', 'fc3.bias', 'bn1.weight', 'bn1.bias')
    l64, p64 = _plain_torch_steps(sd, batches, torch.float64)

    def drifts(losses, params):
        d = dict(loss=max(abs(a - b) for a, b in zip(losses, l64)))
        for k in keys:
            d[k] = float((params[k] - p64[k]).norm() / (p64[k] - sd[k].double()).norm())
        return d
    threads = torch.get_num_threads()
    cpu = []
    try:
        for t in (1, threads):
            torch.set_num_threads(t)
            cpu.append(drifts(*_plain_torch_steps(sd, batches, torch.float32)))
    finally:
        torch.set_num_threads(threads)
    hip = []
    for _ in range(5):
        net = resnet34_pose_trainable(4)
        net.load_state_dict(sd, strict=True)
        tr = PoseEstimatorTrainer(G, net.to(DEV), batch_size=8, lr=1e-4, camera_type='4', stream_kwargs=dict(size=64))
        lh = [float(tr.step(b)['loss']) for b in batches]
        assert all(math.isfinite(v) for v in lh)
        hip.append(drifts(lh, {k: v.detach().cpu().double() for k, v in net.state_dict().items()}))
    for k in ('loss',) + keys:
        yard, runs = max(c[k] for c in cpu), [h[k] for h in hip]
        print(f'{k}: plain fp32 {[f"{c[k]:.3e}" for c in cpu]}; hip {[f"{v:.3e}" for v in runs]}; median / yardstick {statistics.median(runs) / yard:.2f}')
    for k in ('loss',) + keys:
        assert statistics.median(h[k] for h in hip) <= 3 * max(c[k] for c in cpu), k


class _FixedBatch:
    def __init__(self, batch):
        self.batch = batch

    def next(self):
        return self.batch


def test_trainer_overfits_a_fixed_batch(tmp_path):
    """It learns.  The issue's first form -- fit() on the rendered stream, configuration chosen on the CPU with the plain-torch loop in
    about a minute -- was not reached: a plain-torch step at batch 8 and 64^2 takes 0.37 s on the CPU, so a minute is some 150 steps
    before any rendering, and no stream configuration was tried.  This is the issue's fallback: fit() on one fixed batch rendered by the
    stream (8 images, 64^2, He initialisation seed 0, lr 1e-4, use_roll=False, camera type '4'), validated on that batch every 10 steps,
    100 steps.  Baseline: the constant predictor that always outputs the frontal pose, computed from the batch's poses (0.167 rad).

    What is asserted follows the measured spread.  The error at a given step is not stable: the objective's regulariser
    1e-10 / (|R00| - 1)^2 has its pole at the frontal pose, so a tight fit to poses of small yaw meets large gradients, and in the normal
    build the run is not reproducible (float atomics).  Four runs, validation every 10 steps: [1.20 .29 .25 .17 .09 .06 .04 .05 .04 .04],
    [1.17 .26 .17 .10 .27 .40 .36 .27 .19 .12], [1.17 .26 .12 .07 .07 .44 .31 .22 .08 .07], [1.18 .25 .11 .05 .12 .14 .06 .06 .06 .05];
    the deterministic build repeats [1.16 .25 .10 .06 .06 .07 .06 .17 .11 .05] exactly.  No step count up to 100 keeps the last state below
    the baseline in every run, while the checkpoint fit() keeps (model_best.pt, by validation score, the reference's rule) ends at
    0.04 .. 0.07 in all of them, and the last state never exceeds 0.44 against 2.08 at step 0.  Asserted: the kept checkpoint is below the
    baseline with a factor 1.5 to spare (0.111), and the last state is below half the step-0 error."""
    from inv3d_amd.pose_train import PoseEstimatorTrainer, PseudoPoseStream, geodesic_distance, poses_from_angles, resnet34_pose_trainable
    G = _small_generator()
    torch.manual_seed(0)
    net = resnet34_pose_trainable(4).to(DEV)
    img, ext = PseudoPoseStream(G, 8, seed=33, size=64, use_roll=False).next()
    front = poses_from_angles(torch.tensor([math.pi / 2]), torch.tensor([math.pi / 2])).to(DEV)
    baseline = float(geodesic_distance(front[:, :3, :3].expand(8, 3, 3), ext[:, :3, :3]).mean())
    tr = PoseEstimatorTrainer(G, net, batch_size=8, lr=1e-4, camera_type='4', stream=_FixedBatch((img, ext)), validation=[(img, ext)])
    log = tr.fit(100, validate_every=10, out_dir=str(tmp_path))
    e0, e_end = log[0]['geodesic'], log[-1]['geodesic']
    net.load_state_dict(torch.load(tmp_path / 'model_best.pt', map_location='cpu'), strict=True)
    e_best = tr.validate()['geodesic']
    print(f'constant predictor {baseline:.4f}; validations {[round(r["geodesic"], 3) for r in log]}; kept checkpoint {e_best:.4f}')
    assert math.isfinite(e_end) and e_best < baseline / 1.5 and e_best < e0
    assert e_end < 0.5 * e0


def test_fit_keeps_the_best_checkpoint(tmp_path):
    from inv3d_amd.pose_net import resnet34_pose
    from inv3d_amd.pose_train import PoseEstimatorTrainer, resnet34_pose_trainable
    G = _small_generator()
    torch.manual_seed(0)
    net = resnet34_pose_trainable(4).to(DEV)
    tr = PoseEstimatorTrainer(G, net, batch_size=4, lr=1e-4, camera_type='4', val_batches=1, stream_kwargs=dict(size=64))
    log = tr.fit(4, validate_every=2, out_dir=str(tmp_path))
    assert [r['step'] for r in log] == [0, 2, 4] and all(math.isfinite(r['geodesic']) and math.isfinite(r['translation_l1']) for r in log)
    assert log[0]['best'] and os.path.exists(tmp_path / 'model_best.pt') and os.path.exists(tmp_path / 'model_last.pt')
    # model_best.pt holds the state of the best-scoring validation: reloaded, it validates to that score (eval sums with float atomics:
    # 1e-4 relative), and it is the last state exactly when the last validation was the best one
    best = torch.load(tmp_path / 'model_best.pt', map_location='cpu')
    last = torch.load(tmp_path / 'model_last.pt', map_location='cpu')
    plain = resnet34_pose(4)
    plain.load_state_dict(best, strict=True)
    scores = [r['geodesic'] + r['translation_l1'] for r in log]
    i_best = max(i for i, r in enumerate(log) if r['best'])
    assert scores[i_best] == min(scores)
    same_as_last = all(torch.equal(best[k], last[k]) for k in best)
    assert same_as_last == (i_best == len(log) - 1)
    net.load_state_dict(best, strict=True)
    v = tr.validate()
    assert abs(v['geodesic'] + v['translation_l1'] - scores[i_best]) <= 1e-4 * scores[i_best], (v, scores)


def test_stream_is_seeded_and_in_range():
    from inv3d_amd.pose_train import PseudoPoseStream, sample_pseudo_poses
    G = _small_generator()
    a, b = PseudoPoseStream(G, 2, seed=5), PseudoPoseStream(G, 2, seed=5)
    other = PseudoPoseStream(G, 2, seed=6)
    for _ in range(2):
        (ia, ea), (ib, eb) = a.next(), b.next()
        assert torch.equal(ia, ib) and torch.equal(ea, eb)
    io, eo = other.next()
    assert not torch.equal(eo, ea)
    assert ia.shape == (2, 3, 256, 256) and ea.shape == (2, 4, 4) and ia.dtype == torch.float32
    assert float(ia.min()) >= 0.0 and float(ia.max()) <= 255.0 and float(ia.std()) > 0.0
    # the extrinsics are those of sample_pseudo_poses on the stream's generator: z first, then the poses
    g = torch.Generator(device=DEV).manual_seed(5)
    torch.randn((2, G.z_dim), generator=g, device=DEV)
    want = sample_pseudo_poses(2, generator=g, device=DEV, radius=float(G.rendering_kwargs.get('avg_camera_radius', 2.7)))
    first = PseudoPoseStream(G, 2, seed=5).next()[1]
    assert torch.equal(first, want)
    q = PseudoPoseStream(G, 2, seed=5, quantize=True, size=64).next()[0]
    assert q.shape == (2, 3, 64, 64)
