"""graphed.StepGraph under the two loops that use it (inversion.LatentProjector, inversion.PivotalTuner), on the 64^2 generator of
test_gpu_loops._setup: a step graph owns what its captured launches point to, and a refused capture leaves an eager loop on the current
stream.  The twins are the per-launch loops (the generator's own replay off, as inside a captured step), run once and shared."""
import gc
import warnings
import weakref

import pytest
import torch

from oracle import eg3d_oracle as O
from test_gpu_loops import DEV, _setup  # noqa: E402

pytestmark = pytest.mark.gpu
STEPS = 11                   # 2 warm-up calls, the capturing (or refused) call, 8 more
_SHARED = {}


def _projector(use_graph):
    """(projector, step(i)) with the latent noise and the renderer's uniforms pinned."""
    from inv3d_amd.inversion import LatentProjector
    if 'setup' not in _SHARED:
        _SHARED['setup'] = _setup()
    cfg, P, G, cam, u1, u2, target, init_noise = _SHARED['setup']
    G.graph_eager = False
    pr = LatentProjector(G, target.to(DEV), num_steps=30, cam=cam.to(DEV), init_noise=init_noise, start_w=O.synth_ws(cfg, 1, seed=1)[:, :1],
                         use_graph=use_graph, synth_kwargs=dict(render_uniforms=(u1.to(DEV), u2.to(DEV))))

    def step(i):
        out = pr.step(w_noise=O._randn('wn', i, (1, 1, cfg.w_dim)))
        return (pr.w_opt.detach().clone(), out['image'].clone(), float(out['dist']), [b.detach().clone() for b in pr._all_bufs])
    return pr, step


def _projector_close(got, want):
    """The tolerances of test_latent_projection_graph_replay_matches_eager."""
    assert float((got[0] - want[0]).abs().max()) < 1e-5
    assert abs(got[2] - want[2]) <= 1e-4 * max(1.0, abs(want[2]))
    assert float((got[1] - want[1]).abs().max()) < 1e-4
    for a, b in zip(got[3], want[3]):
        assert float((a - b).abs().max()) < 1e-4


def _tuner(use_graph):
    """(tuner, step(i)) as in test_pivotal_tuning_step_replayed_from_a_hip_graph: a fresh generator, a target it rendered itself."""
    from inv3d_amd import synthetic as S
    from inv3d_amd.inversion import PivotalTuner
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device=DEV)
    S.load_synthetic_weights(G, 0)
    G.graph_eager = False
    cam = O.synth_cameras(1, seed=2).float().to(DEV)
    u1, u2 = O.make_uniforms(cfg, 1, seed=4)
    kw = dict(noise_mode='const', render_uniforms=(u1.float().to(DEV), u2.float().to(DEV)))
    with torch.no_grad():
        target = G.synthesis(O.synth_ws(cfg, 1, seed=3).float().to(DEV), cam, **kw)['image'].clamp(-1, 1)
    t = PivotalTuner(G, target, O.synth_ws(cfg, 1, seed=5).float().to(DEV), cam, synth_kwargs=kw, lpips_threshold=0.0, use_graph=use_graph)

    def step(i):
        res = t.step()
        return float(res['loss']), res['image'].clone()
    return t, step


def _tuner_close(got, want):
    """The tolerances of test_pivotal_tuning_step_replayed_from_a_hip_graph."""
    assert abs(got[0] - want[0]) <= 2e-3 * abs(want[0])
    assert float((got[1] - want[1]).abs().max()) <= 2e-2 * float(want[1].abs().max())


LOOPS = {'LatentProjector': (_projector, _projector_close), 'PivotalTuner': (_tuner, _tuner_close)}


def _twin(name):
    """The eager loop's state after each of STEPS steps."""
    if name not in _SHARED:
        _, step = LOOPS[name][0](False)
        _SHARED[name] = [step(i) for i in range(STEPS)]
    return _SHARED[name]


@pytest.mark.parametrize('name', list(LOOPS))
def test_step_graph_owns_the_operands_of_its_captured_launches(name, monkeypatch):
    """Every derived tensor that hipops.memo / fused.WeightCache hand to a launch of the captured step is kept by the step graph (`refs`):
    emptying the memo table, as `memo` does by itself past 512 entries, frees none of them, and the replays after it follow the eager twin."""
    from inv3d_amd import hipops as H
    make, close = LOOPS[name]
    want = _twin(name)[6]                 # (first: the projector's twin optimises the shared generator's noise buffers)
    loop, step = make(True)
    sg = loop._step_graph
    assert sg.warmup == 2
    for i in range(sg.warmup):
        step(i)
    assert sg.graph is None
    handed, keep = [], H.keep_for_capture
    with monkeypatch.context() as m:
        m.setattr(H, 'keep_for_capture', lambda *objs: (handed.extend(o for o in objs if o is not None), keep(*objs))[1])
        step(sg.warmup)
    assert loop._graph is sg.graph is not None and loop.graph_capture_error is None
    assert handed
    held = {id(o) for o in sg.refs}
    assert all(id(o) in held for o in handed)
    alive = [weakref.ref(t) for o in handed for t in (o if isinstance(o, (tuple, list)) else (o,)) if torch.is_tensor(t)]
    assert alive
    del handed, held
    step(sg.warmup + 1)
    H._MEMO.clear()
    gc.collect()
    assert all(r() is not None for r in alive)
    for i in (4, 5, 6):
        got = step(i)
    close(got, want)


@pytest.mark.parametrize('name', list(LOOPS))
def test_a_refused_capture_leaves_an_eager_loop_on_the_current_stream(name, monkeypatch):
    """`graphed.capture` raises before it touches the runtime (a host exception: nothing is captured): one warning, the error kept, no graph,
    the trajectory of the eager twin, and no stream constructed from the failing step on."""
    from inv3d_amd import graphed
    make, close = LOOPS[name]
    twin = _twin(name)
    err = RuntimeError('refused')

    def refuse(fn, *, arena=None, pool=None):
        raise err
    monkeypatch.setattr(graphed, 'capture', refuse)
    made = []

    class CountingStream(torch.cuda.Stream):
        def __new__(cls, *args, **kwargs):
            if 'stream_id' not in kwargs and 'stream_ptr' not in kwargs:       # (current_stream() wraps an existing one)
                made.append(kwargs.get('device', args[:1]))
            return super().__new__(cls, *args, **kwargs)
    monkeypatch.setattr(torch.cuda, 'Stream', CountingStream)
    loop, step = make(True)
    warmup = loop._graph_warmup
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for i in range(warmup):
            close(step(i), twin[i])
        assert len(made) == warmup
        close(step(warmup), twin[warmup])                     # the refused call: the step ran eagerly all the same
        assert loop.graph_capture_error is err and loop._graph is None
        for i in range(warmup + 1, warmup + 9):
            close(step(i), twin[i])
        assert loop.graph_capture_error is err and loop._graph is None
    assert len(made) == warmup
    said = [str(w.message) for w in caught if 'capture failed' in str(w.message)]
    assert said == [f'{name}: HIP graph capture failed (refused); continuing with eager launches']
