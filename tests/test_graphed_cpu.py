"""Host logic of inv3d_amd/graphed.py without a device: `StepGraph` (warm-up -> capture -> replay, or -> eager after a refused capture) with
`graphed.capture` and the stream / synchronise helpers replaced by recorders, and `capture`'s bookkeeping of `hipops.CAPTURE_REFS` with the
runtime's capture replaced by null contexts."""
import contextlib
import warnings

import pytest
import torch

from inv3d_amd import graphed as GR
from inv3d_amd import hipops as H


class _FakeGraph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append('replay')


@pytest.fixture
def machine(monkeypatch):
    """(log, make): `make(warmup, refuse=None, arena=None)` builds a StepGraph whose step function, before_capture, capture, side-stream
    and synchronise calls all append their name to `log`."""
    log = []
    monkeypatch.setattr(GR, '_synchronize', lambda: log.append('sync'))

    def on_side_stream(fn, device):
        log.append('side')
        return fn()
    monkeypatch.setattr(GR, '_on_side_stream', on_side_stream)

    def make(warmup, refuse=None, arena=None):
        refs = [object(), object()]

        def fake_capture(fn, *, arena=None, pool=None):
            log.append(('capture', arena))
            if refuse is not None:
                raise refuse
            return _FakeGraph(log), fn(), refs
        monkeypatch.setattr(GR, 'capture', fake_capture)
        count = [0]

        def step():
            log.append('step')
            count[0] += 1
            return count[0]
        sg = GR.StepGraph('Loop', step, lambda: log.append('before'), arena=arena, warmup=warmup, device='cpu')
        return sg, refs
    return log, make


@pytest.mark.parametrize('warmup', [0, 1, 3])
def test_step_graph_warms_up_captures_once_then_only_replays(machine, warmup):
    log, make = machine
    sg, refs = make(warmup)
    for i in range(warmup):
        assert sg() == i + 1 and sg.graph is None
    assert log == ['side', 'step'] * warmup                       # exactly `warmup` eager calls, each on the side stream
    del log[:]
    assert sg() == warmup + 1
    assert log == ['sync', 'before', ('capture', None), 'step', 'replay']      # before_capture once, in front of the one capture; one replay
    assert sg.graph is not None and sg.error is None and sg.refs is refs
    del log[:]
    for _ in range(4):
        assert sg() == warmup + 1                                 # the capture's static result; the step function is not called again
    assert log == ['replay'] * 4


def test_step_graph_after_a_refused_capture_runs_the_step_directly(machine):
    log, make = machine
    err = RuntimeError('refused')
    sg, _ = make(2, refuse=err)
    sg(), sg()
    del log[:]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        assert sg() == 3
        assert log == ['sync', 'before', ('capture', None), 'sync', 'before', 'step']     # before_capture once more in front of the eager retry
        assert sg.error is err and sg.graph is None and sg.refs is None
        del log[:]
        for i in range(5):
            assert sg() == 4 + i
        assert log == ['step'] * 5                                # no side stream, no synchronise, no further capture
    assert [str(w.message) for w in caught] == ['Loop: HIP graph capture failed (refused); continuing with eager launches']


def test_step_graph_lets_other_exceptions_through(machine):
    log, make = machine
    sg, _ = make(0, refuse=ValueError('not the runtime'))
    with pytest.raises(ValueError):
        sg()
    assert sg.error is None and sg.graph is None


def test_step_graph_routes_its_arena_in_eager_runs_and_hands_it_to_the_capture(machine):
    log, make = machine
    arena = H.ZeroArena('cpu')
    sg, _ = make(1, arena=arena)
    seen = []
    step = sg.fn
    sg.fn = lambda: (seen.append(H.ARENA), step())[1]
    sg()
    assert seen == [arena] and H.ARENA is None
    sg()
    assert ('capture', arena) in log
    sg2, _ = make(0, refuse=RuntimeError('refused'), arena=arena)
    step2 = sg2.fn
    sg2.fn = lambda: (seen.append(H.ARENA), step2())[1]
    with pytest.warns(UserWarning):
        sg2()
    sg2()
    assert seen[-2:] == [arena, arena] and H.ARENA is None


@pytest.fixture
def null_runtime(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda: object())
    monkeypatch.setattr(torch.cuda, 'graph', lambda g, pool=None, capture_error_mode=None: contextlib.nullcontext())
    monkeypatch.setattr(H, 'capture_guard', contextlib.nullcontext)


def test_capture_collects_the_kept_operands_and_restores_capture_refs(null_runtime, monkeypatch):
    outer = ['outer']
    monkeypatch.setattr(H, 'CAPTURE_REFS', outer)
    a, b = object(), object()
    arena = H.ZeroArena('cpu')

    def fn():
        assert H.CAPTURE_REFS == [] and H.CAPTURE_REFS is not outer
        assert H.ARENA is arena                                   # routed inside the capture
        H.keep_for_capture(a, None, b)
        return 'result'
    graph, res, refs = GR.capture(fn, arena=arena)
    assert graph is not None and res == 'result'
    assert len(refs) == 2 and refs[0] is a and refs[1] is b
    assert H.CAPTURE_REFS is outer and outer == ['outer'] and H.ARENA is None
    monkeypatch.setattr(H, 'CAPTURE_REFS', None)
    assert GR.capture(lambda: H.ARENA)[1:] == (None, [])           # no arena given: none routed
    assert H.CAPTURE_REFS is None


@pytest.mark.parametrize('prev', [None, ['outer']])
def test_capture_restores_capture_refs_when_the_captured_function_raises(null_runtime, monkeypatch, prev):
    monkeypatch.setattr(H, 'CAPTURE_REFS', prev)

    def fn():
        H.keep_for_capture(object())
        raise RuntimeError('inside')
    with pytest.raises(RuntimeError, match='inside'):
        GR.capture(fn)
    assert H.CAPTURE_REFS is prev and (prev is None or prev == ['outer'])
