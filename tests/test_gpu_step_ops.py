"""The per-step kernels of csrc/noise_ops.hip on their own -- eg3d_noise_regularizer, eg3d_noise_normalize (both forms), eg3d_adam_step and
eg3d_early_stop_flag -- against the float64 restatement and the derived elementwise bounds of tests/support/step_ref.py (checked without a GPU in
tests/test_step_ops_cpu.py).  The loop-level tests compare trajectories at 1e-3 and up; an error here bends a trajectory slowly and stays below that.

  * regulariser: structured maps in which every pyramid level carries at least a hundred tolerances of the value and of |g|max, so a level that is
    dropped, mis-weighted or read at the wrong ancestor shows; every buffer's value on its own and all together; 17 and 34 buffers; no gradient;
    gradient views; null gradient entries through the C ABI; a randn case;
  * normalise: the multi-block form through hipops and the one-block form through the C ABI, mean / std of 0, 1 and 8;
  * Adam: single steps from arbitrary fp32 states at step counts 0, 999 and 9999, leaves around the 4096-element chunk, renormalised maps, banks of
    33 and 65 items, skip, a 5-step trajectory checked step by step from the device's own state;
  * the same file once more in a fresh interpreter under the deterministic build, where it also asserts run-to-run bit identity and det_misses() == 0.
Every case prints its worst err / tol.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'support'))
import step_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _det():
    from inv3d_amd import _lib as L
    return L.DETERMINISTIC


def _tag():
    return ' (deterministic build)' if _det() else ''


def _no_misses():
    """Deterministic build: no addition of the calls so far fell back to a float atomic (asserted by every kernel test itself, so that it
    holds under any selection or order of tests)."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ regulariser
def _reg(xs, scale, **kw):
    from inv3d_amd import hipops
    total, grads = hipops.noise_regularizer(xs, scale=scale, **kw)
    torch.cuda.synchronize()
    return total, grads


def _check_reg(name, cases, scale, launches=1, randn=False):
    """One call over `cases` = [(res, seed)]: value and every gradient under the bound; deterministic build: a second call is bit-identical."""
    if randn:
        xs = [R.randn_case(r, s) for r, s in cases]
        refs = [R.reg_ref(x, scale) for x in xs]
    else:
        xs, refs = zip(*[R.struct_ref(r, s, scale) for r, s in cases])
    dx = [_dev(x) for x in xs]
    total, grads = _reg(dx, scale)
    for a, x in zip(dx, xs):
        assert np.array_equal(_np(a), x), 'the input was modified'
    ok, worst, what = R.compare_reg(float(total), [_np(g) for g in grads], refs, launches)
    print(f'regulariser {name} scale {scale:g}: worst err/tol {worst:.4f} ({what}){_tag()}')
    assert ok, (name, scale, worst, what)
    if _det():
        total2, grads2 = _reg(dx, scale)
        assert torch.equal(total, total2) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), 'two calls differ under the deterministic build'
    _no_misses()
    return dx, refs, total, grads


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('res', R.STRUCT_RES)
def test_regulariser_of_one_structured_map(res, scale):
    """Every size from 1 to 1024 alone (the value of each buffer on its own); 1024^2 is where the pyramid's band exceeds 64 rows."""
    _check_reg(f'{res}^2 alone', [(res, 100)], scale)


@pytest.mark.parametrize('scale', R.SCALES)
def test_regulariser_of_all_sizes_in_one_call(scale):
    _check_reg('1^2 .. 512^2 together', [c for c in R.SINGLES if c[0] <= 512], scale)


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('copies', [1, 2])
def test_regulariser_of_the_models_17_maps(copies, scale):
    """17 buffers in the generator's order; 34 take two launches whose totals add."""
    _check_reg(f'{17 * copies} maps', list(R.BANK17) * copies, scale, launches=copies)


def test_regulariser_of_randn_maps():
    """The regime the loops live in: white noise, where the fine levels dominate."""
    _check_reg('17 randn maps', list(R.BANK17), 1e5, randn=True)
    _check_reg('randn 1024^2', [(1024, 1)], 1.0, randn=True)


def test_regulariser_without_gradient_and_with_gradient_views():
    """want_grad=False gives the same value; grads= views into [N, 1, r, r] tensors (as the batched projector passes them) are filled and nothing
    around them is written."""
    scale = 1e5
    N, cases = R.VIEW_N, list(R.VIEW_CASES)
    xs, refs = zip(*[R.struct_ref(r, s, scale) for r, s in cases])
    maps = [_dev(np.stack([xs[N * i + n] for n in range(N)])[:, None]) for i in range(len(cases) // N)]          # [N, 1, r, r]
    views = [m[n, 0] for m in maps for n in range(N)]
    total0, none = _reg(views, scale, want_grad=False)
    assert none is None
    ok, worst, _ = R.compare_reg(float(total0), None, refs)
    print(f'regulariser without gradient: worst err/tol {worst:.4f}{_tag()}')
    assert ok, worst
    store = [torch.full((N, 2, m.shape[-1], m.shape[-1]), 7.0, device=DEV) for m in maps]          # channel 1 is a sentinel
    total, grads = _reg(views, scale, grads=[g[n, 0] for g in store for n in range(N)])
    ok, worst, what = R.compare_reg(float(total), [_np(g) for g in grads], refs)
    print(f'regulariser into gradient views: worst err/tol {worst:.4f} ({what}){_tag()}')
    assert ok, (worst, what)
    assert all(bool((g[:, 1] == 7.0).all()) for g in store), 'written outside the gradient views'
    if _det():
        assert torch.equal(total, total0)
    _no_misses()


def test_regulariser_c_abi_with_null_gradient_entries():
    """include/eg3d_hip.h: grad may contain nulls.  The non-null gradients are right and the value includes every buffer."""
    from inv3d_amd import _lib as L
    scale = 1.0
    cases = [(r, 100) for r in (4, 16, 64, 128, 512)]
    xs, refs = zip(*[R.struct_ref(r, s, scale) for r, s in cases])
    dx = [_dev(x) for x in xs]
    n = len(dx)
    grads = [None if i % 2 else torch.empty_like(x) for i, x in enumerate(dx)]
    res = (C.c_int32 * n)(*[x.shape[-1] for x in dx])
    ws = torch.empty(int(L.lib().eg3d_noise_reg_workspace_floats(res, n)), dtype=torch.float32, device=DEV)
    reg = torch.full((), 123.0, device=DEV)
    L.check(L.lib().eg3d_noise_regularizer((C.c_void_p * n)(*[x.data_ptr() for x in dx]), (C.c_void_p * n)(*[g.data_ptr() if g is not None else None for g in grads]),
                                           res, n, L.ptr(ws), L.ptr(reg), scale, L.stream_ptr()), 'noise_regularizer')
    torch.cuda.synchronize()
    ok, worst, what = R.compare_reg(float(reg), [None if g is None else _np(g) for g in grads], refs)
    print(f'regulariser C ABI, null gradient entries: worst err/tol {worst:.4f} ({what}){_tag()}')
    assert ok, (worst, what)
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ normalise
def _normalize(xs, form):
    from inv3d_amd import _lib as L, hipops
    if form == 'multi':
        hipops.noise_normalize_(xs)
    else:                      # one block per buffer: null workspace, at most 32 buffers a call
        for lo in range(0, len(xs), 32):
            part = xs[lo:lo + 32]
            n = len(part)
            L.check(L.lib().eg3d_noise_normalize((C.c_void_p * n)(*[x.data_ptr() for x in part]), (C.c_int32 * n)(*[x.shape[-1] for x in part]), n, None,
                                                 L.stream_ptr()), 'noise_normalize')
    torch.cuda.synchronize()


@pytest.mark.parametrize('form', ['multi', 'block'])
def test_normalise_both_forms(form):
    """Sizes 2, 4, 64, 512 at mean / std 0, 1 and 8, and a bank of 34 maps (two launches) with the three ratios in turn."""
    sets = {'sizes': [(r, m, 0) for r in R.NORM_RES for m in R.NORM_MEANS],
            'bank of 34': [(r, R.NORM_MEANS[i % 3], i) for i, r in enumerate(R.MODEL_RES * 2)]}
    for name, cases in sets.items():
        xs = [R.norm_case(*c) for c in cases]
        dx = [_dev(x) for x in xs]
        _normalize(dx, form)
        worst = {m: (0.0, None) for m in R.NORM_MEANS}
        for (res, m, _), x, d in zip(cases, xs, dx):
            r = R.compare(_np(d), R.normalize_ref(x), R.normalize_tol(x, form))[1]
            if r >= worst[m][0]:
                worst[m] = (r, res)
        print(f'normalise {form} {name}: worst err/tol ' + ', '.join(f'{w:.4f} at mean/std {m:g} ({res}^2)' for m, (w, res) in worst.items()) + _tag())
        assert max(w for w, _ in worst.values()) <= 1.0, (form, name, worst)
        if _det():
            again = [_dev(x) for x in xs]
            _normalize(again, form)
            assert all(torch.equal(a, b) for a, b in zip(dx, again)), 'two calls differ under the deterministic build'
    _no_misses()


# ------------------------------------------------------------------------------------------------------------------ Adam
KINDS = ('g', 'g2', 'both')


class _Leaves:
    """An optimiser over leaves [(shape, kind, slices)] with arbitrary fp32 state; kind: which gradients exist ('g', 'g2', 'both', 'none'), slices:
    0 or the number of slices renormalised separately."""

    def __init__(self, leaves, t0, lr, seed=0, lr_tensor=True):
        from inv3d_amd import hipops
        self.leaves = leaves
        self.params, self.extra, self.norm, self.host = [], {}, {}, []
        for i, (shape, kind, slices) in enumerate(leaves):
            n = int(np.prod(shape))
            p, g, g2, m, v = R.adam_state(n, 1000 * seed + i, **(dict(gmag=(1e-3, 1.0), mean=1.0) if slices else {}))
            self.host.append([a.reshape(shape) for a in (p, g, g2, m, v)])
            q = _dev(p.reshape(shape)).requires_grad_(True)
            if kind in ('g', 'both'):
                q.grad = _dev(g.reshape(shape))
            if kind in ('g2', 'both'):
                self.extra[q] = _dev(g2.reshape(shape))
            if slices:
                self.norm[q] = slices
            self.params.append(q)
        self.opt = hipops.HipAdam(self.params, lr=torch.tensor(float(lr), device=DEV) if lr_tensor else float(lr))
        self.opt.step_t.fill_(float(t0))
        for q, h in zip(self.params, self.host):
            self.opt.state[q]['exp_avg'].copy_(_dev(h[3]))
            self.opt.state[q]['exp_avg_sq'].copy_(_dev(h[4]))

    def state(self):
        return [(_np(q), _np(self.opt.state[q]['exp_avg']), _np(self.opt.state[q]['exp_avg_sq'])) for q in self.params]

    def step(self, skip=None):
        """One step(); returns the workspaces the optimiser handed to the kernel."""
        from inv3d_amd import hipops
        taken, orig = [], hipops.zeros

        def spy(shape, device):
            t = orig(shape, device)
            taken.append(t)
            return t
        hipops.zeros = spy
        try:
            self.opt.step(extra_grads=self.extra, normalize=self.norm, skip=skip)
        finally:
            hipops.zeros = orig
        torch.cuda.synchronize()
        return taken

    def check(self, name, before, t, lr):
        """Every leaf against adam_ref of the state `before`, with step count t."""
        worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
        for (shape, kind, slices), h, (p0, m0, v0), (p1, m1, v1) in zip(self.leaves, self.host, before, self.state()):
            if kind == 'none':
                assert np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1), 'a leaf without gradient was touched'
                continue
            rp, rm, rv, tp, tm, tv = R.adam_ref(p0, h[1] if kind in ('g', 'both') else None, h[2] if kind in ('g2', 'both') else None, m0, v0, t, lr, tol=True)
            for key, got, ref, tol in (('m', m1, rm, tm), ('v', v1, rv, tv)):
                worst[key] = max(worst[key], R.compare(got, ref, tol)[1])
            if not slices:
                worst['p'] = max(worst['p'], R.compare(p1, rp, tp)[1])
            else:
                for s in range(slices):
                    ref, tol = R.adam_norm_ref(rp[s], tp[s])
                    worst['norm'] = max(worst['norm'], R.compare(p1[s], ref, tol)[1])
        print(f'Adam {name}: worst err/tol p {worst["p"]:.4f} m {worst["m"]:.4f} v {worst["v"]:.4f} renormalised {worst["norm"]:.4f}{_tag()}')
        assert max(worst.values()) <= 1.0, (name, worst)
        _no_misses()


def _tick_is_zero(taken):
    """The last word of every workspace HipAdam.step() took from hipops.zeros (2 n moments + the retirement counter, include/eg3d_hip.h) is 0 again.
    Only the LAST bank's launch counts retirements (bump_step != 0); for the earlier banks of a step of more than 32 items the kernel never touches
    the word, and the check says only that nothing else wrote it."""
    ws = [t for t in taken if t.dim() == 1]
    assert ws, 'no workspace seen'
    for t in ws:
        assert int(t[-1:].view(torch.int32)) == 0, 'the retirement counter was left non-zero'


def _standard_leaves():
    leaves = [((n,), k, 0) for n in R.ADAM_SIZES for k in KINDS]
    leaves += [(s, k, s[0]) for s, k in zip(R.ADAM_MAPS, ('both', 'g2', 'g'))]
    return leaves + [((37,), 'none', 0)]            # 24 + 7 slices = 31 items: one launch


@pytest.mark.parametrize('lr', [0.1, 3e-4])
@pytest.mark.parametrize('t0', [0, 999, 9999])
def test_adam_single_step_from_arbitrary_state(t0, lr):
    """Leaves of 1, 3, 4095, 4096, 4097, 8191, 12800 and 3 * 4096 + 1 elements with g, g2 or both; three renormalised maps; a leaf without any gradient;
    gradients from 1e-12 to 1e4 with exact zeros; step counts that reach late bias correction through powf."""
    S = _Leaves(_standard_leaves(), t0, lr, seed=t0 % 7)
    before = S.state()
    taken = S.step()
    S.check(f't {t0} lr {lr:g}', before, t0, lr)
    assert float(S.opt.step_t) == t0 + 1.0
    _tick_is_zero(taken)
    if _det():                       # the renormalised leaves depend on accumulated moments: bit-identical from run to run
        S2 = _Leaves(_standard_leaves(), t0, lr, seed=t0 % 7)
        S2.step()
        for (shape, kind, slices), a, b in zip(S.leaves, S.params, S2.params):
            if slices:
                assert torch.equal(a, b), 'two runs differ under the deterministic build'


@pytest.mark.parametrize('items', [33, 65])
def test_adam_banks_share_one_step_count(items):
    """More than 32 items take several launches: every bank uses the same t (the count is written once, by the last), and it rises by exactly 1."""
    sizes = (1, 5, 100, 4097, 513, 9000)
    leaves = [((sizes[i % len(sizes)],), KINDS[i % 3], 0) for i in range(items)]
    S = _Leaves(leaves, 7, 0.1, seed=3)
    for k in range(2):
        before = S.state()
        taken = S.step()
        S.check(f'{items} items, call {k}', before, 7 + k, 0.1)
        assert float(S.opt.step_t) == 8.0 + k
        assert len([t for t in taken if t.dim() == 1]) == -(-items // 32)
        _tick_is_zero(taken)


def test_adam_trajectory_of_five_steps_with_a_change_of_learning_rate():
    """Five steps with a host learning rate that drops from 0.1 to 3e-4 after the second; each step is compared from the device's own state before it,
    so the reference emulates no fp32 state."""
    leaves = [((12800,), 'both', 0), ((4097,), 'g', 0), ((2, 1, 64, 64), 'both', 2), ((3,), 'g2', 0)]
    S = _Leaves(leaves, 0, 0.1, seed=5, lr_tensor=False)
    for t in range(5):
        lr = 0.1 if t < 2 else 3e-4
        S.opt.param_groups[0]['lr'] = lr
        before = S.state()
        _tick_is_zero(S.step())
        S.check(f'trajectory step {t} lr {lr:g}', before, t, lr)
        assert float(S.opt.step_t) == t + 1.0


def test_adam_skip_changes_nothing():
    """skip = 1: p, m, v and the step count stay bit-identical; the next call with skip = 0 gives what it would have given without the skipped call."""
    leaves = [((12800,), 'both', 0), ((4097,), 'g2', 0), ((2, 1, 128, 128), 'both', 2), ((1,), 'g', 0)]
    S, T = _Leaves(leaves, 999, 3e-4, seed=9), _Leaves(leaves, 999, 3e-4, seed=9)
    flag = torch.ones((), device=DEV)
    before = S.state()
    _tick_is_zero(S.step(skip=flag))
    for a, b in zip(before, S.state()):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'a skipped step changed a leaf'
    assert float(S.opt.step_t) == 999.0
    flag.zero_()
    _tick_is_zero(S.step(skip=flag))
    T.step()
    S.check('after a skipped call', before, 999, 3e-4)
    assert float(S.opt.step_t) == 1000.0
    for (shape, kind, slices), a, b in zip(leaves, S.state(), T.state()):
        if not slices or _det():          # (a renormalised leaf of the normal build depends on the order of its float atomics)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'the step after a skipped one differs from the same step without it'


# ------------------------------------------------------------------------------------------------------------------ early stop
def test_early_stop_flag():
    from inv3d_amd import hipops
    thr = 0.25
    for value, want in ((0.3, 0.0), (float('nan'), 0.0), (float('inf'), 0.0), (0.25, 1.0), (0.2, 1.0)):
        done = torch.zeros((), device=DEV)
        hipops.early_stop_flag(torch.tensor(value, device=DEV), thr, done)
        assert float(done) == want, value
    done = torch.zeros((), device=DEV)
    for value, want in ((0.5, 0.0), (0.1, 1.0), (0.5, 1.0), (float('nan'), 1.0)):          # sticky once set
        hipops.early_stop_flag(torch.tensor(value, device=DEV), thr, done)
        assert float(done) == want, value


# ------------------------------------------------------------------------------------------------------------------ deterministic build
def test_deterministic_build_has_no_misses():
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        assert L.det_misses() == 0


def test_the_same_file_under_the_deterministic_build():
    """A fresh interpreter with EG3D_DETERMINISTIC=1 (the library is chosen at import) runs this file again."""
    from inv3d_amd import _lib as L
    if L.DETERMINISTIC:
        pytest.skip('already the deterministic build')
    env = dict(os.environ)
    env.pop('EG3D_LIBNAME', None)
    env['EG3D_DETERMINISTIC'] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', os.path.join('tests', 'test_gpu_step_ops.py')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print('\n'.join(l for l in r.stdout.splitlines() if 'err/tol' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and '1 skipped' in r.stdout, r.stdout[-1000:]
