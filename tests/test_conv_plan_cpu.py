"""The routing of the style-modulated convolutions (inv3d_amd/conv_plan.py), pinned without a GPU: the planner is pure host code and the
library's `*_supported` geometry queries answer on any machine the library loads on."""
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ('f16x3', 'f16x1')


def _golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')))


def _layers():
    return [(g['Ci'], g['Co'], g['Hi'], g['Wi'], g['up']) for g in (v['geometry'] for v in _golden().values())]


def _odd_geometries():
    """Channel counts that are not multiples of 64 / 128, W > 32 at small H, N = 3, next to the ordinary ones."""
    grids = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (4, 64), (8, 40), (2, 128), (17, 33), (5, 7), (64, 4))
    return itertools.product((1, 2, 3, 8), (16, 48, 64, 96, 200, 256, 512), (3, 32, 96, 128, 192, 512), grids, (1, 2))


def test_routes_of_the_full_size_generator_match_the_golden_table():
    """Every modulated 3x3 layer of the full-size generator (backbone b4 .. b256, both super-resolution blocks: 17 layers) at N in 1, 2, 8, frozen
    and trainable weights, f16x3 and f16x1: forward, data-gradient and weight-gradient plans equal tests/golden/conv_routes.json -- a threshold
    edit that re-routes a full-size layer must show up in a diff of that file.  The table was first written from the routing conditions of
    ModConvLayerFn before the planner existed, evaluated with that commit's hipops; tools/check_conv_routes.py compares it with the launches
    a tree records under hipops.LaunchProfiler.
    Regenerate with:  python tools/conv_launch_table.py --plan --json > tests/golden/conv_routes.json"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('EG3D_')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'conv_launch_table.py'), '--plan', '--json'], env=env, capture_output=True, text=True, check=True).stdout
    now, want = json.loads(out), _golden()
    assert len(want) == 17 and sorted(now) == sorted(want)
    for name in want:
        assert now[name]['geometry'] == want[name]['geometry'], name
        assert sorted(now[name]['routes']) == sorted(want[name]['routes']) and len(want[name]['routes']) == 12, name
        for key, row in want[name]['routes'].items():
            assert now[name]['routes'][key] == row, (name, key, now[name]['routes'][key], row)


def test_forward_predictions_agree_with_the_backward():
    """The forward's promises are read from the backward's own planner (fused.ModConvLayerFn: rec.split_ok from plan_dgrad, ctx.aimg from
    plan_wgrad), so they cannot disagree by construction; what can is checked here over the golden table plus odd geometries (channel counts that
    are not multiples of 64 / 128, W > 32 at small H, N = 3): the form a dz operand image is promised for takes one; the kept operand image does
    not depend on what the backward learns later (max|dz| known or not, which gradients are wanted); and the parity-split FIR adjoint of an up
    layer serves both launches that read it or neither."""
    from inv3d_amd import conv_plan as P
    cases = [(n,) + l for l in _layers() for n in (1, 2, 8)] + [(n, ci, co, h, w, up) for n, ci, co, (h, w), up in _odd_geometries()]
    handed = kept = 0
    for (N, Ci, Co, Hi, Wi, up), prec, frozen in itertools.product(cases, PRECS, (True, False)):
        g = (N, Ci, Co, Hi, Wi, 3, up, prec)
        d0 = P.plan_dgrad(*g, frozen)
        assert d0.takes_image == (d0.form in ('v2', 'v3')) and (d0.form != 'v2' or d0.rows in (4, 8)), (g, d0)
        handed += d0.form == 'v2'
        fwd = P.plan_forward(*g, frozen)
        for amax_known, need_dx in itertools.product((True, False), repeat=2):
            w = P.plan_wgrad(*g, amax_known=amax_known, need_dx=need_dx)
            assert w == P.plan_wgrad(*g, amax_known=amax_known, need_dx=need_dx, fwd=fwd), (g, w)
            assert w.keep_ximg == P.plan_wgrad(*g).keep_ximg and (w.form not in ('v2', 'v2_slabs') or w.keep_ximg), (g, w)
            d = P.plan_dgrad(*g, frozen, amax_known=amax_known, need_dx=need_dx, need_w=True)
            assert (w.form == 'v2_up') == d.fir_split and (d.form in ('s2adj', 'v3_s2adj')) == (d.fir_split and need_dx), (g, w, d)
            kept += w.keep_ximg
    assert handed > 100 and kept > 100          # (the sweep reaches both promises)


@pytest.mark.parametrize('mode', ['f32', 'bf16x6'])
def test_forced_conv_mode_keeps_every_layer_on_the_loader_split_kernel(mode, monkeypatch):
    from inv3d_amd import conv_plan as P, hipops as H
    monkeypatch.setattr(H, 'CONV_MODE', mode)
    monkeypatch.setattr(H, 'CONV_PRECISION', H.PRECISIONS[mode])
    prec = H.modconv_precision()
    assert prec == mode
    for (Ci, Co, Hi, Wi, up), N, frozen in itertools.product(_layers(), (1, 2, 8), (True, False)):
        for p in (prec,) + PRECS:       # (a per-layer 'f16x1' request changes nothing while the mode is forced: the predicates read CONV_MODE)
            g = (N, Ci, Co, Hi, Wi, 3, up, p)
            f, d, w = P.plan_forward(*g, frozen), P.plan_dgrad(*g, frozen, need_w=not frozen), P.plan_wgrad(*g)
            assert f.form in ('igemm', 'igemm_up', 'igemm_splitk') and not f.presplit, (g, f)
            assert not P.consumer_reads_split(N, Co, Hi * up, Wi * up, p)
            assert d.form in ('igemm', 'igemm_splitk') and not d.fir_split and not d.takes_image, (g, d)
            assert w.form == 'igemm' and not w.keep_ximg, (g, w)


def test_monkeypatched_switch_reroutes_the_next_plan(monkeypatch):
    """Switches are read from hipops at call time, not copied at import."""
    from inv3d_amd import conv_plan as P, hipops as H
    g = (1, 256, 256, 128, 128, 3, 1, 'f16x3')
    assert P.plan_forward(*g, True).rows == 4
    monkeypatch.setattr(H, 'V2_HALF', False)
    assert P.plan_forward(*g, True).form != 'v2'
    monkeypatch.setattr(H, 'V2_HALF', True)
    monkeypatch.setattr(H, 'USE_V2', False)
    assert not P.plan_forward(*g, True).presplit and P.plan_dgrad(*g, True).form == 'igemm'
