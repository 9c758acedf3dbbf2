"""CPU-side checks (no GPU needed): the C-ABI library loads and exports every symbol include/eg3d_hip.h declares, the
product refuses CPU tensors instead of falling back, host-side tap-list / packing logic, state-dict schema, and the
product's synthetic-input generator matches the oracle's."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from inv3d_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'eg3d_hip.h')).read()
    declared = set(re.findall(r'\b(eg3d_[a-z0-9_]+)\s*\(', hdr))
    assert declared, 'no declarations parsed'
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/eg3d_hip.h but not exported by libeg3d_hip.so'
    assert declared == set(L.EXPORTED_SYMBOLS), declared ^ set(L.EXPORTED_SYMBOLS)
    assert lib.eg3d_abi_version() == 1
    assert lib.eg3d_status_string(-2) == b'unsupported configuration'


def test_deterministic_build_exports_the_same_symbols():
    """`make det` -> libeg3d_hip_det.so (csrc/det.h): same C-ABI; only it reports eg3d_det_enabled() == 1."""
    import ctypes as C
    from inv3d_amd import _lib as L
    path = os.path.join(os.path.dirname(L.LIB_PATH), 'libeg3d_hip_det.so')
    assert os.path.exists(path), 'build it with `make -C 3dgan-inversion_amd` (both libraries are default targets)'
    det = C.CDLL(path)
    for name in L.EXPORTED_SYMBOLS:
        assert hasattr(det, name), name
    det.eg3d_det_enabled.restype = C.c_int
    assert det.eg3d_det_enabled() == 1
    if not L.DETERMINISTIC:
        assert L.lib().eg3d_det_enabled() == 0
        assert L.lib().eg3d_det_set_workspace(None, 0, None) == -2             # EG3D_ERR_UNSUPPORTED: the normal build has no such mode


def test_render_size_query_is_host_only():
    """eg3d_render_query_sizes: the buffer-size contract of the renderer entries, answerable without a GPU."""
    import ctypes as C
    from inv3d_amd import _lib as L
    p = L.RenderParams()
    p.N, p.R, p.Dc, p.Df, p.Cout = 2, 128 * 128, 48, 48, 32
    z = L.RenderSizes()
    assert L.lib().eg3d_render_query_sizes(C.byref(p), C.byref(z)) == 0
    S = 2 * 128 * 128 * 2 * 48
    assert (z.S, z.rgb, z.depth, z.fine_depths, z.save_rgb, z.pos_rows) == (S, 2 * 16384 * 32, 2 * 16384, 2 * 16384 * 48, S * 32, S * 4)
    assert (z.df_rows, z.df_pos, z.ag_rows, z.gc_rows, z.dump_dout) == (S * 32, S * 4, S * 2, S * 4, S * 33)
    p.Dc = 0
    assert L.lib().eg3d_render_query_sizes(C.byref(p), C.byref(z)) != 0


def test_no_cpu_fallback():
    from inv3d_amd._lib import Eg3dHipError
    from inv3d_amd.torch_utils.ops import bias_act, upfirdn2d, conv2d_resample
    x = torch.randn(1, 4, 8, 8)
    with pytest.raises(Eg3dHipError):
        bias_act.bias_act(x, torch.randn(4))
    with pytest.raises(Eg3dHipError):
        upfirdn2d.upfirdn2d(x, upfirdn2d.setup_filter([1, 3, 3, 1]))
    with pytest.raises(Eg3dHipError):
        conv2d_resample.conv2d_resample(x, torch.randn(4, 4, 3, 3), padding=1)
    # the EXPLICIT impl='ref' is the reference's own keyword (bias_act.py:84-88): a product-owned plain-torch composite (tests/test_ref_impl.py),
    # never reached without that argument
    assert torch.equal(bias_act.bias_act(x, impl='ref'), x)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, '3dgan-inversion_amd', 'inv3d_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, re.M), f'{f} imports the oracle'
                assert '/root/reference' not in src
    # ... and the library reads no environment: what an entry does is a function of its arguments, every switch is one test_default_switch_state sees
    csrc = os.path.join(ROOT, '3dgan-inversion_amd', 'csrc')
    assert [f for f in sorted(os.listdir(csrc)) if 'getenv' in open(os.path.join(csrc, f)).read()] == []


def test_tap_lists():
    from inv3d_amd import hipops as H
    c, = H.classes_corr(8, 8, 3, 3, 1)
    assert c.ntaps == 9 and (c.dy[0], c.dx[0], c.wtap[0]) == (-1, -1, 0) and (c.dy[8], c.dx[8], c.wtap[8]) == (1, 1, 8)
    cls, ho, wo = H.classes_convT(4, 4, 3, 3, 2)
    assert (ho, wo) == (9, 9) and len(cls) == 4
    assert sorted(k.ntaps for k in cls) == [1, 2, 2, 4]
    assert sum(k.Ha * k.Wa for k in cls) == 81                       # the phases tile the (2H+1)^2 output exactly
    ee = [k for k in cls if k.out_py == 0 and k.out_px == 0][0]
    assert (ee.Ha, ee.Wa) == (5, 5) and sorted((ee.dy[i], ee.dx[i]) for i in range(4)) == [(-1, -1), (-1, 0), (0, -1), (0, 0)]
    a, = H.classes_convT_adjoint(4, 4, 3, 3, 2)
    assert a.ntaps == 9 and max(a.dy[i] for i in range(9)) == 2
    f, = H.classes_corr(8, 8, 3, 3, 1, flip_taps=True)
    assert f.wtap[0] == 8 and f.wtap[8] == 0
    w = torch.arange(2 * 4 * 3 * 3, dtype=torch.float32).reshape(2, 4, 3, 3)
    wf, wa = H.pack_weight_fwd(w), H.pack_weight_adj(w)
    assert wf.shape == (2, 36) and wa.shape == (4, 18)
    assert wf[1, (1 * 3 + 2) * 4 + 3] == w[1, 3, 1, 2] and wa[3, (1 * 3 + 2) * 2 + 1] == w[1, 3, 1, 2]


def test_schema_and_synthetic_inputs_match_oracle():
    from inv3d_amd import synthetic as S
    from oracle import eg3d_oracle as O
    cfg = O.small_config()
    G = S.make_generator(w_dim=32, z_dim=32, plane_res=32, channel_base=256, channel_max=16, nrr=16, sr_in_res=16, sr_widths=(16, 8),
                         rendering_kwargs=cfg.rendering, device='cpu')
    W = S.load_synthetic_weights(G, 0)
    P = O.synth_params(cfg, 0)
    assert set(W) == set(P)
    assert all(torch.equal(W[k], P[k]) for k in P)
    assert torch.equal(S.synth_cameras(3), O.synth_cameras(3))
    assert torch.equal(S.synth_ws(cfg.num_ws, 32, 2, wplus=True), O.synth_ws(cfg, 2, wplus=True))
    u1, u2 = S.make_uniforms(2, 256, 12, 12)
    v1, v2 = O.make_uniforms(cfg, 2)
    assert torch.equal(u1, v1) and torch.equal(u2, v2)
    full = S.make_generator(device='cpu')
    assert set(full.state_dict()) == set(O.param_shapes(O.full_config()))
    assert sum(p.numel() for p in full.parameters()) == 30662136
    assert full.backbone.num_ws == 14


def test_zero_arena_and_memo_host_logic():
    """Host-side helpers of the step: ZeroArena (one zero-fill per step, sized by the previous step's demand, fallback when it does not
    fit) and memo() (derived weight images keyed on storage + in-place version + object identity).  Pure host logic, CPU tensors."""
    import torch
    from inv3d_amd import hipops as H
    arena = H.ZeroArena(torch.device('cpu'))
    shapes = [(3, 5), (1, 8, 4, 4), (70,)]
    for step in range(3):
        with H.zero_arena(arena):
            outs = [H.zeros(shapes[0], 'cpu'), H.zeros_cl(*shapes[1], 'cpu'), H.zeros(shapes[2], 'cpu')]
            for t, sh in zip(outs, shapes):
                assert tuple(t.shape) == sh and float(t.abs().sum()) == 0.0
                t += 1.0                                           # dirty it: the next step must see zeros again
            assert outs[1].is_contiguous(memory_format=torch.channels_last)
            if step == 0:
                assert arena.buf is None                           # nothing known yet: plain torch.zeros
            else:
                base = arena.buf.data_ptr()
                assert all(base <= t.data_ptr() < base + arena.buf.numel() * 4 for t in outs)
                assert outs[0].data_ptr() % 256 == outs[2].data_ptr() % 256 == base % 256      # 256-byte granules
        assert arena.prev_demand == 64 + 128 + 128
    assert H.ARENA is None
    with H.zero_arena(arena):
        big = H.zeros((4096,), 'cpu')                              # does not fit: falls back, arena grows for the next step
        assert arena.buf is None or not (arena.buf.data_ptr() <= big.data_ptr() < arena.buf.data_ptr() + arena.buf.numel() * 4)
    assert arena.prev_demand >= 4096

    calls = []
    w = torch.arange(6.).reshape(2, 3)
    f = lambda: (calls.append(1), w * 2)[1]
    a = H.memo('t', [w], f); b = H.memo('t', [w], f)
    assert a is b and len(calls) == 1
    w.add_(1.0)                                                    # in-place update bumps the version -> recompute
    c = H.memo('t', [w], f)
    assert len(calls) == 2 and torch.equal(c, w * 2)
    w2 = w.clone()
    H.memo('t', [w2], lambda: (calls.append(1), w2 * 2)[1])
    assert len(calls) == 3                                         # a different tensor object never hits another one's entry
    # updates that do not bump the version counter (fused multi-tensor optimisers write through raw pointers): weights_changed()
    w2.requires_grad_(True)                                        # an optimiser's parameter (frozen tensors ignore the epoch, below)
    H.memo('t', [w2], lambda: (calls.append(1), w2 * 2)[1])
    n = len(calls)
    w2.data_ptr()
    with torch.no_grad():
        w2.view(-1).numpy()[:] = 7.0                               # same storage, same version
    assert torch.equal(H.memo('t', [w2], lambda: (calls.append(1), w2 * 2)[1]), torch.full((2, 3), 14.0)) is False or len(calls) == n
    H.weights_changed()
    d = H.memo('t', [w2], lambda: (calls.append(1), w2 * 2)[1])
    assert len(calls) == n + 1 and torch.equal(d, torch.full((2, 3), 14.0))
    # frozen sources (loss / pose / encoder networks during pivotal tuning) keep their images across the tuned generator's steps
    fz = torch.ones(2, 2)
    e = H.memo('frozen', [fz], lambda: (calls.append(1), fz * 3)[1])
    n = len(calls)
    H.weights_changed()
    assert H.memo('frozen', [fz], lambda: (calls.append(1), fz * 3)[1]) is e and len(calls) == n
    from inv3d_amd import fused
    cache = fused.WeightCache()
    cache._c = {'k': (w2.data_ptr(), w2._version, tuple(w2.shape), H.WEIGHTS_EPOCH - 1)}
    assert cache._c['k'] != (w2.data_ptr(), w2._version, tuple(w2.shape), H.WEIGHTS_EPOCH)     # an epoch bump invalidates packed conv weights too


def test_install_as_reference_modules_on_a_stand_in_checkout(tmp_path):
    """The binding mechanism itself, runnable anywhere: a directory with the checkout's package skeleton (training/, torch_utils/ops/,
    training/volumetric_rendering/, a persistence module with import_hook, one caller module) is put on sys.path; after
    install_as_reference_modules() the hot-path names are this package's module OBJECTS, the caller module stays the checkout's, and
    putting .../inv3d_amd itself on sys.path (the broken recipe of round 1) is refused with a clear message."""
    import subprocess
    import sys
    for d in ('training/volumetric_rendering', 'training/coaches', 'torch_utils/ops'):
        (tmp_path / d).mkdir(parents=True)
    for d in ('training', 'training/volumetric_rendering', 'training/coaches', 'torch_utils', 'torch_utils/ops'):
        (tmp_path / d / '__init__.py').write_text('')
    (tmp_path / 'torch_utils' / 'persistence.py').write_text('_hooks = []\ndef import_hook(h):\n    _hooks.append(h)\n')
    (tmp_path / 'training' / 'coaches' / 'base_coach.py').write_text(
        'from training.triplane import TriPlaneGenerator\nfrom torch_utils.ops import bias_act, conv2d_gradfix\nWHO = "checkout"\n')
    code = f"""
import sys
sys.path.insert(0, {str(tmp_path)!r}); sys.path.insert(0, {os.path.join(ROOT, '3dgan-inversion_amd')!r})
import inv3d_amd
inv3d_amd.install_as_reference_modules()
import training.coaches.base_coach as bc, training, torch_utils.ops, torch_utils.persistence as P
import inv3d_amd.training.triplane as T, inv3d_amd.torch_utils.ops.conv2d_gradfix as CG
assert bc.WHO == 'checkout' and bc.__file__.startswith({str(tmp_path)!r})
assert bc.TriPlaneGenerator is T.TriPlaneGenerator and training.triplane is T and sys.modules['training.triplane'] is T
assert bc.conv2d_gradfix is CG and torch_utils.ops.conv2d_gradfix is CG
assert len(P._hooks) == 1
inv3d_amd.install_as_reference_modules(); assert len(P._hooks) == 1      # idempotent
print('BOUND')
"""
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'BOUND' in r.stdout, r.stdout + r.stderr[-3000:]
    bad = f"""
import sys
sys.path.insert(0, {os.path.join(ROOT, '3dgan-inversion_amd')!r}); sys.path.insert(0, {os.path.join(ROOT, '3dgan-inversion_amd', 'inv3d_amd')!r})
import inv3d_amd
try:
    inv3d_amd.install_as_reference_modules()
except ImportError as e:
    print('REFUSED', e)
"""
    r = subprocess.run([sys.executable, '-c', bad], capture_output=True, text=True, timeout=300)
    assert 'REFUSED' in r.stdout, r.stdout + r.stderr[-3000:]


def test_round2_entry_points_reject_bad_arguments_before_touching_the_gpu():
    """Argument validation of the entry points added in round 2 returns EG3D_ERR_INVALID / _UNSUPPORTED (negative status, never a launch):
    null pointers, sizes that are not multiples of four floats, misaligned pointers, more layers than a pack batch holds."""
    import ctypes as C
    from inv3d_amd import _lib as L
    lib = L.lib()
    a = 0x10000                                            # a non-null, 16-byte aligned fake address (never dereferenced: validation fails first)
    assert lib.eg3d_sqdist_sum_fwd(None, a, 64, a, 1.0, a, 1.0, None) < 0
    assert lib.eg3d_sqdist_sum_fwd(a, a, 62, a, 1.0, a, 1.0, None) < 0               # n % 4
    assert lib.eg3d_sqdist_sum_fwd(a, a + 4, 64, a, 1.0, a, 1.0, None) < 0           # misaligned
    assert lib.eg3d_sqdist_sum_fwd(a, a, 64, None, 1.0, None, 1.0, None) < 0         # nowhere to write
    assert lib.eg3d_sqdist_sum_bwd(a, a, None, 1.0, a, 64, None) < 0
    assert lib.eg3d_tv_norm_fwd(a, 1, 1, 8, a, 1.0, a, 1.0, None) < 0                # H < 2
    assert lib.eg3d_tv_norm_bwd(a, a, 1.0, None, 1, 8, 8, None) < 0
    assert lib.eg3d_slice_rgb4_fwd(a, a, 16, 30, None) < 0                           # C % 4
    assert lib.eg3d_slice_rgb4_bwd(None, a, 16, 32, None) < 0
    assert lib.eg3d_split_weight_pieces(a, a, 6, None) < 0
    assert lib.eg3d_split_weight_pieces(a, a + 8, 16, None) < 0
    assert lib.eg3d_weight_grad_finish(None, a, a, a, a, a, 1, 8, 8, 9, None) < 0
    assert lib.eg3d_weight_grad_finish(a, a, None, None, a, a, 1, 8, 8, 9, None) < 0  # dd without styles / d
    items = (L.PackItem * 1)()
    assert lib.eg3d_pack_conv_weights_batched(items, 0, None) < 0
    assert lib.eg3d_pack_conv_weights_batched(items, L.PACK_BATCH_MAX + 1, None) < 0
    assert lib.eg3d_pack_conv_weights_batched(items, 1, None) < 0                     # null weight pointer in the item
    assert lib.eg3d_pack_conv_weight_padded(a, a, a, None, 8, 8, 9, 4, None) < 0      # O_pad < O
    ab = L.ActBwd()
    assert lib.eg3d_torgb_dgrad_act(None, a, a, a, None, a, None, 1, 8, 8, 16, C.byref(ab), None, None) < 0
    assert lib.eg3d_torgb_dgrad_act(a, a, a, a, None, a, None, 1, 8, 8, 18, C.byref(ab), None, None) < 0   # C % 4
    assert lib.eg3d_torgb_dgrad_act_split(a, a, a, a, None, None, None, 1, 8, 8, 16, C.byref(ab), None, None, a, a, None) < 0      # no max|dy|
    assert lib.eg3d_torgb_dgrad_act_split(a, a, a, a, a, None, None, 1, 8, 8, 16, C.byref(ab), a, None, a, a, None) < 0            # addend without its maximum
    assert lib.eg3d_torgb_dgrad_act_split(a, a, a, a, None, None, None, 1, 8, 8, 20, C.byref(ab), a, None, a, a, None) < 0         # C % 8
    ts = L.TorgbSmallParams(x=a, w=a, s=a, out=a, N=1, H=4, W=4, C=64, Cp=96, ldx=64, ldo=96, w_row=64, clamp=-1.0)
    assert lib.eg3d_torgb_small_supported(C.byref(ts)) == 1
    ts.Cp = 4                                                                        # outputs not a multiple of 32: the implicit GEMM's case
    assert lib.eg3d_torgb_small_supported(C.byref(ts)) == 0 and lib.eg3d_torgb_small_fwd(C.byref(ts), None) < 0
    tb = L.TorgbSmallBwdParams(dy=a, wa=a, s=a, dx=a, ds=a, N=1, H=4, W=4, C=64, Cp=96, ldg=96, ldx=64, wa_row=96)
    assert lib.eg3d_torgb_small_bwd_supported(C.byref(tb)) == 0                      # a style gradient without the layer input
    tb.xin = a
    assert lib.eg3d_torgb_small_bwd_supported(C.byref(tb)) == 1
    # the streaming forms take the backbone's 128^2 / 256^2 geometries and nothing the small kernels are for
    assert lib.eg3d_torgb_mid_supported(C.byref(ts)) == 0 and lib.eg3d_torgb_mid_bwd_supported(C.byref(tb)) == 0
    for (hw, c, want) in ((128, 256, 1), (256, 128, 1), (64, 512, 0), (128, 512, 0), (120, 96, 1), (100, 128, 0)):
        tm = L.TorgbSmallParams(x=a, w=a, s=a, out=a, N=1, H=hw, W=hw, C=c, Cp=96, ldx=c, ldo=96, w_row=c, clamp=-1.0)
        assert lib.eg3d_torgb_mid_supported(C.byref(tm)) == want, (hw, c)
        tmb = L.TorgbSmallBwdParams(dy=a, wa=a, s=a, dx=a, xin=a, ds=a, N=1, H=hw, W=hw, C=c, Cp=96, ldg=96, ldx=c, wa_row=96)
        assert lib.eg3d_torgb_mid_bwd_supported(C.byref(tmb)) == (1 if hw * hw >= 4096 and (hw * hw) % 32 == 0 else 0), (hw, c)
    tm.pre_z = a                                                                     # a pending finishing epilogue: the small kernel's business
    tm.pre_gain = 1.0
    assert lib.eg3d_torgb_mid_supported(C.byref(tm)) == 0
    ad = L.AdamList(n=1, bump_step=1, beta1=0.9, beta2=0.999, eps=1e-8, lr=a, step=a)
    ad.items[0] = L.AdamItem(a, None, None, a, a, 16, 0)
    assert lib.eg3d_adam_step(C.byref(ad), a, None) < 0                              # no gradient at all
    ad.items[0] = L.AdamItem(a, a, None, a, a, 16, 0)
    assert lib.eg3d_adam_step(C.byref(ad), None, None) < 0                           # no workspace
    ad.n = L.ADAM_ITEMS_MAX + 1
    assert lib.eg3d_adam_step(C.byref(ad), a, None) < 0
    ul = L.UnitLevels(n=1, N=1, eps=1e-10, feat_nstride=64)
    ul.levels[0] = L.UnitLevel(x=a, scale=None, feat=a, dx=None, HW=4, C=16, ldx=16, mul=1.0)
    assert lib.eg3d_unit_normalize_levels(C.byref(ul), 1, None) < 0                  # backward without dx
    ul.n = L.UNIT_LEVELS_MAX + 1
    assert lib.eg3d_unit_normalize_levels(C.byref(ul), 0, None) < 0
    ul.n, ul.levels[0].C = 1, 18
    assert lib.eg3d_unit_normalize_levels(C.byref(ul), 0, None) < 0                  # C % 4
    p = L.ConvParams()
    p.x = p.w = p.out = a
    p.N, p.Hi, p.Wi, p.Ck, p.ldx, p.Nc, p.w_row, p.Ho, p.Wo, p.ldo = 1, 8, 8, 16, 16, 16, 16, 8, 8, 16
    p.in_stride = p.out_stride = p.ncls = p.ksplit = 1
    p.epi, p.precision, p.w_presplit = L.EPI_STORE, 1, 1                             # pre-split weights only exist for the fp16 split
    assert lib.eg3d_conv2d_igemm_f32(C.byref(p), None) < 0


def test_triplane_scatter_refuses_what_is_outside_its_range_before_touching_the_gpu():
    """eg3d_triplane_scatter has one path (row-keyed lists): planes up to 270 x 270 and S = N * rows_per_image (include/eg3d_hip.h).  Outside
    that range both builds answer EG3D_ERR_UNSUPPORTED from the arguments alone -- no HIP call, hence answerable here."""
    import ctypes as C
    from inv3d_amd import _lib as L
    INVALID, UNSUPPORTED = -1, -2
    assert L.lib().eg3d_status_string(INVALID) == b'invalid argument' and L.lib().eg3d_status_string(UNSUPPORTED) == b'unsupported configuration'
    libs = [L.lib()]
    if not L.DETERMINISTIC:
        det = C.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), 'libeg3d_hip_det.so'))
        det.eg3d_triplane_scatter.restype, det.eg3d_triplane_scatter.argtypes = L.lib().eg3d_triplane_scatter.restype, L.lib().eg3d_triplane_scatter.argtypes
        libs.append(det)
    a = 0x10000                                            # non-null fake addresses (never dereferenced: validation fails first)
    for lib in libs:
        #                              df_rows df_pos S rows_per_image d_planes N Hp Wp ldp box_warp workspace ray_w rows_per_ray df_amax stream
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 512, 512, 96, 1.0, a, 0, 0, None, None) == UNSUPPORTED      # 3 * 35 * 35 * 16 > 16384 lists
        assert lib.eg3d_triplane_scatter(a, a, 3, 1, a, 2, 32, 32, 96, 1.0, a, 0, 0, None, None) == UNSUPPORTED          # S != N * rows_per_image
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 32, 32, 64, 1.0, a, 0, 0, None, None) == UNSUPPORTED        # ldp < 96
        assert lib.eg3d_triplane_scatter(None, a, 96, 96, a, 1, 32, 32, 96, 1.0, a, 0, 0, None, None) == INVALID
        assert lib.eg3d_triplane_scatter(a, a, 96, 96, a, 1, 32, 32, 96, 1.0, None, 0, 0, None, None) == INVALID         # no workspace
    # the workspace covers what the entry carves: counts, fill, offsets (+ 1), up to 3 ints of alignment, one 16-byte record per (sample, plane)
    nb16 = 3 * 18 * 18 * 16
    assert L.lib().eg3d_triplane_scatter_workspace_ints(1000, 2, 256, 256) == 3 * nb16 + 1 + 3 + 12 * 1000


def test_default_switch_state():
    """Every EG3D_* environment switch of the package, read in a process with NO EG3D_* variable set, has the value committed in
    tests/golden/default_switches.json -- a default that flips (or a new switch) must show up in a diff of that file, not silently in the
    numbers.  Regenerate with:  env -i PATH=$PATH HOME=$HOME python tests/support/dump_switches.py /root/repo  (then basename any path value)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith('EG3D_')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'support', 'dump_switches.py'), ROOT], env=env, capture_output=True, text=True, check=True).stdout
    now = json.loads(out)
    for k, v in now.items():
        if k != 'inline_defaults' and isinstance(v['value'], str) and os.sep in v['value']:
            v['value'] = os.path.basename(v['value'])
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'default_switches.json')))
    assert sorted(now) == sorted(want), sorted(set(now) ^ set(want))
    for k in want:
        assert now[k] == want[k], (k, now[k], want[k])


def test_ctypes_structures_match_the_header():
    """Every parameter structure of inv3d_amd/_lib.py has the size and the field offsets of its C definition in include/eg3d_hip.h (compiled
    here with gcc: the header is plain C, as an FFI boundary must be) -- a field appended on one side only would otherwise show up as wrong
    numbers on the GPU, or not at all."""
    import ctypes as C
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    from inv3d_amd import _lib as L
    pairs = [('eg3d_conv_class', L.ConvClass), ('eg3d_act_bwd', L.ActBwd), ('eg3d_conv_params', L.ConvParams), ('eg3d_conv_ws_params', L.ConvWsParams),
             ('eg3d_conv_v2_params', L.ConvV2Params), ('eg3d_conv_up2_params', L.ConvUp2Params), ('eg3d_wgrad_params', L.WgradParams),
             ('eg3d_wgrad_v2_params', L.WgradV2Params), ('eg3d_render_params', L.RenderParams), ('eg3d_render_bwd_params', L.RenderBwdParams),
             ('eg3d_render_sizes', L.RenderSizes), ('eg3d_split_w_item', L.SplitWItem), ('eg3d_split_w_batch', L.SplitWBatch),
             ('eg3d_torgb_small_params', L.TorgbSmallParams), ('eg3d_torgb_small_bwd_params', L.TorgbSmallBwdParams),
             ('eg3d_conv3x3_direct_params', L.Conv3x3DirectParams), ('eg3d_adam_item', L.AdamItem), ('eg3d_adam_list', L.AdamList),
             ('eg3d_unit_level', L.UnitLevel), ('eg3d_unit_levels', L.UnitLevels), ('eg3d_flrelu_params', L.FlreluParams),
             ('eg3d_style_layer', L.StyleLayer), ('eg3d_style_bank', L.StyleBank), ('eg3d_wgf_item', L.WgfItem), ('eg3d_pack_item', L.PackItem),
             ('eg3d_mc_params', L.McParams), ('eg3d_ssim_params', L.SsimParams), ('eg3d_batchnorm_params', L.BatchNormParams)]
    header = open(os.path.join(ROOT, 'include', 'eg3d_hip.h')).read()
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eg3d_hip.h"', 'int main(void) {']
    want = []
    for cname, cls in pairs:
        assert cname in header, cname
        src.append(f' printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            if f[0].startswith('pad') or f[0].startswith('_'):          # explicit padding on the Python side, implicit in C
                continue
            src.append(f' printf("%zu\\n", offsetof({cname}, {f[0]}));')
            want.append(getattr(cls, f[0]).offset)
    src += [' return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write('\n'.join(src) + '\n')
        r = subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        got = [int(v) for v in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(want, got)) if a != b][:5]
