"""Which kernel a style-modulated convolution runs on: ONE function of the layer geometry per pass (forward, data gradient, weight
gradient), read by fused.ModConvLayerFn.  Pure host code -- no tensors, no stream, no allocation; the library's `*_supported` geometry
queries read no pointer and answer without a GPU.  tests/test_conv_plan_cpu.py pins the output for every layer of the full-size generator
(tests/golden/conv_routes.json); `python tools/conv_launch_table.py --plan` prints it.

The building blocks (tap-class lists, per-kernel geometry predicates, the environment switches and thresholds they read) stay in hipops and
are read at call time, so a switch patched on that module re-routes the next call."""
from typing import NamedTuple, Optional, Tuple

from . import hipops as H

KS_TARGET = 256       # blocks a split launch aims for (one per CU; 512 measured 0.7 % slower per step)


def _auto_ksplit(classes, N, Nc, Ck):
    """Split-K factor of an implicit GEMM whose output grid is too small to keep 256 CUs busy (the 4^2..64^2 layers): with few
    128x128 tiles each workgroup walks a long K = taps x channels chain on its own and the launch is latency-bound (64^2 x 512
    channels: 91 TF unsplit, 148 TF split 4 ways).  Slices accumulate with fp32 atomics into a zeroed buffer."""
    blocks = sum((N * c.Ha * c.Wa + 127) // 128 for c in classes) * ((Nc + 127) // 128)
    if blocks >= 200:           # measured: splitting layers with 256 tiles (128^2 x 256 ch) costs more in zero-fill + finish passes than it gains
        return 1
    steps = ((Ck + 15) // 16) * min(c.ntaps for c in classes)
    # 64^2 x 512 (128 tiles, one tap class): 4 slices beat 2 (198 vs 164 TFLOP/s stand-alone, +0.2 % per step); smaller grids keep the target
    target = KS_TARGET * 2 if (len(classes) == 1 and blocks >= 64) else KS_TARGET
    return max(1, min(-(-target // blocks), steps // 8))


def presplit_arith(prec) -> bool:
    """The precisions the pre-split kernels (two-piece fp16 operand images) implement; every other one is a loader-split launch."""
    return prec in ('f16x3', 'f16x1')


def products(prec) -> int:
    """MFMA products per fp32 product on the pre-split kernels ('f16x1': the high pieces only)."""
    return 1 if prec == 'f16x1' else 3


def loader_precision(prec) -> str:
    """Arithmetic of a launch that stays on the loader-split kernel: it has no single-product form and keeps the three products."""
    return 'f16x3' if prec == 'f16x1' else prec


class ForwardPlan(NamedTuple):
    form: str                   # 'v2' | 'v3' | 'igemm' | 'ws' | 'igemm_splitk' (up 1);  'up2' | 'igemm_up' | 'ws_up' | 'igemm_splitk' (up 2)
    presplit: bool              # the operands are split images (activation: split_activation, weights: WeightCache.get_split)
    finish: bool                # the launch leaves raw sums: a separate epilogue pass follows (every up layer: its FIR epilogue)
    ksplit: int = 1             # 'igemm_splitk' / 'up2': split-K factor
    rows: int = 0               # 'v2' / 'up2': patch rows
    v3: Optional[Tuple[int, int]] = None        # 'v3': (rows, waves)
    ragged: bool = False        # 'up2': one launch covers the full (Hi + 1) x (Wi + 1) cell grid (else main grid + border classes)
    rgb_head: bool = False      # 'v2': the launch can carry the 1x1 toRGB head in its epilogue


class DgradPlan(NamedTuple):
    form: Optional[str]         # 's2adj' | 'v3_s2adj' | 'v2' | 'v3' | 'ws' | 'ws_s2' | 'igemm' | 'igemm_splitk'; None: no data / style gradient wanted
    fir_split: bool             # up 2: the FIR adjoint writes the gradient operand as parity-split fp16 images (no fp32 g)
    finish: bool = False        # split-K partial sums: dgrad_finish / dgrad_finish_act follows
    ksplit: int = 1             # 'igemm_splitk'
    rows: int = 0               # 'v2'
    v3: Optional[Tuple[int, int]] = None        # 'v3'

    @property
    def takes_image(self) -> bool:
        """The launch reads dz as a split image (a consumer that ran the activation backward may hand one over)."""
        return self.form in ('v2', 'v3')


class WgradPlan(NamedTuple):
    form: str                   # 'v2_up' | 'v2' | 'v2_slabs' | 'igemm'
    keep_ximg: bool             # the forward keeps its activation operand image for this launch
    precision: str              # arithmetic of the launch ('f32' when the range of dz is not known)


def plan_forward(N, Ci, Co, Hi, Wi, k, up, prec, frozen) -> ForwardPlan:
    """Launch form of the forward of a k x k layer Ci -> Co on an Hi x Wi input (up 2: stride-2 transposed conv to (2 Hi + 1) x (2 Wi + 1), then the FIR
    epilogue).  frozen: the weights carry no gradient (the weight-streaming kernel reads a split weight image, re-made every step otherwise)."""
    fp16 = presplit_arith(prec)
    if up == 1:
        cls = H.classes_corr(Hi, Wi, k, k, k // 2)
        ks = _auto_ksplit(cls, N, Co, Ci)
        # under-filled 3x3 grids (64^2 x 512, 32^2 x 512 at one image): the wave-split kernel, fused epilogue, no zero fill / atomics / finishing pass
        v3 = H.conv_v3_plan(Ci, Co, cls, N) if fp16 else None
        if v3:
            return ForwardPlan('v3', True, False, v3=v3)
        rows = H.conv_v2_rows(Ci, Co, cls, N) if (H.USE_V2 and fp16 and ks == 1) else 0
        if rows:
            return ForwardPlan('v2', True, False, rows=rows, rgb_head=bool(H.RGB_HEAD and Co == 128 and rows == 8))
        if ks == 1:
            return ForwardPlan('igemm', False, False)
        # 4^2 .. 16^2: one workgroup per (channel tile, 16-channel chunk), every weight byte fetched once, operand split inside (csrc/conv_ws.hip)
        if fp16 and frozen and H.conv_ws_ok(Ci, Co, cls, N, Hi, Wi):
            return ForwardPlan('ws', False, True)
        return ForwardPlan('igemm_splitk', False, True, ksplit=ks)
    # the four output parities of the transposed conv from one workgroup per input patch (csrc/conv_v2_up.hip)
    u = H.conv_up2_plan(Ci, Co, Hi, Wi, N) if (up == 2 and k == 3 and fp16) else None
    if u:
        return ForwardPlan('up2', True, True, ksplit=u[0], ragged=u[1], rows=u[2])
    ks = _auto_ksplit(H.classes_convT(Hi, Wi, k, k, up)[0], N, Co, Ci)
    if ks == 1:
        return ForwardPlan('igemm_up', False, True)
    # 4^2 / 8^2 input cells: the weight-streaming kernel's transposed form (four parity accumulator sets per wave, csrc/conv_ws.hip)
    if up == 2 and k == 3 and fp16 and frozen and H.conv_ws_up_ok(Ci, Co, N, Hi, Wi):
        return ForwardPlan('ws_up', False, True)
    return ForwardPlan('igemm_splitk', False, True, ksplit=ks)


def consumer_reads_split(N, C, H_, W_, prec) -> bool:
    """A 3x3 layer C -> C on an H_ x W_ grid runs on the pre-split kernel: the up layer that produces its input may write the operand image
    from its own epilogue."""
    return bool(presplit_arith(prec) and H.USE_V2 and H.conv_v2_supported(C, C, H.classes_corr(H_, W_, 3, 3, 1), N))


def _fir_split(N, Ci, Co, Hi, Wi, k, up, fp16, need_dx, need_w) -> bool:
    """An up layer's backward takes the FIR adjoint that writes parity-split fp16 images when every launch that reads the gradient operand
    (data gradient: conv_v2_s2adj / conv_v3_s2adj, weight gradient: conv_wgrad_v2_up) has its parity-split form for this geometry."""
    return bool((need_dx or need_w) and up == 2 and k == 3 and fp16
                and (not need_dx or H.conv_s2adj_ok(Co, Ci, Hi, Wi, N) or H.conv_v3_s2adj_ok(Co, Ci, Hi, Wi, N))
                and (not need_w or H.conv_wgrad_v2_up_ok(Ci, Co, Hi, Wi, N)))


def plan_dgrad(N, Ci, Co, Hi, Wi, k, up, prec, frozen, amax_known=True, need_dx=True, need_w=False) -> DgradPlan:
    """Launch form of the data (+ style) gradient of the same layer: a Co -> Ci convolution onto the Hi x Wi input grid.
    amax_known: max|dz| is at hand (the range normalisation of the fp16 operand image); need_dx / need_w: which gradients this backward
    computes -- they decide the FIR adjoint of an up layer, whose output both launches read."""
    fp16 = presplit_arith(prec) and amax_known
    fir_split = _fir_split(N, Ci, Co, Hi, Wi, k, up, fp16, need_dx, need_w)
    if not need_dx:
        return DgradPlan(None, fir_split)
    if fir_split:
        return DgradPlan('s2adj' if H.conv_s2adj_ok(Co, Ci, Hi, Wi, N) else 'v3_s2adj', True)
    cls = H.classes_corr_adjoint(Hi, Wi, k, k, k // 2) if up == 1 else H.classes_convT_adjoint(Hi, Wi, k, k, up)
    ks = _auto_ksplit(cls, N, Ci, Co)
    if up == 1 and fp16:
        rows = H.conv_v2_rows(Co, Ci, cls, N) if (H.USE_V2 and ks == 1) else 0
        if rows:
            return DgradPlan('v2', False, rows=rows)
        # under-filled 3x3 grid: data gradient, style gradient and the producer's activation backward from one launch of the wave-split kernel
        v3 = H.conv_v3_plan(Co, Ci, cls, N)
        if v3:
            return DgradPlan('v3', False, v3=v3)
    if ks == 1:
        return DgradPlan('igemm', False)
    # low resolution: split K over blocks, then scale / reduce in a finishing pass
    if up == 1 and fp16 and frozen and H.conv_ws_ok(Co, Ci, cls, N, Hi, Wi):
        return DgradPlan('ws', False, finish=True)
    if up == 2 and k == 3 and fp16 and frozen and H.conv_ws_ok(Co, Ci, cls, N, Hi, Wi, in_stride=2):
        return DgradPlan('ws_s2', False, finish=True)
    return DgradPlan('igemm_splitk', False, finish=True, ksplit=ks)


def plan_wgrad(N, Ci, Co, Hi, Wi, k, up, prec, amax_known=True, need_dx=True, fwd: Optional[ForwardPlan] = None) -> WgradPlan:
    """Launch form of the weight gradient (trainable weights: pivotal tuning).  It reads the operand images the other two passes made where it
    can: X from the forward (keep_ximg), G from the data gradient or the parity-split FIR adjoint.  fwd: the layer's forward plan when the
    caller has it at hand (it is computed otherwise)."""
    fp16 = presplit_arith(prec) and amax_known
    fwd = fwd or plan_forward(N, Ci, Co, Hi, Wi, k, up, prec, False)
    keep = bool(fwd.presplit and H.WGRAD_V2 and Ci % 64 == 0 and Co % 64 == 0)
    wprec = prec if fp16 else 'f32'
    if up == 2 and _fir_split(N, Ci, Co, Hi, Wi, k, up, fp16, need_dx, True):
        return WgradPlan('v2_up', keep, wprec)
    if up == 1 and keep and fp16 and H.conv_wgrad_v2_shapes_ok((N, Co, Hi, Wi), (N, Ci, Hi, Wi), H.classes_corr(Hi, Wi, k, k, k // 2)):
        return WgradPlan('v2_slabs' if H.WGRAD_SLABS else 'v2', keep, wprec)
    return WgradPlan('igemm', keep, wprec)


def describe(N, Ci, Co, Hi, Wi, k, up, prec, frozen) -> dict:
    """The plans of one layer as plain data (a row of tests/golden/conv_routes.json): forward and data gradient, and for trainable
    weights the weight gradient."""
    geom = (N, Ci, Co, Hi, Wi, k, up, prec)
    return dict(forward=plan_forward(*geom, frozen)._asdict(), dgrad=plan_dgrad(*geom, frozen, need_w=not frozen)._asdict(),
                wgrad=None if frozen else plan_wgrad(*geom)._asdict())
