/*
 * eg3d_hip.h -- C-ABI of libeg3d_hip.so: the MI355X (gfx950) native hot path of EG3D inversion
 * (TriPlaneGenerator.synthesis forward + backward).  Drop-in boundary for the reference's three JIT-built
 * pybind11 CUDA plugins and for the ATen/cuDNN kernels under G.synthesis.
 *
 * Conventions:
 *   - extern "C", plain device pointers + sizes; no torch / C++ types cross the boundary.
 *   - every entry takes the hipStream_t to launch on (as void*), allocates nothing (the caller owns all
 *     buffers, including workspaces), keeps no global mutable state (re-entrant, multi-stream safe).
 *     ONE exception, in the deterministic build only (libeg3d_hip_det.so, -DEG3D_DET=1; csrc/det.h): the exact accumulators live in a
 *     workspace the caller lends with eg3d_det_set_workspace(), and the table of a call's accumulation targets is one process-global
 *     device object updated in stream order -- that build is single-stream and not re-entrant ("Deterministic build").
 *   - return value: 0 = ok, <0 = invalid argument / unsupported configuration (EG3D_ERR_*),
 *     >0 = hipError_t of a failed launch.  No exceptions.
 *   - tensors are fp32 unless a `dtype` argument says otherwise (EG3D_F32 / EG3D_F16 / EG3D_F64).
 *   - activations on the fused path are NHWC ("channels_last"): element (n,y,x,c) at ((n*H+y)*W+x)*ld + c.
 *
 * Each group cites the reference interface it replaces (paths relative to the reference repo root).
 */
#ifndef EG3D_HIP_H
#define EG3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_OK 0
#define EG3D_ERR_INVALID (-1)      /* bad argument (null pointer, negative size, ...) */
#define EG3D_ERR_UNSUPPORTED (-2)  /* valid request this build has no kernel for        */
#define EG3D_ERR_TOO_LARGE (-3)    /* exceeds int32 indexing, as the reference checks   */
#define EG3D_ERR_WORKSPACE (-4)    /* deterministic build: the call's accumulation targets do not fit the lent workspace */

#define EG3D_F32 0
#define EG3D_F16 1
#define EG3D_F64 2

/* activation ids == the reference's cuda_idx (torch_utils/ops/bias_act.py:23-33) */
#define EG3D_ACT_LINEAR 1
#define EG3D_ACT_RELU 2
#define EG3D_ACT_LRELU 3
#define EG3D_ACT_TANH 4
#define EG3D_ACT_SIGMOID 5
#define EG3D_ACT_ELU 6
#define EG3D_ACT_SELU 7
#define EG3D_ACT_SOFTPLUS 8
#define EG3D_ACT_SWISH 9

int eg3d_abi_version(void);
const char* eg3d_status_string(int status);

/* ------------------------------------------------------------------------------------------------
 * bias_act -- replaces bias_act_plugin.bias_act(x,b,xref,yref,dy,grad,dim,act,alpha,gain,clamp)
 *   torch_utils/ops/bias_act.cpp:36-94 (host), bias_act.cu:27-151 (kernel), bound at bias_act.cpp:100.
 *   grad=0: y = clamp(act(x + b[(i/step_b) % size_b]) * gain)
 *   grad=1: x := incoming dy; y = dx  (uses yref, or xref+b for swish); zero where |yref| >= clamp
 *   grad=2: x := incoming d_dx; `dy` = first-order dy; y = d_x (2nd-order term)
 *   Any dense layout: flat index, bias index from step_b = x.stride(dim)  (bias_act.cpp:77).
 *   Null pointers stand for the reference's empty tensors.  clamp < 0 disables clamping.
 */
int eg3d_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy, void* y,
                  int dtype, int64_t numel, int size_b, int step_b, int grad, int act, float alpha, float gain,
                  float clamp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * upfirdn2d -- replaces upfirdn2d_plugin.upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)
 *   torch_utils/ops/upfirdn2d.cpp:20-102 (host), upfirdn2d.cu:33-204 (kernels), bound at upfirdn2d.cpp:108.
 *   x: [N,C,inH,inW] with arbitrary element strides xs[4] (NCHW or channels_last); f: fp32 [fH,fW] contiguous;
 *   y: [N,C,outH,outW] with strides ys[4];  outW = (inW*upx + padx0 + padx1 - fW + downx) / downx.
 *   Backward w.r.t. x is the same entry with up<->down, !flip and the padding of upfirdn2d.py:258-268.
 */
int eg3d_upfirdn2d(const void* x, const float* f, void* y, int dtype, int N, int C, int inH, int inW,
                   const int64_t xs[4], int fH, int fW, int upx, int upy, int downx, int downy, int padx0,
                   int padx1, int pady0, int pady1, int flip, float gain, int outH, int outW,
                   const int64_t ys[4], void* stream);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, fp32 in / fp32 out, products on the matrix cores in the arithmetic `precision` selects (exact fp32 MFMA
 * or 16-bit MFMA products of operand pieces: EG3D_PREC_* below) -- replaces the ATen/cuDNN calls made by
 * conv2d_resample / modulated_conv2d (torch_utils/ops/conv2d_resample.py:31-43,114-136;
 * training/networks_stylegan2.py:34-91) and their autograd backward (the dX contract of
 * torch_utils/ops/conv2d_gradfix.py:139-143).  One launch computes, for every output-grid cell (n,ay,ax):
 *     acc[n,ay,ax,o] = sum_t sum_k  in_scale[n,k] * x[n, ay*in_stride+dy[t], ax*in_stride+dx[t], k] * w[o, wtap[t], k]
 * and applies one of the epilogues below at out[n, ay*out_stride+out_py, ax*out_stride+out_px, o].
 * The tap list expresses: 3x3 / 1x1 correlation (forward), the four parity classes of a stride-2 transposed
 * conv (forward of up=2 layers), the stride-2 correlation (their data gradient) and the flipped 3x3 (data gradient
 * of plain layers).  Up to 4 classes (tap lists + output grids) run in one launch.
 */
#define EG3D_EPI_STORE 0   /* out = acc                                                                  */
#define EG3D_EPI_ATOMIC 1  /* out += acc  (split-K; out must be pre-zeroed)                               */
#define EG3D_EPI_FWD 2     /* out = clamp(act(acc*out_scale[n,o] + noise[n,y,x]*strength + bias[o])*gain) (+ addend); act: linear | relu | lrelu */
#define EG3D_EPI_BWD 3     /* ds[n,o] += sum_px acc*xin ; out = acc*out_scale[n,o] (+ addend)             */
#define EG3D_EPI_BWD_ACT 4 /* EPI_BWD followed, in the same epilogue, by the activation backward of the layer that PRODUCED xin
                            * (eg3d_act_bwd below): the value EPI_BWD would store is that layer's dout, xin is its saved output, so
                            *   dy = dout * act'(xin) * gain (0 where |xin| >= clamp);  out = dy * d[n,o];  + the reductions of
                            * eg3d_modconv_epilogue_bwd.  Saves that pass: dout is never written, xin is read once.           */

/* The producing layer's activation backward for EG3D_EPI_BWD_ACT (same contract as eg3d_modconv_epilogue_bwd: linear / lrelu, reduction
 * targets pre-zeroed and accumulated with atomics; every pointer optional). */
typedef struct eg3d_act_bwd {
    const float* d;            /* [N,Nc] demodulation coefficients of that layer (out = dy * d), or null */
    const float* bias;         /* [Nc] or null                                                          */
    const float* noise;        /* [*,Ho,Wo] or null; batch stride noise_nstride (0 = shared)            */
    int64_t noise_nstride;
    const float* noise_strength;
    int32_t act;
    float alpha, gain, clamp;
    float* dbias;              /* [Nc]   += sum dy                                                      */
    float* dd;                 /* [N,Nc] += sum_px dy * (pre_act - bias - noise*strength) / d            */
    float* dnoise;             /* [*,Ho,Wo] += strength * sum_c dy; batch stride dnoise_nstride          */
    int64_t dnoise_nstride;
    float* dstrength;          /* scalar += sum dy * noise                                              */
} eg3d_act_bwd;

typedef struct eg3d_conv_class {
    int32_t Ha, Wa;            /* output grid of this class                              */
    int32_t out_py, out_px;    /* output pixel = (ay*out_stride + out_py, ax*out_stride + out_px) */
    int32_t ntaps;
    int32_t dy[9], dx[9];      /* input pixel  = (ay*in_stride + dy[t], ax*in_stride + dx[t]); OOB reads are zero */
    int32_t wtap[9];           /* weight tap index of tap t                              */
} eg3d_conv_class;

/* Arithmetic of the implicit GEMM.  Operands, accumulators and results are fp32 in every mode.
 *   F32     v_mfma_f32_32x32x2_f32, exact fp32 products.
 *   BF16X6  each operand cut into 3 bf16 terms (x = b0+b1+b2, exact to 2^-24), six bf16 MFMA products accumulated in fp32;
 *           the dropped cross terms are < 2^-23 relative per product, i.e. fp32-equivalent (below fp32 accumulation error).
 *   BF16X3  three products (b0b0+b0b1+b1b0), relative error < 2^-15 per product (between TF32 and fp32).
 *   F16X3   each operand cut into 2 fp16 terms (x = h+l; residual <= max(2^-22 |x|, 2^-25)), three fp16 MFMA products (hh+hl+lh)
 *           accumulated in fp32: fp32-like for operands of magnitude ~2^-4 .. 2^16; operands outside that range must be brought
 *           into it by the caller with a power-of-two `a_scale` (the result is rescaled exactly). */
enum { EG3D_PREC_F32 = 0, EG3D_PREC_BF16X6 = 1, EG3D_PREC_BF16X3 = 2, EG3D_PREC_F16X3 = 3,
       /* F16X1: the high fp16 piece of each (range-normalised) operand only, ONE product, fp32 accumulation and fp32 results -- the
        * arithmetic of the reference's own fp16 layers (SynthesisBlock with use_fp16 and force_fp32=False, networks_stylegan2.py:421-424:
        * the super-resolution head during pivotal tuning), with operands rounded to fp16 (rel. 2^-11) but nothing stored in fp16. */
       EG3D_PREC_F16X1 = 4 };

typedef struct eg3d_conv_params {
    const float* x;            /* [N,Hi,Wi,ldx] NHWC, Ck used channels                   */
    const float* w;            /* w[o*w_row + tap*Ck + k]                                */
    float* out;                /* [N,Ho,Wo,ldo] NHWC, Nc used channels                   */
    int32_t N, Hi, Wi, Ck, ldx;
    int32_t Nc, w_row;
    int32_t Ho, Wo, ldo;
    int32_t in_stride, out_stride;
    int32_t ncls;
    eg3d_conv_class cls[4];
    const float* in_scale;     /* [N,Ck] or null                                         */
    int32_t epi;
    int32_t ksplit;            /* >=1; >1 only with EG3D_EPI_ATOMIC                      */
    const float* out_scale;    /* [N,Nc] or null                                         */
    const float* bias;         /* [Nc] or null                                           */
    const float* noise;        /* [*,Ho,Wo] or null; batch stride noise_nstride (0 = shared) */
    int64_t noise_nstride;
    const float* noise_strength; /* device scalar (may be null when noise is null)       */
    int32_t act;
    float alpha, gain, clamp;
    const float* addend;       /* [N,Ho,Wo,ldo] or null; may alias out                   */
    const float* xin;          /* EPI_BWD: [N,Ho,Wo,ldo] layer input for the style-gradient reduction, or null */
    float* ds;                 /* EPI_BWD: [N,Nc] accumulated with atomics (pre-zeroed), or null */
    int32_t precision;         /* EG3D_PREC_*: how the fp32 products are formed on the matrix cores */
    const float* a_amax;       /* F16X3 only, optional: device scalar max|x| of the A operand; the kernel multiplies A by the power of
                                * two that brings a_amax * a_amax_mul to ~2^14 and divides the result by it (exact).  null = none. */
    float a_amax_mul;
    int32_t ds_replicas;       /* EPI_BWD: ds is [ds_replicas][N,Nc]; workgroup b accumulates into replica b % ds_replicas so that
                                * thousands of tiles do not serialise on the same N*Nc addresses; the caller sums the replicas.
                                * 0 or 1 = a single [N,Nc] buffer. */
    float* out_amax;           /* optional, pre-zeroed device scalar: receives max|out| (atomic max; EPI_STORE / FWD / BWD) -- the operand
                                * range a consumer needs to range-normalise its two-piece fp16 split */
    eg3d_act_bwd act_bwd;      /* EG3D_EPI_BWD_ACT only (xin required; vector epilogue only: eg3d_conv2d_igemm_act_bwd_ok) */
    int32_t w_presplit;        /* F16X3 only: w is the image written by eg3d_split_weight_pieces (same indexing as the fp32 matrix; w_row and
                                * Ck multiples of 4): the loader copies the two fp16 pieces instead of forming them -- the weight-side half of
                                * the split arithmetic, which this kernel is bound by, is then done once per weight instead of once per
                                * workgroup and K-step.  Same bits, same results. */
    int32_t addend_up2;        /* EPI_FWD, vector epilogue, one class, even Ho / Wo: `addend` is the HALF-resolution image [N,Ho/2,Wo/2,ldo] and
                                * what is added is upfirdn2d.upsample2d(addend) with the separable 4-tap filter addend_taps (taps already
                                * normalised and multiplied by the per-axis gain 2): the skip image of the 'skip' architecture
                                * (networks_stylegan2.py:433-436) is up-sampled inside the toRGB launch instead of by its own pass.
                                * EG3D_ERR_UNSUPPORTED when the conditions do not hold. */
    float addend_taps[4];
} eg3d_conv_params;

/* 1 when this launch can run EG3D_EPI_BWD_ACT (aligned rows, channel counts that are multiples of 4, no split-K, tiles within one
 * image); otherwise run EG3D_EPI_BWD and eg3d_modconv_epilogue_bwd separately. */
int eg3d_conv2d_igemm_act_bwd_ok(const eg3d_conv_params* p);

int eg3d_conv2d_igemm_f32(const eg3d_conv_params* p, void* stream);
/* image[4j .. 4j+3] (16 bytes) = the four high fp16 pieces of w[4j .. 4j+3] followed by their four low pieces (h = rtz16(w),
 * l = rne16(w - h)): the operand image eg3d_conv_params::w_presplit expects.  n floats, n % 4 == 0, both pointers 16-byte aligned. */
int eg3d_split_weight_pieces(const float* w, void* image, int64_t n, void* stream);
/* Which tile configuration eg3d_conv2d_igemm_f32 will launch for p: 0 = 128x128x32 (the dominant kernel), 1 = 64x128,
 * 2 = 32x128, 3 = 128x32.  Pure host function (used by bench.py to attribute launch times to kernels). */
int eg3d_conv2d_igemm_config(const eg3d_conv_params* p);

/* ------------------------------------------------------------------------------------------------
 * Pre-split implicit-GEMM convolution (csrc/conv_v2.hip): same contract as eg3d_conv2d_igemm_f32 in F16X3 arithmetic -- one launch
 * computes, for every cell of every class grid,
 *     acc[n,ay,ax,o] = sum_t sum_k  A[n, ay+dy[t], ax+dx[t], k] * W[o, wtap[t], k]            (in_stride 1; OOB reads are zero)
 * and applies epilogue STORE / ATOMIC / FWD / BWD (as above) at out[n, ay*out_stride+out_py, ax*out_stride+out_px, o] -- but both operands are
 * "split images" prepared once by eg3d_split_activation / eg3d_split_weight (two fp16 pieces per value, see conv_v2.hip), so the
 * style modulation, the range normalisation and the fp32 -> 2 x fp16 split are NOT repeated per tile and per tap:
 *   A image [N][2][Ck/8][Hi][Wi][8] fp16 = split( x * in_scale[n,k] * a_scale ),  a_scale = the power of two that brings
 *           max|x| * max|in_scale| to [2^13, 2^14)  (device scalar written by eg3d_split_activation);
 *   W image [wtaps][Ck/16][2][2][Nc][8] fp16 = split( w[o, tap, k] * w_scale )    (eg3d_split_weight; cached per weight version).
 * The result is divided by a_scale * w_scale in the epilogue (exact).  out_amax (optional, pre-zeroed device scalar) receives
 * max|out| (atomic max): the operand range of the next layer's split.
 * Restrictions (eg3d_conv2d_v2_supported): Ck % 16 == 0, Nc % 128 == 0, in_stride 1, classes of 9 / 4 / 2 / 1 taps whose offsets span
 * at most 3 x 3, 16-byte aligned rows; everything else stays on eg3d_conv2d_igemm_f32. */
typedef struct eg3d_conv_v2_params {
    const void* a;  const void* w;
    const float* a_scale;  const float* w_scale;
    float* out;
    int32_t N, Hi, Wi, Ck;
    int32_t Nc, wtaps;
    int32_t Ho, Wo, ldo;
    int32_t in_stride, out_stride;
    int32_t ncls;
    eg3d_conv_class cls[4];
    int32_t epi;
    const float* out_scale;  const float* bias;  const float* noise;
    int64_t noise_nstride;
    const float* noise_strength;
    int32_t act;
    float alpha, gain, clamp;
    const float* addend;  const float* xin;
    float* ds;
    float* out_amax;
    eg3d_act_bwd act_bwd;      /* EG3D_EPI_BWD_ACT only */
    int32_t products;          /* 0 / 3: three products (fp32-equivalent);  1: high pieces only (EG3D_PREC_F16X1)            */
    int32_t ksplit;            /* 0 / 1: none.  > 1 (EG3D_EPI_ATOMIC only, `out` pre-zeroed): the contraction's 16-channel chunks are split over
                                * ksplit workgroups per tile which add their partial tiles with fp32 atomics -- the layers whose grids
                                * cannot fill the chip (128^2 x 256: 128 tiles; 64^2 x 512: 64).
                                * 2 with a fused (non-atomic) epilogue and patch_rows == 4 (Ck / 16 even and >= 4, no rgb_out): the split stays INSIDE
                                * the workgroup -- eight waves, each four-wave half takes half of the chunks and the halves meet in LDS before the
                                * epilogue: for 4-row grids that give every CU at most one workgroup (two waves per SIMD instead of one).  Same
                                * result as ksplit 0 up to the rounding of one extra sum per element; no zero fill, nothing leaves the workgroup */
    int32_t patch_rows;        /* 0 / 8: workgroup tile = 8 x 32 cells x 128 channels.  4: 4 x 32 cells -- twice the workgroups for 3x3 layers whose
                                * 8-row grid leaves CUs idle, fused epilogues intact (nine-tap classes, not with EG3D_EPI_ATOMIC) */
    /* Optional 1x1 head on the finished tile (eg3d_conv2d_v2 with EG3D_EPI_FWD, Nc == 128 = one channel tile per cell, one nine-tap class,
     * patch_rows 0 / 8): the toRGB layer
     * that reads this layer's output next (training/networks_stylegan2.py:338-359, the super-resolution head's last block) evaluated while the
     * output values are still in registers instead of by a launch that reads the tensor again --
     *     rgb_out[n,y,x,o] = clamp(sum_c out[n,y,x,c] * rgb_w[o * rgb_ldw + c] * rgb_s[n * Nc + c] + rgb_bias[o], +-rgb_clamp),  o = 0 .. 3
     * (exact fp32 multiply-adds; rgb_w: four rows, zero rows for padding channels; rgb_bias may be null; rgb_clamp < 0: none).  rgb_out null: off. */
    const float* rgb_w;  const float* rgb_s;  const float* rgb_bias;
    float* rgb_out;            /* [N,Ho,Wo,4] */
    float rgb_clamp;
    int32_t rgb_ldw;
    int32_t rgb_nout;          /* 0 / 4: four outputs; 3: the fourth row of rgb_w is a zero padding row (a hint: the result is the same) */
} eg3d_conv_v2_params;
int eg3d_conv2d_v2_supported(const eg3d_conv_v2_params* p);
int eg3d_conv2d_v2(const eg3d_conv_v2_params* p, void* stream);
/* Wave-split form of that convolution (csrc/conv_v3.hip) for the nine-tap layers whose grids cannot fill the chip with 256-cell x 128-channel
 * tiles (64^2 x 512, 32^2 x 512, and the 128^2 / 256^2 backbone layers at one image per GPU; training/networks_stylegan2.py:34-91,417-461): same
 * operand images, contract and epilogues (STORE / FWD / BWD / BWD_ACT) as eg3d_conv2d_v2, but a workgroup tile is r x 32 cells x 64 channels
 * (r = p->patch_rows: 0 / 4 | 2) and the contraction is split over the w waves of the workgroup (w = p->ksplit: 0 / 4 | 8; 8 only with r = 2)
 * and summed in LDS in wave order -- no atomics, zero fill, slabs or finishing pass; run-to-run deterministic.  The waves share nothing in the
 * main loop (private LDS halo per wave by LDS-DMA, weight fragments straight from global memory into registers): no barrier in it.
 * Restrictions (eg3d_conv2d_v3_supported): Ck % 16 == 0, Nc % 64 == 0, in_stride 1, nine-tap classes spanning at most 3 x 3. */
int eg3d_conv2d_v3_supported(const eg3d_conv_v2_params* p);
int eg3d_conv2d_v3(const eg3d_conv_v2_params* p, void* stream);
/* Weight-streaming split-K form (csrc/conv_ws.hip) for the 3x3 stride-1 layers of the 4^2 .. 16^2 blocks at one image per GPU (16 .. 256 cells x
 * 512 -> 512: 9.4 MB of weights for <= 1.2 GFLOP; forward and data gradient of training/networks_stylegan2.py:34-91): EG3D_EPI_ATOMIC's contract --
 *     out[n, y, x, o] += sum_t sum_k  x[n, y + dy[t], x + dx[t], k] * in_scale[n, k] * W[o, wtap[t], k]        (out pre-zeroed, fp32, NHWC)
 * with one workgroup per (32-channel tile, four 16-channel chunks of the contraction -- one per wave, summed in LDS in wave order --, block of
 * <= 256 cells): every byte of the weight image is fetched by exactly one wave, all of its loads are in flight before its first matrix
 * instruction, and the fp32 activation is modulated, range-normalised (x_amax * x_amax_mul * max|in_scale|) and split into the two fp16 pieces inside the kernel (no operand pass).
 * Arithmetic of eg3d_conv2d_v2 (w: the weight image of eg3d_split_weight, w_scale its scale).  W <= 32, |dy|, |dx| <= 1, Ck % 16 == 0,
 * Nc % 32 == 0, ldx % 4 == 0. */
typedef struct eg3d_conv_ws_params {
    const float* x;            /* [N,H,W,ldx] fp32 */
    const float* in_scale;     /* [N,Ck] or null */
    const float* x_amax;       /* device scalar: max|x| (or a bound) */
    float x_amax_mul;
    const void* w;  const float* w_scale;
    float* out;                /* [N,H,W,ldo] fp32, accumulated with atomics */
    int32_t N, H, W, Ck, ldx;
    int32_t Nc, ldo, wtaps;
    int32_t dy[9], dx[9], wtap[9];
    int32_t products;          /* 0 / 3 | 1 */
    int32_t in_stride;         /* 0 / 1: correlation, |dy|, |dx| <= 1, x is [N,H,W,ldx].  2: the stride-2 adjoint (data gradient of the up layers):
                                * out[n,a,b,o] += sum x[n, 2a + dy[t], 2b + dx[t], k] ..., dy, dx in 0 .. 2, x is [N,Hx,Wx,ldx] (zeros beyond it),
                                * H * W <= 256 output cells */
    int32_t Hx, Wx;            /* in_stride 2 only */
    int32_t out_stride;        /* 0 / 1.  2: the stride-2 TRANSPOSED conv (forward of an up layer, in_stride <= 1): x is [N,H,W,ldx], out is
                                * [N, 2H + 1, 2W + 1, ldo], out[n, 2a + ky, 2b + kx, o] += x[n,a,b,k] in_scale[n,k] W[o, wtap[3 ky + kx], k]  (dy, dx unused);
                                * (H + 1)(W + 1) <= 96 */
} eg3d_conv_ws_params;
int eg3d_conv2d_ws_supported(const eg3d_conv_ws_params* p);
int eg3d_conv2d_ws(const eg3d_conv_ws_params* p, void* stream);
/* Data gradient of that transposed convolution (a stride-2 3x3 correlation; csrc/conv_v2_s2adj.hip) with the contract, epilogues and
 * weight image of eg3d_conv2d_v2, for ONE class of nine taps (dy, dx) = (t / 3, t % 3):
 *     acc[n,a,b,o] = sum_t sum_k  G[n, 2a + dy[t], 2b + dx[t], k] * W[o, wtap[t], k]
 * where the A operand is the PARITY-split image of G written by eg3d_fir44_adjoint_split: [N][2][Ck/8][4][Hi][Wi][8] fp16 with
 * parity image (py, px)[a', b'] = G[2a' + py, 2b' + px] (p->Hi, p->Wi = dimensions of one parity image, >= Ha + 1, Wa + 1). */
int eg3d_conv2d_v2_s2adj_supported(const eg3d_conv_v2_params* p);
int eg3d_conv2d_v2_s2adj(const eg3d_conv_v2_params* p, void* stream);
/* The same data gradient, same operands and epilogues (STORE / BWD / BWD_ACT), in the wave-split decomposition of eg3d_conv2d_v3 for the layers
 * whose grids cannot fill the chip with 256 x 128 tiles (the backbone's up layers at one image per GPU): 128-cell x 64-channel tiles, the
 * contraction -- the list of (parity image, 16-channel chunk) items with 4 / 2 / 2 / 1 taps -- dealt to the four waves of a workgroup in runs of
 * equal cost and summed in LDS in wave order (csrc/conv_v3.hip).  Nc % 64 == 0, Ck % 16 == 0; taps (dy, dx) = (t / 3, t % 3) as above. */
int eg3d_conv2d_v3_s2adj_supported(const eg3d_conv_v2_params* p);
int eg3d_conv2d_v3_s2adj(const eg3d_conv_v2_params* p, void* stream);
/* FIR adjoint of an up-sampling layer fused with the operand split: G = upfirdn2d(dz, outer([1,3,3,1]) / 64, padding 2, gain) of
 * dz [N, 2 Hi, 2 Wi, ldz] NHWC fp32 (C used channels, C % 8 == 0) -- the (2 Hi + 1) x (2 Wi + 1) input of the data gradient above
 * (torch_utils/ops/upfirdn2d.py:258-268 applied to conv2d_resample.py:129) -- written as the four parity images [.][Hi + 1][Wi + 1] in the
 * split layout, range-normalised by the bound max|G| <= gain * max|dz| (dz_amax: device scalar max|dz|).  image:
 * eg3d_fir44_adjoint_split_bytes() bytes; scale_out: device scalar (the image's power-of-two scale).  C % 64 == 0 and
 * eg3d_fir44_adjoint_split_bytes(1, Hi, Wi, C) <= 0x7fffffe0 (EG3D_ERR_UNSUPPORTED otherwise). */
int64_t eg3d_fir44_adjoint_split_bytes(int N, int Hi, int Wi, int C);
int eg3d_fir44_adjoint_split(const float* dz, const float* dz_amax, void* image, float* scale_out, int N, int Hi, int Wi, int C, int ldz, float gain,
                             void* stream);
/* Stride-2 3x3 TRANSPOSED convolution on the same split images, all four output parities per workgroup (csrc/conv_v2_up.hip) -- the
 * F.conv_transpose2d of the up-sampling layers (torch_utils/ops/conv2d_resample.py:114-136):
 *     out[n, 2a + py, 2b + px, o] (+)= sum over taps t = 3 ky + kx with ky % 2 == py, kx % 2 == px of
 *                                     A[n, a - ky/2, b - kx/2, k] * W[o, wtap[t], k]                 (OOB reads are zero)
 * for the cells a < Hc, b < Wc (Hc <= Hi + 1, Wc <= Wi + 1) and the output pixels inside Ho x Wo (<= 2 Hi + 1, 2 Wi + 1).  With
 * Hc = Hi, Wc = Wi the launch covers rows / columns 0 .. 2 Hi - 1 / 2 Wi - 1 on perfectly tiled grids; the last output row and column
 * (a = Hi resp. b = Wi: 1-D problems) are then four small tap classes of eg3d_conv2d_igemm_f32.  epi: EG3D_EPI_STORE, or EG3D_EPI_ATOMIC
 * with ksplit workgroups per tile (out pre-zeroed).  Nc % 64 == 0, Ck % 16 == 0; W image with 9 taps. */
typedef struct eg3d_conv_up2_params {
    const void* a;  const void* w;
    const float* a_scale;  const float* w_scale;
    float* out;
    int32_t N, Hi, Wi, Ck, Nc;
    int32_t Hc, Wc;
    int32_t Ho, Wo, ldo;
    int32_t wtap[9];           /* weight tap index of (ky, kx) = (t / 3, t % 3)                                               */
    int32_t epi, products, ksplit;
    int32_t patch_rows;        /* 0 | 8: 8 x 32-cell patches, eight waves, one workgroup per CU; 4: 4 x 32 cells, four waves, tap-row weight ring, two per CU */
} eg3d_conv_up2_params;
int eg3d_conv2d_up2_supported(const eg3d_conv_up2_params* p);
int eg3d_conv2d_up2(const eg3d_conv_up2_params* p, void* stream);
/* Operand preparation.  x: NHWC fp32 [N,H,W,ldx] (C used channels, C % 8 == 0); in_scale [N,C] or null; x_amax / s_amax: device scalars
 * holding max|x| and max|in_scale| (s_amax null: computed from in_scale by the kernel); image: eg3d_split_activation_bytes() bytes; scale_out: device scalar. */
int64_t eg3d_split_activation_bytes(int N, int H, int W, int C);
int eg3d_split_activation(const float* x, const float* in_scale, const float* x_amax, const float* s_amax, void* image, float* scale_out,
                          int N, int H, int W, int C, int ldx, void* stream);
/* w: packed [O][T][I] fp32 with row stride w_row (the forward or adjoint image of eg3d_pack_conv_weight); image: O*T*I*4 bytes. */
int eg3d_split_weight(const float* w, const float* w_amax, void* image, float* scale_out, int O, int I, int T, int w_row, void* stream);
/* Up to EG3D_SPLIT_W_BATCH_MAX dense packed weight matrices (w_row = T * I) in two launches: max|w| into the pre-zeroed `amax` scalars, then
 * the images (pivotal tuning re-splits every weight once per step). */
#define EG3D_SPLIT_W_BATCH_MAX 24
typedef struct eg3d_split_w_item { const float* w; void* image; float* scale_out; float* amax; int32_t O, I, T, w_row; } eg3d_split_w_item;
typedef struct eg3d_split_w_batch { int32_t n; int32_t pad_; eg3d_split_w_item items[EG3D_SPLIT_W_BATCH_MAX]; } eg3d_split_w_batch;
int eg3d_split_weights_batched(const eg3d_split_w_batch* b, void* stream);
/* out (pre-zeroed device scalar) = max(out, max|x|) over n floats. */
int eg3d_absmax(const float* x, int64_t n, float* out, void* stream);

/* Weight-gradient GEMM (PTI phase: grads into generator weights, training/coaches/base_coach.py:96-99):
 *   dw[o, wtap[t], k] += sum_{n,ay,ax} g[n, ay*out_stride+out_py, ax*out_stride+out_px, o]
 *                                       * in_scale[n,k] * x[n, ay*in_stride+dy[t], ax*in_stride+dx[t], k]
 * Same class/tap description as the forward; dw must be pre-zeroed (split over pixels with atomics). */
typedef struct eg3d_wgrad_params {
    const float* x;  const float* g;  float* dw;
    int32_t N, Hi, Wi, Ck, ldx;
    int32_t Nc, w_row;
    int32_t Ho, Wo, ldg;
    int32_t in_stride, out_stride;
    int32_t ncls;
    eg3d_conv_class cls[4];
    const float* in_scale;     /* [N,Ck] or null */
    int32_t psplit;            /* number of pixel slices */
    int32_t precision;         /* EG3D_PREC_F32 (v_mfma_f32_32x32x2_f32), EG3D_PREC_F16X3 (two fp16 pieces per operand, three products) or EG3D_PREC_F16X1 */
    const float* g_amax;       /* F16X3: optional device scalar max|g|; g is scaled by the power of two that brings g_amax * g_amax_mul */
    float g_amax_mul;          /*        to ~2^13 and the result is scaled back (exact).  null = g is used as it is.                   */
} eg3d_wgrad_params;

int eg3d_conv2d_wgrad_f32(const eg3d_wgrad_params* p, void* stream);
/* n launches of eg3d_conv2d_wgrad_f32 (F16X3 / F16X1 only) as ceil(n / EG3D_WGRAD_BATCH_MAX) launches: the weight gradients of a backward
 * pass are independent of each other, and the small layers' launches (a few dozen workgroups, 10 - 25 us) fill the chip only together. */
#define EG3D_WGRAD_BATCH_MAX 5
int eg3d_conv2d_wgrad_batched(const eg3d_wgrad_params* items, int n, void* stream);

/* The same weight gradient for stride-1 layers whose two operands already exist as split images (csrc/conv_wgrad_v2.hip): g = the image of
 * the gradient operand dz [N][2][Co/8][H][W][8] fp16 (what the data gradient of eg3d_conv2d_v2 consumes), x = the image of the layer input
 * times its styles [N][2][Ci/8][H][W][8] (what its forward consumed), both written by eg3d_split_activation or a fused producer:
 *     dw[o, wtap[t], k] += 1 / (g_scale x_scale) * sum_{n,y,x} G[n,y,x,o] * X[n, y + dy[t], x + dx[t], k]        (OOB reads are zero)
 * for ntaps = 9 (3x3, dy / dx in -1 .. 1) or 1.  LDS-DMA staging, transposing LDS reads (ds_read_b64_tr_b16), no per-element VALU work.
 * Co, Ci multiples of 64; dw pre-zeroed (partial tiles are accumulated with atomics).  products: 0 / 3 three products, 1 high pieces only.
 * row_groups: 0 = chosen by the library (about two workgroups per CU). */
typedef struct eg3d_wgrad_v2_params {
    const void* g;  const void* x;
    const float* g_scale;  const float* x_scale;
    float* dw;
    int32_t N, H, W, Co, Ci, w_row;
    int32_t ntaps;
    int32_t dy[9], dx[9], wtap[9];
    int32_t products, row_groups;
    int32_t slabs;             /* 0: partial tiles are ADDED to dw [Co][w_row] with fp32 atomics (dw pre-zeroed).  != 0: no atomics -- workgroup j of a
                                * channel tile STORES its partial tile into slab j of dw [nslab][Co][w_row] (nslab = eg3d_conv2d_wgrad_v2_slabs(p),
                                * every slab fully written, nothing to pre-zero) and the caller sums the slabs in order
                                * (eg3d_weight_grad_finish_slabs): run-to-run deterministic, and cheaper than ~19 M atomics per launch */
} eg3d_wgrad_v2_params;
int eg3d_conv2d_wgrad_v2_supported(const eg3d_wgrad_v2_params* p);
int eg3d_conv2d_wgrad_v2_slabs(const eg3d_wgrad_v2_params* p);      /* number of slabs (= workgroups per channel tile) the launch will write; < 0: error */
int eg3d_conv2d_wgrad_v2(const eg3d_wgrad_v2_params* p, void* stream);
/* The same for an UP-SAMPLING layer (stride-2 3x3 transposed conv, torch_utils/ops/conv2d_resample.py:114-136 under base_coach.py:96-99):
 *     dw[o, wtap[3 ky + kx], k] += 1 / (g_scale x_scale) * sum_{n,a,b} G_p[n, a + (ky >> 1), b + (kx >> 1), o] * X[n, a, b, k],  p = (ky & 1, kx & 1)
 * p->g = the PARITY-split image of the gradient operand as eg3d_fir44_adjoint_split writes it ([N][2][Co/8][4][H + 1][W + 1][8] fp16),
 * p->x = the split image of the layer input times its styles ([N][2][Ci/8][H][W][8]), H x W = the layer's INPUT resolution; ntaps = 9, dy / dx
 * ignored, slabs = 0 (partial tiles added with atomics: dw pre-zeroed). */
int eg3d_conv2d_wgrad_v2_up_supported(const eg3d_wgrad_v2_params* p);
int eg3d_conv2d_wgrad_v2_up(const eg3d_wgrad_v2_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tall-skinny Gram product for the decoder-weight gradients of pivotal tuning (training/triplane.py:116-136 under
 * base_coach.py:96-99):  out[i][j] += sum_s a[s][i]*b[s][j]  (Ka, Kb <= 64, row-major a [S,Ka], b [S,Kb]),
 * colsum[i] += sum_s a[s][i] (or null).  out / colsum must be pre-zeroed (accumulated with atomics).  Exact fp32 MFMA. */
int eg3d_rows_gram(const float* a, const float* b, int64_t S, int Ka, int Kb, float* out, float* colsum, void* stream);
/* ... with every partial sum multiplied by out_scale / colsum_scale before it is accumulated (the decoder's runtime weight gains: one launch
 * instead of the product + two scaling passes). */
int eg3d_rows_gram_scaled(const float* a, const float* b, int64_t S, int Ka, int Kb, float* out, float* colsum, float out_scale, float colsum_scale,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * filtered_lrelu -- replaces filtered_lrelu_plugin.filtered_lrelu / filtered_lrelu_act_ (torch_utils/ops/filtered_lrelu.cpp:20,217;
 * Python wrapper filtered_lrelu.py:161-274; slow reference :123-155).  Contiguous NCHW, fp32 or fp16 (float accumulation).
 *   t = gain1 * FIR_fu( zero_insert_up(x + b[c]) padded by (px0,px1,py0,py1) )                 size Hm x Wm
 *   a = mode 0: clamp(lrelu(t, slope) * gain)   [mask := da/dt written when mask != null]      mode 1: t * mask
 *   y = gain2 * decimate_down( FIR_fd( a padded/cropped by (qx0,qx1,qy0,qy1) ) )               size Ho x Wo (checked)
 * Filters are dense 2-D fp32 ([fh][fw], null = identity), flip_* as upfirdn2d's flip_filter.  Forward: q = 0, gain1 = up^2,
 * gain2 = 1; gradients: mode 1 with the stages transposed (see inv3d_amd/torch_utils/ops/filtered_lrelu.py). */
typedef struct eg3d_flrelu_params {
    const void* x;  const void* b;  void* y;
    const float* fu;  const float* fd;
    float* mask;               /* [N,C,Hm,Wm] fp32 */
    int32_t dtype, N, C, H, W;
    int32_t fuh, fuw, fdh, fdw;
    int32_t up, down;
    int32_t px0, px1, py0, py1;
    int32_t qx0, qx1, qy0, qy1;
    int32_t Ho, Wo;
    int32_t flip_fu, flip_fd, mode;
    float gain1, gain2;
    float gain, slope, clamp;  /* mode 0 only; clamp < 0 = none */
} eg3d_flrelu_params;
int eg3d_filtered_lrelu(const eg3d_flrelu_params* p, void* stream);
/* The plugin's stand-alone activation `filtered_lrelu_act_` (torch_utils/ops/filtered_lrelu.cpp:217-272; kernel filtered_lrelu.cu:1110-1215),
 * in place on a contiguous [NC, H, W] tensor:  v = x * gain, then
 *   mode 1 (write signs)  v < 0 -> v *= slope (sign 1);  |v| > clamp -> v = +-clamp (sign 2);  the 2-bit signs go to `signs`
 *   mode 2 (read signs)   bit 0 of the sign at (x + sx, y + sy) -> v *= slope;  bit 1 -> v = 0;  outside the sign image: gain only
 *   mode 0                as mode 1 without a sign image.
 * signs: [NC][sH][sW / 4] bytes, element x in bits 2 (x & 3) of byte x >> 2, sW % 4 == 0 (mode 1: sH >= H, sW >= W).  clamp < 0: none. */
int eg3d_filtered_lrelu_act(void* x, uint8_t* signs, int dtype, int NC, int H, int W, int sH, int sW, int sx, int sy, float gain, float slope,
                            float clamp, int mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Style affines of a whole synthesis network in one launch (the per-layer FullyConnectedLayer(w_dim -> in_channels) of
 * training/networks_stylegan2.py:98-108 and :129-137, ~26 tiny GEMMs + scalings per forward in the reference):
 *   fwd:  out_l[n,j] = ( sum_k ws[n,wrow_l,k] * (weight_l[j,k]*wgain_l) + bias_l[j]*bgain_l ) * post_l
 *         d_l[n,o]   = rsqrt( sum_j out_l[n,j]^2 wsq_l[o,j] + 1e-8 )                      (layers with wsq: second launch)
 *   bwd:  dout_extra_l[n,j] += -out_l[n,j] * sum_o dd_l[n,o] d_l[n,o]^3 wsq_l[o,j]        (layers with dd: first launch)
 *         dws[n,wrow_l,k] += sum_j (dout_l[n,j] + dout_extra_l[n,j]) * post_l * (weight_l[j,k]*wgain_l)   (dws pre-zeroed; null = skip)
 *         dweight_l[j,k]   = sum_n (dout_l[n,j] + dout_extra_l[n,j]) * post_l * wgain_l * ws[n,wrow_l,k]  (trainable affines: the
 *         dbias_l[j]       = sum_n (dout_l[n,j] + dout_extra_l[n,j]) * post_l * bgain_l                     pivotal-tuning phase)
 * ws/dws: [N,L,D] fp32, D a multiple of 4; weight_l: [C_l,D] row-major. */
#define EG3D_STYLE_BANK_MAX 32
typedef struct eg3d_style_layer {
    const float* weight;  const float* bias;  float* out;  const float* dout;
    int32_t C, wrow;
    float wgain, bgain, post;
    int32_t Co;                /* demodulation (conv layers; 0 = none): number of output channels of the layer's conv          */
    const float* wsq;          /* [Co, C] sum over taps of w^2 (networks_stylegan2.py:62-65), or null                             */
    float* d;                  /* fwd out: [N, Co] demodulation coefficients rsqrt(sum_k out[n,k]^2 wsq[o,k] + 1e-8)               */
    const float* dd;           /* bwd in : [N, Co] gradient w.r.t. d, or null                                                     */
    float* dout_extra;         /* bwd scratch: [N, C] zeroed; receives the style gradient that flows through d; added to dout    */
    float* dweight;            /* bwd out: [C, D] gradient of `weight` (overwritten), or null                                    */
    float* dbias;              /* bwd out: [C] gradient of `bias` (overwritten), or null                                         */
} eg3d_style_layer;
typedef struct eg3d_style_bank {
    const float* ws;  float* dws;
    int32_t N, L, D, nlayers;
    eg3d_style_layer layers[EG3D_STYLE_BANK_MAX];
} eg3d_style_bank;
int eg3d_style_affine_fwd(const eg3d_style_bank* bank, void* stream);
int eg3d_style_affine_bwd(const eg3d_style_bank* bank, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layer epilogues (NHWC fp32) -- the fused replacement of upfirdn2d + noise add + bias_act after a modulated
 * conv (training/networks_stylegan2.py:87-90,327-329; conv2d_resample.py:129) and of its backward.
 *
 * fwd: out[n,y,x,c] = clamp(act( FIR(z)[n,y,x,c] * d[n,c] + noise[n,y,x]*strength + bias[c] ) * gain)
 *      FIR: fir==null -> identity (z is [N,H,W,C]); else a (fh x fw) filter applied with padding pad0 (top/left) on
 *      z [N,Hz,Wz,C] and multiplied by fir_gain (the on-path case: 4x4, pad 1, gain 4, Hz = H+1).
 *      out_amax (optional, pre-zeroed device scalar) receives max|out| (atomic max): the operand range of the next layer's split image.
 */
int eg3d_modconv_epilogue_fwd(const float* z, float* out, int N, int H, int W, int C, int Hz, int Wz,
                              const float* fir, int fh, int fw, int pad0, float fir_gain, const float* d,
                              const float* noise, int64_t noise_nstride, const float* noise_strength,
                              const float* bias, int act, float alpha, float gain, float clamp, float* out_amax, void* stream);
/* The same epilogue for a SEPARABLE 4-tap FIR given by its host-side taps k4 (2-D filter = outer(k4, k4); the [1,3,3,1] / 8 filter of every
 * up-sampling layer), C % 64 == 0, act in {linear, relu, lrelu}: staged through LDS (csrc/epilogue.hip: upconv_epilogue_strip_kernel;
 * one image H * W * C * 4 <= 0x7fffffe0 bytes, EG3D_ERR_UNSUPPORTED beyond: 32-bit offsets into a buffer descriptor per image).  With
 * split_image (+ split_in_scale [N,C] = the CONSUMER layer's styles, split_scale_out = device scalar; clamp >= 0 required, it is the range
 * bound) the launch also writes that layer's operand image split(out * split_in_scale) exactly as eg3d_split_activation would
 * (eg3d_split_activation_bytes(N, H, W, C) bytes), so the consumer needs no split pass of its own. */
int eg3d_upconv_epilogue_fwd(const float* z, float* out, int N, int H, int W, int C, int Hz, int Wz, const float* k4, int pad0, float fir_gain,
                             const float* d, const float* noise, int64_t noise_nstride, const float* noise_strength, const float* bias, int act,
                             float alpha, float gain, float clamp, float* out_amax, const float* split_in_scale, void* split_image,
                             float* split_scale_out, void* stream);

/* bwd: given dout and the saved layer output `out`:
 *      dy = dout * act'(out) * gain   (0 where |out| >= clamp; derivative keyed on the OUTPUT as bias_act.cu:76,145)
 *      dz[n,y,x,c] = dy * d[n,c]                    (written; d==null -> dy)
 *      dbias[c]   += sum dy                         (if dbias)
 *      dd[n,c]    += sum_px dy * (pre_act - bias[c] - noise*strength)   (if dd; pre_act recovered from out)
 *      dnoise[n?,y,x] += strength * sum_c dy        (if dnoise; batch stride dnoise_nstride, 0 = shared buffer)
 *      dstrength  += sum dy * noise                 (if dstrength)
 *   All reduction targets must be pre-zeroed; they are accumulated with atomics. */
int eg3d_modconv_epilogue_bwd(const float* dout, const float* out, float* dz, int N, int H, int W, int C,
                              const float* d, const float* noise, int64_t noise_nstride,
                              const float* noise_strength, const float* bias, int act, float alpha, float gain,
                              float clamp, float* dbias, float* dd, float* dnoise, int64_t dnoise_nstride,
                              float* dstrength, float* dz_amax, void* stream);
/* dz_amax (optional, pre-zeroed device scalar): receives max|dz| (atomic max) -- the operand range an F16X3 data-gradient conv needs. */

/* Finish of a split-K data gradient (low-resolution layers, where one launch cannot fill 256 CUs without splitting K):
 *   z = conv data-gradient accumulated with EG3D_EPI_ATOMIC;  dx = z * s[n,c] (+ addend);  ds[n,c] += sum_px z * x  (if ds). */
int eg3d_dgrad_finish(const float* z, const float* x, const float* s, const float* addend, float* dx, float* ds, int N, int H,
                      int W, int C, void* stream);
/* The same finish followed, in the same pass, by the activation backward of the layer that produced x (EG3D_EPI_BWD_ACT for the split-K
 * layers): the value eg3d_dgrad_finish would store is that layer's dout;  dz = dout * act'(x) * gain * d, reductions as in
 * eg3d_modconv_epilogue_bwd (targets in `ab`, pre-zeroed), dz_amax optional. */
int eg3d_dgrad_finish_act(const float* z, const float* x, const float* s, const float* addend, float* dz, float* ds, int N, int H,
                          int W, int C, const eg3d_act_bwd* ab, float* dz_amax, void* stream);
/* Data gradient of a 1x1 layer with FOUR (padded) outputs -- toRGB of the super-resolution head, networks_stylegan2.py:338-359 -- fused
 * with the activation backward of the layer that produced x, as one element-wise pass (eg3d_conv2d_igemm_f32 with EG3D_EPI_BWD_ACT does the
 * same through a GEMM with a 4-deep contraction):  z[px,c] = sum_o dy4[px,o] * wa4[c,o];  dout = z * s[n,c] (+ addend);  ds[n,c] += sum_px z * x;
 * then dz / dbias / dd / dnoise / dstrength / max|dz| exactly as eg3d_dgrad_finish_act.  dy4 [N,H,W,4], wa4 [C,4], x / addend / dz [N,H,W,C]. */
int eg3d_torgb_dgrad_act(const float* dy4, const float* wa4, const float* x, const float* s, const float* addend, float* dz, float* ds, int N, int H,
                         int W, int C, const eg3d_act_bwd* act_bwd, float* dz_amax, void* stream);
/* The same pass writing dz as the two-piece fp16 operand image of the data gradient that consumes it (layout and scale of
 * eg3d_split_activation; replaces that pass): the range comes from a bound formed inside the kernel from dy_amax = max|dy4| and
 * addend_amax = max|addend| (device scalars written by the producers of those tensors; addend_amax is required with addend).  dz may be
 * null when nothing else reads the fp32 gradient.  C % 8 == 0. */
int eg3d_torgb_dgrad_act_split(const float* dy4, const float* wa4, const float* x, const float* s, const float* addend, float* dz, float* ds,
                               int N, int H, int W, int C, const eg3d_act_bwd* ab, const float* dy_amax, const float* addend_amax,
                               void* split_image, float* split_scale_out, void* stream);

/* NHWC FIR resampler used on the fused path (skip-image 2x upsample and its adjoint, FIR adjoint of up=2 layers):
 *   same arithmetic as eg3d_upfirdn2d on a channels-last fp32 tensor, float4 over channels (C % 4 == 0),
 *   optional accumulate into y (y += result). */
int eg3d_upfirdn2d_nhwc(const float* x, const float* f, float* y, int N, int C, int inH, int inW, int fH, int fW,
                        int up, int down, int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                        int outH, int outW, int accumulate, void* stream);
/* ... and y = result + addend ([N, outH, outW, C] fp32, 16-byte aligned, not y itself; resampling forms only, i.e. not the plain 4x4 FIR): the skip
 * image of a clamped toRGB layer, img = upsample2d(img) + y (training/networks_stylegan2.py:453-455), in one pass instead of an up-sampling
 * pass and an element-wise add. */
int eg3d_upfirdn2d_nhwc_add(const float* x, const float* f, const float* addend, float* y, int N, int C, int inH, int inW, int fH, int fW,
                            int up, int down, int padx0, int padx1, int pady0, int pady1, int flip, float gain, int outH, int outW,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Style / demodulation helpers (training/networks_stylegan2.py:62-67,303,315,354):
 *   wsq[o,k]   = sum_taps w[o,tap,k]^2                               (once per weight update)
 *   demod fwd:  d[n,o] = rsqrt( sum_k s[n,k]^2 * wsq[o,k] + 1e-8 )
 *   demod bwd:  ds[n,k] += sum_o dd[n,o] * ( -d[n,o]^3 * s[n,k] * wsq[o,k] )
 *               dwsq[o,k] += sum_n dd[n,o] * ( -0.5 * d[n,o]^3 * s[n,k]^2 )       (if dwsq)
 */
int eg3d_weight_sqsum(const float* w, float* wsq, int Co, int ntaps, int Ck, void* stream);
/* One pass over a dense conv weight w[O][I][T] (T = kh*kw): wf[o][t*I+i] (forward operand), wa[i][t*O+o] (data-gradient operand),
 * wsq[o][i] = sum_t w^2 (or null).  Used where weights change every step (pivotal tuning). */
int eg3d_pack_conv_weight(const float* w, float* wf, float* wa, float* wsq, int O, int I, int T, void* stream);
/* The same with a per-output-channel scale folded in, w'[o] = w[o] * oscale[o] (an eval-mode BatchNorm folded into the conv that precedes
 * it: scripts/resnet/resnet.py + w_projector.py:62), no wsq; wa may be null (forward image only).  And the gradient of that fold from
 * the packed weight-gradient image g[o][t*Ip + i] (eg3d_conv2d_wgrad_f32 output, Ip >= I padded input channels):
 *   dw[o][i][t] = g[o][t*Ip + i] * oscale[o] (parameter layout),  doscale[o] = sum_{i,t} g[o][t*Ip + i] * w[o][i][t]   (oscale / doscale may be null). */
int eg3d_pack_conv_weight_scaled(const float* w, const float* oscale, float* wf, float* wa, int O, int I, int T, void* stream);
/* eg3d_pack_conv_weight into buffers whose output-channel dimension is padded to O_pad >= O (toRGB: 3 -> 4 channels so that the image
 * is carried with 16-byte pixels): wf has O_pad rows, wa rows of T*O_pad floats (element (i, t, o) at (i*T + t)*O_pad + o).  Only the O real
 * channels are written: the caller zero-fills both buffers once and reuses them while the weights train. */
int eg3d_pack_conv_weight_padded(const float* w, float* wf, float* wa, float* wsq, int O, int I, int T, int O_pad, void* stream);
/* Weight gradient of a demodulated modulated conv, parameter layout, from the packed weight-gradient image g[o][t*I + i] of
 * eg3d_conv2d_wgrad_f32 plus the demodulation path (networks_stylegan2.py:60-63):
 *   dw[o][i][t] = g[o][t*I + i] + 2 w[o][i][t] * sum_n dd[n,o] (-1/2) d[n,o]^3 s[n,i]^2        (dd null: first term only)
 * s [N,I] styles, d [N,O] demodulation coefficients, dd [N,O] their gradient; w, dw [O,I,T]. */
int eg3d_weight_grad_finish(const float* g, const float* w, const float* s, const float* d, const float* dd, float* dw, int N, int O, int I, int T,
                            void* stream);
/* ... with g = the sum, in slab order, of nslab images [O][T*I] that lie slab_stride floats apart (eg3d_wgrad_v2_params::slabs). */
int eg3d_weight_grad_finish_slabs(const float* g, int nslab, int64_t slab_stride, const float* w, const float* s, const float* d, const float* dd, float* dw,
                                  int N, int O, int I, int T, void* stream);
/* eg3d_weight_grad_finish_slabs of up to EG3D_WGF_BATCH_MAX layers in ONE launch (pivotal tuning: the gradients of all conv weights are
 * wanted together, by the optimiser; same arguments per item). */
#define EG3D_WGF_BATCH_MAX 32
typedef struct eg3d_wgf_item {
    const float* g; const float* w; const float* s; const float* d; const float* dd; float* dw;
    int64_t slab_stride;
    int32_t N, O, I, T, nslab;
} eg3d_wgf_item;
int eg3d_weight_grad_finish_batched(const eg3d_wgf_item* items, int n, void* stream);
/* eg3d_pack_conv_weight (O_pad = 0) / eg3d_pack_conv_weight_padded of up to EG3D_PACK_BATCH_MAX layers in ONE launch: during pivotal tuning
 * all generator weights change together once per step.  wa / wsq may be null per item. */
#define EG3D_PACK_BATCH_MAX 40
typedef struct eg3d_pack_item {
    const float* w; float* wf; float* wa; float* wsq;
    int32_t O, I, T, O_pad;
    const float* oscale;       /* [O] per-output-channel scale folded into wf / wa (eg3d_pack_conv_weight_scaled: a folded BatchNorm), or null */
} eg3d_pack_item;
int eg3d_pack_conv_weights_batched(const eg3d_pack_item* items, int n, void* stream);
int eg3d_unpack_weight_grad(const float* g, const float* w, const float* oscale, float* dw, float* doscale, int O, int I, int Ip, int T, void* stream);
int eg3d_demod_fwd(const float* s, const float* wsq, float* d, int N, int Co, int Ck, void* stream);
int eg3d_demod_bwd(const float* s, const float* wsq, const float* d, const float* dd, float* ds, float* dwsq,
                   int N, int Co, int Ck, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Noise-buffer maintenance of the latent projector (training/projectors/w_projector.py:221-237 noise regulariser and its
 * autograd backward; :264-270 renormalisation), all buffers in one launch each.  x[i]: [res[i],res[i]] fp32 device
 * buffers (res a power of two), nbufs <= 32.
 *   regularizer: *reg_out = scale * sum_buffers sum_levels (mean(x*roll(x,1,W))^2 + mean(x*roll(x,1,H))^2) over the avg-pool
 *                pyramid res, res/2, ... (last level <= 8); grad[i] (may be null / contain nulls) = d(*reg_out)/d x[i].
 *   normalize:   x <- (x - mean(x)) * rsqrt(mean((x - mean)^2))   in place.  workspace: 2*nbufs zeroed floats -> two multi-block
 *                launches (moments, apply); null -> one block per buffer in a single launch.
 */
int64_t eg3d_noise_reg_workspace_floats(const int32_t* res, int nbufs);
int eg3d_noise_regularizer(float* const* x, float* const* grad, const int32_t* res, int nbufs, float* workspace,
                           float* reg_out, float scale, void* stream);
int eg3d_noise_normalize(float* const* x, const int32_t* res, int nbufs, float* workspace, void* stream);

/* Low-latency toRGB for small pixel counts (the 4^2 .. 64^2 blocks of the backbone) -- replaces ToRGBLayer.forward
 * (training/networks_stylegan2.py:338-359) + the skip accumulation of SynthesisBlock.forward (:433-436) where eg3d_conv2d_igemm_f32's
 * 32-step contraction loop is all latency:
 *   out[n,p,o] = clamp( sum_c x[n,p,c] s[n,c] w[o,c] + bias[o] ) + addend[n,p,o]
 * with exact fp32 products (v_mfma_f32_32x32x2_f32).  x [N,H*W,ldx] NHWC (C used, C % 8 == 0), w [Cp][w_row] (row per output, Cp % 32 == 0:
 * padded rows are zero), s [N,C], bias [Cp] or null, clamp < 0 = none; addend null | [N,H,W,ldo] | (addend_up2) the half-resolution image
 * [N,H/2,W/2,ldo] added through upsample2d with the separable 4-tap filter addend_taps (as eg3d_conv_params::addend_up2).  out [N,H,W,ldo]. */
typedef struct eg3d_torgb_small_params {
    const float* x;
    const float* w;
    const float* s;
    const float* bias;
    const float* addend;
    float* out;
    int32_t N, H, W, C, Cp;
    int32_t ldx, ldo, w_row;
    int32_t addend_up2;
    float clamp;
    float addend_taps[4];
    /* optional: the producing layer's finishing epilogue inside this launch.  With pre_z set, x is an OUTPUT: pre_z [N,H*W,ldx] holds that layer's
     * split-K sums, x = clamp(pwl(pre_z * pre_d[n,c] + pre_noise[n,p] * *pre_strength + pre_bias[c]) * pre_gain) is formed while the operand loads
     * (eg3d_modconv_epilogue_fwd's arithmetic; pwl = x > 0 ? x : x * pre_slope) and written to x; max|x| goes to x_amax (atomic max, or null). */
    const float* pre_z;
    const float* pre_d;
    const float* pre_bias;
    const float* pre_noise;
    const float* pre_strength;
    float* x_amax;
    int64_t pre_noise_nstride;
    float pre_slope, pre_gain, pre_clamp;
    int32_t pad_;
} eg3d_torgb_small_params;
int eg3d_torgb_small_supported(const eg3d_torgb_small_params* p);
int eg3d_torgb_small_fwd(const eg3d_torgb_small_params* p, void* stream);
/* Large pixel counts (the 128^2 / 256^2 blocks of the backbone: Cp == 96, C % 32 == 0, C <= 256, H*W % 32 == 0, W >= 32, >= 8192 pixels, no
 * pre_z): eg3d_torgb_small_fwd runs the same arithmetic as a persistent streaming kernel (weights resident in LDS, x read once); this
 * reports whether a launch with these parameters takes that form -- callers use it to decide between this entry and the implicit GEMM. */
int eg3d_torgb_mid_supported(const eg3d_torgb_small_params* p);

/* Data gradient of that layer for small pixel counts: dx[n,p,c] = (sum_o dy[n,p,o] wa[c,o]) s[n,c] + addend[n,p,c]; ds[n,c] += the un-scaled
 * sum times xin[n,p,c] (pre-zeroed, optional).  act_on != 0: additionally the activation backward of the layer that produced xin, exactly as
 * EG3D_EPI_BWD_ACT of eg3d_conv2d_igemm_f32 (dx receives that layer's dz; act_bwd's accumulators are filled).  dy [N,H*W,ldg] (Cp used, Cp % 8
 * == 0), wa [C][wa_row] (row per INPUT channel), C % 32 == 0, xin / addend / dx [N,H*W,ldx].  out_amax: optional pre-zeroed max|dx|. */
typedef struct eg3d_torgb_small_bwd_params {
    const float* dy;
    const float* wa;
    const float* s;
    const float* xin;
    const float* addend;
    float* dx;
    float* ds;
    float* out_amax;
    int32_t N, H, W, C, Cp;
    int32_t ldg, ldx, wa_row;
    int32_t act_on;
    int32_t no_mid;              /* != 0: never the streaming form (eg3d_torgb_mid_bwd_supported reports 0): the A/B switch EG3D_TORGB_MID_BWD=0 reaches every launch */
    eg3d_act_bwd act_bwd;
    /* optional (both or neither; needs addend and xin): the addend is the UNFINISHED split-K data gradient z of the layer that consumes x next
     * (eg3d_dgrad_finish not run): this launch adds z * add_scale[n,c] and accumulates add_ds[n,c] += sum_p z[n,p,c] xin[n,p,c] (pre-zeroed). */
    const float* add_scale;
    float* add_ds;
} eg3d_torgb_small_bwd_params;
int eg3d_torgb_small_bwd_supported(const eg3d_torgb_small_bwd_params* p);
int eg3d_torgb_small_bwd(const eg3d_torgb_small_bwd_params* p, void* stream);
/* The streaming form of the data gradient (Cp == 96, H*W % 32 == 0, >= 4096 pixels): waves walk several pixel tiles with the column sums in
 * registers, one set of atomics per workgroup.  Same results up to summation order; reports whether eg3d_torgb_small_bwd takes that form. */
int eg3d_torgb_mid_bwd_supported(const eg3d_torgb_small_bwd_params* p);

/* torch.optim.Adam(betas, eps; no weight decay, no amsgrad) over up to EG3D_ADAM_ITEMS_MAX leaves in one launch (the projector's
 * optimiser, w_projector.py:107-118,256): p, m (exp_avg), v (exp_avg_sq) updated in place from the gradient g + g2 (one of them may be
 * null).  lr and step are DEVICE scalars (a captured graph is replayed for every step index): step holds the number of updates already
 * made as a float and is incremented by the launch when bump_step != 0 (several launches of one optimiser step: set it on the last).
 * normalize != 0: the leaf is then renormalised in place, p <- (p - mean(p)) * rsqrt(var(p)) (w_projector.py:264-270), by a second launch.
 * workspace: 2*n + 1 ZEROED floats (moments of the flagged leaves, retirement counter; left zeroed-counter on exit). */
/* eg3d_early_stop_flag: done = max(done, value <= threshold ? 1 : 0) on the device (sticky; `value` e.g. the LPIPS term of the step). */
#define EG3D_ADAM_ITEMS_MAX 32
typedef struct {
    float* p;
    const float* g;
    const float* g2;
    float* m;
    float* v;
    int64_t n;
    int32_t normalize, pad_;
} eg3d_adam_item;
typedef struct {
    int32_t n, bump_step;
    float beta1, beta2, eps, pad_;
    const float* lr;
    float* step;
    eg3d_adam_item items[EG3D_ADAM_ITEMS_MAX];
    const float* skip;         /* optional device scalar: != 0 -> the launch changes nothing (no update, no step count): the early stop of the
                                * pivotal-tuning loop, which leaves BEFORE the update (training/coaches/single_id_coach.py:68-71), as a device-side
                                * flag, so that a captured step can be replayed while the criterion is checked every step */
} eg3d_adam_list;
int eg3d_adam_step(const eg3d_adam_list* list, float* workspace, void* stream);
int eg3d_early_stop_flag(const float* value, float threshold, float* done, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose chain of the latent projector (training/projectors/w_projector.py:147-172 with utils/camera_utils.py:201-228 quaternion, :259-273
 * six-dimensional, :241-257,158-188 Euler): pose vector [B,np] (mode 0: quaternion w,x,y,z, np 4; 1: 6-D, np 6; 2: two angles added to pi/2,
 * np 2) + optimisable translation [B,3] + intrinsics [9] -> extrinsic ext [B,16] and conditioning vector cam [B,25] = (ext, intrinsics).
 * jac [B,12,9] (Jacobian of rotation 3x3 + translation 3 with respect to (pose, translation), forward-mode duals) and out12 [B,12] are
 * caller-owned work buffers the backward reads: d_pose [B,np], d_translation [B,3] (either may be null) from d_ext [B,16] and / or d_cam [B,25]. */
int eg3d_pose_chain_fwd(const float* pose, const float* translation, const float* intrinsics, int B, int mode, float radius, float* ext, float* cam,
                        float* jac, float* out12, void* stream);
int eg3d_pose_chain_bwd(const float* jac, const float* d_ext, const float* d_cam, int B, int mode, float* d_pose, float* d_translation, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Volume renderer -- replaces RaySampler.forward (training/volumetric_rendering/ray_sampler.py:24-73) and
 * ImportanceRenderer.forward (renderer.py:143-195: sample_stratified, sample_from_planes/grid_sample, OSGDecoder
 * triplane.py:124-136, MipRayMarcher2 ray_marcher.py:25-57, sample_importance/sample_pdf, unify_samples), fused
 * per ray; nothing but the final per-ray outputs is materialised.
 */
int eg3d_ray_gen_fwd(const float* cam2world, const float* intrinsics, float* origins, float* dirs, int N, int res,
                     void* stream);
/* d_cam2world [N,16], d_intrinsics [N,9] (may be null) are overwritten. */
int eg3d_ray_gen_bwd(const float* cam2world, const float* intrinsics, const float* d_origins, const float* d_dirs,
                     float* d_cam2world, float* d_intrinsics, int N, int res, void* stream);

typedef struct eg3d_render_params {
    const float* planes;       /* [N,Hp,Wp,ldp] NHWC; plane p = channels [p*C, (p+1)*C)    */
    int32_t N, Hp, Wp, ldp, C; /* C = 32 features per plane                                */
    const float* origins;      /* [N,R,3]                                                  */
    const float* dirs;         /* [N,R,3]                                                  */
    int32_t R;                 /* rays per image                                           */
    const float* u1;           /* [N,R,Dc] stratified jitter in [0,1)                      */
    const float* u2;           /* [N*R,Df] importance uniforms                             */
    int32_t Dc, Df;            /* coarse / fine samples per ray (Df may be 0)              */
    float ray_start, ray_end;  /* used when ray_limits == null                             */
    const float* ray_limits;   /* [N,R,2] per-ray (start,end) for the 'auto' mode, or null */
    int32_t disparity;         /* disparity_space_sampling                                 */
    float box_warp;
    int32_t white_back;
    /* decoder (OSGDecoder): runtime gains already folded in by the caller */
    const float* w0;           /* [H,C]   = net.0.weight * lr_mul/sqrt(C)                  */
    const float* b0;           /* [H]     = net.0.bias * lr_mul                            */
    const float* w1;           /* [H,1+Cout] = (net.2.weight * lr_mul/sqrt(H))^T  (transposed) */
    const float* b1;           /* [1+Cout]                                                 */
    int32_t Hdim, Cout;        /* 64, 32                                                   */
    /* outputs */
    float* rgb;                /* [N,R,Cout]                                               */
    float* depth;              /* [N,R]  (unclamped; NaN kept -- finalize clamps)          */
    float* wsum;               /* [N,R]                                                    */
    float* depth_minmax;       /* [2] running global (min,max) of all sample depths; init (+inf,-inf) by the caller -- the pipelined forward
                                * (pos_rows + save_* given) initialises it itself */
    float* fine_depths;        /* [N,R,Df] workspace: importance depths (re-used by backward)*/
    /* training mode (both or neither): the forward keeps (sigma, colour) of every sample for the backward.
     * Row ((n*R + ray)*2 + pass)*D + s, pass 0 = coarse / 1 = fine, D = max(Dc,Df).                                  */
    float* save_sigma;         /* [S]                                                      */
    float* save_rgb;           /* [S,Cout]                                                 */
    int32_t ray_tile_width;    /* locality hint only (any value gives identical results): when the R rays of an image are the
                                * row-major pixels of an image ray_tile_width wide (a multiple of 32), workgroups are assigned
                                * to rays in 32-pixel-wide column strips so that each XCD's L2 sees a compact screen tile and
                                * hence a small tri-plane footprint.  0 = rays in no particular order. */
    float* pos_rows;           /* optional workspace [2, N*R, D, 4] (D = max(Dc,Df)).  With it (and save_sigma / save_rgb / fine_depths) the
                                * forward runs as a pipeline -- sample positions -> tri-plane gather + decoder on the matrix cores
                                * (the sample-level kernel of the backward) -> importance sampling -> decoder -> compositing from the
                                * saved rows -- instead of one fused per-ray kernel with the decoder on the vector ALUs.  null = fused. */
    float* feat_rows;          /* optional [S,32] (row order of save_rgb), pipelined forward only: the interpolated tri-plane feature of every
                                * sample.  With it the gather runs as its own high-occupancy pass (the fused gather + decoder kernels hold
                                * ~140 registers and wait on the scattered texel loads most of the time) and the decoder kernels -- forward
                                * and, given the same buffer in eg3d_render_bwd_params.fwd, backward -- read the rows back coalesced.
                                * Same values either way.  null = gather inside the decoder kernels. */
    int32_t* dbg_inds;         /* optional [N*R, Df, 3] (pipelined and fused forward): per fine sample the bin index torch.searchsorted(cdf, u,
                                * right=True) would return, and the `below` / `above` indices after the clamps (renderer.py:292-295) -- the
                                * integer side of sample_pdf, for index-exact parity tests.  null = not written. */
    int32_t* dbg_ranks;        /* optional [N*R, Dc + Df]: position of coarse sample s (entry s) and fine sample s (entry Dc + s) in the depth-sorted
                                * list of unify_samples (the inverse of the permutation torch.sort(stable) returns, renderer.py:212-222).  */
    float* dbg_cdf;            /* optional [N*R, ns = Dc - 3]: the ray's CDF edges cdf[1 .. ns] (cdf[0] = 0) exactly as the bin search accumulates them  */
} eg3d_render_params;

int eg3d_render_fwd(const eg3d_render_params* p, void* stream);

/* Element counts (floats) of every caller-owned buffer of the renderer entries for a given problem -- the contract a binding in another
 * language sizes its allocations from (the reference's plugins allocate inside ATen; this library never allocates).  Only N, R, Dc, Df and
 * Cout of `p` are read.  S = N*R*2*max(Dc,Df) sample rows.  A count of 0 = that buffer does not exist for this problem. */
typedef struct eg3d_render_sizes {
    int64_t S;                 /* sample rows                                                            */
    int64_t rgb, depth, wsum, depth_minmax, fine_depths;      /* eg3d_render_fwd outputs                  */
    int64_t save_sigma, save_rgb, pos_rows;                   /* training-mode forward (pos_rows optional) */
    int64_t df_rows, df_pos, ag_rows, gc_rows;                /* eg3d_render_bwd                          */
    int64_t dump_dpre, dump_h, dump_dout, dump_feat;          /* decoder-weight gradient operands         */
    int64_t feat_rows;                                        /* optional feature rows (pipelined forward) */
} eg3d_render_sizes;
int eg3d_render_query_sizes(const eg3d_render_params* p, eg3d_render_sizes* out);
/* depth <- clamp(nan_to_num(depth, inf), min, max) with the global min/max (ray_marcher.py:49-50). */
int eg3d_render_finalize(float* depth, const float* depth_minmax, int64_t n, void* stream);

typedef struct eg3d_render_bwd_params {
    eg3d_render_params fwd;    /* same inputs as the forward (fine_depths filled by it)     */
    const float* depth_out;    /* [N,R] finalized depth (to know which rays were clamped)   */
    const float* d_rgb;        /* [N,R,Cout]                                               */
    const float* d_depth;      /* [N,R] or null                                            */
    const float* d_wsum;       /* [N,R] or null                                            */
    /* Plane gradient: the kernel dumps one row per (ray, pass, s) -- row ((n*R + ray)*2 + pass)*D + s, D = max(Dc,Df) --
     * holding dL/d(mean feature)/3 and the sample position; eg3d_triplane_scatter then bins the rows by texel tile and
     * accumulates them in LDS (a direct scatter would be 384 float atomics per sample).  Both null = no plane gradient. */
    float* df_rows;            /* [S,32]                                                   */
    float* df_pos;             /* [S,4] (x,y,z,-); x = NaN marks an absent sample          */
    float* ag_rows;            /* [S,2] workspace: per-sample (colour weight, dL/d sigma) from the ray-level pass */
    float* gc_rows;            /* [S,4] workspace: per-sample (dL/d position, depth); required with d_origins/d_dirs */
    float* d_origins;          /* [N,R,3] overwritten, or null                             */
    float* d_dirs;             /* [N,R,3] overwritten, or null                             */
    /* Decoder-weight gradients (PTI phase): when non-null the kernel dumps, for sample row
     * ((n*R + ray)*2 + pass)*D + s  (pass 0 = coarse, 1 = fine, D = max(Dc,Df); rows of absent samples untouched, so
     * pre-zero the buffers), the four GEMM operands; the caller contracts them with a library GEMM:
     *   d_w0 = dump_dpre^T @ dump_feat,  d_b0 = colsum(dump_dpre),  d_w1t = dump_h^T @ dump_dout,  d_b1 = colsum(dump_dout) */
    float* dump_dpre;          /* [S,64]  */
    float* dump_h;             /* [S,64]  */
    float* dump_dout;          /* [S,33]  */
    float* dump_feat;          /* [S,32]  */
    float* df_amax;            /* optional [1]: max|df_rows| of this call (reset by the call itself).  Hand it to eg3d_triplane_scatter and the
                                * accumulation runs on the 16-bit matrix cores (three products of two-piece operands, the arithmetic of the
                                * convolutions, operands scaled by this maximum); null = exact fp32 products on the fp32 matrix cores */
    /* Decoder-weight gradients contracted INSIDE the sample-level kernel (all four or none; pre-zeroed, accumulated; excludes the dumps):
     *   gram_w0 [64,32] += gram_scale0 * dpre^T feat      gram_b0 [64] += gram_bias_scale * colsum(dpre)
     *   gram_w1 [33,64] += gram_scale1 * dout^T h         gram_b1 [33] += gram_bias_scale * colsum(dout)        (row / entry 0 = sigma)
     * exact fp32 products (v_mfma_f32_32x32x2_f32), as the caller's GEMM over the dumps would do: the 1.0 GB of dump rows is never written. */
    float* gram_w0; float* gram_b0; float* gram_w1; float* gram_b1;
    float gram_scale0, gram_scale1, gram_bias_scale;
} eg3d_render_bwd_params;

int eg3d_render_bwd(const eg3d_render_bwd_params* p, void* stream);

/* eg3d_render_bwd = a ray-level kernel (merge, march, reverse scan -> ag_rows) + a sample-level kernel (gather, decoder
 * forward/backward -> df_rows/df_pos, gc_rows, optional decoder dumps) + a per-ray reduction of gc_rows.
 *
 * d_planes[N,Hp,Wp,ldp] (pre-zeroed) += bilinear-adjoint scatter of the S dumped rows (grid_sample backward w.r.t. the
 * planes, renderer.py:64 under autograd).  rows_per_image = R*2*D.  workspace: eg3d_triplane_scatter_workspace_ints() int32.
 * Rows of absent samples (df_pos x = NaN) are never read: their df_rows rows may hold anything, NaN and Inf included (eg3d_render_bwd leaves
 * them unwritten).  The rows of present samples must be finite.
 *
 * Supported range (both builds; EG3D_ERR_UNSUPPORTED outside it, decided from the arguments before any GPU work):
 *   - planes up to 270 x 270: 3 * ceil(Hp / 15) * ceil(Wp / 15) * 16 <= 16384 (tile, texel row) lists per image;
 *   - S = N * rows_per_image exactly, rows_per_image < 2^25 (one image's df_rows below 2^32 bytes; the records hold 27-bit row ids), 12 * S <= INT32_MAX, ldp >= 96.
 * There is one accumulation path (the row-keyed lists of csrc/renderer.hip); earlier versions of the normal build ran calls outside this
 * range on older, unmaintained kernels -- those are gone, and the normal build now refuses what the deterministic build always refused. */
int64_t eg3d_triplane_scatter_workspace_ints(int64_t S, int N, int Hp, int Wp);
/* ray_w, rows_per_ray: optional hint (0, 0 = unknown) -- rays per image row and dumped rows per ray (2 D) of the row layout above; the
 * binning passes then walk the rows in bricks of 16 x 16 rays (fewer bins per block); the result does not depend on it.
 * df_amax: eg3d_render_bwd_params.df_amax of the call that produced df_rows, or null (see there). */
int eg3d_triplane_scatter(const float* df_rows, const float* df_pos, int64_t S, int64_t rows_per_image, float* d_planes, int N,
                          int Hp, int Wp, int ldp, float box_warp, int32_t* workspace, int ray_w, int rows_per_ray, const float* df_amax, void* stream);

/* Decoder-only query (ImportanceRenderer.run_model, renderer.py:197-203; used for density grids):
 *   coords [N,M,3] -> rgb [N,M,Cout], sigma [N,M]. */
int eg3d_sample_decode(const eg3d_render_params* p, const float* coords, int64_t M, float* rgb, float* sigma,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Perceptual-loss network pieces.  The reference evaluates three third-party networks per step:
 * VGG16-LPIPS features (training/projectors/w_projector.py:50-52,112,215-219), torchvision VGG16 features[:15]
 * (training/warping_loss.py:31-37) and lpips.LPIPS(net='alex') (training/coaches/base_coach.py:48,111-112).  Their convolutions
 * go through eg3d_conv2d_igemm_f32 (bias + ReLU in the epilogue); these entry points are the layers in between.  NHWC fp32,
 * C and ldx multiples of 4, 16-byte aligned pointers.
 *
 * Max pooling without padding (torch.nn.MaxPool2d(k, s), floor mode): y[N,Ho,Wo,C] dense, Ho = (H-k)/s+1.  argmax (optional in
 * forward) holds ky*k+kx of the winning tap, one byte per output element; the first maximum in scan order wins. */
int eg3d_maxpool2d_fwd(const float* x, float* y, uint8_t* argmax, int N, int H, int W, int C, int ldx, int k, int s, void* stream);
/* dx[N,H,W,ldx] (every used channel overwritten) from dy[N,Ho,Wo,C] and the forward's argmax; gather form, no atomics. */
int eg3d_maxpool2d_bwd(const float* dy, const uint8_t* argmax, float* dx, int N, int H, int W, int C, int ldx, int k, int s, void* stream);
/* LPIPS feature head (lpips.normalize_tensor + the square root of the 1x1 "lin" layer + spatial mean folded into the features):
 *   feat[n*feat_nstride + (pix*C + c)] = scale[c] * x[n,pix,c] / (sqrt(sum_c x^2) + eps) * mul
 * so that sum((feat_a - feat_b)^2) is the layer's LPIPS term when scale = sqrt(lin weight), mul = 1/sqrt(H*W).  scale may be null (1).
 * feat points at this layer's slice of a flat [N, F] feature vector (feat_nstride = F).
 * eps_inside != 0: the normaliser is rsqrt(sum_c x^2 + eps) instead (the stand-in feature pyramid of the C2 workload). */
int eg3d_unit_normalize_fwd(const float* x, const float* scale, float* feat, int N, int HW, int C, int ldx, float mul, float eps,
                            int64_t feat_nstride, int eps_inside, void* stream);
/* dx[N,HW,ldx] = d feat / d x applied to dfeat (same slice addressing as the forward). */
int eg3d_unit_normalize_bwd(const float* x, const float* scale, const float* dfeat, float* dx, int N, int HW, int C, int ldx, float mul,
                            float eps, int64_t feat_nstride, int eps_inside, void* stream);

/* All taps of the feature pyramid in one launch (grid.y = level).  Per level: x [N,HW,ldx], scale (or null), feat = this level's slice of
 * the flat [N, F] vector (written by the forward, read as dfeat by the backward), dx [N,HW,ldx] (backward only). */
#define EG3D_UNIT_LEVELS_MAX 8
typedef struct {
    const float* x;
    const float* scale;
    const float* feat;      /* forward: output slice (written); backward: dfeat slice */
    float* dx;
    int HW, C, ldx;
    float mul;
} eg3d_unit_level;
typedef struct {
    int n, N, eps_inside;
    float eps;
    int64_t feat_nstride;
    eg3d_unit_level levels[EG3D_UNIT_LEVELS_MAX];
} eg3d_unit_levels;
int eg3d_unit_normalize_levels(const eg3d_unit_levels* batch, int bwd, void* stream);

/* Generator image -> feature-net input, one pass (w_projector.py:198-200,215: (img + 1) * 255/2, then F.interpolate(mode='area') to 256^2):
 *   out[n,y,x,c] = mul * mean_{factor x factor block}(img[n,...,c]) + add  for c < 3,  0 for c = 3.
 * img: [N,H,W,4] NHWC (the SR head's 3-channel image is carried with 4-float pixels), out: [N,H/factor,W/factor,4].
 * bwd: dimg[n,Y,X,c] = mul / factor^2 * dout[n,Y/factor,X/factor,c] (c < 3), 0 for c = 3. */
int eg3d_image_prepare_fwd(const float* img, float* out, int N, int H, int W, int factor, float mul, float add, void* stream);
int eg3d_image_prepare_bwd(const float* dout, float* dimg, int N, int H, int W, int factor, float mul, void* stream);
/* Small-channel 3 x 3 convolution (stride 1, zero padding 1) in exact fp32 on the vector ALUs, for layers too small for the matrix-core tiles
 * (the stand-in feature pyramid of inv3d_amd.inversion.StubFeatureNet: 4 -> 16 -> 32 -> 64 channels at 256^2 .. 64^2; the reference's feature
 * networks are torchvision / lpips modules, w_projector.py:50-58):
 *   y = lrelu(conv(x, W)) * gain (act != 0; plain conv otherwise), written at full resolution (y, optional) and / or as its 2 x 2 average (pooled).
 * x: [N,H,W,Ci] NHWC, Ci % 4 == 0, H and W even.  w: packed [Co/G][Ci/4][9 taps (ky*3+kx)][4][G] (correlation taps: the data gradient passes
 * the flipped, channel-transposed weights).  G in {1,2,4} output channels per thread. */
typedef struct eg3d_conv3x3_direct_params {
    const float* x;
    const float* w;
    float* y;
    float* pooled;
    int N, H, W, Ci, Co, G;
    int act;
    float alpha, gain;
    /* input transform (data gradient of a pooled level; act must be 0, pooled null): with ga or gb set, x is the level's saved full-resolution
     * output and the convolved tensor is  0.25 (ga + gb)[n,y/2,x/2,c] * gain * (x > 0 ? 1 : alpha)  -- eg3d_pool2_act_bwd without its launch */
    const float* ga;
    const float* gb;
} eg3d_conv3x3_direct_params;
int eg3d_conv3x3_direct(const eg3d_conv3x3_direct_params* p, void* stream);
/* Backward of `pooled = avg_pool2(lrelu(z) * gain)` towards z, summing the gradients of the pooled tensor's (up to) two consumers:
 *   dz[n,y,x,c] = 0.25 (ga + gb)[n,y/2,x/2,c] * gain * (yref[n,y,x,c] > 0 ? 1 : alpha)   (ga or gb may be null; NHWC, C % 4 == 0). */
int eg3d_pool2_act_bwd(const float* ga, const float* gb, const float* yref, float* dz, int N, int H, int W, int C, float alpha, float gain, void* stream);
/* out[n] (pre-zeroed) += sum_i (a[n,i] - b[n,i])^2 over flat feature vectors [N,F] (F % 4 == 0) -- the projector's per-image distance
 * (w_projector.py:216-219); bwd: da = 2 g[n] (a - b). */
int eg3d_sqdist_fwd(const float* a, const float* b, float* out, int N, int64_t F, void* stream);
int eg3d_sqdist_bwd(const float* a, const float* b, const float* g, float* da, int N, int64_t F, void* stream);

/* Terms of the pivotal-tuning objective (training/coaches/base_coach.py:104-126 calc_loss; depth TV :294-305) as weighted reductions:
 * each forward adds  value * term_scale  to *term and  value * total_scale  to *total (either may be null; both pre-zeroed), each
 * backward multiplies by the incoming scalar gradient g[0] (device) and the term's weight gscale (host).
 *   sqdist_sum: value = sum_i (a[i] - b[i])^2 over n floats (n % 4 == 0, 16-byte aligned);   da = 2 g gscale (a - b)
 *   tv_norm:    value = sum_{y<H-1, x<W-1} (v - v[x+1])^2 + (v - v[y+1])^2 over a [B,H,W] map;  dv = its gradient * g gscale */
int eg3d_sqdist_sum_fwd(const float* a, const float* b, int64_t n, float* term, float term_scale, float* total, float total_scale, void* stream);
int eg3d_sqdist_sum_bwd(const float* a, const float* b, const float* g, float gscale, float* da, int64_t n, void* stream);
int eg3d_tv_norm_fwd(const float* v, int B, int H, int W, float* term, float term_scale, float* total, float total_scale, void* stream);
int eg3d_tv_norm_bwd(const float* v, const float* g, float gscale, float* dv, int B, int H, int W, void* stream);
/* image_raw with 4-float pixels from the rendered feature image (training/triplane.py:84-85, rgb = features[:, :3]):
 * x [P,C] (C % 4 == 0) -> y4 [P,4] = (x0, x1, x2, 0);  bwd: dx [P,C] = (dy4.xyz, 0, ..., 0) (overwritten). */
int eg3d_slice_rgb4_fwd(const float* x, float* y4, int64_t P, int C, void* stream);
int eg3d_slice_rgb4_bwd(const float* dy4, float* dx, int64_t P, int C, void* stream);
/* ... bwd with the gradient of the feature image's OTHER consumer (the SR head's input, triplane.py:87-88) added in the same pass:
 * dx = addend + (dy4.xyz, 0, ..., 0); addend [P,C], may be dx itself. */
int eg3d_slice_rgb4_bwd_add(const float* dy4, const float* addend, float* dx, int64_t P, int C, void* stream);

/* Depth-reprojection geometry of the warping loss (training/warping_loss.py:18-54 + LinePlaneCollision :58-72) per pixel:
 *   xyz = o + d * depth;  hit = intersection of the line (c, xyz - c) with the plane through P0 with normal -c;
 *   q = A hit + b;  uv = (K (q / q_z) - 0.5) * 2.
 * origins / dirs [P,3], depth [P], uv [P,2]; consts [24] = c[3], P0[3], A[9] (row-major), b[3], K[6] (rows 0..1 of the intrinsics).
 * bwd: gradients w.r.t. origins, dirs and depth from d uv (overwritten). */
int eg3d_warp_project_fwd(const float* origins, const float* dirs, const float* depth, const float* consts, float* uv, int64_t P, void* stream);
int eg3d_warp_project_bwd(const float* origins, const float* dirs, const float* depth, const float* consts, const float* duv, float* d_origins,
                          float* d_dirs, float* d_depth, int64_t P, void* stream);

/* F.grid_sample(input, grid, mode='bilinear', padding_mode='zeros', align_corners=False) for a channels-last input -- the feature warp of the
 * depth-reprojection loss (training/warping_loss.py:50; ATen's kernel takes 152 + 218 us there, this one 6 + 8).
 *   input [N,H,W,C] fp32, C % 4 == 0, 16-byte aligned; grid [N,Ho,Wo,2] (x, y) in [-1,1]; out / dout [N,Ho,Wo,C].
 * bwd: dgrid [N,Ho,Wo,2] is overwritten; dinput (optional, [N,H,W,C], pre-zeroed) is accumulated with atomics. */
int eg3d_grid_sample_nhwc_fwd(const float* input, const float* grid, float* out, int N, int H, int W, int C, int Ho, int Wo, void* stream);
int eg3d_grid_sample_nhwc_bwd(const float* input, const float* grid, const float* dout, float* dgrid, float* dinput, int N, int H, int W, int C, int Ho,
                              int Wo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Marching cubes (shape export) -- replaces skimage.measure.marching_cubes(np.transpose(sigmas, (2,1,0)), level, spacing=[1]*3) in
 *   create_geometry, training/coaches/single_id_coach.py:120-163, and convert_mrc, shape_utils.py:40-100 (csrc/marching_cubes.hip).
 *   vol: contiguous fp32 [D0][D1][D2] (i2 fastest), D0, D1, D2 >= 2, D0*D1*D2 < 2^31, finite values.  A corner is inside iff v > level.
 *   One vertex per grid edge whose ends differ in inside-ness: p = a + t (b - a), t = (level - v_a) / (v_b - v_a) in fp32 (a = the end of
 *   lower linear index); grid point (i0, i1, i2) is the vertex coordinate (i2, i1, i0); written as p * spacing[k] + origin[k].
 *   Faces: int32 triples, right-hand normal toward lower values (a closed surface around a dense blob has positive signed volume).
 *   Order: vertices by (owning grid point = the edge's lower end, axis x, y, z); faces by (cube's min-corner linear index, table order of
 *   csrc/mc_tables.h).  Bit-identical from run to run and between the two builds (no atomics).
 *   Protocol:
 *     eg3d_mc_query_workspace  host only: count workspace bytes, and emit workspace bytes per active point (16-byte aligned buffers)
 *     eg3d_mc_count            fills `workspace` and writes totals[0..3] = (active points A, vertices V, faces F, 0) on the device
 *     (host reads totals: one synchronise; allocates verts [V,3], faces [F,3], emit workspace A * emit_bytes_per_active)
 *     eg3d_mc_emit             writes verts / faces, never beyond vert_capacity / face_capacity rows or the emit workspace
 *   V = F = 0 is a normal result.  A grid of 2^31 points or more, or capacities of 2^31 rows or more: EG3D_ERR_TOO_LARGE (the caller checks
 *   the totals the same way before it allocates).
 */
typedef struct eg3d_mc_params {
    const float* vol;
    int32_t D0, D1, D2;
    float level;
    float origin[3];                   /* per output axis x, y, z; 0 / 1 = the reference's frame */
    float spacing[3];
    void* workspace;                   /* eg3d_mc_query_workspace's count_bytes */
    int64_t workspace_bytes;
    int64_t* totals;                   /* device int64[4] */
    void* emit_workspace;              /* A x emit_bytes_per_active */
    int64_t emit_workspace_bytes;
    float* verts;                      /* [vert_capacity, 3] */
    int64_t vert_capacity;
    int32_t* faces;                    /* [face_capacity, 3] */
    int64_t face_capacity;
} eg3d_mc_params;
int eg3d_mc_query_workspace(const eg3d_mc_params* p, int64_t* count_bytes, int64_t* emit_bytes_per_active);
int eg3d_mc_count(const eg3d_mc_params* p, void* stream);
int eg3d_mc_emit(const eg3d_mc_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Shape views: first-hit iso-surface ray marcher over a regular fp32 grid (csrc/iso_render.hip).  No reference counterpart (the reference
 *   only writes .mrc / .ply for an external viewer).
 *   vol: contiguous fp32 [D0][D1][D2] as for marching cubes, D >= 2, D0*D1*D2 < 2^31.  Grid index i on grid axis a sits at world coordinate
 *   origin[a] + i * spacing[a] of WORLD axis axes[a] (axes: a permutation of 0,1,2; spacing != 0, may be negative).  Inside iff v > level;
 *   NaN never hits.
 *
 * eg3d_iso_bricks (one launch): bricks [B0][B1][B2], B_a = (D_a + 6) / 8; entry b = max of vol over i_a in [8 b_a - 1, 8 b_a + 9] clamped to
 *   the grid (the brick's corner range dilated by one voxel), NaN ignored (-inf when all are NaN), + 0.0f.  Independent of the level.
 *
 * eg3d_iso_render (one launch, one wave per 8 x 8 pixel tile): exactly these fp32 operations in this order, no contraction (the library is
 *   built with -ffp-contract=off); tests/support/iso_ref.py restates them in numpy and the outputs are compared bit for bit.
 *   Ray of pixel (y, x) of camera c[25] (m = c[0..15] row-major cam2world, fx = c[16], sk = c[17], cx = c[18], fy = c[20], cy = c[21]):
 *     xc = (x + 0.5) / res, yc = (y + 0.5) / res;  xl = (((xc - cx) + (cy * sk) / fy) - (sk * yc) / fy) / fx;  yl = (yc - cy) / fy
 *     w_i = ((m_i0 * xl + m_i1 * yl) + m_i2) + m_i3;  o_i = m_i3;  e_i = w_i - o_i;  d_i = e_i / sqrt((e_0^2 + e_1^2) + e_2^2)
 *   Index coordinates, per grid axis a (w = axes[a]):  oi_a = (o_w - origin_a) / spacing_a,  di_a = d_w / spacing_a,  h_a = D_a - 1.
 *   Slabs, tn = 0, tf = +inf:  di_a == 0: the ray is empty unless 0 <= oi_a <= h_a;  else t0 = (0 - oi_a) / di_a, t1 = (h_a - oi_a) / di_a,
 *     tn = max(tn, min(t0, t1)), tf = min(tf, max(t0, t1)), all by explicit comparisons.  Empty or not (tf >= tn): a miss.
 *   dt = step * min |spacing_a|;  K = min(floor((tf - tn) / dt), 2^24);  t_k = tn + float(k) * dt, k = 0..K.
 *   Field at t: p_a = clamp(oi_a + t * di_a, 0, h_a) (p > 0 ? p : 0, then p < h ? p : h);  i_a = min(int(floor(p_a)), D_a - 2);
 *     f_a = p_a - float(i_a);  lerp(a, b, f) = a + f * (b - a) clamped to [min(a, b), max(a, b)] (so the interpolant never leaves the range of
 *     its corners, in fp32 too);  lerps along axis 2, then axis 1, then axis 0.
 *   Hit: the first k with field(t_k) > level.  k = 0: t = tn.  Otherwise ta = t_{k-1}, fa = field(ta), tb = t_k, fb = field(tb); `refine` times
 *     tm = ta + (tb - ta) * 0.5, (fm > level ? (tb, fb) : (ta, fa)) = (tm, fm);  t = ta + (tb - ta) * ((level - fa) / (fb - fa)), replaced by tb
 *     unless ta <= t <= tb.
 *   Skipping (skip != 0): a sample whose cell (i_0 >> 3, i_1 >> 3, i_2 >> 3) has bricks[...] <= level is not evaluated; with
 *     te = min over axes with di_a != 0 of ((di_a > 0 ? 8 b_a + 8 : 8 b_a) - oi_a) / di_a and q = floor((te - tn) / dt), the next k is
 *     q > k + 1 ? min(q, K + 1) : k + 1.  Every skipped sample lies in the brick up to rounding (far less than the one-voxel dilation) and
 *     the interpolant is bounded by its corners: no skipped sample exceeds the level, so every output is bit-identical with skip = 0.
 *   Normal at the hit: per grid axis g_a = (field(p with p_a + 1 clamped) - field(p with p_a - 1 clamped)) / ((p_a^+ - p_a^-) * spacing_a);
 *     n_w = -g_a for w = axes[a];  n / sqrt((n_0^2 + n_1^2) + n_2^2) when that length is > 0, else 0.
 *   Outputs (each may be NULL): depth [F][res][res] = t (world units along the unit ray), 0 on a miss;  normal [F][res][res][3] world space, 0
 *     on a miss;  mask uint8 [F][res][res];  hit_k int32 [F][res][res], -1 on a miss;  shade [F][3][res][res] in [-1, 1]:
 *     EG3D_ISO_LAMBERT  v = ambient + (1 - ambient) * max(0, -((n_0 d_0 + n_1 d_1) + n_2 d_2)), the three channels = v * 2 - 1
 *     EG3D_ISO_NORMAL   channel j = ((m_0j n_0 + m_1j n_1) + m_2j n_2) * 0.5 + 0.5, then * 2 - 1
 *     a miss takes `background` (already in [-1, 1]).
 *   No atomics, no floating-point sum whose order depends on the launch: bit-identical between runs and between the two builds.
 *   Errors, before any launch: EG3D_ERR_INVALID (null vol / cams, no bricks with skip, D < 2, F or res < 1, axes no permutation, spacing 0 or
 *   not finite, level / origin not finite, step outside [1/64, 64], refine outside 0..32, ambient outside [0, 1], unknown shade mode),
 *   EG3D_ERR_TOO_LARGE (grid of 2^31 points or more), EG3D_ERR_UNSUPPORTED (res > 16384 or F > 65535).
 */
#define EG3D_ISO_LAMBERT 0
#define EG3D_ISO_NORMAL 1
typedef struct eg3d_iso_params {
    const float* vol;                  /* [D0][D1][D2] */
    float* bricks;                     /* [B0][B1][B2]: written by eg3d_iso_bricks, read by eg3d_iso_render when skip != 0 */
    const float* cams;                 /* [F][25] */
    float* depth;                      /* [F][res][res] or NULL */
    float* normal;                     /* [F][res][res][3] or NULL */
    uint8_t* mask;                     /* [F][res][res] or NULL */
    int32_t* hit_k;                    /* [F][res][res] or NULL */
    float* shade;                      /* [F][3][res][res] or NULL */
    int32_t D0, D1, D2;
    int32_t F, res;
    int32_t axes[3];                   /* world axis of each grid axis */
    float origin[3];                   /* per grid axis */
    float spacing[3];                  /* per grid axis, signed */
    float level;
    float step;                        /* sample distance in units of min |spacing| */
    int32_t refine;                    /* bisection halvings before the secant step */
    int32_t skip;                      /* 0 = march every sample */
    int32_t shade_mode;                /* EG3D_ISO_LAMBERT | EG3D_ISO_NORMAL */
    float ambient;
    float background;
} eg3d_iso_params;
int eg3d_iso_bricks(const eg3d_iso_params* p, void* stream);
int eg3d_iso_render(const eg3d_iso_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh attributes: per-vertex normals of the density field and view-baked vertex colours (csrc/mesh_bake.hip).  No reference counterpart
 *   (the reference's meshes carry x y z and faces only).  One thread per vertex, no atomics, the views walked in index order: bit-identical
 *   between runs and between the two builds.  Exactly these fp32 operations in this order, no contraction; tests/support/mesh_ref.py restates
 *   them in numpy and the outputs are compared bit for bit.
 *
 * eg3d_mesh_normals (one launch): the unit normal of the trilinear field of vol at points [V][3] (world coordinates).  vol, origin, spacing and
 *   axes as in eg3d_iso_params.  Per grid axis a: r_a = (x_{axes[a]} - origin_a) / spacing_a, h_a = D_a - 1.  If any r_a is NaN the normal is 0.
 *   Otherwise p_a = clamp(r_a, 0, h_a), and with field(), clamp and lerp as "Shape views" defines them, per grid axis
 *     g_a = (field(p with p_a + 1 clamped) - field(p with p_a - 1 clamped)) / ((p_a^+ - p_a^-) * spacing_a);  n_w = -g_a for w = axes[a];
 *     len = sqrt((n_0^2 + n_1^2) + n_2^2);  normal = n / len when 0 < len < inf, else 0 (a NaN or infinite component makes len NaN or inf).
 *   The normal points toward lower values: out of the dense region.
 *   Errors, before any launch: EG3D_ERR_INVALID (null vol, null points / normals with V > 0, V < 0, D < 2, axes no permutation, spacing 0 or not
 *   finite, origin not finite), EG3D_ERR_TOO_LARGE (grid of 2^31 points or more, V >= 2^31).  V = 0: ok, no launch.
 *
 * eg3d_mesh_bake (one launch): the colour of vertex p (normal n) blended from F rendered views.  images fp32 [F][3][H][H] in [-1, 1]; depth
 *   fp32 [F][R][R] and mask uint8 [F][R][R] as eg3d_iso_render writes them for the same cameras (R need not equal H).
 *   acc = 0, wsum = 0, views = 0; for f = 0 .. F-1, camera c[25] named as in "Shape views" (m row-major cam2world, o_i = m_i3):
 *   1. q_i = p_i - o_i;  t = sqrt((q_0^2 + q_1^2) + q_2^2);  c_j = (m_0j q_0 + m_1j q_1) + m_2j q_2, j = 0, 1, 2.
 *      Skip the view unless t > 0 and c_2 > 0 (the camera looks down +z of its own frame).
 *   2. xl = c_0 / c_2, yl = c_1 / c_2;  yc = yl * fy + cy;  xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy  (the inverse of the ray
 *      lift).  At a resolution r: px = xc * float(r) - 0.5, py = yc * float(r) - 0.5, formed for r = H and for r = R.
 *      Skip unless 0 <= px <= r - 1 and 0 <= py <= r - 1 at both resolutions (explicit comparisons: NaN skips).
 *   3. Visibility: x0 = int(floor(px_R)), x1 = min(x0 + 1, R - 1), y0, y1 likewise.  Skip unless one of the pixels (y0,x0), (y0,x1), (y1,x0),
 *      (y1,x1) of view f has mask != 0 and t <= depth + depth_tol.
 *   4. c = -((n_0 q_0 + n_1 q_1) + n_2 q_2) / t.  Skip unless c > cos_min.  w = c, then w = w * c, power - 1 times.
 *   5. H >= 2: bx = min(int(floor(px_H)), H - 2), by likewise, tx = px_H - float(bx), ty = py_H - float(by), lerp(a, b, f) = a + f * (b - a)
 *      (not clamped);  colour_j = lerp(lerp(I[by][bx], I[by][bx+1], tx), lerp(I[by+1][bx], I[by+1][bx+1], tx), ty) of channel j.  H = 1: the
 *      single texel.  acc_j = acc_j + w * colour_j;  wsum = wsum + w;  views = min(views + 1, 255).
 *   Outputs (each may be NULL): color fp32 [V][3] = acc_j / wsum when wsum > 0, else fallback [V][3] (0 without one);  rgb uint8 [V][3] =
 *     uint8(int(min(max(color * 127.5 + 128, 0), 255))) as eg3d_image_grid_u8;  weight fp32 [V] = wsum;  views uint8 [V].
 *   Errors, before any launch: EG3D_ERR_INVALID (null cams / images / depth / mask, null points / normals with V > 0, V < 0, F, H or R < 1,
 *   depth_tol negative or not finite, cos_min outside [0, 1), power outside 1..8), EG3D_ERR_UNSUPPORTED (F > 255, H or R > 16384),
 *   EG3D_ERR_TOO_LARGE (V >= 2^31).  V = 0: ok, no launch.
 */
typedef struct eg3d_mesh_normals_params {
    const float* vol;                  /* [D0][D1][D2] */
    const float* points;               /* [V][3] world */
    float* normals;                    /* [V][3] world */
    int64_t V;
    int32_t D0, D1, D2;
    int32_t axes[3];                   /* world axis of each grid axis */
    float origin[3];                   /* per grid axis */
    float spacing[3];                  /* per grid axis, signed */
} eg3d_mesh_normals_params;
typedef struct eg3d_mesh_bake_params {
    const float* points;               /* [V][3] world */
    const float* normals;              /* [V][3] world */
    const float* cams;                 /* [F][25] */
    const float* images;               /* [F][3][H][H] */
    const float* depth;                /* [F][R][R] */
    const uint8_t* mask;               /* [F][R][R] */
    const float* fallback;             /* [V][3] or NULL */
    float* color;                      /* [V][3] or NULL */
    uint8_t* rgb;                      /* [V][3] or NULL */
    float* weight;                     /* [V] or NULL */
    uint8_t* views;                    /* [V] or NULL */
    int64_t V;
    int32_t F, H, R;
    float depth_tol;                   /* world units, >= 0 */
    float cos_min;                     /* in [0, 1) */
    int32_t power;                     /* 1..8 */
} eg3d_mesh_bake_params;
int eg3d_mesh_normals(const eg3d_mesh_normals_params* p, void* stream);
int eg3d_mesh_bake(const eg3d_mesh_bake_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh texture: a per-face texture atlas baked from the views (csrc/mesh_bake.hip, beside the vertex bake whose view loop it calls).  No
 *   reference counterpart.  One thread per texel, every texel a function of its own face: bit-identical between runs and between the two
 *   builds.  Exactly these fp32 operations in this order, no contraction; tests/support/texture_ref.py restates them in numpy and the outputs
 *   are compared bit for bit.  V vertices, F faces (int32 [F][3]), N views; T = tile, an integer in [4, 64].
 *
 * Layout (eg3d_mesh_texture_size, host only).  Faces 2b and 2b + 1 share block b, a T x T square of texels.  nb = max(ceil(F / 2), 1);
 *   per_row = ceil(sqrt(nb)) (integers);  Wt = T * per_row;  Ht = T * ceil(nb / per_row).  Block b sits at column b % per_row, row
 *   b / per_row of the atlas; texel (i, j) of a block (i along x, j along y, origin top-left) is atlas texel (x, y) = (T * column + i,
 *   T * row + j).  The even face (lower) owns the texels with i + j <= T - 1, the odd face (upper) those with i + j >= T.  A texel whose
 *   face index is >= F (the upper half of a last block, F = 0) holds `fill` in its three channels and 0 views.
 * Corner order.  Corner k of a face has vertex index f_k and position v_k.  e_0 = |v_2 - v_1|^2, e_1 = |v_0 - v_2|^2, e_2 = |v_1 - v_0|^2,
 *   each (dx*dx + dy*dy) + dz*dz of the component differences (the edge opposite corner k).  r = 0;  r = 1 if e_1 > e_r;  r = 2 if e_2 > e_r
 *   (a NaN compares false; ties keep the lower corner).  A_0, A_1, A_2 = corners r, (r + 1) % 3, (r + 2) % 3: cyclic, the winding is kept,
 *   and the corner opposite the longest edge takes the right angle of the texel triangle.
 * Texel triangle (block-local texel centres): lower A_0 (0, 0), A_1 (T - 2, 0), A_2 (0, T - 2); upper A_0 (T - 1, T - 1), A_1 (2, T - 1),
 *   A_2 (T - 1, 2).  A bilinear lookup inside a face's triangle (edges included) reads only texels the face owns.
 * Per texel.  Lower: b_1 = float(i) / float(T - 2), b_2 = float(j) / float(T - 2).  Upper: b_1 = float(T - 1 - i) / float(T - 3),
 *   b_2 = float(T - 1 - j) / float(T - 3).  b_0 = (1 - b_1) - b_2 (negative on the owned texels beyond the hypotenuse: extrapolation in the
 *   face's plane, so no dilation pass).  Position, normal (not renormalised) and fallback colour, per component: (b_0 A_0 + b_1 A_1) + b_2 A_2
 *   of the three vertices' values.  The point and normal go through steps 1-5 of eg3d_mesh_bake's view loop (the same device function);
 *   colour = acc_j / wsum when wsum > 0, else the interpolated fallback (0 without one);  texture = uint8(int(min(max(colour * 127.5 + 128,
 *   0), 255)));  views = the loop's count.  At a triangle corner of a face with finite vertices b is (1, 0, 0), (0, 1, 0) or (0, 0, 1)
 *   and the texel is eg3d_mesh_bake's rgb and views of that vertex.
 * uv [F][3][2]: for corner k of face f in the face's ORIGINAL order, with (x, y) the atlas texel of the triangle corner it was rotated to
 *   (corner k is A_((k - r) mod 3)):  u = (float(x) + 0.5) / float(Wt),  v = (float(y) + 0.5) / float(Ht);  origin top-left.
 *   corner uint8 [F] = r.
 * A face with an index outside [0, V): no vertex of it is read; its texels hold `fill` and 0 views, r = 0 (uv as for r = 0), and
 *   *bad_faces (device int32, cleared by a launch on the same stream, may be NULL) counts such faces -- an integer atomic add on this path
 *   only; no output depends on it.  The caller reads it with one synchronise and discards the result when it is not 0.
 * Outputs (each may be NULL and is then left alone): texture uint8 [Ht][Wt][3], views uint8 [Ht][Wt], uv, corner.  With all of them and
 *   bad_faces NULL: ok, no launch.  Otherwise one launch over the Ht * Wt texels (plus the counter's), F = 0 included.
 * Errors, before any launch: EG3D_ERR_INVALID (null params / cams / images / depth / mask, null points / normals with V > 0, null faces with
 *   F > 0, V or F < 0, N, H or R < 1, depth_tol negative or not finite, cos_min outside [0, 1), power outside 1..8, tile outside [4, 64],
 *   fill outside 0..255), EG3D_ERR_UNSUPPORTED (N > 255, H or R > 16384, an atlas side above 16384), EG3D_ERR_TOO_LARGE (V or F >= 2^31).
 */
typedef struct eg3d_mesh_texture_params {
    const float* points;               /* [V][3] world */
    const float* normals;              /* [V][3] world */
    const int32_t* faces;              /* [F][3] */
    const float* cams;                 /* [N][25] */
    const float* images;               /* [N][3][H][H] */
    const float* depth;                /* [N][R][R] */
    const uint8_t* mask;               /* [N][R][R] */
    const float* fallback;             /* [V][3] or NULL */
    uint8_t* texture;                  /* [Ht][Wt][3] or NULL */
    uint8_t* views;                    /* [Ht][Wt] or NULL */
    float* uv;                         /* [F][3][2] or NULL */
    uint8_t* corner;                   /* [F] or NULL */
    int32_t* bad_faces;                /* device int32[1] or NULL */
    int64_t V, F;
    int32_t N, H, R;
    int32_t tile;                      /* 4..64 */
    int32_t fill;                      /* 0..255 */
    float depth_tol;                   /* world units, >= 0 */
    float cos_min;                     /* in [0, 1) */
    int32_t power;                     /* 1..8 */
} eg3d_mesh_texture_params;
int eg3d_mesh_texture_size(int64_t F, int32_t tile, int32_t* Ht, int32_t* Wt);
int eg3d_mesh_texture(const eg3d_mesh_texture_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh previews: a z-buffer rasteriser for the exported meshes (csrc/mesh_raster.hip).  No reference counterpart (the reference has no
 *   mesh renderer).  It takes the mesh as the exporters hold it (world points, int32 faces, eg3d_mesh_texture's uv and atlas, eg3d_mesh_bake's
 *   colours, eg3d_mesh_normals' normals) and the generator's cameras, and its frames register pixel for pixel with eg3d_iso_render's and with
 *   the generator's images.  Exactly these fp32 and integer operations in this order, no contraction; tests/support/raster_ref.py restates them
 *   in numpy and the outputs are compared bit for bit.  The only atomics are integer ones (a 64-bit unsigned minimum per covered pixel, and
 *   integer adds on counters and a queue no output depends on): every output is a function of the inputs alone, bit-identical between runs and
 *   between the two builds.  V vertices, F faces, N views, res x res pixels; camera c[25] named as in "Shape views".
 *
 * Vertex stage, per view and vertex p:
 *   q_i = p_i - o_i;  c_j = (m_0j q_0 + m_1j q_1) + m_2j q_2;  xl = c_0 / c_2, yl = c_1 / c_2;  yc = yl * fy + cy;
 *   xc = ((xl * fx + cx) - (cy * sk) / fy) + (sk * yc) / fy   (steps 1-2 of eg3d_mesh_bake without t);
 *   px = xc * float(res) - 0.5, py = yc * float(res) - 0.5   (pixel (y, x) has its centre at px = x, py = y).
 *   valid iff c_2 > near and -32768 <= px <= 32768 and -32768 <= py <= 32768 (explicit comparisons: a NaN is invalid).
 *   X = int32(floor(px * 256 + 0.5)), Y = int32(floor(py * 256 + 0.5))   (8 sub-pixel bits);  z = c_2.
 * Face stage, per view and face f with corners S_k = (X_k, Y_k), z_k:
 *   orient(A, B, P) = (B_x - A_x) * (P_y - A_y) - (B_y - A_y) * (P_x - A_x) in int64 (|coordinate| <= 2^23 + 1: no overflow).
 *   Dropped: an index outside [0, V) (no vertex of the face is read; counted once per face in *bad_faces, a device int32 that may be NULL);
 *   a vertex invalid in this view (nothing is clipped);  area2 = orient(S_0, S_1, S_2) = 0;  with cull = 1, area2 > 0.
 *   Front faces have area2 < 0: with a proper-rotation cam2world the camera frame (x right, y down, z forward) is right-handed and px, py grow
 *   with x, y (fx, fy > 0), so a face whose right-hand normal (v_1 - v_0) x (v_2 - v_0) points at the camera -- e.g. (0,0,1), (0,1,1), (1,0,1)
 *   in camera coordinates, normal (0,0,-1) -- has area2 = 0 * 0 - 1 * 1 < 0.
 *   Pixels x in [max(ceil(min_k X_k / 256), 0), min(floor(max_k X_k / 256), res - 1)], y likewise (an empty range drops the face).  P = (256 x,
 *   256 y);  E_0 = orient(S_1, S_2, P), E_1 = orient(S_2, S_0, P), E_2 = orient(S_0, S_1, P), each negated when area2 < 0.  Covered iff all
 *   three are >= 0 (edges inclusive: a shared edge leaves no hole; the depth test settles the doubly covered pixels).
 *   l_k = float(E_k) / float(|area2|) (int64 to fp32, round to nearest even);  w_k = l_k / z_k;  W = (w_0 + w_1) + w_2;  kept iff 0 < W < inf;
 *   zp = 1 / W;  key = (uint64(bits(zp)) << 32) | f;  the pixel's uint64, all ones at the start, takes the minimum of the keys: the nearest face
 *   wins, equal depth goes to the lower face index, in whatever order the faces arrive (one 64-bit unsigned atomic minimum).
 * Resolve stage, per pixel: all ones is a miss.  Otherwise f = the low 32 bits, w_k and W as above, zp = 1 / W, b_k = w_k / W.
 *   Ray lift of pixel (y, x) as eg3d_iso_render forms it: xc = (x + 0.5) / res, yc = (y + 0.5) / res;
 *   xl = (((xc - cx) + (cy * sk) / fy) - (sk * yc) / fy) / fx;  yl = (yc - cy) / fy;  w_i, e_i, d_i as there.
 *   mix(A) = (b_0 A_0 + b_1 A_1) + b_2 A_2 of the three corners' values, per component.
 *   Outputs (each may be NULL): face int32 [N][res][res], -1 on a miss;  z fp32 [N][res][res] = zp, 0 on a miss;  depth fp32 [N][res][res] =
 *   zp * sqrt((xl^2 + yl^2) + 1), the distance along the unit ray that eg3d_iso_render's depth measures, 0 on a miss;  mask uint8 [N][res][res];
 *   bary fp32 [N][res][res][3] = b, 0 on a miss;  image fp32 [N][3][res][res] in [-1, 1], `background` on a miss:
 *     EG3D_RASTER_TEXTURE  (u, v) = mix of uv [F][3][2] rows of face f;  tx = clamp(u * float(Wt) - 0.5, 0, Wt - 1) (p > 0 ? p : 0, then p < h ?
 *                          p : h: NaN gives 0), ty with Ht;  x0 = min(int(floor(tx)), Wt - 2), fx = tx - float(x0), y0, fy likewise;
 *                          lerp(a, b, f) = a + f * (b - a) (not clamped) over the uint8 texels of texture [Ht][Wt][3] converted to float:
 *                          colour_j = lerp(lerp(T[y0][x0], T[y0][x0+1], fx), lerp(T[y0+1][x0], T[y0+1][x0+1], fx), fy);
 *                          image_j = (colour_j - 127.5) / 127.5
 *     EG3D_RASTER_VERTEX   image_j = mix of colors [V][3], column j
 *     EG3D_RASTER_LAMBERT  n = mix of normals [V][3];  len = sqrt((n_0^2 + n_1^2) + n_2^2);  n = n / len when 0 < len < inf, else 0;
 *                          s = -((n_0 d_0 + n_1 d_1) + n_2 d_2);  v = ambient + (1 - ambient) * (s > 0 ? s : 0);  the three channels = v * 2 - 1
 *   stats (device int32[2], may be NULL): [0] = (view, face) pairs drawn one per lane, [1] = pairs drawn by a workgroup.
 * Work distribution: a (view, face) pair whose pixel range is at most EG3D_RASTER_SMALL pixels wide and high is drawn by its own lane; a
 *   larger one is queued and drawn by a workgroup, one lane per pixel of 8 x 8 tiles.  The split changes no output.
 * Workspace (lent by the caller; the library allocates nothing): eg3d_mesh_raster_query_workspace, host only, from V, F, N, res: the
 *   z-buffer (8 bytes a pixel), the projected vertices (16 bytes per view and vertex), the queue (8 bytes per view and face), the counters.
 *   16-byte aligned.  With every output, bad_faces and stats NULL: ok, no launch.  F = 0 is ok: every pixel is a miss.
 * Errors, before any launch: EG3D_ERR_INVALID (null params / cams / workspace, null points with V > 0, null faces with F > 0, null texture,
 *   or null uv with F > 0, in texture mode, null colors / normals with V > 0 in their mode, V or F < 0, N or res < 1, near <= 0 or not
 *   finite, unknown mode or cull, ambient outside [0, 1], a texture side < 2, a short or misaligned workspace), EG3D_ERR_UNSUPPORTED (res >
 *   16384, N > 65535, a texture side > 16384), EG3D_ERR_TOO_LARGE (V or F >= 2^31, N * F >= 2^31: render the views in batches).
 */
#define EG3D_RASTER_TEXTURE 0
#define EG3D_RASTER_VERTEX 1
#define EG3D_RASTER_LAMBERT 2
#define EG3D_RASTER_SMALL 8
typedef struct eg3d_mesh_raster_params {
    const float* points;               /* [V][3] world */
    const int32_t* faces;              /* [F][3] */
    const float* cams;                 /* [N][25] */
    const float* uv;                   /* [F][3][2]: texture mode */
    const uint8_t* texture;            /* [Ht][Wt][3]: texture mode */
    const float* colors;               /* [V][3]: vertex mode */
    const float* normals;              /* [V][3] world: lambert mode */
    int32_t* face;                     /* [N][res][res] or NULL */
    float* z;                          /* [N][res][res] or NULL */
    float* depth;                      /* [N][res][res] or NULL */
    uint8_t* mask;                     /* [N][res][res] or NULL */
    float* bary;                       /* [N][res][res][3] or NULL */
    float* image;                      /* [N][3][res][res] or NULL */
    int32_t* bad_faces;                /* device int32[1] or NULL */
    int32_t* stats;                    /* device int32[2] or NULL */
    void* workspace;                   /* eg3d_mesh_raster_query_workspace's bytes */
    int64_t workspace_bytes;
    int64_t V, F;
    int32_t N, res;
    int32_t Ht, Wt;                    /* texture mode */
    int32_t mode;                      /* EG3D_RASTER_TEXTURE | _VERTEX | _LAMBERT */
    int32_t cull;                      /* 0 none, 1 back faces */
    float near;                        /* camera-space depth a vertex must exceed, > 0 */
    float background;
    float ambient;
} eg3d_mesh_raster_params;
int eg3d_mesh_raster_query_workspace(const eg3d_mesh_raster_params* p, int64_t* workspace_bytes);
int eg3d_mesh_raster(const eg3d_mesh_raster_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grid components: connected-component labelling of {vol > level} and removal of components (csrc/grid_components.hip).  No reference
 *   counterpart (the reference exports every blob above the level).  tests/support/cc_ref.py restates the result in numpy; the outputs are
 *   compared exactly.
 *   vol: contiguous fp32 [D0][D1][D2] (i2 fastest), D0, D1, D2 >= 1, D0*D1*D2 < 2^31.  A voxel is inside iff v > level, the rule of marching
 *   cubes and of the ray marcher: NaN is outside, v == level is outside, +inf is inside.  Two inside voxels are adjacent when their indices
 *   differ by at most one on every axis and, with connectivity 6, on exactly one axis (faces); with 26 on one, two or three (faces, edges,
 *   corners).  A component is a class of the transitive closure.
 *   Result: labels int32 [D0][D1][D2]: 0 outside; inside 1..K, the components numbered in ascending order of their smallest linear index
 *   ((i0 * D1 + i1) * D2 + i2: raster order of first appearance).  roots int32 [K]: that smallest index.  sizes int32 [K]: voxels.
 *   totals int64[2] on the device = (K, inside voxels).  The result is a function of (vol, level, connectivity) alone: integer arithmetic,
 *   and although the merge is lock-free and its intermediate trees depend on the schedule, the partition, each component's smallest index
 *   and the integer sums do not.  Bit-identical between runs and between the two builds.
 *   Protocol (workspace lent by the caller; the library allocates nothing):
 *     eg3d_cc_query_workspace  host only: workspace bytes (a parent volume of one int32 per voxel, plus the scan's counters)
 *     eg3d_cc_label            passes (a)-(d) below; writes totals
 *     (host reads totals: one synchronise; allocates sizes [K], roots [K]; sets count = K)
 *     eg3d_cc_finish           passes (e), (f): writes labels, sizes, roots.  count = 0 (K = 0, a normal result): labels are zero-filled, no
 *                              launch of (e) or (f).  A count below K truncates roots / sizes (never written beyond count entries).
 *   Passes (tile = EG3D_CC_TILE0 x EG3D_CC_TILE1 x EG3D_CC_TILE2 voxels, one workgroup each; chunk = 4096 consecutive voxels):
 *     (a) per tile: occupancy and a union-find over the tile's own adjacencies in LDS; parent[v] = linear index of the smallest voxel of v's
 *         component within the tile (v itself for that voxel: a local root), -1 outside.  16-byte loads and stores when D2 % 4 == 0.
 *     (b) per tile: every inside voxel with a forward neighbour (higher linear index) in another tile unites the two sets: find both roots,
 *         compare-and-swap the larger root's parent from itself to the smaller, on failure continue from the value returned.
 *     (c) per chunk: count roots (parent[v] == v) and inside voxels.            (d) one workgroup: exclusive scan over the chunks, totals.
 *     (e) per chunk: each root takes rank = chunk offset + its place in the chunk; parent[root] = -2 - rank; roots[rank] = root.
 *     (f) per tile: every inside voxel walks to its root, labels[v] = rank + 1; voxel counts are summed in LDS per local root and added to
 *         sizes with one atomic per local root.
 *   Rules of the device code (gfx950: per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores):
 *     - in (b) every access to a parent word is an agent-scope atomic (__hip_atomic_load relaxed, atomicMin, atomicCAS), never a plain load or
 *       store.  A stale value would still be harmless: every value a parent word ever held is an ancestor of the voxel in the final forest;
 *     - (b) writes only parent words of local roots; every other pass reads only what an earlier launch wrote, or its own writes;
 *     - no workgroup waits for another: no flags, no spin loops, no grid barriers.  Every loop over parents ends because a parent is
 *       strictly smaller than its child, and every retry of a union continues from a strictly smaller index;
 *     - counters are cleared by a kernel on the same stream.
 *   Errors, before any launch: EG3D_ERR_INVALID (null params / vol / labels / workspace / totals, any D < 1, connectivity not 6 or 26, short
 *   workspace, count < 0, null sizes / roots with count > 0), EG3D_ERR_TOO_LARGE (2^31 voxels or more).
 *
 * eg3d_cc_keep (one streaming launch): out[i] = (l = labels[i]; l < 1 || l > count || keep[l]) ? vol[i] : fill.  keep: uint8 [count + 1];
 *   entry 0 is never read, the outside stays as it was (NaN included).  out may alias vol.  Errors: EG3D_ERR_INVALID (null params / vol /
 *   labels / out, null keep with count > 0, any D < 1, count < 0), EG3D_ERR_TOO_LARGE.
 */
#define EG3D_CC_TILE0 8
#define EG3D_CC_TILE1 8
#define EG3D_CC_TILE2 64
typedef struct eg3d_cc_params {
    const float* vol;                  /* [D0][D1][D2] */
    int32_t* labels;                   /* [D0][D1][D2] */
    int32_t D0, D1, D2;
    float level;
    int32_t connectivity;              /* 6 | 26 */
    int32_t count;                     /* K: eg3d_cc_finish, eg3d_cc_keep */
    void* workspace;                   /* eg3d_cc_query_workspace's bytes; carries the state from eg3d_cc_label to eg3d_cc_finish */
    int64_t workspace_bytes;
    int64_t* totals;                   /* device int64[2] */
    int32_t* sizes;                    /* [count] */
    int32_t* roots;                    /* [count] */
    const uint8_t* keep;               /* [count + 1] */
    float* out;                        /* [D0][D1][D2] */
    float fill;
} eg3d_cc_params;
int eg3d_cc_query_workspace(const eg3d_cc_params* p, int64_t* workspace_bytes);
int eg3d_cc_label(const eg3d_cc_params* p, void* stream);
int eg3d_cc_finish(const eg3d_cc_params* p, void* stream);
int eg3d_cc_keep(const eg3d_cc_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh simplification and smoothing: vertex clustering (Rossignac-Borrel, mean placement) and Taubin lambda|mu passes
 *   (csrc/mesh_simplify.hip).  No reference counterpart (the reference's PLYs carry every marching-cubes triangle).  One thread per vertex,
 *   cluster or face; no atomics; every floating-point sum has a fixed order: the outputs are functions of the inputs alone, bit-identical
 *   between runs and between the two builds.  Exactly these operations in this order, no contraction; tests/support/simplify_ref.py restates
 *   them in numpy and the outputs are compared bit for bit.  V, F <= INT32_MAX.
 *
 * Simplify.  verts fp32 [V][3], faces int32 [F][3], cell fp32 > 0, origin fp32[3].
 *   1. Cell of vertex v, column k: c_k = floorf(__fdiv_rn(__fsub_rn(v_k, origin_k), cell)).  v is valid when 0 <= c_k < 2^21 for the three
 *      columns (NaN and the infinities are not).
 *   2. key(v) = c_2 * 2^42 + c_1 * 2^21 + c_0 (int64; column 2 slowest: the order in which eg3d_mc_emit lays vertices out).
 *   3. Clusters = the distinct keys in ascending order; id(v) = the rank of key(v); K of them.
 *   4. Position of a cluster, per column: s = 0.0; for the members in ascending v: s = s + (double)v_k (fp64); (float)(s / (double)n).
 *   5. Faces: g = id[f].  A face with two equal ids dies.  The triple is rotated so that its smallest id comes first (winding kept).  A face
 *      dies if a face of lower index survived with the same rotated triple (the oppositely wound triple is another face).  Survivors keep
 *      their relative order.
 *   6. Clusters no surviving face references are removed; the others keep ascending key order and are renumbered from 0, and the faces with
 *      them.  vertex_map int32 [V] = the new index of the vertex's cluster, or -1.
 *   V = 0 or F = 0 is a normal result (F = 0: no faces, no vertices, vertex_map all -1).
 *   flags int32[2] on the device: [0] != 0 when a vertex is invalid, [1] != 0 when a face index lies outside [0, V) (such an index is never
 *   dereferenced; the face dies).  The caller reads them with the counts and discards the result when one is set.
 *   Protocol (the caller sorts and scans between the entries; every sorted or added value is an integer, so those steps are unique too):
 *     eg3d_simplify_query_workspace  host only: bytes of the workspace (ids, segment starts, cluster positions), carried from _clusters to _emit
 *     eg3d_simplify_keys      clears flags; keys[v] = key(v), INT64_MAX for an invalid vertex (flagged)
 *     (caller: stable ascending sort of keys -> sorted_keys, order: the members of a cluster are adjacent, in ascending v)
 *     eg3d_simplify_heads     heads[i] = 1 where sorted_keys[i] opens a cluster, else 0
 *     (caller: head_scan = inclusive prefix sum of heads, int32: rank + 1 of every sorted position; head_scan[V-1] = K)
 *     eg3d_simplify_clusters  ids and segment starts; one thread per cluster walks its segment (step 4); tri [3][F] (planar: column k of face f
 *                             at tri[k * F + f]) = the rotated id triples, (-1, -1, -1) for a face with a bad index; alive[f] = 1 unless the
 *                             face is degenerate or bad; used[0..V) cleared
 *     (caller: face_order = the faces sorted by (tri column 0, 1, 2, index), e.g. three stable sorts by column 2, 1, 0)
 *     eg3d_simplify_mark      alive[face_order[j]] = 0 where its triple equals that of face_order[j-1]; then used[g] = 1 for the ids of
 *                             the faces still alive
 *     (caller: alive_scan, used_scan = inclusive prefix sums, int32; reads flags, K, F' = alive_scan[F-1], V' = used_scan[V-1]: the one
 *      synchronise; allocates out_verts [V'][3], out_faces [F'][3])
 *     eg3d_simplify_emit      out_faces[alive_scan[f] - 1][k] = used_scan[tri_k[f]] - 1 for alive f; out_verts[used_scan[c] - 1] = position
 *                             of used cluster c; vertex_map.  Never writes beyond the capacities.
 *   Errors, before any launch: EG3D_ERR_INVALID (null params, V or F < 0, cell <= 0 or not finite, origin not finite [_keys], a null pointer
 *   among those the entry uses while its count is > 0, short workspace, negative capacity), EG3D_ERR_TOO_LARGE (V, F or a capacity > INT32_MAX).
 *
 * Smooth (eg3d_smooth): Taubin smoothing with uniform (umbrella) weights over a CSR adjacency the caller builds once.  rowptr int32 [V+1],
 *   cols int32 [nnz]: row i = the distinct j != i that share a face edge with i, ascending.  pinned uint8 [V] or NULL: vertices that never move
 *   (the caller passes the endpoints of edges that occur once among the faces' undirected edges).
 *   One pass with factor f reads p and writes q (another buffer), per vertex i with n = its row's length and per component:
 *     s = 0;  for j in row order: s = __fadd_rn(s, p_j);  m = __fdiv_rn(s, (float)n);  d = __fsub_rn(m, p_i);
 *     q_i = __fadd_rn(p_i, __fmul_rn(f, d));   n = 0 or pinned: q_i = p_i.
 *   One iteration = a pass with lam, then a pass with mu: 2 * iterations launches between the workspace and out (verts is only read; out must
 *   not be verts), no host synchronise.  iterations = 0 copies verts to out.  eg3d_smooth_query_workspace, host only: one [V][3] buffer.
 *   Errors, before any launch: EG3D_ERR_INVALID (null params, V, nnz or iterations < 0, lam or mu not finite, null verts / out or out == verts
 *   with V > 0, null rowptr, null cols with nnz > 0, short workspace), EG3D_ERR_TOO_LARGE (V or nnz > INT32_MAX).  V = 0: ok, no launch.
 */
typedef struct eg3d_simplify_params {
    const float* verts;                /* [V][3] */
    const int32_t* faces;              /* [F][3] */
    int64_t V, F;
    float cell;
    float origin[3];
    int32_t* flags;                    /* device int32[2] */
    int64_t* keys;                     /* [V]  _keys writes */
    const int64_t* sorted_keys;        /* [V]  _heads reads */
    const int64_t* order;              /* [V]  the sort's permutation: sorted_keys[i] = keys[order[i]] */
    int32_t* heads;                    /* [V] */
    const int32_t* head_scan;          /* [V] */
    int32_t* tri;                      /* [3][F] */
    int32_t* alive;                    /* [F] */
    const int64_t* face_order;         /* [F] */
    int32_t* used;                     /* [V] */
    const int32_t* alive_scan;         /* [F] */
    const int32_t* used_scan;          /* [V] */
    void* workspace;                   /* eg3d_simplify_query_workspace's bytes */
    int64_t workspace_bytes;
    float* out_verts;                  /* [out_vert_capacity][3] */
    int64_t out_vert_capacity;
    int32_t* out_faces;                /* [out_face_capacity][3] */
    int64_t out_face_capacity;
    int32_t* vertex_map;               /* [V] */
} eg3d_simplify_params;
int eg3d_simplify_query_workspace(const eg3d_simplify_params* p, int64_t* workspace_bytes);
int eg3d_simplify_keys(const eg3d_simplify_params* p, void* stream);
int eg3d_simplify_heads(const eg3d_simplify_params* p, void* stream);
int eg3d_simplify_clusters(const eg3d_simplify_params* p, void* stream);
int eg3d_simplify_mark(const eg3d_simplify_params* p, void* stream);
int eg3d_simplify_emit(const eg3d_simplify_params* p, void* stream);

typedef struct eg3d_smooth_params {
    const float* verts;                /* [V][3] */
    float* out;                        /* [V][3] */
    const int32_t* rowptr;             /* [V + 1] */
    const int32_t* cols;               /* [nnz] */
    const uint8_t* pinned;             /* [V] or NULL */
    int64_t V, nnz;
    int32_t iterations;
    float lam, mu;
    void* workspace;                   /* eg3d_smooth_query_workspace's bytes */
    int64_t workspace_bytes;
} eg3d_smooth_params;
int eg3d_smooth_query_workspace(const eg3d_smooth_params* p, int64_t* workspace_bytes);
int eg3d_smooth(const eg3d_smooth_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SSIM / MS-SSIM (reconstruction metrics) -- pytorch_msssim 1.0's ssim / ms_ssim with win=None, as the reference's evaluation calls it
 *   (training/coaches/single_id_coach.py:87-99; csrc/ssim.hip).  x, y: contiguous fp32 [N,C,H,W], any value range.
 *   Gaussian window win[k] = exp(-(k - win_size/2)^2 / (2 sigma^2)) / sum, applied separably (H then W) per channel, valid (no padding).
 *   Per level: cs = (2 s_xy + C2) / (s_xx + s_yy + C2), ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs, averaged per (image, channel).
 *   ms_ssim (mode 1): `levels` levels, between them avg_pool2d(2, 2, padding = side % 2, count_include_pad) of both images; the value per
 *   channel is prod_l relu(m_l)^weights[l], m_l = mean cs for l < levels-1, mean ssim for the last.  ssim (mode 0): levels = 1, the
 *   mean ssim (relu'd when `nonnegative`).  out: [N] means over channels, or [1] the mean over everything with size_average.
 *   No floating-point atomics: partial sums per workgroup, reduced in a fixed order (bit-identical run to run and between the two builds);
 *   no host synchronise.  Every level's sides must be >= win_size (EG3D_ERR_INVALID otherwise).
 *   Protocol:
 *     eg3d_ssim_query_workspace  host only: floats of the pooled-image pyramid, doubles of the per-channel statistics, workspace bytes of
 *                                the forward and of the backward
 *     eg3d_ssim_forward          levels + 1 launches: writes pyramid (levels 1.., x then y), stats ([N*C][levels+1]: the means m_l, then the
 *                                value) and out
 *     eg3d_ssim_backward         2 launches per level, coarsest first: grad_x / grad_y (either may be NULL) = d(sum_n grad_out[n] out[n]) /
 *                                d(x, y), from the forward's pyramid and stats (moments recomputed).  A term at or below 0 (relu) passes no
 *                                gradient, so a clamped level, or a value that is 0, gives zeros, never NaN.
 */
#define EG3D_SSIM_MAX_LEVELS 8
#define EG3D_SSIM_MAX_WIN 15
typedef struct eg3d_ssim_params {
    const float* x;
    const float* y;
    int32_t N, C, H, W;
    int32_t mode;                      /* 0 = ssim, 1 = ms_ssim */
    int32_t levels;                    /* 1 .. EG3D_SSIM_MAX_LEVELS (1 for ssim) */
    int32_t nonnegative;               /* ssim: relu the per-channel value */
    int32_t size_average;              /* out has 1 value instead of N */
    int32_t win_size;                  /* odd, 1 .. EG3D_SSIM_MAX_WIN */
    float win_sigma;
    float C1, C2;                      /* (K1 data_range)^2, (K2 data_range)^2 */
    float weights[EG3D_SSIM_MAX_LEVELS];
    float* pyramid;                    /* eg3d_ssim_query_workspace's pyramid_floats (may be NULL when levels = 1) */
    double* stats;                     /* N*C*(levels+1) */
    float* out;                        /* N, or 1 with size_average */
    void* workspace;
    int64_t workspace_bytes;
    const float* grad_out;             /* backward: N, or 1 with size_average */
    float* grad_x;                     /* backward: [N,C,H,W] or NULL */
    float* grad_y;
} eg3d_ssim_params;
int eg3d_ssim_query_workspace(const eg3d_ssim_params* p, int64_t* pyramid_floats, int64_t* stats_doubles, int64_t* forward_bytes,
                              int64_t* backward_bytes);
int eg3d_ssim_forward(const eg3d_ssim_params* p, void* stream);
int eg3d_ssim_backward(const eg3d_ssim_params* p, void* stream);

/* Face crop + pool of the identity metric (criteria/id_loss.py IDLoss.extract_feats): x[:, :, r0:r1, c0:c1] (bounds already clamped to the
 * image, non-empty) -> AdaptiveAvgPool2d(S): output i averages rows [floor(i*Hc/S), ceil((i+1)*Hc/S)) of the crop.  x: contiguous fp32 [N,3,H,W];
 * out: [N,S,S,4] (the channels-last [N,4,S,S] image of the IR-SE trunk, fourth channel 0).  One launch. */
int eg3d_face_pool(const float* x, int N, int H, int W, int r0, int r1, int c0, int c1, int S, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm on batch statistics (training mode) -- torch.nn.BatchNorm2d.train() on channels-last fp32 [M = N*H*W, C] (csrc/batchnorm.hip; the
 *   pose estimator's training path).  C a multiple of 4, M >= 2; x, y, residual, dy, dx, dresidual 16-byte aligned.
 *   forward:  mean[c], var[c] (biased) over the M rows; y = act(gamma (x - mean) / sqrt(var + eps) + beta [+ residual]), act linear | relu;
 *             running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with the UNBIASED variance var M / (M - 1),
 *             num_batches_tracked += 1 (each of the three may be NULL); stats [2C] doubles = mean, 1 / sqrt(var + eps), which the backward
 *             reads; save_mean / save_invstd (may be NULL) the same as fp32.  Three launches (chunk sums, per-channel finish, apply).
 *   backward: dy' = dy where the saved output y > 0 (relu; y unused and may be NULL when linear); dbeta = sum dy', dgamma = sum dy' xhat,
 *             dx = gamma invstd (dy' - dbeta / M - xhat dgamma / M), dresidual = dy' (dx, dresidual, dgamma, dbeta may each be NULL).
 *             Three launches (chunk sums, finish, apply); x and dy are read twice.
 *   The moments are double-precision sums of differences from a per-channel shift, per workgroup, combined in a fixed order: no atomics,
 *   bit-identical between runs and between the two builds; no host synchronise.
 *   workspace: eg3d_batchnorm_query_workspace bytes, 16-byte aligned, scratch (need not survive from forward to backward; stats must).
 *   Errors: EG3D_ERR_INVALID (null / misaligned pointer, C % 4 != 0, M < 2, short workspace, momentum outside [0,1]), EG3D_ERR_UNSUPPORTED
 *   (another activation), before anything is launched.
 */
typedef struct eg3d_batchnorm_params {
    const float* x;                    /* [M,C] */
    const float* gamma;                /* [C] */
    const float* beta;                 /* [C] (forward) */
    const float* residual;             /* [M,C] or NULL (forward) */
    float* y;                          /* [M,C]: forward output; backward: the saved output (relu) */
    int64_t M;
    int32_t C;
    int32_t act;                       /* EG3D_ACT_LINEAR | EG3D_ACT_RELU */
    float eps, momentum;
    float* running_mean;               /* [C] or NULL, updated in place (forward) */
    float* running_var;
    int64_t* num_batches_tracked;      /* one counter or NULL */
    float* save_mean;                  /* [C] or NULL (forward) */
    float* save_invstd;
    double* stats;                     /* [2C]: written by forward, read by backward */
    void* workspace;
    int64_t workspace_bytes;
    const float* dy;                   /* backward: [M,C] */
    float* dx;                         /* [M,C] or NULL */
    float* dresidual;                  /* [M,C] or NULL */
    float* dgamma;                     /* [C] or NULL */
    float* dbeta;
} eg3d_batchnorm_params;
int eg3d_batchnorm_query_workspace(int64_t M, int32_t C, int64_t* workspace_bytes);
int eg3d_batchnorm_forward(const eg3d_batchnorm_params* p, void* stream);
int eg3d_batchnorm_backward(const eg3d_batchnorm_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GANSpace latent editing (ganspace/pca_anlaysis.py, estimator.py, run_ganspace.py; csrc/pca.hip): a PCA of W on the device and the
 *   uint8 grids of the edits.  Nothing here accumulates with atomics: both builds of the library give the same bits.
 *
 * Second moments of row data x [S,D] fp32 (leading dimension ldx >= D), 1 <= D <= 512, S >= 1, about a caller-chosen shift [D] (W has a mean
 *   that is large against its spread: the host passes the first chunk's column mean, which is what makes fp32 products viable):
 *     eg3d_pca_moments_slabs       host only: slabs = ceil(S / EG3D_PCA_SLAB_ROWS) -- the rows one fp32 sum runs over -- or a negative status
 *     eg3d_pca_moments             one launch: gram_part [slabs][D][D] = per-slab (x-shift)^T (x-shift), the elements i <= j ONLY (the rest is
 *                                  not written), sum_part [slabs][D] = per-slab column sums of (x-shift).  Exact fp32 products and sums
 *                                  (v_mfma_f32_32x32x2_f32).
 *     eg3d_pca_moments_accumulate  gram [D][D] (full, symmetric) and sum [D], fp64, += the slabs in slab order.  The caller zeroes them before
 *                                  the first chunk; they persist across chunks.
 *     eg3d_pca_covariance          cov [D][D] fp32 = gram / S_total - d d^T with d = sum / S_total (ddof 0, computed in fp64 from the upper
 *                                  triangle and mirrored: exactly symmetric), mean [D] = shift + d. */
#define EG3D_PCA_SLAB_ROWS 256
int eg3d_pca_moments_slabs(int64_t S, int D);
int eg3d_pca_moments(const float* x, int64_t S, int D, int64_t ldx, const float* shift, float* gram_part, float* sum_part, void* stream);
int eg3d_pca_moments_accumulate(const float* gram_part, const float* sum_part, int slabs, int D, double* gram, double* sum, void* stream);
int eg3d_pca_covariance(const double* gram, const double* sum, int64_t S_total, int D, const float* shift, float* cov, float* mean, void* stream);

/* Eigen-decomposition of a symmetric fp32 matrix a [n][n], 1 <= n <= 512: one-sided (Hestenes) Jacobi, round-robin ordering; the n/2 disjoint
 *   rotations of a round are one launch (one wave per pair), so a sweep is n - 1 (n even) or n (n odd, one bye per round) launches plus two.
 *   A pair is rotated when |a_p.a_q| > tol |a_p||a_q| (tol <= 0: 8 * 2^-23) and left alone when its smaller squared norm is below
 *   (n 2^-24)^2 times the largest of the sweep (columns of the numerical null space).  After every sweep the largest criterion seen is read
 *   back: the function SYNCHRONISES the stream once per sweep and cannot be captured into a graph.  It stops after the first sweep that
 *   rotated nothing (converged) or after max_sweeps (>= 1) sweeps, whichever comes first, and reports which in info (HOST memory):
 *   info[0] = sweeps run, info[1] = 1 converged / 0 not.  Either way the outputs are written: evals [n] descending (Rayleigh quotients), evecs
 *   [n][n] with eigenvector i as ROW i, unit length, signed so that its largest-magnitude entry (the first of equals) is positive -- what
 *   sklearn's svd_flip gives the reference's estimator.  Only the symmetric part's upper/lower agreement is assumed, not checked.
 *   workspace: eg3d_sym_eig_workspace bytes of device memory, 16-byte aligned.  Bit-identical from run to run and between the builds. */
int eg3d_sym_eig_workspace(int n, int64_t* bytes);
int eg3d_sym_eig(const float* a, int n, float* evals, float* evecs, int max_sweeps, float tol, void* workspace, int32_t* info, void* stream);

/* img [N,3,H,W] fp32 -> out uint8 [Ht][Wt][3], every value uint8(clamp(x * 127.5 + 128, 0, 255)) (truncated; the reference's
 *   (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)), tiled as torchvision.utils.make_grid(nrow, padding, pad_value) tiles: xmaps = min(nrow, N),
 *   ymaps = ceil(N / xmaps), Ht = ymaps (H + padding) + padding, Wt = xmaps (W + padding) + padding, image k at cell (k / xmaps, k % xmaps)
 *   offset by padding; borders and unused cells = pad_value (0..255).  padding = 0: the plain tiling of gen_videos.layout_grid.  NaN undefined. */
int eg3d_image_grid_u8(const float* img, int N, int H, int W, int nrow, int padding, int pad_value, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG encoder (media export: the frames of gen_interp_video's orbit, gen_videos.py:74-146; csrc/jpeg.hip).
 *   img: contiguous [N,C,H,W], C = 3 (RGB) or 1 (grey), H, W >= 1; dtype EG3D_JPEG_F32 = fp32 in [-1,1], quantised as eg3d_image_grid_u8
 *   (uint8(clamp(x * 127.5 + 128, 0, 255)), truncated), or EG3D_JPEG_U8 taken as is.  Output: N complete JFIF files back to back.
 *   Integer arithmetic throughout (a host restatement equals it bit for bit):
 *     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 *     Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16; grey: Y = the channel;
 *     the full-resolution planes are extended by replicating the last row / column to a multiple of the MCU (8; 16 with 4:2:0);
 *     4:2:0 chroma = (a + b + c + d + 2) >> 2 per 2 x 2 block;  s = p - 128;  T = (CI S + 1024) >> 11;  D = (T CI^T + 16384) >> 15 (arithmetic
 *     shifts, CI = jpeg_ci of csrc/jpeg_tables.h);  q = sign(D) ((|D| + (Q >> 1)) / Q), Q = the Annex K table scaled by `quality` as libjpeg's
 *     jpeg_quality_scaling (clamped to 1..255);  Annex K Huffman tables;  one interleaved scan, 4:2:0 MCU = Y00 Y01 Y10 Y11 Cb Cr.
 *   Restart interval R MCUs (0 = MCUs per row capped at EG3D_JPEG_MAX_RESTART; at most EG3D_JPEG_MAX_RESTART): every interval is coded on
 *   its own (DC prediction restarts, the last byte is filled with 1-bits, 0xFF is followed by 0x00) and followed by RSTm, m = interval index
 *   mod 8, the last one by EOI.  `header` (device, header_bytes): everything of the file up to and including SOS, identical for the N frames;
 *   the caller builds it for the same H, W, C, subsampling, quality and R (inv3d_amd/video.py jpeg_header).
 *   No atomics on global memory and no floating-point sums: bit-identical between runs and between the two builds.
 *   Protocol:
 *     eg3d_jpeg_query_workspace  host only: workspace bytes (coefficients + one worst-case slot per interval: a block is at most
 *                                22 + 63 * 26 bits, doubled by byte stuffing, + the marker)
 *     eg3d_jpeg_encode           three launches: fills the workspace and writes offsets[0..N] (device int64: frame n is out[offsets[n] ..
 *                                offsets[n+1]), offsets[N] = the total)
 *     (host reads offsets[N]: one synchronise; allocates out)
 *     eg3d_jpeg_pack             one launch: headers and interval slots into out, never beyond out_capacity
 */
#define EG3D_JPEG_F32 0
#define EG3D_JPEG_U8 1
#define EG3D_JPEG_444 0
#define EG3D_JPEG_420 1
#define EG3D_JPEG_MAX_RESTART 32
typedef struct eg3d_jpeg_params {
    const void* img;                   /* [N,C,H,W] */
    const uint8_t* header;             /* device, header_bytes */
    void* workspace;                   /* eg3d_jpeg_query_workspace's bytes, 16-byte aligned */
    int64_t workspace_bytes;
    int64_t* offsets;                  /* device int64[N+1] */
    uint8_t* out;                      /* pack: out_capacity bytes */
    int64_t out_capacity;
    int32_t dtype;                     /* EG3D_JPEG_F32 | EG3D_JPEG_U8 */
    int32_t N, C, H, W;
    int32_t subsampling;               /* EG3D_JPEG_444 | EG3D_JPEG_420 (ignored for C = 1) */
    int32_t quality;                   /* 1..100 */
    int32_t restart_interval;          /* MCUs; 0 = default */
    int32_t header_bytes;
} eg3d_jpeg_params;
int eg3d_jpeg_query_workspace(const eg3d_jpeg_params* p, int64_t* workspace_bytes);
int eg3d_jpeg_encode(const eg3d_jpeg_params* p, void* stream);
int eg3d_jpeg_pack(const eg3d_jpeg_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG decoder (target-image ingestion: PIL.Image.open(path).convert('RGB') of utils/ImagesDataset.py and utils/align_data.py for
 * the files photographs arrive as; csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h).  One image per call (N per call: the block after this one).  The output bytes are those of
 * libjpeg(-turbo)'s default decode; tests/support/jpegdec_ref.py restates it.  Integers only, no floating point anywhere; the only atomics
 * are ORs into the status word: the output is a function of the input bytes, bit-identical between runs and between the two builds.
 *   Taken: 8-bit baseline (SOF0) Huffman-coded files with one interleaved scan of three components -- luma sampled hsamp x vsamp = 1 x 1
 *   (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0) beside 1 x 1 chroma -- or of one component; any Huffman tables; any restart interval.  The caller
 *   parses the markers (inv3d_amd/video.py jpeg_scan_plan) and passes
 *     data    device, data_bytes: the entropy-coded segment between SOS and EOI as it stands in the file (stuffing and RSTm included),
 *             16-byte aligned and readable up to the next multiple of 16
 *     tables  device, EG3D_JPEGDEC_TABLE_BYTES: the quantisation tables Tq = 0..3 as uint8 [4][64] in natural (row-major) order, then the
 *             Huffman tables DC 0, DC 1, AC 0, AC 1 as BITS[16] HUFFVAL[256] (zero-filled) each
 *   Stages:
 *   1. Marker pass.  Every FF xx of `data`: FF 00 is a stuffed FF, FF D0..D7 a restart marker, anything else (a trailing FF too) sets
 *      EG3D_JPEGDEC_ERR_MARKER.  A scan and compaction give the unstuffed stream and the start of every restart segment in it.  A number of
 *      restart markers other than the geometry's, or RSTm out of sequence: EG3D_JPEGDEC_ERR_SEGMENTS.
 *   2. Self-synchronising Huffman decode.  Every restart segment is cut into subsequences of subseq_bytes (a power of two, 16..1024); one lane
 *      owns one.  A lane's state is (bit position, block of the MCU, zigzag index).  A lane decodes symbols from its entry state until the bit
 *      position reaches its subsequence's end, or the next symbol does not fit the segment, and records the state it leaves in.  The first lane
 *      of a segment enters in the known state; every other lane first guesses (its first bit, block 0, index 0).  Then, in rounds, every lane
 *      re-decodes from its left neighbour's recorded exit state whenever that changed, inside a workgroup of 256 lanes through LDS, then across
 *      the workgroup borders, until a round changes nothing -- the fixed point, at which every recorded state is the true one.  The number of
 *      subsequences bounds the rounds.
 *   3. Coefficients.  Every lane counted the blocks it starts and summed the DC differences per component; an exclusive scan gives its first
 *      block and its DC predictions (both relative to the segment's first lane: prediction restarts with the segment).  A last decode writes
 *      the values into a zeroed int16 [blocks][64] in natural order, every store guarded by the segment's block range and index < 64; bits
 *      beyond a segment's end read as zero.  A segment whose block total differs from the geometry's, or that ends inside a block:
 *      EG3D_JPEGDEC_ERR_BLOCKS;  bits no code of the table matches, or a run past index 63: EG3D_JPEGDEC_ERR_CODE.
 *   4. Dequantisation and jidctint.c's jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, columns descaled by 11, rows by 18 (32-bit wrap-around
 *      arithmetic), & 1023, libjpeg's range-limit table (the 10-bit value as signed, + 128, clamped) -> one uint8 plane per component, padded
 *      to whole MCUs.
 *   5. jdsample.c's fancy upsampling where the chroma has more than two real columns (h2v1: (3 a + left + 1) >> 2, (3 a + right + 2) >> 2;
 *      h2v2: s = 3 near row + far row, (3 s + s_left + 8) >> 4, (3 s + s_right + 7) >> 4; neighbours clamped to the real down-sampled size
 *      ceil(W / hsamp) x ceil(H / vsamp)), replication otherwise; jdcolor.c's YCbCr -> RGB: R = Y + ((91881 Cr' + 32768) >> 16),
 *      G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), Cb' = Cb - 128, clamped.  Grey is replicated.
 *   out: uint8 [H][W][3].  result: int32 [EG3D_JPEGDEC_RESULT_WORDS] on the device, written by the call: [0] status (0, or an OR of
 *   EG3D_JPEGDEC_ERR_*; `out` means nothing then), [1] rounds of stage 2 inside the workgroups that changed a state (the maximum over the
 *   workgroups), [2] rounds across the borders, [3] lanes, [4] unstuffed bytes, [5] restart markers.  The caller reads it once.
 *   Errors before any launch: EG3D_ERR_INVALID (NULL or misaligned pointers, sizes outside 1..65535, ncomp not 1 or 3, table selectors out of
 *   range, subseq_bytes, a short workspace), EG3D_ERR_UNSUPPORTED (other sampling factors), EG3D_ERR_TOO_LARGE (data_bytes >= 2^28, or
 *   more than 2^24 lanes).
 *     eg3d_jpegdec_query_workspace  host only: workspace bytes (unstuffed stream, per-lane records, coefficients, planes)
 *     eg3d_jpegdec_decode           twelve launches, no host synchronise
 */
#define EG3D_JPEGDEC_TABLE_BYTES (256 + 4 * 272)
#define EG3D_JPEGDEC_RESULT_WORDS 8
#define EG3D_JPEGDEC_ERR_MARKER 1
#define EG3D_JPEGDEC_ERR_SEGMENTS 2
#define EG3D_JPEGDEC_ERR_BLOCKS 4
#define EG3D_JPEGDEC_ERR_CODE 8
#define EG3D_JPEGDEC_STAGE_MARKERS 1  /* result zeroed; marker count, scan, apply */
#define EG3D_JPEGDEC_STAGE_SYNC 2     /* segments, synchronisation inside and across the workgroups, prefix scan and checks */
#define EG3D_JPEGDEC_STAGE_WRITE 4    /* coefficients zeroed and written */
#define EG3D_JPEGDEC_STAGE_IDCT 8
#define EG3D_JPEGDEC_STAGE_COLOUR 16
typedef struct eg3d_jpegdec_params {
    const uint8_t* data;               /* device: the entropy-coded segment */
    int64_t data_bytes;
    const uint8_t* tables;             /* device, EG3D_JPEGDEC_TABLE_BYTES */
    void* workspace;                   /* eg3d_jpegdec_query_workspace's bytes, 16-byte aligned */
    int64_t workspace_bytes;
    uint8_t* out;                      /* device uint8 [H][W][3] */
    int32_t* result;                   /* device int32 [EG3D_JPEGDEC_RESULT_WORDS] */
    int32_t H, W;
    int32_t ncomp;                     /* 1 | 3 */
    int32_t hsamp, vsamp;              /* luma sampling factors (ignored for ncomp = 1) */
    int32_t tq[3], td[3], ta[3];       /* per component: quantisation table 0..3, DC and AC Huffman table 0..1 */
    int32_t restart_interval;          /* MCUs; 0 = none */
    int32_t subseq_bytes;              /* 16..1024, a power of two */
    int32_t stages;                    /* 0 = everything; else an OR of EG3D_JPEGDEC_STAGE_* to run alone on a workspace a full call filled (timing) */
} eg3d_jpegdec_params;
int eg3d_jpegdec_query_workspace(const eg3d_jpegdec_params* p, int64_t* workspace_bytes);
int eg3d_jpegdec_decode(const eg3d_jpegdec_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG decoder, N images per call (a directory of photographs, the frames of a Motion-JPEG file; csrc/jpeg_decode.hip).  The
 * stages, the arithmetic, the status bits and the result words are those of the one-image call above, per image; what changes is that every
 * pass is launched once for the whole batch, so the number of launches does not depend on N and the serial rounds of stage 2 -- latency,
 * not throughput, at the sizes of video frames -- run side by side for all images.
 *   The images are heterogeneous: each has its own H, W, component count, sampling, restart interval, table selectors, tables and
 *   entropy-coded bytes.  subseq_bytes and stages are per call.
 *   Grid: the image is blockIdx.y (blockIdx.z in the colour pass), gridDim.x the largest image's count of workgroups for that pass; a
 *   workgroup past its own image's count leaves at once.  The three one-workgroup kernels (marker scan, segments, stitch) run one
 *   workgroup per image.  No prefix table is walked: a workgroup reads its image's record -- geometry and addresses -- from device memory
 *   by its grid index.  A very large image beside many small ones therefore costs N times the large image's empty workgroups.
 *   One upload: the caller lays out one host buffer as [plan | tables and entropy-coded bytes at offsets of its choice], has
 *   eg3d_jpegdec_batch_plan fill the plan (host only: it needs the device addresses of the upload buffer, the workspace, the result and
 *   every `out`, so those are allocated first) and copies the buffer to `upload` once.
 *     images  host, [n]: per image the geometry as in eg3d_jpegdec_params; data_offset (a multiple of 16; the bytes are readable up to the
 *             next multiple of 16) and tables_offset (EG3D_JPEGDEC_TABLE_BYTES) from `upload`, both at or beyond plan_bytes and inside
 *             upload_bytes; out: device uint8 [H][W][3], any address
 *     result  device int32 [n][EG3D_JPEGDEC_RESULT_WORDS].  A non-zero status of one image touches no other image's pixels or result.
 *     workspace  range after range (sums, offsets, unstuffed stream, ..., coefficients, planes), each range image after image: what a call
 *             zeroes is two stretches whatever n is.  Batch totals are 64-bit; per image the limits of the one-image call hold.
 *   Every entropy-pass store is guarded by that image's geometry, reads beyond a segment's end yield zero bits, integers only, the only
 *   atomics are ORs into an image's own status word: pixels are a function of the bytes, identical between runs and between the builds.
 *   Errors before any launch: EG3D_ERR_INVALID (n < 1, NULL or misaligned pointers, an offset outside the upload, a short workspace, or
 *   what the one-image call rejects, for any image), EG3D_ERR_UNSUPPORTED (sampling factors), EG3D_ERR_TOO_LARGE (n > 65535: the image is a
 *   grid dimension; or an image beyond the one-image limits).
 *     eg3d_jpegdec_batch_query_workspace  host only: workspace bytes, and the bytes of the plan at the start of `upload`
 *     eg3d_jpegdec_batch_plan             host only: fills `plan` (plan_bytes, 8-byte aligned)
 *     eg3d_jpegdec_batch_decode           the launches of the one-image call (twelve), no host synchronise; `upload` holds the copied plan
 */
typedef struct eg3d_jpegdec_image {
    int64_t data_offset;               /* from `upload`: the entropy-coded segment, 16-byte aligned */
    int64_t data_bytes;
    int64_t tables_offset;             /* from `upload`: EG3D_JPEGDEC_TABLE_BYTES */
    uint8_t* out;                      /* device uint8 [H][W][3] */
    int32_t H, W;
    int32_t ncomp;                     /* 1 | 3 */
    int32_t hsamp, vsamp;
    int32_t tq[3], td[3], ta[3];
    int32_t restart_interval;          /* MCUs; 0 = none */
    int32_t reserved;
} eg3d_jpegdec_image;
typedef struct eg3d_jpegdec_batch_params {
    const eg3d_jpegdec_image* images;  /* host, [n] */
    void* plan;                        /* host, plan_bytes: written by eg3d_jpegdec_batch_plan, copied by the caller to upload[0 .. plan_bytes) */
    const uint8_t* upload;             /* device, upload_bytes, 16-byte aligned: plan, tables, entropy-coded bytes */
    int64_t upload_bytes;
    void* workspace;                   /* eg3d_jpegdec_batch_query_workspace's bytes, 16-byte aligned */
    int64_t workspace_bytes;
    int32_t* result;                   /* device int32 [n][EG3D_JPEGDEC_RESULT_WORDS] */
    int32_t n;                         /* 1..65535 */
    int32_t subseq_bytes;              /* 16..1024, a power of two */
    int32_t stages;                    /* as eg3d_jpegdec_params.stages */
    int32_t reserved;
} eg3d_jpegdec_batch_params;
int eg3d_jpegdec_batch_query_workspace(const eg3d_jpegdec_batch_params* p, int64_t* workspace_bytes, int64_t* plan_bytes);
int eg3d_jpegdec_batch_plan(const eg3d_jpegdec_batch_params* p);
int eg3d_jpegdec_batch_decode(const eg3d_jpegdec_batch_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG encoder (media export: every lossless image the package writes -- grids, aligned targets, paste-back outputs, mesh previews, the OBJ
 * exporter's atlas; csrc/png.hip).  Adaptive row filters, then a deflate that only matches runs at distance 1 (what zlib's Z_RLE finds).
 *   img: contiguous uint8 [N][H][W][C], C = 1 (grey) or 3 (RGB), N >= 1, 1 <= H, W <= 16384.  Output: N complete zlib streams back to back
 *   (what a PNG's IDAT holds; the container -- signature, IHDR, IDAT, IEND and their CRCs -- is host code, inv3d_amd/video.py png_container).
 *   Integers only, no atomics on global memory: bit-identical between runs and between the two builds; tests/support/png_ref.py restates it.
 *   1. Row filters (PNG 1.2 section 6, bpp = C).  With x the raw byte, a the byte bpp to its left, b the byte above, c the byte above a (row -1
 *      and the bytes left of column 0 are zero), the filtered byte is (x - q) & 255 with q = 0 (type 0 None), a (1 Sub), b (2 Up),
 *      (a + b) >> 1 (3 Average), Paeth(a, b, c) (4: p = a + b - c; a if |p - a| <= |p - b| and |p - a| <= |p - c|, else b if |p - b| <= |p - c|,
 *      else c).  filter = 0..4 forces the type; filter = -1 picks per row the type with the smallest sum over the row's W * C bytes of
 *      |int8(byte)| (v < 128 ? v : 256 - v), a tie going to the lower type (libpng's heuristic).  The image's filtered stream is H records
 *      [type][W * C bytes], L = H (1 + W C) bytes.
 *   2. Blocks and tokens.  The stream is cut into blocks of block_bytes (64..65536; the last one may be short).  Inside a block, for every
 *      maximal run of r equal bytes v (runs end at the block's end): literal v; with m = r - 1, m / 258 matches of length 258 at distance 1;
 *      with q = m % 258 one more match of length q if q >= 3, else q literals v.  Then end-of-block.
 *   3. Codes.  Every block is a dynamic-Huffman block (BTYPE = 2).  Literal/length code over symbols 0 .. the highest used (256 always is);
 *      exactly one distance code (HDIST = 0) of length 1 when the block has a match, 0 when it has none.  Code lengths of an alphabet:
 *      the used symbols sorted by (count, symbol) ascending; a two-queue Huffman merge (leaves in that order, merged nodes in the order they
 *      are made; of two equal weights the leaf is taken first); the number of codes per depth, depths above the limit counted at the limit;
 *      miniz's tdefl_huffman_enforce_max_code_size (while the Kraft sum exceeds 1: one code fewer at the limit, the deepest shorter depth i
 *      that has a code gives it up for two at i + 1); lengths handed out in increasing length from the most frequent end of the sorted order.
 *      The limit is 15, and 7 for the code-length alphabet; where the unrestricted tree fits the limit the code is optimal.  Codes are
 *      canonical (RFC 1951 3.2.2).  The code-length sequence is the HLIT + 257 literal/length lengths and the distance length, one symbol
 *      0..15 each: the repeat codes 16, 17, 18 are not used (at most ~150 bytes per block), all 19 code-length code lengths are sent (HCLEN = 15).
 *   4. Stream.  78 01; the blocks; after every block but the last an empty stored block (bits 0, 00, zero bits to the byte, 00 00 FF FF) so
 *      that every block starts on a byte; the last block has BFINAL = 1 and is padded with zero bits; Adler-32 of the filtered stream, big
 *      endian, combined on the device from per-block sums (sa = sum d_i, sb = sum (n - i) d_i mod 65521; two strings in a row:
 *      sa1 + sa2, sb1 + n2 sa1 + sb2; in the end a = 1 + sa, b = n + sb).
 *   Protocol (as eg3d_jpeg_*):
 *     eg3d_png_query_workspace  host only: workspace bytes = N (align16(L) + 16) for the filtered streams + one slot per block + per-block
 *                               lengths, destinations and Adler sums.  A slot holds the worst case of a block of block_bytes bytes:
 *                               header 17 + 19 * 3 + 287 * 7 bits; a literal is at most 15 bits for one byte and a match at most
 *                               15 + 5 + 1 bits for at least 3, so at most 15 bits per byte; end-of-block at most 15 bits; 3 bits of the
 *                               stored block, up to 7 bits of padding and its 4 bytes; + 8 bytes (the slot is written and read in dwords)
 *     eg3d_png_encode           four launches: fills the workspace and writes offsets[0..N] (device int64: stream n is out[offsets[n] ..
 *                               offsets[n+1]), offsets[N] = the total)
 *     (host reads offsets[N]: one synchronise; allocates out; passes the total back as total_bytes)
 *     eg3d_png_pack             one launch: the streams into out.  out_capacity < total_bytes is EG3D_ERR_INVALID and nothing is launched;
 *                               the kernel writes nothing at or beyond out_capacity whatever total_bytes says
 *   Errors, before any launch: EG3D_ERR_INVALID for a NULL pointer, C not 1 or 3, N, H or W < 1, filter outside -1..4, block_bytes outside
 *   64..65536, a short or misaligned workspace;  EG3D_ERR_UNSUPPORTED for H or W > 16384;  EG3D_ERR_TOO_LARGE when N H or the number of blocks
 *   leaves int32.
 */
#define EG3D_PNG_FILTER_ADAPTIVE (-1)
typedef struct eg3d_png_params {
    const uint8_t* img;                /* [N,H,W,C] */
    void* workspace;                   /* eg3d_png_query_workspace's bytes, 16-byte aligned */
    int64_t workspace_bytes;
    int64_t* offsets;                  /* device int64[N+1] */
    uint8_t* out;                      /* pack: out_capacity bytes */
    int64_t out_capacity;
    int64_t total_bytes;               /* pack: offsets[N] as the host read it */
    int32_t N, C, H, W;
    int32_t filter;                    /* -1 adaptive, 0..4 forced */
    int32_t block_bytes;               /* 64..65536 */
    int32_t stages;                    /* encode: 0 = everything; 1 = the filter pass alone, 2 = the rest on an already filtered workspace (timing) */
} eg3d_png_params;
int eg3d_png_query_workspace(const eg3d_png_params* p, int64_t* workspace_bytes);
int eg3d_png_encode(const eg3d_png_params* p, void* stream);
int eg3d_png_pack(const eg3d_png_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image ingestion (the pixel work of utils/alignment.py::align_face and of ToTensor / Normalize, scripts/run_pti.py:28-30; csrc/imgprep.hip).
 *   Images are contiguous uint8 [N,H,W,C], C = 1 or 3, sides 1..65535, on the device.  No atomics on floats, no floating-point sum whose order
 *   depends on the launch: bit-identical between runs, batch sizes and the two builds.
 *
 * eg3d_resample8: PIL.Image.resize of an 8-bit image, byte for byte (Pillow's Resample.c, 8bpc path).  The caller builds the integer tables on
 *   the host in float64 (inv3d_amd/hipops.py pil_resize_coeffs: filter support scaled by max(in / out, 1), ksize = 2 ceil(support) + 1, weights
 *   normalised by their left-to-right sum and quantised to 22 fractional bits) and passes them on the device:
 *     hbounds [Wo][2] = (xmin, count) per output column, hcoef [hksize][Wo] (tap-major), hseg = the longest input span
 *     max(xmin + count) - min(xmin) over any tile of EG3D_RESAMPLE_TILE consecutive output columns (tiles start at multiples of it);
 *     vbounds [Ho][2], vcoef [Ho][vksize] (row-major).  A pass runs only when its tables are given: h* must be NULL exactly when Wo == Wi,
 *     v* exactly when Ho == Hi (neither: a copy).
 *   Horizontal pass first (a workgroup stages the row segments it needs in LDS), uint8 intermediate [N,Hi,Wo,C] in the workspace when both
 *   passes run, then the vertical pass (lanes along the row's bytes).  Per sample acc = 2^21 + sum pixel * k in int32, clip(acc >> 22, 0, 255).
 *   A table whose span does not fit hseg yields 0 for that output, never an out-of-range read; hseg * C beyond the LDS budget (48 KB per row)
 *   is EG3D_ERR_UNSUPPORTED.  eg3d_resample8_query_workspace is host only. */
#define EG3D_RESAMPLE_TILE 64
typedef struct eg3d_resample8_params {
    const uint8_t* src;                /* [N,Hi,Wi,C] */
    uint8_t* dst;                      /* [N,Ho,Wo,C] */
    const int32_t* hbounds;            /* device; NULL when Wo == Wi */
    const int32_t* hcoef;
    const int32_t* vbounds;            /* device; NULL when Ho == Hi */
    const int32_t* vcoef;
    void* workspace;                   /* eg3d_resample8_query_workspace's bytes (may be 0: then unused) */
    int64_t workspace_bytes;
    int32_t N, Hi, Wi, C, Ho, Wo;
    int32_t hksize, vksize;
    int32_t hseg;
} eg3d_resample8_params;
int eg3d_resample8_query_workspace(const eg3d_resample8_params* p, int64_t* workspace_bytes);
int eg3d_resample8(const eg3d_resample8_params* p, void* stream);

/* eg3d_quad_warp8: PIL.Image.transform((Wo, Ho), QUAD, data, BILINEAR) with fill 0, byte for byte (Pillow's Geometry.c).  a[0..7] are the
 *   coefficients Pillow derives from the quad (hipops.pil_quad_coeffs); for output (x, y), xi = x + 0.5, yi = y + 0.5:
 *     xin = a0 + a1 xi + a2 yi + a3 xi yi,  yin = a4 + a5 xi + a6 yi + a7 xi yi;  xin < 0 | xin >= Wi | yin < 0 | yin >= Hi: the pixel is 0;
 *     else xin -= 0.5, yin -= 0.5, fx = floor(xin), dx = xin - fx (likewise y), neighbours index-clamped,
 *     r0 = p00 + (p01 - p00) dx, r1 = p10 + (p11 - p10) dx, v = r0 + (r1 - r0) dy, stored as (uint8)v (truncated).
 *   fp64, exactly this operation order, no contraction into FMA.  The same quad for the N images.  One launch. */
typedef struct eg3d_quad_warp8_params {
    const uint8_t* src;                /* [N,Hi,Wi,C] */
    uint8_t* dst;                      /* [N,Ho,Wo,C] */
    double a[8];
    int32_t N, Hi, Wi, C, Ho, Wo;
} eg3d_quad_warp8_params;
int eg3d_quad_warp8(const eg3d_quad_warp8_params* p, void* stream);

/* eg3d_feather_pad: the pad branch of align_face (alignment.py:95-105) in fp32.  With Hp = H + top + bottom, Wp = W + left + right (pads >= 1):
 *     P = float(np.pad(src, 'reflect'))                                    (no edge repeat; any pad width)
 *     B = separable Gaussian of P along y, then x: weights gauss[0..radius] (device fp32, one half of the symmetric normalised kernel, built
 *         on the host in float64), boundary scipy 'reflect' (numpy 'symmetric'), fp32 intermediate; every sum is
 *         g[0] p[0] + g[1] (p[-1] + p[+1]) + ... + g[radius] (p[-radius] + p[+radius]) in this order -- a function of the pixel alone
 *     mask = max(1 - min(x / left, (Wp-1-x) / right), 1 - min(y / top, (Hp-1-y) / bottom))
 *     V = P + (B - P) clip(3 mask + 1, 0, 1)
 *     m[n][c] = median of V[n,:,:,c]: exact, by a radix select over the ordered float bits (integer histograms); an even count takes
 *         (a + b) / 2 of the two middle values in fp32, as np.median
 *     dst = uint8(clip(rint(V + (m - V) clip(mask, 0, 1)), 0, 255)), ties to even
 *   Where both blend weights are 0 the result is src's own byte.  Workspace: two fp32 images [N,Hp,Wp,C] + the select's state; Hp Wp < 2^31.
 *   eg3d_feather_pad_query_workspace is host only. */
typedef struct eg3d_feather_pad_params {
    const uint8_t* src;                /* [N,H,W,C] */
    uint8_t* dst;                      /* [N,Hp,Wp,C] */
    const float* gauss;                /* device [radius + 1] */
    void* workspace;                   /* eg3d_feather_pad_query_workspace's bytes, 16-byte aligned */
    int64_t workspace_bytes;
    int32_t N, H, W, C;
    int32_t left, top, right, bottom;
    int32_t radius;
} eg3d_feather_pad_params;
int eg3d_feather_pad_query_workspace(const eg3d_feather_pad_params* p, int64_t* workspace_bytes);
int eg3d_feather_pad(const eg3d_feather_pad_params* p, void* stream);

/* img uint8 [N,H,W,3] -> out fp32 [N,3,H,W] = (float(v) / 255 - 0.5) / 0.5: torchvision's ToTensor + Normalize(0.5, 0.5), each step one
 *   correctly rounded fp32 operation (a true division by 255, not a multiplication by its reciprocal). */
int eg3d_u8_to_target(const uint8_t* img, int N, int H, int W, float* out, void* stream);

/* eg3d_paste_back8: the inverse of the ingestion -- N edited S x S images (the aligned frame) blended into one photograph, which all frames
 *   share.  m[0..5] is the affine map photo -> aligned frame in Pillow's continuous coordinates (pixel centres at + 0.5; inv3d_amd/images.py
 *   paste_plan builds it from align_plan).  For every photo pixel (X, Y) of the region x0 <= X < x1, y0 <= Y < y1 and every frame, in fp64,
 *   every operation rounded on its own, in this order (no FMA contraction, no division on the device):
 *     Xc = X + 0.5, Yc = Y + 0.5;  u = m0 + m1 Xc + m2 Yc,  v = m3 + m4 Xc + m5 Yc
 *     !(u >= 0 && u < S && v >= 0 && v < S) (NaN too): out = photo
 *     val  = bilinear(edit, u - 0.5, v - 0.5): eg3d_quad_warp8's taps, edge clamp and r0 / r1 / v order, not truncated
 *     d = min(min(u, S - u), min(v, S - v));  f = inv_feather > 0 ? min(d inv_feather, 1) : 1;  a = (f f) (3 - 2 f)
 *     mask given: a = a (bilinear(mask, same taps) (1 / 255))         (1 / 255 a host double)
 *     out = uint8(rint(photo + (val - photo) a)), ties to even
 *   whole = 0: dst holds the region only, [N, y1 - y0, x1 - x0, C] (layout EG3D_PASTE_HWC) or [N, C, y1 - y0, x1 - x0] (EG3D_PASTE_CHW, what
 *   eg3d_jpeg_encode takes).  whole = 1: dst holds the whole photograph per frame, [N,Hp,Wp,C] or [N,C,Hp,Wp]: one launch copies the photo
 *   into every frame, a second one writes the region.  An empty region is valid: nothing is launched for whole = 0, only the copy for whole = 1.
 *   The region must lie inside the photo; sides 1..65535.  No atomics, no sum across threads: both builds give the same bytes. */
#define EG3D_PASTE_HWC 0
#define EG3D_PASTE_CHW 1
typedef struct eg3d_paste_back8_params {
    const uint8_t* photo;              /* [Hp,Wp,C] */
    const uint8_t* edits;              /* [N,S,S,C] */
    const uint8_t* mask;               /* NULL, [S,S] (mask_frames = 1) or [N,S,S] (mask_frames = N) */
    uint8_t* dst;
    double m[6];
    double inv_feather;                /* 1 / feather width in aligned pixels; 0: a hard edge */
    int32_t N, Hp, Wp, C, S;
    int32_t x0, y0, x1, y1;
    int32_t mask_frames;               /* 1 or N; ignored without a mask */
    int32_t whole;
    int32_t layout;
} eg3d_paste_back8_params;
int eg3d_paste_back8(const eg3d_paste_back8_params* p, void* stream);

/* eg3d_paste_blend8 (csrc/blend.hip): eg3d_paste_back8 with a multi-band blend (Burt-Adelson) in place of the one alpha -- the difference
 *   edit - photo is split into L = bands Laplacian levels and every level is weighted by the blend weight reduced to that level, so the
 *   coarse part of the difference (exposure, colour) fades over a wide transition and the detail over a narrow one.  tests/support/blend_ref.py
 *   restates it in numpy; the kernels give its bytes.
 *   The window = the box x0..y1 (the aligned square's bounding box, as for eg3d_paste_back8) grown by M = 2^(L + 2) pixels on every side
 *   and clamped to the photo.  With D and alpha supported in the box, R_0 below is exactly 0 further than 4 2^L - 4 pixels outside it, so
 *   the window truncates nothing unless the photo's border clamps it (there the pyramid sees zeros beyond the border).
 *   Level 0, per frame and window pixel: u, v, val_c and a exactly as eg3d_paste_back8's steps above give them (fp64, the same taps and
 *     order; a = feather x mask).  !(u >= 0 && u < S && v >= 0 && v < S): D_c = 0, alpha = 0; else D_c = (float)(val_c - photo_c),
 *     alpha = (float)a.  From here on fp32, every operation rounded on its own in the order written; fp32 subnormals are KEPT (the tails
 *     of alpha reach them: a small feather value times 16^-2L), as numpy keeps them.
 *   Reduce, level k -> k + 1, applied to every D_c and to alpha: size ceil(n / 2) per axis, taps outside the array read 0, rows first, then
 *     columns; 1-D  r[i] = (((x[2i-2] + x[2i+2]) + 4 (x[2i-1] + x[2i+1])) + 6 x[2i]) (1/16).
 *   Expand E to an h x w level: taps outside read 0, rows first, then columns; 1-D  even i = 2j: ((x[j-1] + x[j+1]) + 6 x[j]) (1/8),
 *     odd i = 2j + 1: (x[j] + x[j+1]) 0.5.
 *   Collapse: R_L = D_L alpha_L;  for k = L - 1 .. 0:  R_k = (D_k - E(D_k+1)) alpha_k + E(R_k+1).
 *   out = uint8(min(max(rintf((float)photo_c + R_0), 0), 255)), ties to even.
 *   alpha == 0 everywhere gives R == 0 exactly (the photo); alpha == 1 returns D only in the interior (zero extension makes alpha_k < 1
 *   near the window's border).  With a mask, D is NOT premultiplied: the coarse bands carry some of the edit's colour from outside the
 *   mask into a halo of at most M pixels.
 *   whole = 1: dst holds the photograph per frame (eg3d_paste_back8's copy launch), and the whole window is written into it.  whole = 0: dst
 *   holds the box only, the shape eg3d_paste_back8 gives; what the blend changes in the margin outside the box is dropped.  An empty box:
 *   as eg3d_paste_back8 (needs no workspace).
 *   workspace: fp32, [N][C + 1][h_k][w_k] (the planes of D_k, then alpha_k) for k = 1..L, then [N][C][h_k][w_k] (R_k) for k = 1..L - 1;
 *   level 0 is never stored: blend_level1 samples it into LDS under each tile of level 1 (EG3D_BLEND_L1_TILE_W x _H level-0 pixels + a
 *   2-pixel halo) and blend_compose samples it again per pixel (a workgroup writes EG3D_BLEND_COMPOSE_TILE_W x _H window pixels).
 *   1 + (L - 1) + (L - 1) + 1 launches (+ the copy); no allocation, no synchronise: capturable.  No atomics, no sum across threads: both
 *   builds give the same bytes.
 *   Errors, before any launch: EG3D_ERR_INVALID for bands outside 1..EG3D_BLEND_MAX_BANDS, a NULL, short or misaligned (4 bytes) workspace
 *   where one is needed, and everything eg3d_paste_back8 refuses.  eg3d_paste_blend8_query_workspace is host only. */
#define EG3D_BLEND_MAX_BANDS 6
#define EG3D_BLEND_L1_TILE_W 64
#define EG3D_BLEND_L1_TILE_H 32
#define EG3D_BLEND_COMPOSE_TILE_W 64
#define EG3D_BLEND_COMPOSE_TILE_H 16
typedef struct eg3d_paste_blend8_params {
    const uint8_t* photo;              /* [Hp,Wp,C] */
    const uint8_t* edits;              /* [N,S,S,C] */
    const uint8_t* mask;               /* NULL, [S,S] (mask_frames = 1) or [N,S,S] (mask_frames = N) */
    uint8_t* dst;
    double m[6];
    double inv_feather;                /* 1 / feather width in aligned pixels; 0: a hard edge */
    int32_t N, Hp, Wp, C, S;
    int32_t x0, y0, x1, y1;            /* the bounding box; the entry derives the window */
    int32_t mask_frames;               /* 1 or N; ignored without a mask */
    int32_t whole;
    int32_t layout;
    int32_t bands;                     /* L = 1..EG3D_BLEND_MAX_BANDS */
    void* workspace;                   /* eg3d_paste_blend8_query_workspace's bytes */
    int64_t workspace_bytes;
} eg3d_paste_blend8_params;
int eg3d_paste_blend8_query_workspace(const eg3d_paste_blend8_params* p, int64_t* workspace_bytes);
int eg3d_paste_blend8(const eg3d_paste_blend8_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Head mattes (csrc/matte.hip; no reference counterpart -- the reference thresholds its depth, training/warping_loss.py:12-16, and never
 * pastes).  From a ragged binary mask in the aligned frame to the soft uint8 matte eg3d_paste_back8 takes as `mask`: an exact Euclidean
 * distance transform, applied once per morphology stage and once more for the edge.  Integers and per-thread fp64, no atomics, no sum
 * across threads: bit-identical between runs, batch sizes and the two builds; tests/support/matte_ref.py restates both entries.
 *
 * eg3d_edt2: src uint8 [N,H,W], foreground = src != 0  ->  sd2 int32 [N,H,W], the signed squared Euclidean distance in pixels between
 *   centres: + the squared distance to the nearest background pixel of the same frame at a foreground pixel, - the squared distance to
 *   the nearest foreground pixel at a background pixel; never 0.  Pixels outside the frame belong to neither class.
 *   1. Columns.  For every pixel, by a down and an up sweep of its column: g_bg = the distance |y - y'| to the nearest background pixel of
 *      the column, g_fg = to its nearest foreground pixel; a column without the class gives the sentinel 2^14.  One of the two is 0 at every
 *      pixel (the pixel itself), so one signed int16 holds both: g = +g_bg at a foreground pixel, -g_fg at a background pixel.
 *   2. Rows.  Foreground (y, x): sd2 = min over x' of (x - x')^2 + g_bg(y, x')^2; background: -min over x' of (x - x')^2 + g_fg(y, x')^2.
 *      A frame without the other class therefore gives exactly 2^28 (x' = x, the sentinel squared) -- every real distance is below 2^25.
 *      Each lane scans x' = x -/+ k from best = g(x)^2 and stops at k^2 >= best: the minimum is exact whatever the stop cuts.
 *   3. Stages.  n_stages = 0..EG3D_EDT_MAX_STAGES thresholds t[i]: for each in order the binary image becomes sd2 > t[i] and the transform
 *      runs again; sd2 is the transform of the last binary image.  Erosion by a disc of radius r (the outside counting as foreground) is
 *      t = floor(r^2); dilation is t = -floor(r^2) - 1.
 *   impl: EG3D_EDT_TILED -- any size; two launches per transform (one thread per column; then one workgroup per row, or several rows where
 *   they fit one, the row's g in LDS), g in the workspace (int16 [N,H,W]), an intermediate binary image written over g as +/-1.
 *   EG3D_EDT_RESIDENT -- frames of H W <= 16384 pixels: one workgroup per frame keeps g in LDS (32 KB) and runs every stage and the final
 *   transform in ONE launch; no workspace.  EG3D_EDT_AUTO -- TILED at every size: measured on MI355X, RESIDENT's one launch takes twice
 *   the time of TILED's ten on the default chain of a 128 x 128 frame (DESIGN.md 3.4 "Head mattes").  All three give the same integers.
 *   Errors, before any GPU work: EG3D_ERR_INVALID for a NULL pointer, N, H or W < 1, n_stages outside 0..4, an unknown impl, a short
 *   workspace; EG3D_ERR_UNSUPPORTED for H or W > 4096, N H W >= 2^31, or EG3D_EDT_RESIDENT with H W > 16384.
 *   eg3d_edt2_query_workspace is host only (0 bytes for the RESIDENT path). */
#define EG3D_EDT_AUTO 0
#define EG3D_EDT_RESIDENT 1
#define EG3D_EDT_TILED 2
#define EG3D_EDT_MAX_STAGES 4
typedef struct eg3d_edt2_params {
    const uint8_t* src;                /* [N,H,W] */
    int32_t* sd2;                      /* [N,H,W] */
    void* workspace;                   /* eg3d_edt2_query_workspace's bytes (may be 0: then unused) */
    int64_t workspace_bytes;
    int32_t N, H, W;
    int32_t n_stages;
    int32_t t[EG3D_EDT_MAX_STAGES];
    int32_t impl;
} eg3d_edt2_params;
int eg3d_edt2_query_workspace(const eg3d_edt2_params* p, int64_t* workspace_bytes);
int eg3d_edt2(const eg3d_edt2_params* p, void* stream);

/* eg3d_matte8: sd2 int32 [N,Hs,Ws] (eg3d_edt2's) -> the soft matte uint8 [N,Ho,Wo], Ho Ws == Wo Hs (one scale for both axes).  Host doubles:
 *   step = Ws / Wo, inv_step = Wo / Ws, shrink_px (output pixels the edge moves inwards; negative: outwards), inv_feather = 1 / the ramp's
 *   width in output pixels (0: a hard edge).  For every output pixel (X, Y), in fp64, every operation rounded on its own, in this order (no
 *   FMA contraction, no division on the device):
 *     1. u = (X + 0.5) step - 0.5,  v = (Y + 0.5) step - 0.5
 *     2. fx = floor(u), dx = u - fx, taps xa = clamp(fx, 0, Ws - 1), xb = clamp(fx + 1, 0, Ws - 1); y likewise
 *     3. a tap's value d = s > 0 ? sqrt(s) - 0.5 : -(sqrt(-s) - 0.5)     (the contour lies half-way between centres; sqrt correctly rounded)
 *     4. r0 = p00 + (p01 - p00) dx,  r1 = p10 + (p11 - p10) dx,  val = r0 + (r1 - r0) dy          (eg3d_paste_back8's order)
 *     5. e = val inv_step - shrink_px
 *     6. t = inv_feather > 0 ? min(max(e inv_feather, 0), 1) : (e > 0 ? 1 : 0)
 *     7. a = (t t) (3 - 2 t)
 *     8. out = uint8(rint(255 a)), ties to even
 *   An all-foreground frame gives 255 everywhere, an all-background frame 0 (the 2^28 sentinel).  One launch, one thread per output pixel.
 *   Errors, before any GPU work: EG3D_ERR_INVALID for a NULL pointer, a size < 1, Ho Ws != Wo Hs, step or inv_step <= 0, inv_feather < 0 or
 *   a NaN; EG3D_ERR_UNSUPPORTED for Hs or Ws > 4096, Ho or Wo > 16384, N Hs Ws or N Ho Wo >= 2^31. */
typedef struct eg3d_matte8_params {
    const int32_t* sd2;                /* [N,Hs,Ws] */
    uint8_t* dst;                      /* [N,Ho,Wo] */
    double step, inv_step, shrink_px, inv_feather;
    int32_t N, Hs, Ws, Ho, Wo;
} eg3d_matte8_params;
int eg3d_matte8(const eg3d_matte8_params* p, void* stream);

/* Measurement aid (bench.py): a register-only v_mfma_f32_32x32x16_f16 loop on caller-supplied fp16 data -- what the matrix pipe sustains on
 * this chip at its current power / clock state, timed inside the benchmark run.  in: 4096 x 8 fp16 (64 KiB); out: blocks x 256 floats;
 * executes blocks x 4 waves x iters x 24 MFMAs of 32 x 32 x 16.  No reference counterpart. */
int eg3d_probe_mfma_f16(const void* in, float* out, int blocks, int iters, void* stream);

/* ---- deterministic build (csrc/det.h; `make det` -> libeg3d_hip_det.so) ----------------------------------------------------------------
 * Both builds export these four.  In the deterministic build every floating-point atomic of the library is an exact fixed-point
 * accumulation (order-independent: bit-identical results from run to run), the accumulators living in a workspace the caller lends:
 *   eg3d_det_enabled()                 1 in the deterministic build, 0 in the normal one
 *   eg3d_det_workspace_bytes(n)        bytes for calls that accumulate into at most n float targets each (32 bytes per target + 4 KB)
 *   eg3d_det_set_workspace(ws, bytes)  lend it (16-byte aligned; cleared here, synchronises the stream); ws = NULL returns to float atomics.
 *                                      Calls of the library must then come from one stream at a time.
 *   eg3d_det_misses(out)               additions that fell back to a float atomic (target not bound by the call, |v| >= 2^53); synchronises
 * The reference has no such mode (PyTorch's backward kernels accumulate with atomicAdd the same way). */
int eg3d_det_enabled(void);
int64_t eg3d_det_workspace_bytes(int64_t max_elements_per_call);
int eg3d_det_set_workspace(void* workspace, int64_t bytes, void* stream);
int eg3d_det_misses(uint32_t* out, void* stream);
/* *target += sum of values[0..n), every value added by its own thread through the library's accumulation primitive: float atomics in the
 * normal build (order-dependent), the exact accumulator in the deterministic one (the sum is exact up to the final rounding whatever the
 * values' order and range -- tests/test_gpu_det.py checks that against an exact sum). */
int eg3d_det_accumulate(const float* values, int64_t n, float* target, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EG3D_HIP_H */
