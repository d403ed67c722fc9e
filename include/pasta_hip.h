/*
 * pasta_hip.h -- C ABI of libpasta_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the PASTA-GAN generator/discriminator hot path.  Every
 * entry point replaces one native (or ATen-delegated) call of the reference;
 * the reference interface it stands in for is cited per function as
 * <file>:<line> relative to the reference repository root.
 *
 * Conventions (all entry points)
 *   - plain pointers + sizes, no torch types.  Device pointers unless noted.
 *   - the CALLER allocates every output and workspace; the library never
 *     allocates device memory and keeps no mutable global state after load.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); the
 *     caller has already selected the device.
 *   - return 0 on success, non-zero on error; pasta_last_error() then returns a
 *     thread-local, NUL-terminated description (the Python shim raises
 *     RuntimeError with it, mirroring TORCH_CHECK in the reference wrappers).
 *   - dtype codes: PASTA_F32 = 0, PASTA_F16 = 1, PASTA_F64 = 2, PASTA_BF16 = 3.
 */
#ifndef PASTA_HIP_H
#define PASTA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PASTA_F32 = 0, PASTA_F16 = 1, PASTA_F64 = 2, PASTA_BF16 = 3 };

/* Library identification / error reporting. */
const char* pasta_last_error(void);
int         pasta_abi_version(void);           /* 22; bumps when a signature changes (entries added since: marked "additive at ABI 22") */
const char* pasta_build_info(void);            /* "gfx950 <date> <hip version>"    */

/* ------------------------------------------------------------------------- *
 * upfirdn2d -- pad, zero-stuff upsample, 2-D FIR, decimate (one launch).
 * Replaces: upfirdn2d_plugin.upfirdn2d(x, f, upx, upy, downx, downy, padx0,
 *           padx1, pady0, pady1, flip, gain)  torch_utils/ops/upfirdn2d.cpp:16
 *           (kernels torch_utils/ops/upfirdn2d.cu:29-200).
 * x: [N,C,inH,inW] with element strides in_stride[4] (N,C,H,W order);
 * f: float32 [fH,fW] dense row-major (always fp32, upfirdn2d.cpp:21);
 * y: [N,C,outH,outW] with out_stride[4]; outH/outW must equal
 *    (in*up + pad0 + pad1 - f + down) / down  (upfirdn2d.cpp:32-33).
 * ------------------------------------------------------------------------- */
int pasta_upfirdn2d(const void* x, const float* f, void* y, int dtype,
                    const int32_t in_size[4], const int64_t in_stride[4],
                    const int32_t f_size[2],
                    const int32_t out_size[4], const int64_t out_stride[4],
                    int upx, int upy, int downx, int downy,
                    int padx0, int padx1, int pady0, int pady1,
                    int flip, float gain, void* stream, float* y_amax,
                    const void* y_add);     /* ABI 18, optional: a tensor with y's shape, strides and type, added to the result on its way out.  The
                                               gradient of upfirdn2d is upfirdn2d (upfirdn2d.py:246-264): when x has further consumers their gradient
                                               rides here instead of in an addition pass over two tensors */

/* -------------------------------------------------------------------------
 * Producer-written operand pieces (ABI 19).  Replaces, for the low-pass in front of a stride-2 convolution
 * (torch_utils/ops/conv2d_resample.py:119-122: `x = upfirdn2d(x, f, padding)` then `conv2d(x, w, stride=2)`), the fp32 NCHW
 * intermediate of the reference by the matrix-core operand itself: y = upfirdn2d(x, f, up = down = 1, padding, flip, gain) for a
 * 4x4 filter f (fp32 [4][4] on the device) is written ONCE as PASTA_LAYOUT_PIECES16 -- units [N][C / 8][OH][2][OW] of 16 bytes: eight fp16
 * values of eight consecutive channels, piece 0 = h = fp16(v S), piece 1 = l' = fp16(2^11 (v S - h)) -- and the consumers (pasta_conv2d_ex /
 * pasta_conv2d_wgrad with pasta_conv_desc.x_layout = PASTA_LAYOUT_PIECES16) copy sixteen-byte pieces into LDS instead of gathering
 * channel-strided fp32 and splitting it at every launch.  OH = H + pady0 + pady1 - 3, OW likewise; the fp32 value in front of the split
 * is bit-identical to pasta_upfirdn2d's.
 *   x_amax  (in)  PASTA_AMAX_PARTS partial |max| of x (its producer's row, or pasta_tensor_amax).
 *   y_amax  (out) PASTA_AMAX_PARTS floats: x_amax times gain * sum |f| -- a bound of |y| known BEFORE the blur runs.  The power of two S
 *                 comes from this row on both sides (pass it as pasta_conv_desc.x_amax); being a power of two, the consumers' results do
 *                 not depend on which admissible S was used (tests/test_pieces_gpu.py scales the row by 2 and by 1/2).
 * pasta_pieces_bytes: size of the piece tensor (-1: C is not a multiple of 8).  pasta_pieces_unpack: (h + 2^-11 l') / S back to fp32
 * NCHW (tests and diagnostics: 22 of the 24 bits).
 * ------------------------------------------------------------------------- */
int64_t pasta_pieces_bytes(int N, int C, int H, int W);
int pasta_blur_pieces(const float* x, const float* f, void* pieces, const float* x_amax, float* y_amax,
                      int N, int C, int H, int W, int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream);
int pasta_pieces_unpack(const void* pieces, const float* y_amax, float* y, int N, int C, int H, int W, void* stream);
/* (ABI 20) an fp32 NCHW tensor whose partial maxima are known, split as the consuming kernels split it in their staging (bit for bit): for a
 * caller whose producer is not one of this library's kernels, and for the tests of the pieces-reading kernels. */
int pasta_pieces_pack(const float* x, const float* x_amax, void* pieces, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------- *
 * bias_act -- fused bias + activation + gain + clamp, and its 1st/2nd grads.
 * Replaces: bias_act_plugin.bias_act(x, b, xref, yref, dy, grad, dim, act,
 *           alpha, gain, clamp)  torch_utils/ops/bias_act.cpp:32
 *           (kernel torch_utils/ops/bias_act.cu:23-147).
 * All tensors are dense with identical layout, n elements; NULL = absent
 * (the reference passes an empty tensor).  b has size_b elements and is
 * indexed by (i / step_b) % size_b.  act = 1..9 (bias_act.py:23-33 cuda_idx).
 * grad = 0 forward, 1 first derivative (x is dy), 2 second derivative.
 * clamp < 0 disables clamping.
 * ------------------------------------------------------------------------- */
int pasta_bias_act(const void* x, const void* b, const void* xref,
                   const void* yref, const void* dy, void* y, int dtype,
                   int64_t n, int size_b, int64_t step_b, int grad, int act,
                   float alpha, float gain, float clamp, void* stream, float* y_amax);

/* Column sums used for the bias gradient (bias_act.py:173 `dx.sum(...)`):
 * db[c] = sum over all i with (i / step_b) % size_b == c of dx[i].
 * fp32 accumulate; db has dtype of dx.  work: size_b*nsplit floats scratch
 * (nsplit returned by pasta_bias_grad_workspace). */
int64_t pasta_bias_grad_workspace(int64_t n, int size_b, int64_t step_b);
int pasta_bias_grad(const void* dx, void* db, float* work, int dtype, int64_t n,
                    int size_b, int64_t step_b, void* stream);

/* First derivative and bias gradient in one pass over HBM (the pair bias_act.py:162-173 `dx = plugin.bias_act(dy, ...,
 * grad=1, ...)` + `db = dx.sum(...)`):  dx = dy * act'(yref / gain) * gain, zero where |yref| >= clamp >= 0, and
 * db[c] = sum of dx over its (n, c) planes (fp32 accumulate, fixed order).  act 1..3 (linear, relu, lrelu), fp32 or
 * fp16, tensors viewed as [outer, size_b, step_b] with step_b a multiple of 16 bytes and >= 256 packs of 16 bytes.
 * pasta_bias_act_grad_db_workspace returns the bytes of `work`, or 0 when the case is not covered (then call
 * pasta_bias_act(grad=1) followed by pasta_bias_grad).  yref may be NULL only for act 1 without clamp. */
int64_t pasta_bias_act_grad_db_workspace(int dtype, int64_t n, int size_b, int64_t step_b, int act);
int pasta_bias_act_grad_db(const void* dy, const void* yref, void* dx, void* db, float* work, int dtype, int64_t n,
                           int size_b, int64_t step_b, int act, float alpha, float gain, float clamp, void* stream, float* dx_amax);

/* ------------------------------------------------------------------------- *
 * Dense convolution family on fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 * Replaces the ATen/cuDNN calls behind torch_utils/ops/conv2d_gradfix.py:38,43
 * (forward), :125-128 (input gradient) and :140-148 (weight gradient).
 *
 * One descriptor covers conv2d, conv_transpose2d and both of their gradients:
 *   y[n, g*Og + o, oy, ox] = sum_{i,r,s} x[n, g*Ig + i, iy, ix] * w[...]
 * `transposed` selects conv_transpose2d semantics (weight [I, O/g, kh, kw]).
 * ------------------------------------------------------------------------- */
typedef struct pasta_conv_desc {
    int32_t N, C_in, H, W;        /* input  x: [N, C_in, H, W]  contiguous NCHW      */
    int32_t C_out, OH, OW;        /* output y: [N, C_out, OH, OW] contiguous NCHW    */
    int32_t kh, kw;               /* kernel size                                      */
    int32_t stride;               /* conv stride (conv2d) or upsampling (transposed) */
    int32_t pad_h, pad_w;         /* symmetric zero padding                           */
    int32_t groups;               /* 1 (training) or N-style grouped (eval modconv)   */
    int32_t transposed;           /* 0 = conv2d, 1 = conv_transpose2d                 */
    int32_t flip;                 /* 1 = true convolution (flip taps), 0 = correlation */
    int32_t math;                 /* PASTA_MATH_*: arithmetic of the matrix-core products (see below)  */
    float   wscale;               /* the weights are used as w * wscale (0 = 1): Conv2dLayer's `self.weight *
                                     self.weight_gain` (networks.py:171) folded into the weight packing; the weight
                                     gradient is returned with respect to the unscaled w (i.e. times wscale)        */
    int32_t io_dtype;             /* storage type of x, y, dy (and the fused residual): PASTA_F32 (default), PASTA_F16 or
                                     PASTA_BF16.  With 16-bit storage the stored element is the matrix-core operand: ONE
                                     product per multiply-add (v_mfma_f32_32x32x16_f16 / _bf16), fp32 accumulation and
                                     epilogue, one rounding on the way out -- the arithmetic of the reference's fp16
                                     blocks (networks.py:1107-1120) and of BASELINE config 5.  Weights, weight gradients,
                                     bias and the scale vectors stay fp32.  Only shapes the matrix-core kernels cover
                                     (>= 16 input channels per group, > 32 output channels; 3x3 / 1x1 weight gradients on
                                     rows of a multiple of 16 / 32 pixels): pasta_conv2d_plan / pasta_conv2d_wgrad_plan
                                     return an error otherwise and the caller converts that launch to fp32.            */
    const float* x_amax;          /* PASTA_MATH_F16X3 only, optional: PASTA_AMAX_PARTS partial |max| of the tensor passed as x
                                     (pasta_tensor_amax wrote them).  NULL: the launch computes them itself into its workspace
                                     (one extra pass over x).  A caller that uses a tensor in several launches (forward and
                                     weight gradient; input gradient and weight gradient) computes them once.            */
    const void*  x2;              /* optional second input tensor of a POINTWISE convolution (kh = kw = 1, stride 1, fp32 storage, PASTA_MATH_F16X3):
                                     x holds input channels [0, C1), x2 ([N, C_in - C1, H, W], contiguous) channels [C1, C_in) -- the convolution of
                                     torch.cat([x, x2], 1) (the merge layers, networks.py:5698-5700) without forming it.  NULL: one tensor.  An error
                                     where the pointwise kernel does not apply (pasta_conv2d_plan reports kernel 9 where it does)           */
    const float* x2_amax;         /* partial |max| of x2, as x_amax                                                      */
    int32_t      C1;              /* channels held by x when x2 is given                                                  */
    const float* dy_amax;         /* the same for dy (pasta_conv2d_wgrad only).  The WEIGHTS need nothing of the kind (ABI 17): their
                                     packing kernel finds one scale per output row itself at every launch, so no |max| of w is
                                     passed, cached or trusted across launches                                            */
    int32_t      x_layout;        /* ABI 19.  0 = x is a contiguous NCHW tensor of io_dtype (everything above).  PASTA_LAYOUT_PIECES16 = x is the
                                     producer-written operand of the three-product arithmetic (pasta_blur_pieces below): [N][C_in / 8][H][2][W] units of
                                     16 bytes, fp16 h[8] / l'[8] of v S, and x_amax (REQUIRED then) is the 256-float row the producer wrote -- the bound
                                     both sides take the power-of-two scale S from.  Served by the 3x3 stride-2 forward kernel and its weight gradient
                                     (pasta_conv2d_plan kernel 10, pasta_conv2d_wgrad_plan kernel 6: fp32 y / dy, PASTA_MATH_F16X3, one group, C_in a
                                     multiple of 8, pad 0) and by the eight-wave 3x3 stride-1 tile kernel, convolution or input gradient
                                     (pasta_conv2d_plan kernel 7: no input scale, one group, C_in a multiple of 8; pasta_pieces_pack writes such an
                                     operand from an fp32 tensor); the planners return an error for every other launch and the caller keeps the
                                     fp32 tensor. */
    int32_t      w_prepacked;     /* ABI 21.  1 = the workspace already holds this launch's packed weights and row scales (pasta_conv2d_pack_pair wrote them
                                     for THIS descriptor and these weights): the launch skips its packing kernel.  0 everywhere else.                 */
} pasta_conv_desc;

#define PASTA_LAYOUT_NCHW      0
#define PASTA_LAYOUT_PIECES16  1

/* Arithmetic of the convolution products.  Accumulation is fp32 in every mode.
 *   PASTA_MATH_F32    v_mfma_f32_32x32x2_f32: every product and sum is an fp32 FMA (bit-exact fp32 chains).
 *   PASTA_MATH_BF16X6 each fp32 operand is split into three bf16 pieces (24 significand bits) and a*b is formed
 *                     from six exact bf16 x bf16 products on v_mfma_f32_32x32x16_bf16: fp32-equivalent accuracy
 *                     (dropped terms < 2^-22 |ab|) at 2.67x the fp32 matrix-core rate.  Used by the 128x128- and
 *                     64x256-tile forward / input-gradient launches with >= 16 input channels per group and
 *                     by the 3x3 stride-1 weight gradient; all other launches run PASTA_MATH_F32.
 *   PASTA_MATH_BF16X3 two bf16 pieces per operand, three products (hi*hi, hi*mid, mid*hi): ~2^-16 relative error per
 *                     product, half of the matrix work -- the counterpart of the reference's `allow_tf32=True`
 *                     (training_loop_wo_flow_fullbody.py:247-249; TF32 keeps 2^-11).  Opt-in, never the default.
 *   PASTA_MATH_BF16   operands rounded to bf16, one product, fp32 accumulate and fp32 tensors in HBM: the arithmetic of
 *                     mixed-precision training (BASELINE config 5).  Opt-in.
 *   PASTA_MATH_F16X3  fp32-equivalent products from THREE fp16 products (v_mfma_f32_32x32x16_f16): each operand is scaled
 *                     by a power of two taken from its tensor's largest magnitude and split into fp16 pieces h + 2^-11 l'
 *                     (22 + 1 significand bits: representation error <= 2^-23, fp32's own rounding is 2^-24); h h, h l'
 *                     and l' h are exact in fp32 and accumulate in fp32; the result is scaled back exactly.  Half the
 *                     matrix work of BF16X6 at the same accuracy class (rms error against fp64 within 10 % of an fp32 FMA
 *                     chain's: the fp32 accumulation dominates both).  Range: activations keep full precision down to 2^-28
 *                     of their tensor's largest element; weights are scaled PER OUTPUT ROW (output channel of the launch) and keep
 *                     full precision down to 2^-16 of their row's largest element; both operands of a weight gradient down to
 *                     2^-17 of their tensor's; smaller elements contribute with an absolute error <= 2^-28 amax each.  Non-finite
 *                     elements are skipped by the scale and stay local.  fp32 storage only; same kernels and coverage as BF16X6,
 *                     per-sample modulated weights (pasta_conv2d_modulated) included since ABI 17.
 *   The split modes share kernels (template argument NP = pieces) and the same coverage.
 *   PASTA_MATH_DEFAULT = PASTA_MATH_F16X3 (round 3; BF16X6 before). */
enum { PASTA_MATH_DEFAULT = 0, PASTA_MATH_F32 = 1, PASTA_MATH_BF16X6 = 2, PASTA_MATH_BF16X3 = 3, PASTA_MATH_BF16 = 4, PASTA_MATH_F16X3 = 5 };

/* Largest finite magnitude of a contiguous fp32 tensor as PASTA_AMAX_PARTS partial maxima (parts[i] >= 0; the maximum over
 * i is the tensor's): the operand scales of PASTA_MATH_F16X3.  One pass at HBM rate, no atomics, no host round trip;
 * non-finite elements are skipped.  parts 16-byte aligned.  No reference counterpart (the reference hands fp32
 * tensors to cuDNN, conv2d_gradfix.py:38); it exists so that a tensor used by several launches is scanned once. */
#define PASTA_AMAX_PARTS 256
int pasta_tensor_amax(const void* x, int64_t numel, int dtype, float* parts, void* stream);
/* Producer-side maxima: the operators that WRITE activation tensors (pasta_upfirdn2d, pasta_bias_act, pasta_bias_act_grad_db,
 * pasta_scale_add, pasta_mod_bias_act(_bwd), pasta_spade_norm(_bwd) and the convolutions through pasta_conv_epilogue.y_amax) take
 * a last argument `float* y_amax` (NULL = off): PASTA_AMAX_PARTS floats ZEROED by the caller, into which the kernel leaves
 * partial maxima of the largest finite magnitude it stored (one agent-scope integer atomic per wavefront on the bit patterns:
 * order-independent, hence deterministic).  What pasta_tensor_amax would find, without the extra pass over the tensor. */

/* Bytes of scratch the forward / weight-gradient launches need (caller allocs). */
int64_t pasta_conv2d_workspace(const pasta_conv_desc* d);
int64_t pasta_conv2d_wgrad_workspace(const pasta_conv_desc* d);

/* Which forward-type kernel instance the launch will use: 0 = 128x128 tile, 1 = 64x256,
 * 2 = 32x256, 3 = 64x64 (rows = output channels, columns = pixels).  Reporting only. */
int pasta_conv2d_tile(const pasta_conv_desc* d);

/* (ABI 21) One weight tensor packed for TWO launches by ONE kernel -- typically a convolution and its input gradient (the same weights, transposed and
 * mirrored), so that the backward pass finds its operand packed: 120 of the 310 packing launches of a training step.  ws_a / ws_b: the workspaces the two
 * launches will be given (pasta_conv2d_workspace(da / db) bytes); *packed_mask = 3 when both were packed (set pasta_conv_desc.w_prepacked = 1 in both
 * launches), 0 when the pair is not served (16-bit storage, another arithmetic than PASTA_MATH_F16X3, few-channel or packed-K launches, scale vectors or
 * modulated weights are the CALLER's business: it must not ask for those) -- the launches then pack for themselves as always. */
int pasta_conv2d_pack_pair(const float* w, const pasta_conv_desc* da, void* ws_a, int64_t ws_a_bytes, const pasta_conv_desc* db, void* ws_b, int64_t ws_b_bytes,
                           void* stream, int* packed_mask);

/* The forward-type kernels (conv2d, conv_transpose2d and both input gradients), as pasta_conv2d_plan names them.  The split kernels (1 - 8) run
 * every split arithmetic and 16-bit storage; 9, 10 and 13 PASTA_MATH_F16X3 on fp32 tensors only. */
enum {
    PASTA_FWD_F32       = 0,   /* conv_fwd_kernel: fp32 MFMA, every shape */
    PASTA_FWD_BASE      = 1,   /* conv_fwd_bf16x6_kernel: split arithmetic, any lattice */
    PASTA_FWD_ROWS      = 2,   /* conv_fwd_rows_bf16x6_kernel: row reuse, 3-wide stride-1 kernels on rows of a multiple of 32 pixels */
    PASTA_FWD_PAIR      = 3,   /* ... its parity-pair mode: 3x3 stride-2 conv_transpose2d onto 2H(+1) x 2W(+1), last row / column by conv_t2_edge_kernel */
    PASTA_FWD_ROWS2D_R4 = 4,   /* conv_fwd_rows2d_bf16x6_kernel<128,128,4>: 3x3 stride 1, pixel tiles of 4 rows x 32 columns */
    PASTA_FWD_ROWS2D_R2 = 5,   /* ... <128,128,2>: 2 rows x 64 columns */
    PASTA_FWD_ROWS2D_R8 = 6,   /* ... <64,256,8>: 8 rows x 32 columns on the 64-channel tile */
    PASTA_FWD_ROWS2D_WIDE = 7, /* ... eight waves on a 128 x 256 tile, fp32-equivalent products on fp32 tensors; takes PASTA_LAYOUT_PIECES16 */
    PASTA_FWD_PACKED_K  = 8,   /* conv_fwd_bf16x6_kernel, K over (channel, tap) pairs: < 16 input channels, >= 64 pairs (the 7x7 RGB stems) */
    PASTA_FWD_1X1       = 9,   /* conv1x1_f16x3_kernel: pointwise, >= 16 input and > 32 output channels, optionally two input tensors (x2) */
    PASTA_FWD_3X3S2     = 10,  /* conv3x3s2_f16x3_kernel: 3x3 stride-2 conv2d, pads 0 / 1, power-of-two output widths; takes PASTA_LAYOUT_PIECES16 */
    PASTA_FWD_FEWCIN    = 11,  /* conv1x1_fewcin_kernel: pointwise, <= 16 input channels, fp32 FMAs on the raw weights (*math = PASTA_MATH_F32) */
    PASTA_FWD_FEWCOUT   = 12,  /* conv1x1_fewcout_kernel: pointwise, <= 16 output channels, likewise */
    PASTA_FWD_T2        = 13   /* conv_t2_f16x3_kernel: 3x3 stride-2 conv_transpose2d, pad 0, onto 2H(+1) x 2W(+1) in one pass over the input lattice */
};

/* The full launch plan of pasta_conv2d(_ex) for d, for reporting (bench.py attributes time and FLOPs to kernel
 * families with it): *tile as pasta_conv2d_tile, *ksplit = number of K slices (> 1: partial sums in the workspace,
 * reduced by a second kernel), *math = the PASTA_MATH_* actually used (launch_flags = OR of PASTA_PLAN_*:
 * what the launch will pass besides x, w, y -- an iscale vector, which the split kernels take in their staging for fp32
 * storage and fp32-equivalent products only; an oscale vector; a fused epilogue), *launches = launches of the main kernel (conv_transpose2d:
 * one per output parity class unless the classes share a grid), *kernel = PASTA_FWD_*.
 * With PASTA_FWD_PACKED_K the workspace also holds the offset table and a zero-padded copy of the input, and two small kernels fill them; with
 * PASTA_FWD_T2 the input's last column, gathered by a small kernel in front.
 * A conv_transpose2d launched as one launch per output parity class (*launches > 1: stride >= 3, or stride 2 on the fp32 kernel or onto a plane
 * under 2 x 2) reports the kernel of each class's launch: every class takes the same one.
 * pasta_conv2d_plan answers with the choice pasta_conv2d(_ex) / pasta_conv2d_modulated make for the same flags.  Any out pointer may be NULL. */
#define PASTA_PLAN_ISCALE   1
#define PASTA_PLAN_OSCALE   2
#define PASTA_PLAN_EPILOGUE 4
#define PASTA_PLAN_MODULATED 8   /* pasta_conv2d_modulated (per-group modulated weights) */
#define PASTA_PLAN_NOISE    16   /* the epilogue adds noise (pasta_conv_epilogue.noise; with PASTA_PLAN_EPILOGUE): not kernels 9 - 12 */
int pasta_conv2d_plan(const pasta_conv_desc* d, int launch_flags, int* tile, int* ksplit, int* math, int* launches, int* kernel);

/* The weight-gradient kernels, as pasta_conv2d_wgrad_plan names them. */
enum {
    PASTA_WGRAD_F32      = 0,  /* conv_wgrad_kernel: fp32 MFMA, taps x 64 x 64 tiles, every shape */
    PASTA_WGRAD_SMALLCIN = 1,  /* conv_wgrad_smallcin_kernel: <= 8 input channels, (channel, tap) pairs as GEMM columns */
    PASTA_WGRAD_3X3      = 2,  /* conv_wgrad3x3_bf16x6_kernel: split; 3x3, stride 1, pad 1, rows of a multiple of 32 pixels, or of exactly 16 */
    PASTA_WGRAD_3X3S2    = 3,  /* conv_wgrad3x3s2_bf16x6_kernel: split; 3x3, stride 2, pad 0 or 1, rows of a multiple of 16 pixels */
    PASTA_WGRAD_1X1      = 4,  /* conv_wgrad1x1_bf16x6_kernel: split; 1x1, stride 1, planes of a multiple of 32 pixels, >= 16 channels */
    PASTA_WGRAD_FEWCIN   = 5,  /* wgrad1x1_fewcin_kernel: 1x1, <= 8 input channels, planes of a multiple of 4 pixels, one fp32 pass over dy */
    PASTA_WGRAD_3X3S2_PIECES = 6   /* conv_wgrad3x3s2_pieces_kernel: PASTA_WGRAD_3X3S2's shapes with pad 0 and x as PASTA_LAYOUT_PIECES16 */
};

/* Same for pasta_conv2d_wgrad: *kernel = PASTA_WGRAD_*.
 * The K slices of kernels 2 - 4 can be read off pasta_conv2d_wgrad_workspace, and tests/conv16_cases.py does: the workspace is 2 x 256 floats
 * (the operands' partial maxima) followed by one slab per slice of groups x kh x kw x A x B floats, A and B the two per-group channel counts
 * rounded up to the channel tile -- 64, or 128 for kernel 4 with more than 64 channels on both sides.  This layout is part of the contract. */
int pasta_conv2d_wgrad_plan(const pasta_conv_desc* d, int* kernel);

/* y = conv(x, w).  w is the PyTorch-layout weight ([C_out, C_in/g, kh, kw], or
 * [C_in, C_out/g, kh, kw] when transposed).  Optional fused epilogue:
 *   y = y * oscale[n, c] (NULL = 1)  -- demodulation, networks.py:77-79
 * and optional fused prologue on x:
 *   x'[n, c, :, :] = x * iscale[n, c] (NULL = 1) -- modulation, networks.py:74. */
int pasta_conv2d(const void* x, const float* w, void* y,      /* x, y: elements of d->io_dtype; w: fp32 */
                 const float* iscale, const float* oscale,
                 const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* Optional fused epilogue of pasta_conv2d_ex: after the output scale,
 *   y = clamp(act(y + noise * noise_strength[0] + res + bias[c]) * gain)
 * -- Conv2dLayer's bias_act (training/networks.py:176-178) and, with oscale = the demodulation coefficients and the noise
 * operand, the whole tail of SynthesisLayer (networks.py:77-82, 313-314: x * dcoefs + noise, bias_act) in the convolution's
 * own epilogue; forward only (the training path keeps pasta_mod_bias_act, whose backward needs the convolution output).
 * act: 1 linear, 2 relu, 3 lrelu (bias_act.py:24-26); bias NULL = none; clamp < 0 = none. */
typedef struct pasta_conv_epilogue {
    const float* bias;            /* [C_out] or NULL */
    int32_t act;
    float alpha, gain, clamp;
    const void* res;              /* (elements of d->io_dtype) [N, C_out, OH, OW] added to the convolution BEFORE bias / activation, or NULL
                                     (residual sums and the halves of a convolution over a channel concatenation without a
                                     pass of their own).  Measured on the two uses this path offers -- merge_conv over
                                     torch.cat (networks.py:5690-5693) as two 1x1 convolutions, and the SPADE block's
                                     y + conv(x) (:5273) -- it is time-neutral (+0.4 % / 0.0 %), so the networks keep the
                                     reference's formulation and the operand stays an option of the operator. */
    const float* noise;           /* fp32 [OH*OW] (noise_per_sample 0) or [N][OH*OW] (1), or NULL */
    const float* noise_strength;  /* device scalar (SynthesisLayer.noise_strength); required with noise */
    int32_t noise_per_sample;
    float* y_amax;                /* optional: PASTA_AMAX_PARTS floats, ZEROED by the caller, that receive partial maxima of the
                                     largest finite |y| (fp32 storage): the launch that consumes y under PASTA_MATH_F16X3 then needs
                                     no scan of y (see "producer-side maxima" below).  NULL = off. */
} pasta_conv_epilogue;

/* pasta_conv2d with the epilogue above (ep NULL = plain pasta_conv2d). */
int pasta_conv2d_ex(const void* x, const float* w, void* y,
                    const float* iscale, const float* oscale, const pasta_conv_epilogue* ep,
                    const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* The input-activation mask (additive at ABI 22).  A launch that writes the gradient dx of a layer's INPUT x holds x; where x is the activated
 * output of the layer in front, y = clamp(act(u) * gain) with act linear / relu / lrelu, the derivative of that activation is a function of y
 * alone (bias_act.cu:38-146: gain or gain * alpha by the sign of y, zero where |y| >= clamp), so the launch can hand back dz = dx * act'(y) --
 * the gradient at the OUTPUT of the convolution in front -- from its own saved tensor, and that layer's stand-alone pass
 * (pasta_bias_act with grad = 1: two reads and a write of the activation) does not run.  The rule is the one pasta_bias_act applies
 * (csrc/common.h, act_grad1): the result is bit-identical to launch + pass. */
typedef struct pasta_act_mask {
    const void* m;                /* the activated tensor, laid out like the launch's output (same shape, strides and element type) */
    int32_t act;                  /* 1 linear, 2 relu, 3 lrelu */
    float alpha, gain, clamp;     /* of the activation that produced m; clamp < 0 = none */
} pasta_act_mask;

/* pasta_conv2d_ex whose store computes  y = (conv [+ ep->res]) * act'(mask->m)  (mask NULL = pasta_conv2d_ex).  The residual is added BEFORE the
 * mask (another consumer's gradient of the same tensor), ep->y_amax sees the masked value.  ep, when given, is linear without bias, gain, clamp or
 * noise; no scale vectors.  Served where pasta_conv2d_mask_available answers 1 for the launch's flags -- the default arithmetic on fp32 tensors
 * without K slices on the 2-D tiles of the 3x3 stride-1 launches (plan kernels 4 - 7) --, an error elsewhere: the caller then runs the pass. */
int pasta_conv2d_masked(const void* x, const float* w, void* y,
                        const float* iscale, const float* oscale, const pasta_conv_epilogue* ep, const pasta_act_mask* mask,
                        const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                        void* stream);
int pasta_conv2d_mask_available(const pasta_conv_desc* d, int launch_flags);       /* 1 / 0; -1: the descriptor is refused */

/* pasta_upfirdn2d whose store computes  y = (gain * fir(x) [+ y_add]) * act'(mask->m)  (mask NULL = pasta_upfirdn2d): the filter's transpose that
 * ends the backward of a low-pass in front of a stride-2 convolution, with the low-pass's saved input as the mask.  Served by the tile and the
 * small-plane kernels on dense fp32 NCHW tensors; pasta_upfirdn2d_mask_available answers 1 where one of them takes the launch
 * (dense NCHW assumed), and the masked launch is an error elsewhere. */
int pasta_upfirdn2d_masked(const void* x, const float* f, void* y, int dtype,
                           const int32_t in_size[4], const int64_t in_stride[4],
                           const int32_t f_size[2],
                           const int32_t out_size[4], const int64_t out_stride[4],
                           int upx, int upy, int downx, int downy,
                           int padx0, int padx1, int pady0, int pady1,
                           int flip, float gain, void* stream, float* y_amax,
                           const void* y_add, const pasta_act_mask* mask);
int pasta_upfirdn2d_mask_available(int dtype, const int32_t in_size[4], const int32_t f_size[2],
                                   int upx, int upy, int downx, int downy,
                                   int padx0, int padx1, int pady0, int pady1);

/* The bias gradient of a layer that deferred its activation gradient to the reader of its output (additive at ABI 22): db[c] = sum of dx over the
 * planes of channel c, where dx already is the gradient at the convolution's output.  One read and no store; the shapes, the workspace
 * (pasta_bias_act_grad_db_workspace with act = 1) and the order of the partial sums are those of pasta_bias_act_grad_db, so db has the bits
 * that pass would have produced. */
int pasta_bias_sum_db(const void* dx, void* db, float* work, int dtype, int64_t n, int size_b, int64_t step_b, void* stream);

/* Modulated convolution in its per-sample-weight form (networks.py:84-94, the `fused_modconv` branch test.py runs):
 * d describes the grouped convolution the reference launches (groups = N samples, C_in = N*I, C_out = N*O, x viewed as
 * [1, N*I, H, W]); w is the ONE shared weight [O, I, kh, kw] ([I, O, kh, kw] when d->transposed).  The weight-packing
 * kernel forms each group's operand  w[o,i,:] * styles[n,i] * dcoefs[n,o]  on its way into the staging layout, so the
 * [N, O, I, kh, kw] tensor of the reference and the passes that build it do not exist (dcoefs NULL = no demodulation;
 * pasta_demod_coefs computes them).  Forward only. */
int pasta_conv2d_modulated(const void* x, const float* w, const float* styles, const float* dcoefs, void* y,
                           const pasta_conv_epilogue* ep, const pasta_conv_desc* d, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* dw = d(conv)/dw given x and dy (same descriptor as the forward); x, dy: elements of d->io_dtype, dw: fp32. */
int pasta_conv2d_wgrad(const void* x, const void* dy, float* dw,
                       const pasta_conv_desc* d, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Weight gradient AND style gradient of the shared-weight modulated convolution  y = conv(x * styles[n, i], w)  (training/networks.py:72-76, the
 * training branch of modulated_conv2d) WITHOUT the tensor x * styles: the weight-gradient kernels run on the unmodulated x with K slices that do
 * not straddle samples, and the reduction forms  dw[o,i,t] = wscale sum_n styles[n,i] Dw_n[o,i,t]  and  dstyles[n,i] = sum_{o,t} wscale w[o,i,t] Dw_n[o,i,t]
 * (Dw_n: sample n's gradient with respect to the weight it saw).  With the forward launched as pasta_conv2d(x, w, iscale = styles) and the input
 * gradient as pasta_conv2d(dy, w, oscale = styles) the reference's  x * styles  (one pass to form it, its saved copy, one pass to scale the input
 * gradient back, two reads for sum_hw dx x) is gone from the training step.  d, x, dy, x_amax / dy_amax as for pasta_conv2d_wgrad (x_amax: of the
 * UNMODULATED x); styles: [N, C_in] fp32; w: the weight; dw: its gradient; dstyles: [N, C_in].  fp32 storage, groups == 1, N <= 32, the split kernels'
 * shapes (pasta_conv2d_wgrad_plan kernels 2 - 4): pasta_conv2d_wgrad_modulated_workspace returns -1 where it does not apply (ABI 18). */
int64_t pasta_conv2d_wgrad_modulated_workspace(const pasta_conv_desc* d);
int pasta_conv2d_wgrad_modulated(const void* x, const void* dy, const float* styles, const float* w, float* dw, float* dstyles,
                                 const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Modulated-convolution helpers (training/networks.py:36-94).
 * ------------------------------------------------------------------------- */
/* Demodulation coefficients (networks.py:65-68):
 *   d[n,o] = rsqrt(sum_{i,k} (w[o,i,k] * styles[n,i])^2 + eps),  w: [O,I,KK] fp32, styles: [N,I] fp32, d: [N,O] fp32.
 * One workgroup per output channel, tap-summed squared weights in LDS, wavefront-shuffle reduction over I (I <= 4096);
 * the reference's per-sample weight tensor [N,O,I,kh,kw] is never formed. */
int pasta_demod_coefs(const float* w, const float* styles, float* d, int N, int O, int I, int KK,
                      float eps, void* stream);

/* y[n,c,h,w] = x[n,c,h,w] * a[n,c] + (b ? b[n,0,h,w] : 0)   fma.py:15 with the
 * broadcast shapes modulated_conv2d uses (a: [N,C], b: [N,HW] or [HW], or NULL) */
/* (this and the following plane kernels: `dtype` = storage type of the activation tensors -- PASTA_F32, PASTA_F16 or
 * PASTA_BF16; per-channel scales, statistics, bias, noise strength and partial sums are always fp32, as is the arithmetic) */
int pasta_scale_add(const void* x, const float* a, const void* b, void* y, int dtype,
                    int N, int C, int64_t HW, int b_per_sample, void* stream, float* y_amax);

/* Per-(n,c) plane reductions used by fma / modulation backward:
 * out[n,c] = sum_hw p[n,c,hw] * q[n,c,hw]   (q NULL => sum of p) */
int pasta_plane_dot(const void* p, const void* q, float* out, int dtype, int64_t planes,
                    int64_t HW, void* stream);

/* Tail of SynthesisLayer in one pass (networks.py:72-82 demodulation + noise, :313-314 bias_act):
 *   y = clamp(act(u * d[n,c] + noise * strength[0] + b[c]) * gain),  act = 1 (linear) or 3 (lrelu),
 * u: [N,C,HW] convolution output, d: [N,C] demodulation coefficients (NULL = 1), noise: [N,HW] (noise_per_sample)
 * or [HW] or NULL, strength: device scalar, b: [C] or NULL, clamp < 0 = none.
 * Backward: du = dz * d with dz = dy * act'(y) * gain (0 where |y| >= clamp), and per (plane, 4096-element chunk)
 * the triple (sum dz*u, sum dz*noise, sum dz) in `partial` ([N*C][chunks][3] floats, pasta_mod_bias_act_bwd_workspace
 * bytes), from which the caller forms dd[n,c], dstrength and db[c]. */
int pasta_mod_bias_act(const void* u, const float* d, const float* noise, const float* strength, const float* b, void* y,
                       int dtype, int N, int C, int64_t HW, int noise_per_sample, int act, float alpha, float gain, float clamp,
                       void* stream, float* y_amax);
int64_t pasta_mod_bias_act_bwd_workspace(int N, int C, int64_t HW);
int pasta_mod_bias_act_bwd(const void* dy, const void* y, const void* u, const float* d, const float* noise, void* du,
                           float* partial, int dtype, int N, int C, int64_t HW, int noise_per_sample, int act, float alpha, float gain,
                           float clamp, void* stream, float* du_amax);

/* ------------------------------------------------------------------------- *
 * SPADE normalisation (training/networks.py:4371-4379):
 *   out = InstanceNorm(x) * (1 + gamma) + beta, eps 1e-5, biased variance.
 * stats: [N*C, 2] (mean, rstd) written by the forward, read by the backward.
 * Optional fused activation (act = 2): out = min(relu(out) * gain, clamp) -- what the Spade_Conv2dLayer that
 * consumes the block's output applies in front of its convolution (networks.py:4346-4352); act 0/1 = none,
 * clamp < 0 = none.  The backward then needs beta (to recompute the activation mask) and a dbeta buffer.
 * gamma and beta (and dgamma, dbeta) may be the two channel halves of ONE [N, 2C, H, W] tensor -- the output (gradient) of a
 * single convolution with the concatenated conv_gamma / conv_beta weights: C = channels of x, gb_stride / dgb_stride = the
 * distance in elements between consecutive samples of gamma (dgamma), 0 = C * HW (separate contiguous tensors).
 * ------------------------------------------------------------------------- */
int pasta_spade_norm(const void* x, const void* gamma, const void* beta,
                     void* out, float* stats, int dtype, int64_t planes, int64_t HW,
                     float eps, int act, float gain, float clamp, int C, int64_t gb_stride, void* stream, float* y_amax);
int pasta_spade_norm_bwd(const void* dout, const void* x, const void* gamma,
                         const float* stats, void* dx, void* dgamma,
                         void* dbeta, int dtype, int64_t planes, int64_t HW,
                         const void* beta, int act, float gain, float clamp, int C, int64_t gb_stride, int64_t dgb_stride,
                         void* stream, float* dx_amax, float* dgb_amax,      /* dgb_amax: |max| over what is written to dgamma AND dbeta (they
                                                                               feed one convolution when they are halves of one tensor) */
                         const void* dx_add);                                /* ABI 18, optional ([planes, HW] like dx): added to dx on its way out -- the
                                                                               gradient another consumer of x returned (a block's second normalisation
                                                                               of the same tensor), instead of an addition pass over both */

/* ------------------------------------------------------------------------- *
 * Garment features of the SPADE stage (training/networks.py:5777-5800, get_spade_feat): fp32, NCHW.
 *   backward = 0:  out[n,c,i] = a[n,c,i] * (1 - hole[n,i]) + hole[n,i]  * inv_count[n] * sum_j a[n,c,j] * valid[n,j]
 *   backward = 1:  out[n,c,i] = a[n,c,i] * (1 - hole[n,i]) + valid[n,i] * inv_count[n] * sum_j a[n,c,j] * hole[n,j]   (a = d out)
 * valid, hole: [N, HW]; inv_count: [N]; a / out: sample strides in elements (0 = C * HW), so that the two garments' results
 * are written into (their gradients read from) the channel halves of ONE [N, 2C, H, W] tensor -- no torch.cat.
 * ------------------------------------------------------------------------- */
int pasta_masked_mean_fill(const float* a, const float* valid, const float* hole, const float* inv_count, float* out,
                           int N, int C, int64_t HW, int64_t a_sample_stride, int64_t out_sample_stride, int backward,
                           void* stream, float* y_amax);

/* ------------------------------------------------------------------------- *
 * ADA augmentation (training/augment.py:121-431).
 * pasta_ada_matrices: sample s turns its draws u[s, :] ~ U(0,1), z[s, :] ~ N(0,1) into the inverse geometric
 *   transform g_inv[s] (3x3 row-major, augment.py:186-263) and the colour transform c[s] (4x4, :306-350); margins[4]
 *   = the reflect-padding widths (x0, y0, x1, y1) over the whole batch (:272-282).  Column order of u / z = the order
 *   augment.py draws them (the enum in csrc/augment.hip; training/augment.py DRAWS_U / DRAWS_Z).  p: device scalar,
 *   the overall probability multiplier (AugmentPipe.p).  debug_percentile < 0 = off (:179-180).
 * pasta_ada_theta: theta[s] = (a @ g_inv[s] @ b)[:2, :]; a, b are HOST arrays of 9 floats (:285-296).
 * pasta_color_affine: mode 0: out[n, :, p] = c[n][:3, :3] @ x[n, :, p] + c[n][:3, 3] for [N,3,HW] images (:356-360);
 *   mode 1: the adjoint (c[n][:3, :3]^T, no offset); mode 2: the linear part alone (for second derivatives).
 * ------------------------------------------------------------------------- */
typedef struct pasta_ada_config {
    float xflip, rotate90, xint, xint_max;
    float scale, rotate, aniso, xfrac, scale_std, rotate_max, aniso_std, xfrac_std;
    float brightness, contrast, lumaflip, hue, saturation, brightness_std, contrast_std, hue_max, saturation_std;
} pasta_ada_config;
int pasta_ada_matrices(const float* u, const float* z, int64_t n, int u_cols, int z_cols, const float* p,
                       const pasta_ada_config* cfg, int width, int height, int channels, int hz_pad,
                       float debug_percentile, float* g_inv, float* c, int32_t* margins, void* stream);
int pasta_ada_theta(const float* g_inv, int64_t n, const float* a, const float* b, float* theta, void* stream);
int pasta_color_affine(const float* x, const float* c, float* out, int64_t n, int64_t hw, int mode, void* stream);
/* grid[n, y, x, :] = theta[n] @ ((2x + 1) / W - 1, (2y + 1) / H - 1, 1): F.affine_grid(theta, [n, C, H, W], align_corners=False) (:297) */
int pasta_ada_grid(const float* theta, int64_t n, int H, int W, float* grid, void* stream);
/* y = grid_sample(x, affine_grid(theta, [n, C, OH, OW], align_corners=False), bilinear, zeros, align_corners=False)
 * (augment.py:297-298) without the grid tensor; x: [n, C, IH, IW], theta: [n, 2, 3].  The adjoint is the gradient with
 * respect to x, computed as a gather (no atomics: bitwise reproducible). */
int pasta_affine_sample(const float* x, const float* theta, float* y, int64_t n, int C, int IH, int IW, int OH, int OW, void* stream);
int pasta_affine_sample_adjoint(const float* dy, const float* theta, float* dx, int64_t n, int C, int IH, int IW, int OH, int OW,
                                void* stream);

/* ------------------------------------------------------------------------- *
 * grid_sample under a general sampling grid.  Replaces: grid_sample_gradfix.grid_sample(input, grid)
 * torch_utils/ops/grid_sample_gradfix.py:22-83 -- F.grid_sample(bilinear, zeros, align_corners=False) forward (:44-51)
 * and aten::grid_sampler_2d_backward for both gradients (:61-67).
 * x: [n, C, IH, IW] dense, dtype PASTA_F32 / PASTA_F16 / PASTA_BF16 / PASTA_F64 (`dtype`); grid: [n, OH, OW, 2] dense,
 * (x, y) in [-1, 1], dtype `grid_dtype` = `dtype` (or PASTA_F32 for a 16-bit image); y, dy: [n, C, OH, OW] of `dtype`.
 * fp32 coordinates, weights and sums (fp64 for PASTA_F64).  n <= 65535, OH * OW < 2^31, C <= 65535 * 16.  Added in ABI 21 without a bump (purely additive).
 * pasta_grid_sample_backward: dx = S^T dy ([n, C, IH, IW], `dtype`; NULL = not wanted) and grad_grid ([n, OH, OW, 2],
 * `grid_dtype`; NULL = not wanted; needs x) in one pass over dy.  dx is accumulated with float atomics, so it is not
 * bitwise reproducible from run to run (ATen's is not either); grad_grid is (one thread per output point, no atomics).
 * ws: fp32 workspace of pasta_grid_sample_backward_workspace() bytes (nonzero only for a 16-bit dx); the entry zeroes it.
 * ------------------------------------------------------------------------- */
int pasta_grid_sample(const void* x, const void* grid, void* y, int64_t n, int C, int IH, int IW, int OH, int OW, int dtype,
                      int grid_dtype, void* stream);
int64_t pasta_grid_sample_backward_workspace(int64_t n, int C, int IH, int IW, int dtype);
int pasta_grid_sample_backward(const void* dy, const void* x, const void* grid, void* dx, void* dgrid, void* ws, int64_t n, int C,
                               int IH, int IW, int OH, int OW, int dtype, int grid_dtype, void* stream);

/* nan_to_num(t, nan, posinf, neginf) in place over n float tensors in one launch per 96 tensors
 * (training_loop_wo_flow_fullbody.py:513-515; misc.py:45).  ptrs / numels: HOST arrays of device pointers / element
 * counts (< 2^31 each); empty tensors are skipped. */
int pasta_nan_to_num_multi(float* const* ptrs, const int64_t* numels, int n, float nan, float posinf, float neginf,
                           void* stream);

/* ------------------------------------------------------------------------- *
 * Body-part patch pipeline (training/dataset.py:838-927 `normalize`,
 * which the reference runs on the host through cv2.warpPerspective, ~28 warps per sample).
 * uint8 HWC images; bilinear interpolation in OpenCV's fixed point (1/32-pixel source
 * coordinates, 2^15 weights).  OpenCV is unavailable where this was built: the arithmetic is
 * held bit for bit to oracle/ref_patches.py's restatement of the published algorithm, parity
 * with cv2 itself is UNPINNED.
 * ------------------------------------------------------------------------- */
/* dst[b] = cv2.warpPerspective(src[src_index ? src_index[b] : b], M_b, (dw, dh), INTER_LINEAR, border) for b < B.
 * src: [*, sh, sw, C] uint8, dst: [B, dh, dw, C]; minv: [B][9] doubles = the INVERTED matrices (destination -> source,
 * what cv2 forms first); valid (optional, [B]): 0 writes zeros; border: 0 = BORDER_CONSTANT (0), 1 = BORDER_REPLICATE. */
int pasta_warp_perspective_u8(const uint8_t* src, const int32_t* src_index, const double* minv, const uint8_t* valid,
                              uint8_t* dst, int B, int sh, int sw, int dh, int dw, int C, int border, void* stream);

/* dataset.py:884-888 / 894-898 for N samples x P parts in one pass: out[n] starts black; for k = 0..P-1 with valid[n][k]:
 * where channel 0 of warpPerspective(masks[n][k], BORDER_CONSTANT) is 255, the pixel becomes warpPerspective(patches[n][k]).
 * patches, masks: [N, P, ph, pw, 3] uint8; minv: [N][P][9] doubles (destination -> patch); out: [N, H, W, 3];
 * part_mask (optional): [N, P, H, W] receives each part's 0 / 1 mask (the reference keeps those of the four arm parts). */
int pasta_patch_composite_u8(const uint8_t* patches, const uint8_t* masks, const double* minv, const uint8_t* valid,
                             uint8_t* out, uint8_t* part_mask, int N, int P, int ph, int pw, int H, int W, void* stream);

/* The geometry of the ten body parts of M people in ONE launch (csrc/part_geometry.hip; added in ABI 22 without a
 * bump, purely additive): what training/patch_pipeline.py's part_matrices and adjugate_inverse do on the host, one part at a
 * time.  keypoints: [M, 18, 3] doubles (x, y, confidence; device).  Every output may be NULL (not written):
 *   quads [M,10,4,2] float32 the source quadrilaterals; fwd / back [M,10,9] doubles, image -> patch and patch -> image;
 *   fwd_inv / back_inv [M,10,9] doubles, their inverses (the `minv` of the warp and composite entries); m_inv [M,10,9] float32,
 *   back cast; valid [M,10] uint8.  A part whose key points are missing is zeros in every output.
 * The rule (a SECOND rule next to the host's LAPACK solve, which no elimination reproduces to the last bit):
 *   1. quadrilateral: part_quadrilateral operation for operation in float32 -- the key points converted to float32 first, x_pad
 *      added after that in float32; a key point is seen when its confidence >= 0.1 (compared in double); a thigh without its knee
 *      and, with shin_fallback, a shin without its ankle go straight down to row image_height - 1; a head without the nose is the
 *      square on the shoulder line whose normal is negated when normal[1] > 0; _box_around's corner order, the head's [b, c, d, a];
 *   2. systems: perspective_matrix's eight rows in its order ((x, y, 1, 0, 0, 0, -x u, -y u | u) four times, then (0, 0, 0, x, y,
 *      1, -x v, -y v | v)), formed in double from the float32 points and the corners (0,0), (0,ph), (pw,ph), (pw,0); solved by
 *      Gaussian elimination, every product and difference rounded on its own: for column c = 0..7 the pivot is the FIRST row
 *      r >= c with the largest |a[r,c]| (a later row replaces it only if strictly larger); a pivot of exactly 0 ends the solve
 *      with h = 0 (the matrix is then 0,...,0,1); the pivot row is swapped into place; for r > c: m = a[r,c] / a[c,c], a[r,k] =
 *      a[r,k] - m a[c,k] for k > c, b[r] = b[r] - m b[c]; back substitution from row 7 up: s = b[r], s = s - a[r,k] x[k] for
 *      k = r+1..7 ascending, x[r] = s / a[r,r];
 *   3. inverses: adjugate_inverse's cofactor expressions in its order, each times 1.0 / det; zeros when det == 0.
 * No address depends on the key points except the pivot row (0..7): non-finite coordinates give some matrices, never a fault.
 * M 1 .. 2^20; image_height, patch_w, patch_h 1 .. 65536; x_pad 0 .. 65536. */
int pasta_part_geometry(const double* keypoints, int M, int image_height, int patch_w, int patch_h, int x_pad, int shin_fallback,
                        float* quads, double* fwd, double* back, double* fwd_inv, double* back_inv, float* m_inv, uint8_t* valid,
                        void* stream);

/* ------------------------------------------------------------------------- *
 * Per-sample preparation of the try-on data set (row f4; UvitonDatasetFull._load_raw_image / __getitem__,
 * training/dataset.py:515-568, 619-736, 929-993, and the loop's conversions, training_loop_wo_flow_fullbody.py:425-456),
 * which the reference runs on the host with OpenCV, pycocotools and skimage.  Each entry does a batch in one launch.
 * The unpadded canvas is H x W (256 x 192), padded by lp = (H - W) / 2 columns on the left into an H x H square.
 * This set passes thickness 2 and radius 2 to the stick figure and boxes (25, 16) to the palm mask.
 * Exact by construction: padding, label masks, gt_parsing, joint discs, the palm rule, the box dilation of a given fill,
 * the erase rule and the float conversions.  Restated (parity with the libraries UNPINNED):
 *   cv2.line(thickness=t)   -> every pixel centre within distance t / 2 of the segment (the capsule of half-width t / 2), in
 *                              integers 4 cross^2 <= t^2 len2 along the segment and 4 d^2 <= t^2 at its ends; for t = 5 cv2
 *                              draws a polygon of half-width t / 2 with round caps in 16.16 fixed point;
 *   pycocotools rleFrPoly   -> its algorithm: corners (int)(5 x + .5), boundary points along each edge, a run toggles at
 *                              ceil(clamp((v + .5) / 5 - .5, 0, h)) where the boundary steps from u = 5X + 2 to 5X + 3;
 *   cv2.resize(INTER_LINEAR, uint8) -> OpenCV's scalar fixed point: (float)((d + .5) * scale - .5), 11-bit coefficients
 *                              rint((1 - f) * 2048), rint(f * 2048); columns outside pinned, rows clamped;
 *                              (b0 * row0 + b1 * row1 + 2^21) >> 22.
 * ------------------------------------------------------------------------- */
/* The pose stick figure (draw_pose_from_cords, dataset.py:704-736) into out [N, H, H, 3] (zero padding): per pixel of the
 * canvas, the 19 limbs in order (limbs [N][19][5] int32 = x0, y0, x1, y1, drawn: int()-truncated key points, coordinates within
 * +-4096) as lines of `thickness`, then the 18 joints (joints [N][18][3] = x, y, drawn) as the discs
 * (r - y)^2 + (c - x)^2 < radius^2, clipped to the canvas -- skimage's ((r - y) / R)^2 + ((c - x) / R)^2 < 1 on every integer
 * offset for R = 2 and R = 5; the last hit wins, colour = kptcolors[index].  H <= 4096, W <= H, 1 <= thickness, radius <= 64. */
int pasta_pose_stickman_u8(const int32_t* limbs, const int32_t* joints, uint8_t* out, int N, int H, int W, int thickness, int radius,
                           void* stream);

/* The palm mask (get_palm, :682-702; get_hand_mask works on the padded S x S square) into out [N, S, S] (0 / 1): parsing
 * [N, S, W] uint8 (unpadded labels); quads [N][4][4][2] doubles = the corners of get_rectangle_mask (in its order, padded
 * coordinates within +-1e5) for the left upper arm, left forearm, right upper arm, right forearm; present [N][4]: 0 = the
 * segment is missing (an all-ones mask).  Each fill is dilated with a k_upper (upper arm) or k_lower (forearm) box; a k x k box
 * covers offsets -(k / 2) .. k - 1 - k / 2 (cv2's default anchor): -12..12 for 25, -8..7 for 16, -17..17 for 35, -10..9 for 20.
 * palm = hand & !upper & !forearm per side (hand = label 14 left, 15 right), the sides OR-ed.  S a multiple of 16,
 * 16 <= S <= 512; W <= S; 1 <= k <= S. */
int pasta_palm_mask_u8(const uint8_t* parsing, const double* quads, const uint8_t* present, uint8_t* out, int N, int S, int W,
                       int k_upper, int k_lower, void* stream);

/* :537-556 from image [N, H, W, 3], parsing [N, H, W] (unpadded) and palm [N, H, H]: retain = shoes(18, 19) + palm +
 * head(1, 2, 4, 13) and gt_parsing = upper(5, 6, 7) + 2 lower(9, 12) + 3 hands(14, 15) + 4 legs(16, 17) + 5 neck(10), [N, H, H];
 * upper_img / lower_img = mask * padded image (pad 255) and upper_mask / lower_mask = 255 * mask, [N, H, H, 3] (the inputs
 * of patch_pipeline.normalize_batch).  Mind the order: both images, then both masks.  The 512 x 320 training set names the
 * same labels and calls this entry too, its four garment pointers being the halves of the stacked [2N, H, H, 3] image and
 * mask tensors patch_pipeline.normalize_outfit_batch takes (upper garments, then lower). */
int pasta_tryon_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, uint8_t* retain, uint8_t* gt_parsing,
                         uint8_t* upper_img, uint8_t* lower_img, uint8_t* upper_mask, uint8_t* lower_mask, int N, int H, int W,
                         void* stream);

/* After the warps: the erase mask erase = (arm_masks[2] + arm_masks[3] + resize(erase_masks, H x H)) > 0 in uint8 arithmetic
 * (the reference's += on uint8 wraps), then the nine fp32 NCHW tensors of SyntheticFullBodyBatch.KEYS, in that order, through
 * outputs (a HOST array of 9 device pointers): real_img [N,3,H,H], style_input [N,c_upper+c_lower,ph,pw], retain [N,3,H,H],
 * pose [N,6,H,H], denorm_upper_input / denorm_lower_input [N,3,H,H], denorm_upper_mask / denorm_lower_mask [N,1,H,H],
 * gt_parsing [N,1,H,H].  x / 127.5 - 1 is evaluated as torch does on the GPU: x * (1 / 127.5f) - 1.
 * image [N,H,W,3]; stick, denorm_upper, denorm_lower [N,H,H,3]; retain_mask, gt_parsing [N,H,H]; norm_img [N,ph,pw,c_upper];
 * norm_img_lower [N,ph,pw,c_lower]; arm_masks [N,4,H,H]; erase_masks [N,mh_max,mw_max] with each sample's (h, w) in
 * erase_hw [N][2] int32 (1 <= h <= mh_max, 1 <= w <= mw_max). */
int pasta_tryon_assemble(const uint8_t* image, const uint8_t* stick, const uint8_t* retain_mask, const uint8_t* gt_parsing,
                         const uint8_t* norm_img, const uint8_t* norm_img_lower, const uint8_t* denorm_upper, const uint8_t* denorm_lower,
                         const uint8_t* arm_masks, const uint8_t* erase_masks, const int32_t* erase_hw, float* const* outputs, int N,
                         int H, int W, int ph, int pw, int c_upper, int c_lower, int mh_max, int mw_max, void* stream);

/* Mirrored people (this project's own rule; --mirror-people of train_wo_flow_fullbody.py, training/tryon_batch.py's
 * mirror_batch).  The reference's --mirror flips the PREPARED tuple, which is undefined for this data (the palm rule pairs label
 * 14 with joints 5-7 and label 15 with joints 2-4).  Here a raw sample with xflip = 1 is the sample as a mirror shows it, formed
 * BEFORE any preparation; everything downstream (stick figure, palm, masks, warps, erase rule, float conversions) is unchanged
 * and does not know about it:
 *   image     image'[y, x, :] = image[y, W-1-x, :];
 *   labels    parsing'[y, x] = lut[parsing[y, W-1-x]], lut a 256-byte table: the identity except 14 <-> 15 (arms), 16 <-> 17
 *             (legs) and 18 <-> 19 (shoes) (training.tryon_batch.mirror_lut);
 *   erase     erase'[y, x] = erase[y, w_n-1-x] inside the sample's own h_n x w_n (erase_hw[n]); the rest of the stacked tensor,
 *             the padding, is copied (collate writes 0 there);
 *   joints    on the host, in float64 (training.tryon_batch.mirror_keypoints): x' = (W-1) - x for every joint whatever its
 *             confidence, y and confidence unchanged, the rows exchanged for (2,5), (3,6), (4,7), (8,11), (9,12), (10,13),
 *             (14,15), (16,17); W is the unpadded width and the shift by the (symmetric) padding happens afterwards, as before.
 * A mirrored batch is NOT the flipped unmirrored batch and is not meant to be: int()-truncation of the joints and the 16 x 16
 * box's offsets -8..7 are not reflection-symmetric.
 * This entry is out of place and does a whole batch in one launch: image [N,H,W,3], parsing [N,H,W], erase_masks
 * [N,mh_max,mw_max] with erase_hw [N][2] int32, flip [N] uint8 and lut [256] on the device -> image_out, parsing_out, erase_out of
 * the inputs' shapes.  An item with flip[n] == 0 is copied through unchanged, the table not applied; the flags are read on the
 * device.  erase_masks and erase_out may both be null (erase_hw, mh_max and mw_max are then not read).  A size in erase_hw outside
 * the stacked tensor is read as the nearest one inside.  With W a multiple of 16 and 16-byte aligned tensors a thread moves 16
 * pixels with 16-byte loads and stores, the pixel order reversed in registers; any other width goes pixel by pixel.
 * Refused before any launch: a null image, parsing, flip, lut, image_out or parsing_out; an output equal to its input; N outside
 * 1..65535, H or W outside 1..16384; an erase pointer pair that is half null; with erase masks, a null erase_hw or mh_max or
 * mw_max outside 1..16384. */
int pasta_tryon_mirror_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* erase_masks, const int32_t* erase_hw,
                          const uint8_t* flip, const uint8_t* lut, uint8_t* image_out, uint8_t* parsing_out, uint8_t* erase_out, int N,
                          int H, int W, int mh_max, int mw_max, void* stream);

/* Jittered people (this project's own rule; --jitter-people of train_wo_flow_fullbody.py, training/tryon_batch.py's
 * jitter_batch).  A raw sample with jitter parameters is the sample as seen after a similarity map, formed BEFORE any preparation
 * and after mirroring; everything downstream (stick figure, palm, masks, warps, erase rule, float conversions) is unchanged and
 * does not know about it.  Canvas: the unpadded H x W image, centre c0 = (cx, cy) = ((W-1)/2, (H-1)/2).  Per item a scale s, an
 * angle theta (degrees, y pointing down) and a shift t = (tx, ty) in pixels: content at p moves to p' = c0 + s R(theta)(p - c0) + t,
 * R = [[cos, -sin], [sin, cos]].
 *   inverse   on the host, in float64 (training.tryon_batch.jitter_affine_q16): x = a x' + b y' + c, y = d x' + e y' + f with
 *             a = e = cos / s, b = sin / s, d = -sin / s, c = cx - (a (cx + tx) + b (cy + ty)), f = cy - (d (cx + tx) + e (cy + ty));
 *             sent as int64 Q16, rint(v * 65536): affine[n] = (A, B, C, D, E, F);
 *   image     for the output pixel (x', y'): X = A x' + B y' + C and Y = D x' + E y' + F in int64 (wrapping);
 *             Xq = (X + 1024) >> 11 (arithmetic: the coordinate in 1/32 pixel), ix = Xq >> 5, ax = Xq & 31, the same for y; the
 *             four taps (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1), each index clamped into the image (replicated border);
 *             v = (sum w tap + 512) >> 10 with w = (32-ax)(32-ay), ax (32-ay), (32-ax) ay, ax ay;
 *   colour    applied to v: colour[n] an int32 [3][4] Q8 matrix M,
 *             out_c = clamp((M[c][0] R + M[c][1] G + M[c][2] B + M[c][3] + 128) >> 8, 0, 255), the sum in int64
 *             (training.tryon_batch.jitter_colour_q8: M3 = k (q I + (1 - q) 1 L^T), L = (0.299, 0.587, 0.114), offset
 *             128 (1 - k) + beta, each rint(v * 256));
 *   labels    the nearest neighbour from the same X, Y: lx = clamp((X + 32768) >> 16, 0, W-1), ly likewise,
 *             parsing'[y', x'] = parsing[ly, lx]; no table, a similarity does not exchange sides;
 *   erase     not touched: the mask is file raw_idx % count of another project's random masks and belongs to the canvas;
 *   joints    on the host, in float64 (training.tryon_batch.jitter_keypoints): with m00 = m11 = s cos, m01 = -(s sin), m10 = s sin,
 *             ox = (cx + tx) - (m00 cx + m01 cy), oy = (cy + ty) - (m10 cx + m11 cy), a joint with confidence >= 0.1 becomes
 *             (m00 x + m01 y + ox, m10 x + m11 y + oy) with its confidence; a joint below 0.1 keeps its three numbers bit for bit;
 *             rows are not exchanged, a joint off the canvas stays as it is (downstream clamps), and the shift by the padding
 *             happens afterwards, as before.
 * The identity (A = E = 65536, the rest 0; M = 256 on the diagonal, the rest 0) returns its input byte for byte under these lines.
 * This entry is out of place and does a whole batch in one launch: image [N,H,W,3], parsing [N,H,W], affine [N][6] int64 and
 * colour [N][12] int32 on the device -> image_out, parsing_out of the inputs' shapes.  The numbers are read on the device; an item
 * whose eighteen numbers are the identity is copied.  A thread owns consecutive output pixels of a row: with W a multiple of 16
 * and 16-byte aligned tensors 16 of them, stored with 16-byte stores; any other width or address goes pixel by pixel.
 * Refused before any launch: a null pointer; an output equal to its input; N outside 1..65535, H or W outside 1..16384. */
int pasta_tryon_jitter_u8(const uint8_t* image, const uint8_t* parsing, const int64_t* affine, const int32_t* colour,
                          uint8_t* image_out, uint8_t* parsing_out, int N, int H, int W, void* stream);

/* Erase strokes (this project's own rule; --erase-masks strokes of train_wo_flow_fullbody.py, training/tryon_batch.py's
 * strokes_batch).  The erase mask of an item is drawn, not read from a file: random thick polylines with round caps and joins on
 * the padded S x S square (S = 256 or 512), anew at every visit, determined by the run's seed and the item's position in the
 * sampler's stream.  The mask belongs to the canvas: it covers the whole square, is formed after mirroring and jittering, is never
 * mirrored, and goes to the unchanged assemble entries as `erase_masks` with erase_hw = (S, S), a size the restated cv2.resize
 * passes unchanged (taps (d, 2048, 0)).
 *   uniforms  per item 169 numbers U on [0, 1): the raw outputs of np.random.PCG64(np.random.SeedSequence((seed, position, 1)))
 *             as (raw >> 11) * 2^-53 (training.tryon_batch.strokes_uniforms).  The third word keeps them independent of the jitter's
 *             (seed, position).  All 169 are drawn in this order whatever the specification says, so changing one strength leaves
 *             what the other parameters give unchanged.
 *   strokes   on the host, in float64, cos and sin the C library's (training.tryon_batch.strokes_segments), from a specification
 *             (strokes 1..8, vertices 1..8, length 0.01..0.5, width 0.01..0.25, turn 0..180 degrees):
 *             K = 1 + floor(U[0] strokes) strokes; stroke j uses the block b = 1 + 21 j: V = 1 + floor(U[b] vertices) segments,
 *             start x = U[b+1] S - 0.5, y = U[b+2] S - 0.5, half-width r = width S (1/3 + 2/3 U[b+3]) / 2, heading a = 2 pi U[b+4];
 *             for segment i < V: a += radians(turn) (2 U[b+5+2i] - 1), l = length S (1 + U[b+6+2i]) / 2, the segment runs from
 *             (x, y) to (x + l cos a, y + l sin a), which becomes the new (x, y).
 *   Q3        coordinates become int32 in 1/8 pixel, clip(rint(v * 8), -8192, 8191); the half-width clip(rint(r * 8), 8, 512).
 *             segments int32 [N, 64, 5] = (x0, y0, x1, y1, r), counts int32 [N] (0..64; a count outside is read as clamped).
 *   pixel     (px, py) of item n is 1 iff for one of its segments, with P = (8 px, 8 py), d = p1 - p0, v = P - p0, t = v.d,
 *             L = d.d:  t <= 0 ? v.v <= r r  :  t >= L ? |P - p1|^2 <= r r  :  cross(v, d)^2 <= r r L;  otherwise 0.
 *             Exact in integers: by the clamps and S <= 1024 every difference is below 2^14, so t, L, v.v and the cross product
 *             fit int32; only cross^2 (< 2^58) and r r L (< 2^47) need 64 bits.  p0 == p1 is a disc.
 * The value is 1, not 255: the reference's erase sum arm_a + arm_b + mask wraps in uint8, so with 255 a stroke that crosses an arm
 * part would punch an un-erased hole (255 + 1 = 0); 1 + 1 + 1 cannot wrap.
 * One launch for a batch: a 256-thread workgroup owns a 64 x 64 tile of one item, keeps the item's segments in LDS, its first wave
 * culls them against the tile (bounding box grown by r) into one 64-bit ballot, and every thread walks the set bits for 16
 * consecutive pixels of a row; with S a multiple of 16 and a 16-byte aligned `out` they leave in one 16-byte store, otherwise
 * byte by byte.  segments, counts and out [N, S, S] are on the device.  n == 0 is nothing to do.  Refused before any launch, outputs
 * untouched: a null pointer with n > 0; n outside 0..65535; S outside 1..1024.  Numbers outside the Q3 clamps give an unspecified
 * mask, never an access outside `out`. */
int pasta_erase_strokes_u8(const int32_t* segments, const int32_t* counts, uint8_t* out, int n, int S, void* stream);

/* People fitted to the canvas (this project's own rule; --fit-people pad | crop and --fit-filter bilinear | box of
 * train_wo_flow_fullbody.py, test.py, test_512.py and calc_metrics.py; training/tryon_batch.py's fit_batch, csrc/fit_people.hip).
 * A raw sample of any size h x w (h >= w) becomes the sample on the canvas H x W of its data set's class, (256, 192) or
 * (512, 320), BEFORE the mirroring, the jitter and any preparation; everything downstream is unchanged and does not know about it.
 *   rectangle in integers, with tall = (h W >= w H) and rhu(a / b) = (2 a + b) // (2 b) (training.tryon_batch.fit_rectangle):
 *             pad   shows the whole photograph: tall ? (Hc, Wc) = (H, rhu(w H / h)) : (Wc, Hc) = (W, rhu(h W / w));
 *                   oy = (H - Hc) // 2, ox = (W - Wc) // 2; outside the rectangle the photograph is 255 and the label 0;
 *             crop  fills the canvas with a centre crop: tall ? (Wc, Hc) = (W, rhu(h W / w)) : (Hc, Wc) = (H, rhu(w H / h));
 *                   oy = -((Hc - H) // 2), ox = -((Wc - W) // 2); only the visible window is computed;
 *             refused by the data set, with the file's name: h > 8 Hc, w > 8 Wc, Hc > 4 h or Wc > 4 w.
 *   taps      per axis, from length n_in to n_out, PIL's 8-bit rule (Pillow's Resample.c, precompute_coeffs / normalize_coeffs_8bpc)
 *             in float64, every operation rounded on its own (training.tryon_batch.fit_taps): scale = n_in / n_out,
 *             fs = max(scale, 1), support = S0 fs (S0 = 0.5 box, 1 bilinear), ss = 1 / fs; for output position xx:
 *             center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), cnt = min(int(center + support + 0.5), n_in) - xmin
 *             (int truncates); wgt[x] = f(((x + xmin) - center + 0.5) ss) for x < cnt, f box: 1 on -0.5 < t <= 0.5, f bilinear:
 *             1 - |t| on |t| < 1, else 0; ww the sum of wgt in order, wgt[x] /= ww when ww != 0; k[x] = int(0.5 + wgt[x] 2^22).
 *             Equal lengths: the single tap 2^22 (PIL skips such a pass; the tap returns the byte).
 *   image     the Hc x Wc image PIL.Image.resize((Wc, Hc), BOX | BILINEAR) returns, byte for byte, placed at (oy, ox):
 *             out[xx] = min(((2^21 + sum_x src[xmin + x] k[x]) >> 22), 255) per channel, the horizontal pass first into uint8
 *             [h, Wc] -- that rounded intermediate is part of the result -- then the vertical pass over it.
 *   labels    a weighted mode over the BOX taps ky, kx of the same two axes, whatever the photograph's filter: the weight of label
 *             L at fitted (r, c) is the int64 sum of ky[r][i] kx[c][j] over the taps with src[ymin + i][xmin + j] == L; the label of
 *             greatest weight wins; among tied labels the label of source pixel (((2 r + 1) h) // (2 Hc), ((2 c + 1) w) // (2 Wc))
 *             when it is one of them, else the smallest.
 *   erase     not touched: the assemble entries resize a mask from its own size.
 *   joints    on the host, in float64 (training.tryon_batch.fit_keypoints): a joint with confidence >= 0.1 becomes
 *             (x sx + ((0.5 sx - 0.5) + ox), y sy + ((0.5 sy - 0.5) + oy)) with sx = Wc / w, sy = Hc / h; one below 0.1 keeps its bits.
 * An item already at the canvas size is an identity in all three.
 *   plan      one int32 array for the batch, plan_words long (training.tryon_batch.fit_plan): N records of 16 words
 *             (h, w, Hc, Wc, oy, ox, the word offsets in the plan of the photograph's x and y tables and of the label map's x and y
 *             tables, the low 31 bits and the rest of the item's first PIXEL in the packed buffers, 0 ...), then the tables, each
 *             distinct (n_in, n_out, filter) once: (n_out, ksize) and n_out rows (xmin, cnt, k[ksize]), ksize <= 17.
 * One entry, out of place, two launches for a whole batch: images [3 pixels] and labels [pixels] are the packed bytes of the N
 * items (item n at byte 3 off_n and off_n), plan is on the device -> image_out [N,H,W,3], parsing_out [N,H,W], every byte written.
 * The photographs: a 256-thread workgroup owns a 16 x 64 tile of one item's canvas, runs the horizontal pass for the at most 144
 * source rows the tile needs into LDS (they never reach HBM), then the vertical pass from LDS; with W a multiple of 16 and a 16-byte
 * aligned image_out the tile leaves in 16-byte stores along the rows, otherwise byte by byte.  The label maps: a thread owns 16
 * pixels of a row (one 16-byte store) or one; the labels present in a footprint are collected in a 256-bit set and the weights
 * summed per present label.  Every number of the plan is read on the device and every index is held inside its buffer whatever the
 * plan says; an item whose record, tables or row span are not what the rule above makes within the limits is written as padding.
 * Refused before any launch: a null pointer; an output equal to its input; N outside 1..65535, H or W outside 1..16384; pixels < 1;
 * plan_words below 16 N or above 2^31 - 1. */
int pasta_fit_people_u8(const uint8_t* images, const uint8_t* labels, int64_t pixels, const int32_t* plan, int64_t plan_words,
                        uint8_t* image_out, uint8_t* parsing_out, int N, int H, int W, void* stream);

/* ------------------------------------------------------------------------- *
 * Per-batch preparation of the try-on TEST pairs (row f4; UvitonDatasetV19_test._load_raw_image / normalize / __getitem__,
 * training/dataset.py:1085-1525, and test.py:104-150).  Same canvas, restated primitives and exactness as the entries
 * above.  Where the test set differs from the training preparation:
 *   1. two people: parts 0-5 are warped from the clothes DONOR's upper garment, stick figure and mask with the donor's key
 *      points, parts 6-9 from the PERSON's lower garment, stick figure and mask with the person's (:1470-1478);
 *   2. the warp-back uses the person's M_inv for all ten parts; an upper part is composited wherever the person's part
 *      exists, its patch being zeros where the donor's does not (:1481-1492);
 *   3. the warped-back mask of parts 0-5 is eroded (cv2.erode, 5 x 5, default border) before the == 255 test (:1460, :1484);
 *   4. the forearm box of the palm rule is 15 x 15 (:1252; training: 16 x 16), the upper arm 25 x 25 in both;
 *   5. the lower garment is labels 6, 9, 12 of the person (:1113), the upper garment labels 5, 6, 7 of the donor (:1133);
 *   6. key points are shifted by the padding in float64 before get_crop's float32 conversion (:1100, :1129; host side);
 * and, on the host too, get_crop's knee-without-ankle fall-back, which the training set's get_crop has commented out (:1355).
 * This set passes thickness 2 and radius 2 to pasta_pose_stickman_u8, boxes (25, 15) to pasta_palm_mask_u8 and
 * six_is_lower = 1 to the label masks below.
 * ------------------------------------------------------------------------- */
/* The label masks of a person in two garments (:1105-1141, :1631-1690) from the person's image [N, H, W, 3], parsing [N, H, W]
 * (unpadded) and palm [N, H, H] and a source per garment, (upper_image, upper_parsing) and (lower_image, lower_parsing), shaped
 * like the person's; they may be the person's own pointers.  retain_img = the person's padded image * (shoes(18, 19) + palm +
 * head(1, 2, 4, 13)), always the person's; upper_img / upper_mask = labels 5, 6, 7 (image, 255) of the upper source;
 * lower_img / lower_mask = labels 9, 12 of the lower source, and label 6 as well where six_is_lower is 1 (0 or 1; anything else
 * is refused).  Outputs [N, H, H, 3], padding 255 in the images before the masks are applied, 0 in the labels.  The reference's
 * 256 pair is the sources (donor, person). */
int pasta_tryon_outfit_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, const uint8_t* upper_image,
                                const uint8_t* upper_parsing, const uint8_t* lower_image, const uint8_t* lower_parsing,
                                uint8_t* retain_img, uint8_t* upper_img, uint8_t* upper_mask, uint8_t* lower_img, uint8_t* lower_mask,
                                int N, int H, int W, int six_is_lower, void* stream);

/* pasta_patch_composite_u8 with the warped-back mask eroded by a (2 r + 1)^2 box before the == 255 test: a pixel takes part k
 * where channel 0 of the warped-back mask is 255 at every in-image pixel within +-r (pixels outside the image do not erode,
 * cv2's default border).  part_mask (optional) receives the eroded 0 / 1 mask of every part.  r = 0 gives
 * pasta_patch_composite_u8's bits and takes no barrier.  radii (optional, uint8 [N] on the device):
 *   null      every sample is eroded by r = radius, 0 <= radius <= 8;
 *   non-null  sample n is eroded by r = radii[n], all samples in the one launch (a workgroup works on one sample, so r is
 *             uniform across it), and radius is not read.  The values live on the device, so the entry cannot refuse one: the
 *             caller checks them on the host (patch_pipeline.composite raises), and the kernel reads a value above 8 as 8, the
 *             halo its LDS tiles hold. */
int pasta_patch_composite_eroded_u8(const uint8_t* patches, const uint8_t* masks, const double* minv, const uint8_t* valid,
                                    uint8_t* out, uint8_t* part_mask, int N, int P, int ph, int pw, int H, int W, int radius,
                                    const uint8_t* radii, void* stream);

/* __getitem__ and the scripts' conversions (:1502-1525 and test.py:104-117; :2196-2214 and test_512.py:115-131): fp32 NCHW
 * tensors through outputs (a HOST array of 10 device pointers) in this order: image, clothes [N,3,H,H] (the padded person and
 * upper_donor_image, padding 255), retain [N,3,H,H] = x / 127.5 - 1 of retain_img (test.py's form; test_512.py's
 * image * mask - (1 - mask) with the 0 / 1 retain mask equals it bit for bit, the label groups being disjoint), pose [N,6,H,H] =
 * stick || retain, style_input [N,3(P+P_lower),ph,pw] = the P patches (channel 3k + c of part k) || the P_lower patches_lower,
 * denorm_upper_input / denorm_lower_input [N,3,H,H], denorm_upper_mask / denorm_lower_mask [N,1,H,H] = channel sum > 0 (no
 * wrap), clothes_lower [N,3,H,H] = the padded lower_donor_image.  x / 127.5 - 1 as torch evaluates it on the GPU:
 * x * (1 / 127.5f) - 1.  image, upper_donor_image, lower_donor_image [N,H,W,3]; retain_img, stick, denorm_upper, denorm_lower
 * [N,H,H,3]; patches [N,P,ph,pw,3], patches_lower [N,P_lower,ph,pw,3] uint8.
 * Outputs 0, 1 and 9 may be null: a null output is not written and its photograph is not read (it may be null too); a non-null
 * one needs its photograph.  Outputs 0 and 1 are null together or not at all, and output 9 needs them.  Outputs 2..8 are
 * required.  The seven tensors G takes at 256 x 192 are outputs 2..8 with the stick-figure patches as patches_lower; test_512.py
 * takes outputs 0..8, an outfit all ten. */
int pasta_tryon_outfit_assemble(const uint8_t* image, const uint8_t* upper_donor_image, const uint8_t* lower_donor_image,
                                const uint8_t* retain_img, const uint8_t* stick, const uint8_t* patches, const uint8_t* patches_lower,
                                const uint8_t* denorm_upper, const uint8_t* denorm_lower, float* const* outputs, int N, int H, int W,
                                int P, int P_lower, int ph, int pw, void* stream);

/* test.py:133-137: images [N, 3, H, Wt] fp32 -> out [N, H, W, 3] uint8 of columns c0 .. c0 + W - 1: (x + 1.0f) * 127.5f with
 * each operation rounded on its own, clipped to [0, 255], truncated.  A NaN becomes 0 (numpy leaves that conversion
 * undefined). */
int pasta_images_to_u8(const float* images, uint8_t* out, int N, int H, int Wt, int c0, int W, void* stream);

/* The photograph's kept parts pasted into the generated bytes (this project's own rule; --kept-parts photo of test.py and
 * test_512.py, training/tryon_pairs.py's images_keep_to_u8), in the launch that makes the bytes, so that they are never
 * written uncomposited.  Per image: g = the bytes pasta_images_to_u8 writes for columns c0 .. c0 + W - 1 of images
 * [N, 3, H, Wt] fp32 (a NaN is 0 here too); p = photo [N, H, W, 3] uint8, the person's photograph; k = (keep [N, H, W] uint8
 * != 0), the kept flag; r = radius, 0..8, the feather; K = (2r + 1)^2.  For pixel (y, x):
 *   s = how many of the K positions (y + dy, x + dx), |dy|, |dx| <= r, lie outside the image or have k = 1.  A position
 *       outside the image counts as kept, as the border of csrc/patch_erode.h's erosion does not erode: hair that touches the
 *       top edge is not faded;
 *   a = k(y, x) ? s : 0.  Nothing of the photograph is taken from outside the kept region, so the old garment at the neck
 *       cannot leak in;
 *   out_c = (g_c * (K - a) + p_c * a + K / 2) / K per channel, in integers with a floor division.
 * So a = K, every pixel whose whole window is kept, gives the photograph's byte; a = 0, every pixel outside the region, gives
 * the generated byte; r = 0 is the hard paste k ? p : g; in between the weight rises linearly with the kept share of the
 * window, and every byte lies between g_c and p_c.  Refused before any launch: a null pointer, the shape and crop conditions
 * of pasta_images_to_u8, a radius outside 0..8. */
int pasta_images_keep_to_u8(const float* images, const uint8_t* photo, const uint8_t* keep, uint8_t* out, int N, int H, int Wt, int c0,
                            int W, int radius, void* stream);

/* Where the photograph may be pasted (this project's own rule; --kept-parts / --background / --kept-garments photo of test.py and
 * test_512.py, training/tryon_pairs.py's photo_paste_mask): the 0 / 1 region that goes to pasta_images_keep_to_u8 as `keep`.  A
 * pixel of the photograph is pasted only where the photograph's label map AND the generator's own statement of what it drew
 * there agree.  Per item n: L = parsing [N, H, W] uint8, the person's labels; palm [N, H, Ht] uint8 or null, the palm mask on
 * the padded rows; c0 = (Ht - W) / 2; rule [N, 256] uint8: rule[n][l] is a 4-bit set of the statements under which label l of
 * item n's photograph may be pasted (256 rows, so that any byte a label file holds indexes it without a check).
 *   The generator's statement s(y, x) in {0 other, 1 upper garment, 2 lower garment, 3 skin}, read at column c0 + x of its heads:
 *     head_planes = 6  heads_a fp32 [N, 6, Ht, Ht], the parsing logits (GeneratorFull), heads_b null: c = argmax over the six
 *                      planes exactly as torch.argmax(dim=1) -- the first NaN if there is one, else the first of the largest --
 *                      and s = 0, 1, 2, 3, 3, 3 for c = 0..5 (gt_parsing's classes: 3 hands, 4 legs, 5 neck);
 *     head_planes = 1  heads_a = u, heads_b = l, fp32 [N, 1, Ht, Ht] each, the sigmoid heads (GeneratorV18): s = 1 if u > 0.5,
 *                      else 2 if l > 0.5, else 0, in IEEE comparisons, so a NaN is "other";
 *     head_planes = 0  both null: s = 0 everywhere.
 *   out [N, H, W] uint8: m(y, x) = (palm(y, c0 + x) != 0) || ((rule[n][L(y, x)] >> s(y, x)) & 1); a null palm has no palm term.
 * The host fills the table (training.tryon_pairs.paste_rules): kept parts 0b1111 at labels 1, 2, 4, 13, 18, 19 (with the palm
 * pointer); the background 0b0001 at label 0 (pasted only where the generator claims neither garment nor skin); the person's
 * own upper garment 0b0010 at the upper labels of an item whose outfit keeps it, the own lower garment 0b0100 at the lower
 * labels likewise -- the label sets of pasta_tryon_outfit_masks_u8 for that size; at 256 x 192 label 6 is in both and the bits
 * OR.  One launch, every pixel independent.  Refused before any launch: a null parsing, rule or out; head_planes outside
 * {0, 1, 6}; a heads pointer that disagrees with head_planes; N outside 1..65535, H or Ht outside 1..4096, H > Ht, W < 1,
 * W > Ht. */
int pasta_photo_paste_mask_u8(const uint8_t* parsing, const uint8_t* palm, const uint8_t* rule, const float* heads_a, const float* heads_b,
                              int head_planes, uint8_t* out, int N, int H, int W, int Ht, void* stream);

/* An OUTFIT at 256 x 192 (this project's own; training/tryon_pairs.py, TryOnPairOutfitBatchBuilder): (P, U, L), the person P in
 * the upper garment of U and the lower garment of L, either of whom may be P.  The pair rules above with a source per garment:
 *   1. retain_img, the palm mask (boxes 25 and 15), the stick figure in `pose` and every M_inv are P's;
 *   2. the upper garment is labels 5, 6, 7 of U; parts 0-5 of the garment, of U's stick figure and of the mask are warped
 *      forward with U's matrices;
 *   3. the lower garment is labels 6, 9, 12 of L; parts 6-9 of the garment, of L's stick figure and of the mask are warped
 *      forward with L's matrices;
 *   4. key points shifted by the padding in float64, x_pad = 0, the knee-without-ankle fall-back, for all three people;
 *   5. all ten parts go back with P's M_inv; a missing forward matrix gives zeros, a part whose M_inv is missing is skipped;
 *   6. parts 0-5 go into denorm_upper through the eroded composite (5 x 5) whoever U is, as the reference erodes them;
 *   7. parts 6-9 go into denorm_lower through the plain composite when L is P (the reference's case, bit for bit) and through
 *      the eroded composite (5 x 5) when L is somebody else: a mask warped onto another body has a fringe, the reference's
 *      reason for rule 6.  The choice is per sample (pasta_patch_composite_eroded_u8 with radii of 0 or 2).
 * The change regions are three outfits: upper body (P, D, P), which is the pair rules above; lower body (P, P, D); full body
 * (P, D, D). */

/* ------------------------------------------------------------------------- *
 * Per-batch preparation of the 512 x 320 try-on pairs with a change region (row f4; UvitonDatasetFull_512_test,
 * training/dataset.py:1528-2214, and test_512.py:115-131).  The unpadded canvas is 512 x 320, padded by 96 columns into a
 * 512 x 512 square.  Same restated primitives and exactness as the entries above.  Where this set differs from the 256 test
 * pairs:
 *   1. the stick figure has lines of thickness 5 and discs of radius 5 (:1851, :1861); only the person's is used;
 *   2. the palm rule works on the 512 square with a 35 x 35 upper-arm and a 20 x 20 forearm box (:1785-1796);
 *   3. the lower garment is labels 9, 12 (:1639, :1669; not 6), the upper garment labels 5, 6, 7;
 *   4. the change region picks whose garment is worn (:1679-1690): full body = both from the donor, upper body = the donor's
 *      upper and the person's own lower garment, lower body = the person's own upper and the donor's lower garment; a garment
 *      is warped forward with the matrices of the person it was taken from, and back with the person's M_inv;
 *   5. all ten parts of the upper garment go into norm_img and denorm_upper, parts 0, 6, 7, 8, 9 of the lower garment into
 *      norm_img_lower and denorm_lower; every warped-back mask is eroded 5 x 5, the legs' included (:2016, :2031);
 *   6. there are no stick-figure patches: style_input is norm_img || norm_img_lower, 45 channels;
 *   7. on the host, get_crop has no knee-without-ankle fall-back (:1893-1900) and its thigh fall-back ends at row 511.
 * This set passes thickness 5 and radius 5 to pasta_pose_stickman_u8, S = 512 and boxes (35, 20) to pasta_palm_mask_u8,
 * six_is_lower = 0 to pasta_tryon_outfit_masks_u8 and radius 2 to pasta_patch_composite_eroded_u8 for both garments.  The
 * sources of pasta_tryon_outfit_masks_u8 by change region: full body (donor, donor), upper body (donor, person), lower body
 * (person, donor); pasta_tryon_outfit_assemble takes the donor's photograph as upper_donor_image and fills outputs 0..8.
 * An OUTFIT at 512 x 320 (this project's own; training/tryon_regions.py, TryOnOutfitBatchBuilder): the person wears the upper
 * garment of one donor and the lower garment of another, either of whom may be the person; the two sources are the two
 * donors', and all ten outputs are filled.
 * ------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------- *
 * Per-batch preparation of the 512 x 320 try-on TRAINING samples (training/tryon_regions.py, FullBodyRegionBatchBuilder).
 * The reference ships no 512 training set: the rules are this project's own, and one rule governs them -- the generator is
 * trained on exactly the inputs test_512.py will later feed it.  A sample is the entries' above full-body preparation of the
 * pair (person, person), with the 256 training set's three extras on top:
 *   1. stick figure of thickness 5 and radius 5 from the unshifted key points, palm boxes 35 and 20 on the 512 square
 *      (pasta_pose_stickman_u8, pasta_palm_mask_u8);
 *   2. the upper garment is labels 5, 6, 7 and the lower garment labels 9, 12, both the person's own;
 *   3. key points are shifted by the padding in float64 (host side), get_crop has no knee-without-ankle fall-back;
 *   4. all ten parts of the upper garment, parts 0, 6, 7, 8, 9 of the lower one; every warped-back mask is eroded 5 x 5
 *      (pasta_patch_composite_eroded_u8); style_input has 45 channels;
 *   5. real_img is the padded photograph (padding 255) and gt_parsing the 256 training set's label rule;
 *   6. erase = (arm[2] + arm[3] + resize(erase mask, 512 x 512)) > 0 in uint8 wrapping arithmetic, arm[k] the ERODED 0 / 1
 *      mask of arm part ARM_PARTS[k] = 2, 3, 4, 5 from the upper composite (the fixed pick the reference's random.seed(1)
 *      makes at 256), resize the restated cv2.resize of pasta_tryon_assemble;
 *   7. the two denormalised inputs are zeroed where erase is 1 before x / 127.5 - 1, their masks are the channel sum > 0 of
 *      the erased image.
 * Retain mask, gt_parsing and both garments (rules 2 and 5) are pasta_tryon_masks_u8's: the two training sets name the same
 * labels.
 * ------------------------------------------------------------------------- */
/* Rules 5-7 and the float conversions: the nine fp32 NCHW tensors of FullBodyBatch.KEYS, in that order, through outputs (a
 * HOST array of 9 device pointers), shaped as pasta_tryon_assemble's with style_input [N,3(P+P_lower),ph,pw] = the P
 * upper-garment patches (channel 3k + c of part k) || the P_lower lower-garment patches, as pasta_tryon_outfit_assemble
 * forms it.  image [N,H,W,3]; stick, denorm_upper, denorm_lower [N,H,H,3]; retain_mask, gt_parsing [N,H,H];
 * patches [N,P,ph,pw,3], patches_lower [N,P_lower,ph,pw,3]; part_masks [N,P,H,H]: the eroded 0 / 1 part masks of the upper
 * composite, of which planes arm_a and arm_b (4 and 5: arm[2] and arm[3]) enter the erase mask; erase_masks
 * [N,mh_max,mw_max] with each sample's (h, w) in erase_hw [N][2] int32.  Every pixel is the body pasta_tryon_assemble runs.
 * pw a multiple of 4 (four patch pixels per thread). */
int pasta_tryon_train_region_assemble(const uint8_t* image, const uint8_t* stick, const uint8_t* retain_mask, const uint8_t* gt_parsing,
                                      const uint8_t* patches, const uint8_t* patches_lower, const uint8_t* denorm_upper,
                                      const uint8_t* denorm_lower, const uint8_t* part_masks, int arm_a, int arm_b,
                                      const uint8_t* erase_masks, const int32_t* erase_hw, float* const* outputs, int N, int H, int W,
                                      int P, int P_lower, int ph, int pw, int mh_max, int mw_max, void* stream);

/* ------------------------------------------------------------------------- *
 * The training run's snapshot image (setup_snapshot_image_grid, denorm_clothes, combine_parts and save_image_grid,
 * training/training_loop_wo_flow_fullbody.py:36-209): a gnum x gnum mix-and-match grid, cell = row * gnum + col, row the
 * person (pose, retain, M_inv) and col the clothes donor; gap = gnum / 3: rows < gap swap the trousers, rows < 2 gap the
 * whole outfit, the others the top.  The reference warps and erodes on the host, about ten thousand OpenCV calls, and keeps
 * fp32 tensors of all cells on the device; here the resident state is uint8 and the fp32 tensors exist per minibatch.  Same
 * restated warp as the entries above (parity with OpenCV UNPINNED).
 * ------------------------------------------------------------------------- */
/* denorm_clothes (:59-107) for all cells of one garment in one launch: pasta_patch_composite_eroded_u8 whose part k of cell i
 * reads patch and mask index[i][k] of a pool [T, ph, pw, 3] (int32; an index outside 0 .. T - 1 skips the part, as valid = 0
 * does), warped with minv [cells][P][9] (doubles, dst -> src) into out [cells, H, W, 3]; parts composite in index order.
 * With index[i][k] = i * P + k it is pasta_patch_composite_eroded_u8 bit for bit.  cells <= 65535, 0 <= radius <= 8. */
int pasta_grid_composite_eroded_u8(const uint8_t* pool, const uint8_t* mask_pool, const int32_t* index, const double* minv,
                                   const uint8_t* valid, uint8_t* out, int cells, int P, int T, int ph, int pw, int H, int W,
                                   int radius, void* stream);

/* The fp32 NCHW tensors G_ema takes (:121-175, :580-583) for cells lo .. lo + n - 1, through outputs (a HOST array of 7 device
 * pointers) in this order: denorm_upper_input / denorm_lower_input [n,3,H,H] = x * (1 / 127.5f) - 1 of the cell's images,
 * denorm_upper_mask / denorm_lower_mask [n,1,H,H] = channel sum > 0 (no uint8 wrap, :104-105), style_input
 * [n,c_upper+c_lower,ph,pw] by combine_parts' rule (:36-56: upper channels of person row when row < gap, else of col; lower
 * channels of col when row < 2 gap, else of row), pose [n,6,H,H] = stick || retain and retain [n,3,H,H] =
 * retain_mask * image - (1 - retain_mask) of person row (:160-175).  denorm_upper, denorm_lower [gnum^2,H,H,3]; image (padded),
 * stick [gnum,H,H,3]; retain_mask [gnum,H,H]; norm_img [gnum,ph,pw,c_upper]; norm_img_lower [gnum,ph,pw,c_lower]; all uint8.
 * H and pw multiples of 4 (four pixels per thread), gnum <= 255. */
int pasta_grid_assemble(const uint8_t* denorm_upper, const uint8_t* denorm_lower, const uint8_t* image, const uint8_t* stick,
                        const uint8_t* retain_mask, const uint8_t* norm_img, const uint8_t* norm_img_lower, float* const* outputs,
                        int lo, int n, int gnum, int H, int ph, int pw, int c_upper, int c_lower, void* stream);

/* Additive at ABI 22.  pasta_grid_assemble's garment tensors for the unpaired pass of TRAINING (training/swap_outfits.py; DESIGN
 * 8k): sample i of a batch of n wears the upper patches of person upper_src[i] and the lower patches of person lower_src[i]
 * (int32, DEVICE memory) of T people.  outputs: a HOST array of 5 device pointers, swap_denorm_upper_input /
 * swap_denorm_lower_input [n,3,H,H] = x * (1 / 127.5f) - 1 of denorm_upper / denorm_lower [n,H,H,3] (sample i's own images, made
 * by pasta_grid_composite_eroded_u8 with the same tables), swap_denorm_upper_mask / swap_denorm_lower_mask [n,1,H,H] = channel
 * sum > 0, swap_style_input [n,c_upper+c_lower,ph,pw]: the channels of norm_img [T,ph,pw,c_upper] of the upper source followed by
 * those of norm_img_lower [T,ph,pw,c_lower] of the lower source.  The same device arithmetic as pasta_grid_assemble: for the
 * sources its cell has, the five tensors are that entry's bit for bit.  A source outside 0 .. T - 1 reads nothing (its style
 * channels are those of zero bytes).  H and pw multiples of 4, n <= 65535. */
int pasta_swap_assemble(const uint8_t* denorm_upper, const uint8_t* denorm_lower, const uint8_t* norm_img, const uint8_t* norm_img_lower,
                        const int32_t* upper_src, const int32_t* lower_src, float* const* outputs, int n, int T, int H, int ph, int pw,
                        int c_upper, int c_lower, void* stream);

/* save_image_grid (:182-203): images [n, C, H, W] fp32 (C = 1 or 3) become tiles first .. first + n - 1 of a uint8 canvas
 * [canvas_h, canvas_w, C]; tile t sits at tile row t / gw + oy and tile column t % gw + ox (the grid proper: gw = gnum,
 * ox = oy = 1; the side column: gw = 1, ox = 0, oy = 1; the top row: ox = 1, oy = 0, its corner tile a tile of zeros at
 * ox = oy = 0).  Per element rint((x - lo) * scale) in fp32 as numpy evaluates :184-186 with scale = 255 / (hi - lo): one
 * subtraction and one multiplication, each rounded on its own, round half to even, clipped to [0, 255].  A NaN becomes 0
 * (numpy leaves that conversion undefined).  W a multiple of 4; the tiles must lie inside the canvas. */
int pasta_image_grid_tile_u8(const float* images, uint8_t* canvas, int n, int C, int H, int W, int first, int gw, int ox, int oy,
                             int canvas_h, int canvas_w, float lo, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * Statistics of the paired-reconstruction metric (metrics/reconstruction.py; csrc/recon_metrics.hip): G_ema's image of a
 * person against that person's photograph, and its parsing against the label map.  Only the content columns
 * c0 .. c0 + W - 1 of the padded square are scored.
 * ------------------------------------------------------------------------- */
/* images [N, 3, H, Wt] fp32, each value first turned into the byte pasta_images_to_u8 writes; photos [N, H, W, 3] uint8.
 * sums [N, 3] int64 = sum |d|, sum d^2 over the H W 3 bytes (exact) and the SSIM window count 3 (H - 10) (W - 10);
 * ssim [N] fp64 = the sum over those windows of SSIM (Wang et al. 2004) per RGB channel: 11 x 11 Gaussian window of sigma 1.5
 * normalised to 1, valid positions, weighted population moments, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 * (2 mx my + C1) (2 sxy + C2) / ((mx^2 + my^2 + C1) (sxx + syy + C2)), evaluated in fp32 on bytes centred at 127.5.  One fp64
 * partial per workgroup, reduced in a fixed order: two launches on the same input give the same bits.  workspace: device
 * memory of pasta_recon_image_stats_workspace(N, H, W) bytes (0 for a shape that is refused).  H >= 11 and W >= 11. */
int64_t pasta_recon_image_stats_workspace(int N, int H, int W);
int pasta_recon_image_stats(const float* images, const uint8_t* photos, int64_t* sums, double* ssim, void* workspace,
                            int64_t workspace_bytes, int N, int H, int Wt, int c0, int W, void* stream);

/* pasta_recon_image_stats restricted to a region (metrics/tryon_fidelity.py scores what an unpaired try-on must keep: the body
 * parts that come in through `retain` against the photograph, the warped garment patches against themselves).  images
 * [N, 3, H, Wt] fp32 as above, content columns c0 .. c0 + W - 1; ref [N, H, Wr, 3] uint8, content columns from r0 (a photograph:
 * Wr = W, r0 = 0; a padded stage: Wr = H, r0 = c0); mask [N, H, Wm] uint8, content columns from m0, nonzero = the pixel is in the
 * region.  sums [N, 4] int64 = sum |d| and sum d^2 over the three bytes of every region pixel (exact), the SSIM windows -- one
 * per RGB channel and valid 11 x 11 position whose 121 pixels are ALL in the region -- and the bytes, 3 x region pixels;
 * ssim [N] fp64 = the sum of SSIM over those windows, the same Gaussian, constants, centring and fp32 evaluation.  Same tiles,
 * same device code and same summation order as pasta_recon_image_stats: with a mask of ones and ref a photograph, sums[:, :3]
 * and ssim are that entry's bit for bit.  An empty region gives four zeros and 0.0; nothing is divided by a count on the
 * device.  One partial per workgroup and a fixed-order second launch: two calls on the same input give the same bits.
 * workspace: pasta_region_image_stats_workspace(N, H, W) bytes (0 for a shape that is refused).  H >= 11, W >= 11, and every
 * column range inside its tensor: anything else is refused before a launch. */
int64_t pasta_region_image_stats_workspace(int N, int H, int W);
int pasta_region_image_stats(const float* images, const uint8_t* ref, const uint8_t* mask, int64_t* sums, double* ssim,
                             void* workspace, int64_t workspace_bytes, int N, int H, int Wt, int c0, int Wr, int r0, int Wm, int m0,
                             int W, void* stream);

/* logits [N, C, H, Wt] and labels [N, 1, H, Wt] fp32, C <= 32: matrix [C, C] int64 (row = label, column = prediction) is
 * ADDED to, the caller zeroes it once.  Prediction: the arg-max over the channels, the lowest index on ties; a NaN never wins,
 * all NaN predicts class 0.  The label is truncated as .long() does; one outside 0 .. C - 1 (or a NaN) skips the pixel, as
 * ignore_index does in the loss. */
int pasta_parsing_confusion(const float* logits, const float* labels, int64_t* matrix, int N, int C, int H, int Wt, int c0, int W,
                            void* stream);

/* ------------------------------------------------------------------------- *
 * The SSIM term of the generator's loss (torch_utils/ops/ssim_loss.py; csrc/ssim_loss.hip): the structural figure
 * the reconstruction metric reports, in a form that can be trained on.
 * x (generated) and y (photograph): [N, 3, H, Wt] fp32 as the networks produce them -- values v of nominally [-1, 1], taken as
 * intensities v + 1 of dynamic range L = 2, NOT clipped and NOT quantised; only the content columns c0 .. c0 + W - 1 are read.
 * Per channel and per valid position of the 11 x 11 Gaussian window of pasta_recon_image_stats (sigma 1.5, the same fp32
 * weights w), (H - 10) (W - 10) of them:
 *   mx = E[x] + 1, my = E[y] + 1, sxx = E[xx] - E[x]^2, syy = E[yy] - E[y]^2, sxy = E[xy] - E[x] E[y],
 *   a1 = 2 mx my + C1, a2 = 2 sxy + C2, b1 = mx^2 + my^2 + C1, b2 = sxx + syy + C2, C1 = (0.01 L)^2 = 4e-4, C2 = (0.03 L)^2 = 3.6e-3,
 *   S = a1 a2 / (b1 b2),      loss = 1 - (sum of S) / M,  M = N 3 (H - 10) (W - 10).
 * The intensities are the bytes the metric scores up to a scale, b = (v + 1) * 127.5, and SSIM does not change under a scaling
 * when the constants scale with L^2 (under a shift it does, hence the means of v + 1 and not of v): on images that lie on the
 * byte grid, 1 - loss is the mean of pasta_recon_image_stats' ssim / windows.  Anywhere else the two differ: the metric scores
 * clipped bytes.
 * Gradient with respect to x only.  Per position: dS/dmx = 2 my a2 / (b1 b2) - 2 mx S / b1, B = dS/dsxx = -S / b2,
 * C = dS/dsxy = 2 a1 / (b1 b2), A = dS/dmx - 2 mx B - my C; per pixel q
 *   dloss/dx[q] = -(1 / M) ((w (*) A)[q] + 2 (x[q] + 1) (w (*) B)[q] + (y[q] + 1) (w (*) C)[q]),
 *   (w (*) F)[q] = sum over the valid positions p with q - 10 <= p <= q (per axis) of w[q - p] F[p].
 * Evaluated in fp32 with both images of a tile of positions centred on the photograph's value at the tile's first pixel (the
 * second moments do not depend on the shift and near white no longer cancel from 1); the sum of S in fp64, one partial per
 * workgroup and a fixed-order second launch, no floating-point atomics: two calls on the same input give the same bits.
 * ------------------------------------------------------------------------- */
/* Bytes of the partials of pasta_ssim_loss; 0 for a shape that is refused. */
int64_t pasta_ssim_loss_workspace(int N, int H, int W);
/* loss: one fp32 in device memory.  dmaps: null for the value alone, else [N, 3, 3, H - 10, W - 10] fp32, what
 * pasta_ssim_loss_backward gathers from (A relative to the tile's shift, B, C per position); it is only meaningful to that entry
 * with the same x and y.  H >= 11, W >= 11, N <= 65535, H and Wt <= 4096, c0 + W <= Wt. */
int pasta_ssim_loss(const float* x, const float* y, float* loss, float* dmaps /* null: value only */, void* workspace,
                    int64_t workspace_bytes, int N, int H, int Wt, int c0, int W, void* stream);
/* dx [N, 3, H, Wt] = *grad_loss * dloss/dx, written everywhere: exactly 0 outside the content columns.  grad_loss is ONE fp32 in
 * device memory (the loss weight times the gain), read by the kernel: nothing waits for the host.  Gather form, every element
 * written by one thread: a run repeats to the bit. */
int pasta_ssim_loss_backward(const float* x, const float* y, const float* dmaps, const float* grad_loss /* device scalar */,
                             float* dx /* [N,3,H,Wt], written everywhere, 0 outside the crop */, int N, int H, int Wt, int c0, int W,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * The region L1 term of training's unpaired pass (torch_utils/ops/region_l1_loss.py; csrc/region_l1.hip).  Additive
 * at ABI 22.  An image generated for a person in somebody else's garments has no photograph to be compared with, but three
 * regions of it have a known answer.
 * images: K (1 .. 4) fp32 [N,3,H,H] tensors x_k; targets retain, upper, lower: fp32 [N,3,H,H]; keep: uint8 [N,H,H];
 * upper_mask, lower_mask: fp32 [N,1,H,H].  A pixel belongs to exactly one region: 0 (keep) where keep != 0, else 1 where
 * upper_mask != 0, else 2 where lower_mask != 0, else none; the targets t_0, t_1, t_2 are retain, upper, lower.
 *   out[k][r] = (1 / M) * sum over the pixels of region r and the 3 channels of |x_k - t_r|,   M = 3 N H H,
 * so that out[k][0] + out[k][1] + out[k][2] is the part of F.l1_loss that falls into the regions.  |x - t| is one fp32
 * subtraction; the sums are fp64, one partial per workgroup and a fixed-order second launch, no floating-point atomics: two
 * calls on the same input give the same bits, and an empty region gives exactly 0.  out: fp32 [K, 3] in device memory.
 * Gradient with respect to the images only: with upstream g fp32 [K, 3] (device memory) and q = g[k][r] / (float)M (one fp32
 * division), dx_k = +q where x > t, -q where x < t, 0 where they are equal or the pixel has no region.
 * H a multiple of 4 (four pixels per thread, 16-byte accesses), H <= 4096, N <= 65535.
 * ------------------------------------------------------------------------- */
/* Bytes of the partials of pasta_region_l1_loss; 0 for a shape that is refused. */
int64_t pasta_region_l1_loss_workspace(int N, int H);
/* images: a HOST array of K device pointers.  maps: null for the values alone, else a HOST array of K device pointers to uint8
 * [N,H,H]: per pixel bits 0-1 = region + 1 (0: none) and bits 2-3, 4-5, 6-7 = channel 0, 1, 2: 0 where x == t, 1 where x > t,
 * 2 where x < t -- all pasta_region_l1_loss_backward reads. */
int pasta_region_l1_loss(const float* const* images, const float* retain, const float* upper, const float* lower, const uint8_t* keep,
                         const float* upper_mask, const float* lower_mask, float* out /* [K,3] */, uint8_t* const* maps,
                         void* workspace, int64_t workspace_bytes, int K, int N, int H, void* stream);
/* dx: a HOST array of K device pointers to fp32 [N,3,H,H], every element written by one thread.  grad_out: fp32 [K, 3] in device
 * memory, read by the kernel: nothing waits for the host. */
int pasta_region_l1_loss_backward(const uint8_t* const* maps, const float* grad_out /* device [K,3] */, float* const* dx, int K, int N,
                                  int H, void* stream);

/* ------------------------------------------------------------------------- *
 * The contextual loss of training's unpaired pass (torch_utils/ops/contextual_loss.py; csrc/contextual_loss.hip).
 * Additive at ABI 22.  It asks for the same texture without asking where: every position of x looks for its nearest position
 * of y, and is rewarded for how much that neighbour stands out among all of y's positions.
 * For feature maps x, y ([B, C, N], N positions, y constant) and the channel mean mu_p of y at position p:
 *   x^_p = (x_p - mu_p) / (|x_p - mu_p|_2 + 2.22e-16),  y^_p likewise          (unit vectors; the front-end forms them)
 *   d_ij = 1 - x^_i . y^_j                                                       (cosine distance, never stored)
 *   m_i  = min over the valid columns j of d_ij,  j*_i the smallest column that attains it,  c_i = 1 / (m_i + 1e-3)
 *   w_ij = exp((1 - d_ij c_i) / h),  S_i = sum over the valid columns of w_ij,  A_ij = w_ij / S_i
 *   CX_i = max_j A_ij = exp((1 - m_i c_i) / h) / S_i                             (w falls as d grows)
 *   loss_b = -log((1 / R) sum over the valid rows of CX_i),  R the number of valid rows.
 * Masks (uint8 [B, N], null = all valid, the same bits as all ones): a column with y_valid == 0 does not exist; a row with
 * x_valid == 0 does not enter the mean and gets gradient 0; a sample without a valid row or a valid column has loss 0 and
 * gradient 0.  Every exponent is at most 1 / h, so nothing is rescaled.
 * Gradient with respect to x^ only.  With E_i = sum_j A_ij d_ij and upstream g_b,
 *   dloss/dx^_i = g_b CX_i / (sum over valid rows of CX) ((c_i / h) (sum_j A_ij y^_j - y^_{j*}) - c_i^2 (E_i - m_i) / h  y^_{j*}).
 * The entries take x^ and y^; all products are the exact fp32-input MFMA; the workspace is O(B N): per row m, j*, S, E, CX,
 * per sample 1 / sum CX.  Row sums run in a fixed order (one lane, its twin, the other column half, then fp64 over the rows):
 * two calls on the same input give the same bits.  Column tiles (64) without a valid column and row groups (32) without a valid
 * row are skipped.  B <= 65535, 1 <= C <= 512, 1 <= N <= 16384; ragged C and N are handled in the kernels.
 * ------------------------------------------------------------------------- */
/* Bytes of the row statistics of pasta_contextual_loss, which pasta_contextual_loss_backward reads; 0 for a refused shape. */
int64_t pasta_contextual_loss_workspace(int B, int C, int N);
/* xh, yh: fp32 [B,C,N] unit vectors; loss: fp32 [B] in device memory.  The workspace must live until the backward has run. */
int pasta_contextual_loss(const float* xh, const float* yh, const uint8_t* x_valid /* [B,N] or null */,
                          const uint8_t* y_valid /* [B,N] or null */, float* loss /* [B] */, void* workspace, int64_t workspace_bytes,
                          int B, int C, int N, float h, void* stream);
/* dxh: fp32 [B,C,N], every element written by one thread.  yhT: yh as [B,N,C].  workspace: as pasta_contextual_loss left it for the
 * same xh, yh and masks.  grad_loss: fp32 [B] in device memory, read by the kernel: nothing waits for the host. */
int pasta_contextual_loss_backward(const float* xh, const float* yh, const float* yhT, const uint8_t* x_valid, const uint8_t* y_valid,
                                   const void* workspace, const float* grad_loss /* device [B] */, float* dxh, int B, int C, int N, float h,
                                   void* stream);

/* ------------------------------------------------------------------------- *
 * PNG files of a batch of RGB8 images, encoded on the GPU (torch_utils/ops/png_encode.py; csrc/png_encode.hip).
 * The stream is this project's own choice of a valid PNG:
 *   1. every row is filter type 4 (Paeth, bpp 3) with left, up and upper-left taken from the ORIGINAL pixels, zero outside the
 *      image; an image's filtered stream is H rows of 1 + 3 W bytes;
 *   2. PASTA_PNG_ROWS consecutive rows are a SEGMENT: one dynamic-Huffman deflate block (BFINAL 0) followed by an empty stored
 *      block (three header bits, BFINAL 1 only on the image's last segment, zeros to the byte boundary, 00 00 FF FF), so every
 *      segment starts and ends on a byte boundary;
 *   3. a segment's bytes are taken in tiles of 32 from its start; a full tile of zeros whose preceding byte in the image's
 *      filtered stream exists and is zero is ONE match (symbol 272 with extra bits 01 = length 32, distance symbol 0 =
 *      distance 1); every other byte is a literal; symbol 256 closes the block;
 *   4. the literal/length code (286 symbols, at most 15 bits) and the code-length code (19 symbols, at most 7 bits) are
 *      pasta_png_code_lengths of the segment's counts; HDIST = 0, the one distance code has length 1 with a match and 0 without;
 *      the header sends the 287 lengths plainly, without the run symbols 16 / 17 / 18;
 *   5. a segment's size follows from its counts and lengths, so every segment is written at its final place.
 * The caller frames the file: signature, IHDR, ONE IDAT of 78 01 | segments | Adler-32 (big-endian), IEND.
 * ------------------------------------------------------------------------- */
#define PASTA_PNG_ROWS        16    /* rows of a segment */
#define PASTA_PNG_SYMS        286   /* literal/length symbols */
#define PASTA_PNG_META_WORDS  288   /* per segment from the filter pass: 286 token counts, then the two Adler parts */
#define PASTA_PNG_TABLE_WORDS 354   /* per segment into the encode pass: 286 symbols, header bits, 0, 66 words of header */

/* images [N, H, W, C] uint8 -> filtered [N, H, 1 + 3 W] uint8 and meta [N, S, PASTA_PNG_META_WORDS] uint32, S = ceil(H /
 * PASTA_PNG_ROWS): words 0 .. 285 the segment's token counts (literals, 272 = matches, 256 = 1), word 286 = sum d_i mod 65521
 * and word 287 = sum (n - i) d_i mod 65521 over the segment's n bytes d_0 .. d_{n-1}; the Adler-32 of the stream follows from
 * A = 1, B = 0 and, per segment in order, B = (B + n A + s2) mod 65521, A = (A + s1) mod 65521.  One workgroup per (image,
 * segment).  Refused: C != 3, N outside 1 .. 65535, H or W outside 1 .. 8192, a filtered stream of 2^31 bytes or more. */
int pasta_png_filter(const uint8_t* images, uint8_t* filtered, uint32_t* meta, int N, int H, int W, int C, void* stream);

/* HOST ONLY, launches nothing: Huffman code lengths of counts[0 .. n - 1], none above `limit` bits (1 .. 15), 0 exactly where
 * the count is 0.  With two or more used symbols the code is COMPLETE, its Kraft sum exactly 1: inflate refuses an incomplete
 * literal/length or code-length set as it refuses an over-subscribed one.  A lone used symbol gets length 1.  Equal to the
 * unlimited Huffman code whenever that fits the limit.  n <= 288; refused when every count is 0 or 2^limit < used symbols. */
int pasta_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths);

/* HOST ONLY, launches nothing: meta [segments, PASTA_PNG_META_WORDS] as pasta_png_filter wrote it (HOST memory) -> tables
 * [segments, PASTA_PNG_TABLE_WORDS] uint32 and seg_bytes [segments], the exact size of every segment.  A table: words 0 .. 285
 * = bit-reversed code | bits << 24 of every symbol (272: the whole match, code | 01 | distance code 0, bits + 3), word 286 the
 * number of header bits, words 288 .. the block header's bits from BFINAL on, least significant bit first. */
int pasta_png_segment_tables(const uint32_t* meta, int64_t segments, uint32_t* tables, int64_t* seg_bytes);

/* filtered and tables as above (device), offsets [N, S] int64 (device): the byte every segment starts at in out.  out: out_bytes
 * bytes, ZEROED by the caller, 4-byte aligned, out_bytes a multiple of 4 and at least the last segment's end; nothing is
 * written past it.  One workgroup per (image, segment), one tile of 32 bytes per thread; bits are OR-ed or stored as whole
 * words, so the result does not depend on the order of execution. */
int pasta_png_encode(const uint8_t* filtered, const uint32_t* tables, const int64_t* offsets, uint8_t* out, int64_t out_bytes,
                     int N, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PASTA_HIP_H */
