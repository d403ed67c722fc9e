// The planner of the convolution family as plain C++: which kernel takes a descriptor, with which tile and how many K slices, where every
// region of its workspace lies, and the tap tables of its lattices.  Pure integer arithmetic on a pasta_conv_desc -- no HIP header, no
// device code: conv_igemm.hip (the C ABI and the launches) includes it, conv_common.h includes it for the constants the kernels share with
// it, and tests/host/conv_plan_check.cpp compiles it with the host compiler alone.  Everything here is decided once:
//   kernels      is_rows2d, is_fewch, wgrad_split over the PASTA_FWD_* / PASTA_WGRAD_* names of include/pasta_hip.h
//   shapes       the host predicates of the kernel families (rows_tile_ok, rows2d_rows, conv3x3s2_shape_ok, conv1x1_fewch_kind, ...)
//   forward      plan_fwd (tile, K slices), choose_fwd (the kernel), fwd_workspace (the one layout of the workspace)
//   gradients    plan_wgrad, plan_wgrad_small, choose_wgrad, wgrad_workspace
//   lattices     TapTable and its builders (conv2d, the parity classes of conv_transpose2d, the pair launch), detect_tap_rows
#ifndef PASTA_CONV_PLAN_H
#define PASTA_CONV_PLAN_H
#include <stddef.h>
#include <stdlib.h>
#include "../../include/pasta_hip.h"
#include "host_common.h"

namespace pasta {

constexpr int MAX_TAPS = 49;   // up to 7x7
constexpr int NP_F16X3 = 4;             // pseudo piece count of the template parameter NP: fp16 pieces, three products
constexpr int AMAX_PARTS = 256;         // partial maxima per tensor
// Leading floats of every convolution workspace: the partial |max| of the two operands (PASTA_MATH_F16X3)
constexpr int WS_AMAX_FLOATS = 2 * AMAX_PARTS;

// Tile choice.  O_pad multiple returned so that the caller can pack weights accordingly.
enum FwdTile { T128x128 = 0, T64x256 = 1, T32x256 = 2, T64x64 = 3 };

static inline int fwd_tile_bm(FwdTile t) { return t == T128x128 ? 128 : t == T32x256 ? 32 : 64; }
static inline int fwd_tile_bn(FwdTile t) { return t == T128x128 ? 128 : 256; }      // of the two tiles the split kernels run on

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

//------------------------------------------------------------------------------------
// Kernel names (include/pasta_hip.h) as predicates.

static inline bool is_rows2d(int k) { return k >= PASTA_FWD_ROWS2D_R4 && k <= PASTA_FWD_ROWS2D_WIDE; }
// the streaming pointwise kernels: raw weights, no packing, no workspace; they take 16-bit tensors themselves
static inline bool is_fewch(int k) { return k == PASTA_FWD_FEWCIN || k == PASTA_FWD_FEWCOUT; }
// The split weight-gradient kernels: 3x3 stride 1, 3x3 stride 2 (x as operand pieces included), pointwise.
static inline bool wgrad_split(int k) { return k == PASTA_WGRAD_3X3 || k == PASTA_WGRAD_3X3S2 || k == PASTA_WGRAD_1X1 || k == PASTA_WGRAD_3X3S2_PIECES; }

//------------------------------------------------------------------------------------
// Descriptor validation shared by the entry points.

static inline int check_desc(const pasta_conv_desc* d, const char* who) {
    PASTA_CHECK(d, "%s: null descriptor", who);
    PASTA_CHECK(d->N >= 1 && d->C_in >= 1 && d->H >= 1 && d->W >= 1 && d->C_out >= 1 && d->OH >= 1 && d->OW >= 1,
                "%s: empty tensor in descriptor", who);
    PASTA_CHECK(d->kh >= 1 && d->kw >= 1 && d->kh * d->kw <= MAX_TAPS, "%s: kernel %dx%d unsupported (max %d taps)", who, d->kh, d->kw, MAX_TAPS);
    PASTA_CHECK(d->stride >= 1 && d->stride <= 4, "%s: stride %d unsupported", who, d->stride);
    PASTA_CHECK(d->pad_h >= 0 && d->pad_w >= 0, "%s: negative padding", who);
    PASTA_CHECK(d->math >= PASTA_MATH_DEFAULT && d->math <= PASTA_MATH_F16X3, "%s: unknown math mode %d", who, d->math);
    PASTA_CHECK(d->io_dtype == PASTA_F32 || d->io_dtype == PASTA_F16 || d->io_dtype == PASTA_BF16, "%s: io_dtype %d is not PASTA_F32 / PASTA_F16 / PASTA_BF16", who, d->io_dtype);
    PASTA_CHECK(d->groups >= 1 && d->C_in % d->groups == 0 && d->C_out % d->groups == 0, "%s: channels not divisible by groups=%d", who, d->groups);
    PASTA_CHECK(d->x_layout == PASTA_LAYOUT_NCHW || d->x_layout == PASTA_LAYOUT_PIECES16, "%s: unknown x_layout %d", who, d->x_layout);
    if (!d->transposed) {
        const int oh = (d->H + 2 * d->pad_h - d->kh) / d->stride + 1, ow = (d->W + 2 * d->pad_w - d->kw) / d->stride + 1;
        PASTA_CHECK(d->H + 2 * d->pad_h >= d->kh && d->W + 2 * d->pad_w >= d->kw && oh == d->OH && ow == d->OW,
                    "%s: conv2d output is %dx%d, descriptor says %dx%d", who, oh, ow, d->OH, d->OW);
    } else {
        const int oh = (d->H - 1) * d->stride - 2 * d->pad_h + d->kh, ow = (d->W - 1) * d->stride - 2 * d->pad_w + d->kw;
        PASTA_CHECK(d->OH >= oh && d->OH < oh + d->stride && d->OW >= ow && d->OW < ow + d->stride,
                    "%s: conv_transpose2d output %dx%d not in [%d,%d)x[%d,%d)", who, d->OH, d->OW, oh, oh + d->stride, ow, ow + d->stride);
    }
    PASTA_CHECK((int64_t)d->N * d->C_in * d->H * d->W <= INT32_MAX && (int64_t)d->N * d->C_out * d->OH * d->OW <= INT32_MAX,
                "%s: tensor too large", who);
    return 0;
}

//------------------------------------------------------------------------------------
// Sub-expressions the predicates below share.

// anything but fp32 MFMA on fp32 tensors: the split kernels can take the launch
static inline bool split_arith(const pasta_conv_desc* d) { return d->math != PASTA_MATH_F32 || d->io_dtype != PASTA_F32; }
// a stride-2 conv_transpose2d whose output covers the doubled input plane: OH in [2H, 2H + 1] and OW in [2W, 2W + 1] ...
static inline bool doubled_plane(const pasta_conv_desc* d) { return d->OH >= 2 * d->H && d->OH <= 2 * d->H + 1 && d->OW >= 2 * d->W && d->OW <= 2 * d->W + 1; }
// ... with a remainder: output row 2H and / or column 2W
static inline bool doubled_remainder(const pasta_conv_desc* d) { return d->OH > 2 * d->H || d->OW > 2 * d->W; }
static inline bool is_3x3(const pasta_conv_desc* d) { return d->kh == 3 && d->kw == 3; }
// equal pads of 0 or 1
static inline bool pads_0_or_1(const pasta_conv_desc* d) { return d->pad_h == d->pad_w && d->pad_h <= 1; }

// The two tensors of a weight gradient: S [P x Q], the smaller-resolution one (dy for conv2d, x for conv_transpose2d), and L [LH x LW].
struct SLDims { int P, Q, LH, LW; };
static inline SLDims sl_dims(const pasta_conv_desc* d) {
    return d->transposed ? SLDims{d->H, d->W, d->OH, d->OW} : SLDims{d->OH, d->OW, d->H, d->W};
}

// bf16 pieces per operand of the split-bf16 kernels for a math mode
// (PASTA_MATH_F16X3: the pseudo count NP_F16X3 -- fp16 pieces, three products; conv_common.h)
static inline int math_pieces(int math) { return math == PASTA_MATH_BF16 ? 1 : math == PASTA_MATH_BF16X3 ? 2 : math == PASTA_MATH_BF16X6 ? 3 : NP_F16X3; }    // PASTA_MATH_DEFAULT = PASTA_MATH_F16X3
static inline bool fp32_equivalent(int pieces) { return pieces == 3 || pieces == NP_F16X3; }

//------------------------------------------------------------------------------------
// Shape predicates of the kernel families (the kernels are in the headers named).

// conv_fwd_bf16x6.h.  Pixel tiles of the row-reuse kernel: full tiles of BN pixels made of whole row segments inside one image.
static inline bool rows_tile_ok(int P, int Q, int BN) {
    const int seg = Q < BN ? Q : BN;
    return Q % 32 == 0 && (seg & (seg - 1)) == 0 && BN % seg == 0 && Q % seg == 0 && ((int64_t)P * Q) % BN == 0;
}

// conv_fwd_rows2d_bf16x6.h.  Is the 2-D tile applicable: 3x3 stride-1 lattice (9 taps in 3 rows of 3, any order), planes divisible into R x (BN / R) tiles.
template <int BN, int R>
static inline bool rows2d_tile_ok(int P, int Q) {
    constexpr int SEG = BN / R;
    return P % R == 0 && Q % SEG == 0;
}
// Rows per 2-D tile for a P x Q lattice on the 128 x 128 tile: 4 (32-column segments), else 2 (64 columns), else 0 = the row kernel.
static inline int rows2d_rows(int P, int Q) {
    if (rows2d_tile_ok<128, 4>(P, Q)) return 4;
    return rows2d_tile_ok<128, 2>(P, Q) ? 2 : 0;
}
// Eight waves on a 128 x 256 tile (8 rows x 32 columns; plain six-product fp32 launches): the weights of a step are fetched from L2
// and stored to LDS once for 256 pixels instead of once for 128 -- +3.7 .. 6 % over the four-wave 128 x 128 tile on every live
// shape (profiles/r2_rows2d.txt).  A 64 x 512 tile on eight waves (the 64-channel layers) spills and is 10 % slower: not kept.
// The 64 x 256 tile takes the same planes as tiles of eight rows.
static inline bool rows2d_r8(int P, int Q) { return rows2d_tile_ok<256, 8>(P, Q); }

// conv_fwd_s2.h.  Output planes of the stride-2 kernel: a width that is a power of two >= 16, planes that divide into 128-pixel tiles of whole rows.
// (The rest of its conditions: choose_fwd.)
static inline bool conv3x3s2_shape_ok(int OH, int OW) {
    if (OW < 16 || (OW & (OW - 1))) return false;
    const int seg = OW < 128 ? OW : 128, R = 128 / seg;
    return OH % R == 0;
}

// conv_fwd_fewch.h.  Which of the two takes a launch (0: neither): fp32 or 16-bit tensors (the stored element is converted on the way in and out: fp32 FMAs), 1x1, stride 1, no padding, one group, plain weights, no output scale / noise,
// planes of a multiple of four pixels, more than 8192 pixels (the K-sliced small-plane path keeps the rest); an input scale on the few-output side only.
static inline int conv1x1_fewch_kind(const pasta_conv_desc* d, bool has_iscale, bool has_oscale, bool has_noise, bool modulated) {
    if (d->kh != 1 || d->kw != 1 || d->stride != 1 || d->pad_h || d->pad_w || d->groups != 1) return 0;
    if (has_oscale || has_noise || modulated || d->x2 || d->x_layout || d->OH != d->H || d->OW != d->W) return 0;
    const int64_t hw = (int64_t)d->H * d->W;
    if (hw % 4 || (int64_t)d->N * hw <= 8192) return 0;
    if (d->C_in <= 16 && !has_iscale && d->C_out >= 16 && d->C_out <= 512) return 1;
    if (d->C_out <= 16 && d->C_in >= 16 && (int64_t)d->C_in * ((d->C_out + 3) & ~3) * 4 <= 64 * 1024) return 2;      // the launch's weights fit the default LDS window
    return 0;
}

// conv_wgrad_f32.h, wgrad_reduce_modulated_kernel.
// rows a per workgroup: 16, or 4 where 16 would leave the grid below 512 workgroups (the 64- and 128-channel layers: 75 MB of slabs each)
static inline int wgrad_mod_rows(int Ap, int Bp, int KK) { return (int64_t)(Bp / 64) * (Ap / 16) * KK >= 512 ? 16 : 4; }

// Chunk geometry of a weight gradient over rows of Q pixels: a chunk is kp lattice pixels, (kp >> cw_log2) rows of (1 << cw_log2) columns, the
// width a power of two that shrinks to cover Q (keep_width: it stays kp).
struct WgradChunks { int cw_log2, qblocks, chunks_total; };
static inline WgradChunks wgrad_chunks(int kp, int rows_total, int Q, bool keep_width = false) {
    WgradChunks c;
    int cw = kp, lg = kp == 32 ? 5 : 4;
    while (cw > 1 && cw / 2 >= Q && !keep_width) { cw /= 2; lg--; }
    const int chh = kp / cw;
    c.cw_log2 = lg;
    c.qblocks = (Q + cw - 1) / cw;
    c.chunks_total = ((rows_total + chh - 1) / chh) * c.qblocks;
    return c;
}

//------------------------------------------------------------------------------------
// Forward-type launches.

// Packed input-channel padding: a multiple of the KC of the kernel instance that will run.
static inline int fwd_ipad(int Ig, FwdTile t) { return (Ig <= 4 && t == T64x256) ? 4 : Ig <= 8 ? 8 : 16; }

// K slices for launches that would leave most CUs idle (the 4..17 pixel layers: K = 9*512 against <= 4624 pixels).
static inline int64_t fwd_lattice_pixels(const pasta_conv_desc* d) {
    if (!d->transposed) return (int64_t)d->N * d->OH * d->OW;
    return (int64_t)d->N * ((d->OH + d->stride - 1) / d->stride) * ((d->OW + d->stride - 1) / d->stride);
}

// The tile, the number of K slices, and whether the split-bf16 kernels may take a forward-type launch of d (choose_fwd below decides).
struct FwdPlan { FwdTile tile; int ksplit; int bf16x6; int packed; };     // packed: the few-input-channel mode (conv_fwd_bf16x6_kernel, KT)

// Do the split-bf16 kernels of this launch take the input scale (modulation) in their staging code?
static inline bool isc_in_staging(const pasta_conv_desc* d) { return d->io_dtype == PASTA_F32 && fp32_equivalent(math_pieces(d->math)); }

static inline FwdPlan plan_fwd(const pasta_conv_desc* d) {
    const int Og = d->C_out / d->groups, Ig = d->C_in / d->groups;
    const int64_t npix = fwd_lattice_pixels(d);
    const bool sb = split_arith(d) && Ig >= 16 && (int64_t)d->N * d->C_in * d->H * d->W < (1ll << 30);
    // fewer than 16 input channels into more than 32 output channels over a large plane with at least 64 (channel, tap) pairs -- the 7x7
    // RGB stems: 0.394 -> 0.234 ms.  Below (3x3: 27 pairs, 1x1: 3) the output store is what the launch costs and the fp32 kernel's
    // epilogue is the faster one: 0.113 -> 0.141 ms and 0.205 -> 0.366 ms when forced (profiles/r3_ab_packed_k.txt)
    const bool few = !d->transposed && d->groups == 1 && Ig < 16 && Og > 32 && npix > 8192 && d->io_dtype == PASTA_F32 &&
                     d->math != PASTA_MATH_F32 && fp32_equivalent(math_pieces(d->math)) && Ig * d->kh * d->kw >= 64 && Ig * d->kh * d->kw <= 1024 &&
                     (int64_t)d->N * d->C_in * (d->H + 2 * d->pad_h) * (d->W + 2 * d->pad_w) < (1ll << 28);
    FwdPlan f;
    f.packed = few;
    // ToRGB / parsing heads (<= 16 output channels): HBM-bound, few rows, fp32 MFMA.  17..32 output channels (the 512^2 block of the
    // 512 generator) take the 64-row split-bf16 tile half empty: 80 (fp32 storage) / 175 (16-bit) TFLOP/s effective against 55 on the
    // fp32 tile, and 16-bit tensors are not converted for the launch.
    if (Og <= 32 && !(sb && Og > 16 && npix > 8192)) f.tile = T32x256;
    else if (npix <= 8192) f.tile = (sb && Og > 64) ? T128x128 : T64x64;     // 4..16 pixel layers: K is sliced to fill the chip
    else if (Og <= 64) f.tile = T64x256;
    else f.tile = T128x128;
    f.bf16x6 = (sb || few) && (f.tile == T128x128 || f.tile == T64x256);
    f.packed = f.packed && f.bf16x6;
    f.ksplit = 1;
    if (npix <= 8192 && f.tile != T32x256) {
        const int bm = fwd_tile_bm(f.tile), bn = f.tile == T64x64 ? 64 : 128;
        int64_t blocks = ceil_div64(npix, bn) * ((Og + bm - 1) / bm) * d->groups;
        // conv_transpose2d: a parity class has between 1 and ceil(k/u)^2 of the taps; the slices are sized for the
        // smallest class, and on the split-bf16 kernel the u*u classes share the grid (merged_classes)
        const int taps = d->transposed ? 1 : d->kh * d->kw;
        if (d->transposed && f.bf16x6 && d->stride == 2) blocks *= 4;
        const int64_t k_total = (int64_t)taps * round_up(Ig, 16);
        int64_t ks = (f.tile == T64x64 ? 768 : 512) / (blocks > 0 ? blocks : 1);
        if (ks > k_total / 64) ks = k_total / 64;                     // at least 64 channel-taps per slice
        if (ks > 32) ks = 32;
        f.ksplit = ks < 2 ? 1 : (int)ks;
    }
    return f;
}

// The four output parity classes of a stride-2 conv_transpose2d share one class-major grid on the split-bf16 kernel:
// four times the workgroups per launch (measured 0.410 -> 0.266 ms on 512->256 @32^2, 0.262 -> 0.239 ms on 512->512 @16^2).
static inline bool merged_classes(const pasta_conv_desc* d, bool bf16x6) {
    return d->transposed && bf16x6 && d->stride == 2 && d->OH >= 2 && d->OW >= 2;
}

// a 3x3 stride-2 conv_transpose2d with fp32 tensors and no K slices onto the doubled plane: what the pair launch and the one-pass kernel share
static inline bool t2_3x3_doubled(const pasta_conv_desc* d, int ksplit) {
    return d->transposed && d->stride == 2 && is_3x3(d) && d->io_dtype == PASTA_F32 && ksplit == 1 && doubled_plane(d);
}

// Stride-2 3x3 conv_transpose2d whose output covers the doubled input plane (OH = 2H or 2H + 1): the parity-pair mode of the row-reuse
// kernel (conv_fwd_bf16x6.h) under the fp32-equivalent arithmetics, no K slices.  pair_small: also planes under 128 x 128 with a remainder.
static inline bool pair_launch_ok(const pasta_conv_desc* d, int pieces, int ksplit, FwdTile tile, bool pair_small) {
    if (!t2_3x3_doubled(d, ksplit) || !pads_0_or_1(d) || !fp32_equivalent(pieces)) return false;
    if (tile != T128x128 && tile != T64x256) return false;
    // Measured (profiles/r2_conv_pairs.txt): onto 2H x 2W outputs (no remainder) the pair kernel is 1.4x the per-class launch at
    // every size; with the remainder row / column it wins where the main launch outlasts the remainder's K loop (a few
    // dozen workgroups, 0.1 - 0.3 ms of serial latency however little they compute): input planes of 128 x 128 and larger.
    if (doubled_remainder(d) && (int64_t)d->H * d->W < 128 * 128 && !pair_small) return false;
    return rows_tile_ok(d->H, d->W, fwd_tile_bn(tile));
}

// ... or the one-pass kernel over the input lattice (conv_fwd_t2.h, round 5; PASTA_FWD_T2): pad 0, the three-product arithmetic, planes of
// 8 x 32 or 16 x 16 tiles, no K slices, one input tensor.  Takes precedence over the pair mode.  (At 32 x 32 and 16 x 16 the regular tiles of a
// batch of 16 fill the chip once or half, and what the edge tiles in front of them take is added to the launch: +7 % / +12 % there, +30 % / +50 %
// on the discriminator's stacked batches of 48 against planes of 64 x 64 and larger only -- profiles/r5_ab_conv_t2.txt.)
static inline bool t2_shape_ok(const pasta_conv_desc* d, int pieces, int ksplit) {
    if (!t2_3x3_doubled(d, ksplit) || d->pad_h != 0 || d->pad_w != 0) return false;
    if (pieces != NP_F16X3 || d->x2 || d->x_layout) return false;
    return d->C_in / d->groups >= 16 && ((d->H % 8 == 0 && d->W % 32 == 0) || (d->H % 16 == 0 && d->W % 16 == 0));
}

// How a conv_transpose2d launch covers its output parity classes.
enum TransposedLaunch { TL_NONE, TL_ONEPASS, TL_PAIR, TL_MERGED, TL_PER_CLASS };

// Everything the planner reports and the launch does for a forward-type launch of d with launch_flags (PASTA_PLAN_*).
struct FwdChoice {
    int kernel;             // PASTA_FWD_*; TL_PER_CLASS: the kernel of every class's launch
    FwdPlan plan;           // the flag-free plan the choice narrows: the workspace layout is a function of it alone (fwd_workspace)
    FwdTile tile;
    int ksplit;
    int pieces;             // operand pieces of the split-bf16 kernels as launched (16-bit storage: 1); 0: fp32 MFMA or a few-channel kernel
    int math;               // PASTA_MATH_* actually used
    int launches;           // launches of the main kernel
    TransposedLaunch tl;
    bool packed;            // the packed-K mode (PASTA_FWD_PACKED_K)
    bool pieces_ok;         // a kernel takes x as PASTA_LAYOUT_PIECES16
};

// The one place that chooses a forward-type kernel: pasta_conv2d_plan reports the choice, conv2d_run launches it.
static inline FwdChoice choose_fwd(const pasta_conv_desc* d, int launch_flags) {
    // Test-only routing overrides (tests/test_conv_rows2d_gpu.py, tests/test_conv_pairs_gpu.py), read once: they send more shapes to kernels
    // that are live elsewhere.  PASTA_ROWS2D=0: no 2-D tiles, =4: no eight-wave tile; PASTA_T2_PAIR=2: the pair mode on every eligible plane.
    static const int rows2d_mode = getenv("PASTA_ROWS2D") ? atoi(getenv("PASTA_ROWS2D")) : 8;
    static const bool pair_small = getenv("PASTA_T2_PAIR") && getenv("PASTA_T2_PAIR")[0] == '2';
    const bool iscale = launch_flags & PASTA_PLAN_ISCALE, oscale = launch_flags & PASTA_PLAN_OSCALE;
    const bool modulated = launch_flags & PASTA_PLAN_MODULATED, noise = launch_flags & PASTA_PLAN_NOISE;
    const FwdPlan f = plan_fwd(d);
    const int np = math_pieces(d->math);
    const bool f32 = d->io_dtype == PASTA_F32;
    FwdChoice c;
    c.plan = f;
    c.tile = f.tile;
    c.tl = TL_NONE;
    c.packed = false;
    c.pieces = 0;
    c.pieces_ok = false;
    if (const int few = conv1x1_fewch_kind(d, iscale, oscale, noise, modulated)) {
        // a streaming fp32 kernel on the raw weights (conv_fwd_fewch.h): no packing, no operand scale
        c.kernel = few == 1 ? PASTA_FWD_FEWCIN : PASTA_FWD_FEWCOUT; c.ksplit = 1; c.math = PASTA_MATH_F32; c.launches = 1;
        return c;
    }
    c.ksplit = f.ksplit;
    // An input scale rides in the staging of the split kernels under fp32-equivalent products on fp32 tensors only; the packed-K mode takes neither
    // an input scale nor modulated weights.
    const bool sb = f.bf16x6 && (!iscale || isc_in_staging(d)) && !(f.packed && (iscale || modulated));
    c.packed = sb && f.packed;
    c.pieces = !sb ? 0 : !f32 ? 1 : np;
    c.math = !sb ? PASTA_MATH_F32 : !f32 ? PASTA_MATH_BF16 : d->math == PASTA_MATH_BF16X3 ? PASTA_MATH_BF16X3 : d->math == PASTA_MATH_BF16 ? PASTA_MATH_BF16 :
             d->math == PASTA_MATH_BF16X6 ? PASTA_MATH_BF16X6 : PASTA_MATH_F16X3;
    const bool f16x3 = sb && f32 && np == NP_F16X3;
    // the pointwise kernel (conv_fwd_1x1.h): one group, no scale vectors or noise, >= 16 input and > 32 output channels, planes of whole pixel tiles
    const int bn1 = (d->C_out / d->groups) <= 64 ? 256 : 128;
    const bool c1x1 = f16x3 && d->groups == 1 && d->kh == 1 && d->kw == 1 && d->stride == 1 && !d->pad_h && !d->pad_w && !iscale && !oscale && !noise &&
                      c.ksplit == 1 && !c.packed && d->C_in >= 16 && d->C_out > 32 && d->OH == d->H && d->OW == d->W && ((int64_t)d->H * d->W) % bn1 == 0;
    // the stride-2 kernel (conv_fwd_s2.h): conv2d, 3x3, equal pads of 0 or 1, one group, no scale vectors (s2_fits) or noise (s2)
    const bool s2_fits = f16x3 && !d->transposed && d->groups == 1 && is_3x3(d) && d->stride == 2 && pads_0_or_1(d) &&
                         !iscale && !oscale && c.ksplit == 1 && !c.packed && d->C_in >= 16 && d->C_out > 32 && conv3x3s2_shape_ok(d->OH, d->OW);
    const bool s2 = s2_fits && !noise;
    const bool t2 = sb && t2_shape_ok(d, np, c.ksplit) && !(launch_flags & ~(PASTA_PLAN_ISCALE | PASTA_PLAN_MODULATED));
    // the pair kernel carries no scale vectors and no epilogue; modulated weights are packed like any others (the edge kernel modulates its own)
    const bool pair = !t2 && sb && !(launch_flags & ~PASTA_PLAN_MODULATED) && pair_launch_ok(d, np, c.ksplit, c.tile, pair_small);
    // the lattice of a stride-1 launch is the output plane itself, its taps kh rows of kw adjacent offsets
    const bool rows = sb && d->stride == 1 && d->kw == 3 && rows_tile_ok(d->OH, d->OW, fwd_tile_bn(c.tile));
    const bool plain6 = sb && d->stride == 1 && is_3x3(d) && rows2d_mode != 0;
    const int rows2d = plain6 && c.tile == T128x128 ? rows2d_rows(d->OH, d->OW) : 0;
    const bool rows2d_256 = plain6 && c.tile == T64x256 && rows2d_r8(d->OH, d->OW);
    // eight waves on 128 x 256: fp32 storage, fp32-equivalent products; an input scale under the three-product arithmetic only
    const bool wide = rows2d && rows2d_mode == 8 && (!iscale || np == NP_F16X3) && fp32_equivalent(np) && f32 && rows2d_r8(d->OH, d->OW);
    c.kernel = !sb ? PASTA_FWD_F32 : c1x1 ? PASTA_FWD_1X1 : s2 ? PASTA_FWD_3X3S2 : c.packed ? PASTA_FWD_PACKED_K : t2 ? PASTA_FWD_T2 : pair ? PASTA_FWD_PAIR :
               wide ? PASTA_FWD_ROWS2D_WIDE : rows2d ? (rows2d == 4 ? PASTA_FWD_ROWS2D_R4 : PASTA_FWD_ROWS2D_R2) : rows2d_256 ? PASTA_FWD_ROWS2D_R8 :
               rows ? PASTA_FWD_ROWS : PASTA_FWD_BASE;
    if (d->transposed)
        c.tl = t2 ? TL_ONEPASS : pair ? TL_PAIR : merged_classes(d, sb) ? TL_MERGED : TL_PER_CLASS;
    c.launches = c.tl == TL_PAIR ? 1 + (doubled_remainder(d) ? 1 : 0) : c.tl != TL_PER_CLASS ? 1 :
                 (d->stride < d->OH ? d->stride : d->OH) * (d->stride < d->OW ? d->stride : d->OW);
    // x as PASTA_LAYOUT_PIECES16: the stride-2 kernel with pad 0, or the eight-wave 2-D tile; plain launches, whole channel octets, one input tensor
    // (the launch refuses noise with it)
    c.pieces_ok = f16x3 && d->groups == 1 && !(launch_flags & (PASTA_PLAN_ISCALE | PASTA_PLAN_MODULATED)) && d->C_in >= 16 && (d->C_in & 7) == 0 && !d->x2 &&
                  (wide || (s2_fits && d->pad_h == 0));
    return c;
}

// Does the store of this launch take the input-activation mask (pasta_act_mask)?  The default arithmetic on fp32 tensors, no K slices, on a 2-D
// tile (3x3, stride 1: the mask is indexed like the output); the launch itself checks that it carries no scale vector, bias, noise or activation
// of its own.  Not the base kernel: with the masked store its three-workgroup instances go to scratch (12 -> 1152 bytes per lane for
// <128,128,3,NP_F16X3>) and EVERY launch of theirs ran at half speed (profiles/act_grad_in_writer_ab.txt); those launches keep the pass.
static inline bool mask_launch_ok(const pasta_conv_desc* d, const FwdChoice& c) {
    return c.pieces == NP_F16X3 && d->io_dtype == PASTA_F32 && c.ksplit == 1 && !d->x2 && !d->x_layout && is_rows2d(c.kernel) &&
           (c.tl == TL_NONE || c.tl == TL_MERGED || c.tl == TL_PER_CLASS);
}

// Where everything lies in the workspace of a forward-type launch, in floats from its (16-byte aligned) base:
//   [amax 2 x 256 | rowinv G x Og_pad | packed weights | K-slice partial sums | packed-K offset table | extra]
// extra: the zero-padded copy of the input (packed-K mode; absent where the convolution has no padding: the input itself serves), or the input's
// last column, gathered (the one-pass transposed kernel).  A function of the flag-free plan, so that one buffer serves every flag combination.
struct FwdWorkspace { int64_t rowinv, pack, partial, koff, extra, total_floats; };

static inline int fwd_workspace(const pasta_conv_desc* d, const FwdPlan& f, FwdWorkspace& ws) {
    const int Ig = d->C_in / d->groups, Og_pad = round_up(d->C_out / d->groups, fwd_tile_bm(f.tile));
    // packed weights: fp32 (4 B) or three bf16 pieces (6 B) per element; sized for the larger, in floats
    int64_t pack = ((int64_t)d->groups * d->kh * d->kw * round_up(Ig, fwd_ipad(Ig, f.tile)) * Og_pad * 3 + 1) / 2;
    const int64_t partial = f.ksplit > 1 ? (int64_t)f.ksplit * d->N * d->C_out * d->OH * d->OW : 0;
    int64_t koff = 0, extra = 0;
    if (f.packed) {         // [O][C_in kh kw] packed as a 1x1 weight, the offset table, the zero-padded copy of the input
        koff = round_up(Ig * d->kh * d->kw, 16);
        const int64_t pk = (koff * Og_pad * 3 + 1) / 2;
        pack = pack > pk ? pack : pk;
        if (d->pad_h || d->pad_w) extra = (int64_t)d->N * d->C_in * (d->H + 2 * d->pad_h) * (d->W + 2 * d->pad_w);
    }
    const bool t2 = t2_shape_ok(d, math_pieces(d->math), f.ksplit);
    if (t2) { koff = 0; extra = (int64_t)d->N * d->C_in * d->H; }      // conv_fwd_t2.h: the input's last column, gathered
    // both regions lie right behind the packed weights: nothing else may
    PASTA_CHECK(!(f.packed || t2) || partial == 0, "conv2d: the packed-K table and the one-pass kernel's column exist without K slices only");
    ws.rowinv = WS_AMAX_FLOATS;
    ws.pack = ws.rowinv + (int64_t)d->groups * Og_pad;      // rowinv: 1 / S_w per packed weight row (PASTA_MATH_F16X3)
    ws.partial = ws.pack + round_up((int)pack, 4);
    ws.koff = ws.partial + partial;
    ws.extra = ws.koff + koff;
    ws.total_floats = ws.koff + round_up((int)(koff + extra), 4);
    return 0;
}

//------------------------------------------------------------------------------------
// Weight gradients.

struct WgradPlan {
    int TR, TS, WA, WB, pipe, npos, kp, bf16x6, tgr, tgs, a_tiles, b_tiles, cw_log2, qblocks, chunks_total, ksplit, rows_total;
    int64_t slab_floats; size_t lds_bytes;
};

// 3x3, stride 1, pad 1 under a split arithmetic, both tensors of the same plane
static inline bool wgrad_3x3s1_same(const pasta_conv_desc* d, const SLDims& t) {
    return split_arith(d) && is_3x3(d) && d->stride == 1 && d->pad_h == 1 && d->pad_w == 1 && t.LH == t.P && t.LW == t.Q;
}

// ks_multiple > 1 (pasta_conv2d_wgrad_modulated: the batch size): the number of K slices is rounded UP to a multiple of it, so that no slice
// straddles two samples (the chunks are numbered sample-major and N divides their count where the caller checked)
// 3x3 stride-1 pad-1 weight gradients over planes of 16-pixel rows under a split arithmetic (round 5): the split kernel's chunk is 32 consecutive
// pixels of a row, so these ran on the fp32-MFMA kernel (75 - 99 TFLOP/s: 157 peak).  A 16-pixel row is taken as a 32-pixel chunk whose second half
// is zero (the S loads of the missing pixels are masked; the L halo's validity bits already zero the columns past the row): half of the MFMAs
// multiply zeros, and the launch still runs twice as fast.  8-pixel rows (a quarter filled) stay where they are.
static inline bool wgrad_wide16(const pasta_conv_desc* d) {
    const SLDims t = sl_dims(d);
    return wgrad_3x3s1_same(d, t) && t.Q == 16 && !d->x_layout;
}

// wide16 (round 5): 16-pixel rows as HALF-FILLED 32-pixel chunks of the split 3x3 stride-1 kernel (wgrad_wide16 above) instead of two-row chunks
// of the fp32 kernel
static inline WgradPlan plan_wgrad(int N, int P, int Q, int G, int Ag, int Bg, int kh, int kw, int st, int ks_multiple = 1, bool wide16 = false) {
    WgradPlan w;
    w.bf16x6 = 0;
    if (kh == 3 && kw == 3) { w.TR = 3; w.TS = 3; }
    else if (kw == 7) { w.TR = 1; w.TS = 7; }
    else if (kw == 4) { w.TR = 1; w.TS = 4; }
    else { w.TR = 1; w.TS = 1; }
    // single-tap kernels carry 16 accumulator registers per tile: give each wave 2 x 2 tiles when both
    // channel counts fill a 128-wide workgroup tile
    w.WA = w.WB = (w.TR * w.TS == 1 && Ag > 64 && Bg > 64) ? 2 : 1;
    const int BA = 64 * w.WA, BB = 64 * w.WB;
    w.tgr = (kh + w.TR - 1) / w.TR; w.tgs = (kw + w.TS - 1) / w.TS;
    w.a_tiles = (Ag + BA - 1) / BA; w.b_tiles = (Bg + BB - 1) / BB;
    // chunk = KP lattice pixels (CHH rows x CW columns, CW a power of two covering Q when Q is small); halve the
    // chunk when the L halo of a 32-pixel chunk is too wide for the register-prefetch pipeline (stride 2)
    int kp = 32;
    w.rows_total = N * P;
    for (;;) {
        const WgradChunks c = wgrad_chunks(kp, w.rows_total, Q, wide16);
        const int cw = 1 << c.cw_log2, chh = kp >> c.cw_log2;
        const int lwid = (cw - 1) * st + w.TS;
        w.cw_log2 = c.cw_log2; w.qblocks = c.qblocks; w.chunks_total = c.chunks_total;
        w.kp = kp; w.npos = chh * w.TR * lwid;
        if (w.npos <= 128 || kp == 16) break;
        kp = 16;
    }
    const int cw = 1 << w.cw_log2, chh = w.kp >> w.cw_log2;
    const int64_t base_blocks = (int64_t)G * w.a_tiles * w.b_tiles * w.tgr * w.tgs;
    int64_t ks = (512 + base_blocks / 2) / base_blocks;  // one full wave of workgroups at 2 per CU (register-limited)
    if (ks > w.chunks_total / 8) ks = w.chunks_total / 8; // at least eight chunks per slice
    if (ks < 1) ks = 1;
    if (ks > 1024) ks = 1024;
    if (ks_multiple > 1) ks = (ks + ks_multiple - 1) / ks_multiple * ks_multiple;
    w.ksplit = (int)ks;
    w.slab_floats = (int64_t)w.ksplit * G * kh * kw * w.a_tiles * BA * w.b_tiles * BB;
    const int lwid = (cw - 1) * st + w.TS, lpitch = lwid | 1, lch = (chh * w.TR * lpitch) | 1;
    w.lds_bytes = (size_t)(BA * (w.kp + 1) + BB * lch) * sizeof(float);
    w.pipe = w.npos <= 128 ? 1 : 0;
    return w;
}

// conv_wgrad_f32.h, conv_wgrad_smallcin_kernel: <= 8 input channels, (channel, tap) pairs as GEMM columns
struct WgradSmallPlan { bool use; int nb, bprime, cw_log2, qblocks, chunks_total, ksplit, a_tiles, rows_total; int64_t slab_floats; size_t lds_bytes; };

static inline WgradSmallPlan plan_wgrad_small(const pasta_conv_desc* d) {
    WgradSmallPlan w{}; w.use = false;
    const int Ig = d->C_in / d->groups;
    if (d->transposed || d->groups != 1 || d->stride != 1 || d->flip || Ig > 8 || Ig * d->kh * d->kw > 160) return w;
    w.use = true;
    w.bprime = Ig * d->kh * d->kw; w.nb = (w.bprime + 31) / 32;
    w.rows_total = d->N * d->OH;
    const WgradChunks c = wgrad_chunks(32, w.rows_total, d->OW);
    w.cw_log2 = c.cw_log2; w.qblocks = c.qblocks; w.chunks_total = c.chunks_total;
    const int cw = 1 << c.cw_log2, chh = 32 >> c.cw_log2;
    w.a_tiles = (d->C_out + 63) / 64;
    int64_t ks = (1024 + w.a_tiles - 1) / w.a_tiles;        // four workgroups per CU: one chunk in flight each
    if (ks > w.chunks_total / 8) ks = w.chunks_total / 8;
    if (ks < 1) ks = 1;
    w.ksplit = (int)ks;
    w.slab_floats = (int64_t)w.ksplit * w.a_tiles * 64 * w.nb * 32;
    w.lds_bytes = (size_t)(64 * 33 + Ig * chh * d->kh * (cw + d->kw - 1) + 4) * sizeof(float);
    if (Ig * chh * d->kh * (cw + d->kw - 1) > 1024) w.use = false;      // four halo slots per thread in the kernel
    return w;
}

// conv_wgrad_f32.h, wgrad1x1_fewcin_kernel.
// Does the few-channel pointwise kernel take this weight gradient, and with how many K slices (<= the slab the small-cin plan reserved)?
static inline int plan_wgrad1x1_fewcin(const pasta_conv_desc* d, const WgradSmallPlan& ws) {
    if (!ws.use || d->kh != 1 || d->kw != 1 || d->pad_h || d->pad_w || d->C_in > 8) return 0;      // (any storage type: round 5)
    const int64_t hw = (int64_t)d->H * d->W;
    if (hw % 4 || d->OH != d->H || d->OW != d->W) return 0;
    int64_t ks = (int64_t)d->N * (hw / 4) / (256 * 8);          // at least eight trips per thread
    ks = ks < 1 ? 1 : ks > 256 ? 256 : ks;
    return (int)(ks < ws.ksplit ? ks : ws.ksplit);
}

// The split-bf16 weight-gradient kernel covers 3x3, stride 1, pad 1, rows of a multiple of 32 pixels.
static inline bool wgrad_bf16x6(const pasta_conv_desc* d, const WgradPlan& w) {
    const SLDims t = sl_dims(d);
    return wgrad_3x3s1_same(d, t) && (t.Q % 32 == 0 || wgrad_wide16(d)) && w.kp == 32 && w.cw_log2 == 5;
}
// ... and its stride-2 sibling: 3x3, stride 2, equal pads of 0 or 1, rows of a multiple of 16 pixels.
static inline bool wgrad_s2_bf16x6(const pasta_conv_desc* d, const WgradPlan& w) {
    return split_arith(d) && is_3x3(d) && d->stride == 2 && pads_0_or_1(d) && sl_dims(d).Q % 16 == 0 && w.kp == 16 && w.cw_log2 == 4;
}
// ... with x as the producer wrote it (PASTA_LAYOUT_PIECES16): conv_wgrad3x3s2_pieces_kernel
static inline bool wgrad_pieces_ok(const pasta_conv_desc* d, const WgradPlan& w) {
    return d->x_layout == PASTA_LAYOUT_PIECES16 && wgrad_s2_bf16x6(d, w) && !d->transposed && d->pad_h == 0 && d->groups == 1 && d->io_dtype == PASTA_F32 &&
           math_pieces(d->math) == NP_F16X3 && (d->C_in & 7) == 0;
}
// ... and the pointwise one: 1x1, stride 1, no padding, planes of a multiple of 32 pixels (ToRGB heads included: the shape is
// bandwidth-bound, so a mostly empty 64-channel tile costs nothing).
static inline bool wgrad_1x1_bf16x6(const pasta_conv_desc* d, const WgradPlan& w) {
    const SLDims t = sl_dims(d);
    const int Ig = d->C_in / d->groups, Og = d->C_out / d->groups;
    return split_arith(d) && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad_h == 0 && d->pad_w == 0 &&
           ((int64_t)t.P * t.Q) % 32 == 0 && (Ig >= 16 || Og >= 16) && w.kp == 32 && w.WA == w.WB &&
           d->H == d->OH && d->W == d->OW && (int64_t)w.chunks_total == (int64_t)d->N * t.P * t.Q / 32;
}

// Everything the planner reports and the launch does for a weight gradient of d.
struct WgradChoice {
    int kernel;             // PASTA_WGRAD_*
    WgradSmallPlan small;   // PASTA_WGRAD_SMALLCIN and PASTA_WGRAD_FEWCIN
    int fewcin_ks;          // PASTA_WGRAD_FEWCIN: K slices
    WgradPlan w;            // every other kernel
};

// The one place that chooses a weight-gradient kernel.  ks_multiple: as plan_wgrad's (pasta_conv2d_wgrad_modulated: the batch size).
static inline WgradChoice choose_wgrad(const pasta_conv_desc* d, int ks_multiple) {
    WgradChoice c{};
    c.small = plan_wgrad_small(d);
    c.fewcin_ks = plan_wgrad1x1_fewcin(d, c.small);
    if (c.small.use) {
        c.kernel = c.fewcin_ks ? PASTA_WGRAD_FEWCIN : PASTA_WGRAD_SMALLCIN;
        return c;
    }
    const int Ig = d->C_in / d->groups, Og = d->C_out / d->groups;
    c.w = d->transposed ? plan_wgrad(d->N, d->H, d->W, d->groups, Ig, Og, d->kh, d->kw, d->stride, ks_multiple, wgrad_wide16(d))
                        : plan_wgrad(d->N, d->OH, d->OW, d->groups, Og, Ig, d->kh, d->kw, d->stride, ks_multiple, wgrad_wide16(d));
    c.kernel = wgrad_bf16x6(d, c.w) ? PASTA_WGRAD_3X3 : wgrad_s2_bf16x6(d, c.w) ? (wgrad_pieces_ok(d, c.w) ? PASTA_WGRAD_3X3S2_PIECES : PASTA_WGRAD_3X3S2) :
               wgrad_1x1_bf16x6(d, c.w) ? PASTA_WGRAD_1X1 : PASTA_WGRAD_F32;
    return c;
}

// Can the weight gradient of a MODULATED convolution come from the plain kernels with sample-aligned K slices (pasta_conv2d_wgrad_modulated)?
// The main split kernels only (3x3 stride 1 / stride 2, pointwise), fp32 storage, one group, up to 32 samples that the chunk count divides into.
static inline bool wgrad_modulated_ok(const pasta_conv_desc* d, const WgradChoice& c) {
    if (d->groups != 1 || d->io_dtype != PASTA_F32 || d->N < 1 || d->N > 32) return false;
    if (!wgrad_split(c.kernel)) return false;
    const WgradPlan& w = c.w;
    const int chh = w.kp >> w.cw_log2;
    return sl_dims(d).P % chh == 0 && w.chunks_total % d->N == 0 && w.ksplit <= w.chunks_total;     // whole chunks per sample, at least one chunk per slice
}
// partial-ds blocks of wgrad_reduce_modulated_kernel: (16-row a blocks | 64-column b tiles when the modulated index is a) x taps
static inline int wgrad_modulated_blocks(const pasta_conv_desc* d, const WgradPlan& w) {
    const int Ap = w.a_tiles * 64 * w.WA, Bp = w.b_tiles * 64 * w.WB;
    return (d->transposed ? Bp / 64 : Ap / wgrad_mod_rows(Ap, Bp, d->kh * d->kw)) * d->kh * d->kw;
}

// The workspace of a weight gradient, in floats from its base: [amax 2 x 256 | one slab per K slice | partial ds], the last for
// pasta_conv2d_wgrad_modulated only: one [N][C_in] block per workgroup row of wgrad_reduce_modulated_kernel.  Contractual (include/pasta_hip.h).
struct WgradWorkspace { int64_t slab, ds_partial, total_floats; };

static inline WgradWorkspace wgrad_workspace(const pasta_conv_desc* d, const WgradChoice& c, bool modulated) {
    WgradWorkspace ws;
    ws.slab = WS_AMAX_FLOATS;
    ws.ds_partial = ws.slab + (c.small.use ? c.small.slab_floats : c.w.slab_floats);
    ws.total_floats = ws.ds_partial + (modulated ? (int64_t)wgrad_modulated_blocks(d, c.w) * d->N * d->C_in : 0);
    return ws;
}

//------------------------------------------------------------------------------------
// Lattices.  A forward-type kernel walks lattices of output pixels: point (p, q) of a lattice is the output pixel (oy0 + p osy, ox0 + q osx),
// and tap t of its table multiplies weight element tap_slab[t] = r * kw + c with the input pixel (p isy + tap_dy[t], q isx + tap_dx[t]),
// zero outside the plane.  conv2d is one lattice (all output pixels, input step = stride); conv_transpose2d with stride u is u * u lattices, one
// per output parity class, so that no multiply ever meets a stuffed zero.

struct TapTable {
    int ncls;                                               // lattices sharing the table; class c owns taps [tap0, tap0 + T)
    struct Lattice { int P, Q, oy0, ox0, T, tap0; } cls[4];
    int tap_dy[MAX_TAPS], tap_dx[MAX_TAPS], tap_slab[MAX_TAPS];
    int isy, isx, osy, osx;
    int rows, rows_d0, rows_rev;                            // detect_tap_rows
};

// The parity rule of conv_transpose2d, along either axis: output row oy = iy * u - pad + r.  For parity class a (oy = a + u * p), tap r
// belongs to the class iff (a + pad - r) mod u == 0, and reads input row p + (a + pad - r) / u = p + *off.
static inline bool parity_tap(int a, int pad, int r, int u, int* off) {
    if (posmod(a + pad - r, u) != 0) return false;
    *off = floordiv(a + pad - r, u);
    return true;
}

// Do the taps of a one-lattice table form rows of three horizontally adjacent offsets (ascending or descending)?
static inline bool detect_tap_rows(TapTable& t) {
    t.rows = 0; t.rows_d0 = 0; t.rows_rev = 0;
    const int T = t.ncls == 1 ? t.cls[0].T : 0;
    if (T == 0 || T % 3 != 0 || t.isx != 1 || t.isy != 1 || t.osx != 1 || t.osy != 1) return false;
    const int step = t.tap_dx[1] - t.tap_dx[0];
    if (step != 1 && step != -1) return false;
    const int d0 = step == 1 ? t.tap_dx[0] : t.tap_dx[2];
    for (int j = 0; j < T; j += 3)
        for (int i = 0; i < 3; i++)
            if (t.tap_dy[j + i] != t.tap_dy[j] || t.tap_dx[j + i] != t.tap_dx[0] + i * step) return false;
    t.rows = 1; t.rows_d0 = d0; t.rows_rev = step == -1 ? 1 : 0;
    return true;
}

// conv2d: every output pixel, taps (r - pad_h, c - pad_w).  one_tap (the packed-K mode): the one tap is the window's corner in the zero-padded
// plane; the (channel, tap) pairs are in the kernel's offset table.
static inline void lattice_conv2d(const pasta_conv_desc* d, bool one_tap, TapTable& t) {
    t = TapTable{};
    t.osy = t.osx = 1; t.isy = t.isx = d->stride;
    int T = 0;
    if (one_tap) T = 1;
    else
        for (int r = 0; r < d->kh; r++)
            for (int c = 0; c < d->kw; c++, T++) { t.tap_dy[T] = r - d->pad_h; t.tap_dx[T] = c - d->pad_w; t.tap_slab[T] = T; }
    t.ncls = 1; t.cls[0] = {d->OH, d->OW, 0, 0, T, 0};
    detect_tap_rows(t);
}

// One parity class (a, b) of a conv_transpose2d appended to the table: the P x Q lattice points whose first output pixel is (oy0, ox0).
// py_shift / px_shift: the class's first lattice point is row / column `shift` of the class, not 0 (the remainder classes of the pair launch:
// one row or column at the far edge); a tap that then reads below the last input row or right of the last input column is zero for the whole
// class and left out.  -> the taps of the class.
static inline int lattice_add_class(const pasta_conv_desc* d, int a, int b, int P, int Q, int oy0, int ox0, int py_shift, int px_shift, TapTable& t) {
    const int u = d->stride;
    const int tap0 = t.ncls ? t.cls[t.ncls - 1].tap0 + t.cls[t.ncls - 1].T : 0;
    int ntap = tap0, dy, dx;
    for (int r = 0; r < d->kh; r++) {
        if (!parity_tap(a, d->pad_h, r, u, &dy)) continue;
        if (py_shift && dy + py_shift >= d->H) continue;
        for (int c = 0; c < d->kw; c++) {
            if (!parity_tap(b, d->pad_w, c, u, &dx)) continue;
            if (px_shift && dx + px_shift >= d->W) continue;
            t.tap_dy[ntap] = dy + py_shift; t.tap_dx[ntap] = dx + px_shift; t.tap_slab[ntap] = r * d->kw + c;
            ntap++;
        }
    }
    t.cls[t.ncls++] = {P, Q, oy0, ox0, ntap - tap0, tap0};
    return ntap - tap0;
}

// conv_transpose2d: all parity classes in one table (only < 0: they share a grid, stride 2), or class number `only` alone, counted a-major over
// the classes the output plane has.
static inline int lattice_transposed(const pasta_conv_desc* d, int only, TapTable& t) {
    const int u = d->stride;
    t = TapTable{};
    t.osy = t.osx = u; t.isy = t.isx = 1;
    int k = 0;
    for (int a = 0; a < u && a < d->OH; a++)
        for (int b = 0; b < u && b < d->OW; b++, k++) {
            if (only >= 0 && k != only) continue;
            if (!lattice_add_class(d, a, b, (d->OH - a + u - 1) / u, (d->OW - b + u - 1) / u, a, b, 0, 0, t))   // no tap reaches this class: the outputs are zero
                return fail("conv_transpose2d: kernel %dx%d smaller than stride %d leaves empty output classes (unsupported)", d->kh, d->kw, u);
        }
    detect_tap_rows(t);
    return 0;
}

// The remainder of the pair launch (3x3, stride 2, pad_h == pad_w): output row 2H and / or column 2W, as up to four one-row / one-column classes.
static inline void lattice_pair_remainder(const pasta_conv_desc* d, TapTable& t) {
    const int H = d->H, W = d->W;
    t = TapTable{};
    t.osy = t.osx = 2; t.isy = t.isx = 1;
    if (d->OH == 2 * H + 1) {                             // oy = 2H (a = 0, p = H): every column
        lattice_add_class(d, 0, 0, 1, (d->OW + 1) / 2, 2 * H, 0, H, 0, t);
        lattice_add_class(d, 0, 1, 1, d->OW / 2, 2 * H, 1, H, 0, t);
    }
    if (d->OW == 2 * W + 1) {                             // ox = 2W (b = 0, q = W): the rows below 2H
        lattice_add_class(d, 0, 0, H, 1, 0, 2 * W, 0, W, t);
        lattice_add_class(d, 1, 0, H, 1, 1, 2 * W, 0, W, t);
    }
}

// The main lattice of the pair launch: (p, q) of the input plane -> outputs (2p + a, 2q + b), a, b in {0, 1}.  Two classes, the vertical
// parities, with their kernel rows from the parity rule; the columns are the kernel's own encoding (conv_fwd_bf16x6.h, PAIR): every tap has
// tap_dx 0, and pair_bx, pair_off and rows_d0 say where the three taps of a kernel row read.
struct PairLattice { TapTable t; int pair_off[3], pair_bx; };

static inline void lattice_pair_main(const pasta_conv_desc* d, PairLattice& pl) {
    const int pad = d->pad_h;
    TapTable& t = pl.t;
    t = TapTable{};
    t.osy = t.osx = 2; t.isy = t.isx = 1;
    t.ncls = 2; t.rows = 1; t.rows_rev = 0;
    pl.pair_bx = pad & 1;                                 // the column with two taps (c = 0, 2)
    const int dx0 = (pl.pair_bx + pad) / 2;               // input offset of tap c = 0; tap c = 2 reads one pixel to its left
    const int dx1 = floordiv((1 - pl.pair_bx) + pad - 1, 2);
    t.rows_d0 = dx0 - 1;
    pl.pair_off[0] = 1; pl.pair_off[1] = dx1 - t.rows_d0; pl.pair_off[2] = 0;
    for (int k = 0; k < 2; k++) {
        const int a = k == 0 ? (pad & 1) : 1 - (pad & 1);          // class 0: the parity with two kernel rows
        int nt = 0, dy;
        for (int r = 0; r < 3; r++) {
            if (!parity_tap(a, pad, r, 2, &dy)) continue;
            for (int c = 0; c < 3; c++, nt++) { t.tap_dy[6 * k + nt] = dy; t.tap_dx[6 * k + nt] = 0; t.tap_slab[6 * k + nt] = r * 3 + c; }
        }
        t.cls[k] = {d->H, d->W, a, 0, nt, 6 * k};
    }
}

}  // namespace pasta

#endif  // PASTA_CONV_PLAN_H
