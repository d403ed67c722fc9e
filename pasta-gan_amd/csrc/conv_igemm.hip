// Dense convolution family for gfx950: conv2d, conv_transpose2d and the weight gradient of either, NCHW fp32, on the
// matrix cores -- split-bf16 with fp32-equivalent products (v_mfma_f32_32x32x16_bf16, default) or fp32 MFMA
// (v_mfma_f32_32x32x2_f32).  This file holds the C entry points and the launches: check, choose, lay out the workspace, find the operand
// scales, pack, build the lattice, launch, reduce.  What is chosen and where it lies is decided in conv_plan.h, plain C++ that a host compiler
// builds and tests alone.  The kernels live in headers this file does not include: every kernel family is compiled in a translation unit of
// its own, conv_tu_*.hip, and reached through the functions of conv_launch.h -- nineteen units built in parallel (one unit of 161 kernels
// took 3 - 12 minutes):
//   conv_plan.h                the planner: kernel choice, shape predicates, workspace layouts, tap tables (no HIP header)
//   conv_common.h              parameter blocks, the shared epilogue of the split forward-type kernels (conv_unscale_rows,
//                              conv_store_subtile) and the (input scale, storage, pieces) -> <NP, IO, ISC> dispatch of their launches
//   conv_fwd_f32.h             fp32-MFMA forward-type kernel, its weight packing    -> conv_tu_pack_f32.hip
//   conv_pack.h                weight packing of the split forward-type kernels     -> conv_tu_pack_f32.hip
//   conv_fwd_mma.h             the K-loop body of the split forward-type kernels, once: operand split (fwd_split2), fragment read order
//                              (fwd_read_frag), product schedule (fwd_products); included by the five headers below
//   conv_fwd_bf16x6.h          split forward-type kernels (base and row-reuse)      -> conv_tu_fwd_base_{128,64}.hip, conv_tu_fwd_rows_{128,64}.hip
//   conv_fwd_rows2d_bf16x6.h   2-D pixel tiles                                      -> conv_tu_rows2d_{wide,wide_xp,128_r4,128_r2,64_r8}.hip
//   conv_fwd_1x1.h, conv_fwd_s2.h  pointwise and stride-2 kernels                   -> conv_tu_fwd_small.hip
//   conv_fwd_t2.h              stride-2 conv_transpose2d in one pass                -> conv_tu_fwd_t2.hip
//   conv_wgrad_f32.h           fp32-MFMA weight gradients, few-channel kernels, slab reductions -> conv_tu_wgrad_f32.hip
//   conv_wgrad_bf16x6.h        split weight-gradient kernels                        -> conv_tu_wgrad_{3x3,3x3s2,1x1}.hip
//   (no header)                K-slice reduction, pair-launch remainder, packed-K set-up -> conv_tu_aux.hip
//
// Stands where the reference hands its convolutions to ATen/cuDNN
// (torch_utils/ops/conv2d_gradfix.py:38,43 forward; :125-128 input gradient through the
// transposed operator; :140-148 weight gradient).  Everything here is an implicit GEMM:
//
//   forward-type kernel   C[o][pix] = sum_{tap,i} Wp[tap][i][o] * X[i][pix + tap offset]
//       rows    = output channels of one group          (MFMA "A" operand = packed weights)
//       columns = a lattice of output pixels            (MFMA "B" operand = gathered activations)
//     conv2d is one lattice (all output pixels, input step = stride); conv_transpose2d with
//     stride u is u*u lattices (one per output parity class) so no multiply ever meets a
//     stuffed zero.  Optional per-(n,channel) input and output scales carry the StyleGAN2
//     modulation / demodulation (training/networks.py:74, 77-79).
//
//   weight-gradient kernel  dW[tap][a][b] = sum_pix S[a][pix] * L[b][pix*stride + tap offset]
//       S = the smaller-resolution tensor (dy for conv2d, x for conv_transpose2d), L the other.
//     K (= pixels) is split across workgroups; partial slabs are summed in a fixed order by a
//     second kernel that also writes PyTorch's [.., .., kh, kw] layout (bitwise reproducible).
//
// C/D fragment map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5).
#include "conv_launch.h"

namespace pasta {

// The split forward-type kernels on a 128 x 128 or 64 x 256 tile: the row-reuse kernel (rows: the lattice is made of whole row segments), else
// the base kernel.
static void launch_fwd_bf16x6(bool tile128, bool rows, const ConvFwdParams& p, hipStream_t s) {
    const int BM = tile128 ? 128 : 64, BN = tile128 ? 128 : 256;
    ConvFwdParams q = p;
    q.o_tiles = (p.Og + BM - 1) / BM;
    int64_t tiles = 0;
    for (int c = 0; c < p.ncls; c++) {
        const int64_t t = ceil_div64((int64_t)p.N * p.cls[c].P * p.cls[c].Q, BN);
        if (t > tiles) tiles = t;
    }
    tiles *= p.ncls;
    const dim3 grid((unsigned)tiles, q.o_tiles * q.ksplit, p.G);
    if (rows) { if (tile128) tu_fwd_rows_128(q, grid, s); else tu_fwd_rows_64(q, grid, s); }
    else      { if (tile128) tu_fwd_base_128(q, grid, s); else tu_fwd_base_64(q, grid, s); }
}

// A 3x3 stride-1 lattice on 2-D tiles (is_rows2d): the rows of the tile start at the lattice's first tap row.
static void launch_fwd_rows2d(int kernel, const ConvFwdParams& p, hipStream_t s) {
    ConvFwdParams q = p;
    q.rows_y0 = p.tap_dy[0];
    for (int t = 1; t < 9; t++) q.rows_y0 = p.tap_dy[t] < q.rows_y0 ? p.tap_dy[t] : q.rows_y0;
    if (kernel == PASTA_FWD_ROWS2D_WIDE) { if (q.x_pieces) tu_rows2d_wide_pieces(q, s); else tu_rows2d_wide(q, s); }
    else if (kernel == PASTA_FWD_ROWS2D_R4) tu_rows2d_128_r4(q, s);
    else if (kernel == PASTA_FWD_ROWS2D_R2) tu_rows2d_128_r2(q, s);
    else tu_rows2d_64_r8(q, s);
}

// One lattice of a forward-type launch on the kernel choose_fwd chose (fp32 MFMA, base, row reuse or a 2-D tile; the table says whether its
// taps form rows).
static void launch_lattice(const FwdChoice& c, const ConvFwdParams& p, hipStream_t s) {
    if (c.kernel == PASTA_FWD_F32) tu_fwd_f32(c.tile, p, s);
    else if (is_rows2d(c.kernel)) launch_fwd_rows2d(c.kernel, p, s);
    else launch_fwd_bf16x6(c.tile == T128x128, c.kernel == PASTA_FWD_ROWS, p, s);
}

// The lattices of a launch as the kernels read them (ConvFwdParams is kernel ABI; P, Q, oy0, ox0, T: those of the table's last lattice).
static void set_lattice(ConvFwdParams& p, const TapTable& t) {
    p.ncls = t.ncls;
    for (int c = 0; c < 4; c++) p.cls[c] = {t.cls[c].P, t.cls[c].Q, t.cls[c].oy0, t.cls[c].ox0, t.cls[c].T, t.cls[c].tap0};
    memcpy(p.tap_dy, t.tap_dy, sizeof(p.tap_dy)); memcpy(p.tap_dx, t.tap_dx, sizeof(p.tap_dx)); memcpy(p.tap_slab, t.tap_slab, sizeof(p.tap_slab));
    p.isy = t.isy; p.isx = t.isx; p.osy = t.osy; p.osx = t.osx;
    p.rows = t.rows; p.rows_d0 = t.rows_d0; p.rows_rev = t.rows_rev;
    const TapTable::Lattice& l = t.cls[t.ncls > 0 ? t.ncls - 1 : 0];
    p.P = l.P; p.Q = l.Q; p.oy0 = l.oy0; p.ox0 = l.ox0; p.T = l.T;
}

// the factor applied to the weights on the way in; a descriptor that leaves it zero means one
static float desc_wscale(const pasta_conv_desc* d) { return d->wscale == 0.f ? 1.f : d->wscale; }

static inline int launch_flags_of(const float* iscale, const float* oscale, const pasta_conv_epilogue* ep, const float* wmod_s) {
    return (iscale ? PASTA_PLAN_ISCALE : 0) | (oscale ? PASTA_PLAN_OSCALE : 0) | (ep ? PASTA_PLAN_EPILOGUE : 0) | (wmod_s ? PASTA_PLAN_MODULATED : 0) |
           (ep && ep->noise ? PASTA_PLAN_NOISE : 0);
}

// The pair launch of a stride-2 conv_transpose2d: the remainder (output row 2H and / or column 2W) by conv_t2_edge_kernel, then the main
// lattice over the input plane.
static void launch_transposed_pairs(const pasta_conv_desc* d, const ConvFwdParams& base, FwdTile tile, hipStream_t s, const EdgeWeights& ew) {
    TapTable rem;
    lattice_pair_remainder(d, rem);
    if (rem.ncls) {
        ConvFwdParams q = base;
        set_lattice(q, rem);
        tu_conv_t2_edge(q, ew, s);
    }
    PairLattice pl;
    lattice_pair_main(d, pl);
    ConvFwdParams p = base;
    set_lattice(p, pl.t);
    p.pair_bx = pl.pair_bx;
    for (int i = 0; i < 3; i++) p.pair_off[i] = pl.pair_off[i];
    if (tile == T128x128) tu_fwd_pair_128(p, s); else tu_fwd_pair_64(p, s);
}

static int conv2d_run(const void* x, const float* w, void* y, const float* iscale, const float* oscale,
                      const pasta_conv_epilogue* ep, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                      void* stream, const float* wmod_s, const float* wmod_d, const pasta_act_mask* mask = nullptr);
static int wgrad_run(const void* xv, const void* dyv, float* dw, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream,
                     const float* mod_s, const float* mod_w, float* ds);

// The packing job of a plain launch (no scale vectors, plain weights, one input tensor) of the default arithmetic on fp32 tensors, as conv2d_run
// would perform it at the head of the launch: false where the launch packs differently or not at all (few-channel kernels, the packed-K
// mode of the stems, 16-bit storage, the other arithmetics) -- the caller then leaves w_prepacked at 0.
static bool pack_job_of(const pasta_conv_desc* d, void* workspace, PackJob& j) {
    const FwdChoice c = choose_fwd(d, 0);
    FwdWorkspace lay;
    if (c.pieces != NP_F16X3 || c.packed || d->io_dtype != PASTA_F32 || d->x2 || fwd_workspace(d, c.plan, lay)) return false;
    const int Ig = d->C_in / d->groups, Og = d->C_out / d->groups;
    j.rowinv = (float*)workspace + lay.rowinv;
    j.wp = (float*)workspace + lay.pack;
    j.G = d->groups; j.Ig = Ig; j.Og = Og;
    j.Ig_pad = round_up(Ig, fwd_ipad(Ig, c.tile)); j.Og_pad = round_up(Og, fwd_tile_bm(c.tile));
    j.kh = d->kh; j.kw = d->kw; j.transposed = d->transposed; j.flip = d->flip;
    j.wscale = desc_wscale(d);
    j.pack_xcd_rows = (j.Og_pad & 63) == 0 ? 1 : 0;
    return true;
}

}  // namespace pasta

//------------------------------------------------------------------------------------
// C ABI.

extern "C" int64_t pasta_conv2d_workspace(const pasta_conv_desc* d) {
    using namespace pasta;
    FwdWorkspace lay;
    if (check_desc(d, "conv2d_workspace") || fwd_workspace(d, plan_fwd(d), lay)) return -1;
    return lay.total_floats * (int64_t)sizeof(float);
}

extern "C" int pasta_conv2d_tile(const pasta_conv_desc* d) {
    using namespace pasta;
    if (check_desc(d, "conv2d_tile")) return -1;
    return (int)plan_fwd(d).tile;
}

extern "C" int pasta_conv2d_plan(const pasta_conv_desc* d, int launch_flags, int* tile, int* ksplit, int* math, int* launches, int* kernel) {
    using namespace pasta;
    if (int e = check_desc(d, "conv2d_plan")) return e;
    const FwdChoice c = choose_fwd(d, launch_flags);
    if (d->io_dtype != PASTA_F32 && !c.pieces && !is_fewch(c.kernel))      // (every other kernel above them runs with pieces)
        return fail("conv2d: no 16-bit-storage kernel for this shape (fewer than 16 input channels per group, at most 32 "
                    "output channels, or an input scale -- pointwise layers over more than 8192 pixels excepted): convert the tensors to fp32 for this launch");
    if (tile) *tile = (int)c.tile;
    if (ksplit) *ksplit = c.ksplit;
    if (math) *math = c.math;
    if (launches) *launches = c.launches;
    if (kernel) *kernel = c.kernel;
    if (d->x_layout == PASTA_LAYOUT_PIECES16 && !c.pieces_ok)
        return fail("conv2d: x_layout = PASTA_LAYOUT_PIECES16 is served by the 3x3 stride-2 forward kernel (conv2d, pad 0, fp32 y, PASTA_MATH_F16X3, one group, "
                    "C_in a multiple of 8 and >= 16, C_out > 32, output width a power of two >= 16, more than 8192 output pixels, no scale vectors) and by the "
                    "eight-wave 3x3 stride-1 tile kernel (plan kernel 7, no input scale, C_in a multiple of 8) only");
    return 0;
}

extern "C" int pasta_conv2d(const void* x, const float* w, void* y, const float* iscale, const float* oscale,
                            const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream) {
    return pasta_conv2d_ex(x, w, y, iscale, oscale, nullptr, d, workspace, workspace_bytes, stream);
}

extern "C" int pasta_conv2d_ex(const void* x, const float* w, void* y, const float* iscale, const float* oscale,
                               const pasta_conv_epilogue* ep, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    return pasta_conv2d_masked(x, w, y, iscale, oscale, ep, nullptr, d, workspace, workspace_bytes, stream);
}

extern "C" int pasta_conv2d_masked(const void* x, const float* w, void* y, const float* iscale, const float* oscale,
                                   const pasta_conv_epilogue* ep, const pasta_act_mask* mask, const pasta_conv_desc* d, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    return pasta::conv2d_run(x, w, y, iscale, oscale, ep, d, workspace, workspace_bytes, stream, nullptr, nullptr, mask);
}

extern "C" int pasta_conv2d_mask_available(const pasta_conv_desc* d, int launch_flags) {
    using namespace pasta;
    if (check_desc(d, "conv2d_mask_available")) return -1;
    if (launch_flags & ~PASTA_PLAN_EPILOGUE) return 0;
    return mask_launch_ok(d, choose_fwd(d, launch_flags)) ? 1 : 0;
}

extern "C" int pasta_conv2d_modulated(const void* x, const float* w, const float* styles, const float* dcoefs, void* y,
                                      const pasta_conv_epilogue* ep, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
    using namespace pasta;
    PASTA_CHECK(styles, "conv2d_modulated: null styles");
    return conv2d_run(x, w, y, nullptr, nullptr, ep, d, workspace, workspace_bytes, stream, styles, dcoefs);
}

extern "C" int pasta_conv2d_pack_pair(const float* w, const pasta_conv_desc* da, void* ws_a, int64_t ws_a_bytes, const pasta_conv_desc* db, void* ws_b,
                                      int64_t ws_b_bytes, void* stream, int* packed_mask) {
    using namespace pasta;
    PASTA_CHECK(w && da && db && ws_a && ws_b && packed_mask, "conv2d_pack_pair: null pointer");
    *packed_mask = 0;
    if (int e = check_desc(da, "conv2d_pack_pair")) return e;
    if (int e = check_desc(db, "conv2d_pack_pair")) return e;
    PASTA_CHECK(ws_a_bytes >= pasta_conv2d_workspace(da) && ws_b_bytes >= pasta_conv2d_workspace(db), "conv2d_pack_pair: workspace too small");
    PASTA_CHECK((((uintptr_t)ws_a | (uintptr_t)ws_b) & 15) == 0, "conv2d_pack_pair: workspaces must be 16-byte aligned");
    PackJob a, b;
    // both or nothing: one orientation alone is the launch the convolution would have made itself
    if (da->groups != db->groups || !pack_job_of(da, ws_a, a) || !pack_job_of(db, ws_b, b)) return 0;
    tu_pack_weights_f16x3_pair(w, a, b, (hipStream_t)stream);
    *packed_mask = 3;
    return launch_status("conv2d_pack_pair");
}

int pasta::conv2d_run(const void* x, const float* w, void* y, const float* iscale, const float* oscale,
                      const pasta_conv_epilogue* ep, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes,
                      void* stream, const float* wmod_s, const float* wmod_d, const pasta_act_mask* mask) {
    // ---- check
    if (int e = check_desc(d, "conv2d")) return e;
    PASTA_CHECK(!ep || (ep->act >= 1 && ep->act <= 3), "conv2d: fused epilogue supports act 1..3 (linear, relu, lrelu), got %d", ep ? ep->act : 0);
    PASTA_CHECK(!ep || !ep->noise || ep->noise_strength, "conv2d: noise without noise_strength");
    PASTA_CHECK(x && w && y, "conv2d: null pointer");
    // ---- choose, and lay out the workspace
    const FwdChoice ch = choose_fwd(d, launch_flags_of(iscale, oscale, ep, wmod_s));
    if (mask) {
        PASTA_CHECK(mask->m && mask->act >= 1 && mask->act <= 3, "conv2d: the input-activation mask needs its tensor and act 1..3 (linear, relu, lrelu)");
        PASTA_CHECK(!iscale && !oscale && !wmod_s && (!ep || (ep->act == 1 && !ep->bias && !ep->noise && ep->gain == 1.f && ep->clamp < 0.f)),
                    "conv2d: a launch with the input-activation mask carries no scale vector, bias, noise or activation of its own");
        PASTA_CHECK(mask_launch_ok(d, ch), "conv2d: no kernel applies the input-activation mask for this launch (pasta_conv2d_mask_available tells "
                                           "beforehand): run pasta_bias_act with grad = 1 on the result instead");
    }
    FwdWorkspace lay;
    if (int e = fwd_workspace(d, ch.plan, lay)) return e;
    const int64_t need = lay.total_floats * (int64_t)sizeof(float);
    PASTA_CHECK(workspace && workspace_bytes >= need, "conv2d: workspace of %lld bytes needed, %lld given", (long long)need, (long long)workspace_bytes);
    PASTA_CHECK(((uintptr_t)workspace & 15) == 0, "conv2d: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (is_fewch(ch.kernel)) {
        FewChParams q;
        q.x = x; q.w = w; q.y = y; q.iscale = iscale; q.io = d->io_dtype;
        q.bias = ep ? ep->bias : nullptr; q.res = ep ? ep->res : nullptr; q.y_amax = ep ? ep->y_amax : nullptr;
        q.N = d->N; q.Cin = d->C_in; q.Cout = d->C_out; q.HW = d->H * d->W;
        q.w_io = d->transposed ? 1 : 0;
        q.wscale = desc_wscale(d);
        q.act = ep ? ep->act : 0; q.alpha = ep ? ep->alpha : 0.f; q.gain = ep ? ep->gain : 1.f; q.clamp = ep ? ep->clamp : -1.f;
        tu_conv1x1_fewch(ch.kernel == PASTA_FWD_FEWCIN ? 1 : 2, q, s);
        return launch_status("conv2d");
    }
    float* const ws = (float*)workspace;
    float* const ws_amax = ws;                                        // [2][AMAX_PARTS]: partial |max| of x (second row: spare)
    float* const ws_rowinv = ws + lay.rowinv;                         // [G][Og_pad]: 1 / S_w per packed weight row (PASTA_MATH_F16X3)
    float* const ws_pack = ws + lay.pack;                             // the packed weights

    ConvFwdParams p{};
    p.x = (const float*)x; p.y = (float*)y; p.wp = ws_pack; p.iscale = iscale; p.oscale = oscale;
    p.x_pieces = d->x_layout == PASTA_LAYOUT_PIECES16;
    if (p.x_pieces) {
        PASTA_CHECK(d->x_amax, "conv2d: x_layout = PASTA_LAYOUT_PIECES16 needs x_amax, the row pasta_blur_pieces wrote (the operand's scale)");
        PASTA_CHECK(ch.pieces_ok && !(ep && ep->noise),
                    "conv2d: no kernel takes x_layout = PASTA_LAYOUT_PIECES16 for this launch (pasta_conv2d_plan tells beforehand)");
    }
    p.x2 = (const float*)d->x2; p.C1 = d->C1;
    PASTA_CHECK(!d->x2 || (d->C1 > 0 && d->C1 < d->C_in && d->groups == 1 && !wmod_s), "conv2d: a second input tensor needs 0 < C1 < C_in, one group and plain weights");
    p.N = d->N; p.Cin = d->C_in; p.H = d->H; p.W = d->W;
    p.Cout = d->C_out; p.OH = d->OH; p.OW = d->OW;
    p.G = d->groups; p.Ig = d->C_in / d->groups; p.Og = d->C_out / d->groups;
    const FwdTile tile = ch.tile;
    p.Ig_pad = round_up(p.Ig, fwd_ipad(p.Ig, tile)); p.Og_pad = round_up(p.Og, fwd_tile_bm(tile));
    p.KK = d->kh * d->kw;
    p.bias = ep ? ep->bias : nullptr; p.act = ep ? ep->act : 0; p.res = ep ? (const float*)ep->res : nullptr;
    p.alpha = ep ? ep->alpha : 0.f; p.gain = ep ? ep->gain : 1.f; p.clamp = ep ? ep->clamp : -1.f;
    p.noise = ep ? ep->noise : nullptr; p.noise_strength = ep ? ep->noise_strength : nullptr; p.noise_ps = ep ? ep->noise_per_sample : 0;
    p.y_amax = ep ? ep->y_amax : nullptr;
    if (mask) { p.mask = (const float*)mask->m; p.m_act = mask->act; p.m_alpha = mask->alpha; p.m_gain = mask->gain; p.m_clamp = mask->clamp; }
    p.ksplit = ch.ksplit;
    p.o_tiles = 1;
    p.partial = ws + lay.partial;
    p.bf16x6 = ch.pieces;            // bf16 pieces per operand (16-bit storage: 1, the stored element is the operand); 0 = fp32 kernel
    p.io = d->io_dtype;
    PASTA_CHECK(p.io == IO_F32 || p.bf16x6, "conv2d: no 16-bit-storage kernel for this shape (pasta_conv2d_plan tells beforehand)");
    p.xcd_order = 1;
    const bool f16x3 = p.bf16x6 == NP_F16X3 && p.io == IO_F32;      // the three-product arithmetic on fp32 tensors: operand scales

    // ---- operand scales
    const float wscale = desc_wscale(d);
    if (f16x3) {
        // operand scale of x: partial |max| (the caller's, or one pass here), times max |iscale| when the styles ride in the staging.
        // The weights carry one scale per output row, found by their packing kernel (no |max| of w is passed or cached).
        const float* xa = d->x_amax;
        if (!xa) {          // (never with the pieces layout: checked above)
            if (int e = tensor_amax(x, (int64_t)d->N * d->C_in * d->H * d->W, PASTA_F32, ws_amax, s)) return e;
            xa = ws_amax;
        }
        if (iscale) {
            tu_amax_times(xa, iscale, d->N * d->C_in, ws_amax, s);
            xa = ws_amax;
        }
        p.x_amax = xa;
        p.w_rowinv = ws_rowinv;
        if (p.x2) {                                     // the second operand's maxima: the caller's, or one pass here (second row of ws_amax)
            p.x2_amax = d->x2_amax;
            if (!p.x2_amax) {
                if (int e = tensor_amax(d->x2, (int64_t)d->N * (d->C_in - d->C1) * d->H * d->W, PASTA_F32, ws_amax + AMAX_PARTS, s)) return e;
                p.x2_amax = ws_amax + AMAX_PARTS;
            }
        }
    }

    // ---- pack
    const bool packed = ch.packed;
    int pk_kh = d->kh, pk_kw = d->kw, pk_tr = d->transposed, pk_flip = d->flip;
    if (packed) {
        // K = (input channel, tap) pairs: one pseudo-tap over C_in kh kw "channels" of a zero-padded input (workspace: ... | offsets | copy)
        const int K = p.Ig * d->kh * d->kw;
        const int Hp = d->H + 2 * d->pad_h, Wp = d->W + 2 * d->pad_w;
        unsigned* const koff = (unsigned*)(ws + lay.koff);
        tu_packed_koff(koff, K, d->kh, d->kw, d->flip, Hp * Wp, Wp, s);
        if (d->pad_h || d->pad_w) {
            float* const xp = ws + lay.extra;
            tu_pad_planes((const float*)x, xp, (int64_t)d->N * d->C_in, d->H, d->W, d->pad_h, d->pad_w, s);
            p.x = xp;
        }
        p.koff = koff;
        p.H = Hp; p.W = Wp;
        p.Ig = K; p.Ig_pad = round_up(K, 16); p.KK = 1;
        pk_kh = pk_kw = 1; pk_tr = 0; pk_flip = 0;           // [O][C_in kh kw] as it lies: a 1x1 weight over the K "channels"
    }
    if (d->w_prepacked) {
        // the caller packed the weights for this very descriptor beforehand (pasta_conv2d_pack_pair): the kinds of launch pack_job_of describes
        PASTA_CHECK(f16x3 && !packed && !wmod_s && !p.x2, "conv2d: w_prepacked with a launch pasta_conv2d_pack_pair does not serve");
    } else {   // pack weights (times wscale)
        if (f16x3) {       // two fp16 pieces, one scale per output row found on the way
            tu_pack_weights_f16x3(w, ws_pack, ws_rowinv, p.G, p.Ig, p.Og, p.Ig_pad, p.Og_pad, pk_kh, pk_kw, pk_tr, pk_flip, wscale, wmod_s, wmod_d,
                                  (p.Og_pad & 63) == 0 ? 1 : 0, s);
        }
        else if (p.bf16x6)
            tu_pack_weights_bf16(w, ws_pack, p.G, p.Ig, p.Og, p.Ig_pad, p.Og_pad, pk_kh, pk_kw, pk_tr, pk_flip, wscale, p.io == IO_F16 ? 1 : 0, wmod_s, wmod_d, s);
        else
            tu_pack_weights_f32(w, ws_pack, p.G, p.Ig, p.Og, p.Ig_pad, p.Og_pad, d->kh, d->kw, d->transposed, d->flip, wscale, wmod_s, wmod_d, s);
    }

    // ---- build the lattice, launch
    if (ch.kernel == PASTA_FWD_1X1) {
        tu_conv1x1(p, s);           // conv2d and conv_transpose2d coincide for 1x1 / stride 1 (the packing kernel reads either weight layout)
        return launch_status("conv2d");
    }
    PASTA_CHECK(!p.x2, "conv2d: a second input tensor is served by the pointwise kernel only (1x1, stride 1, fp32 tensors, PASTA_MATH_F16X3, "
                       ">= 16 input and > 32 output channels, planes that divide into 128- / 256-pixel tiles, no scale vectors or noise)");
    TapTable t;
    if (!d->transposed) {
        lattice_conv2d(d, packed, t);
        set_lattice(p, t);
        if (packed) launch_fwd_bf16x6(tile == T128x128, false, p, s);
        else if (ch.kernel == PASTA_FWD_3X3S2) {
            tu_conv3x3s2(p, s);
            return launch_status("conv2d");
        }
        else launch_lattice(ch, p, s);
    } else if (ch.tl == TL_ONEPASS) {
        p.osy = p.osx = d->stride; p.isy = p.isx = 1;
        p.x2 = ws + lay.extra;                            // the gathered column
        tu_conv_t2(p, s);                                 // the whole lattice, remainder row and column included, in one launch
        return launch_status("conv2d");
    } else if (ch.tl == TL_PAIR) {
        launch_transposed_pairs(d, p, tile, s, EdgeWeights{w, wmod_s, wmod_d, wscale, d->flip});
        return launch_status("conv2d");
    } else {
        // the parity classes share a grid (one table of all: class -1), or take one launch each
        const int first = ch.tl == TL_MERGED ? -1 : 0, last = ch.tl == TL_MERGED ? -1 : ch.launches - 1;
        for (int k = first; k <= last; k++) {
            if (int e = lattice_transposed(d, k, t)) return e;
            set_lattice(p, t);
            launch_lattice(ch, p, s);
        }
    }

    // ---- reduce
    if (p.ksplit > 1) tu_splitk_reduce(p, s);
    // y_amax with a launch whose kernel does not take it (fp32 MFMA tiles; K slices: few pixels, thousands of small workgroups in
    // the reduction): one scan of y
    if (p.y_amax && (!p.bf16x6 || p.ksplit > 1) && p.io == IO_F32)
        if (int e = tensor_amax(y, (int64_t)d->N * d->C_out * d->OH * d->OW, PASTA_F32, p.y_amax, s)) return e;
    return launch_status("conv2d");
}

extern "C" int pasta_conv2d_wgrad_plan(const pasta_conv_desc* d, int* kernel) {
    using namespace pasta;
    if (int e = check_desc(d, "conv2d_wgrad_plan")) return e;
    const int k = choose_wgrad(d, 1).kernel;
    if (kernel) *kernel = k;
    if (d->x_layout == PASTA_LAYOUT_PIECES16 && k != PASTA_WGRAD_3X3S2_PIECES)
        return fail("conv2d_wgrad: x_layout = PASTA_LAYOUT_PIECES16 is served by the 3x3 stride-2 weight gradient only (conv2d, pad 0, fp32 dy, PASTA_MATH_F16X3, "
                    "one group, C_in a multiple of 8, output rows of a multiple of 16 pixels)");
    if (d->io_dtype != PASTA_F32 && (k == PASTA_WGRAD_F32 || k == PASTA_WGRAD_SMALLCIN))
        return fail("conv2d_wgrad: no 16-bit-storage kernel for this shape: convert the tensors to fp32 for this launch");
    return 0;
}

extern "C" int64_t pasta_conv2d_wgrad_workspace(const pasta_conv_desc* d) {
    using namespace pasta;
    if (check_desc(d, "conv2d_wgrad_workspace")) return -1;
    return wgrad_workspace(d, choose_wgrad(d, 1), false).total_floats * (int64_t)sizeof(float);
}

extern "C" int64_t pasta_conv2d_wgrad_modulated_workspace(const pasta_conv_desc* d) {
    using namespace pasta;
    if (check_desc(d, "conv2d_wgrad_modulated_workspace")) return -1;
    const WgradChoice c = choose_wgrad(d, d->N);
    if (!wgrad_modulated_ok(d, c)) return -1;
    return wgrad_workspace(d, c, true).total_floats * (int64_t)sizeof(float);
}

extern "C" int pasta_conv2d_wgrad(const void* xv, const void* dyv, float* dw, const pasta_conv_desc* d, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    return pasta::wgrad_run(xv, dyv, dw, d, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr);
}

extern "C" int pasta_conv2d_wgrad_modulated(const void* x, const void* dy, const float* styles, const float* w, float* dw, float* dstyles,
                                            const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace pasta;
    PASTA_CHECK(styles && w && dstyles, "conv2d_wgrad_modulated: null pointer");
    return wgrad_run(x, dy, dw, d, workspace, workspace_bytes, stream, styles, w, dstyles);
}

int pasta::wgrad_run(const void* xv, const void* dyv, float* dw, const pasta_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream,
                     const float* mod_s, const float* mod_w, float* ds) {
    if (int e = check_desc(d, "conv2d_wgrad")) return e;
    const float* x = (const float*)xv; const float* dy = (const float*)dyv;       // elements of d->io_dtype behind these pointers
    PASTA_CHECK(x && dy && dw, "conv2d_wgrad: null pointer");
    const WgradChoice c = choose_wgrad(d, mod_s ? d->N : 1);      // (modulated: never the small-cin kernels -- wgrad_modulated_ok)
    PASTA_CHECK(!mod_s || wgrad_modulated_ok(d, c), "conv2d_wgrad_modulated: this shape has no sample-aligned split kernel (pasta_conv2d_wgrad_modulated_workspace tells beforehand)");
    const WgradWorkspace lay = wgrad_workspace(d, c, mod_s != nullptr);
    const int64_t need = lay.total_floats * (int64_t)sizeof(float);
    PASTA_CHECK(workspace && workspace_bytes >= need, "conv2d_wgrad: workspace of %lld bytes needed, %lld given", (long long)need, (long long)workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int Ig = d->C_in / d->groups, Og = d->C_out / d->groups;
    PASTA_CHECK(((uintptr_t)workspace & 15) == 0, "conv2d_wgrad: workspace must be 16-byte aligned");
    float* const ws_amax = (float*)workspace;                         // [2][AMAX_PARTS]: x, dy
    float* const slab = (float*)workspace + lay.slab;                 // the partial slabs

    const WgradSmallPlan& ws = c.small;
    if (d->x_layout == PASTA_LAYOUT_PIECES16) {
        if (int e = pasta_conv2d_wgrad_plan(d, nullptr)) return e;
        PASTA_CHECK(!mod_s && d->x_amax, "conv2d_wgrad: x_layout = PASTA_LAYOUT_PIECES16 needs x_amax (the row pasta_blur_pieces wrote) and plain weights");
    }
    PASTA_CHECK(d->io_dtype == PASTA_F32 || c.kernel == PASTA_WGRAD_FEWCIN || wgrad_split(c.kernel), "conv2d_wgrad: no 16-bit-storage kernel for this shape (pasta_conv2d_wgrad_plan tells beforehand)");
    if (c.kernel == PASTA_WGRAD_FEWCIN) {
        const int fks = c.fewcin_ks;
        // few input channels, 1x1: one bandwidth-bound pass over dy with plain FMAs (conv_wgrad_f32.h)
        const int64_t total = (int64_t)d->N * ((int64_t)d->H * d->W / 4);
        const int64_t per = (total + fks - 1) / fks;
        const int a_pad = ws.a_tiles * 64, bpad = ws.nb * 32;
        const dim3 grid((unsigned)fks, (unsigned)((d->C_out + 7) / 8));
        tu_wgrad1x1_fewcin(d->C_in, d->io_dtype, grid, dy, x, slab, d->N, d->C_out, d->H * d->W, per, a_pad, bpad, s);
        tu_wgrad_smallcin_reduce(slab, dw, fks, d->C_out, ws.bprime, a_pad, bpad, desc_wscale(d), s);
        return launch_status("conv2d_wgrad(few-channel 1x1)");
    }
    if (c.kernel == PASTA_WGRAD_SMALLCIN) {
        WgradSmallParams q;
        q.S = dy; q.L = x; q.slab = slab;
        q.N = d->N; q.Ag = d->C_out; q.P = d->OH; q.Q = d->OW; q.Bg = Ig; q.LH = d->H; q.LW = d->W;
        q.kh = d->kh; q.kw = d->kw; q.pad_h = d->pad_h; q.pad_w = d->pad_w;
        q.bprime = ws.bprime; q.nb = ws.nb; q.cw_log2 = ws.cw_log2; q.rows_total = ws.rows_total; q.qblocks = ws.qblocks;
        q.chunks_total = ws.chunks_total; q.ksplit = ws.ksplit; q.a_tiles = ws.a_tiles;
        PASTA_CHECK(ws.lds_bytes <= 64 * 1024, "conv2d_wgrad: small-cin LDS footprint %zu too large", ws.lds_bytes);
        tu_wgrad_smallcin(q, ws.a_tiles * ws.ksplit, ws.lds_bytes, s);
        tu_wgrad_smallcin_reduce(slab, dw, ws.ksplit, d->C_out, ws.bprime, ws.a_tiles * 64, ws.nb * 32, desc_wscale(d), s);
        return launch_status("conv2d_wgrad(small-cin)");
    }

    WgradParams p;
    p.slab = slab;
    p.io = d->io_dtype;
    p.G = d->groups; p.kh = d->kh; p.kw = d->kw; p.st = d->stride; p.pad_h = d->pad_h; p.pad_w = d->pad_w;
    p.N = d->N;
    if (!d->transposed) {   // dw[o][i]: S = dy, L = x
        p.S = dy; p.SC = d->C_out; p.P = d->OH; p.Q = d->OW; p.Ag = Og;
        p.L = x;  p.LC = d->C_in;  p.LH = d->H; p.LW = d->W; p.Bg = Ig;
    } else {                // dw[i][o]: S = x, L = dy
        p.S = x;  p.SC = d->C_in;  p.P = d->H; p.Q = d->W; p.Ag = Ig;
        p.L = dy; p.LC = d->C_out; p.LH = d->OH; p.LW = d->OW; p.Bg = Og;
    }
    const WgradPlan& w = c.w;
    p.cw_log2 = w.cw_log2; p.rows_total = w.rows_total; p.qblocks = w.qblocks; p.chunks_total = w.chunks_total;
    p.ksplit = w.ksplit; p.a_tiles = w.a_tiles; p.b_tiles = w.b_tiles; p.tap_groups_r = w.tgr; p.tap_groups_s = w.tgs;
    // measured (profiles/r3_ab_wgrad_xcd.txt): 256 -> 128 at 128^2 298.6 -> 303.4 TFLOP/s, stride 2 at 256^2 143 -> 154, at 257^2 140.7 -> 143.4,
    // every other shape within 0.5 %
    p.xcd_order = 1;
    p.l_pieces = d->x_layout == PASTA_LAYOUT_PIECES16;
    PASTA_CHECK((int64_t)w.chunks_total * (w.ksplit + 1) < (1ll << 32), "conv2d_wgrad: %d chunks x %d K slices overflow the kernels' 32-bit slice bounds", w.chunks_total, w.ksplit);
    PASTA_CHECK(w.lds_bytes <= 160 * 1024, "conv2d_wgrad: LDS footprint %zu too large", w.lds_bytes);
    PASTA_CHECK(w.npos <= 256, "conv2d_wgrad: halo of %d positions per chunk is not supported", w.npos);

    const int64_t blocks = (int64_t)p.G * w.a_tiles * w.b_tiles * w.tgr * w.tgs * w.ksplit;
    PASTA_CHECK(blocks <= INT32_MAX, "conv2d_wgrad: grid too large");
    const int np = p.io != IO_F32 ? 1 : math_pieces(d->math);          // bf16 pieces per operand of the split-bf16 kernels (NP_F16X3: fp16 pieces)
    p.s_amax = p.l_amax = nullptr;
    if (np == NP_F16X3 && wgrad_split(c.kernel)) {
        const float* xa = d->x_amax; const float* ya = d->dy_amax;
        if (!xa) { if (int e = tensor_amax(x, (int64_t)d->N * d->C_in * d->H * d->W, PASTA_F32, ws_amax, s)) return e; xa = ws_amax; }      // (pieces layout: given, checked above)
        if (!ya) { if (int e = tensor_amax(dy, (int64_t)d->N * d->C_out * d->OH * d->OW, PASTA_F32, ws_amax + AMAX_PARTS, s)) return e; ya = ws_amax + AMAX_PARTS; }
        p.s_amax = d->transposed ? xa : ya;
        p.l_amax = d->transposed ? ya : xa;
    }
    if (c.kernel == PASTA_WGRAD_3X3) tu_wgrad3x3(np, p, blocks, s);
    else if (c.kernel == PASTA_WGRAD_3X3S2 || c.kernel == PASTA_WGRAD_3X3S2_PIECES) tu_wgrad3x3s2(np, p, blocks, s);
    else if (c.kernel == PASTA_WGRAD_1X1) tu_wgrad1x1(np, w.WA, p, blocks, s);
    else if (int e = tu_wgrad_f32(w.TR, w.TS, w.WA, w.pipe, w.kp, p, blocks, w.lds_bytes, s)) return e;
    const int Ap = w.a_tiles * 64 * w.WA, Bp = w.b_tiles * 64 * w.WB;
    if (mod_s) {
        // slices [n m, (n + 1) m) hold sample n's gradient with respect to the modulated weight: dw = sum_n s[n, i] (.), ds[n, i] = sum_{o, taps} w (.)
        float* const dsp = (float*)workspace + lay.ds_partial;
        const int wg_rows = wgrad_mod_rows(Ap, Bp, p.kh * p.kw);
        const dim3 grid((unsigned)(Bp / 64), (unsigned)(Ap / wg_rows), (unsigned)(p.kh * p.kw));
        tu_wgrad_reduce_modulated(d->transposed != 0, grid, slab, mod_s, mod_w, dw, dsp, w.ksplit, d->N, p.Ag, p.Bg, Ap, Bp, p.kh, p.kw, d->flip, desc_wscale(d), wg_rows, s);
        tu_sum_blocks(dsp, ds, wgrad_modulated_blocks(d, w), d->N * d->C_in, s);
        return launch_status("conv2d_wgrad_modulated");
    }
    tu_wgrad_reduce(slab, dw, w.ksplit, p.G, p.Ag, p.Bg, Ap, Bp, p.kh, p.kw, d->flip, desc_wscale(d), s);
    return launch_status("conv2d_wgrad");
}
