// Shared declarations of the convolution family: what the kernel headers and the launches of conv_igemm.hip have in common.  The constants the
// kernels share with the planner (MAX_TAPS, NP_F16X3, AMAX_PARTS, FwdTile, wgrad_chunks, ...) are in conv_plan.h, plain C++.
#pragma once
#include <type_traits>
#include "common.h"
#include "conv_plan.h"
#include <stdlib.h>
#include <string.h>

namespace pasta {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // sixteen bytes in registers (HIP's uint4 is a struct: arrays of it handed to a lambda end up in scratch)

// An empty asm that makes a VGPR value opaque to the SLP vectoriser (no instruction is emitted).
#define PASTA_KEEP_SCALAR(x) asm("" : "+v"(x))
// every component of a 16-byte vector counts as used: a partly used LDS read stays one ds_read_b128
#define PASTA_KEEP_WHOLE(q) asm("" : "+v"((q).x), "+v"((q).y), "+v"((q).z), "+v"((q).w))

__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// bias + activation + gain + clamp of one output element (forward semantics of bias_act.cu:38-146, act 1..3)
__device__ __forceinline__ float conv_epilogue(float v, float b, int act, float alpha, float gain, float clamp) {
    v += b;
    if (act == 2) v = v > 0.f ? v : 0.f;
    else if (act == 3) v = v > 0.f ? v : v * alpha;
    v *= gain;
    if (clamp >= 0.f) v = (v > -clamp && v < clamp) ? v : (v >= 0.f ? clamp : -clamp);
    return v;
}

// The same without a branch: the store loops of the kernels run sixty-four of these per lane, and with three or four wave-uniform
// scalar branches per element (the compiler does not unswitch them) they cost the dominant kernel 5 % -- profiles/r4_ab_epilogues.txt.
// "No activation" is expressed by the caller as b = 0, slope = 1, relu = false, gain = 1, clamp_on = false (EpiAct below): the value then
// passes unchanged (NaN and infinities included).  relu selects an exact 0 for v <= 0 and for NaN, as conv_epilogue does.
struct EpiAct {
    float slope, gain, clamp; bool relu, clamp_on, on;
    // the input-activation mask of an input-gradient launch (pasta_act_mask, conv_epi_input_mask below): the store multiplies by the
    // derivative of the activation that PRODUCED this launch's output position, read from that activation's output
    bool mask; int m_act; float m_alpha, m_gain, m_clamp;
};
__device__ __forceinline__ EpiAct conv_epi_act(int act, float alpha, float gain, float clamp, bool fused) {
    EpiAct e;
    e.on = act != 0 && fused;
    e.slope = (e.on && act == 3) ? alpha : 1.f;
    e.relu = e.on && act == 2;
    e.gain = e.on ? gain : 1.f;
    e.clamp_on = e.on && clamp >= 0.f;
    e.clamp = clamp;
    e.mask = false; e.m_act = 1; e.m_alpha = 0.f; e.m_gain = 1.f; e.m_clamp = -1.f;
    return e;
}
__device__ __forceinline__ float conv_epilogue_u(float v, float b, const EpiAct& e) {
    v += b;
    const float neg = e.relu ? 0.f : v * e.slope;              // selects on wave-uniform values, not branches
    v = v > 0.f ? v : neg;
    v *= e.gain;
    const bool in = (v > -e.clamp && v < e.clamp) || !e.clamp_on;
    return in ? v : (v >= 0.f ? e.clamp : -e.clamp);
}
// The store loops are instantiated per case and chosen ONCE per workgroup.  SPEC kernels (the default arithmetic, 16-bit storage, the fp32
// tiles: what the training and inference steps run) get an instance per (whole tile of output rows?, no activation | activation | activation
// + clamp) -- with the activation's wave-uniform tests resolved at compile time the loop is 1.5 ms per training step faster than the
// branch-free folded form above (profiles/r4_ab_epilogues.txt) --; the other arithmetics keep ONE loop with the row test per element and
// the folded form (compile time: an instance is sixty-four unrolled stores, and those arithmetics are side lines).  Round 4 folded every
// kernel because the family was one translation unit that took 12 minutes with the instances; since round 5 the family is thirteen units
// compiled in parallel (conv_launch.h).  f(full, EpiCase<MODE>{}): full is std::bool_constant for SPEC kernels, bool otherwise.
template <int MODE> struct EpiCase {};          // 0: folded, branch-free (conv_epilogue_u); 1: no activation; 2: activation; 3: activation and clamp;
                                                // 4: the input-activation mask (no bias / activation of the launch's own: conv_store_subtile)
template <int MODE>
__device__ __forceinline__ float conv_epilogue_c(float v, float b, const EpiAct& e, EpiCase<MODE>) {
    if constexpr (MODE == 0) return conv_epilogue_u(v, b, e);
    else if constexpr (MODE == 1) return v;
    else {
        v += b;
        const float neg = e.relu ? 0.f : v * e.slope;          // a select on a wave-uniform value, not a branch (relu: an exact 0 for v <= 0 and for NaN)
        v = v > 0.f ? v : neg;
        v *= e.gain;
        if constexpr (MODE == 3) v = (v > -e.clamp && v < e.clamp) ? v : (v >= 0.f ? e.clamp : -e.clamp);
        return v;
    }
}
#ifndef PASTA_EPI_CASES
#define PASTA_EPI_CASES 1       // build switch for same-box A/B (tools/ab_lib.sh): 0 = round 4's final form, an instance per whole-tile answer with the folded activation
#endif
// MASK: the kernel also carries the instance of the input-activation mask (the default arithmetic on fp32 tensors of the 2-D tiles: what
// mask_launch_ok of conv_plan.h admits); every other kernel compiles what it always did.
template <bool SPEC, bool MASK = false, class F>
__device__ __forceinline__ void conv_epilogue_dispatch(bool full, const EpiAct& e, F&& f) {
    if constexpr (SPEC && MASK) {
        if (e.mask) {
            if (full) f(std::true_type{}, EpiCase<4>{}); else f(std::false_type{}, EpiCase<4>{});
            return;
        }
    }
    if constexpr (SPEC && !PASTA_EPI_CASES) {
        if (full) f(std::true_type{}, EpiCase<0>{}); else f(std::false_type{}, EpiCase<0>{});
    } else if constexpr (SPEC) {
        if (full) {
            if (!e.on) f(std::true_type{}, EpiCase<1>{}); else if (!e.clamp_on) f(std::true_type{}, EpiCase<2>{}); else f(std::true_type{}, EpiCase<3>{});
        } else {
            if (!e.on) f(std::false_type{}, EpiCase<1>{}); else if (!e.clamp_on) f(std::false_type{}, EpiCase<2>{}); else f(std::false_type{}, EpiCase<3>{});
        }
    } else {
        f(full, EpiCase<0>{});
    }
}

//------------------------------------------------------------------------------------
// Storage type of the activations (x, y, dy) of the split-bf16 kernel family.  IO_F32: fp32 tensors, split into bf16 pieces
// by the staging code.  IO_BF16 / IO_F16: 16-bit tensors in HBM (BASELINE config 5; the fp16 discriminator blocks of the
// reference, networks.py:1107-1120): the element IS the matrix-core operand, one product per multiply-add on
// v_mfma_f32_32x32x16_bf16 / _f16, fp32 accumulation, fp32 epilogue, result rounded once on the way out.  Weights and
// weight gradients stay fp32 in HBM (master copies); the packing kernel rounds the weights to the operand type.
enum { IO_F32 = 0, IO_F16 = 1, IO_BF16 = 3 };          // = the PASTA_F32 / PASTA_F16 / PASTA_BF16 dtype codes

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

template <int IO> struct io_size { static constexpr int value = IO == IO_F32 ? 4 : 2; };

// one element at BYTE offset `off` of `base`, as fp32
template <int IO> __device__ __forceinline__ float io_ld(const char* base, unsigned off) {
    if constexpr (IO == IO_F32) return *(const float*)(base + off);
    else if constexpr (IO == IO_BF16) return __builtin_bit_cast(float, (uint32_t)(*(const uint16_t*)(base + off)) << 16);
    else return (float)(*(const _Float16*)(base + off));
}
// four consecutive elements starting at element pointer `p` (naturally aligned to the four-pack), as fp32
template <int IO> __device__ __forceinline__ float4 io_ld4(const void* p) {
    if constexpr (IO == IO_F32) return *(const float4*)p;
    else {
        const uint2 r = *(const uint2*)p;
        if constexpr (IO == IO_BF16)
            return make_float4(__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.x & 0xffff0000u),
                               __builtin_bit_cast(float, r.y << 16), __builtin_bit_cast(float, r.y & 0xffff0000u));
        else {
            typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
            const f16x4 h = __builtin_bit_cast(f16x4, r);
            return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        }
    }
}
template <int IO> __device__ __forceinline__ float io_ld1(const void* p) {
    if constexpr (IO == IO_F32) return *(const float*)p;
    else if constexpr (IO == IO_BF16) return __builtin_bit_cast(float, (uint32_t)(*(const uint16_t*)p) << 16);
    else return (float)(*(const _Float16*)p);
}
// store fp32 `v` as element `idx` of `base`
template <int IO> __device__ __forceinline__ void io_st(void* base, int64_t idx, float v) {
    if constexpr (IO == IO_F32) ((float*)base)[idx] = v;
    else if constexpr (IO == IO_BF16) ((__bf16*)base)[idx] = (__bf16)v;
    else ((_Float16*)base)[idx] = (_Float16)v;
}
// two fp32 values -> one dword of two matrix-core operand elements (bf16 for fp32 / bf16 storage, f16 for f16 storage)
template <int IO> __device__ __forceinline__ uint32_t io_pack2(float a, float b) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ v = {a, b};
    if constexpr (IO == IO_F16) {
        typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_));
    } else {
        typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_));
    }
}
// acc += A * B on the matrix cores, operands given as eight packed 16-bit elements
template <int IO> __device__ __forceinline__ f32x16 io_mfma(bf16x8_t a, bf16x8_t b, f32x16 acc) {
    if constexpr (IO == IO_F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

//------------------------------------------------------------------------------------
// PASTA_MATH_F16X3: fp32-equivalent products from THREE fp16 matrix-core products (v_mfma_f32_32x32x16_f16).
//
// An fp32 operand v is scaled by a power of two S chosen from the largest magnitude of its tensor (amax * S in [2^13, 2^14):
// exact, no overflow) and written as   v S = h + r,  h = fp16(v S)  (round to nearest, 11 significand bits),  r exact in fp32,
// |r| <= 2^-11 |v S|.  The residual is kept as  l' = fp16(2^11 r)  ("pre-scaled low piece": the same magnitude as h, so it is a
// NORMAL fp16 number wherever h is, and |r - 2^-11 l'| <= 2^-23 |v S| thanks to its own sign).  h h, h l' and l' h are
// exact in fp32 (11 x 11 bits), so with a third piece  h'' = h 2^-11  (an exponent shift) on the OTHER operand
//     a b S_a S_b = h_a h_b + h''_a l'_b + l_a h_b          (+ l_a l_b, dropped: <= 2^-22 |a b|)
// is three MFMAs into ONE fp32 accumulator set; the epilogue multiplies by 1 / (S_a S_b) (exact).  Representation error
// per operand <= 2^-23 relative (rms 4e-8; fp32's own rounding is 2^-24), i.e. the products are fp32-class, and the fp32
// accumulation error (measured rms 3 - 8e-7 at K = 2304) dominates as it does for an fp32 FMA chain.
// Pieces by index: 0 = h, 1 = low piece, 2 = h''.
//   forward-type kernels: A = weights (packed once per launch: h, l = fp16(r) unscaled, h'' = h 2^-11), B = activations staged as
//       (h, l'): TWO pieces, two thirds of the split-bf16 staging and LDS traffic.  Products (A,B): (0,0) (2,1) (1,0).
//       Round 4, measured and dropped (profiles/r4_ab_hpp_in_registers.txt, same-box A/B of two source trees under rocprofv3):
//       forming h'' in registers from the h fragment (four v_pk_mul_f16 per fragment) instead of packing, staging and reading it
//       -- a third of the weight stream, of its LDS stores and of its fragment reads gone: the eight-wave 2-D tile 290.9 -> 290.1 us
//       per launch (nothing), the four-wave 64 x 256 tile 294 -> 329 us (11 % SLOWER), the base kernel 121 -> 125 us: eight more
//       VALU instructions per step and wave next to the MFMAs cost what the LDS bytes saved, and more where a wave also stages
//       three units per chunk.
//       The weight scale is PER OUTPUT ROW of the GEMM (round 4): the packing kernel takes the largest magnitude of each
//       output channel's weights (after wscale and, for per-sample weights, after the modulation) itself, so no |max| of w is
//       passed in or cached anywhere, and a row's elements keep full precision down to 2^-16 of THEIR ROW's largest (below
//       that the unscaled l leaves fp16's normal range and an element keeps 11..22 bits: absolute error <= 2^-28 of the row's
//       amax per term).  The epilogue multiplies row o by 1 / (S_x S_w[o]) (p.w_rowinv).  Activations keep full precision
//       down to 2^-28 of their tensor's largest element.
//   weight-gradient kernels: both operands are activations and symmetric, so the exponent-shift trick buys nothing there (h'' of
//       EITHER operand leaves fp16's normal range below 2^-16 of its tensor's largest element, whichever way the low pieces are
//       scaled): each operand is (h, l = fp16(r)), TWO pieces, products (S,L): (0,0) (0,1) (1,0) -- full precision for elements
//       within 2^-17 of their tensor's largest, absolute error <= 2^-39 amax per element below that.
// Scales: the tensor's |max| arrives as 256 partial maxima (pasta_tensor_amax: one pass at HBM rate, non-finite elements
// skipped so that an inf / NaN stays local); every wave reduces them itself (one 16-byte load per lane) -- no finalising
// launch, no atomics, no host round trip.
// (NP_F16X3, the pseudo piece count of the template parameter NP, and AMAX_PARTS, the partial maxima per tensor: conv_plan.h)

template <int NP> struct Arith {
    static constexpr bool f16x3 = NP == NP_F16X3;
    static constexpr int npa = f16x3 ? 3 : NP;          // A pieces in LDS
    static constexpr int npb = f16x3 ? 2 : NP;          // B pieces in LDS (forward-type kernels)
    static constexpr int npw = f16x3 ? 2 : NP;          // pieces of either operand in the weight-gradient kernels
};
// is the product (A piece pa) x (B piece pb) part of the arithmetic?  forward-type kernels
template <int NP> __host__ __device__ constexpr bool mm_on(int pa, int pb) {
    return NP == NP_F16X3 ? ((pa == 0 && pb == 0) || (pa == 2 && pb == 1) || (pa == 1 && pb == 0)) : (pa + pb < NP);
}
// ... weight-gradient kernels (S piece pa, L piece pb)
template <int NP> __host__ __device__ constexpr bool mmw_on(int pa, int pb) {
    return NP == NP_F16X3 ? (pa + pb < 2) : (pa + pb < NP);
}
// the matrix-core instruction of an arithmetic / storage type
template <int IO, int NP> __device__ __forceinline__ f32x16 mfma16(bf16x8_t a, bf16x8_t b, f32x16 acc) {
    if constexpr (IO == IO_F16 || NP == NP_F16X3) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// S (power of two) and 1 / S for a tensor whose largest finite magnitude is amax: amax S in [2^13, 2^14); amax == 0 or
// subnormal: S = 2^120.  Exponent fields stay in [7, 247], so S, 1 / S and every v S are normal or exactly zero.
__host__ __device__ __forceinline__ void scale_from_amax(float amax, float& S, float& invS) {
    const uint32_t eb = __builtin_bit_cast(uint32_t, amax) >> 23;          // amax >= 0
    int field = 267 - (int)eb;                                             // 127 + 14 - (eb - 126)
    field = field < 7 ? 7 : field > 247 ? 247 : field;
    S = __builtin_bit_cast(float, (uint32_t)field << 23);
    invS = __builtin_bit_cast(float, (uint32_t)(254 - field) << 23);
}
// the largest of the AMAX_PARTS partial maxima at `parts`, computed redundantly by every wave (wave-uniform result)
__device__ __forceinline__ float amax_of_parts(const float* __restrict__ parts) {
    const float4 v = ((const float4*)parts)[threadIdx.x & 63];
    float m = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, m)));
}
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// two scaled fp32 values -> h (packed fp16 pair) and the pre-scaled low piece l' = fp16(2^11 (v - h))
__device__ __forceinline__ void f16_split2(float v0, float v1, uint32_t& h, uint32_t& lp) {
    const f16x2_t hh = __builtin_convertvector(f32x2_t{v0, v1}, f16x2_t);
    h = __builtin_bit_cast(uint32_t, hh);
    float r0 = v0 - (float)hh[0], r1 = v1 - (float)hh[1];
    PASTA_KEEP_SCALAR(r0);
    lp = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{r0 * 2048.f, r1 * 2048.f}, f16x2_t));
}
// ... and with the low piece left unscaled: l = fp16(v - h) (weight-gradient kernels)
__device__ __forceinline__ void f16_split2_direct(float v0, float v1, uint32_t& h, uint32_t& l) {
    const f16x2_t hh = __builtin_convertvector(f32x2_t{v0, v1}, f16x2_t);
    h = __builtin_bit_cast(uint32_t, hh);
    float r0 = v0 - (float)hh[0], r1 = v1 - (float)hh[1];
    PASTA_KEEP_SCALAR(r0);
    l = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{r0, r1}, f16x2_t));
}
// AMAX_PARTS partial |max| of a contiguous tensor (amax.hip)
int tensor_amax(const void* x, int64_t numel, int dtype, float* parts, hipStream_t s);

// accumulator -> output value: demodulation scale and noise as mod_bias_act_kernel rounds them (fma(acc, d, noise * strength)),
// residual, then bias / activation / gain / clamp.  d = 1 and nz = 0 leave the accumulator bit-identical.
__device__ __forceinline__ float conv_scale_noise(float v, const float* osb, int o, float nz) {
    return osb ? fmaf(v, osb[o], nz) : v + nz;
}

//------------------------------------------------------------------------------------
// The epilogue of the forward-type kernels, registers -> NCHW: rows of a 32 x 32 accumulator sub-tile are output channels, lanes are pixels.
// Every kernel keeps where its pixels lie (and its `for b` / `for a` loops); what happens to a sub-tile on the way out is here, once.
// Two kernels keep a block of their own, measured: conv_fwd_kernel (conv_fwd_f32.h; through these functions three of its instances ran 15 - 32 %
// faster and <64,256,2,2,4,1> 2.3 % slower, twice) and conv3x3s2_f16x3_kernel (conv_fwd_s2.h) -- profiles/epilogue_single_source_ab.txt.

// Back to the operands' units (PASTA_MATH_F16X3): row o of every accumulator set handed in times `scale` (1 / S_x of the tile) times wri[o]
// (1 / S_w of the weight row, p.w_rowinv, written by the packing kernel; wri points at the tile's first row).  The 16 x WMT row scales of this
// lane are fetched in one go in front of the multiplies (a load in front of every store cost 9 % of the kernel); the pair mode of the row
// kernel hands in both of its sets, which share them.
template <int WMT, int WNT, class... Acc>
__device__ __forceinline__ void conv_unscale_rows(const float* wri, float scale, int wm, int lane, Acc&... accs) {
    float ws[WMT][16];
#pragma unroll
    for (int a = 0; a < WMT; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) ws[a][r] = wri[(wm * WMT + a) * 32 + acc_row(r, lane)];
#pragma unroll
    for (int a = 0; a < WMT; a++)
#pragma unroll
        for (int b = 0; b < WNT; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) ((accs[a][b][r] = (accs[a][b][r] * scale) * ws[a][r]), ...);
}

// What one lane's pixel (column b of the wave's sub-tiles) brings to the epilogue.  Element (row o of the group, this pixel) of y, res and
// partial lies at off + o * ostride; oscale and bias are indexed by o.  An operand that is absent is a null pointer.
struct EpiColumn {
    void* y; const void* res;           // elements of the kernel's storage type
    const void* mask;                   // the input-activation mask's tensor (EpiCase<4>), laid out like y
    float* partial;                     // K slices: this slice's fp32 partial sums; the sub-tile is written there and nothing else happens
    int64_t off, ostride;
    const float* oscale;                // this pixel's sample
    const float* bias;
    float nz; bool has_noise;           // noise * strength of this pixel (0 without noise)
};

// One 32 x 32 sub-tile (rows o0 + acc_row(r, lane) of a group of Og) from registers to memory: output scale with noise (as mod_bias_act_kernel
// rounds them: fma(acc, d, noise * strength)) or noise alone, residual, (K slices: the partial sums, and out), bias, then the sixteen stores.
// What the stores need from memory is fetched in front of them, sixteen loads in a row and then their use (a load in front of every store
// serialises on the memory counter: the input-gradient launches that carry another consumer's gradient as residual ran 4 % SLOWER than launch
// + torch addition that way, profiles/r4_ab_grad_join.txt), and ONE operand kind at a time through the same sixteen registers: output scale,
// residual and bias in arrays of their own spill next to the sixty-four accumulators and the store addresses on the three-workgroup tiles.
// full / case_c: what conv_epilogue_dispatch hands its callable.  y_am: the lane's running |max| of y for amax_commit.  RES_ROWTEST (EPI_RES_ROWTEST at the call): the residual keeps its row test in whole tiles too -- the
// base kernel's 16-bit instances take 3 - 19 more VGPRs than they had with sixteen unconditional loads in flight (the note at the end of
// profiles/epilogue_single_source_resources.txt).
constexpr bool EPI_RES_ROWTEST = true;
template <int IO, bool RES_ROWTEST = false, class Full, int MODE>
__device__ __forceinline__ void conv_store_subtile(f32x16& acc, const EpiColumn& c, int o0, int Og, int lane, const EpiAct& ea, uint32_t& y_am,
                                                   Full full, EpiCase<MODE> case_c) {
    const bool FULL = full;
    constexpr unsigned ES = io_size<IO>::value;
    float tv[16];
    if (c.oscale) {
#pragma unroll
        for (int r = 0; r < 16; r++) { const int o = o0 + acc_row(r, lane); tv[r] = c.oscale[(FULL || o < Og) ? o : Og - 1]; }
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = fmaf(acc[r], tv[r], c.nz);
    } else if (c.has_noise) {
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] += c.nz;
    }
    if (c.res) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = o0 + acc_row(r, lane);
            tv[r] = ((FULL && !RES_ROWTEST) || o < Og) ? io_ld1<IO>((const char*)c.res + (c.off + (int64_t)o * c.ostride) * ES) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] += tv[r];
    }
    if constexpr (MODE == 4) {
        // the input-activation mask: (acc [+ res]) times the derivative of the activation whose output lies at c.mask, the residual's access
        // pattern once more through the same sixteen registers (a masked launch has no K slices, no bias and no activation of its own)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = o0 + acc_row(r, lane);
            tv[r] = ((FULL && !RES_ROWTEST) || o < Og) ? io_ld1<IO>((const char*)c.mask + (c.off + (int64_t)o * c.ostride) * ES) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = o0 + acc_row(r, lane);
            const float v = act_grad1<float>(acc[r], tv[r], ea.m_act, ea.m_alpha, ea.m_gain, ea.m_gain, ea.m_clamp);
            if (FULL || o < Og) { io_st<IO>(c.y, c.off + (int64_t)o * c.ostride, v); amax_take(y_am, v); }
        }
        return;
    }
    if (c.partial) {                    // scale, residual, bias, activation ride in the reduction
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = o0 + acc_row(r, lane);
            if (FULL || o < Og) c.partial[c.off + (int64_t)o * c.ostride] = acc[r];
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; r++) { const int o = o0 + acc_row(r, lane); tv[r] = c.bias ? c.bias[(FULL || o < Og) ? o : Og - 1] : 0.f; }
    // instantiated per (activation, clamp, whole tile of rows): no wave-uniform branch per element (conv_epilogue_dispatch)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = o0 + acc_row(r, lane);
        const float v = conv_epilogue_c(acc[r], tv[r], ea, case_c);
        if (FULL || o < Og) { io_st<IO>(c.y, c.off + (int64_t)o * c.ostride, v); amax_take(y_am, v); }
    }
}

// Parameters of the forward-type kernels (conv2d, conv_transpose2d and both input gradients).
// One packing job of pack_weights_f16x3_(pair_)kernel: where the packed rows and their scales go, and how the weight tensor is read
struct PackJob {
    void* wp; float* rowinv;
    int G, Ig, Og, Ig_pad, Og_pad, kh, kw, transposed, flip, pack_xcd_rows;
    float wscale;
};

struct ConvFwdParams {
    const float* x; const float* wp; float* y;         // x, y (and res): elements of type `io` behind these pointers
    const float* iscale; const float* oscale;
    const float* x_amax;                                // PASTA_MATH_F16X3: AMAX_PARTS partial |max| of x
    const float* x2; const float* x2_amax; int C1;      // conv1x1_f16x3_kernel: channels [C1, Cin) live in a second tensor x2 ([N, Cin - C1, H, W]); null = one tensor
    const float* w_rowinv;                              // PASTA_MATH_F16X3: [G][Og_pad] 1 / S_w of every packed weight row (pack_weights_f16x3_kernel)
    float* y_amax;                                      // optional (fused epilogue): zeroed partial |max| slots of y (common.h, amax_commit)
    int io;                                             // IO_F32 / IO_F16 / IO_BF16
    int N, Cin, H, W;
    int Cout, OH, OW;
    int G, Ig, Og, Ig_pad, Og_pad, KK;   // KK = kh*kw slabs per group in wp
    int P, Q;                             // lattice extent
    int oy0, ox0, osy, osx;               // output pixel = (oy0 + p*osy, ox0 + q*osx)
    int isy, isx;                         // input base   = (p*isy, q*isx)
    int T;                                // taps of this lattice
    int ksplit;                           // > 1: K is cut into slices, partial sums go to `partial`
    float* partial;                       // [ksplit][N*Cout*OH*OW] when ksplit > 1
    int o_tiles;                          // output-channel tiles (blockIdx.y = ks * o_tiles + tile)
    int bf16x6;                           // weights packed as split-bf16 pieces, run conv_fwd_bf16x6_kernel
    const float* bias;                    // fused epilogue (pasta_conv_epilogue); act == 0: none
    const float* res;                     // [N, Cout, OH, OW] added before bias / activation, or null
    const float* noise;                   // [OH*OW] or [N][OH*OW] fp32, times noise_strength[0], added after the output scale (SynthesisLayer), or null
    const float* noise_strength;
    int noise_ps;                         // noise is per sample
    int act;
    float alpha, gain, clamp;
    int tap_dy[MAX_TAPS], tap_dx[MAX_TAPS], tap_slab[MAX_TAPS];     // int so that a wave-uniform index reads them with s_load_dword
    // conv_fwd_bf16x6_kernel reads its lattice from here: ncls lattices (the output parity classes of a stride-2
    // conv_transpose2d, else one) share a grid; class c owns taps [tap0, tap0 + T) of the tables above.
    int ncls;
    struct Lattice { int P, Q, oy0, ox0, T, tap0; } cls[4];
    // conv_fwd_rows_bf16x6_kernel (3-wide stride-1 lattices): smallest horizontal tap offset, and whether the three
    // taps of a kernel row are stored with descending offsets (input-gradient launches)
    int rows, rows_d0, rows_rev;
    int rows_y0;                          // conv_fwd_rows2d_bf16x6_kernel: smallest vertical tap offset
    // parity-pair mode of the row-reuse kernel (stride-2 conv_transpose2d): B-image offset of tap c, and whether the
    // two-tap column (taps 0 and 2) is the odd output column
    int pair_off[3], pair_bx;
    // packed-K mode of conv_fwd_bf16x6_kernel (few input channels): "channel" k of the K loop is (input channel, tap) and lives
    // koff[k] bytes behind the pixel's base address in a zero-padded copy of the input; null = off
    const unsigned* koff;
    int xcd_order;                        // conv_fwd_rows2d_bf16x6_kernel, eight-wave tile: consecutive pixel tiles on ONE XCD (0: off)
    int x_pieces;                         // conv3x3s2_f16x3_kernel: x is PASTA_LAYOUT_PIECES16 (pieces.hip), p.x_amax the producer's bound row
    // the input-activation mask (pasta_act_mask; the 2-D tiles, no K slices): [N, Cout, OH, OW] like y, null = off
    const float* mask; int m_act; float m_alpha, m_gain, m_clamp;
};

// ea for a launch that may carry the input-activation mask (the kernels whose conv_epilogue_dispatch has MASK set call this)
__device__ __forceinline__ void conv_epi_input_mask(EpiAct& e, const ConvFwdParams& p) {
    e.mask = p.mask && p.ksplit == 1;
    e.m_act = p.m_act; e.m_alpha = p.m_alpha; e.m_gain = p.m_gain; e.m_clamp = p.m_clamp;
}

// The column of the pixel at plane offset plane_off of sample n, for group g and K slice ks of a launch: every operand the launch carries
// (output scale, noise, residual, bias and activation exist only without K slices: they ride in the reduction otherwise).
// nstr: p.noise_strength[0], read once per kernel.
__device__ __forceinline__ EpiColumn conv_epi_column(const ConvFwdParams& p, const EpiAct& ea, int g, int ks, int n, int plane_off, float nstr) {
    const int OHW = p.OH * p.OW;
    const bool fused = p.ksplit == 1;
    EpiColumn c;
    c.y = p.y;
    c.res = fused ? p.res : nullptr;
    c.mask = ea.mask ? p.mask : nullptr;
    c.partial = fused ? nullptr : p.partial + (int64_t)ks * p.N * p.Cout * OHW;
    c.off = ((int64_t)n * p.Cout + (int64_t)g * p.Og) * OHW + plane_off;
    c.ostride = OHW;
    c.oscale = (p.oscale && fused) ? p.oscale + (int64_t)n * p.Cout + (int64_t)g * p.Og : nullptr;
    c.bias = (ea.on && p.bias) ? p.bias + g * p.Og : nullptr;
    c.has_noise = p.noise && fused;
    c.nz = c.has_noise ? p.noise[(p.noise_ps ? (int64_t)n * OHW : 0) + plane_off] * nstr : 0.f;
    return c;
}

// The arithmetic of a launch of the split forward-type kernels as their template arguments: f(NP, IO, ISC) with std::integral_constants.
// q.bf16x6 = pieces per operand (3: six products, 2: three, 1: one, NP_F16X3); 16-bit storage is always one product; q.iscale (the input
// scale rides in the staging) implies fp32 storage and fp32-equivalent products (the caller checked).
template <class F>
static void conv_arith_dispatch(const ConvFwdParams& q, F&& f) {
    using std::integral_constant;
    typedef integral_constant<int, NP_F16X3> HX;
    typedef integral_constant<int, IO_F32> F32;
    const bool hx = q.bf16x6 == NP_F16X3;
    if (q.iscale && hx)       f(HX{}, F32{}, std::true_type{});
    else if (q.iscale)        f(integral_constant<int, 3>{}, F32{}, std::true_type{});
    else if (q.io == IO_BF16) f(integral_constant<int, 1>{}, integral_constant<int, IO_BF16>{}, std::false_type{});
    else if (q.io == IO_F16)  f(integral_constant<int, 1>{}, integral_constant<int, IO_F16>{}, std::false_type{});
    else if (q.bf16x6 == 1)   f(integral_constant<int, 1>{}, F32{}, std::false_type{});
    else if (q.bf16x6 == 2)   f(integral_constant<int, 2>{}, F32{}, std::false_type{});
    else if (hx)              f(HX{}, F32{}, std::false_type{});
    else                      f(integral_constant<int, 3>{}, F32{}, std::false_type{});
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Parameters of the weight-gradient kernels: dW[tap][a][b] = sum_pix S[a][pix] * L[b][pix * st + tap offset].
struct WgradParams {
    const float* S; const float* L; float* slab;        // S, L: elements of type `io`; slab: fp32
    const float* s_amax; const float* l_amax;           // PASTA_MATH_F16X3: AMAX_PARTS partial |max| of S and of L
    int io;                 // IO_F32 / IO_F16 / IO_BF16
    int N, SC, P, Q;        // S: [N, SC, P, Q]
    int LC, LH, LW;         // L: [N, LC, LH, LW]
    int G, Ag, Bg;
    int kh, kw, st, pad_h, pad_w;
    int cw_log2;            // chunk width = 1 << cw_log2, chunk height = 32 >> cw_log2
    int rows_total;         // N * P rows of S
    int qblocks;            // ceil(Q / CW)
    int chunks_total;       // ceil(rows_total / CHH) * qblocks
    int ksplit;             // K slices
    int a_tiles, b_tiles, tap_groups_r, tap_groups_s;
    int xcd_order;          // split weight-gradient kernels: workgroup order (0: K slice fastest; 1: see wgrad_workgroup)
    int l_pieces;           // conv_wgrad3x3s2_pieces_kernel: L is PASTA_LAYOUT_PIECES16 (pieces.hip), l_amax the producer's bound row
};

// Parameters of the few-channel pointwise kernels (conv_fwd_fewch.h).
struct FewChParams {
    const void* x; const float* w; void* y;      // x, y, res: elements of the storage type IO (fp32, or 16-bit storage: BASELINE config 5)
    const float* iscale;            // [N][Cin] or null (fewcout only)
    const float* bias; const void* res;
    float* y_amax;
    int io;                         // IO_F32 / IO_F16 / IO_BF16
    int N, Cin, Cout, HW;
    int w_io;                       // the weight tensor is [Cin][Cout] (conv_transpose2d), else [Cout][Cin]
    float wscale;
    int act; float alpha, gain, clamp;
};

// Parameters of the small-cin weight-gradient kernel (conv_wgrad_f32.h, conv_wgrad_smallcin_kernel).
struct WgradSmallParams {
    const float* S; const float* L; float* slab;
    int N, Ag, P, Q;        // S = dy: [N, Ag, P, Q]
    int Bg, LH, LW;         // L = x : [N, Bg, LH, LW]
    int kh, kw, pad_h, pad_w;
    int bprime, nb;         // Bg*kh*kw and its number of 32-column tiles (<= 5)
    int cw_log2, rows_total, qblocks, chunks_total, ksplit, a_tiles;
};

//------------------------------------------------------------------------------------
// What the weight-gradient kernels share (conv_wgrad_f32.h, conv_wgrad_bf16x6.h).  Every kernel keeps its own staging -- which pixels a thread
// fetches, in which order, with which validity -- and its own product loop; where its workgroup is, which chunks its K slice holds, how eight
// fp32 values become pieces in LDS and where the chunk walk stands is here, once, and leaves every kernel's device assembly as it was
// (profiles/wgrad_single_source_resources.txt).  The store of a sub-tile into the slab and the slab sum of the reductions stay in their kernels:
// as shared functions they changed the assembly, and timed against their own blocks they missed the allowance (the notes at those blocks;
// profiles/wgrad_single_source_ab.txt).

// Workgroup -> (K slice, b tile, a tile, group) of the split kernels.  The workgroups that read the same pixels are the tiles (a, b) of one
// K slice.  Order 0 (the original): K slice fastest -- those workgroups are ksplit apart in the grid (on one XCD when ksplit is a multiple
// of 8, but dispatched far from each other).  Order 1: the slice index modulo 8 fastest, then the tile, then the rest of the slice
// index: the tiles of a slice are 8 apart -- the same XCD (workgroups go round-robin to the eight XCDs), dispatched together.
__device__ __forceinline__ void wgrad_workgroup(const WgradParams& p, int& ks, int& bt, int& at, int& g) {
    int bid = blockIdx.x;
    if (p.xcd_order && (p.ksplit & 7) == 0) {
        const int lo = bid & 7; bid >>= 3;
        const int tiles = p.a_tiles * p.b_tiles;
        const int tile = bid % tiles; bid /= tiles;
        const int hi = bid % (p.ksplit >> 3); bid /= (p.ksplit >> 3);
        ks = hi * 8 + lo; bt = tile % p.b_tiles; at = tile / p.b_tiles; g = bid;
        return;
    }
    ks = bid % p.ksplit; bid /= p.ksplit;
    bt = bid % p.b_tiles; bid /= p.b_tiles;
    at = bid % p.a_tiles; bid /= p.a_tiles;
    g = bid;
}

// Chunks [c_begin, c_end) of K slice ks: the slices differ by at most one chunk.  The products are 32-bit and unsigned: the host refuses a launch
// whose chunks_total * (ksplit + 1) does not fit (conv_igemm.hip, the PASTA_CHECK in front of the launch; the small-cin plan stays far below it).
__device__ __forceinline__ void wgrad_slice(int chunks_total, int ksplit, int ks, int& c_begin, int& c_end) {
    c_begin = (int)(((unsigned)chunks_total * (unsigned)ks) / (unsigned)ksplit); c_end = (int)(((unsigned)chunks_total * (unsigned)(ks + 1)) / (unsigned)ksplit);
}

// PASTA_MATH_F16X3: the operand scales from the tensors' partial maxima, and what the slab is multiplied by on the way out; ones otherwise.
template <int NP>
__device__ __forceinline__ void wgrad_scales(const WgradParams& p, float& s_scale, float& l_scale, float& out_scale) {
    s_scale = 1.f; l_scale = 1.f; out_scale = 1.f;
    if constexpr (Arith<NP>::f16x3) {
        float is_, il_;
        scale_from_amax(amax_of_parts(p.s_amax), s_scale, is_);
        scale_from_amax(amax_of_parts(p.l_amax), l_scale, il_);
        out_scale = is_ * il_;
    }
}

// two float4 halves, each possibly invalid -> 0, as eight values
__device__ __forceinline__ void masked8(float4 h0, float4 h1, bool ok0, bool ok1, float (&vals)[8]) {
    vals[0] = ok0 ? h0.x : 0.f; vals[1] = ok0 ? h0.y : 0.f; vals[2] = ok0 ? h0.z : 0.f; vals[3] = ok0 ? h0.w : 0.f;
    vals[4] = ok1 ? h1.x : 0.f; vals[5] = ok1 ? h1.y : 0.f; vals[6] = ok1 ? h1.z : 0.f; vals[7] = ok1 ? h1.w : 0.f;
}

// eight fp32 values -> Arith<NP>::npw packed pieces of eight 16-bit elements (split-bf16: v = q1 + q2 + q3, each the bf16 of what is left;
// PASTA_MATH_F16X3: (h, l) of v * scale; 16-bit storage: the element itself), piece i stored at dst + i * piece_stride
template <int NP, int IO>
__device__ __forceinline__ void wgrad_split_store8(const float (&vals)[8], __bf16* dst, int piece_stride, float scale) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    constexpr int NPW = Arith<NP>::npw;
    uint32_t q1[4], q2[4], q3[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (Arith<NP>::f16x3) {
            f16_split2_direct(vals[2 * j] * scale, vals[2 * j + 1] * scale, q1[j], q2[j]);
            continue;
        }
        f32x2 v = {vals[2 * j], vals[2 * j + 1]};
        uint32_t w = io_pack2<IO>(vals[2 * j], vals[2 * j + 1]);
        q1[j] = w;
        if constexpr (NP >= 2) {
            v[0] -= __builtin_bit_cast(float, w << 16);
            v[1] -= __builtin_bit_cast(float, w & 0xffff0000u);
            w = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
            q2[j] = w;
        }
        if constexpr (NP >= 3) {
            v[0] -= __builtin_bit_cast(float, w << 16);
            v[1] -= __builtin_bit_cast(float, w & 0xffff0000u);
            q3[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
        }
    }
    *(uint4*)(dst) = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    if constexpr (NPW >= 2) *(uint4*)(dst + piece_stride) = make_uint4(q2[0], q2[1], q2[2], q2[3]);
    if constexpr (NPW >= 3) *(uint4*)(dst + 2 * piece_stride) = make_uint4(q3[0], q3[1], q3[2], q3[3]);
}

// Where the chunk walk of the ring kernels stands: the chunks go down a column block (pp fastest), then through the column blocks of an image,
// then through the images.  A position is decoded ONCE per K slice (two divisions by run-time values) and then advanced, for the current
// chunk and for the prefetched one (a decode per chunk and per prefetch was ~200 scalar instructions per chunk in front of the wave's matrix
// instructions).
struct WgradChunkPos { int n, qb, pp; };        // sample, column block, row
// (out-parameters by reference: returned by value, or as member functions, the same arithmetic changes the kernels' register allocation)
__device__ __forceinline__ void wgrad_chunk_at(const WgradParams& p, int ch, WgradChunkPos& c) {
    const int per_img = p.P * p.qblocks;
    c.n = ch / per_img;
    const int rem = ch - c.n * per_img;
    c.qb = rem / p.P; c.pp = rem - c.qb * p.P;
}
__device__ __forceinline__ void wgrad_chunk_next(const WgradParams& p, const WgradChunkPos& c, WgradChunkPos& next) {
    next.pp = c.pp + 1; next.qb = c.qb; next.n = c.n;
    if (next.pp == p.P) { next.pp = 0; next.qb = c.qb + 1; if (next.qb == p.qblocks) { next.qb = 0; next.n = c.n + 1; } }
}

// The three halo rows of a chunk live in a ring in LDS: image row y (>= -1) in slot y mod 3; `row` (0..2) slots after slot0
__device__ __forceinline__ int ring_slot(int y) { return (y + 3) % 3; }
__device__ __forceinline__ int ring_wrap(int slot0, int row) { return slot0 + row >= 3 ? slot0 + row - 3 : slot0 + row; }

// one accumulator sub-tile to zero (the loops over a kernel's sub-tiles stay in the kernel: zeroed by one call for a whole array, the stride-1
// kernel's assembly differs in 1950 of 13964 lines, main loop included)
__device__ __forceinline__ void wgrad_zero(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
}

// The arithmetic of a launch of the split weight-gradient kernels as their template arguments: f(NP, IO) with std::integral_constants.
// np = pieces per operand (3: six products, 2: three, 1: one, NP_F16X3); 16-bit storage is always one product.
template <class F>
static void wgrad_arith_dispatch(int np, int io, F&& f) {
    using std::integral_constant;
    typedef integral_constant<int, IO_F32> F32;
    if (io == IO_BF16)       f(integral_constant<int, 1>{}, integral_constant<int, IO_BF16>{});
    else if (io == IO_F16)   f(integral_constant<int, 1>{}, integral_constant<int, IO_F16>{});
    else if (np == 1)        f(integral_constant<int, 1>{}, F32{});
    else if (np == 2)        f(integral_constant<int, 2>{}, F32{});
    else if (np == NP_F16X3) f(integral_constant<int, NP_F16X3>{}, F32{});
    else                     f(integral_constant<int, 3>{}, F32{});
}

}  // namespace pasta
