// The K-loop body the split forward-type kernels share, written once: the operand split of a pair of activation values, the order in which the
// fragments of a chunk are read, and the order of the product groups with the staging slots between them.  Included by conv_fwd_bf16x6.h,
// conv_fwd_rows2d_bf16x6.h, conv_fwd_1x1.h, conv_fwd_s2.h and conv_fwd_t2.h; templates only (conv_launch.h).
// The product order is a numerical property -- results keep their bits only while every kernel adds the same terms in the same order -- and
// the read order and the slot placement are measured tuning decisions: all three are changed HERE, for every tile at
// once.  The one deliberate exception is the register-diet schedule of the row kernel (step_diet, conv_fwd_bf16x6.h).
#pragma once
#include "conv_common.h"

namespace pasta {

// Border pixel or channel tail: of the eight channels of a staging unit the first nvalid are real; this is pair j (channels 2j, 2j + 1).
// SKIP: whole units (the common case) jump over the two selects; conv_t2_body keeps the selects unconditional, as it always had them
// (with the test the compiler lays out its whole K loop differently, and nobody has measured that layout).
template <bool SKIP = true>
__device__ __forceinline__ void fwd_mask2(float& v0, float& v1, int j, int nvalid) {
    if (!SKIP || nvalid < 8) {
        v0 = 2 * j < nvalid ? v0 : 0.f;
        v1 = 2 * j + 1 < nvalid ? v1 : 0.f;
    }
}

// One step of the residual chain: what the pair keeps once its piece w (two packed bf16) is taken out.
// The two subtractions stay scalar: packed f32 VALU next to MFMAs costs more than it saves (MI355X_MICROARCH.md, cycle table), and the
// empty asm keeps the SLP vectoriser from pairing them.
__device__ __forceinline__ void fwd_residual2(float& v0, float& v1, uint32_t w) {
    v0 -= __builtin_bit_cast(float, w << 16);
    v1 -= __builtin_bit_cast(float, w & 0xffff0000u);
    PASTA_KEEP_SCALAR(v0);
}

// One pair of activation values (masked, input scale applied) -> its operand pieces, two elements per dword: the fp16 pieces h | l' of
// v * x_scale (PASTA_MATH_F16X3: w1, w2), or NP bf16 pieces by the residual chain v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2)
// (v_cvt_pk_bf16_f32 yields the packed pair, the residuals come from its halves).  NP = 1: the element of the storage type IO itself.
template <int NP, int IO>
__device__ __forceinline__ void fwd_split2(float v0, float v1, float x_scale, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
    if constexpr (Arith<NP>::f16x3) {
        f16_split2(v0 * x_scale, v1 * x_scale, w1, w2);
        return;
    }
    w1 = io_pack2<IO>(v0, v1);
    if constexpr (NP >= 2) {
        fwd_residual2(v0, v1, w1);
        w2 = io_pack2<IO_F32>(v0, v1);
    }
    if constexpr (NP >= 3) {
        fwd_residual2(v0, v1, w2);
        w3 = io_pack2<IO_F32>(v0, v1);
    }
}

// Fragments of one chunk: [tile][piece].
template <int WMT, int WNT> struct FwdFrag { bf16x8 a[WMT][3], b[WNT][3]; };

// Reads them in the order the product groups of fwd_products consume them, so that the first group starts when ITS operands have landed
// (the LDS returns reads in order: counted lgkmcnt waits).  a_ptr(piece, a) / b_ptr(piece, b): the caller's fragment addresses.
template <int NP, int WMT, int WNT, class PA, class PB>
__device__ __forceinline__ void fwd_read_frag(FwdFrag<WMT, WNT>& f, PA&& a_ptr, PB&& b_ptr) {
    using std::integral_constant;
    auto lda = [&](auto pc) {
        constexpr int PC = decltype(pc)::value;
        if constexpr (PC < Arith<NP>::npa) {
#pragma unroll
            for (int a = 0; a < WMT; a++) f.a[a][PC] = *a_ptr(PC, a);
        }
    };
    auto ldb = [&](auto pc) {
        constexpr int PC = decltype(pc)::value;
        if constexpr (PC < Arith<NP>::npb) {
#pragma unroll
            for (int b = 0; b < WNT; b++) f.b[b][PC] = *b_ptr(PC, b);
        }
    };
    const integral_constant<int, 0> p0; const integral_constant<int, 1> p1; const integral_constant<int, 2> p2;
    if constexpr (Arith<NP>::f16x3) { lda(p2); ldb(p1); lda(p1); ldb(p0); lda(p0); }      // three-product arithmetic: (h'' l'), (l h), (h h)
    else { lda(p2); ldb(p0); lda(p0); ldb(p2); lda(p1); ldb(p1); }
}

// The product groups of one chunk, smallest terms first -- six products: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1; three (PASTA_MATH_F16X3): h'' l',
// l h, h h; a group = every (a, b) tile of the wave for one pair of pieces (A piece, B piece), acc[a][b] += f.a[a][.] f.b[b][.].
// slot(integral_constant<int, J>), J = 0 .. 3: the four quarters of the caller's staging work for a later chunk (its split), interleaved between
// the groups; before_last(): where the caller's LDS stores go, in front of the last group.  Kernels that stage elsewhere pass empty callables.
template <int NP, int IO, int WMT, int WNT, class Acc, class Slot, class Last>
__device__ __forceinline__ void fwd_products(const FwdFrag<WMT, WNT>& f, Acc&& acc, Slot&& slot, Last&& before_last) {
    using std::integral_constant;
    auto mm = [&](auto pa, auto pb) {
        constexpr int PA = decltype(pa)::value, PB = decltype(pb)::value;
        if constexpr (mm_on<NP>(PA, PB)) {
#pragma unroll
            for (int a = 0; a < WMT; a++)
#pragma unroll
                for (int b = 0; b < WNT; b++) acc[a][b] = mfma16<IO, NP>(f.a[a][PA], f.b[b][PB], acc[a][b]);
        }
    };
    const integral_constant<int, 0> c0; const integral_constant<int, 1> c1; const integral_constant<int, 2> c2; const integral_constant<int, 3> c3;
    if constexpr (Arith<NP>::f16x3) {
        mm(c2, c1);
        slot(c0);
        slot(c1);
        mm(c1, c0);
        slot(c2);
        slot(c3);
    } else {
        mm(c2, c0);
        slot(c0);
        mm(c0, c2);
        slot(c1);
        mm(c1, c1);
        slot(c2);
        mm(c1, c0);
        slot(c3);
        mm(c0, c1);
    }
    before_last();
    mm(c0, c0);
}
// (for the kernels that stage outside the product groups)
struct FwdNoSlot { template <class J> __device__ __forceinline__ void operator()(J) const {} };
struct FwdNoStores { __device__ __forceinline__ void operator()() const {} };

}  // namespace pasta
