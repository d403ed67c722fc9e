// Weight packing of the split forward-type kernels: the split-bf16 pieces, fp16 storage, and the fp16 pieces of PASTA_MATH_F16X3 with one
// scale per output row.  Plain kernels (no templates): defined by conv_tu_pack_f32.hip only (conv_launch.h).
#pragma once
#include "conv_common.h"

namespace pasta {

__device__ __forceinline__ void split3(float v, __bf16& a, __bf16& b, __bf16& c) {
    a = (__bf16)v;
    float r = v - (float)a;
    b = (__bf16)r;
    r -= (float)b;
    c = (__bf16)r;
}

// [g][tap][chunk of 16 channels][piece 3][half 2][O_pad][8]
__global__ __launch_bounds__(256) void pack_weights_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ wp, int G, int Ig,
                                                                int Og, int Ig_pad, int Og_pad, int kh, int kw, int transposed,
                                                                int flip, float wscale, int f16, const float* __restrict__ mod_s,
                                                                const float* __restrict__ mod_d) {
    // f16: 0 = three bf16 pieces, 1 = fp16 storage (leading piece = the fp16 operand).  PASTA_MATH_F16X3: pack_weights_f16x3_kernel
    const int64_t total = (int64_t)G * kh * kw * Ig_pad * Og_pad;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx & 7);
        int64_t r = idx >> 3;
        const int o = (int)(r % Og_pad); r /= Og_pad;
        const int half = (int)(r & 1); r >>= 1;
        const int cc = (int)(r % (Ig_pad / 16)); r /= (Ig_pad / 16);
        const int t = (int)(r % (kh * kw));
        const int g = (int)(r / (kh * kw));
        const int i = cc * 16 + half * 8 + j;
        float v = 0.f;
        if (i < Ig && o < Og) {
            int ty = t / kw, tx = t - ty * kw;
            if (flip) { ty = kh - 1 - ty; tx = kw - 1 - tx; }
            // mod_s: ONE weight of a single group, shared by all groups, modulated per group (= sample) on the way:
            // w[o,i] * s[g,i] (* d[g,o]) rounded in this order, as networks.py:65-68, 84-86 forms its per-sample weights
            const int gs = mod_s ? 0 : g;
            const int64_t src = transposed ? (((int64_t)(gs * Ig + i) * Og + o) * kh + ty) * kw + tx
                                           : (((int64_t)(gs * Og + o) * Ig + i) * kh + ty) * kw + tx;
            v = w[src] * wscale;
            if (mod_s) { v *= mod_s[(int64_t)g * Ig + i]; if (mod_d) v *= mod_d[(int64_t)g * Og + o]; }
        }
        __bf16 p1, p2, p3;
        split3(v, p1, p2, p3);
        if (f16 == 1) p1 = __builtin_bit_cast(__bf16, (_Float16)v);      // fp16 storage: the leading piece is the fp16 operand (the others are unused)
        const int64_t chunk = (((int64_t)g * kh * kw + t) * (Ig_pad / 16) + cc) * 6 * Og_pad * 8;
        const int64_t within = ((int64_t)half * Og_pad + o) * 8 + j;
        wp[chunk + within] = p1;
        wp[chunk + 2 * Og_pad * 8 + within] = p2;
        wp[chunk + 4 * Og_pad * 8 + within] = p3;
    }
}

// PASTA_MATH_F16X3 (conv_common.h): the same layout with the fp16 pieces h = fp16(v S), l = fp16(v S - h), h'' = h 2^-11 and the power-of-two scale S taken
// PER OUTPUT ROW from the row's own largest magnitude, found here: one workgroup owns one row o of one group over the whole K
// range (C_in kh kw values: at most a few thousand), first pass = fetch the row (every load of a thread in flight at once), form
// v = w wscale (s[g,i] d[g,o]), keep it in LDS and reduce |v| over the workgroup (non-finite values skipped, as the tensor scan
// does); second pass = split and store sixteen-byte units out of LDS, plus rowinv[g][o] = 1 / S for the convolution's epilogue.
// Hundreds of short workgroups: 5 - 8 us per layer like the element-parallel kernel it replaces (a first version with eight rows
// per workgroup and serial loads took 50 - 100 us: 341 launches per training step).  Nothing about w is cached between launches: a
// weight written behind autograd's back (`p.data.mul_()`, an optimiser that works on `.data`) cannot meet a stale scale, and
// per-sample modulated weights (pasta_conv2d_modulated) get their own scale per (sample, output channel).
constexpr int PACK_ROW_LDS = 8192;          // floats of a row kept in LDS; longer rows are re-read from global memory (L2)
__device__ __forceinline__ void pack_row_f16x3(const float* __restrict__ w, __bf16* __restrict__ wp, float* __restrict__ rowinv,
                                               int Ig, int Og, int Ig_pad, int Og_pad, int kh, int kw, int transposed, int flip,
                                               float wscale, const float* __restrict__ mod_s, const float* __restrict__ mod_d, int pack_xcd_rows, const unsigned bx) {
    // one packed row.  Eight consecutive rows share every 128-byte line of the packed layout ([...][O_pad][8 x 2 bytes]) and workgroups go round-robin
    // to the eight XCDs: XCD x takes the rows [x O_pad / 8, (x + 1) O_pad / 8), so that the sixteen-byte stores of a line meet in ONE L2 and leave it
    // as a whole line (O_pad is a multiple of 64)
    const int g = blockIdx.y, o = pack_xcd_rows ? (int)(bx & 7u) * (Og_pad >> 3) + (int)(bx >> 3) : (int)bx;
    const int taps = kh * kw, NC = Ig_pad / 16, K = Ig * taps;
    const int tid = threadIdx.x;
    const int gs = mod_s ? 0 : g;
    __shared__ float row[PACK_ROW_LDS];                     // v[i * taps + t], t = the tap index of the WEIGHT tensor (before the flip)
    __shared__ float wmax[4];
    const bool real = o < Og;
    const float md = (real && mod_d) ? mod_d[(int64_t)g * Og + o] : 1.f;
    // element k = i * taps + t of the row, as it lies in the weight tensor: the taps of one input channel are contiguous in both layouts
    auto tap_run = [&](int i) -> const float* {
        return w + (transposed ? ((int64_t)(gs * Ig + i) * Og + o) * taps : ((int64_t)(gs * Og + o) * Ig + i) * taps);
    };
    auto fetch = [&](int k) -> float {                       // rows longer than PACK_ROW_LDS: the second pass re-reads the tail
        const int i = k / taps, t = k - i * taps;
        float v = tap_run(i)[t] * wscale;
        if (mod_s) { v *= mod_s[(int64_t)g * Ig + i]; v *= md; }
        return v;
    };
    float m = 0.f;
    if (real) {
        if (taps <= 9) {
            // a thread owns input channels tid, tid + 256, ...: up to nine contiguous loads in flight, no division
            for (int i = tid; i < Ig; i += 256) {
                const float* const src = tap_run(i);
                const float ms = mod_s ? mod_s[(int64_t)g * Ig + i] : 1.f;
                float v[9];
#pragma unroll
                for (int t = 0; t < 9; t++) v[t] = t < taps ? src[t] : 0.f;
#pragma unroll
                for (int t = 0; t < 9; t++) {
                    if (t < taps) {
                        float x = v[t] * wscale;
                        if (mod_s) { x *= ms; x *= md; }
                        const int k = i * taps + t;
                        if (k < PACK_ROW_LDS) row[k] = x;
                        const float a = fabsf(x);
                        m = (a < __builtin_inff() && a > m) ? a : m;
                    }
                }
            }
        } else {
            for (int k0 = tid; k0 < K; k0 += 256 * 8) {          // eight loads in flight per thread and trip
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { const int k = k0 + 256 * j; v[j] = k < K ? fetch(k) : 0.f; }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int k = k0 + 256 * j;
                    if (k < K && k < PACK_ROW_LDS) row[k] = v[j];
                    const float a = fabsf(v[j]);
                    m = (a < __builtin_inff() && a > m) ? a : m;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    float S, inv;
    scale_from_amax(m, S, inv);
    if (tid == 0) rowinv[(int64_t)g * Og_pad + o] = inv;
    // second pass: unit u = (t_packed NC + cc) 2 + half -> sixteen bytes of h and of l: channels cc 16 + half 8 + 0..7 of packed tap t_packed
    const int units = taps * NC * 2;
    for (int u = tid; u < units; u += 256) {
        const int half = u & 1, k2 = u >> 1;
        const int cc = k2 % NC, tp = k2 / NC;
        int ty = tp / kw, tx = tp - ty * kw;
        if (flip) { ty = kh - 1 - ty; tx = kw - 1 - tx; }
        const int t = ty * kw + tx;
        uint32_t hq[4], lq[4], sq[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = cc * 16 + half * 8 + 2 * j;
            float v0 = 0.f, v1 = 0.f;
            if (real) {
                const int k = i * taps + t;
                if (i < Ig) v0 = k < PACK_ROW_LDS ? row[k] : fetch(k);
                if (i + 1 < Ig) v1 = k + taps < PACK_ROW_LDS ? row[k + taps] : fetch(k + taps);
            }
            f16_split2_direct(v0 * S, v1 * S, hq[j], lq[j]);
            sq[j] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2_t, hq[j]) * f16x2_t{(_Float16)0.00048828125f, (_Float16)0.00048828125f});
        }
        __bf16* const d = wp + (((int64_t)g * taps + tp) * NC + cc) * 6 * Og_pad * 8 + ((int64_t)half * Og_pad + o) * 8;
        *(uint4*)d = make_uint4(hq[0], hq[1], hq[2], hq[3]);
        *(uint4*)(d + 2 * Og_pad * 8) = make_uint4(lq[0], lq[1], lq[2], lq[3]);
        *(uint4*)(d + 4 * Og_pad * 8) = make_uint4(sq[0], sq[1], sq[2], sq[3]);
    }
}
__global__ __launch_bounds__(256) void pack_weights_f16x3_kernel(const float* __restrict__ w, __bf16* __restrict__ wp, float* __restrict__ rowinv,
                                                                 int Ig, int Og, int Ig_pad, int Og_pad, int kh, int kw, int transposed, int flip,
                                                                 float wscale, const float* __restrict__ mod_s, const float* __restrict__ mod_d, int pack_xcd_rows) {
    pack_row_f16x3(w, wp, rowinv, Ig, Og, Ig_pad, Og_pad, kh, kw, transposed, flip, wscale, mod_s, mod_d, pack_xcd_rows, blockIdx.x);
}
// Round 5: ONE weight tensor packed for TWO launches at once -- the forward convolution and its input gradient (the same weights transposed
// and mirrored) -- so that the backward pass finds its operand packed (pasta_conv2d_pack_pair; 120 of the 310 packing launches of a step).
// The first a.rows workgroups of the grid's x axis pack for a, the others for b.
__global__ __launch_bounds__(256) void pack_weights_f16x3_pair_kernel(const float* __restrict__ w, PackJob a, PackJob b) {
    const bool first = blockIdx.x < (unsigned)a.Og_pad;
    const PackJob& j = first ? a : b;
    pack_row_f16x3(w, (__bf16*)j.wp, j.rowinv, j.Ig, j.Og, j.Ig_pad, j.Og_pad, j.kh, j.kw, j.transposed, j.flip, j.wscale, nullptr, nullptr, j.pack_xcd_rows,
                   first ? blockIdx.x : blockIdx.x - (unsigned)a.Og_pad);
}

}  // namespace pasta
