// The small kernels around a convolution launch (conv_launch.h): the K-slice reduction, the operand bound under an input scale, the remainder
// of the parity-pair launch, and the two kernels that prepare the packed-K mode.
#include "conv_launch.h"

namespace pasta {

// y[n,c,:] = oscale[n,c] * sum_ks partial[ks][n,c,:]   (fixed order; split-K epilogue)
template <int IO>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial, void* __restrict__ y,
                                                            const float* __restrict__ oscale, int64_t numel, int ohw, int ksplit,
                                                            const float* __restrict__ bias, int cout, int act, float alpha, float gain,
                                                            float clamp, const void* __restrict__ res, const float* __restrict__ noise,
                                                            const float* __restrict__ noise_strength, int noise_ps, float* __restrict__ y_amax) {
    const float nstr = noise ? noise_strength[0] : 0.f;
    uint32_t am = 0;
    const AmaxSlot aslot = amax_begin(y_amax);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
        float v = 0.f;
        int k = 0;
        for (; k + 4 <= ksplit; k += 4) {                       // four slices in flight, summed in slice order
            const float r0 = partial[(int64_t)k * numel + i], r1 = partial[(int64_t)(k + 1) * numel + i];
            const float r2 = partial[(int64_t)(k + 2) * numel + i], r3 = partial[(int64_t)(k + 3) * numel + i];
            v += r0; v += r1; v += r2; v += r3;
        }
        for (; k < ksplit; k++) v += partial[(int64_t)k * numel + i];
        const int64_t nc = i / ohw;
        const float nz = noise ? noise[(noise_ps ? (nc / cout) * (int64_t)ohw : 0) + (i - nc * ohw)] * nstr : 0.f;
        v = conv_scale_noise(v, oscale ? oscale + nc : nullptr, 0, nz);
        if (res) v += io_ld1<IO>((const char*)res + i * io_size<IO>::value);
        if (act) v = conv_epilogue(v, bias ? bias[nc % cout] : 0.f, act, alpha, gain, clamp);
        io_st<IO>(y, i, v);
        if (y_amax) amax_take(am, v);
    }
    amax_commit(am, aslot);
}

void tu_splitk_reduce(const ConvFwdParams& p, hipStream_t s) {
    const int64_t numel = (int64_t)p.N * p.Cout * p.OH * p.OW;
    int64_t blocks = ceil_div64(numel, 256);
    if (blocks > 2048) blocks = 2048;
#define PASTA_SK(IO_) hipLaunchKernelGGL(splitk_reduce_kernel<IO_>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)p.partial, (void*)p.y, p.oscale, numel, \
                                         p.OH * p.OW, p.ksplit, p.bias, p.Cout, p.act, p.alpha, p.gain, p.clamp, (const void*)p.res, p.noise, p.noise_strength, p.noise_ps, (float*)nullptr)
    if (p.io == IO_BF16) PASTA_SK(IO_BF16); else if (p.io == IO_F16) PASTA_SK(IO_F16); else PASTA_SK(IO_F32);
#undef PASTA_SK
}

// parts[i] *= max |v|: the bound of |x * iscale| from the bound of |x| (one workgroup; iscale is [N, C_in])
__global__ __launch_bounds__(256) void amax_times_kernel(const float* __restrict__ parts_in, const float* __restrict__ v, int n, float* __restrict__ parts_out) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const float a = fabsf(v[i]); m = (a < __builtin_inff() && a > m) ? a : m; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    parts_out[threadIdx.x] = parts_in[threadIdx.x] * m;
}

void tu_amax_times(const float* parts_in, const float* v, int n, float* parts_out, hipStream_t s) {
    hipLaunchKernelGGL(amax_times_kernel, dim3(1), dim3(256), 0, s, parts_in, v, n, parts_out);
}

// The remainder of the parity-pair launch: output row 2H and / or column 2W of a stride-2 conv_transpose2d onto an odd plane --
// 1 % of the outputs, each a dot product over ONE input row or column (one or two taps).  As lattices of the MFMA kernels these
// were a few dozen workgroups whose K loops are as long as anyone's: 0.17 ms of latency behind a 0.2 ms main launch (measured,
// profiles/r3_ab_pair_f16x3.txt).  Here: plain fp32 FMAs on the raw weights, one thread per (pixel, 16 output channels), the
// lanes of a wave along the lattice -- thousands of short independent chains instead of thirty long ones.
template <bool MOD>          // MOD: one shared weight modulated per group on the way (pasta_conv2d_modulated), as the packing kernel does
__global__ __launch_bounds__(256) void conv_t2_edge_kernel(ConvFwdParams p, EdgeWeights ew) {
    constexpr int OC = 16, KC = 64;                      // a workgroup: 64 lattice pixels x 64 output channels, K in chunks of 64 channels
    __shared__ float xs[KC][64];                         // [channel][pixel]
    __shared__ __attribute__((aligned(16))) float wsm[KC][64];     // [channel][output channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.z;
    int c = 0, tile = blockIdx.x;
    for (; c < p.ncls - 1; c++) {                        // classes share the grid's x axis
        const int t = (p.N * p.cls[c].P * p.cls[c].Q + 63) >> 6;
        if (tile < t) break;
        tile -= t;
    }
    const int P = p.cls[c].P, Q = p.cls[c].Q, T = p.cls[c].T, tap0 = p.cls[c].tap0;
    const int pix = tile * 64 + lane;                    // the same pixel in all four waves: lanes along the lattice
    const bool live = pix < p.N * P * Q;
    const int n = live ? pix / (P * Q) : 0;
    const int rem = live ? pix - n * P * Q : 0;
    const int pp = rem / Q, qq = rem - pp * Q;
    const int ob = blockIdx.y * 64;                      // this workgroup's output channels; this wave's: ob + 16 wave ...
    const int HW = p.H * p.W;
    float acc[OC];
#pragma unroll
    for (int j = 0; j < OC; j++) acc[j] = 0.f;
    const float* const xb = p.x + ((int64_t)n * p.Cin + (int64_t)g * p.Ig) * HW;
    const int gs = MOD ? 0 : g;
    const int wo = ob + lane < p.Og ? ob + lane : p.Og - 1;           // staging role of this thread: weight column `lane`
    const float wlive = ob + lane < p.Og ? ew.wscale : 0.f;
    float md = 1.f;
    if constexpr (MOD) md = ew.mod_d ? ew.mod_d[(int64_t)g * p.Og + wo] : 1.f;
    for (int t = 0; t < T; t++) {
        const int iy = pp + p.tap_dy[tap0 + t], ix = qq + p.tap_dx[tap0 + t];
        const bool ok = live && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* const xp = xb + (ok ? iy * p.W + ix : 0);
        const int slab = ew.flip ? 8 - p.tap_slab[tap0 + t] : p.tap_slab[tap0 + t];
        const float* const wt = ew.w + ((int64_t)gs * p.Ig * p.Og + wo) * 9 + slab;      // [C_in][C_out / G][3][3]
        for (int i0 = 0; i0 < p.Ig; i0 += KC) {
            // every load of the chunk in flight at once: one round trip for the column gather, one for the weights
            float xr[KC / 4], wr[KC / 4];
#pragma unroll
            for (int k = 0; k < KC / 4; k++) {
                const int ii = i0 + wave + 4 * k;
                const int ic = ii < p.Ig ? ii : p.Ig - 1;
                xr[k] = (ok && ii < p.Ig) ? xp[(int64_t)ic * HW] : 0.f;
                float wv = wt[(int64_t)ic * p.Og * 9] * (ii < p.Ig ? wlive : 0.f);
                if constexpr (MOD) { wv *= ew.mod_s[(int64_t)g * p.Ig + ic]; wv *= md; }
                wr[k] = wv;
            }
            __syncthreads();                             // the previous chunk has been consumed
#pragma unroll
            for (int k = 0; k < KC / 4; k++) { xs[wave + 4 * k][lane] = xr[k]; wsm[wave + 4 * k][lane] = wr[k]; }
            __syncthreads();
#pragma unroll 8
            for (int ii = 0; ii < KC; ii++) {
                const float xv = xs[ii][lane];
#pragma unroll
                for (int q4 = 0; q4 < OC / 4; q4++) {
                    const float4 w4 = *(const float4*)&wsm[ii][wave * OC + 4 * q4];      // wave-uniform address: a broadcast read
                    acc[4 * q4 + 0] = fmaf(xv, w4.x, acc[4 * q4 + 0]);
                    acc[4 * q4 + 1] = fmaf(xv, w4.y, acc[4 * q4 + 1]);
                    acc[4 * q4 + 2] = fmaf(xv, w4.z, acc[4 * q4 + 2]);
                    acc[4 * q4 + 3] = fmaf(xv, w4.w, acc[4 * q4 + 3]);
                }
            }
        }
    }
    if (!live) return;
    const int o0 = ob + wave * OC;
    float* const yb = p.y + (((int64_t)n * p.Cout + (int64_t)g * p.Og + o0) * p.OH + p.cls[c].oy0 + pp * p.osy) * p.OW + p.cls[c].ox0 + qq * p.osx;
#pragma unroll
    for (int j = 0; j < OC; j++)
        if (o0 + j < p.Og) yb[(int64_t)j * p.OH * p.OW] = acc[j];
}

// (everything stays on the caller's stream: the library owns nothing persistent)
void tu_conv_t2_edge(const ConvFwdParams& q, const EdgeWeights& ew, hipStream_t s) {
    int tiles = 0;
    for (int c = 0; c < q.ncls; c++) tiles += (q.N * q.cls[c].P * q.cls[c].Q + 63) >> 6;
    const dim3 grid((unsigned)tiles, (unsigned)((q.Og + 63) / 64), (unsigned)q.G);
    if (ew.mod_s) hipLaunchKernelGGL(conv_t2_edge_kernel<true>, grid, dim3(256), 0, s, q, ew);
    else hipLaunchKernelGGL(conv_t2_edge_kernel<false>, grid, dim3(256), 0, s, q, ew);
}

// Packed-K mode (conv_fwd_bf16x6_kernel, KT): byte offset of "channel" k = (input channel c, tap (ty, tx)) from a pixel's base
// address in the padded input -- the tap the weight element [o][c][ty][tx] multiplies (mirrored when the launch flips the weight).
__global__ __launch_bounds__(256) void packed_koff_kernel(unsigned* __restrict__ koff, int K, int kh, int kw, int flip, int HWp, int Wp) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int c = k / (kh * kw), t = k - c * kh * kw;
    int ty = t / kw, tx = t - ty * kw;
    if (flip) { ty = kh - 1 - ty; tx = kw - 1 - tx; }
    koff[k] = (unsigned)(c * HWp + ty * Wp + tx) * 4u;
}

void tu_packed_koff(unsigned* koff, int K, int kh, int kw, int flip, int HWp, int Wp, hipStream_t s) {
    hipLaunchKernelGGL(packed_koff_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, koff, K, kh, kw, flip, HWp, Wp);
}

__global__ __launch_bounds__(256) void pad_planes_kernel(const float* __restrict__ x, float* __restrict__ xp, int64_t planes, int H, int W,
                                                         int ph, int pw) {
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int64_t total = planes * Hp * Wp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t plane = i / (Hp * Wp);
        const int r = (int)(i - plane * Hp * Wp);
        const int y = r / Wp - ph, xx = r - (r / Wp) * Wp - pw;
        xp[i] = ((unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W) ? x[(plane * H + y) * W + xx] : 0.f;
    }
}

void tu_pad_planes(const float* x, float* xp, int64_t planes, int H, int W, int ph, int pw, hipStream_t s) {
    const int64_t total = planes * (H + 2 * ph) * (W + 2 * pw);
    hipLaunchKernelGGL(pad_planes_kernel, dim3((unsigned)(ceil_div64(total, 256) < 4096 ? ceil_div64(total, 256) : 4096)), dim3(256), 0, s, x, xp, planes, H, W, ph, pw);
}

}  // namespace pasta
