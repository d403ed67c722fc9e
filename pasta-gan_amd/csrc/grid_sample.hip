// Bilinear grid_sample with zero padding and align_corners = False under a general sampling grid (the reference's
// torch_utils/ops/grid_sample_gradfix.py:22-83: F.grid_sample forward :44-51, aten::grid_sampler_2d_backward for both gradients :61-67).
//
//   grid_sample_fwd   one thread per output point (n, oy, ox) and chunk of channels: the grid pair is read once, the
//                     four tap offsets and weights are computed once, and the thread walks the chunk's planes (lanes =
//                     consecutive ox, so every plane's store is one contiguous wave segment).
//   grid_sample_bwd   the same layout, one pass over dy for both gradients:
//                     dx = S^T dy scatters w * dy into the four taps with no-return global_atomic_add_f32 (lanes =
//                     consecutive ox: for a grid close to the identity a wave's adds land in one or two input rows, the
//                     shape the atomic unit runs at full rate; a rotated grid spreads them over more rows and runs slower);
//                     grad_grid reduces over all C in registers and is stored once per point (no atomics: deterministic).
//                     dx is NOT bitwise reproducible from run to run (float adds in arrival order), nor is ATen's.
//                     16-bit images accumulate dx in an fp32 workspace, converted by one pass at the end.
//
// Coordinates, weights and sums are fp32 for fp32 / fp16 / bf16 storage and fp64 for fp64 images (A = acc_of<T>::type).  Coordinate arithmetic is ATen's
// (GridSampler.cuh: grid_sampler_unnormalize / grid_sampler_2d_backward_kernel): ix = ((gx + 1) * IW - 1) / 2, the
// north-west tap at floor(ix), weights (ix_se - ix) (iy_se - iy) and so on; a tap outside the image contributes 0.
#include "common.h"

namespace pasta {

template <class A> struct Pair { A x, y; };
template <class A, class G> __device__ __forceinline__ Pair<A> ld_grid(const G* g) { return Pair<A>{(A)ld<G>(g), (A)ld<G>(g + 1)}; }
template <>        __device__ __forceinline__ Pair<float> ld_grid<float, float>(const float* g) { const float2 v = *(const float2*)g; return {v.x, v.y}; }

// The bilinear footprint of one sample: tap offsets inside the plane, their weights, and which taps are inside the image.
template <class A>
struct Footprint {
    int64_t o[4];                       // nw, ne, sw, se
    A w[4];
    bool in[4];
    A ix, iy, ix_nw, iy_nw;             // for the weight derivatives
};

template <class A>
__device__ __forceinline__ Footprint<A> footprint(Pair<A> g, int IH, int IW) {
    Footprint<A> f;
    f.ix = ((g.x + A(1)) * IW - A(1)) * A(0.5);
    f.iy = ((g.y + A(1)) * IH - A(1)) * A(0.5);
    // far outside (or NaN): every tap is out of range, and the int conversion below stays defined
    if (!(fabs(f.ix) < A(1e8) && fabs(f.iy) < A(1e8))) f.ix = f.iy = A(-4);
    f.ix_nw = floor(f.ix);
    f.iy_nw = floor(f.iy);
    const A ix_se = f.ix_nw + A(1), iy_se = f.iy_nw + A(1);
    f.w[0] = (ix_se - f.ix) * (iy_se - f.iy);
    f.w[1] = (f.ix - f.ix_nw) * (iy_se - f.iy);
    f.w[2] = (ix_se - f.ix) * (f.iy - f.iy_nw);
    f.w[3] = (f.ix - f.ix_nw) * (f.iy - f.iy_nw);
    const int j0 = (int)f.ix_nw, i0 = (int)f.iy_nw;
    const bool x0 = (unsigned)j0 < (unsigned)IW, x1 = (unsigned)(j0 + 1) < (unsigned)IW;
    const bool y0 = (unsigned)i0 < (unsigned)IH, y1 = (unsigned)(i0 + 1) < (unsigned)IH;
    f.in[0] = y0 && x0; f.in[1] = y0 && x1; f.in[2] = y1 && x0; f.in[3] = y1 && x1;
    const int64_t base = (int64_t)i0 * IW + j0;
    f.o[0] = base; f.o[1] = base + 1; f.o[2] = base + IW; f.o[3] = base + IW + 1;
    return f;
}

// Launch shape: blockIdx.x = 256 output points of one sample, blockIdx.y = the sample, blockIdx.z = a chunk of channels.  A thread
// computes its footprint once per chunk; chunks of kChunk channels give C = 64 maps four times the waves of one thread per point.
static constexpr int kChunk = 16;

template <class T, class G>
__global__ __launch_bounds__(256) void grid_sample_fwd_kernel(const T* __restrict__ x, const G* __restrict__ grid, T* __restrict__ y,
                                                              int OHW, int C, int IH, int IW, int cch) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= OHW) return;
    const int64_t n = blockIdx.y, IHW = (int64_t)IH * IW;
    const int c0 = blockIdx.z * cch, c1 = min(C, c0 + cch);
    typedef typename acc_of<T>::type A;
    const Footprint<A> f = footprint<A>(ld_grid<A, G>(grid + 2 * (n * OHW + q)), IH, IW);
    const T* xp = x + (n * C + c0) * IHW;
    T* yp = y + (n * C + c0) * OHW + q;
#pragma unroll 4
    for (int c = c0; c < c1; c++) {
        // ATen's order of the four terms
        A acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (f.in[k]) acc = fma(ld<T>(xp + f.o[k]), f.w[k], acc);
        st<T>(yp, acc);
        xp += IHW;
        yp += OHW;
    }
}

// DX: scatter w * dy into dxacc (A = fp32 or fp64, zeroed); DG: grad_grid = (IW / 2, IH / 2) * sum_c dy * d(sum_k w_k x_k)/d(ix, iy), so a
// DG launch has one chunk of all C channels.
template <class T, class G, bool DX, bool DG>
__global__ __launch_bounds__(256) void grid_sample_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const G* __restrict__ grid,
                                                              typename acc_of<T>::type* __restrict__ dxacc, G* __restrict__ dgrid, int OHW,
                                                              int C, int IH, int IW, int cch) {
    typedef typename acc_of<T>::type A;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= OHW) return;
    const int64_t n = blockIdx.y, IHW = (int64_t)IH * IW, p = n * OHW + q;
    const int c0 = blockIdx.z * cch, c1 = min(C, c0 + cch);
    const Footprint<A> f = footprint<A>(ld_grid<A, G>(grid + 2 * p), IH, IW);
    // derivatives of the four weights: d/dix = (-(iy_se - iy), iy_se - iy, -(iy - iy_nw), iy - iy_nw), likewise for iy
    const A ay = f.iy - f.iy_nw, by = A(1) - ay, ax = f.ix - f.ix_nw, bx = A(1) - ax;
    const T* dyp = dy + (n * C + c0) * OHW + q;
    const T* xp = DG ? x + (n * C + c0) * IHW : nullptr;
    A* dxp = DX ? dxacc + (n * C + c0) * IHW : nullptr;
    A gix = 0, giy = 0;
#pragma unroll 2
    for (int c = c0; c < c1; c++) {
        const A g = ld<T>(dyp);
        if (DX) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (f.in[k]) unsafeAtomicAdd(dxp + f.o[k], f.w[k] * g);     // no-return global_atomic_add_f32 / _f64
            dxp += IHW;
        }
        if (DG) {
            A v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = f.in[k] ? ld<T>(xp + f.o[k]) : A(0);
            // sum_k v_k dw_k/dix and dw_k/diy
            const A sx = (v[1] - v[0]) * by + (v[3] - v[2]) * ay;
            const A sy = (v[2] - v[0]) * bx + (v[3] - v[1]) * ax;
            gix = fma(g, sx, gix);
            giy = fma(g, sy, giy);
            xp += IHW;
        }
        dyp += OHW;
    }
    if (DG) {
        st<G>(dgrid + 2 * p, gix * (A(0.5) * IW));
        st<G>(dgrid + 2 * p + 1, giy * (A(0.5) * IH));
    }
}

// dst[i] = (T)src[i]: the fp32 workspace of a 16-bit dx, four elements per thread.
template <class T>
__global__ __launch_bounds__(256) void f32_narrow_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 256 * 4) {
        if (i + 4 <= n) st4<T>(dst + i, *(const float4*)(src + i));
        else
            for (int64_t k = i; k < n; k++) st<T>(dst + k, src[k]);
    }
}

// Grid-stride blocks for the conversion pass.
static unsigned blocks_for(int64_t work) {
    const int64_t b = ceil_div64(work, 256);
    return (unsigned)(b < (1 << 20) ? (b > 0 ? b : 1) : (1 << 20));
}

static dim3 point_grid(int64_t n, int OHW, int C, int cch) { return dim3((unsigned)ceil_div64(OHW, 256), (unsigned)n, (unsigned)ceil_div64(C, cch)); }

static int grid_sample_check(const char* who, int64_t n, int C, int IH, int IW, int OH, int OW, int dtype, int grid_dtype) {
    PASTA_CHECK(n >= 1 && C >= 1 && IH >= 1 && IW >= 1 && OH >= 1 && OW >= 1, "%s: %lld images [%d, %d, %d] -> [%d, %d]", who,
                (long long)n, C, IH, IW, OH, OW);
    // tap offsets are int32 inside a plane (row index * IW + column) and int64 across planes; |coordinate| < 1e8 keeps the
    // float -> int conversion defined, so a plane dimension must stay below that
    PASTA_CHECK(IH < (1 << 26) && IW < (1 << 26) && (int64_t)IH * IW < ((int64_t)1 << 62) / C / n, "%s: input [%lld, %d, %d, %d] is too large",
                who, (long long)n, C, IH, IW);
    PASTA_CHECK((int64_t)OH * OW < ((int64_t)1 << 62) / C / n, "%s: output [%lld, %d, %d, %d] is too large", who, (long long)n, C, OH, OW);
    // launch shape (point_grid): output points of one sample in x, samples in y (<= 65535), channel chunks in z
    PASTA_CHECK(n <= 65535 && (int64_t)OH * OW <= ((int64_t)1 << 31) - 256, "%s: %lld samples of %d x %d output points: at most 65535 samples of "
                "2^31 - 256 points", who, (long long)n, OH, OW);
    PASTA_CHECK(ceil_div64(C, kChunk) <= 65535, "%s: %d channels: at most %d", who, C, 65535 * kChunk);
    PASTA_CHECK(dtype == PASTA_F32 || dtype == PASTA_F16 || dtype == PASTA_BF16 || dtype == PASTA_F64, "%s: unsupported image dtype code %d", who,
                dtype);
    PASTA_CHECK(grid_dtype == dtype || (grid_dtype == PASTA_F32 && dtype != PASTA_F64), "%s: the grid must have the image's dtype or, for a "
                "16-bit image, float32 (codes %d, %d)", who, grid_dtype, dtype);
    return 0;
}

template <class T, class G>
static int fwd_launch(const void* x, const void* grid, void* y, int64_t n, int OHW, int C, int IH, int IW, hipStream_t s) {
    hipLaunchKernelGGL((grid_sample_fwd_kernel<T, G>), point_grid(n, OHW, C, kChunk), dim3(256), 0, s, (const T*)x, (const G*)grid, (T*)y, OHW,
                       C, IH, IW, kChunk);
    return launch_status("grid_sample");
}

template <class T, class G>
static int bwd_launch(const void* dy, const void* x, const void* grid, void* dx, void* dgrid, void* ws, int64_t n, int C, int IH, int IW,
                      int OHW, hipStream_t s) {
    typedef typename acc_of<T>::type A;
    const int64_t nx = n * C * IH * IW;
    // fp32 / fp64 images accumulate in dx itself, 16-bit ones in the fp32 workspace
    A* acc = dx ? (sizeof(T) == sizeof(A) ? (A*)dx : (A*)ws) : nullptr;
    if (acc) PASTA_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)nx * sizeof(A), s));
    if (dx && dgrid)
        hipLaunchKernelGGL((grid_sample_bwd_kernel<T, G, true, true>), point_grid(n, OHW, C, C), dim3(256), 0, s, (const T*)dy, (const T*)x,
                           (const G*)grid, acc, (G*)dgrid, OHW, C, IH, IW, C);
    else if (dx)
        hipLaunchKernelGGL((grid_sample_bwd_kernel<T, G, true, false>), point_grid(n, OHW, C, kChunk), dim3(256), 0, s, (const T*)dy, (const T*)x,
                           (const G*)grid, acc, (G*)dgrid, OHW, C, IH, IW, kChunk);
    else
        hipLaunchKernelGGL((grid_sample_bwd_kernel<T, G, false, true>), point_grid(n, OHW, C, C), dim3(256), 0, s, (const T*)dy, (const T*)x,
                           (const G*)grid, acc, (G*)dgrid, OHW, C, IH, IW, C);
    if (int e = launch_status("grid_sample_backward")) return e;
    if constexpr (sizeof(T) != sizeof(A)) {
        if (acc) {
            hipLaunchKernelGGL((f32_narrow_kernel<T>), dim3(blocks_for(ceil_div64(nx, 4))), dim3(256), 0, s, (const float*)acc, (T*)dx, nx);
            return launch_status("grid_sample_backward (narrow dx)");
        }
    }
    return 0;
}

}  // namespace pasta

using namespace pasta;

extern "C" int pasta_grid_sample(const void* x, const void* grid, void* y, int64_t n, int C, int IH, int IW, int OH, int OW, int dtype,
                                 int grid_dtype, void* stream) {
    PASTA_CHECK(x && grid && y, "grid_sample: null pointer");
    if (int e = grid_sample_check("grid_sample", n, C, IH, IW, OH, OW, dtype, grid_dtype)) return e;
    const int OHW = OH * OW;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PASTA_F32) return fwd_launch<float, float>(x, grid, y, n, OHW, C, IH, IW, s);
    if (dtype == PASTA_F64) return fwd_launch<double, double>(x, grid, y, n, OHW, C, IH, IW, s);
    if (dtype == PASTA_F16) return grid_dtype == PASTA_F32 ? fwd_launch<__half, float>(x, grid, y, n, OHW, C, IH, IW, s)
                                                           : fwd_launch<__half, __half>(x, grid, y, n, OHW, C, IH, IW, s);
    return grid_dtype == PASTA_F32 ? fwd_launch<__bf16, float>(x, grid, y, n, OHW, C, IH, IW, s)
                                   : fwd_launch<__bf16, __bf16>(x, grid, y, n, OHW, C, IH, IW, s);
}

extern "C" int64_t pasta_grid_sample_backward_workspace(int64_t n, int C, int IH, int IW, int dtype) {
    if (n < 1 || C < 1 || IH < 1 || IW < 1) return fail("grid_sample_backward_workspace: [%lld, %d, %d, %d]", (long long)n, C, IH, IW), -1;
    return (dtype == PASTA_F32 || dtype == PASTA_F64) ? 0 : n * C * (int64_t)IH * IW * (int64_t)sizeof(float);
}

extern "C" int pasta_grid_sample_backward(const void* dy, const void* x, const void* grid, void* dx, void* dgrid, void* ws, int64_t n, int C,
                                          int IH, int IW, int OH, int OW, int dtype, int grid_dtype, void* stream) {
    PASTA_CHECK(dy && grid, "grid_sample_backward: null pointer");
    PASTA_CHECK(dx || dgrid, "grid_sample_backward: neither gradient requested");
    PASTA_CHECK(!dgrid || x, "grid_sample_backward: the grid gradient needs the image");
    PASTA_CHECK(!dx || dtype == PASTA_F32 || dtype == PASTA_F64 || ws, "grid_sample_backward: a 16-bit dx needs the fp32 workspace");
    if (int e = grid_sample_check("grid_sample_backward", n, C, IH, IW, OH, OW, dtype, grid_dtype)) return e;
    const int OHW = OH * OW;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PASTA_F32) return bwd_launch<float, float>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s);
    if (dtype == PASTA_F64) return bwd_launch<double, double>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s);
    if (dtype == PASTA_F16) return grid_dtype == PASTA_F32 ? bwd_launch<__half, float>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s)
                                                           : bwd_launch<__half, __half>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s);
    return grid_dtype == PASTA_F32 ? bwd_launch<__bf16, float>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s)
                                   : bwd_launch<__bf16, __bf16>(dy, x, grid, dx, dgrid, ws, n, C, IH, IW, OHW, s);
}
