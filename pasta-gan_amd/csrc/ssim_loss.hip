// The SSIM term of the generator's loss (torch_utils/ops/ssim_loss.py): 1 - mean SSIM of a generated image against
// the photograph, with its gradient with respect to the generated image.  The windows and constants are those of the metric
// (csrc/recon_metrics.hip, csrc/recon_window.h) on the networks' own values v as intensities v + 1 in [0, 2]: dynamic range 2,
// not clipped, not quantised.
//   pasta_ssim_loss            the loss (an fp32 scalar in device memory) and, when asked, the three derivative maps per window
//                              position that the backward launch gathers from;
//   pasta_ssim_loss_backward   dloss/dx times an upstream gradient that the kernel reads from device memory.
// Only the content columns c0 .. c0 + W - 1 are read; the gradient outside them is written as 0.
#include "recon_window.h"

namespace pasta {

constexpr float SL_C1 = 4e-4f, SL_C2 = 3.6e-3f;     // (0.01 * 2)^2, (0.03 * 2)^2

// The value both images of a forward tile are centred on before the moments: the photograph at the tile's first pixel (tile
// (ty, tx) of positions starts at pixel (22 ty, 32 tx), which lies inside the image).  The variances and the covariance do not
// depend on it; near white (v about 1) they then cancel from |v - shift|^2 instead of from 1 (DESIGN 8j has both deviations).
__device__ __forceinline__ float tile_shift(const float* __restrict__ y_plane, int Wt, int ty, int tx) {
    return y_plane[(int64_t)(ty * RS_TH) * Wt + tx * RS_TW];
}

// One workgroup: one channel of one tile of 22 x 32 window positions of one image (the geometry of recon_image_stats_kernel).
// Both tiles are staged centred on the tile's shift; the row pass leaves the five moment maps in LDS, the column pass turns them
// into S = a1 a2 / (b1 b2) and, when dmaps is given, into the three maps the backward launch gathers from:
//   Ac = dS/dmx - 2 (mx - shift) B - (my - shift) C,   B = dS/dsxx = -S / b2,   C = dS/dsxy = 2 a1 / (b1 b2),
// Ac being the A of the definition with the means taken relative to the shift (the backward launch adds the rest back from the
// same shift, which it reads at the same place).  One fp64 partial per workgroup, no floating-point atomics.  One kernel with
// and without the maps, so that a value-only call returns the bits of the call that also saves them.
// xs, ys: [N, 3, H, Wt]; dmaps: [N, 3, 3, H - 10, W - 10] or null.
__global__ __launch_bounds__(256) void ssim_loss_kernel(const float* __restrict__ xs, const float* __restrict__ ys, float* __restrict__ dmaps,
                                                        double* __restrict__ partials, ReconWeights gw, int H, int Wt, int c0, int W,
                                                        int tiles_x) {
    __shared__ float ta[RS_IH * RS_LD], tb[RS_IH * RS_LD];
    __shared__ __attribute__((aligned(16))) float maps[RS_MAPS][RS_IH][RS_TW];
    __shared__ double red_f[4];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * RS_TH, x0 = tx * RS_TW;
    const int64_t plane = ((int64_t)n * 3 + ch) * H * Wt + c0;
    const float* px = xs + plane;
    const float* py = ys + plane;
    const float shift = tile_shift(py, Wt, ty, tx);

    for (int i = t; i < RS_IH * RS_IW; i += 256) {
        const int r = i / RS_IW, c = i - r * RS_IW;
        const int y = y0 + r, x = x0 + c;
        float a = 0.f, b = 0.f;
        if (y < H && x < W) {
            a = px[(int64_t)y * Wt + x] - shift;
            b = py[(int64_t)y * Wt + x] - shift;
        }
        ta[r * RS_LD + c] = a;
        tb[r * RS_LD + c] = b;
    }
    __syncthreads();

    {   // row pass: thread = (row, four neighbouring columns), 14 staged values of each image for 4 x 5 sums
        const int r = t >> 3, cg = (t & 7) * 4;
        float va[RS_K + 3], vb[RS_K + 3];
#pragma unroll
        for (int k = 0; k < RS_K + 3; k++) { va[k] = ta[r * RS_LD + cg + k]; vb[k] = tb[r * RS_LD + cg + k]; }
        float s[RS_MAPS][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float ea = 0.f, eb = 0.f, eaa = 0.f, ebb = 0.f, eab = 0.f;
#pragma unroll
            for (int k = 0; k < RS_K; k++) {
                const float w = gw.w[k], a = va[j + k], b = vb[j + k];
                const float wa = w * a, wb = w * b;
                ea += wa; eb += wb; eaa += wa * a; ebb += wb * b; eab += wa * b;
            }
            s[0][j] = ea; s[1][j] = eb; s[2][j] = eaa; s[3][j] = ebb; s[4][j] = eab;
        }
#pragma unroll
        for (int m = 0; m < RS_MAPS; m++) *reinterpret_cast<float4*>(&maps[m][r][cg]) = make_float4(s[m][0], s[m][1], s[m][2], s[m][3]);
    }
    __syncthreads();

    double ssim = 0.0;
    {   // column pass: thread = (column, three neighbouring rows), 13 rows of the five maps for 3 SSIM values
        const int c = t & 31, rq = (t >> 5) * 3;
        float e[RS_MAPS][3];
#pragma unroll
        for (int m = 0; m < RS_MAPS; m++) e[m][0] = e[m][1] = e[m][2] = 0.f;
#pragma unroll
        for (int k = 0; k < RS_K + 2; k++) {
            const int r = rq + k;                               // rq + 12 <= 33: rows 32 and 33 belong to positions past the tile
            if (r < RS_IH) {
#pragma unroll
                for (int m = 0; m < RS_MAPS; m++) {
                    const float v = maps[m][r][c];
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        if (k - j >= 0 && k - j < RS_K) e[m][j] += gw.w[k - j] * v;
                }
            }
        }
        const int Hp = H - RS_R, Wp = W - RS_R;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int r = rq + j;
            if (r < RS_TH && y0 + r < Hp && x0 + c < Wp) {
                const float mx = e[0][j] + (shift + 1.f), my = e[1][j] + (shift + 1.f);       // means of the intensities v + 1
                const float sxx = e[2][j] - e[0][j] * e[0][j], syy = e[3][j] - e[1][j] * e[1][j], sxy = e[4][j] - e[0][j] * e[1][j];
                const float a1 = 2.f * mx * my + SL_C1, a2 = 2.f * sxy + SL_C2;
                const float b1 = mx * mx + my * my + SL_C1, b2 = sxx + syy + SL_C2;
                const float inv = 1.f / (b1 * b2);
                const float S = a1 * a2 * inv;
                ssim += (double)S;
                if (dmaps) {
                    const float dmx = 2.f * my * a2 * inv - 2.f * mx * S / b1;
                    const float B = -S / b2;
                    const float C = 2.f * a1 * inv;
                    const float Ac = dmx - 2.f * e[0][j] * B - e[1][j] * C;
                    float* out = dmaps + ((int64_t)n * 3 + ch) * 3 * Hp * Wp + (int64_t)(y0 + r) * Wp + x0 + c;
                    out[0] = Ac;
                    out[(int64_t)Hp * Wp] = B;
                    out[(int64_t)2 * Hp * Wp] = C;
                }
            }
        }
    }

    // wave butterflies, then the four waves in order: the same grouping in every launch
    ssim = wave_sum(ssim);
    if ((t & 63) == 0) red_f[t >> 6] = ssim;
    __syncthreads();
    if (t == 0) partials[((int64_t)n * 3 + ch) * gridDim.x + tile] = ((red_f[0] + red_f[1]) + red_f[2]) + red_f[3];
}

// One workgroup: the partials in a fixed order (thread t takes t, t + 256, ...; then a halving tree) in fp64, and
// loss = 1 - sum / M as fp32.
__global__ __launch_bounds__(256) void ssim_loss_reduce_kernel(const double* __restrict__ partials, float* __restrict__ loss, int64_t count,
                                                               double windows) {
    __shared__ double rf[256];
    const int t = threadIdx.x;
    double f = 0.0;
    for (int64_t i = t; i < count; i += 256) f += partials[i];
    rf[t] = f;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (t < half) rf[t] += rf[t + half];
        __syncthreads();
    }
    if (t == 0) *loss = (float)(1.0 - rf[0] / windows);
}

// One workgroup: 22 x 32 PIXELS q of one channel of one image.  It stages the 32 x 42 window positions p = q - 10 .. q of the
// three maps (0 where a position is not valid), makes the two separable passes with the weights reversed -- the transpose of
// the forward window -- and writes
//   dx[q] = -(g / M) ((w (*) A)[q] + 2 (x[q] - ref) (w (*) B)[q] + (y[q] - ref) (w (*) C)[q]),   g = *grad_loss,
// where ref is the photograph at this tile's first pixel and the staged A is the forward launch's Ac brought to that reference:
// A = Ac + (2 B + C) (ref - shift of the position's forward tile).  In exact arithmetic that is the definition's
// w (*) A + 2 x w (*) B + y w (*) C; in fp32 the three terms stay of the size of their sum.  Gather form: every dx element is
// written by exactly one thread.  The tiles of the first and of the last column also write the zeros outside the crop.
__global__ __launch_bounds__(256) void ssim_loss_backward_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                                 const float* __restrict__ dmaps, const float* __restrict__ grad_loss,
                                                                 float* __restrict__ dx, ReconWeights gw, float inv_windows, int H, int Wt,
                                                                 int c0, int W, int tiles_x) {
    __shared__ float tq[3][RS_IH * RS_LD];
    __shared__ __attribute__((aligned(16))) float maps[3][RS_IH][RS_TW];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * RS_TH, x0 = tx * RS_TW;                 // the tile's first pixel: inside the image
    const int Hp = H - RS_R, Wp = W - RS_R;
    const int64_t plane = ((int64_t)n * 3 + ch) * H * Wt;
    const float* px = xs + plane + c0;
    const float* py = ys + plane + c0;
    const float* dm = dmaps + ((int64_t)n * 3 + ch) * 3 * Hp * Wp;
    const float ref = py[(int64_t)y0 * Wt + x0];

    for (int i = t; i < RS_IH * RS_IW; i += 256) {
        const int r = i / RS_IW, c = i - r * RS_IW;
        const int y = y0 - RS_R + r, x = x0 - RS_R + c;         // a window position
        float A = 0.f, B = 0.f, C = 0.f;
        if (y >= 0 && y < Hp && x >= 0 && x < Wp) {
            const int64_t at = (int64_t)y * Wp + x;
            B = dm[(int64_t)Hp * Wp + at];
            C = dm[(int64_t)2 * Hp * Wp + at];
            A = dm[at] + (2.f * B + C) * (ref - tile_shift(py, Wt, y / RS_TH, x / RS_TW));
        }
        tq[0][r * RS_LD + c] = A;
        tq[1][r * RS_LD + c] = B;
        tq[2][r * RS_LD + c] = C;
    }
    __syncthreads();

    {   // row pass: thread = (row, four neighbouring pixel columns); pixel column j gathers the staged columns j .. j + 10
        const int r = t >> 3, cg = (t & 7) * 4;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float v[RS_K + 3], s[4];
#pragma unroll
            for (int k = 0; k < RS_K + 3; k++) v[k] = tq[m][r * RS_LD + cg + k];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < RS_K; k++) acc += gw.w[RS_R - k] * v[j + k];
                s[j] = acc;
            }
            *reinterpret_cast<float4*>(&maps[m][r][cg]) = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
    __syncthreads();

    {   // column pass: thread = (column, three neighbouring pixel rows); pixel row j gathers the staged rows j .. j + 10
        const int c = t & 31, rq = (t >> 5) * 3;
        float e[3][3];
#pragma unroll
        for (int m = 0; m < 3; m++) e[m][0] = e[m][1] = e[m][2] = 0.f;
#pragma unroll
        for (int k = 0; k < RS_K + 2; k++) {
            const int r = rq + k;
            if (r < RS_IH) {
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    const float v = maps[m][r][c];
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        if (k - j >= 0 && k - j < RS_K) e[m][j] += gw.w[RS_R - (k - j)] * v;
                }
            }
        }
        const float g = *grad_loss, scale = -inv_windows;       // g last: dx is g times the rounded gradient of the loss itself
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int y = y0 + rq + j, x = x0 + c;
            if (rq + j < RS_TH && y < H && x < W) {
                const int64_t at = (int64_t)y * Wt + x;
                const float xc = px[at] - ref, yc = py[at] - ref;
                dx[plane + c0 + at] = g * (scale * (e[0][j] + 2.f * xc * e[1][j] + yc * e[2][j]));
            }
        }
    }

    // the columns outside the crop, rows of this tile: left of it by the first tile of a row, right of it by the last
    const int rows = H - y0 < RS_TH ? H - y0 : RS_TH;
    if (tx == 0)
        for (int i = t; i < rows * c0; i += 256) dx[plane + (int64_t)(y0 + i / c0) * Wt + i % c0] = 0.f;
    const int right = Wt - c0 - W;
    if (tx == tiles_x - 1)
        for (int i = t; i < rows * right; i += 256) dx[plane + (int64_t)(y0 + i / right) * Wt + c0 + W + i % right] = 0.f;
}

static int pixel_tiles(int extent, int tile) { return (extent + tile - 1) / tile; }

}  // namespace pasta

extern "C" int64_t pasta_ssim_loss_workspace(int N, int H, int W) {
    using namespace pasta;
    if (N < 1 || H < RS_K || W < RS_K) return 0;
    return (int64_t)N * 3 * recon_tiles(W, RS_TW) * recon_tiles(H, RS_TH) * (int64_t)sizeof(double);
}

#define PASTA_SSIM_SHAPE_CHECKS(what)                                                                                                 \
    PASTA_CHECK(H >= RS_K && W >= RS_K, what ": %d x %d is smaller than the %d x %d SSIM window", H, W, RS_K, RS_K);                  \
    PASTA_CHECK(N >= 1 && N <= 65535 && H <= 4096 && Wt >= 1 && Wt <= 4096 && c0 >= 0 && c0 + W <= Wt,                                \
                what ": bad shape or crop (columns %d + %d of %d)", c0, W, Wt)

extern "C" int pasta_ssim_loss(const float* x, const float* y, float* loss, float* dmaps, void* workspace, int64_t workspace_bytes, int N,
                               int H, int Wt, int c0, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(x && y && loss && workspace, "ssim_loss: null pointer");
    PASTA_SSIM_SHAPE_CHECKS("ssim_loss");
    PASTA_CHECK(workspace_bytes >= pasta_ssim_loss_workspace(N, H, W), "ssim_loss: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)pasta_ssim_loss_workspace(N, H, W));
    const int tiles_x = recon_tiles(W, RS_TW), tiles_y = recon_tiles(H, RS_TH);
    dim3 grid((unsigned)(tiles_x * tiles_y), 3u, (unsigned)N);
    hipLaunchKernelGGL(ssim_loss_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, dmaps, (double*)workspace, recon_weights(), H, Wt, c0, W,
                       tiles_x);
    if (int status = launch_status("ssim_loss")) return status;
    hipLaunchKernelGGL(ssim_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, loss,
                       (int64_t)N * 3 * tiles_x * tiles_y, (double)N * 3.0 * (H - RS_R) * (W - RS_R));
    return launch_status("ssim_loss (reduce)");
}

extern "C" int pasta_ssim_loss_backward(const float* x, const float* y, const float* dmaps, const float* grad_loss, float* dx, int N, int H,
                                        int Wt, int c0, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(x && y && dmaps && grad_loss && dx, "ssim_loss_backward: null pointer");
    PASTA_SSIM_SHAPE_CHECKS("ssim_loss_backward");
    const int tiles_x = pixel_tiles(W, RS_TW), tiles_y = pixel_tiles(H, RS_TH);
    dim3 grid((unsigned)(tiles_x * tiles_y), 3u, (unsigned)N);
    const float inv_windows = (float)(1.0 / ((double)N * 3.0 * (H - RS_R) * (W - RS_R)));
    hipLaunchKernelGGL(ssim_loss_backward_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, dmaps, grad_loss, dx, recon_weights(),
                       inv_windows, H, Wt, c0, W, tiles_x);
    return launch_status("ssim_loss_backward");
}
