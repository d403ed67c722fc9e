// Statistics of the paired-reconstruction metric (metrics/reconstruction.py): G_ema's image of a person against that person's
// photograph, and its parsing against the label map the loss trains it on.
//   pasta_recon_image_stats    per image: sum |d| and sum d^2 of the bytes test.py would write against the photograph's (exact
//                              integers), and the sum of SSIM (Wang et al. 2004: 11 x 11 Gaussian, sigma 1.5, valid positions,
//                              per RGB channel) with its window count;
//   pasta_region_image_stats   the same statistics inside a region (metrics/tryon_fidelity.py): the difference sums over the
//                              region's pixels, SSIM over the windows whose 121 pixels all lie in it; the same device code;
//   pasta_parsing_confusion    the [C, C] confusion matrix (row = label, column = arg-max of the logits) of the content columns.
// Only the content columns c0 .. c0 + W - 1 of the padded square are scored.
#include <type_traits>

#include "recon_window.h"
#include "tryon_common.h"

namespace pasta {

// ---- image statistics ----

struct ReconPartial { double ssim; int64_t sad, ssd; };
struct RegionPartial { double ssim; int64_t sad, ssd, windows, bytes; };
template <bool MASKED> using PartialOf = std::conditional_t<MASKED, RegionPartial, ReconPartial>;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One workgroup: one channel of one tile of one image.  The generated tile, quantised to test.py's bytes, and the photograph's
// are staged once, centred (byte - 127.5, exact in fp32: the products of the second moments then cancel in sigma^2 from at most
// 127.5^2 instead of 255^2); the row pass leaves the five moment maps in LDS, the column pass turns them into SSIM values.
// Every pixel's difference is counted by exactly one workgroup: the one whose SSIM positions start at it, the last tile of a
// row or column taking the halo as well.  One partial per workgroup, no floating-point atomics.
// MASKED: a pixel counts where mask != 0, and a window where all its 121 pixels do.  The region's flags are staged next to the
// images (0 outside the image) and, in a phase of its own before the moments, AND-ed over 11 columns and then over 11 rows (the
// separable AND of csrc/patch_erode.h); each thread keeps one bit per position of its column pass.  The moments and the window's
// expression are the same source in the same blocks as without a mask -- a window that counts has no pixel outside the region --
// and compile to the same fp32 instructions: a mask of ones gives the bits of the unmasked kernel (held by a test).
// photos: rows of Wr pixels, already at column r0 and this channel.
template <bool MASKED>
__global__ __launch_bounds__(256) void recon_image_stats_kernel(const float* __restrict__ images, const uint8_t* __restrict__ photos,
                                                                const uint8_t* __restrict__ mask, PartialOf<MASKED>* __restrict__ partials,
                                                                ReconWeights gw, int H, int Wt, int c0, int Wr, int r0, int Wm, int m0,
                                                                int W, int tiles_x, int tiles_y) {
    __shared__ float ta[RS_IH * RS_LD], tb[RS_IH * RS_LD];
    __shared__ __attribute__((aligned(16))) float maps[RS_MAPS][RS_IH][RS_TW];
    __shared__ __attribute__((aligned(4))) uint8_t tm[MASKED ? RS_IH * RS_LD : 4], tmr[MASKED ? RS_IH * RS_TW : 4];    // flags; their row AND
    __shared__ double red_f[4];
    __shared__ int red_i[4][MASKED ? 4 : 2];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * RS_TH, x0 = tx * RS_TW;
    const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
    const float* img = images + ((int64_t)n * 3 + ch) * H * Wt + c0;
    const uint8_t* pho = photos + ((int64_t)n * H * Wr + r0) * 3 + ch;
    const uint8_t* msk = MASKED ? mask + (int64_t)n * H * Wm + m0 : nullptr;

    int sad = 0, ssd = 0, pixels = 0, windows = 0;      // at most six pixels and three windows per thread; the last two MASKED only
    for (int i = t; i < RS_IH * RS_IW; i += 256) {
        const int r = i / RS_IW, c = i - r * RS_IW;
        const int y = y0 + r, x = x0 + c;
        float a = 0.f, b = 0.f;
        bool in = false;
        if (y < H && x < W) {
            const int g = unit_to_u8(img[(int64_t)y * Wt + x]);
            const int p = pho[((int64_t)y * Wr + x) * 3];
            a = (float)g - 127.5f;
            b = (float)p - 127.5f;
            in = !MASKED || msk[(int64_t)y * Wm + x] != 0;
            if (in && (r < RS_TH || last_y) && (c < RS_TW || last_x)) {
                const int d = g - p;
                sad += d < 0 ? -d : d;
                ssd += d * d;
                if (MASKED) pixels++;
            }
        }
        ta[r * RS_LD + c] = a;
        tb[r * RS_LD + c] = b;
        if (MASKED) tm[r * RS_LD + c] = in;
    }
    __syncthreads();

    uint32_t counted = 7;                               // bit j: position j of this thread's column pass is valid and counts
    if constexpr (MASKED) {
        {   // thread = (row, four neighbouring columns) as in the row pass: are the 11 pixels to the right all in the region?
            const int r = t >> 3, cg = (t & 7) * 4;
            uint32_t bits = 0, all = 0;
#pragma unroll
            for (int k = 0; k < RS_K + 3; k++) bits |= (uint32_t)tm[r * RS_LD + cg + k] << k;
#pragma unroll
            for (int j = 0; j < 4; j++) all |= (uint32_t)(((bits >> j) & 0x7ffu) == 0x7ffu) << (8 * j);
            *reinterpret_cast<uint32_t*>(&tmr[r * RS_TW + cg]) = all;
        }
        __syncthreads();
        {   // thread = (column, three neighbouring rows) as in the column pass: and the 11 rows below?
            const int c = t & 31, rq = (t >> 5) * 3;
            uint32_t col = 0;
#pragma unroll
            for (int k = 0; k < RS_K + 2; k++)
                if (rq + k < RS_IH) col |= (uint32_t)tmr[(rq + k) * RS_TW + c] << k;
            counted = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (rq + j < RS_TH && y0 + rq + j < H - RS_R && x0 + c < W - RS_R && ((col >> j) & 0x7ffu) == 0x7ffu) counted |= 1u << j;
            windows = __popc(counted);
        }
    }

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
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int r = rq + j;
            if (r < RS_TH && y0 + r < H - RS_R && x0 + c < W - RS_R && (counted >> j & 1u)) {
                const float C1 = 6.5025f, C2 = 58.5225f;       // (0.01 * 255)^2, (0.03 * 255)^2
                const float mx = e[0][j] + 127.5f, my = e[1][j] + 127.5f;
                const float sxx = e[2][j] - e[0][j] * e[0][j], syy = e[3][j] - e[1][j] * e[1][j], sxy = e[4][j] - e[0][j] * e[1][j];
                const float num = (2.f * mx * my + C1) * (2.f * sxy + C2);
                const float den = (mx * mx + my * my + C1) * (sxx + syy + C2);
                ssim += (double)(num / den);
            }
        }
    }

    // wave butterflies, then the four waves in order: the same grouping in every launch
    ssim = wave_sum(ssim); sad = wave_sum(sad); ssd = wave_sum(ssd);
    if (MASKED) { windows = wave_sum(windows); pixels = wave_sum(pixels); }
    if ((t & 63) == 0) {
        red_f[t >> 6] = ssim; red_i[t >> 6][0] = sad; red_i[t >> 6][1] = ssd;
        if (MASKED) { red_i[t >> 6][2] = windows; red_i[t >> 6][3] = pixels; }
    }
    __syncthreads();
    if (t == 0) {
        PartialOf<MASKED> p;
        p.ssim = ((red_f[0] + red_f[1]) + red_f[2]) + red_f[3];
        p.sad = (int64_t)red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0];
        p.ssd = (int64_t)red_i[0][1] + red_i[1][1] + red_i[2][1] + red_i[3][1];
        if constexpr (MASKED) {
            p.windows = (int64_t)red_i[0][2] + red_i[1][2] + red_i[2][2] + red_i[3][2];
            p.bytes = (int64_t)red_i[0][3] + red_i[1][3] + red_i[2][3] + red_i[3][3];      // this channel's byte of every region pixel
        }
        partials[((int64_t)n * 3 + ch) * gridDim.x + tile] = p;
    }
}

// One workgroup per image: its partials in a fixed order (thread t takes t, t + 256, ...; then a halving tree), in fp64.
// sums: [N, 3] with the window count the caller knows, or MASKED [N, 4] with the counted windows and bytes.
template <bool MASKED>
__global__ __launch_bounds__(256) void recon_image_reduce_kernel(const PartialOf<MASKED>* __restrict__ partials, int64_t* __restrict__ sums,
                                                                 double* __restrict__ ssim, int per_image, int64_t windows) {
    __shared__ double rf[256];
    __shared__ int64_t ra[256], rs[256], rw[MASKED ? 256 : 1], rb[MASKED ? 256 : 1];
    const int t = threadIdx.x, n = blockIdx.x;
    const PartialOf<MASKED>* p = partials + (int64_t)n * per_image;
    double f = 0.0;
    int64_t a = 0, s = 0, w = 0, b = 0;
    for (int i = t; i < per_image; i += 256) {
        f += p[i].ssim; a += p[i].sad; s += p[i].ssd;
        if constexpr (MASKED) { w += p[i].windows; b += p[i].bytes; }
    }
    rf[t] = f; ra[t] = a; rs[t] = s;
    if (MASKED) { rw[t] = w; rb[t] = b; }
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (t < half) {
            rf[t] += rf[t + half]; ra[t] += ra[t + half]; rs[t] += rs[t + half];
            if (MASKED) { rw[t] += rw[t + half]; rb[t] += rb[t + half]; }
        }
        __syncthreads();
    }
    if (t == 0) {
        int64_t* out = sums + (int64_t)n * (MASKED ? 4 : 3);
        out[0] = ra[0]; out[1] = rs[0]; out[2] = MASKED ? rw[0] : windows;
        if (MASKED) out[3] = rb[0];
        ssim[n] = rf[0];
    }
}

// ---- parsing confusion ----

constexpr int PC_MAX_C = 32;

// One thread per content pixel; the workgroup counts in LDS and adds its non-empty cells to the matrix with integer atomics
// (exact, so the order does not matter).
__global__ __launch_bounds__(256) void parsing_confusion_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                                unsigned long long* __restrict__ matrix, int C, int H, int Wt, int c0, int W) {
    __shared__ unsigned int hist[PC_MAX_C * PC_MAX_C];
    const int t = threadIdx.x, n = blockIdx.y;
    for (int i = t; i < C * C; i += 256) hist[i] = 0;
    __syncthreads();
    const int pix = blockIdx.x * 256 + t;
    if (pix < H * W) {
        const int y = pix / W, x = pix - y * W;
        const int64_t at = (int64_t)y * Wt + c0 + x;
        const float lab = labels[(int64_t)n * H * Wt + at];
        if (lab > -1.0f && lab < (float)C) {                    // as .long() truncates; anything else (255, C, a NaN) is ignored
            int best = -1;
            float bestv = 0.f;
            for (int c = 0; c < C; c++) {
                const float v = logits[((int64_t)n * C + c) * H * Wt + at];
                if (v == v && (best < 0 || v > bestv)) { best = c; bestv = v; }     // a NaN never wins; the lowest index on ties
            }
            atomicAdd(&hist[(int)lab * C + (best < 0 ? 0 : best)], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&matrix[i], (unsigned long long)hist[i]);
}

}  // namespace pasta

extern "C" int64_t pasta_recon_image_stats_workspace(int N, int H, int W) {
    using namespace pasta;
    if (N < 1 || H < RS_K || W < RS_K) return 0;
    return (int64_t)N * 3 * recon_tiles(W, RS_TW) * recon_tiles(H, RS_TH) * (int64_t)sizeof(ReconPartial);
}

extern "C" int pasta_recon_image_stats(const float* images, const uint8_t* photos, int64_t* sums, double* ssim, void* workspace,
                                       int64_t workspace_bytes, int N, int H, int Wt, int c0, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && photos && sums && ssim && workspace, "recon_image_stats: null pointer");
    PASTA_CHECK(H >= RS_K && W >= RS_K, "recon_image_stats: %d x %d is smaller than the %d x %d SSIM window", H, W, RS_K, RS_K);
    PASTA_CHECK(N >= 1 && N <= 65535 && H <= 4096 && Wt >= 1 && Wt <= 4096 && c0 >= 0 && c0 + W <= Wt,
                "recon_image_stats: bad shape or crop (columns %d + %d of %d)", c0, W, Wt);
    PASTA_CHECK(workspace_bytes >= pasta_recon_image_stats_workspace(N, H, W), "recon_image_stats: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)pasta_recon_image_stats_workspace(N, H, W));
    const int tiles_x = recon_tiles(W, RS_TW), tiles_y = recon_tiles(H, RS_TH);
    dim3 grid((unsigned)(tiles_x * tiles_y), 3u, (unsigned)N);
    hipLaunchKernelGGL(recon_image_stats_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, images, photos, (const uint8_t*)nullptr,
                       (ReconPartial*)workspace, recon_weights(), H, Wt, c0, W, 0, 0, 0, W, tiles_x, tiles_y);
    if (int status = launch_status("recon_image_stats")) return status;
    hipLaunchKernelGGL(recon_image_reduce_kernel<false>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const ReconPartial*)workspace, sums,
                       ssim, 3 * tiles_x * tiles_y, (int64_t)3 * (H - RS_R) * (W - RS_R));
    return launch_status("recon_image_stats (reduce)");
}

extern "C" int64_t pasta_region_image_stats_workspace(int N, int H, int W) {
    using namespace pasta;
    if (N < 1 || H < RS_K || W < RS_K) return 0;
    return (int64_t)N * 3 * recon_tiles(W, RS_TW) * recon_tiles(H, RS_TH) * (int64_t)sizeof(RegionPartial);
}

extern "C" int pasta_region_image_stats(const float* images, const uint8_t* ref, const uint8_t* mask, int64_t* sums, double* ssim,
                                        void* workspace, int64_t workspace_bytes, int N, int H, int Wt, int c0, int Wr, int r0, int Wm, int m0,
                                        int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && ref && mask && sums && ssim && workspace, "region_image_stats: null pointer");
    PASTA_CHECK(H >= RS_K && W >= RS_K, "region_image_stats: %d x %d is smaller than the %d x %d SSIM window", H, W, RS_K, RS_K);
    PASTA_CHECK(N >= 1 && N <= 65535 && H <= 4096 && Wt >= 1 && Wt <= 4096 && c0 >= 0 && c0 + W <= Wt,
                "region_image_stats: bad shape or crop of the images (columns %d + %d of %d)", c0, W, Wt);
    PASTA_CHECK(Wr >= 1 && Wr <= 4096 && r0 >= 0 && r0 + W <= Wr, "region_image_stats: bad crop of the reference (columns %d + %d of %d)", r0, W,
                Wr);
    PASTA_CHECK(Wm >= 1 && Wm <= 4096 && m0 >= 0 && m0 + W <= Wm, "region_image_stats: bad crop of the mask (columns %d + %d of %d)", m0, W, Wm);
    PASTA_CHECK(workspace_bytes >= pasta_region_image_stats_workspace(N, H, W), "region_image_stats: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)pasta_region_image_stats_workspace(N, H, W));
    const int tiles_x = recon_tiles(W, RS_TW), tiles_y = recon_tiles(H, RS_TH);
    dim3 grid((unsigned)(tiles_x * tiles_y), 3u, (unsigned)N);
    hipLaunchKernelGGL(recon_image_stats_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, images, ref, mask, (RegionPartial*)workspace,
                       recon_weights(), H, Wt, c0, Wr, r0, Wm, m0, W, tiles_x, tiles_y);
    if (int status = launch_status("region_image_stats")) return status;
    hipLaunchKernelGGL(recon_image_reduce_kernel<true>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const RegionPartial*)workspace, sums,
                       ssim, 3 * tiles_x * tiles_y, (int64_t)0);
    return launch_status("region_image_stats (reduce)");
}

extern "C" int pasta_parsing_confusion(const float* logits, const float* labels, int64_t* matrix, int N, int C, int H, int Wt, int c0, int W,
                                       void* stream) {
    using namespace pasta;
    PASTA_CHECK(logits && labels && matrix, "parsing_confusion: null pointer");
    PASTA_CHECK(C >= 1 && C <= PC_MAX_C, "parsing_confusion: %d classes (1..%d)", C, PC_MAX_C);
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && Wt >= 1 && Wt <= 4096 && W >= 1 && c0 >= 0 && c0 + W <= Wt,
                "parsing_confusion: bad shape or crop (columns %d + %d of %d)", c0, W, Wt);
    dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(parsing_confusion_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits, labels, (unsigned long long*)matrix, C, H, Wt,
                       c0, W);
    return launch_status("parsing_confusion");
}
