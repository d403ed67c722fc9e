// People of any size fitted to the canvas of their data set (this project's own rule, --fit-people: include/pasta_hip.h,
// pasta_fit_people_u8; training/tryon_batch.py's fit_batch), before the mirroring, the jitter and every preparation:
//   fit_photo_kernel   the photographs of a packed batch, resampled by PIL's 8-bit two-pass rule with taps the host has made:
//                      a workgroup owns a 16 x 64 tile of one item's canvas, runs the horizontal pass for the source rows the tile
//                      needs into LDS (the rounded bytes PIL keeps between its passes never reach HBM), then the vertical pass;
//   fit_label_kernel   the label maps: the weighted mode over the box taps' footprint with the stated tie rule.
// Both read every number of the plan on the device and hold every index inside its buffer whatever the plan says: an item whose
// record or tables are not what the host's rule makes is written as padding (photograph 255, label 0).
#include "common.h"

namespace pasta {

constexpr int FIT_RECORD = 16;              // words of an item's record in the plan (training.tryon_batch.FIT_RECORD)
constexpr int FIT_KSIZE = 17;               // taps per output position at most: bilinear at 8 source pixels per fitted one
constexpr int FIT_TILE_H = 16, FIT_TILE_W = 64;
constexpr int FIT_ROWS = 144;               // source rows a tile's 16 fitted rows can need: 8 * 16 + 2 * 8
constexpr int FIT_SIDE = 16384;

struct FitItem {
    int h, w, Hc, Wc, oy, ox;
    const int32_t *tx, *ty;                 // the axis tables' rows: (xmin, cnt, k[ksize]) per output position
    int kx, ky;                             // their ksize
    int64_t off;                            // the item's first pixel in the packed buffers
    bool ok;
};

// The table at word t of the plan: (n_out, ksize) then n_out rows of 2 + ksize words.  False unless it lies inside the plan, is
// for n_out positions and has 1..17 taps.
__device__ __forceinline__ bool fit_table(const int32_t* __restrict__ plan, int64_t words, int t, int n_out, const int32_t** rows, int* ksize) {
    if (t < 0 || (int64_t)t + 2 > words) return false;
    const int n = plan[t], k = plan[t + 1];
    if (n != n_out || k < 1 || k > FIT_KSIZE) return false;
    if ((int64_t)t + 2 + (int64_t)n * (2 + k) > words) return false;
    *rows = plan + t + 2;
    *ksize = k;
    return true;
}

// Item n of the plan with the photograph's tables (first = 6) or the label map's (first = 8), checked against the buffers.
__device__ __forceinline__ FitItem fit_item(const int32_t* __restrict__ plan, int64_t words, int64_t pixels, int n, int first) {
    const int32_t* q = plan + (int64_t)n * FIT_RECORD;
    FitItem it;
    it.h = q[0]; it.w = q[1]; it.Hc = q[2]; it.Wc = q[3]; it.oy = q[4]; it.ox = q[5];
    it.off = (int64_t)q[10] + ((int64_t)q[11] << 31);
    it.tx = it.ty = nullptr;
    it.kx = it.ky = 0;
    it.ok = it.h >= 1 && it.h <= FIT_SIDE && it.w >= 1 && it.w <= FIT_SIDE && it.Hc >= 1 && it.Hc <= FIT_SIDE && it.Wc >= 1 &&
            it.Wc <= FIT_SIDE && it.oy >= -FIT_SIDE && it.oy <= FIT_SIDE && it.ox >= -FIT_SIDE && it.ox <= FIT_SIDE && q[10] >= 0 &&
            q[11] >= 0 && it.off + (int64_t)it.h * it.w <= pixels;
    it.ok = it.ok && fit_table(plan, words, q[first], it.Wc, &it.tx, &it.kx) && fit_table(plan, words, q[first + 1], it.Hc, &it.ty, &it.ky);
    return it;
}

// Output position p of a table: its first source index and tap count, held inside 0 .. n_in, and its taps.
__device__ __forceinline__ const int32_t* fit_taps(const int32_t* __restrict__ rows, int ksize, int p, int n_in, int* first, int* count) {
    const int32_t* e = rows + (int64_t)p * (2 + ksize);
    int x = e[0], c = e[1];
    x = x < 0 ? 0 : (x > n_in - 1 ? n_in - 1 : x);
    c = c < 0 ? 0 : (c > ksize ? ksize : c);
    c = c > n_in - x ? n_in - x : c;
    *first = x;
    *count = c;
    return e + 2;
}

__device__ __forceinline__ uint32_t fit_byte(uint32_t sum) {
    const uint32_t v = sum >> 22;
    return v > 255u ? 255u : v;
}

// One launch for the photographs of a batch: item n = blockIdx.y, blockIdx.x one 16 x 64 tile of its canvas.  WIDE (W % 16 == 0,
// `out` 16-byte aligned): the tile's bytes are gathered in LDS and leave in 16-byte stores along the rows; otherwise a thread
// stores its four pixels byte by byte, the column checked.
template <bool WIDE>
__global__ __launch_bounds__(256) void fit_photo_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ plan, int64_t words,
                                                        int64_t pixels, uint8_t* __restrict__ out, int H, int W, int tiles_x) {
    __shared__ uint32_t mid[FIT_ROWS * FIT_TILE_W];                                  // the horizontal pass: R | G << 8 | B << 16
    __shared__ __align__(16) uint32_t stage[FIT_TILE_H * FIT_TILE_W * 3 / 4];        // WIDE: the tile's output bytes, 192 per row
    const int n = blockIdx.y;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int r0 = tile_y * FIT_TILE_H, c0 = tile_x * FIT_TILE_W;
    const FitItem it = fit_item(plan, words, pixels, n, 6);
    // the fitted rows and columns this tile shows, [lo, hi)
    const int fr_lo = max(r0 - it.oy, 0), fr_hi = min(min(r0 + FIT_TILE_H, H) - it.oy, it.Hc);
    const int fc_lo = max(c0 - it.ox, 0), fc_hi = min(min(c0 + FIT_TILE_W, W) - it.ox, it.Wc);
    bool any = it.ok && fr_lo < fr_hi && fc_lo < fc_hi;
    int src_lo = 0, src_hi = 0;
    if (any) {
        src_lo = it.h;
        for (int fr = fr_lo; fr < fr_hi; fr++) {
            int first, count;
            fit_taps(it.ty, it.ky, fr, it.h, &first, &count);
            src_lo = min(src_lo, first);
            src_hi = max(src_hi, first + count);
        }
        any = src_hi > src_lo && src_hi - src_lo <= FIT_ROWS;          // more rows than the limits allow: not the host's plan
    }
    if (any) {
        const uint8_t* img = images + it.off * 3;
        const int cols = fc_hi - fc_lo, cells = (src_hi - src_lo) * FIT_TILE_W;
        for (int u = threadIdx.x; u < cells; u += 256) {
            const int rr = u >> 6, cc = u & (FIT_TILE_W - 1);
            if (cc >= cols) continue;
            int first, count;
            const int32_t* k = fit_taps(it.tx, it.kx, fc_lo + cc, it.w, &first, &count);
            const uint8_t* p = img + ((int64_t)(src_lo + rr) * it.w + first) * 3;
            uint32_t s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
            for (int j = 0; j < count; j++) {
                const uint32_t kk = (uint32_t)k[j];
                s0 += p[3 * j] * kk;
                s1 += p[3 * j + 1] * kk;
                s2 += p[3 * j + 2] * kk;
            }
            mid[u] = fit_byte(s0) | fit_byte(s1) << 8 | fit_byte(s2) << 16;
        }
    }
    __syncthreads();
    const int ry = threadIdx.x >> 4, g = threadIdx.x & 15;
    const int r = r0 + ry, fr = r - it.oy;
    const bool row_in = any && fr >= fr_lo && fr < fr_hi;
    int y_first = 0, y_count = 0;
    const int32_t* ky = nullptr;
    if (row_in) ky = fit_taps(it.ty, it.ky, fr, it.h, &y_first, &y_count);
    uint32_t px[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int fc = c0 + 4 * g + q - it.ox;
        uint32_t v = 0x00ffffffu;
        if (row_in && fc >= fc_lo && fc < fc_hi) {
            const uint32_t* m = mid + (y_first - src_lo) * FIT_TILE_W + (fc - fc_lo);
            uint32_t s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
            for (int j = 0; j < y_count; j++) {
                const uint32_t t = m[j * FIT_TILE_W], kk = (uint32_t)ky[j];
                s0 += (t & 255u) * kk;
                s1 += ((t >> 8) & 255u) * kk;
                s2 += (t >> 16) * kk;
            }
            v = fit_byte(s0) | fit_byte(s1) << 8 | fit_byte(s2) << 16;
        }
        px[q] = v;
    }
    if constexpr (WIDE) {
        uint32_t* s = stage + ry * (FIT_TILE_W * 3 / 4) + g * 3;
        s[0] = px[0] | (px[1] & 0xffu) << 24;
        s[1] = (px[1] >> 8) | (px[2] & 0xffffu) << 16;
        s[2] = (px[2] >> 16) | px[3] << 8;
        __syncthreads();
        if (threadIdx.x < FIT_TILE_H * 12) {
            const int row = threadIdx.x / 12, chunk = threadIdx.x - row * 12;
            const int64_t at = (int64_t)c0 * 3 + chunk * 16;                         // byte of the canvas row
            if (r0 + row < H && at < (int64_t)W * 3)
                *reinterpret_cast<uint4*>(out + ((int64_t)n * H + r0 + row) * W * 3 + at) =
                    *reinterpret_cast<const uint4*>(stage + row * (FIT_TILE_W * 3 / 4) + chunk * 4);
        }
    } else {
        if (r >= H) return;
        uint8_t* d = out + (((int64_t)n * H + r) * W + c0 + 4 * g) * 3;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (c0 + 4 * g + q >= W) break;
            d[3 * q] = (uint8_t)(px[q] & 255u);
            d[3 * q + 1] = (uint8_t)((px[q] >> 8) & 255u);
            d[3 * q + 2] = (uint8_t)(px[q] >> 16);
        }
    }
}

// The label of fitted pixel (fr, fc): the label of greatest weight over the box taps' footprint, the weight of a label the int64
// sum of ky[i] * kx[j] over its pixels.  The labels present go into a 256-bit set first, and the sums are formed per present label
// (one label: no sums at all).  Ties: the label of source pixel (((2 fr + 1) h) / (2 Hc), ((2 fc + 1) w) / (2 Wc)) when it is among
// the tied, else the smallest tied label.
__device__ __forceinline__ uint32_t fit_label_pixel(const uint8_t* __restrict__ lab, const FitItem& it, int fr, int fc) {
    int y_first, y_count, x_first, x_count;
    const int32_t* ky = fit_taps(it.ty, it.ky, fr, it.h, &y_first, &y_count);
    const int32_t* kx = fit_taps(it.tx, it.kx, fc, it.w, &x_first, &x_count);
    const int cy = min((int)(((2 * (int64_t)fr + 1) * it.h) / (2 * (int64_t)it.Hc)), it.h - 1);
    const int cx = min((int)(((2 * (int64_t)fc + 1) * it.w) / (2 * (int64_t)it.Wc)), it.w - 1);
    const uint32_t centre = lab[(int64_t)cy * it.w + cx];
    uint64_t present[4] = {0, 0, 0, 0};
    for (int i = 0; i < y_count; i++) {
        const uint8_t* row = lab + (int64_t)(y_first + i) * it.w + x_first;
        for (int j = 0; j < x_count; j++) {
            const uint32_t L = row[j];
            const uint64_t bit = 1ull << (L & 63u);
#pragma unroll
            for (int q = 0; q < 4; q++) present[q] |= (L >> 6) == (uint32_t)q ? bit : 0ull;
        }
    }
    const int labels = __popcll(present[0]) + __popcll(present[1]) + __popcll(present[2]) + __popcll(present[3]);
    if (labels == 0) return centre;                                          // no tap at all: not the host's plan
    int64_t best = -1, at_centre = 0;
    uint32_t winner = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint64_t todo = present[q];
        while (todo) {
            const uint32_t L = 64u * q + (uint32_t)(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1;
            if (labels == 1) return L;
            int64_t sum = 0;
            for (int i = 0; i < y_count; i++) {
                const uint8_t* row = lab + (int64_t)(y_first + i) * it.w + x_first;
                int64_t across = 0;
                for (int j = 0; j < x_count; j++) across += row[j] == L ? (int64_t)kx[j] : 0;
                sum += across * (int64_t)ky[i];
            }
            if (sum > best) { best = sum; winner = L; }
            if (L == centre) at_centre = sum;
        }
    }
    return at_centre == best ? centre : winner;
}

// One launch for the label maps of a batch: item n = blockIdx.y, a thread owns PX consecutive pixels of a canvas row.  WIDE
// (W % 16 == 0, `out` 16-byte aligned): 16 pixels and one 16-byte store; otherwise one pixel.
template <bool WIDE>
__global__ __launch_bounds__(256) void fit_label_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ plan, int64_t words,
                                                        int64_t pixels, uint8_t* __restrict__ out, int H, int W) {
    constexpr int PX = WIDE ? 16 : 1;
    const int n = blockIdx.y;
    const int cw = W / PX;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= H * cw) return;
    const int r = t / cw, x0 = (t - r * cw) * PX;
    const FitItem it = fit_item(plan, words, pixels, n, 8);
    const uint8_t* lab = labels + it.off;
    const int fr = r - it.oy;
    const bool row_in = it.ok && fr >= 0 && fr < it.Hc;
    uint8_t* d = out + ((int64_t)n * H + r) * W + x0;
    if constexpr (WIDE) {
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int p = 0; p < 16; p++) {
            const int fc = x0 + p - it.ox;
            const uint32_t v = row_in && fc >= 0 && fc < it.Wc ? fit_label_pixel(lab, it, fr, fc) : 0u;
            const uint32_t s = v << (8 * (p & 3));
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] |= (p >> 2) == q ? s : 0u;
        }
        *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int fc = x0 - it.ox;
        *d = (uint8_t)(row_in && fc >= 0 && fc < it.Wc ? fit_label_pixel(lab, it, fr, fc) : 0u);
    }
}

}  // namespace pasta

extern "C" int pasta_fit_people_u8(const uint8_t* images, const uint8_t* labels, int64_t pixels, const int32_t* plan, int64_t plan_words,
                                   uint8_t* image_out, uint8_t* parsing_out, int N, int H, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && labels && plan && image_out && parsing_out, "fit_people_u8: null pointer");
    PASTA_CHECK(image_out != images && parsing_out != labels, "fit_people_u8: an output is its input (the entry is out of place)");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= FIT_SIDE && W >= 1 && W <= FIT_SIDE, "fit_people_u8: bad shape (N %d, %d x %d)", N, H, W);
    PASTA_CHECK(pixels >= 1, "fit_people_u8: the packed buffers hold %lld pixels", (long long)pixels);
    PASTA_CHECK(plan_words >= (int64_t)N * FIT_RECORD && plan_words <= 0x7fffffffLL,
                "fit_people_u8: a plan of %lld words for %d items (a record is %d words; at most 2^31 - 1)", (long long)plan_words, N, FIT_RECORD);
    const int tiles_x = (W + FIT_TILE_W - 1) / FIT_TILE_W, tiles_y = (H + FIT_TILE_H - 1) / FIT_TILE_H;
    dim3 tiles((unsigned)(tiles_x * tiles_y), (unsigned)N);
    if (W % 16 == 0 && (uintptr_t)image_out % 16 == 0)
        hipLaunchKernelGGL(fit_photo_kernel<true>, tiles, dim3(256), 0, (hipStream_t)stream, images, plan, plan_words, pixels, image_out, H, W, tiles_x);
    else
        hipLaunchKernelGGL(fit_photo_kernel<false>, tiles, dim3(256), 0, (hipStream_t)stream, images, plan, plan_words, pixels, image_out, H, W, tiles_x);
    int status = launch_status("fit_people_u8 (photographs)");
    if (status != 0) return status;
    const bool wide = W % 16 == 0 && (uintptr_t)parsing_out % 16 == 0;
    const int64_t threads = (int64_t)H * (W / (wide ? 16 : 1));                     // <= 2^28: an int in the kernel
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N);
    if (wide)
        hipLaunchKernelGGL(fit_label_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, labels, plan, plan_words, pixels, parsing_out, H, W);
    else
        hipLaunchKernelGGL(fit_label_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, labels, plan, plan_words, pixels, parsing_out, H, W);
    return launch_status("fit_people_u8 (label maps)");
}
