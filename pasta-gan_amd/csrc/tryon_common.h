// Device helpers of the try-on preparation shared by csrc/tryon_inputs.hip (the training set) and csrc/tryon_pairs.hip (both sets
// of test pairs): separately rounded arithmetic, the restated rleFrPoly fill of a quadrilateral, the palm rule with its box
// dilations, torch's x / 127.5 - 1 and test.py's conversion of a generated value to a byte (also csrc/recon_metrics.hip), the
// pixel of a padded square, the per-pixel body of the assemble kernels, the erase rule with its restated cv2.resize and the
// per-pixel body of the two training sets' assemble kernels, four-pixel loads and stores (also csrc/train_grid.hip) and the copy
// of an entry's output-pointer array.
#pragma once
#include "common.h"

namespace pasta {

// The library is compiled with -ffp-contract=fast, which fuses a * b + c into one fma whatever a pragma says.  The polygon,
// resize and float-conversion arithmetic below must round every product on its own (as the C, numpy and torch expressions it
// restates do): tr_rounded() makes the product a value the compiler cannot fuse into the next addition.
__device__ __forceinline__ float tr_rounded(float x) { __asm__ volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ double tr_rounded(double x) { __asm__ volatile("" : "+v"(x)); return x; }

// ---- palm mask ----

constexpr int PALM_S_MAX = 512;     // the largest square (one thread per column; the 512 x 320 set's 512 x 512)
constexpr int PALM_BAND = 16;       // output rows per block
constexpr int PALM_SEGS = 4;        // left upper arm, left forearm, right upper arm, right forearm

// rleFrPoly's boundary points: u = t + xs, v = (int)(ys + s * t + .5) (dx >= dy), or v = t + ys, u = (int)(xs + s * t + .5)
__device__ __forceinline__ int rle_round(double a, double s, int t) { return (int)(a + tr_rounded(s * (double)t) + .5); }

// The y boundary of edge (xs, ys) -> (xe, ye) (5x upsampled integers) at pixel column X: the smaller v of the two consecutive
// boundary points whose u are 5X + 2 and 5X + 3, turned into the row where the run toggles; -1 when the edge does not cross.
__device__ inline int rle_edge_crossing(int xs, int ys, int xe, int ye, int X, int h) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    const int u0 = 5 * X + 2;
    int vmin;
    if (dx >= dy) {
        if (dx == 0) return -1;
        const double s = (double)(ye - ys) / dx;
        if (u0 < xs || u0 + 1 > xs + dx) return -1;
        const int t = u0 - xs;
        const int v1 = rle_round(ys, s, t), v2 = rle_round(ys, s, t + 1);
        vmin = v1 < v2 ? v1 : v2;
    } else {
        const double s = (double)(xe - xs) / dy;
        const int ua = rle_round(xs, s, 0), ub = rle_round(xs, s, dy);
        const bool up = ub >= ua;
        if (up ? !(ua <= u0 && ub >= u0 + 1) : !(ua >= u0 + 1 && ub <= u0)) return -1;
        int lo = 1, hi = dy;                   // the first t past the step: u(t) >= u0 + 1 (rising) or u(t) <= u0 (falling)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int u = rle_round(xs, s, mid);
            if (up ? u >= u0 + 1 : u <= u0) hi = mid; else lo = mid + 1;
        }
        vmin = ys + lo - 1;
    }
    double yd = ((double)vmin + .5) / 5 - .5;
    if (yd < 0) yd = 0; else if (yd > h) yd = h;
    return (int)ceil(yd);
}

// Fill of the quadrilateral `q` (4 corners, x then y, doubles) at column X: up to two runs [r[0], r[1]) and [r[2], r[3]).
__device__ inline void rle_column_runs(const double* __restrict__ q, int X, int h, int16_t* r) {
    int x[5], y[5];
    for (int j = 0; j < 4; j++) { x[j] = (int)(tr_rounded(5.0 * q[2 * j]) + .5); y[j] = (int)(tr_rounded(5.0 * q[2 * j + 1]) + .5); }
    x[4] = x[0]; y[4] = y[0];
    int c[4], k = 0;
    for (int j = 0; j < 4; j++) {
        const int v = rle_edge_crossing(x[j], y[j], x[j + 1], y[j + 1], X, h);
        if (v >= 0) {                          // insertion into the sorted list
            int i = k++;
            while (i > 0 && c[i - 1] > v) { c[i] = c[i - 1]; i--; }
            c[i] = v;
        }
    }
    for (int i = k; i < 4; i++) c[i] = h;     // an odd count toggles to the end of the column
    for (int i = 0; i < 4; i++) r[i] = (int16_t)c[i];
}

__device__ __forceinline__ bool dilated_hit(const int16_t (*runs)[4], int X, int y, int lo, int hi, int S) {
    const int x0 = X - lo < 0 ? 0 : X - lo, x1 = X + hi > S - 1 ? S - 1 : X + hi;
    const int y0 = y - lo, y1 = y + hi;
    for (int xx = x0; xx <= x1; xx++) {
        const int16_t* r = runs[xx];
        if ((r[0] < r[1] && r[0] <= y1 && r[1] - 1 >= y0) || (r[2] < r[3] && r[2] <= y1 && r[3] - 1 >= y0)) return true;
    }
    return false;
}

// The palm rule for one band of PALM_BAND rows of one sample on an S x S square (blockIdx.x = band, blockIdx.y = sample, S
// threads = columns): each fill is dilated with the box of offsets -u_lo..u_hi (upper arm) or -b_lo..b_hi (forearm); runs: the
// block's [PALM_SEGS][S][4] LDS array.
__device__ __forceinline__ void palm_mask_band(const uint8_t* __restrict__ parsing, const double* __restrict__ quads,
                                               const uint8_t* __restrict__ present, uint8_t* __restrict__ out, int S, int W, int lp,
                                               int u_lo, int u_hi, int b_lo, int b_hi, int16_t (*runs)[4]) {
    const int n = blockIdx.y;
    const int X = threadIdx.x;
    const uint8_t* pres = present + n * PALM_SEGS;
    for (int sgm = 0; sgm < PALM_SEGS; sgm++)
        if (pres[sgm]) rle_column_runs(quads + ((int64_t)n * PALM_SEGS + sgm) * 8, X, S, runs[sgm * S + X]);
    __syncthreads();
    const uint8_t* lab = parsing + (int64_t)n * S * W;
    for (int yy = 0; yy < PALM_BAND; yy++) {
        const int y = blockIdx.x * PALM_BAND + yy;
        const int c = X - lp;
        const int label = (c >= 0 && c < W) ? lab[(int64_t)y * W + c] : 0;
        int palm = 0;
        if (label == 14 || label == 15) {     // hand: left = 14 (segments 0, 1), right = 15 (segments 2, 3)
            const int s0 = label == 14 ? 0 : 2;
            // a missing segment is an all-ones mask
            const bool up = !pres[s0] || dilated_hit(runs + s0 * S, X, y, u_lo, u_hi, S);
            const bool bottom = !pres[s0 + 1] || dilated_hit(runs + (s0 + 1) * S, X, y, b_lo, b_hi, S);
            palm = !up && !bottom;
        }
        out[((int64_t)n * S + y) * S + X] = (uint8_t)palm;
    }
}

__device__ __forceinline__ float to_unit(int v) {           // torch's x / 127.5 - 1 on the GPU: x * (1 / 127.5f) - 1
    const float inv = 1.0f / 127.5f;
    return tr_rounded((float)v * inv) - 1.0f;
}

// test.py:133-137 on fp32: (x + 1.0) * 127.5 with each operation rounded on its own, clip to [0, 255], truncation.  A NaN
// becomes 0 (numpy leaves its uint8 conversion undefined).
__device__ __forceinline__ uint8_t unit_to_u8(float x) {
    const float v = tr_rounded(x + 1.0f) * 127.5f;
    return v != v ? 0 : (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// ---- the padded square and the tensors G takes ----

// Pixel `pix` of sample n's padded H x H square, whose W-wide image has lp columns of padding to its left: row y and column c
// of the unpadded image, whether the pixel lies inside it, and the index of its pixel (n, y, c) there.
struct SquarePixel { int y, c; bool inside; int64_t src; };
__device__ __forceinline__ SquarePixel square_pixel(int n, int pix, int H, int W, int lp) {
    const int y = pix / H, c = pix - y * H - lp;
    return {y, c, c >= 0 && c < W, (int64_t)n * H * W + (int64_t)y * W + c};
}

// Every fp32 tensor an assemble entry may write; an entry sets those of its KEYS and leaves the others null.
struct TryonOut {
    float *image, *clothes, *clothes_lower, *gt_parsing, *style_input, *retain, *pose, *denorm_upper_input, *denorm_lower_input,
          *denorm_upper_mask, *denorm_lower_mask;
};

// outputs[i] -> *fields[i] for the `count` tensors of an entry; the index of the first null output, -1 when there is none.
inline int take_outputs(float* const* outputs, float** const* fields, int count) {
    for (int i = 0; i < count; i++) {
        if (!outputs[i]) return i;
        *fields[i] = outputs[i];
    }
    return -1;
}

// Pixel `pix` of sample n of what every data set gives G: `ret` (the caller's retain value per channel) into retain and
// pose[3..5], the stick figure into pose[0..2], the two denormalised inputs (times keep, 0 or 1) and their masks.  stick, den_u
// and den_l point at the pixel's three bytes.  numpy sums uint8 in a wider type, so the masks' channel sums do not wrap.
__device__ __forceinline__ void tryon_pixel(const TryonOut& o, int n, int pix, int HH, const float* ret, const uint8_t* __restrict__ stick,
                                            const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l, int keep) {
    const int64_t p = (int64_t)n * HH + pix;
    int s[3], u[3], l[3], su = 0, sl = 0;
    for (int ch = 0; ch < 3; ch++) {           // every load before the first store
        s[ch] = stick[ch];
        u[ch] = den_u[ch] * keep; l[ch] = den_l[ch] * keep;
        su += u[ch]; sl += l[ch];
    }
    for (int ch = 0; ch < 3; ch++) {
        const int64_t oc = ((int64_t)n * 3 + ch) * HH + pix;
        o.retain[oc] = ret[ch];
        o.pose[((int64_t)n * 6 + ch) * HH + pix] = to_unit(s[ch]);
        o.pose[((int64_t)n * 6 + 3 + ch) * HH + pix] = ret[ch];
        o.denorm_upper_input[oc] = to_unit(u[ch]);
        o.denorm_lower_input[oc] = to_unit(l[ch]);
    }
    o.denorm_upper_mask[p] = su > 0 ? 1.f : 0.f;
    o.denorm_lower_mask[p] = sl > 0 ? 1.f : 0.f;
}

// ---- the training sets: erase mask and the photograph ----

// cv2.resize(INTER_LINEAR) on uint8, one axis: source index and the two 11-bit coefficients of destination index d.
__device__ __forceinline__ void resize_taps(int d, double scale, int size, bool clamp_coord, int& s0, int& s1, int& a0, int& a1) {
    float f = (float)(tr_rounded(((double)d + 0.5) * scale) - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp_coord) {                         // columns: coordinates outside the source are pinned with weight (1, 0)
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= size - 1) { f = 0.f; s = size - 1; }
    }
    a0 = (int)rintf((1.f - f) * 2048.f);
    a1 = (int)rintf(f * 2048.f);
    s0 = s < 0 ? 0 : s > size - 1 ? size - 1 : s;          // rows: the row index is clamped, the weights are kept
    s1 = s + 1 < 0 ? 0 : s + 1 > size - 1 ? size - 1 : s + 1;
}

// Pixel `pix` of sample n of what both training sets give the loop beyond tryon_pixel: the erase mask
// erase = (arm_a + arm_b + resize(erase mask, H x H)) in uint8 (wrapping) > 0, which zeroes the two denormalised inputs, the
// photograph (real_img = o.image), retain = real_img * mask - (1 - mask) from the 0 / 1 retain mask, and gt_parsing.
// arm_a, arm_b: the sample's two [H, H] arm-part masks; erase_src [N, mh_max, mw_max] with the sample's own size in erase_hw.
__device__ __forceinline__ void train_pixel(const TryonOut& o, int n, int pix, int H, int W, int lp, const uint8_t* __restrict__ image,
                                            const uint8_t* __restrict__ stick, const uint8_t* __restrict__ retain_mask,
                                            const uint8_t* __restrict__ gt, const uint8_t* __restrict__ den_u,
                                            const uint8_t* __restrict__ den_l, const uint8_t* __restrict__ arm_a,
                                            const uint8_t* __restrict__ arm_b, const uint8_t* __restrict__ erase_src,
                                            const int32_t* __restrict__ erase_hw, int mh_max, int mw_max) {
    const int HH = H * H;
    const SquarePixel s = square_pixel(n, pix, H, W, lp);
    const int y = s.y, x = s.c + lp;
    const int64_t p = (int64_t)n * HH + pix;

    const int mh = erase_hw[2 * n], mw = erase_hw[2 * n + 1];
    int sx0, sx1, ax0, ax1, sy0, sy1, by0, by1;
    resize_taps(x, (double)mw / H, mw, true, sx0, sx1, ax0, ax1);
    resize_taps(y, (double)mh / H, mh, false, sy0, sy1, by0, by1);
    const uint8_t* m = erase_src + (int64_t)n * mh_max * mw_max;
    const int r0 = m[(int64_t)sy0 * mw_max + sx0] * ax0 + m[(int64_t)sy0 * mw_max + sx1] * ax1;
    const int r1 = m[(int64_t)sy1 * mw_max + sx0] * ax0 + m[(int64_t)sy1 * mw_max + sx1] * ax1;
    int rs = (int)(((int64_t)r0 * by0 + (int64_t)r1 * by1 + (1 << 21)) >> 22);
    rs = rs < 0 ? 0 : rs > 255 ? 255 : rs;
    const int sum8 = (arm_a[pix] + arm_b[pix] + rs) & 255;
    const int keep = sum8 > 0 ? 0 : 1;

    const int rm = retain_mask[p];
    const float label = (float)gt[p];
    float real[3], ret[3];
    for (int ch = 0; ch < 3; ch++) {           // real_img is the photograph; retain = real_img * mask - (1 - mask) from the 0 / 1 mask
        real[ch] = to_unit(s.inside ? image[s.src * 3 + ch] : 255);
        ret[ch] = tr_rounded((float)rm * real[ch]) - (float)(uint8_t)(1 - rm);
    }
    tryon_pixel(o, n, pix, HH, ret, stick + p * 3, den_u + p * 3, den_l + p * 3, keep);
    for (int ch = 0; ch < 3; ch++) o.image[((int64_t)n * 3 + ch) * HH + pix] = real[ch];
    o.gt_parsing[p] = label;
}

// ---- four pixels per thread ----

struct Px4 { uint8_t v[12]; };      // four RGB pixels of a uint8 HWC image

__device__ __forceinline__ Px4 load_px4(const uint8_t* __restrict__ p) {     // p is 4-byte aligned: pixel index a multiple of 4
    union { uint3 w; Px4 px; } u;
    u.w = *reinterpret_cast<const uint3*>(p);
    return u.px;
}

__device__ __forceinline__ void store4(float* __restrict__ p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

}  // namespace pasta
