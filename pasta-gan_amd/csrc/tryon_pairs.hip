// Per-batch preparation of the try-on TEST pairs on the GPU (row f4, UvitonDatasetV19_test._load_raw_image / normalize /
// __getitem__, training/dataset.py:1085-1525, and test.py:104-150), which the reference runs per sample on the host in four
// loader processes with OpenCV, pycocotools and skimage:
//   pasta_palm_mask_box_u8           the palm mask with both box sizes as arguments (25 / 15 here, :1240-1253), and
//                                    pasta_palm_mask_square_u8 with the side of the square as well (512 for the 512 x 320 set);
//   pasta_tryon_pair_masks_u8        retain image, the person's lower garment and the donor's upper garment (:1105-1141);
//   pasta_patch_composite_eroded_u8  the warp-back composite with cv2.erode(5 x 5) of the mask before the == 255 test
//                                    (:1480-1492);
//   pasta_tryon_pair_assemble        __getitem__ (:1502-1525) and test.py's conversions (:104-117) into the seven fp32 tensors;
//   pasta_images_to_u8               test.py's (x + 1) * 127.5, crop, clip and uint8 truncation (:133-137).
// The forward warps are csrc/patches.hip's pasta_warp_perspective_u8 and the stick figures tryon_inputs.hip's stick-figure
// entry.  Where the test set differs from the training preparation (the six rules of include/pasta_hip.h): two people (the
// donor's upper garment with the donor's key points, the person's lower garment with the person's), the person's M_inv for
// every part, an eroded mask for parts 0-5, a 15 x 15 forearm box, lower garment = labels 6, 9, 12, and key points shifted by
// the padding in float64 on the host.  Every entry does a whole batch in one launch.
#include "common.h"
#include "tryon_common.h"

#pragma clang fp contract(off)      // the warp-back coordinates must round as csrc/patches.hip's do
#include "patch_erode.h"

namespace pasta {

// ---- palm mask with the box sizes as arguments ----

__global__ __launch_bounds__(PALM_S_MAX) void palm_mask_box_kernel(const uint8_t* __restrict__ parsing, const double* __restrict__ quads,
                                                                   const uint8_t* __restrict__ present, uint8_t* __restrict__ out, int S,
                                                                   int W, int lp, int k_upper, int k_lower) {
    extern __shared__ int16_t runs[][4];        // [PALM_SEGS][S][4]: 8 KB at 256, 16 KB at 512
    // a k x k box with cv2's default anchor k / 2: offsets -(k / 2) .. k - 1 - k / 2
    palm_mask_band(parsing, quads, present, out, S, W, lp, k_upper / 2, k_upper - 1 - k_upper / 2, k_lower / 2, k_lower - 1 - k_lower / 2, runs);
}

// ---- label masks of a pair ----

__global__ __launch_bounds__(256) void tryon_pair_masks_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                               const uint8_t* __restrict__ palm, const uint8_t* __restrict__ d_image,
                                                               const uint8_t* __restrict__ d_parsing, uint8_t* __restrict__ retain_img,
                                                               uint8_t* __restrict__ lower_img, uint8_t* __restrict__ lower_mask,
                                                               uint8_t* __restrict__ upper_img, uint8_t* __restrict__ upper_mask, int H, int W,
                                                               int lp) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * H) return;
    const int y = pix / H, c = pix - y * H - lp;
    const bool inside = c >= 0 && c < W;
    const int64_t src = (int64_t)n * H * W + (int64_t)y * W + c;
    const int L = inside ? parsing[src] : 0, D = inside ? d_parsing[src] : 0;
    const int64_t o = (int64_t)n * H * H + pix;
    const int keep = (L == 18 || L == 19) + palm[o] + (L == 1 || L == 2 || L == 4 || L == 13);      // shoes + palm + head
    const int low = L == 6 || L == 9 || L == 12;                                                    // rule 5: label 6 too
    const int up = D == 5 || D == 6 || D == 7;                                                      // the donor's
    for (int ch = 0; ch < 3; ch++) {
        const int v = inside ? image[src * 3 + ch] : 255, dv = inside ? d_image[src * 3 + ch] : 255;
        retain_img[o * 3 + ch] = (uint8_t)(keep * v);
        lower_img[o * 3 + ch] = (uint8_t)(low * v);
        lower_mask[o * 3 + ch] = (uint8_t)(low * 255);
        upper_img[o * 3 + ch] = (uint8_t)(up * dv);
        upper_mask[o * 3 + ch] = (uint8_t)(up * 255);
    }
}

// ---- eroded composite ----

// The tile work is csrc/patch_erode.h's (shared with the snapshot grid's indexed composite); here part k of sample n is item n * P + k.
__global__ __launch_bounds__(256) void patch_composite_eroded_kernel(const uint8_t* __restrict__ patches, const uint8_t* __restrict__ masks,
                                                                     const double* __restrict__ minv, const uint8_t* __restrict__ valid,
                                                                     uint8_t* __restrict__ out, uint8_t* __restrict__ part_mask, int P, int ph,
                                                                     int pw, int H, int W, int r, int tiles_x) {
    __shared__ uint8_t flags[ER_S * ER_S];
    __shared__ uint8_t rows[ER_S * ER_T];
    const int n = blockIdx.y;
    const auto part_of = [=](int k) {
        const int64_t item = (int64_t)n * P + k;
        return ErPart{patches + item * ph * pw * 3, valid[item] ? masks + item * ph * pw * 3 : nullptr, minv + item * 9};
    };
    composite_eroded_tile(part_of, out + (int64_t)n * H * W * 3, part_mask ? part_mask + (int64_t)n * P * H * W : nullptr, P, ph, pw, H, W, r,
                          blockIdx.x, tiles_x, flags, rows);
}

// ---- the seven tensors G takes ----

struct PairOut {
    float *retain, *pose, *style_input, *denorm_upper_input, *denorm_lower_input, *denorm_upper_mask, *denorm_lower_mask;
};

__global__ __launch_bounds__(256) void tryon_pair_assemble_kernel(const uint8_t* __restrict__ retain_img, const uint8_t* __restrict__ stick,
                                                                  const uint8_t* __restrict__ patches, const uint8_t* __restrict__ stick_patches,
                                                                  const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                                  PairOut o, int H, int P, int ph, int pw) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HH) {                // style_input = cat(norm_img, norm_pose): channel 3k + c of part k, patches then stick patches
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int CP = 3 * P;
        for (int ch = 0; ch < 2 * CP; ch++) {
            const int cc = ch < CP ? ch : ch - CP, k = cc / 3, c = cc - 3 * k;
            const uint8_t* src = ch < CP ? patches : stick_patches;
            o.style_input[((int64_t)n * 2 * CP + ch) * ph * pw + q] = to_unit(src[(((int64_t)n * P + k) * ph * pw + q) * 3 + c]);
        }
        return;
    }
    const int64_t p = (int64_t)n * HH + pix;
    int su = 0, sl = 0;
    for (int ch = 0; ch < 3; ch++) {
        const int64_t oc = ((int64_t)n * 3 + ch) * HH + pix;
        const float ret = to_unit(retain_img[p * 3 + ch]);
        o.retain[oc] = ret;
        o.pose[((int64_t)n * 6 + ch) * HH + pix] = to_unit(stick[p * 3 + ch]);
        o.pose[((int64_t)n * 6 + 3 + ch) * HH + pix] = ret;
        const int u = den_u[p * 3 + ch], l = den_l[p * 3 + ch];
        su += u; sl += l;                                       // numpy sums uint8 in a wider type: no wrap
        o.denorm_upper_input[oc] = to_unit(u);
        o.denorm_lower_input[oc] = to_unit(l);
    }
    o.denorm_upper_mask[p] = su > 0 ? 1.f : 0.f;
    o.denorm_lower_mask[p] = sl > 0 ? 1.f : 0.f;
}

// ---- generated images to uint8 ----

// test.py:133-137 on fp32, per value csrc/tryon_common.h's unit_to_u8.
__global__ __launch_bounds__(256) void images_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int H, int Wt, int c0,
                                                           int W) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    uint8_t* o = dst + ((int64_t)n * H * W + pix) * 3;
    for (int ch = 0; ch < 3; ch++) o[ch] = unit_to_u8(src[(((int64_t)n * 3 + ch) * H + y) * Wt + c0 + x]);
}

}  // namespace pasta

extern "C" int pasta_palm_mask_square_u8(const uint8_t* parsing, const double* quads, const uint8_t* present, uint8_t* out, int N, int S,
                                         int W, int k_upper, int k_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(parsing && quads && present && out, "palm_mask_square_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && S >= PALM_BAND && S <= PALM_S_MAX && S % PALM_BAND == 0 && W >= 1 && W <= S,
                "palm_mask_square_u8: bad shape (the padded square: a multiple of %d up to %d)", PALM_BAND, PALM_S_MAX);
    PASTA_CHECK(k_upper >= 1 && k_upper <= S && k_lower >= 1 && k_lower <= S, "palm_mask_square_u8: box sizes %d, %d (1..%d)", k_upper,
                k_lower, S);
    dim3 grid((unsigned)(S / PALM_BAND), (unsigned)N);
    hipLaunchKernelGGL(palm_mask_box_kernel, grid, dim3(S), (size_t)PALM_SEGS * S * 4 * sizeof(int16_t), (hipStream_t)stream, parsing, quads,
                       present, out, S, W, (S - W) / 2, k_upper, k_lower);
    return launch_status("palm_mask_square_u8");
}

extern "C" int pasta_palm_mask_box_u8(const uint8_t* parsing, const double* quads, const uint8_t* present, uint8_t* out, int N, int H,
                                      int W, int k_upper, int k_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(H == PALM_S, "palm_mask_box_u8: bad shape (the padded square is 256 x 256)");
    return pasta_palm_mask_square_u8(parsing, quads, present, out, N, H, W, k_upper, k_lower, stream);
}

extern "C" int pasta_tryon_pair_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, const uint8_t* donor_image,
                                         const uint8_t* donor_parsing, uint8_t* retain_img, uint8_t* lower_img, uint8_t* lower_mask,
                                         uint8_t* upper_img, uint8_t* upper_mask, int N, int H, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && palm && donor_image && donor_parsing && retain_img && lower_img && lower_mask && upper_img && upper_mask,
                "tryon_pair_masks_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H, "tryon_pair_masks_u8: bad shape");
    dim3 grid((unsigned)((H * H + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_pair_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, palm, donor_image, donor_parsing,
                       retain_img, lower_img, lower_mask, upper_img, upper_mask, H, W, (H - W) / 2);
    return launch_status("tryon_pair_masks_u8");
}

extern "C" int pasta_patch_composite_eroded_u8(const uint8_t* patches, const uint8_t* masks, const double* minv, const uint8_t* valid,
                                               uint8_t* out, uint8_t* part_mask, int N, int P, int ph, int pw, int H, int W, int radius,
                                               void* stream) {
    using namespace pasta;
    PASTA_CHECK(patches && masks && minv && valid && out, "patch_composite_eroded_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && P >= 1 && ph >= 1 && pw >= 1 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
                "patch_composite_eroded_u8: bad shape");
    PASTA_CHECK(radius >= 0 && radius <= ER_MAX_R, "patch_composite_eroded_u8: radius %d (0..%d)", radius, ER_MAX_R);
    const int tiles_x = (W + ER_T - 1) / ER_T, tiles_y = (H + ER_T - 1) / ER_T;
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
    hipLaunchKernelGGL(patch_composite_eroded_kernel, grid, dim3(256), 0, (hipStream_t)stream, patches, masks, minv, valid, out, part_mask, P,
                       ph, pw, H, W, radius, tiles_x);
    return launch_status("patch_composite_eroded_u8");
}

extern "C" int pasta_tryon_pair_assemble(const uint8_t* retain_img, const uint8_t* stick, const uint8_t* patches, const uint8_t* stick_patches,
                                         const uint8_t* denorm_upper, const uint8_t* denorm_lower, float* const* outputs, int N, int H, int P,
                                         int ph, int pw, void* stream) {
    using namespace pasta;
    PASTA_CHECK(retain_img && stick && patches && stick_patches && denorm_upper && denorm_lower && outputs, "tryon_pair_assemble: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && P >= 1 && P <= 64 && ph >= 1 && pw >= 1 && ph * pw <= H * H,
                "tryon_pair_assemble: bad shape");
    PairOut o;
    float** f[7] = {&o.retain, &o.pose, &o.style_input, &o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask, &o.denorm_lower_mask};
    for (int i = 0; i < 7; i++) {
        PASTA_CHECK(outputs[i], "tryon_pair_assemble: output %d is null", i);
        *f[i] = outputs[i];
    }
    dim3 grid((unsigned)((H * H + ph * pw + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_pair_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, retain_img, stick, patches, stick_patches,
                       denorm_upper, denorm_lower, o, H, P, ph, pw);
    return launch_status("tryon_pair_assemble");
}

extern "C" int pasta_images_to_u8(const float* images, uint8_t* out, int N, int H, int Wt, int c0, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && out, "images_to_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && Wt >= 1 && Wt <= 4096 && W >= 1 && c0 >= 0 && c0 + W <= Wt,
                "images_to_u8: bad shape or crop (columns %d + %d of %d)", c0, W, Wt);
    dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(images_to_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, images, out, H, Wt, c0, W);
    return launch_status("images_to_u8");
}
