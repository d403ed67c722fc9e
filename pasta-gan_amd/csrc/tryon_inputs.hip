// Per-sample preparation of the try-on data sets on the GPU (row f4, the part of UvitonDatasetFull._load_raw_image /
// __getitem__ and of the training loop's float conversions that is not the body-part warps of csrc/patches.hip):
//   pasta_pose_stickman_u8  the pose stick figure (draw_pose_from_cords, dataset.py:704-736), padded, with the line thickness and
//                           the disc radius as arguments: every data set's (2 and 2 at 256 x 192, 5 and 5 at 512 x 320);
//   pasta_tryon_masks_u8    retain mask, gt_parsing, garment images and garment masks (:537-556) of both training sets;
//   pasta_tryon_assemble    erase mask (__getitem__ :951-973) and the loop's conversions (training_loop...:425-456); its
//                           per-pixel body is csrc/tryon_common.h's train_pixel (the erase rule with the restated resize, then
//                           tryon_pixel), shared with the 512 x 320 training kernel of csrc/tryon_pairs.hip.
// The palm mask (get_palm / get_hand_mask / get_rectangle_mask, :626-702) is csrc/tryon_pairs.hip's pasta_palm_mask_u8.
// Every entry is its checks and one launch for a whole batch.  The reference does this on the host with OpenCV, pycocotools and
// skimage.  What is defined by numpy / skimage is exact here; three primitives are restated (include/pasta_hip.h states the rules,
// DESIGN.md section 9): cv2.line(thickness), pycocotools' rleFrPoly and cv2.resize(INTER_LINEAR) on uint8.
#include "common.h"
#include "tryon_common.h"

namespace pasta {

__constant__ uint8_t kpt_colors[19][3] = {          // dataset.py kptcolors
    {255, 0, 0}, {255, 85, 0}, {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0}, {0, 255, 85},
    {0, 255, 170}, {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {0, 0, 255}, {85, 0, 255}, {170, 0, 255}, {255, 0, 255},
    {255, 0, 170}, {255, 0, 85}, {255, 0, 0}};

constexpr int TRYON_LIMBS = 19, TRYON_JOINTS = 18;

// The pixel (px, py) lies within distance t / 2 (the half-thickness) of the segment a -> b: the capsule of a thickness-t line,
// in integers with t2 = t * t: 4 d^2 <= t^2 at the caps and 4 cross^2 <= t^2 len2 along the segment.  t = 2 is the thickness-2
// rule d^2 <= 1, cross^2 <= len2.  Coordinates are within +-4096 (+ the canvas), so 4 cross^2 < 2^58.
__device__ __forceinline__ bool capsule_hit(int px, int py, int x0, int y0, int x1, int y1, int64_t t2) {
    const int64_t dx = x1 - x0, dy = y1 - y0, ux = px - x0, uy = py - y0;
    const int64_t len2 = dx * dx + dy * dy, t = ux * dx + uy * dy;
    if (len2 == 0 || t <= 0) return 4 * (ux * ux + uy * uy) <= t2;
    if (t >= len2) { const int64_t vx = px - x1, vy = py - y1; return 4 * (vx * vx + vy * vy) <= t2; }
    const int64_t cr = ux * dy - uy * dx;
    return 4 * cr * cr <= t2 * len2;
}

// out[n, y, x, :] for the padded H x H square: limbs of thickness t (t2 = t * t) in order, then the joint discs of radius r
// (r2 = r * r), the last hit wins.
__global__ __launch_bounds__(256) void pose_stickman_kernel(const int32_t* __restrict__ limbs, const int32_t* __restrict__ joints,
                                                            uint8_t* __restrict__ out, int H, int W, int lp, int t2, int r2) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * H) return;
    const SquarePixel s = square_pixel(n, pix, H, W, lp);
    const int y = s.y, c = s.c;                          // c: column of the unpadded canvas
    int color = -1;
    if (s.inside) {
        const int32_t* lb = limbs + (int64_t)n * TRYON_LIMBS * 5;
        for (int i = 0; i < TRYON_LIMBS; i++, lb += 5)
            if (lb[4] && capsule_hit(c, y, lb[0], lb[1], lb[2], lb[3], t2)) color = i;
        const int32_t* jt = joints + (int64_t)n * TRYON_JOINTS * 3;
        for (int j = 0; j < TRYON_JOINTS; j++, jt += 3) {
            const int64_t ddx = c - jt[0], ddy = y - jt[1];
            if (jt[2] && ddx * ddx + ddy * ddy < r2) color = j;          // (r - y)^2 + (c - x)^2 < radius^2 (radius 2: the 3 x 3 square)
        }
    }
    uint8_t* o = out + ((int64_t)n * H * H + pix) * 3;
    o[0] = color < 0 ? 0 : kpt_colors[color][0];
    o[1] = color < 0 ? 0 : kpt_colors[color][1];
    o[2] = color < 0 ? 0 : kpt_colors[color][2];
}

// ---- label masks ----

__global__ __launch_bounds__(256) void tryon_masks_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                          const uint8_t* __restrict__ palm, uint8_t* __restrict__ retain,
                                                          uint8_t* __restrict__ gt, uint8_t* __restrict__ upper_img,
                                                          uint8_t* __restrict__ lower_img, uint8_t* __restrict__ upper_mask,
                                                          uint8_t* __restrict__ lower_mask, int H, int W, int lp) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * H) return;
    const SquarePixel s = square_pixel(n, pix, H, W, lp);
    const int L = s.inside ? parsing[s.src] : 0;
    const int64_t o = (int64_t)n * H * H + pix;
    const int shoes = L == 18 || L == 19, head = L == 1 || L == 2 || L == 4 || L == 13;
    const int up = L == 5 || L == 6 || L == 7, low = L == 9 || L == 12;
    const int hands = L == 14 || L == 15, legs = L == 16 || L == 17, neck = L == 10;
    retain[o] = (uint8_t)(shoes + palm[o] + head);
    gt[o] = (uint8_t)(up + low * 2 + hands * 3 + legs * 4 + neck * 5);
    for (int ch = 0; ch < 3; ch++) {
        const int v = s.inside ? image[s.src * 3 + ch] : 255;
        upper_img[o * 3 + ch] = (uint8_t)(up * v);
        lower_img[o * 3 + ch] = (uint8_t)(low * v);
        upper_mask[o * 3 + ch] = (uint8_t)(up * 255);
        lower_mask[o * 3 + ch] = (uint8_t)(low * 255);
    }
}

// ---- erase mask and float conversions ----

__global__ __launch_bounds__(256) void tryon_assemble_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ stick,
                                                             const uint8_t* __restrict__ retain_mask, const uint8_t* __restrict__ gt,
                                                             const uint8_t* __restrict__ norm_img, const uint8_t* __restrict__ norm_lower,
                                                             const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                             const uint8_t* __restrict__ arm_masks, const uint8_t* __restrict__ erase_src,
                                                             const int32_t* __restrict__ erase_hw, TryonOut o, int H, int W, int lp,
                                                             int ph, int pw, int CU, int CL, int mh_max, int mw_max) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HH) {                           // style_input = cat(norm_img, norm_img_lower) / 127.5 - 1 at (ph, pw)
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int CS = CU + CL;
        for (int ch = 0; ch < CS; ch++) {
            const int v = ch < CU ? norm_img[((int64_t)n * ph * pw + q) * CU + ch] : norm_lower[((int64_t)n * ph * pw + q) * CL + ch - CU];
            o.style_input[((int64_t)n * CS + ch) * ph * pw + q] = to_unit(v);
        }
        return;
    }
    // the erase rule on arm_masks[2] and arm_masks[3], the photograph, gt_parsing and csrc/tryon_common.h's tryon_pixel
    train_pixel(o, n, pix, H, W, lp, image, stick, retain_mask, gt, den_u, den_l, arm_masks + ((int64_t)n * 4 + 2) * HH,
                arm_masks + ((int64_t)n * 4 + 3) * HH, erase_src, erase_hw, mh_max, mw_max);
}

}  // namespace pasta

extern "C" int pasta_pose_stickman_u8(const int32_t* limbs, const int32_t* joints, uint8_t* out, int N, int H, int W, int thickness, int radius,
                                      void* stream) {
    using namespace pasta;
    PASTA_CHECK(limbs && joints && out, "pose_stickman_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H, "pose_stickman_u8: bad shape");
    PASTA_CHECK(thickness >= 1 && thickness <= 64 && radius >= 1 && radius <= 64, "pose_stickman_u8: thickness %d, radius %d (1..64)",
                thickness, radius);
    dim3 grid((unsigned)((H * H + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(pose_stickman_kernel, grid, dim3(256), 0, (hipStream_t)stream, limbs, joints, out, H, W, (H - W) / 2,
                       thickness * thickness, radius * radius);
    return launch_status("pose_stickman_u8");
}

extern "C" int pasta_tryon_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, uint8_t* retain, uint8_t* gt_parsing,
                                    uint8_t* upper_img, uint8_t* lower_img, uint8_t* upper_mask, uint8_t* lower_mask, int N, int H, int W,
                                    void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && palm && retain && gt_parsing && upper_img && lower_img && upper_mask && lower_mask,
                "tryon_masks_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H, "tryon_masks_u8: bad shape");
    dim3 grid((unsigned)((H * H + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, palm, retain, gt_parsing, upper_img,
                       lower_img, upper_mask, lower_mask, H, W, (H - W) / 2);
    return launch_status("tryon_masks_u8");
}

extern "C" int pasta_tryon_assemble(const uint8_t* image, const uint8_t* stick, const uint8_t* retain_mask, const uint8_t* gt_parsing,
                                    const uint8_t* norm_img, const uint8_t* norm_img_lower, const uint8_t* denorm_upper,
                                    const uint8_t* denorm_lower, const uint8_t* arm_masks, const uint8_t* erase_masks,
                                    const int32_t* erase_hw, float* const* outputs, int N, int H, int W, int ph, int pw, int c_upper,
                                    int c_lower, int mh_max, int mw_max, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && stick && retain_mask && gt_parsing && norm_img && norm_img_lower && denorm_upper && denorm_lower && arm_masks &&
                erase_masks && erase_hw && outputs, "tryon_assemble: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H && ph >= 1 && pw >= 1 && c_upper >= 1 && c_lower >= 1 &&
                mh_max >= 1 && mw_max >= 1, "tryon_assemble: bad shape");
    TryonOut o{};
    float** f[9] = {&o.image, &o.style_input, &o.retain, &o.pose, &o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask,
                    &o.denorm_lower_mask, &o.gt_parsing};          // FullBodyBatch.KEYS; real_img is o.image
    const int missing = take_outputs(outputs, f, 9);
    PASTA_CHECK(missing < 0, "tryon_assemble: output %d is null", missing);
    dim3 grid((unsigned)((H * H + ph * pw + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, stick, retain_mask, gt_parsing, norm_img,
                       norm_img_lower, denorm_upper, denorm_lower, arm_masks, erase_masks, erase_hw, o, H, W, (H - W) / 2, ph, pw, c_upper,
                       c_lower, mh_max, mw_max);
    return launch_status("tryon_assemble");
}
