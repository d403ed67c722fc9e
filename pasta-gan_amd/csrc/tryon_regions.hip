// Per-batch preparation of the 512 x 320 try-on pairs with a change region on the GPU (row f4,
// UvitonDatasetFull_512_test._load_raw_image / normalize_full / normalize_upper / normalize_lower / __getitem__,
// training/dataset.py:1528-2214, and test_512.py:115-131), which the reference runs per sample on the host:
//   pasta_tryon_region_masks_u8   retain image and the upper and lower garment, each taken from the donor or the person as the
//                                 region says (:1631-1690);
//   pasta_tryon_region_assemble   __getitem__ (:2196-2214) and test_512.py's conversions (:115-131) into the nine fp32 tensors.
// The stick figure (thickness 5, radius 5) is csrc/tryon_inputs.hip's pasta_pose_stickman_thick_u8, the palm mask on the 512
// square (boxes 35 and 20) csrc/tryon_pairs.hip's pasta_palm_mask_square_u8, the warps csrc/patches.hip's
// pasta_warp_perspective_u8 and both composites pasta_patch_composite_eroded_u8 (every part eroded 5 x 5, the legs included).
// Every entry does a whole batch in one launch.
#include "common.h"
#include "tryon_common.h"

namespace pasta {

// ---- label masks with a change region ----

__global__ __launch_bounds__(256) void tryon_region_masks_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                                 const uint8_t* __restrict__ palm, const uint8_t* __restrict__ d_image,
                                                                 const uint8_t* __restrict__ d_parsing, uint8_t* __restrict__ retain_img,
                                                                 uint8_t* __restrict__ upper_img, uint8_t* __restrict__ upper_mask,
                                                                 uint8_t* __restrict__ lower_img, uint8_t* __restrict__ lower_mask, int H, int W,
                                                                 int lp, int upper_from_donor, int lower_from_donor) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * H) return;
    const int y = pix / H, c = pix - y * H - lp;
    const bool inside = c >= 0 && c < W;
    const int64_t src = (int64_t)n * H * W + (int64_t)y * W + c;
    const int L = inside ? parsing[src] : 0, D = inside ? d_parsing[src] : 0;
    const int64_t o = (int64_t)n * H * H + pix;
    const int keep = (L == 18 || L == 19) + palm[o] + (L == 1 || L == 2 || L == 4 || L == 13);      // shoes + palm + head, the person's
    const int U = upper_from_donor ? D : L, Lo = lower_from_donor ? D : L;
    const int up = U == 5 || U == 6 || U == 7;
    const int low = Lo == 9 || Lo == 12;                                                            // not 6, unlike the 256 test pairs
    for (int ch = 0; ch < 3; ch++) {
        const int v = inside ? image[src * 3 + ch] : 255, dv = inside ? d_image[src * 3 + ch] : 255;
        retain_img[o * 3 + ch] = (uint8_t)(keep * v);
        upper_img[o * 3 + ch] = (uint8_t)(up * (upper_from_donor ? dv : v));
        upper_mask[o * 3 + ch] = (uint8_t)(up * 255);
        lower_img[o * 3 + ch] = (uint8_t)(low * (lower_from_donor ? dv : v));
        lower_mask[o * 3 + ch] = (uint8_t)(low * 255);
    }
}

// ---- the nine tensors of test_512.py ----

struct RegionOut {
    float *image, *clothes, *retain, *pose, *style_input, *denorm_upper_input, *denorm_lower_input, *denorm_upper_mask, *denorm_lower_mask;
};

// retain: test_512.py forms image * mask - (1 - mask) from the 0 / 1 retain mask (shoes, palm and head are disjoint label groups,
// the palm a subset of labels 14 / 15, so the mask never exceeds 1).  Where the mask is 1 that is to_unit(v) * 1 - 0 = to_unit(v);
// where it is 0 it is (+-0) - 1 = -1 = to_unit(0).  Both are to_unit(mask * v) = to_unit(retain_img) bit for bit.
__global__ __launch_bounds__(256) void tryon_region_assemble_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ d_image,
                                                                    const uint8_t* __restrict__ retain_img, const uint8_t* __restrict__ stick,
                                                                    const uint8_t* __restrict__ patches, const uint8_t* __restrict__ patches_lower,
                                                                    const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                                    RegionOut o, int H, int W, int lp, int PU, int PL, int ph, int pw) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HH) {                // style_input = cat(norm_img, norm_img_lower): channel 3k + c of part k of its list
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int CS = 3 * (PU + PL);
        for (int ch = 0; ch < CS; ch++) {
            const int k = ch / 3, c = ch - 3 * k;
            const uint8_t* src = k < PU ? patches + (((int64_t)n * PU + k) * ph * pw + q) * 3 : patches_lower + (((int64_t)n * PL + k - PU) * ph * pw + q) * 3;
            o.style_input[((int64_t)n * CS + ch) * ph * pw + q] = to_unit(src[c]);
        }
        return;
    }
    const int y = pix / H, c = pix - y * H - lp;
    const bool inside = c >= 0 && c < W;
    const int64_t src = ((int64_t)n * H * W + (int64_t)y * W + c) * 3;
    const int64_t p = (int64_t)n * HH + pix;
    int su = 0, sl = 0;
    for (int ch = 0; ch < 3; ch++) {
        const int64_t oc = ((int64_t)n * 3 + ch) * HH + pix;
        o.image[oc] = to_unit(inside ? image[src + ch] : 255);
        o.clothes[oc] = to_unit(inside ? d_image[src + ch] : 255);
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

}  // namespace pasta

extern "C" int pasta_tryon_region_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, const uint8_t* donor_image,
                                           const uint8_t* donor_parsing, uint8_t* retain_img, uint8_t* upper_img, uint8_t* upper_mask,
                                           uint8_t* lower_img, uint8_t* lower_mask, int N, int H, int W, int region, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && palm && donor_image && donor_parsing && retain_img && upper_img && upper_mask && lower_img && lower_mask,
                "tryon_region_masks_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H, "tryon_region_masks_u8: bad shape");
    PASTA_CHECK(region >= 0 && region <= 2, "tryon_region_masks_u8: region %d (0 full body, 1 upper body, 2 lower body)", region);
    dim3 grid((unsigned)((H * H + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_region_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, palm, donor_image, donor_parsing,
                       retain_img, upper_img, upper_mask, lower_img, lower_mask, H, W, (H - W) / 2, region != 2, region != 1);
    return launch_status("tryon_region_masks_u8");
}

extern "C" int pasta_tryon_region_assemble(const uint8_t* image, const uint8_t* donor_image, const uint8_t* retain_img, const uint8_t* stick,
                                           const uint8_t* patches, const uint8_t* patches_lower, const uint8_t* denorm_upper,
                                           const uint8_t* denorm_lower, float* const* outputs, int N, int H, int W, int P, int P_lower, int ph,
                                           int pw, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && donor_image && retain_img && stick && patches && patches_lower && denorm_upper && denorm_lower && outputs,
                "tryon_region_assemble: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H && P >= 1 && P <= 64 && P_lower >= 1 && P_lower <= 64 &&
                ph >= 1 && pw >= 1 && ph * pw <= H * H, "tryon_region_assemble: bad shape");
    RegionOut o;
    float** f[9] = {&o.image, &o.clothes, &o.retain, &o.pose, &o.style_input, &o.denorm_upper_input, &o.denorm_lower_input,
                    &o.denorm_upper_mask, &o.denorm_lower_mask};
    for (int i = 0; i < 9; i++) {
        PASTA_CHECK(outputs[i], "tryon_region_assemble: output %d is null", i);
        *f[i] = outputs[i];
    }
    dim3 grid((unsigned)((H * H + ph * pw + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_region_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, donor_image, retain_img, stick, patches,
                       patches_lower, denorm_upper, denorm_lower, o, H, W, (H - W) / 2, P, P_lower, ph, pw);
    return launch_status("tryon_region_assemble");
}
