// Per-batch preparation of both sets of try-on TEST pairs on the GPU (row f4), which the reference runs per sample on the host
// in four loader processes with OpenCV, pycocotools and skimage: the 256 x 192 pairs (UvitonDatasetV19_test._load_raw_image /
// normalize / __getitem__, training/dataset.py:1085-1525, and test.py:104-150) and the 512 x 320 pairs with a change region
// (UvitonDatasetFull_512_test._load_raw_image / normalize_full / normalize_upper / normalize_lower / __getitem__, :1528-2214,
// and test_512.py:115-131).  The same entries prepare the OUTFITS of both sizes (this
// project's own: a person, an upper garment and a lower garment from up to three people; a pair with a region is the outfit
// whose two sources are the donor or the person) and the 512 x 320 TRAINING samples (this project's own as well).  One entry
// per kernel, each its checks and one launch for a whole batch:
//   pasta_palm_mask_u8                 the palm mask on an S x S square with both box sizes as arguments (:1240-1253,
//                                      :1779-1799): every data set's, the two training sets included;
//   pasta_tryon_outfit_masks_u8        retain image, upper and lower garment with a source of its own for each garment
//                                      (:1105-1141, :1631-1690); six_is_lower: label 6 belongs to the lower garment (256 x 192);
//   pasta_patch_composite_eroded_u8    the warp-back composite with cv2.erode of the mask before the == 255 test (:1480-1492),
//                                      by one radius or by a radius per sample (0, the plain composite, for a person's own
//                                      lower garment and 2 for another's in the 256 outfits);
//   pasta_tryon_outfit_assemble        __getitem__ and the scripts' conversions (:1502-1525 and test.py:104-117; :2196-2214 and
//                                      test_512.py:115-131) into the seven fp32 tensors G takes, with image and clothes nine,
//                                      with clothes_lower (the lower garment's donor) ten;
//   pasta_tryon_train_region_assemble  the erase mask from two eroded arm-part masks and the nine fp32 tensors of the loop at
//                                      512 x 320 (the label masks of that set are csrc/tryon_inputs.hip's pasta_tryon_masks_u8);
//   pasta_images_to_u8                 test.py's (x + 1) * 127.5, crop, clip and uint8 truncation (:133-137);
//   pasta_images_keep_to_u8            the same with the photograph's kept parts pasted in under a feathered weight (this
//                                      project's own, --kept-parts photo), in the one launch;
//   pasta_photo_paste_mask_u8          the region that entry pastes, widened to the background and the person's own garments
//                                      (this project's own, --background / --kept-garments photo): the photograph's label map,
//                                      the palm mask and the generator's own region heads, agreed per pixel, in one pass.
// The 256 pairs are the 512 rules with label 6 added to the lower garment, stick patches as the second patch list and no image /
// clothes tensors.  The forward warps are csrc/patches.hip's pasta_warp_perspective_u8 and the stick figures
// csrc/tryon_inputs.hip's entry.  include/pasta_hip.h lists where the data sets differ and the constants each one passes.
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

// The upper and the lower garment each have a source of their own, (u_image, u_parsing) and (l_image, l_parsing): the person's
// pointers again, a donor's, or two different donors'; label 6 belongs to the lower garment at 256 x 192 only.
__global__ __launch_bounds__(256) void tryon_pair_masks_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                               const uint8_t* __restrict__ palm, const uint8_t* __restrict__ u_image,
                                                               const uint8_t* __restrict__ u_parsing, const uint8_t* __restrict__ l_image,
                                                               const uint8_t* __restrict__ l_parsing, uint8_t* __restrict__ retain_img,
                                                               uint8_t* __restrict__ upper_img, uint8_t* __restrict__ upper_mask,
                                                               uint8_t* __restrict__ lower_img, uint8_t* __restrict__ lower_mask, int H, int W,
                                                               int lp, int six_is_lower) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * H) return;
    const SquarePixel s = square_pixel(n, pix, H, W, lp);
    const int L = s.inside ? parsing[s.src] : 0, U = s.inside ? u_parsing[s.src] : 0, Lo = s.inside ? l_parsing[s.src] : 0;
    const int64_t o = (int64_t)n * H * H + pix;
    const int keep = (L == 18 || L == 19) + palm[o] + (L == 1 || L == 2 || L == 4 || L == 13);      // shoes + palm + head, the person's
    const int up = U == 5 || U == 6 || U == 7;
    const int low = Lo == 9 || Lo == 12 || (six_is_lower && Lo == 6);
    for (int ch = 0; ch < 3; ch++) {
        const int v = s.inside ? image[s.src * 3 + ch] : 255;
        const int uv = s.inside ? u_image[s.src * 3 + ch] : 255, lv = s.inside ? l_image[s.src * 3 + ch] : 255;
        retain_img[o * 3 + ch] = (uint8_t)(keep * v);
        upper_img[o * 3 + ch] = (uint8_t)(up * uv);
        upper_mask[o * 3 + ch] = (uint8_t)(up * 255);
        lower_img[o * 3 + ch] = (uint8_t)(low * lv);
        lower_mask[o * 3 + ch] = (uint8_t)(low * 255);
    }
}

// ---- eroded composite ----

// The tile work is csrc/patch_erode.h's (shared with the snapshot grid's indexed composite); here part k of sample n is item n * P + k.
// Sample n is eroded by radius[n], or by r where radius is null.  A block works on one sample, so
// its radius is uniform across the block; a value above ER_MAX_R (the entry's callers check theirs on the host) is taken as
// ER_MAX_R, what the LDS tiles hold.
__global__ __launch_bounds__(256) void patch_composite_eroded_kernel(const uint8_t* __restrict__ patches, const uint8_t* __restrict__ masks,
                                                                     const double* __restrict__ minv, const uint8_t* __restrict__ valid,
                                                                     uint8_t* __restrict__ out, uint8_t* __restrict__ part_mask, int P, int ph,
                                                                     int pw, int H, int W, const uint8_t* __restrict__ radius, int r,
                                                                     int tiles_x) {
    __shared__ uint8_t flags[ER_S * ER_S];
    __shared__ uint8_t rows[ER_S * ER_T];
    const int n = blockIdx.y;
    if (radius) r = radius[n] < ER_MAX_R ? radius[n] : ER_MAX_R;
    const auto part_of = [=](int k) {
        const int64_t item = (int64_t)n * P + k;
        return ErPart{patches + item * ph * pw * 3, valid[item] ? masks + item * ph * pw * 3 : nullptr, minv + item * 9};
    };
    composite_eroded_tile(part_of, out + (int64_t)n * H * W * 3, part_mask ? part_mask + (int64_t)n * P * H * W : nullptr, P, ph, pw, H, W, r,
                          blockIdx.x, tiles_x, flags, rows);
}

// ---- the seven tensors G takes, or the nine of test_512.py ----

// Two lists of patches, PA and PB parts, make style_input: (patches, stick patches) at 256 x 192, (patches, patches_lower) at
// 512 x 320.  o.image and o.clothes are written from image and d_image (W wide, lp columns of padding) unless they are null, and
// o.clothes_lower from d_image_l, the lower garment's donor of an outfit, unless that is null.
// retain: test_512.py forms image * mask - (1 - mask) from the 0 / 1 retain mask (shoes, palm and head are disjoint label groups,
// the palm a subset of labels 14 / 15, so the mask never exceeds 1).  Where the mask is 1 that is to_unit(v) * 1 - 0 = to_unit(v);
// where it is 0 it is (+-0) - 1 = -1 = to_unit(0).  Both are to_unit(mask * v) = to_unit(retain_img) bit for bit, test.py's form.
__global__ __launch_bounds__(256) void tryon_pair_assemble_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ d_image,
                                                                  const uint8_t* __restrict__ d_image_l,
                                                                  const uint8_t* __restrict__ retain_img, const uint8_t* __restrict__ stick,
                                                                  const uint8_t* __restrict__ patches_a, const uint8_t* __restrict__ patches_b,
                                                                  const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                                  TryonOut o, int H, int W, int lp, int PA, int PB, int ph, int pw) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HH) {                // style_input = cat of the two lists: channel 3k + c of part k of its list
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int CS = 3 * (PA + PB);
        for (int ch = 0; ch < CS; ch++) {
            const int k = ch / 3, c = ch - 3 * k;
            const uint8_t* src = k < PA ? patches_a + (((int64_t)n * PA + k) * ph * pw + q) * 3 : patches_b + (((int64_t)n * PB + k - PA) * ph * pw + q) * 3;
            o.style_input[((int64_t)n * CS + ch) * ph * pw + q] = to_unit(src[c]);
        }
        return;
    }
    const int64_t p = (int64_t)n * HH + pix;
    float ret[3], person[3] = {}, donor[3] = {}, donor_l[3] = {};
    for (int ch = 0; ch < 3; ch++) ret[ch] = to_unit(retain_img[p * 3 + ch]);
    if (o.image) {                  // read before anything is stored
        const SquarePixel s = square_pixel(n, pix, H, W, lp);
        for (int ch = 0; ch < 3; ch++) {
            person[ch] = to_unit(s.inside ? image[s.src * 3 + ch] : 255);
            donor[ch] = to_unit(s.inside ? d_image[s.src * 3 + ch] : 255);
            if (o.clothes_lower) donor_l[ch] = to_unit(s.inside ? d_image_l[s.src * 3 + ch] : 255);
        }
    }
    tryon_pixel(o, n, pix, HH, ret, stick + p * 3, den_u + p * 3, den_l + p * 3, 1);
    if (o.image)
        for (int ch = 0; ch < 3; ch++) {
            o.image[((int64_t)n * 3 + ch) * HH + pix] = person[ch];
            o.clothes[((int64_t)n * 3 + ch) * HH + pix] = donor[ch];
            if (o.clothes_lower) o.clothes_lower[((int64_t)n * 3 + ch) * HH + pix] = donor_l[ch];
        }
}

// ---- the nine tensors of the training loop at 512 x 320 ----

// style_input as tryon_pair_assemble_kernel forms it from the two per-part lists, four patch pixels per thread (12-byte loads,
// 16-byte stores); every pixel of the square is csrc/tryon_common.h's train_pixel, the 256 training kernel's own body, with the
// eroded masks of parts arm_a and arm_b of the upper composite (part_masks [N, PA, H, H]) as the two arm masks.
__global__ __launch_bounds__(256) void tryon_train_region_assemble_kernel(
    const uint8_t* __restrict__ image, const uint8_t* __restrict__ stick, const uint8_t* __restrict__ retain_mask,
    const uint8_t* __restrict__ gt, const uint8_t* __restrict__ patches_a, const uint8_t* __restrict__ patches_b,
    const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l, const uint8_t* __restrict__ part_masks, int arm_a, int arm_b,
    const uint8_t* __restrict__ erase_src, const int32_t* __restrict__ erase_hw, TryonOut o, int H, int W, int lp, int PA, int PB, int ph,
    int pw, int mh_max, int mw_max) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HH) {
        const int q = (pix - HH) * 4;          // ph * pw is a multiple of 4: the four pixels lie in the patch
        if (q >= ph * pw) return;
        const int CS = 3 * (PA + PB);
        for (int k = 0; k < PA + PB; k++) {
            const uint8_t* src = k < PA ? patches_a + (((int64_t)n * PA + k) * ph * pw + q) * 3 : patches_b + (((int64_t)n * PB + k - PA) * ph * pw + q) * 3;
            const Px4 px = load_px4(src);
            for (int c = 0; c < 3; c++)
                store4(o.style_input + ((int64_t)n * CS + 3 * k + c) * ph * pw + q, to_unit(px.v[c]), to_unit(px.v[3 + c]), to_unit(px.v[6 + c]),
                       to_unit(px.v[9 + c]));
        }
        return;
    }
    train_pixel(o, n, pix, H, W, lp, image, stick, retain_mask, gt, den_u, den_l, part_masks + ((int64_t)n * PA + arm_a) * HH,
                part_masks + ((int64_t)n * PA + arm_b) * HH, erase_src, erase_hw, mh_max, mw_max);
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

// ---- generated images to uint8 with the photograph's kept parts pasted in ----

// include/pasta_hip.h's rule of pasta_images_keep_to_u8 (this project's own).  A block of 256 threads makes a tile of 16 rows by
// 16 * PX columns, PX adjacent pixels of a row per thread: PX = 4 where the entry found every row of every tensor aligned for it
// (16-byte loads of the three fp32 planes, one 12-byte load of the photograph and one 12-byte store), PX = 1 for any other
// width.  The kept flags of the tile and an r-pixel halo (1 outside the image) go to LDS as bytes, are summed along rows (at
// most 17, a byte) and then along columns into a register (at most 289).  r is the launch's scalar; with r == 0 the pixel's own
// flag decides and the kernel touches neither LDS nor a barrier (csrc/patch_erode.h's convention).
constexpr int KC_TY = 16;           // tile rows
constexpr int KC_MAX_R = 8;         // largest feather radius (a 17 x 17 window)

template <int PX>
__global__ __launch_bounds__(256) void images_keep_to_u8_kernel(const float* __restrict__ src, const uint8_t* __restrict__ photo,
                                                                const uint8_t* __restrict__ keep, uint8_t* __restrict__ dst, int H, int Wt,
                                                                int c0, int W, int r, int tiles_x) {
    constexpr int TX = 16 * PX;
    __shared__ uint8_t flags[(KC_TY + 2 * KC_MAX_R) * (TX + 2 * KC_MAX_R)];
    __shared__ __attribute__((aligned(4))) uint8_t rows[(KC_TY + 2 * KC_MAX_R) * TX];
    const int n = blockIdx.y;
    const int tx0 = (blockIdx.x % tiles_x) * TX, ty0 = (blockIdx.x / tiles_x) * KC_TY;
    const int ty = threadIdx.x / 16, tg = (threadIdx.x % 16) * PX;
    const int y = ty0 + ty, x = tx0 + tg;
    const bool mine = y < H && x < W;           // PX == 4: W is a multiple of 4, so a thread's four pixels are inside together
    const uint8_t* kp = keep + (int64_t)n * H * W;
    const int64_t pix = ((int64_t)n * H + y) * W + x;

    float g[3][PX];                             // every global load of the pixels before the LDS phases
    uint8_t p[3 * PX];
    if (mine) {
        for (int ch = 0; ch < 3; ch++) {
            const float* s = src + (((int64_t)n * 3 + ch) * H + y) * Wt + c0 + x;
            if constexpr (PX == 4) {
                const float4 v = *reinterpret_cast<const float4*>(s);
                g[ch][0] = v.x; g[ch][1] = v.y; g[ch][2] = v.z; g[ch][3] = v.w;
            } else {
                g[ch][0] = s[0];
            }
        }
        if constexpr (PX == 4) {
            const Px4 px = load_px4(photo + pix * 3);
            for (int i = 0; i < 12; i++) p[i] = px.v[i];
        } else {
            for (int i = 0; i < 3; i++) p[i] = photo[pix * 3 + i];
        }
    }

    int a[PX];                                  // the photograph's weight out of K
    if (r > 0) {                                // uniform across the launch
        const int SX = TX + 2 * r, SY = KC_TY + 2 * r;
        for (int i = threadIdx.x; i < SY * SX; i += 256) {
            const int gy = ty0 - r + i / SX, gx = tx0 - r + i % SX;
            flags[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? kp[(int64_t)gy * W + gx] != 0 : 1;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < SY * 16; i += 256) {     // PX adjacent row sums per item, a sliding window
            const int ry = i / 16, cx = (i % 16) * PX;
            const uint8_t* f = flags + ry * SX + cx;
            int s = 0;
            for (int d = 0; d <= 2 * r; d++) s += f[d];
            for (int j = 0; j < PX; j++) {
                rows[ry * TX + cx + j] = (uint8_t)s;
                if (j + 1 < PX) s += f[j + 2 * r + 1] - f[j];
            }
        }
        __syncthreads();
        for (int j = 0; j < PX; j++) a[j] = 0;
        for (int d = 0; d <= 2 * r; d++) {
            const uint8_t* rp = rows + (ty + d) * TX + tg;
            if constexpr (PX == 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(rp);
                for (int j = 0; j < 4; j++) a[j] += (w >> (8 * j)) & 255;
            } else {
                a[0] += rp[0];
            }
        }
        for (int j = 0; j < PX; j++)
            if (!flags[(ty + r) * SX + tg + r + j]) a[j] = 0;
    } else if (mine) {
        if constexpr (PX == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(kp + (int64_t)y * W + x);
            for (int j = 0; j < 4; j++) a[j] = ((w >> (8 * j)) & 255) != 0;
        } else {
            a[0] = kp[(int64_t)y * W + x] != 0;
        }
    }
    if (!mine) return;                          // after the last barrier

    // (g (K - a) + p a + K / 2) / K by a multiplication: m = ceil(2^32 / K) gives the floor quotient of every numerator up to
    // 2^32 / K, and the largest here is 255 * 289 + 144.  K is odd and at least 9 in this branch; r == 0 divides nothing.
    const uint32_t K = (uint32_t)((2 * r + 1) * (2 * r + 1));
    const uint32_t m = 0xFFFFFFFFu / K + 1;
    uint8_t o[3 * PX];
    for (int j = 0; j < PX; j++)
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t gb = unit_to_u8(g[ch][j]), pb = p[3 * j + ch], w = (uint32_t)a[j];
            o[3 * j + ch] = r > 0 ? (uint8_t)__umulhi(gb * (K - w) + pb * w + K / 2, m) : (uint8_t)(w ? pb : gb);
        }
    if constexpr (PX == 4) {
        uint3 words;
        words.x = o[0] | o[1] << 8 | o[2] << 16 | (uint32_t)o[3] << 24;
        words.y = o[4] | o[5] << 8 | o[6] << 16 | (uint32_t)o[7] << 24;
        words.z = o[8] | o[9] << 8 | o[10] << 16 | (uint32_t)o[11] << 24;
        *reinterpret_cast<uint3*>(dst + pix * 3) = words;
    } else {
        for (int i = 0; i < 3; i++) dst[pix * 3 + i] = o[i];
    }
}

// ---- where the photograph may be pasted: the label map and the generator's statement agree ----

// include/pasta_hip.h's rule of pasta_photo_paste_mask_u8 (this project's own).  Every pixel is independent: its label indexes the
// item's 256-byte rule row (in LDS, one byte per thread of the block), whose bit s says whether the generator's statement s allows
// the paste; a palm pixel is pasted whatever the heads say.  PLANES is the kind of heads: 6 logit planes in heads_a (argmax as
// torch.argmax: the first NaN, else the first largest), 1 sigmoid plane in each of heads_a and heads_b, or 0, no statement.
// PX = 4 where the entry found every row aligned for it (a dword of labels, a dword of palm flags, 16-byte loads of the planes,
// one dword store), PX = 1 otherwise.  Every global load stands before the barrier.
template <int PX, int PLANES>
__global__ __launch_bounds__(256) void photo_paste_mask_kernel(const uint8_t* __restrict__ parsing, const uint8_t* __restrict__ palm,
                                                               const uint8_t* __restrict__ rule, const float* __restrict__ heads_a,
                                                               const float* __restrict__ heads_b, uint8_t* __restrict__ out, int H, int W,
                                                               int Ht, int c0) {
    constexpr int NV = PLANES == 6 ? 6 : PLANES == 1 ? 2 : 0;
    __shared__ uint8_t row[256];
    const int n = blockIdx.y;
    row[threadIdx.x] = rule[(int64_t)n * 256 + threadIdx.x];
    const int first = (blockIdx.x * 256 + threadIdx.x) * PX;    // PX == 4: W is a multiple of 4, so the four pixels share a row
    const bool mine = first < H * W;
    const int y = first / W, x = first - y * W;
    const int64_t pix = (int64_t)n * H * W + first;

    uint8_t label[PX], hand[PX];
    float v[NV > 0 ? NV : 1][PX];
    if (mine) {
        if constexpr (PX == 4) {
            const uint32_t lw = *reinterpret_cast<const uint32_t*>(parsing + pix);
            const uint32_t pw = palm ? *reinterpret_cast<const uint32_t*>(palm + ((int64_t)n * H + y) * Ht + c0 + x) : 0u;
            for (int j = 0; j < 4; j++) label[j] = (uint8_t)(lw >> (8 * j)), hand[j] = (uint8_t)(pw >> (8 * j));
        } else {
            label[0] = parsing[pix];
            hand[0] = palm ? palm[((int64_t)n * H + y) * Ht + c0 + x] : (uint8_t)0;
        }
        for (int k = 0; k < NV; k++) {
            const float* plane = PLANES == 6 ? heads_a + ((int64_t)n * 6 + k) * Ht * Ht : (k == 0 ? heads_a : heads_b) + (int64_t)n * Ht * Ht;
            const float* s = plane + (int64_t)y * Ht + c0 + x;
            if constexpr (PX == 4) {
                const float4 q = *reinterpret_cast<const float4*>(s);
                v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
            } else {
                v[k][0] = s[0];
            }
        }
    }
    __syncthreads();
    if (!mine) return;

    uint32_t word = 0;
    for (int j = 0; j < PX; j++) {
        int s = 0;                              // the generator's statement: 0 other, 1 upper, 2 lower, 3 skin
        if constexpr (PLANES == 6) {
            float best = v[0][j];
            int c = 0;
            for (int k = 1; k < 6; k++) {       // a later plane wins only when it is larger, or the first NaN
                const float t = v[k][j];
                if (!(best != best) && (t != t || t > best)) best = t, c = k;
            }
            s = c < 3 ? c : 3;                  // gt_parsing's classes: 3 hands, 4 legs, 5 neck are skin
        } else if constexpr (PLANES == 1) {
            s = v[0][j] > 0.5f ? 1 : v[1][j] > 0.5f ? 2 : 0;        // IEEE comparisons: a NaN claims nothing
        }
        const uint32_t m = (hand[j] != 0) | ((row[label[j]] >> s) & 1u);
        word |= m << (8 * j);
    }
    if constexpr (PX == 4)
        *reinterpret_cast<uint32_t*>(out + pix) = word;
    else
        out[pix] = (uint8_t)word;
}

}  // namespace pasta

extern "C" int pasta_palm_mask_u8(const uint8_t* parsing, const double* quads, const uint8_t* present, uint8_t* out, int N, int S, int W,
                                  int k_upper, int k_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(parsing && quads && present && out, "palm_mask_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && S >= PALM_BAND && S <= PALM_S_MAX && S % PALM_BAND == 0 && W >= 1 && W <= S,
                "palm_mask_u8: bad shape (the padded square: a multiple of %d up to %d)", PALM_BAND, PALM_S_MAX);
    PASTA_CHECK(k_upper >= 1 && k_upper <= S && k_lower >= 1 && k_lower <= S, "palm_mask_u8: box sizes %d, %d (1..%d)", k_upper, k_lower, S);
    dim3 grid((unsigned)(S / PALM_BAND), (unsigned)N);
    hipLaunchKernelGGL(palm_mask_box_kernel, grid, dim3(S), (size_t)PALM_SEGS * S * 4 * sizeof(int16_t), (hipStream_t)stream, parsing, quads,
                       present, out, S, W, (S - W) / 2, k_upper, k_lower);
    return launch_status("palm_mask_u8");
}

extern "C" int pasta_tryon_outfit_masks_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* palm, const uint8_t* upper_image,
                                           const uint8_t* upper_parsing, const uint8_t* lower_image, const uint8_t* lower_parsing,
                                           uint8_t* retain_img, uint8_t* upper_img, uint8_t* upper_mask, uint8_t* lower_img,
                                           uint8_t* lower_mask, int N, int H, int W, int six_is_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && palm && upper_image && upper_parsing && lower_image && lower_parsing && retain_img && upper_img &&
                upper_mask && lower_img && lower_mask, "tryon_outfit_masks_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H, "tryon_outfit_masks_u8: bad shape");
    PASTA_CHECK(six_is_lower == 0 || six_is_lower == 1, "tryon_outfit_masks_u8: six_is_lower %d (0 or 1)", six_is_lower);
    dim3 grid((unsigned)((H * H + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_pair_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, palm, upper_image, upper_parsing,
                       lower_image, lower_parsing, retain_img, upper_img, upper_mask, lower_img, lower_mask, H, W, (H - W) / 2, six_is_lower);
    return launch_status("tryon_outfit_masks_u8");
}

extern "C" int pasta_patch_composite_eroded_u8(const uint8_t* patches, const uint8_t* masks, const double* minv, const uint8_t* valid,
                                               uint8_t* out, uint8_t* part_mask, int N, int P, int ph, int pw, int H, int W, int radius,
                                               const uint8_t* radii, void* stream) {
    using namespace pasta;
    PASTA_CHECK(patches && masks && minv && valid && out, "patch_composite_eroded_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && P >= 1 && ph >= 1 && pw >= 1 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
                "patch_composite_eroded_u8: bad shape");
    PASTA_CHECK(radii || (radius >= 0 && radius <= ER_MAX_R), "patch_composite_eroded_u8: radius %d (0..%d)", radius, ER_MAX_R);
    const int tiles_x = (W + ER_T - 1) / ER_T, tiles_y = (H + ER_T - 1) / ER_T;
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
    hipLaunchKernelGGL(patch_composite_eroded_kernel, grid, dim3(256), 0, (hipStream_t)stream, patches, masks, minv, valid, out, part_mask, P,
                       ph, pw, H, W, radii, radius, tiles_x);
    return launch_status("patch_composite_eroded_u8");
}

extern "C" int pasta_tryon_outfit_assemble(const uint8_t* image, const uint8_t* upper_donor_image, const uint8_t* lower_donor_image,
                                           const uint8_t* retain_img, const uint8_t* stick, const uint8_t* patches,
                                           const uint8_t* patches_lower, const uint8_t* denorm_upper, const uint8_t* denorm_lower,
                                           float* const* outputs, int N, int H, int W, int P, int P_lower, int ph, int pw, void* stream) {
    using namespace pasta;
    PASTA_CHECK(retain_img && stick && patches && patches_lower && denorm_upper && denorm_lower && outputs, "tryon_outfit_assemble: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H && P >= 1 && P <= 64 && P_lower >= 1 && P_lower <= 64 &&
                ph >= 1 && pw >= 1 && ph * pw <= H * H, "tryon_outfit_assemble: bad shape");
    TryonOut o{};
    float** f[7] = {&o.retain, &o.pose, &o.style_input, &o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask, &o.denorm_lower_mask};
    const int missing = take_outputs(outputs + 2, f, 7);
    PASTA_CHECK(missing < 0, "tryon_outfit_assemble: output %d is null", missing + 2);
    // image, clothes and clothes_lower may be null: a null tensor is not written and its photograph is not read.  The kernel
    // writes the photographs' tensors under `if (o.image)`, so clothes comes with image and clothes_lower only with both.
    o.image = outputs[0], o.clothes = outputs[1], o.clothes_lower = outputs[9];
    PASTA_CHECK(!o.image == !o.clothes && (o.image || !o.clothes_lower),
                "tryon_outfit_assemble: outputs 0 and 1 (image, clothes) are null together or not at all, and output 9 needs them");
    PASTA_CHECK((!o.image || (image && upper_donor_image)) && (!o.clothes_lower || lower_donor_image),
                "tryon_outfit_assemble: null photograph of a requested output");
    dim3 grid((unsigned)((H * H + ph * pw + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_pair_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, upper_donor_image, lower_donor_image, retain_img,
                       stick, patches, patches_lower, denorm_upper, denorm_lower, o, H, W, (H - W) / 2, P, P_lower, ph, pw);
    return launch_status("tryon_outfit_assemble");
}

extern "C" int pasta_tryon_train_region_assemble(const uint8_t* image, const uint8_t* stick, const uint8_t* retain_mask,
                                                 const uint8_t* gt_parsing, const uint8_t* patches, const uint8_t* patches_lower,
                                                 const uint8_t* denorm_upper, const uint8_t* denorm_lower, const uint8_t* part_masks,
                                                 int arm_a, int arm_b, const uint8_t* erase_masks, const int32_t* erase_hw,
                                                 float* const* outputs, int N, int H, int W, int P, int P_lower, int ph, int pw, int mh_max,
                                                 int mw_max, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && stick && retain_mask && gt_parsing && patches && patches_lower && denorm_upper && denorm_lower && part_masks &&
                erase_masks && erase_hw && outputs, "tryon_train_region_assemble: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= H && P >= 1 && P <= 64 && P_lower >= 1 && P_lower <= 64 &&
                ph >= 1 && pw >= 4 && pw % 4 == 0 && ph * pw <= H * H && mh_max >= 1 && mw_max >= 1,
                "tryon_train_region_assemble: bad shape (pw a multiple of 4)");
    PASTA_CHECK(arm_a >= 0 && arm_a < P && arm_b >= 0 && arm_b < P, "tryon_train_region_assemble: arm parts %d, %d of %d", arm_a, arm_b, P);
    TryonOut o{};
    float** f[9] = {&o.image, &o.style_input, &o.retain, &o.pose, &o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask,
                    &o.denorm_lower_mask, &o.gt_parsing};          // FullBodyBatch.KEYS; real_img is o.image
    const int missing = take_outputs(outputs, f, 9);
    PASTA_CHECK(missing < 0, "tryon_train_region_assemble: output %d is null", missing);
    dim3 grid((unsigned)((H * H + ph * pw / 4 + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(tryon_train_region_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, stick, retain_mask, gt_parsing,
                       patches, patches_lower, denorm_upper, denorm_lower, part_masks, arm_a, arm_b, erase_masks, erase_hw, o, H, W,
                       (H - W) / 2, P, P_lower, ph, pw, mh_max, mw_max);
    return launch_status("tryon_train_region_assemble");
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

extern "C" int pasta_images_keep_to_u8(const float* images, const uint8_t* photo, const uint8_t* keep, uint8_t* out, int N, int H, int Wt,
                                       int c0, int W, int radius, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && photo && keep && out, "images_keep_to_u8: null pointer");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && Wt >= 1 && Wt <= 4096 && W >= 1 && c0 >= 0 && c0 + W <= Wt,
                "images_keep_to_u8: bad shape or crop (columns %d + %d of %d)", c0, W, Wt);
    PASTA_CHECK(radius >= 0 && radius <= KC_MAX_R, "images_keep_to_u8: radius %d (0..%d)", radius, KC_MAX_R);
    // four pixels per thread where every row of every tensor starts on the boundary its wide access needs
    const bool wide = W % 4 == 0 && Wt % 4 == 0 && c0 % 4 == 0 && (uintptr_t)images % 16 == 0 && (uintptr_t)photo % 4 == 0 &&
                      (uintptr_t)keep % 4 == 0 && (uintptr_t)out % 4 == 0;
    const int tile_w = wide ? 64 : 16;
    const int tiles_x = (W + tile_w - 1) / tile_w, tiles_y = (H + KC_TY - 1) / KC_TY;
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
    if (wide)
        hipLaunchKernelGGL(images_keep_to_u8_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, images, photo, keep, out, H, Wt, c0, W, radius,
                           tiles_x);
    else
        hipLaunchKernelGGL(images_keep_to_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, images, photo, keep, out, H, Wt, c0, W, radius,
                           tiles_x);
    return launch_status("images_keep_to_u8");
}

template <int PLANES>
static void launch_photo_paste_mask(bool wide, dim3 grid, hipStream_t stream, const uint8_t* parsing, const uint8_t* palm, const uint8_t* rule,
                                    const float* heads_a, const float* heads_b, uint8_t* out, int H, int W, int Ht, int c0) {
    using namespace pasta;
    if (wide)
        hipLaunchKernelGGL((photo_paste_mask_kernel<4, PLANES>), grid, dim3(256), 0, stream, parsing, palm, rule, heads_a, heads_b, out, H, W, Ht, c0);
    else
        hipLaunchKernelGGL((photo_paste_mask_kernel<1, PLANES>), grid, dim3(256), 0, stream, parsing, palm, rule, heads_a, heads_b, out, H, W, Ht, c0);
}

extern "C" int pasta_photo_paste_mask_u8(const uint8_t* parsing, const uint8_t* palm, const uint8_t* rule, const float* heads_a,
                                         const float* heads_b, int head_planes, uint8_t* out, int N, int H, int W, int Ht, void* stream) {
    using namespace pasta;
    PASTA_CHECK(parsing && rule && out, "photo_paste_mask_u8: null pointer");
    PASTA_CHECK(head_planes == 0 || head_planes == 1 || head_planes == 6, "photo_paste_mask_u8: head_planes %d (0, 1 or 6)", head_planes);
    PASTA_CHECK(!heads_a == (head_planes == 0) && !heads_b == (head_planes != 1),
                "photo_paste_mask_u8: %d head planes want %s", head_planes,
                head_planes == 0 ? "no heads" : head_planes == 1 ? "heads_a and heads_b" : "heads_a alone");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 4096 && Ht >= 1 && Ht <= 4096 && H <= Ht && W >= 1 && W <= Ht,
                "photo_paste_mask_u8: bad shape (%d x %d in a square of %d)", H, W, Ht);
    const int c0 = (Ht - W) / 2;
    // four pixels per thread where every row of every tensor starts on the boundary its wide access needs
    const bool wide = W % 4 == 0 && Ht % 4 == 0 && c0 % 4 == 0 && (uintptr_t)parsing % 4 == 0 && (uintptr_t)palm % 4 == 0 &&
                      (uintptr_t)heads_a % 16 == 0 && (uintptr_t)heads_b % 16 == 0 && (uintptr_t)out % 4 == 0;
    const int per_block = wide ? 1024 : 256;
    dim3 grid((unsigned)((H * W + per_block - 1) / per_block), (unsigned)N);
    if (head_planes == 6)
        launch_photo_paste_mask<6>(wide, grid, (hipStream_t)stream, parsing, palm, rule, heads_a, heads_b, out, H, W, Ht, c0);
    else if (head_planes == 1)
        launch_photo_paste_mask<1>(wide, grid, (hipStream_t)stream, parsing, palm, rule, heads_a, heads_b, out, H, W, Ht, c0);
    else
        launch_photo_paste_mask<0>(wide, grid, (hipStream_t)stream, parsing, palm, rule, heads_a, heads_b, out, H, W, Ht, c0);
    return launch_status("photo_paste_mask_u8");
}
