// Per-sample preparation of the try-on data sets on the GPU (row f4, the part of UvitonDatasetFull._load_raw_image /
// __getitem__ and of the training loop's float conversions that is not the body-part warps of csrc/patches.hip):
//   pasta_pose_stickman_u8  the pose stick figure (draw_pose_from_cords, dataset.py:704-736), padded, with the line thickness and
//                           the disc radius as arguments: every data set's (2 and 2 at 256 x 192, 5 and 5 at 512 x 320);
//   pasta_tryon_masks_u8    retain mask, gt_parsing, garment images and garment masks (:537-556) of both training sets;
//   pasta_tryon_assemble    erase mask (__getitem__ :951-973) and the loop's conversions (training_loop...:425-456); its
//                           per-pixel body is csrc/tryon_common.h's train_pixel (the erase rule with the restated resize, then
//                           tryon_pixel), shared with the 512 x 320 training kernel of csrc/tryon_pairs.hip;
//   pasta_tryon_mirror_u8   the raw samples of a batch as a mirror shows them (this project's own rule, --mirror-people): the
//                           photograph, the label map with left and right exchanged and the erase mask, before any of the above;
//   pasta_tryon_jitter_u8   the raw samples of a batch after a similarity map and a colour map per item (this project's own rule,
//                           --jitter-people): the photograph resampled from four taps, the label map from the nearest one;
//   pasta_erase_strokes_u8  the erase masks of a batch drawn on the padded square (this project's own rule, --erase-masks strokes):
//                           thick polylines with round caps and joins, exact in integers, after both of the above.
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

// ---- mirrored people (this project's own rule: include/pasta_hip.h, pasta_tryon_mirror_u8) ----

// Byte b of the little-endian words w; with constant b the compiler folds a word of these into byte permutes.
__device__ __forceinline__ uint32_t word_byte(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 0xffu; }

// One launch for a batch: item n = blockIdx.y; its threads are, in this order, the image's units, the label map's units and the
// erase mask's bytes.  WIDE: a unit is 16 pixels of a row (W % 16 == 0, 16-byte aligned tensors): three 16-byte loads of the
// image, the pixel order reversed in registers, three 16-byte stores at the mirrored place; one load and one store of the labels.
// Otherwise a unit is one pixel.  An item whose flag is 0 is copied; the table (in LDS) is applied to flagged items only.
template <bool WIDE>
__global__ __launch_bounds__(256) void tryon_mirror_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                           const uint8_t* __restrict__ erase, const int32_t* __restrict__ erase_hw,
                                                           const uint8_t* __restrict__ flip, const uint8_t* __restrict__ lut,
                                                           uint8_t* __restrict__ image_out, uint8_t* __restrict__ parsing_out,
                                                           uint8_t* __restrict__ erase_out, int H, int W, int eh, int ew) {
    __shared__ uint8_t table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    constexpr int PX = WIDE ? 16 : 1;
    const int n = blockIdx.y;
    const bool f = flip[n] != 0;                         // uniform over the workgroup
    const int cw = W / PX, units = H * cw;
    int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 2 * units) {
        const bool labels = t >= units;
        if (labels) t -= units;
        const int y = t / cw, x0 = (t - y * cw) * PX;
        const int64_t row = ((int64_t)n * H + y) * W;
        const int64_t src = row + x0, dst = row + (f ? W - PX - x0 : x0);
        if constexpr (WIDE) {
            if (!labels) {
                const uint4* s = reinterpret_cast<const uint4*>(image + src * 3);
                uint4* d = reinterpret_cast<uint4*>(image_out + dst * 3);
                const uint4 a = s[0], b = s[1], c = s[2];
                if (!f) { d[0] = a; d[1] = b; d[2] = c; return; }
                const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
                uint32_t o[12];
#pragma unroll
                for (int k = 0; k < 12; k++) {           // byte j of the output is channel j % 3 of pixel 15 - j / 3
                    o[k] = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) o[k] |= word_byte(w, (15 - (4 * k + i) / 3) * 3 + (4 * k + i) % 3) << (8 * i);
                }
                d[0] = make_uint4(o[0], o[1], o[2], o[3]);
                d[1] = make_uint4(o[4], o[5], o[6], o[7]);
                d[2] = make_uint4(o[8], o[9], o[10], o[11]);
            } else {
                const uint4 a = *reinterpret_cast<const uint4*>(parsing + src);
                uint4* d = reinterpret_cast<uint4*>(parsing_out + dst);
                if (!f) { *d = a; return; }
                const uint32_t w[4] = {a.x, a.y, a.z, a.w};
                uint32_t o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    o[k] = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) o[k] |= (uint32_t)table[word_byte(w, 15 - (4 * k + i))] << (8 * i);
                }
                *d = make_uint4(o[0], o[1], o[2], o[3]);
            }
        } else {
            if (!labels) {
                for (int ch = 0; ch < 3; ch++) image_out[dst * 3 + ch] = image[src * 3 + ch];
            } else {
                const uint8_t L = parsing[src];
                parsing_out[dst] = f ? table[L] : L;
            }
        }
        return;
    }
    t -= 2 * units;
    if (erase == nullptr || t >= eh * ew) return;
    const int y = t / ew, x = t - y * ew;
    // the sample's own size, held inside the stacked tensor whatever the device array says
    const int hn = min(max(erase_hw[2 * n], 0), eh), wn = min(max(erase_hw[2 * n + 1], 0), ew);
    const int64_t base = ((int64_t)n * eh + y) * ew;
    erase_out[base + x] = erase[base + ((f && y < hn && x < wn) ? wn - 1 - x : x)];
}

// ---- jittered people (this project's own rule: include/pasta_hip.h, pasta_tryon_jitter_u8) ----

// An int64 coordinate held into 0 .. hi: every tap and every label read lies inside its item whatever the six numbers are.
__device__ __forceinline__ int jitter_clamp(int64_t v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); }

// The photograph's output pixel whose source coordinate is (X, Y) in Q16 -> out[3]: four taps at 1/32 pixel with a replicated
// border, then the Q8 colour map M[3][4].  img: the item's H x W x 3 bytes.  The sums wrap in 64 bits, as the statement's do.
__device__ __forceinline__ void jitter_photo_pixel(const uint8_t* __restrict__ img, int H, int W, uint64_t X, uint64_t Y, const int32_t* M,
                                                   uint32_t* out) {
    const int64_t Xq = (int64_t)(X + 1024u) >> 11, Yq = (int64_t)(Y + 1024u) >> 11;
    const int ax = (int)(Xq & 31), ay = (int)(Yq & 31);
    const int64_t ix = Xq >> 5, iy = Yq >> 5;
    const int x0 = jitter_clamp(ix, W - 1), x1 = jitter_clamp(ix + 1, W - 1);
    const int y0 = jitter_clamp(iy, H - 1), y1 = jitter_clamp(iy + 1, H - 1);
    const uint8_t* p00 = img + (y0 * W + x0) * 3;        // < 16384 * 16384 * 3: an int
    const uint8_t* p01 = img + (y0 * W + x1) * 3;
    const uint8_t* p10 = img + (y1 * W + x0) * 3;
    const uint8_t* p11 = img + (y1 * W + x1) * 3;
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 512) >> 10;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t m = ((int64_t)M[4 * c] * v[0] + (int64_t)M[4 * c + 1] * v[1] + (int64_t)M[4 * c + 2] * v[2] + M[4 * c + 3] + 128) >> 8;
        out[c] = (uint32_t)(m < 0 ? 0 : (m > 255 ? 255 : m));
    }
}

// One launch for a batch: item n = blockIdx.y; its threads are the image's units, then the label map's units.  A unit is PX
// consecutive output pixels of a row, gathered through the cache and stored together.  WIDE (W % 16 == 0, 16-byte aligned
// tensors): 16 pixels, three 16-byte stores of the image and one of the labels.  Otherwise one pixel, byte stores.  The six and
// twelve numbers of the item are uniform over the workgroup (scalar loads); an item whose numbers are the identity is copied.
template <bool WIDE>
__global__ __launch_bounds__(256) void tryon_jitter_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ parsing,
                                                           const int64_t* __restrict__ affine, const int32_t* __restrict__ colour,
                                                           uint8_t* __restrict__ image_out, uint8_t* __restrict__ parsing_out, int H, int W) {
    constexpr int PX = WIDE ? 16 : 1;
    const int n = blockIdx.y;
    const int64_t* q = affine + (int64_t)n * 6;
    const uint64_t A = (uint64_t)q[0], B = (uint64_t)q[1], C = (uint64_t)q[2], D = (uint64_t)q[3], E = (uint64_t)q[4], F = (uint64_t)q[5];
    int32_t M[12];
    bool same = A == 65536u && B == 0 && C == 0 && D == 0 && E == 65536u && F == 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        M[k] = colour[(int64_t)n * 12 + k];
        same = same && M[k] == (k % 5 == 0 ? 256 : 0);
    }
    const int cw = W / PX, units = H * cw;
    int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * units) return;
    const bool labels = t >= units;
    if (labels) t -= units;
    const int y = t / cw, x0 = (t - y * cw) * PX;
    const int64_t item = (int64_t)n * H * W, at = item + (int64_t)y * W + x0;
    uint64_t X = A * (uint64_t)x0 + B * (uint64_t)y + C, Y = D * (uint64_t)x0 + E * (uint64_t)y + F;
    if (!labels) {
        const uint8_t* img = image + item * 3;
        if constexpr (WIDE) {
            uint4* d = reinterpret_cast<uint4*>(image_out + at * 3);
            if (same) {
                const uint4* s = reinterpret_cast<const uint4*>(image + at * 3);
                const uint4 a = s[0], b = s[1], c = s[2];
                d[0] = a; d[1] = b; d[2] = c;
                return;
            }
            uint32_t o[12];
#pragma unroll
            for (int k = 0; k < 12; k++) o[k] = 0;
#pragma unroll
            for (int p = 0; p < 16; p++, X += A, Y += D) {
                uint32_t px[3];
                jitter_photo_pixel(img, H, W, X, Y, M, px);
#pragma unroll
                for (int c = 0; c < 3; c++) o[(3 * p + c) >> 2] |= px[c] << (8 * ((3 * p + c) & 3));
            }
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d[2] = make_uint4(o[8], o[9], o[10], o[11]);
        } else {
            uint32_t px[3];
            if (same) {
                for (int c = 0; c < 3; c++) px[c] = image[at * 3 + c];
            } else {
                jitter_photo_pixel(img, H, W, X, Y, M, px);
            }
            for (int c = 0; c < 3; c++) image_out[at * 3 + c] = (uint8_t)px[c];
        }
        return;
    }
    const uint8_t* lab = parsing + item;
    if constexpr (WIDE) {
        uint4* d = reinterpret_cast<uint4*>(parsing_out + at);
        if (same) { *d = *reinterpret_cast<const uint4*>(parsing + at); return; }
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 16; p++, X += A, Y += D) {
            const int lx = jitter_clamp((int64_t)(X + 32768u) >> 16, W - 1), ly = jitter_clamp((int64_t)(Y + 32768u) >> 16, H - 1);
            o[p >> 2] |= (uint32_t)lab[ly * W + lx] << (8 * (p & 3));
        }
        *d = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int lx = jitter_clamp((int64_t)(X + 32768u) >> 16, W - 1), ly = jitter_clamp((int64_t)(Y + 32768u) >> 16, H - 1);
        parsing_out[at] = same ? parsing[at] : lab[ly * W + lx];
    }
}

// ---- erase strokes (this project's own rule: include/pasta_hip.h, pasta_erase_strokes_u8) ----

constexpr int STROKE_SEGMENTS = 64, STROKE_TILE = 64;

// The point (X, Y), in 1/8 pixel as the segment p0 -> p1 is, lies within r (r2 = r * r) of the segment.  With the Q3 clamps and
// S <= 1024 every difference is below 2^14: the dot products and the cross product fit an int, its square and r2 * L need 64 bits.
__device__ __forceinline__ bool stroke_hit(int X, int Y, int x0, int y0, int x1, int y1, int r2) {
    const int dx = x1 - x0, dy = y1 - y0, vx = X - x0, vy = Y - y0;
    const int t = vx * dx + vy * dy, L = dx * dx + dy * dy;
    if (t <= 0) return vx * vx + vy * vy <= r2;                       // also p0 == p1: a disc
    if (t >= L) { const int wx = X - x1, wy = Y - y1; return wx * wx + wy * wy <= r2; }
    const int cr = vx * dy - vy * dx;
    return (int64_t)cr * cr <= (int64_t)r2 * L;
}

// One launch for a batch: item n = blockIdx.y, blockIdx.x one 64 x 64 tile of its S x S mask.  The item's segments go to LDS, the
// first wave keeps those whose bounding box grown by r meets the tile (one segment per lane, one ballot), and thread t walks the
// kept ones for the 16 pixels from column 16 (t % 4) of the tile's row t / 4.  WIDE (S % 16 == 0, `out` 16-byte aligned): one
// 16-byte store; otherwise byte stores with the column checked.
template <bool WIDE>
__global__ __launch_bounds__(256) void erase_strokes_kernel(const int32_t* __restrict__ segments, const int32_t* __restrict__ counts,
                                                            uint8_t* __restrict__ out, int S, int tiles) {
    __shared__ int32_t seg[STROKE_SEGMENTS * 5];
    __shared__ unsigned long long kept;
    const int n = blockIdx.y;
    const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
    int count = counts[n];
    count = count < 0 ? 0 : (count > STROKE_SEGMENTS ? STROKE_SEGMENTS : count);
    for (int i = threadIdx.x; i < count * 5; i += 256) seg[i] = segments[(int64_t)n * STROKE_SEGMENTS * 5 + i];
    __syncthreads();
    if (threadIdx.x < 64) {
        bool meets = false;
        if ((int)threadIdx.x < count) {
            const int32_t* q = seg + 5 * threadIdx.x;
            const int r = q[4], lo_x = 8 * STROKE_TILE * tx, lo_y = 8 * STROKE_TILE * ty, span = 8 * (STROKE_TILE - 1);
            meets = min(q[0], q[2]) - r <= lo_x + span && max(q[0], q[2]) + r >= lo_x && min(q[1], q[3]) - r <= lo_y + span &&
                    max(q[1], q[3]) + r >= lo_y;
        }
        const unsigned long long ballot = __ballot(meets);
        if (threadIdx.x == 0) kept = ballot;
    }
    __syncthreads();
    const int y = STROKE_TILE * ty + (threadIdx.x >> 2), xb = STROKE_TILE * tx + 16 * (threadIdx.x & 3);
    if (y >= S || xb >= S) return;
    unsigned long long todo = kept;
    uint32_t hit = 0;                                                    // bit p: pixel xb + p
    const int Y = 8 * y, X = 8 * xb;
    while (todo) {                                                       // no kept segment: zeros, and LDS is not read again
        const int32_t* q = seg + 5 * (__ffsll(todo) - 1);
        todo &= todo - 1;
        const int x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], r = q[4];
        if (Y < min(y0, y1) - r || Y > max(y0, y1) + r || X + 120 < min(x0, x1) - r || X > max(x0, x1) + r) continue;
#pragma unroll
        for (int p = 0; p < 16; p++)
            if (stroke_hit(X + 8 * p, Y, x0, y0, x1, y1, r * r)) hit |= 1u << p;
    }
    uint8_t* row = out + ((int64_t)n * S + y) * S + xb;
    if constexpr (WIDE) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = (((hit >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u;       // bit j -> byte j
        *reinterpret_cast<uint4*>(row) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int p = 0; p < 16 && xb + p < S; p++) row[p] = (uint8_t)((hit >> p) & 1u);
    }
}

}  // namespace pasta

extern "C" int pasta_erase_strokes_u8(const int32_t* segments, const int32_t* counts, uint8_t* out, int n, int S, void* stream) {
    using namespace pasta;
    PASTA_CHECK(n >= 0 && n <= 65535 && S >= 1 && S <= 1024, "erase_strokes_u8: bad shape (n %d, S %d)", n, S);
    if (n == 0) return 0;
    PASTA_CHECK(segments && counts && out, "erase_strokes_u8: null pointer");
    const int tiles = (S + STROKE_TILE - 1) / STROKE_TILE;
    dim3 grid((unsigned)(tiles * tiles), (unsigned)n);
    if (S % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(erase_strokes_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, segments, counts, out, S, tiles);
    else
        hipLaunchKernelGGL(erase_strokes_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, segments, counts, out, S, tiles);
    return launch_status("erase_strokes_u8");
}

extern "C" int pasta_tryon_jitter_u8(const uint8_t* image, const uint8_t* parsing, const int64_t* affine, const int32_t* colour,
                                     uint8_t* image_out, uint8_t* parsing_out, int N, int H, int W, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && affine && colour && image_out && parsing_out, "tryon_jitter_u8: null pointer");
    PASTA_CHECK(image_out != image && parsing_out != parsing, "tryon_jitter_u8: an output is its input (the entry is out of place)");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "tryon_jitter_u8: bad shape (N %d, %d x %d)", N, H, W);
    const uintptr_t all = (uintptr_t)image | (uintptr_t)parsing | (uintptr_t)image_out | (uintptr_t)parsing_out;
    const bool wide = W % 16 == 0 && all % 16 == 0;
    const int64_t threads = 2 * (int64_t)H * (W / (wide ? 16 : 1));                             // <= 2^29: an int in the kernel
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N);
    if (wide)
        hipLaunchKernelGGL(tryon_jitter_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, affine, colour, image_out,
                           parsing_out, H, W);
    else
        hipLaunchKernelGGL(tryon_jitter_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, affine, colour, image_out,
                           parsing_out, H, W);
    return launch_status("tryon_jitter_u8");
}

extern "C" int pasta_tryon_mirror_u8(const uint8_t* image, const uint8_t* parsing, const uint8_t* erase_masks, const int32_t* erase_hw,
                                     const uint8_t* flip, const uint8_t* lut, uint8_t* image_out, uint8_t* parsing_out,
                                     uint8_t* erase_out, int N, int H, int W, int mh_max, int mw_max, void* stream) {
    using namespace pasta;
    PASTA_CHECK(image && parsing && flip && lut && image_out && parsing_out, "tryon_mirror_u8: null pointer");
    PASTA_CHECK(image_out != image && parsing_out != parsing && (erase_out == nullptr || erase_out != erase_masks),
                "tryon_mirror_u8: an output is its input (the entry is out of place)");
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "tryon_mirror_u8: bad shape (N %d, %d x %d)", N, H, W);
    const bool masks = erase_masks != nullptr;
    PASTA_CHECK(masks == (erase_out != nullptr), "tryon_mirror_u8: erase_masks and erase_out are null together or not at all");
    PASTA_CHECK(!masks || (erase_hw && mh_max >= 1 && mh_max <= 16384 && mw_max >= 1 && mw_max <= 16384),
                "tryon_mirror_u8: erase masks need erase_hw and a stack of 1..16384 rows and columns (%d x %d)", mh_max, mw_max);
    const int eh = masks ? mh_max : 0, ew = masks ? mw_max : 0;
    const uintptr_t all = (uintptr_t)image | (uintptr_t)parsing | (uintptr_t)image_out | (uintptr_t)parsing_out;
    const bool wide = W % 16 == 0 && all % 16 == 0;
    const int64_t threads = 2 * (int64_t)H * (W / (wide ? 16 : 1)) + (int64_t)eh * ew;         // < 2^30: an int in the kernel
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N);
    if (wide)
        hipLaunchKernelGGL(tryon_mirror_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, erase_masks, erase_hw, flip, lut,
                           image_out, parsing_out, erase_out, H, W, eh, ew);
    else
        hipLaunchKernelGGL(tryon_mirror_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, image, parsing, erase_masks, erase_hw, flip, lut,
                           image_out, parsing_out, erase_out, H, W, eh, ew);
    return launch_status("tryon_mirror_u8");
}

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
