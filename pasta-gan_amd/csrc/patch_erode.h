// The warp-back composite with an eroded mask, one 16 x 16 output tile per block: shared by csrc/tryon_pairs.hip (the test
// pairs' pasta_patch_composite_eroded_u8) and csrc/train_grid.hip (the snapshot grid's indexed composite), which differ only
// in where a part's patch, mask and matrix are found.  An including unit sets `#pragma clang fp contract(off)` first.
#pragma once
#include "patch_warp.h"

namespace pasta {

constexpr int ER_T = 16;            // output tile side: one thread per pixel of a 16 x 16 tile
constexpr int ER_MAX_R = 8;         // largest erosion radius (a 17 x 17 box)
constexpr int ER_S = ER_T + 2 * ER_MAX_R;

struct ErPart { const uint8_t* patch; const uint8_t* mask; const double* m; };      // mask == nullptr: the part is skipped

// patch_composite_u8_kernel with cv2.erode(mask, ones(2r+1, 2r+1)) of the warped-back mask before the == 255 test.  Since
// 255 is the largest uint8, the eroded channel 0 is 255 exactly where every in-image pixel within +-r has channel 0 == 255
// (cv2's default erode border: pixels outside the image do not erode).  Per part: the == 255 flags of the tile and an r-pixel
// halo go to LDS, are AND-ed along rows and then along columns; the running RGB stays in registers.  r is a run-time value that
// is the same in every thread of the block (a launch's scalar, or the radius of the block's sample); with r == 0 a part is
// patch_composite_u8_kernel's own test and touches neither LDS nor a barrier.
// part_of(k) names part k of this block's image (the same answer in every thread of the block); out: the image [H, W, 3];
// part_mask: its [P, H, W] masks or nullptr; flags [ER_S * ER_S] and rows [ER_S * ER_T]: the block's LDS.  256 threads.
template <class PartOf>
__device__ __forceinline__ void composite_eroded_tile(PartOf part_of, uint8_t* __restrict__ out, uint8_t* __restrict__ part_mask, int P, int ph,
                                                      int pw, int H, int W, int r, int tile, int tiles_x, uint8_t* flags, uint8_t* rows) {
    const int tx0 = (tile % tiles_x) * ER_T, ty0 = (tile / tiles_x) * ER_T;
    const int S = ER_T + 2 * r;
    const int ty = threadIdx.x / ER_T, tx = threadIdx.x % ER_T;
    const int y = ty0 + ty, x = tx0 + tx;
    const bool mine = y < H && x < W;
    int red = 0, green = 0, blue = 0;
    for (int k = 0; k < P; k++) {
        const ErPart part = part_of(k);
        if (!part.mask) {                                       // uniform across the block: no barrier is skipped by a part
            if (part_mask && mine) part_mask[((int64_t)k * H + y) * W + x] = 0;
            continue;
        }
        if (r > 0) {                                            // uniform across the block, as r is
            for (int i = threadIdx.x; i < S * S; i += 256) {
                const int gy = ty0 - r + i / S, gx = tx0 - r + i % S;
                uint8_t f = 1;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    int X, Y;
                    pw_source(part.m, gx, gy, X, Y);
                    f = pw_sample(part.mask, pw, 3, 0, pw_taps(X, Y, pw, ph, 0)) == 255;
                }
                flags[i] = f;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < S * ER_T; i += 256) {
                const int ry = i / ER_T, rx = i % ER_T;
                uint8_t f = 1;
                for (int d = 0; d <= 2 * r; d++) f &= flags[ry * S + rx + d];
                rows[i] = f;
            }
            __syncthreads();
        }
        if (mine) {
            uint8_t hit = 1;
            if (r > 0)
                for (int d = 0; d <= 2 * r; d++) hit &= rows[(ty + d) * ER_T + tx];
            if (hit) {                                          // r == 0: the pixel's own mask value decides, no LDS and no barrier
                int X, Y;
                pw_source(part.m, x, y, X, Y);
                const PwTaps t = pw_taps(X, Y, pw, ph, 0);
                if (r == 0) hit = pw_sample(part.mask, pw, 3, 0, t) == 255;
                if (hit) {
                    red = pw_sample(part.patch, pw, 3, 0, t); green = pw_sample(part.patch, pw, 3, 1, t); blue = pw_sample(part.patch, pw, 3, 2, t);
                }
            }
            if (part_mask) part_mask[((int64_t)k * H + y) * W + x] = hit;
        }
        // the next part writes `flags` only after this barrier pair, and `rows` only after its own first barrier
    }
    if (mine) {
        uint8_t* o = out + ((int64_t)y * W + x) * 3;
        o[0] = (uint8_t)red; o[1] = (uint8_t)green; o[2] = (uint8_t)blue;
    }
}

}  // namespace pasta
