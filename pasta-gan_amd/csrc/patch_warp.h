// OpenCV's fixed-point bilinear warpPerspective, restated (oracle/ref_patches.py): the per-pixel source coordinates, tap
// weights and the sample of one channel.  Shared by csrc/patches.hip (the training set's body-part warps) and
// csrc/tryon_pairs.hip (the eroded composite of the test pairs); an including unit sets `#pragma clang fp contract(off)` first.
#pragma once
#include "common.h"

namespace pasta {

constexpr int PW_TAB = 32;          // sub-pixel positions per pixel
constexpr int PW_BLOCK_W = 64;      // the projective map is evaluated relative to the first column of 64-column blocks

// destination pixel (x, y) -> source coordinates in 1/32 pixel; m = the inverted 3 x 3 matrix (dst -> src), row-major doubles
__device__ __forceinline__ void pw_source(const double* __restrict__ m, int x, int y, int& X, int& Y) {
    const int xb = (x / PW_BLOCK_W) * PW_BLOCK_W;
    const double x1 = (double)(x - xb), xbd = (double)xb, yd = (double)y;
    const double x0 = m[0] * xbd + m[1] * yd + m[2];
    const double y0 = m[3] * xbd + m[4] * yd + m[5];
    const double w0 = m[6] * xbd + m[7] * yd + m[8];
    double w = w0 + m[6] * x1;
    w = w != 0.0 ? (double)PW_TAB / w : 0.0;
    double fx = (x0 + m[0] * x1) * w, fy = (y0 + m[3] * x1) * w;
    fx = fmin(fmax(fx, -2147483648.0), 2147483647.0);
    fy = fmin(fmax(fy, -2147483648.0), 2147483647.0);
    X = (int)rint(fx);              // round half to even
    Y = (int)rint(fy);
}

struct PwTaps { int x0, x1, y0, y1; int w00, w01, w10, w11; bool in00, in01, in10, in11; };

// tap positions and weights of one destination pixel; border = 1: coordinates clamped (replicate), 0: taps outside read 0
__device__ __forceinline__ PwTaps pw_taps(int X, int Y, int sw, int sh, int border) {
    PwTaps t;
    int sx = X >> 5, sy = Y >> 5;
    sx = sx < -32768 ? -32768 : sx > 32767 ? 32767 : sx;           // remap carries short coordinates
    sy = sy < -32768 ? -32768 : sy > 32767 ? 32767 : sy;
    const int ax = X & 31, ay = Y & 31;
    t.w00 = (32 - ay) * (32 - ax) * 32; t.w01 = (32 - ay) * ax * 32;
    t.w10 = ay * (32 - ax) * 32;        t.w11 = ay * ax * 32;
    const int xa = sx, xb = sx + 1, ya = sy, yb = sy + 1;
    const bool xin0 = (unsigned)xa < (unsigned)sw, xin1 = (unsigned)xb < (unsigned)sw;
    const bool yin0 = (unsigned)ya < (unsigned)sh, yin1 = (unsigned)yb < (unsigned)sh;
    t.in00 = border || (xin0 && yin0); t.in01 = border || (xin1 && yin0);
    t.in10 = border || (xin0 && yin1); t.in11 = border || (xin1 && yin1);
    t.x0 = xa < 0 ? 0 : xa >= sw ? sw - 1 : xa; t.x1 = xb < 0 ? 0 : xb >= sw ? sw - 1 : xb;
    t.y0 = ya < 0 ? 0 : ya >= sh ? sh - 1 : ya; t.y1 = yb < 0 ? 0 : yb >= sh ? sh - 1 : yb;
    return t;
}

__device__ __forceinline__ int pw_sample(const uint8_t* __restrict__ img, int sw, int C, int c, const PwTaps& t) {
    const int v00 = t.in00 ? img[((int64_t)t.y0 * sw + t.x0) * C + c] : 0, v01 = t.in01 ? img[((int64_t)t.y0 * sw + t.x1) * C + c] : 0;
    const int v10 = t.in10 ? img[((int64_t)t.y1 * sw + t.x0) * C + c] : 0, v11 = t.in11 ? img[((int64_t)t.y1 * sw + t.x1) * C + c] : 0;
    const int acc = v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11;
    const int r = (acc + (1 << 14)) >> 15;
    return r < 0 ? 0 : r > 255 ? 255 : r;
}

}  // namespace pasta
