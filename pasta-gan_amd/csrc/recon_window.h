// The SSIM window and tile geometry shared by csrc/recon_metrics.hip (SSIM of the written bytes) and csrc/ssim_loss.hip (the
// differentiable, un-quantised SSIM of the training loss): Wang et al. 2004, 11 x 11 Gaussian of sigma 1.5, valid positions.
#pragma once
#include <math.h>

#include "common.h"

namespace pasta {

constexpr int RS_K = 11, RS_R = RS_K - 1;       // window and halo
constexpr int RS_TW = 32, RS_TH = 22;           // SSIM positions per workgroup: 22 rows of 32
constexpr int RS_IW = RS_TW + RS_R;             // 42 staged columns
constexpr int RS_IH = RS_TH + RS_R;             // 32 staged rows: 32 rows x 8 groups of four columns = 256 threads in the row pass
constexpr int RS_LD = RS_IW + 1;                // 43: odd, so the four rows a half-wave reads in the row pass fall on different banks
constexpr int RS_MAPS = 5;                      // E[a], E[b], E[aa], E[bb], E[ab]

struct ReconWeights { float w[RS_K]; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

static inline int recon_tiles(int extent, int tile) { return (extent - RS_R + tile - 1) / tile; }

static inline ReconWeights recon_weights() {
    // the Gaussian in fp64, normalised; after the rounding to fp32 the centre weight takes up what the sum lacks of 1
    ReconWeights gw;
    double g[RS_K], total = 0.0;
    for (int k = 0; k < RS_K; k++) { g[k] = exp(-0.5 * (k - RS_K / 2) * (k - RS_K / 2) / (1.5 * 1.5)); total += g[k]; }
    double rest = 0.0;
    for (int k = 0; k < RS_K; k++) { gw.w[k] = (float)(g[k] / total); if (k != RS_K / 2) rest += (double)gw.w[k]; }
    gw.w[RS_K / 2] = (float)(1.0 - rest);
    return gw;
}

}  // namespace pasta
