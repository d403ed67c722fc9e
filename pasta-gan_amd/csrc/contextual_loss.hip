// The contextual loss of the swapped-outfit pass (torch_utils/ops/contextual_loss.py; include/pasta_hip.h states the definition,
// DESIGN 8l what is exact and what it costs): for unit feature vectors x^_i, y^_j ([B, C, N], position contiguous) the N x N
// matrix d_ij = 1 - x^_i . y^_j is never stored; every kernel here forms it 32 x 64 entries at a time in the accumulators of the
// exact fp32-input MFMA (32x32x2) and reduces it along j at once.
//   pasta_contextual_loss            one launch, two sweeps over the column tiles: m_i = min_j d_ij with its arg-min j*, then
//                                    S_i = sum_j w_ij and E_i = sum_j w_ij d_ij / S_i; a second, one-workgroup-per-sample launch
//                                    adds CX_i = exp((1 - m_i c_i) / h) / S_i over the valid rows in a fixed order.
//   pasta_contextual_loss_backward   one more sweep: the tile A_ij = w_ij / S_i stays in the accumulator registers, whose layout
//                                    is already that of the B operand of the next product, sum_j y^_j[c] A_ij; the two rank-one
//                                    terms at j* are added where the gradient is written.
// The tile is computed transposed (MFMA rows = columns j, MFMA columns = rows i), so a lane owns one row i and sixteen columns
// per 32 x 32 product: every row reduction is a chain of fp32 operations in one lane, then the lane's twin (lane ^ 32), then the
// workgroup's other column shares through LDS -- the same order in every launch, no atomics.
#include "recon_window.h"      // wave_sum

namespace pasta {

typedef float cx_f32x16 __attribute__((ext_vector_type(16)));

constexpr int CX_FWD_GROUPS = 1;     // forward: one group of 32 rows per workgroup, its four waves sweep every fourth column tile
                                     // (measured against two groups x two waves, DESIGN 8l: more workgroups for a small N)
constexpr int CX_ROWS = 64;          // backward: rows per workgroup, two groups of 32, each swept by two waves (even and odd column tiles)
constexpr int CX_JT = 64;            // columns per tile and wave: two 32 x 32 products
constexpr int CX_STATS = 5;          // per row: m, j*, S, E, CX
constexpr float CX_NONE = 3.0e38f;   // "no valid column yet"

#ifndef PASTA_CX_BWD_BLOCKS
#define PASTA_CX_BWD_BLOCKS 1         // workgroups of the backward per compute unit the register budget is set for
#endif

struct CxRow {        // what a lane knows about its row
    int i;            // the row; may be >= N in the last workgroup
    int ic;           // min(i, N - 1): every load is in bounds
    bool valid;
};

// The column tile's validity as 64 bits (bit q: column j0 + q exists and is valid), the same value in every lane.
__device__ __forceinline__ uint64_t cx_column_bits(const uint8_t* __restrict__ yv, int N, int j0, int lane) {
    const int j = j0 + lane;
    return __ballot(j < N && (yv == nullptr || yv[j] != 0));
}

// The column a lane holds in accumulator register v of product t of the tile at j0 (the standard C/D map, rows = columns j here).
__device__ __forceinline__ int cx_col(int t, int v, int half) { return 32 * t + 8 * (v >> 2) + 4 * half + (v & 3); }

// acc[t][v] = x^_i . y^_j for the lane's row and its sixteen columns of product t: A operand y^[k][j], B operand x^[k][i], two
// channels per instruction (lanes 0-31 channel k, lanes 32-63 channel k + 1), eight channels per trip with the next trip's ten
// loads issued before this trip's eight products.  Channels past C contribute exact zeros; rows and columns past N read the last
// one again (their results are never used).
__device__ __forceinline__ void cx_dot_tile(const float* __restrict__ xb, const float* __restrict__ yb, int C, int N, int ic, int j0, int lane,
                                            cx_f32x16 (&acc)[2]) {
    const int half = lane >> 5, col = lane & 31;
    const int jc0 = min(j0 + col, N - 1), jc1 = min(j0 + 32 + col, N - 1);
#pragma unroll
    for (int v = 0; v < 16; v++) acc[0][v] = acc[1][v] = 0.f;
    float xf[4], y0[4], y1[4], xn[4] = {}, n0[4] = {}, n1[4] = {};
    auto load = [&](int k, float (&fx)[4], float (&f0)[4], float (&f1)[4]) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k + 2 * u + half;
            const bool ok = kk < C;
            const int row = min(kk, C - 1) * N;
            const float a = xb[row + ic], b0 = yb[row + jc0], b1 = yb[row + jc1];
            fx[u] = ok ? a : 0.f;
            f0[u] = ok ? b0 : 0.f;
            f1[u] = ok ? b1 : 0.f;
        }
    };
    load(0, xf, y0, y1);
    for (int k = 0; k < C; k += 8) {
        if (k + 8 < C) load(k + 8, xn, n0, n1);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0[u], xf[u], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1[u], xf[u], acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { xf[u] = xn[u]; y0[u] = n0[u]; y1[u] = n1[u]; }
    }
}

// (d, j) pairs are ordered by d, then by j: the smallest column wins a tie, whatever the sweep order.
__device__ __forceinline__ void cx_take_min(float& m, int& jm, float d, int j) {
    if (d < m || (d == m && j < jm)) { m = d; jm = j; }
}

__device__ __forceinline__ CxRow cx_row(const uint8_t* __restrict__ xv, int N, int i0, int lane) {
    CxRow r;
    r.i = i0 + (lane & 31);
    r.ic = min(r.i, N - 1);
    r.valid = r.i < N && (xv == nullptr || xv[r.i] != 0);
    return r;
}

// grid (row blocks, B), 256 threads as GROUPS x SPLITS waves: wave w sweeps the 32 rows of group w / SPLITS over the column tiles
// w % SPLITS, w % SPLITS + SPLITS, ...
// stats: [5][B][N] fp32 (j* as its bits).  An invalid row, and every row of a sample without a valid column, gets m 0, j* 0, S 1,
// E 0, CX 0, so that the backward multiplies finite numbers by zero.
template <int GROUPS, int SPLITS>
__global__ __launch_bounds__(256) void cx_forward_kernel(const float* __restrict__ xh, const float* __restrict__ yh, const uint8_t* __restrict__ x_valid,
                                                         const uint8_t* __restrict__ y_valid, float* __restrict__ stats, int B, int C, int N,
                                                         float inv_h) {
    static_assert(GROUPS * SPLITS == 4, "four waves");
    __shared__ float ex_f[GROUPS][SPLITS][2][32];
    __shared__ int ex_i[GROUPS][SPLITS][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = wave / SPLITS, js = wave % SPLITS, half = lane >> 5, col = lane & 31;
    const int b = blockIdx.y;
    const float* xb = xh + (int64_t)b * C * N;
    const float* yb = yh + (int64_t)b * C * N;
    const uint8_t* xv = x_valid ? x_valid + (int64_t)b * N : nullptr;
    const uint8_t* yv = y_valid ? y_valid + (int64_t)b * N : nullptr;
    const CxRow row = cx_row(xv, N, blockIdx.x * (32 * GROUPS) + 32 * grp, lane);
    const bool active = __ballot(row.valid) != 0;          // the same in every wave of a group
    const int tiles = (N + CX_JT - 1) / CX_JT;
    cx_f32x16 acc[2];

    // sweep 1: the smallest distance and where it is
    float m = CX_NONE;
    int jm = 0x7fffffff;
    if (active) {
        for (int jt = js; jt < tiles; jt += SPLITS) {
            const int j0 = jt * CX_JT;
            const uint64_t bits = cx_column_bits(yv, N, j0, lane);
            if (bits == 0) continue;
            cx_dot_tile(xb, yb, C, N, row.ic, j0, lane, acc);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const int q = cx_col(t, v, half);
                    if ((bits >> q) & 1) cx_take_min(m, jm, 1.f - acc[t][v], j0 + q);
                }
        }
        cx_take_min(m, jm, __shfl_xor(m, 32, 64), __shfl_xor(jm, 32, 64));
    }
    if (half == 0) { ex_f[grp][js][0][col] = m; ex_i[grp][js][col] = jm; }
    __syncthreads();
    m = ex_f[grp][0][0][col];
    jm = ex_i[grp][0][col];
#pragma unroll
    for (int s = 1; s < SPLITS; s++) cx_take_min(m, jm, ex_f[grp][s][0][col], ex_i[grp][s][col]);
    const bool found = m < CX_NONE;
    const float c = 1.f / (m + 1e-3f);
    __syncthreads();

    // sweep 2: S = sum w, sum w d
    float S = 0.f, Ed = 0.f;
    if (active) {
        for (int jt = js; jt < tiles; jt += SPLITS) {
            const int j0 = jt * CX_JT;
            const uint64_t bits = cx_column_bits(yv, N, j0, lane);
            if (bits == 0) continue;
            cx_dot_tile(xb, yb, C, N, row.ic, j0, lane, acc);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const float d = 1.f - acc[t][v];
                    const float w = ((bits >> cx_col(t, v, half)) & 1) ? expf((1.f - d * c) * inv_h) : 0.f;
                    S += w;
                    Ed += w * d;
                }
        }
        S += __shfl_xor(S, 32, 64);
        Ed += __shfl_xor(Ed, 32, 64);
    }
    if (half == 0) { ex_f[grp][js][0][col] = S; ex_f[grp][js][1][col] = Ed; }
    __syncthreads();
    if (js == 0 && half == 0 && row.i < N) {
        S = ex_f[grp][0][0][col];
        Ed = ex_f[grp][0][1][col];
#pragma unroll
        for (int s = 1; s < SPLITS; s++) { S += ex_f[grp][s][0][col]; Ed += ex_f[grp][s][1][col]; }
        const bool ok = row.valid && found;
        const int64_t at = (int64_t)b * N + row.i, plane = (int64_t)B * N;
        stats[at] = ok ? m : 0.f;
        stats[plane + at] = __int_as_float(ok ? jm : 0);
        stats[2 * plane + at] = ok ? S : 1.f;
        stats[3 * plane + at] = ok ? Ed / S : 0.f;
        stats[4 * plane + at] = ok ? expf((1.f - m * c) * inv_h) / S : 0.f;
    }
}

// One workgroup per sample: thread t adds CX of rows t, t + 256, ... in fp64, wave butterflies, the four waves in order.
// loss = -log(sum / R); scale = 1 / sum, so that CX_i / (R mean CX) = CX_i scale.  Without a valid row or a valid column: 0 and 0.
__global__ __launch_bounds__(256) void cx_reduce_kernel(const float* __restrict__ stats, const uint8_t* __restrict__ x_valid,
                                                        const uint8_t* __restrict__ y_valid, float* __restrict__ loss, float* __restrict__ scale, int B,
                                                        int N) {
    __shared__ double red[4][3];
    const int t = threadIdx.x, b = blockIdx.x;
    const float* cx = stats + (4 * (int64_t)B + b) * N;
    double sum = 0.0, rows = 0.0, cols = 0.0;
    for (int i = t; i < N; i += 256) {
        sum += (double)cx[i];
        rows += (x_valid == nullptr || x_valid[(int64_t)b * N + i] != 0) ? 1.0 : 0.0;
        cols += (y_valid == nullptr || y_valid[(int64_t)b * N + i] != 0) ? 1.0 : 0.0;
    }
    sum = wave_sum(sum); rows = wave_sum(rows); cols = wave_sum(cols);
    if ((t & 63) == 0) { red[t >> 6][0] = sum; red[t >> 6][1] = rows; red[t >> 6][2] = cols; }
    __syncthreads();
    if (t == 0) {
        sum = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        rows = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        cols = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
        const bool ok = rows > 0.0 && cols > 0.0;
        loss[b] = ok ? (float)(-log(sum / rows)) : 0.f;
        scale[b] = ok ? (float)(1.0 / sum) : 0.f;
    }
}

// grid (row blocks of 64, B), 256 threads as 2 groups x 2 column halves; CT 32-channel tiles of the gradient in registers (8 for
// C <= 256, 16 up to 512: 256 accumulator registers, one wave per SIMD).  Per column tile: the distances again,
// A_ij = w_ij / S_i in the same registers, then for each 32-channel tile of the chunk 32 products G[c][i] += y^T[j][c] A[j][i]
// whose B operand IS accumulator register v (lanes 0-31 hold column q, lanes 32-63 column q + 4: the two K values of one
// instruction) and whose A operand is a coalesced row piece of y^T ([B, N, C]).  Then, with G from both column halves,
//   dx^[c][i] = g_b CX_i scale_b ((c_i / h) (G[c][i] - y^[c][j*]) - c_i^2 (E_i - m_i) / h  y^[c][j*]),   0 for an invalid row.
template <int CT>
__global__ __launch_bounds__(256, PASTA_CX_BWD_BLOCKS) void cx_backward_kernel(const float* __restrict__ xh, const float* __restrict__ yh, const float* __restrict__ yhT,
                                                          const uint8_t* __restrict__ x_valid, const uint8_t* __restrict__ y_valid,
                                                          const float* __restrict__ stats, const float* __restrict__ scale,
                                                          const float* __restrict__ grad_loss, float* __restrict__ dxh, int B, int C, int N,
                                                          float inv_h) {
    __shared__ float ex_g[2][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = wave >> 1, js = wave & 1, half = lane >> 5, col = lane & 31;
    const int b = blockIdx.y, cb = 0;      // the first channel of the workgroup: all C fit in CT tiles
    const float* xb = xh + (int64_t)b * C * N;
    const float* yb = yh + (int64_t)b * C * N;
    const float* ytb = yhT + (int64_t)b * N * C;
    const uint8_t* xv = x_valid ? x_valid + (int64_t)b * N : nullptr;
    const uint8_t* yv = y_valid ? y_valid + (int64_t)b * N : nullptr;
    const CxRow row = cx_row(xv, N, blockIdx.x * CX_ROWS + 32 * grp, lane);
    const bool active = __ballot(row.valid) != 0;
    const int tiles = (N + CX_JT - 1) / CX_JT;
    const int64_t at = (int64_t)b * N + row.ic, plane = (int64_t)B * N;
    const float m = stats[at], S = stats[2 * plane + at], E = stats[3 * plane + at], cxi = stats[4 * plane + at];
    const int jstar = min(max(__float_as_int(stats[plane + at]), 0), N - 1);
    const float c = 1.f / (m + 1e-3f), inv_S = 1.f / S;

    cx_f32x16 G[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++)
#pragma unroll
        for (int v = 0; v < 16; v++) G[ct][v] = 0.f;

    if (active) {
        cx_f32x16 acc[2];
        for (int jt = js; jt < tiles; jt += 2) {
            const int j0 = jt * CX_JT;
            const uint64_t bits = cx_column_bits(yv, N, j0, lane);
            if (bits == 0) continue;
            cx_dot_tile(xb, yb, C, N, row.ic, j0, lane, acc);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const float d = 1.f - acc[t][v];
                    acc[t][v] = ((bits >> cx_col(t, v, half)) & 1) ? expf((1.f - d * c) * inv_h) * inv_S : 0.f;
                }
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                if (cb + 32 * ct >= C) continue;           // uniform
                const int cc = min(cb + 32 * ct + col, C - 1);
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int v = 0; v < 16; v++) {
                        const int j = min(j0 + cx_col(t, v, half), N - 1);     // a column past N has A = 0
                        G[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(ytb[j * (int64_t)C + cc], acc[t][v], G[ct], 0, 0, 0);
                    }
            }
        }
    }

    const float coef = row.valid ? grad_loss[b] * cxi * scale[b] : 0.f;
    const float ka = c * inv_h, kb = c * c * (E - m) * inv_h;
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        if (cb + 32 * ct >= C) continue;                   // uniform over the workgroup
        if (js == 1) {
#pragma unroll
            for (int v = 0; v < 16; v++) ex_g[grp][v][lane] = G[ct][v];
        }
        __syncthreads();
        if (js == 0 && row.i < N) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int ch = cb + 32 * ct + 8 * (v >> 2) + 4 * half + (v & 3);
                if (ch < C) {
                    const float g = G[ct][v] + ex_g[grp][v][lane];
                    const float ys = yb[(int64_t)ch * N + jstar];
                    dxh[((int64_t)b * C + ch) * N + row.i] = row.valid ? coef * (ka * (g - ys) - kb * ys) : 0.f;
                }
            }
        }
        __syncthreads();
    }
}

static bool cx_shape_ok(int B, int C, int N) { return B >= 1 && B <= 65535 && C >= 1 && C <= 512 && N >= 1 && N <= 16384; }
static int64_t cx_stats_floats(int B, int N) { return (int64_t)CX_STATS * B * N; }

}  // namespace pasta

#define PASTA_CX_SHAPE_CHECKS(what)                                                                                                   \
    PASTA_CHECK(cx_shape_ok(B, C, N), what ": bad shape (B %d, C %d, N %d: B <= 65535, C <= 512, N <= 16384)", B, C, N);              \
    PASTA_CHECK(h > 0.f, what ": the bandwidth h must be positive")

extern "C" int64_t pasta_contextual_loss_workspace(int B, int C, int N) {
    using namespace pasta;
    if (!cx_shape_ok(B, C, N)) return 0;
    return (cx_stats_floats(B, N) + B) * (int64_t)sizeof(float);
}

extern "C" int pasta_contextual_loss(const float* xh, const float* yh, const uint8_t* x_valid, const uint8_t* y_valid, float* loss,
                                     void* workspace, int64_t workspace_bytes, int B, int C, int N, float h, void* stream) {
    using namespace pasta;
    PASTA_CHECK(xh && yh && loss && workspace, "contextual_loss: null pointer");
    PASTA_CX_SHAPE_CHECKS("contextual_loss");
    PASTA_CHECK(workspace_bytes >= pasta_contextual_loss_workspace(B, C, N), "contextual_loss: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)pasta_contextual_loss_workspace(B, C, N));
    float* stats = (float*)workspace;
    hipLaunchKernelGGL((cx_forward_kernel<CX_FWD_GROUPS, 4 / CX_FWD_GROUPS>), dim3((unsigned)((N + 32 * CX_FWD_GROUPS - 1) / (32 * CX_FWD_GROUPS)), (unsigned)B),
                       dim3(256), 0, (hipStream_t)stream, xh, yh, x_valid, y_valid, stats, B, C, N, 1.f / h);
    if (int status = launch_status("contextual_loss")) return status;
    hipLaunchKernelGGL(cx_reduce_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const float*)stats, x_valid, y_valid, loss,
                       stats + cx_stats_floats(B, N), B, N);
    return launch_status("contextual_loss (reduce)");
}

extern "C" int pasta_contextual_loss_backward(const float* xh, const float* yh, const float* yhT, const uint8_t* x_valid,
                                              const uint8_t* y_valid, const void* workspace, const float* grad_loss, float* dxh, int B, int C,
                                              int N, float h, void* stream) {
    using namespace pasta;
    PASTA_CHECK(xh && yh && yhT && workspace && grad_loss && dxh, "contextual_loss_backward: null pointer");
    PASTA_CX_SHAPE_CHECKS("contextual_loss_backward");
    const float* stats = (const float*)workspace;
    const dim3 grid((unsigned)((N + CX_ROWS - 1) / CX_ROWS), (unsigned)B);
    if (C <= 256)
        hipLaunchKernelGGL((cx_backward_kernel<8>), grid, dim3(256), 0, (hipStream_t)stream, xh, yh, yhT, x_valid, y_valid, stats,
                           stats + cx_stats_floats(B, N), grad_loss, dxh, B, C, N, 1.f / h);
    else
        hipLaunchKernelGGL((cx_backward_kernel<16>), grid, dim3(256), 0, (hipStream_t)stream, xh, yh, yhT, x_valid, y_valid, stats,
                           stats + cx_stats_floats(B, N), grad_loss, dxh, B, C, N, 1.f / h);
    return launch_status("contextual_loss_backward");
}
