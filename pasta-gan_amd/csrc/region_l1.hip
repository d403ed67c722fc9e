// The region L1 term of the unpaired (swapped-outfit) pass of training (torch_utils/ops/region_l1_loss.py): the part
// of F.l1_loss that falls into each of the three regions of a swapped image that have a known answer -- the kept body parts
// against `retain`, the upper garment's region against the warped upper patches, the lower garment's against the lower ones --
// for up to four generated images at once, with its gradient with respect to the images.
//   pasta_region_l1_loss            out[k][r] (fp32 [K, 3] in device memory) and, when asked, one byte per pixel and image that
//                                   holds the pixel's region and the three signs of x - t, which is all the backward needs;
//   pasta_region_l1_loss_backward   dx_k from that byte and an upstream gradient [K, 3] that the kernel reads from device memory.
// The byte, not a second reading of the inputs: per pixel the backward then moves K + 12 K bytes instead of 1 + 8 + 12 (the
// targets of one region) + 12 K + 12 K, for K more bytes written by the forward (DESIGN 8k counts both).
#include "recon_window.h"      // wave_sum

namespace pasta {

constexpr int RL_MAX_K = 4;         // images per call
constexpr int RL_PIX = 4;           // pixels per thread: one 16-byte load per fp32 plane
constexpr int RL_SLOTS = RL_MAX_K * 3;

struct RegionImages { const float* x[RL_MAX_K]; };
struct RegionMaps { uint8_t* m[RL_MAX_K]; };
struct RegionMapsIn { const uint8_t* m[RL_MAX_K]; };
struct RegionGrads { float* dx[RL_MAX_K]; };

// The pixel's region by priority: 0 keep, 1 upper, 2 lower, -1 none.
__device__ __forceinline__ int region_of(int keep, float um, float lm) { return keep != 0 ? 0 : um != 0.f ? 1 : lm != 0.f ? 2 : -1; }

// One thread: four consecutive pixels of one sample (H H is a multiple of 4).  The masks are read once for all K images; a
// target is read only by the threads that hold a pixel of its region.  |x - t| is one fp32 subtraction; the sums are fp64, per
// thread, then wave butterflies, then the four waves in order: one partial per (workgroup, image, region), no atomics.
// map byte: bits 0-1 = region + 1 (0: none), bits 2-3, 4-5, 6-7 = channel 0, 1, 2: 0 where x == t (or no region), 1 where
// x > t, 2 where x < t.
__global__ __launch_bounds__(256) void region_l1_kernel(RegionImages im, const float* __restrict__ retain, const float* __restrict__ upper,
                                                        const float* __restrict__ lower, const uint8_t* __restrict__ keep,
                                                        const float* __restrict__ upper_mask, const float* __restrict__ lower_mask,
                                                        RegionMaps maps, double* __restrict__ partials, int K, int HH) {
    __shared__ double red[4][RL_SLOTS];
    const int t = threadIdx.x, n = blockIdx.y;
    const int pix = (blockIdx.x * 256 + t) * RL_PIX;
    double acc[RL_MAX_K][3];
#pragma unroll
    for (int k = 0; k < RL_MAX_K; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;

    if (pix < HH) {
        const int64_t p1 = (int64_t)n * HH + pix;
        const uchar4 k4 = *reinterpret_cast<const uchar4*>(keep + p1);
        const float4 um = *reinterpret_cast<const float4*>(upper_mask + p1), lm = *reinterpret_cast<const float4*>(lower_mask + p1);
        const int reg[RL_PIX] = {region_of(k4.x, um.x, lm.x), region_of(k4.y, um.y, lm.y), region_of(k4.z, um.z, lm.z),
                                 region_of(k4.w, um.w, lm.w)};
        bool has[3] = {false, false, false};
#pragma unroll
        for (int j = 0; j < RL_PIX; j++) { has[0] |= reg[j] == 0; has[1] |= reg[j] == 1; has[2] |= reg[j] == 2; }
        uint32_t code[RL_MAX_K][RL_PIX];
#pragma unroll
        for (int k = 0; k < RL_MAX_K; k++)
#pragma unroll
            for (int j = 0; j < RL_PIX; j++) code[k][j] = (uint32_t)(reg[j] + 1);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int64_t p3 = ((int64_t)n * 3 + ch) * HH + pix;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 t0 = has[0] ? *reinterpret_cast<const float4*>(retain + p3) : zero;
            const float4 t1 = has[1] ? *reinterpret_cast<const float4*>(upper + p3) : zero;
            const float4 t2 = has[2] ? *reinterpret_cast<const float4*>(lower + p3) : zero;
            const float tg[3][RL_PIX] = {{t0.x, t0.y, t0.z, t0.w}, {t1.x, t1.y, t1.z, t1.w}, {t2.x, t2.y, t2.z, t2.w}};
#pragma unroll
            for (int k = 0; k < RL_MAX_K; k++) {
                if (k < K) {
                    const float4 x4 = *reinterpret_cast<const float4*>(im.x[k] + p3);
                    const float xs[RL_PIX] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                    for (int j = 0; j < RL_PIX; j++) {
                        const int r = reg[j];
                        if (r >= 0) {
                            const float tv = r == 0 ? tg[0][j] : r == 1 ? tg[1][j] : tg[2][j];
                            const float d = xs[j] - tv;
                            const double a = (double)fabsf(d);
                            acc[k][0] += r == 0 ? a : 0.0;
                            acc[k][1] += r == 1 ? a : 0.0;
                            acc[k][2] += r == 2 ? a : 0.0;
                            code[k][j] |= (xs[j] > tv ? 1u : xs[j] < tv ? 2u : 0u) << (2 + 2 * ch);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RL_MAX_K; k++)
            if (k < K && maps.m[k])
                *reinterpret_cast<uchar4*>(maps.m[k] + p1) = make_uchar4((uint8_t)code[k][0], (uint8_t)code[k][1], (uint8_t)code[k][2], (uint8_t)code[k][3]);
    }

    // every thread of the workgroup arrives here: the same grouping in every launch.  Slots of images past K are neither summed
    // nor written; the reduce launch does not read them
#pragma unroll
    for (int k = 0; k < RL_MAX_K; k++)
        if (k < K) {
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double s = wave_sum(acc[k][r]);
                if ((t & 63) == 0) red[t >> 6][k * 3 + r] = s;
            }
        }
    __syncthreads();
    if (t < K * 3)
        partials[((int64_t)n * gridDim.x + blockIdx.x) * RL_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// One workgroup, all slots at once, in a fixed order in fp64: thread t adds the partials of workgroups t, t + 256, ... of every
// slot s = k * 3 + r (the K * 3 doubles of a workgroup are contiguous) in registers; then wave butterflies, then the four waves
// in order, and out[k][r] = sum / M as fp32.
__global__ __launch_bounds__(256) void region_l1_reduce_kernel(const double* __restrict__ partials, float* __restrict__ out, int64_t count,
                                                               int K, double M) {
    __shared__ double red[4][RL_SLOTS];
    const int t = threadIdx.x, slots = K * 3;
    double f[RL_SLOTS];
#pragma unroll
    for (int s = 0; s < RL_SLOTS; s++) f[s] = 0.0;
    for (int64_t i = t; i < count; i += 256) {
#pragma unroll
        for (int s = 0; s < RL_SLOTS; s++)
            if (s < slots) f[s] += partials[i * RL_SLOTS + s];
    }
#pragma unroll
    for (int s = 0; s < RL_SLOTS; s++)
        if (s < slots) {
            const double v = wave_sum(f[s]);
            if ((t & 63) == 0) red[t >> 6][s] = v;
        }
    __syncthreads();
    if (t < slots) out[t] = (float)((((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]) / M);
}

// One thread: four consecutive pixels of one sample of image k = blockIdx.z.  q = g[k][r] / (float)M, one fp32 division;
// dx = +q, -q or 0 by the byte's sign code.  Gather form: every dx element is written by exactly one thread.
__global__ __launch_bounds__(256) void region_l1_backward_kernel(RegionMapsIn maps, const float* __restrict__ grad_out, RegionGrads grads,
                                                                 float Mf, int HH) {
    const int n = blockIdx.y, k = blockIdx.z;
    const int pix = (blockIdx.x * 256 + threadIdx.x) * RL_PIX;
    if (pix >= HH) return;
    const float q[3] = {grad_out[k * 3] / Mf, grad_out[k * 3 + 1] / Mf, grad_out[k * 3 + 2] / Mf};
    const uchar4 c4 = *reinterpret_cast<const uchar4*>(maps.m[k] + (int64_t)n * HH + pix);
    const uint32_t code[RL_PIX] = {c4.x, c4.y, c4.z, c4.w};
    float qp[RL_PIX];
#pragma unroll
    for (int j = 0; j < RL_PIX; j++) {
        const uint32_t r = code[j] & 3u;
        qp[j] = r == 1u ? q[0] : r == 2u ? q[1] : r == 3u ? q[2] : 0.f;
    }
    float* dx = grads.dx[k];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float v[RL_PIX];
#pragma unroll
        for (int j = 0; j < RL_PIX; j++) {
            const uint32_t s = (code[j] >> (2 + 2 * ch)) & 3u;
            v[j] = s == 1u ? qp[j] : s == 2u ? -qp[j] : 0.f;
        }
        *reinterpret_cast<float4*>(dx + ((int64_t)n * 3 + ch) * HH + pix) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

static int region_blocks(int H) { return (H * H / RL_PIX + 255) / 256; }

}  // namespace pasta

#define PASTA_REGION_SHAPE_CHECKS(what)                                                                                              \
    PASTA_CHECK(K >= 1 && K <= RL_MAX_K, what ": %d images (1..%d)", K, RL_MAX_K);                                                   \
    PASTA_CHECK(N >= 1 && N <= 65535 && H >= 4 && H <= 4096 && H % 4 == 0, what ": bad shape (N %d, H %d: H a multiple of 4)", N, H)

extern "C" int64_t pasta_region_l1_loss_workspace(int N, int H) {
    using namespace pasta;
    if (N < 1 || N > 65535 || H < 4 || H > 4096 || H % 4 != 0) return 0;
    return (int64_t)N * region_blocks(H) * RL_SLOTS * (int64_t)sizeof(double);
}

extern "C" int pasta_region_l1_loss(const float* const* images, const float* retain, const float* upper, const float* lower,
                                    const uint8_t* keep, const float* upper_mask, const float* lower_mask, float* out,
                                    uint8_t* const* maps, void* workspace, int64_t workspace_bytes, int K, int N, int H, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && retain && upper && lower && keep && upper_mask && lower_mask && out && workspace, "region_l1_loss: null pointer");
    PASTA_REGION_SHAPE_CHECKS("region_l1_loss");
    PASTA_CHECK(workspace_bytes >= pasta_region_l1_loss_workspace(N, H), "region_l1_loss: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)pasta_region_l1_loss_workspace(N, H));
    RegionImages im = {};
    RegionMaps mp = {};
    for (int k = 0; k < K; k++) {
        PASTA_CHECK(images[k], "region_l1_loss: image %d is null", k);
        PASTA_CHECK(!maps || maps[k], "region_l1_loss: map %d is null", k);
        im.x[k] = images[k];
        mp.m[k] = maps ? maps[k] : nullptr;
    }
    const int blocks = region_blocks(H);
    hipLaunchKernelGGL(region_l1_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, (hipStream_t)stream, im, retain, upper, lower, keep,
                       upper_mask, lower_mask, mp, (double*)workspace, K, H * H);
    if (int status = launch_status("region_l1_loss")) return status;
    hipLaunchKernelGGL(region_l1_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, out, (int64_t)N * blocks,
                       K, 3.0 * N * H * H);
    return launch_status("region_l1_loss (reduce)");
}

extern "C" int pasta_region_l1_loss_backward(const uint8_t* const* maps, const float* grad_out, float* const* dx, int K, int N, int H,
                                             void* stream) {
    using namespace pasta;
    PASTA_CHECK(maps && grad_out && dx, "region_l1_loss_backward: null pointer");
    PASTA_REGION_SHAPE_CHECKS("region_l1_loss_backward");
    RegionMapsIn mp = {};
    RegionGrads gr = {};
    for (int k = 0; k < K; k++) {
        PASTA_CHECK(maps[k] && dx[k], "region_l1_loss_backward: map or gradient %d is null", k);
        mp.m[k] = maps[k];
        gr.dx[k] = dx[k];
    }
    hipLaunchKernelGGL(region_l1_backward_kernel, dim3((unsigned)region_blocks(H), (unsigned)N, (unsigned)K), dim3(256), 0, (hipStream_t)stream,
                       mp, grad_out, gr, (float)(3.0 * N * H * H), H * H);
    return launch_status("region_l1_loss_backward");
}
