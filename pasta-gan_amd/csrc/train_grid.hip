// The training run's snapshot image on the GPU (setup_snapshot_image_grid, denorm_clothes, combine_parts and save_image_grid,
// training/training_loop_wo_flow_fullbody.py:36-209), which the reference prepares with about ten thousand OpenCV calls on the
// host, keeps as fp32 tensors of all gnum^2 cells on the device and tiles through numpy:
//   pasta_grid_composite_eroded_u8   denorm_clothes (:59-107) for every cell of one garment in one launch: patches and masks
//                                    picked from the per-person pool through an index, every mask eroded 5 x 5;
//   pasta_grid_assemble              the fp32 tensors G_ema takes for cells lo .. lo + n - 1 (:121-175, :580-583);
//   pasta_image_grid_tile_u8         save_image_grid's conversion and tiling (:182-203) into the uint8 canvas;
//   pasta_swap_assemble              pasta_grid_assemble's garment tensors for a TRAINING batch whose samples wear a batch-mate's
//                                    patches (training/swap_outfits.py): per-sample source tables in place of (lo, gnum).
// Cell = row * gnum + col: row is the person (pose, retain, M_inv), col the clothes donor.
#include "common.h"
#include "tryon_common.h"      // Px4, load_px4, store4

#pragma clang fp contract(off)      // the warp-back coordinates must round as csrc/patches.hip's do
#include "patch_erode.h"

namespace pasta {

// ---- indexed eroded composite ----

__global__ __launch_bounds__(256) void grid_composite_eroded_kernel(const uint8_t* __restrict__ pool, const uint8_t* __restrict__ mask_pool,
                                                                    const int32_t* __restrict__ index, const double* __restrict__ minv,
                                                                    const uint8_t* __restrict__ valid, uint8_t* __restrict__ out, int P, int T,
                                                                    int ph, int pw, int H, int W, int r, int tiles_x) {
    __shared__ uint8_t flags[ER_S * ER_S];
    __shared__ uint8_t rows[ER_S * ER_T];
    const int cell = blockIdx.y;
    const auto part_of = [=](int k) {
        const int64_t item = (int64_t)cell * P + k;
        const int t = index[item];
        const bool use = valid[item] && t >= 0 && t < T;        // an index outside the pool reads nothing: the part is skipped
        const int64_t off = (int64_t)(use ? t : 0) * ph * pw * 3;
        return ErPart{pool + off, use ? mask_pool + off : nullptr, minv + item * 9};
    };
    composite_eroded_tile(part_of, out + (int64_t)cell * H * W * 3, nullptr, P, ph, pw, H, W, r, blockIdx.x, tiles_x, flags, rows);
}

// ---- the tensors of a minibatch of cells ----

// a * b rounded to fp32 on its own, for an integer a of at most 29 bits: the double product is exact, so its conversion IS the
// fp32 product, and no contraction setting can fuse it into the subtraction that follows
__device__ __forceinline__ float mul_rounded(int a, float b) { return (float)((double)a * (double)b); }

// torch's x / 127.5 - 1 on the GPU: x * (1 / 127.5f) - 1, as csrc/tryon_common.h's to_unit
__device__ __forceinline__ float grid_to_unit(int v) { return mul_rounded(v, 1.0f / 127.5f) - 1.0f; }

struct GridOut {
    float *denorm_upper_input, *denorm_lower_input, *denorm_upper_mask, *denorm_lower_mask, *style_input, *pose, *retain;
};

// One thread per four consecutive pixels: 12-byte loads from the uint8 images, 16-byte stores into the fp32 planes.
__global__ __launch_bounds__(256) void grid_assemble_kernel(const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                            const uint8_t* __restrict__ image, const uint8_t* __restrict__ stick,
                                                            const uint8_t* __restrict__ retain_mask, const uint8_t* __restrict__ norm_img,
                                                            const uint8_t* __restrict__ norm_lower, GridOut o, int lo, int gnum, int H,
                                                            int ph, int pw, int CU, int CL) {
    const int n = blockIdx.y;
    const int cell = lo + n, row = cell / gnum, col = cell - row * gnum, gap = gnum / 3;
    const int HH = H * H;
    const int pix = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (pix >= HH) {
        // combine_parts (:36-56): the upper patches are the row's own while the trousers are swapped (row < gap), else the
        // donor's; the lower patches are the donor's until the last third (row < 2 gap), then the row's own
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int up = row < gap ? row : col, low = row < 2 * gap ? col : row;
        const int CS = CU + CL;
        for (int ch = 0; ch < CS; ch++) {
            const uint8_t* src = ch < CU ? norm_img + ((int64_t)up * ph * pw + q) * CU + ch : norm_lower + ((int64_t)low * ph * pw + q) * CL + ch - CU;
            const int step = ch < CU ? CU : CL;
            store4(o.style_input + ((int64_t)n * CS + ch) * ph * pw + q, grid_to_unit(src[0]), grid_to_unit(src[step]), grid_to_unit(src[2 * step]),
                   grid_to_unit(src[3 * step]));
        }
        return;
    }
    const Px4 u = load_px4(den_u + ((int64_t)cell * HH + pix) * 3), l = load_px4(den_l + ((int64_t)cell * HH + pix) * 3);
    const Px4 im = load_px4(image + ((int64_t)row * HH + pix) * 3), st = load_px4(stick + ((int64_t)row * HH + pix) * 3);
    const uchar4 rm4 = *reinterpret_cast<const uchar4*>(retain_mask + (int64_t)row * HH + pix);
    const int rm[4] = {rm4.x, rm4.y, rm4.z, rm4.w};
    for (int ch = 0; ch < 3; ch++) {
        float ret[4], pose[4], du[4], dl[4];
        for (int j = 0; j < 4; j++) {
            // retain = retain_mask * image - (1 - retain_mask) (:166), the mask uint8 as in the reference
            ret[j] = mul_rounded(rm[j], grid_to_unit(im.v[3 * j + ch])) - (float)(uint8_t)(1 - rm[j]);
            pose[j] = grid_to_unit(st.v[3 * j + ch]);
            du[j] = grid_to_unit(u.v[3 * j + ch]);
            dl[j] = grid_to_unit(l.v[3 * j + ch]);
        }
        const int64_t oc = ((int64_t)n * 3 + ch) * HH + pix;
        store4(o.retain + oc, ret[0], ret[1], ret[2], ret[3]);
        store4(o.pose + ((int64_t)n * 6 + ch) * HH + pix, pose[0], pose[1], pose[2], pose[3]);
        store4(o.pose + ((int64_t)n * 6 + 3 + ch) * HH + pix, ret[0], ret[1], ret[2], ret[3]);
        store4(o.denorm_upper_input + oc, du[0], du[1], du[2], du[3]);
        store4(o.denorm_lower_input + oc, dl[0], dl[1], dl[2], dl[3]);
    }
    float mu[4], ml[4];
    for (int j = 0; j < 4; j++) {                               // numpy sums uint8 in a wider type: no wrap (:104-105)
        mu[j] = u.v[3 * j] + u.v[3 * j + 1] + u.v[3 * j + 2] > 0 ? 1.f : 0.f;
        ml[j] = l.v[3 * j] + l.v[3 * j + 1] + l.v[3 * j + 2] > 0 ? 1.f : 0.f;
    }
    store4(o.denorm_upper_mask + (int64_t)n * HH + pix, mu[0], mu[1], mu[2], mu[3]);
    store4(o.denorm_lower_mask + (int64_t)n * HH + pix, ml[0], ml[1], ml[2], ml[3]);
}

// ---- the swapped tensors of a training batch ----

struct SwapOut {
    float *denorm_upper_input, *denorm_lower_input, *denorm_upper_mask, *denorm_lower_mask, *style_input;
};

// grid_assemble_kernel's body for the unpaired pass of training (training/swap_outfits.py): sample n wears the upper patches of
// person upper_src[n] and the lower patches of person lower_src[n] of the batch's T people, and den_u / den_l hold its own two
// images.  The person's pose and retain are the paired batch's tensors and are not written again.  A source outside 0 .. T - 1
// reads nothing: its style channels are those of zero bytes.
__global__ __launch_bounds__(256) void swap_assemble_kernel(const uint8_t* __restrict__ den_u, const uint8_t* __restrict__ den_l,
                                                            const uint8_t* __restrict__ norm_img, const uint8_t* __restrict__ norm_lower,
                                                            const int32_t* __restrict__ upper_src, const int32_t* __restrict__ lower_src,
                                                            SwapOut o, int T, int H, int ph, int pw, int CU, int CL) {
    const int n = blockIdx.y;
    const int HH = H * H;
    const int pix = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (pix >= HH) {
        const int q = pix - HH;
        if (q >= ph * pw) return;
        const int up = upper_src[n], low = lower_src[n];
        const bool up_ok = up >= 0 && up < T, low_ok = low >= 0 && low < T;
        const int CS = CU + CL;
        for (int ch = 0; ch < CS; ch++) {
            const bool ok = ch < CU ? up_ok : low_ok;
            const uint8_t* src = ch < CU ? norm_img + ((int64_t)(up_ok ? up : 0) * ph * pw + q) * CU + ch
                                         : norm_lower + ((int64_t)(low_ok ? low : 0) * ph * pw + q) * CL + ch - CU;
            const int step = ch < CU ? CU : CL;
            store4(o.style_input + ((int64_t)n * CS + ch) * ph * pw + q, grid_to_unit(ok ? src[0] : 0), grid_to_unit(ok ? src[step] : 0),
                   grid_to_unit(ok ? src[2 * step] : 0), grid_to_unit(ok ? src[3 * step] : 0));
        }
        return;
    }
    const Px4 u = load_px4(den_u + ((int64_t)n * HH + pix) * 3), l = load_px4(den_l + ((int64_t)n * HH + pix) * 3);
    for (int ch = 0; ch < 3; ch++) {
        const int64_t oc = ((int64_t)n * 3 + ch) * HH + pix;
        store4(o.denorm_upper_input + oc, grid_to_unit(u.v[ch]), grid_to_unit(u.v[3 + ch]), grid_to_unit(u.v[6 + ch]), grid_to_unit(u.v[9 + ch]));
        store4(o.denorm_lower_input + oc, grid_to_unit(l.v[ch]), grid_to_unit(l.v[3 + ch]), grid_to_unit(l.v[6 + ch]), grid_to_unit(l.v[9 + ch]));
    }
    float mu[4], ml[4];
    for (int j = 0; j < 4; j++) {
        mu[j] = u.v[3 * j] + u.v[3 * j + 1] + u.v[3 * j + 2] > 0 ? 1.f : 0.f;
        ml[j] = l.v[3 * j] + l.v[3 * j + 1] + l.v[3 * j + 2] > 0 ? 1.f : 0.f;
    }
    store4(o.denorm_upper_mask + (int64_t)n * HH + pix, mu[0], mu[1], mu[2], mu[3]);
    store4(o.denorm_lower_mask + (int64_t)n * HH + pix, ml[0], ml[1], ml[2], ml[3]);
}

// ---- image grid tiling ----

// save_image_grid:184-186 per element in fp32, as numpy evaluates it: one subtraction and one multiplication (a difference
// times a factor is not a contraction candidate), rint (half to even), clip to [0, 255]; a NaN becomes 0.
__device__ __forceinline__ uint8_t grid_to_u8(float x, float lo, float scale) {
    const float v = rintf((x - lo) * scale);
    return v != v ? 0 : (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
}

template <int C>
__global__ __launch_bounds__(256) void image_grid_tile_kernel(const float* __restrict__ images, uint8_t* __restrict__ canvas, int H, int W,
                                                              int first, int gw, int ox, int oy, int canvas_w, float lo, float scale) {
    const int n = blockIdx.y;
    const int pix = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (pix >= H * W) return;
    const int tile = first + n, ty = tile / gw + oy, tx = tile % gw + ox;
    const int y = pix / W, x = pix - y * W;                     // W is a multiple of 4: the four pixels share a row
    uint8_t px[4 * C];
    for (int ch = 0; ch < C; ch++) {
        const float4 v = *reinterpret_cast<const float4*>(images + ((int64_t)n * C + ch) * H * W + pix);
        px[ch] = grid_to_u8(v.x, lo, scale); px[C + ch] = grid_to_u8(v.y, lo, scale);
        px[2 * C + ch] = grid_to_u8(v.z, lo, scale); px[3 * C + ch] = grid_to_u8(v.w, lo, scale);
    }
    uint8_t* dst = canvas + (((int64_t)ty * H + y) * canvas_w + (int64_t)tx * W + x) * C;
    uint32_t words[C];
    for (int i = 0; i < C; i++)
        words[i] = (uint32_t)px[4 * i] | (uint32_t)px[4 * i + 1] << 8 | (uint32_t)px[4 * i + 2] << 16 | (uint32_t)px[4 * i + 3] << 24;
    if constexpr (C == 3) *reinterpret_cast<uint3*>(dst) = make_uint3(words[0], words[1], words[2]);     // dst is 4-byte aligned
    else *reinterpret_cast<uint32_t*>(dst) = words[0];
}

}  // namespace pasta

extern "C" int pasta_grid_composite_eroded_u8(const uint8_t* pool, const uint8_t* mask_pool, const int32_t* index, const double* minv,
                                              const uint8_t* valid, uint8_t* out, int cells, int P, int T, int ph, int pw, int H, int W,
                                              int radius, void* stream) {
    using namespace pasta;
    PASTA_CHECK(pool && mask_pool && index && minv && valid && out, "grid_composite_eroded_u8: null pointer");
    PASTA_CHECK(cells >= 1 && cells <= 65535 && P >= 1 && T >= 1 && ph >= 1 && pw >= 1 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
                "grid_composite_eroded_u8: bad shape");
    PASTA_CHECK(radius >= 0 && radius <= ER_MAX_R, "grid_composite_eroded_u8: radius %d (0..%d)", radius, ER_MAX_R);
    const int tiles_x = (W + ER_T - 1) / ER_T, tiles_y = (H + ER_T - 1) / ER_T;
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)cells);
    hipLaunchKernelGGL(grid_composite_eroded_kernel, grid, dim3(256), 0, (hipStream_t)stream, pool, mask_pool, index, minv, valid, out, P, T,
                       ph, pw, H, W, radius, tiles_x);
    return launch_status("grid_composite_eroded_u8");
}

extern "C" int pasta_grid_assemble(const uint8_t* denorm_upper, const uint8_t* denorm_lower, const uint8_t* image, const uint8_t* stick,
                                   const uint8_t* retain_mask, const uint8_t* norm_img, const uint8_t* norm_img_lower, float* const* outputs,
                                   int lo, int n, int gnum, int H, int ph, int pw, int c_upper, int c_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(denorm_upper && denorm_lower && image && stick && retain_mask && norm_img && norm_img_lower && outputs,
                "grid_assemble: null pointer");
    PASTA_CHECK(gnum >= 1 && gnum <= 255 && lo >= 0 && n >= 1 && lo + n <= gnum * gnum, "grid_assemble: cells %d .. %d of a %d x %d grid", lo,
                lo + n - 1, gnum, gnum);
    PASTA_CHECK(H >= 4 && H <= 4096 && H % 4 == 0 && ph >= 1 && pw >= 4 && pw % 4 == 0 && c_upper >= 1 && c_lower >= 1,
                "grid_assemble: bad shape (H and pw multiples of 4)");
    GridOut o;
    float** f[7] = {&o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask, &o.denorm_lower_mask, &o.style_input, &o.pose, &o.retain};
    for (int i = 0; i < 7; i++) {
        PASTA_CHECK(outputs[i], "grid_assemble: output %d is null", i);
        *f[i] = outputs[i];
    }
    dim3 grid((unsigned)(((H * H + ph * pw) / 4 + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(grid_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, denorm_upper, denorm_lower, image, stick, retain_mask,
                       norm_img, norm_img_lower, o, lo, gnum, H, ph, pw, c_upper, c_lower);
    return launch_status("grid_assemble");
}

extern "C" int pasta_swap_assemble(const uint8_t* denorm_upper, const uint8_t* denorm_lower, const uint8_t* norm_img,
                                   const uint8_t* norm_img_lower, const int32_t* upper_src, const int32_t* lower_src, float* const* outputs,
                                   int n, int T, int H, int ph, int pw, int c_upper, int c_lower, void* stream) {
    using namespace pasta;
    PASTA_CHECK(denorm_upper && denorm_lower && norm_img && norm_img_lower && upper_src && lower_src && outputs, "swap_assemble: null pointer");
    PASTA_CHECK(n >= 1 && n <= 65535 && T >= 1, "swap_assemble: %d samples of %d people", n, T);
    PASTA_CHECK(H >= 4 && H <= 4096 && H % 4 == 0 && ph >= 1 && pw >= 4 && pw % 4 == 0 && c_upper >= 1 && c_lower >= 1,
                "swap_assemble: bad shape (H and pw multiples of 4)");
    SwapOut o;
    float** f[5] = {&o.denorm_upper_input, &o.denorm_lower_input, &o.denorm_upper_mask, &o.denorm_lower_mask, &o.style_input};
    for (int i = 0; i < 5; i++) {
        PASTA_CHECK(outputs[i], "swap_assemble: output %d is null", i);
        *f[i] = outputs[i];
    }
    dim3 grid((unsigned)(((H * H + ph * pw) / 4 + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(swap_assemble_kernel, grid, dim3(256), 0, (hipStream_t)stream, denorm_upper, denorm_lower, norm_img, norm_img_lower,
                       upper_src, lower_src, o, T, H, ph, pw, c_upper, c_lower);
    return launch_status("swap_assemble");
}

extern "C" int pasta_image_grid_tile_u8(const float* images, uint8_t* canvas, int n, int C, int H, int W, int first, int gw, int ox, int oy,
                                        int canvas_h, int canvas_w, float lo, float scale, void* stream) {
    using namespace pasta;
    PASTA_CHECK(images && canvas, "image_grid_tile_u8: null pointer");
    PASTA_CHECK(n >= 1 && n <= 65535 && (C == 1 || C == 3) && H >= 1 && H <= 4096 && W >= 4 && W <= 4096 && W % 4 == 0,
                "image_grid_tile_u8: bad shape (C 1 or 3, W a multiple of 4)");
    PASTA_CHECK(first >= 0 && gw >= 1 && ox >= 0 && oy >= 0 && canvas_h >= 1 && canvas_w >= 1 && canvas_h % H == 0 && canvas_w % W == 0 &&
                gw + ox <= canvas_w / W && (first + n - 1) / gw + oy < canvas_h / H,
                "image_grid_tile_u8: tiles %d .. %d of %d columns at offset (%d, %d) leave the %d x %d canvas", first, first + n - 1, gw, ox,
                oy, canvas_h, canvas_w);
    dim3 grid((unsigned)((H * W / 4 + 255) / 256), (unsigned)n);
    if (C == 3)
        hipLaunchKernelGGL(image_grid_tile_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, images, canvas, H, W, first, gw, ox, oy, canvas_w,
                           lo, scale);
    else
        hipLaunchKernelGGL(image_grid_tile_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, images, canvas, H, W, first, gw, ox, oy, canvas_w,
                           lo, scale);
    return launch_status("image_grid_tile_u8");
}
