// The body-part geometry of a batch on the GPU (training/patch_pipeline.py, part_geometry): what part_matrices and
// adjugate_inverse do on the host in numpy, one part at a time, as ONE launch for the M distinct people of a batch.
//   pasta_part_geometry   per (person, part): the source quadrilateral (part_quadrilateral restated operation for operation in
//                         float32), the two 8 x 8 systems of perspective_matrix solved in float64 by the elimination
//                         include/pasta_hip.h states, and the adjugate inverses of both solutions (adjugate_inverse's expressions).
// One thread per (person, part, direction): direction 0 solves image -> patch and inverts it, direction 1 patch -> image.  The
// pivot search makes the row index a run-time value, so each thread's 8 x 9 system lives in LDS (64 threads x 576 B = 36 KB), never
// in a private array; the pivot row (0..7 by construction) is the only data-dependent address of the kernel.
#include "common.h"
#include "tryon_common.h"      // tr_rounded: the library is built with -ffp-contract=fast, every product here rounds on its own

namespace pasta {

constexpr int PG_THREADS = 64;
constexpr int PG_PARTS = 10;

// joints of JOINT_ORDER (training/patch_pipeline.py)
enum { J_NOSE = 0, J_RSHO = 2, J_RELB = 3, J_RWRI = 4, J_LSHO = 5, J_LELB = 6, J_LWRI = 7, J_RHIP = 8, J_RKNEE = 9, J_RANK = 10, J_LHIP = 11,
       J_LKNEE = 12, J_LANK = 13 };

struct PgPoint { float x, y; };

__device__ __forceinline__ bool pg_seen(const double* __restrict__ kp, int j) { return kp[j * 3 + 2] >= 0.1; }
// np.float32(joints[j, :2]), then pts[:, 0] + x_pad in float32
__device__ __forceinline__ PgPoint pg_point(const double* __restrict__ kp, int j, float x_pad) {
    PgPoint p = {(float)kp[j * 3] + x_pad, (float)kp[j * 3 + 1]};
    return p;
}

// _box_around(p, q, ratio): [p + n, p - n, q - n, q + n], n = (-seg.y, seg.x) * ratio
__device__ __forceinline__ void pg_box(PgPoint p, PgPoint q, float ratio, PgPoint* out) {
    const float sx = q.x - p.x, sy = q.y - p.y;
    const float nx = tr_rounded(-sy * ratio), ny = tr_rounded(sx * ratio);
    out[0] = {p.x + nx, p.y + ny};
    out[1] = {p.x - nx, p.y - ny};
    out[2] = {q.x - nx, q.y - ny};
    out[3] = {q.x + nx, q.y + ny};
}

// part_quadrilateral: false when the part's key points are missing
__device__ inline bool pg_quadrilateral(const double* __restrict__ kp, int part, int image_height, float x_pad, int shin_fallback, PgPoint* quad) {
    if (part == 0) {                                    // torso: the four points themselves
        if (!(pg_seen(kp, J_LSHO) && pg_seen(kp, J_LHIP) && pg_seen(kp, J_RHIP) && pg_seen(kp, J_RSHO))) return false;
        quad[0] = pg_point(kp, J_LSHO, x_pad); quad[1] = pg_point(kp, J_LHIP, x_pad);
        quad[2] = pg_point(kp, J_RHIP, x_pad); quad[3] = pg_point(kp, J_RSHO, x_pad);
        return true;
    }
    if (part == 1) {                                    // head
        if (!(pg_seen(kp, J_LSHO) && pg_seen(kp, J_RSHO))) return false;
        const PgPoint p0 = pg_point(kp, J_LSHO, x_pad), p1 = pg_point(kp, J_RSHO, x_pad);
        if (!pg_seen(kp, J_NOSE)) {                     // without the nose: a square above the shoulders
            const float sx = p1.x - p0.x, sy = p1.y - p0.y;
            float nx = -sy, ny = sx;
            if (ny > 0.0f) { nx = -nx; ny = -ny; }
            quad[0] = {p0.x + nx, p0.y + ny}; quad[1] = p0; quad[2] = p1; quad[3] = {p1.x + nx, p1.y + ny};
            return true;
        }
        const PgPoint p2 = pg_point(kp, J_NOSE, x_pad);
        const PgPoint neck = {tr_rounded(0.5f * (p0.x + p1.x)), tr_rounded(0.5f * (p0.y + p1.y))};
        const PgPoint top = {neck.x + tr_rounded(2.0f * (p2.x - neck.x)), neck.y + tr_rounded(2.0f * (p2.y - neck.y))};
        PgPoint box[4];
        pg_box(top, neck, 0.5f, box);
        quad[0] = box[1]; quad[1] = box[2]; quad[2] = box[3]; quad[3] = box[0];
        return true;
    }
    // limbs: parts 2..5 the arms, 6 / 8 the thighs, 7 / 9 the shins
    const int first = part == 2 ? J_LSHO : part == 3 ? J_LELB : part == 4 ? J_RSHO : part == 5 ? J_RELB : part == 6 ? J_LHIP : part == 7 ? J_LKNEE
                    : part == 8 ? J_RHIP : J_RKNEE;
    const int second = part == 2 ? J_LELB : part == 3 ? J_LWRI : part == 4 ? J_RELB : part == 5 ? J_RWRI : part == 6 ? J_LKNEE : part == 7 ? J_LANK
                     : part == 8 ? J_RKNEE : J_RANK;
    if (!pg_seen(kp, first)) return false;
    const PgPoint p = pg_point(kp, first, x_pad);
    if (pg_seen(kp, second)) {
        pg_box(p, pg_point(kp, second, x_pad), 0.25f, quad);
        return true;
    }
    const bool thigh = part == 6 || part == 8, shin = part == 7 || part == 9;
    if (!(thigh || (shin && shin_fallback))) return false;
    const PgPoint down = {p.x, (float)(image_height - 1)};    // straight down to the image's last row
    pg_box(p, down, 0.25f, quad);
    return true;
}

// adjugate_inverse: cofactor times 1.0 / det, zeros when det == 0
__device__ inline void pg_inverse(const double* m, double* out) {
    const auto pd = [](double a, double b, double c, double d) { return tr_rounded(a * b) - tr_rounded(c * d); };
    double c[9];
    c[0] = pd(m[4], m[8], m[5], m[7]); c[1] = pd(m[2], m[7], m[1], m[8]); c[2] = pd(m[1], m[5], m[2], m[4]);
    c[3] = pd(m[5], m[6], m[3], m[8]); c[4] = pd(m[0], m[8], m[2], m[6]); c[5] = pd(m[2], m[3], m[0], m[5]);
    c[6] = pd(m[3], m[7], m[4], m[6]); c[7] = pd(m[1], m[6], m[0], m[7]); c[8] = pd(m[0], m[4], m[1], m[3]);
    const double det = tr_rounded(m[0] * pd(m[4], m[8], m[5], m[7])) - tr_rounded(m[1] * pd(m[3], m[8], m[5], m[6])) +
                       tr_rounded(m[2] * pd(m[3], m[7], m[4], m[6]));
    if (det != 0) {
        const double inv = 1.0 / det;
#pragma unroll
        for (int i = 0; i < 9; i++) out[i] = c[i] * inv;
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) out[i] = 0.0;
    }
}

__global__ __launch_bounds__(PG_THREADS) void part_geometry_kernel(const double* __restrict__ keypoints, int M, int image_height, int pw, int ph,
                                                                   float x_pad, int shin_fallback, float* __restrict__ quads,
                                                                   double* __restrict__ fwd, double* __restrict__ back,
                                                                   double* __restrict__ fwd_inv, double* __restrict__ back_inv,
                                                                   float* __restrict__ m_inv, uint8_t* __restrict__ valid) {
    __shared__ double sys[72][PG_THREADS];              // element (r, k) of this thread's system at sys[r * 9 + k][tid]; k = 8 is the right side
    const int tid = threadIdx.x;
    const int64_t item = (int64_t)blockIdx.x * PG_THREADS + tid;
    if (item >= (int64_t)M * PG_PARTS * 2) return;      // no barrier below: every thread works on its own column of `sys`
    const int dir = (int)(item & 1);
    const int64_t pp = item >> 1;                       // person * 10 + part
    const int part = (int)(pp % PG_PARTS);
    const double* kp = keypoints + (pp / PG_PARTS) * 54;

    PgPoint quad[4];
    const bool ok = pg_quadrilateral(kp, part, image_height, x_pad, shin_fallback, quad);
    double h[9], hinv[9];
    if (ok) {
        const PgPoint corners[4] = {{0.f, 0.f}, {0.f, (float)ph}, {(float)pw, (float)ph}, {(float)pw, 0.f}};
#pragma unroll
        for (int i = 0; i < 4; i++) {                   // perspective_matrix's rows, float64 from the float32 points
            const double x = dir == 0 ? (double)quad[i].x : (double)corners[i].x, y = dir == 0 ? (double)quad[i].y : (double)corners[i].y;
            const double u = dir == 0 ? (double)corners[i].x : (double)quad[i].x, v = dir == 0 ? (double)corners[i].y : (double)quad[i].y;
            const double row_u[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u};
            const double row_v[9] = {0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v};
#pragma unroll
            for (int k = 0; k < 9; k++) { sys[i * 9 + k][tid] = row_u[k]; sys[(i + 4) * 9 + k][tid] = row_v[k]; }
        }
        bool singular = false;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (!singular) {
                int p = c;                              // the first row with the largest |a[r, c]|
                double best = fabs(sys[c * 9 + c][tid]);
#pragma unroll
                for (int r = c + 1; r < 8; r++) {
                    const double a = fabs(sys[r * 9 + c][tid]);
                    if (a > best) { best = a; p = r; }
                }
                if (best == 0.0) {
                    singular = true;
                } else {
#pragma unroll
                    for (int k = c; k < 9; k++) {       // swap the pivot row into place (p in c..7; p == c swaps a row with itself)
                        const double a = sys[p * 9 + k][tid], b = sys[c * 9 + k][tid];
                        sys[p * 9 + k][tid] = b;
                        sys[c * 9 + k][tid] = a;
                    }
                    const double piv = sys[c * 9 + c][tid];
#pragma unroll
                    for (int r = c + 1; r < 8; r++) {
                        const double m = sys[r * 9 + c][tid] / piv;
#pragma unroll
                        for (int k = c + 1; k < 9; k++) sys[r * 9 + k][tid] = sys[r * 9 + k][tid] - tr_rounded(m * sys[c * 9 + k][tid]);
                    }
                }
            }
        }
        if (singular) {
#pragma unroll
            for (int i = 0; i < 8; i++) h[i] = 0.0;
        } else {
#pragma unroll
            for (int r = 7; r >= 0; r--) {
                double s = sys[r * 9 + 8][tid];
#pragma unroll
                for (int k = r + 1; k < 8; k++) s = s - tr_rounded(sys[r * 9 + k][tid] * h[k]);
                h[r] = s / sys[r * 9 + r][tid];
            }
        }
        h[8] = 1.0;
        pg_inverse(h, hinv);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) { h[i] = 0.0; hinv[i] = 0.0; }
    }

    double* m_out = dir == 0 ? fwd : back;
    double* i_out = dir == 0 ? fwd_inv : back_inv;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        if (m_out) m_out[pp * 9 + i] = h[i];
        if (i_out) i_out[pp * 9 + i] = hinv[i];
    }
    if (dir == 0) {
        if (valid) valid[pp] = ok ? 1 : 0;
        if (quads) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                quads[pp * 8 + 2 * i] = ok ? quad[i].x : 0.f;
                quads[pp * 8 + 2 * i + 1] = ok ? quad[i].y : 0.f;
            }
        }
    } else if (m_inv) {
#pragma unroll
        for (int i = 0; i < 9; i++) m_inv[pp * 9 + i] = (float)h[i];      // zeros where invalid
    }
}

}  // namespace pasta

extern "C" int pasta_part_geometry(const double* keypoints, int M, int image_height, int patch_w, int patch_h, int x_pad, int shin_fallback,
                                   float* quads, double* fwd, double* back, double* fwd_inv, double* back_inv, float* m_inv, uint8_t* valid,
                                   void* stream) {
    using namespace pasta;
    PASTA_CHECK(keypoints, "part_geometry: null key points");
    PASTA_CHECK(M >= 1 && M <= (1 << 20), "part_geometry: %d people (1 .. 2^20)", M);
    PASTA_CHECK(image_height >= 1 && image_height <= 65536 && patch_w >= 1 && patch_w <= 65536 && patch_h >= 1 && patch_h <= 65536 &&
                x_pad >= 0 && x_pad <= 65536, "part_geometry: bad shape (height %d, patch %d x %d, x_pad %d)", image_height, patch_w, patch_h, x_pad);
    const int64_t items = (int64_t)M * PG_PARTS * 2;
    hipLaunchKernelGGL(part_geometry_kernel, dim3((unsigned)((items + PG_THREADS - 1) / PG_THREADS)), dim3(PG_THREADS), 0, (hipStream_t)stream,
                       keypoints, M, image_height, patch_w, patch_h, (float)x_pad, shin_fallback ? 1 : 0, quads, fwd, back, fwd_inv, back_inv,
                       m_inv, valid);
    return launch_status("part_geometry");
}
