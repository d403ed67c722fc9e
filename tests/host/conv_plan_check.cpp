// Stand-alone check of the convolution planner's lattice builders and forward workspace layout (pasta-gan_amd/csrc/conv_plan.h) against
// their definitions, by brute force.  Plain C++: built and run by tests/test_conv_plan_table_cpu.py with the host compiler and
// -fsanitize=address,undefined.  Exits non-zero on the first violation.
//
//   conv_plan_check [descriptors.txt]      lines of N C_in H W C_out OH OW kh kw stride pad_h pad_w groups transposed flip math io_dtype x2 C1
//                                          x_layout, then the bytes pasta_conv2d_workspace recorded for the descriptor
//
// Lattices: stride 1 - 4, kernels 1 - 7 in either direction, pads 0 - 3 (equal and unequal), planes that give output sizes 1, u - 1, u, 2H and 2H + 1.  For
// conv2d, for the parity classes of conv_transpose2d one table each and all in one, and for the remainder classes of the pair launch:
//   * every (class, lattice point, table tap) whose input pixel lies inside the plane satisfies oy = iy u - pad + r, ox = ix u - pad + c with
//     (r, c) read from tap_slab (conv2d: iy = oy u - pad + r);
//   * every (output pixel, weight tap, in-plane input pixel) triple of the definition is produced exactly once, and nothing else is.
// detect_tap_rows: exactly the 3-wide stride-1 tables form rows, ascending for conv2d, descending for conv_transpose2d.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../pasta-gan_amd/csrc/conv_plan.h"

namespace pasta {
static char g_error[512];
char* error_buffer() { return g_error; }
int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return 1;
}
}  // namespace pasta

using namespace pasta;

static const pasta_conv_desc* g_desc;
static const char* g_what;

#define REQUIRE(cond)                                                                                                                     \
    do {                                                                                                                                  \
        if (!(cond)) {                                                                                                                    \
            const pasta_conv_desc* d_ = g_desc;                                                                                           \
            fprintf(stderr, "%s:%d: %s: !(%s)\n  N %d C_in %d %dx%d -> C_out %d %dx%d, k %dx%d stride %d pad %d,%d groups %d transposed %d math %d io %d\n", \
                    __FILE__, __LINE__, g_what, #cond, d_->N, d_->C_in, d_->H, d_->W, d_->C_out, d_->OH, d_->OW, d_->kh, d_->kw, d_->stride,         \
                    d_->pad_h, d_->pad_w, d_->groups, d_->transposed, d_->math, d_->io_dtype);                                            \
            exit(1);                                                                                                                      \
        }                                                                                                                                 \
    } while (0)

// produced[((oy OW + ox) kh + r) kw + c]: how often the tables multiplied weight tap (r, c) into output pixel (oy, ox) from inside the plane
struct Produced {
    const pasta_conv_desc* d;
    std::vector<int> n, covered;
    explicit Produced(const pasta_conv_desc* d_) : d(d_), n((size_t)d_->OH * d_->OW * d_->kh * d_->kw, 0), covered((size_t)d_->OH * d_->OW, 0) {}

    // walk a table: the first property, and the counts for the second
    void take(const TapTable& t) {
        const int u = d->stride;
        for (int c = 0; c < t.ncls; c++) {
            const TapTable::Lattice& l = t.cls[c];
            REQUIRE(l.tap0 >= 0 && l.T >= 0 && l.tap0 + l.T <= MAX_TAPS);
            for (int p = 0; p < l.P; p++)
                for (int q = 0; q < l.Q; q++) {
                    const int oy = l.oy0 + p * t.osy, ox = l.ox0 + q * t.osx;
                    REQUIRE(oy >= 0 && oy < d->OH && ox >= 0 && ox < d->OW);
                    covered[(size_t)oy * d->OW + ox]++;
                    for (int k = l.tap0; k < l.tap0 + l.T; k++) {
                        const int iy = p * t.isy + t.tap_dy[k], ix = q * t.isx + t.tap_dx[k];
                        if (iy < 0 || iy >= d->H || ix < 0 || ix >= d->W) continue;
                        REQUIRE(t.tap_slab[k] >= 0 && t.tap_slab[k] < d->kh * d->kw);
                        const int r = t.tap_slab[k] / d->kw, cc = t.tap_slab[k] % d->kw;
                        if (d->transposed) REQUIRE(oy == iy * u - d->pad_h + r && ox == ix * u - d->pad_w + cc);
                        else REQUIRE(iy == oy * u - d->pad_h + r && ix == ox * u - d->pad_w + cc);
                        n[(((size_t)oy * d->OW + ox) * d->kh + r) * d->kw + cc]++;
                    }
                }
        }
    }

    // does the definition have an in-plane input pixel for (oy, ox, r, c)?
    bool defined(int oy, int ox, int r, int c) const {
        const int u = d->stride;
        if (!d->transposed) {
            const int iy = oy * u - d->pad_h + r, ix = ox * u - d->pad_w + c;
            return iy >= 0 && iy < d->H && ix >= 0 && ix < d->W;
        }
        const int ny = oy + d->pad_h - r, nx = ox + d->pad_w - c;
        return ny >= 0 && nx >= 0 && ny % u == 0 && nx % u == 0 && ny / u < d->H && nx / u < d->W;
    }

    // the second property over the output pixels `in` selects: each exactly once, every other pixel never
    template <class In>
    void complete(In in) const {
        for (int oy = 0; oy < d->OH; oy++)
            for (int ox = 0; ox < d->OW; ox++) {
                REQUIRE(covered[(size_t)oy * d->OW + ox] == (in(oy, ox) ? 1 : 0));
                for (int r = 0; r < d->kh; r++)
                    for (int c = 0; c < d->kw; c++)
                        REQUIRE(n[(((size_t)oy * d->OW + ox) * d->kh + r) * d->kw + c] == (in(oy, ox) && defined(oy, ox, r, c) ? 1 : 0));
            }
    }
};

// is there an output parity class that no tap reaches?
static bool has_empty_class(const pasta_conv_desc* d) {
    const int u = d->stride;
    for (int a = 0; a < u && a < d->OH; a++)
        for (int b = 0; b < u && b < d->OW; b++) {
            int taps = 0;
            for (int r = 0; r < d->kh; r++)
                for (int c = 0; c < d->kw; c++) taps += (a + d->pad_h - r) % u == 0 && (b + d->pad_w - c) % u == 0;
            if (!taps) return true;
        }
    return false;
}

static long check_lattices() {
    long checked = 0;
    static const int planes[][2] = {{1, 1}, {2, 3}, {5, 4}};
    for (int transposed = 0; transposed < 2; transposed++)
    for (int u = 1; u <= 4; u++)
    for (int kh = 1; kh <= 7; kh++)
    for (int kw = 1; kw <= 7; kw++)
    for (int pad = 0; pad <= 3; pad++)
    for (int pad_w = pad; pad_w >= 0; pad_w = pad_w == pad ? 3 - pad : -1)          // equal pads, and unequal ones
    for (const auto& hw : planes)
    for (int op = 0; op < (transposed ? u : 1); op++) {
        pasta_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.N = 1; d.C_in = 16; d.C_out = 16; d.groups = 1; d.H = hw[0]; d.W = hw[1]; d.kh = kh; d.kw = kw; d.stride = u; d.pad_h = pad; d.pad_w = pad_w;
        d.transposed = transposed; d.math = PASTA_MATH_DEFAULT; d.io_dtype = PASTA_F32;
        if (transposed) { d.OH = (d.H - 1) * u - 2 * pad + kh + op; d.OW = (d.W - 1) * u - 2 * pad_w + kw + op; }
        else { d.OH = (d.H + 2 * pad - kh) / u + 1; d.OW = (d.W + 2 * pad_w - kw) / u + 1; }
        if ((!transposed && (d.H + 2 * pad < kh || d.W + 2 * pad_w < kw)) || check_desc(&d, "check")) continue;      // no such convolution
        g_desc = &d;
        const auto all = [](int, int) { return true; };
        TapTable t;
        if (!transposed) {
            g_what = "conv2d lattice";
            lattice_conv2d(&d, false, t);
            REQUIRE(t.ncls == 1 && t.cls[0].T == kh * kw);
            Produced pr(&d);
            pr.take(t);
            pr.complete(all);
            g_what = "detect_tap_rows, conv2d";
            REQUIRE(t.rows == (u == 1 && kw == 3 ? 1 : 0));
            if (t.rows) REQUIRE(t.rows_rev == 0 && t.rows_d0 == -pad_w);
            checked++;
            continue;
        }
        g_what = "conv_transpose2d, all classes in one table";
        const int nclasses = (u < d.OH ? u : d.OH) * (u < d.OW ? u : d.OW);
        const bool empty = has_empty_class(&d);
        if (nclasses <= 4) {       // (the launch merges the classes of stride 2 only; the table holds four)
            REQUIRE((lattice_transposed(&d, -1, t) != 0) == empty);
            if (!empty) {
                REQUIRE(t.ncls == nclasses);
                Produced pr(&d);
                pr.take(t);
                pr.complete(all);
            }
        }
        g_what = "conv_transpose2d, one table per class";
        Produced pr(&d);
        bool refused = false;
        for (int k = 0; k < nclasses && !refused; k++) {
            refused = lattice_transposed(&d, k, t) != 0;
            if (refused) break;
            REQUIRE(t.ncls == 1 && t.cls[0].tap0 == 0);
            pr.take(t);
            if (u == 1) {
                g_what = "detect_tap_rows, conv_transpose2d";
                REQUIRE(t.rows == (kw == 3 ? 1 : 0));
                if (t.rows) REQUIRE(t.rows_rev == 1 && t.rows_d0 == pad_w - 2);
            } else REQUIRE(t.rows == 0);
        }
        REQUIRE(refused == empty);
        if (!refused) pr.complete(all);
        if (u == 2 && kh == 3 && kw == 3 && pad <= 1 && pad_w == pad && doubled_plane(&d)) {
            g_what = "remainder classes of the pair launch";
            lattice_pair_remainder(&d, t);
            REQUIRE(t.ncls == 2 * ((d.OH == 2 * d.H + 1) + (d.OW == 2 * d.W + 1)));
            Produced rem(&d);
            rem.take(t);
            rem.complete([&](int oy, int ox) { return oy == 2 * d.H || ox == 2 * d.W; });
        }
        checked++;
    }
    return checked;
}

// the regions of the forward workspace: ascending, 16-byte aligned, each as large as what is written into it, the total as recorded
static long check_workspaces(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
    long checked = 0;
    int v[20];
    long long bytes;
    for (;;) {
        int got = 0;
        for (int i = 0; i < 20; i++) got += fscanf(f, "%d", &v[i]) == 1;
        if (got != 20 || fscanf(f, "%lld", &bytes) != 1) break;
        pasta_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.N = v[0]; d.C_in = v[1]; d.H = v[2]; d.W = v[3]; d.C_out = v[4]; d.OH = v[5]; d.OW = v[6]; d.kh = v[7]; d.kw = v[8]; d.stride = v[9];
        d.pad_h = v[10]; d.pad_w = v[11]; d.groups = v[12]; d.transposed = v[13]; d.flip = v[14]; d.math = v[15]; d.io_dtype = v[16];
        d.x2 = v[17] ? (const void*)&d : nullptr; d.C1 = v[18]; d.x_layout = v[19];
        g_desc = &d;
        g_what = "fwd_workspace";
        FwdWorkspace ws;
        if (check_desc(&d, "check")) { REQUIRE(bytes == -1); continue; }
        const FwdPlan p = plan_fwd(&d);
        REQUIRE(fwd_workspace(&d, p, ws) == 0);
        REQUIRE(ws.total_floats * 4 == bytes);
        REQUIRE(ws.rowinv == WS_AMAX_FLOATS && ws.rowinv < ws.pack && ws.pack < ws.partial && ws.partial <= ws.koff && ws.koff <= ws.extra && ws.extra <= ws.total_floats);
        REQUIRE(ws.rowinv % 4 == 0 && ws.pack % 4 == 0 && ws.partial % 4 == 0 && ws.koff % 4 == 0 && ws.extra % 4 == 0 && ws.total_floats % 4 == 0);
        // what the launch writes into each region
        const int Ig = d.C_in / d.groups, Og_pad = round_up(d.C_out / d.groups, fwd_tile_bm(p.tile));
        const int Kpad = round_up(Ig * d.kh * d.kw, 16);
        REQUIRE(ws.pack - ws.rowinv >= (int64_t)d.groups * Og_pad);
        // (six bytes per element: three bf16 pieces, or two fp16 pieces and fp32 weights in less)
        REQUIRE((ws.partial - ws.pack) * 4 >= (int64_t)d.groups * d.kh * d.kw * round_up(Ig, fwd_ipad(Ig, p.tile)) * Og_pad * 6);
        if (p.packed) REQUIRE((ws.partial - ws.pack) * 4 >= (int64_t)Kpad * Og_pad * 6);
        REQUIRE(ws.koff - ws.partial >= (p.ksplit > 1 ? (int64_t)p.ksplit * d.N * d.C_out * d.OH * d.OW : 0));
        REQUIRE(ws.extra - ws.koff >= (p.packed ? Kpad : 0));
        int64_t extra = 0;
        if (p.packed && (d.pad_h || d.pad_w)) extra = (int64_t)d.N * d.C_in * (d.H + 2 * d.pad_h) * (d.W + 2 * d.pad_w);
        if (t2_shape_ok(&d, math_pieces(d.math), p.ksplit)) { REQUIRE(!p.packed && p.ksplit == 1); extra = (int64_t)d.N * d.C_in * d.H; }
        REQUIRE(ws.total_floats - ws.extra >= extra);
        checked++;
    }
    fclose(f);
    return checked;
}

int main(int argc, char** argv) {
    const long lattices = check_lattices();
    const long workspaces = argc > 1 ? check_workspaces(argv[1]) : 0;
    printf("conv_plan_check: %ld lattice configurations, %ld workspaces\n", lattices, workspaces);
    return lattices > 1000 && (argc == 1 || workspaces > 0) ? 0 : 1;
}
