// PNG files of a batch of RGB8 images, encoded where the pixels are (torch_utils/ops/png_encode.py).
//   pasta_png_filter           Paeth-filters every row from the ORIGINAL pixels, counts each segment's tokens and sums its
//                              Adler-32 parts: one workgroup per (image, segment of PASTA_PNG_ROWS rows);
//   pasta_png_code_lengths     HOST ONLY: length-limited, COMPLETE Huffman code lengths of a histogram;
//   pasta_png_segment_tables   HOST ONLY: every segment's code table, dynamic-Huffman block header and byte size;
//   pasta_png_encode           writes every segment's bits at its final place in a compact, zeroed buffer.
// The stream: a segment is one dynamic-Huffman deflate block followed by an empty stored block, so it begins and ends on a byte
// boundary and segments are independent.  Its bytes are taken in tiles of 32 from its start; a full tile of zeros whose
// preceding byte in the image's filtered stream exists and is zero is ONE match (length 32, distance 1), every other byte a
// literal.  Nothing here depends on the order in which threads run: two calls give the same bytes.
#include <algorithm>
#include <string.h>

#include "common.h"

namespace pasta {

constexpr int PNG_ROWS = PASTA_PNG_ROWS, PNG_TILE = 32, PNG_SYMS = PASTA_PNG_SYMS;
constexpr int PNG_META = PASTA_PNG_META_WORDS, PNG_TABLE = PASTA_PNG_TABLE_WORDS;
constexpr int PNG_HDR_AT = PNG_SYMS + 2;                    // table words 0..285 symbols, 286 header bits, 287 zero, 288.. header
constexpr int PNG_HDR_WORDS = PNG_TABLE - PNG_HDR_AT;       // 66 words: 17 + 19 * 3 + 287 * 7 = 2083 bits at the most
constexpr int PNG_MATCH = 272;                              // lengths 31..34, two extra bits: value 1 is length 32
constexpr int PNG_NT = 256;
constexpr int PNG_MAX_SIDE = 8192;
static_assert(PNG_HDR_WORDS * 32 >= 17 + 19 * 3 + (PNG_SYMS + 1) * 7, "header words");

// Byte `col` of filtered row `row` (col 0 is the filter type, 4): Paeth with bpp 3, left / up / upper-left from the original pixels,
// zero outside the image.  p - a = b - c, p - b = a - c, p - c = a + b - 2 c.
__device__ __forceinline__ int png_filtered_byte(const uint8_t* __restrict__ img, int W3, int row, int col) {
    if (col == 0) return 4;
    const int k = col - 1;
    const uint8_t* p = img + (int64_t)row * W3 + k;
    const int x = p[0];
    const int a = k >= 3 ? p[-3] : 0;
    const int b = row > 0 ? p[-W3] : 0;
    const int c = (k >= 3 && row > 0) ? p[-W3 - 3] : 0;
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return (x - pred) & 255;
}

__device__ __forceinline__ uint64_t png_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// One workgroup: one segment of one image.  Thread t takes bytes t, t + 256, ... of the segment, so a tile of 32 is half a wave
// and "all zero, and a zero before it" is one ballot; the lane at the head of a tile computes the byte before the tile itself
// (it may belong to the segment above).  Histograms are kept per wave in LDS and stored once.
__global__ __launch_bounds__(PNG_NT) void png_filter_kernel(const uint8_t* __restrict__ images, uint8_t* __restrict__ filtered,
                                                            uint32_t* __restrict__ meta, int H, int W, int S) {
    __shared__ uint32_t hist[PNG_NT / 64][PNG_META];
    __shared__ uint64_t red[PNG_NT / 64][2];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int seg = blockIdx.x, n = blockIdx.y;
    const int W3 = 3 * W, stride = W3 + 1;
    const int r0 = seg * PNG_ROWS, rows = min(PNG_ROWS, H - r0);
    const int len = rows * stride;
    const int64_t seg_pos = (int64_t)r0 * stride;                   // of the segment's first byte in the image's filtered stream
    const uint8_t* img = images + (int64_t)n * H * W3;
    uint8_t* out = filtered + (int64_t)n * H * stride + seg_pos;
    for (int i = t; i < (PNG_NT / 64) * PNG_META; i += PNG_NT) (&hist[0][0])[i] = 0;
    __syncthreads();

    uint64_t s1 = 0, s2 = 0;
    for (int base = 0; base < len; base += PNG_NT) {
        const int i = base + t;
        const bool in = i < len;
        int d = 0;
        bool run = false;                                           // this byte does not stand against its tile being a match
        if (in) {
            const int r = i / stride, c = i - r * stride;
            d = png_filtered_byte(img, W3, r0 + r, c);
            out[i] = (uint8_t)d;
            s1 += (uint64_t)d;
            s2 += (uint64_t)(len - i) * (uint64_t)d;
            run = d == 0;
            if (run && (lane & 31) == 0) {
                const int64_t before = seg_pos + i - 1;
                if (before < 0) run = false;
                else {
                    const int rb = (int)(before / stride), cb = (int)(before - (int64_t)rb * stride);
                    run = png_filtered_byte(img, W3, rb, cb) == 0;
                }
            }
        }
        const uint64_t ballot = __ballot(run);
        const bool match = (uint32_t)(lane < 32 ? ballot : ballot >> 32) == 0xffffffffu;       // 32 bytes in the segment: a full tile
        if (match) {
            if ((lane & 31) == 0) atomicAdd(&hist[wave][PNG_MATCH], 1u);
        } else if (in) {
            atomicAdd(&hist[wave][d], 1u);
        }
    }
    s1 = png_wave_sum(s1);
    s2 = png_wave_sum(s2);
    if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
    __syncthreads();
    uint32_t* m = meta + ((int64_t)n * S + seg) * PNG_META;
    for (int s = t; s < PNG_SYMS; s += PNG_NT) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < PNG_NT / 64; w++) v += hist[w][s];
        m[s] = s == 256 ? 1u : v;                                   // the block's one end-of-block symbol
    }
    if (t < 2) {
        uint64_t v = 0;
#pragma unroll
        for (int w = 0; w < PNG_NT / 64; w++) v += red[w][t];
        m[PNG_SYMS + t] = (uint32_t)(v % 65521u);
    }
}

// OR up to 32 bits into the zeroed output at bit `pos`; a zero part is not sent, so nothing is touched past the last bit set.
__device__ __forceinline__ void png_or_bits(uint32_t* out, int64_t out_words, uint64_t pos, uint32_t v) {
    const int64_t word = (int64_t)(pos >> 5);
    const int sh = (int)(pos & 31);
    const uint32_t lo = v << sh, hi = sh ? v >> (32 - sh) : 0u;
    if (lo && word < out_words) atomicOr(out + word, lo);
    if (hi && word + 1 < out_words) atomicOr(out + word + 1, hi);
}

// A thread's bits, appended at an absolute bit position: words the thread fills whole are plain stores, the word it shares with
// the thread before it and the one it leaves unfinished are OR-ed into the zeroed buffer.
struct PngBits {
    uint32_t* out;
    int64_t out_words, word;
    uint64_t acc;
    int nb;
    bool shared;
    __device__ __forceinline__ PngBits(uint32_t* o, int64_t words, uint64_t pos)
        : out(o), out_words(words), word((int64_t)(pos >> 5)), acc(0), nb((int)(pos & 31)), shared((pos & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t entry) {           // a table word: bits | count << 24
        acc |= (uint64_t)(entry & 0xffffffu) << nb;
        nb += (int)(entry >> 24);
        if (nb >= 32) {
            if (word < out_words) {
                if (shared) atomicOr(out + word, (uint32_t)acc);
                else out[word] = (uint32_t)acc;
            }
            shared = false;
            word++;
            acc >>= 32;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if ((uint32_t)acc && word < out_words) atomicOr(out + word, (uint32_t)acc);
    }
};

// One workgroup: one segment of one image; one tile of 32 bytes per thread and 256 tiles per round.  A round stages its 8 KB in
// LDS (tile t at word 9 t: an odd stride, so the threads' word reads fall on different banks), every thread counts its tile's
// bits, a workgroup scan places it, and it writes them.  The running bit offset carries over the rounds of a long segment.
__global__ __launch_bounds__(PNG_NT) void png_encode_kernel(const uint8_t* __restrict__ filtered, const uint32_t* __restrict__ tables,
                                                            const int64_t* __restrict__ offsets, uint32_t* __restrict__ out,
                                                            int64_t out_words, int H, int W, int S) {
    __shared__ uint32_t table[PNG_HDR_AT];
    __shared__ uint32_t stage[PNG_NT * 9];
    __shared__ uint32_t wave_bits[PNG_NT / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int seg = blockIdx.x, n = blockIdx.y;
    const int stride = 3 * W + 1;
    const int r0 = seg * PNG_ROWS, rows = min(PNG_ROWS, H - r0);
    const int len = rows * stride;
    const int64_t seg_pos = (int64_t)r0 * stride;
    const uint8_t* src = filtered + (int64_t)n * H * stride + seg_pos;
    const uint32_t* tab = tables + ((int64_t)n * S + seg) * PNG_TABLE;
    const uint64_t bit0 = (uint64_t)offsets[(int64_t)n * S + seg] * 8u;
    for (int i = t; i < PNG_HDR_AT; i += PNG_NT) table[i] = tab[i];
    const uint32_t header_bits = min(tab[PNG_SYMS], (uint32_t)(PNG_HDR_WORDS * 32));
    if (t < PNG_HDR_WORDS && (uint32_t)t * 32u < header_bits) png_or_bits(out, out_words, bit0 + 32u * t, tab[PNG_HDR_AT + t]);

    const int ntiles = (len + PNG_TILE - 1) / PNG_TILE;
    uint32_t carry = header_bits;                                   // bits of the segment before this round
    for (int tile0 = 0; tile0 < ntiles; tile0 += PNG_NT) {
        __syncthreads();
        const int round_base = tile0 * PNG_TILE, round_bytes = min(PNG_NT * PNG_TILE, len - round_base);
        uint8_t* sb = (uint8_t*)stage;
        for (int j = t; j < round_bytes; j += PNG_NT) sb[(j >> 5) * 36 + (j & 31)] = src[round_base + j];
        __syncthreads();
        const int tile = tile0 + t;
        const int cnt = tile < ntiles ? min(PNG_TILE, len - tile * PNG_TILE) : 0;
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = stage[t * 9 + k];
        bool match = false;
        if (cnt == PNG_TILE && (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0u && seg_pos + (int64_t)tile * PNG_TILE > 0)
            match = src[(int64_t)tile * PNG_TILE - 1] == 0;
        const bool closes = tile == ntiles - 1;
        uint32_t bits = 0;
        if (match) bits = table[PNG_MATCH] >> 24;
        else {
#pragma unroll
            for (int k = 0; k < PNG_TILE; k++)
                if (k < cnt) bits += table[(w[k >> 2] >> (8 * (k & 3))) & 255u] >> 24;
        }
        if (closes) bits += table[256] >> 24;

        uint32_t inc = bits;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) wave_bits[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < PNG_NT / 64; k++) {
            before += k < wave ? wave_bits[k] : 0u;
            total += wave_bits[k];
        }
        if (cnt > 0) {
            PngBits bw(out, out_words, bit0 + carry + before + inc - bits);
            if (match) bw.put(table[PNG_MATCH]);
            else {
#pragma unroll
                for (int k = 0; k < PNG_TILE; k++)
                    if (k < cnt) bw.put(table[(w[k >> 2] >> (8 * (k & 3))) & 255u]);
            }
            if (closes) bw.put(table[256]);
            bw.finish();
        }
        carry += total;
    }
    // the empty stored block: BFINAL on the image's last segment, BTYPE 00, zeros to the byte boundary, LEN 0000, NLEN FFFF
    if (t == 0) {
        if (seg == S - 1) png_or_bits(out, out_words, bit0 + carry, 1u);
        const uint64_t stored = (bit0 + carry + 3u + 7u) >> 3;      // the byte LEN starts at
        png_or_bits(out, out_words, (stored + 2u) * 8u, 0xffffu);
    }
}

// ---- host side ----

// Length-limited Huffman code lengths.  The unlimited code comes from the two-queue construction over the used symbols sorted by
// (count, symbol); depths beyond `limit` are cut to it, which over-subscribes the code by a whole number of 2^-limit, and each
// repair step takes exactly one unit back: a leaf at the deepest level below the limit becomes an inner node whose children are
// that leaf and one taken from the limit level.  The loop therefore ends on a Kraft sum of exactly 1 -- a COMPLETE code, which
// inflate demands of the literal/length and the code-length alphabets -- and the lengths go to the symbols by count, the
// shortest to the most frequent.
static int png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths) {
    struct Leaf { uint64_t w; int s; };
    Leaf leaf[PNG_META];
    uint64_t weight[2 * PNG_META];
    int parent[2 * PNG_META], depth[2 * PNG_META];
    int used = 0;
    for (int s = 0; s < n; s++) {
        lengths[s] = 0;
        if (counts[s]) leaf[used++] = Leaf{counts[s], s};
    }
    PASTA_CHECK(used >= 1, "png_code_lengths: every one of the %d counts is zero", n);
    if (used == 1) { lengths[leaf[0].s] = 1; return 0; }           // a lone symbol: one bit, the only incomplete code there is
    PASTA_CHECK(used <= (1 << limit), "png_code_lengths: %d symbols do not fit codes of at most %d bits", used, limit);
    std::sort(leaf, leaf + used, [](const Leaf& a, const Leaf& b) { return a.w != b.w ? a.w < b.w : a.s < b.s; });
    for (int i = 0; i < used; i++) weight[i] = leaf[i].w;
    int next_leaf = 0, next_inner = used, made = used;
    auto take = [&]() {
        if (next_leaf < used && (next_inner >= made || weight[next_leaf] <= weight[next_inner])) return next_leaf++;
        return next_inner++;
    };
    for (; made < 2 * used - 1; made++) {
        const int a = take(), b = take();
        weight[made] = weight[a] + weight[b];
        parent[a] = parent[b] = made;
    }
    int num[16] = {0};
    depth[2 * used - 2] = 0;
    for (int i = 2 * used - 3; i >= 0; i--) {
        depth[i] = depth[parent[i]] + 1;
        if (i < used) num[std::min(depth[i], limit)]++;
    }
    int64_t total = 0;
    for (int l = 1; l <= limit; l++) total += (int64_t)num[l] << (limit - l);
    while (total > ((int64_t)1 << limit)) {
        int i = limit - 1;
        while (i >= 1 && num[i] == 0) i--;
        PASTA_CHECK(i >= 1 && num[limit] >= 1, "png_code_lengths: cannot repair the code (limit %d, %d symbols)", limit, used);
        num[limit]--;
        num[i]--;
        num[i + 1] += 2;
        total--;
    }
    PASTA_CHECK(total == ((int64_t)1 << limit), "png_code_lengths: incomplete code (limit %d, %d symbols)", limit, used);
    int at = 0;                                                     // the rarest symbols take the longest codes
    for (int l = limit; l >= 1; l--)
        for (int k = 0; k < num[l]; k++) lengths[leaf[at++].s] = (uint8_t)l;
    return 0;
}

// Canonical codes (RFC 1951 3.2.2) of `lengths`, bit-reversed: deflate sends a Huffman code from its most significant bit.
static void png_canonical(const uint8_t* lengths, int n, uint32_t* codes) {
    int count[16] = {0}, next[16] = {0};
    for (int s = 0; s < n; s++) count[lengths[s]]++;
    count[0] = 0;
    for (int b = 1, code = 0; b < 16; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (int s = 0; s < n; s++) {
        uint32_t c = lengths[s] ? (uint32_t)next[lengths[s]]++ : 0u, r = 0;
        for (int b = 0; b < lengths[s]; b++) r |= ((c >> b) & 1u) << (lengths[s] - 1 - b);
        codes[s] = r;
    }
}

struct PngHeaderBits {
    uint32_t* words;
    uint32_t bits;
    void put(uint32_t v, int n) {
        for (int b = 0; b < n; b++, bits++)
            if ((v >> b) & 1u) words[bits >> 5] |= 1u << (bits & 31);
    }
};

static const int PNG_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// One segment: the table the encode kernel reads and the segment's size in bytes.
static int png_segment_table(const uint32_t* hist, uint32_t* table, int64_t* bytes) {
    uint8_t ll[PNG_SYMS + 1], cl[19];
    uint32_t lc[PNG_SYMS], cc[19], clf[19] = {0};
    PASTA_CHECK(hist[256] == 1, "png_segment_tables: a segment counts %u end-of-block symbols, not 1", hist[256]);
    if (int e = png_code_lengths(hist, PNG_SYMS, 15, ll)) return e;
    png_canonical(ll, PNG_SYMS, lc);
    ll[PNG_SYMS] = hist[PNG_MATCH] ? 1 : 0;                         // HDIST = 0: the one distance code, absent without a match
    for (int s = 0; s <= PNG_SYMS; s++) clf[ll[s]]++;
    if (int e = png_code_lengths(clf, 19, 7, cl)) return e;
    png_canonical(cl, 19, cc);
    int hclen = 4;
    for (int i = 0; i < 19; i++)
        if (cl[PNG_CL_ORDER[i]]) hclen = std::max(hclen, i + 1);
    memset(table, 0, sizeof(uint32_t) * PNG_TABLE);
    PngHeaderBits h{table + PNG_HDR_AT, 0};
    h.put(0, 1);                                                    // BFINAL travels on the stored block that closes the segment
    h.put(2, 2);                                                    // BTYPE 10
    h.put(PNG_SYMS - 257, 5);
    h.put(0, 5);
    h.put((uint32_t)hclen - 4, 4);
    for (int i = 0; i < hclen; i++) h.put(cl[PNG_CL_ORDER[i]], 3);
    for (int s = 0; s <= PNG_SYMS; s++) h.put(cc[ll[s]], cl[ll[s]]);   // plain lengths, no run symbols
    int64_t bits = h.bits;
    for (int s = 0; s < PNG_SYMS; s++) {
        table[s] = lc[s] | (uint32_t)ll[s] << 24;
        bits += (int64_t)hist[s] * ll[s];
    }
    if (hist[PNG_MATCH]) {                                          // the whole match: code, extra bits 01 (length 32), distance code 0
        table[PNG_MATCH] = lc[PNG_MATCH] | 1u << ll[PNG_MATCH] | (uint32_t)(ll[PNG_MATCH] + 3) << 24;
        bits += (int64_t)hist[PNG_MATCH] * 3;
    }
    table[PNG_SYMS] = h.bits;
    *bytes = (bits + 3 + 7) / 8 + 4;
    return 0;
}

static int png_check_shape(const char* what, int N, int H, int W, int C) {
    PASTA_CHECK(C == 3, "%s: %d channels; only RGB (3) is encoded", what, C);
    PASTA_CHECK(N >= 1 && N <= 65535, "%s: batch of %d images (1 .. 65535)", what, N);
    PASTA_CHECK(H >= 1 && H <= PNG_MAX_SIDE, "%s: height %d (1 .. %d)", what, H, PNG_MAX_SIDE);
    PASTA_CHECK(W >= 1 && W <= PNG_MAX_SIDE, "%s: width %d (1 .. %d)", what, W, PNG_MAX_SIDE);
    PASTA_CHECK((int64_t)H * (3 * (int64_t)W + 1) < ((int64_t)1 << 31), "%s: a filtered stream of %lld bytes per image (below 2^31)", what,
                (long long)((int64_t)H * (3 * (int64_t)W + 1)));
    return 0;
}

}  // namespace pasta

extern "C" int pasta_png_filter(const uint8_t* images, uint8_t* filtered, uint32_t* meta, int N, int H, int W, int C, void* stream) {
    using namespace pasta;
    if (int e = png_check_shape("png_filter", N, H, W, C)) return e;
    PASTA_CHECK(images && filtered && meta, "png_filter: null pointer");
    const int S = (H + PNG_ROWS - 1) / PNG_ROWS;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)S, (unsigned)N), dim3(PNG_NT), 0, (hipStream_t)stream, images, filtered, meta, H, W, S);
    return launch_status("png_filter");
}

extern "C" int pasta_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths) {
    using namespace pasta;
    PASTA_CHECK(counts && lengths, "png_code_lengths: null pointer");
    PASTA_CHECK(n >= 1 && n <= PNG_META, "png_code_lengths: %d symbols (1 .. %d)", n, PNG_META);
    PASTA_CHECK(limit >= 1 && limit <= 15, "png_code_lengths: limit of %d bits (1 .. 15)", limit);
    return png_code_lengths(counts, n, limit, lengths);
}

extern "C" int pasta_png_segment_tables(const uint32_t* meta, int64_t segments, uint32_t* tables, int64_t* seg_bytes) {
    using namespace pasta;
    PASTA_CHECK(meta && tables && seg_bytes, "png_segment_tables: null pointer");
    PASTA_CHECK(segments >= 1, "png_segment_tables: %lld segments", (long long)segments);
    for (int64_t i = 0; i < segments; i++)
        if (int e = png_segment_table(meta + i * PNG_META, tables + i * PNG_TABLE, seg_bytes + i)) return e;
    return 0;
}

extern "C" int pasta_png_encode(const uint8_t* filtered, const uint32_t* tables, const int64_t* offsets, uint8_t* out, int64_t out_bytes,
                                int N, int H, int W, void* stream) {
    using namespace pasta;
    if (int e = png_check_shape("png_encode", N, H, W, 3)) return e;
    PASTA_CHECK(filtered && tables && offsets && out, "png_encode: null pointer");
    PASTA_CHECK(out_bytes >= 4 && out_bytes % 4 == 0 && (uintptr_t)out % 4 == 0,
                "png_encode: the output is %lld bytes at %p; it is written in whole aligned 32-bit words", (long long)out_bytes, (void*)out);
    const int S = (H + PNG_ROWS - 1) / PNG_ROWS;
    hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)S, (unsigned)N), dim3(PNG_NT), 0, (hipStream_t)stream, filtered, tables, offsets,
                       (uint32_t*)out, out_bytes / 4, H, W, S);
    return launch_status("png_encode");
}
