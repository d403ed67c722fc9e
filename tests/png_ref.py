"""numpy restatement of the PNG stream csrc/png_encode.hip writes (include/pasta_hip.h lists the rules): Paeth filter
from the original pixels, segments of ROWS rows, tiles of 32 bytes that are one match when all zero behind a zero, tables from
GIVEN code lengths, bit packing, the stored block that closes a segment, the Adler-32 combination and the chunk framing.

The code lengths are not restated: ``code_lengths(counts, limit) -> lengths`` is passed in (the host-only entry
pasta_png_code_lengths, which tests/test_png_cpu.py holds to its own conditions).  Everything else here is independent of the
library, and ``zlib`` and PIL are the judges of whether the result is a PNG."""

import struct
import zlib

import numpy as np

ROWS, TILE, SYMS, MATCH = 16, 32, 286, 272
META_WORDS, TABLE_WORDS, HEADER_AT = 288, 354, 288
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
SIGNATURE = b'\x89PNG\r\n\x1a\n'


def filtered(img):
    """[H, W, 3] uint8 -> [H, 1 + 3 W] uint8: filter type 4 on every row, predictors from the original pixels."""
    h, w, _ = img.shape
    x = img.reshape(h, w * 3).astype(np.int32)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty([h, 1 + 3 * w], np.uint8)
    out[:, 0] = 4
    out[:, 1:] = (x - pred) & 255
    return out


def tiles(stream, start, n):
    """The tokens of the segment stream[start : start + n]: (full [T, 32] tiles, match [T] bool, the ragged rest)."""
    data = stream[start:start + n]
    full = data[:n // TILE * TILE].reshape(-1, TILE)
    heads = start + TILE * np.arange(len(full))
    before_is_zero = np.array([p > 0 and stream[p - 1] == 0 for p in heads], bool)
    match = (full.max(axis=1, initial=0) == 0) & before_is_zero
    return full, match, data[len(full) * TILE:]


def histogram(stream, start, n):
    full, match, rest = tiles(stream, start, n)
    counts = np.bincount(np.concatenate([full[~match].reshape(-1), rest]), minlength=SYMS).astype(np.uint32)
    counts[256] = 1
    counts[MATCH] = match.sum()
    return counts


def adler_parts(data):
    d, n = data.astype(np.uint64), len(data)
    return int(d.sum() % 65521), int((d * (n - np.arange(n, dtype=np.uint64))).sum() % 65521)


def canonical(lengths):
    """Canonical codes of RFC 1951 3.2.2, bit-reversed (deflate sends a Huffman code from its most significant bit)."""
    count = np.bincount(lengths, minlength=17)
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = []
    for l in lengths:
        if l:
            codes.append(int(format(nxt[l], '0%db' % l)[::-1], 2))
            nxt[l] += 1
        else:
            codes.append(0)
    return codes


def pack(values, counts):
    """Bit strings (value, count), least significant bit first, concatenated -> (bytes padded with zero bits, bit count)."""
    values, counts = np.asarray(values, np.uint64), np.asarray(counts, np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    total = int(offsets[-1])
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    for k in range(int(counts.max(initial=0))):
        sel = counts > k
        bits[offsets[:-1][sel] + k] = (values[sel] >> np.uint64(k)) & np.uint64(1)
    return np.packbits(bits, bitorder='little').tobytes(), total


def table(counts, code_lengths):
    """The segment's table as pasta_png_segment_tables lays it out, from the counts and the given length rule."""
    ll = [int(v) for v in code_lengths(counts, 15)]
    lc = canonical(ll)
    seq = ll + [1 if counts[MATCH] else 0]
    cl = [int(v) for v in code_lengths(np.bincount(seq, minlength=19).astype(np.uint32), 7)]
    cc = canonical(cl)
    hclen = max(max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1, 4)
    values = [0, 2, SYMS - 257, 0, hclen - 4] + [cl[s] for s in CL_ORDER[:hclen]] + [cc[s] for s in seq]
    widths = [1, 2, 5, 5, 4] + [3] * hclen + [cl[s] for s in seq]
    header, header_bits = pack(values, widths)
    out = np.zeros(TABLE_WORDS, np.uint32)
    out[:SYMS] = np.array(lc, np.uint32) | (np.array(ll, np.uint32) << 24)
    if counts[MATCH]:
        out[MATCH] = lc[MATCH] | (1 << ll[MATCH]) | ((ll[MATCH] + 3) << 24)
    out[SYMS] = header_bits
    words = np.frombuffer(header + b'\0' * (-len(header) % 4), '<u4')
    out[HEADER_AT:HEADER_AT + len(words)] = words
    return out


def segment(stream, start, n, last, tab):
    """The bytes of one segment: header, tokens, end of block, then the empty stored block."""
    full, match, rest = tiles(stream, start, n)
    header_bits = int(tab[SYMS])
    values = [int(w) for w in tab[HEADER_AT:HEADER_AT + (header_bits + 31) // 32]]
    widths = [32] * (header_bits // 32) + ([header_bits % 32] if header_bits % 32 else [])
    code, bits = (tab[:SYMS] & 0xffffff).astype(np.uint64), (tab[:SYMS] >> 24).astype(np.int64)
    v, w = np.zeros(full.shape, np.uint64), np.zeros(full.shape, np.int64)
    v[~match], w[~match] = code[full[~match]], bits[full[~match]]
    v[match, 0], w[match, 0] = code[MATCH], bits[MATCH]
    values = np.concatenate([np.array(values, np.uint64), v.reshape(-1), code[rest], code[[256]]])
    widths = np.concatenate([np.array(widths, np.int64), w.reshape(-1), bits[rest], bits[[256]]])
    body, total = pack(values, widths)
    body = bytearray(body)
    if total % 8 == 0:
        body.append(0)
    if last:
        body[total // 8] |= 1 << (total % 8)
    body += b'\0' * ((total + 3 + 7) // 8 - len(body))        # the three header bits may straddle a byte
    return bytes(body) + b'\x00\x00\xff\xff'


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def encode(img, code_lengths):
    """[H, W, 3] uint8 -> dict(filtered [H, 1 + 3 W], meta [S, 288] uint32 as pasta_png_filter writes it, tables [S, 354],
    sizes [S], idat: the zlib stream, file: the PNG)."""
    h, w, _ = img.shape
    f = filtered(img)
    stream, stride = f.reshape(-1), 1 + 3 * w
    segs = [(r * stride, min(ROWS, h - r) * stride) for r in range(0, h, ROWS)]
    meta = np.zeros([len(segs), META_WORDS], np.uint32)
    tabs = np.zeros([len(segs), TABLE_WORDS], np.uint32)
    parts, A, B = [b'\x78\x01'], 1, 0
    for i, (start, n) in enumerate(segs):
        meta[i, :SYMS] = histogram(stream, start, n)
        meta[i, SYMS:] = adler_parts(stream[start:start + n])
        tabs[i] = table(meta[i, :SYMS], code_lengths)
        parts.append(segment(stream, start, n, i == len(segs) - 1, tabs[i]))
        B = (B + n * A + int(meta[i, SYMS + 1])) % 65521
        A = (A + int(meta[i, SYMS])) % 65521
    sizes = np.array([len(p) for p in parts[1:]], np.int64)
    parts.append(struct.pack('>I', (B << 16) | A))
    idat = b''.join(parts)
    png = SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', idat) + chunk(b'IEND', b'')
    return dict(filtered=f, meta=meta, tables=tabs, sizes=sizes, idat=idat, file=png)


def chunks(png):
    """[(kind, data, stored crc)] of a PNG file's chunks."""
    assert png[:8] == SIGNATURE
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack('>I', png[at:at + 4])
        out.append((png[at + 4:at + 8], png[at + 8:at + 8 + n], struct.unpack('>I', png[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(png)
    return out


# ---- the fixtures of the size conditions ----

def photograph(h, w, seed):
    r = np.random.RandomState(seed)
    field = np.kron(r.randn(h // 8 + 2, w // 8 + 2, 3), np.ones((8, 8, 1)))[:h, :w]
    box = np.ones(9) / 9
    for axis in (0, 1):
        field = np.apply_along_axis(lambda v: np.convolve(v, box, 'same'), axis, field)
    return np.clip(128 + 60 * field + 3 * r.randn(h, w, 3), 0, 255).astype(np.uint8)


def panel(h, w, content_w, seed):
    """Three squares of side h in a row, white but for content_w columns of photograph in the middle of each (w = 3 h)."""
    out = np.full((h, w, 3), 255, np.uint8)
    left = (h - content_w) // 2
    for k in range(3):
        out[:, h * k + left:h * k + left + content_w] = photograph(h, content_w, seed + k)
    return out
