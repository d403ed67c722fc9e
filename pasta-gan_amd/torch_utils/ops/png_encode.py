"""PNG files of a batch of RGB8 images, encoded on the GPU (csrc/png_encode.hip; include/pasta_hip.h lists the stream's rules,
DESIGN 8g what it costs).

``encode(images)``: filter launch -> ONE copy back of the token counts and Adler parts -> the segments' tables and sizes on the
host (the host-only entry pasta_png_segment_tables) -> encode launch into a compact buffer -> ONE copy back of exactly the
compressed bytes -> chunk framing and CRC-32 (zlib) on the host.  There is no CPU path: a CPU tensor is refused."""

import ctypes
import os
import struct
import time
import zlib

import numpy as np
import torch

from . import _native

ROWS = 16                   # PASTA_PNG_ROWS
META_WORDS = 288            # PASTA_PNG_META_WORDS
TABLE_WORDS = 354           # PASTA_PNG_TABLE_WORDS
SYMS = 286                  # PASTA_PNG_SYMS
_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_IEND = struct.pack('>I', 0) + b'IEND' + struct.pack('>I', zlib.crc32(b'IEND'))


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def code_lengths(counts, limit):
    """The host-only entry: complete Huffman code lengths of ``counts``, none above ``limit`` bits.  Needs no GPU."""
    counts = np.ascontiguousarray(counts, np.uint32)
    lengths = np.zeros(len(counts), np.uint8)
    _native.check(_native.lib().pasta_png_code_lengths(_np_ptr(counts), len(counts), int(limit), _np_ptr(lengths)))
    return lengths


def segment_tables(meta):
    """meta [M, META_WORDS] uint32 (host) -> (tables [M, TABLE_WORDS] uint32, sizes [M] int64).  Needs no GPU."""
    meta = np.ascontiguousarray(meta, np.uint32).reshape(-1, META_WORDS)
    tables = np.empty([len(meta), TABLE_WORDS], np.uint32)
    sizes = np.empty([len(meta)], np.int64)
    _native.check(_native.lib().pasta_png_segment_tables(_np_ptr(meta), len(meta), _np_ptr(tables), _np_ptr(sizes)))
    return tables, sizes


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def filter_pass(images):
    """uint8 [N, H, W, 3] on the GPU -> (filtered [N, H, 1 + 3 W] uint8, meta [N, S, META_WORDS] int32 holding uint32 words)."""
    _native.require_gpu(images, 'png_encode')
    if images.dtype != torch.uint8 or images.ndim != 4:
        raise RuntimeError('png_encode: expected a uint8 [N, H, W, 3] tensor, got %s %s' % (images.dtype, list(images.shape)))
    images = images.contiguous()
    n, h, w, c = images.shape
    filtered = torch.empty([n, h, 1 + 3 * w], dtype=torch.uint8, device=images.device)
    meta = torch.empty([n, -(-h // ROWS), META_WORDS], dtype=torch.int32, device=images.device)
    with torch.cuda.device(images.device):
        _native.check(_native.lib().pasta_png_filter(_native.ptr(images), _native.ptr(filtered), _native.ptr(meta), n, h, w, c, _native.stream()))
    return filtered, meta


def encode(images, times=None):
    """uint8 [N, H, W, 3] on the GPU -> the N PNG files as ``bytes``.  ``times``: a dict that receives the seconds of every step
    (filter, copy_meta, tables, upload, encode, copy_out, frame, of which crc), each ended by a synchronise; None measures nothing."""
    clock = [time.perf_counter()]

    def lap(name, sync=True):
        if times is not None:
            if sync:
                torch.cuda.synchronize()
            now = time.perf_counter()
            times[name] = times.get(name, 0.0) + now - clock[0]
            clock[0] = now

    filtered, meta = filter_pass(images)
    n, h, stride = filtered.shape
    w, segs = (stride - 1) // 3, meta.shape[1]
    lap('filter')
    meta_host = meta.cpu().numpy().view(np.uint32)
    lap('copy_meta')
    tables, sizes = segment_tables(meta_host)
    # an image's segments follow one another; every image starts on a 4-byte boundary of the compact buffer
    sizes = sizes.reshape(n, segs)
    image_bytes = sizes.sum(axis=1)
    image_at = np.concatenate([[0], np.cumsum((image_bytes + 3) // 4 * 4)])
    offsets = image_at[:-1, None] + np.cumsum(sizes, axis=1) - sizes
    lap('tables', sync=False)
    tables_dev = torch.from_numpy(tables.view(np.int32)).to(images.device)
    offsets_dev = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(images.device)
    out = torch.zeros([int(image_at[-1])], dtype=torch.uint8, device=images.device)
    lap('upload')
    with torch.cuda.device(images.device):
        _native.check(_native.lib().pasta_png_encode(_native.ptr(filtered), _native.ptr(tables_dev), _native.ptr(offsets_dev), _native.ptr(out),
                                                     out.numel(), n, h, w, _native.stream()))
    lap('encode')
    packed = memoryview(out.cpu().numpy())
    lap('copy_out')
    ihdr = _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
    files, crc_seconds = [], 0.0
    for i in range(n):
        a, b = 1, 0
        for s in range(segs):
            length = min(ROWS, h - s * ROWS) * stride
            b = (b + length * a + int(meta_host[i, s, SYMS + 1])) % 65521
            a = (a + int(meta_host[i, s, SYMS])) % 65521
        body = packed[int(image_at[i]):int(image_at[i]) + int(image_bytes[i])]
        adler = struct.pack('>I', (b << 16) | a)
        start = time.perf_counter()
        crc = zlib.crc32(adler, zlib.crc32(body, zlib.crc32(b'IDAT\x78\x01')))
        crc_seconds += time.perf_counter() - start
        files.append(b''.join([_SIGNATURE, ihdr, struct.pack('>I', len(body) + 6), b'IDAT\x78\x01', body, adler, struct.pack('>I', crc), _IEND]))
    lap('frame', sync=False)
    if times is not None:
        times['crc'] = times.get('crc', 0.0) + crc_seconds
    return files


def save(images, paths):
    """Encode the batch and write file i to ``paths[i]``, creating directories on the way."""
    paths = list(paths)
    if len(paths) != images.shape[0]:
        raise RuntimeError('png_encode.save: %d images and %d paths' % (images.shape[0], len(paths)))
    for data, path in zip(encode(images), paths):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)
