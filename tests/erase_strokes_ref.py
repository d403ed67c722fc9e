"""The numpy statement of the erase strokes (include/pasta_hip.h, pasta_erase_strokes_u8): the draws, the segments and
the mask, written from the rule and from nothing of training/tryon_batch.py.  Everything the mask test multiplies is a Python
integer or an int64, so nothing here can overflow where the kernel's int32 might."""
import math

import numpy as np

DEFAULTS = dict(strokes=6, vertices=6, length=0.25, width=0.12, turn=60.0)
UNIFORMS = 169
SEGMENTS = 64


def uniforms(seed, position):
    """The 169 uniforms on [0, 1) of (seed, position), as Python floats."""
    raw = np.random.PCG64(np.random.SeedSequence((int(seed), int(position), 1))).random_raw(UNIFORMS)
    return [float(int(r) >> 11) * 2.0 ** -53 for r in raw]


def q3(v, low=-8192, top=8191):
    return int(min(max(float(np.rint(v * 8.0)), low), top))


def vertices(spec, seed, position, S):
    """The strokes of one item before quantisation: a list of (half-width r, [(x, y), ...]) with V + 1 points each, in float64."""
    spec = dict(DEFAULTS, **spec)
    u = uniforms(seed, position)
    out = []
    for j in range(1 + int(math.floor(u[0] * spec['strokes']))):
        b = 1 + 21 * j
        x, y = u[b + 1] * S - 0.5, u[b + 2] * S - 0.5
        r = spec['width'] * S * (1.0 / 3.0 + 2.0 / 3.0 * u[b + 3]) / 2.0
        a = 2.0 * math.pi * u[b + 4]
        points = [(x, y)]
        for i in range(1 + int(math.floor(u[b] * spec['vertices']))):
            a += math.radians(spec['turn']) * (2.0 * u[b + 5 + 2 * i] - 1.0)
            l = spec['length'] * S * (1.0 + u[b + 6 + 2 * i]) / 2.0
            x, y = x + l * math.cos(a), y + l * math.sin(a)
            points.append((x, y))
        out.append((r, points))
    return out


def segments(spec, seed, positions, S):
    """(segments int32 [N, 64, 5], counts int32 [N]) of the items at ``positions``."""
    positions = [int(t) for t in np.asarray(positions).reshape(-1)]
    seg = np.zeros([len(positions), SEGMENTS, 5], np.int32)
    counts = np.zeros([len(positions)], np.int32)
    for n, t in enumerate(positions):
        k = 0
        for r, points in vertices(spec, seed, t, S):
            for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
                seg[n, k] = q3(x0), q3(y0), q3(x1), q3(y1), q3(r, 8, 512)
                k += 1
        counts[n] = k
    return seg, counts


def hit(px, py, x0, y0, x1, y1, r):
    """The pixel test on Python integers: no width to overflow."""
    X, Y = 8 * int(px), 8 * int(py)
    x0, y0, x1, y1, r = int(x0), int(y0), int(x1), int(y1), int(r)
    dx, dy, vx, vy = x1 - x0, y1 - y0, X - x0, Y - y0
    t, L = vx * dx + vy * dy, dx * dx + dy * dy
    if t <= 0:
        return vx * vx + vy * vy <= r * r
    if t >= L:
        return (X - x1) ** 2 + (Y - y1) ** 2 <= r * r
    return (vx * dy - vy * dx) ** 2 <= r * r * L


def mask(seg, counts, S, whole_planes=False):
    """uint8 [N, S, S] of 0 / 1 from segments [N, 64, 5] and counts [N] (read as clamped to 0..64), in int64.  A segment is
    evaluated on the pixels of its bounding box grown by r >= 0, outside of which no point is within r of it; with
    ``whole_planes`` on every pixel of the square (the same bytes, slower)."""
    seg = np.asarray(seg, np.int64)
    out = np.zeros([len(seg), S, S], np.uint8)
    for n in range(len(seg)):
        for x0, y0, x1, y1, r in seg[n, :min(max(int(counts[n]), 0), SEGMENTS)].tolist():
            xa, xb, ya, yb = 0, S, 0, S
            if not whole_planes and r >= 0:
                xa, xb = max((min(x0, x1) - r) // 8, 0), min((max(x0, x1) + r) // 8 + 1, S)
                ya, yb = max((min(y0, y1) - r) // 8, 0), min((max(y0, y1) + r) // 8 + 1, S)
                if xa >= xb or ya >= yb:
                    continue
            X, Y = np.meshgrid(8 * np.arange(xa, xb, dtype=np.int64), 8 * np.arange(ya, yb, dtype=np.int64))
            dx, dy, vx, vy = x1 - x0, y1 - y0, X - x0, Y - y0
            t, L = vx * dx + vy * dy, dx * dx + dy * dy
            cap0 = vx * vx + vy * vy <= r * r
            cap1 = (X - x1) ** 2 + (Y - y1) ** 2 <= r * r
            side = (vx * dy - vy * dx) ** 2 <= r * r * L
            out[n, ya:yb, xa:xb] |= np.where(t <= 0, cap0, np.where(t >= L, cap1, side)).astype(np.uint8)
    return out


def item_mask(spec, seed, position, S):
    seg, counts = segments(spec, seed, [position], S)
    return mask(seg, counts, S)[0]
