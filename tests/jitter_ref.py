"""A jittered person in numpy (include/pasta_hip.h, pasta_tryon_jitter_u8; this project's own rule), written directly
from the statement.  Nothing is imported from the package: the draws, the Q16 and Q8 integers, the resampling and the joints are
written out again here.

    canvas     the unpadded H x W image, centre (cx, cy) = ((W-1)/2, (H-1)/2); content at p moves to
               p' = c0 + s R(theta)(p - c0) + t, theta in degrees with y pointing down
    inverse    x = a x' + b y' + c, y = d x' + e y' + f in float64: a = e = cos/s, b = sin/s, d = -sin/s,
               c = cx - (a (cx + tx) + b (cy + ty)), f = cy - (d (cx + tx) + e (cy + ty)); int64 Q16 = rint(v * 65536)
    image      X = A x' + B y' + C (int64); Xq = (X + 1024) >> 11; ix = Xq >> 5, ax = Xq & 31 (y likewise); four clamped taps;
               v = (sum w tap + 512) >> 10, w = (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay
    colour     out_c = clamp((M[c][0] R + M[c][1] G + M[c][2] B + M[c][3] + 128) >> 8, 0, 255), M int32 [3][4] in Q8
    labels     parsing'[y', x'] = parsing[clamp((Y + 32768) >> 16), clamp((X + 32768) >> 16)]
    erase      not touched
    joints     confidence >= 0.1: (m00 x + m01 y + ox, m10 x + m11 y + oy), m00 = m11 = s cos, m01 = -(s sin), m10 = s sin,
               ox = (cx + tx) - (m00 cx + m01 cy), oy = (cy + ty) - (m10 cx + m11 cy); below 0.1 the three numbers are kept

The jittered sample is then prepared by the unchanged builders and restatements."""
import math

import numpy as np

LUMA = (0.299, 0.587, 0.114)
IDENTITY_AFFINE = (65536, 0, 0, 0, 65536, 0)
IDENTITY_COLOUR = (256, 0, 0, 0, 0, 256, 0, 0, 0, 0, 256, 0)
IDENTITY_GEOMETRY = (1.0, 0.0, 0.0, 0.0)        # s, theta, tx, ty
IDENTITY_TONE = (1.0, 1.0, 0.0)                 # contrast k, saturation q, brightness beta


def uniforms(seed, position):
    """Seven uniforms on (-1, 1) from PCG64 seeded with SeedSequence((seed, position)): the top 53 bits of each raw output."""
    raw = np.random.PCG64(np.random.SeedSequence([seed, position])).random_raw(7)
    return [int(r >> np.uint64(11)) / 2.0 ** 52 - 1.0 for r in raw]


def parameters(spec, seed, position, H, W):
    """(s, theta, tx, ty), (k, q, beta) of one stream position; ``spec`` holds scale, rotate, shift, colour (absent: 0)."""
    scale, rotate, shift, colour = (float(spec.get(k, 0.0)) for k in ('scale', 'rotate', 'shift', 'colour'))
    u = uniforms(seed, position)
    geometry = ((1.0 + scale) ** u[0], rotate * u[1], shift * W * u[2], shift * H * u[3])
    tone = ((1.0 + colour) ** u[4], (1.0 + colour) ** u[5], 64.0 * colour * u[6])
    return geometry, tone


def affine_q16(geometry, H, W):
    s, theta, tx, ty = geometry
    cx, cy = (W - 1) / 2, (H - 1) / 2
    cos, sin = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    a, b, d, e = cos / s, sin / s, -sin / s, cos / s
    c = cx - (a * (cx + tx) + b * (cy + ty))
    f = cy - (d * (cx + tx) + e * (cy + ty))
    return [int(np.rint(v * 65536.0)) for v in (a, b, c, d, e, f)]


def colour_q8(tone):
    k, q, beta = tone
    rows = []
    for c in range(3):
        rows += [int(np.rint(k * ((q if c == j else 0.0) + (1.0 - q) * LUMA[j]) * 256.0)) for j in range(3)]
        rows.append(int(np.rint((128.0 * (1.0 - k) + beta) * 256.0)))
    return rows


def resample(image, parsing, affine, colour):
    """One item: image uint8 [H, W, 3], parsing uint8 [H, W], the six Q16 and the twelve Q8 integers -> (image', parsing')."""
    H, W = parsing.shape
    A, B, C, D, E, F = (np.int64(v) for v in affine)
    M = np.asarray(colour, np.int64).reshape(3, 4)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    X, Y = A * xx + B * yy + C, D * xx + E * yy + F
    Xq, Yq = (X + 1024) >> 11, (Y + 1024) >> 11
    ix, ax, iy, ay = Xq >> 5, Xq & 31, Yq >> 5, Yq & 31
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    src = image.astype(np.int64)
    w = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    taps = [src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]]
    v = (sum(wk[..., None] * tk for wk, tk in zip(w, taps)) + 512) >> 10
    out = np.stack([np.clip((M[c, 0] * v[..., 0] + M[c, 1] * v[..., 1] + M[c, 2] * v[..., 2] + M[c, 3] + 128) >> 8, 0, 255)
                    for c in range(3)], axis=-1).astype(np.uint8)
    lx, ly = np.clip((X + 32768) >> 16, 0, W - 1), np.clip((Y + 32768) >> 16, 0, H - 1)
    return out, np.ascontiguousarray(parsing[ly, lx])


def resample_arrays(image, parsing, affine, colour):
    """The entry's statement on stacked arrays: image [N, H, W, 3], parsing [N, H, W], affine [N, 6], colour [N, 12]."""
    pairs = [resample(image[n], parsing[n], affine[n], colour[n]) for n in range(len(image))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def keypoints(kp, geometry, H, W):
    """float64 [18, 3] of one person on the unpadded canvas."""
    s, theta, tx, ty = geometry
    cx, cy = (W - 1) / 2, (H - 1) / 2
    cos, sin = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    m00, m01, m10, m11 = s * cos, -(s * sin), s * sin, s * cos
    ox = (cx + tx) - (m00 * cx + m01 * cy)
    oy = (cy + ty) - (m10 * cx + m11 * cy)
    out = np.asarray(kp, np.float64).copy()
    for j in range(out.shape[0]):
        x, y, conf = (float(v) for v in out[j])
        if conf >= 0.1:
            out[j, 0], out[j, 1] = m00 * x + m01 * y + ox, m10 * x + m11 * y + oy
    return out


def jitter_raw(sample, geometry, tone):
    """A raw sample of ``UvitonDatasetFull`` under the given parameters; every other key (``raw_idx``, ``erase_mask``) is kept:
    the result is an ordinary sample."""
    H, W = sample['parsing'].shape
    out = dict(sample)
    out['image'], out['parsing'] = resample(sample['image'], sample['parsing'], affine_q16(geometry, H, W), colour_q8(tone))
    out['keypoints'] = keypoints(sample['keypoints'], geometry, H, W)
    return out
