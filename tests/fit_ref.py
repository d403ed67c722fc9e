"""TEST INFRASTRUCTURE ONLY: people fitted to the canvas in numpy (include/pasta_hip.h, pasta_fit_people_u8; this
project's own rule), written directly from the statement, one output position at a time, and sharing no code with
training/tryon_batch.py or csrc/fit_people.hip: the fitted rectangle, the tap tables, the two-pass resample (PIL's 8-bit rule),
the label map's weighted mode with its tie rule, and the joints."""
import math

import numpy as np

FILTERS = {'box': 0.5, 'bilinear': 1.0}


def rhu(a, b):
    return (2 * a + b) // (2 * b)


def rectangle(h, w, H, W, mode):
    """(Hc, Wc, oy, ox)."""
    tall = h * W >= w * H
    if mode == 'pad':
        Hc, Wc = (H, rhu(w * H, h)) if tall else (rhu(h * W, w), W)
        return Hc, Wc, (H - Hc) // 2, (W - Wc) // 2
    assert mode == 'crop'
    Hc, Wc = (rhu(h * W, w), W) if tall else (H, rhu(w * H, h))
    return Hc, Wc, -((Hc - H) // 2), -((Wc - W) // 2)


def refused(h, w, Hc, Wc):
    return h > 8 * Hc or w > 8 * Wc or Hc > 4 * h or Wc > 4 * w


def taps(n_in, n_out, filter):
    """Per output position (xmin, k int64 [cnt]); an axis of equal lengths is the single tap 2^22."""
    if n_in == n_out:
        return [(xx, np.array([1 << 22], np.int64)) for xx in range(n_out)]
    s0 = FILTERS[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = s0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - xmin
        wgt = []
        for x in range(cnt):
            t = ((x + xmin) - center + 0.5) * ss
            if filter == 'box':
                wgt.append(1.0 if -0.5 < t <= 0.5 else 0.0)
            else:
                wgt.append(1.0 - abs(t) if abs(t) < 1.0 else 0.0)
        ww = 0.0
        for v in wgt:
            ww += v
        if ww != 0.0:
            wgt = [v / ww for v in wgt]
        out.append((xmin, np.array([int(0.5 + v * 4194304.0) for v in wgt], np.int64)))
    return out


def _pass(src, table):
    """src uint8 [rows, n_in, ...] along axis 1 -> uint8 [rows, n_out, ...]."""
    out = np.zeros((src.shape[0], len(table)) + src.shape[2:], np.uint8)
    wide = src.astype(np.int64)
    for xx, (xmin, k) in enumerate(table):
        acc = np.tensordot(wide[:, xmin:xmin + len(k)], k, axes=([1], [0]))
        out[:, xx] = np.clip(((1 << 21) + acc) >> 22, 0, 255)
    return out


def resample(image, Hc, Wc, filter):
    """uint8 [h, w] or [h, w, 3] -> [Hc, Wc(, 3)]: the horizontal pass into uint8 first, then the vertical one; a pass of equal
    lengths is skipped."""
    h, w = image.shape[:2]
    out = image
    if w != Wc:
        out = _pass(out, taps(w, Wc, filter))
    if h != Hc:
        out = np.swapaxes(_pass(np.swapaxes(out, 0, 1), taps(h, Hc, filter)), 0, 1)
    return np.ascontiguousarray(out)


def label_mode(labels, Hc, Wc):
    """uint8 [h, w] -> (uint8 [Hc, Wc], the number of pixels whose greatest weight two or more labels share).  The weights are
    formed as float64 matrix products: every entry is a sum of products of integers that stays below 2^45, so it is exact."""
    h, w = labels.shape
    ky, kx = np.zeros([Hc, h]), np.zeros([Wc, w])
    for table, dense in ((taps(h, Hc, 'box'), ky), (taps(w, Wc, 'box'), kx)):
        for p, (xmin, k) in enumerate(table):
            dense[p, xmin:xmin + len(k)] = k
    present = [int(v) for v in np.unique(labels)]                       # ascending
    weight = np.stack([ky @ (labels == L).astype(np.float64) @ kx.T for L in present])       # [labels, Hc, Wc]
    assert weight.max() < 2.0 ** 50
    best = weight.max(axis=0)
    tied = weight == best[None]
    smallest = np.asarray(present, np.uint8)[np.argmax(tied, axis=0)]
    cy = ((2 * np.arange(Hc) + 1) * h) // (2 * Hc)
    cx = ((2 * np.arange(Wc) + 1) * w) // (2 * Wc)
    centre = labels[cy[:, None], cx[None, :]]
    centre_tied = np.take_along_axis(tied, np.searchsorted(present, centre)[None], axis=0)[0]
    return np.where(centre_tied, centre, smallest).astype(np.uint8), int((tied.sum(axis=0) > 1).sum())


def place(fitted, canvas, oy, ox, fill):
    """The fitted array at (oy, ox) of a canvas filled with ``fill``; what lies outside the canvas is cut."""
    H, W = canvas
    out = np.full((H, W) + fitted.shape[2:], fill, np.uint8)
    Hc, Wc = fitted.shape[:2]
    r0, r1, c0, c1 = max(oy, 0), min(oy + Hc, H), max(ox, 0), min(ox + Wc, W)
    out[r0:r1, c0:c1] = fitted[r0 - oy:r1 - oy, c0 - ox:c1 - ox]
    return out


def keypoints(kp, h, w, rect):
    Hc, Wc, oy, ox = rect
    kp = np.array(kp, np.float64)
    sx, sy = Wc / w, Hc / h
    for j in range(kp.shape[0]):
        if kp[j, 2] >= 0.1:
            kp[j, 0] = kp[j, 0] * sx + ((0.5 * sx - 0.5) + ox)
            kp[j, 1] = kp[j, 1] * sy + ((0.5 * sy - 0.5) + oy)
    return kp


def fit_person(image, parsing, kp, canvas, mode, filter):
    """(image [H, W, 3], parsing [H, W], key points [18, 3], tied label pixels) of one person on ``canvas``."""
    h, w = parsing.shape
    Hc, Wc, oy, ox = rect = rectangle(h, w, canvas[0], canvas[1], mode)
    assert not refused(h, w, Hc, Wc)
    lab, tied = label_mode(parsing, Hc, Wc)
    return (place(resample(image, Hc, Wc, filter), canvas, oy, ox, 255), place(lab, canvas, oy, ox, 0), keypoints(kp, h, w, rect), tied)


def voronoi_labels(h, w, seed, cells=12, top=20):
    """A seeded label map of ``cells`` Voronoi cells with labels below ``top``: large regions with slanted borders."""
    rng = np.random.default_rng(seed)
    sites = rng.uniform(0, 1, [cells, 2]) * (h, w)
    values = rng.integers(0, top, cells).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[None] - sites[:, 0, None, None]) ** 2 + (xx[None] - sites[:, 1, None, None]) ** 2
    return values[np.argmin(d, axis=0)]
