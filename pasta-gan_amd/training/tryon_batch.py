"""A batch of the try-on data set prepared on the GPU: what the reference's ``UvitonDatasetFull._load_raw_image`` /
``__getitem__`` (training/dataset.py:515-568, 619-736, 929-993) and its training loop (training_loop_wo_flow_fullbody.py:425-456)
do per sample on the host, as a few launches per batch:

    pasta_pose_stickman_u8   stick figure, thickness 2 and radius 2   (csrc/tryon_inputs.hip)
    pasta_palm_mask_u8       palm part of the retain mask, boxes 25 and 16   (csrc/tryon_pairs.hip)
    pasta_tryon_masks_u8     retain mask, gt_parsing, garment images and masks   (csrc/tryon_inputs.hip)
    patch_pipeline.normalize_batch   the ten body-part warps    (csrc/patches.hip)
    pasta_tryon_assemble     erase mask and every float conversion, into the nine tensors of SyntheticFullBodyBatch.KEYS

and, before all of them, for a packed batch of a data set opened with ``fit`` (people of their own sizes; ``fit_batch``):

    pasta_fit_people_u8      photograph and label map of every person resampled and placed on the canvas

and then, for a batch of a data set opened with ``mirror_people`` that holds a flagged item (``mirror_batch``):

    pasta_tryon_mirror_u8    photograph, label map (left and right exchanged) and erase mask as a mirror shows them

and after that, for a batch the training loop has numbered for ``--jitter-people`` (``jitter_batch``):

    pasta_tryon_jitter_u8    photograph and label map after a similarity map per item, the photograph through a colour map

and after that, for a batch that carries ``raw['erase_strokes']`` (``--erase-masks strokes``; ``strokes_batch``):

    pasta_erase_strokes_u8   the erase masks of the batch, drawn: random thick polylines on the padded square, one mask per item

The host keeps the file decoding (training/dataset.py), the key-point geometry below and the 8 x 8 solves of the warps
(patch_pipeline.part_maps; a builder with geometry='gpu': one launch instead).

The steps every builder takes are stated here once, for this one and for training/tryon_pairs.py and training/tryon_regions.py:
``upload_person`` (upload, ``fit_batch`` for a packed batch, and checks), ``upload_images`` (a pair batch's tensors), ``upload_erase`` (the training sets' erase
masks), ``mirror_batch`` (the training sets' mirrored people), ``jitter_batch`` (their jittered people), ``strokes_batch`` (their drawn erase masks),
``device_tables`` (stick and palm tables), ``allocator``, ``output_tensors`` (the fp32 tensors of a KEYS list with their pointer array) and
``shift_keypoints``.
``builder_for`` picks the training builder of a data set: this one, or training/tryon_regions.py's at 512 x 320."""

import ctypes
import functools
import math

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline
from training.swap_outfits import SWAP_KEYS, attach as attach_swap

# dataset.py:43-52 (1-based joint pairs)
LIMBSEQ = ((2, 3), (2, 6), (3, 4), (4, 5), (6, 7), (7, 8), (2, 9), (9, 10), (10, 11), (2, 12), (12, 13), (13, 14), (2, 1), (1, 15),
           (15, 17), (1, 16), (16, 18), (3, 17), (6, 18))
ARMS = ((5, 6, 7), (2, 3, 4))       # left, right: shoulder, elbow, wrist (get_palm :683-684)
COORD_LIMIT = 4096                  # stick-figure coordinates are clamped to +-COORD_LIMIT (integer arithmetic in the kernel)
QUAD_LIMIT = 1e5                    # palm quadrilateral corners are clamped to +-QUAD_LIMIT
STICK_THICKNESS = 2                 # cv2.line(..., 2) of both 256 x 192 sets (dataset.py:724, :1307)
STICK_RADIUS = 2                    # circle(..., radius=2) (:734, :1318)
PALM_BOXES = (25, 16)               # get_hand_mask of the training set: upper arm 25 x 25, forearm 16 x 16 (:663, :668)
# A mirrored person (this project's own rule, include/pasta_hip.h: pasta_tryon_mirror_u8): the labels and the joints that change sides
MIRROR_LABELS = ((14, 15), (16, 17), (18, 19))          # arms, legs, shoes
MIRROR_JOINTS = ((2, 5), (3, 6), (4, 7), (8, 11), (9, 12), (10, 13), (14, 15), (16, 17))   # shoulders .. ankles, eyes, ears
# A jittered person (this project's own rule, include/pasta_hip.h: pasta_tryon_jitter_u8): the strengths of a specification with
# the top of their ranges (rotate in degrees, shift as a fraction of the canvas side), and the luma weights of the saturation
JITTER_RANGES = dict(scale=0.5, rotate=45.0, shift=0.25, colour=0.5)
JITTER_LUMA = (0.299, 0.587, 0.114)
# Erase strokes (this project's own rule, include/pasta_hip.h: pasta_erase_strokes_u8): the names of a specification with their
# type, range and default; the uniforms of an item (1 + 8 blocks of 21) and the segments the device takes per item
STROKES_RANGES = dict(strokes=(int, 1, 8, 6), vertices=(int, 1, 8, 6), length=(float, 0.01, 0.5, 0.25), width=(float, 0.01, 0.25, 0.12),
                      turn=(float, 0.0, 180.0, 60.0))
STROKES_UNIFORMS = 169
STROKES_SEGMENTS = 64
# People fitted to the canvas (this project's own rule, include/pasta_hip.h: pasta_fit_people_u8): the modes, the filters of the
# photograph (the label map always takes the box taps), and the words of an item's record in the plan
FIT_MODES = ('pad', 'crop')
FIT_FILTERS = ('bilinear', 'box')
FIT_RECORD = 16


def stick_tables(keypoints):
    """[N, 18, 3] key points (unpadded x, y, confidence) -> (limbs int32 [N, 19, 5] = x0, y0, x1, y1, drawn;
    joints int32 [N, 18, 3] = x, y, drawn) of draw_pose_from_cords (:704-736): int()-truncated, drawn when confidence >= 0.1."""
    kp = np.asarray(keypoints, np.float64)
    xy = np.clip(np.trunc(np.nan_to_num(kp[..., :2])), -COORD_LIMIT, COORD_LIMIT).astype(np.int32)
    seen = kp[..., 2] >= 0.1
    f = np.array([a - 1 for a, _ in LIMBSEQ])
    t = np.array([b - 1 for _, b in LIMBSEQ])
    limbs = np.concatenate([xy[:, f], xy[:, t], (seen[:, f] & seen[:, t])[..., None].astype(np.int32)], axis=2)
    joints = np.concatenate([xy, seen[..., None].astype(np.int32)], axis=2)
    return np.ascontiguousarray(limbs), np.ascontiguousarray(joints)


def rectangle_corners(a, b, c, d):
    """The polygon of get_rectangle_mask(a, b, c, d) (:626-650), float64 [4, 2], in its corner order."""
    a, b, c, d = (np.float64(v) for v in (a, b, c, d))
    x1, y1 = a + (b - d) / 4, b + (c - a) / 4
    x2, y2 = a - (b - d) / 4, b - (c - a) / 4
    x3, y3 = c + (b - d) / 4, d + (c - a) / 4
    x4, y4 = c - (b - d) / 4, d - (c - a) / 4
    v0_x, v0_y = c - a, d - b
    v1_x, v1_y = x3 - x1, y3 - y1
    v2_x, v2_y = x4 - x1, y4 - y1
    with np.errstate(divide='ignore', invalid='ignore'):
        cos1 = (v0_x * v1_x + v0_y * v1_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v1_x * v1_x + v1_y * v1_y))
        cos2 = (v0_x * v2_x + v0_y * v2_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v2_x * v2_x + v2_y * v2_y))
    tail = [x3, y3, x4, y4] if cos1 < cos2 else [x4, y4, x3, y3]
    return np.array([x1, y1, x2, y2] + tail, np.float64).reshape(4, 2)


def palm_quads(keypoints, left_padding):
    """(quads float64 [N, 4, 4, 2], present uint8 [N, 4]) for the left upper arm, left forearm, right upper arm, right forearm
    (get_hand_mask :652-672: key points shifted by the padding; a segment needs both confidences > 0.1)."""
    kp = np.asarray(keypoints, np.float64)
    n = kp.shape[0]
    quads, present = np.zeros([n, 4, 4, 2]), np.zeros([n, 4], np.uint8)
    for i in range(n):
        for side, (s, e, w) in enumerate(ARMS):
            arm = kp[i, [s, e, w]].copy()
            arm[:, 0] += left_padding
            for k, (p, q) in enumerate(((0, 1), (1, 2))):
                if arm[p, 2] > 0.1 and arm[q, 2] > 0.1:
                    quads[i, 2 * side + k] = rectangle_corners(arm[p, 0], arm[p, 1], arm[q, 0], arm[q, 1])
                    present[i, 2 * side + k] = 1
    return np.ascontiguousarray(np.clip(np.nan_to_num(quads), -QUAD_LIMIT, QUAD_LIMIT)), present


def fit_check(mode, filter):
    """(mode, filter) of a fit, checked: a ValueError names an unknown one."""
    if mode not in FIT_MODES:
        raise ValueError('fit=%r is none of %s' % (mode, ', '.join(FIT_MODES)))
    if filter not in FIT_FILTERS:
        raise ValueError('fit_filter=%r is none of %s' % (filter, ', '.join(FIT_FILTERS)))
    return mode, filter


def _rhu(a, b):
    return (2 * a + b) // (2 * b)


def fit_rectangle(h, w, H, W, mode):
    """The fitted rectangle (Hc, Wc, oy, ox) of an ``h x w`` item on the ``H x W`` canvas (include/pasta_hip.h: ``rectangle``), in
    integers.  No limit is checked here (``fit_limits``)."""
    h, w, H, W = int(h), int(w), int(H), int(W)
    tall = h * W >= w * H
    if mode not in FIT_MODES:
        raise ValueError('fit=%r is none of %s' % (mode, ', '.join(FIT_MODES)))
    if tall == (mode == 'pad'):
        Hc, Wc = H, _rhu(w * H, h)
    else:
        Hc, Wc = _rhu(h * W, w), W
    if mode == 'pad':
        return Hc, Wc, (H - Hc) // 2, (W - Wc) // 2
    return Hc, Wc, -((Hc - H) // 2), -((Wc - W) // 2)


def fit_limits(h, w, Hc, Wc):
    """None, or what is wrong with resampling ``h x w`` to ``Hc x Wc``: more than 8 source pixels per fitted one, or more than 4
    fitted ones per source pixel, along either axis (the tap footprints the kernels are built for)."""
    if Hc < 1 or Wc < 1:
        return 'fits to an empty %d x %d' % (Hc, Wc)
    if h > 8 * Hc or w > 8 * Wc:
        return '%d x %d is more than 8 times the fitted %d x %d' % (h, w, Hc, Wc)
    if Hc > 4 * h or Wc > 4 * w:
        return 'the fitted %d x %d is more than 4 times %d x %d' % (Hc, Wc, h, w)
    return None


@functools.lru_cache(maxsize=256)
def fit_taps(n_in, n_out, filter):
    """The fixed-point taps of one axis from length ``n_in`` to ``n_out`` (include/pasta_hip.h: ``taps``; PIL's 8-bit rule in
    float64): (xmin int32 [n_out], cnt int32 [n_out], k int32 [n_out, ksize]), k zero past cnt.  Equal lengths: the single tap
    2^22, which returns the source byte.  Cached per (n_in, n_out, filter); the arrays are read-only."""
    n_in, n_out = int(n_in), int(n_out)
    assert n_in >= 1 and n_out >= 1 and filter in FIT_FILTERS
    if n_in == n_out:
        out = np.arange(n_out, dtype=np.int32), np.ones([n_out], np.int32), np.full([n_out, 1], 1 << 22, np.int32)
    else:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = (0.5 if filter == 'box' else 1.0) * fs
        ss = 1.0 / fs
        ksize = int(math.ceil(support)) * 2 + 1
        center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)             # astype truncates, as C's (int)
        cnt = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
        x = np.arange(ksize, dtype=np.int64)
        t = (((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss
        if filter == 'box':
            wgt = np.where((t > -0.5) & (t <= 0.5), 1.0, 0.0)
        else:
            wgt = np.where(np.abs(t) < 1.0, 1.0 - np.abs(t), 0.0)
        wgt = np.where(x[None, :] < cnt[:, None], wgt, 0.0)
        ww = np.zeros([n_out], np.float64)
        for j in range(ksize):                                                       # summed in tap order
            ww = ww + wgt[:, j]
        wgt = np.where(ww[:, None] != 0.0, wgt / np.where(ww == 0.0, 1.0, ww)[:, None], wgt)
        k = (0.5 + wgt * float(1 << 22)).astype(np.int64)
        out = xmin.astype(np.int32), cnt.astype(np.int32), np.ascontiguousarray(k.astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def fit_keypoints(keypoints, hw, rectangles):
    """[N, 18, 3] key points of items of sizes ``hw`` [N, 2] -> a float64 copy on the canvas (include/pasta_hip.h: ``joints``): a
    joint with confidence >= 0.1 moves with the content, one below keeps its bits, an item already at its fitted size and offset
    0 keeps all of them."""
    kp = np.asarray(keypoints, np.float64).copy()
    assert kp.ndim == 3 and kp.shape[1:] == (18, 3) and len(hw) == len(rectangles) == kp.shape[0]
    for i, ((h, w), (Hc, Wc, oy, ox)) in enumerate(zip(np.asarray(hw).tolist(), rectangles)):
        if (h, w, 0, 0) == (Hc, Wc, oy, ox):
            continue
        sx, sy = Wc / w, Hc / h
        seen = kp[i, :, 2] >= 0.1
        x, y = kp[i, :, 0].copy(), kp[i, :, 1].copy()
        with np.errstate(all='ignore'):
            kp[i, :, 0] = np.where(seen, x * sx + ((0.5 * sx - 0.5) + ox), x)
            kp[i, :, 1] = np.where(seen, y * sy + ((0.5 * sy - 0.5) + oy), y)
    return kp


def fit_rectangles(hw, canvas, mode):
    """[(Hc, Wc, oy, ox)] of items of sizes ``hw`` [N, 2] on ``canvas`` (``fit_rectangle``), the rule's limits asserted: the data
    sets refuse such a file by name at load."""
    out = []
    for h, w in np.asarray(hw, np.int64).reshape(-1, 2).tolist():
        rect = fit_rectangle(h, w, canvas[0], canvas[1], mode)
        wrong = fit_limits(h, w, rect[0], rect[1])
        assert h >= 1 and w >= 1 and wrong is None, wrong
        out.append(rect)
    return out


def fit_plan(hw, offsets, rectangles, filter):
    """The one int32 array ``pasta_fit_people_u8`` reads for a packed batch (include/pasta_hip.h: ``plan``): a record of FIT_RECORD
    words per item, then every distinct tap table the batch uses, once.  ``rectangles``: (Hc, Wc, oy, ox) per item."""
    assert filter in FIT_FILTERS
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    n = len(hw)
    assert len(offsets) == len(rectangles) == n and (offsets >= 0).all()
    records = np.zeros([n, FIT_RECORD], np.int32)
    tables, where, words = [], {}, n * FIT_RECORD

    def table(n_in, n_out, f):
        nonlocal words
        key = (n_in, n_out, f if n_in != n_out else 'box')
        if key not in where:
            xmin, cnt, k = fit_taps(*key)
            flat = np.concatenate([np.array([n_out, k.shape[1]], np.int32),
                                   np.concatenate([xmin[:, None], cnt[:, None], k], axis=1).reshape(-1)])
            where[key] = words
            tables.append(flat)
            words += len(flat)
        return where[key]

    for i, ((h, w), (Hc, Wc, oy, ox)) in enumerate(zip(hw.tolist(), rectangles)):
        off = int(offsets[i])
        records[i, :12] = (h, w, Hc, Wc, oy, ox, table(w, Wc, filter), table(h, Hc, filter), table(w, Wc, 'box'), table(h, Hc, 'box'),
                           off & 0x7fffffff, off >> 31)
    return np.concatenate([records.reshape(-1)] + tables)


def fit_batch(raw, device, prefix=''):
    """The people of a PACKED batch (``training.dataset.collate`` / ``collate_outfits`` of samples that carry ``fit``) fitted to
    their canvas: (image uint8 [N, H, W, 3], parsing uint8 [N, H, W] on ``device``, key points float64 [N, 18, 3] on the host).
    Three uploads (the packed photographs, the packed label maps, the plan with its tap tables) and two launches for the batch
    (pasta_fit_people_u8), ``fit_keypoints`` on the host; before ``mirror_batch``, ``jitter_batch`` and ``strokes_batch``."""
    fit = raw['fit']
    H, W = (int(v) for v in fit['canvas'])
    hw = np.asarray(raw[prefix + 'image_hw'], np.int64)
    offsets = np.asarray(raw[prefix + 'image_offsets'], np.int64)
    n = len(hw)
    packed_image, packed_parsing = torch.as_tensor(raw[prefix + 'image']), torch.as_tensor(raw[prefix + 'parsing'])
    assert packed_image.dtype == torch.uint8 and packed_parsing.dtype == torch.uint8 and packed_image.ndim == 1 and packed_parsing.ndim == 1
    assert hw.shape == (n, 2) and offsets.shape == (n,) and n >= 1
    assert (offsets + hw[:, 0] * hw[:, 1] <= packed_parsing.numel()).all() and packed_image.numel() == 3 * packed_parsing.numel()
    mode, filter = fit_check(fit['mode'], fit['filter'])
    rectangles = fit_rectangles(hw, (H, W), mode)
    plan = fit_plan(hw, offsets, rectangles, filter)
    image_s, parsing_s = (t.to(device, non_blocking=True).contiguous() for t in (packed_image, packed_parsing))
    plan_d = torch.from_numpy(plan).to(device, non_blocking=True)
    _native.require_gpu(image_s, 'fit_batch')
    image = torch.empty([n, H, W, 3], dtype=torch.uint8, device=image_s.device)
    parsing = torch.empty([n, H, W], dtype=torch.uint8, device=image_s.device)
    P = _native.ptr
    with torch.cuda.device(image_s.device):
        _native.check(_native.lib().pasta_fit_people_u8(P(image_s), P(parsing_s), int(packed_parsing.numel()), P(plan_d), int(plan.size),
                                                        P(image), P(parsing), n, H, W, _native.stream()))
    return image, parsing, fit_keypoints(raw[prefix + 'keypoints'], hw, rectangles)


def fitted(raw, device, prefix=''):
    """``raw`` itself when its people are stacked; for a packed batch a copy with the fitted people in their place (``fit_batch``:
    ``image`` and ``parsing`` on ``device``, the key points moved) and without the packing's keys: what a caller takes that reads a
    batch's people itself (training/snapshot_grid.py)."""
    if 'fit' not in raw or prefix + 'image_hw' not in raw:
        return raw
    image, parsing, keypoints = fit_batch(raw, device, prefix)
    out = {k: v for k, v in raw.items() if k not in ('fit', prefix + 'image_hw', prefix + 'image_offsets')}
    out.update({prefix + 'image': image, prefix + 'parsing': parsing, prefix + 'keypoints': torch.from_numpy(keypoints)})
    return out


def upload_person(raw, device, who, prefix=''):
    """One person set of a collated batch (``prefix`` 'clothes_': the donors) -> (image uint8 [N, H, W, 3], parsing uint8 [N, H, W]
    on ``device``, key points float64 [N, 18, 3] on the host), checked.  A packed batch (people of their own sizes, ``fit``) is
    fitted to its canvas here (``fit_batch``), so every builder gets the shapes it always got."""
    if 'fit' in raw and prefix + 'image_hw' in raw:
        image, parsing, keypoints = fit_batch(raw, device, prefix)
        n, H, W, _ = image.shape
        assert H >= W and keypoints.shape == (n, 18, 3)
        return image, parsing, keypoints
    up = lambda t: torch.as_tensor(t).to(device, non_blocking=True).contiguous()
    image, parsing = up(raw[prefix + 'image']), up(raw[prefix + 'parsing'])
    keypoints = np.asarray(raw[prefix + 'keypoints'], np.float64)
    _native.require_gpu(image, who)
    assert image.dtype == torch.uint8 and parsing.dtype == torch.uint8
    n, H, W, _ = image.shape
    assert H >= W and tuple(parsing.shape) == (n, H, W) and keypoints.shape == (n, 18, 3)
    return image, parsing, keypoints


def upload_erase(raw, device, n):
    """The erase masks of a batch of ``training.dataset.collate`` -> (masks uint8 [N, h_max, w_max], their sizes int32 [N, 2]) on
    ``device``, checked: every size lies within the stacked tensor."""
    erase = torch.as_tensor(raw['erase_masks']).to(device, non_blocking=True).contiguous()
    erase_hw = torch.as_tensor(raw['erase_hw'], dtype=torch.int32).to(device, non_blocking=True).contiguous()
    hw = np.asarray(raw['erase_hw'])
    assert erase.dtype == torch.uint8 and erase.ndim == 3 and erase.shape[0] == n and hw.shape == (n, 2) and (hw >= 1).all()
    assert (hw[:, 0] <= erase.shape[1]).all() and (hw[:, 1] <= erase.shape[2]).all()
    return erase, erase_hw


def mirror_lut():
    """The label table of a mirrored person, uint8 [256]: the identity except MIRROR_LABELS exchanged."""
    lut = np.arange(256, dtype=np.uint8)
    for a, b in MIRROR_LABELS:
        lut[a], lut[b] = b, a
    return lut


def mirror_keypoints(keypoints, W, flags):
    """[N, 18, 3] key points of an UNPADDED canvas ``W`` wide -> a float64 copy in which every item with a non-zero flag is the
    mirrored person's: x' = (W - 1) - x for every joint whatever its confidence, y and confidence kept, the rows of MIRROR_JOINTS
    exchanged.  Items with flag 0 keep their bits."""
    kp = np.asarray(keypoints, np.float64).copy()
    flagged = np.asarray(flags).reshape(-1) != 0
    assert kp.ndim == 3 and kp.shape[1:] == (18, 3) and flagged.shape == (kp.shape[0],)
    rows = np.arange(18)
    for a, b in MIRROR_JOINTS:
        rows[a], rows[b] = b, a
    m = kp[flagged][:, rows]
    m[..., 0] = (W - 1) - m[..., 0]
    kp[flagged] = m
    return kp


def mirror_batch(raw, image, parsing, keypoints, erase, erase_hw):
    """What both training builders call straight after ``upload_person`` / ``upload_erase``: (image, parsing, keypoints, erase)
    with the items that ``raw['xflip']`` flags mirrored, in one launch for the batch (pasta_tryon_mirror_u8) and
    ``mirror_keypoints`` on the host.  A batch without ``xflip``, or with no flag set, comes back as it is and launches nothing."""
    if 'xflip' not in raw:
        return image, parsing, keypoints, erase
    flags = np.ascontiguousarray(np.asarray(raw['xflip']), dtype=np.uint8)
    n, H, W, _ = image.shape
    assert flags.shape == (n,) and (flags <= 1).all()
    if not flags.any():
        return image, parsing, keypoints, erase
    dev = image.device
    flip, lut = torch.from_numpy(flags).to(dev, non_blocking=True), torch.from_numpy(mirror_lut()).to(dev, non_blocking=True)
    image_m, parsing_m, erase_m = torch.empty_like(image), torch.empty_like(parsing), torch.empty_like(erase)
    P = _native.ptr
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_tryon_mirror_u8(P(image), P(parsing), P(erase), P(erase_hw), P(flip), P(lut), P(image_m), P(parsing_m),
                                                          P(erase_m), n, H, W, int(erase.shape[1]), int(erase.shape[2]), _native.stream()))
    return image_m, parsing_m, mirror_keypoints(keypoints, W, flags), erase_m


def jitter_spec(spec):
    """A jitter specification -> a dict of all four JITTER_RANGES names as floats (absent names are 0), checked: a ValueError
    names an unknown name, a value outside its range, or a specification without a positive value."""
    spec = dict(spec)
    for name in spec:
        if name not in JITTER_RANGES:
            raise ValueError(f'unknown name {name!r} (known: {", ".join(JITTER_RANGES)})')
    out = {}
    for name, top in JITTER_RANGES.items():
        value = float(spec.get(name, 0.0))
        if not 0.0 <= value <= top:          # a NaN fails too
            raise ValueError(f'{name}={spec[name]} is outside 0..{top:g}')
        out[name] = value
    if not any(v > 0 for v in out.values()):
        raise ValueError('no positive value: ' + ','.join(f'{k}={v:g}' for k, v in out.items()))
    return out


def jitter_uniforms(seed, position):
    """The seven uniforms on (-1, 1) of stream position ``position`` of the run seeded ``seed``: from the raw 64-bit outputs of
    ``np.random.PCG64(np.random.SeedSequence((seed, position)))``, whose stream numpy guarantees, as (raw >> 11) * 2^-52 - 1."""
    raw = np.random.PCG64(np.random.SeedSequence((int(seed), int(position)))).random_raw(7)
    return (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def jitter_parameters(spec, seed, positions, H, W):
    """(geometry float64 [N, 4] = s, theta in degrees, tx, ty in pixels; colour float64 [N, 3] = contrast k, saturation q,
    brightness beta) of the items at ``positions`` of the sampler's global stream.  A draw depends on (seed, position) alone, and
    all seven uniforms are drawn in this order whichever strengths are zero."""
    spec = jitter_spec(spec)
    positions = np.asarray(positions, np.int64).reshape(-1)
    geometry, colour = np.zeros([len(positions), 4]), np.zeros([len(positions), 3])
    for i, t in enumerate(positions.tolist()):
        u = [float(v) for v in jitter_uniforms(seed, t)]
        geometry[i] = (1.0 + spec['scale']) ** u[0], spec['rotate'] * u[1], spec['shift'] * W * u[2], spec['shift'] * H * u[3]
        colour[i] = (1.0 + spec['colour']) ** u[4], (1.0 + spec['colour']) ** u[5], 64.0 * spec['colour'] * u[6]
    return geometry, colour


def _jitter_rotation(theta):
    r = math.radians(theta)
    return math.cos(r), math.sin(r)


def jitter_affine_q16(geometry, H, W):
    """geometry float64 [N, 4] -> int64 [N, 6]: the INVERSE map (A, B, C, D, E, F) of include/pasta_hip.h in Q16."""
    geometry = np.asarray(geometry, np.float64).reshape(-1, 4)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    out = np.zeros([len(geometry), 6], np.int64)
    for i, (s, theta, tx, ty) in enumerate(geometry.tolist()):
        cos, sin = _jitter_rotation(theta)
        a, b, d, e = cos / s, sin / s, -sin / s, cos / s
        c = cx - (a * (cx + tx) + b * (cy + ty))
        f = cy - (d * (cx + tx) + e * (cy + ty))
        out[i] = [int(np.rint(v * 65536.0)) for v in (a, b, c, d, e, f)]
    return out


def jitter_colour_q8(colour):
    """colour float64 [N, 3] = k, q, beta -> int32 [N, 12]: M3 = k (q I + (1 - q) 1 L^T) and the offset 128 (1 - k) + beta as the
    rows (M[c][0..2], offset) of include/pasta_hip.h's matrix in Q8."""
    k, q, beta = (np.asarray(colour, np.float64).reshape(-1, 3)[:, i, None, None] for i in range(3))
    m3 = k * (q * np.eye(3) + (1.0 - q) * np.asarray(JITTER_LUMA)) * 256.0                       # [N, 3, 3], term by term as stated
    offset = np.broadcast_to((128.0 * (1.0 - k) + beta) * 256.0, [len(m3), 3, 1])
    return np.ascontiguousarray(np.rint(np.concatenate([m3, offset], axis=2)).astype(np.int32).reshape(-1, 12))


def jitter_keypoints(keypoints, geometry, H, W):
    """[N, 18, 3] key points of the UNPADDED ``H x W`` canvas -> a float64 copy in which every joint with confidence >= 0.1 has
    moved where the content moves (include/pasta_hip.h: ``joints``), its confidence kept; a joint below 0.1 keeps its bits."""
    kp = np.asarray(keypoints, np.float64).copy()
    geometry = np.asarray(geometry, np.float64).reshape(-1, 4)
    assert kp.ndim == 3 and kp.shape[1:] == (18, 3) and len(geometry) == kp.shape[0]
    cx, cy = (W - 1) / 2, (H - 1) / 2
    rotation = np.array([_jitter_rotation(theta) for theta in geometry[:, 1].tolist()]).reshape(-1, 2)
    s, cos, sin, tx, ty = (v[:, None] for v in (geometry[:, 0], rotation[:, 0], rotation[:, 1], geometry[:, 2], geometry[:, 3]))
    m00, m01, m10, m11 = s * cos, -(s * sin), s * sin, s * cos
    ox = (cx + tx) - (m00 * cx + m01 * cy)
    oy = (cy + ty) - (m10 * cx + m11 * cy)
    seen = kp[..., 2] >= 0.1
    x, y = kp[..., 0].copy(), kp[..., 1].copy()
    with np.errstate(all='ignore'):                  # the unseen joints' numbers may be anything; they are not used
        kp[..., 0] = np.where(seen, m00 * x + m01 * y + ox, x)
        kp[..., 1] = np.where(seen, m10 * x + m11 * y + oy, y)
    return kp


def jitter_batch(raw, image, parsing, keypoints):
    """What both training builders call straight after ``mirror_batch``: (image, parsing, keypoints) of the people as
    ``raw['jitter']`` (``spec``, ``seed``, int64 ``positions`` [N]; attached by the training loop's ``_data_batches``) jitters
    them, in one launch for the batch (pasta_tryon_jitter_u8) and ``jitter_keypoints`` on the host.  A batch without ``jitter``
    comes back as it is and launches nothing."""
    if 'jitter' not in raw:
        return image, parsing, keypoints
    jitter = raw['jitter']
    n, H, W, _ = image.shape
    positions = np.asarray(jitter['positions'], np.int64)
    assert positions.shape == (n,)
    geometry, colour = jitter_parameters(jitter['spec'], jitter['seed'], positions, H, W)
    dev = image.device
    affine = torch.from_numpy(jitter_affine_q16(geometry, H, W)).to(dev, non_blocking=True)
    matrix = torch.from_numpy(jitter_colour_q8(colour)).to(dev, non_blocking=True)
    image_j, parsing_j = torch.empty_like(image), torch.empty_like(parsing)
    P = _native.ptr
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_tryon_jitter_u8(P(image), P(parsing), P(affine), P(matrix), P(image_j), P(parsing_j), n, H, W,
                                                          _native.stream()))
    return image_j, parsing_j, jitter_keypoints(keypoints, geometry, H, W)


def strokes_spec(spec):
    """An erase-stroke specification -> a dict of all five STROKES_RANGES names (``strokes`` and ``vertices`` ints, the rest floats;
    absent names take their defaults), checked: a ValueError names an unknown name, a value that is not a whole number where one is
    asked for, or a value outside its range."""
    spec = dict(spec)
    for name in spec:
        if name not in STROKES_RANGES:
            raise ValueError(f'unknown name {name!r} (known: {", ".join(STROKES_RANGES)})')
    out = {}
    for name, (kind, low, top, default) in STROKES_RANGES.items():
        value = float(spec.get(name, default))
        if kind is int and not value.is_integer():              # a NaN fails here and below
            raise ValueError(f'{name}={spec[name]} is not a whole number')
        if not low <= value <= top:
            raise ValueError(f'{name}={spec[name]} is outside {low:g}..{top:g}')
        out[name] = kind(value)
    return out


def strokes_uniforms(seed, position):
    """The 169 uniforms on [0, 1) of stream position ``position`` of the run seeded ``seed``: from the raw 64-bit outputs of
    ``np.random.PCG64(np.random.SeedSequence((seed, position, 1)))`` as (raw >> 11) * 2^-53.  The third word keeps them
    independent of ``jitter_uniforms``' (seed, position)."""
    raw = np.random.PCG64(np.random.SeedSequence((int(seed), int(position), 1))).random_raw(STROKES_UNIFORMS)
    return (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _strokes_q3(v, low, top):
    return int(min(max(np.rint(v * 8.0), low), top))


def strokes_segments(spec, seed, positions, S):
    """(segments int32 [N, 64, 5] = (x0, y0, x1, y1, r) in 1/8 pixel, counts int32 [N]) of the items at ``positions`` of the
    sampler's global stream on the padded ``S x S`` square (include/pasta_hip.h: ``strokes`` and ``Q3``).  A draw depends on
    (seed, position) alone; rows past an item's count are 0."""
    spec = strokes_spec(spec)
    positions = np.asarray(positions, np.int64).reshape(-1)
    segments = np.zeros([len(positions), STROKES_SEGMENTS, 5], np.int32)
    counts = np.zeros([len(positions)], np.int32)
    turn = math.radians(spec['turn'])
    for n, t in enumerate(positions.tolist()):
        u = strokes_uniforms(seed, t).tolist()
        k = 0
        for j in range(1 + int(math.floor(u[0] * spec['strokes']))):
            b = 1 + 21 * j
            x, y = u[b + 1] * S - 0.5, u[b + 2] * S - 0.5
            r = _strokes_q3(spec['width'] * S * (1.0 / 3.0 + 2.0 / 3.0 * u[b + 3]) / 2.0, 8, 512)
            a = 2.0 * math.pi * u[b + 4]
            for i in range(1 + int(math.floor(u[b] * spec['vertices']))):
                a += turn * (2.0 * u[b + 5 + 2 * i] - 1.0)
                l = spec['length'] * S * (1.0 + u[b + 6 + 2 * i]) / 2.0
                x1, y1 = x + l * math.cos(a), y + l * math.sin(a)
                segments[n, k] = (_strokes_q3(x, -8192, 8191), _strokes_q3(y, -8192, 8191), _strokes_q3(x1, -8192, 8191),
                                  _strokes_q3(y1, -8192, 8191), r)
                x, y, k = x1, y1, k + 1
        counts[n] = k
    return segments, counts


def attach_strokes(raw, spec, seed, positions):
    """``raw`` with ``raw['erase_strokes']`` = (``spec``, ``seed``, int64 ``positions`` [N]): the one place that writes the key
    ``strokes_batch`` reads.  The training loop numbers its items by their position in the sampler's stream; the scores and the
    sample grid by the person (seed 0, ``raw_idx``)."""
    positions = np.asarray(positions, np.int64).reshape(-1)
    assert positions.shape == (int(raw['raw_idx'].shape[0]),)
    raw['erase_strokes'] = dict(spec=strokes_spec(spec), seed=int(seed), positions=positions)
    return raw


def strokes_batch(raw, erase, erase_hw, S):
    """What both training builders call straight after ``jitter_batch``: (erase, erase_hw) for the assemble entry.  With
    ``raw['erase_strokes']`` (``attach_strokes``) the masks are drawn on the padded ``S x S`` square in one launch for the batch
    (pasta_erase_strokes_u8): uint8 [N, S, S] of 0 / 1 with sizes (S, S), after mirroring and jittering and never mirrored.  A
    batch without the key comes back as it is and launches nothing."""
    if 'erase_strokes' not in raw:
        return erase, erase_hw
    strokes = raw['erase_strokes']
    n = int(erase.shape[0])
    positions = np.asarray(strokes['positions'], np.int64)
    assert positions.shape == (n,)
    segments, counts = strokes_segments(strokes['spec'], strokes['seed'], positions, S)
    assert segments.shape == (n, STROKES_SEGMENTS, 5) and ((counts >= 0) & (counts <= STROKES_SEGMENTS)).all()   # the entry clamps; say so here
    dev = erase.device
    segments_d = torch.from_numpy(segments).to(dev, non_blocking=True)
    counts_d = torch.from_numpy(counts).to(dev, non_blocking=True)
    mask = torch.empty([n, S, S], dtype=torch.uint8, device=dev)
    sizes = torch.full([n, 2], S, dtype=torch.int32, device=dev)
    P = _native.ptr
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_erase_strokes_u8(P(segments_d), P(counts_d), P(mask), n, S, _native.stream()))
    return mask, sizes


def upload_images(raw, device):
    """``raw`` with its photographs and label maps (every ``*image`` / ``*parsing`` tensor) on ``device``; key points, names and
    indices stay on the host.  The pair builders stack a batch of ``training.dataset.collate_pairs`` after this, on the device."""
    return {k: torch.as_tensor(v).to(device, non_blocking=True) if k.endswith(('image', 'parsing')) else v for k, v in raw.items()}


def device_tables(stick_keypoints, palm_keypoints, left_padding, device):
    """(limbs, joints, quads, present) on ``device``: stick_tables of the first (UNSHIFTED) key points, palm_quads of the second."""
    arrays = stick_tables(stick_keypoints) + palm_quads(palm_keypoints, left_padding)
    return tuple(torch.from_numpy(a).to(device, non_blocking=True) for a in arrays)


def allocator(dtype, device):
    return lambda *shape: torch.empty(shape, dtype=dtype, device=device)


# the ten outputs of pasta_tryon_outfit_assemble in its order; the test batches' KEYS are this list or a part of it
OUTFIT_OUTPUTS = ['image', 'clothes', 'retain', 'pose', 'style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask',
                  'denorm_lower_mask', 'clothes_lower']


def output_tensors(keys, n, H, style_shape, device, slots=None):
    """The fp32 tensors an assemble entry fills, in the order of ``keys``, and the array of their pointers: style_input
    [n, *style_shape]; on the padded square pose has 6 planes, the masks and gt_parsing 1, every other tensor 3.  ``slots``: the
    entry's own output order where ``keys`` is a part of it (OUTFIT_OUTPUTS); a slot the batch has no key for is a null pointer."""
    f32, planes = allocator(torch.float32, device), dict(pose=6, denorm_upper_mask=1, denorm_lower_mask=1, gt_parsing=1)
    t = {k: f32(n, *style_shape) if k == 'style_input' else f32(n, planes.get(k, 3), H, H) for k in keys}
    slots = keys if slots is None else slots
    assert set(keys) <= set(slots)
    return t, (ctypes.c_void_p * len(slots))(*[t[k].data_ptr() if k in t else None for k in slots])


def shift_keypoints(keypoints, left_padding):
    """float64, as the test sets' keypoints[:, 0] += left_padding before get_crop's float32 conversion."""
    return np.concatenate([keypoints[..., :1] + left_padding, keypoints[..., 1:]], axis=-1)


class FullBodyBatch:
    """The interface TrainingStep.run consumes (as SyntheticFullBodyBatch): ``tensors`` (the nine KEYS), ``batch``, ``split``.
    A batch built with ``swap`` also carries the six SWAP_KEYS of training/swap_outfits.py, which ``split`` passes along.
    ``stages`` holds the uint8 intermediates when the builder was asked to keep them; ``image`` is the photographs' uint8 batch
    [N, H, W, 3] as the builder uploaded it (the reconstruction metric scores against it), mirrored and jittered where the batch says so."""
    KEYS = ['real_img', 'style_input', 'retain', 'pose', 'denorm_upper_input', 'denorm_lower_input',
            'denorm_upper_mask', 'denorm_lower_mask', 'gt_parsing']

    def __init__(self, tensors, stages=None, image=None):
        self.tensors = tensors
        self.batch = int(tensors['real_img'].shape[0])
        self.stages = stages
        self.image = image

    def split(self, batch_gpu):
        parts = {k: v.split(batch_gpu) for k, v in self.tensors.items()}
        keys = self.KEYS + [k for k in SWAP_KEYS if k in parts]          # a batch built with ``swap`` carries six more
        return [{k: parts[k][i] for k in keys} for i in range(len(parts['real_img']))]


class FullBodyBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate`` -> FullBodyBatch on ``device``.  ``swap`` = dict(region=,
    group=) or dict(upper_src=, lower_src=): the batch also carries the swapped inputs of training/swap_outfits.py, made from this
    batch's stages; kept stages then include that module's two SWAP_STAGES.  ``geometry`` = 'host' or 'gpu': where the body parts'
    matrices are solved (patch_pipeline.part_maps: DESIGN 8n)."""

    # how the warp-back matrices of this builder's stages are formed (training/snapshot_grid.py forms them again per cell):
    # the parts also cut from the lower garment, part_matrices' x_pad and shin_fallback, and whether the key points are shifted
    # by the padding in float64 first
    lower_parts, x_pad, shin_fallback, shifted = (6, 7, 8, 9), 32, False, False

    def __init__(self, device, box_factor=2, geometry='host'):
        self.device = torch.device(device)
        self.box_factor = box_factor
        self.geometry = patch_pipeline.check_geometry(geometry)

    def build(self, raw, keep_stages=False, swap=None):
        dev = self.device
        image, parsing, keypoints = upload_person(raw, dev, 'FullBodyBatchBuilder')
        n, H, W, _ = image.shape
        erase, erase_hw = upload_erase(raw, dev, n)
        image, parsing, keypoints, erase = mirror_batch(raw, image, parsing, keypoints, erase, erase_hw)
        image, parsing, keypoints = jitter_batch(raw, image, parsing, keypoints)
        erase, erase_hw = strokes_batch(raw, erase, erase_hw, H)
        limbs, joints, quads, present = device_tables(keypoints, keypoints, (H - W) // 2, dev)
        u8 = allocator(torch.uint8, dev)
        stick, palm, retain_mask, gt = u8(n, H, H, 3), u8(n, H, H), u8(n, H, H), u8(n, H, H)
        garments = [u8(n, H, H, 3) for _ in range(4)]          # upper image, lower image, upper mask, lower mask
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            s = _native.stream()
            _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(stick), n, H, W, STICK_THICKNESS, STICK_RADIUS, s))
            _native.check(lib.pasta_palm_mask_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, *PALM_BOXES, s))
            _native.check(lib.pasta_tryon_masks_u8(P(image), P(parsing), P(palm), P(retain_mask), P(gt), *[P(g) for g in garments], n, H, W, s))
        norm_img, norm_lower, den_u, den_l, m_invs, hand_masks, norm_mask, norm_mask_lower, back, valid = patch_pipeline.normalize_batch(
            *garments, keypoints, self.box_factor, want_matrices=True, geometry=self.geometry)
        norm_img, norm_lower, den_u, den_l = (t.contiguous() for t in (norm_img, norm_lower, den_u, den_l))
        arm = hand_masks.reshape(n, 4, H, H).contiguous()
        ph, pw, cu, cl = norm_img.shape[1], norm_img.shape[2], norm_img.shape[3], norm_lower.shape[3]
        t, outs = output_tensors(FullBodyBatch.KEYS, n, H, (cu + cl, ph, pw), dev)
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_assemble(P(image), P(stick), P(retain_mask), P(gt), P(norm_img), P(norm_lower), P(den_u), P(den_l),
                                                   P(arm), P(erase), P(erase_hw), outs, n, H, W, ph, pw, cu, cl,
                                                   int(erase.shape[1]), int(erase.shape[2]), _native.stream()))
        stages = None
        if keep_stages or swap is not None:
            stages = dict(stick=stick, palm=palm, retain_mask=retain_mask, gt_parsing=gt, upper_img=garments[0], lower_img=garments[1],
                          upper_mask=garments[2], lower_mask=garments[3], norm_img=norm_img, norm_img_lower=norm_lower,
                          denorm_upper=den_u, denorm_lower=den_l, arm_masks=arm, M_invs=m_invs, norm_clothes_mask=norm_mask.contiguous(),
                          norm_clothes_mask_lower=norm_mask_lower.contiguous())
        if swap is not None:
            attach_swap(t, stages, back, valid, self, swap, keep_stages)
        return FullBodyBatch(t, stages if keep_stages else None, image)


def builder_for(training_set, device, geometry='host'):
    """The builder that prepares the batches of ``training_set``: by the data set's class."""
    from training import dataset
    if isinstance(training_set, dataset.UvitonDatasetFull_512):
        from training.tryon_regions import FullBodyRegionBatchBuilder
        return FullBodyRegionBatchBuilder(device, geometry=geometry)
    if isinstance(training_set, dataset.UvitonDatasetFull):
        return FullBodyBatchBuilder(device, geometry=geometry)
    raise TypeError('no training batch builder for %s' % type(training_set).__name__)
