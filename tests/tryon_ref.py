"""numpy restatement of the try-on data set's per-sample preparation (reference training/dataset.py:515-568, 619-736, 929-993 and
training_loop_wo_flow_fullbody.py:425-456), written as literally as the reference, one sample at a time.  The kernels of
csrc/tryon_inputs.hip are held to it bit for bit (tests/test_tryon_batch_gpu.py).

Three primitives of the reference come from libraries that are not available here; they are restated from their published
algorithms (parity with the libraries UNPINNED):
  ``cv2.line(img, p, q, color, 2)``    -> ``thick_line``: every pixel centre within distance 1 of the segment;
  pycocotools ``rleFrPoly``             -> ``rle_fr_poly``: a line-by-line port of the C routine, decoded;
  ``cv2.resize(INTER_LINEAR)``, uint8   -> ``resize_linear_u8``: OpenCV's scalar fixed-point path."""
import math
import random

import numpy as np

KPTCOLORS = [[255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0], [85, 255, 0], [0, 255, 0], [0, 255, 85],
             [0, 255, 170], [0, 255, 255], [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255], [255, 0, 255],
             [255, 0, 170], [255, 0, 85], [255, 0, 0]]
LIMBSEQ = [[2, 3], [2, 6], [3, 4], [4, 5], [6, 7], [7, 8], [2, 9], [9, 10], [10, 11], [2, 12], [12, 13], [13, 14], [2, 1], [1, 15],
           [15, 17], [1, 16], [16, 18], [3, 17], [6, 18]]

# ---- the three restated primitives ----

def thick_line(img, p, q, color):
    """cv2.line(img, p, q, color, thickness=2) restated: pixels (x, y) within distance 1 of the segment p -> q (integer points)."""
    h, w = img.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    x0, y0 = p
    x1, y1 = q
    dx, dy = x1 - x0, y1 - y0
    ux, uy = xs - x0, ys - y0
    len2 = dx * dx + dy * dy
    t = ux * dx + uy * dy
    near0 = ux * ux + uy * uy <= 1
    near1 = (xs - x1) ** 2 + (ys - y1) ** 2 <= 1
    if len2 == 0:
        hit = near0
    else:
        hit = np.where(t <= 0, near0, np.where(t >= len2, near1, (ux * dy - uy * dx) ** 2 <= len2))
    img[hit] = color


def rle_fr_poly(xy, h, w):
    """pycocotools maskApi.c rleFrPoly + rleDecode: the 0 / 1 uint8 [h, w] mask of polygon xy = [x0, y0, x1, y1, ...]."""
    k = len(xy) // 2
    scale = 5.0
    x = [int(scale * xy[2 * j] + .5) for j in range(k)]
    y = [int(scale * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else None         # 0 / 0: one point whose u equals its neighbours' (never used)
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5) if s is not None else 0)
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / scale - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / scale - .5
            yd = 0 if yd < 0 else h if yd > h else yd
            a.append(int(xd) * h + int(math.ceil(yd)))
    a = np.sort(np.array(a, np.int64))
    flat = np.arange(h * w)
    on = (np.searchsorted(a, flat, side='right') % 2).astype(np.uint8)
    return on.reshape(w, h).T.copy()                   # column-major runs


def resize_linear_u8(src, dh, dw):
    """cv2.resize(src, (dw, dh), interpolation=INTER_LINEAR) for a uint8 [sh, sw] image (OpenCV's scalar fixed-point path)."""
    sh, sw = src.shape

    def taps(dsize, ssize, is_x):
        scale = ssize / dsize
        ofs, c0, c1 = [], [], []
        for d in range(dsize):
            f = np.float32((d + 0.5) * scale - 0.5)
            s = int(math.floor(f))
            f = np.float32(f - np.float32(s))
            if is_x:
                if s < 0:
                    f, s = np.float32(0), 0
                if s >= ssize - 1:
                    f, s = np.float32(0), ssize - 1
            ofs.append(s)
            c0.append(int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048))))
            c1.append(int(np.rint(f * np.float32(2048))))
        return np.array(ofs), np.array(c0, np.int64), np.array(c1, np.int64)

    xo, a0, a1 = taps(dw, sw, True)
    yo, b0, b1 = taps(dh, sh, False)
    s = src.astype(np.int64)
    hrow = s[:, np.clip(xo, 0, sw - 1)] * a0 + s[:, np.clip(xo + 1, 0, sw - 1)] * a1       # [sh, dw]
    out = (hrow[np.clip(yo, 0, sh - 1)] * b0[:, None] + hrow[np.clip(yo + 1, 0, sh - 1)] * b1[:, None] + (1 << 21)) >> 22
    return np.clip(out, 0, 255).astype(np.uint8)


def dilate(mask, k):
    """cv2.dilate(mask, np.ones((k, k))) by brute force: the maximum over offsets -(k // 2) .. k - 1 - k // 2, image border ignored."""
    h, w = mask.shape
    a = k // 2
    out = np.zeros_like(mask)
    pad = np.zeros([h + k, w + k], mask.dtype)
    pad[a:a + h, a:a + w] = mask
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, pad[dy:dy + h, dx:dx + w])
    return out

# ---- dataset.py, sample by sample ----

def draw_pose_from_cords(pose_joints, img_size=(256, 192)):
    """dataset.py:704-736 (no affine): limbs with the restated thick line, then skimage.draw.circle(int(y), int(x), 2) discs."""
    colors = np.zeros(img_size + (3,), dtype=np.uint8)
    for i, p in enumerate(LIMBSEQ):
        f, t = p[0] - 1, p[1] - 1
        if pose_joints[f][2] < 0.1 or pose_joints[t][2] < 0.1:
            continue
        pf = pose_joints[f][0], pose_joints[f][1]
        pt = pose_joints[t][0], pose_joints[t][1]
        fx, fy = int(pf[1]), int(pf[0])
        tx, ty = int(pt[1]), int(pt[0])
        thick_line(colors, (fy, fx), (ty, tx), KPTCOLORS[i])
    for i, joint in enumerate(pose_joints):
        if pose_joints[i][2] < 0.1:
            continue
        x, y = int(joint[1]), int(joint[0])
        rr, cc = np.mgrid[0:img_size[0], 0:img_size[1]]
        disc = ((rr - x) / 2) ** 2 + ((cc - y) / 2) ** 2 < 1          # skimage _ellipse_in_shape, rotation 0
        colors[disc] = KPTCOLORS[i]
    return colors


def get_rectangle_mask(a, b, c, d, img_h, img_w):
    x1, y1 = a + (b - d) / 4, b + (c - a) / 4
    x2, y2 = a - (b - d) / 4, b - (c - a) / 4
    x3, y3 = c + (b - d) / 4, d + (c - a) / 4
    x4, y4 = c - (b - d) / 4, d - (c - a) / 4
    kps = [x1, y1, x2, y2]
    v0_x, v0_y = c - a, d - b
    v1_x, v1_y = x3 - x1, y3 - y1
    v2_x, v2_y = x4 - x1, y4 - y1
    with np.errstate(divide='ignore', invalid='ignore'):
        cos1 = (v0_x * v1_x + v0_y * v1_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v1_x * v1_x + v1_y * v1_y))
        cos2 = (v0_x * v2_x + v0_y * v2_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v2_x * v2_x + v2_y * v2_y))
    kps.extend([x3, y3, x4, y4] if cos1 < cos2 else [x4, y4, x3, y3])
    return rle_fr_poly([float(v) for v in kps], img_h, img_w).astype(np.float32) * 255.0


def get_hand_mask(hand_keypoints):
    s_x, s_y, s_c = hand_keypoints[0]
    e_x, e_y, e_c = hand_keypoints[1]
    w_x, w_y, w_c = hand_keypoints[2]
    up_mask = np.ones((256, 256), dtype=np.float32)
    bottom_mask = np.ones((256, 256), dtype=np.float32)
    if s_c > 0.1 and e_c > 0.1:
        up_mask = (dilate(get_rectangle_mask(s_x, s_y, e_x, e_y, 256, 256), 25) > 0).astype(np.float32)
    if e_c > 0.1 and w_c > 0.1:
        bottom_mask = (dilate(get_rectangle_mask(e_x, e_y, w_x, w_y, 256, 256), 16) > 0).astype(np.float32)
    return up_mask, bottom_mask


def get_palm_mask(hand_mask, hand_up_mask, hand_bottom_mask):
    inter_up_mask = ((hand_mask + hand_up_mask) == 2).astype(np.float32)
    hand_mask = hand_mask - inter_up_mask
    inter_bottom_mask = ((hand_mask + hand_bottom_mask) == 2).astype(np.float32)
    return hand_mask - inter_bottom_mask


def get_palm(keypoints, parsing_padded, left_padding):
    """dataset.py:682-702; parsing_padded [256, 256]."""
    left = keypoints[[5, 6, 7], :].copy()
    right = keypoints[[2, 3, 4], :].copy()
    left[:, 0] += left_padding
    right[:, 0] += left_padding
    lu, lb = get_hand_mask(left)
    ru, rb = get_hand_mask(right)
    lpalm = get_palm_mask((parsing_padded == 14).astype(np.float32), lu, lb)
    rpalm = get_palm_mask((parsing_padded == 15).astype(np.float32), ru, rb)
    return ((lpalm + rpalm) > 0).astype(np.uint8)


def label_masks(image_unpadded, parsing_unpadded, keypoints):
    """_load_raw_image (:515-563) up to the call of normalize: (image, pose, retain_mask, gt_parsing, upper_img, lower_img,
    upper_mask_rgb, lower_mask_rgb, palm), HWC uint8 on the padded square."""
    h, w = image_unpadded.shape[:2]
    lp, rp = (h - w) // 2, h - w - (h - w) // 2
    image = np.pad(image_unpadded, ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(255, 255))
    pose = np.pad(draw_pose_from_cords(keypoints, (h, w)), ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    parsing = np.pad(parsing_unpadded[..., None], ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    shoes = (parsing == 18).astype(np.uint8) + (parsing == 19).astype(np.uint8)
    head = (parsing == 1).astype(np.uint8) + (parsing == 2).astype(np.uint8) + (parsing == 4).astype(np.uint8) + (parsing == 13).astype(np.uint8)
    palm = get_palm(keypoints, parsing[..., 0], lp)
    retain = shoes + palm[..., None] + head
    upper = (parsing == 5).astype(np.uint8) + (parsing == 6).astype(np.uint8) + (parsing == 7).astype(np.uint8)
    lower = (parsing == 9).astype(np.uint8) + (parsing == 12).astype(np.uint8)
    hands = (parsing == 14).astype(np.uint8) + (parsing == 15).astype(np.uint8)
    legs = (parsing == 16).astype(np.uint8) + (parsing == 17).astype(np.uint8)
    neck = (parsing == 10).astype(np.uint8)
    gt = upper * 1 + lower * 2 + hands * 3 + legs * 4 + neck * 5
    um = np.concatenate([upper, upper, upper], axis=2) * 255
    lm = np.concatenate([lower, lower, lower], axis=2) * 255
    return image, pose, retain[..., 0], gt[..., 0], upper * image, lower * image, um, lm, palm


def erase_mask(denorm_hand_masks, acgpn_channel0):
    """__getitem__ :951-969: the draws after random.seed(1), the += in uint8 (it wraps), then > 0.  -> uint8 [256, 256]."""
    m = np.zeros((256, 256, 1), dtype=np.uint8)
    random.seed(1)
    if random.random() < 0.4:
        for mask in denorm_hand_masks:
            if random.random() < 0.5:
                m += mask
    if random.random() < 0.9:
        m += resize_linear_u8(acgpn_channel0, 256, 256)[..., None]
    return (m > 0).astype(np.uint8)[..., 0]
